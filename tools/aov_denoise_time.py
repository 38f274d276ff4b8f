"""Times the first-hit AOV pass against the render call it mirrors, and the denoiser, at 1920 x 1080 (HIP events, warm-up, several repeats):
  * Cornell 512 spp and the hall 256 spp: one terra_amd_render_device call and one terra_amd_render_aov_device call of the whole frame;
  * the denoiser at K = 5 (and per iteration: K = 0 .. 8) on the Cornell frame's buffers.
    python tools/aov_denoise_time.py [--repeats 5] [--quick]   (--quick: 64 spp, for a first look)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats):
    import torch
    fn(); torch.cuda.synchronize()                     # warm-up
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    import torch  # before the library (terra_amd/runtime.py)
    from terra_amd import api, runtime, scenes
    ap = argparse.ArgumentParser(); ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    L = runtime.load()
    for name, make, spp in (("cornell", scenes.cornell_box, 512), ("hall", scenes.sponza_hall, 256)):
        spp = 64 if a.quick else spp
        d = make(1920, 1080, spp, integrator=api.kTerraIntegratorSimple)
        s = scenes.build_scene(L, d, counters=False)
        runtime.check(L.set_sample_split(s, 0))
        cam = scenes.camera_of(d)
        fb = runtime.DeviceFramebuffer(1920, 1080); aov = runtime.DeviceAov(1920, 1080)
        r_med, r_min = timed(lambda: runtime.render_device(L, cam, s, fb), a.repeats)
        a_med, a_min = timed(lambda: runtime.render_aov_device(L, cam, s, aov), a.repeats)
        print(f"{name} 1080p {spp} spp: render {r_med:.2f} ms (min {r_min:.2f}), AOV pass {a_med:.2f} ms (min {a_min:.2f}): {a_med / r_med:.3f} of the render", flush=True)
        if name == "cornell":
            rad = torch.zeros(1920 * 1080 * 3, dtype=torch.float32, device="cuda"); pix = torch.zeros_like(rad)
            prev = None
            for k in range(9):
                t, tmin = timed(lambda: runtime.denoise_device(L, s, fb, aov, k, radiance=rad, pixels=pix), a.repeats)
                step = f", +{t - prev:.3f} ms for iteration {k}" if prev is not None else ""
                print(f"denoise 1080p K={k}: {t:.3f} ms (min {tmin:.3f}){step}", flush=True)
                prev = t
        L.scene_destroy(s)


if __name__ == "__main__":
    main()
