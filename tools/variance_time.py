"""Times the moments accumulate, the tile error and the variance-guided denoiser (K = 5) beside terra_amd_denoise_device (K = 5) on the same Cornell
1920 x 1080 buffers (HIP events, median of 5 after a warm-up), then adaptive tiles against a uniform run taken to the same largest tile error: samples and
milliseconds of both.
    python tools/variance_time.py [--repeats 5] [--spp 4] [--batches 8] [--target 0.5] [--max-batches 64]"""
import argparse
import os
import sys
import time

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--spp", type=int, default=4); ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--target", type=float, default=0.5); ap.add_argument("--max-batches", type=int, default=64)
    a = ap.parse_args()
    L = runtime.load()
    W, H = 1920, 1080
    d = scenes.cornell_box(W, H, a.spp, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d, counters=False)
    cam = scenes.camera_of(d)
    fb = runtime.DeviceFramebuffer(W, H); aov = runtime.DeviceAov(W, H); dm = runtime.DeviceMoments(W, H)
    for _ in range(a.batches):
        runtime.render_device(L, cam, s, fb); runtime.render_aov_device(L, cam, s, aov); runtime.accumulate_moments_device(L, s, fb, dm)
    torch.cuda.synchronize()
    rad = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    # an accumulate with nothing new reads both buffers and stores nothing. The timed one alternates between two framebuffers of different sample counts, so that
    # every call rewrites every entry: fb -> fb2 is a batch of dn > 0, fb2 -> fb a cleared framebuffer (dn < 0: the entry starts over with one batch)
    t_idle, _ = timed(lambda: runtime.accumulate_moments_device(L, s, fb, dm), a.repeats)
    fb2 = runtime.DeviceFramebuffer(W, H)
    for _ in range(2 * a.batches):
        runtime.render_device(L, cam, s, fb2)
    dm2 = runtime.DeviceMoments(W, H); dm2.data.copy_(dm.data); torch.cuda.synchronize()
    turn = [0]
    def acc_once():
        turn[0] ^= 1
        runtime.accumulate_moments_device(L, s, fb2 if turn[0] else fb, dm2)
    t_acc, _ = timed(acc_once, 2 * a.repeats)
    t_err, _ = timed(lambda: runtime.tile_error_device(L, fb, dm, tile=128), a.repeats)
    t_old, _ = timed(lambda: runtime.denoise_device(L, s, fb, aov, 5, radiance=rad), a.repeats)
    t_new, _ = timed(lambda: runtime.denoise_variance_device(L, s, fb, aov, dm, 5, radiance=rad), a.repeats)
    print(f"1080p: accumulate {t_acc:.3f} ms with every entry rewritten ({t_idle:.3f} ms with nothing new), tile error (128) {t_err:.3f} ms", flush=True)
    print(f"1080p K=5: a-trous {t_old:.3f} ms, variance-guided {t_new:.3f} ms, ratio {t_new / t_old:.2f}", flush=True)
    # adaptive against uniform at the same largest tile error
    fb.clear(); aov.clear(); dm.clear(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = runtime.render_adaptive_device(L, cam, s, fb, dm, None, tile=128, min_batches=4, max_batches=a.max_batches, target_error=a.target)
    t_ad = (time.perf_counter() - t0) * 1e3
    left = max(rep["max_error"], 0.0)
    print(f"adaptive (tile 128, target {a.target}): {rep}, {t_ad:.1f} ms", flush=True)
    fb.clear(); dm.clear(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while n < a.max_batches:
        runtime.render_device(L, cam, s, fb); runtime.accumulate_moments_device(L, s, fb, dm); n += 1
        if n >= 2 and float(runtime.tile_error_device(L, fb, dm, tile=128).max()) <= max(left, a.target):
            break
    torch.cuda.synchronize()
    t_un = (time.perf_counter() - t0) * 1e3
    e = float(runtime.tile_error_device(L, fb, dm, tile=128).max())
    print(f"uniform to the same largest tile error: {n} batches, {n * W * H * a.spp} samples, largest error {e:.4f}, {t_un:.1f} ms; adaptive took {rep['samples']} samples", flush=True)
    L.scene_destroy(s)


if __name__ == "__main__":
    main()
