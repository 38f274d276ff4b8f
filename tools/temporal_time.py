"""Times terra_amd_reproject_device on Cornell 1920 x 1080 buffers: history full, the camera moved sideways by a few pixels (HIP events, median of --repeats
launches after a warm-up), and sets the bytes the kernel must move -- per pixel 16 (result) + 2 x 16 (the AOV words read) + 48 (each history entry, read once
however many taps share it) read, 48 + 16 + 32 written -- against the 6.3 TB/s a float4 copy reaches on this part.
    python tools/temporal_time.py [--repeats 20] [--step 0.01] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_ACHIEVABLE_GBS = 6300.0


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
    ap.add_argument("--repeats", type=int, default=20); ap.add_argument("--step", type=float, default=0.01); ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = runtime.load()
    W, H = 1920, 1080
    d = scenes.cornell_box(W, H, 1, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d, counters=False)
    cam0 = scenes.camera_of(d)
    cam1 = scenes.camera_of(d); cam1.position.x += a.step          # 0.01 of a room 2 wide and 4.4 away: about 4 pixels at 1920
    fb = runtime.DeviceFramebuffer(W, H); aov = runtime.DeviceAov(W, H)
    h0, h1 = runtime.DeviceHistory(W, H), runtime.DeviceHistory(W, H)
    ofb = runtime.DeviceFramebuffer(W, H); om = runtime.DeviceMoments(W, H)
    runtime.render_device(L, cam0, s, fb); runtime.render_aov_device(L, cam0, s, aov)
    runtime.reproject_device(L, s, cam0, cam0, fb, aov, None, h0)
    fb.clear(); aov.clear()
    runtime.render_device(L, cam1, s, fb); runtime.render_aov_device(L, cam1, s, aov)
    torch.cuda.synchronize()
    lines = []
    n = W * H
    for name, fn, rd, wr in (
            ("first frame (no history), history only", lambda: runtime.reproject_device(L, s, cam1, cam0, fb, aov, None, h1), 16 + 32, 48),
            ("moved camera, history only", lambda: runtime.reproject_device(L, s, cam1, cam0, fb, aov, h0, h1), 16 + 32 + 48, 48),
            ("moved camera, all outputs", lambda: runtime.reproject_device(L, s, cam1, cam0, fb, aov, h0, h1, ofb, om), 16 + 32 + 48, 48 + 16 + 32),
            ("same camera (snapped taps), all outputs", lambda: runtime.reproject_device(L, s, cam0, cam0, fb, aov, h0, h1, ofb, om), 16 + 32 + 48, 48 + 16 + 32)):
        med, best = timed(fn, a.repeats)
        gbs = n * (rd + wr) / (med * 1e-3) / 1e9
        lines.append(f"1080p reproject, {name}: median {med:.4f} ms (best {best:.4f}) over {a.repeats} launches; {rd} B read + {wr} B written per pixel = {n * (rd + wr) / 1e6:.1f} MB "
                     f"-> {gbs:.0f} GB/s, {100 * gbs / HBM_ACHIEVABLE_GBS:.0f} % of {HBM_ACHIEVABLE_GBS:.0f} GB/s achievable")
    runtime.reproject_device(L, s, cam1, cam0, fb, aov, h0, h1); torch.cuda.synchronize()
    hist = h1.host()
    lines.append(f"after the moved frame: {100 * float((hist['length'] >= 2).mean()):.1f} % of the pixels took history, {100 * float((hist['length'] == 1).mean()):.1f} % restarted")
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    L.scene_destroy(s)


if __name__ == "__main__":
    main()
