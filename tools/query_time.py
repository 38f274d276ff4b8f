"""Times the batched ray queries (include/terra_amd.h "Ray queries") against the first-hit AOV pass of the same scene and frame, in one run.
    python tools/query_time.py [--width 1920 --height 1080] [--launches 20] [--warmup 3] [--out profiles/query_measurements/query_time.log]
Workloads: the pixel-centre camera rays of the Cornell box and of the hall, in pixel order (coherent) and in a fixed pseudo-random permutation (incoherent), through
terra_amd_intersect_device and terra_amd_occluded_device with no limit; on the hall also occlusion with tmax = half of each ray's own hit distance (nothing is
occluded: the limit's culling is all that helps). Yardstick: terra_amd_render_aov_device at 1 spp, which does strictly more per ray. Every figure is the median of
`launches` launches, each timed with a pair of HIP events after `warmup` untimed ones. Bytes per ray are the ray read and the answer written (32 + 32, 32 + 4);
the scene's nodes and triangles come on top. Needs a GPU: there is no CPU path."""
import argparse, ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes


def camera_rays(d):
    """origin and pixel-centre direction per pixel, row-major (the render's camera_sample at r1 = r2 = 0.5 without jitter, up to rounding)"""
    f = np.float32
    z = np.asarray(d.camera_direction, f); z /= np.linalg.norm(z)
    x = np.cross(np.asarray(d.camera_up, f), z).astype(f); x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(f)
    t = f(np.tan(np.float64(f(d.camera_fov) * f(0.0174533)) / 2)); aspect = f(d.width) / f(d.height)
    px, py = np.meshgrid(np.arange(d.width, dtype=f), np.arange(d.height, dtype=f))
    sx = f(2) * ((px + f(0.5)) / f(d.width)) - f(1); sy = f(1) - f(2) * ((py + f(0.5)) / f(d.height))
    e = np.stack([sx * aspect * t, sy * t, np.ones_like(sx)], axis=-1).reshape(-1, 3)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    dirs = (e[:, :1] * x + e[:, 1:2] * y + e[:, 2:] * z).astype(f)
    rays = np.zeros(len(dirs), api.RAY_DTYPE)
    rays["origin"] = np.asarray(d.camera_position, f); rays["direction"] = dirs; rays["tmax"] = np.inf
    return rays


def median_ms(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/query_measurements/query_time.log")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/query_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# tools/query_time.py {a.width}x{a.height}: median (min .. max) of {a.launches} launches after {a.warmup} warm-up launches, HIP events; {torch.cuda.get_device_name(0)}")
    for name, d in (("cornell", scenes.cornell_box(a.width, a.height, 1)), ("hall", scenes.sponza_hall(a.width, a.height, 1))):
        scene = scenes.build_scene(L, d, counters=False)
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(scene, C.byref(ti)))
        cam = scenes.camera_of(d)
        rays = camera_rays(d); n = len(rays)
        perm = np.random.RandomState(1234).permutation(n)
        aov = runtime.DeviceAov(d.width, d.height)
        med, lo, hi = median_ms(torch, lambda: runtime.render_aov_device(L, cam, scene, aov), a.launches, a.warmup)
        say(f"{name:8s} {'AOV pass, 1 spp (yardstick)':44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {n / med / 1e3:9.1f} Mrays/s  48 B read-modify-write per ray   [{ti.note.decode()}]")
        upload = lambda r: torch.from_numpy(r.view(np.float32).reshape(-1, 8).copy()).cuda()
        sets = {"coherent": upload(rays), "incoherent": upload(rays[perm])}
        hits = runtime.intersect(L, scene, sets["coherent"]).cpu().numpy().view(api.HIT_DTYPE).reshape(-1)
        say(f"{name:8s} {(hits['object'] >= 0).mean() * 100:.1f} % of the camera rays hit")
        for order, t in sets.items():
            for what, fn, nbytes in (("intersect", runtime.intersect, 64), ("occluded", runtime.occluded, 36)):
                med, lo, hi = median_ms(torch, lambda: fn(L, scene, t), a.launches, a.warmup)
                say(f"{name:8s} {what + ', ' + order + ', no limit':44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {n / med / 1e3:9.1f} Mrays/s  {nbytes} B per ray")
        if name == "hall":
            half = rays.copy(); half["tmax"] = np.where(hits["object"] >= 0, np.float32(0.5) * hits["t"], np.float32(np.inf))
            for order, r in (("coherent", half), ("incoherent", half[perm])):
                t = upload(r)
                assert int(runtime.occluded(L, scene, t).sum()) == 0
                med, lo, hi = median_ms(torch, lambda: runtime.occluded(L, scene, t), a.launches, a.warmup)
                say(f"{name:8s} {'occluded, ' + order + ', tmax = half the hit':44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {n / med / 1e3:9.1f} Mrays/s  36 B per ray   (nothing occluded)")
        L.scene_destroy(scene)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
