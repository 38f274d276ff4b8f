"""Times the multi-hit ray queries (include/terra_amd.h "Multi-hit ray queries") against the closest-hit and occlusion queries on the same rays, in one run.
    python tools/multi_hit_time.py [--width 1920 --height 1080] [--launches 20] [--warmup 3] [--out profiles/multi_hit/multi_hit_time.log]
Workloads: the pixel-centre camera rays of the Cornell box (brute force over 32 triangles) and of the hall (the fast tree's walk), in pixel order (coherent) and in
a fixed pseudo-random permutation (incoherent); on the hall also as many rays from around it -- origins uniform in (-12.5, -4, -12.5) .. (12.5, 12.5, 12.5), aimed
at uniform points inside the hall --, on which a list of 8 actually fills. Per workload: terra_amd_intersect_device and terra_amd_occluded_device (the yardsticks),
terra_amd_intersect_all_device at K = 1, 2, 4, 8 and terra_amd_count_hits_device, with the ratios to the closest-hit call (occlusion for the count) and the
hits-per-ray histogram. Every figure is the median of `launches` launches, each timed with a pair of HIP events after `warmup` untimed ones. Needs a GPU."""
import argparse, ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes
from tools.query_time import camera_rays, median_ms


def outer_rays(n, seed=82):
    r = np.random.default_rng(seed)
    lo, hi = np.array((-12.5, -4.0, -12.5)), np.array((12.5, 12.5, 12.5))
    ilo, ihi = np.array((-9.5, 0.3, -4.5)), np.array((9.5, 7.5, 4.5))
    o = (lo + (hi - lo) * r.uniform(0, 1, size=(n, 3))).astype(np.float32)
    d = ((ilo + (ihi - ilo) * r.uniform(0, 1, size=(n, 3))).astype(np.float32) - o).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, api.RAY_DTYPE)
    rays["origin"] = o; rays["direction"] = d; rays["tmax"] = np.inf
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/multi_hit/multi_hit_time.log")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/multi_hit_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    say(f"# tools/multi_hit_time.py {a.width}x{a.height}: median (min .. max) of {a.launches} launches after {a.warmup} warm-up launches, HIP events; {torch.cuda.get_device_name(0)}")
    upload = lambda r: torch.from_numpy(r.view(np.float32).reshape(-1, 8).copy()).cuda()
    for name, d in (("cornell", scenes.cornell_box(a.width, a.height, 1)), ("hall", scenes.sponza_hall(a.width, a.height, 1))):
        scene = scenes.build_scene(L, d, counters=False)
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(scene, C.byref(ti)))
        rays = camera_rays(d); n = len(rays)
        perm = np.random.RandomState(1234).permutation(n)
        sets = {"camera, coherent": upload(rays), "camera, incoherent": upload(rays[perm])}
        if name == "hall":
            sets["from around the hall"] = upload(outer_rays(n))
        say(f"{name:8s} {sum(len(ob.triangles) for ob in d.objects)} triangles, {n} rays per set, multi-hit kernel: {'fast-tree walk' if ti.fast_tree else 'brute force'}   [{ti.note.decode()}]")
        for what, t in sets.items():
            total = runtime.count_hits(L, scene, t).cpu().numpy()
            hist = np.bincount(total)
            say(f"{name:8s} {what}: hits per ray {hist.tolist()}  (mean {total.mean():.2f}, {100 * (total > 8).mean():.1f} % above 8)")
            base = median_ms(torch, lambda: runtime.intersect(L, scene, t), a.launches, a.warmup)
            occ = median_ms(torch, lambda: runtime.occluded(L, scene, t), a.launches, a.warmup)
            row = lambda label, m, ref, against: say(f"{name:8s} {what:22s} {label:28s} {m[0]:9.3f} ms ({m[1]:.3f} .. {m[2]:.3f})  {n / m[0] / 1e3:9.1f} Mrays/s" + (f"  {m[0] / ref[0]:6.2f} x {against}" if ref else ""))
            row("intersect (yardstick)", base, None, "")
            row("occluded (yardstick)", occ, None, "")
            for k in (1, 2, 4, 8):
                row(f"intersect_all K = {k}", median_ms(torch, lambda: runtime.intersect_all(L, scene, t, k), a.launches, a.warmup), base, "intersect")
            cnt = median_ms(torch, lambda: runtime.count_hits(L, scene, t), a.launches, a.warmup)
            row("count_hits", cnt, occ, "occluded")
            say(f"{name:8s} {what:22s} {'count_hits':28s} {'':44s} {cnt[0] / base[0]:6.2f} x intersect")
        L.scene_destroy(scene)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
