"""Times the nearest-surface queries (include/terra_amd.h "Nearest-surface queries") against closest-hit ray queries of as many rays, in one run.
    python tools/nearest_time.py [--side 128] [--brute 65536] [--launches 20] [--warmup 3] [--out profiles/nearest/nearest_time.log]
Points: side^3 (2 M) points, one uniformly placed in each cell of a side x side x side grid over the scene's bounding box -- in grid order (neighbouring lanes ask
about neighbouring points) and again in a fixed pseudo-random permutation. Hall: the fast-tree kernel on all of them; the brute-force kernel (the same scene
committed in tree mode 0, which builds no fast tree) on the first `brute` points of each order; terra_amd_intersect_device of as many rays -- from the same points,
in uniformly random directions -- as the yardstick. Cornell: the brute force (32 triangles) on all of them. Every figure is the median of `launches` launches, each
timed with a pair of HIP events after `warmup` untimed ones. Needs a GPU: there is no CPU path."""
import argparse, ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes


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


def grid_points(d, side, seed):
    """one uniform point per cell of a side^3 grid over the scene's bounding box, x fastest"""
    v = np.concatenate([np.asarray(ob.triangles, np.float32).reshape(-1, 3) for ob in d.objects]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    r = np.random.RandomState(seed)
    i = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1)[..., ::-1].reshape(-1, 3)      # (z, y, x) loops, (x, y, z) columns
    return (lo + (hi - lo) * (i + r.uniform(0, 1, size=i.shape)) / side).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=128); ap.add_argument("--brute", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/nearest/nearest_time.log")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/nearest_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def row(name, what, n, t, note=""):
        med, lo, hi = t
        say(f"{name:8s} {what:52s} {n:9d}  {med:9.3f} ms ({lo:.3f} .. {hi:.3f})  {n / med / 1e3:9.2f} M/s  {med * 1e6 / n:9.2f} ns each{note}")

    say(f"# tools/nearest_time.py side {a.side}: median (min .. max) of {a.launches} launches after {a.warmup} warm-up launches, HIP events; {torch.cuda.get_device_name(0)}")
    for name, d in (("cornell", scenes.cornell_box(16, 16, 1)), ("hall", scenes.sponza_hall(32, 18, 1))):
        pts = grid_points(d, a.side, 99); n = len(pts)
        perm = np.random.RandomState(1234).permutation(n)
        q = np.zeros(n, api.NEAREST_QUERY_DTYPE); q["position"] = pts; q["max_distance"] = np.inf
        up4 = lambda r: torch.from_numpy(r.view(np.float32).reshape(-1, 4).copy()).cuda()
        sets = {"grid order": up4(q), "permuted": up4(q[perm])}
        scene = scenes.build_scene(L, d, counters=False)
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(scene, C.byref(ti)))
        say(f"{name:8s} {sum(len(ob.triangles) for ob in d.objects)} triangles   [{ti.note.decode()}]")
        kernel = "fast tree" if ti.fast_tree else "brute force"
        t_fast = {}
        for order, t in sets.items():
            t_fast[order] = median_ms(torch, lambda: runtime.nearest(L, scene, t), a.launches, a.warmup)
            row(name, f"nearest, {kernel}, {order}", n, t_fast[order])
        if name == "hall":
            dirs = np.random.RandomState(77).normal(size=(n, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            rays = np.zeros(n, api.RAY_DTYPE); rays["origin"] = pts; rays["direction"] = dirs.astype(np.float32); rays["tmax"] = np.inf
            up8 = lambda r: torch.from_numpy(r.view(np.float32).reshape(-1, 8).copy()).cuda()
            t_ray = {}
            for order, t in (("grid order", up8(rays)), ("permuted", up8(rays[perm]))):
                t_ray[order] = median_ms(torch, lambda: runtime.intersect(L, scene, t), a.launches, a.warmup)
                row(name, f"intersect (yardstick), {order}", n, t_ray[order])
            slow = scenes.build_scene(L, d, counters=False, tree_mode=0)          # no fast tree: the brute force answers
            ts = runtime.TraversalInfo(); runtime.check(L.traversal_info(slow, C.byref(ts)))
            assert not ts.fast_tree
            m = min(a.brute, n)
            t_brute = {}
            for order, t in sets.items():
                part = t[:m].contiguous()
                same = runtime.nearest(L, slow, part).cpu().numpy().tobytes() == runtime.nearest(L, scene, part).cpu().numpy().tobytes()
                t_brute[order] = median_ms(torch, lambda: runtime.nearest(L, slow, part), a.launches, a.warmup)
                row(name, f"nearest, brute force (tree mode 0), {order}", m, t_brute[order], f"   same bits as the fast tree: {same}")
            for order in sets:
                per_fast, per_ray, per_brute = t_fast[order][0] / n, t_ray[order][0] / n, t_brute[order][0] / m
                say(f"{name:8s} {order}: a nearest query costs {per_fast / per_ray:.2f} x a closest-hit ray; the brute force costs {per_brute / per_fast:.0f} x the fast tree per query")
            L.scene_destroy(slow)
        L.scene_destroy(scene)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
