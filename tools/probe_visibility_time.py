"""Times the steps of a probe visibility bake and of the visible lookup (include/terra_amd.h "Probe visibility") in one run.
    python tools/probe_visibility_time.py [--grid 32x16x32] [--cells 16] [--texels 8,16] [--sharpness 6] [--spp 16] [--queries 1000000] [--rounds 5] [--out profiles/probe_visibility/ab.md]
The scene is the hall (scenes.sponza_hall, 8 bounces, Simple integrator) with a grid of probes cell-centred over its bounding box (runtime.probe_grid_over); a miss
and the cap are the diagonal of that box.
  1. terra_amd_intersect_device along the cell-centre probe rays;
  2. terra_amd_probe_visibility_device on those hits, accumulate 0, per map size in --texels;
  3. terra_amd_sh_irradiance_visible_device: `queries` points uniform in the grid's box, normals uniform over the sphere, per map size;
  4. terra_amd_sh_irradiance_device in grid mode on the same queries;
  5. terra_amd_render_rays_device on the probe frame at `spp` samples per ray: the yardstick a bake's other steps are held against.
Timed with HIP events, one call per figure, ALTERNATING through the steps for `rounds` rounds after one untimed round; the table gives the mean, the standard
deviation and the range of each. Needs a GPU: there is no CPU path."""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="32x16x32"); ap.add_argument("--cells", type=int, default=16); ap.add_argument("--texels", default="8,16")
    ap.add_argument("--sharpness", type=int, default=6); ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1000000); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/probe_visibility/ab.md")
    a = ap.parse_args()
    counts = tuple(int(v) for v in a.grid.split("x"))
    sizes = [int(v) for v in a.texels.split(",")]
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/probe_visibility_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    def device(records):
        return torch.from_numpy(np.ascontiguousarray(records).view(F).reshape(len(records), -1)).cuda()

    K = a.cells * a.cells
    d = scenes.sponza_hall(K, 16, a.spp)
    scene = scenes.build_scene(L, d, counters=False)
    v = runtime.scene_vertex_points(L, scene)["position"]
    lo, hi = v.min(0), v.max(0)
    grid, probes = runtime.probe_grid_over(L, lo, hi, counts)
    P = len(probes)
    diagonal = float(np.sqrt(np.square((hi - lo).astype(np.float64)).sum()))
    options = {m: runtime.probe_visibility_options(texels=m, sharpness=a.sharpness, max_distance=diagonal) for m in sizes}
    d_probes = device(probes)
    fb = runtime.DeviceFramebuffer(K, P)
    rng = np.random.default_rng(1)
    q = np.zeros(a.queries, api.POINT_DTYPE)
    q["position"] = rng.uniform(lo, hi, (a.queries, 3))
    q["normal"] = rng.normal(0, 1, (a.queries, 3))
    d_queries = device(q)
    rays = runtime.probe_rays(L, d_probes, a.cells)
    runtime.render_rays_device(L, scene, rays, fb)
    sh = runtime.sh_project(L, fb, rays, a.cells)
    state = {}

    def intersect():
        state["hits"] = runtime.intersect(L, scene, rays.view(-1, 8))

    def project(m):
        state[m] = runtime.probe_visibility(L, state["hits"], rays, a.cells, options[m])

    def visible(m):
        state["E", m] = runtime.sh_irradiance_visible(L, sh, state[m], d_queries, grid, options[m])

    def plain():
        state["E"] = runtime.sh_irradiance(L, sh, d_queries, grid=grid)

    steps = {"intersect, cell-centre rays": (None, intersect)}
    for m in sizes:
        steps[f"probe_visibility, {m} x {m} texels, sharpness {a.sharpness}"] = (None, lambda m=m: project(m))
    for m in sizes:
        steps[f"sh_irradiance_visible, {m} x {m} texels, {a.queries} queries"] = (None, lambda m=m: visible(m))
    steps[f"sh_irradiance, grid mode, {a.queries} queries"] = (None, plain)
    steps[f"render_rays_device, {a.spp} spp"] = (fb.clear, lambda: runtime.render_rays_device(L, scene, rays, fb))
    ms = {k: [] for k in steps}
    for rnd in range(a.rounds + 1):          # (the first round is untimed)
        for k, (before, fn) in steps.items():
            if before:
                before()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if rnd:
                ms[k].append(e0.elapsed_time(e1))
    hits = state["hits"].cpu().numpy().view(api.HIT_DTYPE).reshape(-1)
    missed = int((hits["object"] < 0).sum())
    dimmed = {m: float((np.abs(state["E", m].cpu().numpy()[:, :3] - state["E"].cpu().numpy()[:, :3]).max(-1) > 1e-6).mean()) for m in sizes}
    L.scene_destroy(scene)

    say("# The steps of a probe visibility bake and the visible lookup (`tools/probe_visibility_time.py`)")
    say()
    say(f"The hall, {d.triangle_count} triangles, {counts[0]} x {counts[1]} x {counts[2]} = {P} probes cell-centred over its bounding box, {a.cells} x {a.cells} cells each: "
        f"{K * P} rays, {missed} of them misses; max_distance = the box's diagonal, {diagonal:.3f}; 8 bounces, Simple integrator; {torch.cuda.get_device_name(0)}. One call per "
        f"figure, HIP events, alternating for {a.rounds} rounds after one untimed round.")
    say()
    say("| step | mean ms | std | min .. max |")
    say("|---|---|---|---|")
    mean = {}
    for n, (k, t) in enumerate(ms.items(), 1):
        t = np.asarray(t, np.float64); mean[k] = t.mean()
        say(f"| {n}. {k} | {t.mean():.3f} | {t.std(ddof=1) if len(t) > 1 else 0.0:.3f} | {t.min():.3f} .. {t.max():.3f} |")
    keys = list(ms)
    render = mean[keys[-1]]
    say()
    for n, m in enumerate(sizes):
        t = mean[keys[1 + n]]
        say(f"The projection onto {m} x {m} texels is {100 * t / render:.2f} % of the {a.spp} spp render of the same frame: {K * P * m * m / t / 1e6:.1f} G weight evaluations per second "
            f"({K * P * m * m} of them).")
    say(f"The distances (step 1) are {100 * mean[keys[0]] / render:.2f} % of that render.")
    for n, m in enumerate(sizes):
        t = mean[keys[1 + len(sizes) + n]]
        say(f"The visible lookup on {m} x {m} texel maps answers {a.queries / t / 1e3:.1f} M queries per second, the plain one {a.queries / mean[keys[-2]] / 1e3:.1f} M; "
            f"{100 * dimmed[m]:.1f} % of the queries get another answer than the plain lookup's.")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
