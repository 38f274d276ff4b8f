"""Times the steps of a probe bake (include/terra_amd.h "Probe harmonics") in one run, and reports how far order-2 SH irradiance is from a gathered one.
    python tools/probe_time.py [--grid 32x16x32] [--cells 16] [--spp 16] [--queries 1000000] [--rounds 5] [--out profiles/probes/ab.md]
The scene is the hall (scenes.sponza_hall, 8 bounces, Simple integrator) with a grid of probes cell-centred over its bounding box (runtime.probe_grid_over).
  1. terra_amd_probe_rays_device, cell centres;
  2. terra_amd_render_rays_device on the probe frame (cells * cells wide, one row per probe), `spp` samples per ray;
  3. terra_amd_sh_project_device, batch 0, on the frame of 2;
  4. terra_amd_sh_irradiance_device in grid mode: `queries` points uniform in the grid's box, normals uniform over the sphere.
Timed with HIP events, one call per figure, ALTERNATING 1, 2, 3, 4, 1, ... for `rounds` rounds after one untimed round; the table gives the mean, the standard
deviation and the range of each, and the share of 1 and 3 in the bake 1 + 2 + 3.
Accuracy (nothing is asserted): on the Cornell box, SH irradiance at a few probes -- baked at `cells` x `cells` cells, once along the cell centres (4 batches into
one frame) and once as 16 batches of one independent jitter per cell each -- against the point door's cosine-weighted irradiance (runtime.irradiance, 64 batches) at
the same points and normals. Needs a GPU: there is no CPU path."""
import argparse, math, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="32x16x32"); ap.add_argument("--cells", type=int, default=16); ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1000000); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/probes/ab.md")
    a = ap.parse_args()
    counts = tuple(int(v) for v in a.grid.split("x"))
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/probe_time.py measures on a GPU; none is visible")
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
    grid, probes = runtime.probe_grid_over(L, v.min(0), v.max(0), counts)
    P = len(probes)
    d_probes = device(probes)
    fb = runtime.DeviceFramebuffer(K, P)
    rng = np.random.default_rng(1)
    q = np.zeros(a.queries, api.POINT_DTYPE)
    q["position"] = rng.uniform(v.min(0), v.max(0), (a.queries, 3))
    q["normal"] = rng.normal(0, 1, (a.queries, 3))
    d_queries = device(q)
    state = {}

    def rays():
        state["rays"] = runtime.probe_rays(L, d_probes, a.cells)

    def project():
        state["sh"] = runtime.sh_project(L, fb, state["rays"], a.cells)

    def lookup():
        state["E"] = runtime.sh_irradiance(L, state["sh"], d_queries, grid=grid)

    steps = {"probe_rays, cell centres": (None, rays), f"render_rays_device, {a.spp} spp": (fb.clear, lambda: runtime.render_rays_device(L, scene, state["rays"], fb)),
             "sh_project, batch 0": (None, project), f"sh_irradiance, grid mode, {a.queries} queries": (None, lookup)}
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
    lit = int((runtime.probe_sh_host(state["sh"])["c"][:, 0].sum(-1) > 0).sum())
    L.scene_destroy(scene)

    say("# The steps of a probe bake (`tools/probe_time.py`)")
    say()
    say(f"The hall, {d.triangle_count} triangles, {counts[0]} x {counts[1]} x {counts[2]} = {P} probes cell-centred over its bounding box ({lit} of them see light), "
        f"{a.cells} x {a.cells} cells each: a probe frame of {K} x {P} = {K * P} rays; 8 bounces, Simple integrator; {torch.cuda.get_device_name(0)}. One call per figure, "
        f"HIP events, alternating for {a.rounds} rounds after one untimed round.")
    say()
    say("| step | mean ms | std | min .. max |")
    say("|---|---|---|---|")
    mean = {}
    for n, (k, t) in enumerate(ms.items(), 1):
        t = np.asarray(t, np.float64); mean[n] = t.mean()
        say(f"| {n}. {k} | {t.mean():.3f} | {t.std(ddof=1) if len(t) > 1 else 0.0:.3f} | {t.min():.3f} .. {t.max():.3f} |")
    bake = mean[1] + mean[2] + mean[3]
    say()
    say(f"The bake 1 + 2 + 3 takes {bake:.2f} ms: the rays are {100 * mean[1] / bake:.2f} % of it, the projection {100 * mean[3] / bake:.2f} % "
        f"({48 * K * P / mean[3] / 1e6:.0f} GB/s over the 48 bytes it reads per cell). The lookup answers {a.queries / mean[4] / 1e3:.0f} M queries per second.")

    # accuracy: order-2 SH against a gathered irradiance, Cornell box
    c = scenes.cornell_box(16, 16, 16, bounces=4, integrator=api.kTerraIntegratorDirect)
    scene = scenes.build_scene(L, c, counters=False)
    where = np.array([[0.0, 1.0, -0.2], [0.0, 1.0, -0.2], [0.0, 1.0, -0.2], [-0.5, 0.4, -0.5], [0.5, 1.5, 0.5]], F)
    facing = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1, 0], [-1, 0, -1]], F)
    pts = np.zeros(len(where), api.POINT_DTYPE)
    pts["position"], pts["normal"] = where, np.array([0, 0, 1], F)
    sh = runtime.bake_probes(L, scene, device(pts), cells=a.cells, batches=4)
    sh_jittered = runtime.bake_probes(L, scene, device(pts), cells=a.cells, batches=16, jitter=1)
    pts["normal"] = facing
    index = torch.arange(len(where), dtype=torch.int32, device="cuda")
    E_sh = runtime.sh_irradiance(L, sh, device(pts), index=index).cpu().numpy()[:, :3]
    E_jit = runtime.sh_irradiance(L, sh_jittered, device(pts), index=index).cpu().numpy()[:, :3]
    E_gather = runtime.irradiance(L, scene, torch.from_numpy(where).cuda(), torch.from_numpy(facing).cuda(), spp_batches=64).cpu().numpy()
    L.scene_destroy(scene)
    say()
    say("# Order-2 SH irradiance against a gathered one")
    say()
    say(f"The Cornell box, Direct integrator, 4 bounces: probes of {a.cells} x {a.cells} cells -- along the cell centres, 4 x 16 samples per cell, and as 16 batches of 16 "
        f"samples with one independent jitter per cell each -- against the point door's cosine-weighted irradiance at the same point and normal, 64 x 16 samples. "
        f"Nothing is asserted: nine coefficients cannot hold a small bright light, and a fixed set of centres sees such a light through whole cells.")
    say()
    say("| position | normal | SH, cell centres (r g b) | SH, jittered batches (r g b) | gathered (r g b) | centres / gathered | jittered / gathered |")
    say("|---|---|---|---|---|---|---|")
    for k in range(len(where)):
        ratio = [float(np.mean(E[k] / np.maximum(E_gather[k], 1e-9))) for E in (E_sh, E_jit)]
        say(f"| {where[k][0]:g} {where[k][1]:g} {where[k][2]:g} | {facing[k][0]:g} {facing[k][1]:g} {facing[k][2]:g} | {E_sh[k][0]:.4f} {E_sh[k][1]:.4f} {E_sh[k][2]:.4f} | "
            f"{E_jit[k][0]:.4f} {E_jit[k][1]:.4f} {E_jit[k][2]:.4f} | {E_gather[k][0]:.4f} {E_gather[k][1]:.4f} {E_gather[k][2]:.4f} | {ratio[0]:.3f} | {ratio[1]:.3f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
