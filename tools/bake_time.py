"""Times the steps of a lightmap bake (include/terra_amd.h "Lightmap baking") in one run.
    python tools/bake_time.py [--atlas 1024] [--spp 64] [--passes 4] [--rounds 5] [--out profiles/bake/ab.md]
The scene is the hall (scenes.sponza_hall, 8 bounces, Simple integrator) with an atlas this tool generates: one square cell per triangle, row-major in scene triangle
order, the triangle's chart the cell's lower-left half inset by half a texel (the hall's 97,478 triangles leave cells of 3.3 texels at 1024 x 1024).
  1. terra_amd_atlas_points_device, margin 0;
  2. terra_amd_atlas_points_device, margin 0.5;
  3. terra_amd_render_points_device, distribution 0, `spp` samples per texel, on the points of 2: the launch the rasteriser feeds;
  4. terra_amd_dilate_device, `passes` passes, on the irradiance of 3 with triangle >= 0 as the validity (a fresh copy each time, made outside the timed span).
Timed with HIP events, one call per figure, ALTERNATING 1, 2, 3, 4, 1, ... for `rounds` rounds after one untimed round; the table gives the mean, the standard
deviation and the range of each, and the rasteriser's and the dilation's share of the bake 2 + 3 + 4. Needs a GPU: there is no CPU path."""
import argparse, math, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import scenes

F = np.float32


def cell_uvs(triangles, size):
    """[triangles, 6] float32: triangle k's chart in cell k of a square grid over a size x size atlas; returns (uvs, cells per side)"""
    cells = int(math.ceil(math.sqrt(triangles)))
    step = size / cells
    k = np.arange(triangles)
    x0, y0 = (k % cells) * step + 0.5, (k // cells) * step + 0.5
    x1, y1 = x0 + step - 1.0, y0 + step - 1.0
    return np.stack([x0, y0, x1, y0, x0, y1], axis=1).astype(F), cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atlas", type=int, default=1024); ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--passes", type=int, default=4); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/bake/ab.md")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/bake_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    d = scenes.sponza_hall(a.atlas, a.atlas, a.spp)
    scene = scenes.build_scene(L, d, counters=False)
    uvs_host, cells = cell_uvs(d.triangle_count, a.atlas)
    uvs = torch.from_numpy(uvs_host).cuda()
    state = {}

    def raster(margin):
        state["points"], state["texels"] = runtime.atlas_points(L, scene, runtime.atlas_of(a.atlas, a.atlas, margin=margin), uvs)

    fb = runtime.DeviceFramebuffer(a.atlas, a.atlas)
    cosine = runtime.point_sampling(0)

    def gather():
        runtime.render_points_device(L, scene, cosine, state["points"], fb)

    def prepare_dilate():
        res = fb.results.view(a.atlas, a.atlas, 4)
        state["irradiance"] = (math.pi * res[..., :3].view(torch.float32) / res[..., 3:4].to(torch.float32)).contiguous()
        state["valid"] = (state["texels"][..., 0] >= 0).to(torch.int32).contiguous()

    steps = {"atlas_points, margin 0": (None, lambda: raster(0.0)), "atlas_points, margin 0.5": (None, lambda: raster(0.5)),
             f"render_points_device, distribution 0, {a.spp} spp": (fb.clear, gather),
             f"dilate, {a.passes} passes, 3 channels": (prepare_dilate, lambda: runtime.dilate(state["irradiance"], state["valid"], a.passes))}
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
    covered = int((state["texels"][..., 0] >= 0).sum().item())
    grown = int((state["valid"] != 0).sum().item())
    L.scene_destroy(scene)

    say("# The steps of a lightmap bake (`tools/bake_time.py`)")
    say()
    say(f"The hall, {d.triangle_count} triangles, one atlas cell per triangle ({cells} x {cells} cells) on a {a.atlas} x {a.atlas} atlas: {covered} texels covered at margin 0.5, "
        f"{grown} valid after {a.passes} dilation passes; 8 bounces, Simple integrator; {torch.cuda.get_device_name(0)}. One call per figure, HIP events, alternating for "
        f"{a.rounds} rounds after one untimed round.")
    say()
    say("| step | mean ms | std | min .. max |")
    say("|---|---|---|---|")
    mean = {}
    for n, (k, v) in enumerate(ms.items(), 1):
        v = np.asarray(v, np.float64); mean[n] = v.mean()
        say(f"| {n}. {k} | {v.mean():.3f} | {v.std(ddof=1) if len(v) > 1 else 0.0:.3f} | {v.min():.3f} .. {v.max():.3f} |")
    bake = mean[2] + mean[3] + mean[4]
    say()
    say(f"The bake 2 + 3 + 4 takes {bake:.2f} ms: the rasteriser is {100 * mean[2] / bake:.2f} % of it, the dilation {100 * mean[4] / bake:.2f} %.")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
