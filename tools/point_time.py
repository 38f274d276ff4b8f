"""Times point rendering (include/terra_amd.h "Point rendering") against the camera and lens doors of the same commit and against what a client had to do before it,
in one run.
    python tools/point_time.py [--width 1920 --height 1080] [--spp 512] [--split 8] [--rounds 5] [--batch-rounds 2] [--out profiles/points/ab.md]
The scene is the Cornell box, 8 bounces, Simple integrator, subpixel jitter 0.5, explicit sample split `split`; the points frame holds a grid on the floor (normal +y)
in its upper half and a grid on the back wall (normal -z) in its lower half, one point per pixel:
  1. terra_amd_render_device with terra_amd_set_job_order(scene, 0): the scale of a render launch of this size (a point launch never has the job order or the empty skip);
  2. terra_amd_render_lens_device with a thin lens (radius 0.05): the nearest existing in-kernel generator;
  3. terra_amd_render_points_device, distribution 0 (cosine-weighted hemisphere);
  4. terra_amd_render_points_device, distribution 1 (uniform sphere);
  5. what a client must do without the point door for frame 3: spp / 8 batches of 8 spp through the ray door (sample split 1), each with a new full-frame ray
     buffer -- the host draws (g1, g2) per point, terra_amd_unit_point_rays makes the rays, the buffer is uploaded. Host clock around the whole loop, ending in a device
     synchronise: it counts the host's share, which is the point. With a library that has no point door (TERRA_AMD_LIB set to a build of the parent commit) only
     launch 1, 2 and 5 run, and the rays of 5 are made by the numpy generator below (the same formulas, numpy's sine and cosine).
Launches 1 - 4 are timed with HIP events, one launch per figure, ALTERNATING 1, 2, 3, 4, 1, ... for `rounds` rounds after one untimed round; the table gives the mean,
the standard deviation and the range of each. Needs a GPU: there is no CPU path."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes

F = np.float32


def bake_points(w, h):
    """[h, w, 8] float32 TerraAmdPoint records: the floor in the upper half of the frame, the back wall in the lower half"""
    pts = np.zeros((h, w, 8), F)
    u = (-0.95 + 1.9 * (np.arange(w) + 0.5) / w).astype(F)
    top = h // 2
    pts[:, :, 0] = u
    pts[:top, :, 1] = 0.0; pts[:top, :, 2] = (-0.95 + 1.9 * (np.arange(top) + 0.5) / top).astype(F)[:, None]; pts[:top, :, 5] = 1.0
    pts[top:, :, 1] = (0.05 + 1.9 * (np.arange(h - top) + 0.5) / (h - top)).astype(F)[:, None]; pts[top:, :, 2] = 1.0; pts[top:, :, 6] = -1.0
    return pts


def host_point_rays(points, g):
    """the header's distribution 0 in numpy float32 (numpy's sine and cosine): TerraAmdRay records [n, 8] for a library without terra_amd_unit_point_rays"""
    p = points.reshape(-1, 8); g1, g2 = g[:, 0], g[:, 1]
    n = p[:, 4:7] / np.sqrt((p[:, 4:7] * p[:, 4:7]).sum(axis=1, keepdims=True))
    s = np.copysign(F(1), n[:, 2]); a = F(-1) / (s + n[:, 2]); b = n[:, 0] * n[:, 1] * a
    t = np.stack([F(1) + s * n[:, 0] * n[:, 0] * a, s * b, -s * n[:, 0]], axis=1)
    bt = np.stack([b, s + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    ca, cb = F(2) * g1 - F(1), F(2) * g2 - F(1)
    with np.errstate(all="ignore"):
        wide = np.abs(ca) > np.abs(cb)
        r = np.where(wide, ca, cb)
        phi = np.where(wide, F(np.pi / 4) * (cb / ca), F(np.pi / 2) - F(np.pi / 4) * (ca / cb))
        phi = np.where((ca == 0) & (cb == 0), F(0), phi).astype(F)
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(F(0), F(1) - x * x - y * y))
    d = x[:, None] * t + y[:, None] * bt + z[:, None] * n
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    rays = np.zeros((len(p), 8), F)
    rays[:, 0:3] = p[:, 0:3]; rays[:, 3] = np.finfo(F).max; rays[:, 4:7] = d
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=512); ap.add_argument("--split", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--batch-rounds", type=int, default=2)
    ap.add_argument("--out", default="profiles/points/ab.md")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/point_time.py measures on a GPU; none is visible")
    L = runtime.load()
    has_points = hasattr(L, "render_points_device")
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    d = scenes.cornell_box(a.width, a.height, a.spp)
    cam = scenes.camera_of(d)
    scene = scenes.build_scene(L, d, counters=False)
    runtime.check(L.set_sample_split(scene, a.split)); runtime.check(L.set_job_order(scene, 0))
    fb = runtime.DeviceFramebuffer(d.width, d.height)
    host_pts = bake_points(d.width, d.height)
    pts = torch.from_numpy(host_pts).cuda()
    thin = api.Lens(); thin.model, thin.lens_radius, thin.focus_distance = 0, 0.05, 3.4
    doors = {"camera door, job order off (the scale of a render launch)": lambda: runtime.render_device(L, cam, scene, fb),
             "lens door, thin lens (radius 0.05)": lambda: runtime.render_lens_device(L, cam, thin, scene, fb)}
    if has_points:
        cosine, sphere = runtime.point_sampling(0), runtime.point_sampling(1)
        doors["point door, distribution 0 (cosine-weighted hemisphere)"] = lambda: runtime.render_points_device(L, scene, cosine, pts, fb)
        doors["point door, distribution 1 (uniform sphere)"] = lambda: runtime.render_points_device(L, scene, sphere, pts, fb)
    for fn in doors.values():          # the untimed round
        fb.clear(); fn(); torch.cuda.synchronize()
    ms = {k: [] for k in doors}
    for _ in range(a.rounds):
        for k, fn in doors.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    L.scene_destroy(scene)

    # the ray door in batches
    batches = a.spp // 8
    d8 = scenes.cornell_box(a.width, a.height, 8)
    scene8 = scenes.build_scene(L, d8, counters=False)
    runtime.check(L.set_sample_split(scene8, 1))
    rng = np.random.default_rng(1)
    flat = host_pts.reshape(-1, 8)
    batch_ms = []
    for rnd in range(a.batch_rounds + 1):          # (the first round is the warm-up)
        fb.clear(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            g = rng.random((len(flat), 2), dtype=np.float32)
            rays = runtime.point_rays(L, cosine, flat, g).view(np.float32) if has_points else host_point_rays(flat, g)
            dev = torch.from_numpy(rays.reshape(d.height, d.width, 8)).cuda()
            runtime.render_rays_device(L, scene8, dev, fb)
        torch.cuda.synchronize()
        if rnd:
            batch_ms.append((time.perf_counter() - t0) * 1e3)
    L.scene_destroy(scene8)
    made = "terra_amd_unit_point_rays" if has_points else "numpy on the host (a library without the point door)"
    ms[f"ray door, {batches} batches of 8 spp, a generated ray buffer each: {made} (host clock)"] = batch_ms

    say("# Point door against the camera and lens doors and against batches through the ray door (`tools/point_time.py`)")
    say()
    say(f"Cornell box, {a.width} x {a.height} points (floor and back wall), {a.spp} spp, 8 bounces, Simple integrator, jitter 0.5, explicit sample split {a.split}; "
        f"{torch.cuda.get_device_name(0)}. The in-kernel launches: one launch per figure, HIP events, alternating for {a.rounds} rounds after one untimed round. "
        f"The batched ray door: {a.batch_rounds} timed round(s) after one untimed, host clock around the whole loop up to a device synchronise.")
    say()
    say("| launch | mean ms | std | min .. max | against 1 |")
    say("|---|---|---|---|---|")
    like = float(np.mean(next(iter(ms.values()))))
    for n, (k, v) in enumerate(ms.items(), 1):
        v = np.asarray(v, np.float64)
        say(f"| {n}. {k} | {v.mean():.2f} | {v.std(ddof=1) if len(v) > 1 else 0.0:.2f} | {v.min():.2f} .. {v.max():.2f} | {v.mean() / like:.3f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
