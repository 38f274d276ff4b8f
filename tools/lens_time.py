"""Times lens rendering (include/terra_amd.h "Lens rendering") against the camera door of the same commit and against what a client had to do before it, in one run.
    python tools/lens_time.py [--width 1920 --height 1080] [--spp 512] [--split 8] [--rounds 5] [--batch-rounds 2] [--out profiles/lens/ab.md]
The frame is the Cornell box, 8 bounces, Simple integrator, subpixel jitter 0.5, explicit sample split `split`:
  1. terra_amd_render_device with terra_amd_set_job_order(scene, 0): the like-for-like camera launch (a lens launch never has the job order or the empty skip);
  2. terra_amd_render_lens_device, model 0 with lens_radius 0 (the same rays; its framebuffer is compared with launch 1's on bits before anything is timed);
  3. terra_amd_render_lens_device with a thin lens (radius 0.05, focused on the middle of the box);
  4. what a client must do without the lens door for the same thin-lens frame: spp / 8 batches of 8 spp through the ray door (sample split 1), each with a new
     full-frame ray buffer -- the host draws (r1, r2, l1, l2) per pixel, terra_amd_unit_lens_rays makes the rays, the buffer is uploaded. Host clock around the whole
     loop, ending in a device synchronise: it counts the host's share, which is the point.
Launches 1 - 3 are timed with HIP events, one launch per figure, ALTERNATING 1, 2, 3, 1, 2, 3 ... for `rounds` rounds after one untimed round; the table gives the
mean, the standard deviation and the range of each. Needs a GPU: there is no CPU path."""
import argparse, ctypes as C, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes


def lens_of(model=0, lens_radius=0.0, focus_distance=0.0):
    l = api.Lens()
    l.model, l.lens_radius, l.focus_distance = model, lens_radius, focus_distance
    return l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=512); ap.add_argument("--split", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--batch-rounds", type=int, default=2)
    ap.add_argument("--out", default="profiles/lens/ab.md")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/lens_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    d = scenes.cornell_box(a.width, a.height, a.spp)
    cam = scenes.camera_of(d)
    scene = scenes.build_scene(L, d, counters=False)
    runtime.check(L.set_sample_split(scene, a.split)); runtime.check(L.set_job_order(scene, 0))
    fb = runtime.DeviceFramebuffer(d.width, d.height)
    pinhole, thin = lens_of(0), lens_of(0, 0.05, 3.4)
    doors = {"camera door, job order off (like for like)": lambda: runtime.render_device(L, cam, scene, fb),
             "lens door, lens_radius 0": lambda: runtime.render_lens_device(L, cam, pinhole, scene, fb),
             "lens door, thin lens (radius 0.05)": lambda: runtime.render_lens_device(L, cam, thin, scene, fb)}
    got = []
    for fn in list(doors.values())[:2]:          # the untimed round doubles as the check: the pinhole through the lens door is the camera door
        fb.clear(); fn(); torch.cuda.synchronize()
        got.append(fb.results.cpu().numpy().tobytes())
    assert got[0] == got[1], "lens door at lens_radius 0 and camera door: the framebuffers differ"
    list(doors.values())[2](); torch.cuda.synchronize()
    ms = {k: [] for k in doors}
    for _ in range(a.rounds):
        for k, fn in doors.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    L.scene_destroy(scene)

    # 4. the ray door in batches
    batches = a.spp // 8
    d8 = scenes.cornell_box(a.width, a.height, 8)
    scene8 = scenes.build_scene(L, d8, counters=False)
    runtime.check(L.set_sample_split(scene8, 1))
    xy = np.stack(np.meshgrid(np.arange(d.width, dtype=np.uint32), np.arange(d.height, dtype=np.uint32)), axis=-1).reshape(-1, 2).copy()
    rng = np.random.default_rng(1)
    batch_ms = []
    for rnd in range(a.batch_rounds + 1):          # (the first round is the warm-up)
        fb.clear(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            r4 = rng.random((len(xy), 4), dtype=np.float32)
            rays = runtime.lens_rays(L, cam, thin, d.width, d.height, xy, d.jitter, r4)
            dev = torch.from_numpy(rays.view(np.float32).reshape(d.height, d.width, 8)).cuda()
            runtime.render_rays_device(L, scene8, dev, fb)
        torch.cuda.synchronize()
        if rnd:
            batch_ms.append((time.perf_counter() - t0) * 1e3)
    L.scene_destroy(scene8)
    ms[f"ray door, {batches} batches of 8 spp, a generated ray buffer each (host clock)"] = batch_ms

    say("# Lens door against the camera door and against batches through the ray door (`tools/lens_time.py`)")
    say()
    say(f"Cornell box, {a.width} x {a.height}, {a.spp} spp, 8 bounces, Simple integrator, jitter 0.5, explicit sample split {a.split}; {torch.cuda.get_device_name(0)}. "
        f"Launches 1 - 3: one launch per figure, HIP events, alternating for {a.rounds} rounds after one untimed round (in which the framebuffers of 1 and 2 were "
        f"compared: bit-identical). Launch 4: {a.batch_rounds} timed round(s) after one untimed, host clock around the whole loop up to a device synchronise.")
    say()
    say("| launch | mean ms | std | min .. max | against 1 |")
    say("|---|---|---|---|---|")
    like = float(np.mean(ms["camera door, job order off (like for like)"]))
    for n, (k, v) in enumerate(ms.items(), 1):
        v = np.asarray(v, np.float64)
        say(f"| {n}. {k} | {v.mean():.2f} | {v.std(ddof=1) if len(v) > 1 else 0.0:.2f} | {v.min():.2f} .. {v.max():.2f} | {v.mean() / like:.3f} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
