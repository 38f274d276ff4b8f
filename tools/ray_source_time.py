"""Times ray-sourced rendering (include/terra_amd.h "Ray-sourced rendering") against the camera door of the same commit, in one run.
    python tools/ray_source_time.py [--width 1920 --height 1080] [--split 8] [--launches 7] [--warmup 2] [--out profiles/ray_source/ab.md]
Per scene -- the headline configuration (Cornell box, 512 spp, 8 bounces, jitter 0) and the hall at 256 spp -- three launches of the same frame with the same
explicit sample split:
  1. terra_amd_render_rays_device with the camera's own rays (the camera position and the device camera unit's direction per pixel);
  2. terra_amd_render_device with terra_amd_set_job_order(scene, 0): the like-for-like launch (a ray launch never has the job order or the empty skip);
  3. terra_amd_render_device with the defaults.
The yardstick of the ray door is launch 2; the gap to launch 3 is the known price of having no job order and no empty skip. The three framebuffers are compared on
bits before anything is timed. Every figure is the median of `launches` launches, each timed with a pair of HIP events on one stream after `warmup` untimed ones.
Needs a GPU: there is no CPU path."""
import argparse, ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from terra_amd import api, scenes


def camera_rays(L, d):
    """[height, width, 8] float32: the camera's own rays at jitter 0, directions from terra_amd_unit_camera (the render's camera_sample, bit for bit)"""
    from terra_amd import runtime
    xy = np.stack(np.meshgrid(np.arange(d.width, dtype=np.uint32), np.arange(d.height, dtype=np.uint32)), axis=-1).reshape(-1, 2).copy()
    r = np.zeros((len(xy), 2), np.float32); dirs = np.zeros((len(xy), 3), np.float32)
    cam = scenes.camera_of(d)
    f = L.fn("terra_amd_unit_camera", C.c_int, [C.POINTER(api.TerraCamera), C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p])
    runtime.check(f(C.byref(cam), d.width, d.height, len(xy), xy.ctypes.data, 0.0, r.ctypes.data, dirs.ctypes.data), "terra_amd_unit_camera")
    rays = np.zeros((len(xy), 8), np.float32)
    rays[:, 0:3] = np.asarray(d.camera_position, np.float32); rays[:, 3] = np.inf; rays[:, 4:7] = dirs
    return rays.reshape(d.height, d.width, 8)


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
    ap.add_argument("--split", type=int, default=8)
    ap.add_argument("--launches", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/ray_source/ab.md")
    a = ap.parse_args()
    import torch  # before the library: libterra_amd.so must bind to the HIP runtime torch loaded
    from terra_amd import runtime
    if not torch.cuda.is_available():
        sys.exit("tools/ray_source_time.py measures on a GPU; none is visible")
    L = runtime.load()
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    say("# Ray door against the camera door (`tools/ray_source_time.py`)")
    say()
    say(f"{a.width} x {a.height}, jitter 0, 8 bounces, Simple integrator, explicit sample split {a.split} on every launch; median (min .. max) of {a.launches} launches after "
        f"{a.warmup} warm-up launches, HIP events on one stream; {torch.cuda.get_device_name(0)}. The three framebuffers of a scene are bit-identical (checked before timing).")
    say()
    say("| scene | launch | ms | against the like-for-like camera launch |")
    say("|---|---|---|---|")
    for name, d in (("Cornell box, 512 spp", scenes.cornell_box(a.width, a.height, 512, jitter=0.0)), ("hall, 256 spp", scenes.sponza_hall(a.width, a.height, 256, jitter=0.0))):
        scene = scenes.build_scene(L, d, counters=False)
        runtime.check(L.set_sample_split(scene, a.split))
        cam = scenes.camera_of(d)
        rays = torch.from_numpy(camera_rays(L, d)).cuda()
        fb = runtime.DeviceFramebuffer(d.width, d.height)

        def door(which):
            if which == "rays":
                return lambda: runtime.render_rays_device(L, scene, rays, fb)
            return lambda: runtime.render_device(L, cam, scene, fb)
        got = {}
        for which, order in (("rays", 1), ("camera", 0), ("camera", 1)):          # one untimed launch each, into a cleared frame: the same bits
            runtime.check(L.set_job_order(scene, order)); fb.clear(); door(which)(); torch.cuda.synchronize()
            got[(which, order)] = fb.results.cpu().numpy().tobytes()
        assert got[("rays", 1)] == got[("camera", 0)] == got[("camera", 1)], f"{name}: the doors' framebuffers differ"
        ms = {}
        for label, which, order in (("ray door, the camera's own rays", "rays", 1), ("camera door, job order off (like for like)", "camera", 0), ("camera door, defaults", "camera", 1)):
            runtime.check(L.set_job_order(scene, order))
            ms[label] = median_ms(torch, door(which), a.launches, a.warmup)
        like = ms["camera door, job order off (like for like)"][0]
        for label, (med, lo, hi) in ms.items():
            say(f"| {name} | {label} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | {med / like:.3f} |")
        L.scene_destroy(scene)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
