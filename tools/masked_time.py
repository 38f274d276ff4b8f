"""Times adaptive tiles three ways on a 1920 x 1080 frame (HIP events over the whole call, one untimed round first): the tile driver
(terra_amd_render_adaptive_device: one call per active tile), the masked driver (terra_amd_render_adaptive_masked_device: one masked launch per round) and a
uniform run taken to the same largest tile error; samples traced and rounds of each. Then the fixed cost of a masked launch: an all-zero mask over the frame
(classifier, order, streams, an empty render grid, resolve), which every sparse round pays.
    python tools/masked_time.py [--scene cornell|hall] [--spp 4] [--tile 128] [--target 0.5] [--max-batches 64] [--repeats 5] [--tree-mode N]
The sample split is the library's automatic one: the masked launch takes the split of the whole rectangle, a tile call that of a tile."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


def main():
    import torch  # before the library (terra_amd/runtime.py)
    from terra_amd import api, runtime, scenes
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell", choices=["cornell", "hall"]); ap.add_argument("--spp", type=int, default=4); ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--target", type=float, default=0.5); ap.add_argument("--max-batches", type=int, default=64); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-mode", type=int, default=-1, help="terra_amd_set_tree_mode (default: the library's automatic choice)")
    a = ap.parse_args()
    L = runtime.load()
    W, H = 1920, 1080
    make = scenes.cornell_box if a.scene == "cornell" else scenes.sponza_hall
    d = make(W, H, a.spp, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d, tree_mode=None if a.tree_mode < 0 else a.tree_mode, counters=False)
    cam = scenes.camera_of(d)
    fb = runtime.DeviceFramebuffer(W, H); dm = runtime.DeviceMoments(W, H)

    def adaptive(masked):
        fb.clear(); dm.clear()
        return event_ms(lambda: runtime.render_adaptive_device(L, cam, s, fb, dm, None, tile=a.tile, min_batches=4, max_batches=a.max_batches, target_error=a.target, masked=masked))

    def uniform(stop_at):
        fb.clear(); dm.clear()
        def run():
            n = 0
            while n < a.max_batches:
                runtime.render_device(L, cam, s, fb); runtime.accumulate_moments_device(L, s, fb, dm); n += 1
                if n >= 2 and float(runtime.tile_error_device(L, fb, dm, tile=a.tile).max()) <= stop_at:
                    break
            return n
        return event_ms(run)

    ti = runtime.TraversalInfo()
    adaptive(False)                                      # untimed round
    can_mask = True
    try:
        adaptive(True)
    except runtime.TerraAmdError as e:                   # a scene that is not LDS-resident: the masked calls refuse it (include/terra_amd.h "Masked rendering")
        can_mask = False; L.clear_error()
        print(f"masked driver refused: {e}", flush=True)
    runtime.check(L.traversal_info(s, __import__("ctypes").byref(ti)))
    print(f"{a.scene} {W} x {H}, Direct, batches of {a.spp} spp, tile {a.tile}, target {a.target}; lds_resident {ti.lds_resident}, last_call {ti.last_call} ({runtime.CALL_TRAVERSAL.get(ti.last_call)}); {torch.cuda.get_device_name(0)}", flush=True)
    rows = {"tile": [], "masked": [], "uniform": []}
    rep_t = rep_m = None
    for _ in range(a.repeats):
        ms, rep_t = adaptive(False); rows["tile"].append(ms)
        if can_mask:
            ms, rep_m = adaptive(True); rows["masked"].append(ms)
        ms, n_un = uniform(max(rep_t["max_error"], a.target)); rows["uniform"].append(ms)
    for k, v in rows.items():
        if not v:
            continue
        v.sort()
        print(f"{k:8s} median {v[len(v) // 2]:9.2f} ms   min {v[0]:9.2f}   max {v[-1]:9.2f}", flush=True)
    print(f"tile driver:   {rep_t}", flush=True)
    print(f"masked driver: {rep_m}", flush=True)
    print(f"uniform: {n_un} batches, {n_un * W * H * a.spp} samples", flush=True)
    if not can_mask:
        L.scene_destroy(s)
        return
    # the fixed cost of a masked launch
    zero = torch.zeros(runtime.mask_shape(W, H), dtype=torch.int32, device="cuda")
    one = torch.ones(runtime.mask_shape(W, H), dtype=torch.int32, device="cuda")
    for name, m in (("all-zero mask", zero), ("all-one mask", one)):
        ts = sorted(event_ms(lambda: runtime.render_masked_device(L, cam, s, fb, m))[0] for _ in range(a.repeats + 1))[: a.repeats]
        print(f"masked launch, {name}: median {ts[len(ts) // 2]:.3f} ms, min {ts[0]:.3f}", flush=True)
    ts = sorted(event_ms(lambda: runtime.render_device(L, cam, s, fb))[0] for _ in range(a.repeats + 1))[: a.repeats]
    print(f"unmasked launch: median {ts[len(ts) // 2]:.3f} ms, min {ts[0]:.3f}", flush=True)
    L.scene_destroy(s)


if __name__ == "__main__":
    main()
