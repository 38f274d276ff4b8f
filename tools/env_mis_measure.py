"""Environment MIS, measured on one GPU: image means of the three estimators of the courtyard's light -- plain (no environment sampling),
section 12's environment sampling alone, and section 12 + environment MIS -- on a diffuse and on a GGX floor, at growing sample counts and two frame seeds, so that
a gap between them can be told from their noise; and the time of one Direct + MIS render of a 1080p courtyard at 64 spp with section 12 alone and with MIS.

    python tools/env_mis_measure.py [--means] [--timing]

With TERRA_AMD_LIB pointing at an older build that lacks terra_amd_set_environment_mis, only the section-12-alone timings run (an A/B of that path)."""
import argparse
import dataclasses
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from terra_amd import api, runtime, scenes  # noqa: E402
from test_environment_sampling import courtyard  # noqa: E402

DM = api.kTerraIntegratorDirectMis


def scene(w, h, spp, sampling, mis, floor):
    d = courtyard(w, h, spp, DM, sampling)
    if floor == "ggx":
        d.objects[0] = dataclasses.replace(d.objects[0], material=scenes.Material(kind="ggx", specular_color=(0.9, 0.9, 0.9), roughness=0.05))
    d.environment_mis = mis
    return d


def mean_of(L, d, seed):
    s = scenes.build_scene(L, d, counters=False)
    L.set_frame_seed(s, seed)
    fb = runtime.DeviceFramebuffer(d.width, d.height)
    runtime.render_device(L, scenes.camera_of(d), s, fb); torch.cuda.synchronize()
    r = fb.results_host()
    L.scene_destroy(s)
    return float((r["acc"] / r["samples"][..., None]).astype(np.float64).mean())


def means(L):
    for floor in ("diffuse", "ggx"):
        for spp in (512, 4096, 32768):
            for seed in (1, 2):
                m = {k: mean_of(L, scene(96, 64, spp * f, s, x, floor), seed) for k, s, x, f in (("plain", False, False, 8), ("section12", True, False, 1), ("mis", True, True, 1))}
                print(f"means {floor:7s} spp {spp:6d} (plain x8) seed {seed}: plain {m['plain']:.5f} section12 {m['section12']:.5f} mis {m['mis']:.5f}   "
                      f"mis/plain {m['mis'] / m['plain'] - 1:+.4f} mis/section12 {m['mis'] / m['section12'] - 1:+.4f} section12/plain {m['section12'] / m['plain'] - 1:+.4f}", flush=True)


def timing(L):
    runs = [False, True] * 2 if L.has("terra_amd_set_environment_mis") else [False] * 2
    for mis in runs:
        d = scene(1920, 1080, 64, True, mis, "ggx")
        s = scenes.build_scene(L, d, counters=False); cam = scenes.camera_of(d)
        fb = runtime.DeviceFramebuffer(d.width, d.height)
        runtime.render_device(L, cam, s, fb); torch.cuda.synchronize()          # warm-up
        ts = []
        for _ in range(5):
            fb.clear(); torch.cuda.synchronize(); t = time.perf_counter()
            runtime.render_device(L, cam, s, fb); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
        print(f"timing {runtime.LIB_PATH.name}: courtyard 1920x1080 64 spp GGX floor, Direct + MIS, {'section 12 + MIS' if mis else 'section 12 alone'}: "
              f"min {min(ts):.2f} ms (runs {', '.join(f'{t:.2f}' for t in ts)})", flush=True)
        L.scene_destroy(s)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--means", action="store_true"); ap.add_argument("--timing", action="store_true")
    a = ap.parse_args()
    L = runtime.load()
    if a.means:
        means(L)
    if a.timing:
        timing(L)
