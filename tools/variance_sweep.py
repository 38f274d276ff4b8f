"""The quality figures of DESIGN.md sections 15/16 for the variance-guided denoiser: Cornell 128 x 128, Direct, 8 calls of 1 spp, K = 5, against a converged frame at
another seed. Prints, per (sigma_l, cap), the full-frame RMSE ratio to the noisy frame, the ratio on the 99 % of the pixels below the noisy error's 99th percentile,
and the mean error.

    python tools/variance_sweep.py --cpu [--ref-spp 1024]      oracle-rendered radiance, first-hit guides cast at the pixel centres in numpy, moments and filter by
                                                               the numpy restatements of tests/test_moments.py and tests/test_denoise_variance.py: every
                                                               (sigma_l, cap) of --sigmas x --caps. No GPU.
    python tools/variance_sweep.py --gpu --label "4 / 4"       device-rendered inputs (4096-spp reference) and the device filter of the library that is loaded: one
                                                               row. sigma_l and the cap are compile-time constants (-DTERRA_VAR_SIGMA_L=, -DTERRA_VAR_PREFILTER_CAP=
                                                               through terra_amd.build.build(variant=...)); TERRA_AMD_LIB selects the variant."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def stats(den, noisy, ref):
    err = ((noisy - ref) ** 2).sum(-1)
    keep = err <= np.quantile(err, 0.99)
    rmse = lambda x, m=None: float(np.sqrt(np.mean(((x - ref) ** 2)[m] if m is not None else (x - ref) ** 2)))
    return rmse(den) / rmse(noisy), rmse(den, keep) / rmse(noisy, keep), den.mean() / ref.mean() - 1


def row(label, den, noisy, ref):
    f, r, m = stats(den.astype(np.float64), noisy, ref)
    print(f"{label:>28}: full {f:.3f}  99 % {r:.3f}  mean {m * 100:+.2f} %", flush=True)


def centre_guides(d):
    """first-hit albedo, normal, depth at the pixel centres (coverage 1 where hit), AOV_DTYPE; the camera of csrc/trace_geometry.h"""
    from terra_amd import runtime
    W, H = d.width, d.height
    nrm = lambda v: v / np.linalg.norm(v)
    z = nrm(np.array(d.camera_direction, np.float64)); xa = nrm(np.cross(np.array(d.camera_up, np.float64), z)); ya = np.cross(z, xa)
    t = np.tan(np.radians(d.camera_fov) / 2)
    py, px = np.mgrid[0:H, 0:W]
    fx = (2 * (px + 0.5) / W - 1) * (W / H) * t; fy = (1 - 2 * (py + 0.5) / H) * t
    dl = np.stack([fx, fy, np.ones_like(fx)], -1); dl /= np.linalg.norm(dl, axis=-1, keepdims=True)
    dirs = dl[..., 0:1] * xa + dl[..., 1:2] * ya + dl[..., 2:3] * z
    o = np.array(d.camera_position, np.float64)
    best = np.full((H, W), np.inf); alb = np.zeros((H, W, 3)); nv = np.zeros((H, W, 3))
    for ob in d.objects:
        for tri, tn in zip(np.asarray(ob.triangles, np.float64), np.asarray(ob.normals, np.float64)):
            e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
            p = np.cross(dirs, e2); det = p @ e1
            with np.errstate(all="ignore"):
                inv = 1.0 / det
                tv = o - tri[0]
                u = (p @ tv) * inv
                q = np.cross(tv, e1)
                v = (dirs @ q) * inv
                tt = (q @ e2) * inv
            hit = (np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 1e-6) & (tt < best)
            n = (1 - u - v)[..., None] * tn[0] + u[..., None] * tn[1] + v[..., None] * tn[2]
            n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
            best = np.where(hit, tt, best); alb[hit] = ob.material.albedo; nv[hit] = n[hit]
    a = np.zeros((H, W), runtime.AOV_DTYPE)
    hit = np.isfinite(best)
    a["coverage"] = hit; a["albedo"] = alb * hit[..., None]; a["normal"] = nv * hit[..., None]; a["depth"] = np.where(hit, best, 0); a["samples"] = 1
    return a


def cpu(a):
    import harness as H
    from terra_amd import api, scenes
    from test_denoise import restate
    from test_denoise_variance import restate_variance
    from test_moments import restate_accumulate
    orc = H.Unit("orc")
    d = scenes.cornell_box(128, 128, 1, integrator=api.kTerraIntegratorDirect)
    mom = np.zeros((128, 128), api.MOMENTS_DTYPE)
    res = np.zeros((128, 128), api.RESULT_DTYPE)
    for k in range(1, 9):                               # (passes on one framebuffer are the calls: the streams are keyed by the samples already in the pixel)
        o = orc.render_pixels(d, passes=k, want_calls=False, threads=8)
        res["acc"] = o["acc"]; res["samples"] = o["samples"]
        mom = restate_accumulate(res, mom)
    assert np.all(res["samples"] == 8) and np.all(mom["batches"] == 8)
    dr = scenes.cornell_box(128, 128, 256, integrator=api.kTerraIntegratorDirect)
    o = orc.render_pixels(dr, passes=a.ref_spp // 256, frame_seed=0xC0FFEE, want_calls=False, threads=8)
    ref = (o["acc"] / o["samples"][..., None]).astype(np.float64)
    noisy = (res["acc"] / res["samples"][..., None]).astype(np.float64)
    g = centre_guides(d)
    print(f"oracle inputs, guides at the pixel centres, {a.ref_spp}-spp reference; noisy mean {(noisy.mean() / ref.mean() - 1) * 100:+.2f} %", flush=True)
    row("a-trous", restate(res, g, 5)[0], noisy, ref)
    for cap in a.caps:
        for sl in a.sigmas:
            row(f"sigma_l {sl:g}, cap {cap:g}", restate_variance(res, g, mom, 5, sigma_l=sl, cap=cap), noisy, ref)


def gpu(a):
    import torch
    from terra_amd import api, runtime, scenes
    L = runtime.load()
    d = scenes.cornell_box(128, 128, 1, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d); cam = scenes.camera_of(d)
    fb = runtime.DeviceFramebuffer(128, 128); aov = runtime.DeviceAov(128, 128); dm = runtime.DeviceMoments(128, 128)
    for _ in range(8):
        runtime.render_device(L, cam, s, fb); runtime.render_aov_device(L, cam, s, aov); runtime.accumulate_moments_device(L, s, fb, dm)
    dr = scenes.cornell_box(128, 128, 256, integrator=api.kTerraIntegratorDirect)
    sr = scenes.build_scene(L, dr); L.set_frame_seed(sr, 0xC0FFEE)
    fr = runtime.DeviceFramebuffer(128, 128)
    for _ in range(16):
        runtime.render_device(L, scenes.camera_of(dr), sr, fr)
    torch.cuda.synchronize()
    r, rr = fb.results_host(), fr.results_host()
    noisy = (r["acc"] / r["samples"][..., None]).astype(np.float64); ref = (rr["acc"] / rr["samples"][..., None]).astype(np.float64)
    rad = torch.zeros(128 * 128 * 3, dtype=torch.float32, device="cuda")
    if a.label == "a-trous":
        runtime.denoise_device(L, s, fb, aov, 5, radiance=rad)
    else:
        runtime.denoise_variance_device(L, s, fb, aov, dm, 5, radiance=rad)
    torch.cuda.synchronize()
    row(f"MI355X {a.label}", rad.cpu().numpy().reshape(128, 128, 3), noisy, ref)
    L.scene_destroy(s); L.scene_destroy(sr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true"); ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1, 2, 4, 8, 16]); ap.add_argument("--caps", type=float, nargs="+", default=[4, 1e30])
    ap.add_argument("--ref-spp", type=int, default=1024); ap.add_argument("--label", default="sigma_l 4, cap 4")
    a = ap.parse_args()
    assert a.cpu != a.gpu
    (cpu if a.cpu else gpu)(a)
