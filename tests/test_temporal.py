"""Temporal reprojection (terra_amd_reproject_device / terra_amd_reproject; include/terra_amd.h "Temporal reprojection") against a float32 numpy restatement of
the header's rule. The current sample (c, valid, a, z, n, u_c) is tests/test_denoise.py's restatement of the "Denoiser" section; what is added, restated:

  camera frame: Z = normalize(direction), X = normalize(up x Z), Y = Z x X; t = float(tan(double((fov * 0.0174533f) / 2))); aspect = float(W) / float(H);
  D = X e.x + Y e.y + Z e.z, e = normalize((sx aspect) t, sy t, 1), sx = 2 ((px + 0.5) / W) - 1, sy = 1 - 2 ((py + 0.5) / H);
  coverage > 0: P = pos + D z, v = P - prev_pos, d = |v|, (xc, yc, zc) = v in the previous camera's frame; no history unless zc > 0, -1 <= fx < W, -1 <= fy < H with
    fx = (((xc / zc) / (aspect t') + 1) / 2) W - 0.5, fy = ((1 - (yc / zc) / t') / 2) H - 0.5;
    snap (|fx - floor(fx + 0.5)| <= 1/64, same for fy): that one tap, its values copied; else the four bilinear taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1);
    tap accepted: weight > 0, in the rectangle, length > 0, |d - depth_q| <= tol max(d, depth_q), normals both zero or n . normal_q >= normal_cos (one zero fails);
    accepted if the weight sum >= 1e-3; u_h, mu1_h, mu2_h = weighted sums / weight sum; N_h = min length;
  coverage == 0: only if the cameras are equal byte for byte: tap p itself if its length > 0 and depth == 0;
  history: alpha_p = max(alpha, 1 / (N_h + 1)); valid: x' = x_h + alpha_p (x_c - x_h) for u, mu1 (l_c), mu2 (l_c l_c), length' = min(N_h + 1, floor(1 / alpha)); not valid: carried;
  no history: valid restarts (u_c, l_c, l_c l_c, 1), not valid is written empty; normal, depth: the current frame's;
  out_results = ((u' A) n, samples) (empty: the input result); out_moments = (out_results, mu1', var, 2, 1) with var = (max(0, mu2' - mu1'^2) alpha_p) r^2,
    r = max(l(u' A), 1e-6) / l(u'); zeros after seen_* where length' < 2, l(u') is not > 0 or var is not finite.

Every operation of the rule (+, -, *, /, sqrt, floor, compare) is correctly rounded on both sides and the build contracts nothing, so the comparison is bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

from terra_amd import api, scenes
from test_denoise import close, device_denoise, restate, synthetic
from test_denoise_variance import bits, lum, restate_variance

pytestmark = pytest.mark.gpu
F = np.float32
FW, FH = 32, 24
RECT = (3, 2, 26, 20)


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    from terra_amd import runtime
    assert torch.cuda.is_available()
    return runtime.load()


@pytest.fixture(scope="module")
def plain_scene(L):
    s = scenes.build_scene(L, scenes.cornell_box(16, 16, 1))
    yield s
    L.scene_destroy(s)


def camera(pos, direction, up=(0.0, 1.0, 0.0), fov=45.0):
    cam = api.TerraCamera()
    cam.position = api.f3(pos); cam.direction = api.f3(direction); cam.up = api.f3(up); cam.fov = fov
    return cam


def f3(v):
    return np.array([v.x, v.y, v.z], F)


def cross(a, b, T):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], T)


def norm(a, T):
    l = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return np.array([a[0] / l, a[1] / l, a[2] / l], T)


def frame_of(cam, W, H, T=F):
    """(X, Y, Z, tan of the half angle, aspect, position) in dtype T (float32: the host side's own arithmetic)"""
    Z = norm(f3(cam.direction).astype(T), T)
    X = norm(cross(f3(cam.up).astype(T), Z, T), T)
    Y = cross(Z, X, T)
    t = T(math.tan(float((F(cam.fov) * F(0.0174533)) / F(2))))
    return X, Y, Z, t, T(W) / T(H), f3(cam.position).astype(T)


def project(cam, prev, z, W, H, xx, yy, T=F):
    """fx, fy, zc, d of the header's rule for pixels (xx, yy) with first-hit distance z, every operation in dtype T"""
    X, Y, Z, t, aspect, pos = frame_of(cam, W, H, T)
    Xp, Yp, Zp, tp, _, ppos = frame_of(prev, W, H, T)
    with np.errstate(all="ignore"):
        sx = T(2) * ((xx.astype(T) + T(0.5) + T(0)) / T(W)) - T(1)
        sy = T(1) - T(2) * ((yy.astype(T) + T(0.5) + T(0)) / T(H))
        ex, ey, ez = sx * aspect * t, sy * t, np.ones_like(sx)
        ln = np.sqrt(ex * ex + ey * ey + ez * ez)
        ex, ey, ez = ex / ln, ey / ln, ez / ln
        D = [X[k] * ex + Y[k] * ey + Z[k] * ez for k in range(3)]
        v = [(pos[k] + D[k] * z) - ppos[k] for k in range(3)]
        xc = Xp[0] * v[0] + Xp[1] * v[1] + Xp[2] * v[2]
        yc = Yp[0] * v[0] + Yp[1] * v[1] + Yp[2] * v[2]
        zc = Zp[0] * v[0] + Zp[1] * v[1] + Zp[2] * v[2]
        fx = (((xc / zc) / (aspect * tp) + T(1)) / T(2)) * T(W) - T(0.5)
        fy = ((T(1) - (yc / zc) / tp) / T(2)) * T(H) - T(0.5)
        d = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return fx, fy, zc, d


def current(res, aov):
    """c, valid, A = max(a, 0.01), z, n, u_c of every pixel: the "Denoiser" section's. tests/test_denoise.py's `restate` hands out two of them, the mean c and the
    samples > 0 mask (its K = 0 form), and those are taken from it; the means over the AOV hits are locals of that function which it does not return, so their five
    lines are written out here as they stand there."""
    with np.errstate(all="ignore"):
        c0, sampled = restate(res, aov, 0)
        s = res["samples"]
        c = np.where(sampled[..., None], c0, res["acc"].astype(F) / s.astype(F)[..., None])          # (samples == 0: c is never used; kept as the device forms it)
        valid = sampled & np.isfinite(c).all(-1)
        cov = aov["coverage"].astype(F)
        hit = cov > 0
        dv = np.where(hit, cov, F(1))
        a = np.where(hit[..., None], aov["albedo"] / dv[..., None], F(0)).astype(F)
        z = np.where(hit, aov["depth"] / dv, F(0)).astype(F)
        nv = np.where(hit[..., None], aov["normal"] / dv[..., None], F(0)).astype(F)
        ln = np.sqrt(nv[..., 0] * nv[..., 0] + nv[..., 1] * nv[..., 1] + nv[..., 2] * nv[..., 2])
        nv = np.where((ln > F(1e-6))[..., None], nv / np.where(ln > 0, ln, F(1))[..., None], F(0)).astype(F)
        A = np.maximum(a, F(0.01))
        u = np.where(valid[..., None], c / A, F(0)).astype(F)
    return c, valid, A, z, nv, u, hit


def restate_temporal(res, aov, hin, cam, prev, rect=RECT, alpha=0.2, tol=0.05, ncos=0.9, hout=None, ores=None, omom=None):
    """(history_out, out_results, out_moments, info) over whole frames; only the rectangle is written (the rest is what hout / ores / omom held, zero by default)"""
    H, W = res.shape
    x0r, y0r, rw, rh = rect
    hout = np.zeros((H, W), api.HISTORY_DTYPE) if hout is None else hout.copy()
    ores = np.zeros((H, W), api.RESULT_DTYPE) if ores is None else ores.copy()
    omom = np.zeros((H, W), api.MOMENTS_DTYPE) if omom is None else omom.copy()
    alpha, tol, ncos = F(alpha), F(tol), F(ncos)
    c, valid, A, z, nv, uc, hit = current(res, aov)
    lc = lum(uc)
    yy, xx = np.mgrid[0:H, 0:W]
    inrect = (xx >= x0r) & (xx < x0r + rw) & (yy >= y0r) & (yy < y0r + rh)
    nz = (nv == 0).all(-1)
    have = np.zeros((H, W), bool)
    uh = np.zeros((H, W, 3), F); m1h = np.zeros((H, W), F); m2h = np.zeros((H, W), F); nh = np.zeros((H, W), F)
    snapped = np.zeros((H, W), bool); bilinear = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        if hin is not None:
            fx, fy, zc, d = project(cam, prev, z, W, H, xx, yy)
            geo = hit & (zc > 0) & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
            fx = np.where(geo, fx, F(0)); fy = np.where(geo, fy, F(0))
            rx, ry = np.floor(fx + F(0.5)), np.floor(fy + F(0.5))
            snap = (np.abs(fx - rx) <= F(1 / 64)) & (np.abs(fy - ry) <= F(1 / 64))

            def tap(qx, qy, wq, mask):
                inside = (qx >= x0r) & (qx < x0r + rw) & (qy >= y0r) & (qy < y0r + rh)
                h = hin[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                hn = h["normal"]; qz = (hn == 0).all(-1)
                dot = nv[..., 0] * hn[..., 0] + nv[..., 1] * hn[..., 1] + nv[..., 2] * hn[..., 2]
                n_ok = np.where(nz | qz, nz & qz, dot >= ncos)
                z_ok = np.abs(d - h["depth"]) <= tol * np.where(d > h["depth"], d, h["depth"])
                return mask & (wq > 0) & inside & (h["length"] > 0) & z_ok & n_ok, h

            ok, h = tap(rx.astype(np.int64), ry.astype(np.int64), np.ones((H, W), F), geo & snap)
            have |= ok; snapped = ok
            uh = np.where(ok[..., None], h["radiance"], uh); m1h = np.where(ok, h["mu1"], m1h); m2h = np.where(ok, h["mu2"], m2h); nh = np.where(ok, h["length"], nh)
            bx, by = np.floor(fx), np.floor(fy)
            tx, ty = fx - bx, fy - by
            ix, iy = bx.astype(np.int64), by.astype(np.int64)
            sw = np.zeros((H, W), F); su = np.zeros((H, W, 3), F); s1 = np.zeros((H, W), F); s2 = np.zeros((H, W), F); sl = np.full((H, W), np.inf, F)
            for dx, dy, wq in ((0, 0, (F(1) - tx) * (F(1) - ty)), (1, 0, tx * (F(1) - ty)), (0, 1, (F(1) - tx) * ty), (1, 1, tx * ty)):
                ok, h = tap(ix + dx, iy + dy, wq, geo & ~snap)
                sw = np.where(ok, sw + wq, sw)
                su = np.where(ok[..., None], su + wq[..., None] * h["radiance"], su)
                s1 = np.where(ok, s1 + wq * h["mu1"], s1); s2 = np.where(ok, s2 + wq * h["mu2"], s2)
                sl = np.where(ok & (h["length"] < sl), h["length"], sl)
            ok = geo & ~snap & (sw >= F(1e-3))
            have |= ok; bilinear = ok
            div = np.where(ok, sw, F(1))
            uh = np.where(ok[..., None], su / div[..., None], uh); m1h = np.where(ok, s1 / div, m1h); m2h = np.where(ok, s2 / div, m2h); nh = np.where(ok, sl, nh)
            if bytes(cam) == bytes(prev):
                ok = ~hit & (hin["length"] > 0) & (hin["depth"] == 0)
                have |= ok
                uh = np.where(ok[..., None], hin["radiance"], uh); m1h = np.where(ok, hin["mu1"], m1h); m2h = np.where(ok, hin["mu2"], m2h); nh = np.where(ok, hin["length"], nh)
        ap = np.where(have, np.maximum(alpha, F(1) / (nh + F(1))), F(1)).astype(F)
        cap = np.floor(F(1) / alpha)
        blend = have & valid; carry = have & ~valid; restart = ~have & valid
        un = np.where(blend[..., None], uh + ap[..., None] * (uc - uh), np.where(carry[..., None], uh, np.where(restart[..., None], uc, F(0)))).astype(F)
        m1 = np.where(blend, m1h + ap * (lc - m1h), np.where(carry, m1h, np.where(restart, lc, F(0)))).astype(F)
        m2 = np.where(blend, m2h + ap * (lc * lc - m2h), np.where(carry, m2h, np.where(restart, lc * lc, F(0)))).astype(F)
        ln = np.where(blend, np.minimum(nh + F(1), cap), np.where(carry, nh, np.where(restart, F(1), F(0)))).astype(F)
        new = np.zeros((H, W), api.HISTORY_DTYPE)
        new["radiance"] = un; new["length"] = ln; new["normal"] = nv; new["depth"] = z; new["mu1"] = m1; new["mu2"] = m2
        hout[inrect] = new[inrect]
        n = res["samples"].astype(F)
        cn = (un * A).astype(F)
        o = np.zeros((H, W), api.RESULT_DTYPE)
        o["acc"] = np.where((ln > 0)[..., None], cn * n[..., None], res["acc"]); o["samples"] = res["samples"]
        lu = lum(un)
        r = np.where(lum(cn) > F(1e-6), lum(cn), F(1e-6)) / lu
        var = ((np.where(m2 - m1 * m1 > 0, m2 - m1 * m1, F(0)) * ap) * (r * r)).astype(F)
        known = (ln >= 2) & (lu > 0) & np.isfinite(var)
        mo = np.zeros((H, W), api.MOMENTS_DTYPE)
        mo["seen_acc"] = o["acc"]; mo["seen_samples"] = o["samples"]
        mo["mean"] = np.where(known, m1, F(0)); mo["m2"] = np.where(known, var, F(0)); mo["batches"] = np.where(known, 2, 0); mo["weight"] = np.where(known, 1, 0)
        ores[inrect] = o[inrect]; omom[inrect] = mo[inrect]
    info = {"have": have & inrect, "restart": restart & inrect, "snapped": snapped & inrect, "bilinear": bilinear & inrect, "carry": carry & inrect, "blend": blend & inrect,
            "empty": (ln == 0) & inrect, "known": known & inrect, "inrect": inrect}
    return hout, ores, omom, info


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_device(t, a):
    import torch
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).view(t.dtype))


def device_reproject(L, scene, cam, prev, res, aov, hin, rect=RECT, alpha=0.0, tol=0.0, ncos=0.0, fill=None):
    """(history_out, out_results, out_moments) of the whole frame after terra_amd_reproject_device; fill: what the three output buffers hold before the call"""
    import torch
    from terra_amd import runtime
    h, w = res.shape
    fb = runtime.DeviceFramebuffer(w, h); to_device(fb.results, res)
    dv = runtime.DeviceAov(w, h); to_device(dv.data, aov)
    hi = None
    if hin is not None:
        hi = runtime.DeviceHistory(w, h); to_device(hi.data, hin)
    ho = runtime.DeviceHistory(w, h); ofb = runtime.DeviceFramebuffer(w, h); om = runtime.DeviceMoments(w, h)
    if fill is not None:
        to_device(ho.data, fill[0]); to_device(ofb.results, fill[1]); to_device(om.data, fill[2])
    runtime.reproject_device(L, scene, cam, prev, fb, dv, hi, ho, ofb, om, rect=rect, alpha=alpha, depth_tolerance=tol, normal_cos=ncos)
    torch.cuda.synchronize()
    return ho.host().copy(), ofb.results_host().copy(), om.host().copy()


def sentinel(h, w):
    r = np.random.RandomState(99)
    return (r.randint(1, 1 << 30, size=(h, w, 12)).astype(np.uint32).view(api.HISTORY_DTYPE).reshape(h, w),
            r.randint(1, 1 << 30, size=(h, w, 4)).astype(np.uint32).view(api.RESULT_DTYPE).reshape(h, w),
            r.randint(1, 1 << 30, size=(h, w, 8)).astype(np.uint32).view(api.MOMENTS_DTYPE).reshape(h, w))


def same(got, want):
    for g, w, name in zip(got, want, ("history_out", "out_results", "out_moments")):
        bad = np.argwhere((raw(g).reshape(FH, FW, -1) != raw(w).reshape(FH, FW, -1)).any(-1))
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


CAM = dict(pos=(0.1, 1.02, -3.3), direction=(0.05, -0.02, 1.0))
PREV = dict(pos=(0.0, 1.0, -3.4), direction=(0.0, 0.0, 1.0))


def synthetic_frame(seed):
    """tests/test_denoise.py's synthetic results (samples == 0, NaN / inf means) with geometry a history can match: a depth step at x = 20, a normal crease at
    y = 11, pixels without a hit; and a random history over the same geometry with some empty entries, some foreign depths and normals"""
    r = np.random.RandomState(seed)
    res, aov = synthetic(FW, FH, seed)
    cov = aov["coverage"]
    depth = np.where(np.arange(FW)[None, :] < 20, F(3.5), F(5.0)) * np.ones((FH, 1), F)
    nrm = np.zeros((FH, FW, 3), F); nrm[:11] = (0, 0, -1); nrm[11:] = (0, 0.6, -0.8)
    aov["depth"] = (depth * cov).astype(F)
    aov["normal"] = (nrm * cov[..., None]).astype(F)
    hin = np.zeros((FH, FW), api.HISTORY_DTYPE)
    hin["radiance"] = r.gamma(0.6, 1.0, size=(FH, FW, 3)); hin["length"] = r.randint(0, 9, size=(FH, FW))
    hin["normal"] = np.where((cov > 0)[..., None], nrm, F(0)); hin["depth"] = np.where(cov > 0, depth * r.uniform(0.985, 1.015, size=(FH, FW)), 0)
    odd = r.rand(FH, FW) < 0.1
    hin["depth"][odd] *= F(1.2)
    hin["normal"][r.rand(FH, FW) < 0.05] = (1, 0, 0)
    hin["mu1"] = r.gamma(0.6, 1.0, size=(FH, FW)); hin["mu2"] = hin["mu1"] ** 2 + r.gamma(0.5, 0.3, size=(FH, FW))
    hin["radiance"][hin["length"] == 0] = F(777.0)           # an empty entry's other fields must not be read
    return res, aov, hin


def test_synthetic_matches_restatement_bit_for_bit(L, plain_scene):
    """Camera translated and rotated. Bit for bit: no operation of the rule differs between numpy's float32 and the device (division and square root are correctly
    rounded in this build, nothing is contracted), so no bound on a difference is needed; none was observed."""
    cam, prev = camera(**CAM), camera(**PREV)
    res, aov, hin = synthetic_frame(5)
    fill = sentinel(FH, FW)
    want = restate_temporal(res, aov, hin, cam, prev, hout=fill[0], ores=fill[1], omom=fill[2])
    info = want[3]
    n = RECT[2] * RECT[3]
    print({k: int(v.sum()) for k, v in info.items()})
    x, y, w, h = RECT
    sl = (slice(y, y + h), slice(x, x + w))
    assert (res["samples"][sl] == 0).any() and (aov["coverage"][sl] == 0).any() and (hin["length"][sl] == 0).any()
    with np.errstate(all="ignore"):
        mean = res["acc"][sl] / res["samples"][sl].astype(F)[..., None]
    assert ((res["samples"][sl] > 0) & np.isnan(mean).any(-1)).any()         # a NaN mean
    assert info["bilinear"].sum() > n // 4 and info["restart"].sum() > n // 50 and info["carry"].sum() > 0 and info["empty"].sum() > 0 and info["known"].sum() > n // 8
    got = device_reproject(L, plain_scene, cam, prev, res, aov, hin, fill=fill)
    same(got, want[:3])
    same(device_reproject(L, plain_scene, cam, prev, res, aov, hin, fill=fill), got)          # the same inputs give the same bits
    # other options than the defaults, and the whole frame as the rectangle
    want = restate_temporal(res, aov, hin, cam, prev, rect=(0, 0, FW, FH), alpha=0.5, tol=0.01, ncos=0.99)
    same(device_reproject(L, plain_scene, cam, prev, res, aov, hin, rect=(0, 0, FW, FH), alpha=0.5, tol=0.01, ncos=0.99), want[:3])


@pytest.fixture(scope="module")
def cornell(L):
    """the Cornell box at 32 x 24, 2 spp, Direct, no subpixel jitter (so that a frame's AOVs do not depend on its seed): render(cam, seed) -> (results, aov) on the host"""
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(FW, FH, 2, integrator=api.kTerraIntegratorDirect, jitter=0.0)
    s = scenes.build_scene(L, d)
    fb = runtime.DeviceFramebuffer(FW, FH); aov = runtime.DeviceAov(FW, FH)

    def render(cam, seed):
        L.set_frame_seed(s, seed)
        fb.clear(); aov.clear()
        runtime.render_device(L, cam, s, fb); runtime.render_aov_device(L, cam, s, aov)
        torch.cuda.synchronize()
        return fb.results_host().copy(), aov.host().copy()
    yield s, scenes.camera_of(d), render
    L.scene_destroy(s)


STEP = 0.25         # the sideways step between the two cameras, world units (the room is 2 wide, 3.4 .. 5.4 away)


def two_frames(L, cornell):
    s, cam0, render = cornell
    cam1 = camera((cam0.position.x + STEP, cam0.position.y, cam0.position.z), (0.0, 0.0, 1.0))
    res0, aov0 = render(cam0, 11)
    h0 = device_reproject(L, s, cam0, cam0, res0, aov0, None)[0]
    res1, aov1 = render(cam1, 12)
    return s, cam0, cam1, (res0, aov0, h0), (res1, aov1)


def test_cornell_two_cameras_match_restatement(L, cornell):
    s, cam0, cam1, (res0, aov0, h0), (res1, aov1) = two_frames(L, cornell)
    want0 = restate_temporal(res0, aov0, None, cam0, cam0)
    same((h0,), want0[:1])
    want = restate_temporal(res1, aov1, h0, cam1, cam0)
    frac = want[3]["restart"].sum() / (RECT[2] * RECT[3])
    print(f"restarted pixels: {frac:.3f} of the rectangle; {({k: int(v.sum()) for k, v in want[3].items()})}")
    assert 0.01 <= frac <= 0.60, frac
    assert want[3]["blend"].sum() > 0
    same(device_reproject(L, s, cam1, cam0, res1, aov1, h0), want[:3])


def test_identity_same_camera_no_samples(L, plain_scene):
    """the snap rule and the carry-through: under the same camera a frame without samples hands every non-empty entry on unchanged"""
    cam = camera(**CAM)
    res, aov, hin = synthetic_frame(7)
    res["samples"] = 0; res["acc"] = 0
    _, _, _, z, nv, _, _ = current(res, aov)
    hin["normal"] = nv; hin["depth"] = z
    got = device_reproject(L, plain_scene, cam, cam, res, aov, hin)[0]
    x, y, w, h = RECT
    gi, hi = got[y:y + h, x:x + w], hin[y:y + h, x:x + w]
    full = hi["length"] > 0
    assert full.sum() > 400 and (~full).sum() > 20 and (aov["coverage"][y:y + h, x:x + w][full] == 0).any()
    assert np.array_equal(raw(gi[full]), raw(hi[full]))
    assert np.all(gi["length"][~full] == 0) and np.all(gi["radiance"][~full] == 0)


def test_a_miss_keeps_its_history_only_over_a_miss(L, plain_scene):
    """coverage == 0 under the same camera: the pixel's own entry is its history only if that entry was written over a miss too (depth == 0). Where the entry has
    a depth, the pixel restarts (valid) or is written empty (not valid), against the restatement bit for bit and by its own rule."""
    cam = camera(**CAM)
    res, aov, hin = synthetic_frame(13)
    x, y, w, h = RECT
    sl = (slice(y, y + h), slice(x, x + w))
    miss = aov["coverage"] == 0
    foreign = miss & (hin["length"] > 0) & (np.arange(FW)[None, :] % 2 == 0)
    hin["depth"][foreign] = F(2.5)
    kept = miss & (hin["length"] > 0) & ~foreign
    want = restate_temporal(res, aov, hin, cam, cam)
    got = device_reproject(L, plain_scene, cam, cam, res, aov, hin)
    same(got, want[:3])
    _, valid, _, _, _, uc, _ = current(res, aov)
    assert (foreign[sl] & valid[sl]).sum() > 10 and (foreign[sl] & ~valid[sl]).sum() > 0 and (kept[sl] & valid[sl]).sum() > 10
    g = got[0][sl]
    f_valid, f_not, k = (foreign & valid)[sl], (foreign & ~valid)[sl], (kept & valid)[sl]
    assert np.all(g["length"][f_valid] == 1) and np.array_equal(raw(g["radiance"][f_valid]), raw(uc[sl][f_valid]))
    assert np.all(g["length"][f_not] == 0) and np.all(g["radiance"][f_not] == 0)
    assert np.array_equal(g["length"][k], np.minimum(hin["length"][sl][k] + 1, 5))           # blended: floor(1 / 0.2) = 5 caps the length


def test_accumulation_is_the_running_mean(L, cornell):
    """N = 6 frames under one camera, alpha = 1/64: alpha_p = 1 / (k + 1) in frame k, the running mean. The tolerance is what the float32 restatement of the six
    blends shows against the float64 mean of the same u on this data (printed; about 1e-7 relative to the largest u), and the device equals that restatement."""
    s, cam, render = cornell
    N = 6
    hist32 = None; dev = None; us = []
    for k in range(N):
        res, aov = render(cam, 100 + k)
        us.append(current(res, aov)[5].astype(np.float64))
        dev = device_reproject(L, s, cam, cam, res, aov, dev, alpha=1 / 64)[0]
        hist32 = restate_temporal(res, aov, hist32, cam, cam, alpha=1 / 64)[0]
    x, y, w, h = RECT
    sl = (slice(y, y + h), slice(x, x + w))
    assert np.all(dev["length"][sl] == N)
    mean64 = np.mean(us, axis=0)[sl]
    tol = np.abs(hist32["radiance"][sl] - mean64).max()
    print(f"float32 restatement against the float64 running mean: {tol:.3g} (largest u {mean64.max():.3g})")
    assert tol <= 1e-5 * max(1.0, mean64.max())
    assert np.abs(dev["radiance"][sl] - mean64).max() <= tol
    mu1 = np.mean([lum(u.astype(F)).astype(np.float64) for u in us], axis=0)[sl]
    np.testing.assert_allclose(dev["mu1"][sl], mu1, rtol=1e-5, atol=1e-6)


def test_geometry_a_sideways_step_shifts_a_ramp(L, plain_scene):
    """A plane facing the camera at distance 4, the history a horizontal ramp (radiance = the pixel's column), the camera moved to the right by exactly K = 3 pixels'
    width at that distance: the history of pixel px is the ramp at px + 3. Without the restatement: only `project` (the header's formulas in one dtype) is used, to
    bound the rounding: fx in float32 differs from float64 by at most 3.9e-6 pixel on this input (printed), the ramp's slope is 1 per pixel, tolerance 4 x that."""
    K, Z0 = 3, 4.0
    prev = camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    t = math.tan(float((F(45.0) * F(0.0174533)) / F(2)))
    width = 2.0 * Z0 * t * (FW / FH) / FW
    cam = camera((K * width, 0.0, 0.0), (0.0, 0.0, 1.0))
    yy, xx = np.mgrid[0:FH, 0:FW]
    ex = (2 * ((xx + 0.5) / FW) - 1) * (FW / FH) * t; ey = (1 - 2 * ((yy + 0.5) / FH)) * t
    dist = (Z0 * np.sqrt(ex * ex + ey * ey + 1)).astype(F)
    aov = np.zeros((FH, FW), __import__("terra_amd.runtime", fromlist=["AOV_DTYPE"]).AOV_DTYPE)
    aov["coverage"] = 1; aov["albedo"] = 0.5; aov["normal"] = (0, 0, -1); aov["depth"] = dist; aov["samples"] = 1
    res = np.zeros((FH, FW), api.RESULT_DTYPE)
    hin = np.zeros((FH, FW), api.HISTORY_DTYPE)
    hin["radiance"] = xx[..., None].astype(F); hin["length"] = 4; hin["normal"] = (0, 0, -1); hin["depth"] = dist; hin["mu1"] = xx; hin["mu2"] = xx * xx
    z = current(res, aov)[3]
    f32 = project(cam, prev, z, FW, FH, xx, yy, F); f64 = project(cam, prev, z.astype(np.float64), FW, FH, xx, yy, np.float64)
    dev = max(np.abs(f32[0] - f64[0]).max(), np.abs(f32[1] - f64[1]).max())
    print(f"fx, fy float32 against float64: {dev:.3g} pixel")
    assert np.abs(f64[0] - (xx + K)).max() < 1e-9 + dev and dev < 1 / 64
    got = device_reproject(L, plain_scene, cam, prev, res, aov, hin)[0]
    x, y, w, h = RECT
    for py in range(y, y + h):
        for px in range(x, x + w):
            if px + K < x + w:
                assert got["length"][py, px] == 4 and abs(got["radiance"][py, px, 0] - (px + K)) <= 4 * dev, (px, py, got[py, px])
            else:
                assert got["length"][py, px] == 0, (px, py, got[py, px])


def test_chain_into_the_variance_guided_denoiser(L, cornell):
    """out_results / out_moments of a second frame fed to terra_amd_denoise_variance_device equal tests/test_denoise_variance.py's restatement on the same buffers at
    its tolerance; after a first frame (every length' = 1: every variance unknown) that filter gives terra_amd_denoise_device's bits."""
    import torch
    from terra_amd import runtime
    s, cam0, cam1, (res0, aov0, h0), (res1, aov1) = two_frames(L, cornell)
    x, y, w, h = RECT
    sl = (slice(y, y + h), slice(x, x + w))

    def variance_denoise(ores, aov, omom, K):
        fb = runtime.DeviceFramebuffer(FW, FH); to_device(fb.results, ores)
        dv = runtime.DeviceAov(FW, FH); to_device(dv.data, aov)
        dm = runtime.DeviceMoments(FW, FH); to_device(dm.data, omom)
        rad = torch.zeros(FH * FW * 3, dtype=torch.float32, device="cuda")
        runtime.denoise_variance_device(L, s, fb, dv, dm, K, rect=RECT, radiance=rad); torch.cuda.synchronize()
        return rad.cpu().numpy().reshape(FH, FW, 3)
    _, ores, omom = device_reproject(L, s, cam1, cam0, res1, aov1, h0)
    assert (omom["batches"][sl] == 2).sum() > 100 and (omom["batches"][sl] == 0).sum() > 0
    assert np.array_equal(raw(omom["seen_acc"]), raw(ores["acc"])) and np.array_equal(omom["seen_samples"], ores["samples"])
    for K in (1, 3):
        close(variance_denoise(ores, aov1, omom, K)[sl], restate_variance(ores[sl], aov1[sl], omom[sl], K))
    # the denoiser's own division and demodulation give u' back (to the rounding of a multiplication and a division by n, and one by A)
    hist = restate_temporal(res1, aov1, h0, cam1, cam0)[0]
    c, valid, A, _, _, u, _ = current(ores, aov1)
    np.testing.assert_allclose(u[sl][valid[sl]], hist["radiance"][sl][valid[sl]], rtol=4 * np.finfo(F).eps, atol=0)
    _, ores0, omom0 = device_reproject(L, s, cam0, cam0, res0, aov0, None)
    assert np.all(omom0["batches"][sl] == 0) and np.all(omom0["m2"][sl] == 0)
    plain = device_denoise(L, s, ores0[sl], aov0[sl], 3)[0]
    assert np.array_equal(raw(variance_denoise(ores0, aov0, omom0, 3)[sl]), raw(plain))


def test_arguments_and_the_host_form(L, plain_scene):
    import torch
    from terra_amd import runtime
    cam, prev = camera(**CAM), camera(**PREV)
    res, aov, hin = synthetic_frame(9)
    fb = runtime.DeviceFramebuffer(FW, FH); to_device(fb.results, res)
    dv = runtime.DeviceAov(FW, FH); to_device(dv.data, aov)
    hi = runtime.DeviceHistory(FW, FH); to_device(hi.data, hin)
    ho = runtime.DeviceHistory(FW, FH)
    r, a, i, o = fb.results.data_ptr(), dv.data.data_ptr(), hi.data.data_ptr(), ho.data.data_ptr()

    def call(scene=plain_scene, c=cam, p=prev, r=r, a=a, i=i, o=o, rect=RECT, opt=None, fw=FW, fh=FH):
        return L.reproject_device(scene, C.byref(c) if c is not None else None, C.byref(p) if p is not None else None, r, a, i, o, None, None, fw, fh, *rect,
                                  C.byref(opt) if opt is not None else None, None)
    assert call() == 0                                                     # NULL options, NULL outputs
    assert call(i=o) == -4                                                 # in place
    assert call(r=None) == -4 and call(a=None) == -4 and call(o=None) == -4 and call(c=None) == -4 and call(p=None) == -4
    assert call(rect=(3, 2, 30, 20)) == -4 and "bad reproject rectangle" in runtime.last_error()
    assert call(rect=(3, 2, 0, 20)) == -4 and call(rect=(3, 2, 26, 23)) == -4
    # pixel coordinates are floats: a frame side above 2^24 is refused before anything is launched (the rectangle itself is a good one in such a frame)
    assert call(fw=(1 << 24) + 1) == -4 and "2^24" in runtime.last_error()
    assert call(fh=(1 << 24) + 1) == -4 and "2^24" in runtime.last_error()
    for bad in ((1.5, 0, 0), (-0.1, 0, 0), (float("nan"), 0, 0), (0.2, -0.01, 0), (0.2, 0, -0.5)):
        assert call(opt=api.TerraAmdTemporalOptions(*bad, 0)) == -4, bad
    assert call(opt=api.TerraAmdTemporalOptions(1.0, 0, 0, 0)) == 0
    fresh = L.scene_create()
    assert call(scene=fresh) == -2
    L.scene_destroy(fresh)
    L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
    torch.cuda.synchronize()
    # NULL history_in: the first frame, every valid pixel restarts
    want = restate_temporal(res, aov, None, cam, prev)
    got = device_reproject(L, plain_scene, cam, prev, res, aov, None)
    same(got, want[:3])
    assert not want[3]["have"].any() and want[3]["restart"].sum() > 400
    # the host-buffer form: the device form's bits, and nothing outside the rectangle is touched
    fill = sentinel(FH, FW)
    dev = device_reproject(L, plain_scene, cam, prev, res, aov, hin, fill=fill, alpha=0.3)
    hfb = api.Framebuffer(L, FW, FH)
    np.copyto(hfb.results, res)
    h_out, h_res, h_mom = (np.ascontiguousarray(f.copy()) for f in fill)
    opt = api.TerraAmdTemporalOptions(0.3, 0, 0, 0)
    hin_c, aov_c = np.ascontiguousarray(hin), np.ascontiguousarray(aov)
    runtime.check(L.reproject(plain_scene, C.byref(cam), C.byref(prev), C.byref(hfb.fb), aov_c.ctypes.data, hin_c.ctypes.data, h_out.ctypes.data, h_res.ctypes.data, h_mom.ctypes.data,
                              *RECT, C.byref(opt)), "terra_amd_reproject")
    same((h_out, h_res, h_mom), dev)
    assert L.reproject(plain_scene, C.byref(cam), C.byref(prev), C.byref(hfb.fb), aov_c.ctypes.data, h_out.ctypes.data, h_out.ctypes.data, None, None, *RECT, None) == -4
    runtime.check(L.reproject(plain_scene, C.byref(cam), C.byref(prev), C.byref(hfb.fb), aov_c.ctypes.data, None, h_out.ctypes.data, None, None, *RECT, None), "terra_amd_reproject")
    same((h_out,), (restate_temporal(res, aov, None, cam, prev, hout=fill[0])[0],))
    L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
    hfb.destroy()
