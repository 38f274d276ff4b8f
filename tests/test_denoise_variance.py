"""The variance-guided denoiser (terra_amd_denoise_variance_device; include/terra_amd.h "Variance-guided denoiser") against a float32 numpy restatement.
Everything but the colour weight is tests/test_denoise.py's restatement of the a-trous filter; what is added, restated:

  var_p = m2 / (weight (batches - 1)) for batches >= 2; v_p = var_p (l(u_p) / max(l(c_p), 1e-6))^2 where p is valid and var_p known (and v_p finite), else unknown;
  centre p with known v:  g_p = sum k min(v_q, 4 v_p) / sum k over the 3 x 3 pixels around p (dy outer, dx inner) in the rectangle, valid, with known v; k = (1/4, 1/8, 1/16) w_n w_z (w_z of step 1);
    w_c = exp(-(|l(u_p) - l(u_q)| / (sigma_l sqrt(g_p) + 1e-6))), sigma_l = 8;  v'_p = sum W^2 v_q / (sum W)^2 over the taps with known v;
  centre p with unknown v (or being rescued): the a-trous w_c, v' unknown.

exp is the only operation the two sides compute differently: tolerance 1e-5 relative / 1e-6 absolute, as in tests/test_denoise.py."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, scenes
from test_denoise import HK, close, device_denoise, restate, synthetic

pytestmark = pytest.mark.gpu
F = np.float32
SIGMA_L = 8.0


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


def lum(v):
    return F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1] + F(0.0722) * v[..., 2]


def restate_variance(results, aov, mom, K, sigma_l=SIGMA_L, sigma_c2=0.25, sigma_z=0.05, cap=4.0):
    """radiance (h, w, 3) of the rectangle given as (h, w) arrays"""
    if K == 0:
        return restate(results, aov, 0)[0]
    with np.errstate(all="ignore"):
        acc = results["acc"].astype(F); s = results["samples"]
        n = s.astype(F)
        c = acc / n[..., None]
        finite = (s > 0) & np.isfinite(c).all(-1)
        pending = (s > 0) & ~finite
        cov = aov["coverage"].astype(F)
        hit = cov > 0
        dv = np.where(hit, cov, F(1))
        a = np.where(hit[..., None], aov["albedo"] / dv[..., None], F(0)).astype(F)
        z = np.where(hit, aov["depth"] / dv, F(0)).astype(F)
        nv = np.where(hit[..., None], aov["normal"] / dv[..., None], F(0)).astype(F)
        ln = np.sqrt(nv[..., 0] * nv[..., 0] + nv[..., 1] * nv[..., 1] + nv[..., 2] * nv[..., 2])
        nv = np.where((ln > F(1e-6))[..., None], nv / np.where(ln > 0, ln, F(1))[..., None], F(0)).astype(F)
        amax = np.maximum(a, F(0.01))
        u = np.where(finite[..., None], c / amax, F(0)).astype(F)
        valid = finite.copy()
        kn = mom["batches"] >= 2
        var = np.where(kn, mom["m2"] / np.where(kn, mom["weight"].astype(F) * (mom["batches"] - 1).astype(F), F(1)), F(-1)).astype(F)
        r = lum(u) / np.maximum(lum(c), F(1e-6))
        v = (var * (r * r)).astype(F)
        known = valid & kn & (var >= 0) & np.isfinite(v) & (v >= 0)
        v = np.where(known, v, F(-1))
        H, W = s.shape
        nz = (nv == 0).all(-1)
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(K):
            st = 1 << i
            sc2 = F(sigma_c2) * F(4.0 ** -i)
            active = valid | (pending if i == 0 else False)
            pend = pending & ~valid if i == 0 else np.zeros_like(valid)
            kc = known & ~pend & valid
            gs = np.zeros((H, W), F); gw = np.zeros((H, W), F)
            vcap = (F(cap) * v).astype(F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = yy + dy, xx + dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    okq = inside & valid[qyc, qxc] & known[qyc, qxc]
                    nq = nv[qyc, qxc]; nqz = nz[qyc, qxc]
                    dot = np.maximum(F(0), nv[..., 0] * nq[..., 0] + nv[..., 1] * nq[..., 1] + nv[..., 2] * nq[..., 2])
                    for _ in range(7):
                        dot = dot * dot
                    wn = np.where(nz | nqz, np.where(nz & nqz, F(1), F(0)), dot)
                    zq = z[qyc, qxc]
                    wz = np.exp(-(np.abs(z - zq) / (F(sigma_z) * np.maximum(z, zq) + F(1e-6)))).astype(F)
                    k = ((F((0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)) * wn) * wz).astype(F)
                    gs = np.where(okq, gs + k * np.minimum(v[qyc, qxc], vcap), gs).astype(F); gw = np.where(okq, gw + k, gw).astype(F)
            tol = (F(sigma_l) * np.sqrt(gs / np.where(gw > 0, gw, F(1))) + F(1e-6)).astype(F)
            lp = lum(u)
            sw = np.zeros((H, W), F); su = np.zeros((H, W, 3), F); swk = np.zeros((H, W), F); sv = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = yy + st * dy, xx + st * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    uq = u[qyc, qxc]; vq_ok = valid[qyc, qxc] & inside
                    e = u - uq
                    d2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]
                    lq = lum(uq)
                    wc = np.exp(-(d2 / (sc2 * (lp * lp + lq * lq) + F(1e-8)))).astype(F)
                    wcv = np.exp(-(np.abs(lp - lq) / tol)).astype(F)
                    wc = np.where(pend, F(1), np.where(kc, wcv, wc))
                    nq = nv[qyc, qxc]; nqz = nz[qyc, qxc]
                    dot = np.maximum(F(0), nv[..., 0] * nq[..., 0] + nv[..., 1] * nq[..., 1] + nv[..., 2] * nq[..., 2])
                    for _ in range(7):
                        dot = dot * dot
                    wn = np.where(nz | nqz, np.where(nz & nqz, F(1), F(0)), dot)
                    zq = z[qyc, qxc]
                    wz = np.exp(-(np.abs(z - zq) / ((F(sigma_z) * F(st)) * np.maximum(z, zq) + F(1e-6)))).astype(F)
                    Wt = (((HK[dx + 2] * HK[dy + 2]) * wc) * wn) * wz
                    Wt = np.where(vq_ok & active, Wt, F(0)).astype(F)
                    sw = sw + Wt
                    su = su + Wt[..., None] * np.where(vq_ok[..., None], uq, F(0))
                    kq = vq_ok & known[qyc, qxc] & kc
                    swk = np.where(kq, swk + Wt, swk).astype(F); sv = np.where(kq, sv + (Wt * Wt) * v[qyc, qxc], sv).astype(F)
            ok = active & (sw > 0)
            u = np.where(ok[..., None], su / np.where(ok, sw, F(1))[..., None], F(0)).astype(F)
            known = kc & ok & (swk > 0)
            v = np.where(known, sv / np.where(known, swk * swk, F(1)), F(-1)).astype(F)
            valid = ok
        return np.where(valid[..., None], u * amax, F(0)).astype(F)


def synthetic_moments(res, seed, unknown=0.2):
    """moments that go with res: a plausible variance for most pixels, fewer than two batches for the rest"""
    r = np.random.RandomState(seed)
    h, w = res.shape
    m = np.zeros((h, w), api.MOMENTS_DTYPE)
    m["seen_acc"] = res["acc"]; m["seen_samples"] = res["samples"]
    m["batches"] = np.where(r.rand(h, w) < unknown, r.randint(0, 2, size=(h, w)), r.randint(2, 9, size=(h, w)))
    m["weight"] = np.maximum(res["samples"], m["batches"])
    with np.errstate(all="ignore"):
        l = np.nan_to_num(lum(res["acc"] / np.maximum(res["samples"], 1)[..., None].astype(F)), nan=0.0, posinf=0.0, neginf=0.0).astype(F)
    m["mean"] = l
    m["m2"] = (r.gamma(0.5, 0.3, size=(h, w)) * (l * l + F(0.01)) * m["weight"] * np.maximum(m["batches"] - 1, 0)).astype(F)
    return m


def device_denoise_variance(L, scene, res, aov, mom, K, rect=None, in_place=False):
    import torch
    from terra_amd import runtime
    h, w = res.shape
    fb = runtime.DeviceFramebuffer(w, h)
    fb.results.copy_(torch.from_numpy(np.ascontiguousarray(res).view(np.int32).reshape(-1)))
    dv = runtime.DeviceAov(w, h)
    dv.data.copy_(torch.from_numpy(np.ascontiguousarray(aov).view(np.int32).reshape(-1)))
    dm = runtime.DeviceMoments(w, h)
    dm.data.copy_(torch.from_numpy(np.ascontiguousarray(mom).view(np.int32).reshape(-1)))
    rad = torch.full((h * w * 3,), -7.0, dtype=torch.float32, device="cuda")
    pix = torch.full((h * w * 3,), -7.0, dtype=torch.float32, device="cuda")
    runtime.denoise_variance_device(L, scene, fb, dv, dm, K, rect=rect, radiance=rad, pixels=pix)
    torch.cuda.synchronize()
    return rad.cpu().numpy().reshape(h, w, 3), pix.cpu().numpy().reshape(h, w, 3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_synthetic_matches_restatement(L, plain_scene, K):
    res, aov = synthetic(64, 48, 21 + K)
    mom = synthetic_moments(res, 31 + K)
    rad, pix = device_denoise_variance(L, plain_scene, res, aov, mom, K)
    want = restate_variance(res, aov, mom, K)
    close(rad, want)
    assert np.array_equal(bits(pix), bits(rad))
    assert not np.allclose(rad, restate(res, aov, K)[0], rtol=1e-3, atol=1e-4)          # (the variance does change the filter)
    rad2, _ = device_denoise_variance(L, plain_scene, res, aov, mom, K)
    assert np.array_equal(bits(rad), bits(rad2))


def cornell_batches(L, width, height, spp, calls, tonemap=api.kTerraTonemappingOperatorNone, exposure=1.0):
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(width, height, spp, integrator=api.kTerraIntegratorDirect, tonemap=tonemap, exposure=exposure)
    s = scenes.build_scene(L, d)
    cam = scenes.camera_of(d)
    fb = runtime.DeviceFramebuffer(width, height); aov = runtime.DeviceAov(width, height); dm = runtime.DeviceMoments(width, height)
    for _ in range(calls):
        runtime.render_device(L, cam, s, fb)
        runtime.render_aov_device(L, cam, s, aov)
        runtime.accumulate_moments_device(L, s, fb, dm)
    torch.cuda.synchronize()
    return s, fb, aov, dm


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_cornell_matches_restatement(L, K):
    s, fb, aov, dm = cornell_batches(L, 64, 48, 1, 8)
    res, a, m = fb.results_host().copy(), aov.host().copy(), dm.host().copy()
    assert np.all(m["batches"] == 8)
    rad, _ = device_denoise_variance(L, s, res, a, m, K)
    close(rad, restate_variance(res, a, m, K))
    L.scene_destroy(s)


def test_zeroed_moments_give_the_a_trous_filter_bit_for_bit_and_zero_iterations_the_identity(L, plain_scene):
    import torch
    from terra_amd import runtime
    res, aov = synthetic(64, 48, 4)
    zero = np.zeros((48, 64), api.MOMENTS_DTYPE)
    for K in (1, 3, 5, 8):
        r0, p0 = device_denoise(L, plain_scene, res, aov, K)
        r1, p1 = device_denoise_variance(L, plain_scene, res, aov, zero, K)
        assert np.array_equal(bits(r0), bits(r1)) and np.array_equal(bits(p0), bits(p1)), K
    one = zero.copy(); one["batches"] = 1; one["weight"] = 4; one["m2"] = 3.0          # one batch: still unknown
    assert np.array_equal(bits(device_denoise_variance(L, plain_scene, res, aov, one, 4)[0]), bits(device_denoise(L, plain_scene, res, aov, 4)[0]))
    # K = 0: the identity, in place on the framebuffer's own pixels too, and through the host form
    s, fb, av, dm = cornell_batches(L, 64, 48, 2, 4, tonemap=api.kTerraTonemappingOperatorLinear)
    rad = torch.zeros(64 * 48 * 3, dtype=torch.float32, device="cuda"); pix = torch.zeros_like(rad)
    runtime.denoise_variance_device(L, s, fb, av, dm, 0, radiance=rad, pixels=pix); torch.cuda.synchronize()
    r = fb.results_host()
    assert np.array_equal(bits(pix.cpu().numpy()), bits(fb.pixels.cpu().numpy()))
    assert np.array_equal(bits(rad.cpu().numpy().reshape(48, 64, 3)), bits((r["acc"] / r["samples"][..., None].astype(F)).astype(F)))
    before = fb.pixels.clone()
    runtime.denoise_variance_device(L, s, fb, av, dm, 0, pixels=fb.pixels); torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), fb.pixels.view(torch.int32))
    hfb = api.Framebuffer(L, 64, 48)
    np.copyto(hfb.results, r)
    ha, hm = av.host().copy(), dm.host().copy()
    hr = np.zeros((48, 64, 3), F)
    runtime.check(L.denoise_variance(s, C.byref(hfb.fb), ha.ctypes.data, hm.ctypes.data, 0, 0, 64, 48, 3, hr.ctypes.data, None), "terra_amd_denoise_variance")
    dr = torch.zeros_like(rad)
    runtime.denoise_variance_device(L, s, fb, av, dm, 3, radiance=dr); torch.cuda.synchronize()
    assert np.array_equal(bits(hr), bits(dr.cpu().numpy().reshape(48, 64, 3)))
    args = (s, fb.results.data_ptr(), av.data.data_ptr(), dm.data.data_ptr(), 64, 48)
    assert L.denoise_variance_device(*args, 0, 0, 64, 48, 9, None, fb.pixels.data_ptr(), None) == -4
    assert L.denoise_variance_device(*args, 1, 0, 64, 48, 2, None, fb.pixels.data_ptr(), None) == -4
    assert L.denoise_variance_device(s, fb.results.data_ptr(), av.data.data_ptr(), None, 64, 48, 0, 0, 64, 48, 2, None, fb.pixels.data_ptr(), None) == -4
    L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
    hfb.destroy(); L.scene_destroy(s)


def test_constant_radiance_stays_constant(L, plain_scene):
    res, aov = synthetic(64, 48, 3)
    res["samples"] = np.maximum(res["samples"], 1)
    col = np.array([0.37, 1.25, 0.05], F)
    res["acc"] = (col * res["samples"][..., None].astype(F)).astype(F)
    aov["albedo"] = (np.array([0.6, 0.3, 0.8], F) * aov["coverage"][..., None]).astype(F)
    mom = synthetic_moments(res, 8)
    for K in (1, 4, 8):
        rad, _ = device_denoise_variance(L, plain_scene, res, aov, mom, K)
        np.testing.assert_allclose(rad, np.broadcast_to(res["acc"] / res["samples"][..., None].astype(F), rad.shape), rtol=1e-6, atol=0)


def test_no_leakage_across_a_normal_edge_and_outside_the_rectangle(L, plain_scene):
    res, aov = synthetic(64, 48, 5)
    mom = synthetic_moments(res, 6)
    aov["coverage"] = np.maximum(aov["coverage"], 1)
    aov["albedo"] = (np.full((48, 64, 3), 0.5, F) * aov["coverage"][..., None]).astype(F)
    half = np.zeros((48, 64, 3), F); half[:, :32] = (1, 0, 0); half[:, 32:] = (0, 1, 0)
    aov["normal"] = (half * aov["coverage"][..., None]).astype(F)
    r0, _ = device_denoise_variance(L, plain_scene, res, aov, mom, 5)
    res2 = res.copy(); res2["acc"][:, 32:] *= F(3.0)
    r1, _ = device_denoise_variance(L, plain_scene, res2, aov, mom, 5)          # (g_p too stops at the edge: its neighbours carry w_n w_z)
    assert np.array_equal(bits(r0[:, :32]), bits(r1[:, :32]))
    assert not np.array_equal(r0[:, 32:], r1[:, 32:])
    rect = (8, 4, 40, 36)
    res, aov = synthetic(64, 48, 6)
    mom = synthetic_moments(res, 7)
    g0, p0 = device_denoise_variance(L, plain_scene, res, aov, mom, 4, rect=rect)
    res3, aov3, mom3 = res.copy(), aov.copy(), mom.copy()
    out = np.ones((48, 64), bool); out[4:40, 8:48] = False
    res3["acc"][out] = F(123.0); res3["samples"][out] = 5; aov3["albedo"][out] = F(0.01); aov3["coverage"][out] = F(1.0)
    mom3["m2"][out] = F(55.0); mom3["batches"][out] = 4; mom3["weight"][out] = 5
    g1, p1 = device_denoise_variance(L, plain_scene, res3, aov3, mom3, 4, rect=rect)
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(p0), bits(p1))
    assert np.all(g0[out] == F(-7.0)) and np.all(p0[out] == F(-7.0))
    close(g0[4:40, 8:48], restate_variance(res[4:40, 8:48], aov[4:40, 8:48], mom[4:40, 8:48], 4))


@pytest.mark.parametrize("with_radiance", [True, False], ids=["radiance-and-pixels", "pixels-only"])
def test_host_form_on_a_rectangle_gives_the_device_form_s_bits_and_writes_nothing_outside(L, plain_scene, with_radiance):
    """terra_amd_denoise_variance on a rectangle that is no multiple of the 16 x 16 block, K = 3 (the taps of step 4 cross its edge), pixels of known and of unknown
    variance inside it; radiance may be NULL."""
    from terra_amd import runtime
    res, aov = synthetic(64, 48, 18)
    mom = synthetic_moments(res, 19)
    x, y, w, h = rect = (5, 3, 40, 30)
    inside = np.zeros((48, 64), bool); inside[y:y + h, x:x + w] = True
    known = (mom["batches"] >= 2) & (res["samples"] > 0)
    assert (known & inside).any() and (~known & inside & (res["samples"] > 0)).any()
    rad, pix = device_denoise_variance(L, plain_scene, res, aov, mom, 3, rect=rect)
    assert not np.array_equal(bits(rad[inside]), bits(device_denoise(L, plain_scene, res, aov, 3, rect=rect)[0][inside]))          # (the variance is in play)
    hfb = api.Framebuffer(L, 64, 48)
    np.copyto(hfb.results, res)
    hr, hp = np.full((48, 64, 3), -7.0, F), np.full((48, 64, 3), -7.0, F)
    runtime.check(L.denoise_variance(plain_scene, C.byref(hfb.fb), aov.ctypes.data, mom.ctypes.data, x, y, w, h, 3, hr.ctypes.data if with_radiance else None, hp.ctypes.data),
                  "terra_amd_denoise_variance")
    assert np.all(pix[inside] != F(-7.0))
    assert np.array_equal(bits(hp[inside]), bits(pix[inside])) and np.all(hp[~inside] == F(-7.0))
    if with_radiance:
        assert np.array_equal(bits(hr[inside]), bits(rad[inside])) and np.all(hr[~inside] == F(-7.0))
    else:
        assert np.all(hr == F(-7.0))
    hfb.destroy()


def test_a_quiet_pixel_rejects_a_firefly_neighbour(L, plain_scene):
    """constant image, 8 batches of 4 samples all equal -- except one pixel, one of whose batches is 1000 x. After K = 5 the eight neighbours deviate less from the
    constant than terra_amd_denoise_device leaves them on the same inputs."""
    h, w, c0 = 33, 33, F(0.5)
    res = np.zeros((h, w), api.RESULT_DTYPE)
    res["samples"] = 32; res["acc"] = c0 * F(32)
    mom = np.zeros((h, w), api.MOMENTS_DTYPE)
    mom["seen_acc"] = res["acc"]; mom["seen_samples"] = 32; mom["mean"] = c0; mom["batches"] = 8; mom["weight"] = 32
    y = x = 16
    bm = np.full(8, c0, np.float64); bm[3] = 1000.0 * c0
    res["acc"][y, x] = F(bm.sum() * 4)
    mom["seen_acc"][y, x] = res["acc"][y, x]; mom["mean"][y, x] = F(bm.mean()); mom["m2"][y, x] = F((4 * (bm - bm.mean()) ** 2).sum())
    aov = np.zeros((h, w), __import__("terra_amd.runtime", fromlist=["AOV_DTYPE"]).AOV_DTYPE)
    aov["coverage"] = 1; aov["albedo"] = 1.0; aov["normal"] = (0, 0, 1); aov["depth"] = 2.0; aov["samples"] = 32
    old, _ = device_denoise(L, plain_scene, res, aov, 5)
    new, _ = device_denoise_variance(L, plain_scene, res, aov, mom, 5)
    ring = np.zeros((h, w), bool); ring[y - 1:y + 2, x - 1:x + 2] = True; ring[y, x] = False
    dev_old, dev_new = np.abs(old[ring] - c0).max(), np.abs(new[ring] - c0).max()
    print(f"eight neighbours of the firefly, largest deviation from {c0}: a-trous {dev_old:.6g}, variance-guided {dev_new:.6g}; the firefly itself {old[y, x, 0]:.4g} -> {new[y, x, 0]:.4g}")
    assert dev_new < dev_old
    # the neighbours' tolerance is 1e-6 (their g_p is 0: the firefly's v is capped at 4 x 0), so its weight is exp(-5e8) = 0: what is left is the rounding of five
    # weighted means of (nearly) equal values, each 25 additions and a division of half an ulp at the most: 5 x 26 x eps / 2 relative
    assert dev_new <= 65 * np.finfo(F).eps * c0
    assert abs(new[y, x, 0] - c0) < abs(old[y, x, 0] - c0)          # ... and the firefly, whose tolerance is wide, takes its neighbours' value


def test_quality_cornell_direct_8_calls_of_1spp(L):
    """The scene and reference frame of tests/test_denoise.py::test_quality_cornell_direct_8spp, rendered as 8 calls of 1 spp with an accumulate after each. Against
    4096 spp at another seed: full-frame RMSE ratio, the ratio on the 99 % of the pixels whose noisy error is below its 99th percentile, and the mean, for the noisy
    frame, the a-trous filter and the variance-guided one.
    Measured on an MI355X (sigma_l = 8, cap 4): noisy RMSE 0.12518 (0.04369 on the 99 %), mean +0.41 %; a-trous 1.169 / 1.005 / +0.67 %; variance-guided 0.763 / 0.510 / -2.49 %.
    The goals full ratio < 1.0 and 99 % ratio no worse than the a-trous filter's are met; the goal |mean| <= 1 % is NOT, for any sigma_l from 1 to 16, with the cap or
    without (-1.8 % .. -3.7 %): a firefly takes its quiet neighbours' value and they reject its, so its excess is dropped. Asserted, as the issue
    sets it: the measurement plus the margin tests/test_denoise.py took over its own (full + 0.05, 99 % + 0.07, mean + 0.78 points), and in any case a full ratio
    below the a-trous filter's."""
    import torch
    from terra_amd import runtime
    s, fb, aov, dm = cornell_batches(L, 128, 128, 1, 8)
    r = fb.results_host()
    assert np.all(r["samples"] == 8)
    noisy = (r["acc"] / r["samples"][..., None]).astype(np.float64)
    outs = {}
    for name in ("a-trous", "variance"):
        rad = torch.zeros(128 * 128 * 3, dtype=torch.float32, device="cuda")
        if name == "a-trous":
            runtime.denoise_device(L, s, fb, aov, 5, radiance=rad)
        else:
            runtime.denoise_variance_device(L, s, fb, aov, dm, 5, radiance=rad)
        torch.cuda.synchronize()
        outs[name] = rad.cpu().numpy().reshape(128, 128, 3).astype(np.float64)
    d_ref = scenes.cornell_box(128, 128, 256, integrator=api.kTerraIntegratorDirect)
    sr = scenes.build_scene(L, d_ref)
    L.set_frame_seed(sr, 0xC0FFEE)
    fr = runtime.DeviceFramebuffer(128, 128)
    for _ in range(16):
        runtime.render_device(L, scenes.camera_of(d_ref), sr, fr)
    torch.cuda.synchronize()
    rr = fr.results_host()
    assert np.all(rr["samples"] == 4096)
    ref = (rr["acc"] / rr["samples"][..., None]).astype(np.float64)
    err = ((noisy - ref) ** 2).sum(-1)
    keep = err <= np.quantile(err, 0.99)
    rmse = lambda x, m=None: float(np.sqrt(np.mean(((x - ref) ** 2)[m] if m is not None else (x - ref) ** 2)))
    stats = {}
    print(f"noisy: RMSE {rmse(noisy):.5f}, on 99 % of the pixels {rmse(noisy, keep):.5f}, mean {noisy.mean() / ref.mean() - 1:+.4f}")
    for name, den in outs.items():
        stats[name] = (rmse(den) / rmse(noisy), rmse(den, keep) / rmse(noisy, keep), den.mean() / ref.mean() - 1)
        print(f"{name}: full ratio {stats[name][0]:.3f}, 99 % ratio {stats[name][1]:.3f}, mean {stats[name][2]:+.4f}")
        e2 = ((den - ref) ** 2).sum(-1)
        print(f"  share of the squared error in the worst 1 % / 0.1 % of the pixels: {np.sort(e2)[-164:].sum() / e2.sum():.3f} / {np.sort(e2)[-16:].sum() / e2.sum():.3f}")
    print(f"goals: full ratio < 1.0: {stats['variance'][0] < 1.0}; 99 % ratio no worse than a-trous: {stats['variance'][1] <= stats['a-trous'][1]}")
    print(f"goal |mean| <= 1 %: {abs(stats['variance'][2]) <= 0.01}")
    assert stats["variance"][0] < stats["a-trous"][0], stats
    assert stats["variance"][0] <= 0.813 and stats["variance"][1] <= 0.58 and abs(stats["variance"][2]) <= 0.0327, stats
    L.scene_destroy(s); L.scene_destroy(sr)
