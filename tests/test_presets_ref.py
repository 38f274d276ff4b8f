"""The GGX conductor and the dielectric glass against a binary64 statement of their rules (include/TerraPresets.h "THE RULES", tests/presets_ref.py).

These two presets have no reference behaviour, so until now the device was held only to the oracle -- the same formulas in the same binary32 order. Here the
oracle (CPU legs) and the device (gpu legs) are both held to presets_ref on edge rows (H.preset_edge_cases), at directions the sampler did not produce
(H.ggx_at_cases, Unit.bsdf_at), and the device to the oracle bit for bit on all of them.

TOLERANCES. Every constant below is the largest deviation of the CPU oracle (the binary32 statement of the rule) from presets_ref on the rows of this module,
DOUBLED because other rows land differently in the last bits. `python tests/test_presets_ref.py` prints the measured values again.

GGX pdf / eval at a given (wi, wo), rows with NoL, NoV, HoV > 0.01, relative:   (A / den + C / cond + B [+ FZ * fres]) * 2^-23
    den  = NoH^2 alpha^2 + 1 - NoH^2 (D's cancelling sum),  cond = min (NoL, NoV, HoV)  (h = normalize (wi + wo), 1 / (NoL NoV))
    fres = 5 (1 - F0) m^4 / F, m = 1 - HoV: the condition number of Schlick's F = F0 + (1 - F0) m^5 in m, eval only. Without it no relative bound holds on the
           F0 = 0 rows: F = m^5 there, m = 1 - HoV carries the absolute error of HoV, and m -> 0 as wi nears the mirror direction of a wo near n.
           It is a linearisation in m, so rows where it alone reaches 0.1 (F0 = 0 with m < ~1e-5), and rows where the whole bound reaches 1 (alpha = 0.001
           at the peak), are held to "finite and >= 0" only.
    measured  B 5.022 (rows with den, cond > 0.5)   C 1.065 (den > 0.5)   A 12.640 (all; pdf, and eval where fres <= 1)   FZ 1.063 (eval where fres > 1)
GGX sampler, rows not clamped with h.wo > 0.1, absolute per component of wi:   measured 4.39 * 2^-23 (5.23e-7)
Glass, absolute: prob and direction, apart for rows with cos_t2 >= 0.01 and for rows nearer the critical angle (cos_t = sqrt (cos_t2) loses 2^-24 / cos_t there)
    measured  prob 2.09e-7 / 6.87e-5    direction 1.86e-7 / 1.48e-5
"""
import functools

import numpy as np
import pytest

import presets_ref as P

EPS = 2.0 ** -23
GGX_A, GGX_B, GGX_C, GGX_FZ = 2 * 12.640, 2 * 5.022, 2 * 1.065, 2 * 1.063
GGX_WI_TOL = 2 * 4.39 * EPS
GLASS_WELL = 0.01                                       # cos_t2 from which a row counts as away from the critical angle
GLASS_PROB_TOL = (2 * 2.09e-7, 2 * 6.87e-5)             # (cos_t2 >= GLASS_WELL or total internal reflection far from it, nearer the critical angle)
GLASS_DIR_TOL = (2 * 1.86e-7, 2 * 1.48e-5)
CUT = 0.01
FRES_LINEAR = 0.1                                       # the Fresnel term is a linearisation in m = 1 - HoV: rows where it reaches this are not held to the bound
QUADRATURE = [(a, nov) for a in (0.1, 0.3, 0.9) for nov in (1.0, 0.7)]


def _harness():
    import harness
    return harness


# ---- rows (made once, shared, never modified) ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ggx_at_rows():
    """every row on which GGX pdf / eval are evaluated at a given direction: the off-sample directions of each alpha, then the edge rows at the direction the
    reference sampler gives them (rounded to binary32 once)"""
    H = _harness()
    parts = [H.ggx_at_cases(a)[:3] for a in H.GGX_EDGE_ALPHAS]
    opposite = np.concatenate([H.ggx_at_cases(a)[3]["opposite"] for a in H.GGX_EDGE_ALPHAS])
    surf, e, wo, _ = H.preset_edge_cases(2)
    wi = P.ggx_sample(P.basis_of(surf), surf[:, 26], e[:, 0], e[:, 1], wo)["wi"].astype(np.float32)
    parts.append((surf, wi, wo))
    surf, wi, wo = [np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(3)]
    opposite = np.concatenate([opposite, np.zeros(len(surf) - len(opposite), bool)])
    for a in (surf, wi, wo, opposite):
        a.setflags(write=False)
    return surf, wi, wo, opposite


@functools.lru_cache(maxsize=None)
def quadrature_rows():
    """the 64 x 128 Gauss-Legendre x azimuth nodes about n = +y for each (alpha, NoV) of QUADRATURE: surfaces (F0 = 1), wi, wo, cos(theta), weights"""
    H = _harness()
    out = []
    nrm = np.array([[0, 1, 0]], np.float32)
    basis = P.basis_of(H._surfaces_of(nrm))[0]
    assert np.allclose(basis @ basis.T, np.eye(3), atol=0)           # an axis normal: the frame is orthonormal, exactly
    for a, nov in QUADRATURE:
        wi, mu, w = P.hemisphere_nodes(basis)
        surf = np.repeat(H._surfaces_of(nrm), len(wi), axis=0)
        surf[:, 23:26] = 1; surf[:, 26:29] = np.float32(a)
        wo = np.repeat(np.array([[np.sqrt(1 - nov * nov), nov, 0]], np.float32), len(wi), axis=0)
        out.append((np.ascontiguousarray(surf), np.ascontiguousarray(wi, np.float32), np.ascontiguousarray(wo), mu, w))
    return out


def ggx_tolerance(ref, f0=None):
    """relative tolerance per row (pdf) or per row and channel (eval, f0 given); inf where the row is under the cut or the bound reaches 1"""
    with np.errstate(all="ignore"):
        base = GGX_A / ref["den"] + GGX_C / ref["cond"] + GGX_B
        if f0 is not None:
            f0 = f0.astype(np.float64)
            m = np.maximum(0.0, 1.0 - ref["HoV"])
            F = f0 + (1.0 - f0) * (m ** 5)[:, None]
            fres = GGX_FZ * 5.0 * (1.0 - f0) * (m ** 4)[:, None] / np.where(F > 0, F, 1.0) + np.where(F > 0, 0.0, np.inf)
            base = base[:, None] + np.where(fres * EPS < FRES_LINEAR, fres, np.inf)
        tol = base * EPS
        live = (ref["NoL"] > CUT) & (ref["NoV"] > CUT) & (ref["HoV"] > CUT)
        live = live if f0 is None else live[:, None]
        return np.where(live & (tol < 1.0), tol, np.inf)


def check_ggx_at(U, surf, wi, wo, opposite=None):
    """pdf / eval of backend U at (wi, wo) against binary64, and the exact expectations of the rule"""
    pdf, f = U.bsdf_at(2, surf, wi, wo)
    n, al, f0 = surf[:, 16:19], surf[:, 26], surf[:, 23:26]
    rp, rf = P.ggx_pdf(n, al, wi, wo), P.ggx_eval(n, al, f0, wi, wo)
    # every output finite and >= 0, on every row (under the cut too)
    assert np.isfinite(pdf).all() and np.isfinite(f).all() and (pdf >= 0).all() and (f >= 0).all()
    tp, tf = ggx_tolerance(rp), ggx_tolerance(rf, f0)
    with np.errstate(all="ignore"):
        ep = np.abs(pdf - rp["pdf"]) / rp["pdf"]; ef = np.abs(f - rf["f"]) / rf["f"]
    held_p, held_f = np.isfinite(tp), np.isfinite(tf)
    print(f"GGX at: {len(pdf)} rows, held to the bound: pdf {held_p.sum()}, eval {held_f.sum()} channel values; worst error / bound: pdf {np.max(ep[held_p] / tp[held_p]):.3f} eval {np.max(ef[held_f] / tf[held_f]):.3f}")
    assert held_p.sum() > 0.5 * len(pdf)
    assert (ep[held_p] <= tp[held_p]).all()
    assert (ef[held_f] <= tf[held_f]).all()
    # eval is 0 off the upper hemisphere -- decided on the binary32 dot products the rule names, so no tolerance
    f32 = np.float32
    dots = lambda a, b: ((a[:, 0] * b[:, 0]).astype(f32) + (a[:, 1] * b[:, 1]).astype(f32)).astype(f32) + (a[:, 2] * b[:, 2]).astype(f32)
    off = (dots(n, wi) <= 0) | (dots(n, wo) <= 0)
    assert not f[off].any()
    if opposite is not None:
        assert off.sum() > 100 and opposite.any() and not pdf[opposite].any() and not f[opposite].any()          # wi = -wo: the sampler's clamp. pdf was NaN here
    return pdf, f, rp, rf


def check_ggx_sampler(U, H):
    surf, e, wo, lab = H.preset_edge_cases(2)
    wi, pdf, f, _ = U.bsdf(2, surf, e, wo)
    assert np.isfinite(wi).all() and np.isfinite(pdf).all() and np.isfinite(f).all() and (pdf >= 0).all() and (f >= 0).all()
    s = P.ggx_sample(P.basis_of(surf), surf[:, 26], e[:, 0], e[:, 1], wo)
    # the clamp decision: rows may differ only where h.wo is within the tolerance of 0, and at most 1 % of them
    clamped = np.all(wi == -wo, axis=1)
    differ = clamped != s["clamped"]
    assert s["clamped"].sum() > 100 and (~s["clamped"]).sum() > 1000
    assert (np.abs(s["HoV"][differ]) < GGX_WI_TOL).all() and differ.mean() <= 0.01
    assert not pdf[clamped].any() and not f[clamped].any()
    use = ~s["clamped"] & (s["HoV"] > 0.1)
    dev = np.abs(wi.astype(np.float64) - s["wi"])[use]
    print(f"GGX sampler: {use.sum()} rows, worst |wi - ref| {dev.max():.3g} = {dev.max() / EPS:.2f} * 2^-23 (bound {GGX_WI_TOL / EPS:.2f}); clamped {clamped.sum()}, decisions that differ {differ.sum()}")
    assert use.sum() > 3000 and (dev <= GGX_WI_TOL).all()
    # e1 = 0: h = n and wi is wo mirrored about n. On an axis normal every step of that is exact in binary32: the components across n change sign, the one along n stays
    axis = (e[:, 0] == 0) & (np.abs(surf[:, 16:19]).max(axis=1) == 1) & ~clamped
    along = np.abs(surf[:, 16:19]) == 1
    assert axis.sum() >= 20 and np.array_equal(wi[axis], np.where(along[axis], wo[axis], -wo[axis]))
    z = (e[:, 0] == 0) & ~s["clamped"]
    n64, wo64 = surf[:, 16:19].astype(np.float64), wo.astype(np.float64)
    nn = n64 / np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(wi[z] - (2 * np.einsum("nc,nc->n", nn, wo64)[:, None] * nn - wo64)[z]).max() <= GGX_WI_TOL


def check_quadrature(U):
    """the backend's pdf at the quadrature nodes under the pointwise bound; its eval's furnace integral with F0 = 1"""
    for (a, nov), (surf, wi, wo, mu, w) in zip(QUADRATURE, quadrature_rows()):
        pdf, f, rp, rf = check_ggx_at(U, surf, wi, wo)
        furnace = float(np.sum(f[:, 0].astype(np.float64) * mu * w))
        print(f"alpha {a} NoV {nov}: sum pdf w = {np.sum(pdf.astype(np.float64) * w):.5f}, furnace {furnace:.5f}")
        assert furnace <= 1 + 1e-3


def check_reciprocity(U):
    surf, wi, wo, _ = ggx_at_rows()
    _, f1 = U.bsdf_at(2, surf, wi, wo)
    _, f2 = U.bsdf_at(2, surf, wo, wi)
    tol = 2 * ggx_tolerance(P.ggx_eval(surf[:, 16:19], surf[:, 26], surf[:, 23:26], wi, wo), surf[:, 23:26])
    held = np.isfinite(tol)
    with np.errstate(all="ignore"):
        err = np.abs(f1.astype(np.float64) - f2) / np.maximum(f1, f2)
    err = np.where(f1 == f2, 0.0, err)
    print(f"reciprocity: {held.sum()} channel values, worst error / bound {np.max(err[held] / tol[held]):.3f}")
    assert held.sum() > 10000 and (err[held] <= tol[held]).all()


def ulps(a, b):
    return np.abs(np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64))


def check_glass(U, H):
    surf, e, wo, lab = H.preset_edge_cases(3)
    wi, pdf, f, after = U.bsdf(3, surf, e, wo)
    n, ior, tint = surf[:, 16:19], surf[:, 22], surf[:, 23:26]
    g = P.glass_sample(n, ior, wo, e[:, 2])
    assert np.isfinite(wi).all() and np.isfinite(pdf).all() and np.isfinite(f).all() and (pdf > 0).all() and (pdf <= 1).all()
    near = np.abs(g["cos_t2"]) < GLASS_WELL
    ptol = np.where(near, GLASS_PROB_TOL[1], GLASS_PROB_TOL[0]); dtol = np.where(near, GLASS_DIR_TOL[1], GLASS_DIR_TOL[0])
    # the branch decisions -- side, total internal reflection, reflect or refract -- as the backend's outputs show them. A row may differ from the reference only
    # where the reference's own margin (e3 - R, cos_t2) is under the tolerance on R, and at most 1 % of the rows
    cos_o, cos_i = np.einsum("nc,nc->n", wo, n), np.einsum("nc,nc->n", wi, n)
    tangent = lab["tangent"]
    reflected = np.where(tangent, True, (cos_o > 0) == (cos_i > 0))
    differ = (reflected != g["reflect"]) | (g["tir"] & (pdf != 1))
    slack = (np.abs(g["margin_R"]) < ptol) | (np.abs(g["cos_t2"]) < ptol)
    print(f"glass: {len(wi)} rows, total internal reflection {g['tir'].sum()}, reflect {g['reflect'].sum()}, decisions that differ {differ.sum()}, rows within the tolerance of a decision {slack.sum()}")
    assert g["tir"].sum() > 500 and (g["reflect"] & ~g["tir"]).sum() > 500 and (~g["reflect"]).sum() > 500 and g["inside"].sum() > 1000 and (~g["inside"]).sum() > 1000
    assert slack[differ].all() and differ.mean() <= 0.01
    same = ~differ
    dp = np.abs(pdf - g["prob"]); dd = np.abs(wi.astype(np.float64) - g["dir"]).max(axis=1)
    for name, m in (("away from", ~near), ("near", near)):
        print(f"   {name} the critical angle: {(same & m).sum()} rows, worst |prob - ref| {dp[same & m].max():.3g}, |dir - ref| {dd[same & m].max():.3g}")
    assert (dp[same] <= ptol[same]).all() and (dd[same] <= dtol[same]).all()
    # total internal reflection: probability 1, the mirror direction
    t = g["tir"] & same
    assert (pdf[t] == 1).all() and (np.abs(wi[t] - g["mirror"][t]).max(axis=1) <= dtol[t]).all()
    # wo = +-n and ior = 1: what is transmitted goes along -wo
    straight = (lab["wo_kind"] == 0) & ~g["reflect"] & same
    assert straight.sum() > 100 and (np.abs(wi[straight] + wo[straight]).max(axis=1) <= dtol[straight]).all()
    one = (ior == 1) & same
    assert (g["R0"][one] == 0).all()
    one &= ~g["reflect"]
    assert one.sum() > 100 and (np.abs(wi[one] + wo[one]).max(axis=1) <= dtol[one]).all()
    # the two branches of one surface: rows 8 k (e3 = 0) and 8 k + 1 (e3 = 1 - 2^-24) share everything else
    assert np.array_equal(lab["group"][0::8], lab["group"][1::8]) and not e[0::8, 2].any() and (e[1::8, 2] == H.U24_MAX).all()
    pair = g["reflect"][0::8] & ~g["reflect"][1::8] & same[0::8] & same[1::8]
    assert pair.sum() > 100 and ((pdf[0::8] + pdf[1::8]).astype(np.float32)[pair] == 1).all()
    # the path weight f (n.wi) / pdf is the tint (in binary32, as terra_trace multiplies it), except in the surface's plane where eval is 0 and the path dies
    flat = cos_i.astype(np.float32) == 0
    assert flat[tangent].all() and not f[flat].any()
    weight = ((f * cos_i.astype(np.float32)[:, None]).astype(np.float32) / pdf[:, None]).astype(np.float32)
    print(f"   path weight: worst distance to the tint {ulps(weight[~flat], tint[~flat]).max()} ulp; rows in the surface's plane {flat.sum()}")
    assert (ulps(weight[~flat], tint[~flat]) <= 4).all()
    # a delta lobe, through bsdf_at on the surfaces bsdf returned: at the sampled direction pdf and f are the ones bsdf gave; one ulp beside it, and at 64 random
    # directions, both are exactly 0
    p2, f2 = U.bsdf_at(3, after, wi, wo)
    assert H.same_bits(p2, pdf) and H.same_bits(f2, f)
    k = np.argmax(np.abs(wi), axis=1)
    beside = wi.copy()
    beside[np.arange(len(wi)), k] = np.nextafter(wi[np.arange(len(wi)), k], np.float32(0))
    assert (beside != wi).any(axis=1).all()
    p3, f3 = U.bsdf_at(3, after, beside, wo)
    assert not p3.any() and not f3.any()
    pick = np.arange(0, len(wi), max(1, len(wi) // 96))[:96]
    other = H.unit_dirs(H.rng(4301), 64)
    p4, f4 = U.bsdf_at(3, np.repeat(after[pick], 64, axis=0), np.tile(other, (len(pick), 1)), np.repeat(wo[pick], 64, axis=0))
    assert not p4.any() and not f4.any()
    # a surface no sample has touched (scratch probability 0) has no lobe at all
    p5, f5 = U.bsdf_at(3, surf, wi, wo)
    assert not p5.any() and not f5.any()


# ---- CPU legs: the oracle against binary64, and the reference alone -------------------------------------------------------------------------------------

def test_oracle_ggx_pdf_and_eval_at_given_directions(H, orc_lib):
    check_ggx_at(H.Unit("orc"), *ggx_at_rows())


def test_oracle_ggx_sampler(H, orc_lib):
    check_ggx_sampler(H.Unit("orc"), H)


def test_oracle_ggx_quadrature_nodes_and_furnace(H, orc_lib):
    check_quadrature(H.Unit("orc"))


def test_oracle_ggx_reciprocity(H, orc_lib):
    check_reciprocity(H.Unit("orc"))


def test_oracle_glass(H, orc_lib):
    check_glass(H.Unit("orc"), H)


@pytest.mark.parametrize("alpha,nov", QUADRATURE)
def test_stated_pdf_is_the_density_of_the_stated_sampler(H, alpha, nov):
    """presets_ref alone: the stated pdf integrated over the upper hemisphere is what the stated sampler puts there -- 1 minus the mass it clamps to wi = -wo
    (pdf 0) and the mass it sends below the horizon, both counted on a 512 x 512 stratified (e1, e2) lattice. (NoV = 0.2 is left out: this quadrature has not
    converged there.) pi / terra_PI = 1 - 3.2e-5 is inside the 1e-3."""
    i = QUADRATURE.index((alpha, nov))
    surf, wi, wo, mu, w = quadrature_rows()[i]
    basis = P.basis_of(surf[:1])[0]
    total = float(np.sum(P.ggx_pdf(surf[:, 16:19], surf[:, 26], wi, wo)["pdf"] * w))
    u = (np.arange(512) + 0.5) / 512
    E1, E2 = [x.reshape(-1) for x in np.meshgrid(u, u, indexing="ij")]
    s = P.ggx_sample(np.broadcast_to(basis, (len(E1), 3, 3)), np.full(len(E1), alpha), E1, E2, np.broadcast_to(wo[0], (len(E1), 3)), widen=False)
    clamped = float(s["clamped"].mean())
    below = float((~s["clamped"] & (s["wi"] @ surf[0, 16:19].astype(np.float64) <= 0)).mean())
    print(f"alpha {alpha} NoV {nov}: sum pdf w = {total:.5f}; sampler: clamped {clamped:.5f}, below the horizon {below:.5f}, so {1 - clamped - below:.5f}")
    assert abs(total - (1 - clamped - below)) <= 1e-3


@pytest.mark.parametrize("roughness", [0.9, 0.3])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_oracle_plate_scene_is_finite(H, orc_lib, devmath_mode, roughness, integ):
    """a GGX plate under the light, Direct + MIS: the sampler's clamped wi = -wo made ggx_pdf NaN, NaN passed the integrator's `bpdf != 0`, and 0 * NaN reached
    the framebuffer (33 pixels at roughness 0.9, 9 at 0.3)"""
    got = H.Unit("orc").render_pixels(H.ggx_plate_scene(roughness, integ))
    assert np.isfinite(got["pixels"]).all() and np.isfinite(got["acc"]).all()
    assert got["pixels"].mean() > 0.01


# ---- GPU legs: the device against binary64 and against the oracle, bit for bit ---------------------------------------------------------------------------

def same_bits_nan(H, x, y):
    """the NaN-ness rule of test_device_bsdf_matches_oracle"""
    return np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(H.bits(x)[~np.isnan(x)], H.bits(y)[~np.isnan(y)])


@pytest.mark.gpu
def test_device_ggx_pdf_and_eval_at_given_directions(H, orc_lib, amd_lib):
    rows = ggx_at_rows()
    pdf, f, _, _ = check_ggx_at(H.Unit("amd"), *rows)
    want = H.Unit("orc").bsdf_at(2, *rows[:3])
    assert same_bits_nan(H, pdf, want[0]) and same_bits_nan(H, f, want[1])


@pytest.mark.gpu
def test_device_ggx_sampler(H, amd_lib):
    check_ggx_sampler(H.Unit("amd"), H)


@pytest.mark.gpu
def test_device_ggx_quadrature_nodes_and_furnace(H, amd_lib):
    check_quadrature(H.Unit("amd"))


@pytest.mark.gpu
def test_device_ggx_reciprocity(H, amd_lib):
    check_reciprocity(H.Unit("amd"))


@pytest.mark.gpu
def test_device_glass(H, amd_lib):
    check_glass(H.Unit("amd"), H)


@pytest.mark.gpu
@pytest.mark.parametrize("kind_id", [2, 3])
def test_device_matches_oracle_on_the_edge_rows(H, orc_lib, amd_lib, kind_id):
    """bsdf (sample, then pdf and eval there) and bsdf_at (the surfaces bsdf left, the sampled direction and, for glass, one beside it) bit for bit"""
    surf, e, wo, _ = H.preset_edge_cases(kind_id)
    a, b = H.Unit("amd").bsdf(kind_id, surf, e, wo), H.Unit("orc").bsdf(kind_id, surf, e, wo)
    for x, y in zip(a[:3], b[:3]):
        assert same_bits_nan(H, x, y)
    assert H.same_bits(a[3][:, 29:33], b[3][:, 29:33])
    wi = b[0]
    for d in (wi, np.roll(wi, 1, axis=0)):
        x, y = H.Unit("amd").bsdf_at(kind_id, b[3], d, wo), H.Unit("orc").bsdf_at(kind_id, b[3], d, wo)
        assert same_bits_nan(H, x[0], y[0]) and same_bits_nan(H, x[1], y[1])


@pytest.mark.gpu
@pytest.mark.parametrize("roughness", [0.9, 0.3])
@pytest.mark.parametrize("integ", [0, 1, 2])
def test_device_plate_scene_matches_oracle(H, orc_lib, amd_lib, devmath_mode, roughness, integ):
    from test_gpu_render import render_dev, render_host
    from terra_amd import runtime
    L = runtime.load()
    d = H.ggx_plate_scene(roughness, integ)
    want = H.Unit("orc").render_pixels(d)
    got = render_dev(L, d, calls=True)
    assert np.array_equal(got["rand_calls"], want["rand_calls"])
    assert H.same_bits(got["pixels"], want["pixels"]) and H.same_bits(got["acc"], want["acc"])
    assert H.same_bits(render_host(L, d)["pixels"], want["pixels"])
    assert np.isfinite(got["pixels"]).all() and np.isfinite(got["acc"]).all()


# ---- the measurement the constants above come from -------------------------------------------------------------------------------------------------------

def measure():
    H = _harness()
    U = H.Unit("orc")
    surf, wi, wo, _ = ggx_at_rows()
    pdf, f = U.bsdf_at(2, surf, wi, wo)
    n, al, f0 = surf[:, 16:19], surf[:, 26], surf[:, 23:26].astype(np.float64)
    rp, rf = P.ggx_pdf(n, al, wi, wo), P.ggx_eval(n, al, surf[:, 23:26], wi, wo)
    live = (rp["NoL"] > CUT) & (rp["NoV"] > CUT) & (rp["HoV"] > CUT)
    with np.errstate(all="ignore"):
        m = np.maximum(0, 1 - rp["HoV"]); F = f0 + (1 - f0) * (m ** 5)[:, None]
        fres = (5 * (1 - f0) * (m ** 4)[:, None] / F)[live]
        r_pdf = (np.abs(pdf - rp["pdf"]) / rp["pdf"] / EPS)[live]; r_f = (np.abs(f - rf["f"]) / rf["f"] / EPS)[live]
    den, cond = rp["den"][live], rp["cond"][live]
    free = fres <= 1                                                          # Schlick's F no worse conditioned than a product (F0 = 1: F is exactly 1)
    r = np.concatenate([r_pdf, r_f[free]]); d = np.concatenate([den, np.broadcast_to(den[:, None], free.shape)[free]]); c = np.concatenate([cond, np.broadcast_to(cond[:, None], free.shape)[free]])
    B = r[(d > 0.5) & (c > 0.5)].max(); C = max(0.0, ((r - B) * c)[d > 0.5].max()); A = max(0.0, ((r - B - C / c) * d).max())
    with np.errstate(all="ignore"):
        q = (r_f - (A / den + C / cond + B)[:, None]) / fres
    FZ = np.max(np.where(np.isfinite(q) & (fres > 1) & (fres * EPS <= 0.02), q, 0.0))      # where the linearisation in m holds: the rows the tests hold to it
    print(f"GGX at {live.sum()} rows: B {B:.3f} C {C:.3f} A {A:.3f} FZ {FZ:.3f}")
    check_ggx_sampler(U, H); check_glass(U, H)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    measure()
