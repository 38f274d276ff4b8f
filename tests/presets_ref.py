"""The GGX conductor and the dielectric glass of include/TerraPresets.h ("THE RULES"), restated in binary64 with numpy alone.

Written from the header's prose, not from the oracle: the straightforward formula in double precision, vectorised over rows. Inputs are the
binary32 values the device receives, widened to binary64 -- nothing is re-rounded on the way, no direction is re-normalised unless the rule says
so. Besides the results every function returns the quantities that say how well conditioned a row is, which the tests' tolerances are built on:

  den     = NoH^2 alpha^2 + 1 - NoH^2   (binary32 loses ~2^-23 / den of D, TerraPresets.h)
  cond    = min (NoL, NoV, HoV)         (h = normalize (wi + wo) and the 1 / (NoL NoV) lose ~2^-24 / cond)
  e3 - R, cos_t2                        (the glass branch decisions flip where these are within rounding of 0)
"""
import numpy as np

# "pi" in the rules is the library's terra_PI (include/TerraMath.h): the reference's constant 3.1416926535f, 1e-4 above pi. The azimuth 2 pi e2 and the
# normalisation of D both use it, so the stated pdf integrates to pi / terra_PI = 1 - 3.2e-5 over its lobe and the azimuth of e2 -> 1 overshoots a turn by 2e-4 rad.
PI = float(np.float32(3.1416926535))


def _w(a):
    """binary32 values, widened"""
    return np.asarray(a, np.float32).astype(np.float64)


def _dot(a, b):
    return np.einsum("nc,nc->n", a, b)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[:, None]


def basis_of(surfaces47):
    """the 3 x 3 transform of each surface record: rows of the row-major 4 x 4 at floats 0..15 (columns tangent, normal, bitangent)"""
    return _w(surfaces47)[:, :16].reshape(-1, 4, 4)[:, :3, :3]


def ggx_sample(basis, alpha, e1, e2, wo, widen=True):
    """(surface basis [n, 3, 3], alpha, e1, e2, wo) -> dict h, wi, clamped, HoV (signed, before the clamp). widen=False: the inputs are binary64 as they
    are (an integration lattice, not device inputs)"""
    w = _w if widen else (lambda x: np.asarray(x, np.float64))
    M, a, e1, e2, wo = np.asarray(basis, np.float64), w(alpha), w(e1), w(e2), w(wo)
    t2 = a * a * e1 / (1.0 - e1)
    cos_t = 1.0 / np.sqrt(1.0 + t2)
    sin_t = np.sqrt(t2) * cos_t
    phi = 2.0 * PI * e2
    local = np.stack([sin_t * np.cos(phi), cos_t, sin_t * np.sin(phi)], axis=1)
    h = _unit(np.einsum("nrc,nc->nr", M, local))
    hv = _dot(h, wo)
    wi = 2.0 * np.maximum(0.0, hv)[:, None] * h - wo
    return dict(h=h, wi=wi, clamped=~(hv > 0.0), HoV=hv)


def _ggx_terms(n, alpha, wi, wo):
    n, a, wi, wo = _w(n), _w(alpha), _w(wi), _w(wo)
    h = _unit(wi + wo)                              # NaN where wi = -wo
    with np.errstate(invalid="ignore"):
        NoH, HoV, NoL, NoV = _dot(n, h), _dot(h, wo), _dot(n, wi), _dot(n, wo)
        a2 = a * a
        den = NoH * NoH * a2 + (1.0 - NoH * NoH)
        D = np.where(NoH > 0.0, a2 / (PI * den * den), 0.0)
    return dict(n=n, a2=a2, wi=wi, wo=wo, h=h, NoH=NoH, HoV=HoV, NoL=NoL, NoV=NoV, den=den, D=D)


def _cond(t):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmin(t["NoL"], t["NoV"]), t["HoV"])


def ggx_pdf(n, alpha, wi, wo):
    """pdf at a GIVEN (wi, wo) -> dict pdf, den, cond, NoL, NoV, HoV, NoH"""
    t = _ggx_terms(n, alpha, wi, wo)
    with np.errstate(invalid="ignore", divide="ignore"):
        live = t["HoV"] > 0.0                        # False for NaN
        pdf = np.where(live, t["D"] * t["NoH"] / (4.0 * np.where(live, t["HoV"], 1.0)), 0.0)
    return dict(pdf=pdf, den=t["den"], cond=_cond(t), NoL=t["NoL"], NoV=t["NoV"], HoV=t["HoV"], NoH=t["NoH"])


def _g1(v, n, h, a2):
    with np.errstate(invalid="ignore", divide="ignore"):
        vh, vn = _dot(v, h), _dot(v, n)
        tan2 = (1.0 - vn * vn) / (vn * vn)
        return np.where(vh / vn > 0.0, 2.0 / (1.0 + np.sqrt(1.0 + a2 * tan2)), 0.0)


def ggx_eval(n, alpha, f0, wi, wo):
    """f at a GIVEN (wi, wo) -> dict f [n, 3], den, cond, NoL, NoV, HoV, NoH"""
    t = _ggx_terms(n, alpha, wi, wo)
    f0 = _w(f0)
    with np.errstate(invalid="ignore", divide="ignore"):
        live = (t["NoL"] > 0.0) & (t["NoV"] > 0.0)
        w5 = np.maximum(0.0, 1.0 - np.maximum(0.0, t["HoV"])) ** 5
        F = f0 + (1.0 - f0) * w5[:, None]
        G = _g1(t["wo"], t["n"], t["h"], t["a2"]) * _g1(t["wi"], t["n"], t["h"], t["a2"])
        k = G * t["D"] / (4.0 * t["NoL"] * t["NoV"])
        f = np.where(live[:, None], F * k[:, None], 0.0)
    return dict(f=f, den=t["den"], cond=_cond(t), NoL=t["NoL"], NoV=t["NoV"], HoV=t["HoV"], NoH=t["NoH"])


def glass_sample(n, ior, wo, e3):
    """(n, ior, wo, e3) -> dict inside (wo on the medium's side), tir, R (NaN under total internal reflection), reflect (the chosen branch), dir, prob,
    and the margins e3 - R and cos_t2 of the two decisions"""
    n, ior, wo, e3 = _w(n), _w(ior), _w(wo), _w(e3)
    i = -wo
    c = _dot(n, i)
    inside = c > 0.0
    n1 = np.where(inside, ior, 1.0); n2 = np.where(inside, 1.0, ior)
    N = np.where(inside[:, None], -n, n)
    cos_i = np.abs(c)
    refl = i - N * (2.0 * _dot(N, i))[:, None]
    nni = n1 / n2
    cos_t2 = 1.0 - nni * nni * (1.0 - cos_i * cos_i)
    tir = cos_t2 < 0.0
    cos_t = np.sqrt(np.where(tir, 0.0, cos_t2))
    x = np.where(n1 <= n2, cos_i, cos_t)
    R0 = ((n1 - n2) / (n1 + n2)) ** 2
    R = R0 + (1.0 - R0) * (1.0 - x) ** 5
    reflect = tir | (e3 < R)
    refr = _unit(N * (nni * cos_i - cos_t)[:, None] + i * nni[:, None])
    d = np.where(reflect[:, None], refl, refr)
    prob = np.where(tir, 1.0, np.where(reflect, R, 1.0 - R))
    return dict(inside=inside, tir=tir, R=np.where(tir, np.nan, R), R0=R0, reflect=reflect, dir=d, prob=prob, margin_R=np.where(tir, np.inf, e3 - R), cos_t2=cos_t2,
                mirror=refl)


# ---- Gauss-Legendre in cos(theta) x uniform azimuth about the normal: the quadrature of the normalisation and furnace tests -------------------------------------------

def hemisphere_nodes(basis3, n_cos=64, n_phi=128):
    """directions [n_cos * n_phi, 3] over the upper hemisphere of the ORTHONORMAL frame basis3 (columns tangent, normal, bitangent), their cos(theta) and their
    solid-angle weights (sum = 2 pi)"""
    x, w = np.polynomial.legendre.leggauss(n_cos)
    mu = 0.5 * (x + 1.0); wm = 0.5 * w                                  # cos(theta) in (0, 1)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    MU, PHI = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1.0 - MU * MU)
    local = np.stack([s * np.cos(PHI), MU, s * np.sin(PHI)], axis=-1).reshape(-1, 3)
    W = (wm[:, None] * np.full(n_phi, 2.0 * np.pi / n_phi)[None, :]).reshape(-1)
    return local @ np.asarray(basis3, np.float64).T, MU.reshape(-1), W
