"""Point rendering on the GPU (include/terra_amd.h "Point rendering"): terra_amd_render_points* / terra_amd_render_aov_points* / terra_amd_unit_point_rays pinned by a
chain onto the ray door, which is itself pinned to the oracle and to the camera door:

  1. the generator (terra_amd_unit_point_rays) equals a numpy restatement of the header's definition bit for bit, inactive points give the all-zero record;
  2. its directions have the geometry the distributions promise (means on the 64 x 64 midpoint grid against a float64 evaluation, unit length, the hemisphere, an
     orthonormal frame);
  3. a points call cut into one-sample chunks equals as many 1 spp ray-door calls whose rays the host made with the generator from the chunks' stream-A draws;
  4. a chunk of several samples advances stream A as specified (r1 r2, the sampler integration's pair, then g1 g2);
  5. the point AOV pass equals the ray-door AOV pass of the same rays; 6. host form = device form, and the camera_limit rule; 7. a sky furnace and
  runtime.irradiance; 8. the denoiser and the moments accept a points frame.

Frames are 48 x 32, whole and as the rectangle (5, 3, 37, 25) -- partial blocks on every side."""
import ctypes as C
import math

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, HGT = 48, 32
RECT = (5, 3, 37, 25)
RECTS = [None, RECT]
CALL_REPLICA = 1
PI2, PI4, TWO_PI = (np.array([b], np.uint32).view(F)[0] for b in (0x3FC90FDB, 0x3F490FDB, 0x40C90FDB))
NAN, INF = float("nan"), float("inf")
DISTRIBUTIONS = [0, 1]
DIST_IDS = ["cosine", "sphere"]
# the pairs that reach every branch of the concentric map (tests/test_lens_gpu.py): a = b = 0; |a| = |b| (both signs); a = 0; b = 0
SPECIAL_PAIRS = [(0.5, 0.5), (0.75, 0.75), (0.25, 0.75), (0.5, 0.3), (0.3, 0.5)]


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def make_scene(L, d, tree_mode=None, split=1):
    L.clear_error()
    s = scenes.build_scene(L, d, tree_mode=tree_mode)
    assert runtime.last_error() == "", runtime.last_error()
    runtime.check(L.set_sample_split(s, split))
    return s


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Frame:
    """a device framebuffer with its per-pixel draw counts"""

    def __init__(self, w=W, h=HGT):
        import torch
        self.fb = runtime.DeviceFramebuffer(w, h)
        self.calls = torch.full((h * w,), 0x5ca1ab1e, dtype=torch.int32, device="cuda")

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.fb.pixels_host().copy(), self.fb.results_host().copy(), self.calls.cpu().numpy().reshape(self.fb.height, self.fb.width).copy()


def assert_same_frames(H, a, b, what):
    (pa, ra, ca), (pb, rb, cb) = a, b
    assert np.array_equal(ra["samples"], rb["samples"]), what
    assert H.same_bits(ra["acc"], rb["acc"]), what
    assert H.same_bits(pa, pb), what
    assert np.array_equal(ca, cb), what


def last_call(L, s):
    ti = runtime.TraversalInfo()
    runtime.check(L.traversal_info(s, C.byref(ti)))
    return ti.last_call


def points_of(positions, normals):
    """[n, 8] float32 TerraAmdPoint records"""
    p = np.zeros((len(positions), 8), F)
    p[:, 0:3] = positions
    p[:, 4:7] = normals
    return p


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------------------------------------
def dev_math(L, fn, x):
    """terra_amd_unit_math: fn 0 = the device's sinf, 1 = its cosf"""
    x = np.ascontiguousarray(x, F)
    out = np.zeros_like(x)
    rc = L.fn("terra_amd_unit_math", C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])(fn, len(x), x.ctypes.data, None, out.ctypes.data)
    assert rc == 0, runtime.last_error()
    return out


def inactive_mask(points):
    """the header's "inactive point", in binary32"""
    p = np.ascontiguousarray(points, F)
    with np.errstate(all="ignore"):
        finite = np.isfinite(p[:, 0:3]).all(axis=1) & np.isfinite(p[:, 4:7]).all(axis=1)
        q = p[:, 4] * p[:, 4] + p[:, 5] * p[:, 5] + p[:, 6] * p[:, 6]
        return ~finite | ~((q > 0) & np.isfinite(q))


def restate(distribution, points, g, T=F, sin=None, cos=None):
    """the header's "ray of a sample" in numpy, every operation in the order written, in the type T (float32: the definition; float64: the same formulas, for the
    geometry test); sin / cos: the device's for T = float32. Returns (origins, directions, t, bt, n) -- active points only make sense"""
    p = np.ascontiguousarray(points, T)
    g1, g2 = np.ascontiguousarray(g[:, 0], T), np.ascontiguousarray(g[:, 1], T)
    one, two, zero = T(1), T(2), T(0)

    def normalize(v):
        ln = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return [v[0] / ln, v[1] / ln, v[2] / ln]
    with np.errstate(all="ignore"):
        n = normalize([p[:, 4], p[:, 5], p[:, 6]])
        s = np.copysign(one, n[2]).astype(T)
        a = -one / (s + n[2])
        b = (n[0] * n[1]) * a
        t = [one + (s * (n[0] * n[0])) * a, s * b, (-s) * n[0]]
        bt = [b, s + (n[1] * n[1]) * a, -n[1]]
        if distribution == 0:
            ca, cb = two * g1 - one, two * g2 - one
            origin = (ca == 0) & (cb == 0)
            wide = np.abs(ca) > np.abs(cb)
            r = np.where(wide, ca, cb)
            phi = np.where(wide, T(PI4) * (cb / ca), T(PI2) - T(PI4) * (ca / cb))
            phi = np.where(origin, zero, phi).astype(T)
            x = np.where(origin, zero, r * cos(phi)).astype(T)
            y = np.where(origin, zero, r * sin(phi)).astype(T)
            z = np.sqrt(np.maximum(zero, (one - x * x) - y * y))
        else:
            z = one - two * g1
            r = np.sqrt(np.maximum(zero, one - z * z))
            phi = T(TWO_PI) * g2
            x, y = r * cos(phi), r * sin(phi)
        d = normalize([(x * t[k] + y * bt[k]) + z * n[k] for k in range(3)])
    stack = lambda v: np.stack(v, axis=1).astype(T)          # noqa: E731
    return p[:, 0:3].copy(), stack(d), stack(t), stack(bt), stack(n)


def restate32(L, distribution, points, g):
    return restate(distribution, points, g, F, lambda x: dev_math(L, 0, x), lambda x: dev_math(L, 1, x))


G1_MAX = np.nextafter(F(1), F(0))          # the largest draw: 1 - 2^-24
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, -0.0), (0, 1, -0.0), (-0.6, 0.8, -0.0)]


def generator_inputs(H):
    """(points [n, 8], g [n, 2]): every special normal with every special pair; random unnormalised normals -- as they are and scaled by 2^20 and 2^-20 -- with random
    pairs, g1 = 0 and the largest draw among them; 3,000 random ones after the specials"""
    r = H.rng(11)
    special_g = SPECIAL_PAIRS + [(0.0, 0.37), (float(G1_MAX), 0.61), (0.0, 0.0), (float(G1_MAX), float(G1_MAX)), (0.1, 0.9), (0.97, 0.4)]
    normals, pairs = [], []
    for ax in AXES:
        for pr in special_g:
            for scale in (1.0, 2.0 ** 20, 2.0 ** -20):
                normals.append(np.array(ax, F) * F(scale)); pairs.append(pr)
    n_rand = 3000
    rn = r.normal(size=(n_rand, 3)).astype(F) * r.uniform(0.2, 3.0, size=(n_rand, 1)).astype(F)
    rn[1000:2000] *= F(2.0 ** 20); rn[2000:3000] *= F(2.0 ** -20)
    rg = r.uniform(size=(n_rand, 2)).astype(F)
    rg[::50, 0] = 0.0; rg[25::50, 0] = G1_MAX
    for k, pr in enumerate(SPECIAL_PAIRS):
        rg[7 + 100 * k] = pr
    normals = np.concatenate([np.array(normals, F), rn])
    g = np.concatenate([np.array(pairs, F), rg])
    positions = r.uniform(-2, 2, size=(len(normals), 3)).astype(F)
    return points_of(positions, normals), g


@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
def test_generator_equals_the_numpy_restatement(H, L, distribution):
    points, g = generator_inputs(H)
    assert len(points) >= 3000 and not inactive_mask(points).any()
    # both arms and the centre of the concentric map are among the inputs
    a, b = F(2) * g[:, 0] - F(1), F(2) * g[:, 1] - F(1)
    assert ((a == 0) & (b == 0)).any() and (np.abs(a) > np.abs(b)).sum() > 1000 and ((np.abs(a) <= np.abs(b)) & ~((a == 0) & (b == 0))).sum() > 1000
    assert (np.signbit(points[:, 6]) & (points[:, 6] == 0)).any() and ((points[:, 6] == -1) & (points[:, 4] == 0) & (points[:, 5] == 0)).any()
    got = runtime.point_rays(L, runtime.point_sampling(distribution), points, g)
    o, d, _, _, _ = restate32(L, distribution, points, g)
    assert np.isfinite(d).all()
    assert H.same_bits(got["origin"], o)
    bad = np.flatnonzero((got["direction"].view(np.uint32) != d.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], points[bad[:5]], g[bad[:5]], got["direction"][bad[:5]], d[bad[:5]])
    assert (got["tmax"] == np.finfo(F).max).all() and not got["reserved"].view(np.uint32).any()


INACTIVE_POINTS = {
    "nan position x": ((NAN, 0, 0), (0, 1, 0)), "inf position y": ((0, INF, 0), (0, 1, 0)), "-inf position z": ((0, 0, -INF), (0, 1, 0)),
    "nan normal x": ((0, 0, 0), (NAN, 1, 0)), "inf normal y": ((0, 0, 0), (0, INF, 0)), "-inf normal z": ((0, 0, 0), (0, 1, -INF)),
    "zero normal": ((1, 2, 3), (0, 0, 0)), "negative zero normal": ((1, 2, 3), (-0.0, -0.0, -0.0)),
    "normal whose squared length underflows to 0": ((1, 2, 3), (1e-30, -1e-30, 1e-30)), "normal whose squared length overflows": ((1, 2, 3), (1e30, 0, 0)),
}


@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
def test_inactive_points_give_the_all_zero_record(H, L, distribution):
    pts = points_of([v[0] for v in INACTIVE_POINTS.values()], [v[1] for v in INACTIVE_POINTS.values()])
    assert inactive_mask(pts).all()
    live = points_of([(1, 2, 3)], [(0, 2, 0)])
    both = np.concatenate([pts, live])
    got = runtime.point_rays(L, runtime.point_sampling(distribution), both, np.full((len(both), 2), 0.3, F))
    assert not got["origin"][:-1].view(np.uint32).any() and not got["direction"][:-1].view(np.uint32).any(), list(INACTIVE_POINTS)
    assert (got["tmax"] == np.finfo(F).max).all() and not got["reserved"].view(np.uint32).any()
    assert got["direction"][-1].any() and H.same_bits(got["origin"][-1], np.array([1, 2, 3], F))


# ---- 2. geometry -------------------------------------------------------------------------------------------------------------------------------------------------
def test_generator_geometry(H, L):
    """On the 64 x 64 midpoint grid g = ((i + .5) / 64, (j + .5) / 64), normal (0.3, -0.5, 0.8): the device's means equal a float64 evaluation of the same formulas to
    1e-5 (each binary32 sample is within about ten roundings, 6e-7, of its float64 value), and the float64 means are the distribution's moments to the grid's own
    quadrature error, computed on the CPU for this grid: cosine mean dot 2/3 within 2e-3 (1.02e-3), mean squared tangent component 1/4 within 2e-4 (1.2e-4); sphere
    mean dot 0 within 1e-6, mean dot^2 1/3 within 2e-4 (8.1e-5)."""
    i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    g = np.stack([(i.ravel() + 0.5) / 64, (j.ravel() + 0.5) / 64], axis=1)
    normal = np.array([0.3, -0.5, 0.8])
    pts = points_of(np.tile([0.5, 1.0, -0.25], (len(g), 1)), np.tile(normal, (len(g), 1)))
    nh = normal / np.linalg.norm(normal)
    for distribution in DISTRIBUTIONS:
        got = runtime.point_rays(L, runtime.point_sampling(distribution), pts, g.astype(F))
        d32 = got["direction"].astype(np.float64)
        _, d64, t64, bt64, n64 = restate(distribution, pts.astype(np.float64), g, np.float64, np.sin, np.cos)
        assert np.abs(n64[0] - nh).max() <= 1e-7          # (the normal as float32 holds it)
        stats = {}
        for name, d in (("device", d32), ("float64", d64)):
            dot = d @ n64[0]
            stats[name] = dict(dot=dot.mean(), dot2=(dot * dot).mean(), t2=((d @ t64[0]) ** 2).mean(), bt2=((d @ bt64[0]) ** 2).mean())
        dev, ref = stats["device"], stats["float64"]
        print(f"distribution {distribution}: float64 means {ref}; device - float64 " + ", ".join(f"{k} {dev[k] - ref[k]:.3g}" for k in ref))
        for k in ref:
            assert abs(dev[k] - ref[k]) <= 1e-5, (distribution, k, dev[k], ref[k])
        if distribution == 0:
            assert abs(ref["dot"] - 2 / 3) <= 2e-3 and abs(ref["t2"] - 0.25) <= 2e-4 and abs(ref["bt2"] - 0.25) <= 2e-4, ref
            assert (d32 @ n64[0]).min() >= -1e-6
        else:
            assert abs(ref["dot"]) <= 1e-6 and abs(ref["dot2"] - 1 / 3) <= 2e-4, ref
        assert np.abs(np.linalg.norm(d32, axis=1) - 1).max() <= 1e-6
    # the frame itself, from the device: the disk's (1, 0), (0, 1) and centre map to t, bt and n
    frame = runtime.point_rays(L, runtime.point_sampling(0), pts[:3], np.array([(1.0, 0.5), (0.5, 1.0), (0.5, 0.5)], F))["direction"].astype(np.float64)
    gram = frame @ frame.T
    assert np.abs(gram - np.eye(3)).max() <= 1e-6, gram
    assert np.abs(frame[2] - nh).max() <= 1e-6 and np.abs(frame[0] - t64[0]).max() <= 1e-6 and np.abs(frame[1] - bt64[0]).max() <= 1e-6


# ---- 3. - 5. chunks against the ray door -----------------------------------------------------------------------------------------------------------------------
SPP8 = 8


def cornell(integrator, spp=SPP8, **kw):
    return scenes.cornell_box(W, HGT, spp, integrator=integrator, jitter=0.5, **kw)


def far_hall(integrator, spp=SPP8):
    from tools.scaled_hall import scaled
    return scaled(scenes.sponza_hall(W, HGT, spp, integrator=integrator, jitter=0.5, detail=0.25), 100.0)


INACTIVE_EVERY = 37
_INACTIVE_KINDS = list(INACTIVE_POINTS.values())


def bake_points(to_world=lambda p: p):
    """[HGT, W, 8]: rows 0 - 13 a grid on the Cornell floor with normal +y, rows 14 - 27 a grid on the back wall with normal -z, rows 28 - 31 a row in mid-air with
    tilted, unnormalised normals; every 37th pixel an inactive point of another kind. to_world maps the Cornell box's coordinates into another scene's."""
    pos = np.zeros((HGT, W, 3), F); nrm = np.zeros((HGT, W, 3), F)
    u = -0.9 + 1.8 * (np.arange(W) + 0.5) / W
    for y in range(14):
        pos[y, :, 0] = u; pos[y, :, 1] = 0.0; pos[y, :, 2] = -0.9 + 1.8 * (y + 0.5) / 14
        nrm[y] = (0, 1, 0)
    for y in range(14, 28):
        pos[y, :, 0] = u; pos[y, :, 1] = 0.1 + 1.8 * (y - 14 + 0.5) / 14; pos[y, :, 2] = 1.0
        nrm[y] = (0, 0, -1)
    for y in range(28, HGT):
        pos[y, :, 0] = u; pos[y, :, 1] = 1.0 + 0.1 * (y - 28); pos[y, :, 2] = -0.3
        ang = 2 * math.pi * (np.arange(W) + 0.25 * (y - 28)) / W
        nrm[y, :, 0] = 1.7 * np.cos(ang); nrm[y, :, 1] = 0.6 * (y - 29.5); nrm[y, :, 2] = 1.7 * np.sin(ang)
    pts = points_of(to_world(pos.reshape(-1, 3)).astype(F), nrm.reshape(-1, 3))
    for k, at in enumerate(range(5, W * HGT, INACTIVE_EVERY)):
        p, n = _INACTIVE_KINDS[k % len(_INACTIVE_KINDS)]
        pts[at, 0:3] = p; pts[at, 4:7] = n
    return pts.reshape(HGT, W, 8)


def hall_world(p):
    """the Cornell box's coordinates into the hall scaled by 100 (x +-1000, y 0..800, z +-500): above its heightfield floor, between its columns"""
    return p * np.array([800.0, 300.0, 200.0], F) + np.array([0.0, 8.0, 0.0], F)


def stream_a_draws(H, L, prior, n_draws):
    """[HGT, W, n_draws]: the first draws of every pixel's stream A keyed (frame seed + pixel index, `prior` samples so far)"""
    pix = np.arange(W * HGT, dtype=np.uint64)
    k = np.full(W * HGT, prior, np.uint64)
    out = np.zeros((W * HGT, 3), np.uint64)
    rc = L.fn("terra_amd_unit_stream_keys", C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])(scenes.FRAME_SEED, pix.ctypes.data, k.ctypes.data, len(pix), out.ctypes.data)
    assert rc == 0, runtime.last_error()
    return H.Unit("amd").pcg(out[:, 0].astype(np.uint32), n_draws).reshape(HGT, W, n_draws)


def rays_of(L, ps, pts, g):
    """the generator's rays of every pixel of the frame for the pairs g [HGT, W, 2], as the ray door takes them"""
    rays = runtime.point_rays(L, ps, pts.reshape(-1, 8), g.reshape(-1, 2))
    return to_device(rays.view(F).reshape(HGT, W, 8))


# (scene, tree mode, TerraAmdTraversalInfo::last_call of the launch, the points): the LDS-resident template MODE, the fast tree, the reachability mode
CHUNK_SCENES = {"mode1": (cornell, 2, 2, None), "mode2": (cornell, 1, 3, None), "hall-x100": (far_hall, None, 4, hall_world)}


@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
@pytest.mark.parametrize("scene", list(CHUNK_SCENES))
def test_one_sample_chunks_equal_the_ray_door(H, L, scene, distribution, rect):
    import torch
    make, tree_mode, want_call, world = CHUNK_SCENES[scene]
    ps = runtime.point_sampling(distribution)
    pts = bake_points(world) if world else bake_points()
    dead = inactive_mask(pts.reshape(-1, 8)).reshape(HGT, W)
    d8, d1 = make(api.kTerraIntegratorDirect, 8), make(api.kTerraIntegratorDirect, 1)
    s8, s1 = make_scene(L, d8, tree_mode=tree_mode, split=8), make_scene(L, d1, tree_mode=tree_mode, split=1)
    try:
        fp, fr = Frame(), Frame()
        runtime.render_points_device(L, s8, ps, to_device(pts), fp.fb, rect=rect, rand_calls=fp.calls)
        call_points = last_call(L, s8)
        assert runtime.empty_skip_info(L, s8)[0] == 0                      # a point launch never skips
        total = torch.zeros_like(fr.calls)
        x, y, w, h = rect or (0, 0, W, HGT)
        for chunk in range(8):
            rays = rays_of(L, ps, pts, stream_a_draws(H, L, chunk, 4)[..., 2:4])          # r1, r2 drawn and unused, then g1, g2
            runtime.render_rays_device(L, s1, rays, fr.fb, rect=rect, rand_calls=fr.calls)
            total.view(HGT, W)[y:y + h, x:x + w] += fr.calls.view(HGT, W)[y:y + h, x:x + w]
        assert last_call(L, s1) == call_points == want_call, (last_call(L, s1), call_points)
        (pp, rp, cp), (pr, rr, _) = fp.host(), fr.host()
        inside = np.zeros((HGT, W), bool); inside[y:y + h, x:x + w] = True
        assert (rp["samples"][inside] == 8).all() and (rp["samples"][~inside] == 0).all() and rp["acc"].max() > 0
        assert (dead & inside).sum() >= 10
        assert not rp["acc"][dead & inside].view(np.uint32).any() and (cp[dead & inside] == 0).all()          # +0, and nothing drawn
        assert rp.tobytes() == rr.tobytes() and H.same_bits(pp, pr), scene
        assert np.array_equal(cp[inside], total.cpu().numpy().reshape(HGT, W)[inside]) and (cp[~inside] == 0x5ca1ab1e).all()
    finally:
        L.scene_destroy(s8); L.scene_destroy(s1)


@pytest.mark.parametrize("stratified", [False, True], ids=["random", "stratified"])
@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
@pytest.mark.parametrize("integrator", [api.kTerraIntegratorDebugDepth, api.kTerraIntegratorDebugNormals], ids=["depth", "normals"])
def test_chunk_of_four_samples_advances_stream_a(H, L, integrator, distribution, stratified):
    """spp 4 in one chunk: sample s of a pixel takes r1, r2 (unused), then the stratified sampler's two offsets (two trng_a_float of the pixel's stream A per sample;
    no sampler draws none), then g1, g2: with D = 2 + (2 if stratified) + 2 draws per sample, the pair is the last two of the sample's D. The debug integrators' value
    depends on the primary ray alone."""
    ps = runtime.point_sampling(distribution)
    pts = bake_points()
    kw = dict(sampling=api.kTerraSamplingMethodStratified, strata=2, sampler_integration=True) if stratified else {}
    d4, d1 = cornell(integrator, 4, **kw), cornell(integrator, 1)
    per_sample = 2 + (2 if stratified else 0) + 2
    s4, s1 = make_scene(L, d4, split=1), make_scene(L, d1, split=1)
    try:
        fp, fr = Frame(), Frame()
        runtime.render_points_device(L, s4, ps, to_device(pts), fp.fb, rect=RECT)
        draws = stream_a_draws(H, L, 0, 4 * per_sample)
        for smp in range(4):
            at = smp * per_sample
            runtime.render_rays_device(L, s1, rays_of(L, ps, pts, draws[..., at + per_sample - 2:at + per_sample]), fr.fb, rect=RECT)
        (pp, rp, _), (pr, rr, _) = fp.host(), fr.host()
        assert rp["samples"].sum() == 4 * RECT[2] * RECT[3] and rp["acc"].max() > 0
        assert rp.tobytes() == rr.tobytes() and H.same_bits(pp, pr)
    finally:
        L.scene_destroy(s4); L.scene_destroy(s1)


@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
def test_aov_equals_the_ray_door_aov(H, L, distribution, rect):
    import torch
    ps = runtime.point_sampling(distribution)
    pts = bake_points()
    d8, d1 = cornell(api.kTerraIntegratorSimple, 8), cornell(api.kTerraIntegratorSimple, 1)
    s8, s1 = make_scene(L, d8, split=8), make_scene(L, d1, split=1)
    try:
        ap, ar = runtime.DeviceAov(W, HGT), runtime.DeviceAov(W, HGT)
        runtime.render_aov_points_device(L, s8, ps, to_device(pts), ap, rect=rect)
        for chunk in range(8):
            runtime.render_aov_rays_device(L, s1, rays_of(L, ps, pts, stream_a_draws(H, L, chunk, 4)[..., 2:4]), ar, rect=rect)
        torch.cuda.synchronize()
        a, b = ap.host(), ar.host()
        x, y, w, h = rect or (0, 0, W, HGT)
        assert (a["samples"][y:y + h, x:x + w] == 8).all() and a["samples"].sum() == 8 * w * h and a["coverage"].max() > 0
        assert a.tobytes() == b.tobytes()
        # the host form, frame-indexed
        host = np.zeros((HGT, W), runtime.AOV_DTYPE)
        keep, hp = aligned_copy(pts)
        assert L.render_aov_points(s8, C.byref(ps), hp.ctypes.data, host.ctypes.data, W, HGT, x, y, w, h) == 0, runtime.last_error()
        assert host.tobytes() == a.tobytes()
    finally:
        L.scene_destroy(s8); L.scene_destroy(s1)


# ---- 6. host form, camera_limit ----------------------------------------------------------------------------------------------------------------------------------
def aligned_copy(a):
    """a float32 copy of `a` whose first byte is 16-byte aligned; returns (keep-alive, the copy)"""
    a = np.ascontiguousarray(a, F)
    raw = np.zeros(a.nbytes + 16, np.uint8)
    at = (-raw.ctypes.data) % 16
    out = raw[at:at + a.nbytes].view(F).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == 0
    return raw, out


@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("distribution", DISTRIBUTIONS, ids=DIST_IDS)
def test_host_form_equals_device_form(H, L, distribution, rect):
    ps = runtime.point_sampling(distribution)
    d = cornell(api.kTerraIntegratorDirect, 4)
    s = make_scene(L, d, split=2)
    try:
        keep, hp = aligned_copy(bake_points())
        dp = to_device(hp)
        f = Frame()
        fb = api.Framebuffer(L, W, HGT)
        x, y, w, h = rect or (0, 0, W, HGT)
        for _ in range(2):
            runtime.render_points_device(L, s, ps, dp, f.fb, rect=rect)
            L.clear_error()
            assert L.render_points(s, C.byref(ps), hp.ctypes.data, C.byref(fb.fb), x, y, w, h) == 0, runtime.last_error()
        pix, res, _ = f.host()
        assert fb.results.tobytes() == res.tobytes() and H.same_bits(fb.pixels, pix)
        assert res["samples"].sum() == 2 * 4 * w * h and res["acc"].max() > 0
        fb.destroy()
    finally:
        L.scene_destroy(s)


def test_beyond_camera_limit_runs_the_replica(H, L):
    """the host forms look at the ACTIVE points' positions: with all of them within camera_limit the call keeps the commit's traversal; with one beyond it on one axis
    the call runs the replica and the image is tree mode 0's; an INACTIVE point beyond it decides nothing"""
    ps = runtime.point_sampling(0)
    d = cornell(api.kTerraIntegratorDirect, 4)
    s, s0 = make_scene(L, d, split=2), make_scene(L, d, tree_mode=0, split=2)
    try:
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
        limit = float(ti.camera_limit)
        assert ti.leaf_cull == 1 and limit > 4
        base = bake_points()
        live_at = (10, 20)
        assert not inactive_mask(base[live_at][None])[0]
        for name, position, normal, replica in (("all within", None, None, False), ("one beyond on y", (0.2, limit + 1.0, 0.1), (0.1, -1.0, 0.2), True),
                                                ("an inactive one beyond", (0.2, limit + 1.0, 0.1), (0.0, 0.0, 0.0), False)):
            pts = base.copy()
            if position:
                pts[live_at][0:3] = position; pts[live_at][4:7] = normal
            keep, hp = aligned_copy(pts)
            fb = api.Framebuffer(L, W, HGT)
            assert L.render_points(s, C.byref(ps), hp.ctypes.data, C.byref(fb.fb), 0, 0, W, HGT) == 0, runtime.last_error()
            assert (last_call(L, s) == CALL_REPLICA) == replica, name
            f0 = Frame()
            runtime.render_points_device(L, s0, ps, to_device(hp), f0.fb)
            assert last_call(L, s0) == CALL_REPLICA
            pix0, res0, _ = f0.host()
            assert res0["acc"].max() > 0 and (res0["samples"] == 4).all()
            assert fb.results.tobytes() == res0.tobytes() and H.same_bits(fb.pixels, pix0), name
            # the AOV host form decides alike
            host = np.zeros((HGT, W), runtime.AOV_DTYPE)
            assert L.render_aov_points(s, C.byref(ps), hp.ctypes.data, host.ctypes.data, W, HGT, 0, 0, W, HGT) == 0, runtime.last_error()
            a0 = runtime.DeviceAov(W, HGT)
            runtime.render_aov_points_device(L, s0, ps, to_device(hp), a0)
            assert host.tobytes() == a0.host().tobytes(), name
            fb.destroy()
    finally:
        L.scene_destroy(s); L.scene_destroy(s0)


# ---- 7. sky furnace ----------------------------------------------------------------------------------------------------------------------------------------------
def sky_scene(spp):
    """one small diffuse triangle far below the points under a constant environment, environment lighting on, the Simple integrator"""
    tri = np.array([[[-0.5, -50.0, -0.5], [0.5, -50.0, -0.5], [0.0, -50.0, 0.5]]], F)
    nrm = np.broadcast_to(np.array([0, 1, 0], F), (1, 3, 3)).copy()
    obj = scenes.ObjectDesc(tri, nrm, np.zeros((1, 3, 2), F), scenes.Material(albedo=(0.5, 0.5, 0.5)), "speck")
    return scenes.SceneDesc(objects=[obj], width=W, height=HGT, spp=spp, bounces=4, integrator=api.kTerraIntegratorSimple, jitter=0.5,
                            environment=(0.25, 0.5, 1.5), environment_lighting=True, name="sky")


def test_sky_furnace_and_irradiance(H, L):
    import torch
    spp = 8
    s = make_scene(L, sky_scene(spp), split=2)
    try:
        r = H.rng(5)
        pos = r.uniform(-3, 3, size=(HGT, W, 3)).astype(F); pos[..., 1] = r.uniform(0.5, 4.0, size=(HGT, W)).astype(F)
        pts = points_of(pos.reshape(-1, 3), np.tile(np.array([0, 2.5, 0], F), (W * HGT, 1))).reshape(HGT, W, 8)
        up = np.zeros((HGT, W, 8), F); up[..., 0:3] = pos; up[..., 3] = np.finfo(F).max; up[..., 5] = 1.0
        fp, fr = Frame(), Frame()
        runtime.render_points_device(L, s, runtime.point_sampling(0), to_device(pts), fp.fb, rand_calls=fp.calls)
        runtime.render_rays_device(L, s, to_device(up), fr.fb, rand_calls=fr.calls)
        (pp, rp, cp), (pr, rr, cr) = fp.host(), fr.host()
        assert (rp["samples"] == spp).all() and rp["acc"].min() > 0
        assert rp.tobytes() == rr.tobytes() and H.same_bits(pp, pr) and np.array_equal(cp, cr)          # every sample escapes: the sky's radiance, spp times
        mean = rr["acc"].reshape(-1, 3) / F(spp)
        # runtime.irradiance: the points folded into a frame 256 wide, PI * acc / samples; a point count that is no multiple of the row, so the padding is inactive points
        n = 300
        e = runtime.irradiance(L, s, to_device(pos.reshape(-1, 3)[:n]), to_device(np.tile(np.array([0, 1, 0], F), (n, 1))), spp_batches=2)
        torch.cuda.synchronize()
        e = e.cpu().numpy()
        assert e.shape == (n, 3) and e.dtype == F
        want = (mean[:n].astype(np.float64) * math.pi)
        assert np.abs(e - want).max() <= 4e-7 * want.max(), np.abs(e - want).max()          # (two float32 roundings: the quotient and the product)
        assert np.allclose(e[0], math.pi * np.array([0.25, 0.5, 1.5]), rtol=1e-6)           # E = PI L under a constant sky
    finally:
        L.scene_destroy(s)


# ---- 8. downstream -----------------------------------------------------------------------------------------------------------------------------------------------
def test_denoiser_and_moments_take_a_points_frame(H, L):
    import torch
    d = cornell(api.kTerraIntegratorDirect, 4)
    ps = runtime.point_sampling(0)
    s = make_scene(L, d, split=2)
    try:
        pts = to_device(bake_points())
        fb, aov, mom = runtime.DeviceFramebuffer(W, HGT), runtime.DeviceAov(W, HGT), runtime.DeviceMoments(W, HGT)
        for _ in range(2):
            runtime.render_points_device(L, s, ps, pts, fb); runtime.render_aov_points_device(L, s, ps, pts, aov)
            runtime.accumulate_moments_device(L, s, fb, mom)
        rad = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda"); pix = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda")
        runtime.denoise_device(L, s, fb, aov, 3, radiance=rad, pixels=pix)
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        r = rad.cpu().numpy()
        assert np.isfinite(r).all() and r.max() > 0 and np.isfinite(pix.cpu().numpy()).all()
        assert (aov.host()["samples"] == 8).all() and (fb.results_host()["samples"] == 8).all()
        assert mom.data.cpu().numpy().any()
    finally:
        L.scene_destroy(s)
