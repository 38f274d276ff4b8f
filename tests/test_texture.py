"""The texture lookup, texel by texel (terra_texture_sample / terra_texture_sample_latlong, reference src/Terra.c:368-477): the device's texture_sample and
environment lookup through terra_amd_unit_texture_*, the library's host functions and the oracle against

  * tests/golden/texture_sample.npz, dumped from the compiled reference, wherever the reference defines the answer (the file's `defined` mask), bit for bit;
  * each other, bit for bit, on fresh inputs over the whole domain the product defines: 1 to 4 components, coordinates <= -1, NaN, +-inf,
    >= 2^32, the mirror positions the reference addresses out of range, the padding behind the last texel;
  * a model written from the DESIGN.md rule in numpy int64 / float64 that shares no code with any of them.

The atlas wall (scenes.atlas) then pins the lookup where the renderer uses it: surface records per ray, images in every kernel layout, the AOV albedo,
and tests/golden/render_atlas.npz from the compiled reference. Tests without the gpu mark run the oracle and the host functions only."""
import numpy as np
import pytest

from terra_amd import api, runtime, scenes

SIZES = [(1, 1), (1, 13), (13, 1), (5, 3), (13, 3), (16, 16), (65535, 1), (1, 65535)]      # (W, H)
F32 = np.float32


@pytest.fixture(scope="module")
def golden(H):
    return np.load(H.GOLDEN / "texture_sample.npz")


@pytest.fixture(scope="module")
def L(amd_lib):
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def same(H, a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(H.bits(a)[~nan], H.bits(b)[~nan])


# ---------------------------------------------------------------------------
# the goldens
# ---------------------------------------------------------------------------

def golden_cases(g):
    for k, (W, Ht, comps, depth, filt, addr) in enumerate(g["cases"].tolist()):
        data = g[f"texels_{W}x{Ht}_d{depth}"][: W * Ht * comps].reshape(Ht, W, comps)
        yield k, data, filt, addr, g["uv"][k], g["out"][k], g["defined"][k]


def check_golden(H, g, sample, latlong):
    n = 0
    for k, data, filt, addr, uv, want, defined in golden_cases(g):
        assert defined.sum() >= 100
        got = sample(data, filt, addr, uv)
        assert np.array_equal(H.bits(got[defined]), H.bits(want[defined])), (k, g["cases"][k].tolist())
        n += 1
    assert n == 98
    for k, (W, Ht, depth, addr) in enumerate(g["ll_cases"].tolist()):
        assert np.array_equal(H.bits(latlong(g[f"ll_texels_{k}"], addr, g["ll_dirs"])), H.bits(g[f"ll_out_{k}"])), k


def test_golden_covers_what_it_should(golden):
    cases = golden["cases"].tolist()
    combos = {(f, a, d, c) for (_, _, c, d, f, a) in cases}
    assert all((f, a, d, c) in combos for f in (0, 1) for a in (0, 1, 2) for d in (1, 4) for c in (1, 2, 3))
    assert {(w, h) for (w, h, *_) in cases} >= set(SIZES) and {f for (*_, f, _) in cases} == {0, 1, 2, 3}
    for (W, Ht, comps, depth, filt, addr), defined in zip(cases, golden["defined"]):
        assert defined.sum() >= 100 and (~defined).sum() <= 0.3 * defined.size
        if comps == 3 and addr != 1:
            assert defined.all()


def test_oracle_equals_the_golden_libm(H, orc_lib, golden, libm_mode):
    U = H.Unit("orc")
    check_golden(H, golden, U.texture_sample, U.texture_latlong)


def test_oracle_equals_the_golden_devmath(H, orc_lib, golden, devmath_mode):
    U = H.Unit("orc")
    check_golden(H, golden, U.texture_sample, U.texture_latlong)


def test_host_functions_equal_the_golden(H, amd_lib, golden):
    U = H.Unit("amd")
    check_golden(H, golden, lambda *a: U.texture_sample(*a, host=True), lambda *a: U.texture_latlong(*a, host=True))


@pytest.mark.gpu
def test_device_equals_the_golden(H, L, golden):
    U = H.Unit("amd")
    check_golden(H, golden, U.texture_sample, U.texture_latlong)


# ---------------------------------------------------------------------------
# fresh inputs over the product's whole domain
# ---------------------------------------------------------------------------

def texels(r, W, Ht, comps, depth):
    n = W * Ht * comps
    base = r.randint(0, 256, min(n, 5003)).astype(np.uint8) if depth == 1 else r.uniform(-2, 4, min(n, 5003)).astype(np.float32)
    return np.resize(base, n).reshape(Ht, W, comps)


def wide_uv(r, W, Ht, n=160):
    """coordinates inside and outside the reference's domain: several tiles either side of 0, exact integers, every mirror position the golden leaves out
    (odd tile, x % W == 0 or y % H == 0), the last texel, <= -1, huge of either sign, NaN, +-inf, >= 2^32"""
    uv = np.stack([r.uniform(-2 * W, 4 * W, n), r.uniform(-2 * Ht, 4 * Ht, n)], axis=1)
    uv[: n // 4] = np.floor(uv[: n // 4])
    uv[n // 4: n // 2] = np.stack([r.uniform(0, W, n // 4), r.uniform(0, Ht, n // 4)], axis=1)
    odd = np.array([1, 3, 5, 7])
    mx = np.stack([W * r.choice(odd, 24) + np.r_[np.zeros(12), r.uniform(0, 1, 12)], r.uniform(0, 3 * Ht, 24)], axis=1)                       # x % W == 0 in an odd tile
    my = np.stack([W * r.choice(odd, 24) + r.uniform(0, W, 24), Ht * r.randint(0, 4, 24) + np.r_[np.zeros(12), r.uniform(0, 1, 12)]], axis=1)    # y % H == 0 in an odd tile
    big = 2.0 ** 32
    sp = [-1.0, -1.5, -0.999, -0.0, 0.0, W - 1.0, W - 0.5, float(W), 2.0 * W, Ht - 1.0, float(Ht), -1e30, -3e9, 3e9, 2.0 ** 24, 2.0 ** 24 + 1, 2.0 ** 31, big - 256, big, 2 * big, 5e9, 1e19, 3e38,
          np.inf, -np.inf, np.nan]
    s1 = np.stack([sp, r.uniform(0, 2 * Ht, len(sp))], axis=1); s2 = np.stack([r.uniform(0, 2 * W, len(sp)), sp], axis=1); s3 = np.stack([sp, sp[::-1]], axis=1)
    return np.ascontiguousarray(np.concatenate([uv, mx, my, s1, s2, s3]), np.float32)


def fresh_cases(seed):
    r = np.random.RandomState(seed)
    for W, Ht in SIZES:
        for comps in (1, 2, 3, 4):
            for depth in (1, 4):
                data = texels(r, W, Ht, comps, depth)
                for filt in (0, 1):
                    for addr in (0, 1, 2):
                        yield data, filt, addr, wide_uv(r, W, Ht)
    yield texels(r, 5, 3, 7, 1), 1, 1, wide_uv(r, 5, 3)           # more components than an image has: the first three of each texel
    yield texels(r, 4, 4, 7, 4), 0, 0, wide_uv(r, 4, 4)
    yield texels(r, 5, 3, 3, 4), 2, 0, wide_uv(r, 5, 3)           # trilinear / anisotropic: zero
    yield texels(r, 5, 3, 4, 1), 3, 1, wide_uv(r, 5, 3)


def test_oracle_equals_the_host_functions(H, orc_lib, amd_lib):
    O = H.Unit("orc"); A = H.Unit("amd")
    for data, filt, addr, uv in fresh_cases(4001):
        want = O.texture_sample(data, filt, addr, uv)
        assert same(H, A.texture_sample(data, filt, addr, uv, host=True), want), (data.shape, data.dtype, filt, addr)
        if filt > 1:
            assert not want.any()


@pytest.mark.gpu
def test_device_equals_oracle_and_host_functions(H, L, orc_lib):
    O = H.Unit("orc"); A = H.Unit("amd")
    for data, filt, addr, uv in fresh_cases(4002):
        got = A.texture_sample(data, filt, addr, uv)
        assert same(H, got, O.texture_sample(data, filt, addr, uv)), (data.shape, data.dtype, filt, addr)
        assert same(H, got, A.texture_sample(data, filt, addr, uv, host=True)), (data.shape, data.dtype, filt, addr)


# ---------------------------------------------------------------------------
# a model that shares no code with the three implementations (restated)
# ---------------------------------------------------------------------------

def model_coord(u):
    """the coordinate the lookup uses: u itself inside (-1, 2^32); 0 for u <= -1 and NaN; the largest float below 2^32 from 2^32 on"""
    u = np.asarray(u, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(u > -1, np.minimum(u, 4294967040.0), 0.0)


def model_read(data, addr, x, y):
    """(n, 3) float32: three consecutive elements from element (y' W + x') c of the flat data, 0 past its end; bytes as float32(b) / float32(255)"""
    Ht, W, c = data.shape
    if addr == 2:
        xa, ya = np.minimum(x, W - 1), np.minimum(y, Ht - 1)
    elif addr == 0:
        xa, ya = x % W, y % Ht
    else:       # mirror: the tile's parity from x alone; column W / row H, which x % W == 0 / y % H == 0 reach in an odd tile, become the last ones
        odd = (x // W) % 2 == 1
        xa = np.where(odd, np.minimum(W - x % W, W - 1), x % W); ya = np.where(odd, np.minimum(Ht - y % Ht, Ht - 1), y % Ht)
    assert (xa >= 0).all() and (xa < W).all() and (ya >= 0).all() and (ya < Ht).all()
    flat = data.reshape(-1)
    flat = (flat.astype(np.float32) / F32(255)).astype(np.float32) if data.dtype == np.uint8 else flat
    padded = np.concatenate([flat, np.zeros(2, np.float32)])
    e = (ya * W + xa) * c
    return np.stack([padded[e], padded[e + 1], padded[e + 2]], axis=1)


def model_sample(data, filt, addr, uv):
    """(value (n, 3) float64, bound (n, 3) float64): point samples exact (bound 0). Bilinear: the float64 value of the reference's expression
        (n1 wou + n2 wu) wov + (n3 wou + n4 wu) wv,   wu = u - x, wou = 1 - wu  (v alike),
    with the exact weights, and a bound on what float32 arithmetic may add. wu = u - x is exact in float32 (u and its integer part are floats and the
    difference is representable). Every other operation rounds once, with relative error at most eps = 2^-24 while nothing underflows: wou (1), n * w (2),
    the inner sum (3), the product with wov or wv (4) whose factor was rounded too (5), the outer sum (6). A texel's term so passes through at most six
    roundings: |error| <= ((1 + eps)^6 - 1) * sum_k |n_k| |a_k| |b_k|, taken with the exact weights, plus 6 * 2^-149 for results in the subnormal range."""
    Ht, W, c = data.shape
    u = model_coord(uv[:, 0]); v = model_coord(uv[:, 1])
    ix = np.trunc(u).astype(np.int64); iy = np.trunc(v).astype(np.int64)
    n = len(uv)
    if filt == 0:
        return model_read(data, addr, ix, iy).astype(np.float64), np.zeros((n, 3))
    if filt != 1:
        return np.zeros((n, 3)), np.zeros((n, 3))
    x2 = np.minimum(ix + 1, W - 1); y2 = np.minimum(iy + 1, Ht - 1)
    n1, n2, n3, n4 = (model_read(data, addr, a, b).astype(np.float64) for a, b in ((ix, iy), (x2, iy), (ix, y2), (x2, y2)))
    wu = (u - ix)[:, None]; wv = (v - iy)[:, None]
    value = (n1 * (1 - wu) + n2 * wu) * (1 - wv) + (n3 * (1 - wu) + n4 * wu) * wv
    mass = (abs(n1) * abs(1 - wu) + abs(n2) * abs(wu)) * abs(1 - wv) + (abs(n3) * abs(1 - wu) + abs(n4) * abs(wu)) * abs(wv)
    eps = 2.0 ** -24
    return value, ((1 + eps) ** 6 - 1) * mass + 6 * 2.0 ** -149


def check_model(sample, seed):
    worst = 0.0
    for data, filt, addr, uv in fresh_cases(seed):
        got = sample(data, filt, addr, uv).astype(np.float64)
        value, bound = model_sample(data, filt, addr, uv)
        assert not np.isnan(got).any()            # (finite texels, weights in (-1, 2): nothing to make one)
        if filt != 1:
            assert np.array_equal(got, value), (data.shape, data.dtype, filt, addr)
        else:
            err = abs(got - value)
            assert (err <= bound).all(), (data.shape, data.dtype, filt, addr, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"bilinear: largest error / bound = {worst:.3f}")


def test_host_functions_follow_the_model(H, amd_lib):
    A = H.Unit("amd")
    check_model(lambda *a: A.texture_sample(*a, host=True), 4003)


def test_oracle_follows_the_model(H, orc_lib):
    check_model(H.Unit("orc").texture_sample, 4004)


@pytest.mark.gpu
def test_device_follows_the_model(H, L):
    check_model(H.Unit("amd").texture_sample, 4005)


# ---------------------------------------------------------------------------
# the padding behind the last texel
# ---------------------------------------------------------------------------

def last_texel_cases():
    for depth, one in ((1, np.uint8(255)), (4, F32(7.5))):
        for comps in (1, 2):
            for W, Ht in ((1, 1), (3, 2), (64, 1)):
                data = np.full((Ht, W, comps), one, np.uint8 if depth == 1 else np.float32)
                v = 1.0 if depth == 1 else 7.5
                # the last texel: its own elements, then 0
                yield data, np.array([[W - 1, Ht - 1]], np.float32), np.array([[v, v if comps == 2 else 0.0, 0.0]], np.float32)


def test_last_texel_on_the_host(H, amd_lib, orc_lib):
    for data, uv, want in last_texel_cases():
        for addr in (0, 1, 2):
            assert np.array_equal(H.Unit("amd").texture_sample(data, 0, addr, uv, host=True), want)
            assert np.array_equal(H.Unit("orc").texture_sample(data, 0, addr, uv), want)


@pytest.mark.gpu
def test_last_texel_on_the_device_after_other_data(H, L, orc_lib):
    """the two elements behind a texture's data read as 0, also in device memory that has just held something else: a lookup on a texture of the same
    footprint filled with ones, and a whole textured scene committed and destroyed, come first"""
    A = H.Unit("amd")
    for data, uv, want in last_texel_cases():
        loud = np.full((data.shape[0], data.shape[1], data.shape[2] + 2), 255 if data.dtype == np.uint8 else 3.0e38, data.dtype)
        A.texture_sample(loud, 0, 0, uv)
        assert np.array_equal(A.texture_sample(data, 0, 0, uv), want), (data.shape, data.dtype)
    # the same through a scene: Cornell with one-component textures on the checker and the light, after a scene with other textures was destroyed
    o, d = H.scene_rays(77, 4096)
    U = H.Unit("orc")
    first = scenes.cornell_textured(16, 16, 1)
    for ob in first.objects:
        for t in (ob.material.albedo_texture, ob.material.emissive_texture):
            if t is not None:
                t.data = np.full(t.data.shape, 255 if t.data.dtype == np.uint8 else 9.0e37, t.data.dtype)
    L.scene_destroy(scenes.build_scene(L, first))
    second = scenes.cornell_textured(16, 16, 1)
    m0 = second.objects[0].material; m0.albedo_texture = scenes.TextureDesc(m0.albedo_texture.data[..., :1].copy(), 0, 0)
    m3 = second.objects[3].material; m3.emissive_texture = scenes.TextureDesc(m3.emissive_texture.data[..., :2].copy(), 0, 2)
    sd = scenes.build_scene(L, second); so = scenes.build_scene(U.L, second)
    got = A.raycast(sd, o, d); want = U.raycast(so, o, d)
    assert np.array_equal(got[0], want[0]) and (got[0] >= 0).sum() > 1000
    hit = got[0] >= 0; phong = got[0] == 4
    # frame, normal, emissive (floats 0-21) and the first attribute slot (23-25) of every hit, the Phong box's textured albedo (slot 1, 26-28) on that box
    assert same(H, got[3][hit][:, :22], want[3][hit][:, :22]) and same(H, got[3][hit][:, 23:26], want[3][hit][:, 23:26])
    assert phong.sum() > 50 and same(H, got[3][phong][:, 26:29], want[3][phong][:, 26:29])
    light = got[0] == 3; floor = got[0] == 0
    assert light.sum() > 20 and floor.sum() > 500 and len(np.unique(got[3][light][:, 19:22], axis=0)) > 1 and len(np.unique(got[3][floor][:, 23:26], axis=0)) > 1
    # the padded reads themselves occur: the checker's last texel (one component: value, 0, 0) and the light's (two components: value, value, 0); every
    # other texel of either texture has non-zero successors
    a = got[3][floor][:, 23:26]; e = got[3][light][:, 19:22]
    assert ((a[:, 0] > 0) & (a[:, 1] == 0) & (a[:, 2] == 0)).sum() >= 5 and ((a[:, 1] > 0) & (a[:, 2] == 0)).sum() >= 5
    assert ((e[:, 1] > 0) & (e[:, 2] == 0)).sum() >= 5 and (e[:, 2] > 0).sum() >= 5
    L.scene_destroy(sd); U.L.scene_destroy(so)


def test_light_power_uses_the_lookup_the_device_shades_with(H, amd_lib, orc_lib):
    """the commit evaluates a textured emissive on the host at uv (0.5, 0.5): for a 1-component texture that is the texel and its two successors, not (texel, 0, 0)"""
    data = np.array([[[2.0], [3.0]], [[5.0], [7.0]]], np.float32)
    uv = np.array([[0.5, 0.5]], np.float32)
    for U, kw in ((H.Unit("amd"), dict(host=True)), (H.Unit("orc"), {})):
        assert np.array_equal(U.texture_sample(data, 0, 2, uv, **kw), [[2.0, 3.0, 5.0]])
        assert np.array_equal(U.texture_sample(data, 0, 2, uv + 1, **kw), [[7.0, 0.0, 0.0]])


# ---------------------------------------------------------------------------
# the lat-long lookup by direction
# ---------------------------------------------------------------------------

def index_map(W, Ht):
    """a float texture whose texel (x, y) holds (x, y, y W + x): a lookup's result names the texel it read"""
    yy, xx = np.meshgrid(np.arange(Ht), np.arange(W), indexing="ij")
    return np.stack([xx, yy, yy * W + xx], axis=2).astype(np.float32)


def latlong_dirs(r):
    tiny = [1e-30, 1e-38, 1e-45, 1e-7]
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.0, 1.0, -0.0], [-0.0, -1.0, 0.0]]
    for t in tiny:
        d += [[-1, 0, t], [-1, 0, -t], [-1, t, 0], [-3, 0.5, t], [-3, 0.5, -t], [t, 1, 0], [t, -1, t], [-t, 1, -t], [t, 0, 0], [0, t, 0], [-t, -t, -t]]      # the atan2 seam, the poles, very short
    d += [[-1, 0, 0.0], [-1, 0, -0.0], [1e19, 0, 0], [0, -1e19, 1], [3e38, 3e38, 3e38], [1e-20, 1e19, 0], [0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [2, -3, 6], [-0.5, 0.001, -1e-3]]
    rnd = r.normal(size=(400, 3)) * r.choice([1e-12, 1e-3, 1, 50, 1e12], size=(400, 1))
    return np.ascontiguousarray(np.concatenate([np.array(d, np.float64), rnd]), np.float32)


def check_latlong_in_range(out, W, Ht):
    assert not np.isnan(out).any()
    x, y, k = out[:, 0], out[:, 1], out[:, 2]
    assert ((x >= 0) & (x < W) & (y >= 0) & (y < Ht) & (k == y * W + x)).all()


def test_latlong_host_and_oracle(H, amd_lib, orc_lib, libm_mode):
    dirs = latlong_dirs(np.random.RandomState(4010))
    for W, Ht in ((16, 8), (1, 1), (7, 5), (65535, 1), (1, 65535)):
        for addr in (0, 1, 2):
            data = index_map(W, Ht)
            want = H.Unit("orc").texture_latlong(data, addr, dirs)
            check_latlong_in_range(want, W, Ht)
            assert np.array_equal(H.Unit("amd").texture_latlong(data, addr, dirs, host=True), want), (W, Ht, addr)


@pytest.mark.gpu
def test_latlong_device_equals_oracle(H, L, orc_lib, devmath_mode):
    dirs = latlong_dirs(np.random.RandomState(4011))
    for W, Ht in ((16, 8), (1, 1), (7, 5), (65535, 1), (1, 65535)):
        for addr in (0, 1, 2):
            data = index_map(W, Ht)
            got = H.Unit("amd").texture_latlong(data, addr, dirs)
            check_latlong_in_range(got, W, Ht)
            assert np.array_equal(got, H.Unit("orc").texture_latlong(data, addr, dirs)), (W, Ht, addr)


# ---------------------------------------------------------------------------
# the lookup where the renderer uses it: the atlas wall (scenes.atlas)
# ---------------------------------------------------------------------------

ATTR = slice(23, 35)        # attribute slots 0-3 of a surface record; floats 0-21 are the frame, the normal and the emissive


def atlas_rays(n, seed=4020):
    """from around the camera at the wall's quads, the light and the floor"""
    r = np.random.RandomState(seed)
    o = (np.array([0, 1, -3.4]) + r.uniform(-0.3, 0.3, size=(n, 3))).astype(np.float32)
    tgt = np.stack([r.uniform(-1, 1, n), r.uniform(0, 2, n), np.ones(n)], axis=1)
    k = n // 8
    tgt[:k] = np.stack([r.uniform(-0.5, 0.5, k), np.full(k, 1.99), r.uniform(-0.5, 0.5, k)], axis=1)
    tgt[k:2 * k] = np.stack([r.uniform(-1, 1, k), np.zeros(k), r.uniform(-1, 1, k)], axis=1)
    return o, np.ascontiguousarray(tgt - o, np.float32)


def test_atlas_per_ray_oracle_equals_reference_where_defined(H, orc_lib, ref_lib):
    d = scenes.atlas(reference_defined=True)
    o, dd = atlas_rays(3000)
    so = scenes.build_scene(orc_lib, d); sr = scenes.build_scene(ref_lib, d)
    a = H.Unit("orc").raycast(so, o, dd); b = H.Unit("ref").raycast(sr, o, dd)
    hit = a[0] >= 0
    assert np.array_equal(a[0], b[0]) and hit.sum() > 2500
    assert same(H, a[3][hit][:, :22], b[3][hit][:, :22]) and same(H, a[3][hit][:, 23:26], b[3][hit][:, 23:26])
    orc_lib.scene_destroy(so); ref_lib.scene_destroy(sr)


@pytest.mark.gpu
def test_atlas_per_ray(H, L, orc_lib):
    """surface records (interpolated texcoord -> emissive and the four attribute slots) of 6,000 rays, device against oracle, every object hit"""
    d = scenes.atlas()
    o, dd = atlas_rays(6000)
    sd = scenes.build_scene(L, d); so = scenes.build_scene(orc_lib, d)
    assert runtime.last_error() == "", runtime.last_error()
    got = H.Unit("amd").raycast(sd, o, dd); want = H.Unit("orc").raycast(so, o, dd)
    hit = got[0] >= 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and hit.sum() > 5000
    assert set(got[0][hit].tolist()) == set(range(len(d.objects)))
    assert same(H, got[3][hit][:, :22], want[3][hit][:, :22])
    phong = np.array([ob.material.kind == "phong" for ob in d.objects])[got[0][hit]]
    assert same(H, got[3][hit][phong][:, ATTR], want[3][hit][phong][:, ATTR]) and same(H, got[3][hit][~phong][:, 23:26], want[3][hit][~phong][:, 23:26])
    # every slot is wired to its own texture: on a Phong quad the four slots differ from one another, and the exponents (slot 2) are the integers of their texture
    rec = got[3][hit][phong]
    assert (rec[:, 29] == np.round(rec[:, 29])).all() and (rec[:, 29] >= 1).all()
    for a in range(4):
        for b in range(a + 1, 4):
            assert (rec[:, 23 + 3 * a] != rec[:, 23 + 3 * b]).mean() > 0.9, (a, b)
    emissive = np.array([ob.material.emissive_texture is not None for ob in d.objects])[got[0][hit]]
    assert (got[3][hit][emissive][:, 19:22] != 0).any(axis=1).all() and not got[3][hit][~emissive][:, 19:22].any()
    L.scene_destroy(sd); orc_lib.scene_destroy(so)


def atlas_device(L, d, tree_mode, split=1, calls=False):
    import ctypes as C
    import torch
    s = scenes.build_scene(L, d, tree_mode=tree_mode)
    assert runtime.last_error() == "", runtime.last_error()
    runtime.check(L.set_sample_split(s, split))
    fb = runtime.DeviceFramebuffer(d.width, d.height); cam = scenes.camera_of(d)
    rc = torch.zeros(d.width * d.height, dtype=torch.int32, device="cuda") if calls else None
    runtime.render_device(L, cam, s, fb, None, rc)
    torch.cuda.synchronize()
    ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
    out = dict(pixels=fb.pixels_host().copy(), acc=fb.results_host()["acc"].copy(), resident=ti.lds_resident,
               rand_calls=rc.cpu().numpy().astype(np.uint32).reshape(d.height, d.width) if calls else None)
    L.scene_destroy(s)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False])
def test_atlas_images(H, L, orc_lib, devmath_mode, resident):
    """integrators 0-2 in every kernel layout (tree modes 0, 1, 2; the scene small enough to be staged in LDS, and not), 4 samples as 2 lanes of 2"""
    import dataclasses
    for integ in (0, 1, 2):
        d = scenes.atlas(48, 32, 4, integrator=integ, cells=10) if resident else scenes.atlas(48, 32, 4, integrator=integ, filler=24)
        want = H.Unit("orc").render_pixels(dataclasses.replace(d, spp=2), passes=2, want_calls=False)
        for tree_mode in (0, 1, 2):
            got = atlas_device(L, d, tree_mode, split=2)
            if tree_mode == 0:
                assert bool(got["resident"]) == resident, (integ, got["resident"])
            assert same(H, got["acc"], want["acc"]) and same(H, got["pixels"], want["pixels"]), (integ, tree_mode)
        assert want["pixels"].mean() > 0.05


@pytest.mark.gpu
def test_atlas_aov_albedo_equals_the_per_ray_values(H, L):
    """one unjittered sample per pixel: the first-hit albedo sum of a pixel is the albedo slot of its camera ray's surface record"""
    import torch
    d = scenes.atlas(64, 48, 1, jitter=0.0)
    s = scenes.build_scene(L, d); cam = scenes.camera_of(d)
    aov = runtime.DeviceAov(d.width, d.height)
    runtime.render_aov_device(L, cam, s, aov); torch.cuda.synchronize()
    a = aov.host()
    yy, xx = np.meshgrid(np.arange(d.height), np.arange(d.width), indexing="ij")
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.uint32)
    dirs = H.Unit("amd").camera_dirs(cam, d.width, d.height, xy, 0.0, np.zeros((len(xy), 2), np.float32))
    o = np.tile(np.array(d.camera_position, np.float32), (len(xy), 1))
    obj, _, _, surf = H.Unit("amd").raycast(s, np.ascontiguousarray(o), dirs)
    hit = obj >= 0
    phong = np.array([ob.material.kind == "phong" for ob in d.objects])[np.maximum(obj, 0)]
    want = np.where(phong[:, None], surf[:, 26:29], surf[:, 23:26]) * hit[:, None]
    assert hit.mean() > 0.4 and np.array_equal(a["coverage"].ravel() > 0, hit)
    assert np.array_equal(a["albedo"].reshape(-1, 3), want.astype(np.float32))
    L.scene_destroy(s)


def check_atlas_golden(H, render):
    g = np.load(H.GOLDEN / "render_atlas.npz")
    for integ in (0, 1, 2):
        out = render(scenes.atlas(64, 48, 3, integrator=integ, reference_defined=True))
        assert H.same_bits(out["pixels"], g[f"i{integ}_pixels"]), integ
        if out["rand_calls"] is not None:
            assert np.array_equal(out["rand_calls"], g[f"i{integ}_calls"].astype(np.uint32)), integ


def test_atlas_golden_oracle(H, orc_lib, libm_mode):
    check_atlas_golden(H, lambda d: H.Unit("orc").render_pixels(d, passes=2))


@pytest.mark.gpu
def test_atlas_golden_device(H, L):
    """the reference-defined atlas from the compiled reference: pixels and per-pixel rand() counts, two accumulating passes"""
    import torch

    def two_passes(d, tree_mode, calls):
        s = scenes.build_scene(L, d, tree_mode=tree_mode)
        fb = runtime.DeviceFramebuffer(d.width, d.height); cam = scenes.camera_of(d)
        rc = torch.zeros(d.width * d.height, dtype=torch.int32, device="cuda") if calls else None
        for _ in range(2):
            runtime.render_device(L, cam, s, fb, None, rc)
        torch.cuda.synchronize()
        out = dict(pixels=fb.pixels_host().copy(), rand_calls=rc.cpu().numpy().astype(np.uint32).reshape(d.height, d.width) if calls else None)
        L.scene_destroy(s)
        return out
    check_atlas_golden(H, lambda d: two_passes(d, 0, True))
    check_atlas_golden(H, lambda d: two_passes(d, 1, False))
