"""The shading stages of the LDS-resident kernels without work counters (csrc/exact_div.h "Shading stages"): the next ray's reciprocals (trace_math.h ray_stage), a
hit's barycentrics and normal (shading_device.h surface_stage) and the continuation (integrators_device.h continue_stage) run their short exact quotients and roots
unguarded, AND the sites' range tests into one lane mask, take one vote per wave and compute the stage again with the guarded helpers where any lane failed.

* terra_amd_unit_shade_stages runs a stage both ways on rows of operands -- 4,096 rows per stage, 64 consecutive rows a wave: waves of ordinary rows, waves with one
  row that fails a range test, waves in which every row fails one. The operands' edge set is tests/test_exact_div_gpu.py's: +-0, the smallest and the largest
  denormal, 2^-61, 2^-60, 2^60, 2^61, a significand of all ones, +-inf, NaN. The two forms must agree bit for bit (two NaNs count as equal), and the mask must be 0
  on exactly the rows where a site's guard fails: restated here in numpy for stages 1 and 2; for stage 3, whose operands pass through a sine and five roots, the
  unit kernel runs path_continue itself as the guarded form and restates its nine sites' guards over the plain helpers, a bit per site. The one test a stage
  does not make is the all-ones test of a normalised vector's length: it takes that reciprocal in closed form.
* The range tests that were left out: all 2^24 stream variates through both roots of the diffuse sample against sqrt_exact (stage 4, a device count of offenders);
  the same launch holds the closed-form reciprocal of a length whose significand is all ones to 1.f / d on all 242 of them in range, and a sample of 2^24
  quotients by such lengths to "/".
* Frames that take the second run, 8 spp under Simple and Direct, against the oracle bit for bit: a camera looking along an axis at an odd-sized frame with no
  jitter, whose centre column and row hold a direction component of exactly 0 (stage 1 falls back in every wave that holds such a pixel); the same camera
  in front of a back wall made of two quads that meet on the plane x = 0, so that the centre column's hits lie exactly on a shared edge and have a barycentric
  numerator of exactly 0 (stage 2 falls back in the waves that hold them, whose other lanes pass); the Cornell box scaled by 2^18, where every triangle's
  barycentric denominator lies above 2^60 (stage 2 falls back at every hit); and a launch just outside the camera limits, which reports the guarded ray start.
* The camera sample's normalisation without its range tests on the corner pixels and the centre column, at both ends of the admitted tan_half_fov (stage 5)."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_leaf_boxes_gpu import dev
from test_leaf_pairs_gpu import dev as pairs_dev
from test_flat_loop_layout_gpu import oracle, equals_oracle

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
ROWS, WAVE = 4096, 64
LO, HI = F(2.0 ** -60), F(2.0 ** 60)
ALL_ONES = F(2.0) - F(2.0 ** -23)
EDGE = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -126 - 2.0 ** -149, -(2.0 ** -126 - 2.0 ** -149), 2.0 ** -61, -2.0 ** -61, 2.0 ** -60, -2.0 ** -60, 2.0 ** 60, -2.0 ** 60,
                 2.0 ** 61, -2.0 ** 61, ALL_ONES, -ALL_ONES, ALL_ONES * F(2.0 ** -3), np.inf, -np.inf, np.nan], F)


@pytest.fixture(scope="module")
def X(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    f = lib.fn("terra_amd_unit_shade_stages", C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])

    def run(stage, drops, rows):
        rows = np.ascontiguousarray(rows, F); n = len(rows)
        assert rows.shape == (n, 16)
        staged = np.zeros((n, 8), U); guarded = np.zeros((n, 8), U); mask = np.zeros(n, U); full = np.zeros(n, U)
        rc = f(stage, drops, rows.ctypes.data, n, staged.ctypes.data, guarded.ctypes.data, mask.ctypes.data, full.ctypes.data, None)
        assert rc == 0, runtime.last_error()
        return staged, guarded, mask, full

    def variate_roots():
        bad = np.zeros(1, U)
        rc = f(4, 1, None, 0, None, None, None, None, bad.ctypes.data)
        assert rc == 0, runtime.last_error()
        return int(bad[0])

    class Entry:
        pass
    e = Entry(); e.run = run; e.variate_roots = variate_roots
    return e


def same_words(a, b):
    """== on the words; NaN results count as equal when both are NaN"""
    fa, fb = a.view(F), b.view(F)
    nan = np.isnan(fa)
    return np.array_equal(nan, np.isnan(fb)) and np.array_equal(a[~nan], b[~nan])


def in_range(v):
    a = np.abs(v)
    return (a >= LO) & (a <= HI)          # (False for a NaN)


def rcp_ok(v):
    return in_range(v) & ((v.view(U) & U(0x7fffff)) != U(0x7fffff))


def component_ok(c):
    return (c == 0) | (np.abs(c) >= LO)


def waves_with_edges(rows, operands, failing, failing_operands=None):
    """rows (ROWS, 16) of ordinary operands, in place: wave w keeps them (w % 4 == 0), gets one row with one operand of `operands` replaced by a member of EDGE
    (w % 4 == 1), a member of EDGE in one operand of every row (w % 4 == 2), or one of `failing` -- values that fail the range test of every one of
    `failing_operands` (default: `operands`) -- in one of those of every row (w % 4 == 3). Operands and values are taken round robin, so every pair turns up."""
    k = 0
    for w in range(ROWS // WAVE):
        kind = w % 4
        lanes = [] if kind == 0 else [(7 * w) % WAVE] if kind == 1 else range(WAVE)
        for lane in lanes:
            vals, ops = (failing, failing_operands or operands) if kind == 3 else (EDGE, operands)
            rows[w * WAVE + lane, ops[k % len(ops)]] = vals[(k // len(ops)) % len(vals)]
            k += 1
    return rows


def wave_failures(mask):
    return set((mask.reshape(-1, WAVE) == 0).sum(axis=1).tolist())


def unit_vectors(r, n):
    v = r.normal(size=(n, 3)).astype(F)
    return (v / np.sqrt((v * v).sum(axis=1, dtype=F))[:, None]).astype(F)


def stage1_rows(seed=1):
    r = np.random.default_rng(seed)
    rows = np.zeros((ROWS, 16), F)
    rows[:, 0:3] = unit_vectors(r, ROWS)
    return waves_with_edges(rows, [0, 1, 2], np.array([0.0, -0.0, np.nan, 1e-45, 2.0 ** -61], F))


def test_ray_stage_equals_make_ray_guarded(X):
    rows = stage1_rows()
    staged, guarded, mask, full = X.run(1, 0, rows)
    assert same_words(staged, guarded)
    want = rcp_ok(rows[:, 0]) & rcp_ok(rows[:, 1]) & rcp_ok(rows[:, 2])
    assert np.array_equal(mask != 0, want) and np.array_equal(mask, full)
    assert {0, 1, WAVE} <= wave_failures(mask)
    # the short sequence really ran: an ordinary row's reciprocals are the correctly rounded quotients
    ordinary = rows[:WAVE, 0:3]
    assert np.array_equal(staged[:WAVE, 0:3].view(F), (F(1.0) / ordinary).astype(F))


def test_ray_stage_without_the_upper_bound(X):
    """what the stage is handed in a launch inside the camera limits: a component below 8 in magnitude (a normalised vector, rotated by a frame whose entries are
    at most 2), or a NaN -- test_continue_stage_equals_path_continue holds that the continuation never hands it an infinity. On such rows the stage without the
    upper-bound comparisons gives make_ray_guarded's reciprocals and the mask of the whole guard"""
    rows = stage1_rows(seed=2)
    big = np.abs(rows[:, 0:3]) >= 8                    # (False for a NaN)
    rows[:, 0:3] = np.where(big, np.sign(rows[:, 0:3]) * F(7.5), rows[:, 0:3])
    staged, guarded, mask, full = X.run(1, 1, rows)
    assert same_words(staged, guarded) and np.array_equal(mask, full)
    assert np.array_equal(mask != 0, rcp_ok(rows[:, 0]) & rcp_ok(rows[:, 1]) & rcp_ok(rows[:, 2]))
    assert {0, 1, WAVE} <= wave_failures(mask)


def film_vectors(width, height, pixels, jitter, draws, aspect_tan, tan):
    """( fx, fy ) as camera_film and camera_sample form them in float32, for every pixel x draw pair"""
    out = []
    for px, py in pixels:
        for r1 in draws:
            for r2 in draws:
                j = F(jitter)
                dx = -j + F(2) * F(r1) * j; dy = -j + F(2) * F(r2) * j
                ndc_x = (F(px) + F(0.5) + dx) / F(width); ndc_y = (F(py) + F(0.5) + dy) / F(height)
                sx = F(2) * ndc_x - F(1); sy = F(1) - F(2) * ndc_y
                aspect = F(width) / F(height)
                out.append((sx * aspect * F(tan), sy * F(tan)))
    return np.array(out, F)


def test_camera_normalisation_without_range_tests(X):
    """the four corner pixels and the centre column of a 64 x 48 frame, jitter 0 and 0.5 (draws at both ends and the middle of [0, 1)), tan_half_fov at both
    ends of what the host admits (2^-30; 0.75 * 2^20, where aspect * tan_half_fov = 2^20) and at two ordinary values: the film vector normalised without a
    range test (trace_geometry.h camera_film_normalize) against normalize_plain, bit for bit. The conditions the form rests on are asserted on the rows"""
    W, Hh = 64, 48
    pixels = [(0, 0), (W - 1, 0), (0, Hh - 1), (W - 1, Hh - 1)] + [(W // 2, y) for y in range(Hh)]
    draws = [0.0, 0.5, float(F(1.0) - F(2.0 ** -24))]
    rows = []
    for tan in (2.0 ** -30, 0.75 * 2.0 ** 20, 1.0, float(np.tan(np.float64(F(45.0) * F(0.0174533)) / 2))):
        assert F(W) / F(Hh) * F(tan) >= LO * F(2.0 ** 30) and F(W) / F(Hh) * F(tan) <= F(2.0 ** 20)
        for jitter in (0.0, 0.5):
            rows.append(film_vectors(W, Hh, pixels, jitter, draws, None, tan))
    # film vectors whose length is 2 - 2^-23, the one all-ones significand a length in [1, 2) can have: fx among the floats around sqrt ( 3 ), fy = 0
    c = (np.arange(-64, 64) + int(F(np.sqrt(3.0)).view(U))).astype(U).view(F)
    lc = np.sqrt(c * c + F(0) * F(0) + F(1))
    c = c[(lc.view(U) & U(0x7fffff)) == U(0x7fffff)]
    assert len(c) >= 1          # (consecutive fx give consecutive lengths there: one of them)
    rows.append(np.stack([c, np.zeros_like(c)], 1))
    f = np.concatenate(rows)
    a = np.abs(f)
    assert (((a == 0) | (a >= F(2.0 ** -55))) & (a <= F(2.0 ** 21))).all() and (f == 0).any()          # 0 or far above 2^-60; the centre column at jitter 0.5, draw 0, is 0
    data = np.zeros((len(f), 16), F); data[:, 0:2] = f
    staged, guarded, mask, full = X.run(5, 0, data)
    assert np.array_equal(staged, guarded) and not np.isnan(staged[:, :3].view(F)).any()


def test_surface_stage_equals_surface_init(X):
    r = np.random.default_rng(3)
    rows = np.zeros((ROWS, 16), F)
    rows[:, 2] = r.uniform(0.5, 4.0, ROWS)                                                  # div
    rows[:, 0] = r.uniform(0.05, 0.45, ROWS) * rows[:, 2]; rows[:, 1] = r.uniform(0.05, 0.45, ROWS) * rows[:, 2]      # nu, nv: barycentrics inside the triangle
    base = unit_vectors(r, ROWS)
    for k in range(3):                                                                        # three vertex normals near one direction
        rows[:, 3 + 3 * k:6 + 3 * k] = base + r.normal(scale=0.1, size=(ROWS, 3)).astype(F)
    wall = (np.arange(ROWS) // WAVE % 4 == 0) & (np.arange(ROWS) % WAVE < WAVE // 2)      # half of every ordinary wave, 512 rows:
    rows[wall, 3:12] = np.tile(np.array([0.0, 1.0, 0.0], F), 3)                           # a wall's normals: the interpolated length is a float next to 1
    waves_with_edges(rows, list(range(12)), np.array([np.nan], F))
    rows[5 * WAVE + 3, 3:12] = 0.0                                                          # a wave with one row whose normals are all zero: the root's guard
    rows[9 * WAVE + 11, 3:12] = F(2.0 ** -50)                                               # ... and one whose squared length lies below 2^-96
    staged, guarded, mask, full = X.run(2, 0, rows)
    assert same_words(staged, guarded)
    # the guards, restated: the quotients' (surface_init), then -- on u, v as the guarded code returns them -- the root's and the normalisation's
    nu, nv, div = rows[:, 0], rows[:, 1], rows[:, 2]
    u, v = guarded[:, 0].view(F), guarded[:, 1].view(F)
    with np.errstate(all="ignore"):
        w = F(1.0) - u - v
        nrm = (rows[:, 9:12] * v[:, None] + rows[:, 6:9] * u[:, None]) + rows[:, 3:6] * w[:, None]
        l2 = nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2]
        l = np.sqrt(l2)
        want = (rcp_ok(div) & in_range(nu) & in_range(nv) & (l2 >= F(2.0 ** -96)) & (l2 <= np.finfo(F).max)
                & (l >= LO) & (l <= HI) & component_ok(nrm[:, 0]) & component_ok(nrm[:, 1]) & component_ok(nrm[:, 2]))
        all_ones = (l.view(U) & U(0x7fffff)) == U(0x7fffff)
    assert np.array_equal(mask != 0, want)
    # a length whose significand is all ones (1 - 2^-24 is one of the few floats a unit normal's length can be) stays on the short path: the stage takes its
    # reciprocal in closed form (exact_div.h xd_rcp_all_ones) where the guarded code divides
    # (about one such row in fifteen: (v + u) + w with w = 1 - u - v rounds to 1 - 2^-24 that often; 34 expected among the 512)
    assert (all_ones & want & wall).sum() >= 8, int((all_ones & want & wall).sum())
    assert {0, 1, WAVE} <= wave_failures(mask)
    assert mask[5 * WAVE + 3] == 0 and mask[9 * WAVE + 11] == 0
    # ordinary rows: unit normals, and the quotients nu / div, nv / div correctly rounded
    assert np.array_equal(staged[:WAVE, 0].view(F), (nu[:WAVE] / div[:WAVE]).astype(F)) and np.array_equal(staged[:WAVE, 1].view(F), (nv[:WAVE] / div[:WAVE]).astype(F))
    assert np.allclose(np.linalg.norm(staged[:WAVE, 2:5].view(F).astype(np.float64), axis=1), 1.0, atol=1e-6)


def stage3_rows(seed=4):
    r = np.random.default_rng(seed)
    rows = np.zeros((ROWS, 16), F)
    rows[:, 0:3] = unit_vectors(r, ROWS)                                  # the shading normal
    wall = (np.arange(ROWS) // WAVE % 4 == 0) & (np.arange(ROWS) % WAVE < WAVE // 2)      # half of every ordinary wave, 512 rows: a wall's normal, one of the six
    rows[wall, 0:3] = np.eye(3, dtype=F)[np.arange(ROWS)[wall] % 3] * np.where(np.arange(ROWS)[wall] % 2, F(-1), F(1))[:, None]      # axis directions
    rows[:, 3:6] = r.uniform(0.05, 0.95, (ROWS, 3))                      # albedo
    rows[:, 6:9] = r.uniform(0.05, 1.0, (ROWS, 3))                       # throughput
    rows[:, 9:11] = r.integers(1, 1 << 24, (ROWS, 2)).astype(U).view(F)  # the variates' 24 bits, as words
    rows[:, 11] = r.uniform(0.0, 0.2, ROWS)                               # the roulette's variate: most paths live
    # (a NaN in the normal fails the tangent frame's or wi's root; one in a single colour component can lose every compare-select and pass)
    waves_with_edges(rows, [0, 1, 2, 3, 4, 5, 6, 7, 8, 11], np.array([np.nan], F), failing_operands=[0, 1, 2])
    return rows


def test_continue_stage_equals_path_continue(X):
    rows = stage3_rows()
    words = rows.view(U)
    words[13 * WAVE + 5, 9] = 0                       # e0 = 0: the variate root's guard, one row of a wave
    words[17 * WAVE + 9, 9] = (1 << 24) - 1           # e0 = 1 - 2^-24, e1 = 0: the ends of the variates' range, inside every guard
    words[17 * WAVE + 9, 10] = 0
    rows[21 * WAVE + 1, 0:3] = (0.0, 0.0, 1.0)        # an axis-aligned normal: wi gets components of exactly 0 only beside a zero sine, which passes
    rows[25 * WAVE + 2, 0:3] = (1e-30, 0.0, 0.0)      # normals that are not of unit length: the tangent frame's and the normalisation's roots leave their range
    rows[29 * WAVE + 3, 0:3] = (1e30, 1e30, 1e30)
    rows[33 * WAVE + 4, 6:9] = (-0.5, -0.25, -1.0)    # a negative throughput with a roulette variate below it: roulette_scale's lower bound
    rows[33 * WAVE + 4, 11] = -2.0
    rows[37 * WAVE + 6, 3:6] = 0.0                    # a black surface: the throughput becomes 0, which roulette_scale admits
    for drops in (0, 1):
        staged, guarded, mask, full = X.run(3, drops, rows)
        assert same_words(staged[:, :7], guarded[:, :7]), drops      # (the guarded form is path_continue itself)
        assert np.array_equal(mask, full), drops     # the range tests that were left out change no row's mask
        # the mask is 0 on exactly the rows where a site's own guard fails: the guards as the guarded helpers make them, a bit per site, from the kernel's
        # restatement over the plain helpers (unit_kernels.hip) -- all but bit 5, the all-ones test of wi's length, which a stage replaces by the closed form
        bits = guarded[:, 7]
        assert np.array_equal(mask != 0, (bits | U(32)) == U(0x1ff)), drops
        # and such lengths are common where the tangent frame is orthonormal, as it is about a wall's normal: wi's vector is then nearly a unit vector, whose
        # length is 1 - 2^-24 in three cases of ten (profiles/shade_stages/ab.md). At least one in twenty of the 512 wall rows; all of them pass
        wall = (np.arange(ROWS) // WAVE % 4 == 0) & (np.arange(ROWS) % WAVE < WAVE // 2)
        assert (((bits & U(32)) == 0) & wall).sum() >= 512 // 20, (drops, int((((bits & U(32)) == 0) & wall).sum()))
        for bit in (0, 2, 3, 4, 8):                                      # every site that a row here can fail does fail somewhere
            assert ((bits >> U(bit)) & U(1) == 0).any(), (drops, bit)
        assert {0, 1, WAVE} <= wave_failures(mask)
        assert (mask.reshape(-1, WAVE)[0::4] != 0).all()                      # ordinary waves pass whole
        assert (mask.reshape(-1, WAVE)[3::4] == 0).all()                      # a NaN in the normal fails its row
        for row in (13 * WAVE + 5, 25 * WAVE + 2, 29 * WAVE + 3, 33 * WAVE + 4):
            assert mask[row] == 0, (drops, row)
        for row in (17 * WAVE + 9, 37 * WAVE + 6):
            assert mask[row] != 0, (drops, row)
        # ordinary rows: wi is a unit vector in the normal's hemisphere and the path lives or dies by the roulette alone
        wi = staged[:WAVE, 0:3].view(F).astype(np.float64)
        assert np.allclose(np.linalg.norm(wi, axis=1), 1.0, atol=1e-6) and ((wi * rows[:WAVE, 0:3]).sum(axis=1) > 0).all()
        assert set(staged[:, 6].tolist()) <= {0, int(F(1.0).view(U))}


def test_no_infinite_direction_reaches_the_next_ray(X):
    """The next ray's stage leaves out its upper bound (exact_div.h xd_rcp_unit_ok), which rests on this: whatever vertex normals a scene has, the direction the
    continuation hands on has no infinite component. Chained as the render loop chains them: stage 2's normal -- from vertex normals with zero, denormal, tiny,
    huge, infinite and NaN components, whole vectors of them included -- is stage 3's shading normal. (A normal that no normalisation can return, such as
    ( 1e-30, 0, 0 ), does give an infinity: the statement is about the loop's data, and so is this test.)"""
    r = np.random.default_rng(5)
    rows2 = np.zeros((ROWS, 16), F)
    rows2[:, 2] = r.uniform(0.5, 4.0, ROWS)
    rows2[:, 0] = r.uniform(0.05, 0.45, ROWS) * rows2[:, 2]; rows2[:, 1] = r.uniform(0.05, 0.45, ROWS) * rows2[:, 2]
    base = unit_vectors(r, ROWS)
    tiny = np.array([0.0, -0.0, 1e-45, 1e-40, 1e-30, 2.0 ** -50, 2.0 ** -63, 1e-20, 1.0, -1.0, 1e20, 2.0 ** 63, 2.0 ** 64, 3e38, np.inf, -np.inf, np.nan], F)
    for k in range(3):
        rows2[:, 3 + 3 * k:6 + 3 * k] = base
    scale = tiny[np.arange(ROWS) % len(tiny)]
    whole = np.arange(ROWS) % 3 == 0                                      # every third row: the three vertex normals scaled whole
    rows2[whole, 3:12] = rows2[whole, 3:12] * scale[whole, None]
    one = np.arange(ROWS) % 3 == 1                                        # every third: one component of each vertex normal replaced
    col = 3 + (np.arange(ROWS) // 3) % 3
    for k in range(3):
        rows2[one, col[one] + 3 * k] = scale[one]
    axis = np.arange(ROWS) % 3 == 2                                       # every third: normals along one axis, scaled (two components exactly zero)
    rows2[axis, 3:12] = 0.0
    for k in range(3):
        rows2[axis, col[axis] + 3 * k] = scale[axis]
    with np.errstate(all="ignore"):
        staged2, guarded2, mask2, _ = X.run(2, 0, rows2)
    assert same_words(staged2, guarded2)
    normals = guarded2[:, 2:5].view(F)
    assert np.isinf(normals).any() and np.isnan(normals).any() and (normals == 0).any()          # the degenerate normals are there
    rows3 = stage3_rows(seed=6)
    rows3[:, 0:3] = normals
    for drops in (0, 1):
        staged3, guarded3, mask3, _ = X.run(3, drops, rows3)
        assert same_words(staged3[:, :7], guarded3[:, :7]), drops
        assert not np.isinf(guarded3[:, 0:3].view(F)).any() and not np.isinf(staged3[:, 0:3].view(F)).any(), drops


def test_variate_roots_need_no_range_test(X):
    """sqrt ( e ) for e = k 2^-24 needs k != 0 and nothing else, sqrt ( sel_max ( 0, 1 - e ) ) needs no test: all 2^24 variates against sqrt_exact. And the
    reciprocal of an all-ones significand in closed form: all 242 of them inside the guarded range, and 2^24 hashed numerators over them"""
    assert X.variate_roots() == 0


# ---- frames that take the second run ----------------------------------------------------------------------------------------------------------------------------
SIMPLE, DIRECT = api.kTerraIntegratorSimple, api.kTerraIntegratorDirect


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def axis_camera(integ, width, height, jitter):
    # (the Cornell box's camera looks along +z with up = +y: its frame is the identity, so a film position of 0 is a direction component of +0)
    return scenes.cornell_box(width, height, 8, integrator=integ, jitter=jitter)


def scaled_cornell(integ):
    d = scenes.cornell_box(64, 48, 8, integrator=integ)
    s = F(2.0 ** 18)
    for ob in d.objects:
        ob.triangles = (np.asarray(ob.triangles, F) * s).astype(F)
    d.camera_position = tuple(float(F(c) * s) for c in d.camera_position)
    return d


@pytest.mark.parametrize("integ", [SIMPLE, DIRECT], ids=["simple", "direct"])
@pytest.mark.parametrize("shape", [(64, 48, 0.5), (65, 49, 0.0)], ids=["64x48", "65x49-no-jitter"])
def test_axis_camera_frame_equals_oracle(G, H, orc_lib, integ, shape):
    mk = lambda: axis_camera(integ, *shape)
    got = dev(G, mk(), 1)
    assert (got["samples"] == 8).all() and got["acc"].sum() > 0
    assert equals_oracle(got, oracle(H, mk()))


def edge_wall(integ):
    """The Cornell box without its short box (24 triangles: the launch keeps the pair form), its back wall two quads (a, b, c, d) = fans (a, b, c), (a, c, d) with
    a = (0, 0, 1), b = (0, 2, 1): the edge a-b is the line x = 0 of the wall. 65 x 49, no jitter: the centre column's film position is exactly 0
    ((32 + 0.5) / 65 = 0.5), the camera stands at x = 0 and its frame is the identity, so those rays have d.x = +0 and every point on them has x = 0 exactly.
    On the wall such a point is on the edge a-b of both fans' first triangles: p = point - a = (0, py, pz), e0 = b - a = (0, 2, 0), e1 = c - a = (+-1, 2, 0), so
    dp0 = dp1 = 2 py bit for bit (the other terms are zeros), d00 = d01 = 4, and nv = d00 dp1 - d01 dp0 = 0 exactly: surface_init's numerator test fails in those
    lanes, and in no other lane of their waves."""
    d = scenes.cornell_box(65, 49, 8, integrator=integ, jitter=0.0)
    floor = scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))
    ceiling = scenes._quad((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1), (0, -1, 0))
    right = scenes._quad((0, 0, 1), (0, 2, 1), (1, 2, 1), (1, 0, 1), (0, 0, -1))
    left = scenes._quad((0, 0, 1), (0, 2, 1), (-1, 2, 1), (-1, 0, 1), (0, 0, -1))
    d.objects[0] = scenes.ObjectDesc(*scenes._merge([floor, ceiling, right, left]), scenes.Material(albedo=(0.73, 0.73, 0.73)), "white")
    d.objects = [ob for ob in d.objects if ob.name != "short_box"]
    assert d.triangle_count == 24
    return d


@pytest.mark.parametrize("integ", [SIMPLE, DIRECT], ids=["simple", "direct"])
def test_hits_on_a_shared_edge_frame_equals_oracle(G, H, orc_lib, integ):
    # the film position of the centre column, as camera_film forms it in float32
    assert F(2) * (F(32 + 0.5) / F(65)) - F(1) == 0
    # ... and the centre column's rays do reach the wall: from ( 0, 1, -3.4 ) a ray ( 0, fy, 1 ) meets z = 1 at y = 1 + 4.4 fy, and nothing else of the scene
    # touches the plane x = 0 below y = 1.99 (the tall box ends at x = -0.15; the light lies at y = 1.99). Rows that arrive well inside the wall's height:
    tan = np.tan(np.float64(F(45.0) * F(0.0174533)) / 2)
    y_wall = 1 + 4.4 * (1 - 2 * (np.arange(49) + 0.5) / 49) * tan
    assert ((y_wall > 0.05) & (y_wall < 1.9)).sum() >= 20
    got = pairs_dev(G, edge_wall(integ), 1)
    assert got["used"] and (got["samples"] == 8).all() and got["acc"].sum() > 0          # (the pair form, whose launches stage the constants surface_stage reads)
    assert equals_oracle(got, oracle(H, edge_wall(integ)))


def stage_info(G, d):
    f = G.fn("terra_amd_shade_stage_info", C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int)])
    cam = scenes.camera_of(d); out = C.c_int(-1)
    assert f(C.addressof(cam), d.width, d.height, C.byref(out)) == 0, runtime.last_error()
    return out.value


@pytest.mark.parametrize("integ", [SIMPLE, DIRECT], ids=["simple", "direct"])
def test_launch_outside_the_camera_limits_keeps_every_test(G, H, orc_lib, integ):
    """a field of view of 10^-8 degrees: tan_half_fov = 8.7e-11 is below 2^-30, just outside what the host admits (at 1.1e-7 degrees it is inside). The launch
    reports the guarded ray start and renders the oracle's frame; the ordinary camera reports the stages"""
    # (aimed at the ceiling light, which all of its nearly parallel rays then hit: the frame is not black)
    mk = lambda: scenes.cornell_box(64, 48, 8, integrator=integ, camera_fov=1e-8, camera_direction=(0.0, 0.99, 3.4))
    assert stage_info(G, mk()) == 1 and stage_info(G, scenes.cornell_box(64, 48, 8, camera_fov=1.1e-7)) == 0 and stage_info(G, scenes.cornell_box(64, 48, 8)) == 0
    got = dev(G, mk(), 1)
    assert (got["samples"] == 8).all() and got["acc"].sum() > 0
    assert equals_oracle(got, oracle(H, mk()))


@pytest.mark.parametrize("integ", [SIMPLE, DIRECT], ids=["simple", "direct"])
def test_barycentric_fallback_frame_equals_oracle(G, H, orc_lib, integ):
    mk = lambda: scaled_cornell(integ)
    got = dev(G, mk(), 1)
    assert (got["samples"] == 8).all()
    assert equals_oracle(got, oracle(H, mk()))
