"""The start of a ray (csrc/trace_geometry.h ray_state_init and ray_start_masks, csrc/trace_math.h make_ray), restated on the host in float32.

* Two selections of the ray's axes: the integer form -- iz by the three comparisons, ix = iz + 1, iy = ix + 1 (mod 3), swapped when d[iz] < 0, every operand
  picked by index -- and the predicate form of ray_start_masks: z0, z1, flip, the component at iz by two selects, those at iz + 1 and iz + 2 by two selects each
  and two more that put the pair in order, the numbers (perm = 2 iz + flip, the word offsets) from the predicates and from perm's two tables. On every direction
  of {+-0, +-denormal, +-1, +-nextafter(1), +-2, +-inf, NaN}^3 -- 2,197 cases: all six (axis, sign) classes, every tie, a NaN in every place -- both must pick
  the same operands for the shear, the scale and the permuted origin, bit for bit.
* The implication the traversal entries rest on (trace_geometry.h "One range test per ray"): a direction component that passes exact_div.h's xd_rcp_ok has a
  reciprocal that passes ray_is_tame's test (and ray_is_regular's, which is wider). Held on 2^20 float patterns -- every exponent with sign, with the significands
  at both ends and random ones between -- and at the guard's own edges."""
import itertools

import numpy as np

f32, u32 = np.float32, np.uint32
DENORMAL = np.array([1], u32).view(f32)[0]
VALUES = [f32(0.0), f32(-0.0), DENORMAL, -DENORMAL, f32(1), f32(-1), np.nextafter(f32(1), f32(2)), -np.nextafter(f32(1), f32(2)), f32(2), f32(-2),
          f32(np.inf), f32(-np.inf), f32(np.nan)]


def directions():
    d = np.array(list(itertools.product(VALUES, repeat=3)), f32)
    assert d.shape == (13 ** 3, 3)
    return d


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def integer_form(d, inv, o):
    """the reference's selection (src/TerraGeometry.c), as the kernels ran it before: indices, then picks by index"""
    out = []
    for k in range(len(d)):
        ax, ay, az = np.abs(d[k])
        iz = (0 if ax > az else 2) if ax > ay else (1 if ay > az else 2)
        ix = 0 if iz + 1 == 3 else iz + 1
        iy = 0 if ix + 1 == 3 else ix + 1
        if d[k, iz] < 0:
            ix, iy = iy, ix
        perm = 2 * iz + int(ix != (0 if iz == 2 else iz + 1))
        out.append((d[k, ix], d[k, iy], inv[k, iz], o[k, ix], o[k, iy], o[k, iz], ix, iy, iz, perm))
    return out


def predicate_form(d, inv, o):
    """ray_start_masks: three predicates, picks by select, the numbers from perm"""
    sel = lambda c, a, b: a if c else b
    out = []
    for k in range(len(d)):
        ax, ay, az = np.abs(d[k])
        xy, xz, yz = bool(ax > ay), bool(ax > az), bool(ay > az)
        z0, z1 = xy and xz, (not xy) and yz
        pick_z = lambda a: sel(z0, a[0], sel(z1, a[1], a[2]))
        flip = bool(pick_z(d[k]) < 0)

        def pick_xy(a):
            u = sel(z0, a[1], sel(z1, a[2], a[0])); v = sel(z0, a[2], sel(z1, a[0], a[1]))
            return sel(flip, v, u), sel(flip, u, v)
        perm = sel(z0, 0, sel(z1, 2, 4)) + sel(flip, 1, 0)
        ix, iy, iz = (0x429 >> (2 * perm)) & 3, (0x186 >> (2 * perm)) & 3, perm >> 1
        dx, dy = pick_xy(d[k]); ox, oy = pick_xy(o[k])
        out.append((dx, dy, pick_z(inv[k]), ox, oy, pick_z(o[k]), ix, iy, iz, perm))
    return out


def test_both_selections_pick_the_same_operands():
    d = directions()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (f32(1) / d).astype(f32)
    # an origin with three different components, so that a wrong pick shows
    o = np.tile(np.array([0.25, 1.5, -3.0], f32), (len(d), 1))
    a, b = integer_form(d, inv, o), predicate_form(d, inv, o)
    classes = set()
    for k, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(bits(p[:6]), bits(q[:6])) and p[6:] == q[6:], (d[k], p, q)
        assert sorted(p[6:9]) == [0, 1, 2]
        classes.add(p[9])
        # the products the kernel forms of them: same operands, same operation
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.array_equal(bits([p[0] * p[2], p[1] * p[2]]), bits([q[0] * q[2], q[1] * q[2]]))
    assert classes == {0, 1, 2, 3, 4, 5}
    nan = np.isnan(d)
    assert nan.any(axis=1).sum() == 13 ** 3 - 12 ** 3 and (np.abs(d[:, 0]) == np.abs(d[:, 1])).sum() > 300      # NaNs in every place, ties


def xd_rcp_ok(d):
    """exact_div.h: normal, 2^-60 <= |d| <= 2^60, significand not all ones"""
    a = np.abs(d)
    with np.errstate(invalid="ignore"):
        return (a >= f32(2.0 ** -60)) & (a <= f32(2.0 ** 60)) & ((bits(d) & u32(0x7fffff)) != u32(0x7fffff))


def passes(inv, limit):
    """ray_is_regular (limit 0x7f7fffff) / ray_is_tame (0x6f7fffff) on one component: bits without the sign, minus one, below the limit -- in uint32, so that 0 wraps"""
    return ((bits(inv) & u32(0x7fffffff)) - u32(1)) < u32(limit)


def test_a_guarded_component_has_a_tame_reciprocal():
    r = np.random.default_rng(5)
    n = 1 << 20
    per = n // 512                                                        # 512 (sign, exponent) classes
    head = np.repeat(np.arange(512, dtype=u32) << u32(23), per)
    sig = r.integers(0, 1 << 23, size=n, dtype=np.uint32)
    sig.reshape(512, per)[:, :6] = np.array([0, 1, 2, 0x400000, 0x7ffffe, 0x7fffff], u32)      # both ends of every class
    d = (head | sig).view(f32)
    assert len(d) == n
    ok = xd_rcp_ok(d)
    assert 0.4 < ok.mean() < 0.5                                          # 121 of 256 exponents
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (f32(1) / d).astype(f32)                                    # the short sequence returns the quotient's bits (exact_div.h; all 2^32 patterns: test_exact_div_gpu.py)
    assert passes(inv[ok], 0x6f7fffff).all() and passes(inv[ok], 0x7f7fffff).all()
    lo, hi = bits(np.abs(inv[ok])).min(), bits(np.abs(inv[ok])).max()
    assert lo >= bits(f32(2.0 ** -60))[()] and hi <= bits(f32(2.0 ** 60))[()]
    # the second test is not idle: among the components the guard turns away some are tame and some are not
    assert passes(inv[~ok], 0x6f7fffff).any() and (~passes(inv[~ok], 0x6f7fffff)).any()
    # the guard's own edges
    edge = np.array([2.0 ** -60, 2.0 ** 60, -2.0 ** -60, -2.0 ** 60], f32)
    assert xd_rcp_ok(edge).all() and passes(f32(1) / edge, 0x6f7fffff).all()
    out = np.array([np.nextafter(f32(2.0 ** -60), f32(0)), np.nextafter(f32(2.0 ** 60), f32(np.inf)), np.nextafter(f32(1), f32(0)), 0.0, -0.0, DENORMAL, np.inf, np.nan], f32)
    assert not xd_rcp_ok(out).any()
