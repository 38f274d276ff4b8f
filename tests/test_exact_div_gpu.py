"""The exact-quotient helpers of the shading code (csrc/exact_div.h: rcp_exact, div_exact_r, div_exact_rk, normalize on top of them) against the plain float
division, bit for bit, through terra_amd_unit_exact_div. The contract is "the bits `/` returns, for every input"; the helper's guards (2^-60 <= |operand| <= 2^60,
a reciprocal's denominator without an all-ones significand, a vector component +-0 or >= 2^-60) only choose between a short fma sequence and the plain division.

Per element the kernel computes the helper and `/` and compares the two 32-bit words there (two NaNs count as equal): the large sets -- all 2^32 patterns, 2 * 10^9
hashed pairs -- are generated on the device from a counter and come back as a mismatch count plus the first 16 offenders, which the assertion prints. The sets
built here (guard boundaries, special components) use the explicit form, which also returns both bit patterns: those are compared here with ==."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import runtime

pytestmark = pytest.mark.gpu

LO, HI = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
PI = np.float32(3.1416926535)          # the reference's terra_PI


@pytest.fixture(scope="module")
def X(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    f = lib.fn("terra_amd_unit_exact_div", C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_uint64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])

    def generated(op, count, first=0, d=0.0, r=0.0, seed=0):
        mism = np.zeros(1, np.uint64); bad = np.zeros((16, 9), np.uint32)
        rc = f(op, None, None, None, first, count, float(d), float(r), seed, None, None, mism.ctypes.data, bad.ctypes.data)
        assert rc == 0, runtime.last_error()
        return int(mism[0]), bad

    def explicit(op, a, b=None, c=None, d=0.0, r=0.0):
        arr = [np.ascontiguousarray(v, np.float32) if v is not None else None for v in (a, b, c)]
        n = arr[0].size; per = 3 if op == 4 else 1
        hb = np.zeros(n * per, np.uint32); pb = np.zeros(n * per, np.uint32)
        mism = np.zeros(1, np.uint64); bad = np.zeros((16, 9), np.uint32)
        rc = f(op, *[v.ctypes.data if v is not None else None for v in arr], 0, n, float(d), float(r), 0, hb.ctypes.data, pb.ctypes.data, mism.ctypes.data, bad.ctypes.data)
        assert rc == 0, runtime.last_error()
        return hb, pb, int(mism[0])

    class Entry:
        pass
    e = Entry(); e.generated = generated; e.explicit = explicit
    return e


def report(bad, n):
    rows = bad[:min(n, 16)]
    return "first offenders {inputs | helper | plain}: " + "; ".join(" ".join("%08x" % w for w in row) for row in rows)


def same_words(hb, pb):
    """== on the words; NaN results count as equal when both are NaN"""
    h, p = hb.view(np.float32), pb.view(np.float32)
    return np.array_equal(np.isnan(h), np.isnan(p)) and np.array_equal(hb[~np.isnan(h)], pb[~np.isnan(p)])


def neighbours(v):
    """v and the floats one ulp below and above it, both signs"""
    b = np.asarray(v, np.float32).view(np.uint32)
    m = np.concatenate([b - 1, b, b + 1]).astype(np.uint32)
    return np.concatenate([m, m | np.uint32(0x80000000)]).view(np.float32)


def test_rcp_exact_all_patterns(X):
    n, bad = X.generated(0, 1 << 32)
    assert n == 0, report(bad, n)


@pytest.mark.parametrize("d", [float(PI), 1920.0, 1080.0, 64.0, 48.0], ids=["terra_pi", "1920", "1080", "64", "48"])
def test_division_by_a_constant_all_numerators(X, d):
    d32 = np.float32(d); r32 = np.float32(1.0) / d32          # IEEE float32 division: the correctly rounded reciprocal, as the host forms it
    n, bad = X.generated(1, 1 << 32, d=d32, r=r32)
    assert n == 0, report(bad, n)


def test_a_wrong_reciprocal_is_caught(X):
    """positive control of the generated form's comparison. (A reciprocal a few ulps off would not do: the remainder step corrects the quotient all the same.
    One that is 2^-10 off leaves an error of 2^-20 after the correction, far above half an ulp.)"""
    r = np.float32(1.0009765625) / np.float32(1920.0)
    n, bad = X.generated(1, 1 << 24, first=0x3f800000, d=np.float32(1920.0), r=r)
    assert n > (1 << 23) and bad[0, 3] != bad[0, 6]


def test_pi_reciprocal_literal():
    assert float(np.float32(1.0) / PI) == float.fromhex("0x1.45f06p-2")          # TERRA_INV_PI_F (csrc/shading_device.h)


def test_two_operand_random_pairs(X):
    """2^31 hashed pairs: the even elements uniform in bit pattern (every fallback runs), the odd ones inside the guarded range (the short sequence runs)"""
    n, bad = X.generated(2, 1 << 31, seed=0x5eed)
    assert n == 0, report(bad, n)


def test_two_operand_directed_pairs(X):
    """4 * 10^6 elements x 3 pairs: x = RN(d (q + s ulp(q) / 2)), s = -1, 0, +1, and x's float neighbours -- exact quotients within a few 2^-48 (relative) of a
    rounding midpoint (s = +-1) or of a float (s = 0), on either side of it"""
    n, bad = X.generated(3, 4_000_000, seed=0xd1ec7ed)
    assert n == 0, report(bad, n)


def test_two_operand_guard_boundaries(X):
    """both operands at the ends of the guarded range +-1 ulp, zero, the smallest normal, denormals, the largest float, infinities, NaN, all-ones significands"""
    edge = np.concatenate([neighbours([LO, HI, 1.0, np.float32(2.0) - np.float32(2.0 ** -23), np.finfo(np.float32).tiny, np.finfo(np.float32).max, 2.0 ** -103, 2.0 ** -126 * 1.5]),
                           np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3e-39, float(PI), 1920.0, 0.75, -3.0], np.float32),
                           (np.arange(0x3f7ffffd, 0x3f800003, dtype=np.uint32)).view(np.float32), (np.arange(0x5d7ffffd, 0x5d800003, dtype=np.uint32)).view(np.float32),
                           (np.arange(0x217ffffd, 0x21800003, dtype=np.uint32)).view(np.float32)])
    x, d = [g.ravel() for g in np.meshgrid(edge, edge)]
    hb, pb, n = X.explicit(2, x, d)
    assert same_words(hb, pb) and n == 0
    hb, pb, n = X.explicit(0, edge)
    assert same_words(hb, pb) and n == 0
    for dc in (float(PI), 1920.0, float(LO), float(HI)):
        hb, pb, n = X.explicit(1, edge, d=np.float32(dc), r=np.float32(1.0) / np.float32(dc))
        assert same_words(hb, pb) and n == 0, dc


def test_normalize_random_vectors(X):
    n, bad = X.generated(4, 10_000_000, seed=0x0123)
    assert n == 0, report(bad, n)


def test_normalize_special_components(X):
    """every vector over a set of special components (+-0, denormals, the guard's ends +-1 ulp, huge, infinite, NaN) and ordinary ones: one, two or three of them special"""
    comp = np.concatenate([np.array([0.0, -0.0, 1e-45, -3e-39, 1e30, -3e38, np.inf, np.nan, 1.0, -0.5, 0.3, 1e-10, -1e10, 2.0 ** -30, 2.0 ** 30], np.float32), neighbours([LO, HI])])
    x, y, z = [g.ravel() for g in np.meshgrid(comp, comp, comp)]
    hb, pb, n = X.explicit(4, x, y, z)
    assert same_words(hb, pb) and n == 0
    # the short sequence really ran on the ordinary ones: a unit vector with a -0 component keeps the sign of its zero
    v = np.array([[0.0, -0.0, 2.0], [-0.0, 3.0, 4.0]], np.float32)
    hb, pb, n = X.explicit(4, v[:, 0], v[:, 1], v[:, 2])
    assert hb.reshape(2, 3).tolist() == [[0x00000000, 0x80000000, 0x3f800000], [0x80000000, np.float32(0.6).view(np.uint32), np.float32(0.8).view(np.uint32)]] and same_words(hb, pb)
