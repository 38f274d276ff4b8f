"""The short square root of the shading code (csrc/exact_sqrt.h sqrt_exact, normalize on top of it), the one-path tangent frame (trace_math.h make_basis) and the
short roulette rescale (exact_div.h roulette_scale) against their plain forms -- sqrtf, make_basis_plain, (float) (1.0 / ((double) pr + 1e-4)), normalize_plain --
bit for bit, through terra_amd_unit_exact_sqrt. The contract is "the bits the plain form returns, for every input"; the guards (a finite x >= 2^-96; 0 <= pr <=
2^60; normalize: the root's guard on the squared length, then the quotients' guard on the length) only choose between a short sequence and the plain one.

Per element the kernel computes both forms and compares the words there (two NaNs count as equal): the large sets -- all 2^32 patterns, hashed normals and vectors
-- are generated on the device from a counter and come back as a mismatch count plus the first 16 offenders, which the assertion prints. The sets built here
(guard boundaries, directed normals, special components) use the explicit form, which also returns both bit patterns: those are compared here with ==."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = np.finfo(F).max


@pytest.fixture(scope="module")
def X(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    f = lib.fn("terra_amd_unit_exact_sqrt", *api.EXACT_SQRT_SIGNATURES["terra_amd_unit_exact_sqrt"])

    def generated(op, count, first=0, seed=0):
        mism = np.zeros(1, np.uint64); bad = np.zeros((16, 21), np.uint32)
        rc = f(op, None, None, None, first, count, seed, None, None, mism.ctypes.data, bad.ctypes.data)
        assert rc == 0, runtime.last_error()
        return int(mism[0]), bad

    def explicit(op, a, b=None, c=None):
        arr = [np.ascontiguousarray(v, F) if v is not None else None for v in (a, b, c)]
        n = arr[0].size; per = {2: 9, 4: 3}.get(op, 1)
        hb = np.zeros(n * per, np.uint32); pb = np.zeros(n * per, np.uint32)
        mism = np.zeros(1, np.uint64); bad = np.zeros((16, 21), np.uint32)
        rc = f(op, *[v.ctypes.data if v is not None else None for v in arr], 0, n, 0, hb.ctypes.data, pb.ctypes.data, mism.ctypes.data, bad.ctypes.data)
        assert rc == 0, runtime.last_error()
        return hb, pb, int(mism[0])

    class Entry:
        pass
    e = Entry(); e.generated = generated; e.explicit = explicit
    return e


def report(bad, n):
    rows = bad[:min(n, 16)]
    return "first offenders {inputs[3] | helper[9] | plain[9]}: " + "; ".join(" ".join("%08x" % w for w in row) for row in rows)


def same_words(hb, pb):
    """== on the words; NaN results count as equal when both are NaN"""
    h, p = hb.view(F), pb.view(F)
    return np.array_equal(np.isnan(h), np.isnan(p)) and np.array_equal(hb[~np.isnan(h)], pb[~np.isnan(p)])


def neighbours(v):
    """v and the floats one ulp below and above it, both signs"""
    b = np.asarray(v, F).view(np.uint32)
    m = np.concatenate([b - 1, b, b + 1]).astype(np.uint32)
    return np.concatenate([m, m | np.uint32(0x80000000)]).view(F)


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3e-39, -3e-39, 1.0, -1.0, 0.25, 2.0, 3.0, -3.0, 1e-30, 1e30], F)


def test_sqrt_exact_all_patterns(X):
    n, bad = X.generated(0, 1 << 32)
    assert n == 0, report(bad, n)


def test_sqrt_guard_boundaries(X):
    """the guard's ends +-1 ulp (2^-96: the expansion's scale-up threshold; FLT_MAX, whose upper neighbour is +inf), the smallest normal, denormals, zeros, negative
    values, NaN, and a few exact and inexact roots"""
    edge = np.concatenate([neighbours([2.0 ** -96, FLT_MAX, np.finfo(F).tiny, 2.0 ** -126 * 1.5, 2.0 ** -140, 1.0, 4.0, 2.0, 2.0 ** 96, 2.0 ** -64]), SPECIAL])
    hb, pb, n = X.explicit(0, edge)
    assert same_words(hb, pb) and n == 0
    got = dict(zip(edge.view(np.uint32).tolist(), hb.tolist()))
    assert got[0x00000000] == 0x00000000 and got[0x80000000] == 0x80000000 and got[0x7f800000] == 0x7f800000          # +-0 and +inf return themselves
    assert got[F(4.0).view(np.uint32).item()] == F(2.0).view(np.uint32).item() and got[F(2.0 ** -96).view(np.uint32).item()] == F(2.0 ** -48).view(np.uint32).item()
    assert np.isnan(np.uint32(got[F(-1.0).view(np.uint32).item()]).view(F))


def test_a_wrong_core_is_caught(X):
    """positive control of the generated form's comparison: op 1 is the short root with the upper candidate dropped, so every input whose hardware estimate lies one
    unit below the correctly rounded root comes back wrong. Over one binade pair [1, 4) the estimate is low for a fraction of the inputs; all of them must be reported"""
    n, bad = X.generated(1, 1 << 24, first=0x3f800000)
    assert n > 0 and bad[0, 3] != bad[0, 12] and bad[0, 3] + 1 == bad[0, 12], (n, report(bad, n))
    assert X.generated(0, 1 << 24, first=0x3f800000)[0] == 0


def test_make_basis_generated_normals(X):
    """10^7 hashed normals: unit vectors, scaled by 1, 2^40 and 2^-40 (the root's argument leaves the guarded range at the lower end), every fourth uniform in bits"""
    n, bad = X.generated(2, 10_000_000, seed=0xba515)
    assert n == 0, report(bad, n)


def test_make_basis_directed_normals(X):
    """axis-aligned normals, |n.x| == |n.y| ties (the comparison is strict: a tie takes the second arm), +-0 components, NaN and infinite components"""
    comp = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, F(0.70710678), -F(0.70710678), 0.6, -0.8, np.inf, -np.inf, np.nan, 1e-30, -1e30, 3e-39, 2.0 ** -48, 2.0 ** -49], F)
    x, y, z = [g.ravel() for g in np.meshgrid(comp, comp, comp)]
    hb, pb, n = X.explicit(2, x, y, z)
    assert same_words(hb, pb) and n == 0
    # the two arms as the source writes them, on normals that are exact in float: n = (0.6, 0, 0.8) takes the first arm, (0, 0.6, 0.8) and the tie (0.6, 0.6, 0) the second
    v = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, -1.0, 0.0]], F)
    hb, pb, n = X.explicit(2, v[:, 0], v[:, 1], v[:, 2])
    t = hb.view(F).reshape(-1, 3, 3)[:, :, 0]          # the tangent: column 0 of the rows
    assert same_words(hb, pb) and n == 0
    assert t.tolist() == [[0.0, 0.0, -1.0], [0.0, -0.0, 1.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [0.0, -0.0, -1.0]]
    assert np.signbit(t[1, 1]) and np.signbit(t[4, 1]) and not np.signbit(t[0, 1])          # (-n.z) k = -0 in the second arm, 0 k = +0 in the first


def test_roulette_scale_all_patterns(X):
    n, bad = X.generated(3, 1 << 32)
    assert n == 0, report(bad, n)


def test_roulette_scale_guard_boundaries(X):
    edge = np.concatenate([neighbours([2.0 ** 60, 1e-4, 1.0, np.finfo(F).tiny, FLT_MAX]), SPECIAL])
    hb, pb, n = X.explicit(3, edge)
    assert same_words(hb, pb) and n == 0
    got = dict(zip(edge.view(np.uint32).tolist(), hb.tolist()))
    assert got[F(1.0).view(np.uint32).item()] == F(1.0 / (1.0 + 1e-4)).view(np.uint32).item() and got[0] == F(1.0 / 1e-4).view(np.uint32).item()


def test_normalize_generated_vectors(X):
    """10^7 hashed vectors: test_exact_div_gpu.py's set (every fourth uniform in bits) and, every eighth, components of magnitude 2^-49 .. 2^-47 or 2^47 .. 2^49, whose
    squared length falls on either side of 2^-96 (the root's guard) and of 2^96"""
    n, bad = X.generated(4, 10_000_000, seed=0x0123)
    assert n == 0, report(bad, n)


def test_normalize_special_components_and_guard_ends(X):
    """test_exact_div_gpu.py's special components, and the ends of the quotients' guard (l = 2^+-60) and of the root's (len^2 = 2^-96: l = 2^-48; 2^96 for symmetry) +-1 ulp"""
    comp = np.concatenate([np.array([0.0, -0.0, 1e-45, -3e-39, 1e30, -3e38, np.inf, np.nan, 1.0, -0.5, 0.3, 1e-10, -1e10, 2.0 ** -30, 2.0 ** 30], F),
                           neighbours([2.0 ** -60, 2.0 ** 60, 2.0 ** -48, 2.0 ** 48])])
    x, y, z = [g.ravel() for g in np.meshgrid(comp, comp, comp)]
    hb, pb, n = X.explicit(4, x, y, z)
    assert same_words(hb, pb) and n == 0
    # single-component vectors around the guard's ends: len^2 = c^2 on either side of 2^-96 and 2^96
    c = np.concatenate([neighbours([2.0 ** -48, 2.0 ** 48]), (np.arange(-4, 5) + int(F(2.0 ** -48).view(np.uint32))).astype(np.uint32).view(F),
                        (np.arange(-4, 5) + int(F(2.0 ** 48).view(np.uint32))).astype(np.uint32).view(F)])
    zero = np.zeros_like(c)
    for order in ((c, zero, zero), (zero, c, zero), (c, c, zero), (c, c, c)):
        hb, pb, n = X.explicit(4, *order)
        assert same_words(hb, pb) and n == 0
    # the short sequence really ran on the ordinary ones: a unit vector with a -0 component keeps the sign of its zero
    v = np.array([[0.0, -0.0, 2.0], [-0.0, 3.0, 4.0]], F)
    hb, pb, n = X.explicit(4, v[:, 0], v[:, 1], v[:, 2])
    assert hb.reshape(2, 3).tolist() == [[0x00000000, 0x80000000, 0x3f800000], [0x80000000, F(0.6).view(np.uint32), F(0.8).view(np.uint32)]] and same_words(hb, pb)
