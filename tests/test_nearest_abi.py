"""Nearest-surface queries at the C boundary and as a rule, without a GPU: the three entry points are exported, TerraAmdNearestQuery / TerraAmdNearest have the layout
include/terra_amd.h pins -- in C (a gcc-compiled probe of the header) and in the ctypes and numpy mirrors of terra_amd/api.py --, an uncommitted scene is refused,
and the numpy statement of the rule (tests/nearest_ref.py, the reference of the GPU tests) answers hand-made triangles as the header says."""
import ctypes as C
import subprocess

import numpy as np

import nearest_ref
from terra_amd import api, runtime

QUERY = {"position": 0, "max_distance": 12}
NEAREST = {"distance": 0, "object": 4, "triangle": 8, "feature": 12, "point": 16, "side": 28}
SYMBOLS = ("terra_amd_nearest_device", "terra_amd_nearest", "terra_amd_unit_nearest_brute")
ERR_NOT_COMMITTED = -2
FLT_MAX = np.finfo(np.float32).max


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.NEAREST_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        assert callable(getattr(lib, name[len("terra_amd_"):])), name


def test_layouts_in_c_ctypes_and_numpy(H, tmp_path):
    assert C.sizeof(api.TerraAmdNearestQuery) == 16 and C.sizeof(api.TerraAmdNearest) == 32 and api.NEAREST_QUERY_DTYPE.itemsize == 16 and api.NEAREST_DTYPE.itemsize == 32
    for struct, dtype, offsets in ((api.TerraAmdNearestQuery, api.NEAREST_QUERY_DTYPE, QUERY), (api.TerraAmdNearest, api.NEAREST_DTYPE, NEAREST)):
        assert [n for n, _ in struct._fields_] == list(offsets) == list(dtype.names)
        for f, off in offsets.items():
            assert getattr(struct, f).offset == off, f
            assert dtype.fields[f][1] == off, f
    assert api.NEAREST_DTYPE["object"] == np.int32 and api.NEAREST_DTYPE["triangle"] == np.uint32 and api.NEAREST_DTYPE["feature"] == np.uint32
    probe = (["sizeof ( TerraAmdNearestQuery )"] + [f"offsetof ( TerraAmdNearestQuery, {f} )" for f in QUERY] + ["sizeof ( TerraAmdNearest )"]
             + [f"offsetof ( TerraAmdNearest, {f} )" for f in NEAREST])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { printf ( "' + " ".join(["%zu"] * len(probe)) + '\\n", '
                   + ", ".join(probe) + " ); return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ["16"] + [str(v) for v in QUERY.values()] + ["32"] + [str(v) for v in NEAREST.values()]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == want


def test_uncommitted_scene_is_refused_without_a_device(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    q = nearest_ref.pack(np.zeros((4, 3), np.float32))
    out = np.zeros(4, api.NEAREST_DTYPE)
    try:
        for k, call in enumerate((lambda: lib.nearest_device(scene, q.ctypes.data, 4, out.ctypes.data, None), lambda: lib.nearest(scene, q.ctypes.data, 4, out.ctypes.data),
                                  lambda: lib.unit_nearest_brute(scene, q.ctypes.data, 4, out.ctypes.data), lambda: lib.nearest(scene, None, 4, None))):
            lib.clear_error()
            assert call() == ERR_NOT_COMMITTED, k                 # "not committed" comes first: before anything else is looked at
            assert runtime.last_error() != "", k
        assert not out.view(np.uint8).any()
    finally:
        lib.clear_error()
        lib.scene_destroy(scene)


# ---- the rule on hand-made triangles ----------------------------------------------------------------------------------------------------------------
T0 = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], np.float32)          # A, B, C counter-clockwise seen from +z: cross(ab, ac) = (0, 0, 4)
ONE = (np.zeros(1, np.int32), np.zeros(1, np.int32))


def ask(tris, p, R=np.inf, obj=None, idx=None):
    obj = np.zeros(len(tris), np.int32) if obj is None else obj
    idx = np.arange(len(tris), dtype=np.int32) if idx is None else idx
    return nearest_ref.nearest_one(np.asarray(tris, np.float32), obj, idx, np.asarray(p, np.float32), R)[:2]


def test_one_query_per_feature_code():
    cases = {0: ((0.5, 0.5, 1.0), (0.5, 0.5, 0.0), 1.0, 1.0),            # feature: (P, Q, distance, side)
             1: ((-1.0, -1.0, 0.0), (0.0, 0.0, 0.0), np.sqrt(2.0), 0.0),
             2: ((3.0, -1.0, 0.0), (2.0, 0.0, 0.0), np.sqrt(2.0), 0.0),
             3: ((-1.0, 3.0, 0.0), (0.0, 2.0, 0.0), np.sqrt(2.0), 0.0),
             4: ((1.0, -1.0, -1.0), (1.0, 0.0, 0.0), np.sqrt(2.0), -1.0),
             5: ((2.0, 2.0, 0.5), (1.0, 1.0, 0.0), 1.5, 1.0),
             6: ((-1.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0, 0.0)}
    for feature, (p, q, dist, side) in cases.items():
        rec, ties = ask(T0, p)
        assert rec["feature"] == feature and ties == 1, (feature, rec)
        assert rec["object"] == 0 and rec["triangle"] == 0
        assert np.array_equal(rec["point"], np.asarray(q, np.float32)), (feature, rec)
        assert rec["distance"] == np.float32(dist) and rec["side"] == side, (feature, rec)
    # the order of the regions: a point that satisfies both the vertex-A test and the edge tests is A's
    assert ask(T0, (0.0, 0.0, 0.0))[0]["feature"] == 1 and ask(T0, (0.0, 0.0, 0.0))[0]["distance"] == 0.0
    assert ask(T0, (2.0, 0.0, 0.0))[0]["feature"] == 2 and ask(T0, (0.0, 2.0, 0.0))[0]["feature"] == 3
    assert ask(T0, (1.0, 0.0, 0.0))[0]["feature"] == 4                    # on the edge AB itself: vc == 0


def test_degenerate_triangles():
    # a zero-length edge (A == B): d1 = d3 = 0 and vc = 0, so region 3 takes the point, its quotient's divisor is exactly 0 and v = 0: the rule answers A -- a
    # finite answer on the triangle, not the nearest point of the segment A C (the rule is Ericson's, degenerate cases included, not a geometric promise)
    t = np.array([[[0, 0, 0], [0, 0, 0], [0, 2, 0]]], np.float32)
    rec, _ = ask(t, (1.0, 1.0, 0.0))
    assert rec["feature"] == 4 and rec["distance"] == np.float32(np.sqrt(2.0)) and np.array_equal(rec["point"], np.zeros(3, np.float32)), rec
    assert ask(t, (1.0, -1.0, 0.0))[0]["feature"] == 1
    # ... and C == A: region 5's divisor is 0 the same way
    t = np.array([[[0, 0, 0], [2, 0, 0], [0, 0, 0]]], np.float32)
    rec, _ = ask(t, (1.0, 1.0, 0.0))
    assert np.isfinite(rec["distance"]) and rec["object"] == 0 and rec["distance"] == 1.0 and rec["feature"] == 4, rec
    # all three vertices the same: every d is d1, region 1 or 2 takes it; never NaN
    t = np.array([[[1, 1, 1], [1, 1, 1], [1, 1, 1]]], np.float32)
    for p in ((0, 0, 0), (2, 2, 2), (1, 1, 1), (3, 0, 1)):
        rec, _ = ask(t, p)
        assert rec["object"] == 0 and np.array_equal(rec["point"], np.ones(3, np.float32)) and rec["feature"] in (1, 2), (p, rec)
    # a zero-area triangle (A, B, C on a line, B between): va = vb = vc = 0 exactly for these coordinates, so an edge region takes every point above the segment
    t = np.array([[[0, 0, 0], [1, 0, 0], [2, 0, 0]]], np.float32)
    rec, _ = ask(t, (0.5, 1.0, 0.0))
    assert rec["feature"] in (4, 5, 6) and rec["distance"] == 1.0 and np.array_equal(rec["point"], np.array([0.5, 0, 0], np.float32)) and rec["side"] == 0.0, rec
    rec, _ = ask(t, (3.0, 0.0, 0.0))
    assert rec["distance"] == 1.0 and np.array_equal(rec["point"], np.array([2, 0, 0], np.float32)), rec
    # a NaN vertex: every comparison is false, the face formula gives NaN, the triangle does not count -- and does not hide the one behind it
    t = np.array([[[0, 0, 0], [1, 0, np.nan], [0, 1, 0]], [[0, 0, 5], [1, 0, 5], [0, 1, 5]]], np.float32)
    rec, ties = ask(t, (0.2, 0.2, 1.0))
    assert rec["triangle"] == 1 and rec["distance"] == 4.0 and ties == 1, rec
    miss, ties = ask(t[:1], (0.2, 0.2, 1.0))
    assert ties == 0 and miss["object"] == -1 and miss["distance"] == FLT_MAX and (miss["point"] == FLT_MAX).all() and miss["triangle"] == 0 and miss["feature"] == 0 and miss["side"] == 0


def test_a_tie_goes_to_the_smaller_pair():
    # two triangles that share the edge (0,0,0)-(0,2,0); a point beside... on the plane through the edge that both see at the same distance
    a = [[0, 0, 0], [2, 0, 0], [0, 2, 0]]
    b = [[0, 0, 0], [0, 2, 0], [-2, 0, 0]]
    p = (0.0, 1.0, 1.0)                                                  # closest point (0, 1, 0), on the shared edge, for both
    for order, obj, idx, want in (((a, b), (0, 0), (0, 1), (0, 0)), ((a, b), (1, 0), (0, 5), (0, 5)), ((a, b), (2, 2), (7, 3), (2, 3)), ((b, a), (0, 0), (1, 0), (0, 0))):
        rec, ties = ask(np.array(order, np.float32), p, obj=np.array(obj, np.int32), idx=np.array(idx, np.int32))
        assert ties == 2 and (rec["object"], rec["triangle"]) == want and rec["distance"] == 1.0, (obj, idx, rec)


def test_limits_and_positions():
    p = (0.5, 0.5, 3.0)                                                  # distance exactly 3
    for R in (3.0, 3.5, np.inf, np.nan, FLT_MAX):
        assert ask(T0, p, R)[0]["distance"] == 3.0, R
    for R in (np.nextafter(np.float32(3.0), np.float32(0)), 1.5, 0.0, -0.5, -np.inf):
        assert ask(T0, p, R)[0]["object"] == -1, R
    assert ask(T0, (0.5, 0.5, 0.0), 0.0)[0]["distance"] == 0.0 and ask(T0, (0.5, 0.5, 0.0), -0.0)[0]["object"] == 0        # a limit of 0 (or -0) admits a point on the surface
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        for R in (np.inf, 1.0, np.nan):
            assert ask(T0, bad, R)[0]["object"] == -1
    far, _ = ask(T0, (3e38, 0.0, 0.0))                                   # finite, however far: answered (binary64 holds the square)
    assert far["object"] == 0 and far["distance"] == np.float32(3e38) and far["feature"] == 2
