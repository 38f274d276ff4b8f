"""Multi-hit ray queries at the C boundary and as a rule, without a GPU: the six entry points are exported and declared, bad arguments and an uncommitted scene
are refused with a message and nothing written, n == 0 succeeds, the CPU statement of the rule (tests/multi_hit_ref.py, the reference of the GPU tests) answers
hand-made triangles as the header says -- and THE CONDITIONS ON EVERY RAY SET of tests/test_multi_hit.py are asserted here, on the reference's answers alone."""
import ctypes as C
import re

import numpy as np

import multi_hit_ref as ref
from terra_amd import api, runtime, scenes

SYMBOLS = ("terra_amd_intersect_all_device", "terra_amd_intersect_all", "terra_amd_count_hits_device", "terra_amd_count_hits",
           "terra_amd_unit_intersect_all_brute", "terra_amd_unit_count_hits_brute")
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4


def test_new_symbols_are_exported_and_declared(H, amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.MULTI_HIT_SIGNATURES) == set(SYMBOLS) and api.MAX_HITS == 8
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        assert callable(getattr(lib, name[len("terra_amd_"):])), name
    header = (H.ROOT / "include" / "terra_amd.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+TERRA_AMD_MAX_HITS\s+8\b", header) and "Multi-hit ray queries" in header
    for fn in ("intersect_all", "count_hits", "inside"):
        assert callable(getattr(runtime, fn)), fn


def calls(lib, scene, rays, n, k, hits, counts):
    """every form with the given arguments: (name, call) -- the device forms are given the host addresses, which a refused call never looks at"""
    r = rays.ctypes.data if rays is not None else None
    h = hits.ctypes.data if hits is not None else None
    c = counts.ctypes.data if counts is not None else None
    return [("intersect_all_device", lambda: lib.intersect_all_device(scene, r, n, k, h, c, None)), ("intersect_all", lambda: lib.intersect_all(scene, r, n, k, h, c)),
            ("unit_intersect_all_brute", lambda: lib.unit_intersect_all_brute(scene, r, n, k, h, c)),
            ("count_hits_device", lambda: lib.count_hits_device(scene, r, n, c, None)), ("count_hits", lambda: lib.count_hits(scene, r, n, c)),
            ("unit_count_hits_brute", lambda: lib.unit_count_hits_brute(scene, r, n, c))]


def test_refused_calls_leave_a_message_and_write_nothing(amd_lib):
    lib = runtime.load(need_torch=False)
    fresh = lib.scene_create()
    committed = scenes.build_scene(lib, ref.cornell_desc())
    rays = np.zeros(4, api.RAY_DTYPE); rays["direction"] = (0, 0, 1); rays["tmax"] = np.inf
    hits = np.zeros((4, 8), api.HIT_DTYPE); counts = np.zeros(4, np.uint32)
    takes_k = lambda name: "intersect_all" in name

    def refused(what, status, scene, r, n, k, h, c, only=lambda name: True):
        for name, call in calls(lib, scene, r, n, k, h, c):
            if not only(name):
                continue
            lib.clear_error()
            assert call() == status, (what, name)
            assert runtime.last_error() != "", (what, name)
    try:
        refused("uncommitted", ERR_NOT_COMMITTED, fresh, rays, 4, 2, hits, counts)
        refused("uncommitted, everything else wrong too", ERR_NOT_COMMITTED, fresh, None, 1 << 31, 9, None, None)          # "not committed" comes first
        refused("K = 0", ERR_BAD_ARGUMENT, committed, rays, 4, 0, hits, counts, takes_k)
        refused("K = 9", ERR_BAD_ARGUMENT, committed, rays, 4, 9, hits, counts, takes_k)
        refused("K = 0 with n = 0", ERR_BAD_ARGUMENT, committed, rays, 0, 0, hits, counts, takes_k)
        refused("null rays", ERR_BAD_ARGUMENT, committed, None, 4, 2, hits, counts)
        refused("null hits", ERR_BAD_ARGUMENT, committed, rays, 4, 2, None, counts, takes_k)
        refused("null counts", ERR_BAD_ARGUMENT, committed, rays, 4, 2, hits, None, lambda name: "count_hits" in name)
        refused("n = 2^31", ERR_BAD_ARGUMENT, committed, rays, 1 << 31, 2, hits, counts)
        assert not hits.view(np.uint8).any() and not counts.any()
        # n == 0 succeeds and launches nothing (no device is needed for it), whatever the buffers
        for name, call in calls(lib, committed, None, 0, 3, None, None) + calls(lib, committed, rays, 0, 8, hits, counts):
            lib.clear_error()
            assert call() == 0 and runtime.last_error() == "", name
        assert not hits.view(np.uint8).any() and not counts.any()
    finally:
        lib.clear_error()
        lib.scene_destroy(fresh); lib.scene_destroy(committed)


def test_the_reference_checks_itself(H, orc_lib):
    ref.self_check(orc_lib)
    for a, b, c in runtime.INSIDE_DIRECTIONS:
        assert (48 * 48 + 64 * 64 + 60 * 60 == 100 * 100) and sorted(round(abs(v) * 100) for v in (a, b, c)) == [48, 60, 64]
    d = np.array(runtime.INSIDE_DIRECTIONS)
    assert np.abs((d * d).sum(axis=1) - 1.0).max() < 1e-15 and np.linalg.matrix_rank(d) == 3          # unit length, three different lines


# ---- the conditions on the ray sets -------------------------------------------------------------------------------------------------------------------
def test_conditions_on_the_cornell_sets(H, orc_lib, amd_lib):
    L = runtime.load(need_torch=False)
    c = ref.cornell_reference(H, L)
    assert len(c["o"]) == 4461 + 1024
    total = ref.totals(ref.ordered(c["rows"], c["o"], c["d"], ref.INF, c["ranks"]))
    print("cornell A", ref.histogram(total[:4461]), "B", ref.histogram(total[4461:]))
    ref.cornell_conditions(total)


def test_conditions_on_the_exact_tie_sets(H, orc_lib, amd_lib):
    L = runtime.load(need_torch=False)
    for name in ("seed-0", "big"):
        t = ref.tie_reference(H, L, name)
        assert len(t["o"]) == 2113 and len(t["obj"]) == (32 if name == "seed-0" else 80)
        rows = ref.ordered(t["rows"], t["o"], t["d"], ref.INF, t["ranks"])
        print(name, ref.histogram(ref.totals(rows)))
        ref.tie_conditions(name, rows)


def test_conditions_on_the_hall_sets_and_the_prefilter(H, orc_lib, amd_lib):
    L = runtime.load(need_torch=False)
    for which in ("inner", "outer"):
        h = ref.hall_reference(H, L, which, 128)
        assert len(h["tris"]) == 97478
        total = ref.totals(ref.ordered(h["rows"], h["o"], h["d"], ref.INF, h["ranks"]))
        print(which, "candidates per ray", ref.agrees_with_the_full_matrix(H, h, 8 if which == "inner" else 4), ">= 2", (total >= 2).mean(), "> 4", (total > 4).mean(), "max", total.max())
        ref.hall_conditions(total)
    h = ref.hall_reference(H, L, "outer", 64, 100.0)
    total = ref.totals(ref.ordered(h["rows"], h["o"], h["d"], ref.INF, h["ranks"]))
    print("x100 candidates per ray", ref.agrees_with_the_full_matrix(H, h, 2), ">= 2", (total >= 2).mean(), "> 4", (total > 4).mean())
    ref.hall_conditions(total)
