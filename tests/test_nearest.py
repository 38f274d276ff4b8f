"""Nearest-surface queries (include/terra_amd.h "Nearest-surface queries"): terra_amd_nearest* against the numpy statement of the rule (tests/nearest_ref.py) and
the fast-tree kernel against the brute-force kernel (terra_amd_unit_nearest_brute). Every comparison is on bits, every field.

Query sets (per scene): uniform points in the scene's box grown by 1 on every side, plus constructed vertex queries (a vertex pushed away from its triangle's
centroid). Cornell: 2,048 + 16 against numpy in tree modes 0 and 2 (brute force) and 1 (fast tree on 32 triangles). Hall (97k triangles, fast tree): 128 + 8 against
numpy (0.04 s per query), 4,096 fast tree == brute force; the hall x 100 (reachability boxes) the same; points up to 10^6 out on one axis. The conditions on a set
-- enough faces, edges, vertices and ties -- are asserted on the numpy answers alone."""
import ctypes as C
import time

import numpy as np
import pytest

import nearest_ref
from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
SCALE = {"cornell": 1.0, "hall": 1.0, "hall_x100": 100.0}
SEED = {"cornell": 51, "hall": 52, "hall_x100": 53}
N_REF = {"cornell": 2048, "hall": 128}
N_VERTEX = {"cornell": 16, "hall": 8}
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4
CANARY = 0x5ca1ab1e


@pytest.fixture(scope="module")
def L(amd_lib):
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def desc(name):
    if name == "cornell":
        return scenes.cornell_box(16, 16, 1)
    d = scenes.sponza_hall(32, 18, 1)
    if name == "hall_x100":
        from tools.scaled_hall import scaled
        d = scaled(d, 100.0)
    return d


_soup = {}


def soup(name):
    """(triangles (m, 3, 3), object of each, index in its object) in the order the scene holds them"""
    if name not in _soup:
        d = desc(name)
        tris = np.concatenate([np.asarray(ob.triangles, np.float32).reshape(-1, 3, 3) for ob in d.objects])
        obj = np.concatenate([np.full(len(ob.triangles), k, np.int32) for k, ob in enumerate(d.objects)])
        idx = np.concatenate([np.arange(len(ob.triangles), dtype=np.int32) for ob in d.objects])
        _soup[name] = (np.ascontiguousarray(tris), obj, idx)
    return _soup[name]


def uniform_points(name, n, seed):
    """n points, uniform in the scene's box grown by 1 (by the scene's scale) on every side"""
    tris = soup(name)[0].reshape(-1, 3).astype(np.float64)
    k = SCALE[name]
    lo, hi = tris.min(axis=0) - k, tris.max(axis=0) + k
    return (lo + (hi - lo) * np.random.default_rng(seed).uniform(0, 1, size=(n, 3))).astype(np.float32)


def vertex_points(name, n, seed):
    """constructed vertex queries: a vertex of a triangle pushed away from that triangle's centroid"""
    tris = soup(name)[0]
    r = np.random.default_rng(seed)
    t, v = r.integers(0, len(tris), size=n), r.integers(0, 3, size=n)
    vert = tris[t, v].astype(np.float64)
    return (vert + 0.25 * (vert - tris[t].astype(np.float64).mean(axis=1))).astype(np.float32)


_reference = {}


def reference(name):
    """the scene's reference query set and the numpy rule's answers, computed once: (points, records, ties, D2). The conditions on the set are asserted here, on
    these answers alone: at least 25 % faces, 10 % edges, 3 % vertices, 10 % ties (more than one triangle at the minimal D2) -- the constructed vertex queries are
    ADDED to the uniform ones, none is dropped."""
    if name not in _reference:
        tris, obj, idx = soup(name)
        pts = np.concatenate([uniform_points(name, N_REF[name], SEED[name]), vertex_points(name, N_VERTEX[name], SEED[name] + 100)])
        rec, ties, d2 = nearest_ref.nearest(tris, obj, idx, nearest_ref.pack(pts))
        assert (rec["object"] >= 0).all() and (rec["distance"] > 0).mean() > 0.9          # (a constructed query may land on a neighbouring coplanar triangle: distance 0)
        f = rec["feature"]
        share = {"faces": (f == 0).mean(), "vertices": ((f >= 1) & (f <= 3)).mean(), "edges": (f >= 4).mean(), "ties": (ties > 1).mean()}
        print(name, {k: round(float(v), 3) for k, v in share.items()})
        assert share["faces"] >= 0.25 and share["edges"] >= 0.10 and share["vertices"] >= 0.03 and share["ties"] >= 0.10, (name, share)
        _reference[name] = (pts, rec, ties, d2)
    return _reference[name]


_scenes = {}


@pytest.fixture(scope="module")
def device_scene(L):
    def get(name, mode):
        if (name, mode) not in _scenes:
            L.clear_error()
            s = scenes.build_scene(L, desc(name), tree_mode=mode)
            assert runtime.last_error() == "", runtime.last_error()
            ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
            assert ti.fast_tree == (1 if (mode == 1 or name != "cornell") else 0), (name, mode, ti.note)      # which kernel answers: the fast tree's, or the brute force
            if name == "hall_x100": assert b"reachability" in ti.note, ti.note
            _scenes[(name, mode)] = s
        return _scenes[(name, mode)]
    yield get
    for s in _scenes.values():
        L.scene_destroy(s)
    _scenes.clear()


def to_device(q):
    import torch
    return torch.from_numpy(q.view(np.float32).reshape(-1, 4).copy()).cuda()


def ask(L, scene, pts, R=INF):
    """the tensor form"""
    return runtime.nearest(L, scene, to_device(nearest_ref.pack(pts, R))).cpu().numpy().view(api.NEAREST_DTYPE).reshape(-1)


def brute(L, scene, pts, R=INF):
    q = nearest_ref.pack(pts, R)
    out = np.zeros(len(q), api.NEAREST_DTYPE)
    assert L.unit_nearest_brute(scene, q.ctypes.data, len(q), out.ctypes.data) == 0, runtime.last_error()
    return out


def miss_records(n):
    out = np.zeros(n, api.NEAREST_DTYPE)
    out["distance"] = FLT_MAX; out["object"] = -1; out["point"] = FLT_MAX
    return out


def assert_same_records(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


# ---- 1. / 2. the rule, bit for bit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("cornell", 0), ("cornell", 1), ("cornell", 2), ("hall", 2)])
def test_equals_the_rule_bit_for_bit(L, device_scene, name, mode):
    pts, rec, ties, _ = reference(name)
    got = ask(L, device_scene(name, mode), pts)
    assert_same_records(got, rec, (name, mode))
    tied = ties > 1                                                              # the winner of a tie is the smaller pair: part of the records, said once more
    assert tied.any() and np.array_equal(got["object"][tied], rec["object"][tied]) and np.array_equal(got["triangle"][tied], rec["triangle"][tied])


@pytest.mark.parametrize("name", ["cornell", "hall", "hall_x100"])
def test_fast_tree_equals_the_brute_force(L, device_scene, name):
    scene = device_scene(name, 1 if name == "cornell" else 2)
    pts = np.concatenate([uniform_points(name, 4096, SEED[name] + 1), vertex_points(name, 64, SEED[name] + 2)])
    want = brute(L, scene, pts)
    assert (want["object"] >= 0).all()
    assert_same_records(ask(L, scene, pts), want, name)
    # ... and under a limit that cuts about half of them off
    R = np.float32(np.median(want["distance"]))
    cut = brute(L, scene, pts, R)
    assert 0.25 <= (cut["object"] >= 0).mean() <= 0.75
    assert_same_records(ask(L, scene, pts, R), cut, (name, "limit"))


def test_points_far_from_the_hall(L, device_scene):
    """no camera_limit contract: points as far as 10^6 out on one axis, no limit"""
    scene = device_scene("hall", 2)
    pts = uniform_points("hall", 512, SEED["hall"] + 3)
    r = np.random.default_rng(SEED["hall"] + 4)
    axis, sign, mag = r.integers(0, 3, size=512), r.choice([-1.0, 1.0], size=512), 10.0 ** r.uniform(1, 6, size=512)
    mag[:8] = 1e6
    pts[np.arange(512), axis] += (sign * mag).astype(np.float32)
    want = brute(L, scene, pts)
    assert (want["object"] >= 0).all() and want["distance"].max() > 9e5
    assert_same_records(ask(L, scene, pts), want, "far")


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("cornell", 2), ("cornell", 1), ("hall", 2)])
def test_the_limit(L, device_scene, name, mode):
    pts, rec, _, d2 = reference(name)
    scene = device_scene(name, mode)
    dist = rec["distance"]
    misses = miss_records(len(pts))
    up = np.nextafter(dist, INF)
    for what, R in (("the float above", up), ("exactly the distance", dist), ("the float below", np.nextafter(dist, np.float32(0))), ("half", np.float32(0.5) * dist)):
        # D2 <= (double) R * (double) R decides for the winner, and with it for every triangle: none has a smaller D2. distance = (float) sqrt(D2) is ROUNDED:
        # where it was rounded down, a limit of exactly the distance squares to less than D2 and the rule says miss; where it was rounded up or is exact,
        # found. So "exactly the distance" is held to the rule record by record (both outcomes must occur), the float above is always found, half never.
        found = d2 <= R.astype(np.float64) * R.astype(np.float64)
        want = rec.copy(); want[~found] = misses[~found]
        if what == "the float above": assert found.all()
        if what == "exactly the distance": assert found.any() and not found.all(), found.mean()
        if what == "the float below": assert not found.all()
        if what == "half": assert np.array_equal(found, d2 == 0)          # (a point ON the surface is within any limit >= 0)
        assert_same_records(ask(L, scene, pts, R), want, what)
    assert_same_records(ask(L, scene, pts, np.float32(-1.0)), misses, "negative")
    assert_same_records(ask(L, scene, pts, -INF), misses, "-inf")
    for R in (np.float32(np.nan), INF, FLT_MAX):
        assert_same_records(ask(L, scene, pts, R), rec, R)
    bad = pts[:96].copy()
    for i in range(96):
        bad[i, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    for R in (INF, np.float32(np.nan), FLT_MAX, np.float32(1.0), np.float32(-1.0), np.float32(0.0)):
        assert_same_records(ask(L, scene, bad, R), miss_records(96), ("non-finite position", R))


# ---- 5. the stack's HBM part ----------------------------------------------------------------------------------------------------------------------------------
def test_the_spill(L, device_scene):
    import torch
    pts, rec, _, _ = reference("hall")
    scene = device_scene("hall", 2)
    more = uniform_points("hall", 4096, SEED["hall"] + 1)
    want_more = ask(L, scene, more)
    runtime.check(L.debug_fast_stack_lds(scene, 2))
    try:
        assert_same_records(ask(L, scene, pts), rec, "two stack entries in LDS")
        # two calls back to back on a stream of their own, nothing in between: the spill of the first must outlive its kernel and no longer
        ta, tb = to_device(nearest_ref.pack(more)), to_device(nearest_ref.pack(more[::-1]))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ha = runtime.nearest(L, scene, ta); hb = runtime.nearest(L, scene, tb)
        side.synchronize()
        ha, hb = (x.cpu().numpy().view(api.NEAREST_DTYPE).reshape(-1) for x in (ha, hb))
        assert_same_records(ha, want_more, "first"); assert_same_records(hb, want_more[::-1], "second")
    finally:
        L.debug_fast_stack_lds(scene, 0)


def test_a_padded_stack_beyond_64_kb(L, device_scene):
    """debug_pad_stack adds LDS stack entries to a fast-tree plan: above 64 KB the launcher opts in, as the ray query's does"""
    pts, rec, _, _ = reference("cornell")
    scene = device_scene("cornell", 1)
    runtime.check(L.debug_pad_stack(scene, 70))
    try:
        L.clear_error()
        assert_same_records(ask(L, scene, pts), rec, "70 more stack entries")
        assert runtime.last_error() == ""
    finally:
        L.debug_pad_stack(scene, 0)
    assert_same_records(ask(L, scene, pts), rec, "the plan restored")


# ---- 6. edges of the call -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_edges_of_the_call(L, device_scene, mode):
    import torch
    pts, rec, _, _ = reference("cornell")
    scene = device_scene("cornell", mode)
    R = np.where(np.arange(300) % 3 == 0, np.float32(0.3), INF).astype(np.float32)          # a limit on every third query
    q = nearest_ref.pack(pts[:300], R)
    t = to_device(q)
    base = runtime.nearest(L, scene, t).cpu().numpy().view(api.NEAREST_DTYPE).reshape(-1)
    assert (base["object"] < 0).any() and (base["object"][np.arange(300) % 3 != 0] >= 0).all()
    assert runtime.nearest(L, scene, t).cpu().numpy().tobytes() == base.tobytes()            # again: the same bits
    canary = lambda n: torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    for n in (0, 1, 257):
        out = canary(8 * (n + 1))
        L.clear_error()
        assert L.nearest_device(scene, t.data_ptr(), n, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        out = out.cpu().numpy()
        assert (out[8 * n:] == CANARY).all(), n                                              # nothing past the last record (n = 0: nothing at all)
        assert out[:8 * n].tobytes() == base[:n].tobytes(), n
    assert L.nearest_device(scene, None, 0, None, None) == 0 and L.nearest(scene, None, 0, None) == 0 and L.unit_nearest_brute(scene, None, 0, None) == 0
    host = np.zeros(300, api.NEAREST_DTYPE)                                                  # host, device and tensor forms agree
    assert L.nearest(scene, q.ctypes.data, 300, host.ctypes.data) == 0, runtime.last_error()
    assert host.tobytes() == base.tobytes()
    assert_same_records(brute(L, scene, pts[:300], R), base, "brute")
    # failures: the documented status, a message, nothing launched
    fresh = L.scene_create()
    out = canary(8 * 4)
    host4 = np.zeros(4, api.NEAREST_DTYPE)
    calls = {
        "uncommitted": (ERR_NOT_COMMITTED, [lambda: L.nearest_device(fresh, t.data_ptr(), 4, out.data_ptr(), None), lambda: L.nearest(fresh, q.ctypes.data, 4, host4.ctypes.data),
                                            lambda: L.unit_nearest_brute(fresh, q.ctypes.data, 4, host4.ctypes.data)]),
        "null queries": (ERR_BAD_ARGUMENT, [lambda: L.nearest_device(scene, None, 4, out.data_ptr(), None), lambda: L.nearest(scene, None, 4, host4.ctypes.data),
                                            lambda: L.unit_nearest_brute(scene, None, 4, host4.ctypes.data)]),
        "null output": (ERR_BAD_ARGUMENT, [lambda: L.nearest_device(scene, t.data_ptr(), 4, None, None), lambda: L.nearest(scene, q.ctypes.data, 4, None),
                                           lambda: L.unit_nearest_brute(scene, q.ctypes.data, 4, None)]),
        "n = 2^31": (ERR_BAD_ARGUMENT, [lambda: L.nearest_device(scene, t.data_ptr(), 1 << 31, out.data_ptr(), None), lambda: L.nearest(scene, q.ctypes.data, 1 << 31, host4.ctypes.data),
                                        lambda: L.unit_nearest_brute(scene, q.ctypes.data, 1 << 31, host4.ctypes.data)]),
    }
    for what, (status, fs) in calls.items():
        for k, f in enumerate(fs):
            L.clear_error()
            assert f() == status, (what, k)
            assert runtime.last_error() != "", (what, k)
    L.clear_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all() and not host4.view(np.uint8).any()
    L.scene_destroy(fresh)


def test_stats_and_a_framebuffer_are_untouched(H, L, device_scene):
    import torch
    pts = reference("cornell")[0]
    scene = device_scene("cornell", 2)
    dsc = desc("cornell"); cam = scenes.camera_of(dsc)
    fb = runtime.DeviceFramebuffer(dsc.width, dsc.height)
    runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    before = (fb.pixels_host().copy(), fb.results_host().copy())
    stats = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(stats))); stats = stats.as_dict()
    ask(L, scene, pts); brute(L, scene, pts[:64])
    after = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(after)))
    assert after.as_dict() == stats                                                          # the queries record nothing
    assert H.same_bits(fb.pixels_host(), before[0]) and fb.results_host().tobytes() == before[1].tobytes()
    fb.clear(); runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    assert H.same_bits(fb.pixels_host(), before[0]) and fb.results_host().tobytes() == before[1].tobytes()


# ---- 7. the helpers -------------------------------------------------------------------------------------------------------------------------------------------
def test_distance_field_and_probe_clearance(L, device_scene):
    import torch
    scene = device_scene("cornell", 2)
    tris = soup("cornell")[0].reshape(-1, 3)
    lo, hi = tris.min(axis=0), tris.max(axis=0)
    dims = (8, 8, 8)
    spacing = ((hi - lo) / np.asarray(dims, np.float32)).astype(np.float32)
    q = runtime.distance_field_points(lo, spacing, dims)
    assert q.shape == (8, 8, 8) and np.array_equal(q["position"][3, 2, 1], ((np.array([1, 2, 3], np.float32) + np.float32(0.5)) * spacing + lo).astype(np.float32))
    direct = ask(L, scene, q["position"].reshape(-1, 3))
    runtime.distance_field(L, scene, lo, spacing, dims); torch.cuda.synchronize()            # (first call: allocations)
    t0 = time.perf_counter()
    field = runtime.distance_field(L, scene, lo, spacing, dims)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.25                                                   # "well under a second": upload, one launch of 512 queries, synchronise
    assert tuple(field.shape) == (8, 8, 8) and field.dtype == torch.float32
    assert field.cpu().numpy().tobytes() == direct["distance"].tobytes()
    signed = runtime.distance_field(L, scene, lo, spacing, dims, signed=True).cpu().numpy().reshape(-1)
    want = np.where(direct["feature"] == 0, direct["distance"] * np.where(direct["side"] != 0, direct["side"], np.float32(1)), direct["distance"]).astype(np.float32)
    assert (direct["feature"] == 0).any() and (direct["feature"] != 0).any() and signed.tobytes() == want.tobytes()
    limited = runtime.distance_field(L, scene, lo, spacing, dims, max_distance=0.2).cpu().numpy().reshape(-1)
    cut = ask(L, scene, q["position"].reshape(-1, 3), np.float32(0.2))
    assert (limited == FLT_MAX).any() and (limited != FLT_MAX).any() and limited.tobytes() == cut["distance"].tobytes()
    # probe_clearance: TerraAmdPoint records in, distance and closest point out
    probes = np.zeros(100, api.POINT_DTYPE)
    probes["position"] = reference("cornell")[0][:100]; probes["normal"] = (0, 1, 0)
    dist, point = runtime.probe_clearance(L, scene, torch.from_numpy(probes.view(np.float32).reshape(-1, 8).copy()).cuda())
    want = reference("cornell")[1][:100]
    assert dist.cpu().numpy().tobytes() == want["distance"].tobytes() and point.cpu().numpy().tobytes() == np.ascontiguousarray(want["point"]).tobytes()
