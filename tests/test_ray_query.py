"""Batched ray queries (include/terra_amd.h "Ray queries"): terra_amd_intersect* / terra_amd_occluded* against the oracle's reference traversal, the unit-level
replica traversal and a brute force over the oracle's watertight test. Every comparison is on bits.

Ray sets (per scene, from harness.scene_rays over a box that contains the scene): 4,096 + 37 rays (the last block is partial), 200 rays with one or two zero
direction components, 64 rays that start on a vertex and run along an edge of its triangle (depth ties), 64 rays with directions scaled x 0.01 and x 100.
Scenes: the Cornell box in tree mode 0 (replica), 1 (fast tree) and 2 (automatic: reference tree + leaf-box cull), the 97k-triangle hall (fast tree) and the hall
x 100 (fast tree + reachability replay). Every query() below also asserts occluded == (intersect.object >= 0) and the form of the records."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
BOXES = {"cornell": ((-1.2, -0.2, -3.5), (1.2, 2.2, 1.2)), "hall": ((-9.5, 0.3, -4.5), (9.5, 7.5, 4.5)), "hall_x100": ((-9.5, 0.3, -4.5), (9.5, 7.5, 4.5))}
SCALE = {"cornell": 1.0, "hall": 1.0, "hall_x100": 100.0}
SEED = {"cornell": 41, "hall": 42, "hall_x100": 43}
CASES = [("cornell", 0), ("cornell", 1), ("cornell", 2), ("hall", 2), ("hall_x100", 2)]
N_MAIN = 4096 + 37
# The hall is a closed room: of the rays that start inside the box above 99.7 % hit, whatever the seed. The condition "at least 10 % of the rays miss" is met by
# ADDING rays that start around the hall, inside the +-13 units the commit's containment proof covers (TerraAmdTraversalInfo::camera_limit); no ray is dropped.
OUTER, N_OUTER = ((-12.5, -4.0, -12.5), (12.5, 12.5, 12.5)), 2048
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4


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


def soup(d):
    """(triangles (m, 3, 3), object of each, index in its object) in the order the scene holds them"""
    tris = np.concatenate([np.asarray(ob.triangles, np.float32).reshape(-1, 3, 3) for ob in d.objects])
    obj = np.concatenate([np.full(len(ob.triangles), k, np.int32) for k, ob in enumerate(d.objects)])
    idx = np.concatenate([np.arange(len(ob.triangles), dtype=np.int32) for ob in d.objects])
    return np.ascontiguousarray(tris), obj, idx


def ray_set(H, name):
    d = desc(name)
    tris, _, _ = soup(d)
    box, k, seed = BOXES[name], np.float32(SCALE[name]), SEED[name]
    r = np.random.default_rng(seed)
    o, dd = H.scene_rays(seed, N_MAIN, box=box)
    oz, dz = H.scene_rays(seed + 100, 200, box=box)
    for i in range(200):                                     # one zero component; the second hundred: two
        a = r.integers(0, 3); dz[i, a] = 0.0
        if i >= 100: dz[i, (a + 1 + r.integers(0, 2)) % 3] = 0.0
        if not dz[i].any(): dz[i, (a + 1) % 3] = 1.0
    dz /= np.linalg.norm(dz, axis=1, keepdims=True)
    if name != "cornell":                                    # the hall is closed: rays from around it (see OUTER) bring the misses
        oo, do = H.scene_rays(seed + 200, N_OUTER, box=OUTER)
        o = np.concatenate([o, oo]); dd = np.concatenate([dd, do])
    o = o * k; oz = oz * k                                   # (the scaled hall: origins move with the scene, directions stay)
    t = r.integers(0, len(tris), size=64)                    # on a vertex, along an edge of its triangle: ties at depth 0 between the triangles that share it
    ov, dv = tris[t, 0].copy(), (tris[t, 1] - tris[t, 0]).astype(np.float32)
    assert dv.any(axis=1).all()
    ou, du = o[:64].copy(), dd[:64].copy()
    du[:32] *= np.float32(0.01); du[32:] *= np.float32(100.0)
    o = np.concatenate([o, oz, ov, ou]); dd = np.concatenate([dd, dz, dv, du])
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(dd, np.float32)


_oracle, _scenes = {}, {}


def oracle(H, name):
    """rays of the scene and the oracle's reference traversal of them, computed once; the conditions on the ray set are asserted on these answers alone"""
    if name not in _oracle:
        u = H.Unit("orc")
        sc = scenes.build_scene(u.L, desc(name))
        o, d = ray_set(H, name)
        found, prim, point = u.bvh_traverse(sc, o, d)
        u.L.scene_destroy(sc)
        frac = float((found != 0).mean())
        assert 0.1 <= frac <= 0.9, (name, frac)              # at least 10 % of the rays hit and at least 10 % miss
        _oracle[name] = (o, d, found, prim, point)
    return _oracle[name]


@pytest.fixture(scope="module")
def device_scene(L):
    def get(name, mode):
        if (name, mode) not in _scenes:
            L.clear_error()
            s = scenes.build_scene(L, desc(name), tree_mode=mode)
            assert runtime.last_error() == "", runtime.last_error()
            ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
            assert ti.fast_tree == (1 if (mode == 1 or name != "cornell") else 0), (name, mode, ti.note)
            if name == "hall_x100": assert b"reachability" in ti.note, ti.note
            _scenes[(name, mode)] = s
        return _scenes[(name, mode)]
    yield get
    for s in _scenes.values():
        L.scene_destroy(s)
    _scenes.clear()


def pack(o, d, tmax):
    rays = np.zeros(len(o), api.RAY_DTYPE)
    rays["origin"] = o; rays["direction"] = d; rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    return rays


def to_device(rays):
    import torch
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()


def check_records(H, hits, o, d):
    hit = hits["object"] >= 0
    miss = ~hit
    assert not hits["reserved"].any() and not hits["reserved2"].view(np.uint32).any()
    assert (hits["object"][miss] == -1).all() and (hits["triangle"][miss] == 0).all()
    assert (hits["t"][miss] == FLT_MAX).all() and (hits["point"][miss] == FLT_MAX).all()
    with np.errstate(over="ignore", invalid="ignore"):                       # (the misses' FLT_MAX; not compared)
        want = (o + d * hits["t"][:, None]).astype(np.float32)              # float32: multiply, then add
    assert H.same_bits(hits["point"][hit], want[hit])


def query(H, L, scene, o, d, tmax):
    """both queries of one ray set through the tensor forms; occlusion must be the closest hit's "hit" element for element"""
    t = to_device(pack(o, d, tmax))
    hits = runtime.intersect(L, scene, t).cpu().numpy().view(api.HIT_DTYPE).reshape(-1)
    occ = runtime.occluded(L, scene, t).cpu().numpy()
    assert occ.dtype == np.int32 and np.array_equal(occ, (hits["object"] >= 0).astype(np.int32))
    check_records(H, hits, o, d)
    return hits


def assert_matches_traversal(H, hits, found, prim, point, what):
    hit = found != 0
    assert np.array_equal(hit, hits["object"] >= 0), what
    assert np.array_equal(hits["object"][hit].astype(np.int64), (prim[hit] & 0xff).astype(np.int64)), what
    assert np.array_equal(hits["triangle"][hit].astype(np.int64), (prim[hit] >> 8).astype(np.int64)), what
    assert H.same_bits(hits["point"][hit], point[hit]), what


# ---- 1. closest hit equals the reference, everywhere ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", CASES)
def test_closest_hit_equals_the_reference(H, L, orc_lib, device_scene, name, mode):
    o, d, found, prim, point = oracle(H, name)
    scene = device_scene(name, mode)
    hits = query(H, L, scene, o, d, INF)
    assert_matches_traversal(H, hits, found, prim, point, "oracle")
    assert_matches_traversal(H, hits, *H.Unit("amd").bvh_traverse(scene, o, d), "terra_amd_unit_bvh_traverse")


# ---- 2. the limit ----------------------------------------------------------------------------------------------------------------------------------
def depth_matrix(H, o, d, tris):
    """orc_watertight of every ray on every triangle: (n, m) depths, NaN where the test rejects"""
    f = H.lib("orc").fn("orc_watertight", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32); tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    out = np.zeros(8, np.float32)
    D = np.full((len(o), len(tris)), np.nan, np.float32)
    po, pd, pt, pout = o.ctypes.data, d.ctypes.data, tris.ctypes.data, out.ctypes.data
    for i in range(len(o)):
        for j in range(len(tris)):
            if f(po + 12 * i, pd + 12 * i, pt + 36 * j, pout):
                D[i, j] = out[3]
    return D


def brute_force(D, ranks, limit):
    """(hit, triangle, depth): the minimum over the triangles with a depth <= limit of (depth, reference visit rank)"""
    counts = ~np.isnan(D) & (D <= np.broadcast_to(np.asarray(limit, np.float32), (len(D),))[:, None])
    depth = np.where(counts, D, INF).min(axis=1)
    first = np.where(counts & (D == depth[:, None]), ranks[None, :].astype(np.int64), 1 << 40).argmin(axis=1)
    return counts.any(axis=1), first, depth


def leaf_ranks(L, scene, n):
    f = L.fn("terra_amd_scene_leaf_ranks", C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    out = np.zeros(n, np.uint32)
    assert f(scene, out.ctypes.data, n) == n
    return out


def assert_is_brute_force(hits, D, ranks, limit, obj, idx, what):
    hit, tri, depth = brute_force(D, ranks, limit)
    assert np.array_equal(hit, hits["object"] >= 0), what
    assert np.array_equal(hits["object"][hit], obj[tri[hit]]) and np.array_equal(hits["triangle"][hit], idx[tri[hit]]), what
    assert np.array_equal(hits["t"][hit].view(np.uint32), depth[hit].view(np.uint32)), what


_depths = {}


def cornell_depths(H):
    if "D" not in _depths:
        o, d = oracle(H, "cornell")[:2]
        _depths["D"] = depth_matrix(H, o, d, soup(desc("cornell"))[0])
    return _depths["D"]


@pytest.mark.parametrize("name", ["cornell", "hall"])
def test_the_limit(H, L, orc_lib, device_scene, name):
    o, d = oracle(H, name)[:2]
    scene = device_scene(name, 2)
    base = query(H, L, scene, o, d, INF)
    hit, t = base["object"] >= 0, base["t"]
    lim = lambda v: np.where(hit, v, INF).astype(np.float32)
    limits = {"t": lim(t), "below t": lim(np.nextafter(t, np.float32(0))), "half t": lim(np.float32(0.5) * t)}
    got = {k: query(H, L, scene, o, d, v) for k, v in limits.items()}
    assert got["t"].tobytes() == base.tobytes()                              # a limit of exactly the depth: the same hit
    for k in ("below t", "half t"):                                          # below it: a miss, or a hit within the limit; a miss stays a miss
        h = got[k]
        assert ((h["object"] < 0) | (h["t"] <= limits[k])).all() and (h["object"][~hit] < 0).all(), k
    if name == "cornell":
        _, obj, idx = soup(desc(name))
        D, ranks = cornell_depths(H), leaf_ranks(L, scene, len(obj))
        assert_is_brute_force(base, D, ranks, FLT_MAX, obj, idx, "no limit")
        for k, v in limits.items():
            assert_is_brute_force(got[k], D, ranks, np.minimum(v, FLT_MAX), obj, idx, k)
    for tm in (FLT_MAX, INF, np.float32(np.nan)):                            # all three: no limit
        assert query(H, L, scene, o, d, tm).tobytes() == base.tobytes(), tm
    assert (query(H, L, scene, o, d, np.float32(-1.0))["object"] < 0).all()  # a negative limit: every ray misses


# ---- 3. occlusion (query() asserts it against the closest hit for every ray set and limit above) ------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_segments_between_points_against_the_brute_force(H, L, orc_lib, device_scene, mode):
    r = H.rng(7)
    lo, hi = np.array([-0.95, 0.05, -0.95], np.float32), np.array([0.95, 1.95, 0.95], np.float32)
    a = (lo + (hi - lo) * r.uniform(0, 1, size=(2048, 3))).astype(np.float32)
    b = (lo + (hi - lo) * r.uniform(0, 1, size=(2048, 3))).astype(np.float32)
    d = (b - a).astype(np.float32)
    if "seg" not in _depths:
        _depths["seg"] = depth_matrix(H, a, d, soup(desc("cornell"))[0])
    D = _depths["seg"]
    blocked = (~np.isnan(D) & (D <= np.float32(1.0))).any(axis=1)
    assert 0.1 <= blocked.mean() <= 0.9, blocked.mean()                      # at least 10 % blocked and at least 10 % clear
    hits = query(H, L, device_scene("cornell", mode), a, d, np.float32(1.0))
    assert np.array_equal(hits["object"] >= 0, blocked)


# ---- 4. deep stacks and the HBM spill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,pad,fast_lds", [("hall", 2, 0, 2), ("cornell", 0, 60, 0), ("cornell", 1, 60, 2), ("cornell", 2, 60, 0)])
def test_deep_stacks_and_the_spill(H, L, orc_lib, device_scene, name, mode, pad, fast_lds):
    import torch
    o, d, found, prim, point = oracle(H, name)
    scene = device_scene(name, mode)
    runtime.check(L.debug_pad_stack(scene, pad)); runtime.check(L.debug_fast_stack_lds(scene, fast_lds))
    try:
        assert_matches_traversal(H, query(H, L, scene, o, d, INF), found, prim, point, "oracle")
        # two queries back to back on a stream of their own, nothing in between: the spill of the first must outlive its kernel and no longer
        ta, tb = to_device(pack(o, d, INF)), to_device(pack(o[::-1], d[::-1], INF))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ha = runtime.intersect(L, scene, ta); hb = runtime.intersect(L, scene, tb); oa = runtime.occluded(L, scene, ta)
        side.synchronize()
        ha, hb = (x.cpu().numpy().view(api.HIT_DTYPE).reshape(-1) for x in (ha, hb))
        assert_matches_traversal(H, ha, found, prim, point, "first")
        assert_matches_traversal(H, hb, found[::-1], prim[::-1], point[::-1], "second")
        assert np.array_equal(oa.cpu().numpy() != 0, found != 0)
    finally:
        L.debug_pad_stack(scene, 0); L.debug_fast_stack_lds(scene, 0)


# ---- 5. edges of the call -----------------------------------------------------------------------------------------------------------------------------------
CANARY = 0x5ca1ab1e


def test_edges_of_the_call(H, L, orc_lib, device_scene):
    import torch
    o, d = oracle(H, "cornell")[:2]
    scene = device_scene("cornell", 2)
    base = query(H, L, scene, o[:300], d[:300], INF)
    rays = to_device(pack(o[:300], d[:300], INF))
    canary = lambda n: torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    for n in (0, 1, 257):
        hits, occ = canary(8 * (n + 1)), canary(n + 1)
        L.clear_error()
        assert L.intersect_device(scene, rays.data_ptr(), n, hits.data_ptr(), None) == 0 and L.occluded_device(scene, rays.data_ptr(), n, occ.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        hits, occ = hits.cpu().numpy(), occ.cpu().numpy()
        assert (hits[8 * n:] == CANARY).all() and (occ[n:] == CANARY).all(), n       # nothing past the last record (n = 0: nothing at all)
        assert hits[:8 * n].tobytes() == base[:n].tobytes() and np.array_equal(occ[:n], (base["object"][:n] >= 0).astype(np.int32)), n
    assert L.intersect_device(scene, None, 0, None, None) == 0 and L.occluded(scene, None, 0, None) == 0
    # failures: the documented status, a message, nothing launched
    fresh = L.scene_create()
    hits, occ = canary(8 * 4), canary(4)
    host_rays, host_hits, host_occ = pack(o[:4], d[:4], INF), np.zeros(4, api.HIT_DTYPE), np.zeros(4, np.uint32)
    calls = {
        "uncommitted": (ERR_NOT_COMMITTED, [lambda: L.intersect_device(fresh, rays.data_ptr(), 4, hits.data_ptr(), None), lambda: L.occluded_device(fresh, rays.data_ptr(), 4, occ.data_ptr(), None),
                                            lambda: L.intersect(fresh, host_rays.ctypes.data, 4, host_hits.ctypes.data), lambda: L.occluded(fresh, host_rays.ctypes.data, 4, host_occ.ctypes.data)]),
        "null rays": (ERR_BAD_ARGUMENT, [lambda: L.intersect_device(scene, None, 4, hits.data_ptr(), None), lambda: L.occluded_device(scene, None, 4, occ.data_ptr(), None),
                                         lambda: L.intersect(scene, None, 4, host_hits.ctypes.data), lambda: L.occluded(scene, None, 4, host_occ.ctypes.data)]),
        "null output": (ERR_BAD_ARGUMENT, [lambda: L.intersect_device(scene, rays.data_ptr(), 4, None, None), lambda: L.occluded_device(scene, rays.data_ptr(), 4, None, None),
                                           lambda: L.intersect(scene, host_rays.ctypes.data, 4, None), lambda: L.occluded(scene, host_rays.ctypes.data, 4, None)]),
        "n = 2^31": (ERR_BAD_ARGUMENT, [lambda: L.intersect_device(scene, rays.data_ptr(), 1 << 31, hits.data_ptr(), None), lambda: L.occluded_device(scene, rays.data_ptr(), 1 << 31, occ.data_ptr(), None),
                                        lambda: L.intersect(scene, host_rays.ctypes.data, 1 << 31, host_hits.ctypes.data), lambda: L.occluded(scene, host_rays.ctypes.data, 1 << 31, host_occ.ctypes.data)]),
    }
    for what, (status, fs) in calls.items():
        for k, f in enumerate(fs):
            L.clear_error()
            assert f() == status, (what, k)
            assert runtime.last_error() != "", (what, k)
    L.clear_error()
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == CANARY).all() and (occ.cpu().numpy() == CANARY).all() and not host_hits.view(np.uint8).any() and not host_occ.any()
    L.scene_destroy(fresh)


# ---- 6. independence and determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("cornell", 2), ("hall", 2)])
def test_forms_agree_and_nothing_else_changes(H, L, orc_lib, device_scene, name, mode):
    import torch
    o, d = oracle(H, name)[:2]
    scene = device_scene(name, mode)
    dsc = desc(name); cam = scenes.camera_of(dsc)
    fb = runtime.DeviceFramebuffer(dsc.width, dsc.height)
    runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    before = (fb.pixels_host().copy(), fb.results_host().copy())
    stats = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(stats))); stats = stats.as_dict()
    tmax = np.where(np.arange(len(o)) % 3 == 0, np.float32(2.0) * np.float32(SCALE[name]), INF).astype(np.float32)      # a limit on every third ray
    rays = pack(o, d, tmax)
    first = query(H, L, scene, o, d, tmax)                                                  # the tensor forms
    assert query(H, L, scene, o, d, tmax).tobytes() == first.tobytes()                      # again: the same bits
    t = to_device(rays)
    dev_hits = torch.zeros((len(o), 8), dtype=torch.float32, device="cuda"); dev_occ = torch.zeros(len(o), dtype=torch.int32, device="cuda")
    assert L.intersect_device(scene, t.data_ptr(), len(o), dev_hits.data_ptr(), None) == 0 and L.occluded_device(scene, t.data_ptr(), len(o), dev_occ.data_ptr(), None) == 0
    torch.cuda.synchronize()
    host_hits, host_occ = np.zeros(len(o), api.HIT_DTYPE), np.zeros(len(o), np.uint32)
    assert L.intersect(scene, rays.ctypes.data, len(o), host_hits.ctypes.data) == 0 and L.occluded(scene, rays.ctypes.data, len(o), host_occ.ctypes.data) == 0, runtime.last_error()
    assert dev_hits.cpu().numpy().tobytes() == first.tobytes() and host_hits.tobytes() == first.tobytes()
    want_occ = (first["object"] >= 0).astype(np.int32)
    assert np.array_equal(dev_occ.cpu().numpy(), want_occ) and np.array_equal(host_occ.astype(np.int32), want_occ)
    after = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(after)))
    assert after.as_dict() == stats                                                        # queries record nothing
    fb.clear(); runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    assert H.same_bits(fb.pixels_host(), before[0]) and fb.results_host().tobytes() == before[1].tobytes()
