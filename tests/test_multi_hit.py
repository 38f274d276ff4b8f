"""Multi-hit ray queries (include/terra_amd.h "Multi-hit ray queries"): terra_amd_intersect_all* / terra_amd_count_hits* against the CPU statement of the rule
(tests/multi_hit_ref.py: the oracle's watertight test on every triangle, sorted by (depth, rank)), the fast-tree walk against the brute-force kernel
(terra_amd_unit_intersect_all_brute / terra_amd_unit_count_hits_brute) and K = 1 against the ray queries. Every comparison is on bits, every field.

Ray sets (tests/multi_hit_ref.py builds them; tests/test_multi_hit_abi.py asserts their conditions without a GPU, and every test here asserts them again before it
uses a set; no ray is ever dropped): Cornell A + B (5,485 rays; tree modes 0 and 2: brute force, mode 1: the fast tree on 32 triangles), the exact-tie scenes
seed-0 (brute force) and big (fast tree) under 2,113 rays that hit everything at depth 4.0, the hall (97k triangles, fast tree) from inside and from around it, and
the hall x 100 (reachability boxes)."""
import ctypes as C

import numpy as np
import pytest

import multi_hit_ref as ref
from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
CANARY = 0x5ca1ab1e
KS = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def L(amd_lib):
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def spheres_only():
    d = scenes.cornell_spheres(16, 16, 1)
    d.objects = d.objects[4:]
    return d


DESCS = {"cornell": ref.cornell_desc, "hall": ref.hall_desc, "hall_x100": lambda: ref.hall_desc(100.0), "spheres": lambda: scenes.cornell_spheres(16, 16, 1), "spheres_only": spheres_only}
_scenes = {}


@pytest.fixture(scope="module")
def device_scene(L):
    def get(name, mode=2):
        """the committed scene, and the assertion of WHICH kernel answers it: the fast tree's walk or the brute force (TerraAmdTraversalInfo::fast_tree)"""
        if (name, mode) not in _scenes:
            import exact_ties
            L.clear_error()
            d = exact_ties.scene(name) if name in exact_ties.SCENES else DESCS[name]()
            s = scenes.build_scene(L, d, tree_mode=mode)
            assert runtime.last_error() == "", runtime.last_error()
            ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
            fast = mode == 1 or name in ("hall", "hall_x100", "big")
            if not name.startswith("spheres"): assert ti.fast_tree == (1 if fast else 0), (name, mode, ti.note)
            if name == "hall_x100": assert b"reachability" in ti.note, ti.note
            _scenes[(name, mode)] = (s, float(ti.camera_limit))
        return _scenes[(name, mode)][0]
    yield get
    for s, _ in _scenes.values():
        L.scene_destroy(s)
    _scenes.clear()


def camera_limit(name, mode=2):
    return _scenes[(name, mode)][1]


def pack(o, d, tmax=INF):
    rays = np.zeros(len(o), api.RAY_DTYPE)
    rays["origin"] = o; rays["direction"] = d; rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    return rays


def to_device(rays):
    import torch
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()


def ask(L, scene, rays, k):
    """the tensor form: (hits [n, k] api.HIT_DTYPE, counts uint32 [n])"""
    hits, counts = runtime.intersect_all(L, scene, to_device(rays), k)
    assert tuple(hits.shape) == (len(rays), k, 8) and tuple(counts.shape) == (len(rays),)
    return hits.cpu().numpy().view(api.HIT_DTYPE).reshape(len(rays), k), counts.cpu().numpy().view(np.uint32)


def count(L, scene, rays):
    return runtime.count_hits(L, scene, to_device(rays)).cpu().numpy().view(np.uint32)


def brute(L, scene, rays, k):
    hits = np.zeros((len(rays), k), api.HIT_DTYPE); counts = np.zeros(len(rays), np.uint32)
    assert L.unit_intersect_all_brute(scene, rays.ctypes.data, len(rays), k, hits.ctypes.data, counts.ctypes.data) == 0, runtime.last_error()
    return hits, counts


def brute_count(L, scene, rays):
    counts = np.zeros(len(rays), np.uint32)
    assert L.unit_count_hits_brute(scene, rays.ctypes.data, len(rays), counts.ctypes.data) == 0, runtime.last_error()
    return counts


def assert_same(got, want, what):
    (gh, gc), (wh, wc) = got, want
    if gh.tobytes() != wh.tobytes():
        bad = np.argwhere((gh.view(np.uint32).reshape(gh.shape + (8,)) != wh.view(np.uint32).reshape(wh.shape + (8,))).any(axis=-1))
        i, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {gh.size} records differ, first ray {i} hit {j}: got {gh[i, j]}, want {wh[i, j]}")
    assert np.array_equal(gc, wc), (what, "counts", np.flatnonzero(gc != wc)[:8])


def against_the_rule(L, scene, r, ks, tmax=INF, what="", brute_too=True):
    """every K, its counts and the crossing count against the reference, through the tensor forms and (brute_too) the brute-force unit entries"""
    rows = ref.ordered(r["rows"], r["o"], r["d"], tmax, r["ranks"])
    rays = pack(r["o"], r["d"], tmax)
    total = ref.totals(rows)
    for k in ks:
        want = ref.records(rows, r["o"], r["d"], r["obj"], r["idx"], k)
        assert_same(ask(L, scene, rays, k), want, (what, "K", k))
        if brute_too:
            assert_same(brute(L, scene, rays, k), want, (what, "brute K", k))
    assert np.array_equal(count(L, scene, rays), total), (what, "count")
    if brute_too:
        assert np.array_equal(brute_count(L, scene, rays), total), (what, "brute count")
    return rows, total


# ---- 1. the rule, bit for bit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cornell_equals_the_rule(H, L, orc_lib, device_scene, mode):
    c = ref.cornell_reference(H, L)
    total = ref.totals(ref.ordered(c["rows"], c["o"], c["d"], INF, c["ranks"]))
    ref.cornell_conditions(total)
    against_the_rule(L, device_scene("cornell", mode), c, KS, what=("cornell", mode))


@pytest.mark.parametrize("name", ["seed-0", "big"])
def test_exact_ties_rank_alone_decides(H, L, orc_lib, device_scene, name):
    t = ref.tie_reference(H, L, name)
    ref.tie_conditions(name, ref.ordered(t["rows"], t["o"], t["d"], INF, t["ranks"]))
    rows, total = against_the_rule(L, device_scene(name), t, (1, 2, 4, 8), what=name)
    # which of the equal depths stay at K = 4 and K = 8 is the K lowest ranks among the ray's triangles: said once more, on the records themselves
    rays = pack(t["o"], t["d"])
    prim_rank = {(int(o), int(i)): int(rk) for o, i, rk in zip(t["obj"], t["idx"], t["ranks"])}
    for k in (4, 8):
        hits, counts = ask(L, device_scene(name), rays, k)
        over = np.flatnonzero(total > k)
        assert len(over) > 50 or (name == "seed-0" and k == 8 and total.max() <= 8)          # (seed-0 has at most 6 triangles on a ray: K = 8 never fills there)
        for i in over[:200]:
            got = [prim_rank[(int(h["object"]), int(h["triangle"]))] for h in hits[i]]
            assert got == sorted(int(rk) for rk in t["ranks"][rows[i][0]])[:k] and counts[i] == k and (hits["t"][i] == np.float32(4.0)).all(), (name, k, i)


@pytest.mark.parametrize("name", ["hall", "hall_x100"])
def test_hall_equals_the_rule(H, L, orc_lib, device_scene, name):
    scale = 100.0 if name == "hall_x100" else 1.0
    scene = device_scene(name)
    for which, n in ((("inner", 128), ("outer", 128)) if name == "hall" else (("outer", 64),)):
        h = ref.hall_reference(H, L, which, n, scale)
        assert np.abs(h["o"]).max() <= camera_limit(name), (np.abs(h["o"]).max(), camera_limit(name))
        assert ref.agrees_with_the_full_matrix(H, h, 2) > 0
        ref.hall_conditions(ref.totals(ref.ordered(h["rows"], h["o"], h["d"], INF, h["ranks"])))
        against_the_rule(L, scene, h, (8,), what=(name, which), brute_too=False)


@pytest.mark.parametrize("name", ["hall", "hall_x100"])
def test_hall_fast_tree_equals_the_brute_force(H, L, device_scene, name):
    scale = 100.0 if name == "hall_x100" else 1.0
    scene = device_scene(name)
    sets = [ref.hall_rays(which, 2048, scale) for which in (("inner", "outer") if name == "hall" else ("outer",))]
    for o, d in sets:
        assert np.abs(o).max() <= camera_limit(name)
        rays = pack(o, d)
        total = brute_count(L, scene, rays)
        ref.hall_conditions(total)                                      # (the brute force's own counts: the first 128 rays of each set are held to the reference above)
        assert np.array_equal(count(L, scene, rays), total), name
        for k in (1, 4, 8):
            want = brute(L, scene, rays, k)
            assert np.array_equal(want[1], np.minimum(total, k))
            assert_same(ask(L, scene, rays, k), want, (name, "K", k))
    # under a limit that cuts about half of the hits off
    o, d = sets[-1]
    t8 = brute(L, scene, pack(o, d), 8)[0]["t"]
    rays = pack(o, d, np.float32(np.median(t8[t8 < FLT_MAX])))
    assert_same(ask(L, scene, rays, 8), brute(L, scene, rays, 8), (name, "limit"))
    assert np.array_equal(count(L, scene, rays), brute_count(L, scene, rays))


# ---- 2. the property: K = 1 is the closest hit, a count above 0 is occlusion -----------------------------------------------------------------------------
def property_rays(H, L, name):
    if name == "cornell":
        c = ref.cornell_reference(H, L)
        return c["o"], c["d"]
    o, d = zip(ref.hall_rays("inner", 2048), ref.hall_rays("outer", 2048))
    return np.concatenate(o), np.concatenate(d)


@pytest.mark.parametrize("name,mode", [("cornell", 0), ("cornell", 1), ("cornell", 2), ("hall", 2)])
def test_one_hit_is_the_closest_hit_and_a_count_is_occlusion(H, L, orc_lib, device_scene, name, mode):
    scene = device_scene(name, mode)
    o, d = property_rays(H, L, name)
    assert ref.active(o, d).all() and np.abs(o).max() <= camera_limit(name, mode)
    for tmax in (INF, np.float32(2.5)):
        t = to_device(pack(o, d, tmax))
        hits, counts = runtime.intersect_all(L, scene, t, 1)
        closest = runtime.intersect(L, scene, t)
        assert hits.cpu().numpy().tobytes() == closest.cpu().numpy().tobytes(), (name, mode, tmax)
        occ = runtime.occluded(L, scene, t).cpu().numpy()
        total = runtime.count_hits(L, scene, t).cpu().numpy()
        assert occ.mean() > 0.05 and (tmax == INF or not occ.all())          # (the hall is closed: without a limit every ray hits)
        assert np.array_equal(total > 0, occ == 1) and np.array_equal(counts.cpu().numpy(), occ)


@pytest.mark.parametrize("name,mode", [("cornell", 2), ("cornell", 1), ("hall", 2)])
def test_inactive_rays_count_nothing(L, device_scene, name, mode):
    scene = device_scene(name, mode)
    o = np.tile(np.array([[0.1, 1.0, -0.3]], np.float32), (16, 1)); d = np.tile(np.array([[0.3, -0.2, 0.9]], np.float32), (16, 1))
    d[0:4] = 0.0; d[1, 2] = -0.0                                        # the zero direction, signed zeros included
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        o[4 + i, i] = v; d[7 + i, i] = v; d[10 + i] = 0.0; o[10 + i, i] = v
    o[13] = np.nan; d[14] = np.inf; d[15] = (np.nan, 0.0, 0.0)
    assert not ref.active(o, d).any()
    for tmax in (INF, np.float32(np.nan), np.float32(1.0)):
        rays = pack(o, d, tmax)
        for k in (1, 8):
            assert_same(ask(L, scene, rays, k), (ref.miss_records((16, k)), np.zeros(16, np.uint32)), ("inactive", k))
            assert_same(brute(L, scene, rays, k), (ref.miss_records((16, k)), np.zeros(16, np.uint32)), ("inactive, brute", k))
        assert not count(L, scene, rays).any() and not brute_count(L, scene, rays).any()
    # an active ray beside them is answered: inactive lanes do not disturb their wave
    o[5] = (0.1, 1.0, -0.3); d[5] = (0.0, 0.0, 1.0)
    assert (count(L, scene, pack(o, d)) > 0).tolist() == [i == 5 for i in range(16)]


# ---- 3. limits ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("cornell", 1), ("cornell", 2), ("big", 2), ("seed-0", 2)])
def test_the_limit(H, L, orc_lib, device_scene, name, mode):
    r = ref.cornell_reference(H, L) if name == "cornell" else ref.tie_reference(H, L, name)
    scene = device_scene(name, mode)
    rows = ref.ordered(r["rows"], r["o"], r["d"], INF, r["ranks"])
    deep = np.flatnonzero(ref.totals(rows) >= 3)
    assert len(deep) >= 200
    sub = dict(r, o=r["o"][deep], d=r["d"][deep], rows=[r["rows"][i] for i in deep])
    second = np.array([rows[i][1][1] for i in deep], np.float32)        # exactly the second hit's depth
    at, total_at = against_the_rule(L, scene, sub, (8,), tmax=second, what=(name, "the second depth"))
    for j, i in enumerate(deep):                                        # exactly the hits with depth <= it remain: a tie at that depth stays whole
        assert total_at[j] == (rows[i][1] <= second[j]).sum() >= 2 and (at[j][1] <= second[j]).all()
    below = np.nextafter(second + np.float32(0), np.float32(-1))          # (below a depth of 0: the negative denormal, under which nothing counts)
    under, total_under = against_the_rule(L, scene, sub, (8,), tmax=below, what=(name, "the float below"))
    for j, i in enumerate(deep):                                        # that depth's hits are all gone
        assert total_under[j] == (rows[i][1] < second[j]).sum() and (under[j][1] < second[j]).all()
    if name != "cornell":
        assert (total_at >= 3).any() and (total_under == 0).all()         # the tie scenes: everything is at one depth
    rays = pack(sub["o"], sub["d"])
    base = ask(L, scene, rays, 8); base_count = count(L, scene, rays)
    for tm in (FLT_MAX, INF, np.float32(np.nan)):                        # all three: no limit
        rays = pack(sub["o"], sub["d"], tm)
        assert_same(ask(L, scene, rays, 8), base, tm); assert np.array_equal(count(L, scene, rays), base_count)
    for tm in (np.float32(-1.0), -INF, -np.float32(1e-30)):              # a negative limit: nothing
        rays = pack(sub["o"], sub["d"], tm)
        assert_same(ask(L, scene, rays, 8), (ref.miss_records((len(deep), 8)), np.zeros(len(deep), np.uint32)), tm); assert not count(L, scene, rays).any()


# ---- 4. deep stacks and the HBM spill ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,pad,fast_lds", [("hall", 2, 0, 2), ("cornell", 1, 60, 2)])
def test_deep_stacks_and_the_spill(H, L, orc_lib, device_scene, name, mode, pad, fast_lds):
    import torch
    scene = device_scene(name, mode)
    if name == "cornell":
        c = ref.cornell_reference(H, L); o, d = c["o"], c["d"]
    else:
        o, d = ref.hall_rays("outer", 2048)
    ra, rb = pack(o, d), pack(o[::-1], d[::-1])
    want = {k: ask(L, scene, ra, k) for k in (1, 8)}; want_count = count(L, scene, ra)
    assert (want_count > 8).any() or name == "cornell"
    runtime.check(L.debug_pad_stack(scene, pad)); runtime.check(L.debug_fast_stack_lds(scene, fast_lds))
    try:
        for k in (1, 8):
            assert_same(ask(L, scene, ra, k), want[k], (name, "short column", k))
        assert np.array_equal(count(L, scene, ra), want_count)
        # two calls back to back on a stream of their own, nothing in between: the spill of the first must outlive its kernel and no longer
        ta, tb = to_device(ra), to_device(rb)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ha = runtime.intersect_all(L, scene, ta, 8); hb = runtime.intersect_all(L, scene, tb, 8); ca = runtime.count_hits(L, scene, ta); cb = runtime.count_hits(L, scene, tb)
        side.synchronize()
        view = lambda x: (x[0].cpu().numpy().view(api.HIT_DTYPE).reshape(len(o), 8), x[1].cpu().numpy().view(np.uint32))
        assert_same(view(ha), want[8], "first"); assert_same(view(hb), (want[8][0][::-1], want[8][1][::-1]), "second")
        assert np.array_equal(ca.cpu().numpy().view(np.uint32), want_count) and np.array_equal(cb.cpu().numpy().view(np.uint32), want_count[::-1])
    finally:
        L.debug_pad_stack(scene, 0); L.debug_fast_stack_lds(scene, 0)
    assert_same(ask(L, scene, ra, 8), want[8], "the plan restored")


# ---- 5. edges of the call ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_edges_of_the_call(H, L, orc_lib, device_scene, mode):
    import torch
    c = ref.cornell_reference(H, L)
    scene = device_scene("cornell", mode)
    tmax = np.where(np.arange(300) % 3 == 0, np.float32(2.0), INF).astype(np.float32)          # a limit on every third ray
    rays = pack(c["o"][:300], c["d"][:300], tmax)
    t = to_device(rays)
    canary = lambda n: torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    for k in (1, 3, 8):
        base, base_counts = ask(L, scene, rays, k)
        assert_same(ask(L, scene, rays, k), (base, base_counts), "again")                       # a second call: the same bytes
        for n in (0, 1, 257):
            hits, counts, totals = canary(8 * (n * k + 1)), canary(n + 1), canary(n + 1)
            L.clear_error()
            assert L.intersect_all_device(scene, t.data_ptr(), n, k, hits.data_ptr(), counts.data_ptr(), None) == 0 and L.count_hits_device(scene, t.data_ptr(), n, totals.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert runtime.last_error() == ""
            hits, counts, totals = hits.cpu().numpy(), counts.cpu().numpy(), totals.cpu().numpy()
            assert (hits[8 * n * k:] == CANARY).all() and (counts[n:] == CANARY).all() and (totals[n:] == CANARY).all(), (k, n)          # nothing past the last record
            assert hits[:8 * n * k].tobytes() == base[:n].tobytes() and np.array_equal(counts[:n].view(np.uint32), base_counts[:n]), (k, n)
            assert np.array_equal(np.minimum(totals[:n].view(np.uint32), k), base_counts[:n])
            again = canary(8 * (n * k + 1))                                                     # counts NULL: the records alone
            assert L.intersect_all_device(scene, t.data_ptr(), n, k, again.data_ptr(), None, None) == 0
            torch.cuda.synchronize()
            assert again.cpu().numpy().tobytes() == hits.tobytes(), (k, n)
        host, host_counts = np.zeros((300, k), api.HIT_DTYPE), np.zeros(300, np.uint32)          # host, device and tensor forms: the same bytes
        assert L.intersect_all(scene, rays.ctypes.data, 300, k, host.ctypes.data, host_counts.ctypes.data) == 0, runtime.last_error()
        assert_same((host, host_counts), (base, base_counts), "host form")
        host2 = np.zeros((300, k), api.HIT_DTYPE)
        assert L.intersect_all(scene, rays.ctypes.data, 300, k, host2.ctypes.data, None) == 0 and host2.tobytes() == base.tobytes()
    host_total = np.zeros(300, np.uint32)
    assert L.count_hits(scene, rays.ctypes.data, 300, host_total.ctypes.data) == 0 and np.array_equal(host_total, count(L, scene, rays))
    assert L.intersect_all_device(scene, None, 0, 4, None, None, None) == 0 and L.count_hits(scene, None, 0, None) == 0
    # refused with a device in reach too: nothing is launched, nothing is written
    hits, counts = canary(8 * 4 * 8), canary(4)
    for what, f in (("K = 0", lambda: L.intersect_all_device(scene, t.data_ptr(), 4, 0, hits.data_ptr(), counts.data_ptr(), None)),
                    ("K = 9", lambda: L.intersect_all_device(scene, t.data_ptr(), 4, 9, hits.data_ptr(), counts.data_ptr(), None)),
                    ("null hits", lambda: L.intersect_all_device(scene, t.data_ptr(), 4, 2, None, counts.data_ptr(), None)),
                    ("null counts", lambda: L.count_hits_device(scene, t.data_ptr(), 4, None, None)),
                    ("n = 2^31", lambda: L.count_hits_device(scene, t.data_ptr(), 1 << 31, counts.data_ptr(), None))):
        L.clear_error()
        assert f() == -4 and runtime.last_error() != "", what
    L.clear_error()
    torch.cuda.synchronize()
    assert (hits.cpu().numpy() == CANARY).all() and (counts.cpu().numpy() == CANARY).all()


def test_a_host_batch_with_an_origin_beyond_the_camera_limit(L, device_scene):
    scene = device_scene("hall")
    o, d = ref.hall_rays("outer", 256)
    o[7] *= np.float32(1000.0)                                           # one active origin far outside: the host form gives the tree up for the batch
    o[9] = np.inf                                                        # (an inactive ray does not: it counts nothing anywhere)
    assert np.abs(o[7]).max() > camera_limit("hall")
    rays = pack(o, d)
    host, host_counts, host_total = np.zeros((256, 8), api.HIT_DTYPE), np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    assert L.intersect_all(scene, rays.ctypes.data, 256, 8, host.ctypes.data, host_counts.ctypes.data) == 0 and L.count_hits(scene, rays.ctypes.data, 256, host_total.ctypes.data) == 0
    assert_same((host, host_counts), brute(L, scene, rays, 8), "beyond the limit")
    assert np.array_equal(host_total, brute_count(L, scene, rays)) and host_total[9] == 0 and host_total.max() > 4


def test_stats_and_a_framebuffer_are_untouched(H, L, orc_lib, device_scene):
    import torch
    c = ref.cornell_reference(H, L)
    scene = device_scene("cornell", 2)
    dsc = ref.cornell_desc(); cam = scenes.camera_of(dsc)
    fb = runtime.DeviceFramebuffer(dsc.width, dsc.height)
    runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    before = (fb.pixels_host().copy(), fb.results_host().copy())
    stats = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(stats))); stats = stats.as_dict()
    rays = pack(c["o"][:512], c["d"][:512])
    ask(L, scene, rays, 8); count(L, scene, rays); brute(L, scene, rays, 2); brute_count(L, scene, rays)
    after = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(after)))
    assert after.as_dict() == stats                                                          # the queries record nothing
    assert H.same_bits(fb.pixels_host(), before[0]) and fb.results_host().tobytes() == before[1].tobytes()
    fb.clear(); runtime.render_device(L, cam, scene, fb); torch.cuda.synchronize()
    assert H.same_bits(fb.pixels_host(), before[0]) and fb.results_host().tobytes() == before[1].tobytes()


# ---- 6. inside / outside by crossings --------------------------------------------------------------------------------------------------------------------------------
SPHERES = (((0.45, 0.45, -0.35), 0.4), ((-0.45, 0.5, 0.35), 0.5))          # scenes.cornell_spheres: the glass and the metal sphere


def sphere_points():
    """256 points uniform in each sphere's bounding cube; judged: |p - c| < 0.9 r inside, |p - c| > 1.1 r and inside no other sphere outside, the rest not judged"""
    r = np.random.default_rng(91)
    pts = np.concatenate([(np.array(c) + rad * r.uniform(-1, 1, size=(256, 3))).astype(np.float32) for c, rad in SPHERES])
    dist = np.stack([np.linalg.norm(pts.astype(np.float64) - np.array(c), axis=1) / rad for c, rad in SPHERES])
    inner = (dist < 0.9).any(axis=0)
    outer = (dist > 1.1).all(axis=0)
    assert (inner | outer).sum() >= 256 and inner.sum() >= 0.2 * (inner | outer).sum() and outer.sum() >= 0.2 * (inner | outer).sum()
    return pts, inner, outer


def test_inside_on_closed_surfaces(L, device_scene):
    """the two spheres of scenes.cornell_spheres by themselves, closed surfaces both: inside is 1 exactly in the spheres"""
    import torch
    scene = device_scene("spheres_only")
    pts, inner, outer = sphere_points()
    got = runtime.inside(L, scene, torch.from_numpy(pts).cuda()).cpu().numpy()
    assert got.dtype == np.int32 and (got[inner] == 1).all() and (got[outer] == 0).all()


def test_inside_and_the_crossing_signed_field(H, L, orc_lib, device_scene):
    """scenes.cornell_spheres itself. Its room is five sheets, open towards -z, and the three directions of inside() all run towards +z: a ray from a point in the
    room leaves through exactly one sheet, so the room adds one crossing to every ray and the parity reads the other way round -- 0 in the spheres, 1 in the room.
    The expectation is therefore made of both parts: the sheets' crossings counted by the oracle's watertight test (the 12 triangles of the first four objects)
    plus one for a point in a sphere; inside() must be the majority of the three parities."""
    import torch
    scene = device_scene("spheres")
    pts, inner, outer = sphere_points()
    judged = inner | outer
    assert (np.abs(pts[:, [0, 2]]) < 1).all() and (pts[:, 1] > 0).all() and (pts[:, 1] < 2).all()          # every point is in the room
    room = ref.soup(scenes.cornell_spheres(16, 16, 1))[0][:12]
    odd = np.zeros((3, len(pts)), np.int64)
    for v, direction in enumerate(runtime.INSIDE_DIRECTIONS):
        d = np.tile(np.asarray(direction, np.float32), (len(pts), 1))
        odd[v] = (np.array([len(ti) for ti, _ in ref.accepted(orc_lib, pts, d, room)]) + inner) & 1
    assert (odd[:, ~inner] == 1).mean() > 0.95                           # the room's one sheet, almost everywhere (a ray through an edge of the sheets may count two)
    want = (odd.sum(axis=0) >= 2).astype(np.int32)
    got = runtime.inside(L, scene, torch.from_numpy(pts).cuda()).cpu().numpy()
    assert np.array_equal(got[judged], want[judged]) and (got[inner] == 0).all() and (got[outer] == 1).all()
    # distance_field(signed="crossings") is -distance exactly where inside() is 1; signed=True and signed=False are what they were
    tris = ref.soup(scenes.cornell_spheres(16, 16, 1))[0].reshape(-1, 3)
    lo, hi = tris.min(axis=0), tris.max(axis=0)
    dims = (9, 8, 7)
    spacing = ((hi - lo) / np.asarray(dims, np.float32)).astype(np.float32)
    q = runtime.distance_field_points(lo, spacing, dims)
    plain = runtime.distance_field(L, scene, lo, spacing, dims)
    crossing = runtime.distance_field(L, scene, lo, spacing, dims, signed="crossings")
    cells = runtime.inside(L, scene, torch.from_numpy(np.ascontiguousarray(q["position"].reshape(-1, 3))).cuda()).cpu().numpy().reshape(q.shape)
    plain, crossing = plain.cpu().numpy(), crossing.cpu().numpy()
    assert tuple(crossing.shape) == (7, 8, 9) and (cells == 1).any() and (cells == 0).any() and (plain > 0).all()
    assert crossing.tobytes() == np.where(cells == 1, -plain, plain).astype(np.float32).tobytes()
    with pytest.raises(runtime.TerraAmdError):
        runtime.distance_field(L, scene, lo, spacing, dims, signed="winding")
