"""Every closest-hit door of the device held to (depth, rank) on scenes whose DIFFERENT triangles lie at depths equal bit for bit (tests/exact_ties.py; the
conditions that make these scenes discriminate are asserted on the CPU in tests/test_exact_ties.py). What the duplicated quad of tests/test_leaf_pairs_gpu.py cannot
tell apart -- the pair form's (depth, key) record from "the first trip wins" -- differs here on 89 to 96 rays per scene, and every case below asserts that its image
is not the one "the first trip wins" would give.

* ray-sourced render (terra_amd_render_rays_device), Simple, no bounce, on the three 32-triangle scenes: pairs off then on, bit-equal, terra_amd_leaf_pair_info says
  which form ran; `results.acc` equals the float32 sums of the oracle's orc_trace_one and is the winning triangle's emission; inactive pixels hold spp samples of +0.
  Variants: the flat leaf-box test off, tree mode 0 (the walk, no cull), counters on (the ranked single form), and 4 samples per pixel with split 2;
* ray-sourced AOV on a scene with per-triangle albedo: base colour, normal and depth of the oracle's surface;
* ray queries (terra_amd_intersect_device / _occluded_device) from the pushed origin, tree modes 0, 1 and 2 on the 32-triangle scenes and the fast tree of both
  builders on the 80-triangle scene (up to 13 triangles tie on a ray): object, triangle, t and point are the model's and the oracle's traversal's; a limit of
  exactly 4.0 changes nothing, the float below 4.0 makes every ray miss with the documented record; the unit traversals answer the same.

Mutants (profiles/exact_ties/mutants.md): with the tie half of traverse_pairs' clause removed for closest hits the ten pair cases here fail and
tests/test_leaf_pairs_gpu.py still passes; with the fast tree's tie half removed the five fast-tree query cases fail. With traverse_pairs' tie half removed for
ANYHIT only (the shadow rays' preset record) NOTHING fails: no case here casts a shadow ray, and the duplicated quad of tests/test_leaf_pairs_gpu.py under Direct
passes too. That half of the clause is still without a test that notices its removal.
"""
import ctypes as C

import numpy as np
import pytest

import exact_ties as X
from terra_amd import api, runtime, scenes
from test_ray_query import query, assert_matches_traversal, FLT_MAX, INF

pytestmark = pytest.mark.gpu

N = 2113
W, HGT = X.FRAME_W, X.FRAME_H


@pytest.fixture(scope="module")
def G(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


_tables = {}


def table(key, make):
    """the oracle's tables, computed once per module"""
    if key not in _tables:
        _tables[key] = make()
    return _tables[key]


def device_rays():
    import torch
    return torch.from_numpy(np.ascontiguousarray(X.ray_frame())).cuda()


def render(G, name, pairs, flat=1, tree_mode=None, counters=False, spp=1, split=1):
    import torch
    G.clear_error()
    scene = scenes.build_scene(G, X.scene(name, spp=spp), tree_mode=tree_mode, counters=counters)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        ti = runtime.TraversalInfo(); runtime.check(G.traversal_info(scene, C.byref(ti)))
        assert float(abs(X.Z_ORIGIN)) < ti.camera_limit                       # the device form cannot look at the origins: they lie inside what the commit verified
        runtime.check(G.set_leaf_pairs(scene, int(pairs))); runtime.check(G.set_leaf_box_test(scene, int(flat))); runtime.check(G.set_sample_split(scene, split))
        fb = runtime.DeviceFramebuffer(W, HGT); rays = device_rays()
        runtime.render_rays_device(G, scene, rays, fb)
        torch.cuda.synchronize()
        assert runtime.last_error() == "", runtime.last_error()
        used, n_pairs = runtime.leaf_pair_info(G, scene)
        flat_used, _ = runtime.leaf_box_info(G, scene)
        res = fb.results_host()
        return dict(pixels=fb.pixels_host().copy(), acc=res["acc"].reshape(-1, 3).copy(), samples=res["samples"].reshape(-1).copy(), used=used, n_pairs=n_pairs, flat=flat_used)
    finally:
        G.scene_destroy(scene)


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("acc", "pixels")) and np.array_equal(a["samples"], b["samples"])


def check_render(H, G, name, expect_pairs, expect_flat, spp=1, **kw):
    off = render(G, name, 0, spp=spp, **kw)
    on = render(G, name, 1, spp=spp, **kw)
    assert same(off, on), (name, kw)
    assert not off["used"] and on["used"] == expect_pairs and on["n_pairs"] == 16, (on["used"], on["n_pairs"], kw)
    assert on["flat"] == expect_flat, kw
    m = X.model_of(H, G, name)
    sums = table(("sums", name), lambda: X.oracle_sums(H, X.scene(name), 4))
    for out in (off, on):
        assert (out["samples"] == spp).all()
        assert not out["acc"][N:].view(np.uint32).any()                       # inactive pixels: spp samples of +0
        assert H.same_bits(out["acc"][:N], sums[spp - 1]), (name, kw)
        assert H.same_bits(out["acc"][:N], X.image_of(m["expected"], m["generated"], spp)), (name, kw)          # the winning triangle's emission, spp times
        differs = (out["acc"][:N] != X.image_of(m["first_trip"], m["generated"], spp)).any(axis=1)
        assert differs.sum() >= 64 and np.array_equal(differs, m["discriminating"]), (name, int(differs.sum()))   # not the image of "the first trip wins"
    return on


# ---- ray-sourced render ----------------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"default": (dict(), True, True), "flat-test-off": (dict(flat=0), True, False), "tree-mode-reference": (dict(tree_mode=0), True, False),
            "counters": (dict(counters=True), False, False)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(X.PAIR_SCENES))
def test_ray_render_names_the_lowest_rank(H, G, orc_lib, name, variant):
    kw, pairs, flat = VARIANTS[variant]
    check_render(H, G, name, pairs, flat, **kw)


def test_ray_render_four_samples_split_two(H, G, orc_lib):
    check_render(H, G, "seed-0", True, True, spp=4, split=2)


# ---- ray-sourced AOV ---------------------------------------------------------------------------------------------------------------------------------------
def test_ray_aov_is_the_oracle_surface(H, G, orc_lib):
    import torch
    name = "seed-5"
    d = X.scene(name, albedo=True)
    m = X.model_of(H, G, name)
    obj, tri, point, surf = table(("surface", name), lambda: X.oracle_raycast(H, d))
    hit = m["hit"]
    assert np.array_equal(obj >= 0, hit) and np.array_equal(tri[hit].astype(np.int64), m["prim"][m["expected"]][hit] >> 8)
    G.clear_error()
    s = scenes.build_scene(G, d)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        runtime.check(G.set_sample_split(s, 1))
        aov = runtime.DeviceAov(W, HGT); rays = device_rays()
        runtime.render_aov_rays_device(G, s, rays, aov)
        torch.cuda.synchronize()
        a = aov.host().reshape(-1)
    finally:
        G.scene_destroy(s)
    assert (a["samples"] == 1).all() and not a["reserved"].any()
    live = np.zeros(W * HGT, bool); live[:N] = hit
    assert np.array_equal(a["coverage"], live.astype(np.float32))
    for k in ("albedo", "normal", "depth"):
        assert not a[k][~live].view(np.uint32).any(), k
    su = api.TerraShadingSurface
    n_off, a_off = su.normal.offset // 4, su.attributes.offset // 4
    got = a[:N][hit]
    assert H.same_bits(got["normal"], surf[hit, n_off:n_off + 3])
    assert H.same_bits(got["albedo"], surf[hit, a_off:a_off + 3])                 # diffuse: TERRA_DIFFUSE_ALBEDO is attribute 0
    want_albedo = np.array([X.albedo_of(int(g)) for g in m["generated"]], np.float32)[m["expected"][hit]]
    assert H.same_bits(got["albedo"], want_albedo)                                # ... which is the winning triangle's texel
    other = np.array([X.albedo_of(int(g)) for g in m["generated"]], np.float32)[m["first_trip"][m["discriminating"]]]
    assert (a[:N][m["discriminating"]]["albedo"] != other).any(axis=1).all() and m["discriminating"].sum() >= 64
    o, _ = X.rays(X.Z_ORIGIN)
    want = np.linalg.norm(point[hit].astype(np.float64) - o[hit].astype(np.float64), axis=1)
    # float32 sqrt of a three-term sum of squares of float32 differences: a handful of roundings of 2^-24 each, far inside 1e-6
    np.testing.assert_allclose(got["depth"].astype(np.float64), want, rtol=1e-6, atol=0)


# ---- ray queries -------------------------------------------------------------------------------------------------------------------------------------------
def check_queries(H, G, name, tree_mode, tree_builder=None):
    m = X.model_of(H, G, name)
    d = X.scene(name)
    found, prim, point = table(("traverse", name), lambda: X.oracle_traverse(H, d))
    o, dirs = X.rays(X.Z_PUSHED)
    hit, want = m["hit"], m["prim"][m["expected"]]
    G.clear_error()
    s = scenes.build_scene(G, d, tree_mode=tree_mode, tree_builder=tree_builder)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        ti = runtime.TraversalInfo(); runtime.check(G.traversal_info(s, C.byref(ti)))
        if tree_builder is not None:
            assert ti.fast_tree == 1 and ti.fast_tree_built_on_device == tree_builder, ti.note
        what = (name, tree_mode, tree_builder, ti.note)
        base = query(H, G, s, o, dirs, INF)                                       # (asserts occluded == hit and the form of the records, misses included)
        assert np.array_equal(base["object"] >= 0, hit), what
        assert np.array_equal(base["object"][hit].astype(np.int64), want[hit] & 0xff) and np.array_equal(base["triangle"][hit].astype(np.int64), want[hit] >> 8), what
        assert (base["t"][hit].view(np.uint32) == X.DEPTH.view(np.uint32)).all(), what
        assert_matches_traversal(H, base, found, prim, point, what)
        U = X.device_unit(H, G)
        assert_matches_traversal(H, base, *U.bvh_traverse(s, o, dirs), what)
        if ti.fast_tree:
            assert_matches_traversal(H, base, *U.bvh_traverse_fast(s, o, dirs)[:3], what)
        assert query(H, G, s, o, dirs, X.DEPTH).tobytes() == base.tobytes(), what                      # a depth equal to the limit counts
        below = query(H, G, s, o, dirs, np.nextafter(X.DEPTH, np.float32(0)))
        assert (below["object"] == -1).all() and (below["t"] == FLT_MAX).all(), what                   # (check_records: the documented miss record)
    finally:
        G.scene_destroy(s)


@pytest.mark.parametrize("tree_mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(X.PAIR_SCENES))
def test_queries_on_the_pair_scenes(H, G, orc_lib, name, tree_mode):
    check_queries(H, G, name, tree_mode)


@pytest.mark.parametrize("tree_builder", [0, 1], ids=["host-sah", "device-lbvh"])
def test_queries_on_eighty_triangles(H, G, orc_lib, tree_builder):
    check_queries(H, G, "big", 1, tree_builder)
