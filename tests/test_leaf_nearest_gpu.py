"""terra_amd_set_leaf_nearest_first on the device: a lane of a flat pair-form launch tests the pair of its nearest leaf box first and drops the pairs whose boxes it
enters strictly beyond the record (csrc/traverse_ref.h "Nearest first"). No bit may move:

* every case renders with the switch off, then on, into fresh frames and asks for the same `pixels` and `results` bit for bit (the pattern and the helpers of
  tests/test_leaf_pairs_gpu.py and tests/test_leaf_boxes_gpu.py);
* Cornell under Simple, Direct and Direct + MIS (the shadow rays' preset record: the skip in front of every box), sample split 4 against four successive calls,
  two passes into one frame, a rectangle at an odd origin, both ranks of a 2-rank shard, the Phong variant;
* launches that keep the walk -- the flat test off, tree mode `reference`, the scene scaled by 100 out of the coordinate range --: the switch changes nothing and
  terra_amd_leaf_box_info says the launch still walked;
* the duplicated quad of tests/test_leaf_pairs_gpu.py: two entries share one leaf box and therefore one entry distance. The host leaves nearest first off for such
  a scene (the flat loop numbers a key by its box; csrc/scene_host.cpp leaf_pairs_one_per_box), so the launch runs the leaf loop in entry order; held against the
  oracle;
* the exact-tie scenes of tests/exact_ties.py: different triangles at one depth, the key half of the record decides. (Their rays run along +z: not tame, so their
  waves walk the tree and the leaf loop runs without a cut, in entry order.)
* the diagonal quads of tests/test_leaf_nearest.py: the nearest box's pair is often missed, the record comes from a later trip; Simple and Direct, against the oracle.
"""
import numpy as np
import pytest

import exact_ties as X
from terra_amd import api, runtime, scenes
from test_leaf_boxes_gpu import same_fb, _cornell_x100
from test_flat_loop_layout_gpu import oracle, equals_oracle
from test_leaf_pairs_gpu import tie_scene, TIE_ORDERS
from test_leaf_nearest import diagonal_quads
import test_exact_ties_gpu as T

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def dev(L, d, nearest, flat=1, split=1, passes=1, shard=None, rect=None, tree_mode=None):
    import torch
    scene = scenes.build_scene(L, d, tree_mode=tree_mode, counters=False)
    assert runtime.last_error() == "", runtime.last_error()
    assert L.get_leaf_nearest_first(scene) == 1                  # the default
    assert L.set_leaf_nearest_first(scene, int(nearest)) == 0 and L.get_leaf_nearest_first(scene) == int(nearest)
    assert L.set_leaf_box_test(scene, int(flat)) == 0
    assert L.set_sample_split(scene, split) == 0
    fb = runtime.DeviceFramebuffer(d.width, d.height); cam = scenes.camera_of(d)
    for _ in range(passes):
        if shard:
            runtime.render_device_sharded(L, cam, scene, fb, *shard)
        else:
            runtime.render_device(L, cam, scene, fb, rect)
    torch.cuda.synchronize()
    assert runtime.last_error() == ""
    used, n_pairs = runtime.leaf_pair_info(L, scene)
    flat_used, _ = runtime.leaf_box_info(L, scene)
    res = fb.results_host()
    out = dict(pixels=fb.pixels_host().copy(), acc=res["acc"].copy(), samples=res["samples"].copy(), pairs=used, n_pairs=n_pairs, flat=flat_used)
    L.scene_destroy(scene)
    return out


def off_then_on(G, mk, expect_flat=True, **kw):
    off = dev(G, mk(), 0, **kw)
    on = dev(G, mk(), 1, **kw)
    assert same_fb(off, on), kw
    assert off["pairs"] and on["pairs"]                          # the switch is an option of the pair form: both launches have it
    assert off["flat"] == on["flat"] == expect_flat, kw
    return off, on


CORNELL = dict(width=64, height=48, spp=8)


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis], ids=["simple", "direct", "direct-mis"])
def test_cornell_integrators(G, integ):
    off, on = off_then_on(G, lambda: scenes.cornell_box(integrator=integ, **CORNELL))
    assert on["n_pairs"] == 16 and (on["samples"] == 8).all() and on["acc"].sum() > 0


@gpu
def test_cornell_equals_the_oracle(G, H, orc_lib):
    mk = lambda: scenes.cornell_box(**CORNELL)
    on = dev(G, mk(), 1)
    assert on["pairs"] and on["flat"]
    assert equals_oracle(on, oracle(H, mk()))


@gpu
def test_split_four_equals_four_successive_calls(G):
    one = dev(G, scenes.cornell_box(64, 48, 8), 1, split=4)
    many = dev(G, scenes.cornell_box(64, 48, 2), 1, passes=4)
    off = dev(G, scenes.cornell_box(64, 48, 8), 0, split=4)
    assert same_fb(one, many) and same_fb(one, off) and (one["samples"] == 8).all()


@gpu
@pytest.mark.parametrize("kw", [dict(passes=2), dict(rect=(7, 5, 24, 20)), dict(shard=(16, 0, 2)), dict(shard=(16, 1, 2))],
                         ids=["two-passes-into-one-frame", "rectangle-at-an-odd-origin", "shard-0-of-2", "shard-1-of-2"])
def test_cornell_launch_shapes(G, kw):
    off, on = off_then_on(G, lambda: scenes.cornell_box(**CORNELL), **kw)
    assert on["acc"].sum() > 0


@gpu
def test_cornell_phong(G):
    off, on = off_then_on(G, lambda: scenes.cornell_phong(64, 48, 4))
    assert on["n_pairs"] == 16


@gpu
@pytest.mark.parametrize("case", ["flat-test-off", "tree-mode-reference", "out-of-range"])
def test_launches_that_walk_the_tree(G, case):
    kw, mk = {}, (lambda: scenes.cornell_box(**CORNELL))
    if case == "flat-test-off":
        kw["flat"] = 0
    if case == "tree-mode-reference":
        kw["tree_mode"] = 0
    if case == "out-of-range":
        mk = _cornell_x100
    off, on = off_then_on(G, mk, expect_flat=False, **kw)
    assert on["n_pairs"] == 16 and on["acc"].sum() > 0


@gpu
@pytest.mark.parametrize("order", list(TIE_ORDERS))
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect], ids=["simple", "direct"])
def test_duplicated_quad(G, H, orc_lib, integ, order):
    mk = lambda: tie_scene(integ, TIE_ORDERS[order])
    off, on = off_then_on(G, mk)
    assert on["n_pairs"] == 4 and np.any(on["acc"] != 0)
    assert equals_oracle(on, oracle(H, mk()))


def render_ties(G, name, nearest):
    """tests/test_exact_ties_gpu.py render(), pair form on, with the switch set"""
    import torch
    G.clear_error()
    scene = scenes.build_scene(G, X.scene(name), counters=False)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        runtime.check(G.set_leaf_nearest_first(scene, int(nearest))); runtime.check(G.set_sample_split(scene, 1))
        fb = runtime.DeviceFramebuffer(T.W, T.HGT); rays = T.device_rays()
        runtime.render_rays_device(G, scene, rays, fb)
        torch.cuda.synchronize()
        assert runtime.last_error() == "", runtime.last_error()
        used, _ = runtime.leaf_pair_info(G, scene)
        res = fb.results_host()
        return dict(pixels=fb.pixels_host().copy(), acc=res["acc"].reshape(-1, 3).copy(), samples=res["samples"].reshape(-1).copy(), used=used)
    finally:
        G.scene_destroy(scene)


@gpu
@pytest.mark.parametrize("name", list(X.PAIR_SCENES))
def test_exact_tie_scenes(G, H, orc_lib, name):
    off = render_ties(G, name, 0)
    on = render_ties(G, name, 1)
    assert off["used"] and on["used"] and T.same(off, on)
    m = X.model_of(H, G, name)
    assert H.same_bits(on["acc"][:T.N], X.image_of(m["expected"], m["generated"], 1))          # the lowest rank among equal depths
    assert (on["acc"][:T.N] != X.image_of(m["first_trip"], m["generated"], 1)).any(axis=1).sum() >= 64


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect], ids=["simple", "direct"])
def test_diagonal_quads_equal_the_oracle(G, H, orc_lib, integ):
    mk = lambda: diagonal_quads(integrator=integ)
    off, on = off_then_on(G, mk)
    assert on["n_pairs"] == 10 and (on["samples"] == 8).all() and np.any(on["acc"] != 0)
    want = oracle(H, mk())
    assert equals_oracle(on, want) and equals_oracle(off, want)
