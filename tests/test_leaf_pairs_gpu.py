"""terra_amd_set_leaf_pairs on the device: a ranked launch without work counters of a scene that has the pair form tests a quad's two triangles in one trip of its
leaf loop (csrc/traverse_ref.h "Pair form", csrc/trace_geometry.h watertight_pair). No bit may move:

* every case renders with the switch off, then on, into fresh frames and asks for the same `pixels` and `results` bit for bit, and terra_amd_leaf_pair_info must
  say that the second render used the pair form where the launch qualifies and did not where it does not (the pattern of tests/test_leaf_boxes_gpu.py);
* the pair form is independent of the flat leaf-box test: with that test off, in tree mode `reference` (no cull: every pair is tested) and out of range (the
  walk with regular slabs) the launch walks the tree and its staged nodes carry entry bits;
* the tie scene -- a quad duplicated exactly, so that coincident triangles lie in different entries whose ranks interleave, in objects of different colour, one
  of them emissive -- is held against the oracle under Simple and Direct: it pins the images and the shadow rays' preset record. (The closest hits' (depth, rank)
  record is held apart from "first trip wins" by tests/test_exact_ties_gpu.py, on different triangles at equal depths; coincident copies cannot do that.)
* k_watertight_pair equals k_watertight run on each triangle, bit for bit, on about 10^5 rays: random ones, rays aimed exactly at points of the diagonal, at each
  of the four vertices and at the outer edges, axis-parallel ones, a degenerate pair (p3 on the line p0-p2: T2's double-precision fallback) and a folded pair.
"""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_leaf_boxes_gpu import same_fb, _cornell_x100
from test_flat_loop_layout_gpu import oracle, equals_oracle, QUAD_COLOURS
from test_leaf_pairs import NO_PAIR_FORM

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def dev(L, d, pairs, flat=1, split=1, passes=1, shard=None, rect=None, counters=False, tree_mode=None):
    import torch
    scene = scenes.build_scene(L, d, tree_mode=tree_mode, counters=counters)
    assert runtime.last_error() == "", runtime.last_error()
    assert L.get_leaf_pairs(scene) == 1                      # the default
    assert L.set_leaf_pairs(scene, int(pairs)) == 0 and L.get_leaf_pairs(scene) == int(pairs)
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
    out = dict(pixels=fb.pixels_host().copy(), acc=res["acc"].copy(), samples=res["samples"].copy(), used=used, n_pairs=n_pairs, flat=flat_used)
    L.scene_destroy(scene)
    return out


def off_then_on(G, mk, expect, **kw):
    off = dev(G, mk(), 0, **kw)
    on = dev(G, mk(), 1, **kw)
    assert same_fb(off, on), kw
    assert not off["used"]
    assert on["used"] == expect, (on["used"], on["n_pairs"], kw)
    return off, on


CORNELL = dict(width=64, height=48, spp=8)


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis], ids=["simple", "direct", "direct-mis"])
def test_cornell_integrators(G, integ):
    off, on = off_then_on(G, lambda: scenes.cornell_box(integrator=integ, **CORNELL), True)
    assert on["n_pairs"] == 16 and on["flat"] and (on["samples"] == 8).all() and on["acc"].sum() > 0


@gpu
def test_cornell_phong(G):
    off, on = off_then_on(G, lambda: scenes.cornell_phong(64, 48, 4), True)
    assert on["n_pairs"] == 16


@gpu
@pytest.mark.parametrize("kw", [dict(shard=(16, 0, 2)), dict(shard=(16, 1, 2)), dict(rect=(7, 5, 24, 20))], ids=["shard-0-of-2", "shard-1-of-2", "rectangle-at-an-odd-origin"])
def test_cornell_launch_shapes(G, kw):
    off, on = off_then_on(G, lambda: scenes.cornell_box(**CORNELL), True, **kw)
    assert on["acc"].sum() > 0


@gpu
def test_split_four_equals_four_successive_calls(G):
    one = dev(G, scenes.cornell_box(64, 48, 8), 1, split=4)
    many = dev(G, scenes.cornell_box(64, 48, 2), 1, passes=4)
    single = dev(G, scenes.cornell_box(64, 48, 8), 0, split=4)
    assert one["used"] and many["used"] and not single["used"]
    assert same_fb(one, many) and same_fb(one, single) and (one["samples"] == 8).all()


@gpu
@pytest.mark.parametrize("case", ["flat-test-off", "tree-mode-reference", "out-of-range"])
def test_pair_launches_that_walk_the_tree(G, case):
    kw, mk = {}, (lambda: scenes.cornell_box(**CORNELL))
    if case == "flat-test-off":
        kw["flat"] = 0
    if case == "tree-mode-reference":
        kw["tree_mode"] = 0
    if case == "out-of-range":
        mk = _cornell_x100
    off, on = off_then_on(G, mk, True, **kw)
    assert not on["flat"] and on["n_pairs"] == 16 and on["acc"].sum() > 0


@gpu
def test_counting_launch_keeps_the_single_form(G):
    off, on = off_then_on(G, lambda: scenes.cornell_box(**CORNELL), False, counters=True)
    assert on["n_pairs"] == 16 and not on["flat"]


@gpu
@pytest.mark.parametrize("name", list(NO_PAIR_FORM))
def test_scenes_without_a_pair_form_keep_the_single_form(G, H, name):
    def mk():
        d = NO_PAIR_FORM[name](H)
        d.width, d.height, d.spp = 32, 32, 4
        return d
    off, on = off_then_on(G, mk, False)
    assert on["n_pairs"] == 0


# ---- the tie scene ------------------------------------------------------------------------------------------------------------------

TIE_ORDERS = {"far-quads-first": [4, 5, 0, 1, 2, 3], "reversed": [5, 4, 3, 2, 1, 0]}


def tie_scene(integ, order):
    """a quad facing the camera twice over, as four single-triangle objects A B A B of four colours -- the first one emissive --, and two larger emissive quads behind
    it. The coincident triangles share one leaf box and, with the objects in these orders, lie in different entries whose ranks interleave."""
    def quad(h, z):
        return scenes._merge([scenes._quad((-h, 1 - h, z), (h, 1 - h, z), (h, 1 + h, z), (-h, 1 + h, z), (0, 0, -1))])
    near = quad(0.6, 0.0)
    objs = []
    for k in range(4):
        tris, nrm, uv = (a[k % 2:k % 2 + 1].copy() for a in near)
        objs.append(scenes.ObjectDesc(tris, nrm, uv, scenes.Material(albedo=(0.2 + 0.2 * k, 0.5, 0.9 - 0.2 * k), emissive=QUAD_COLOURS[0] if k == 0 else (0.0, 0.0, 0.0)), "near%d" % k))
    for k, z in enumerate((0.5, 1.0)):
        objs.append(scenes.ObjectDesc(*quad(0.7 + 0.1 * k, z), scenes.Material(albedo=(0.5, 0.5, 0.5), emissive=QUAD_COLOURS[1 + k]), "far%d" % k))
    return scenes.SceneDesc(objects=[objs[i] for i in order], width=32, height=32, spp=4, bounces=2, integrator=integ, name="tie")


@gpu
@pytest.mark.parametrize("order", list(TIE_ORDERS))
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect], ids=["simple", "direct"])
def test_tie_scene_equals_the_oracle(G, H, orc_lib, integ, order):
    mk = lambda: tie_scene(integ, TIE_ORDERS[order])
    scene = scenes.build_scene(G, mk(), counters=False)
    pairs, masks = runtime.scene_leaf_pairs(G, scene)
    G.scene_destroy(scene)
    assert len(pairs) == 4
    (both,) = [int(m) for m in masks if bin(int(m)).count("1") == 2]          # the box of the quad and its duplicate: two entries ...
    x, y = [pairs["rank"][e] for e in range(4) if both >> e & 1]
    assert x.min() < y.min() < x.max()                                       # ... whose ranks interleave: the later trip holds a rank below one of the earlier trip
    off, on = off_then_on(G, mk, True)
    assert np.any(on["acc"] != 0)                                            # (Direct's sums may be negative here: the quads' normals face the camera, as the reference has it)
    assert equals_oracle(on, oracle(H, mk()))


# ---- the pair test against the single test ------------------------------------------------------------------------------------------

def _unit(G, name, n, o, d, geom, width):
    f = G.fn(name, C.c_int, [C.c_int] + [C.c_void_p] * 5)
    hit = np.zeros((n, width[0]), np.int32); out = np.zeros((n, width[1]), np.float32)
    o, d, geom = (np.ascontiguousarray(a, np.float32) for a in (o, d, geom))
    assert f(n, o.ctypes.data, d.ctypes.data, geom.ctypes.data, hit.ctypes.data, out.ctypes.data) == 0, runtime.last_error()
    return hit, out


def _pair_cases(seed=7):
    r = np.random.default_rng(seed)
    O, D, Q = [], [], []

    def add(o, d, q):
        O.append(np.asarray(o, np.float32)); D.append(np.asarray(d, np.float32)); Q.append(np.asarray(q, np.float32).reshape(n_of(q), 12))

    def n_of(q):
        return np.asarray(q).reshape(-1, 12).shape[0]

    def random_quads(n, planar=True):
        c = r.uniform(-2, 2, (n, 1, 3)); u = r.normal(size=(n, 1, 3)); v = r.normal(size=(n, 1, 3))
        st = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)[None] + r.uniform(-0.2, 0.2, (n, 4, 2))
        q = c + st[..., :1] * u + st[..., 1:] * v
        if not planar:
            q = q + r.normal(scale=0.3, size=(n, 4, 3))
        return q.astype(np.float32)

    def aimed(q, w):
        """rays from random origins through the points sum_k w[k] p_k, the direction computed in float32 from float32 operands"""
        n = len(q)
        tgt = (w[..., None] * q.astype(np.float64)).sum(1).astype(np.float32)
        o = (tgt + r.normal(size=(n, 3)) * 3).astype(np.float32)
        return o, (tgt - o).astype(np.float32)

    n = 30000
    q = random_quads(n)                                                      # random rays at random planar quads: most hit one triangle or none
    w = r.dirichlet(np.ones(4), n); add(*aimed(q, w), q)
    q = random_quads(n, planar=False); w = r.dirichlet(np.ones(4), n); add(*aimed(q, w), q)      # ... and at folded quads
    n = 12000
    q = random_quads(n); t = r.uniform(0, 1, n); w = np.zeros((n, 4)); w[:, 0] = 1 - t; w[:, 2] = t          # points of the diagonal p0-p2
    add(*aimed(q, w), q)
    for k in range(4):                                                       # each of the four vertices
        q = random_quads(3000); w = np.zeros((3000, 4)); w[:, k] = 1; add(*aimed(q, w), q)
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 0)):                            # the outer edges
        q = random_quads(3000); t = r.uniform(0, 1, 3000); w = np.zeros((3000, 4)); w[:, a] = 1 - t; w[:, b] = t; add(*aimed(q, w), q)
    # axis-parallel rays at axis-aligned quads on a dyadic grid: edge functions that are exactly 0, on the diagonal and on the rim
    n = 6000
    ax = r.integers(3, size=n); g = lambda *s: r.integers(-8, 9, s) / 4.0
    q = np.zeros((n, 4, 3)); lo, hi = g(n, 2), None
    hi = lo + r.integers(1, 9, (n, 2)) / 4.0; z = g(n)
    o = np.zeros((n, 3)); d = np.zeros((n, 3))
    for i in range(n):
        u_ax, v_ax = [(1, 2), (2, 0), (0, 1)][ax[i]]
        for k, (cu, cv) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
            q[i, k, u_ax] = (lo[i, 0], hi[i, 0])[cu]; q[i, k, v_ax] = (lo[i, 1], hi[i, 1])[cv]; q[i, k, ax[i]] = z[i]
        s = r.integers(0, 5, 2) / 4.0                                        # a grid point of the quad: corners, rim, diagonal, inside
        o[i, u_ax] = lo[i, 0] + s[0] * (hi[i, 0] - lo[i, 0]); o[i, v_ax] = lo[i, 1] + s[1] * (hi[i, 1] - lo[i, 1]); o[i, ax[i]] = z[i] - r.integers(1, 9) / 2.0
        d[i, ax[i]] = 1.0 if i % 2 else 2.5
    add(o, d, q)
    # a degenerate pair: p3 on the line p0-p2 exactly (dyadic coordinates): T2 has no area, its edge functions vanish -> its double-precision fallback
    n = 6000
    q = (r.integers(-16, 17, (n, 4, 3)) / 8.0)
    q[:, 3] = q[:, 0] + (q[:, 2] - q[:, 0]) * (r.integers(0, 5, (n, 1)) / 4.0)
    w = r.dirichlet(np.ones(4), n); w[::3, 1] = 0; w[::3] /= w[::3].sum(1, keepdims=True)
    add(*aimed(q.astype(np.float32), w), q)
    # a folded pair: p3 on p1's side of the diagonal, so that T2 lies over T1 and a ray can pass both
    n = 12000
    q = random_quads(n).astype(np.float64)
    q[:, 3] = q[:, 0] + 0.6 * (q[:, 1] - q[:, 0]) + 0.3 * (q[:, 2] - q[:, 0]) + r.normal(scale=0.05, size=(n, 3))
    w = r.dirichlet(np.ones(4), n); add(*aimed(q.astype(np.float32), w), q)
    return np.concatenate(O), np.concatenate(D), np.concatenate(Q)


@gpu
def test_watertight_pair_equals_watertight_on_each_triangle(G):
    o, d, q = _pair_cases()
    n = len(o)
    assert 90000 <= n <= 130000
    q = q.reshape(n, 4, 3)
    hp, dp = _unit(G, "terra_amd_unit_watertight_pair", n, o, d, q, (2, 2))
    t1 = q[:, [0, 1, 2]].reshape(n, 9); t2 = q[:, [0, 2, 3]].reshape(n, 9)
    both = 0
    for k, tri in enumerate((t1, t2)):
        hs, os_ = _unit(G, "terra_amd_unit_watertight", n, o, d, tri, (1, 8))
        assert np.array_equal(hp[:, k], hs[:, 0]), (k, int((hp[:, k] != hs[:, 0]).sum()))
        hit = hs[:, 0] == 1
        assert np.array_equal(dp[hit, k].view(np.uint32), os_[hit, 3].view(np.uint32)), k
        assert hit.sum() > n // 20
    both = int(((hp[:, 0] == 1) & (hp[:, 1] == 1)).sum())
    assert both > 1000                                                       # the diagonal and the folded pairs: the second run of the shared part
