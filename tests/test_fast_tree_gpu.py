"""The device LBVH (terra_amd/csrc/tree_build_device.hip: k_boxes, k_keys, k_hierarchy, k_fit, k_keep, k_emit, k_soup and hipCUB's sort and scan) held to its
restatement bit for bit, and both builders' trees traversed against the reference tree. No tolerance anywhere: the build is deterministic (tests/lbvh_ref.py
says why), so the whole DevNode array is compared byte for byte.

* terra_amd_unit_fast_tree with builder 1 on every soup of tests/fast_tree_soups.py: node count, node bytes, order, pad words and max_stack are the restatement's;
  the tree and its widening at three scales pass tests/fast_tree_checks.py (coverage, plain unions, tightest binary16 planes, the stack bound recomputed
  top-down, max_stack <= 64).
* Two builds of 20,000 triangles give identical bytes (the fit's atomics only order arrivals).
* n = 2 and n = 0 are the builder's invalid-argument error and write nothing.
* Every soup of more than 64 triangles (the commit asks for the device builder above that) committed with tree_mode = 1 by both builders: bvh_traverse_fast
  equals bvh_traverse, and the two builders' scenes equal each other, in found, prim and the point's bits, over 1,024 rays of which at least half hit
  (tests/test_fast_tree.py asserts that share with the oracle first).
"""
import ctypes as C

import numpy as np
import pytest

import fast_tree_checks as K
import fast_tree_soups as S
import lbvh_ref as R
from terra_amd import runtime, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


@pytest.fixture(scope="module")
def U(H, G):
    u = H.Unit.__new__(H.Unit)          # over the library under test itself (runtime.load())
    u.kind, u.L, u.p = "amd", G, "terra_amd_unit_"
    return u


_ref = {}


def ref(name):
    if name not in _ref:
        s = S.soup(name)
        _ref[name] = R.build(s.tris, s.rank, s.extra)
    return _ref[name]


def device(U, name, scale=1.0):
    s = S.soup(name)
    rc, out = U.fast_tree(s.tris, s.rank, 1, s.extra, scale)
    assert rc == 0, runtime.last_error()
    return out


def first_difference(got, want):
    n = min(len(got), len(want))
    for f in R.NODE.names:
        bad = np.nonzero((got[f][:n].view(np.uint32) != want[f][:n].view(np.uint32)).reshape(n, -1).any(axis=1))[0]
        if len(bad):
            return f"{len(bad)} nodes differ in {f}, first at {int(bad[0])}: device {got[f][bad[0]]} restatement {want[f][bad[0]]}"
    return f"{len(got)} nodes against {len(want)}"


@pytest.mark.parametrize("name", S.NAMES)
def test_device_builder_equals_the_restatement(U, name):
    s = S.soup(name)
    want = ref(name)
    scales = S.scales_of(name)
    got = device(U, name, scales[0])
    print(f"{name}: {got['n_nodes']} nodes (restatement {want['n_nodes']}), max_stack {got['max_stack']} ({want['max_stack']}), wide {got['n_wide']} nodes, stack {got['wide_max_stack']}")
    assert got["n_nodes"] == want["n_nodes"] and got["max_stack"] == want["max_stack"]
    assert np.array_equal(got["order"], want["order"])
    assert np.array_equal(got["pad"], want["pad"])
    assert got["nodes"].tobytes() == want["nodes"].tobytes(), first_difference(got["nodes"], want["nodes"])
    K.check(s.tris, s.extra, s.rank, got["nodes"], got["order"], got["pad"], got["max_stack"], 2, True, got["wide"], got["wide_max_stack"], scales[0])
    for scale in scales[1:]:
        again = device(U, name, scale)
        assert again["nodes"].tobytes() == want["nodes"].tobytes() and np.array_equal(again["order"], want["order"])
        K.check(s.tris, s.extra, s.rank, again["nodes"], again["order"], again["pad"], again["max_stack"], 2, True, again["wide"], again["wide_max_stack"], scale)


def test_two_builds_give_identical_bytes(U):
    a, b = device(U, "u20k"), device(U, "u20k")
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["wide"].tobytes() == b["wide"].tobytes()
    assert np.array_equal(a["order"], b["order"]) and np.array_equal(a["pad"], b["pad"]) and (a["max_stack"], a["wide_max_stack"]) == (b["max_stack"], b["wide_max_stack"])


@pytest.mark.parametrize("n", [2, 0])
def test_too_few_triangles_are_the_builders_invalid_argument(U, n):
    s = S.soup("n5")
    rc, out = U.fast_tree(s.tris[:n], s.rank[:n] % max(n, 1), 1, 0.0, 1.0)          # (fast_tree asserts that a refused call wrote nothing)
    assert rc == -5 and out is None and "device tree build: invalid argument" in runtime.last_error()


def traverse(G, U, name, builder):
    G.clear_error()
    sc = scenes.build_scene(G, S.scene_desc(name), tree_mode=1, tree_builder=builder)
    assert runtime.last_error() == "", runtime.last_error()
    try:
        ti = runtime.TraversalInfo(); runtime.check(G.traversal_info(sc, C.byref(ti)))
        assert ti.fast_tree == 1 and ti.fast_tree_built_on_device == builder, ti.note
        o, d = S.rays(name)
        fast = U.bvh_traverse_fast(sc, o, d)[:3]
        walk = U.bvh_traverse(sc, o, d)
    finally:
        G.scene_destroy(sc)
    return fast, walk


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


@pytest.mark.parametrize("name", [n for n in S.NAMES if len(S.soup(n).tris) > 64])
def test_both_builders_trees_traverse_like_the_reference_tree(G, U, name):
    fast0, walk0 = traverse(G, U, name, 0)
    fast1, walk1 = traverse(G, U, name, 1)
    print(f"{name}: {walk0[0].mean():.3f} of the rays hit")
    assert walk0[0].mean() >= 0.5
    assert same(walk0, walk1)
    assert same(fast0, walk0), ("host-built", int((fast0[0] != walk0[0]).sum()), int((fast0[1] != walk0[1]).sum()))
    assert same(fast1, walk1), ("device-built", int((fast1[0] != walk1[0]).sum()), int((fast1[1] != walk1[1]).sum()))
    assert same(fast0, fast1)
