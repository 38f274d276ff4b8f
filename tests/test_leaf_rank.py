"""Commit-time leaf ranks (terra_amd_scene_leaf_ranks) against the reference traversal's leaf order.

LDS-resident launches of at most 32 triangles collect the leaves a ray meets as a set of ranks and test them from the
lowest rank up, instead of listing them in the order met. That is the same sequence exactly when every ray's leaf
list is ordered by rank. Here both traversals walk the committed reference tree (terra_amd_scene_bvh_nodes) over
random rays, with the same box decisions, with and without the leaf-box cull, and must produce the same triangles in
the same order. No GPU needed.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from terra_amd import runtime, scenes
from test_oracle_vs_reference import soup_scene


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


def _ranks(L, scene, n):
    f = L.fn("terra_amd_scene_leaf_ranks", C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert f(scene, None, 0) == n
    out = np.zeros(max(n, 1), np.uint32)
    assert f(scene, out.ctypes.data, n) == n
    return out[:n]


def _boxes(nodes):
    f = nodes.view(np.float32)
    return f[:, 0:6].reshape(-1, 2, 3), f[:, 6:12].reshape(-1, 2, 3)      # [node, min/max, axis] of child 0 and of child 1


def _slab(bmin, bmax, o, inv):
    t1, t2 = (bmin - o) * inv, (bmax - o) * inv
    tmin, tmax = np.minimum(t1, t2).max(), np.maximum(t1, t2).min()
    return bool(tmax > max(tmin, 0.0))


def _walk(nodes, soup_of, o, d, cull, ranks):
    """(triangles in the order the list traversal tests them, triangles in the order the rank-set traversal tests them)"""
    b0, b1 = _boxes(nodes)
    idx, typ = nodes[:, 12:14].view(np.int32), nodes[:, 14:16].view(np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.float32(1.0) / d
    listed, rank_set, stack = [], 0, [0]
    while stack:
        k = stack.pop()
        hit = (_slab(b0[k, 0], b0[k, 1], o, inv), _slab(b1[k, 0], b1[k, 1], o, inv))
        for c in (0, 1):
            if typ[k, c] == -1 and hit[c]:
                stack.append(int(idx[k, c]))
        for c in (0, 1):
            if typ[k, c] == 1 and (hit[c] or not cull):
                t = soup_of(int(idx[k, c]))
                listed.append(t)
                rank_set |= 1 << int(ranks[t])
    by_rank = np.argsort(ranks)
    ranked = [int(by_rank[r]) for r in range(len(ranks)) if rank_set >> r & 1]
    return listed, ranked


def _check(L, H, d, seed, n_rays=300):
    scene = scenes.build_scene(L, d)
    nodes = H.Unit("amd").bvh_nodes(scene)
    n = sum(len(ob.triangles) for ob in d.objects)
    ranks = _ranks(L, scene, n)
    L.scene_destroy(scene)
    assert sorted(ranks.tolist()) == list(range(n))          # a permutation: one rank per triangle
    first = np.cumsum([0] + [len(ob.triangles) for ob in d.objects])
    soup_of = lambda ref: int(first[ref & 0xff] + (ref >> 8))   # HostNode leaf index = object | triangle << 8
    pts = np.concatenate([ob.triangles.reshape(-1, 3) for ob in d.objects]) if n else np.zeros((1, 3), np.float32)
    lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
    r = np.random.default_rng(seed)
    met = 0
    for i in range(n_rays):
        o = r.uniform(lo, hi).astype(np.float32)
        tgt = pts[r.integers(len(pts))] if i % 2 else r.uniform(lo, hi).astype(np.float32)
        dd = (tgt - o).astype(np.float32)
        if i % 17 == 0:
            dd[r.integers(3)] = 0.0                                # axis-parallel rays too
        if not np.any(dd):
            continue
        for cull in (False, True):
            listed, ranked = _walk(nodes, soup_of, o, dd, cull, ranks)
            assert listed == ranked, (i, cull, listed, ranked)
            met += len(listed)
    return met


def test_leaf_ranks_cornell(L, H):
    assert _check(L, H, scenes.cornell_box(16, 16, 1), 1) > 0


@pytest.mark.parametrize("n_tris,seed", [(1, 11), (2, 12), (3, 13), (5, 14), (8, 15), (17, 16), (31, 17), (32, 18), (33, 19), (47, 20), (64, 21)])
def test_leaf_ranks_random_scenes(L, H, n_tris, seed):
    _check(L, H, soup_scene(H, n_tris, seed, n_objects=min(3, n_tris)), seed)


def test_leaf_ranks_coincident_triangles(L, H):
    # a degenerate tree: every triangle in the same place, so the builder's splits say nothing about position
    d = soup_scene(H, 12, 5, n_objects=2)
    for ob in d.objects:
        ob.triangles[:] = ob.triangles[0]
    _check(L, H, d, 5)
