"""The commit-time table of distinct leaf boxes (terra_amd_scene_leaf_boxes) and the set relation the flat leaf-box test rests on. No GPU needed.

A ranked launch may test every distinct leaf box of the scene instead of walking the tree (csrc/traverse_ref.h "Flat leaf-box test"). Here:
  * the table's structure: the masks partition the ranks, every triangle's leaf box in the committed tree equals its entry's planes bit for bit, no two entries
    are equal, the Cornell box has 16, scenes of more than 32 triangles have none;
  * the set relation: over random and path-like rays, the ranks the culled tree walk collects are a subset of the ranks the flat test collects (with the same
    slab arithmetic on the same floats, in the reference's form and in the fused form the device applies), and no triangle of the difference is hit by a
    double-precision Moeller-Trumbore test -- so the closest hit cannot change.
"""
from __future__ import annotations

import numpy as np
import pytest

from terra_amd import runtime, scenes
from test_leaf_rank import _boxes, _ranks
from test_oracle_vs_reference import soup_scene


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


def coincident_scene(H):
    d = soup_scene(H, 12, 5, n_objects=2)          # (the scene of test_leaf_rank.py::test_leaf_ranks_coincident_triangles)
    for ob in d.objects:
        ob.triangles[:] = ob.triangles[0]
    return d


SCENES = {"cornell": lambda H: scenes.cornell_box(16, 16, 1), "coincident": coincident_scene}
for _n, _seed in [(1, 11), (2, 12), (3, 13), (5, 14), (17, 16), (31, 17), (32, 18)]:
    SCENES[f"soup{_n}"] = (lambda n, seed: lambda H: soup_scene(H, n, seed, n_objects=min(3, n)))(_n, _seed)


class Committed:
    """the host side of a committed scene: reference tree, ranks, soup, table"""

    def __init__(self, L, H, d):
        scene = scenes.build_scene(L, d)
        self.nodes = H.Unit("amd").bvh_nodes(scene)
        self.n = sum(len(ob.triangles) for ob in d.objects)
        self.ranks = _ranks(L, scene, self.n)
        self.table = runtime.scene_leaf_boxes(L, scene)
        L.scene_destroy(scene)
        self.first = np.cumsum([0] + [len(ob.triangles) for ob in d.objects])
        self.tris = np.concatenate([ob.triangles.reshape(-1, 3, 3) for ob in d.objects]).astype(np.float32) if self.n else np.zeros((0, 3, 3), np.float32)
        self.d = d
        b0, b1 = _boxes(self.nodes)
        self.child_box = np.stack([b0, b1], 1)                                   # [node, child, min/max, axis]
        self.idx, self.typ = self.nodes[:, 12:14].view(np.int32), self.nodes[:, 14:16].view(np.int32)

    def soup_of(self, ref):
        return int(self.first[ref & 0xff] + (ref >> 8))          # HostNode leaf index = object | triangle << 8


@pytest.fixture(scope="module")
def committed(L, H):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Committed(L, H, SCENES[name](H))
        return cache[name]
    return get


# ---- the table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_table_structure(committed, name):
    c = committed(name)
    t = c.table
    assert 1 <= len(t) <= min(c.n, 32)
    masks = [int(m) for m in t["mask"]]
    assert all(masks) and sum(masks) == (1 << c.n) - 1                 # non-empty ...
    acc = 0
    for m in masks:
        assert acc & m == 0                                           # ... disjoint: with the sum above, a partition of the ranks 0 .. n - 1
        acc |= m
    lowest = [(m & -m) for m in masks]
    assert lowest == sorted(lowest)                                   # ordered by lowest rank
    planes = np.concatenate([t["min"], t["max"]], 1).view(np.uint32)
    assert len({p.tobytes() for p in planes}) == len(t)               # no two entries are equal
    entry_of_rank = {r: k for k, m in enumerate(masks) for r in range(32) if m >> r & 1}
    seen = 0
    for k in range(len(c.nodes)):
        for ch in (0, 1):
            if c.typ[k, ch] != 1:
                continue                                              # (an inner child, or the empty slot of a scene of fewer than 2 triangles)
            tri = c.soup_of(int(c.idx[k, ch]))
            e = entry_of_rank[int(c.ranks[tri])]
            assert np.array_equal(c.child_box[k, ch].reshape(6).view(np.uint32), planes[e]), (k, ch)
            seen += 1
    assert seen == c.n
    if name == "cornell":
        assert len(t) == 16 and c.n == 32
        assert all(bin(m).count("1") == 2 for m in masks)             # the two triangles of every quad share one box
    if name == "coincident":
        assert len(t) == 2                                            # two objects, each with all of its triangles in one place
    if name == "soup1":
        assert len(t) == 1 and masks == [1]


@pytest.mark.parametrize("n_tris,seed", [(33, 19), (64, 21)])
def test_larger_scenes_have_no_table(L, H, n_tris, seed):
    scene = scenes.build_scene(L, soup_scene(H, n_tris, seed))
    assert len(runtime.scene_leaf_boxes(L, scene)) == 0
    L.scene_destroy(scene)


def test_empty_scene_has_no_table(L):
    scene = scenes.build_scene(L, scenes.SceneDesc(objects=[], width=16, height=16, spp=1))
    assert len(runtime.scene_leaf_boxes(L, scene)) == 0
    L.scene_destroy(scene)


# ---- the set relation --------------------------------------------------------------------------------------------------------------

def _slab_reference(bmin, bmax, o, inv, oi):
    t1, t2 = (bmin - o) * inv, (bmax - o) * inv
    tmin, tmax = np.minimum(t1, t2).max(), np.maximum(t1, t2).min()
    return bool(tmax > max(tmin, 0.0))


def _slab_fused(bmin, bmax, o, inv, oi):
    # slab_near_far_fused: t = fma(plane, inv, -(o * inv)), planes picked by the sign of inv. float32 x float32 is exact in float64; the sum is then rounded once
    # more to float32 (a double rounding the device's fma does not have: both sides of the comparison below share it)
    near = np.where(inv < 0, bmax, bmin).astype(np.float64); far = np.where(inv < 0, bmin, bmax).astype(np.float64)
    tn = (near * inv.astype(np.float64) - oi.astype(np.float64)).astype(np.float32)
    tf = (far * inv.astype(np.float64) - oi.astype(np.float64)).astype(np.float32)
    return bool(tf.min() > max(tn.max(), np.float32(0)))


def _tame(inv):
    a = np.abs(inv)
    return bool(np.all(np.isfinite(inv)) and np.all(a > 0) and np.all(a < np.float32(2.0) ** 96))


def _walk_set(c, slab, o, inv, oi):
    rank_set, stack, visited = 0, [0], 0
    while stack:
        k = stack.pop(); visited += 1
        for ch in (0, 1):
            if c.typ[k, ch] not in (1, -1):          # (the empty slot of a scene of fewer than 2 triangles)
                continue
            if not slab(c.child_box[k, ch, 0], c.child_box[k, ch, 1], o, inv, oi):
                continue
            if c.typ[k, ch] == -1:
                stack.append(int(c.idx[k, ch]))
            else:
                rank_set |= 1 << int(c.ranks[c.soup_of(int(c.idx[k, ch]))])
    return rank_set, visited


def _flat_set(c, slab, o, inv, oi):
    s = 0
    for e in c.table:
        if slab(e["min"], e["max"], o, inv, oi):
            s |= int(e["mask"])
    return s


def _hit_double(tri, o, d):
    """Moeller-Trumbore in double precision, no epsilons, edges included"""
    a, b, cc = tri.astype(np.float64); o = o.astype(np.float64); d = d.astype(np.float64)
    e1, e2 = b - a, cc - a
    h = np.cross(d, e2); det = e1 @ h
    if det == 0:
        return False
    s = o - a; u = (s @ h) / det; q = np.cross(s, e1); v = (d @ q) / det; t = (e2 @ q) / det
    return bool(u >= 0 and v >= 0 and u + v <= 1 and t > 0)


def _check_rays(c, rays):
    by_rank = np.argsort(c.ranks)
    extra = tested = 0
    for o, d in rays:
        if not np.any(d):
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = (np.float32(1.0) / d).astype(np.float32); oi = (o * inv).astype(np.float32)
            forms = [_slab_reference] + ([_slab_fused] if _tame(inv) else [])      # (the device applies the fused form to tame waves only, and the flat test with it)
            for slab in forms:
                walk, _ = _walk_set(c, slab, o, inv, oi)
                flat = _flat_set(c, slab, o, inv, oi)
                assert walk & ~flat == 0, (o, d, slab.__name__, bin(walk), bin(flat))
                more = flat & ~walk
                for r in range(32):
                    if more >> r & 1:
                        assert not _hit_double(c.tris[by_rank[r]], o, d), (o, d, slab.__name__, r)
                        extra += 1
                tested += 1
    return tested, extra


def _random_rays(c, seed, n_rays):
    """drawn as test_leaf_rank.py::_check draws them, axis-parallel ones included"""
    pts = c.tris.reshape(-1, 3)
    lo, hi = pts.min(0) - 1.0, pts.max(0) + 1.0
    r = np.random.default_rng(seed)
    for i in range(n_rays):
        o = r.uniform(lo, hi).astype(np.float32)
        tgt = pts[r.integers(len(pts))] if i % 2 else r.uniform(lo, hi).astype(np.float32)
        dd = (tgt - o).astype(np.float32)
        if i % 17 == 0:
            dd[r.integers(3)] = 0.0
        yield o, dd


def _path_rays(c, seed, n_rays):
    """origins 1e-4 off random surface points, leaving in a random direction on that side; and rays from the scene's camera"""
    r = np.random.default_rng(seed)
    for i in range(n_rays):
        if i % 3 == 2:
            o = np.asarray(c.d.camera_position, np.float32)
            tgt = c.tris.reshape(-1, 3)[r.integers(3 * c.n)] + r.normal(size=3) * 0.3
            dd = (tgt - o).astype(np.float32)
            yield o, (dd / np.linalg.norm(dd)).astype(np.float32)
            continue
        a, b, cc = c.tris[r.integers(c.n)].astype(np.float64)
        u, v = r.uniform(size=2)
        if u + v > 1:
            u, v = 1 - u, 1 - v
        p = a + u * (b - a) + v * (cc - a)
        nrm = np.cross(b - a, cc - a); ln = np.linalg.norm(nrm)
        nrm = nrm / ln if ln > 0 else np.array([0.0, 0.0, 1.0])
        if r.integers(2):
            nrm = -nrm
        dd = r.normal(size=3); dd /= np.linalg.norm(dd)
        if dd @ nrm < 0:
            dd = -dd
        yield (p + 1e-4 * nrm).astype(np.float32), dd.astype(np.float32)


@pytest.mark.parametrize("name", list(SCENES))
def test_set_relation_random_rays(committed, name):
    c = committed(name)
    tested, _ = _check_rays(c, _random_rays(c, 100 + len(name), 200))
    assert tested >= 200


@pytest.mark.parametrize("name", list(SCENES))
def test_set_relation_path_like_rays(committed, name):
    c = committed(name)
    tested, _ = _check_rays(c, _path_rays(c, 200 + len(name), 200))
    assert tested >= 200
