"""Nearest first on the host (csrc/traverse_ref.h "Nearest first"): the cut of the pair form's leaf loop drops an entry whose box the ray enters
strictly beyond the record. That is exact only if, for every triangle a ray HITS, the entry distance of its own leaf box as the flat loop computes it lies strictly
below the depth the watertight test computes. No GPU needed.

Held here over seeded rays through the Cornell box and through a scene of quads that stand diagonally in their boxes (`diagonal_quads`, also rendered by
tests/test_leaf_nearest_gpu.py):

* the box planes are the commit's (terra_amd_scene_leaf_boxes), a triangle's box is the one whose mask holds its rank;
* the entry distance is slab_near_far_fused's, operation for operation: inv = 1 / d and oi = o * inv rounded to float32, t = fma ( near plane, inv, -oi ) with ONE
  rounding (the float64 sum is rounded to odd before the conversion to float32, so the two roundings equal the single one of a fused multiply-add), the largest of
  the three and of 0 -- then the low five bits cleared, as the key of the flat loop holds it;
* the depth is the oracle's watertight test (orc_watertight), the arithmetic the device's pair test repeats bit for bit (tests/test_leaf_pairs_gpu.py);
* every ray the tame-ray condition admits is checked against every triangle; the tests assert how many rays they drew, that none of the tame ones was left out,
  and that the rays did hit.

The rays' directions are taken as drawn: camera and bounce rays of unit length, random ones of any length (ray-sourced launches do not normalise). Entry distance
and depth are both parameters along the same direction and scale alike.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from terra_amd import runtime, scenes
from test_leaf_rank import _ranks
from test_leaf_boxes import _random_rays, _path_rays, _tame


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


DIAGONAL_COLOURS = [(1.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, 4.0), (8.0, 8.0, 0.0), (0.0, 3.0, 3.0), (5.0, 0.0, 5.0), (0.5, 0.5, 0.5), (2.0, 1.0, 0.25)]


def diagonal_quads(width=64, height=48, spp=8, bounces=3, **kw) -> scenes.SceneDesc:
    """Eight quads standing diagonally in their leaf boxes, one behind the other and overlapping on the screen, in front of a wall and over a floor: ten quads, ten
    distinct boxes, the pair form. Four slant in y-z (a louvre), four in x-z (a door ajar), alternating; a ray that enters such a box passes over or under the quad
    more often than it hits it, so the nearest box's pair is often missed and the record is found in a later trip. Every quad is an emitter of its own colour."""
    objs = []
    for k in range(8):
        z0 = -0.6 + 0.3 * k; z1 = z0 + 0.7                      # the boxes overlap in depth
        w = 0.75 - 0.05 * k; y0 = 0.25 + 0.06 * k; y1 = y0 + 1.0
        if k % 2 == 0:                                          # slanted in y-z, alternately rising towards and away from the camera
            za, zb = (z0, z1) if k % 4 == 0 else (z1, z0)
            q = scenes._quad((-w, y0, za), (w, y0, za), (w, y1, zb), (-w, y1, zb), (0, 0, -1))
        else:                                                   # slanted in x-z
            za, zb = (z0, z1) if k % 4 == 1 else (z1, z0)
            q = scenes._quad((-w, y0, za), (w, y0, zb), (w, y1, zb), (-w, y1, za), (0, 0, -1))
        objs.append(scenes.ObjectDesc(*scenes._merge([q]), scenes.Material(albedo=(0.6, 0.6, 0.6), emissive=DIAGONAL_COLOURS[k]), "slant%d" % k))
    room = scenes._merge([scenes._quad((-1.5, 0, 2.6), (1.5, 0, 2.6), (1.5, 2.5, 2.6), (-1.5, 2.5, 2.6), (0, 0, -1)),
                          scenes._quad((-1.5, 0, -1.5), (1.5, 0, -1.5), (1.5, 0, 2.6), (-1.5, 0, 2.6), (0, 1, 0))])
    objs.append(scenes.ObjectDesc(*room, scenes.Material(albedo=(0.7, 0.7, 0.7), emissive=(0.25, 0.25, 0.25)), "room"))
    d = scenes.SceneDesc(objects=objs, width=width, height=height, spp=spp, bounces=bounces, name="diagonal-quads")
    for k, v in kw.items():
        setattr(d, k, v)
    assert d.triangle_count == 20
    return d


SCENES = {"cornell": lambda: scenes.cornell_box(16, 16, 1), "diagonal-quads": lambda: diagonal_quads(16, 16, 1)}


class Committed:
    """what the rays are drawn from (tests/test_leaf_boxes.py _random_rays / _path_rays read tris, n, d) and the commit's boxes"""

    def __init__(self, L, d):
        scene = scenes.build_scene(L, d)
        self.d = d
        self.n = d.triangle_count
        self.tris = np.concatenate([ob.triangles.reshape(-1, 3, 3) for ob in d.objects]).astype(np.float32)
        self.ranks = _ranks(L, scene, self.n)
        self.table = runtime.scene_leaf_boxes(L, scene)
        self.pairs, self.masks = runtime.scene_leaf_pairs(L, scene)
        L.scene_destroy(scene)
        box_of_rank = {r: k for k, m in enumerate(self.table["mask"]) for r in range(32) if int(m) >> r & 1}
        self.box_of_tri = np.array([box_of_rank[int(r)] for r in self.ranks])


def fma32(a, b, c):
    """float32 fma ( a, b, c ), exactly: a * b is exact in float64; the float64 sum, rounded to odd, converts to float32 with the rounding of the exact sum"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                             # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def entry_distances(table, o, d):
    """slab_near_far_fused's t_enter of every box for one tame ray, with the low five bits cleared (the flat loop's key without its index)"""
    inv = (np.float32(1.0) / d).astype(np.float32)
    oi = (o * inv).astype(np.float32)
    near = np.where(inv < 0, table["max"], table["min"]).astype(np.float32)          # [box, axis]
    tn = fma32(near, np.broadcast_to(inv, near.shape), np.broadcast_to(-oi, near.shape))
    te = np.maximum(tn.max(axis=1), np.float32(0))
    return (te.view(np.uint32) & np.uint32(0xffffffe0)).view(np.float32), te


def check_rays(orc, c, rays):
    f = orc.fn("orc_watertight", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    out = np.zeros(8, np.float32)
    soup = np.ascontiguousarray(c.tris.reshape(-1, 9))
    drawn = tame = checked = hits = 0
    closest_margin = np.inf
    for o, d in rays:
        drawn += 1
        o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = (np.float32(1.0) / d).astype(np.float32)
        if not _tame(inv):
            continue                                            # the flat loop never sees this ray: its wave walks the tree
        tame += 1
        key, te = entry_distances(c.table, o, d)
        assert np.all(key <= te)                                # clearing the low bits rounds down
        for t in range(c.n):
            if f(o.ctypes.data, d.ctypes.data, soup.ctypes.data + 36 * t, out.ctypes.data):
                depth = out[3]
                k = c.box_of_tri[t]
                assert key[k] < depth, (o, d, t, float(key[k]), float(depth))
                closest_margin = min(closest_margin, float(depth) - float(key[k]))
                hits += 1
        checked += 1
    return dict(drawn=drawn, tame=tame, checked=checked, hits=hits, margin=closest_margin)


@pytest.mark.parametrize("name", list(SCENES))
def test_every_box_holds_one_entry(L, name):
    """what the flat loop numbers its keys by: box k holds exactly entry k (the host switches nearest first off for a scene where that fails)"""
    c = Committed(L, SCENES[name]())
    assert len(c.pairs) == len(c.table) == c.n // 2
    assert [int(m) for m in c.masks] == [1 << k for k in range(len(c.table))]


@pytest.mark.parametrize("name", list(SCENES))
def test_entry_distance_lies_below_the_depth(L, H, orc_lib, name):
    c = Committed(L, SCENES[name]())
    n_random, n_path = 1500, 1500
    got = [check_rays(orc_lib, c, _random_rays(c, 300 + len(name), n_random)), check_rays(orc_lib, c, _path_rays(c, 400 + len(name), n_path))]
    for g, n in zip(got, (n_random, n_path)):
        assert g["drawn"] == n and g["checked"] == g["tame"]   # 3,000 rays per scene; no tame ray was skipped
        assert g["tame"] >= n * 9 // 10                         # (one random ray in 17 is axis-parallel by construction: not tame, not the flat loop's)
        assert g["hits"] >= n // 2 and g["margin"] > 0
    print(name, got)


def test_the_switch_refuses_other_values(L):
    scene = scenes.build_scene(L, scenes.cornell_box(16, 16, 1))
    assert L.get_leaf_nearest_first(scene) == 1
    assert L.set_leaf_nearest_first(scene, 2) != 0 and L.set_leaf_nearest_first(scene, -1) != 0 and L.get_leaf_nearest_first(scene) == 1
    L.clear_error()
    assert L.set_leaf_nearest_first(scene, 0) == 0 and L.get_leaf_nearest_first(scene) == 0
    L.scene_destroy(scene)
