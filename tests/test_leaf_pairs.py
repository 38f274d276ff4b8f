"""The commit-time pair form of a scene (terra_amd_scene_leaf_pairs) and the LDS layout of a pair launch (terra_amd_leaf_pair_offsets). No GPU needed.

A scene has the pair form when every triangle is one half of a fan T1 = (a, b, c), T2 = (a, c, d) inside one distinct leaf box (csrc/traverse_ref.h "Pair form";
csrc/scene_host.cpp leaf_pair_table): the two triangles of a quad. Here:
  * the Cornell box and its Phong variant give 16 entries; every entry's two triangles share a leaf box, T2.a == T1.a and T2.b == T1.c bit for bit, the
    entries ascend by their lowest rank, the ranks are the scene's, and the boxes' masks in entry bits partition the entries and are the images of the rank masks;
  * scenes that have no pair form: a random soup, the Cornell box plus one loose triangle, the Cornell box with one quad's second triangle rotated to (c, d, a)
    -- the same triangle, another vertex order --, a quad scene of 34 triangles;
  * a quad duplicated exactly (four triangles in one box) pairs into two valid fans;
  * the offsets: entries and plane pairs disjoint and inside the section, box k's plane pairs a constant 48 k from box 0's, the section smaller than the ranked
    entries it replaces.
(tests/test_leaf_pairs_gpu.py checks through terra_amd_leaf_pair_info that the launches of the scenes without a pair form keep the single form.)
"""
from __future__ import annotations

import numpy as np
import pytest

from terra_amd import runtime, scenes
from test_leaf_rank import _ranks
from test_oracle_vs_reference import soup_scene
from test_flat_loop_layout_gpu import quads


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


def cornell_plus_loose_triangle():
    d = scenes.cornell_box(16, 16, 1)
    tri = np.array([[[-0.5, 0.5, -0.5], [0.0, 0.9, -0.5], [0.4, 0.5, -0.4]]], np.float32)
    d.objects.append(scenes.ObjectDesc(tri, np.broadcast_to(np.float32([0, 0, -1]), (1, 3, 3)).copy(), np.zeros((1, 3, 2), np.float32), scenes.Material(), "loose"))
    return d


def cornell_with_a_rotated_triangle():
    d = scenes.cornell_box(16, 16, 1)
    t = d.objects[1].triangles          # the red wall: (a, b, c), (a, c, d) -> the second one as (c, d, a)
    t[1] = t[1][[1, 2, 0]]
    return d


def quad_scene(n_quads):
    """n_quads parallel quads of different extents, one object"""
    parts = []
    for k in range(n_quads):
        h, z = 0.3 + 0.01 * k, 0.1 * k
        parts.append(scenes._quad((-h, 1 - h, z), (h, 1 - h, z), (h, 1 + h, z), (-h, 1 + h, z), (0, 0, -1)))
    return scenes.SceneDesc(objects=[scenes.ObjectDesc(*scenes._merge(parts), scenes.Material(emissive=(1.0, 1.0, 1.0)), "quads")], width=16, height=16, spp=1, name="quads")


NO_PAIR_FORM = {"soup-8": lambda H: soup_scene(H, 8, 31, n_objects=2), "soup-32": lambda H: soup_scene(H, 32, 18, n_objects=3),
                "cornell-plus-a-loose-triangle": lambda H: cornell_plus_loose_triangle(), "cornell-with-a-rotated-triangle": lambda H: cornell_with_a_rotated_triangle(),
                "34-triangle-quads": lambda H: quad_scene(17)}


def committed(L, d):
    scene = scenes.build_scene(L, d)
    n = sum(len(ob.triangles) for ob in d.objects)
    out = dict(n=n, ranks=_ranks(L, scene, n), boxes=runtime.scene_leaf_boxes(L, scene), tris=np.concatenate([ob.triangles.reshape(-1, 3, 3) for ob in d.objects]).astype(np.float32))
    out["pairs"], out["masks"] = runtime.scene_leaf_pairs(L, scene)
    L.scene_destroy(scene)
    return out


def check_pair_form(c, n_entries):
    pairs, masks, ranks, tris = c["pairs"], c["masks"], c["ranks"], c["tris"].view(np.uint32)
    assert len(pairs) == n_entries == c["n"] // 2
    assert sorted(pairs["tri"].reshape(-1).tolist()) == list(range(c["n"]))                 # every triangle in exactly one pair
    assert np.array_equal(pairs["rank"], ranks[pairs["tri"]])                                # the ranks are the scene's
    low = pairs["rank"].min(1)
    assert np.all(low[1:] > low[:-1])                                                        # entries ascend by their lowest rank
    box_of_rank = {r: k for k, m in enumerate(c["boxes"]["mask"]) for r in range(32) if int(m) >> r & 1}
    for e, p in enumerate(pairs):
        t1, t2 = tris[p["tri"][0]], tris[p["tri"][1]]
        assert np.array_equal(t2[0], t1[0]) and np.array_equal(t2[1], t1[2]), e               # the fan, bit for bit: T2.a == T1.a, T2.b == T1.c
        assert box_of_rank[int(p["rank"][0])] == box_of_rank[int(p["rank"][1])], e            # the two share a distinct leaf box
    # the boxes' masks in entry bits: a partition of the entries, each the image of the box's rank mask
    assert len(masks) == len(c["boxes"])
    assert sum(int(m) for m in masks) == (1 << n_entries) - 1 and all(int(a) & int(b) == 0 for i, a in enumerate(masks) for b in masks[:i])
    for k, m in enumerate(masks):
        image = 0
        for e, p in enumerate(pairs):
            in_box = [int(c["boxes"]["mask"][k]) >> int(r) & 1 for r in p["rank"]]
            assert in_box[0] == in_box[1]
            image |= in_box[0] << e
        assert int(m) == image, k


@pytest.mark.parametrize("mk", [scenes.cornell_box, scenes.cornell_phong], ids=["cornell", "cornell-phong"])
def test_cornell_has_sixteen_pairs(L, mk):
    c = committed(L, mk(16, 16, 1))
    assert c["n"] == 32 and len(c["boxes"]) == 16
    check_pair_form(c, 16)
    # entry order is not rank order across pairs: some pair starts between the two ranks of an earlier one (why the leaf loop's record is (depth, rank))
    r = c["pairs"]["rank"]
    assert any(r[e].max() > r[e + 1:].min() for e in range(15))


@pytest.mark.parametrize("name", list(NO_PAIR_FORM))
def test_scenes_without_a_pair_form(L, H, name):
    c = committed(L, NO_PAIR_FORM[name](H))
    assert len(c["pairs"]) == 0 and len(c["masks"]) == 0


def test_empty_scene_has_no_pair_form(L):
    scene = scenes.build_scene(L, scenes.SceneDesc(objects=[], width=16, height=16, spp=1))
    pairs, masks = runtime.scene_leaf_pairs(L, scene)
    assert len(pairs) == 0 and len(masks) == 0
    L.scene_destroy(scene)


@pytest.mark.parametrize("reverse", [False, True], ids=["given-order", "reversed"])
def test_a_quad_duplicated_exactly_pairs_into_two_fans(L, reverse):
    c = committed(L, quads((0.0, 0.5, 1.0, 0.0), reverse))
    assert c["n"] == 8 and len(c["boxes"]) == 3
    check_pair_form(c, 4)
    assert sorted(bin(int(m)).count("1") for m in c["masks"]) == [1, 1, 2]              # the duplicate's box holds two entries


def test_32_triangle_quads_have_the_pair_form(L):
    check_pair_form(committed(L, quad_scene(16)), 16)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 15, 16])
def test_offsets_of_the_pair_section(L, n):
    entries, planes, size = runtime.leaf_pair_offsets(L, n)
    assert size == 6 * n * 64 + n * 48 and size <= 6 * 48 * 2 * n                        # never more than the ranked entries of the 2 n triangles
    spans = sorted([(int(o), 64) for o in entries.reshape(-1)] + [(int(o), 8) for o in planes.reshape(-1)])
    assert spans[0][0] == 0 and all(a + w <= b for (a, w), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == size      # disjoint, inside, no gap
    assert np.all(entries % 16 == 0) and np.all(planes % 8 == 0)
    assert np.array_equal(entries, (np.arange(6)[:, None] * n + np.arange(n)[None, :]) * 64)
    assert np.array_equal(planes - planes[0], np.broadcast_to((48 * np.arange(n))[:, None, None], planes.shape))                             # box k: an immediate from box 0
    assert planes[min(7, n - 1), 0, 0] - planes[0, 0, 0] == 48 * min(7, n - 1) <= 336


def test_offsets_refuse_more_than_sixteen_entries(L):
    assert L.leaf_pair_offsets(17, None, None) != 0 and "16" in runtime.last_error()
    L.clear_error()
