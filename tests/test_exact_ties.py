"""The exact-tie scenes of tests/exact_ties.py, on the CPU: the conditions under which tests/test_exact_ties_gpu.py means anything, computed from the oracle and the
library's commit-time tables alone. No GPU needed.

* every depth the oracle's watertight test gives on the plane is 4.0 bit for bit, from interior rays and from rays on rims, corners and diagonals alike;
* the model -- argmin (depth, leaf visit rank) -- is the oracle: its raycast from z = -4 (which pushes the origin itself) and its reference traversal from the
  pushed origin name the model's triangle on every ray;
* each 32-triangle scene has the pair form with 16 entries and is LDS-resident (so that a launch can use that form; as 32 single-triangle objects it is not, and
  gets the fast tree), at least 1,000 rays hit, at least 500 tie for nearest, and on at least 64 a leaf loop that walked the entries in table order and kept "the
  first trip wins" would name a triangle of another entry, of another emission, than (depth, rank) does. Measured (hit / tie / differ): seed 0: 1,178 / 758 / 95;
  seed 5: 1,351 / 559 / 96; seed 8 reversed: 1,411 / 737 / 89. Rays on which T2 of an entry beats T1 by rank: 0 in all three (reported, not required);
* the 80-triangle scene has no pair form (the fast tree and the reference tree traverse it) and more than half of its hits tie: 1,899 / 1,463, up to 13 triangles
  on one ray.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import exact_ties as X
from terra_amd import runtime, scenes


@pytest.fixture(scope="module")
def L(amd_lib):
    lib = runtime.load(need_torch=False)
    yield lib
    lib.clear_error()                                          # (a commit without a device records that it could not upload)


@pytest.mark.parametrize("name", list(X.SCENES))
def test_every_depth_is_four(H, L, orc_lib, name):
    D = X.model_of(H, L, name)["D"]
    fin = np.isfinite(D)
    assert fin.any() and np.array_equal(D[fin].view(np.uint32), np.full(int(fin.sum()), X.DEPTH, np.float32).view(np.uint32))
    assert fin[1024:].any(axis=1).sum() > 500                   # the 33 x 33 grid: rays on edges and vertices count as hits (the double-precision fallback)


@pytest.mark.parametrize("name", list(X.SCENES))
def test_the_model_is_the_oracle(H, L, orc_lib, name):
    m = X.model_of(H, L, name)
    d = X.scene(name)
    hit, want = m["hit"], m["prim"][m["expected"]]
    found, prim, point = X.oracle_traverse(H, d)
    assert np.array_equal(found != 0, hit)
    assert np.array_equal(prim[hit].astype(np.int64), want[hit])
    o, dirs = X.rays(X.Z_PUSHED)
    assert H.same_bits(point[hit], (o + dirs * X.DEPTH).astype(np.float32)[hit])
    obj, tri, rpoint, _ = X.oracle_raycast(H, d)
    assert np.array_equal(obj >= 0, hit) and np.array_equal(obj[hit].astype(np.int64), want[hit] & 0xff) and np.array_equal(tri[hit].astype(np.int64), want[hit] >> 8)
    assert H.same_bits(rpoint[hit], point[hit])                 # the raycast's own push lands on o'


def traversal_info(L, d):
    s = scenes.build_scene(L, d, counters=False)
    ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
    L.scene_destroy(s)
    return ti


@pytest.mark.parametrize("name", list(X.PAIR_SCENES))
def test_pair_scenes_discriminate(H, L, orc_lib, name):
    m = X.model_of(H, L, name)
    hit, ties, differ = int(m["hit"].sum()), int(m["ties"].sum()), int(m["discriminating"].sum())
    report = dict(hit=hit, tie=ties, differ=differ, second_beats_first=m["second_beats_first"], most_tied=m["max_tied"])
    print(name, report)
    assert len(m["pairs"]) == 16, report
    assert sorted(m["ranks"].tolist()) == list(range(32)), report
    assert hit >= 1000 and ties >= 500 and differ >= 64, report
    assert not (m["discriminating"] & ~m["ties"]).any(), report                        # only a tie can tell the two records apart
    a, b = m["expected"][m["discriminating"]], m["first_trip"][m["discriminating"]]
    entry_of = np.zeros(32, np.int64)
    for e, p in enumerate(m["pairs"]):
        entry_of[p["tri"]] = e
    assert (b >= 0).all() and (entry_of[a] != entry_of[b]).all(), report               # between two entries, every one
    assert (X.image_of(a, m["generated"]) != X.image_of(b, m["generated"])).any(axis=1).all(), report          # of different emission: a pixel shows it
    lone = m["hit"] & ~m["ties"]
    assert np.array_equal(m["first_trip"][lone], m["expected"][lone]), report
    # a launch can have the pair form: the automatic mode keeps the reference tree with the leaf-box cull, which it does for LDS-resident scenes only
    ti = traversal_info(L, X.scene(name))
    assert ti.fast_tree == 0 and ti.leaf_cull == 1 and b"LDS-resident" in ti.note and ti.camera_limit > 4.0, ti.note
    # ... which the same triangles as 32 objects with 32 materials and 32 lights are not (why these scenes are one textured object)
    ti = traversal_info(L, X.scene(name, one_object=False))
    assert ti.fast_tree == 1 and b"not LDS-resident" in ti.note, ti.note


def test_big_scene_has_no_pair_form_and_mostly_ties(H, L, orc_lib):
    m = X.model_of(H, L, "big")
    hit, ties = int(m["hit"].sum()), int(m["ties"].sum())
    print("big", dict(hit=hit, tie=ties, most_tied=m["max_tied"]))
    assert len(m["pairs"]) == 0 and len(m["ranks"]) == 80 and sorted(m["ranks"].tolist()) == list(range(80))
    assert len(X.scene("big").objects) == 80
    assert hit >= 1000 and 2 * ties >= hit, (hit, ties)


def test_the_frame_and_the_colours():
    f = X.ray_frame().reshape(-1, 8)
    assert f.shape == (2176, 8) and (f[:2113, 2] == X.Z_ORIGIN).all() and (f[:2113, 6] == 1.0).all() and np.isinf(f[:2113, 3]).all()
    assert not f[2113:].view(np.uint32).any()                  # the padding: zero directions, inactive by the ABI
    assert len({tuple(x) for x in X.ray_xy().tolist()}) == 2113
    e = [X.emission_of(t) for t in range(80)]
    assert len(set(e)) == 80 and all(np.float32(4 * c) == 4 * c for t in e for c in t)
    assert len({X.albedo_of(t) for t in range(32)}) == 32
    d = X.scene("seed-8-reversed", albedo=True)
    assert list(d.generated) == list(range(31, -1, -1)) and np.array_equal(d.objects[0].texcoords[:, 0, 0], d.generated + 0.5)
