"""The fast tree's builders, widening and commit check, held to exact rules on the CPU (the device half is tests/test_fast_tree_gpu.py).

* tests/lbvh_ref.py restates the device LBVH; here it passes tests/fast_tree_checks.py on every soup of tests/fast_tree_soups.py, and its hierarchy equals the one
  worked by hand below.
* The checker rejects each of eighteen mutations of a good tree, with the message of the rule that was broken.
* The product's own commit check (verify_fast_tree, through terra_amd_unit_verify_fast_tree) accepts the good tree and refuses the structural mutations, each for
  its own reason; the cycle runs in a child process under a time limit, so a check that loops fails instead of hanging the suite.
* The host builder through terra_amd_unit_fast_tree passes the checker on every soup at every scale and does not depend on its thread count.
* The traversal comparison of the device half needs rays of which at least half hit: asserted here with the oracle's reference traversal.

Six keys by hand (Karras 2012, figure 3's first six; as 64-bit keys the common prefix of two keys is 59 + the 5-bit one):

    k   key     delta (k, k + 1)
    0   00001   62   (00001 ^ 00010 = 00011)
    1   00010   61   (00010 ^ 00100 = 00110)
    2   00100   63   (00100 ^ 00101 = 00001)
    3   00101   59   (00101 ^ 10011 = 10110)
    4   10011   60   (10011 ^ 11000 = 01011)
    5   11000

  node 0: delta (0, 1) - delta (0, -1) = 62 + 1 >= 0, d = +1, dmin = -1; lmax grows 2 -> 4 -> 8 (delta (0, 2) = 61, delta (0, 4) = 59, 8 out of range); l = 4 + 1 = 5,
          j = 5, dnode = 59; split: t = 3: delta (0, 3) = 61 > 59, s = 3; t = 2: delta (0, 5) = 59 no; t = 1: delta (0, 4) = 59 no; gamma = 3: children (3, 4), range [0, 5]
  node 1: 61 - 62 < 0, d = -1, dmin = 61; lmax = 2 (-1 out of range); l = 1 (delta (1, 0) = 62 > 61), j = 0, dnode = 62; no step; gamma = 1 + 0 - 1 = 0: leaves (~0, ~1), [0, 1]
  node 2: 63 - 61 >= 0, d = +1, dmin = 61; l = 1, j = 3, dnode = 63; gamma = 2: leaves (~2, ~3), [2, 3]
  node 3: 59 - 63 < 0, d = -1, dmin = 59; lmax 2 -> 4 (delta (3, 1) = 61 > 59; -1 out of range); l = 2 + 1 = 3 (delta (3, 0) = 61), j = 0, dnode = 61; split: t = 2:
          delta (3, 1) = 61 no; t = 1: delta (3, 2) = 63 > 61, s = 1; gamma = 3 - 1 - 1 = 1: children (1, 2), range [0, 3] -- BOTH BELOW THEIR PARENT'S INDEX
  node 4: 60 - 59 >= 0, d = +1, dmin = 59; l = 1, j = 5, dnode = 60; gamma = 4: leaves (~4, ~5), [4, 5]
  keep = 1 0 0 1 0 (ranges of 6, 2, 2, 4, 2 triangles), new index 0 . . 1 .; emitted: node 0 = (inner 1, leaf of 2 at 4), node 1 = (leaf of 2 at 0, leaf of 2 at 2);
  deepest kept node 2, max_stack 3.
"""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

import fast_tree_checks as K
import fast_tree_soups as S
import lbvh_ref as R

LEAF, EMPTY = R.CHILD_LEAF, R.CHILD_EMPTY


@pytest.fixture(scope="module")
def U(H, amd_lib):
    return H.Unit("amd")


_ref, _host = {}, {}


def ref(name):
    if name not in _ref:
        s = S.soup(name)
        _ref[name] = R.build(s.tris, s.rank, s.extra)
    return _ref[name]


def host(U, name, scale=1.0):
    if (name, scale) not in _host:
        s = S.soup(name)
        rc, out = U.fast_tree(s.tris, s.rank, 0, s.extra, scale)
        assert rc == 0
        _host[name, scale] = out
    return _host[name, scale]


def check_ref(name, b=None, **changed):
    s = S.soup(name)
    b = dict(b or ref(name), **changed)
    K.check(s.tris, s.extra, s.rank, b["nodes"], b["order"], b["pad"], b["max_stack"], 2, True)


def check_host(name, h, scale=1.0, **changed):
    s = S.soup(name)
    h = dict(h, **changed)
    K.check(s.tris, s.extra, s.rank, h["nodes"], h["order"], h["pad"], h["max_stack"], 4, False, h["wide"], h["wide_max_stack"], scale)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.QUICK) + [pytest.param(n, id=n + "-slow-cpu-case") for n in S.SLOW])
def test_restatement_passes_the_checker(name):
    check_ref(name)
    b = ref(name)
    assert b["max_stack"] <= 63                                   # 62 significant key bits
    top = b["q"].max(axis=0)                                      # the largest centre has t = 1 -> 1024 -> the clamp, on every axis with an extent
    assert ((top == 1023) | (top == 0)).all() and ((top == 1023).any() or name == "coincident")


def test_six_keys_by_hand():
    keys = np.array([0b00001, 0b00010, 0b00100, 0b00101, 0b10011, 0b11000], np.uint64)
    child, rng, parent_inner, parent_leaf = R.hierarchy(keys)
    assert child.tolist() == [[3, 4], [~0, ~1], [~2, ~3], [1, 2], [~4, ~5]]
    assert rng.tolist() == [[0, 5], [0, 1], [2, 3], [0, 3], [4, 5]]
    assert parent_inner.tolist() == [-1, 3, 3, 0, 0] and parent_leaf.tolist() == [1, 1, 2, 2, 4, 4]
    assert R.clz64(np.array([0, 1, 1 << 63, 0b10110], np.uint64)).tolist() == [64, 63, 0, 59]
    assert R.depths(parent_inner).tolist() == [1, 3, 3, 2, 2]
    assert (child[3] < 3).all()                                   # a node whose range extends to the left has its children below its own index


def test_restatement_figures():
    """what each degenerate soup is there for, read off the restatement"""
    c = ref("coincident")
    assert len(np.unique(c["keys"] >> np.uint64(32))) == 1 and c["n_nodes"] == 499 and c["max_stack"] == 9 + 1       # keys split by the index alone: balanced
    assert np.array_equal(c["order"], np.arange(1000))
    assert not ref("planar")["q"][:, 2].any() and ref("planar")["q"][:, :2].max() == 1023                            # ext == 0 on z
    assert not ref("line")["q"][:, 1:].any()
    g = ref("geometric")
    assert len(np.unique(g["keys"] >> np.uint64(32))) == 11 and g["max_stack"] == 19 + 1
    assert not ref("signed")["q"][:, 1].any()                     # +-1e-30 vanishes beside the 1e-4 margin: every y centre is 0
    assert ref("margin")["n_nodes"] == ref("b257")["n_nodes"] and not np.array_equal(ref("margin")["nodes"]["min0"], ref("b257")["nodes"]["min0"])
    # the device builder numbers nodes in Karras index order: kept children below their parent's index are its normal case (fast_tree_checks.py)
    ch = ref("b257")["nodes"]["child"]
    inner = (ch & LEAF) == 0
    assert (ch[inner] < np.broadcast_to(np.arange(len(ch))[:, None], ch.shape)[inner]).any()


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------
def _leaf_slot(nodes, want_count=None, room=False, n=None):
    """(node, slot) of a leaf child, optionally of a given count / with a triangle slot after it"""
    ch = nodes["child"]
    for i in range(len(ch)):
        for c in range(2):
            w = int(ch[i, c])
            if w == EMPTY or not w & LEAF:
                continue
            first, cnt = w & 0x07FFFFFF, ((w >> 27) & 0xF) + 1
            if (want_count is None or cnt == want_count) and (not room or first + cnt < n):
                return i, c
    raise AssertionError("no such leaf")


def _inner_slot(nodes):
    """(node, slot) of an inner child of a node other than the root"""
    ch = nodes["child"]
    for i in range(1, len(ch)):
        for c in range(2):
            if not int(ch[i, c]) & LEAF:
                return i, c
    raise AssertionError("no inner child below the root")


def structural_mutations(nodes, n):
    """name -> (mutated copy of the binary tree, the checker's message, the product verifier's reason)"""
    out = {}

    def mutant(name, checker_says, verifier_says):
        m = nodes.copy()
        out[name] = (m, checker_says, verifier_says)
        return m

    m = mutant("leaf-dropped", "lies in no leaf", "a triangle lies in no leaf")
    i, c = _leaf_slot(m); m["child"][i, c] = EMPTY
    m = mutant("range-doubled", "lies in more than one leaf", "a triangle lies in more than one leaf")
    i, c = _leaf_slot(m, want_count=1, room=True, n=n); m["child"][i, c] += 1 << 27
    m = mutant("child-is-its-parent", "reached twice", "a node is reached twice")
    i, c = _inner_slot(m); m["child"][i, c] = i
    m = mutant("child-is-the-root", "reached twice", "a node is reached twice")
    i, c = _inner_slot(m); m["child"][i, c] = 0
    m = mutant("box-plane-one-ulp-inward", "not the union of the triangle boxes", "does not contain the triangle boxes below it")
    m["min1"][len(m) // 2, 1] = np.nextafter(m["min1"][len(m) // 2, 1], np.float32(np.inf))
    m = mutant("leaf-count-five", "a leaf holds more than", "a leaf holds more than 4 triangles")
    i, c = _leaf_slot(m); m["child"][i, c] = (int(m["child"][i, c]) & ~(0xF << 27)) | (4 << 27)
    m = mutant("range-past-the-soup", "past the soup", "leaf range out of range")
    i, c = _leaf_slot(m); m["child"][i, c] = (int(m["child"][i, c]) & ~0x07FFFFFF) | n
    return out


MUTATIONS = ("leaf-dropped", "range-doubled", "child-is-its-parent", "child-is-the-root", "box-plane-one-ulp-inward", "leaf-count-five", "range-past-the-soup")


@pytest.mark.parametrize("which", MUTATIONS)
@pytest.mark.parametrize("tree", ["host", "device-restated"])
def test_checker_rejects_structural_mutations(U, tree, which):
    name = "b257"
    good = host(U, name) if tree == "host" else ref(name)
    run = (lambda **kw: check_host(name, good, **kw)) if tree == "host" else (lambda **kw: check_ref(name, good, **kw))
    run()
    m, says, _ = structural_mutations(good["nodes"], 257)[which]
    assert m.tobytes() != good["nodes"].tobytes()
    with pytest.raises(K.Violation, match=says):
        run(nodes=m)


def test_checker_rejects_the_other_mutations(U):
    name, scale = "b257", 2.0 ** -3
    good = host(U, name, scale)
    check_host(name, good, scale)
    # one binary16 plane moved inward by one unit, both direction groups kept consistent
    w = good["wide"].copy()
    lo = np.uint16(w["q"][3, 0, 0, 0] & 0xFFFF); hi = int(w["q"][3, 0, 0, 0] >> 16)
    lo_in = int(np.nextafter(lo.view(np.float16), np.float16(np.inf)).view(np.uint16))
    w["q"][3, 0, 0, 0] = lo_in | (hi << 16); w["q"][3, 0, 1, 0] = hi | (lo_in << 16)
    with pytest.raises(K.Violation, match="lower plane is not the tightest"):
        check_host(name, good, scale, wide=w)
    w = good["wide"].copy()
    lo = int(w["q"][5, 2, 0, 1] & 0xFFFF); hi = np.uint16(w["q"][5, 2, 0, 1] >> 16)
    hi_in = int(np.nextafter(hi.view(np.float16), np.float16(-np.inf)).view(np.uint16))
    w["q"][5, 2, 0, 1] = lo | (hi_in << 16); w["q"][5, 2, 1, 1] = hi_in | (lo << 16)
    with pytest.raises(K.Violation, match="upper plane is not the tightest"):
        check_host(name, good, scale, wide=w)
    # a plane moved OUTWARD contains its box and is still refused: the rule is tightest, not merely outside
    w = good["wide"].copy()
    lo = np.uint16(w["q"][3, 0, 0, 0] & 0xFFFF); hi = int(w["q"][3, 0, 0, 0] >> 16)
    lo_out = int(np.nextafter(lo.view(np.float16), np.float16(-np.inf)).view(np.uint16))
    w["q"][3, 0, 0, 0] = lo_out | (hi << 16); w["q"][3, 0, 1, 0] = hi | (lo_out << 16)
    with pytest.raises(K.Violation, match="lower plane is not the tightest"):
        check_host(name, good, scale, wide=w)
    w = good["wide"].copy(); w["q"][2, 1, 1, 0] ^= 1
    with pytest.raises(K.Violation, match="direction groups disagree"):
        check_host(name, good, scale, wide=w)
    with pytest.raises(K.Violation, match="wide tree: max_stack"):
        check_host(name, good, scale, wide_max_stack=good["wide_max_stack"] - 1)
    with pytest.raises(K.Violation, match="binary tree: max_stack"):
        check_host(name, good, scale, max_stack=good["max_stack"] - 1)
    o = good["order"].copy(); o[1] = o[0]
    with pytest.raises(K.Violation, match="not a permutation"):
        check_host(name, good, scale, order=o)
    p = good["pad"].copy(); p[[0, 1]] = p[[1, 0]]
    with pytest.raises(K.Violation, match="pad is not the rank"):
        check_host(name, good, scale, pad=p)
    w = good["wide"].copy()
    assert (w["child"] == EMPTY).any()
    k = int(np.argmax((w["child"] == EMPTY).any(axis=1))); slot = int(np.argmax(w["child"][k] == EMPTY))
    w["q"][k, 0, 0, slot] = 0; w["q"][k, 0, 1, slot] = 0
    with pytest.raises(K.Violation, match="empty slot without inverted planes"):
        check_host(name, good, scale, wide=w)
    w = good["wide"].copy(); w["pad"][1, 2] = 1
    with pytest.raises(K.Violation, match="pad word"):
        check_host(name, good, scale, wide=w)
    w = good["wide"].copy()
    inner = (w["child"] != EMPTY) & ((w["child"] & LEAF) == 0); k = int(np.argmax(inner[1:].any(axis=1))) + 1; slot = int(np.argmax(inner[k]))
    w["child"][k, slot] = k
    with pytest.raises(K.Violation, match="wide tree: a node is reached twice"):
        check_host(name, good, scale, wide=w)


# ---- the product's commit check ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["host", "device-restated"])
def test_product_verifier_accepts_the_good_tree_and_refuses_each_mutation(U, tree):
    name = "b257"
    s = S.soup(name)
    good = host(U, name) if tree == "host" else ref(name)
    leaf_tris = s.tris[good["order"]]
    assert U.verify_fast_tree(good["nodes"], leaf_tris, s.extra) == (True, "")
    reasons = {}
    for which, (m, _, says) in structural_mutations(good["nodes"], 257).items():
        if which.startswith("child-is"):
            continue                                              # the cycles run in a child process below
        ok, why = U.verify_fast_tree(m, leaf_tris, s.extra)
        assert not ok and says in why, (which, why)
        reasons[which] = why
    assert len(set(reasons.values())) == len(reasons)            # each refusal has its own reason
    m = good["nodes"].copy(); m["child"][len(m) - 1, 0] = len(m)
    ok, why = U.verify_fast_tree(m, leaf_tris, s.extra)
    assert not ok and "child index out of range" in why
    # the margin belongs to the boxes: a tree built without it does not contain the inflated triangle boxes
    ok, why = U.verify_fast_tree(good["nodes"], leaf_tris, 0.25)
    assert not ok and "does not contain" in why


CYCLE_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import harness as H
import lbvh_ref as R
z = np.load(sys.argv[2])
U = H.Unit("amd")
print(json.dumps({k: U.verify_fast_tree(z[k].view(R.NODE), z["tris"], 0.0) for k in ("parent", "root", "good")}))
"""


def test_product_verifier_ends_on_a_cycle(H, U, tmp_path):
    """a child index that points back at its own node or at the root: refused, and within the time limit (the check keeps a visited bitmap; without one the walk
    never ends and its stack grows without bound)"""
    name = "b257"
    s = S.soup(name)
    good = ref(name)
    muts = structural_mutations(good["nodes"], 257)
    np.savez(tmp_path / "trees.npz", parent=muts["child-is-its-parent"][0].view(np.uint8), root=muts["child-is-the-root"][0].view(np.uint8), good=good["nodes"].view(np.uint8),
             tris=s.tris[good["order"]])
    r = subprocess.run([sys.executable, "-c", CYCLE_CHILD, str(H.ROOT / "tests"), str(tmp_path / "trees.npz")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["good"] == [True, ""]
    for k in ("parent", "root"):
        assert got[k][0] is False and "a node is reached twice" in got[k][1], got


# ---- the host builder --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_host_builder_passes_the_checker(U, name):
    for scale in S.scales_of(name):
        check_host(name, host(U, name, scale), scale)
    h = host(U, name)
    for scale in S.scales_of(name)[1:]:                           # the scale reaches the planes alone
        o = host(U, name, scale)
        assert o["nodes"].tobytes() == h["nodes"].tobytes() and np.array_equal(o["wide"]["child"], h["wide"]["child"]) and o["wide_max_stack"] == h["wide_max_stack"]
    if name == "signed":                                          # planes beyond binary16 at scale 1: +-65504 towards zero, +-inf away from it
        halves = np.concatenate([(h["wide"]["q"][:, 0, 0, :] & 0xFFFF).ravel(), (h["wide"]["q"][:, 0, 0, :] >> 16).ravel()])
        assert {0x7C00, 0xFC00, 0x7BFF, 0xFBFF} <= set(halves.tolist())


def test_host_builder_does_not_depend_on_its_threads(H, U):
    s = S.soup("u20k")                                            # 20,000 triangles: the smallest soup the builder shares among threads
    set_threads = H.lib("amd").fn("terra_amd_set_build_threads", C.c_int, [C.c_int])
    built = []
    try:
        for threads in (1, 3):
            assert set_threads(threads) == 0
            rc, out = U.fast_tree(s.tris, s.rank, 0, s.extra, 1.0)
            assert rc == 0
            built.append(out)
    finally:
        set_threads(0)
    a, b = built
    assert a["nodes"].tobytes() == b["nodes"].tobytes() and a["wide"].tobytes() == b["wide"].tobytes()
    assert np.array_equal(a["order"], b["order"]) and np.array_equal(a["pad"], b["pad"]) and (a["max_stack"], a["wide_max_stack"]) == (b["max_stack"], b["wide_max_stack"])
    assert a["nodes"].tobytes() == host(U, "u20k")["nodes"].tobytes()


def test_host_builder_peels_coincident_triangles(U):
    """what scene_host.cpp says beside TERRA_FAST_STACK_MAX: the deep tree over coincident geometry is the HOST builder's (its sweep takes the first of equal costs),
    not the device builder's, whose keys split such a soup by index into a balanced tree"""
    assert host(U, "coincident")["max_stack"] == 176 + 1 and host(U, "coincident")["wide_max_stack"] == 187
    assert ref("coincident")["max_stack"] == 9 + 1


def test_unit_entry_refusals(H, U):
    s = S.soup("n5")
    assert U.fast_tree(s.tris, s.rank, 2, 0.0, 1.0)[0] == -4 and "builder outside" in H.last_error()
    assert U.fast_tree(s.tris, s.rank, 0, -1.0, 1.0)[0] == -4 and U.fast_tree(s.tris, s.rank, 0, 0.0, 0.0)[0] == -4


def test_device_builder_needs_a_device(H, U):
    if H.lib("amd").fn("terra_amd_device_count", C.c_int, [])() > 0:
        pytest.skip("a device is visible: tests/test_fast_tree_gpu.py runs the builder")
    s = S.soup("n5")
    rc, out = U.fast_tree(s.tris, s.rank, 1, 0.0, 1.0)           # (fast_tree asserts that a refused call wrote nothing)
    assert rc == -1 and out is None and "no HIP device visible" in H.last_error()


# ---- the rays of the device half -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in S.NAMES if len(S.soup(n).tris) > 64])
def test_at_least_half_of_the_rays_hit(H, orc_lib, name):
    """the reference tree alone decides (the oracle's bvh_traverse); tests/test_fast_tree_gpu.py compares the device's traversals on these rays"""
    from terra_amd import scenes
    o, d = S.rays(name)
    assert len(o) == 1024 and (d[:S.N_AIMED] != 0).all() and ((d[S.N_AIMED:] == 0).sum(axis=1) >= 1).all()
    t = S.soup(name).tris.reshape(-1, 3)
    assert ((o < t.min(axis=0)) | (o > t.max(axis=0))).any(axis=1).all()          # every origin lies outside the bounds
    u = H.Unit("orc")
    sc = scenes.build_scene(u.L, S.scene_desc(name))
    try:
        found, _, _ = u.bvh_traverse(sc, o, d)
    finally:
        u.L.scene_destroy(sc)
    assert found.mean() >= 0.5, found.mean()
