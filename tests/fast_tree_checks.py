"""What a fast tree must be, checked on a (binary tree, order, wide tree) triple without any knowledge of how it was built. Every rule below raises Violation
with its own message, so a test can tell WHICH rule a mutated tree broke.

Binary tree (DevNode array, root at 0; leaf word = LEAF | (count - 1) << 27 | first)
  * every node is reached exactly once from the root (so: child indices in range, no cycle, no node with two parents, no orphan);
  * with children_after_parent (the host builder's numbering and the wide tree's; NOT the device builder's, see below) every child index exceeds its parent's;
  * leaf ranges partition [0, n); a leaf holds at most leaf_max triangles (4 host, 2 device); `order` is a permutation of 0 .. n - 1; pad[k] = rank[order[k]];
  * every child box EQUALS the union of the triangle boxes below it (both builders document plain unions of the +-1e-4 (+ extra) triangle boxes);
  * the builder's max_stack = deepest node + 1 (root = 1); at most 64 for the device builder (its keys have 62 significant bits).
Wide tree (DevFastNode array, 4 children)
  * every node reached exactly once, children after their parent, fewer than 2^25 nodes; its leaf words are the binary tree's, as a multiset;
  * per used slot and axis the binary16 planes are the TIGHTEST ones with lo <= mn * scale and hi >= mx * scale, mn / mx the union of the triangle boxes below;
  * q[a][1][k] is q[a][0][k] with its halves swapped; a slot is DEV_CHILD_EMPTY exactly when its planes are 0x7bff / 0xfbff; pad words are 0;
  * max_stack = 2 + the worst number of pending entries, computed here top-down: the maximum over root-to-node paths of the sum of (children in use - 1).

The device builder numbers its nodes in Karras index order (tree_build_device.hip k_emit: out[new_index[i]], new_index an exclusive sum over i), and a Karras
node whose range extends to the LEFT of its index (d = -1 in k_hierarchy) has its children at gamma, gamma + 1 <= i: a child index below its parent's is that
numbering's normal case, not an error (tests/test_fast_tree.py shows it on six keys). Nothing reads the binary tree in index order -- fastbvh::widen follows
child words -- so for device-built trees the ordering rule is replaced by the reached-exactly-once rule alone, which is what rules out cycles.
"""
from __future__ import annotations

import numpy as np

import lbvh_ref as R

LEAF = R.CHILD_LEAF
EMPTY = R.CHILD_EMPTY
HALF_MAX_BITS, HALF_MIN_BITS = 0x7BFF, 0xFBFF          # +65504, -65504: an empty slot's inverted planes


class Violation(AssertionError):
    pass


def _need(ok, msg):
    if not ok:
        raise Violation(msg)


def _walk(child, what, children_after_parent):
    """levels of a tree given its (N, k) child words: every node reached exactly once. Returns depth (root = 1) and parent per node."""
    N = len(child)
    _need(N >= 1, f"{what}: no root")
    depth = np.zeros(N, np.int64); parent = np.full(N, -1, np.int64)
    depth[0] = 1
    frontier = np.array([0], np.int64)
    while len(frontier):
        w = child[frontier]
        inner = (w != EMPTY) & ((w & LEAF) == 0)
        par = np.broadcast_to(frontier[:, None], w.shape)[inner]; ch = w[inner].astype(np.int64)
        _need((ch < N).all(), f"{what}: child index out of range")
        _need((depth[ch] == 0).all(), f"{what}: a node is reached twice (cycle or second parent)")
        _need(len(np.unique(ch)) == len(ch), f"{what}: a node is reached twice (cycle or second parent)")
        if children_after_parent:
            _need((ch > par).all(), f"{what}: a child index does not exceed its parent's")
        depth[ch] = depth[par] + 1; parent[ch] = par
        frontier = ch
    _need((depth > 0).all(), f"{what}: a node is not reachable from the root")
    return depth, parent


def _leaf_ranges(words):
    return (words & 0x07FFFFFF).astype(np.int64), (((words >> 27) & 0xF) + 1).astype(np.int64)


def _unions_below(child, depth, tmn, tmx):
    """per node and slot, the union of the triangle boxes (tmn, tmx: leaf order) below it: leaves by ranges, inner slots deepest level first"""
    N, K = child.shape
    mn = np.full((N, K, 3), np.inf, np.float32); mx = np.full((N, K, 3), -np.inf, np.float32)
    leaf = (child != EMPTY) & ((child & LEAF) != 0)
    first, cnt = _leaf_ranges(child[leaf])
    lmn = tmn[first].copy(); lmx = tmx[first].copy()
    for j in range(1, int(cnt.max()) if len(cnt) else 0):
        m = cnt > j
        lmn[m] = np.minimum(lmn[m], tmn[first[m] + j]); lmx[m] = np.maximum(lmx[m], tmx[first[m] + j])
    mn[leaf] = lmn; mx[leaf] = lmx
    inner = (child != EMPTY) & ((child & LEAF) == 0)
    for level in range(int(depth.max()) - 1, 0, -1):
        sel = inner & (depth == level)[:, None]
        ch = child[sel].astype(np.int64)
        mn[sel] = mn[ch].min(axis=1); mx[sel] = mx[ch].max(axis=1)
    return mn, mx


def check_binary(tris, extra, rank, nodes, order, pad, max_stack, leaf_max, device):
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = len(tris)
    nodes = np.asarray(nodes); child = nodes["child"]
    depth, _ = _walk(child, "binary tree", children_after_parent=not device)
    order = np.asarray(order, np.int64)
    _need(len(order) == n and np.array_equal(np.sort(order), np.arange(n)), "order is not a permutation of the soup")
    _need(np.array_equal(np.asarray(pad, np.uint32), np.asarray(rank, np.uint32)[order]), "pad is not the rank of the triangle in its slot")
    leaf =(child != EMPTY) & ((child & LEAF) != 0)
    first, cnt = _leaf_ranges(child[leaf])
    _need((cnt <= leaf_max).all(), f"binary tree: a leaf holds more than {leaf_max} triangles")
    _need((first + cnt <= n).all(), "binary tree: a leaf range lies past the soup")
    cover = np.zeros(n + 1, np.int64)
    np.add.at(cover, first, 1); np.add.at(cover, first + cnt, -1)
    cover = np.cumsum(cover)[:n]
    _need((cover >= 1).all(), "binary tree: a leaf slot lies in no leaf")
    _need((cover <= 1).all(), "binary tree: a leaf slot lies in more than one leaf")
    # an empty slot exists only beside a root leaf that holds the whole soup (the host builder's tree of at most 4 triangles)
    _need(not (child == EMPTY).any() or (len(nodes) == 1 and child[0, 1] == EMPTY and child[0, 0] != EMPTY), "binary tree: an empty child")
    tmn, tmx = R.tri_boxes(tris[order], extra)
    mn, mx = _unions_below(child, depth, tmn, tmx)
    for c, (a, b) in enumerate((("min0", "max0"), ("min1", "max1"))):
        used = child[:, c] != EMPTY
        _need((nodes[a][used] == mn[used, c]).all() and (nodes[b][used] == mx[used, c]).all(), "binary tree: a child box is not the union of the triangle boxes below it")
    _need(int(max_stack) == int(depth.max()) + 1, f"binary tree: max_stack {max_stack} is not the deepest node {int(depth.max())} + 1")
    if device:
        _need(int(max_stack) <= 64, f"binary tree: the device builder's max_stack {max_stack} exceeds 64")
    return depth


def _half_planes(x, up):
    """x (float64) must have a binary16 h on the wanted side with the next binary16 towards x on the wrong one (tests/test_host_side.py
    test_binary16_planes_are_rounded_outward states the same of half_outward itself). Returns the mask of planes that are tightest."""
    def ok(bits):
        h16 = bits.astype(np.uint16).view(np.float16); h = h16.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            if up:
                nxt = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
                return (h >= x) & ((nxt < x) | (h == x))
            nxt = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
            return (h <= x) & ((nxt > x) | (h == x))
    return ok


def check_wide(tris, extra, nodes, order, wide, wide_max_stack, scale):
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    wide = np.asarray(wide); child = wide["child"]; q = wide["q"]
    _need(len(wide) < (1 << 25), "wide tree: 2^25 nodes or more")
    depth, parent = _walk(child, "wide tree", children_after_parent=True)
    used = child != EMPTY
    bin_child = np.asarray(nodes)["child"]
    bin_leaves = np.sort(bin_child[(bin_child != EMPTY) & ((bin_child & LEAF) != 0)]); wide_leaves = np.sort(child[used & ((child & LEAF) != 0)])
    _need(np.array_equal(bin_leaves, wide_leaves), "wide tree: its leaf words are not the binary tree's")
    _need(not wide["pad"].any(), "wide tree: a pad word is not zero")
    _need(np.array_equal(q[:, :, 1, :], (q[:, :, 0, :] >> 16) | ((q[:, :, 0, :] & 0xFFFF) << 16)), "wide tree: the two direction groups disagree")
    lo = q[:, :, 0, :] & 0xFFFF; hi = q[:, :, 0, :] >> 16                    # (N, axis, slot)
    inverted = (lo == HALF_MAX_BITS) & (hi == HALF_MIN_BITS)
    _need(inverted[np.broadcast_to(~used[:, None, :], inverted.shape)].all(), "wide tree: an empty slot without inverted planes")
    _need(not inverted[np.broadcast_to(used[:, None, :], inverted.shape)].any(), "wide tree: inverted planes on a slot in use")
    tmn, tmx = R.tri_boxes(tris[np.asarray(order, np.int64)], extra)
    mn, mx = _unions_below(child, depth, tmn, tmx)                          # (N, slot, 3)
    for a in range(3):
        xl = mn[:, :, a][used].astype(np.float64) * float(scale); xh = mx[:, :, a][used].astype(np.float64) * float(scale)
        _need(_half_planes(xl, False)(lo[:, a, :][used]).all(), "wide tree: a lower plane is not the tightest binary16 at or below its box")
        _need(_half_planes(xh, True)(hi[:, a, :][used]).all(), "wide tree: an upper plane is not the tightest binary16 at or above its box")
    # the stack: pending entries along every root-to-node path, top-down (a node with k children in use leaves up to k - 1 pending while the ray is below one)
    kids = used.sum(axis=1)
    pending = np.zeros(len(wide), np.int64)
    for level in range(1, int(depth.max()) + 1):
        sel = depth == level
        above = np.where(parent[sel] >= 0, pending[np.maximum(parent[sel], 0)], 0)
        pending[sel] = above + np.maximum(kids[sel] - 1, 0)
    _need(int(wide_max_stack) == int(pending.max()) + 2, f"wide tree: max_stack {wide_max_stack} is not the worst pending count {int(pending.max())} + 2")
    return int(pending.max())


def check(tris, extra, rank, nodes, order, pad, max_stack, leaf_max, device, wide=None, wide_max_stack=None, scale=1.0):
    check_binary(tris, extra, rank, nodes, order, pad, max_stack, leaf_max, device)
    if wide is not None:
        check_wide(tris, extra, nodes, order, wide, wide_max_stack, scale)
