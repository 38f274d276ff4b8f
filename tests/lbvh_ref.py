"""The device LBVH (terra_amd/csrc/tree_build_device.hip) restated in numpy and Python integers, kernel by kernel and operation by operation, so that the
builder's whole output -- the DevNode array, the soup's order, the ranks and the stack bound -- can be compared bit for bit. It reads nothing from the library.

Why the comparison can be exact: the library is built with -ffp-contract=off and correctly rounded float division, every float operation below is one binary32
(or, for the 1e-4, one binary64) operation that numpy performs the same way, the hierarchy is integer logic on the sorted 64-bit keys, fminf / fmaxf unions do not
depend on the order the fit's lanes arrive in, and the compaction is an exclusive sum in Karras index order.

  k_boxes      triangle box = (float) ((double) min - 1e-4) - extra, (float) ((double) max + 1e-4) + extra; centre = 0.5f * (mn + mx); the bounds of the centres
               through atomicMin / atomicMax on ordered(), a monotone map of the float's bits (so -0 sorts below +0)
  k_keys       t = ext > 0 ? (c - lo) / ext : 0;  q = (uint32) fminf (fmaxf (t * 1024, 0), 1023);  morton = spread10 (qx) << 2 | spread10 (qy) << 1 | spread10 (qz);
               key = morton << 32 | i
  (hipCUB)     ascending radix sort of the keys, bits 0 .. 61
  k_hierarchy  Karras 2012 section 4 with delta (i, j) = clz64 (key[i] ^ key[j]), -1 out of range
  k_fit        leaf box k = box of triangle (uint32) key[k]; inner box = union of its two children's
  k_keep       keep[i] = i == 0 or last - first + 1 > TERRA_LBVH_LEAF_MAX (2)
  (hipCUB)     new_index = exclusive sum of keep over the Karras index
  k_emit       per kept node and slot: a leaf child -> (leaf box, LEAF | k); a child not kept -> (its box, LEAF | (last - first) << 27 | first); else (its box,
               new_index[child]); prim words 0; depth = 1 + the number of ancestors
  k_soup       out[k] = tris[(uint32) key[k]] with pad = rank of that triangle
  host         n_nodes = new_index[n - 1]; max_stack = deepest kept node + 1

On an axis with an extent the largest centre has t = 1 exactly ((hi - lo) / (hi - lo)), so t * 1024 = 1024 and the clamp to 1023 runs for any such input.
"""
from __future__ import annotations

import numpy as np

LEAF_MAX = 2                    # TERRA_LBVH_LEAF_MAX
CHILD_LEAF = 0x80000000
CHILD_EMPTY = 0xFFFFFFFF

# DevNode (terra_amd/csrc/dev_types.h): 64 bytes
NODE = np.dtype([("min0", "<f4", 3), ("max0", "<f4", 3), ("min1", "<f4", 3), ("max1", "<f4", 3), ("child", "<u4", 2), ("prim", "<u4", 2)])
assert NODE.itemsize == 64
# DevFastNode: q[axis][direction group][child], child[4], pad[4]
WIDE = np.dtype([("q", "<u4", (3, 2, 4)), ("child", "<u4", 4), ("pad", "<u4", 4)])
assert WIDE.itemsize == 128

f32 = np.float32


def tri_boxes(tris, extra=0.0):
    """tri_box: (n, 3, 3) float32 vertices -> (mn, mx), each (n, 3) float32"""
    tris = np.ascontiguousarray(tris, f32).reshape(-1, 3, 3)
    lo = np.minimum(tris[:, 0], np.minimum(tris[:, 1], tris[:, 2]))
    hi = np.maximum(tris[:, 0], np.maximum(tris[:, 1], tris[:, 2]))
    mn = (lo.astype(np.float64) - 1e-4).astype(f32) - f32(extra)
    mx = (hi.astype(np.float64) + 1e-4).astype(f32) + f32(extra)
    return mn, mx


def ordered(f):
    u = np.ascontiguousarray(f, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unordered(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(f32)


def spread10(v):
    v = np.asarray(v, np.uint64)
    for mul, mask in ((0x00010001, 0xFF0000FF), (0x00000101, 0x0F00F00F), (0x00000011, 0xC30C30C3), (0x00000005, 0x49249249)):
        v = ((v * np.uint64(mul)) & np.uint64(0xFFFFFFFF)) & np.uint64(mask)
    return v


def morton_keys(mn, mx):
    """k_boxes' centre bounds and k_keys: (n,) uint64 keys, unsorted, plus the quantised coordinates (n, 3)"""
    with np.errstate(over="ignore"):
        c = f32(0.5) * (mn + mx)
    lo = unordered(ordered(c).min(axis=0)); hi = unordered(ordered(c).max(axis=0))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ext = (hi - lo).astype(f32)
        t = np.where(ext > 0, ((c - lo).astype(f32) / ext).astype(f32), f32(0)).astype(f32)
        t = np.minimum(np.maximum((t * f32(1024)).astype(f32), f32(0)), f32(1023))
    q = t.astype(np.uint32)
    m = (spread10(q[:, 0]) << np.uint64(2)) | (spread10(q[:, 1]) << np.uint64(1)) | spread10(q[:, 2])
    return (m << np.uint64(32)) | np.arange(len(c), dtype=np.uint64), q


def clz64(x):
    """__clzll on an array of uint64 (64 for 0)"""
    x = np.array(x, np.uint64)
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> np.uint64(64 - s)) == 0
        n += np.where(top_clear, s, 0)
        x = np.where(top_clear, x << np.uint64(s), x)
    return n + (x == 0)


def hierarchy(keys):
    """k_hierarchy on the sorted keys, every inner node at once. Returns child (n - 1, 2) and range (n - 1, 2) as int64 (a leaf child k is ~k), parent_inner (n - 1,)
    and parent_leaf (n,)"""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    i = np.arange(n - 1, dtype=np.int64)

    def delta(j):
        ok = (j >= 0) & (j < n)
        jj = np.where(ok, j, 0)
        return np.where(ok, clz64(keys[i] ^ keys[jj]), -1)

    d = np.where(delta(i + 1) - delta(i - 1) >= 0, 1, -1)
    dmin = delta(i - d)
    lmax = np.full(n - 1, 2, np.int64)
    while True:                                     # while ( delta ( i + lmax * d ) > dmin ) lmax <<= 1;
        m = delta(i + lmax * d) > dmin
        if not m.any():
            break
        lmax = np.where(m, lmax << 1, lmax)
    l = np.zeros(n - 1, np.int64); t = lmax >> 1
    while (t >= 1).any():                           # for ( t = lmax >> 1; t >= 1; t >>= 1 ) if ( delta ( i + ( l + t ) * d ) > dmin ) l += t;
        m = (t >= 1) & (delta(i + (l + t) * d) > dmin)
        l = np.where(m, l + t, l); t = t >> 1
    j = i + l * d
    dnode = delta(j)
    s = np.zeros(n - 1, np.int64); t = l.copy(); active = np.ones(n - 1, bool)
    while active.any():                             # do { t = ( t + 1 ) >> 1; if ( delta ( i + ( s + t ) * d ) > dnode ) s += t; } while ( t > 1 );
        t = np.where(active, (t + 1) >> 1, t)
        m = active & (delta(i + (s + t) * d) > dnode)
        s = np.where(m, s + t, s)
        active &= t > 1
    gamma = i + s * d + np.minimum(d, 0)
    first = np.minimum(i, j); last = np.maximum(i, j)
    left = np.where(first == gamma, ~gamma, gamma); right = np.where(last == gamma + 1, ~(gamma + 1), gamma + 1)
    child = np.stack([left, right], 1); rng = np.stack([first, last], 1)
    parent_inner = np.full(n - 1, -2, np.int64); parent_leaf = np.full(n, -2, np.int64)
    for c in (left, right):
        parent_leaf[~c[c < 0]] = i[c < 0]
        parent_inner[c[c >= 0]] = i[c >= 0]
    parent_inner[0] = -1
    return child, rng, parent_inner, parent_leaf


def depths(parent_inner):
    """1 + the number of ancestors of every inner node (k_emit's loop), top-down one level at a time"""
    n1 = len(parent_inner)
    depth = np.zeros(n1, np.int64); depth[0] = 1
    todo = np.arange(1, n1)
    while len(todo):                                # a node's depth is known one pass after its parent's
        p = parent_inner[todo]
        assert (p >= 0).all(), "an inner node other than the root has no parent"
        known = depth[p] > 0
        assert known.any(), "inner nodes that do not hang below the root"
        depth[todo[known]] = depth[p[known]] + 1
        todo = todo[~known]
    return depth


def build(tris, rank, extra=0.0):
    """terra_build_fast_tree_device. tris (n, 3, 3) float32, rank (n,) uint32, n > 2"""
    tris = np.ascontiguousarray(tris, f32).reshape(-1, 3, 3)
    n = len(tris)
    assert n > LEAF_MAX
    mn, mx = tri_boxes(tris, extra)
    keys0, q = morton_keys(mn, mx)
    keys = np.sort(keys0)
    child, rng, parent_inner, parent_leaf = hierarchy(keys)
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    leaf_mn, leaf_mx = mn[order], mx[order]
    # k_fit: an inner node's box once both children have theirs -- deepest level first
    depth = depths(parent_inner)
    in_mn = np.zeros((n - 1, 3), f32); in_mx = np.zeros((n - 1, 3), f32)

    def boxes_of(c):
        leaf = c < 0
        k = np.where(leaf, ~c, 0); j = np.where(leaf, 0, c)
        return np.where(leaf[:, None], leaf_mn[k], in_mn[j]), np.where(leaf[:, None], leaf_mx[k], in_mx[j])

    for level in range(int(depth.max()), 0, -1):
        idx = np.nonzero(depth == level)[0]
        a_mn, a_mx = boxes_of(child[idx, 0]); b_mn, b_mx = boxes_of(child[idx, 1])
        in_mn[idx] = np.minimum(a_mn, b_mn); in_mx[idx] = np.maximum(a_mx, b_mx)
    # k_keep and the exclusive sum
    keep = (np.arange(n - 1) == 0) | (rng[:, 1] - rng[:, 0] + 1 > LEAF_MAX)
    new_index = np.concatenate([[0], np.cumsum(keep)])[:n - 1]
    n_nodes = int(keep.sum())
    # k_emit
    nodes = np.zeros(n_nodes, NODE)
    kept = np.nonzero(keep)[0]
    for slot, (fmn, fmx) in enumerate((("min0", "max0"), ("min1", "max1"))):
        c = child[kept, slot]
        leaf = c < 0
        j = np.where(leaf, 0, c)
        collapsed = ~leaf & ~keep[j]
        b_mn, b_mx = boxes_of(c)
        word = np.where(leaf, CHILD_LEAF | (~c & 0xFFFFFFFF),
                        np.where(collapsed, CHILD_LEAF | ((rng[j, 1] - rng[j, 0]) << 27) | rng[j, 0], new_index[j]))
        nodes[fmn][new_index[kept]] = b_mn; nodes[fmx][new_index[kept]] = b_mx
        nodes["child"][new_index[kept], slot] = word.astype(np.uint32)
    max_stack = int(depth[kept].max()) + 1
    return dict(nodes=nodes, n_nodes=n_nodes, order=order, pad=np.asarray(rank, np.uint32)[order], max_stack=max_stack,
                keys=keys, q=q, child=child, range=rng, parent_inner=parent_inner, keep=keep, depth=depth)
