"""The triangle soups the fast tree's builders are held to (tests/test_fast_tree.py on the CPU, tests/test_fast_tree_gpu.py on the device), and the rays their
committed scenes are traversed with. Everything is seeded; a soup is made once per process.

  n3 n4 n5            the smallest inputs the device builder accepts (n > TERRA_LBVH_LEAF_MAX = 2)
  b255 b256 b257      one 256-lane block less one, exactly, plus one
  coincident          one triangle 1,000 times: every Morton code equal, the keys differ in the index alone
  planar              2,000 axis-aligned right triangles exactly in z = 0: the centres' z extent is 0 (k_keys' `ext > 0 ? .. : 0` arm)
  line                500 triangles whose box centres lie on the x axis: two degenerate axes
  geometric           40 copies of centres 2^-k (1, 1, 1), k = 0 .. 23, jittered by 1e-9: long runs of equal codes beside single ones -- the deepest tree here
  signed              2,000 triangles, x within +-1e30, y within +-1e-30, z within +-1, some vertices exactly +0.0 / -0.0: negative floats through ordered(), a y
                      extent that vanishes beside the 1e-4 margin, and planes beyond binary16's range at scale 1
  big_small           one triangle spanning the whole box and 3,000 tiny ones
  margin              b257 with extra_margin = 0.25 (the reachability mode's inflated boxes)
  u20k, u150k         uniform in [-5, 5]^3; u150k is the size case for the library's sort and scan (which of their paths ran cannot be seen from here)

`rank` is a random permutation of 0 .. n - 1 in every case, so a pad word carried from the wrong triangle shows. On every axis with an extent the largest box centre
quantises to t = (hi - lo) / (hi - lo) = 1, t * 1024 = 1024: the clamp to 1023 runs in every soup but `coincident` (no extent at all) and needs no case of its own.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Soup = namedtuple("Soup", "name tris rank extra")
SCALES = (1.0, 2.0 ** -3, 2.0 ** 6)
NAMES = ("n3", "n4", "n5", "b255", "b256", "b257", "coincident", "planar", "line", "geometric", "signed", "big_small", "margin", "u20k", "u150k")
SLOW = ("u150k",)
QUICK = tuple(n for n in NAMES if n not in SLOW)


def scales_of(name):
    return (1.0,) if name == "signed" else SCALES          # signed's planes overflow binary16 at scale 1: the +-65504 / +-inf arm of half_outward


def _around(r, centres, size):
    """one triangle per centre: vertices within `size` of it"""
    c = np.asarray(centres, np.float64)
    return (c[:, None, :] + r.uniform(-1, 1, (len(c), 3, 3)) * size).astype(np.float32)


def _uniform(r, n, half, size):
    return _around(r, r.uniform(-(half - size), half - size, (n, 3)), size)


def _make(name):
    r = np.random.default_rng([0x7ee, NAMES.index(name)])
    extra = 0.0
    if name in ("n3", "n4", "n5"):
        t = _uniform(r, int(name[1:]), 1.0, 0.3)
    elif name in ("b255", "b256", "b257"):
        t = _uniform(r, int(name[1:]), 1.0, 0.1)
    elif name == "margin":
        t = _make("b257").tris.copy(); extra = 0.25
    elif name == "coincident":
        t = np.repeat(_uniform(r, 1, 1.0, 0.3), 1000, axis=0)
    elif name == "planar":
        xy = r.uniform(-1, 0.9, (2000, 2)); s = r.uniform(0.01, 0.1, 2000)
        t = np.zeros((2000, 3, 3), np.float64)
        t[:, :, :2] = xy[:, None, :]; t[:, 1, 0] += s; t[:, 2, 1] += s
        t = t.astype(np.float32)
        assert not t[:, :, 2].any()
    elif name == "line":
        x = r.uniform(-1, 0.9, 500); s = 0.05
        t = np.zeros((500, 3, 3), np.float64)
        t[:, 0] = np.stack([x, np.full(500, -s), np.full(500, -s)], 1)
        t[:, 1] = np.stack([x + s, np.full(500, s), np.full(500, s)], 1)
        t[:, 2] = np.stack([x, np.full(500, s), np.full(500, -s)], 1)
        t = t.astype(np.float32)
    elif name == "geometric":
        c = np.repeat((2.0 ** -np.arange(24))[:, None] * np.ones(3), 40, axis=0) + r.uniform(-1e-9, 1e-9, (960, 3))
        off = np.array([[0, 0, 0], [1e-5, 0, 0], [0, 1e-5, 1e-5]])
        t = (c[:, None, :] + off[None]).astype(np.float32)
    elif name == "signed":
        span = np.array([1e30, 1e-30, 1.0])
        c = r.uniform(-1, 1, (2000, 3)) * span * 0.9
        t = (c[:, None, :] + r.uniform(-1, 1, (2000, 3, 3)) * span * 0.01).astype(np.float32)
        t[::50, 0] = np.float32(0.0); t[25::50, 1] = np.float32(-0.0)
        t[10::50, 2, 1] = np.float32(-0.0); t[10::50, 2, 2] = np.float32(0.0)
        assert np.signbit(t[25, 1]).all() and not np.signbit(t[0, 0]).any()
    elif name == "big_small":
        big = np.array([[[-1, -1, -1], [1, 1, 1], [1, -1, 1]]], np.float32)
        t = np.concatenate([big, _uniform(r, 3000, 1.0, 0.005)])
    elif name == "u20k":
        t = _uniform(r, 20000, 5.0, 0.05)
    elif name == "u150k":
        t = _uniform(r, 150000, 5.0, 0.02)
    else:
        raise KeyError(name)
    t = np.ascontiguousarray(t, np.float32)
    rank = r.permutation(len(t)).astype(np.uint32)
    t.setflags(write=False); rank.setflags(write=False)
    return Soup(name, t, rank, extra)


_soups = {}


def soup(name) -> Soup:
    if name not in _soups:
        _soups[name] = _make(name)
    return _soups[name]


def scene_desc(name):
    """the soup as a scene of one diffuse object (terra_amd.scenes.SceneDesc): what the traversal comparison commits"""
    from terra_amd import scenes
    s = soup(name)
    n = len(s.tris)
    normals = np.zeros((n, 3, 3), np.float32); normals[:, :, 1] = 1.0
    return scenes.SceneDesc(objects=[scenes.ObjectDesc(s.tris, normals, np.zeros((n, 3, 2), np.float32), name=name)], width=8, height=8, spp=1, bounces=1, name=name)


# ---- rays for the traversal comparison -------------------------------------------------------------------------------------------------------------------
N_AIMED, N_AXIAL = 768, 256


def rays(name):
    """1,024 rays (origins, directions; float32, contiguous) for a soup's committed scene: 768 from outside the bounds towards the centroids of random triangles,
    256 with one or two zero direction components, through centroids as well. A ray through a centroid hits that triangle or a nearer one unless it runs
    edge-on, so well over half of them hit; tests/test_fast_tree.py asserts that share with the oracle's reference traversal before the device is asked."""
    s = soup(name)
    r = np.random.default_rng([0x4a7, NAMES.index(name)])
    t = s.tris.astype(np.float64)
    lo = t.reshape(-1, 3).min(0); hi = t.reshape(-1, 3).max(0)
    reach = None
    n = N_AIMED + N_AXIAL
    target = t[r.integers(0, len(t), n)].mean(axis=1)
    d = r.normal(size=(n, 3))
    # the last 256: one zero component (even) or two (odd); the component that stays is drawn per ray
    ax = r.integers(0, 3, N_AXIAL); ax2 = (ax + 1 + r.integers(0, 2, N_AXIAL)) % 3
    if name == "planar":          # the triangles lie in z = 0: a ray inside that plane runs edge-on to all of them, so z is never the zero component
        ax = ax % 2; ax2 = 1 - ax
    if name == "signed":
        # In float32 this soup is planar too: a vertex's y (1e-30) vanishes beside any origin that is not itself within 1e-30 of the plane, and a ray that leaves
        # the bounds along x (1e30) multiplies two such numbers in its edge functions and overflows. So its rays cross the plane y = 0 steeply, from one unit
        # outside the bounds in y; their x and z components are small but not zero, and the zero components of the last 256 are x or z, never y.
        d *= np.array([1e-3, 1.0, 1e-3]); reach = 1.0
        ax = np.where(ax == 1, 0, ax); ax2 = 2 - ax
    tail = d[N_AIMED:]
    tail[np.arange(N_AXIAL), ax] = 0.0
    odd = np.arange(N_AXIAL) % 2 == 1
    tail[odd, ax2[odd]] = 0.0
    d /= np.linalg.norm(d, axis=1)[:, None]
    if reach is None:
        # back along the ray to where it leaves the bounds, and a little further: the origins stay within about one box of the soup (the containment argument
        # of scene_host.cpp bounds the origin's distance as it bounds the vertices')
        with np.errstate(divide="ignore", invalid="ignore"):
            t_exit = np.where(d > 0, (target - lo) / d, np.where(d < 0, (target - hi) / d, np.inf)).min(axis=1)
        reach = (1.05 * t_exit + 0.05 * np.linalg.norm(hi - lo))[:, None]
    o = target - d * reach
    assert ((d[N_AIMED:] == 0).sum(axis=1) >= 1).all() and ((d[N_AIMED:] == 0).sum(axis=1) <= 2).all()
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
