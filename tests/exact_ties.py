"""Scenes in which different triangles lie at depths that are equal bit for bit, and the CPU model of what a closest hit must answer there (shared by
tests/test_exact_ties.py and tests/test_exact_ties_gpu.py; no fixtures).

The reference keeps the first triangle it meets among equal depths (a strict "<"), which is the triangle of the lowest leaf visit rank. The device paths that meet
triangles in another order restate that as the lexicographic minimum of (depth, rank): the pair form's leaf loop (csrc/traverse_ref.h traverse_pairs), the fast
tree (csrc/traverse_fast.h) and the ray queries on both. Exactly duplicated triangles cannot tell that record from "the first trip wins": the commit gives the
lower-ranked copy to the earlier entry. Different triangles at one depth can.

The plane. Rays run along +z from z = -4 with x and y on a dyadic lattice. A render door pushes the origin to o' = fl(-4 + fl(0.001)) and every vertex lies at
z = fl(4 + o'), so A_z - o'_z is exactly 4: the shear is 0, every edge function is an exact product of small dyadics, T = 4 det and the watertight depth is 4.0 on
every hit (asserted on the oracle, tests/test_exact_ties.py). The ray queries push nothing: they start at o'.

The quads are axis-aligned rectangles in that plane that overlap at random, and every triangle has an emission of its own (and, for the AOV case, an albedo of
its own; otherwise albedo 0), so under the Simple integrator without bounces a pixel names the triangle that won. In the 80-triangle scene every triangle is an
object of its own with constant colours. The 32-triangle scenes cannot be built that way: 32 materials and 32 lights take 6 KB of a block's LDS, the scene is then
not LDS-resident, the commit gives it the fast tree and no launch ever has the pair form (tests/test_exact_ties.py asserts both halves of this). There the 32
triangles are ONE object whose emission and albedo are point-sampled rows of texels, one texel per triangle, every vertex of a triangle on the middle of its texel:
the same per-triangle colours, one material, one light, LDS-resident. The ray queries name the triangle by its index in that object.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from terra_amd import api, runtime, scenes
from test_leaf_rank import _ranks

Z_ORIGIN = np.float32(-4.0)
PUSH = np.float32(0.001)                                      # scene_raycast's origin offset along a direction of (0, 0, 1)
Z_PUSHED = np.float32(Z_ORIGIN + PUSH)                        # o'
Z_PLANE = np.float32(np.float32(4.0) + Z_PUSHED)
DEPTH = np.float32(4.0)
assert float(Z_PUSHED) == -3.999000072479248 and float(Z_PLANE) == 0.0009999275207519531 and np.float32(Z_PLANE - Z_PUSHED) == DEPTH

# the scenes in use (tests/test_exact_ties.py holds each to its conditions): reversing the triangles changes the ranks -- seed 0 reversed keeps 11 discriminating rays
# and seed 5 reversed 59 -- so the reversed scene has a seed of its own
PAIR_SCENES = {"seed-0": dict(n_quads=16, seed=0, one_object=True), "seed-5": dict(n_quads=16, seed=5, one_object=True),
               "seed-8-reversed": dict(n_quads=16, seed=8, order="reversed", one_object=True)}
BIG_SCENE = dict(n_quads=40, seed=0)
SCENES = dict(PAIR_SCENES, big=BIG_SCENE)

FRAME_W, FRAME_H = 64, 34                                     # 2,176 pixels: the 2,113 rays, then zero-direction (inactive) records
ORDERS = ("given", "reversed")


def emission_of(t: int):
    """the emission of generated triangle t: distinct for t < 128, every component and every sum of four of them exact in float32"""
    return (float(t + 1), float((7 * t) % 32 + 1), (t % 5 + 1) / 4.0)


def albedo_of(t: int):
    return ((t % 8 + 1) / 16.0, ((3 * t) % 16 + 1) / 32.0, (t // 8 + 1) / 16.0)


def _texel_uv(t: int) -> np.ndarray:
    """texcoords (texel units) that put all three vertices of a triangle on the middle of texel t of a row of texels"""
    uv = np.zeros((1, 3, 2), np.float32); uv[..., 0] = t + 0.5; uv[..., 1] = 0.5
    return uv


def quad_scene(n_quads: int, seed: int, order: str = "given", albedo: bool = False, spp: int = 1, one_object: bool = False) -> scenes.SceneDesc:
    """n_quads random rectangles on the lattice of quarters inside [-2, 2]^2 at z = Z_PLANE, their 2 n_quads triangles in the order generated or reversed.
    one_object False: every triangle an object of its own, with a constant emission (and albedo) of its own.
    one_object True: one object whose emission (and albedo) is a point-sampled row of texels, one texel per triangle -- the same per-triangle colours from one
    material and one light, which is what lets a 32-triangle scene stay LDS-resident (module docstring)."""
    assert order in ORDERS
    r = np.random.default_rng(seed)
    z = float(Z_PLANE)
    parts = []                                                  # (generated index, triangle, normals)
    for q in range(n_quads):
        x0, y0 = r.integers(-8, 5, 2) / 4
        w, h = r.integers(2, 9, 2) / 4
        x1, y1 = min(x0 + w, 2), min(y0 + h, 2)
        tris, nrm = scenes._quad((x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z), (0, 0, -1))
        assert np.all(tris[..., 2] == Z_PLANE)
        parts += [(2 * q + k, tris[k:k + 1].copy(), nrm[k:k + 1].copy()) for k in range(2)]
    if order == "reversed":
        parts = parts[::-1]
    black = (0.0, 0.0, 0.0)
    if one_object:
        n = len(parts)
        row = lambda f: scenes.TextureDesc(np.array([[f(t) for t in range(n)]], np.float32), 0, 2)          # (1, n, 3) float texels, point filter, clamp
        m = scenes.Material(albedo=black, emissive_texture=row(emission_of), albedo_texture=row(albedo_of) if albedo else None)
        objs = [scenes.ObjectDesc(np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([_texel_uv(p[0]) for p in parts]), m, "quads")]
    else:
        objs = [scenes.ObjectDesc(tri, nrm, np.zeros((1, 3, 2), np.float32), scenes.Material(albedo=albedo_of(t) if albedo else black, emissive=emission_of(t)), "t%d" % t)
                for t, tri, nrm in parts]
    d = scenes.SceneDesc(objects=objs, width=FRAME_W, height=FRAME_H, spp=spp, bounces=0, integrator=api.kTerraIntegratorSimple, jitter=0.0, name="exact-ties")
    d.generated = np.array([p[0] for p in parts], np.int64)      # soup triangle k -> the generated triangle it is (emission_of / albedo_of go by that)
    return d


def scene(name: str, **kw) -> scenes.SceneDesc:
    return quad_scene(**dict(SCENES[name], **kw))


def prim_of(d: scenes.SceneDesc) -> np.ndarray:
    """soup triangle k -> its reference primitive word, object | triangle in the object << 8"""
    return np.concatenate([np.full(len(ob.triangles), j, np.int64) | (np.arange(len(ob.triangles), dtype=np.int64) << 8) for j, ob in enumerate(d.objects)])


def ray_xy() -> np.ndarray:
    """(2113, 2): 32 x 32 odd multiples of 1/16 in [-2, 2] (quad interiors), then 33 x 33 multiples of 1/8 (rims, corners and diagonals: edge functions that are 0)"""
    a = (2 * np.arange(32) + 1) / 16.0 - 2.0
    b = np.arange(33) / 8.0 - 2.0
    grids = [np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(-1, 2) for g in (a, b)]
    xy = np.concatenate(grids).astype(np.float32)
    assert len(xy) == 2113 and np.abs(xy).max() == 2.0
    return xy


def rays(z) -> tuple:
    """(origins, directions) of the 2,113 rays from height z, contiguous float32"""
    xy = ray_xy()
    o = np.zeros((len(xy), 3), np.float32); o[:, :2] = xy; o[:, 2] = np.float32(z)
    d = np.zeros((len(xy), 3), np.float32); d[:, 2] = 1.0
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def ray_frame() -> np.ndarray:
    """[FRAME_H, FRAME_W, 8] api.RAY_DTYPE words for a render door: ray i from z = -4 at pixel (i % FRAME_W, i // FRAME_W), the rest of the frame inactive"""
    o, d = rays(Z_ORIGIN)
    f = np.zeros((FRAME_W * FRAME_H, 8), np.float32)
    f[:len(o), 0:3] = o; f[:len(o), 3] = np.inf; f[:len(o), 4:7] = d
    return f.reshape(FRAME_H, FRAME_W, 8)


def soup(d: scenes.SceneDesc) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([np.asarray(ob.triangles, np.float32).reshape(-1, 9) for ob in d.objects]))


def depth_matrix(orc, o, d, tris) -> np.ndarray:
    """orc_watertight of every ray on every triangle: (rays, triangles) float32 depths, +inf where the test rejects"""
    f = orc.fn("orc_watertight", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    out = np.zeros(8, np.float32)
    D = np.full((len(o), len(tris)), np.inf, np.float32)
    po, pd, pt, pout = o.ctypes.data, d.ctypes.data, tris.ctypes.data, out.ctypes.data
    for i in range(len(o)):
        for j in range(len(tris)):
            if f(po + 12 * i, pd + 12 * i, pt + 36 * j, pout):
                D[i, j] = out[3]
    return D


def committed(L, d: scenes.SceneDesc) -> dict:
    """the library's commit-time tables of the scene (no device needed): leaf visit ranks and the pair form"""
    scene = scenes.build_scene(L, d)
    n = d.triangle_count
    out = dict(ranks=_ranks(L, scene, n).astype(np.int64))
    out["pairs"], out["masks"] = runtime.scene_leaf_pairs(L, scene)
    L.scene_destroy(scene)
    return out


def argmin_depth_rank(D, ranks):
    """(hit, triangle): per ray the lexicographic minimum of (depth, rank) over the triangles the watertight test accepts"""
    depth = D.min(axis=1)
    hit = np.isfinite(depth)
    tri = np.where(np.isfinite(D) & (D == depth[:, None]), ranks[None, :], 1 << 40).argmin(axis=1)
    return hit, np.where(hit, tri, -1)


def first_trip_wins(D, pairs):
    """per ray the answer of a leaf loop that walks the entries in table order, T1 before T2, and keeps a record by the strict "<" alone (-1: no hit)"""
    best = np.full(len(D), np.inf, np.float32)
    tri = np.full(len(D), -1, np.int64)
    for p in pairs:
        for t in p["tri"]:
            closer = D[:, int(t)] < best
            best = np.where(closer, D[:, int(t)], best); tri = np.where(closer, int(t), tri)
    return tri


def second_beats_first(D, ranks, pairs) -> int:
    """rays on which both triangles of one entry tie for nearest and T2 has the lower rank (reported; the commit's pairing seems never to produce it)"""
    depth = D.min(axis=1)
    n = np.zeros(len(D), bool)
    for p in pairs:
        t1, t2 = (int(t) for t in p["tri"])
        if ranks[t2] < ranks[t1]:
            n |= np.isfinite(depth) & (D[:, t1] == depth) & (D[:, t2] == depth)
    return int(n.sum())


def model(orc, L, d: scenes.SceneDesc) -> dict:
    """everything the tests hold a door against, from the oracle's watertight test at o' and the commit tables alone"""
    o, dirs = rays(Z_PUSHED)
    D = depth_matrix(orc, o, dirs, soup(d))
    c = committed(L, d)
    hit, expected = argmin_depth_rank(D, c["ranks"])
    nearest = D.min(axis=1)
    ties = hit & ((D == nearest[:, None]).sum(axis=1) >= 2)
    m = dict(D=D, hit=hit, expected=expected, ties=ties, max_tied=int((D == nearest[:, None])[hit].sum(axis=1).max()), generated=d.generated, prim=prim_of(d), **c)
    if len(c["pairs"]):
        m["first_trip"] = first_trip_wins(D, c["pairs"])
        m["discriminating"] = hit & (m["first_trip"] != expected)
        m["second_beats_first"] = second_beats_first(D, c["ranks"], c["pairs"])
    return m


_models = {}


def model_of(H, L, name: str) -> dict:
    """model() of a scene in use, computed once per process"""
    if name not in _models:
        _models[name] = model(H.lib("orc"), L, scene(name))
    return _models[name]


def device_unit(H, lib):
    """harness.Unit("amd") over `lib` itself, so that a scene handle never crosses from the library under test (runtime.load(), which TERRA_AMD_LIB can point at an
    experiment build) into the tree's own copy"""
    u = H.Unit.__new__(H.Unit)
    u.kind, u.L, u.p = "amd", lib, "terra_amd_unit_"
    return u


def oracle_scene(H, d):
    u = H.Unit("orc")
    return u, scenes.build_scene(u.L, d)


def oracle_traverse(H, d):
    """(found, prim, point) of the oracle's reference traversal from o' -- what a ray query must answer"""
    u, sc = oracle_scene(H, d)
    try:
        return u.bvh_traverse(sc, *rays(Z_PUSHED))
    finally:
        u.L.scene_destroy(sc)


def oracle_raycast(H, d):
    """(object, triangle, point, surface) of the oracle's raycast from z = -4, which pushes the origin to o' itself (device arithmetic)"""
    H.set_oracle_math(1)
    try:
        u, sc = oracle_scene(H, d)
        try:
            return u.raycast(sc, *rays(Z_ORIGIN))
        finally:
            u.L.scene_destroy(sc)
    finally:
        H.set_oracle_math(0)


def oracle_sums(H, d, passes: int) -> list:
    """float32 running sums of orc_trace_one along the frame's active rays over samples 0 .. passes-1, keyed (frame seed, pixel, sample): what `results.acc`
    holds after so many samples (the pattern of tests/test_ray_source_gpu.py oracle_sums)"""
    o, dirs = rays(Z_ORIGIN)
    n = len(o)
    H.set_oracle_math(1)
    try:
        u, sc = oracle_scene(H, d)
        key = u.L.fn("orc_pixel_stream_key", None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
        acc = np.zeros((n, 3), np.float32); sums = []
        for s in range(passes):
            k3 = np.zeros((n, 3), np.uint64)
            for i in range(n):
                key(scenes.FRAME_SEED, i, s, k3[i].ctypes.data)
            rad, _ = u.trace(sc, o, dirs, np.ascontiguousarray(k3[:, 1]), np.ascontiguousarray(k3[:, 2]))
            acc = (acc + rad).astype(np.float32)
            sums.append(acc.copy())
        u.L.scene_destroy(sc)
        return sums
    finally:
        H.set_oracle_math(0)


def image_of(tri, generated, samples: int = 1) -> np.ndarray:
    """the `acc` a door would leave if triangle tri[i] (scene order, -1 none) won ray i: samples x its emission"""
    e = np.array([emission_of(int(g)) for g in generated] + [(0.0, 0.0, 0.0)], np.float32)
    return (e[tri] * np.float32(samples)).astype(np.float32)
