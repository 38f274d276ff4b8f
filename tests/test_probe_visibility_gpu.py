"""Probe visibility on the GPU (include/terra_amd.h "Probe visibility"): terra_amd_probe_visibility* and terra_amd_sh_irradiance_visible* against the numpy
restatement of the header's rules (tests/probe_visibility_ref.py), bit for bit; open space against the plain lookup; the leak through a wall, on analytic distances
and rendered; then the chain runtime.bake_probe_visibility runs and the headless tool's --probe-visibility against the runtime."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import probe_ref
import probe_visibility_ref as ref
from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
FLT_MAX = np.finfo(F).max


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(a):
    """a structured array as float32 words, one row per record"""
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view(F).reshape(len(a), -1)


def points_of(positions, normals):
    p = np.zeros(len(positions), api.POINT_DTYPE)
    p["position"], p["normal"] = positions, normals
    return p


# ---- projection on synthetic hits and rays --------------------------------------------------------------------------------------------------------------------
def synthetic(P, K, m, cap, seed):
    """hits and rays [P, K]: directions of any length, some exactly on texel centres and on the octahedron's edges and corners (z = 0, x = 0, -z), distances on both
    sides of the cap, misses, t = 0, t = NaN, and every kind of inactive ray"""
    r = np.random.default_rng(seed)
    rays = np.zeros((P, K), api.RAY_DTYPE)
    rays["origin"] = r.uniform(-1, 1, (P, K, 3))
    rays["tmax"] = FLT_MAX
    d = r.normal(0, 1, (P, K, 3))
    rays["direction"] = d / np.linalg.norm(d, axis=-1, keepdims=True) * r.choice([1.0, 1.0, 0.25, 1.1], (P, K, 1))          # (no longer: 1.1^256 is still a binary32)
    hits = np.zeros((P, K), api.HIT_DTYPE)
    hits["t"] = r.uniform(0, 1.5 * cap, (P, K))
    hits["object"] = r.integers(0, 5, (P, K))
    hits["triangle"] = r.integers(0, 9, (P, K))
    flat_h, flat_r = hits.reshape(-1), rays.reshape(-1)
    n = P * K
    centres = ref.texel_directions(m).astype(F)
    edges = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [-0.28, 0.96, 0], [0, 0.6, 0.8], [0, -0.8, -0.6], [0.5, -0.5, 0],
                      [-0.0, 0.0, -1.125], [0, 0.3, -0.7], [0.25, 0, -0.75], [1e-30, -1e-30, -1], [-1e-30, -1e-30, -1]], F)
    special = np.concatenate([centres, centres * F(1.25), edges])
    kind = r.integers(0, 30, n)
    pick = kind >= 22          # about a quarter of the cells look along a special direction
    flat_r["direction"][pick] = special[r.integers(0, len(special), pick.sum())]
    flat_h["object"][kind == 0] = -1
    flat_h["t"][kind == 0] = FLT_MAX
    flat_h["object"][kind == 1] = -1          # (a miss whatever t says)
    flat_h["t"][kind == 2] = 0
    flat_h["t"][kind == 3] = NAN
    flat_h["t"][kind == 4] = INF
    flat_h["t"][kind == 5] = F(cap)
    flat_h["t"][kind == 6] = np.nextafter(F(cap), F(INF))
    flat_r["direction"][kind == 7] = 0
    flat_r["direction"][kind == 8, 1] = NAN
    flat_r["direction"][kind == 9, 0] = -INF
    flat_r["origin"][kind == 10, 2] = INF
    flat_r["origin"][kind == 11, 0] = NAN
    return hits, rays


def project_device(L, hits, rays, n, options, vis_map=None):
    import torch
    out = runtime.probe_visibility(L, to_device(words(hits)), to_device(words(rays)), n, options, vis_map)
    torch.cuda.synchronize()
    return out


def same_map(H, got, want):
    return H.same_bits(got["weight"], want["weight"]) and H.same_bits(got["distance"], want["distance"]) and H.same_bits(got["distance2"], want["distance2"]) and \
        np.array_equal(got["cells"], want["cells"])


@pytest.mark.parametrize("n,P,m,s", [(1, 1, 1, 0), (2, 3, 2, 1), (8, 5, 3, 6), (9, 3, 8, 8), (16, 5, 16, 6), (64, 1, 8, 6), (8, 257, 8, 1), (16, 3, 16, 8), (2, 5, 16, 0), (9, 1, 1, 6)])
def test_projection_against_the_restatement(H, L, n, P, m, s):
    K, cap = n * n, 2.5
    options = runtime.probe_visibility_options(texels=m, sharpness=s, max_distance=cap, bias=7.0, backface=True)          # (the projection looks at neither of the last two)
    sh, want = None, None
    for batch in range(3):          # accumulate 0, then 1, then 1 again
        hits, rays = synthetic(P, K, m, cap, 1000 * n + 10 * P + batch)
        want = ref.project(hits, rays, n, m, s, cap, want)
        sh = project_device(L, hits, rays, n, options, sh)
        got = runtime.visibility_map_host(sh)
        assert got.shape == (P, m * m) and same_map(H, got, want), batch
        if batch == 0:
            on = ref.takes_part(rays)
            assert (want["cells"] <= on.sum(-1)[:, None]).all() and np.isfinite(want["distance2"]).all()
            if K >= 64:
                assert (want["cells"] > 0).all() and (on.sum(-1) < K).any()
            if (n, P) in ((2, 3), (16, 5), (9, 1)):          # the host form
                host = np.zeros((P, m * m), api.VISIBILITY_TEXEL_DTYPE)
                assert L.probe_visibility(hits.ctypes.data, rays.ctypes.data, P, n, C.byref(options), 0, host.ctypes.data) == 0, runtime.last_error()
                assert host.tobytes() == got.tobytes()
                assert L.probe_visibility(hits.ctypes.data, rays.ctypes.data, P, n, C.byref(options), 1, host.ctypes.data) == 0, runtime.last_error()
                assert same_map(H, host, ref.project(hits, rays, n, m, s, cap, want))


# ---- the lookup -----------------------------------------------------------------------------------------------------------------------------------------------
def random_sh(P, seed):
    sh = np.zeros(P, api.PROBE_SH_DTYPE)
    sh["c"] = np.random.default_rng(seed).normal(0, 1, (P, 9, 3))
    sh["cells"] = 256
    return sh


def random_map(P, m, scale, seed):
    """sums of a random weight with means around `scale` and some variance; one texel in seven has no weight at all"""
    r = np.random.default_rng(seed)
    vm = np.zeros((P, m * m), api.VISIBILITY_TEXEL_DTYPE)
    w = r.uniform(0.5, 40, (P, m * m))
    mean = r.uniform(0.2, 1.5, (P, m * m)) * scale
    var = r.uniform(0, 0.05, (P, m * m)) * scale * scale
    vm["weight"], vm["distance"], vm["distance2"], vm["cells"] = w, w * mean, w * (mean * mean + var), r.integers(1, 200, (P, m * m))
    empty = r.integers(0, 7, (P, m * m)) == 0
    for f in ("weight", "distance", "distance2", "cells"):
        vm[f][empty] = 0
    return vm


def constant_map(P, m, weight, mean):
    vm = np.zeros((P, m * m), api.VISIBILITY_TEXEL_DTYPE)
    vm["weight"], vm["distance"], vm["distance2"], vm["cells"] = weight, weight * mean, weight * mean * mean, 1
    return vm


def visible_device(L, sh, vm, points, grid, options):
    import torch
    out = runtime.sh_irradiance_visible(L, to_device(words(sh)), to_device(words(vm)).view(len(vm), -1, 4), to_device(words(points)), grid, options)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def plain_device(L, sh, points, grid):
    import torch
    out = runtime.sh_irradiance(L, to_device(words(sh)), to_device(words(points)), grid)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def lookup_points(probes, origin, spacing, counts, seed):
    """queries on probes, along every axis and diagonal from them (so that the taps cross the map's four edges and four corners), on faces, outside every side,
    inside, at NaN and infinite positions; random normals, a zero one and non-finite ones"""
    r = np.random.default_rng(seed)
    o, s, top = np.array(origin), np.array(spacing), np.array(counts) - 1
    steps = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], D)
    near = np.concatenate([steps * 0.3, steps * 0.3 + [1e-4, -1e-4, 0], np.array([[-1e-4, -1e-4, -0.3], [1e-4, -1e-4, -0.3], [-1e-4, 1e-4, -0.3], [1e-4, 1e-4, -0.3], [1e-4, 1e-4, 0.3]])])
    around = (probes["position"].astype(D)[:, None, :] + near[None] * np.abs(s)).reshape(-1, 3)
    faces = o + s * r.integers(0, 4, (150, 3)) * np.where(r.integers(0, 2, (150, 3)) > 0, 1.0, r.uniform(0, 1, (150, 3)))
    outside = o + s * (r.uniform(-2, 2, (200, 3)) * (top + 1) + np.where(r.integers(0, 2, (200, 3)) > 0, 4.0 * (top + 1), 0.0))
    inside = o + s * r.uniform(0, 1, (400, 3)) * np.maximum(top, 0.5)
    special = np.array([[NAN, 0, 0], [0, NAN, 0], [0, 0, NAN], [INF, 0, 0], [-INF, INF, 0], [0, 0, -INF]])
    positions = np.concatenate([probes["position"], around, faces, outside, inside, special]).astype(F)
    normals = r.normal(0, 1, (len(positions), 3)).astype(F)
    normals[len(probes):len(probes) + 26] = steps          # along the offsets themselves: the back-face term at both ends
    normals[-7] = 0
    normals[-8] = (NAN, 0, 1)
    normals[-9] = (0, INF, 1)
    return points_of(positions, normals)


@pytest.mark.parametrize("counts,origin,spacing", [((3, 2, 2), (-1.0, 0.5, 2.0), (0.75, 1.5, 0.3)), ((1, 1, 1), (0.1, 0.2, 0.3), (1.0, 2.0, 3.0)), ((4, 1, 3), (0.0, 1.0, -1.0), (0.5, 1.0, -0.7))])
def test_visible_lookup_against_the_restatement(H, L, counts, origin, spacing):
    P = counts[0] * counts[1] * counts[2]
    sh = random_sh(P, P)
    grid, probes = runtime.probe_grid(L, origin, spacing, counts)
    points = lookup_points(probes, origin, spacing, counts, sum(counts))
    g = (origin, spacing, counts)
    scale = float(np.abs(spacing).mean())
    for m, bias, flags in ((1, 0.0, 0), (1, 0.25, 1), (3, 0.0, 1), (3, 0.125, 0), (8, 0.0, 0), (8, 0.25, 1), (16, 0.0, 1)):
        vm = random_map(P, m, scale, 17 * m + flags)
        options = runtime.probe_visibility_options(texels=m, sharpness=6, max_distance=10.0, bias=bias, backface=bool(flags))
        detail = {}
        want = ref.irradiance_visible(sh, vm, points, g, m, bias, flags, detail)
        got = visible_device(L, sh, vm, points, grid, options)
        assert H.same_bits(got, want), (m, bias, flags)
        assert not got[-6:-3].view(np.uint32).any() and not got[-9:-6].view(np.uint32).any() and not got[:, 3].view(np.uint32).any()
        wv = detail["wv"][:, :-9]
        assert P * m * m == 1 or ((wv == 1).any() and ((wv > 0) & (wv < 1)).any())          # both arms of the Chebyshev test (a lone texel may be an empty one)
        if (m, flags) in ((3, 1), (8, 0)):          # the host form
            host = np.zeros((len(points), 4), F)
            assert L.sh_irradiance_visible(words(sh).ctypes.data, vm.ctypes.data, P, C.byref(grid), C.byref(options), points.ctypes.data, len(points), host.ctypes.data) == 0, runtime.last_error()
            assert H.same_bits(host, got)
    # the taps of these queries reach over every edge and corner of a map (the header's encode for m = 3, from the first probe)
    V = points["position"][P:P + 57].astype(D) - probes["position"][0].astype(D)
    a = np.abs(V).sum(-1)
    px, py = V[:, 0] / a, V[:, 1] / a
    fold = V[:, 2] < 0
    px, py = np.where(fold, (1 - np.abs(py)) * ref.sgn(px), px), np.where(fold, (1 - np.abs(px)) * ref.sgn(py), py)
    i0, j0 = np.floor((px * 0.5 + 0.5) * 3 - 0.5).astype(int), np.floor((py * 0.5 + 0.5) * 3 - 0.5).astype(int)
    crossed = {(int(i), int(j)) for i, j in zip(i0, j0)}
    assert {(-1, -1), (2, 2), (-1, 2), (2, -1)} <= crossed and any(i == -1 and 0 <= j < 2 for i, j in crossed) and any(j == 2 and 0 <= i < 2 for i, j in crossed)


@pytest.mark.parametrize("counts,origin,spacing", [((3, 2, 2), (-1.0, 0.5, 2.0), (0.75, 1.5, 0.3)), ((4, 1, 3), (0.0, 1.0, -1.0), (0.5, 1.0, -0.7))])
def test_hidden_and_open_maps(H, L, counts, origin, spacing):
    P = counts[0] * counts[1] * counts[2]
    sh = random_sh(P, 3 * P)
    grid, probes = runtime.probe_grid(L, origin, spacing, counts)
    points = lookup_points(probes, origin, spacing, counts, 5)
    plain = plain_device(L, sh, points, grid)
    # every probe hidden: mean 0 and variance 0 make every Chebyshev term exactly 0 away from the probes, S is 0, and the answer is the plain lookup's, bit for bit
    away = points[~(points["position"][:, None, :] == probes["position"][None]).all(-1).any(-1)]
    plain_away = plain_device(L, sh, away, grid)
    for m in (1, 8):
        options = runtime.probe_visibility_options(texels=m, max_distance=10.0, backface=True)
        hidden = visible_device(L, sh, constant_map(P, m, 1.0, 0.0), away, grid, options)
        detail = {}
        want = ref.irradiance_visible(sh, constant_map(P, m, 1.0, 0.0), away, (origin, spacing, counts), m, 0.0, 1, detail)
        assert H.same_bits(hidden, want) and H.same_bits(hidden, plain_away)
        finite = np.isfinite(away["position"]).all(-1) & np.isfinite(away["normal"]).all(-1)          # (a query that is answered at all)
        assert (detail["S"][finite] == 0).all() and finite.sum() > 800
    # open space: every mean is max_distance, further than any query: within 1 binary32 ulp of the plain lookup (the weights sum to 1 up to binary64 rounding)
    for m in (1, 16):
        options = runtime.probe_visibility_options(texels=m, max_distance=64.0)
        vm = constant_map(P, m, 3.0, 64.0)
        near = points[np.isfinite(points["position"]).all(-1) & (np.abs(points["position"]).max(-1) < 30)]
        got = visible_device(L, sh, vm, near, grid, options)
        assert H.same_bits(got, ref.irradiance_visible(sh, vm, near, (origin, spacing, counts), m))
        base = plain_device(L, sh, near, grid)
        assert (np.abs(got - base) <= np.spacing(np.maximum(np.abs(got), np.abs(base)))).all() and np.abs(base[:, :3]).max() > 0.1


# ---- the leak through a wall ----------------------------------------------------------------------------------------------------------------------------------
LEAK_GRID = ((-0.5, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 1))          # probe 0 in room A (-1 <= x <= 0), probe 1 in room B (0 <= x <= 1); |y|, |z| <= 1
LEAK_CAP = 4.0


def centre_rays(P_positions, n):
    """the cell-centre rays terra_amd_probe_rays lays about the pole +z, analytically (tests/test_probe_gpu.py pins that form to 1e-6): for the CPU-only check"""
    c = np.arange(n * n)
    i, j = c % n, c // n
    z = 1 - 2 * (i + 0.5) / n
    phi = 2 * math.pi * (j + 0.5) / n
    rr = np.sqrt(1 - z * z)
    rays = np.zeros((len(P_positions), n * n), api.RAY_DTYPE)
    rays["direction"] = np.stack([rr * np.cos(phi), rr * np.sin(phi), z], axis=1)[None]
    rays["origin"] = np.asarray(P_positions, F)[:, None, :]
    rays["tmax"] = FLT_MAX
    return rays


def box_distances(rays, lo, hi):
    """the distance from each ray's origin (inside the box) to the box lo .. hi, in float64; lo, hi: [P, 3]"""
    o, d = rays["origin"].astype(D), rays["direction"].astype(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (np.asarray(hi, D)[:, None, :] - o) / d, np.where(d < 0, (np.asarray(lo, D)[:, None, :] - o) / d, INF))
    return t.min(-1)


def room_hits(rays, wall, half=0.0):
    """the hit records of the two probes' rays in their rooms; wall: the wall stands, `half` its half thickness about the plane x = 0"""
    lo = [[-1, -1, -1], [half, -1, -1]] if wall else [[-1, -1, -1], [-1, -1, -1]]
    hi = [[-half, 1, 1], [1, 1, 1]] if wall else [[1, 1, 1], [1, 1, 1]]
    hits = np.zeros(rays.shape, api.HIT_DTYPE)
    hits["t"] = box_distances(rays, lo, hi)
    return hits


def leak_queries():
    return points_of([[x, 0, 0] for x in (0.05, 0.25, 0.45) for _ in range(3)], [[1, 0, 0], [-1, 0, 0], [0, 1, 0]] * 3)


def leak_sh(lit=1.0):
    sh = np.zeros(2, api.PROBE_SH_DTYPE)
    sh["c"][0, 0] = lit          # probe 0 (room A) carries c0 = 1, probe 1 (room B) nothing
    return sh


def leak_conditions(visible, visible_open, plain):
    """the issue's three conditions on the queries in the dark room"""
    assert (plain[:, :3] > 0).all()
    assert (visible[:, :3] <= 0.01 * plain[:, :3]).all(), (visible[:, :3] / plain[:, :3]).max()
    assert (visible_open[:, :3] >= 0.5 * plain[:, :3]).all(), (visible_open[:, :3] / plain[:, :3]).min()


def leak_on_the_restatement(rays):
    """(visible, visible with the wall removed, plain) from the numpy restatement alone"""
    out = []
    for wall in (True, False):
        vm = ref.project(room_hits(rays, wall), rays, 16, 8, 6, LEAK_CAP)
        out.append(ref.irradiance_visible(leak_sh(), vm, leak_queries(), LEAK_GRID, 8))
    return out[0], out[1], probe_ref.irradiance(leak_sh(), leak_queries(), grid=LEAK_GRID)


def test_the_leak_on_analytic_distances(H, L):
    """Two probes either side of a wall in the plane x = 0, the lit one carrying c0 = 1: in the dark room the visible lookup gives at most 0.01 of the plain one's
    leak, and at least half of it once the wall is taken out of the distances. The numpy restatement alone gives, on the analytic centre rays, visible / plain of
    at most 6.3e-5 with the wall (2.5e-5 against a plain 0.399 at x = 0.05) and exactly 1 without."""
    grid, probes = runtime.probe_grid(L, *LEAK_GRID)
    assert np.array_equal(probes["position"], np.array([[-0.5, 0, 0], [0.5, 0, 0]], F))
    d_rays = runtime.probe_rays(L, to_device(words(probes)), 16)
    rays = d_rays.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 256)
    options = runtime.probe_visibility_options(texels=8, sharpness=6, max_distance=LEAK_CAP)
    queries, sh = leak_queries(), leak_sh()
    plain = plain_device(L, sh, queries, grid)
    got = []
    for wall in (True, False):
        hits = room_hits(rays, wall)
        vm = runtime.visibility_map_host(project_device(L, hits, rays, 16, options))
        want = ref.project(hits, rays, 16, 8, 6, LEAK_CAP)
        assert same_map(H, vm, want) and (vm["cells"] > 0).all()
        got.append(visible_device(L, sh, vm, queries, grid, options))
        assert H.same_bits(got[-1], ref.irradiance_visible(sh, want, queries, LEAK_GRID, 8))
    print("visible / plain with the wall:", (got[0][:, 0] / plain[:, 0]).tolist(), "without:", (got[1][:, 0] / plain[:, 0]).tolist())
    leak_conditions(got[0], got[1], plain)


WALL_HALF = 2.0 ** -10


def two_rooms(emissive=(20.0, 20.0, 20.0)):
    """a closed box -1 .. 1 on every axis, an opaque wall about the plane x = 0, and room A's ceiling (x < 0) emissive; normals into the rooms. The wall is a slab
    2^-9 thick with a face towards each room: the renderer starts a hit's shadow and bounce rays 1e-4 off the surface along its shading normal, so a wall of one
    quad, or of two faces closer together than that, is lit from behind (seen on the device: the dark probe's c0 was 8.3 with one quad, -4.4 with faces 2^-18 apart)"""
    q = scenes._quad
    e = WALL_HALF
    shell = scenes._merge([
        q((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), (0, 1, 0)),          # floor
        q((0, 1, -1), (1, 1, -1), (1, 1, 1), (0, 1, 1), (0, -1, 0)),               # room B's ceiling
        q((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1)),          # z = -1
        q((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1), (0, 0, -1)),             # z = +1
        q((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1), (1, 0, 0)),          # x = -1
        q((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1), (-1, 0, 0)),             # x = +1
    ])
    wall = scenes._merge([q((-e, -1, -1), (-e, -1, 1), (-e, 1, 1), (-e, 1, -1), (-1, 0, 0)), q((e, -1, -1), (e, -1, 1), (e, 1, 1), (e, 1, -1), (1, 0, 0))])
    light = scenes._merge([q((-1, 1, -1), (0, 1, -1), (0, 1, 1), (-1, 1, 1), (0, -1, 0))])
    objs = [scenes.ObjectDesc(*shell, scenes.Material(albedo=(0.7, 0.7, 0.7)), "shell"), scenes.ObjectDesc(*wall, scenes.Material(albedo=(0.7, 0.7, 0.7)), "wall"),
            scenes.ObjectDesc(*light, scenes.Material(albedo=(0.7, 0.7, 0.7), emissive=emissive), "light")]
    return scenes.SceneDesc(objects=objs, width=16, height=16, spp=4, bounces=3, integrator=api.kTerraIntegratorDirect, environment=(0.0, 0.0, 0.0), name="two_rooms")


def test_the_leak_rendered(H, L):
    import torch
    grid, probes = runtime.probe_grid(L, *LEAK_GRID)
    options = runtime.probe_visibility_options(texels=8, sharpness=6, max_distance=LEAK_CAP)
    dp = to_device(words(probes))
    L.clear_error()
    s = scenes.build_scene(L, two_rooms())
    try:
        sh = runtime.bake_probes(L, s, dp, cells=16)
        vm = runtime.bake_probe_visibility(L, s, dp, 16, options)
        d_rays = runtime.probe_rays(L, dp, 16)
        hits = runtime.intersect(L, s, d_rays.view(-1, 8)).cpu().numpy().view(api.HIT_DTYPE).reshape(2, 256)
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    rays = d_rays.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 256)
    analytic = room_hits(rays, True, WALL_HALF)["t"].astype(D)
    assert (hits["object"] >= 0).all() and np.abs(hits["t"].astype(D) / analytic - 1).max() <= 1e-5
    coeff = runtime.probe_sh_host(sh)
    assert not coeff["c"][1].view(np.uint32).any() and (coeff["c"][0, 0] > 0).all() and (coeff["cells"] == 256).all()          # the dark probe: exactly 0
    queries = to_device(words(leak_queries()))
    visible = runtime.sh_irradiance_visible(L, sh, vm, queries, grid, options).cpu().numpy()
    plain = runtime.sh_irradiance(L, sh, queries, grid).cpu().numpy()
    open_map = project_device(L, room_hits(rays, False), rays, 16, options)
    visible_open = runtime.sh_irradiance_visible(L, sh, open_map, queries, grid, options).cpu().numpy()
    host_sh, host_map = coeff, runtime.visibility_map_host(vm)
    assert H.same_bits(visible, ref.irradiance_visible(host_sh, host_map, leak_queries(), LEAK_GRID, 8))
    print("rendered: visible / plain with the wall:", (visible[:, 0] / plain[:, 0]).tolist(), "without:", (visible_open[:, 0] / plain[:, 0]).tolist())
    leak_conditions(visible, visible_open, plain)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------
def test_bake_probe_visibility_is_the_chain(H, L):
    import torch
    d = scenes.cornell_box(16, 16, 4, bounces=4, integrator=api.kTerraIntegratorDirect)
    probes = points_of([[-0.4, 1.0, -0.3], [0.5, 1.4, 0.2]], [[0, 0, 1], [0.2, 1.0, -0.3]])
    options = runtime.probe_visibility_options(texels=4, sharpness=3, max_distance=3.0)
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        dp = to_device(words(probes))
        got = runtime.bake_probe_visibility(L, s, dp, 8, options)
        jit = runtime.bake_probe_visibility(L, s, dp, 8, options, batches=2, jitter=5)
        with pytest.raises(runtime.TerraAmdError):
            runtime.bake_probe_visibility(L, s, dp, 8, options, batches=2)
        # by hand
        rays = runtime.probe_rays(L, dp, 8)
        hits = runtime.intersect(L, s, rays.view(-1, 8))
        hand = runtime.probe_visibility(L, hits, rays, 8, options)
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        hand_jit, frames = None, []
        for b in range(2):
            rj = runtime.probe_rays(L, dp, 8, torch.rand((64, 2), generator=gen, dtype=torch.float32, device="cuda"))
            hj = runtime.intersect(L, s, rj.view(-1, 8))
            hand_jit = runtime.probe_visibility(L, hj, rj, 8, options, map=hand_jit)
            frames.append((hj.cpu().numpy().view(api.HIT_DTYPE).reshape(2, 64), rj.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 64)))
        torch.cuda.synchronize()
        host_hits, host_rays = hits.cpu().numpy().view(api.HIT_DTYPE).reshape(2, 64), rays.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 64)
    finally:
        L.scene_destroy(s)
    assert tuple(got.shape) == (2, 16, 4) and torch.equal(got, hand) and torch.equal(jit, hand_jit) and not torch.equal(got, jit)
    want = ref.project(host_hits, host_rays, 8, 4, 3, 3.0)
    assert same_map(H, runtime.visibility_map_host(got), want) and (want["cells"] > 0).all() and (host_hits["object"] < 0).any()          # (the box is open towards -z: misses)
    want = ref.project(*frames[1], 8, 4, 3, 3.0, ref.project(*frames[0], 8, 4, 3, 3.0))
    assert same_map(H, runtime.visibility_map_host(jit), want)


def test_headless_probe_visibility_against_the_runtime(H, L, tmp_path):
    import torch
    from test_headless_tool import build_tool, read_pfm, write_obj
    d = scenes.cornell_box(8, 8, 4, bounces=4, integrator=api.kTerraIntegratorDirect, environment=(0.4, 0.52, 1.0))
    obj = tmp_path / "cornell.obj"
    write_obj(d, obj)
    exe = build_tool(H, tmp_path, "amd")
    out, maps = tmp_path / "probes.pfm", tmp_path / "maps.pfm"
    r = subprocess.run([str(exe), str(obj), str(out), "--bake-probes", "2x1x1", "--probe-cells", "4", "--probe-visibility", str(maps), "--probe-texels", "4", "--spp", "4", "--bounces", "4",
                        "--integrator", "direct", "--no-flip-z", "--normals", "file"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "probe visibility" in r.stdout
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        v = runtime.scene_vertex_points(L, s)["position"]
        lo, hi = v.min(0), v.max(0)
        grid, probes = runtime.probe_grid_over(L, lo, hi, (2, 1, 1))
        e = (hi - lo).astype(D)
        options = runtime.probe_visibility_options(texels=4, sharpness=6, max_distance=float(F(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]))))
        want = runtime.visibility_map_host(runtime.bake_probe_visibility(L, s, to_device(words(probes)), 4, options))
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    got = read_pfm(maps)
    assert got.shape == (2, 16, 3) and (want["weight"] > 0).all()
    assert H.same_bits(got[..., 0], want["weight"]) and H.same_bits(got[..., 1], want["distance"]) and H.same_bits(got[..., 2], want["distance2"])
    assert read_pfm(out).shape == (2, 9, 3)
