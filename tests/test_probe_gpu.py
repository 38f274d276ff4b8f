"""Probe harmonics on the GPU (include/terra_amd.h "Probe harmonics"): terra_amd_probe_rays* against terra_amd_unit_point_rays on host-built pairs, terra_amd_sh_project*
and terra_amd_sh_irradiance* against the numpy restatement of the header's rules (tests/probe_ref.py), all bit for bit; then the chain runtime.bake_probes runs, a sky
furnace, and the headless tool's --bake-probes against the runtime."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import probe_ref
from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
ONE_BELOW = F(1) - F(2.0 ** -24)


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
    return np.ascontiguousarray(a).view(F).reshape(len(a), -1)


def points_of(positions, normals):
    p = np.zeros(len(positions), api.POINT_DTYPE)
    p["position"], p["normal"] = positions, normals
    return p


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------------------------
def probes_of(P):
    """P = 1: one probe with the pole +z; otherwise tilted poles of any length, and probe 2 inactive (a zero normal)"""
    if P == 1:
        return points_of([[0.25, 1.0, -0.5]], [[0, 0, 1]])
    r = np.random.default_rng(7)
    p = points_of(r.uniform(-2, 2, (P, 3)), r.uniform(-1, 1, (P, 3)) * np.array([1, 3, 0.5]))
    p["normal"][2] = 0
    p["normal"][0] = (0.3, -0.2, -2.0)          # a pole in the lower half: the frame's other sign
    return p


def jitters(n):
    K = n * n
    mixed = np.full((K, 2), 0.5, F)
    mixed[::2, 0], mixed[1::2, 1], mixed[::3, 1] = 1.5, -0.25, -1.0
    some_nan = np.random.default_rng(3).uniform(0, 1, (K, 2)).astype(F)
    some_nan[::2, 0], some_nan[-1, 1] = NAN, NAN
    return {"centres": None, "zero": np.zeros((K, 2), F), "top": np.full((K, 2), ONE_BELOW, F), "clamped": mixed, "nan": some_nan,
            "random": np.random.default_rng(n).uniform(0, 1, (K, 2)).astype(F)}


def expected_rays(L, probes, n, jitter):
    """terra_amd_unit_point_rays (distribution 1) on the pairs the header's rule gives, made here in binary32; an inactive probe's records all zero"""
    K = n * n
    c = np.arange(K)
    j = np.full((K, 2), 0.5, F) if jitter is None else jitter
    with np.errstate(invalid="ignore"):
        g = np.stack([(F(1) * (c % n).astype(F) + j[:, 0]) / F(n), ((c // n).astype(F) + j[:, 1]) / F(n)], axis=1).astype(F)
        g = np.where(~(g >= 0), F(0), g)
        g = np.where(g > ONE_BELOW, ONE_BELOW, g).astype(F)
    assert g.dtype == F and (g >= 0).all() and (g <= ONE_BELOW).all()
    want = runtime.point_rays(L, runtime.point_sampling(1), np.repeat(probes, K), np.tile(g, (len(probes), 1))).reshape(len(probes), K)
    inactive = ~(np.square(probes["normal"].astype(D)).sum(-1) > 0)
    want[inactive] = np.zeros((), api.RAY_DTYPE)
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 8, 64])
def test_probe_rays_are_the_point_generator_on_stratified_pairs(H, L, n):
    import torch
    for P in (1, 5):
        probes = probes_of(P)
        d_probes = to_device(words(probes))
        for name, jitter in jitters(n).items():
            got = runtime.probe_rays(L, d_probes, n, None if jitter is None else to_device(jitter))
            torch.cuda.synchronize()
            assert tuple(got.shape) == (P, n * n, 8)
            got = got.cpu().numpy().view(api.RAY_DTYPE).reshape(P, n * n)
            want = expected_rays(L, probes, n, jitter)
            assert got.tobytes() == want.tobytes(), (P, name)
            if P == 5:
                assert not words(got[2]).view(np.uint32).any() and (got["tmax"][[0, 1, 3, 4]] == np.finfo(F).max).all()
                assert np.abs(np.square(got["direction"][[0, 1, 3, 4]].astype(D)).sum(-1) - 1).max() < 1e-6
    # the host form: the same records
    probes, jitter = probes_of(5), jitters(n)["random"]
    for j in (None, jitter):
        host = np.zeros(5 * n * n, api.RAY_DTYPE)
        assert L.probe_rays(probes.ctypes.data, 5, n, None if j is None else j.ctypes.data, host.ctypes.data) == 0, runtime.last_error()
        assert host.tobytes() == expected_rays(L, probes, n, j).tobytes()


def test_cell_centres_are_stratified_over_the_sphere(L):
    """what the map is for: with the pole +z, cell (i, j) of n x n has z = 1 - 2 (i + 0.5) / n and the azimuth 2 PI (j + 0.5) / n"""
    n = 8
    rays = runtime.probe_rays(L, to_device(words(probes_of(1))), n).cpu().numpy().view(api.RAY_DTYPE).reshape(n, n)          # [j, i]
    d = rays["direction"].astype(D)
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    assert np.abs(d[..., 2] - (1 - 2 * (i + 0.5) / n)).max() < 1e-6
    phi = 2 * math.pi * (j + 0.5) / n
    r = np.sqrt(1 - d[..., 2] ** 2)
    assert np.abs(d[..., 0] - r * np.cos(phi)).max() < 1e-6 and np.abs(d[..., 1] - r * np.sin(phi)).max() < 1e-6
    assert (rays["origin"] == probes_of(1)["position"][0]).all()


# ---- projection on synthetic frames ---------------------------------------------------------------------------------------------------------------------------
def synthetic_frame(P, K, seed):
    """results and rays [P, K]: radiance of both signs and of magnitude 1e-30 and 1e30, samples 0 and negative among the counts, directions of any length, and
    every kind of inactive ray"""
    r = np.random.default_rng(seed)
    res = np.zeros((P, K), api.RESULT_DTYPE)
    res["samples"] = r.integers(1, 9, (P, K))
    res["acc"] = (r.normal(0, 1, (P, K, 3)) * res["samples"][..., None]).astype(F)
    res["acc"] *= r.choice(np.array([1, 1, 1, 1e-30, 1e30], F), (P, K, 1))
    rays = np.zeros((P, K), api.RAY_DTYPE)
    rays["origin"] = r.uniform(-1, 1, (P, K, 3))
    rays["tmax"] = np.finfo(F).max
    rays["direction"] = r.normal(0, 1, (P, K, 3)) * r.choice([1.0, 1.0, 0.25, 3.0], (P, K, 1))
    flat_res, flat_rays = res.reshape(-1), rays.reshape(-1)
    kind = r.integers(0, 24, P * K)
    flat_res["samples"][kind == 0] = 0
    flat_res["samples"][kind == 1] = -3
    flat_rays["direction"][kind == 2] = 0
    flat_rays["direction"][kind == 3, 1] = NAN
    flat_rays["direction"][kind == 4, 0] = -INF
    flat_rays["origin"][kind == 5, 2] = INF
    flat_rays["origin"][kind == 6, 0] = NAN
    return res, rays


def project_device(L, res, rays, n, batch=0, sh=None):
    import torch
    sh = runtime.sh_project(L, to_device(words(res.reshape(-1)).view(np.int32)), to_device(words(rays.reshape(-1))), n, batch, sh)
    torch.cuda.synchronize()
    return sh


@pytest.mark.parametrize("n,P", [(1, 1), (2, 3), (3, 5), (8, 1), (9, 3), (16, 5), (64, 3), (8, 257)])
def test_projection_against_the_restatement(H, L, n, P):
    K = n * n
    res, rays = synthetic_frame(P, K, 100 * n + P)
    want = probe_ref.project(res, rays, n)
    got = runtime.probe_sh_host(project_device(L, res, rays, n))
    assert np.array_equal(got["cells"], want["cells"]) and np.array_equal(want["cells"], probe_ref.contributes(res, rays).sum(-1))
    assert H.same_bits(got["c"], want["c"])
    if K >= 64:
        assert (want["cells"] < K).any() and (want["cells"] > 0).all() and np.isfinite(want["c"]).all() and (np.abs(want["c"]) > 1e20).any()
    if (n, P) in ((3, 5), (16, 5)):          # the host form, on the framebuffer struct
        fb = api.TerraFramebuffer()
        pixels = np.zeros((P * K, 3), F)
        flat = np.ascontiguousarray(res.reshape(-1))
        fb.pixels, fb.results = C.cast(pixels.ctypes.data, type(fb.pixels)), C.cast(flat.ctypes.data, type(fb.results))
        fb.width, fb.height = K, P
        host = np.zeros(P, api.PROBE_SH_DTYPE)
        assert L.sh_project(C.byref(fb), np.ascontiguousarray(rays.reshape(-1)).ctypes.data, P, n, 0, host.ctypes.data) == 0, runtime.last_error()
        assert host.tobytes() == got.tobytes() and not pixels.any()


@pytest.mark.parametrize("n,P", [(3, 3), (16, 5)])
def test_batches_average_in_place(H, L, n, P):
    sh, want = None, None
    for batch in range(3):
        res, rays = synthetic_frame(P, n * n, 31 * n + batch)
        res["acc"] = np.where(np.abs(res["acc"]) > 1e20, F(1), res["acc"])          # (keep the batches of one magnitude: the mean is then not one batch alone)
        want = probe_ref.project(res, rays, n, batch, want)
        sh = project_device(L, res, rays, n, batch, sh)
        got = runtime.probe_sh_host(sh)
        assert H.same_bits(got["c"], want["c"]) and np.array_equal(got["cells"], want["cells"]), batch
    one = probe_ref.project(res, rays, n)
    assert not H.same_bits(one["c"], want["c"])


# ---- projection, analytic --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,gram", [(16, 1.95e-2), (64, 1.22e-3)])
def test_projection_recovers_band_limited_radiance(H, L, n, gram):
    """radiance sum_k a_k Y_k(d) along the device's own centre rays: the device equals the restatement bit for bit, and nothing more is asked of it. How far the
    restatement is from `a` is a property of the centre set -- its Gram matrix deviates from identity by at most `gram` (computed on the CPU in binary64) -- and is
    printed; it is held to 9 * gram * max |a|, the row sum of that deviation."""
    K = n * n
    rays = runtime.probe_rays(L, to_device(words(probes_of(1))), n).cpu().numpy().view(api.RAY_DTYPE).reshape(1, K)
    a = np.random.default_rng(n).uniform(-1, 1, (9, 3))
    d = rays["direction"][0].astype(D)
    Y = np.stack([y * np.ones(K) for y in probe_ref.basis(d[:, 0], d[:, 1], d[:, 2])], axis=1)          # [K, 9]
    res = np.zeros((1, K), api.RESULT_DTYPE)
    res["acc"][0], res["samples"] = (Y @ a).astype(F), 1
    want = probe_ref.project(res, rays, n)
    got = runtime.probe_sh_host(project_device(L, res, rays, n))
    assert H.same_bits(got["c"], want["c"]) and got["cells"][0] == K
    G = Y.T @ Y * (4 * math.pi / K)
    off = np.abs(want["c"][0].astype(D) - a).max()
    print(f"n = {n}: Gram deviation {np.abs(G - np.eye(9)).max():.3e}, restatement's distance from a {off:.3e}")
    assert np.abs(G - np.eye(9)).max() <= 1.01 * gram and off <= 9 * 1.01 * gram * np.abs(a).max() + 1e-6          # (the figures are quoted to three digits)


# ---- irradiance -----------------------------------------------------------------------------------------------------------------------------------------------
def random_sh(P, seed):
    sh = np.zeros(P, api.PROBE_SH_DTYPE)
    sh["c"] = np.random.default_rng(seed).normal(0, 1, (P, 9, 3))
    sh["cells"] = 256
    return sh


def irradiance_device(L, sh, points, grid=None, index=None):
    import torch
    out = runtime.sh_irradiance(L, to_device(words(sh)), to_device(words(points)), grid, None if index is None else to_device(np.asarray(index, np.int32)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_irradiance_of_one_probe_per_query(H, L):
    r = np.random.default_rng(11)
    sh = random_sh(7, 5)
    special = np.array([[0, 0, 0], [NAN, 0, 1], [0, INF, 1], [1, 2, -INF], [0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1e-30, 0, 0], [3e38, 3e38, 3e38], [1e-45, 1e-45, 0], [-0.0, 0.0, 0.0]], F)
    unit = r.normal(0, 1, (10000, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    normals = np.concatenate([special, unit, unit[32:96].astype(F) * 2.0 ** 20, unit[96:160].astype(F) * 2.0 ** -20, r.normal(0, 5, (500, 3))]).astype(F)
    points = points_of(r.uniform(-1, 1, (len(normals), 3)), normals)
    points["position"][::50] = NAN          # the position is not looked at
    index = r.integers(0, 7, len(normals))
    index[20:30] = [-1, 7, 8, -2 ** 31, 2 ** 31 - 1, 0, 6, 100, -7, 7]
    base = len(special)
    index[base + 10000:base + 10128] = index[base + 32:base + 160]          # (the scaled normals ask the probes their originals ask)
    want = probe_ref.irradiance(sh, points, index=index)
    got = irradiance_device(L, sh, points, index=index)
    assert H.same_bits(got, want)          # (10 000 normals of every length: the square root under N = normal / sqrt(q) is the correctly rounded one, or bits differ)
    assert not got[:4].view(np.uint32).any() and not got[11].view(np.uint32).any() and not got[[20, 21, 22, 23, 24, 27, 28, 29]].view(np.uint32).any()
    assert np.abs(got[4:11, :3]).min() > 0 and not got[:, 3].view(np.uint32).any()
    # a normal scaled by a power of two gives the same bits: q scales exactly, and so does its correctly rounded root
    assert H.same_bits(got[base + 10000:base + 10128], got[base + 32:base + 160])
    # the host form
    host = np.zeros((len(points), 4), F)
    idx = np.asarray(index, np.int32)
    assert L.sh_irradiance(words(sh).ctypes.data, 7, None, points.ctypes.data, idx.ctypes.data, len(points), host.ctypes.data) == 0, runtime.last_error()
    assert H.same_bits(host, got)


@pytest.mark.parametrize("counts,origin,spacing", [((3, 2, 2), (-1.0, 0.5, 2.0), (0.75, 1.5, 0.3)), ((1, 1, 1), (0.1, 0.2, 0.3), (1.0, 2.0, 3.0)), ((4, 1, 3), (0.0, 1.0, -1.0), (0.5, 1.0, -0.7))])
def test_irradiance_blended_in_a_grid(H, L, counts, origin, spacing):
    r = np.random.default_rng(sum(counts))
    P = counts[0] * counts[1] * counts[2]
    sh = random_sh(P, P)
    grid, probes = runtime.probe_grid(L, origin, spacing, counts)
    o, s, top = np.array(origin), np.array(spacing), np.array(counts) - 1
    faces = o + s * r.integers(0, 4, (200, 3)) * np.where(r.integers(0, 2, (200, 3)) > 0, 1.0, r.uniform(0, 1, (200, 3)))          # integer coordinates on some axes
    outside = o + s * (r.uniform(-2, 2, (300, 3)) * (top + 1) + np.where(r.integers(0, 2, (300, 3)) > 0, 4.0 * (top + 1), 0.0))
    inside = o + s * r.uniform(0, 1, (500, 3)) * top
    special = np.array([[NAN, 0, 0], [0, NAN, 0], [0, 0, NAN], [INF, 0, 0], [-INF, INF, 0], [0, 0, -INF]])
    positions = np.concatenate([probes["position"], faces, outside, inside, special]).astype(F)
    normals = r.normal(0, 1, (len(positions), 3)).astype(F)
    normals[-7] = 0
    points = points_of(positions, normals)
    want = probe_ref.irradiance(sh, points, grid=(origin, spacing, counts))
    got = irradiance_device(L, sh, points, grid=grid)
    assert H.same_bits(got, want)
    assert not got[-6:-3].view(np.uint32).any() and not got[-7].view(np.uint32).any() and np.abs(got[-3:, :3]).min() > 0
    # a query on a probe gets that probe's coefficients: the index-mode answer
    on = irradiance_device(L, sh, points[:P], index=np.arange(P))
    assert np.abs(got[:P] - on).max() <= 1e-6 * math.pi * np.abs(sh["c"]).max() * 9
    # constant coefficients across the grid: the index-mode answer wherever the query lies (the eight weights sum to 1 within binary64 rounding; the output is binary32)
    const = np.repeat(random_sh(1, 77), P)
    flat = irradiance_device(L, const, points, grid=grid)
    alone = irradiance_device(L, const, points, index=np.zeros(len(points), np.int32))
    alone[-6:-3] = 0          # (NaN positions: index mode does not look at them)
    assert np.abs(flat - alone).max() <= 1e-6 * math.pi * np.abs(const["c"]).max() * 9
    # the host form
    host = np.zeros((len(points), 4), F)
    assert L.sh_irradiance(words(sh).ctypes.data, P, C.byref(grid), points.ctypes.data, None, len(points), host.ctypes.data) == 0, runtime.last_error()
    assert H.same_bits(host, got)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------------
def test_bake_probes_is_the_chain(H, L):
    import torch
    d = scenes.cornell_box(16, 16, 4, bounces=4, integrator=api.kTerraIntegratorDirect)
    probes = points_of([[-0.4, 1.0, -0.3], [0.5, 1.4, 0.2]], [[0, 0, 1], [0.2, 1.0, -0.3]])
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        dp = to_device(words(probes))
        got = runtime.bake_probes(L, s, dp, cells=8)
        got2 = runtime.bake_probes(L, s, dp, cells=8, batches=2)
        jit = runtime.bake_probes(L, s, dp, cells=8, batches=2, jitter=5)
        # by hand: the four calls
        rays = runtime.probe_rays(L, dp, 8)
        fb = runtime.DeviceFramebuffer(64, 2)
        runtime.render_rays_device(L, s, rays, fb)
        sh1 = runtime.sh_project(L, fb, rays, 8)
        frame1 = fb.results_host().copy()
        runtime.render_rays_device(L, s, rays, fb)
        sh2 = runtime.sh_project(L, fb, rays, 8)
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        shj, frames = None, []
        for b in range(2):
            fj = runtime.DeviceFramebuffer(64, 2)
            rj = runtime.probe_rays(L, dp, 8, torch.rand((64, 2), generator=gen, dtype=torch.float32, device="cuda"))
            runtime.render_rays_device(L, s, rj, fj)
            shj = runtime.sh_project(L, fj, rj, 8, batch=b, sh=shj)
            frames.append((fj.results_host().copy(), rj.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 64)))
        torch.cuda.synchronize()
        host_rays = rays.cpu().numpy().view(api.RAY_DTYPE).reshape(2, 64)
        frame2 = fb.results_host()
    finally:
        L.scene_destroy(s)
    assert torch.equal(got, sh1) and torch.equal(got2, sh2) and torch.equal(jit, shj) and not torch.equal(got, got2) and not torch.equal(got2, jit)
    assert (frame1["samples"] == 4).all() and (frame2["samples"] == 8).all() and (frame1["acc"].sum(-1) > 0).mean() > 0.5
    # the frames are what the coefficients were made from: the restatement on them gives the same records
    for sh, frame in ((got, frame1), (got2, frame2)):
        want = probe_ref.project(frame, host_rays, 8)
        assert runtime.probe_sh_host(sh).tobytes() == want.tobytes() and (want["cells"] == 64).all()
    want = probe_ref.project(*frames[1], 8, 1, probe_ref.project(*frames[0], 8))
    assert runtime.probe_sh_host(jit).tobytes() == want.tobytes()


def test_probes_under_a_constant_sky(H, L):
    """environment lighting on, a constant sky S, nothing in sight: every cell's radiance is S, so the coefficients are the restatement's projection of a frame that
    is S everywhere (to 1e-5 S: the frame's means are S within a unit of the last place) and the irradiance is PI S within the centre set's own deviation, which the
    restatement gives, plus 1e-5"""
    import torch
    sky = np.array((0.5, 0.7, 0.9))
    n, K = 16, 256
    tris, nrm = scenes._quad((900.0, -900.0, 900.0), (900.001, -900.0, 900.0), (900.001, -900.0, 900.001), (900.0, -900.0, 900.001), (0, 1, 0))          # a speck, far off
    d = scenes.SceneDesc(objects=[scenes.ObjectDesc(tris, nrm, np.zeros((2, 3, 2), F))], width=16, height=16, spp=4, bounces=2, environment=tuple(sky), environment_lighting=True)
    probes = points_of([[0, 0, 0], [1, 2, 3], [-4, 0.5, 2]], [[0, 0, 1], [1, 1, 1], [0, -1, 0.2]])
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        dp = to_device(words(probes))
        sh = runtime.bake_probes(L, s, dp, cells=n)
        rays = runtime.probe_rays(L, dp, n).cpu().numpy().view(api.RAY_DTYPE).reshape(3, K)
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    frame = np.zeros((3, K), api.RESULT_DTYPE)
    frame["acc"], frame["samples"] = (4 * sky).astype(F), 4
    want = probe_ref.project(frame, rays, n)
    got = runtime.probe_sh_host(sh)
    assert (got["cells"] == K).all() and np.abs(got["c"].astype(D) - want["c"]).max() <= 1e-5 * sky.max()
    others = np.abs(want["c"][:, 1:] / sky).max()
    queries = points_of(np.zeros((6, 3)), [[0, 0, 1], [0, 1, 0], [1, 0, 0], [-1, -1, -1], [0.3, -2, 0.1], [0, 0, -5]])
    for p in range(3):
        E_ref = probe_ref.irradiance(want, queries, index=np.full(6, p))[:, :3] / (math.pi * sky)
        E = irradiance_device(L, got, queries, index=np.full(6, p))[:, :3] / (math.pi * sky)
        own = np.abs(E_ref - 1).max()
        print(f"probe {p}: other coefficients <= {others:.4f} S, restatement E / (PI S) - 1 in [{(E_ref - 1).min():.2e}, {(E_ref - 1).max():.2e}], device {np.abs(E - 1).max():.2e}")
        assert np.abs(E - 1).max() <= own + 1e-5
    assert others <= 0.0155 + 1e-4


def test_headless_probe_bake_against_the_runtime(H, L, tmp_path):
    import torch
    from test_headless_tool import build_tool, read_pfm, write_obj
    d = scenes.cornell_box(8, 8, 4, bounces=4, integrator=api.kTerraIntegratorDirect, environment=(0.4, 0.52, 1.0))
    obj = tmp_path / "cornell.obj"
    write_obj(d, obj)
    exe = build_tool(H, tmp_path, "amd")
    out = tmp_path / "probes.pfm"
    r = subprocess.run([str(exe), str(obj), str(out), "--bake-probes", "2x1x1", "--probe-cells", "4", "--spp", "4", "--passes", "2", "--bounces", "4", "--integrator", "direct",
                        "--no-flip-z", "--normals", "file"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "2x1x1 probes" in r.stdout
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        v = runtime.scene_vertex_points(L, s)["position"]
        grid, probes = runtime.probe_grid_over(L, v.min(0), v.max(0), (2, 1, 1))
        want = runtime.probe_sh_host(runtime.bake_probes(L, s, to_device(words(probes)), cells=4, batches=2))
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    assert np.array_equal(probes["position"], np.array([[-0.5, 1, 0], [0.5, 1, 0]], F)) and (want["cells"] == 16).all()
    got = read_pfm(out)
    assert got.shape == (2, 9, 3) and (want["c"][:, 0] > 0).all() and H.same_bits(got, want["c"])
