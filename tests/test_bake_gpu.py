"""Lightmap baking on the GPU (include/terra_amd.h "Lightmap baking"): terra_amd_atlas_points* and terra_amd_dilate* against the brute-force numpy restatement of
the header's two rules (tests/bake_ref.py), bit for bit over every texel of the points and of the texel records; then the chain runtime.bake_lightmap runs, and the
headless tool's --bake-lightmap against it. Frames are small: the reference tests every texel against every triangle."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import bake_ref
from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")


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


def soup(n, seed):
    """n triangles' world positions and (unnormalised) vertex normals, [n, 3, 3] float32 each"""
    r = np.random.default_rng(seed)
    return r.uniform(-1, 1, (n, 3, 3)).astype(F), r.uniform(-1, 1, (n, 3, 3)).astype(F)


def scene_of(L, pos, nrm, uv, cuts=()):
    """a committed scene of the triangles, cut into objects at the indices `cuts`"""
    pos, nrm, uv = (np.asarray(a, F) for a in (pos, nrm, uv))
    edges = [0, *cuts, len(pos)]
    objs = [scenes.ObjectDesc(pos[a:b], nrm[a:b], uv[a:b].reshape(-1, 3, 2)) for a, b in zip(edges[:-1], edges[1:])]
    L.clear_error()
    s = scenes.build_scene(L, scenes.SceneDesc(objects=objs, width=4, height=4, spp=1))
    assert runtime.last_error() == "", runtime.last_error()
    return s


def run_device(L, s, w, h, uvs=None, **kw):
    import torch
    pts, tex = runtime.atlas_points(L, s, runtime.atlas_of(w, h, **kw), None if uvs is None else to_device(np.asarray(uvs, F).reshape(-1, 6)))
    torch.cuda.synchronize()
    return pts.cpu().numpy(), tex.cpu().numpy().view(api.ATLAS_TEXEL_DTYPE).reshape(h, w)


def same(H, got, want):
    """every texel of the points and of the records, bit for bit"""
    return H.same_bits(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


def check(H, L, pos, nrm, uv, w, h, cuts=(), explicit=False, **kw):
    """device == reference for the scene's own texcoords (or the same uvs passed explicitly); returns the device's (points, texels)"""
    uv = np.asarray(uv, F).reshape(-1, 6)
    s = scene_of(L, pos, nrm, np.zeros_like(uv) if explicit else uv, cuts)
    try:
        got = run_device(L, s, w, h, uvs=uv if explicit else None, **kw)
    finally:
        L.scene_destroy(s)
    want = bake_ref.atlas_points(pos, nrm, uv, w, h, kw.get("uv_scale", (1, 1)), kw.get("uv_offset", (0, 0)), kw.get("margin", 0.5))
    assert same(H, got, want), f"{int((got[1]['triangle'] != want[1]['triangle']).sum())} texels took another triangle"
    return got


ONE = [[1.25, 0.75, 13.5, 3.0, 5.0, 10.25]]


@pytest.mark.parametrize("margin", [0.0, 1.0, 4.0])
def test_one_triangle(H, L, margin):
    pos, nrm = soup(1, 1)
    pts, tex = check(H, L, pos, nrm, ONE, 16, 12, margin=margin)
    covered = tex["triangle"] == 0
    assert 0 < covered.sum() < 16 * 12 or margin == 4.0
    assert (tex["triangle"][~covered] == -1).all() and not pts[~covered].view(np.uint32).any()
    assert ((tex["distance2"] > 0).any()) == (margin > 0)


@pytest.mark.parametrize("w,h", [(37, 19), (1, 1)])
def test_sizes_that_are_no_multiple_of_the_tile(H, L, w, h):
    pos, nrm = soup(3, 2)
    uv = [[-2.0, -1.0, w + 3.0, 0.5 * h, 0.25 * w, h + 2.0], [0.0, 0.0, w, 0.0, 0.0, h], [w, h, 0.5 * w, h, w, 0.25 * h]]
    check(H, L, pos, nrm, uv, w, h, margin=0.5)


def test_a_shared_edge_through_texel_centres_goes_to_the_lower_index(H, L):
    pos, nrm = soup(2, 3)
    quad = np.array([[0, 0, 8, 0, 8, 8], [0, 0, 8, 8, 0, 8]], F)
    for uv in (quad, quad[:, [0, 1, 4, 5, 2, 3]], quad[::-1]):          # as it is; reversed winding (area2 < 0); the two triangles swapped
        pts, tex = check(H, L, pos, nrm, uv, 8, 8, margin=0.0)
        assert (np.diag(tex["triangle"]) == 0).all() and (tex["triangle"] >= 0).all()


def test_overlapping_triangles_in_both_orders(H, L):
    pos, nrm = soup(2, 4)
    uv = np.array([[1, 1, 14, 2, 3, 13], [2, 12, 4, 1, 15, 9]], F)
    a = check(H, L, pos, nrm, uv, 16, 16, margin=1.0)
    b = check(H, L, pos[::-1], nrm[::-1], uv[::-1], 16, 16, margin=1.0)
    assert (a[1]["triangle"] == 0).any() and (a[1]["triangle"] == 1).any() and (b[1]["triangle"] == 0).any() and (b[1]["triangle"] == 1).any()


def test_triangles_that_cover_nothing_do_not_disturb_their_neighbours(H, L):
    pos, nrm = soup(5, 5)
    good = [[1, 1, 14, 2, 3, 13], [9, 14, 15, 6, 15, 15]]
    uv = np.array([[4, 4, 8, 8, 12, 12], good[0], [2, 2, NAN, 9, 12, 3], [5, 5, 5, 5, 5, 5], good[1]], F)          # collinear, NaN, a point
    pts, tex = check(H, L, pos, nrm, uv, 16, 16, margin=0.75)
    assert set(np.unique(tex["triangle"])) == {-1, 1, 4}
    alone = bake_ref.atlas_points(pos[[1, 4]], nrm[[1, 4]], good, 16, 16, margin=0.75)
    assert H.same_bits(pts, alone[0])


def test_triangles_off_the_atlas(H, L):
    pos, nrm = soup(3, 6)
    uv = np.array([[-30, -30, -20, -30, -25, -18], [40, 5, 60, 5, 50, 30], [-6.5, -3.25, 9, 4, -2, 11]], F)          # wholly off, twice; half off with negative coordinates
    pts, tex = check(H, L, pos, nrm, uv, 16, 16, margin=1.0)
    assert set(np.unique(tex["triangle"])) == {-1, 2}


def test_scale_and_offset_take_normalised_uvs_to_the_atlas(H, L):
    pos, nrm = soup(12, 7)
    uv = np.random.default_rng(7).uniform(-0.1, 1.1, (12, 6)).astype(F)
    check(H, L, pos, nrm, uv, 64, 64, uv_scale=(64.0, 64.0), uv_offset=(0.25, -0.5), margin=0.5)
    check(H, L, pos, nrm, uv, 64, 64, uv_scale=(-64.0, 32.0), uv_offset=(64.0, 16.0), margin=0.0)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_triangles(H, L, seed):
    pos, nrm = soup(200, seed)
    r = np.random.default_rng(seed)
    centre = r.uniform(-4, 68, (200, 1, 2))
    uv = (centre + r.normal(0, 1, (200, 1, 1)) ** 2 * 4 * r.uniform(-1, 1, (200, 3, 2))).astype(F)
    uv[::7] = np.round(uv[::7] * 2) / 2          # vertices on texel centres and borders
    check(H, L, pos, nrm, uv, 64, 64, cuts=(50, 51, 120), margin=0.75)


def grid_uvs(cells, size):
    """cells x cells quads of size x size texels, two triangles each"""
    j, i = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    x0, y0, x1, y1 = (a.reshape(-1).astype(F) for a in (i * size, j * size, (i + 1) * size, (j + 1) * size))
    return np.stack([np.stack([x0, y0, x1, y0, x1, y1], 1), np.stack([x0, y0, x1, y1, x0, y1], 1)], 1).reshape(-1, 6)


def test_a_grid_of_quads(H, L):
    uv = grid_uvs(32, 4.0)
    pos, nrm = soup(len(uv), 8)
    pts, tex = check(H, L, pos, nrm, uv, 128, 128, margin=0.5)
    assert len(uv) == 2048 and (tex["triangle"] >= 0).all() and len(np.unique(tex["triangle"])) == 2048


def test_one_triangle_over_a_large_atlas(H, L):
    pos, nrm = soup(1, 9)
    pts, tex = check(H, L, pos, nrm, [[-5, -5, 700, -5, -5, 700]], 300, 300, margin=0.5)
    assert (tex["triangle"] == 0).all()


def test_the_scenes_own_texcoords_against_the_same_uvs_passed(H, L):
    d = scenes.atlas(16, 16, 1)
    pos = np.concatenate([o.triangles for o in d.objects]); nrm = np.concatenate([o.normals for o in d.objects])
    uv = np.concatenate([np.asarray(o.texcoords, F).reshape(-1, 6) for o in d.objects])
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        own = run_device(L, s, 96, 64, margin=0.5, uv_scale=(2.0, 2.0), uv_offset=(24.0, 16.0))
        passed = run_device(L, s, 96, 64, uvs=uv, margin=0.5, uv_scale=(2.0, 2.0), uv_offset=(24.0, 16.0))
    finally:
        L.scene_destroy(s)
    want = bake_ref.atlas_points(pos, nrm, uv, 96, 64, (2.0, 2.0), (24.0, 16.0), 0.5)
    assert same(H, own, want) and same(H, passed, want) and (want[1]["triangle"] >= 0).any()
    # ... and uvs passed win over the scene's own
    pos2, nrm2 = soup(2, 10)
    check(H, L, pos2, nrm2, [[1, 1, 14, 2, 3, 13], [2, 12, 4, 1, 15, 9]], 16, 16, explicit=True, margin=0.5)


def test_host_form_against_device_form(H, L):
    pos, nrm = soup(40, 14)
    uv = np.random.default_rng(14).uniform(-3, 36, (40, 6)).astype(F)
    s = scene_of(L, pos, nrm, uv, cuts=(7,))
    try:
        dev = run_device(L, s, 33, 21, margin=1.5)
        dev_passed = run_device(L, s, 33, 21, uvs=uv[::-1], margin=1.5)
        atlas = runtime.atlas_of(33, 21, margin=1.5)
        for uvs, want in ((None, dev), (np.ascontiguousarray(uv[::-1]), dev_passed)):
            raw = np.full(33 * 21 * 8 + 4, 0x5ca1ab1e, np.uint32)
            at = ((-raw.ctypes.data) % 16) // 4
            tex = np.zeros((21, 33), api.ATLAS_TEXEL_DTYPE)
            assert L.atlas_points(s, C.byref(atlas), None if uvs is None else uvs.ctypes.data, raw.ctypes.data + 4 * at, tex.ctypes.data) == 0, runtime.last_error()
            assert raw[at:at + 33 * 21 * 8].tobytes() == want[0].tobytes() and tex.tobytes() == want[1].tobytes()
            assert (raw[:at] == 0x5ca1ab1e).all() and (raw[at + 33 * 21 * 8:] == 0x5ca1ab1e).all()
            assert L.atlas_points(s, C.byref(atlas), None if uvs is None else uvs.ctypes.data, raw.ctypes.data + 4 * at, None) == 0, runtime.last_error()          # texels are optional
            assert raw[at:at + 33 * 21 * 8].tobytes() == want[0].tobytes()
    finally:
        L.scene_destroy(s)


def test_objects_added_in_reverse_order(H, L):
    # one triangle in each 5 x 5 texel cell of a 6 x 6 grid, clear of the cell's border: no two triangles overlap or share an edge, so no texel is a tie between two
    # indices (a tie goes to the lower index, which the reversal changes); a gutter texel within the margin of two triangles takes the nearer
    pos, nrm = soup(36, 15)
    r = np.random.default_rng(15)
    j, i = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    uv = (np.stack([i, j], -1).reshape(36, 1, 2) * 5.0 + r.uniform(0.3, 4.7, (36, 3, 2))).astype(F)
    cuts = (5, 6, 20)
    fwd = check(H, L, pos, nrm, uv, 32, 32, cuts=cuts, margin=1.0)
    spans = list(zip([0, *cuts], [*cuts, 36]))[::-1]
    order = np.concatenate([np.arange(a, b) for a, b in spans])          # new index -> old index
    rev = check(H, L, pos[order], nrm[order], uv[order], 32, 32, cuts=tuple(np.cumsum([b - a for a, b in spans])[:-1]), margin=1.0)
    old = np.where(rev[1]["triangle"] >= 0, order[np.maximum(rev[1]["triangle"], 0)], -1)
    assert np.array_equal(old, fwd[1]["triangle"]) and (old >= 0).any() and (old < 0).any()
    assert H.same_bits(fwd[0], rev[0])
    for f in ("wb", "wc", "distance2"):
        assert H.same_bits(fwd[1][f], rev[1][f]), f


# ---- dilation --------------------------------------------------------------------------------------------------------------------------------------------------
def dilate_device(data, valid, passes):
    import torch
    d, v = to_device(data), to_device(valid)
    runtime.dilate(d, v, passes)
    torch.cuda.synchronize()
    return d.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(5, 4), (33, 17)])
def test_dilation(H, L, w, h, channels):
    r = np.random.default_rng(100 * w + channels)
    data = r.uniform(-2, 2, (h, w, channels)).astype(F)
    valid = (r.uniform(0, 1, (h, w)) < (0.2 if w == 5 else 0.04)).astype(np.int32) * r.integers(1, 9, (h, w)).astype(np.int32)          # islands; non-zero = valid
    assert valid.any() and not valid.all()
    for passes in (0, 1, 2, 3, 64):
        got = dilate_device(data, valid, passes)
        want = bake_ref.dilate(data, valid, passes)
        assert H.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), passes
        assert H.same_bits(got[0][valid != 0], data[valid != 0]) and np.array_equal(got[1][valid != 0], valid[valid != 0]), passes          # valid texels never change
        if passes == 0:
            assert H.same_bits(got[0], data) and np.array_equal(got[1], valid)
        if passes == 64:
            assert got[1].all()
    # the pass count matters where the islands are far apart: one pass does not fill the 33 x 17 frame
    if w == 33:
        assert not dilate_device(data, valid, 1)[1].all()


def test_dilation_of_an_all_invalid_frame_and_the_host_form(H, L):
    r = np.random.default_rng(5)
    data = r.uniform(-2, 2, (17, 33, 3)).astype(F)
    none = np.zeros((17, 33), np.int32)
    got = dilate_device(data, none, 3)
    assert H.same_bits(got[0], data) and not got[1].any()
    valid = (r.uniform(0, 1, (17, 33)) < 0.05).astype(np.int32)
    for passes in (0, 2, 5):
        d, v = data.copy(), valid.copy()
        assert L.dilate(d.ctypes.data, 3, v.ctypes.data, 33, 17, passes) == 0, runtime.last_error()
        want = bake_ref.dilate(data, valid, passes)
        assert H.same_bits(d, want[0]) and np.array_equal(v, want[1]), passes


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------------------------
FLOOR_UV = np.array([[3, 3, 12.5, 3, 12.5, 12.5], [3, 3, 12.5, 12.5, 3, 12.5]], F)          # the floor's quad on a 16 x 16 atlas, gutters around it


def test_bake_lightmap_is_the_chain(H, L):
    import torch
    d = scenes.cornell_box(16, 16, 16, bounces=4, integrator=api.kTerraIntegratorDirect)
    uv = np.zeros((32, 6), F); uv[0:2] = FLOOR_UV          # (the floor is the first two triangles of the first object; the other triangles' uvs are a point: nothing)
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        duv = to_device(uv)
        got, tex = runtime.bake_lightmap(L, s, 16, 16, uvs=duv, margin=0.5, dilate=2, batches=2)
        plain, _ = runtime.bake_lightmap(L, s, 16, 16, uvs=duv, margin=0.5, dilate=0, batches=2)
        # by hand
        points, texels = runtime.atlas_points(L, s, runtime.atlas_of(16, 16, margin=0.5), duv)
        fb = runtime.DeviceFramebuffer(16, 16)
        for _ in range(2):
            runtime.render_points_device(L, s, runtime.point_sampling(0), points, fb)
        res = fb.results.view(16, 16, 4)
        irr = (math.pi * res[..., :3].view(torch.float32) / res[..., 3:4].to(torch.float32)).contiguous()
        before = irr.cpu().numpy()
        valid = (texels[..., 0] >= 0).to(torch.int32).contiguous()
        runtime.dilate(irr, valid, 2)
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    t = tex.cpu().numpy().view(api.ATLAS_TEXEL_DTYPE).reshape(16, 16)
    assert torch.equal(tex, texels) and set(np.unique(t["triangle"])) == {-1, 0, 1}
    assert H.same_bits(got.cpu().numpy(), irr.cpu().numpy()) and H.same_bits(plain.cpu().numpy(), before)
    assert (before[t["triangle"] >= 0].sum(axis=-1) > 0).any() and not before[t["triangle"] < 0].view(np.uint32).any()          # uncovered texels are 0 before dilation
    want = bake_ref.dilate(before, (t["triangle"] >= 0).astype(np.int32), 2)
    assert H.same_bits(got.cpu().numpy(), want[0]) and (want[1] != 0).sum() > (t["triangle"] >= 0).sum()


def test_a_floor_under_a_constant_sky(H, L):
    sky = (0.5, 0.7, 0.9)
    tris, nrm = scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))
    d = scenes.SceneDesc(objects=[scenes.ObjectDesc(tris, nrm, FLOOR_UV.reshape(2, 3, 2))], width=16, height=16, spp=4, bounces=2, environment=sky, environment_lighting=True)
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        got, tex = runtime.bake_lightmap(L, s, 16, 16, margin=0.5, dilate=2)
        got = got.cpu().numpy(); t = tex.cpu().numpy().view(api.ATLAS_TEXEL_DTYPE).reshape(16, 16)
    finally:
        L.scene_destroy(s)
    valid = bake_ref.dilate(np.zeros((16, 16, 1), F), (t["triangle"] >= 0).astype(np.int32), 2)[1] != 0
    assert (t["triangle"] >= 0).sum() >= 81 and valid.sum() > (t["triangle"] >= 0).sum() and not valid.all()
    want = math.pi * np.array(sky)
    assert np.abs(got[valid] / want - 1).max() <= 1e-6          # (the dilated ones are means of equal values)
    assert not got[~valid].view(np.uint32).any()


def test_headless_bake_against_the_runtime(H, L, tmp_path):
    from test_headless_tool import build_tool, read_pfm
    floor = scenes._quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))
    light = scenes._quad((-0.25, 1.5, -0.25), (0.25, 1.5, -0.25), (0.25, 1.5, 0.25), (-0.25, 1.5, 0.25), (0, -1, 0))
    block = scenes._quad((-0.8, 0.6, -0.8), (-0.1, 0.6, -0.8), (-0.1, 0.6, -0.1), (-0.8, 0.6, -0.1), (0, 1, 0))
    vt = np.array([[[0.25, 0.25], [0.75, 0.25], [0.75, 0.75]], [[0.25, 0.25], [0.75, 0.75], [0.25, 0.75]]], F)          # the floor's chart; the others have none
    objs = [scenes.ObjectDesc(*floor, vt, scenes.Material(albedo=(0.7, 0.6, 0.5))), scenes.ObjectDesc(*light, np.zeros((2, 3, 2), F), scenes.Material(albedo=(0.5, 0.5, 0.5), emissive=(9.0, 8.0, 7.0))),
            scenes.ObjectDesc(*block, np.zeros((2, 3, 2), F), scenes.Material(albedo=(0.2, 0.3, 0.4)))]
    d = scenes.SceneDesc(objects=objs, width=8, height=8, spp=16, bounces=4, integrator=api.kTerraIntegratorDirect, environment=(0.4, 0.52, 1.0))
    obj = tmp_path / "lm.obj"
    with open(obj, "w") as f, open(obj.with_suffix(".mtl"), "w") as m:
        f.write("mtllib lm.mtl\n")
        vi = 1
        for k, o in enumerate(d.objects):
            mt = o.material
            m.write(f"newmtl m{k}\nKd {mt.albedo[0]:.9g} {mt.albedo[1]:.9g} {mt.albedo[2]:.9g}\nKe {mt.emissive[0]:.9g} {mt.emissive[1]:.9g} {mt.emissive[2]:.9g}\n")
            f.write(f"usemtl m{k}\n")
            for t, n, uv in zip(o.triangles, o.normals, o.texcoords):
                for c in range(3):
                    f.write(f"v {t[c][0]:.9g} {t[c][1]:.9g} {t[c][2]:.9g}\nvt {uv[c][0]:.9g} {uv[c][1]:.9g}\nvn {n[c][0]:.9g} {n[c][1]:.9g} {n[c][2]:.9g}\n")
                f.write(f"f {vi}/{vi}/{vi} {vi + 1}/{vi + 1}/{vi + 1} {vi + 2}/{vi + 2}/{vi + 2}\n")
                vi += 3
    exe = build_tool(H, tmp_path, "amd")
    out = tmp_path / "lm.pfm"
    r = subprocess.run([str(exe), str(obj), str(out), "--bake-lightmap", "--atlas", "8x8", "--bake-margin", "0.5", "--bake-dilate", "1", "--spp", "16", "--bounces", "4",
                        "--integrator", "direct", "--no-flip-z", "--normals", "file"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        want, tex = runtime.bake_lightmap(L, s, 8, 8, uv_scale=(8.0, 8.0), margin=0.5, dilate=1)
        want = want.cpu().numpy(); t = tex.cpu().numpy().view(api.ATLAS_TEXEL_DTYPE).reshape(8, 8)["triangle"]
    finally:
        L.scene_destroy(s)
    got = read_pfm(out)
    assert got.shape == (8, 8, 3) and (t >= 0).sum() == 32 and set(np.unique(t)) == {-1, 0, 1} and (want[t >= 0].sum(axis=-1) > 0).any() and (want[t < 0] > 0).any()
    assert not want[0, 0].any() and H.same_bits(got, want)
