"""First-hit AOV buffers (terra_amd_render_aov_device / terra_amd_render_aov; include/terra_amd.h "AOV buffers").

The contract: sample n of a pixel in the AOV buffer traces exactly the camera ray sample n of the same pixel traces in the render, when the AOV calls mirror the
render calls. The DebugMono integrator adds 1 per sample whose camera ray hits (acc.x = coverage, bit for bit), DebugDepth adds |hit - camera| / 500 per hit
(acc.x ~ depth / 500: the two sums round differently, at most 32 samples per pixel here). So these tests also pin the job / stream machinery -- sample split,
job order, stream keys, sampler draws -- from outside the render kernel."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    from terra_amd import runtime
    assert torch.cuda.is_available()
    return runtime.load()


def _scene(L, d, tree_mode=None, split=None, job_order=None):
    from terra_amd import runtime
    L.clear_error()
    s = scenes.build_scene(L, d, tree_mode=tree_mode)
    assert runtime.last_error() == "", runtime.last_error()
    if split is not None:
        runtime.check(L.set_sample_split(s, split))
    if job_order is not None:
        runtime.check(L.set_job_order(s, job_order))
    return s


def _calls(d, rects, repeat):
    return [r for _ in range(repeat) for r in (rects or [(0, 0, d.width, d.height)])]


def aligned_frames(L, make, rects=None, repeat=1, **kw):
    """(AOV sums, DebugMono results, DebugDepth results) of the same calls"""
    import torch
    from terra_amd import runtime
    out = {}
    for integ in (api.kTerraIntegratorDebugMono, api.kTerraIntegratorDebugDepth):
        d = make(integ)
        s = _scene(L, d, **kw)
        cam = scenes.camera_of(d)
        fb = runtime.DeviceFramebuffer(d.width, d.height)
        aov = runtime.DeviceAov(d.width, d.height) if integ == api.kTerraIntegratorDebugMono else None
        for r in _calls(d, rects, repeat):
            runtime.render_device(L, cam, s, fb, rect=r)
            if aov is not None:
                runtime.render_aov_device(L, cam, s, aov, rect=r)
        torch.cuda.synchronize()
        out[integ] = fb.results_host().copy()
        if aov is not None:
            out["aov"] = aov.host().copy()
        L.scene_destroy(s)
    return out["aov"], out[api.kTerraIntegratorDebugMono], out[api.kTerraIntegratorDebugDepth]


def check_alignment(aov, mono, depth):
    assert np.array_equal(aov["samples"], mono["samples"]) and np.array_equal(aov["samples"], depth["samples"])
    assert np.array_equal(aov["coverage"].view(np.uint32), mono["acc"][..., 0].view(np.uint32)), "coverage differs from DebugMono's hit count"
    assert aov["coverage"].max() > 0
    np.testing.assert_allclose(aov["depth"] / np.float32(500), depth["acc"][..., 0], rtol=1e-5, atol=0)
    assert np.all(aov["reserved"] == 0)


@pytest.mark.parametrize("split,order", [(1, 0), (4, 0), (4, 2), (0, 0), (0, 2)])
def test_alignment_cornell_split_and_job_order(L, split, order):
    aov, mono, depth = aligned_frames(L, lambda i: scenes.cornell_box(64, 48, 32, integrator=i), split=split, job_order=order)
    check_alignment(aov, mono, depth)


def test_alignment_stratified_sampler_integration(L):
    def make(i):
        return scenes.cornell_box(48, 32, 16, integrator=i, sampling=api.kTerraSamplingMethodStratified, strata=4, sampler_integration=True)
    check_alignment(*aligned_frames(L, make, split=4))


def test_alignment_two_successive_calls(L):
    aov, mono, depth = aligned_frames(L, lambda i: scenes.cornell_box(48, 32, 8, integrator=i), repeat=2, split=2)
    assert np.all(aov["samples"] == 16)
    check_alignment(aov, mono, depth)


def test_alignment_tiles_and_full_frame(L):
    tiles = [(x, y, min(32, 80 - x), min(32, 48 - y)) for y in (0, 32) for x in (0, 32, 64)]
    make = lambda i: scenes.cornell_box(80, 48, 8, integrator=i)
    aov_t, mono, depth = aligned_frames(L, make, rects=tiles, split=1)
    check_alignment(aov_t, mono, depth)
    aov_f, _, _ = aligned_frames(L, make, split=1)
    assert np.array_equal(aov_t.view(np.uint8), aov_f.view(np.uint8)), "tile-by-tile AOV calls differ from one full-frame call"


def test_alignment_small_hall_fast_tree(L):
    from terra_amd import runtime
    aov, mono, depth = aligned_frames(L, lambda i: scenes.sponza_hall(96, 64, 4, integrator=i), split=2)
    check_alignment(aov, mono, depth)
    d = scenes.sponza_hall(32, 16, 1)
    s = _scene(L, d)
    ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
    assert ti.fast_tree == 1
    L.scene_destroy(s)


def test_alignment_replica_tree(L):
    check_alignment(*aligned_frames(L, lambda i: scenes.cornell_box(64, 48, 16, integrator=i), tree_mode=0, split=2))


def test_alignment_hall_x100_reachability_mode(L):
    from tools.scaled_hall import scaled
    check_alignment(*aligned_frames(L, lambda i: scaled(scenes.sponza_hall(64, 36, 2, integrator=i), 100.0)))


def test_fast_tree_stack_hooks_leave_the_buffer_unchanged(H, L):
    """The AOV launcher sizes its LDS and its stack spill from the plan the call hands it (launch_plan.h: terra_clamp_leaf_cap, terra_spill_bytes). On the forced
    fast tree (tree mode 1: the launcher takes the stack from the call; the reference tree's it plans itself, so the hooks do nothing there) a short LDS column
    sends nearly every push to the HBM part, and 60 padded entries make the block ask for more than 64 KB, which the launcher opts in to: the same buffer, bit
    for bit, each time."""
    import torch
    from terra_amd import runtime
    from test_oracle_vs_reference import soup_scene
    d = soup_scene(H, 1500, 77); d.width, d.height, d.spp = 64, 40, 2
    s = _scene(L, d, tree_mode=1)
    cam = scenes.camera_of(d)

    def render():
        aov = runtime.DeviceAov(d.width, d.height)
        runtime.render_aov_device(L, cam, s, aov); torch.cuda.synchronize()
        return aov.host().copy()
    try:
        plain = render()
        assert plain["coverage"].sum() > 0
        for fast_lds, pad in ((1, 0), (2, 0), (0, 60)):
            runtime.check(L.debug_fast_stack_lds(s, fast_lds)); runtime.check(L.debug_pad_stack(s, pad))
            assert np.array_equal(render().view(np.uint8), plain.view(np.uint8)), (fast_lds, pad)
    finally:
        L.debug_fast_stack_lds(s, 0); L.debug_pad_stack(s, 0)
        L.scene_destroy(s)


@pytest.mark.parametrize("make", [scenes.cornell_box, scenes.cornell_phong], ids=["diffuse", "phong"])
def test_exact_first_hits(H, L, make):
    """spp 1, no jitter: every pixel's first hit is the pixel-centre ray's, as the unit camera + raycast give it"""
    import torch
    from terra_amd import runtime
    d = make(40, 30, 1, jitter=0.0)
    s = _scene(L, d)
    cam = scenes.camera_of(d)
    aov = runtime.DeviceAov(d.width, d.height)
    runtime.render_aov_device(L, cam, s, aov); torch.cuda.synchronize()
    a = aov.host().reshape(-1)
    U = H.Unit("amd")
    xy = np.stack(np.meshgrid(np.arange(d.width), np.arange(d.height)), -1).reshape(-1, 2).astype(np.uint32)
    dirs = U.camera_dirs(cam, d.width, d.height, xy, 0.0, np.zeros((len(xy), 2), np.float32))
    o = np.tile(np.asarray(d.camera_position, np.float32), (len(xy), 1))
    obj, _, point, surf = U.raycast(s, o, dirs)
    hit = obj >= 0
    assert hit.any()
    assert np.array_equal(a["coverage"], hit.astype(np.float32))
    assert np.array_equal(a["normal"][hit].view(np.uint32), surf[hit, 16:19].view(np.uint32))
    slot = np.array([1 if d.objects[k].material.kind == "phong" else 0 for k in range(len(d.objects))])
    want_albedo = np.stack([surf[i, 23 + 3 * slot[obj[i]]: 26 + 3 * slot[obj[i]]] for i in np.nonzero(hit)[0]])
    assert np.array_equal(a["albedo"][hit].view(np.uint32), want_albedo.view(np.uint32))
    v = point[hit] - o[hit]
    want_depth = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    assert np.all(np.abs(a["depth"][hit].view(np.int32).astype(np.int64) - want_depth.view(np.int32).astype(np.int64)) <= 1)
    assert np.all(a["normal"][~hit] == 0) and np.all(a["albedo"][~hit] == 0) and np.all(a["depth"][~hit] == 0)
    if make is scenes.cornell_phong:
        assert any(d.objects[k].material.kind == "phong" for k in set(obj[hit].tolist()))
    L.scene_destroy(s)


def test_textured_albedo(H, L):
    import torch
    from terra_amd import runtime
    d = scenes.cornell_textured(64, 48, 1)
    s = _scene(L, d)
    cam = scenes.camera_of(d)
    aov = runtime.DeviceAov(d.width, d.height)
    runtime.render_aov_device(L, cam, s, aov); torch.cuda.synchronize()
    a = aov.host()
    # by value: a point-filtered checker albedo is one of its texels / 255, the untextured green wall's is its constant
    checker = d.objects[0].material.albedo_texture.data.reshape(-1, 3)
    texels = {tuple(np.float32(c) / np.float32(255) for c in t) for t in checker.tolist()}
    green = tuple(np.float32(c) for c in d.objects[2].material.albedo)
    got = [tuple(np.float32(c) for c in v) for v in a["albedo"].reshape(-1, 3).tolist()]
    n_checker = sum(1 for g in got if g in texels)
    n_green = sum(1 for g in got if g == green)
    assert n_checker > 0.2 * len(got) and n_green > 0.02 * len(got), (n_checker, n_green)
    assert len({g for g in got if g in texels}) == 2          # both checker colours are seen
    L.scene_destroy(s)


def test_misses_are_zero_and_host_form_equals_device_form(L):
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(48, 32, 4)
    s = _scene(L, d, split=2)
    cam = scenes.camera_of(d)
    away = scenes.camera_of(d); away.direction = api.f3((0.0, 0.0, -1.0))       # out of the open front: every camera ray leaves the scene
    aov = runtime.DeviceAov(d.width, d.height)
    runtime.render_aov_device(L, away, s, aov); torch.cuda.synchronize()
    a = aov.host()
    assert np.all(a["samples"] == 4)
    for f in ("albedo", "coverage", "normal", "depth", "reserved"):
        assert np.all(a[f].view(np.uint32) == 0), f
    dev = runtime.DeviceAov(d.width, d.height)
    host = np.zeros((d.height, d.width), runtime.AOV_DTYPE)
    for r in [(0, 0, 48, 32), (5, 3, 20, 17), (0, 0, 48, 32)]:
        runtime.render_aov_device(L, cam, s, dev, rect=r)
        runtime.check(L.render_aov(C.byref(cam), s, host.ctypes.data, d.width, d.height, *r), "terra_amd_render_aov")
    torch.cuda.synchronize()
    assert np.array_equal(dev.host().view(np.uint8), host.view(np.uint8))
    assert host["coverage"].max() > 0
    L.scene_destroy(s)


def test_framebuffer_and_stats_untouched(L):
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(64, 48, 8, integrator=api.kTerraIntegratorDirect)
    frames, stats = [], []
    for with_aov in (False, True):
        s = _scene(L, d, split=0, job_order=2)
        cam = scenes.camera_of(d)
        fb = runtime.DeviceFramebuffer(d.width, d.height)
        aov = runtime.DeviceAov(d.width, d.height)
        for r in [(0, 0, 64, 48), (16, 16, 32, 32)]:
            if with_aov:
                runtime.render_aov_device(L, cam, s, aov, rect=r)
            runtime.render_device(L, cam, s, fb, rect=r)
            if with_aov:
                runtime.render_aov_device(L, cam, s, aov, rect=r)
        torch.cuda.synchronize()
        st = runtime.Stats(); runtime.check(L.get_stats(s, C.byref(st)))
        frames.append((fb.pixels_host().copy(), fb.results_host().copy()))
        stats.append(st.as_dict())
        L.scene_destroy(s)
    assert np.array_equal(frames[0][0].view(np.uint32), frames[1][0].view(np.uint32))
    assert np.array_equal(frames[0][1].view(np.uint8), frames[1][1].view(np.uint8))
    assert stats[0] == stats[1]


def test_error_paths_write_nothing(L):
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(32, 16, 2)
    cam = scenes.camera_of(d)
    aov = runtime.DeviceAov(d.width, d.height)
    aov.data.fill_(0x12345678)
    before = aov.data.clone()
    raw = L.scene_create()            # objects added, never committed
    obj = L.scene_add_object(raw, len(d.objects[0].triangles)).contents
    scenes.fill_object(L, obj, d.objects[0])
    assert L.render_aov_device(C.byref(cam), raw, aov.data.data_ptr(), 32, 16, 0, 0, 32, 16, None) == -2
    s = _scene(L, d)
    assert L.render_aov_device(C.byref(cam), s, aov.data.data_ptr(), 32, 16, 8, 0, 32, 16, None) == -4       # rectangle beyond the frame
    assert L.render_aov_device(C.byref(cam), s, aov.data.data_ptr(), 32, 16, 0, 0, 0, 16, None) == -4        # empty rectangle
    assert L.render_aov_device(C.byref(cam), s, None, 32, 16, 0, 0, 32, 16, None) == -4                      # null buffer
    assert L.render_aov(C.byref(cam), s, None, 32, 16, 0, 0, 32, 16) == -4
    assert "null" in runtime.last_error()
    torch.cuda.synchronize()
    assert torch.equal(aov.data, before)
    L.scene_destroy(s); L.scene_destroy(raw)
    L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()       # (the errors provoked here are not the next test's)
