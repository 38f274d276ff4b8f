"""Ray-sourced rendering on the GPU (include/terra_amd.h "Ray-sourced rendering"): terra_amd_render_rays* / terra_amd_render_aov_rays* pinned, on bits, against the
two things the project already trusts -- the camera door for rays that equal the camera's, and the oracle's orc_trace_one / orc_raycast for rays that are no camera's.

Frames are 48 x 40 (three by three 16 x 16 blocks, the last column and row partial), rendered whole and as the rectangle (5, 3, 37, 30); 4 samples per pixel with the
sample split set to 2 on both doors (the automatic split differs between them by design: a ray launch never has the job order)."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

W, HGT, SPP, SPLIT = 48, 40, 4, 2
RECT = (5, 3, 37, 30)
RECTS = [None, RECT]
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4
CALL_REPLICA = 1
INTEGRATORS = [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis, api.kTerraIntegratorDebugMono, api.kTerraIntegratorDebugDepth,
               api.kTerraIntegratorDebugNormals, api.kTerraIntegratorDebugMisWeights]
LIGHT3 = [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis]


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def make_scene(L, d, tree_mode=None, split=SPLIT):
    L.clear_error()
    s = scenes.build_scene(L, d, tree_mode=tree_mode)
    assert runtime.last_error() == "", runtime.last_error()
    runtime.check(L.set_sample_split(s, split))
    return s


def pinhole_rays(H, d):
    """the camera's own rays at jitter 0, [height, width, 8]: the camera position and the direction the device's camera unit gives the pixel"""
    xy = np.array([(x, y) for y in range(d.height) for x in range(d.width)], np.uint32)
    dirs = H.Unit("amd").camera_dirs(scenes.camera_of(d), d.width, d.height, xy, 0.0, np.zeros((len(xy), 2), np.float32))
    rays = np.zeros((d.height * d.width, 8), np.float32)
    rays[:, 0:3] = np.asarray(d.camera_position, np.float32); rays[:, 3] = np.inf; rays[:, 4:7] = dirs
    return rays.reshape(d.height, d.width, 8)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Frame:
    """a device framebuffer with its per-pixel draw counts"""

    def __init__(self, w=W, h=HGT):
        import torch
        self.fb = runtime.DeviceFramebuffer(w, h)
        self.calls = torch.full((h * w,), 0x5ca1ab1e, dtype=torch.int32, device="cuda")

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.fb.pixels_host().copy(), self.fb.results_host().copy(), self.calls.cpu().numpy().reshape(self.fb.height, self.fb.width).copy()


def assert_same_frames(H, a, b, what):
    (pa, ra, ca), (pb, rb, cb) = a, b
    assert np.array_equal(ra["samples"], rb["samples"]), what
    assert H.same_bits(ra["acc"], rb["acc"]), what
    assert H.same_bits(pa, pb), what
    assert np.array_equal(ca, cb), what


def both_doors(H, L, d, rect, calls=1, tree_mode=None):
    """the same calls through the camera door and through the ray door with the camera's own rays: (camera frame, ray frame, last_call of each)"""
    s = make_scene(L, d, tree_mode=tree_mode)
    try:
        cam = scenes.camera_of(d)
        rays = to_device(pinhole_rays(H, d))
        fc, fr = Frame(d.width, d.height), Frame(d.width, d.height)
        ti = runtime.TraversalInfo()
        for _ in range(calls):
            runtime.render_device(L, cam, s, fc.fb, rect=rect, rand_calls=fc.calls)
        runtime.check(L.traversal_info(s, C.byref(ti))); last_cam = ti.last_call
        for _ in range(calls):
            runtime.render_rays_device(L, s, rays, fr.fb, rect=rect, rand_calls=fr.calls)
        runtime.check(L.traversal_info(s, C.byref(ti))); last_ray = ti.last_call
        assert runtime.empty_skip_info(L, s)[0] == 0                      # a ray launch never skips
        return fc.host(), fr.host(), last_cam, last_ray
    finally:
        L.scene_destroy(s)


def check_doors(H, L, d, rect, calls=1, tree_mode=None):
    cam, ray, last_cam, last_ray = both_doors(H, L, d, rect, calls, tree_mode)
    x, y, w, h = rect or (0, 0, d.width, d.height)
    assert (cam[1]["samples"][y:y + h, x:x + w] == calls * d.spp).all() and cam[1]["samples"].sum() == calls * d.spp * w * h
    assert cam[1]["acc"].max() > 0
    assert_same_frames(H, cam, ray, (d.integrator, rect, calls, tree_mode))
    assert last_cam == last_ray and last_ray != 0
    return ray


# ---- 1. the ray door with the camera's rays is the camera door -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_camera_rays_cornell_all_integrators(H, L, integrator, rect):
    check_doors(H, L, scenes.cornell_box(W, HGT, SPP, integrator=integrator, jitter=0.0), rect)


@pytest.mark.parametrize("tree_mode", [0, 1])
@pytest.mark.parametrize("integrator", LIGHT3)
def test_camera_rays_cornell_tree_modes(H, L, integrator, tree_mode):
    check_doors(H, L, scenes.cornell_box(W, HGT, SPP, integrator=integrator, jitter=0.0), RECT, tree_mode=tree_mode)


@pytest.mark.parametrize("integrator", LIGHT3)
def test_camera_rays_small_hall_fast_tree(H, L, integrator):
    d = scenes.sponza_hall(W, HGT, SPP, integrator=integrator, jitter=0.0, detail=0.25)
    cam, ray, last_cam, last_ray = both_doors(H, L, d, RECT)
    assert_same_frames(H, cam, ray, integrator)
    assert last_ray == last_cam == 3                                        # fast tree, read from HBM


def test_camera_rays_out_of_range_scene(H, L):
    from tools.scaled_hall import scaled
    d = scaled(scenes.sponza_hall(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0, detail=0.25), 100.0)
    cam, ray, last_cam, last_ray = both_doors(H, L, d, RECT)
    assert_same_frames(H, cam, ray, "hall x 100")
    assert last_ray == last_cam == 4                                        # fast tree + reachability replay


@pytest.mark.parametrize("integrator", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirectMis])
@pytest.mark.parametrize("make", [scenes.cornell_phong, scenes.cornell_spheres], ids=["phong", "spheres"])
def test_camera_rays_other_materials(H, L, make, integrator):
    check_doors(H, L, make(W, HGT, SPP, integrator=integrator, jitter=0.0), None)


def test_camera_rays_two_successive_calls(H, L):
    check_doors(H, L, scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0), RECT, calls=2)


@pytest.mark.parametrize("sampling,strata", [(api.kTerraSamplingMethodStratified, 2), (api.kTerraSamplingMethodHalton, 0)], ids=["stratified", "halton"])
def test_camera_rays_sampler_integration(H, L, sampling, strata):
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorSimple, jitter=0.0, sampling=sampling, strata=strata, sampler_integration=True)
    check_doors(H, L, d, RECT, calls=2)


# ---- 2. rays that are no camera's: the oracle ------------------------------------------------------------------------------------------------------------------
N_FREE = 256
FREE_W, FREE_H = 16, 16


def free_rays(H):
    o, d = H.scene_rays(91, N_FREE)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)      # (scene_rays leaves a few diagonal ones unnormalised)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def free_frame(o, d):
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = np.inf; rays[:, 4:7] = d
    return rays.reshape(FREE_H, FREE_W, 8)


_oracle = {}


def oracle_sums(H, integrator, passes=3):
    """float32 running sums of orc_trace_one over passes 0 .. passes-1 (one sample each, keyed (frame seed, pixel, s)) and the draws of each pass, computed once"""
    if integrator not in _oracle:
        H.set_oracle_math(1)
        try:
            u = H.Unit("orc")
            d = scenes.cornell_box(FREE_W, FREE_H, 1, integrator=integrator, jitter=0.0)
            sc = scenes.build_scene(u.L, d)
            o, dirs = free_rays(H)
            key = u.L.fn("orc_pixel_stream_key", None, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p])
            acc = np.zeros((N_FREE, 3), np.float32); sums, calls = [], []
            for s in range(passes):
                k3 = np.zeros((N_FREE, 3), np.uint64)
                for i in range(N_FREE):
                    key(scenes.FRAME_SEED, i, s, k3[i].ctypes.data)
                rad, c = u.trace(sc, o, dirs, np.ascontiguousarray(k3[:, 1]), np.ascontiguousarray(k3[:, 2]))
                acc = (acc + rad).astype(np.float32)
                sums.append(acc.copy()); calls.append(c.copy())
            u.L.scene_destroy(sc)
            _oracle[integrator] = (sums, calls)
        finally:
            H.set_oracle_math(0)
    return _oracle[integrator]


@pytest.mark.parametrize("integrator", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect])
def test_free_rays_equal_the_oracle(H, L, orc_lib, integrator):
    sums, calls = oracle_sums(H, integrator)
    assert sums[2].max() > 0 and (sums[2].sum(axis=1) == 0).any()                 # some rays gather light, some none
    o, dirs = free_rays(H)
    rays = to_device(free_frame(o, dirs))
    d = scenes.cornell_box(FREE_W, FREE_H, 1, integrator=integrator, jitter=0.0)
    s = make_scene(L, d, split=1)
    try:
        f = Frame(FREE_W, FREE_H)
        for p in range(3):
            runtime.render_rays_device(L, s, rays, f.fb, rand_calls=f.calls)
            _, res, c = f.host()
            assert (res["samples"] == p + 1).all()
            assert H.same_bits(res["acc"].reshape(-1, 3), sums[p]), (integrator, p)
            assert np.array_equal(c.reshape(-1).astype(np.uint32), calls[p]), (integrator, p)
    finally:
        L.scene_destroy(s)
    # one call at 4 samples per pixel, split 4 = four calls at 1
    d4 = scenes.cornell_box(FREE_W, FREE_H, 4, integrator=integrator, jitter=0.0)
    s1, s4 = make_scene(L, d, split=1), make_scene(L, d4, split=4)
    try:
        f1, f4 = Frame(FREE_W, FREE_H), Frame(FREE_W, FREE_H)
        for _ in range(4):
            runtime.render_rays_device(L, s1, rays, f1.fb)
        runtime.render_rays_device(L, s4, rays, f4.fb)
        (p1, r1, _), (p4, r4, _) = f1.host(), f4.host()
        assert r1.tobytes() == r4.tobytes() and H.same_bits(p1, p4)
        assert (r1["samples"] == 4).all()
    finally:
        L.scene_destroy(s1); L.scene_destroy(s4)


# ---- 3. inactive rays -----------------------------------------------------------------------------------------------------------------------------------------
def test_inactive_rays(H, L):
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0)
    base = pinhole_rays(H, d)
    marked = base.copy()
    r = H.rng(5)
    off = r.uniform(size=(HGT, W)) < 0.1                                       # a scattered tenth: a zero direction
    marked[off, 4:7] = 0.0
    odd = [((7, 9), 0, np.nan), ((20, 30), 1, np.inf), ((33, 2), 2, -np.inf), ((12, 40), 4, np.nan), ((25, 11), 5, np.inf), ((39, 47), 6, -np.inf), ((0, 0), 4, np.nan)]
    for (y, x), word, v in odd:                                                # one of the six components not finite
        marked[y, x, word] = v; off[y, x] = True
    marked[3, 3, 3] = np.nan; marked[3, 4, 7] = np.inf; marked[3, 5, 3] = -1.0  # tmax and reserved are ignored: these stay active
    assert not off[3, 3:6].any() and 0.05 < off.mean() < 0.2
    s = make_scene(L, d)
    try:
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
        frames = {}
        for rect in RECTS:
            for name, rays in (("base", base), ("marked", marked)):
                f = Frame()
                runtime.render_rays_device(L, s, to_device(rays), f.fb, rect=rect, rand_calls=f.calls)
                frames[name] = f.host()
            runtime.check(L.traversal_info(s, C.byref(ti)))
            assert ti.last_call == (2 if ti.leaf_cull else 1)                      # what the commit chose (the Cornell box: reference tree + leaf-box cull)
            x, y, w, h = rect or (0, 0, W, HGT)
            inside = np.zeros((HGT, W), bool); inside[y:y + h, x:x + w] = True
            (pb, rb, cb), (pm, rm, cm) = frames["base"], frames["marked"]
            dead, live = off & inside, ~off & inside
            assert dead.sum() > 50
            assert not rm["acc"][dead].view(np.uint32).any()                       # +0, not -0
            assert (rm["samples"][dead] == SPP).all() and (cm[dead] == 0).all()
            assert not pm[dead].view(np.uint32).any()
            assert H.same_bits(rm["acc"][live], rb["acc"][live]) and np.array_equal(rm["samples"][live], rb["samples"][live])
            assert H.same_bits(pm[live], pb[live]) and np.array_equal(cm[live], cb[live])
            assert (cb[live] > 0).any()
            assert not rm[~inside].tobytes().strip(b"\0") and (cm[~inside] == 0x5ca1ab1e).all()
    finally:
        L.scene_destroy(s)


# ---- 4. host form -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
def test_host_form_equals_device_form(H, L, rect):
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0)
    rays = np.ascontiguousarray(pinhole_rays(H, d))
    s = make_scene(L, d)
    try:
        f = Frame()
        fb = api.Framebuffer(L, W, HGT)
        x, y, w, h = rect or (0, 0, W, HGT)
        for _ in range(2):
            runtime.render_rays_device(L, s, to_device(rays), f.fb, rect=rect)
            L.clear_error()
            assert L.render_rays(s, rays.ctypes.data, C.byref(fb.fb), x, y, w, h) == 0, runtime.last_error()
        pix, res, _ = f.host()
        assert fb.results.tobytes() == res.tobytes() and H.same_bits(fb.pixels, pix)
        assert res["samples"].sum() == 2 * SPP * w * h
        fb.destroy()
    finally:
        L.scene_destroy(s)


def test_host_form_far_origin_runs_the_replica(H, L, orc_lib):
    sums, _ = oracle_sums(H, api.kTerraIntegratorSimple)
    o, dirs = free_rays(H)
    d = scenes.cornell_box(FREE_W, FREE_H, 1, integrator=api.kTerraIntegratorSimple, jitter=0.0)
    s = make_scene(L, d, split=1)
    try:
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
        assert ti.leaf_cull == 1 and np.abs(o).max() < ti.camera_limit
        frame = free_frame(o, dirs)
        far = frame.copy()
        # ray 17 from beyond camera_limit towards where it was aimed: not the oracle's ray 17, so that pixel is left out of the comparison below
        far[17 // FREE_W, 17 % FREE_W, 0:3] = o[17] - dirs[17] * np.float32(4.0 * ti.camera_limit)
        assert np.abs(far[17 // FREE_W, 17 % FREE_W, 0:3]).max() > ti.camera_limit
        keep = np.arange(N_FREE) != 17
        for rays, want_call in ((frame, 2), (far, CALL_REPLICA)):
            fb = api.Framebuffer(L, FREE_W, FREE_H)
            for p in range(3):
                L.clear_error()
                assert L.render_rays(s, np.ascontiguousarray(rays).ctypes.data, C.byref(fb.fb), 0, 0, FREE_W, FREE_H) == 0, runtime.last_error()
                runtime.check(L.traversal_info(s, C.byref(ti)))
                assert ti.last_call == want_call
                assert H.same_bits(fb.results["acc"].reshape(-1, 3)[keep], sums[p][keep]), (want_call, p)
            fb.destroy()
        # an INACTIVE record out there does not give up the shortcut
        idle = frame.copy(); idle[0, 0, 0:3] = 1e6; idle[0, 0, 4:7] = 0.0
        fb = api.Framebuffer(L, FREE_W, FREE_H)
        assert L.render_rays(s, np.ascontiguousarray(idle).ctypes.data, C.byref(fb.fb), 0, 0, FREE_W, FREE_H) == 0
        runtime.check(L.traversal_info(s, C.byref(ti)))
        assert ti.last_call == 2
        fb.destroy()
    finally:
        L.scene_destroy(s)


# ---- 5. AOV ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
def test_aov_camera_rays_equal_the_camera_aov(H, L, rect):
    import torch
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorSimple, jitter=0.0)
    rays = to_device(pinhole_rays(H, d))
    s = make_scene(L, d)
    try:
        cam = scenes.camera_of(d)
        ac, ar = runtime.DeviceAov(W, HGT), runtime.DeviceAov(W, HGT)
        for _ in range(2):
            runtime.render_aov_device(L, cam, s, ac, rect=rect)
            runtime.render_aov_rays_device(L, s, rays, ar, rect=rect)
        torch.cuda.synchronize()
        a, b = ac.host(), ar.host()
        assert a["coverage"].max() == 2 * SPP and a.tobytes() == b.tobytes()
        # the host form, frame-indexed
        x, y, w, h = rect or (0, 0, W, HGT)
        host = np.zeros((HGT, W), runtime.AOV_DTYPE)
        hr = np.ascontiguousarray(pinhole_rays(H, d))
        for _ in range(2):
            assert L.render_aov_rays(s, hr.ctypes.data, host.ctypes.data, W, HGT, x, y, w, h) == 0, runtime.last_error()
        assert host.tobytes() == b.tobytes()
    finally:
        L.scene_destroy(s)


def test_aov_free_rays_equal_the_oracle_surface(H, L, orc_lib):
    import torch
    o, dirs = free_rays(H)
    frame = free_frame(o, dirs)
    frame[2, 3, 4:7] = 0.0                                                     # one inactive ray
    active = np.ones(N_FREE, bool); active[2 * FREE_W + 3] = False
    d = scenes.cornell_box(FREE_W, FREE_H, 1, integrator=api.kTerraIntegratorSimple, jitter=0.0)
    H.set_oracle_math(1)
    try:
        u = H.Unit("orc")
        sc = scenes.build_scene(u.L, d)
        obj, tri, point, surf = u.raycast(sc, o, dirs)
        u.L.scene_destroy(sc)
    finally:
        H.set_oracle_math(0)
    hit = (obj >= 0) & active
    assert 0.1 < hit.mean() < 0.95
    s = make_scene(L, d, split=1)
    try:
        aov = runtime.DeviceAov(FREE_W, FREE_H)
        runtime.render_aov_rays_device(L, s, to_device(frame), aov)
        torch.cuda.synchronize()
        a = aov.host().reshape(-1)
        assert (a["samples"] == 1).all() and not a["reserved"].any()
        assert np.array_equal(a["coverage"], hit.astype(np.float32))
        miss = ~hit
        assert not a["albedo"][miss].view(np.uint32).any() and not a["normal"][miss].view(np.uint32).any() and not a["depth"][miss].view(np.uint32).any()
        dobj, dtri, dpoint, dsurf = H.Unit("amd").raycast(s, o, dirs)
        assert np.array_equal(dobj, obj) and H.same_bits(dsurf[obj >= 0], surf[obj >= 0]) and H.same_bits(dpoint[obj >= 0], point[obj >= 0])
        su = api.TerraShadingSurface
        n_off, a_off = su.normal.offset // 4, su.attributes.offset // 4
        assert H.same_bits(a["normal"][hit], surf[hit, n_off:n_off + 3])
        assert H.same_bits(a["albedo"][hit], surf[hit, a_off:a_off + 3])         # the Cornell box is diffuse: TERRA_DIFFUSE_ALBEDO is attribute 0
        want = np.linalg.norm(point[hit].astype(np.float64) - o[hit].astype(np.float64), axis=1)
        # float32 sqrt of a three-term sum of squares of float32 differences: a handful of roundings of 2^-24 each, far inside 1e-6
        np.testing.assert_allclose(a["depth"][hit].astype(np.float64), want, rtol=1e-6, atol=0)
    finally:
        L.scene_destroy(s)


def test_denoise_on_a_ray_rendered_frame(H, L):
    import torch
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0)
    rays = to_device(pinhole_rays(H, d))
    s = make_scene(L, d)
    try:
        cam = scenes.camera_of(d)
        out = {}
        for door in ("camera", "rays"):
            fb, aov = runtime.DeviceFramebuffer(W, HGT), runtime.DeviceAov(W, HGT)
            if door == "camera":
                runtime.render_device(L, cam, s, fb); runtime.render_aov_device(L, cam, s, aov)
            else:
                runtime.render_rays_device(L, s, rays, fb); runtime.render_aov_rays_device(L, s, rays, aov)
            rad = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda"); pix = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda")
            runtime.denoise_device(L, s, fb, aov, 3, radiance=rad, pixels=pix)
            torch.cuda.synchronize()
            out[door] = (rad.cpu().numpy(), pix.cpu().numpy())
        assert out["camera"][0].max() > 0
        assert H.same_bits(out["camera"][0], out["rays"][0]) and H.same_bits(out["camera"][1], out["rays"][1])
    finally:
        L.scene_destroy(s)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing(H, L):
    import torch
    d = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorSimple, jitter=0.0)
    host_rays = np.ascontiguousarray(pinhole_rays(H, d))
    spare = torch.zeros(W * HGT * 8 + 8, dtype=torch.float32, device="cuda")
    spare[4:4 + W * HGT * 8] = to_device(host_rays).reshape(-1)
    rays = to_device(host_rays)
    assert rays.data_ptr() % 16 == 0
    misaligned = spare.data_ptr() + 16 - (spare.data_ptr() % 16) + 4            # 4 bytes past a 16-byte boundary, inside `spare`
    s = make_scene(L, d)
    fresh = L.scene_create()
    try:
        f = Frame(); aov = runtime.DeviceAov(W, HGT)
        hfb = api.Framebuffer(L, W, HGT); haov = np.zeros((HGT, W), runtime.AOV_DTYPE)
        P, R, A = f.fb.pixels.data_ptr(), f.fb.results.data_ptr(), aov.data.data_ptr()
        hr, hm = host_rays.ctypes.data, host_rays.ctypes.data + 4
        full = (0, 0, W, HGT)
        bad_rects = [(0, 0, 0, HGT), (0, 0, W, 0), (W - 4, 0, 5, 4), (0, HGT - 4, 4, 5)]

        def four(scene, dr, hrays, rect):
            x, y, w, h = rect
            return [lambda: L.render_rays_device(scene, dr, P, R, W, HGT, x, y, w, h, f.calls.data_ptr(), None),
                    lambda: L.render_aov_rays_device(scene, dr, A, W, HGT, x, y, w, h, None),
                    lambda: L.render_rays(scene, hrays, C.byref(hfb.fb), x, y, w, h),
                    lambda: L.render_aov_rays(scene, hrays, haov.ctypes.data, W, HGT, x, y, w, h)]
        cases = {"uncommitted": (ERR_NOT_COMMITTED, four(fresh, rays.data_ptr(), hr, full)),
                 "null rays": (ERR_BAD_ARGUMENT, four(s, None, None, full)),
                 "misaligned rays": (ERR_BAD_ARGUMENT, four(s, misaligned, hm, full))}
        for k, r in enumerate(bad_rects):
            cases[f"bad rectangle {k}"] = (ERR_BAD_ARGUMENT, four(s, rays.data_ptr(), hr, r))
        cases["null framebuffer"] = (ERR_BAD_ARGUMENT, [lambda: L.render_rays_device(s, rays.data_ptr(), None, R, W, HGT, 0, 0, W, HGT, None, None),
                                                        lambda: L.render_rays_device(s, rays.data_ptr(), P, None, W, HGT, 0, 0, W, HGT, None, None),
                                                        lambda: L.render_aov_rays_device(s, rays.data_ptr(), None, W, HGT, 0, 0, W, HGT, None),
                                                        lambda: L.render_rays(s, hr, None, 0, 0, W, HGT), lambda: L.render_aov_rays(s, hr, None, W, HGT, 0, 0, W, HGT)])
        for what, (status, fs) in cases.items():
            for k, call in enumerate(fs):
                L.clear_error()
                assert call() == status, (what, k)
                assert runtime.last_error() != "", (what, k)
        L.clear_error()
        pix, res, calls = f.host()
        assert not pix.view(np.uint32).any() and not res.view(np.uint8).any() and (calls == 0x5ca1ab1e).all()
        assert not aov.host().view(np.uint8).any() and not haov.view(np.uint8).any()
        assert not hfb.results.view(np.uint8).any() and not hfb.pixels.view(np.uint32).any()
        # the integrators that need a light keep their check
        dark = scenes.cornell_box(W, HGT, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0)
        for ob in dark.objects:
            ob.material.emissive = (0.0, 0.0, 0.0)
        sd = scenes.build_scene(L, dark)
        L.clear_error()
        assert L.render_rays_device(sd, rays.data_ptr(), P, R, W, HGT, 0, 0, W, HGT, None, None) == ERR_BAD_ARGUMENT and runtime.last_error() != ""
        L.clear_error()
        L.scene_destroy(sd)
        hfb.destroy()
    finally:
        L.scene_destroy(s); L.scene_destroy(fresh)


# ---- 7. runtime.radiance -------------------------------------------------------------------------------------------------------------------------------------------
def test_radiance_equals_a_hand_folded_call(H, L):
    import torch
    n = 300
    o, dirs = H.scene_rays(93, n)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    flat = np.zeros((n, 8), np.float32); flat[:, 0:3] = o; flat[:, 3] = np.inf; flat[:, 4:7] = dirs
    flat[7, 4:7] = 0.0                                                         # an inactive ray: mean 0
    d = scenes.cornell_box(256, 2, SPP, integrator=api.kTerraIntegratorDirect, jitter=0.0)
    s = make_scene(L, d)
    try:
        got = runtime.radiance(L, s, to_device(flat), batches=2)
        assert tuple(got.shape) == (n, 3) and got.dtype == torch.float32 and got.is_cuda
        frame = np.zeros((2, 256, 8), np.float32); frame.reshape(-1, 8)[:n] = flat
        fb = runtime.DeviceFramebuffer(256, 2)
        for _ in range(2):
            runtime.render_rays_device(L, s, to_device(frame), fb)
        torch.cuda.synchronize()
        res = fb.results_host().reshape(-1)
        assert (res["samples"] == 2 * SPP).all()
        want = (res["acc"] / res["samples"][:, None].astype(np.float32)).astype(np.float32)[:n]
        assert H.same_bits(got.cpu().numpy(), want) and want.max() > 0 and not got.cpu().numpy()[7].any()
        with pytest.raises(runtime.TerraAmdError):
            runtime.radiance(L, s, to_device(flat)[:, :7].contiguous())
    finally:
        L.scene_destroy(s)
