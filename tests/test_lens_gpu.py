"""Lens rendering on the GPU (include/terra_amd.h "Lens rendering"): terra_amd_render_lens* / terra_amd_render_aov_lens* / terra_amd_unit_lens_rays pinned by a chain
onto the ray door, which is itself pinned to the oracle and to the camera door:

  1. the generator (terra_amd_unit_lens_rays) equals a numpy restatement of the header's definition bit for bit, and its rays have the geometry the models promise;
  2. model 0 with lens_radius 0 through the lens door IS the camera door (pixels, results, draw counts, last_call), in all four template MODEs;
  3. a lens call cut into one-sample chunks equals as many 1 spp ray-door calls whose rays the host made with the generator from the chunks' stream-A draws;
  4. a chunk of several samples advances stream A as specified (r1 r2, the sampler integration's pair, then the lens pair -- and no lens pair without a lens);
  5. the lens AOV pass equals the ray-door AOV pass of the same rays; 6. host form = device form, and the camera_limit rule; 7. the denoiser and the moments
  accept lens frames; 8. terra_headless --camera-model.

Frames are 48 x 40 (three by three 16 x 16 blocks, the last column and row partial), whole and as the rectangle (5, 3, 37, 30)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, HGT = 48, 40
RECT = (5, 3, 37, 30)
RECTS = [None, RECT]
CALL_REPLICA = 1
LIGHT3 = [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis]
PI, PI2, PI4 = (np.array([b], np.uint32).view(F)[0] for b in (0x40490FDB, 0x3FC90FDB, 0x3F490FDB))


def lens_of(model, lens_radius=0.0, focus_distance=0.0, ortho_height=0.0, fisheye_fov=0.0):
    l = api.Lens()
    l.model, l.lens_radius, l.focus_distance, l.ortho_height, l.fisheye_fov = model, lens_radius, focus_distance, ortho_height, fisheye_fov
    return l


THIN = dict(model=0, lens_radius=0.15, focus_distance=3.0)
LENSES = {"thin": THIN, "ortho": dict(model=1, ortho_height=2.5), "equirect": dict(model=2), "fisheye": dict(model=3, fisheye_fov=200.0)}


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    assert torch.cuda.is_available()
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def make_scene(L, d, tree_mode=None, split=1):
    L.clear_error()
    s = scenes.build_scene(L, d, tree_mode=tree_mode)
    assert runtime.last_error() == "", runtime.last_error()
    runtime.check(L.set_sample_split(s, split))
    return s


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


def last_call(L, s):
    ti = runtime.TraversalInfo()
    runtime.check(L.traversal_info(s, C.byref(ti)))
    return ti.last_call


def all_pixels(w=W, h=HGT):
    return np.array([(x, y) for y in range(h) for x in range(w)], np.uint32)


# ---- 1. the generator ------------------------------------------------------------------------------------------------------------------------------------------
def dev_math(L, fn, x):
    """terra_amd_unit_math: fn 0 = the device's sinf, 1 = its cosf"""
    x = np.ascontiguousarray(x, F)
    out = np.zeros_like(x)
    rc = L.fn("terra_amd_unit_math", C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])(fn, len(x), x.ctypes.data, None, out.ctypes.data)
    assert rc == 0, runtime.last_error()
    return out


def camera_frame(cam, w, h):
    """fill_camera in float32, as tests/test_temporal.py restates it: X, Y, Z (the columns of cam_rot), tan of the half angle, aspect, position"""
    def f3(v):
        return np.array([v.x, v.y, v.z], F)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)

    def norm(a):
        l = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        return np.array([a[0] / l, a[1] / l, a[2] / l], F)
    Z = norm(f3(cam.direction)); X = norm(cross(f3(cam.up), Z)); Y = cross(Z, X)
    t = F(math.tan(float((F(cam.fov) * F(0.0174533)) / F(2))))
    return X, Y, Z, t, F(w) / F(h), f3(cam.position)


def restate(L, cam, lens, w, h, xy, jitter, r4):
    """the header's "ray of a sample" in numpy float32, every operation in the order written; sinf / cosf are the device's. Returns (origins, directions) [n, 3]"""
    X, Y, Z, t, aspect, pos = camera_frame(cam, w, h)
    j = F(jitter)
    r1, r2, l1, l2 = (np.ascontiguousarray(r4[:, k], F) for k in range(4))
    n = len(xy)
    with np.errstate(all="ignore"):
        dx = -j + F(2) * r1 * j
        dy = -j + F(2) * r2 * j
        ndc_x = (xy[:, 0].astype(F) + F(0.5) + dx) / F(w)
        ndc_y = (xy[:, 1].astype(F) + F(0.5) + dy) / F(h)
        sx = F(2) * ndc_x - F(1)
        sy = F(1) - F(2) * ndc_y

        def R(v):
            return np.stack([X[k] * v[0] + Y[k] * v[1] + Z[k] * v[2] for k in range(3)], axis=1).astype(F)

        def normalize(v):
            ln = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            return [v[0] / ln, v[1] / ln, v[2] / ln]

        def shifted(Lx, Ly):
            return np.stack([pos[k] + (X[k] * Lx + Y[k] * Ly) for k in range(3)], axis=1).astype(F)
        here = np.tile(pos, (n, 1)).astype(F)
        one, zero = np.ones(n, F), np.zeros(n, F)
        if lens.model == 0:
            d = normalize([sx * aspect * t, sy * t, one])
            if not lens.lens_radius > 0:
                return here, R(d)
            a, b = F(2) * l1 - F(1), F(2) * l2 - F(1)
            origin = (a == 0) & (b == 0)
            wide = np.abs(a) > np.abs(b)
            r = np.where(wide, a, b)
            phi = np.where(wide, PI4 * (b / a), PI2 - PI4 * (a / b))
            phi = np.where(origin, F(0), phi).astype(F)
            u = np.where(origin, F(0), r * dev_math(L, 1, phi)).astype(F)
            v = np.where(origin, F(0), r * dev_math(L, 0, phi)).astype(F)
            Lx, Ly = F(lens.lens_radius) * u, F(lens.lens_radius) * v
            tt = F(lens.focus_distance) / d[2]
            Fp = [d[0] * tt, d[1] * tt, d[2] * tt]
            return shifted(Lx, Ly), R(normalize([Fp[0] - Lx, Fp[1] - Ly, Fp[2]]))
        if lens.model == 1:
            half = F(lens.ortho_height) * F(0.5)
            return shifted((sx * aspect) * half, sy * half), R([zero, zero, one])
        if lens.model == 2:
            phi, theta = sx * PI, sy * PI2
            ct, st = dev_math(L, 1, theta), dev_math(L, 0, theta)
            return here, R([ct * dev_math(L, 0, phi), st, ct * dev_math(L, 1, phi)])
        hh = (F(lens.fisheye_fov) * F(0.0174533)) / F(2)
        ux, uy = sx * aspect, sy
        rr = np.sqrt(ux * ux + uy * uy)
        theta = rr * hh
        s_, c_ = dev_math(L, 0, theta), dev_math(L, 1, theta)
        centre = rr == 0
        safe = np.where(centre, F(1), rr)
        return here, R([np.where(centre, F(0), (s_ * ux) / safe).astype(F), np.where(centre, F(0), (s_ * uy) / safe).astype(F), np.where(centre, F(1), c_).astype(F)])


def tilted_camera():
    cam = api.TerraCamera()
    cam.position = api.f3((0.3, 1.1, -3.2)); cam.direction = api.f3((-0.2, -0.1, 1.0)); cam.up = api.f3((0.1, 1.0, 0.05)); cam.fov = 52.0
    return cam


# the lens pairs that reach every branch of the concentric map: a = b = 0; |a| = |b| (both signs); a = 0; b = 0; then the interior
SPECIAL_PAIRS = [(0.5, 0.5), (0.75, 0.75), (0.25, 0.75), (0.5, 0.3), (0.3, 0.5)]


def generator_inputs(H, w, h, full):
    """(xy, r4): every pixel (or the corners) of a w x h frame with random draws, the special lens pairs on the first pixels, and one sample aimed at the centre"""
    xy = all_pixels(w, h) if full else np.array([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)], np.uint32)
    r4 = H.rng(7 + w).uniform(size=(len(xy), 4)).astype(F)
    for k, pair in enumerate(SPECIAL_PAIRS[:len(xy)]):
        r4[k, 2:4] = pair
    if full:
        centre = (h // 2) * w + w // 2          # with jitter 0.5 and r1 = r2 = 0 the sample of pixel (w / 2, h / 2) is the frame's centre: sx = sy = 0
        r4[centre, 0:2] = 0.0
    return xy, r4


@pytest.mark.parametrize("name", list(LENSES) + ["pinhole"])
def test_generator_equals_the_numpy_restatement(H, L, name):
    cam = tilted_camera()
    lens = lens_of(**LENSES[name]) if name != "pinhole" else lens_of(0)
    total = 0
    for (w, h, full) in ((W, HGT, True), (1920, 1080, False)):
        for jitter in (0.0, 0.5):
            xy, r4 = generator_inputs(H, w, h, full)
            got = runtime.lens_rays(L, cam, lens, w, h, xy, jitter, r4)
            o, d = restate(L, cam, lens, w, h, xy, jitter, r4)
            assert H.same_bits(got["origin"], o), (name, w, jitter)
            assert H.same_bits(got["direction"], d), (name, w, jitter)
            assert (got["tmax"] == np.finfo(F).max).all() and not got["reserved"].view(np.uint32).any()
            total += len(xy)
            if name == "fisheye" and full and jitter == 0.5:
                assert H.same_bits(got["direction"][(h // 2) * w + w // 2], camera_frame(cam, w, h)[2])          # rr == 0: the camera axis
    assert total == 2 * (W * HGT + 4)          # 3,848 inputs per model


def test_generator_geometry(H, L):
    cam = tilted_camera()
    X, Y, Z, t, aspect, pos = (np.asarray(v, np.float64) for v in camera_frame(cam, W, HGT))
    xy = all_pixels()
    n = len(xy)
    # model 0: with the jitter fixed, all lens samples of a pixel meet the plane z_cam = focus_distance in one point; origins lie on the lens
    thin = lens_of(**THIN)
    pairs = SPECIAL_PAIRS + [(0.1, 0.9), (0.97, 0.4)]
    points = []
    for pair in pairs:
        r4 = np.zeros((n, 4), F); r4[:, 2:4] = pair
        rays = runtime.lens_rays(L, cam, thin, W, HGT, xy, 0.0, r4)
        o = rays["origin"].astype(np.float64) - pos; d = rays["direction"].astype(np.float64)
        oc = np.stack([o @ X, o @ Y, o @ Z], axis=1); dc = np.stack([d @ X, d @ Y, d @ Z], axis=1)
        # (float32 origins around a position of magnitude 3: half an ulp, 1.2e-7, per axis)
        assert (np.linalg.norm(o, axis=1) <= THIN["lens_radius"] + 1e-6).all()
        assert np.abs(oc[:, 2]).max() <= 1e-6                                      # ... in the lens plane
        tt = (THIN["focus_distance"] - oc[:, 2]) / dc[:, 2]
        points.append(oc + dc * tt[:, None])
    spread = np.abs(np.array(points) - points[0]).max()
    print(f"thin lens: largest distance between the focus-plane points of one pixel's lens samples {spread:.3g} (bound {1e-4 * THIN['focus_distance']:.3g})")
    assert spread <= 1e-4 * THIN["focus_distance"]
    r4 = H.rng(3).uniform(size=(n, 4)).astype(F)
    ortho = runtime.lens_rays(L, cam, lens_of(**LENSES["ortho"]), W, HGT, xy, 0.5, r4)
    assert (ortho["direction"].view(np.uint32) == ortho["direction"].view(np.uint32)[0]).all()          # model 1: one direction
    assert len(np.unique(ortho["origin"], axis=0)) == n
    for name in ("equirect", "fisheye"):
        d = runtime.lens_rays(L, cam, lens_of(**LENSES[name]), W, HGT, xy, 0.5, r4)["direction"].astype(np.float64)
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 1e-6, name


# ---- 2. the pinhole through the lens door is the camera door ---------------------------------------------------------------------------------------------------
SPP8 = 8


def cornell(integrator, spp=SPP8, **kw):
    return scenes.cornell_box(W, HGT, spp, integrator=integrator, jitter=0.5, **kw)


def far_hall(integrator, spp=SPP8):
    from tools.scaled_hall import scaled
    return scaled(scenes.sponza_hall(W, HGT, spp, integrator=integrator, jitter=0.5, detail=0.25), 100.0)


# (scene, tree mode, TerraAmdTraversalInfo::last_call of the launch): template MODE 0, 2, 1 and 3
PINHOLE_SCENES = {"cornell-replica": (cornell, 0, 1), "cornell-fast": (cornell, 1, 3), "cornell-auto": (cornell, 2, 2), "hall-x100": (far_hall, None, 4)}


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("integrator", LIGHT3)
@pytest.mark.parametrize("scene", list(PINHOLE_SCENES))
def test_pinhole_lens_is_the_camera_door(H, L, scene, integrator, split):
    make, tree_mode, want_call = PINHOLE_SCENES[scene]
    d = make(integrator)
    s = make_scene(L, d, tree_mode=tree_mode, split=split)
    try:
        cam, lens = scenes.camera_of(d), lens_of(0)
        for rect in RECTS:
            fc, fl = Frame(), Frame()
            runtime.render_device(L, cam, s, fc.fb, rect=rect, rand_calls=fc.calls)
            call_cam = last_call(L, s)
            runtime.render_lens_device(L, cam, lens, s, fl.fb, rect=rect, rand_calls=fl.calls)
            call_lens = last_call(L, s)
            assert runtime.empty_skip_info(L, s)[0] == 0                      # a lens launch never skips
            a, b = fc.host(), fl.host()
            x, y, w, h = rect or (0, 0, W, HGT)
            assert (a[1]["samples"][y:y + h, x:x + w] == SPP8).all() and a[1]["samples"].sum() == SPP8 * w * h and a[1]["acc"].max() > 0
            assert_same_frames(H, a, b, (scene, integrator, split, rect))
            assert call_cam == call_lens == want_call, (call_cam, call_lens)
    finally:
        L.scene_destroy(s)


# ---- 3. - 5. chunks against the ray door -----------------------------------------------------------------------------------------------------------------------
def stream_a_draws(H, L, prior, n_draws):
    """[HGT, W, n_draws]: the first draws of every pixel's stream A keyed (frame seed + pixel index, `prior` samples so far)"""
    pix = np.arange(W * HGT, dtype=np.uint64)
    k = np.full(W * HGT, prior, np.uint64)
    out = np.zeros((W * HGT, 3), np.uint64)
    rc = L.fn("terra_amd_unit_stream_keys", C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])(scenes.FRAME_SEED, pix.ctypes.data, k.ctypes.data, len(pix), out.ctypes.data)
    assert rc == 0, runtime.last_error()
    return H.Unit("amd").pcg(out[:, 0].astype(np.uint32), n_draws).reshape(HGT, W, n_draws)


def rays_of(L, cam, lens, jitter, r4):
    """the generator's rays of every pixel of the frame for the draws r4 [HGT, W, 4], as the ray door takes them"""
    rays = runtime.lens_rays(L, cam, lens, W, HGT, all_pixels(), jitter, r4.reshape(-1, 4))
    return to_device(rays.view(F).reshape(HGT, W, 8))


@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("tree_mode", [2, 1], ids=["mode1", "mode2"])
@pytest.mark.parametrize("name", list(LENSES))
def test_one_sample_chunks_equal_the_ray_door(H, L, name, tree_mode, rect):
    lens = lens_of(**LENSES[name])
    d8, d1 = cornell(api.kTerraIntegratorDirect, 8), cornell(api.kTerraIntegratorDirect, 1)
    cam = scenes.camera_of(d8)
    s8, s1 = make_scene(L, d8, tree_mode=tree_mode, split=8), make_scene(L, d1, tree_mode=tree_mode, split=1)
    try:
        fl, fr = Frame(), Frame()
        runtime.render_lens_device(L, cam, lens, s8, fl.fb, rect=rect, rand_calls=fl.calls)
        call_lens = last_call(L, s8)
        import torch
        total = torch.zeros_like(fr.calls)
        for chunk in range(8):
            rays = rays_of(L, cam, lens, d8.jitter, stream_a_draws(H, L, chunk, 4))
            runtime.render_rays_device(L, s1, rays, fr.fb, rect=rect, rand_calls=fr.calls)
            x, y, w, h = rect or (0, 0, W, HGT)
            total.view(HGT, W)[y:y + h, x:x + w] += fr.calls.view(HGT, W)[y:y + h, x:x + w]
        assert last_call(L, s1) == call_lens == (2 if tree_mode == 2 else 3)
        (pl, rl, cl), (pr, rr, _) = fl.host(), fr.host()
        x, y, w, h = rect or (0, 0, W, HGT)
        inside = np.zeros((HGT, W), bool); inside[y:y + h, x:x + w] = True
        assert (rl["samples"][inside] == 8).all() and rl["acc"].max() > 0
        assert rl.tobytes() == rr.tobytes() and H.same_bits(pl, pr), name
        assert np.array_equal(cl[inside], total.cpu().numpy().reshape(HGT, W)[inside]) and (cl[~inside] == 0x5ca1ab1e).all()
    finally:
        L.scene_destroy(s8); L.scene_destroy(s1)


@pytest.mark.parametrize("stratified", [False, True], ids=["random", "stratified"])
@pytest.mark.parametrize("radius", [THIN["lens_radius"], 0.0], ids=["lens", "no-lens"])
@pytest.mark.parametrize("integrator", [api.kTerraIntegratorDebugDepth, api.kTerraIntegratorDebugNormals], ids=["depth", "normals"])
def test_chunk_of_four_samples_advances_stream_a(H, L, integrator, radius, stratified):
    """spp 4 in one chunk: sample s of a pixel takes r1, r2, then the stratified sampler's two offsets (sampling_device.h stratified_next_pair / integrators_device.h
    sampler_pair_draw: two trng_a_float of the pixel's stream A per sample; Halton and no sampler draw none), then -- only with a lens -- l1, l2. So with D draws per
    sample, r = draws D s, D s + 1 and the lens pair = the last two of the sample's D. The debug integrators' value depends on the primary ray alone."""
    lens = lens_of(0, radius, THIN["focus_distance"] if radius else 0.0)
    kw = dict(sampling=api.kTerraSamplingMethodStratified, strata=2, sampler_integration=True) if stratified else {}
    d4, d1 = cornell(integrator, 4, **kw), cornell(integrator, 1)
    per_sample = 2 + (2 if stratified else 0) + (2 if radius else 0)
    cam = scenes.camera_of(d4)
    s4, s1 = make_scene(L, d4, split=1), make_scene(L, d1, split=1)
    try:
        fl, fr = Frame(), Frame()
        runtime.render_lens_device(L, cam, lens, s4, fl.fb, rect=RECT)
        draws = stream_a_draws(H, L, 0, 4 * per_sample)
        for smp in range(4):
            at = smp * per_sample
            r4 = np.zeros((HGT, W, 4), F)
            r4[..., 0:2] = draws[..., at:at + 2]
            if radius:
                r4[..., 2:4] = draws[..., at + per_sample - 2:at + per_sample]
            runtime.render_rays_device(L, s1, rays_of(L, cam, lens, d4.jitter, r4), fr.fb, rect=RECT)
        (pl, rl, _), (pr, rr, _) = fl.host(), fr.host()
        assert rl["samples"].sum() == 4 * RECT[2] * RECT[3] and rl["acc"].max() > 0
        assert rl.tobytes() == rr.tobytes() and H.same_bits(pl, pr)
    finally:
        L.scene_destroy(s4); L.scene_destroy(s1)


@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("name", list(LENSES))
def test_aov_equals_the_ray_door_aov(H, L, name, rect):
    import torch
    lens = lens_of(**LENSES[name])
    d8, d1 = cornell(api.kTerraIntegratorSimple, 8), cornell(api.kTerraIntegratorSimple, 1)
    cam = scenes.camera_of(d8)
    s8, s1 = make_scene(L, d8, split=8), make_scene(L, d1, split=1)
    try:
        al, ar = runtime.DeviceAov(W, HGT), runtime.DeviceAov(W, HGT)
        runtime.render_aov_lens_device(L, cam, lens, s8, al, rect=rect)
        for chunk in range(8):
            runtime.render_aov_rays_device(L, s1, rays_of(L, cam, lens, d8.jitter, stream_a_draws(H, L, chunk, 4)), ar, rect=rect)
        torch.cuda.synchronize()
        a, b = al.host(), ar.host()
        x, y, w, h = rect or (0, 0, W, HGT)
        assert (a["samples"][y:y + h, x:x + w] == 8).all() and a["samples"].sum() == 8 * w * h and a["coverage"].max() > 0
        assert a.tobytes() == b.tobytes(), name
        # the host form, frame-indexed
        host = np.zeros((HGT, W), runtime.AOV_DTYPE)
        assert L.render_aov_lens(C.byref(cam), C.byref(lens), s8, host.ctypes.data, W, HGT, x, y, w, h) == 0, runtime.last_error()
        assert host.tobytes() == a.tobytes()
    finally:
        L.scene_destroy(s8); L.scene_destroy(s1)


# ---- 6. host form, camera_limit ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", RECTS, ids=["frame", "rect"])
@pytest.mark.parametrize("name", ["thin", "fisheye"])
def test_host_form_equals_device_form(H, L, name, rect):
    lens = lens_of(**LENSES[name])
    d = cornell(api.kTerraIntegratorDirect, 4)
    s = make_scene(L, d, split=2)
    try:
        cam = scenes.camera_of(d)
        f = Frame()
        fb = api.Framebuffer(L, W, HGT)
        x, y, w, h = rect or (0, 0, W, HGT)
        for _ in range(2):
            runtime.render_lens_device(L, cam, lens, s, f.fb, rect=rect)
            L.clear_error()
            assert L.render_lens(C.byref(cam), C.byref(lens), s, C.byref(fb.fb), x, y, w, h) == 0, runtime.last_error()
        pix, res, _ = f.host()
        assert fb.results.tobytes() == res.tobytes() and H.same_bits(fb.pixels, pix)
        assert res["samples"].sum() == 2 * 4 * w * h and res["acc"].max() > 0
        fb.destroy()
    finally:
        L.scene_destroy(s)


def test_beyond_camera_limit_runs_the_replica(H, L):
    """an orthographic camera sees the box the same from any distance: from within camera_limit the call keeps the commit's traversal, from where |position| + e
    passes it -- by the position alone, or only by the film window's half diagonal e -- it runs the replica, and the image is tree mode 0's"""
    d = cornell(api.kTerraIntegratorDirect, 4)
    s, s0 = make_scene(L, d, split=2), make_scene(L, d, tree_mode=0, split=2)
    try:
        ti = runtime.TraversalInfo(); runtime.check(L.traversal_info(s, C.byref(ti)))
        limit = float(ti.camera_limit)
        assert ti.leaf_cull == 1 and limit > 4
        lens = lens_of(1, ortho_height=2.5)
        e = 1.25 * math.sqrt((W / HGT) ** 2 + 1)
        for z, replica in ((-3.4, False), (-(limit - 0.5 * e), True), (-(limit + 1.0), True)):
            cam = scenes.camera_of(d); cam.position = api.f3((0.0, 1.0, z))
            f, f0 = Frame(), Frame()
            runtime.render_lens_device(L, cam, lens, s, f.fb, rand_calls=f.calls)
            assert (last_call(L, s) == CALL_REPLICA) == replica, z
            runtime.render_lens_device(L, cam, lens, s0, f0.fb, rand_calls=f0.calls)
            assert last_call(L, s0) == CALL_REPLICA
            a, b = f.host(), f0.host()
            assert a[1]["acc"].max() > 0
            assert_same_frames(H, a, b, z)
            # the host form decides alike
            fb = api.Framebuffer(L, W, HGT)
            assert L.render_lens(C.byref(cam), C.byref(lens), s, C.byref(fb.fb), 0, 0, W, HGT) == 0, runtime.last_error()
            assert (last_call(L, s) == CALL_REPLICA) == replica
            assert fb.results.tobytes() == a[1].tobytes()
            fb.destroy()
    finally:
        L.scene_destroy(s); L.scene_destroy(s0)


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------------------------------------------
def test_denoiser_and_moments_take_a_lens_frame(H, L):
    import torch
    d = cornell(api.kTerraIntegratorDirect, 4)
    lens = lens_of(**THIN)
    s = make_scene(L, d, split=2)
    try:
        cam = scenes.camera_of(d)
        fb, aov, mom = runtime.DeviceFramebuffer(W, HGT), runtime.DeviceAov(W, HGT), runtime.DeviceMoments(W, HGT)
        for _ in range(2):
            runtime.render_lens_device(L, cam, lens, s, fb); runtime.render_aov_lens_device(L, cam, lens, s, aov)
            runtime.accumulate_moments_device(L, s, fb, mom)
        rad = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda"); pix = torch.zeros(W * HGT * 3, dtype=torch.float32, device="cuda")
        runtime.denoise_device(L, s, fb, aov, 3, radiance=rad, pixels=pix)
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        r = rad.cpu().numpy()
        assert np.isfinite(r).all() and r.max() > 0 and np.isfinite(pix.cpu().numpy()).all()
        assert (aov.host()["samples"] == 8).all() and (fb.results_host()["samples"] == 8).all()
        assert mom.data.cpu().numpy().any()
    finally:
        L.scene_destroy(s)


# ---- 8. the tool -------------------------------------------------------------------------------------------------------------------------------------------------
def test_headless_camera_models(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "amd")
    obj = tmp_path / "c.obj"
    write_obj(scenes.cornell_phong(W, HGT, 1), obj, mirror_z=True)
    args = ["--width", str(W), "--height", str(HGT), "--integrator", "direct", "--tonemap", "none", "--normals", "file", "--spp", "4", "--sample-split", "2", "--seed", "77"]

    def run(out, extra):
        return subprocess.run([str(exe), str(obj), str(tmp_path / out)] + args + extra, capture_output=True, text=True, timeout=600)
    for out, extra in (("plain.pfm", []), ("zero.pfm", ["--camera-model", "thinlens", "--aperture", "0"]), ("dof.pfm", ["--camera-model", "thinlens", "--aperture", "0.05", "--focus", "3.5"]),
                       ("fish.pfm", ["--camera-model", "fisheye", "--fisheye-fov", "170", "--aov", str(tmp_path / "fish"), "--denoise", "1", "--passes", "2"])):
        r = run(out, extra)
        assert r.returncode == 0 and "libterra_amd.so" not in r.stderr, r.stderr
    assert (tmp_path / "zero.pfm").read_bytes() == (tmp_path / "plain.pfm").read_bytes()
    plain, dof, fish = (read_pfm(tmp_path / n) for n in ("plain.pfm", "dof.pfm", "fish.pfm"))
    assert not np.array_equal(plain, dof) and dof.max() > 0 and np.isfinite(dof).all()
    assert not np.array_equal(plain, fish) and fish.max() > 0 and (tmp_path / "fish.depth.pfm").exists()
    r = run("t.pfm", ["--camera-model", "ortho", "--frames", "2", "--temporal", "0.25", "--denoise", "1"])
    assert r.returncode != 0 and "reprojection is defined for the pinhole camera only" in r.stderr
    assert not (tmp_path / "t.pfm").exists() and not (tmp_path / "t.0000.pfm").exists()
