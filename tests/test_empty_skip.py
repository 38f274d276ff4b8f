"""terra_amd_set_empty_skip: job-ordered launches prove 16x16 pixel blocks empty before the launch (csrc/empty_proof.h) and neither key, queue nor
trace them; the resolve kernel gives their pixels the +0 sums the render would have stored. What a camera ray that misses contributes is the reference's: nothing
(src/Terra.c:1056, the environment term is commented out), and the pixel still counts its samples (src/Terra.c:570-572). So the framebuffer must be the same bit for
bit with the switch on and off -- checked here on whole frames, rectangles, shards, accumulation, at the edges of the proof, on degenerate views, under every condition
that turns the class off, and on random triangle soups; the predicate itself is checked on the host against a dense grid of double-precision rays."""
import ctypes as C
import math

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

gpu = pytest.mark.gpu
WIDE = dict(camera_position=(0.0, 1.0, -7.0))         # far enough back that a good share of a small frame's blocks see nothing


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


@pytest.fixture(scope="module")
def G(L):
    assert L.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return L


# ---- the predicate on the host ------------------------------------------------------------------------------------------------

def proof(L, rot, pos, thf, aspect, jitter, fb_w, fb_h, x0, y0, x1, y1, tris):
    rot = np.ascontiguousarray(rot, dtype=np.float32).reshape(9); pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(3)
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    return L.empty_proof(rot.ctypes.data, pos.ctypes.data, float(thf), float(aspect), float(jitter), fb_w, fb_h, x0, y0, x1, y1, tris.ctypes.data, len(tris))


def random_rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rays_hit(o, dirs, tris):
    """Moeller-Trumbore in double precision, no epsilons: True where some ray dirs[i] from o meets some triangle at t > 0 (edges included)"""
    a, b, c = tris[:, 0][None], tris[:, 1][None], tris[:, 2][None]
    d = dirs[:, None, :]
    e1, e2 = b - a, c - a
    h = np.cross(d, e2)
    det = (e1 * h).sum(-1)
    ok = det != 0
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    s = o[None, None, :] - a
    u = inv * (s * h).sum(-1)
    q = np.cross(s, e1)
    v = inv * (d * q).sum(-1)
    t = inv * (e2 * q).sum(-1)
    return (ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)).any()


def footprint_dirs(rot, thf, aspect, jitter, fb_w, fb_h, x0, y0, x1, y1, n=41):
    """world directions over the block's own footprint (pixels +- jitter, no guard), a dense grid with the borders included"""
    X = np.linspace(x0 + 0.5 - jitter, x1 - 1 + 0.5 + jitter, n); Y = np.linspace(y0 + 0.5 - jitter, y1 - 1 + 0.5 + jitter, n)
    X, Y = np.meshgrid(X, Y)
    fx = (2 * X / fb_w - 1) * aspect * thf; fy = (1 - 2 * Y / fb_h) * thf
    cam = np.stack([fx, fy, np.ones_like(fx)], -1).reshape(-1, 3)
    return cam @ np.asarray(rot, dtype=np.float64).T


def test_predicate_is_sound_against_dense_double_rays(L):
    rng = np.random.default_rng(20260417)
    proved = near = 0
    for case in range(400):
        rot = random_rotation(rng).astype(np.float32); pos = rng.uniform(-3, 3, 3).astype(np.float32)
        fov = rng.uniform(20, 100); thf = np.float32(math.tan(math.radians(fov) / 2)); fb_w, fb_h = int(rng.integers(32, 200)), int(rng.integers(32, 200))
        aspect = np.float32(fb_w / fb_h); jitter = np.float32(rng.choice([0.0, 0.5, 0.5, 1.5]))
        x0, y0 = int(rng.integers(0, fb_w - 1)), int(rng.integers(0, fb_h - 1)); x1, y1 = min(x0 + 16, fb_w), min(y0 + 16, fb_h)
        R = rot.astype(np.float64)
        if case % 2:      # near-tangent: a triangle whose nearest vertex sits a fraction of a pixel either side of the guarded footprint's border
            edge = rng.integers(0, 4); off = rng.uniform(-0.6, 0.6)
            gx = {0: x0 + 0.5 - jitter - 1 - off, 1: x1 - 0.5 + jitter + 1 + off}.get(int(edge), rng.uniform(x0, x1))
            gy = {2: y0 + 0.5 - jitter - 1 - off, 3: y1 - 0.5 + jitter + 1 + off}.get(int(edge), rng.uniform(y0, y1))
            away = np.array([[-1, 0], [1, 0], [0, -1], [0, 1]][int(edge)], dtype=np.float64)
            pts2 = np.array([[gx, gy], [gx, gy] + away * rng.uniform(1, 30) + rng.normal(size=2), [gx, gy] + away * rng.uniform(1, 30) + rng.normal(size=2) * 5])
            z = rng.uniform(0.5, 8, 3)
            cam = np.stack([(2 * pts2[:, 0] / fb_w - 1) * float(aspect) * float(thf) * z, (1 - 2 * pts2[:, 1] / fb_h) * float(thf) * z, z], -1)
            tris = (cam @ R.T + pos.astype(np.float64))[None].astype(np.float32)
            near += 1
        else:
            centre = pos + rng.normal(size=3) * 4
            tris = (centre[None, None, :] + rng.normal(size=(int(rng.integers(1, 6)), 3, 3)) * rng.uniform(0.05, 2)).astype(np.float32)
        if proof(L, rot, pos, thf, aspect, jitter, fb_w, fb_h, x0, y0, x1, y1, tris):
            proved += 1
            dirs = footprint_dirs(R, float(thf), float(aspect), float(jitter), fb_w, fb_h, x0, y0, x1, y1)
            assert not rays_hit(pos.astype(np.float64), dirs, tris.astype(np.float64)), case
    assert proved > 60 and near == 200, (proved, near)          # (the inputs really exercise both answers)


def test_predicate_refuses_what_it_must(L):
    rot = np.eye(3, dtype=np.float32); pos = np.zeros(3, dtype=np.float32)
    behind = np.array([[[-1, -1, -5], [1, -1, -5], [0, 1, -5]]], dtype=np.float32)        # wholly behind the camera: proved for any block
    args = dict(rot=rot, pos=pos, thf=0.5, aspect=1.5, jitter=0.5, fb_w=96, fb_h=64, x0=32, y0=16, x1=48, y1=32, tris=behind)
    assert proof(L, **args) == 1
    assert proof(L, **{**args, "tris": np.array([[[-1, -1, 5], [1, -1, 5], [0, 1, 5]]], dtype=np.float32)}) == 0      # the same triangle in front of it
    for bad in (np.nan, np.inf, -np.inf):
        assert proof(L, **{**args, "thf": bad}) == 0
        assert proof(L, **{**args, "aspect": bad}) == 0
        assert proof(L, **{**args, "jitter": bad}) == 0
        r = rot.copy(); r[1, 1] = bad
        assert proof(L, **{**args, "rot": r}) == 0
        q = pos.copy(); q[2] = bad
        assert proof(L, **{**args, "pos": q}) == 0
        t = behind.copy(); t[0, 1, 0] = bad
        assert proof(L, **{**args, "tris": t}) == 0
    assert proof(L, **{**args, "thf": 0.0}) == 0                  # degenerate footprints: no field of view, no pixels, no frame
    assert proof(L, **{**args, "x1": 32}) == 0 and proof(L, **{**args, "y1": 16}) == 0
    assert proof(L, **{**args, "fb_w": 0}) == 0
    assert proof(L, **{**args, "rot": np.zeros((3, 3), dtype=np.float32)}) == 0
    assert proof(L, **{**args, "tris": np.zeros((1, 3, 3), dtype=np.float32) - 5}) == 0      # a zero-area triangle proves nothing


# ---- on the device -------------------------------------------------------------------------------------------------------------

def dev(L, d, skip, order=None, split=1, passes=1, shard=None, rect=None, counters=False, want_calls=False):
    import torch
    scene = scenes.build_scene(L, d, counters=counters)
    assert L.get_empty_skip(scene) == 1                      # the default
    assert L.set_empty_skip(scene, int(skip)) == 0 and L.get_empty_skip(scene) == int(skip)
    if order is not None:
        assert L.set_job_order(scene, order) == 0
    assert L.set_sample_split(scene, split) == 0
    fb = runtime.DeviceFramebuffer(d.width, d.height); cam = scenes.camera_of(d)
    rc = torch.zeros(d.width * d.height, dtype=torch.int32, device="cuda") if want_calls else None
    for _ in range(passes):
        if shard:
            runtime.render_device_sharded(L, cam, scene, fb, *shard)
        else:
            runtime.render_device(L, cam, scene, fb, rect, rc)
    torch.cuda.synchronize()
    assert runtime.last_error() == ""
    info = runtime.empty_skip_info(L, scene)
    res = fb.results_host()
    stats = None
    if counters:
        st = runtime.Stats(); runtime.check(L.get_stats(scene, C.byref(st))); stats = st.as_dict()
    out = dict(pixels=fb.pixels_host().copy(), acc=res["acc"].copy(), samples=res["samples"].copy(), calls=rc.cpu().numpy().copy() if want_calls else None, info=info, stats=stats)
    L.scene_destroy(scene)
    return out


def same_fb(a, b):
    return (np.array_equal(a["acc"].view(np.uint32), b["acc"].view(np.uint32)) and np.array_equal(a["samples"], b["samples"])
            and np.array_equal(a["pixels"].view(np.uint32), b["pixels"].view(np.uint32)) and (a["calls"] is None or np.array_equal(a["calls"], b["calls"])))


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis])
@pytest.mark.parametrize("split", [1, 2, 0])
def test_bit_equality_on_the_cornell_frame(G, integ, split):
    # 20 x 16 = 320 pixel blocks: job-ordered by default
    mk = lambda: scenes.cornell_box(320, 256, 8, integrator=integ)
    on = dev(G, mk(), 1, split=split, passes=2)             # two successive calls into the same framebuffer
    off = dev(G, mk(), 0, split=split, passes=2)
    assert same_fb(on, off), (integ, split)
    assert (on["samples"] == 16).all()
    proved, total = on["info"]
    assert total == 320 and 0 < proved < total, on["info"]
    assert off["info"] == (0, 320)


@gpu
def test_skipped_frame_equals_the_oracle(H, G, orc_lib):
    mk = lambda: scenes.cornell_box(320, 256, 8, integrator=api.kTerraIntegratorSimple)
    H.set_oracle_math(1)
    try:
        want = H.Unit("orc").render_pixels(mk(), passes=1, want_calls=False)
    finally:
        H.set_oracle_math(0)
    got = dev(G, mk(), 1)
    assert got["info"][0] > 0
    assert np.array_equal(got["acc"].view(np.uint32), np.ascontiguousarray(want["acc"]).view(np.uint32))
    assert np.array_equal(got["pixels"].view(np.uint32), np.ascontiguousarray(want["pixels"]).view(np.uint32))


@gpu
@pytest.mark.parametrize("kw", [dict(rect=(5, 3, 83, 55)), dict(shard=(16, 1, 3))], ids=["ragged-rectangle", "shard-1-of-3"])
def test_small_shapes_with_the_order_forced(G, kw):
    mk = lambda: scenes.cornell_box(96, 64, 8, integrator=api.kTerraIntegratorDirect, **WIDE)
    on = dev(G, mk(), 1, order=2, split=2, **kw)
    off = dev(G, mk(), 0, order=2, split=2, **kw)
    assert same_fb(on, off), kw
    assert on["info"][0] > 0 and off["info"][0] == 0, (on["info"], off["info"])


BLOCKS = 32       # a 96 x 64 frame is two 64 x 64 tiles = 32 pixel blocks, 24 of which have pixels (a block without pixels is never proved: it has no footprint)


# one emissive triangle soup seen from the origin along +z: film position (X, Y) in pixels at depth z -> world
W, Hh, FOV = 96, 64, 50.0


def thf_of(fov):
    return np.float32(math.tan(float((np.float32(fov) * np.float32(0.0174533)) / np.float32(2))))


def film(X, Y, z, pos=(0.0, 0.0, 0.0)):
    t = float(thf_of(FOV)); a = float(np.float32(W) / np.float32(Hh))
    return ((2 * X / W - 1) * a * t * z + pos[0], (1 - 2 * Y / Hh) * t * z + pos[1], z + pos[2])


def soup_scene(tris, spp=16, pos=(0.0, 0.0, 0.0), direction=(0.0, 0.0, 1.0), fov=FOV, width=W, height=Hh, **kw):
    tris = np.asarray(tris, dtype=np.float32).reshape(-1, 3, 3)
    nrm = np.zeros_like(tris); nrm[..., 2] = -1.0
    obj = scenes.ObjectDesc(tris, nrm, np.zeros((len(tris), 3, 2), dtype=np.float32), scenes.Material(albedo=(0.5, 0.5, 0.5), emissive=(1.0, 2.0, 3.0)), "soup")
    return scenes.SceneDesc(objects=[obj], camera_position=tuple(pos), camera_direction=tuple(direction), camera_fov=fov, width=width, height=height, spp=spp, bounces=2, name="soup", **kw)


def host_proved_blocks(L, d, tris):
    """the blocks the host predicate proves, for a camera that looks along +z (identity frame)"""
    out = set()
    for by in range(0, d.height, 16):
        for bx in range(0, d.width, 16):
            if proof(L, np.eye(3), d.camera_position, thf_of(d.camera_fov), np.float32(d.width) / np.float32(d.height), d.jitter, d.width, d.height,
                     bx, by, min(bx + 16, d.width), min(by + 16, d.height), tris):
                out.add((bx // 16, by // 16))
    return out


FILLER = [film(4.0, 4.0, 4.0), film(8.0, 4.0, 4.0), film(6.0, 8.0, 4.0)]      # (a scene of fewer than two triangles runs the replica traversal, which has no leaf-box cull)
EDGES = {
    # a sliver 0.4 pixel wide that reaches one pixel into block (3, 1), which is otherwise empty
    "sliver": ([film(40.0, 24.5, 4.0), film(49.0, 24.3, 4.0), film(49.0, 24.7, 4.0)], (3, 1)),
    # an edge of the triangle lies on the boundary between blocks (2, 1) and (3, 1)
    "edge-on-the-boundary": ([film(36.0, 24.0, 4.0), film(48.0, 20.0, 4.0), film(48.0, 28.0, 4.0)], (3, 1)),
    # the triangle ends inside block (3, 1)'s guard pixel, outside the block
    "inside-the-guard": ([film(36.0, 24.0, 4.0), film(47.4, 20.0, 4.0), film(47.4, 28.0, 4.0)], (3, 1)),
}


@gpu
@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_the_proof(G, name):
    tris, block = EDGES[name]
    mk = lambda: soup_scene([tris, FILLER])
    on = dev(G, mk(), 1, order=2)
    off = dev(G, mk(), 0, order=2)
    assert same_fb(on, off), name
    proved = host_proved_blocks(G, mk(), np.asarray([tris, FILLER], dtype=np.float32))
    assert block not in proved and (5, 3) in proved and (2, 1) not in proved and (0, 0) not in proved, (name, sorted(proved))
    assert on["info"] == (len(proved), BLOCKS), (on["info"], len(proved))      # the device proves what the host proves, no more
    if name == "sliver":
        assert on["acc"][24, 48].sum() > 0, "the sliver's pixel in the otherwise empty block"
        assert on["acc"][16:32, 49:64].sum() == 0 and on["acc"][16:24, 48].sum() == 0, "the rest of that block is empty"


@gpu
def test_camera_inside_a_closed_view_proves_nothing(G):
    mk = lambda: scenes.cornell_box(96, 64, 4, camera_position=(0.0, 1.0, 0.0), camera_fov=60.0)          # inside the room, looking at its back wall
    on, off = dev(G, mk(), 1, order=2), dev(G, mk(), 0, order=2)
    assert same_fb(on, off) and on["info"] == (0, BLOCKS)
    assert (on["acc"].sum(-1) >= 0).all()


@gpu
def test_scene_wholly_behind_the_camera_is_all_proved(G):
    mk = lambda: scenes.cornell_box(96, 64, 4, camera_direction=(0.0, 0.0, -1.0))
    on, off = dev(G, mk(), 1, order=2, split=2, passes=2), dev(G, mk(), 0, order=2, split=2, passes=2)
    assert same_fb(on, off) and on["info"] == (24, BLOCKS)          # every block that has a pixel
    assert not on["acc"].view(np.uint32).any() and not on["pixels"].view(np.uint32).any() and (on["samples"] == 8).all()


@gpu
@pytest.mark.parametrize("integ", list(range(7)))
def test_every_integrator_deposits_plus_zero_for_a_camera_miss(G, integ):
    # none is excluded: in the coupled loop of LDS-resident scenes a camera ray that misses never reaches the integrator
    mk = lambda: scenes.cornell_box(96, 64, 4, integrator=integ, **WIDE)
    on, off = dev(G, mk(), 1, order=2), dev(G, mk(), 0, order=2)
    assert same_fb(on, off), integ
    assert on["info"][0] > 0


@gpu
@pytest.mark.parametrize("case", ["environment", "work-counters", "rand-calls", "out-of-range"])
def test_conditions_that_turn_the_class_off(G, case):
    kw, scene_kw = {}, dict(WIDE)
    if case == "environment":
        scene_kw.update(environment=(0.25, 0.5, 0.75), environment_lighting=True)
    if case == "work-counters":
        kw["counters"] = True
    if case == "rand-calls":
        kw["want_calls"] = True
    mk = lambda: scenes.cornell_box(96, 64, 4, **scene_kw)
    if case == "out-of-range":                                    # the box and its camera x 100: beyond the coordinate range of the leaf-box cull
        def mk():
            d = scenes.cornell_box(96, 64, 4)
            for o in d.objects:
                o.triangles = (o.triangles * np.float32(100)).astype(np.float32)
            d.camera_position = (0.0, 100.0, -700.0)
            return d
    on, off = dev(G, mk(), 1, order=2, **kw), dev(G, mk(), 0, order=2, **kw)
    assert same_fb(on, off), case
    assert on["info"] == (0, BLOCKS), (case, on["info"])
    if case == "work-counters":                                   # the counters are defined by the walk: every pixel walked, the same figures
        assert on["stats"] == off["stats"], (on["stats"], off["stats"])
        assert on["stats"]["rays"] >= 96 * 64 * 4 and on["stats"]["nodes"] > 0 and on["stats"]["tri_tests"] > 0 and on["stats"]["hits"] > 0 and on["stats"]["samples"] == 96 * 64 * 4              # the launch behaved as with the switch off: every block traced
    if case == "environment":
        assert (on["acc"][:, :8].sum(-1) > 0).all()               # the empty columns carry the environment's colour


SOUP_SEED = 7


def soup_cases(seed):
    rng = np.random.default_rng(seed)
    for case in range(40):
        n = int(rng.integers(2, 12))
        centre = rng.normal(size=3) * 0.8 + (0, 0, 4)
        tris = centre[None, None, :] + rng.normal(size=(n, 1, 3)) * rng.uniform(0.1, 1.2) + rng.normal(size=(n, 3, 3)) * rng.uniform(0.02, 0.6)
        direction = np.array([0.0, 0.0, 1.0]) + rng.normal(size=3) * 0.25
        yield dict(tris=tris.astype(np.float32), direction=direction, pos=rng.normal(size=3) * 0.5, split=int(rng.choice([1, 2])), fov=float(rng.uniform(30, 80)))


@gpu
def test_random_soups_through_random_cameras(G):
    mixed = 0
    for k, c in enumerate(soup_cases(SOUP_SEED)):
        mk = lambda: soup_scene(c["tris"], spp=2, pos=c["pos"], direction=c["direction"], fov=c["fov"])
        on, off = dev(G, mk(), 1, order=2, split=c["split"]), dev(G, mk(), 0, order=2, split=c["split"])
        diff = int((on["acc"].view(np.uint32) != off["acc"].view(np.uint32)).sum() + (on["pixels"].view(np.uint32) != off["pixels"].view(np.uint32)).sum() + (on["samples"] != off["samples"]).sum())
        assert diff == 0, (k, diff)
        mixed += 0 < on["info"][0] < 24        # of the 24 blocks that have pixels
    assert 3 * mixed >= 40, mixed          # at least a third of the cases have proved and unproved blocks side by side
