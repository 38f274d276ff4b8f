"""Frames through the exact-quotient helpers (csrc/exact_div.h) against the oracle, which divides with the CPU's `/`: 64 x 48 at 4 spp, every device frame bit for
bit the oracle's. The cases are chosen for the helpers' guards: the three integrators and the Phong preset (every normalize, pdf and make_ray of the path), launch
shapes that move the camera's numerators (a shard, a rectangle at an odd origin, a sample split), the Cornell box scaled by 2^-20 and 2^20 (the barycentric
denominator of surface_init leaves the guarded range at both ends: 2^-80 and 2^80 times its usual size) a quad of 2^-32 edges whose denominator is a denormal, and a light of 2^33
edges whose denominator overflows -- each the only light of its scene, so that a lit pixel proves it was hit and shaded."""
import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_leaf_boxes_gpu import dev
from test_flat_loop_layout_gpu import oracle, equals_oracle

gpu = pytest.mark.gpu
SHAPE = dict(width=64, height=48, spp=4)


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def scaled(d, k):
    """the scene and its camera scaled by the power of two k: every coordinate changes its exponent only"""
    for o in d.objects:
        o.triangles = (np.asarray(o.triangles, np.float32) * np.float32(k)).astype(np.float32)
    d.camera_position = tuple(float(np.float32(c) * np.float32(k)) for c in d.camera_position)
    return d


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis], ids=["simple", "direct", "direct-mis"])
def test_cornell_integrators(G, H, orc_lib, integ):
    mk = lambda: scenes.cornell_box(integrator=integ, **SHAPE)
    got = dev(G, mk(), 1)
    assert got["acc"].sum() > 0 and equals_oracle(got, oracle(H, mk()))


@gpu
def test_cornell_phong(G, H, orc_lib):
    mk = lambda: scenes.cornell_phong(**SHAPE)
    assert equals_oracle(dev(G, mk(), 1), oracle(H, mk()))


@gpu
@pytest.mark.parametrize("kw", [dict(shard=(16, 1, 2)), dict(rect=(7, 5, 24, 20))], ids=["shard-1-of-2", "rectangle-at-an-odd-origin"])
def test_part_of_the_frame(G, H, orc_lib, kw):
    mk = lambda: scenes.cornell_box(**SHAPE)
    got, want = dev(G, mk(), 1, **kw), oracle(H, mk())
    own = got["samples"] == 4
    assert own.any() and not own.all() and (got["samples"][~own] == 0).all()
    assert np.array_equal(got["acc"].view(np.uint32)[own], np.ascontiguousarray(want["acc"]).view(np.uint32)[own])


@gpu
def test_split_four_against_four_calls(G, H, orc_lib):
    one = dev(G, scenes.cornell_box(64, 48, 4), 1, split=4)
    many = dev(G, scenes.cornell_box(64, 48, 1), 1, passes=4)
    assert np.array_equal(one["acc"].view(np.uint32), many["acc"].view(np.uint32)) and np.array_equal(one["pixels"].view(np.uint32), many["pixels"].view(np.uint32))
    H.set_oracle_math(1)
    try:
        want = H.Unit("orc").render_pixels(scenes.cornell_box(64, 48, 1), passes=4, want_calls=False)
    finally:
        H.set_oracle_math(0)
    assert equals_oracle(one, want)


@gpu
@pytest.mark.parametrize("k", [2.0 ** -20, 2.0 ** 20], ids=["scaled-down", "scaled-up"])
def test_scaled_cornell(G, H, orc_lib, k):
    mk = lambda: scaled(scenes.cornell_box(**SHAPE), k)
    assert equals_oracle(dev(G, mk(), 1), oracle(H, mk()))


def sliver_div(tri):
    """surface_init's barycentric denominator of a triangle, restated in float32 operation by operation"""
    f = np.float32
    a, b, c = (np.asarray(v, np.float32) for v in tri)
    e0, e1 = b - a, c - a
    dot = lambda u, v: f(f(f(u[0] * v[0]) + f(u[1] * v[1])) + f(u[2] * v[2]))
    d00, d11, d01 = dot(e0, e0), dot(e1, e1), dot(e0, e1)
    with np.errstate(over="ignore"):
        return f(f(d00 * d11) - f(d01 * d01))


def sliver_scene():
    """a quad of 2^-32 x 2^-32 at the origin, the scene's only light, seen from (0, 0, -1) through a field of view of 2e-7 degrees: the frame is about 2^-28 wide
    there and the quad covers a few pixels right of and above its centre. Near 0 float32 holds these coordinates exactly. Both triangles: e0 . e0 = e1 . e1 = 2^-64
    (or 2^-63 for the diagonal), so div is about 2^-128: a denormal"""
    s = 2.0 ** -32
    tris, nrm, uv = scenes._merge([scenes._quad((0, 0, 0), (s, 0, 0), (s, s, 0), (0, s, 0), (0, 0, -1))])
    for t in tris:
        assert 0 < abs(float(sliver_div(t))) < 2.0 ** -126, sliver_div(t)
    return scenes.SceneDesc(objects=[scenes.ObjectDesc(tris, nrm, uv, scenes.Material(albedo=(0.6, 0.6, 0.6), emissive=(1.0, 0.5, 0.25)), "sliver")],
                            camera_position=(0.0, 0.0, -1.0), camera_fov=2e-7, width=64, height=48, spp=4, bounces=2, name="sliver")


def overflow_scene():
    """a light whose edges are 2^33 long and meet at a right angle at (-1, 0, 3), before the default camera: d00 d11 = 2^132 overflows, d01 = 0, so div = +inf
    (not NaN) and every hit near the corner has u = v = 0: the camera rays are shaded with the corner's normal and see the emission"""
    n = np.tile(np.array([0, 0, -1], np.float32), (3, 1))
    tri = np.array([[(-1, 0, 3), (2.0 ** 33, 0, 3), (-1, 2.0 ** 33, 3)]], np.float32)
    assert np.isinf(sliver_div(tri[0]))
    return scenes.SceneDesc(objects=[scenes.ObjectDesc(tri, n[None], np.zeros((1, 3, 2), np.float32), scenes.Material(albedo=(0.6, 0.6, 0.6), emissive=(1.0, 0.5, 0.25)), "huge")],
                            width=64, height=48, spp=4, bounces=2, name="overflow")


def nan_aware_equal(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@gpu
@pytest.mark.parametrize("mk", [sliver_scene, overflow_scene], ids=["denormal-div", "overflowing-div"])
def test_denormal_and_overflowing_denominators(G, H, orc_lib, mk):
    """the triangle is the only light and only its own emission can light a pixel: a lit pixel is a path that hit it and ran surface_init on it. Frames compared by
    bits, and by NaN-ness where a NaN reaches the frame"""
    got, want = dev(G, mk(), 1), oracle(H, mk())
    lit = np.asarray(want["acc"])[..., 0] > 0
    assert lit.sum() >= 4 and np.isfinite(np.asarray(want["acc"])).all()
    assert nan_aware_equal(got["acc"], want["acc"]) and nan_aware_equal(got["pixels"], want["pixels"])
