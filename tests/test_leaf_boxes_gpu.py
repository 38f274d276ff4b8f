"""terra_amd_set_leaf_box_test on the device: a ranked launch with the fused box test and no work counters tests the scene's distinct leaf boxes in one
wave-uniform loop instead of walking the tree (csrc/traverse_ref.h "Flat leaf-box test"). The set of triangles a ray then tests can only gain triangles the
ray cannot hit (tests/test_leaf_boxes.py checks that on the host), so every case here renders with the switch off, then on, into fresh frames and asks for the
same `pixels` and `results` bit for bit -- and terra_amd_leaf_box_info must say that the second render used the flat form where the launch qualifies and did not
where it does not.

The rule for a scene of ONE triangle: the commit gives scenes of fewer than two triangles the replica traversal (no leaf-box cull, hence no fused box test:
scene_host.cpp choose_tree), and the flat form is defined for cull launches only, so that launch walks the tree: `flat` is expected False there, the frame must
be equal and the one-entry table must exist. The empty child slot of such a tree is therefore covered by the host test of the table (tests/test_leaf_boxes.py,
"soup1"), not by a flat launch."""
import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_oracle_vs_reference import soup_scene

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


@pytest.fixture(scope="module")
def G(L):
    assert L.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return L


def dev(L, d, flat, split=1, passes=1, shard=None, rect=None, counters=False, tree_mode=None):
    import torch
    scene = scenes.build_scene(L, d, tree_mode=tree_mode, counters=counters)
    assert runtime.last_error() == "", runtime.last_error()
    assert L.get_leaf_box_test(scene) == 1                      # the default
    assert L.set_leaf_box_test(scene, int(flat)) == 0 and L.get_leaf_box_test(scene) == int(flat)
    assert L.set_sample_split(scene, split) == 0
    fb = runtime.DeviceFramebuffer(d.width, d.height); cam = scenes.camera_of(d)
    for _ in range(passes):
        if shard:
            runtime.render_device_sharded(L, cam, scene, fb, *shard)
        else:
            runtime.render_device(L, cam, scene, fb, rect)
    torch.cuda.synchronize()
    assert runtime.last_error() == ""
    used, boxes = runtime.leaf_box_info(L, scene)
    res = fb.results_host()
    out = dict(pixels=fb.pixels_host().copy(), acc=res["acc"].copy(), samples=res["samples"].copy(), used=used, boxes=boxes)
    L.scene_destroy(scene)
    return out


def same_fb(a, b):
    return (np.array_equal(a["acc"].view(np.uint32), b["acc"].view(np.uint32)) and np.array_equal(a["samples"], b["samples"])
            and np.array_equal(a["pixels"].view(np.uint32), b["pixels"].view(np.uint32)))


def off_then_on(G, mk, expect_flat, **kw):
    off = dev(G, mk(), 0, **kw)
    on = dev(G, mk(), 1, **kw)
    assert same_fb(off, on), kw
    assert not off["used"]
    assert on["used"] == expect_flat, (on["used"], on["boxes"], kw)
    return off, on


CORNELL = dict(width=64, height=48, spp=8)


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis])
def test_cornell_integrators(G, integ):
    off, on = off_then_on(G, lambda: scenes.cornell_box(integrator=integ, **CORNELL), True)
    assert on["boxes"] == 16 and (on["samples"] == 8).all() and on["acc"].sum() > 0


@gpu
@pytest.mark.parametrize("kw", [dict(split=4), dict(rect=(7, 5, 24, 20)), dict(shard=(16, 1, 2)), dict(passes=2)],
                         ids=["sample-split-4", "rectangle-at-an-odd-origin", "shard-1-of-2-tile-16", "two-accumulating-calls"])
def test_cornell_simple_launch_shapes(G, kw):
    off, on = off_then_on(G, lambda: scenes.cornell_box(**CORNELL), True, **kw)
    assert on["acc"].sum() > 0


@gpu
def test_cornell_with_the_job_order_and_the_empty_skip(G):
    # 20 x 16 = 320 pixel blocks: job-ordered by default, and some of them proved empty
    off, on = off_then_on(G, lambda: scenes.cornell_box(320, 256, 2), True)
    assert (on["samples"] == 2).all()


@gpu
def test_cornell_phong(G):
    off_then_on(G, lambda: scenes.cornell_phong(64, 48, 4), True)


@gpu
@pytest.mark.parametrize("n_tris,seed,flat", [(1, 11, False), (2, 12, True), (3, 13, True), (32, 18, True)])
def test_soups(G, H, n_tris, seed, flat):
    def mk():
        d = soup_scene(H, n_tris, seed, n_objects=min(3, n_tris))
        d.width, d.height, d.spp = 32, 32, 4
        return d
    off, on = off_then_on(G, mk, flat)
    assert 1 <= on["boxes"] <= n_tris


@gpu
def test_flat_frame_equals_the_oracle(H, G, orc_lib):
    mk = lambda: scenes.cornell_box(**CORNELL)
    H.set_oracle_math(1)
    try:
        want = H.Unit("orc").render_pixels(mk(), passes=1, want_calls=False)
    finally:
        H.set_oracle_math(0)
    got = dev(G, mk(), 1)
    assert got["used"]
    assert np.array_equal(got["acc"].view(np.uint32), np.ascontiguousarray(want["acc"]).view(np.uint32))
    assert np.array_equal(got["pixels"].view(np.uint32), np.ascontiguousarray(want["pixels"]).view(np.uint32))


def _cornell_x100():
    d = scenes.cornell_box(**CORNELL)
    for o in d.objects:
        o.triangles = (o.triangles * np.float32(100)).astype(np.float32)
    d.camera_position = tuple(100.0 * c for c in d.camera_position)
    return d


@gpu
@pytest.mark.parametrize("case", ["33-triangles", "out-of-range", "tree-mode-reference", "work-counters"])
def test_launches_that_keep_the_walk(G, H, case):
    kw = {}
    mk = lambda: scenes.cornell_box(**CORNELL)
    if case == "33-triangles":
        def mk():
            d = soup_scene(H, 33, 19)
            d.width, d.height, d.spp = 32, 32, 4
            return d
    if case == "out-of-range":
        mk = _cornell_x100
    if case == "tree-mode-reference":
        kw["tree_mode"] = 0
    if case == "work-counters":
        kw["counters"] = True
    off, on = off_then_on(G, mk, False, **kw)
    assert on["boxes"] == (0 if case == "33-triangles" else 16)


@gpu
def test_frame_with_axis_parallel_camera_rays_is_equal(G):
    # camera at an integer position looking down +z, no jitter, an odd width: the camera rays of the central pixel column have direction x == 0 exactly, so
    # their inverse direction is infinite there and their waves are not tame: the code sends such a wave down the tree walk inside a launch that uses the flat
    # form. What is CHECKED is the frame (terra_amd_leaf_box_info speaks of the launch, not of a wave)
    mk = lambda: scenes.cornell_box(65, 48, 4, camera_position=(0.0, 1.0, -3.0), jitter=0.0)
    d = mk()
    assert (2.0 * (32 + 0.5) / d.width - 1.0) == 0.0
    off, on = off_then_on(G, mk, True)
    assert on["acc"][:, 32].sum() > 0
