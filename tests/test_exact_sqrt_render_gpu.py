"""Frames through the short square root, the one-path tangent frame and the short roulette rescale (csrc/exact_sqrt.h, trace_math.h make_basis, exact_div.h
roulette_scale) against the oracle, which calls the CPU's sqrtf, branches in its tangent frame and divides in double precision: 64 x 48 at 8 spp, every device
frame bit for bit the oracle's. The Cornell box (diffuse walls facing every axis: both arms of the tangent frame in one wave), the Phong preset (make_basis of the
reflected direction, which is no unit normal) and the sphere scene (curved normals, the LDS-resident kernels on a tree) under Simple and Direct; Direct + MIS on
the Cornell box (the light sample's root)."""
import pytest

from terra_amd import api, runtime, scenes
from test_leaf_boxes_gpu import dev
from test_flat_loop_layout_gpu import oracle, equals_oracle

gpu = pytest.mark.gpu
SHAPE = dict(width=64, height=48, spp=8)
SIMPLE, DIRECT, MIS = api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis
CASES = [(scenes.cornell_box, SIMPLE), (scenes.cornell_box, DIRECT), (scenes.cornell_box, MIS), (scenes.cornell_phong, SIMPLE), (scenes.cornell_phong, DIRECT),
         (scenes.cornell_spheres, SIMPLE), (scenes.cornell_spheres, DIRECT)]
IDS = ["cornell-simple", "cornell-direct", "cornell-direct-mis", "phong-simple", "phong-direct", "spheres-simple", "spheres-direct"]


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


@gpu
@pytest.mark.parametrize("scene,integ", CASES, ids=IDS)
def test_frame_equals_oracle(G, H, orc_lib, scene, integ):
    mk = lambda: scene(integrator=integ, **SHAPE)
    got = dev(G, mk(), 1)
    assert (got["samples"] == SHAPE["spp"]).all() and got["acc"].sum() > 0
    assert equals_oracle(got, oracle(H, mk()))
