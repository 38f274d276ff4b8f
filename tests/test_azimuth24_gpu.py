"""The samplers' azimuth on the device: computed from the variate's 24 bits (csrc/dev_math.h tdm_azimuth24) or read from the 128 MB table
(terra_amd_set_azimuth_table) -- no bit may differ.

* terra_amd_unit_azimuth24: one launch writes tdm_azimuth24 ( k ) for every k < 2^24 into a second buffer and compares it with a table filled as a commit fills
  it (tdm_sincosf_pair itself); the mismatch count that comes back must be 0.
* Frames rendered from scenes committed with the table on and with it off must be equal in `pixels` and `results`, bit for bit: Cornell at 64 x 64, 8 spp under
  Simple, Direct and MIS (path_draw's azimuth and the MIS integrator's own draw; the LDS-resident kernels, the only ones that read the table); cornell_phong (its
  diffuse arm takes the azimuth); a 32-triangle soup that has no pair form (tools/leaf_boxes_soup.py's scene); the sphere scene at 64 x 48 (a kernel that reads
  its scene from global memory and always computes; GGX and glass samplers). terra_amd_azimuth_table_info must say that the first render's kernel was handed
  the table and the second one's was not (the sphere scene's: neither), so that a table which could not be had does not pass as two computing renders.
* The hall at 128 x 72, 4 spp (a global-memory kernel: it ran the two-arm computation before and runs tdm_azimuth24 now) against
  tests/golden/azimuth24_hall_parent.npz: hall_frame()'s arrays as the build of the commit before tdm_azimuth24 rendered them, byte for byte. Under Simple a
  path shows only where it reaches one of the three ceiling lights (293 of the 9,216 pixels are lit), so the same frame under Direct, where every surface in
  sight is lit, is held as well."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_oracle_vs_reference import soup_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load()
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def frame(L, d, table=None):
    """(pixels, results, terra_amd_azimuth_table_info) of d rendered once by a scene committed with the azimuth table on / off (None: the library's default); the switch is put back"""
    import torch
    default = L.get_azimuth_table()
    if table is not None:
        L.set_azimuth_table(int(table))
    try:
        scene = scenes.build_scene(L, d, counters=False)
        assert runtime.last_error() == "", runtime.last_error()
    finally:
        L.set_azimuth_table(default)
    try:
        fb = runtime.DeviceFramebuffer(d.width, d.height)
        runtime.render_device(L, scenes.camera_of(d), scene, fb)
        torch.cuda.synchronize()
        assert runtime.last_error() == ""
        return fb.pixels.cpu().numpy(), fb.results.cpu().numpy(), L.azimuth_table_info(scene)
    finally:
        L.scene_destroy(scene)


HALL = {"simple": api.kTerraIntegratorSimple, "direct": api.kTerraIntegratorDirect}


def hall_frame(L, integ):
    return frame(L, scenes.sponza_hall(128, 72, 4, integrator=HALL[integ]))[:2]


def soup(H):
    d = soup_scene(H, 32, 18, n_objects=3)
    d.width, d.height, d.spp = 64, 64, 8
    return d


CASES = {
    "cornell-simple": lambda H: scenes.cornell_box(64, 64, 8, integrator=api.kTerraIntegratorSimple),
    "cornell-direct": lambda H: scenes.cornell_box(64, 64, 8, integrator=api.kTerraIntegratorDirect),
    "cornell-mis": lambda H: scenes.cornell_box(64, 64, 8, integrator=api.kTerraIntegratorDirectMis),
    "cornell-phong": lambda H: scenes.cornell_phong(64, 64, 8),
    "soup-32": soup,
    "spheres": lambda H: scenes.cornell_spheres(64, 48, 8),
}


def test_computed_azimuth_equals_the_table_on_the_device(G):
    count = C.c_uint32(0xffffffff)
    runtime.check(G.unit_azimuth24(C.byref(count)), "terra_amd_unit_azimuth24")
    assert count.value == 0


def test_switch_reads_back(G):
    default = G.get_azimuth_table()
    try:
        for on in (1, 0, 1):
            G.set_azimuth_table(on)
            assert G.get_azimuth_table() == on
    finally:
        G.set_azimuth_table(default)


@pytest.mark.parametrize("name", list(CASES))
def test_table_on_and_off_render_the_same_bits(G, H, name):
    on_pixels, on_results, on_read = frame(G, CASES[name](H), table=1)
    off_pixels, off_results, off_read = frame(G, CASES[name](H), table=0)
    assert (on_read, off_read) == ((0, 0) if name == "spheres" else (1, 0))
    assert on_results.view(np.int32).reshape(-1, 4)[:, 3].min() == 8 and np.abs(on_pixels).sum() > 0      # every pixel took its samples, the frame is lit
    assert np.array_equal(on_pixels.view(np.uint32), off_pixels.view(np.uint32))
    assert np.array_equal(on_results, off_results)


@pytest.mark.parametrize("integ", list(HALL))
def test_hall_equals_the_build_before_the_single_arm_form(G, H, integ):
    g = np.load(H.GOLDEN / "azimuth24_hall_parent.npz")
    pixels, results = hall_frame(G, integ)
    assert (g[f"pixels_{integ}"] != 0).sum() > (5000 if integ == "direct" else 500)
    assert pixels.tobytes() == g[f"pixels_{integ}"].tobytes()
    assert results.tobytes() == g[f"results_{integ}"].tobytes()
