"""Ray-sourced rendering at the C boundary, without a GPU (include/terra_amd.h "Ray-sourced rendering"): the four entry points are exported and terra_amd/api.py
carries their signatures, a gcc-compiled probe of the header links against them with the prototypes the issue fixed, an uncommitted scene is refused before anything
touches a device, and runtime.radiance's folding of a 1-D batch into a frame is the pure function it is documented to be."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from terra_amd import api, runtime

SYMBOLS = ("terra_amd_render_rays_device", "terra_amd_render_rays", "terra_amd_render_aov_rays_device", "terra_amd_render_aov_rays")
ERR_NOT_COMMITTED = -2


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.RAY_SOURCE_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.RAY_SOURCE_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_render_rays_device ) ( HTerraScene, const void*, void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, void*, void* ) = terra_amd_render_rays_device;
static int ( *const p_render_rays ) ( HTerraScene, const TerraAmdRay*, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) = terra_amd_render_rays;
static int ( *const p_render_aov_rays_device ) ( HTerraScene, const void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, void* ) = terra_amd_render_aov_rays_device;
static int ( *const p_render_aov_rays ) ( HTerraScene, const TerraAmdRay*, TerraAmdAovResult*, size_t, size_t, size_t, size_t, size_t, size_t ) = terra_amd_render_aov_rays;
int main ( void ) {
    printf ( "%d\\n", p_render_rays_device != 0 && p_render_rays != 0 && p_render_aov_rays_device != 0 && p_render_aov_rays != 0 );
    return 0;
}
"""


def test_header_probe_compiles_and_links(H, amd_lib, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{H.ROOT / 'include'}", str(src), f"-L{H.ROOT / 'terra_amd'}", "-lterra_amd",
                        f"-Wl,-rpath,{H.ROOT / 'terra_amd'}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_uncommitted_scene_is_refused_without_a_device(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    rays = np.zeros((4, 4), api.RAY_DTYPE)
    aov = np.zeros((4, 4), runtime.AOV_DTYPE)
    fb = api.Framebuffer(lib, 4, 4)
    try:
        for call in (lambda: lib.render_rays_device(scene, rays.ctypes.data, rays.ctypes.data, rays.ctypes.data, 4, 4, 0, 0, 4, 4, None, None),
                     lambda: lib.render_rays(scene, rays.ctypes.data, C.byref(fb.fb), 0, 0, 4, 4),
                     lambda: lib.render_aov_rays_device(scene, rays.ctypes.data, aov.ctypes.data, 4, 4, 0, 0, 4, 4, None),
                     lambda: lib.render_aov_rays(scene, rays.ctypes.data, aov.ctypes.data, 4, 4, 0, 0, 4, 4)):
            lib.clear_error()
            assert call() == ERR_NOT_COMMITTED
            assert runtime.last_error() != ""
        assert not aov.view(np.uint8).any() and not fb.results.view(np.uint8).any()
    finally:
        lib.clear_error()
        fb.destroy()
        lib.scene_destroy(scene)


def numbered_rays(n):
    """n active records that carry their own index"""
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0] = np.arange(n); rays[:, 3] = np.inf; rays[:, 6] = 1.0
    return rays


@pytest.mark.parametrize("n,height", [(1, 1), (255, 1), (256, 1), (257, 2)])
def test_radiance_folding(n, height):
    assert runtime.RADIANCE_FRAME_WIDTH == 256 and runtime.radiance_frame_shape(n) == (height, 256)
    rays = numbered_rays(n)
    frame = runtime.fold_rays(rays)
    assert frame.shape == (height, 256, 8) and frame.dtype == np.float32 and frame.flags["C_CONTIGUOUS"]
    flat = frame.reshape(-1, 8)
    assert np.array_equal(flat[:n].view(np.uint32), rays.view(np.uint32))           # ray i is pixel (i % 256, i // 256)
    for i in (0, n - 1):
        assert frame[i // 256, i % 256, 0] == i
    pad = flat[n:]
    assert len(pad) == height * 256 - n
    assert not pad[:, 4:7].any() and np.isfinite(pad).all()                            # the padding is inactive: a direction of exactly (0, 0, 0)
    assert np.array_equal(runtime.unfold_pixels(frame, n).view(np.uint32), rays.view(np.uint32))      # the unfold returns the rays' order
    per_pixel = np.arange(height * 256 * 3, dtype=np.float32).reshape(height, 256, 3)
    assert np.array_equal(runtime.unfold_pixels(per_pixel, n), per_pixel.reshape(-1, 3)[:n])
    assert np.array_equal(rays.view(np.uint32), numbered_rays(n).view(np.uint32))      # the input is left as it was
