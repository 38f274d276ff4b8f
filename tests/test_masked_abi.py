"""Masked rendering at the C boundary, without a GPU (include/terra_amd.h "Masked rendering"): the new entry points are exported and terra_amd/api.py carries
their signatures, a gcc-compiled probe of the header links against them with the prototypes spelled out, and the five that take a scene refuse an uncommitted one
before anything touches a device or a buffer."""
import ctypes as C
import subprocess

import numpy as np

from terra_amd import api, runtime

SCENE_SYMBOLS = ("terra_amd_render_masked_device", "terra_amd_render_masked", "terra_amd_render_aov_masked_device",
                 "terra_amd_render_adaptive_masked_device", "terra_amd_render_adaptive_masked")
SYMBOLS = SCENE_SYMBOLS + ("terra_amd_error_mask_device",)
ERR_NOT_COMMITTED = -2


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.MASKED_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.MASKED_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("render_masked_device", "render_aov_masked_device", "error_mask_device", "mask_shape"):
        assert callable(getattr(runtime, name)), name
    assert runtime.mask_shape(100, 70) == (5, 7) and runtime.mask_shape(16, 17) == (2, 1)


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_render_masked_device ) ( const TerraCamera*, HTerraScene, void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, const void*, void*, void* ) = terra_amd_render_masked_device;
static int ( *const p_render_masked ) ( const TerraCamera*, HTerraScene, const TerraFramebuffer*, size_t, size_t, size_t, size_t, const uint32_t* ) = terra_amd_render_masked;
static int ( *const p_render_aov_masked_device ) ( const TerraCamera*, HTerraScene, void*, size_t, size_t, size_t, size_t, size_t, size_t, const void*, void* ) = terra_amd_render_aov_masked_device;
static int ( *const p_error_mask_device ) ( const void*, size_t, size_t, size_t, float, int, void*, void* ) = terra_amd_error_mask_device;
static int ( *const p_render_adaptive_masked_device ) ( const TerraCamera*, HTerraScene, void*, void*, void*, void*, size_t, size_t, size_t, size_t, size_t, size_t,
                                                        const TerraAmdAdaptiveOptions*, TerraAmdAdaptiveReport*, void* ) = terra_amd_render_adaptive_masked_device;
static int ( *const p_render_adaptive_masked ) ( const TerraCamera*, HTerraScene, TerraFramebuffer*, TerraAmdMoments*, TerraAmdAovResult*, size_t, size_t, size_t, size_t,
                                                 const TerraAmdAdaptiveOptions*, TerraAmdAdaptiveReport* ) = terra_amd_render_adaptive_masked;
int main ( void ) {
    printf ( "%d\\n", p_render_masked_device != 0 && p_render_masked != 0 && p_render_aov_masked_device != 0 && p_error_mask_device != 0
                      && p_render_adaptive_masked_device != 0 && p_render_adaptive_masked != 0 );
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


def test_uncommitted_scene_is_refused_with_no_byte_changed(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    cam = api.TerraCamera()
    cam.position = api.f3((0.0, 0.0, 0.0)); cam.direction = api.f3((0.0, 0.0, 1.0)); cam.up = api.f3((0.0, 1.0, 0.0)); cam.fov = 45.0
    SENT = 0xA5
    pix = np.full(4 * 4 * 3, SENT, np.uint8).repeat(4).view(np.float32)
    res = np.full(4 * 4 * 16, SENT, np.uint8)
    mom = np.full(4 * 4 * 32, SENT, np.uint8)
    aov = np.full(4 * 4 * 48, SENT, np.uint8)
    mask = np.ones(1, np.uint32)
    fb = api.Framebuffer(lib, 4, 4)
    fb.pixels.view(np.uint8)[...] = SENT; fb.results.view(np.uint8)[...] = SENT
    rep = api.TerraAmdAdaptiveReport()
    rep_before = bytes(rep)
    try:
        for call in (lambda: lib.render_masked_device(C.byref(cam), scene, pix.ctypes.data, res.ctypes.data, 4, 4, 0, 0, 4, 4, mask.ctypes.data, None, None),
                     lambda: lib.render_masked(C.byref(cam), scene, C.byref(fb.fb), 0, 0, 4, 4, mask.ctypes.data),
                     lambda: lib.render_aov_masked_device(C.byref(cam), scene, aov.ctypes.data, 4, 4, 0, 0, 4, 4, mask.ctypes.data, None),
                     lambda: lib.render_adaptive_masked_device(C.byref(cam), scene, pix.ctypes.data, res.ctypes.data, mom.ctypes.data, aov.ctypes.data, 4, 4, 0, 0, 4, 4, None, C.byref(rep), None),
                     lambda: lib.render_adaptive_masked(C.byref(cam), scene, C.byref(fb.fb), mom.ctypes.data, aov.ctypes.data, 0, 0, 4, 4, None, C.byref(rep))):
            lib.clear_error()
            assert call() == ERR_NOT_COMMITTED
            assert runtime.last_error() != ""
        for buf in (pix, res, mom, aov, fb.pixels, fb.results):
            assert (np.asarray(buf).view(np.uint8) == SENT).all()
        assert mask[0] == 1 and bytes(rep) == rep_before
    finally:
        lib.clear_error()
        lib.fn("terra_amd_clear_first_error", None, [])()
        fb.destroy()
        lib.scene_destroy(scene)


def test_headless_flag_needs_adaptive(H, amd_lib, tmp_path):
    """terra_headless --adaptive-masked is valid only with --adaptive: refused at the command line, before anything is read"""
    exe = tmp_path / "terra_headless"
    r = subprocess.run(["gcc", "-std=gnu11", f"-I{H.ROOT / 'include'}", str(H.ROOT / "apps" / "terra_headless.c"), f"-L{H.ROOT / 'terra_amd'}", "-lterra_amd",
                        f"-Wl,-rpath,{H.ROOT / 'terra_amd'}", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tmp_path / "none.obj"), str(tmp_path / "out.pfm"), "--adaptive-masked"], capture_output=True, text=True)
    assert r.returncode == 64 and "--adaptive-masked is valid only with --adaptive" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "out.pfm").exists()
