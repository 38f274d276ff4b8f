"""Lens rendering at the C boundary, without a GPU (include/terra_amd.h "Lens rendering"): the five entry points are exported and terra_amd/api.py carries their
signatures, TerraAmdLens has the pinned layout in C and in the ctypes mirror, a gcc-compiled probe of the header links against the spelled-out prototypes, an
uncommitted scene is refused before anything touches a device, every bad lens is refused before the call asks for a device, and terra_headless linked against
the compiled reference says that --camera-model needs libterra_amd.so and writes the pinhole image."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from terra_amd import api, runtime, scenes

SYMBOLS = ("terra_amd_render_lens_device", "terra_amd_render_lens", "terra_amd_render_aov_lens_device", "terra_amd_render_aov_lens", "terra_amd_unit_lens_rays")
LENS_OFFSETS = {"model": 0, "lens_radius": 4, "focus_distance": 8, "ortho_height": 12, "fisheye_fov": 16, "reserved": 20}
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.LENS_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.LENS_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("render_lens_device", "render_aov_lens_device", "lens_rays"):
        assert hasattr(runtime, name), name


def test_lens_layout_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.Lens) == 32
    for f, off in LENS_OFFSETS.items():
        assert getattr(api.Lens, f).offset == off, f
    items = ["sizeof ( TerraAmdLens )"] + [f"offsetof ( TerraAmdLens, {f} )" for f in LENS_OFFSETS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [32] + list(LENS_OFFSETS.values())


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_render_lens_device ) ( const TerraCamera*, const TerraAmdLens*, HTerraScene, void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, void*, void* ) = terra_amd_render_lens_device;
static int ( *const p_render_lens ) ( const TerraCamera*, const TerraAmdLens*, HTerraScene, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) = terra_amd_render_lens;
static int ( *const p_render_aov_lens_device ) ( const TerraCamera*, const TerraAmdLens*, HTerraScene, void*, size_t, size_t, size_t, size_t, size_t, size_t, void* ) = terra_amd_render_aov_lens_device;
static int ( *const p_render_aov_lens ) ( const TerraCamera*, const TerraAmdLens*, HTerraScene, TerraAmdAovResult*, size_t, size_t, size_t, size_t, size_t, size_t ) = terra_amd_render_aov_lens;
static int ( *const p_unit_lens_rays ) ( const TerraCamera*, const TerraAmdLens*, size_t, size_t, int, const uint32_t*, float, const float*, TerraAmdRay* ) = terra_amd_unit_lens_rays;
int main ( void ) {
    printf ( "%d\\n", p_render_lens_device != 0 && p_render_lens != 0 && p_render_aov_lens_device != 0 && p_render_aov_lens != 0 && p_unit_lens_rays != 0 );
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


def lens_of(model=0, lens_radius=0.0, focus_distance=0.0, ortho_height=0.0, fisheye_fov=0.0, reserved=(0, 0, 0)):
    l = api.Lens()
    l.model, l.lens_radius, l.focus_distance, l.ortho_height, l.fisheye_fov = model, lens_radius, focus_distance, ortho_height, fisheye_fov
    l.reserved[:] = reserved
    return l


def four_forms(lib, cam, lens, scene, fb, aov):
    """the four render forms on host memory (the device forms are refused before they look at a pointer)"""
    pc = C.byref(cam) if cam is not None else None
    pl = C.byref(lens) if lens is not None else None
    return [lambda: lib.render_lens_device(pc, pl, scene, fb.pixels.ctypes.data, fb.results.ctypes.data, 4, 4, 0, 0, 4, 4, None, None),
            lambda: lib.render_lens(pc, pl, scene, C.byref(fb.fb), 0, 0, 4, 4),
            lambda: lib.render_aov_lens_device(pc, pl, scene, aov.ctypes.data, 4, 4, 0, 0, 4, 4, None),
            lambda: lib.render_aov_lens(pc, pl, scene, aov.ctypes.data, 4, 4, 0, 0, 4, 4)]


def test_uncommitted_scene_is_refused_without_a_device(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    aov = np.zeros((4, 4), runtime.AOV_DTYPE)
    fb = api.Framebuffer(lib, 4, 4)
    cam = scenes.camera_of(scenes.cornell_box(4, 4, 1))
    try:
        for lens in (lens_of(0), lens_of(7)):                # "not committed" comes first: before the lens is looked at
            for k, call in enumerate(four_forms(lib, cam, lens, scene, fb, aov)):
                lib.clear_error()
                assert call() == ERR_NOT_COMMITTED, k
                assert runtime.last_error() != ""
        assert not aov.view(np.uint8).any() and not fb.results.view(np.uint8).any() and not fb.pixels.view(np.uint32).any()
    finally:
        lib.clear_error()
        fb.destroy()
        lib.scene_destroy(scene)


NAN, INF = float("nan"), float("inf")
BAD_LENSES = {
    "model -1": dict(model=-1), "model 4": dict(model=4),
    "negative radius": dict(lens_radius=-0.1, focus_distance=1.0), "nan radius": dict(lens_radius=NAN, focus_distance=1.0), "inf radius": dict(lens_radius=INF, focus_distance=1.0),
    "negative focus": dict(focus_distance=-1.0), "nan focus": dict(focus_distance=NAN), "inf focus": dict(lens_radius=0.1, focus_distance=INF),
    "negative ortho height": dict(ortho_height=-1.0), "nan ortho height": dict(model=1, ortho_height=NAN), "inf fisheye fov": dict(fisheye_fov=INF), "negative fisheye fov": dict(model=3, fisheye_fov=-10.0),
    "lens without focus": dict(lens_radius=0.1, focus_distance=0.0),
    "ortho with a lens": dict(model=1, lens_radius=0.1, focus_distance=1.0, ortho_height=2.0), "equirect with a lens": dict(model=2, lens_radius=0.1, focus_distance=1.0),
    "fisheye with a lens": dict(model=3, lens_radius=0.1, focus_distance=1.0, fisheye_fov=180.0),
    "ortho height 0": dict(model=1, ortho_height=0.0), "fisheye fov 0": dict(model=3, fisheye_fov=0.0), "fisheye fov 361": dict(model=3, fisheye_fov=361.0),
    "reserved 0": dict(reserved=(1, 0, 0)), "reserved 2": dict(model=2, reserved=(0, 0, -1)),
}


def test_bad_arguments_are_refused(amd_lib):
    """on a committed scene, with or without a device: the lens is checked before the call asks for the scene's device replica"""
    lib = runtime.load(need_torch=False)
    d = scenes.cornell_box(4, 4, 1)
    lib.clear_error()
    scene = scenes.build_scene(lib, d)
    aov = np.zeros((4, 4), runtime.AOV_DTYPE)
    fb = api.Framebuffer(lib, 4, 4)
    cam = scenes.camera_of(d)
    xy = np.zeros((1, 2), np.uint32); r4 = np.zeros((1, 4), np.float32); out = np.zeros(1, api.RAY_DTYPE)
    try:
        cases = {name: (cam, lens_of(**kw)) for name, kw in BAD_LENSES.items()}
        cases["null lens"] = (cam, None)
        cases["null camera"] = (None, lens_of(0))
        for name, (c, lens) in cases.items():
            calls = four_forms(lib, c, lens, scene, fb, aov)
            calls.append(lambda: lib.unit_lens_rays(C.byref(c) if c is not None else None, C.byref(lens) if lens is not None else None, 4, 4, 1, xy.ctypes.data, 0.0, r4.ctypes.data, out.ctypes.data))
            for k, call in enumerate(calls):
                lib.clear_error()
                assert call() == ERR_BAD_ARGUMENT, (name, k, runtime.last_error())
                assert runtime.last_error() != "", (name, k)
        assert not aov.view(np.uint8).any() and not fb.results.view(np.uint8).any() and not fb.pixels.view(np.uint32).any() and not out.view(np.uint8).any()
        # the limits themselves are good lenses: whatever these calls answer, it is not "bad argument" about the lens
        for kw in (dict(model=3, fisheye_fov=360.0), dict(lens_radius=0.1, focus_distance=1e-3), dict(model=1, ortho_height=1e-3), dict(model=0, focus_distance=5.0)):
            lib.clear_error()
            rc = lib.render_aov_lens(C.byref(cam), C.byref(lens_of(**kw)), scene, aov.ctypes.data, 4, 4, 0, 0, 4, 4)
            assert rc == 0 or "lens" not in runtime.last_error(), (kw, runtime.last_error())
    finally:
        lib.clear_error()
        fb.destroy()
        lib.scene_destroy(scene)


def test_headless_help_lists_the_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    out = subprocess.run([str(exe), "--help"], capture_output=True, text=True).stdout
    for flag in ("--camera-model pinhole|thinlens|ortho|equirect|fisheye", "--aperture R", "--focus D", "--ortho-height H", "--fisheye-fov DEG"):
        assert flag in out, flag


def test_headless_against_the_reference_says_so_and_writes_the_pinhole_image(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "ref")
    obj = tmp_path / "c.obj"
    write_obj(scenes.cornell_box(40, 30, 2), obj)
    args = ["--width", "40", "--height", "30", "--spp", "2", "--integrator", "normals", "--tonemap", "none"]
    plain = subprocess.run([str(exe), str(obj), str(tmp_path / "plain.pfm")] + args, capture_output=True, text=True)
    assert plain.returncode == 0 and "libterra_amd.so" not in plain.stderr, plain.stderr
    r = subprocess.run([str(exe), str(obj), str(tmp_path / "lens.pfm")] + args + ["--camera-model", "thinlens", "--aperture", "0.05", "--focus", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--camera-model needs libterra_amd.so; ignored, the pinhole image is written" in r.stderr
    assert np.array_equal(read_pfm(tmp_path / "lens.pfm"), read_pfm(tmp_path / "plain.pfm")) and read_pfm(tmp_path / "plain.pfm").any()
    bad = subprocess.run([str(exe), str(obj), str(tmp_path / "bad.pfm")] + args + ["--camera-model", "telephoto"], capture_output=True, text=True)
    assert bad.returncode == 64 and "--camera-model pinhole|thinlens|ortho|equirect|fisheye" in bad.stderr
