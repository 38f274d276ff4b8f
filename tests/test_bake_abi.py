"""Lightmap baking at the C boundary, without a GPU (include/terra_amd.h "Lightmap baking"): the four entry points are exported and terra_amd/api.py carries their
signatures, TerraAmdAtlas and TerraAmdAtlasTexel have the pinned layout in C and in the ctypes mirror, a gcc-compiled probe of the spelled-out prototypes links, an
uncommitted scene is refused before anything else is looked at, every bad argument is refused before the call asks for a device with the outputs untouched, the
runtime helpers exist and the headless tool's --help names the four flags."""
import ctypes as C
import subprocess

import numpy as np

from terra_amd import api, runtime, scenes

SYMBOLS = ("terra_amd_atlas_points_device", "terra_amd_atlas_points", "terra_amd_dilate_device", "terra_amd_dilate")
ATLAS_OFFSETS = {"width": 0, "height": 4, "uv_scale": 8, "uv_offset": 16, "margin": 24, "reserved": 28}
TEXEL_OFFSETS = {"triangle": 0, "wb": 4, "wc": 8, "distance2": 12}
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4
GUARD = 0x5ca1ab1e


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.BAKE_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.BAKE_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("atlas_points", "dilate", "bake_lightmap"):
        assert callable(getattr(runtime, name, None)), name


def test_bake_layouts_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.Atlas) == 48 and C.sizeof(api.AtlasTexel) == 16
    assert api.ABI_SIZES[api.Atlas] == 48 and api.ABI_SIZES[api.AtlasTexel] == 16
    for f, off in ATLAS_OFFSETS.items():
        assert getattr(api.Atlas, f).offset == off, f
    for f, off in TEXEL_OFFSETS.items():
        assert getattr(api.AtlasTexel, f).offset == off, f
        assert api.ATLAS_TEXEL_DTYPE.fields[f][1] == off, f
    assert api.ATLAS_TEXEL_DTYPE.itemsize == 16
    items = ["sizeof ( TerraAmdAtlas )"] + [f"offsetof ( TerraAmdAtlas, {f} )" for f in ATLAS_OFFSETS]
    items += ["sizeof ( TerraAmdAtlasTexel )"] + [f"offsetof ( TerraAmdAtlasTexel, {f} )" for f in TEXEL_OFFSETS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [48] + list(ATLAS_OFFSETS.values()) + [16] + list(TEXEL_OFFSETS.values())


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_atlas_points_device ) ( HTerraScene, const TerraAmdAtlas*, const void*, void*, void*, void* ) = terra_amd_atlas_points_device;
static int ( *const p_atlas_points ) ( HTerraScene, const TerraAmdAtlas*, const float*, TerraAmdPoint*, TerraAmdAtlasTexel* ) = terra_amd_atlas_points;
static int ( *const p_dilate_device ) ( void*, int, void*, int, int, int, void* ) = terra_amd_dilate_device;
static int ( *const p_dilate ) ( float*, int, int*, int, int, int ) = terra_amd_dilate;
int main ( void ) {
    printf ( "%d\\n", p_atlas_points_device != 0 && p_atlas_points != 0 && p_dilate_device != 0 && p_dilate != 0 );
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


def atlas_of(width=4, height=4, uv_scale=(1.0, 1.0), uv_offset=(0.0, 0.0), margin=0.5, reserved=(0, 0, 0, 0, 0)):
    a = api.Atlas()
    a.width, a.height, a.margin = width, height, margin
    a.uv_scale[:] = uv_scale
    a.uv_offset[:] = uv_offset
    a.reserved[:] = reserved
    return a


class Buffers:
    """guard-filled outputs of a 4 x 4 atlas: 16-byte aligned points (and the same buffer 4 bytes on), texel records"""

    def __init__(self):
        self.raw = np.full(16 * 8 + 8, GUARD, np.uint32)
        at = ((-self.raw.ctypes.data) % 16) // 4
        self.points = self.raw.ctypes.data + 4 * at
        self.odd = self.points + 4
        self.texels = np.full(16 * 4, GUARD, np.uint32)

    def untouched(self):
        return bool((self.raw == GUARD).all() and (self.texels == GUARD).all())


def atlas_forms(lib, scene, atlas, points, texels):
    pa = C.byref(atlas) if atlas is not None else None
    return [lambda: lib.atlas_points_device(scene, pa, None, points, texels, None),
            lambda: lib.atlas_points(scene, pa, None, points, texels)]


def test_uncommitted_scene_is_refused_first(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    b = Buffers()
    try:
        for atlas, pts in ((atlas_of(), b.points), (atlas_of(width=0), b.points), (None, None)):          # "not committed" comes before anything else is looked at
            for k, call in enumerate(atlas_forms(lib, scene, atlas, pts, b.texels.ctypes.data)):
                lib.clear_error()
                assert call() == ERR_NOT_COMMITTED, k
                assert runtime.last_error() != ""
        assert b.untouched()
    finally:
        lib.clear_error()
        lib.scene_destroy(scene)


INF, NAN = float("inf"), float("nan")
BAD_ATLASES = {"width 0": dict(width=0), "width 16385": dict(width=16385), "height 0": dict(height=0), "height -3": dict(height=-3), "height 16385": dict(height=16385),
               "scale x inf": dict(uv_scale=(INF, 1.0)), "scale y nan": dict(uv_scale=(1.0, NAN)), "offset x nan": dict(uv_offset=(NAN, 0.0)), "offset y -inf": dict(uv_offset=(0.0, -INF)),
               "margin nan": dict(margin=NAN), "margin inf": dict(margin=INF), "margin below 0": dict(margin=-0.25), "margin above 4": dict(margin=4.5),
               "reserved 0": dict(reserved=(1, 0, 0, 0, 0)), "reserved 2": dict(reserved=(0, 0, -1, 0, 0)), "reserved 4": dict(reserved=(0, 0, 0, 0, 7))}


def test_bad_atlas_arguments_are_refused(amd_lib):
    """on a committed scene, with or without a device: every argument is checked before the call asks for the scene's device replica"""
    lib = runtime.load(need_torch=False)
    lib.clear_error()
    scene = scenes.build_scene(lib, scenes.cornell_box(4, 4, 1))
    b = Buffers()
    try:
        cases = {name: (atlas_of(**kw), b.points) for name, kw in BAD_ATLASES.items()}
        cases["null atlas"] = (None, b.points)
        cases["null points"] = (atlas_of(), None)
        cases["misaligned points"] = (atlas_of(), b.odd)
        for name, (atlas, pts) in cases.items():
            for k, call in enumerate(atlas_forms(lib, scene, atlas, pts, b.texels.ctypes.data)):
                lib.clear_error()
                assert call() == ERR_BAD_ARGUMENT, (name, k, runtime.last_error())
                assert runtime.last_error() != "", (name, k)
        assert b.untouched()
        # the edges of the ranges are good: whatever these calls answer without a device, it is not "bad argument"; NULL texels are allowed
        for atlas, tex in ((atlas_of(1, 1, margin=0.0), b.texels.ctypes.data), (atlas_of(4, 4, margin=4.0), None)):
            lib.clear_error()
            assert lib.atlas_points(scene, C.byref(atlas), None, b.points, tex) != ERR_BAD_ARGUMENT, runtime.last_error()
    finally:
        lib.clear_error()
        lib.scene_destroy(scene)


def test_bad_dilate_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    data = np.full(5 * 4 * 4, GUARD, np.uint32)
    valid = np.full(5 * 4, GUARD, np.uint32)
    d, v = data.ctypes.data, valid.ctypes.data
    cases = {"null data": (None, 3, v, 5, 4, 1), "null valid": (d, 3, None, 5, 4, 1), "channels 0": (d, 0, v, 5, 4, 1), "channels 5": (d, 5, v, 5, 4, 1),
             "width 0": (d, 3, v, 0, 4, 1), "width -1": (d, 3, v, -1, 4, 1), "height 0": (d, 3, v, 5, 0, 1), "height -2": (d, 3, v, 5, -2, 1),
             "passes -1": (d, 3, v, 5, 4, -1), "passes 65": (d, 3, v, 5, 4, 65)}
    try:
        for name, args in cases.items():
            for k, call in enumerate((lambda: lib.dilate_device(*args, None), lambda: lib.dilate(*args))):
                lib.clear_error()
                assert call() == ERR_BAD_ARGUMENT, (name, k, runtime.last_error())
                assert runtime.last_error() != "", (name, k)
        # passes = 0 writes nothing and needs no device
        lib.clear_error()
        assert lib.dilate(d, 4, v, 5, 4, 0) == 0 and lib.dilate_device(d, 1, v, 5, 4, 0, None) == 0 and runtime.last_error() == ""
        assert (data == GUARD).all() and (valid == GUARD).all()
    finally:
        lib.clear_error()


def test_headless_bake_flag_against_the_reference_is_reported_and_ignored(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm
    exe = build_tool(H, tmp_path, "ref")
    obj = tmp_path / "q.obj"
    obj.write_text("".join(f"v {x} {y} {z}\n" for x in (0, 1) for y in (0, 1) for z in (2, 3)) + "f 1 2 4 3\nf 5 7 8 6\nf 1 5 6 2\nf 3 4 8 7\nf 1 3 7 5\nf 2 6 8 4\n")
    args = ["--width", "16", "--height", "12", "--spp", "1", "--integrator", "normals", "--tonemap", "none"]
    for out, extra in (("plain.pfm", []), ("bake.pfm", ["--bake-lightmap", "--atlas", "8x8", "--bake-margin", "1", "--bake-dilate", "3"])):
        r = subprocess.run([str(exe), str(obj), str(tmp_path / out)] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert ("--bake-lightmap needs libterra_amd.so" in r.stderr) == bool(extra)
    assert np.array_equal(read_pfm(tmp_path / "bake.pfm"), read_pfm(tmp_path / "plain.pfm")) and read_pfm(tmp_path / "bake.pfm").shape == (12, 16, 3)


def test_headless_help_names_the_bake_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--bake-lightmap", "--atlas", "--bake-margin", "--bake-dilate"):
        assert flag in r.stdout, flag
