"""Point rendering at the C boundary, without a GPU (include/terra_amd.h "Point rendering"): the six entry points are exported and terra_amd/api.py carries their
signatures, TerraAmdPoint and TerraAmdPointSampling have the pinned layout in C and in the ctypes mirror, a gcc-compiled probe of the header links against the
spelled-out prototypes, an uncommitted scene is refused before anything touches a device, every bad argument is refused before the call asks for a device, and
terra_amd_scene_vertex_points hands back the vertices and normals the scene was built from."""
import ctypes as C
import subprocess

import numpy as np

from terra_amd import api, runtime, scenes

SYMBOLS = ("terra_amd_render_points_device", "terra_amd_render_points", "terra_amd_render_aov_points_device", "terra_amd_render_aov_points",
           "terra_amd_unit_point_rays", "terra_amd_scene_vertex_points")
POINT_OFFSETS = {"position": 0, "reserved": 12, "normal": 16, "reserved2": 28}
SAMPLING_OFFSETS = {"distribution": 0, "reserved": 4}
ERR_NOT_COMMITTED, ERR_BAD_ARGUMENT = -2, -4


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.POINT_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.POINT_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("render_points_device", "render_aov_points_device", "point_rays", "scene_vertex_points", "irradiance"):
        assert hasattr(runtime, name), name


def test_point_layouts_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.Point) == 32 and C.sizeof(api.PointSampling) == 16
    assert api.ABI_SIZES[api.Point] == 32 and api.ABI_SIZES[api.PointSampling] == 16
    for f, off in POINT_OFFSETS.items():
        assert getattr(api.Point, f).offset == off, f
        assert api.POINT_DTYPE.fields[f][1] == off, f
    assert api.POINT_DTYPE.itemsize == 32
    for f, off in SAMPLING_OFFSETS.items():
        assert getattr(api.PointSampling, f).offset == off, f
    items = ["sizeof ( TerraAmdPoint )"] + [f"offsetof ( TerraAmdPoint, {f} )" for f in POINT_OFFSETS]
    items += ["sizeof ( TerraAmdPointSampling )"] + [f"offsetof ( TerraAmdPointSampling, {f} )" for f in SAMPLING_OFFSETS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [32] + list(POINT_OFFSETS.values()) + [16] + list(SAMPLING_OFFSETS.values())


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_render_points_device ) ( HTerraScene, const TerraAmdPointSampling*, const void*, void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, void*, void* ) = terra_amd_render_points_device;
static int ( *const p_render_points ) ( HTerraScene, const TerraAmdPointSampling*, const TerraAmdPoint*, const TerraFramebuffer*, size_t, size_t, size_t, size_t ) = terra_amd_render_points;
static int ( *const p_render_aov_points_device ) ( HTerraScene, const TerraAmdPointSampling*, const void*, void*, size_t, size_t, size_t, size_t, size_t, size_t, void* ) = terra_amd_render_aov_points_device;
static int ( *const p_render_aov_points ) ( HTerraScene, const TerraAmdPointSampling*, const TerraAmdPoint*, TerraAmdAovResult*, size_t, size_t, size_t, size_t, size_t, size_t ) = terra_amd_render_aov_points;
static int ( *const p_unit_point_rays ) ( const TerraAmdPointSampling*, int, const TerraAmdPoint*, const float*, TerraAmdRay* ) = terra_amd_unit_point_rays;
static int ( *const p_scene_vertex_points ) ( HTerraScene, TerraAmdPoint*, int ) = terra_amd_scene_vertex_points;
int main ( void ) {
    printf ( "%d\\n", p_render_points_device != 0 && p_render_points != 0 && p_render_aov_points_device != 0 && p_render_aov_points != 0 && p_unit_point_rays != 0 && p_scene_vertex_points != 0 );
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


def sampling_of(distribution=0, reserved=(0, 0, 0)):
    ps = api.PointSampling()
    ps.distribution = distribution
    ps.reserved[:] = reserved
    return ps


def aligned_points(n, offset=0):
    """n api.POINT_DTYPE records (position 0, normal +y) whose first byte lies `offset` bytes past a 16-byte boundary; returns (keep-alive, address)"""
    raw = np.zeros(n * 32 + 32, np.uint8)
    at = (-raw.ctypes.data) % 16 + offset
    pts = raw[at:at + n * 32].view(np.float32).reshape(n, 8)
    pts[:, 5] = 1.0
    return raw, raw.ctypes.data + at


def four_forms(lib, ps, points, scene, fb, aov, rect=(0, 0, 4, 4)):
    """the four render forms on host memory (the device forms are refused before they look at a pointer)"""
    pp = C.byref(ps) if ps is not None else None
    x, y, w, h = rect
    return [lambda: lib.render_points_device(scene, pp, points, fb.pixels.ctypes.data, fb.results.ctypes.data, 4, 4, x, y, w, h, None, None),
            lambda: lib.render_points(scene, pp, points, C.byref(fb.fb), x, y, w, h),
            lambda: lib.render_aov_points_device(scene, pp, points, aov.ctypes.data, 4, 4, x, y, w, h, None),
            lambda: lib.render_aov_points(scene, pp, points, aov.ctypes.data, 4, 4, x, y, w, h)]


def test_uncommitted_scene_is_refused_without_a_device(amd_lib):
    lib = runtime.load(need_torch=False)
    scene = lib.scene_create()
    aov = np.zeros((4, 4), runtime.AOV_DTYPE)
    fb = api.Framebuffer(lib, 4, 4)
    keep, points = aligned_points(16)
    try:
        for ps, pts in ((sampling_of(0), points), (sampling_of(7), points), (None, None)):                # "not committed" comes first: before anything else is looked at
            for k, call in enumerate(four_forms(lib, ps, pts, scene, fb, aov)):
                lib.clear_error()
                assert call() == ERR_NOT_COMMITTED, k
                assert runtime.last_error() != ""
        lib.clear_error()
        out = np.zeros(4, api.POINT_DTYPE)
        assert lib.scene_vertex_points(scene, out.ctypes.data, 4) == ERR_NOT_COMMITTED and runtime.last_error() != ""
        assert not aov.view(np.uint8).any() and not fb.results.view(np.uint8).any() and not fb.pixels.view(np.uint32).any() and not out.view(np.uint8).any()
    finally:
        lib.clear_error()
        fb.destroy()
        lib.scene_destroy(scene)


BAD_SAMPLINGS = {"distribution -1": dict(distribution=-1), "distribution 2": dict(distribution=2), "reserved 0": dict(reserved=(1, 0, 0)), "reserved 1": dict(distribution=1, reserved=(0, -1, 0)),
                 "reserved 2": dict(reserved=(0, 0, 5))}
BAD_RECTS = {"empty width": (0, 0, 0, 4), "empty height": (0, 0, 4, 0), "past the right edge": (1, 0, 4, 4), "past the bottom edge": (0, 2, 4, 3)}


def test_bad_arguments_are_refused(amd_lib):
    """on a committed scene, with or without a device: every argument is checked before the call asks for the scene's device replica"""
    lib = runtime.load(need_torch=False)
    d = scenes.cornell_box(4, 4, 1)
    lib.clear_error()
    scene = scenes.build_scene(lib, d)
    aov = np.zeros((4, 4), runtime.AOV_DTYPE)
    fb = api.Framebuffer(lib, 4, 4)
    keep, points = aligned_points(16)
    keep_odd, odd = aligned_points(16, offset=4)
    g2 = np.zeros((1, 2), np.float32); out = np.zeros(1, api.RAY_DTYPE)
    try:
        good = sampling_of(0)
        cases = {name: (sampling_of(**kw), points, (0, 0, 4, 4)) for name, kw in BAD_SAMPLINGS.items()}
        cases["null sampling"] = (None, points, (0, 0, 4, 4))
        cases["null points"] = (good, None, (0, 0, 4, 4))
        cases["misaligned points"] = (good, odd, (0, 0, 4, 4))
        for name, rect in BAD_RECTS.items():
            cases[name] = (good, points, rect)
        for name, (ps, pts, rect) in cases.items():
            calls = four_forms(lib, ps, pts, scene, fb, aov, rect)
            if name in BAD_SAMPLINGS or name == "null sampling":
                calls.append(lambda: lib.unit_point_rays(C.byref(ps) if ps is not None else None, 1, points, g2.ctypes.data, out.ctypes.data))
            for k, call in enumerate(calls):
                lib.clear_error()
                assert call() == ERR_BAD_ARGUMENT, (name, k, runtime.last_error())
                assert runtime.last_error() != "", (name, k)
        # the unit entry's own arrays
        for args in ((1, None, g2.ctypes.data, out.ctypes.data), (1, points, None, out.ctypes.data), (1, points, g2.ctypes.data, None), (-1, points, g2.ctypes.data, out.ctypes.data)):
            lib.clear_error()
            assert lib.unit_point_rays(C.byref(good), *args) == ERR_BAD_ARGUMENT and runtime.last_error() != "", args
        assert not aov.view(np.uint8).any() and not fb.results.view(np.uint8).any() and not fb.pixels.view(np.uint32).any() and not out.view(np.uint8).any()
        # both distributions are good: whatever these calls answer without a device, it is not "bad argument"
        for dist in (0, 1):
            lib.clear_error()
            rc = lib.render_aov_points(scene, C.byref(sampling_of(dist)), points, aov.ctypes.data, 4, 4, 0, 0, 4, 4)
            assert rc != ERR_BAD_ARGUMENT, (dist, runtime.last_error())
    finally:
        lib.clear_error()
        fb.destroy()
        lib.scene_destroy(scene)


def test_scene_vertex_points_are_the_vertices_the_scene_was_built_from(amd_lib):
    lib = runtime.load(need_torch=False)
    d = scenes.cornell_box(4, 4, 1)
    lib.clear_error()
    scene = scenes.build_scene(lib, d)
    try:
        n = 3 * d.triangle_count
        assert lib.scene_vertex_points(scene, None, 0) == n == 96
        guard = np.full(n + 2, 0x5ca1ab1e, np.uint32).repeat(8).reshape(n + 2, 8)
        assert lib.scene_vertex_points(scene, guard.ctypes.data, 0) == n                     # capacity 0: the count, nothing written
        assert (guard == 0x5ca1ab1e).all()
        assert lib.scene_vertex_points(scene, guard.ctypes.data, 5) == n                     # a short buffer: the first records, nothing beyond them
        assert (guard[5:] == 0x5ca1ab1e).all() and (guard[:5] != 0x5ca1ab1e).any()
        out = np.zeros(n + 2, api.POINT_DTYPE)
        out.view(np.uint32).reshape(n + 2, 8)[n:] = 0x5ca1ab1e
        assert lib.scene_vertex_points(scene, out.ctypes.data, n + 2) == n
        assert (out.view(np.uint32).reshape(n + 2, 8)[n:] == 0x5ca1ab1e).all()
        want_pos = np.concatenate([np.asarray(o.triangles, np.float32).reshape(-1, 3) for o in d.objects])
        want_nrm = np.concatenate([np.asarray(o.normals, np.float32).reshape(-1, 3) for o in d.objects])
        assert out["position"][:n].tobytes() == want_pos.tobytes()
        assert out["normal"][:n].tobytes() == want_nrm.tobytes()
        assert not out["reserved"][:n].view(np.uint32).any() and not out["reserved2"][:n].view(np.uint32).any()
        assert out[:5].tobytes() == guard[:5].tobytes()
        assert runtime.scene_vertex_points(lib, scene).tobytes() == out[:n].tobytes()
    finally:
        lib.clear_error()
        lib.scene_destroy(scene)
