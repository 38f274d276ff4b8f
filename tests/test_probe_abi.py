"""Probe harmonics at the C boundary, without a GPU (include/terra_amd.h "Probe harmonics"): the seven entry points are exported and terra_amd/api.py carries their
signatures, TerraAmdProbeSH and TerraAmdProbeGrid have the pinned layout in C and in the ctypes mirror, a gcc-compiled probe of the spelled-out prototypes links,
every bad argument is refused before the call asks for a device with the guard-filled outputs untouched, terra_amd_probe_grid_points lays a grid out on the host,
the runtime helpers exist and the headless tool's --help names the two flags."""
import ctypes as C
import subprocess

import numpy as np

from terra_amd import api, runtime

SYMBOLS = ("terra_amd_probe_rays_device", "terra_amd_probe_rays", "terra_amd_sh_project_device", "terra_amd_sh_project", "terra_amd_sh_irradiance_device",
           "terra_amd_sh_irradiance", "terra_amd_probe_grid_points")
GRID_OFFSETS = {"origin": 0, "nx": 12, "spacing": 16, "ny": 28, "nz": 32, "reserved": 36}
ERR_BAD_ARGUMENT = -4
GUARD = 0x5ca1ab1e
INF, NAN = float("inf"), float("nan")


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.PROBE_SIGNATURES) == set(SYMBOLS)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.PROBE_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("probe_rays", "sh_project", "sh_irradiance", "probe_grid", "bake_probes"):
        assert callable(getattr(runtime, name, None)), name


def test_probe_layouts_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.ProbeSH) == 112 and C.sizeof(api.ProbeGrid) == 48
    assert api.ABI_SIZES[api.ProbeSH] == 112 and api.ABI_SIZES[api.ProbeGrid] == 48
    assert api.ProbeSH.c.offset == 0 and api.ProbeSH.cells.offset == 108
    assert api.PROBE_SH_DTYPE.itemsize == 112 and api.PROBE_SH_DTYPE.fields["c"][1] == 0 and api.PROBE_SH_DTYPE.fields["cells"][1] == 108
    assert api.PROBE_SH_DTYPE.fields["c"][0].shape == (9, 3)
    for f, off in GRID_OFFSETS.items():
        assert getattr(api.ProbeGrid, f).offset == off, f
    items = ["sizeof ( TerraAmdProbeSH )", "offsetof ( TerraAmdProbeSH, c )", "offsetof ( TerraAmdProbeSH, cells )", "sizeof ( ( ( TerraAmdProbeSH* ) 0 )->c[0] )"]
    items += ["sizeof ( TerraAmdProbeGrid )"] + [f"offsetof ( TerraAmdProbeGrid, {f} )" for f in GRID_OFFSETS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [112, 0, 108, 12, 48] + list(GRID_OFFSETS.values())


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_rays_device ) ( const void*, size_t, int, const void*, void*, void* ) = terra_amd_probe_rays_device;
static int ( *const p_rays ) ( const TerraAmdPoint*, size_t, int, const float*, TerraAmdRay* ) = terra_amd_probe_rays;
static int ( *const p_project_device ) ( const void*, const void*, size_t, int, int, void*, void* ) = terra_amd_sh_project_device;
static int ( *const p_project ) ( const TerraFramebuffer*, const TerraAmdRay*, size_t, int, int, TerraAmdProbeSH* ) = terra_amd_sh_project;
static int ( *const p_irradiance_device ) ( const void*, size_t, const TerraAmdProbeGrid*, const void*, const void*, size_t, void*, void* ) = terra_amd_sh_irradiance_device;
static int ( *const p_irradiance ) ( const TerraAmdProbeSH*, size_t, const TerraAmdProbeGrid*, const TerraAmdPoint*, const int*, size_t, float* ) = terra_amd_sh_irradiance;
static int ( *const p_grid_points ) ( const TerraAmdProbeGrid*, TerraAmdPoint*, int ) = terra_amd_probe_grid_points;
int main ( void ) {
    printf ( "%d\\n", p_rays_device != 0 && p_rays != 0 && p_project_device != 0 && p_project != 0 && p_irradiance_device != 0 && p_irradiance != 0 && p_grid_points != 0 );
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


class Buffers:
    """guard-filled, 16-byte aligned buffers of a frame of 3 probes x 2 x 2 cells and of 5 queries; .odd(name) is the same buffer 4 bytes on"""
    WORDS = {"probes": 3 * 8, "rays": 12 * 8, "results": 12 * 4, "pixels": 12 * 3, "sh": 3 * 28, "points": 5 * 8, "index": 5, "out": 5 * 4, "jitter": 8}

    def __init__(self):
        self.raw = {k: np.full(n + 8, GUARD, np.uint32) for k, n in self.WORDS.items()}
        self.at = {k: a.ctypes.data + (-a.ctypes.data) % 16 for k, a in self.raw.items()}

    def __getitem__(self, name):
        return self.at[name]

    def odd(self, name):
        return self.at[name] + 4

    def untouched(self):
        return all(bool((a == GUARD).all()) for a in self.raw.values())

    def framebuffer(self, width=4, height=3, results="results"):
        fb = api.TerraFramebuffer()
        fb.pixels = C.cast(self.at["pixels"], C.POINTER(api.TerraFloat3))
        fb.results = C.cast(self.at[results] if results else None, type(fb.results))
        fb.width, fb.height = width, height
        return fb


def grid_of(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), counts=(3, 1, 1), reserved=(0, 0, 0)):
    g = api.ProbeGrid()
    g.origin[:] = origin
    g.spacing[:] = spacing
    g.nx, g.ny, g.nz = counts
    g.reserved[:] = reserved
    return g


def refused(lib, cases, b):
    for name, call in cases.items():
        lib.clear_error()
        assert call() == ERR_BAD_ARGUMENT, (name, runtime.last_error())
        assert runtime.last_error() != "", name
    assert b.untouched()
    lib.clear_error()


def test_bad_probe_rays_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    b = Buffers()
    cases = {}
    for form, call in (("device", lambda p, n, c, j, r: lib.probe_rays_device(p, n, c, j, r, None)), ("host", lambda p, n, c, j, r: lib.probe_rays(p, n, c, j, r))):
        for name, args in {"null probes": (None, 3, 2, None, b["rays"]), "null rays": (b["probes"], 3, 2, None, None), "odd probes": (b.odd("probes"), 3, 2, None, b["rays"]),
                           "odd rays": (b["probes"], 3, 2, None, b.odd("rays")), "cells 0": (b["probes"], 3, 0, None, b["rays"]), "cells -1": (b["probes"], 3, -1, b["jitter"], b["rays"]),
                           "cells 65": (b["probes"], 3, 65, None, b["rays"]), "too many rays": (b["probes"], 2 ** 31 // 4, 2, None, b["rays"]),
                           "too many rays at 64": (b["probes"], 2 ** 19, 64, None, b["rays"]), "null probes, none asked": (None, 0, 2, None, b["rays"])}.items():
            cases[f"{form}: {name}"] = (lambda call=call, args=args: call(*args))
    refused(lib, cases, b)
    # no probes: nothing to do, no device needed
    assert lib.probe_rays(b["probes"], 0, 2, None, b["rays"]) == 0 and lib.probe_rays_device(b["probes"], 0, 64, b["jitter"], b["rays"], None) == 0 and runtime.last_error() == ""
    # the edges are good: whatever these answer without a device, it is not "bad argument"
    for cells, probes in ((1, 3), (2, 3)):
        lib.clear_error()
        assert lib.probe_rays(b["probes"], probes, cells, None, b["rays"]) != ERR_BAD_ARGUMENT, runtime.last_error()
    lib.clear_error()


def test_bad_sh_project_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    b = Buffers()
    dev = lambda res, rays, n, c, batch, sh: lib.sh_project_device(res, rays, n, c, batch, sh, None)
    cases = {}
    for name, args in {"null results": (None, b["rays"], 3, 2, 0, b["sh"]), "null rays": (b["results"], None, 3, 2, 0, b["sh"]), "null sh": (b["results"], b["rays"], 3, 2, 0, None),
                       "odd results": (b.odd("results"), b["rays"], 3, 2, 0, b["sh"]), "odd rays": (b["results"], b.odd("rays"), 3, 2, 0, b["sh"]), "odd sh": (b["results"], b["rays"], 3, 2, 0, b.odd("sh")),
                       "cells 0": (b["results"], b["rays"], 3, 0, 0, b["sh"]), "cells 65": (b["results"], b["rays"], 3, 65, 0, b["sh"]), "batch -1": (b["results"], b["rays"], 3, 2, -1, b["sh"]),
                       "too many cells": (b["results"], b["rays"], 2 ** 31 // 4, 2, 0, b["sh"])}.items():
        cases["device: " + name] = (lambda args=args: dev(*args))
    host = lambda fb, rays, n, c, batch, sh: lib.sh_project(C.byref(fb) if fb is not None else None, rays, n, c, batch, sh)
    for name, args in {"null framebuffer": (None, b["rays"], 3, 2, 0, b["sh"]), "null results": (b.framebuffer(results=None), b["rays"], 3, 2, 0, b["sh"]),
                       "null rays": (b.framebuffer(), None, 3, 2, 0, b["sh"]), "null sh": (b.framebuffer(), b["rays"], 3, 2, 0, None), "odd rays": (b.framebuffer(), b.odd("rays"), 3, 2, 0, b["sh"]),
                       "odd sh": (b.framebuffer(), b["rays"], 3, 2, 0, b.odd("sh")), "cells 0": (b.framebuffer(), b["rays"], 3, 0, 0, b["sh"]), "cells 65": (b.framebuffer(), b["rays"], 3, 65, 0, b["sh"]),
                       "batch -1": (b.framebuffer(), b["rays"], 3, 2, -1, b["sh"]), "frame too narrow": (b.framebuffer(3, 3), b["rays"], 3, 2, 0, b["sh"]),
                       "frame too high": (b.framebuffer(4, 4), b["rays"], 3, 2, 0, b["sh"]), "frame transposed": (b.framebuffer(3, 4), b["rays"], 3, 2, 0, b["sh"]),
                       "frame of another cell count": (b.framebuffer(4, 3), b["rays"], 3, 1, 0, b["sh"])}.items():
        cases["host: " + name] = (lambda args=args: host(*args))
    refused(lib, cases, b)
    assert dev(b["results"], b["rays"], 0, 2, 3, b["sh"]) == 0 and host(b.framebuffer(4, 0), b["rays"], 0, 2, 0, b["sh"]) == 0 and runtime.last_error() == ""
    lib.clear_error()
    assert host(b.framebuffer(), b["rays"], 3, 2, 2, b["sh"]) != ERR_BAD_ARGUMENT, runtime.last_error()
    lib.clear_error()


BAD_GRIDS = {"nx 0": dict(counts=(0, 1, 3)), "ny -1": dict(counts=(3, -1, 1)), "nz 0": dict(counts=(3, 1, 0)), "product 6": dict(counts=(3, 2, 1)), "product 2": dict(counts=(2, 1, 1)),
             "product overflows": dict(counts=(65536, 65536, 3)), "spacing x 0": dict(spacing=(0.0, 1.0, 1.0)), "spacing y nan": dict(spacing=(1.0, NAN, 1.0)),
             "spacing z inf": dict(spacing=(1.0, 1.0, INF)), "origin x nan": dict(origin=(NAN, 0.0, 0.0)), "origin z -inf": dict(origin=(0.0, 0.0, -INF)),
             "reserved 0": dict(reserved=(1, 0, 0)), "reserved 2": dict(reserved=(0, 0, -7))}


def test_bad_sh_irradiance_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    b = Buffers()
    forms = (("device", lambda sh, p, g, pts, idx, n, out: lib.sh_irradiance_device(sh, p, C.byref(g) if g is not None else None, pts, idx, n, out, None)),
             ("host", lambda sh, p, g, pts, idx, n, out: lib.sh_irradiance(sh, p, C.byref(g) if g is not None else None, pts, idx, n, out)))
    cases = {}
    for form, call in forms:
        bad = {"null sh": (None, 3, None, b["points"], b["index"], 5, b["out"]), "null points": (b["sh"], 3, None, None, b["index"], 5, b["out"]),
               "null index without a grid": (b["sh"], 3, None, b["points"], None, 5, b["out"]), "null out": (b["sh"], 3, None, b["points"], b["index"], 5, None),
               "odd sh": (b.odd("sh"), 3, None, b["points"], b["index"], 5, b["out"]), "odd points": (b["sh"], 3, grid_of(), b.odd("points"), None, 5, b["out"]),
               "too many queries": (b["sh"], 3, None, b["points"], b["index"], 2 ** 31, b["out"])}
        if form == "device":
            bad["odd out"] = (b["sh"], 3, None, b["points"], b["index"], 5, b.odd("out"))
        for name, kw in BAD_GRIDS.items():
            bad["grid " + name] = (b["sh"], 3, grid_of(**kw), b["points"], b["index"], 5, b["out"])
        for name, args in bad.items():
            cases[f"{form}: {name}"] = (lambda call=call, args=args: call(*args))
    refused(lib, cases, b)
    for form, call in forms:          # no queries: nothing to do; a negative spacing is a grid like any other
        assert call(b["sh"], 3, grid_of(spacing=(-1.0, 2.0, 0.5)), b["points"], None, 0, b["out"]) == 0 and runtime.last_error() == "", form
    lib.clear_error()
    assert lib.sh_irradiance(b["sh"], 3, grid_of(), b["points"], None, 5, b.odd("out")) != ERR_BAD_ARGUMENT, runtime.last_error()          # (the host form's output is plain floats)
    lib.clear_error()


def test_probe_grid_points_on_the_host(amd_lib):
    lib = runtime.load(need_torch=False)
    origin, spacing = (np.float32(0.1), np.float32(-2.0), np.float32(1e-3)), (np.float32(0.3), np.float32(0.7), np.float32(-1.1))
    g = grid_of(origin, spacing, (3, 2, 2))
    assert lib.probe_grid_points(C.byref(g), None, 0) == 12 and lib.probe_grid_points(C.byref(g), None, 5) == 12          # the count, whatever the capacity
    raw = np.full(12 * 8, GUARD, np.uint32)
    assert lib.probe_grid_points(C.byref(g), raw.ctypes.data, 0) == 12 and (raw == GUARD).all()
    assert lib.probe_grid_points(C.byref(g), raw.ctypes.data, 7) == 12 and (raw[7 * 8:] == GUARD).all() and (raw[:7 * 8] != GUARD).all()
    assert lib.probe_grid_points(C.byref(g), raw.ctypes.data, 100) == 12
    got = raw.view(api.POINT_DTYPE)
    want = np.zeros(12, api.POINT_DTYPE)
    for iz in range(2):
        for iy in range(2):
            for ix in range(3):
                at = (iz * 2 + iy) * 3 + ix
                want["position"][at] = [np.float32(np.float64(origin[a]) + np.float64(i) * np.float64(spacing[a])) for a, i in enumerate((ix, iy, iz))]
    want["normal"][:] = (0, 0, 1)
    assert got.tobytes() == want.tobytes()
    grid, points = runtime.probe_grid(lib, origin, spacing, (3, 2, 2))
    assert points.tobytes() == want.tobytes() and (grid.nx, grid.ny, grid.nz) == (3, 2, 2)
    _, centred = runtime.probe_grid_over(lib, (-1.0, 0.0, 2.0), (1.0, 0.0, 3.0), (2, 1, 4))          # a box with no extent on y
    assert np.array_equal(centred["position"][:2], np.array([[-0.5, 0.5, 2.125], [0.5, 0.5, 2.125]], np.float32)) and centred["position"][-1, 2] == np.float32(2.875)
    for name, kw in BAD_GRIDS.items():
        if name.startswith("product") and "overflows" not in name:
            continue
        lib.clear_error()
        bad = grid_of(**{"counts": (3, 1, 1), **kw})
        assert lib.probe_grid_points(C.byref(bad), raw.ctypes.data, 12) == ERR_BAD_ARGUMENT, name
    assert lib.probe_grid_points(None, raw.ctypes.data, 12) == ERR_BAD_ARGUMENT
    assert got.tobytes() == want.tobytes()
    lib.clear_error()


def test_headless_probe_flag_against_the_reference_is_reported_and_ignored(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm
    exe = build_tool(H, tmp_path, "ref")
    obj = tmp_path / "q.obj"
    obj.write_text("".join(f"v {x} {y} {z}\n" for x in (0, 1) for y in (0, 1) for z in (2, 3)) + "f 1 2 4 3\nf 5 7 8 6\nf 1 5 6 2\nf 3 4 8 7\nf 1 3 7 5\nf 2 6 8 4\n")
    args = ["--width", "16", "--height", "12", "--spp", "1", "--integrator", "normals", "--tonemap", "none"]
    for out, extra in (("plain.pfm", []), ("probes.pfm", ["--bake-probes", "2x1x1", "--probe-cells", "4"])):
        r = subprocess.run([str(exe), str(obj), str(tmp_path / out)] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert ("--bake-probes needs libterra_amd.so" in r.stderr) == bool(extra)
    assert np.array_equal(read_pfm(tmp_path / "probes.pfm"), read_pfm(tmp_path / "plain.pfm")) and read_pfm(tmp_path / "probes.pfm").shape == (12, 16, 3)


def test_headless_help_names_the_probe_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--bake-probes", "--probe-cells"):
        assert flag in r.stdout, flag
    for bad in (["--bake-probes", "2x2"], ["--bake-probes", "0x1x1"], ["--bake-probes", "2x1x1", "--probe-cells", "65"]):
        r = subprocess.run([str(exe), "none.obj", str(tmp_path / "o.pfm")] + bad, capture_output=True, text=True)
        assert r.returncode == 64, bad
