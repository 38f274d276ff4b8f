"""Probe visibility at the C boundary, without a GPU (include/terra_amd.h "Probe visibility"): the four entry points are exported and terra_amd/api.py carries their
signatures in PROBE_VISIBILITY_SIGNATURES, TerraAmdProbeVisibility and TerraAmdVisibilityTexel have the pinned layout in C and in the ctypes mirror, a gcc-compiled
probe of the spelled-out prototypes links, every bad argument is refused before the call asks for a device with the guard-filled buffers untouched, the runtime
helpers exist and the headless tool's --help names the two flags."""
import ctypes as C
import subprocess

import numpy as np

from terra_amd import api, runtime

SYMBOLS = ("terra_amd_probe_visibility_device", "terra_amd_probe_visibility", "terra_amd_sh_irradiance_visible_device", "terra_amd_sh_irradiance_visible")
OPTION_OFFSETS = {"texels": 0, "sharpness": 4, "max_distance": 8, "bias": 12, "flags": 16, "reserved": 20}
TEXEL_OFFSETS = {"weight": 0, "distance": 4, "distance2": 8, "cells": 12}
ERR_BAD_ARGUMENT = -4
GUARD = 0x5ca1ab1e
INF, NAN = float("inf"), float("nan")


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.PROBE_VISIBILITY_SIGNATURES) == set(SYMBOLS)
    assert not set(api.PROBE_VISIBILITY_SIGNATURES) & set(api.PROBE_SIGNATURES)
    lib = runtime.load(need_torch=False)
    for name in SYMBOLS:
        f = getattr(lib, name[len("terra_amd_"):])
        res, args = api.PROBE_VISIBILITY_SIGNATURES[name]
        assert f.restype is res and list(f.argtypes) == list(args), name
    for name in ("probe_visibility_options", "probe_visibility", "sh_irradiance_visible", "bake_probe_visibility"):
        assert callable(getattr(runtime, name, None)), name
    o = runtime.probe_visibility_options(texels=4, sharpness=3, max_distance=2.5, bias=0.125, backface=True)
    assert (o.texels, o.sharpness, o.max_distance, o.bias, o.flags, tuple(o.reserved)) == (4, 3, 2.5, 0.125, 1, (0, 0, 0))
    assert runtime.probe_visibility_options().flags == 0


def test_visibility_layouts_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.ProbeVisibility) == 32 and C.sizeof(api.VisibilityTexel) == 16
    assert api.ABI_SIZES[api.ProbeVisibility] == 32 and api.ABI_SIZES[api.VisibilityTexel] == 16
    for f, off in OPTION_OFFSETS.items():
        assert getattr(api.ProbeVisibility, f).offset == off, f
    for f, off in TEXEL_OFFSETS.items():
        assert getattr(api.VisibilityTexel, f).offset == off and api.VISIBILITY_TEXEL_DTYPE.fields[f][1] == off, f
    assert api.VISIBILITY_TEXEL_DTYPE.itemsize == 16 and api.VISIBILITY_TEXEL_DTYPE.fields["cells"][0] == np.int32
    items = ["sizeof ( TerraAmdProbeVisibility )"] + [f"offsetof ( TerraAmdProbeVisibility, {f} )" for f in OPTION_OFFSETS]
    items += ["sizeof ( TerraAmdVisibilityTexel )"] + [f"offsetof ( TerraAmdVisibilityTexel, {f} )" for f in TEXEL_OFFSETS] + ["kTerraAmdProbeVisibilityBackface"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == [32] + list(OPTION_OFFSETS.values()) + [16] + list(TEXEL_OFFSETS.values()) + [1]


PROBE = """
#include <stdio.h>
#include "terra_amd.h"
/* the prototypes, spelled out: an assignment to a pointer of another type is a constraint violation (-Werror) */
static int ( *const p_project_device ) ( const void*, const void*, size_t, int, const TerraAmdProbeVisibility*, int, void*, void* ) = terra_amd_probe_visibility_device;
static int ( *const p_project ) ( const TerraAmdHit*, const TerraAmdRay*, size_t, int, const TerraAmdProbeVisibility*, int, TerraAmdVisibilityTexel* ) = terra_amd_probe_visibility;
static int ( *const p_visible_device ) ( const void*, const void*, size_t, const TerraAmdProbeGrid*, const TerraAmdProbeVisibility*, const void*, size_t, void*, void* ) = terra_amd_sh_irradiance_visible_device;
static int ( *const p_visible ) ( const TerraAmdProbeSH*, const TerraAmdVisibilityTexel*, size_t, const TerraAmdProbeGrid*, const TerraAmdProbeVisibility*, const TerraAmdPoint*, size_t, float* ) = terra_amd_sh_irradiance_visible;
int main ( void ) {
    printf ( "%d\\n", p_project_device != 0 && p_project != 0 && p_visible_device != 0 && p_visible != 0 );
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
    """guard-filled, 16-byte aligned buffers of 3 probes x 2 x 2 cells, maps of up to 16 x 16 texels and 5 queries; .odd(name) is the same buffer 4 bytes on"""
    WORDS = {"hits": 12 * 8, "rays": 12 * 8, "map": 3 * 256 * 4, "sh": 3 * 28, "points": 5 * 8, "out": 5 * 4}

    def __init__(self):
        self.raw = {k: np.full(n + 8, GUARD, np.uint32) for k, n in self.WORDS.items()}
        self.at = {k: a.ctypes.data + (-a.ctypes.data) % 16 for k, a in self.raw.items()}

    def __getitem__(self, name):
        return self.at[name]

    def odd(self, name):
        return self.at[name] + 4

    def untouched(self):
        return all(bool((a == GUARD).all()) for a in self.raw.values())


def options_of(texels=2, sharpness=6, max_distance=10.0, bias=0.0, flags=0, reserved=(0, 0, 0)):
    o = api.ProbeVisibility()
    o.texels, o.sharpness, o.max_distance, o.bias, o.flags = texels, sharpness, max_distance, bias, flags
    o.reserved[:] = reserved
    return o


def grid_of(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), counts=(3, 1, 1), reserved=(0, 0, 0)):
    g = api.ProbeGrid()
    g.origin[:] = origin
    g.spacing[:] = spacing
    g.nx, g.ny, g.nz = counts
    g.reserved[:] = reserved
    return g


BAD_OPTIONS = {"texels 0": dict(texels=0), "texels -1": dict(texels=-1), "texels 17": dict(texels=17), "sharpness -1": dict(sharpness=-1), "sharpness 9": dict(sharpness=9),
               "max_distance 0": dict(max_distance=0.0), "max_distance -1": dict(max_distance=-1.0), "max_distance inf": dict(max_distance=INF), "max_distance nan": dict(max_distance=NAN),
               "bias -1": dict(bias=-1.0), "bias inf": dict(bias=INF), "bias nan": dict(bias=NAN), "flags 2": dict(flags=2), "flags 3": dict(flags=3), "flags -1": dict(flags=-1),
               "flags 1 << 31": dict(flags=-2 ** 31), "reserved 0": dict(reserved=(1, 0, 0)), "reserved 2": dict(reserved=(0, 0, -7))}
BAD_GRIDS = {"nx 0": dict(counts=(0, 1, 3)), "ny -1": dict(counts=(3, -1, 1)), "nz 0": dict(counts=(3, 1, 0)), "product 6": dict(counts=(3, 2, 1)), "product 2": dict(counts=(2, 1, 1)),
             "product overflows": dict(counts=(65536, 65536, 3)), "spacing x 0": dict(spacing=(0.0, 1.0, 1.0)), "spacing y nan": dict(spacing=(1.0, NAN, 1.0)),
             "spacing z inf": dict(spacing=(1.0, 1.0, INF)), "origin x nan": dict(origin=(NAN, 0.0, 0.0)), "origin z -inf": dict(origin=(0.0, 0.0, -INF)),
             "reserved 0": dict(reserved=(1, 0, 0)), "reserved 2": dict(reserved=(0, 0, -7))}


def refused(lib, cases, b):
    for name, call in cases.items():
        lib.clear_error()
        assert call() == ERR_BAD_ARGUMENT, (name, runtime.last_error())
        assert runtime.last_error() != "", name
    assert b.untouched()
    lib.clear_error()


def ref(o):
    return C.byref(o) if o is not None else None


def test_bad_probe_visibility_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    b = Buffers()
    forms = (("device", lambda h, r, n, c, o, acc, m: lib.probe_visibility_device(h, r, n, c, ref(o), acc, m, None)),
             ("host", lambda h, r, n, c, o, acc, m: lib.probe_visibility(h, r, n, c, ref(o), acc, m)))
    cases = {}
    for form, call in forms:
        good = options_of()
        bad = {"null hits": (None, b["rays"], 3, 2, good, 0, b["map"]), "null rays": (b["hits"], None, 3, 2, good, 0, b["map"]), "null map": (b["hits"], b["rays"], 3, 2, good, 1, None),
               "null options": (b["hits"], b["rays"], 3, 2, None, 0, b["map"]), "odd hits": (b.odd("hits"), b["rays"], 3, 2, good, 0, b["map"]),
               "odd rays": (b["hits"], b.odd("rays"), 3, 2, good, 0, b["map"]), "odd map": (b["hits"], b["rays"], 3, 2, good, 0, b.odd("map")),
               "cells 0": (b["hits"], b["rays"], 3, 0, good, 0, b["map"]), "cells -1": (b["hits"], b["rays"], 3, -1, good, 0, b["map"]), "cells 65": (b["hits"], b["rays"], 3, 65, good, 0, b["map"]),
               "too many rays": (b["hits"], b["rays"], 2 ** 31 // 4, 2, good, 0, b["map"]), "too many rays at 64": (b["hits"], b["rays"], 2 ** 19, 64, good, 0, b["map"]),
               "too many texels": (b["hits"], b["rays"], 2 ** 23, 1, options_of(texels=16), 0, b["map"]), "null hits, none asked": (None, b["rays"], 0, 2, good, 0, b["map"])}
        for name, kw in BAD_OPTIONS.items():
            bad["options " + name] = (b["hits"], b["rays"], 3, 2, options_of(**kw), 0, b["map"])
        for name, args in bad.items():
            cases[f"{form}: {name}"] = (lambda call=call, args=args: call(*args))
    refused(lib, cases, b)
    for form, call in forms:          # no probes: nothing to do, no device needed
        assert call(b["hits"], b["rays"], 0, 64, options_of(texels=16, sharpness=8, flags=1), 1, b["map"]) == 0 and runtime.last_error() == "", form
    # the edges are good: whatever these answer without a device, it is not "bad argument"
    for kw in (dict(texels=1, sharpness=0), dict(texels=16, sharpness=8, bias=3.0, flags=1), dict(max_distance=3e38)):
        lib.clear_error()
        assert lib.probe_visibility(b["hits"], b["rays"], 3, 2, ref(options_of(**kw)), 0, b["map"]) != ERR_BAD_ARGUMENT, (kw, runtime.last_error())
    lib.clear_error()


def test_bad_sh_irradiance_visible_arguments_are_refused(amd_lib):
    lib = runtime.load(need_torch=False)
    b = Buffers()
    forms = (("device", lambda sh, m, p, g, o, pts, n, out: lib.sh_irradiance_visible_device(sh, m, p, ref(g), ref(o), pts, n, out, None)),
             ("host", lambda sh, m, p, g, o, pts, n, out: lib.sh_irradiance_visible(sh, m, p, ref(g), ref(o), pts, n, out)))
    cases = {}
    for form, call in forms:
        good, grid = options_of(), grid_of()
        bad = {"null sh": (None, b["map"], 3, grid, good, b["points"], 5, b["out"]), "null map": (b["sh"], None, 3, grid, good, b["points"], 5, b["out"]),
               "null grid": (b["sh"], b["map"], 3, None, good, b["points"], 5, b["out"]), "null options": (b["sh"], b["map"], 3, grid, None, b["points"], 5, b["out"]),
               "null points": (b["sh"], b["map"], 3, grid, good, None, 5, b["out"]), "null out": (b["sh"], b["map"], 3, grid, good, b["points"], 5, None),
               "odd sh": (b.odd("sh"), b["map"], 3, grid, good, b["points"], 5, b["out"]), "odd map": (b["sh"], b.odd("map"), 3, grid, good, b["points"], 5, b["out"]),
               "odd points": (b["sh"], b["map"], 3, grid, good, b.odd("points"), 5, b["out"]), "too many queries": (b["sh"], b["map"], 3, grid, good, b["points"], 2 ** 31, b["out"]),
               "too many texels": (b["sh"], b["map"], 2 ** 23, grid_of(counts=(2 ** 23, 1, 1)), options_of(texels=16), b["points"], 5, b["out"]),
               "probes 4 for a grid of 3": (b["sh"], b["map"], 4, grid, good, b["points"], 5, b["out"])}
        if form == "device":
            bad["odd out"] = (b["sh"], b["map"], 3, grid, good, b["points"], 5, b.odd("out"))
        for name, kw in BAD_GRIDS.items():
            bad["grid " + name] = (b["sh"], b["map"], 3, grid_of(**kw), good, b["points"], 5, b["out"])
        for name, kw in BAD_OPTIONS.items():
            bad["options " + name] = (b["sh"], b["map"], 3, grid, options_of(**kw), b["points"], 5, b["out"])
        for name, args in bad.items():
            cases[f"{form}: {name}"] = (lambda call=call, args=args: call(*args))
    refused(lib, cases, b)
    for form, call in forms:          # no queries: nothing to do; a negative spacing is a grid like any other
        assert call(b["sh"], b["map"], 3, grid_of(spacing=(-1.0, 2.0, 0.5)), options_of(texels=16, flags=1, bias=0.5), b["points"], 0, b["out"]) == 0 and runtime.last_error() == "", form
    lib.clear_error()
    assert lib.sh_irradiance_visible(b["sh"], b["map"], 3, ref(grid_of()), ref(options_of()), b["points"], 5, b.odd("out")) != ERR_BAD_ARGUMENT, runtime.last_error()          # (the host form's output is plain floats)
    lib.clear_error()


def test_headless_help_names_the_visibility_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--probe-visibility", "--probe-texels"):
        assert flag in r.stdout, flag
    for bad in (["--bake-probes", "2x1x1", "--probe-visibility", str(tmp_path / "v.pfm"), "--probe-texels", "0"], ["--probe-texels", "17"]):
        r = subprocess.run([str(exe), "none.obj", str(tmp_path / "o.pfm")] + bad, capture_output=True, text=True)
        assert r.returncode == 64, bad
