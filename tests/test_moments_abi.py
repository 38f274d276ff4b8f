"""Moments, tile error, the variance-guided denoiser and adaptive tiles at the C boundary, without a GPU: the entry points are exported, TerraAmdMoments and
the adaptive structures have the layout include/terra_amd.h pins (in C, in C++ and in the ctypes mirror), terra_headless offers the flags -- linked against
the compiled reference it says so and writes the plain image -- and the sanitizer harness' host stand-ins cover every launcher the host side calls."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from terra_amd import api, scenes

NEW = ("terra_amd_accumulate_moments_device", "terra_amd_accumulate_moments", "terra_amd_tile_error_device", "terra_amd_tile_error",
       "terra_amd_denoise_variance_device", "terra_amd_denoise_variance", "terra_amd_render_adaptive_device", "terra_amd_render_adaptive")
OFFSETS = {"seen_acc": 0, "seen_samples": 12, "mean": 16, "m2": 20, "batches": 24, "weight": 28}
OPT_OFFSETS = {"tile_size": 0, "min_batches": 8, "max_batches": 12, "target_error": 16, "reserved": 20}
REP_OFFSETS = {"rounds": 0, "hit_max_batches": 4, "tiles": 8, "tiles_converged": 12, "tile_calls": 16, "samples": 24, "max_error": 32, "reserved": 36}


def test_new_symbols_are_exported(amd_lib):
    for name in NEW:
        assert amd_lib.has(name), name
    out = subprocess.run(["nm", "-D", "--defined-only", amd_lib.path], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported


def test_runtime_binds_the_new_calls():
    from terra_amd import runtime
    for name in NEW:
        assert name in runtime._EXTRA, name
    for name in ("DeviceMoments", "accumulate_moments_device", "tile_error_device", "denoise_variance_device", "render_adaptive_device"):
        assert hasattr(runtime, name), name


@pytest.mark.parametrize("compiler, std, ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_layouts_in_c_cxx_and_ctypes(H, tmp_path, compiler, std, ext):
    assert C.sizeof(api.TerraAmdMoments) == 32 and api.MOMENTS_DTYPE.itemsize == 32
    for f, off in OFFSETS.items():
        assert getattr(api.TerraAmdMoments, f).offset == off, f
        assert api.MOMENTS_DTYPE.fields[f][1] == off, f
    for f, off in OPT_OFFSETS.items():
        assert getattr(api.TerraAmdAdaptiveOptions, f).offset == off, f
    for f, off in REP_OFFSETS.items():
        assert getattr(api.TerraAmdAdaptiveReport, f).offset == off, f
    items = ["sizeof ( TerraAmdMoments )"] + [f"offsetof ( TerraAmdMoments, {f} )" for f in OFFSETS]
    items += ["sizeof ( TerraAmdAdaptiveOptions )"] + [f"offsetof ( TerraAmdAdaptiveOptions, {f} )" for f in OPT_OFFSETS]
    items += ["sizeof ( TerraAmdAdaptiveReport )"] + [f"offsetof ( TerraAmdAdaptiveReport, {f} )" for f in REP_OFFSETS]
    src = tmp_path / f"layout.{ext}"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run([compiler, std, "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [32] + list(OFFSETS.values()) + [24] + list(OPT_OFFSETS.values()) + [40] + list(REP_OFFSETS.values())
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == want


def test_headless_help_lists_the_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    out = subprocess.run([str(exe), "--help"], capture_output=True, text=True).stdout
    for flag in ("--passes N", "--denoise-variance K", "--adaptive TARGET", "--min-passes A", "--max-passes B", "--variance out.pfm"):
        assert flag in out, flag


def test_headless_against_the_reference_says_so_and_writes_the_plain_image(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "ref")
    d = scenes.cornell_box(40, 30, 2)
    obj = tmp_path / "c.obj"
    write_obj(d, obj)
    args = ["--width", "40", "--height", "30", "--spp", "2", "--integrator", "normals", "--tonemap", "none"]
    plain = subprocess.run([str(exe), str(obj), str(tmp_path / "plain.pfm")] + args, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    for k, extra in enumerate((["--passes", "4", "--denoise-variance", "3", "--variance", str(tmp_path / "v.pfm")],
                               ["--adaptive", "0.05", "--min-passes", "2", "--max-passes", "4", "--variance", str(tmp_path / "v.pfm")])):
        r = subprocess.run([str(exe), str(obj), str(tmp_path / f"o{k}.pfm")] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "--passes / --denoise-variance / --adaptive / --variance need libterra_amd.so" in r.stderr
        assert np.array_equal(read_pfm(tmp_path / f"o{k}.pfm"), read_pfm(tmp_path / "plain.pfm"))
        assert not (tmp_path / "v.pfm").exists()


def test_sanitizer_stand_ins_cover_every_launcher(H, tmp_path):
    """the harness links the host layer against tools/sanitize/stub_launchers.cpp: every launcher kernels.h declares that the host layer calls is defined
    there, every terra_ function defined there is such a launcher, and the host layer plus the stand-ins link with no undefined terra_ symbol"""
    csrc = H.ROOT / "terra_amd" / "csrc"
    declared = set(re.findall(r"\b(terra_launch_\w+|terra_unit_\w+|terra_build_fast_tree_device|terra_fill_sincos24)\s*\(", (csrc / "kernels.h").read_text()))
    stubs = (H.ROOT / "tools" / "sanitize" / "stub_launchers.cpp").read_text()
    host = (csrc / "scene_host.cpp").read_text() + (csrc / "multi_gpu.cpp").read_text()
    for name in sorted(declared):
        if re.search(rf"\b{name}\s*\(", host):
            assert re.search(rf"\b{name}\s*\(", stubs), f"{name} has no stand-in"
    for name in ("terra_launch_moments_accumulate", "terra_launch_tile_error", "terra_launch_denoise_variance"):
        assert name in stubs
    # ... and the converse: the stand-in file defines launchers only -- how a launch is planned is launch_plan.h, which the CPU build runs as the product does
    defined = set(re.findall(r"^[\w\s\*]*?\b(terra_\w+)\s*\(", stubs, re.M))
    assert defined and defined <= declared, f"stand-ins that kernels.h does not declare as launchers: {sorted(defined - declared)}"
    so = tmp_path / "libhost.so"
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{csrc}", "-w", "-shared", "-o", str(so),
                        str(csrc / "scene_host.cpp"), str(csrc / "tree_build.cpp"), str(csrc / "multi_gpu.cpp"), str(H.ROOT / "tools" / "sanitize" / "stub_launchers.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    undefined = subprocess.run(["nm", "-D", "--undefined-only", str(so)], capture_output=True, text=True).stdout
    assert not [ln for ln in undefined.splitlines() if " terra_" in ln or "_Z" in ln and "terra_" in ln], undefined
