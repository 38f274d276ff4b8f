"""Temporal reprojection at the C boundary, without a GPU: the entry points are exported, TerraAmdHistory and TerraAmdTemporalOptions have the layout
include/terra_amd.h pins (in C, in C++ and in the ctypes / numpy mirrors), the runtime binds the calls, terra_headless offers --frames / --camera-to / --temporal,
and linked against the compiled reference it says so and writes the plain frames."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from terra_amd import api, scenes

NEW = ("terra_amd_reproject_device", "terra_amd_reproject")
HIST_OFFSETS = {"radiance": 0, "length": 12, "normal": 16, "depth": 28, "mu1": 32, "mu2": 36, "reserved": 40}
OPT_OFFSETS = {"alpha": 0, "depth_tolerance": 4, "normal_cos": 8, "reserved": 12}


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
    assert len(runtime._EXTRA["terra_amd_reproject_device"][1]) == 17 and len(runtime._EXTRA["terra_amd_reproject"][1]) == 14
    for name in ("DeviceHistory", "reproject_device"):
        assert hasattr(runtime, name), name


@pytest.mark.parametrize("compiler, std, ext", [("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")])
def test_layouts_in_c_cxx_and_ctypes(H, tmp_path, compiler, std, ext):
    assert C.sizeof(api.TerraAmdHistory) == 48 and api.HISTORY_DTYPE.itemsize == 48 and C.sizeof(api.TerraAmdTemporalOptions) == 16
    for f, off in HIST_OFFSETS.items():
        assert getattr(api.TerraAmdHistory, f).offset == off, f
        assert api.HISTORY_DTYPE.fields[f][1] == off, f
    for f, off in OPT_OFFSETS.items():
        assert getattr(api.TerraAmdTemporalOptions, f).offset == off, f
    items = ["sizeof ( TerraAmdHistory )"] + [f"offsetof ( TerraAmdHistory, {f} )" for f in HIST_OFFSETS]
    items += ["sizeof ( TerraAmdTemporalOptions )"] + [f"offsetof ( TerraAmdTemporalOptions, {f} )" for f in OPT_OFFSETS]
    src = tmp_path / f"layout.{ext}"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { ' + " ".join(f'printf ( "%zu\\n", ( size_t ) {i} );' for i in items) + " return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run([compiler, std, "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = [48] + list(HIST_OFFSETS.values()) + [16] + list(OPT_OFFSETS.values())
    assert [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()] == want


def test_headless_help_lists_the_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    out = subprocess.run([str(exe), "--help"], capture_output=True, text=True).stdout
    for flag in ("--frames N", "--camera-to px py pz dx dy dz", "--temporal ALPHA"):
        assert flag in out, flag


def test_headless_against_the_reference_says_so_and_writes_the_plain_frames(H, ref_lib, tmp_path):
    """three frames along a camera move: each equals the plain single-frame run at that frame's camera (the first, middle and last of the interpolation)"""
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "ref")
    d = scenes.cornell_box(40, 30, 2)
    obj = tmp_path / "c.obj"
    write_obj(d, obj)
    args = ["--width", "40", "--height", "30", "--spp", "2", "--integrator", "normals", "--tonemap", "none"]
    cams = [["0", "1", "-3.5", "0", "0", "1"], ["0.125", "1", "-3.25", "0", "0", "1"], ["0.25", "1", "-3", "0", "0", "1"]]
    r = subprocess.run([str(exe), str(obj), str(tmp_path / "out.pfm")] + args + ["--camera"] + cams[0] + ["--camera-to"] + cams[2] + ["--frames", "3", "--temporal", "0.25", "--denoise", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--temporal needs libterra_amd.so; ignored, the plain frames are written" in r.stderr
    assert not (tmp_path / "out.pfm").exists()
    for f, cam in enumerate(cams):
        plain = subprocess.run([str(exe), str(obj), str(tmp_path / f"plain{f}.pfm")] + args + ["--camera"] + cam, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
        assert np.array_equal(read_pfm(tmp_path / f"out.{f:04d}.pfm"), read_pfm(tmp_path / f"plain{f}.pfm")), f
    assert not np.array_equal(read_pfm(tmp_path / "out.0000.pfm"), read_pfm(tmp_path / "out.0002.pfm"))
    # --frames and --camera-to alone need nothing of libterra_amd.so: no word about it
    r = subprocess.run([str(exe), str(obj), str(tmp_path / "two.pfm")] + args + ["--camera"] + cams[0] + ["--camera-to"] + cams[2] + ["--frames", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and "libterra_amd.so" not in r.stderr, r.stderr
    assert np.array_equal(read_pfm(tmp_path / "two.0001.pfm"), read_pfm(tmp_path / "plain2.pfm"))
