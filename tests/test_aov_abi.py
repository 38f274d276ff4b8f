"""The AOV pass and the denoiser at the C boundary, without a GPU: the entry points are exported, TerraAmdAovResult has the layout
include/terra_amd.h pins (in C and in the ctypes mirror), and terra_headless offers --aov / --denoise -- linked against the compiled reference it
warns and writes the plain image."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from terra_amd import api, scenes

OFFSETS = {"albedo": 0, "coverage": 12, "normal": 16, "depth": 28, "samples": 32, "reserved": 36}


def test_new_symbols_are_exported(amd_lib):
    for name in ("terra_amd_render_aov_device", "terra_amd_render_aov", "terra_amd_denoise_device", "terra_amd_denoise"):
        assert amd_lib.has(name), name


def test_aov_result_layout_in_c_and_ctypes(H, tmp_path):
    from terra_amd import runtime
    assert C.sizeof(runtime.AovResult) == 48 and runtime.AOV_DTYPE.itemsize == 48
    for f, off in OFFSETS.items():
        assert getattr(runtime.AovResult, f).offset == off, f
        assert runtime.AOV_DTYPE.fields[f][1] == off, f
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { printf ( "%zu %zu %zu %zu %zu %zu %zu\\n", sizeof ( TerraAmdAovResult ), '
                   + ", ".join(f"offsetof ( TerraAmdAovResult, {f} )" for f in OFFSETS) + " ); return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["48"] + [str(v) for v in OFFSETS.values()]


def test_headless_help_lists_the_flags(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    out = subprocess.run([str(exe), "--help"], capture_output=True, text=True).stdout
    assert "--aov PREFIX" in out and "--denoise K" in out


def test_headless_against_the_reference_warns_and_writes_the_plain_image(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "ref")
    d = scenes.cornell_box(40, 30, 2)
    obj = tmp_path / "c.obj"
    write_obj(d, obj)
    args = ["--width", "40", "--height", "30", "--spp", "2", "--integrator", "normals", "--tonemap", "none"]
    plain = subprocess.run([str(exe), str(obj), str(tmp_path / "plain.pfm")] + args, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run([str(exe), str(obj), str(tmp_path / "dn.pfm")] + args + ["--denoise", "3", "--aov", str(tmp_path / "a")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--denoise need libterra_amd.so" in r.stderr
    assert np.array_equal(read_pfm(tmp_path / "dn.pfm"), read_pfm(tmp_path / "plain.pfm"))
    assert not (tmp_path / "a.albedo.pfm").exists()
