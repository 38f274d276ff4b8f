"""Ray queries at the C boundary, without a GPU: the four entry points are exported, and TerraAmdRay / TerraAmdHit have the layout include/terra_amd.h pins --
in C (a gcc-compiled probe of the header) and in the ctypes and numpy mirrors of terra_amd/api.py."""
import ctypes as C
import subprocess

from terra_amd import api

RAY = {"origin": 0, "tmax": 12, "direction": 16, "reserved": 28}
HIT = {"t": 0, "object": 4, "triangle": 8, "reserved": 12, "point": 16, "reserved2": 28}
SYMBOLS = ("terra_amd_intersect_device", "terra_amd_occluded_device", "terra_amd_intersect", "terra_amd_occluded")


def test_new_symbols_are_exported(amd_lib):
    for name in SYMBOLS:
        assert amd_lib.has(name), name
    assert set(api.RAY_QUERY_SIGNATURES) == set(SYMBOLS)


def test_ray_and_hit_layout_in_c_and_ctypes(H, tmp_path):
    assert C.sizeof(api.TerraAmdRay) == 32 and C.sizeof(api.TerraAmdHit) == 32 and api.RAY_DTYPE.itemsize == 32 and api.HIT_DTYPE.itemsize == 32
    for struct, dtype, offsets in ((api.TerraAmdRay, api.RAY_DTYPE, RAY), (api.TerraAmdHit, api.HIT_DTYPE, HIT)):
        assert [n for n, _ in struct._fields_] == list(offsets) == list(dtype.names)
        for f, off in offsets.items():
            assert getattr(struct, f).offset == off, f
            assert dtype.fields[f][1] == off, f
    probe = ["sizeof ( TerraAmdRay )"] + [f"offsetof ( TerraAmdRay, {f} )" for f in RAY] + ["sizeof ( TerraAmdHit )"] + [f"offsetof ( TerraAmdHit, {f} )" for f in HIT]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "terra_amd.h"\nint main ( void ) { printf ( "' + " ".join(["%zu"] * len(probe)) + '\\n", '
                   + ", ".join(probe) + " ); return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", f"-I{H.ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ["32"] + [str(v) for v in RAY.values()] + ["32"] + [str(v) for v in HIT.values()]
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == want
