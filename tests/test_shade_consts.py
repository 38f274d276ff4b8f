"""The LDS plan with the per-triangle shading constants (csrc/dev_types.h "shading constants"; csrc/launch_plan.h terra_lds_bytes), through
terra_amd_scene_lds_plan. No GPU needed.

A pair-form launch stages 48 bytes per triangle behind its pair section -- e0[3], e1[3], d00, d11, d01, div, the reciprocal of div, a flag word -- and nothing
else changes: the Cornell block is 29,456 + 32 x 48 = 30,992 bytes, inside the budget that keeps five blocks per CU resident. Launches without a pair form
stage no constants. The table is filled on the device (make_tracer), by surface_init's own operations: tests/test_shade_consts_gpu.py holds the frames."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import runtime, scenes
from test_oracle_vs_reference import soup_scene


@pytest.fixture(scope="module")
def L(amd_lib):
    return runtime.load(need_torch=False)


def plan(L, d):
    scene = scenes.build_scene(L, d)
    out = np.zeros(6, np.uint32)
    rc = L.fn("terra_amd_scene_lds_plan", C.c_int, [C.c_void_p, C.c_void_p])(scene, out.ctypes.data)
    assert rc == 0, runtime.last_error()
    return dict(zip(("bytes", "consts", "pairs", "budget", "tris", "ranked"), (int(v) for v in out)))


@pytest.mark.parametrize("mk", [lambda: scenes.cornell_box(16, 16, 1), lambda: scenes.cornell_phong(16, 16, 1)], ids=["cornell", "cornell-phong"])
def test_cornell_block_is_the_documented_sum(L, mk):
    p = plan(L, mk())
    assert p["tris"] == 32 and p["ranked"] == 1
    assert p["pairs"] == 6 * 16 * 64 + 16 * 48 == 6912          # six permuted copies of 16 entries, the 16-box table
    assert p["consts"] == 32 * 48 == 1536
    assert p["budget"] == 32358                                   # (158 KB of a CU's LDS over five blocks)
    if mk().objects[1].material.kind == "diffuse":
        assert p["bytes"] == 29456 + 1536 == 30992
    assert p["bytes"] <= p["budget"]
    assert p["consts"] + p["pairs"] <= 32 * 6 * 48               # never more than the ranked entries the plan budgeted


def test_no_pair_form_no_constants(L, H):
    p = plan(L, soup_scene(H, 32, 18, n_objects=3))
    assert p["tris"] == 32 and p["pairs"] == 0 and p["consts"] == 0
    q = plan(L, scenes.sponza_hall(16, 16, 1))
    assert q["tris"] == 0 and q["consts"] == 0
