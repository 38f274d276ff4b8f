"""Frames of launches that read surface_init's per-triangle constants from LDS (csrc/dev_types.h "shading constants"; make_tracer fills them, pair-form launches
only) against the oracle, which computes them per hit: 64 x 48 at 4 spp, bit for bit. The cases are those of tests/test_exact_div_render_gpu.py, which this file
reuses -- the Cornell integrators, the Phong variant, a shard, a rectangle at an odd origin, split 4 against four calls, the box scaled by 2^-20 and 2^20 (the flag of
every triangle's div flips to "plain division") -- and every one but the scaled-up box (outside the range of the pair form's box test: it must simply keep the oracle's bits) asserts that its launch took the pair
form, so that the section was really staged and read;
the quad of 2^-32 edges (a denormal div: flag 0) is a fan of two triangles, so it has the pair form too; the one-triangle overflowing light has none and
stays in that file."""
import numpy as np
import pytest

from terra_amd import api, runtime, scenes
from test_leaf_pairs_gpu import dev
from test_flat_loop_layout_gpu import oracle, equals_oracle
from test_exact_div_render_gpu import SHAPE, scaled, sliver_scene, nan_aware_equal

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(amd_lib):
    lib = runtime.load(need_torch=False)
    assert lib.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    return lib


def staged_n(got, n):
    assert got["used"] and got["n_pairs"] == n          # the pair form: the launch staged the constants and surface_init read them
    return got


def staged(got):
    return staged_n(got, 16)


@gpu
@pytest.mark.parametrize("integ", [api.kTerraIntegratorSimple, api.kTerraIntegratorDirect, api.kTerraIntegratorDirectMis], ids=["simple", "direct", "direct-mis"])
def test_cornell_integrators(G, H, orc_lib, integ):
    mk = lambda: scenes.cornell_box(integrator=integ, **SHAPE)
    got = staged(dev(G, mk(), 1))
    assert got["acc"].sum() > 0 and equals_oracle(got, oracle(H, mk()))


@gpu
def test_cornell_phong(G, H, orc_lib):
    mk = lambda: scenes.cornell_phong(**SHAPE)
    assert equals_oracle(staged(dev(G, mk(), 1)), oracle(H, mk()))


@gpu
@pytest.mark.parametrize("kw", [dict(shard=(16, 1, 2)), dict(rect=(7, 5, 24, 20))], ids=["shard-1-of-2", "rectangle-at-an-odd-origin"])
def test_part_of_the_frame(G, H, orc_lib, kw):
    mk = lambda: scenes.cornell_box(**SHAPE)
    got, want = staged(dev(G, mk(), 1, **kw)), oracle(H, mk())
    own = got["samples"] == 4
    assert own.any() and not own.all() and (got["samples"][~own] == 0).all()
    assert np.array_equal(got["acc"].view(np.uint32)[own], np.ascontiguousarray(want["acc"]).view(np.uint32)[own])


@gpu
def test_split_four_against_four_calls(G, H, orc_lib):
    one = staged(dev(G, scenes.cornell_box(64, 48, 4), 1, split=4))
    many = staged(dev(G, scenes.cornell_box(64, 48, 1), 1, passes=4))
    assert np.array_equal(one["acc"].view(np.uint32), many["acc"].view(np.uint32)) and np.array_equal(one["pixels"].view(np.uint32), many["pixels"].view(np.uint32))
    H.set_oracle_math(1)
    try:
        want = H.Unit("orc").render_pixels(scenes.cornell_box(64, 48, 1), passes=4, want_calls=False)
    finally:
        H.set_oracle_math(0)
    assert equals_oracle(one, want)


@gpu
@pytest.mark.parametrize("k", [2.0 ** -20, 2.0 ** 20], ids=["scaled-down", "scaled-up"])
def test_scaled_cornell(G, H, orc_lib, k):
    """every triangle's div is 2^-80 / 2^80 times its usual size: outside the guarded range, so every flag word says: plain division"""
    mk = lambda: scaled(scenes.cornell_box(**SHAPE), k)
    on, off, want = dev(G, mk(), 1), dev(G, mk(), 0), oracle(H, mk())
    if k < 1:
        staged(on)
    assert not off["used"] and equals_oracle(on, want) and equals_oracle(off, want)


@gpu
def test_denormal_div_is_flagged_for_the_plain_division(G, H, orc_lib):
    got, want = staged_n(dev(G, sliver_scene(), 1), 1), oracle(H, sliver_scene())
    assert (np.asarray(want["acc"])[..., 0] > 0).sum() >= 4          # paths hit the quad: its emission is the only light
    assert nan_aware_equal(got["acc"], want["acc"]) and nan_aware_equal(got["pixels"], want["pixels"])
