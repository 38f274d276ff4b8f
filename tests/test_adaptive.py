"""Adaptive tiles (terra_amd_render_adaptive_device; include/terra_amd.h "Adaptive tiles") on Cornell 256 x 256, Direct, batches of 2 spp, tiles of 64: the
driver's rounds restated from its own outputs, against a uniform run, and against the same terra_amd_render_device tile calls issued by hand."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import api, scenes

pytestmark = pytest.mark.gpu
W = H_ = 256
TILE, SPP, MIN_B, MAX_B, TARGET = 64, 2, 3, 12, 0.06


@pytest.fixture(scope="module")
def L(amd_lib):
    import torch
    from terra_amd import runtime
    assert torch.cuda.is_available()
    return runtime.load()


@pytest.fixture(scope="module")
def cornell(L):
    d = scenes.cornell_box(W, H_, SPP, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d)
    yield s, scenes.camera_of(d)
    L.scene_destroy(s)


def buffers():
    from terra_amd import runtime
    return runtime.DeviceFramebuffer(W, H_), runtime.DeviceMoments(W, H_), runtime.DeviceAov(W, H_)


def tile_view(a, t, tx=W // TILE):
    y0, x0 = (t // tx) * TILE, (t % tx) * TILE
    return a[y0:y0 + TILE, x0:x0 + TILE]


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_rounds_counts_and_the_hand_issued_sequence(L, cornell):
    import torch
    from terra_amd import runtime
    s, cam = cornell
    fb, dm, aov = buffers()
    rep = runtime.render_adaptive_device(L, cam, s, fb, dm, aov, tile=TILE, min_batches=MIN_B, max_batches=MAX_B, target_error=TARGET)
    print("adaptive report:", rep)
    res, m, a = fb.results_host(), dm.host(), aov.host()
    tiles = (W // TILE) * (H_ // TILE)
    assert rep["tiles"] == tiles
    # every sampled pixel: samples == batches * spp == the AOV's samples; whole tiles share one batch count
    assert np.array_equal(res["samples"], m["batches"] * SPP) and np.array_equal(res["samples"], a["samples"]) and np.array_equal(m["weight"], res["samples"])
    per_tile = []
    for t in range(tiles):
        b = np.unique(tile_view(m["batches"], t))
        assert len(b) == 1, t
        per_tile.append(int(b[0]))
    assert min(per_tile) >= MIN_B and max(per_tile) <= MAX_B
    assert rep["tile_calls"] == sum(per_tile) and rep["samples"] == int(res["samples"].sum()) and rep["rounds"] == max(per_tile)
    err = runtime.tile_error_device(L, fb, dm, tile=TILE).cpu().numpy()
    assert rep["tiles_converged"] == int((err <= TARGET).sum())
    assert rep["max_error"] == np.float32(err[np.isfinite(err)].max())
    assert rep["hit_max_batches"] == int((err > TARGET).any())
    assert err.max() <= TARGET or rep["hit_max_batches"] == 1
    print("batches per tile:", per_tile)
    # the same calls by hand: a tile is rendered in round r while r < MIN_B or its error after round r - 1 exceeds the target -- no batch after a round in which it
    # was at or below the target -- and the framebuffer, the moments and the AOV buffer come out bit for bit
    fb2, dm2, aov2 = buffers()
    e = np.full(tiles, np.inf, np.float32)
    calls = 0
    for r in range(MAX_B):
        active = [t for t in range(tiles) if r < MIN_B or e[t] > TARGET]
        if not active:
            break
        for t in active:
            rect = ((t % (W // TILE)) * TILE, (t // (W // TILE)) * TILE, TILE, TILE)
            runtime.render_device(L, cam, s, fb2, rect=rect)
            runtime.render_aov_device(L, cam, s, aov2, rect=rect)
            calls += 1
        runtime.accumulate_moments_device(L, s, fb2, dm2)
        e = runtime.tile_error_device(L, fb2, dm2, tile=TILE).cpu().numpy()
    torch.cuda.synchronize()
    assert calls == rep["tile_calls"]
    assert np.array_equal(bits(fb.results), bits(fb2.results)) and np.array_equal(bits(fb.pixels), bits(fb2.pixels))
    assert np.array_equal(bits(dm.data), bits(dm2.data)) and np.array_equal(bits(aov.data), bits(aov2.data))
    # a second run, without the AOV buffer: the same framebuffer and the same report
    fb3, dm3, _ = buffers()
    rep3 = runtime.render_adaptive_device(L, cam, s, fb3, dm3, None, tile=TILE, min_batches=MIN_B, max_batches=MAX_B, target_error=TARGET)
    assert rep3 == rep and np.array_equal(bits(fb.results), bits(fb3.results)) and np.array_equal(bits(dm.data), bits(dm3.data))


def test_against_a_uniform_run(L):
    """a camera moved back so that the frame's outer tiles see nothing: they stop at min_batches, the run takes fewer samples than max_batches everywhere, and
    what it leaves is at or below the target unless the report says max_batches ended it"""
    import torch
    from terra_amd import runtime
    d = scenes.cornell_box(W, H_, SPP, integrator=api.kTerraIntegratorDirect)
    s = scenes.build_scene(L, d)
    cam = scenes.camera_of(d)
    cam.position = api.TerraFloat3(cam.position.x - 8.0 * cam.direction.x, cam.position.y - 8.0 * cam.direction.y, cam.position.z - 8.0 * cam.direction.z)
    fb, dm, aov = buffers()
    rep = runtime.render_adaptive_device(L, cam, s, fb, dm, aov, tile=TILE, min_batches=MIN_B, max_batches=MAX_B, target_error=TARGET)
    print("adaptive report:", rep)
    m, a = dm.host(), aov.host()
    tiles = (W // TILE) * (H_ // TILE)
    empty = [t for t in range(tiles) if not tile_view(a["coverage"], t).any()]
    assert empty, "the camera still sees geometry in every tile"
    for t in empty:
        assert np.all(tile_view(m["batches"], t) == MIN_B), t
    uniform = W * H_ * SPP * MAX_B
    assert rep["samples"] < uniform
    err = runtime.tile_error_device(L, fb, dm, tile=TILE).cpu().numpy()
    print(f"samples {rep['samples']} against {uniform} uniform; largest tile error {err.max():.4f}")
    assert err.max() <= TARGET or rep["hit_max_batches"] == 1
    # the options are checked like any argument
    opt = api.TerraAmdAdaptiveOptions(TILE, 1, 4, 0.1, 0)
    args = (C.byref(cam), s, fb.pixels.data_ptr(), fb.results.data_ptr(), dm.data.data_ptr(), None, W, H_, 0, 0, W, H_)
    assert L.render_adaptive_device(*args, C.byref(opt), None, None) == -4
    opt = api.TerraAmdAdaptiveOptions(24, 2, 4, 0.1, 0)
    assert L.render_adaptive_device(*args, C.byref(opt), None, None) == -4
    L.clear_error(); L.fn("terra_amd_clear_first_error", None, [])()
    L.scene_destroy(s)
