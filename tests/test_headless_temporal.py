"""terra_headless --frames / --camera-to / --temporal on the GPU, against libterra_amd.so: every frame renders under its own frame seed, --seed + f * 2^32 (the
device keys a pixel's stream with seed + pixel index: seeds closer than the frame has pixels give one noise field moved along the rows), so a still camera
accumulates independent frames; the flags the frames path does not act on are reported."""
import subprocess

import numpy as np
import pytest

from terra_amd import scenes

pytestmark = pytest.mark.gpu
W, HGT, SEED = 48, 32, 100


@pytest.fixture(scope="module")
def tool(H, amd_lib, tmp_path_factory):
    """run(out, extra) -> the finished process; the scene tests/test_headless_variance.py sends through the tool, smaller, at 1 spp"""
    from test_headless_tool import build_tool, write_obj
    tmp = tmp_path_factory.mktemp("headless_temporal")
    exe = build_tool(H, tmp, "amd")
    obj = tmp / "c.obj"
    write_obj(scenes.cornell_phong(W, HGT, 1), obj, mirror_z=True)
    args = ["--width", str(W), "--height", str(HGT), "--integrator", "direct", "--tonemap", "none", "--normals", "file"]

    def run(out, extra, spp=1):
        r = subprocess.run([str(exe), str(obj), str(tmp / out)] + args + ["--spp", str(spp)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r
    return tmp, run


def test_frames_render_under_their_own_seeds_and_report_dropped_flags(tool):
    """without a blend frame f is the plain run under --seed + f * 2^32, bit for bit; --temporal without a filter to write through, --aov and --variance are reported.
    Frame 1 is not frame 0's noise moved by a pixel (what seed + 1 gives: seed + 1 at pixel p is seed at pixel p + 1). At 1 spp without jitter the difference
    of two independent frames is noise whether one of them is moved by a pixel or not, so the two mean absolute differences are of one size (the move adds
    the image's own gradient, which only raises it); of a moved copy the difference is that gradient alone. The bound, half the unmoved difference, lies
    between: the image's gradient is far below its 1 spp noise on the walls that fill this frame."""
    from test_headless_tool import read_pfm
    tmp, run = tool
    r = run("f.pfm", ["--seed", str(SEED), "--frames", "2", "--temporal", "0.25", "--aov", str(tmp / "a"), "--variance", str(tmp / "v.pfm")])
    assert "--temporal writes the blended frame through --denoise K or --denoise-variance K" in r.stderr and "the plain frames are written" in r.stderr
    assert "--aov / --variance are not written with --frames; ignored" in r.stderr
    assert "libterra_amd.so" not in r.stderr
    assert not (tmp / "f.pfm").exists() and not (tmp / "a.albedo.pfm").exists() and not (tmp / "v.pfm").exists()
    for f in range(2):
        run(f"p{f}.pfm", ["--seed", str(SEED + (f << 32))])
        assert np.array_equal(read_pfm(tmp / f"f.{f:04d}.pfm"), read_pfm(tmp / f"p{f}.pfm")), f
    f0, f1 = read_pfm(tmp / "f.0000.pfm").astype(np.float64), read_pfm(tmp / "f.0001.pfm").astype(np.float64)
    assert not np.array_equal(f0, f1)
    plain = np.abs(f1[:, 1:-1] - f0[:, 1:-1]).mean()
    moved = [np.abs(f1[:, 1:-1] - f0[:, 2:]).mean(), np.abs(f1[:, 1:-1] - f0[:, :-2]).mean()]
    print(f"mean |frame 1 - frame 0|: {plain:.4g}; frame 0 moved a pixel to the left, to the right: {moved[0]:.4g}, {moved[1]:.4g}")
    assert plain > 0 and min(moved) > 0.5 * plain, (plain, moved)
    r = run("g.pfm", ["--frames", "1", "--denoise", "1"])
    assert "--denoise / --denoise-variance with --frames go with --temporal; ignored" in r.stderr


def test_a_still_camera_accumulates_independent_frames(tool):
    """--frames 4 --temporal 0.25 under one camera: alpha_p = 1, 1/2, 1/3, 1/4, the running mean of four frames. The frames differ (under one seed they would be
    equal bit for bit: u_h + alpha (u_c - u_h) = u_h where u_c = u_h), and the fourth lies closer to a 256 spp render through the same filter than the first: the
    mean of four independent frames has a quarter of one frame's variance, and the filter's own bias is on both sides. The history's variance reaches
    --denoise-variance from the second frame on: its first frame (every length 1: unknown) is --denoise's bit for bit, its fourth is not."""
    from test_headless_tool import read_pfm
    tmp, run = tool
    still = ["--seed", str(SEED), "--frames", "4", "--temporal", "0.25"]
    run("t.pfm", still + ["--denoise", "1"])
    run("ref.pfm", ["--seed", str(SEED + 1000), "--denoise", "1"], spp=256)
    ref = read_pfm(tmp / "ref.pfm").astype(np.float64)
    out = [read_pfm(tmp / f"t.{f:04d}.pfm") for f in range(4)]
    assert all(np.isfinite(o).all() for o in out)
    for f in range(3):
        assert not np.array_equal(out[f], out[f + 1]), f
    rmse = [float(np.sqrt(np.mean((o - ref) ** 2))) for o in out]
    print(f"rmse against 256 spp, frames 0 .. 3: {rmse}")
    assert rmse[3] < rmse[0], rmse
    run("v.pfm", still + ["--denoise-variance", "1"])
    assert np.array_equal(read_pfm(tmp / "v.0000.pfm"), out[0])
    assert not np.array_equal(read_pfm(tmp / "v.0003.pfm"), out[3])
