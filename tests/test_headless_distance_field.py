"""terra_headless --distance-field NXxNYxNZ field.pfm: the switch parses and refuses bad sizes (no GPU), is reported and ignored against the reference, and on the
GPU the field it writes is runtime.distance_field of the same cells, bit for bit."""
import subprocess

import numpy as np
import pytest

from terra_amd import runtime, scenes

CUBE = "".join(f"v {x} {y} {z}\n" for x in (0, 1) for y in (0, 1) for z in (2, 3)) + "f 1 2 4 3\nf 5 7 8 6\nf 1 5 6 2\nf 3 4 8 7\nf 1 3 7 5\nf 2 6 8 4\n"


def test_the_switch_parses_and_refuses_bad_sizes(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--distance-field NXxNYxNZ PATH" in r.stdout
    field = str(tmp_path / "f.pfm")
    for bad in (["--distance-field", "2x2", field], ["--distance-field", "0x1x1", field], ["--distance-field", "2x-1x2", field], ["--distance-field", "4096x4096x2", field],
                ["--distance-field", "abc", field], ["--distance-field", "2x2x2"], ["--distance-field", "2x2x2", "--spp"], ["--distance-field"]):
        r = subprocess.run([str(exe), "none.obj", str(tmp_path / "o.pfm")] + bad, capture_output=True, text=True)
        assert r.returncode == 64 and "--distance-field" in r.stderr, (bad, r.stderr)
    # a good size goes on to the next step: the mesh, which is not there
    r = subprocess.run([str(exe), str(tmp_path / "none.obj"), str(tmp_path / "o.pfm"), "--distance-field", "6x5x4", field], capture_output=True, text=True)
    assert r.returncode == 66, r.stderr


def test_the_switch_against_the_reference_is_reported_and_ignored(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm
    exe = build_tool(H, tmp_path, "ref")
    obj = tmp_path / "q.obj"
    obj.write_text(CUBE)
    args = ["--width", "16", "--height", "12", "--spp", "1", "--integrator", "normals", "--tonemap", "none"]
    for out, extra in (("plain.pfm", []), ("with.pfm", ["--distance-field", "2x2x2", str(tmp_path / "field.pfm")])):
        r = subprocess.run([str(exe), str(obj), str(tmp_path / out)] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert ("--distance-field needs libterra_amd.so" in r.stderr) == bool(extra)
    assert np.array_equal(read_pfm(tmp_path / "with.pfm"), read_pfm(tmp_path / "plain.pfm")) and not (tmp_path / "field.pfm").exists()


@pytest.mark.gpu
def test_the_field_against_the_runtime(H, amd_lib, tmp_path):
    import torch
    from test_headless_tool import build_tool, read_pfm, write_obj
    L = runtime.load()
    assert L.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    d = scenes.cornell_box(8, 8, 1)
    obj = tmp_path / "cornell.obj"
    write_obj(d, obj)
    exe = build_tool(H, tmp_path, "amd")
    out, field = tmp_path / "image.pfm", tmp_path / "field.pfm"
    r = subprocess.run([str(exe), str(obj), str(out), "--distance-field", "6x5x4", str(field), "--width", "8", "--height", "8", "--spp", "1", "--no-flip-z", "--normals", "file"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "6x5x4 cells" in r.stdout and out.exists()
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        v = runtime.scene_vertex_points(L, s)["position"]
        lo, hi = v.min(0), v.max(0)
        spacing = ((hi - lo) / np.array([6, 5, 4], np.float32)).astype(np.float32)
        want = runtime.distance_field(L, s, lo, spacing, (6, 5, 4)).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    got = read_pfm(field)
    assert got.shape == (4 * 5, 6, 3) and want.shape == (4, 5, 6) and (want > 0).all() and (want < 2).all()
    for c in range(3):
        assert got[..., c].tobytes() == want.reshape(20, 6).tobytes(), c          # slices stacked vertically: slice iz in rows iz * NY ..
