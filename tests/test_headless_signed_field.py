"""terra_headless --distance-field NXxNYxNZ field.pfm --signed: the switch parses and is refused without --distance-field (no GPU) and against a library without
terra_amd_count_hits (the reference), and on the GPU the field it writes is runtime.distance_field(signed="crossings") of the same cells, bit for bit."""
import subprocess

import numpy as np
import pytest

from terra_amd import runtime, scenes

CUBE = "".join(f"v {x} {y} {z}\n" for x in (0, 1) for y in (0, 1) for z in (2, 3)) + "f 1 2 4 3\nf 5 7 8 6\nf 1 5 6 2\nf 3 4 8 7\nf 1 3 7 5\nf 2 6 8 4\n"


def test_the_switch_parses_and_needs_a_field(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "amd")
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--signed" in r.stdout and "terra_amd_count_hits" in r.stdout
    r = subprocess.run([str(exe), "none.obj", str(tmp_path / "o.pfm"), "--signed"], capture_output=True, text=True)
    assert r.returncode == 64 and "--signed goes with --distance-field" in r.stderr, r.stderr
    # with a field the flag goes on to the next step: the mesh, which is not there
    r = subprocess.run([str(exe), str(tmp_path / "none.obj"), str(tmp_path / "o.pfm"), "--distance-field", "6x5x4", str(tmp_path / "f.pfm"), "--signed"], capture_output=True, text=True)
    assert r.returncode == 66, r.stderr


def test_the_switch_against_a_library_without_the_counts_is_refused(H, ref_lib, tmp_path):
    from test_headless_tool import build_tool
    exe = build_tool(H, tmp_path, "ref")
    obj = tmp_path / "q.obj"
    obj.write_text(CUBE)
    r = subprocess.run([str(exe), str(obj), str(tmp_path / "o.pfm"), "--width", "16", "--height", "12", "--spp", "1", "--integrator", "normals", "--tonemap", "none",
                        "--distance-field", "2x2x2", str(tmp_path / "field.pfm"), "--signed"], capture_output=True, text=True)
    assert r.returncode == 64 and "--signed needs a libterra_amd.so with terra_amd_count_hits" in r.stderr, r.stderr
    assert not (tmp_path / "field.pfm").exists() and not (tmp_path / "o.pfm").exists()


@pytest.mark.gpu
def test_the_signed_field_against_the_runtime(H, amd_lib, tmp_path):
    import torch
    from test_headless_tool import build_tool, read_pfm, write_obj
    L = runtime.load()
    assert L.device_count() > 0, "gpu tests need a visible MI355X: " + runtime.last_error()
    d = scenes.cornell_spheres(8, 8, 1)
    d.objects = d.objects[4:]                                            # the two spheres: closed surfaces
    obj = tmp_path / "spheres.obj"
    write_obj(d, obj)
    exe = build_tool(H, tmp_path, "amd")
    out, field = tmp_path / "image.pfm", tmp_path / "field.pfm"
    r = subprocess.run([str(exe), str(obj), str(out), "--distance-field", "7x6x5", str(field), "--signed", "--width", "8", "--height", "8", "--spp", "1", "--no-flip-z", "--normals", "file",
                        "--integrator", "normals", "--tonemap", "none"],          # (the spheres emit nothing: an integrator that needs no light)
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "7x6x5 cells" in r.stdout and "signed by crossings" in r.stdout and out.exists()
    L.clear_error()
    s = scenes.build_scene(L, d)
    try:
        v = runtime.scene_vertex_points(L, s)["position"]
        lo, hi = v.min(0), v.max(0)
        spacing = ((hi - lo) / np.array([7, 6, 5], np.float32)).astype(np.float32)
        want = runtime.distance_field(L, s, lo, spacing, (7, 6, 5), signed="crossings").cpu().numpy()
        plain = runtime.distance_field(L, s, lo, spacing, (7, 6, 5)).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        L.scene_destroy(s)
    got = read_pfm(field)
    assert got.shape == (5 * 6, 7, 3) and want.shape == (5, 6, 7) and (want < 0).any() and (want > 0).any() and np.array_equal(np.abs(want), plain)
    assert f"{int((want < 0).sum())} of 210 cells inside" in r.stdout
    for c in range(3):
        assert got[..., c].tobytes() == want.reshape(30, 7).tobytes(), c          # slices stacked vertically: slice iz in rows iz * NY ..
