"""terra_headless --passes / --denoise-variance / --adaptive / --variance on the GPU, against libterra_amd.so."""
import subprocess

import numpy as np
import pytest

from terra_amd import scenes

pytestmark = pytest.mark.gpu


def test_passes_variance_and_adaptive(H, amd_lib, tmp_path):
    from test_headless_tool import build_tool, read_pfm, write_obj
    exe = build_tool(H, tmp_path, "amd")
    d = scenes.cornell_phong(96, 64, 2)          # (the scene tests/test_headless_tool.py sends through the tool with the direct integrator)
    obj = tmp_path / "c.obj"
    write_obj(d, obj, mirror_z=True)
    args = ["--width", "96", "--height", "64", "--spp", "2", "--integrator", "direct", "--tonemap", "none", "--normals", "file"]
    run = lambda out, extra: subprocess.run([str(exe), str(obj), str(tmp_path / out)] + args + extra, capture_output=True, text=True, timeout=600)
    plain = run("plain.pfm", [])
    assert plain.returncode == 0, plain.stderr
    # one pass with the new flags absent or --passes 1 is the plain image
    one = run("one.pfm", ["--passes", "1"])
    assert one.returncode == 0 and np.array_equal(read_pfm(tmp_path / "one.pfm"), read_pfm(tmp_path / "plain.pfm"))
    r = run("p4.pfm", ["--passes", "4", "--variance", str(tmp_path / "v.pfm")])
    assert r.returncode == 0, r.stderr
    v = read_pfm(tmp_path / "v.pfm")
    assert v.shape[:2] == (64, 96) and np.isfinite(v).all() and (v >= 0).all() and (v > 0).mean() > 0.2
    k0 = run("k0.pfm", ["--passes", "4", "--denoise-variance", "0"])
    assert k0.returncode == 0 and np.array_equal(read_pfm(tmp_path / "k0.pfm"), read_pfm(tmp_path / "p4.pfm"))
    k3 = run("k3.pfm", ["--passes", "4", "--denoise-variance", "3"])
    assert k3.returncode == 0, k3.stderr
    a, b = read_pfm(tmp_path / "k3.pfm"), read_pfm(tmp_path / "p4.pfm")
    assert np.isfinite(a).all() and not np.array_equal(a, b) and abs(a.mean() / b.mean() - 1) < 0.05
    ad = run("ad.pfm", ["--adaptive", "0.1", "--min-passes", "2", "--max-passes", "6", "--tile", "32", "--variance", str(tmp_path / "va.pfm")])
    assert ad.returncode == 0, ad.stderr
    assert "adaptive:" in ad.stderr and "tile calls" in ad.stderr
    assert np.isfinite(read_pfm(tmp_path / "ad.pfm")).all() and (read_pfm(tmp_path / "va.pfm") >= 0).all()
    g = run("g.pfm", ["--gpus", "1", "--passes", "4"])
    assert g.returncode == 0 and "do not mirror --gpus" in g.stderr
