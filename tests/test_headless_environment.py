"""apps/terra_headless.c's environment options: --environment FILE (Radiance .hdr, flat or run-length encoded, -Y H +X W; .pfm in either byte order),
--environment-color, --env-light and --env-sampling off|table|mis. On the CPU the tool is linked against the compiled reference (which drops the environment
term) and the map loader is checked against numpy decoders; on the GPU, against libterra_amd.so, its render with a map equals the oracle's bit for bit."""
import subprocess

import numpy as np
import pytest

from terra_amd import api, scenes
from test_headless_tool import build_tool, read_pfm, write_obj

# a unit cube in front of the default camera (quads: the reference's tree builder wants more than one triangle)
TINY_OBJ = "".join(f"v {x} {y} {z}\n" for x in (0, 1) for y in (0, 1) for z in (2, 3)) + "f 1 2 4 3\nf 5 7 8 6\nf 1 5 6 2\nf 3 4 8 7\nf 1 3 7 5\nf 2 6 8 4\n"


def write_pfm(path, img, little=True):
    """img (h, w, 3) with row 0 = top; the file holds the bottom row first"""
    h, w, _ = img.shape
    dt = "<f4" if little else ">f4"
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n%s\n" % (w, h, b"-1.0" if little else b"1.0"))
        f.write(np.ascontiguousarray(img[::-1], dtype=dt).tobytes())


def rgbe(img):
    """float (h, w, 3) -> RGBE bytes (h, w, 4)"""
    mx = img.max(axis=2)
    e = np.zeros(mx.shape, np.int32); m = np.zeros(img.shape, np.uint8)
    nz = mx > 1e-32
    fr, ex = np.frexp(mx[nz])
    e[nz] = ex + 128
    m[nz] = np.clip(img[nz] * (256.0 / np.ldexp(1.0, ex))[:, None], 0, 255).astype(np.uint8)
    return np.concatenate([m, e[..., None].astype(np.uint8)], axis=2)


def decode_rgbe(b):
    """the numpy decoder: m 2^(e - 136), e = 0 -> 0"""
    e = b[..., 3].astype(np.int32)
    v = np.ldexp(b[..., :3].astype(np.float64), (e - 136)[..., None])
    v[e == 0] = 0
    return v.astype(np.float32)


def write_hdr(path, b, rle=False, orientation=None):
    h, w, _ = b.shape
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\n# written by the test\nFORMAT=32-bit_rle_rgbe\n\n")
        f.write((orientation or "-Y %d +X %d" % (h, w)).encode() + b"\n")
        for y in range(h):
            if not rle:
                f.write(b[y].tobytes())
                continue
            f.write(bytes([2, 2, w >> 8, w & 255]))
            for ch in range(4):
                row = b[y, :, ch]; x = 0
                while x < w:
                    run = 1
                    while x + run < w and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 3:
                        f.write(bytes([128 + run, int(row[x])])); x += run
                    else:
                        n = 1
                        while x + n < w and n < 128 and not (x + n + 2 < w and row[x + n] == row[x + n + 1] == row[x + n + 2]):
                            n += 1
                        f.write(bytes([n]) + row[x:x + n].tobytes()); x += n


def env_line(stderr):
    lines = [ln for ln in stderr.splitlines() if ln.startswith("environment: ")]
    assert len(lines) == 1, stderr
    w = lines[0].split()
    return int(w[1]), int(w[3].rstrip(",")), np.array([float(w[5]), float(w[6]), float(w[7])])


def test_maps_load_and_report(H, ref_lib, tmp_path):
    exe = build_tool(H, tmp_path, "ref")
    (tmp_path / "t.obj").write_text(TINY_OBJ)
    rs = np.random.RandomState(4)
    img = (rs.uniform(0, 1, size=(9, 37, 3)) ** 3 * 20).astype(np.float32)
    img[2, 5:30] = (3.0, 3.0, 3.0)                          # long runs for the RLE writer
    img[4] = 0                                             # a black row (e = 0)
    b = rgbe(img)
    cases = {"flat.hdr": (lambda p: write_hdr(p, b), decode_rgbe(b)),
             "rle.hdr": (lambda p: write_hdr(p, b, rle=True), decode_rgbe(b)),
             "le.pfm": (lambda p: write_pfm(p, img, True), img),
             "be.pfm": (lambda p: write_pfm(p, img, False), img)}
    for name, (write, want) in cases.items():
        write(tmp_path / name)
        r = subprocess.run([str(exe), str(tmp_path / "t.obj"), str(tmp_path / "o.pfm"), "--environment", str(tmp_path / name), "--no-render"], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        w, h, mean = env_line(r.stderr)
        assert (w, h) == (37, 9), name
        assert np.allclose(mean, want.astype(np.float64).reshape(-1, 3).mean(axis=0), rtol=1e-5, atol=1e-9), (name, mean)
    assert (tmp_path / "rle.hdr").stat().st_size < (tmp_path / "flat.hdr").stat().st_size      # (the RLE file really is run-length encoded)
    # the switches need libterra_amd.so: against the reference they print a notice and the render goes on
    r = subprocess.run([str(exe), str(tmp_path / "t.obj"), str(tmp_path / "o.pfm"), "--environment", str(tmp_path / "le.pfm"), "--env-light", "--env-sampling", "mis",
                        "--width", "8", "--height", "8", "--spp", "1", "--integrator", "simple"], capture_output=True, text=True)
    assert r.returncode == 0 and "need libterra_amd.so" in r.stderr, r.stderr
    r = subprocess.run([str(exe), str(tmp_path / "t.obj"), str(tmp_path / "o.pfm"), "--environment-color", "1", "2", "3", "--width", "8", "--height", "8", "--spp", "1",
                        "--integrator", "simple"], capture_output=True, text=True)
    assert r.returncode == 0 and "environment:" not in r.stderr, r.stderr


def test_bad_maps_exit_65_and_help(H, ref_lib, tmp_path):
    exe = build_tool(H, tmp_path, "ref")
    (tmp_path / "t.obj").write_text(TINY_OBJ)
    b = rgbe(np.ones((4, 10, 3), np.float32))
    write_hdr(tmp_path / "flip.hdr", b, orientation="+Y 4 +X 10")
    write_hdr(tmp_path / "short.hdr", b, rle=True)
    data = (tmp_path / "short.hdr").read_bytes(); (tmp_path / "short.hdr").write_bytes(data[:-7])
    write_hdr(tmp_path / "short_flat.hdr", b)
    data = (tmp_path / "short_flat.hdr").read_bytes(); (tmp_path / "short_flat.hdr").write_bytes(data[:-3])
    (tmp_path / "wide.pfm").write_bytes(b"PF\n65536 1\n-1.0\n" + b"\0" * 64)
    (tmp_path / "short.pfm").write_bytes(b"PF\n4 4\n-1.0\n" + b"\0" * 100)
    (tmp_path / "grey.pfm").write_bytes(b"Pf\n1 1\n-1.0\n" + b"\0" * 4)
    (tmp_path / "junk.hdr").write_bytes(b"hello\n")
    for name in ("flip.hdr", "short.hdr", "short_flat.hdr", "wide.pfm", "short.pfm", "grey.pfm", "junk.hdr", "missing.hdr"):
        r = subprocess.run([str(exe), str(tmp_path / "t.obj"), str(tmp_path / "o.pfm"), "--environment", str(tmp_path / name), "--no-render"], capture_output=True, text=True)
        assert r.returncode == 65 and name in r.stderr, (name, r.returncode, r.stderr)
    # a header inside the size limit that asks for more memory than the process may have (65535 x 65535 x 3 floats = 51 GB): refused, not crashed on
    import resource
    (tmp_path / "huge.pfm").write_bytes(b"PF\n65535 65535\n-1.0\n" + b"\0" * 64)
    r = subprocess.run([str(exe), str(tmp_path / "t.obj"), str(tmp_path / "o.pfm"), "--environment", str(tmp_path / "huge.pfm"), "--no-render"], capture_output=True, text=True,
                       preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_AS, (2 << 30, 2 << 30)))
    assert r.returncode == 65 and "out of memory" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--environment FILE", "--environment-color", "--env-light", "--env-sampling off|table|mis"):
        assert opt in r.stdout, opt


@pytest.mark.gpu
def test_tool_with_a_map_equals_the_oracle(H, amd_lib, orc_lib, devmath_mode, tmp_path):
    """the tool (linked against libterra_amd.so) with --environment sky.pfm --env-light --env-sampling table --integrator mis == the oracle's render of the same
    scene and map with section 12's sampling, bit for bit; with --env-sampling mis the image differs, is finite and is deterministic"""
    from test_environment_sampling import courtyard, sky
    exe = build_tool(H, tmp_path, "amd")
    tex = sky()
    d = courtyard(96, 64, 4, api.kTerraIntegratorDirectMis, True, tex=tex, tonemap=api.kTerraTonemappingOperatorReinhard)
    want = H.Unit("orc").render_pixels(d, want_calls=False, threads=8)["pixels"]
    obj = tmp_path / "courtyard.obj"
    write_obj(d, obj, mirror_z=True)
    write_pfm(tmp_path / "sky.pfm", tex.data, little=False)
    args = [str(exe), str(obj), str(tmp_path / "out.pfm"), "--width", "96", "--height", "64", "--spp", "4", "--bounces", str(d.bounces), "--integrator", "mis",
            "--tonemap", "reinhard", "--jitter", str(d.jitter), "--normals", "file", "--camera", *[str(v) for v in d.camera_position + d.camera_direction],
            "--environment", str(tmp_path / "sky.pfm"), "--env-light"]
    r = subprocess.run(args + ["--env-sampling", "table"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert env_line(r.stderr)[:2] == (32, 16)
    table = read_pfm(tmp_path / "out.pfm").copy()
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    outs = []
    for _ in range(2):
        r = subprocess.run(args + ["--env-sampling", "mis"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        outs.append(read_pfm(tmp_path / "out.pfm").copy())
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert not np.array_equal(outs[0].view(np.uint32), table.view(np.uint32))
