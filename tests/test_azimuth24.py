"""tdm_azimuth24 (csrc/dev_math.h), the samplers' azimuth of a stream-B variate in one arm, on the host: tests/azimuth24_check.cpp compares it with
tdm_sincosf_pair -- the function the azimuth table is filled by -- for all 2^24 arguments, both outputs as bit patterns, holds the quadrant's thresholds against
the reference reduction and the early result's range against the reference's test, and prints the first mismatch of each kind. Built with the host compiler and
the library's -ffp-contract=off; a second or two."""
import subprocess


def test_single_arm_form_equals_the_two_arm_form_on_every_variate(H, tmp_path):
    csrc = H.ROOT / "terra_amd" / "csrc"
    exe = tmp_path / "azimuth24_check"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", f"-I{csrc}", str(H.ROOT / "tests" / "azimuth24_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().splitlines()[-1] == "mismatches 0 quadrant 0 early 0", run.stdout
