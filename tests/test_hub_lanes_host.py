"""The lane-split hub pose of k_clear (csrc/lvx_resid.h: hub_lanes_*) against pose_eval + hub_matrix in a stand-alone host program (tests/native/hub_lanes_host_check.cpp):
the phases run as loops over lanes; every output must have the value the one-lane evaluation gives."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hub_lanes_host_check(tmp_path):
    exe = str(tmp_path / "hub_lanes_host_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", os.path.join(ROOT, "tests", "native", "hub_lanes_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hub_lanes_host_check: OK" in out.stdout
    m = re.search(r"(\d+) cases, (\d+) values compared, (\d+) differ", out.stdout)
    assert m and int(m.group(1)) >= 400 and int(m.group(2)) > 100000 and int(m.group(3)) == 0
