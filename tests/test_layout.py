"""The batch layouts of the audio utilities (emotivoice_amd/csrc/ev_layout.h) on the CPU: tests/layout_check.cpp is compiled as a stand-alone program
with the host's address and undefined-behaviour sanitizers and run.  The builders are pure -- host arrays in, host vectors out -- so the program makes
no HIP runtime call and needs neither the library nor a GPU; what it holds them to (prefix sums, frame counts len / hop + 1, tiles that cover every
sequence exactly once, the rejection codes at the shortest and longest legal lengths) is stated in the program itself."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_layout_builders_hold_their_invariants_under_the_host_sanitizers(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed: " + HIPCC)
    exe = str(tmp_path / "layout_check")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "layout_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("layout_check: ") and r.stdout.rstrip().endswith(" checks"), r.stdout
    assert int(r.stdout.split()[1]) > 1000      # every family of cases ran, not an empty main
