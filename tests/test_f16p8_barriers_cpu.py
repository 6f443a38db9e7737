"""conv_f16p8_kernel: the MFMA waves and the producer waves meet at the same workgroup barriers.

Both roles take their barriers from neural_marionette_amd/csrc/nm_f16p8_plan.h.  tests/cpp/f16p8_barrier_walk.cpp walks both roles'
control flow on the host with those functions for 1 ... 4 channel chunks and 1 ... 3 bricks per workgroup and compares the sequences."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "neural_marionette_amd", "csrc")


def test_barrier_sequences_match(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "f16p8_barrier_walk")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "f16p8_barrier_walk.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 12 and "MISMATCH" not in r.stdout
