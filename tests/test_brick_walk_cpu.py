"""The brick walk of the persistent conv kernels (neural_marionette_amd/csrc/nm_brick_walk.h), on the host.

conv_f16s and the five producer / consumer kernels take their bricks, cout groups and channel chunks from that header.
tests/cpp/brick_walk.cpp walks every workgroup of a launch with the same functions - brick depth 4 and 8, with and without cout groups,
1 / 2 / 8 chunks, linear order on small odd grids and the XCD super-tile order at 256 workgroups, with the multiply-high decode and with
plain divisions - and requires every (frame, brick, cout group, chunk) exactly once."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "neural_marionette_amd", "csrc")


def test_every_step_visited_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "brick_walk")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "brick_walk.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "FAILED" not in r.stdout and r.stdout.count(" ok\n") == 769 and "769 cases, 0 failed" in r.stdout
