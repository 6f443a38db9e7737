"""The launch plan of the weight gradients (neural_marionette_amd/csrc/nm_wgrad_plan.h), on the host.

nm_launch_wgrad, nm_launch_wgrad_k5occ and the two workspace-size functions take kernel, grid, LDS bytes, partial-sum slots and workspace
floats from that header.  tests/cpp/wgrad_plan.cpp holds it against a pinned table of the network's layers and the op-level test shapes
(written by the decision functions the plan replaced), checks over a sweep that every plan fits the workspace its caller reserves, the
LDS, the kernels' bfloat16 instantiations and the frame-group partition, and checks the first layer's workspace layout."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "neural_marionette_amd", "csrc")


def test_plans_match_the_pinned_table_and_fit_their_workspace(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "wgrad_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "wgrad_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "FAILED" not in r.stdout and "pinned table: 464 rows" in r.stdout and "sweep: 14068320 plans" in r.stdout
    assert ", 0 failed: all plans hold" in r.stdout
