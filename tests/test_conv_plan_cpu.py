"""The launch plan of the forward convs (neural_marionette_amd/csrc/nm_conv_plan.h), on the host.

nm_launch_conv, nm_launch_conv_up2c, nm_conv_blocks_per_frame and the routing questions of nm_net.hip take kernel, instantiation, grid,
LDS bytes, the ConvParams integers and the GroupNorm partial rows from that header.  tests/cpp/conv_plan.cpp holds it against a pinned
table of the network's layers and the op-level test shapes (written by the decision code the plan replaced), checks over a sweep that
every plan fits the LDS, names a kernel instantiation that exists, sizes its partial rows as the kernel indexes them and never below the
conv mode 0 plan's, and checks the three routing queries against the full plan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "neural_marionette_amd", "csrc")


def test_plans_match_the_pinned_table_and_size_their_partial_rows(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "conv_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "conv_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "FAILED" not in r.stdout and "pinned table: 695 rows" in r.stdout and "sweep: 3500684 plans, 1297706 not refused" in r.stdout
    assert "queries: 268800 shapes" in r.stdout and ", 0 failed: all plans hold" in r.stdout
