"""Inventory of the library's NM355_* environment switches: every switch a context reads lets a caller's environment choose
which kernels run, so its non-default arm is product code.  Each one must be named by a test (the child-process parity tests
set them), or stand in the allow-list below with the reason it is not."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# switches no test names, and why they are still there
UNTESTED = {
    "NM355_CHAIN_BACKOFF": "its value is a kernel argument of vrnn_prior_chain_kernel: removing it changes that kernel's device code",
    "NM355_HG_DIAG": "it sets a __device__ symbol hg_core_kernel reads: removing it changes that kernel's device code",
}


def _switches_read_by_the_library():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "neural_marionette_amd", "csrc", "*.hip")):
        names.update(re.findall(r"\b(?:getenv|env_int)\(\s*\"(NM355_[A-Z0-9_]+)\"", open(path).read()))
    return sorted(names)


def test_every_switch_is_named_by_a_test():
    switches = _switches_read_by_the_library()
    me = os.path.abspath(__file__)
    tests = "\n".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) if os.path.abspath(p) != me)
    untested = [s for s in switches if not re.search(r"\b%s\b" % s, tests)]
    assert sorted(untested) == sorted(UNTESTED), f"switches no test names: {untested}; allow-list: {sorted(UNTESTED)}"
    assert len(switches) == 35, switches
