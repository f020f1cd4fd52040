"""The host-compilable pieces of the normalising caller-table kernel
(k_prepare_addends_staged<ed25519_niels_msm, true>, blitzar_amd/csrc/msm/kernels.h), driven by the
stand-alone program tests/native/batch_normalise_check.cc that __graft_entry__.build() compiles
twice -- plain, and under the address and undefined-behaviour sanitizers.  The program prints one
line per check, `<check> <failures> <cases>`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")


def _run(name):
    exe = os.path.join(BUILD, name)
    assert os.path.exists(exe), f"{exe} is missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = {}
    for line in r.stdout.split("\n"):
        if line:
            check, failures, cases = line.split()
            out[check] = (int(failures), int(cases))
    return out


@pytest.fixture(scope="module")
def report():
    return _run("batch_normalise_check")


def test_zero_is_recognised_in_every_encoding(report):
    """0, p and 2 p in loose 51-bit limbs are zero, p +- 1, 2 p +- 1 and +-1 are not; the tree's leaf
    is one() for a zero and for a lane without a row, and the value itself otherwise"""
    assert report["zero_test"] == (0, 10)


def test_niels_of_equals_to_niels_whatever_z(report):
    """niels_of(lambda X, lambda Y, 1 / (lambda Z)) against to_niels of the point, 2000 points"""
    assert report["niels_of"] == (0, 2000)


def test_zero_leaves_do_not_reach_the_shared_product(report):
    """256 leaves with zeros at 0, 63, 64 and 255, the tree's levels in the kernel's order: the
    root is not zero, every other leaf ends as its own inverse, the zero leaves as 1"""
    assert report["tree_with_zero_leaves"] == (0, 257)


def test_clean_under_address_and_undefined_sanitizers(report):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert _run("batch_normalise_check_san") == report
