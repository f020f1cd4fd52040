"""The halved Z = 1 addend of curve25519, ((y+x)/2, (y-x)/2, d x y), on the host
(blitzar_amd/csrc/curve/ed29.h: to_niels, add_niels, from_niels; msm/curve_traits.h: niels_of) and
the 32-bit piece offsets of k_accumulate's row gather (msm/lds_gather.h), driven by the stand-alone
program tests/native/niels_halved_check.cc that __graft_entry__.build() compiles twice -- plain, and
under the address and undefined-behaviour sanitizers.  The program prints `<check> <failures>
<cases>` per check, every check wants no failure, and `max <name> <value>` / `min <name> <value>`
for what the bounds check saw."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")


def _run(name):
    exe = os.path.join(BUILD, name)
    assert os.path.exists(exe), f"{exe} is missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    checks, seen = {}, {}
    for line in r.stdout.split("\n"):
        if not line:
            continue
        first, second, third = line.split()
        if first in ("max", "min"):
            seen[second] = float(third)
        else:
            checks[first] = (int(second), int(third))
    return checks, seen


@pytest.fixture(scope="module")
def report():
    return _run("niels_halved_check")


def test_stored_form_is_the_halved_affine_triple(report):
    """to_niels and niels_of, doubled, against y + x, y - x and 2d x y of the affine point: the
    identity, (0, -1), 598 other points, each as it stands, scaled to another Z, and with unreduced
    X, Y and Z; limbs below the bound of a product's output, padding zero"""
    assert report[0]["stored_form"] == (0, 600 * 3 * 2)


def test_addition_and_first_entry_match_the_general_addition(report):
    """add_niels, from_niels and the traits' accumulate / first against ed29::add, both signs"""
    assert report[0]["addition_matches_add"] == (0, 500 * 2 * 4)


def test_chains_pass_through_the_identity(report):
    """8 chains of 64 additions that alternate P and -P, from the identity and from a loaded -P: every
    step against ed29::add, and the accumulator is (0 : z : z : 0) where it must be"""
    assert report[0]["chains_through_identity"] == (0, 8 * 64)


def test_contract_of_the_seven_products(report):
    """add_niels rebuilt in 128-bit integers from accumulators and rows whose limbs sit at the largest
    value a product leaves (and at zero, and mixed), fed back for several steps: no column sum
    reaches 2^64, no limb-wise subtraction goes below zero, every limb fits 32 bits, a product's
    output stays below 2^29 + 2^18, the largest B(f) B(g) is at most 6 in units of that bound, and
    the rebuilt limbs are the code's"""
    checks, seen = report
    print(seen)
    failures, cases = checks["contract"]
    assert failures == 0 and cases > 10000
    assert seen["high_column_over_2_64"] < 1.0
    assert seen["low_column_over_2_64"] < 1.0
    assert seen["product_limb_over_unit"] < 1.0
    assert seen["limb_over_2_32"] < 1.0
    assert seen["b_times_b"] <= 6.0
    assert seen["sub_limb"] >= 0


def test_piece_offsets_32_bit_equal_the_64_bit_address(report):
    """row << 7 | chunk << 4 is row * 128 + chunk * 16 for every piece of tasks narrow_offsets
    admits, whose last piece ends inside 4 GiB; tasks that can name a row beyond are refused (the
    64-bit form, which no test shape reaches on a device, is the parent's address arithmetic)"""
    failures, cases = report[0]["piece_offsets"]
    assert failures == 0 and cases > 5000


def test_clean_under_address_and_undefined_sanitizers(report):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert _run("niels_halved_check_san") == report
