"""The plain C++ half of blitzar_amd/csrc/proof/key_sums.h (the chunk split, the signed
accumulation, the recombination into a wide two's-complement integer) on the host, driven by the
stand-alone program tests/native/key_sums_check.cc, which checks it against 320-bit arithmetic of
its own at the accumulator bounds and on random rows.  This test compiles the program itself with g++,
once plain and once under the address and undefined-behaviour sanitizers, runs both, compares
their lines and checks the printed sums once more with Python integers."""
import os
import subprocess

import pytest

from blitzar_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "key_sums_check.cc")
FLAGS = {"plain": ["-O2"],
         "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = {}
    for name, flags in FLAGS.items():
        exe = str(tmp_path_factory.mktemp("key_sums_check") / name)
        subprocess.run(["g++", *flags, "-std=c++20", "-I" + ROOT, SOURCE, "-o", exe], check=True,
                       timeout=600)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        out[name] = [line for line in r.stdout.split("\n") if line]
    return out


def _fields(line):
    return dict(f.split("=") for f in line.split()[1:])


def _signed(hex_digits):
    value = int(hex_digits, 16)
    return value - (1 << 320) if value >> 319 else value


def test_program_agrees_with_its_own_arithmetic(lines):
    assert lines["plain"][-1] == "ok" and not any("MISMATCH" in x for x in lines["plain"])


def test_clean_under_address_and_undefined_sanitizers(lines):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert lines["san"] == lines["plain"]


def test_bounds_against_python_integers(lines):
    """every accumulator at +-(2^62 - 1): sum_k acc_k 2^(32 k), its sign and its magnitude"""
    bounds = [_fields(x) for x in lines["plain"] if x.startswith("bounds ")]
    assert len(bounds) == 256
    most = (1 << 62) - 1
    for case in bounds:
        signs = int(case["signs"], 16)
        want = sum((-most if (signs >> k) & 1 else most) << (32 * k) for k in range(8))
        assert _signed(case["wide"]) == want
        assert int(case["negative"]) == (want < 0) and int(case["magnitude"], 16) == abs(want)
    assert max(abs(_signed(c["wide"])) for c in bounds) < 1 << 287


def test_random_rows(lines):
    cases = [_fields(x) for x in lines["plain"] if x.startswith("random ")]
    assert len(cases) == 12 + 9   # twelve widths unsigned, nine of them signed as well
    assert all(c["wide"] == c["sum"] for c in cases)
    assert any(_signed(c["sum"]) < 0 for c in cases) and any(_signed(c["sum"]) > 0 for c in cases)
    assert {int(c["chunks"]) for c in cases} == {1, 2, 3, 4, 5, 8}


def test_workspace_is_the_librarys(lines):
    line = next(x for x in lines["plain"] if x.startswith("workspace"))
    got = [tuple(int(v) for v in x.split(":")) for x in line.split()[1:]]
    assert len(got) == 32
    for m, values, size in got:
        assert api.sum_by_key_workspace_bytes(m, values) == size, (m, values)
