"""The sequential model of the multiplicity count (blitzar_amd/csrc/proof/multiplicities.h: the
hash, the slot count, insert and count over one open-addressing table) on the host, driven by the
stand-alone program tests/native/multiplicities_check.cc that __graft_entry__.build() compiles
twice -- plain, and under the address and undefined-behaviour sanitizers.  The program prints its
tables, its lookups and what the model made of them; the Python model (tests/multiplicity_cases.py)
must make the same of the same keys, and the two builds must print the same lines."""
import os
import subprocess

import pytest

from blitzar_amd import api
from tests import multiplicity_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")
CASES = ["wrap", "duplicates", "cluster", "one_row", "two_rows", "all_equal", "no_lookups"]


def _run(name):
    exe = os.path.join(BUILD, name)
    assert os.path.exists(exe), f"{exe} is missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return [line for line in r.stdout.split("\n") if line]


def _numbers(text, base=10):
    return [int(x, base) for x in text.split(",")] if text else []


def _parse(line):
    name, *fields = line.split()
    case = dict(f.split("=") for f in fields)
    return name, {"m": int(case["m"]), "slots": int(case["slots"]),
                  "table": _numbers(case["table"], 16), "first": _numbers(case["first"]),
                  "lookups": _numbers(case["lookups"], 16),
                  "multiplicities": _numbers(case["multiplicities"]),
                  "misses": int(case["misses"]), "longest_probe": int(case["longest_probe"])}


@pytest.fixture(scope="module")
def lines():
    return _run("multiplicities_check")


@pytest.fixture(scope="module")
def report(lines):
    return dict(_parse(line) for line in lines[2:])


def test_slot_count_and_workspace(lines):
    got = {int(m): (int(s), int(w)) for m, s, w in (x.split(":") for x in lines[0].split()[1:])}
    assert got == {0: (0, 0), 1: (2, 264), 2: (4, 272), 3: (8, 288), 4: (8, 288), 5: (16, 320),
                   2**28: (2**29, 2**31 + 256), 2**28 + 1: (0, 0)}
    assert lines[1] == "spread worst=ok"


@pytest.mark.parametrize("kind", ["small", "wide"])
@pytest.mark.parametrize("name", CASES)
def test_model_agrees_with_python(report, name, kind):
    case = report[f"{name}_{kind}"]
    assert len(case["table"]) == case["m"] and case["slots"] == mc.slots(case["m"])
    assert all(first < case["slots"] for first in case["first"])
    assert (case["multiplicities"], case["misses"]) == mc.count(case["table"], case["lookups"])


@pytest.mark.parametrize("kind", ["small", "wide"])
def test_cases_are_what_they_were_built_for(report, kind):
    wrap = report[f"wrap_{kind}"]
    assert wrap["first"] == [15, 15, 15, 15, 0] and wrap["longest_probe"] == 3
    assert wrap["multiplicities"] == [1, 0, 1, 2, 3] and wrap["misses"] == 5
    cluster = report[f"cluster_{kind}"]
    assert cluster["first"] == [100] * 40 and cluster["longest_probe"] == 39
    assert cluster["multiplicities"] == [1] + [0] * 38 + [5] and cluster["misses"] == 5
    duplicates = report[f"duplicates_{kind}"]
    assert duplicates["multiplicities"] == [2, 1, 0, 0, 3, 0, 0] and duplicates["misses"] == 1
    assert report[f"all_equal_{kind}"]["multiplicities"] == [2] + [0] * 8
    assert report[f"no_lookups_{kind}"]["multiplicities"] == [0, 0]


def test_first_slots_are_the_librarys(report):
    """bzamd_multiplicity_first_slot on the same keys (field 0, whose element form is the integer
    itself: every key of the program is below p)"""
    for name, case in report.items():
        for key, first in zip(case["table"], case["first"]):
            element = mc.rows_of(0, [key], 32, raw=True)[0]
            assert api.multiplicity_first_slot(0, element, case["m"]) == first, name


def test_clean_under_address_and_undefined_sanitizers(lines):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert _run("multiplicities_check_san") == lines
