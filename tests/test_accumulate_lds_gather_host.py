"""The wavefront-cooperative row gather of k_accumulate (blitzar_amd/csrc/msm/lds_gather.h) on the
host: the piece mapping the kernel uses and the walk of its 64 lanes, driven by the stand-alone
program tests/native/lds_gather_check.cc that __graft_entry__.build() compiles twice -- plain, and
under the address and undefined-behaviour sanitizers.  The program prints one line per check,
`<check> <failures> <cases>`; every check wants no failure."""
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
    return _run("lds_gather_check")


def test_every_piece_is_fetched_exactly_once(report):
    """7 instructions x 64 lanes = the 448 (lane, chunk) pairs, each once"""
    assert report["pieces_exactly_once"] == (0, 2 * 448)


def test_offsets_stay_inside_the_region(report):
    """landing offsets (aligned, at base + lane * 16, every byte of the 7168 written once) and the
    lanes' read offsets"""
    assert report["offsets_inside_region"] == (0, 448 + 7168 + 448)
    assert report["piece_lands_where_its_lane_reads"] == (0, 448)


def test_lane_reads_its_own_row(report):
    """after a round every lane with an entry reads the 112 bytes of that entry's row, and the entry
    whose sign it applies is that entry; every entry of every task is added exactly once"""
    failures, cases = report["lane_reads_its_row"]
    assert failures == 0 and cases > 100000
    assert report["every_entry_added_once"] == (0, cases)


def test_lanes_without_an_entry_hand_over_supplied_rows_only(report):
    """every row index that reaches an address, from a lane with or without an entry, occurs in the
    task's entries (row 0 never does); no lane has more entries than the wavefront has rounds, lane 0
    has exactly that many; wavefronts behind the task's end take no part"""
    failures, cases = report["handed_rows_were_supplied"]
    assert failures == 0 and cases > 100000
    failures, cases = report["trip_counts"]
    assert failures == 0 and cases > 0
    failures, cases = report["wavefronts_without_entries"]
    assert failures == 0 and cases > 0


def test_clean_under_address_and_undefined_sanitizers(report):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert _run("lds_gather_check_san") == report
