"""The tile digest of the caller tables (blitzar_amd/csrc/msm/tile_digest.h) on the host: the text the
staged prepare kernel runs per wavefront, driven by the stand-alone program
tests/native/tile_digest_check.cc that __graft_entry__.build() compiles twice -- plain, and under the
address and undefined-behaviour sanitizers.  The program prints one line per check,
`<stride> <check> <failures> <cases>`; a changed tile is missed by the kernel exactly when two
digests are equal, so every check counts equal digests and wants none."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")

# generator strides of the four curves (curve25519, bls12-381, bn254 = grumpkin) and, per stride,
# the single-bit flips of one tile of 64 rows
STRIDES = {160: 81920, 104: 53248, 72: 36864}


def _run(name):
    exe = os.path.join(BUILD, name)
    assert os.path.exists(exe), f"{exe} is missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = {}
    for line in r.stdout.split("\n"):
        if line:
            stride, check, failures, cases = line.split()
            out[(int(stride), check)] = (int(failures), int(cases))
    return out


@pytest.fixture(scope="module")
def report():
    return _run("tile_digest_check")


@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_every_bit_flip_changes_the_digest(report, stride):
    """each of the 64 * stride * 8 bits of a random tile in turn; both 64-bit halves change"""
    assert report[(stride, "bit_flip")] == (0, STRIDES[stride])
    assert report[(stride, "bit_flip_either_half")] == (0, STRIDES[stride])


@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_swapped_words_change_the_digest(report, stride):
    """two different 16-byte words exchanged: neighbours (two lanes), 64 words apart (one lane, two
    rounds) and mirrored pairs"""
    failures, cases = report[(stride, "word_swap")]
    assert failures == 0 and cases > 4 * stride


@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_partial_tile_differs_from_its_padding(report, stride):
    """63 rows against the same bytes padded to 64 rows (zeros; row 62 again); 63 rows read 63 rows"""
    assert report[(stride, "partial_tile")] == (0, 2)
    assert report[(stride, "partial_tile_reads_its_rows_only")] == (0, 1)


@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_same_bit_in_several_lanes_changes_the_digest(report, stride):
    """the lanes' states are combined by xor, so equal differences in two or four lanes must not
    cancel: top / lowest bit of either half of a word, last / first word of the lanes, 1500 random
    tiles; neither the digest nor one of its halves stays equal"""
    assert report[(stride, "multi_lane_same_bit")] == (0, 1500 * 16)
    assert report[(stride, "multi_lane_same_bit_either_half")] == (0, 1500 * 16)


@pytest.mark.parametrize("stride", sorted(STRIDES))
def test_every_bit_flip_changes_the_row_digest(report, stride):
    assert report[(stride, "row_bit_flip_either_half")] == (0, stride * 8)


def test_clean_under_address_and_undefined_sanitizers(report):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert _run("tile_digest_check_san") == report
