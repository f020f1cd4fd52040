"""The plain C++ half of blitzar_amd/csrc/proof/select_rows.h (the span partition, the rank of a
lane from a wavefront's four ballots, the workspace size) on the host, driven by the stand-alone
program tests/native/select_rows_check.cc, which checks it and a sequential model of the two
launches built from it against plain loops.  This test compiles the program itself with g++, once
plain and once under the address and undefined-behaviour sanitizers, runs both, compares their
lines and checks the printed partitions and workspace sizes once more."""
import os
import subprocess

import pytest

from blitzar_amd import api
from tests import select_row_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "native", "select_rows_check.cc")
FLAGS = {"plain": ["-O2"],
         "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = {}
    for name, flags in FLAGS.items():
        exe = str(tmp_path_factory.mktemp("select_rows_check") / name)
        subprocess.run(["g++", *flags, "-std=c++20", "-I" + ROOT, SOURCE, "-o", exe], check=True,
                       timeout=600)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        out[name] = [line for line in r.stdout.split("\n") if line]
    return out


def _fields(line):
    return {k: int(v) for k, v in (f.split("=") for f in line.split()[1:])}


def test_program_agrees_with_its_own_loops(lines):
    assert lines["plain"][-1] == "ok" and not any("MISMATCH" in x for x in lines["plain"])


def test_clean_under_address_and_undefined_sanitizers(lines):
    """the same program built with -fsanitize=address,undefined (reports are fatal): same lines"""
    assert lines["san"] == lines["plain"]


def test_partitions_are_the_models(lines):
    """the printed partitions, the edges of the span count among them, against the model's"""
    cases = [_fields(x) for x in lines["plain"] if x.startswith("partition ")]
    sizes = {c["n"] for c in cases}
    tile = sc.TILE
    assert {0, 1, tile - 1, tile, tile + 1, 3 * tile + 1, 2048 * tile - 1, 2048 * tile,
            2048 * tile + 1, 4096 * tile - 1, 4096 * tile, 4096 * tile + 1, 2**30} <= sizes
    for c in cases:
        assert (c["spans"], c["tiles_per_span"]) == sc.spans(c["n"]), c
    assert max(c["spans"] for c in cases) == sc.MAX_SPANS


def test_models_ran(lines):
    cases = [_fields(x) for x in lines["plain"] if x.startswith("model ")]
    assert {c["width"] for c in cases} == set(range(1, 9))
    assert any(c["kept"] == 0 for c in cases) and any(c["kept"] == c["n"] > 0 for c in cases)
    assert any(c["n"] > 2 * sc.TILE * sc.MAX_SPANS and 0 < c["kept"] < c["n"] for c in cases)
    ranks, = (_fields(x) for x in lines["plain"] if x.startswith("ranks "))
    assert ranks["masks"] >= 256


def test_workspace_is_the_librarys(lines):
    line = next(x for x in lines["plain"] if x.startswith("workspace"))
    got = [tuple(int(v) for v in x.split(":")) for x in line.split()[1:]]
    assert len(got) == 10
    for n, size in got:
        assert api.select_rows_workspace_bytes(n) == size == sc.workspace_bytes(n), n
