"""The workspace sizes are part of the interface: callers allocate by them.  The recorded values
(tests/golden/workspace_sizes.json) are what the four *_workspace_bytes functions returned before
the layouts were written over one carver; offsets inside a workspace may move, the totals may not.
The grid crosses the tail-only boundary of the column chain (n = 512 | 513 at round degree <= 5),
the round degrees without a tail, and n that is no power of two.  Needs no backend."""
import itertools
import json
import os

import pytest

from blitzar_amd import api

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "workspace_sizes.json")

SUMCHECK_N = [1, 2, 3, 256, 257, 512, 513, 1027, 2 ** 15, 2 ** 20 + 1]
SUMCHECK_DEGREES = [1, 5, 6, 8]
SUMCHECK_COUNTS = [(1, 1, 1), (12, 5, 13)]  # num_mles, num_products, num_product_terms
INNER_PRODUCT_N = [1, 2, 3, 1000, 2 ** 16]


def sumcheck_cases():
    return list(itertools.product((0, 1), SUMCHECK_N, SUMCHECK_DEGREES, SUMCHECK_COUNTS))


def sumcheck_key(field_id, n, degree, counts):
    return "field=%d n=%d degree=%d mles=%d products=%d terms=%d" % (field_id, n, degree, *counts)


def current_sizes():
    sizes = {"sumcheck_transcript": {}, "sumcheck_transcript_columns": {}, "inner_product": {},
             "inner_product_verify": {}}
    for field_id, n, degree, counts in sumcheck_cases():
        key = sumcheck_key(field_id, n, degree, counts)
        sizes["sumcheck_transcript"][key] = api.sumcheck_transcript_workspace_bytes(
            field_id, n, *counts, degree)
        sizes["sumcheck_transcript_columns"][key] = api.sumcheck_transcript_columns_workspace_bytes(
            field_id, n, *counts, degree)
    for n in INNER_PRODUCT_N:
        sizes["inner_product"]["n=%d" % n] = api.inner_product_workspace_bytes(n)
        sizes["inner_product_verify"]["n=%d" % n] = api.inner_product_verify_workspace_bytes(n)
    return sizes


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return current_sizes()


@pytest.mark.parametrize("function", ["sumcheck_transcript", "sumcheck_transcript_columns",
                                      "inner_product", "inner_product_verify"])
def test_workspace_sizes_are_the_recorded_ones(recorded, current, function):
    expected_entries = (len(sumcheck_cases()) if function.startswith("sumcheck")
                        else len(INNER_PRODUCT_N))
    assert len(recorded[function]) == expected_entries
    assert sorted(current[function]) == sorted(recorded[function])
    different = {key: (current[function][key], want) for key, want in recorded[function].items()
                 if current[function][key] != want}
    assert not different
