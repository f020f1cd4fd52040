"""The verifier's checks in front of the inner-product verifier (include/blitzar_amd.h), the forms
on host operands: bzamd_check_sumcheck_evaluations against Python integers,
bzamd_combine_commitments on the host backend against commitments of known logarithm, the three
workspace functions, the aborts of every new entry point, and the compiler's resource report of
proof/verify_opening.hip.  The device forms are in tests/test_verify_opening_device.py, on the same
cases (tests/verify_opening_cases.py)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import merlin_ref, refmath
from tests.test_inner_product_verify_device import host_rejects
from tests.test_sumcheck_device import MODULUS, make_inputs, to_int
from tests.verify_opening_cases import (REJECTION_CLASSES, Commitments, Proof, Statement,
                                        decode_class, encoding_of, fail_rounds_of, flipped,
                                        raw_element, rejected_encodings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [1, 3, 64, 65, 1000]


#--------------------------------------------------------------------------------------------------
# the proofs the device tests verify: the Python transcript against the host verifier
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,d", [(1, 1), (3, 2), (5, 8)])
def test_constructed_proofs_are_what_the_host_verifier_says(field_id, v, d):
    """the proofs of tests/verify_opening_cases.py need no prover; the host verifier (pinned to
    the reference elsewhere) accepts them, fails where they are made to fail, and leaves the
    bytes the Python transcript leaves"""
    from blitzar_amd import api  # noqa: F401  (the host verifier needs no backend)
    t0 = merlin_ref.padded_starts()[37 + d]
    for seed, fail_round in enumerate(fail_rounds_of(v)):
        proof = Proof(field_id, v, d, t0, 500 + seed, fail_round)
        assert proof.ok == (fail_round is None)
        proof.check_host()


#--------------------------------------------------------------------------------------------------
# the final evaluation check
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("num_products", [1, 5, 200])
def test_evaluation_check_host_form(field_id, num_products):
    """needs no backend; multipliers and evaluations at 0, 1, p - 1 and unreduced; the expected sum
    canonical or unreduced; any one bit of it flipped gives 0"""
    from blitzar_amd import api
    for seed in range(4):
        st = Statement(field_id, num_products, 40 + seed)
        evaluations, values = st.evaluations(60 + seed)
        want = st.expected_sum(values)
        for unreduced in (False, True):
            expected = raw_element(field_id, want, unreduced)
            passed = evaluations.copy()
            assert api.check_sumcheck_evaluations(field_id, expected, passed, st.table, st.terms)
            assert np.array_equal(passed, evaluations)
            for bit in (0, 77 + seed, 251):
                assert not api.check_sumcheck_evaluations(field_id, flipped(expected, bit),
                                                          evaluations, st.table, st.terms), bit
        wrong = raw_element(field_id, (want + 1) % MODULUS[field_id])
        assert not api.check_sumcheck_evaluations(field_id, wrong, evaluations, st.table, st.terms)


def test_evaluation_check_closes_a_proven_sumcheck(cpu_backend):
    """the identity it stands for: behind the library's own prover and verifier the check holds,
    and fails for another evaluation"""
    for field_id in (0, 1):
        n, num_mles, products = 37, 5, [[0, 1, 2, 3], [4, 0], [2]]
        mles, _, table, terms, degree = make_inputs(field_id, n, num_mles, products, 91)
        t0 = merlin_ref.Transcript(label="closing").array()
        polys, _, evaluations, _ = cpu_backend.prove_sumcheck_transcript(
            field_id, mles, table, terms, n, degree, t0)
        p = MODULUS[field_id]
        claimed = 0
        for i in range(n):
            at = 0
            for t in products:
                term = to_int(field_id, table[at][:32])
                for j in t:
                    term = term * to_int(field_id, mles[j, i]) % p
                claimed, at = (claimed + term) % p, at + 1
        ok, expected, _, _ = cpu_backend.verify_sumcheck(field_id, raw_element(field_id, claimed),
                                                         polys, t0)
        assert ok
        assert cpu_backend.check_sumcheck_evaluations(field_id, expected, evaluations, table, terms)
        evaluations[2] = flipped(evaluations[2], 9)
        assert not cpu_backend.check_sumcheck_evaluations(field_id, expected, evaluations, table,
                                                          terms)


#--------------------------------------------------------------------------------------------------
# combining compressed commitments
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_combine_commitments_host_backend(cpu_backend, count):
    """sum_j c_j encode(k_j B) = encode((sum_j c_j k_j mod l) B); coefficients at 0, l - 1, l and
    2^256 - 1, the identity's encoding among the commitments; the inputs are what they were"""
    case = Commitments(count, 700 + count)
    commitments, coefficients = case.commitments.copy(), case.coefficients.copy()
    valid, combined = cpu_backend.combine_commitments(commitments, coefficients)
    assert valid
    assert np.array_equal(encoding_of(combined), case.expected_encoding())
    assert np.array_equal(commitments, case.commitments)
    assert np.array_equal(coefficients, case.coefficients)


def test_rejection_classes_are_what_the_host_decoder_rejects():
    encodings = rejected_encodings()
    assert sorted(encodings) == sorted(REJECTION_CLASSES)
    for why, raw in encodings.items():
        s = int.from_bytes(raw.tobytes(), "little")
        assert decode_class(s) == why
        assert host_rejects(s), why
    assert decode_class(0) is None and not host_rejects(0)


@pytest.mark.parametrize("why", REJECTION_CLASSES)
def test_combine_commitments_rejected_encoding(cpu_backend, why):
    """returns 0, and the sum is that of the other terms"""
    encoding = rejected_encodings()[why]
    for count, at in ((1, 0), (65, 64), (65, 7)):
        case = Commitments(count, 800 + count + at, {at: encoding})
        valid, combined = cpu_backend.combine_commitments(case.commitments, case.coefficients)
        assert not valid
        assert np.array_equal(encoding_of(combined), case.expected_encoding())


def test_combine_commitments_every_class_at_once(cpu_backend):
    encodings = rejected_encodings()
    case = Commitments(64, 850, {3 + 13 * k: encodings[why] for k, why in enumerate(REJECTION_CLASSES)})
    valid, combined = cpu_backend.combine_commitments(case.commitments, case.coefficients)
    assert not valid
    assert np.array_equal(encoding_of(combined), case.expected_encoding())


#--------------------------------------------------------------------------------------------------
# workspace sizes
#--------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    """no backend needed; 0 for what the calls reject; monotone in every argument"""
    from blitzar_amd import api
    size = api.check_sumcheck_evaluations_workspace_bytes
    for field_id in (0, 1):
        assert size(field_id, 0, 0) == 0
        assert size(field_id, 0, 5) == 0
        assert size(field_id, 3, 2) == 0       # a product without a term
        assert size(field_id, 1, 1) > 0
        counts = [1, 2, 7, 8, 9, 200, 1000, 1 << 16]
        for a, b in zip(counts, counts[1:]):
            for extra in (0, 1, 1000):
                assert size(field_id, a, b + extra) <= size(field_id, b, b + extra)
                assert size(field_id, a, a + extra) <= size(field_id, a, b + extra)
        # the products (an element and two words each) and the terms, padded: nothing else
        assert size(field_id, 200, 900) <= 200 * 64 + 4 * 900 + 1024
    assert size(2, 3, 5) == 0

    size = api.combine_commitments_workspace_bytes
    assert size(0) == 0
    assert size((1 << 28) + 1) == 0
    counts = [1, 2, 3, 64, 65, 1000, 1 << 20, 1 << 28]
    for a, b in zip(counts, counts[1:]):
        assert 0 < size(a) <= size(b)
    for count in counts:
        assert 160 * count <= size(count) <= 160 * count + 1024


#--------------------------------------------------------------------------------------------------
# aborts (host backend; each in a child process)
#--------------------------------------------------------------------------------------------------
PRE = ("import ctypes\nlib = api.load()\n"
       "def buf(n):\n    return np.zeros(n, np.uint8)\n"
       "b = [buf(4096) for _ in range(8)]\n"
       "p = [x.ctypes.data for x in b]\n")
VERIFY = "lib.bzamd_verify_sumcheck_device({}, {}, {}, {}, {}, {}, {}, {}, {}, None)\n"
NULL_VERIFY = "null argument to `bzamd_verify_sumcheck_device`"
# one product of two terms over three MLEs, field 0
STATEMENT = ("table = np.zeros((1, 36), np.uint8)\ntable[0, 32] = {length}\n"
             "terms = np.array({terms}, np.uint32)\n")
CHECK = ("lib.bzamd_check_sumcheck_evaluations({field}, p[0], p[1], {mles}, table.ctypes.data, "
         "terms.ctypes.data, 1, {count})\n")
CHECK_DEVICE = ("lib.bzamd_check_sumcheck_evaluations_device({}, 0, {}, {}, 3, {}, {}, 1, 2, {}, {}, "
                "4096, None)\n")
NULL_CHECK_DEVICE = "null argument to `bzamd_check_sumcheck_evaluations_device`"
GOOD = STATEMENT.format(length=2, terms=[0, 2])
TT = "table.ctypes.data", "terms.ctypes.data"
COMBINE = "lib.bzamd_combine_commitments({}, {}, {}, {})\n"
COMBINE_DEVICE = "lib.bzamd_combine_commitments_device({}, {}, {}, {}, {}, {}, 4096, None)\n"
NULL_COMBINE_DEVICE = "null argument to `bzamd_combine_commitments_device`"
LIMITS = "the commitment combination needs 1 <= num_commitments <= 2^28"
NEEDS_GPU = "device entry points need the GPU backend"
ABORTS = {
    "verify_null_verdicts": (VERIFY.format(None, "p[1]", "p[2]", "p[3]", 0, "p[4]", 2, 2, 1),
                             NULL_VERIFY),
    "verify_null_sums": (VERIFY.format("p[0]", None, "p[2]", "p[3]", 0, "p[4]", 2, 2, 1), NULL_VERIFY),
    "verify_null_points": (VERIFY.format("p[0]", "p[1]", None, "p[3]", 0, "p[4]", 2, 2, 1),
                           NULL_VERIFY),
    "verify_null_transcripts": (VERIFY.format("p[0]", "p[1]", "p[2]", None, 0, "p[4]", 2, 2, 1),
                                NULL_VERIFY),
    "verify_null_polynomials": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, None, 2, 2, 1),
                                NULL_VERIFY),
    "verify_no_variables": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]", 0, 2, 1),
                            "sumcheck verification needs num_variables > 0 and round_degree > 0"),
    "verify_degree_0": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]", 2, 0, 1),
                        "sumcheck verification needs num_variables > 0 and round_degree > 0"),
    "verify_degree_9": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]", 2, 9, 1),
                        "round_degree must be in [1, 8]"),
    "verify_no_proofs": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]", 2, 2, 0),
                         "the sumcheck verifier needs at least one proof"),
    "verify_field_2": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 2, "p[4]", 2, 2, 1),
                       "unsupported field id"),
    "verify_on_cpu": (VERIFY.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]", 2, 2, 1), NEEDS_GPU),
    "check_null_sum": (GOOD + "lib.bzamd_check_sumcheck_evaluations(0, None, p[1], 3, "
                       "table.ctypes.data, terms.ctypes.data, 1, 2)\n",
                       "null argument to `bzamd_check_sumcheck_evaluations`"),
    "check_null_evaluations": (GOOD + "lib.bzamd_check_sumcheck_evaluations(0, p[0], None, 3, "
                               "table.ctypes.data, terms.ctypes.data, 1, 2)\n",
                               "null argument to `bzamd_check_sumcheck_evaluations`"),
    "check_null_table": (GOOD + "lib.bzamd_check_sumcheck_evaluations(0, p[0], p[1], 3, None, "
                         "terms.ctypes.data, 1, 2)\n",
                         "null argument to `bzamd_check_sumcheck_evaluations`"),
    "check_null_terms": (GOOD + "lib.bzamd_check_sumcheck_evaluations(0, p[0], p[1], 3, "
                         "table.ctypes.data, None, 1, 2)\n",
                         "null argument to `bzamd_check_sumcheck_evaluations`"),
    "check_product_without_terms": (STATEMENT.format(length=0, terms=[0])
                                    + CHECK.format(field=0, mles=3, count=0),
                                    "a sumcheck product must have at least one term"),
    "check_term_past_the_mles": (STATEMENT.format(length=2, terms=[0, 3])
                                 + CHECK.format(field=0, mles=3, count=2),
                                 "product term refers to a missing MLE"),
    "check_terms_do_not_match": (GOOD + CHECK.format(field=0, mles=3, count=3),
                                 "num_product_terms does not match the product table"),
    "check_no_mles": (GOOD + CHECK.format(field=0, mles=0, count=2),
                      "the evaluation check needs at least one MLE and one product"),
    "check_field_2": (GOOD + CHECK.format(field=2, mles=3, count=2), "unsupported field id"),
    "check_device_null_verdicts": (GOOD + CHECK_DEVICE.format(None, "p[1]", "p[2]", *TT, 1, "p[3]"),
                                   NULL_CHECK_DEVICE),
    "check_device_null_workspace": (GOOD + CHECK_DEVICE.format("p[0]", "p[1]", "p[2]", *TT, 1, None),
                                    NULL_CHECK_DEVICE),
    "check_device_no_proofs": (GOOD + CHECK_DEVICE.format("p[0]", "p[1]", "p[2]", *TT, 0, "p[3]"),
                               "the evaluation check needs at least one proof"),
    "check_device_on_cpu": (GOOD + CHECK_DEVICE.format("p[0]", "p[1]", "p[2]", *TT, 1, "p[3]"),
                            NEEDS_GPU),
    "combine_null_combined": (COMBINE.format(None, "p[1]", "p[2]", 1),
                              "null argument to `bzamd_combine_commitments`"),
    "combine_null_commitments": (COMBINE.format("p[0]", None, "p[2]", 1),
                                 "null argument to `bzamd_combine_commitments`"),
    "combine_null_coefficients": (COMBINE.format("p[0]", "p[1]", None, 1),
                                  "null argument to `bzamd_combine_commitments`"),
    "combine_none": (COMBINE.format("p[0]", "p[1]", "p[2]", 0), LIMITS),
    "combine_too_many": (COMBINE.format("p[0]", "p[1]", "p[2]", 2**28 + 1), LIMITS),
    "combine_device_null_valid": (COMBINE_DEVICE.format("p[0]", None, "p[2]", "p[3]", 1, "p[4]"),
                                  NULL_COMBINE_DEVICE),
    "combine_device_null_workspace": (COMBINE_DEVICE.format("p[0]", "p[1]", "p[2]", "p[3]", 1, None),
                                      NULL_COMBINE_DEVICE),
    "combine_device_none": (COMBINE_DEVICE.format("p[0]", "p[1]", "p[2]", "p[3]", 0, "p[4]"), LIMITS),
    "combine_device_too_many": (COMBINE_DEVICE.format("p[0]", "p[1]", "p[2]", "p[3]", 2**28 + 1,
                                                      "p[4]"), LIMITS),
    "combine_device_on_cpu": (COMBINE_DEVICE.format("p[0]", "p[1]", "p[2]", "p[3]", 1, "p[4]"),
                              NEEDS_GPU),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_arguments_abort(name):
    call, message = ABORTS[name]
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            + PRE + call)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# the kernels' resources
#--------------------------------------------------------------------------------------------------
def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/verify_opening.hip with the flags the library
    is built with: no kernel of the verifier's side uses scratch memory, both fields"""
    from blitzar_amd import build
    src = "proof/verify_opening.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "verify_opening.o")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None:
            scratch[name] = int(m.group(1))
    print(scratch)
    for kernel, variants in (("k_verify_sumcheck", 2), ("k_check_evaluations", 2),
                             ("k_decode_commitments", 1)):
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == variants, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
    assert len(scratch) == 5, sorted(scratch)
