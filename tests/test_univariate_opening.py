"""The field work of a HyperKZG opening (include/blitzar_amd.h: bzamd_fold_polynomial,
bzamd_evaluate_polynomials, bzamd_batch_quotients), host forms on the host backend.

Every expected value is Python integers (tests/univariate_cases.py) and every comparison is of
bytes.  The opening is checked without a pairing: with generators G_i = tau^i G for a known tau the
commitments satisfy (tau - u_k) C(h_k) + remainders[k] G = sum_i q^i C(P_i).  The device forms are in
tests/test_univariate_opening_device.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import univariate_cases as uc
from tests.test_mle_opening import expected_vector, point_of
from tests.test_sumcheck_device import MODULUS, to_bytes, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 1), (1, 2), (2, 3), (3, 5), (3, 8), (5, 3), (10, 513), (11, 1025), (30, 3)]


#--------------------------------------------------------------------------------------------------
# the model checks itself
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
def test_model_quotient_identity(field_id):
    """B == (X - u) h + remainder, coefficient by coefficient"""
    p = MODULUS[field_id]
    for seed in (0, 1, 2, 3):
        case = uc.Opening(field_id, 6, 37, seed, num_points=4)
        b = case.batched()
        hs, remainders = case.quotients()
        evaluations = case.evaluations()
        for k, u in enumerate(case.points):
            h = hs[k]
            assert h[-1] == 0
            product = [((h[j - 1] if j > 0 else 0) - u * h[j]) % p for j in range(len(b))]
            product[0] = (product[0] + remainders[k]) % p
            assert product == b
            assert remainders[k] == uc.evaluate(field_id, b, u)
            assert remainders[k] == sum(pow(case.q, i, p) * e
                                        for i, e in enumerate(evaluations[k])) % p


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", [(1, 1), (1, 2), (4, 11), (6, 37), (7, 3)])
def test_model_evaluation_is_the_inner_product_with_the_evaluation_vector(field_id, v, n):
    p = MODULUS[field_id]
    case = uc.Opening(field_id, v, n, 5)
    vector = expected_vector(field_id, case.point, n)
    assert case.evaluation == sum(a * b for a, b in zip(case.p0, vector)) % p


def test_folded_layout():
    want = [(0, 2)] + [(2 + i, 1) for i in range(28)]
    assert uc.folded_layout(3, 30) == want
    assert api.folded_layout(3, 30) == want
    assert api.folded_layout(5, 1) == [] and api.folded_layout(1, 2) == [(0, 1)]
    assert api.folded_layout(1025, 11)[:3] == [(0, 513), (513, 257), (770, 129)]
    for n, v in ((1025, 11), (37, 6), (3, 30)):
        layout = api.folded_layout(n, v)
        assert layout == uc.folded_layout(n, v)
        assert layout[-1][0] + layout[-1][1] <= n + v


#--------------------------------------------------------------------------------------------------
# host forms against the model
#--------------------------------------------------------------------------------------------------
def run_host_forms(lib_api, case, num_points):
    """fold, evaluate and divide through the host forms, each checked byte for byte"""
    f, v, n = case.field_id, case.num_variables, case.n
    polynomial = case.polynomial_bytes()
    keep = polynomial.copy()
    folded, scalars, evaluation = lib_api.fold_polynomial(f, polynomial, case.point_bytes())
    assert np.array_equal(folded, case.folded_bytes())
    assert np.array_equal(scalars, case.folded_bytes(scalar=True))
    assert np.array_equal(evaluation, to_bytes(f, case.evaluation))
    points = case.points_bytes()[:num_points]
    got = lib_api.evaluate_polynomials(f, polynomial, folded, points, v)
    want = case.evaluations()[:num_points]
    assert got.shape == (num_points, v, 32)
    for k in range(num_points):
        assert np.array_equal(got[k], uc.element_rows(f, want[k])), f"point {k}"
    quotients, remainders = lib_api.batch_quotients(f, polynomial, folded, case.q_bytes(), points, v)
    hs, rs = case.quotients()
    for k in range(num_points):
        assert np.array_equal(quotients[k], uc.scalar_rows(f, hs[k])), f"point {k}"
        assert not quotients[k][n - 1].any()
    assert np.array_equal(remainders, uc.element_rows(f, rs[:num_points]))
    assert np.array_equal(polynomial, keep), "the polynomial was modified"
    return folded, scalars, quotients, remainders


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("v,n", CASES)
def test_host_forms(cpu_backend, field_id, v, n):
    p = MODULUS[field_id]
    for seed, num_points, q in ((0, 3, None), (1, 4, 0), (2, 1, 1), (3, 4, None)):
        case = uc.Opening(field_id, v, n, seed, num_points=4, q=q)
        run_host_forms(cpu_backend, case, num_points)
    assert {0, 1, p - 1} <= {u for seed in (1, 2, 3) for u in uc.points_of(field_id, 4, seed)}


@pytest.mark.parametrize("field_id", [0, 1])
def test_unreduced_rows(cpu_backend, field_id):
    """rows at and above the modulus mean their residues"""
    p, v, n = MODULUS[field_id], 3, 6
    top = (1 << 256) - 1 if field_id == 0 else p + 5
    raw = [top, p, p + 1, p - 1, 7, 0]
    polynomial = np.stack([np.frombuffer(x.to_bytes(32, "little"), np.uint8) for x in raw])
    scale = pow(1 << 256, -1, p) if field_id == 1 else 1
    case = uc.Opening(field_id, v, n, 9)
    case.p0 = [x * scale % p for x in raw]
    case.levels, case.evaluation = uc.levels(field_id, case.p0, case.point)
    folded, scalars, evaluation = cpu_backend.fold_polynomial(field_id, polynomial,
                                                              case.point_bytes())
    assert np.array_equal(folded, case.folded_bytes())
    assert np.array_equal(evaluation, to_bytes(field_id, case.evaluation))
    points = case.points_bytes()
    got = cpu_backend.evaluate_polynomials(field_id, polynomial, folded, points, v)
    for k, want in enumerate(case.evaluations()):
        assert np.array_equal(got[k], uc.element_rows(field_id, want))
    quotients, remainders = cpu_backend.batch_quotients(field_id, polynomial, folded,
                                                        case.q_bytes(), points, v)
    hs, rs = case.quotients()
    for k in range(3):
        assert np.array_equal(quotients[k], uc.scalar_rows(field_id, hs[k]))
    assert np.array_equal(remainders, uc.element_rows(field_id, rs))


@pytest.mark.parametrize("field_id", [0, 1])
def test_optional_outputs(cpu_backend, field_id):
    case = uc.Opening(field_id, 4, 11, 3)
    polynomial, point = case.polynomial_bytes(), case.point_bytes()
    folded, scalars, evaluation = cpu_backend.fold_polynomial(field_id, polynomial, point)
    if field_id == 0:
        assert np.array_equal(scalars, folded)
    else:
        plain = [to_int(1, row) for row in folded]
        assert uc.scalar_values(scalars) == plain
    # null pointers: nothing is written anywhere near
    lib = cpu_backend.load()
    rows = folded.shape[0]
    again = np.full((rows + 2, 32), 0x5A, np.uint8)
    lib.bzamd_fold_polynomial(again.ctypes.data, None, None, field_id, polynomial.ctypes.data, 11,
                              point.ctypes.data, 4)
    assert np.array_equal(again[:rows], folded) and np.all(again[rows:] == 0x5A)
    only, none_scalars, none_evaluation = cpu_backend.fold_polynomial(
        field_id, polynomial, point, scalars=None, evaluation=None)
    assert np.array_equal(only, folded) and none_scalars is None and none_evaluation is None
    out = np.full((3 * 11 + 2, 32), 0x5A, np.uint8)
    q, points = case.q_bytes(), case.points_bytes()
    lib.bzamd_batch_quotients(out.ctypes.data, None, field_id, polynomial.ctypes.data,
                              folded.ctypes.data, 11, 4, q.ctypes.data, points.ctypes.data, 3)
    hs, _ = case.quotients()
    for k in range(3):
        assert np.array_equal(out[11 * k:11 * (k + 1)], uc.scalar_rows(field_id, hs[k]))
    assert np.all(out[33:] == 0x5A)
    quotients, none_remainders = cpu_backend.batch_quotients(field_id, polynomial, folded, q,
                                                             points, 4, remainders=None)
    assert none_remainders is None and np.array_equal(quotients.reshape(-1, 32), out[:33])


#--------------------------------------------------------------------------------------------------
# the opening without a pairing (field 1, BN254 G1)
#--------------------------------------------------------------------------------------------------
def commit(lib_api, columns, generators):
    out = lib_api.compute_pedersen_commitments(api.SXT_CURVE_BN_254,
                                               [(c, False) for c in columns], generators=generators)
    return [uc.affine_point(row) for row in out]


@pytest.mark.parametrize("n", [64, 37])
def test_opening_equation_without_a_pairing(cpu_backend, n):
    v = 6
    case = uc.Opening(1, v, n, 0)
    polynomial = case.polynomial_bytes()
    folded, scalars, evaluation = cpu_backend.fold_polynomial(1, polynomial, case.point_bytes())
    points = case.points_bytes()
    evaluations = cpu_backend.evaluate_polynomials(1, polynomial, folded, points, v)
    quotients, remainders = cpu_backend.batch_quotients(1, polynomial, folded, case.q_bytes(),
                                                        points, v)
    generators = uc.affine_bytes(uc.tau_generators(64))
    p0_scalars = uc.scalar_rows(1, case.p0)
    columns = [p0_scalars] + [scalars[off:off + length] for off, length in api.folded_layout(n, v)]
    level_commitments = commit(cpu_backend, columns, generators)
    quotient_commitments = commit(cpu_backend, [quotients[k] for k in range(3)], generators)
    rs = uc.element_values(1, remainders)
    assert uc.opening_equation_holds(v, case.q, case.points, level_commitments,
                                     quotient_commitments, rs)
    # and the equation notices a wrong remainder
    assert not uc.opening_equation_holds(v, case.q, case.points, level_commitments,
                                         quotient_commitments, [rs[0] + 1] + rs[1:])
    p = MODULUS[1]
    es = [uc.element_values(1, evaluations[k]) for k in range(3)]
    assert rs == [sum(pow(case.q, i, p) * e for i, e in enumerate(es[k])) % p for k in range(3)]


#--------------------------------------------------------------------------------------------------
# workspace sizes
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["evaluate", "quotients"])
def test_workspace_sizes(which):
    size = (api.evaluate_polynomials_workspace_bytes if which == "evaluate"
            else api.batch_quotients_workspace_bytes)
    for field_id in (0, 1):
        assert size(field_id, 5, 3, 3) > 0
        assert size(field_id, 0, 3, 3) == 0
        assert size(field_id, 9, 3, 3) == 0          # n > 2^l
        assert size(field_id, 5, 31, 3) == 0
        assert size(field_id, 5, 0, 3) == 0
        assert size(field_id, 5, 3, 0) == 0
        assert size(field_id, 5, 3, 5) == 0
    assert size(2, 5, 3, 3) == 0
    for t in (1, 3, 4):
        previous = 0
        for n in (1, 2, 1023, 1024, 1025, 2**16, 2**20, 2**20 + 1, 2**22 + 5, 2**26, 2**30 - 1,
                  2**30):
            got = size(1, n, 30, t)
            assert got >= previous, (n, t)
            # B is never materialised: no n x 32 term
            assert got < 64 * 1024 * t + (1 << 20), (n, t)
            previous = got


#--------------------------------------------------------------------------------------------------
# aborts (host backend only; each in a child process)
#--------------------------------------------------------------------------------------------------
SETUP = ("lib = api.load()\n"
         "poly = np.zeros((8, 32), np.uint8); folded = np.zeros((16, 32), np.uint8)\n"
         "scalars = np.zeros((16, 32), np.uint8); point = np.zeros((4, 32), np.uint8)\n"
         "out = np.zeros((64, 32), np.uint8); q = np.zeros(32, np.uint8)\n"
         "space = np.zeros(4096, np.uint8)\n"
         "P, F, S, X, O, Q, W = (a.ctypes.data for a in (poly, folded, scalars, point, out, q, space))\n")
FOLD = "lib.bzamd_fold_polynomial(%s, %s, %s, 0, %s, %s, %s, %s)\n"
EVAL = "lib.bzamd_evaluate_polynomials(%s, 0, %s, %s, %s, %s, %s, %s)\n"
QUOT = "lib.bzamd_batch_quotients(%s, %s, 0, %s, %s, %s, %s, %s, %s, %s)\n"
ABORTS = {
    "fold_null_folded": (FOLD % ("None", "S", "None", "P", 5, "X", 3),
                         "null argument to `bzamd_fold_polynomial`"),
    "fold_null_polynomial": (FOLD % ("F", "S", "None", "None", 5, "X", 3),
                             "null argument to `bzamd_fold_polynomial`"),
    "fold_null_point": (FOLD % ("F", "S", "None", "P", 5, "None", 3),
                        "null argument to `bzamd_fold_polynomial`"),
    "evaluate_null_evaluations": (EVAL % ("None", "P", "F", 5, 3, "X", 3),
                                  "null argument to `bzamd_evaluate_polynomials`"),
    "evaluate_null_points": (EVAL % ("O", "P", "F", 5, 3, "None", 3),
                             "null argument to `bzamd_evaluate_polynomials`"),
    "evaluate_null_folded": (EVAL % ("O", "P", "None", 5, 3, "X", 3),
                             "null argument to `bzamd_evaluate_polynomials`"),
    "quotients_null_quotients": (QUOT % ("None", "None", "P", "F", 5, 3, "Q", "X", 3),
                                 "null argument to `bzamd_batch_quotients`"),
    "quotients_null_q": (QUOT % ("O", "None", "P", "F", 5, 3, "None", "X", 3),
                         "null argument to `bzamd_batch_quotients`"),
    "fold_v_0": (FOLD % ("F", "S", "None", "P", 1, "X", 0), "needs 1 <= num_variables <= 30"),
    "fold_v_31": (FOLD % ("F", "S", "None", "P", 1, "X", 31), "needs 1 <= num_variables <= 30"),
    "evaluate_v_31": (EVAL % ("O", "P", "F", 1, 31, "X", 1), "needs 1 <= num_variables <= 30"),
    "quotients_v_0": (QUOT % ("O", "None", "P", "F", 1, 0, "Q", "X", 1),
                      "needs 1 <= num_variables <= 30"),
    "fold_n_0": (FOLD % ("F", "S", "None", "P", 0, "X", 3), "needs 1 <= n <= 2^num_variables"),
    "fold_n_above_2_pow_v": (FOLD % ("F", "S", "None", "P", 9, "X", 3),
                             "needs 1 <= n <= 2^num_variables"),
    "evaluate_n_above_2_pow_v": (EVAL % ("O", "P", "F", 5, 2, "X", 1),
                                 "needs 1 <= n <= 2^num_variables"),
    "quotients_n_0": (QUOT % ("O", "None", "P", "F", 0, 3, "Q", "X", 1),
                      "needs 1 <= n <= 2^num_variables"),
    "evaluate_no_points": (EVAL % ("O", "P", "F", 5, 3, "X", 0), "needs 1 <= num_points <= 4"),
    "evaluate_five_points": (EVAL % ("O", "P", "F", 5, 3, "X", 5), "needs 1 <= num_points <= 4"),
    "quotients_five_points": (QUOT % ("O", "None", "P", "F", 5, 3, "Q", "X", 5),
                              "needs 1 <= num_points <= 4"),
    "fold_misaligned_polynomial": (FOLD % ("F", "S", "None", "P + 4", 5, "X", 3),
                                   "must be 8-byte aligned"),
    "fold_misaligned_folded": (FOLD % ("F + 4", "S", "None", "P", 5, "X", 3),
                               "must be 8-byte aligned"),
    "fold_misaligned_scalars": (FOLD % ("F", "S + 4", "None", "P", 5, "X", 3),
                                "must be 8-byte aligned"),
    "quotients_misaligned_quotients": (QUOT % ("O + 4", "None", "P", "F", 5, 3, "Q", "X", 1),
                                       "must be 8-byte aligned"),
    "fold_folded_overlaps_polynomial": (FOLD % ("P + 64", "S", "None", "P", 5, "X", 3),
                                        "an output overlaps an input"),
    "fold_evaluation_overlaps_point": (FOLD % ("F", "S", "X + 40", "P", 5, "X", 3),
                                       "an output overlaps an input"),
    "evaluate_output_overlaps_folded": (EVAL % ("F + 32", "P", "F", 5, 3, "X", 1),
                                        "an output overlaps an input"),
    "quotients_overlap_polynomial": (QUOT % ("P + 32", "None", "P", "F", 5, 3, "Q", "X", 1),
                                     "an output overlaps an input"),
    "quotients_remainders_overlap_q": (QUOT % ("O", "Q", "P", "F", 5, 3, "Q", "X", 1),
                                       "an output overlaps an input"),
    "field_2": ("lib.bzamd_fold_polynomial(F, S, None, 2, P, 5, X, 3)\n", "unsupported field id"),
    "evaluate_field_2": ("lib.bzamd_evaluate_polynomials(O, 2, P, F, 5, 3, X, 1)\n",
                         "unsupported field id"),
    "fold_device_form_on_cpu": ("api.fold_polynomial_device(0, F, S, None, P, 5, X, 3)\n",
                                "device entry points need the GPU backend"),
    "evaluate_device_form_on_cpu": (
        "api.evaluate_polynomials_device(0, O, P, F, 5, 3, X, 1, W, 4096)\n",
        "device entry points need the GPU backend"),
    "quotients_device_form_on_cpu": (
        "api.batch_quotients_device(0, O, None, P, F, 5, 3, Q, X, 1, W, 4096)\n",
        "device entry points need the GPU backend"),
    "evaluate_workspace_too_small": (
        "size = api.evaluate_polynomials_workspace_bytes(0, 5, 3, 1)\n"
        "api.evaluate_polynomials_device(0, O, P, F, 5, 3, X, 1, W, size - 1)\n",
        "the polynomial evaluation workspace is too small"),
    "evaluate_null_workspace": (
        "api.evaluate_polynomials_device(0, O, P, F, 5, 3, X, 1, None, 4096)\n",
        "null argument to `bzamd_evaluate_polynomials_device`"),
    "quotients_workspace_too_small": (
        "size = api.batch_quotients_workspace_bytes(0, 5, 3, 1)\n"
        "api.batch_quotients_device(0, O, None, P, F, 5, 3, Q, X, 1, W, size - 1)\n",
        "the quotient workspace is too small"),
    "quotients_workspace_overlaps_polynomial": (
        "api.batch_quotients_device(0, O, None, P, F, 5, 3, Q, X, 1, P + 64, 4096)\n",
        "an output overlaps an input"),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_arguments_abort(name):
    call, message = ABORTS[name]
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            + SETUP + call)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


#--------------------------------------------------------------------------------------------------
# the kernels' resources
#--------------------------------------------------------------------------------------------------
def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


KERNELS = ("k_fold_levels", "k_evaluate_partials", "k_evaluate_finish", "k_quotient_sums",
           "k_quotient_carries", "k_quotients")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of proof/univariate_opening.hip with the flags the
    library is built with: every kernel of the file, both fields"""
    from blitzar_amd import build
    src = "proof/univariate_opening.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "univariate_opening.o")],
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
    assert len(scratch) == 2 * len(KERNELS), sorted(scratch)
    for kernel in KERNELS:
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == 2, f"{kernel}: found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found
