"""Sumcheck over typed columns with the library's own transcript (include/blitzar_amd.h:
bzamd_prove_sumcheck_transcript_columns, bzamd_sumcheck_transcript_columns_workspace_bytes,
bzamd_prove_sumcheck_transcript_device_columns).

The columns are those of tests/test_sumcheck_columns.py (widths 1, 2, 3, 4, 8, 16, 31 and 32, signed
and unsigned, lengths 0, 1, mid, mid + 1 and n, every other column at an odd address, extreme values
first).  The expected side is always the reference's prover with the Python Merlin of
tests/merlin_ref.py on the columns widened to 32 bytes and padded with zero rows
(tests/test_sumcheck_transcript.py reference_proof): round polynomials, evaluation point and the
203 bytes of the transcript after the proof byte for byte, mle_evaluations against the fold written
in Python integers."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.test_sumcheck import elements, product_table
from tests.test_sumcheck_columns import Case
from tests.test_sumcheck_device import MODULUS, folded_evaluations, to_bytes
from tests.test_sumcheck_transcript import (SWEEP_PRODUCTS, expected_evaluations, reference_proof,
                                            sweep_fields, sweep_model, variables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL_ROWS = 256     # kTailRows of proof/sumcheck_transcript.hip
FIXED_DEGREE = 5    # kFixedDegree of proof/sumcheck_rows.h


def want_of(oracle, case, t0):
    return reference_proof(oracle, case.field_id, case.widened, case.table, case.terms, case.n,
                           case.degree, t0)


def check_proof(case, got, want, with_evaluations=True):
    polys, point, evaluations, t = got
    assert np.array_equal(polys, want[0]), "round polynomials differ"
    assert np.array_equal(point, want[1]), "evaluation points differ"
    assert np.array_equal(t, want[2]), "transcripts differ"
    if with_evaluations:
        assert np.array_equal(evaluations, folded_evaluations(case.field_id, case.widened, point))
    else:
        assert evaluations is None


def host_call(lib_api, case, t0, with_evaluations=True):
    return lib_api.prove_sumcheck_transcript_columns(
        case.field_id, case.host_columns(), case.table, case.terms, case.n, case.degree, t0,
        with_evaluations=with_evaluations)


#--------------------------------------------------------------------------------------------------
# host backend
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("degree", [1, 3, 5, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 41])
def test_host_form_matches_reference(cpu_backend, oracle, field_id, degree, n):
    case = Case(field_id, n, degree, 3000 + 10 * n + degree)
    flat = case.flat.copy()
    t0 = merlin_ref.Transcript(label="host columns").array()
    want = want_of(oracle, case, t0)
    check_proof(case, host_call(cpu_backend, case, t0), want)
    check_proof(case, host_call(cpu_backend, case, t0, with_evaluations=False), want, False)
    assert np.array_equal(case.flat, flat), "the columns were modified"


@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n", [1, 5, 41])
def test_full_width_columns_equal_the_matrix_form(cpu_backend, field_id, n):
    """all columns 32 bytes and full length: bzamd_prove_sumcheck_transcript byte for byte"""
    case = Case(field_id, n, 3, 3100 + n, mles=[(32, False, "n")] * 12)
    t0 = merlin_ref.Transcript(label="full width").array()
    want = cpu_backend.prove_sumcheck_transcript(field_id, case.widened, case.table, case.terms, n,
                                                 3, t0)
    got = host_call(cpu_backend, case, t0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(got[2], expected_evaluations(cpu_backend, field_id, case.widened,
                                                       case.table, case.terms, n, 3, got[1]))


@pytest.mark.parametrize("field_id", [0, 1])
def test_workspace_bytes_need_no_backend(field_id):
    """a function of the field and the counts alone (no widths, no pointers: the wrapper passes
    none).  At 2^15 rows the tables are two of 36-byte elements at 1/2 and 1/4 of the padded rows,
    27 bytes per row and MLE; the fixed part is the partials (1024 workgroups x 9 coefficients x 36
    bytes = 331 776) and seven blocks padded to 256 bytes"""
    api.reset_for_testing()
    assert api.load().bzamd_active_backend() == 0
    size = api.sumcheck_transcript_columns_workspace_bytes
    at = [size(field_id, n, 12, 5, 13, 3) for n in (512, 513, 1027)]
    print(at)
    assert at[0] <= at[1] <= at[2] and at[0] < at[2]
    n = 1 << 15
    ours = size(field_id, n, 12, 5, 13, 3)
    theirs = api.sumcheck_transcript_workspace_bytes(field_id, n, 12, 5, 13, 3)
    print(ours, theirs, ours / theirs)
    assert ours <= 27 * n * 12 + 512 * 1024
    assert ours < 0.6 * theirs
    # degrees above the fixed ones have no tail-only form: the same two tables at every n
    assert size(field_id, 300, 12, 4, 12, 6) <= 36 * (256 + 128) * 12 + 512 * 1024
    assert api.load().bzamd_active_backend() == 0


ABORTS = {
    "null_transcript": ("c, t0 = [np.ones((2, 8), np.uint8)], None\n",
                        "null argument to `bzamd_prove_sumcheck_transcript_columns`"),
    "longer_than_n": ("c = [np.ones((3, 8), np.uint8)]\n", "a sumcheck column is longer than n"),
    "width_0": ("c = [np.ones((2, 0), np.uint8)]\n", "element_nbytes must be in [1, 32]"),
    "width_33": ("c = [np.ones((2, 33), np.uint8)]\n", "element_nbytes must be in [1, 32]"),
    "signed_17": ("c = [(np.ones((2, 17), np.uint8), True)]\n",
                  "signed sequences need element_nbytes <= 16"),
    "device_form_on_cpu": ("c = None\n", "device entry points need the GPU backend"),
}


@pytest.mark.parametrize("name", sorted(ABORTS))
def test_bad_arguments_abort(name):
    setup, message = ABORTS[name]
    code = ("import numpy as np\nfrom blitzar_amd import api\napi.init(api.SXT_CPU_BACKEND, 0)\n"
            "t = np.zeros((1, 36), np.uint8)\nt[0, 0] = 1\nt[0, 32] = 1\n"
            "t0 = np.zeros(203, np.uint8)\n" + setup +
            "if c is None:\n"
            "    m, out = np.ones((2, 8), np.uint8), np.zeros(4096, np.uint8)\n"
            "    p = out.ctypes.data\n"
            "    api.prove_sumcheck_transcript_device_columns(\n"
            "        0, [(m.ctypes.data, 2, 8, False)], t, [0], 2, 1, p, p, None, p, p, out.size)\n"
            "else:\n"
            "    api.prove_sumcheck_transcript_columns(0, c, t, [0], 2, 1, t0)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode < 0 and message in r.stderr, r.stderr


def _hipcc():
    from blitzar_amd import build
    return build.HIPCC if os.path.exists(build.HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")
def test_column_chain_kernels_use_no_scratch(tmp_path):
    """the compiler's own resource report of the translation unit that holds the chain, with the
    flags the library is built with: the column load, the column fold from the slot and the flagged
    challenge kernel, both fields.  Round 0 over typed columns is not compiled here a second time:
    proof/sumcheck_columns.hip owns those kernels (test_sumcheck_columns.py checks them there)"""
    from blitzar_amd import build
    src = "proof/sumcheck_transcript.hip"
    assert src in build.SOURCES
    r = subprocess.run([_hipcc(), *build.FLAGS, *build.TU_FLAGS.get(src, []), "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(build.CSRC, src), "-o", str(tmp_path / "transcript.o")],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None:
            scratch[name] = int(m.group(1))
    print({k: v for k, v in scratch.items() if "k_sumcheck_columns" in k})
    for kernel, count in (("k_sumcheck_columns_fold_slot", 2), ("k_sumcheck_columns_load", 2),
                          ("k_sumcheck_columns_challenge", 2), ("k_sumcheck_columns_round", 0),
                          ("k_sumcheck_columns_generic", 0)):
        found = {k: v for k, v in scratch.items() if kernel in k}
        assert len(found) == count, f"{kernel}: expected {count}, found {sorted(found)}"
        assert all(v == 0 for v in found.values()), found


#--------------------------------------------------------------------------------------------------
# GPU
#--------------------------------------------------------------------------------------------------
def expected_launches(n, degree, with_evaluations):
    """the column load and the tail; or three per round before the tail (round
    0 on the columns) and the tail; round degrees above 5 have no tail and no last fold without
    mle_evaluations"""
    v = variables(n)
    if degree <= FIXED_DEGREE:
        if n <= 2 * TAIL_ROWS:
            return 2
        return 3 * (v - 1 - (TAIL_ROWS.bit_length() - 1)) + 1
    return 3 * v - (0 if with_evaluations else 1)


def _launches():
    return api.load().bzamd_kernel_launch_count()


class DeviceColumnsProof:
    """operands of one bzamd_prove_sumcheck_transcript_device_columns call in torch tensors"""

    def __init__(self, case, d_flat, transcript, with_evaluations=True, workspace=None,
                 workspace_offset=0):
        import torch
        dev = d_flat.device
        v = variables(case.n)
        self.case, self.d_flat = case, d_flat
        self.polys = torch.zeros((v, case.degree + 1, 32), dtype=torch.uint8, device=dev)
        self.point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
        self.evaluations = (torch.zeros((len(case.specs), 32), dtype=torch.uint8, device=dev)
                            if with_evaluations else None)
        if isinstance(transcript, np.ndarray):
            transcript = torch.from_numpy(transcript.copy()).to(dev)
        self.transcript = transcript  # a device tensor is used in place
        self.workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(
            case.field_id, case.n, len(case.specs), len(case.products), len(case.terms), case.degree)
        if workspace is None:
            workspace = torch.empty(self.workspace_bytes + workspace_offset, dtype=torch.uint8,
                                    device=dev)
        assert workspace.numel() >= self.workspace_bytes + workspace_offset
        self.workspace, self.workspace_offset = workspace, workspace_offset

    def enqueue(self, lib_api, stream):
        case = self.case
        lib_api.prove_sumcheck_transcript_device_columns(
            case.field_id, case.device_descriptors(self.d_flat.data_ptr()), case.table, case.terms,
            case.n, case.degree, self.polys.data_ptr(), self.point.data_ptr(),
            None if self.evaluations is None else self.evaluations.data_ptr(),
            self.transcript.data_ptr(), self.workspace.data_ptr() + self.workspace_offset,
            self.workspace_bytes, stream=stream.cuda_stream)

    def results(self):
        return (self.polys.cpu().numpy(), self.point.cpu().numpy(),
                None if self.evaluations is None else self.evaluations.cpu().numpy(),
                self.transcript.cpu().numpy())


DEVICE_FORM_CASES = (
    # the column load and the tail; 512 is the last size on that path
    [(n, 3) for n in (1, 2, 5, 41, 300, 512)]
    # one column round, then the tail; a column round, one dense chain round (both ping-pong tables
    # in use), then the tail; 128 workgroups' partials in the column round
    + [(513, 3), (1027, 3), ((1 << 14) + 77, 3)]
    # the other instantiations of the column round at the threshold
    + [(513, 1), (513, 5)]
    # round 0 is the last round: the column fold writes the evaluations or is skipped; the generic
    # chain to the end
    + [(2, 6), (41, 6), (513, 6)])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("case_index", range(len(DEVICE_FORM_CASES)))
def test_device_form(gpu_backend, oracle, field_id, case_index):
    import torch
    dev = torch.device("cuda", 0)
    n, degree = DEVICE_FORM_CASES[case_index]
    case = Case(field_id, n, degree, 3200 + case_index)
    t0 = merlin_ref.Transcript(label="device columns").array()
    want = want_of(oracle, case, t0)
    d_flat = torch.from_numpy(case.flat.copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    for with_evaluations in (True, False):
        proof = DeviceColumnsProof(case, d_flat, t0, with_evaluations)
        torch.cuda.synchronize()
        before = _launches()
        proof.enqueue(gpu_backend, side)
        assert _launches() - before == expected_launches(n, degree, with_evaluations)
        side.synchronize()
        check_proof(case, proof.results(), want, with_evaluations)
    # the columns, the gaps between them and the guard bytes around them are only read
    assert np.array_equal(d_flat.cpu().numpy(), case.flat), "device memory was modified"


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,degree", [(300, 3), (1027, 3), (41, 6)])
def test_workspace_at_any_alignment(gpu_backend, oracle, field_id, n, degree):
    """a workspace one byte past a 256-byte boundary: the layout aligns itself"""
    import torch
    dev = torch.device("cuda", 0)
    case = Case(field_id, n, degree, 3300 + degree)
    t0 = merlin_ref.Transcript(label="odd workspace").array()
    d_flat = torch.from_numpy(case.flat.copy()).to(dev)
    size = api.sumcheck_transcript_columns_workspace_bytes(field_id, n, len(case.specs),
                                                           len(case.products), len(case.terms), degree)
    workspace = torch.empty(size + 256, dtype=torch.uint8, device=dev)
    offset = (257 - workspace.data_ptr() % 256) % 256
    proof = DeviceColumnsProof(case, d_flat, t0, workspace=workspace, workspace_offset=offset)
    assert (proof.workspace.data_ptr() + proof.workspace_offset) % 256 == 1
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    proof.enqueue(gpu_backend, side)
    side.synchronize()
    check_proof(case, proof.results(), want_of(oracle, case, t0))


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
def test_device_form_back_to_back(gpu_backend, oracle, field_id):
    """two proofs of different shape enqueued on one stream with nothing between them but the final
    synchronise, a third that continues the first one's transcript where it lies, each with its
    own workspace, and a fourth that reuses the first workspace behind the others"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [Case(field_id, 1027, 3, 3400), Case(field_id, 300, 5, 3401),
             Case(field_id, 513, 6, 3402), Case(field_id, 600, 1, 3403)]
    t0 = [merlin_ref.Transcript(label=f"proof {i}").array() for i in (0, 1, 3)]
    d_flat = [torch.from_numpy(c.flat.copy()).to(dev) for c in cases]
    proofs = [DeviceColumnsProof(cases[0], d_flat[0], t0[0]),
              DeviceColumnsProof(cases[1], d_flat[1], t0[1])]
    proofs.append(DeviceColumnsProof(cases[2], d_flat[2], proofs[0].transcript))
    proofs.append(DeviceColumnsProof(cases[3], d_flat[3], t0[2], workspace=proofs[0].workspace))
    assert proofs[3].workspace_bytes <= proofs[0].workspace_bytes
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for proof in proofs:
        proof.enqueue(gpu_backend, side)
    side.synchronize()
    first = want_of(oracle, cases[0], t0[0])
    want = [first, want_of(oracle, cases[1], t0[1]), want_of(oracle, cases[2], first[2]),
            want_of(oracle, cases[3], t0[2])]
    for i in (1, 2, 3):
        check_proof(cases[i], proofs[i].results(), want[i])
    polys, point, evaluations, _ = proofs[0].results()  # its transcript went on into the third
    assert np.array_equal(polys, want[0][0]) and np.array_equal(point, want[0][1])
    assert np.array_equal(evaluations, folded_evaluations(field_id, cases[0].widened, point))


@pytest.mark.gpu
def test_commit_then_prove_over_one_descriptor_array(gpu_backend, oracle):
    """8-byte signed, 1-byte and 32-byte columns on the device: the same descriptor array goes to
    bzamd_msm_device and then to the prover, on one stream with one synchronise"""
    import torch
    lib, dev, field_id, n = api.load(), torch.device("cuda", 0), 0, 1000
    rng = np.random.default_rng(3500)
    p = MODULUS[field_id]
    cols = [(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64).view(np.uint8).reshape(n, 8), True),
            (rng.integers(0, 256, (n - 300, 1), dtype=np.uint8), False),
            (elements(rng, field_id, n - 1), False)]
    gens = oracle.ristretto_generators(n)
    want_commitments = oracle.commit(0, cols, gens)
    widened = np.zeros((len(cols), n, 32), np.uint8)
    for j, (c, signed) in enumerate(cols):
        for i in range(len(c)):
            v = int.from_bytes(c[i].tobytes(), "little", signed=signed)
            widened[j, i] = c[i] if c.shape[1] == 32 else to_bytes(field_id, v % p)
    products = [[0, 1, 2], [2, 2], [0]]
    table = product_table(field_id, elements(rng, field_id, 3), [3, 2, 1],
                          api.SUMCHECK_PRODUCT_STRIDE[field_id])
    terms = [i for t in products for i in t]
    t0 = merlin_ref.Transcript(label="commit then prove").array()
    want = reference_proof(oracle, field_id, widened, table, terms, n, 3, t0)

    side = torch.cuda.Stream(device=dev)
    stream = ctypes.c_void_p(side.cuda_stream)
    keep = [torch.from_numpy(c.copy()).to(dev) for c, _ in cols]
    desc = (api.sxt_sequence_descriptor * len(cols))()
    for i, (c, signed) in enumerate(cols):
        desc[i] = api.sxt_sequence_descriptor(c.shape[1], len(c), keep[i].data_ptr(), int(signed))
    d_gens = torch.from_numpy(gens.copy()).to(dev)
    out = torch.zeros((len(cols), 32), dtype=torch.uint8, device=dev)
    v = variables(n)
    polys = torch.zeros((v, 4, 32), dtype=torch.uint8, device=dev)
    point = torch.zeros((v, 32), dtype=torch.uint8, device=dev)
    transcript = torch.from_numpy(t0.copy()).to(dev)
    workspace_bytes = api.sumcheck_transcript_columns_workspace_bytes(field_id, n, len(cols), 3,
                                                                      len(terms), 3)
    workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    lib.bzamd_msm_device(0, ctypes.c_void_p(out.data_ptr()), len(cols), desc,
                         ctypes.c_void_p(d_gens.data_ptr()), stream)
    # the same array, with no synchronise in between
    before = _launches()
    gpu_backend.prove_sumcheck_transcript_device_columns(
        field_id, desc, table, terms, n, 3, polys.data_ptr(), point.data_ptr(), None,
        transcript.data_ptr(), workspace.data_ptr(), workspace_bytes, stream=side.cuda_stream)
    assert _launches() - before == expected_launches(n, 3, False)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want_commitments)
    assert np.array_equal(polys.cpu().numpy(), want[0])
    assert np.array_equal(point.cpu().numpy(), want[1])
    assert np.array_equal(transcript.cpu().numpy(), want[2])


@pytest.mark.gpu
@pytest.mark.parametrize("field_id", [0, 1])
@pytest.mark.parametrize("n,degree", [(3, 3), (41, 6), (2300, 5)])
def test_host_form_on_gpu_equals_device_form(gpu_backend, oracle, field_id, n, degree):
    import torch
    dev = torch.device("cuda", 0)
    case = Case(field_id, n, degree, 3600 + degree)
    t0 = merlin_ref.Transcript(label="host form on the gpu").array()
    flat = case.flat.copy()
    before = _launches()
    host = host_call(gpu_backend, case, t0)
    assert _launches() > before, "no kernel ran"
    assert api.load().bzamd_sumcheck_device_bytes() > 0
    assert np.array_equal(case.flat, flat), "the columns were modified"
    proof = DeviceColumnsProof(case, torch.from_numpy(case.flat.copy()).to(dev), t0)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    proof.enqueue(gpu_backend, side)
    side.synchronize()
    for h, d in zip(host, proof.results()):
        assert np.array_equal(h, d)
    check_proof(case, host, want_of(oracle, case, t0))
    without = host_call(gpu_backend, case, t0, with_evaluations=False)
    assert without[2] is None
    for k in (0, 1, 3):
        assert np.array_equal(without[k], host[k])


class SweepCase:
    """n = 2, one 8-byte signed column, one product (SWEEP_PRODUCTS): round degree 1 is the column
    load and k_sumcheck_tail, 6 the column round, k_sumcheck_columns_challenge and
    k_sumcheck_columns_fold_slot writing the evaluations"""

    def __init__(self, field_id, degree):
        rng = np.random.default_rng(3700 + degree + field_id)
        self.field_id, self.n, self.degree = field_id, 2, degree
        self.products = SWEEP_PRODUCTS[degree]
        values = np.array([-(1 << 63) + 5 + field_id, (1 << 62) + 3], np.int64)
        self.flat = np.full(64 + 16 + 64, 0xA5, np.uint8)
        self.flat[64:80] = values.view(np.uint8)
        self.specs = [(64, 2, 8, True)]
        self.widened = np.zeros((1, 2, 32), np.uint8)
        for i, v in enumerate(values):
            self.widened[0, i] = to_bytes(field_id, int(v) % MODULUS[field_id])
        self.terms = [i for t in self.products for i in t]
        self.table = product_table(field_id, elements(rng, field_id, 1), [len(self.products[0])],
                                   api.SUMCHECK_PRODUCT_STRIDE[field_id])

    def device_descriptors(self, base_ptr):
        return [(base_ptr + o, rows, w, signed) for o, rows, w, signed in self.specs]


@pytest.mark.gpu
@pytest.mark.parametrize("degree", sorted(SWEEP_PRODUCTS))
def test_device_form_at_every_sponge_position(gpu_backend, oracle, degree):
    """a caller who continues a transcript hands the prover any position of the sponge: the
    starting-transcript sweep of tests/test_sumcheck_transcript.py through the columns form, which
    puts k_sumcheck_columns_challenge at every rate boundary"""
    import torch
    dev = torch.device("cuda", 0)
    cases = [SweepCase(field_id, degree) for field_id in (0, 1)]
    d_flat = [torch.from_numpy(c.flat.copy()).to(dev) for c in cases]
    side = torch.cuda.Stream(device=dev)
    reached = set()
    for pos, t0 in enumerate(merlin_ref.padded_starts()):
        for field_id in sweep_fields(pos):
            case = cases[field_id]
            proof = DeviceColumnsProof(case, d_flat[field_id], t0)
            proof.enqueue(gpu_backend, side)
            side.synchronize()
            polys, point, evaluations, t = proof.results()
            where = f"position {pos}, field {field_id}"
            # the Python model fed the device's own polynomial first: a difference there is the sponge's
            model, r = sweep_model(t0, field_id, degree, polys[0].tobytes())
            assert np.array_equal(t, model.array()), f"{where}: the transcript differs from the model"
            assert point[0].tobytes() == r, f"{where}: the challenge differs from the model"
            reached |= model.classes
            want = want_of(oracle, case, t0)
            assert np.array_equal(polys, want[0]), f"{where}: round polynomials differ"
            assert np.array_equal(point, want[1]), f"{where}: evaluation points differ"
            assert np.array_equal(t, want[2]), f"{where}: transcripts differ"
            assert np.array_equal(evaluations, folded_evaluations(field_id, case.widened, point)), where
    assert reached == merlin_ref.BOUNDARY_CLASSES
    for c, d in zip(cases, d_flat):
        assert np.array_equal(d.cpu().numpy(), c.flat), "device memory was modified"
