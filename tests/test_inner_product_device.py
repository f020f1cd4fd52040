"""The inner-product prover on device-resident vectors (include/blitzar_amd.h:
bzamd_inner_product_workspace_bytes, bzamd_prove_inner_product_device) against the reference's own
prover (oracle.ip_prove): L, R, the final scalar and the 203 bytes of the transcript after the
proof are byte-identical, for the built-in generators and for caller-supplied resident ones, for
proofs enqueued back to back on one stream, for unreduced input scalars, and from a caller's
transcript at every position of the sponge."""
import ctypes

import numpy as np
import pytest

from blitzar_amd import api
from tests import merlin_ref
from tests.golden.make_golden_inner_product import GOLDEN, golden_inputs
from tests.test_inner_product import scalars


def rounds_of(n):
    return max(int(n) - 1, 0).bit_length()


def padded(n):
    return 1 << rounds_of(n)


def test_workspace_bytes_need_no_backend():
    """a function of np = 2^ceil_log2(n) alone, callable before sxt_init"""
    size = api.inner_product_workspace_bytes
    assert size(0) == 0
    assert size((1 << 30) + 1) == 0
    assert size(513) == size(1000) == size(1024)
    assert size(1025) > size(1024) > size(512)
    for n in (1, 2, 3, 513, 1024, 1025, 1 << 20):
        np_ = padded(n)
        # a and b padded to np, np + 1 generators of 160 bytes
        assert size(n) >= 2 * 32 * np_ + 160 * (np_ + 1)


class DeviceProof:
    """operands of one bzamd_prove_inner_product_device call in torch tensors"""

    def __init__(self, n, offset, d_a, d_b, transcript, workspace=None, d_generators=None):
        import torch
        dev = d_a.device
        self.n, self.offset, self.d_a, self.d_b = n, offset, d_a, d_b
        rounds = rounds_of(n)
        self.l = torch.zeros((max(rounds, 1), 32), dtype=torch.uint8, device=dev)
        self.r = torch.zeros((max(rounds, 1), 32), dtype=torch.uint8, device=dev)
        self.ap = torch.zeros(32, dtype=torch.uint8, device=dev)
        if isinstance(transcript, np.ndarray):
            transcript = torch.from_numpy(transcript.copy()).to(dev)
        self.transcript = transcript  # a device tensor is used in place
        if workspace is None:
            workspace = torch.empty(api.inner_product_workspace_bytes(n), dtype=torch.uint8,
                                    device=dev)
        self.workspace = workspace
        self.d_generators = d_generators

    def enqueue(self, lib_api, stream):
        lib_api.prove_inner_product_device(
            self.n, self.offset, self.d_a.data_ptr(), self.d_b.data_ptr(), self.l.data_ptr(),
            self.r.data_ptr(), self.ap.data_ptr(), self.transcript.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel(),
            None if self.d_generators is None else self.d_generators.data_ptr(),
            stream=stream.cuda_stream)

    def results(self):
        rounds = rounds_of(self.n)
        return (self.l.cpu().numpy()[:rounds], self.r.cpu().numpy()[:rounds], self.ap.cpu().numpy(),
                self.transcript.cpu().numpy())


def assert_proof_equal(got, want):
    for name, g, w in zip(("L", "R", "ap", "transcript"), got, want):
        assert np.array_equal(g, w), f"{name} differs"


def prove_on_device(lib_api, n, offset, a, b, t0, d_generators=None):
    """-> (proof bytes, launches the call counted); checks that a and b are left alone"""
    import torch
    dev = torch.device("cuda", 0)
    d_a, d_b = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    proof = DeviceProof(n, offset, d_a, d_b, t0, d_generators=d_generators)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    launches = lib_api.load().bzamd_kernel_launch_count
    before = launches()
    proof.enqueue(lib_api, side)
    moved = launches() - before
    side.synchronize()
    assert np.array_equal(d_a.cpu().numpy(), a), "a_vector was modified"
    assert np.array_equal(d_b.cpu().numpy(), b), "b_vector was modified"
    return proof.results(), moved


DEVICE_FORM_CASES = [(1, 0), (2, 0), (3, 5), (5, 9), (64, 0), (100, 3), (257, 0), (1000, 17),
                     (4096, 0), (4097, 1)]
VERIFIED_CASES = [(5, 9), (1000, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", DEVICE_FORM_CASES)
def test_device_form(gpu_backend, oracle, n, offset):
    rng = np.random.default_rng(2400 + n)
    a, b = scalars(rng, n), scalars(rng, n)
    t0 = oracle.transcript_new("device form")
    want = oracle.ip_prove(t0, n, offset, a, b)
    got, moved = prove_on_device(gpu_backend, n, offset, a, b, t0)
    assert_proof_equal(got, want)
    if n > 1:
        assert moved > 0, "no kernel ran"
    if (n, offset) in VERIFIED_CASES:
        gens = oracle.ristretto_generators(n, offset)
        commit = oracle.msm_projective(0, [(a, False)], gens)[0]
        product = oracle.s25_inner_product(a, b)
        ok, t_after = gpu_backend.verify_inner_product(t0, n, offset, b, product, commit, *got[:3])
        assert ok and np.array_equal(t_after, got[3])


@pytest.mark.gpu
def test_unreduced_scalars(gpu_backend, oracle):
    """raw 256-bit inputs: the reference multiplies them as given"""
    n, offset = 37, 4
    rng = np.random.default_rng(2500)
    a, b = scalars(rng, n, reduced=False), scalars(rng, n, reduced=False)
    t0 = oracle.transcript_new("unreduced")
    got, _ = prove_on_device(gpu_backend, n, offset, a, b, t0)
    assert_proof_equal(got, oracle.ip_prove(t0, n, offset, a, b))


@pytest.mark.gpu
def test_callers_generators(gpu_backend, oracle):
    """np + 1 resident generators of the caller's, the last one Q; generators_offset is ignored"""
    import torch
    dev = torch.device("cuda", 0)
    n, offset = 300, 2
    np_ = padded(n)
    rng = np.random.default_rng(2600)
    a, b = scalars(rng, n), scalars(rng, n)
    t0 = oracle.transcript_new("caller's generators")
    d_generators = torch.empty((np_ + 1, 160), dtype=torch.uint8, device=dev)
    gpu_backend.load().bzamd_ristretto255_generators_device(
        ctypes.c_void_p(d_generators.data_ptr()), offset + 7, np_ + 1,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    generators = d_generators.cpu().numpy().copy()
    got, _ = prove_on_device(gpu_backend, n, 0, a, b, t0, d_generators=d_generators)
    assert_proof_equal(got, oracle.ip_prove(t0, n, offset + 7, a, b))
    assert np.array_equal(d_generators.cpu().numpy(), generators), "the generators were modified"


@pytest.mark.gpu
def test_back_to_back(gpu_backend, oracle):
    """three proofs enqueued on one stream with nothing between them but the final synchronise:
    the first two share one workspace, the third continues the first one's transcript where it
    lies on the device"""
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(1000, 3), (64, 0), (5, 11)]
    rng = np.random.default_rng(2700)
    inputs = [(scalars(rng, n), scalars(rng, n)) for n, _ in shapes]
    t0 = [oracle.transcript_new(f"proof {i}") for i in range(2)]
    shared = torch.empty(api.inner_product_workspace_bytes(1000), dtype=torch.uint8, device=dev)
    proofs = []
    for i, ((n, offset), (a, b)) in enumerate(zip(shapes, inputs)):
        d_a, d_b = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
        transcript = t0[i] if i < 2 else proofs[0].transcript
        proofs.append(DeviceProof(n, offset, d_a, d_b, transcript,
                                  workspace=shared if i < 2 else None))
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for proof in proofs:
        proof.enqueue(gpu_backend, side)
    side.synchronize()
    want = [oracle.ip_prove(t0[i], shapes[i][0], shapes[i][1], *inputs[i]) for i in range(2)]
    want.append(oracle.ip_prove(want[0][3], shapes[2][0], shapes[2][1], *inputs[2]))
    assert_proof_equal(proofs[1].results(), want[1])
    assert_proof_equal(proofs[2].results(), want[2])
    # the first proof's transcript went on into the third
    assert_proof_equal(proofs[0].results()[:3], want[0][:3])


def sponge_model(t0, n, l_values=None, r_values=None):
    """the instrumented Python transcript through a proof of n elements from t0; L and R (zeros when
    not given: which edges of the rate boundary are reached depends on lengths alone)"""
    t = merlin_ref.TracedTranscript(raw=t0)
    merlin_ref.inner_product_begin(t, n)
    for i in range(rounds_of(n)):
        merlin_ref.inner_product_round(t, bytes(32) if l_values is None else l_values[i].tobytes(),
                                       bytes(32) if r_values is None else r_values[i].tobytes())
    return t


def single_element_positions():
    """n = 1 is the transcript's init alone: the positions from which it fills the sponge, and two
    from which it does not"""
    starts = merlin_ref.padded_starts()
    return sorted({0, 108} | {pos for pos in range(merlin_ref.RATE) if sponge_model(starts[pos], 1).classes})


def test_sponge_sweep_reaches_every_boundary_class():
    """a caller who continues a transcript hands the prover any of the 166 positions: the smallest
    proof with a round (n = 2), from each, crosses the rate boundary in every way a 32-byte
    challenge can"""
    starts = merlin_ref.padded_starts()
    reached = set()
    for t0 in starts:
        reached |= sponge_model(t0, 2).classes
    assert reached == merlin_ref.BOUNDARY_CLASSES, sorted(merlin_ref.BOUNDARY_CLASSES - reached)
    assert {0, 108, 109, 164, 165} <= set(single_element_positions())


@pytest.mark.gpu
def test_device_form_at_every_sponge_position(gpu_backend, oracle):
    """n = 2 (k_round_challenge and one round) from every position, n = 1 (k_single_element) from the
    positions at which the init fills the sponge.  The transcript is compared with the Python model
    fed the device's own L and R first: a difference there is the sponge's, not the MSM's."""
    starts = merlin_ref.padded_starts()
    rng = np.random.default_rng(2800)
    reached = set()
    for n, positions in ((2, range(merlin_ref.RATE)), (1, single_element_positions())):
        for pos in positions:
            a, b = scalars(rng, n), scalars(rng, n)
            got, _ = prove_on_device(gpu_backend, n, 0, a, b, starts[pos])
            model = sponge_model(starts[pos], n, got[0], got[1])
            assert np.array_equal(got[3], model.array()), f"n = {n}, position {pos}: the transcript differs"
            for name, g, w in zip(("L", "R", "ap", "transcript"), got, oracle.ip_prove(starts[pos], n, 0, a, b)):
                assert np.array_equal(g, w), f"n = {n}, position {pos}: {name} differs"
            if n == 2:
                reached |= model.classes
    assert reached == merlin_ref.BOUNDARY_CLASSES


@pytest.mark.gpu
def test_many_partials_golden(gpu_backend):
    """n = 2^17 + 3: np = 2^18, mid = 2^17, so k_inner_product's grid-stride loop runs two
    iterations under its cap of 256 workgroups.  Expected bytes recorded once from oracle.ip_prove
    (the reference's prover takes minutes at this size)."""
    golden = np.load(GOLDEN)
    n, offset, seed = int(golden["n"]), int(golden["offset"]), int(golden["seed"])
    assert n == (1 << 17) + 3
    a, b = golden_inputs(n, seed)
    t0 = api.transcript_new(golden["label"].tobytes())
    got, _ = prove_on_device(gpu_backend, n, offset, a, b, t0)
    assert_proof_equal(got, (golden["l"], golden["r"], golden["ap"], golden["transcript"]))
