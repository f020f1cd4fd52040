"""The inner-product verifier on device-resident proofs (include/blitzar_amd.h:
bzamd_inner_product_verify_workspace_bytes, bzamd_verify_inner_product_device) against the
reference's own verifier (oracle.ip_verify): the verdict word and the 203 bytes of the transcript
after the call, for accepted and tampered proofs, undecodable L / R points, unreduced scalars, a
misaligned b, caller-supplied resident generators, calls enqueued back to back behind the device
prover, and from a caller's transcript at every position of the sponge.  Every expected value
comes from the oracle (or the committed golden); the verdict word holds the opposite before every
call."""
import ctypes

import numpy as np
import pytest

from blitzar_amd import api
from tests import hooks, merlin_ref
from tests.golden.make_golden_inner_product import GOLDEN, golden_inputs
from tests.test_inner_product import L_ORDER, scalars
from tests.test_inner_product_device import DeviceProof, padded, rounds_of, sponge_model

P_FIELD = 2**255 - 19
SIZES = (1, 2, 3, 513, 1024, 1025, 1 << 20)  # what the prover's workspace test lists


def test_verify_workspace_bytes_need_no_backend():
    """a function of np = 2^ceil_log2(n) alone, callable before sxt_init"""
    size = api.inner_product_verify_workspace_bytes
    assert size(0) == 0
    assert size((1 << 30) + 1) == 0
    assert size(513) == size(1000) == size(1024)
    assert size(1025) > size(1024) > size(512)
    for n in SIZES:
        np_, rounds = padded(n), rounds_of(n)
        # b, the generator array [a_commit | Q | g | L | R], the exponents over [Q | g | L | R]
        assert size(n) >= (32 * n + 160 * (np_ + 2 * rounds + 2) + 32 * (np_ + 2 * rounds + 1))


class Statement:
    """what a verifier is handed, on the host: (t0, n, offset, b, product, commit, l, r, ap)"""

    def __init__(self, oracle, n, offset, seed, label="verify on device", reduced=True, t0=None):
        rng = np.random.default_rng(seed)
        self.n, self.offset = n, offset
        a, self.b = scalars(rng, n, reduced), scalars(rng, n, reduced)
        self.t0 = oracle.transcript_new(label) if t0 is None else t0
        self.l, self.r, self.ap, _ = oracle.ip_prove(self.t0, n, offset, a, self.b)
        gens = oracle.ristretto_generators(n, offset)
        self.commit = oracle.msm_projective(0, [(a, False)], gens)[0]
        self.product = oracle.s25_inner_product(a, self.b)

    def copy(self, **changed):
        other = object.__new__(Statement)
        other.__dict__.update(self.__dict__)
        other.__dict__.update(changed)
        return other

    def expected(self, oracle):
        """-> (verdict, transcript after) of the reference's verifier"""
        return oracle.ip_verify(self.t0, self.n, self.offset, self.b, self.product, self.commit,
                                self.l, self.r, self.ap)


class DeviceVerify:
    """operands of one bzamd_verify_inner_product_device call in torch tensors; `resident`: tensors
    that are used where they lie instead of an upload (transcript, l, r, ap, b, workspace)"""

    def __init__(self, st, expected_verdict, offset=None, d_generators=None, misalign_b=False,
                 **resident):
        import torch
        dev = torch.device("cuda", 0)

        def up(name, array, dtype=np.uint8):
            if name in resident:
                return resident[name]
            return torch.from_numpy(np.ascontiguousarray(array).view(dtype).copy()).to(dev)

        self.n = st.n
        self.offset = st.offset if offset is None else offset
        self.rounds = rounds_of(st.n)
        self.host = {"b": st.b, "product": st.product, "commit": np.asarray(st.commit).view(np.uint8),
                     "l": st.l, "r": st.r, "ap": st.ap}
        if misalign_b:
            buffer = torch.zeros(32 * st.n + 8, dtype=torch.uint8, device=dev)
            buffer[1:1 + 32 * st.n] = torch.from_numpy(st.b.reshape(-1).copy()).to(dev)
            self.b = buffer[1:1 + 32 * st.n]
            assert self.b.data_ptr() % 8 == 1
        else:
            self.b = up("b", st.b)
        self.product, self.ap = up("product", st.product), up("ap", st.ap)
        self.commit = up("commit", np.asarray(st.commit).view(np.uint8))
        pad = np.zeros((1, 32), np.uint8)
        self.l = up("l", st.l if self.rounds else pad)
        self.r = up("r", st.r if self.rounds else pad)
        self.transcript = up("transcript", st.t0)
        # the opposite of what is expected
        self.verdict = torch.full((1,), 0 if expected_verdict else 1, dtype=torch.int32, device=dev)
        self.workspace = resident.get("workspace")
        if self.workspace is None:
            self.workspace = torch.empty(api.inner_product_verify_workspace_bytes(st.n),
                                         dtype=torch.uint8, device=dev)
        self.d_generators = d_generators

    def enqueue(self, lib_api, stream):
        lib_api.verify_inner_product_device(
            self.n, self.offset, self.b.data_ptr(), self.product.data_ptr(), self.commit.data_ptr(),
            self.l.data_ptr(), self.r.data_ptr(), self.ap.data_ptr(), self.transcript.data_ptr(),
            self.verdict.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
            None if self.d_generators is None else self.d_generators.data_ptr(),
            stream=stream.cuda_stream)

    def results(self):
        return int(self.verdict.cpu().numpy()[0]), self.transcript.cpu().numpy()

    def assert_inputs_unchanged(self):
        for name in ("b", "product", "commit", "ap"):
            got = getattr(self, name).cpu().numpy().reshape(-1)
            assert np.array_equal(got, self.host[name].reshape(-1)), f"{name} was modified"
        if self.rounds:
            assert np.array_equal(self.l.cpu().numpy()[:self.rounds], self.host["l"]), "L was modified"
            assert np.array_equal(self.r.cpu().numpy()[:self.rounds], self.host["r"]), "R was modified"


def verify_on_device(lib_api, oracle, st, **how):
    """one call on a side stream, checked against the oracle -> (verdict, launches counted)"""
    import torch
    want_ok, want_t = st.expected(oracle)
    call = DeviceVerify(st, want_ok, **how)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    launches = lib_api.load().bzamd_kernel_launch_count
    before = launches()
    call.enqueue(lib_api, side)
    moved = launches() - before
    side.synchronize()
    verdict, t_after = call.results()
    assert verdict == int(want_ok), f"verdict {verdict}, the reference says {want_ok}"
    assert np.array_equal(t_after, want_t), "the transcript differs from the reference's"
    call.assert_inputs_unchanged()
    return verdict, moved


ACCEPTED_CASES = [(1, 0), (2, 0), (3, 5), (5, 9), (64, 0), (100, 3), (257, 0), (1000, 17),
                  (4096, 0), (4097, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", ACCEPTED_CASES)
def test_accepted(gpu_backend, oracle, n, offset):
    st = Statement(oracle, n, offset, 3400 + n)
    verdict, moved = verify_on_device(gpu_backend, oracle, st)
    assert verdict == 1
    assert moved > 0, "no kernel ran"


def tampered(oracle, st):
    """-> [(name, statement, how)]: each one the reference rejects"""
    def flipped(x, at=0, bit=1):
        y = x.copy()
        y.reshape(-1)[at] ^= bit
        return y

    b_last = st.b.copy()
    b_last[st.n - 1, 0] ^= 1
    cases = [("ap bit", st.copy(ap=flipped(st.ap)), {}),
             ("product bit", st.copy(product=flipped(st.product, 3, 0x10)), {}),
             ("last b entry", st.copy(b=b_last), {}),
             ("a_commit is another generator",
              st.copy(commit=oracle.ristretto_generators(1, st.offset + 1)[0]), {}),
             ("another transcript label", st.copy(t0=oracle.transcript_new("another label")), {}),
             ("another offset", st.copy(offset=st.offset + 1), {})]
    if st.n > 1:
        l_bad = st.l.copy()
        l_bad[-1] = st.r[-1]
        r_bad = st.r.copy()
        r_bad[0] = oracle.commit(0, [(np.array([7], np.uint8), False)],
                                 oracle.ristretto_generators(1, 12345))[0]
        assert not np.array_equal(r_bad[0], st.r[0])
        cases += [("last L replaced by last R", st.copy(l=l_bad), {}),
                  ("first R replaced by a valid point", st.copy(r=r_bad), {})]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset", [(1, 2), (5, 9), (1000, 17)])
def test_rejected(gpu_backend, oracle, n, offset):
    """(n = 1 has no round and so no challenge: there the label changes the transcript alone, and
    the verdict is the reference's, as everywhere)"""
    st = Statement(oracle, n, offset, 3500 + n)
    for name, bad, how in tampered(oracle, st):
        verdict, _ = verify_on_device(gpu_backend, oracle, bad, **how)
        if n > 1 or name != "another transcript label":
            assert verdict == 0, name


def host_rejects(s_value):
    try:
        hooks.ristretto_decode(np.frombuffer(s_value.to_bytes(32, "little"), np.uint8))
    except AssertionError:
        return True
    return False


def undecodable_encodings():
    """-> [(name, 32 bytes)]; the last three: the first even s the host decoder rejects for not
    being a square or for a negative t"""
    found = [s for s in range(2, 2 + 2 * 64, 2) if host_rejects(s)][:3]
    assert len(found) == 3, "fewer than three rejected even s among the first 64 candidates"
    named = [("p", P_FIELD), ("p + 1", P_FIELD + 1), ("1", 1), ("p - 1", P_FIELD - 1)]
    named += [(f"s = {s}", s) for s in found]
    return [(name, np.frombuffer(v.to_bytes(32, "little"), np.uint8)) for name, v in named]


@pytest.mark.gpu
def test_undecodable_points(gpu_backend, oracle):
    """an L or R that is no canonical encoding: verdict 0, the reference's transcript, no fault,
    and the chain is fit for the next call on the same stream"""
    import torch
    n, offset = 5, 9
    st = Statement(oracle, n, offset, 3600)
    rounds = rounds_of(n)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    workspace = torch.empty(api.inner_product_verify_workspace_bytes(n), dtype=torch.uint8,
                            device=torch.device("cuda", 0))
    good_ok, good_t = st.expected(oracle)
    assert good_ok
    case = 0
    for name, encoding in undecodable_encodings():
        for which in ("l", "r"):
            points = getattr(st, which).copy()
            points[case % rounds] = encoding
            case += 1
            bad = st.copy(**{which: points})
            want_ok, want_t = bad.expected(oracle)
            assert not want_ok
            first = DeviceVerify(bad, want_ok, workspace=workspace)
            second = DeviceVerify(st, good_ok, workspace=workspace)
            torch.cuda.synchronize()
            first.enqueue(gpu_backend, side)
            second.enqueue(gpu_backend, side)
            side.synchronize()
            verdict, t_after = first.results()
            assert verdict == 0, f"{which} = {name}"
            assert np.array_equal(t_after, want_t), f"{which} = {name}: the transcript differs"
            verdict, t_after = second.results()
            assert verdict == 1, f"the untampered proof after {which} = {name}"
            assert np.array_equal(t_after, good_t)


@pytest.mark.gpu
def test_unreduced_scalars(gpu_backend, oracle):
    """raw 256-bit b, product and ap are taken as given"""
    n, offset = 37, 4
    st = Statement(oracle, n, offset, 3700, reduced=False)
    verify_on_device(gpu_backend, oracle, st)
    raw = np.random.default_rng(3701).integers(0, 256, (2, 32), dtype=np.uint8)
    raw[:, 31] |= 0xf0
    ap_value = int.from_bytes(st.ap.tobytes(), "little")
    lifted = np.frombuffer((ap_value + L_ORDER).to_bytes(32, "little"), np.uint8)
    for bad in (st.copy(ap=lifted), st.copy(ap=raw[0]), st.copy(product=raw[1])):
        verify_on_device(gpu_backend, oracle, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 300])
def test_misaligned_b(gpu_backend, oracle, n):
    st = Statement(oracle, n, 2, 3800 + n)
    verdict, _ = verify_on_device(gpu_backend, oracle, st, misalign_b=True)
    assert verdict == 1
    b_last = st.b.copy()
    b_last[n - 1, 0] ^= 1
    verdict, _ = verify_on_device(gpu_backend, oracle, st.copy(b=b_last), misalign_b=True)
    assert verdict == 0


@pytest.mark.gpu
def test_callers_generators(gpu_backend, oracle):
    """np + 1 resident generators of the caller's, the last one Q; generators_offset is ignored"""
    import torch
    dev = torch.device("cuda", 0)
    n, offset = 300, 9
    np_ = padded(n)
    st = Statement(oracle, n, offset, 3900)
    d_generators = torch.empty((np_ + 1, 160), dtype=torch.uint8, device=dev)
    gpu_backend.load().bzamd_ristretto255_generators_device(
        ctypes.c_void_p(d_generators.data_ptr()), offset, np_ + 1,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    generators = d_generators.cpu().numpy().copy()
    verdict, _ = verify_on_device(gpu_backend, oracle, st, offset=0, d_generators=d_generators)
    assert verdict == 1
    assert np.array_equal(d_generators.cpu().numpy(), generators), "the generators were modified"


@pytest.mark.gpu
def test_back_to_back_behind_the_prover(gpu_backend, oracle):
    """prove, verify the proof where the prover left it, verify a tampered copy in the same
    workspace, verify a second statement on the first verify's transcript: one side stream, nothing
    but the final synchronise"""
    import torch
    dev = torch.device("cuda", 0)
    n, offset = 1000, 3
    rng = np.random.default_rng(4000)
    a, b = scalars(rng, n), scalars(rng, n)
    t0 = oracle.transcript_new("prove then verify")
    gens = oracle.ristretto_generators(n, offset)
    st = object.__new__(Statement)
    st.__dict__.update(n=n, offset=offset, b=b, t0=t0,
                       commit=oracle.msm_projective(0, [(a, False)], gens)[0],
                       product=oracle.s25_inner_product(a, b))
    st.l, st.r, st.ap, t_proved = oracle.ip_prove(t0, n, offset, a, b)
    t_verified = st.expected(oracle)[1]
    third_st = Statement(oracle, 5, 11, 4001, t0=t_verified)  # proved on what the first verify leaves

    d_a, d_b = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    proof = DeviceProof(n, offset, d_a, d_b, t0)
    shared = torch.empty(api.inner_product_verify_workspace_bytes(n), dtype=torch.uint8, device=dev)
    first = DeviceVerify(st, True, workspace=shared, b=d_b, l=proof.l, r=proof.r, ap=proof.ap)
    bad_ap = st.ap.copy()
    bad_ap[0] ^= 1
    bad = st.copy(ap=bad_ap)
    second = DeviceVerify(bad, False, workspace=shared, b=d_b, l=proof.l, r=proof.r)
    want3_ok, want3_t = third_st.expected(oracle)
    assert want3_ok
    third = DeviceVerify(third_st, want3_ok, transcript=first.transcript)

    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    proof.enqueue(gpu_backend, side)
    for call in (first, second, third):
        call.enqueue(gpu_backend, side)
    side.synchronize()
    got_l, got_r, got_ap, got_t = proof.results()
    assert np.array_equal(got_l, st.l) and np.array_equal(got_r, st.r)
    assert np.array_equal(got_ap, st.ap) and np.array_equal(got_t, t_proved)
    assert first.results()[0] == 1
    verdict, t_after = second.results()
    want_ok, want_t = bad.expected(oracle)
    assert verdict == 0 and not want_ok and np.array_equal(t_after, want_t)
    verdict, t_after = third.results()
    assert verdict == 1 and np.array_equal(t_after, want3_t)


@pytest.mark.gpu
def test_verify_at_every_sponge_position(gpu_backend, oracle):
    """n = 2 (one round in k_verify_challenges) from every position of the sponge; the proofs come
    from the reference at that start"""
    import torch
    dev = torch.device("cuda", 0)
    starts = merlin_ref.padded_starts()
    side = torch.cuda.Stream(device=dev)
    workspace = torch.empty(api.inner_product_verify_workspace_bytes(2), dtype=torch.uint8, device=dev)
    reached = set()
    calls = []
    for pos in range(merlin_ref.RATE):
        st = Statement(oracle, 2, 0, 4200 + pos, t0=starts[pos])
        calls.append((pos, st, DeviceVerify(st, True, workspace=workspace)))
    torch.cuda.synchronize()
    for _, _, call in calls:
        call.enqueue(gpu_backend, side)
    side.synchronize()
    for pos, st, call in calls:
        verdict, t_after = call.results()
        model = sponge_model(starts[pos], 2, st.l, st.r)
        want_ok, want_t = st.expected(oracle)
        assert want_ok and verdict == 1, f"position {pos}"
        assert np.array_equal(t_after, model.array()), f"position {pos}: differs from the model"
        assert np.array_equal(t_after, want_t), f"position {pos}: differs from the reference"
        reached |= model.classes
    assert reached == merlin_ref.BOUNDARY_CLASSES


@pytest.mark.gpu
def test_many_partials_golden(gpu_backend):
    """n = 2^17 + 3: k_inner_product's grid-stride loop runs a second iteration over <e, b> under
    its cap of 256 workgroups.  The proof is the committed golden's, the commitment this library's
    own MSM on the gpu backend, the product Python integers."""
    import torch
    golden = np.load(GOLDEN)
    n, offset, seed = int(golden["n"]), int(golden["offset"]), int(golden["seed"])
    assert n == (1 << 17) + 3
    a, b = golden_inputs(n, seed)
    st = object.__new__(Statement)
    commit = gpu_backend.msm_projective(0, [(a, False)], gpu_backend.get_generators(n, offset))[0]
    words = lambda x: [int.from_bytes(row.tobytes(), "little") for row in x]  # noqa: E731
    product = sum(x * y for x, y in zip(words(a), words(b))) % L_ORDER
    st.__dict__.update(n=n, offset=offset, b=b, t0=api.transcript_new(golden["label"].tobytes()),
                       commit=commit, product=np.frombuffer(product.to_bytes(32, "little"), np.uint8),
                       l=golden["l"], r=golden["r"], ap=golden["ap"])
    bad_ap = st.ap.copy()
    bad_ap[0] ^= 1
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    for statement, want in ((st, 1), (st.copy(ap=bad_ap), 0)):
        call = DeviceVerify(statement, bool(want))
        torch.cuda.synchronize()
        call.enqueue(gpu_backend, side)
        side.synchronize()
        verdict, t_after = call.results()
        assert verdict == want
        assert np.array_equal(t_after, golden["transcript"])
        call.assert_inputs_unchanged()
