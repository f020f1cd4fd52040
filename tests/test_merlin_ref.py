"""tests/merlin_ref.py (the plain-Python Merlin the sumcheck transcript tests take their expected
bytes from) against the compiled reference, through what the oracle exposes: a fresh
prft::transcript for several labels, and the transcript the reference's inner-product prover
leaves behind, replayed here from the L and R values it returned (labels:
sxt/proof/inner_product/proof_computation.cc)."""
import numpy as np
import pytest

from tests import merlin_ref


def test_keccak_constants():
    """the generated tables against the published ones (FIPS 202)"""
    assert merlin_ref.RC[:4] == [1, 0x8082, 0x800000000000808a, 0x8000000080008000]
    assert merlin_ref.RC[23] == 0x8000000080008008
    assert [merlin_ref.ROT[x][0] for x in range(5)] == [0, 1, 62, 28, 27]
    assert [merlin_ref.ROT[x][4] for x in range(5)] == [18, 2, 61, 56, 14]


@pytest.mark.parametrize("label", ["", "a", "smoke", "sumcheck", "x" * 200])
def test_fresh_transcript(oracle, label):
    assert np.array_equal(merlin_ref.Transcript(label=label).array(), oracle.transcript_new(label))


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_inner_product_transcript_replayed(oracle, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    b[:, 31] &= 0x0f
    t0 = oracle.transcript_new("replay")
    l, r, _, after = oracle.ip_prove(t0, n, 0, a, b)
    t = merlin_ref.Transcript(raw=t0)
    t.append_message(b"domain-sep", b"inner product proof v1")
    t.append_u64(b"n", n)
    for i in range(l.shape[0]):
        t.append_message(b"L", l[i].tobytes())
        t.append_message(b"R", r[i].tobytes())
        t.challenge_bytes(b"x", 32)
    assert l.shape[0] == max(n - 1, 0).bit_length()
    assert np.array_equal(t.array(), after)
