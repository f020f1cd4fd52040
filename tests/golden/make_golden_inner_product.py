"""Records tests/golden/inner_product_golden.npz: the reference's own inner-product proof
(oracle.ip_prove) of n = 2^17 + 3 elements, a size at which the reference's CPU prover is too slow
to run inside a GPU test.  Only the proof is stored (L, R, ap, the transcript after it: under
2 KB); tests/test_inner_product_device.py regenerates the inputs from the seed.

    python tests/golden/make_golden_inner_product.py      (where oracle/_ref is built)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "inner_product_golden.npz")
N, OFFSET, SEED, LABEL = (1 << 17) + 3, 0, 2800, b"many partials"


def golden_inputs(n, seed):
    """a and b: a seeded numpy stream, top four bits cleared (below 2^252: reduced)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f
    b[:, 31] &= 0x0f
    return a, b


def main():
    from oracle import ref_oracle
    a, b = golden_inputs(N, SEED)
    t0 = ref_oracle.transcript_new(LABEL)
    l, r, ap, t = ref_oracle.ip_prove(t0, N, OFFSET, a, b)
    np.savez(GOLDEN, n=np.uint64(N), offset=np.uint64(OFFSET), seed=np.uint64(SEED),
             label=np.frombuffer(LABEL, np.uint8), l=l, r=r, ap=ap, transcript=t)
    print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
