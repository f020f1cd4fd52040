"""The two kernels that end every variable-base MSM, run directly on the GPU: k_reduce /
k_reduce_compact and k_horner of msm/kernels.h, instantiated as msm/engine.h launches them
(tests/native/tail_hooks.hip), on plain arrays of points and offsets, against the integer model of
tests/tail_cases.py (checked on the CPU by tests/test_tail_cases.py).  Everything is exact: partials
and projective outputs as group elements, encodings byte for byte, and the slots a kernel must leave
alone still hold the harness's sentinel.

Each test prints its case count (run with -s to see them)."""
import numpy as np
import pytest

from tests import hooks
from tests import refmath as rm
from tests import tail_cases as tc
from tests import tail_hooks as th
from tests.test_device_arith import FAMILIES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    import ctypes
    n = ctypes.c_int(0)      # (the HIP runtime the harness library is linked against)
    assert th.lib().hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0, "these tests need a GPU"


def count(op, n):
    print(f"[msm_tails] {op}: {n} cases")


def untouched(a):
    return bool(np.all(np.asarray(a, np.uint32) == th.SENTINEL))


#--------------------------------------------------------------------------------------------------
# k_reduce
#--------------------------------------------------------------------------------------------------
def run_reduce(fam, case, variant):
    pool = tc.pool(fam)
    return th.reduce(fam, variant, case.lane_log2, case.params, case.ends, pool[case.sum_idx], pool[case.head_idx],
                     case.partial_stride(variant))


def check_reduce(fam, case, variant):
    partials, totals = run_reduce(fam, case, variant)
    what = (fam, case.name, th.REDUCE_VARIANTS[variant][0])
    checked = 0
    for t, (task, want) in enumerate(zip(case.tasks, case.expected(variant))):
        assert int(totals[t]) == task.total == int(task.ends[-1]), what + (t,)
        assert len(want) == case.blocks(variant, t) < partials.shape[1]
        for blk, k in enumerate(want):
            assert tc.same_point(fam, partials[t, blk], k), what + (t, blk)
        # slots at or beyond the task's own block count are not written
        assert untouched(partials[t, len(want):]), what + (t, "slots beyond the task's blocks")
        checked += len(want)
    return checked


REDUCE_CASE_NAMES = [c.name for c in tc.reduce_cases()]


@pytest.mark.parametrize("name", REDUCE_CASE_NAMES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_reduce(fam, name):
    """every variant the engine launches for the curve, on: dense buckets (no or one head each, blocks with
    a non-zero first bucket), sparse buckets (empty blocks and lanes, stale sums everywhere else), 17-bit
    block offsets, long buckets (0 .. 300 heads, on and off segment and wavefront boundaries), more heavy
    buckets than the cooperative fold takes, sums that pass through the identity, tasks of different size
    and an empty one under one stride"""
    case = {c.name: c for c in tc.reduce_cases()}[name]
    total = 0
    for variant in th.reduce_variants(fam):
        total += check_reduce(fam, case, variant)
    count(f"{fam}/reduce {name} ({len(th.reduce_variants(fam))} variants, {len(case.tasks)} tasks)", total)


@pytest.mark.parametrize("fam", FAMILIES)
def test_heads_of_closed_form_equals_the_walk(fam):
    table = tc.heads_of_table()
    got = th.heads_of(fam, table)
    for (begin, end, seg_log2), row in zip(table, got):
        walk = tc.visited(begin, end, seg_log2)
        assert int(row[0]) == len(walk), (begin, end, seg_log2)
        assert [int(v) for v in row[1:1 + len(walk)]] == walk, (begin, end, seg_log2)
    count(f"{fam}/heads_of", len(table))


#--------------------------------------------------------------------------------------------------
# k_horner
#--------------------------------------------------------------------------------------------------
def encoded(fam, k):
    """the canonical encoding of k G: tests/refmath.py where it has the encoder, the host encoders of the
    product's headers (tests/hooks.py) on the model's point otherwise"""
    pt = tc.point_of(fam, k)
    if fam == "ed":
        return rm.ristretto_encode(rm.ed_extended(pt, 1))
    c = rm.CURVES[fam]
    p64 = np.array(rm.sw_point64(c, c.projective(pt, 1)), np.uint64)
    if fam == "bls12_381":
        return bytes(hooks.bls_compress(p64))
    xy, inf = hooks.sw_to_affine(c.cid, p64)
    return xy.tobytes() + int(inf).to_bytes(8, "little")


def projective_is(fam, out_bytes, k):
    ls = [int(v) for v in np.frombuffer(out_bytes.tobytes(), np.uint64)]
    if fam == "ed":
        return rm.ed_same(rm.ed_from51(ls), tc.point_of(fam, k))
    c = rm.CURVES[fam]
    return c.same(rm.sw_from64(c, ls), tc.point_of(fam, k))


def point_words(fam, k, salt):
    if k != 0 and abs(k) <= 128:
        return tc.pool(fam)[tc.pool_index(k)]
    return tc.encode(fam, k, 2 + salt)


def horner_partials(fam, case):
    """every slot holds a point: the pool's where no column owns it (slots >= blocks, tasks in between)"""
    pool = tc.pool(fam)
    idx = (7 + 13 * np.arange(case.num_tasks * case.partial_stride)) % 256
    partials = pool[idx].reshape(case.num_tasks, case.partial_stride, -1).copy()
    for (t, blk), k in case.partial_scalars().items():
        partials[t, blk] = point_words(fam, k, t + blk)
    return partials


def run_horner(fam, case, partials, projective_out=0, w_lo=0, w_hi=0xffffffff, first=1, last=1, state=None):
    return th.horner(fam, case.lanes, case.params(), partials, case.partial_stride, case.task_total(), w_lo, w_hi,
                     first, last, projective_out, case.block_log2, state)


HORNER_CASE_NAMES = [c.name for c in tc.horner_cases()]


@pytest.mark.parametrize("name", HORNER_CASE_NAMES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_horner(fam, name):
    """columns of 1 .. T windows in one launch, blocks per window below, at and above the lanes per window,
    empty top / middle / all windows, identity, doubling and cancellation in the chain; encoded and
    projective output; state is not written by a whole-column launch"""
    case = {c.name: c for c in tc.horner_cases()}[name]
    partials = horner_partials(fam, case)
    out, state = run_horner(fam, case, partials)
    for i, col in enumerate(case.columns):
        assert out[i].tobytes() == encoded(fam, col.value()), (fam, name, i, col.windows, col.bits, col.kind)
    assert untouched(state)
    proj, state = run_horner(fam, case, partials, projective_out=1)
    for i, col in enumerate(case.columns):
        assert projective_is(fam, proj[i], col.value()), (fam, name, i, col.windows, col.bits, col.kind)
    assert untouched(state)
    count(f"{fam}/horner {name}", 2 * len(case.columns))


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("fam", FAMILIES)
def test_horner_window_ranges_compose(fam, lanes):
    """[k, W) with first = 1, last = 0, then [0, k) with first = 0, last = 1 gives the bytes of the single
    full launch, for split points below, inside and above columns -- and inside the empty top windows the
    chain trims; w_hi beyond a column's windows clamps"""
    case = [c for c in tc.horner_cases() if c.lanes == lanes and c.block_log2 == 9][0]
    partials = horner_partials(fam, case)
    full, _ = run_horner(fam, case, partials)
    for split in tc.HORNER_SPLITS:
        out, state = run_horner(fam, case, partials, w_lo=split, first=1, last=0)
        assert np.all(out == (th.SENTINEL & 0xff)), "a launch that is not the last one writes no output"
        for i, col in enumerate(case.columns):
            upper = col.value(min(split, col.windows))
            assert tc.same_point(fam, state[i], upper), (fam, lanes, split, i)
        out, state2 = run_horner(fam, case, partials, w_lo=0, w_hi=split, first=0, last=1, state=state)
        assert np.array_equal(state2, state), "the last launch leaves the state alone"
        for i, col in enumerate(case.columns):
            assert out[i].tobytes() == full[i].tobytes() == encoded(fam, col.value()), (fam, lanes, split, i)
    count(f"{fam}/horner ranges T = {lanes}", 2 * len(tc.HORNER_SPLITS) * len(case.columns))


@pytest.mark.parametrize("fam", FAMILIES)
def test_horner_without_tasks(fam):
    """the engine's launch for a call whose columns are all empty: null partials, identity encodings"""
    columns = [(0, 9, 0), (0, 16, 0), (0, 1, 0)]
    for lanes in (64, 256):
        for projective_out in (0, 1):
            out, _ = th.horner(fam, lanes, columns, None, 1, None, 0, 0, 1, 1, projective_out, 8)
            for row in out:
                if projective_out:
                    assert projective_is(fam, row, 0)
                else:
                    assert row.tobytes() == encoded(fam, 0)
    count(f"{fam}/horner without tasks", 4 * len(columns))


@pytest.mark.parametrize("fam", FAMILIES)
def test_reduce_feeds_horner(fam):
    """one column of three 9-bit windows through k_reduce at 64 lanes of two buckets and k_horner at 128
    buckets per block: the expected value comes from the bucket contents alone"""
    case = tc.chained_case()
    partials, totals = run_reduce(fam, case, 1)
    want = sum(task.total_scalar() << (9 * w) for w, task in enumerate(case.tasks))
    assert case.blocks(1, 0) == 2 and partials.shape[1] == 3
    for lanes in (64, 256):
        out, _ = th.horner(fam, lanes, [(0, 9, 3)], partials, partials.shape[1], totals, 0, 0xffffffff, 1, 1, 0, 7)
        assert out[0].tobytes() == encoded(fam, want), (fam, lanes)
    count(f"{fam}/reduce -> horner", 2)


@pytest.mark.parametrize("fam", FAMILIES)
def test_harness_rejects_what_it_cannot_validate(fam):
    th.assert_tail_rejections(fam)
