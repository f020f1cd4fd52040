"""The case tables of the MSM tail tests (tests/tail_cases.py), on the CPU: every launch passes the
harness's validation rules, the integer model equals a point-by-point evaluation with the group law
of tests/refmath.py, the transcribed closed form of heads_of equals the walk, and the tables hold the
edges they are there for -- as assertions, so that an edit cannot quietly lose one."""
import numpy as np
import pytest

from tests import refmath as rm
from tests import tail_cases as tc
from tests.test_device_arith import FAMILIES, family


def group(fam):
    """(add, identity, k -> k G by the family's own double-and-add)"""
    if fam == "ed":
        return rm.ed_add, rm.ED_IDENTITY, lambda k: rm.ed_mul(k, rm.ED_BASE)
    c = rm.CURVES[fam]
    return c.add, None, lambda k: c.mul(k, c.base)


@pytest.mark.parametrize("fam", FAMILIES)
def test_group_orders_and_pool(fam):
    _, identity, mul = group(fam)
    assert mul(tc.ORDER[fam]) == identity and mul(1) != identity
    assert tc.point_of(fam, -3) == tc.point_of(fam, tc.ORDER[fam] - 3) != tc.point_of(fam, 3)
    pool = tc.pool(fam)
    assert pool.shape == (256, family(fam).words)
    assert len({row.tobytes() for row in pool}) == 256
    for i in (0, 1, 127, 128, 200, 255):
        assert tc.pool_index(tc.POOL_K[i]) == i and tc.same_point(fam, pool[i], tc.POOL_K[i])
        assert not tc.same_point(fam, pool[i], tc.POOL_K[i] + 1)


def test_every_reduce_launch_passes_the_harness_rules():
    for case in tc.reduce_cases() + [tc.chained_case()]:
        for variant in case.variants or tc.REDUCE_LANES:
            stride = case.partial_stride(variant)
            assert tc.reduce_valid(case, variant, stride), (case.name, variant)
            assert not tc.reduce_valid(case, variant, stride - 2) or stride == 2
        assert not tc.reduce_valid(case, 0, case.partial_stride(0), num_heads=case.num_heads - 3)
        assert not tc.reduce_valid(case, 0, case.partial_stride(0), num_buckets=case.num_buckets - 4)
        # neighbouring slots differ, so a wrong index changes the result
        for task in case.tasks:
            assert np.all(np.diff(task.sum_idx) != 0) or (case.name == "algebra" and len(set(task.sum_idx)) == 1)
            assert np.all(np.diff(task.head_idx) != 0)


def test_every_horner_launch_passes_the_harness_rules():
    for case in tc.horner_cases():
        assert tc.horner_valid(case.lanes, case.params(), case.num_tasks, case.partial_stride, case.block_log2)
        used = max(ft + c.windows for ft, c in zip(case.first_task, case.columns))
        assert not tc.horner_valid(case.lanes, case.params(), used - 1, case.partial_stride, case.block_log2)
        # (the stride has one slot more than the widest task needs: garbage the kernel must not read)
        assert tc.horner_valid(case.lanes, case.params(), case.num_tasks, case.partial_stride - 1, case.block_log2)
        assert not tc.horner_valid(case.lanes, case.params(), case.num_tasks, case.partial_stride - 2, case.block_log2)
        owned = case.partial_scalars()
        assert all(t < case.num_tasks and blk < case.partial_stride - 1 for t, blk in owned)
        for ft, c in zip(case.first_task, case.columns):
            for w in range(c.windows):
                assert sum(c.block_scalars[w]) == c.sums[w] and (c.totals[w] == 0) == (w in c.zero)
    assert tc.horner_valid(256, [(0, 9, 0)] * 3, 0, 1, 8, null=True)


@pytest.mark.parametrize("fam", FAMILIES)
def test_harness_rejects_before_it_launches(fam):
    """every refusal of the tails objects is decided on the host: no GPU is needed to see it (the harness
    library is: __graft_entry__.build() compiles it, and tests/tail_hooks.py does where hipcc is installed)"""
    import subprocess

    from tests import tail_hooks as th
    try:
        th.lib()
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail(f"the device-hook harness is neither built nor buildable here (it needs hipcc): {e}")
    assert th.tail_sizes(fam)[0] == family(fam).words
    assert set(th.reduce_variants(fam)) <= set(tc.REDUCE_LANES)
    assert all(th.REDUCE_VARIANTS[v][1] == tc.REDUCE_LANES[v] for v in tc.REDUCE_LANES)
    th.assert_tail_rejections(fam)


def direct_partials(fam, task, block_buckets):
    """the model's sum with the group law, point by point"""
    add, identity, mul = group(fam)
    pts = [mul(k) if k > 0 else (rm.ed_neg(mul(-k)) if fam == "ed" else rm.CURVES[fam].neg(mul(-k)))
           for k in tc.POOL_K]
    out = [identity] * ((task.nb + block_buckets - 1) // block_buckets)
    for b in range(task.nb):
        begin, end = task.bounds(b)
        if begin == end:
            continue
        bucket = pts[task.sum_idx[b]]
        for i in tc.visited(begin, end, task.seg_log2):
            bucket = add(bucket, pts[task.head_idx[i]])
        running, weighted = bucket, identity           # (b + 1) * bucket by double-and-add
        for bit in bin(b + 1)[:1:-1]:
            if bit == "1":
                weighted = add(weighted, running)
            running = add(running, running)
        out[b // block_buckets] = add(out[b // block_buckets], weighted)
    return out


@pytest.mark.parametrize("fam", FAMILIES)
def test_model_equals_direct_evaluation(fam):
    dense = tc.reduce_cases()[0].tasks[3]                    # 64 buckets of 1 .. 3 entries
    long = tc.long_bucket_tasks(3)[7]                        # a middle bucket with two head partials
    assert dense.nb == 64 and len(long.heads(long.long_bucket)) == 2
    for task, block_buckets in ((dense, 16), (long, 64)):
        want = direct_partials(fam, task, block_buckets)
        got = task.partials(block_buckets)
        assert len(want) == len(got) and any(got)
        for k, pt in zip(got, want):
            assert tc.point_of(fam, k) == pt
    # a column: Horner over the window sums against the sum of shifted windows
    col = tc.horner_cases()[0].columns[3]
    assert col.windows == 17
    add, identity, mul = group(fam)
    acc = identity
    for w in reversed(range(col.windows)):
        for _ in range(col.bits):
            acc = add(acc, acc)
        for k in col.block_scalars[w]:
            acc = add(acc, tc.point_of(fam, k))
    assert tc.point_of(fam, col.value()) == acc
    assert col.value() == sum(s << (col.bits * w) for w, s in enumerate(col.sums))
    for k in tc.HORNER_SPLITS:
        assert col.value(0, k, col.value(k)) == col.value()


def test_closed_form_of_heads_equals_the_walk():
    table = tc.heads_of_table()
    assert 3000 < len(table) < (1 << 16) and {L for _, _, L in table} == {3, 5, 7}
    counts = set()
    for begin, end, L in table:
        walk = tc.visited(begin, end, L)
        assert tc.heads_closed_form(begin, end, L) == (len(walk), walk), (begin, end, L)
        assert len(walk) <= tc.HEADS_RETURNED and all(a < b for a, b in zip(walk, walk[1:]))
        assert not walk or (begin >> L) < walk[0] and walk[-1] <= (end - 1) >> L
        counts.add(len(walk))
    assert {0, 1, 2, 3, 16, 17, 18, 19} <= counts
    for task in tc.long_bucket_tasks(3) + tc.long_bucket_tasks(7) + tc.reduce_cases()[7].tasks:
        for b in range(task.nb):
            begin, end = task.bounds(b)
            if begin != end:
                walk = tc.visited(begin, end, task.seg_log2)
                assert tc.heads_closed_form(begin, end, task.seg_log2) == (len(walk), walk)


def test_tables_hold_their_edges():
    cases = {c.name: c for c in tc.reduce_cases()}
    assert [c.name for c in tc.reduce_cases()] == [
        "dense_lanes0", "dense_lanes1", "dense_lanes3", "sparse", "large_offsets", "long_buckets_seg3",
        "long_buckets_seg7", "heavy_overflow", "algebra", "mixed"]
    # long buckets: exactly 0, 1, 2, 16, 17, 40 and 300 heads (16 and 17 straddle the heavy threshold, 300
    # is a second round of the gather at 256 lanes), at both segment sizes, in every placement
    for seg_log2 in (3, 7):
        seen = set()
        for task in cases[f"long_buckets_seg{seg_log2}"].tasks:
            b = task.long_bucket
            begin, end = task.bounds(b)
            s0 = (begin >> seg_log2) + 1
            seen.add((len(task.heads(b)), b, s0 % 64 if b else None, begin % (1 << seg_log2) == 0,
                      end % (1 << seg_log2) == 0))
        heads = {s[0] for s in seen}
        assert heads == set(tc.LONG_HEADS) and 16 == tc.HEAVY_HEADS and max(heads) > 256
        for h in tc.LONG_HEADS:
            assert {s[1] for s in seen if s[0] == h} == {0, 7, 15}          # first, middle, last of the block
        for h in (16, 17):
            assert {s[2] for s in seen if s[0] == h} >= {None, 0, 63}       # first + 1 mod 64
            assert {s[3] for s in seen if s[0] == h} == {True, False}       # begin on / off a boundary
            assert {s[4] for s in seen if s[0] == h} == {True, False}       # end on / off a boundary
        assert {s[2] for s in seen} >= {0, 63} and {(s[3], s[4]) for s in seen} == {
            (True, True), (True, False), (False, True), (False, False)}
    # heavy buckets: 7, 8, 9 and 12 in one block of every variant, two of them in one lane's range
    heavy = cases["heavy_overflow"]
    assert [len(t.heavy) for t in heavy.tasks] == [7, 8, 9, 12]
    assert any(len(t.heavy) > tc.MAX_HEAVY for t in heavy.tasks)
    for variant in tc.REDUCE_LANES:
        assert all(heavy.blocks(variant, t) == 1 for t in range(4))
    lane = 1 << heavy.lane_log2
    for t in heavy.tasks:
        assert len({b // lane for b in t.heavy}) < len(t.heavy)
    # a block with block_first != 0 that holds entries, for every block size
    for variant, lanes in tc.REDUCE_LANES.items():
        for name in ("dense_lanes0", "dense_lanes1", "sparse", "large_offsets") + (("dense_lanes3",) if lanes == 64
                                                                                   else ()):
            case = cases[name]
            per = lanes << case.lane_log2
            assert any(any(task.partials(per)[1:]) for task in case.tasks), (name, variant)
    # a whole empty block, an empty lane, a 17-bit block offset
    sparse, large = cases["sparse"].tasks[0], cases["large_offsets"].tasks[0]
    assert sparse.nb == 1 << 15 and large.nb == 1 << 17 and cases["large_offsets"].lane_log2 == 6
    for lanes in (64, 256):
        assert 0 in sparse.partials(lanes << 3) and sparse.partials(lanes << 3)[-1] != 0
        assert large.partials(lanes << 6)[-1] != 0 and (large.nb - (lanes << 6)) >> 16 == 1
    # algebra: one point everywhere, and a populated block whose total is the identity
    same, _, _, zero = cases["algebra"].tasks
    assert len(set(same.sum_idx)) == 1 and zero.total != 0 and zero.partials(512) == [0, 0]
    # mixed: an empty task beside populated ones, under one stride
    mixed = cases["mixed"]
    assert [t.nb for t in mixed.tasks] == [1024, 64, 1024] and mixed.tasks[2].total == 0
    assert mixed.blocks(1, 1) == 1 < mixed.blocks(1, 0) == mixed.partial_stride(1) - 1
    # k_horner: every relation of team and blocks, for both block sizes
    for lanes in (64, 256):
        geo = [g for case in tc.horner_cases() if case.lanes == lanes for g in case.geometry()]
        assert any(team == 1 for team, _ in geo)
        assert any(team > blocks > 1 for team, blocks in geo) and any(blocks == 1 for _, blocks in geo)
        assert any(1 < team < blocks for team, blocks in geo) and any(team == blocks > 1 for team, blocks in geo)
        windows = {c.windows for case in tc.horner_cases() if case.lanes == lanes for c in case.columns}
        assert windows == set(tc.HORNER_WINDOWS[lanes]) and max(windows) == lanes
    assert (4, 64) in tc.horner_cases()[1].geometry() or (2, 64) in tc.horner_cases()[1].geometry()
    assert (8, 64) in tc.horner_cases()[4].geometry()                       # 64 blocks at W = 17, 256 lanes
    for case in tc.horner_cases():
        kinds = {c.kind for c in case.columns}
        zeros = [(c.windows, sorted(c.zero)) for c in case.columns if c.zero]
        assert len(kinds) >= 7 and (17, [16]) in zeros and (17, list(range(17))) in zeros and (17, [8]) in zeros
        assert {c.bits for c in case.columns} >= ({1, 2, 9, 12} if case.block_log2 == 6 else {1, 2, 9, 16})
    kinds = {c.kind for case in tc.horner_cases() for c in case.columns}
    assert kinds == set(tc.HORNER_KINDS)
    # the column whose top five windows are empty: the split at 16 lies inside what the chain trims
    assert any(c.zero == set(range(12, 17)) for c in tc.horner_cases()[0].columns) and 16 in tc.HORNER_SPLITS
