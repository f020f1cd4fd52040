"""k_reduce's phase 1 -- a lane's bucket sums, head partials and r += s taken as one chain through one
addition site (msm/kernels.h) -- on the shapes at which that walk can go wrong, through the harness of
tests/tail_hooks.py against the integer model of tests/tail_cases.py.  Every case is ONE task of at
most 4096 buckets; the partials are compared as group elements, the untouched slots with the sentinel.

What the tables below build, and assert about themselves before anything is launched:

    head_spread     buckets with 0, 1, 2 and 3 heads inside one lane's range; a wavefront in which one
                    lane's chain is several times the others'; nb no multiple of the block, the task's
                    last lane short of its buckets; two 256-lane blocks (block_first == 0 and != 0)
    empty_buckets   empty buckets at the start, the end and in the middle of a lane; a lane, and a
                    whole wavefront, of empty buckets between populated ones
    whole_segments  buckets over runs of 64 whole segments (the "multiples of 64" heads of heads_of),
                    at 8- and at 32-entry segments, on and off a segment boundary
    heavy           exactly kReduceHeavyHeads heads (stays with its lane), one more (folded by the
                    workgroup), and more than kReduceMaxHeavy heavy buckets in one block, two of them
                    in one lane
    equal_points    the incoming item equal to s (the same limbs, and the same point under another Z),
                    its negative, and the identity -- as a bucket sum and as a head partial; r == s
                    when r += s runs (an empty bucket under the lane's first populated one)

curve25519 runs every case, bn254 head_spread and empty_buckets (which hold both block offsets), each
at 8 and at 64 buckets per lane and in every k_reduce<C, Scan, T> the engine launches for the curve.
k_reduce_compact keeps its own walk and is covered by tests/test_msm_tails_device.py."""
import functools

import numpy as np
import pytest

from tests import tail_cases as tc
from tests import tail_hooks as th

pytestmark = pytest.mark.gpu

LANE_LOG2 = (3, 6)
COMPACT = 4                      # harness variant of k_reduce_compact


@pytest.fixture(scope="module", autouse=True)
def device():
    import ctypes
    n = ctypes.c_int(0)
    assert th.lib().hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0, "these tests need a GPU"


class ChainTask(tc.Task):
    """a task some of whose bucket sums and head partials are k G for a k outside the pool (0: the
    identity), written over the pool's rows before the launch"""

    def __init__(self, counts, seg_log2, salt=0):
        super().__init__(counts, seg_log2, salt)
        self.sum_k, self.head_k = {}, {}

    def bucket_scalar(self, b):
        own = self.sum_k.get(b, tc.POOL_K[self.sum_idx[b]])
        return own + sum(self.head_k.get(i, tc.POOL_K[self.head_idx[i]]) for i in self.heads(b))

    def head_counts(self, first, last):
        return [len(self.heads(b)) for b in range(first, last)]


def grow_to_heads(counts, b, heads, seg_log2):
    """the smallest count of bucket b (the buckets below it fixed) that gives it `heads` heads"""
    begin = int(sum(counts[:b]))
    for n in range(1, (64 * (heads + 2)) << seg_log2):
        if len(tc.visited(begin, begin + n, seg_log2)) == heads:
            counts[b] = n
            return
    raise AssertionError((b, heads, seg_log2))


@functools.lru_cache(None)
def head_spread():
    nb = 2048 + 128 * 8 + 5              # 256 x 8: two blocks, the second 128 lanes and one of 5 buckets
    counts = [1] * nb
    for b, h in ((40, 0), (41, 1), (42, 2), (43, 3), (45, 1), (47, 2)):       # lane 5 of block 0
        grow_to_heads(counts, b, h, 3)
    for b in range(2048 + 8 * 70, 2048 + 8 * 71):                             # block 1, wave 1, lane 6 alone
        grow_to_heads(counts, b, 2 + b % 2, 3)
    for b in range(2048 + 8 * 100, 2048 + 8 * 128):                           # ... whose upper lanes hold nothing
        counts[b] = 0
    for b, h in ((nb - 4, 2), (nb - 2, 1), (nb - 1, 3)):                      # the short last lane
        grow_to_heads(counts, b, h, 3)
    task = ChainTask(counts, 3, 41)
    assert task.head_counts(40, 44) == [0, 1, 2, 3]
    long_lane = sum(task.head_counts(2048 + 560, 2048 + 568))
    assert long_lane >= 20 and all(sum(task.head_counts(2048 + 8 * t, 2048 + 8 * t + 8)) == 0
                                   for t in range(64, 128) if t != 70)
    assert nb % 512 != 0 and nb % 8 == 5 and task.head_counts(nb - 4, nb) == [2, 0, 1, 3]
    return task


@functools.lru_cache(None)
def empty_buckets():
    nb = 2048 + 300
    counts = [2] * nb
    lanes = {3: [0, 0, 0, 5, 1, 9, 1, 2],        # empty at the start of the lane (its lowest buckets)
             4: [1, 9, 2, 3, 17, 0, 0, 0],       # ... at the end: the walk starts on empty buckets
             5: [3, 0, 0, 12, 0, 1, 0, 20],      # ... in the middle
             6: [0] * 8,                         # a lane of empty buckets between populated ones
             7: [0, 0, 0, 0, 0, 0, 0, 25],
             8: [30, 0, 0, 0, 0, 0, 0, 0],
             0: [0, 0, 4, 0, 0, 0, 0, 0],        # the block's first lane, bucket 0 empty
             256 + 10: [0, 19, 0, 0, 33, 0, 0, 0]}
    for lane, c in lanes.items():
        counts[8 * lane:8 * lane + 8] = c
    counts[8 * 64:8 * 128] = [0] * 512           # a wavefront of empty lanes
    counts[nb - 3:] = [0, 7, 0]
    task = ChainTask(counts, 3, 42)
    assert max(task.head_counts(8 * 5, 8 * 6)) >= 2 and task.total != 0
    return task


@functools.lru_cache(None)
def whole_segments(seg_log2):
    nb = 600
    counts = [1, 2, 1, 3] * (nb // 4)
    seg = 1 << seg_log2
    counts[13] = 64 * seg * 3 + 5                # ends off a segment boundary
    counts[14] = 64 * seg + 1
    counts[300] = 64 * seg * 2 - (sum(counts[:300]) % seg)     # ends on one
    counts[301] = 64 * seg * 2
    counts[597] = 64 * seg * 5 + seg // 2
    task = ChainTask(counts, seg_log2, 43 + seg_log2)
    for b in (13, 300, 301, 597):
        begin, end = task.bounds(b)
        count, index = tc.heads_closed_form(begin, end, seg_log2)
        assert index == task.heads(b) and 2 <= count <= tc.HEAVY_HEADS
        assert any(i % 64 == 0 and (i + 1) << seg_log2 <= end for i in index[1:])      # a run's first segment
    assert task.bounds(300)[1] % seg == 0 and task.bounds(13)[1] % seg != 0
    return task


@functools.lru_cache(None)
def heavy():
    nb = 300                                     # one 256-lane block, five 64-lane blocks
    counts = [1, 0, 2, 1, 3, 1] * (nb // 6)
    at = [(9, 16), (20, 17), (21, 18), (75, 17), (130, 19), (131, 16), (190, 17), (200, 18), (230, 17), (255, 17),
          (270, 18), (280, 17), (290, 17), (299, 16)]
    for b, heads in at:                          # in bucket order: every begin is final when its end is chosen
        begin = int(sum(counts[:b]))
        counts[b] = tc.long_bucket_end(begin, heads, 3, b % 2 == 0) - begin
    task = ChainTask(counts, 3, 44)
    assert [len(task.heads(b)) for b, _ in at] == [h for _, h in at]
    heavies = [b for b, h in at if h > tc.HEAVY_HEADS]
    assert len(heavies) > tc.MAX_HEAVY and 20 // 8 == 21 // 8 and 16 in dict(at).values()
    return task


@functools.lru_cache(None)
def equal_points():
    nb = 600
    counts = [0] * nb
    lanes = {2: [1, 0, 1, 1, 0, 1, 1, 1],        # sums below
             3: [0, 0, 0, 9, 0, 0, 0, 12],       # one head each
             5: [1, 1, 0, 0, 1, 1, 1, 1],
             9: [0, 0, 1, 0, 0, 20, 0, 0],       # two heads
             70: [1, 1, 1, 1, 1, 1, 1, 1]}
    for lane, c in lanes.items():
        counts[8 * lane:8 * lane + 8] = c
    for b, h in ((27, 1), (31, 1), (77, 2)):
        grow_to_heads(counts, b, h, 3)
    task = ChainTask(counts, 3, 45)
    # lane 2, from its last bucket down: s = 5 G, + 5 G (the same limbs), + 10 G as 5 G + 5 G had it ...
    for b, k in ((23, 5), (22, 5), (21, 10), (19, -20), (18, 7), (16, 7)):
        task.set_sum(b, k)
    task.sum_k[19] = -20                         # s = 20 G, the item its negative under another Z: s = 0
    # lane 3: the head equal to the bucket's sum; then s = 2 * 9 G and the item -18 G: through the identity
    (h31,), (h27,) = task.heads(31), task.heads(27)
    task.set_sum(31, 9)
    task.head_idx[h31] = tc.pool_index(9)
    task.sum_k[27] = -18
    task.head_k[h27] = 0                         # ... and the identity as a head partial
    # lane 5: identities as bucket sums, at the start of the chain (s = 0 + 0) and inside it
    for b in (47, 45, 41):
        task.sum_k[b] = 0
    task.set_sum(46, 3)
    task.set_sum(44, 3)                          # s = 3 G + 0 + 3 G: equal again
    # lane 9: both heads the identity, then a bucket whose sum cancels the lane's s
    for i in task.heads(77):
        task.head_k[i] = 0
    task.set_sum(77, 11)
    task.set_sum(74, -11)
    # lane 70 (the second wavefront): the same pool row in every bucket
    task.sum_idx[560:568] = tc.pool_index(-6)
    assert len(task.heads(31)) == 1 and len(task.heads(77)) == 2
    return task


CASES = {"head_spread": head_spread, "empty_buckets": empty_buckets,
         "whole_segments_seg3": lambda: whole_segments(3), "whole_segments_seg5": lambda: whole_segments(5),
         "heavy": heavy, "equal_points": equal_points}
ON_CURVE = {"ed": list(CASES), "bn254": ["head_spread", "empty_buckets"]}


def launch_arrays(fam, case, task):
    pool = tc.pool(fam)
    sums, heads = pool[case.sum_idx].copy(), pool[case.head_idx].copy()
    _, _, bucket_base, segment_base = case.params[0]
    for b, k in task.sum_k.items():
        sums[bucket_base + b] = tc.encode(fam, k, 3 + b)
    for i, k in task.head_k.items():
        heads[segment_base + i] = tc.encode(fam, k, 5 + i)
    return sums, heads


@pytest.mark.parametrize("lane_log2", LANE_LOG2)
@pytest.mark.parametrize("fam,name", [(fam, name) for fam, names in ON_CURVE.items() for name in names])
def test_reduce_chain(fam, name, lane_log2):
    task = CASES[name]()
    assert task.nb <= 4096
    case = tc.ReduceCase(name, lane_log2, [task])
    sums, heads = launch_arrays(fam, case, task)
    variants = [v for v in th.reduce_variants(fam) if v != COMPACT]
    assert 0 in variants and 1 in variants
    blocks_seen = set()
    for variant in variants:
        stride = case.partial_stride(variant)
        assert tc.reduce_valid(case, variant, stride)
        partials, totals = th.reduce(fam, variant, lane_log2, case.params, case.ends, sums, heads, stride)
        want = case.expected(variant)[0]
        what = (fam, name, lane_log2, th.REDUCE_VARIANTS[variant][0])
        assert int(totals[0]) == task.total, what
        assert len(want) == case.blocks(variant, 0) < partials.shape[1]
        for blk, k in enumerate(want):
            assert tc.same_point(fam, partials[0, blk], k), what + (blk,)
        assert bool(np.all(partials[0, len(want):] == th.SENTINEL)), what + ("slots beyond the task's blocks",)
        blocks_seen.add(len(want))
    if lane_log2 == 3 and name in ("head_spread", "empty_buckets"):
        assert max(blocks_seen) > 1 and 2 in blocks_seen      # block_first != 0, at 256 and at 64 lanes
    print(f"[reduce_chain] {fam}/{name} at {1 << lane_log2} buckets per lane: {len(variants)} variants, "
          f"{task.nb} buckets, {task.total} entries")
