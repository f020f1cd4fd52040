"""Case tables and integer model of tests/test_msm_tails_device.py: the inputs that put k_reduce /
k_reduce_compact and k_horner (msm/kernels.h) on every path their indexing, thresholds and LDS trees
have, with what they must compute.  Pure Python, built once per process; tests/test_tail_cases.py
checks the tables on the CPU, the GPU module compares the kernels with them.

Every point is k G for an integer k.  bucket_sums and head partials are gathered from a pool of 256
encoded points (k = +-1 .. +-128, varied Z) by index arrays, so a case is a handful of integer arrays
and its expectation is integer arithmetic modulo the group order:

    partial[task][block] = sum over the block's buckets with begin != end of
                           (b + 1) * (k_sum[b] + sum of k_head[i] for i in visited(begin, end, L))
    column               = sum_w 2^(c w) * sum_blk partial[w][blk]

`visited` is written from the comment above load_bucket ("the owner's partial plus the heads of the
following segments the bucket extends into.  Whole segments of one wavefront (64 consecutive
segments) were folded into the first of them"), as the walk; `heads_closed_form` transcribes the
closed form heads_of of the same header for the comparison of the two."""
import functools
import random

import numpy as np

from tests import refmath as rm
from tests.test_device_arith import FAMILIES, family

HEAVY_HEADS, MAX_HEAVY = 16, 8            # kReduceHeavyHeads, kReduceMaxHeavy of msm/kernels.h
REDUCE_LANES = {0: 256, 1: 64, 2: 256, 3: 64, 4: 256}     # lanes of a block per harness variant
HEADS_RETURNED = 24

# orders of the base points' groups (bls12-381: of the whole curve, h r -- the first point of the curve
# is not in the prime-order subgroup); tests/test_tail_cases.py checks ORDER G = identity
ORDER = {
    "ed": rm.ED_L,
    "bn254": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
    "grumpkin": rm.BN254.p,
    "bls12_381": 0x396c8c005555e1568c00aaab0000aaab
    * 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}

#--------------------------------------------------------------------------------------------------
# points
#--------------------------------------------------------------------------------------------------
POOL_K = list(range(1, 129)) + [-k for k in range(1, 129)]
POOL_ZS = [1, 2, 3, 0x10001, (1 << 200) + 12345, (1 << 253) - 7, 0xdeadbeefcafef00d, 5 << 100]


def pool_index(k):
    """pool slot of k G, 1 <= |k| <= 128"""
    assert 1 <= abs(k) <= 128
    return k - 1 if k > 0 else 127 - k


@functools.lru_cache(None)
def _point(fam, k):
    f = family(fam)
    if fam == "ed":
        pt = f.point(abs(k))
        return rm.ed_neg(pt) if k < 0 else pt
    return f.point(k)


def point_of(fam, k):
    """k G for any integer k, through the representative of k of least magnitude"""
    k %= ORDER[fam]
    if k > ORDER[fam] // 2:
        k -= ORDER[fam]
    return _point(fam, k)


def encode(fam, k, z):
    """k G in the engine's limbs (a C::point) with the given Z"""
    return family(fam).encode(point_of(fam, k), z)


@functools.lru_cache(None)
def pool(fam):
    """(256, words) uint32"""
    return np.array([encode(fam, k, POOL_ZS[(i * 3 + i // 8) % len(POOL_ZS)] + i) for i, k in enumerate(POOL_K)],
                    dtype=np.uint32)


def same_point(fam, words, k):
    """the engine-form point in `words` is k G (any limbs the kernels leave: compared as a group element)"""
    words = [int(w) for w in words]
    if fam == "ed":
        return rm.ed_same(rm.ed_from29(words), point_of(fam, k))
    c = rm.CURVES[fam]
    return c.same(rm.sw_from29(c, words), point_of(fam, k))


#--------------------------------------------------------------------------------------------------
# head partials of a bucket
#--------------------------------------------------------------------------------------------------
def visited(begin, end, seg_log2):
    """segments whose head partial belongs to the bucket of sorted entries [begin, end): the walk.  The
    bucket's owner lane sits in segment `first`; every later segment the bucket reaches into left a head,
    except that the whole segments of one wavefront (64 consecutive segments, 64 k .. 64 k + 63) were
    folded into the first of them that lies in the bucket"""
    assert begin < end
    first, last = begin >> seg_log2, (end - 1) >> seg_log2
    whole_end = end >> seg_log2          # segments first + 1 .. whole_end - 1 lie entirely in the bucket
    out, s = [], first + 1
    while s <= last:
        out.append(s)
        if s < whole_end:                # a whole segment: it carries the rest of its wavefront's run
            s = min((s // 64 + 1) * 64, whole_end)
        else:                            # the trailing partial segment
            s += 1
    return out


def heads_closed_form(begin, end, seg_log2):
    """heads_of of msm/kernels.h, transcribed: (count, [index(j) for j < count])"""
    first, last = begin >> seg_log2, (end - 1) >> seg_log2
    after_whole = end >> seg_log2
    s0 = first + 1
    k_lo = s0 // 64 + 1
    k_hi_plus_1 = (after_whole + 63) // 64
    middle = k_hi_plus_1 - k_lo if k_hi_plus_1 > k_lo else 0
    tail = 1 if after_whole <= last and after_whole > s0 else 0
    count = 0 if s0 > last else 1 + middle + tail
    index = lambda j: s0 if j == 0 else ((k_lo + j - 1) * 64 if j <= middle else after_whole)  # noqa: E731
    return count, [index(j) for j in range(count)]


@functools.lru_cache(None)
def heads_of_table():
    """(begin, end, segment_log2) triples around segment and wavefront boundaries"""
    out = []
    for L in (3, 5, 7):
        seg, wave = 1 << L, 64 << L
        begins = {0, 1, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 5 * seg + 3}
        for at in (62 * seg, 63 * seg, wave, wave + seg, 2 * wave - seg, 2 * wave, 126 * seg + wave, 3 * wave):
            begins |= {at - 1, at, at + 1, at + seg // 2}
        lengths = {1, 2, seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 2 * seg + 1, 3 * seg - 1, 3 * seg, 3 * seg + 1}
        for waves in (1, 2, 15, 16, 17, 18):
            for d in (-seg, 0, seg):
                lengths |= {waves * wave + d - 1, waves * wave + d, waves * wave + d + 1}
        out += [(b, b + n, L) for b in sorted(begins) for n in sorted(lengths)]
    return out


#--------------------------------------------------------------------------------------------------
# k_reduce: tasks, launches, model
#--------------------------------------------------------------------------------------------------
class Task:
    """one (column, window): bucket end offsets and the pool slot of every bucket sum and head partial.
    Every slot holds a point -- empty buckets and heads the walk skips too -- and neighbours differ"""

    def __init__(self, counts, seg_log2, salt=0):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.nb, self.seg_log2 = len(self.counts), seg_log2
        self.ends = np.cumsum(self.counts).astype(np.uint32)
        self.total = int(self.ends[-1])
        assert int(self.counts.sum()) == self.total
        self.num_heads = (self.total >> seg_log2) + 2
        self.sum_idx = (3 + salt + 7 * np.arange(self.nb)) % 256
        self.head_idx = (11 + 3 * salt + 5 * np.arange(self.num_heads)) % 256

    def set_sum(self, b, k):
        self.sum_idx[b] = pool_index(k)

    def bounds(self, b):
        return (0 if b == 0 else int(self.ends[b - 1])), int(self.ends[b])

    def heads(self, b):
        begin, end = self.bounds(b)
        return visited(begin, end, self.seg_log2) if begin != end else []

    def bucket_scalar(self, b):
        return POOL_K[self.sum_idx[b]] + sum(POOL_K[self.head_idx[i]] for i in self.heads(b))

    def partials(self, block_buckets):
        """the integer of every block"""
        blocks = (self.nb + block_buckets - 1) // block_buckets
        out = [0] * blocks
        for b in np.nonzero(self.counts)[0]:
            out[int(b) // block_buckets] += (int(b) + 1) * self.bucket_scalar(int(b))
        return out

    def total_scalar(self):
        return sum(self.partials(self.nb))


class ReduceCase:
    """one launch: several tasks with distinct bucket_base / segment_base, laid out back to front with a
    few unowned buckets and head slots between them"""

    def __init__(self, name, lane_log2, tasks, variants=None):
        self.name, self.lane_log2, self.tasks, self.variants = name, lane_log2, tasks, variants
        bucket_at, head_at, self.params = 2, 1, [None] * len(tasks)
        for t in reversed(range(len(tasks))):
            task = tasks[t]
            self.params[t] = (task.nb, task.seg_log2, bucket_at, head_at)
            bucket_at += task.nb + 3
            head_at += task.num_heads + 2
        self.num_buckets, self.num_heads = bucket_at, head_at
        self.ends = np.zeros(self.num_buckets, np.uint32)
        self.sum_idx = (5 * np.arange(self.num_buckets) + 1) % 256
        self.head_idx = (9 * np.arange(self.num_heads) + 2) % 256
        for task, (nb, _, bb, sb) in zip(tasks, self.params):
            self.ends[bb:bb + nb] = task.ends
            self.sum_idx[bb:bb + nb] = task.sum_idx
            self.head_idx[sb:sb + task.num_heads] = task.head_idx

    def blocks(self, variant, t):
        per = REDUCE_LANES[variant] << self.lane_log2
        return (self.tasks[t].nb + per - 1) // per

    def partial_stride(self, variant):
        """one slot more than the largest task needs: every task has slots beyond its own blocks"""
        return max(self.blocks(variant, t) for t in range(len(self.tasks))) + 1

    def expected(self, variant):
        """per task: the integers of its blocks"""
        return [task.partials(REDUCE_LANES[variant] << self.lane_log2) for task in self.tasks]


def reduce_valid(case, variant, partial_stride, num_buckets=None, num_heads=None):
    """the harness's rules for a k_reduce launch (tests/native/tail_hooks.hip), re-stated"""
    num_buckets = case.num_buckets if num_buckets is None else num_buckets
    num_heads = case.num_heads if num_heads is None else num_heads
    if variant not in REDUCE_LANES or case.lane_log2 > 6 or not case.params or partial_stride < 1:
        return False
    bucket_ranges, segment_ranges = [], []
    for nb, seg_log2, bb, sb in case.params:
        if nb < 1 or not 3 <= seg_log2 <= 7 or bb + nb > num_buckets:
            return False
        ends = case.ends[bb:bb + nb].astype(np.int64)
        if np.any(np.diff(ends) < 0):
            return False
        segments = (int(ends[-1]) >> seg_log2) + 2
        if sb + segments > num_heads:
            return False
        per = REDUCE_LANES[variant] << case.lane_log2
        if (nb + per - 1) // per > partial_stride:
            return False
        bucket_ranges.append((bb, bb + nb))
        segment_ranges.append((sb, sb + segments))
    return disjoint(bucket_ranges) and disjoint(segment_ranges)


def disjoint(ranges):
    ranges = sorted(ranges)
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


def long_bucket_end(begin, heads, seg_log2, on_boundary):
    """the smallest end (on / off a segment boundary) for which [begin, end) has exactly `heads` heads"""
    first = begin >> seg_log2
    for nseg in range(max(0, 64 * (heads - 3)), 64 * (heads + 3)):
        end = ((first + nseg) << seg_log2) + (0 if on_boundary else 5)
        if end > begin and len(visited(begin, end, seg_log2)) == heads:
            return end
    raise AssertionError((begin, heads, seg_log2, on_boundary))


def long_bucket_task(heads, seg_log2, position, first, begin_off, end_on, salt):
    """16 buckets; bucket `position` starts in segment `first` (+ begin_off entries) and has `heads` heads"""
    nb = 16
    begin = 0 if position == 0 else (first << seg_log2) + begin_off
    if heads == 0:
        end = begin + (1 if begin_off else 3)               # inside one segment
        assert (end - 1) >> seg_log2 == begin >> seg_log2
    else:
        end = long_bucket_end(begin, heads, seg_log2, end_on)
    counts = [1] * nb
    counts[position] = end - begin
    if position:
        counts[0] = begin - (position - 1)
    task = Task(counts, seg_log2, salt)
    assert task.bounds(position) == (begin, end) and len(task.heads(position)) == heads
    task.long_bucket = position
    return task


LONG_HEADS = [0, 1, 2, 16, 17, 40, 300]


def long_bucket_tasks(seg_log2):
    out = []
    for i, h in enumerate(LONG_HEADS):
        # bucket 0 | a middle bucket, first + 1 = 63 mod 64, begin on a boundary | the last bucket of the
        # block, first + 1 = 0 mod 64, begin off a boundary
        out.append(long_bucket_task(h, seg_log2, 0, 0, 0, i % 2 == 0, 10 * i))
        out.append(long_bucket_task(h, seg_log2, 7, 62, 0, i % 2 == 1, 10 * i + 1))
        out.append(long_bucket_task(h, seg_log2, 15, 63, 3, i % 2 == 0, 10 * i + 2))
    for i, h in enumerate((16, 17)):
        out.append(long_bucket_task(h, seg_log2, 7, 63, 0, True, 100 + i))
        out.append(long_bucket_task(h, seg_log2, 15, 62 + 64, 3, False, 110 + i))
    return out


def heavy_task(num_heavy, salt):
    """100 buckets at two per lane, `num_heavy` of them with 17 .. 19 heads; buckets 4 and 5, and 90 and
    91, share a lane"""
    rng = random.Random(salt)
    at = [4, 5, 20, 33, 47, 60, 71, 90, 91, 80, 95, 99][:num_heavy]
    counts = [rng.choice([0, 1, 1, 2, 3]) for _ in range(100)]
    for j, b in enumerate(at):
        counts[b] = ((16 + j % 3) * 64 + 7 * j + 70) * 8 + j
    task = Task(counts, 3, salt)
    task.heavy = [b for b in range(100) if len(task.heads(b)) > HEAVY_HEADS]
    assert sorted(at) == task.heavy
    return task


def sparse_task(nb, populated, seg_log2=3, salt=0):
    counts = np.zeros(nb, np.int64)
    for i, b in enumerate(populated):
        counts[b] = 1 + i % 3
    return Task(counts, seg_log2, salt)


def algebra_tasks():
    """600 buckets at eight per lane: two 64-lane blocks, one 256-lane block"""
    nb = 600
    same = Task([1] * nb, 3, 1)                      # every populated bucket holds the same point
    same.sum_idx[:] = pool_index(5)
    s_zero = sparse_task(nb, [3, 12, 14, 15, 40, 520, 599], salt=2)   # lane 1: s = 3 G, 0, 7 G
    for b, k in ((15, 3), (14, -3), (12, 7)):
        s_zero.set_sum(b, k)
    r_zero = sparse_task(nb, [1, 20, 22, 23, 300, 530], salt=3)       # lane 2: s = 4 G, -4 G; r = 4 G, 0, -4 G ..
    for b, k in ((23, 4), (22, -8), (20, 9)):
        r_zero.set_sum(b, k)
    zero = sparse_task(nb, [0, 2, 49, 99], salt=4)                    # a populated block whose total is 0
    for b, k in ((0, -6), (2, 2), (49, -4), (99, 2)):
        zero.set_sum(b, k)
    assert zero.total_scalar() == 0 and zero.total != 0
    return [same, s_zero, r_zero, zero]


def dense_task(nb, salt):
    rng = random.Random(1000 + nb + salt)
    return Task([rng.randrange(1, 4) for _ in range(nb)], 3, salt)


@functools.lru_cache(None)
def reduce_cases():
    cases = []
    for lane_log2 in (0, 1, 3):
        cases.append(ReduceCase(f"dense_lanes{lane_log2}", lane_log2,
                                [dense_task(nb, lane_log2) for nb in (1, 2, 32, 64, 128, 256, 1024)]))
    nb = 1 << 15
    cases.append(ReduceCase("sparse", 3, [sparse_task(nb, [0, 1, 2047, 2048, nb - 1], salt=5)]))
    nb = 1 << 17
    cases.append(ReduceCase("large_offsets", 6, [sparse_task(
        nb, [0, 5, 4095, 4096, 4097, 8191, 16383, 16384, 16385, 20000, 32767, nb - 16384, nb - 4096, nb - 4095,
             nb - 70, nb - 1], salt=6)]))
    for seg_log2 in (3, 7):
        cases.append(ReduceCase(f"long_buckets_seg{seg_log2}", 1, long_bucket_tasks(seg_log2)))
    cases.append(ReduceCase("heavy_overflow", 1, [heavy_task(n, 20 + n) for n in (7, 8, 9, 12)]))
    cases.append(ReduceCase("algebra", 3, algebra_tasks()))
    cases.append(ReduceCase("mixed", 0, [dense_task(1024, 7), dense_task(64, 8), Task([0] * 1024, 3, 9)]))
    return cases


def chained_case():
    """three windows of one column at 9 bits (256 buckets), 64-lane blocks of two buckets per lane"""
    tasks = []
    for w in range(3):
        rng = random.Random(70 + w)
        tasks.append(Task([rng.choice([0, 1, 2, 9, 17]) for _ in range(256)], 3, 30 + w))
    return ReduceCase("chained", 1, tasks, variants=(1,))


#--------------------------------------------------------------------------------------------------
# k_horner: columns, launches, model
#--------------------------------------------------------------------------------------------------
HORNER_KINDS = ["plain", "identity_top", "identity_low", "double_top", "double_low", "cancel_top", "cancel_low",
                "all_identity"]      # the placements of tests/device_cases.py


def team_of(lanes, windows):
    team = 1
    while team * 2 * windows <= lanes:
        team *= 2
    return team


def window_sums(rng, windows, bits, kind, zero=()):
    """window scalars for acc = 2^bits acc + w_i from the top window down; `kind` places an identity, the
    running value (the addition is a doubling) or its negative (the chain passes through the identity);
    the windows in `zero` hold nothing"""
    ws = [0 if w in zero else rng.choice(POOL_K) for w in range(windows)]
    if kind == "plain":
        return ws
    if kind == "all_identity":
        return [0] * windows
    top = windows - 1
    at = top if kind.endswith("top") else 0
    assert at not in zero
    running = 0
    for i in range(top, -1, -1):
        running <<= bits
        if i == at:
            ws[i] = 0 if kind.startswith("identity") else (running or 5) * (1 if kind.startswith("double") else -1)
        running += ws[i]
    return ws


class Column:
    """`windows` tasks; the window sums are dealt out over the blocks of each task's partials.
    `zero`: windows without entries (task_total 0, identity partials, as k_reduce leaves them)"""

    def __init__(self, rng, windows, bits, blocks, kind="plain", zero=()):
        self.windows, self.bits, self.blocks, self.kind, self.zero = windows, bits, blocks, kind, set(zero)
        self.sums = window_sums(rng, windows, bits, kind, self.zero)
        self.block_scalars = []
        for w in range(windows):
            if w in self.zero:
                self.block_scalars.append([0] * blocks)
                continue
            ks = [rng.choice(POOL_K) for _ in range(blocks)]
            at = rng.randrange(blocks)
            ks[at] += self.sums[w] - sum(ks)
            self.block_scalars.append(ks)
        self.totals = [0 if w in self.zero else 1 + (7 * w) % 5 for w in range(windows)]

    def value(self, lo=0, hi=None, acc=0):
        """the chain over windows [lo, hi) from `acc`"""
        for w in reversed(range(lo, self.windows if hi is None else hi)):
            acc = (acc << self.bits) + self.sums[w]
        return acc


HORNER_WINDOWS = {64: [1, 2, 3, 17, 32, 33, 64], 256: [1, 2, 3, 17, 32, 33, 64, 65, 128, 256]}
WINDOW_BITS = {1: 16, 2: 2, 3: 9, 17: 16, 32: 9, 33: 1, 64: 9, 65: 2, 128: 2, 256: 1}
HORNER_BLOCK_LOG2 = (6, 9, 14)


def horner_bits(windows, block_log2):
    """at 64 buckets per block 16-bit windows would take 512 partial slots each: 12 bits there"""
    return min(WINDOW_BITS[windows], 12) if block_log2 == 6 else WINDOW_BITS[windows]


class HornerCase:
    """one launch: columns of different first_task, window_bits and num_tasks"""

    def __init__(self, lanes, block_log2, salt=0):
        self.lanes, self.block_log2 = lanes, block_log2
        self.name = f"T{lanes}_block{block_log2}"
        rng = random.Random(lanes + 31 * block_log2 + salt)
        blocks = lambda bits: ((1 << (bits - 1)) + (1 << block_log2) - 1) >> block_log2  # noqa: E731
        specs = [(w, HORNER_KINDS[(i + block_log2) % 8], ()) for i, w in enumerate(HORNER_WINDOWS[lanes])]
        # windows without entries: the top 1 .. W, all of them, one in the middle
        specs += [(17, "plain", [16]), (17, "plain", range(12, 17)), (17, "plain", range(17)), (17, "plain", [8]),
                  (3, "plain", [1, 2]), (2, "plain", [0, 1]), (3, "double_low", [2]), (17, "cancel_low", [15, 16])]
        self.columns = [Column(rng, w, horner_bits(w, block_log2), blocks(horner_bits(w, block_log2)), kind, zero)
                        for w, kind, zero in specs]
        self.partial_stride = max(c.blocks for c in self.columns) + 1
        # tasks in a shuffled column order, with unowned tasks in between
        order = list(range(len(self.columns)))
        rng.shuffle(order)
        at, self.first_task = 1, [0] * len(self.columns)
        for c in order:
            self.first_task[c] = at
            at += self.columns[c].windows + (c % 2)
        self.num_tasks = at

    def params(self):
        return [(ft, c.bits, c.windows) for ft, c in zip(self.first_task, self.columns)]

    def task_total(self):
        tt = np.full(self.num_tasks, 3, np.uint32)
        for ft, c in zip(self.first_task, self.columns):
            tt[ft:ft + c.windows] = c.totals
        return tt

    def partial_scalars(self):
        """(task, slot) -> integer, for the slots the columns own; every other slot is garbage"""
        out = {}
        for ft, c in zip(self.first_task, self.columns):
            for w in range(c.windows):
                for blk, k in enumerate(c.block_scalars[w]):
                    out[(ft + w, blk)] = k
        return out

    def geometry(self):
        """(team, blocks) per column"""
        return [(team_of(self.lanes, c.windows), c.blocks) for c in self.columns]


def horner_valid(lanes, params, num_tasks, partial_stride, block_log2, null=False, first=1, last=1):
    """the harness's rules for a k_horner launch, re-stated"""
    if lanes not in (64, 256) or not params or partial_stride < 1 or not 6 <= block_log2 <= 14:
        return False
    if null and (num_tasks != 0 or first != 1 or last != 1):
        return False
    ranges = []
    for first_task, bits, windows in params:
        if not 1 <= bits <= 21 or windows > lanes or first_task + windows > num_tasks:
            return False
        if windows and (((1 << (bits - 1)) + (1 << block_log2) - 1) >> block_log2) > partial_stride:
            return False
        if windows:
            ranges.append((first_task, first_task + windows))
    return disjoint(ranges)


@functools.lru_cache(None)
def horner_cases():
    return [HornerCase(lanes, block_log2) for lanes in (64, 256) for block_log2 in HORNER_BLOCK_LOG2]


HORNER_SPLITS = (1, 5, 16)     # 16: inside the trimmed top of the columns whose top windows are empty
assert FAMILIES == ["ed", "bn254", "grumpkin", "bls12_381"]
