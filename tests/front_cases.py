"""Case tables and the integer model for the front of a variable-base MSM (tests/test_msm_front_device.py
runs them on the GPU through tests/front_hooks.py; tests/test_front_cases.py checks the model and the
cases themselves on the CPU).  Written from the comments of msm/kernels.h and msm/plan.h, in plain
Python integers and numpy; msm/recode.h is not called.

    digits     unsigned field value x, c-bit windows u_w, t = u_w + carry: t > 2^(c-1) gives D = t - 2^c and
               a carry, otherwise D = t; signed columns recode |x| and negate every digit; stored E = -D
    layout     separate windows: digits[task(first + w).entry_base + row]; merged (window tables):
               entry_base + w * stride + row, zero filler for rows n..stride of every slice but the last
    record     sign << 31 | (bucket mod 2^s) << (31 - s) | row, bucket = |E| - 1, sign set when E > 0
    sorted     (row_base + row) | sign << 31, grouped by bucket; bucket_end; segment -> bucket map
"""
from types import SimpleNamespace

import numpy as np

SENTINEL = 0xA5A5A5A5
LOCAL_SORT_CAPACITY = 6144            # kLocalSortCapacity
STREAMED_SORT_RECORDS = 16 * 6144     # kStreamedSortRecords
MAX_STAGED_GROUPS = 1024              # kMaxStagedGroups
STAGED_SLICE_ROWS = 1 << 14           # kStagedSliceRows
DIRECT_SLICE_ROWS = 1 << 16           # kDirectSliceRows
GROUP_TARGET_ENTRIES = 4096           # kGroupTargetEntries
MAX_GROUP_BITS = 10                   # kMaxGroupBits
MAX_GROUPS_LOG2 = 10                  # kMaxGroupsLog2
PRIME = (1 << 61) - 1                 # the closing identity's modulus


#--------------------------------------------------------------------------------------------------
# digits
#--------------------------------------------------------------------------------------------------
def field_bits(buffer, offset, n, row_stride, bit_offset, bit_width):
    """(n, bit_width) matrix of the little-endian bit fields of a column's rows"""
    nbytes = (bit_offset + bit_width + 7) // 8
    idx = offset + np.arange(n, dtype=np.int64)[:, None] * row_stride + np.arange(nbytes, dtype=np.int64)[None, :]
    rows = np.asarray(buffer, np.uint8)[idx]
    return np.unpackbits(rows, axis=1, bitorder="little")[:, bit_offset:bit_offset + bit_width]


def bits_to_ints(bits):
    """rows of little-endian bits -> Python integers"""
    packed = np.packbits(bits, axis=1, bitorder="little")
    return [int.from_bytes(r.tobytes(), "little") for r in packed]


def column_values(buffer, col):
    """the column's scalars as (signed) Python integers"""
    bits = field_bits(buffer, col.offset, col.n, col.row_stride, col.bit_offset, col.bit_width)
    vals = bits_to_ints(bits)
    if col.is_signed:
        vals = [v - (1 << col.bit_width) if v >> (col.bit_width - 1) else v for v in vals]
    return vals


def digits_of_int(x, c, w):
    """the model on ONE integer (signed: |x| recoded, every digit negated)"""
    mag, carry, out = abs(x), 0, []
    for _ in range(w):
        t = (mag & ((1 << c) - 1)) + carry
        mag >>= c
        d, carry = (t - (1 << c), 1) if t > (1 << (c - 1)) else (t, 0)
        out.append(-d if x < 0 else d)
    assert mag == 0 and carry == 0, "W * c >= bit_width + 1: the top digit never carries"
    return out


def recode_bits(bits, is_signed, c, w):
    """the same walk on a whole column at once: (w, n) int64 digits D"""
    n, width = bits.shape
    bits = bits.astype(np.uint8)
    negative = np.zeros(n, bool)
    if is_signed:
        negative = bits[:, width - 1] == 1
        # |x| = 2^width - x: the bits up to and including the lowest set one stay, those above flip
        first = np.argmax(bits, axis=1)
        flipped = np.where(np.arange(width)[None, :] <= first[:, None], bits, 1 - bits)
        bits = np.where(negative[:, None], flipped, bits)
    padded = np.zeros((n, w * c), np.uint8)
    padded[:, :min(width, w * c)] = bits[:, :w * c]
    assert width <= w * c
    out = np.zeros((w, n), np.int64)
    carry = np.zeros(n, np.int64)
    half = 1 << (c - 1)
    weights = np.int64(1) << np.arange(c, dtype=np.int64)
    for k in range(w):
        t = padded[:, k * c:(k + 1) * c].astype(np.int64) @ weights + carry
        over = t > half
        out[k] = np.where(over, t - (1 << c), t)
        carry = over.astype(np.int64)
    assert not carry.any()
    return np.where(negative[None, :], -out, out)


def digits_value(D, c):
    """sum_w D_w 2^(c w) per row, as Python integers (object array)"""
    total = np.zeros(D.shape[1], object)
    for k in range(D.shape[0]):
        total = total + (D[k].astype(object) << (c * k))
    return total


#--------------------------------------------------------------------------------------------------
# the planner's geometry, restated (checked against the host hook of plan.h by tests/test_front_cases.py)
#--------------------------------------------------------------------------------------------------
def choose_window_bits(n, bits, max_window_bits=16, force=0, bucket_cost=2.5, task_cost=0.0):
    cmax = min(max_window_bits, bits + 1)
    if force:
        return max(2, min(force, cmax))
    best, best_cost = 1, 1e300
    for c in range(2, cmax + 1):
        cost = float(-(-(bits + 1) // c)) * (float(n) + bucket_cost * float(1 << (c - 1)) + task_cost)
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def choose_segment_log2(total_entries, task_rows):
    s = 5
    while s < 7 and (total_entries >> (s + 1)) >= (1 << 19):
        s += 1
    while s > 3 and (task_rows >> s) < 128:
        s -= 1
    while s > 3 and (total_entries >> s) < (1 << 16):
        s -= 1
    return s


def choose_partition(n, window_bits, target=GROUP_TARGET_ENTRIES):
    """-> (group_bits, num_groups, slice_rows, num_slices)"""
    bucket_bits = window_bits - 1
    row_bits = 0
    while row_bits < 31 and (1 << row_bits) < n:
        row_bits += 1
    desired = 0
    while desired < bucket_bits and ((n << (desired + 1)) >> bucket_bits) <= target:
        desired += 1
    few = max(bucket_bits - MAX_GROUPS_LOG2, 0)
    s = min(max(desired, few), bucket_bits, MAX_GROUP_BITS, 31 - row_bits)
    groups = 1 << (bucket_bits - s)
    slice_rows = STAGED_SLICE_ROWS if groups <= MAX_STAGED_GROUPS else DIRECT_SLICE_ROWS
    return s, groups, slice_rows, -(-n // slice_rows)


def column(offset, n, row_stride, bit_offset, bit_width, is_signed=False, generator_offset=0):
    return SimpleNamespace(offset=offset, n=n, row_stride=row_stride, bit_offset=bit_offset, bit_width=bit_width,
                           is_signed=bool(is_signed), generator_offset=generator_offset)


def column_tuple(col):
    return (col.offset, col.n, col.row_stride, col.bit_offset, col.bit_width, int(col.is_signed),
            col.generator_offset)


def lay_out(task_shapes, segment_log2):
    """task descriptors with the bases laid out as the planner lays them (entry ranges padded to 8);
    task_shapes: (column, window, rows, window_bits, group_bits, slice_rows, row_base) each"""
    tasks, buckets, entries, groups, segments = [], 0, 0, 0, 0
    for col, window, rows, c, s, slice_rows, row_base in task_shapes:
        t = SimpleNamespace(column=col, window=window, rows=rows, num_buckets=1 << (c - 1),
                            num_slices=-(-rows // slice_rows), slice_rows=slice_rows, group_bits=s,
                            num_groups=1 << (c - 1 - s), segment_log2=segment_log2, bucket_base=buckets,
                            entry_base=entries, group_base=groups, segment_base=segments, row_base=row_base)
        buckets += t.num_buckets
        entries += (rows + 7) & ~7
        groups += t.num_groups + 1
        segments += -(-rows // (1 << segment_log2))
        tasks.append(t)
    return tasks, SimpleNamespace(num_tasks=len(tasks), total_buckets=buckets, total_entries=entries,
                                  total_groups=groups, total_segments=segments,
                                  max_task_groups=max(t.num_groups for t in tasks),
                                  max_task_slices=max(t.num_slices for t in tasks),
                                  max_slice_rows=max(t.slice_rows for t in tasks),
                                  max_task_rows=max(t.rows for t in tasks))


def finish_plan(plan, wide_digits=False, stream_mode=0):
    """the engine's rules on a laid-out plan: small_tasks, staged or direct scatter, stream_limit"""
    plan.wide_digits = int(wide_digits)
    plan.small_tasks = int(plan.max_task_groups == 1 and plan.max_task_rows <= LOCAL_SORT_CAPACITY)
    plan.staged = int(plan.max_task_groups <= MAX_STAGED_GROUPS and plan.max_slice_rows <= STAGED_SLICE_ROWS)
    engine = LOCAL_SORT_CAPACITY if plan.total_entries <= (1 << 22) else STREAMED_SORT_RECORDS
    plan.stream_limit = (engine, LOCAL_SORT_CAPACITY, STREAMED_SORT_RECORDS)[stream_mode]
    plan.zero_words = plan.total_groups + 1 + plan.num_tasks + 2
    plan.zeroed_words = plan.total_groups + 1 + plan.num_tasks + 1 + 1 + plan.num_tasks
    return plan


def plan_columns(cols, force_window_bits=0, force_segment_log2=0, partition_group_entries=0, window_table=None,
                 force_window_tables=False, stream_mode=0):
    """make_msm_plan for the tuning the harness exposes -> (column descriptors, tasks, plan)"""
    nonempty = sum(1 for c in cols if c.n)
    throughput = nonempty >= 4
    bucket_cost, task_cost = (3.5, 800.0) if throughput else (2.5, 0.0)
    max_bits = 15 if any(c.is_signed for c in cols) else 16
    target = partition_group_entries or GROUP_TARGET_ENTRIES

    def shape(c):
        merged = False
        if window_table is not None and window_table[1] and not c.is_signed and c.n:
            stride, windows, bits = window_table
            w = -(-(c.bit_width + 1) // bits)
            fits = c.generator_offset + c.n <= stride and 2 * c.n >= stride and 1 < w <= windows
            assert not fits or force_window_tables, "the model restates forced tables only"
            merged = fits
        cb = window_table[2] if merged else choose_window_bits(c.n, c.bit_width, max_bits, force_window_bits,
                                                               bucket_cost, task_cost)
        w = -(-(c.bit_width + 1) // cb)
        return merged, cb, w, ((w - 1) * window_table[0] + c.n) if merged else c.n

    shapes = [shape(c) if c.n else None for c in cols]
    entries = sum(sh[3] * (1 if sh[0] else sh[2]) for sh in shapes if sh)
    squares = sum(float(sh[3]) * float(sh[3]) * float(1 if sh[0] else sh[2]) for sh in shapes if sh)
    seg = force_segment_log2 or choose_segment_log2(entries, int(squares / float(entries)) if entries else 0)
    descs, task_shapes = [], []
    for ci, (c, sh) in enumerate(zip(cols, shapes)):
        d = SimpleNamespace(n=c.n, window_bits=1, num_windows=0, first_task=len(task_shapes), num_tasks=0,
                            merged_stride=0, offset=c.offset)
        if sh:
            merged, cb, w, task_rows = sh
            group_entries = target
            if merged and window_table[0] < LOCAL_SORT_CAPACITY - 1024:
                group_entries = min(group_entries, LOCAL_SORT_CAPACITY - window_table[0])
            s, _, slice_rows, _ = choose_partition(task_rows, cb, group_entries)
            d.window_bits, d.num_windows, d.num_tasks = cb, w, 1 if merged else w
            d.merged_stride = window_table[0] if merged else 0
            for wi in range(d.num_tasks):
                task_shapes.append((ci, wi, task_rows, cb, s, slice_rows, c.generator_offset))
        descs.append(d)
    tasks, plan = lay_out(task_shapes, seg)
    wide = any(d.window_bits > 16 for d in descs)
    return descs, tasks, finish_plan(plan, wide, stream_mode)


def expected_recoder(cols, descs, plan):
    """0 k_recode, 1 k_recode_rows32_c16, 2 k_recode_packed: engine.h's choice (bases 16-aligned + offset)"""
    def bytes_of(c):
        return ((c.bit_offset & 7) + c.bit_width + 7) // 8
    packed = len(cols) >= 2
    for i, c in enumerate(cols):
        packed = packed and c.row_stride == cols[0].row_stride and (i == 0 or c.offset >= cols[i - 1].offset) \
            and c.offset - cols[0].offset + bytes_of(c) <= cols[0].row_stride
    if packed:
        return 2
    rows32 = all(c.n == 0 or (c.bit_offset == 0 and c.bit_width == 256 and c.row_stride == 32 and not c.is_signed
                              and d.merged_stride == 0 and d.window_bits == 16 and d.num_windows == 17
                              and c.offset % 16 == 0) for c, d in zip(cols, descs))
    return 1 if rows32 and not plan.wide_digits else 0


#--------------------------------------------------------------------------------------------------
# the model of the front's arrays
#--------------------------------------------------------------------------------------------------
def stored_digits(buffer, cols, descs, tasks, plan):
    """-> (digits array E = -D with SENTINEL where no kernel writes, per-column digit matrices D (w, n))"""
    dtype = np.int32 if plan.wide_digits else np.int16
    filler = np.array([SENTINEL], np.uint32).view(np.int32)[0] if plan.wide_digits \
        else np.array([SENTINEL & 0xffff], np.uint16).view(np.int16)[0]
    digits = np.full(plan.total_entries + 8, filler, dtype)
    per_column = []
    for c, d in zip(cols, descs):
        if c.n == 0:
            per_column.append(np.zeros((0, 0), np.int64))
            continue
        bits = field_bits(buffer, c.offset, c.n, c.row_stride, c.bit_offset, c.bit_width)
        D = recode_bits(bits, c.is_signed, d.window_bits, d.num_windows)
        per_column.append(D)
        for w in range(d.num_windows):
            if d.merged_stride:
                base = tasks[d.first_task].entry_base + w * d.merged_stride
                if w + 1 < d.num_windows:
                    digits[base + c.n:base + d.merged_stride] = 0
            else:
                base = tasks[d.first_task + w].entry_base
            digits[base:base + c.n] = (-D[w]).astype(dtype)
    return digits, per_column


def big_chunks_of(total, stream_limit):
    return np.where(total <= stream_limit, 0, -(-total // LOCAL_SORT_CAPACITY))


def sort_task(task, E, stream_limit):
    """the sort of one task from its stored digits E (the task's rows, int64)"""
    s, G, B = task.group_bits, task.num_groups, task.num_buckets
    rows = np.nonzero(E)[0].astype(np.int64)
    e = E[rows]
    bucket = np.abs(e) - 1
    sign = (e > 0).astype(np.int64)
    assert bucket.size == 0 or bucket.max() < B
    group = bucket >> s
    counts = np.bincount(group, minlength=G).astype(np.int64)
    group_start = np.concatenate(([0], np.cumsum(counts)))
    chunks = big_chunks_of(counts, stream_limit).astype(np.int64)
    group_chunk = np.concatenate(([0], np.cumsum(chunks)))
    records = (sign << 31) | ((bucket & ((1 << s) - 1)) << (31 - s)) | rows
    bucket_end = np.cumsum(np.bincount(bucket, minlength=B).astype(np.int64))
    order = np.argsort(bucket, kind="stable")
    entries = (task.row_base + rows[order]) | (sign[order] << 31)
    sorted_bucket = bucket[order]
    starts = np.arange(0, rows.size, 1 << task.segment_log2)
    return SimpleNamespace(entries=int(rows.size), group_of_record=group, records=records, group_start=group_start,
                           group_chunk=group_chunk, bucket_end=bucket_end, sorted=entries, sorted_bucket=sorted_bucket,
                           segment_bucket=sorted_bucket[starts], oversized=bool(chunks.any()))


def task_digits(digits, task):
    return np.asarray(digits[task.entry_base:task.entry_base + task.rows], np.int64)


def model_front(digits, tasks, plan, stage, workers_passed):
    """every array the front leaves behind, as comparable pieces (see compare_front)"""
    per_task = [sort_task(t, task_digits(digits, t), plan.stream_limit) for t in tasks]
    zeroed = np.full(plan.zeroed_words, SENTINEL, np.int64)
    zeroed[:plan.zero_words] = 0
    big = []
    if stage >= 2 and not plan.small_tasks:
        for i, (t, m) in enumerate(zip(tasks, per_task)):
            zeroed[t.group_base:t.group_base + t.num_groups] = m.group_start[1:]      # cursors, all bumped
            zeroed[plan.total_groups + 1 + i] = t.num_slices                           # arrival tickets
            if m.oversized:
                big.append(i)
        barrier = plan.total_groups + 1 + plan.num_tasks
        zeroed[barrier + 1] = len(big)
        if stage >= 3 and big:
            zeroed[barrier] = min(plan.max_task_groups, workers_passed)
    return SimpleNamespace(tasks=per_task, zeroed=zeroed, big_tasks=sorted(big))


def _keys_by_range(values, ends):
    """values tagged with the index of the range (given by its end offsets) their position falls in, sorted"""
    pos = np.arange(values.size)
    tag = np.searchsorted(ends, pos, side="right").astype(np.uint64)
    return np.sort((tag << np.uint64(32)) | values.astype(np.uint64))


def compare_front(out, tasks, plan, model, stage, what=""):
    """exact comparison of the device's arrays with the model; order inside a group's records and inside a
    bucket is not defined: multisets per group, sets per bucket, nothing looser"""
    def untouched(a, why):
        assert np.all(np.asarray(a).view(np.uint32) == SENTINEL), (what, why)

    barrier = plan.total_groups + 1 + plan.num_tasks
    zeroed = out.zeroed.astype(np.int64)
    listed = int(zeroed[barrier + 1])
    assert listed == len(model.big_tasks), (what, "big_tasks[0]", listed, model.big_tasks)
    assert sorted(zeroed[barrier + 2:barrier + 2 + listed].tolist()) == model.big_tasks, (what, "big_tasks")
    untouched(out.zeroed[barrier + 2 + listed:], "big_tasks past its list")
    assert np.array_equal(zeroed[:barrier + 2], model.zeroed[:barrier + 2]), \
        (what, "cursors, tickets, barrier", np.nonzero(zeroed[:barrier + 2] != model.zeroed[:barrier + 2])[0][:8])
    partitioned = stage >= 2 and not plan.small_tasks
    sorted_too = stage >= 3
    if not partitioned:
        untouched(out.group_start, "group_start")
        untouched(out.group_chunk, "group_chunk")
        untouched(out.records, "records")
    if not sorted_too:
        untouched(out.sorted, "sorted")
        untouched(out.bucket_end, "bucket_end")
        untouched(out.segment_bucket, "segment_bucket")
    end_of = lambda i, field, total: getattr(tasks[i + 1], field) if i + 1 < len(tasks) else total  # noqa: E731
    for i, (t, m) in enumerate(zip(tasks, model.tasks)):
        w = (what, "task", i)
        entry_end = end_of(i, "entry_base", plan.total_entries + 8)
        if partitioned:
            gs = out.group_start[t.group_base:t.group_base + t.num_groups + 1].astype(np.int64)
            assert np.array_equal(gs, m.group_start), w + ("group_start",)
            gc = out.group_chunk[t.group_base:t.group_base + t.num_groups + 1].astype(np.int64)
            assert np.array_equal(gc, m.group_chunk), w + ("group_chunk",)
            got = out.records[t.entry_base:t.entry_base + m.entries]
            order = np.argsort(m.group_of_record, kind="stable")       # the model's records, by group
            assert np.array_equal(_keys_by_range(got, m.group_start[1:]),
                                  _keys_by_range(m.records[order], m.group_start[1:])), w + ("records",)
            untouched(out.records[t.entry_base + m.entries:entry_end], w + ("records past the entries",))
        if sorted_too:
            ends = out.bucket_end[t.bucket_base:t.bucket_base + t.num_buckets].astype(np.int64)
            assert np.array_equal(ends, m.bucket_end), \
                w + ("bucket_end", np.nonzero(ends != m.bucket_end)[0][:8])
            got = out.sorted[t.entry_base:t.entry_base + m.entries]
            assert np.array_equal(_keys_by_range(got, m.bucket_end), _keys_by_range(m.sorted, m.bucket_end)), \
                w + ("sorted",)
            untouched(out.sorted[t.entry_base + m.entries:entry_end], w + ("sorted past the entries",))
            started = m.segment_bucket.size
            seg = out.segment_bucket[t.segment_base:t.segment_base + started].astype(np.int64)
            assert np.array_equal(seg, m.segment_bucket), \
                w + ("segment_bucket", np.nonzero(seg != m.segment_bucket)[0][:8])
            untouched(out.segment_bucket[t.segment_base + started:end_of(i, "segment_base", plan.total_segments + 1)],
                      w + ("segment_bucket past the last started segment",))
    if sorted_too:
        untouched(out.bucket_end[plan.total_buckets:], "bucket_end's spare word")


#--------------------------------------------------------------------------------------------------
# the closing identity: what k_accumulate, k_reduce and k_horner would make of the device's arrays
#--------------------------------------------------------------------------------------------------
def generators(count, seed=61):
    rng = np.random.default_rng(seed)
    return rng.integers(1, PRIME, count, dtype=np.int64)


def commitment_of(sorted_entries, bucket_end, tasks, descs, column_index, gens):
    """sum_w 2^(c w) sum_b (b + 1) sum_{e in b} +-g[row(e)] mod PRIME, from `sorted` and `bucket_end` alone"""
    d = descs[column_index]
    total = 0
    for k in range(d.num_tasks):
        t = tasks[d.first_task + k]
        ends = bucket_end[t.bucket_base:t.bucket_base + t.num_buckets].astype(np.int64)
        e = sorted_entries[t.entry_base:t.entry_base + int(ends[-1])].astype(np.int64)
        bucket = np.searchsorted(ends, np.arange(e.size), side="right")
        row = e & 0x7fffffff
        sign = np.where(e >> 31 != 0, -1, 1)
        # a merged task holds every window of its column: virtual row = window * stride + row
        windows, first = (int(d.num_windows), 0) if d.merged_stride else (1, t.window)
        window = row // d.merged_stride if d.merged_stride else np.zeros(e.size, np.int64)
        if d.merged_stride:
            row = row % d.merged_stride
        g = gens[row]
        # exact sums of the two 31-bit halves per (window, bucket): float64 holds integers below 2^53
        assert e.size < (1 << 21)
        key = window * t.num_buckets + bucket
        size = windows * t.num_buckets
        hi = np.bincount(key, weights=(sign * (g >> 31)).astype(np.float64), minlength=size)
        lo = np.bincount(key, weights=(sign * (g & 0x7fffffff)).astype(np.float64), minlength=size)
        sums = hi.astype(np.int64).astype(object) * (1 << 31) + lo.astype(np.int64).astype(object)
        weight = np.tile(np.arange(1, t.num_buckets + 1).astype(object), windows)
        per_window = (sums * weight).reshape(windows, t.num_buckets).sum(axis=1)
        for wi, v in enumerate(per_window):
            total += int(v) << (d.window_bits * (first + wi))
    return total % PRIME


def commitment_wanted(values, generator_offset, gens):
    return sum(int(x) * int(g) for x, g in zip(values, gens[generator_offset:generator_offset + len(values)])) % PRIME


#--------------------------------------------------------------------------------------------------
# data
#--------------------------------------------------------------------------------------------------
def windows_equal(value, c, bit_width):
    """the field whose every c-bit window holds `value`"""
    x = 0
    for k in range(-(-bit_width // c)):
        x |= value << (c * k)
    return x & ((1 << bit_width) - 1)


def pattern_values(n, bit_width, is_signed, c, rng, shift=0):
    """n field values (unsigned representation): row r takes pattern (r + shift) mod 9 of
    zero, ones, the tie 2^(c-1) in every window, the tie + 1, [signed: -2^(bits-1), -1, 2^(bits-1) - 1], random"""
    full = (1 << bit_width) - 1
    special = [0, full, windows_equal(1 << (c - 1), c, bit_width), windows_equal(((1 << (c - 1)) + 1) & ((1 << c) - 1),
                                                                                  c, bit_width)]
    if is_signed:
        special += [1 << (bit_width - 1), full, (1 << (bit_width - 1)) - 1]
    out = []
    for r in range(n):
        k = (r + shift) % 9
        out.append(special[k] if k < len(special)
                   else int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") & full)
    return out


def put_field(buffer, offset, row_stride, bit_offset, bit_width, values):
    """OR the values into the buffer's rows as little-endian bit fields"""
    nbytes = (bit_offset + bit_width + 7) // 8
    for r, v in enumerate(values):
        at = offset + r * row_stride
        chunk = np.frombuffer((int(v) << bit_offset).to_bytes(nbytes, "little"), np.uint8)
        buffer[at:at + nbytes] |= chunk


def generic_launch(c, seed=1):
    """columns of 1, 2, 4, 8, 16, 31 and 32 bytes, signed and unsigned, of 1 .. 2049 rows and an empty one, the
    32-byte data 8-aligned and at an odd address, generator offsets on some: -> (buffer, columns)"""
    rng = np.random.default_rng(seed)
    lengths = [1, 7, 8, 9, 255, 256, 257, 2049]
    shapes = []
    k = 0
    for nbytes in (1, 2, 4, 8, 16, 31, 32):
        for signed in (False, True):
            if c == 2 and nbytes >= 16 and signed:
                continue        # (128 windows per column: keep the launch small)
            shapes.append((nbytes, signed, lengths[k % len(lengths)], 8))
            k += 3
    shapes.append((32, False, 257, 8))       # 8-aligned: the whole-word load
    shapes.append((32, False, 2049, 1))      # an odd address: the byte-wise load
    shapes.append((4, False, 0, 4))          # an empty column
    shapes.append((32, False, 9, 16))
    cols, at = [], 0
    for i, (nbytes, signed, n, align) in enumerate(shapes):
        at = (at + 15) & ~15
        at += align % 16
        cols.append(column(at, n, nbytes, 0, 8 * nbytes, signed, generator_offset=(0, 5, 1000)[i % 3]))
        at += n * nbytes
    buffer = np.zeros(at + 16, np.uint8)
    max_bits = 15 if any(col.is_signed for col in cols) else 16
    for i, col in enumerate(cols):
        width = choose_window_bits(col.n, col.bit_width, max_bits, c)       # the column's own window width
        put_field(buffer, col.offset, col.row_stride, 0, col.bit_width,
                  pattern_values(col.n, col.bit_width, col.is_signed, width, rng, shift=i))
    return buffer, cols


def rows32_launch(base_offset, seed=2):
    """unsigned 32-byte columns for the c = 16 recoder, at base_offset + multiples of 16"""
    rng = np.random.default_rng(seed)
    cols, at = [], base_offset
    for n in (1, 255, 0, 257, 1000):
        cols.append(column(at, n, 32, 0, 256))
        at += (32 * n + 15) & ~15
    buffer = np.zeros(at + 16, np.uint8)
    for i, col in enumerate(cols):
        vals = []
        for r in range(col.n):
            k = (r + i) % 6
            vals.append([(1 << 256) - 1, windows_equal(0x8000, 16, 256), windows_equal(0x8001, 16, 256), 0][k]
                        if k < 4 else int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little"))
        put_field(buffer, col.offset, 32, 0, 256, vals)
    return buffer, cols


PACKED_WIDTHS = (1, 7, 8, 13, 64, 252, 256)


def packed_launch(rows, row_stride, misalign, c, seed=3, short_column=True):
    """bit fields of common rows: widths 1 .. 256 at bit offsets 0 .. 7, signed mixed in, repeated along the
    row at row_stride 4500 (several tiles); the buffer base misaligned"""
    rng = np.random.default_rng(seed + rows + misalign)
    cols, byte, k = [], 0, 0
    repeats = 1 if row_stride < 2000 else 3
    for rep in range(repeats):
        byte = max(byte, rep * 2100)
        for width in PACKED_WIDTHS:
            bit_offset = k % 8
            signed = k % 3 == 1 and width > 1
            n = max(1, rows - 3) if (short_column and k % 5 == 4) else rows
            cols.append(column(misalign + byte, n, row_stride, bit_offset, width, signed))
            byte += (bit_offset + width + 7) // 8 - (1 if k % 2 else 0)   # (every other field shares a byte)
            k += 1
    assert byte + 1 <= row_stride
    buffer = np.zeros(misalign + rows * row_stride, np.uint8)
    for i, col in enumerate(cols):
        width = choose_window_bits(col.n, col.bit_width, 15, c)             # (signed columns among them)
        put_field(buffer, col.offset, row_stride, col.bit_offset, col.bit_width,
                  pattern_values(col.n, col.bit_width, col.is_signed, width, rng, shift=i))
    # neighbouring fields overlap where they share a byte: the values are whatever the buffer now holds
    return buffer, cols


def table_launch(bits, packed, seed=4):
    """columns for window tables of stride 512: n in {256, 300, 512} of 256 bits (merged), and a narrow one"""
    rng = np.random.default_rng(seed)
    ns = (256, 300, 512)
    if packed:
        row_stride = 100
        cols = [column(32 * i, n, row_stride, 0, 256) for i, n in enumerate(ns)] + [column(96, 300, row_stride, 3, 5)]
        buffer = rng.integers(0, 256, 512 * row_stride, dtype=np.uint8)
    else:
        cols, at = [], 8
        for n in ns:
            cols.append(column(at, n, 32, 0, 256))
            at += 32 * n
        cols.append(column(at, 300, 1, 0, 8))
        at += 300
        buffer = rng.integers(0, 256, at, dtype=np.uint8)
    for col in cols[:3]:        # a few rows of ties and of all ones per merged column
        put_field_over(buffer, col, 0, (1 << 256) - 1)
        put_field_over(buffer, col, 1, windows_equal(1 << (bits - 1), bits, 256))
        put_field_over(buffer, col, col.n - 1, windows_equal((1 << (bits - 1)) + 1, bits, 256))
    windows = -(-257 // bits)
    return buffer, cols, (512, windows, bits)


def put_field_over(buffer, col, row, value):
    at = col.offset + row * col.row_stride
    nbytes = (col.bit_offset + col.bit_width + 7) // 8
    assert col.bit_offset == 0 and col.bit_width % 8 == 0
    buffer[at:at + nbytes] = np.frombuffer(int(value).to_bytes(nbytes, "little"), np.uint8)


def narrow_launch(seed=5):
    """40 narrow columns of 1 .. 4096 rows: every task one bucket group (k_task_sort)"""
    rng = np.random.default_rng(seed)
    cols, at = [], 0
    for i in range(40):
        n = (1, 8, 100, 4096)[i % 4]
        nbytes = (1, 2)[(i // 4) % 2]
        cols.append(column(at, n, nbytes, 0, 8 * nbytes, is_signed=(i % 5 == 0), generator_offset=(i % 3) * 11))
        at += n * nbytes
    return rng.integers(0, 256, at, dtype=np.uint8), cols


def scalars32(n, kind, seed=6):
    """(n, 32) bytes for one 32-byte column: 'uniform', 'equal' (every scalar equal, every digit non-zero),
    'two_in_three' (two rows in three equal), 'one_in_four' (one row in four equal)"""
    rng = np.random.default_rng(seed)
    one = np.frombuffer(b"".join(int(v).to_bytes(2, "little") for v in rng.integers(0x9000, 0xf000, 16)), np.uint8)
    if kind == "equal":
        return np.tile(one, (n, 1))
    data = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if kind == "two_in_three":
        data[1::3] = one
        data[2::3] = one
    elif kind == "one_in_four":
        data[::4] = one
    else:
        assert kind == "uniform"
    return data


#--------------------------------------------------------------------------------------------------
# explicit sort cases (bz_fh_sort): paths the planner cannot reach at small sizes
#--------------------------------------------------------------------------------------------------
def sort_case(name, shapes, digit_fns, segment_log2=5, wide=False, garbage=True, seed=7):
    """shapes: (rows, window_bits, group_bits, slice_rows, row_base) each; digit_fns: per task, rng -> E (rows)"""
    rng = np.random.default_rng(seed)
    tasks, plan = lay_out([(0, i, r, c, s, sl, rb) for i, (r, c, s, sl, rb) in enumerate(shapes)], segment_log2)
    digits = np.zeros(plan.total_entries + 8, np.int32)
    if garbage:    # what lies past a task's rows must be ignored
        digits[:] = rng.integers(-(1 << 11), 1 << 11, digits.size)
    for t, fn in zip(tasks, digit_fns):
        e = np.asarray(fn(rng), np.int64)
        assert e.shape == (t.rows,) and np.abs(e).max(initial=0) <= t.num_buckets
        digits[t.entry_base:t.entry_base + t.rows] = e
    return SimpleNamespace(name=name, shapes=shapes, tasks=tasks, plan=plan, digits=digits, wide=wide,
                           segment_log2=segment_log2)


def uniform_digits(rows, c):
    return lambda rng: rng.integers(-(1 << (c - 1)), (1 << (c - 1)) + 1, rows)


def grouped_digits(counts, group_bits, zeros=0):
    """counts[g] non-zero digits in bucket group g (random buckets and signs inside it), then `zeros` zero
    digits, all shuffled"""
    def make(rng):
        parts = [(rng.integers(0, 1 << group_bits, k) + (g << group_bits) + 1) * rng.choice([-1, 1], k)
                 for g, k in enumerate(counts)]
        e = np.concatenate(parts + [np.zeros(zeros, np.int64)])
        rng.shuffle(e)
        return e
    return make


def periodic_digits(rows, keys):
    """digits periodic in 64 rows: `keys` = (digit, rows per period) each, the rest of the period distinct"""
    def make(rng):
        period = []
        for digit, k in keys:
            period += [digit] * k
        period += [100 + i for i in range(64 - len(period))]
        return np.resize(np.array(period, np.int64), rows)
    return make


def sort_cases():
    S14, S16 = STAGED_SLICE_ROWS, DIRECT_SLICE_ROWS
    cases = []
    for wide in (False, True):
        tag = "i32" if wide else "i16"
        # direct scatter: more than 1024 groups, two slices of 2^16 rows, the loop past the held vectors
        cases.append(sort_case(f"direct_{tag}", [(70000, 12, 0, S16, 3)], [uniform_digits(70000, 12)], wide=wide))
        # staged scatter at exactly 1024 groups and at exactly 1 group; rows no multiple of the vector width
        cases.append(sort_case(f"staged_1024_groups_{tag}", [(16384 + 5, 11, 0, S14, 0)],
                               [uniform_digits(16384 + 5, 11)], wide=wide))
        cases.append(sort_case(f"staged_1_group_{tag}", [(16384 + 5, 11, 10, S14, 7)],
                               [uniform_digits(16384 + 5, 11)], wide=wide))
    # group sizes on both sides of kLocalSortCapacity, and of kStreamedSortRecords
    cases.append(sort_case("groups_6144_6145", [(6144 + 6145 + 3, 12, 10, S14, 0)],
                           [grouped_digits([6144, 6145], 10, zeros=3)]))
    cases.append(sort_case("groups_98304_98305", [(98304 + 98305 + 3, 12, 10, S14, 0)],
                           [grouped_digits([98304, 98305], 10, zeros=3)]))
    # k_task_sort at its bound: 6144 rows, none zero, 1024 buckets
    cases.append(sort_case("task_sort_bound", [(6144, 11, 10, S14, 0), (6144, 11, 10, S14, 9)],
                           [grouped_digits([6144], 10), uniform_digits(6144, 11)]))
    # degenerate tasks: all digits zero beside a full one; one row; the row base at its bound
    cases.append(sort_case("degenerate", [(5000, 12, 10, S14, 0), (7000, 12, 10, S14, 0), (1, 12, 10, S14, 5),
                                          (1, 12, 10, S14, 5), (7001, 12, 10, S14, (1 << 31) - 7001 - 1)],
                           [lambda rng: np.zeros(5000, np.int64), grouped_digits([3500, 3500], 10),
                            lambda rng: np.array([-2048]), lambda rng: np.array([0]), uniform_digits(7001, 12)]))
    # signs: +-D of one magnitude share a bucket; |D| = 2^(c-1) lands in the top bucket
    cases.append(sort_case("signs", [(9000, 12, 10, S14, 0)],
                           [lambda rng: np.resize(np.array([5, -5, 2048, -2048, 1, -1, 1025, -1025, 1024, -1024]),
                                                  9000)]))
    cases.append(sort_case("signs_c16", [(9000, 16, 10, S14, 0)],
                           [lambda rng: np.resize(np.array([-32768, 32767, -32767, 1, -1, 0]), 9000)]))
    # heavy keys for wave_aggregated_add (oversized groups only): 7 and 8 equal keys per 64 rows, and four
    # heavy keys, so three rounds run and then the fallback
    cases.append(sort_case("heavy_7", [(20000, 11, 10, S14, 0), (300, 11, 10, S14, 0)],
                           [periodic_digits(20000, [(3, 7)]), uniform_digits(300, 11)]))
    cases.append(sort_case("heavy_8", [(20000, 11, 10, S14, 0), (300, 11, 10, S14, 0)],
                           [periodic_digits(20000, [(-3, 8)]), uniform_digits(300, 11)]))
    cases.append(sort_case("heavy_four_keys", [(20000, 11, 10, S14, 0), (300, 11, 10, S14, 0)],
                           [periodic_digits(20000, [(3, 16), (-3, 16), (9, 16), (1024, 16)]),
                            uniform_digits(300, 11)]))
    for seg in (3, 4, 5, 6, 7):
        cases.append(sort_case(f"segment_log2_{seg}", [(7000, 11, 9, S14, 2), (6500, 12, 8, S14, 0)],
                               [uniform_digits(7000, 11), grouped_digits([200, 6000, 1, 0, 0, 0, 7, 100], 8, 192)],
                               segment_log2=seg))
    return cases


def sort_commitment_ok(case, out):
    """the closing identity for explicit digits: per task, sum_b (b + 1) sum_e +-g[row(e)] = sum_i D_i g_i"""
    for t in case.tasks:
        gens = generators(t.rows, seed=t.window + 1)
        ends = out.bucket_end[t.bucket_base:t.bucket_base + t.num_buckets].astype(np.int64)
        e = out.sorted[t.entry_base:t.entry_base + int(ends[-1])].astype(np.int64)
        bucket = np.searchsorted(ends, np.arange(e.size), side="right") + 1
        row = (e & 0x7fffffff) - t.row_base
        assert e.size == 0 or (row.min() >= 0 and row.max() < t.rows)
        got = sum(int(b) * int(g) * (-1 if s else 1) for b, g, s in zip(bucket, gens[row], e >> 31)) % PRIME
        D = -case.digits[t.entry_base:t.entry_base + t.rows].astype(np.int64)
        want = sum(int(d) * int(g) for d, g in zip(D, gens)) % PRIME
        if got != want:
            return False
    return True


def model_output(digits, tasks, plan, model, stage):
    """the model's arrays in the shape of the device's (records and entries in the model's own order):
    what compare_front accepts, and what the CPU tests corrupt to see that it refuses"""
    full = lambda n: np.full(n, SENTINEL, np.uint32)  # noqa: E731
    entries = plan.total_entries + 8
    out = SimpleNamespace(digits=digits, zeroed=(model.zeroed & 0xffffffff).astype(np.uint32),
                          group_start=full(plan.total_groups + 1), group_chunk=full(plan.total_groups + 1),
                          records=full(entries), sorted=full(entries), bucket_end=full(plan.total_buckets + 1),
                          segment_bucket=full(plan.total_segments + 1))
    first = plan.total_groups + 1 + plan.num_tasks + 2
    out.zeroed[first:first + len(model.big_tasks)] = model.big_tasks
    for t, m in zip(tasks, model.tasks):
        if stage >= 2 and not plan.small_tasks:
            out.group_start[t.group_base:t.group_base + t.num_groups + 1] = m.group_start
            out.group_chunk[t.group_base:t.group_base + t.num_groups + 1] = m.group_chunk
            order = np.argsort(m.group_of_record, kind="stable")
            out.records[t.entry_base:t.entry_base + m.entries] = m.records[order]
        if stage >= 3:
            out.bucket_end[t.bucket_base:t.bucket_base + t.num_buckets] = m.bucket_end
            out.sorted[t.entry_base:t.entry_base + m.entries] = m.sorted
            out.segment_bucket[t.segment_base:t.segment_base + m.segment_bucket.size] = m.segment_bucket
    return out
