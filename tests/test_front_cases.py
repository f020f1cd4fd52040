"""The integer model and the case tables of the MSM front (tests/front_cases.py), checked on the CPU: the
model's digits against the host build of msm/recode.h, its restatement of the planner's geometry against the
host build of msm/plan.h, the paths every case is meant to reach, and the model's own identities.  The GPU
side is tests/test_msm_front_device.py."""
import numpy as np
import pytest

from tests import front_cases as fc
from tests import hooks


def sample_rows(n):
    return range(n) if n <= 64 else sorted(set(list(range(24)) + list(range(n - 8, n)) + list(range(0, n, 97))))


def check_digits(buffer, cols, descs):
    """model == host recoder == the one-integer walk, and x = sum_w D_w 2^(c w), per column"""
    checked = 0
    for col, d in zip(cols, descs):
        if col.n == 0:
            continue
        bits = fc.field_bits(buffer, col.offset, col.n, col.row_stride, col.bit_offset, col.bit_width)
        D = fc.recode_bits(bits, col.is_signed, d.window_bits, d.num_windows)
        values = fc.column_values(buffer, col)
        assert fc.digits_value(D, d.window_bits).tolist() == values
        assert np.abs(D).max() <= 1 << (d.window_bits - 1)
        for r in sample_rows(col.n):
            at = col.offset + r * col.row_stride
            row = buffer[at:at + (col.bit_offset + col.bit_width + 7) // 8]
            host = hooks.recode(row, col.bit_offset, col.bit_width, col.is_signed, d.window_bits, d.num_windows)
            assert host.tolist() == D[:, r].tolist(), (col, r)
            assert fc.digits_of_int(values[r], d.window_bits, d.num_windows) == D[:, r].tolist(), (col, r)
            checked += 1
    return checked


@pytest.mark.parametrize("c", [2, 9, 15, 16])
def test_generic_launch_digits(c):
    buffer, cols = fc.generic_launch(c)
    descs, tasks, plan = fc.plan_columns(cols, force_window_bits=c)
    assert fc.expected_recoder(cols, descs, plan) == 0 and not plan.wide_digits
    assert {col.n for col in cols} == {0, 1, 7, 8, 9, 255, 256, 257, 2049}
    assert -(-max(col.n for col in cols) // 256) % 8 != 0          # chunks no multiple of 8: the XCD numbering
    aligned = [col.offset % 8 for col in cols if col.bit_width == 256 and col.n]
    assert 0 in aligned and any(a % 2 for a in aligned)            # both load paths of the 32-byte field
    assert max(d.window_bits for d in descs) == min(c, 15)         # signed columns in the launch: c <= 15
    assert check_digits(buffer, cols, descs) > 300
    # the tie t == 2^(c-1) stays positive (no carry), one more goes negative with a carry
    for col, d in zip(cols, descs):
        if col.n >= 9 and not col.is_signed and col.bit_width >= 2 * d.window_bits:
            half = 1 << (d.window_bits - 1)
            assert fc.digits_of_int(fc.windows_equal(half, d.window_bits, d.window_bits * 2), d.window_bits, 3) \
                == [half, half, 0]
            assert fc.digits_of_int(fc.windows_equal(half + 1, d.window_bits, d.window_bits * 2), d.window_bits, 3) \
                == [half + 1 - 2 * half, half + 2 - 2 * half, 1]


def test_generic_launch_unsigned_c16():
    buffer, cols = fc.generic_launch(16)
    cols = [col for col in cols if not col.is_signed]
    descs, tasks, plan = fc.plan_columns(cols, force_window_bits=16)
    assert max(d.window_bits for d in descs) == 16 and fc.expected_recoder(cols, descs, plan) == 0
    assert check_digits(buffer, cols, descs) > 100


def test_rows32_launch():
    for base, recoder in ((0, 1), (8, 0)):
        buffer, cols = fc.rows32_launch(base)
        descs, tasks, plan = fc.plan_columns(cols, force_window_bits=16)
        assert fc.expected_recoder(cols, descs, plan) == recoder
        assert all(d.num_windows == 17 for col, d in zip(cols, descs) if col.n)
        assert check_digits(buffer, cols, descs) > 100
        D = fc.recode_bits(fc.field_bits(buffer, cols[0].offset, 1, 32, 0, 256), False, 16, 17)
        assert D[:, 0].tolist() == [-1] + [0] * 15 + [1]           # 0xffff...: the carry reaches the 17th digit


@pytest.mark.parametrize("row_stride", [100, 4500])
def test_packed_launch(row_stride):
    ranges_seen = set()
    for rows, misalign in ((1, 1), (63, 7), (64, 15), (65, 1), (130, 7)):
        buffer, cols = fc.packed_launch(rows, row_stride, misalign, 13)
        descs, tasks, plan = fc.plan_columns(cols, force_window_bits=13)
        assert fc.expected_recoder(cols, descs, plan) == 2
        ranges = hooks.packed_ranges([col.offset for col in cols], [col.row_stride for col in cols],
                                     [col.bit_offset for col in cols], [col.bit_width for col in cols])
        ranges_seen.add(len(ranges))
        assert {col.bit_offset for col in cols} == set(range(8) if row_stride > 100 else range(7))
        assert check_digits(buffer, cols, descs) > 0
    assert ranges_seen == ({1} if row_stride == 100 else {3})       # 4500 > kPackedTileSpan: several tiles


@pytest.mark.parametrize("bits", [12, 18])
@pytest.mark.parametrize("packed", [False, True])
def test_table_launch(bits, packed):
    buffer, cols, table = fc.table_launch(bits, packed)
    descs, tasks, plan = fc.plan_columns(cols, window_table=table, force_window_tables=True)
    assert fc.expected_recoder(cols, descs, plan) == (2 if packed else 0)
    assert plan.wide_digits == (bits > 16)
    assert [d.merged_stride for d in descs] == [512, 512, 512, 0]
    per, totals = hooks.plan_tables([col.n for col in cols], [col.bit_width for col in cols], [0] * len(cols), 512,
                                    table[1], force=True, bits=bits)
    for d, p, col in zip(descs, per, cols):
        rows = tasks[d.first_task].rows
        assert (d.window_bits, d.num_windows, d.num_tasks, d.merged_stride, rows) == tuple(int(v) for v in p[:5])
    assert (plan.num_tasks, plan.total_buckets, plan.total_entries, plan.max_task_rows) == \
        tuple(int(v) for v in totals[:4])
    assert check_digits(buffer, cols, descs) > 100
    digits, _ = fc.stored_digits(buffer, cols, descs, tasks, plan)
    t = tasks[descs[1].first_task]                                  # n = 300: filler, and nothing past the rows
    piece = digits[t.entry_base:t.entry_base + ((t.rows + 7) & ~7)]
    assert t.rows == (descs[1].num_windows - 1) * 512 + 300
    assert not piece[300:512].any() and not piece[512 + 300:1024].any()
    assert np.all(piece[t.rows:].view(np.uint32 if bits > 16 else np.uint16) == (fc.SENTINEL >> (0 if bits > 16 else 16)))


def against_planner(cols, descs, tasks, plan):
    per, totals = hooks.plan([col.n for col in cols], [col.bit_width for col in cols],
                             [int(col.is_signed) for col in cols],
                             max_window_bits=15 if any(col.is_signed for col in cols) else 16)
    for d, p in zip(descs, per):
        t = tasks[d.first_task] if d.num_windows else None
        mine = (d.window_bits, d.num_windows, t.num_slices if t else 0, d.first_task, t.slice_rows if t else 0,
                t.group_bits if t else 0)
        assert mine == tuple(int(v) for v in p), (mine, p)
    assert (plan.num_tasks, plan.total_buckets, plan.total_entries, plan.total_segments) == \
        tuple(int(v) for v in totals[:4])
    assert plan.total_groups == int(totals[5]) and tasks[0].segment_log2 == int(totals[6])


def test_plan_restated():
    """the model's restatement of make_msm_plan, choose_partition and choose_segment_log2 against the host
    build of plan.h, at the planner's own window widths (the host hook forces none)"""
    buffer, cols = fc.generic_launch(9)
    against_planner(cols, *fc.plan_columns(cols))
    buffer, cols = fc.narrow_launch()
    descs, tasks, plan = fc.plan_columns(cols)
    against_planner(cols, descs, tasks, plan)
    assert plan.small_tasks and plan.max_task_groups == 1 and plan.max_task_rows == 4096
    for n in (1, 5, 4096, 4097, 6144, 20000, 70000, 250000, 1 << 20, (1 << 22) + 3):
        for bits in (8, 64, 256):
            cols = [fc.column(0, n, bits // 8, 0, bits)]
            against_planner(cols, *fc.plan_columns(cols))
    # above 4096 rows the planner gives a one-window task two groups: it never sends k_task_sort more
    for c in range(2, 12):
        assert fc.choose_partition(4096, c)[1] == 1
        assert fc.choose_partition(4097, c)[1] == 2 and fc.choose_partition(6144, c)[1] == 2


def test_sort_paths_of_the_column_cases():
    """the paths the 32-byte column cases are meant to reach"""
    col = [fc.column(0, 20000, 32, 0, 256)]
    descs, tasks, plan = fc.plan_columns(col, force_window_bits=16)
    assert fc.expected_recoder(col, descs, plan) == 1 and plan.num_tasks == 17 and not plan.small_tasks
    assert all((t.num_groups, 1 << t.group_bits, t.num_slices, t.slice_rows) == (32, 1024, 2, 1 << 14) for t in tasks)
    assert plan.staged and plan.stream_limit == fc.LOCAL_SORT_CAPACITY
    for kind, chunks in (("equal", 4), ("two_in_three", 3)):
        buffer = fc.scalars32(20000, kind).reshape(-1)
        digits, _ = fc.stored_digits(buffer, col, descs, tasks, plan)
        for mode, limit in ((1, fc.LOCAL_SORT_CAPACITY), (2, fc.STREAMED_SORT_RECORDS)):
            fc.finish_plan(plan, stream_mode=mode)
            model = fc.model_front(digits, tasks, plan, 3, 8)
            if mode == 1:       # chunked: all 17 tasks oversized
                assert model.big_tasks == list(range(17))
                assert all(int(m.group_chunk[-1]) == chunks for m in model.tasks)
            else:               # streamed by one workgroup: four (three) rounds of kLocalSortCapacity
                assert model.big_tasks == []
                assert all(-(-int(np.diff(m.group_start).max()) // fc.LOCAL_SORT_CAPACITY) == chunks
                           for m in model.tasks)
    # the engine's own switch: above 2^22 entries groups up to 16 x 6144 records are streamed
    col = [fc.column(0, 250000, 32, 0, 256)]
    descs, tasks, plan = fc.plan_columns(col, force_window_bits=16)
    assert plan.total_entries > 1 << 22 and plan.stream_limit == fc.STREAMED_SORT_RECORDS
    assert all((t.num_groups, t.num_slices) == (64, 16) for t in tasks)


def test_sort_cases_reach_their_paths():
    cases = {c.name: c for c in fc.sort_cases()}
    for tag, wide in (("i16", False), ("i32", True)):
        c = cases[f"direct_{tag}"]
        plan = fc.finish_plan(c.plan, wide)
        assert not plan.staged and not plan.small_tasks and plan.max_task_groups == 2048
        assert c.tasks[0].num_slices == 2 and c.tasks[0].slice_rows == 1 << 16
        vector = 4 if wide else 8
        assert 65536 // vector > 1024 * ((1 << 14) // (vector * 1024))     # vectors past the held ones
        for name, groups in ((f"staged_1024_groups_{tag}", 1024), (f"staged_1_group_{tag}", 1)):
            plan = fc.finish_plan(cases[name].plan, wide)
            assert plan.staged and not plan.small_tasks and plan.max_task_groups == groups
            assert cases[name].tasks[0].rows % vector != 0 and cases[name].tasks[0].num_slices == 2
    plan = fc.finish_plan(cases["task_sort_bound"].plan)
    assert plan.small_tasks and plan.max_task_rows == 6144 and cases["task_sort_bound"].tasks[0].num_buckets == 1024
    assert not np.any(cases["task_sort_bound"].digits[:6144] == 0)
    for name, sizes in (("groups_6144_6145", [6144, 6145]), ("groups_98304_98305", [98304, 98305])):
        c = cases[name]
        for mode in (1, 2):
            plan = fc.finish_plan(c.plan, stream_mode=mode)
            m = fc.sort_task(c.tasks[0], fc.task_digits(c.digits, c.tasks[0]), plan.stream_limit)
            assert np.diff(m.group_start).tolist() == sizes
            want = [0 if s <= plan.stream_limit else -(-s // 6144) for s in sizes]
            assert np.diff(m.group_chunk).tolist() == want
    assert np.diff(fc.big_chunks_of(np.array([6144, 6145]), 6144)).tolist() == [2]
    assert fc.big_chunks_of(np.array([98304, 98305]), fc.STREAMED_SORT_RECORDS).tolist() == [0, 17]
    assert {c.segment_log2 for c in cases.values()} == {3, 4, 5, 6, 7}
    assert {t.group_bits for c in cases.values() for t in c.tasks} >= {0, 10}
    t = cases["degenerate"].tasks[-1]
    assert t.row_base + t.rows == (1 << 31) - 1
    for name, heavy in (("heavy_7", [7]), ("heavy_8", [8]), ("heavy_four_keys", [16, 16, 16, 16])):
        c = cases[name]
        period = c.digits[c.tasks[0].entry_base:c.tasks[0].entry_base + 64]
        assert sorted(k for k in np.unique(period, return_counts=True)[1] if k > 1) == heavy
        assert np.array_equal(period, c.digits[64:128])
        assert fc.finish_plan(c.plan, stream_mode=1).stream_limit < c.tasks[0].rows and not c.plan.small_tasks


SMALL = ("degenerate", "signs", "signs_c16", "groups_6144_6145", "heavy_four_keys", "segment_log2_3",
         "segment_log2_7", "task_sort_bound")


@pytest.mark.parametrize("name", SMALL)
def test_model_identities(name):
    """the model's own arrays pass the comparison, satisfy the closing identity, and stop passing when one
    word is wrong in the way a hand-off error would be"""
    case = {c.name: c for c in fc.sort_cases()}[name]
    plan = fc.finish_plan(case.plan, case.wide, stream_mode=1)
    model = fc.model_front(case.digits, case.tasks, plan, 3, 8)
    out = fc.model_output(case.digits, case.tasks, plan, model, 3)
    fc.compare_front(out, case.tasks, plan, model, 3, name)
    assert fc.sort_commitment_ok(case, out)
    for m, t in zip(model.tasks, case.tasks):
        assert m.group_start[-1] == m.entries == m.bucket_end[-1] == np.count_nonzero(fc.task_digits(case.digits, t))
        assert m.segment_bucket.size == -(-m.entries // (1 << t.segment_log2))
    t, m = next((t, m) for t, m in zip(case.tasks, model.tasks) if m.entries > 1)

    def refused(field, index, value):
        bad = fc.model_output(case.digits, case.tasks, plan, model, 3)
        getattr(bad, field)[index] = value
        with pytest.raises(AssertionError):
            fc.compare_front(bad, case.tasks, plan, model, 3, name)
            assert fc.sort_commitment_ok(case, bad)

    refused("sorted", t.entry_base, int(out.sorted[t.entry_base]) ^ 0x80000000)           # a sign
    refused("sorted", t.entry_base + m.entries, 0)                                         # a slot left alone
    refused("bucket_end", t.bucket_base + int(m.sorted_bucket[0]), int(m.bucket_end[m.sorted_bucket[0]]) - 1)
    refused("segment_bucket", t.segment_base + m.segment_bucket.size - 1, int(m.segment_bucket[-1]) + 1)
    refused("segment_bucket", t.segment_base + m.segment_bucket.size, 0) if \
        m.segment_bucket.size < -(-t.rows // (1 << t.segment_log2)) else None
    if not plan.small_tasks:
        refused("group_chunk", t.group_base + t.num_groups, int(m.group_chunk[-1]) + 1)
        refused("records", t.entry_base, int(out.records[t.entry_base]) ^ 0x80000000)
        refused("zeroed", t.group_base, int(out.zeroed[t.group_base]) + 1)


def test_closing_identity_of_a_column_launch():
    buffer, cols = fc.narrow_launch()
    descs, tasks, plan = fc.plan_columns(cols)
    digits, _ = fc.stored_digits(buffer, cols, descs, tasks, plan)
    model = fc.model_front(digits, tasks, plan, 3, 8)
    out = fc.model_output(digits, tasks, plan, model, 3)
    fc.compare_front(out, tasks, plan, model, 3)
    gens = fc.generators(5000)
    for i, col in enumerate(cols):
        want = fc.commitment_wanted(fc.column_values(buffer, col), col.generator_offset, gens)
        assert fc.commitment_of(out.sorted, out.bucket_end, tasks, descs, i, gens) == want
    buffer, cols, table = fc.table_launch(12, False)
    descs, tasks, plan = fc.plan_columns(cols, window_table=table, force_window_tables=True)
    digits, _ = fc.stored_digits(buffer, cols, descs, tasks, plan)
    model = fc.model_front(digits, tasks, plan, 3, 8)
    out = fc.model_output(digits, tasks, plan, model, 3)
    fc.compare_front(out, tasks, plan, model, 3)
    for i, col in enumerate(cols):
        want = fc.commitment_wanted(fc.column_values(buffer, col), col.generator_offset, gens)
        assert fc.commitment_of(out.sorted, out.bucket_end, tasks, descs, i, gens) == want
