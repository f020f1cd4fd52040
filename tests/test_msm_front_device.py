"""The front of every variable-base MSM, run directly on the GPU: the three recode kernels and the two-pass
bucket sort of msm/kernels.h, planned by msm/plan.h and launched as msm/engine.h launches them
(tests/native/front_hooks.hip), against the integer model of tests/front_cases.py (checked on the CPU by
tests/test_front_cases.py).  Everything is exact: the stored digits, the group tables, the records as
multisets per group, the sorted entries as sets per bucket, every bucket end, the segment -> bucket map, the
final state of the block the recode kernel clears -- and every word no kernel writes still holds the
harness's sentinel.  Each launch ends with the identity the rest of the MSM relies on, computed from the
device's `sorted` and `bucket_end` alone over integer "generators".

Each test prints what it compared (run with -s to see it)."""
import ctypes

import numpy as np
import pytest

from tests import front_cases as fc
from tests import front_hooks as fh
from tests.device_hooks import HarnessError

pytestmark = pytest.mark.gpu

GENS = fc.generators(1 << 18)


@pytest.fixture(scope="module", autouse=True)
def device():
    n = ctypes.c_int(0)      # (the HIP runtime the harness library is linked against)
    assert fh.lib().hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0, "these tests need a GPU"
    local, streamed, staged_groups, staged_rows, big_blocks = fh.constants()[3:]
    assert (local, streamed, staged_groups, staged_rows) == (fc.LOCAL_SORT_CAPACITY, fc.STREAMED_SORT_RECORDS,
                                                             fc.MAX_STAGED_GROUPS, fc.STAGED_SLICE_ROWS)
    assert big_blocks == 128


def same_descriptors(got, want, fields, what):
    for f in fields:
        assert getattr(got, f) == getattr(want, f), (what, f, getattr(got, f), getattr(want, f))


PLAN_CHECKED = ("num_tasks", "total_entries", "total_groups", "total_buckets", "total_segments", "max_task_groups",
                "max_task_slices", "max_slice_rows", "max_task_rows", "wide_digits", "small_tasks", "staged",
                "stream_limit", "zero_words", "zeroed_words")


def check_workers(res, max_workers):
    if res.plan.workers == 0:
        return
    assert 0 < res.plan.workers <= 128
    if max_workers:
        assert res.plan.workers == max_workers


def run_front(name, buffer, cols, stage=3, recoder=None, identity=True, **tuning):
    """one launch through the planner, compared with the model in full -> the harness's result"""
    res = fh.front(buffer, [fc.column_tuple(c) for c in cols], stage=stage, **tuning)
    plan_tuning = {k: v for k, v in tuning.items() if k != "max_workers"}
    descs, tasks, plan = fc.plan_columns(cols, **plan_tuning)
    same_descriptors(res.plan, plan, PLAN_CHECKED, name)
    for i, (got, want) in enumerate(zip(res.tasks, tasks)):
        same_descriptors(got, want, fh.TASK_FIELDS, (name, "task", i))
    for i, (got, want) in enumerate(zip(res.columns, descs)):
        same_descriptors(got, want, fh.COLUMN_FIELDS, (name, "column", i))
    assert res.plan.recoder == fc.expected_recoder(cols, descs, plan), (name, fh.RECODERS[res.plan.recoder])
    if recoder is not None:
        assert fh.RECODERS[res.plan.recoder] == recoder, (name, fh.RECODERS[res.plan.recoder])
    check_workers(res, tuning.get("max_workers", 0))
    digits, per_column = fc.stored_digits(buffer, cols, descs, tasks, plan)
    wrong = np.nonzero(res.out.digits != digits)[0]
    assert wrong.size == 0, (name, "digits (sentinel where nothing is written)", wrong[:8],
                             res.out.digits[wrong[:8]], digits[wrong[:8]])
    model = fc.model_front(digits, tasks, plan, stage, res.plan.workers)
    fc.compare_front(res.out, tasks, plan, model, stage, name)
    if identity:
        for i, (col, d, D) in enumerate(zip(cols, descs, per_column)):
            if col.n == 0:
                continue
            values = fc.column_values(buffer, col)
            assert fc.digits_value(D, d.window_bits).tolist() == values, (name, "x = sum D 2^(cw)", i)
            if stage == 3:
                want = fc.commitment_wanted(values, col.generator_offset, GENS)
                got = fc.commitment_of(res.out.sorted, res.out.bucket_end, tasks, descs, i, GENS)
                assert got == want, (name, "closing identity, column", i)
    print(f"[msm_front] {name}: {fh.RECODERS[res.plan.recoder]}, {plan.num_tasks} tasks, {plan.total_entries} "
          f"entries, stage {stage}, small_tasks {plan.small_tasks}, staged {plan.staged}, "
          f"oversized tasks {len(model.big_tasks)}")
    return res


#--------------------------------------------------------------------------------------------------
# recode
#--------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [2, 9, 15])
def test_recode_generic(c):
    """k_recode<i16>: columns of 1 .. 32 bytes, signed and unsigned, 0 .. 2049 rows (nine chunks: the XCD
    numbering), the 32-byte field through both loads, zero / ones / tie / tie + 1 / signed bounds / random rows,
    generator offsets; at c = 9 through the whole sort"""
    buffer, cols = fc.generic_launch(c)
    run_front(f"generic c={c}", buffer, cols, stage=3 if c == 9 else 1, recoder="k_recode", force_window_bits=c)


def test_recode_generic_c16_unsigned():
    buffer, cols = fc.generic_launch(16)
    cols = [col for col in cols if not col.is_signed]
    res = run_front("generic c=16", buffer, cols, stage=1, recoder="k_recode", force_window_bits=16)
    assert max(c.window_bits for c in res.columns) == 16


def test_recode_rows32_c16():
    """k_recode_rows32_c16 on 16-aligned columns (0xffff...: the carry reaches the 17th digit; halves of 0x8000
    and 0x8001); the same data 8 bytes further falls back to the generic kernel with identical results"""
    buffer, cols = fc.rows32_launch(0)
    fast = run_front("rows32", buffer, cols, recoder="k_recode_rows32_c16", force_window_bits=16)
    shifted, cols8 = fc.rows32_launch(8)
    assert np.array_equal(shifted[8:], buffer)
    slow = run_front("rows32 + 8", shifted, cols8, recoder="k_recode", force_window_bits=16)
    assert np.array_equal(fast.out.digits, slow.out.digits)
    assert np.array_equal(fast.out.bucket_end, slow.out.bucket_end)
    assert np.array_equal(fast.out.segment_bucket, slow.out.segment_bucket)


@pytest.mark.parametrize("row_stride", [100, 4500])
def test_recode_packed(row_stride):
    """k_recode_packed: bit fields of 1 .. 256 bits at bit offsets 0 .. 7 of common rows, signed mixed in, one
    and several tiles per row, 1 .. 130 rows, the buffer base misaligned by 1, 7 and 15"""
    for rows, misalign, c, stage in ((1, 1, 13, 1), (63, 7, 9, 1), (64, 15, 13, 3), (65, 1, 15, 1), (130, 7, 9, 3),
                                     (130, 15, 13, 1)):
        buffer, cols = fc.packed_launch(rows, row_stride, misalign, c)
        res = run_front(f"packed stride={row_stride} rows={rows} +{misalign}", buffer, cols, stage=stage,
                        recoder="k_recode_packed", force_window_bits=c)
        assert res.plan.num_ranges == (1 if row_stride == 100 else 3)


@pytest.mark.parametrize("bits", [12, 18])
@pytest.mark.parametrize("packed", [False, True])
def test_recode_window_tables(bits, packed):
    """merged columns (window tables of stride 512, n = 256, 300, 512) with 16-bit and with 32-bit digits,
    through the generic and the packed recoder: zero filler, nothing past a task's rows"""
    buffer, cols, table = fc.table_launch(bits, packed)
    res = run_front(f"tables bits={bits} packed={packed}", buffer, cols,
                    recoder="k_recode_packed" if packed else "k_recode", window_table=table, force_window_tables=True)
    assert res.plan.wide_digits == (bits > 16) and [c.merged_stride for c in res.columns] == [512, 512, 512, 0]


#--------------------------------------------------------------------------------------------------
# sort, through the planner
#--------------------------------------------------------------------------------------------------
def test_task_sort():
    """k_task_sort: 40 narrow columns of 1, 8, 100 and 4096 rows"""
    buffer, cols = fc.narrow_launch()
    res = run_front("narrow", buffer, cols)
    assert res.plan.small_tasks and res.plan.max_task_rows == 4096


COLUMN = [fc.column(0, 20000, 32, 0, 256)]


def test_sort_uniform():
    """the three-launch path: 32 groups of 1024 buckets, two slices of 2^14 rows"""
    res = run_front("uniform", fc.scalars32(20000, "uniform").reshape(-1), COLUMN, force_window_bits=16)
    assert all((t.num_groups, t.num_slices) == (32, 2) for t in res.tasks)


@pytest.mark.parametrize("kind,max_workers", [("equal", 1), ("equal", 3), ("equal", 0), ("two_in_three", 8)])
def test_sort_chunked(kind, max_workers):
    """every task has an oversized group, cut into chunks for the workers of the in-launch barrier"""
    run_front(f"chunked {kind} workers={max_workers}", fc.scalars32(20000, kind).reshape(-1), COLUMN,
              force_window_bits=16, max_workers=max_workers)


@pytest.mark.parametrize("kind", ["equal", "two_in_three"])
def test_sort_streamed(kind):
    """the same groups streamed by one workgroup each, kLocalSortCapacity records a round"""
    run_front(f"streamed {kind}", fc.scalars32(20000, kind).reshape(-1), COLUMN, force_window_bits=16, stream_mode=2)


def test_sort_engine_switch():
    """4.25 M entries: the engine's own rule streams groups of up to 16 x 6144 records (62500 equal rows here)"""
    col = [fc.column(0, 250000, 32, 0, 256)]
    res = run_front("engine switch", fc.scalars32(250000, "one_in_four").reshape(-1), col, force_window_bits=16)
    assert res.plan.total_entries > 1 << 22 and res.plan.stream_limit == fc.STREAMED_SORT_RECORDS


#--------------------------------------------------------------------------------------------------
# sort, explicit geometry: paths the planner cannot reach at small sizes
#--------------------------------------------------------------------------------------------------
SORT_CASES = {c.name: c for c in fc.sort_cases()}
MODES = {"direct_i16": (0,), "direct_i32": (0,), "task_sort_bound": (0,), "groups_98304_98305": (2,),
         "heavy_7": (1,), "heavy_8": (1,), "heavy_four_keys": (1,)}


@pytest.mark.parametrize("name", list(SORT_CASES))
def test_sort_explicit(name):
    """direct and staged scatter at their group bounds, groups on both sides of the two stream limits,
    k_task_sort at 6144 rows and 1024 buckets, group_bits 0 and 10, segment_log2 3 .. 7, all-zero and one-row
    tasks, signs and the top bucket, the row base at its bound, heavy keys in oversized groups"""
    case = SORT_CASES[name]
    for mode in MODES.get(name, (1, 2)):
        workers = 3 if mode == 1 else 0
        res = fh.sort(case.shapes, case.digits, case.segment_log2, wide=case.wide, stream_mode=mode,
                      max_workers=workers)
        plan = fc.finish_plan(case.plan, case.wide, stream_mode=mode)
        same_descriptors(res.plan, plan, PLAN_CHECKED, name)
        for i, (got, want) in enumerate(zip(res.tasks, case.tasks)):
            same_descriptors(got, want, fh.TASK_FIELDS, (name, "task", i))
        check_workers(res, workers)
        assert res.plan.recoder == 3
        model = fc.model_front(case.digits, case.tasks, plan, 3, res.plan.workers)
        fc.compare_front(res.out, case.tasks, plan, model, 3, (name, mode))
        assert fc.sort_commitment_ok(case, res.out), (name, mode, "closing identity")
        print(f"[msm_front] {name} mode {mode}: small_tasks {plan.small_tasks}, staged {plan.staged}, oversized tasks "
              f"{len(model.big_tasks)}, chunks {[int(m.group_chunk[-1]) for m in model.tasks]}")


def test_partition_alone():
    """stage 2: histogram and scatter without pass 2 -- nothing of pass 2's is written"""
    case = SORT_CASES["segment_log2_5"]
    res = fh.sort(case.shapes, case.digits, 5, stage=2, stream_mode=1)
    plan = fc.finish_plan(case.plan, stream_mode=1)
    fc.compare_front(res.out, case.tasks, plan, fc.model_front(case.digits, case.tasks, plan, 2, res.plan.workers), 2)


def test_rejections():
    """what the harness refuses before anything is launched: the kernels' written contract"""
    S14, S16 = fc.STAGED_SLICE_ROWS, fc.DIRECT_SLICE_ROWS

    def refused(fn, *args, **kw):
        with pytest.raises(HarnessError, match="parameters out of range"):
            fn(*args, **kw)

    ok = np.zeros(1008, np.int32)
    fh.sort([(1000, 12, 10, S14, 0)], ok, 5, plan_only=True)
    refused(fh.sort, [(1000, 12, 11, S14, 0)], ok, 5)                  # group_bits > kMaxGroupBits
    refused(fh.sort, [(1000, 12, 12, S14, 0)], ok, 5)                  # more group bits than bucket bits
    refused(fh.sort, [(1 << 21, 12, 10, S14, 0)], ok, 5)               # rows >= 2^(31 - group_bits)
    refused(fh.sort, [(1000, 12, 10, S14, (1 << 31) - 1000)], ok, 5)   # row_base + rows >= 2^31
    refused(fh.sort, [(1000, 12, 10, S16, 0)], ok, 5)                  # 2^14 wherever groups <= 1024
    refused(fh.sort, [(1000, 12, 10, 1 << 13, 0)], ok, 5)
    refused(fh.sort, [(1000, 17, 10, S14, 0)], ok, 5)                  # 16-bit digits: c <= 16
    for seg in (2, 8):
        refused(fh.sort, [(1000, 12, 10, S14, 0)], ok, seg)
    refused(fh.sort, [(1000, 12, 10, S14, 0)], ok, 5, stream_mode=3)
    refused(fh.sort, [(1000, 12, 10, S14, 0)], ok, 5, max_workers=17)
    refused(fh.sort, [(1000, 12, 10, S14, 0)], ok[:-1], 5)             # digits: total_entries + 8
    bad = ok.copy()
    bad[999] = 2049                                                    # |E| <= 2^(c-1)
    refused(fh.sort, [(1000, 12, 10, S14, 0)], bad, 5)
    bad[999], bad[1000] = -2048, 30000                                 # past the rows: ignored
    fh.sort([(1000, 12, 10, S14, 0)], bad, 5, plan_only=True)
    top = np.zeros(1008, np.int32)
    top[0] = 32768                                                     # E = -D: D = -2^15 does not exist at c = 16
    refused(fh.sort, [(1000, 16, 10, S14, 0)], top, 5)
    buffer = np.zeros(64, np.uint8)
    fh.front(buffer, [(0, 2, 32, 0, 256, 0, 0)], plan_only=True)
    refused(fh.front, buffer, [(0, 3, 32, 0, 256, 0, 0)])              # rows past the buffer
    refused(fh.front, buffer, [(1, 2, 32, 0, 256, 0, 0)])
    refused(fh.front, buffer, [(0, 2, 32, 8, 8, 0, 0)])                # bit offsets 0 .. 7
    refused(fh.front, buffer, [(0, 2, 32, 0, 257, 0, 0)])
    refused(fh.front, buffer, [(0, 2, 32, 0, 256, 0, 0)], force_window_bits=17)
    refused(fh.front, buffer, [(0, 2, 32, 0, 256, 0, 0)], stream_mode=3)
    refused(fh.front, buffer, [(0, 2, 32, 0, 256, 0, 0)], max_workers=17)
    refused(fh.front, buffer, [(0, 2, 32, 0, 256, 0, 0)], stage=4)
    refused(fh.front, buffer, [(0, 0, 32, 0, 256, 0, 0)])              # no task at all
    # a packed launch whose longest column reaches past the buffer with another column's bytes
    refused(fh.front, np.zeros(99, np.uint8), [(0, 10, 10, 0, 8, 0, 0), (5, 2, 10, 0, 40, 0, 0)])
