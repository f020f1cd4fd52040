"""ctypes view of tests/native/_build/libbz_front_hooks.so: the front of a variable-base MSM -- the three
recode kernels and the two-pass bucket sort of msm/kernels.h, planned by msm/plan.h and launched as
msm/engine.h launches them (tests/native/front_hooks.hip) -- so GPU tests can look at every array the
front hands on, not only at the commitment bytes.  The sibling of tests/tail_hooks.py, built the same
way.  The front kernels depend on the digit type only, so there is ONE object, compiled with the flags
of msm/msm_curve25519.hip, taken from blitzar_amd.build (never copied); the other curve translation
units compile the same source with their own scheduling flags and are not covered.

The entry points, not Python, plan the launch, build every descriptor and refuse (-3) what is outside
the kernels' written contract before anything is launched.

BZ_FRONT_HOOKS_LIB=<path> loads another build of the library instead (build(root=<modified copy of the
headers>, out=...): how one shows that the tests notice a wrong kernel).  Mutate VALUES only, so that every
index stays inside its array: a digit within [-2^(c-1), 2^(c-1)] still names a bucket of its task (`t > half` ->
`>=`, `t > 32768u` -> `>=`, the bit shift `8 * (at & 3)`, the negation of signed columns); the sign bit of a
record, the row a record or a sorted entry carries (`row0`, `task.row_base`) and what is stored into
`bucket_end` and `segment_bucket` are read by no kernel of the front as an index; `big_chunks_of` `<=` -> `<`
keeps hist, scatter and both bodies of pass 2 on ONE chunk table.  Not such mutants: the ticket and barrier
code, `group_chunk` / `group_start` values, the ranks of `wave_aggregated_add`, the filler condition of the
merged recode.  (`chunk == 0` -> `chunk == 1` in big_sort_body changes nothing: an oversized group has at
least two chunks and chunk 1 stores the same bucket ends.)"""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np

from tests.device_hooks import ROOT, HarnessError

SRC = os.path.join(ROOT, "tests", "native", "front_hooks.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build")
LIB = os.path.join(OUT, "libbz_front_hooks.so")
ENV = "BZ_FRONT_HOOKS_LIB"
TU = "msm/msm_curve25519.hip"


def _newest_input():
    newest = os.path.getmtime(SRC)
    for d, _, fs in os.walk(os.path.join(ROOT, "blitzar_amd", "csrc")):
        for f in fs:
            if f.endswith(".h"):
                newest = max(newest, os.path.getmtime(os.path.join(d, f)))
    return newest


def build(root=ROOT, out=OUT, force=False, verbose=True):
    """compile the harness against the headers under `root` into `out`; returns the library path"""
    from blitzar_amd import build as bz_build
    lib = os.path.join(out, "libbz_front_hooks.so")
    if root == ROOT and not force and os.path.exists(lib) and os.path.getmtime(lib) >= _newest_input():
        return lib
    os.makedirs(out, exist_ok=True)
    assert TU in bz_build.SOURCES, TU
    flags = [f for f in bz_build.FLAGS if not f.startswith("-I")] + ["-I" + root]
    obj = os.path.join(out, "front_hooks.o")
    subprocess.run([bz_build.HIPCC, *flags, *bz_build.TU_FLAGS.get(TU, []), "-c", SRC, "-o", obj], check=True)
    subprocess.run([bz_build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    if verbose:
        print(f"[front_hooks] built {lib}")
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get(ENV)
        if not path:
            path = LIB
            have_hipcc = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
            if have_hipcc and (not os.path.exists(LIB) or os.path.getmtime(LIB) < _newest_input()):
                build()
        _lib = ctypes.CDLL(path)
    return _lib


SENTINEL = 0xA5A5A5A5      # what every output word holds before a launch: "not written" is observable
RECODERS = {0: "k_recode", 1: "k_recode_rows32_c16", 2: "k_recode_packed", 3: "none"}
_VP = ctypes.c_void_p
PLAN_FIELDS = ("num_tasks", "num_columns", "total_entries", "total_groups", "total_buckets", "total_segments",
               "max_task_groups", "max_task_slices", "max_slice_rows", "max_task_rows", "max_recode_rows",
               "max_rows", "wide_digits", "recoder", "small_tasks", "staged", "stream_limit", "zero_words",
               "zeroed_words", "num_ranges", "workers")
TASK_FIELDS = ("column", "window", "rows", "num_buckets", "num_slices", "slice_rows", "group_bits", "num_groups",
               "segment_log2", "bucket_base", "entry_base", "group_base", "segment_base", "row_base")
COLUMN_FIELDS = ("n", "window_bits", "num_windows", "first_task", "num_tasks", "merged_stride", "offset")


def constants():
    """words of a plan / column / task description, kLocalSortCapacity, kStreamedSortRecords,
    kMaxStagedGroups, kStagedSliceRows, kBigSortBlocks of the headers the library was built from"""
    c = np.zeros(8, np.uint32)
    fn = lib().bz_fh_constants
    fn.restype, fn.argtypes = None, [_VP]
    fn(c.ctypes.data)
    return [int(v) for v in c]


def _status(what, rc):
    if rc != 0:
        raise HarnessError(f"{what}: {'parameters out of range' if rc == -3 else 'HIP error %d' % rc}")


def _named(fields, words):
    return SimpleNamespace(**{k: int(v) for k, v in zip(fields, words)})


def _outputs(plan):
    """the front's arrays, every word the sentinel: sized as engine.h carves them from its arena"""
    full = lambda n: np.full(n, SENTINEL, np.uint32)  # noqa: E731
    entries = plan.total_entries + 8
    digits = np.full(entries, SENTINEL & 0xffff, np.uint16).view(np.int16) if not plan.wide_digits \
        else full(entries).view(np.int32)
    return SimpleNamespace(digits=digits, zeroed=full(plan.zeroed_words), group_start=full(plan.total_groups + 1),
                           group_chunk=full(plan.total_groups + 1), records=full(entries), sorted=full(entries),
                           bucket_end=full(plan.total_buckets + 1), segment_bucket=full(plan.total_segments + 1))


def _output_pointers(o):
    return [a.ctypes.data for a in (o.digits, o.zeroed, o.group_start, o.group_chunk, o.records, o.sorted,
                                    o.bucket_end, o.segment_bucket)]


def _result(plan_words, task_words, out, column_words=None):
    plan = _named(PLAN_FIELDS, plan_words)
    res = SimpleNamespace(plan=plan, tasks=[_named(TASK_FIELDS, w) for w in task_words[:plan.num_tasks]], out=out)
    if column_words is not None:
        res.columns = [_named(COLUMN_FIELDS, w) for w in column_words]
    return res


def front(buffer, columns, stage=3, force_window_bits=0, force_segment_log2=0, partition_group_entries=0,
          window_table=None, force_window_tables=False, stream_mode=0, max_workers=0, plan_only=False):
    """buffer: bytes (numpy uint8); columns: (offset, n, row_stride, bit_offset, bit_width, is_signed,
    generator_offset) each; window_table: (stride, windows, bits) or None.
    -> plan, tasks, columns (named descriptors) and out (the arrays; None with plan_only)"""
    buf = np.ascontiguousarray(buffer, dtype=np.uint8)
    cols = np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1, 7)
    nplan, ncol, ntask = constants()[:3]
    capacity = int(sum((int(c[4]) + 1) // 2 + 1 for c in cols)) + 1
    stride, windows, bits = window_table if window_table is not None else (0, 0, 0)
    fn = lib().bz_fh_front
    fn.restype, fn.argtypes = ctypes.c_int, [_VP] * 14

    def call(only, out):
        params = np.array([len(cols), buf.size, force_window_bits, force_segment_log2, partition_group_entries,
                           stride, windows, bits, 1 if force_window_tables else 0, stage, stream_mode, max_workers,
                           1 if only else 0, capacity], np.uint64)
        plan_words = np.zeros(nplan, np.uint64)
        column_words = np.zeros((len(cols), ncol), np.uint64)
        task_words = np.zeros((capacity, ntask), np.uint64)
        ptrs = _output_pointers(out) if out is not None else [None] * 8
        rc = fn(params.ctypes.data, buf.ctypes.data if buf.size else None, cols.ctypes.data, plan_words.ctypes.data,
                column_words.ctypes.data, task_words.ctypes.data, *ptrs)
        _status("front", rc)
        return _result(plan_words, task_words, out, column_words)

    planned = call(True, None)
    if plan_only:
        return planned
    return call(False, _outputs(planned.plan))


def sort(tasks, digits, segment_log2, wide=False, stage=3, stream_mode=0, max_workers=0, plan_only=False):
    """tasks: (rows, window_bits, group_bits, slice_rows, row_base) each; digits: the stored digits E = -D
    as int32, laid out as the planner lays the tasks out (entry ranges padded to 8, 8 more at the end)
    -> plan, tasks and out as front()"""
    tp = np.ascontiguousarray(tasks, dtype=np.uint64).reshape(-1, 5)
    nplan, _, ntask = constants()[:3]
    fn = lib().bz_fh_sort
    fn.restype, fn.argtypes = ctypes.c_int, [_VP] * 13

    def call(only, out, dig):
        params = np.array([len(tp), segment_log2, 1 if wide else 0, stage, stream_mode, max_workers,
                           1 if only else 0, 0 if dig is None else dig.size], np.uint64)
        plan_words = np.zeros(nplan, np.uint64)
        task_words = np.zeros((len(tp), ntask), np.uint64)
        ptrs = _output_pointers(out) if out is not None else [None] * 8
        rc = fn(params.ctypes.data, tp.ctypes.data, None if dig is None else dig.ctypes.data, plan_words.ctypes.data,
                task_words.ctypes.data, *ptrs)
        _status("sort", rc)
        return _result(plan_words, task_words, out)

    planned = call(True, None, None)
    if plan_only:
        return planned
    dig = np.ascontiguousarray(digits, dtype=np.int32)
    return call(False, _outputs(planned.plan), dig)
