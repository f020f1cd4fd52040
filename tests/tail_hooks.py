"""ctypes view of tests/native/_build/libbz_tail_hooks.so: k_reduce, k_reduce_compact and k_horner of
msm/kernels.h as msm/engine.h launches them (tests/native/tail_hooks.hip), so GPU tests can run the
tails of an MSM alone, on plain arrays of points and offsets.  The sibling of tests/device_hooks.py,
built the same way: one object per curve family, compiled with the flags of the product translation
unit that instantiates the tails, taken from blitzar_amd.build (never copied):

    tag              built like                                  holds
    ed_tails         msm/msm_curve25519.hip                      k_reduce<C, Scan, 256 / 64>, k_reduce_compact<C>,
    <curve>_tails    msm/msm_<curve>.hip                         k_horner<C, 256 / 64>, heads_of per lane

The entry points, not Python, build task_desc and column_desc from scalar parameters and refuse (-3)
every range a kernel would index past, before anything is launched.

BZ_TAIL_HOOKS_LIB=<path> loads another build of the library instead (build(root=<modified copy of the
headers>, out=...): how one shows that the tests notice a wrong kernel)."""
import concurrent.futures
import ctypes
import os
import subprocess

import numpy as np

from tests.device_hooks import CURVES, ROOT, HarnessError

SRC = os.path.join(ROOT, "tests", "native", "tail_hooks.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build")
LIB = os.path.join(OUT, "libbz_tail_hooks.so")
ENV = "BZ_TAIL_HOOKS_LIB"


def objects():
    """tag -> (product translation unit whose flags it takes, defines); the longest compile first"""
    objs = {}
    for name, (trait, _) in reversed(CURVES.items()):
        bls = ["-DBZ_DH_SW_BLS=1"] if name == "bls12_381" else []
        objs[name + "_tails"] = (f"msm/msm_{name}.hip", [f"-DBZ_DH_C={trait}"] + bls)
    objs["ed_tails"] = ("msm/msm_curve25519.hip", ["-DBZ_DH_C=ed25519_msm"])
    return objs


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
    lib = os.path.join(out, "libbz_tail_hooks.so")
    if root == ROOT and not force and os.path.exists(lib) and os.path.getmtime(lib) >= _newest_input():
        return lib
    os.makedirs(out, exist_ok=True)
    flags = [f for f in bz_build.FLAGS if not f.startswith("-I")] + ["-I" + root]

    def job(item):
        tag, (tu, defs) = item
        assert tu in bz_build.SOURCES, tu
        obj = os.path.join(out, f"tail_hooks_{tag}.o")
        subprocess.run([bz_build.HIPCC, *flags, *bz_build.TU_FLAGS.get(tu, []), f"-DBZ_DH_TAG={tag}",
                        *defs, "-c", SRC, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:  # (four objects)
        objs = list(ex.map(job, objects().items()))
    subprocess.run([bz_build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    if verbose:
        print(f"[tail_hooks] built {lib}")
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


# `fam` below is "ed" or a key of CURVES
SENTINEL = 0xA5A5A5A5      # what every output word holds before a launch: "not written" is observable
REDUCE_VARIANTS = {0: ("k_reduce<C, true>", 256), 1: ("k_reduce<C, true, 64>", 64), 2: ("k_reduce<C, false>", 256),
                   3: ("k_reduce<C, false, 64>", 64), 4: ("k_reduce_compact<C>", 256)}
HEADS_RETURNED = 24
_U32P, _U8P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)


def _tail_fn(name, fam, argtypes, restype=ctypes.c_int):
    fn = getattr(lib(), f"bz_dh_{name}_{fam}_tails")
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def _tail_status(what, rc):
    if rc != 0:
        raise HarnessError(f"{what}: {'parameters out of range' if rc == -3 else 'HIP error %d' % rc}")


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a, kind=_U32P):
    return None if a is None else a.ctypes.data_as(kind)


def tail_sizes(fam):
    """(words of a point, bytes of an encoded output, bytes of a projective output, Scan = false is launched)"""
    s = np.zeros(4, np.uint32)
    _tail_fn("tail_sizes", fam, [_U32P], None)(_ptr(s))
    return int(s[0]), int(s[1]), int(s[2]), bool(s[3])


def reduce_variants(fam):
    return [v for v in REDUCE_VARIANTS if v not in (2, 3) or tail_sizes(fam)[3]]


def reduce(fam, variant, lane_log2, tasks, bucket_end, bucket_sums, heads, partial_stride):
    """tasks: (num_buckets, segment_log2, bucket_base, segment_base) each; bucket_sums (buckets, words),
    heads (segments, words) -> partials (tasks, partial_stride, words), task_total (tasks,)"""
    words = tail_sizes(fam)[0]
    tp, ends, sums, hd = _u32(tasks).reshape(-1, 4), _u32(bucket_end), _u32(bucket_sums), _u32(heads)
    assert sums.shape == (ends.size, words) and hd.ndim == 2 and hd.shape[1] == words
    partials = np.full((len(tp), max(int(partial_stride), 1), words), SENTINEL, np.uint32)
    total = np.full(len(tp), SENTINEL, np.uint32)
    fn = _tail_fn("reduce", fam, [ctypes.c_uint32] * 3 + [_U32P] * 3 + [ctypes.c_uint64, _U32P, ctypes.c_uint64,
                                                                     ctypes.c_uint32, _U32P, _U32P])
    rc = fn(variant, lane_log2, len(tp), _ptr(tp), _ptr(ends), _ptr(sums), ends.size, _ptr(hd), hd.shape[0],
            partial_stride, _ptr(partials), _ptr(total))
    _tail_status(f"{fam}/reduce variant {variant}", rc)
    return partials, total


def horner(fam, lanes, columns, partials, partial_stride, task_total, w_lo, w_hi, first, last, projective_out,
           reduce_block_log2, state=None):
    """columns: (first_task, window_bits, num_tasks) each; partials (tasks, partial_stride, words) or None
    for the engine's launch without tasks -> out (columns, bytes), state (columns, words)"""
    words, out_bytes, proj_bytes, _ = tail_sizes(fam)
    cp = _u32(columns).reshape(-1, 3)
    out = np.full((len(cp), proj_bytes if projective_out else out_bytes), SENTINEL & 0xff, np.uint8)
    st = np.full((len(cp), words), SENTINEL, np.uint32) if state is None else _u32(state).copy()
    assert st.shape == (len(cp), words)
    if partials is None:
        pt, tt, num_partials, num_tasks = None, None, 0, 0
    else:
        pt, tt = _u32(partials), _u32(task_total)
        assert pt.ndim == 3 and pt.shape[2] == words and pt.shape[0] == tt.size
        num_partials, num_tasks = pt.shape[0] * pt.shape[1], tt.size
    fn = _tail_fn("horner", fam, [ctypes.c_uint32] * 2 + [_U32P] * 2 + [ctypes.c_uint64, ctypes.c_uint32, _U32P]
                  + [ctypes.c_uint32] * 7 + [_U32P, _U8P])
    rc = fn(lanes, len(cp), _ptr(cp), _ptr(pt), num_partials, partial_stride, _ptr(tt), num_tasks, w_lo, w_hi,
            first, last, projective_out, reduce_block_log2, _ptr(st), _ptr(out, _U8P))
    _tail_status(f"{fam}/horner T = {lanes}", rc)
    return out, st


def heads_of(fam, triples):
    """(lanes, 3) of begin, end, segment_log2 -> (lanes, 1 + 24): count, index(j) for j < min(count, 24)"""
    t = _u32(triples).reshape(-1, 3)
    out = np.full((len(t), 1 + HEADS_RETURNED), SENTINEL, np.uint32)
    rc = _tail_fn("heads_of", fam, [_U32P, ctypes.c_uint32, _U32P])(_ptr(t), len(t), _ptr(out))
    _tail_status(f"{fam}/heads_of", rc)
    return out


def assert_tail_rejections(fam):
    """what the tails objects refuse on the host, before anything is launched: every range a kernel
    would index with, against the arrays supplied"""
    words = tail_sizes(fam)[0]
    pts = lambda n: np.zeros((n, words), np.uint32)  # noqa: E731

    def refused(fn, *args):
        try:
            fn(fam, *args)
        except HarnessError as e:
            assert "parameters out of range" in str(e), str(e)
        else:
            raise AssertionError(f"{fam}/{fn.__name__} accepted {args[:3]}")

    ends = [1, 2, 2, 9]                                   # 4 buckets, 9 entries: 1 + 2 head slots at 2^3
    ok = dict(variant=0, lane_log2=0, tasks=[(4, 3, 0, 0)], ends=ends, sums=4, heads=3, stride=1)

    def reduce_refused(**change):
        a = {**ok, **change}
        refused(reduce, a["variant"], a["lane_log2"], a["tasks"], a["ends"], pts(a["sums"]), pts(a["heads"]),
                a["stride"])

    reduce_refused(ends=[1, 2, 1, 9])                     # bucket_end not non-decreasing
    reduce_refused(heads=2)                               # (total >> segment_log2) + 2 head slots
    reduce_refused(tasks=[(4, 3, 0, 1)])                  # ... from segment_base on
    reduce_refused(tasks=[(5, 3, 0, 0)])                  # buckets past the array
    reduce_refused(tasks=[(3, 3, 2, 0)])
    reduce_refused(tasks=[(2, 3, 0, 0), (3, 3, 1, 1)], heads=8)    # bucket ranges overlap
    reduce_refused(tasks=[(2, 3, 0, 0), (2, 3, 2, 1)], heads=8)    # segment ranges overlap
    reduce_refused(lane_log2=7)
    for seg in (2, 8):
        reduce_refused(tasks=[(4, seg, 0, 0)], heads=8)
    reduce_refused(variant=5)
    if not tail_sizes(fam)[3]:
        reduce_refused(variant=2)                         # never launched for this curve
    reduce_refused(variant=1, tasks=[(65, 3, 0, 0)], ends=list(range(65)), sums=65, heads=10)  # two blocks, a grid of one
    reduce_refused(stride=0)

    col = dict(lanes=64, columns=[(0, 9, 2)], tasks=2, stride=1, total=[1, 1], rb=8, first=1, last=1)

    def horner_refused(null=False, **change):
        a = {**col, **change}
        partials = None if null else np.zeros((a["tasks"], a["stride"], words), np.uint32)
        refused(horner, a["lanes"], a["columns"], partials, a["stride"], a["total"], 0, 0xffffffff, a["first"],
                a["last"], 0, a["rb"])

    horner_refused(lanes=128)
    horner_refused(columns=[(0, 1, 65)], tasks=65, total=[1] * 65)      # W > T
    horner_refused(columns=[(1, 9, 2)])                                 # tasks past the arrays
    horner_refused(columns=[(0, 9, 2), (1, 9, 1)])                      # first_task ranges overlap
    horner_refused(columns=[(0, 10, 2)])                                # two blocks per task, a stride of one
    horner_refused(columns=[(0, 0, 2)])
    horner_refused(rb=5)
    horner_refused(rb=15)
    horner_refused(null=True, columns=[(0, 9, 1)], tasks=0, total=[])   # tasks without partials
    horner_refused(null=True, columns=[(0, 9, 0)], tasks=0, total=[], last=0)

    for triple in ((8, 8, 3), (9, 8, 3), (0, 8, 2), (0, 8, 8)):
        refused(heads_of, [triple])
