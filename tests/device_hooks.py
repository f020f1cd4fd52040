"""ctypes view of tests/native/_build/libbz_device_hooks.so: the product's field / curve headers
wrapped in gfx950 kernels (tests/native/device_hooks.hip), so GPU tests can run single primitives --
the lane-spread arithmetic that has no host build, and the device compile of the shared headers --
and compare them with tests/hooks.py, tools/models and tests/refmath.py.  Test infrastructure only;
needs neither torch nor the product library.

One object per (unit, flag set): the harness source is compiled with the flags of the product
translation unit that instantiates the code, taken from blitzar_amd.build (never copied):

    tag              built like                                  holds
    ed               msm/msm_curve25519.hip                      f29, ed29, ed16w, ed25519_msm wave ops
    ed_niels         msm/msm_curve25519_niels_accumulate.hip     f29, the Z = 1 addition forms of ed29
    <curve>          msm/msm_<curve>.hip                         mont29, sw29, sww::wave, add_coop4
    <curve>_acc      msm/msm_<curve>_accumulate.hip              mont29, sw29 (add_mixed_acc's flag set)
    proof            proof/sumcheck_transcript.hip               wave_sponge, Merlin, scalar25, the element
                                                                 conversions, the protocol steps of the provers

BZ_DEVICE_HOOKS_LIB=<path> loads another build of the library instead (a harness compiled from a
modified copy of the headers: how one shows that the tests notice a wrong kernel)."""
import concurrent.futures
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "device_hooks.hip")
OUT = os.path.join(ROOT, "tests", "native", "_build")
LIB = os.path.join(OUT, "libbz_device_hooks.so")
ENV = "BZ_DEVICE_HOOKS_LIB"

CURVES = {"bn254": ("bn254_msm", "bn254_g1_29"), "grumpkin": ("grumpkin_msm", "grumpkin_29"),
          "bls12_381": ("bls12_381_msm", "bls12_381_g1_28")}


def objects():
    """tag -> (product translation unit whose flags it takes, defines)"""
    objs = {"ed": ("msm/msm_curve25519.hip", ["-DBZ_DH_ED=1", "-DBZ_DH_ED_WAVE=1"]),
            "ed_niels": ("msm/msm_curve25519_niels_accumulate.hip", ["-DBZ_DH_ED=1", "-DBZ_DH_ED_NIELS=1"]),
            "proof": ("proof/sumcheck_transcript.hip", ["-DBZ_DH_PROOF=1"])}
    for name, (trait, curve) in CURVES.items():
        defs = [f"-DBZ_DH_SW={trait}", f"-DBZ_DH_G={curve}"]
        if name == "bls12_381":
            defs.append("-DBZ_DH_SW_BLS=1")
        objs[name] = (f"msm/msm_{name}.hip", defs + ["-DBZ_DH_SW_WAVE=1"])
        objs[name + "_acc"] = (f"msm/msm_{name}_accumulate.hip", defs)
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
    lib = os.path.join(out, "libbz_device_hooks.so")
    if root == ROOT and not force and os.path.exists(lib) and os.path.getmtime(lib) >= _newest_input():
        return lib
    os.makedirs(out, exist_ok=True)
    flags = [f for f in bz_build.FLAGS if not f.startswith("-I")] + ["-I" + root]

    def job(item):
        tag, (tu, defs) = item
        assert tu in bz_build.SOURCES, tu
        obj = os.path.join(out, f"device_hooks_{tag}.o")
        subprocess.run([bz_build.HIPCC, *flags, *bz_build.TU_FLAGS.get(tu, []), f"-DBZ_DH_TAG={tag}",
                        *defs, "-c", SRC, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:  # (at most 16 compile jobs)
        objs = list(ex.map(job, objects().items()))
    subprocess.run([bz_build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    if verbose:
        print(f"[device_hooks] built {lib}")
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


class HarnessError(RuntimeError):
    pass


def run(tag, op, inputs, out_words, params=()):
    """inputs: (cases, in_words) uint32 -> (cases, out_words) uint32"""
    a = np.ascontiguousarray(inputs, dtype=np.uint32)
    assert a.ndim == 2 and a.shape[0] >= 1
    out = np.zeros((a.shape[0], out_words), np.uint32)
    pr = np.zeros(4, np.uint32)
    pr[:len(params)] = params
    fn = getattr(lib(), f"bz_dh_run_{tag}")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                   ctypes.c_uint32, ctypes.c_void_p]
    rc = fn(op.encode(), a.ctypes.data, a.size, out.ctypes.data, out.size, a.shape[0], pr.ctypes.data)
    if rc != 0:
        what = {-1: "unknown op", -2: "record sizes do not match the op", -3: "parameters out of range"}
        raise HarnessError(f"{tag}/{op}: {what.get(rc, 'HIP error %d' % rc)}")
    return out


def assert_proof_rejections():
    """what the `proof` object cannot validate it rejects on the host, before anything is launched:
    the record fields a kernel would index memory with, and parameters out of range"""
    rate, scalar_bits = 166, 253        # kRate of proof/transcript.h, kScalarBits of proof/inner_product_protocol.h

    def refused(what, op, record_words, out_words, params=(), byte=None, value=0):
        rec = np.zeros((2, record_words), np.uint32)      # (the second record is the offending one)
        if byte is not None:
            rec[1].view(np.uint8)[byte] = value
        try:
            run("proof", op, rec, out_words, params)
        except HarnessError as e:
            assert what in str(e), (op, params, byte, value, str(e))
        else:
            raise AssertionError(f"proof/{op} accepted params {params}, byte {byte} = {value}")

    # a transcript's position indexes LDS
    for pos in (rate, rate + 1, 255):
        refused("parameters out of range", "merlin_wave", 183, 115, (1, 0, 32, 0), 200, pos)
        refused("parameters out of range", "sumcheck_round_wave", 123, 75, (0, 2), 200, pos)
        refused("parameters out of range", "ip_round_wave", 69, 67, (0,), 200, pos)
    # digits pick one of three terms, the count (the word behind the 256 digits) bounds the walk
    for byte, value in ((0, 4), (255, 0xff), (256, scalar_bits + 1), (259, 1)):
        refused("parameters out of range", "ip_fold_point", 145, 40, (), byte, value)
    # parameter ranges
    for params in ((0,), (3,)):
        refused("parameters out of range", "keccak_wave", 50, 50, params)
    for params in ((0, 0, 32, 0), (17, 0, 32, 0), (1, 513, 32, 0), (1, 0, 0, 0), (1, 0, 257, 0),
                   (1, 8, 32, 2), (1, 7, 32, 1)):
        refused("parameters out of range", "merlin_wave", 183, 115, params)
    for n in (0, 65):
        refused("parameters out of range", "s25_dot", 16 * n, 8, (n,))
    for params in ((2, 2), (0, 1), (0, 10)):
        refused("parameters out of range", "sumcheck_round_wave", 123, 75, params)
    refused("parameters out of range", "ip_round_wave", 69, 67, (2,))
    # sizes that do not match the op's record, and an op of another object
    refused("record sizes", "merlin_wave", 182, 115, (1, 0, 32, 0))
    refused("unknown op", "f29_mul", 18, 9)
