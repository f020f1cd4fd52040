"""The drop-in boundary pinned against the reference's OWN text:

  * tests/native/boundary/signatures.cc prints every struct's size / alignment / field offsets, every
    macro value and the exact type of all 18 exported functions; compiled once against the reference's
    cbindings/blitzar_api.h and once against include/blitzar_api.h (both linked against
    libblitzar_amd.so -- a missing symbol fails the link), the two programs must print the same lines:
    what bindgen would generate for blitzar-sys (rust/blitzar-sys/build.rs) is the same either way;
  * the reference's example program example/cbindings1/main.cc, compiled unchanged where it lies and
    linked against libblitzar_amd.so, prints what the reference's CPU backend computes;
  * BLITZAR_LOG_LEVEL (sxt/base/log/setup.cc:28-65): `info` lines where the reference has them
    (cbindings/backend.cc:78,122,127, bucket_method2/multiexponentiation.h:55,71), nothing by default.

__graft_entry__.build() compiles sig_ours into tests/native/_build/; the two compiled from the reference
tree are built by the oracle's recipe (oracle/ref/build_ref.py, which build() runs) into oracle/_ref/
(only where that tree is present; elsewhere they are used prebuilt, like the oracle itself)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "native", "_build")
REF_BUILD = os.path.join(ROOT, "oracle", "_ref")


def _exe(name):
    path = os.path.join(BUILD if name == "sig_ours" else REF_BUILD, name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built (__graft_entry__.build() with the reference tree present)")
    return path


def _run(name, **env):
    full = {k: v for k, v in os.environ.items() if not k.startswith("BLITZAR_")}
    full.update(env)
    r = subprocess.run([_exe(name)], env=full, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _example_expected(oracle):
    """what example/cbindings1/main.cc prints: the commitment of the bytes {1, 2, 3} to the built-in
    generators 0..2, every byte through `std::hex` (no zero padding)"""
    want = oracle.commit(0, [(np.array([[1], [2], [3]], np.uint8), False)],
                         oracle.ristretto_generators(3))
    return "".join("%x" % b for b in want[0]) + "\n"


def test_both_headers_describe_the_same_abi():
    theirs, ours = _run("sig_ref"), _run("sig_ours")
    assert theirs == ours
    lines = ours.splitlines()
    assert sum(ln.startswith("fn sxt_") for ln in lines) == 18
    assert sum(ln.startswith("struct ") for ln in lines) == 14
    assert "struct sxt_sequence_descriptor size 32 align 8" in lines
    assert "  sxt_transcript.bytes offset 0 size 203" in lines


def test_reference_example_program_on_the_host_backend(oracle):
    assert _run("ref_example_cbindings1", BLITZAR_BACKEND="cpu") == _example_expected(oracle)


@pytest.mark.gpu
def test_reference_example_program_on_the_gpu_backend(oracle):
    """unchanged: the example asks for SXT_GPU_BACKEND itself"""
    assert _run("ref_example_cbindings1") == _example_expected(oracle)


STAMP = r"\[\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\.\d{3}\] "


def test_log_level_info_lines(oracle):
    quiet = _run("ref_example_cbindings1", BLITZAR_BACKEND="cpu")
    assert quiet == _example_expected(oracle)                      # default level: err
    out = _run("ref_example_cbindings1", BLITZAR_BACKEND="cpu", BLITZAR_LOG_LEVEL="INFO")
    lines = out.splitlines()
    assert lines[-1] + "\n" == quiet
    want = ["override default backend with environmental variable BLITZAR_BACKEND=cpu",
            "initializing CPU backend",
            "compute a multiexponentiation with 1 outputs of length 3",
            "finished multiexponentiation with 1 outputs of length 3"]
    assert len(lines) == 5
    for line, message in zip(lines, want):
        assert re.fullmatch(STAMP + r"\[info\] " + re.escape(message), line), line
    # the reference's mapping (setup.cc:35-55): "error" selects debug (sic), "warn" / "off" silence info
    assert len(_run("ref_example_cbindings1", BLITZAR_BACKEND="cpu",
                    BLITZAR_LOG_LEVEL="error").splitlines()) == 5
    for level in ("warn", "critical", "off"):
        assert _run("ref_example_cbindings1", BLITZAR_BACKEND="cpu", BLITZAR_LOG_LEVEL=level) == quiet
