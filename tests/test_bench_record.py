"""bench.py's record: the LAST stdout line is one compact strict-JSON object under 4 KB with the
contract's members, `roofline` and `cpu_baseline` as flat objects; everything else goes to a sidecar
file.  (Round 5's single 24 KB line could not be recovered by the driver: BENCH_r05.parsed == null.)
The canned input is that very record, profiles/round5_bench_final.json."""
import importlib.util
import io
import json
import os
import subprocess
import sys
import types
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_record_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _strict(line):
    def refuse(name):
        raise ValueError(f"{name} is not JSON")
    return json.loads(line, parse_constant=refuse)


def _canned():
    with open(os.path.join(ROOT, "profiles", "round5_bench_final.json")) as fh:
        return json.load(fh)


def test_compact_record_is_small_strict_and_complete(bench):
    full = _canned()
    assert len(json.dumps(full)) > 20000  # the record that broke the driver's parse
    line = bench.compact_record(full)
    assert len(line) < 4096 and "\n" not in line
    d = _strict(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "verified"):
        assert k in d, k
    assert d["config"]["workload"] == full["config"]["workload"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(full["value"], rel=1e-5) and d["verified"] is True
    roof = d["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic",
              "algorithmic_bytes_per_launch", "kernel_ms", "valu_busy", "alu_frac", "box_fetch_kind"):
        assert k in roof, k
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and roof["unit"] == "GB/s"
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-4)
    # achieved = algorithmic bytes per launch / the kernel's duration
    assert roof["achieved"] == pytest.approx(
        roof["algorithmic_bytes_per_launch"] / (roof["kernel_ms"] * 1e-3) / 1e9, rel=1e-4)
    assert all(not isinstance(v, (dict, list)) for v in roof.values())
    cpu = d["cpu_baseline"]
    assert set(cpu) == {"value", "unit", "cores", "kind", "sample"} and cpu["kind"] == "reference"
    assert all(not isinstance(v, (dict, list)) for v in cpu.values())


def test_compact_record_survives_nan_and_oversized_members(bench):
    full = _canned()
    full["roofline"]["traffic"] = float("nan")
    full["stage_ms"] = {f"stage_{i}": 0.001 * i for i in range(400)}     # an over-eager later edit
    full["strong_scaling"] = {"ms_per_call": float("inf"), "verified": "bit-exact ...", "columns_per_gpu": 32}
    line = bench.compact_record(full)
    assert len(line) < 4096
    d = _strict(line)
    assert d["roofline"]["traffic"] is None and "stage_ms" not in d
    assert d["strong_scaling"] == {"ms_per_call": None, "verified": True, "columns_per_gpu": 32}


def test_emit_prints_the_compact_record_last_and_writes_the_sidecar(bench, tmp_path):
    full = _canned()
    args = types.SimpleNamespace(detail_file=str(tmp_path / "sub" / "detail.json"), full=True)
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(full, args)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096          # nothing before or after it on stdout
    d = _strict(lines[-1])
    with open(tmp_path / "sub" / "detail.json") as fh:
        detail = _strict(fh.read())
    assert detail["configs"] and detail["host_api"] and detail["value"] == full["value"]
    assert "detail_file" in d


def test_issue_frac_prices_the_whole_instruction_mix(bench):
    """`issue_frac` = `alu_frac` scaled by the loop's whole instruction mix over its multiply-adds
    alone (profiles/isa_counts.json: every VALU instruction at the measured issue cost of its
    class); it enters the compact record beside `alu_frac`."""
    kernel = "k_accumulate<bz::ed25519_msm>"
    with open(os.path.join(ROOT, "profiles", "isa_counts.json")) as fh:
        isa = json.load(fh)["kernels"][kernel]
    classes = isa["issue_classes"]
    assert classes["mad64"] == isa["mads_per_addition"]
    assert sum(classes.values()) == isa["loop_valu"]
    assert isa["issue_cycles_per_addition"] > isa["mad_issue_cycles_per_addition"] > 0
    roof = bench.roofline_of(kernel, 192 << 20, 0.64, additions=16 << 20)
    mix = isa["issue_cycles_per_addition"] / isa["mad_issue_cycles_per_addition"]
    assert roof["issue_frac"] == pytest.approx(roof["alu_frac"] * mix, rel=1e-9)
    assert roof["alu_frac"] < roof["issue_frac"] < 1.05
    full = _canned()
    full["roofline"]["issue_frac"] = roof["issue_frac"]
    d = _strict(bench.compact_record(full))
    assert d["roofline"]["issue_frac"] == pytest.approx(roof["issue_frac"], rel=1e-5)


def test_plain_and_full_options(bench):
    """a plain run is the default; --detail implies --full; --steps sets the timed steps (>= 1)"""
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert bench.parse_args(["--full"]).full and bench.parse_args(["--detail"]).full
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_plain_emit_prints_the_compact_record_and_writes_nothing(bench, tmp_path):
    full = _canned()
    args = types.SimpleNamespace(detail_file=str(tmp_path / "detail.json"), full=False)
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(full, args)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096
    d = _strict(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert not (tmp_path / "detail.json").exists() and "detail_file" not in d


def test_dump_outputs_are_float64_and_exact(bench, tmp_path):
    c = np.arange(64, dtype=np.uint8).reshape(2, 32)
    bench.dump_outputs(str(tmp_path / "d"), {"commitments": c})
    got = np.load(tmp_path / "d" / "commitments.npy")
    assert got.dtype == np.float64 and np.array_equal(got, c)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_commitment(oracle, tmp_path):
    """a plain run at reduced rows prints the headline line only, and --dump-outputs holds the last
    timed step's commitment: the reference CPU backend's on the same scalars and generators"""
    log2n = 12
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--log2n", str(log2n), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _strict(r.stdout.splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["higher_is_better"] is True and "roofline" not in d and "cpu_baseline" not in d
    got = np.load(tmp_path / "out" / "commitments.npy")
    assert got.dtype == np.float64 and got.shape == (1, 32)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import baseline_workloads as wl
    scalars = wl.mt19937_scalars(1, 1 << log2n, 32, top_mask=0x0f, seed=0)[0]
    want = oracle.commit(0, [(scalars, False)], oracle.ristretto_generators(1 << log2n))
    assert np.array_equal(got, want.astype(np.float64))
