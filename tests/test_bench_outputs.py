"""bench.py --dump-outputs and --full.

--dump-outputs DIR writes what the last timed step left in its output set,
and the timed region's counters, as DIR/<name>.npy in float32 / float64, at
most bench.DUMP_BYTES in all; the inputs are seeded, so the files of two runs
with the same arguments are equal. A plain run leaves the CPU baseline out
(cpu_baseline: null); --full runs it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from fastclick_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_outputs_formats_cap_and_sample(tmp_path):
    arrs = dict(verdict=np.arange(70_000, dtype=np.uint32).astype(np.uint16),
                hash=np.arange(70_000, dtype=np.uint32) * np.uint32(61_357) + np.uint32(0xFFFF0000),
                big=np.arange(3_000_000, dtype=np.uint32),
                counters=np.arange(81, dtype=np.uint64) << np.uint64(40))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.write_outputs(a, arrs)
    bench.write_outputs(b, arrs)
    bench.write_outputs(b, arrs, rank=1)
    assert sorted(os.listdir(a)) == ["big.npy", "counters.npy", "hash.npy", "verdict.npy"]
    assert sorted(os.listdir(b)) == sorted(os.listdir(a) + [f"{k}.rank1.npy" for k in arrs])
    got = {k: np.load(os.path.join(a, k + ".npy")) for k in arrs}
    for k in arrs:
        assert np.array_equal(got[k], np.load(os.path.join(b, k + ".npy")))
    assert got["verdict"].dtype == np.float32 and got["hash"].dtype == np.float64
    assert got["counters"].dtype == np.float64
    for k in ("verdict", "hash", "counters"):       # whole, and exact
        assert np.array_equal(got[k].astype(np.uint64), arrs[k].astype(np.uint64))
    # over its share (a quarter of DUMP_BYTES): a sample at ascending positions
    share = bench.DUMP_BYTES // 4
    assert got["big"].nbytes <= share and got["big"].size == share // 8
    assert (np.diff(got["big"]) > 0).all() and got["big"].max() < 3_000_000
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_BYTES


def test_plain_run_is_lean_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None
    assert bench.parse(["--full"]).full is True
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


class _DumpingProcessor:
    """tests.test_bench_dist.OracleProcessor plus outputs(), as DeviceProcessor has."""

    def __new__(cls, args, lo, hi, gpu):
        from tests.test_bench_dist import OracleProcessor
        p = OracleProcessor(args, lo, hi, gpu)
        p.outputs = lambda: {"verdict": np.full(p.n, 0x0806, np.uint16)}
        return p


def test_rank_main_runs_cpu_baseline_only_with_full(oracle, tmp_path, monkeypatch):
    """bench.rank_main at world 1 over the CPU stand-in: a plain run never
    starts the CPU baseline and leaves cpu_baseline null, --full runs it (and
    --no-cpu still leaves it out); --dump-outputs writes the processor's
    outputs and the timed region's counters."""
    calls = []
    real = bench.cpu_baseline
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: calls.append(a) or real(*a, **k))
    common = ["--gpus", "1", "--packets", "5000", "--steps", "2", "--warmup", "1", "--nbuf", "1",
              "--cpu-seconds", "0.3"]
    d = str(tmp_path / "d")

    def run(*extra):
        return bench.rank_main(bench.parse(common + list(extra)), _DumpingProcessor, world=1, rank=0, gpu=0,
                               backend="gloo", dev_for_collectives="cpu")

    plain = run("--dump-outputs", d)
    assert plain["cpu_baseline"] is None and not calls
    assert plain["steps"] == 2 and plain["ms_per_step"] >= 0
    assert sorted(os.listdir(d)) == ["counters.npy", "verdict.npy"]
    assert np.load(os.path.join(d, "counters.npy"))[N.CTR_COUNT] == 2 * 5000
    assert run("--full", "--no-cpu")["cpu_baseline"] is None and not calls
    full = run("--full")
    assert len(calls) == 1 and full["cpu_baseline"]["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k]


def _bench(tmp_path, name, *extra):
    d = str(tmp_path / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--packets", "5000", "--workload", "c4", "--errors", "0.01", "--nbuf", "2",
                        "--dump-outputs", d, *extra], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_gpu_bench_dump_outputs_vs_oracle(oracle, tmp_path):
    """The dumped verdicts, hashes and counters of a 5,000-packet C4 run with
    the with-errors mix equal the oracle's on the same batch (3 timed steps:
    the counters are 3 x one batch's), a second run writes the same files, and
    only --full fills cpu_baseline."""
    line, got = _bench(tmp_path, "a")
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    args = bench.parse(["--packets", "5000", "--workload", "c4", "--errors", "0.01"])
    b, _ = bench.make_host_batch(args)
    cfg = N.make_cfg(offset=14, checksum=True, classify=N.CLS_LB_HASH, nports=16,
                     badsrc=[N.raw_addr(a) for a in bench.ERROR_BADSRC])
    exp = oracle.process_batch(cfg, b)
    assert set(got) == {"verdict", "hash", "tile_perm", "tile_count", "counters"}
    assert got["verdict"].dtype == np.float32 and got["hash"].dtype == np.float64
    assert np.array_equal(got["verdict"].astype(np.uint16), exp["verdict"].astype(np.uint16))
    assert np.array_equal(got["hash"].astype(np.uint32), exp["hash"])
    assert np.array_equal(got["counters"].astype(np.uint64), 3 * exp["counters"].astype(np.uint64))
    line2, again = _bench(tmp_path, "b", "--full", "--cpu-seconds", "0.3")
    assert sorted(again) == sorted(got)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    assert line2["cpu_baseline"] is not None and line2["cpu_baseline"]["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert line[k] == line2[k]
