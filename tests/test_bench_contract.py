"""bench.py keeps the driver's contract: ONE JSON line with the agreed keys, BASELINE.json's metric,
a roofline object and a cpu_baseline object; without a GPU it fails loudly instead of measuring a
fallback."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT)


def test_bench_refuses_to_run_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out = _run(["--workload", "c2_n1008", "--steps", "1", "--warmup", "0"], 300)
    assert out.returncode != 0
    assert not any(line.startswith("{") for line in out.stdout.splitlines())   # no number from a fallback


@pytest.mark.gpu
def test_bench_json_contract(gpu):
    out = _run(["--workload", "c2_n1008", "--steps", "2", "--warmup", "1", "--full"], 900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "syndromes/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma", "infinity_cache") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "syndromes/s" and c["sample"]
    assert c["gpu_matches_oracle_on_sample"] is True and c["reference_faithful_1_thread"]["cores"] == 1
    # N = 1 runs the multi-GPU path's own code (sharding.batchdecode_sharded) in its degenerate form
    assert d["config"]["mode"] == "scatter" and d["exchange"]["scatter_bytes_per_peer"] == 0


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_stays_within_budget_and_samples_rows_by_seed(tmp_path):
    """dump_outputs writes per-syndrome scalars whole and a seeded sample of the per-bit rows, float32 / float64 only,
    at most DUMP_BYTES in all; the same arrays give the same files."""
    import numpy as np
    import torch

    bench = _bench_module()
    batch, n = 4096, 16384            # 256 MiB of float32 hard decisions: must be sampled
    g = torch.Generator().manual_seed(3)
    arrays = {"errors": (torch.rand((batch, n), generator=g) < 0.1).to(torch.uint8),
              "converged": (torch.rand(batch, generator=g) < 0.5).to(torch.uint8),
              "iterations": torch.randint(0, 51, (batch,), generator=g, dtype=torch.int32),
              "llr": torch.randn((batch, n), generator=g, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch, arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["converged.npy", "errors.npy", "iterations.npy", "llr.npy", "rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values()) and got["llr"].dtype == np.float64
    rows = got["rows"].astype(np.int64)
    assert 0 < len(rows) < batch and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["errors"], arrays["errors"].numpy()[rows].astype(np.float32))
    assert np.array_equal(got["llr"], arrays["llr"].numpy()[rows])
    assert np.array_equal(got["converged"], arrays["converged"].numpy().astype(np.float32))
    assert np.array_equal(got["iterations"], arrays["iterations"].numpy().astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    # a batch that fits is written whole
    small = {k: v[:64] for k, v in arrays.items()}
    bench.dump_outputs(str(tmp_path / "c"), torch, small)
    assert np.array_equal(np.load(tmp_path / "c" / "rows.npy"), np.arange(64, dtype=np.float64))


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_reproducible_outputs(gpu, tmp_path):
    """Without --full the result line holds the headline figure and its roofline, not the CPU baselines or the `also`
    workloads; --steps sets the number of timed steps; --dump-outputs writes the last step's results, and two runs with
    the same arguments write the same arrays."""
    import numpy as np

    for d in ("a", "b"):
        out = _run(["--workload", "c2_n1008", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)], 900)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [line for line in out.stdout.splitlines() if line.startswith("{")]
        assert len(lines) == 1
        r = json.loads(lines[0])
        assert r["steps"] == 3 and r["ms_per_step"] > 0 and "roofline" in r
        assert "cpu_baseline" not in r and "also" not in r
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["converged.npy", "errors.npy", "iterations.npy", "rows.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["errors"].shape == (4096, 1008) and got["converged"].shape == (4096,)
    assert abs(float(got["converged"].astype(np.float64).mean()) - r["config"]["converged_frac"]) < 1e-6
    assert abs(float(got["iterations"].astype(np.float64).mean()) - r["config"]["mean_iters"]) < 1e-6
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
