"""bench.py's --dump-outputs and --full: the dump helper on the CPU (dtype, file names, the
seeded sample of an output above the size limit), and on the GPU the smallest config
(mlp.onnx, batch 4096): a plain run prints the headline fields only and writes the logits of
its last timed step; the same arguments with --full give the same logits and the checks."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")


def test_dump_outputs_files_and_dtypes(tmp_path):
    one = types.SimpleNamespace(rank=0, world=1)
    a32 = np.arange(12, dtype=np.float32).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "d"), one, {"logits": a32, "f64": a32.astype(np.float64),
                                                   "ints": np.arange(5, dtype=np.int8)})
    got = np.load(tmp_path / "d" / "logits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a32)
    assert np.load(tmp_path / "d" / "f64.npy").dtype == np.float64
    ints = np.load(tmp_path / "d" / "ints.npy")
    assert ints.dtype == np.float32 and np.array_equal(ints, np.arange(5))
    rank1 = types.SimpleNamespace(rank=1, world=2)
    bench.dump_outputs(str(tmp_path / "d"), rank1, {"logits": a32})
    assert np.array_equal(np.load(tmp_path / "d" / "logits_rank1.npy"), a32)


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 100)
    one = types.SimpleNamespace(rank=0, world=1)
    a = np.random.default_rng(3).standard_normal((37, 11)).astype(np.float32)  # 407 elements > 100
    bench.dump_outputs(str(tmp_path / "a"), one, {"logits": a})
    bench.dump_outputs(str(tmp_path / "b"), one, {"logits": a})
    s = np.load(tmp_path / "a" / "logits.npy")
    assert s.shape == (100,) and s.nbytes <= 400
    assert np.array_equal(s, np.load(tmp_path / "b" / "logits.npy"))  # the same sample every run
    assert np.isin(s, a).all()


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "mlp4096", *argv],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_logits(tmp_path):
    plain = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    for k in HEADLINE:
        assert k in plain, k
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    # samples/s and ms_per_step are the same measurement (ms_per_step is printed to 1e-4 ms)
    assert plain["value"] == pytest.approx(4096 / (plain["ms_per_step"] * 1e-3), rel=1e-4 / plain["ms_per_step"])
    for k in ("verified", "roofline", "kernels", "cpu_baseline", "secondary"):
        assert k not in plain, k
    assert os.listdir(tmp_path / "plain") == ["logits.npy"]
    a = np.load(tmp_path / "plain" / "logits.npy")
    assert a.dtype == np.float32 and a.shape == (4096, 2) and np.isfinite(a).all()

    full = _bench("--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert full["verified"] is True and "roofline" in full
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype")} == \
           {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype")}
    assert np.array_equal(a, np.load(tmp_path / "full" / "logits.npy"))
