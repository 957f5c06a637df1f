"""bench.py command line: a plain run prints only the headline result line,
--full adds the sanity figures and the companion GLM measurement, and
--dump-outputs writes the last timed step's arrays, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--gpus", "1", "--rows", "4000", "--cols", "6", "--max-depth", "3", "--steps", "2", "--warmup", "1"]
MOVED = {"train_logloss_after", "trees_built", "glm_iters_per_sec", "glm_ms_per_iter", "glm_model",
         "glm_hessian_tier", "glm_precision"}


def _bench(*extra):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SHAPE, *extra], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def plain_dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench("--dump-outputs", str(d / "a")), d


def test_plain_run_prints_headline_only(plain_dump):
    out, _ = plain_dump
    assert out["metric"] == "gbm_trees_per_sec" and out["unit"] == "trees/s" and out["higher_is_better"] is True
    assert out["dtype"] == "fp32" and out["steps"] == 2 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] / 1000 - 1) < 1e-3
    assert not MOVED & set(out)


def test_full_run_adds_sanity_and_glm():
    out = _bench("--full")
    assert MOVED <= set(out)
    assert out["trees_built"] == 3 and 0 < out["train_logloss_after"] < 0.7
    assert out["glm_iters_per_sec"] > 0 and out["glm_ms_per_iter"] > 0
    assert not {"glm_iters_per_sec", "glm_ms_per_iter"} & set(_bench("--full", "--no-glm"))


def test_dump_outputs_same_from_run_to_run(plain_dump):
    _, d = plain_dump
    _bench("--dump-outputs", str(d / "b"))
    assert os.listdir(d / "a") == ["predictions.npy"] == os.listdir(d / "b")
    a, b = np.load(d / "a" / "predictions.npy"), np.load(d / "b" / "predictions.npy")
    assert a.dtype == np.float32 and a.shape == (4000,) and np.isfinite(a).all()
    assert a.min() >= 0 and a.max() <= 1 and a.std() > 0
    assert np.array_equal(a, b)


def test_dump_outputs_samples_a_large_array(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(bench._DUMP_BYTES // 8 + 1000, dtype=torch.float32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": np.arange(5, dtype=np.float64)})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and a.nbytes <= bench._DUMP_BYTES // 2 and np.all(np.diff(a) >= 0)
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, np.arange(5))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000
