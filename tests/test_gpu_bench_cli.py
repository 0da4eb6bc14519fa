"""The driver's command shapes for bench.py, run as the driver runs them (a child process, no
launcher around it) on the one GPU there is: `--gpus 2` must start its own ranks, train the
field-pair-sharded model through the staged host path and print ONE JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=900):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_gpus_2_launches_its_own_ranks_and_reports_both_scalings():
    d = _run(["--gpus", "2", "--same-device", "--backend", "gloo", "--steps", "3", "--warmup", "1",
              "--n-feats", "780000", "--no-cpu-baseline", "--full"])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["unit"] == "samples/s"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["rows_per_step"] == 2 * 8192
    assert d["config"]["sharding"].startswith("field-pair x2")
    o = d["other_scaling"]
    assert o["scaling"] == "strong" and o["rows_per_step"] == 8192 and o["value"] > 0
    # what each block size costs in logloss against the per-sample loop rides along (north-star bound 1e-4)
    assert abs(d["block_logloss_cost"]["d_eval_logloss"]) < 1e-4
    assert abs(o["block_logloss_cost"]["d_eval_logloss"]) < 1e-4
    assert 0.5 < d["train_logloss"] < 0.9


def test_gpus_1_default_shape_line_has_roofline():
    d = _run(["--steps", "3", "--warmup", "2", "--n-feats", "780000", "--no-cpu-baseline", "--no-eval", "--full"])
    assert d["n_gpus"] == 1 and d["config"]["sharding"] == "none"
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3


def test_plain_line_is_lean_and_its_dump_repeats(tmp_path):
    """Without --full the line carries the headline figure and none of the extras; --dump-outputs
    writes the last timed step's logits, loss and a sample of the state it left, float32 / float64,
    at most 64 MB, and two runs with the same arguments write the same bits."""
    args = ["--steps", "3", "--warmup", "2", "--n-feats", "780000", "--dump-outputs"]
    d = _run(args + [str(tmp_path / "a")])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert not {"resident", "eval", "roofline", "cpu_baseline"} & set(d)
    _run(args + [str(tmp_path / "b")])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"logits.npy", "loss_sum.npy", "bias3.npy", "state_ids.npy", "state_vec_w.npy"} <= set(names)
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, b, equal_nan=True), name
        total += a.nbytes
    assert total <= 64 << 20
    logits = np.load(tmp_path / "a" / "logits.npy")
    assert logits.shape == (8192,) and np.isfinite(logits).all() and np.any(logits != 0)
    assert 0.3 < float(np.load(tmp_path / "a" / "loss_sum.npy")[0]) / 8192 < 1.2
