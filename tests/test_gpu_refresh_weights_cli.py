"""The trainer CLI's --refresh_weights: with it every stored weight is set from its accumulators after
each epoch's training (before that epoch's evaluation), and so before the model, the checkpoint and the
scores are written; each refresh prints one `weights:` line.  Without it not a byte changes; with it the
training losses and the accumulators are the same bits, the evaluation is not; a checkpoint written under
the flag scores like the run that wrote it, and so does a stale checkpoint refreshed when it is loaded;
two shards agree with one engine.
(run_cli / without_times / read_scores are those of tests/test_gpu_scores_cli.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

pytestmark = pytest.mark.gpu

# the wording of the line, pinned
WEIGHTS_LINE = re.compile(r"^epoch (\d+) weights: linear (\d+) live, (\d+) nonzero, (\d+) moved; "
                          r"latent (\d+) live, (\d+) nonzero, (\d+) moved$", re.M)
F, PER, K, ROWS, BATCH = 8, 300, 4, 1500, 256


def run_cli(tmp_path, args, env=None):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def without_times(stdout):
    return re.sub(r"time: [0-9.]+s", "time: Ts", stdout)


def read_scores(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "", "the file ends with a line end"
    return np.array([np.float32(s) for s in lines[:-1]], np.float32)


def _data(tmp_path):
    """A small libffm file with a Zipf tail; asserts that it holds features that occur exactly once."""
    blk = synth.Generator(F, F * PER, "zipf", seed=8).block(ROWS)
    path = tmp_path / "s.ffm"
    path.write_text(synth.to_libffm_text(blk))
    ids = [int(tok.split(":")[1]) for line in path.read_text().splitlines() for tok in line.split()[1:]]
    _, cnt = np.unique(ids, return_counts=True)
    assert (cnt == 1).sum() >= 50, "the data must contain single-occurrence features"
    return str(path)


def _base(path, online="true"):
    return ["--train_data", path, "--model_type", "FFM", "--n_fields", str(F), "--n_feats", str(F * PER), "--n_factors", str(K),
            "--online", online, "--batch_size", str(BATCH), "--batch_ramp", "32", "--w_alpha", "0.05", "--w_l1", "0.01",
            "--w_l2", "0.1"]


def _files(tmp_path, names):
    return {n: (tmp_path / n).read_bytes() for n in names}


def test_nothing_changes_without_the_flag(tmp_path):
    path = _data(tmp_path)
    args = _base(path) + ["--eval_data", path, "--n_epochs", "2", "--metrics", "auc", "--predict_data", path,
                          "--model_path", "m.txt", "--checkpoint_path", "ck", "--predict_out", "p.txt"]
    names = ["ck", "m.txt", "m.txt.nz", "p.txt"]
    (tmp_path / "plain").mkdir()
    (tmp_path / "off").mkdir()
    plain = run_cli(tmp_path / "plain", args)  # (the same file names in two directories: the output names them)
    off = run_cli(tmp_path / "off", args + ["--refresh_weights", "false"])
    assert "weights:" not in plain and "weights:" not in off
    assert without_times(off) == without_times(plain)
    a, b = _files(tmp_path / "plain", names), _files(tmp_path / "off", names)
    assert a == b and all(len(v) > 0 for v in a.values())
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "off")) == names


@pytest.mark.parametrize("online,learn", [("true", "false"), ("false", "false"), ("true", "true")],
                         ids=["online", "offline", "online-learn"])
def test_flag_changes_what_is_evaluated_and_nothing_that_is_trained(tmp_path, online, learn):
    path = _data(tmp_path)
    base = _base(path, online) + ["--eval_data", path, "--n_epochs", "2", "--learn", learn]
    plain = run_cli(tmp_path, base + ["--model_path", "m0.txt"])
    fresh = run_cli(tmp_path, base + ["--model_path", "m1.txt", "--refresh_weights", "true"])
    train = re.compile(r"train loss: (\S+)")
    assert train.findall(fresh) == train.findall(plain) and len(train.findall(plain)) == 2
    # the accumulators the run leaves behind are the same bytes; the weights are not
    assert (tmp_path / "m1.txt.nz").read_bytes() == (tmp_path / "m0.txt.nz").read_bytes()
    assert (tmp_path / "m1.txt").read_bytes() != (tmp_path / "m0.txt").read_bytes()
    lines = WEIGHTS_LINE.findall(fresh)
    assert [m[0] for m in lines] == ["1", "2"], fresh
    for m in lines:
        ep, lin_live, lin_nz, lin_moved, lat_live, lat_nz, lat_moved = map(int, m)
        assert 0 < lin_nz <= lin_live <= F * PER + 1 and 0 < lin_moved <= lin_live
        assert 0 <= lat_nz <= lat_live <= F * PER * F * K and 0 <= lat_moved <= lat_live
        # (the reference's rule never moves a latent accumulator off zero; --learn does)
        assert (lat_live > 0) == (learn == "true") and (lat_moved > 0) == (learn == "true")
    # each line sits between its epoch's training line and its evaluation line
    order = [ln.split()[2] for ln in fresh.splitlines() if ln.startswith("epoch ")]
    assert order == ["train", "weights:", "eval"] * 2, order
    assert not WEIGHTS_LINE.search(plain)
    # the text without the weights lines differs exactly where the evaluation is
    evals = re.compile(r"eval loss: (\S+)")
    assert len(evals.findall(plain)) == 2 and evals.findall(fresh) != evals.findall(plain)
    assert evals.findall(fresh)[0] != evals.findall(plain)[0]


def test_checkpoints_and_scores_are_self_consistent(tmp_path):
    path = _data(tmp_path)
    base = _base(path) + ["--n_epochs", "1"]
    score = ["--predict_data", path, "--predict_out"]
    a = run_cli(tmp_path, base + ["--refresh_weights", "true", "--checkpoint_path", "ck"] + score + ["P0"])
    run_cli(tmp_path, _base(path) + ["--resume_from", "ck", "--n_epochs", "0"] + score + ["P1"])
    p0 = (tmp_path / "P0").read_bytes()
    assert len(p0) > 0 and (tmp_path / "P1").read_bytes() == p0  # the checkpoint carries the refreshed w
    b = run_cli(tmp_path, base + ["--checkpoint_path", "ckB"] + score + ["PB"])
    assert "weights:" not in b and (tmp_path / "PB").read_bytes() != p0  # (the stale model scores differently)
    c = run_cli(tmp_path, _base(path) + ["--resume_from", "ckB", "--n_epochs", "0", "--refresh_weights", "true"] + score + ["P2"])
    assert (tmp_path / "P2").read_bytes() == p0
    # the refresh of the loaded model saw what the training run's refresh saw
    la, lc = WEIGHTS_LINE.findall(a), WEIGHTS_LINE.findall(c)
    assert len(la) == 1 and la == lc, (la, lc)


def test_two_shards_score_what_one_engine_scores_under_the_flag(tmp_path):
    path = _data(tmp_path)
    plain = _base(path) + ["--n_epochs", "1", "--field_ranges", "uniform", "--predict_data", path]
    base = plain + ["--refresh_weights", "true"]
    one = run_cli(tmp_path, base + ["--predict_out", "one.txt"])
    two = run_cli(tmp_path, base + ["--predict_out", "two.txt", "--n_gpus", "2"], {"FTRL_SAME_DEVICE": "1"})
    assert "2 field-pair shards" in two and "field-pair shards" not in one
    stale = run_cli(tmp_path, plain + ["--predict_out", "stale.txt"])
    assert "weights:" not in stale
    a = read_scores(tmp_path / "one.txt")
    b = read_scores(tmp_path / "two.txt")
    s = read_scores(tmp_path / "stale.txt")
    assert a.size == b.size == ROWS and np.isfinite(a).all()
    # (the comparison of tests/test_host.py::test_cli_n_gpus_shards_match_one_engine)
    assert np.allclose(b, a, atol=2e-4), float(np.max(np.abs(a - b)))
    assert not np.allclose(s, a, atol=2e-4)  # (the flag is what moved the scores)
    assert WEIGHTS_LINE.findall(one) == WEIGHTS_LINE.findall(two)
