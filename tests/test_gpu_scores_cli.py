"""The trainer CLI's --predict_data / --predict_out / --predict_output: after training (and after the
model and the checkpoint are written) the file is scored through the pipelined prediction and one
prediction per row is written, in file order, as the shortest decimal that parses back to the float.
The lines are the bits the Python binding predicts with an engine trained by the same schedule; a
saved model scored by a second run (--resume_from ck --n_epochs 0) gives the same bytes; without the
flags nothing printed changes; two shards (the synchronous group call) agree with one engine.
(run_cli / parse_libffm / the schedule of replay are those of tests/test_gpu_metrics_cli.py.)"""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import Csr
from util import GOLDEN, assert_bitwise

pytestmark = pytest.mark.gpu

SCORED_LINE = re.compile(r"^scored (\d+) rows time: [0-9.]+s\n", re.M)
BATCH = 256


def _bundled(tmp_path):
    with gzip.open(os.path.join(GOLDEN, "data", "libffm_data.txt.gz"), "rt") as f:
        text = f.read()
    p = tmp_path / "libffm_data.txt"
    p.write_text(text)
    return str(p), text


def parse_libffm(text):
    """The file as the CLI reads it: zero values dropped (parser.cpp:65), labels > 0 positive."""
    rows, labels = [], []
    for line in text.splitlines():
        t = line.split()
        labels.append(1 if int(t[0]) > 0 else 0)
        rows.append([(int(f), int(i), float(np.float32(v))) for f, i, v in (tok.split(":") for tok in t[1:])
                     if np.float32(v) != 0])
    return Csr.from_rows(rows, labels)


def run_cli(tmp_path, args, env=None):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def without_times(stdout):
    return re.sub(r"time: [0-9.]+s", "time: Ts", stdout)


def train_online(model, data, batch, ramp, epochs):
    """The online trainer's schedule through the Python binding: rows in file order, block t of
    min(batch, max(1, rows_seen / ramp)) rows (ramp 0: batch)."""
    total, seen = data.n_rows, 0
    for _ in range(epochs):
        pos = 0
        while pos < total:
            n = min(batch, max(1, seen // ramp)) if ramp > 0 else batch
            n = min(n, total - pos)
            model.train_batch(data.rows(pos, pos + n))
            seen += n
            pos += n


def read_scores(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "", "the file ends with a line end"
    return np.array([np.float32(s) for s in lines[:-1]], np.float32), lines[:-1]


_trained = {}


def trained_reference(text):
    """(logits, probabilities) of every row of the bundled file by a binding engine trained one online
    epoch in blocks of BATCH: computed once, shared, never written to."""
    if not _trained:
        data = parse_libffm(text)
        e = fa.Engine("FFM", 10000, 8, 16, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256)
        train_online(e, data, BATCH, fa.default_batch_ramp(1e-4), 1)
        for name, prob in (("logit", False), ("prob", True)):
            out = np.concatenate([e.predict_batch(data.rows(p, min(data.n_rows, p + BATCH)), output_prob=prob)[0]
                                  for p in range(0, data.n_rows, BATCH)])
            out.setflags(write=False)
            _trained[name] = out
        e.close()
    return _trained["logit"], _trained["prob"]


BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH)]


def test_online_training_then_scoring(tmp_path):
    path, text = _bundled(tmp_path)
    logit, prob = trained_reference(text)
    n = len(text.splitlines())
    for flag, want, out_name in (([], prob, "p.txt"), (["--predict_output", "prob"], prob, "p2.txt"),
                                 (["--predict_output", "logit"], logit, "l.txt")):
        stdout = run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "1", "--predict_data", path,
                                           "--predict_out", out_name] + flag)
        m = SCORED_LINE.findall(stdout)
        assert m == [str(n)], stdout
        assert stdout.rstrip("\n").splitlines()[-1].startswith("scored "), stdout  # (after training and saving)
        got, lines = read_scores(tmp_path / out_name)
        assert got.size == n  # one line per input row
        assert_bitwise(got, want, "CLI scores %s" % (flag or ["default"])[-1])
        # the shortest spelling: no line is longer than nine significant digits need
        assert max(len(s) for s in lines) <= 16
    assert 0.0 < prob.min() and prob.max() < 1.0 and (logit < 0).any()


def test_scoring_a_saved_model(tmp_path):
    path, text = _bundled(tmp_path)
    first = run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "1", "--checkpoint_path", "ck",
                                      "--predict_data", path, "--predict_out", "first.txt"])
    assert "epoch 1 train time" in first
    second = run_cli(tmp_path, BASE + ["--resume_from", "ck", "--n_epochs", "0", "--predict_data", path,
                                       "--predict_out", "second.txt"])
    assert "epoch" not in second, second
    assert SCORED_LINE.findall(second) == SCORED_LINE.findall(first) == [str(len(text.splitlines()))]
    a, b = (tmp_path / "first.txt").read_bytes(), (tmp_path / "second.txt").read_bytes()
    assert len(a) > 0 and a == b
    # the same with the training file named and the offline task: still nothing trained, the same bytes
    third = run_cli(tmp_path, BASE[:2] + ["--online", "false", "--batch_size", str(BATCH), "--train_data", path,
                                          "--resume_from", "ck", "--n_epochs", "0", "--predict_data", path,
                                          "--predict_out", "third.txt"])
    assert "epoch" not in third, third
    assert (tmp_path / "third.txt").read_bytes() == a


def test_nothing_changes_without_the_flags(tmp_path):
    path, _ = _bundled(tmp_path)
    base = BASE + ["--train_data", path, "--eval_data", path, "--n_epochs", "2", "--metrics", "auc"]
    plain = run_cli(tmp_path, base)
    with_flags = run_cli(tmp_path, base + ["--predict_data", path, "--predict_out", "p.txt"])
    assert "scored" not in plain and len(SCORED_LINE.findall(with_flags)) == 1
    assert without_times(SCORED_LINE.sub("", with_flags)) == without_times(plain)
    assert sorted(os.listdir(tmp_path)) == ["libffm_data.txt", "p.txt"]  # (nothing else is written)
    main_bin, _ = fa.build_host()
    for alone in (["--predict_data", path], ["--predict_out", "q.txt"]):
        bad = subprocess.run([main_bin] + base + alone, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and "--predict_data and --predict_out go together" in bad.stderr, bad.stderr
        assert bad.stdout == ""  # (refused before anything is trained)
    bad = subprocess.run([main_bin] + base + ["--predict_data", path, "--predict_out", "q.txt", "--predict_output", "odds"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--predict_output takes prob or logit" in bad.stderr
    assert not os.path.exists(tmp_path / "q.txt")


def test_two_shards_score_what_one_engine_scores(tmp_path):
    """--n_gpus 2 (the synchronous ffm_group_predict_batch behind the same Scorer) on generated rows laid
    out per field: the scores of the one-engine run to rtol 1e-5, the project's bound for cross-shard
    sums (their association order differs)."""
    F, per, k, rows, batch = 12, 500, 8, 4000, 512
    data = synth.Generator(F, F * per, "zipf", seed=5).block(rows)
    path = tmp_path / "s.ffm"
    path.write_text(synth.to_libffm_text(data))
    base = ["--train_data", str(path), "--model_type", "FFM", "--n_fields", str(F), "--n_feats", str(F * per),
            "--n_factors", str(k), "--online", "true", "--n_epochs", "1", "--batch_size", str(batch), "--batch_ramp", "32",
            "--w_alpha", "0.05", "--w_l1", "0.01", "--w_l2", "0.1", "--field_ranges", "uniform", "--predict_data", str(path)]
    one = run_cli(tmp_path, base + ["--predict_out", "one.txt"])
    two = run_cli(tmp_path, base + ["--predict_out", "two.txt", "--n_gpus", "2"], {"FTRL_SAME_DEVICE": "1"})
    assert "2 field-pair shards" in two and "field-pair shards" not in one
    assert SCORED_LINE.findall(one) == SCORED_LINE.findall(two) == [str(rows)]
    a, _ = read_scores(tmp_path / "one.txt")
    b, _ = read_scores(tmp_path / "two.txt")
    assert a.size == b.size == rows and np.isfinite(a).all() and a.std() > 0.01
    print("two shards against one engine: largest relative difference %.3g" % float(np.max(np.abs(a - b) / np.abs(a))))
    np.testing.assert_allclose(b, a, rtol=1e-5, atol=0)
