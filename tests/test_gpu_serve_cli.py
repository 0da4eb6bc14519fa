"""The trainer CLI's --serve_weights: a model trained with --learn true and saved as a sparse checkpoint is scored
by a second run (--resume_from ck --n_epochs 0 --predict_data F --predict_out P) from a training engine, from an
fp32 serving engine -- the same bytes, the same output -- and from an fp16 one -- line by line what the binding's
fp16 serving engine predicts, filled from the Python reproduction of the trained model.  The printed `bytes of
model` are ffm_engine_model_bytes' formulas.  (run_cli / parse_libffm / the schedule are those of
tests/test_gpu_scores_cli.py.)"""
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import BATCH, SCORED_LINE, _bundled, parse_libffm, read_scores, run_cli, train_online, without_times
from util import assert_bitwise

pytestmark = pytest.mark.gpu

NF, F, K = 10000, 8, 16  # the CLI's defaults
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--learn", "true"]
SERVING_LINE = re.compile(r"^serving weights: (\w+), (\d+) bytes of model\n", re.M)


def rank_auc(score, label):
    """Exact rank AUC, ties counted 1/2 (reported, never asserted)."""
    order = np.argsort(score, kind="stable")
    s, y = score[order], label[order]
    ranks = np.empty(s.size)
    i = 0
    while i < s.size:
        j = i
        while j + 1 < s.size and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = (i + j) / 2.0 + 1.0
        i = j + 1
    p, n = int(y.sum()), int(y.size - y.sum())
    return (ranks[y > 0].sum() - p * (p + 1) / 2.0) / (p * n)


def test_scoring_a_checkpoint_from_serving_engines(tmp_path):
    path, text = _bundled(tmp_path)
    data = parse_libffm(text)
    n = data.n_rows
    first = run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "1", "--checkpoint_path", "ck"])
    assert "epoch 1 train time" in first and not SERVING_LINE.search(first)
    score = BASE + ["--resume_from", "ck", "--n_epochs", "0", "--predict_data", path, "--metrics", "auc"]
    out = {}
    for fmt in ("none", "f32", "f16"):
        flag = [] if fmt == "none" else ["--serve_weights", fmt]
        out[fmt] = run_cli(tmp_path, score + ["--predict_out", fmt + ".txt"] + flag)
        assert SCORED_LINE.findall(out[fmt]) == [str(n)], out[fmt]
    # without the flag nothing is said about serving; with it, the format and the bytes of the formulas
    assert not SERVING_LINE.search(out["none"])
    L = F * K
    assert SERVING_LINE.findall(out["f32"]) == [("f32", str(4 + 4 * NF + 4 * NF * L))]
    assert SERVING_LINE.findall(out["f16"]) == [("f16", str(4 + 4 * NF + 2 * NF * L))]
    # fp32 serving: the score file byte for byte, and every other line printed (the AUC lines of --metrics auc,
    # where the run prints any, among them)
    a = (tmp_path / "none.txt").read_bytes()
    assert len(a) > 0 and (tmp_path / "f32.txt").read_bytes() == a
    for fmt in ("f32", "f16"):
        assert without_times(SERVING_LINE.sub("", out[fmt])) == without_times(out["none"]), out[fmt]
    # fp16 serving: the binding's fp16 serving engine, filled from the reproduction of the trained model
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    train_online(t, data, BATCH, fa.default_batch_ramp(1e-4), 1)
    s = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True, serve="f16")
    s.load_sparse_weights(t.sparse_state())
    want = np.concatenate([s.predict_batch(data.rows(p, min(n, p + BATCH)), output_prob=True)[0] for p in range(0, n, BATCH)])
    p16, _ = read_scores(tmp_path / "f16.txt")
    assert_bitwise(p16, want, "CLI --serve_weights f16 against the binding's fp16 serving engine")
    # ... which is also what pack_from makes of the same training engine
    s2 = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, serve="f16", skip_init=True)
    s2.pack_from(t)
    assert_bitwise(s2.get_weights()["vec_w"], s.get_weights()["vec_w"], "load_sparse_weights against pack_from")
    for e in (t, s, s2):
        e.close()
    # the quality of the format on this model: recorded (profiles/serve_weights.md), not asserted
    p32, _ = read_scores(tmp_path / "none.txt")
    y = data.label.astype(np.float64)
    for name, p in (("f32", p32.astype(np.float64)), ("f16", p16.astype(np.float64))):
        ll = float(np.mean(-(y * np.log(p) + (1 - y) * np.log1p(-p))))
        print("serve quality %s: mean logloss %.9f, auc %.9f" % (name, ll, rank_auc(p, data.label)))
    print("serve quality: %d of %d probabilities differ between f32 and f16, largest difference %.3g"
          % (int((p32 != p16).sum()), n, float(np.abs(p32 - p16).max())))
