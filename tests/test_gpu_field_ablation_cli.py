"""The trainer CLI's --field_importance: a model trained for one epoch and saved as a sparse checkpoint is loaded
by a second run (--resume_from ck --n_epochs 0 --eval_data F --metrics auc --field_importance true), plain and
from an fp32 serving engine; the per-field losses and AUCs it prints are, at the printed precision, what the
binding's predict_ablated / ablation_metrics give on the same file and the same model, both runs print the same
lines, and without the flag nothing else of the output changes.  (run_cli / parse_libffm / the schedule are
those of tests/test_gpu_scores_cli.py.)"""
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from test_gpu_scores_cli import BATCH, parse_libffm, run_cli, train_online, without_times

pytestmark = pytest.mark.gpu

NF, F, K, ROWS = 2000, 8, 4, 1000
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--learn", "true", "--n_feats", str(NF),
        "--n_fields", str(F), "--n_factors", str(K)]
SERVING_LINE = re.compile(r"^serving weights: (\w+), (\d+) bytes of model\n", re.M)
IMPORTANCE = re.compile(r"^(field importance: .*|field \d+: without it .*)\n", re.M)


def expected_lines(e, data):
    """The lines of run_importance for the fields from the binding: the file in blocks of BATCH rows through
    predict_ablated, the loss sums added in block order."""
    n = data.n_rows
    loss = np.zeros(F + 1)
    for p in range(0, n, BATCH):
        loss += e.predict_ablated(data.rows(p, min(n, p + BATCH)))[1]
    auc = [m["auc"] for m in e.ablation_metrics(reset=True)]
    lines = ["field importance: %d rows, loss %.6f, auc %.6f" % (n, loss[F] / n, auc[F])]
    for f in range(F):
        lines.append("field %d: without it loss %.6f (delta %+.6f), auc %.6f (delta %+.6f)"
                     % (f, loss[f] / n, (loss[f] - loss[F]) / n, auc[f], auc[f] - auc[F]))
    return lines


def test_field_importance_lines(tmp_path):
    text = synth.to_libffm_text(synth.Generator(F, NF, "zipf", seed=21).block(ROWS))
    path = tmp_path / "d.ffm"
    path.write_text(text)
    data = parse_libffm(text)
    assert data.n_rows == ROWS and (data.label > 0).any() and (data.label <= 0).any()
    first = run_cli(tmp_path, BASE + ["--train_data", str(path), "--n_epochs", "1", "--checkpoint_path", "ck"])
    assert "epoch 1 train time" in first and not IMPORTANCE.search(first)
    again = BASE + ["--train_data", str(path), "--resume_from", "ck", "--n_epochs", "0", "--eval_data", str(path), "--metrics", "auc"]
    out = {fmt: run_cli(tmp_path, again + ["--field_importance", "true"] + ([] if fmt == "none" else ["--serve_weights", fmt]))
           for fmt in ("none", "f32")}
    # the same model through the binding
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    train_online(t, data, BATCH, fa.default_batch_ramp(1e-4), 1)
    t.ablation_enable(auc=True)
    want = expected_lines(t, data)
    t.close()
    for fmt in ("none", "f32"):
        assert IMPORTANCE.findall(out[fmt]) == want, (fmt, out[fmt])
        assert "epoch 1 eval time" in out[fmt] and "epoch 1 eval auc" in out[fmt]  # after the one evaluation
        assert out[fmt].index("epoch 1 eval auc") < out[fmt].index("field importance:")
    assert without_times(SERVING_LINE.sub("", out["f32"])) == without_times(out["none"])
    # the ablation moved something: the fields do not all print the same loss
    assert len({line.split(" loss ")[1].split(" ")[0] for line in want[1:]}) > 1, want
    # without the flag: nothing of it; and with it, a training run prints what it printed, then the lines
    plain = run_cli(tmp_path, again)
    assert not IMPORTANCE.search(plain) and "eval time" not in plain  # (no evaluation either, as ever)
    train = BASE + ["--train_data", str(path), "--eval_data", str(path), "--n_epochs", "1", "--metrics", "auc"]
    a, b = run_cli(tmp_path, train), run_cli(tmp_path, train + ["--field_importance", "true"])
    assert not IMPORTANCE.search(a)
    assert IMPORTANCE.findall(b) == want
    assert without_times(IMPORTANCE.sub("", b)) == without_times(a)
