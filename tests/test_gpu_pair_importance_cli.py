"""The trainer CLI's --pair_importance on a synthetic 4-field file of a few hundred rows: the whole loss and every
listed pair's loss (and, with --metrics auc, the AUCs) are, at the printed precision, what the binding's
predict_pair_ablated / pair_ablation_metrics give on the same file and the same model; without the flag the
stdout and the model file's bytes are those of a run that does not name it; --resume_from ck --n_epochs 0, with and
without --serve_weights f16, prints the same structure.  (run_cli / parse_libffm / the schedule are those of
tests/test_gpu_scores_cli.py.)"""
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from test_gpu_scores_cli import BATCH, parse_libffm, run_cli, train_online, without_times

pytestmark = pytest.mark.gpu

NF, F, K, ROWS = 400, 4, 4, 300
V = F * (F + 1) // 2
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--learn", "true", "--n_feats", str(NF),
        "--n_fields", str(F), "--n_factors", str(K)]
SERVING_LINE = re.compile(r"^serving weights: (\w+), (\d+) bytes of model\n", re.M)
LINES = re.compile(r"^(pair importance: .*|pair \d+ \d+: without it .*)\n", re.M)
NUMBER = re.compile(r"[-+]?\d+\.\d+")


def expected_lines(e, data, auc):
    """The lines of run_importance for the pairs from the binding: the file in blocks of BATCH rows through
    predict_pair_ablated (scores left on the device), the loss sums added in block order."""
    n = data.n_rows
    loss = np.zeros(V + 1)
    for p in range(0, n, BATCH):
        loss += e.predict_pair_ablated(data.rows(p, min(n, p + BATCH)), scores=False)[1]
    a = [m["auc"] for m in e.pair_ablation_metrics(reset=True)] if auc else None
    lines = ["pair importance: %d score histograms, %d bytes of device memory" % (V + 1, (V + 1) * (2 * fa.METRIC_BINS + 1) * 8)] if auc else []
    lines.append("pair importance: %d rows, loss %.6f" % (n, loss[V] / n) + (", auc %.6f" % a[V] if auc else ""))
    listed = 0
    for v in range(V):
        if loss[v] == loss[V]:
            continue
        f, g = fa.pair_fields(F, v)
        lines.append("pair %d %d: without it loss %.6f (delta %+.6f)" % (f, g, loss[v] / n, (loss[v] - loss[V]) / n) +
                     (", auc %.6f (delta %+.6f)" % (a[v], a[v] - a[V]) if auc else ""))
        listed += 1
    lines.append("pair importance: %d of %d pairs listed, %d never changed a row" % (listed, V, V - listed))
    return lines


def test_pair_importance_lines(tmp_path):
    text = synth.to_libffm_text(synth.Generator(F, NF, "zipf", seed=23).block(ROWS))
    path = tmp_path / "d.ffm"
    path.write_text(text)
    data = parse_libffm(text)
    assert data.n_rows == ROWS and (data.label > 0).any() and (data.label <= 0).any()
    train = BASE + ["--train_data", str(path), "--eval_data", str(path), "--n_epochs", "1"]
    # without the flag: the stdout and the model's bytes of a run that does not name it
    plain = run_cli(tmp_path, train + ["--model_path", "plain.txt", "--checkpoint_path", "ck"])
    ck_plain = (tmp_path / "ck").read_bytes()
    with_flag = run_cli(tmp_path, train + ["--model_path", "named.txt", "--checkpoint_path", "ck", "--pair_importance", "true"])
    assert not LINES.search(plain)
    assert without_times(LINES.sub("", with_flag)).replace("named.txt", "plain.txt") == without_times(plain)
    for name in ("named.txt", "named.txt.nz"):
        assert (tmp_path / name).read_bytes() == (tmp_path / name.replace("named", "plain")).read_bytes(), name
    assert (tmp_path / "ck").read_bytes() == ck_plain
    # the same model through the binding
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    train_online(t, data, BATCH, fa.default_batch_ramp(1e-4), 1)
    t.pair_ablation_enable(auc=True)
    want_auc = expected_lines(t, data, True)  # (first: it reads the histograms of its own pass and zeroes them)
    want = expected_lines(t, data, False)
    t.close()
    assert LINES.findall(with_flag) == want, with_flag
    assert len(want) > 3, want  # pairs moved the loss sums
    assert with_flag.index("epoch 1 eval time") < with_flag.index("pair importance:")  # after the last evaluation
    # --resume_from ck --n_epochs 0: after the one evaluation of the loaded model, with the AUC parts; after
    # --field_importance's pass when both are given
    again = BASE + ["--train_data", str(path), "--resume_from", "ck", "--n_epochs", "0", "--eval_data", str(path), "--metrics", "auc",
                    "--pair_importance", "true"]
    out = {fmt: run_cli(tmp_path, again + ([] if fmt == "none" else ["--serve_weights", fmt])) for fmt in ("none", "f16")}
    assert LINES.findall(out["none"]) == want_auc, out["none"]
    assert out["none"].index("epoch 1 eval auc") < out["none"].index("pair importance:")
    both = run_cli(tmp_path, again + ["--field_importance", "true"])
    assert LINES.findall(both) == want_auc and both.index("field 3: without it") < both.index("pair importance:")
    # an fp16 serving engine: the same structure -- the same lines with other digits
    assert SERVING_LINE.search(out["f16"])
    got16 = LINES.findall(out["f16"])
    assert [NUMBER.sub("#", line) for line in got16] == [NUMBER.sub("#", line) for line in want_auc], out["f16"]
    assert got16[0] == want_auc[0] and got16[-1] == want_auc[-1]
