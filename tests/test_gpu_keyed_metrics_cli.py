"""The trainer CLI's --auc_key_field: after every AUC line of --metrics auc one more with the grouped AUC of the
same rows, `epoch N <train|eval> gauc: G (K keys, M mixed, R of T rows; U unkeyed, O over capacity, X nan)`.  The
printed digits and every count are what the Python binding reports on the same rows in the same schedule (the
method of tests/test_gpu_metrics_cli.py: the online trainer's blocks replayed through Engine.train_batch /
predict_batch), and a second run that loads the first one's checkpoint and trains nothing (--resume_from ck
--n_epochs 0 --eval_data F) prints the same eval line, from a training engine and from an fp32 serving engine."""
import re
import subprocess

import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_metrics_cli import AUC_LINE, _bundled, parse_libffm, run_cli, without_times

pytestmark = pytest.mark.gpu

GAUC_LINE = re.compile(r"^epoch (\d+) (train|eval) gauc: (\S+) \((\d+) keys, (\d+) mixed, (\d+) of (\d+) rows; (\d+) unkeyed, "
                       r"(\d+) over capacity, (\d+) nan\)$", re.M)
BATCH = 256


def gauc_text(m):
    return ("%.6f" % m["gauc"],) + tuple(str(m[k]) for k in ("n_keys", "n_keys_mixed", "n_rows_mixed", "n_rows", "n_unkeyed",
                                                             "n_overflow", "n_nan"))


def replay(model, data, batch, ramp, epochs, key_field, capacity):
    """test_gpu_metrics_cli.replay with keyed capture on: [(epoch, channel, gauc, counts ...) as printed]."""
    model.metrics_enable(eval=True, train=True)
    model.metrics_key_field(key_field, capacity, eval=True, train=True)
    total, seen, lines = data.n_rows, 0, []
    for ep in range(1, epochs + 1):
        pos = 0
        while pos < total:
            n = min(batch, max(1, seen // ramp)) if ramp > 0 else batch
            n = min(n, total - pos)
            model.train_batch(data.rows(pos, pos + n))
            seen += n
            pos += n
        lines.append((str(ep), "train") + gauc_text(model.metrics_read_keyed("train", reset=True)))
        for pos in range(0, total, batch):
            model.predict_batch(data.rows(pos, min(total, pos + batch)))
        lines.append((str(ep), "eval") + gauc_text(model.metrics_read_keyed("eval", reset=True)))
    return lines


def test_online_prints_the_gauc_the_binding_computes(tmp_path):
    path, text = _bundled(tmp_path)
    data = parse_libffm(text)
    base = ["--train_data", path, "--eval_data", path, "--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH),
            "--n_epochs", "1", "--metrics", "auc"]
    first = run_cli(tmp_path, base + ["--auc_key_field", "0", "--checkpoint_path", "ck"])
    got = GAUC_LINE.findall(first)
    assert [g[:2] for g in got] == [("1", "train"), ("1", "eval")], first
    # every gauc line follows its auc line
    lines = first.splitlines()
    for i, line in enumerate(lines):
        m = re.match(r"epoch (\d+) (train|eval) auc: ", line)
        if m:
            assert lines[i + 1].startswith("epoch %s %s gauc: " % (m.group(1), m.group(2))), lines[i:i + 2]
    e = fa.Engine("FFM", 10000, 8, 16, max_batch_rows=BATCH, max_batch_nnz=BATCH * 8)
    want = replay(e, data, BATCH, fa.default_batch_ramp(1e-4), 1, 0, 1 << 24)
    e.close()
    assert got == want, (got, want)
    assert int(got[0][6]) + int(got[0][7]) + int(got[0][9]) == data.n_rows and got[0][8] == "0", got  # rows + unkeyed + nan
    # without the flag nothing else changes
    plain = run_cli(tmp_path, base)
    assert " gauc: " not in plain
    first_plain = re.sub(r"^saving to ck.*\n", "", GAUC_LINE.sub("", first).replace("\n\n", "\n"), flags=re.M)
    assert without_times(first_plain) == without_times(plain)
    # a small capacity: the rest is counted as over capacity, line by line what the binding reports
    small = run_cli(tmp_path, base + ["--auc_key_field", "0", "--auc_key_rows", "100"])
    e = fa.Engine("FFM", 10000, 8, 16, max_batch_rows=BATCH, max_batch_nnz=BATCH * 8)
    want_small = replay(e, data, BATCH, fa.default_batch_ramp(1e-4), 1, 0, 100)
    e.close()
    got_small = GAUC_LINE.findall(small)
    assert [g[:2] + g[6:] for g in got_small] == [w[:2] + w[6:] for w in want_small], (got_small, want_small)
    assert all(g[6] == "100" and int(g[8]) > 0 for g in got_small), got_small
    # the loaded model, trained no further: the same eval line, from a training engine and from a serving engine
    for serve in ([], ["--serve_weights", "f32"]):
        again = run_cli(tmp_path, ["--train_data", path, "--eval_data", path, "--model_type", "FFM", "--online", "true",
                                   "--batch_size", str(BATCH), "--resume_from", "ck", "--n_epochs", "0", "--metrics", "auc",
                                   "--auc_key_field", "0"] + serve)
        assert GAUC_LINE.findall(again) == [got[1]], again
        assert [a[:2] for a in AUC_LINE.findall(again)] == [("1", "eval")], again
    # refused before a device is opened
    main_bin, _ = fa.build_host()
    bad = subprocess.run([main_bin] + base + ["--auc_key_field", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "is not a field of this model" in bad.stderr and bad.stdout == ""
