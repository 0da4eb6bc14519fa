"""The trainer CLI's --metrics auc: after every loss line one line with the AUC of the same rows, from the
engine's device histogram -- `epoch N train auc: ...` (the pre-update predictions of the epoch:
progressive validation) and `epoch N eval auc: ...` --, in online and offline mode and with --n_gpus 2;
the printed numbers are what the Python binding computes on the same rows in the same schedule, and
without the flag nothing printed changes.

Two notes on the cases.  (1) --n_gpus > 1 needs per-field id ranges (--field_ranges uniform), which the
bundled libffm_data.txt does not have (field 0 holds id 3736, field 2 id 9729): the two-shard case runs
on generated rows laid out per field, as tests/test_host.py's does.  (2) Offline mode visits the rows in
a seeded std::shuffle, which Python cannot replay; with one block per epoch (--batch_size above the row
count, --batch_ramp 0) every row's pre-update logit is computed from the epoch-start weights, so the
epoch's training histogram does not depend on the order at all, and the model after it only through the
association order of the block's folded updates -- that case is compared with the file-order block."""
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
from util import GOLDEN

pytestmark = pytest.mark.gpu

AUC_LINE = re.compile(r"^epoch (\d+) (train|eval) auc: (\S+) \(\+-(\S+)\)$", re.M)


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


def auc_text(m):
    return "%.6f" % m["auc"], "%.1e" % m["auc_slack"]


def replay(model, data, batch, ramp, epochs):
    """The online trainer's schedule through the Python binding: rows in file order, block t of
    min(batch, max(1, rows_seen / ramp)) rows (ramp 0: batch), then the file again in full blocks through
    predict.  Returns [(epoch, "train" | "eval", auc, slack) as printed]."""
    model.metrics_enable(eval=True, train=True)
    total, seen, lines = data.n_rows, 0, []
    for ep in range(1, epochs + 1):
        pos = 0
        while pos < total:
            n = min(batch, max(1, seen // ramp)) if ramp > 0 else batch
            n = min(n, total - pos)
            model.train_batch(data.rows(pos, pos + n))
            seen += n
            pos += n
        lines.append((str(ep), "train") + auc_text(model.metrics("train", reset=True)))
        for pos in range(0, total, batch):
            model.predict_batch(data.rows(pos, min(total, pos + batch)))
        lines.append((str(ep), "eval") + auc_text(model.metrics("eval", reset=True)))
    return lines


def check_lines(stdout, epochs):
    """Exactly one auc line behind each loss line; returns them as AUC_LINE's groups."""
    text = stdout.splitlines()
    for i, line in enumerate(text):
        m = re.match(r"epoch (\d+) (train|eval) time: .* (train|eval) loss: ", line)
        if m:
            assert re.match(r"epoch %s %s auc: [0-9.]+ \(\+-[0-9.e+-]+\)$" % (m.group(1), m.group(2)), text[i + 1]), text[i:i + 2]
    got = AUC_LINE.findall(stdout)
    assert [g[:2] for g in got] == [(str(ep), ch) for ep in range(1, epochs + 1) for ch in ("train", "eval")], stdout
    return got


def test_online_prints_the_auc_the_binding_computes(tmp_path):
    path, text = _bundled(tmp_path)
    base = ["--train_data", path, "--eval_data", path, "--model_type", "FFM", "--online", "true", "--batch_size", "256",
            "--n_epochs", "2"]
    with_flag = run_cli(tmp_path, base + ["--metrics", "auc"])
    got = check_lines(with_flag, 2)
    e = fa.Engine("FFM", 10000, 8, 16, max_batch_rows=256, max_batch_nnz=256 * 8)
    want = replay(e, parse_libffm(text), 256, fa.default_batch_ramp(1e-4), 2)
    e.close()
    assert got == want, (got, want)
    # without the flag: the same bytes as before it existed -- no auc line, everything else unchanged
    plain = run_cli(tmp_path, base)
    assert " auc: " not in plain
    assert without_times(AUC_LINE.sub("", with_flag).replace("\n\n", "\n")) == without_times(plain)
    assert without_times(run_cli(tmp_path, base + ["--metrics", "none"])) == without_times(plain)
    main_bin, _ = fa.build_host()
    bad = subprocess.run([main_bin] + base + ["--metrics", "roc"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--metrics takes auc or none" in bad.stderr


def test_offline_prints_the_auc_the_binding_computes(tmp_path):
    path, text = _bundled(tmp_path)
    base = ["--train_data", path, "--eval_data", path, "--model_type", "FFM", "--online", "false"]
    # one block per epoch: the case Python can compute (see the module docstring)
    one = ["--batch_size", "16384", "--batch_ramp", "0", "--n_epochs", "1"]
    with_flag = run_cli(tmp_path, base + one + ["--metrics", "auc"])
    got = check_lines(with_flag, 1)
    e = fa.Engine("FFM", 10000, 8, 16, max_batch_rows=16384, max_batch_nnz=16384 * 8)
    want = replay(e, parse_libffm(text), 16384, 0, 1)
    e.close()
    assert got == want, (got, want)
    # the usual shape -- shuffled blocks under the ramp, two epochs: the lines are there, and the run
    # without the flag prints the same losses and nothing else
    many = ["--batch_size", "256", "--n_epochs", "2"]
    with_flag = run_cli(tmp_path, base + many + ["--metrics", "auc"])
    for _, _, auc, slack in check_lines(with_flag, 2):
        assert 0.0 < float(auc) < 1.0 and 0.0 <= float(slack) <= 0.5
    plain = run_cli(tmp_path, base + many)
    assert " auc: " not in plain
    assert without_times(AUC_LINE.sub("", with_flag).replace("\n\n", "\n")) == without_times(plain)


def test_two_shards_print_the_auc_the_group_computes(tmp_path):
    F, per, k, rows, batch = 12, 500, 8, 4000, 512
    data = synth.Generator(F, F * per, "zipf", seed=5).block(rows)
    text = synth.to_libffm_text(data)
    path = tmp_path / "s.ffm"
    path.write_text(text)
    base = ["--train_data", str(path), "--eval_data", str(path), "--model_type", "FFM", "--n_fields", str(F),
            "--n_feats", str(F * per), "--n_factors", str(k), "--online", "true", "--n_epochs", "2",
            "--batch_size", str(batch), "--batch_ramp", "32", "--w_alpha", "0.05", "--w_l1", "0.01", "--w_l2", "0.1", "--field_ranges", "uniform",
            "--n_gpus", "2"]
    env = {"FTRL_SAME_DEVICE": "1"}
    with_flag = run_cli(tmp_path, base + ["--metrics", "auc"], env)
    assert "2 field-pair shards" in with_flag
    got = check_lines(with_flag, 2)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    g = fa.Group([0, 0], "FFM", F * per, F, k, w_alpha=0.05, w_l1=0.01, w_l2=0.1, max_batch_rows=batch,
                 max_batch_nnz=batch * F, field_start=fs)
    want = replay(g, parse_libffm(text), batch, 32, 2)
    g.close()
    assert got == want, (got, want)
    plain = run_cli(tmp_path, base, env)
    assert " auc: " not in plain
    assert without_times(AUC_LINE.sub("", with_flag).replace("\n\n", "\n")) == without_times(plain)
