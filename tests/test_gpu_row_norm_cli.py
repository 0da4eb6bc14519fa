"""The trainer CLI's --normalize_rows on the bundled libffm data: a run with the flag prints the loss and AUC lines and
writes the --predict_out bytes of a run WITHOUT it on a copy of the file whose values were normalised on the host with
fa.normalize_rows and printed with 9 significant digits (which round-trip a float32 exactly) -- plainly, and under
--hash_feats true --bucket_fields 7, where the copy is prepared with the binding's host functions (bucket_ids, hash_ids,
normalize_rows: a bucketed entry counts as the 1 it became, the ids that decide are the hashed ones); the `normalized
rows:` line; a checkpoint saved with the flag is refused without it and the other way round; a serving engine that is
handed the flag again scores what the training run scored.
(_bundled / parse_libffm / run_cli / without_times are those of tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import bucket_ref
import ftrl_ffm_amd as fa
from test_gpu_scores_cli import _bundled, parse_libffm, run_cli, without_times

pytestmark = pytest.mark.gpu

BATCH, F, NF, FIELD, B = 256, 8, 10000, 7, 16
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1", "--metrics", "auc"]
HASHED = ["--hash_feats", "true", "--field_ranges", "uniform"]
LINE = re.compile(r"^.*(?:loss|auc).*$", re.M | re.I)
NORM_LINE = re.compile(r"^normalized rows: (\d+) scaled, (\d+) left as they came \(zero or non-finite norm\)\n", re.M)


def to_text(data, val):
    """The block as a libffm file, values with 9 significant digits."""
    lines = []
    for r in range(data.n_rows):
        b, e = int(data.row_ptr[r]), int(data.row_ptr[r + 1])
        lines.append(" ".join([str(int(data.label[r]))] + ["%d:%d:%.9g" % (data.field[p], data.feat[p], val[p]) for p in range(b, e)]))
    return "\n".join(lines) + "\n"


def unscaled_rows(data, keep, val):
    s = np.add.reduceat(np.where(keep, val.astype(np.float64) ** 2, 0.0), data.row_ptr[:-1].astype(np.int64)) if val.size else np.zeros(0)
    empty = np.diff(data.row_ptr) == 0
    return int(np.count_nonzero(empty | (s == 0)))


_runs = {}


def runs(tmp_path):
    """The flagged runs and the plain runs on the normalised copies: made once, shared."""
    if _runs:
        return _runs
    path, text = _bundled(tmp_path)
    data = parse_libffm(text)
    io = ["--eval_data", path, "--predict_data", path]
    # ---- plainly: ids >= n_feats are erased, left out of the sum and scaled
    keep = (data.feat >= 0) & (data.feat < NF) & (data.field >= 0) & (data.field < F)
    val = fa.normalize_rows(data.row_ptr, data.field, data.feat, data.val, NF, F)
    assert np.array_equal(np.array([np.float32("%.9g" % v) for v in val[:2000]], np.float32).view(np.uint32), val[:2000].view(np.uint32))
    assert not (val == 0).any(), "no value leaves the file by becoming 0"
    (tmp_path / "normed.txt").write_text(to_text(data, val))
    _runs["flag"] = run_cli(tmp_path, BASE + io + ["--train_data", path, "--normalize_rows", "true", "--predict_out", "pf.txt", "--checkpoint_path", "ck_norm"])
    _runs["copy"] = run_cli(tmp_path, BASE + ["--train_data", "normed.txt", "--eval_data", "normed.txt", "--predict_data", "normed.txt",
                                              "--predict_out", "pc.txt"])
    _runs["plain"] = run_cli(tmp_path, BASE + io + ["--train_data", path, "--predict_out", "pp.txt", "--checkpoint_path", "ck_plain"])
    _runs["unscaled"] = unscaled_rows(data, keep, data.val)
    # ---- hashed and bucketed: field 7 becomes 7:<bucket>:1, then every id is hashed into its field's range
    counts = bucket_ref.np_hist(data.field, data.val, F)[0]
    edges = fa.bucket_edges(counts[FIELD], B)
    ft, v, hit = fa.bucket_ids(data.field, data.feat, data.val, F, {FIELD: edges})
    assert hit.any() and (v[hit] == 1).all()
    fs = (np.arange(F + 1) * (NF // F)).astype(np.int32)
    hashed = fa.hash_ids(data.field, ft, NF, field_start=fs, n_fields=F)
    vb = fa.normalize_rows(data.row_ptr, data.field, hashed, v, NF, F)
    assert not (vb == 0).any()
    bucketed = parse_libffm(text)
    bucketed.feat = ft
    (tmp_path / "normed_b.txt").write_text(to_text(bucketed, vb))
    _runs["flag_b"] = run_cli(tmp_path, BASE + HASHED + io + ["--train_data", path, "--bucket_fields", str(FIELD), "--n_buckets", str(B),
                                                              "--normalize_rows", "true", "--predict_out", "pfb.txt"])
    _runs["copy_b"] = run_cli(tmp_path, BASE + HASHED + ["--train_data", "normed_b.txt", "--eval_data", "normed_b.txt",
                                                         "--predict_data", "normed_b.txt", "--predict_out", "pcb.txt"])
    for name in ("pf", "pc", "pp", "pfb", "pcb"):
        _runs[name] = (tmp_path / (name + ".txt")).read_bytes()
    _runs.update(dir=tmp_path, path=path, n_rows=data.n_rows)
    return _runs


def test_flag_gives_the_plain_run_on_the_normalised_copy(tmp_path):
    r = runs(tmp_path)
    lines = {k: LINE.findall(without_times(NORM_LINE.sub("", r[k]))) for k in ("flag", "copy", "plain")}
    assert len(lines["flag"]) >= 3 and any("train loss" in ln for ln in lines["flag"]) and any("auc" in ln.lower() for ln in lines["flag"])
    assert lines["flag"] == lines["copy"]
    assert len(r["pf"]) > 0 and r["pf"] == r["pc"]
    assert lines["plain"] != lines["flag"] and r["pp"] != r["pf"], "the data's rows are not of unit length as they come"


def test_flag_with_hashing_and_buckets(tmp_path):
    r = runs(tmp_path)
    lines = {k: LINE.findall(without_times(NORM_LINE.sub("", r[k]))) for k in ("flag_b", "copy_b")}
    keep = [ln for ln in lines["flag_b"] if not ln.startswith("value buckets") and not ln.startswith("field ")]
    assert len(keep) >= 3 and keep == lines["copy_b"]
    assert len(r["pfb"]) > 0 and r["pfb"] == r["pcb"] and r["pfb"] != r["pf"]


def test_the_normalized_rows_line(tmp_path):
    r = runs(tmp_path)
    got = NORM_LINE.findall(r["flag"])
    # one epoch of training and its evaluation, both through the training engine; the scoring pass comes after the line
    assert got == [(str(2 * (r["n_rows"] - r["unscaled"])), str(2 * r["unscaled"]))], r["flag"]
    assert r["flag"].index("normalized rows:") > r["flag"].index("train loss")
    assert "scored" not in r["flag"] or r["flag"].index("normalized rows:") < r["flag"].index("scored")
    assert len(NORM_LINE.findall(r["flag_b"])) == 1
    assert "normalized rows" not in r["plain"] and "normalized rows" not in r["copy"]


def test_checkpoints_record_the_setting(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    main_bin, _ = fa.build_host()
    score = ["--model_type", "FFM", "--batch_size", str(BATCH), "--n_epochs", "0", "--predict_data", r["path"], "--predict_out", "x.txt"]
    out = subprocess.run([main_bin] + score + ["--resume_from", "ck_norm"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "ck_norm: was saved with --normalize_rows, this model is the other variant" in out.stderr, out.stderr
    out = subprocess.run([main_bin] + score + ["--resume_from", "ck_plain", "--normalize_rows", "true"], cwd=d, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "ck_plain: was saved without --normalize_rows, this model is the other variant" in out.stderr, out.stderr
    out = subprocess.run([main_bin] + score + ["--resume_from", "ck_norm", "--normalize_rows", "true", "--n_gpus", "2", "--field_ranges", "uniform"],
                         cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and out.stdout == "" and "--n_gpus > 1 is not allowed with it" in out.stderr


def test_saved_model_scored_with_the_flag_again(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    score = ["--model_type", "FFM", "--batch_size", str(BATCH), "--resume_from", "ck_norm", "--n_epochs", "0", "--normalize_rows", "true",
             "--predict_data", r["path"]]
    run_cli(d, score + ["--predict_out", "s_train.txt"])
    run_cli(d, score + ["--predict_out", "s_serve.txt", "--serve_weights", "f32"])
    assert (d / "s_train.txt").read_bytes() == r["pf"] and (d / "s_serve.txt").read_bytes() == r["pf"]
