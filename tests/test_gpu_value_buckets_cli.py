"""The trainer CLI's --bucket_fields / --n_buckets / --buckets @FILE / --buckets_out on the bundled libffm data, whose
field 7 is a numeric column: the counting run prints the figures the numpy restatement gives (tests/bucket_ref.py); a
run handed the table in a file prints the same loss lines and writes the same scores; both equal a run WITHOUT either
flag on a copy of the file whose field-7 tokens are spelled 7:<bucket>:1; a saved model scored with the table from the
file -- on a training and on a serving engine -- gives the same scores again; --min_count never folds a bucketed
entry; --field_ranges counted takes a bucketed field's count as its edges + 2.
(_bundled / parse_libffm / run_cli / without_times are those of tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import bucket_ref
import ftrl_ffm_amd as fa
import rare_ref
from test_gpu_scores_cli import _bundled, parse_libffm, run_cli, without_times

pytestmark = pytest.mark.gpu

BATCH, F, FIELD, B = 256, 8, 7, 16
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1", "--hash_feats", "true"]
FLAGS = ["--bucket_fields", str(FIELD), "--n_buckets", str(B)]
BUCKET_FIELD_LINE = re.compile(r"^field (\d+): (\d+) values in (\d+) bins -> (\d+) buckets\n", re.M)
BUCKET_LINE = re.compile(r"^value buckets: counted (\d+) rows \((\d+) entries, (\d+) nan\) in [0-9.]+ s\n", re.M)
RANGE_LINE = re.compile(r"^field (\d+): ~(\d+) distinct ids, ids \[(\d+), (\d+)\)\n", re.M)
LOSS_LINE = re.compile(r"^.*loss.*$", re.M)


def reference(data):
    """(edges, values counted, bins in use, entries, NaNs) of field 7 by the reference alone."""
    counts, n_valid, n_bad, n_nan = bucket_ref.np_hist(data.field, data.val, F)
    edges, dropped = bucket_ref.edges(counts[FIELD], B)
    assert edges.size + 1 >= 3 and dropped >= 1, (edges.size, dropped)
    return edges, int(counts[FIELD].sum()), int(np.count_nonzero(counts[FIELD])), n_valid + n_bad, n_nan


def bucketed_text(text, edges):
    """The file with every field-7 token spelled 7:<bucket>:1 (tokens whose value is 0 are dropped by the parser: as
    they are)."""
    out = []
    for line in text.splitlines():
        t = line.split()
        toks = []
        for tok in t[1:]:
            f, i, v = tok.split(":")
            if int(f) == FIELD and np.float32(v) != 0:
                b, nan = bucket_ref.np_bin(np.array([v], np.float32))
                assert not nan[0]
                tok = "%d:%d:1" % (FIELD, int(bucket_ref.np_bucket(edges, b)[0]))
            toks.append(tok)
        out.append(" ".join([t[0]] + toks))
    return "\n".join(out) + "\n"


_runs = {}


def runs(tmp_path):
    """The counting run, the run from the file, the run on the bucketed copy, the run without: made once, shared."""
    if not _runs:
        path, text = _bundled(tmp_path)
        data = parse_libffm(text)
        _runs["data"] = data
        _runs["ref"] = reference(data)
        common = BASE + ["--field_ranges", "uniform", "--eval_data", path, "--predict_data", path]
        _runs["a"] = run_cli(tmp_path, common + FLAGS + ["--train_data", path, "--buckets_out", "b.txt", "--predict_out", "pa.txt",
                                                         "--checkpoint_path", "ck"])
        _runs["b"] = run_cli(tmp_path, common + ["--train_data", path, "--buckets", "@b.txt", "--predict_out", "pb.txt",
                                                 "--checkpoint_path", "cb"])
        _runs["ck_same"] = (tmp_path / "ck").read_bytes() == (tmp_path / "cb").read_bytes()
        (tmp_path / "bucketed.txt").write_text(bucketed_text(text, _runs["ref"][0]))
        _runs["c"] = run_cli(tmp_path, BASE + ["--field_ranges", "uniform", "--eval_data", "bucketed.txt", "--predict_data", "bucketed.txt",
                                               "--train_data", "bucketed.txt", "--predict_out", "pc.txt"])
        _runs["plain"] = run_cli(tmp_path, common + ["--train_data", path, "--predict_out", "pp.txt"])
        for name in ("pa", "pb", "pc", "pp"):
            _runs[name] = (tmp_path / (name + ".txt")).read_bytes()
        _runs["dir"] = tmp_path
        _runs["path"] = path
    return _runs


def test_counting_run_prints_the_reference_figures(tmp_path):
    r = runs(tmp_path)
    edges, n_values, n_bins, n_entries, n_nan = r["ref"]
    per_field = BUCKET_FIELD_LINE.findall(r["a"])
    assert [tuple(int(x) for x in m) for m in per_field] == [(FIELD, n_values, n_bins, edges.size + 1)], r["a"]
    total = BUCKET_LINE.findall(r["a"])
    assert len(total) == 1 and tuple(int(x) for x in total[0]) == (r["data"].n_rows, n_entries, n_nan), r["a"]
    assert r["a"].index("field %d: " % FIELD) < r["a"].index("value buckets: counted") < r["a"].index("train loss"), "counted before a model trains"
    assert not BUCKET_LINE.findall(r["b"]) and not BUCKET_LINE.findall(r["c"])
    # the table's file: the header and field 7's line
    lines = (r["dir"] / "b.txt").read_text().splitlines()
    assert lines == ["FFMBUCKETS 1 %d" % F, " ".join(str(x) for x in [FIELD, edges.size] + edges.tolist())]


def test_table_from_a_file_and_bucketed_copy_give_the_counting_run(tmp_path):
    r = runs(tmp_path)
    loss = {k: LOSS_LINE.findall(without_times(r[k])) for k in ("a", "b", "c", "plain")}
    assert len(loss["a"]) >= 2 and any("train loss" in ln for ln in loss["a"])
    assert loss["a"] == loss["b"] == loss["c"]
    assert len(r["pa"]) > 0 and r["pa"] == r["pb"] == r["pc"]
    # ... which the run without the table does not print or write
    assert loss["plain"] != loss["a"] and r["pp"] != r["pa"]
    assert r["ck_same"], "the two runs leave the same checkpoint"


def test_saved_model_scored_with_the_table_from_the_file(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    score = ["--model_type", "FFM", "--batch_size", str(BATCH), "--hash_feats", "true", "--field_ranges", "uniform", "--resume_from", "ck",
             "--n_epochs", "0", "--predict_data", r["path"]]
    run_cli(d, score + ["--buckets", "@b.txt", "--predict_out", "s_train.txt"])
    run_cli(d, score + ["--buckets", "@b.txt", "--predict_out", "s_serve.txt", "--serve_weights", "f32"])
    run_cli(d, score + ["--predict_out", "s_none.txt"])
    assert (d / "s_train.txt").read_bytes() == r["pa"] and (d / "s_serve.txt").read_bytes() == r["pa"]
    assert (d / "s_none.txt").read_bytes() != r["pa"], "the table is not in the checkpoint: without --buckets nothing is bucketed"


def test_min_count_does_not_fold_bucketed_entries(tmp_path):
    """--min_count 3 counts RAW ids, so the bucket ids (7, b) are ids it never saw: a fold behind the bucket step
    would send them all to field 7's rare id.  The run equals the run on the bucketed copy, where the same flag
    counts the spelled-out bucket ids as frequent and keeps them."""
    r = runs(tmp_path)
    data, edges, bits = r["data"], r["ref"][0], 20
    # on the reference alone: the raw file's map would fold bucket ids, and the two files' maps agree on every other entry
    copy = parse_libffm((r["dir"] / "bucketed.txt").read_text())
    m_raw = rare_ref.np_keep(rare_ref.np_counts(data.field, data.feat, F, bits, 3)[0], 3)[0]
    m_copy = rare_ref.np_keep(rare_ref.np_counts(copy.field, copy.feat, F, bits, 3)[0], 3)[0]
    ids = np.arange(edges.size + 1, dtype=np.int32)
    fld = np.full(ids.size, FIELD, np.int32)
    assert (rare_ref.np_fold(fld, ids, F, bits, m_raw) == rare_ref.RARE_ID).any(), "the raw file's map folds bucket ids"
    assert (rare_ref.np_fold(fld, ids, F, bits, m_copy) == ids).all(), "the copy's map keeps them"
    other = data.field != FIELD
    assert np.array_equal(rare_ref.np_fold(data.field[other], data.feat[other], F, bits, m_raw),
                          rare_ref.np_fold(data.field[other], data.feat[other], F, bits, m_copy))
    rare = ["--min_count", "3", "--rare_bits", str(bits), "--field_ranges", "uniform"]
    a = run_cli(r["dir"], BASE + rare + FLAGS + ["--train_data", r["path"], "--predict_data", r["path"], "--predict_out", "ra.txt"])
    c = run_cli(r["dir"], BASE + rare + ["--train_data", "bucketed.txt", "--predict_data", "bucketed.txt", "--predict_out", "rc.txt"])
    assert a.index("value buckets: counted") < a.index("rare ids: counted") < a.index("train loss")
    assert LOSS_LINE.findall(without_times(a)) == LOSS_LINE.findall(without_times(c))
    assert (r["dir"] / "ra.txt").read_bytes() == (r["dir"] / "rc.txt").read_bytes() != r["pa"]


def test_counted_ranges_take_a_bucketed_field_as_its_edges_plus_two(tmp_path):
    r = runs(tmp_path)
    edges = r["ref"][0]
    out = run_cli(r["dir"], BASE + FLAGS + ["--train_data", r["path"], "--field_ranges", "counted"])
    plain = run_cli(r["dir"], BASE + ["--train_data", r["path"], "--field_ranges", "counted"])
    got = {int(f): (int(n), int(lo), int(hi)) for f, n, lo, hi in RANGE_LINE.findall(out)}
    was = {int(f): (int(n), int(lo), int(hi)) for f, n, lo, hi in RANGE_LINE.findall(plain)}
    assert sorted(got) == sorted(was) == list(range(F))
    assert got[FIELD][0] == edges.size + 2 and was[FIELD][0] == 1, (got[FIELD], was[FIELD])
    assert all(got[f][0] == was[f][0] for f in range(F) if f != FIELD), "the other fields' counts are the sketch's"
    assert got[FIELD][2] - got[FIELD][1] >= edges.size + 2, "the range holds every bucket and the NaN id"
    assert out.index("value buckets: counted") < out.index("field ranges: counted") < out.index("train loss")


def test_a_damaged_table_ends_the_run_before_it_trains(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    lines = (d / "b.txt").read_text().splitlines()
    t = lines[1].split()
    t[2], t[3] = t[3], t[2]  # (two edges out of order)
    (d / "bad.txt").write_text(lines[0] + "\n" + " ".join(t) + "\n")
    main_bin, _ = fa.build_host()
    args = BASE + ["--field_ranges", "uniform", "--train_data", r["path"]]
    out = subprocess.run([main_bin] + args + ["--buckets", "@bad.txt"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "bad.txt" in out.stderr and "strictly ascending" in out.stderr and "train loss" not in out.stdout
    out = subprocess.run([main_bin] + args + ["--buckets", "@b.txt", "--n_fields", "9"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "b.txt" in out.stderr and "8 fields" in out.stderr and "train loss" not in out.stdout
    out = subprocess.run([main_bin] + args + FLAGS + ["--hash_feats", "false"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and out.stdout == "" and "--hash_feats true" in out.stderr
