"""The trainer CLI's --min_count / --rare_ids @FILE / --rare_ids_out on the bundled libffm data: the counting run
prints the figures the numpy restatement gives (tests/rare_ref.py); a run handed the map in a file prints the same
loss lines and writes the same scores; both equal a run WITHOUT either flag on a copy of the file in which the rare
ids are spelled 2147483647; a saved model scored with the map from the file -- on a training and on a serving engine
-- gives the same scores again; --field_ranges counted sizes the ranges by the ids that stay.
(_bundled / parse_libffm / run_cli / without_times are those of tests/test_gpu_scores_cli.py.)"""
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
import rare_ref
import sketch_ref
from test_gpu_scores_cli import _bundled, parse_libffm, run_cli, without_times

pytestmark = pytest.mark.gpu

BATCH, N_FEATS, F, T, BITS = 256, 10000, 8, 3, 16  # (BITS: --rare_bits' default for 10000 features)
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1", "--hash_feats", "true"]
RARE_LINE = re.compile(r"^rare ids: counted (\d+) rows \((\d+) entries, (\d+) erased\) in [0-9.]+ s; (\d+) of 2\^(\d+) slots kept "
                       r"at min_count (\d+), (\d+) entries folded\n", re.M)
FIELD_LINE = re.compile(r"^field (\d+): ~(\d+) distinct ids, ids \[(\d+), (\d+)\)\n", re.M)
LOSS_LINE = re.compile(r"^.*loss.*$", re.M)


def keep_map(data):
    counts, n_valid, n_bad = rare_ref.np_counts(data.field, data.feat, F, BITS, T)
    words, kept, folded = rare_ref.np_keep(counts, T)
    return words, kept, folded, n_valid, n_bad


def folded_text(text, words):
    """The file with every rare id spelled 2147483647 (tokens whose value is 0 are dropped by the parser: as they are)."""
    out = []
    for line in text.splitlines():
        t = line.split()
        toks = [tok.split(":") for tok in t[1:]]
        fld = np.array([int(f) for f, _, _ in toks], np.int32)
        ids = np.array([int(i) for _, i, _ in toks], np.int32)
        new = rare_ref.np_fold(fld, ids, F, BITS, words)
        out.append(" ".join([t[0]] + ["%s:%d:%s" % (f, n, v) for (f, _, v), n in zip(toks, new)]))
    return "\n".join(out) + "\n"


_runs = {}


def runs(tmp_path):
    """The counting run, the run from the file, the run on the folded copy: made once, shared, read-only."""
    if not _runs:
        path, text = _bundled(tmp_path)
        data = parse_libffm(text)
        _runs["data"] = data
        _runs["map"] = keep_map(data)
        common = BASE + ["--field_ranges", "uniform", "--eval_data", path, "--predict_data", path]
        _runs["a"] = run_cli(tmp_path, common + ["--train_data", path, "--min_count", str(T), "--rare_ids_out", "m.rare",
                                                 "--predict_out", "pa.txt", "--checkpoint_path", "ck"])
        _runs["b"] = run_cli(tmp_path, common + ["--train_data", path, "--rare_ids", "@m.rare", "--predict_out", "pb.txt",
                                                 "--checkpoint_path", "cb"])
        _runs["ck_same"] = (tmp_path / "ck").read_bytes() == (tmp_path / "cb").read_bytes()
        (tmp_path / "folded.txt").write_text(folded_text(text, _runs["map"][0]))
        _runs["c"] = run_cli(tmp_path, BASE + ["--field_ranges", "uniform", "--eval_data", "folded.txt", "--predict_data", "folded.txt",
                                               "--train_data", "folded.txt", "--predict_out", "pc.txt"])
        _runs["plain"] = run_cli(tmp_path, common + ["--train_data", path, "--predict_out", "pp.txt"])
        for name in ("pa", "pb", "pc", "pp"):
            _runs[name] = (tmp_path / (name + ".txt")).read_bytes()
        _runs["dir"] = tmp_path
        _runs["path"] = path
    return _runs


def test_counting_run_prints_the_reference_figures(tmp_path):
    r = runs(tmp_path)
    words, kept, folded, n_valid, n_bad = r["map"]
    m = RARE_LINE.findall(r["a"])
    assert len(m) == 1, r["a"]
    assert tuple(int(x) for x in m[0]) == (r["data"].n_rows, n_valid + n_bad, n_bad, kept, BITS, T, folded)
    assert 0 < folded < n_valid and 0 < kept < 1 << BITS
    assert r["a"].index("rare ids: counted") < r["a"].index("train loss"), "counted before a model trains"
    assert not RARE_LINE.findall(r["b"]) and not RARE_LINE.findall(r["c"])


def test_map_from_a_file_and_folded_copy_give_the_counting_run(tmp_path):
    r = runs(tmp_path)
    loss = {k: LOSS_LINE.findall(without_times(r[k])) for k in ("a", "b", "c", "plain")}
    assert len(loss["a"]) >= 2 and any("train loss" in ln for ln in loss["a"])
    assert loss["a"] == loss["b"] == loss["c"]
    assert len(r["pa"]) > 0 and r["pa"] == r["pb"] == r["pc"]
    # ... which the run without the fold does not print or write
    assert loss["plain"] != loss["a"] and r["pp"] != r["pa"]
    # apart from the counting line and the line that names the map's file the two runs print the same, and they
    # leave the same checkpoint (the names are printed)
    strip = lambda s: "\n".join(ln for ln in without_times(RARE_LINE.sub("", s)).splitlines() if "m.rare" not in ln)  # noqa: E731
    assert strip(r["a"]) == strip(r["b"]).replace("saving to cb,", "saving to ck,")
    assert r["ck_same"]


def test_saved_model_scored_with_the_map_from_the_file(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    score = ["--model_type", "FFM", "--batch_size", str(BATCH), "--hash_feats", "true", "--field_ranges", "uniform", "--resume_from", "ck",
             "--n_epochs", "0", "--predict_data", r["path"]]
    run_cli(d, score + ["--rare_ids", "@m.rare", "--predict_out", "s_train.txt"])
    run_cli(d, score + ["--rare_ids", "@m.rare", "--predict_out", "s_serve.txt", "--serve_weights", "f32"])
    run_cli(d, score + ["--predict_out", "s_none.txt"])
    assert (d / "s_train.txt").read_bytes() == r["pa"] and (d / "s_serve.txt").read_bytes() == r["pa"]
    assert (d / "s_none.txt").read_bytes() != r["pa"], "the map is not in the checkpoint: without --rare_ids nothing folds"


def test_counted_ranges_are_sized_by_the_ids_that_stay(tmp_path):
    r = runs(tmp_path)
    data, words = r["data"], r["map"][0]
    out = run_cli(r["dir"], BASE + ["--train_data", r["path"], "--field_ranges", "counted", "--min_count", str(T)])
    kept = rare_ref.np_fold(data.field, data.feat, F, BITS, words)
    reg, _, _ = sketch_ref.np_sketch(data.field, kept, F)
    count = np.maximum(1, np.round(fa.sketch_estimate(reg))).astype(np.int64)
    ranges = sketch_ref.np_field_ranges(count, N_FEATS)
    lines = [tuple(int(x) for x in ln) for ln in FIELD_LINE.findall(out)]
    assert lines == [(f, int(count[f]), ranges[f], ranges[f + 1]) for f in range(F)]
    plain_count = np.maximum(1, np.round(fa.sketch_estimate(sketch_ref.np_sketch(data.field, data.feat, F)[0]))).astype(np.int64)
    assert (count <= plain_count).all() and count.sum() < plain_count.sum(), "folding shrinks the large fields"
    assert out.index("rare ids: counted") < out.index("field ranges: counted") < out.index("train loss")


def test_a_damaged_map_ends_the_run_before_it_trains(tmp_path):
    r = runs(tmp_path)
    d = r["dir"]
    raw = bytearray((d / "m.rare").read_bytes())
    raw[40] ^= 0x10  # (a byte of the header's checksum)
    (d / "bad.rare").write_bytes(bytes(raw))
    main_bin, _ = fa.build_host()
    args = BASE + ["--field_ranges", "uniform", "--train_data", r["path"]]
    out = subprocess.run([main_bin] + args + ["--rare_ids", "@bad.rare"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "bad.rare" in out.stderr and "checksum" in out.stderr and "train loss" not in out.stdout
    out = subprocess.run([main_bin] + args + ["--rare_ids", "@m.rare", "--n_fields", "9"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "m.rare" in out.stderr and "8 fields" in out.stderr and "train loss" not in out.stdout
    out = subprocess.run([main_bin] + args + ["--min_count", "3", "--hash_feats", "false"], cwd=d, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and out.stdout == "" and "--hash_feats true" in out.stderr
