"""The trainer CLI's --field_ranges counted / @FILE / --field_ranges_out on the bundled libffm data (fields of 4556,
3204, 2, 21, 18, 18, 16 and 1 distinct ids): the counting pass gives the ranges the sketch's numpy restatement gives;
a run that is handed those ranges in a file prints and saves what the counting run does; both train as the binding
does with the same ranges; --field_ranges uniform prints what the commit before this feature printed
(tests/golden/field_sketch_cli/, recorded from its binary); the refusals come before a device is opened.
(_bundled / parse_libffm / run_cli / without_times / train_online are those of tests/test_gpu_scores_cli.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
import sketch_ref
from test_gpu_scores_cli import _bundled, parse_libffm, run_cli, without_times
from util import GOLDEN

pytestmark = pytest.mark.gpu

BATCH, N_FEATS, F, K = 256, 10000, 8, 16
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1", "--hash_feats", "true"]
# the runs whose output the commit before this feature recorded: name -> arguments after --train_data libffm_data.txt
# (the file by its name inside the working directory: the offline trainer prints the path it loads)
UNIFORM_RUNS = {
    "uniform_online_hashed": ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1",
                              "--hash_feats", "true", "--field_ranges", "uniform", "--eval_data", "libffm_data.txt", "--metrics", "auc"],
    "uniform_offline_hashed": ["--model_type", "FFM", "--online", "false", "--batch_size", str(BATCH), "--n_epochs", "2",
                               "--hash_feats", "true", "--field_ranges", "uniform", "--eval_data", "libffm_data.txt"],
    "none_online": ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH), "--n_epochs", "1",
                    "--field_ranges", "none", "--eval_data", "libffm_data.txt"],
}
FIELD_LINE = re.compile(r"^field (\d+): ~(\d+) distinct ids, ids \[(\d+), (\d+)\)\n", re.M)
SUMMARY_LINE = re.compile(r"^field ranges: counted from (\d+) rows \((\d+) entries, (\d+) erased\) in [0-9.]+ s; "
                          r"~(\d+) distinct ids for (\d+) features \(load ([0-9.]+)\)\n", re.M)


def without_range_lines(stdout):
    return SUMMARY_LINE.sub("", FIELD_LINE.sub("", without_times(stdout)))


_counted = {}


def counted_runs(tmp_path):
    """Run A (counted, ranges written) and run B (the same ranges read back): made once, shared, read-only."""
    if not _counted:
        path, text = _bundled(tmp_path)
        _counted["text"] = text
        _counted["a"] = run_cli(tmp_path, BASE + ["--train_data", path, "--field_ranges", "counted", "--field_ranges_out", "r.txt",
                                                  "--checkpoint_path", "ck"])
        _counted["ck_a"] = (tmp_path / "ck").read_bytes()
        os.remove(tmp_path / "ck")  # (both runs name their checkpoint alike: the name is printed)
        _counted["b"] = run_cli(tmp_path, BASE + ["--train_data", path, "--field_ranges", "@r.txt", "--checkpoint_path", "ck"])
        _counted["r"] = (tmp_path / "r.txt").read_text()
        _counted["ck_b"] = (tmp_path / "ck").read_bytes()
    return _counted


def expected_ranges(text):
    data = parse_libffm(text)
    reg, n_valid, n_bad = sketch_ref.np_sketch(data.field, data.feat, F)
    count = np.maximum(1, np.round(fa.sketch_estimate(reg))).astype(np.int64)
    assert np.allclose(fa.sketch_estimate(reg), sketch_ref.np_estimate(reg), rtol=1e-12, atol=0)
    return count, fa.field_ranges(count, N_FEATS), data, n_valid, n_bad


def test_counted_ranges_are_the_reference_ranges(tmp_path):
    runs = counted_runs(tmp_path)
    count, ranges, data, n_valid, n_bad = expected_ranges(runs["text"])
    assert runs["r"] == "".join("%d\n" % v for v in ranges)
    assert [int(v) for v in ranges] == sketch_ref.np_field_ranges(count, N_FEATS)
    lines = FIELD_LINE.findall(runs["a"])
    assert [tuple(int(x) for x in ln) for ln in lines] == [(f, int(count[f]), int(ranges[f]), int(ranges[f + 1])) for f in range(F)]
    # the sketch is within 5 % of the file's true cardinalities (here: exact for the small fields)
    truth = [np.unique(data.feat[data.field == f]).size for f in range(F)]
    assert all(abs(int(c) - t) <= 0.05 * t for c, t in zip(count, truth)), (count, truth)
    m = SUMMARY_LINE.findall(runs["a"])
    assert len(m) == 1
    rows, entries, erased, total, n_feats, load = m[0]
    assert (int(rows), int(entries), int(erased), int(total), int(n_feats)) == (data.n_rows, n_valid + n_bad, n_bad, int(count.sum()), N_FEATS)
    assert load == "%.3f" % (count.sum() / N_FEATS)
    assert runs["a"].index("field ranges: counted") < runs["a"].index("train loss"), "counted before a model trains"
    assert not FIELD_LINE.findall(runs["b"]) and not SUMMARY_LINE.findall(runs["b"])


def test_ranges_from_a_file_give_the_counting_run(tmp_path):
    runs = counted_runs(tmp_path)
    assert without_range_lines(runs["a"]) == without_times(runs["b"])
    assert "train loss" in runs["b"]
    assert runs["ck_a"] == runs["ck_b"] and len(runs["ck_a"]) > 0


def test_both_train_as_the_binding_does_with_those_ranges(tmp_path):
    runs = counted_runs(tmp_path)
    _, ranges, data, _, _ = expected_ranges(runs["text"])
    e = fa.Engine("FFM", N_FEATS, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, field_start=ranges, hash_ids=True)
    total, seen, pos, ramp = 0.0, 0, 0, fa.default_batch_ramp(1e-4)
    while pos < data.n_rows:  # (train_online's schedule, keeping the losses)
        n = min(BATCH, max(1, seen // ramp), data.n_rows - pos)
        total += e.train_batch(data.rows(pos, pos + n))[1]
        seen += n
        pos += n
    e.close()
    want = "train loss: %.4f" % (total / data.n_rows)
    for name in ("a", "b"):
        got = re.findall(r"train loss: [0-9.]+", runs[name])
        assert got == [want], (name, got, want)
    # ... which are not the uniform ones: the small fields gave their ids to the large ones
    width = np.diff(ranges)
    assert width[0] > N_FEATS // F > width[2] and int(width.min()) >= min(4096, N_FEATS // (2 * F))


@pytest.mark.parametrize("name", sorted(UNIFORM_RUNS))
def test_old_spellings_print_what_they_printed(tmp_path, name):
    """Byte for byte (times aside) the output recorded from the binary of the commit before this feature."""
    _bundled(tmp_path)
    want = open(os.path.join(GOLDEN, "field_sketch_cli", name + ".txt")).read()
    got = run_cli(tmp_path, ["--train_data", "libffm_data.txt"] + UNIFORM_RUNS[name])
    assert without_times(got) == want
    assert "train loss" in want and "field ranges" not in want


def test_ranges_out_with_uniform_and_ranges_in_for_scoring(tmp_path):
    path, _ = _bundled(tmp_path)
    uni = run_cli(tmp_path, BASE + ["--train_data", path, "--field_ranges", "uniform", "--field_ranges_out", "u.txt",
                                    "--checkpoint_path", "cu"])
    per = N_FEATS // F
    assert (tmp_path / "u.txt").read_text() == "".join("%d\n" % v for v in [f * per for f in range(F)] + [N_FEATS])
    # the uniform ranges read back from their file: the same run, the same checkpoint
    again = run_cli(tmp_path, BASE + ["--train_data", path, "--field_ranges", "@u.txt", "--checkpoint_path", "cu2"])
    assert without_times(again).replace("saving to cu2,", "saving to cu,") == without_times(uni)  # (the name is printed)
    assert (tmp_path / "cu").read_bytes() == (tmp_path / "cu2").read_bytes()
    # a saved model scored with its ranges from the file, on a training and on a serving engine: the same scores
    score = ["--model_type", "FFM", "--batch_size", str(BATCH), "--hash_feats", "true", "--resume_from", "cu", "--n_epochs", "0",
             "--predict_data", path]
    run_cli(tmp_path, score + ["--field_ranges", "uniform", "--predict_out", "p_uniform.txt"])
    run_cli(tmp_path, score + ["--field_ranges", "@u.txt", "--predict_out", "p_file.txt"])
    run_cli(tmp_path, score + ["--field_ranges", "@u.txt", "--predict_out", "p_serve.txt", "--serve_weights", "f32"])
    want = (tmp_path / "p_uniform.txt").read_bytes()
    assert len(want) > 0 and (tmp_path / "p_file.txt").read_bytes() == want and (tmp_path / "p_serve.txt").read_bytes() == want


def refused(tmp_path, args):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and out.stdout == "", out.stdout + out.stderr
    return out.stderr


def test_refusals_come_before_a_device_is_opened(tmp_path):
    path, _ = _bundled(tmp_path)
    counted = ["--model_type", "FFM", "--field_ranges", "counted"]
    assert "it needs --train_data" in refused(tmp_path, counted + ["--n_epochs", "0", "--predict_data", path, "--predict_out", "p.txt"])
    msg = refused(tmp_path, counted + ["--train_data", path, "--resume_from", "ck"])
    assert "is not allowed with --resume_from" in msg and "--field_ranges @FILE" in msg
    assert "--n_gpus > 1 is not allowed with it" in refused(tmp_path, counted + ["--train_data", path, "--n_gpus", "2"])
    libsvm = tmp_path / "d.svm"
    libsvm.write_text("1 1:1 7:0.5\n0 2:1 8:1\n")
    assert "only FFM rows have (got --model_type FM)" in refused(
        tmp_path, ["--model_type", "FM", "--field_ranges", "counted", "--train_data", str(libsvm)])
    # several GPUs keep demanding uniform ranges, in the words they always used
    (tmp_path / "r.txt").write_text("".join("%d\n" % v for v in [f * 1250 for f in range(8)] + [10000]))
    assert "--n_gpus > 1 needs --field_ranges uniform (per-field id ranges)" in refused(
        tmp_path, ["--model_type", "FFM", "--train_data", path, "--field_ranges", "@r.txt", "--n_gpus", "2", "--hash_feats", "true"])
    # a ranges file that does not fit the model: file:line
    (tmp_path / "bad.txt").write_text("0\n10\n5\n")
    msg = refused(tmp_path, ["--model_type", "FFM", "--train_data", path, "--field_ranges", "@bad.txt", "--hash_feats", "true"])
    assert "bad.txt:3: the values must ascend: 5 after 10" in msg
