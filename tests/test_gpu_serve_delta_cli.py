"""The trainer CLI's --publish_path / --publish_weights / --apply_deltas on the bundled libffm file: a consumer
that only ever sees PREFIX.<epoch>.delta files scores, byte for byte, what a serving engine loaded from the
trainer's checkpoint scores -- for both formats, with and without --refresh_weights true.  (run_cli and the
bundled file are those of tests/test_gpu_scores_cli.py.)"""
import functools
import os
import pathlib
import re
import shutil
import subprocess

import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import BATCH, _bundled, run_cli, without_times

pytestmark = pytest.mark.gpu

BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH)]
PUBLISHED = re.compile(r"^epoch (\d+) published: (\d+) of (\d+) features moved, (\d+) bytes -> (\S+)\n", re.M)
APPLIED = re.compile(r"^applied (\d+) deltas: (\d+) features, (\d+) bytes\n", re.M)
CASES = [(fmt, refresh) for fmt in ("f32", "f16") for refresh in (False, True)]


def scoring_lines(stdout):
    """What a scoring run prints, without the lines that say where its model came from."""
    keep = [ln for ln in without_times(stdout).splitlines()
            if not ln.startswith(("applied ", "loading from ", "serving weights: "))]
    return "\n".join(keep)


@functools.lru_cache(maxsize=None)
def _runs(root, fmt, refresh):
    """One 3-epoch run that publishes P.* and writes ck3; one cut after 2 epochs (Q.*, ck2) and resumed for 1."""
    os.makedirs(root)
    path, _ = _bundled(pathlib.Path(root))
    flags = ["--train_data", path, "--publish_weights", fmt] + (["--refresh_weights", "true"] if refresh else [])
    whole = run_cli(root, BASE + flags + ["--n_epochs", "3", "--publish_path", "P", "--checkpoint_path", "ck3"])
    cut = run_cli(root, BASE + flags + ["--n_epochs", "2", "--publish_path", "Q", "--checkpoint_path", "ck2"])
    resumed = run_cli(root, BASE + flags + ["--n_epochs", "1", "--publish_path", "Q", "--resume_from", "ck2"])
    return path, whole, cut, resumed


@pytest.fixture
def runs(request, tmp_path_factory):
    fmt, refresh = request.param
    root = str(tmp_path_factory.getbasetemp() / ("serve_delta_cli_%s_%d" % (fmt, refresh)))
    return (root, fmt) + _runs(root, fmt, refresh)


def score(root, fmt, source, out_name, path):
    return run_cli(root, BASE + ["--serve_weights", fmt, "--n_epochs", "0", "--predict_data", path, "--predict_out", out_name,
                                 "--eval_data", path, "--metrics", "auc", "--auc_key_field", "0"] + source)


@pytest.mark.parametrize("runs", CASES, indirect=True, ids=lambda c: "%s-refresh%d" % c)
def test_publish_against_checkpoint(runs):
    root, fmt, path, whole, cut, resumed = runs
    lines = PUBLISHED.findall(whole)
    assert [(ln[0], ln[4]) for ln in lines] == [("1", "P.1.delta"), ("2", "P.2.delta"), ("3", "P.3.delta")], whole
    for ep, moved, total, nbytes, name in lines:
        assert 0 < int(moved) <= int(total) == 10000 and int(nbytes) == os.path.getsize(os.path.join(root, name))
    # the publication sits after the epoch's training (and refresh) and before anything else of the epoch
    order = [ln.split()[2] for ln in whole.splitlines() if ln.startswith("epoch 1 ")]
    assert order.index("published:") == (2 if "weights:" in order else 1) and order[0] == "train", order
    by_deltas = score(root, fmt, ["--apply_deltas", "P"], "deltas.txt", path)
    by_ck = score(root, fmt, ["--resume_from", "ck3"], "ck.txt", path)
    got = APPLIED.findall(by_deltas)
    assert len(got) == 1 and got[0][0] == "3" and int(got[0][1]) == sum(int(ln[1]) for ln in lines), by_deltas
    assert int(got[0][2]) == sum(int(ln[3]) for ln in lines)
    a, b = open(os.path.join(root, "deltas.txt"), "rb").read(), open(os.path.join(root, "ck.txt"), "rb").read()
    assert len(b) > 0 and a == b, "the consumer of deltas scores differently from the checkpoint's serving engine"
    assert "auc" in scoring_lines(by_ck).lower() and scoring_lines(by_deltas) == scoring_lines(by_ck), by_deltas + by_ck


@pytest.mark.parametrize("runs", CASES, indirect=True, ids=lambda c: "%s-refresh%d" % c)
def test_prefix_colon_n_and_resume(runs):
    root, fmt, path, whole, cut, resumed = runs
    # P:2 is the model after two epochs: the checkpoint of the run that stopped there
    two = score(root, fmt, ["--apply_deltas", "P:2"], "two.txt", path)
    ck2 = score(root, fmt, ["--resume_from", "ck2"], "ck2.txt", path)
    assert APPLIED.findall(two)[0][0] == "2"
    assert open(os.path.join(root, "two.txt"), "rb").read() == open(os.path.join(root, "ck2.txt"), "rb").read()
    assert scoring_lines(two) == scoring_lines(ck2)
    # a run cut after 2 epochs and resumed for 1 publishes the one-piece run's third delta, byte for byte
    assert [ln[0] for ln in PUBLISHED.findall(cut)] == ["1", "2"] and [ln[0] for ln in PUBLISHED.findall(resumed)] == ["3"]
    for n in (1, 2, 3):
        p, q = (open(os.path.join(root, "%s.%d.delta" % (x, n)), "rb").read() for x in "PQ")
        assert len(p) > 96 and p == q, "delta %d of the resumed run differs from the one-piece run's" % n


@pytest.mark.parametrize("runs", CASES[:1] + CASES[3:], indirect=True, ids=lambda c: "%s-refresh%d" % c)
def test_missing_delta(runs):
    root, fmt, path, whole, cut, resumed = runs
    for n in (1, 3):
        shutil.copy(os.path.join(root, "P.%d.delta" % n), os.path.join(root, "M.%d.delta" % n))
    stops = score(root, fmt, ["--apply_deltas", "M"], "m.txt", path)
    assert APPLIED.findall(stops)[0][0] == "1", stops
    main_bin, _ = fa.build_host()
    for source, name in ((["--apply_deltas", "M:3"], "M.2.delta"), (["--apply_deltas", "N"], "N.1.delta")):
        out = subprocess.run([main_bin] + BASE + ["--serve_weights", fmt, "--n_epochs", "0", "--predict_data", path,
                                                  "--predict_out", "never.txt"] + source,
                             cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode != 0 and name in out.stderr, out.stdout + out.stderr
    # a resumed publisher without its earlier deltas stops before any training
    out = subprocess.run([main_bin] + BASE + ["--train_data", path, "--n_epochs", "1", "--publish_path", "M", "--publish_weights", fmt,
                                              "--resume_from", "ck2"] + (["--refresh_weights", "true"] if "weights:" in whole else []),
                         cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "M.2.delta" in out.stderr and "train time" not in out.stdout, out.stdout + out.stderr
