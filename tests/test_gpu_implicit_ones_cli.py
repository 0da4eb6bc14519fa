"""The trainer CLI's --compact_rows: blocks whose values are all 1 go to the engine without their value array
(val == NULL, include/ffm_engine.h "Rows without values"), FFM blocks of one entry per field in field order
without their field array.  Every printed loss and AUC line, the model file, the checkpoint and the scores are
those of the same run with `false`, byte for byte -- online and offline, with and without --hash_feats, and
scoring from an f16 serving engine; the run reports how many blocks went without which array.
(run_cli / without_times are those of tests/test_gpu_scores_cli.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

pytestmark = pytest.mark.gpu

F, PER, K, ROWS, BATCH = 8, 300, 4, 2000, 256
NF = F * PER
LINE = re.compile(r"^compact rows: (\d+) of (\d+) blocks without values, (\d+) without fields\n", re.M)


def run_cli(tmp_path, args):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def without_times(stdout):
    return re.sub(r"time: [0-9.]+s", "time: Ts", stdout)


def _write(tmp_path, irregular):
    """s.ffm in directories a and b: regular rows of ones; irregular: a few rows carry a value other than 1, a
    few lack a field."""
    blk = synth.Generator(F, NF, "zipf", seed=8, ones="array").block(ROWS)
    lines = synth.to_libffm_text(blk).split("\n")[:-1]
    assert len(lines) == ROWS and all(len(ln.split()) == F + 1 and ln.count(":1 ") + ln.endswith(":1") == F for ln in lines)
    if irregular:
        for r in (5, 6, 1200):  # a value of 0.5 in the first and in a later block
            t = lines[r].split()
            t[3] = t[3][:-1] + "0.5"
            lines[r] = " ".join(t)
        for r in (300, 1700, 1701):  # a row without its field 2
            t = lines[r].split()
            del t[3]
            lines[r] = " ".join(t)
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
        (tmp_path / name / "s.ffm").write_text("\n".join(lines) + "\n")


def _base(online, hashed):
    return ["--train_data", "s.ffm", "--model_type", "FFM", "--n_fields", str(F), "--n_feats", str(NF), "--n_factors", str(K),
            "--online", online, "--batch_size", str(BATCH), "--batch_ramp", "32", "--w_alpha", "0.05", "--w_l1", "0.01",
            "--w_l2", "0.1", "--field_ranges", "uniform", "--hash_feats", hashed, "--n_threads", "2"]


def _files(path):
    return {n: (path / n).read_bytes() for n in sorted(os.listdir(path)) if n != "s.ffm"}


def _pair(tmp_path, args):
    """The run with --compact_rows true in a, false in b: (V, B, F) of the line, after every output compared."""
    on = run_cli(tmp_path / "a", args + ["--compact_rows", "true"])
    off = run_cli(tmp_path / "b", args + ["--compact_rows", "false"])
    assert "compact rows" not in off, off
    m = LINE.findall(on)
    assert len(m) == 1, on
    assert without_times(LINE.sub("", on)) == without_times(off)
    assert re.findall(r"(?:train|eval) (?:loss|auc): \S+", on) == re.findall(r"(?:train|eval) (?:loss|auc): \S+", off)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert a == b and all(len(v) > 0 for v in a.values()), sorted(a)
    return tuple(int(x) for x in m[0]), on, a


TRAIN = ["--eval_data", "s.ffm", "--n_epochs", "2", "--metrics", "auc", "--predict_data", "s.ffm", "--model_path", "m.txt",
         "--checkpoint_path", "ck", "--predict_out", "p.txt", "--refresh_weights", "true"]


@pytest.mark.parametrize("hashed", ["false", "true"], ids=["ids", "hashed"])
@pytest.mark.parametrize("online", ["true", "false"], ids=["online", "offline"])
def test_regular_file_of_ones(tmp_path, online, hashed):
    _write(tmp_path, irregular=False)
    (v, b, f), on, files = _pair(tmp_path, _base(online, hashed) + TRAIN)
    assert sorted(files) == ["ck", "m.txt", "m.txt.nz", "p.txt"]
    assert b > 0 and v == b and f == b, (v, b, f)  # every block of such a file: training, evaluation and scoring
    losses = [float(x) for x in re.findall(r"train loss: ([0-9.]+)", on)]
    assert len(losses) == 2 and losses[1] < losses[0], "the rows train"
    assert len(re.findall(r"auc: ", on)) == 4


@pytest.mark.parametrize("online", ["true", "false"], ids=["online", "offline"])
def test_file_with_a_few_other_rows(tmp_path, online):
    _write(tmp_path, irregular=True)
    (v, b, f), on, files = _pair(tmp_path, _base(online, "true") + TRAIN)
    assert sorted(files) == ["ck", "m.txt", "m.txt.nz", "p.txt"]
    assert 0 < v < b and 0 < f < b, (v, b, f)


def test_scoring_from_an_f16_serving_engine(tmp_path):
    _write(tmp_path, irregular=False)
    base = _base("true", "true")
    for d in ("a", "b"):
        run_cli(tmp_path / d, base + ["--n_epochs", "1", "--checkpoint_path", "ck", "--refresh_weights", "true", "--learn", "true"])
    serve = [x for x in base if x != "--train_data"]
    serve.remove("s.ffm")
    serve += ["--resume_from", "ck", "--n_epochs", "0", "--serve_weights", "f16", "--learn", "true", "--metrics", "auc",
              "--predict_data", "s.ffm", "--predict_out", "p.txt"]
    (v, b, f), on, files = _pair(tmp_path, serve)
    assert "serving weights: f16" in on
    assert b > 0 and v == b and f == b, (v, b, f)
    scores = np.array([np.float32(s) for s in files["p.txt"].decode().split("\n")[:-1]], np.float32)
    assert scores.size == ROWS and np.isfinite(scores).all() and scores.std() > 0
