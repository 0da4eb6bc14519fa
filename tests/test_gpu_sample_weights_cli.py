"""The trainer CLI's sample weights: --pos_weight / --neg_weight (a weight per class) and --weight_data
(one decimal per row of --train_data); a row's weight is the float product of the two.

  (a) no flag at all and --pos_weight 1 --neg_weight 1 print the same loss lines and write byte-identical
      model files (weights of one are exact: the weighted kernels compute the unweighted bits, and
      sum(w * loss) / sum(w) is the same double division as sum(loss) / rows);
  (b) a weight file that spells the class weights label by label is --pos_weight 0.5 --neg_weight 2.5 --
      same loss lines, byte-identical model files, and not the unweighted run's -- online, offline over two
      epochs (the shuffled gather carries each row's weight by its row number) and on two shards;
  (c) a weight file with another line count than the data, an unparsable, a negative and a non-finite
      weight: refused before any training, the message names the file and the line.
All on generated 4-field rows (synth)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

pytestmark = pytest.mark.gpu

F, PER, ROWS = 4, 500, 6000


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_cli")
    blk = synth.Generator(F, F * PER, "zipf", seed=5).block(ROWS)
    path = d / "s.ffm"
    path.write_text(synth.to_libffm_text(blk))
    return d, str(path), blk.label.copy()


def run(d, data_path, name, extra, mode=(), env=None, ok=True):
    """One run of the CLI; returns (stdout without the times and the run's name, model file bytes, accumulator
    file bytes)."""
    main_bin, _ = fa.build_host()
    model = os.path.join(str(d), name + ".model")
    cmd = [main_bin, "--train_data", data_path, "--eval_data", data_path, "--model_type", "FFM", "--n_fields", str(F),
           "--n_feats", str(F * PER), "--n_factors", "4", "--batch_size", "512", "--w_alpha", "0.05", "--w_l1", "0.01",
           "--w_l2", "0.1", "--model_path", model] + list(mode) + list(extra)
    out = subprocess.run(cmd, cwd=str(d), capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    if not ok:
        return out
    assert out.returncode == 0, out.stdout + out.stderr
    text = re.sub(r"time: [0-9.]+s", "time: Ts", out.stdout).replace(name + ".model", "RUN.model")  # (the files are named in it)
    return text, open(model, "rb").read(), open(model + ".nz", "rb").read()


def loss_lines(text):
    return re.findall(r"^epoch \d+ (?:train|eval) time: Ts, (?:train|eval) loss: \S+$", text, re.M)


MODES = {
    "online": (["--online", "true", "--n_epochs", "2"], None),
    "offline": (["--online", "false", "--n_epochs", "2", "--n_threads", "2"], None),
    "two_shards": (["--online", "true", "--n_epochs", "2", "--n_gpus", "2", "--field_ranges", "uniform"], {"FTRL_SAME_DEVICE": "1"}),
}


@pytest.mark.parametrize("mode", ["online", "offline"])
def test_class_weights_of_one_change_nothing(data, mode):
    d, path, _ = data
    args, env = MODES[mode]
    plain = run(d, path, "plain_" + mode, [], args, env)
    ones = run(d, path, "ones_" + mode, ["--pos_weight", "1", "--neg_weight", "1"], args, env)
    assert len(loss_lines(plain[0])) == 4
    assert plain[0] == ones[0], "every printed line (times aside)"
    assert plain[1] == ones[1] and plain[2] == ones[2], "model and accumulator files"


@pytest.mark.parametrize("mode", list(MODES))
def test_weight_file_spelling_the_class_weights_is_the_class_weights(data, mode):
    d, path, label = data
    args, env = MODES[mode]
    wfile = os.path.join(str(d), "w_%s.txt" % mode)
    with open(wfile, "w") as f:
        f.write("".join("0.5\n" if y > 0 else "2.5\n" for y in label))
    by_class = run(d, path, "class_" + mode, ["--pos_weight", "0.5", "--neg_weight", "2.5"], args, env)
    by_file = run(d, path, "file_" + mode, ["--weight_data", wfile], args, env)
    plain = run(d, path, "plain2_" + mode, [], args, env)
    assert len(loss_lines(by_class[0])) == 4
    assert loss_lines(by_class[0]) == loss_lines(by_file[0])
    assert by_class[1] == by_file[1] and by_class[2] == by_file[2], "model and accumulator files"
    assert by_class[1] != plain[1] and by_class[2] != plain[2], "the weights must change the model"
    train = [ln for ln in loss_lines(by_class[0]) if "train loss" in ln]
    assert train != [ln for ln in loss_lines(plain[0]) if "train loss" in ln]
    # the weighted mean of a log loss below ln 2 on a model that learns: a number, not nan
    assert all(0.0 < float(ln.rsplit(" ", 1)[1]) < 0.6932 for ln in train), train


def test_all_zero_weights_print_nan(data):
    """sum(w) == 0 has no mean: the train loss line says nan, and the run still ends well."""
    d, path, _ = data
    args, env = MODES["online"]
    text, _, _ = run(d, path, "zero", ["--pos_weight", "0", "--neg_weight", "0"], args, env)
    train = [ln for ln in loss_lines(text) if "train loss" in ln]
    assert len(train) == 2 and all(ln.endswith("train loss: nan") for ln in train), train


@pytest.mark.parametrize("case", ["short", "long", "unparsable", "negative", "non_finite", "nan"])
def test_bad_weight_files_are_refused_before_any_training(data, case):
    d, path, label = data
    lines = ["1"] * ROWS
    where = 17
    if case == "short":
        lines, where = lines[:-3], ROWS - 2
    elif case == "long":
        lines, where = lines + ["1"], ROWS + 1
    else:
        lines[where - 1] = {"unparsable": "1.0x", "negative": "-0.5", "non_finite": "inf", "nan": "nan"}[case]
    wfile = os.path.join(str(d), "bad_%s.txt" % case)
    with open(wfile, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = run(d, path, "bad_" + case, ["--weight_data", wfile], MODES["online"][0], ok=False)
    assert out.returncode != 0, out.stdout
    assert "epoch" not in out.stdout, out.stdout
    assert "%s:%d:" % (wfile, where) in out.stderr, out.stderr
    assert not os.path.exists(os.path.join(str(d), "bad_" + case + ".model"))
