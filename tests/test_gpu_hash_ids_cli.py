"""The trainer CLI's --hash_feats (FFM_FLAG_HASH_IDS): a file with one global id space, fields interleaved,
trains as the same file pre-hashed by the binding's hash_ids does without the flag -- the model file, the
scores and the output byte for byte --, online and offline, with --field_ranges none and uniform, FFM on
libffm and FM on libsvm data; without the flag not a byte changes; --n_gpus 2 takes such a file and agrees
with one engine; a checkpoint written under the other setting is refused.
(run_cli / without_times / read_scores are those of tests/test_gpu_scores_cli.py.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

pytestmark = pytest.mark.gpu

F, PER, K, ROWS, BATCH = 8, 300, 4, 1500, 256
NF = F * PER
ID_SPACE = 10 ** 7  # what converters emit: one global space, usually a hash modulo 10^6 or 10^7


def run_cli(tmp_path, args, env=None, fails=False):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **(env or {})))
    if fails:
        assert out.returncode != 0, out.stdout + out.stderr
        return out.stdout + out.stderr
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def without_times(stdout):
    return re.sub(r"time: [0-9.]+s", "time: Ts", stdout)


def read_scores(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "", "the file ends with a line end"
    return np.array([np.float32(s) for s in lines[:-1]], np.float32)


def _raw_block(libsvm=False):
    """Rows whose ids come from one global space of 10^7, the same raw id under several fields now and then."""
    blk = synth.Generator(F, NF, "zipf", seed=8).block(ROWS)
    table = np.random.default_rng(3).integers(0, ID_SPACE, NF // 2)  # (half as many raw ids: fields share them)
    blk.feat = table[blk.feat % table.size].astype(np.int32)
    if libsvm:
        blk.field[:] = 0
    assert (blk.feat >= NF).mean() > 0.99, "without hashing almost every entry would be erased"
    return blk


def _write_pair(tmp_path, field_ranges, libsvm=False):
    """a/s.ffm: the raw file; b/s.ffm: the same rows with the ids the flagged engine gives them."""
    blk = _raw_block(libsvm)
    fs = (np.arange(F + 1) * PER).astype(np.int32) if field_ranges == "uniform" and not libsvm else None
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
    (tmp_path / "a" / "s.ffm").write_text(synth.to_libffm_text(blk, libsvm=libsvm))
    raw = blk.feat.copy()
    blk.feat = fa.hash_ids(None if libsvm else blk.field, raw, NF, field_start=fs, model="fm" if libsvm else "ffm", n_fields=F)
    assert blk.feat.min() >= 0 and blk.feat.max() < NF and not np.array_equal(blk.feat, raw)
    if fs is not None:
        assert (blk.feat // PER == blk.field).all(), "every hashed id lies in its field's range"
    (tmp_path / "b" / "s.ffm").write_text(synth.to_libffm_text(blk, libsvm=libsvm))


def _base(model="FFM", online="true", field_ranges="none"):
    return ["--train_data", "s.ffm", "--model_type", model, "--n_fields", str(F), "--n_feats", str(NF), "--n_factors", str(K),
            "--online", online, "--batch_size", str(BATCH), "--batch_ramp", "32", "--w_alpha", "0.05", "--w_l1", "0.01",
            "--w_l2", "0.1", "--field_ranges", field_ranges]


def _files(path):
    return {n: (path / n).read_bytes() for n in sorted(os.listdir(path)) if n != "s.ffm"}


def test_nothing_changes_without_the_flag(tmp_path):
    _write_pair(tmp_path, "none")
    args = _base() + ["--eval_data", "s.ffm", "--n_epochs", "2", "--metrics", "auc", "--predict_data", "s.ffm",
                      "--model_path", "m.txt", "--checkpoint_path", "ck", "--predict_out", "p.txt"]
    shutil.copy(tmp_path / "b" / "s.ffm", tmp_path / "a" / "s.ffm")  # (the hashed file twice: its ids are in range)
    plain = run_cli(tmp_path / "a", args)
    off = run_cli(tmp_path / "b", args + ["--hash_feats", "false"])
    assert without_times(off) == without_times(plain)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert a == b and sorted(a) == ["ck", "m.txt", "m.txt.nz", "p.txt"] and all(len(v) > 0 for v in a.values())


@pytest.mark.parametrize("field_ranges", ["none", "uniform"])
@pytest.mark.parametrize("online", ["true", "false"], ids=["online", "offline"])
def test_raw_file_with_the_flag_is_the_hashed_file_without(tmp_path, online, field_ranges):
    _write_pair(tmp_path, field_ranges)
    args = _base("FFM", online, field_ranges) + ["--eval_data", "s.ffm", "--n_epochs", "2", "--predict_data", "s.ffm",
                                                   "--model_path", "m.txt", "--predict_out", "p.txt", "--refresh_weights", "true"]
    a = run_cli(tmp_path / "a", args + ["--hash_feats", "true"])
    b = run_cli(tmp_path / "b", args)
    assert without_times(a) == without_times(b)
    fa_, fb = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert fa_ == fb and "m.txt" in fa_ and "p.txt" in fa_ and all(len(v) > 0 for v in fa_.values())
    losses = [float(x) for x in re.findall(r"train loss: ([0-9.]+)", a)]
    assert len(losses) == 2 and losses[1] < losses[0], "the hashed rows train"
    # ... and without the flag the raw file trains on next to nothing: another model
    raw = run_cli(tmp_path / "a", args[:-6] + ["--model_path", "raw.txt", "--predict_out", "raw_p.txt", "--refresh_weights", "true"])
    assert (tmp_path / "a" / "raw_p.txt").read_bytes() != fa_["p.txt"] and without_times(raw) != without_times(a)


def test_fm_on_libsvm_data(tmp_path):
    _write_pair(tmp_path, "none", libsvm=True)
    args = _base("FM") + ["--eval_data", "s.ffm", "--n_epochs", "1", "--predict_data", "s.ffm", "--model_path", "m.txt",
                          "--predict_out", "p.txt", "--learn", "true"]
    a = run_cli(tmp_path / "a", args + ["--hash_feats", "true"])
    b = run_cli(tmp_path / "b", args)
    assert without_times(a) == without_times(b)
    fa_, fb = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert fa_ == fb and "m.txt" in fa_ and len(fa_["p.txt"]) > 0


def test_two_shards_train_a_file_with_a_global_id_space(tmp_path):
    _write_pair(tmp_path, "uniform")
    args = _base("FFM", "true", "uniform") + ["--eval_data", "s.ffm", "--n_epochs", "2", "--predict_data", "s.ffm", "--hash_feats", "true"]
    one = run_cli(tmp_path / "a", args + ["--predict_out", "one.txt"])
    two = run_cli(tmp_path / "a", args + ["--predict_out", "two.txt", "--n_gpus", "2"], {"FTRL_SAME_DEVICE": "1"})
    assert "2 field-pair shards" in two and "field-pair shards" not in one
    # (the comparison of tests/test_host.py::test_cli_n_gpus_shards_match_one_engine)
    for key in ("train", "eval"):
        l1 = [float(x) for x in re.findall(key + r" loss: ([0-9.]+)", one)]
        l2 = [float(x) for x in re.findall(key + r" loss: ([0-9.]+)", two)]
        assert len(l1) == 2 and np.allclose(l2, l1, atol=2e-4), (key, l1, l2)
    p1, p2 = read_scores(tmp_path / "a" / "one.txt"), read_scores(tmp_path / "a" / "two.txt")
    assert p1.size == p2.size == ROWS and np.isfinite(p1).all()
    assert np.allclose(p2, p1, atol=2e-4), float(np.max(np.abs(p1 - p2)))


def test_resume_refuses_a_checkpoint_of_the_other_setting(tmp_path):
    _write_pair(tmp_path, "none")
    d = tmp_path / "a"
    base = _base() + ["--n_epochs", "1"]
    run_cli(d, base + ["--checkpoint_path", "ck_on", "--hash_feats", "true"])
    run_cli(d, base + ["--checkpoint_path", "ck_off"])
    text = run_cli(d, base + ["--resume_from", "ck_on"], fails=True)
    assert "was saved with --hash_feats, this model is the other variant" in text, text
    text = run_cli(d, base + ["--resume_from", "ck_off", "--hash_feats", "true"], fails=True)
    assert "was saved without --hash_feats, this model is the other variant" in text, text
    ok = run_cli(d, base + ["--resume_from", "ck_on", "--hash_feats", "true"])  # (the same setting resumes)
    assert "loading from ck_on" in ok
