"""The trainer CLI's --device_rows true on the bundled libffm data (10 000 rows): online training, evaluation and
--predict_data read their files as raw bytes, the device parses them and cuts the blocks in HBM -- and every line
printed, every score, model file and checkpoint is what it is without the flag, byte for byte: at the default slot
size (one chunk) and with slots of 64 KB (blocks that straddle chunks, carried tails), with the whole recipe of device
pre-passes in front, from a serving engine, with a value the device leaves to the host, a line longer than a slot and
a malformed line.  (_bundled / run_cli are those of tests/test_gpu_scores_cli.py.)"""
import os
import re
import subprocess

import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from test_gpu_scores_cli import _bundled, run_cli

pytestmark = pytest.mark.gpu

BATCH, N_ROWS = 256, 10000
BASE = ["--model_type", "FFM", "--online", "true", "--batch_size", str(BATCH)]
ROWS_LINE = re.compile(r"^device rows: (train|eval|predict) (\d+) chunks, (\d+) bytes, (\d+) parsed by the host(?: \(first at byte (\d+)\))?, (\d+) blocks\n",
                       re.M)
VARIANTS = (("plain", [], None), ("dev", ["--device_rows", "true"], None), ("dev64k", ["--device_rows", "true"], {"FFM_TEXT_SLOT_BYTES": "65536"}))


def _lines(stdout):
    """What the run printed, times masked; the lines of the device paths are extra."""
    lines = [ln for ln in stdout.splitlines() if not ln.startswith(("device rows:", "device parse:"))]
    return [re.sub(r"in [0-9.]+ s", "in T s", re.sub(r"time: [0-9.]+s", "time: Ts", ln)) for ln in lines]


def _ramp_blocks(epochs, seen=0):
    """Blocks per epoch of the online trainer's ramp over the bundled rows (8 entries a row: the entry budget never
    ends a block)."""
    ramp = fa.default_batch_ramp(1e-4)
    out = []
    for _ in range(epochs):
        pos = blocks = 0
        while pos < N_ROWS:
            n = min(BATCH, max(1, seen // ramp)) if ramp > 0 else BATCH
            n = min(n, N_ROWS - pos)
            pos += n
            seen += n
            blocks += 1
        out.append(blocks)
    return out


def _run_variants(tmp_path, args, extra_dev=(), files=(), variants=VARIANTS):
    """The same command without the flag and with it (each in a directory of its own, so that the file names printed
    are the same): {variant: stdout}; the lines and the files named must be equal."""
    outs = {}
    for name, flags, env in variants:
        cwd = tmp_path / name
        cwd.mkdir(exist_ok=True)
        outs[name] = run_cli(cwd, args + (flags + list(extra_dev) if flags else []), env=env)
    assert not ROWS_LINE.findall(outs["plain"])
    for name, _, _ in variants[1:]:
        assert _lines(outs[name]) == _lines(outs["plain"]), name
        for f in files:
            a, b = (tmp_path / "plain" / f).read_bytes(), (tmp_path / name / f).read_bytes()
            assert len(a) > 0 and a == b, (name, f)
    return outs


def _check_rows_lines(stdout, n_bytes, want, many):
    """want: [(pass, blocks)] in order; H == 0; one chunk at the default slot size, 12 or more at 64 KB."""
    got = ROWS_LINE.findall(stdout)
    assert [(p, int(k)) for p, _, _, _, _, k in got] == want, (got, want)
    for _, chunks, b, h, first, _ in got:
        assert int(b) == n_bytes and h == "0" and first == ""
        assert int(chunks) >= 12 if many else int(chunks) == 1


def test_online_training_with_evaluation_metrics_model_and_checkpoint(tmp_path):
    path, text = _bundled(tmp_path)
    args = BASE + ["--train_data", path, "--eval_data", path, "--n_epochs", "2", "--metrics", "auc", "--auc_key_field", "0",
                   "--model_path", "model.txt", "--checkpoint_path", "ck"]
    outs = _run_variants(tmp_path, args, files=("model.txt", "model.txt.nz", "ck"))
    plain = outs["plain"]
    assert "epoch 2 train auc:" in plain and "epoch 2 eval gauc:" in plain and "epoch 2 eval time" in plain
    per_epoch = _ramp_blocks(2)
    eval_blocks = -(-N_ROWS // BATCH)
    want = [("train", per_epoch[0]), ("eval", eval_blocks), ("train", per_epoch[1]), ("eval", eval_blocks)]
    assert per_epoch[0] > per_epoch[1] == eval_blocks  # (the ramp's small blocks lie in the first epoch)
    _check_rows_lines(outs["dev"], len(text), want, many=False)
    _check_rows_lines(outs["dev64k"], len(text), want, many=True)


def test_the_whole_recipe_on_the_device(tmp_path):
    path, text = _bundled(tmp_path)
    args = BASE + ["--train_data", path, "--eval_data", path, "--n_epochs", "1", "--metrics", "auc", "--hash_feats", "true",
                   "--bucket_fields", "7", "--min_count", "3", "--field_ranges", "counted", "--normalize_rows", "true",
                   "--model_path", "model.txt", "--checkpoint_path", "ck", "--predict_data", path, "--predict_out", "p.txt"]
    outs = _run_variants(tmp_path, args, extra_dev=["--device_parse", "true"], files=("model.txt", "model.txt.nz", "ck", "p.txt"))
    assert any(ln.startswith("normalized rows:") for ln in outs["plain"].splitlines())
    for name in ("dev", "dev64k"):
        assert sum(ln.startswith("device parse:") for ln in outs[name].splitlines()) == 3
    want = [("train", _ramp_blocks(1)[0]), ("eval", -(-N_ROWS // BATCH)), ("predict", -(-N_ROWS // BATCH))]
    _check_rows_lines(outs["dev"], len(text), want, many=False)
    _check_rows_lines(outs["dev64k"], len(text), want, many=True)


@pytest.mark.parametrize("serve", ["none", "f16"])
def test_scoring_a_saved_model(tmp_path, serve):
    path, text = _bundled(tmp_path)
    run_cli(tmp_path, BASE + ["--train_data", path, "--n_epochs", "1", "--checkpoint_path", "ck"])
    ck = str(tmp_path / "ck")
    args = BASE + ["--resume_from", ck, "--n_epochs", "0", "--predict_data", path, "--predict_out", "p.txt", "--serve_weights", serve]
    outs = _run_variants(tmp_path, args, files=("p.txt",))
    assert any(ln.startswith("scored %d rows" % N_ROWS) for ln in outs["plain"].splitlines())
    assert (tmp_path / "plain" / "p.txt").read_bytes().count(b"\n") == N_ROWS
    want = [("predict", -(-N_ROWS // BATCH))]
    _check_rows_lines(outs["dev"], len(text), want, many=False)
    _check_rows_lines(outs["dev64k"], len(text), want, many=True)


def test_a_value_outside_the_grammar_and_a_long_line_go_to_the_host(tmp_path):
    """The file of tests/test_gpu_text_parse_cli.py: one value spelled 1e-3, one line longer than a 64 KB slot."""
    path, text = _bundled(tmp_path)
    lines = text.splitlines()
    assert lines[4321].split()[-1].startswith("7:")
    lines[4321] = " ".join(lines[4321].split()[:-1] + ["7:9803:1e-3"])
    lines[7000] = lines[7000] + " " * 70000  # longer than a 64 KB slot: the host parser's
    off = sum(len(ln) + 1 for ln in lines[:4321])
    p = tmp_path / "exp.txt"
    p.write_text("\n".join(lines) + "\n")
    n_bytes = p.stat().st_size
    args = BASE + ["--train_data", str(p), "--eval_data", str(p), "--n_epochs", "1", "--metrics", "auc", "--model_path", "model.txt",
                   "--checkpoint_path", "ck", "--predict_data", str(p), "--predict_out", "p.txt"]
    outs = _run_variants(tmp_path, args, files=("model.txt", "model.txt.nz", "ck", "p.txt"))
    for name, hosted in (("dev", "1"), ("dev64k", "2")):
        got = ROWS_LINE.findall(outs[name])
        assert [g[0] for g in got] == ["train", "eval", "predict"], got
        assert all(int(b) == n_bytes and h == hosted and int(first) == off for _, _, b, h, first, _ in got), (name, got)
    assert all(c == "1" for _, c, _, _, _, _ in ROWS_LINE.findall(outs["dev"]))


def test_a_malformed_line_ends_the_run_the_same_way(tmp_path):
    path, text = _bundled(tmp_path)
    lines = text.splitlines()
    lines[2500] = "1 0:17:1 3:4: 5:6:1"
    p = tmp_path / "bad.txt"
    p.write_text("\n".join(lines) + "\n")
    main_bin, _ = fa.build_host()
    outs = []
    for extra, env in ([], None), (["--device_rows", "true"], None), (["--device_rows", "true"], {"FFM_TEXT_SLOT_BYTES": "65536"}):
        out = subprocess.run([main_bin] + BASE + ["--train_data", str(p), "--n_epochs", "1"] + extra, cwd=tmp_path, capture_output=True,
                             text=True, timeout=600, env=dict(os.environ, **(env or {})))
        outs.append(out)
        assert out.returncode != 0
        assert [ln for ln in out.stdout.splitlines() if ln.startswith("wrong input:")] == ["wrong input: " + lines[2500]], out.stdout
    assert outs[0].returncode == outs[1].returncode == outs[2].returncode
    assert outs[0].stderr == outs[1].stderr == outs[2].stderr


def test_refused_combinations_name_both_flags(tmp_path):
    """Refused while the options are parsed (the stand-alone option program checks every one; here: the binary itself)."""
    path, _ = _bundled(tmp_path)
    main_bin, _ = fa.build_host()
    bad = subprocess.run([main_bin] + BASE[:2] + ["--train_data", path, "--online", "false", "--device_rows", "true"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--device_rows true" in bad.stderr and "--online false" in bad.stderr
    assert bad.stdout == ""  # (before anything is trained)
