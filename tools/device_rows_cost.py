#!/usr/bin/env python3
"""What --device_rows true costs and buys (include/ffm_engine.h "Resident rows"; the numbers of profiles/device_rows.md).

Four steps, a child process each under its own `timeout`, one after another; the first that fails ends the run
(nothing more is started on the GPU).  Every step runs the trainer CLI over a file of the 39-field Zipf libffm text of
profiles/device_parse.md (c) (20 000 generated rows written --rows / 20 000 times), with and without `--device_rows
true`, at --n_threads 8 and 16, five runs each after one dropped round that warms the page cache, the four
configurations alternating; rows/s from the time the CLI prints for the pass:
  eval      the evaluation pass (`epoch 1 eval time`) of an FFM model of C3's shape (39 fields, k = 4, 1 M hashed
            features, blocks of 8192 rows) that trained one epoch on the first 20 000 rows
  predict   `--predict_data` (`scored N rows time`) from an f16 serving engine of that model (--resume_from ck
            --n_epochs 0 --serve_weights f16)
  train_c2  one online training epoch (`epoch 1 train time`) at C2's shape: 8 fields, k = 16, 10 000 features, blocks of
            4096 rows, over an 8-field file of as many rows
  train_headline  one online training epoch at the headline shape: 39 fields, k = 16, 33 M features, blocks of 8192 rows
The flag-off runs are the parent commit's code path.  It needs a GPU and fails without one.  bench.py stays the
project's yardstick; this tool only compares paths."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("eval", "predict", "train_c2", "train_headline")
TAG = "DEVICE_ROWS_COST "
UNIT = 20000
C3 = ["--model_type", "FFM", "--n_fields", "39", "--n_feats", "1000000", "--n_factors", "4", "--hash_feats", "true", "--batch_size", "8192"]
C2 = ["--model_type", "FFM", "--n_fields", "8", "--n_feats", "10000", "--n_factors", "16", "--batch_size", "4096"]
HEADLINE = ["--model_type", "FFM", "--n_fields", "39", "--n_feats", "33000000", "--n_factors", "16", "--batch_size", "8192"]
TIMES = {"eval": re.compile(r"^epoch 1 eval time: ([0-9.]+)s", re.M), "predict": re.compile(r"^scored \d+ rows time: ([0-9.]+)s", re.M),
         "train": re.compile(r"^epoch 1 train time: ([0-9.]+)s", re.M)}
ROWS_LINE = re.compile(r"^device rows: (\w+) (\d+) chunks, (\d+) bytes, (\d+) parsed by the host.*, (\d+) blocks$", re.M)


def write_files(tmp, rows, n_fields, feats):
    """(path of the big file, path of its first 20 000 rows, rows, bytes)"""
    from ftrl_ffm_amd import synth
    unit = synth.to_libffm_text(synth.Generator(n_fields, feats, "zipf", seed=3).block(UNIT)).encode()
    reps = max(1, rows // UNIT)
    big, small = os.path.join(tmp, "big.ffm"), os.path.join(tmp, "small.ffm")
    with open(big, "wb") as f:
        for _ in range(reps):
            f.write(unit)
    with open(small, "wb") as f:
        f.write(unit)
    return big, small, UNIT * reps, len(unit) * reps


def run_cli(cmd, tmp):
    t0 = time.perf_counter()
    out = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if out.returncode != 0:
        raise SystemExit("device_rows_cost: the CLI ended with status %d: %s" % (out.returncode, (out.stdout + out.stderr)[-1500:]))
    return out.stdout, wall


def compare(step, base, which, rows, n_bytes, tmp, reps, want_pass):
    """The four configurations alternating, reps + 1 rounds (the first is dropped): rows/s per run."""
    res, chunks = {}, {}
    for rep in range(reps + 1):
        for threads in (8, 16):
            for flag in (False, True):
                stdout, wall = run_cli(base + ["--n_threads", str(threads)] + (["--device_rows", "true"] if flag else []), tmp)
                got = TIMES[which].findall(stdout)
                assert len(got) == 1, stdout
                lines = [ln for ln in ROWS_LINE.findall(stdout) if ln[0] == want_pass]
                assert len(lines) == (1 if flag else 0), stdout
                key = "%d threads, %s" % (threads, "device rows" if flag else "host parser")
                if flag:
                    assert int(lines[0][2]) == n_bytes, stdout
                    chunks[key] = dict(chunks=int(lines[0][1]), by_host=int(lines[0][3]), blocks=int(lines[0][4]))
                if rep:
                    res.setdefault(key, []).append(dict(seconds=float(got[0]), rows_per_s=rows / float(got[0]), wall=wall))
    print(TAG + json.dumps({"step": step, "rows": rows, "bytes": n_bytes, "runs": res, "device_rows_lines": chunks}))


def step_eval(args, tmp, main_bin):
    big, small, rows, n_bytes = write_files(tmp, args.rows, 39, 33_000_000)
    compare("eval", [main_bin] + C3 + ["--train_data", small, "--eval_data", big, "--n_epochs", "1"], "eval", rows, n_bytes, tmp, args.reps, "eval")


def step_predict(args, tmp, main_bin):
    big, small, rows, n_bytes = write_files(tmp, args.rows, 39, 33_000_000)
    run_cli([main_bin] + C3 + ["--train_data", small, "--n_epochs", "1", "--checkpoint_path", "ck", "--refresh_weights", "true"], tmp)
    base = [main_bin] + C3 + ["--resume_from", "ck", "--n_epochs", "0", "--serve_weights", "f16", "--predict_data", big, "--predict_out", "p.txt"]
    compare("predict", base, "predict", rows, n_bytes, tmp, args.reps, "predict")


def step_train_c2(args, tmp, main_bin):
    big, _, rows, n_bytes = write_files(tmp, args.rows, 8, 10_000)
    compare("train_c2", [main_bin] + C2 + ["--train_data", big, "--n_epochs", "1"], "train", rows, n_bytes, tmp, args.reps, "train")


def step_train_headline(args, tmp, main_bin):
    big, _, rows, n_bytes = write_files(tmp, args.rows, 39, 33_000_000)
    compare("train_headline", [main_bin] + HEADLINE + ["--train_data", big, "--n_epochs", "1"], "train", rows, n_bytes, tmp, args.reps, "train")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--only", help="comma-separated steps to run (default: all)")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=900)
    args = ap.parse_args()
    if args.step:
        import ftrl_ffm_amd as fa
        main_bin, _ = fa.build_host()
        with tempfile.TemporaryDirectory() as tmp:
            return globals()["step_" + args.step](args, tmp, main_bin)
    for step in (args.only.split(",") if args.only else STEPS):
        rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--rows", str(args.rows), "--reps", str(args.reps)]).returncode
        if rc != 0:
            raise SystemExit("device_rows_cost: step %s ended with status %d; nothing more is started" % (step, rc))


if __name__ == "__main__":
    main()
