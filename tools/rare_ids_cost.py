#!/usr/bin/env python3
"""What rare ids cost and what they buy (include/ffm_engine.h "Rare ids"; the numbers of profiles/rare_ids.md).

Three steps, a child process each under its own `timeout`, one after another; the first that fails ends the run
(nothing more is started on the GPU):
  prepass   the trainer CLI's counting pre-pass (`--min_count 10 --n_epochs 0`) next to its `--field_ranges
            counted --n_epochs 0` pass on the same generated file (39 fields, Zipf ids): rows/s from the `in S s`
            of their summary lines, the two alternating
  train     rows/s from page-locked host memory at the headline shape (bench.py's: FFM 39 x 16, 33 M features,
            8192-row Zipf blocks, staged two ahead, zero_copy) on ONE hashed engine, with a keep-map of 2^27
            slots and without one, in alternating windows; the no-map run's own spread over its windows
  quality   eval logloss and AUC of one `--learn true` epoch over the bundled data (first 8000 rows train, last
            2000 evaluate) at --min_count 0, 2, 5 and 10.  Recorded, not judged: a property of the data
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares paths."""
import argparse
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIELDS, N_FACTORS, FEATS, ROWS = 39, 16, 33_000_000, 8192
STEPS = ("prepass", "train", "quality")


def cli(args, cwd):
    import ftrl_ffm_amd as fa
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=cwd, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit("rare_ids_cost: the CLI ended with status %d: %s" % (out.returncode, out.stderr[-1000:]))
    return out.stdout


def step_prepass(args):
    from ftrl_ffm_amd import synth
    nf = 975000
    with tempfile.TemporaryDirectory() as d:
        text = synth.to_libffm_text(synth.Generator(N_FIELDS, nf, "zipf", seed=42, ones="array").block(args.file_rows))
        path = os.path.join(d, "zipf.ffm")
        with open(path, "w") as f:
            for _ in range(args.file_copies):
                f.write(text)
        rows = args.file_rows * args.file_copies
        base = ["--model_type", "FFM", "--train_data", path, "--n_epochs", "0", "--hash_feats", "true", "--n_fields", str(N_FIELDS),
                "--n_feats", str(nf), "--n_threads", "8"]
        runs = {"min_count": base + ["--field_ranges", "uniform", "--min_count", "10"], "counted": base + ["--field_ranges", "counted"]}
        secs = {name: [] for name in runs}
        lines = {}
        cli(runs["counted"], d)  # (the page cache warm)
        for _ in range(args.repeats):
            for name, a in runs.items():
                out = cli(a, d)
                line = [ln for ln in out.splitlines() if ln.startswith("rare ids: counted" if name == "min_count" else "field ranges: counted")][-1]
                lines[name] = line
                secs[name].append(float(re.search(r" in ([0-9.]+) s;", line).group(1)))
        res = dict(rows=rows, bytes=os.path.getsize(path), seconds=secs,
                   rows_per_s={name: [round(rows / s) for s in v] for name, v in secs.items()}, last_line=lines)
    print("RARE_IDS_COST " + json.dumps(dict(step="prepass", **res)), flush=True)


def step_train(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rare_ids_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks, keep_alive = [], []
    ct = fa.IdCounter(N_FIELDS, args.bits, args.min_count)
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        ct.add(b.field, b.feat)
        for name in ("row_ptr", "field", "feat", "val", "label"):
            t = torch.from_numpy(getattr(b, name)).pin_memory()
            keep_alive.append(t)
            setattr(b, name, t.numpy())
        blocks.append(b)
    words, kept, folded = ct.keep(args.min_count)
    n_valid = ct.read()[1]
    ct.close()
    # (the counter is gone before the model takes the HBM it needs; raw ids of any size hash into the model's ranges,
    # so a model that had to be made smaller, as bench.py makes it, trains the same blocks)
    eng, model_feats = None, nf
    while eng is None:
        fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (model_feats // N_FIELDS)).astype(np.int32)
        try:
            eng = fa.Engine("FFM", model_feats, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                            max_row_nnz=N_FIELDS, field_start=fs, hash_ids=True)
        except fa.EngineError as err:
            if err.code != fa.engine.E_NOMEM or model_feats < 10 * N_FIELDS:
                raise
            model_feats = int(model_feats * 0.9)
            model_feats -= model_feats % N_FIELDS
    eng.fill_state(seed=7, n_lo=0.05, n_hi=1.0, z_stddev=0.3)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")

    def run(count):
        staged = 0
        for i in range(count):
            while staged < min(i + 3, count):
                eng.stage_batch(blocks[staged % len(blocks)], True)
                staged += 1
            eng.train_staged(None, loss.data_ptr())
        eng.sync()

    rates = {"no_map": [], "map": []}
    for which in ("no_map", "map"):  # warm-up of both paths (the folding upload kernel's code object too)
        eng.set_rare_fold(args.bits, words) if which == "map" else eng.set_rare_fold(None)
        run(args.warmup)
    for _ in range(args.repeats):  # alternating windows
        for which in ("no_map", "map"):
            eng.set_rare_fold(args.bits, words) if which == "map" else eng.set_rare_fold(None)
            t0 = time.perf_counter()
            run(args.steps)
            rates[which].append(ROWS * args.steps / (time.perf_counter() - t0))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    res = dict(n_feats=model_feats, bits=args.bits, min_count=args.min_count, kept_slots=kept, folded_share=round(folded / max(1, n_valid), 4),
               steps_per_window=args.steps, rows_per_s={k: [round(x) for x in v] for k, v in rates.items()},
               median={k: round(x) for k, x in med.items()},
               no_map_spread=round((max(rates["no_map"]) - min(rates["no_map"])) / med["no_map"], 4),
               map_below_no_map=round(1.0 - med["map"] / med["no_map"], 4))
    eng.close()
    print("RARE_IDS_COST " + json.dumps(dict(step="train", **res)), flush=True)


def step_quality(args):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "data", "libffm_data.txt.gz"), "rt") as f:
        lines = f.read().splitlines()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "train.ffm"), "w") as f:
            f.write("\n".join(lines[:8000]) + "\n")
        with open(os.path.join(d, "eval.ffm"), "w") as f:
            f.write("\n".join(lines[8000:]) + "\n")
        for T in (0, 2, 5, 10):
            text = cli(["--model_type", "FFM", "--train_data", "train.ffm", "--eval_data", "eval.ffm", "--n_epochs", "1", "--learn", "true",
                        "--hash_feats", "true", "--field_ranges", "uniform", "--metrics", "auc", "--batch_size", "256", "--w_alpha", "0.05",
                        "--w_l1", "0.01", "--w_l2", "0.1", "--min_count", str(T)], d)
            rare = [ln for ln in text.splitlines() if ln.startswith("rare ids:")]
            out[str(T)] = dict(eval_loss=float(re.search(r"eval loss: ([0-9.]+)", text).group(1)),
                               eval_auc=float(re.search(r"eval auc: ([0-9.]+)", text).group(1)),
                               train_loss=float(re.search(r"train loss: ([0-9.]+)", text).group(1)), rare_line=rare[-1] if rare else "")
    print("RARE_IDS_COST " + json.dumps(dict(step="quality", min_count=out)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="run this step in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--bits", type=int, default=27, help="train: slots of the keep-map, 2^bits")
    ap.add_argument("--min-count", type=int, default=2, help="train: the keep-map's min_count over the blocks it trains on")
    ap.add_argument("--blocks", type=int, default=64, help="train: distinct page-locked blocks, cycled")
    ap.add_argument("--steps", type=int, default=200, help="train: blocks per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="windows per path (prepass: runs per path)")
    ap.add_argument("--file-rows", type=int, default=65536, help="prepass: generated rows ...")
    ap.add_argument("--file-copies", type=int, default=8, help="prepass: ... written this many times")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.step:
        return dict(prepass=step_prepass, train=step_train, quality=step_quality)[args.step](args)
    results = []
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--n-feats", str(args.n_feats), "--bits", str(args.bits), "--min-count", str(args.min_count), "--blocks", str(args.blocks),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats),
               "--file-rows", str(args.file_rows), "--file-copies", str(args.file_copies)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("rare_ids_cost: %s ended with status %d" % (step, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith("RARE_IDS_COST ")][-1]
        results.append(json.loads(line[len("RARE_IDS_COST "):]))
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
