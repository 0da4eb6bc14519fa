#!/usr/bin/env python3
"""What value buckets cost and what they buy (include/ffm_engine.h "Value buckets"; the numbers of
profiles/value_buckets.md).

Three steps, a child process each under its own `timeout`, one after another; the first that fails ends the run
(nothing more is started on the GPU):
  prepass   the trainer CLI's counting pre-pass (`--bucket_fields 0-12 --n_epochs 0`) next to its `--field_ranges
            counted --n_epochs 0` pass on the same generated file (39 fields; fields 0 .. 12 numeric, half of each
            one's entries one value) with the same --n_threads: seconds from the `in S s` of their summary lines, the
            two alternating; and the counting kernel's global adds per entry, from a sequential model of one
            workgroup's cache over its share of a block of the file (evictions plus the final flush)
  train     rows/s from page-locked host memory at the headline shape (bench.py's: FFM 39 x 16, 33 M features,
            8192-row Zipf blocks, staged two ahead, zero_copy) on ONE hashed engine, with a bucket table on 13 of its
            39 fields and without one, in alternating windows; the no-table run's own spread over its windows
  quality   eval logloss and AUC of one `--learn true` epoch over the bundled data (first 8000 rows train, last
            2000 evaluate) with field 7 raw and bucketed at B = 16 and 32.  Recorded, not judged
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

N_FIELDS, N_NUMERIC, N_FACTORS, FEATS, ROWS = 39, 13, 16, 33_000_000, 8192
STEPS = ("prepass", "train", "quality")
TAG = "VALUE_BUCKETS_COST "


def cli(args, cwd):
    import ftrl_ffm_amd as fa
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin] + args, cwd=cwd, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit("value_buckets_cost: the CLI ended with status %d: %s" % (out.returncode, out.stderr[-1000:]))
    return out.stdout


def skewed(block, seed):
    """Fields 0 .. 12 numeric: half of each one's entries hold 1.0, the others a log-normal count."""
    import numpy as np
    rng = np.random.default_rng(seed)
    numeric = block.field < N_NUMERIC
    n = int(numeric.sum())
    v = np.floor(rng.lognormal(3.0, 2.0, n)).astype(np.float32) + 2.0
    v[rng.random(n) < 0.5] = 1.0
    block.val = block.val.copy()
    block.val[numeric] = v
    return block


def step_prepass(args):
    import numpy as np
    from ftrl_ffm_amd import synth
    nf = 975000
    with tempfile.TemporaryDirectory() as d:
        blk = skewed(synth.Generator(N_FIELDS, nf, "zipf", seed=42, ones="array").block(args.file_rows), 1)
        text = synth.to_libffm_text(blk)
        path = os.path.join(d, "skewed.ffm")
        with open(path, "w") as f:
            for _ in range(args.file_copies):
                f.write(text)
        rows = args.file_rows * args.file_copies
        base = ["--model_type", "FFM", "--train_data", path, "--n_epochs", "0", "--hash_feats", "true", "--n_fields", str(N_FIELDS),
                "--n_feats", str(nf), "--n_threads", str(args.threads)]
        runs = {"buckets": base + ["--field_ranges", "uniform", "--bucket_fields", "0-%d" % (N_NUMERIC - 1)],
                "counted": base + ["--field_ranges", "counted"]}
        starts = {"buckets": "value buckets: counted", "counted": "field ranges: counted"}
        secs = {name: [] for name in runs}
        lines = {}
        cli(runs["counted"], d)  # (the page cache warm)
        for _ in range(args.repeats):
            for name, a in runs.items():
                out = cli(a, d)
                line = [ln for ln in out.splitlines() if ln.startswith(starts[name])][-1]
                lines[name] = line
                secs[name].append(float(re.search(r" in ([0-9.]+) s", line).group(1)))
        med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
        # the counting kernel's global adds per entry: workgroup 0's share of one counted block (32768 rows, 24
        # workgroups of 256 lanes, a lane four entries) through a sequential model of its cache (kernels_valhist.h)
        import ftrl_ffm_amd as fa
        n_blk = min(args.file_rows, 32768) * N_FIELDS
        bins, _ = fa.value_bins(blk.val[:n_blk])
        key = (blk.field[:n_blk].astype(np.int64) << 16) | bins
        mine = key[((np.arange(n_blk) // 4 // 256) % 24) == 0]
        ways, adds = {}, 0
        for k in mine.tolist():
            w = ways.setdefault(((k * 0x9e3779b1) & 0xffffffff) >> 22, {})
            if k in w:
                w[k] += 1
            elif len(w) < 2:
                w[k] = 1
            else:
                del w[min(w, key=w.get)]
                adds += 1
                w[k] = 1
        adds += sum(len(w) for w in ways.values())
        res = dict(rows=rows, bytes=os.path.getsize(path), threads=args.threads, seconds=secs, median_s=med,
                   counted_spread_s=round(max(secs["counted"]) - min(secs["counted"]), 4),
                   buckets_minus_counted_s=round(med["buckets"] - med["counted"], 4),
                   rows_per_s={name: round(rows / s) for name, s in med.items()},
                   model_entries=int(mine.size), model_distinct_pairs=int(np.unique(mine).size), model_global_adds=adds,
                   model_adds_per_entry=round(adds / max(1, mine.size), 4), last_line=lines)
    print(TAG + json.dumps(dict(step="prepass", **res)), flush=True)


def step_train(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("value_buckets_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42, ones="array")
    blocks, keep_alive = [], []
    vh = fa.ValueHistogram(N_FIELDS)
    for i in range(args.blocks):
        b = skewed(gen.block(ROWS), i)
        vh.add(b.field, b.val)
        for name in ("row_ptr", "field", "feat", "val", "label"):
            t = torch.from_numpy(getattr(b, name)).pin_memory()
            keep_alive.append(t)
            setattr(b, name, t.numpy())
        blocks.append(b)
    counts = vh.read()[0]
    vh.close()
    table = {f: fa.bucket_edges(counts[f], 32) for f in range(N_NUMERIC)}
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

    rates = {"no_table": [], "table": []}
    for which in ("no_table", "table"):  # warm-up of both paths (the bucketing upload kernel's code object too)
        eng.set_buckets(table if which == "table" else None)
        run(args.warmup)
    for _ in range(args.repeats):  # alternating windows
        for which in ("no_table", "table"):
            eng.set_buckets(table if which == "table" else None)
            t0 = time.perf_counter()
            run(args.steps)
            rates[which].append(ROWS * args.steps / (time.perf_counter() - t0))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    res = dict(n_feats=model_feats, edges={str(f): int(e.size) for f, e in table.items()}, steps_per_window=args.steps,
               rows_per_s={k: [round(x) for x in v] for k, v in rates.items()}, median={k: round(x) for k, x in med.items()},
               no_table_spread=round((max(rates["no_table"]) - min(rates["no_table"])) / med["no_table"], 4),
               table_over_no_table=round(med["table"] / med["no_table"], 4))
    eng.close()
    print(TAG + json.dumps(dict(step="train", **res)), flush=True)


def step_quality(args):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "data", "libffm_data.txt.gz"), "rt") as f:
        lines = f.read().splitlines()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "train.ffm"), "w") as f:
            f.write("\n".join(lines[:8000]) + "\n")
        with open(os.path.join(d, "eval.ffm"), "w") as f:
            f.write("\n".join(lines[8000:]) + "\n")
        for B in (0, 16, 32):
            text = cli(["--model_type", "FFM", "--train_data", "train.ffm", "--eval_data", "eval.ffm", "--n_epochs", "1", "--learn", "true",
                        "--hash_feats", "true", "--field_ranges", "uniform", "--metrics", "auc", "--batch_size", "256", "--w_alpha", "0.05",
                        "--w_l1", "0.01", "--w_l2", "0.1"] + (["--bucket_fields", "7", "--n_buckets", str(B)] if B else []), d)
            line = [ln for ln in text.splitlines() if ln.startswith("field 7:")]
            out["raw" if B == 0 else str(B)] = dict(eval_loss=float(re.search(r"eval loss: ([0-9.]+)", text).group(1)),
                                                    eval_auc=float(re.search(r"eval auc: ([0-9.]+)", text).group(1)),
                                                    train_loss=float(re.search(r"train loss: ([0-9.]+)", text).group(1)),
                                                    field_line=line[-1] if line else "")
    print(TAG + json.dumps(dict(step="quality", n_buckets=out)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=STEPS, help="run this step in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=64, help="train: distinct page-locked blocks, cycled")
    ap.add_argument("--steps", type=int, default=200, help="train: blocks per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="windows per path (prepass: runs per path)")
    ap.add_argument("--threads", type=int, default=8, help="prepass: --n_threads of both passes (at most 16)")
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
               "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--repeats", str(args.repeats), "--threads", str(args.threads), "--file-rows", str(args.file_rows),
               "--file-copies", str(args.file_copies)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("value_buckets_cost: %s ended with status %d" % (step, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith(TAG)][-1]
        results.append(json.loads(line[len(TAG):]))
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
