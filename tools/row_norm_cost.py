#!/usr/bin/env python3
"""What FFM_FLAG_NORM_ROWS costs (include/ffm_engine.h "Normalised rows"); the numbers of profiles/row_norm.md.

  python tools/row_norm_cost.py --prev PATH    the whole comparison: the kernel times once, then the staged training
                                               step with this tree's library (flag off and on) and the parent commit's
                                               (PATH: its libffm_engine.so) in alternating child processes, `--rounds`
                                               of each; medians and spreads at the end
  python tools/row_norm_cost.py                this tree's library alone
  python tools/row_norm_cost.py --case step --flag on     one case in this process, one JSON line

Shape: the headline one -- FFM 39 fields x 16 factors, 33 M features, blocks of 8192 rows x 39 entries from synth.py
with log-normal values (sigma = 2), a ring of page-locked blocks handed over zero_copy (train_batch_async_pinned).
Cases:
  kernels  the engine's per-kernel profile of 64 staged blocks on a flagged engine: normalize_rows_kernel next to
           pull_block_kernel (the upload of the same blocks, from the same run) -- profiling serialises the streams,
           so these are the kernels' own times, not what a step pays for them
  step     the staged training step, profiler off: windows of about `--window` seconds, rows/s and ms per block
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares settings."""
import argparse
import copy
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIELDS, N_FACTORS, FEATS, ROWS = 39, 16, 33_000_000, 8192
NEW_SYMBOLS = ("ffm_engine_normalize_rows_device", "ffm_engine_normalize_rows_host", "ffm_engine_norm_stats")


def run_case(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("row_norm_cost needs a GPU: none found")
    if args.lib:
        os.environ["FFM_ENGINE_LIB"] = args.lib
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    if args.lib:  # (a library of the parent commit: it has every symbol but the three this flag added)
        fa.engine.ABI[:] = [a for a in fa.engine.ABI if a[0] not in NEW_SYMBOLS]
    else:
        fa.build()
    flagged = args.flag == "on"
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    kw = dict(normalize=True) if flagged else {}
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, **kw)
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    rng = np.random.default_rng(42)
    ring = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        own = copy.copy(b)
        for key in ("row_ptr", "field", "feat", "val", "label"):
            a = fa.page_aligned(getattr(b, key).size, getattr(b, key).dtype)
            a[:] = getattr(b, key)
            setattr(own, key, a)
        own.val[:] = rng.lognormal(0.0, 2.0, own.val.size).astype(np.float32)
        eng.pin_block(own)
        ring.append(own)
    torch.cuda.synchronize()

    def window(steps):
        t0 = time.perf_counter()
        for i in range(steps):
            eng.train_batch_async_pinned(ring[i % len(ring)])
        window.loss = eng.train_flush()
        return time.perf_counter() - t0

    window(2 * args.blocks)  # warm-up: every block, code objects loaded
    res = dict(case=args.case, flag=args.flag, lib=args.lib or "this tree", n_feats=nf, rows_per_block=ROWS, blocks=args.blocks)
    if args.case == "kernels":
        eng.profile_enable(True)
        window(64)
        table = eng.profile_dump()
        eng.profile_enable(False)
        res["profile"] = {m.group(1): dict(launches=int(m.group(2)), avg_us=float(m.group(3)))
                          for m in re.finditer(r"^(\S+)\s+launches=\s*(\d+)\s+total_ms=\s*[0-9.]+\s+avg_us=\s*([0-9.]+)", table, re.M)}
        res["block_bytes"] = dict(upload=4 * (ROWS + 1) + 4 * ROWS + 12 * ROWS * N_FIELDS, normalize_read_write=(4 + 4 + 4 + 4 + 4) * ROWS * N_FIELDS)
    else:
        per_block = window(64) / 64
        steps = max(64, int(args.window / per_block) + 1)
        ms = [1e3 * window(steps) / steps for _ in range(args.repeats)]
        res.update(steps_per_window=steps, ms_per_block=[round(x, 4) for x in ms], ms_per_block_median=statistics.median(ms),
                   rows_per_s_median=ROWS / statistics.median(ms) * 1e3, loss_sum=window.loss)
        if flagged:
            res["norm_stats"] = eng.norm_stats()
    eng.sync()
    for c in ring:
        eng.unpin_block(c)
    eng.close()
    print("ROW_NORM " + json.dumps(res), flush=True)


def child(args, case, flag, lib):
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--flag", flag,
           "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window), "--repeats", str(args.repeats)]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(p.stderr[-2000:])
    if p.returncode != 0:  # the first that fails ends the run (nothing more is started on the GPU)
        sys.stdout.write(p.stdout[-2000:])
        raise SystemExit("row_norm_cost: %s, flag %s (%s) ended with status %d" % (case, flag, lib or "this tree", p.returncode))
    line = [s for s in p.stdout.splitlines() if s.startswith("ROW_NORM ")][-1]
    print(line, flush=True)
    return json.loads(line[len("ROW_NORM "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("kernels", "step"), help="measure this case in this process (default: both, a child process each)")
    ap.add_argument("--flag", choices=("on", "off"), default="on")
    ap.add_argument("--lib", help="the engine library to load (default: this tree's)")
    ap.add_argument("--prev", help="the parent commit's libffm_engine.so: alternate with it")
    ap.add_argument("--rounds", type=int, default=5, help="child processes per setting")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=16, help="distinct page-locked blocks, cycled")
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, about")
    ap.add_argument("--repeats", type=int, default=5, help="windows per process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.case:
        return run_case(args)
    runs = [child(args, "kernels", "on", None)]
    prof = runs[0]["profile"]
    print("\n| kernel | launches | avg us |\n|---|---|---|")
    for name in ("pull_block_kernel", "normalize_rows_kernel"):
        print("| %s | %d | %.2f |" % (name, prof[name]["launches"], prof[name]["avg_us"]))
    settings = ([("parent", "off", os.path.abspath(args.prev))] if args.prev else []) + [("flag off", "off", None), ("flag on", "on", None)]
    steps = {name: [] for name, _, _ in settings}
    for _ in range(args.rounds):  # alternating: parent, off, on, parent, ...
        for name, flag, lib in settings:
            r = child(args, "step", flag, lib)
            runs.append(r)
            steps[name].append(r["ms_per_block_median"])
    base = "parent" if args.prev else "flag off"
    ref = statistics.median(steps[base])
    spread = (max(steps[base]) - min(steps[base])) / ref
    print("\n| setting | ms per block (median of %d runs) | min .. max | vs %s | %s's spread |\n|---|---|---|---|---|" % (args.rounds, base, base))
    for name, v in steps.items():
        rel = statistics.median(v) / ref - 1
        print("| %s | %.4f | %.4f .. %.4f | %+.2f%%%s | %.2f%% |" % (name, statistics.median(v), min(v), max(v), 100 * rel,
                                                                 "" if abs(rel) > spread or name == base else " (not established)", 100 * spread))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
