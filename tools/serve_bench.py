#!/usr/bin/env python3
"""Prediction rate of a training engine, an fp32 serving engine and an fp16 serving engine on the same blocks
(include/ffm_engine.h "Serving engines"; the numbers of profiles/serve_weights.md).

  python tools/serve_bench.py                 the three kinds, one process each, one after another (the three
                                              models do not fit in HBM together), a summary at the end
  python tools/serve_bench.py --kind f16      one kind, one JSON line

Shape: the headline one -- 39 fields x 16 factors, 33 M features --, Zipf blocks of 8192 rows from synth.py,
resident in HBM, through ffm_engine_predict_batch_device with labels (logits + logloss sum, as the evaluation
does).  Per kind: warm-up, then `--repeats` timed windows of at least `--window` seconds, each ending in a
synchronise; then, profiler on, the predict kernel's time per block from ffm_engine_profile_read.
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares kinds."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIELDS, N_FACTORS, FEATS, ROWS = 39, 16, 33_000_000, 8192
KINDS = ("training", "f32", "f16")
HBM_PEAK = 8e12  # bytes/s (spec)


def bytes_per_row(kind, n_fields=N_FIELDS, k=N_FACTORS):
    """Bytes the algorithm needs per row: both slots of every field pair (k elements of 4 or 2 bytes each),
    the entries (field, id, value), their linear weights, the row's pointer, label and output."""
    elem = 2 if kind == "f16" else 4
    pairs = n_fields * (n_fields - 1) // 2
    return pairs * 2 * k * elem + n_fields * (12 + 4) + 4 + 4 + 4


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    t0 = time.perf_counter()
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    create_s = time.perf_counter() - t0
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        blocks.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def predict(i):
        n, nnz, d = blocks[i % len(blocks)]
        eng.predict_batch_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                                 d["label"].data_ptr(), 0, out.data_ptr(), loss.data_ptr())

    for i in range(3 * len(blocks)):  # warm-up: every block, code objects loaded
        predict(i)
    eng.sync()
    # how many blocks make a window of the asked length
    t0 = time.perf_counter()
    for i in range(64):
        predict(i)
    eng.sync()
    per_block = (time.perf_counter() - t0) / 64
    steps = max(64, int(args.window / per_block * 1.1) + 1)
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for i in range(steps):
            predict(i)
        eng.sync()
        el = time.perf_counter() - t0
        assert el >= args.window * 0.9, (el, args.window)
        rates.append(ROWS * steps / el)
    checksum = float(out.double().sum().cpu())
    # the kernel alone: every launch timed by events (its own run: the event pairs slow the host)
    eng.profile_enable(True)
    for i in range(args.profile_blocks):
        predict(i)
    eng.sync()
    name, launches, ms = eng.profile_read()
    dump = eng.profile_dump()
    eng.profile_enable(False)
    kernel_us = 1e3 * ms / max(1, launches)
    bpr = bytes_per_row(args.kind)
    rates.sort()
    res = dict(kind=args.kind, n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, rows_per_block=ROWS, blocks=len(blocks),
               steps_per_window=steps, create_s=round(create_s, 2), model_bytes=eng.model_bytes(),
               rows_per_s_median=rates[len(rates) // 2], rows_per_s_min=rates[0], rows_per_s_max=rates[-1],
               rows_per_s_all=[round(r, 1) for r in rates],
               kernel=name, kernel_launches=launches, kernel_us_per_block=round(kernel_us, 2),
               algorithmic_bytes_per_row=bpr, algorithmic_bytes_per_s=ROWS * bpr / (kernel_us * 1e-6),
               share_of_hbm_peak=ROWS * bpr / (kernel_us * 1e-6) / HBM_PEAK, bound="bandwidth (8 TB/s HBM peak)",
               out_checksum=checksum, profile=dump.strip().splitlines())
    eng.close()
    print("SERVE_BENCH " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=KINDS, help="measure this kind in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=16, help="distinct blocks resident in HBM, cycled")
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-blocks", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.kind:
        return run_kind(args)
    results = []
    for kind in KINDS:  # one after another; the first that fails ends the run (nothing more is started on the GPU)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--kind", kind,
               "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window),
               "--repeats", str(args.repeats), "--profile-blocks", str(args.profile_blocks)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("serve_bench: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith("SERVE_BENCH ")][-1]
        results.append(json.loads(line[len("SERVE_BENCH "):]))
        print(line, flush=True)
    base = results[0]
    spread = (base["rows_per_s_max"] - base["rows_per_s_min"]) / base["rows_per_s_median"]
    print("\n%-9s %14s %22s %12s %10s %9s %16s" % ("kind", "rows/s median", "min .. max", "kernel us", "bytes/row", "of 8 TB/s", "model bytes"))
    for r in results:
        print("%-9s %14.0f %10.0f .. %-10.0f %12.2f %10d %8.1f%% %16d" % (
            r["kind"], r["rows_per_s_median"], r["rows_per_s_min"], r["rows_per_s_max"], r["kernel_us_per_block"],
            r["algorithmic_bytes_per_row"], 100 * r["share_of_hbm_peak"], r["model_bytes"]))
    f32 = results[1]
    ok = f32["rows_per_s_median"] >= base["rows_per_s_median"] * (1 - spread)
    print("\nbaseline spread (max - min) / median: %.2f%%; fp32 serving / training engine: %.4f -> %s" % (
        100 * spread, f32["rows_per_s_median"] / base["rows_per_s_median"], "within the spread or faster" if ok else "SLOWER than the spread allows"))
    print("fp16 serving / fp32 serving: %.4f" % (results[2]["rows_per_s_median"] / f32["rows_per_s_median"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results, baseline_spread=spread, f32_not_slower=ok), f, indent=1)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
