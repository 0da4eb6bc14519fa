#!/usr/bin/env python3
"""What per-row sample weights cost staged training (profiles/sample_weights.md).

The headline shape (FFM, 39 fields, k = 16, as many features as fit the device up to 33 M), 8192-row
zero-copy blocks in page-locked memory, the H2D inside the loop: `--steps` (200) calls of
ffm_engine_train_batch_async_weighted(zero_copy = 1) after `--warmup` (5), ending in train_flush(),
timed with a host clock around the device synchronise.  Two legs, alternating, `--repeats` (5) times
each: weight = NULL (the unweighted launches) and a page-locked weight array per block (the weighted
row kernel, the sixth array of the upload).  `--profile` adds one pass per leg with per-kernel events.

`--lib PATH`: another build of the library (the legs it has symbols for).

One JSON line on stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K, ROWS = 39, 16, 8192


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 3) for x in xs]}


def main(args):
    import torch
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import engine as eng_mod
    from ftrl_ffm_amd import synth
    if args.lib:
        have = ctypes.CDLL(args.lib)
        eng_mod.ABI[:] = [a for a in eng_mod.ABI if hasattr(have, a[0])]
        fa.load_library(args.lib)
    free_b, _ = torch.cuda.mem_get_info()
    rec = 3 * F * K * 4
    nf = min(args.n_feats, (int(free_b * 0.9) - (4 << 30)) // rec)
    nf -= nf % F
    fs = (np.arange(F + 1, dtype=np.int64) * (nf // F)).astype(np.int32)
    e = fa.Engine("FFM", nf, F, K, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, max_row_nnz=F, seed=42, field_start=fs)
    e.fill_state(seed=7, n_lo=0.05, n_hi=1.0, z_stddev=0.3)
    gen = synth.Generator(F, nf, "zipf", seed=42)
    blocks, weights, keep = [gen.block(ROWS) for _ in range(args.n_blocks)], [], []
    rng = np.random.default_rng(1)
    for b in blocks:
        for name in ("row_ptr", "field", "feat", "val", "label"):
            t = torch.from_numpy(getattr(b, name)).pin_memory()
            keep.append(t)
            setattr(b, name, t.numpy())
        # the class weights of negatives down-sampled one in four, times a file weight near one
        w = np.where(b.label > 0, 1.0, 4.0).astype(np.float32) * (0.5 + rng.random(ROWS).astype(np.float32))
        t = torch.from_numpy(w).pin_memory()
        keep.append(t)
        weights.append(t.numpy())
    legs = [leg for leg in args.legs.split(",") if leg == "null" or hasattr(e.lib, "ffm_engine_train_batch_async_weighted")]

    def run(leg, first, count):
        for i in range(count):
            j = (first + i) % args.n_blocks
            if leg == "null":
                e.train_batch_async_pinned(blocks[j])
            else:
                e.train_batch_async_pinned(blocks[j], weight=weights[j])
        return e.train_flush()

    rates = {leg: [] for leg in legs}
    for _ in range(args.repeats):
        for leg in legs:  # (alternating: both legs see the same minutes of the machine)
            run(leg, 0, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(leg, args.warmup, args.steps)
            torch.cuda.synchronize()
            rates[leg].append(ROWS * args.steps / (time.perf_counter() - t0) / 1e6)
    out = {"what": "staged training, zero-copy", "lib": args.lib or "this tree", "n_feats": nf, "rows": ROWS,
           "steps": args.steps, "warmup": args.warmup, "unit": "M rows/s", "legs": {leg: spread(v) for leg, v in rates.items()}}
    if len(legs) == 2:
        a, b = (statistics.median(rates[leg]) for leg in ("null", "weights"))
        out["ms_per_block"] = {"null": round(ROWS / a / 1e3, 4), "weights": round(ROWS / b / 1e3, 4),
                               "difference": round(ROWS / b / 1e3 - ROWS / a / 1e3, 4)}
    if args.profile:
        prof = {}
        for leg in legs:
            e.profile_enable(True)
            run(leg, 0, 50)
            prof[leg] = [ln for ln in e.profile_dump().splitlines() if ln.startswith(("row_kernel<train>", "update_kernel", "refresh"))]
            e.profile_enable(False)
        out["profile_50_steps"] = prof
    print(json.dumps(out), flush=True)
    e.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--legs", default="null,weights")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=16)
    ap.add_argument("--n-feats", type=int, default=33_000_000)
    ap.add_argument("--profile", action="store_true")
    main(ap.parse_args())
