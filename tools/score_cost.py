#!/usr/bin/env python3
"""What per-row scores cost the pipelined prediction (profiles/score_cost.md).

Engine legs: the C5 shape (FFM, 39 fields, k = 16), 8192-row zero-copy blocks in page-locked memory,
the H2D inside the loop; `--steps` (200) calls of predict_batch_async after `--warmup` (5), ending in
train_flush(), timed with a host clock around the device synchronise.  Two legs, alternating, `--repeats`
(5) times each: scores=None and scores into a ring of page-locked buffers.  `--grid N` sets the download
kernel's workgroups (FFM_GRID_PUSH) for the engine it creates.  `--profile` adds one pass with per-kernel
events (profile_dump: the predict kernel beside the upload, the download kernel).

`--lib PATH --legs none`: the scores=None leg on another build of the library -- the parent commit's, on
the same machine and day -- bound through this binding (symbols that build lacks are left unbound).

`--cli`: the C++ trainer end to end on a generated libffm file: its evaluation pass (parse + upload +
predict + loss) against its scoring pass (the same, plus the scores back, formatted and written).

One JSON line per measurement on stdout."""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K, ROWS = 39, 16, 8192


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": [round(x, 1) for x in xs]}


def engine_legs(args):
    import torch
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import engine as eng_mod
    from ftrl_ffm_amd import synth
    if args.lib:
        have = ctypes.CDLL(args.lib)
        eng_mod.ABI[:] = [a for a in eng_mod.ABI if hasattr(have, a[0])]
        fa.load_library(args.lib)
    if args.grid:
        os.environ["FFM_GRID_PUSH"] = str(args.grid)
    free_b, _ = torch.cuda.mem_get_info()
    rec = 3 * F * K * 4
    nf = min(args.n_feats, (int(free_b * 0.9) - (4 << 30)) // rec)
    nf -= nf % F
    fs = (np.arange(F + 1, dtype=np.int64) * (nf // F)).astype(np.int32)
    e = fa.Engine("FFM", nf, F, K, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, max_row_nnz=F, seed=42, field_start=fs)
    e.fill_state(seed=7, n_lo=0.05, n_hi=1.0, z_stddev=0.3)
    gen = synth.Generator(F, nf, "zipf", seed=42)
    blocks, keep = [gen.block(ROWS) for _ in range(args.n_blocks)], []
    for b in blocks:
        for name in ("row_ptr", "field", "feat", "val", "label"):
            t = torch.from_numpy(getattr(b, name)).pin_memory()
            keep.append(t)
            setattr(b, name, t.numpy())
    legs = args.legs.split(",")
    bufs = [e.score_buffer(ROWS) for _ in range(args.n_blocks)] if "scores" in legs else []

    def run(leg, first, count):
        for i in range(count):
            j = (first + i) % args.n_blocks
            e.predict_batch_async(blocks[j], zero_copy=True, **({"scores": bufs[j], "output_prob": True} if leg == "scores" else {}))
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
    out = {"what": "engine", "lib": args.lib or "this tree", "n_feats": nf, "rows": ROWS, "steps": args.steps,
           "warmup": args.warmup, "grid_push": args.grid or "default", "unit": "M rows/s",
           "legs": {leg: spread(v) for leg, v in rates.items()}}
    if "scores" in legs:  # the last block's scores against the synchronous call: the timed path computes the same
        want, _ = e.predict_batch(blocks[(args.warmup + args.steps - 1) % args.n_blocks], output_prob=True)
        got = bufs[(args.warmup + args.steps - 1) % args.n_blocks]
        out["scores_equal_predict_batch"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    if args.profile:
        prof = {}
        for leg in legs:
            e.profile_enable(True)
            run(leg, 0, 50)
            prof[leg] = [ln for ln in e.profile_dump().splitlines() if ln.startswith(("row_kernel<predict>", "push_scores", "loss_sum"))]
            e.profile_enable(False)
        out["profile_50_steps"] = prof
    print(json.dumps(out), flush=True)
    for b in bufs:
        e.free_score_buffer(b)
    e.close()


def cli_legs(args):
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    main_bin, _ = fa.build_host()
    per = 25000
    gen = synth.Generator(F, F * per, "zipf", seed=42)
    pre = ["%d:" % j for j in range(F)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synth.ffm")
        t0 = time.time()
        with open(path, "w") as f:
            for _ in range(args.cli_rows // 32768):
                blk = gen.block(32768)
                feat, last, lab = blk.feat.reshape(-1, F).tolist(), blk.val.reshape(-1, F)[:, F - 1].tolist(), blk.label.tolist()
                f.write("".join("%d %s %d:%d:%.6g\n" % (lab[r], " ".join([pre[j] + str(feat[r][j]) + ":1" for j in range(F - 1)]),
                                                         F - 1, feat[r][F - 1], last[r]) for r in range(len(lab))))
        wrote = time.time() - t0
        cmd = [main_bin, "--train_data", path, "--eval_data", path, "--model_type", "FFM", "--n_fields", str(F),
               "--n_feats", str(F * per), "--n_factors", str(K), "--online", "true", "--n_epochs", "1", "--batch_size", str(ROWS),
               "--n_threads", str(args.threads), "--predict_data", path, "--predict_out", os.path.join(tmp, "scores.txt")]
        ev, sc = [], []
        for _ in range(args.repeats):
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(out.stdout + out.stderr)
            n = int(re.search(r"scored (\d+) rows", out.stdout).group(1))
            ev.append(n / float(re.search(r"eval time: ([0-9.]+)s", out.stdout).group(1)) / 1e6)
            sc.append(n / float(re.search(r"scored \d+ rows time: ([0-9.]+)s", out.stdout).group(1)) / 1e6)
        print(json.dumps({"what": "cli", "rows": n, "file_mb": round(os.path.getsize(path) / 1e6, 1), "threads": args.threads,
                          "scores_mb": round(os.path.getsize(os.path.join(tmp, "scores.txt")) / 1e6, 1),
                          "file_written_in_s": round(wrote, 1), "unit": "M rows/s",
                          "eval_pass": spread(ev), "scoring_pass": spread(sc)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--legs", default="none,scores")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-blocks", type=int, default=16)
    ap.add_argument("--n-feats", type=int, default=33_000_000)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-rows", type=int, default=262144)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    cli_legs(a) if a.cli else engine_legs(a)
