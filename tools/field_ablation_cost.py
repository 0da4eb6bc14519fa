#!/usr/bin/env python3
"""What field ablation in one pass costs (include/ffm_engine.h "Field ablation"; the numbers of
profiles/field_ablation.md).

Per block of 8192 rows, on a training engine, an fp32 and an fp16 serving engine (one process each, one after
another: the three models do not fit in HBM together):
  one       ffm_engine_predict_batch_device of the block               (one prediction pass)
  ablated   ffm_engine_predict_ablated_device of the block             (all n_fields + 1 variants)
  forty     n_fields + 1 ffm_engine_predict_batch_device calls over the pre-built drop_field blocks
            (what ablation takes without the kernel)
Shape and model set-up: tools/serve_bench.py's -- 39 fields x 16 factors, 33 M features, Zipf blocks from
synth.py resident in HBM, labels given (logits + logloss sums, as the evaluation does).  The three paths run in
alternating timed windows of at least `--window` seconds, each ending in a synchronise; medians, and the
baseline's spread.  Before timing, `ablated` is checked against `forty` bit for bit on every block.
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares paths."""
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


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("field_ablation_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    V = N_FIELDS + 1
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    eng.ablation_enable()
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)

    def up(b):
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        return (b.n_rows, int(b.row_ptr[-1]), d)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        blocks.append((up(b), [up(fa.drop_field(b, v)) for v in range(N_FIELDS)]))
    out = torch.zeros(V * ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(V, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def predict(blk, v=0):
        n, nnz, d = blk
        eng.predict_batch_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                                 d["label"].data_ptr(), 0, out.data_ptr() + 4 * v * ROWS, loss.data_ptr() + 8 * v)

    def one(i):
        predict(blocks[i % len(blocks)][0])

    def ablated(i):
        n, nnz, d = blocks[i % len(blocks)][0]
        eng.predict_ablated_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                                   d["label"].data_ptr(), 0, out.data_ptr(), loss.data_ptr())

    def forty(i):
        whole, dropped = blocks[i % len(blocks)]
        for v in range(N_FIELDS):
            predict(dropped[v], v)
        predict(whole, N_FIELDS)

    # the two ways to the n_fields + 1 variants give the same bits on every block (also the warm-up of every shape)
    for i in range(len(blocks)):
        forty(i)
        eng.sync()
        want, want_loss = out.cpu().numpy().copy(), loss.cpu().numpy().copy()
        out.zero_()
        ablated(i)
        eng.sync()
        if not (out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all() or not np.array_equal(loss.cpu().numpy(), want_loss):
            raise SystemExit("field_ablation_cost: predict_ablated and the predictions of the dropped blocks differ in bits")
    paths = dict(one=one, ablated=ablated, forty=forty)
    steps = {}
    for name, fn in paths.items():
        for i in range(2 * len(blocks)):
            fn(i)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(8):
            fn(i)
        eng.sync()
        steps[name] = max(8, int(args.window / ((time.perf_counter() - t0) / 8) * 1.1) + 1)
    us = {name: [] for name in paths}
    for _ in range(args.repeats):  # alternating windows
        for name, fn in paths.items():
            t0 = time.perf_counter()
            for i in range(steps[name]):
                fn(i)
            eng.sync()
            el = time.perf_counter() - t0
            assert el >= args.window * 0.9, (name, el, args.window)
            us[name].append(1e6 * el / steps[name])
    med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
    res = dict(kind=args.kind, n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, rows_per_block=ROWS, blocks=len(blocks),
               bitwise_equal=True, steps_per_window=steps,
               us_per_block={name: dict(median=round(med[name], 2), min=round(min(v), 2), max=round(max(v), 2), all=[round(x, 2) for x in v])
                             for name, v in us.items()},
               baseline_spread=round((max(us["one"]) - min(us["one"])) / med["one"], 4),
               ablated_over_one=round(med["ablated"] / med["one"], 3), forty_over_ablated=round(med["forty"] / med["ablated"], 3))
    eng.close()
    print("FIELD_ABLATION_COST " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=KINDS, help="measure this kind in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=4, help="distinct blocks resident in HBM (each with its 39 dropped copies), cycled")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.kind:
        return run_kind(args)
    results = []
    for kind in KINDS:  # one after another; the first that fails ends the run (nothing more is started on the GPU)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--kind", kind,
               "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("field_ablation_cost: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith("FIELD_ABLATION_COST ")][-1]
        results.append(json.loads(line[len("FIELD_ABLATION_COST "):]))
        print(line, flush=True)
    print("\n%-9s %-8s %14s %24s" % ("kind", "path", "us/block median", "min .. max"))
    for r in results:
        for path in ("one", "ablated", "forty"):
            w = r["us_per_block"][path]
            print("%-9s %-8s %14.1f %11.1f .. %-11.1f" % (r["kind"], path, w["median"], w["min"], w["max"]))
        print("%-9s ablated / one = %.2f, forty / ablated = %.2f, spread of one (max - min) / median = %.1f%%" % (
            r["kind"], r["ablated_over_one"], r["forty_over_ablated"], 100 * r["baseline_spread"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
