#!/usr/bin/env python3
"""What pair ablation in one pass costs (include/ffm_engine.h "Pair ablation"; the numbers of
profiles/pair_ablation.md).  A sibling of tools/field_ablation_cost.py.

Per block of 8192 rows, on a training engine, an fp32 and an fp16 serving engine (one process each, one after
another: the three models do not fit in HBM together):
  one       ffm_engine_predict_batch_device of the block                    (one prediction pass)
  fields    ffm_engine_predict_ablated_device of the block                  (the n_fields + 1 field variants)
  pairs     ffm_engine_predict_pair_ablated_device of the block, out == NULL (all V + 1 = 781 pair variants: the
            scores stay in the engine's scratch, the V + 1 loss sums are written)
Shape and model set-up: tools/serve_bench.py's -- 39 fields x 16 factors, 33 M features, Zipf blocks from
synth.py resident in HBM, labels given (logits + logloss sums, as the evaluation does).  The three paths run in
alternating timed windows of at least `--window` seconds, each ending in a synchronise; medians, and the
baseline's spread.  Before timing, variant V of `pairs` (scores written this once) is checked against `one` bit
for bit on every block, and its loss sum too.
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
TAG = "PAIR_ABLATION_COST "


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_ablation_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    V = fa.pair_count(N_FIELDS)
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    eng.ablation_enable()
    eng.pair_ablation_enable()
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        blocks.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros((V + 1) * ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(V + 1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def csr(i):
        n, nnz, d = blocks[i % len(blocks)]
        return (n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(), d["label"].data_ptr(), 0)

    def one(i):
        eng.predict_batch_device(*csr(i), out.data_ptr(), loss.data_ptr())

    def fields(i):
        eng.predict_ablated_device(*csr(i), out.data_ptr(), loss.data_ptr())

    def pairs(i, scores=None):
        eng.predict_pair_ablated_device(*csr(i), scores, loss.data_ptr())

    # variant V is the prediction itself, bit for bit, on every block (also the warm-up of every shape)
    for i in range(len(blocks)):
        one(i)
        eng.sync()
        want, want_loss = out[:ROWS].cpu().numpy().copy(), float(loss[0].cpu())
        out.zero_()
        pairs(i, out.data_ptr())
        eng.sync()
        got = out[V * ROWS:(V + 1) * ROWS].cpu().numpy()
        if not (got.view(np.uint32) == want.view(np.uint32)).all() or float(loss[V].cpu()) != want_loss:
            raise SystemExit("pair_ablation_cost: variant V of predict_pair_ablated and predict_batch differ in bits")
        fields(i)
    eng.sync()
    paths = dict(one=one, fields=fields, pairs=pairs)
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
    res = dict(kind=args.kind, n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, variants=V + 1, rows_per_block=ROWS, blocks=len(blocks),
               bitwise_equal=True, steps_per_window=steps,
               us_per_block={name: dict(median=round(med[name], 2), min=round(min(v), 2), max=round(max(v), 2), all=[round(x, 2) for x in v])
                             for name, v in us.items()},
               baseline_spread=round((max(us["one"]) - min(us["one"])) / med["one"], 4),
               pairs_over_one=round(med["pairs"] / med["one"], 3), fields_over_one=round(med["fields"] / med["one"], 3),
               passes_replaced_over_pairs=round(V * med["one"] / med["pairs"], 2))
    eng.close()
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=KINDS, help="measure this kind in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=4, help="distinct blocks resident in HBM, cycled")
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
            raise SystemExit("pair_ablation_cost: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith(TAG)][-1]
        results.append(json.loads(line[len(TAG):]))
        print(line, flush=True)
    print("\n%-9s %-8s %14s %24s" % ("kind", "path", "us/block median", "min .. max"))
    for r in results:
        for path in ("one", "fields", "pairs"):
            w = r["us_per_block"][path]
            print("%-9s %-8s %14.1f %11.1f .. %-11.1f" % (r["kind"], path, w["median"], w["min"], w["max"]))
        print("%-9s pairs / one = %.2f, fields / one = %.2f, %d passes / pairs = %.1f, spread of one (max - min) / median = %.1f%%" % (
            r["kind"], r["pairs_over_one"], r["fields_over_one"], r["variants"] - 1, r["passes_replaced_over_pairs"], 100 * r["baseline_spread"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
