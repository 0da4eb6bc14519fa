#!/usr/bin/env python3
"""What the pruning curve in one pass costs (include/ffm_engine.h "Pruning curve"; the numbers of
profiles/pair_curve.md).  A sibling of tools/pair_ablation_cost.py.

Per block of 8192 rows, on a training engine, an fp32 and an fp16 serving engine (one process each, one after
another: the three models do not fit in HBM together):
  one       ffm_engine_predict_batch_device of the block                    (one prediction pass)
  fields    ffm_engine_predict_ablated_device of the block                  (the n_fields + 1 field variants)
  curve64   ffm_engine_predict_pair_curve_device, 64 cuts, out == NULL      (the auto ladder: round(i V / 63); the scores
  curve8    the same with 8 cuts (every ninth of them)                       stay in the engine's scratch, the loss sums
                                                                            are written)
  masked    ffm_engine_predict_batch_device under each of the 64 cuts' masks, one after another: the 64 passes that
            curve64 replaces, summed (and the pass under the mask that keeps a quarter of the pairs, on its own)
With --baseline (a library built from another commit, loaded through FFM_ENGINE_LIB) only one, fields and the
quarter mask are timed: what the other commit has.  (That library lacks the curve's symbols, so --baseline takes
their entries out of the binding's ABI list, in place, for this process, before the library is loaded.)
Shape and model set-up: tools/serve_bench.py's -- 39 fields x 16 factors, 33 M features, Zipf blocks from synth.py
resident in HBM, labels given.  The level table is a seeded permutation of the 780 pairs.  The paths run in
alternating timed windows of at least `--window` seconds, each ending in a synchronise; medians, and the baseline's
spread.  Before timing, every variant of curve64 (scores written this once) is checked against the masked pass bit
for bit on the first block, and the last variant against `one` on every block.
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
TAG = "PAIR_CURVE_COST "


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_curve_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    if args.baseline:  # (a library from before the curve lacks its symbols: bind what it has)
        fa.engine.ABI[:] = [entry for entry in fa.engine.ABI if "pair_curve" not in entry[0]]
    else:
        fa.build()
    V = fa.pair_count(N_FIELDS)
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    eng.ablation_enable()
    # the ladder: a seeded order of the pairs as ranks (numpy here, so that a baseline library's binding can make it too)
    rank = np.empty(V, np.int64)
    rank[np.random.default_rng(7).permutation(V)] = np.arange(V)
    f, g = np.triu_indices(N_FIELDS)
    level = np.zeros((N_FIELDS, N_FIELDS), np.uint16)
    level[f, g] = rank
    level[g, f] = rank
    cuts64 = [(2 * i * V + 63) // 126 for i in range(64)]
    cuts8 = cuts64[::9]

    def mask_of(cut):
        bit = np.uint64(1) << np.arange(N_FIELDS, dtype=np.uint64)
        return ((level.astype(np.int64) < cut).astype(np.uint64) * bit[None, :]).sum(axis=1, dtype=np.uint64)

    quarter = mask_of(V // 4)
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        blocks.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros(65 * ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(65, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def csr(i):
        n, nnz, d = blocks[i % len(blocks)]
        return (n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(), d["label"].data_ptr(), 0)

    def one(i):
        eng.predict_batch_device(*csr(i), out.data_ptr(), loss.data_ptr())

    def fields(i):
        eng.predict_ablated_device(*csr(i), out.data_ptr(), loss.data_ptr())

    def curve(i, scores=None):
        eng.predict_pair_curve_device(*csr(i), scores, loss.data_ptr())

    if not args.baseline:
        # every variant is the masked pass of its cut, bit for bit (first block); the last is the prediction itself
        eng.pair_curve_enable(level, cuts64)
        curve(0, out.data_ptr())
        eng.sync()
        got, got_loss = out.cpu().numpy().reshape(65, ROWS).copy(), loss.cpu().numpy().copy()
        for c, cut in enumerate(cuts64):
            eng.set_pair_mask(mask_of(cut))
            one(0)
            eng.sync()
            if not (out[:ROWS].cpu().numpy().view(np.uint32) == got[c].view(np.uint32)).all() or float(loss[0].cpu()) != got_loss[c]:
                raise SystemExit("pair_curve_cost: variant %d of predict_pair_curve and the masked predict_batch differ in bits" % c)
        eng.set_pair_mask(None)
        for i in range(len(blocks)):
            one(i)
            eng.sync()
            want, want_loss = out[:ROWS].cpu().numpy().copy(), float(loss[0].cpu())
            curve(i, out.data_ptr())
            eng.sync()
            if not (out[64 * ROWS:].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all() or float(loss[64].cpu()) != want_loss:
                raise SystemExit("pair_curve_cost: the last variant of predict_pair_curve and predict_batch differ in bits")
    for i in range(len(blocks)):
        one(i)
        fields(i)
    eng.sync()

    # name -> (what to do before a window, outside its time; the call; what to do after)
    paths = {"one": (None, one, None), "fields": (None, fields, None),
             "quarter": (lambda: eng.set_pair_mask(quarter), one, lambda: eng.set_pair_mask(None))}
    if not args.baseline:
        paths["curve64"] = (lambda: eng.pair_curve_enable(level, cuts64), curve, None)
        paths["curve8"] = (lambda: eng.pair_curve_enable(level, cuts8), curve, None)

    def window(name, n):
        before, fn, after = paths[name]
        if before:
            before()
        for i in range(len(blocks)):
            fn(i)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        eng.sync()
        el = time.perf_counter() - t0
        if after:
            after()
        return el

    steps = {name: max(8, int(args.window / (window(name, 256) / 256) * 1.1) + 1) for name in paths}
    us = {name: [] for name in paths}
    masked_sum = []
    for _ in range(args.repeats):  # alternating windows
        for name in paths:
            el = window(name, steps[name])
            if el < args.window * 0.9:  # (the calibration ran slow: a longer window from here on, this one measured again)
                steps[name] = int(steps[name] * args.window / el * 1.1) + 1
                el = window(name, steps[name])
            assert el >= args.window * 0.9, (name, el, args.window)
            us[name].append(1e6 * el / steps[name])
        if not args.baseline:  # the 64 masked passes, each mask a short window of its own
            total = 0.0
            for cut in cuts64:
                eng.set_pair_mask(mask_of(cut))
                one(0)
                eng.sync()
                t0 = time.perf_counter()
                for i in range(args.mask_steps):
                    one(i)
                eng.sync()
                total += 1e6 * (time.perf_counter() - t0) / args.mask_steps
            eng.set_pair_mask(None)
            masked_sum.append(total)
    if masked_sum:
        us["masked64_sum"] = masked_sum
    med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
    res = dict(kind=args.kind, baseline=bool(args.baseline), n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, rows_per_block=ROWS,
               blocks=len(blocks), bitwise_equal=not args.baseline, steps_per_window=steps,
               us_per_block={name: dict(median=round(med[name], 2), min=round(min(v), 2), max=round(max(v), 2), all=[round(x, 2) for x in v])
                             for name, v in us.items()},
               baseline_spread=round((max(us["one"]) - min(us["one"])) / med["one"], 4),
               over_one={name: round(med[name] / med["one"], 3) for name in us})
    eng.close()
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", choices=KINDS, help="measure this kind in this process (default: all three, a child process each)")
    ap.add_argument("--baseline", action="store_true", help="the loaded library is another commit's: time only what it has")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=4, help="distinct blocks resident in HBM, cycled")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mask-steps", type=int, default=40, help="passes timed under each of the 64 masks, per repeat")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.kind:
        return run_kind(args)
    results = []
    for kind in KINDS:  # one after another; the first that fails ends the run (nothing more is started on the GPU)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--kind", kind,
               "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window), "--repeats", str(args.repeats),
               "--mask-steps", str(args.mask_steps)] + (["--baseline"] if args.baseline else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("pair_curve_cost: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith(TAG)][-1]
        results.append(json.loads(line[len(TAG):]))
        print(line, flush=True)
    print("\n%-9s %-13s %14s %24s %10s" % ("kind", "path", "us/block median", "min .. max", "/ one"))
    for r in results:
        for path, w in r["us_per_block"].items():
            print("%-9s %-13s %14.1f %11.1f .. %-11.1f %10.2f" % (r["kind"], path, w["median"], w["min"], w["max"], r["over_one"][path]))
        print("%-9s spread of one (max - min) / median = %.1f%%" % (r["kind"], 100 * r["baseline_spread"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
