#!/usr/bin/env python3
"""What prediction under a pair mask costs (include/ffm_engine.h "Pair masks"; the numbers of
profiles/pair_mask.md).  A sibling of tools/pair_ablation_cost.py.

Per block of 8192 rows, on a training engine, an fp32 and an fp16 serving engine (one process each, one after
another: the three models do not fit in HBM together), ffm_engine_predict_batch_device of the block
  unmasked  without a mask: ffm_row_wave_kernel, the baseline
  full      under the mask that keeps every pair (the same bits: what the candidate walk and the queue cost)
  keep50 / keep25 / keep10
            under fixed-seed masks that keep that share of the 741 cross pairs (the diagonal's bits are set too: a
            row of this shape has one entry per field and so no diagonal pair)
Shape and model set-up: tools/serve_bench.py's -- 39 fields x 16 factors, 33 M features, Zipf blocks from
synth.py resident in HBM, labels given (logits + logloss sums, as the evaluation does).  The paths run in
alternating timed windows of at least `--window` seconds, each ending in a synchronise (set_pair_mask between two
windows, outside the timed part); medians, min .. max, and the baseline's spread.  Before timing, the full mask is
checked against the unmasked prediction bit for bit on every block, and its loss sum too.
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
SHARES = (50, 25, 10)
TAG = "PAIR_MASK_COST "


def masks(np, fa):
    """{path: kept pairs or None}: unmasked, full, and the seeded shares of the cross pairs."""
    cross = [(f, g) for f in range(N_FIELDS) for g in range(f + 1, N_FIELDS)]
    diagonal = [(f, f) for f in range(N_FIELDS)]
    out = {"unmasked": None, "full": cross + diagonal}
    for share in SHARES:
        order = np.random.default_rng(1000 + share).permutation(len(cross))
        out["keep%d" % share] = [cross[i] for i in sorted(order[:round(len(cross) * share / 100)])] + diagonal
    return out


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_mask_cost needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        blocks.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def one(i):
        n, nnz, d = blocks[i % len(blocks)]
        eng.predict_batch_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                                 d["label"].data_ptr(), 0, out.data_ptr(), loss.data_ptr())

    paths = masks(np, fa)
    words = {name: None if kept is None else fa.pair_mask(N_FIELDS, kept) for name, kept in paths.items()}
    # the full mask gives the unmasked bits and loss sum on every block (also the warm-up of both kernels)
    for i in range(len(blocks)):
        eng.set_pair_mask(None)
        one(i)
        eng.sync()
        want, want_loss = out.cpu().numpy().copy(), float(loss[0].cpu())
        out.zero_()
        eng.set_pair_mask(words["full"])
        one(i)
        eng.sync()
        if not (out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all() or float(loss[0].cpu()) != want_loss:
            raise SystemExit("pair_mask_cost: the full mask and the unmasked prediction differ in bits")
    steps = {}
    for name in paths:
        eng.set_pair_mask(words[name])
        for i in range(2 * len(blocks)):
            one(i)
        eng.sync()
        t0 = time.perf_counter()
        for i in range(8):
            one(i)
        eng.sync()
        steps[name] = max(8, int(args.window / ((time.perf_counter() - t0) / 8) * 1.1) + 1)
    us = {name: [] for name in paths}
    for _ in range(args.repeats):  # alternating windows
        for name in paths:
            eng.set_pair_mask(words[name])
            eng.sync()
            t0 = time.perf_counter()
            for i in range(steps[name]):
                one(i)
            eng.sync()
            el = time.perf_counter() - t0
            assert el >= args.window * 0.9, (name, el, args.window)
            us[name].append(1e6 * el / steps[name])
    med = {name: sorted(v)[len(v) // 2] for name, v in us.items()}
    res = dict(kind=args.kind, n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, rows_per_block=ROWS, blocks=len(blocks),
               bitwise_equal=True, steps_per_window=steps,
               cross_pairs_kept={name: None if kept is None else len(kept) - N_FIELDS for name, kept in paths.items()},
               us_per_block={name: dict(median=round(med[name], 2), min=round(min(v), 2), max=round(max(v), 2), all=[round(x, 2) for x in v])
                             for name, v in us.items()},
               baseline_spread=round((max(us["unmasked"]) - min(us["unmasked"])) / med["unmasked"], 4),
               over_unmasked={name: round(med[name] / med["unmasked"], 3) for name in paths})
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
            raise SystemExit("pair_mask_cost: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith(TAG)][-1]
        results.append(json.loads(line[len(TAG):]))
        print(line, flush=True)
    print("\n%-9s %-9s %6s %15s %24s %10s" % ("kind", "path", "pairs", "us/block median", "min .. max", "/ unmasked"))
    for r in results:
        for path, w in r["us_per_block"].items():
            kept = r["cross_pairs_kept"][path]
            print("%-9s %-9s %6s %15.1f %11.1f .. %-11.1f %9.2f" % (r["kind"], path, "741" if kept is None else kept, w["median"], w["min"],
                                                                     w["max"], r["over_unmasked"][path]))
        print("%-9s spread of unmasked (max - min) / median = %.1f%%" % (r["kind"], 100 * r["baseline_spread"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()
