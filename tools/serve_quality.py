#!/usr/bin/env python3
"""What a serving format costs in quality, and what its pack pass costs in time (profiles/serve_f8.md).

  quality   an FFM model (the CLI's defaults: 10000 features, 8 fields, 16 factors, --learn true) is trained online
            for --epochs epochs on the bundled libffm file, refreshed, and packed into an f32, an f16 and an f8
            serving engine (ffm_engine_pack_weights).  Per format: the pack counters, mean logloss and exact rank AUC of
            predict_batch on the same rows, and how far the probabilities are from the f32 engine's.
  pack      a 39 x 16 training engine of --pack-feats features with its create-time draws, packed --repeats times into
            an f16 and an f8 serving engine in turn; pack_weights is synchronous, so a host clock around it is the pass.
It needs a GPU and fails without one.  One JSON line per part."""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "tests", "golden", "data", "libffm_data.txt.gz")
NF, F, K, BATCH = 10000, 8, 16, 256


def rank_auc(score, label):
    order = np.argsort(score, kind="stable")
    s, y = score[order], label[order]
    edges = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1], [True]]))
    ranks = np.repeat((edges[:-1] + edges[1:] + 1) / 2.0, np.diff(edges))  # ties share their mean rank
    p = int(y.sum())
    return float((ranks[y > 0].sum() - p * (p + 1) / 2.0) / (p * (y.size - p)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--pack-feats", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_quality needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    rows = [ln.split() for ln in gzip.open(DATA, "rt").read().splitlines()]
    ent = [[tok.split(":") for tok in r[1:]] for r in rows]
    blk = synth.Block(np.concatenate([[0], np.cumsum([len(e) for e in ent])]).astype(np.int32),
                      np.array([int(t[0]) for e in ent for t in e], np.int32), np.array([int(t[1]) for e in ent for t in e], np.int32),
                      np.array([float(t[2]) for e in ent for t in e], np.float32), np.array([int(r[0]) > 0 for r in rows], np.int32))
    n, y = blk.n_rows, blk.label.astype(np.float64)
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, learn=True)
    for _ in range(args.epochs):
        for lo in range(0, n, BATCH):
            t.train_batch(blk.rows(lo, min(n, lo + BATCH)))
    t.refresh_weights()
    res, p32 = {}, None
    for fmt in ("f32", "f16", "f8"):
        s = fa.Engine("FFM", NF, F, K, max_batch_rows=BATCH, max_batch_nnz=BATCH * 256, serve=fmt, skip_init=True)
        stats = s.pack_from(t)
        p = np.concatenate([s.predict_batch(blk.rows(lo, min(n, lo + BATCH)), output_prob=True)[0] for lo in range(0, n, BATCH)]).astype(np.float64)
        p32 = p if p32 is None else p32
        res[fmt] = dict(stats, logloss=float(np.mean(-(y * np.log(p) + (1 - y) * np.log1p(-p)))), auc=rank_auc(p, blk.label),
                        probs_differing_from_f32=int((p != p32).sum()), largest_difference=float(np.abs(p - p32).max()))
        s.close()
    w = t.get_weights()["vec_w"]
    t.close()
    print("SERVE_QUALITY " + json.dumps(dict(rows=n, epochs=args.epochs, nonzero_w=int((w != 0).sum()), largest_w=float(np.abs(w).max()),
                                             formats=res)), flush=True)
    nf = args.pack_feats - args.pack_feats % 39
    t = fa.Engine("FFM", nf, 39, 16, max_batch_rows=64, max_batch_nnz=64 * 39)
    serve = {fmt: fa.Engine("FFM", nf, 39, 16, max_batch_rows=64, max_batch_nnz=64 * 39, serve=fmt, skip_init=True) for fmt in ("f16", "f8")}
    times = {fmt: [] for fmt in serve}
    for i in range(args.repeats + 1):  # (the first round warms up: code objects, the counter buffer)
        for fmt, s in serve.items():
            t0 = time.perf_counter()
            st = s.pack_from(t)
            if i:
                times[fmt].append(time.perf_counter() - t0)
    src_bytes = nf * 39 * 16 * 4
    print("SERVE_PACK " + json.dumps(dict(n_feats=nf, source_bytes_of_w=src_bytes, last_f8_stats=st, formats={
        fmt: dict(ms_median=1e3 * sorted(v)[len(v) // 2], ms_min=1e3 * min(v), ms_max=1e3 * max(v),
                  source_GBps=src_bytes / sorted(v)[len(v) // 2] / 1e9) for fmt, v in times.items()})), flush=True)


if __name__ == "__main__":
    main()
