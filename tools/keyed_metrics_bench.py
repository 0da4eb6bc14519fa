"""What keyed capture (the grouped AUC, include/ffm_engine.h "Metrics") costs: profiles/keyed_metrics.md is
written from one run of this.

Shape: the headline's rows -- FFM, 39 fields, k = 16, blocks of 8192 rows of one entry per field, Zipf(1.1) ids,
resident in HBM -- through ffm_engine_predict_batch_device with labels.  n_feats is smaller than the headline's
(--n-feats, default 39 * 65536): prediction reads the same bytes per row, and the model need not fill the device
to time a capture kernel.

  rows/s with capture off and on: windows of --blocks predictions, off and on alternating in one process,
      the median of five with min .. max
  one metrics_read_keyed over --read-rows captured rows (default 2^24), wall time, and its split into sort and
      rank pass by ffm_engine_profile_dump (a second read, timed per kernel)

Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ftrl_ffm_amd as fa  # noqa: E402
from ftrl_ffm_amd import synth  # noqa: E402

F, K, ROWS = 39, 16, 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-feats", type=int, default=F * 65536)
    ap.add_argument("--blocks", type=int, default=200, help="predictions per timed window")
    ap.add_argument("--resident", type=int, default=8, help="distinct blocks kept in HBM")
    ap.add_argument("--read-rows", type=int, default=1 << 24)
    ap.add_argument("--key-field", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    fa.build()
    e = fa.Engine("FFM", args.n_feats, F, K, max_batch_rows=ROWS, max_batch_nnz=ROWS * F)
    gen = synth.Generator(F, args.n_feats, "zipf", seed=42)
    dev = []
    for _ in range(args.resident):
        b = gen.block(ROWS)
        dev.append({k: torch.from_numpy(np.ascontiguousarray(getattr(b, k))).cuda() for k in ("row_ptr", "field", "feat", "val", "label")})
    torch.cuda.synchronize()

    def predict(i):
        t = dev[i % len(dev)]
        e.predict_batch_device(ROWS, ROWS * F, t["row_ptr"].data_ptr(), t["field"].data_ptr(), t["feat"].data_ptr(),
                               t["val"].data_ptr(), t["label"].data_ptr(), 0, None, None)

    def window(n):
        e.sync()
        t0 = time.perf_counter()
        for i in range(n):
            predict(i)
        e.sync()
        return n * ROWS / (time.perf_counter() - t0)

    cap = max(args.read_rows, 5 * args.blocks * ROWS)
    window(20)  # warm-up
    rates = {"off": [], "on": []}
    for _ in range(5):
        e.metrics_key_field(args.key_field, cap, eval=False, train=False)
        rates["off"].append(window(args.blocks))
        e.metrics_key_field(args.key_field, cap, eval=True)
        rates["on"].append(window(args.blocks))
    # one read over read_rows captured rows
    e.metrics_key_field(args.key_field, cap, eval=False, train=False)
    e.metrics_key_field(args.key_field, args.read_rows, eval=True)
    for i in range((args.read_rows + ROWS - 1) // ROWS):
        predict(i)
    e.sync()
    t0 = time.perf_counter()
    m = e.metrics_read_keyed("eval")
    read_s = time.perf_counter() - t0
    e.profile_enable(True)
    e.metrics_read_keyed("eval")
    dump = e.profile_dump()
    e.profile_enable(False)
    ms = {name: float(t) for name, t in re.findall(r"^(keyed_\S+)\s+launches=\s*\d+\s+total_ms=\s*([0-9.]+)", dump, re.M)}
    sort_ms = sum(v for k, v in ms.items() if k.startswith("keyed_sort"))
    rank_ms = sum(v for k, v in ms.items() if k.startswith("keyed_rank"))
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    out = {"shape": "FFM F=%d k=%d rows=%d n_feats=%d zipf resident=%d" % (F, K, ROWS, args.n_feats, args.resident),
           "window_blocks": args.blocks, "rows_per_s_off": summary(rates["off"]), "rows_per_s_on": summary(rates["on"]),
           "read_rows": m["n_rows"], "read_keys": m["n_keys"], "read_keys_mixed": m["n_keys_mixed"], "read_overflow": m["n_overflow"],
           "gauc": m["gauc"], "read_wall_ms": 1e3 * read_s, "read_sort_ms": sort_ms, "read_rank_ms": rank_ms, "read_kernels_ms": ms}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
