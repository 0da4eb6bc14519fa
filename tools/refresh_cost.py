#!/usr/bin/env python3
"""What ffm_engine_refresh_weights costs at the headline size (profiles/refresh_cost.md).

Creates the headline model (FFM 39 x 16, 32 999 967 features; fewer when the device has less free memory)
and times the entry point -- a host clock around the synchronous call: drain, memset of the counters, the
kernel, 48 bytes back -- best of two, in three states:
  (a) the fresh model: no accumulator is live, everything is read, nothing is written;
  (b) after fill_state: every element is live and moves (a second fill_state with another seed sets up
      the second timing);
  (c) a second call right after (b): every element is live, nothing moves, nothing is written.
Beside each time: the bytes the pass must move -- 12 per stored element read, 4 written per moved one --
the rate they give and that rate as a fraction of the 6.0 TB/s the row kernel streams at (README).
A call on a small engine of the same record shape comes first, so that no timed call loads the kernel.

One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, K = 39, 16
ROW_KERNEL_TBPS = 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-feats", type=int, default=32_999_967)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import ftrl_ffm_amd as fa

    warm = fa.Engine("FFM", 39 * 64, F, K, max_batch_rows=64)
    warm.fill_state(seed=1)
    warm.refresh_weights()
    warm.close()

    free_b, _ = torch.cuda.mem_get_info()
    rec = 3 * F * K * 4 + 12
    nf = min(args.n_feats, (int(free_b * 0.95) - (6 << 30)) // rec)
    t0 = time.perf_counter()
    e = fa.Engine("FFM", nf, F, K, max_batch_rows=8192, max_batch_nnz=8192 * F, max_row_nnz=F, seed=42)
    create_s = time.perf_counter() - t0
    elements = nf + 1 + nf * F * K

    def timed():
        t = time.perf_counter()
        st = e.refresh_weights()
        return time.perf_counter() - t, st

    def record(times, st):
        best = min(times)
        nbytes = 12 * elements + 4 * (st["lin_moved"] + st["lat_moved"])
        return {"s": times, "best_s": best, "counters": st, "bytes": nbytes, "gb_per_s": nbytes / best / 1e9,
                "fraction_of_row_kernel_rate": nbytes / best / (ROW_KERNEL_TBPS * 1e12)}

    out = {"n_feats": nf, "row_len": F * K, "stored_elements": elements, "tensor_gb": 12 * elements / 1e9,
           "create_s": create_s, "row_kernel_tb_per_s": ROW_KERNEL_TBPS}
    ta, sa = zip(*[timed() for _ in range(2)])
    out["a_fresh"] = record(list(ta), sa[0])
    tb, tc, sb, sc = [], [], None, None
    for seed in (7, 8):
        t = time.perf_counter()
        e.fill_state(seed=seed, n_lo=0.05, n_hi=1.0, z_stddev=0.3)
        out.setdefault("fill_state_s", []).append(time.perf_counter() - t)
        dt, sb = timed()
        tb.append(dt)
        dt, sc = timed()
        tc.append(dt)
    out["b_filled"] = record(tb, sb)
    out["c_second_call"] = record(tc, sc)
    e.close()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
