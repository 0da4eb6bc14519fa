#!/usr/bin/env python3
"""What a block gains on the wire when it crosses PCIe without its value array (val == NULL: every value is
1.0f, include/ffm_engine.h "Rows without values") and / or without its field array; the numbers of
profiles/implicit_ones.md.

  python tools/implicit_ones_cost.py --prev PATH     the whole comparison: this tree's library and the parent
                                                     commit's (PATH: its libffm_engine.so) in alternating child
                                                     processes, `--rounds` of each, medians and spreads at the end
  python tools/implicit_ones_cost.py                 this tree's library alone
  python tools/implicit_ones_cost.py --case f16      one case in this process, one JSON line

Shape: the headline one -- FFM 39 fields x 16 factors, 33 M features, blocks of 8192 rows from synth.py with
every value 1.0, a ring of page-locked blocks handed over zero_copy.  Cases:
  eval   evaluation on a training engine      (predict_batch_async, labels, loss at the flush)
  f32    the same on an fp32 serving engine
  f16    the same on an fp16 serving engine
  train  the training step                     (train_batch_async_pinned)
Each case, four wire forms -- five arrays | without fields | without values | without both (train: with and
without values) --, measured in interleaved windows of one process, and for the prediction cases the resident
rate (predict_batch_device on blocks already in HBM): the ceiling to quote next to them.  A library that
predates the convention (--old-abi) measures the forms it knows.
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares forms."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIELDS, N_FACTORS, FEATS, ROWS = 39, 16, 33_000_000, 8192
CASES = ("eval", "f32", "f16", "train")
FORMS = ("five", "no_field", "no_val", "neither")


def wire_bytes(form, rows=ROWS, n_fields=N_FIELDS):
    nnz = rows * n_fields
    return 4 * (rows + 1) + 4 * rows + 4 * nnz * (3 - (form in ("no_field", "neither")) - (form in ("no_val", "neither")))


def run_case(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("implicit_ones_cost needs a GPU: none found")
    if args.lib:
        os.environ["FFM_ENGINE_LIB"] = args.lib
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    if not args.lib:
        fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    train = args.case == "train"
    t0 = time.perf_counter()
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=args.case if args.case in ("f32", "f16") else None)
    create_s = time.perf_counter() - t0
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42, ones="array")
    forms = [f for f in (("five", "no_val") if train else FORMS) if not (args.old_abi and f in ("no_val", "neither"))]
    ring = {f: [] for f in forms}
    resident = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        own = copy.copy(b)
        for key in ("row_ptr", "field", "feat", "val", "label"):
            a = fa.page_aligned(getattr(b, key).size, getattr(b, key).dtype)
            a[:] = getattr(b, key)
            setattr(own, key, a)
        eng.pin_block(own)
        for f in forms:  # the same page-locked arrays, handed over with or without the optional two
            c = copy.copy(own)
            c.field = None if f in ("no_field", "neither") else own.field
            c.val = None if f in ("no_val", "neither") else own.val
            ring[f].append(c)
        if not train:
            d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
            resident.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def window(form, steps):
        """`steps` blocks of one form, through the flush; seconds."""
        t0 = time.perf_counter()
        if form == "resident":
            for i in range(steps):
                n, nnz, d = resident[i % len(resident)]
                eng.predict_batch_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                                         d["val"].data_ptr(), d["label"].data_ptr(), 0, out.data_ptr(), loss.data_ptr())
            eng.sync()
        else:
            blocks = ring[form]
            for i in range(steps):
                if train:
                    eng.train_batch_async_pinned(blocks[i % len(blocks)])
                else:
                    eng.predict_batch_async(blocks[i % len(blocks)], zero_copy=True)
            window.loss[form] = eng.train_flush()
        return time.perf_counter() - t0
    window.loss = {}

    kinds = list(forms) + ([] if train else ["resident"])
    for k in kinds:  # warm-up: every block of every form, code objects loaded
        window(k, 2 * args.blocks)
    per_block = max(window(k, 64) for k in kinds) / 64
    steps = max(64, int(args.window / per_block) + 1)
    rates = {k: [] for k in kinds}
    for _ in range(args.repeats):  # interleaved: form after form, `repeats` times over
        for k in kinds:
            rates[k].append(ROWS * steps / window(k, steps))
    res = dict(case=args.case, lib=args.lib or "this tree", old_abi=bool(args.old_abi), n_feats=nf, rows_per_block=ROWS,
               blocks=args.blocks, steps_per_window=steps, create_s=round(create_s, 2),
               rows_per_s={k: [round(r, 1) for r in v] for k, v in rates.items()},
               rows_per_s_median={k: statistics.median(v) for k, v in rates.items()},
               wire_bytes={k: wire_bytes(k) for k in forms},
               # (the forms of a prediction case see the same ids and the same values: the same loss)
               loss_sum={k: v for k, v in window.loss.items()})
    eng.sync()
    for c in ring[forms[0]]:
        eng.unpin_block(c)
    eng.close()
    print("IMPLICIT_ONES " + json.dumps(res), flush=True)


def child(args, case, lib, old_abi):
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
           "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window), "--repeats", str(args.repeats)]
    if lib:
        cmd += ["--lib", lib]
    if old_abi:
        cmd += ["--old-abi"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(p.stderr[-2000:])
    if p.returncode != 0:  # the first that fails ends the run (nothing more is started on the GPU)
        sys.stdout.write(p.stdout[-2000:])
        raise SystemExit("implicit_ones_cost: %s (%s) ended with status %d" % (case, lib or "this tree", p.returncode))
    line = [s for s in p.stdout.splitlines() if s.startswith("IMPLICIT_ONES ")][-1]
    print(line, flush=True)
    return json.loads(line[len("IMPLICIT_ONES "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=CASES, help="measure this case in this process (default: all, a child process each)")
    ap.add_argument("--cases", default=",".join(CASES), help="the cases of the whole comparison")
    ap.add_argument("--lib", help="the engine library to load (default: this tree's)")
    ap.add_argument("--old-abi", action="store_true", help="--lib predates val == NULL: skip the forms without values")
    ap.add_argument("--prev", help="the parent commit's libffm_engine.so: alternate with it")
    ap.add_argument("--rounds", type=int, default=5, help="child processes per library and case")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=16, help="distinct page-locked blocks, cycled")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window, about")
    ap.add_argument("--repeats", type=int, default=5, help="windows per form and process")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.case:
        return run_case(args)
    runs = []
    for case in args.cases.split(","):
        for _ in range(args.rounds):  # alternating: parent, this tree, parent, ...
            if args.prev:
                runs.append(child(args, case, os.path.abspath(args.prev), True))
            runs.append(child(args, case, None, False))
    print("\n| case | form | wire bytes | rows/s (median of %d runs) | min .. max | vs parent's five arrays | parent's spread |" % args.rounds)
    print("|---|---|---|---|---|---|---|")
    for case in args.cases.split(","):
        cur = [r for r in runs if r["case"] == case and not r["old_abi"]]
        old = [r for r in runs if r["case"] == case and r["old_abi"]]
        base = sorted(r["rows_per_s_median"]["five"] for r in old) if old else None
        spread = (base[-1] - base[0]) / statistics.median(base) if base else None
        rows = [("parent: " + k, old, k) for k in (old[0]["rows_per_s_median"] if old else ())]
        rows += [(k, cur, k) for k in cur[0]["rows_per_s_median"]]
        for label, group, k in rows:
            v = sorted(r["rows_per_s_median"][k] for r in group)
            med = statistics.median(v)
            rel = med / statistics.median(base) - 1 if base else None
            verdict = "" if rel is None else ("%+.2f%%%s" % (100 * rel, "" if abs(rel) > spread else " (not established)"))
            print("| %s | %s | %s | %.0f | %.0f .. %.0f | %s | %s |" % (
                case, label, wire_bytes(k) if k in FORMS else "-", med, v[0], v[-1], verdict,
                "" if spread is None else "%.2f%%" % (100 * spread)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
