#!/usr/bin/env python3
"""Prediction rate of a training engine, an fp32 serving engine and an fp16 serving engine on the same blocks
(include/ffm_engine.h "Serving engines"; the numbers of profiles/serve_weights.md).

  python tools/serve_bench.py                 the three kinds, one process each, one after another (the three
                                              models do not fit in HBM together), a summary at the end
  python tools/serve_bench.py --kind f16      one kind, one JSON line
  python tools/serve_bench.py --candidates 26:13:64
                                              one context against many candidates (include/ffm_engine.h "Scoring
                                              candidates"; profiles/score_candidates.md): per serving format,
                                              ffm_engine_score_candidates[_device] against the same data spelled out
                                              as rows through ffm_engine_predict_batch[_device], same engine, same
                                              process, alternating windows

Shape: the headline one -- 39 fields x 16 factors, 33 M features --, Zipf blocks of 8192 rows from synth.py,
resident in HBM, through ffm_engine_predict_batch_device with labels (logits + logloss sum, as the evaluation
does).  Per kind: warm-up, then `--repeats` timed windows of at least `--window` seconds, each ending in a
synchronise; then, profiler on, the predict kernel's time per block from ffm_engine_profile_read.
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares kinds."""
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
HBM_PEAK = 8e12  # bytes/s (spec)


def bytes_per_row(kind, n_fields=N_FIELDS, k=N_FACTORS):
    """Bytes the algorithm needs per row: both slots of every field pair (k elements of 4 or 2 bytes each),
    the entries (field, id, value), their linear weights, the row's pointer, label and output."""
    elem = 2 if kind == "f16" else 4
    pairs = n_fields * (n_fields - 1) // 2
    return pairs * 2 * k * elem + n_fields * (12 + 4) + 4 + 4 + 4


def run_kind(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    t0 = time.perf_counter()
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42,
                    max_row_nnz=N_FIELDS, field_start=fs, serve=None if args.kind == "training" else args.kind)
    create_s = time.perf_counter() - t0
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        blocks.append((b.n_rows, int(b.row_ptr[-1]), d))
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def predict(i):
        n, nnz, d = blocks[i % len(blocks)]
        eng.predict_batch_device(n, nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                                 d["label"].data_ptr(), 0, out.data_ptr(), loss.data_ptr())

    for i in range(3 * len(blocks)):  # warm-up: every block, code objects loaded
        predict(i)
    eng.sync()
    # how many blocks make a window of the asked length
    t0 = time.perf_counter()
    for i in range(64):
        predict(i)
    eng.sync()
    per_block = (time.perf_counter() - t0) / 64
    steps = max(64, int(args.window / per_block * 1.1) + 1)
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for i in range(steps):
            predict(i)
        eng.sync()
        el = time.perf_counter() - t0
        assert el >= args.window * 0.9, (el, args.window)
        rates.append(ROWS * steps / el)
    checksum = float(out.double().sum().cpu())
    # the kernel alone: every launch timed by events (its own run: the event pairs slow the host)
    eng.profile_enable(True)
    for i in range(args.profile_blocks):
        predict(i)
    eng.sync()
    name, launches, ms = eng.profile_read()
    dump = eng.profile_dump()
    eng.profile_enable(False)
    kernel_us = 1e3 * ms / max(1, launches)
    bpr = bytes_per_row(args.kind)
    rates.sort()
    res = dict(kind=args.kind, n_feats=nf, n_fields=N_FIELDS, n_factors=N_FACTORS, rows_per_block=ROWS, blocks=len(blocks),
               steps_per_window=steps, create_s=round(create_s, 2), model_bytes=eng.model_bytes(),
               rows_per_s_median=rates[len(rates) // 2], rows_per_s_min=rates[0], rows_per_s_max=rates[-1],
               rows_per_s_all=[round(r, 1) for r in rates],
               kernel=name, kernel_launches=launches, kernel_us_per_block=round(kernel_us, 2),
               algorithmic_bytes_per_row=bpr, algorithmic_bytes_per_s=ROWS * bpr / (kernel_us * 1e-6),
               share_of_hbm_peak=ROWS * bpr / (kernel_us * 1e-6) / HBM_PEAK, bound="bandwidth (8 TB/s HBM peak)",
               out_checksum=checksum, profile=dump.strip().splitlines())
    eng.close()
    print("SERVE_BENCH " + json.dumps(res), flush=True)


def candidate_bytes(kind, cf, kf, per, k=N_FACTORS):
    """Algorithmic bytes per candidate of both paths.  Spelled out: bytes_per_row.  Candidate path: both slots of the
    pairs with a candidate member, 4 bytes per stored context x context term, the candidate's entries and linear
    weights, the staged context survivors (16 bytes each), pointer and output; plus the request's share (1 / per) of
    the context kernel: both slots of the context pairs, the terms and survivors written, the entries read."""
    elem = 2 if kind == "f16" else 4
    F = cf + kf
    shared = cf * (cf - 1) // 2
    gathered = F * (F - 1) // 2 - shared
    cand = gathered * 2 * k * elem + shared * 4 + kf * (12 + 4) + cf * 16 + 4 + 4 + 4 + 8
    ctx = shared * 2 * k * elem + shared * 4 + cf * (12 + 4) + cf * 16 + 4 + 8
    return dict(spelled_out=bytes_per_row(kind, F, k), candidate_path=cand + ctx / per, candidate_kernel=cand,
                context_kernel_per_request=ctx, pairs_gathered_per_candidate=gathered, terms_stored_per_request=shared)


def run_candidates(args):
    """--candidates CTXFIELDS:CANDFIELDS:PER_REQUEST on one serving engine: ffm_engine_score_candidates[_device]
    against ffm_engine_predict_batch[_device] on the spelled-out blocks of the same data, alternating windows."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    cf, kf, per = (int(x) for x in args.candidates.split(":"))
    F = cf + kf
    if cf < 0 or kf < 1 or per < 1 or ROWS % per or F > 128:
        raise SystemExit("--candidates CTXFIELDS:CANDFIELDS:PER_REQUEST: PER_REQUEST must divide %d, at most 128 fields" % ROWS)
    n_req = ROWS // per
    nf = args.n_feats - args.n_feats % F
    fs = (np.arange(F + 1, dtype=np.int64) * (nf // F)).astype(np.int32)
    eng = fa.Engine("FFM", nf, F, N_FACTORS, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, seed=42, max_row_nnz=F,
                    field_start=fs, serve=args.kind)
    gen = synth.Generator(F, nf, dist="zipf", seed=42)
    rq = (np.arange(n_req + 1, dtype=np.int64) * per).astype(np.int32)
    host, dev = [], []

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        field, feat, val = (getattr(b, key).reshape(ROWS, F) for key in ("field", "feat", "val"))
        first = np.arange(n_req) * per  # the row whose first CTXFIELDS fields are the request's context
        ctx = synth.Block((np.arange(n_req + 1, dtype=np.int64) * cf).astype(np.int32), field[first, :cf].reshape(-1).copy(),
                          feat[first, :cf].reshape(-1).copy(), val[first, :cf].reshape(-1).copy(), np.zeros(n_req, np.int32))
        cand = synth.Block((np.arange(ROWS + 1, dtype=np.int64) * kf).astype(np.int32), field[:, cf:].reshape(-1).copy(),
                           feat[:, cf:].reshape(-1).copy(), val[:, cf:].reshape(-1).copy(), np.zeros(ROWS, np.int32))
        rows = fa.spell_out_candidates(ctx, rq, cand)
        host.append((ctx, cand, rows))
        dev.append(dict(ctx={key: up(getattr(ctx, key)) for key in ("row_ptr", "field", "feat", "val")},
                        cand={key: up(getattr(cand, key)) for key in ("row_ptr", "field", "feat", "val")},
                        rows={key: up(getattr(rows, key)) for key in ("row_ptr", "field", "feat", "val")},
                        nnz=(int(ctx.row_ptr[-1]), int(cand.row_ptr[-1]), int(rows.row_ptr[-1]))))
    d_rq = up(rq)
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def spelled_dev(i):
        d = dev[i % len(dev)]
        r = d["rows"]
        eng.predict_batch_device(ROWS, d["nnz"][2], r["row_ptr"].data_ptr(), r["field"].data_ptr(), r["feat"].data_ptr(),
                                 r["val"].data_ptr(), None, 0, out.data_ptr(), None)

    def cand_dev(i):
        d = dev[i % len(dev)]
        c, k = d["ctx"], d["cand"]
        eng.score_candidates_device(n_req, c["row_ptr"].data_ptr(), c["field"].data_ptr(), c["feat"].data_ptr(), c["val"].data_ptr(),
                                    d_rq.data_ptr(), ROWS, k["row_ptr"].data_ptr(), k["field"].data_ptr(), k["feat"].data_ptr(),
                                    k["val"].data_ptr(), d["nnz"][0], d["nnz"][1], cf, 0, out.data_ptr())

    def spelled_host(i):
        eng.predict_batch(host[i % len(host)][2], with_loss=False)

    def cand_host(i):
        ctx, cand, _ = host[i % len(host)]
        eng.score_candidates(ctx, rq, cand)

    # the two paths give the same bits on every block (also the warm-up of every shape)
    equal = True
    for i in range(len(dev)):
        spelled_dev(i)
        eng.sync()
        want = out.cpu().numpy().copy()
        out.zero_()
        cand_dev(i)
        eng.sync()
        got = out.cpu().numpy()
        equal = equal and bool((got.view(np.uint32) == want.view(np.uint32)).all())
        ctx, cand, rows = host[i]
        equal = equal and bool((eng.score_candidates(ctx, rq, cand).view(np.uint32) == want.view(np.uint32)).all())
        equal = equal and bool((eng.predict_batch(rows, with_loss=False)[0].view(np.uint32) == want.view(np.uint32)).all())
    if not equal:
        raise SystemExit("serve_bench: the candidate path and the spelled-out rows differ in bits")

    def windows(paths):
        """Alternating timed windows of the paths; returns candidates/s per path."""
        steps = {}
        for name, fn in paths.items():
            for i in range(2 * len(dev)):
                fn(i)
            eng.sync()
            t0 = time.perf_counter()
            for i in range(16):
                fn(i)
            eng.sync()
            steps[name] = max(16, int(args.window / ((time.perf_counter() - t0) / 16) * 1.1) + 1)
        rates = {name: [] for name in paths}
        for _ in range(args.repeats):
            for name, fn in paths.items():
                t0 = time.perf_counter()
                for i in range(steps[name]):
                    fn(i)
                eng.sync()
                el = time.perf_counter() - t0
                assert el >= args.window * 0.9, (name, el, args.window)
                rates[name].append(ROWS * steps[name] / el)
        return {name: dict(median=sorted(r)[len(r) // 2], min=min(r), max=max(r), all=[round(x, 1) for x in r], steps_per_window=steps[name])
                for name, r in rates.items()}

    resident = windows(dict(spelled_out=spelled_dev, candidates=cand_dev))
    from_host = windows(dict(spelled_out=spelled_host, candidates=cand_host))

    def kernel_us(fn):
        eng.profile_enable(True)
        for i in range(args.profile_blocks):
            fn(i)
        eng.sync()
        dump = eng.profile_dump().strip().splitlines()
        eng.profile_enable(False)
        return {ln.split()[0]: float(ln.split("avg_us=")[1]) for ln in dump}, dump
    us_spelled, dump_spelled = kernel_us(spelled_dev)
    us_cand, dump_cand = kernel_us(cand_dev)
    by = candidate_bytes(args.kind, cf, kf, per)
    t_spelled = us_spelled["serve_wave_kernel"]
    t_cand = us_cand["serve_context_kernel"] + us_cand["serve_candidate_kernel"]

    def verdict(r):
        base, new = r["spelled_out"], r["candidates"]
        return dict(ratio_of_medians=new["median"] / base["median"], baseline_spread=base["max"] - base["min"],
                    faster=bool(new["median"] - base["median"] > base["max"] - base["min"]))
    res = dict(mode="candidates", kind=args.kind, n_feats=nf, ctx_fields=cf, cand_fields=kf, per_request=per, n_factors=N_FACTORS,
               candidates_per_block=ROWS, requests_per_block=n_req, blocks=len(dev), bitwise_equal=equal,
               resident=resident, resident_verdict=verdict(resident), from_host=from_host, from_host_verdict=verdict(from_host),
               kernel_us_per_block=dict(spelled_out=us_spelled, candidates=us_cand),
               kernel_us_per_block_sum=dict(spelled_out=t_spelled, candidates=t_cand),
               algorithmic_bytes_per_candidate=by,
               algorithmic_bytes_per_s=dict(spelled_out=ROWS * by["spelled_out"] / (t_spelled * 1e-6),
                                            candidates=ROWS * by["candidate_path"] / (t_cand * 1e-6)),
               share_of_hbm_peak=dict(spelled_out=ROWS * by["spelled_out"] / (t_spelled * 1e-6) / HBM_PEAK,
                                      candidates=ROWS * by["candidate_path"] / (t_cand * 1e-6) / HBM_PEAK),
               bound="bandwidth (8 TB/s HBM peak)", profile=dict(spelled_out=dump_spelled, candidates=dump_cand))
    eng.close()
    print("SERVE_BENCH " + json.dumps(res), flush=True)


def main_candidates(args):
    results = []
    for kind in ("f32", "f16"):  # one after another; the first that fails ends the run (nothing more is started on the GPU)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--kind", kind,
               "--candidates", args.candidates, "--n-feats", str(args.n_feats), "--blocks", str(args.blocks),
               "--window", str(args.window), "--repeats", str(args.repeats), "--profile-blocks", str(args.profile_blocks)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("serve_bench: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith("SERVE_BENCH ")][-1]
        results.append(json.loads(line[len("SERVE_BENCH "):]))
        print(line, flush=True)
    print("\n%-5s %-9s %-12s %16s %26s %8s" % ("kind", "blocks", "path", "cand/s median", "min .. max", "faster"))
    for r in results:
        for where in ("resident", "from_host"):
            for path in ("spelled_out", "candidates"):
                w = r[where][path]
                print("%-5s %-9s %-12s %16.0f %12.0f .. %-12.0f %8s" % (
                    r["kind"], where, path, w["median"], w["min"], w["max"],
                    r[where + "_verdict"]["faster"] if path == "candidates" else ""))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--candidates", metavar="CTXFIELDS:CANDFIELDS:PER_REQUEST",
                    help="score candidates against contexts (include/ffm_engine.h \"Scoring candidates\") on the serving kinds: "
                         "the first CTXFIELDS fields of one row are a request's context, the remaining CANDFIELDS fields of "
                         "PER_REQUEST rows its candidates; the baseline is the same data spelled out as rows, same engine")
    ap.add_argument("--kind", choices=KINDS, help="measure this kind in this process (default: all three, a child process each)")
    ap.add_argument("--n-feats", type=int, default=FEATS)
    ap.add_argument("--blocks", type=int, default=16, help="distinct blocks resident in HBM, cycled")
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-blocks", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", help="also write the results there as JSON")
    args = ap.parse_args()
    if args.candidates:
        if args.kind == "training":
            raise SystemExit("--candidates needs a serving kind (f32 or f16)")
        return run_candidates(args) if args.kind else main_candidates(args)
    if args.kind:
        return run_kind(args)
    results = []
    for kind in KINDS:  # one after another; the first that fails ends the run (nothing more is started on the GPU)
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--kind", kind,
               "--n-feats", str(args.n_feats), "--blocks", str(args.blocks), "--window", str(args.window),
               "--repeats", str(args.repeats), "--profile-blocks", str(args.profile_blocks)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            sys.stdout.write(p.stdout[-2000:])
            raise SystemExit("serve_bench: %s ended with status %d" % (kind, p.returncode))
        line = [s for s in p.stdout.splitlines() if s.startswith("SERVE_BENCH ")][-1]
        results.append(json.loads(line[len("SERVE_BENCH "):]))
        print(line, flush=True)
    base = results[0]
    spread = (base["rows_per_s_max"] - base["rows_per_s_min"]) / base["rows_per_s_median"]
    print("\n%-9s %14s %22s %12s %10s %9s %16s" % ("kind", "rows/s median", "min .. max", "kernel us", "bytes/row", "of 8 TB/s", "model bytes"))
    for r in results:
        print("%-9s %14.0f %10.0f .. %-10.0f %12.2f %10d %8.1f%% %16d" % (
            r["kind"], r["rows_per_s_median"], r["rows_per_s_min"], r["rows_per_s_max"], r["kernel_us_per_block"],
            r["algorithmic_bytes_per_row"], 100 * r["share_of_hbm_peak"], r["model_bytes"]))
    f32 = results[1]
    ok = f32["rows_per_s_median"] >= base["rows_per_s_median"] * (1 - spread)
    print("\nbaseline spread (max - min) / median: %.2f%%; fp32 serving / training engine: %.4f -> %s" % (
        100 * spread, f32["rows_per_s_median"] / base["rows_per_s_median"], "within the spread or faster" if ok else "SLOWER than the spread allows"))
    print("fp16 serving / fp32 serving: %.4f" % (results[2]["rows_per_s_median"] / f32["rows_per_s_median"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(results=results, baseline_spread=spread, f32_not_slower=ok), f, indent=1)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
