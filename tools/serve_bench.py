#!/usr/bin/env python3
"""Prediction rate of a training engine, an fp32 serving engine and an fp16 serving engine on the same blocks
(include/ffm_engine.h "Serving engines"; the numbers of profiles/serve_weights.md).

  python tools/serve_bench.py                 the three kinds, one process each, one after another (the three
                                              models do not fit in HBM together), a summary at the end
  python tools/serve_bench.py --kind f16      one kind (training, f32, f16, f8), one JSON line
  python tools/serve_bench.py --pruned --kind f16
                                              pruned serving tables (include/ffm_engine.h "Pruned serving tables"):
                                              model bytes and per-block time against the unpruned engine under the
                                              same mask, keeping all, half, a quarter and a tenth of the cross pairs
  python tools/serve_bench.py --candidates 26:13:64
                                              one context against many candidates (include/ffm_engine.h "Scoring
                                              candidates"; profiles/score_candidates.md): per serving format,
                                              ffm_engine_score_candidates[_device] against the same data spelled out
                                              as rows through ffm_engine_predict_batch[_device], same engine, same
                                              process, alternating windows
  python tools/serve_bench.py --catalog --kind f16 [--topk 8 16 64]
                                              request contexts against a whole id range (include/ffm_engine.h "Scoring
                                              a catalogue"; profiles/score_catalog.md): ffm_engine_score_catalog_device
                                              for 32 and 128 requests x 65536 and 1048576 candidates, against the rate
                                              of ffm_engine_predict_batch_device on the same scores spelled out as rows,
                                              same engine, same process

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
KINDS = ("training", "f32", "f16", "f8")
HBM_PEAK = 8e12  # bytes/s (spec)


def bytes_per_row(kind, n_fields=N_FIELDS, k=N_FACTORS):
    """Bytes the algorithm needs per row: both slots of every field pair (k elements of 4 or 2 bytes each),
    the entries (field, id, value), their linear weights, the row's pointer, label and output."""
    elem = 1 if kind == "f8" else 2 if kind == "f16" else 4
    pairs = n_fields * (n_fields - 1) // 2
    scales = 4 * n_fields if kind == "f8" else 0  # (one scale word per entry: kernels_serve8.h)
    return pairs * 2 * k * elem + n_fields * (12 + 4) + scales + 4 + 4 + 4


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


def run_catalog(args):
    """One JSON line per (requests, candidates): median and spread of score_catalog_device's time, candidate-scores
    per second, bytes per second of the slab (n_cand rows of the table per pass of 128 requests); and the same
    engine's predict_batch_device on blocks of spelled-out rows [context..., (g, c, 1)], whose rate gives the time
    the same scores take as rows (measured on --blocks blocks of 8192 such rows, not on all of them)."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    nf = min(args.n_feats, 4_000_000)
    nf -= nf % N_FIELDS
    g, first, cf = N_FIELDS - 1, 1000, N_FIELDS - 1  # contexts: one entry in each of the other 38 fields
    lists = [int(x) for x in args.item_lists.replace(":", ",").split(",")] if args.item_lists else None  # [slots, len, len, ...]
    longest = N_FIELDS + max(args.catalog_items, lists[0] if lists else 0)  # (a spelled-out item row: the context and the item's entries)
    rows_cap = max(ROWS, 128 * max(lists[1:])) if lists else ROWS  # (the lists' baselines score every entry as a row)
    eng = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, max_batch_rows=rows_cap, max_batch_nnz=rows_cap * longest, seed=42,
                    max_row_nnz=longest, serve=args.kind)
    elem = 2 if args.kind == "f16" else 4
    blk = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42).block(128)
    keep = blk.field != g
    ctx = synth.Block(np.arange(129, dtype=np.int32) * cf, blk.field[keep], blk.feat[keep], blk.val[keep], np.zeros(128, np.int32))

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [up(ctx.row_ptr), up(ctx.field), up(ctx.feat), up(ctx.val)]
    out = torch.zeros(128 * (1 << 20), dtype=torch.float32, device="cuda")

    def windows(call, repeats=args.repeats, window=args.window):
        for _ in range(3):
            call()
        eng.sync()
        t0 = time.perf_counter()
        call()
        eng.sync()
        n = max(4, int(window / max(time.perf_counter() - t0, 1e-6)) + 1)
        us = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(n):
                call()
            eng.sync()
            us.append(1e6 * (time.perf_counter() - t0) / n)
        return sorted(us)

    if args.dict_slots:  # (its own baselines, in this process: no spelled-out rows)
        catalog_dict_lines(args, eng, windows, d, out, cf, up, nf)
        eng.close()
        return
    if lists:  # (its own baselines too)
        item_lists_lines(args, eng, windows, d, out, ctx, cf, up, nf, lists[0], lists[1:], elem)
        eng.close()
        return
    # the baseline: spelled-out rows of request r against candidates first + j, blocks of 8192 rows, cycled
    rows = []
    for b in range(args.blocks):
        cand = synth.Block(np.arange(ROWS + 1, dtype=np.int32), np.full(ROWS, g, np.int32),
                           (first + b * ROWS + np.arange(ROWS)).astype(np.int32), np.ones(ROWS, np.float32), np.zeros(ROWS, np.int32))
        one = synth.Block(ctx.row_ptr[b % 128:b % 128 + 2] - ctx.row_ptr[b % 128], *[a[(b % 128) * cf:(b % 128 + 1) * cf] for a in (ctx.field, ctx.feat, ctx.val)], np.zeros(1, np.int32))
        s = fa.spell_out_candidates(one, np.array([0, ROWS], np.int32), cand)
        rows.append((int(s.row_ptr[-1]), [up(a) for a in (s.row_ptr, s.field, s.feat, s.val)]))
    turn = [0]

    def spelled():
        nnz, a = rows[turn[0] % len(rows)]
        turn[0] += 1
        eng.predict_batch_device(ROWS, nnz, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), None, 0, out.data_ptr(), None)
    base_us = windows(spelled)
    base_rate = ROWS / (base_us[len(base_us) // 2] * 1e-6)
    for n_req in (32, 128):
        for n_cand in (65536, 1 << 20):
            us = windows(lambda: eng.score_catalog_device(n_req, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), g, first,
                                                          n_cand, 1.0, n_req * cf, cf, 0, out.data_ptr()))
            med = us[len(us) // 2]
            slab = n_cand * N_FIELDS * N_FACTORS * elem
            print("SERVE_BENCH " + json.dumps(dict(
                catalog=True, kind=args.kind, n_req=n_req, n_cand=n_cand, us_median=round(med, 1), us_min=round(us[0], 1),
                us_max=round(us[-1], 1), scores_per_s=n_req * n_cand / (med * 1e-6), slab_bytes=slab,
                slab_bytes_per_s=slab * ((n_req + 127) // 128) / (med * 1e-6), share_of_hbm_peak=slab / (med * 1e-6) / HBM_PEAK,
                rows_baseline_us_per_8192=[round(x, 1) for x in base_us], rows_baseline_scores_per_s=base_rate,
                rows_baseline_us_for_the_same_scores=round(n_req * n_cand / base_rate * 1e6, 1),
                speedup=n_req * n_cand / base_rate * 1e6 / med, checksum=float(out[:n_req * n_cand:4099].double().sum().cpu()))), flush=True)
            for K in args.topk:
                catalog_topk_line(args, eng, windows, d, out, g, first, cf, n_req, n_cand, K, med)
    if args.catalog_items:
        catalog_items_lines(args, eng, windows, d, out, ctx, cf, up, nf)
    eng.close()


def catalog_items_lines(args, eng, windows, d, out, ctx, cf, up, nf):
    """--catalog-items M: 2^20 items of M slots (the last M fields; slot 0's ids distinct, the others drawn from 1000,
    100, 10, 10, ... ids) through score_items_device and score_items_topk_device (K = 8), beside score_catalog_device on
    as many candidates and the spelled-out rows (65 536 of them, scaled), per 32 and 128 requests: one JSON line each."""
    import numpy as np
    import torch
    import ftrl_ffm_amd as fa
    M, n_items, K = args.catalog_items, 1 << 20, 8
    per = nf // N_FIELDS
    rng = np.random.default_rng(42)
    fld = np.arange(N_FIELDS - M, N_FIELDS, dtype=np.int32)[::-1].copy()  # slot 0: the catalogue's own field
    pool = [n_items] + [max(1, 1000 // 10 ** a) for a in range(M - 1)]
    feat = np.stack([1000 + np.arange(n_items) if a == 0 else fld[a] * per + rng.integers(pool[a], size=n_items) for a in range(M)],
                    axis=1).astype(np.int32)
    d_feat = up(feat)
    ptrs = [t.data_ptr() for t in d]
    score = torch.zeros(128 * K, dtype=torch.float32, device="cuda")
    ids = torch.zeros(128 * K, dtype=torch.int32, device="cuda")
    blocks, turn = [], [0]
    for b in range(8):  # 65 536 spelled-out rows as blocks of 8192, cycled
        sp = fa.spell_out_items(ctx.rows(b, b + 1), fld, feat[b * ROWS:(b + 1) * ROWS])
        blocks.append((int(sp.row_ptr[-1]), [up(a) for a in (sp.row_ptr, sp.field, sp.feat, sp.val)]))

    def spelled():
        nnz, a = blocks[turn[0] % len(blocks)]
        turn[0] += 1
        eng.predict_batch_device(ROWS, nnz, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), None, 0, out.data_ptr(), None)
    spelled_us = windows(spelled)
    rate = ROWS / (spelled_us[len(spelled_us) // 2] * 1e-6)
    for n_req in (32, 128):
        cells = dict(
            score_items_device=lambda: eng.score_items_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, n_req * cf, cf, 0,
                                                              out.data_ptr()),
            score_items_topk_device=lambda: eng.score_items_topk_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, K, n_req * cf,
                                                                        cf, 0, score.data_ptr(), ids.data_ptr()),
            score_catalog_device=lambda: eng.score_catalog_device(n_req, *ptrs, N_FIELDS - 1, 1000, n_items, 1.0, n_req * cf, cf, 0,
                                                                  out.data_ptr()))
        res = dict(catalog_items=M, kind=args.kind, n_req=n_req, n_items=n_items, top_k=K)
        for name, call in cells.items():
            us = windows(call, window=max(args.window, 0.3))
            res[name + "_us"] = dict(median=round(us[len(us) // 2], 1), min=round(us[0], 1), max=round(us[-1], 1))
        res["rows_us_for_the_same_scores"] = round(n_req * n_items / rate * 1e6, 1)
        res["rows_scores_per_s"] = rate
        res["items_over_catalog"] = res["score_items_device_us"]["median"] / res["score_catalog_device_us"]["median"]
        res["items_scores_per_s"] = n_req * n_items / (res["score_items_device_us"]["median"] * 1e-6)
        print("SERVE_BENCH " + json.dumps(res), flush=True)


def catalog_dict_lines(args, eng, windows, d, out, cf, up, nf):
    """--catalog-items M --dict-slots D: catalog_items_lines' table (2^20 items; slot 0's ids distinct, the others drawn
    from 1000, 100, 10, ... ids) with its last D slots as dictionaries (factor_items), through score_items_dict_device
    and its top 8, beside score_items_device on the expanded table and score_catalog_device on as many candidates, per
    32 and 128 requests: one JSON line each, medians of the windows with min .. max; score_items_device is measured
    twice, and the distance of the two medians is the run-to-run spread of this process."""
    import numpy as np
    import torch
    import ftrl_ffm_amd as fa
    M, D, n_items, K = args.catalog_items, args.dict_slots, 1 << 20, 8
    per = nf // N_FIELDS
    rng = np.random.default_rng(42)
    fld = np.arange(N_FIELDS - M, N_FIELDS, dtype=np.int32)[::-1].copy()
    pool = [n_items] + [max(1, 1000 // 10 ** a) for a in range(M - 1)]
    feat = np.stack([1000 + np.arange(n_items) if a == 0 else fld[a] * per + rng.integers(pool[a], size=n_items) for a in range(M)],
                    axis=1).astype(np.int32)
    gathered, code, dicts = fa.factor_items(feat, M - D)
    ptr = np.cumsum([0] + [len(x) for x in dicts]).astype(np.int32)
    d_feat, d_gath, d_code, d_dict = up(feat), up(gathered), up(code), up(np.concatenate(dicts))
    ptrs = [t.data_ptr() for t in d]
    score = torch.zeros(128 * K, dtype=torch.float32, device="cuda")
    ids = torch.zeros(128 * K, dtype=torch.int32, device="cuda")
    for n_req in (32, 128):
        def items():
            eng.score_items_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, n_req * cf, cf, 0, out.data_ptr())
        cells = dict(
            score_items_dict_device=lambda: eng.score_items_dict_device(n_req, *ptrs, M - D, fld, d_gath.data_ptr(), d_code.data_ptr(), ptr,
                                                                        d_dict.data_ptr(), None, n_items, n_req * cf, cf, 0, out.data_ptr()),
            score_items_dict_topk_device=lambda: eng.score_items_dict_topk_device(
                n_req, *ptrs, M - D, fld, d_gath.data_ptr(), d_code.data_ptr(), ptr, d_dict.data_ptr(), None, n_items, K, n_req * cf, cf, 0,
                score.data_ptr(), ids.data_ptr()),
            score_items_device=items,
            score_items_topk_device=lambda: eng.score_items_topk_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, K, n_req * cf, cf,
                                                                        0, score.data_ptr(), ids.data_ptr()),
            score_catalog_device=lambda: eng.score_catalog_device(n_req, *ptrs, N_FIELDS - 1, 1000, n_items, 1.0, n_req * cf, cf, 0,
                                                                  out.data_ptr()),
            score_items_device_again=items)
        res = dict(catalog_items=M, dict_slots=D, dict_sizes=[len(x) for x in dicts], kind=args.kind, n_req=n_req, n_items=n_items, top_k=K)
        for name, call in cells.items():
            us = windows(call, window=max(args.window, 0.3))
            res[name + "_us"] = dict(median=round(us[len(us) // 2], 1), min=round(us[0], 1), max=round(us[-1], 1))
        res["items_over_dict"] = res["score_items_device_us"]["median"] / res["score_items_dict_device_us"]["median"]
        res["dict_over_catalog"] = res["score_items_dict_device_us"]["median"] / res["score_catalog_device_us"]["median"]
        eng.profile_enable(True)
        for _ in range(10):
            cells["score_items_dict_device"]()
        eng.sync()
        res["profile"] = [ln for ln in eng.profile_dump().strip().splitlines() if "catalog" in ln]
        eng.profile_enable(False)
        print("SERVE_BENCH " + json.dumps(res), flush=True)


def item_lists_lines(args, eng, windows, d, out, ctx, cf, up, nf, M, lens, elem):
    """--item-lists SLOTS:LEN[,LEN...]: catalog_items_lines' table of 2^20 items of SLOTS slots; per 32 and 128 requests
    and per LEN, lists of LEN items drawn from the whole table through score_item_lists_device, beside (a)
    score_candidates_device on the same lists as candidates of SLOTS entries, (b) the same entries spelled out as rows
    through predict_batch_device and (c) score_items_device over the whole table: one JSON line each, medians of the
    windows with min .. max.  The list call is measured twice: the distance of its two medians is the run-to-run spread
    of this process.  gather_bytes: the table rows a call must read, entries * SLOTS * row bytes."""
    import numpy as np
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    n_items, per = 1 << 20, nf // N_FIELDS
    rng = np.random.default_rng(42)
    fld = np.arange(N_FIELDS - M, N_FIELDS, dtype=np.int32)[::-1].copy()
    pool = [n_items] + [max(1, 1000 // 10 ** a) for a in range(M - 1)]
    feat = np.stack([1000 + np.arange(n_items) if a == 0 else fld[a] * per + rng.integers(pool[a], size=n_items) for a in range(M)],
                    axis=1).astype(np.int32)
    d_feat, ptrs = up(feat), [t.data_ptr() for t in d]
    for n_req in (32, 128):
        whole = windows(lambda: eng.score_items_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, n_req * cf, cf, 0, out.data_ptr()),
                        window=max(args.window, 0.3))
        for ln in lens:
            n_list = n_req * ln
            lptr = (np.arange(n_req + 1, dtype=np.int64) * ln).astype(np.int32)
            item = rng.integers(n_items, size=n_list).astype(np.int32)
            cand = synth.Block((np.arange(n_list + 1, dtype=np.int64) * M).astype(np.int32), np.tile(fld, n_list), feat[item].reshape(-1),
                               np.ones(n_list * M, np.float32), np.zeros(n_list, np.int32))
            rows = fa.spell_out_candidates(ctx.rows(0, n_req), lptr, cand)
            keep =[up(a) for a in (lptr, item, cand.row_ptr, cand.field, cand.feat, cand.val, rows.row_ptr, rows.field, rows.feat, rows.val)]
            d_l, d_c, d_r = [t.data_ptr() for t in keep[:2]], [t.data_ptr() for t in keep[2:6]], [t.data_ptr() for t in keep[6:]]

            def listed():
                eng.score_item_lists_device(n_req, *ptrs, fld, d_feat.data_ptr(), None, n_items, *d_l, n_req * cf, cf, n_list, ln, 0,
                                            out.data_ptr())
            cells = dict(
                score_item_lists_device=listed,
                score_candidates_device=lambda: eng.score_candidates_device(n_req, *ptrs, d_l[0], n_list, *d_c, n_req * cf, n_list * M, cf, 0,
                                                                            out.data_ptr()),
                rows_predict_batch_device=lambda: eng.predict_batch_device(n_list, int(rows.row_ptr[-1]), *d_r, None, 0, out.data_ptr(), None),
                score_item_lists_device_again=listed)
            res = dict(item_lists=M, list_len=ln, kind=args.kind, n_req=n_req, n_items=n_items, entries=n_list,
                       gather_bytes=n_list * M * N_FIELDS * N_FACTORS * elem)
            for name, call in cells.items():
                us = windows(call, window=max(args.window, 0.3))
                res[name + "_us"] = dict(median=round(us[len(us) // 2], 1), min=round(us[0], 1), max=round(us[-1], 1))
            med = res["score_item_lists_device_us"]["median"]
            res["score_items_device_whole_table_us"] = dict(median=round(whole[len(whole) // 2], 1), min=round(whole[0], 1), max=round(whole[-1], 1))
            res["entries_per_s"] = n_list / (med * 1e-6)
            res["over_score_candidates"] = res["score_candidates_device_us"]["median"] / med
            res["over_rows"] = res["rows_predict_batch_device_us"]["median"] / med
            # the list length, as a share of the table, at which scoring the whole table costs what the lists cost (linear in LEN)
            res["break_even_share_of_table"] = whole[len(whole) // 2] / med * ln / n_items
            listed()
            eng.sync()
            res["checksum"] = float(out[:n_list].double().sum().cpu())
            eng.profile_enable(True)
            for _ in range(10):
                listed()
            eng.sync()
            res["profile"] = [x for x in eng.profile_dump().strip().splitlines() if "catalog_lists" in x or "row" in x]
            eng.profile_enable(False)
            print("SERVE_BENCH " + json.dumps(res), flush=True)


def catalog_topk_line(args, eng, windows, d, out, g, first, cf, n_req, n_cand, K, matrix_us):
    """score_catalog_topk_device against what a caller does without it -- score_catalog_device, then torch.topk on its
    matrix -- in this process; the profile calls' split between the two kernels; the bytes of partial lists a call
    writes and reads again."""
    import torch
    ptrs = [t.data_ptr() for t in d]
    score = torch.zeros(n_req * K, dtype=torch.float32, device="cuda")
    ids = torch.zeros(n_req * K, dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(eng.stream)

    def topk():
        eng.score_catalog_topk_device(n_req, *ptrs, g, first, n_cand, 1.0, K, n_req * cf, cf, 0, score.data_ptr(), ids.data_ptr())

    def matrix_then_topk():
        eng.score_catalog_device(n_req, *ptrs, g, first, n_cand, 1.0, n_req * cf, cf, 0, out.data_ptr())
        with torch.cuda.stream(stream):
            torch.topk(out[:n_req * n_cand].view(n_req, n_cand), K, dim=1)
    us, base = windows(topk), windows(matrix_then_topk)
    eng.profile_enable(True)
    for _ in range(20):
        topk()
    eng.sync()
    dump = eng.profile_dump()
    eng.profile_enable(False)
    kp = 1 << (K - 1).bit_length()
    grid = min((n_cand + 127) // 128, 2 * torch.cuda.get_device_properties(0).multi_processor_count)
    med, bmed = us[len(us) // 2], base[len(base) // 2]
    print("SERVE_BENCH " + json.dumps(dict(
        catalog_topk=True, kind=args.kind, n_req=n_req, n_cand=n_cand, top_k=K, us_median=round(med, 1), us_min=round(us[0], 1),
        us_max=round(us[-1], 1), matrix_then_torch_topk_us_median=round(bmed, 1), matrix_then_torch_topk_us_min=round(base[0], 1),
        matrix_then_torch_topk_us_max=round(base[-1], 1), matrix_alone_us_median=round(matrix_us, 1), speedup=bmed / med,
        over_matrix_alone=med / matrix_us, partial_list_bytes=n_req * grid * 4 * kp * 8,
        profile=[ln for ln in dump.strip().splitlines() if "catalog" in ln])), flush=True)


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


def run_pruned(args):
    """--pruned: per kept share of the 741 cross pairs (all, half, a quarter, a tenth; the diagonal kept), a pruned
    serving table (include/ffm_engine.h "Pruned serving tables") against the unpruned engine of the same format under
    the same mask, same process, alternating windows: model bytes, and predict_batch_device per block."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: none found")
    import ftrl_ffm_amd as fa
    from ftrl_ffm_amd import synth
    fa.build()
    fmt = args.kind or "f16"
    nf = args.n_feats - args.n_feats % N_FIELDS
    fs = (np.arange(N_FIELDS + 1, dtype=np.int64) * (nf // N_FIELDS)).astype(np.int32)
    kw = dict(max_batch_rows=ROWS, max_batch_nnz=ROWS * N_FIELDS, seed=42, max_row_nnz=N_FIELDS, field_start=fs, serve=fmt)
    gen = synth.Generator(N_FIELDS, nf, dist="zipf", seed=42)
    blocks = []
    for _ in range(args.blocks):
        b = gen.block(ROWS)
        blocks.append((b.n_rows, int(b.row_ptr[-1]),
                       [torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")]))
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    masked = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, **kw)
    cross = [(f, g) for f in range(N_FIELDS) for g in range(f + 1, N_FIELDS)]
    order = np.random.default_rng(7).permutation(len(cross))

    def window(eng, steps):
        t0 = time.perf_counter()
        for i in range(steps):
            n, nnz, d = blocks[i % len(blocks)]
            eng.predict_batch_device(n, nnz, *[a.data_ptr() for a in d], 0, out.data_ptr(), loss.data_ptr())
        eng.sync()
        return 1e6 * (time.perf_counter() - t0) / steps

    for share in (1.0, 0.5, 0.25, 0.1):
        kept = [cross[v] for v in order[:int(round(share * len(cross)))]] + [(f, f) for f in range(N_FIELDS)]
        words = fa.pair_mask(N_FIELDS, kept)
        masked.set_pair_mask(words)
        pruned = fa.Engine("FFM", nf, N_FIELDS, N_FACTORS, prune=words, **kw)
        steps = max(64, int(args.window / (window(masked, 64) * 1e-6)) + 1)  # (also the warm-up of both)
        window(pruned, 64)
        us = {"masked": [], "pruned": []}
        for _ in range(args.repeats):
            us["masked"].append(window(masked, steps))
            us["pruned"].append(window(pruned, steps))
        res = dict(fmt=fmt, n_feats=nf, kept_cross_pairs=len(kept) - N_FIELDS, steps_per_window=steps,
                   model_bytes_unpruned=masked.model_bytes(), model_bytes_pruned=pruned.model_bytes(),
                   **{key + "_us_per_block": dict(median=sorted(v)[len(v) // 2], min=min(v), max=max(v)) for key, v in us.items()})
        res["pruned_over_masked"] = res["pruned_us_per_block"]["median"] / res["masked_us_per_block"]["median"]
        pruned.close()
        print("SERVE_BENCH " + json.dumps(res), flush=True)
    masked.close()


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
    ap.add_argument("--pruned", action="store_true",
                    help="pruned serving tables against the masked unpruned engine, --kind f32 or f16 (default f16)")
    ap.add_argument("--catalog", action="store_true",
                    help="request contexts against a whole id range (include/ffm_engine.h \"Scoring a catalogue\"), --kind f32 or f16")
    ap.add_argument("--topk", type=int, nargs="*", default=[], metavar="K",
                    help="with --catalog: also the best K per request (score_catalog_topk_device) against the matrix call "
                         "followed by torch.topk")
    ap.add_argument("--catalog-items", type=int, default=0, metavar="M",
                    help="with --catalog: also items of M slots (score_items_device, its top 8) against score_catalog_device on as "
                         "many candidates and against spelled-out rows, in the same process (profiles/score_items.md)")
    ap.add_argument("--dict-slots", type=int, default=0, metavar="D",
                    help="with --catalog-items M: the last D of the M slots as dictionaries (score_items_dict_device, its top 8) "
                         "against score_items_device on the expanded table and score_catalog_device (profiles/score_items_dict.md)")
    ap.add_argument("--item-lists", metavar="SLOTS:LEN[,LEN...]",
                    help="per-request lists of LEN items of SLOTS slots out of 2^20 (score_item_lists_device) against "
                         "score_candidates_device, spelled-out rows and score_items_device over the whole table, --kind f32 or f16 "
                         "(profiles/score_item_lists.md)")
    args = ap.parse_args()
    if args.dict_slots and not 1 <= args.dict_slots < args.catalog_items:
        raise SystemExit("--dict-slots D needs --catalog-items M with 1 <= D < M")
    if args.catalog or args.dict_slots or args.item_lists:
        if args.kind not in ("f32", "f16"):
            raise SystemExit("--catalog needs --kind f32 or f16")
        return run_catalog(args)
    if args.pruned:
        if args.kind in ("training", "f8"):
            raise SystemExit("--pruned needs a format with a pruned layout (f32 or f16)")
        return run_pruned(args)
    if args.candidates:
        if args.kind in ("training", "f8"):  # (an f8 engine refuses score_candidates)
            raise SystemExit("--candidates needs a serving kind that scores candidates (f32 or f16)")
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
