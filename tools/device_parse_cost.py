#!/usr/bin/env python3
"""What the device text parser costs and what it buys (include/ffm_engine.h "Text blocks"; the numbers of
profiles/device_parse.md).

Three steps, a child process each under its own `timeout`, one after another; the first that fails ends the run
(nothing more is started on the GPU):
  parser    rows/s of ffm_textparse on chunks of a generated 39-field Zipf libffm text: from page-locked host memory
            with the two slots in flight (parse t + 1 issued before wait t), and from pageable memory (the parser's own
            copy first); five windows each, alternating
  hostparser  parse_csr_range through CsrStream on its own (`host_tests stream`, no device work) over the file of the
            prepass step, at 8 and 16 threads; five runs each, alternating, the page cache warm
  prepass   the trainer CLI's three counting pre-passes (`--bucket_fields 0-12 --min_count 3 --field_ranges counted
            --n_epochs 0`) over a file of that text, with and without `--device_parse true`, at --n_threads 8 and 16:
            seconds from the `in S s` of the passes' summary lines; five runs each, alternating, page cache warm
It needs a GPU and fails without one.  bench.py stays the project's yardstick; this tool only compares paths."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIELDS, FEATS = 39, 33_000_000
STEPS = ("parser", "hostparser", "prepass")
TAG = "DEVICE_PARSE_COST "


def make_text(rows):
    """`rows` rows of 39-field Zipf libffm text: 20 000 generated rows, repeated (the parser's work per byte does
    not depend on which ids repeat)."""
    from ftrl_ffm_amd import synth
    g = synth.Generator(N_FIELDS, FEATS, "zipf", seed=3)
    unit = synth.to_libffm_text(g.block(20000)).encode()
    reps = max(1, rows // 20000)
    return unit * reps, 20000 * reps


def step_parser(args):
    import numpy as np
    import ftrl_ffm_amd as fa
    text, rows = make_text(32768 * 2)
    unit_rows = 20000
    unit = text[:len(text) // (rows // unit_rows)]
    chunk = unit + unit[:len(unit) // 2 + unit[len(unit) // 2:].index(b"\n") + 1]  # about 30 000 rows, whole lines
    n_rows = fa.parse_text_host(chunk)["n_rows"]
    tp = fa.TextParser(has_field=True, max_bytes=len(chunk), max_rows=n_rows, max_nnz=n_rows * N_FIELDS)
    lib = fa.load_library()
    pinned = []
    for _ in range(2):
        a = fa.page_aligned(len(chunk), np.uint8)
        a[:] = np.frombuffer(chunk, np.uint8)
        assert lib.ffm_engine_pin_host(a.ctypes.data, a.nbytes) == 0
        pinned.append(a)

    def window(zero_copy, n):
        src = pinned if zero_copy else [chunk, chunk]
        t0 = time.perf_counter()
        tp.parse(src[0], slot=0, zero_copy=zero_copy)
        for t in range(n):
            if t + 1 < n:
                tp.parse(src[(t + 1) & 1], slot=(t + 1) & 1, zero_copy=zero_copy)
            blk = tp.wait(t & 1)
            assert blk["n_rows"] == n_rows and blk["n_slow"] == 0
        return n_rows * n / (time.perf_counter() - t0)

    window(True, 4)
    window(False, 4)
    out = {"pinned": [], "pageable": []}
    for _ in range(5):
        out["pinned"].append(window(True, args.chunks))
        out["pageable"].append(window(False, args.chunks))
    for a in pinned:
        lib.ffm_engine_unpin_host(a.ctypes.data)
    tp.close()
    print(TAG + json.dumps({"step": "parser", "chunk_rows": n_rows, "chunk_bytes": len(chunk), "chunks_per_window": args.chunks,
                            "rows_per_s": out}))


STREAM = re.compile(r"^pass 1: rows (\d+)  csr_stream (\d+) rows/s", re.M)


def step_hostparser(args):
    """parse_csr_range through CsrStream alone (`host_tests stream`: no device work), its second pass over the file
    (page cache warm), at 8 and 16 threads, five runs each, alternating."""
    import ftrl_ffm_amd as fa
    _, test_bin = fa.build_host()
    text, rows = make_text(args.rows)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "train.ffm")
        with open(path, "wb") as f:
            f.write(text)
        res = {}
        for _ in range(5):
            for threads in (8, 16):
                out = subprocess.run([test_bin, "stream", path, "libffm", str(threads)], cwd=tmp, capture_output=True, text=True)
                if out.returncode != 0:
                    raise SystemExit("device_parse_cost: host_tests stream ended with status %d: %s" % (out.returncode, out.stderr[-1000:]))
                got = STREAM.findall(out.stdout)
                assert len(got) == 1 and int(got[0][0]) == rows, out.stdout
                res.setdefault("%d threads" % threads, []).append(int(got[0][1]))
        print(TAG + json.dumps({"step": "hostparser", "rows": rows, "bytes": len(text), "rows_per_s": res}))


SECONDS = re.compile(r"^(value buckets|rare ids|field ranges): counted .* in ([0-9.]+) s", re.M)


def step_prepass(args):
    import ftrl_ffm_amd as fa
    main_bin, _ = fa.build_host()
    text, rows = make_text(args.rows)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "train.ffm")
        with open(path, "wb") as f:
            f.write(text)
        base = [main_bin, "--model_type", "FFM", "--n_fields", str(N_FIELDS), "--n_feats", str(FEATS), "--hash_feats", "true", "--bucket_fields",
                "0-12", "--min_count", "3", "--field_ranges", "counted", "--n_epochs", "0", "--train_data", path]
        res = {}
        for rep in range(5 + 1):  # (the first round warms the page cache and is dropped)
            for threads in (8, 16):
                for flag in (False, True):
                    cmd = base + ["--n_threads", str(threads)] + (["--device_parse", "true"] if flag else [])
                    t0 = time.perf_counter()
                    out = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
                    wall = time.perf_counter() - t0
                    if out.returncode != 0:
                        raise SystemExit("device_parse_cost: the CLI ended with status %d: %s" % (out.returncode, out.stderr[-1000:]))
                    secs = {k: float(v) for k, v in SECONDS.findall(out.stdout)}
                    assert len(secs) == 3, out.stdout
                    if rep:
                        res.setdefault("%d threads, %s" % (threads, "device" if flag else "host"), []).append(dict(secs, wall=wall))
        print(TAG + json.dumps({"step": "prepass", "rows": rows, "bytes": len(text), "runs": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--timeout", type=int, default=400)
    args = ap.parse_args()
    if args.step:
        return {"parser": step_parser, "hostparser": step_hostparser, "prepass": step_prepass}[args.step](args)
    for step in STEPS:
        rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                             "--rows", str(args.rows), "--chunks", str(args.chunks)]).returncode
        if rc != 0:
            raise SystemExit("device_parse_cost: step %s ended with status %d; nothing more is started" % (step, rc))


if __name__ == "__main__":
    main()
