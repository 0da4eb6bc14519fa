"""The `f8` serving format as numpy defines it (ftrl_ffm_amd.serve_f8_encode / serve_f8_decode; include/ffm_engine.h
"Serving engines"): checked against a brute-force nearest-value search in float64 over the 254 finite e4m3fn codes.
Nothing here has a tolerance, and nothing needs a GPU."""
import math
import subprocess

import numpy as np
import pytest

import ftrl_ffm_amd as fa

F32 = np.float32


def edge_rows(row_len, n_rows=64, seed=5):
    """float32 [n_rows, row_len]: the format's edge rows first, seeded normals at stddev 0.01 behind them."""
    up, dn = lambda x: np.nextafter(F32(x), F32(np.inf)), lambda x: np.nextafter(F32(x), F32(0))  # noqa: E731
    heads = []
    for t in (0, -20, 30):  # A = 448 * 2^t: ties at both parities (17 -> 16, 19 -> 20, and the subnormal 2^-10, 3 * 2^-10)
        heads.append([448.0 * 2.0 ** t] + [v * 2.0 ** t for v in (17, 19, -17, -19, 2.0 ** -10, 3 * 2.0 ** -10, -2.0 ** -10, 2.0 ** -11)])
        heads.append([up(448.0) * F32(2.0 ** t), 1.0 * 2.0 ** t, -3.0 * 2.0 ** t])  # just above 448: the s += 1 branch
        heads.append([dn(448.0) * F32(2.0 ** t), dn(F32(2.0 ** (t - 9))), up(F32(2.0 ** (t - 10)))])
    heads += [[1e-45, 2.0 ** -127, -2.0 ** -140], [dn(2.0 ** -126), 2.0 ** -130],          # A subnormal
              [3.4e38, -3.0e38, 1e30, 1.0], [2.0 ** 127, -2.0 ** 120], [dn(np.inf), 0.5],   # A near FLT_MAX
              [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.5, -0.25], [np.inf], [np.nan, -np.inf, 1e-3],
              [-0.0], [0.0, 0.0, 0.0, -0.0171]]                                             # zeros; one nonzero value
    with np.errstate(over="ignore"):
        w = (np.random.default_rng(seed).standard_normal((n_rows, row_len)) * 0.01).astype(F32)
    w[len(heads)] = 0.0                  # an all-zero row
    w[len(heads) + 1] = F32(np.inf)      # no finite element at all
    for r, h in enumerate(heads):
        w[r] = 0.0
        w[r, :len(h)] = np.asarray(h, F32)[:row_len]
    return w


def brute(w):
    """(bytes, scales) by search: the nearest finite code of the element's sign in float64, a tie to the even code."""
    val = fa.SERVE_F8_VALUE.astype(np.float64)
    assert [val[c] for c in (0x01, 0x08, 0x09, 0x7e, 0x80, 0xfe)] == [2.0 ** -9, 2.0 ** -6, 9 * 2.0 ** -9, 448.0, 0.0, -448.0]
    assert np.isnan(val[0x7f]) and np.isnan(val[0xff]) and np.signbit(val[0x80]) and np.isfinite(val).sum() == 254
    q, scales = np.zeros(w.shape, np.uint8), np.ones(w.shape[0], F32)
    for r, row in enumerate(w.astype(np.float64)):
        fin = np.isfinite(row)
        a = float(np.abs(row[fin]).max()) if fin.any() else 0.0
        s = 0
        if a > 0:
            s = min(max(math.frexp(a)[1] - 1 - 8, -117), 119)
            s += 1 if a * 2.0 ** -s > 448 else 0
        scales[r] = F32(2.0 ** s)
        for j, x in enumerate(row):
            sign = 128 if np.signbit(x) else 0
            if not np.isfinite(x):
                q[r, j] = 127 | sign
                continue
            d = np.abs(val[sign:sign + 127] - x * 2.0 ** -s)
            best = np.flatnonzero(d == d.min())
            q[r, j] = sign + (best[0] if best.size == 1 else best[best % 2 == 0][0])
    return q, scales


@pytest.mark.parametrize("row_len", [12, 16, 624])
def test_encode_and_decode_match_the_search(row_len):
    w = edge_rows(row_len, n_rows=64 if row_len < 100 else 36)
    q, scales = fa.serve_f8_encode(w)
    want_q, want_s = brute(w)
    assert q.dtype == np.uint8 and q.shape == (w.shape[0], (row_len + 15) // 16 * 16) and not q[:, row_len:].any()
    assert np.array_equal(scales.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(q[:, :row_len], want_q), np.argwhere(q[:, :row_len] != want_q)[:4]
    exps = np.log2(scales.astype(np.float64))
    assert (exps == np.round(exps)).all() and exps.min() == -117 and exps.max() == 120
    assert fa.serve_f8_stride(row_len) == 16 + q.shape[1]
    # decoding: fl(value * scale) in fp32, exact below the overflow; the NaN byte is NaN; no decoded value is subnormal
    d = fa.serve_f8_decode(q, scales, row_len)
    with np.errstate(all="ignore"):
        want_d = (fa.SERVE_F8_VALUE.astype(np.float64)[want_q] * want_s.astype(np.float64)[:, None]).astype(F32)
    assert np.array_equal(np.isnan(d), ~np.isfinite(w)) and np.array_equal(d.view(np.uint32)[~np.isnan(d)], want_d.view(np.uint32)[~np.isnan(d)])
    assert not ((d != 0) & (np.abs(d) < F32(2.0 ** -126))).any()
    assert np.isinf(d).sum() == 2  # 3.4e38 and the largest float: only within a factor of two of FLT_MAX


@pytest.mark.parametrize("flags", [["--publish_path", "P", "--publish_weights", "f8", "--n_epochs", "1"],
                                   ["--apply_deltas", "P", "--serve_weights", "f8", "--n_epochs", "0"]])
def test_the_cli_refuses_f8_deltas_before_it_opens_a_device(tmp_path, flags):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin, "--model_type", "FFM", "--train_data", "none.txt"] + flags, cwd=tmp_path, capture_output=True, text=True)
    assert out.returncode != 0 and "f8" in out.stdout + out.stderr and "serving deltas" in out.stdout + out.stderr, out
