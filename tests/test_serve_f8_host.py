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


# ---- scales that differ, and the extremes (the GPU side: tests/test_gpu_serve_f8.py::test_rows_of_mixed_scales) ------
# F = 6 fields of SCALE_PER ids each; feature i belongs to field i // SCALE_PER.  The first ids of the LAST field are the
# extreme features, one edge_rows row each; every other feature is a varied one: N(0, 1) * 2^m(i), m(i) uniform in
# SCALE_M per feature.  With m <= 20 a pair term stays below 2^45 * k and a logit below 2^60: the varied rows are finite
# by construction (checked below), so a kernel cannot pass on NaN == NaN.
SCALE_F, SCALE_PER, SCALE_M, SCALE_KS = 6, 64, (-40, 20), (4, 16, 64)
SCALE_NF = SCALE_F * SCALE_PER
# name -> (the edge_rows row it carries, the scale numpy gives it, the class of the named row's oracle logit)
EXTREMES = {
    "scale 2^-117, one value left": (10, 2.0 ** -117, "finite"),
    "scale 2^-117, all rounded to zero": (9, 2.0 ** -117, "finite"),
    "scale 2^120": (11, 2.0 ** 120, "inf"),       # 3.4e38 decodes to 256 * 2^120: the one infinity of the row
    "zeros, +-inf, +-NaN": (14, 2.0 ** -9, "nan"),
    "+inf alone": (15, 1.0, "nan"),
    "NaN, -inf, 1e-3": (16, 2.0 ** -18, "nan"),
    "-0.0 alone": (17, 1.0, "finite"),
    "one nonzero value": (18, 2.0 ** -14, "finite"),
    "all zero": (19, 1.0, "finite"),
    "no finite element": (20, 1.0, "nan"),
}


def scale_case(k, seed=71, n_varied_rows=56):
    """dict(w [SCALE_NF, 6 k], lin_w, bias, block, extreme_ids {name: id}, named {name: row index}, varied_rows): the
    table and block of the mixed-scale case at k factors.  The block's first n_varied_rows rows (1 .. 40 entries, any
    field, ids of varied features only) are followed by one named row per extreme feature: a varied entry in each of
    the fields 0 .. 4 and the extreme feature in field 5, so that its slots 0 .. 4 -- elements 0 .. 5 k - 1, every value
    an edge_rows row holds -- are read and nothing else of the row is extreme."""
    from oracle.pyoracle import Csr
    rng = np.random.default_rng(seed + k)
    L = SCALE_F * k
    m = rng.integers(SCALE_M[0], SCALE_M[1] + 1, SCALE_NF)
    w = (rng.standard_normal((SCALE_NF, L)) * 2.0 ** m[:, None]).astype(F32)
    edge = edge_rows(L, n_rows=32)
    first = (SCALE_F - 1) * SCALE_PER
    extreme_ids = {name: first + j for j, name in enumerate(EXTREMES)}
    for name, i in extreme_ids.items():
        w[i] = edge[EXTREMES[name][0]]
    varied = np.setdiff1d(np.arange(SCALE_NF), list(extreme_ids.values()))
    rows = []
    for r in range(n_varied_rows):
        ids = rng.choice(varied, int(rng.integers(1, 41)), replace=False)
        rows.append([(int(i) // SCALE_PER, int(i), 1.0 if rng.random() < 0.5 else float(F32(rng.random() + 0.25))) for i in ids])
    named = {}
    for name, i in extreme_ids.items():
        named[name] = len(rows)
        row = [(f, int(rng.choice(varied[varied // SCALE_PER == f])), float(F32(rng.random() + 0.25))) for f in range(SCALE_F - 1)]
        rows.append(row + [(SCALE_F - 1, i, 1.0)])
    block = Csr.from_rows(rows, [r % 2 for r in range(len(rows))])
    return dict(w=w, m=m, lin_w=rng.normal(0, 0.02, SCALE_NF).astype(F32), bias=F32(0.013), block=block,
                extreme_ids=extreme_ids, named=named, varied_rows=np.arange(n_varied_rows))


def scale_oracle(c, k):
    """The oracle holding the decoded table of scale_case(k), and that table."""
    from oracle.pyoracle import CpuModel
    from util import STRESS_HP
    d = fa.serve_f8_decode(*fa.serve_f8_encode(c["w"]), row_len=SCALE_F * k)
    o = CpuModel("oracle", "FFM", SCALE_NF, SCALE_F, k, **STRESS_HP)
    st = o.zero_state()
    st["bias3"][0], st["lin_w"][...], st["vec_w"][...] = c["bias"], c["lin_w"], d
    o.set_state(st)
    return o, d


def logit_class(x):
    return "nan" if np.isnan(x) else "inf" if np.isinf(x) else "finite"


@pytest.mark.parametrize("k", SCALE_KS)
def test_mixed_scale_case_cannot_pass_on_nan_alone(k):
    """What tests/test_gpu_serve_f8.py::test_rows_of_mixed_scales takes for granted, on the oracle alone: no decoded
    value is subnormal, at most 1 varied row in 8 has a non-finite logit (here: none), every named row has its class,
    the extreme features carry the scales they are named for, and a varied row mixes scales dozens of binades apart."""
    c = scale_case(k)
    o, d = scale_oracle(c, k)
    assert not ((d != 0) & (np.abs(d) < F32(2.0 ** -126))).any(), "a decoded value is subnormal"
    scales = fa.serve_f8_encode(c["w"])[1]
    for name, i in c["extreme_ids"].items():
        assert scales[i] == F32(EXTREMES[name][1]), (name, scales[i])
    assert np.isinf(d[c["extreme_ids"]["scale 2^120"]]).sum() == 1 and (d[c["extreme_ids"]["scale 2^-117, one value left"]] != 0).sum() == 1
    blk = c["block"]
    assert not np.isin(take_feats(blk, c["varied_rows"]), list(c["extreme_ids"].values())).any()
    lg = o.predict_batch(blk)[0]
    assert (~np.isfinite(lg[c["varied_rows"]])).mean() <= 1 / 8
    for name, r in c["named"].items():
        feats = blk.feat[blk.row_ptr[r]:blk.row_ptr[r + 1]]
        assert np.isin(feats, list(c["extreme_ids"].values())).sum() == 1 and feats[-1] == c["extreme_ids"][name]
        assert logit_class(lg[r]) == EXTREMES[name][2], (name, lg[r])
    # the scale exponents within a row: dozens of binades apart in most rows of more than a few entries
    exps = np.log2(scales.astype(np.float64))
    spread = [np.ptp(exps[blk.feat[blk.row_ptr[r]:blk.row_ptr[r + 1]]]) for r in c["varied_rows"] if blk.row_ptr[r + 1] - blk.row_ptr[r] >= 6]
    assert len(spread) >= 30 and np.median(spread) >= 36 and exps.min() == -117 and exps.max() == 120


def take_feats(blk, rows):
    return np.concatenate([blk.feat[blk.row_ptr[r]:blk.row_ptr[r + 1]] for r in rows])


@pytest.mark.parametrize("flags", [["--publish_path", "P", "--publish_weights", "f8", "--n_epochs", "1"],
                                   ["--apply_deltas", "P", "--serve_weights", "f8", "--n_epochs", "0"]])
def test_the_cli_refuses_f8_deltas_before_it_opens_a_device(tmp_path, flags):
    main_bin, _ = fa.build_host()
    out = subprocess.run([main_bin, "--model_type", "FFM", "--train_data", "none.txt"] + flags, cwd=tmp_path, capture_output=True, text=True)
    assert out.returncode != 0 and "f8" in out.stdout + out.stderr and "serving deltas" in out.stdout + out.stderr, out
