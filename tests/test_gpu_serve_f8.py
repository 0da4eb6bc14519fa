"""`f8` serving engines (include/ffm_engine.h "Serving engines"; csrc/kernels_serve8.h): the encoder against numpy's
definition of the format (ftrl_ffm_amd.serve_f8_encode / _decode), and the row kernel against an fp32 serving engine
that holds the decoded table -- the same fp32 arithmetic in the same order, so every comparison is bit for bit (NaN
with NaN: util.assert_bitwise).  The two row kernels share their staging, pair order and ordered sum, so the row kernel
is also compared with the oracle (oracle.pyoracle.CpuModel holding test_gpu_serve.decoded(w, "f8")): on the ladder of
row lengths with the pair counts at which its lane shape changes trip count, on every row cap, on signed zeros, and on
tables whose rows differ in scale by dozens of binades or sit at the format's extremes; and the encoder, the decoder and
the whole-table transfers run past their first grid-stride trip and their first staging chunk.  Nothing has a
tolerance."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import Csr
from test_gpu_serve import NF as LADDER_NF
from test_gpu_serve import LENGTHS, check_predict, decoded, ladder_weights, oracle_with, serving
from test_serve_f8_host import EXTREMES, SCALE_F, SCALE_KS, SCALE_NF, edge_rows, logit_class, scale_case, scale_oracle
from util import (ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, row_cap_prefixes, row_length_block,
                  take_rows)

pytestmark = pytest.mark.gpu
NF = 64


def engine(F, k, serve=None, **kw):
    return fa.Engine("FFM", NF, F, k, serve=serve, max_batch_rows=16, max_batch_nnz=4096, **dict(STRESS_HP, **kw))


def counted(w, d):
    nan = np.isnan(w)
    return dict(n_latent=w.size, n_inexact=int((~nan & (w.view(np.uint32) != d.view(np.uint32))).sum()),
                n_to_inf=int((np.isfinite(w) & ~np.isfinite(d)).sum()), n_to_zero=int((~nan & (w != 0) & (d == 0)).sum()))


# F x k: row lengths 12 .. 2496 (both lane groups, rows that stay in registers and rows read twice, a last chunk with
# padding) and the group's boundaries: 256 = the last length of the 16-lane group (every lane owns a chunk), 272 = the
# first of the 64-lane group, 1024 = the last a 64-lane group keeps wholly in registers, 1040 = the first read twice
ENCODER_SHAPES = [(F, k) for F in (3, 39) for k in (4, 16, 64)] + [(16, 16), (17, 16), (16, 64), (65, 16)]


@pytest.mark.parametrize("F,k", ENCODER_SHAPES)
def test_encoder_is_the_numpy_definition(F, k):
    """pack_from, set_rows and the create-time contents."""
    w = edge_rows(F * k, NF)
    want = fa.serve_f8_decode(*fa.serve_f8_encode(w), row_len=F * k)
    t = engine(F, k, skip_init=True)
    t.set_weights(bias=[0.25], lin_w=np.arange(NF, dtype=np.float32), vec_w=w)
    s = engine(F, k, "f8", skip_init=True)
    ids = np.arange(NF, dtype=np.int32)
    assert not s.get_rows(ids)["vec_w"].any() and s.model_bytes() == 4 + 4 * NF + NF * fa.serve_f8_stride(F * k)
    assert s.pack_from(t) == counted(w, want)
    got = s.get_weights()
    assert_bitwise(got["vec_w"], want, "pack_from")
    assert got["bias"][0] == 0.25 and np.array_equal(got["lin_w"], np.arange(NF))
    some = ids[::-3].copy()  # set_rows: whole rows, each scale from the values given
    s.set_rows(some, dict(vec_w=w[some][:, ::-1].copy()))
    want[some] = fa.serve_f8_decode(*fa.serve_f8_encode(w[some][:, ::-1]), row_len=F * k)
    assert_bitwise(s.get_rows(ids)["vec_w"], want, "set_rows")
    assert s.encode_stats() == counted(w[some][:, ::-1], want[some])
    fresh_t, fresh_s = engine(F, k, seed=9), engine(F, k, "f8", seed=9)
    draws = fresh_t.get_weights()["vec_w"]
    assert_bitwise(fresh_s.get_weights()["vec_w"], fa.serve_f8_decode(*fa.serve_f8_encode(draws), row_len=F * k), "create")
    for e in (t, s, fresh_t, fresh_s):
        e.close()


def block(F, lengths, seed):
    """Rows of the given lengths over ids -2 .. NF + 1 and fields -1 .. F: out of range both ways, fields twice."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    return Csr(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), rng.integers(-1, F + 1, n).astype(np.int32),
               rng.integers(-2, NF + 2, n).astype(np.int32), rng.standard_normal(n).astype(np.float32),
               rng.integers(0, 2, len(lengths)).astype(np.int32))


def pair(F, k):
    """An f8 engine of seeded rows (feature 5 holds the NaN byte) and the fp32 serving engine of its decoded table."""
    w = (np.random.default_rng(k * 100 + F).standard_normal((NF, F * k)) * 0.3).astype(np.float32)
    w[5, F * k // 2] = np.nan
    s8, s32 = engine(F, k, "f8", skip_init=True), engine(F, k, "f32", skip_init=True)
    s8.set_weights(bias=[0.1], lin_w=np.linspace(-1, 1, NF).astype(np.float32), vec_w=w)
    s32.set_weights(**s8.get_weights())
    return s8, s32


def on_device(e, b):
    d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
    out = torch.full((b.n_rows,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.predict_batch_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                           d["val"].data_ptr(), d["label"].data_ptr(), True, out.data_ptr(), None)
    try:
        e.sync()
    except fa.EngineError as err:
        return out.cpu().numpy(), err.code
    return out.cpu().numpy(), 0


@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("F", [3, 39, 64])
def test_rows_are_the_fp32_kernel_on_the_decoded_table(F, k):
    """The 129-entry row goes through predict_batch_device: predict_batch refuses it on the host (FFM_E_CAPACITY) before
    anything is queued, so only a device block reaches the kernel's own refusal."""
    s8, s32 = pair(F, k)
    blk = block(F, [0, 1, 2, 39, 64, 65, 128, 2], seed=F + k)
    blk.field[-2:], blk.feat[-2:] = [0, F // 2], [5, 6]  # the last row reads the slot that holds the NaN byte
    for prob in (False, True):
        a, b = s8.predict_batch(blk, output_prob=prob), s32.predict_batch(blk, output_prob=prob)
        assert_bitwise(a[0], b[0], "F=%d k=%d prob=%d" % (F, k, prob))
        assert a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1]))
    assert np.isnan(a[0][-1]) and np.isfinite(a[0][:3]).all()
    (o8, c8), (o32, c32) = (on_device(e, block(F, [5, 129, 2], seed=k)) for e in (s8, s32))
    assert c8 == c32 == fa.engine.E_CAPACITY and np.isnan(o8[1]) and np.isnan(o32[1])
    assert_bitwise(o8, o32, "beside a row of 129 entries")
    s8.close()
    s32.close()


def test_entry_points_give_predict_batch_bits():
    s8, s32 = pair(39, 16)
    blk = block(39, [7, 0, 128, 39, 40], seed=1)
    want = s8.predict_batch(blk, output_prob=True)[0]
    out, code = on_device(s8, blk)
    assert code == 0
    assert_bitwise(out, want, "predict_batch_device")
    buf = s8.score_buffer(blk.n_rows)
    cutter = fa.RowCutter(blk.n_rows, int(blk.row_ptr[-1]), n_blocks=2)
    cutter.take_host(blk.n_rows, blk.row_ptr, blk.field, blk.feat, blk.val, blk.label)
    res = cutter.close()
    for what, call in (("predict_batch_async", lambda: s8.predict_batch_async(blk, scores=buf, output_prob=True)),
                       ("predict_async_resident", lambda: s8.predict_async_resident(res, scores=buf, output_prob=True))):
        buf[:] = np.float32(-7.0)
        call()
        s8.train_flush()
        assert_bitwise(buf[:blk.n_rows].copy(), want, what)
    s8.free_score_buffer(buf)
    cutter.release(res)
    cutter.destroy()
    s8.close()
    s32.close()


REFUSED = {
    "score_candidates": lambda e, t, b: e.score_candidates(take_rows(b, [0]), np.array([0, 1], np.int32), take_rows(b, [1])),
    "set_pair_mask": lambda e, t, b: e.set_pair_mask(fa.pair_mask(3, [(0, 1)])),
    "ablation": lambda e, t, b: e.ablation_enable(),
    "predict_ablated": lambda e, t, b: e.predict_ablated(b),
    "pair_ablation": lambda e, t, b: e.pair_ablation_enable(),
    "predict_pair_ablated": lambda e, t, b: e.predict_pair_ablated(b),
    "pair_curve": lambda e, t, b: e.pair_curve_enable(fa.pair_curve_levels(3, list(range(6))), [1]),
    "predict_pair_curve": lambda e, t, b: (setattr(e, "_curve_variants", 2), e.predict_pair_curve(b)),
    "sync_from": lambda e, t, b: e.sync_from(t),
    "get_rows_raw": lambda e, t, b: e.get_rows_raw([1, 2]),
    "set_rows_raw": lambda e, t, b: e.set_rows_raw([1], lat=np.zeros((1, 12), np.float32)),
    "export_delta": lambda e, t, b: e.export_delta(),
    "apply_delta": lambda e, t, b: e.apply_delta(dict(fmt="f8", ids=[1], bias=[0], lin_w=[0], lat=np.zeros((1, 12), np.uint8))),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_on_an_f8_engine(name):
    t, s = engine(3, 4), engine(3, 4, "f8")
    before = s.get_weights()
    with pytest.raises(fa.EngineError) as err:
        REFUSED[name](s, t, block(3, [3, 2], seed=3))
    assert err.value.code == fa.engine.E_UNSUPPORTED and "f8" in str(err.value), str(err.value)
    after = s.get_weights()
    assert all(np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)) for key in before)
    t.close()
    s.close()


# ---- the row kernel against the oracle (oracle.pyoracle.CpuModel on test_gpu_serve.decoded(w, "f8")) ------------------
# ffm_row8_wave_kernel shares its staging, pair order and ordered sum with ffm_row_wave_kernel, so the comparisons above
# cannot see a mistake the two have in common, and what is its own -- a pair per lane (2 / 4 lanes per pair at k = 32 /
# 64), 64 / 32 / 16 pairs per step, kPredTerms = 256 pairs per trip of the unrolled loop, the tail around ok[u] and
# cur.advance -- changes trip count at 16, 32, 64, 256 and 512 pairs: rows of 6 / 7, 8 / 9, 11 / 12, 23 / 24 and 32 / 33
# SURVIVING entries (15 / 21, 28 / 36, 55 / 66, 253 / 276, 496 / 528 pairs).

LADDER8_LENGTHS = tuple(sorted(set(LENGTHS) | {6, 7, 9, 23, 24}))
PAIR_EDGES = (6, 7, 8, 9, 11, 12, 23, 24, 32, 33)
KS = (4, 8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def ladder8_block(seed=3):
    blk, nf = row_length_block("FFM", ROW_FIELDS, ROW_IDS_PER_FIELD, seed, lengths=LADDER8_LENGTHS)
    assert nf == LADDER_NF and blk.n_rows % 4 != 0 and int(np.diff(blk.row_ptr).max()) == 128
    return blk


def surviving(blk, n_feats, n_fields):
    """Per row: the entries whose id and field are in range (what wave_stage_entries keeps)."""
    ok = (blk.feat >= 0) & (blk.feat < n_feats) & (blk.field >= 0) & (blk.field < n_fields)
    return np.add.reduceat(np.concatenate([ok, [False]]).astype(np.int64), blk.row_ptr[:-1].astype(np.int64)) * (np.diff(blk.row_ptr) > 0)


def ladder8(k):
    """(f8 engine, oracle on the decoded table) of test_gpu_serve's ladder model at k factors."""
    st = ladder_weights(k)
    return serving(k, "f8", st), oracle_with(k, st["bias3"][0], st["lin_w"], decoded(st["vec_w"], "f8", ROW_FIELDS * k))


@pytest.mark.parametrize("k", KS)
def test_parity_ladder(k):
    """test_gpu_serve.test_parity_ladder for the f8 engine, on a block that adds rows of 6, 7, 9, 23 and 24 entries."""
    blk = ladder8_block()
    alive = surviving(blk, LADDER_NF, ROW_FIELDS)
    assert (alive <= np.diff(blk.row_ptr)).all() and (alive < np.diff(blk.row_ptr)).any()
    assert set(PAIR_EDGES) <= set(alive.tolist()), sorted(set(PAIR_EDGES) - set(alive.tolist()))
    e, o = ladder8(k)
    check_predict(e, o, blk, "k=%d f8 ladder" % k)
    lens = np.diff(blk.row_ptr)
    longest = int(np.argmax(lens))
    check_predict(e, o, take_rows(blk, [longest]), "k=%d f8 one row of %d" % (k, lens[longest]))
    five = [int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33)]
    check_predict(e, o, take_rows(blk, five), "k=%d f8 five rows" % k)
    e.close()


@pytest.mark.parametrize("k", [4, 16, 64])
def test_every_row_cap_from_host_memory(k):
    """Blocks whose longest row is 1, 3, 5, 64, 65 and 128 entries, from host memory: predict_batch sizes the launch by
    the longest row, so lds_cap takes those values and wave_lds places the second to fourth wave's entries and terms
    accordingly (every piece has at least four rows: all four waves of a workgroup are live)."""
    e, o = ladder8(k)
    caps = (1, 3, 5, 64, 65, 128)
    pieces = list(row_cap_prefixes(ladder8_block(), caps))
    assert [int(np.diff(p.row_ptr).max()) for p in pieces] == list(caps) and min(p.n_rows for p in pieces) >= 4
    for piece in pieces:
        assert (np.diff(piece.row_ptr) > 0).sum() >= 3
        check_predict(e, o, piece, "k=%d f8 piece with row cap %d" % (k, np.diff(piece.row_ptr).max()))
    e.close()


@pytest.mark.parametrize("sign", [-0.0, 0.0], ids=["minus", "plus"])
@pytest.mark.parametrize("k", [4, 16, 64])
def test_predict_keeps_the_sign_of_a_zero_logit(k, sign):
    """test_gpu_row_lengths.test_predict_keeps_the_sign_of_a_zero_logit on an all-zero f8 table (zero bytes behind scale
    1.0: every decoded value is +0.0): two survivors per row, one value of each sign, lin_w = -0.0 under the positive
    value and +0.0 under the negative one, so every linear product and the only pair term are -0.0.  With the bias -0.0
    every logit is -0.0 -- one +0.0 padded into an ordered sum would turn it -- and with +0.0 it is +0.0."""
    per = ROW_IDS_PER_FIELD
    rows = []
    for n in LENGTHS:
        for keep in ((0, n - 1), (63, 64)):
            if n < 2 or keep[1] >= n:
                continue
            r = len(rows)
            row = [((j % ROW_FIELDS, -7, 1.0), (j % ROW_FIELDS, LADDER_NF + 3, 0.5), (ROW_FIELDS + 2, j, 1.0))[j % 3] for j in range(n)]
            row[keep[0]], row[keep[1]] = (0, r, 0.75), (1, per + r, -0.5)
            rows.append(row)
    blk = Csr.from_rows(rows, [r % 2 for r in range(len(rows))])
    assert (surviving(blk, LADDER_NF, ROW_FIELDS) == 2).all() and blk.n_rows % 4 != 0
    lin = np.zeros(LADDER_NF, np.float32)
    lin[:per] = -0.0
    o = oracle_with(k, np.float32(sign), lin, np.zeros((LADDER_NF, ROW_FIELDS * k), np.float32))
    po = o.predict_batch(blk)[0]
    assert (po == 0).all() and (np.signbit(po) == np.signbit(np.float32(sign))).all(), "the oracle's logits are all %r" % sign
    e = serving(k, "f8")
    e.set_weights(bias=np.float32([sign]), lin_w=lin)
    assert not e.get_rows(np.arange(64, dtype=np.int32))["vec_w"].view(np.uint32).any()
    check_predict(e, o, blk, "k=%d f8 signed zeros, bias %r" % (k, sign))
    e.close()


# ---- scales that differ, and the extremes (the case and its CPU conditions: tests/test_serve_f8_host.py) --------------

@pytest.mark.parametrize("k", SCALE_KS)
def test_rows_of_mixed_scales(k):
    """Rows that mix features whose scales lie dozens of binades apart, and rows that hold one feature at an edge of the
    format (scale 2^-117, scale 2^120, the NaN byte, infinities, zero rows): the decode is one exact multiply and no
    product is subnormal, so the oracle on the decoded table is the expected output bit for bit.  It cannot pass on NaN
    == NaN: the varied rows are finite (at most 1 in 8 may not be) and every named row has the class the host file
    names."""
    c = scale_case(k)
    o, d = scale_oracle(c, k)
    assert not ((d != 0) & (np.abs(d) < np.float32(2.0 ** -126))).any(), "a decoded value is subnormal"
    e = fa.Engine("FFM", SCALE_NF, SCALE_F, k, serve="f8", skip_init=True, max_batch_rows=128, **STRESS_HP)
    e.set_weights(bias=[c["bias"]], lin_w=c["lin_w"], vec_w=c["w"])
    assert_bitwise(e.get_weights()["vec_w"], d, "the table decoded on the device")
    blk = c["block"]
    check_predict(e, o, blk, "k=%d mixed scales" % k)
    check_predict(e, o, take_rows(blk, c["varied_rows"]), "k=%d mixed scales, varied rows alone (a finite loss sum)" % k)
    for prob in (False, True):
        got = e.predict_batch(blk, output_prob=prob)[0]
        assert np.isfinite(got[c["varied_rows"]]).mean() >= 7 / 8
        for name, r in c["named"].items():
            want = EXTREMES[name][2] if not prob or EXTREMES[name][2] == "nan" else "finite"  # (a sigmoid of +-inf is 0 or 1)
            assert logit_class(got[r]) == want, (name, prob, got[r])
    e.close()


# ---- the encoder's, the decoder's and the transfer's loops past their first trip --------------------------------------
# serve8_grid caps at 2048 workgroups of 256 threads: 32 768 rows per trip of a 16-lane group, 8192 of a 64-lane group
# (serve_pack8_kernel: 8 x CUs workgroups, fewer still); serve8_decode_kernel runs 1024 x 256 threads; serve_vec_transfer
# moves 16 Mi floats per chunk.  F = 3, k = 4 at 40 000 features: two trips of the 16-lane group.  F = 39, k = 16 at 27 000:
# two chunks (26 886 rows, four trips of the 64-lane group, and 114 rows with f0 > 0), 4.2 M vectors on 262 144 threads.

def planted(row_len, n_feats, n_edge=32):
    """edge_rows with a copy of its first rows (every edge row of the format, a few seeded ones) at the END of the table
    too, where the last trip and the second chunk meet them."""
    w = edge_rows(row_len, n_rows=n_feats)
    w[-n_edge:] = w[:n_edge]
    return w


def f8_rows(w):
    return fa.serve_f8_decode(*fa.serve_f8_encode(w), row_len=w.shape[1])


@pytest.mark.parametrize("F,k,n_feats,n_ids", [(3, 4, 40000, 36000), (39, 16, 27000, 9000)])
def test_encoder_and_decoder_past_their_first_trip(F, k, n_feats, n_ids):
    """set_weights / get_weights, set_rows / get_rows on an id list longer than one trip, encode_stats and pack_from
    against numpy over the WHOLE table: a counter reset or counted twice between trips, a row skipped or written by two
    groups, a chunk placed at the wrong feature all show."""
    L = F * k
    assert n_feats > (32768 if L <= 256 else 8192) and n_ids > (32768 if L <= 256 else 8192)
    assert L > 256 or n_feats * L < (16 << 20)  # (the small case is one chunk: two trips alone)
    assert L <= 256 or (16 << 20) // L < n_feats  # (the large one: a second chunk)
    w = planted(L, n_feats)
    want = f8_rows(w)
    lin = np.arange(n_feats, dtype=np.float32)
    kw = dict(max_batch_rows=16, max_batch_nnz=4096, skip_init=True, **STRESS_HP)
    s = fa.Engine("FFM", n_feats, F, k, serve="f8", **kw)
    s.set_weights(bias=[0.25], lin_w=lin, vec_w=w)
    assert s.encode_stats(reset=True) == counted(w, want)
    assert_bitwise(s.get_weights()["vec_w"], want, "set_weights -> get_weights")
    # an id list with ids outside the table is refused whole, before anything is written
    bad = np.arange(64, dtype=np.int32)
    bad[1::2] = [-1, n_feats] * 16
    with pytest.raises(fa.EngineError) as err:
        s.set_rows(bad, dict(vec_w=np.ones((64, L), np.float32)))
    assert err.value.code == fa.engine.E_INVALID
    assert s.encode_stats() == dict(n_latent=0, n_inexact=0, n_to_inf=0, n_to_zero=0)
    # a strided id list longer than one trip: every row reversed (the same scale, other bytes)
    ids = (np.arange(n_ids, dtype=np.int64) * 7 % n_feats).astype(np.int32)
    assert np.unique(ids).size == n_ids and ids.max() >= n_feats - 8
    rows = w[ids][:, ::-1].copy()
    s.set_rows(ids, dict(vec_w=rows))
    after = want.copy()
    after[ids] = f8_rows(rows)
    assert s.encode_stats(reset=True) == counted(rows, after[ids])
    everything = np.arange(n_feats, dtype=np.int32)
    got = s.get_rows(everything)
    assert_bitwise(got["vec_w"], after, "set_rows -> get_rows of every feature")
    assert np.array_equal(got["lin_w"], lin)
    assert_bitwise(s.get_rows(ids[::-1])["vec_w"], after[ids[::-1]], "get_rows on the strided list, backwards")
    # pack_from a training engine that holds the table (set_weights: no training)
    t = fa.Engine("FFM", n_feats, F, k, **kw)
    t.set_weights(bias=[-0.5], lin_w=lin[::-1], vec_w=w)
    assert s.pack_from(t) == counted(w, want)
    got = s.get_weights()
    assert_bitwise(got["vec_w"], want, "pack_from -> get_weights")
    assert got["bias"][0] == -0.5 and np.array_equal(got["lin_w"], lin[::-1])
    t.close()
    s.close()
