"""Pair masks (include/ffm_engine.h "Pair masks"; csrc/kernels_mask.h, csrc/engine_mask.h): prediction with the
kept field pairs only.

Three yardsticks, all of them older than the masked kernel: the same engine's unmasked predict_batch (all pairs
kept), the same engine's predict_pair_ablated (exactly one pair dropped: this holds on any block), and
predict_batch on weights whose slot "towards field g" is +0.0 for field f's ids for every dropped pair -- on
oracle.pyoracle.CpuModel or on a twin engine (ftrl_ffm_amd.drop_pair_weights, applied per pair; the argument and its
two conditions are those of tests/test_pair_ablation_host.py, and the tests here assert the conditions).  Logits and
probabilities bit for bit (NaN with NaN), double loss sums by util.loss_close.  Nothing else has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_pair_weights, pair_count, pair_fields, pair_index, pair_mask, pair_mask_pairs
from oracle.pyoracle import CpuModel, Csr
from test_gpu_field_ablation import engine_of, lanes_block, numpy_histogram, training
from test_gpu_pair_ablation import LADDER_SUBSETS, device_arrays, ladder_sub, one_field_per_id
from test_gpu_serve import NF, decoded, ladder_block, ladder_weights, own_pages, serving
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, assert_state_bitwise, loss_close, rand_state, take_rows

pytestmark = pytest.mark.gpu

KINDS = ("train", "f32", "f16")  # a training engine, the two serving formats
E_INVALID, E_CAPACITY, E_UNSUPPORTED = fa.engine.E_INVALID, fa.engine.E_CAPACITY, fa.engine.E_UNSUPPORTED
V6 = 21  # the pairs of the ladder's 6 fields


def all_pairs(F):
    return [(f, g) for f in range(F) for g in range(f, F)]


def seeded_pairs(F, seed, density):
    """A fixed-seed subset of the V pairs, the diagonal included, each kept with probability `density`."""
    keep = np.random.default_rng(seed).random(pair_count(F)) < density
    return [p for p, kp in zip(all_pairs(F), keep) if kp]


def masked_weights(vec_w, F, per, kept):
    """vec_w [n_feats, F * k] with, for every pair (f, g) that `kept` lacks, the slot towards g zeroed for field f's ids
    and the slot towards f for field g's (ids of field f: [f * per, (f + 1) * per))."""
    w3 = np.array(vec_w, np.float32).reshape(vec_w.shape[0], F, -1)
    kept = set(kept)
    for f, g in all_pairs(F):
        if (f, g) not in kept:
            w3 = drop_pair_weights(w3, np.arange(f * per, (f + 1) * per), g)
            w3 = drop_pair_weights(w3, np.arange(g * per, (g + 1) * per), f)
    return w3.reshape(vec_w.shape)


def pairs_present(blk, F):
    """The field pairs (f <= g) that some row of the block holds among the entries the model keeps."""
    seen = set()
    for r in range(blk.n_rows):
        lo, hi = int(blk.row_ptr[r]), int(blk.row_ptr[r + 1])
        fl, ft = blk.field[lo:hi], blk.feat[lo:hi]
        fl = fl[(fl >= 0) & (fl < F) & (ft >= 0)]
        cnt = np.bincount(fl, minlength=F)
        for f in np.flatnonzero(cnt):
            for g in np.flatnonzero(cnt):
                if f < g or (f == g and cnt[f] > 1):
                    seen.add((int(f), int(g)))
    return seen


def outputs(e, blk):
    lg, ls = e.predict_batch(blk)
    return lg, e.predict_batch(blk, output_prob=True)[0], ls


def check(e, blk, want, what):
    got = outputs(e, blk)
    assert_rows_bitwise(got[0], want[0], blk, what + " logits")
    assert_rows_bitwise(got[1], want[1], blk, what + " probabilities")
    assert loss_close(got[2], want[2]), "%s: loss sum %r vs %r" % (what, got[2], want[2])


# ---- 1. the ladder ---------------------------------------------------------------------------------------

LADDER_MASKS = {"none kept": [], "seed 1": seeded_pairs(ROW_FIELDS, 1, 0.5), "seed 2": seeded_pairs(ROW_FIELDS, 2, 0.5),
                "seed 3": seeded_pairs(ROW_FIELDS, 3, 0.5)}


@functools.lru_cache(maxsize=None)
def ladder_masked(k, fmt):
    """{mask name: {subset: (logits, probabilities, loss sum)}} under the oracle that holds the ladder weights as an
    engine of format `fmt` does, the dropped pairs' slots zeroed ("none kept": vec_w all zero).  Asserts the
    zeroed-slot argument's conditions and that no mask is vacuous.  Read-only."""
    st = ladder_weights(k)
    assert st["bias3"][:1].view(np.uint32)[0] != 0x80000000, "the bias is not -0.0"
    assert one_field_per_id(ladder_block(), ROW_IDS_PER_FIELD, ROW_FIELDS)
    held = decoded(st["vec_w"], fmt)
    o = CpuModel("oracle", "FFM", NF, ROW_FIELDS, k, **STRESS_HP)
    z = o.zero_state()
    z["bias3"][0] = st["bias3"][0]
    z["lin_w"][...] = st["lin_w"]
    z["vec_w"] = held
    o.set_state(z)
    whole = o.predict_batch(ladder_block())[0]
    present = pairs_present(ladder_block(), ROW_FIELDS)
    done = {}
    for name, kept in LADDER_MASKS.items():
        z["vec_w"] = np.zeros_like(held) if not kept else masked_weights(held, ROW_FIELDS, ROW_IDS_PER_FIELD, kept)
        o.set_state(z)
        done[name] = {}
        for s in LADDER_SUBSETS:
            b = ladder_sub(s)
            lg, ls = o.predict_batch(b)
            done[name][s] = (lg, o.predict_batch(b, output_prob=True)[0], ls)
            for a in done[name][s][:2]:
                a.setflags(write=False)
        assert (done[name]["all"][0].view(np.uint32) != whole.view(np.uint32)).any(), "mask %s changes no row" % name
        if kept:
            assert 0 < len(kept) < V6 and set(kept) & present, "mask %s keeps no pair of the block" % name
    return done


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_ladder(k, kind):
    """Rows of 0 .. 128 entries (erased ids and fields, descending fields, an id twice; 128 entries are 8128
    candidate pairs -- 127 walk steps, many refills of the queue, most of them diagonal pairs with 6 fields), and
    blocks of 1, 5 and 0 rows.  (a) all kept: the engine's own unmasked bits; (b) none kept and (d) three half-density
    masks: the oracle on zeroed slots; (c) each of the 21 masks that drops one pair: the engine's own
    predict_pair_ablated variant, taken before the mask is set."""
    fmt = "f16" if kind == "f16" else "f32"  # (a training engine and an fp32 serving engine hold the same bits)
    want = ladder_masked(k, fmt)
    e = engine_of(kind, k, ladder_weights(k))
    e.pair_ablation_enable()
    plain, ablated = {}, {}
    for s in LADDER_SUBSETS:
        b = ladder_sub(s)
        plain[s] = outputs(e, b)
        lg, ls = e.predict_pair_ablated(b)
        ablated[s] = (lg, e.predict_pair_ablated(b, output_prob=True)[0], ls)
    e.set_pair_mask(all_pairs(ROW_FIELDS))
    for s in LADDER_SUBSETS:
        check(e, ladder_sub(s), plain[s], "k=%d %s all kept, rows %s" % (k, kind, s))
    for name, kept in LADDER_MASKS.items():
        e.set_pair_mask(kept)
        for s in LADDER_SUBSETS:
            check(e, ladder_sub(s), want[name][s], "k=%d %s mask %s, rows %s" % (k, kind, name, s))
    for v in range(V6):
        e.set_pair_mask([p for p in all_pairs(ROW_FIELDS) if p != pair_fields(ROW_FIELDS, v)])
        for s in LADDER_SUBSETS:
            check(e, ladder_sub(s), tuple(a[v] for a in ablated[s]), "k=%d %s without pair %r, rows %s" % (k, kind, pair_fields(ROW_FIELDS, v), s))
    e.close()


# ---- 2. every word and bit -------------------------------------------------------------------------------

def word_masks(F):
    one = [(0, 0), (0, 1), (0, F - 1), (F - 2, F - 1), (F - 1, F - 1)]  # (F = 64: bit 63 of word 63 and of word 0)
    masks = {"checkerboard": [(f, g) for f, g in all_pairs(F) if (f + g) % 2 == 0],
             "band": [(f, g) for f, g in all_pairs(F) if g - f <= 1],
             "diagonal": [(f, f) for f in range(F)],
             "seed 25%": seeded_pairs(F, 100 + F, 0.25)}
    masks.update({"only %r" % (p,): [p] for p in one})
    return masks


@pytest.mark.parametrize("F", [10, 11, 39, 64])
def test_every_word_and_bit(F):
    """13 rows of up to F + 1 entries (regular rows, rows that lack fields, a row with two entries of the last
    field).  Every mask against a twin engine's unmasked predict_batch with the dropped pairs' slots zeroed through
    set_rows; the checkerboard, the seeded mask and the two corner bits against the oracle as well."""
    k, per = 8, 3
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(70 + F), o)
    assert st["bias3"][:1].view(np.uint32)[0] != 0x80000000
    blk = lanes_block(F, per, seed=F)
    assert blk.n_rows == 13 and int(np.diff(blk.row_ptr).max()) == F + 1 and one_field_per_id(blk, per, F)
    present = pairs_present(blk, F)
    e, twin = training(k, st, nf, F, max_batch_rows=16), training(k, st, nf, F, max_batch_rows=16)
    whole = outputs(e, blk)
    ids = np.arange(nf)
    with_oracle = ("checkerboard", "seed 25%", "only %r" % ((0, F - 1),), "only %r" % ((F - 1, F - 1),))
    for name, kept in word_masks(F).items():
        # (no row has two entries of field 0: that mask keeps a bit no row uses, and every term goes)
        assert set(kept) & present or kept == [(0, 0)], (F, name)
        words = pair_mask(F, kept)
        assert pair_mask_pairs(words) == sorted(kept)
        e.set_pair_mask(words)
        assert np.array_equal(e.pair_mask(), words)
        w = masked_weights(st["vec_w"], F, per, kept)
        twin.set_rows(ids, {"vec_w": w})
        want = outputs(twin, blk)
        assert (want[0].view(np.uint32) != whole[0].view(np.uint32)).any(), (F, name, "the mask changes no row")
        check(e, blk, want, "F=%d mask %s vs the twin" % (F, name))
        if name in with_oracle:
            o.set_state(dict(st, vec_w=w))
            check(e, blk, (o.predict_batch(blk)[0], o.predict_batch(blk, output_prob=True)[0], o.predict_batch(blk)[1]),
                  "F=%d mask %s vs the oracle" % (F, name))
    e.set_pair_mask(None)
    assert e.pair_mask() is None
    check(e, blk, whole, "F=%d after clearing" % F)
    e.close()
    twin.close()


# ---- 3. every prediction entry point ---------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f16", "train"])
def test_every_entry_point_gives_the_masked_predict_batch_bits(kind):
    k = 16
    kept = LADDER_MASKS["seed 2"]
    e = engine_of(kind, k, ladder_weights(k))
    blocks = [ladder_block(3), ladder_block(4), take_rows(ladder_block(3), []), ladder_block(5)]
    unmasked = e.predict_batch(blocks[0])[0]
    e.set_pair_mask(kept)
    want = [outputs(e, b) for b in blocks]
    assert (want[0][0].view(np.uint32) != unmasked.view(np.uint32)).any()
    e.metrics_enable(eval=True)
    pos, neg = np.zeros(fa.METRIC_BINS, np.uint64), np.zeros(fa.METRIC_BINS, np.uint64)
    n_nan = 0

    def counted(b, w):
        nonlocal pos, neg, n_nan
        p, n, nn = numpy_histogram(w[1], b.label)
        pos, neg, n_nan = pos + p, neg + n, n_nan + nn

    # _device (the row cap is the engine's max_row_nnz)
    for b, w in zip(blocks, want):
        if b.n_rows == 0:
            continue
        d = device_arrays(b)
        out = torch.full((b.n_rows,), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.predict_batch_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                               d["val"].data_ptr(), d["label"].data_ptr(), True, out.data_ptr(), loss.data_ptr())
        e.sync()
        counted(b, w)
        assert_rows_bitwise(out.cpu().numpy(), w[1], b, "predict_batch_device")
        assert loss_close(float(loss.cpu()[0]), w[2])
    # _async without scores: the flush's loss sum; with scores: the bits; copied and zero-copy
    total = sum(w[2] for w in want)
    for zero_copy in (False, True):
        host = [own_pages(b) for b in blocks] if zero_copy else blocks
        if zero_copy:
            for b in host:
                e.pin_block(b)
        for b, w in zip(host, want):
            e.predict_batch_async(b, zero_copy=zero_copy)
            counted(b, w)
        assert loss_close(e.train_flush(), total), zero_copy
        for prob in (False, True):
            outs = [e.score_buffer(b.n_rows + 8) for b in blocks]
            for b, out, w in zip(host, outs, want):
                out[:] = np.float32(-7.0)
                e.predict_batch_async(b, zero_copy=zero_copy, scores=out, output_prob=prob)
                counted(b, w)
            assert loss_close(e.train_flush(), total)
            for b, out, w in zip(blocks, outs, want):
                assert_rows_bitwise(out[:b.n_rows], w[1 if prob else 0], b, "async scores zero_copy=%d prob=%d" % (zero_copy, prob))
                assert (out[b.n_rows:] == np.float32(-7.0)).all()
            for out in outs:
                e.free_score_buffer(out)
        if zero_copy:
            for b in host:
                e.unpin_block(b)
    # a block resident in HBM
    b, w = blocks[1], want[1]
    cutter = fa.RowCutter(b.n_rows, int(b.row_ptr[-1]), n_blocks=2)
    cutter.take_host(b.n_rows, b.row_ptr, b.field, b.feat, b.val, b.label)
    res = cutter.close()
    for prob in (False, True):
        buf = e.score_buffer(b.n_rows)
        e.predict_async_resident(res, scores=buf, output_prob=prob)
        counted(b, w)
        assert loss_close(e.train_flush(), w[2])
        assert_rows_bitwise(buf[:b.n_rows].copy(), w[1 if prob else 0], b, "predict_async_resident prob=%d" % prob)
        e.free_score_buffer(buf)
    cutter.release(res)
    cutter.destroy()
    # the eval channel saw the masked scores of every labelled block since it was turned on
    hp, hn = e.metrics_histogram("eval")[:2]
    assert np.array_equal(hp, pos) and np.array_equal(hn, neg) and n_nan == 0
    e.close()


# ---- 4. order --------------------------------------------------------------------------------------------

def test_blocks_are_scored_under_the_mask_they_were_queued_under():
    k = 16
    kept = LADDER_MASKS["seed 1"]
    e = serving(k, "f32", ladder_weights(k))
    A, B, C = ladder_block(3), ladder_block(4), ladder_block(5)
    plain = {id(b): e.predict_batch(b)[0] for b in (A, B, C)}
    e.set_pair_mask(kept)
    masked = e.predict_batch(B)[0]
    assert (masked.view(np.uint32) != plain[id(B)].view(np.uint32)).any()
    e.set_pair_mask(None)
    assert e.pair_mask() is None
    bufs = [e.score_buffer(b.n_rows) for b in (A, B, C)]
    e.predict_batch_async(A, scores=bufs[0])
    e.set_pair_mask(kept)
    assert np.array_equal(e.pair_mask(), pair_mask(ROW_FIELDS, kept))
    e.predict_batch_async(B, scores=bufs[1])
    e.set_pair_mask(None)
    assert e.pair_mask() is None
    e.predict_batch_async(C, scores=bufs[2])
    e.train_flush()
    assert_rows_bitwise(bufs[0][:A.n_rows].copy(), plain[id(A)], A, "A: queued before the mask")
    assert_rows_bitwise(bufs[1][:B.n_rows].copy(), masked, B, "B: queued under the mask")
    assert_rows_bitwise(bufs[2][:C.n_rows].copy(), plain[id(C)], C, "C: queued after clearing")
    for buf in bufs:
        e.free_score_buffer(buf)
    e.close()


# ---- 5. hashed ids, rows without values, normalised rows -------------------------------------------------

def test_hash_ids_no_values_and_normalize_act_before_the_mask():
    """A hash_ids=True, normalize=True engine on raw ids without values against a plain engine on the block that
    fa.hash_ids and fa.normalize_rows make of it, both under the same mask: the norm is the whole row's."""
    k = 8
    st, b = ladder_weights(k), ladder_block()
    kept = LADDER_MASKS["seed 3"]
    fs = (np.arange(ROW_FIELDS + 1) * ROW_IDS_PER_FIELD).astype(np.int32)
    h = training(k, st, hash_ids=True, field_start=fs, normalize=True)
    e = training(k, st)
    rng = np.random.default_rng(8)
    fld = np.clip(b.field, 0, ROW_FIELDS - 1)  # (hashing needs a field in range for every entry)
    raw = Csr(b.row_ptr, fld, rng.integers(0, 2 ** 31 - 1, b.feat.size).astype(np.int32), None, b.label)
    ids = fa.hash_ids(fld, raw.feat, NF, fs)
    val = fa.normalize_rows(b.row_ptr, fld, ids, np.ones(ids.size, np.float32), NF, ROW_FIELDS)
    prepared = Csr(b.row_ptr, fld, ids, val, b.label)
    unmasked = e.predict_batch(prepared)[0]
    for x in (h, e):
        x.set_pair_mask(kept)
    want = outputs(e, prepared)
    assert (want[0].view(np.uint32) != unmasked.view(np.uint32)).any()
    check(h, raw, want, "hash_ids + val=None + normalize under a mask")
    h.close()
    e.close()


# ---- 6. a row too long -----------------------------------------------------------------------------------

def test_overlong_row_is_nan_on_a_masked_training_engine():
    """max_row_nnz = 150 and one row of 129 entries: more than a wave stages, and a masked engine launches no other
    row kernel.  That row is NaN, the others are what they are without it, and the call reports the row."""
    k = 16
    st = ladder_weights(k)
    kept = LADDER_MASKS["seed 2"]
    base = take_rows(ladder_block(), [int(np.flatnonzero(np.diff(ladder_block().row_ptr) == n)[0]) for n in (5, 128, 0, 33)])
    rng = np.random.default_rng(5)
    long_field = rng.integers(0, ROW_FIELDS, 129).astype(np.int32)
    long_feat = (long_field * ROW_IDS_PER_FIELD + rng.integers(0, ROW_IDS_PER_FIELD, 129)).astype(np.int32)
    at = 2  # the long row goes in as row 2
    lens = np.insert(np.diff(base.row_ptr), at, 129)
    cut = int(base.row_ptr[at])
    b = Csr(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.insert(base.field, cut, long_field),
            np.insert(base.feat, cut, long_feat), np.insert(base.val, cut, np.ones(129, np.float32)), np.insert(base.label, at, 1))
    assert int(np.diff(b.row_ptr)[at]) == 129
    e = training(k, st, max_row_nnz=150)
    e.set_pair_mask(kept)
    want = e.predict_batch(base)[0]  # (pinned to the oracle by test_ladder)
    lib = e.lib
    out = np.zeros(b.n_rows, np.float32)
    loss = ctypes.c_double(0.0)
    n, rp, fld, ft, v, lab = e._csr(b)
    rc = lib.ffm_engine_predict_batch(e.h, n, rp, fld, ft, v, lab, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(loss))
    assert rc == E_CAPACITY and "max_row_nnz" in lib.ffm_engine_last_error().decode()
    others = [r for r in range(b.n_rows) if r != at]
    assert np.isnan(out[at]) and np.isnan(loss.value)
    assert_bitwise(out[others], want, "beside the long row")
    e.sync()  # the report cleared the flag
    e.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------

def code_of(call):
    with pytest.raises(fa.EngineError) as ei:
        call()
    return ei.value.code, str(ei.value)


def test_unsupported_engines(monkeypatch):
    for what, e in (("LR", fa.Engine("LR", 64, 1, 1, max_batch_rows=16)), ("FM", fa.Engine("FM", 64, 1, 4, max_batch_rows=16)),
                    ("n_fields = 65", fa.Engine("FFM", 130, 65, 4, max_batch_rows=16)),
                    ("n_factors = 12", fa.Engine("FFM", 64, 4, 12, max_batch_rows=16)),
                    ("a shard", fa.Engine("FFM", 64, 4, 4, max_batch_rows=16, n_shards=2, shard_rank=0))):
        code, msg = code_of(lambda: e.set_pair_mask(np.zeros(e.n_fields, np.uint64)))
        assert code == E_UNSUPPORTED and "pair mask" in msg, (what, msg)
        assert e.pair_mask() is None
        e.close()
    g = fa.Group([0], "FFM", NF, ROW_FIELDS, 4, max_batch_rows=256, max_batch_nnz=256 * 128)
    code, msg = code_of(lambda: g.engines[0].set_pair_mask(all_pairs(ROW_FIELDS)))
    assert code == E_UNSUPPORTED and "group" in msg, msg
    g.close()
    monkeypatch.setenv("FFM_PREDICT_WAVE", "0")
    e = training(16, ladder_weights(16))
    monkeypatch.delenv("FFM_PREDICT_WAVE")
    code, msg = code_of(lambda: e.set_pair_mask(all_pairs(ROW_FIELDS)))
    assert code == E_UNSUPPORTED and "FFM_PREDICT_WAVE" in msg, msg
    e.close()
    s = serving(16, "f16", ladder_weights(16))  # (a serving engine has the wave kernels whatever the variable says)
    s.set_pair_mask(all_pairs(ROW_FIELDS))
    s.close()


def test_a_refused_mask_leaves_the_previous_one_in_force():
    k = 16
    b = ladder_block()
    kept = LADDER_MASKS["seed 1"]
    e = training(k, ladder_weights(k))
    e.set_pair_mask(kept)
    want = outputs(e, b)
    good = pair_mask(ROW_FIELDS, kept)
    lopsided = good.copy()
    f, g = next(p for p in all_pairs(ROW_FIELDS) if p[0] != p[1])
    lopsided[f] ^= np.uint64(1 << g)
    high = good.copy()
    high[0] |= np.uint64(1 << ROW_FIELDS)
    for what, words in (("7 fields", pair_mask(ROW_FIELDS + 1, kept)), ("5 fields", good[:-1]), ("symmetric", lopsided),
                        ("at or above", high)):
        code, msg = code_of(lambda: e.set_pair_mask(words))
        assert code == E_INVALID and what in msg, (what, msg)
        assert np.array_equal(e.pair_mask(), good)
        check(e, b, want, "after a refused mask (%s)" % what)
    e.close()


def test_what_would_run_unmasked_is_refused_and_changes_nothing():
    k = 16
    st, b = ladder_weights(k), ladder_block()
    w = np.ones(b.n_rows, np.float32)
    e = training(k, st)
    e.ablation_enable()
    e.pair_ablation_enable()
    e.set_pair_mask(LADDER_MASKS["seed 1"])
    before = e.get_state()
    calls = {
        "train_batch": lambda: e.train_batch(b),
        "train_batch_weighted": lambda: e.train_batch(b, weight=w),
        "train_batch_async": lambda: e.train_batch_async(b),
        "train_batch_async_pinned": lambda: e.train_batch_async_pinned(b),
        "stage_batch": lambda: e.stage_batch(b),
        "train_staged": lambda: e.train_staged(),
        "train_forward_staged": lambda: e.train_forward_staged(),
        "train_batch_device": lambda: e.train_batch_device(0, 0, None, None, None, None, None),
        "train_forward_device": lambda: e.train_forward_device(0, 0, None, None, None, None, None, None),
        "train_update_device": lambda: e.train_update_device(None),
        "prepare_device": lambda: e.prepare_device(0, 0, None, None, None, None),
        "predict_ablated": lambda: e.predict_ablated(b),
        "predict_ablated_device": lambda: e.predict_ablated_device(0, 0, None, None, None, None, None, 0, None),
        "predict_pair_ablated": lambda: e.predict_pair_ablated(b),
        "predict_pair_ablated_device": lambda: e.predict_pair_ablated_device(0, 0, None, None, None, None, None, 0, None),
    }
    for name, call in calls.items():
        code, msg = code_of(call)
        assert code == E_INVALID and "pair mask" in msg, (name, msg)
    assert e.blocks_pulled() == 0
    assert_state_bitwise(e.get_state(), before, "the state after the refusals")
    e.set_pair_mask(None)
    e.train_batch(b)  # (and training is back once the mask is gone)
    e.close()
    # candidates on a serving engine
    s = serving(k, "f16", st)
    ctx = take_rows(b, [int(np.flatnonzero(np.diff(b.row_ptr) == 5)[0])])
    cand = take_rows(b, [int(np.flatnonzero(np.diff(b.row_ptr) == n)[0]) for n in (3, 4)])
    req = np.array([0, 2], np.int32)
    want = s.score_candidates(ctx, req, cand)
    s.set_pair_mask(LADDER_MASKS["seed 1"])
    code, msg = code_of(lambda: s.score_candidates(ctx, req, cand))
    assert code == E_INVALID and "pair mask" in msg, msg
    code, msg = code_of(lambda: s.score_candidates_device(1, None, None, None, None, None, 1, None, None, None, None, 0, 0, 1, 0, None))
    assert code == E_INVALID and "pair mask" in msg, msg
    s.set_pair_mask(None)
    assert_bitwise(s.score_candidates(ctx, req, cand), want, "candidates after clearing the mask")
    s.close()
