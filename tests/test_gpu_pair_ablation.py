"""Pair ablation (include/ffm_engine.h "Pair ablation"; csrc/kernels_ablate_pairs.h, csrc/engine_ablate.h):
the V + 1 = n_fields (n_fields + 1) / 2 + 1 variants of every row from one pass.

The expected value of variant (f, g) is predict_batch of the SAME block on weights whose latent slot "towards field
g" is +0.0 for every id of field f (ftrl_ffm_amd.drop_pair_weights): in a block where every id occurs under one
field only, on a model whose bias is not -0.0, those terms become +-0.0, and adding +-0.0 to a running sum that
is never -0.0 equals leaving the term out (the argument is checked on the oracle alone in
tests/test_pair_ablation_host.py).  So the yardsticks are oracle.pyoracle.CpuModel and a twin engine's existing
predict_batch: logits and probabilities bit for bit (NaN with NaN), double loss sums by util.loss_close.  Nothing
else here has a tolerance."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_pair_weights, pair_count, pair_fields, pair_index
from oracle.pyoracle import CpuModel, Csr
from test_gpu_field_ablation import engine_of, lanes_block, numpy_histogram, training
from test_gpu_serve import NF, decoded, ladder_block, ladder_weights, serving
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, loss_close, rand_state, take_rows

pytestmark = pytest.mark.gpu

KINDS = ("train", "f32", "f16")  # a training engine, the two serving formats
BINS = fa.METRIC_BINS
E_INVALID, E_CAPACITY, E_UNSUPPORTED = fa.engine.E_INVALID, fa.engine.E_CAPACITY, fa.engine.E_UNSUPPORTED
V6 = 21  # the pairs of the ladder's 6 fields: one round of 64 lanes


def one_field_per_id(blk, per, n_fields):
    """The input condition of the zeroed-slot argument, over the entries the model keeps."""
    kept = (blk.feat >= 0) & (blk.feat < n_fields * per) & (blk.field >= 0) & (blk.field < n_fields)
    return bool(np.array_equal(blk.field[kept], blk.feat[kept] // per))


def variant_weights(vec_w, n_fields, per, v):
    """vec_w [n_feats, n_fields * k] for variant v: the pair's slot zeroed, or vec_w itself for v == V."""
    if v == pair_count(n_fields):
        return vec_w
    f, g = pair_fields(n_fields, v)
    w3 = np.asarray(vec_w).reshape(vec_w.shape[0], n_fields, -1)
    return drop_pair_weights(w3, np.arange(f * per, (f + 1) * per), g).reshape(vec_w.shape)


LADDER_SUBSETS = ("all", "longest", "five", "none")


@functools.lru_cache(maxsize=None)
def ladder_rows(subset):
    blk = ladder_block()
    lens = np.diff(blk.row_ptr)
    if subset == "all":
        return None
    if subset == "longest":
        return (int(np.argmax(lens)),)
    if subset == "five":
        return tuple(int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33))
    return ()


def ladder_sub(subset):
    rows = ladder_rows(subset)
    return ladder_block() if rows is None else take_rows(ladder_block(), list(rows))


@functools.lru_cache(maxsize=None)
def ladder_expected(k, fmt):
    """{subset: (logits, probabilities, loss sums)} of the 22 variants of the ladder block and its sub-blocks under
    one oracle that holds, variant after variant, the ladder weights as an engine of format `fmt` does with the
    pair's slot zeroed.  Read-only."""
    st = ladder_weights(k)
    assert st["bias3"][:1].view(np.uint32)[0] != 0x80000000, "the bias is not -0.0"
    assert one_field_per_id(ladder_block(), ROW_IDS_PER_FIELD, ROW_FIELDS)
    held = decoded(st["vec_w"], fmt)
    o = CpuModel("oracle", "FFM", NF, ROW_FIELDS, k, **STRESS_HP)
    z = o.zero_state()
    z["bias3"][0] = st["bias3"][0]
    z["lin_w"][...] = st["lin_w"]
    out = {s: ([], [], []) for s in LADDER_SUBSETS}
    for v in range(V6 + 1):
        z["vec_w"] = variant_weights(held, ROW_FIELDS, ROW_IDS_PER_FIELD, v)
        o.set_state(z)
        for s in LADDER_SUBSETS:
            b = ladder_sub(s)
            a, l = o.predict_batch(b)
            out[s][0].append(a)
            out[s][1].append(o.predict_batch(b, output_prob=True)[0])
            out[s][2].append(l)
    done = {}
    for s, (lg, pr, ls) in out.items():
        done[s] = (np.stack(lg), np.stack(pr), np.array(ls))
        for a in done[s]:
            a.setflags(write=False)
    return done


def check_pairs(e, blk, want, what):
    lg, pr, ls = want
    for prob, exp in ((False, lg), (True, pr)):
        got, gl = e.predict_pair_ablated(blk, output_prob=prob)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        for v in range(exp.shape[0]):
            assert_rows_bitwise(got[v], exp[v], blk, "%s variant %d %s" % (what, v, "probabilities" if prob else "logits"))
        for v in range(exp.shape[0]):
            assert loss_close(gl[v], ls[v]), "%s variant %d: loss sum %r vs %r" % (what, v, gl[v], ls[v])


# ---- 1. the ladder ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_ladder(k, kind):
    """Rows of 0 .. 128 entries (erased ids and fields, descending fields, an id twice, a row count that is no
    multiple of 4; 128 entries are 8128 pairs, many 256-term batches), and blocks of 1, 5 and 0 rows: all 22
    variants, logits and probabilities, bit for bit; loss sums by loss_close."""
    fmt = "f16" if kind == "f16" else "f32"  # (a training engine and an fp32 serving engine hold the same bits)
    want = ladder_expected(k, fmt)
    e = engine_of(kind, k, ladder_weights(k))
    e.pair_ablation_enable()
    for s in LADDER_SUBSETS:
        check_pairs(e, ladder_sub(s), want[s], "k=%d %s ladder rows %s" % (k, kind, s))
    e.close()


# ---- 2. every round and lane -----------------------------------------------------------------------------

@pytest.mark.parametrize("F", [10, 11, 39, 64])
def test_every_round_and_lane(F):
    """V = 55 (a partly filled single round), 66 (two rounds, 2 variants in the second), 780 (the headline shape: 13
    rounds, the last partly filled) and 2080 (33 rounds).  A few variants against the oracle, every other one
    against a twin engine's predict_batch with the slot zeroed through set_rows; then the identities."""
    k, per = 8, 3
    nf, V = F * per, pair_count(F)
    o = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(70 + F), o)
    assert st["bias3"][:1].view(np.uint32)[0] != 0x80000000
    blk = lanes_block(F, per, seed=F)
    assert blk.n_rows == 13 and int(np.diff(blk.row_ptr).max()) == F + 1 and one_field_per_id(blk, per, F)
    e, twin = training(k, st, nf, F, max_batch_rows=16), training(k, st, nf, F, max_batch_rows=16)
    e.pair_ablation_enable()
    got = {prob: e.predict_pair_ablated(blk, output_prob=prob) for prob in (False, True)}
    assert got[False][0].shape == (V + 1, blk.n_rows)
    with_oracle = {pair_index(F, 0, 0), pair_index(F, 0, 1), pair_index(F, 0, F - 1), pair_index(F, F - 2, F - 1),
                   pair_index(F, F - 1, F - 1), V} | {v for v in (63, 64, 127, 128) if v < V}

    def compare(v, model):
        for prob in (False, True):
            want, wl = model.predict_batch(blk, output_prob=prob)
            assert_rows_bitwise(got[prob][0][v], want, blk, "F=%d variant %d %r prob=%d" % (F, v, pair_fields(F, v) if v < V else "whole", prob))
            assert loss_close(got[prob][1][v], wl), (F, v, got[prob][1][v], wl)

    z = dict(st)
    for v in sorted(with_oracle):
        z["vec_w"] = variant_weights(st["vec_w"], F, per, v)
        o.set_state(z)
        compare(v, o)
    w3 = st["vec_w"].reshape(nf, F, k)
    for f in range(F):
        ids = np.arange(f * per, (f + 1) * per)
        for g in range(f, F):
            v = pair_index(F, f, g)
            if v in with_oracle:
                continue
            twin.set_rows(ids, {"vec_w": drop_pair_weights(w3, ids, g)[ids].reshape(per, F * k)})  # (also puts slot g - 1 back)
            compare(v, twin)
        twin.set_rows(ids, {"vec_w": st["vec_w"][ids]})
    lg = got[False][0]
    # variant V is the engine's own predict_batch
    assert_bitwise(lg[V], e.predict_batch(blk)[0], "F=%d variant V" % F)
    assert_bitwise(lg[V], twin.predict_batch(blk)[0], "F=%d the twin was put back" % F)
    # a row lacking g has variant (f, g) equal to variant V
    lacking = blk.n_rows - 3  # (the row of the first half of the fields)
    for g in range(F // 2, F):
        for f in range(0, g + 1):
            v = pair_index(F, f, g)
            assert lg[v, lacking].view(np.uint32) == lg[V, lacking].view(np.uint32), (f, g)
    # variant (F - 1, F - 1) differs from V only in the row with the repeated field
    differs = lg[pair_index(F, F - 1, F - 1)].view(np.uint32) != lg[V].view(np.uint32)
    assert differs.tolist() == [False] * (blk.n_rows - 1) + [True]
    e.close()
    twin.close()


# ---- 3. the other ways in --------------------------------------------------------------------------------

def device_arrays(b):
    return {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}


def test_device_entry_point_gives_the_host_call_bits():
    k = 16
    e = serving(k, "f16", ladder_weights(k))
    e.pair_ablation_enable()
    b = ladder_block()
    V = V6 + 1
    d = device_arrays(b)
    for prob in (False, True):
        want, wl = e.predict_pair_ablated(b, output_prob=prob)
        out = torch.full((V * b.n_rows,), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.full((V,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.predict_pair_ablated_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                                      d["val"].data_ptr(), d["label"].data_ptr(), prob, out.data_ptr(), loss.data_ptr())
        e.sync()
        assert_bitwise(out.cpu().numpy().reshape(V, b.n_rows), want, "predict_pair_ablated_device prob=%d" % prob)
        assert np.array_equal(loss.cpu().numpy(), wl)
    e.close()


def test_rows_without_values_and_hashed_ids():
    """val=None gives the bits of numpy.ones; a hash_ids=True engine on raw ids gives the bits of a plain engine
    on fa.hash_ids ids (fields are not touched by hashing)."""
    k = 8
    st, b = ladder_weights(k), ladder_block()
    e = training(k, st)
    e.pair_ablation_enable()
    ones = Csr(b.row_ptr, b.field, b.feat, np.ones(b.feat.size, np.float32), b.label)
    none = Csr(b.row_ptr, b.field, b.feat, None, b.label)
    a, la = e.predict_pair_ablated(ones)
    c, lc = e.predict_pair_ablated(none)
    assert_bitwise(c, a, "val=None")
    assert np.array_equal(la, lc)
    fs = (np.arange(ROW_FIELDS + 1) * ROW_IDS_PER_FIELD).astype(np.int32)
    h = training(k, st, hash_ids=True, field_start=fs)
    h.pair_ablation_enable()
    rng = np.random.default_rng(8)
    fld = np.clip(b.field, 0, ROW_FIELDS - 1)  # (hashing needs a field in range for every entry)
    raw = Csr(b.row_ptr, fld, rng.integers(0, 2 ** 31 - 1, b.feat.size).astype(np.int32), b.val, b.label)
    hashed = Csr(b.row_ptr, fld, fa.hash_ids(fld, raw.feat, NF, fs), b.val, b.label)
    a, la = h.predict_pair_ablated(raw)
    c, lc = e.predict_pair_ablated(hashed)
    assert_bitwise(a, c, "hash_ids")
    assert np.array_equal(la, lc)
    h.close()
    e.close()


def test_scores_false_returns_the_same_loss_sums():
    k = 16
    b = ladder_block()
    e = serving(k, "f32", ladder_weights(k))
    e.pair_ablation_enable()
    out, want = e.predict_pair_ablated(b)
    none, got = e.predict_pair_ablated(b, scores=False)
    assert out is not None and none is None
    assert got.shape == (V6 + 1,) and np.array_equal(got, want) and (want != 0).all()
    assert not e.predict_pair_ablated(b, with_loss=False, scores=False)[1].any()
    e.close()


# ---- 4. the histograms -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prob", [False, True])
def test_auc_of_five_variants(prob):
    """After two blocks pair_ablation_metrics()[v] is fa.metrics_from_histogram of the numpy histogram of the
    oracle's probabilities on the zeroed-slot weights: the integers and auc exactly; reset zeroes them."""
    k = 16
    st = ladder_weights(k)
    blocks = [ladder_block(3), ladder_block(4)]
    for b in blocks:  # the input conditions: both classes in both blocks, an id under one field
        assert (b.label > 0).any() and (b.label <= 0).any() and one_field_per_id(b, ROW_IDS_PER_FIELD, ROW_FIELDS)
    e = training(k, st)
    e.pair_ablation_enable(auc=True)
    for b in blocks:
        e.predict_pair_ablated(b, output_prob=prob)
    got = e.pair_ablation_metrics()
    assert len(got) == V6 + 1
    o = CpuModel("oracle", "FFM", NF, ROW_FIELDS, k, **STRESS_HP)
    z = o.zero_state()
    z["bias3"][0] = st["bias3"][0]
    z["lin_w"][...] = st["lin_w"]
    chosen = (pair_index(6, 0, 0), pair_index(6, 0, 5), pair_index(6, 2, 3), pair_index(6, 5, 5), V6)
    for v in chosen:
        z["vec_w"] = variant_weights(st["vec_w"], ROW_FIELDS, ROW_IDS_PER_FIELD, v)
        o.set_state(z)
        pos, neg, n_nan = np.zeros(BINS, np.uint64), np.zeros(BINS, np.uint64), 0
        for b in blocks:
            p, n, nn = numpy_histogram(o.predict_batch(b, output_prob=True)[0], b.label)
            pos, neg, n_nan = pos + p, neg + n, n_nan + nn
        want = fa.metrics_from_histogram(pos, neg, n_nan)
        assert got[v] == want, (v, got[v], want)
        assert want["n_pos"] + want["n_neg"] == sum(b.n_rows for b in blocks)
    assert len({got[v]["auc"] for v in chosen}) > 1, "the variants' AUCs should not all coincide on these weights"
    assert e.pair_ablation_metrics(reset=True) == got
    for m in e.pair_ablation_metrics():
        assert m["n_pos"] == 0 and m["n_neg"] == 0 and m["n_nan"] == 0
    e.close()


def test_channels_and_field_ablation_untouched():
    """With the eval channel, keyed capture and field ablation on, predict_pair_ablated changes none of them."""
    k = 16
    b = ladder_block()
    e = training(k, ladder_weights(k))
    e.metrics_enable(eval=True, train=True)
    e.metrics_key_field(0, 1000, eval=True)
    e.ablation_enable(auc=True)
    e.pair_ablation_enable(auc=True)
    e.predict_batch(b)
    field_out, field_loss = e.predict_ablated(b)
    before, train_before, keyed_before, field_before = e.metrics("eval"), e.metrics("train"), e.metrics_read_keyed("eval"), e.ablation_metrics()
    assert before["n_pos"] + before["n_neg"] == b.n_rows
    e.predict_pair_ablated(b)
    e.predict_pair_ablated(b, output_prob=True)
    assert e.metrics("eval") == before
    counts = lambda m: (m["n_pos"], m["n_neg"], m["n_nan"])  # noqa: E731  (an empty channel's auc is NaN)
    assert counts(e.metrics("train")) == counts(train_before) == (0, 0, 0)
    assert e.metrics_read_keyed("eval") == keyed_before
    assert e.ablation_metrics() == field_before
    assert e.pair_ablation_metrics()[V6]["n_pos"] == 2 * before["n_pos"]
    again, again_loss = e.predict_ablated(b)
    assert_bitwise(again, field_out, "field ablation after pair calls")
    assert np.array_equal(again_loss, field_loss)
    e.close()


# ---- 5. rows too long, refusals --------------------------------------------------------------------------

def test_overlong_row_is_nan_in_every_variant():
    """A training engine with max_row_nnz = 150 and one row of 129 entries: more than a wave stages.  That row is
    NaN in every variant, every other row is what it is without the long row, and sync reports the row."""
    k = 16
    st = ladder_weights(k)
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
    e.pair_ablation_enable()
    want = e.predict_pair_ablated(base)[0]  # (pinned to the oracle by test_ladder)
    V = V6 + 1
    d = device_arrays(b)
    out = torch.zeros((V * b.n_rows,), dtype=torch.float32, device="cuda")
    loss = torch.zeros((V,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.predict_pair_ablated_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                                  d["val"].data_ptr(), d["label"].data_ptr(), False, out.data_ptr(), loss.data_ptr())
    with pytest.raises(fa.EngineError) as ei:
        e.sync()
    assert ei.value.code == E_CAPACITY and "max_row_nnz" in str(ei.value)
    got = out.cpu().numpy().reshape(V, b.n_rows)
    others = [r for r in range(b.n_rows) if r != at]
    assert np.isnan(got[:, at]).all()
    assert_bitwise(got[:, others], want, "beside the long row")
    assert np.isnan(loss.cpu().numpy()).all()
    e.sync()  # the report cleared the flag
    with pytest.raises(fa.EngineError) as ei:  # the host call reports it itself
        e.predict_pair_ablated(b)
    assert ei.value.code == E_CAPACITY
    e.close()


def code_of(call):
    with pytest.raises(fa.EngineError) as ei:
        call()
    return ei.value.code, str(ei.value)


def test_failed_histogram_allocation_leaves_the_engine_as_it_was(monkeypatch):
    """FFM_PAIR_HIST_FAIL=1 makes the histograms' allocation fail as an exhausted device does (the library's test
    hook).  A first enable(auc=True) then is FFM_E_NOMEM, pair ablation stays off and the scratch the call had made
    is given back; on an engine that is already on, the same failure leaves it on without histograms and its
    results unchanged.  Then with_auc on later calls: 0 stops the collection, 1 starts it from zero."""
    k = 16
    b = ladder_sub("five")
    want = ladder_expected(k, "f32")["five"]
    rows = 1 << 16  # (22 variants x 65536 rows x 12 bytes = 17 MB of scratch: visible in the device's free memory)
    E_NOMEM = fa.engine.E_NOMEM
    e = training(k, ladder_weights(k), max_batch_rows=rows)
    e.sync()
    free_before = torch.cuda.mem_get_info()[0]
    monkeypatch.setenv("FFM_PAIR_HIST_FAIL", "1")
    code, msg = code_of(lambda: e.pair_ablation_enable(auc=True))
    assert code == E_NOMEM and "bytes failed" in msg, msg
    assert torch.cuda.mem_get_info()[0] >= free_before - (4 << 20), "the scratch made before the failure was given back"
    code, msg = code_of(lambda: e.predict_pair_ablated(b))
    assert code == E_INVALID and "pair_ablation_enable" in msg
    e.pair_ablation_enable()  # (no histograms asked for: nothing to fail)
    check_pairs(e, b, want, "on, after a failed enable")
    code, msg = code_of(lambda: e.pair_ablation_enable(auc=True))
    assert code == E_NOMEM
    code, msg = code_of(e.pair_ablation_metrics)
    assert code == E_INVALID and "with_auc" in msg
    check_pairs(e, b, want, "still on without histograms")
    monkeypatch.delenv("FFM_PAIR_HIST_FAIL")
    e.pair_ablation_enable(auc=True)
    e.predict_pair_ablated(b)
    counts = lambda m: (m["n_pos"], m["n_neg"], m["n_nan"])  # noqa: E731
    counted = counts(e.pair_ablation_metrics()[V6])
    assert counted[0] + counted[1] == b.n_rows and counted[2] == 0
    e.pair_ablation_enable(auc=True)  # collection that stays on keeps its counts
    assert counts(e.pair_ablation_metrics()[V6]) == counted
    e.pair_ablation_enable(auc=False)  # stops it
    assert code_of(e.pair_ablation_metrics)[0] == E_INVALID
    e.predict_pair_ablated(b)
    e.pair_ablation_enable(auc=True)  # and a later one starts from zero
    assert counts(e.pair_ablation_metrics()[V6]) == (0, 0, 0)
    check_pairs(e, b, want, "after the switches")
    e.close()


def test_refusals():
    b = ladder_block()
    for what, e in (("LR", fa.Engine("LR", 64, 1, 1, max_batch_rows=16)), ("FM", fa.Engine("FM", 64, 1, 4, max_batch_rows=16)),
                    ("n_fields = 65", fa.Engine("FFM", 130, 65, 4, max_batch_rows=16)),
                    ("n_factors = 12", fa.Engine("FFM", 64, 4, 12, max_batch_rows=16)),
                    ("a shard", fa.Engine("FFM", 64, 4, 4, max_batch_rows=16, n_shards=2, shard_rank=0))):
        code, msg = code_of(e.pair_ablation_enable)
        assert code == E_UNSUPPORTED and "pair ablation" in msg, (what, msg)
        code, msg = code_of(lambda: e.predict_pair_ablated(b))
        assert code == E_INVALID and "pair_ablation_enable" in msg, (what, msg)
        e.close()
    # a group's engine (a group of one holds a whole model, and still refuses), and the group goes on predicting
    g = fa.Group([0], "FFM", NF, ROW_FIELDS, 4, max_batch_rows=256, max_batch_nnz=256 * 128)
    code, msg = code_of(g.engines[0].pair_ablation_enable)
    assert code == E_UNSUPPORTED and "pair ablation" in msg and "group" in msg, msg
    code, msg = code_of(lambda: g.engines[0].predict_pair_ablated(b))
    assert code == E_INVALID and "pair_ablation_enable" in msg, msg
    out, _ = g.predict_batch(b)
    assert out.shape == (b.n_rows,) and not np.isnan(out).any()
    g.close()
    k = 16
    e = training(k, ladder_weights(k))
    code, msg = code_of(lambda: e.predict_pair_ablated(b))
    assert code == E_INVALID and "pair_ablation_enable" in msg
    assert code_of(e.pair_ablation_metrics)[0] == E_INVALID
    e.ablation_enable()  # (field ablation being on does not turn pair ablation on)
    assert code_of(lambda: e.predict_pair_ablated(b))[0] == E_INVALID
    e.pair_ablation_enable()
    code, msg = code_of(e.pair_ablation_metrics)
    assert code == E_INVALID and "with_auc" in msg
    # field == NULL stays refused on this synchronous call
    assert code_of(lambda: e.predict_pair_ablated(Csr(b.row_ptr, None, b.feat, b.val, b.label)))[0] == E_INVALID
    e.close()
    # more rows than max_batch_rows
    small = training(k, ladder_weights(k), max_batch_rows=16)
    small.pair_ablation_enable()
    assert b.n_rows > 16
    code, msg = code_of(lambda: small.predict_pair_ablated(b))
    assert code == E_CAPACITY and "max_batch_rows" in msg, msg
    # and the engine goes on working
    five = ladder_sub("five")
    assert_bitwise(small.predict_pair_ablated(five)[0], ladder_expected(k, "f32")["five"][0], "after the refusals")
    small.close()
