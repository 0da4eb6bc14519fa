"""The pruning curve (include/ffm_engine.h "Pruning curve"; csrc/kernels_curve.h, csrc/engine_ablate.h): the scores,
loss sums and AUC of up to 64 pair masks from one pass.

The yardstick is older than the curve's kernel: variant c is the same engine's predict_batch of the same block under
set_pair_mask(pair_curve_mask(level, cut[c])) (ffm_row_mask_kernel, pinned to the oracle by tests/test_gpu_pair_mask.py),
the last variant its unmasked predict_batch, and one dropped pair is that pair's variant of predict_pair_ablated.
Logits and probabilities bit for bit (NaN with NaN), double loss sums by util.loss_close.  Nothing else has a
tolerance."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import pair_count, pair_curve_levels, pair_curve_mask, pair_fields, pair_index
from oracle.pyoracle import CpuModel, Csr
from test_gpu_field_ablation import engine_of, lanes_block, numpy_histogram, training
from test_gpu_pair_ablation import device_arrays
from test_gpu_serve import NF, ladder_block, ladder_weights, serving
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, assert_state_bitwise, loss_close, rand_state, take_rows

pytestmark = pytest.mark.gpu

KINDS = ("train", "f32", "f16")  # a training engine, the two serving formats
E_INVALID, E_CAPACITY, E_UNSUPPORTED, E_NOMEM = fa.engine.E_INVALID, fa.engine.E_CAPACITY, fa.engine.E_UNSUPPORTED, fa.engine.E_NOMEM
V6 = 21  # the pairs of the ladder's 6 fields
LADDER_CUTS = [0, 3, 7, 21, 65536, 7]  # no pairs, a duplicate, all pairs


def seeded_levels(F, seed, hi):
    """A fixed-seed symmetric uint16 table with levels in [0, hi)."""
    a = np.random.default_rng(seed).integers(0, hi, (F, F))
    return np.triu(a).astype(np.uint16) + np.triu(a, 1).T.astype(np.uint16)


def outputs(e, blk):
    lg, ls = e.predict_batch(blk)
    return lg, e.predict_batch(blk, output_prob=True)[0], ls


def curve_outputs(e, blk):
    lg, ls = e.predict_pair_curve(blk)
    return lg, e.predict_pair_curve(blk, output_prob=True)[0], ls


def masked_yardstick(e, blk, level, cuts):
    """[(logits, probabilities, loss sum)] per cut under the cut's mask, then the unmasked ones; the mask is cleared."""
    want = []
    for c in cuts:
        e.set_pair_mask(pair_curve_mask(level, c))
        want.append(outputs(e, blk))
    e.set_pair_mask(None)
    want.append(outputs(e, blk))
    return want


def check_variants(got, want, blk, what):
    lg, pr, ls = got
    assert lg.shape == pr.shape == (len(want), blk.n_rows) and ls.shape == (len(want),), (what, lg.shape, ls.shape)
    for v, w in enumerate(want):
        assert_rows_bitwise(lg[v], w[0], blk, "%s variant %d logits" % (what, v))
        assert_rows_bitwise(pr[v], w[1], blk, "%s variant %d probabilities" % (what, v))
        assert loss_close(ls[v], w[2]), "%s variant %d: loss sum %r vs %r" % (what, v, ls[v], w[2])


def check_curve(e, blk, level, cuts, what, vacuous_ok=()):
    """Enables the curve and checks all its variants on blk against the masked yardstick; every cut that keeps fewer
    than all pairs must change at least one row (vacuous_ok: the cuts that by construction change nothing)."""
    want = masked_yardstick(e, blk, level, cuts)
    whole = want[-1][0].view(np.uint32)
    for c, w in zip(cuts, want):
        if c <= int(np.asarray(level).max()) and c not in vacuous_ok:
            assert (w[0].view(np.uint32) != whole).any(), "%s: the mask of cut %d changes no row" % (what, c)
    e.pair_curve_enable(level, cuts)
    check_variants(curve_outputs(e, blk), want, blk, what)
    return want


# ---- 1. the curve equals the masks -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_ladder(k, kind):
    """Rows of 0 .. 128 entries (erased ids and fields, descending fields, an id twice, a row count that is no
    multiple of 4; 128 entries are 8128 pairs, 32 batches of 256 terms), and blocks of 1, 5 and 0 rows."""
    blk = ladder_block()
    level = seeded_levels(ROW_FIELDS, 11, V6)
    assert len(np.unique(level)) > 6 and int(level.max()) < V6
    e = engine_of(kind, k, ladder_weights(k))
    check_curve(e, blk, level, LADDER_CUTS, "k=%d %s ladder" % (k, kind))
    lens = np.diff(blk.row_ptr)
    for rows in ([int(np.argmax(lens))], [int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33)], []):
        sub = take_rows(blk, rows)
        check_variants(curve_outputs(e, sub), masked_yardstick(e, sub, level, LADDER_CUTS), sub, "k=%d %s rows %r" % (k, kind, rows))
    e.close()


# ---- 2. one dropped pair equals pair ablation -------------------------------------------------------------

@pytest.mark.parametrize("kind", ["train", "f16"])
def test_one_dropped_pair_is_its_pair_ablation_variant(kind):
    k = 16
    blk = ladder_block()
    e = engine_of(kind, k, ladder_weights(k))
    e.pair_ablation_enable()
    ab, ab_loss = e.predict_pair_ablated(blk)
    ab_prob = e.predict_pair_ablated(blk, output_prob=True)[0]
    for last in (pair_index(ROW_FIELDS, 0, 0), pair_index(ROW_FIELDS, 1, 4), pair_index(ROW_FIELDS, 5, 5)):
        order = [v for v in range(V6) if v != last] + [last]
        level = pair_curve_levels(ROW_FIELDS, order)
        f, g = pair_fields(ROW_FIELDS, last)
        assert level[f, g] == level[g, f] == V6 - 1
        e.pair_curve_enable(level, [V6 - 1])
        lg, pr, ls = curve_outputs(e, blk)
        assert (ab[last].view(np.uint32) != ab[V6].view(np.uint32)).any(), "dropping pair %d changes no row" % last
        check_variants((lg, pr, ls), [(ab[last], ab_prob[last], ab_loss[last]), (ab[V6], ab_prob[V6], ab_loss[V6])], blk,
                       "%s without pair %r" % (kind, (f, g)))
    e.close()


# ---- 3. shapes where the kernel can go wrong ---------------------------------------------------------------

def regular_rows(F, per, n_rows, seed):
    rng = np.random.default_rng(seed)
    field = np.tile(np.arange(F, dtype=np.int32), n_rows)
    feat = (field.astype(np.int64) * per + rng.integers(0, per, field.size)).astype(np.int32)
    val = (rng.random(field.size) + 0.25).astype(np.float32)
    return Csr((np.arange(n_rows + 1) * F).astype(np.int32), field, feat, val, (np.arange(n_rows) % 2).astype(np.int32))


def test_39_fields_7_rows_three_batches():
    """39 fields x k = 16, one entry per field: 741 pairs are three batches of 256 terms (256 + 256 + 229), and 7 rows
    leave one wave of the second workgroup without a row."""
    F, k, per = 39, 16, 5
    o = CpuModel("oracle", "FFM", F * per, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(139), o)
    blk = regular_rows(F, per, 7, 39)
    assert blk.n_rows == 7 and (np.diff(blk.row_ptr) == 39).all()
    V = pair_count(F)
    level = pair_curve_levels(F, np.random.default_rng(39).permutation(V))
    for kind in KINDS:
        e = training(k, st, F * per, F, max_batch_rows=16) if kind == "train" else serving(k, kind, st, n_feats=F * per, n_fields=F, max_batch_rows=16)
        check_curve(e, blk, level, [0, 1, 39, 255, 256, 257, 512, 740, V], "39 fields %s" % kind)
        e.close()


def test_64_fields_64_cuts():
    """Lane 63 is live, lane 0 carries a cut and the whole row."""
    F, k, per = 64, 8, 3
    o = CpuModel("oracle", "FFM", F * per, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(164), o)
    blk = lanes_block(F, per, seed=64)
    V = pair_count(F)
    level = pair_curve_levels(F, np.random.default_rng(64).permutation(V))
    cuts = [int(c) for c in np.random.default_rng(65).permutation(np.round(np.arange(64) * V / 63.0).astype(np.int64))]
    assert len(cuts) == 64 and 0 in cuts and V in cuts and cuts[0] not in (0, V) and cuts[63] not in (0, V)
    e = training(k, st, F * per, F, max_batch_rows=16)
    want = check_curve(e, blk, level, cuts, "64 fields, 64 cuts")
    assert len({w[0].tobytes() for w in want}) >= 60, "the cuts' masks should give different rows"
    e.close()


def test_one_cut():
    k = 16
    blk = ladder_block()
    e = serving(k, "f32", ladder_weights(k))
    check_curve(e, blk, seeded_levels(ROW_FIELDS, 12, V6), [9], "n_cuts = 1")
    e.close()


def test_short_rows_long_row_erased_entries():
    """Rows of 0, 1 and 2 entries; a row of 128 entries with multi-valued fields (diagonal pairs, 8128 pairs); a row
    with an id >= n_feats and a field >= n_fields."""
    k = 8
    lad = ladder_block()
    lens = np.diff(lad.row_ptr)
    rows = [int(np.flatnonzero(lens == n)[0]) for n in (0, 1, 2, 128, 12)]
    blk = take_rows(lad, rows)
    field, feat = np.array(blk.field, np.int32), np.array(blk.feat, np.int32)
    lo = int(blk.row_ptr[4])  # the row of 12: two entries erased by hand
    feat[lo + 3] = NF
    field[lo + 7] = ROW_FIELDS
    blk = Csr(blk.row_ptr, field, feat, blk.val, blk.label)
    long_fields = field[int(blk.row_ptr[3]):int(blk.row_ptr[4])]
    assert long_fields.size == 128 and np.bincount(long_fields[(long_fields >= 0) & (long_fields < ROW_FIELDS)]).max() > 1
    e = training(k, ladder_weights(k))
    # (rows of 0 and 1 entries have no pair: no mask changes them, and the check below looks at the block)
    check_curve(e, blk, seeded_levels(ROW_FIELDS, 13, V6), [0, 5, 11, 20, 65536], "short, long and erased")
    e.close()


def test_level_65535():
    """A level of 65535 is dropped by cut 65535 and kept by cut 65536."""
    k = 16
    blk = ladder_block()
    level = seeded_levels(ROW_FIELDS, 14, 2) * np.uint16(65535)
    assert set(np.unique(level)) == {0, 65535}
    e = training(k, ladder_weights(k))
    want = check_curve(e, blk, level, [65535, 65536, 1, 0], "level 65535")
    assert (want[0][0].view(np.uint32) != want[1][0].view(np.uint32)).any(), "cut 65535 drops what cut 65536 keeps"
    assert_bitwise(want[1][0], want[4][0], "cut 65536 keeps all")
    assert_bitwise(want[0][0], want[2][0], "cut 65535 and cut 1 keep the level-0 pairs")
    e.close()


# ---- 4. a row too long -----------------------------------------------------------------------------------

def test_overlong_row_is_nan_in_every_variant():
    """max_row_nnz = 129 and one row of 129 entries: more than a wave stages.  That row is NaN in every variant, the
    others are what they are without it, and the call reports the row."""
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
    e = training(k, st, max_row_nnz=129)
    level = seeded_levels(ROW_FIELDS, 15, V6)
    cuts = [4, 0, 65536, 13]
    want = check_curve(e, base, level, cuts, "beside the long row")
    V = len(cuts) + 1
    lib = e.lib
    out = np.zeros((V, b.n_rows), np.float32)
    loss = np.zeros(V, np.float64)
    n, rp, fld, ft, v, lab = e._csr(b)
    rc = lib.ffm_engine_predict_pair_curve(e.h, n, rp, fld, ft, v, lab, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           loss.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == E_CAPACITY and "max_row_nnz" in lib.ffm_engine_last_error().decode()
    others = [r for r in range(b.n_rows) if r != at]
    assert np.isnan(out[:, at]).all() and np.isnan(loss).all()
    for c in range(V):
        assert_bitwise(out[c, others], want[c][0], "variant %d beside the long row" % c)
    e.sync()  # the report cleared the flag
    e.close()


# ---- 5. the device entry point ---------------------------------------------------------------------------

def test_device_entry_point_and_scores_false():
    k = 16
    b = ladder_block()
    e = serving(k, "f16", ladder_weights(k))
    e.pair_curve_enable(seeded_levels(ROW_FIELDS, 16, V6), LADDER_CUTS)
    V = len(LADDER_CUTS) + 1
    d = device_arrays(b)
    args = (b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
            d["label"].data_ptr())
    for prob in (False, True):
        want, wl = e.predict_pair_curve(b, output_prob=prob)
        assert (wl != 0).all()
        out = torch.full((V * b.n_rows,), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.full((V,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.predict_pair_curve_device(*args, prob, out.data_ptr(), loss.data_ptr())
        e.sync()
        assert_bitwise(out.cpu().numpy().reshape(V, b.n_rows), want, "predict_pair_curve_device prob=%d" % prob)
        assert np.array_equal(loss.cpu().numpy(), wl)
        # loss sums only: the scores stay in the engine's scratch
        loss.fill_(float("nan"))
        torch.cuda.synchronize()
        e.predict_pair_curve_device(*args, prob, None, loss.data_ptr())
        e.sync()
        assert np.array_equal(loss.cpu().numpy(), wl)
        none, got = e.predict_pair_curve(b, output_prob=prob, scores=False)
        assert none is None and np.array_equal(got, wl)
    assert not e.predict_pair_curve(b, with_loss=False, scores=False)[1].any()
    e.close()


# ---- 6. the histograms -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prob", [False, True])
def test_auc_per_variant(prob):
    """After two blocks pair_curve_metrics()[c] is fa.metrics_from_histogram of the numpy histogram of that variant's
    probabilities (themselves pinned to the masks above); collection that stays on keeps its counts; reset zeroes."""
    k = 16
    blocks = [ladder_block(3), ladder_block(4)]
    level = seeded_levels(ROW_FIELDS, 17, V6)
    e = training(k, ladder_weights(k))
    e.pair_curve_enable(level, LADDER_CUTS, auc=True)
    V = len(LADDER_CUTS) + 1
    pos, neg, n_nan = np.zeros((V, fa.METRIC_BINS), np.uint64), np.zeros((V, fa.METRIC_BINS), np.uint64), [0] * V
    for b in blocks:
        assert (b.label > 0).any() and (b.label <= 0).any()
        e.predict_pair_curve(b, output_prob=prob)
        e.pair_curve_enable(level, LADDER_CUTS, auc=True)  # (stays on: keeps its counts)
    got = e.pair_curve_metrics()
    assert len(got) == V
    e2 = training(k, ladder_weights(k))  # the probabilities, from an engine whose histograms are not the ones under test
    e2.pair_curve_enable(level, LADDER_CUTS)
    for b in blocks:
        pr = e2.predict_pair_curve(b, output_prob=True)[0]
        for c in range(V):
            p, n, nn = numpy_histogram(pr[c], b.label)
            pos[c], neg[c], n_nan[c] = pos[c] + p, neg[c] + n, n_nan[c] + nn
    e2.close()
    for c in range(V):
        want = fa.metrics_from_histogram(pos[c], neg[c], n_nan[c])
        assert got[c] == want, (c, got[c], want)
        assert want["n_pos"] + want["n_neg"] == sum(b.n_rows for b in blocks)
    assert got[2] == got[5], "the duplicate cut has the same histogram"
    assert len({m["auc"] for m in got}) > 1, "the variants' AUCs should not all coincide on these weights"
    assert e.pair_curve_metrics(reset=True) == got
    for m in e.pair_curve_metrics():
        assert m["n_pos"] == 0 and m["n_neg"] == 0 and m["n_nan"] == 0
    e.close()


# ---- 7. state and refusals -------------------------------------------------------------------------------

def code_of(call):
    with pytest.raises(fa.EngineError) as ei:
        call()
    return ei.value.code, str(ei.value)


def test_reenable_and_refused_enables():
    k = 16
    b = ladder_block()
    e = training(k, ladder_weights(k))
    before = e.get_state()
    level = seeded_levels(ROW_FIELDS, 18, V6)
    check_curve(e, b, level, LADDER_CUTS, "first table")
    other = seeded_levels(ROW_FIELDS, 19, 300)
    check_curve(e, b, other, [150, 0, 299], "another table, another n_cuts")
    check_curve(e, b, level, [5, 65536, 2, 9, 14, 1, 20, 3], "the first table again, more cuts")
    want = masked_yardstick(e, b, level, [5, 65536, 2, 9, 14, 1, 20, 3])
    lopsided = level.copy()
    lopsided[1, 4] ^= 1
    for what, call in (("symmetric", lambda: e.pair_curve_enable(lopsided, [3])),
                       ("n_cuts", lambda: e.pair_curve_enable(other, [])),
                       ("n_cuts", lambda: e.pair_curve_enable(other, list(range(65)))),
                       ("65537", lambda: e.pair_curve_enable(other, [3, 65537])),
                       ("-1", lambda: e.pair_curve_enable(other, [-1])),
                       ("7 fields", lambda: e.pair_curve_enable(seeded_levels(ROW_FIELDS + 1, 1, 9), [3])),
                       ("5 fields", lambda: e.pair_curve_enable(seeded_levels(ROW_FIELDS - 1, 1, 9), [3]))):
        code, msg = code_of(call)
        assert code == E_INVALID and what in msg, (what, msg)
        check_variants(curve_outputs(e, b), want, b, "after a refused enable (%s)" % what)
    # refused while a mask is set, and back once it is gone
    e.set_pair_mask(pair_curve_mask(level, 9))
    for name, call in (("predict_pair_curve", lambda: e.predict_pair_curve(b)),
                       ("predict_pair_curve_device", lambda: e.predict_pair_curve_device(0, 0, None, None, None, None, None, 0, None))):
        code, msg = code_of(call)
        assert code == E_INVALID and "pair mask" in msg, (name, msg)
    e.set_pair_mask(None)
    check_variants(curve_outputs(e, b), want, b, "after clearing the mask")
    assert e.blocks_pulled() == 0
    assert_state_bitwise(e.get_state(), before, "a training engine's state after the curve's calls")
    e.close()


def test_unsupported_engines_and_off():
    b = ladder_block()
    for what, e in (("LR", fa.Engine("LR", 64, 1, 1, max_batch_rows=16)), ("FM", fa.Engine("FM", 64, 1, 4, max_batch_rows=16)),
                    ("n_fields = 65", fa.Engine("FFM", 130, 65, 4, max_batch_rows=16)),
                    ("n_factors = 12", fa.Engine("FFM", 64, 4, 12, max_batch_rows=16))):
        F = e.n_fields
        code, msg = code_of(lambda: e.pair_curve_enable(np.zeros((F, F), np.uint16), [1]))
        assert code == E_UNSUPPORTED and "pruning curve" in msg, (what, msg)
        code, msg = code_of(lambda: e.predict_pair_curve(b))
        assert code == E_INVALID and "pair_curve_enable" in msg, (what, msg)
        e.close()
    k = 16
    e = training(k, ladder_weights(k))
    e.pair_ablation_enable()  # (pair ablation being on does not turn the curve on)
    code, msg = code_of(lambda: e.predict_pair_curve(b))
    assert code == E_INVALID and "pair_curve_enable" in msg
    assert code_of(e.pair_curve_metrics)[0] == E_INVALID
    n, rp, fld, ft, v, lab = e._csr(b)
    assert e.lib.ffm_engine_predict_pair_curve(e.h, n, rp, fld, ft, v, lab, 0, None, None) == E_INVALID
    assert "ffm_engine_pair_curve_enable" in e.lib.ffm_engine_last_error().decode()
    e.pair_curve_enable(seeded_levels(ROW_FIELDS, 20, V6), [4])
    code, msg = code_of(e.pair_curve_metrics)
    assert code == E_INVALID and "with_auc" in msg
    e.close()


def test_failed_histogram_allocation_leaves_the_engine_as_it_was(monkeypatch):
    """FFM_CURVE_HIST_FAIL=1 makes the histograms' allocation fail as an exhausted device does (the library's test
    hook): a first enable(auc=True) is FFM_E_NOMEM and the curve stays off with what the call made given back; on an
    engine that is on, the failure -- with the same or another n_cuts -- leaves table, cuts and results as they were."""
    k = 16
    b = ladder_block()
    level, other = seeded_levels(ROW_FIELDS, 21, V6), seeded_levels(ROW_FIELDS, 22, V6)
    rows = 1 << 16  # (7 variants x 65536 rows x 12 bytes = 5.5 MB of scratch: visible in the device's free memory)
    e = training(k, ladder_weights(k), max_batch_rows=rows)
    e.sync()
    free_before = torch.cuda.mem_get_info()[0]
    monkeypatch.setenv("FFM_CURVE_HIST_FAIL", "1")
    code, msg = code_of(lambda: e.pair_curve_enable(level, LADDER_CUTS, auc=True))
    assert code == E_NOMEM and "bytes failed" in msg, msg
    assert torch.cuda.mem_get_info()[0] >= free_before - (2 << 20), "what the call made before the failure was given back"
    n, rp, fld, ft, v, lab = e._csr(b)
    assert e.lib.ffm_engine_predict_pair_curve(e.h, n, rp, fld, ft, v, lab, 0, None, None) == E_INVALID
    want = check_curve(e, b, level, LADDER_CUTS, "on, after a failed enable")  # (no histograms asked for: nothing to fail)
    for cuts in (LADDER_CUTS, [1, 2, 3]):
        assert code_of(lambda: e.pair_curve_enable(other, cuts, auc=True))[0] == E_NOMEM
        code, msg = code_of(e.pair_curve_metrics)
        assert code == E_INVALID and "with_auc" in msg
        check_variants(curve_outputs(e, b), want, b, "still the first table and cuts")
    monkeypatch.delenv("FFM_CURVE_HIST_FAIL")
    e.pair_curve_enable(level, LADDER_CUTS, auc=True)
    e.predict_pair_curve(b)
    counts = lambda m: (m["n_pos"], m["n_neg"], m["n_nan"])  # noqa: E731
    counted = counts(e.pair_curve_metrics()[len(LADDER_CUTS)])
    assert counted[0] + counted[1] == b.n_rows and counted[2] == 0
    e.pair_curve_enable(other, [1, 2, 3], auc=True)  # another n_cuts: the histograms start from zero
    assert [counts(m) for m in e.pair_curve_metrics()] == [(0, 0, 0)] * 4
    e.close()
