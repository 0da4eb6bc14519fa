"""Field ablation (include/ffm_engine.h "Field ablation"; csrc/kernels_ablate.h, csrc/engine_ablate.h): the
n_fields + 1 variants of every row from one pass.

The expected value everywhere is oracle.pyoracle.CpuModel.predict_batch(drop_field(blk, v)) with the oracle
holding the engine's weights (decoded for fp16 as test_gpu_serve.decoded does): logits and probabilities bit
for bit (NaN with NaN), double loss sums by util.loss_close.  Nothing else here has a tolerance."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import drop_field
from oracle.pyoracle import CpuModel, Csr
from test_gpu_serve import MAX_ROWS, NF, decoded, ladder_block, ladder_weights, oracle_with, serving
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, loss_close, rand_state, take_rows

pytestmark = pytest.mark.gpu

KINDS = ("train", "f32", "f16")  # a training engine, the two serving formats
BINS = fa.METRIC_BINS
E_INVALID, E_CAPACITY, E_UNSUPPORTED = fa.engine.E_INVALID, fa.engine.E_CAPACITY, fa.engine.E_UNSUPPORTED


def training(k, st, n_feats=NF, n_fields=ROW_FIELDS, **kw):
    kw.setdefault("max_batch_rows", MAX_ROWS)
    e = fa.Engine("FFM", n_feats, n_fields, k, skip_init=True, **dict(STRESS_HP, **kw))
    e.set_state({key: st[key] for key in st})
    return e


def engine_of(kind, k, st, **kw):
    return training(k, st, **kw) if kind == "train" else serving(k, kind, st, **kw)


def variants(blk, n_fields):
    """The blocks whose predict_batch is the definition: drop_field(blk, v) for every field, then blk."""
    return [drop_field(blk, v) for v in range(n_fields)] + [blk]


@functools.lru_cache(maxsize=None)
def ladder_expected(k, fmt, rows=None):
    """(logits, probabilities, loss sums) of the 7 variants of the ladder block (or of its rows `rows`) under
    the oracle that holds the ladder weights as an engine of format `fmt` does.  Read-only."""
    st = ladder_weights(k)
    blk = ladder_block() if rows is None else take_rows(ladder_block(), list(rows))
    o = oracle_with(k, st["bias3"][0], st["lin_w"], decoded(st["vec_w"], fmt))
    lg, pr, ls = [], [], []
    for b in variants(blk, ROW_FIELDS):
        a, l = o.predict_batch(b)
        lg.append(a)
        ls.append(l)
        pr.append(o.predict_batch(b, output_prob=True)[0])
    out = np.stack(lg), np.stack(pr), np.array(ls)
    for a in out:
        a.setflags(write=False)
    return out


def check_ablated(e, blk, want, what):
    lg, pr, ls = want
    for prob, exp in ((False, lg), (True, pr)):
        got, gl = e.predict_ablated(blk, output_prob=prob)
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
    multiple of 4; 128 entries are 8128 pairs, many 256-term batches), and blocks of 1, 5 and 0 rows: all 7
    variants, logits and probabilities, bit for bit; loss sums by loss_close."""
    blk = ladder_block()
    fmt = "f16" if kind == "f16" else "f32"  # (a training engine and an fp32 serving engine hold the same bits)
    e = engine_of(kind, k, ladder_weights(k))
    e.ablation_enable()
    check_ablated(e, blk, ladder_expected(k, fmt), "k=%d %s ladder" % (k, kind))
    lens = np.diff(blk.row_ptr)
    longest = int(np.argmax(lens))
    check_ablated(e, take_rows(blk, [longest]), ladder_expected(k, fmt, (longest,)), "k=%d %s one row of %d" % (k, kind, lens[longest]))
    five = tuple(int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33))
    check_ablated(e, take_rows(blk, list(five)), ladder_expected(k, fmt, five), "k=%d %s five rows" % (k, kind))
    check_ablated(e, take_rows(blk, []), ladder_expected(k, fmt, ()), "k=%d %s no rows" % (k, kind))
    e.close()


# ---- 2. every lane ---------------------------------------------------------------------------------------

def lanes_block(F, per, seed):
    """9 regular rows (one entry per field, in field order), 3 rows that lack fields (every third, the first
    half, all but the last), one row with two entries of the last field."""
    rng = np.random.default_rng(seed)
    rows = [list(range(F)) for _ in range(9)]
    rows += [[f for f in range(F) if f % 3 != 1], list(range(F // 2)), list(range(F - 1))]
    rows += [list(range(F)) + [F - 1]]
    field = np.concatenate([np.asarray(r, np.int32) for r in rows])
    feat = (field.astype(np.int64) * per + rng.integers(0, per, field.size)).astype(np.int32)
    twice = len(field) - 1  # (the second entry of the last field: another id of its range)
    feat[twice] = field[twice] * per + (feat[twice - 1] - field[twice] * per + 1) % per
    val = (rng.random(field.size) + 0.25).astype(np.float32)
    val[rng.random(field.size) < 0.5] = 1.0
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    label = (np.arange(len(rows)) % 3 == 0).astype(np.int32)
    return Csr(row_ptr, field, feat, val, label)


@pytest.mark.parametrize("F", [64, 39])
def test_every_lane(F):
    """One lane per variant: n_fields = 64 fills the wave (and lane 0 carries two variants), 39 is the headline
    shape.  Variants 0, 31, 32, F - 2, F - 1 and F against the oracle, every other one against a twin engine's
    predict_batch of the dropped block."""
    k, per = 16, 50
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(7 + F), o)
    o.set_state(st)
    blk = lanes_block(F, per, seed=F)
    assert blk.n_rows == 13 and int(np.diff(blk.row_ptr).max()) == F + 1
    e, twin = training(k, st, nf, F, max_batch_rows=16), training(k, st, nf, F, max_batch_rows=16)
    e.ablation_enable()
    with_oracle = {0, 31, 32, F - 2, F - 1, F}
    for prob in (False, True):
        got, gl = e.predict_ablated(blk, output_prob=prob)
        assert got.shape == (F + 1, blk.n_rows)
        for v, b in enumerate(variants(blk, F)):
            want, wl = (o if v in with_oracle else twin).predict_batch(b, output_prob=prob)
            assert_rows_bitwise(got[v], want, blk, "F=%d variant %d prob=%d" % (F, v, prob))
            assert loss_close(gl[v], wl), (F, v, gl[v], wl)
    # a row without field v: variant v is variant n_fields, bit for bit
    got = e.predict_ablated(blk)[0]
    lacking = blk.n_rows - 3  # (the row of the first half of the fields)
    for v in range(F // 2, F):
        assert got[v, lacking].view(np.uint32) == got[F, lacking].view(np.uint32), v
    e.close()
    twin.close()


# ---- 3. the other ways in --------------------------------------------------------------------------------

def test_device_entry_point_gives_the_host_call_bits():
    k = 16
    e = serving(k, "f16", ladder_weights(k))
    e.ablation_enable()
    b = ladder_block()
    V = ROW_FIELDS + 1
    d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
    for prob in (False, True):
        want, wl = e.predict_ablated(b, output_prob=prob)
        out = torch.full((V * b.n_rows,), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.full((V,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.predict_ablated_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                                 d["val"].data_ptr(), d["label"].data_ptr(), prob, out.data_ptr(), loss.data_ptr())
        e.sync()
        assert_bitwise(out.cpu().numpy().reshape(V, b.n_rows), want, "predict_ablated_device prob=%d" % prob)
        assert np.array_equal(loss.cpu().numpy(), wl)
    e.close()


def test_rows_without_values_and_hashed_ids():
    """val=None gives the bits of numpy.ones; a hash_ids=True engine on raw ids gives the bits of a plain engine
    on fa.hash_ids ids (fields are not touched by hashing)."""
    k = 8
    st, b = ladder_weights(k), ladder_block()
    e = training(k, st)
    e.ablation_enable()
    ones = Csr(b.row_ptr, b.field, b.feat, np.ones(b.feat.size, np.float32), b.label)
    none = Csr(b.row_ptr, b.field, b.feat, None, b.label)
    for prob in (False, True):
        a, la = e.predict_ablated(ones, output_prob=prob)
        c, lc = e.predict_ablated(none, output_prob=prob)
        assert_bitwise(c, a, "val=None prob=%d" % prob)
        assert np.array_equal(la, lc)
    fs = (np.arange(ROW_FIELDS + 1) * ROW_IDS_PER_FIELD).astype(np.int32)
    h = training(k, st, hash_ids=True, field_start=fs)
    h.ablation_enable()
    rng = np.random.default_rng(8)
    fld = np.clip(b.field, 0, ROW_FIELDS - 1)  # (hashing needs a field in range for every entry)
    raw = Csr(b.row_ptr, fld, rng.integers(0, 2 ** 31 - 1, b.feat.size).astype(np.int32), b.val, b.label)
    hashed = Csr(b.row_ptr, fld, fa.hash_ids(fld, raw.feat, NF, fs), b.val, b.label)
    a, la = h.predict_ablated(raw)
    c, lc = e.predict_ablated(hashed)
    assert_bitwise(a, c, "hash_ids")
    assert np.array_equal(la, lc)
    h.close()
    e.close()


# ---- 4. the histograms -----------------------------------------------------------------------------------

def numpy_histogram(p, label):
    p, label = np.asarray(p, np.float32), np.asarray(label)
    ok = ~np.isnan(p)
    b = np.minimum((p[ok] * np.float32(1048576.0)).astype(np.int64), BINS - 1)
    y = label[ok] > 0
    return (np.bincount(b[y], minlength=BINS).astype(np.uint64), np.bincount(b[~y], minlength=BINS).astype(np.uint64),
            int((~ok).sum()))


@pytest.mark.parametrize("prob", [False, True])
def test_auc_per_variant(prob):
    """After two blocks ablation_metrics()[v] is fa.metrics_from_histogram of the numpy histogram of the oracle's
    probabilities for drop_field(., v): the integers and auc exactly; reset zeroes them."""
    k = 16
    st = ladder_weights(k)
    blocks = [ladder_block(3), ladder_block(4)]
    for b in blocks:  # the input condition: both classes in both blocks
        assert (b.label > 0).any() and (b.label <= 0).any()
    o = oracle_with(k, st["bias3"][0], st["lin_w"], st["vec_w"])
    e = training(k, st)
    e.ablation_enable(auc=True)
    for b in blocks:
        e.predict_ablated(b, output_prob=prob)
    got = e.ablation_metrics()
    assert len(got) == ROW_FIELDS + 1
    for v in range(ROW_FIELDS + 1):
        pos, neg, n_nan = np.zeros(BINS, np.uint64), np.zeros(BINS, np.uint64), 0
        for b in blocks:
            p, n, nn = numpy_histogram(o.predict_batch(variants(b, ROW_FIELDS)[v], output_prob=True)[0], b.label)
            pos, neg, n_nan = pos + p, neg + n, n_nan + nn
        want = fa.metrics_from_histogram(pos, neg, n_nan)
        assert got[v] == want, (v, got[v], want)
        assert want["n_pos"] + want["n_neg"] == sum(b.n_rows for b in blocks)
    aucs = {m["auc"] for m in got}
    assert len(aucs) > 1, "the variants' AUCs should not all coincide on these weights"
    assert e.ablation_metrics(reset=True) == got
    for m in e.ablation_metrics():
        assert m["n_pos"] == 0 and m["n_neg"] == 0 and m["n_nan"] == 0
    e.close()


def test_channels_untouched():
    """With the eval channel and keyed capture on, predict_ablated changes neither."""
    k = 16
    b = ladder_block()
    e = training(k, ladder_weights(k))
    e.metrics_enable(eval=True)
    e.metrics_key_field(0, 1000, eval=True)
    e.ablation_enable(auc=True)
    e.predict_batch(b)
    before, keyed_before = e.metrics("eval"), e.metrics_read_keyed("eval")
    assert before["n_pos"] + before["n_neg"] == b.n_rows
    e.predict_ablated(b)
    e.predict_ablated(b, output_prob=True)
    assert e.metrics("eval") == before
    assert e.metrics_read_keyed("eval") == keyed_before
    assert e.ablation_metrics()[ROW_FIELDS]["n_pos"] == 2 * before["n_pos"]
    e.close()


# ---- 5. rows too long, refusals --------------------------------------------------------------------------

def test_overlong_row_is_nan_in_every_variant():
    """A training engine with max_row_nnz = 150 and one row of 129 entries: more than a wave stages.  That row is
    NaN in every variant, every other row is right, and sync reports the row (FFM_E_CAPACITY)."""
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
    o = oracle_with(k, st["bias3"][0], st["lin_w"], st["vec_w"])
    e = training(k, st, max_row_nnz=150)
    e.ablation_enable()
    V = ROW_FIELDS + 1
    d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
    out = torch.zeros((V * b.n_rows,), dtype=torch.float32, device="cuda")
    loss = torch.zeros((V,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.predict_ablated_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                             d["val"].data_ptr(), d["label"].data_ptr(), False, out.data_ptr(), loss.data_ptr())
    with pytest.raises(fa.EngineError) as ei:
        e.sync()
    assert ei.value.code == E_CAPACITY and "max_row_nnz" in str(ei.value)
    got = out.cpu().numpy().reshape(V, b.n_rows)
    others = [r for r in range(b.n_rows) if r != at]
    for v, bv in enumerate(variants(b, ROW_FIELDS)):
        assert np.isnan(got[v, at]), v
        want = o.predict_batch(bv)[0]
        assert_bitwise(got[v, others], want[others], "variant %d beside the long row" % v)
    assert np.isnan(loss.cpu().numpy()).all()
    e.sync()  # the report cleared the flag
    with pytest.raises(fa.EngineError) as ei:  # the host call reports it itself
        e.predict_ablated(b)
    assert ei.value.code == E_CAPACITY
    e.close()


def code_of(call):
    with pytest.raises(fa.EngineError) as ei:
        call()
    return ei.value.code, str(ei.value)


def test_failed_histogram_allocation_leaves_the_engine_as_it_was(monkeypatch):
    """FFM_FIELD_HIST_FAIL=1 makes the histograms' allocation fail as an exhausted device does (the library's test
    hook).  A first enable(auc=True) then is FFM_E_NOMEM, field ablation stays off and the scratch the call had made
    is given back; on an engine that is already on, the same failure leaves it on without histograms and its
    results unchanged.  Then with_auc on later calls: 0 stops the collection, 1 starts it from zero."""
    k = 16
    lens = np.diff(ladder_block().row_ptr)
    five = tuple(int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33))  # (test_ladder's five rows)
    b = take_rows(ladder_block(), list(five))
    want = ladder_expected(k, "f32", five)
    rows = 1 << 16  # (7 variants x 65536 rows x 12 bytes = 5.5 MB of scratch: visible in the device's free memory)
    E_NOMEM = fa.engine.E_NOMEM
    e = training(k, ladder_weights(k), max_batch_rows=rows)
    e.sync()
    free_before = torch.cuda.mem_get_info()[0]
    monkeypatch.setenv("FFM_FIELD_HIST_FAIL", "1")
    code, msg = code_of(lambda: e.ablation_enable(auc=True))
    assert code == E_NOMEM and "bytes failed" in msg, msg
    assert torch.cuda.mem_get_info()[0] >= free_before - (4 << 20), "the scratch made before the failure was given back"
    code, msg = code_of(lambda: e.predict_ablated(b))
    assert code == E_INVALID and "ablation_enable" in msg
    e.ablation_enable()  # (no histograms asked for: nothing to fail)
    check_ablated(e, b, want, "on, after a failed enable")
    code, msg = code_of(lambda: e.ablation_enable(auc=True))
    assert code == E_NOMEM
    code, msg = code_of(e.ablation_metrics)
    assert code == E_INVALID and "with_auc" in msg
    check_ablated(e, b, want, "still on without histograms")
    monkeypatch.delenv("FFM_FIELD_HIST_FAIL")
    e.ablation_enable(auc=True)
    e.predict_ablated(b)
    counts = lambda m: (m["n_pos"], m["n_neg"], m["n_nan"])  # noqa: E731
    counted = counts(e.ablation_metrics()[ROW_FIELDS])
    assert counted[0] + counted[1] == b.n_rows and counted[2] == 0
    e.ablation_enable(auc=True)  # collection that stays on keeps its counts
    assert counts(e.ablation_metrics()[ROW_FIELDS]) == counted
    e.ablation_enable(auc=False)  # stops it
    assert code_of(e.ablation_metrics)[0] == E_INVALID
    e.predict_ablated(b)
    e.ablation_enable(auc=True)  # and a later one starts from zero
    assert counts(e.ablation_metrics()[ROW_FIELDS]) == (0, 0, 0)
    check_ablated(e, b, want, "after the switches")
    e.close()


def test_refusals():
    b = ladder_block()
    for what, e in (("LR", fa.Engine("LR", 64, 1, 1, max_batch_rows=16)), ("FM", fa.Engine("FM", 64, 1, 4, max_batch_rows=16)),
                    ("n_fields = 65", fa.Engine("FFM", 130, 65, 4, max_batch_rows=16)),
                    ("n_factors = 12", fa.Engine("FFM", 64, 4, 12, max_batch_rows=16)),
                    ("a shard", fa.Engine("FFM", 64, 4, 4, max_batch_rows=16, n_shards=2, shard_rank=0))):
        code, msg = code_of(e.ablation_enable)
        assert code == E_UNSUPPORTED and "field ablation" in msg, (what, msg)
        code, msg = code_of(lambda: e.predict_ablated(b))
        assert code == E_INVALID and "ablation_enable" in msg, (what, msg)
        e.close()
    k = 16
    e = training(k, ladder_weights(k))
    code, msg = code_of(lambda: e.predict_ablated(b))
    assert code == E_INVALID and "ablation_enable" in msg
    assert code_of(e.ablation_metrics)[0] == E_INVALID
    e.ablation_enable()
    code, msg = code_of(e.ablation_metrics)
    assert code == E_INVALID and "with_auc" in msg
    # field == NULL stays refused on this synchronous call
    assert code_of(lambda: e.predict_ablated(Csr(b.row_ptr, None, b.feat, b.val, b.label)))[0] == E_INVALID
    # and the engine goes on working
    want = ladder_expected(k, "f32")
    assert_bitwise(e.predict_ablated(b)[0], want[0], "after the refusals")
    e.close()
