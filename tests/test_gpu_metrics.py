"""AUC accumulated on the device (include/ffm_engine.h "Metrics"): metric_hist_kernel's histogram of
p = sigmoid(logit) in 2^20 bins per class, count for count against numpy over the oracle's sigmoid, on
every labelled predict entry point (eval channel) and every training path (train channel: the
pre-update logits), for a group, with NaN scores, and the bound the histogram AUC promises on the exact
rank AUC.  Small models throughout: FFM 5 fields x k 4 over 97 features, FM k 8 over 33, LR over 65.
FFM_ENGINE_METRICS=<mask> turns the channels on at create."""
import copy
import ctypes
import math
import re
from fractions import Fraction

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise, rand_state

pytestmark = pytest.mark.gpu

BINS = fa.METRIC_BINS
FFM_FIELD_START = np.array([0, 20, 40, 60, 80, 97], np.int32)
MODELS = {"FFM": ("FFM", 97, 5, 4), "FM": ("FM", 33, 1, 8), "LR": ("LR", 65, 1, 1)}
MAX_ROWS = 1024
ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


# ---- shared helpers -------------------------------------------------------------------------

def bins_of(p):
    """bin(p) = min((int)(p * 2^20), 2^20 - 1) of float32 probabilities (no NaN among them)."""
    p = np.asarray(p, np.float32)
    return np.minimum((p * np.float32(1048576.0)).astype(np.int64), BINS - 1)


def want_hist(p, label):
    """(pos, neg, n_nan) the channel must hold after these rows."""
    p, label = np.asarray(p, np.float32), np.asarray(label)
    ok = ~np.isnan(p)
    b = bins_of(p[ok])
    y = label[ok] > 0
    return (np.bincount(b[y], minlength=BINS).astype(np.uint64), np.bincount(b[~y], minlength=BINS).astype(np.uint64),
            int((~ok).sum()))


_scalar_oracle = []


def _sig():
    """The oracle's scalar helpers (CpuModel.sigmoid), made on first use: the checker is built by then."""
    if not _scalar_oracle:
        _scalar_oracle.append(CpuModel("oracle", "LR", 1))
    return _scalar_oracle[0]


def oracle_sigmoid(x):
    sig = _sig().sigmoid
    return np.array([sig(float(v)) for v in np.asarray(x, np.float32)], np.float32)


def assert_hist(e, channel, want, what):
    pos, neg = e.metrics_histogram(channel)
    wp, wn, wnan = want
    for name, got, exp in (("pos", pos, wp), ("neg", neg, wn)):
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, "%s: %s differs in %d bins, first bin %d: %d, expected %d" % (
            what, name, bad.size, bad[0], got[bad[0]], exp[bad[0]])
    m = e.metrics(channel)
    assert (m["n_pos"], m["n_neg"], m["n_nan"]) == (int(wp.sum()), int(wn.sum()), wnan), (what, m)


def add_hist(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


EMPTY = (np.zeros(BINS, np.uint64), np.zeros(BINS, np.uint64), 0)


def restart(e, eval=False, train=False):
    """The named channels on and at zero (a channel that turns on starts from zero)."""
    e.metrics_enable()
    e.metrics_enable(eval=eval, train=train)


def make_block(name, n_rows, seed):
    """Rows of one entry per field in field order (FFM: ids from the field's range; FM / LR: five
    distinct ids, field 0), values 1.0 or uniform, four labels in ten positive."""
    mt, nf, F, _ = MODELS[name]
    rng = np.random.default_rng(seed)
    if mt == "FFM":
        lo, hi = FFM_FIELD_START[:-1], FFM_FIELD_START[1:]
        feat = (lo[None, :] + (rng.random((n_rows, F)) * (hi - lo)[None, :]).astype(np.int64)).astype(np.int32)
        field = np.broadcast_to(np.arange(F, dtype=np.int32), (n_rows, F)).copy()
    else:
        feat = np.stack([rng.choice(nf, 5, replace=False) for _ in range(n_rows)]).astype(np.int32).reshape(n_rows, 5)
        field = np.zeros((n_rows, 5), np.int32)
    per = feat.shape[1] if n_rows else (F if mt == "FFM" else 5)
    val = (rng.random((n_rows, per)) + 0.25).astype(np.float32)
    val[rng.random((n_rows, per)) < 0.5] = 1.0
    label = (rng.random(n_rows) < 0.4).astype(np.int32)
    row_ptr = (np.arange(n_rows + 1, dtype=np.int64) * per).astype(np.int32)
    return Csr(row_ptr, field.reshape(-1), feat.reshape(-1), val.reshape(-1), label)


def make_pair(name, seed=3, learn=False, state=None, **kw):
    """(oracle, engine) of one small model holding the same random state."""
    mt, nf, F, k = MODELS[name]
    o = CpuModel("oracle", mt, nf, F, k, learn=learn, **STRESS_HP)
    st = rand_state(np.random.default_rng(seed), o) if state is None else state
    o.set_state(st)
    return o, make_engine(name, st, learn=learn, **kw), st


def make_engine(name, st, learn=False, **kw):
    mt, nf, F, k = MODELS[name]
    e = fa.Engine(mt, nf, F, k, skip_init=True, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 8, learn=learn,
                  **STRESS_HP, **kw)
    e.set_state(st)
    return e


class DeviceBlock:
    """The block's arrays in HBM (torch tensors), for the *_device entry points."""

    def __init__(self, c):
        self.n_rows, self.nnz = c.n_rows, int(c.row_ptr[-1])
        self.t = {k: torch.from_numpy(np.ascontiguousarray(getattr(c, k))).cuda()
                  for k in ("row_ptr", "field", "feat", "val", "label")}
        torch.cuda.synchronize()

    def args(self):
        return [self.n_rows, self.nnz] + [self.t[k].data_ptr() for k in ("row_ptr", "field", "feat", "val", "label")]


def pinned(c):
    """A copy of the block whose arrays are page-locked (kept alive on the copy)."""
    d = copy.copy(c)
    d.__dict__.pop("_ffm_csr_args", None)
    d._pins = []
    for k in ("row_ptr", "field", "feat", "val", "label"):
        a = getattr(c, k)
        if a is None:
            continue
        t = torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
        d._pins.append(t)
        setattr(d, k, t.numpy())
    return d


def without_field_array(c):
    d = copy.copy(c)
    d.__dict__.pop("_ffm_csr_args", None)
    d.field = None
    return d


# ---- 1. the kernel's edges, through predict_finish_device with crafted logits ----------------

def _nan(sign):
    return np.array([0xffc00000 if sign else 0x7fc00000], np.uint32).view(np.float32)[0]


def crafted_logits(pattern, n):
    """(logits, labels) of n rows."""
    rng = np.random.default_rng(1000 + n)
    if pattern == "one_bin":  # every row in one bin, labels alternating: the key is (bin, class)
        return np.full(n, 0.3, np.float32), (np.arange(n) % 2).astype(np.int32)
    if pattern == "distinct":  # every lane of a wave in a bin of its own
        lg = np.linspace(-4.0, 4.0, max(n, 2), dtype=np.float32)[:n]
        return lg, (rng.random(n) < 0.5).astype(np.int32)
    if pattern == "special":
        f = np.float32
        pool = np.array([np.inf, -np.inf, 0.0, -0.0, 200.0, -200.0, _nan(0), _nan(1), 88.0, -80.0, 17.0, -104.0, 1e-30,
                         0.25, 0.25, -3.0], f)
        lg = pool[(np.arange(n) * 7 + rng.integers(0, 3, n)) % pool.size]
        return lg, (rng.random(n) < 0.5).astype(np.int32)
    assert pattern == "runs"  # runs of equal scores of random lengths and labels, a wave's keys repeating
    vals = rng.normal(0, 2.5, 40).astype(np.float32)
    return vals[rng.integers(0, vals.size, n)], rng.integers(-1, 3, n).astype(np.int32)  # (labels -1 .. 2: positive iff > 0)


@pytest.fixture(scope="module")
def edge_engine():
    _, e, _ = make_pair("FFM")
    e.metrics_enable(eval=True)
    yield e
    e.close()


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("pattern", ["one_bin", "distinct", "special", "runs"])
def test_kernel_edges_through_predict_finish(edge_engine, n, pattern):
    e = edge_engine
    lg, label = crafted_logits(pattern, n)
    p = oracle_sigmoid(lg)
    want = want_hist(p, label)
    if pattern == "distinct" and n:
        b = bins_of(p)
        for w0 in range(0, n, 64):
            assert np.unique(b[w0:w0 + 64]).size == b[w0:w0 + 64].size
    if pattern == "one_bin" and n:
        assert np.unique(bins_of(p)).size == 1
    if pattern == "special" and n >= 63:
        assert want[2] > 0 and want[0][BINS - 1] + want[1][BINS - 1] > 0 and want[0][0] + want[1][0] > 0
    d_label = torch.from_numpy(label).cuda()
    for output_prob in (0, 1):
        for mode in ("null", "separate", "alias"):
            d_logit = torch.from_numpy(lg.copy()).cuda()
            d_out = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            out_ptr = {"null": None, "separate": d_out.data_ptr(), "alias": d_logit.data_ptr()}[mode]
            restart(e, eval=True)
            e.predict_finish_device(n, d_logit.data_ptr(), d_label.data_ptr(), output_prob, out_ptr)
            e.sync()
            assert_hist(e, "eval", want, "%s n=%d output_prob=%d out=%s" % (pattern, n, output_prob, mode))
            if mode != "null" and n:
                got = (d_out if mode == "separate" else d_logit)[:n].cpu().numpy()
                assert_bitwise(got, p if output_prob else lg, "what predict_finish returns")
    # an unlabelled call counts nothing
    restart(e, eval=True)
    e.predict_finish_device(n, d_logit.data_ptr(), None, 0, None)
    e.sync()
    assert_hist(e, "eval", EMPTY, "label == NULL")


# ---- 2. every labelled predict entry point ---------------------------------------------------

@pytest.mark.parametrize("name", list(MODELS))
def test_every_labelled_predict_entry_point(name):
    o, e, st = make_pair(name)
    off = make_engine(name, st)
    blocks = [make_block(name, n, 50 + i) for i, n in enumerate((300, 257, 64, 1))]
    probs = [o.predict_batch(b, output_prob=True)[0] for b in blocks]
    want_all = EMPTY
    for b, p in zip(blocks, probs):
        want_all = add_hist(want_all, want_hist(p, b.label))
    e.metrics_enable(eval=True, train=True)
    # predict_batch, logits and probabilities out
    for output_prob in (False, True):
        restart(e, eval=True, train=True)
        for b, p in zip(blocks, probs):
            out, loss = e.predict_batch(b, output_prob=output_prob)
            out_off, loss_off = off.predict_batch(b, output_prob=output_prob)
            assert_bitwise(out, out_off, "predict_batch output with the channel on")
            assert loss == loss_off
            if output_prob:
                assert_bitwise(out, p, "probabilities against the oracle")
        assert_hist(e, "eval", want_all, "%s predict_batch output_prob=%d" % (name, output_prob))
    # ... and an unlabelled one adds nothing
    e.predict_batch(blocks[0], with_loss=False)
    assert_hist(e, "eval", want_all, "unlabelled predict_batch")
    # predict_batch_async, copying and zero-copy, with and without the field array
    for zero_copy in (False, True):
        for bare in (False, True):
            cs = [without_field_array(b) if bare else b for b in blocks]
            if zero_copy:
                cs = [pinned(c) for c in cs]
            restart(e, eval=True, train=True)
            for c in cs:
                e.predict_batch_async(c, zero_copy=zero_copy)
                off.predict_batch_async(c, zero_copy=zero_copy)
            assert e.train_flush() == off.train_flush()
            assert_hist(e, "eval", want_all, "%s predict_batch_async zero_copy=%d bare=%d" % (name, zero_copy, bare))
    # reading launches the deferred block itself: no flush in between
    restart(e, eval=True, train=True)
    for b in blocks:
        e.predict_batch_async(b)
    assert_hist(e, "eval", want_all, "read without a flush")
    e.train_flush()
    # predict_batch_device
    for output_prob in (0, 1):
        restart(e, eval=True, train=True)
        for b, p in zip(blocks, probs):
            d = DeviceBlock(b)
            d_out = torch.zeros(b.n_rows, dtype=torch.float32, device="cuda")
            d_loss = torch.zeros(1, dtype=torch.float64, device="cuda")
            e.predict_batch_device(*d.args(), output_prob, d_out.data_ptr(), d_loss.data_ptr())
            e.sync()
            if output_prob:
                assert_bitwise(d_out.cpu().numpy(), p, "predict_batch_device probabilities")
            assert float(d_loss.cpu()[0]) == off.predict_batch(b)[1]
            # out == NULL: the engine's own output array
            e.predict_batch_device(*d.args(), output_prob, None, None)
            e.sync()
        assert_hist(e, "eval", add_hist(want_all, want_all), "%s predict_batch_device output_prob=%d" % (name, output_prob))
    assert_hist(e, "train", EMPTY, "predicting leaves the train channel alone")
    e.close()
    off.close()


# ---- 3. the train channel on every training path --------------------------------------------

def _run_train(e, path, blocks):
    keep = []
    if path == "train_batch":
        for b in blocks:
            e.train_batch(b)
    elif path == "train_batch_async":
        for b in blocks:
            e.train_batch_async(b)
        e.train_flush()
    elif path == "train_batch_async_pinned":
        keep = [pinned(b) for b in blocks]
        for c in keep:
            e.train_batch_async_pinned(c)
        e.train_flush()
    elif path == "stage_batch+train_staged":
        for b in blocks:
            e.stage_batch(b)
            e.train_staged()
        e.sync()
    elif path == "train_batch_device":
        for b in blocks:
            d = DeviceBlock(b)
            keep.append(d)
            e.train_batch_device(*d.args())
        e.sync()
    else:
        assert path == "train_forward_device+train_update_device"
        buf = torch.zeros(MAX_ROWS, dtype=torch.float32, device="cuda")
        for i, b in enumerate(blocks):
            d = DeviceBlock(b)
            keep.append(d)
            e.train_forward_device(*d.args(), buf.data_ptr())
            # the logits handed back (what a shard gets from the all-reduce), or the engine's own
            e.train_update_device(buf.data_ptr() if i % 2 == 0 else None)
        e.sync()
    return keep


TRAIN_PATHS = ["train_batch", "train_batch_async", "train_batch_async_pinned", "stage_batch+train_staged",
               "train_batch_device", "train_forward_device+train_update_device"]


@pytest.fixture(scope="module")
def train_reference():
    """Per model: the start state, four blocks, the oracle's pre-update logits of each (the histogram
    they make) and its final state -- computed once, shared by the six paths."""
    out = {}
    for name in MODELS:
        mt, nf, F, k = MODELS[name]
        o = CpuModel("oracle", mt, nf, F, k, **STRESS_HP)
        st = rand_state(np.random.default_rng(3), o)
        o.set_state(st)
        blocks = [make_block(name, n, 70 + i) for i, n in enumerate((256, 300, 65, 129))]
        want = EMPTY
        for b in blocks:
            lg, _ = o.train_batch(b)
            want = add_hist(want, want_hist(oracle_sigmoid(lg), b.label))
        out[name] = (st, blocks, want, o.get_state())
    return out


@pytest.mark.parametrize("path", TRAIN_PATHS)
@pytest.mark.parametrize("name", list(MODELS))
def test_train_channel_on_every_training_path(train_reference, name, path):
    st, blocks, want, final = train_reference[name]
    e, off = make_engine(name, st), make_engine(name, st)
    e.metrics_enable(eval=True, train=True)
    keep = _run_train(e, path, blocks)
    keep_off = _run_train(off, path, blocks)
    assert_hist(e, "train", want, "%s %s" % (name, path))
    assert_hist(e, "eval", EMPTY, "training leaves the eval channel alone")
    se = e.get_state()
    assert_state_bitwise(se, off.get_state(), "final state, metrics on against off")
    assert_state_bitwise(se, final, "final state against the oracle")
    del keep, keep_off
    e.close()
    off.close()


# ---- 4. a group: two shards sharing the one GPU ----------------------------------------------

def _group():
    mt, nf, F, k = MODELS["FFM"]
    g = fa.Group([0, 0], "FFM", nf, F, k, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * F, seed=4, max_row_nnz=F,
                 field_start=FFM_FIELD_START, **STRESS_HP)
    for e in g.engines:
        e.fill_state(seed=6)
    return g


def test_group_channels_hold_what_the_group_returns():
    """The cross-shard sum is not the oracle's association order, so the expected bins come from the
    logits / probabilities the same group returns with the channels off."""
    blocks = [make_block("FFM", n, 90 + i) for i, n in enumerate((300, 64, 257))]
    a = _group()
    assert a.collective == "device-local sum"
    with pytest.raises(fa.EngineError) as err:
        a.metrics("eval")
    assert err.value.code == fa.engine.E_INVALID
    logits = [a.train_batch(b)[0].copy() for b in blocks]
    want_train = EMPTY
    for b, lg in zip(blocks, logits):
        want_train = add_hist(want_train, want_hist(oracle_sigmoid(lg), b.label))
    pred_logit = [a.predict_batch(b, output_prob=False)[0].copy() for b in blocks]
    pred_prob = [a.predict_batch(b, output_prob=True)[0].copy() for b in blocks]
    want_eval = EMPTY
    for b, lg, p in zip(blocks, pred_logit, pred_prob):
        assert_bitwise(p, oracle_sigmoid(lg), "the group's probabilities are the sigmoid of its logits")
        want_eval = add_hist(want_eval, want_hist(p, b.label))
    # the same group, channels on: predicting changes no state, so it predicts the same again
    a.metrics_enable(eval=True, train=True)
    for output_prob in (False, True):
        for b in blocks:
            a.predict_batch(b, output_prob=output_prob)
    a.predict_batch(blocks[0], with_loss=False)  # unlabelled: not counted
    pos, neg = a.metrics_histogram("eval")
    assert np.array_equal(pos, 2 * want_eval[0]) and np.array_equal(neg, 2 * want_eval[1])
    m = a.metrics("eval", reset=True)
    assert m["n_pos"] + m["n_neg"] == 2 * sum(b.n_rows for b in blocks) and m["n_nan"] == 0
    assert a.metrics("eval")["n_pos"] == 0
    a.close()
    # a second and a third group from the same start, channels on: block by block and pipelined
    for pipelined in (False, True):
        g = _group()
        g.metrics_enable(eval=True, train=True)
        for i, b in enumerate(blocks):
            if pipelined:
                g.train_batch_async(b)
            else:
                assert_bitwise(g.train_batch(b)[0], logits[i], "group logits with the channel on")
        if pipelined:
            g.train_flush()
        assert_hist(g.engines[0], "train", want_train, "group train channel, pipelined=%d" % pipelined)
        assert g.metrics("train")["n_pos"] == int(want_train[0].sum())
        assert_hist(g.engines[0], "eval", EMPTY, "group eval channel after training")
        with pytest.raises(fa.EngineError):  # rank 1 keeps no channel
            g.engines[1].metrics("train")
        g.close()


# ---- 5. bookkeeping --------------------------------------------------------------------------

def _metric_launches(e):
    m = re.search(r"metric_hist_kernel\s+launches=\s*(\d+)", e.profile_dump())
    return int(m.group(1)) if m else 0


def test_bookkeeping(monkeypatch):
    o, e, st = make_pair("FFM")
    blocks = [make_block("FFM", n, 110 + i) for i, n in enumerate((200, 100, 65))]
    probs = [o.predict_batch(b, output_prob=True)[0] for b in blocks]
    hists = [want_hist(p, b.label) for b, p in zip(blocks, probs)]
    # off by default: reading is FFM_E_INVALID, and no launch is made
    for ch in ("eval", "train"):
        with pytest.raises(fa.EngineError) as err:
            e.metrics(ch)
        assert err.value.code == fa.engine.E_INVALID
        with pytest.raises(fa.EngineError):
            e.metrics_histogram(ch)
    with pytest.raises(fa.EngineError):
        e._check(e.lib.ffm_engine_metrics_enable(e.h, 4))
    with pytest.raises(fa.EngineError):
        e._check(e.lib.ffm_engine_metrics_read(e.h, 2, 0, ctypes.byref(fa.Metrics())))
    e.profile_enable(True)
    for b in blocks:
        e.predict_batch(b)
    assert _metric_launches(e) == 0 and "metric_hist_kernel" not in e.profile_dump()
    # on: exactly one launch per labelled block
    e.metrics_enable(eval=True)
    e.profile_enable(True)
    for b in blocks:
        e.predict_batch(b)
    e.predict_batch(blocks[0], with_loss=False)
    assert _metric_launches(e) == len(blocks)
    # counts add up across blocks
    assert_hist(e, "eval", add_hist(add_hist(hists[0], hists[1]), hists[2]), "three blocks")
    with pytest.raises(fa.EngineError):  # the channels are independent: train is still off
        e.metrics("train")
    # enabling a channel that is on keeps its counts; the other one starts from zero
    e.metrics_enable(eval=True, train=True)
    assert_hist(e, "eval", add_hist(add_hist(hists[0], hists[1]), hists[2]), "after a second enable")
    assert_hist(e, "train", EMPTY, "a channel that turned on")
    # reset returns the numbers and clears
    m = e.metrics("eval", reset=True)
    assert m["n_pos"] + m["n_neg"] == sum(b.n_rows for b in blocks)
    assert_hist(e, "eval", EMPTY, "after reset")
    e.predict_batch(blocks[1])
    assert_hist(e, "eval", hists[1], "counting again after reset")
    # the train channel: one launch per training block, the eval channel untouched by it
    e.profile_enable(True)
    lg = [o.train_batch(b)[0] for b in blocks[:2]]
    for b in blocks[:2]:
        e.train_batch(b)
    assert _metric_launches(e) == 2
    assert_hist(e, "train", add_hist(want_hist(oracle_sigmoid(lg[0]), blocks[0].label),
                                     want_hist(oracle_sigmoid(lg[1]), blocks[1].label)), "two training blocks")
    assert_hist(e, "eval", hists[1], "eval channel after training")
    # a channel turned off stops counting and cannot be read; turned on again it starts from zero
    e.metrics_enable(train=True)
    e.profile_enable(True)
    e.predict_batch(blocks[0])
    assert _metric_launches(e) == 0
    with pytest.raises(fa.EngineError):
        e.metrics("eval")
    e.metrics_enable(eval=True, train=True)
    assert_hist(e, "eval", EMPTY, "eval channel back on")
    e.profile_enable(False)
    e.close()
    # FFM_ENGINE_METRICS=3 at create is metrics_enable(3)
    monkeypatch.setenv("FFM_ENGINE_METRICS", "3")
    a = make_engine("FFM", st)
    monkeypatch.delenv("FFM_ENGINE_METRICS")
    b_eng = make_engine("FFM", st)
    with pytest.raises(fa.EngineError):
        b_eng.metrics("eval")
    b_eng.metrics_enable(eval=True, train=True)
    for x in (a, b_eng):
        x.predict_batch(blocks[0])
        x.train_batch(blocks[1])
    for ch in ("eval", "train"):
        pa, na = a.metrics_histogram(ch)
        pb, nb = b_eng.metrics_histogram(ch)
        assert np.array_equal(pa, pb) and np.array_equal(na, nb) and int(pa.sum() + na.sum()) > 0
        assert a.metrics(ch) == b_eng.metrics(ch)
    monkeypatch.setenv("FFM_ENGINE_METRICS", "1")
    c = make_engine("FFM", st)
    assert c.metrics("eval")["n_pos"] == 0
    with pytest.raises(fa.EngineError):
        c.metrics("train")
    for x in (a, b_eng, c):
        x.close()


# ---- 6. NaN scores ---------------------------------------------------------------------------

def test_nan_scores_are_counted_apart():
    """The state of test_quirk_nans_flow_through_the_folds (n near 0, a third of it 0: sqrt(n + g2*g1) of
    ffm.cpp:118 goes NaN): after two blocks the model holds NaN accumulators and weights, and rows that touch
    them score NaN -- in no bin, counted in n_nan, on both channels.  Two training blocks of eight rows: in
    a model of 97 features longer ones leave no finite score at all."""
    mt, nf, F, k = MODELS["FFM"]
    rng = np.random.default_rng(23)
    o = CpuModel("oracle", mt, nf, F, k, **STRESS_HP)
    st = rand_state(rng, o, n_hi=0.02)
    st["vec_n"][rng.random(st["vec_n"].shape) < 0.3] = 0.0
    o.set_state(st)
    e = make_engine("FFM", st)
    e.metrics_enable(eval=True, train=True)
    blocks = [make_block("FFM", n, 130 + i) for i, n in enumerate((8, 8, 300))]
    want_train = EMPTY
    for b in blocks[:2]:
        lg, _ = o.train_batch(b)
        assert_bitwise(e.train_batch(b)[0], lg, "pre-update logits")
        want_train = add_hist(want_train, want_hist(oracle_sigmoid(lg), b.label))
    p = o.predict_batch(blocks[2], output_prob=True)[0]
    n_nan = int(np.isnan(p).sum())
    assert 0 < n_nan < blocks[2].n_rows, "the case must produce NaN scores beside finite ones"
    assert 0 < want_train[2] < 16, "... and NaN pre-update logits in the second block"
    e.predict_batch(blocks[2])
    assert_hist(e, "eval", want_hist(p, blocks[2].label), "eval channel with NaN rows")
    assert e.metrics("eval")["n_nan"] == n_nan
    assert_hist(e, "train", want_train, "train channel with NaN rows")
    e.close()


# ---- 7. the guarantee ------------------------------------------------------------------------

def exact_rank_auc(p, label):
    """The rank AUC of the scores with ties counted 1/2 (average ranks), as a Fraction."""
    p, y = np.asarray(p, np.float64), np.asarray(label) > 0
    order = np.argsort(p, kind="stable")
    ps = p[order]
    twice_rank = np.zeros(p.size, np.int64)  # 2 x the average 1-based rank: an integer
    i = 0
    while i < p.size:
        j = i
        while j + 1 < p.size and ps[j + 1] == ps[i]:
            j += 1
        twice_rank[order[i:j + 1]] = (i + 1) + (j + 1)
        i = j + 1
    P, N = int(y.sum()), int((~y).sum())
    return Fraction(int(twice_rank[y].sum()) - P * (P + 1), 2 * P * N)


def test_the_exact_rank_auc_lies_within_the_slack():
    o, e, _ = make_pair("FFM")
    e.metrics_enable(eval=True)
    blk = make_block("FFM", 1000, 150)
    p = o.predict_batch(blk, output_prob=True)[0]
    assert not np.isnan(p).any()
    e.predict_batch(blk)
    m = e.metrics("eval")
    pos, neg = e.metrics_histogram("eval")
    # the bound in exact arithmetic, from the counters ...
    P = N = below = ties = 0
    for b in np.flatnonzero((pos != 0) | (neg != 0)):
        below += int(pos[b]) * N
        ties += int(pos[b]) * int(neg[b])
        P += int(pos[b])
        N += int(neg[b])
    auc, slack = Fraction(2 * below + ties, 2 * P * N), Fraction(ties, 2 * P * N)
    exact = exact_rank_auc(p, blk.label)
    print("auc %.9f slack %.3e exact %.9f mixed bins %d" % (m["auc"], m["auc_slack"], float(exact), m["n_mixed_bins"]))
    assert abs(exact - auc) <= slack
    # ... and the doubles the engine reports are those fractions (two conversions and a divide: 4 ulp)
    assert abs(Fraction(m["auc"]) - auc) <= 4 * Fraction(math.ulp(float(auc)))
    assert abs(Fraction(m["auc_slack"]) - slack) <= 4 * Fraction(math.ulp(float(slack))) if slack else m["auc_slack"] == 0.0
    assert (m["n_pos"], m["n_neg"]) == (int((blk.label > 0).sum()), int((blk.label <= 0).sum()))
    if slack == 0:  # no bin holds rows of both classes: the histogram AUC is the rank AUC
        assert exact == auc
    # the bound met with equality: two scores that differ, in one bin, of opposite labels
    x1 = np.float32(0.0)
    x2 = next(np.float32(j * 2.0 ** -24) for j in range(1, 64)
              if _sig().sigmoid(float(np.float32(j * 2.0 ** -24))) != _sig().sigmoid(0.0))
    p1, p2 = oracle_sigmoid([x1, x2])
    assert p1 != p2 and bins_of([p1])[0] == bins_of([p2])[0]
    for labels, exact_auc in (((0, 1), 1), ((1, 0), 0)):  # (the higher score is x2's)
        restart(e, eval=True)
        d_logit = torch.tensor([float(x1), float(x2)], dtype=torch.float32, device="cuda")
        d_label = torch.tensor(labels, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.predict_finish_device(2, d_logit.data_ptr(), d_label.data_ptr(), 0, None)
        e.sync()
        m = e.metrics("eval")
        assert m["auc"] == 0.5 and m["auc_slack"] == 0.5 and m["n_mixed_bins"] == 1
        assert exact_rank_auc([p1, p2], labels) == exact_auc
        assert abs(exact_auc - m["auc"]) == m["auc_slack"]
    e.close()
