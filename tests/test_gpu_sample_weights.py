"""Per-row sample weights (include/ffm_engine.h "Sample weights"): tmp_grad[r] = (sigmoid(logit[r]) -
y[r]) * weight[r], one fp32 multiply; the loss term (double)weight[r] * loss; nothing else changes.

  1. ones are nothing: the *_weighted call with all-1.0f weights, the *_weighted call with NULL and the
     legacy call give bitwise equal state, logit_out and loss sum -- FFM / FM / LR, blocks of 1, 7 and
     300 rows, every path a weight can take (sync host, device whole step, split forward + update,
     staged copy, staged zero_copy, the async pipeline);
  2. the fold against the numpy restatement (tests/test_block_semantics.py: numpy_block takes the
     per-row gradient as an input): the oracle trains the block unweighted -- its pre-update logits and
     its refreshed w --, tg = f32(f32(sigmoid(l) - y) * weight) goes into numpy_block, and the engine's
     n, z, w are those bit for bit, NaN positions included, through the whole step (the row kernel
     makes tg) and through the split step (tmp_grad_weighted_kernel), with and without field_start;
  3. FM: one-row blocks against a numpy restatement of fm.cpp:80-101 with tmp_grad scaled; blocks of
     several rows: weighted whole step == weighted split step;
  4. the weighted loss sum is sum((double)w * loss(y, logit_out));
  5. the pipeline: seven blocks of 515 rows, each with other weights, one with NULL, copying and
     zero_copy, against the sync weighted calls;
  6. groups of 2 and 4 shards on one device; 6b. the weighted row kernels that hold no (n, z), with rows
     staged above 64 KB of dynamic LDS; 7. refusals.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import CpuModel, Csr
from test_block_semantics import numpy_block, numpy_refresh
from util import (DEFAULT_HP, STRESS_HP, assert_bitwise, assert_state_bitwise, bits, block_ids_per_field,
                  irregular_copy, loss_close, occurrence_block, rand_state)

pytestmark = pytest.mark.gpu

f32 = np.float32
LEGACY = "legacy"  # the entry point without a weight argument
ROWS = 300
COUNTS = [300, 130, 40, 12, 5, 2]  # one giant, one huge, one big, few-occurrence; the rest once-only
F4 = 4
PER = block_ids_per_field(ROWS)
NF = F4 * PER
_f32p = ctypes.POINTER(ctypes.c_float)


def _own_pages(a):
    out = fa.page_aligned(a.size, a.dtype)
    out[:] = a
    return out


def _own_pages_block(c):
    return Csr(*[_own_pages(getattr(c, key)) for key in ("row_ptr", "field", "feat", "val", "label")])


def _engine(mt, k, hp, rows=ROWS, field_start=False, nf=NF, F=F4, **kw):
    fs = (np.arange(F + 1) * (nf // F)).astype(np.int32) if field_start else None
    return fa.Engine(mt, nf, F if mt == "FFM" else 1, k, max_batch_rows=rows, max_batch_nnz=rows * F,
                     max_row_nnz=F, field_start=fs, **hp, **kw)


def _block(mt, n_rows, seed=5):
    """Rows of the 300-row occurrence block (ids stay inside their fields' ranges)."""
    blk = occurrence_block(F4, COUNTS, ROWS, seed=seed)[0].rows(0, n_rows)
    if mt != "FFM":
        blk.field[:] = 0
    return blk


def _mixed_weights(n, seed, values=(0, 0.25, 1, 3.5, 1e-3, 64)):
    """Drawn from {0, 0.25, 1, 3.5, 1e-3, 64} mixed with uniform values in [0, 2)."""
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array(values, f32), n)
    u = rng.random(n) < 0.4
    w[u] = rng.random(int(u.sum())).astype(f32) * f32(2)
    return np.ascontiguousarray(w, f32)


# ---- every path a block (and its weights) can take --------------------------------------------------


class _Dev:
    """The block, its weights and the outputs in device memory."""

    def __init__(self, e, c, weight):
        self.t = {key: torch.from_numpy(np.ascontiguousarray(getattr(c, key))).cuda()
                  for key in ("row_ptr", "field", "feat", "val", "label")}
        self.w = torch.from_numpy(weight).cuda() if isinstance(weight, np.ndarray) else None
        self.out = torch.full((max(c.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
        self.part = torch.full_like(self.out, float("nan"))
        self.loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t = self.t
        self.csr = (c.n_rows, int(c.row_ptr[-1]), t["row_ptr"].data_ptr(),
                    t["field"].data_ptr() if e.model_type == fa.engine.FFM else None, t["feat"].data_ptr(),
                    t["val"].data_ptr(), t["label"].data_ptr())
        self.n = c.n_rows

    def wptr(self):
        return self.w.data_ptr() if self.w is not None else None

    def result(self, e):
        e.sync()
        return self.out[:self.n].cpu().numpy(), float(self.loss.cpu()[0])


def _run(e, path, c, weight):
    """One block through `path`.  weight: LEGACY (the entry point without weights), None (the weighted
    one with NULL) or a float32 array.  Returns (logits or None, loss sum)."""
    lib, legacy = e.lib, isinstance(weight, str)
    wa = weight if isinstance(weight, np.ndarray) else None
    if path == "host":
        out = np.zeros(max(c.n_rows, 1), f32)
        loss = ctypes.c_double(0.0)
        if legacy:
            e._check(lib.ffm_engine_train_batch(e.h, *e._csr(c), out.ctypes.data_as(_f32p), ctypes.byref(loss)))
        else:
            e._check(lib.ffm_engine_train_batch_weighted(e.h, *e._csr(c), None if wa is None else wa.ctypes.data_as(_f32p),
                                                         out.ctypes.data_as(_f32p), ctypes.byref(loss)))
        return out[:c.n_rows], float(loss.value)
    if path in ("device", "split"):
        d = _Dev(e, c, weight)
        if path == "device":
            if legacy:
                e._check(lib.ffm_engine_train_batch_device(e.h, *d.csr, d.out.data_ptr(), d.loss.data_ptr()))
            else:
                e._check(lib.ffm_engine_train_batch_device_weighted(e.h, *d.csr, d.wptr(), d.out.data_ptr(), d.loss.data_ptr()))
        else:
            if legacy:
                e._check(lib.ffm_engine_train_forward_device(e.h, *d.csr, d.part.data_ptr()))
            else:
                e._check(lib.ffm_engine_train_forward_device_weighted(e.h, *d.csr, d.wptr(), d.part.data_ptr()))
            e.sync()
            e.train_update_device(d.part.data_ptr(), d.out.data_ptr(), d.loss.data_ptr())
        return d.result(e)
    if path in ("staged", "staged_zc", "staged_split"):
        zc = path == "staged_zc"
        cb, wb = c, wa
        if zc:
            cb = _own_pages_block(c)
            e.pin_block(cb)
            if wa is not None:
                wb = _own_pages(wa)
                e._check(lib.ffm_engine_pin_host(wb.ctypes.data, wb.nbytes))
        out = torch.full((max(c.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        try:
            if legacy:
                e._check(lib.ffm_engine_stage_batch(e.h, *e._csr(cb), int(zc)))
            else:
                e._check(lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(cb), None if wb is None else wb.ctypes.data, int(zc)))
            if path == "staged_split":  # the logits handed back in: tmp_grad(_weighted)_kernel makes tg
                part = torch.full_like(out, float("nan"))
                e.train_forward_staged(part.data_ptr())
                e.sync()
                e.train_update_device(part.data_ptr(), out.data_ptr(), loss.data_ptr())
            else:
                e.train_staged(out.data_ptr(), loss.data_ptr())
            e.sync()
        finally:
            if zc:
                e.sync()
                e.unpin_block(cb)
                if wa is not None:
                    lib.ffm_engine_unpin_host(wb.ctypes.data)
        return out[:c.n_rows].cpu().numpy(), float(loss.cpu()[0])
    assert path == "async"
    if legacy:
        e._check(lib.ffm_engine_train_batch_async(e.h, *e._csr(c)))
    else:
        e._check(lib.ffm_engine_train_batch_async_weighted(e.h, *e._csr(c), None if wa is None else wa.ctypes.data, 0))
    return None, e.train_flush()


PATHS = ("host", "device", "split", "staged", "staged_zc", "async")
MODELS = [("FFM", 4), ("FFM", 2), ("FM", 4), ("FM", 65), ("LR", 1)]


# ---- 1. ones are nothing -----------------------------------------------------------------------------


@pytest.mark.parametrize("mt,k", MODELS, ids=["%s-k%d" % m for m in MODELS])
def test_weights_of_one_are_the_unweighted_call_bit_for_bit(mt, k):
    engines = [_engine(mt, k, STRESS_HP, seed=9) for _ in range(3)]
    for e in engines:
        e.fill_state(seed=6)
    init = engines[0].get_state()
    assert_state_bitwise(engines[1].get_state(), init, "twin engines")
    for n_rows in (1, 7, 300):
        c = _block(mt, n_rows)
        for path in PATHS:
            got = []
            for e, weight in zip(engines, (LEGACY, None, np.ones(n_rows, f32))):
                e.set_state(init)
                lg, ls = _run(e, path, c, weight)
                got.append((lg, ls, e.get_state()))
            for name, (lg, ls, st) in zip(("NULL", "ones"), got[1:]):
                what = "%s k=%d %d rows %s: %s vs legacy" % (mt, k, n_rows, path, name)
                if lg is not None:
                    assert_bitwise(lg, got[0][0], what + " logits")
                assert np.float64(ls).tobytes() == np.float64(got[0][1]).tobytes() or (np.isnan(ls) and np.isnan(got[0][1])), (what, ls, got[0][1])
                assert_state_bitwise(st, got[0][2], what)
            assert not np.array_equal(bits(got[0][2]["lin_n"]), bits(init["lin_n"])), "the block must train something"
    for e in engines:
        e.close()


# ---- 2. the fold against the numpy restatement ----------------------------------------------------------


def _oracle_sigmoid_minus_y(o, logits, label):
    return np.array([f32(o.sigmoid(float(l))) - f32(y) for l, y in zip(logits, label)], f32)


@functools.lru_cache(maxsize=None)
def _fold_blocks(mt):
    regular = _block(mt, ROWS)
    irregular = irregular_copy(occurrence_block(F4, COUNTS, ROWS, seed=5)[0], seed=5)
    if mt != "FFM":
        irregular.field[:] = 0
    return (("regular", regular), ("irregular", irregular), ("7 rows", regular.rows(0, 7)), ("1 row", regular.rows(0, 1)))


def _fold_reference(o, st, c, weight, hp, kk):
    """(unweighted logits, unweighted state after the block, the weighted state numpy_block gives, the
    weighted loss sum)."""
    o.set_state(st)
    logits, _ = o.train_batch(c)
    with np.errstate(all="ignore"):
        tg = (_oracle_sigmoid_minus_y(o, logits, c.label) * weight).astype(f32)
        want = numpy_block(o, st, c, tg, hp, F4 if kk else 1, kk)
    loss = 0.0
    for l, y, w in zip(logits, c.label, weight):
        loss += float(np.float64(w) * np.float64(o.loss(int(y), float(l))))
    return logits, o.get_state(), want, loss


FOLD_MODELS = [("FFM", 4), ("FFM", 2), ("LR", 1)]


@pytest.mark.parametrize("hp_name", ["stress_hp", "default_hp"])
@pytest.mark.parametrize("mt,k", FOLD_MODELS, ids=["%s-k%d" % m for m in FOLD_MODELS])
def test_weighted_fold_is_the_numpy_restatement_bit_for_bit(mt, k, hp_name):
    hp = STRESS_HP if hp_name == "stress_hp" else DEFAULT_HP
    kk = k if mt == "FFM" else 0
    o = CpuModel("oracle", mt, NF, F4 if mt == "FFM" else 1, k, **hp)
    st = rand_state(np.random.default_rng(21), o, n_hi=1e-4, w_sd=0.5)  # (as test_block_semantics._fold_case)
    engines = [(fs, _engine(mt, k, hp, field_start=fs, skip_init=True)) for fs in ((False, True) if mt == "FFM" else (False,))]
    saw_nan = differs_most = False
    for name, c in _fold_blocks(mt):
        sets = [("mixed", _mixed_weights(c.n_rows, 31))]
        if name == "regular":
            sets.append(("all zero", np.zeros(c.n_rows, f32)))
        for wname, weight in sets:
            logits, unweighted, want, want_loss = _fold_reference(o, st, c, weight, hp, kk)
            saw_nan = saw_nan or bool(np.isnan(want["vec_z"]).any())
            if wname == "mixed" and c.n_rows == ROWS:
                for kn, kz in (("lin_n", "lin_z"), ("vec_n", "vec_z")):
                    touched = bits(unweighted[kn]) != bits(st[kn])
                    both_nan = np.isnan(want[kz]) & np.isnan(unweighted[kz])
                    other = touched & ((bits(want[kn]) != bits(unweighted[kn])) | ((bits(want[kz]) != bits(unweighted[kz])) & ~both_nan))
                    if touched.sum() > 0:
                        assert other.sum() > touched.sum() / 2, (name, kn, int(other.sum()), int(touched.sum()))
                        differs_most = True
            for fs, e in engines:
                for path in ("host", "staged_split"):  # the row kernel makes tg | tmp_grad_weighted_kernel does
                    e.set_state(st)
                    lg, ls = _run(e, path, c, weight)
                    what = "%s k=%d %s %s, %s weights, field_start=%s, %s" % (mt, k, hp_name, name, wname, fs, path)
                    assert_bitwise(lg, logits, what + ": weights must not touch the forward pass")
                    assert loss_close(ls, want_loss), (what, ls, want_loss)
                    assert_state_bitwise(e.get_state(), want, what)
    assert differs_most, "one case must differ from the unweighted result in most touched accumulators"
    if mt == "FFM" and hp_name == "stress_hp":
        assert saw_nan, "the stress case should reach ffm.cpp:118's NaN"
    for _, e in engines:
        e.close()


# ---- 3. FM ---------------------------------------------------------------------------------------------


def _fm_one_row(o, st, c, weight, hp, k):
    """fm.cpp:21-32 and :80-101 (and ftrl_model.cpp:66-85) for ONE row with tmp_grad scaled by the row's
    weight: the oracle's unweighted step gives the logit and the refreshed w, the rest is restated."""
    o.set_state(st)
    logits, _ = o.train_batch(c)
    w = o.get_state()  # (w as the refresh left it; n and z are restated below)
    out = {key: st[key].copy() for key in st}
    out["lin_w"], out["vec_w"], out["bias3"][0] = w["lin_w"], w["vec_w"], w["bias3"][0]
    alpha = f32(hp["w_alpha"])
    tg = f32(f32(f32(o.sigmoid(float(logits[0]))) - f32(c.label[0])) * f32(weight[0]))
    ids, xs = c.feat, c.val
    vw = w["vec_w"].reshape(-1, k)
    s_vx = np.zeros(k, f32)
    for f in range(k):
        for i, x in zip(ids, xs):
            s_vx[f] = f32(s_vx[f] + f32(vw[i, f] * x))

    def step(n, z, wv, g):
        s = f32(f32(np.sqrt(f32(n + f32(g * g))) - np.sqrt(n)) / alpha)
        return f32(n + f32(g * g)), s

    for i, x in zip(ids, xs):
        g = f32(tg * x)
        n, s = step(st["lin_n"][i], st["lin_z"][i], w["lin_w"][i], g)
        out["lin_z"][i] = f32(st["lin_z"][i] + f32(g - f32(s * w["lin_w"][i])))
        out["lin_n"][i] = n
        for f in range(k):
            v = vw[i, f]
            g = f32(tg * f32(f32(x * s_vx[f]) - f32(f32(v * x) * x)))
            n, s = step(st["vec_n"].reshape(-1, k)[i, f], None, v, g)
            out["vec_z"].reshape(-1, k)[i, f] = f32(f32(st["vec_z"].reshape(-1, k)[i, f] + g) - f32(s * v))
            out["vec_n"].reshape(-1, k)[i, f] = n
    n, s = step(st["bias3"][1], None, None, tg)
    out["bias3"][2] = f32(st["bias3"][2] + f32(tg - f32(s * w["bias3"][0])))
    out["bias3"][1] = n
    return logits, out


@pytest.mark.parametrize("k", [4, 65])
def test_fm_weighted_step(k):
    o = CpuModel("oracle", "FM", NF, 1, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(41), o)
    st["vec_n"] += f32(0.05)
    st["lin_n"] += f32(0.05)
    e = _engine("FM", k, STRESS_HP, skip_init=True)
    for row, wv in ((0, 3.5), (1, 0.25), (2, 0.0)):
        c = _block("FM", ROWS).rows(row, row + 1)
        weight = np.array([wv], f32)
        with np.errstate(all="ignore"):
            logits, want = _fm_one_row(o, st, c, weight, STRESS_HP, k)
        for path in ("host", "staged_split"):
            e.set_state(st)
            lg, _ = _run(e, path, c, weight)
            what = "FM k=%d one row, weight %g, %s" % (k, wv, path)
            assert_bitwise(lg, logits, what)
            assert_state_bitwise(e.get_state(), want, what)
    for n_rows in (7, 300):  # several rows: the whole step (fm_row_wave_kernel makes tg at k <= 64) == the split step
        c = _block("FM", n_rows)
        weight = _mixed_weights(n_rows, 43)
        got = []
        for path in ("host", "staged_split"):
            e.set_state(st)
            lg, ls = _run(e, path, c, weight)
            got.append((lg, ls, e.get_state()))
        e.set_state(st)
        unweighted = (_run(e, "host", c, LEGACY), e.get_state())
        what = "FM k=%d %d rows whole vs split" % (k, n_rows)
        assert_bitwise(got[0][0], got[1][0], what)
        assert np.float64(got[0][1]).tobytes() == np.float64(got[1][1]).tobytes(), (what, got[0][1], got[1][1])
        assert_state_bitwise(got[0][2], got[1][2], what)
        assert_bitwise(got[0][0], unweighted[0][0], what + ": weights must not touch the forward pass")
        assert not np.array_equal(bits(got[0][2]["vec_z"]), bits(unweighted[1]["vec_z"])), "the weights must change the update"
    e.close()


# ---- 4. the loss ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("mt,k", [("FFM", 4), ("FM", 4), ("FM", 65), ("LR", 1)])
def test_weighted_loss_sum_is_the_sum_of_weight_times_loss(mt, k):
    o = CpuModel("oracle", mt, NF, F4 if mt == "FFM" else 1, k, **DEFAULT_HP)
    e = _engine(mt, k, DEFAULT_HP, seed=3)
    e.fill_state(seed=8)
    init = e.get_state()
    c = _block(mt, ROWS)
    weight = _mixed_weights(ROWS, 51)
    for path in PATHS:
        e.set_state(init)
        lg, ls = _run(e, path, c, weight)
        if lg is None:  # (the pipeline returns no logits: those of the sync call, the same bits)
            e.set_state(init)
            lg, _ = _run(e, "host", c, weight)
        want = 0.0
        for l, y, w in zip(lg, c.label, weight):
            want += float(np.float64(w) * np.float64(o.loss(int(y), float(l))))
        assert abs(ls - want) <= 1e-12 * max(1.0, abs(want)) * 64, (mt, k, path, ls, want)  # (util.loss_close's bound)
        assert loss_close(ls, want)
    e.close()


# ---- 5. the pipeline -------------------------------------------------------------------------------------


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copying", "zero_copy"])
def test_weighted_pipeline_is_the_sync_calls_block_by_block(zero_copy):
    n_blocks, rows, F, k = 7, 515, 4, 4
    nf = F * 600
    gen = synth.Generator(F, nf, "zipf", seed=61)
    blocks = [gen.block(rows) for _ in range(n_blocks)]
    weights = [_mixed_weights(rows, 70 + i) for i in range(n_blocks)]
    weights[3] = None  # one block handed over with NULL
    ref = _engine("FFM", k, STRESS_HP, rows=rows, nf=nf, seed=5)
    ref.fill_state(seed=6)
    init = ref.get_state()
    losses = [ref.train_batch(b, weight=w)[1] for b, w in zip(blocks, weights)]
    want = ref.get_state()
    ref.set_state(init)
    for b in blocks:
        ref.train_batch(b)
    assert not np.array_equal(bits(ref.get_state()["vec_z"]), bits(want["vec_z"])), "the weights must matter"
    ref.close()
    e = _engine("FFM", k, STRESS_HP, rows=rows, nf=nf, seed=5)
    e.set_state(init)
    ring = [(b, w) for b, w in zip(blocks, weights)]
    if zero_copy:
        ring = [(_own_pages_block(b), None if w is None else _own_pages(w)) for b, w in ring]
        for b, w in ring:
            e.pin_block(b)
            if w is not None:
                e._check(e.lib.ffm_engine_pin_host(w.ctypes.data, w.nbytes))
    try:
        for b, w in ring:
            e._check(e.lib.ffm_engine_train_batch_async_weighted(e.h, *e._csr(b), None if w is None else w.ctypes.data,
                                                                 int(zero_copy)))
        total = e.train_flush()
        assert e.blocks_pulled() == n_blocks
    finally:
        if zero_copy:
            e.sync()
            for b, w in ring:
                e.unpin_block(b)
                if w is not None:
                    e.lib.ffm_engine_unpin_host(w.ctypes.data)
    assert_state_bitwise(e.get_state(), want, "pipelined weighted blocks")
    acc = 0.0
    for ls in losses:  # (the flush sum adds the blocks' sums one by one, in order)
        acc += ls
    assert np.float64(total).tobytes() == np.float64(acc).tobytes(), (total, acc)
    e.close()


# ---- 6. groups -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [2, 4])
def test_weighted_group_on_one_device(n):
    F, k, per, rows, n_blocks = 12, 8, 40, 515, 3
    nf = F * per
    gen = synth.Generator(F, nf, "zipf", seed=31)
    blocks = [gen.block(rows) for _ in range(n_blocks)]
    # (a comparison within a tolerance wants finite numbers: under the stress hyper-parameters rows of weight
    # 64 drive the second block's logits to NaN, so the weights here stay at 2 and below)
    weights = [_mixed_weights(rows, 80 + i, values=(0, 0.25, 1, 2, 1e-3)) for i in range(n_blocks)]
    kw = dict(max_batch_rows=rows, max_batch_nnz=rows * F, seed=4, max_row_nnz=F, **STRESS_HP)
    ref = fa.Engine("FFM", nf, F, k, **kw)
    ref.fill_state(seed=6)
    init = ref.get_state()
    logits, losses = zip(*[ref.train_batch(b, weight=w) for b, w in zip(blocks, weights)])
    want = ref.get_state()
    ref.close()
    assert np.isfinite(losses).all() and all(np.isfinite(lg).all() for lg in logits)
    fs = (np.arange(F + 1) * per).astype(np.int32)

    def group():
        g = fa.Group([0] * n, "FFM", nf, F, k, field_start=fs, **kw)
        for e in g.engines:
            e.set_state(init)
        return g

    # ones == unweighted, bit for bit, synchronous and pipelined
    runs = []
    for weight in (None, np.ones(rows, f32)):
        g = group()
        lg, ls = g.train_batch(blocks[0], weight=weight)
        for b in blocks[1:]:
            g.train_batch_async(b, weight=weight)
        total = g.train_flush()
        runs.append((lg, ls, total, [e.get_state() for e in g.engines]))
        g.close()
    assert_bitwise(runs[1][0], runs[0][0], "group logits, ones vs unweighted")
    assert np.float64(runs[1][1]).tobytes() == np.float64(runs[0][1]).tobytes()
    assert np.float64(runs[1][2]).tobytes() == np.float64(runs[0][2]).tobytes()
    for r in range(n):
        assert_state_bitwise(runs[1][3][r], runs[0][3][r], "group rank %d, ones vs unweighted" % r)
    # the weighted group against the weighted engine (the cross-shard logit sum has another association
    # order: the tolerance tests/test_gpu_group.py uses for the same comparison unweighted)
    g = group()
    for i, (b, w) in enumerate(zip(blocks, weights)):
        lg, ls = g.train_batch(b, weight=w)
        np.testing.assert_allclose(lg, logits[i], rtol=2e-4, atol=2e-5, err_msg="block %d" % i)
        assert abs(ls - losses[i]) <= 2e-4 * abs(losses[i])
    plan = fa.shard_plan(F, n, field_map=True)
    states = [e.get_state() for e in g.engines]
    fld = np.arange(nf) // per
    owner = np.repeat(plan["pair_owner"][fld], k, axis=1)
    for key in ("vec_n", "vec_z"):
        merged = np.zeros_like(want[key])
        for r in range(n):
            merged = np.where(owner == r, states[r][key], merged)
        np.testing.assert_allclose(merged, want[key], rtol=2e-4, atol=2e-5, err_msg=key)
    lin_owner = plan["lin_owner"][fld]
    for key in ("lin_n", "lin_z"):
        merged = np.zeros_like(want[key])
        for r in range(n):
            merged = np.where(lin_owner == r, states[r][key], merged)
        np.testing.assert_allclose(merged, want[key], rtol=2e-4, atol=2e-5, err_msg=key)
    g.close()


# ---- 6b. the weighted row kernels that hold nothing, above 64 KB of dynamic LDS ------------------------------


@pytest.mark.parametrize("k,row_hold", [(4, "0"), (3, None)], ids=["k4-FFM_ROW_HOLD=0", "k3"])
def test_weighted_row_kernel_with_rows_staged_above_64kb_of_lds(monkeypatch, k, row_hold):
    """A device entry point stages every row for max_row_nnz entries.  At max_row_nnz = 2048 and three
    fields that is 8192 + 32 * 2048 + 32 = 73 760 bytes of dynamic LDS -- above 64 KB, which a kernel only
    gets when create opted it in.  The two weighted instantiations that hold no (n, z) -- k % 4 == 0 with
    FFM_ROW_HOLD=0, and k % 4 != 0 -- must be among them: one weighted whole step on such an engine
    and on one with max_row_nnz = 3 (the path the rest of this module pins to the oracle) are bit-identical."""
    if row_hold is None:
        monkeypatch.delenv("FFM_ROW_HOLD", raising=False)
    else:
        monkeypatch.setenv("FFM_ROW_HOLD", row_hold)
    F, rows, per = 3, 8, 5
    rng = np.random.default_rng(31)
    feat = (np.arange(F) * per + rng.integers(0, per, (rows, F))).astype(np.int32)  # 5 ids per field: rows share them
    c = Csr(np.arange(rows + 1, dtype=np.int32) * F, np.tile(np.arange(F, dtype=np.int32), rows),
            np.ascontiguousarray(feat.reshape(-1)), rng.uniform(0.5, 1.5, rows * F).astype(f32),
            rng.integers(0, 2, rows).astype(np.int32))
    weight = np.array([0, 0.25, 1, 3.5, 1e-3, 64, 1.75, 0.5], f32)
    got = []
    for max_row_nnz in (F, 2048):
        e = fa.Engine("FFM", F * per, F, k, max_batch_rows=rows, max_batch_nnz=rows * F, max_row_nnz=max_row_nnz,
                      seed=3, **STRESS_HP)
        e.fill_state(seed=6)
        lg, ls = _run(e, "device", c, weight)
        e.check_errors()
        got.append((lg, ls, e.get_state()))
        e.close()
    assert np.isfinite(got[0][0]).all()
    assert_bitwise(got[1][0], got[0][0], "logits, max_row_nnz 2048 vs 3")
    assert bits(np.float64(got[1][1])) == bits(np.float64(got[0][1])), ("loss sum", got[1][1], got[0][1])
    assert_state_bitwise(got[1][2], got[0][2], "state, max_row_nnz 2048 vs 3")


# ---- 7. refusals -------------------------------------------------------------------------------------------


def test_bad_weights_are_refused_and_leave_the_model_untouched():
    e = _engine("FFM", 4, STRESS_HP, seed=11)
    c = _block("FFM", 7)
    cp = _own_pages_block(c)
    e.pin_block(cp)
    wp = fa.page_aligned(16, f32)
    e._check(e.lib.ffm_engine_pin_host(wp.ctypes.data, 4096))
    out = np.zeros(7, f32)
    loss = ctypes.c_double(0.0)
    try:
        for bad in (np.nan, np.inf, -1.0):
            w = np.ones(7, f32)
            w[4] = bad
            wp[:7] = w
            calls = {
                "train_batch_weighted": lambda: e.lib.ffm_engine_train_batch_weighted(
                    e.h, *e._csr(c), w.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p), ctypes.byref(loss)),
                "stage_batch_weighted": lambda: e.lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(c), w.ctypes.data, 0),
                "stage_batch_weighted zero_copy": lambda: e.lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(cp), wp.ctypes.data, 1),
                "train_batch_async_weighted": lambda: e.lib.ffm_engine_train_batch_async_weighted(e.h, *e._csr(c), w.ctypes.data, 0),
                "train_batch_async_weighted zero_copy": lambda: e.lib.ffm_engine_train_batch_async_weighted(
                    e.h, *e._csr(cp), wp.ctypes.data, 1),
            }
            for name, call in calls.items():
                assert call() == fa.engine.E_INVALID, (name, bad)
                assert b"weight" in e.lib.ffm_engine_last_error(), (name, bad)
        wp[:] = 1.0
        # a zero_copy weight array that is page-locked but not 16-byte aligned, and one that is not page-locked
        assert e.lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(cp), wp.ctypes.data + 4, 1) == fa.engine.E_INVALID
        assert b"16-byte aligned" in e.lib.ffm_engine_last_error()
        loose = fa.page_aligned(16, f32)
        loose[:] = 1.0
        assert e.lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(cp), loose.ctypes.data, 1) == fa.engine.E_INVALID
        assert b"page-locked" in e.lib.ffm_engine_last_error()
        assert e.train_flush() == 0.0 and e.blocks_pulled() == 0  # nothing was queued
        assert e.changed_features().size == 0, "a refused block must leave the model untouched"
        # ... and the engine still trains: the same block, good weights, through the entry point that refused
        e._check(e.lib.ffm_engine_stage_batch_weighted(e.h, *e._csr(cp), wp.ctypes.data, 1))
        e.train_staged()
        e.sync()
        assert e.changed_features().size > 0
    finally:
        e.sync()
        e.unpin_block(cp)
        e.lib.ffm_engine_unpin_host(wp.ctypes.data)
    e.close()
    # a group refuses on its first engine: no shard holds a block the others lack
    F, per = 4, PER
    g = fa.Group([0, 0], "FFM", NF, F, 4, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, max_row_nnz=F, seed=4,
                 field_start=(np.arange(F + 1) * per).astype(np.int32), **STRESS_HP)
    w = np.ones(7, f32)
    w[0] = -1.0
    with pytest.raises(fa.EngineError) as ei:
        g.train_batch(c, weight=w)
    assert ei.value.code == fa.engine.E_INVALID
    lg, _ = g.train_batch(c, weight=np.ones(7, f32))  # (not poisoned)
    assert np.isfinite(lg).all()
    g.close()
