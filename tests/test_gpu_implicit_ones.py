"""val == NULL means "every value is 1.0f" (include/ffm_engine.h "Rows without values") on every entry point
that takes rows in host memory.

The yardstick everywhere: an engine of the same config and seed fed the same blocks with numpy.ones(nnz,
float32) spelled out.  Logits, loss sums, scores and the whole state (every touched feature, every untouched
one, the bias triple) must be equal bit for bit.  One FFM and one FM case are also held against the oracle on
the explicit array, so that the pair cannot be wrong together.

Shapes (the smallest at which the fill can go wrong; FFM 5 fields x k = 4): nnz % 4 in {0, 1, 2, 3}, nnz in
{1, 2, 3}, a block of empty rows only, and one block beyond one grid stride of the upload kernel
(701 rows x 39 fields = 27 339 entries against 24 workgroups x 256 lanes x 4 values = 24 576).
"""
import copy
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise, get_bias3, loss_close, rand_state

pytestmark = pytest.mark.gpu

f32 = np.float32
F, K, PER = 5, 4, 40
NF = F * PER
ROWS_MAX = 64
SLOTS = 4  # staging slots of an engine (ffm_engine::kSlots)


# ---- blocks ---------------------------------------------------------------------------------------------


def _regular(n_rows, seed, n_fields=F, per=PER, val=None):
    """One entry per field and row, fields in order, ids of field f in [f * per, (f + 1) * per); values 1.0
    spelled out unless `val` gives them."""
    rng = np.random.default_rng(seed)
    feat = (rng.integers(0, per, (n_rows, n_fields)) + np.arange(n_fields)[None, :] * per).astype(np.int32)
    field = np.broadcast_to(np.arange(n_fields, dtype=np.int32), (n_rows, n_fields)).reshape(-1).copy()
    row_ptr = (np.arange(n_rows + 1, dtype=np.int64) * n_fields).astype(np.int32)
    v = np.ones(n_rows * n_fields, f32) if val is None else np.ascontiguousarray(val, f32)
    return Csr(row_ptr, field, feat.reshape(-1), v, (rng.random(n_rows) < 0.4).astype(np.int32))


def _short(nnz, seed):
    """An empty row, then one row of `nnz` entries (fields 0 .. nnz - 1): nnz in {1, 2, 3}."""
    rng = np.random.default_rng(seed)
    feat = (rng.integers(0, PER, nnz) + np.arange(nnz) * PER).astype(np.int32)
    return Csr(np.array([0, 0, nnz], np.int32), np.arange(nnz, dtype=np.int32), feat, np.ones(nnz, f32),
               np.array([1, 0], np.int32))


def _empty_rows(n_rows=3):
    z = np.zeros(0, np.int32)
    return Csr(np.zeros(n_rows + 1, np.int32), z, z.copy(), np.zeros(0, f32), np.array([1, 0, 1][:n_rows], np.int32))


def _bare(c, fields=True):
    """The block without its values (and, fields=False, without its field array)."""
    b = copy.copy(c)
    b.__dict__.pop("_ffm_csr_args", None)
    b.val = None
    if not fields:
        b.field = None
    return b


def _own_pages(c):
    """A copy whose arrays own their pages (for pin_block); None stays None."""
    out = copy.copy(c)
    out.__dict__.pop("_ffm_csr_args", None)
    for key in ("row_ptr", "field", "feat", "val", "label"):
        a = getattr(c, key)
        if a is None:
            continue
        b = fa.page_aligned(a.size, a.dtype)
        b[:] = a
        setattr(out, key, b)
    return out


# nnz % 4 = 0, 1, 2, 3 (4, 1, 2, 3 rows of 5 entries; 63 rows: more than one workgroup's worth of lanes), then nnz = 1, 2, 3
REGULAR = [_regular(n, 10 + n) for n in (4, 1, 2, 3, 63)]
SHORT = [_short(n, 20 + n) for n in (1, 2, 3)]
assert [int(c.row_ptr[-1]) % 4 for c in REGULAR] == [0, 1, 2, 3, 3]


def _weights(n, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).choice(np.array([0, 0.25, 1, 3.5], f32), n), f32)


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b))


# ---- engines and paths ----------------------------------------------------------------------------------


def _pair(mt="FFM", k=K, n_fields=F, nf=NF, rows_max=ROWS_MAX, **kw):
    mk = lambda: fa.Engine(mt, nf, n_fields if mt == "FFM" else 1, k, max_batch_rows=rows_max,  # noqa: E731
                           max_batch_nnz=rows_max * n_fields, max_row_nnz=n_fields, seed=9, **dict(STRESS_HP, **kw))
    a, b = mk(), mk()
    for e in (a, b):
        e.fill_state(seed=6)
    return a, b, a.get_state()


def _train(e, path, c, weight):
    """One block through `path`; returns (logits or None, loss sum)."""
    if path == "host":
        return e.train_batch(c, weight=weight)
    if path == "async":
        e.train_batch_async(c, weight=weight)
        return None, e.train_flush()
    if path == "async_zc":
        cb, wb = _own_pages(c), weight
        e.pin_block(cb)
        if weight is not None:
            wb = fa.page_aligned(weight.size, f32)
            wb[:] = weight
            e._check(e.lib.ffm_engine_pin_host(wb.ctypes.data, wb.nbytes))
        try:
            e.train_batch_async_pinned(cb, weight=wb)
            return None, e.train_flush()
        finally:
            e.sync()
            e.unpin_block(cb)
            if weight is not None:
                e.lib.ffm_engine_unpin_host(wb.ctypes.data)
    assert path in ("staged", "staged_zc")
    zc = path == "staged_zc"
    cb, wb = c, weight
    if zc:
        cb = _own_pages(c)
        e.pin_block(cb)
        if weight is not None:
            wb = fa.page_aligned(weight.size, f32)
            wb[:] = weight
            e._check(e.lib.ffm_engine_pin_host(wb.ctypes.data, wb.nbytes))
    out = torch.full((max(c.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    try:
        e.stage_batch(cb, zero_copy=zc, weight=wb)
        e.train_staged(out.data_ptr(), loss.data_ptr())
        e.sync()
    finally:
        if zc:
            e.sync()
            e.unpin_block(cb)
            if weight is not None:
                e.lib.ffm_engine_unpin_host(wb.ctypes.data)
    return out[:c.n_rows].cpu().numpy(), float(loss.cpu()[0])


PATHS = ("host", "async", "async_zc", "staged", "staged_zc")
STAGED_PATHS = PATHS[1:]  # (field=None is the staged calls' convention: the synchronous ones want the array)


def _check_training(a, b, init, bare, full, what, paths=PATHS, weighted=(False, True)):
    """Engine a takes `bare`, engine b `full`, from the same state, through every path."""
    for path in paths:
        for with_w in weighted:
            w = _weights(full.n_rows, 3) if with_w and full.n_rows else None
            tag = "%s, %s%s" % (what, path, ", weighted" if w is not None else "")
            a.set_state(init)
            b.set_state(init)
            lg_a, ls_a = _train(a, path, bare, w)
            lg_b, ls_b = _train(b, path, full, w)
            if lg_a is not None:
                assert_bitwise(lg_a, lg_b, tag + ": logits")
            assert _same_double(ls_a, ls_b), (tag, ls_a, ls_b)
            assert_state_bitwise(a.get_state(), b.get_state(), tag)
            assert_bitwise(get_bias3(a), get_bias3(b), tag + ": bias triple")


def _check_prediction(a, b, bare, full, what):
    """predict_batch, predict_batch_async (pageable and zero_copy) and _async_scores: a on `bare`, b on `full`.
    (A block without its field array: the synchronous call gets the array back.)"""
    sync = bare
    if bare.field is None and full.field is not None:
        sync = _bare(full)
    out_a, ls_a = a.predict_batch(sync, output_prob=True)
    out_b, ls_b = b.predict_batch(full, output_prob=True)
    assert_bitwise(out_a, out_b, what + ": predict_batch")
    assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
    scores = [e.score_buffer(max(full.n_rows, 1)) for e in (a, b)]
    try:
        for zc in (False, True):
            ca, cb = (bare, full) if not zc else (_own_pages(bare), _own_pages(full))
            if zc:
                a.pin_block(ca)
                b.pin_block(cb)
            try:
                a.predict_batch_async(ca, zero_copy=zc)
                b.predict_batch_async(cb, zero_copy=zc)
                la, lb = a.train_flush(), b.train_flush()
                assert _same_double(la, lb), (what, zc, la, lb)
                for s in scores:
                    s[:] = np.nan
                a.predict_batch_async(ca, zero_copy=zc, scores=scores[0], output_prob=True)
                b.predict_batch_async(cb, zero_copy=zc, scores=scores[1], output_prob=True)
                la, lb = a.train_flush(), b.train_flush()
                assert _same_double(la, lb), (what, zc, la, lb)
                assert_bitwise(scores[0][:full.n_rows], scores[1][:full.n_rows], what + ": scores, zero_copy %d" % zc)
                assert_bitwise(scores[0][:full.n_rows], out_a, what + ": scores are predict_batch's")
            finally:
                if zc:
                    a.sync()
                    b.sync()
                    a.unpin_block(ca)
                    b.unpin_block(cb)
    finally:
        for e, s in zip((a, b), scores):
            e.free_score_buffer(s)


# ---- 1. every path, every shape -------------------------------------------------------------------------


def test_ffm_every_path_and_shape():
    a, b, init = _pair()
    for c in REGULAR + SHORT:
        what = "FFM, %d rows, nnz %d" % (c.n_rows, int(c.row_ptr[-1]))
        _check_training(a, b, init, _bare(c), c, what)
        _check_prediction(a, b, _bare(c), c, what)
    a.close()
    b.close()


def test_ffm_without_values_and_without_fields():
    """field=None together with val=None on the staged calls: the yardstick engine gets both arrays spelled out."""
    a, b, init = _pair()
    for c in REGULAR:
        what = "FFM bare, %d rows" % c.n_rows
        _check_training(a, b, init, _bare(c, fields=False), c, what, paths=STAGED_PATHS)
        _check_prediction(a, b, _bare(c, fields=False), c, what)
    # rows that are not one entry per field stay refused, with or without values
    with pytest.raises(fa.EngineError) as ei:
        a.stage_batch(_bare(SHORT[1], fields=False))
    assert ei.value.code == fa.engine.E_INVALID
    a.close()
    b.close()


def test_block_of_empty_rows():
    a, b, init = _pair()
    c = _empty_rows()
    bare = _bare(c)
    assert bare.val is None and int(c.row_ptr[-1]) == 0
    _check_training(a, b, init, bare, c, "empty rows")
    _check_prediction(a, b, bare, c, "empty rows")
    a.close()
    b.close()


@pytest.mark.parametrize("mt,k", [("FM", 8), ("LR", 1)])
def test_fm_and_lr(mt, k):
    a, b, init = _pair(mt, k)
    for c in REGULAR[:4] + SHORT:
        what = "%s, %d rows, nnz %d" % (mt, c.n_rows, int(c.row_ptr[-1]))
        _check_training(a, b, init, _bare(c), c, what, paths=("host", "async", "staged_zc"))
        _check_prediction(a, b, _bare(c), c, what)
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [dict(hash_ids=True), dict(learn=True)], ids=["hashed", "learn"])
def test_hashed_and_learning_engines(kw):
    a, b, init = _pair(**kw)
    for c in REGULAR[1:4]:
        if "hash_ids" in kw:  # raw ids from [0, 2^31): the upload hashes them and writes the ones
            c = copy.copy(c)
            c.feat = np.random.default_rng(5).integers(0, 2 ** 31, c.feat.size, dtype=np.int64).astype(np.int32)
        what = "%s, %d rows" % (list(kw)[0], c.n_rows)
        _check_training(a, b, init, _bare(c), c, what)
        _check_training(a, b, init, _bare(c, fields=False), c, what + ", no fields", paths=("async", "staged_zc"))
        _check_prediction(a, b, _bare(c), c, what)
        _check_prediction(a, b, _bare(c, fields=False), c, what + ", no fields")
    a.close()
    b.close()


def test_beyond_one_grid_stride():
    """701 rows x 39 fields = 27 339 entries (% 4 == 3): more than the upload kernel's grid covers in one
    stride of four values per lane."""
    n_fields, per, rows = 39, 50, 701
    grid_pull = int(os.environ.get("FFM_GRID_PULL", "24"))
    c = _regular(rows, 77, n_fields, per)
    nnz = int(c.row_ptr[-1])
    assert nnz == 27339 and nnz % 4 == 3
    assert grid_pull != 24 or nnz > grid_pull * 256 * 4
    a, b, init = _pair(n_fields=n_fields, nf=n_fields * per, rows_max=rows)
    _check_training(a, b, init, _bare(c), c, "27339 entries", paths=("host", "async", "staged_zc"), weighted=(False,))
    _check_training(a, b, init, _bare(c, fields=False), c, "27339 entries, no fields", paths=("async_zc", "staged"), weighted=(True,))
    _check_prediction(a, b, _bare(c), c, "27339 entries")
    a.close()
    b.close()


# ---- 2. against the oracle ------------------------------------------------------------------------------


@pytest.mark.parametrize("mt,k", [("FFM", 4), ("FM", 8)])
def test_against_the_oracle_on_the_explicit_array(mt, k):
    c = REGULAR[4]
    if mt != "FFM":
        c = copy.copy(c)
        c.field = np.zeros_like(c.field)
    nfld = F if mt == "FFM" else 1
    o = CpuModel("oracle", mt, NF, nfld, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(21), o, n_hi=1e-4, w_sd=0.5)  # (as test_block_semantics._fold_case)
    o.set_state(st)
    want_lg, want_loss = o.train_batch(c)
    want = o.get_state()
    want_p, want_pl = o.predict_batch(c)
    for path in ("host", "async", "staged"):
        e = fa.Engine(mt, NF, nfld, k, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F, skip_init=True,
                      **STRESS_HP)
        e.set_state(st)
        lg, ls = _train(e, path, _bare(c), None)
        if lg is not None:
            assert_bitwise(lg, want_lg, path + ": logits against the oracle")
        assert loss_close(ls, want_loss), (path, ls, want_loss)
        assert_state_bitwise(e.get_state(), want, path + ": state against the oracle")
        got_p, got_pl = e.predict_batch(_bare(c))
        assert_bitwise(got_p, want_p, path + ": predictions against the oracle")
        assert loss_close(got_pl, want_pl), (path, got_pl, want_pl)
        e.close()


# ---- 3. stale slots -------------------------------------------------------------------------------------


def _stale_sequence():
    """(rows, valued) per block: the first seeded draw in which every staging slot (block i uses slot i mod
    SLOTS) is refilled valued -> bare with a shorter and with a longer successor, and bare -> valued."""
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        n = 9 * SLOTS
        rows = rng.integers(1, ROWS_MAX + 1, n)
        valued = rng.random(n) < 0.5
        ok = True
        for s in range(SLOTS):
            seq = [(bool(valued[i]), int(rows[i])) for i in range(s, n, SLOTS)]
            steps = list(zip(seq[:-1], seq[1:]))
            ok = ok and any(p[0] and not q[0] and q[1] < p[1] for p, q in steps)
            ok = ok and any(p[0] and not q[0] and q[1] > p[1] for p, q in steps)
            ok = ok and any(not p[0] and q[0] for p, q in steps)
            ok = ok and any(not p[0] and not q[0] and q[1] > p[1] for p, q in steps)
        if ok:
            return rows.tolist(), valued.tolist()
    raise AssertionError("no seed gives the wanted sequence")


@pytest.mark.parametrize("zero_copy", [False, True], ids=["pageable", "zero_copy"])
def test_stale_slots_in_one_pipeline(zero_copy):
    """Blocks that bring values drawn from [0.5, 2) and blocks without values share the four staging slots
    over nine turns; the yardstick gets the same sequence with the ones spelled out."""
    rows, valued = _stale_sequence()
    assert len(rows) >= 9 and len(rows) > 2 * SLOTS
    rng = np.random.default_rng(2)
    full, handed = [], []
    for i, (n, v) in enumerate(zip(rows, valued)):
        vals = (0.5 + 1.5 * rng.random(n * F)).astype(f32) if v else None
        c = _regular(n, 100 + i, val=vals)
        full.append(c)
        handed.append(c if v else _bare(c))
    a, b, init = _pair()
    if zero_copy:
        handed, full = [_own_pages(c) for c in handed], [_own_pages(c) for c in full]
        for ca, cb in zip(handed, full):
            a.pin_block(ca)
            b.pin_block(cb)
    try:
        for e, blocks in ((a, handed), (b, full)):
            for c in blocks:
                if zero_copy:
                    e.train_batch_async_pinned(c)
                else:
                    e.train_batch_async(c)
        la, lb = a.train_flush(), b.train_flush()
        assert _same_double(la, lb), (la, lb)
        assert_state_bitwise(a.get_state(), b.get_state(), "after the training pipeline")
        # the same sequence once more as an evaluation pipeline with scores
        bufs = [[e.score_buffer(ROWS_MAX) for _ in rows] for e in (a, b)]
        for e, blocks, out in ((a, handed, bufs[0]), (b, full, bufs[1])):
            for c, s in zip(blocks, out):
                s[:] = np.nan
                e.predict_batch_async(c, zero_copy=zero_copy, scores=s)
        la, lb = a.train_flush(), b.train_flush()
        assert _same_double(la, lb), (la, lb)
        for i, n in enumerate(rows):
            assert_bitwise(bufs[0][i][:n], bufs[1][i][:n], "scores of block %d" % i)
            assert not np.isnan(bufs[0][i][:n]).any()
        for e, out in zip((a, b), bufs):
            for s in out:
                e.free_score_buffer(s)
    finally:
        if zero_copy:
            a.sync()
            b.sync()
            for ca, cb in zip(handed, full):
                a.unpin_block(ca)
                b.unpin_block(cb)
    a.close()
    b.close()


# ---- 4. serving engines and groups ----------------------------------------------------------------------


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_serving_engines(fmt):
    t = fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F, seed=9, **STRESS_HP)
    t.fill_state(seed=6)
    mk = lambda: fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F,  # noqa: E731
                           serve=fmt, skip_init=True, **STRESS_HP)
    a, b = mk(), mk()
    a.pack_from(t)
    b.pack_from(t)
    for c in REGULAR + SHORT:
        what = "serve %s, %d rows, nnz %d" % (fmt, c.n_rows, int(c.row_ptr[-1]))
        _check_prediction(a, b, _bare(c), c, what)
    for c in REGULAR:
        _check_prediction(a, b, _bare(c, fields=False), c, "serve %s, %d rows, no fields" % (fmt, c.n_rows))
    for e in (a, b, t):
        e.close()


def test_group_of_two_engines():
    mk = lambda: fa.Group([0, 0], "FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F,  # noqa: E731
                          seed=4, **STRESS_HP)
    ga, gb = mk(), mk()
    for c in REGULAR:
        for bare in (_bare(c), _bare(c, fields=False)):
            lg_a, ls_a = ga.train_batch(bare)
            lg_b, ls_b = gb.train_batch(c)
            assert_bitwise(lg_a, lg_b, "group train_batch logits")
            assert _same_double(ls_a, ls_b), (ls_a, ls_b)
            w = _weights(c.n_rows, 8)
            lg_a, ls_a = ga.train_batch(bare, weight=w)
            lg_b, ls_b = gb.train_batch(c, weight=w)
            assert_bitwise(lg_a, lg_b, "group train_batch_weighted logits")
            assert _same_double(ls_a, ls_b), (ls_a, ls_b)
            ga.train_batch_async(bare)
            gb.train_batch_async(c)
            la, lb = ga.train_flush(), gb.train_flush()
            assert _same_double(la, lb), (la, lb)
            p_a, pl_a = ga.predict_batch(_bare(c), output_prob=True)  # (synchronous: with the field array)
            p_b, pl_b = gb.predict_batch(c, output_prob=True)
            assert_bitwise(p_a, p_b, "group predict_batch")
            assert _same_double(pl_a, pl_b), (pl_a, pl_b)
    for ea, eb in zip(ga.engines, gb.engines):
        assert_state_bitwise(ea.get_state(), eb.get_state(), "group rank state")
    ga.close()
    gb.close()


# ---- 5. the metrics channels ----------------------------------------------------------------------------


def test_metrics_channels():
    a, b, init = _pair()
    for e in (a, b):
        e.set_state(init)
        e.metrics_enable(eval=True, train=True)
    c = REGULAR[4]
    for e, blk in ((a, _bare(c)), (b, c)):
        e.train_batch(blk)
        e.train_batch_async(blk)
        e.train_flush()
        e.predict_batch(blk)
        e.predict_batch_async(blk)
        e.train_flush()
    for ch in ("train", "eval"):
        (pa, na), (pb, nb) = a.metrics_histogram(ch), b.metrics_histogram(ch)
        assert pa.sum() + na.sum() == 2 * c.n_rows, ch
        assert np.array_equal(pa, pb) and np.array_equal(na, nb), ch
    a.close()
    b.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------


def test_device_entry_points_refuse():
    """The _device entry points and prepare_device take arrays as they are: val == NULL with nnz > 0 stays
    FFM_E_INVALID there, and the engine goes on working."""
    c = REGULAR[3]
    e = fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F, seed=9, **STRESS_HP)
    d = {k: torch.from_numpy(getattr(c, k)).cuda() for k in ("row_ptr", "field", "feat", "val", "label")}
    out = torch.zeros(c.n_rows, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    n, nnz = c.n_rows, int(c.row_ptr[-1])
    rp, fld, ft, lab = (d[k].data_ptr() for k in ("row_ptr", "field", "feat", "label"))
    calls = {
        "train_batch_device": lambda: e.train_batch_device(n, nnz, rp, fld, ft, None, lab),
        "predict_batch_device": lambda: e.predict_batch_device(n, nnz, rp, fld, ft, None, lab, False, out.data_ptr()),
        "prepare_device": lambda: e.prepare_device(n, nnz, rp, fld, ft, None),
        "train_forward_device": lambda: e.train_forward_device(n, nnz, rp, fld, ft, None, lab, None),
    }
    for name, call in calls.items():
        with pytest.raises(fa.EngineError) as ei:
            call()
        assert ei.value.code == fa.engine.E_INVALID, name
        assert "null CSR array" in str(ei.value), (name, str(ei.value))
    assert e.changed_features().size == 0, "a refused block must leave the model untouched"
    e.train_batch_device(n, nnz, rp, fld, ft, d["val"].data_ptr(), lab)  # the same block with its values
    e.sync()
    assert e.changed_features().size > 0
    e.close()


# ---- 7. blocks that bring values change nothing ---------------------------------------------------------


def _profile_lines(e):
    """{label: launches} of the engine's profile."""
    out = {}
    for ln in e.profile_dump().splitlines():
        if "launches=" in ln:
            out[ln.split()[0]] = int(ln.split("launches=")[1].split()[0])
    return out


def test_profile_labels_are_unchanged():
    """With profiling on, a block WITH its values shows the labels and launch counts it always did: the
    upload carries no label of its own (before and after), and neither fill kernel appears under one -- a
    block without values lists exactly the same labels and counts."""
    a, b, init = _pair()
    c = REGULAR[4]
    for e, blk in ((a, _bare(c)), (b, c)):
        e.set_state(init)
        e.profile_enable(True)
        e.train_batch(blk)
        e.train_batch_async(blk)
        e.train_flush()
        e.predict_batch(blk)
        e.predict_batch_async(blk)
        e.train_flush()
    la, lb = _profile_lines(a), _profile_lines(b)
    assert lb and la == lb, (la, lb)
    assert not any("pull_block" in k or "fill_" in k or "ones" in k for k in lb), lb
    a.close()
    b.close()
