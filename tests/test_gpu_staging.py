"""The per-block path that carries host rows onto the device (csrc/kernels_stage.h: pull_block_kernel's eight
instantiations; csrc/engine_stage.h: claim_slot, launch_upload, slot_commit).

1. Every upload variant -- weights {none, given} x hash_ids {off, on} x val {given, None} x field {given, None}
   -- against the SYNCHRONOUS calls, which move the same block with hipMemcpyAsync, fill_ones_kernel and
   hash_ids_kernel and share no code with the upload kernel: logits (where the path returns them), the loss sum
   and the whole state after train_batch equal those after stage_batch + train_staged (pageable and zero-copy)
   and after train_batch_async + train_flush, bit for bit; predict_batch equals the scores of
   predict_batch_async, bit for bit, with nothing written behind the block.
   Blocks (FFM, 5 fields, k = 4): 4, 1, 2, 3 and 63 rows of one entry per field (nnz % 4 = 0, 1, 2, 3, 3 and
   n_rows % 4 = 0, 1, 2, 3, 3: every 16-byte tail of the five arrays and of the weight array), one ragged block
   with its field array, one block of 0 rows.
2. A refused call leaves nothing behind: after a host block was refused behind its validation, the next
   _device call on that engine behaves as on an engine that never saw the refused block (the row kernels are
   sized by an argument of the call, not by what an earlier call left in the engine).
"""
import copy

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise, get_bias3

pytestmark = pytest.mark.gpu

f32 = np.float32
F, K, PER = 5, 4, 40
NF = F * PER
ROWS_MAX = 64
CANARY = np.uint32(0xC0FFEE42)
PAD = 8


# ---- blocks ---------------------------------------------------------------------------------------------


def _regular(n_rows, seed):
    """One entry per field and row, fields in order; values from [0.5, 2)."""
    rng = np.random.default_rng(seed)
    feat = (rng.integers(0, PER, (n_rows, F)) + np.arange(F)[None, :] * PER).astype(np.int32)
    field = np.broadcast_to(np.arange(F, dtype=np.int32), (n_rows, F)).reshape(-1).copy()
    row_ptr = (np.arange(n_rows + 1, dtype=np.int64) * F).astype(np.int32)
    val = (0.5 + 1.5 * rng.random(n_rows * F)).astype(f32)
    return Csr(row_ptr, field, feat.reshape(-1), val, (rng.random(n_rows) < 0.4).astype(np.int32))


def _ragged(seed):
    """Seven rows of 0 .. 5 entries, fields in any order and some twice: 19 entries."""
    rng = np.random.default_rng(seed)
    lens = np.array([3, 0, 5, 1, 4, 2, 4], np.int64)
    field = np.concatenate([rng.integers(0, F, n) for n in lens]).astype(np.int32)
    feat = (field * PER + rng.integers(0, PER, field.size)).astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    val = (0.5 + 1.5 * rng.random(field.size)).astype(f32)
    return Csr(row_ptr, field, feat, val, (rng.random(lens.size) < 0.4).astype(np.int32))


def _no_rows():
    z = np.zeros(0, np.int32)
    return Csr(np.zeros(1, np.int32), z, z.copy(), np.zeros(0, f32), z.copy())


REGULAR = [_regular(n, 30 + n) for n in (4, 1, 2, 3, 63)]
assert [int(c.row_ptr[-1]) % 4 for c in REGULAR] == [0, 1, 2, 3, 3] and [c.n_rows % 4 for c in REGULAR] == [0, 1, 2, 3, 3]
BLOCKS = [(c, True) for c in REGULAR] + [(_ragged(50), False), (_no_rows(), False)]  # (block, one entry per field)
assert int(BLOCKS[5][0].row_ptr[-1]) == 19


def _variant(i, hashed, valued, fields=True):
    """Block i as a variant hands it over: raw ids from [0, 2^31) for a hashing engine, val / field None.
    (Ids and weights are drawn per block: what an earlier block left in a staging slot never equals what an
    upload that skips a tail should have written.)"""
    c = BLOCKS[i][0]
    b = copy.copy(c)
    b.__dict__.pop("_ffm_csr_args", None)
    if hashed:
        b.feat = np.random.default_rng(500 + i).integers(0, 2 ** 31, c.feat.size, dtype=np.int64).astype(np.int32)
    if not valued:
        b.val = None
    if not fields:
        b.field = None
    return b


def _own_pages(a):
    if a is None:
        return None
    out = fa.page_aligned(a.size, a.dtype)
    out[:] = a
    return out


def _own_pages_block(c):
    out = copy.copy(c)
    out.__dict__.pop("_ffm_csr_args", None)
    for key in ("row_ptr", "field", "feat", "val", "label"):
        setattr(out, key, _own_pages(getattr(c, key)))
    return out


def _weights(i):
    n = BLOCKS[i][0].n_rows
    return np.ascontiguousarray(np.random.default_rng(300 + i).choice(np.array([0, 0.25, 0.5, 1, 2, 3.5], f32), n), f32)


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ---- engines --------------------------------------------------------------------------------------------


def _engine(**kw):
    return fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F, seed=9,
                     **dict(STRESS_HP, **kw))


def _twins(**kw):
    """Twin engines that start from one fill_state, and that state."""
    x, y = _engine(**kw), _engine(**kw)
    for e in (x, y):
        e.fill_state(seed=6)
    return x, y, x.get_state()


def _train_staged(e, c, weight, zero_copy):
    """stage_batch + train_staged; returns (logits, loss sum)."""
    cb, wb = c, weight
    if zero_copy:
        cb = _own_pages_block(c)
        e.pin_block(cb)
        if weight is not None and weight.size:
            wb = _own_pages(weight)
            e._check(e.lib.ffm_engine_pin_host(wb.ctypes.data, wb.nbytes))
    out = torch.full((max(c.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    try:
        e.stage_batch(cb, zero_copy=zero_copy, weight=wb)
        e.train_staged(out.data_ptr(), loss.data_ptr())
        e.sync()
    finally:
        if zero_copy:
            e.sync()
            e.unpin_block(cb)
            if wb is not weight:
                e.lib.ffm_engine_unpin_host(wb.ctypes.data)
    return out[:c.n_rows].cpu().numpy(), float(loss.cpu()[0])


def _train(e, path, c, weight):
    if path == "async":
        e.train_batch_async(c, weight=weight)
        return None, e.train_flush()
    return _train_staged(e, c, weight, path == "staged_zc")


# ---- 1. every upload variant against the synchronous path -----------------------------------------------


@pytest.mark.parametrize("hashed", [False, True], ids=["raw", "hashed"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_training_upload_variants_match_the_synchronous_call(weighted, hashed):
    x, y, init = _twins(hash_ids=hashed)
    for i, (c, one_per_field) in enumerate(BLOCKS):
        w = _weights(i) if weighted else None
        for valued in (True, False):
            # the yardstick, once per (block, val): the synchronous call always gets the field array
            x.set_state(init)
            want_lg, want_ls = x.train_batch(_variant(i, hashed, valued), weight=w)
            want_st, want_b3 = x.get_state(), get_bias3(x)
            assert np.isfinite(want_lg).all() and np.isfinite(want_ls)
            for fields in ((True, False) if one_per_field else (True,)):
                blk = _variant(i, hashed, valued, fields)
                for path in ("staged", "staged_zc", "async"):
                    tag = "block %d (%d rows, nnz %d), val %s, field %s, %s" % (
                        i, c.n_rows, int(c.row_ptr[-1]), "given" if valued else "None", "given" if fields else "None", path)
                    y.set_state(init)
                    lg, ls = _train(y, path, blk, w)
                    if lg is not None:
                        assert_bitwise(lg, want_lg, tag + ": logits")
                    assert _same_double(ls, want_ls), (tag, ls, want_ls)
                    assert_state_bitwise(y.get_state(), want_st, tag)
                    assert_bitwise(get_bias3(y), want_b3, tag + ": bias triple")
    x.close()
    y.close()


@pytest.mark.parametrize("hashed", [False, True], ids=["raw", "hashed"])
def test_prediction_upload_variants_match_the_synchronous_call(hashed):
    x, y, _ = _twins(hash_ids=hashed)
    buf = y.score_buffer(ROWS_MAX + PAD)
    try:
        for i, (c, one_per_field) in enumerate(BLOCKS):
            n = c.n_rows
            for valued in (True, False):
                want, want_ls = x.predict_batch(_variant(i, hashed, valued), output_prob=True)
                assert np.isfinite(want).all()
                for fields in ((True, False) if one_per_field else (True,)):
                    blk = _variant(i, hashed, valued, fields)
                    for zc in (False, True):
                        tag = "block %d (%d rows), val %s, field %s, zero_copy %d" % (
                            i, n, "given" if valued else "None", "given" if fields else "None", zc)
                        cb = _own_pages_block(blk) if zc else blk
                        if zc:
                            y.pin_block(cb)
                        buf.view(np.uint32)[:] = CANARY
                        try:
                            y.predict_batch_async(cb, zero_copy=zc, scores=buf, output_prob=True)
                            ls = y.train_flush()
                        finally:
                            if zc:
                                y.sync()
                                y.unpin_block(cb)
                        assert_bitwise(buf[:n], want, tag + ": scores")
                        assert (buf.view(np.uint32)[n:] == CANARY).all(), tag + ": written behind the block"
                        assert _same_double(ls, want_ls), (tag, ls, want_ls)
    finally:
        y.free_score_buffer(buf)
    x.close()
    y.close()


# ---- 2. a refused call leaves nothing behind ------------------------------------------------------------


def _short():
    """4 ragged rows of 2 entries."""
    rng = np.random.default_rng(70)
    field = np.array([0, 3, 1, 2, 4, 0, 2, 3], np.int32)
    feat = (field * PER + rng.integers(0, PER, 8)).astype(np.int32)
    return Csr(np.arange(0, 9, 2, dtype=np.int32), field, feat, np.ones(8, f32), np.array([1, 0, 0, 1], np.int32))


class _Long:
    """4 rows of 5 entries, already in device arrays."""

    def __init__(self):
        c = REGULAR[0]
        self.c, self.n, self.nnz = c, c.n_rows, int(c.row_ptr[-1])
        self.d = {k: torch.from_numpy(getattr(c, k)).cuda() for k in ("row_ptr", "field", "feat", "val", "label")}
        torch.cuda.synchronize()

    def args(self, label=True):
        d = self.d
        return (self.n, self.nnz, d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(), d["val"].data_ptr(),
                d["label"].data_ptr() if label else None)


def _refuse_without_labels(e):
    short = _short()
    short.label = None
    with pytest.raises(fa.EngineError) as ei:
        e.train_batch(short)
    assert ei.value.code == fa.engine.E_INVALID and "training needs labels" in str(ei.value), str(ei.value)


def _out(n):
    return torch.zeros(n, dtype=torch.float32, device="cuda")


def test_refused_training_block_leaves_the_next_device_step_alone():
    a, b, _ = _twins()
    long = _Long()
    _refuse_without_labels(a)
    lg = [_out(long.n), _out(long.n)]
    for e, o in zip((a, b), lg):
        e.train_batch_device(*long.args(), logit_out=o.data_ptr())
        e.sync()  # (raises where the device flagged a row longer than the row kernel was sized for)
    la, lb = (o.cpu().numpy() for o in lg)
    assert np.isfinite(la).all(), la
    assert_bitwise(la, lb, "logits after a refused block")
    assert_state_bitwise(a.get_state(), b.get_state(), "state after a refused block")
    a.close()
    b.close()


def test_refused_block_on_a_shard_leaves_the_next_forward_alone():
    a, b = (_engine(n_shards=2, shard_rank=0) for _ in range(2))
    long = _Long()
    with pytest.raises(fa.EngineError) as ei:
        a.train_batch(_short())
    assert ei.value.code == fa.engine.E_INVALID and "sharded engines train with" in str(ei.value), str(ei.value)
    part = [_out(long.n), _out(long.n)]
    for e, o in zip((a, b), part):
        e.train_forward_device(*long.args(), o.data_ptr())
        e.sync()
    pa, pb = (o.cpu().numpy() for o in part)
    assert np.isfinite(pa).all(), pa
    assert_bitwise(pa, pb, "partial logits after a refused block")
    for e, o in zip((a, b), part):  # (the step's second half, so that nothing is left pending)
        e.train_update_device(o.data_ptr())
        e.sync()
    a.close()
    b.close()


def test_refused_block_leaves_the_next_device_prediction_alone():
    a, b, _ = _twins()
    long = _Long()
    _refuse_without_labels(a)
    out = [_out(long.n), _out(long.n)]
    for e, o in zip((a, b), out):
        e.predict_batch_device(*long.args(label=False), False, o.data_ptr())
        e.sync()
    oa, ob = (o.cpu().numpy() for o in out)
    assert np.isfinite(oa).all(), oa
    assert_bitwise(oa, ob, "predictions after a refused block")
    a.close()
    b.close()
