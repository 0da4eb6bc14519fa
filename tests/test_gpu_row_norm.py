"""FFM_FLAG_NORM_ROWS (include/ffm_engine.h "Normalised rows"): every row of a host block scaled to unit length on the
device, on every entry point that takes rows in host memory.

The yardstick is the one of test_gpu_implicit_ones.py: two engines of the same config and seed, both after
fill_state; one is flagged (normalize=True) and fed the raw blocks, the other is unflagged and fed
fa.normalize_rows(...) of them.  Logits, loss sums, scores and the whole state (every touched feature, every
untouched one, the bias triple) must be equal bit for bit, NaN positions included.  One FFM and one FM case also go
against the oracle on the pre-normalised array, so that the pair cannot be wrong together.

Shapes (FFM 5 fields x k = 4, 40 ids per field; FM k = 8; LR): 1, 2, 3, 4 and 63 regular rows (nnz % 4 in 0 .. 3),
empty rows only, a ragged block of row lengths 0, 1, 2, 63, 64, 65, 129, the edge rows of tests/test_row_norm_host.py
(subnormal, underflowing and overflowing sums, NaN, zeros), erased entries, val=None.  The kernel takes a run of 64
consecutive rows per workgroup and holds a run of up to 4096 entries in LDS (csrc/kernels_norm.h), so beyond one tile
means: 600 rows (ten runs, the last one partial; with FFM_GRID_NORM=2 each workgroup strides over five runs), and
100 rows x 129 entries, whose runs of 64 x 129 = 8256 entries take the kernel's plain path through global memory.
"""
import copy
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from test_gpu_implicit_ones import _check_prediction, _check_training, _own_pages, _same_double, _train
from util import STRESS_HP, assert_bitwise, assert_state_bitwise, loss_close, rand_state

pytestmark = pytest.mark.gpu

f32 = np.float32
F, K, PER = 5, 4, 40
NF = F * PER
ROWS_MAX, ROW_NNZ = 64, 129


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _variant(c, **kw):
    h = copy.copy(c)
    h.__dict__.pop("_ffm_csr_args", None)
    for key, v in kw.items():
        setattr(h, key, v)
    return h


# ---- blocks ---------------------------------------------------------------------------------------------


def _regular(n_rows, seed):
    """One entry per field and row, log-normal values (sigma = 2)."""
    rng = np.random.default_rng(seed)
    feat = (rng.integers(0, PER, (n_rows, F)) + np.arange(F)[None, :] * PER).astype(np.int32)
    field = np.broadcast_to(np.arange(F, dtype=np.int32), (n_rows, F)).reshape(-1).copy()
    row_ptr = (np.arange(n_rows + 1, dtype=np.int64) * F).astype(np.int32)
    return Csr(row_ptr, field, feat.reshape(-1), rng.lognormal(0.0, 2.0, n_rows * F).astype(f32), (rng.random(n_rows) < 0.4).astype(np.int32))


def _ragged(lengths, seed):
    rng = np.random.default_rng(seed)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(row_ptr[-1])
    field = rng.integers(0, F, n).astype(np.int32)
    feat = (rng.integers(0, PER, n) + field * PER).astype(np.int32)
    return Csr(row_ptr, field, feat, rng.lognormal(0.0, 2.0, n).astype(f32), (rng.random(len(lengths)) < 0.4).astype(np.int32))


def _edge():
    """The edge rows of tests/test_row_norm_host.py, then two ordinary rows."""
    rows = [[1e-20, 2e-20], [1e-30], [3e19, 3e19], [np.nan, 1.0], [0.0, 0.0], [2.5], [], [0.5, 3.0, 1.5], [4.0]]
    rng = np.random.default_rng(4)
    return Csr.from_rows([[(j % F, int(rng.integers(0, PER)) + (j % F) * PER, v) for j, v in enumerate(r)] for r in rows],
                         [1, 0, 1, 0, 1, 1, 0, 1, 0])


EDGE_UNSCALED = 5  # 1e-30, (3e19, 3e19), (nan, 1), (0, 0) and the empty row


def _erased(seed):
    """16 rows of 7 entries; about a quarter of the entries are erased: feat = -1, feat = n_feats, field = n_fields, field = -1."""
    c = _ragged([7] * 16, seed)
    rng = np.random.default_rng(seed + 1)
    kind = rng.integers(0, 16, c.feat.size)
    c.feat[kind == 0] = -1
    c.feat[kind == 1] = NF
    c.field[kind == 2] = F
    c.field[kind == 3] = -1
    return c


def _empty_rows():
    z = np.zeros(0, np.int32)
    return Csr(np.zeros(4, np.int32), z, z.copy(), np.zeros(0, f32), np.array([1, 0, 1], np.int32))


@functools.lru_cache(maxsize=None)
def _blocks():
    d = {"regular %d" % n: _regular(n, 10 + n) for n in (4, 1, 2, 3, 63)}
    assert [int(c.row_ptr[-1]) % 4 for c in d.values()] == [0, 1, 2, 3, 3]
    d["empty rows"] = _empty_rows()
    d["ragged"] = _ragged([0, 1, 2, 63, 64, 65, 129], 31)
    d["edge"] = _edge()
    d["erased"] = _erased(41)
    return d


def _norm(c, mt="FFM", val="own"):
    """The block the unflagged engine takes: fa.normalize_rows of the values (val=None: of the ones they stand for)."""
    v = c.val if isinstance(val, str) else val
    return _variant(c, val=fa.normalize_rows(c.row_ptr, c.field, c.feat, v, NF, F if mt == "FFM" else None, model=mt))


# ---- engines --------------------------------------------------------------------------------------------


def _pair(mt="FFM", k=K, rows_max=ROWS_MAX, row_nnz=ROW_NNZ, nnz_max=None, **kw):
    """(flagged, unflagged, the state both start from)."""
    mk = lambda **more: fa.Engine(mt, NF, F if mt == "FFM" else 1, k, max_batch_rows=rows_max,  # noqa: E731
                                  max_batch_nnz=nnz_max or rows_max * 8 + 2 * row_nnz, max_row_nnz=row_nnz, seed=9, **dict(STRESS_HP, **kw), **more)
    a, b = mk(normalize=True), mk()
    for e in (a, b):
        e.fill_state(seed=6)
    init = a.get_state()
    assert_state_bitwise(b.get_state(), init, "twin engines")
    return a, b, init


# ---- 1. every path, every shape -------------------------------------------------------------------------


def test_ffm_every_path_and_shape():
    a, b, init = _pair()
    for name, c in _blocks().items():
        h = _norm(c)
        if c.val.size and name != "edge":
            assert not np.array_equal(_bits(h.val), _bits(c.val)), name
        _check_training(a, b, init, c, h, "FFM, " + name)
        _check_prediction(a, b, c, h, "FFM, " + name)
    assert b.norm_stats() == (0, 0), "an unflagged engine normalises nothing"
    a.close()
    b.close()


@pytest.mark.parametrize("mt,k", [("FM", 8), ("LR", 1)])
def test_fm_and_lr(mt, k):
    a, b, init = _pair(mt, k)
    for name in ("regular 4", "regular 1", "regular 2", "regular 3", "ragged", "edge", "erased", "empty rows"):
        c = _blocks()[name]
        h = _norm(c, mt)
        _check_training(a, b, init, c, h, "%s, %s" % (mt, name), paths=("host", "async", "staged_zc"))
        _check_prediction(a, b, c, h, "%s, %s" % (mt, name))
    a.close()
    b.close()


def test_rows_without_values():
    """val=None on the flagged engine: the yardstick gets fa.normalize_rows of the ones."""
    a, b, init = _pair()
    for name in ("regular 3", "regular 63", "ragged", "erased"):
        c = _blocks()[name]
        h = _norm(c, val=None)
        assert h.val.size and np.all(h.val[c.row_ptr[0]:c.row_ptr[1]] <= 1.0)
        _check_training(a, b, init, _variant(c, val=None), h, name + ", val=None", weighted=(False,))
        _check_prediction(a, b, _variant(c, val=None), h, name + ", val=None")
    c = _blocks()["regular 63"]  # field=None too, on the staged calls
    bare = _variant(c, val=None, field=None)
    _check_training(a, b, init, bare, _norm(c, val=None), "regular 63, bare", paths=("async", "staged_zc"), weighted=(True,))
    a.close()
    b.close()


def test_learning_engine():
    a, b, init = _pair(learn=True)
    for name in ("regular 63", "erased"):
        c = _blocks()[name]
        _check_training(a, b, init, c, _norm(c), "learn, " + name, paths=("host", "staged"))
    a.close()
    b.close()


def test_beyond_one_run_and_beyond_the_lds_tile(monkeypatch):
    """600 rows: ten runs of the kernel's 64, the last one partial -- once with a workgroup per run, once with
    FFM_GRID_NORM=2, where each workgroup strides over five runs.  100 rows x 129 entries: runs of 8256 entries,
    more than the 4096 the kernel holds in LDS: its plain path (the second run, 36 rows = 4644 entries, too)."""
    many = _ragged(np.random.default_rng(8).integers(0, 9, 600).tolist(), 51)
    wide = _ragged([129] * 100, 52)
    assert 36 * 129 > 4096 and many.n_rows > 2 * 64 * 2
    for grid in (None, "2"):
        if grid:
            monkeypatch.setenv("FFM_GRID_NORM", grid)
        a, b, init = _pair(rows_max=600, nnz_max=13000)
        for name, c in (("600 rows", many), ("100 x 129", wide)):
            h = _norm(c)
            _check_training(a, b, init, c, h, name, paths=("host", "async_zc"), weighted=(False,))
            _check_prediction(a, b, c, h, name)
        a.close()
        b.close()


# ---- 2. against the oracle ------------------------------------------------------------------------------


@pytest.mark.parametrize("mt,k", [("FFM", 4), ("FM", 8)])
def test_against_the_oracle_on_the_normalised_array(mt, k):
    c = _blocks()["regular 63"]
    if mt != "FFM":
        c = _variant(c, field=np.zeros_like(c.field))
    h = _norm(c, mt)
    nfld = F if mt == "FFM" else 1
    o = CpuModel("oracle", mt, NF, nfld, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(21), o, n_hi=1e-4, w_sd=0.5)
    o.set_state(st)
    want_lg, want_loss = o.train_batch(h)
    want = o.get_state()
    want_p, want_pl = o.predict_batch(h)
    for path in ("host", "async", "staged"):
        e = fa.Engine(mt, NF, nfld, k, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * F, max_row_nnz=F, skip_init=True,
                      normalize=True, **STRESS_HP)
        e.set_state(st)
        lg, ls = _train(e, path, c, None)
        if lg is not None:
            assert_bitwise(lg, want_lg, path + ": logits against the oracle")
        assert loss_close(ls, want_loss), (path, ls, want_loss)
        assert_state_bitwise(e.get_state(), want, path + ": state against the oracle")
        got_p, got_pl = e.predict_batch(c)
        assert_bitwise(got_p, want_p, path + ": predictions against the oracle")
        assert loss_close(got_pl, want_pl), (path, got_pl, want_pl)
        e.close()


# ---- 3. ablation, serving, hashed engines ---------------------------------------------------------------


def test_predict_ablated_drops_a_field_after_normalising():
    a, b, _ = _pair(row_nnz=128, rows_max=ROWS_MAX)
    a.ablation_enable()
    b.ablation_enable()
    for name in ("regular 63", "erased", "edge"):
        c = _blocks()[name]
        h = _norm(c)
        out_a, ls_a = a.predict_ablated(c, output_prob=True)
        out_b, ls_b = b.predict_ablated(h, output_prob=True)
        assert_bitwise(out_a, out_b, name + ": ablated scores")
        assert all(_same_double(x, y) for x, y in zip(ls_a, ls_b)), (name, ls_a, ls_b)
        for v in range(F):  # variant v: the NORMALISED block without field v -- the norm is not recomputed
            want, _ = b.predict_batch(fa.drop_field(h, v), output_prob=True)
            assert_bitwise(out_a[v], want, "%s: without field %d" % (name, v))
    a.close()
    b.close()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_serving_engines(fmt):
    kw = dict(max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * 8, max_row_nnz=128, **STRESS_HP)
    t = fa.Engine("FFM", NF, F, K, seed=9, **kw)
    t.fill_state(seed=6)
    a = fa.Engine("FFM", NF, F, K, serve=fmt, skip_init=True, normalize=True, **kw)
    b = fa.Engine("FFM", NF, F, K, serve=fmt, skip_init=True, **kw)
    a.pack_from(t)
    b.pack_from(t)
    for name in ("regular 4", "regular 1", "regular 2", "regular 3", "regular 63", "edge", "erased", "empty rows"):
        c = _blocks()[name]
        _check_prediction(a, b, c, _norm(c), "serve %s, %s" % (fmt, name))
    c = _blocks()["regular 63"]
    _check_prediction(a, b, _variant(c, val=None), _norm(c, val=None), "serve %s, val=None" % fmt)
    # scoring candidates would need a scale per candidate: refused before anything is queued
    ctx = Csr(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3], np.int32), np.ones(1, f32), np.zeros(1, np.int32))
    cand = Csr(np.array([0, 1], np.int32), np.array([1], np.int32), np.array([PER + 3], np.int32), np.ones(1, f32), np.zeros(1, np.int32))
    with pytest.raises(fa.EngineError, match="scale per candidate") as ei:
        a.score_candidates(ctx, np.array([0, 1], np.int32), cand)
    assert ei.value.code == fa.engine.E_INVALID
    assert b.score_candidates(ctx, np.array([0, 1], np.int32), cand).shape == (1,)
    for e in (a, b, t):
        e.close()


def test_hashed_engine_with_keep_map_and_buckets():
    """A flagged hashed engine with a keep-map and a bucket table on raw blocks, against fa.bucket_ids / fold_rare /
    hash_ids followed by fa.normalize_rows on the host: buckets count as the 1 they become, and the ids that decide
    what a row keeps are the hashed ones."""
    import test_gpu_value_buckets as vb
    table, words = vb._table(False), vb._keep_map(False)
    a, b = vb._engine(normalize=True), vb._engine()
    a.set_buckets(table)
    a.set_rare_fold(vb.BITS, words)
    for e in (a, b):
        e.fill_state(seed=6)
    init = a.get_state()
    for i, c in enumerate(vb._blocks(False)):
        h = vb._host_bucketed(c, table, words)
        hashed = fa.hash_ids(h.field, h.feat, vb.NF, field_start=vb.FS, n_fields=vb.F)
        assert (hashed < 0).any(), "some entries are erased"
        h = _variant(h, val=fa.normalize_rows(h.row_ptr, h.field, hashed, h.val, vb.NF, vb.F))
        _check_training(a, b, init, c, h, "hashed, block %d" % i, paths=("host", "async", "staged_zc"), weighted=(i == 1,))
        _check_prediction(a, b, c, h, "hashed, block %d" % i)
    a.close()
    b.close()


# ---- 4. the helpers, the counters, the caller's memory, the refusals ----------------------------------


@pytest.mark.parametrize("mt", ["FFM", "FM"])
def test_normalize_rows_device(mt):
    """In place and out of place, with values and without, on a flagged and on an unflagged engine; arrays at a
    16-byte boundary and 4 bytes off it."""
    engines = [fa.Engine(mt, NF, F if mt == "FFM" else 1, K, max_batch_rows=8, seed=1, normalize=flag, **STRESS_HP) for flag in (False, True)]
    dev = lambda x, off: torch.cat([torch.zeros(off, dtype=torch.from_numpy(x).dtype), torch.from_numpy(x)]).cuda()[off:]  # noqa: E731
    for e in engines:
        for name in ("ragged", "edge", "erased", "regular 63", "empty rows"):
            c = _blocks()[name]
            n, nnz = c.n_rows, int(c.row_ptr[-1])
            want = _norm(c, mt).val
            for off in (0, 1):
                rp, fld, ft = dev(c.row_ptr, 0), dev(c.field, off), dev(c.feat, off)
                val, out = dev(c.val, off), torch.full((nnz + off,), -7.0, dtype=torch.float32, device="cuda")[off:]
                torch.cuda.synchronize()
                e.normalize_rows_device(n, nnz, rp.data_ptr(), fld.data_ptr(), ft.data_ptr(), val.data_ptr(), out.data_ptr())
                e.sync()
                assert_bitwise(out.cpu().numpy(), want, "%s: out of place, offset %d" % (name, off))
                assert_bitwise(val.cpu().numpy(), c.val, name + ": the input stays")
                e.normalize_rows_device(n, nnz, rp.data_ptr(), fld.data_ptr(), ft.data_ptr(), val.data_ptr(), val.data_ptr())
                e.sync()
                assert_bitwise(val.cpu().numpy(), want, "%s: in place, offset %d" % (name, off))
                e.normalize_rows_device(n, nnz, rp.data_ptr(), fld.data_ptr(), ft.data_ptr(), None, out.data_ptr())
                e.sync()
                assert_bitwise(out.cpu().numpy(), _norm(c, mt, val=None).val, "%s: val_in = NULL, offset %d" % (name, off))
        e.close()


def test_norm_stats_and_reset():
    a, b, init = _pair()
    assert a.norm_stats() == (0, 0) and b.norm_stats() == (0, 0)
    edge, reg = _blocks()["edge"], _blocks()["regular 63"]
    a.train_batch(edge)
    assert a.norm_stats() == (edge.n_rows, EDGE_UNSCALED)
    a.train_batch_async(reg)
    a.train_batch_async(edge)
    a.train_flush()
    assert a.norm_stats() == (2 * edge.n_rows + 63, 2 * EDGE_UNSCALED)
    a.predict_batch(_blocks()["empty rows"])
    a.predict_batch_async(edge)
    a.train_flush()
    assert a.norm_stats(reset=True) == (3 * edge.n_rows + 63 + 3, 3 * EDGE_UNSCALED + 3)
    assert a.norm_stats() == (0, 0)
    a.predict_batch(reg)
    assert a.norm_stats() == (63, 0)
    assert b.norm_stats() == (0, 0)
    a.close()
    b.close()


def test_zero_copy_arrays_are_never_written():
    a, b, init = _pair()
    c = _blocks()["regular 63"]
    cb = _own_pages(c)
    a.pin_block(cb)
    try:
        a.train_batch_async_pinned(cb)
        a.train_flush()
        a.predict_batch_async(cb, zero_copy=True)
        a.train_flush()
        a.sync()
        assert_bitwise(cb.val, c.val, "the caller's val after the zero-copy calls")
        assert np.array_equal(cb.feat, c.feat) and np.array_equal(cb.field, c.field) and np.array_equal(cb.row_ptr, c.row_ptr)
    finally:
        a.sync()
        a.unpin_block(cb)
    pageable = _variant(c, val=c.val.copy())
    a.train_batch(pageable)
    a.predict_batch(pageable)
    assert_bitwise(pageable.val, c.val, "the caller's val after the synchronous calls")
    a.close()
    b.close()


def test_refusals():
    kw = dict(max_batch_rows=8, **STRESS_HP)
    with pytest.raises(fa.EngineError, match="a shard does not own whole rows") as ei:
        fa.Group([0, 0], "FFM", NF, F, K, normalize=True, **kw)
    assert ei.value.code == fa.engine.E_INVALID and "ffm_group_create" in str(ei.value)
    with pytest.raises(fa.EngineError, match="a shard does not own whole rows") as ei:
        fa.Engine("FFM", NF, F, K, n_shards=2, shard_rank=0, normalize=True, **kw)
    assert ei.value.code == fa.engine.E_INVALID and "n_shards" in str(ei.value)
    fa.Engine("FFM", NF, F, K, n_shards=2, shard_rank=0, **kw).close()  # (the flag is what is refused)
    assert fa.load_library().ffm_engine_abi_version() == 4
