"""FFM_FLAG_HASH_IDS on the device (include/ffm_engine.h "Hashed ids"): every entry point that takes host
rows hashes feat into its field's id range before any kernel reads it.

  1. ffm_engine_hash_ids_device is ffm_engine_hash_ids_host bit for bit (tests/test_hash_ids_host.py pins
     that one to the contract), every vector / tail length, explicit and implicit fields, in place or not;
  2. THE PIN: an engine created with the flag and fed RAW rows (ids from [0, 2^31), negatives, multi-valued
     rows, rows in which two raw ids collide) equals a twin without the flag fed the numpy-hashed rows --
     logits, loss sums and every w, n, z bit for bit -- through every path a host block can take;
  3. one case against the oracle on the hashed rows;
  4. a Group of two compact shards takes raw ids that are NOT in their fields' ranges and agrees with the
     flagged single engine; without the flag the same group reports FFM_E_INVALID;
  5. FFM_ENGINE_HASH_IDS=1 on an unflagged create gives the flagged engine's bits.
"""
import copy
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from hash_ref import np_hash_ids
from oracle.pyoracle import CpuModel, Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise, loss_close, rand_state

pytestmark = pytest.mark.gpu

f32 = np.float32
F, NF, K = 5, 203, 4
UNEVEN = np.array([0, 7, 8, 108, 150, 203], np.int32)  # widths 7, 1, 100, 42, 53
ROWS_MAX, ROW_NNZ = 300, 16
# (rows, nnz % 4) of the pin's blocks
SHAPES = ((1, 1), (7, 2), (64, 3), (300, 0))


# ---- 1. the kernel against the host function ----------------------------------------------------------


@pytest.mark.parametrize("n_fields", [5, 39])
def test_hash_ids_device_is_the_host_function(n_fields):
    nf = 20 * n_fields + 3
    fs = np.round(np.linspace(0, nf, n_fields + 1)).astype(np.int32)
    fs[1] = fs[0] + 1  # a field of width 1
    engines = [(None, fa.Engine("FFM", nf, n_fields, K, max_batch_rows=64, hash_ids=True)),
               (fs, fa.Engine("FFM", nf, n_fields, K, max_batch_rows=64, hash_ids=True, field_start=fs)),
               ("fm", fa.Engine("FM", nf, 1, K, max_batch_rows=64, hash_ids=True))]
    rng = np.random.default_rng(n_fields)
    for nnz in (0, 1, 2, 3, 4, 5, 7, 64, 65, 255, 1027):
        feat = rng.integers(0, 2 ** 31, nnz, dtype=np.int64).astype(np.int32)
        feat[::9] = -feat[::9] - 1
        field = rng.integers(-1, n_fields + 1, nnz).astype(np.int32)
        for which, e in engines:
            ffm = not isinstance(which, str)
            start = which if ffm and which is not None else None
            for fld in (field, None):
                want = fa.hash_ids(fld, feat, nf, field_start=start, model="ffm" if ffm else "fm", n_fields=n_fields)
                assert np.array_equal(want, np_hash_ids(fld, feat, nf, n_fields, start, ffm))
                d_feat = torch.from_numpy(feat.copy()).cuda() if nnz else torch.zeros(1, dtype=torch.int32, device="cuda")
                d_field = torch.from_numpy(fld).cuda() if fld is not None and nnz else None
                d_out = torch.full((max(nnz, 1) + 4,), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                e.hash_ids_device(nnz, d_field.data_ptr() if d_field is not None else None, d_feat.data_ptr(), d_out.data_ptr())
                e.sync()
                got = d_out.cpu().numpy()
                what = "nnz %d, %s, fields %s" % (nnz, "fm" if not ffm else "ranges" if start is not None else "one range",
                                                  "given" if fld is not None else "implicit")
                assert np.array_equal(got[:nnz], want), what
                assert (got[nnz:] == -7).all(), what + ": nothing is written behind the block"
                if nnz:
                    assert np.array_equal(d_feat.cpu().numpy(), feat), what + ": the input is not written"
                    e.hash_ids_device(nnz, d_field.data_ptr() if d_field is not None else None, d_feat.data_ptr(), d_feat.data_ptr())
                    e.sync()
                    assert np.array_equal(d_feat.cpu().numpy(), want), what + ": in place"
    for _, e in engines:
        e.close()
    plain = fa.Engine("FFM", nf, n_fields, K, max_batch_rows=64)
    with pytest.raises(fa.EngineError) as ei:
        plain.hash_ids_device(0, None, None, None)
    assert ei.value.code == fa.engine.E_INVALID
    plain.close()


# ---- 2. the pin ---------------------------------------------------------------------------------------


def _hashed(c, mt, fs):
    h = copy.copy(c)
    h.__dict__.pop("_ffm_csr_args", None)
    h.feat = np_hash_ids(c.field if mt == "FFM" else None, c.feat, NF, F if mt == "FFM" else 1, fs, ffm=mt == "FFM")
    return h


@functools.lru_cache(maxsize=None)
def _raw_blocks(mt, with_fs, regular):
    """Blocks of SHAPES' sizes with raw ids from [0, 2^31).  regular: exactly one entry per field and row, in
    field order (what a block without a field array must be); otherwise some rows are multi-valued or
    lack a field, and the last row of every block holds two raw ids that collide under one field."""
    fs = UNEVEN if with_fs and mt == "FFM" else None
    ffm = mt == "FFM"
    rng = np.random.default_rng(11 + 2 * with_fs + regular)
    pool = [rng.integers(0, 2 ** 31, 40, dtype=np.int64) for _ in range(F)]
    pool[0][0], pool[1][0], pool[2][0] = 0, 2 ** 31 - 1, NF  # the edges of the id space
    pool[3][0] = 5  # (inside [0, n_feats) and, with UNEVEN, outside field 3's range: what an unflagged shard refuses)
    pair = None  # (field, a, b): two raw ids of one field with one model id
    for f in range(F):
        ids = pool[f] if ffm else np.concatenate(pool)
        h = np_hash_ids(np.full(ids.size, f), ids, NF, F, fs, ffm)
        for i in range(ids.size):
            same = np.flatnonzero((h == h[i]) & (ids != ids[i]))
            if same.size and pair is None:
                pair = (f, int(ids[i]), int(ids[same[0]]))
    assert pair is not None, "the pools must hold two raw ids that collide"
    blocks = []
    for n_rows, residue in SHAPES:
        rows = []
        for r in range(n_rows):
            row = [(f, int(rng.choice(pool[f])), float(f32(0.5 + rng.random()))) for f in range(F)]
            u = rng.random()
            if not regular and u < 0.25:  # multi-valued: fields repeated, out of order
                for _ in range(int(rng.integers(1, 5))):
                    f = int(rng.integers(0, F))
                    row.append((f, int(rng.choice(pool[f])), float(f32(0.5 + rng.random()))))
            elif not regular and u > 0.9:
                del row[int(rng.integers(0, F))]
            if rng.random() < 0.1:  # an entry the reference erases
                j = int(rng.integers(0, len(row)))
                row[j] = (row[j][0], -1 - int(rng.integers(0, 1000)), row[j][2])
            rows.append(row)
        if not regular:
            rows[-1] += [(pair[0], pair[1], 1.25), (pair[0], pair[2], 0.75)]
            while sum(len(r) for r in rows) % 4 != residue:
                f = int(rng.integers(0, F))
                rows[-1].append((f, int(rng.choice(pool[f])), 1.0))
        c = Csr.from_rows(rows, rng.integers(0, 2, n_rows))
        if not ffm:
            c.field[:] = 0
        assert max(len(r) for r in rows) <= ROW_NNZ
        blocks.append(c)
    # the generated data holds every case the pin is about
    feat = np.concatenate([c.feat for c in blocks]).astype(np.int64)
    assert (feat < 0).any() and (feat >= NF).mean() > 0.8 and feat.max() == 2 ** 31 - 1 and (feat == 0).any()
    if regular:
        for c in blocks:
            assert (np.diff(c.row_ptr) == F).all()
            assert not ffm or (c.field.reshape(-1, F) == np.arange(F)).all()
    else:
        assert sorted(int(c.row_ptr[-1]) % 4 for c in blocks) == [0, 1, 2, 3]
        assert any((np.diff(c.row_ptr) > F).any() for c in blocks), "multi-valued rows"
        for c in blocks:  # the last row: two different raw ids, one model id, one field
            b = int(c.row_ptr[-2])
            h = _hashed(c, mt, fs).feat[b:]
            raw, fld = c.feat[b:], c.field[b:]
            assert any(h[i] == h[j] >= 0 and raw[i] != raw[j] and fld[i] == fld[j]
                       for i in range(h.size) for j in range(i)), "a row in which two raw ids collide"
    return tuple(blocks)


def _own_pages_block(c, with_field=True):
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


def _weights(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([0, 0.25, 1, 3.5], f32), n)
    return np.ascontiguousarray(w, f32)


def _train(e, path, c, weight):
    """One block through `path`; returns (logits or None, loss sum)."""
    if path == "host":
        return e.train_batch(c, weight=weight)
    if path == "async":
        e.train_batch_async(c, weight=weight)
        return None, e.train_flush()
    assert path in ("staged", "staged_zc")
    zc = path == "staged_zc"
    cb, wb = c, weight
    if zc:
        cb = _own_pages_block(c)
        e.pin_block(cb)
        if weight is not None:
            wb = fa.page_aligned(weight.size, f32)
            wb[:] = weight
            e._check(e.lib.ffm_engine_pin_host(wb.ctypes.data, wb.nbytes))
    out = torch.full((max(c.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    try:
        raw_before = cb.feat.copy()
        e.stage_batch(cb, zero_copy=zc, weight=wb)
        e.train_staged(out.data_ptr(), loss.data_ptr())
        e.sync()
        assert np.array_equal(cb.feat, raw_before), "the caller's buffers are never written"
    finally:
        if zc:
            e.sync()
            e.unpin_block(cb)
            if weight is not None:
                e.lib.ffm_engine_unpin_host(wb.ctypes.data)
    return out[:c.n_rows].cpu().numpy(), float(loss.cpu()[0])


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b))


def _engine_pair(mt, with_fs, **kw):
    fs = UNEVEN if with_fs and mt == "FFM" else None
    mk = lambda flag: fa.Engine(mt, NF, F if mt == "FFM" else 1, K, max_batch_rows=ROWS_MAX,  # noqa: E731
                                max_batch_nnz=ROWS_MAX * ROW_NNZ, max_row_nnz=ROW_NNZ, field_start=fs, seed=9,
                                hash_ids=flag, **STRESS_HP, **kw)
    return fs, mk(True), mk(False)


CONFIGS = [("FFM", False), ("FFM", True), ("FM", False), ("LR", False)]
CONFIG_IDS = ["FFM", "FFM-field_start", "FM", "LR"]


@pytest.mark.parametrize("mt,with_fs", CONFIGS, ids=CONFIG_IDS)
def test_flagged_engine_on_raw_rows_is_the_plain_engine_on_hashed_rows(mt, with_fs):
    fs, flagged, plain = _engine_pair(mt, with_fs)
    for e in (flagged, plain):
        e.fill_state(seed=6)
    init = flagged.get_state()
    assert_state_bitwise(plain.get_state(), init, "twin engines")
    blocks = _raw_blocks(mt, with_fs, False)
    trained = False
    for c in blocks:
        h = _hashed(c, mt, fs)
        assert (h.feat < NF).all() and not np.array_equal(h.feat, c.feat)
        for path in ("host", "async", "staged", "staged_zc"):
            for weight in (None, _weights(c.n_rows, c.n_rows)):
                what = "%s field_start=%s, %d rows, %s, %s" % (mt, with_fs, c.n_rows, path, "weighted" if weight is not None else "unweighted")
                flagged.set_state(init)
                plain.set_state(init)
                lg_a, ls_a = _train(flagged, path, c, weight)
                lg_b, ls_b = _train(plain, path, h, weight)
                if lg_a is not None:
                    assert_bitwise(lg_a, lg_b, what + ": logits")
                assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
                st = flagged.get_state()
                assert_state_bitwise(st, plain.get_state(), what)
                trained = trained or not np.array_equal(st["lin_n"], init["lin_n"])
    assert trained, "the blocks must train something"
    # prediction, on the state the last block left: synchronous, pipelined, pipelined with a score buffer
    scores = [e.score_buffer(ROWS_MAX) for e in (flagged, plain)]
    for c in blocks:
        h = _hashed(c, mt, fs)
        what = "%s field_start=%s, %d rows" % (mt, with_fs, c.n_rows)
        for prob in (False, True):
            out_a, ls_a = flagged.predict_batch(c, output_prob=prob)
            out_b, ls_b = plain.predict_batch(h, output_prob=prob)
            assert_bitwise(out_a, out_b, what + ": predict_batch")
            assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
        for zc in (False, True):
            ca, cb = (_own_pages_block(c), _own_pages_block(h)) if zc else (c, h)
            if zc:
                flagged.pin_block(ca)
                plain.pin_block(cb)
            flagged.predict_batch_async(ca, zero_copy=zc)
            plain.predict_batch_async(cb, zero_copy=zc)
            la, lb = flagged.train_flush(), plain.train_flush()
            assert _same_double(la, lb) and abs(la - ls_a) <= 1e-12 * abs(ls_a), (what, zc, la, lb, ls_a)
            for s in scores:
                s[:] = np.nan
            flagged.predict_batch_async(ca, zero_copy=zc, scores=scores[0], output_prob=True)
            plain.predict_batch_async(cb, zero_copy=zc, scores=scores[1], output_prob=True)
            la, lb = flagged.train_flush(), plain.train_flush()
            assert _same_double(la, lb), (what, zc, la, lb)
            assert_bitwise(scores[0][:c.n_rows], scores[1][:c.n_rows], what + ": scores")
            assert_bitwise(scores[0][:c.n_rows], out_a, what + ": scores are predict_batch's")
            if zc:
                assert np.array_equal(ca.feat, c.feat), "the caller's buffers are never written"
                flagged.unpin_block(ca)
                plain.unpin_block(cb)
    for e, s in zip((flagged, plain), scores):
        e.free_score_buffer(s)
        e.close()


@pytest.mark.parametrize("mt,with_fs", CONFIGS[:2], ids=CONFIG_IDS[:2])
def test_blocks_without_a_field_array(mt, with_fs):
    """field == NULL (one entry per field in field order): the upload kernel writes the fields AND hashes
    by them."""
    fs, flagged, plain = _engine_pair(mt, with_fs)
    for e in (flagged, plain):
        e.fill_state(seed=6)
    init = flagged.get_state()
    for c in _raw_blocks(mt, with_fs, True):
        h = _hashed(c, mt, fs)
        bare = copy.copy(c)
        bare.__dict__.pop("_ffm_csr_args", None)
        bare.field = None
        for path in ("async", "staged", "staged_zc"):
            what = "%d rows, %s" % (c.n_rows, path)
            flagged.set_state(init)
            plain.set_state(init)
            lg_a, ls_a = _train(flagged, path, bare, None)
            lg_b, ls_b = _train(plain, path, h, None)
            if lg_a is not None:
                assert_bitwise(lg_a, lg_b, what + ": logits")
            assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
            assert_state_bitwise(flagged.get_state(), plain.get_state(), what)
        flagged.predict_batch_async(bare)
        plain.predict_batch_async(h)
        la, lb = flagged.train_flush(), plain.train_flush()
        assert _same_double(la, lb), (c.n_rows, la, lb)
    flagged.close()
    plain.close()


# ---- 3. against the oracle ------------------------------------------------------------------------------


def test_flagged_engine_is_the_oracle_on_the_hashed_rows():
    c = _raw_blocks("FFM", True, False)[2]
    h = _hashed(c, "FFM", UNEVEN)
    o = CpuModel("oracle", "FFM", NF, F, K, **STRESS_HP)
    st = rand_state(np.random.default_rng(21), o, n_hi=1e-4, w_sd=0.5)  # (as test_block_semantics._fold_case)
    o.set_state(st)
    want_lg, want_loss = o.train_batch(h)
    want = o.get_state()
    e = fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * ROW_NNZ, max_row_nnz=ROW_NNZ,
                  field_start=UNEVEN, skip_init=True, hash_ids=True, **STRESS_HP)
    e.set_state(st)
    lg, ls = e.train_batch(c)
    assert_bitwise(lg, want_lg, "logits against the oracle")
    assert loss_close(ls, want_loss), (ls, want_loss)
    assert_state_bitwise(e.get_state(), want, "state against the oracle")
    want_p, want_pl = o.predict_batch(h)
    out, pl = e.predict_batch(c)
    assert_bitwise(out, want_p, "predict against the oracle")
    assert loss_close(pl, want_pl), (pl, want_pl)
    e.close()


# ---- 4. a group of compact shards takes any ids -------------------------------------------------------


def test_group_of_compact_shards_takes_raw_ids():
    fs = UNEVEN
    blocks = _raw_blocks("FFM", True, False)
    raw = np.concatenate([c.feat for c in blocks])
    fld = np.concatenate([c.field for c in blocks])
    ok = raw >= 0
    assert ((raw[ok] < fs[fld[ok]]) | (raw[ok] >= fs[fld[ok] + 1])).mean() > 0.9, "raw ids outside their fields' ranges"
    kw = dict(max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * ROW_NNZ, max_row_nnz=ROW_NNZ, field_start=fs, seed=4, **STRESS_HP)
    ref = fa.Engine("FFM", NF, F, K, hash_ids=True, **kw)
    ref.fill_state(seed=6)
    init = ref.get_state()
    logits, losses = zip(*[ref.train_batch(c) for c in blocks])
    pred, pred_loss = ref.predict_batch(blocks[-1])
    for pipelined in (False, True):
        g = fa.Group([0, 0], "FFM", NF, F, K, hash_ids=True, **kw)
        for e in g.engines:
            e.set_state(init)
        if pipelined:
            for c in blocks:
                g.train_batch_async(c)
            total = g.train_flush()
            assert abs(total - sum(losses)) <= 2e-4 * abs(sum(losses))
        else:
            for i, c in enumerate(blocks):
                lg, ls = g.train_batch(c)
                # (the tolerances of tests/test_gpu_group.py for the same comparison)
                np.testing.assert_allclose(lg, logits[i], rtol=2e-4, atol=2e-5, err_msg="block %d" % i)
                assert abs(ls - losses[i]) <= 2e-4 * abs(losses[i])
        out, ls = g.predict_batch(blocks[-1])
        np.testing.assert_allclose(out, pred, rtol=2e-4, atol=2e-5)
        assert abs(ls - pred_loss) <= 2e-4 * abs(pred_loss)
        g.close()
    ref.close()
    # the same group without the flag: an id outside its field's range voids the block
    g = fa.Group([0, 0], "FFM", NF, F, K, **kw)
    with pytest.raises(fa.EngineError) as ei:
        g.train_batch(blocks[-1])
    assert ei.value.code == fa.engine.E_INVALID and "field" in str(ei.value)
    g.close()


# ---- 5. the switch ----------------------------------------------------------------------------------------


def test_the_environment_switch_turns_the_flag_on(monkeypatch):
    c = _raw_blocks("FFM", True, False)[2]
    kw = dict(max_batch_rows=ROWS_MAX, max_batch_nnz=ROWS_MAX * ROW_NNZ, max_row_nnz=ROW_NNZ, field_start=UNEVEN, seed=4, **STRESS_HP)
    flagged = fa.Engine("FFM", NF, F, K, hash_ids=True, **kw)
    monkeypatch.setenv("FFM_ENGINE_HASH_IDS", "1")
    switched = fa.Engine("FFM", NF, F, K, **kw)
    monkeypatch.setenv("FFM_ENGINE_HASH_IDS", "0")
    off = fa.Engine("FFM", NF, F, K, **kw)
    monkeypatch.delenv("FFM_ENGINE_HASH_IDS")
    got = []
    for e in (flagged, switched, off):
        e.fill_state(seed=6)
        lg, ls = e.train_batch(c)
        e.train_batch_async(c)
        got.append((lg, ls, e.train_flush(), e.get_state()))
        e.close()
    assert_bitwise(got[1][0], got[0][0], "logits under FFM_ENGINE_HASH_IDS=1")
    assert _same_double(got[1][1], got[0][1]) and _same_double(got[1][2], got[0][2])
    assert_state_bitwise(got[1][3], got[0][3], "state under FFM_ENGINE_HASH_IDS=1")
    assert not np.array_equal(got[2][0], got[0][0]), "FFM_ENGINE_HASH_IDS=0 leaves the flag off: raw ids >= n_feats are erased"
