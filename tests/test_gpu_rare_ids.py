"""Rare ids on the device (include/ffm_engine.h "Rare ids"), against the numpy restatement (tests/rare_ref.py).

  1. the counter: read() is min(bincount, cap) word for word and n_valid / n_bad are exact -- vector and tail
     lengths, with a field array and without, LR, aligned and offset by one word, slots that collide, a hot id,
     entries that do not count, halves, pageable / page-locked / device arrays;
  2. the keep-map: words, n_kept_slots and n_folded_entries;
  3. THE PIN: an engine with a map fed RAW blocks equals an engine without a map fed the same blocks with the
     rare ids replaced by INT32_MAX in numpy -- logits, loss sums and every w, n, z bit for bit -- through every
     path a host block can take, on a serving engine, for the candidates, and for ffm_engine_hash_ids_device;
  4. the filtered sketch's registers are sketch_ref's on the folded entries.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
import rare_ref
import sketch_ref
from hash_ref import np_hash_ids
from oracle.pyoracle import Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise

pytestmark = pytest.mark.gpu

f32 = np.float32
INT32_MAX = 2 ** 31 - 1
NNZ = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)
CAPS = (1, 2, 7)


# ---- 1. the counter ---------------------------------------------------------------------------------------


def entries(nnz, n_fields, seed):
    """Entries that repeat (a pool of 40 ids beside random ones), with everything that must not count mixed in."""
    rng = np.random.default_rng(seed)
    F = max(n_fields, 1)
    field = rng.integers(0, F, size=nnz, dtype=np.int64)
    feat = rng.integers(0, 2 ** 31, size=nnz, dtype=np.int64)
    kind = rng.integers(0, 16, size=nnz)
    field[kind == 0] = -1
    field[kind == 1] = F
    feat[kind == 2] = -1
    feat[kind == 3] = -2 ** 31
    feat[kind == 4] = 0
    feat[kind == 5] = INT32_MAX
    feat[kind >= 9] = rng.integers(0, 40, size=int((kind >= 9).sum()))
    return field.astype(np.int32), feat.astype(np.int32)


def pinned_copy(a):
    if a is None:
        return None
    p = fa.page_aligned(max(1, a.size), np.int32)
    p[:a.size] = a
    assert fa.load_library().ffm_engine_pin_host(p.ctypes.data, max(1, p.size) * 4) == 0
    return p


def unpin(p):
    if p is not None:
        assert fa.load_library().ffm_engine_unpin_host(p.ctypes.data) == 0


def feed(ct, field, feat, how):
    n = feat.size
    if how == "pageable":
        ct.add(field, feat)
    elif how in ("zero_copy", "zero_copy_offset"):  # offset: the arrays start one word into their pages -- no 16-byte loads
        o = 1 if how == "zero_copy_offset" else 0
        pad = lambda a: None if a is None else pinned_copy(np.concatenate([np.zeros(o, np.int32), a]).astype(np.int32))  # noqa: E731
        pf, pi = pad(field), pad(feat)
        try:
            ct.add(None if pf is None else pf[o:n + o], pi[o:n + o], zero_copy=True)
        finally:
            unpin(pf)
            unpin(pi)
    elif how in ("device", "device_offset"):
        o = 1 if how == "device_offset" else 0
        dev = lambda a: None if a is None else torch.from_numpy(np.concatenate([np.zeros(o, np.int32), a]).astype(np.int32)).cuda()  # noqa: E731
        df, di = dev(field), dev(feat)
        torch.cuda.synchronize()
        ct.add_device(n, None if df is None else df.data_ptr() + 4 * o, di.data_ptr() + 4 * o if n else None)
        ct.read()  # (waits for the counter's stream before the tensors go)
    else:
        raise ValueError(how)


def gpu_counts(n_fields, bits, cap, field, feat, how="pageable"):
    ct = fa.IdCounter(n_fields, bits, cap)
    try:
        feed(ct, field, feat, how)
        return ct.read()
    finally:
        ct.close()


def assert_same(got, want, what):
    cnt, nv, nb = got
    wcnt, wnv, wnb = want
    assert (nv, nb) == (wnv, wnb), (what, nv, nb, wnv, wnb)
    assert cnt.dtype == np.uint32 and cnt.shape == wcnt.shape
    bad = np.flatnonzero(cnt != wcnt)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), cnt[bad[:5]].tolist(), wcnt[bad[:5]].tolist())


HOWS = ("pageable", "zero_copy", "zero_copy_offset", "device", "device_offset")


@pytest.mark.parametrize("n_fields,with_field", [(8, True), (8, False), (0, False), (0, True)],
                         ids=["field array", "no field array", "LR", "LR given fields"])
def test_counts_and_counters_are_exact(n_fields, with_field):
    bits = 8
    for nnz in NNZ:
        field, feat = entries(nnz, n_fields, seed=100 * n_fields + nnz)
        fld = field if with_field else None
        for cap in CAPS:
            want = rare_ref.np_counts(fld if n_fields else None, feat, n_fields, bits, cap)
            if nnz == 4099:
                assert want[2] > 0 and want[0].max() == cap, "the cap must cut something"
            for how in HOWS if cap == 2 else ("pageable", "device"):
                assert_same(gpu_counts(n_fields, bits, cap, fld, feat, how), want, (n_fields, nnz, cap, how))


def test_distinct_ids_share_slots():
    """4099 distinct ids of one field in 256 slots: every slot holds about sixteen of them."""
    rng = np.random.default_rng(1)
    feat = rng.choice(2 ** 24, size=4099, replace=False).astype(np.int32)
    field = np.zeros(4099, np.int32)
    for cap in CAPS + (65535,):
        want = rare_ref.np_counts(field, feat, 1, 8, cap)
        assert want[1] == 4099 and (cap < 65535 or (want[0].sum() == 4099 and want[0].min() >= 2))
        for how in ("pageable", "zero_copy", "device"):
            assert_same(gpu_counts(1, 8, cap, field, feat, how), want, (cap, how))
    # more slots: the same ids spread out
    want = rare_ref.np_counts(field, feat, 1, 20, 7)
    assert want[0].max() <= 2
    assert_same(gpu_counts(1, 20, 7, field, feat), want, "2^20 slots")


@pytest.mark.parametrize("cap", CAPS + (65535,))
def test_one_id_ten_thousand_times_in_one_call(cap):
    rng = np.random.default_rng(2)
    feat = np.concatenate([np.full(10000, 123456789, np.int64), rng.integers(0, 2 ** 31, size=300, dtype=np.int64)])
    field = np.concatenate([np.full(10000, 2, np.int64), rng.integers(0, 4, size=300)])
    order = rng.permutation(feat.size)
    field, feat = field[order].astype(np.int32), feat[order].astype(np.int32)
    want = rare_ref.np_counts(field, feat, 4, 12, cap)
    hot = int(rare_ref.np_slot([2], [123456789], 12)[0])
    assert min(cap, 10000) <= want[0][hot] <= min(cap, 10300) and want[0].max() == want[0][hot]
    for how in ("pageable", "zero_copy", "device"):
        assert_same(gpu_counts(4, 12, cap, field, feat, how), want, (cap, how))


def test_halves_in_two_calls_and_any_way_of_feeding():
    F, nnz, bits = 8, 4099, 8
    field, feat = entries(nnz, F, seed=9)
    for cap in CAPS:
        want = rare_ref.np_counts(field, feat, F, bits, cap)
        assert_same(gpu_counts(F, bits, cap, field, feat), want, "one call")
        ct = fa.IdCounter(F, bits, cap)
        ct.add(field[:nnz // 2].copy(), feat[:nnz // 2].copy())
        first = ct.read()
        assert_same(first, rare_ref.np_counts(field[:nnz // 2], feat[:nnz // 2], F, bits, cap), "the first half")
        ct.add(field[nnz // 2:].copy(), feat[nnz // 2:].copy())
        assert_same(ct.read(), want, "two halves")
        ct.close()
        cuts = [0, 5, 5, 260, 1027, 3000, nnz]
        ct = fa.IdCounter(F, bits, cap)
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            feed(ct, field[lo:hi].copy(), feat[lo:hi].copy(), ("pageable", "zero_copy", "device")[i % 3])
        assert_same(ct.read(), want, "six ragged calls, the ways mixed")
        ct.close()
    # rows without a field array in two calls: each call's entry p is field p mod F
    half = 8 * 100
    both = np.concatenate([np.arange(half) % F, np.arange(nnz - half) % F]).astype(np.int32)
    ct = fa.IdCounter(F, bits, 7)
    ct.add(None, feat[:half].copy())
    ct.add(None, feat[half:].copy())
    assert_same(ct.read(), rare_ref.np_counts(both, feat, F, bits, 7), "no field array, two calls")
    ct.close()


def test_pageable_call_longer_than_a_staging_chunk():
    """A pageable call is staged in chunks of 2^22 entries; without a field array the second chunk's fields go on
    where the first one's stopped (2^22 mod 7 = 2), with one both chunks' entries land where they belong."""
    nnz, F, bits, cap = (1 << 22) + 7, 7, 22, 7
    rng = np.random.default_rng(3)
    feat = rng.integers(0, 1 << 20, size=nnz, dtype=np.int64).astype(np.int32)
    feat[rng.integers(0, nnz, size=1000)] = -5
    assert_same(gpu_counts(F, bits, cap, None, feat), rare_ref.np_counts(None, feat, F, bits, cap), "no field array")
    field = ((np.arange(nnz, dtype=np.int64) * 5 + 3) % (F + 1)).astype(np.int32)  # (field 7 of 7: does not count)
    assert_same(gpu_counts(F, bits, cap, field, feat), rare_ref.np_counts(field, feat, F, bits, cap), "with a field array")


def test_pageable_call_of_three_staging_chunks():
    """The third chunk goes into the first chunk's image, once the first launch has read it; its fields go on where
    the second chunk's stopped (2^23 mod 7 = 4)."""
    nnz, F, bits, cap = 2 * (1 << 22) + 5, 7, 22, 15
    rng = np.random.default_rng(4)
    feat = rng.integers(0, 1 << 20, size=nnz, dtype=np.int64).astype(np.int32)
    feat[rng.integers(0, nnz, size=1000)] = -5
    want = rare_ref.np_counts(None, feat, F, bits, cap)
    assert np.unique(want[0]).size > 4 and want[2] > 0  # (the cap leaves the counts apart: a misplaced entry shows)
    assert_same(gpu_counts(F, bits, cap, None, feat), want, "three chunks")


def test_counter_arguments():
    lib = fa.load_library()
    for bad in ((4, 7, 3), (4, 31, 3), (4, 8, 0), (4, 8, 65536), (-1, 8, 3)):
        with pytest.raises(fa.EngineError) as ei:
            fa.IdCounter(*bad)
        assert ei.value.code == fa.engine.E_INVALID, bad
    ct = fa.IdCounter(4, 8, 3)
    cnt, nv, nb = ct.read()
    assert not cnt.any() and cnt.shape == (256,) and (nv, nb) == (0, 0)
    feat = np.arange(8, dtype=np.int32)
    assert lib.ffm_engine_idcount_add(ct.h, -1, None, feat.ctypes.data, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_idcount_add(ct.h, 8, None, None, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_idcount_add_device(ct.h, -1, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_idcount_add_device(ct.h, 8, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_idcount_add(ct.h, 0, None, None, 0) == 0 and lib.ffm_engine_idcount_add_device(ct.h, 0, None, None) == 0
    assert lib.ffm_engine_idcount_add(ct.h, 8, None, feat.ctypes.data, 1) == fa.engine.E_INVALID
    assert b"page-locked" in lib.ffm_engine_last_error()
    nv, nb = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.ffm_engine_idcount_read(ct.h, None, ctypes.byref(nv), ctypes.byref(nb)) == 0  # (counts may be NULL)
    assert (nv.value, nb.value) == (0, 0)
    ct.close()
    ct.close()  # (twice is fine)


# ---- 2. the keep-map --------------------------------------------------------------------------------------


@pytest.mark.parametrize("cap", CAPS + (300,))
def test_keep_map_against_numpy(cap):
    F, bits = 8, 8
    field, feat = entries(4099, F, seed=21)
    ct = fa.IdCounter(F, bits, cap)
    ct.add(field, feat)
    counts = ct.read()[0]
    assert_same((counts, 0, 0), (rare_ref.np_counts(field, feat, F, bits, cap)[0], 0, 0), "counts")
    true_counts = rare_ref.np_counts(field, feat, F, bits, 1 << 30)[0]
    for T in sorted({1, 2, cap}):
        if T > cap:
            continue
        words, kept, folded = ct.keep(T)
        wwords, wkept, wfolded = rare_ref.np_keep(counts, T)
        assert words.dtype == np.uint64 and np.array_equal(words, wwords), (cap, T)
        assert (kept, folded) == (wkept, wfolded), (cap, T, kept, folded, wkept, wfolded)
        # what the figures mean: the slots seen at least T times, and the counted entries in the other slots
        assert kept == int((true_counts >= T).sum()) and folded == int(true_counts[true_counts < T].sum())
        assert ct.keep(T)[1:] == (kept, folded), "a second call gives the same sums"
    assert ct.keep(1)[2] == 0 and ct.keep(1)[1] == int((true_counts > 0).sum())
    for T in (0, -1, cap + 1):
        with pytest.raises(fa.EngineError) as ei:
            ct.keep(T)
        assert ei.value.code == fa.engine.E_INVALID, T
    ct.close()
    # 2^14 slots: more words than one workgroup's waves
    ct = fa.IdCounter(F, 14, cap)
    ct.add(field, feat)
    got = ct.keep(min(2, cap))
    want = rare_ref.np_keep(ct.read()[0], min(2, cap))
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    ct.close()


# ---- 3. the pin -------------------------------------------------------------------------------------------

F, K, NF, BITS = 8, 4, 4096, 8
FS = (np.arange(F + 1) * (NF // F)).astype(np.int32)
ROWS, ROW_NNZ = 257, 16


@functools.lru_cache(maxsize=None)
def _blocks(mt, regular):
    """Three blocks of 257 rows, raw ids from [0, 2^31) drawn from per-field pools with a heavy head, a few erased
    entries.  regular: exactly one entry per field and row in field order; otherwise some rows are multi-valued
    and the entry count is no multiple of 4."""
    ffm = mt == "FFM"
    rng = np.random.default_rng(5 + regular)
    pool = [rng.integers(0, 2 ** 31, 400, dtype=np.int64) for _ in range(F)]
    pool[0][0], pool[1][0] = 0, INT32_MAX
    p = 1.0 / (1.0 + np.arange(400)) ** 1.1
    p /= p.sum()
    blocks = []
    for b in range(3):
        rows = []
        for r in range(ROWS):
            row = [(f, int(rng.choice(pool[f], p=p)), float(f32(0.5 + rng.random()))) for f in range(F)]
            if not regular and rng.random() < 0.25:
                for _ in range(int(rng.integers(1, 5))):
                    f = int(rng.integers(0, F))
                    row.append((f, int(rng.choice(pool[f], p=p)), float(f32(0.5 + rng.random()))))
            if rng.random() < 0.1:
                j = int(rng.integers(0, len(row)))
                row[j] = (row[j][0], -1 - int(rng.integers(0, 1000)), row[j][2])
            rows.append(row)
        while not regular and sum(len(r) for r in rows) % 4 != b + 1:
            f = int(rng.integers(0, F))
            rows[-1].append((f, int(rng.choice(pool[f], p=p)), 1.0))
        c = Csr.from_rows(rows, rng.integers(0, 2, ROWS))
        if not ffm:
            c.field[:] = 0
        assert max(len(r) for r in rows) <= ROW_NNZ
        blocks.append(c)
    if not regular:
        assert sorted(int(c.row_ptr[-1]) % 4 for c in blocks) == [1, 2, 3]
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def _map(mt, regular):
    """(T, words) counted on the device from the blocks, T chosen so that about half the entries fold."""
    blocks = _blocks(mt, regular)
    n_fields = F if mt == "FFM" else 0
    field = np.concatenate([c.field for c in blocks])
    feat = np.concatenate([c.feat for c in blocks])
    true_counts = rare_ref.np_counts(field, feat, n_fields, BITS, 65535)[0].astype(np.int64)
    total = int(true_counts.sum())
    T = min(range(2, 400), key=lambda t: abs(int(true_counts[true_counts < t].sum()) - total // 2))
    ct = fa.IdCounter(n_fields, BITS, T)
    for c in blocks:
        ct.add(c.field if n_fields else None, c.feat)
    words, kept, folded = ct.keep(T)
    ct.close()
    assert np.array_equal(words, rare_ref.np_keep(np.minimum(true_counts, T), T)[0])
    assert 0.3 * total < folded < 0.7 * total and 0 < kept < 256, (T, kept, folded, total)
    return T, words


def _folded(c, mt, words):
    h = copy.copy(c)
    h.__dict__.pop("_ffm_csr_args", None)
    h.feat = rare_ref.np_fold(c.field if mt == "FFM" else None, c.feat, F if mt == "FFM" else 0, BITS, words)
    assert (h.feat != c.feat).mean() > 0.25 and (h.feat == c.feat).mean() > 0.25
    return h


def _variant(c, **kw):
    h = copy.copy(c)
    h.__dict__.pop("_ffm_csr_args", None)
    for key, v in kw.items():
        setattr(h, key, v)
    return h


def _own_pages_block(c):
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
    return np.ascontiguousarray(np.random.default_rng(seed).choice(np.array([0, 0.25, 1, 3.5], f32), n), f32)


def _train(e, path, c, weight):
    """One block through `path`; returns (logits or None, loss sum)."""
    if path == "host":
        return e.train_batch(c, weight=weight)
    if path == "async":
        e.train_batch_async(c, weight=weight)
        return None, e.train_flush()
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


def _engine(mt, **kw):
    return fa.Engine(mt, NF, F if mt == "FFM" else 1, K, max_batch_rows=ROWS, max_batch_nnz=ROWS * ROW_NNZ, max_row_nnz=ROW_NNZ,
                     field_start=FS if mt == "FFM" else None, seed=9, hash_ids=True, **dict(STRESS_HP, **kw))


def _pair(mt, regular=False):
    """(a with the map, b without, the map's words, the state both start from)."""
    _, words = _map(mt, regular)
    a, b = _engine(mt), _engine(mt)
    a.set_rare_fold(BITS, words)
    for e in (a, b):
        e.fill_state(seed=6)
    init = a.get_state()
    assert_state_bitwise(b.get_state(), init, "twin engines")
    return a, b, words, init


@pytest.mark.parametrize("mt", ["FFM", "LR"])
def test_engine_with_a_map_on_raw_blocks_is_the_plain_engine_on_folded_blocks(mt):
    a, b, words, init = _pair(mt)
    blocks = _blocks(mt, False)
    trained = False
    for c in blocks:
        h = _folded(c, mt, words)
        for path in ("host", "async", "staged", "staged_zc"):
            for weight in (None, _weights(c.n_rows, 3)):
                for bare in (False, True):  # val=None: the values are written on the device
                    if bare and weight is not None:
                        continue
                    ca, cb = (_variant(c, val=None), _variant(h, val=np.ones_like(h.val))) if bare else (c, h)
                    what = "%s, %s, %s%s" % (mt, path, "weighted" if weight is not None else "unweighted", ", val=None" if bare else "")
                    a.set_state(init)
                    b.set_state(init)
                    lg_a, ls_a = _train(a, path, ca, weight)
                    lg_b, ls_b = _train(b, path, cb, weight)
                    if lg_a is not None:
                        assert_bitwise(lg_a, lg_b, what + ": logits")
                    assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
                    st = a.get_state()
                    assert_state_bitwise(st, b.get_state(), what)
                    trained = trained or not np.array_equal(st["lin_n"], init["lin_n"])
    assert trained, "the blocks must train something"
    # the fold changes what is trained: the plain engine on the RAW block ends elsewhere
    a.set_state(init)
    b.set_state(init)
    a.train_batch(blocks[0])
    b.train_batch(blocks[0])
    assert not np.array_equal(a.get_state()["lin_n"], b.get_state()["lin_n"])
    # prediction on the state the last folded block left: synchronous and pipelined, with scores
    a.set_state(init)
    b.set_state(init)
    scores = [e.score_buffer(ROWS) for e in (a, b)]
    for c in blocks:
        h = _folded(c, mt, words)
        for prob in (False, True):
            out_a, ls_a = a.predict_batch(c, output_prob=prob)
            out_b, ls_b = b.predict_batch(h, output_prob=prob)
            assert_bitwise(out_a, out_b, mt + ": predict_batch")
            assert _same_double(ls_a, ls_b), (ls_a, ls_b)
        for zc in (False, True):
            ca, cb = (_own_pages_block(c), _own_pages_block(h)) if zc else (c, h)
            if zc:
                a.pin_block(ca)
                b.pin_block(cb)
            for s in scores:
                s[:] = np.nan
            a.predict_batch_async(ca, zero_copy=zc, scores=scores[0], output_prob=True)
            b.predict_batch_async(cb, zero_copy=zc, scores=scores[1], output_prob=True)
            la, lb = a.train_flush(), b.train_flush()
            assert _same_double(la, lb), (zc, la, lb)
            assert_bitwise(scores[0][:c.n_rows], scores[1][:c.n_rows], mt + ": pipelined scores")
            assert_bitwise(scores[0][:c.n_rows], out_a, mt + ": pipelined scores are predict_batch's")
            if zc:
                a.unpin_block(ca)
                b.unpin_block(cb)
    # turning the fold off restores the plain hashed results
    a.set_rare_fold(None)
    for c in blocks[:1]:
        a.set_state(init)
        b.set_state(init)
        for path in ("host", "staged"):
            lg_a, ls_a = _train(a, path, c, None)
            lg_b, ls_b = _train(b, path, c, None)
            assert_bitwise(lg_a, lg_b, "fold off: logits")
            assert _same_double(ls_a, ls_b)
        assert_state_bitwise(a.get_state(), b.get_state(), "fold off")
    for e, s in zip((a, b), scores):
        e.free_score_buffer(s)
        e.close()


def test_blocks_without_a_field_array():
    """field == NULL (one entry per field in field order): the upload kernel folds and hashes by the fields it writes."""
    a, b, words, init = _pair("FFM", regular=True)
    for c in _blocks("FFM", True):
        assert int(c.row_ptr[-1]) == ROWS * F
        h = _folded(c, "FFM", words)
        assert np.array_equal(h.feat, rare_ref.np_fold(None, c.feat, F, BITS, words))
        for bare_val in (False, True):
            ca = _variant(c, field=None, val=None) if bare_val else _variant(c, field=None)
            cb = _variant(h, val=np.ones_like(h.val)) if bare_val else h
            for path in ("async", "staged", "staged_zc"):
                what = "no field array, %s%s" % (path, ", val=None" if bare_val else "")
                a.set_state(init)
                b.set_state(init)
                lg_a, ls_a = _train(a, path, ca, None)
                lg_b, ls_b = _train(b, path, cb, None)
                if lg_a is not None:
                    assert_bitwise(lg_a, lg_b, what + ": logits")
                assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
                assert_state_bitwise(a.get_state(), b.get_state(), what)
        a.predict_batch_async(_variant(c, field=None))
        b.predict_batch_async(h)
        la, lb = a.train_flush(), b.train_flush()
        assert _same_double(la, lb), (la, lb)
    a.close()
    b.close()


def test_serving_engine_and_candidates():
    _, words = _map("FFM", False)
    t = _engine("FFM")
    t.fill_state(seed=6)
    w = t.get_weights()
    t.close()
    mk = lambda: fa.Engine("FFM", NF, F, K, skip_init=True, serve="f32", max_batch_rows=4 * ROWS, max_batch_nnz=4 * ROWS * ROW_NNZ,  # noqa: E731
                           field_start=FS, hash_ids=True, **STRESS_HP)
    a, b = mk(), mk()
    for e in (a, b):
        e.set_weights(bias=w["bias"], lin_w=w["lin_w"], vec_w=w["vec_w"])
    a.set_rare_fold(BITS, words)
    for c in _blocks("FFM", False):
        h = _folded(c, "FFM", words)
        for prob in (False, True):
            assert_bitwise(a.predict_batch(c, output_prob=prob)[0], b.predict_batch(h, output_prob=prob)[0], "serving predict_batch")
    # candidates: the context holds fields 0 .. 3, every candidate fields 4 .. 7
    c = _blocks("FFM", True)[0]
    n_req, per = 5, 7
    rows = lambda blk, lo, hi, cols: Csr.from_rows(  # noqa: E731
        [[(int(blk.field[r * F + j]), int(blk.feat[r * F + j]), float(blk.val[r * F + j])) for j in cols] for r in range(lo, hi)],
        np.zeros(hi - lo, np.int32))
    rq = (np.arange(n_req + 1) * per).astype(np.int32)
    ctx, cand = rows(c, 0, n_req, range(0, 4)), rows(c, n_req, n_req + n_req * per, range(4, 8))
    fctx = _variant(ctx, feat=rare_ref.np_fold(ctx.field, ctx.feat, F, BITS, words))
    fcand = _variant(cand, feat=rare_ref.np_fold(cand.field, cand.feat, F, BITS, words))
    assert (fctx.feat != ctx.feat).any() and (fcand.feat != cand.feat).any()
    for prob in (False, True):
        got = a.score_candidates(ctx, rq, cand, output_prob=prob)
        assert_bitwise(got, b.score_candidates(fctx, rq, fcand, output_prob=prob), "score_candidates")
        assert_bitwise(got, a.predict_batch(fa.spell_out_candidates(ctx, rq, cand), output_prob=prob)[0], "candidates vs predict_batch")
    assert not np.array_equal(a.score_candidates(ctx, rq, cand), b.score_candidates(ctx, rq, cand)), "the fold changes the scores"
    a.set_rare_fold(None)
    assert_bitwise(a.score_candidates(ctx, rq, cand), b.score_candidates(ctx, rq, cand), "fold off")
    a.close()
    b.close()


@pytest.mark.parametrize("mt", ["FFM", "FM"])
def test_hash_ids_device_folds_like_the_host_twin(mt):
    ffm = mt == "FFM"
    n_fields = F if ffm else 0
    e = _engine(mt)
    rng = np.random.default_rng(8)
    for nnz in (0, 1, 3, 4, 5, 64, 65, 255, 1027):
        field, feat = entries(nnz, F, seed=nnz)
        if nnz:
            feat[rng.integers(0, nnz, size=max(1, nnz // 4))] = 5  # a frequent id
        for fld in (field, None):
            imp = (np.arange(nnz) % F).astype(np.int32) if ffm else None
            cnt_field = None if not ffm else fld if fld is not None else imp
            counts = rare_ref.np_counts(cnt_field, feat, n_fields, BITS, 3)[0]
            words = rare_ref.np_keep(counts, 3)[0]
            e.set_rare_fold(BITS, words)
            folded = fa.fold_rare(fld, feat, n_fields, BITS, words)
            assert np.array_equal(folded, rare_ref.np_fold(fld if ffm else None, feat, n_fields, BITS, words))
            want = fa.hash_ids(fld, folded, NF, field_start=FS if ffm else None, model=mt.lower(), n_fields=F)
            assert np.array_equal(want, np_hash_ids(fld, folded, NF, F, FS if ffm else None, ffm))
            d_feat = torch.from_numpy(feat.copy()).cuda() if nnz else torch.zeros(1, dtype=torch.int32, device="cuda")
            d_field = torch.from_numpy(fld).cuda() if fld is not None and nnz else None
            d_out = torch.full((max(nnz, 1) + 4,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            e.hash_ids_device(nnz, d_field.data_ptr() if d_field is not None else None, d_feat.data_ptr(), d_out.data_ptr())
            e.sync()
            got = d_out.cpu().numpy()
            what = "%s nnz %d, fields %s" % (mt, nnz, "given" if fld is not None else "implicit")
            assert np.array_equal(got[:nnz], want), what
            assert (got[nnz:] == -7).all(), what + ": nothing is written behind the block"
            if nnz >= 64:
                plain = fa.hash_ids(fld, feat, NF, field_start=FS if ffm else None, model=mt.lower(), n_fields=F)
                assert not np.array_equal(want, plain), what + ": the map folds something"
    e.close()


def test_refusals_and_the_idle_rule():
    _, words = _map("FFM", False)
    plain = fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS, field_start=FS)
    with pytest.raises(fa.EngineError) as ei:
        plain.set_rare_fold(BITS, words)
    assert ei.value.code == fa.engine.E_INVALID and "FFM_FLAG_HASH_IDS" in str(ei.value)
    plain.close()
    g = fa.Group([0, 0], "FFM", NF, F, K, max_batch_rows=ROWS, field_start=FS, hash_ids=True)
    with pytest.raises(fa.EngineError) as ei:
        g.engines[0].set_rare_fold(BITS, words)
    assert ei.value.code == fa.engine.E_UNSUPPORTED
    g.close()
    e = _engine("FFM")
    lib = fa.load_library()
    assert lib.ffm_engine_set_rare_fold(e.h, 7, words.ctypes.data) == fa.engine.E_INVALID
    assert lib.ffm_engine_set_rare_fold(e.h, 31, words.ctypes.data) == fa.engine.E_INVALID
    assert lib.ffm_engine_set_rare_fold(None, BITS, words.ctypes.data) == fa.engine.E_INVALID
    with pytest.raises(ValueError):
        e.set_rare_fold(BITS, words[:3])
    e.set_rare_fold(None)  # (off when it is off already)
    # a staged block that waits to be trained: the engine is not idle
    c = _blocks("FFM", False)[0]
    e.stage_batch(c)
    with pytest.raises(fa.EngineError) as ei:
        e.set_rare_fold(BITS, words)
    assert ei.value.code == fa.engine.E_INVALID and "idle" in str(ei.value)
    e.train_staged(None, None)
    e.set_rare_fold(BITS, words)
    e.set_rare_fold(BITS, words)  # (a map replaces a map)
    e.sync()
    e.close()


# ---- 4. the filtered sketch -------------------------------------------------------------------------------


@pytest.mark.parametrize("with_field", [True, False], ids=["field array", "no field array"])
def test_filtered_sketch_counts_the_folded_entries(with_field):
    n_fields, nnz, bits = 8, 4099, 12
    field, feat = entries(nnz, n_fields, seed=31)
    fld = field if with_field else None
    counts = rare_ref.np_counts(fld, feat, n_fields, bits, 3)[0]
    words = rare_ref.np_keep(counts, 3)[0]
    folded = rare_ref.np_fold(fld, feat, n_fields, bits, words)
    assert (folded != feat).mean() > 0.1
    want = sketch_ref.np_sketch(fld, folded, n_fields)
    plain = sketch_ref.np_sketch(fld, feat, n_fields)
    assert not np.array_equal(want[0], plain[0]) and want[1:] == plain[1:]
    for how in ("pageable", "zero_copy", "zero_copy_offset", "device"):
        sk = fa.FieldSketch(n_fields)
        sk.set_filter(bits, words)
        feed(sk, fld, feat, how)
        reg, nv, nb = sk.read()
        assert np.array_equal(reg, want[0]) and (nv, nb) == want[1:], how
        sk.close()
    sk = fa.FieldSketch(n_fields)
    sk.set_filter(bits, words)
    sk.set_filter(None)
    sk.add(fld, feat)
    assert np.array_equal(sk.read()[0], plain[0]), "filter off: the plain sketch"
    with pytest.raises(ValueError):
        sk.set_filter(bits, words[:2])
    sk.close()
