"""Value buckets on the device (include/ffm_engine.h "Value buckets"), against the numpy restatement
(tests/bucket_ref.py).

  1. the histogram: read() is np.bincount word for word and n_valid / n_bad / n_nan are exact -- vector and tail
     lengths, with a field array and without, aligned and offset by one word, one call and three, pageable /
     page-locked / device arrays, one (field, value) 4096 times, keys that share a set of the kernel's cache;
  2. THE PIN: an engine with a bucket table fed RAW blocks equals a flagged engine without a table fed the
     host-bucketed blocks (bucket_ids, then fold_rare on the entries it left alone) -- logits, loss sums, every w, n,
     z and every score bit for bit -- through every path a host block can take, with and without a keep-map, on
     training and serving engines, for the candidates and the ablation;
  3. bucket_ids_device is the host composition; the refusals of set_buckets; set_buckets(None).
"""
import copy
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import bucket_ref
import ftrl_ffm_amd as fa
import rare_ref
from hash_ref import np_hash_ids
from oracle.pyoracle import Csr
from util import STRESS_HP, assert_bitwise, assert_state_bitwise

pytestmark = pytest.mark.gpu

f32 = np.float32
F, BUCKETED, B = 5, (1, 3), 16
NNZ = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)


# ---- 1. the histogram --------------------------------------------------------------------------------------


def entries(nnz, seed):
    """Values with a heavy head, both signs, zeros of both signs, infinities, NaNs; fields with bad ones mixed in."""
    rng = np.random.default_rng(seed)
    field = rng.integers(0, F, size=nnz).astype(np.int64)
    val = (rng.lognormal(0.0, 3.0, nnz) * np.where(rng.random(nnz) < 0.3, -1.0, 1.0)).astype(f32)
    kind = rng.integers(0, 16, size=nnz)
    field[kind == 0] = -1
    field[kind == 1] = F
    val[kind == 2] = np.nan
    val[kind == 3] = -0.0
    val[kind == 4] = 0.0
    val[kind == 5] = np.inf
    val[kind >= 10] = 3.0  # half of a count column is one value
    return field.astype(np.int32), val


def pinned_copy(a):
    if a is None:
        return None
    p = fa.page_aligned(max(1, a.size), a.dtype)
    p[:a.size] = a
    assert fa.load_library().ffm_engine_pin_host(p.ctypes.data, max(1, p.size) * 4) == 0
    return p


def unpin(p):
    if p is not None:
        assert fa.load_library().ffm_engine_unpin_host(p.ctypes.data) == 0


def feed(vh, field, val, how):
    n = val.size
    if how == "pageable":
        vh.add(field, val)
    elif how in ("zero_copy", "zero_copy_offset"):  # offset: the arrays start one word into their pages -- no 16-byte loads
        o = 1 if how == "zero_copy_offset" else 0
        pad = lambda a: None if a is None else pinned_copy(np.concatenate([np.zeros(o, a.dtype), a]))  # noqa: E731
        pf, pv = pad(field), pad(val)
        try:
            vh.add(None if pf is None else pf[o:n + o], pv[o:n + o], zero_copy=True)
        finally:
            unpin(pf)
            unpin(pv)
    elif how in ("device", "device_offset"):
        o = 1 if how == "device_offset" else 0
        dev = lambda a: None if a is None else torch.from_numpy(np.concatenate([np.zeros(o, a.dtype), a])).cuda()  # noqa: E731
        df, dv = dev(field), dev(val)
        torch.cuda.synchronize()
        vh.add_device(n, None if df is None else df.data_ptr() + 4 * o, dv.data_ptr() + 4 * o if n else None)
        vh.read()  # (waits for the histogram's stream before the tensors go)
    else:
        raise ValueError(how)


HOWS = ("pageable", "zero_copy", "zero_copy_offset", "device", "device_offset")


def gpu_hist(field, val, how="pageable", cuts=None):
    vh = fa.ValueHistogram(F)
    try:
        if cuts is None:
            feed(vh, field, val, how)
        else:
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                feed(vh, None if field is None else field[lo:hi].copy(), val[lo:hi].copy(), how)
        return vh.read()
    finally:
        vh.close()


def assert_same(got, want, what):
    cnt, wcnt = got[0], want[0]
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    assert cnt.dtype == np.uint64 and cnt.shape == wcnt.shape == (F, bucket_ref.BINS)
    bad = np.argwhere(cnt != wcnt)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), [int(cnt[tuple(i)]) for i in bad[:5]], [int(wcnt[tuple(i)]) for i in bad[:5]])


@pytest.mark.parametrize("with_field", [True, False], ids=["field array", "no field array"])
def test_histogram_is_bincount(with_field):
    for nnz in NNZ:
        field, val = entries(nnz, seed=nnz)
        fld = field if with_field else None
        want = bucket_ref.np_hist(fld, val, F)
        assert int(want[0].sum()) == want[1] - want[3]
        if nnz == 4099:
            assert want[3] > 0 and (not with_field or want[2] > 0) and int(want[0].max()) > 100
        for how in HOWS:
            assert_same(gpu_hist(fld, val, how), want, (nnz, how))
        if nnz >= 63 and with_field:
            cuts = [0, nnz // 3, nnz // 3 + 1 + nnz // 2, nnz]
            for how in ("pageable", "zero_copy", "device"):
                assert_same(gpu_hist(fld, val, how, cuts), want, (nnz, how, "three calls"))
    # rows without a field array in three calls: each call's entry p is field p mod F
    field, val = entries(4099, seed=1)
    cuts = [0, 5 * 100, 5 * 100 + 7, 4099]
    own = np.concatenate([np.arange(hi - lo) % F for lo, hi in zip(cuts[:-1], cuts[1:])]).astype(np.int32)
    assert_same(gpu_hist(None, val, "pageable", cuts), bucket_ref.np_hist(own, val, F), "no field array, three calls")


def test_one_value_4096_times_and_keys_that_share_a_set():
    """The contention path (one word of the cache takes every entry) and the eviction path: the cache holds two keys
    per set, the set being the top 10 bits of key * 0x9e3779b1 with key = field << 16 | bin (kernels_valhist.h) --
    five keys of one set, interleaved, evict one another all the way."""
    val = np.full(4096, 123.5, f32)
    field = np.full(4096, 3, np.int32)
    want = bucket_ref.np_hist(field, val, F)
    assert int(want[0].max()) == 4096
    for how in ("pageable", "zero_copy", "device"):
        assert_same(gpu_hist(field, val, how), want, ("one value", how))
    keys = np.arange(F * bucket_ref.BINS, dtype=np.uint64)
    sets = ((keys * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)) >> np.uint64(22)
    # bins of positive normal values only (so that each key is a value that can be written down)
    ok = ((keys & np.uint64(0xffff)) >= 0x8080) & ((keys & np.uint64(0xffff)) < 0xff80)
    target = int(np.bincount(sets[ok].astype(np.int64), minlength=1024).argmax())
    share = keys[ok & (sets == target)][:5]
    assert share.size == 5
    vals = ((((share & np.uint64(0xffff)) << np.uint64(16)) & np.uint64(0x7fffffff)).astype(np.uint32)).view(f32)
    flds = (share >> np.uint64(16)).astype(np.int32)
    b, nan = bucket_ref.np_bin(vals)
    assert not nan.any() and np.array_equal(flds.astype(np.int64) * bucket_ref.BINS + b, share.astype(np.int64))
    rng = np.random.default_rng(3)
    pick = rng.integers(0, 5, 4099)
    pick[:2000:2] = 0  # one of the five is hot
    field, val = flds[pick], vals[pick]
    want = bucket_ref.np_hist(field, val, F)
    assert np.count_nonzero(want[0]) == 5
    for how in ("pageable", "zero_copy", "device", "device_offset"):
        assert_same(gpu_hist(field, val, how), want, ("one set", how))


def test_pageable_call_longer_than_a_staging_chunk():
    """A pageable call is staged in chunks of 2^22 entries; without a field array the second chunk's fields go on
    where the first one's stopped (2^22 mod 7 = 2), with one both chunks' entries land where they belong.  NaNs and
    fields that do not count lie on both sides of the cut."""
    nnz, n_fields, cut = (1 << 22) + 7, 7, 1 << 22
    rng = np.random.default_rng(5)
    val = rng.integers(1, 200, size=nnz).astype(f32)  # (a count column: few bins, so a field that is off by two shows)
    val[cut:] = 2.0 ** np.arange(10, 17)  # (the second chunk's entries: a bin each)
    val[[5, 1000, cut - 2, cut - 1, cut, cut + 3, nnz - 1]] = np.nan

    def hist(field):
        vh = fa.ValueHistogram(n_fields)
        try:
            vh.add(field, val)
            got, want = vh.read(), bucket_ref.np_hist(field, val, n_fields)
        finally:
            vh.close()
        assert got[1:] == want[1:], (got[1:], want[1:])
        bad = np.argwhere(got[0] != want[0])
        assert bad.size == 0, (len(bad), bad[:5].tolist())
        return want

    assert hist(None)[1:] == (nnz, 0, 7)
    field = (np.arange(nnz, dtype=np.int64) * 5 + 3) % n_fields
    field[[7, cut - 3, cut - 1, cut + 1, cut + 3, nnz - 2]] = [-1, n_fields, -1, n_fields, 9, -7]  # (cut - 1, cut + 3: NaNs too)
    assert hist(field.astype(np.int32))[1:] == (nnz - 6, 6, 5)


def test_histogram_arguments():
    lib = fa.load_library()
    for bad in (0, -1, 4097):
        with pytest.raises(fa.EngineError) as ei:
            fa.ValueHistogram(bad)
        assert ei.value.code == fa.engine.E_INVALID, bad
    vh = fa.ValueHistogram(F)
    cnt, nv, nb, nn = vh.read()
    assert not cnt.any() and (nv, nb, nn) == (0, 0, 0)
    val = np.arange(8, dtype=f32)
    assert lib.ffm_engine_valhist_add(vh.h, -1, None, val.ctypes.data, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_valhist_add(vh.h, 8, None, None, 0) == fa.engine.E_INVALID
    assert lib.ffm_engine_valhist_add_device(vh.h, 8, None, None) == fa.engine.E_INVALID
    assert lib.ffm_engine_valhist_add(vh.h, 0, None, None, 0) == 0 and lib.ffm_engine_valhist_add_device(vh.h, 0, None, None) == 0
    assert lib.ffm_engine_valhist_add(vh.h, 8, None, val.ctypes.data, 1) == fa.engine.E_INVALID
    assert b"page-locked" in lib.ffm_engine_last_error()
    assert lib.ffm_engine_valhist_read(vh.h, None, None, None, None) == 0  # (every output may be NULL)
    vh.close()
    vh.close()  # (twice is fine)


# ---- 2. the pin ----------------------------------------------------------------------------------------------

K, NF, BITS = 4, 4000, 12
FS = (np.arange(F + 1) * (NF // F)).astype(np.int32)
ROWS, ROW_NNZ = 257, 12


def _value(rng):
    r = rng.random()
    if r < 0.3:
        return 2.0  # the heavy value
    if r < 0.33:
        return float("nan")
    if r < 0.36:
        return -0.0
    return float(f32(rng.lognormal(0.0, 2.0) * (-1.0 if rng.random() < 0.25 else 1.0)))


@functools.lru_cache(maxsize=None)
def _blocks(regular):
    """Three blocks of 257 rows: fields 1 and 3 numeric (raw ids a keep-map would fold, values with a heavy head, NaNs, -0.0, both
    signs), fields 0, 2, 4 categorical with raw ids from per-field pools; a few negative ids and, where a field array
    goes along, fields out of range.  regular: exactly one entry per field and row in field order."""
    rng = np.random.default_rng(11 + regular)
    pool = [rng.integers(0, 2 ** 31, 300, dtype=np.int64) for _ in range(F)]
    p = 1.0 / (1.0 + np.arange(300)) ** 1.1
    p /= p.sum()

    def entry(f):
        if f in BUCKETED:
            return (f, int(rng.integers(0, 2 ** 31)), _value(rng))  # (the raw id of a numeric entry is ignored)
        return (f, int(rng.choice(pool[f], p=p)), float(f32(0.5 + rng.random())))

    blocks = []
    for b in range(3):
        rows = []
        for r in range(ROWS):
            row = [entry(f) for f in range(F)]
            if not regular and rng.random() < 0.3:
                row += [entry(int(rng.integers(0, F))) for _ in range(int(rng.integers(1, 5)))]
            if rng.random() < 0.15:
                j = int(rng.integers(0, len(row)))
                row[j] = (row[j][0], -1 - int(rng.integers(0, 1000)), row[j][2])
            if not regular and rng.random() < 0.1:
                j = int(rng.integers(0, len(row)))
                row[j] = (F if rng.random() < 0.5 else -1, row[j][1], row[j][2])
            rows.append(row)
        while not regular and sum(len(r) for r in rows) % 4 != b + 1:
            rows[-1].append(entry(int(rng.integers(0, F))))
        assert max(len(r) for r in rows) <= ROW_NNZ
        blocks.append(Csr.from_rows(rows, rng.integers(0, 2, ROWS)))
    if not regular:
        assert sorted(int(c.row_ptr[-1]) % 4 for c in blocks) == [1, 2, 3]
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def _table(regular):
    """{field: edges} counted on the device from the blocks; the reference alone says that it is worth testing."""
    blocks = _blocks(regular)
    field = np.concatenate([c.field for c in blocks])
    val = np.concatenate([c.val for c in blocks])
    want = bucket_ref.np_hist(field, val, F)
    vh = fa.ValueHistogram(F)
    for c in blocks:
        vh.add(c.field, c.val)
    got = vh.read()
    vh.close()
    assert_same(got, want, "the blocks' histogram")
    table = {}
    for f in BUCKETED:
        e, dropped = bucket_ref.edges(want[0][f], B)
        assert e.size + 1 >= 3 and dropped >= 1, (f, e.size, dropped)
        assert np.array_equal(fa.bucket_edges(got[0][f], B).astype(np.int64), e)
        table[f] = e
    return table


@functools.lru_cache(maxsize=None)
def _keep_map(regular):
    """A keep-map that folds about half of the categorical entries (counted by the reference)."""
    blocks = _blocks(regular)
    field = np.concatenate([c.field for c in blocks])
    feat = np.concatenate([c.feat for c in blocks])
    counts = rare_ref.np_counts(field, feat, F, BITS, 65535)[0].astype(np.int64)
    words = rare_ref.np_keep(np.minimum(counts, 4), 4)[0]
    return words


def _variant(c, **kw):
    h = copy.copy(c)
    h.__dict__.pop("_ffm_csr_args", None)
    for key, v in kw.items():
        setattr(h, key, v)
    return h


def _host_bucketed(c, table, words, implicit=False, bare=False):
    """bucket_ids, then fold_rare on the entries it left alone: the block a flagged engine without a table takes."""
    fld = None if implicit else c.field
    val = None if bare else c.val
    ft, v, hit = fa.bucket_ids(fld, c.feat, val, F, table)
    wf, wv, whit = bucket_ref.np_apply(fld, c.feat, val, F, table)
    assert np.array_equal(ft, wf) and np.array_equal(v.view(np.uint32), wv.view(np.uint32)) and np.array_equal(hit, whit)
    assert 0.2 < hit.mean() < 0.6 and (ft[hit] == 65536).any() and np.unique(ft[hit]).size >= 4
    if words is not None:
        folded = fa.fold_rare(fld, c.feat, F, BITS, words)
        assert ((folded != c.feat) & ~hit).mean() > 0.05 and ((folded != c.feat) & hit).any(), "the map would fold bucketed entries too"
        ft = np.where(hit, ft, folded).astype(np.int32)
    return _variant(c, feat=ft, val=v)


def _own_pages_block(c):
    out = _variant(c)
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
        before = (cb.feat.copy(), None if cb.val is None else cb.val.copy())
        e.stage_batch(cb, zero_copy=zc, weight=wb)
        e.train_staged(out.data_ptr(), loss.data_ptr())
        e.sync()
        assert np.array_equal(cb.feat, before[0]), "the caller's buffers are never written"
        assert cb.val is None or np.array_equal(cb.val.view(np.uint32), before[1].view(np.uint32))
    finally:
        if zc:
            e.sync()
            e.unpin_block(cb)
            if weight is not None:
                e.lib.ffm_engine_unpin_host(wb.ctypes.data)
    return out[:c.n_rows].cpu().numpy(), float(loss.cpu()[0])


def _same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (np.isnan(a) and np.isnan(b))


def _engine(**kw):
    return fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS, max_batch_nnz=ROWS * ROW_NNZ, max_row_nnz=ROW_NNZ, field_start=FS, seed=9,
                     hash_ids=True, **dict(STRESS_HP, **kw))


def _pair(regular, with_map):
    """(a with the table -- and the keep-map --, b with neither, the table, the map's words or None, the state both start from)."""
    table = _table(regular)
    words = _keep_map(regular) if with_map else None
    a, b = _engine(), _engine()
    a.set_buckets(table)
    if with_map:
        a.set_rare_fold(BITS, words)
    for e in (a, b):
        e.fill_state(seed=6)
    init = a.get_state()
    assert_state_bitwise(b.get_state(), init, "twin engines")
    return a, b, table, words, init


@pytest.mark.parametrize("with_map", [False, True], ids=["no keep-map", "keep-map"])
def test_engine_with_a_table_on_raw_blocks_is_the_plain_engine_on_bucketed_blocks(with_map):
    a, b, table, words, init = _pair(False, with_map)
    blocks = _blocks(False)
    # w, n, z after the three blocks, through each path
    for path in ("host", "async", "staged", "staged_zc"):
        for weighted in (False, True):
            a.set_state(init)
            b.set_state(init)
            for i, c in enumerate(blocks):
                h = _host_bucketed(c, table, words)
                weight = _weights(c.n_rows, i) if weighted else None
                what = "%s, %s, block %d" % (path, "weighted" if weighted else "unweighted", i)
                lg_a, ls_a = _train(a, path, c, weight)
                lg_b, ls_b = _train(b, path, h, weight)
                if lg_a is not None:
                    assert_bitwise(lg_a, lg_b, what + ": logits")
                assert _same_double(ls_a, ls_b), (what, ls_a, ls_b)
            st = a.get_state()
            assert_state_bitwise(st, b.get_state(), "%s after 3 blocks" % path)
            assert not np.array_equal(st["lin_n"], init["lin_n"]), "the blocks must train something"
    # val=None: every value is 1.0, bucketed like any other
    for path in ("host", "async", "staged", "staged_zc"):
        c = blocks[0]
        ft, v, hit = fa.bucket_ids(c.field, c.feat, None, F, table)
        if words is not None:
            ft = np.where(hit, ft, fa.fold_rare(c.field, c.feat, F, BITS, words)).astype(np.int32)
        h = _variant(c, feat=ft, val=v)
        assert (v == 1.0).all() and 1 <= np.unique(ft[hit]).size <= 2
        a.set_state(init)
        b.set_state(init)
        lg_a, ls_a = _train(a, path, _variant(c, val=None), None)
        lg_b, ls_b = _train(b, path, h, None)
        if lg_a is not None:
            assert_bitwise(lg_a, lg_b, path + ", val=None: logits")
        assert _same_double(ls_a, ls_b), (path, ls_a, ls_b)
        assert_state_bitwise(a.get_state(), b.get_state(), path + ", val=None")
    # the table changes what is trained: the plain engine on the RAW block ends elsewhere
    a.set_state(init)
    b.set_state(init)
    la = a.train_batch(blocks[0])[0]
    lb = b.train_batch(blocks[0])[0]
    assert not np.array_equal(la, lb)
    # prediction: synchronous and pipelined, with scores
    a.set_state(init)
    b.set_state(init)
    scores = [e.score_buffer(ROWS) for e in (a, b)]
    for c in blocks:
        h = _host_bucketed(c, table, words)
        for prob in (False, True):
            out_a, ls_a = a.predict_batch(c, output_prob=prob)
            out_b, ls_b = b.predict_batch(h, output_prob=prob)
            assert_bitwise(out_a, out_b, "predict_batch")
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
            assert_bitwise(scores[0][:c.n_rows], scores[1][:c.n_rows], "pipelined scores")
            assert_bitwise(scores[0][:c.n_rows], out_a, "pipelined scores are predict_batch's")
            if zc:
                a.unpin_block(ca)
                b.unpin_block(cb)
    # the ablation: every variant's scores and loss
    for e in (a, b):
        e.ablation_enable()
    c = blocks[1]
    out_a, ls_a = a.predict_ablated(c)
    out_b, ls_b = b.predict_ablated(_host_bucketed(c, table, words))
    assert_bitwise(out_a, out_b, "predict_ablated")
    assert ls_a.tobytes() == ls_b.tobytes()
    assert not np.array_equal(out_a[1], out_a[F]) and not np.array_equal(out_a[3], out_a[F]), "the bucketed fields matter"
    # set_buckets(None) restores the unbucketed results (the keep-map, if any, stays: b gets it too)
    a.set_buckets(None)
    if with_map:
        b.set_rare_fold(BITS, words)
    for path in ("host", "staged"):
        a.set_state(init)
        b.set_state(init)
        lg_a, ls_a = _train(a, path, blocks[0], None)
        lg_b, ls_b = _train(b, path, blocks[0], None)
        assert_bitwise(lg_a, lg_b, "table off: logits")
        assert _same_double(ls_a, ls_b)
        assert_state_bitwise(a.get_state(), b.get_state(), "table off")
    for e, s in zip((a, b), scores):
        e.free_score_buffer(s)
        e.close()


@pytest.mark.parametrize("with_map", [False, True], ids=["no keep-map", "keep-map"])
def test_blocks_without_a_field_array(with_map):
    """field == NULL (one entry per field in field order): the upload kernel buckets by the fields it writes."""
    a, b, table, words, init = _pair(True, with_map)
    for c in _blocks(True):
        assert int(c.row_ptr[-1]) == ROWS * F
        h = _host_bucketed(c, table, words, implicit=True)
        assert np.array_equal(h.feat, _host_bucketed(c, table, words).feat)
        for bare in (False, True):
            ca = _variant(c, field=None, val=None) if bare else _variant(c, field=None)
            cb = h
            if bare:
                ft, v, hit = fa.bucket_ids(None, c.feat, None, F, table)
                if words is not None:
                    ft = np.where(hit, ft, fa.fold_rare(None, c.feat, F, BITS, words)).astype(np.int32)
                cb = _variant(c, feat=ft, val=v)
            for path in ("async", "staged", "staged_zc"):
                what = "no field array, %s%s" % (path, ", val=None" if bare else "")
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


@pytest.mark.parametrize("serve", ["f32", "f16"])
def test_serving_engines_and_candidates(serve):
    table, words = _table(False), _keep_map(False)
    t = _engine()
    t.fill_state(seed=6)
    w = t.get_weights()
    t.close()
    mk = lambda: fa.Engine("FFM", NF, F, K, skip_init=True, serve=serve, max_batch_rows=4 * ROWS, max_batch_nnz=4 * ROWS * ROW_NNZ,  # noqa: E731
                           field_start=FS, hash_ids=True, **STRESS_HP)
    a, b = mk(), mk()
    for e in (a, b):
        e.set_weights(bias=w["bias"], lin_w=w["lin_w"], vec_w=w["vec_w"])
    a.set_buckets(table)
    a.set_rare_fold(BITS, words)
    for c in _blocks(False):
        h = _host_bucketed(c, table, words)
        for prob in (False, True):
            assert_bitwise(a.predict_batch(c, output_prob=prob)[0], b.predict_batch(h, output_prob=prob)[0], "serving predict_batch")
    # candidates: the context holds fields 0 .. 1, every candidate fields 2 .. 4 -- a bucketed field on each side
    c = _blocks(True)[0]
    n_req, per = 5, 7
    rows = lambda blk, lo, hi, cols: Csr.from_rows(  # noqa: E731
        [[(int(blk.field[r * F + j]), int(blk.feat[r * F + j]), float(blk.val[r * F + j])) for j in cols] for r in range(lo, hi)],
        np.zeros(hi - lo, np.int32))
    rq = (np.arange(n_req + 1) * per).astype(np.int32)
    ctx, cand = rows(c, 0, n_req, range(0, 2)), rows(c, n_req, n_req + n_req * per, range(2, 5))

    def bucketed(blk):
        ft, v, hit = fa.bucket_ids(blk.field, blk.feat, blk.val, F, table)
        assert hit.any()
        return _variant(blk, feat=np.where(hit, ft, fa.fold_rare(blk.field, blk.feat, F, BITS, words)).astype(np.int32), val=v)

    for prob in (False, True):
        got = a.score_candidates(ctx, rq, cand, output_prob=prob)
        assert_bitwise(got, b.score_candidates(bucketed(ctx), rq, bucketed(cand), output_prob=prob), "score_candidates")
        assert_bitwise(got, a.predict_batch(fa.spell_out_candidates(ctx, rq, cand), output_prob=prob)[0], "candidates vs predict_batch")
    assert not np.array_equal(a.score_candidates(ctx, rq, cand), b.score_candidates(ctx, rq, cand)), "the table changes the scores"
    a.set_buckets(None)
    a.set_rare_fold(None)
    assert_bitwise(a.score_candidates(ctx, rq, cand), b.score_candidates(ctx, rq, cand), "table off")
    a.close()
    b.close()


# ---- 3. bucket_ids_device, refusals ----------------------------------------------------------------------------


@pytest.mark.parametrize("with_map", [False, True], ids=["no keep-map", "keep-map"])
def test_bucket_ids_device_is_the_host_composition(with_map):
    table = _table(False)
    words = _keep_map(False) if with_map else None
    e = _engine()
    e.set_buckets(table)
    if with_map:
        e.set_rare_fold(BITS, words)
    c = _blocks(False)[0]
    for nnz in (0, 1, 3, 4, 5, 64, 65, 255, 1027):
        for fld in (c.field[:nnz].copy(), None):
            feat, val = c.feat[:nnz].copy(), c.val[:nnz].copy()
            ft, v, hit = fa.bucket_ids(fld, feat, val, F, table)
            if with_map:
                ft = np.where(hit, ft, fa.fold_rare(fld, feat, F, BITS, words)).astype(np.int32)
            want = fa.hash_ids(fld, ft, NF, field_start=FS, n_fields=F)
            assert np.array_equal(want, np_hash_ids(fld, ft, NF, F, FS, True))
            for o in (0, 1):  # (o = 1: arrays one word off a 16-byte boundary)
                pad = lambda x: torch.from_numpy(np.concatenate([np.zeros(o, x.dtype), x, np.zeros(1, x.dtype)])).cuda()  # noqa: E731
                d_feat, d_val = pad(feat), pad(val)
                d_field = pad(fld) if fld is not None else None
                d_out = torch.full((nnz + 8,), -7, dtype=torch.int32, device="cuda")
                d_vout = torch.full((nnz + 8,), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                at = 4 * o
                e.bucket_ids_device(nnz, d_field.data_ptr() + at if d_field is not None else None, d_feat.data_ptr() + at,
                                    d_val.data_ptr() + at, d_out.data_ptr() + 4 * o, d_vout.data_ptr() + 4 * o)
                e.sync()
                got, gv = d_out.cpu().numpy(), d_vout.cpu().numpy()
                what = "nnz %d, fields %s, offset %d" % (nnz, "given" if fld is not None else "implicit", o)
                assert np.array_equal(got[o:o + nnz], want), what
                assert np.array_equal(gv[o:o + nnz].view(np.uint32), v.view(np.uint32)), what
                assert (got[:o] == -7).all() and (got[o + nnz:] == -7).all() and (gv[o + nnz:] == -7.0).all(), what + ": nothing is written outside the block"
    # hash_ids_device keeps taking ids as they are
    feat = c.feat[:257].copy()
    d_feat, d_field = torch.from_numpy(feat).cuda(), torch.from_numpy(c.field[:257].copy()).cuda()
    d_out = torch.zeros(257, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.hash_ids_device(257, d_field.data_ptr(), d_feat.data_ptr(), d_out.data_ptr())
    e.sync()
    raw = fa.fold_rare(c.field[:257], feat, F, BITS, words) if with_map else feat
    assert np.array_equal(d_out.cpu().numpy(), fa.hash_ids(c.field[:257], raw, NF, field_start=FS, n_fields=F))
    e.close()


def test_refusals_and_the_idle_rule():
    table = _table(False)
    plain = fa.Engine("FFM", NF, F, K, max_batch_rows=ROWS, field_start=FS)
    with pytest.raises(fa.EngineError) as ei:
        plain.set_buckets(table)
    assert ei.value.code == fa.engine.E_INVALID and "FFM_FLAG_HASH_IDS" in str(ei.value)
    plain.close()
    lr = fa.Engine("LR", NF, 1, K, max_batch_rows=ROWS, hash_ids=True)
    with pytest.raises(fa.EngineError) as ei:
        lr.set_buckets({0: [5]})
    assert ei.value.code == fa.engine.E_INVALID and "FFM" in str(ei.value)
    lr.close()
    g = fa.Group([0, 0], "FFM", NF, F, K, max_batch_rows=ROWS, field_start=FS, hash_ids=True)
    with pytest.raises(fa.EngineError) as ei:
        g.engines[0].set_buckets(table)
    assert ei.value.code == fa.engine.E_UNSUPPORTED
    g.close()
    e = _engine()
    with pytest.raises(fa.EngineError) as ei:
        e.set_buckets({1: [9, 8, 7]})
    assert ei.value.code == fa.engine.E_INVALID and "strictly ascending" in str(ei.value)
    with pytest.raises(fa.EngineError) as ei:
        e.set_buckets({1: [9, 9]})
    assert ei.value.code == fa.engine.E_INVALID
    lib = fa.load_library()
    n_edges = np.array([-1, 256, -1, -1, -1], np.int32)
    edges = np.zeros((F, 255), np.uint16)
    assert lib.ffm_engine_set_buckets(e.h, n_edges.ctypes.data, edges.ctypes.data) == fa.engine.E_INVALID
    assert lib.ffm_engine_set_buckets(None, None, None) == fa.engine.E_INVALID
    with pytest.raises(ValueError):
        e.set_buckets({F: [1]})
    with pytest.raises(fa.EngineError):
        e.bucket_ids_device(0, None, None, None, None, None)  # (no table)
    e.set_buckets(None)  # (off when it is off already)
    # a staged block that waits to be trained: the engine is not idle
    c = _blocks(False)[0]
    e.stage_batch(c)
    with pytest.raises(fa.EngineError) as ei:
        e.set_buckets(table)
    assert ei.value.code == fa.engine.E_INVALID and "idle" in str(ei.value)
    e.train_staged(None, None)
    e.set_buckets(table)
    e.set_buckets(table)  # (a table replaces a table)
    e.sync()
    e.close()
