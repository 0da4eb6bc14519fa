"""Serving deltas (include/ffm_engine.h "Serving deltas"; csrc/kernels_delta.h, csrc/engine_delta.h):
ffm_engine_sync_weights brings a serving engine to a training engine's stored weights by comparing, keeps the
moved set on the device, and the raw row calls move rows in the table's own bits.

The definition is numpy: the target of a feature is its lin_w bits and its w row encoded to the table's format
(fp32: the bits; fp16: astype(np.float16).view(np.uint16)); a feature is moved iff any of those patterns differs
from what the serving engine stored before the call.  The result is pinned to ffm_engine_pack_weights on a second
serving engine.  Everything is compared bit for bit; nothing here has a tolerance."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from ftrl_ffm_amd.engine import E_INVALID, E_UNSUPPORTED
from util import STRESS_HP

pytestmark = pytest.mark.gpu

NF, FIELDS, ROWS = 2597, 5, 256  # 40 full bitmap words and a tail of 37 features
FORMATS = ("f32", "f16")
KS = (4, 8, 16, 32, 64)
ALL = np.arange(NF, dtype=np.int32)


def trainer(k, n_feats=NF, n_fields=FIELDS, **kw):
    return fa.Engine("FFM", n_feats, n_fields, k, max_batch_rows=ROWS, **dict(STRESS_HP, **kw))


def server(k, fmt, n_feats=NF, n_fields=FIELDS, **kw):
    return fa.Engine("FFM", n_feats, n_fields, k, max_batch_rows=ROWS, serve=fmt, **dict(STRESS_HP, **kw))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def raw_bits(e):
    """Everything a serving engine stores, as integers: (bias, lin_w [n_feats], table [n_feats, row_len])."""
    ids = np.arange(e.n_feats, dtype=np.int32)
    lw, lat = e.get_rows_raw(ids)
    assert lat.dtype == (np.uint16 if e.serve == "f16" else np.float32) and lat.shape == (e.n_feats, e.row_len)
    return bits(e.get_weights()["bias"]).copy(), bits(lw).copy(), bits(lat).copy()


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("bias", "lin_w", "table")):
        bad = np.flatnonzero(x.ravel() != y.ravel())
        assert bad.size == 0, "%s: %d %s patterns differ, first at %d: %#x vs %#x" % (
            what, bad.size, name, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])


def target_bits(src, fmt):
    """The target of every feature in the format's own bits, from the training engine's stored weights."""
    w = src.get_weights()
    with np.errstate(over="ignore", invalid="ignore"):
        lat = bits(w["vec_w"]) if fmt == "f32" else w["vec_w"].astype(np.float16).view(np.uint16)
    return bits(w["bias"]).copy(), bits(w["lin_w"]).copy(), lat.copy()


def expected(prev, target):
    """(moved ids, stats) of a sync that found `prev` stored and has `target` to reach."""
    lin = prev[1] != target[1]
    lat = prev[2] != target[2]
    moved = np.flatnonzero(lin | lat.any(axis=1)).astype(np.int32)
    return moved, dict(n_moved=int(moved.size), n_lin_moved=int(lin.sum()), n_lat_moved=int(lat.sum()),
                       bias_moved=int(prev[0][0] != target[0][0]))


def checked_sync(dst, src, what, with_stats=False):
    """sync_from with the numpy definition beside it; returns the moved ids (and the stats)."""
    prev, target = raw_bits(dst), target_bits(src, dst.serve)
    want_ids, want = expected(prev, target)
    got = dst.sync_from(src)
    ids = dst.sync_moved()
    assert got == want, "%s: stats %r, numpy says %r" % (what, got, want)
    assert ids.dtype == np.int32 and np.array_equal(ids, want_ids), "%s: moved ids differ from numpy's" % what
    same_bits(raw_bits(dst), target, what + ": dst against the target")
    return (ids, got) if with_stats else ids


def blocks(seed, n, lo=0, hi=NF, n_fields=FIELDS):
    """n blocks of ROWS synthetic rows whose ids all lie in [lo, hi)."""
    g = synth.Generator(n_fields, NF, seed=seed)
    out = []
    for _ in range(n):
        b = g.block(ROWS)
        b.feat = np.ascontiguousarray(lo + b.feat.astype(np.int64) % (hi - lo), np.int32)
        out.append(b)
    return out


# ---- 1. fresh into fresh, training blocks, a sub-range -----------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k", KS)
def test_sync_follows_training(k, fmt):
    src, dst, ref = trainer(k), server(k, fmt), server(k, fmt)
    # a fresh training engine into a fresh serving engine of the same seed: nothing to do
    st = dst.sync_from(src)
    assert st == dict(n_moved=0, n_lin_moved=0, n_lat_moved=0, bias_moved=0), st
    assert dst.sync_moved().size == 0
    for b in blocks(100 + k, 3):
        src.train_batch(b)
    ids = checked_sync(dst, src, "k=%d %s after three blocks" % (k, fmt))
    assert 0 < ids.size < NF
    ref.pack_from(src)
    same_bits(raw_bits(dst), raw_bits(ref), "k=%d %s: sync_from against pack_from" % (k, fmt))
    # nothing happened in between: a second sync moves nothing and leaves an empty list
    st = dst.sync_from(src)
    assert st == dict(n_moved=0, n_lin_moved=0, n_lat_moved=0, bias_moved=0), st
    assert dst.sync_moved().size == 0
    same_bits(raw_bits(dst), raw_bits(ref), "k=%d %s: the second sync wrote something" % (k, fmt))
    # further blocks whose ids all lie in a sub-range move only ids inside it
    lo, hi = 700, 1500
    for b in blocks(200 + k, 2, lo, hi):
        src.train_batch(b)
    ids = checked_sync(dst, src, "k=%d %s sub-range" % (k, fmt))
    assert ids.size > 0 and ids.min() >= lo and ids.max() < hi, (ids.min(), ids.max())
    ref.pack_from(src)
    same_bits(raw_bits(dst), raw_bits(ref), "k=%d %s sub-range: sync_from against pack_from" % (k, fmt))
    for e in (src, dst, ref):
        e.close()


# ---- 2. crafted patterns -----------------------------------------------------------------------------------

# (n_feats, n_fields, k): the issue's shape at its shortest and longest row, and a row of 1088 elements --
# more than the 1024 a wave holds in flight, so its features take a second chunk
CRAFT_SHAPES = [(NF, FIELDS, 4), (NF, FIELDS, 64), (130, 17, 64)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", CRAFT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_crafted_patterns(shape, fmt):
    nf, F, k = shape
    src, dst = trainer(k, nf, F), server(k, fmt, nf, F)
    RL = src.row_len
    f = np.float32

    def put(i, lin_w=None, row=None):
        st = {}
        if lin_w is not None:
            st["lin_w"] = np.array([lin_w], f)
        if row is not None:
            st["vec_w"] = np.ascontiguousarray(row, f).reshape(1, RL)
        src.set_rows(np.array([i], np.int32), st)

    def sync(what, ids, n_lin, n_lat, bias=0):
        got, stats = checked_sync(dst, src, "%s %s: %s" % (shape, fmt, what), with_stats=True)
        st = dict(n_moved=len(ids), n_lin_moved=n_lin, n_lat_moved=n_lat, bias_moved=bias)
        assert got.tolist() == list(ids), "%s: moved %r, expected %r" % (what, got.tolist(), ids)
        assert stats == st, "%s: %r, expected %r" % (what, stats, st)

    row = src.get_rows(np.array([7], np.int32))["vec_w"][0].copy()
    # +0.0 -> -0.0 is moved: patterns, not values
    row[3] = f(0.0)
    put(7, row=row)
    sync("+0.0 stored", [7], 0, 1)
    row[3] = f(-0.0)
    put(7, row=row)
    sync("+0.0 -> -0.0", [7], 0, 1)
    # a change below half resolution: moved on f32, the same half on f16
    row[5] = f(1.0)
    put(7, row=row)
    sync("1.0 stored", [7], 0, 1)
    row[5] = f(1.0 + 2.0 ** -20)
    put(7, row=row)
    sync("1.0 -> 1.0 + 2^-20", [7] if fmt == "f32" else [], 0, 1 if fmt == "f32" else 0)
    # a NaN moves once; unchanged, its encoded bits are the stored ones
    row[0] = f(np.nan)
    put(7, row=row)
    sync("a NaN arrives", [7], 0, 1)
    sync("the NaN stays", [], 0, 0)
    # only lin_w changes
    put(11, lin_w=0.625)
    sync("lin_w alone", [11], 1, 0)
    # only the last element of a row changes
    last = src.get_rows(np.array([12], np.int32))["vec_w"][0].copy()
    last[RL - 1] = f(-3.5)
    put(12, row=last)
    sync("the last element of a row", [12], 0, 1)
    # the last bit of a word, the first bit of the next, the last feature of the tail
    for i in (63, 64, nf - 1):
        r = src.get_rows(np.array([i], np.int32))["vec_w"][0].copy()
        r[RL // 2] = f(0.75)
        put(i, lin_w=-0.25, row=r)
    sync("features 63, 64 and n_feats - 1", [63, 64, nf - 1], 3, 3)
    # only the bias changes: it is in no list
    src.set_weights(bias=np.array([0.3125], f))
    sync("the bias alone", [], 0, 0, bias=1)
    assert dst.get_weights()["bias"][0] == f(0.3125)
    src.close()
    dst.close()


# ---- 3. a consumer that only ever sees deltas ----------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_delta_chain(fmt):
    k = 16
    src, dst, consumer, ref = trainer(k), server(k, fmt), server(k, fmt), server(k, fmt)
    probe = blocks(999, 1)[0]
    for rnd, b in enumerate(blocks(300, 3)):
        src.train_batch(b)
        st = dst.sync_from(src)
        d = dst.export_delta()
        assert d["fmt"] == fmt and d["ids"].size == st["n_moved"] > 0
        assert d["lat"].dtype == (np.uint16 if fmt == "f16" else np.float32) and d["lat"].shape == (d["ids"].size, dst.row_len)
        consumer.apply_delta(d)
        same_bits(raw_bits(consumer), raw_bits(dst), "%s round %d: the consumer against dst" % (fmt, rnd))
        ref.pack_from(src)
        for prob in (False, True):
            got, gl = consumer.predict_batch(probe, output_prob=prob)
            want, wl = ref.predict_batch(probe, output_prob=prob)
            assert np.array_equal(bits(got), bits(want)), "%s round %d: predictions differ" % (fmt, rnd)
            assert gl == wl
    for e in (src, dst, consumer, ref):
        e.close()


# ---- 4. rows in the table's own bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_raw_round_trip(fmt):
    k = 8
    e = server(k, fmt)
    RL = e.row_len
    before = raw_bits(e)
    ids = np.array([NF - 1, 0, 64, 1300], np.int32)
    rng = np.random.default_rng(5)
    if fmt == "f16":
        lat = rng.integers(0, 1 << 16, (ids.size, RL)).astype(np.uint16)
        lat[1, 2] = 0x7e55  # a NaN with a payload
        lat[2, RL - 1] = 0xfdab
    else:
        lat = rng.integers(0, 1 << 32, (ids.size, RL), dtype=np.uint64).astype(np.uint32).view(np.float32)
        bits(lat)[1, 2] = 0x7fc12345
        bits(lat)[2, RL - 1] = 0xffabcdef
    lw = rng.normal(0, 1, ids.size).astype(np.float32)
    bits(lw)[3] = 0x7fc00099
    e.set_rows_raw(ids, lw, lat)
    got_lw, got_lat = e.get_rows_raw(ids)
    assert np.array_equal(bits(got_lw), bits(lw)) and np.array_equal(bits(got_lat), bits(lat))
    after = raw_bits(e)
    others = np.setdiff1d(ALL, ids)
    assert np.array_equal(after[1][others], before[1][others]) and np.array_equal(after[2][others], before[2][others])
    assert np.array_equal(after[2][ids], bits(lat)) and after[0][0] == before[0][0]
    # either array alone
    e.set_rows_raw(ids[:1], lin_w=np.array([2.5], np.float32))
    e.set_rows_raw(ids[1:2], lat=lat[:1])
    lw2, lat2 = e.get_rows_raw(ids[:2])
    assert lw2[0] == np.float32(2.5) and np.array_equal(bits(lat2[0]), bits(lat[0])) and np.array_equal(bits(lat2[1]), bits(lat[0]))
    assert bits(lw2)[1] == bits(lw)[1]
    # out-of-range ids: refused whole, as get_rows / set_rows refuse them
    held = raw_bits(e)
    for bad in ([3, NF], [-1, 3]):
        bad = np.array(bad, np.int32)
        for call in (lambda: e.get_rows_raw(bad), lambda: e.set_rows_raw(bad, np.zeros(2, np.float32), lat[:2])):
            with pytest.raises(fa.EngineError) as err:
                call()
            assert err.value.code == E_INVALID
        with pytest.raises(fa.EngineError) as err:
            e.get_rows(bad)
        assert err.value.code == E_INVALID
    same_bits(raw_bits(e), held, "%s: a refused raw call wrote something" % fmt)
    # no ids at all
    lw0, lat0 = e.get_rows_raw(np.zeros(0, np.int32))
    assert lw0.size == 0 and lat0.shape == (0, RL)
    e.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_refusals(fmt):
    k = 8
    other = "f16" if fmt == "f32" else "f32"
    src, dst, dst2 = trainer(k), server(k, fmt), server(k, fmt)
    for b in blocks(400, 1):
        src.train_batch(b)
    held = raw_bits(dst)

    def refused(call, code, what):
        with pytest.raises(fa.EngineError) as err:
            call()
        assert err.value.code == code, "%s: code %d, expected %d (%s)" % (what, err.value.code, code, err.value)
        same_bits(raw_bits(dst), held, what + ": dst changed")

    refused(lambda: dst.sync_moved(), E_INVALID, "sync_moved before any sync")
    t2 = trainer(k)
    refused(lambda: t2.sync_from(src), E_INVALID, "dst is a training engine")
    refused(lambda: dst.sync_from(dst2), E_INVALID, "src is a serving engine")
    for shape in ((NF + 1, FIELDS, k), (NF, FIELDS + 1, k), (NF, FIELDS, 2 * k)):
        odd = trainer(shape[2], shape[0], shape[1])
        refused(lambda: dst.sync_from(odd), E_INVALID, "src of shape %r" % (shape,))
        odd.close()
    refused(lambda: dst.sync_moved(), E_INVALID, "sync_moved after refused syncs only")
    refused(lambda: src.get_rows_raw(ALL[:3]), E_UNSUPPORTED, "get_rows_raw on a training engine")
    refused(lambda: src.set_rows_raw(ALL[:3], np.zeros(3, np.float32)), E_UNSUPPORTED, "set_rows_raw on a training engine")
    refused(lambda: src.export_delta(), E_UNSUPPORTED, "export_delta on a training engine")
    # a delta of the other format, and one of another row length
    for e2 in (server(k, other), server(2 * k, fmt)):
        t = trainer_like(e2, src)
        e2.sync_from(t)
        d = e2.export_delta()
        assert d["ids"].size > 0
        refused(lambda: dst.apply_delta(d), E_INVALID, "a delta of %s, row_len %d" % (d["fmt"], d["lat"].shape[1]))
        e2.close()
        if t is not src:
            t.close()
    # and the engine still works
    dst.sync_from(src)
    dst2.pack_from(src)
    same_bits(raw_bits(dst), raw_bits(dst2), "%s: sync after the refusals" % fmt)
    for e in (src, dst, dst2, t2):
        e.close()


def trainer_like(serving_engine, src):
    """A training engine of the serving engine's shape that has seen a block (src itself when the shapes agree)."""
    if serving_engine.n_factors == src.n_factors:
        return src
    t = trainer(serving_engine.n_factors)
    t.train_batch(blocks(401, 1)[0])
    return t
