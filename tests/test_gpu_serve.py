"""Serving engines (include/ffm_engine.h "Serving engines"; csrc/kernels_serve.h, csrc/engine_serve.h): an
engine that stores the bias, lin_w and a latent table of w alone, in fp32 bits or IEEE binary16.

The reference everywhere is the oracle (oracle/pyoracle.CpuModel) holding the DECODED weights --
vec_w.astype(float16).astype(float32) for fp16, vec_w itself for fp32: its predict_batch on those weights is
the expected output bit for bit (NaN with NaN), losses by util.loss_close.  Nothing here has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import CpuModel, Csr
from util import (EDGE_COUNTS, ROW_FIELDS, ROW_IDS_PER_FIELD, ROW_LENGTHS, STRESS_HP, assert_bitwise, assert_rows_bitwise,
                  assert_state_bitwise, block_ids_per_field, loss_close, occurrence_block, rand_state, row_length_block,
                  take_rows)

pytestmark = pytest.mark.gpu

NF = ROW_FIELDS * ROW_IDS_PER_FIELD  # 12 000 features, 6 fields
LENGTHS = [n for n in ROW_LENGTHS if n <= 128]
FORMATS = ("f32", "f16")
MAX_ROWS = 128
REFUSAL = "a serving engine holds no accumulators"


def decoded(w, fmt):
    """What a serving engine of format `fmt` holds for the fp32 weights w, as fp32."""
    if fmt == "f32":
        return np.ascontiguousarray(w, np.float32)
    with np.errstate(over="ignore"):
        return np.asarray(w, np.float32).astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ladder_block(seed=3):
    blk, nf = row_length_block("FFM", ROW_FIELDS, ROW_IDS_PER_FIELD, seed, lengths=LENGTHS)
    assert nf == NF and blk.n_rows % 4 != 0 and int(np.diff(blk.row_ptr).max()) == 128
    return blk


@functools.lru_cache(maxsize=2)
def ladder_weights(k):
    """The weights of the ladder cases at k factors: rand_state's vec_w, lin_w and bias (read-only)."""
    o = CpuModel("oracle", "FFM", NF, ROW_FIELDS, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(1000 + k), o)
    for a in st.values():
        a.setflags(write=False)
    return st


def oracle_with(k, bias, lin_w, vec_w, n_feats=NF, n_fields=ROW_FIELDS):
    o = CpuModel("oracle", "FFM", n_feats, n_fields, k, **STRESS_HP)
    st = o.zero_state()
    st["bias3"][0] = np.float32(bias)
    st["lin_w"][...] = lin_w
    st["vec_w"][...] = vec_w
    o.set_state(st)
    return o


def serving(k, fmt, st=None, **kw):
    kw.setdefault("max_batch_rows", MAX_ROWS)
    e = fa.Engine("FFM", kw.pop("n_feats", NF), kw.pop("n_fields", ROW_FIELDS), k, skip_init=kw.pop("skip_init", True),
                  serve=fmt, **dict(STRESS_HP, **kw))
    if st is not None:
        e.set_weights(bias=st["bias3"][:1], lin_w=st["lin_w"], vec_w=st["vec_w"])
    return e


def check_predict(e, o, blk, what):
    for prob in (False, True):
        want, wl = o.predict_batch(blk, output_prob=prob)
        got, gl = e.predict_batch(blk, output_prob=prob)
        assert_rows_bitwise(got, want, blk, "%s %s" % (what, "probabilities" if prob else "logits"))
        assert loss_close(gl, wl), "%s: loss sum %r vs %r" % (what, gl, wl)


# ---- 1. the parity ladder --------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_parity_ladder(k, fmt):
    """Rows of 0 .. 128 entries (erased ids and fields, descending fields, an id twice, a row count that is
    no multiple of 4; 128 entries are 8128 pairs, many 256-term batches), and blocks of 1 and 5 rows."""
    st, blk = ladder_weights(k), ladder_block()
    e = serving(k, fmt, st)
    o = oracle_with(k, st["bias3"][0], st["lin_w"], decoded(st["vec_w"], fmt))
    check_predict(e, o, blk, "k=%d %s ladder" % (k, fmt))
    lens = np.diff(blk.row_ptr)
    longest = int(np.argmax(lens))
    check_predict(e, o, take_rows(blk, [longest]), "k=%d %s one row of %d" % (k, fmt, lens[longest]))
    five = [int(np.flatnonzero(lens == n)[0]) for n in (127, 0, 65, 1, 33)]
    check_predict(e, o, take_rows(blk, five), "k=%d %s five rows" % (k, fmt))
    e.close()


# ---- 2. fp32 serving is the training engine's prediction -------------------------------------------------

def test_f32_serving_equals_the_training_engine():
    k = 16
    st, blk = ladder_weights(k), ladder_block()
    t = fa.Engine("FFM", NF, ROW_FIELDS, k, skip_init=True, max_batch_rows=MAX_ROWS, **STRESS_HP)
    t.set_state({key: st[key] for key in st})
    s = serving(k, "f32", st)
    hist = []
    for e in (t, s):
        e.metrics_enable(eval=True)
    for prob in (False, True):
        a, la = t.predict_batch(blk, output_prob=prob)
        b, lb = s.predict_batch(blk, output_prob=prob)
        assert_rows_bitwise(b, a, blk, "serving f32 vs training engine, prob=%d" % prob)
        assert la == lb or (np.isnan(la) and np.isnan(lb))
    for e in (t, s):
        hist.append(e.metrics_histogram("eval"))
        e.close()
    assert hist[0][0].sum() + hist[0][1].sum() > 0
    assert np.array_equal(hist[0][0], hist[1][0]) and np.array_equal(hist[0][1], hist[1][1])


# ---- 3. the rounding rule --------------------------------------------------------------------------------

RF, RK, RNF = 4, 4, 96  # the rounding cases' model: 96 features x 16 elements


def rounding_table():
    f = np.float32
    up, dn = lambda x: np.nextafter(f(x), f(np.inf)), lambda x: np.nextafter(f(x), f(-np.inf))  # noqa: E731
    big_sub = f(2.0 ** -14 - 2.0 ** -24)  # the largest half subnormal
    sp = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, up(2.0 ** -25), dn(2.0 ** -25), -2.0 ** -25,
          big_sub, up(big_sub), dn(big_sub), 2.0 ** -14, up(2.0 ** -14), dn(2.0 ** -14),
          1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -11),
          65504.0, dn(65520.0), 65520.0, -65520.0, up(65520.0), 1e30, np.inf, -np.inf, np.nan, -0.0,
          1e-40, -1e-45, 2.0 ** -127, -2.0 ** -149, 2.0 ** -126]
    assert float(dn(65520.0)) == 65519.99609375
    rng = np.random.default_rng(77)
    n = RNF * RF * RK
    body = np.concatenate([rng.normal(0, 0.02, (n - len(sp)) // 2), rng.normal(0, 1.0, n - len(sp) - (n - len(sp)) // 2)])
    w = np.concatenate([np.array(sp, np.float64).astype(np.float32), body.astype(np.float32)])
    w = w[rng.permutation(n)].reshape(RNF, RF * RK)
    lin = rng.normal(0, 0.02, RNF).astype(np.float32)
    return w, lin


def test_fp16_rounding_rule_set_get_and_pack():
    w, lin = rounding_table()
    want = decoded(w, "f16")
    # the table holds what the rule is about (numpy is the rule: IEEE binary16, nearest even, subnormals kept)
    assert np.isinf(want[w == np.float32(65520.0)]).all() and (want[w == np.float32(65519.996)] == 65504.0).all()
    assert (want[w == np.float32(2.0 ** -25)] == 0).all() and (want[w == np.float32(2.0 ** -24)] == np.float32(2.0 ** -24)).all()
    rng = np.random.default_rng(5)
    # set_weights
    e = serving(RK, "f16", n_feats=RNF, n_fields=RF)
    e.set_weights(bias=np.float32([0.25]), lin_w=lin, vec_w=w)
    got = e.get_weights()
    assert_bitwise(got["vec_w"], want, "set_weights -> get_weights")
    assert_bitwise(got["lin_w"], lin, "lin_w stays fp32")
    assert got["bias"][0] == np.float32(0.25)
    e.close()
    # set_rows on a shuffled id list
    e = serving(RK, "f16", n_feats=RNF, n_fields=RF)
    ids = rng.permutation(RNF).astype(np.int32)
    e.set_rows(ids, dict(lin_w=lin[ids], vec_w=w[ids]))
    rows = e.get_rows(ids)
    assert sorted(rows) == ["lin_w", "vec_w"]
    assert_bitwise(rows["vec_w"], want[ids], "set_rows -> get_rows")
    assert_bitwise(rows["lin_w"], lin[ids], "set_rows -> get_rows lin_w")
    assert_bitwise(e.get_weights()["vec_w"], want, "set_rows -> get_weights")
    e.close()
    # pack_from a training engine holding the same table (its n and z are not looked at)
    t = fa.Engine("FFM", RNF, RF, RK, skip_init=True, max_batch_rows=MAX_ROWS, **STRESS_HP)
    st = rand_state(rng, t)
    st["vec_w"][...] = w
    st["lin_w"][...] = lin
    t.set_state(st)
    finite = np.isfinite(w)
    counts = dict(n_latent=w.size,
                  n_inexact=int(((want.view(np.uint32) != w.view(np.uint32)) & ~np.isnan(w)).sum()),
                  n_to_inf=int((finite & np.isinf(want)).sum()),
                  n_to_zero=int((~np.isnan(w) & (w != 0) & (want == 0)).sum()))
    assert counts["n_to_inf"] >= 4 and counts["n_to_zero"] >= 6 and counts["n_inexact"] > w.size // 2
    for fmt in FORMATS:
        e = serving(RK, fmt, n_feats=RNF, n_fields=RF)
        stats = e.pack_from(t)
        assert stats == (counts if fmt == "f16" else dict(n_latent=w.size, n_inexact=0, n_to_inf=0, n_to_zero=0)), (fmt, stats)
        got = e.get_weights()
        assert_bitwise(got["vec_w"], decoded(w, fmt), "pack_from " + fmt)
        assert_bitwise(got["lin_w"], lin, "pack_from lin_w " + fmt)
        assert got["bias"][0] == st["bias3"][0]
        e.close()
    assert_state_bitwise(t.get_state(), st, "pack_from leaves the training engine alone")
    t.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_create_time_contents_are_the_training_draws_rounded(fmt):
    seed, mean, sd = 1234, 0.01, 0.05
    e = serving(RK, fmt, n_feats=RNF, n_fields=RF, skip_init=False, seed=seed, init_mean=mean, init_stddev=sd)
    L = RF * RK
    want = decoded(fa.init_weights_host(seed, mean, sd, True, 0, RNF * L).reshape(RNF, L), fmt)
    got = e.get_weights()
    assert_bitwise(got["vec_w"], want, "create-time vec_w " + fmt)
    assert_bitwise(got["lin_w"], fa.init_weights_host(seed, mean, sd, False, 0, RNF), "create-time lin_w")
    assert got["bias"][0] == 0.0
    ids = np.array([95, 0, 17, 17, 42], np.int32)
    assert_bitwise(e.get_rows(ids)["vec_w"], want[ids], "create-time get_rows " + fmt)
    e.close()
    z = serving(RK, fmt, n_feats=RNF, n_fields=RF)  # FFM_FLAG_SKIP_INIT: zero bits
    assert not z.get_weights()["vec_w"].view(np.uint32).any()
    z.close()


# ---- 4. pack_from after real training --------------------------------------------------------------------

def test_pack_from_after_training():
    F, k, n_rows = 8, 16, 1024
    counts = [c for c in EDGE_COUNTS if c <= 257]
    nf = F * block_ids_per_field(n_rows)
    blocks = [occurrence_block(F, counts, n_rows, seed=60 + j)[0] for j in range(4)]
    t = fa.Engine("FFM", nf, F, k, learn=True, max_batch_rows=n_rows, seed=9, **STRESS_HP)
    for b in blocks[:3]:
        t.train_batch(b)
    stats = t.refresh_weights()
    assert stats["lat_moved"] > 0
    before = t.get_state()
    for fmt in FORMATS:
        s = fa.Engine("FFM", nf, F, k, max_batch_rows=n_rows, serve=fmt, skip_init=True, **STRESS_HP)
        ps = s.pack_from(t)
        assert ps["n_latent"] == nf * F * k
        o = oracle_with(k, before["bias3"][0], before["lin_w"], decoded(before["vec_w"], fmt), n_feats=nf, n_fields=F)
        check_predict(s, o, blocks[3], "packed %s after training" % fmt)
        s.close()
    assert_state_bitwise(t.get_state(), before, "the training engine after pack_from")
    t.close()


# ---- 5. every prediction entry point ---------------------------------------------------------------------

def own_pages(c):
    def cp(a):
        out = fa.page_aligned(a.size, a.dtype)
        out[:] = a
        return out
    return Csr(cp(c.row_ptr), cp(c.field), cp(c.feat), cp(c.val), cp(c.label))


def test_every_prediction_entry_point_gives_predict_batch_bits():
    k = 16
    st = ladder_weights(k)
    e = serving(k, "f16", st)
    blocks = [ladder_block(3), ladder_block(4), take_rows(ladder_block(3), []), ladder_block(5)]
    want = [(e.predict_batch(b)[0], e.predict_batch(b, output_prob=True)[0], e.predict_batch(b)[1]) for b in blocks]
    # _device (the row cap is the engine's max_row_nnz: 128)
    for b, (lg, pr, ls) in zip(blocks, want):
        if b.n_rows == 0:
            continue
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
        out = torch.full((b.n_rows,), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        e.predict_batch_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                               d["val"].data_ptr(), d["label"].data_ptr(), True, out.data_ptr(), loss.data_ptr())
        e.sync()
        assert_rows_bitwise(out.cpu().numpy(), pr, b, "predict_batch_device")
        assert loss_close(float(loss.cpu()[0]), ls)
    # _async without scores: the flush's loss sum; with scores: the bits; copied and zero-copy
    total = sum(w[2] for w in want)
    for zero_copy in (False, True):
        host = [own_pages(b) for b in blocks] if zero_copy else blocks
        if zero_copy:
            for b in host:
                e.pin_block(b)
        for b in host:
            e.predict_batch_async(b, zero_copy=zero_copy)
        got = e.train_flush()
        assert abs(got - total) <= 1e-9 * max(1.0, abs(total)), (zero_copy, got, total)
        for prob in (False, True):
            outs = [e.score_buffer(b.n_rows + 8) for b in blocks]
            for b, out in zip(host, outs):
                out[:] = np.float32(-7.0)
                e.predict_batch_async(b, zero_copy=zero_copy, scores=out, output_prob=prob)
            e.train_flush()
            for b, out, w in zip(blocks, outs, want):
                assert_rows_bitwise(out[:b.n_rows], w[1 if prob else 0], b, "async scores zero_copy=%d prob=%d" % (zero_copy, prob))
                assert (out[b.n_rows:] == np.float32(-7.0)).all()
            for out in outs:
                e.free_score_buffer(out)
        if zero_copy:
            for b in host:
                e.unpin_block(b)
    # field == NULL: regular rows, one entry per field in field order
    reg = synth.Generator(ROW_FIELDS, NF, "zipf", seed=11).block(101)
    lg = e.predict_batch(reg)[0]
    out = e.score_buffer(reg.n_rows)
    e.predict_batch_async(Csr(reg.row_ptr, None, reg.feat, reg.val, reg.label), scores=out)
    e.train_flush()
    assert_bitwise(out[:reg.n_rows], lg, "field == NULL rows")
    e.free_score_buffer(out)
    # hashed ids: a flagged engine on raw ids against this one on the host-hashed ids
    fs = (np.arange(ROW_FIELDS + 1) * ROW_IDS_PER_FIELD).astype(np.int32)
    h = serving(k, "f16", st, hash_ids=True, field_start=fs)
    rng = np.random.default_rng(8)
    raw = Csr(reg.row_ptr, reg.field, rng.integers(0, 2 ** 31 - 1, reg.feat.size).astype(np.int32), reg.val, reg.label)
    hashed = Csr(reg.row_ptr, reg.field, fa.hash_ids(reg.field, raw.feat, NF, fs), reg.val, reg.label)
    assert_bitwise(h.predict_batch(raw)[0], e.predict_batch(hashed)[0], "hash_ids on a serving engine")
    h.close()
    e.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------

def _rc(fn, *args):
    lib = fa.load_library()
    rc = fn(*args)
    return rc, lib.ffm_engine_last_error().decode()


def _create_rc(**over):
    lib = fa.load_library()
    cfg = fa.Config()
    lib.ffm_engine_default_config(ctypes.byref(cfg))
    cfg.n_feats, cfg.n_fields, cfg.n_factors, cfg.max_batch_rows, cfg.max_batch_nnz = 64, 4, 4, 16, 1024
    for key, v in over.items():
        setattr(cfg, key, v)
    h = ctypes.c_void_p()
    rc = lib.ffm_engine_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = lib.ffm_engine_last_error().decode()
    if rc == 0:
        lib.ffm_engine_destroy(h)
    return rc, msg, cfg


def test_refusals_leave_the_model_unchanged():
    k = 16
    st, blk = ladder_weights(k), ladder_block()
    e = serving(k, "f16", st)
    want = decoded(st["vec_w"], "f16")
    lib = e.lib
    w = np.ones(blk.n_rows, np.float32)
    one = np.zeros(1, np.float32)
    fp = one.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n = ctypes.c_int64(0)
    calls = {
        "train_batch": lambda: e.train_batch(blk),
        "train_batch_weighted": lambda: e.train_batch(blk, weight=w),
        "train_batch_async": lambda: e.train_batch_async(blk),
        "train_batch_async_weighted": lambda: e.train_batch_async(blk, weight=w),
        "train_batch_async_pinned": lambda: e.train_batch_async_pinned(blk),
        "stage_batch": lambda: e.stage_batch(blk),
        "stage_batch_weighted": lambda: e.stage_batch(blk, weight=w),
        "train_staged": lambda: e.train_staged(),
        "train_forward_staged": lambda: e.train_forward_staged(),
        "train_batch_device": lambda: e.train_batch_device(0, 0, None, None, None, None, None),
        "train_batch_device_weighted": lambda: e.train_batch_device(0, 0, None, None, None, None, None, weight=1),
        "train_forward_device": lambda: e.train_forward_device(0, 0, None, None, None, None, None, None),
        "train_forward_device_weighted": lambda: e.train_forward_device(0, 0, None, None, None, None, None, None, weight=1),
        "train_update_device": lambda: e.train_update_device(None),
        "prepare_device": lambda: e.prepare_device(0, 0, None, None, None, None),
        "set_state": lambda: e._check(lib.ffm_engine_set_state(e.h, fp, None, None, None, None, None)),
        "get_state": lambda: e._check(lib.ffm_engine_get_state(e.h, None, None, None, None, None, fp)),
        "changed_features": lambda: e._check(lib.ffm_engine_changed_features(e.h, None, 0, ctypes.byref(n))),
        "refresh_weights": lambda: e.refresh_weights(),
        "fill_state": lambda: e.fill_state(),
        "set_rows with n": lambda: e.set_rows(np.array([3], np.int32), dict(lin_n=one)),
        "get_rows with z": lambda: e._check(lib.ffm_engine_get_rows(e.h, 1, np.array([3], np.int32).ctypes.data_as(
            ctypes.POINTER(ctypes.c_int32)), None, None, None, None, None, fp)),
    }
    for name, call in calls.items():
        with pytest.raises(fa.EngineError) as ei:
            call()
        assert ei.value.code == fa.engine.E_UNSUPPORTED and REFUSAL in str(ei.value), (name, str(ei.value))
    for name, call in {"Engine.get_state": e.get_state, "Engine.sparse_state": e.sparse_state}.items():
        with pytest.raises(fa.EngineError):
            call()
    # all-NULL state calls have nothing to refuse
    assert lib.ffm_engine_set_state(e.h, None, None, None, None, None, None) == 0
    # a host block holding a 129-entry row: refused before anything is queued
    long_row = Csr(np.array([0, 129], np.int32), np.zeros(129, np.int32), np.arange(129, dtype=np.int32),
                   np.ones(129, np.float32), np.zeros(1, np.int32))
    for call in (lambda: e.predict_batch(long_row), lambda: e.predict_batch_async(long_row)):
        with pytest.raises(fa.EngineError) as ei:
            call()
        assert ei.value.code == fa.engine.E_CAPACITY
    assert e.blocks_pulled() == 0
    e.sync()
    # pack_from: a mismatched shape, a serving src
    other = fa.Engine("FFM", NF, ROW_FIELDS, 8, skip_init=True, max_batch_rows=MAX_ROWS, **STRESS_HP)
    for src in (other, e):
        with pytest.raises(fa.EngineError) as ei:
            e.pack_from(src)
        assert ei.value.code == fa.engine.E_INVALID
    other.close()
    got = e.get_weights()
    assert_bitwise(got["vec_w"], want, "the model after the refusals")
    assert_bitwise(got["lin_w"], st["lin_w"], "lin_w after the refusals")
    e.close()
    # create
    both = fa.engine.FLAG_SERVE_F32 | fa.engine.FLAG_SERVE_F16
    assert _create_rc(flags=both)[0] == fa.engine.E_INVALID
    assert _create_rc(flags=fa.engine.FLAG_SERVE_F16, max_row_nnz=129)[0] == fa.engine.E_INVALID
    assert _create_rc(flags=fa.engine.FLAG_SERVE_F16, max_row_nnz=128)[0] == 0
    for over in (dict(model_type=fa.FM), dict(model_type=fa.LR), dict(n_shards=2), dict(n_factors=6)):
        rc, msg, _ = _create_rc(flags=fa.engine.FLAG_SERVE_F32, **over)
        assert rc == fa.engine.E_UNSUPPORTED and msg, (over, rc, msg)
    cfg = _create_rc(flags=0)[2]
    cfg.flags = fa.engine.FLAG_SERVE_F16
    g = ctypes.c_void_p()
    dev = np.zeros(1, np.int32)
    rc = fa.load_library().ffm_group_create(ctypes.byref(cfg), 1, dev.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(g))
    assert rc == fa.engine.E_UNSUPPORTED


# ---- 7. model_bytes --------------------------------------------------------------------------------------

def test_model_bytes():
    nf, F, k = 1000, 5, 8
    L = F * k
    t = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=16)
    assert t.model_bytes() == 12 + 12 * nf + 12 * nf * L
    t.close()
    for fmt, B in (("f32", 4), ("f16", 2)):
        s = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=16, serve=fmt)
        assert s.model_bytes() == 4 + 4 * nf + B * nf * L
        s.close()
