"""One context against many candidates on a serving engine (include/ffm_engine.h "Scoring candidates";
csrc/kernels_serve.h serve_context_kernel / serve_candidate_kernel, csrc/engine_serve.h).

The reference is twofold and has NO tolerance: the same engine's predict_batch on the spelled-out rows
(fa.spell_out_candidates) and the oracle (oracle/pyoracle.CpuModel) holding the decoded weights.  Scores are
compared bit for bit, NaN with NaN, logits and probabilities."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block
from oracle.pyoracle import CpuModel
from util import ROW_FIELDS, ROW_IDS_PER_FIELD, STRESS_HP, assert_bitwise, assert_rows_bitwise, rand_state, take_rows

pytestmark = pytest.mark.gpu

F, PER = ROW_FIELDS, ROW_IDS_PER_FIELD
NF = F * PER  # 12 000 features, 6 fields
FORMATS = ("f32", "f16")
KS = (4, 8, 16, 32, 64)
MAX_ROWS = 256
CTX_LENGTHS = (0, 1, 2, 3, 17, 23, 24, 64, 65, 100, 127)
CAND_LENGTHS = (0, 1, 2, 28)  # and, for each context, the length that makes the row exactly 128
_i32p, _f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


# ---- the model ---------------------------------------------------------------------------------------------

def decoded(w, fmt):
    if fmt == "f32":
        return np.ascontiguousarray(w, np.float32)
    with np.errstate(over="ignore"):
        return np.asarray(w, np.float32).astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=2)
def weights(k):
    o = CpuModel("oracle", "FFM", NF, F, k, **STRESS_HP)
    st = rand_state(np.random.default_rng(1000 + k), o)
    for a in st.values():
        a.setflags(write=False)
    return st


def oracle(k, fmt):
    st = weights(k)
    o = CpuModel("oracle", "FFM", NF, F, k, **STRESS_HP)
    z = o.zero_state()
    z["bias3"][0] = st["bias3"][0]
    z["lin_w"][...] = st["lin_w"]
    z["vec_w"][...] = decoded(st["vec_w"], fmt)
    o.set_state(z)
    return o


def serving(k, fmt, **kw):
    st = weights(k)
    e = fa.Engine("FFM", NF, F, k, skip_init=True, serve=fmt, max_batch_rows=kw.pop("max_batch_rows", MAX_ROWS),
                  max_batch_nnz=MAX_ROWS * 128, **dict(STRESS_HP, **kw))
    e.set_weights(bias=st["bias3"][:1], lin_w=st["lin_w"], vec_w=st["vec_w"])
    return e


# ---- the ladder --------------------------------------------------------------------------------------------

def entries(rng, n):
    """n entries of multi-valued fields: any field, an id of its range; values 1.0 for half of them, else
    uniform in [0.25, 1.25), one in ten negative."""
    field = rng.integers(0, F, n)
    feat = field * PER + rng.integers(0, PER, n)
    val = np.where(rng.random(n) < 0.5, 1.0, rng.random(n) + 0.25)
    val = np.where(rng.random(n) < 0.1, -val, val)
    return [[int(f), int(i), float(np.float32(v))] for f, i, v in zip(field, feat, val)]


def spoil_context(ent):
    """Erased entries (id -1, id n_feats, field -1, field n_fields), a value of -0.0 and one id twice, wherever
    the context is long enough to hold them."""
    n = len(ent)
    for pos, what in ((0, "id-1"), (2, "idNF"), (5, "f-1"), (9, "fF"), (3, "-0.0"), (7, "twice")):
        if pos >= n:
            continue
        if what == "id-1":
            ent[pos][1] = -1
        elif what == "idNF":
            ent[pos][1] = NF
        elif what == "f-1":
            ent[pos][0] = -1
        elif what == "fF":
            ent[pos][0] = F
        elif what == "-0.0":
            ent[pos][2] = -0.0
        else:
            ent[pos][0], ent[pos][1] = ent[4][0], ent[4][1]  # entry 4's id again


def spoil_candidate(ent, ctx):
    n = len(ent)
    if n > 0 and len(ctx) > 1:
        ent[0][0], ent[0][1] = ctx[1][0], ctx[1][1]  # an id of the context again (entry 1 is never erased)
    for pos, what in ((1, "idNF"), (2, "-0.0"), (3, "f-1"), (4, "id-1"), (6, "fF")):
        if pos >= n:
            continue
        if what == "idNF":
            ent[pos][1] = NF
        elif what == "id-1":
            ent[pos][1] = -1
        elif what == "f-1":
            ent[pos][0] = -1
        elif what == "fF":
            ent[pos][0] = F
        else:
            ent[pos][2] = -0.0


def to_block(rows):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return Block(ptr, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.int32),
                 np.array([e[2] for e in flat], np.float32), np.zeros(len(rows), np.int32))


@functools.lru_cache(maxsize=None)
def ladder(seed=3):
    """(ctx, cand_req_ptr, cand): every context length twice -- clean, and spoiled (erasures, -0.0, an id twice;
    its candidates spoiled too, the first of them repeating an id of the context) --, each with candidates of
    0, 1, 2, 28 entries and of the length that makes the row exactly 128; requests without candidates first, in
    the middle and last.  Clean contexts of 24 with an empty candidate (276 pairs, all from the table, across a
    256-term batch) and of 23 with a one-entry candidate are part of it by construction; contexts of 64, 100 and
    127 give runs of context pairs that cross every multiple of 4, 16, 64, 128 and 256 terms (PPS * U for k = 64,
    32, 16, 8, 4)."""
    rng = np.random.default_rng(seed)
    ctxs, cands, per_req = [entries(rng, 5)], [], [0]
    for j, n in enumerate(CTX_LENGTHS):
        for spoiled in (False, True):
            ctx = entries(rng, n)
            if spoiled:
                spoil_context(ctx)
            lens = sorted(set(m for m in CAND_LENGTHS + (128 - n,) if n + m <= 128))
            for m in lens:
                c = entries(rng, m)
                if spoiled:
                    spoil_candidate(c, ctx)
                cands.append(c)
            ctxs.append(ctx)
            per_req.append(len(lens))
        if j == len(CTX_LENGTHS) // 2:
            ctxs.append(entries(rng, 40))
            per_req.append(0)
    ctxs.append(entries(rng, 128))
    per_req.append(0)
    if len(cands) % 4 == 0:  # (a last workgroup that is not whole)
        ctxs.insert(-1, entries(rng, 7))
        per_req.insert(-1, 1)
        cands.append(entries(rng, 3))
    rq = np.cumsum([0] + per_req).astype(np.int32)
    assert len(cands) % 4 != 0 and 64 < len(cands) <= MAX_ROWS and per_req[0] == 0 and per_req[-1] == 0
    return to_block(ctxs), rq, to_block(cands)


def take_requests(ctx, rq, cand, idx):
    """The requests idx with their candidates, in that order."""
    def rows(b, ids):
        ids = np.asarray(ids, np.int64)
        pos = np.concatenate([np.arange(b.row_ptr[r], b.row_ptr[r + 1]) for r in ids] + [np.zeros(0, np.int64)]).astype(np.int64)
        ptr = np.concatenate([[0], np.cumsum(np.diff(b.row_ptr)[ids])]).astype(np.int32)
        return Block(ptr, b.field[pos].copy(), b.feat[pos].copy(), b.val[pos].copy(), np.zeros(len(ids), np.int32))
    cids = np.concatenate([np.arange(rq[r], rq[r + 1]) for r in idx] + [np.zeros(0, np.int64)])
    new_rq = np.concatenate([[0], np.cumsum([rq[r + 1] - rq[r] for r in idx])]).astype(np.int32)
    return rows(ctx, idx), new_rq, rows(cand, cids)


@functools.lru_cache(maxsize=None)
def ladder_reference(k, fmt):
    """The oracle's (logits, probabilities) of the ladder's spelled-out rows on the decoded weights."""
    blk = fa.spell_out_candidates(*ladder())
    o = oracle(k, fmt)
    out = tuple(o.predict_batch(blk, output_prob=p)[0].copy() for p in (False, True))
    for a in out:
        a.setflags(write=False)
    return out


def check(e, o, ctx, rq, cand, what, want=None):
    blk = fa.spell_out_candidates(ctx, rq, cand)
    for prob in (False, True):
        got = e.score_candidates(ctx, rq, cand, output_prob=prob)
        name = "%s %s" % (what, "probabilities" if prob else "logits")
        assert_rows_bitwise(got, e.predict_batch(blk, output_prob=prob)[0], blk, name + " vs predict_batch")
        ref = want[int(prob)] if want is not None else o.predict_batch(blk, output_prob=prob)[0]
        assert_rows_bitwise(got, ref, blk, name + " vs the oracle")


# ---- 1. the ladder -----------------------------------------------------------------------------------------

def test_the_ladder_holds_what_it_must():
    ctx, rq, cand = ladder()
    nc, per = np.diff(ctx.row_ptr), np.diff(rq)
    own = np.diff(cand.row_ptr)
    req = np.repeat(np.arange(ctx.n_rows), per)
    assert set(CTX_LENGTHS) <= set(nc.tolist()) and cand.n_rows % 4 != 0
    assert per[0] == 0 and per[-1] == 0 and (per[1:-1] == 0).any()
    rows = set(zip(nc[req].tolist(), own.tolist()))
    assert (24, 0) in rows and (23, 1) in rows
    for n in CTX_LENGTHS:
        assert (n, 128 - n) in rows and (n, 0) in rows
    assert (ctx.feat == -1).any() and (ctx.feat == NF).any() and (ctx.field == -1).any() and (ctx.field == F).any()
    assert (cand.feat == -1).any() and (cand.feat == NF).any() and (cand.field == -1).any() and (cand.field == F).any()
    neg0 = np.float32(-0.0).view(np.uint32)
    assert (ctx.val.view(np.uint32) == neg0).any() and (cand.val.view(np.uint32) == neg0).any() and (ctx.val != 1).any()
    r = int(np.flatnonzero(nc == 17)[1])  # the spoiled context of 17: entry 4's id at 7 again, entry 1's in a candidate
    ids = ctx.feat[ctx.row_ptr[r]:ctx.row_ptr[r + 1]]
    assert ids[7] == ids[4] and cand.feat[cand.row_ptr[rq[r] + 1]] == ids[1]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k", KS)
def test_parity_ladder(k, fmt):
    e = serving(k, fmt)
    check(e, None, *ladder(), "k=%d %s ladder" % (k, fmt), want=ladder_reference(k, fmt))
    e.close()


# ---- 2. a regrown or stale table leaks nothing ---------------------------------------------------------------

def test_a_sequence_of_calls_small_large_small():
    k, fmt = 16, "f16"
    ctx, rq, cand = ladder()
    nc = np.diff(ctx.row_ptr)
    small = [int(r) for r in np.flatnonzero(nc <= 3)]
    large = [int(r) for r in np.flatnonzero((nc >= 17) & (nc <= 100))]
    other = [int(r) for r in np.flatnonzero(nc <= 7)][::-1]
    e, o = serving(k, fmt), oracle(k, fmt)
    for name, idx in (("small", small), ("large", large), ("small again", other)):
        check(e, o, *take_requests(ctx, rq, cand, idx), "sequence: " + name)
    e.close()


# ---- 3. fp32 serving against a training engine -----------------------------------------------------------------

def test_f32_scores_equal_the_training_engines_prediction():
    k = 16
    st = weights(k)
    t = fa.Engine("FFM", NF, F, k, skip_init=True, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 128, **STRESS_HP)
    t.set_state({key: st[key] for key in st})
    s = fa.Engine("FFM", NF, F, k, skip_init=True, serve="f32", max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 128, **STRESS_HP)
    s.pack_from(t)
    ctx, rq, cand = ladder()
    blk = fa.spell_out_candidates(ctx, rq, cand)
    for prob in (False, True):
        assert_rows_bitwise(s.score_candidates(ctx, rq, cand, output_prob=prob), t.predict_batch(blk, output_prob=prob)[0], blk,
                            "packed f32 vs the training engine, prob=%d" % prob)
    t.close()
    s.close()


# ---- the raw calls -------------------------------------------------------------------------------------------

def raw_call(e, ctx, rq, cand, out, n_req=None, n_cand=None, null=()):
    def a(name, arr, tp):
        return None if name in null or arr is None else np.ascontiguousarray(arr).ctypes.data_as(tp)
    rq = np.ascontiguousarray(rq, np.int32)
    rc = e.lib.ffm_engine_score_candidates(
        e.h, ctx.n_rows if n_req is None else n_req, a("ctx_ptr", ctx.row_ptr, _i32p), a("ctx_field", ctx.field, _i32p),
        a("ctx_feat", ctx.feat, _i32p), a("ctx_val", ctx.val, _f32p), a("cand_req_ptr", rq, _i32p),
        cand.n_rows if n_cand is None else n_cand, a("cand_ptr", cand.row_ptr, _i32p), a("cand_field", cand.field, _i32p),
        a("cand_feat", cand.feat, _i32p), a("cand_val", cand.val, _f32p), 0, a("out", out, _f32p))
    return rc, e.lib.ffm_engine_last_error().decode()


def device_scores(e, ctx, rq, cand, prob, ctx_cap=None):
    """score_candidates_device on copies of the arrays in HBM.  Returns (scores, the EngineError sync raised or None)."""
    def up(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    d = [up(ctx.row_ptr, np.int32), up(ctx.field, np.int32), up(ctx.feat, np.int32), up(ctx.val, np.float32), up(rq, np.int32),
         up(cand.row_ptr, np.int32), up(cand.field, np.int32), up(cand.feat, np.int32), up(cand.val, np.float32)]
    out = torch.full((max(1, cand.n_rows),), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() if t.numel() else None for t in d]
    cap = int(np.diff(ctx.row_ptr).max()) if ctx_cap is None else ctx_cap
    e.score_candidates_device(ctx.n_rows, p[0], p[1], p[2], p[3], p[4], cand.n_rows, p[5], p[6], p[7], p[8],
                              int(ctx.row_ptr[-1]), int(cand.row_ptr[-1]), cap, prob, out.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return out.cpu().numpy()[:cand.n_rows], err


# ---- 4. too long ---------------------------------------------------------------------------------------------

def too_long_case():
    """Three requests: contexts of 5, 100 and 17; the second's middle candidate makes a row of 129."""
    rng = np.random.default_rng(21)
    ctx = to_block([entries(rng, 5), entries(rng, 100), entries(rng, 17)])
    cand = to_block([entries(rng, 3), entries(rng, 0), entries(rng, 28), entries(rng, 29), entries(rng, 2), entries(rng, 9),
                     entries(rng, 111)])
    return ctx, np.array([0, 2, 5, 7], np.int32), cand


def test_too_long_rows_and_contexts():
    k, fmt = 16, "f32"
    e, o = serving(k, fmt), oracle(k, fmt)
    ctx, rq, cand = too_long_case()
    # host: refused before anything is queued, out untouched, the next valid call is right
    out = np.full(cand.n_rows, -7.0, np.float32)
    rc, msg = raw_call(e, ctx, rq, cand, out)
    assert rc == fa.engine.E_CAPACITY and "max_row_nnz" in msg and (out == np.float32(-7.0)).all()
    e.sync()
    check(e, o, *take_requests(ctx, rq, cand, [0, 2]), "after a refused call")
    # device: the 129-entry row alone is NaN
    blk = fa.spell_out_candidates(ctx, rq, cand)
    fine = np.diff(blk.row_ptr) <= 128
    assert (~fine).sum() == 1 and not fine[3]
    for prob in (False, True):
        want = np.full(cand.n_rows, np.nan, np.float32)
        want[fine] = o.predict_batch(take_rows(blk, np.flatnonzero(fine)), output_prob=prob)[0]
        got, err = device_scores(e, ctx, rq, cand, prob)
        assert err is not None and err.code == fa.engine.E_CAPACITY, err
        assert_bitwise(got, want, "device call, one row too long, prob=%d" % prob)
        assert np.isnan(got[3]) and not np.isnan(np.delete(got, 3)).any()
    e.sync()  # (reported once)
    # device: a context beyond ctx_cap voids every candidate of its request, and nobody else's
    rq_ok = np.array([0, 2, 3, 5], np.int32)
    kept = take_rows(cand, [0, 1, 2, 4, 5])  # (without the long candidates: every row fits)
    cand_ok = Block(kept.row_ptr, kept.field, kept.feat, kept.val, kept.label)
    for prob in (False, True):
        want = o.predict_batch(fa.spell_out_candidates(ctx, rq_ok, cand_ok), output_prob=prob)[0].copy()
        want[2] = np.nan
        got, err = device_scores(e, ctx, rq_ok, cand_ok, prob, ctx_cap=17)
        assert err is not None and err.code == fa.engine.E_CAPACITY, err
        assert_bitwise(got, want, "device call, one context beyond ctx_cap, prob=%d" % prob)
        assert np.isnan(got[2]) and not np.isnan(np.delete(got, 2)).any()
    got, err = device_scores(e, ctx, rq_ok, cand_ok, False)
    assert err is None
    assert_bitwise(got, e.score_candidates(ctx, rq_ok, cand_ok), "the same call with the true ctx_cap")
    e.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_model_unchanged():
    k, fmt = 16, "f16"
    st = weights(k)
    e = serving(k, fmt)
    ctx, rq, cand = take_requests(*ladder(), [1, 2, 3, 4, 5])
    assert cand.n_rows > 4
    out = np.full(cand.n_rows, -7.0, np.float32)
    t = fa.Engine("FFM", NF, F, k, skip_init=True, max_batch_rows=MAX_ROWS, **STRESS_HP)
    rc, msg = raw_call(t, ctx, rq, cand, out)
    assert rc == fa.engine.E_UNSUPPORTED and "ffm_engine_pack_weights" in msg
    rc = t.lib.ffm_engine_score_candidates_device(t.h, 1, None, None, None, None, None, 1, None, None, None, None, 0, 0, 0, 0, None)
    assert rc == fa.engine.E_UNSUPPORTED
    t.close()
    for name in ("ctx_ptr", "ctx_field", "ctx_feat", "cand_req_ptr", "cand_ptr", "cand_field", "cand_feat", "out"):
        rc, msg = raw_call(e, ctx, rq, cand, out, null=(name,))
        assert rc == fa.engine.E_INVALID, (name, rc, msg)
    down = Block(cand.row_ptr.copy(), cand.field, cand.feat, cand.val, cand.label)
    down.row_ptr[2] = down.row_ptr[3] + 1
    assert raw_call(e, ctx, rq, down, out)[0] == fa.engine.E_INVALID
    off = Block(cand.row_ptr + 1, cand.field, cand.feat, cand.val, cand.label)
    assert raw_call(e, ctx, rq, off, out)[0] == fa.engine.E_INVALID
    bad_rq = rq.copy()
    bad_rq[-1] -= 1
    assert raw_call(e, ctx, bad_rq, cand, out)[0] == fa.engine.E_INVALID
    down_rq = rq.copy()
    down_rq[1] = rq[2] + 1
    assert raw_call(e, ctx, down_rq, cand, out)[0] == fa.engine.E_INVALID
    rc, msg = raw_call(e, ctx, rq, cand, out, n_cand=MAX_ROWS + 1)
    assert rc == fa.engine.E_CAPACITY, msg
    assert raw_call(e, ctx, rq, cand, out, n_req=0)[0] == 0
    assert raw_call(e, ctx, rq, cand, out, n_req=0, n_cand=0, null=("ctx_ptr", "cand_ptr", "cand_req_ptr", "out"))[0] == 0
    assert (out == np.float32(-7.0)).all()
    e.sync()
    got = e.get_weights()
    assert_bitwise(got["vec_w"], decoded(st["vec_w"], fmt), "the model after the refusals")
    assert_bitwise(got["lin_w"], st["lin_w"], "lin_w after the refusals")
    assert got["bias"][0] == st["bias3"][0]
    check(e, oracle(k, fmt), ctx, rq, cand, "after the refusals")
    e.close()


# ---- 6. hashed ids and missing values ------------------------------------------------------------------------

def test_hashed_ids_and_missing_values():
    k, fmt = 16, "f16"
    rng = np.random.default_rng(8)
    ctx, rq, cand = take_requests(*ladder(), [r for r in range(1, 12)])
    e = serving(k, fmt)
    fs = (np.arange(F + 1) * PER).astype(np.int32)
    h = serving(k, fmt, hash_ids=True, field_start=fs)

    def with_ids(b, raw):
        return Block(b.row_ptr, b.field, raw, b.val, b.label)
    raw_c = rng.integers(0, 2 ** 31 - 1, ctx.feat.size).astype(np.int32)
    raw_k = rng.integers(0, 2 ** 31 - 1, cand.feat.size).astype(np.int32)
    assert (raw_c >= NF).any() and (raw_k >= NF).any()
    hashed = (with_ids(ctx, fa.hash_ids(ctx.field, raw_c, NF, fs)), rq, with_ids(cand, fa.hash_ids(cand.field, raw_k, NF, fs)))
    for prob in (False, True):
        assert_bitwise(h.score_candidates(with_ids(ctx, raw_c), rq, with_ids(cand, raw_k), output_prob=prob),
                       e.score_candidates(*hashed, output_prob=prob), "hash_ids engine on raw ids")
    check(e, oracle(k, fmt), *hashed, "hashed ids")
    h.close()
    # val=None is numpy.ones, whatever the call before left in the staging arrays
    assert (ctx.val != 1).any() and (cand.val != 1).any()
    e.score_candidates(ctx, rq, cand)
    ones = (Block(ctx.row_ptr, ctx.field, ctx.feat, np.ones_like(ctx.val), ctx.label), rq,
            Block(cand.row_ptr, cand.field, cand.feat, np.ones_like(cand.val), cand.label))
    none = (Block(ctx.row_ptr, ctx.field, ctx.feat, None, ctx.label), rq, Block(cand.row_ptr, cand.field, cand.feat, None, cand.label))
    got = e.score_candidates(*none)
    e.score_candidates(ctx, rq, cand)
    assert_bitwise(got, e.score_candidates(*ones), "val=None vs numpy.ones")
    assert_bitwise(got, e.predict_batch(fa.spell_out_candidates(*none))[0], "val=None vs predict_batch")
    e.score_candidates(ctx, rq, cand)
    mixed = (none[0], rq, cand)
    assert_bitwise(e.score_candidates(*mixed), e.predict_batch(fa.spell_out_candidates(*mixed))[0], "ctx val=None alone")
    e.close()


# ---- 7. the device entry point -------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_device_entry_point_equals_the_host_entry_point(fmt):
    k = 16
    e = serving(k, fmt)
    ctx, rq, cand = ladder()
    want = ladder_reference(k, fmt)
    blk = fa.spell_out_candidates(ctx, rq, cand)
    for prob in (False, True):
        got, err = device_scores(e, ctx, rq, cand, prob)
        assert err is None, err
        assert_rows_bitwise(got, e.score_candidates(ctx, rq, cand, output_prob=prob), blk, "device vs host entry point")
        assert_rows_bitwise(got, want[int(prob)], blk, "device entry point vs the oracle")
    e.close()
