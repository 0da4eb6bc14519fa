"""The best K of a catalogue on the device (include/ffm_engine.h "Scoring a catalogue: the best K";
csrc/kernels_catalog_topk.h).  Expected is always catalog_topk_reference on score_catalog's matrix from the same engine
(that matrix is pinned to float64 by test_gpu_score_catalog.py): the ids and the scores' bits must be equal."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

FORMATS = ("f32", "f16")
NAN_BITS = 0x7FC00000


def engine(fmt, F, k, per, **kw):
    return fa.Engine("FFM", F * per, F, k, serve=fmt, max_batch_rows=256, **kw)


def contexts(F, per, n_req, long_at=None):
    """Rows of five kinds in turn: three fields; two entries of one field; an erased id; one entry per field; empty.
    long_at: that row has 129 entries instead."""
    rng = np.random.default_rng(100 + n_req)

    def ent(f, i=None):
        return (f, f * per + int(rng.integers(per)) if i is None else i, float(np.float32(rng.uniform(-1.5, 1.5))))
    kinds = [lambda: [ent(0), ent(F - 1), ent(F // 2)], lambda: [ent(F // 2), ent(0), ent(F // 2)],
             lambda: [ent(0), ent(1, F * per), ent(F - 1)], lambda: [ent(f) for f in range(F)], lambda: []]
    rows = [kinds[r % 5]() for r in range(n_req)]
    if long_at is not None:
        rows[long_at] = [(p % F, (p % F) * per + p % per, 0.5) for p in range(129)]
    flat = [e for r in rows for e in r]
    return Block(np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([e[0] for e in flat], np.int32),
                 np.array([e[1] for e in flat], np.int32), np.array([e[2] for e in flat], np.float32), np.zeros(n_req, np.int32))


def same(got, want):
    (gs, gi), (ws, wi) = got, want
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == wi.shape == gs.shape
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:4]
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


def check(e, ctx, g, first, count, K, val=1.0):
    want = fa.catalog_topk_reference(e.score_catalog(ctx, g, first, count, val), first, K)
    same(e.score_catalog_topk(ctx, g, first, count, K, val), want)
    return want


@pytest.mark.parametrize("F,k,per", ((3, 4, 300), (39, 16, 70)))
@pytest.mark.parametrize("fmt", FORMATS)
def test_shapes_values_fill_and_probabilities(fmt, F, k, per):
    e = engine(fmt, F, k, per)
    for n_req, count, K in ((1, 1, 1), (33, 31, 8), (33, 31, 64), (33, 130, 64), (129, 200, 16), (129, 200, 1)):
        ctx = contexts(F, per, n_req)
        for val in (1.0, -0.75):
            ws, wi = check(e, ctx, F - 1, 5, count, K, val)
            assert (wi[:, min(K, count):] == -1).all() and (ws.view(np.uint32)[:, min(K, count):] == NAN_BITS).all()
    ps, pi = e.score_catalog_topk(ctx, F - 1, 5, 200, 16, -0.75, output_prob=True)
    ws, wi = e.score_catalog_topk(ctx, F - 1, 5, 200, 16, -0.75)
    assert np.array_equal(pi, wi) and np.array_equal(ps.view(np.uint32), e.eval_sigmoid(ws.ravel()).reshape(ws.shape).view(np.uint32))
    fs, fi = e.score_catalog_topk(ctx, 0, 7, 0, 4)  # no candidates: the fill alone
    assert (fi == -1).all() and (fs.view(np.uint32) == NAN_BITS).all()
    e.close()


@pytest.mark.parametrize("grid", (None, 1, 2))
@pytest.mark.parametrize("fmt", FORMATS)
def test_trips_of_a_forced_grid(fmt, grid, monkeypatch):
    """600 candidates are five slabs: a wave makes five trips on one workgroup, three and two on two, the last
    slab partly empty."""
    if grid:
        monkeypatch.setenv("FFM_GRID_CATALOG", str(grid))
    e = engine(fmt, 3, 4, 300)
    for n_req, K in ((33, 8), (129, 16), (40, 64)):
        check(e, contexts(3, 300, n_req), 1, 150, 600, K)
    e.close()


@pytest.mark.parametrize("grid", (None, 2))
@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_go_to_the_lower_id(fmt, grid, monkeypatch):
    """Rows and lin_w repeat with period 7: equal scores sit in different lanes, waves, workgroups and trips."""
    if grid:
        monkeypatch.setenv("FFM_GRID_CATALOG", str(grid))
    F, k, per = 3, 4, 300
    e = engine(fmt, F, k, per)
    rng = np.random.default_rng(7)
    rows, lin = rng.normal(0, 0.5, (7, F * k)).astype(np.float32), rng.normal(0, 0.5, 7).astype(np.float32)
    at = np.arange(F * per) % 7
    e.set_weights(bias=np.zeros(1, np.float32), lin_w=lin[at], vec_w=rows[at])
    ws, wi = check(e, contexts(F, per, 33), 0, 11, 300, 16)
    live = ~np.isnan(ws[:, 0])
    tied = ws.view(np.uint32)[:, 1:] == ws.view(np.uint32)[:, :-1]
    assert tied[live].any(axis=1).all(), "every request has equal scores inside its top 16"
    assert (np.diff(wi, axis=1)[tied] > 0).all(), "... in ascending id order"
    e.close()


def device_call(e, ctx, g, first, count, K, val=1.0, prob=False):
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ctx.row_ptr, ctx.field, ctx.feat, ctx.val)]
    score = torch.full((ctx.n_rows, K), -7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((ctx.n_rows, K), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.score_catalog_topk_device(ctx.n_rows, *[t.data_ptr() for t in d], g, first, count, val, K, int(ctx.row_ptr[-1]),
                                int(np.diff(ctx.row_ptr).max()), prob, score.data_ptr(), ids.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return (score.cpu().numpy(), ids.cpu().numpy()), err


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_entry_point_and_a_flagged_request(fmt):
    F, k, per = 3, 4, 300
    e = engine(fmt, F, k, per)
    ctx = contexts(F, per, 33)
    for prob in (False, True):
        got, err = device_call(e, ctx, 2, 603, 200, 16, -0.75, prob)
        assert err is None, err
        same(got, e.score_catalog_topk(ctx, 2, 603, 200, 16, -0.75, output_prob=prob))
    fine = e.score_catalog_topk(ctx, 0, 5, 200, 8)
    long_ctx = contexts(F, per, 33, long_at=7)
    (gs, gi), err = device_call(e, long_ctx, 0, 5, 200, 8)
    assert err is not None and err.code == fa.engine.E_CAPACITY, err
    assert (gi[7] == -1).all() and (gs.view(np.uint32)[7] == NAN_BITS).all()
    keep = np.arange(33) != 7
    same((gs[keep], gi[keep]), (fine[0][keep], fine[1][keep]))
    with pytest.raises(fa.EngineError) as ei:
        e.score_catalog_topk(long_ctx, 0, 5, 200, 8)
    assert ei.value.code == fa.engine.E_CAPACITY
    e.close()


def test_past_the_matrix_calls_cap():
    """256 requests x 8 388 609 candidates is 2^31 + 256 scores: score_catalog refuses it; the selection does not."""
    F, k, n_cand, K = 3, 4, (1 << 23) + 1, 8
    e = fa.Engine("FFM", n_cand + 9, F, k, serve="f16", max_batch_rows=256)
    ctx = contexts(F, 1000, 256)
    _, cp, cfld, cft, cv, _ = e._csr(ctx)
    assert e.lib.ffm_engine_score_catalog(e.h, 256, cp, cfld, cft, cv, 1, 3, n_cand, 1.0, 0, None) == fa.engine.E_CAPACITY
    gs, gi = e.score_catalog_topk(ctx, 1, 3, n_cand, K)
    for r in (3, 255):
        one = Block(ctx.row_ptr[r:r + 2] - ctx.row_ptr[r], *[a[ctx.row_ptr[r]:ctx.row_ptr[r + 1]] for a in (ctx.field, ctx.feat, ctx.val)],
                    np.zeros(1, np.int32))
        same((gs[r:r + 1], gi[r:r + 1]), fa.catalog_topk_reference(e.score_catalog(one, 1, 3, n_cand), 3, K))
    e.close()


REFUSALS = {  # name: (engine arguments, top_k, code, what the message names)
    "zero": (dict(serve="f32"), 0, fa.engine.E_INVALID, "top_k"),
    "above": (dict(serve="f16"), 65, fa.engine.E_INVALID, "top_k"),
    "training": (dict(serve=None), 8, fa.engine.E_UNSUPPORTED, "ffm_engine_pack_weights"),
    "f8": (dict(serve="f8"), 8, fa.engine.E_UNSUPPORTED, "FFM_FLAG_SERVE_F8"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_write_nothing(name):
    kw, K, code, word = REFUSALS[name]
    e = fa.Engine("FFM", 900, 3, 4, max_batch_rows=256, **kw)
    score, ids = np.full((2, 64), -7.0, np.float32), np.full((2, 64), -7, np.int32)
    _, cp, cfld, cft, cv, _ = e._csr(contexts(3, 300, 2))
    rc = e.lib.ffm_engine_score_catalog_topk(e.h, 2, cp, cfld, cft, cv, 0, 0, 8, 1.0, K, 0, score.ctypes.data_as(fa.engine._f32p),
                                             ids.ctypes.data_as(fa.engine._i32p))
    msg = e.lib.ffm_engine_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert e.lib.ffm_engine_score_catalog_topk_device(e.h, 2, None, None, None, None, 0, 0, 8, 1.0, K, 0, 0, 0, None, None) == code
    e.sync()
    assert (score == np.float32(-7.0)).all() and (ids == -7).all()
    e.close()
