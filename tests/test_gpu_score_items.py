"""Scoring items of several entries on the device (include/ffm_engine.h "Scoring a catalogue: items of several
entries"; csrc/kernels_catalog_items.h): the gathered MFMA path against score_items_reference in float64 plus
predict_batch(ctx) as base, under the header's bound (N + 32) * 2^-24 * (|base| + scale), N = m L + m + m (m - 1) / 2 k;
the best K against catalog_topk_reference on the matrix; the device entry points; the refusals.  The tables are the
engines' seeded init."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

PER = 70  # ids per field
SHAPES = ((4, 4, 1), (4, 4, 3), (4, 64, 2), (39, 16, 4))  # (F, k, m)
FORMATS = ("f32", "f16")


def engine(fmt, F, k, **kw):
    return fa.Engine("FFM", F * PER, F, k, serve=fmt, max_batch_rows=256, **kw)


def contexts(F, n_req, ones=False, long_at=None):
    """Rows of six kinds in turn: entries of the first and the last field (item fields); two entries of one field; an
    erased id; an erased field; one entry per field; empty.  long_at: that row has 129 entries instead."""
    rng = np.random.default_rng(100 + n_req)
    nf, mid = F * PER, F // 2

    def ent(f, i=None):
        return (f, f * PER + int(rng.integers(PER)) if i is None else i, float(np.float32(rng.uniform(-1.5, 1.5))))
    kinds = [lambda: [ent(0), ent(F - 1), ent(mid)], lambda: [ent(mid), ent(0), ent(mid)], lambda: [ent(0), ent(1, nf), ent(F - 1)],
             lambda: [ent(F, 3), ent(mid)], lambda: [ent(f) for f in range(F)], lambda: []]
    rows = [kinds[r % 6]() for r in range(n_req)]
    if long_at is not None:
        rows[long_at] = [(p % F, (p % F) * PER + p % PER, 0.5) for p in range(129)]
    flat = [e for r in rows for e in r]
    return Block(np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([e[0] for e in flat], np.int32),
                 np.array([e[1] for e in flat], np.int32), None if ones else np.array([e[2] for e in flat], np.float32),
                 np.zeros(n_req, np.int32))


def table(F, m, n_items, mixed=True):
    """Slots in the last, the first and then the middle fields; ids drawn from 1, 7, 3, ... per slot, so they repeat
    across items; every fifth item has a slot of -1 and (m > 1) every seventh one of n_feats."""
    rng = np.random.default_rng(7 * n_items + m)
    fld = np.array(([F - 1, 0] + list(range(1, F - 1)))[:m], np.int32)
    feat = np.stack([fld[a] * PER + rng.integers((PER, 7, 3, 2)[a % 4], size=n_items) for a in range(m)], axis=1).astype(np.int32)
    feat[::5, 0] = -1
    if m > 1:
        feat[::7, m - 1] = F * PER
    val = np.array([1.0, -0.75, 0.5, 1.25, -1.0, 2.0, 0.25, -0.5][:m], np.float32) if mixed else None
    return fld, feat, val


@pytest.mark.parametrize("F,k,m", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_contract_and_probabilities(fmt, F, k, m):
    e = engine(fmt, F, k)
    w, L = e.get_weights(), e.row_len
    N = m * L + m + m * (m - 1) // 2 * k
    for n_req in ((1, 33, 129) if (F, k, m) == (4, 4, 1) else (1, 33)):
        for n_items in (1, 33, 130):
            mixed = n_items != 33
            ctx = contexts(F, n_req, ones=not mixed)  # (val=None: ones, written on the device)
            fld, feat, val = table(F, m, n_items, mixed)
            base = e.predict_batch(ctx, with_loss=False)[0].astype(np.float64)[:, None]
            ref, scale = fa.score_items_reference(w, ctx, fld, feat, val, n_fields=F)
            got = e.score_items(ctx, fld, feat, val)
            assert got.shape == (n_req, n_items) and got.dtype == np.float32
            err, bound = np.abs(got - (base + ref)), (N + 32) * 2.0 ** -24 * (np.abs(base) + scale)
            print(fmt, F, k, m, n_req, n_items, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (n_req, n_items, float((err / np.maximum(bound, 1e-300)).max()))
            if n_req == 33:
                prob, want = e.score_items(ctx, fld, feat, val, output_prob=True), e.eval_sigmoid(got.ravel()).reshape(got.shape)
                assert (np.abs(prob - want) <= np.spacing(want)).all(), "probabilities are the sigmoid of the logits"
    e.close()


@pytest.mark.parametrize("n_items", (5, 130))
@pytest.mark.parametrize("fmt", FORMATS)
def test_topk_is_the_reference_on_the_matrix(fmt, n_items):
    F, k, m = 4, 64, 2
    e = engine(fmt, F, k)
    ctx = contexts(F, 33)
    fld, feat, val = table(F, m, n_items)
    full = e.score_items(ctx, fld, feat, val)
    for K in (1, 8, 64):
        want_s, want_i = fa.catalog_topk_reference(full, 0, K)
        got_s, got_i = e.score_items_topk(ctx, fld, feat, K, val)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), K
    e.close()


def device_calls(e, ctx, fld, feat, val, K):
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ctx.row_ptr, ctx.field, ctx.feat, ctx.val, feat)]
    n_req, n_items = ctx.n_rows, feat.shape[0]
    out = torch.full((n_req, n_items), -7.0, dtype=torch.float32, device="cuda")
    ts = torch.full((n_req, K), -7.0, dtype=torch.float32, device="cuda")
    ti = torch.full((n_req, K), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr, nnz, cap = [t.data_ptr() for t in d], int(ctx.row_ptr[-1]), int(np.diff(ctx.row_ptr).max())
    e.score_items_device(n_req, *ptr[:4], fld, ptr[4], val, n_items, nnz, cap, False, out.data_ptr())
    e.score_items_topk_device(n_req, *ptr[:4], fld, ptr[4], val, n_items, K, nnz, cap, False, ts.data_ptr(), ti.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return out.cpu().numpy(), ts.cpu().numpy(), ti.cpu().numpy(), err


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_entry_points_and_a_context_too_long(fmt):
    F, k, m, K = 4, 4, 3, 8
    e = engine(fmt, F, k)
    ctx = contexts(F, 33)
    fld, feat, val = table(F, m, 40)
    got, ts, ti, err = device_calls(e, ctx, fld, feat, val, K)
    assert err is None, err
    want = e.score_items(ctx, fld, feat, val)
    ws, wi = e.score_items_topk(ctx, fld, feat, K, val)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "device vs host entry point"
    assert np.array_equal(ti, wi) and np.array_equal(ts.view(np.uint32), ws.view(np.uint32))
    bad, bs, bi, err = device_calls(e, contexts(F, 33, long_at=7), fld, feat, val, K)
    assert err is not None and err.code == fa.engine.E_CAPACITY, err
    keep = np.arange(33) != 7
    assert np.isnan(bad[7]).all() and (bi[7] == -1).all() and np.isnan(bs[7]).all()
    assert np.array_equal(bad[keep].view(np.uint32), got[keep].view(np.uint32))
    assert np.array_equal(bi[keep], ti[keep]) and np.array_equal(bs[keep].view(np.uint32), ts[keep].view(np.uint32))
    e.close()


F0, K0 = 3, 4
RANGES = (np.arange(F0 + 1) * PER).astype(np.int32)
REFUSALS = {  # name: (engine arguments, set a mask, item_field, code, what the message names)
    "training": (dict(serve=None), False, (0, 2), fa.engine.E_UNSUPPORTED, "ffm_engine_pack_weights"),
    "f8": (dict(serve="f8"), False, (0, 2), fa.engine.E_UNSUPPORTED, "FFM_FLAG_SERVE_F8"),
    "pruned": (dict(serve="f16", field_start=RANGES, prune=fa.pair_mask(F0, [(0, 1), (1, 2)])), False, (0, 2), fa.engine.E_UNSUPPORTED, "pruned"),
    "mask": (dict(serve="f16"), True, (0, 2), fa.engine.E_INVALID, "pair mask"),
    "normalised": (dict(serve="f32", normalize=True), False, (0, 2), fa.engine.E_INVALID, "FFM_FLAG_NORM_ROWS"),
    "no slots": (dict(serve="f32"), False, (), fa.engine.E_INVALID, "item_field"),
    "nine slots": (dict(serve="f32"), False, (0, 1, 2, 0, 1, 2, 0, 1, 2), fa.engine.E_INVALID, "item_field"),
    "repeated field": (dict(serve="f32"), False, (2, 0, 2), fa.engine.E_INVALID, "item_field"),
    "field": (dict(serve="f32"), False, (0, F0), fa.engine.E_INVALID, "item_field"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_leave_the_model(name):
    kw, mask, fields, code, word = REFUSALS[name]
    e = fa.Engine("FFM", F0 * PER, F0, K0, max_batch_rows=256, **kw)
    if mask:
        e.set_pair_mask([(0, 1), (1, 2), (0, 0)])
    before = e.get_weights()
    out = np.full((2, 8), -7.0, np.float32)
    ctx = contexts(F0, 2)
    _, cp, cfld, cft, cv, _ = e._csr(ctx)
    fld = np.array(fields + (0,), np.int32)  # (never empty: n_slots says how many count)
    feat = np.zeros((8, max(len(fields), 1)), np.int32)
    i32, f32 = fa.engine._i32p, fa.engine._f32p
    rc = e.lib.ffm_engine_score_items(e.h, 2, cp, cfld, cft, cv, len(fields), fld.ctypes.data_as(i32), feat.ctypes.data_as(i32), None, 8,
                                      0, out.ctypes.data_as(f32))
    msg = e.lib.ffm_engine_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert e.lib.ffm_engine_score_items_topk_device(e.h, 2, None, None, None, None, len(fields), fld.ctypes.data_as(i32), None, None, 8, 4,
                                                    0, 0, 0, None, None) == code
    e.sync()
    after = e.get_weights()
    assert (out == np.float32(-7.0)).all()
    for key in before:
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    e.close()
