"""Scoring items with dictionary slots on the device (include/ffm_engine.h "Scoring a catalogue: dictionary slots";
csrc/kernels_catalog_dict.h): the factorised path against score_items_reference on expand_items(...) in float64 plus
predict_batch(ctx) as base, under the header's bound (N + 32) * 2^-24 * (|base| + scale), N = m L + m + m (m - 1) / 2 k,
m = n_gather + n_dict; the best K against catalog_topk_reference on the matrix; the device entry points; the refusals.
The tables are the engines' seeded init."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

PER = 70  # ids per field
SHAPES = ((4, 4, 1, 1), (4, 4, 1, 3), (4, 64, 2, 1), (39, 16, 1, 3))  # (F, k, n_gather, n_dict)
SIZES = (33, 1, 40)  # of the dictionaries: none a multiple of 32, so padding and a slot boundary fall inside a workgroup
FORMATS = ("f32", "f16")


def engine(fmt, F, k, **kw):
    return fa.Engine("FFM", F * PER, F, k, serve=fmt, max_batch_rows=256, **kw)


def contexts(F, n_req, long_at=None):
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
                 np.array([e[1] for e in flat], np.int32), np.array([e[2] for e in flat], np.float32), np.zeros(n_req, np.int32))


def table(F, n_gather, n_dict, n_items):
    """Slots in the last, the first and then the middle fields, mixed values.  Every fifth item has a code of -1 in the
    first dictionary slot, every seventh one of D in the last; one id of the first dictionary is n_feats; items 0 and 1
    are identical."""
    rng = np.random.default_rng(7 * n_items + n_gather)
    m = n_gather + n_dict
    fld = np.array(([F - 1, 0] + list(range(1, F - 1)))[:m], np.int32)
    feat = np.stack([fld[a] * PER + rng.integers(PER, size=n_items) for a in range(n_gather)], axis=1).astype(np.int32)
    dicts = [(fld[n_gather + a] * PER + rng.choice(PER, SIZES[a], replace=False)).astype(np.int32) for a in range(n_dict)]
    dicts[0][2] = F * PER
    code = np.stack([rng.integers(SIZES[a], size=n_items) for a in range(n_dict)], axis=1).astype(np.int32)
    code[::5, 0] = -1
    code[::7, n_dict - 1] = SIZES[n_dict - 1]
    if n_items > 1:
        feat[1], code[1] = feat[0], code[0]
    return fld, feat, code, dicts, np.array([1.0, -0.75, 0.5, 1.25][:m], np.float32)


@pytest.mark.parametrize("F,k,n_gather,n_dict", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_contract_and_probabilities(fmt, F, k, n_gather, n_dict):
    e = engine(fmt, F, k)
    w, L, m = e.get_weights(), e.row_len, n_gather + n_dict
    N = m * L + m + m * (m - 1) // 2 * k
    for n_req in ((1, 33, 129) if (F, k, n_gather, n_dict) == SHAPES[0] else (1, 33)):
        ctx = contexts(F, n_req)
        base = e.predict_batch(ctx, with_loss=False)[0].astype(np.float64)[:, None]
        for n_items in (1, 33, 130):
            fld, feat, code, dicts, val = table(F, n_gather, n_dict, n_items)
            ref, scale = fa.score_items_reference(w, ctx, fld, fa.expand_items(feat, code, dicts, F * PER), val, n_fields=F)
            got = e.score_items_dict(ctx, fld, feat, code, dicts, val)
            assert got.shape == (n_req, n_items) and got.dtype == np.float32
            err, bound = np.abs(got - (base + ref)), (N + 32) * 2.0 ** -24 * (np.abs(base) + scale)
            print(fmt, F, k, n_gather, n_dict, n_req, n_items, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (n_req, n_items, float((err / np.maximum(bound, 1e-300)).max()))
            if n_req == 33:
                prob = e.score_items_dict(ctx, fld, feat, code, dicts, val, output_prob=True)
                want = e.eval_sigmoid(got.ravel()).reshape(got.shape)
                assert (np.abs(prob - want) <= np.spacing(want)).all(), "probabilities are the sigmoid of the logits"
    e.close()


@pytest.mark.parametrize("n_items", (5, 130))
@pytest.mark.parametrize("fmt", FORMATS)
def test_topk_is_the_reference_on_the_matrix(fmt, n_items):
    F, k = 4, 64
    e = engine(fmt, F, k)
    ctx = contexts(F, 33)
    fld, feat, code, dicts, val = table(F, 1, 2, n_items)
    full = e.score_items_dict(ctx, fld, feat, code, dicts, val)
    assert np.array_equal(full[:, 0].view(np.uint32), full[:, 1].view(np.uint32)), "identical items score alike"
    for K in (1, 8, 64):
        want_s, want_i = fa.catalog_topk_reference(full, 0, K)
        got_s, got_i = e.score_items_dict_topk(ctx, fld, feat, code, dicts, K, val)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), K
    e.close()


def device_calls(e, ctx, fld, feat, code, dicts, val, K):
    ptr = np.cumsum([0] + [len(d) for d in dicts]).astype(np.int32)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ctx.row_ptr, ctx.field, ctx.feat, ctx.val, feat, code, np.concatenate(dicts))]
    n_req, n_items = ctx.n_rows, feat.shape[0]
    out = torch.full((n_req, n_items), -7.0, dtype=torch.float32, device="cuda")
    ts = torch.full((n_req, K), -7.0, dtype=torch.float32, device="cuda")
    ti = torch.full((n_req, K), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p, nnz, cap = [t.data_ptr() for t in d], int(ctx.row_ptr[-1]), int(np.diff(ctx.row_ptr).max())
    e.score_items_dict_device(n_req, *p[:4], feat.shape[1], fld, p[4], p[5], ptr, p[6], val, n_items, nnz, cap, False, out.data_ptr())
    e.score_items_dict_topk_device(n_req, *p[:4], feat.shape[1], fld, p[4], p[5], ptr, p[6], val, n_items, K, nnz, cap, False, ts.data_ptr(),
                                   ti.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return out.cpu().numpy(), ts.cpu().numpy(), ti.cpu().numpy(), err


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_entry_points_and_a_context_too_long(fmt):
    F, k, K = 4, 4, 8
    e = engine(fmt, F, k)
    ctx = contexts(F, 33)
    fld, feat, code, dicts, val = table(F, 1, 3, 40)
    got, ts, ti, err = device_calls(e, ctx, fld, feat, code, dicts, val, K)
    assert err is None, err
    want = e.score_items_dict(ctx, fld, feat, code, dicts, val)
    ws, wi = e.score_items_dict_topk(ctx, fld, feat, code, dicts, K, val)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "device vs host entry point"
    assert np.array_equal(ti, wi) and np.array_equal(ts.view(np.uint32), ws.view(np.uint32))
    bad, bs, bi, err = device_calls(e, contexts(F, 33, long_at=7), fld, feat, code, dicts, val, K)
    assert err is not None and err.code == fa.engine.E_CAPACITY, err
    keep = np.arange(33) != 7
    assert np.isnan(bad[7]).all() and (bi[7] == -1).all() and np.isnan(bs[7]).all()
    assert np.array_equal(bad[keep].view(np.uint32), got[keep].view(np.uint32))
    assert np.array_equal(bi[keep], ti[keep]) and np.array_equal(bs[keep].view(np.uint32), ts[keep].view(np.uint32))
    e.close()


F0, K0 = 3, 4
RANGES = (np.arange(F0 + 1) * PER).astype(np.int32)
OK = ((0,), (2,), (0, 2))  # gathered fields, dictionary fields, dict_ptr
REFUSALS = {  # name: (engine arguments, set a mask, (gathered fields, dictionary fields, dict_ptr), code, what the message names)
    "training": (dict(serve=None), False, OK, fa.engine.E_UNSUPPORTED, "ffm_engine_pack_weights"),
    "f8": (dict(serve="f8"), False, OK, fa.engine.E_UNSUPPORTED, "FFM_FLAG_SERVE_F8"),
    "pruned": (dict(serve="f16", field_start=RANGES, prune=fa.pair_mask(F0, [(0, 1), (1, 2)])), False, OK, fa.engine.E_UNSUPPORTED, "pruned"),
    "mask": (dict(serve="f16"), True, OK, fa.engine.E_INVALID, "pair mask"),
    "normalised": (dict(serve="f32", normalize=True), False, OK, fa.engine.E_INVALID, "FFM_FLAG_NORM_ROWS"),
    "no gathered slot": (dict(serve="f32"), False, ((), (2,), (0, 2)), fa.engine.E_INVALID, "n_gather"),
    "no dictionary slot": (dict(serve="f32"), False, ((0,), (), (0,)), fa.engine.E_INVALID, "n_dict"),
    "nine slots": (dict(serve="f32"), False, ((0, 1, 2, 0), (1, 2, 0, 1, 2), (0, 1, 2, 3, 4, 5)), fa.engine.E_INVALID, "item_field"),
    "field in both kinds": (dict(serve="f32"), False, ((2, 0), (2,), (0, 2)), fa.engine.E_INVALID, "item_field"),
    "decreasing dict_ptr": (dict(serve="f32"), False, ((0,), (1, 2), (0, 2, 1)), fa.engine.E_INVALID, "dict_ptr"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_leave_the_model(name):
    kw, mask, (gathered, coded, ptr), code, word = REFUSALS[name]
    e = fa.Engine("FFM", F0 * PER, F0, K0, max_batch_rows=256, **kw)
    if mask:
        e.set_pair_mask([(0, 1), (1, 2), (0, 0)])
    before = e.get_weights()
    out = np.full((2, 8), -7.0, np.float32)
    _, cp, cfld, cft, cv, _ = e._csr(contexts(F0, 2))
    i32, f32 = fa.engine._i32p, fa.engine._f32p
    arrays = [np.array(gathered + coded, np.int32), np.zeros((8, max(len(gathered), 1)), np.int32), np.zeros((8, max(len(coded), 1)), np.int32),
              np.array(ptr, np.int32), np.zeros(8, np.int32)]
    fld, feat, cod, dptr, dfeat = [a.ctypes.data_as(i32) for a in arrays]
    rc = e.lib.ffm_engine_score_items_dict(e.h, 2, cp, cfld, cft, cv, len(gathered), len(coded), fld, feat, cod, dptr, dfeat, None, 8, 0,
                                           out.ctypes.data_as(f32))
    msg = e.lib.ffm_engine_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert e.lib.ffm_engine_score_items_dict_topk_device(e.h, 2, None, None, None, None, len(gathered), len(coded), fld, None, None, dptr, None,
                                                         None, 8, 4, 0, 0, 0, None, None) == code
    e.sync()
    after = e.get_weights()
    assert (out == np.float32(-7.0)).all()
    for key in before:
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    e.close()
