"""Per-request item lists on the device (include/ffm_engine.h "Scoring a catalogue: per-request item lists";
csrc/kernels_catalog_lists.h): every entry against score_items_reference in float64 plus predict_batch(ctx) as base,
under the header's bound (N + 32) * 2^-24 * (|base| + scale), N = m L + m + m (m - 1) / 2 k; a score's bits as a function
of (request, item) alone; the device entry point; probabilities; a context too long; the refusals.  The tables are the
engines' seeded init.  A workgroup takes 64 list positions per pass and owns 128."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

PER, N_ITEMS = 70, 40  # ids per field; items of the table
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 5)  # around a pass (64) and a workgroup's segment (128); longer than the table: repeats
CASES = [(fmt, F, k, m) for fmt in ("f32", "f16") for F, k in ((3, 4), (3, 64), (39, 16)) for m in ((1, 3, 8) if F == 39 else (1, 3))]


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


def table(F, m):
    """Slots in the last, the first and then the middle fields, mixed values; item 2's first slot is n_feats and item 3's
    last slot -1 (erased)."""
    rng = np.random.default_rng(7 + m)
    fld = np.array(([F - 1, 0] + list(range(1, F - 1)))[:m], np.int32)
    feat = np.stack([fld[a] * PER + rng.integers(PER, size=N_ITEMS) for a in range(m)], axis=1).astype(np.int32)
    feat[2, 0], feat[3, m - 1] = F * PER, -1
    return fld, feat, np.array([1.0, -0.75, 0.5, 1.25, -1.5, 0.25, 2.0, -0.5][:m], np.float32)


def lists(seed, lengths=LENGTHS):
    """(list_ptr, list_item): items drawn with repeats inside and across lists; the first entry of the 65-long list
    lies outside the table (N_ITEMS)."""
    rng = np.random.default_rng(seed)
    ptr = np.cumsum((0,) + tuple(lengths)).astype(np.int32)
    item = rng.integers(N_ITEMS, size=int(ptr[-1])).astype(np.int32)
    item[ptr[lengths.index(65)]] = N_ITEMS
    return ptr, item


def reference(e, F, ctx, fld, feat, val):
    """base + ref64 and the scale, [n_req, N_ITEMS + 1]: the last column is an item whose slots are all erased."""
    ext = np.concatenate([feat, np.full((1, feat.shape[1]), -1, np.int32)])
    ref, scale = fa.score_items_reference(e.get_weights(), ctx, fld, ext, val, n_fields=F)
    base = e.predict_batch(ctx, with_loss=False)[0].astype(np.float64)[:, None]
    return base + ref, np.abs(base) + scale


@pytest.mark.parametrize("fmt,F,k,m", CASES)
def test_contract(fmt, F, k, m):
    e = engine(fmt, F, k)
    ctx, (fld, feat, val), (ptr, item) = contexts(F, len(LENGTHS)), table(F, m), lists(1)
    want, mag = reference(e, F, ctx, fld, feat, val)
    got = e.score_item_lists(ctx, fld, feat, ptr, item, val)
    assert got.shape == (ptr[-1],) and got.dtype == np.float32
    req = np.repeat(np.arange(len(LENGTHS)), np.diff(ptr))
    N = m * e.row_len + m + m * (m - 1) // 2 * k
    err, bound = np.abs(got - want[req, item]), (N + 32) * 2.0 ** -24 * mag[req, item]
    print(fmt, F, k, m, "worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    e.close()


def device_call(e, ctx, fld, feat, val, ptr, item):
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ctx.row_ptr, ctx.field, ctx.feat, ctx.val, feat, ptr, item)]
    out = torch.full((int(ptr[-1]),), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in d]
    e.score_item_lists_device(ctx.n_rows, *p[:4], fld, p[4], val, feat.shape[0], p[5], p[6], int(ctx.row_ptr[-1]),
                              int(np.diff(ctx.row_ptr).max()), int(ptr[-1]), int(np.diff(ptr).max()), False, out.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return out.cpu().numpy(), err


@pytest.mark.parametrize("fmt", ("f32", "f16"))
def test_bits_depend_on_request_and_item_alone(fmt):
    F, k, m, n_req = 39, 16, 3, len(LENGTHS)
    e = engine(fmt, F, k)
    ctx, (fld, feat, val), (ptr, item) = contexts(F, n_req), table(F, m), lists(1)
    got = e.score_item_lists(ctx, fld, feat, ptr, item, val)
    ptr2, item2 = lists(2, LENGTHS[::-1])  # other lengths per request, other items around them
    got2 = e.score_item_lists(ctx, fld, feat, ptr2, item2, val)
    key = np.concatenate([np.repeat(np.arange(n_req), np.diff(ptr)) * 64 + item, np.repeat(np.arange(n_req), np.diff(ptr2)) * 64 + item2])
    bits = np.concatenate([got, got2]).view(np.uint32)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    assert same.sum() > 200 and (bits[order][1:][same] == bits[order][:-1][same]).all(), "one (request, item), one score"
    dev, err = device_call(e, ctx, fld, feat, val, ptr, item)
    assert err is None and np.array_equal(dev.view(np.uint32), bits[:len(got)]), "device vs host entry point"
    prob, sig = e.score_item_lists(ctx, fld, feat, ptr, item, val, output_prob=True), e.eval_sigmoid(got)
    assert (np.abs(prob - sig) <= np.spacing(sig)).all(), "probabilities are the sigmoid of the logits"
    bad, err = device_call(e, contexts(F, n_req, long_at=4), fld, feat, val, ptr, item)
    assert err is not None and err.code == fa.engine.E_CAPACITY, err
    mine = np.repeat(np.arange(n_req), np.diff(ptr)) == 4
    assert np.isnan(bad[mine]).all() and np.array_equal(bad[~mine].view(np.uint32), got[~mine].view(np.uint32))
    e.close()


F0, K0 = 3, 4
RANGES = (np.arange(F0 + 1) * PER).astype(np.int32)
REFUSALS = {  # name: (engine arguments, set a mask, item fields, list_ptr, code, what the message names)
    "training": (dict(serve=None), False, (0, 2), (0, 3, 8), fa.engine.E_UNSUPPORTED, "ffm_engine_pack_weights"),
    "f8": (dict(serve="f8"), False, (0, 2), (0, 3, 8), fa.engine.E_UNSUPPORTED, "FFM_FLAG_SERVE_F8"),
    "pruned": (dict(serve="f16", field_start=RANGES, prune=fa.pair_mask(F0, [(0, 1), (1, 2)])), False, (0, 2), (0, 3, 8),
               fa.engine.E_UNSUPPORTED, "pruned"),
    "mask": (dict(serve="f16"), True, (0, 2), (0, 3, 8), fa.engine.E_INVALID, "pair mask"),
    "normalised": (dict(serve="f32", normalize=True), False, (0, 2), (0, 3, 8), fa.engine.E_INVALID, "FFM_FLAG_NORM_ROWS"),
    "no slot": (dict(serve="f32"), False, (), (0, 3, 8), fa.engine.E_INVALID, "item_field"),
    "nine slots": (dict(serve="f32"), False, (0, 1, 2, 0, 1, 2, 0, 1, 2), (0, 3, 8), fa.engine.E_INVALID, "item_field"),
    "field named twice": (dict(serve="f32"), False, (2, 0, 2), (0, 3, 8), fa.engine.E_INVALID, "item_field"),
    "descending list_ptr": (dict(serve="f32"), False, (0, 2), (0, 8, 3), fa.engine.E_INVALID, "list_ptr"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_leave_the_model(name):
    kw, mask, fields, lptr, code, word = REFUSALS[name]
    e = fa.Engine("FFM", F0 * PER, F0, K0, max_batch_rows=256, **kw)
    if mask:
        e.set_pair_mask([(0, 1), (1, 2), (0, 0)])
    before = e.get_weights()
    out = np.full(8, -7.0, np.float32)
    _, cp, cfld, cft, cv, _ = e._csr(contexts(F0, 2))
    arrays = [np.array(fields, np.int32), np.zeros((8, max(len(fields), 1)), np.int32), np.array(lptr, np.int32), np.zeros(8, np.int32)]
    fld, feat, ptr, item = [a.ctypes.data_as(fa.engine._i32p) for a in arrays]
    rc = e.lib.ffm_engine_score_item_lists(e.h, 2, cp, cfld, cft, cv, len(fields), fld, feat, None, 8, ptr, item, 0,
                                           out.ctypes.data_as(fa.engine._f32p))
    msg = e.lib.ffm_engine_last_error().decode()
    assert rc == code and word in msg and ("list" in msg or "item_field" in msg), (rc, msg)
    e.sync()
    after = e.get_weights()
    assert (out == np.float32(-7.0)).all()
    for key in before:
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    e.close()
