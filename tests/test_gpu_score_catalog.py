"""Scoring a catalogue on the device (include/ffm_engine.h "Scoring a catalogue"; csrc/kernels_catalog.h): the MFMA
path against score_catalog_reference in float64 plus predict_batch(ctx) as base, under the header's bound
(L + 32) * 2^-24 * (|base| + scale).  The tables are the engines' seeded init."""
import itertools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

PER = 70  # ids per field
SHAPES = ((3, 4), (3, 64), (39, 16))  # L = 12 (under one chunk), 192, 624
FORMATS = ("f32", "f16")


def engine(fmt, F, k, **kw):
    return fa.Engine("FFM", F * PER, F, k, serve=fmt, max_batch_rows=256, **kw)


def contexts(F, n_req, ones=False, long_at=None):
    """Rows of six kinds in turn: entries of the first and the last field (the candidates' own); two entries of one
    field; an erased id; an erased field; one entry per field; empty.  long_at: that row has 129 entries instead."""
    rng = np.random.default_rng(100 + n_req)
    nf, mid = F * PER, F // 2

    def ent(f, i=None):
        return (f, f * PER + int(rng.integers(PER)) if i is None else i, float(np.float32(rng.uniform(-1.5, 1.5))))
    kinds = [lambda: [ent(0), ent(F - 1), ent(mid)], lambda: [ent(mid), ent(0), ent(mid)], lambda: [ent(0), ent(1, nf), ent(F - 1)],
             lambda: [ent(F, 3), ent(mid)], lambda: [ent(f) for f in range(F)], lambda: []]
    rows = [kinds[r % 6]() for r in range(n_req)]
    if long_at is not None:  # (the other rows stay what they are without it)
        rows[long_at] = [(p % F, (p % F) * PER + p % PER, 0.5) for p in range(129)]
    flat = [e for r in rows for e in r]
    return Block(np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([e[0] for e in flat], np.int32),
                 np.array([e[1] for e in flat], np.int32), None if ones else np.array([e[2] for e in flat], np.float32),
                 np.zeros(n_req, np.int32))


def check_contract(e, w, F, ctx, g, first, count, val):
    L = e.row_len
    base = e.predict_batch(ctx, with_loss=False)[0].astype(np.float64)[:, None]
    dot, scale = fa.score_catalog_reference(w, ctx, g, first, count, val, n_fields=F)
    got = e.score_catalog(ctx, g, first, count, val)
    assert got.shape == (ctx.n_rows, count) and got.dtype == np.float32
    err, bound = np.abs(got - (base + dot)), (L + 32) * 2.0 ** -24 * (np.abs(base) + scale)
    assert (err <= bound).all(), (g, first, count, val, float((err / np.maximum(bound, 1e-300)).max()))
    return got


@pytest.mark.parametrize("F,k", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_contract_zero_value_probabilities(fmt, F, k):
    e = engine(fmt, F, k)
    w = e.get_weights()
    reqs = (1, 33, 129) if (F, k) == (3, 4) else (1, 33)
    for n_req, (count, first), g, val in itertools.product(reqs, ((1, 69), (31, 37), (130, 3)), (0, F - 1), (1.0, -0.75)):
        ctx = contexts(F, n_req, ones=(count == 31 and val == 1.0))  # (val=None: ones, written on the device)
        got = check_contract(e, w, F, ctx, g, first + g * PER if count < PER else first, count, val)
        if val == 1.0 and g == 0:
            args = (ctx, g, first, count)
            base = e.predict_batch(ctx, with_loss=False)[0]
            assert np.array_equal(e.score_catalog(*args, 0.0), np.repeat(base[:, None], count, axis=1)), "val = 0 is predict_batch(ctx)"
            prob, want = e.score_catalog(*args, val, output_prob=True), e.eval_sigmoid(got.ravel()).reshape(got.shape)
            assert (np.abs(prob - want) <= np.spacing(want)).all(), "probabilities are the sigmoid of the logits"
    e.close()


def device_call(e, ctx, g, first, count, val, prob=False):
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ctx.row_ptr, ctx.field, ctx.feat, ctx.val)]
    out = torch.full((ctx.n_rows, count), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.score_catalog_device(ctx.n_rows, *[t.data_ptr() for t in d], g, first, count, val, int(ctx.row_ptr[-1]),
                           int(np.diff(ctx.row_ptr).max()), prob, out.data_ptr())
    err = None
    try:
        e.sync()
    except fa.EngineError as ex:
        err = ex
    return out.cpu().numpy(), err


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_entry_point_and_a_context_too_long(fmt):
    F, k = 3, 64
    e = engine(fmt, F, k)
    ctx = contexts(F, 33)
    for prob in (False, True):
        got, err = device_call(e, ctx, F - 1, 2 * PER + 3, 40, -0.75, prob)
        assert err is None, err
        want = e.score_catalog(ctx, F - 1, 2 * PER + 3, 40, -0.75, output_prob=prob)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "device vs host entry point"
    long_ctx = contexts(F, 33, long_at=7)
    got, err = device_call(e, long_ctx, 0, 5, 40, 1.0)
    assert err is not None and err.code == fa.engine.E_CAPACITY, err
    assert np.isnan(got[7]).all() and not np.isnan(np.delete(got, 7, axis=0)).any()
    fine, _ = device_call(e, ctx, 0, 5, 40, 1.0)
    keep = np.arange(33) != 7
    assert np.array_equal(got[keep].view(np.uint32), fine[keep].view(np.uint32))
    e.close()


F0, K0 = 3, 4
RANGES = (np.arange(F0 + 1) * PER).astype(np.int32)
REFUSALS = {  # name: (engine arguments, set a mask, (field, first, count), code, what the message names)
    "training": (dict(serve=None), False, (0, 0, 8), fa.engine.E_UNSUPPORTED, "ffm_engine_pack_weights"),
    "f8": (dict(serve="f8"), False, (0, 0, 8), fa.engine.E_UNSUPPORTED, "FFM_FLAG_SERVE_F8"),
    "pruned": (dict(serve="f16", field_start=RANGES, prune=fa.pair_mask(F0, [(0, 1), (1, 2)])), False, (0, 0, 8), fa.engine.E_UNSUPPORTED, "pruned"),
    "mask": (dict(serve="f16"), True, (0, 0, 8), fa.engine.E_INVALID, "pair mask"),
    "normalised": (dict(serve="f32", normalize=True), False, (0, 0, 8), fa.engine.E_INVALID, "FFM_FLAG_NORM_ROWS"),
    "field": (dict(serve="f32"), False, (F0, 0, 8), fa.engine.E_INVALID, "cand_field"),
    "range": (dict(serve="f32"), False, (0, F0 * PER - 7, 8), fa.engine.E_INVALID, "n_feats"),
    "count": (dict(serve="f32"), False, (0, 0, -1), fa.engine.E_INVALID, "negative"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_their_reason_and_leave_the_model(name):
    kw, mask, (g, first, count), code, word = REFUSALS[name]
    e = fa.Engine("FFM", F0 * PER, F0, K0, max_batch_rows=256, **kw)
    if mask:
        e.set_pair_mask([(0, 1), (1, 2), (0, 0)])
    before = e.get_weights()
    out = np.full((2, 8), -7.0, np.float32)
    ctx = contexts(F0, 2)
    _, cp, cfld, cft, cv, _ = e._csr(ctx)
    rc = e.lib.ffm_engine_score_catalog(e.h, 2, cp, cfld, cft, cv, g, first, count, 1.0, 0, out.ctypes.data_as(fa.engine._f32p))
    msg = e.lib.ffm_engine_last_error().decode()
    assert rc == code and word in msg, (rc, msg)
    assert e.lib.ffm_engine_score_catalog_device(e.h, 2, None, None, None, None, g, first, count, 1.0, 0, 0, 0, None) == code
    e.sync()
    after = e.get_weights()
    assert (out == np.float32(-7.0)).all()
    for key in before:
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    e.close()
