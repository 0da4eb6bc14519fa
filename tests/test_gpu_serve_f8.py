"""`f8` serving engines (include/ffm_engine.h "Serving engines"; csrc/kernels_serve8.h): the encoder against numpy's
definition of the format (ftrl_ffm_amd.serve_f8_encode / _decode), and the row kernel against an fp32 serving engine
that holds the decoded table -- the same fp32 arithmetic in the same order, so every comparison is bit for bit (NaN
with NaN: util.assert_bitwise)."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import Csr
from test_serve_f8_host import edge_rows
from util import STRESS_HP, assert_bitwise, take_rows

pytestmark = pytest.mark.gpu
NF = 64


def engine(F, k, serve=None, **kw):
    return fa.Engine("FFM", NF, F, k, serve=serve, max_batch_rows=16, max_batch_nnz=4096, **dict(STRESS_HP, **kw))


def counted(w, d):
    nan = np.isnan(w)
    return dict(n_latent=w.size, n_inexact=int((~nan & (w.view(np.uint32) != d.view(np.uint32))).sum()),
                n_to_inf=int((np.isfinite(w) & ~np.isfinite(d)).sum()), n_to_zero=int((~nan & (w != 0) & (d == 0)).sum()))


@pytest.mark.parametrize("k", [4, 16, 64])
@pytest.mark.parametrize("F", [3, 39])
def test_encoder_is_the_numpy_definition(F, k):
    """pack_from, set_rows and the create-time contents; row lengths 12 .. 2496: both lane groups, rows that stay in
    registers and rows read twice, a last chunk with padding."""
    w = edge_rows(F * k, NF)
    want = fa.serve_f8_decode(*fa.serve_f8_encode(w), row_len=F * k)
    t = engine(F, k, skip_init=True)
    t.set_weights(bias=[0.25], lin_w=np.arange(NF, dtype=np.float32), vec_w=w)
    s = engine(F, k, "f8", skip_init=True)
    ids = np.arange(NF, dtype=np.int32)
    assert not s.get_rows(ids)["vec_w"].any() and s.model_bytes() == 4 + 4 * NF + NF * fa.serve_f8_stride(F * k)
    assert s.pack_from(t) == counted(w, want)
    got = s.get_weights()
    assert_bitwise(got["vec_w"], want, "pack_from")
    assert got["bias"][0] == 0.25 and np.array_equal(got["lin_w"], np.arange(NF))
    some = ids[::-3].copy()  # set_rows: whole rows, each scale from the values given
    s.set_rows(some, dict(vec_w=w[some][:, ::-1].copy()))
    want[some] = fa.serve_f8_decode(*fa.serve_f8_encode(w[some][:, ::-1]), row_len=F * k)
    assert_bitwise(s.get_rows(ids)["vec_w"], want, "set_rows")
    assert s.encode_stats() == counted(w[some][:, ::-1], want[some])
    fresh_t, fresh_s = engine(F, k, seed=9), engine(F, k, "f8", seed=9)
    draws = fresh_t.get_weights()["vec_w"]
    assert_bitwise(fresh_s.get_weights()["vec_w"], fa.serve_f8_decode(*fa.serve_f8_encode(draws), row_len=F * k), "create")
    for e in (t, s, fresh_t, fresh_s):
        e.close()


def block(F, lengths, seed):
    """Rows of the given lengths over ids -2 .. NF + 1 and fields -1 .. F: out of range both ways, fields twice."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    return Csr(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), rng.integers(-1, F + 1, n).astype(np.int32),
               rng.integers(-2, NF + 2, n).astype(np.int32), rng.standard_normal(n).astype(np.float32),
               rng.integers(0, 2, len(lengths)).astype(np.int32))


def pair(F, k):
    """An f8 engine of seeded rows (feature 5 holds the NaN byte) and the fp32 serving engine of its decoded table."""
    w = (np.random.default_rng(k * 100 + F).standard_normal((NF, F * k)) * 0.3).astype(np.float32)
    w[5, F * k // 2] = np.nan
    s8, s32 = engine(F, k, "f8", skip_init=True), engine(F, k, "f32", skip_init=True)
    s8.set_weights(bias=[0.1], lin_w=np.linspace(-1, 1, NF).astype(np.float32), vec_w=w)
    s32.set_weights(**s8.get_weights())
    return s8, s32


def on_device(e, b):
    d = {key: torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")}
    out = torch.full((b.n_rows,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.predict_batch_device(b.n_rows, int(b.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(), d["feat"].data_ptr(),
                           d["val"].data_ptr(), d["label"].data_ptr(), True, out.data_ptr(), None)
    try:
        e.sync()
    except fa.EngineError as err:
        return out.cpu().numpy(), err.code
    return out.cpu().numpy(), 0


@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("F", [3, 39, 64])
def test_rows_are_the_fp32_kernel_on_the_decoded_table(F, k):
    """The 129-entry row goes through predict_batch_device: predict_batch refuses it on the host (FFM_E_CAPACITY) before
    anything is queued, so only a device block reaches the kernel's own refusal."""
    s8, s32 = pair(F, k)
    blk = block(F, [0, 1, 2, 39, 64, 65, 128, 2], seed=F + k)
    blk.field[-2:], blk.feat[-2:] = [0, F // 2], [5, 6]  # the last row reads the slot that holds the NaN byte
    for prob in (False, True):
        a, b = s8.predict_batch(blk, output_prob=prob), s32.predict_batch(blk, output_prob=prob)
        assert_bitwise(a[0], b[0], "F=%d k=%d prob=%d" % (F, k, prob))
        assert a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1]))
    assert np.isnan(a[0][-1]) and np.isfinite(a[0][:3]).all()
    (o8, c8), (o32, c32) = (on_device(e, block(F, [5, 129, 2], seed=k)) for e in (s8, s32))
    assert c8 == c32 == fa.engine.E_CAPACITY and np.isnan(o8[1]) and np.isnan(o32[1])
    assert_bitwise(o8, o32, "beside a row of 129 entries")
    s8.close()
    s32.close()


def test_entry_points_give_predict_batch_bits():
    s8, s32 = pair(39, 16)
    blk = block(39, [7, 0, 128, 39, 40], seed=1)
    want = s8.predict_batch(blk, output_prob=True)[0]
    out, code = on_device(s8, blk)
    assert code == 0
    assert_bitwise(out, want, "predict_batch_device")
    buf = s8.score_buffer(blk.n_rows)
    cutter = fa.RowCutter(blk.n_rows, int(blk.row_ptr[-1]), n_blocks=2)
    cutter.take_host(blk.n_rows, blk.row_ptr, blk.field, blk.feat, blk.val, blk.label)
    res = cutter.close()
    for what, call in (("predict_batch_async", lambda: s8.predict_batch_async(blk, scores=buf, output_prob=True)),
                       ("predict_async_resident", lambda: s8.predict_async_resident(res, scores=buf, output_prob=True))):
        buf[:] = np.float32(-7.0)
        call()
        s8.train_flush()
        assert_bitwise(buf[:blk.n_rows].copy(), want, what)
    s8.free_score_buffer(buf)
    cutter.release(res)
    cutter.destroy()
    s8.close()
    s32.close()


REFUSED = {
    "score_candidates": lambda e, t, b: e.score_candidates(take_rows(b, [0]), np.array([0, 1], np.int32), take_rows(b, [1])),
    "set_pair_mask": lambda e, t, b: e.set_pair_mask(fa.pair_mask(3, [(0, 1)])),
    "ablation": lambda e, t, b: e.ablation_enable(),
    "predict_ablated": lambda e, t, b: e.predict_ablated(b),
    "pair_ablation": lambda e, t, b: e.pair_ablation_enable(),
    "predict_pair_ablated": lambda e, t, b: e.predict_pair_ablated(b),
    "pair_curve": lambda e, t, b: e.pair_curve_enable(fa.pair_curve_levels(3, list(range(6))), [1]),
    "predict_pair_curve": lambda e, t, b: (setattr(e, "_curve_variants", 2), e.predict_pair_curve(b)),
    "sync_from": lambda e, t, b: e.sync_from(t),
    "get_rows_raw": lambda e, t, b: e.get_rows_raw([1, 2]),
    "set_rows_raw": lambda e, t, b: e.set_rows_raw([1], lat=np.zeros((1, 12), np.float32)),
    "export_delta": lambda e, t, b: e.export_delta(),
    "apply_delta": lambda e, t, b: e.apply_delta(dict(fmt="f8", ids=[1], bias=[0], lin_w=[0], lat=np.zeros((1, 12), np.uint8))),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_on_an_f8_engine(name):
    t, s = engine(3, 4), engine(3, 4, "f8")
    before = s.get_weights()
    with pytest.raises(fa.EngineError) as err:
        REFUSED[name](s, t, block(3, [3, 2], seed=3))
    assert err.value.code == fa.engine.E_UNSUPPORTED and "f8" in str(err.value), str(err.value)
    after = s.get_weights()
    assert all(np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)) for key in before)
    t.close()
    s.close()
