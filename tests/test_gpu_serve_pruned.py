"""Pruned serving tables (include/ffm_engine.h; csrc/kernels_pruned.h) against an unpruned serving engine of the same
format and weights under set_pair_mask(keep), the oracle on fa.prune_rows of the decoded table, and fa.pruned_layout."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from test_gpu_serve import decoded
from util import STRESS_HP, assert_bitwise, loss_close

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 2, 23, 24, 39, 64, 65, 128)


def ranges(F):  # unequal id ranges, one of them empty from 39 fields on
    return np.concatenate([[0], np.cumsum([0 if f == 7 and F >= 39 else 2 + f % 3 for f in range(F)])]).astype(np.int32)


def masks(F):
    half = np.triu(np.random.default_rng(5 + F).random((F, F)) < 0.5)
    every = [(f, g) for f in range(F) for g in range(f, F)]
    return {"all": fa.pair_mask(F, every), "diagonal": fa.pair_mask(F, [(f, f) for f in range(F)]),
            "half": fa.pair_mask(F, list(zip(*np.nonzero(half)))),
            "lone": fa.pair_mask(F, [p for p in every if F // 2 not in p]),  # field F // 2 without any partner
            "empty": fa.pair_mask(F, [])}


@functools.lru_cache(maxsize=None)
def block(F):  # rows on the length ladder: ids inside their field's range, fields repeated inside a row
    rng, fs = np.random.default_rng(1), ranges(F)
    live = np.flatnonzero(np.diff(fs) > 0)
    rows = [[(int(f), int(rng.integers(fs[f], fs[f + 1])), float(rng.uniform(0.5, 1.5))) for f in rng.choice(live, n)] for n in LENGTHS]
    return Csr.from_rows(rows, rng.integers(0, 2, len(rows)).astype(np.int32))


@functools.lru_cache(maxsize=None)
def weights(F, k):
    rng, nf = np.random.default_rng(F * 100 + k), int(ranges(F)[-1])
    return dict(bias=np.array([0.25], np.float32), lin_w=rng.normal(0, 0.1, nf).astype(np.float32),
                vec_w=rng.normal(0, 0.25, (nf, F * k)).astype(np.float32))


def engine(F, k, fmt, prune=None, st=None, **kw):
    kw.setdefault("skip_init", True)
    e = fa.Engine("FFM", int(ranges(F)[-1]), F, k, serve=fmt, field_start=ranges(F), prune=prune, max_batch_rows=32,
                  max_batch_nnz=2048, **dict(STRESS_HP, **kw))
    if st is not None:
        e.set_weights(**st)
    return e


def device_predict(e, b, prob):
    d = [torch.from_numpy(np.ascontiguousarray(getattr(b, key))).cuda() for key in ("row_ptr", "field", "feat", "val", "label")]
    out = torch.full((b.n_rows,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.predict_batch_device(b.n_rows, int(b.row_ptr[-1]), *[a.data_ptr() for a in d], prob, out.data_ptr(), None)
    return e.lib.ffm_engine_sync(e.h), out.cpu().numpy()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("F", [3, 39, 64])
def test_rows_against_a_masked_engine(F, k, fmt):
    blk, st = block(F), weights(F, k)
    half, fl = masks(F)["half"], [blk.field[blk.row_ptr[r]:blk.row_ptr[r + 1]] for r in (5, 8)]  # the rows of 39 and 128 entries
    kept = [sum(int(half[int(f[a])]) >> int(f[b]) & 1 for a in range(len(f)) for b in range(a + 1, len(f))) for f in fl]
    assert 0 < kept[0] and kept[1] > 256 + 64, "the half mask crosses a batch of terms and the queue behind it"
    masked = engine(F, k, fmt, st=st)
    for name, words in masks(F).items():
        masked.set_pair_mask(words)
        e = engine(F, k, fmt, prune=words, st=st)
        for prob in (False, True):
            want, wl = masked.predict_batch(blk, output_prob=prob)
            got, gl = e.predict_batch(blk, output_prob=prob)
            what = "F=%d k=%d %s mask %s prob=%d" % (F, k, fmt, name, prob)
            assert_bitwise(got, want, what)
            assert loss_close(gl, wl), what
            assert_bitwise(device_predict(e, blk, prob)[1], want, what + " device")
        out = e.score_buffer(blk.n_rows)
        e.predict_batch_async(blk, scores=out, output_prob=True)
        e.train_flush()
        assert_bitwise(out[:blk.n_rows], want, what + " async")
        e.free_score_buffer(out)
        e.close()
    masked.close()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_rows_against_the_oracle(k, fmt):
    F = 39
    blk, st, words = block(F), weights(F, k), masks(F)["half"]
    o = CpuModel("oracle", "FFM", int(ranges(F)[-1]), F, k, **STRESS_HP)
    z = o.zero_state()
    z["bias3"][0], z["lin_w"], z["vec_w"] = st["bias"][0], st["lin_w"], fa.prune_rows(decoded(st["vec_w"], fmt), words, ranges(F))
    o.set_state(z)
    e = engine(F, k, fmt, prune=words, st=st)
    for prob in (False, True):
        want, wl = o.predict_batch(blk, output_prob=prob)
        # The oracle adds a +-0.0 term for every zeroed slot; that changes no bit unless a partial sum is -0.0.  A
        # round-to-nearest sum is -0.0 only as (-0.0) + (-0.0), and the chain starts at the bias: with a positive bias
        # and no -0.0 among the final sums, no partial sum was -0.0 (the partial sums themselves are not read here).
        if not prob:
            assert st["bias"][0] > 0 and (want.view(np.uint32) != 0x80000000).all()
        got, gl = e.predict_batch(blk, output_prob=prob)
        assert_bitwise(got, want, "k=%d %s prob=%d" % (k, fmt, prob))
        assert loss_close(gl, wl)
    e.close()


def test_edges():
    """An id outside its field's range is erased whole: the same block with that entry removed.  A 129-entry device
    row is NaN and E_CAPACITY, and its neighbours keep their bits."""
    F, k = 39, 16
    blk, fs = block(F), ranges(F)
    e = engine(F, k, "f16", prune=masks(F)["half"], st=weights(F, k))
    want = e.predict_batch(blk)[0]
    feat, keep = blk.feat.copy(), np.ones(blk.feat.size, bool)
    for r in range(2, blk.n_rows):  # entry 1 of every row of two entries or more gets an id of a neighbouring range
        p = int(blk.row_ptr[r]) + 1
        f = int(blk.field[p])
        feat[p], keep[p] = (fs[f + 1] if fs[f + 1] < fs[-1] else fs[f] - 1), False
    ptr = np.concatenate([[0], np.cumsum([keep[blk.row_ptr[r]:blk.row_ptr[r + 1]].sum() for r in range(blk.n_rows)])]).astype(np.int32)
    erased = e.predict_batch(Csr(blk.row_ptr, blk.field, feat, blk.val, blk.label))[0]
    assert_bitwise(erased, e.predict_batch(Csr(ptr, blk.field[keep], blk.feat[keep], blk.val[keep], blk.label))[0], "erased entries")
    assert (erased[2:].view(np.uint32) != want[2:].view(np.uint32)).all()
    # the block, a row of 129 entries, the block again
    n, end = blk.n_rows, int(blk.row_ptr[-1])
    long_f = np.resize(np.flatnonzero(np.diff(fs) > 0), 129).astype(np.int32)
    cat = lambda a, b: np.concatenate([a, b, a]).astype(a.dtype)  # noqa: E731
    big = Csr(np.concatenate([blk.row_ptr, [end + 129], end + 129 + blk.row_ptr[1:]]).astype(np.int32), cat(blk.field, long_f),
              cat(blk.feat, fs[long_f]), cat(blk.val, np.ones(129, np.float32)), cat(blk.label, np.zeros(1, np.int32)))
    code, got = device_predict(e, big, False)
    assert code == fa.engine.E_CAPACITY and np.isnan(got[n])
    assert_bitwise(np.concatenate([got[:n], got[n + 1:]]), np.concatenate([want, want]), "the long row's neighbours")
    e.close()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("F,k", [(3, 4), (39, 8)])  # the pack kernel's 16 and 64 lanes per feature; f16's 8- and 16-byte items
def test_contents(F, k, fmt):
    fs, words, st = ranges(F), masks(F)["half"], weights(F, k)
    nf = int(fs[-1])
    base, P = fa.pruned_layout(words, fs)
    # create: the training engine's draws, pruned and rounded; the layout, the mask and the bytes
    t = fa.Engine("FFM", nf, F, k, max_batch_rows=16, max_batch_nnz=2048, seed=9, **STRESS_HP)
    e = engine(F, k, fmt, prune=words, skip_init=False, seed=9)
    drawn = t.get_weights()
    assert_bitwise(e.get_weights()["vec_w"], fa.prune_rows(decoded(drawn["vec_w"], fmt), words, fs), "create-time table")
    assert np.array_equal(e.pruned_layout()[0], base) and np.array_equal(e.pruned_layout()[1], P) and np.array_equal(e.pair_mask(), words)
    assert 0 < base[-1] < nf * F and e.model_bytes() == 4 + 4 * nf + int(base[-1]) * k * {"f32": 4, "f16": 2}[fmt]
    # pack_from and its counters
    t.set_weights(**st)
    stats = e.pack_from(t)
    held = decoded(st["vec_w"], fmt)
    live = fa.prune_rows(np.ones_like(held), words, fs) != 0
    assert_bitwise(e.get_weights()["vec_w"], fa.prune_rows(held, words, fs), "packed table")
    assert_bitwise(e.get_weights()["lin_w"], st["lin_w"], "packed lin_w")
    assert stats["n_latent"] == int(base[-1]) * k == int(live.sum()) and stats["n_inexact"] == int((held != st["vec_w"])[live].sum())
    # set_rows on an id list that crosses fields, then get_rows: dropped slots read +0.0
    ids = np.array([nf - 1, 0, int(fs[F // 2]), int(fs[1]) + 1], np.int32)
    full = np.array(held)
    full[ids] = decoded(np.random.default_rng(2).normal(0, 1, (ids.size, F * k)).astype(np.float32), fmt)
    e.set_rows(ids, {"vec_w": full[ids]})
    want = fa.prune_rows(full, words, fs)
    assert_bitwise(e.get_rows(ids)["vec_w"], want[ids], "get_rows")
    assert_bitwise(e.get_weights()["vec_w"], want, "the table behind set_rows")  # (bitwise: the dropped slots are +0.0)
    t.close()
    e.close()


TABLE = "pruned serving table"
REFUSED = {  # name: (the call, what its message names)
    "set_pair_mask": (lambda e, t: e.set_pair_mask(masks(e.n_fields)["all"]), ("set_pair_mask", TABLE)),
    "set_pair_mask(None)": (lambda e, t: e.set_pair_mask(None), ("set_pair_mask", TABLE)),
    "score_candidates": (lambda e, t: e.score_candidates(block(3).rows(1, 2), np.array([0, 1], np.int32), block(3).rows(2, 3)),
                         ("score_candidates", TABLE)),
    "ablation_enable": (lambda e, t: e.ablation_enable(), ("field ablation", TABLE)),
    "pair_ablation_enable": (lambda e, t: e.pair_ablation_enable(), ("pair ablation", TABLE)),
    "pair_curve_enable": (lambda e, t: e.pair_curve_enable(np.zeros((3, 3), np.uint16), [1]), ("pruning curve", TABLE)),
    "sync_from": (lambda e, t: e.sync_from(t), ("sync_weights", TABLE)),
    "get_rows_raw": (lambda e, t: e.get_rows_raw(np.array([0], np.int32)), ("get_rows_raw", TABLE)),
    "set_rows_raw": (lambda e, t: e.set_rows_raw(np.array([0], np.int32), lin_w=np.zeros(1, np.float32)), ("set_rows_raw", TABLE)),
    "export_delta": (lambda e, t: e.export_delta(), ("export_delta", TABLE)),
    "apply_delta": (lambda e, t: e.apply_delta(dict(fmt="f32", ids=np.array([0], np.int32), bias=np.zeros(1, np.float32),
                                                    lin_w=np.zeros(1, np.float32), lat=np.zeros((1, e.row_len), np.float32))),
                    ("apply_delta", TABLE)),
    "train_batch": (lambda e, t: e.train_batch(block(3)), ("serving engine",)),  # (as on any serving engine)
    "FFM_FLAG_SERVE_F8": (lambda e, t: engine(3, 4, "f8", prune=masks(3)["half"]), ("FFM_FLAG_SERVE_F8", TABLE)),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_by_name(name):
    F, k = 3, 4
    e = engine(F, k, "f32", prune=masks(F)["half"], st=weights(F, k))
    t = fa.Engine("FFM", int(ranges(F)[-1]), F, k, max_batch_rows=16, max_batch_nnz=2048, **STRESS_HP)
    before = e.get_weights()
    call, named = REFUSED[name]
    with pytest.raises(fa.EngineError) as ei:
        call(e, t)
    assert ei.value.code == fa.engine.E_UNSUPPORTED and all(text in str(ei.value) for text in named), str(ei.value)
    for key, a in e.get_weights().items():
        assert_bitwise(a, before[key], "%s after %s" % (key, name))
    t.close()
    e.close()
