"""FFM_FLAG_LEARN (the opt-in learning variant) against the oracle's
restatement on every update and refresh path: the refresh keeps a latent slot's w until its first
gradient (not n > 0), and ffm.cpp:118 takes g2*g2.  Every kernel family branches on the flag on its
own, so each case names the occurrence classes (util.EDGE_COUNTS / FM_EDGE_COUNTS) its blocks reach
and checks that the kept-w branch is live there.  With g2*g2 no square root goes negative, so the
state stays finite and blocks are chained without resetting it.  Every comparison is bit for bit:
logits and the whole state after every block (compact shards: owned rows, unowned rows zero)."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import CpuModel
from util import (DEFAULT_HP, EDGE_COUNTS, FM_EDGE_COUNTS, STRESS_HP, assert_bitwise, assert_rank_rows,
                  assert_state_bitwise, bits, block_ids_per_field, fast_state, ftrl_w, get_bias3,
                  grid_block, grid_want, irregular_copy, keep_columns, kept_copy, occurrence_block,
                  run_rank_staged)

pytestmark = pytest.mark.gpu

ROWS = 6144  # the largest count (4097) in one field, every field with room for once-only ids
# per-block occurrence classes (kernels_group.h): [lo, hi] counts
FFM_CLASSES = dict(once=(1, 1), few=(2, 10), hot=(11, 128), very_hot=(129, 256), giant=(257, 2047),
                   super=(2048, 1 << 30))
FM_CLASSES = dict(once=(1, 1), few=(2, 10), hot=(11, 64), giant=(65, 1 << 30))


def class_counts(blk, table):
    """How many features of the block fall in each occurrence class, counted from the block."""
    c = np.unique(blk.feat, return_counts=True)[1]
    return {name: int(((c >= lo) & (c <= hi)).sum()) for name, (lo, hi) in table.items()}


def assert_reaches(blk, table, what):
    cnt = class_counts(blk, table)
    assert all(v > 0 for v in cnt.values()), (what, cnt)


def train_both(o, e, blk, what):
    lo, so = o.train_batch(blk)
    lg, sg = e.train_batch(blk)
    assert_bitwise(lg, lo, what + " logits")
    if np.isnan(so):  # (a saturated logit: 0 * log(0) in the loss)
        assert np.isnan(sg), what
    else:
        assert abs(sg - so) <= 1e-9 * max(1.0, abs(so)), (what, sg, so)


def assert_branches_live(st0, learn1, ref1, ids, counts, table, cols_of, hp, what):
    """Per occurrence class, on the edge features: (a) a touched slot with n0 = 0 whose w0 is not
    W(0, z0) still holds w0 after block 1; (b) the reference rule's block 1 ends elsewhere in the
    features' (n, z)."""
    counts = np.asarray(counts)
    for name, (lo, hi) in table.items():
        sel = ids[(counts >= lo) & (counts <= hi)]
        kept = 0
        for i in sel:
            cols = cols_of(int(i))
            n0, z0, w0 = st0["vec_n"][i, cols], st0["vec_z"][i, cols], st0["vec_w"][i, cols]
            cand = (n0 == 0) & (bits(learn1["vec_w"][i, cols]) == bits(w0)) & (learn1["vec_n"][i, cols] > 0)
            kept += sum(ftrl_w(0.0, z, hp) != w for z, w in zip(z0[cand], w0[cand]))
        assert kept > 0, "%s %s: no touched slot kept its w0 != W(0, z0)" % (what, name)
        assert any((bits(learn1[key][sel]) != bits(ref1[key][sel])).any() for key in ("vec_n", "vec_z")), (
            "%s %s: the learning variant's (n, z) equal the reference rule's" % (what, name))


def _ffm_edges(F, k, split, with_field_start, monkeypatch, seed):
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    per = block_ids_per_field(ROWS)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, learn=True, **STRESS_HP)
    st = fast_state(np.random.default_rng(seed), o, n_zero=0.4)  # w ~ N(0, 0.02): not W(n, z)
    o.set_state(st)
    fs = (np.arange(F + 1) * per).astype(np.int32) if with_field_start else None
    e = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F,
                  max_row_nnz=F, field_start=fs, learn=True, **STRESS_HP)
    e.set_state(st)
    first, ids, field_of = occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed)
    blocks = [("regular", first),
              ("irregular", irregular_copy(occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed + 1)[0], seed=seed)),
              ("regular", occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed + 2)[0])]
    for b, (name, blk) in enumerate(blocks):
        what = "learn k=%d split=%s fs=%s block %d (%s)" % (k, split, with_field_start, b, name)
        assert_reaches(blk, FFM_CLASSES, what)
        train_both(o, e, blk, what)
        so = o.get_state()
        assert all(np.isfinite(v).all() for v in so.values()), what + ": the oracle left finite values"
        assert_state_bitwise(e.get_state(), so, what)
        if b == 0:
            ref = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
            ref.set_state(st)
            ref.train_batch(first)
            partners = lambda i: np.flatnonzero(np.repeat(np.arange(F) != field_of[list(ids).index(i)], k))
            assert_branches_live(st, so, ref.get_state(), ids, EDGE_COUNTS, FFM_CLASSES, partners, STRESS_HP,
                                 what)
            del ref
    e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
@pytest.mark.parametrize("k", [4, 8, 16, 32])
def test_learn_every_edge_count_whole_model(k, split, monkeypatch):
    """F = 8 with field_start (the range sort and the regular-block folds), three chained blocks."""
    _ffm_edges(8, k, split, True, monkeypatch, seed=600 + k)


def test_learn_every_edge_count_generic_kernel(monkeypatch):
    """k = 6: the scalar refresh and the generic update kernel."""
    _ffm_edges(8, 6, "0", True, monkeypatch, seed=611)


def test_learn_every_edge_count_library_sort(monkeypatch):
    """No field_start: the library sort and the general folds."""
    _ffm_edges(8, 16, "0", False, monkeypatch, seed=612)


@pytest.mark.parametrize("k", [8, 64, 128])
def test_learn_every_fm_edge_count(k):
    """FM: the wave kernel (k <= 64) and fm_row_kernel (k = 128); giants from 65 occurrences."""
    cols, n_rows = 4, 1024
    per = block_ids_per_field(n_rows)
    nf = cols * per
    o = CpuModel("oracle", "FM", nf, 1, k, learn=True, **STRESS_HP)
    st = fast_state(np.random.default_rng(700 + k), o, n_zero=0.4)
    o.set_state(st)
    e = fa.Engine("FM", nf, 1, k, skip_init=True, max_batch_rows=n_rows, max_row_nnz=cols, learn=True,
                  **STRESS_HP)
    e.set_state(st)
    first, ids, _ = occurrence_block(cols, FM_EDGE_COUNTS, n_rows, seed=710)
    blocks = [first, irregular_copy(occurrence_block(cols, FM_EDGE_COUNTS, n_rows, seed=711)[0], seed=7),
              occurrence_block(cols, FM_EDGE_COUNTS, n_rows, seed=712)[0]]
    for blk in blocks:
        blk.field[:] = 0  # libsvm rows
    for b, blk in enumerate(blocks):
        what = "learn FM k=%d block %d" % (k, b)
        assert_reaches(blk, FM_CLASSES, what)
        train_both(o, e, blk, what)
        so = o.get_state()
        assert all(np.isfinite(v).all() for v in so.values()), what
        assert_state_bitwise(e.get_state(), so, what)
        if b == 0:
            ref = CpuModel("oracle", "FM", nf, 1, k, **STRESS_HP)
            ref.set_state(st)
            ref.train_batch(first)
            assert_branches_live(st, so, ref.get_state(), ids, FM_EDGE_COUNTS, FM_CLASSES,
                                 lambda i: np.arange(k), STRESS_HP, what)
    e.close()


def test_learn_every_edge_count_on_eight_compact_shards(monkeypatch):
    """F = 39, k = 16 through eight compact shards (kept columns, staged two ahead as bench.py does,
    the oracle's logits in place of the all-reduce): the flat few kernel, the once-only kernel and
    the rank's row kernel under the flag; then rank 0 again at FFM_GRID_SMALL=1, so that the flat
    few kernel takes later rounds."""
    F, k, S, n_rows = 39, 16, 8, 4352
    per = block_ids_per_field(n_rows)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, learn=True, **STRESS_HP)
    st = fast_state(np.random.default_rng(800), o, n_zero=0.4)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    plan = fa.shard_plan(F, S, field_map=True)
    o.set_state(st)
    blocks = [occurrence_block(F, EDGE_COUNTS, n_rows, seed=810 + s)[0] for s in range(2)]
    for b in blocks:
        assert_reaches(b, FFM_CLASSES, "compact shards")
    logits = [o.train_batch(b)[0] for b in blocks]
    assert np.isfinite(o._view("vec_z", (nf * F * k,))).all()
    ids = np.arange(nf, dtype=np.int32)
    want = {key: o._view(key, (nf, F * k) if key.startswith("vec") else (nf,)) for key in fa.Engine.ROW_KEYS}

    def rank(r):
        e = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=n_rows, max_batch_nnz=n_rows * F,
                      n_shards=S, shard_rank=r, max_row_nnz=F, field_start=fs, learn=True, **STRESS_HP)
        e.set_state(st)
        keep = keep_columns(plan, r)
        parts = run_rank_staged(e, [kept_copy(b, keep) for b in blocks], logits)
        assert_rank_rows(e, r, ids, ids // per, want, plan, k, "learn edge counts")
        if r == plan["bias_owner"]:
            assert_bitwise(get_bias3(e), o._view("bias3", (3,)), "bias3")
        e.close()
        return parts

    total = [np.zeros(n_rows, np.float64) for _ in blocks]
    for r in range(S):
        for i, p in enumerate(rank(r)):
            total[i] += p
    for i in range(len(blocks)):
        np.testing.assert_allclose(total[i].astype(np.float32), logits[i], rtol=1e-5, atol=2e-6)
    monkeypatch.setenv("FFM_GRID_SMALL", "1")
    rank(0)


# ---- every refresh site on the special values of the rule ---------------------------------------
GRID_CASES = ([("FFM", 4, {}), ("FFM", 6, {}), ("FFM", 16, {}), ("FM", 8, {}), ("FM", 128, {})]
              + [("FFM", 16, {"FFM_ENGINE_ROW_REFRESH": v}) for v in "0123"]
              + [("FFM", 16, {"FFM_ROW_PARK": v}) for v in ("0", "96")])


@pytest.mark.parametrize("occurrences", [1, 2], ids=["in_row_refresh", "refresh_kernel"])
@pytest.mark.parametrize("mt,k,env", GRID_CASES,
                         ids=["%s_k%d%s" % (m, k, "".join("_%s=%s" % kv for kv in env.items()))
                              for m, k, env in GRID_CASES])
def test_learn_refresh_on_special_values(mt, k, env, occurrences, monkeypatch):
    """util.special_grid injected as latent and linear accumulators and touched once (the row
    kernel refreshes) or twice (ffm_refresh_kernel / the FM row kernel): the w the engine stores
    (the update never writes w) against the oracle and against util.latent_w / ftrl_w."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    hp = STRESS_HP
    g = grid_block(mt, k, hp, occurrences)
    assert_reaches(g["block"], dict(touches=(occurrences, occurrences)), mt)
    assert class_counts(g["block"], dict(other=(1, 1 << 30)))["other"] == class_counts(
        g["block"], dict(touches=(occurrences, occurrences)))["touches"]
    o = CpuModel("oracle", mt, g["nf"], g["F"], k, learn=True, **hp)
    o.set_state(g["state"])
    e = fa.Engine(mt, g["nf"], g["F"], k, skip_init=True, max_batch_rows=g["block"].n_rows, max_row_nnz=2,
                  field_start=g["field_start"], learn=True, **hp)
    e.set_state(g["state"])
    lo, _ = o.train_batch(g["block"])
    lg, _ = e.train_batch(g["block"])
    assert_bitwise(lg, lo, "logits")
    got = e.get_state()
    assert_state_bitwise(got, o.get_state(), "learn %s k=%d %s" % (mt, k, env))
    want, want_lin = grid_want(g, hp, True)
    assert_bitwise(got["vec_w"][g["slots"]], want, "latent w = the rule")
    assert_bitwise(got["lin_w"][g["lin"]], want_lin, "linear w = W(n, z)")
    e.close()


def test_learn_refresh_on_special_values_compact_shards():
    """The same grid through two compact shards of F = 2 (rank 0 owns the pair, rank 1 the linear
    terms and the bias), touched once and twice."""
    hp, k, S = STRESS_HP, 16, 2
    plan = fa.shard_plan(2, S, field_map=True)
    for occ in (1, 2):
        g = grid_block("FFM", k, hp, occ)
        o = CpuModel("oracle", "FFM", g["nf"], 2, k, learn=True, **hp)
        o.set_state(g["state"])
        blk = g["block"]
        logits = [o.train_batch(blk)[0]]
        so = o.get_state()
        want, _ = grid_want(g, hp, True)
        assert_bitwise(so["vec_w"][g["slots"]], want, "oracle latent w")
        ids = np.arange(g["nf"], dtype=np.int32)
        for r in range(S):
            e = fa.Engine("FFM", g["nf"], 2, k, skip_init=True, max_batch_rows=blk.n_rows, n_shards=S,
                          shard_rank=r, max_row_nnz=2, field_start=g["field_start"], learn=True, **hp)
            e.set_state(g["state"])
            run_rank_staged(e, [kept_copy(blk, keep_columns(plan, r))], logits)
            assert_rank_rows(e, r, ids, (ids >= g["field_start"][1]).astype(np.int32), so, plan, k,
                             "grid occ=%d" % occ)
            if r == plan["bias_owner"]:
                assert_bitwise(get_bias3(e), so["bias3"], "bias3")
            e.close()


def test_learn_fresh_model_end_to_end():
    """What a --learn user starts from: a seeded engine (no skip_init) against the oracle on the same
    initial bits, n = z = 0.  FFM 39 x 16 with field_start, the reference's default hyper-parameters,
    Zipf blocks of 8192 rows over about 1000 ids per field: four staged zero-copy blocks, then
    predict_batch with loss on a fifth.  The factors must move off their initial values, where the
    reference rule's first refresh writes W(0, 0) = 0."""
    F, k, per, B, seed = 39, 16, 1000, 8192, 77
    nf = F * per
    hp = DEFAULT_HP
    assert ftrl_w(0.0, 0.0, hp) == 0
    o = CpuModel("oracle", "FFM", nf, F, k, learn=True, **hp)
    st = o.zero_state()
    st["vec_w"][...] = fa.init_weights_host(seed, 0.0, 0.02, 1, 0, nf * F * k).reshape(nf, F * k)
    st["lin_w"][...] = fa.init_weights_host(seed, 0.0, 0.02, 0, 0, nf)
    o.set_state(st)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    e = fa.Engine("FFM", nf, F, k, seed=seed, max_batch_rows=B, max_batch_nnz=B * F, max_row_nnz=F,
                  field_start=fs, learn=True, **hp)
    gen = synth.Generator(F, nf, "zipf", seed=78)

    def own(c):
        def cp(a):
            out = fa.page_aligned(a.size, a.dtype)
            out[:] = a
            return out
        return type(c)(cp(c.row_ptr), cp(c.field), cp(c.feat), cp(c.val), cp(c.label))
    blocks = [own(gen.block(B)) for _ in range(4)]
    cnt = class_counts(blocks[0], FFM_CLASSES)
    assert cnt["once"] > 0 and cnt["few"] > 0 and cnt["hot"] > 0 and cnt["giant"] > 0, cnt
    want_logits = [o.train_batch(b)[0] for b in blocks[:1]]
    w1 = o.get_state()["vec_w"]
    ref = CpuModel("oracle", "FFM", nf, F, k, **hp)
    ref.set_state(st)
    ref.train_batch(blocks[0])
    assert_bitwise(w1, st["vec_w"], "first refresh (n = 0 keeps the initial w ...)")
    r1 = ref.get_state()["vec_w"]
    zeroed = (r1 == 0) & (st["vec_w"] != 0)  # (... where the reference rule writes W(0, 0) = 0)
    assert zeroed.sum() > 10000
    del ref, r1
    want_logits += [o.train_batch(b)[0] for b in blocks[1:]]
    for b in blocks:
        e.pin_block(b)
    out = torch.zeros(B, dtype=torch.float32, device="cuda")
    staged = 0
    for i, b in enumerate(blocks):
        while staged < min(i + 3, len(blocks)):  # (two ahead, as bench.py stages them)
            e.stage_batch(blocks[staged], zero_copy=True)
            staged += 1
        e.train_staged(out.data_ptr())
        e.sync()
        assert_bitwise(out.cpu().numpy(), want_logits[i], "fresh model block %d logits" % i)
    so = o.get_state()
    assert_state_bitwise(e.get_state(), so, "fresh model after four blocks")
    moved = (so["vec_w"] != st["vec_w"]) & zeroed
    assert moved.sum() > 10000, moved.sum()
    test = gen.block(B)
    lo, so_loss = o.predict_batch(test)
    lg, sg = e.predict_batch(test)
    assert_bitwise(lg, lo, "fresh model predict")
    assert abs(sg - so_loss) <= 1e-9 * max(1.0, abs(so_loss)), (sg, so_loss)
    for b in blocks:
        e.unpin_block(b)
    e.close()


def test_learn_flag_leaves_lr_unchanged():
    """LR has no latent factors: the flag changes no bit."""
    nf = 3000
    blk = synth.Generator(13, nf, "zipf", seed=9).block(4096)
    blk.field[:] = 0
    out = []
    for learn in (False, True):
        e = fa.Engine("LR", nf, 1, 1, skip_init=True, max_batch_rows=4096, learn=learn, **STRESS_HP)
        e.fill_state(seed=3)
        lg = [e.train_batch(blk.rows(lo, lo + 1024)) for lo in range(0, 4096, 1024)]
        out.append((lg, e.get_state()))
        e.close()
    for (la, sa), (lb, sb) in zip(out[0][0], out[1][0]):
        assert_bitwise(la, lb, "LR logits")
        assert sa == sb
    assert_state_bitwise(out[0][1], out[1][1], "LR state")
