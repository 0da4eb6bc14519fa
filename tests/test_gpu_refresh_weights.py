"""ffm_engine_refresh_weights / ffm_group_refresh_weights (include/ffm_engine.h "Refresh"): one pass over
everything the engine stores sets w = W(n, z) wherever (n, z) are not both zero bits, counts what it saw,
and leaves (n, z) -- and with them the training trajectory -- alone.

  * every element against the rule, W from the oracle's maybe_zero_weight, on the smallest shapes that
    reach every path of the kernel (one feature, a partial last wave, both scalar record lengths, the
    16-byte path), with and without the short divide, with planted edge values, with the learning variant;
  * idempotence, the unchanged trajectory, the unchanged changed-feature set, the drain of staged blocks;
  * what it is for: after it the engine predicts what an oracle with refreshed weights predicts, and a
    feature seen in a single block is no longer scored by its create-time weight;
  * groups of compact and full-length shards against the unsharded engine."""
import numpy as np
import pytest

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from util import HP_SETS, STRESS_HP, assert_bitwise, bits, loss_close

pytestmark = pytest.mark.gpu

COUNT_KEYS = ("lin_live", "lin_nonzero", "lin_moved", "lat_live", "lat_nonzero", "lat_moved")
# (model type, n_feats, fields, factors): LR with one feature; LR with a partial last wave; FM with a
# record of 5 floats (scalar path); FFM 4 x 4 (row_len 16: the 16-byte path, 300 records = more than one
# wave of vectors); FFM 3 x 3 (row_len 9, scalar path, one feature past a 64 boundary)
SHAPES = [("LR", 1, 1, 1), ("LR", 257, 1, 1), ("FM", 40, 1, 5), ("FFM", 300, 4, 4), ("FFM", 65, 3, 3)]
# the defaults, and an alpha above 2^30: ffm_engine_create leaves fast_div (and fast_w) off for it
HPS = ["default_hp", "alpha_above_2p30"]


def _rule(hp):
    o = CpuModel("oracle", "LR", 1, 1, 1, **hp)
    cache = {}

    def w_of(n, z):
        key = (int(bits(np.float32(n).reshape(1))[0]), int(bits(np.float32(z).reshape(1))[0]))
        if key not in cache:
            cache[key] = np.float32(o.maybe_zero_weight(float(n), float(z)))
        return cache[key]
    return w_of


def _expected(st, hp, learn):
    """(expected state w arrays, counts) of the rule applied to the state's (w, n, z)."""
    w_of = _rule(hp)
    out, cnt = {}, dict.fromkeys(COUNT_KEYS, 0)
    parts = [("lin", st["lin_w"].ravel(), st["lin_n"].ravel(), st["lin_z"].ravel(), False),
             ("lin", st["bias3"][0:1], st["bias3"][1:2], st["bias3"][2:3], False),
             ("lat", st["vec_w"].ravel(), st["vec_n"].ravel(), st["vec_z"].ravel(), True)]
    res = []
    for part, w, n, z, latent in parts:
        live = (bits(n) | bits(z)) != 0
        new = w.copy()
        for i in np.flatnonzero(live):
            if latent and learn and not (n[i] > 0):
                continue  # keeps w_old
            new[i] = w_of(n[i], z[i])
        res.append(new)
        cnt[part + "_live"] += int(live.sum())
        cnt[part + "_nonzero"] += int((live & ~(new == 0)).sum())
        cnt[part + "_moved"] += int((live & (bits(new) != bits(w))).sum())
    out["lin_w"] = res[0]
    out["bias_w"] = res[1]
    out["vec_w"] = res[2].reshape(st["vec_w"].shape)
    return out, cnt


def _counts_from(before, after):
    """The six counters derived from the arrays the engine holds before and after the call."""
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    for part, w0, w1, n, z in (("lin", before["lin_w"], after["lin_w"], before["lin_n"], before["lin_z"]),
                               ("lin", before["bias3"][0:1], after["bias3"][0:1], before["bias3"][1:2], before["bias3"][2:3]),
                               ("lat", before["vec_w"], after["vec_w"], before["vec_n"], before["vec_z"])):
        live = (bits(n) | bits(z)) != 0
        cnt[part + "_live"] += int(live.sum())
        cnt[part + "_nonzero"] += int((live & ~(w1 == 0)).sum())
        cnt[part + "_moved"] += int((live & (bits(w1) != bits(w0))).sum())
    return cnt


def _prepared_engine(shape, hp, learn, seed=3):
    """An engine after fill_state with (n, z) of about a third of the elements zeroed and the edge values
    planted; returns (engine, the state it holds)."""
    mt, nf, F, k = shape
    e = fa.Engine(mt, nf, F, k, seed=seed, learn=learn, max_batch_rows=64, **hp)
    e.fill_state(seed=seed + 1)
    st = e.get_state()
    rng = np.random.default_rng(seed)
    f32 = np.float32
    l1 = f32(hp["w_l1"])
    # (n, z) edge pairs: -0.0 with n = 0 (live by its bits); |z| == l1; |z| one ulp above l1 (both signs);
    # n = 0 with z != 0; a NaN z; a NaN n (the learning variant keeps w_old there)
    edges = [(f32(0), f32(-0.0)), (f32(0.5), l1), (f32(0.5), -l1), (f32(0.5), np.nextafter(l1, f32(np.inf))),
             (f32(0.5), -np.nextafter(l1, f32(np.inf))), (f32(0), f32(0.3)), (f32(0.25), f32(np.nan)),
             (f32(np.nan), f32(0.3))]
    for nk, zk in (("lin_n", "lin_z"), ("vec_n", "vec_z")):
        n, z = st[nk].reshape(-1), st[zk].reshape(-1)
        if n.size == 0:
            continue
        dead = rng.random(n.size) < 1 / 3
        n[dead] = 0
        z[dead] = 0
        at = rng.permutation(n.size)[:len(edges)]  # (LR with one feature: the first edge only)
        for p, (en, ez) in zip(at, edges):
            n[p], z[p] = en, ez
    e.set_state(st)
    held = e.get_state()
    for key in st:
        assert np.array_equal(bits(held[key]), bits(st[key])), key  # (the planted patterns arrived)
    return e, held


def _check_refresh(shape, hp, learn):
    e, before = _prepared_engine(shape, hp, learn)
    mt = shape[0]
    assert mt == "LR" or ((bits(before["vec_n"]) | bits(before["vec_z"])) == 0).any()  # dead elements exist
    assert np.isnan(before["lin_z"]).any() or shape[1] == 1
    got = e.refresh_weights()
    after = e.get_state()
    want, want_cnt = _expected(before, hp, learn)
    assert_bitwise(after["lin_w"], want["lin_w"], "lin_w")
    assert_bitwise(after["bias3"][0:1], want["bias_w"], "bias")
    assert_bitwise(after["vec_w"], want["vec_w"], "vec_w")
    # dead elements: the very bits they held
    for wk, nk, zk in (("lin_w", "lin_n", "lin_z"), ("vec_w", "vec_n", "vec_z")):
        dead = (bits(before[nk]) | bits(before[zk])) == 0
        assert np.array_equal(bits(after[wk])[dead], bits(before[wk])[dead]), wk + ": a dead element was written"
    # (n, z) untouched, bit for bit (NaN payloads included)
    for key in ("lin_n", "lin_z", "vec_n", "vec_z"):
        assert np.array_equal(bits(after[key]), bits(before[key])), key
    assert np.array_equal(bits(after["bias3"][1:]), bits(before["bias3"][1:]))
    derived = _counts_from(before, after)
    assert got == derived, (got, derived)
    assert got == want_cnt, (got, want_cnt)
    assert got["lin_live"] > 0 and (mt == "LR") == (got["lat_live"] == 0)
    if mt == "LR":
        assert got["lat_nonzero"] == 0 and got["lat_moved"] == 0
    # idempotence: a second pass moves nothing and leaves every w where it is
    again = e.refresh_weights()
    assert again["lin_moved"] == 0 and again["lat_moved"] == 0, again
    assert {k: again[k] for k in COUNT_KEYS if "moved" not in k} == {k: got[k] for k in COUNT_KEYS if "moved" not in k}
    twice = e.get_state()
    for key in twice:
        assert np.array_equal(bits(twice[key]), bits(after[key])), "second pass: " + key
    e.close()
    return got


@pytest.mark.parametrize("hp_name", HPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-%d-%dx%d" % s)
def test_every_element_follows_the_rule(shape, hp_name):
    """Tests 1 and 3 of the issue: elementwise against the oracle, counters, idempotence."""
    _check_refresh(shape, HP_SETS[hp_name], learn=False)


@pytest.mark.parametrize("hp_name", HPS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "LR"], ids=lambda s: "%s-%d-%dx%d" % s)
def test_learning_variant_keeps_slots_without_a_gradient(shape, hp_name):
    """FFM_FLAG_LEARN: latent elements whose n is not > 0 (n = 0 with z != 0, n = NaN) keep w_old; linear
    elements do not take the exception."""
    hp = HP_SETS[hp_name]
    e, before = _prepared_engine(shape, hp, True)
    n, z = before["vec_n"], before["vec_z"]
    kept = ((bits(n) | bits(z)) != 0) & ~(n > 0)
    assert (kept & (n == 0) & (z != 0)).any() and (kept & np.isnan(n)).any()
    lin_excepted = ((bits(before["lin_n"]) | bits(before["lin_z"])) != 0) & ~(before["lin_n"] > 0)
    assert lin_excepted.any()
    e.refresh_weights()
    after = e.get_state()
    assert np.array_equal(bits(after["vec_w"])[kept], bits(before["vec_w"])[kept])
    # a linear element with n = 0 and |z| > l1 moved all the same
    moved_lin = lin_excepted & (np.abs(before["lin_z"]) > np.float32(hp["w_l1"]))
    assert moved_lin.any() and (bits(after["lin_w"])[moved_lin] != bits(before["lin_w"])[moved_lin]).all()
    e.close()
    _check_refresh(shape, hp, learn=True)


# ---- blocks in which some features occur in one block only and some in all ----

N_BLOCKS, ROWS, COMMON, EXCL = 6, 64, 3, 40


def _make_blocks(mt, F, seed=5, n_blocks=N_BLOCKS):
    """n_blocks blocks of ROWS rows, one entry per column f < F.  Column f owns the ids [f * per, (f + 1) *
    per): COMMON ids that every block draws from, then EXCL ids per block that only this block draws from.
    Returns (blocks, n_feats, per)."""
    rng = np.random.default_rng(seed)
    per = COMMON + n_blocks * EXCL
    blocks = []
    for b in range(n_blocks):
        rows, labels = [], []
        for _ in range(ROWS):
            row = []
            for f in range(F):
                local = int(rng.integers(COMMON)) if rng.random() < 0.5 else COMMON + b * EXCL + int(rng.integers(EXCL))
                v = 1.0 if rng.random() < 0.5 else float(np.float32(rng.random() + 0.25))
                row.append((f if mt == "FFM" else 0, f * per + local, v))
            rows.append(row)
            labels.append(int(rng.random() < 0.4))
        blocks.append(Csr.from_rows(rows, labels))
    return blocks, F * per, per


MODELS = [("FFM", 4, 4), ("FM", 1, 5), ("LR", 1, 1)]


@pytest.mark.parametrize("learn", [False, True], ids=["reference", "learn"])
@pytest.mark.parametrize("model", MODELS, ids=lambda m: m[0])
def test_training_after_a_refresh_is_bit_identical(model, learn):
    mt, F, k = model
    blocks, nf, _ = _make_blocks(mt, 4)
    kw = dict(seed=9, learn=learn, max_batch_rows=ROWS, **STRESS_HP)
    a = fa.Engine(mt, nf, F, k, **kw)
    b = fa.Engine(mt, nf, F, k, **kw)
    la = lb = 0.0
    moved = 0
    for i, blk in enumerate(blocks):
        ga, sa = a.train_batch(blk)
        gb, sb = b.train_batch(blk)
        assert np.array_equal(bits(ga), bits(gb)), "logits of block %d" % i
        assert np.float64(sa).tobytes() == np.float64(sb).tobytes()
        la, lb = la + sa, lb + sb
        r = b.refresh_weights()
        moved += r["lin_moved"] + r["lat_moved"]
    assert np.float64(la).tobytes() == np.float64(lb).tobytes() and moved > 0
    sa, sb = a.get_state(), b.get_state()
    for key in ("lin_n", "lin_z", "vec_n", "vec_z"):
        assert np.array_equal(bits(sa[key]), bits(sb[key])), key
    assert np.array_equal(bits(sa["bias3"][1:]), bits(sb["bias3"][1:]))
    assert not np.array_equal(bits(sa["lin_w"]), bits(sb["lin_w"]))  # (only the stored weights differ)
    a.close()
    b.close()


@pytest.mark.parametrize("learn", [False, True], ids=["reference", "learn"])
@pytest.mark.parametrize("model", MODELS, ids=lambda m: m[0])
def test_refreshed_engine_predicts_what_the_refreshed_oracle_predicts(model, learn):
    """(Under the reference's rule the latent accumulators of FM / FFM never leave zero -- W(0, 0) = 0 makes
    every latent gradient zero --, so the latent part of this test is live in the learning variant.)"""
    mt, F, k = model
    blocks, nf, per = _make_blocks(mt, 4, n_blocks=N_BLOCKS + 1)
    train, held_out = blocks[:N_BLOCKS], blocks[N_BLOCKS]
    hp = STRESS_HP
    o = CpuModel("oracle", mt, nf, F, k, learn=learn, **hp)
    st = o.zero_state()
    rng = np.random.default_rng(2)
    for key in ("lin_w", "vec_w"):
        st[key][...] = rng.normal(0, 0.02, st[key].shape).astype(np.float32)
    o.set_state(st)
    e = fa.Engine(mt, nf, F, k, skip_init=True, learn=learn, max_batch_rows=ROWS, **hp)
    e.set_state(st)
    for blk in train:
        lo, _ = o.train_batch(blk)
        lg, _ = e.train_batch(blk)
        assert_bitwise(lg, lo, "training logits")
    # the held-out block reuses ids of the training blocks; a probe block scores, one row each, features
    # that occurred in exactly one training block
    ids = np.unique(np.concatenate([b.feat for b in train]))
    in_blocks = sum(np.isin(ids, b.feat).astype(np.int64) for b in train)
    single = ids[(in_blocks == 1)][:32]
    assert single.size == 32
    probe = Csr.from_rows([[(int(i // per) if mt == "FFM" else 0, int(i), 1.0)] for i in single], [0] * single.size)
    mix_rows = []
    for r in range(ROWS):
        lo_, hi_ = held_out.row_ptr[r], held_out.row_ptr[r + 1]
        row = [(int(held_out.field[p]), int(rng.choice(ids[ids // per == held_out.feat[p] // per])), float(held_out.val[p]))
               for p in range(lo_, hi_)]
        mix_rows.append(row)
    mixed = Csr.from_rows(mix_rows, held_out.label.tolist())
    stale_probe, _ = e.predict_batch(probe)
    stale_mixed, _ = e.predict_batch(mixed)
    # the oracle's weights from its accumulators, by the rule (numpy + set_state)
    so = o.get_state()
    for wk, nk, zk in (("lin_w", "lin_n", "lin_z"), ("vec_w", "vec_n", "vec_z")):
        w, n, z = so[wk].reshape(-1), so[nk].reshape(-1), so[zk].reshape(-1)
        for i in np.flatnonzero((bits(n) | bits(z)) != 0):
            if not (learn and wk == "vec_w" and not (n[i] > 0)):
                w[i] = o.maybe_zero_weight(float(n[i]), float(z[i]))
    so["bias3"][0] = o.maybe_zero_weight(float(so["bias3"][1]), float(so["bias3"][2]))
    o.set_state(so)
    r = e.refresh_weights()
    assert r["lin_moved"] > 0 and (r["lat_moved"] > 0) == (learn and mt != "LR")
    for blk, name in ((probe, "probe"), (mixed, "held-out")):
        pe, le = e.predict_batch(blk)
        po, lo = o.predict_batch(blk)
        assert_bitwise(pe, po, "predict after the refresh: " + name)  # (tests/test_gpu_parity.py's comparison)
        assert loss_close(le, lo)
    fresh_probe, _ = e.predict_batch(probe)
    fresh_mixed, _ = e.predict_batch(mixed)
    # without the refresh these rows were scored by create-time weights
    assert (bits(fresh_probe) != bits(stale_probe)).any()
    assert (bits(fresh_mixed) != bits(stale_mixed)).any()
    e.close()


def test_changed_feature_set_is_the_same_before_and_after():
    blocks, nf, _ = _make_blocks("FFM", 4)
    e = fa.Engine("FFM", nf, 4, 4, seed=11, learn=True, max_batch_rows=ROWS, **STRESS_HP)
    for blk in blocks[:2]:
        e.train_batch(blk)
    before = e.changed_features()
    assert 0 < before.size < nf
    r = e.refresh_weights()
    assert r["lin_moved"] > 0 and r["lat_moved"] > 0
    assert np.array_equal(e.changed_features(), before)
    e.close()


def test_staged_blocks_are_trained_first_and_keep_their_losses():
    blocks, nf, _ = _make_blocks("FFM", 4)
    kw = dict(seed=13, learn=True, max_batch_rows=ROWS, **STRESS_HP)
    s = fa.Engine("FFM", nf, 4, 4, **kw)
    want_loss = sum(s.train_batch(b)[1] for b in blocks[:2])
    want = s.refresh_weights()
    want_state = s.get_state()
    a = fa.Engine("FFM", nf, 4, 4, **kw)
    a.train_batch_async(blocks[0])
    a.train_batch_async(blocks[1])
    got = a.refresh_weights()  # (no flush before it)
    assert got == want and got["lat_moved"] > 0
    got_state = a.get_state()
    for key in want_state:
        assert np.array_equal(bits(got_state[key]), bits(want_state[key])), key
    assert loss_close(a.train_flush(), want_loss)
    s.close()
    a.close()


GF, GK, GPER = 8, 4, 3 + N_BLOCKS * EXCL


@pytest.mark.parametrize("n,compact", [(2, True), (4, True), (2, False)], ids=["2-compact", "4-compact", "2-full-length"])
def test_group_refresh_matches_the_unsharded_engine(n, compact):
    blocks, nf, per = _make_blocks("FFM", GF)
    assert per == GPER
    # (the learning variant: under the reference's rule no latent accumulator ever leaves zero)
    kw = dict(seed=21, learn=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * GF, **STRESS_HP)
    ref = fa.Engine("FFM", nf, GF, GK, **kw)
    for blk in blocks[:3]:
        ref.train_batch(blk)
    want_cnt = ref.refresh_weights()
    want = ref.get_state()
    ref.close()
    fs = (np.arange(GF + 1) * per).astype(np.int32) if compact else None
    g = fa.Group([0] * n, "FFM", nf, GF, GK, field_start=fs, **kw)
    for blk in blocks[:3]:
        g.train_batch(blk)
    ids = np.arange(nf, dtype=np.int32)
    pre = [e.get_rows(ids) for e in g.engines]
    got_cnt = g.refresh_weights()
    assert got_cnt == want_cnt, (got_cnt, want_cnt)
    assert got_cnt["lat_moved"] > 0 and got_cnt["lin_moved"] > 0
    plan = fa.shard_plan(GF, n, field_map=compact)
    fld = ids // per
    w_of = _rule(STRESS_HP)
    for r, e in enumerate(g.engines):
        rows = e.get_rows(ids)
        own = np.repeat(plan["pair_owner"][fld] == r, GK, axis=1)
        lin_own = plan["lin_owner"][fld] == r
        for wk, nk, zk, mask in (("vec_w", "vec_n", "vec_z", own), ("lin_w", "lin_n", "lin_z", lin_own)):
            assert np.array_equal(bits(rows[nk]), bits(pre[r][nk])) and np.array_equal(bits(rows[zk]), bits(pre[r][zk]))
            live = (bits(rows[nk]) | bits(rows[zk])) != 0
            assert not (live & ~mask).any(), "rank %d holds live %s it does not own" % (r, nk)
            # the shard's own accumulators decide its weights, exactly ...
            exp = pre[r][wk].copy()
            for i in zip(*np.nonzero(live)):
                if wk == "lin_w" or rows[nk][i] > 0:  # (the learning variant's exception)
                    exp[i] = w_of(rows[nk][i], rows[zk][i])
            assert_bitwise(rows[wk], exp, "rank %d %s by the rule" % (r, wk))
            # ... and they are the unsharded model's refreshed weights on the slots it owns (the cross-shard
            # logit sum has another association order: tests/test_gpu_group.py's bound)
            np.testing.assert_allclose(rows[wk][mask], want[wk][mask], rtol=2e-4, atol=2e-5, err_msg="rank %d %s" % (r, wk))
    # one rank alone: succeeds, and has nothing left to move
    alone = g.engines[0].refresh_weights()
    assert alone["lin_moved"] == 0 and alone["lat_moved"] == 0
    # pipelined blocks the group still holds are trained before the pass
    g.train_batch_async(blocks[3])
    moved = g.refresh_weights()
    assert moved["lat_moved"] > 0
    assert g.train_flush() > 0.0
    g.close()
