"""The exact arithmetic of the update and refresh kernels (ftrl_math.h, kernels_touch.h, kernels_fold.h)
against the oracle along the axis the other modules hold fixed: the hyper-parameters, which set the
create-time flags fast_div / fast_w, and the operands on and around the guards of the short square
root and the short x / alpha (sqrt_fast_ok, chain_operand_ok / fold_strict_ok, div_fast_ok), which
wave votes choose between.  util.HP_SETS reaches every state of the flags with both ends of both
ranges and the first float outside; util.range_grid puts n on every guard edge.

Every case compares logits and the whole state bit for bit, NaN positions included, and the loss
sum as the neighbouring modules do.  Every case also asserts, from the oracle alone, that it is not
empty: a cap on the share of non-finite logits and touched state words (a tenth; a quarter in the
hand-built cases, which also name the slots meant to go non-finite) and, with the numpy
restatements of the guards in util, operands on both sides of the guard it is about."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle import pyoracle
from oracle.pyoracle import CpuModel, Csr
from test_gpu_learn_variant import GRID_CASES
from util import (EDGE_COUNTS, FM_EDGE_COUNTS, HP_SETS, STATE_KEYS, arith_flags, assert_bitwise, assert_rank_rows,
                  assert_state_bitwise, bits, block_ids_per_field, chain_operand_ok, div_fast_ok, fast_state,
                  get_bias3, grid_block, grid_want, irregular_copy, keep_columns, kept_copy, occurrence_block,
                  range_grid, run_rank_staged, sqrt_fast_ok)

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = 6144  # the largest count (4097) in one field, every field with room for once-only ids
FM_ROWS, FM_COLS = 1024, 4


def _engine(*args, **kw):
    return fa.Engine(*args, **kw)


def _same_loss(sg, so, what):
    if np.isfinite(so):
        assert abs(sg - so) <= 1e-9 * max(1.0, abs(so)), (what, sg, so)
    else:  # (a saturated logit: log(0) or 0 * log(0) in the loss)
        assert (np.isnan(so) and np.isnan(sg)) or sg == so, (what, sg, so)


def train_both(o, e, blk, what):
    lo, so = o.train_batch(blk)
    lg, sg = e.train_batch(blk)
    assert_bitwise(lg, lo, what + " logits")
    _same_loss(sg, so, what)
    return lo


def predict_both(o, e, blk, what):
    lo, so = o.predict_batch(blk)
    lg, sg = e.predict_batch(blk)
    assert_bitwise(lg, lo, what + " predict")
    _same_loss(sg, so, what + " predict")
    return lo


def touched_words(st0, st1):
    """The state words a run changed, as one flat array of their final values."""
    return np.concatenate([st1[key].ravel()[bits(st1[key]).ravel() != bits(st0[key]).ravel()] for key in STATE_KEYS])


def assert_not_empty(logits, st0, st1, cap, what):
    """At most `cap` of the final logits and of the touched state words are non-finite."""
    bad = int((~np.isfinite(logits)).sum())
    assert bad <= cap * logits.size, "%s: %d of %d logits non-finite" % (what, bad, logits.size)
    t = touched_words(st0, st1)
    assert t.size > 0, what + ": nothing touched"
    bad = int((~np.isfinite(t)).sum())
    assert bad <= cap * t.size, "%s: %d of %d touched state words non-finite" % (what, bad, t.size)


# ---- a. the hyper-parameter grid -----------------------------------------------------------------
# Start states with n bounded further away from 0: sets in which W(n, z) of a slot with small n is large
# (l2 = 0 with beta = 0), and alpha = 3e-38, where a root difference above 10 overflows the step
# (sqrt(n + sum g*g) - sqrt(n)) / alpha of a feature a block holds 4097 times
N_ADD = {"l2_zero_beta_zero": 0.5, "all_zero": 0.5, "alpha_3e-38": 1e5}
# every entry runs FFM k = 8 (one launch), FM k = 8 and LR; the rest rotate over the entries
EXTRAS = ("ffm_k4", "ffm_k16", "ffm_k32", "ffm_k6_generic", "ffm_three_launches", "ffm_irregular", "fm_k128",
          "ffm_eight_shards")
HP_NAMES = list(HP_SETS)


def _warm(o, seed, name):
    st = fast_state(np.random.default_rng(seed), o, n_add=N_ADD.get(name, 0.05))
    st["bias3"][1] += f32(N_ADD.get(name, 0.0))  # (the bias is touched by every row of the block)
    return st


def _chain(o, e, st, blocks, test_blk, what):
    """Two chained blocks (the second consumes w refreshed from state the first wrote), then predict."""
    o.set_state(st)
    e.set_state(st)
    for b, blk in enumerate(blocks):
        train_both(o, e, blk, "%s block %d" % (what, b))
        assert_state_bitwise(e.get_state(), o.get_state(), "%s block %d" % (what, b))
    so = o.get_state()
    lo = predict_both(o, e, test_blk, what)
    assert_state_bitwise(e.get_state(), o.get_state(), what + " after predict")
    assert_not_empty(lo, st, so, 0.10, what)


def _ffm_chain(name, k, seed, monkeypatch, split="0", irregular=False):
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    hp, F = HP_SETS[name], 8
    per = block_ids_per_field(ROWS)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **hp)
    st = _warm(o, seed, name)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    e = _engine("FFM", nf, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, max_row_nnz=F,
                field_start=fs, **hp)
    blocks = [occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed + s)[0] for s in range(3)]
    if irregular:
        blocks = [irregular_copy(b, seed=seed) for b in blocks]
    _chain(o, e, st, blocks[:2], blocks[2], "%s FFM k=%d split=%s irregular=%s" % (name, k, split, irregular))
    e.close()


def _fm_chain(name, k, seed):
    hp = HP_SETS[name]
    per = block_ids_per_field(FM_ROWS)
    nf = FM_COLS * per
    o = CpuModel("oracle", "FM", nf, 1, k, **hp)
    st = _warm(o, seed, name)
    e = _engine("FM", nf, 1, k, skip_init=True, max_batch_rows=FM_ROWS, max_row_nnz=FM_COLS, **hp)
    blocks = [occurrence_block(FM_COLS, FM_EDGE_COUNTS, FM_ROWS, seed=seed + s)[0] for s in range(3)]
    for blk in blocks:
        blk.field[:] = 0  # libsvm rows
    _chain(o, e, st, blocks[:2], blocks[2], "%s FM k=%d" % (name, k))
    e.close()


def _lr_chain(name, seed):
    hp = HP_SETS[name]
    per = block_ids_per_field(FM_ROWS)
    nf = FM_COLS * per
    o = CpuModel("oracle", "LR", nf, 1, 1, **hp)
    st = _warm(o, seed, name)
    e = _engine("LR", nf, 1, 1, skip_init=True, max_batch_rows=FM_ROWS, max_row_nnz=FM_COLS, **hp)
    blocks = [occurrence_block(FM_COLS, FM_EDGE_COUNTS, FM_ROWS, seed=seed + s)[0] for s in range(3)]
    for blk in blocks:
        blk.field[:] = 0
    _chain(o, e, st, blocks[:2], blocks[2], "%s LR" % name)
    e.close()


def _shards_chain(name, seed):
    """Eight compact shards of F = 8, k = 8 (kept columns, staged ahead, the oracle's logits in place
    of the all-reduce), two chained blocks."""
    hp, F, k, S = HP_SETS[name], 8, 8, 8
    per = block_ids_per_field(ROWS)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **hp)
    st = _warm(o, seed, name)
    o.set_state(st)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    plan = fa.shard_plan(F, S, field_map=True)
    blocks = [occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed + s)[0] for s in range(2)]
    logits = [o.train_batch(b)[0] for b in blocks]
    so = o.get_state()
    assert_not_empty(logits[-1], st, so, 0.10, name + " shards")
    ids = np.arange(nf, dtype=np.int32)
    total = [np.zeros(ROWS, np.float64) for _ in blocks]
    for r in range(S):
        e = _engine("FFM", nf, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F, n_shards=S,
                    shard_rank=r, max_row_nnz=F, field_start=fs, **hp)
        e.set_state(st)
        keep = keep_columns(plan, r)
        for i, p in enumerate(run_rank_staged(e, [kept_copy(b, keep) for b in blocks], logits)):
            total[i] += p
        assert_rank_rows(e, r, ids, ids // per, so, plan, k, name + " shards")
        if r == plan["bias_owner"]:
            assert_bitwise(get_bias3(e), so["bias3"], "bias3")
        e.close()
    for i in range(len(blocks)):
        scale = float(np.abs(logits[i]).max())
        np.testing.assert_allclose(total[i].astype(np.float32), logits[i], rtol=1e-5, atol=2e-6 * max(1.0, scale))


def test_rotation_gives_every_shape_two_states_of_the_flags():
    for j, extra in enumerate(EXTRAS):
        states = {arith_flags(HP_SETS[n]) for i, n in enumerate(HP_NAMES) if i % len(EXTRAS) == j}
        assert len(states) >= 2, (extra, states)


@pytest.mark.parametrize("name", HP_NAMES)
def test_hyper_parameter_grid(name, monkeypatch):
    """FFM k = 8 with field_start as one launch, FM k = 8, LR, and one more shape in rotation: two
    chained blocks over every edge occurrence count from warm state, then predict_batch."""
    i = HP_NAMES.index(name)
    seed = 1000 + 10 * i
    _ffm_chain(name, 8, seed, monkeypatch)
    _fm_chain(name, 8, seed + 3)
    _lr_chain(name, seed + 6)
    extra = EXTRAS[i % len(EXTRAS)]
    if extra == "ffm_k4":
        _ffm_chain(name, 4, seed + 1, monkeypatch)
    elif extra == "ffm_k16":
        _ffm_chain(name, 16, seed + 1, monkeypatch)
    elif extra == "ffm_k32":
        _ffm_chain(name, 32, seed + 1, monkeypatch)
    elif extra == "ffm_k6_generic":
        _ffm_chain(name, 6, seed + 1, monkeypatch)
    elif extra == "ffm_three_launches":
        _ffm_chain(name, 8, seed + 1, monkeypatch, split="2")
    elif extra == "ffm_irregular":
        _ffm_chain(name, 8, seed + 1, monkeypatch, irregular=True)
    elif extra == "fm_k128":
        _fm_chain(name, 128, seed + 1)
    else:
        _shards_chain(name, seed + 1)


# ---- a'. a feature twice in one row: the row-order walk ---------------------------------------------
@pytest.mark.parametrize("mt,k", [("LR", 1), ("FM", 8), ("FFM", 4)], ids=["LR", "FM_k8", "FFM_k4"])
@pytest.mark.parametrize("name", ["stress_hp", "beta_zero", "alpha_below_2m30", "l1_zero", "alpha_0.3"])
def test_feature_twice_in_a_row_is_walked_touch_by_touch(name, mt, k):
    """An accumulator that ONE row touches twice is not folded: it takes its touches one by one in row
    order, z + (g - s*w) and (z + g) - s*w as the reference writes them (nz_step_linear_carry,
    nz_step_latent_carry).  LR and FM: an id that repeats inside a row -- one in every row (hot), one in
    four rows (few).  FFM, where the reference deadlocks on a repeated id and so defines no bits: the same
    entries under distinct ids, field 0 holding three or five values per row, so that every other
    field's slot for field 0 is touched several times by one row.  Two chained blocks, then predict."""
    hp = HP_SETS[name]
    F, per, n_rows = (4, 40, 256) if mt == "FFM" else (1, 160, 256)
    nf = F * per
    o = CpuModel("oracle", mt, nf, F, k, **hp)
    st = _warm(o, 3000, name)
    rng = np.random.default_rng(3001)
    second = 1 if mt == "FFM" else 0  # (FFM: ids 0 and 1 of field 0; LR, FM: id 0 twice)

    def block():
        rows = []
        for r in range(n_rows):
            row = [(f if mt == "FFM" else 0, (f if mt == "FFM" else 0) * per + 4 + int(rng.integers(0, per - 4)),
                    float(f32(rng.random() + 0.25))) for f in range(4)]
            row.insert(int(rng.integers(0, 5)), (0, 0, float(f32(rng.random() + 0.25))))
            row.append((0, second, 0.5))
            if r % 64 == 5:
                row += [(0, 2, 1.0), (0, 2 + second, float(f32(rng.random() + 0.25)))]
            rows.append(row)
        return Csr.from_rows(rows, list(rng.integers(0, 2, n_rows)))
    blocks = [block() for _ in range(3)]
    assert np.bincount(blocks[0].feat)[:4].tolist() == ([n_rows, n_rows, 4, 4] if mt == "FFM" else [2 * n_rows, 0, 8, 0])
    e = _engine(mt, nf, F, k, skip_init=True, max_batch_rows=n_rows, max_row_nnz=8, **hp)
    _chain(o, e, st, blocks[:2], blocks[2], "%s %s twice in a row" % (name, mt))
    e.close()


# ---- b. the guard edges at every refresh site ----------------------------------------------------
# one set per state of (fast_div, fast_w); each keeps l2 + (beta + sqrt(n)) / alpha >= 1, so that W of
# z = +-2^61 stays below 2^61 and a pair of such weights does not overflow the logit
FLAG_SETS = {(1, 1): "stress_hp", (1, 0): "beta_1.4e-38", (0, 0): "alpha_below_2m30"}


@pytest.mark.parametrize("learn", [False, True], ids=["reference", "learn"])
@pytest.mark.parametrize("flags", list(FLAG_SETS), ids=["div%d_w%d" % f for f in FLAG_SETS])
@pytest.mark.parametrize("occurrences", [1, 2], ids=["in_row_refresh", "refresh_kernel"])
@pytest.mark.parametrize("mt,k,env", GRID_CASES,
                         ids=["%s_k%d%s" % (m, k, "".join("_%s=%s" % kv for kv in env.items()))
                              for m, k, env in GRID_CASES])
def test_guard_edges_at_every_refresh_site(mt, k, env, occurrences, flags, learn, monkeypatch):
    """util.range_grid injected as latent and linear accumulators and touched once (the row kernel
    refreshes and updates) or twice (the refresh kernel, the few-occurrence folds): the stored w against
    the oracle and against util.grid_want, and n, z after the touch against the oracle -- the edges pass
    through nz_step_*, ffm_touch_n and fold_root_diffs as well as through W(n, z)."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    hp = HP_SETS[FLAG_SETS[flags]]
    assert arith_flags(hp) == flags
    g = grid_block(mt, k, hp, occurrences, grid=range_grid(hp))
    n = g["n"]
    with np.errstate(all="ignore"):
        operand = (f32(hp["w_beta"]) + np.sqrt(n)).astype(f32)
    for guard, x in ((sqrt_fast_ok, n), (chain_operand_ok, n), (div_fast_ok, operand)):
        assert guard(x).any() and not guard(x).all(), guard.__name__
    what = "%s k=%d %s occ=%d %s learn=%s" % (mt, k, env, occurrences, FLAG_SETS[flags], learn)
    o = CpuModel("oracle", mt, g["nf"], g["F"], k, learn=learn, **hp)
    o.set_state(g["state"])
    e = _engine(mt, g["nf"], g["F"], k, skip_init=True, max_batch_rows=g["block"].n_rows, max_row_nnz=2,
                field_start=g["field_start"], learn=learn, **hp)
    e.set_state(g["state"])
    lo = train_both(o, e, g["block"], what)
    got, so = e.get_state(), o.get_state()
    assert_state_bitwise(got, so, what)
    want, want_lin = grid_want(g, hp, learn)
    assert_bitwise(got["vec_w"][g["slots"]], want, "latent w = the rule")
    assert_bitwise(got["lin_w"][g["lin"]], want_lin, "linear w = W(n, z)")
    assert (bits(so["vec_n"][g["slots"]]) != bits(n[g["idx"]])).any(), "the touch moved n"
    assert_not_empty(lo, g["state"], so, 0.10, what)
    e.close()


# ---- c. one discriminating operand per guard and flag --------------------------------------------
# (hyper-parameters, n of the chosen accumulators, their z): the divide operand beta + sqrt(n) is one for
# which the unguarded short divide gives other bits than x / alpha (tests/test_block_semantics.py:
# DIV_DISCRIMINATORS proves it on the CPU for the same three operands)
DISCRIMINATORS = dict(
    # under div_fast_ok's 2^-60, fast_div = 1, fast_w = 0; l1 = l2 = 0 so that the quotient's last bit
    # is not absorbed by l2 and W = -z / (beta / alpha) of a tiny z is an ordinary number
    below_2m60=(dict(w_alpha=float(f32(1e-4)), w_beta=float(f32(1.4e-38)), w_l1=0.0, w_l2=0.0), 0.0, 1.7e-33,
                float(f32(1.4e-38))),
    # alpha outside [2^-30, 2^30] (fast_div = 0): sqrt(2^118) = 2^59 is inside div_fast_ok, x * (1 / alpha)
    # overflows and the short form gives NaN where x / alpha is inf and W = -0
    alpha_out_of_range=(HP_SETS["alpha_3e-38"], 2.0 ** 118, 0.37, 2.0 ** 59),
    # over div_fast_ok's 2^60 through beta (a square root alone never exceeds 2^64, which an alpha in
    # range does not overflow): fast_div = 1, fast_w = 0, the short form NaN, x / alpha inf, W = -0
    above_2p60=(dict(w_alpha=2.0 ** -30, w_beta=2.0 ** 100, w_l1=0.01, w_l2=0.1), 0.5, 0.37, 2.0 ** 100))


@pytest.mark.parametrize("mt,k", [("FFM", 4), ("FFM", 6), ("FM", 8), ("LR", 1)], ids=["FFM_k4", "FFM_k6", "FM_k8", "LR"])
@pytest.mark.parametrize("case", list(DISCRIMINATORS))
def test_discriminating_operand(case, mt, k):
    """A small block in which a linear term, a latent slot (FFM, FM) and the bias hold the n whose
    divide operand beta + sqrt(n) the short divide gets wrong: the engine must take the IEEE divide
    there, through the flag or the wave vote, although the other lanes of the wave hold ordinary n."""
    hp, n_x, z_x, operand = DISCRIMINATORS[case]
    alpha, beta, l1, l2 = (f32(hp[key]) for key in ("w_alpha", "w_beta", "w_l1", "w_l2"))
    F, per, n_rows = (2, 16, 64) if mt == "FFM" else (1, 32, 64)
    nf = F * per
    o = CpuModel("oracle", mt, nf, F, k, **hp)
    rng = np.random.default_rng(5)
    st = fast_state(rng, o, n_add=0.05)
    chosen = np.arange(0, nf, 3)  # every third feature: its linear term and all its latent slots
    for key in ("lin", "vec"):
        st[key + "_n"][chosen] = f32(n_x)
        st[key + "_z"][chosen] = (f32(z_x) * rng.choice([-1.0, 1.0], st[key + "_z"][chosen].shape)).astype(f32)
    st["bias3"][1:] = f32(n_x), f32(z_x)
    st["vec_z"][...] = -np.abs(st["vec_z"])  # every latent w >= 0: ffm.cpp:118's root stays real, n = 0 included
    if mt == "FFM":
        rows = [[(0, int(rng.integers(0, per)), 1.0), (1, per + int(rng.integers(0, per)), float(f32(rng.random() + 0.25)))]
                for _ in range(n_rows)]
    else:
        rows = [[(0, int(i), float(f32(rng.random() + 0.25))) for i in rng.choice(nf, 3, replace=False)]
                for _ in range(n_rows)]
    blk = Csr.from_rows(rows, list(rng.integers(0, 2, n_rows)))
    assert np.isin(chosen, blk.feat).sum() >= 4 and (~np.isin(blk.feat, chosen)).sum() >= 4
    # the operand the block produces, from the state: not covered by the guards, and other bits
    with np.errstate(all="ignore"):
        x = f32(beta + np.sqrt(f32(n_x)))
    assert x == f32(operand) and beta + np.sqrt(st["bias3"][1]) == x and beta + np.sqrt(st["lin_n"][chosen[0]]) == x
    assert not (arith_flags(hp)[0] and div_fast_ok(x)), "the operand lies outside the guards"
    assert arith_flags(hp)[1] == 0
    quick, exact = pyoracle.div_alpha_fast(alpha, np.array([x], f32))
    assert bits(quick)[0] != bits(exact)[0]
    e = _engine(mt, nf, F, k, skip_init=True, max_batch_rows=n_rows, max_row_nnz=3, **hp)
    what = "%s %s k=%d" % (case, mt, k)
    o.set_state(st)
    e.set_state(st)
    lo = train_both(o, e, blk, what)
    so = o.get_state()
    assert_state_bitwise(e.get_state(), so, what)
    # ... and the stored weights depend on it: W with the short quotient is another float
    with np.errstate(all="ignore"):
        for w, z in [(so["bias3"][0], st["bias3"][2])] + [(so["lin_w"][i], st["lin_z"][i]) for i in chosen
                                                          if i in blk.feat]:
            assert abs(z) > l1
            num = f32(z - f32((f32(1) if z > 0 else f32(-1)) * l1))
            w_exact = f32(np.float64(-1.0) * np.float64(num) / np.float64(f32(l2 + exact[0])))
            w_quick = f32(np.float64(-1.0) * np.float64(num) / np.float64(f32(l2 + quick[0])))
            assert bits(w)[()] == bits(w_exact)[()] and np.isfinite(w)
            assert bits(w_quick)[()] != bits(w_exact)[()], (w_quick, w_exact)
    lp = predict_both(o, e, blk, what)
    # nothing is meant to go non-finite here, and nothing does
    assert np.isfinite(lo).all() and np.isfinite(lp).all() and all(np.isfinite(v).all() for v in so.values()), what
    assert_not_empty(lp, st, so, 0.25, what)
    e.close()


@pytest.mark.parametrize("k", [4, 16])
def test_touch_step_that_overflows_with_alpha_out_of_range(k):
    """alpha = 3e-38 (fast_div = 0) in the per-touch step of once-only FFM features (ffm_touch_n): every
    square-root operand is comfortably normal, so only the flag keeps the short divide out.  One row
    in eight holds x = 2^70 against latent z = -2^61 (w about 3e-20, g about 20): the root difference,
    about 17, divided by alpha overflows -- x / alpha is inf where the short form's x * (1 / alpha) gives
    NaN -- and z of the pair's first slot ends at +-inf.  Named non-finite words: those rows' features'
    linear n (g*g overflows) and z, and the z of the two latent slots the pair touches."""
    hp, P = HP_SETS["alpha_3e-38"], 64
    assert arith_flags(hp) == (0, 0)
    nf = 2 * P
    o = CpuModel("oracle", "FFM", nf, 2, k, **hp)
    rng = np.random.default_rng(41)
    st = fast_state(rng, o, n_add=1.0)
    st["vec_z"][...] = -np.abs(st["vec_z"])  # every w >= 0: ffm.cpp:118's operand n + g2*g1 stays in range too,
    big = np.arange(0, P, 8)                 # so that no lane of a wave votes the short forms down
    first, second = (big[:, None], k + np.arange(k)[None, :]), (P + big[:, None], np.arange(k)[None, :])
    for sl in (first, second):
        st["vec_z"][sl] = f32(-(2.0 ** 61))
    assert chain_operand_ok(st["vec_n"]).all() and chain_operand_ok(st["vec_n"] + f32(450)).all()
    rows = [[(0, r, float(2.0 ** 70) if r in big else float(f32(rng.random() + 0.25))), (1, P + r, 1.0)] for r in range(P)]
    blk = Csr.from_rows(rows, list(rng.integers(0, 2, P)))
    fs = np.array([0, P, nf], np.int32)
    e = _engine("FFM", nf, 2, k, skip_init=True, max_batch_rows=P, max_row_nnz=2, field_start=fs, **hp)
    what = "alpha 3e-38 overflowing touch k=%d" % k
    o.set_state(st)
    e.set_state(st)
    train_both(o, e, blk, what)
    so = o.get_state()
    assert_state_bitwise(e.get_state(), so, what)
    assert np.isinf(so["vec_z"][first]).all(), "the first slot's step (root difference / alpha) overflowed to inf"
    d = np.sqrt(so["vec_n"][first]) - np.sqrt(st["vec_n"][first])
    quick, exact = pyoracle.div_alpha_fast(hp["w_alpha"], d.ravel())
    assert np.isinf(exact).all() and np.isnan(quick).all() and div_fast_ok(d).all()
    named = {key: np.zeros(so[key].shape, bool) for key in STATE_KEYS}
    named["lin_n"][big] = named["lin_z"][big] = True
    named["vec_z"][first] = named["vec_z"][second] = True
    assert np.isinf(so["lin_n"][big]).all() and not np.isfinite(so["vec_z"][second]).any()
    for key in STATE_KEYS:
        assert np.isfinite(so[key][~named[key]]).all(), key
    lp = predict_both(o, e, blk, what)
    assert_not_empty(lp, st, so, 0.25, what)
    e.close()


# ---- d. mixed waves --------------------------------------------------------------------------------
EDGE_N = np.array([np.nextafter(f32(2.0 ** -96), f32(0)), 2.0 ** -96, np.nextafter(f32(2.0 ** -70), f32(0)), 2.0 ** -70,
                   2.0 ** 96, np.nextafter(f32(2.0 ** 96), f32(np.inf)), 2.0 ** 118], f32)


def _mixed_state(o, seed, kind, l1):
    """Warm state whose latent and linear n alternate, factor by factor and feature by feature, between
    ordinary values and guard edges (kind "mixed"), or hold only the one or the other.  Every z lies
    below -l1, so every w is positive and ffm.cpp:118's root stays real."""
    rng = np.random.default_rng(seed)
    st = fast_state(rng, o, n_add=0.05)
    for key in ("lin_z", "vec_z"):
        st[key][...] = -(np.abs(st[key]) + f32(2 * l1 + 0.01))
    for key in ("lin_n", "vec_n"):
        a = st[key]
        if a.size == 0:
            continue
        col = np.arange(a.shape[1] if a.ndim == 2 else 1)[None, :]
        row = np.arange(a.shape[0])[:, None]
        edge = ((row + col) % 2 == 1) if kind == "mixed" else np.full((a.shape[0], col.size), kind == "edges")
        vals = EDGE_N[(3 * row + col) % EDGE_N.size]
        a[...] = np.where(edge, vals, a.reshape(a.shape[0], -1)).reshape(a.shape)
    return st


def _mixed_case(mt, F, k, n_rows, counts, split, monkeypatch, seed):
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    hp = HP_SETS["stress_hp"]
    assert arith_flags(hp) == (1, 1)
    per = block_ids_per_field(n_rows)
    cols = F if mt == "FFM" else FM_COLS
    nf = cols * per
    o = CpuModel("oracle", mt, nf, F, k, **hp)
    fs = (np.arange(F + 1) * per).astype(np.int32) if mt == "FFM" else None
    e = _engine(mt, nf, F, k, skip_init=True, max_batch_rows=n_rows, max_batch_nnz=n_rows * cols, max_row_nnz=cols,
                field_start=fs, **hp)
    blocks = [occurrence_block(cols, counts, n_rows, seed=seed + s)[0] for s in range(2)]
    if mt != "FFM":
        for blk in blocks:
            blk.field[:] = 0
    for kind in ("mixed", "ordinary", "edges"):
        st = _mixed_state(o, seed, kind, hp["w_l1"])
        windows = st["vec_n"][np.unique(blocks[0].feat)].reshape(-1, 64)
        for guard in (chain_operand_ok, sqrt_fast_ok):
            ok = guard(windows)
            if kind == "mixed":  # both kinds inside every window of 64 consecutive factors
                assert (ok.any(axis=1) & ~ok.all(axis=1)).all(), guard.__name__
            elif kind == "ordinary":
                assert ok.all()
            else:
                assert not ok.all(axis=1).any()
        what = "mixed waves %s k=%d split=%s %s" % (mt, k, split, kind)
        o.set_state(st)
        e.set_state(st)
        train_both(o, e, blocks[0], what)
        so = o.get_state()
        assert_state_bitwise(e.get_state(), so, what)
        lo = predict_both(o, e, blocks[1], what)
        assert_state_bitwise(e.get_state(), o.get_state(), what + " after predict")
        assert_not_empty(lo, st, so, 0.10, what)
    e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
def test_mixed_waves_ffm(split, monkeypatch):
    """FFM F = 8, k = 16 over every edge occurrence count: guard-edge and ordinary n alternate inside
    every 64 consecutive factors (the lanes of one vote), from one feature to the next (the partners of
    consecutive touches of one slot, gathered four at a time) and between a feature's linear term and
    its neighbours'; then the two uniform halves, which take one side of every vote."""
    _mixed_case("FFM", 8, 16, ROWS, EDGE_COUNTS, split, monkeypatch, seed=2100)


def test_mixed_waves_fm(monkeypatch):
    """FM k = 64: one feature's factors are one wave."""
    _mixed_case("FM", 1, 64, FM_ROWS, FM_EDGE_COUNTS, "0", monkeypatch, seed=2200)


# ---- e. feature values -----------------------------------------------------------------------------
VALUE_CLASSES = ("ordinary", "negative", "plus_one", "minus_one", "subnormal", "two_m40", "two_p20", "two_p40",
                 "negative_two_p40", "two_p60")


def _class_value(c, rng):
    return {"ordinary": f32(rng.random() + 0.25), "negative": f32(-(rng.random() + 0.25)), "plus_one": f32(1.0),
            "minus_one": f32(-1.0), "subnormal": f32(1e-40), "two_m40": f32(2.0 ** -40), "two_p20": f32(2.0 ** 20),
            "two_p40": f32(2.0 ** 40), "negative_two_p40": f32(-(2.0 ** 40)), "two_p60": f32(2.0 ** 60)}[VALUE_CLASSES[c]]


def _value_block(cols, counts, n_rows, seed):
    """util.occurrence_block with feature values of every class (feature_classes); row r carries ONE value of a class, in its entry of column r mod cols (the
    class of that entry's feature), every other entry of the row keeps its ordinary value in
    [0.25, 1.25] -- so a row's pair terms hold at most one extreme factor and stay finite, and a
    feature has its class's value in the rows that single it out, once-only, few, hot and giant
    features alike.  Returns (block, ids, the mask of the singled-out entries)."""
    blk, ids, _ = occurrence_block(cols, counts, n_rows, seed=seed)
    rng = np.random.default_rng(seed)
    val = blk.val.reshape(n_rows, cols)
    feat = blk.feat.reshape(n_rows, cols)
    mask = np.zeros((n_rows, cols), bool)
    mask[np.arange(n_rows), np.arange(n_rows) % cols] = True
    cls = feature_classes(ids)
    for r in range(n_rows):
        c = r % cols
        val[r, c] = _class_value(cls(int(feat[r, c])), rng)
    return blk, ids, mask.reshape(-1)


def feature_classes(ids):
    """A feature's class of value: its place in the list of edge counts for the listed features (so that
    every class meets few, hot and giant ones), its id for the once-only rest."""
    listed = {int(i): j % len(VALUE_CLASSES) for j, i in enumerate(ids)}
    return lambda i: listed.get(i, i % len(VALUE_CLASSES))


def _values_case(mt, F, k, n_rows, counts, classes, seed, monkeypatch):
    hp = HP_SETS["stress_hp"]
    cols = F if mt == "FFM" else FM_COLS
    per = block_ids_per_field(n_rows)
    nf = cols * per
    o = CpuModel("oracle", mt, nf, F, k, **hp)
    st = fast_state(np.random.default_rng(seed), o, n_add=0.05)
    blocks = [_value_block(cols, counts, n_rows, seed + s) for s in range(2)]
    blk, ids, mask = blocks[0]
    # the named handful: the (at most three) features of the 2^60 class that eight rows or more single
    # out start at n = FLT_MAX, where n + g*g (g = tmp_grad * 2^60, or * w * 2^60, in a row whose
    # saturated sigmoid does not equal its label) overflows to inf: the linear term, and latent slots
    ids60, n60 = np.unique(blk.feat[mask & (blk.val == f32(2.0 ** 60))], return_counts=True)
    huge = ids60[n60 >= 8][:3]
    assert huge.size >= 1
    st["lin_n"][huge] = np.finfo(f32).max
    if st["vec_n"].size:
        st["vec_n"][huge] = np.finfo(f32).max
    if mt != "FFM":
        for b, _, _ in blocks:
            b.field[:] = 0
    # every class of value reaches every class of feature
    cnt = dict(zip(*np.unique(blk.feat, return_counts=True)))
    cls = feature_classes(ids)
    seen = {(name, VALUE_CLASSES[cls(int(i))]) for i in blk.feat[mask]
            for name, (lo, hi) in classes.items() if lo <= cnt[i] <= hi}
    for name in classes:
        got = {v for n_, v in seen if n_ == name}
        assert len(got) >= (len(VALUE_CLASSES) if name == "once" else 2), (name, got)
    assert {"subnormal", "two_p40", "negative_two_p40", "minus_one"} <= {v for _, v in seen}
    fs = (np.arange(F + 1) * per).astype(np.int32) if mt == "FFM" else None
    e = _engine(mt, nf, F, k, skip_init=True, max_batch_rows=n_rows, max_batch_nnz=n_rows * cols, max_row_nnz=cols,
                field_start=fs, **hp)
    what = "values %s k=%d" % (mt, k)
    o.set_state(st)
    e.set_state(st)
    train_both(o, e, blk, what)
    so = o.get_state()
    assert_state_bitwise(e.get_state(), so, what)
    # the overflow happened in the named slots and nowhere else
    assert np.isinf(so["lin_n"][huge]).all(), "n + g*g overflows in the named linear terms"
    rest = np.ones(nf, bool)
    rest[huge] = False
    assert np.isfinite(so["lin_n"][rest]).all() and np.isfinite(so["lin_z"][rest]).all()
    if st["vec_n"].size:
        assert np.isinf(so["vec_n"][huge]).any(), "n + g*g overflows in the named latent slots"
        assert np.isfinite(so["vec_n"][rest]).all()
    # predict on the second block, the named features' entries moved to their column's last id (their
    # z is inf or NaN now, and so is their refreshed w)
    test_blk = blocks[1][0]
    sel = np.isin(test_blk.feat, huge)
    test_blk.feat[sel] = (test_blk.feat[sel] // per) * per + per - 1
    lo = predict_both(o, e, test_blk, what)
    assert_state_bitwise(e.get_state(), o.get_state(), what + " after predict")
    assert_not_empty(lo, st, so, 0.25, what)
    e.close()


def test_feature_values_ffm(monkeypatch):
    """FFM F = 8, k = 8: negative, subnormal, 2^-40 ... 2^40 and exactly +-1 feature values on once-only,
    few, hot and giant features."""
    _values_case("FFM", 8, 8, ROWS, EDGE_COUNTS, dict(once=(1, 1), few=(2, 10), hot=(11, 256), giant=(257, 1 << 30)),
                 2300, monkeypatch)


@pytest.mark.parametrize("mt,k", [("FM", 8), ("LR", 1)])
def test_feature_values_fm_lr(mt, k, monkeypatch):
    _values_case(mt, 1, k, FM_ROWS, FM_EDGE_COUNTS, dict(once=(1, 1), few=(2, 10), hot=(11, 64), giant=(65, 1 << 30)),
                 2400, monkeypatch)
