"""The FFM row kernel's held (n, z) (csrc/kernels_row.h, HOLD): the first HOLD 16-byte vectors each
thread refreshes of the row's once-only records stay in registers through the pair phase, and the
in-row update takes them from there instead of loading them again; vectors beyond HOLD * threads take
the re-read path.  FFM_ROW_HOLD (read when the engine is created) replaces the launcher's choice:
0 = the kernel that holds nothing, n = the smallest instantiated count (2, 4, 6, 8) that covers n.
Same operands, same order: logits, loss and the whole state (w, n, z) must be the oracle's bits for
FFM_ROW_HOLD 0, the default and every instantiated count, at 64 and 256 threads per row.

Blocks of 64 rows in which row r has a chosen number s of once-only features: ids that occur nowhere
else in its first s fields, ids shared with other rows in the rest.  s is chosen per shape so that a
row's once-only vectors fall just under, (where the sizes allow) exactly on and just over HOLD *
threads, next to s = 0, s = 1 and every entry once-only, all in one block together with a row that
misses a field and a row that carries a field twice (the update's loop over several partners).

  39 x 16, 152 vectors per record: s = 3 / 4 around 512 (HOLD 8 at 64 threads), 13 / 14 around 2048
           (HOLD 8 at 256 threads), 26 (beyond every hold at 64 threads)
  8 x 16,  28 vectors: with FFM_ROW_HOLD=2 at 64 threads (128 vectors) s = 4 / 5 straddle it and the 224
           vectors of a row whose 8 entries are all once-only lie beyond it
  16 x 4,  16 vectors: s = 7 / 8 / 9 under, exactly on and over 128 (HOLD 2 at 64 threads)
  39 x 8,  78 vectors: s = 6 / 7 around 512, 26 / 27 around 2048
  8 x 32,  64 vectors: s = 7 / 8: under and exactly on 512 (HOLD 8 at 64, HOLD 2 at 256 threads)
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from test_block_semantics import numpy_block
from util import DEFAULT_HP, STRESS_HP, assert_bitwise, assert_state_bitwise, fast_state, loss_close

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = 64
PER = 128  # ids per field: [0, 32) shared by rows, [32, 96) row r's own, [96, 128) the irregular rows' extras
SHAPES = {(39, 16): (0, 0, 1, 3, 4, 13, 14, 39, 26), (8, 16): (0, 0, 1, 4, 5, 8, 3), (16, 4): (0, 0, 1, 7, 8, 9, 16),
          (39, 8): (0, 0, 1, 6, 7, 26, 27, 39), (8, 32): (0, 0, 1, 7, 8, 4)}
# warm: |z| on both sides of l1; cold: n near 0 and a fifth of vec_n zero, so that ffm.cpp:118's square roots of
# negative numbers (NaN) pass through held vectors
STATES = {"warm_default_hp": (DEFAULT_HP, dict(n_add=0.05)), "warm_stress_hp": (STRESS_HP, dict(n_add=0.05)),
          "cold_stress_hp": (STRESS_HP, dict(n_hi=0.02, n_zero=0.2)), "cold_default_hp": (DEFAULT_HP, dict(n_hi=0.02, n_zero=0.2))}
HOLDS = ("0", None, "2", "4", "6", "8")  # (None: the launcher's choice)
THREADS = ("64", "256")


def hold_block(F, s_cycle, seed, irregular=True):
    """(block, s): row r has s[r] = s_cycle[r % len] once-only features, in its first s[r] fields.  Field f's
    other rows share ids two by two (three where their number is odd).  irregular: the last row with s >= 1
    loses its (once-only) entry of field 0, and the last row with s = 0 gets a second entry of field 1, with
    an id that occurs nowhere else."""
    rng = np.random.default_rng(seed)
    s = np.array([s_cycle[r % len(s_cycle)] for r in range(ROWS)])
    feat = np.zeros((ROWS, F), np.int64)
    for f in range(F):
        shared = np.flatnonzero(s <= f)
        assert shared.size >= 2
        idx = np.arange(shared.size) // 2
        if shared.size % 2:
            idx[-1] = idx[-2]
        feat[shared, f] = f * PER + idx
        own = np.flatnonzero(s > f)
        feat[own, f] = f * PER + 32 + own
    val = (rng.random((ROWS, F)) + 0.25).astype(f32)
    val[rng.random((ROWS, F)) < 0.5] = 1.0
    label = (rng.random(ROWS) < 0.4).astype(np.int32)
    drop = int(np.flatnonzero(s >= 1)[-1]) if irregular else -1
    twice = int(np.flatnonzero(s == 0)[-1]) if irregular else -1
    fields, ids, vals, row_ptr = [], [], [], [0]
    for r in range(ROWS):
        for f in range(F):
            if r == drop and f == 0:
                continue
            fields.append(f)
            ids.append(feat[r, f])
            vals.append(val[r, f])
            if r == twice and f == 1:
                fields.append(1)
                ids.append(1 * PER + 96)
                vals.append(f32(0.75))
        row_ptr.append(len(fields))
    blk = Csr(np.array(row_ptr, np.int32), np.array(fields, np.int32), np.array(ids, np.int32),
              np.array(vals, f32), label)
    # the construction, checked: once-only features per row
    uniq, cnt = np.unique(blk.feat, return_counts=True)
    once = set(uniq[cnt == 1].tolist())
    got = np.array([sum(int(i) in once for i in blk.feat[row_ptr[r]:row_ptr[r + 1]]) for r in range(ROWS)])
    want = s.copy()
    if irregular:
        want[drop] -= 1
        want[twice] += 1
    assert np.array_equal(got, want), (got, want)
    return blk, s


def _engine(F, k, hp, with_field_start=True, **kw):
    fs = (np.arange(F + 1) * PER).astype(np.int32) if with_field_start else None
    return fa.Engine("FFM", F * PER, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F + 1,
                     max_row_nnz=F + 1, field_start=fs, **hp, **kw)


def _set(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _check(e, blk, want, what, weight=None):
    lg_o, ls_o, st_o = want
    lg, ls = e.train_batch(blk) if weight is None else e.train_batch(blk, weight)
    assert_bitwise(lg, lg_o, what + " logits")
    assert (np.isnan(ls) and np.isnan(ls_o)) or loss_close(ls, ls_o), (what, ls, ls_o)
    assert_state_bitwise(e.get_state(), st_o, what)
    e.close()


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("F,k", sorted(SHAPES), ids=["f%dk%d" % s for s in sorted(SHAPES)])
def test_held_vectors_give_the_oracles_bits(F, k, state, monkeypatch):
    hp, st_kw = STATES[state]
    o = CpuModel("oracle", "FFM", F * PER, F, k, **hp)
    st = fast_state(np.random.default_rng(2000 + 10 * F + k), o, **st_kw)
    blk, _ = hold_block(F, SHAPES[(F, k)], seed=F + k)
    o.set_state(st)
    lg, ls = o.train_batch(blk)
    want = (lg, ls, o.get_state())
    if state.startswith("cold"):
        once = np.flatnonzero(np.bincount(blk.feat, minlength=F * PER) == 1)
        assert np.isnan(want[2]["vec_z"][once]).any(), "the NaNs must pass through once-only records"
    for threads in THREADS:
        for hold in HOLDS:
            # (without field_start -- a record of n_fields slots, its own field's among them -- at one count)
            for with_fs in ((True, False) if hold == "8" else (True,)):
                _set(monkeypatch, "FFM_ROW_THREADS", threads)
                _set(monkeypatch, "FFM_ROW_HOLD", hold)
                e = _engine(F, k, hp, with_fs)
                e.set_state(st)
                _check(e, blk, want, "F=%d k=%d %s FFM_ROW_THREADS=%s FFM_ROW_HOLD=%s field_start=%s"
                       % (F, k, state, threads, hold, with_fs))


@pytest.mark.parametrize("park", ["park_0", "park_default", "budget_48k", "park_4k"])
def test_held_vectors_with_parking(park, monkeypatch):
    """FFM_ROW_PARK 0 (every w of the update read back from memory), the default (the budget that
    follows the kernel's occupancy), 4096 bytes (a part parked) and a budget above 32 KB."""
    F, k = 39, 16
    hp, st_kw = STATES["cold_stress_hp"]
    o = CpuModel("oracle", "FFM", F * PER, F, k, **hp)
    st = fast_state(np.random.default_rng(31), o, **st_kw)
    blk, _ = hold_block(F, SHAPES[(F, k)], seed=5)
    o.set_state(st)
    lg, ls = o.train_batch(blk)
    want = (lg, ls, o.get_state())
    _set(monkeypatch, "FFM_ROW_PARK", {"park_0": "0", "park_4k": "4096"}.get(park))
    _set(monkeypatch, "FFM_ROW_PARK_BUDGET", "49152" if park == "budget_48k" else None)
    for threads in THREADS:
        for hold in HOLDS:
            _set(monkeypatch, "FFM_ROW_THREADS", threads)
            _set(monkeypatch, "FFM_ROW_HOLD", hold)
            e = _engine(F, k, hp)
            e.set_state(st)
            _check(e, blk, want, "%s FFM_ROW_THREADS=%s FFM_ROW_HOLD=%s" % (park, threads, hold))


@pytest.mark.parametrize("F,k", [(39, 16), (16, 4)], ids=["f39k16", "f16k4"])
def test_held_vectors_learning_variant(F, k, monkeypatch):
    """FFM_FLAG_LEARN: the refresh keeps the stored w where n is not positive, so a held slot's old w is
    read beside its (n, z); a fifth of vec_n is zero."""
    hp, st_kw = STATES["cold_stress_hp"]
    o = CpuModel("oracle", "FFM", F * PER, F, k, learn=True, **hp)
    st = fast_state(np.random.default_rng(41 + k), o, **st_kw)
    blk, _ = hold_block(F, SHAPES[(F, k)], seed=6)
    o.set_state(st)
    lg, ls = o.train_batch(blk)
    want = (lg, ls, o.get_state())
    for threads in THREADS:
        for hold in HOLDS:
            _set(monkeypatch, "FFM_ROW_THREADS", threads)
            _set(monkeypatch, "FFM_ROW_HOLD", hold)
            e = _engine(F, k, hp, learn=True)
            e.set_state(st)
            _check(e, blk, want, "learn F=%d k=%d FFM_ROW_THREADS=%s FFM_ROW_HOLD=%s" % (F, k, threads, hold))


def test_held_vectors_with_sample_weights(monkeypatch):
    """Per-row sample weights scale tmp_grad, which the in-row update applies to held vectors: the
    weighted twin of every holding instantiation against the numpy restatement of the fold
    (test_block_semantics) on the regular rows."""
    F, k, hp = 8, 32, STRESS_HP  # (64 vectors per record: 2 at 256 and 8 at 64 threads hold a whole row's)
    o = CpuModel("oracle", "FFM", F * PER, F, k, **hp)
    st = fast_state(np.random.default_rng(51), o, n_add=0.05)
    blk, _ = hold_block(F, SHAPES[(F, k)], seed=7, irregular=False)
    rng = np.random.default_rng(52)
    weight = np.ascontiguousarray(rng.choice(np.array([0, 0.25, 1, 3.5, 1e-3, 64], f32), ROWS), f32)
    o.set_state(st)
    logits, _ = o.train_batch(blk)
    tg = (np.array([f32(o.sigmoid(float(l))) - f32(y) for l, y in zip(logits, blk.label)], f32) * weight).astype(f32)
    with np.errstate(all="ignore"):
        want_state = numpy_block(o, st, blk, tg, hp, F, k)
    want_loss = sum(float(np.float64(w) * np.float64(o.loss(int(y), float(l)))) for l, y, w in zip(logits, blk.label, weight))
    for threads in THREADS:
        for hold in HOLDS:
            _set(monkeypatch, "FFM_ROW_THREADS", threads)
            _set(monkeypatch, "FFM_ROW_HOLD", hold)
            e = _engine(F, k, hp)
            e.set_state(st)
            _check(e, blk, (logits, want_loss, want_state), "weighted FFM_ROW_THREADS=%s FFM_ROW_HOLD=%s" % (threads, hold),
                   weight)
