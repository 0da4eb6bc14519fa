"""The few-occurrence range of the FFM update (2..kSmallMax = 10 occurrences per block, one wave per
feature, csrc/kernels_update.h) on regular blocks: the partner ids and values of all of a feature's
touches are fetched once per feature from the CSR rows and parked in LDS, and the passes over the
record read them there instead of gathering the row table batch by batch -- where a record is more
than one pass of 64 vectors; a one-pass record keeps the row table.  FFM_FEW_STAGE=0 selects the
row-table path on regular blocks too.  Same operands, same order: every case below must give
the oracle's bits -- logits, loss and the whole state (w, n, z of every record) -- with the
staging on and with the switch off.

Blocks of 160 rows in which chosen features occur exactly 2, 3, 4, 5, 8, 9, 10 times (the batches
of four and kSmallMax), 11 times (the hot range's first count) and once, all together.  Each shape
runs in three forms: regular on an engine with field_start (the staged path), the same rows with
one row missing a field and one row carrying a field twice (irregular: the row table, and serial
slots for the features of that row), and the regular rows on an engine without field_start (never
regular); the update as one launch (the few range inside the tile region of the launch's dynamic
LDS, eight-wave workgroups at k >= 16) and as three launches side by side (the few launch with a
staging area of its own).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from test_block_semantics import numpy_block
from util import (DEFAULT_HP, STRESS_HP, assert_bitwise, assert_state_bitwise, block_ids_per_field, fast_state,
                  loss_close, occurrence_block)

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = 160
COUNTS = (2, 3, 4, 5, 8, 9, 10, 11, 1, 2, 10, 4)  # (53 + 17 occurrences: fits one field of a 3-field block)
# three passes of 64 vectors, the last partial | NF 4, one pass | NF 1, one pass | k 32, one pass | exactly two passes |
# NF 2 (k = 8), 78 vectors: staged in that instantiation | 48 fields: ten touches are 480 staged words, so the
# staging loop's second round (past 448 words) runs
# (records of one pass keep the row table on regular blocks too: both sides of that threshold)
SHAPES = [(39, 16), (39, 4), (8, 16), (3, 32), (16, 32), (39, 8), (48, 16)]
# warm: |z| on both sides of l1 (z ~ N(0, 0.3); l1 = 0.1 / 0.01); cold: n near 0 and a fifth of vec_n zero, so
# that ffm.cpp:118's square roots of negative numbers reach the folds
STATES = {"warm_default_hp": (DEFAULT_HP, dict(n_add=0.05)), "warm_stress_hp": (STRESS_HP, dict(n_add=0.05)),
          "cold_stress_hp": (STRESS_HP, dict(n_hi=0.02, n_zero=0.2)), "cold_default_hp": (DEFAULT_HP, dict(n_hi=0.02, n_zero=0.2))}


def _irregular(blk, ids, counts):
    """The block with one row missing a field and one row carrying a field twice.  Both rows hold a
    few-occurrence feature: the one that occurs 3 times loses its right-hand neighbour in its first
    row, the one that occurs 9 times gets a second entry of its neighbour's field in its first row."""
    n_rows = blk.n_rows
    F = int(blk.row_ptr[1] - blk.row_ptr[0])
    feat, fld, val = (a.reshape(n_rows, F) for a in (blk.feat, blk.field, blk.val))
    at3 = np.argwhere(feat == ids[counts.index(3)])[0]
    at9 = np.argwhere(feat == ids[counts.index(9)])[0]
    assert at3[0] != at9[0]
    drop = (int(at3[0]), (int(at3[1]) + 1) % F)
    twice = (int(at9[0]), (int(at9[1]) + 1) % F)
    rows_f, rows_i, rows_v, row_ptr = [], [], [], [0]
    for r in range(n_rows):
        cols = [c for c in range(F) if (r, c) != drop]
        f_r, i_r, v_r = list(fld[r, cols]), list(feat[r, cols]), list(val[r, cols])
        if r == twice[0]:  # (an id of the same field from the next row, right behind the field's entry)
            at = cols.index(twice[1]) + 1
            f_r.insert(at, twice[1])
            i_r.insert(at, feat[(r + 1) % n_rows, twice[1]])
            v_r.insert(at, f32(0.75))
        rows_f += f_r
        rows_i += i_r
        rows_v += v_r
        row_ptr.append(len(rows_f))
    return Csr(np.array(row_ptr, np.int32), np.array(rows_f, np.int32), np.array(rows_i, np.int32),
               np.array(rows_v, f32), blk.label.copy())


def _engine(F, k, hp, with_field_start, nnz):
    per = block_ids_per_field(ROWS)
    fs = (np.arange(F + 1) * per).astype(np.int32) if with_field_start else None
    return fa.Engine("FFM", F * per, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=nnz,
                     max_row_nnz=F + 1, field_start=fs, **hp)


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("F,k", SHAPES, ids=["f%dk%d" % s for s in SHAPES])
def test_few_range_gives_the_oracles_bits_staged_and_not(F, k, state, monkeypatch):
    hp, st_kw = STATES[state]
    per = block_ids_per_field(ROWS)
    o = CpuModel("oracle", "FFM", F * per, F, k, **hp)
    st = fast_state(np.random.default_rng(1000 + 10 * F + k), o, **st_kw)
    regular, ids, _ = occurrence_block(F, COUNTS, ROWS, seed=F + k)
    _, cnt = np.unique(regular.feat, return_counts=True)
    assert set(COUNTS) <= set(cnt.tolist()) and (cnt == 1).sum() > F
    forms = (("regular", regular, True), ("irregular", _irregular(regular, ids, list(COUNTS)), True),
             ("regular, no field_start", regular, False))
    want = {}
    for name, blk, _ in forms:
        if name.startswith("irregular") or "regular" not in want:
            o.set_state(st)
            lg, ls = o.train_batch(blk)
            want["irregular" if name.startswith("irregular") else "regular"] = (lg, ls, o.get_state())
    if state.startswith("cold"):
        assert np.isnan(want["regular"][2]["vec_z"][ids]).any(), "the NaNs must reach the few-occurrence folds"
    for stage in ("1", "0"):
        for split in ("0", "2"):
            monkeypatch.setenv("FFM_FEW_STAGE", stage)
            monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
            for name, blk, with_fs in forms:
                lg_o, ls_o, st_o = want["irregular" if name.startswith("irregular") else "regular"]
                e = _engine(F, k, hp, with_fs, ROWS * F + 1)
                e.set_state(st)
                lg, ls = e.train_batch(blk)
                what = "F=%d k=%d %s %s FFM_FEW_STAGE=%s FFM_UPDATE_SPLIT=%s" % (F, k, state, name, stage, split)
                assert_bitwise(lg, lg_o, what + " logits")
                assert (np.isnan(ls) and np.isnan(ls_o)) or loss_close(ls, ls_o), (what, ls, ls_o)
                assert_state_bitwise(e.get_state(), st_o, what)
                e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
def test_few_range_with_sample_weights(split, monkeypatch):
    """Per-row sample weights scale tmp_grad, which the staged path reads where the row-table path
    does: the weighted block against the numpy restatement of the fold (test_block_semantics), staged
    and not."""
    F, k, hp = 9, 32, STRESS_HP  # (72 vectors per record: two passes, so the regular block is staged)
    per = block_ids_per_field(ROWS)
    o = CpuModel("oracle", "FFM", F * per, F, k, **hp)
    st = fast_state(np.random.default_rng(77), o, n_add=0.05)
    blk = occurrence_block(F, COUNTS, ROWS, seed=3)[0]
    rng = np.random.default_rng(78)
    weight = np.ascontiguousarray(rng.choice(np.array([0, 0.25, 1, 3.5, 1e-3, 64], f32), ROWS), f32)
    o.set_state(st)
    logits, _ = o.train_batch(blk)
    tg = (np.array([f32(o.sigmoid(float(l))) - f32(y) for l, y in zip(logits, blk.label)], f32) * weight).astype(f32)
    with np.errstate(all="ignore"):
        want = numpy_block(o, st, blk, tg, hp, F, k)
    want_loss = sum(float(np.float64(w) * np.float64(o.loss(int(y), float(l)))) for l, y, w in zip(logits, blk.label, weight))
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    for stage in ("1", "0"):
        monkeypatch.setenv("FFM_FEW_STAGE", stage)
        e = _engine(F, k, hp, True, ROWS * F)
        e.set_state(st)
        lg, ls = e.train_batch(blk, weight)
        what = "weighted, FFM_FEW_STAGE=%s FFM_UPDATE_SPLIT=%s" % (stage, split)
        assert_bitwise(lg, logits, what + " logits")
        assert loss_close(ls, want_loss), (what, ls, want_loss)
        assert_state_bitwise(e.get_state(), want, what)
        e.close()
