"""Blocks built so that chosen features occur EXACTLY at the per-block occurrence counts where the
update changes path (util.EDGE_COUNTS: once only | few, gathered four at a time | hot, tiles of 16 |
very hot | giant, one workgroup | super, ranges of 256 all over the chip), each edge with its
neighbours.  The grouping lists a feature by its count (kernels_group.h) and the kernels test the
count again themselves: an off-by-one between the two, or a wrong partial last batch, tile, segment
or range, changes bits the oracle pins.  Every case: logits and the whole state bit for bit, NaN
positions included (stress hyper-parameters on state with n near 0 and a fifth of vec_n zero, so
ffm.cpp:118's NaNs reach the folds; the sharded case on warm state, so that its second block stays
finite) -- but for the sharded case's summed partial logits (rtol 1e-5).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel
from util import (DEFAULT_HP, EDGE_COUNTS, FM_EDGE_COUNTS, STRESS_HP, assert_bitwise, assert_rank_rows,
                  assert_state_bitwise, block_ids_per_field, fast_state, get_bias3, irregular_copy,
                  keep_columns, kept_copy, occurrence_block, run_rank_staged)

pytestmark = pytest.mark.gpu

ROWS = 6144  # the largest count (4097) in one field, every field with room for once-only ids


def _state(o, seed, hp_name):
    rng = np.random.default_rng(seed)
    if hp_name == "stress":
        return fast_state(rng, o, n_hi=0.02, n_zero=0.2)
    return fast_state(rng, o, n_add=0.05)  # warm


def _train_both(o, e, blk, what):
    lo, so = o.train_batch(blk)
    lg, sg = e.train_batch(blk)
    assert_bitwise(lg, lo, what + " logits")
    if np.isnan(so):
        assert np.isnan(sg), what
    else:
        assert abs(sg - so) <= 1e-9 * max(1.0, abs(so)), (what, sg, so)


def _ffm_case(F, k, hp_name, split, monkeypatch, seed):
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    hp = STRESS_HP if hp_name == "stress" else DEFAULT_HP
    per = block_ids_per_field(ROWS)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **hp)
    st = _state(o, seed, hp_name)
    o.set_state(st)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    e = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F,
                  max_row_nnz=F, field_start=fs, **hp)
    # each block from the start state (after one such block most of the state is NaN): as built --
    # one entry per field, fields in order, ids in their field's range, so the range sort's short
    # cut and the regular folds apply -- and irregular (a third of one field's entries gone, some
    # rows in reverse field order)
    regular, ids, _ = occurrence_block(F, EDGE_COUNTS, ROWS, seed=seed)
    for name, blk in (("regular", regular), ("irregular", irregular_copy(regular, seed=seed))):
        o.set_state(st)
        e.set_state(st)
        what = "%s k=%d %s split=%s" % (name, k, hp_name, split)
        _train_both(o, e, blk, what)
        so = o.get_state()
        if hp_name == "stress":
            assert np.isnan(so["vec_z"][ids]).any(), "the NaNs must reach the edge features' folds"
        assert_state_bitwise(e.get_state(), so, what)
    e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
@pytest.mark.parametrize("k", [4, 8, 16, 32])
def test_every_edge_count_whole_model(k, split, monkeypatch):
    """FFM F=8, k = 4 / 8 / 16 (the three fact-record shapes) and 32, the update as one launch and
    as three side by side."""
    _ffm_case(8, k, "stress", split, monkeypatch, seed=100 + k)


def test_every_edge_count_default_hyper_parameters_warm_state(monkeypatch):
    _ffm_case(8, 16, "default", "0", monkeypatch, seed=7)


def test_every_edge_count_generic_kernel(monkeypatch):
    """k = 6: not a multiple of 4, the generic update kernel."""
    _ffm_case(8, 6, "stress", "0", monkeypatch, seed=11)


@pytest.mark.parametrize("k", [8, 64])
def test_every_fm_edge_count(k):
    """FM: giants from 65 occurrences, folded in ranges of 64 and joined; the small-class edges."""
    cols = 4
    n_rows = 1024
    per = block_ids_per_field(n_rows)
    nf = cols * per
    o = CpuModel("oracle", "FM", nf, 1, k, **STRESS_HP)
    st = _state(o, 200 + k, "stress")
    o.set_state(st)
    e = fa.Engine("FM", nf, 1, k, skip_init=True, max_batch_rows=n_rows, max_row_nnz=cols, **STRESS_HP)
    for s in (0, 1):  # (each from the start state: after one such block most of it is NaN)
        o.set_state(st)
        e.set_state(st)
        blk = occurrence_block(cols, FM_EDGE_COUNTS, n_rows, seed=300 + s)[0]
        blk.field[:] = 0  # libsvm rows
        _train_both(o, e, blk, "FM k=%d block %d" % (k, s))
        assert_state_bitwise(e.get_state(), o.get_state(), "FM k=%d block %d" % (k, s))
    e.close()


def test_every_edge_count_on_eight_compact_shards():
    """F = 39, k = 16 through eight compact shards, each fed its kept columns and staged ahead as
    bench.py does, updates driven by the oracle's logits: the edge counts now reach the shards' flat
    few-occurrence and once-only kernels and their super ranges."""
    F, k, S, n_rows = 39, 16, 8, 4352
    per = block_ids_per_field(n_rows)
    nf = F * per
    o = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    st = _state(o, 400, "warm")  # (stress hyper-parameters; n away from 0: the second block stays finite)
    fs = (np.arange(F + 1) * per).astype(np.int32)
    plan = fa.shard_plan(F, S, field_map=True)
    ranks = []
    for r in range(S):
        e = fa.Engine("FFM", nf, F, k, skip_init=True, max_batch_rows=n_rows, max_batch_nnz=n_rows * F,
                      n_shards=S, shard_rank=r, max_row_nnz=F, field_start=fs, **STRESS_HP)
        e.set_state(st)
        ranks.append(e)
    o.set_state(st)
    del st
    blocks = [occurrence_block(F, EDGE_COUNTS, n_rows, seed=500 + s)[0] for s in range(2)]
    logits = [o.train_batch(b)[0] for b in blocks]
    ids = np.arange(nf, dtype=np.int32)
    want = {key: o._view(key, (nf, F * k) if key.startswith("vec") else (nf,)) for key in fa.Engine.ROW_KEYS}
    total = [np.zeros(n_rows, np.float64) for _ in blocks]
    for r, e in enumerate(ranks):
        keep = keep_columns(plan, r)
        parts = run_rank_staged(e, [kept_copy(b, keep) for b in blocks], logits)
        for i, p in enumerate(parts):
            total[i] += p
        assert_rank_rows(e, r, ids, ids // per, want, plan, k, "edge counts")
        if r == plan["bias_owner"]:
            assert_bitwise(get_bias3(e), o._view("bias3", (3,)), "bias3")
        e.close()
    for i in range(len(blocks)):
        np.testing.assert_allclose(total[i].astype(np.float32), logits[i], rtol=1e-5, atol=2e-6)
