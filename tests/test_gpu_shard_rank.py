"""One rank of the 8-GPU job exactly as bench.py --emulate-shards 8 --emulate-rank r runs it, against
the oracle: FFM 39x16, 8 compact shards (per-field id ranges), 65 536-row blocks (the weak-scaling
leg) and an 8 192-row one (the strong-scaling leg), each rank fed only the columns it keeps, the
blocks staged two ahead so that their grouping has run when the step reads it.

At this size a block has features with >= 2048 occurrences (the super ranges: pass A inside the
update launch, then the second pass and the join), ~10^5 few-occurrence and once-only features (the
flat kernels' item loops take more than one pass) and the h_super gate of a prepared block decides
whether the few-occurrence launch is deferred behind the super pass.  The smaller tests' Zipf blocks
reach none of that.

Partial logits summed over the ranks: rtol 1e-5 / atol 2e-6 of the oracle's (the association order
differs); every update is driven by the oracle's logits (an exact all-reduce), so every rank's
owned state is the oracle's bit for bit.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import CpuModel, Csr
from util import (STRESS_HP, assert_bitwise, assert_rank_rows, fast_state, get_bias3, keep_columns,
                  kept_copy, run_rank_staged, set_bias3)

pytestmark = pytest.mark.gpu

F, K, S = 39, 16, 8
PER = 10_000
SUPER_MIN = 2048  # kSuperMin


def _dev(blk):
    return {n: torch.from_numpy(np.ascontiguousarray(getattr(blk, n))).cuda()
            for n in ("row_ptr", "field", "feat", "val", "label")}


def test_emulated_rank_matches_the_oracle_at_bench_size():
    n_feats = F * PER
    fs = (np.arange(F + 1) * PER).astype(np.int32)
    g = synth.Generator(F, n_feats, "zipf", seed=42)
    blocks = [g.block(65536), g.block(8192), g.block(65536)]
    feats = np.unique(np.concatenate([b.feat for b in blocks]))
    fld = (feats // PER).astype(np.int64)
    plan = fa.shard_plan(F, S, field_map=True)

    # coverage: what the test is meant to reach is in the blocks every rank sees
    for r in range(S):
        keep = keep_columns(plan, r)
        owns = (plan["pair_owner"] == r).any(axis=1)
        for i, b in enumerate(blocks):
            u, c = np.unique(b.feat, return_counts=True)
            f_u = u // PER
            kept = keep[f_u]
            if b.n_rows == 65536:
                assert (owns[f_u] & (c >= SUPER_MIN)).any(), "rank %d: no super feature in block %d" % (r, i)
                assert (kept & (c >= 2) & (c <= 10)).sum() >= 20000, (r, i)
                assert (kept & (c == 1)).sum() >= 20000, (r, i)
            else:
                assert c.max() < SUPER_MIN  # the strong-scaling block has none: h_super must reset

    # start state: the ranks' engines first (they keep it in HBM), then the oracle
    rng = np.random.default_rng(17)
    o = CpuModel("oracle", "FFM", feats.size, F, K, **STRESS_HP)
    st = fast_state(rng, o, n_add=0.05)
    mk = lambda r: fa.Engine("FFM", n_feats, F, K, skip_init=True, max_batch_rows=65536,  # noqa: E731
                             max_batch_nnz=65536 * F, n_shards=S, shard_rank=r, max_row_nnz=F,
                             field_start=fs, **STRESS_HP)
    ranks, whole = [], []
    for r in range(S):
        for lst in (ranks, whole):
            e = mk(r)
            e.set_rows(feats, {key: st[key] for key in fa.Engine.ROW_KEYS})
            set_bias3(e, st["bias3"])
            lst.append(e)
    o.set_state(st)
    del st

    remap = lambda b: Csr(b.row_ptr, b.field, np.searchsorted(feats, b.feat).astype(np.int32),  # noqa: E731
                          b.val, b.label)
    logits = [o.train_batch(remap(b))[0] for b in blocks]
    want = {key: o._view(key, (feats.size, F * K) if key.startswith("vec") else (feats.size,))
            for key in fa.Engine.ROW_KEYS}
    bias = o._view("bias3", (3,)).copy()

    # the first block with every column: what a kept-columns rank computes must not depend on the
    # columns it drops (checked on the block's super / giant features and a sample of the rest)
    u0, c0 = np.unique(blocks[0].feat, return_counts=True)
    probe = np.union1d(u0[c0 > 256], np.random.default_rng(5).choice(u0, 20000, replace=False)).astype(np.int32)
    d0 = _dev(blocks[0])
    exact0 = torch.from_numpy(logits[0]).cuda()
    parts_sum = [np.zeros(b.n_rows, np.float64) for b in blocks]
    for r in range(S):
        keep = keep_columns(plan, r)
        mine = [kept_copy(b, keep) for b in blocks]
        e, ew = ranks[r], whole[r]
        part = torch.zeros(65536, device="cuda")
        ew.train_forward_device(65536, blocks[0].nnz, d0["row_ptr"].data_ptr(), d0["field"].data_ptr(),
                                d0["feat"].data_ptr(), d0["val"].data_ptr(), d0["label"].data_ptr(),
                                part.data_ptr())
        ew.sync()
        ew.train_update_device(exact0.data_ptr())
        ew.sync()
        timed = {}

        def after(i):
            if i == 0:
                rows_kept = e.get_rows(probe)
                rows_all = ew.get_rows(probe)
                for key in fa.Engine.ROW_KEYS:
                    assert_bitwise(rows_kept[key], rows_all[key], "rank %d kept vs all columns %s" % (r, key))
            if i < 2:
                timed[i] = e.profile_dump()
                e.profile_enable(True)  # (resets the counts)

        e.profile_enable(True)
        parts = run_rank_staged(e, mine, logits, ahead=2, after_step=after)
        assert "update_giant_kernel" in timed[0], "rank %d: no super pass on the 65536-row block\n%s" % (r, timed[0])
        assert "update_giant_kernel" not in timed[1], "rank %d: super pass on the 8192-row block\n%s" % (r, timed[1])
        e.profile_enable(False)
        for i, p in enumerate(parts):
            parts_sum[i] += p
        assert_rank_rows(e, r, feats, fld, want, plan, K, "kept columns")
        if r == plan["bias_owner"]:
            assert_bitwise(get_bias3(e), bias, "rank %d bias3" % r)
        e.close()
        ew.close()
    for i, b in enumerate(blocks):
        np.testing.assert_allclose(parts_sum[i].astype(np.float32), logits[i], rtol=1e-5, atol=2e-6,
                                   err_msg="block %d: summed partial logits" % i)
