"""The CPU side of tests/test_gpu_big_offsets.py, at the real feature counts: the id helpers against brute-force
arithmetic in Python integers, and what the GPU module takes for granted about its blocks -- the tier counts, every
straddling feature present, the cap on non-finite results, and the witness that a read which lands elsewhere (on
zero, or on another feature's weights) changes every row.  Only the compact oracle runs here."""
import numpy as np
import pytest

import ftrl_ffm_amd as fa
from util import (BIG_F, BIG_FM_STRIDE, BIG_K, BIG_L, BIG_NF, BIG_NF_FM, BIG_NF_TRAIN_INIT, BIG_NF_VEC_SERVE, BIG_NF_VEC_TRAIN, alias_ids, big_case,
                  big_step, big_tier_entries, big_upper_zeroed, bits, count_past, edge_ids, nonfinite_share, offset_tier,
                  straddling_ids)

CASES = ("ffm", "fm", "vec_serve", "vec_train")


@pytest.fixture(scope="module", autouse=True)
def _built():
    fa.build()


def test_feature_counts_cross_both_thresholds():
    assert BIG_F * BIG_K == BIG_L
    # serving layout: 3 441 480 holds element 2^31, 6 882 960 holds element 2^32, 8 records lie wholly past 2^32
    assert 3441480 * BIG_L < 2 ** 31 < 3441481 * BIG_L
    assert 6882960 * BIG_L < 2 ** 32 < 6882961 * BIG_L
    assert (BIG_NF - 8) * BIG_L >= 2 ** 32 > (BIG_NF - 9) * BIG_L and BIG_NF == 6882969
    assert (BIG_NF_FM - 8) * BIG_FM_STRIDE >= 2 ** 32 > (BIG_NF_FM - 9) * BIG_FM_STRIDE and BIG_NF_FM == 22369630
    assert (BIG_NF_TRAIN_INIT - 8) * 3 * BIG_L >= 2 ** 32 > (BIG_NF_TRAIN_INIT - 9) * 3 * BIG_L
    # in vectors of four factors (the unit several kernels count in): 8 records wholly past vector 2^32
    assert (BIG_NF_VEC_SERVE - 8) * BIG_L >= 4 * 2 ** 32 > (BIG_NF_VEC_SERVE - 9) * BIG_L and BIG_NF_VEC_SERVE == 27531850
    assert (BIG_NF_VEC_TRAIN - 8) * 3 * BIG_L >= 4 * 2 ** 32 > (BIG_NF_VEC_TRAIN - 9) * 3 * BIG_L and BIG_NF_VEC_TRAIN == 9177289
    assert BIG_NF * 3 * BIG_L // 4 < 2 ** 32 and BIG_NF * BIG_L // 4 < 2 ** 31  # which BIG_NF does not reach
    assert max(BIG_NF_FM, BIG_NF_VEC_SERVE) < 2 ** 26  # no bitmap-word edge at 2^26 or 2^27 features inside either table: the last word's it is
    for limit, stride, n in ((2 ** 32, 7, 3), (100, 10, 1), (101, 10, 8)):
        c = count_past(limit, stride, n)
        assert (c - n) * stride >= limit > (c - n - 1) * stride


@pytest.mark.parametrize("n_feats,stride,elem_bytes,unit", [
    (BIG_NF, BIG_L, 2, 1), (BIG_NF, BIG_L, 4, 1), (BIG_NF, 3 * BIG_L, 4, 1), (BIG_NF_FM, BIG_FM_STRIDE, 4, 1), (3441481, BIG_L, 4, 1),
    (1000, 16, 4, 1), (BIG_NF_VEC_SERVE, BIG_L, 2, 4), (BIG_NF_VEC_TRAIN, 3 * BIG_L, 4, 4)])
def test_edge_ids_against_brute_force(n_feats, stride, elem_bytes, unit):
    elems = [2 ** 31 * unit, 2 ** 32 * unit]
    byte_offsets = [2 ** 32, 2 ** 33, 2 ** 34]
    want_straddle = set()
    for h in _records_near(elems + [b // elem_bytes for b in byte_offsets], stride, n_feats):
        lo, hi = h * stride, (h + 1) * stride  # the record's elements [lo, hi), bytes [lo * eb, hi * eb)
        if any(lo <= t < hi for t in elems) or any(lo * elem_bytes <= b < hi * elem_bytes for b in byte_offsets):
            want_straddle.add(h)
    assert straddling_ids(n_feats, stride, elem_bytes, unit) == sorted(want_straddle)
    want = sorted({h + d for h in want_straddle for d in (-1, 0, 1) if 0 <= h + d < n_feats})
    got = edge_ids(n_feats, stride, elem_bytes, unit)
    assert got.dtype == np.int64 and got.tolist() == want
    if n_feats * stride * elem_bytes > 2 ** 32:
        assert len(want_straddle) >= 1
    tiers = offset_tier(got, stride, unit)
    for h, t in zip(got.tolist(), tiers.tolist()):
        lo, hi = h * stride // unit, ((h + 1) * stride - 1) // unit  # the first and the last unit of the record
        assert t == (0 if hi < 2 ** 31 else 1 if lo >= 2 ** 31 and hi < 2 ** 32 else 2 if lo >= 2 ** 32 else -1)


def _records_near(offsets, stride, n_feats):
    """Every record within two of one that could hold one of the offsets: the candidates of the brute-force scan."""
    out = set()
    for t in offsets:
        for h in range(t // stride - 2, t // stride + 3):
            if 0 <= h < n_feats:
                out.add(h)
    return sorted(out)


@pytest.mark.parametrize("name", CASES)
def test_alias_ids_against_brute_force(name):
    c = big_case(name)
    probes = set(c.probes.tolist())
    for kind, (stride, eb) in c.layouts.items():
        got = c.aliases(kind)
        want = set()
        for h in probes:
            first = h * stride  # the first element of the record, as a Python integer
            wrapped = [first & 0xffffffff, first & 0x7fffffff, ((first * eb) & 0xffffffff) // eb]
            if c.unit > 1:  # an index counted in units (stride is a whole number of them), wrapped, back in elements
                assert stride % c.unit == 0
                wrapped += [((first // c.unit) & 0xffffffff) * c.unit, ((first // c.unit) & 0x7fffffff) * c.unit]
            for x in wrapped:
                for e in (x, x + stride - 1):  # the first and the last element a wrapped record would touch
                    want.add(e // stride)
        want = sorted(a for a in want if a not in probes and a < c.n_feats)
        assert got.dtype == np.int32 and got.tolist() == want, kind
        assert not probes & set(got.tolist())
        if kind in c.tier_kinds:
            assert (offset_tier(got, stride, c.unit) == 0).sum() >= 8, kind  # the records past 2^32 alone alias 8 low ones
    # the plain signature: element-index wraps only
    plain = alias_ids(c.probes, stride, c.n_feats)
    assert set(plain.tolist()) <= set(alias_ids(c.probes, stride, c.n_feats, 4).tolist())


@pytest.mark.parametrize("name", CASES)
def test_probe_set_and_compact_twin(name):
    c = big_case(name)
    assert np.array_equal(np.unique(c.probes), c.probes) and c.probes[0] == 0 and c.probes[-1] == c.n_feats - 1
    for kind, (stride, eb) in c.layouts.items():
        for unit in (1, c.unit):
            assert set(edge_ids(c.n_feats, stride, eb, unit).tolist()) <= set(c.probes.tolist())
    assert {1, c.n_feats - 1 - 64}.issubset(c.probes.tolist()) and set(range(c.n_feats - 8, c.n_feats)) <= set(c.probes.tolist())
    assert 200 <= c.probes.size <= 300
    # the compact ids: a bijection onto part of [0, n_compact), field f's ids in [f * per, (f + 1) * per)
    assert np.unique(c.compact).size == c.probes.size and c.compact.max() < c.n_compact
    assert np.array_equal(c.compact // c.per, c.field_of)
    blk, cb = c.block, c.compact_block
    assert np.array_equal(c.probes[np.searchsorted(c.probes, blk.feat)], blk.feat)
    if name != "fm":
        assert np.array_equal(cb.field, cb.feat // c.per)  # one field per id: the zeroed-slot argument's condition
    else:
        assert not blk.field.any()
    lens = np.diff(blk.row_ptr)
    assert (lens == 0).sum() == 1 and lens[-1] == BIG_F + 1 and (np.delete(lens, [np.argmin(lens), lens.size - 1]) == BIG_F).all()
    last = blk.feat[blk.row_ptr[-2]:]
    assert np.unique(last).size == last.size - 1  # an id twice
    assert blk.n_rows >= 64


@pytest.mark.parametrize("name", CASES)
def test_tier_counts_and_straddlers(name):
    c = big_case(name)
    for kind in c.tier_kinds:
        n = big_tier_entries(c, kind)
        assert min(n[0], n[1], n[2]) >= 100, (kind, n)
    present = set(c.block.feat.tolist())
    assert c.straddlers() and set(c.straddlers()) <= present
    # every non-empty row mixes the tiers of every layout: an id past 2^32 beside one below 2^31
    lens = np.diff(c.block.row_ptr)
    for kind in c.tier_kinds:
        t = c.tiers(kind, c.block.feat)
        for r in np.flatnonzero(lens):
            row = t[c.block.row_ptr[r]:c.block.row_ptr[r + 1]]
            assert (row == 2).any() and (row == 0).any(), (kind, r)


@pytest.mark.parametrize("name", CASES)
def test_a_read_that_lands_elsewhere_changes_every_row(name):
    """Elsewhere is zero (the tables start zeroed and only probe rows are written) or another probe's weights."""
    c = big_case(name)
    whole = c.weights_oracle(c.state["vec_w"]).predict_batch(c.compact_block)[0]
    nonempty = np.diff(c.block.row_ptr) > 0
    assert np.isfinite(whole).all()
    for kind in c.tier_kinds:
        for tiers in ((1, 2, -1), (2,)):  # everything not wholly below 2^31; the records past 2^32 alone
            vw, lw = big_upper_zeroed(c, kind, tiers)
            got = c.weights_oracle(vw, lw).predict_batch(c.compact_block)[0]
            assert (bits(got) != bits(whole))[nonempty].all(), (kind, tiers)
    # another feature's weights: every upper-tier probe reads the row of the next probe instead
    vw = c.state["vec_w"].copy()
    up = c.compact[c.tiers(c.tier_kinds[0]) != 0]
    vw[up] = c.state["vec_w"][np.roll(up, 1)]
    got = c.weights_oracle(vw).predict_batch(c.compact_block)[0]
    assert (bits(got) != bits(whole))[nonempty].all()
    # ... and the fp16 table's decoded weights are not the fp32 ones (the two serving formats are two references)
    if name != "fm":
        half = c.state["vec_w"].astype(np.float16).astype(np.float32)
        assert (bits(c.weights_oracle(half).predict_batch(c.compact_block)[0]) != bits(whole))[nonempty].all()


@pytest.mark.parametrize("name", CASES)
def test_at_most_a_tenth_is_non_finite(name):
    c = big_case(name)
    lg, ls, after = big_step(c)
    bad_logits, bad_words, n_touched = nonfinite_share(lg, c.state, after)
    assert n_touched > 0 and bad_logits <= 0.1 and bad_words <= 0.1, (bad_logits, bad_words, n_touched)
    assert np.isfinite(ls)
    # every probe of the block is touched, no other compact id is
    changed = np.flatnonzero(bits(after["lin_n"]) != bits(c.state["lin_n"]))
    assert np.array_equal(changed, np.unique(c.compact_block.feat))
    # prediction on the stepped model, which the GPU module compares as well
    assert np.isfinite(c.oracle(after).predict_batch(c.compact_block)[0]).mean() >= 0.9
