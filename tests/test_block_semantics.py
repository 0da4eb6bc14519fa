"""The block update by reductions (oracle/ffm_oracle.c: fo_train_batch) -- properties of the
definition itself, checked on the CPU:

* a block of ONE row is the reference's train() bit for bit, whatever the row looks like
  (multi-valued fields, repeated ids, fields out of order) -- against the oracle's sequential loop
  and, where it can run them, against the compiled reference;
* on blocks of many rows the reductions and the strict row-order walk of rounds 1-4
  (fo_train_batch_rowwalk) are the same update in exact arithmetic: same logits (the forward is
  shared), state within rounding distance, NaNs at the same places;
* a second, independent restatement of the fold in numpy float32 scalars (segments of 16 occurrences
  of the feature, left to right; telescoped step sizes; per-touch terms from the first ffm.cpp:118 touch on)
  agrees with the C bit for bit -- under the reference rule and under the learning variant
  (FFM_FLAG_LEARN), whose refresh it restates from the start state;
* the refresh rule itself on special values of n, z and the stored w (util.special_grid).
"""
import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import CpuModel, Csr
from util import (DEFAULT_HP, HP_SETS, STRESS_HP, arith_flags, assert_bitwise, assert_close,
                  assert_state_bitwise, bits, div_fast_ok, ftrl_w, grid_block, grid_want, latent_w, rand_state,
                  range_grid, special_grid)

SEG = 16  # FO_SEG


def test_the_three_statements_of_the_tree_share_one_segment_length():
    """The segment length is part of the block semantics: the oracle (FO_SEG), this
    file's numpy restatement (SEG) and the engine (kSeg, through the C ABI) must not drift apart."""
    import ftrl_ffm_amd as fa
    fa.build()
    assert pyoracle._lib("oracle")[0].fo_block_segment() == SEG
    assert fa.load_library().ffm_engine_block_segment() == SEG


def rand_rows(rng, n, F, nf, multi=False, dup=False, ordered=True, zipf=1.5, drop=0.15):
    per = nf // F
    rows, labels = [], []
    for _ in range(n):
        row = []
        for f in range(F):
            if rng.random() < drop:
                continue
            ids = set()
            for _ in range(1 + (multi and rng.random() < 0.2)):
                i = f * per + int(rng.zipf(zipf)) % per
                if i in ids:  # (the same id twice in a row only where `dup` asks for it)
                    continue
                ids.add(i)
                row.append((f, i, float(np.float32(rng.uniform(0.2, 1.5)))))
        if dup and row and rng.random() < 0.3:
            row.append(row[int(rng.integers(len(row)))])
        if not ordered:
            rng.shuffle(row)
        rows.append([tuple(e) for e in row])
        labels.append(int(rng.integers(2)))
    return Csr.from_rows(rows, labels)


SHAPES = [("FFM", 6, 4), ("FM", 1, 8), ("LR", 1, 1)]
KINDS = [(False, False, True), (True, False, True), (True, True, False), (False, True, True)]


@pytest.mark.parametrize("mt,F,k", SHAPES)
@pytest.mark.parametrize("multi,dup,ordered", KINDS)
@pytest.mark.parametrize("hp", [DEFAULT_HP, STRESS_HP], ids=["default_hp", "stress_hp"])
def test_block_of_one_row_is_the_sequential_step(mt, F, k, multi, dup, ordered, hp):
    rng = np.random.default_rng(11)
    nf = 60
    a = CpuModel("oracle", mt, nf, F, k, **hp)
    b = CpuModel("oracle", mt, nf, F, k, **hp)
    st = rand_state(rng, a)
    a.set_state(st)
    b.set_state(st)
    c = rand_rows(rng, 60, F if mt == "FFM" else 6, nf, multi, dup, ordered)
    if mt != "FFM":
        c.field[:] = 0
    la, _ = a.train_rows(c)
    lb = np.array([b.train_batch(c.rows(r, r + 1))[0][0] for r in range(c.n_rows)], np.float32)
    assert_bitwise(la, lb, "logits")
    assert_state_bitwise(a.get_state(), b.get_state(), "state")
    # FFM rows with a repeated id deadlock the reference
    if pyoracle.have_ref() and not (mt == "FFM" and dup):
        r = CpuModel("ref", mt, nf, F, k, **hp)
        r.set_state(st)
        lr, _ = r.train_rows(c)
        assert_bitwise(lr, lb, "logits vs reference")
        assert_state_bitwise(r.get_state(), b.get_state(), "state vs reference")


@pytest.mark.parametrize("mt,F,k", SHAPES)
@pytest.mark.parametrize("multi,dup,ordered", KINDS)
def test_reductions_equal_the_row_walk_up_to_rounding(mt, F, k, multi, dup, ordered):
    rng = np.random.default_rng(5)
    nf = 60
    a = CpuModel("oracle", mt, nf, F, k, **STRESS_HP)
    b = CpuModel("oracle", mt, nf, F, k, **STRESS_HP)
    st = rand_state(rng, a)
    a.set_state(st)
    b.set_state(st)
    c = rand_rows(rng, 700, F if mt == "FFM" else 6, nf, multi, dup, ordered)
    if mt != "FFM":
        c.field[:] = 0
    la, sa = a.train_batch(c)
    lb, sb = b.train_batch(c, rowwalk=True)
    assert_bitwise(la, lb, "logits")  # same refresh, same forward
    assert sa == sb
    A, B = a.get_state(), b.get_state()
    for key in A:
        # z is a sum with cancellation: bound the distance by the size of what was added
        assert_close(A[key], B[key], rtol=2e-5, atol=2e-5, what=key)
    changed = sum(int(np.count_nonzero(A[k_] != st[k_])) for k_ in A)
    assert changed > 50


def test_one_row_touching_a_slot_twice_keeps_the_walk_for_the_block():
    """A field with two entries in ONE row of a 200-row block: the slots that see both entries are
    walked in row order for the whole block (bit-identical to the row walk there), all other
    accumulators are reduced."""
    rng = np.random.default_rng(8)
    F, k, nf = 4, 4, 40
    c = rand_rows(rng, 200, F, nf, drop=0.0, zipf=3.0)
    rows = [[(int(c.field[p]), int(c.feat[p]), float(c.val[p])) for p in range(c.row_ptr[r], c.row_ptr[r + 1])]
            for r in range(c.n_rows)]
    rows[17].insert(2, (1, 10 + 7, 0.5))  # a second entry of field 1 in row 17
    c = Csr.from_rows(rows, c.label)
    a = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    b = CpuModel("oracle", "FFM", nf, F, k, **STRESS_HP)
    st = rand_state(rng, a)
    a.set_state(st)
    b.set_state(st)
    a.train_batch(c)
    b.train_batch(c, rowwalk=True)
    A, B = a.get_state(), b.get_state()
    L = F * k
    # the features of row 17 in fields 0, 2, 3: their slot for partner field 1 is serial
    for (f, i, _) in rows[17]:
        if f == 1:
            continue
        sl = slice(1 * k, 2 * k)
        assert_bitwise(A["vec_n"].reshape(nf, L)[i, sl], B["vec_n"].reshape(nf, L)[i, sl], "serial n")
        assert_bitwise(A["vec_z"].reshape(nf, L)[i, sl], B["vec_z"].reshape(nf, L)[i, sl], "serial z")
    assert (A["vec_z"] != B["vec_z"]).any()  # ... and the reductions do round differently elsewhere


# ---- an independent restatement of the fold ---------------------------------------------------

f32 = np.float32
NEG0 = f32(-0.0)


class Acc:
    def __init__(self, n0, alpha):
        self.P = self.G = self.D = self.Gacc = self.Dacc = NEG0
        self.B = f32(n0)
        self.n0 = f32(n0)
        self.alpha = f32(alpha)
        self.any = self.seen = self.head_plain = False
        self.ncap = f32(0)

    def flush(self):
        self.B = f32(self.B + self.P)
        self.Gacc = f32(self.Gacc + self.G)
        self.Dacc = f32(self.Dacc + self.D)
        self.P = self.G = self.D = NEG0

    def at(self, occ):
        """Before the touches of the feature's occurrence number occ: segments are cut by occurrence."""
        if occ > 0 and occ % SEG == 0:
            self.flush()

    def touch(self, w, g, q, plain):
        nt = f32(self.B + self.P)
        if not self.any:
            self.any, self.head_plain = True, plain
        if not plain and not self.seen:
            self.seen, self.ncap = True, nt
        if self.seen:
            with np.errstate(invalid="ignore"):
                d = f32(np.sqrt(f32(nt + q)) - np.sqrt(nt))
            self.D = f32(self.D + d)
        self.G = f32(self.G + g)
        self.P = f32(self.P + f32(g * g))

    def sigma_w_total(self, w):
        S = NEG0
        if self.head_plain:
            ncap = self.ncap if self.seen else self.B
            S = f32(S + f32(np.sqrt(ncap) - np.sqrt(self.n0)))
        S = f32(S + self.Dacc)
        return f32(f32(S / self.alpha) * w)

    def finish_latent(self, w, z0):
        self.flush()
        return self.B, f32(f32(f32(z0) + self.Gacc) - self.sigma_w_total(w))

    def finish_linear(self, w, z0):
        self.flush()
        si = f32(f32(np.sqrt(self.B) - np.sqrt(self.n0)) / self.alpha)
        return self.B, f32(f32(z0) + f32(self.Gacc - f32(si * w)))


def numpy_refresh(st, c, hp, F, k, learn):
    """The block's lazy refresh of the start state `st`, restated: the bias, every feature the rows
    hold and every latent slot (feature, partner field) a pair of entries touches get W(n, z)
    (util.ftrl_w); under the learning variant a latent slot with not n > 0 keeps its w instead."""
    w = {key: st[key].copy() for key in ("bias3", "lin_w", "vec_w")}
    if c.n_rows:
        w["bias3"][0] = ftrl_w(st["bias3"][1], st["bias3"][2], hp)
    for i in np.unique(c.feat):
        w["lin_w"][i] = ftrl_w(st["lin_n"][i], st["lin_z"][i], hp)
    L = F * k
    if not L:
        return w
    vw, vn, vz = w["vec_w"].reshape(-1, L), st["vec_n"].reshape(-1, L), st["vec_z"].reshape(-1, L)
    touched = set()
    for r in range(c.n_rows):
        ent = range(c.row_ptr[r], c.row_ptr[r + 1])
        touched.update((int(c.feat[p]), int(c.field[q])) for p in ent for q in ent if p != q)
    for i, fp in touched:
        for e in range(fp * k, fp * k + k):
            vw[i, e] = latent_w(vn[i, e], vz[i, e], vw[i, e], hp, learn)
    return w


def numpy_block(model, st, c, tg, hp, F, k, learn=False):
    """(n, z) of every accumulator after one block, from the frozen w and the rows' tmp_grad; rows
    hold one entry per field at most and no repeated ids.  The reference rule takes w from `model`
    (already refreshed); the learning variant restates the refresh from `st` (numpy_refresh) and
    makes every live latent touch a plain one (g*g: ffm.cpp:118 then takes g2*g2)."""
    alpha = hp["w_alpha"]
    w = numpy_refresh(st, c, hp, F, k, True) if learn else model.get_state()
    out = {key: st[key].copy() for key in st}
    out["lin_w"], out["vec_w"], out["bias3"][0] = w["lin_w"], w["vec_w"], w["bias3"][0]
    a = Acc(st["bias3"][1], alpha)
    for r in range(c.n_rows):
        a.at(r)
        a.touch(w["bias3"][0], tg[r], f32(tg[r] * tg[r]), True)
    out["bias3"][1], out["bias3"][2] = a.finish_linear(w["bias3"][0], st["bias3"][2])
    row_of = np.repeat(np.arange(c.n_rows), np.diff(c.row_ptr))
    order = np.lexsort((np.arange(len(c.feat)), c.feat))
    L = F * k
    vw = w["vec_w"].reshape(-1, L) if L else None
    byrow = {}
    for p in range(len(c.feat)):
        byrow[(int(row_of[p]), int(c.field[p]))] = p
    lo = 0
    while lo < len(order):
        hi = lo
        while hi < len(order) and c.feat[order[hi]] == c.feat[order[lo]]:
            hi += 1
        i = int(c.feat[order[lo]])
        a = Acc(st["lin_n"][i], alpha)
        for occ, p in enumerate(order[lo:hi]):
            g = f32(tg[row_of[p]] * c.val[p])
            a.at(occ)
            a.touch(w["lin_w"][i], g, f32(g * g), True)
        out["lin_n"][i], out["lin_z"][i] = a.finish_linear(w["lin_w"][i], st["lin_z"][i])
        for fp in range(F if L else 0):
            for f in range(k):
                e = fp * k + f
                wv = vw[i, e]
                a = Acc(st["vec_n"].reshape(-1, L)[i, e], alpha)
                for occ, p in enumerate(order[lo:hi]):
                    r = int(row_of[p])
                    q = byrow.get((r, fp))
                    a.at(occ)
                    if q is None or q == p:
                        continue
                    x = f32(c.val[p] * c.val[q])
                    vp = vw[int(c.feat[q]), int(c.field[p]) * k + f]
                    g = f32(f32(tg[r] * vp) * x)
                    if p < q or learn:
                        a.touch(wv, g, f32(g * g), True)
                    else:
                        g1 = f32(f32(tg[r] * wv) * x)
                        a.touch(wv, g, f32(g * g1), False)
                if a.any:
                    n_, z_ = a.finish_latent(wv, st["vec_z"].reshape(-1, L)[i, e])
                    out["vec_n"].reshape(-1, L)[i, e] = n_
                    out["vec_z"].reshape(-1, L)[i, e] = z_
        lo = hi
    return out


FOLD_CASES = [("FFM", 4, 2, True), ("FFM", 4, 2, False), ("LR", 1, 1, True)]


@pytest.mark.parametrize("mt,F,k,ordered,learn",
                         [pytest.param(*c, False, id="-".join(map(str, c))) for c in FOLD_CASES]
                         + [pytest.param(*c, True, id="learn-" + "-".join(map(str, c))) for c in FOLD_CASES])
def test_numpy_restatement_of_the_fold_agrees_bit_for_bit(mt, F, k, ordered, learn):
    """The reference rule, and the learning variant (FFM_FLAG_LEARN): its refresh restated from the
    start state and its all-plain touches."""
    _fold_case(mt, F, k, ordered, learn, STRESS_HP, "random", strict=True)


@pytest.mark.parametrize("start", ["random", "range_grid"])
@pytest.mark.parametrize("mt,F,k", [("FFM", 4, 2), ("LR", 1, 1)])
@pytest.mark.parametrize("hp_name", [h for h in HP_SETS if h != "stress_hp"])
def test_numpy_restatement_of_the_fold_at_every_hyper_parameter_set(hp_name, mt, F, k, start):
    """The same restatement at every util.HP_SETS entry, from the random start state and from one whose
    n are util.range_grid's (the guard edges of the engine's short square root, 2^118, FLT_MAX)."""
    _fold_case(mt, F, k, True, False, HP_SETS[hp_name], start, strict=False)


def _fold_case(mt, F, k, ordered, learn, hp, start, strict):
    rng = np.random.default_rng(21)
    nf = 24
    m = CpuModel("oracle", mt, nf, F, k, learn=learn, **hp)
    st = rand_state(rng, m, n_hi=1e-4, w_sd=0.5)  # n small, w large: some ffm.cpp:118 roots go negative (NaN)
    if learn:  # four slots in ten have not seen a gradient yet; their w is not W(0, z)
        st["vec_n"][np.random.default_rng(22).random(st["vec_n"].shape) < 0.4] = 0.0
    if start == "range_grid":
        gn = np.unique(range_grid(hp)[0])
        for key in ("lin_n", "vec_n"):
            st[key][...] = gn[np.random.default_rng(23).integers(0, gn.size, st[key].shape)]
    m.set_state(st)
    c = rand_rows(rng, 300, 4, nf, ordered=ordered, zipf=2.0, drop=0.1)
    if mt != "FFM":
        c.field[:] = 0
        # distinct ids per row for LR here (a repeated id makes the feature serial)
        rows = []
        for r in range(c.n_rows):
            seen, row = set(), []
            for p in range(c.row_ptr[r], c.row_ptr[r + 1]):
                if int(c.feat[p]) not in seen:
                    seen.add(int(c.feat[p]))
                    row.append((0, int(c.feat[p]), float(c.val[p])))
            rows.append(row)
        c = Csr.from_rows(rows, c.label)
    logits, _ = m.train_batch(c)
    tg = np.array([f32(m.sigmoid(float(l))) - f32(y) for l, y in zip(logits, c.label)], f32)
    kk = k if mt == "FFM" else 0
    want = numpy_block(m, st, c, tg, hp, F, kk, learn=learn)
    got = m.get_state()
    w = numpy_refresh(st, c, hp, F, kk, learn)
    for key in ("bias3", "lin_w", "vec_w"):
        assert_bitwise(got[key].ravel()[:1] if key == "bias3" else got[key].ravel(),
                       w[key].ravel()[:1] if key == "bias3" else w[key].ravel(), "refresh " + key)
    if mt == "FFM" and not learn and strict:
        assert np.isnan(got["vec_z"]).any(), "the case should reach ffm.cpp:118's NaN"
        assert got["vec_z"].size - np.isnan(got["vec_z"]).sum() > 100
    if mt == "FFM" and learn:
        assert np.isfinite(got["vec_z"]).all() and np.isfinite(got["vec_n"]).all(), "g2*g2: no negative root"
        # the kept-w branch is live: touched slots with n = 0 whose w is not W(0, z) still hold it
        kept = (got["vec_n"] != st["vec_n"]) & (st["vec_n"] == 0) & (got["vec_w"] == st["vec_w"])
        w0 = np.array([ftrl_w(0.0, z, hp) for z in st["vec_z"][kept]], f32)
        assert (w0 != st["vec_w"][kept]).sum() > 20
    for key in ("bias3", "lin_n", "lin_z", "vec_n", "vec_z"):
        assert_bitwise(got[key].ravel(), want[key].ravel(), key)


@pytest.mark.parametrize("F,n_rows,counts", [(8, 6144, "ffm"), (39, 4352, "ffm"), (4, 1024, "fm")])
def test_occurrence_block_builder_hits_every_count_exactly(F, n_rows, counts):
    """The builder the occurrence-class GPU tests use (util.occurrence_block): each listed feature
    occurs exactly its count times, in its own field; every other id occurs once; one entry per field
    and row in field order; the irregular copy keeps every listed count and drops a third of one
    field's entries; every id lies in its field's range."""
    from util import EDGE_COUNTS, FM_EDGE_COUNTS, block_ids_per_field, irregular_copy, occurrence_block
    want = EDGE_COUNTS if counts == "ffm" else FM_EDGE_COUNTS
    blk, ids, field_of = occurrence_block(F, want, n_rows, seed=3)
    per = block_ids_per_field(n_rows)
    assert blk.n_rows == n_rows and blk.row_ptr[-1] == n_rows * F
    assert np.array_equal(blk.field, np.tile(np.arange(F, dtype=np.int32), n_rows))
    assert np.array_equal(blk.feat // per, blk.field)
    u, c = np.unique(blk.feat, return_counts=True)
    got = dict(zip(u.tolist(), c.tolist()))
    assert [got[int(i)] for i in ids] == list(want)
    assert np.array_equal(ids // per, field_of)
    assert len(set(ids.tolist())) == len(want)
    rest = np.setdiff1d(u, ids)
    assert (c[np.isin(u, rest)] == 1).all()
    assert rest.size == n_rows * F - sum(want)
    hist = np.bincount(c)
    assert hist[1] == rest.size + sum(1 for x in want if x == 1)
    for x in set(want) - {1}:
        assert hist[x] == list(want).count(x), x
    irr = irregular_copy(blk, seed=4)
    assert irr.row_ptr[-1] == n_rows * F - n_rows // 3
    u2, c2 = np.unique(irr.feat, return_counts=True)
    got2 = dict(zip(u2.tolist(), c2.tolist()))
    assert [got2[int(i)] for i in ids] == list(want)
    assert np.array_equal(irr.feat // per, irr.field)
    order = [np.all(np.diff(irr.field[irr.row_ptr[r]:irr.row_ptr[r + 1]]) > 0) for r in range(n_rows)]
    assert 0 < order.count(False) < n_rows


def _in_range(blk, nf, F):
    return (blk.feat >= 0) & (blk.feat < nf) & (blk.field >= 0) & (blk.field < F)


@pytest.mark.parametrize("mt", ["FFM", "FM"])
def test_row_length_block_builder_has_every_listed_property(mt):
    """The builder the row-length GPU tests use (util.row_length_block, row_cap_prefixes), for FFM F = 6
    and for FM: every property its docstring lists, asserted from the arrays."""
    from util import (ROW_CAPS, ROW_ERASED_AT, ROW_FIELDS, ROW_IDS_PER_FIELD, ROW_LENGTHS, ROW_POOL,
                      ROW_POSITION_CLASSES, ROW_SEED, row_cap_prefixes, row_length_block)
    F, per, repeats = ROW_FIELDS, ROW_IDS_PER_FIELD, 3
    for seed in (ROW_SEED, ROW_SEED + 1, ROW_SEED + 2):
        blk, nf = row_length_block(mt, F, per, seed)
        assert nf == F * per
        lens = np.diff(blk.row_ptr)
        n_rows = blk.n_rows
        # the ladder, shuffled, between an empty first row and last rows of 0 and 1 entries; one
        # two-entry row more, since 3 * 27 + 3 is a multiple of 4
        assert n_rows == len(ROW_LENGTHS) * repeats + 4 and n_rows % 4 != 0
        assert lens[0] == 0 and lens[-2] == 0 and lens[-1] == 1
        extra = {0: 2, 1: 1, 2: 1}
        for n in ROW_LENGTHS:
            assert (lens == n).sum() == repeats + extra.get(n, 0), n
        assert set(lens.tolist()) == set(ROW_LENGTHS)
        body = lens[2:-2]
        assert (np.diff(body) < 0).any() and (np.diff(body) > 0).any()
        assert blk.label.size == n_rows and set(blk.label.tolist()) == {0, 1}
        row_of = np.repeat(np.arange(n_rows), lens)
        pos = np.arange(lens.sum()) - blk.row_ptr[:-1][row_of]
        ok = _in_range(blk, nf, F if mt == "FFM" else 1)
        # FM / LR: field 0 everywhere; FFM: the field of an id (where it was not put out of range)
        if mt == "FFM":
            fld_ok = (blk.field >= 0) & (blk.field < F)
            assert np.array_equal(blk.field[ok], blk.feat[ok] // per)
            multi = [np.unique(blk.field[blk.row_ptr[r]:blk.row_ptr[r + 1]]).size < lens[r] for r in range(n_rows)
                     if lens[r] >= 8]
            assert all(multi), "fields repeat within a row"
        else:
            assert not blk.field.any()
        # once-only ids and pool ids, both in every position class
        u, inv, cnt = np.unique(blk.feat[ok], return_inverse=True, return_counts=True)
        once = np.zeros(ok.size, bool)
        once[ok] = cnt[inv] == 1
        pooled = ok & (blk.feat % per < ROW_POOL)
        assert 0.42 < once.sum() / ok.sum() < 0.58, once.sum() / ok.sum()
        assert not (once & pooled).sum() > 0.02 * ok.sum()  # (a pool id may happen to occur once)
        assert (ok & ~once & ~pooled).sum() <= 2 * 10  # (only the ids that a row holds twice)
        pool_ids, pool_cnt = np.unique(blk.feat[pooled], return_counts=True)
        assert pool_ids.size > 0.9 * F * ROW_POOL and np.median(pool_cnt) >= 4
        rows_of_pool = [np.unique(row_of[blk.feat == i]).size for i in pool_ids[pool_cnt >= 4][:50]]
        assert min(rows_of_pool) >= 3, "pool features repeat across rows"
        for lo, hi in ROW_POSITION_CLASSES:
            in_class = (pos >= lo) & (pos < hi)
            assert (once & in_class).sum() >= 8 and (pooled & ~once & in_class).sum() >= 8, (lo, hi)
        # the erased entries: in every fifth non-empty row (16 rows), at ROW_ERASED_AT clamped to the
        # row's last entry and nowhere else; ids -7 and n_feats + 3, FFM also fields F + 2 and -1
        bad_rows = np.unique(row_of[~ok])
        assert bad_rows.size == (len(ROW_LENGTHS) - 1) * repeats // 5 + 1
        for r in bad_rows:
            want = sorted({min(p, lens[r] - 1) for p in ROW_ERASED_AT})
            assert pos[~ok & (row_of == r)].tolist() == want, (r, lens[r])
        bad_lens = set(lens[bad_rows].tolist())
        assert {1, 3, 5, 64, 65, 128, 130, 150} <= bad_lens, bad_lens
        assert set(blk.feat[(blk.feat < 0) | (blk.feat >= nf)].tolist()) == {-7, nf + 3}
        if mt == "FFM":
            assert set(blk.field[~fld_ok].tolist()) == {F + 2, -1}
            assert 0 < np.unique(row_of[~fld_ok]).size < bad_rows.size
            assert ((blk.feat[~fld_ok] >= 0) & (blk.feat[~fld_ok] < nf)).all()
        for p in ROW_ERASED_AT:  # a parked position, a chunk, both sides of the 64-entry pass boundary
            assert (~ok & (pos == p) & (lens[row_of] > 64)).any(), p
        # ... and the lengths still count them: a row of more than 128 entries with at most 128 survivors
        nv = np.bincount(row_of[ok], minlength=n_rows)
        assert ((lens > 128) & (nv <= 128)).any() and ((lens > 64) & (nv <= 64)).any()
        assert ((lens == 130) & (nv == 125)).any() and ((lens == 128) & (nv == 123)).any()
        # one id twice, below position 64 and above, in ten rows of at least 66 entries
        twice = 0
        for r in range(n_rows):
            sl = slice(blk.row_ptr[r], blk.row_ptr[r + 1])
            ids, okr = blk.feat[sl], ok[sl]
            uu, cc = np.unique(ids[okr], return_counts=True)
            if (cc > 1).any():
                assert lens[r] >= 66 and (cc > 1).sum() == 1 and cc.max() == 2
                at = np.flatnonzero(okr & (ids == uu[cc > 1][0]))
                assert 5 <= at[0] < 63 and at[1] >= 65
                twice += 1
        assert twice == 10
        # FFM: some rows in descending field order, the others not
        if mt == "FFM":
            desc = [r for r in range(n_rows) if lens[r] >= 8 and r not in set(bad_rows.tolist())
                    and (np.diff(blk.field[blk.row_ptr[r]:blk.row_ptr[r + 1]]) <= 0).all()]
            assert 3 <= len(desc) <= 12
        # values: 1.0 for half of the entries, [0.25, 1.25) otherwise
        assert 0.45 < (blk.val == 1.0).mean() < 0.55
        assert (blk.val >= 0.25).all() and (blk.val < 1.25).all() and blk.val.dtype == np.float32
        # the pieces: rows in a stable order by length, the longest exactly L, an empty row first
        order = np.argsort(lens, kind="stable")
        pieces = list(row_cap_prefixes(blk))
        assert len(pieces) == len(ROW_CAPS) == 8
        for cap, piece in zip(ROW_CAPS, pieces):
            pl = np.diff(piece.row_ptr)
            assert pl.max() == cap and pl[0] == 0 and (np.diff(pl) >= 0).all()
            assert piece.n_rows == (lens <= cap).sum()
            idx = order[:piece.n_rows]
            assert np.array_equal(piece.label, blk.label[idx])
            assert np.array_equal(piece.feat, np.concatenate([blk.feat[blk.row_ptr[r]:blk.row_ptr[r + 1]] for r in idx]))
            assert np.array_equal(piece.val, np.concatenate([blk.val[blk.row_ptr[r]:blk.row_ptr[r + 1]] for r in idx]))
        assert pieces[-1].n_rows == n_rows


def _assert_all_finite(o, logits, what):
    assert np.isfinite(logits).all(), what + ": logits"
    for key, a in o.get_state().items():
        assert np.isfinite(a).all(), "%s: %s" % (what, key)


def test_oracle_stays_finite_on_every_row_length_case():
    """What keeps tests/test_gpu_row_lengths.py from passing on NaNs alone: on every shape of
    util.ROW_SHAPES, from the warm start state, the oracle's logits of both training blocks, its
    predict outputs and its whole state (so every word it touched) are finite -- all of them --; the
    same over the row-cap pieces chained as blocks, for the shapes that run them (util.row_pieces_shape),
    all logits below 16; and training does touch the state."""
    from util import (ROW_ENTRY_SHAPES, ROW_SEED, ROW_SHAPES, row_cap_prefixes, row_length_case, row_pieces_shape,
                      row_shape_id)
    top = 0.0
    for shape in ROW_SHAPES:
        o, st, blocks, _ = row_length_case(shape, ROW_SEED)
        what = row_shape_id(shape)
        for j in (0, 1):
            lg, loss = o.train_batch(blocks[j])
            _assert_all_finite(o, lg, "%s block %d" % (what, j))
            assert np.isfinite(loss)
            top = max(top, float(np.abs(lg).max()))
        after = o.get_state()
        assert sum(int(np.count_nonzero(after[key] != st[key])) for key in after) > 4000
        for prob in (False, True):
            out, loss = o.predict_batch(blocks[2], output_prob=prob)
            assert np.isfinite(out).all() and np.isfinite(loss), what + " predict"
    for shape in ROW_ENTRY_SHAPES:
        shape = row_pieces_shape(shape)
        o, st, blocks, _ = row_length_case(shape, ROW_SEED)
        what = row_shape_id(shape)
        for j in (0, 1):
            for piece in row_cap_prefixes(blocks[j]):
                lg, loss = o.train_batch(piece)
                _assert_all_finite(o, lg, "%s pieces of block %d" % (what, j))
                assert np.isfinite(loss) and np.abs(lg).max() < 16.0, what
        for piece in row_cap_prefixes(blocks[2]):
            out, loss = o.predict_batch(piece)
            assert np.isfinite(out).all() and np.isfinite(loss), what + " predict pieces"
    assert top < 16.0, top  # (sigmoid's argument stays out of the range where a float sigmoid is exactly 1)


GRIDS = dict(special=special_grid, range=range_grid)


@pytest.mark.parametrize("hp", list(HP_SETS.values()), ids=list(HP_SETS))
@pytest.mark.parametrize("mt", ["FFM", "FM"])
@pytest.mark.parametrize("learn", [False, True], ids=["reference", "learn"])
def test_refresh_rule_on_range_grid(mt, learn, hp):
    """test_refresh_rule_on_special_values on util.range_grid."""
    test_refresh_rule_on_special_values(mt, learn, hp, grid="range")


@pytest.mark.parametrize("hp", list(HP_SETS.values()), ids=list(HP_SETS))
@pytest.mark.parametrize("mt", ["FFM", "FM"])
@pytest.mark.parametrize("learn", [False, True], ids=["reference", "learn"])
def test_refresh_rule_on_special_values(mt, learn, hp, grid="special"):
    """The oracle's refresh (mzw_latent, mzw) against util.latent_w / util.ftrl_w on the special
    values: n = +-0, subnormal, FLT_MIN, +inf, NaN; z = +-0, +-l1 and just past it; w_old = -0.0, a
    subnormal, NaN.  Under the learning variant a latent slot with not n > 0 keeps its w, -0.0 and
    subnormals bit for bit; linear terms and the bias keep the reference rule.  At every
    util.HP_SETS entry; test_refresh_rule_on_range_grid runs it on util.range_grid (n on the guard edges
    of the engine's short square root, 2^118, FLT_MAX; |z| = 2^61)."""
    g = grid_block(mt, 4 if mt == "FFM" else 8, hp, grid=GRIDS[grid](hp))
    m = CpuModel("oracle", mt, g["nf"], g["F"], g["k"], learn=learn, **hp)
    m.set_state(g["state"])
    m.train_batch(g["block"])
    got = m.get_state()
    want, want_lin = grid_want(g, hp, learn)
    assert_bitwise(got["vec_w"][g["slots"]], want, "latent w")
    assert_bitwise(got["lin_w"][g["lin"]], want_lin, "linear w")
    if grid == "range":  # (every n > 0: W(n, z) in every slot, under both rules)
        assert (g["n"] > 0).all() and np.count_nonzero(want) > 20
        return
    kept = ~(g["n"][g["idx"]] > 0)
    if learn:  # -0.0, subnormals and NaN kept, the W branch taken elsewhere
        assert (np.signbit(want[kept]) & (want[kept] == 0)).any() and (np.abs(want[kept]) == f32(3e-41)).any()
        assert np.isnan(want[kept]).any() and np.count_nonzero(want[~kept]) > 20
    else:
        assert not (np.abs(want) == f32(3e-41)).any()


@pytest.mark.parametrize("hp", list(HP_SETS.values()), ids=list(HP_SETS))
def test_refresh_rule_is_the_compiled_references(hp):
    """util.ftrl_w (numpy, an IEEE double divide), the oracle's and the compiled reference's
    maybe_zero_weight on every (n, z) of both grids and on subnormal, huge and zero operands: with l1 = 0
    the numerator nextafter(l1) is subnormal, with l2 = 0 and beta = 0 the denominator of n = 0 is zero."""
    if not pyoracle.have_ref():
        pytest.skip("oracle/_ref not built here")
    o = CpuModel("oracle", "LR", 4, **hp)
    r = CpuModel("ref", "LR", 4, **hp)
    pairs = set()
    for grid in GRIDS.values():
        gn, gz, _ = grid(hp)
        pairs.update(zip(bits(gn).tolist(), bits(gz).tolist()))
    ns = np.array([0, 2.0 ** -149, 2.0 ** -97, 2.0 ** -96, 2.0 ** -70, 0.37, 2.0 ** 96, 2.0 ** 118, 3e38], f32)
    l1 = f32(hp["w_l1"])
    zs = np.array([2.0 ** -149, -2.0 ** -149, 1e-40, -3e-39, 0.3, -0.011, 2.0 ** 61, -2.0 ** 61,
                   np.nextafter(l1, f32(np.inf)), -np.nextafter(l1, f32(np.inf))], f32)
    pairs.update((a, b) for a in bits(ns).tolist() for b in bits(zs).tolist())
    pairs = np.array(sorted(pairs), np.uint32)
    n, z = pairs[:, 0].copy().view(f32), pairs[:, 1].copy().view(f32)
    want = np.array([ftrl_w(a, b, hp) for a, b in zip(n, z)], f32)
    assert_bitwise(np.array([r.maybe_zero_weight(a, b) for a, b in zip(n, z)], f32), want, "reference")
    assert_bitwise(np.array([o.maybe_zero_weight(a, b) for a, b in zip(n, z)], f32), want, "oracle")
    if l1 == 0:
        sub = (np.abs(z) < np.finfo(f32).tiny) & (z != 0) & (n > 0) & np.isfinite(n)
        assert sub.sum() > 10 and np.count_nonzero(want[sub]) > 0, "subnormal numerators reach the divide"
    if hp["w_l2"] == 0 and hp["w_beta"] == 0:
        assert np.isinf(want[(n == 0) & (np.abs(z) > l1)]).all(), "x / 0 is inf, as in the reference"


def test_table_of_hyper_parameter_sets_reaches_every_state_of_the_flags():
    """util.HP_SETS: every reachable (fast_div, fast_w), both inclusive ends of both ranges and the
    first float outside each, the zero settings, and the two sets every older test uses."""
    flags = {name: arith_flags(hp) for name, hp in HP_SETS.items()}
    assert set(flags.values()) == {(1, 1), (1, 0), (0, 0)}
    assert HP_SETS["default_hp"] is DEFAULT_HP and HP_SETS["stress_hp"] is STRESS_HP
    lo, hi = f32(2.0 ** -30), f32(2.0 ** 30)
    alphas = {f32(hp["w_alpha"]) for hp in HP_SETS.values()}
    assert {lo, hi, np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf)), f32(3e-38), f32(1.3 * 2.0 ** 31)} <= alphas
    lo, hi = f32(2.0 ** -40), f32(2.0 ** 40)
    betas = {f32(hp["w_beta"]) for hp in HP_SETS.values() if arith_flags(hp)[0]}
    assert {f32(0), lo, hi, np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf)), f32(1.4e-38)} <= betas
    for name, want in (("alpha_2m30", (1, 1)), ("alpha_2p30", (1, 1)), ("alpha_below_2m30", (0, 0)),
                       ("alpha_above_2p30", (0, 0)), ("beta_2m40", (1, 1)), ("beta_2p40", (1, 1)),
                       ("beta_below_2m40", (1, 0)), ("beta_above_2p40", (1, 0)), ("beta_zero", (1, 0))):
        assert flags[name] == want, name
    assert any(hp["w_l1"] == 0 for hp in HP_SETS.values()) and any(hp["w_l2"] == 0 for hp in HP_SETS.values())
    for hp in HP_SETS.values():  # (exactly the float32 the engine gets, but for the two older sets)
        assert all(np.float32(v) == v for v in hp.values()) or hp in (DEFAULT_HP, STRESS_HP)


# The operands with which tests/test_gpu_arith_paths.py tells each guard of the short divide from its
# absence: (alpha, x) with x outside the guard -- or alpha outside [2^-30, 2^30] -- and other bits.
DIV_DISCRIMINATORS = dict(
    below_2m60=(1e-4, f32(1.4e-38)),         # beta + sqrt(0) with beta = 1.4e-38: under div_fast_ok's 2^-60
    alpha_out_of_range=(3e-38, f32(2.0 ** 59)),  # sqrt(2^118): inside div_fast_ok, x * (1 / alpha) overflows
    above_2p60=(2.0 ** -30, f32(2.0 ** 100)))    # beta = 2^100: over div_fast_ok's 2^60, x * 2^30 overflows


def test_short_divide_is_the_ieee_divide_inside_its_guards_and_not_outside():
    """fo_div_alpha_fast (the engine's div_alpha_fast, restated with explicit fmaf) against x / alpha:
    no differing bits for any alpha of util.HP_SETS in [2^-30, 2^30] over x = +-2^e * significand, e from
    -60 to 60 in steps of 5 and the guard's last binade, 2^16 significands each (the top and bottom 2^14
    of the binade and a random rest) -- the rounding of the quotient depends on the significands only
    while nothing under- or overflows, which is why the engine's create-time proof checks one pair of
    binades.  And outside each guard an operand that does give other bits."""
    rng = np.random.default_rng(3)
    sig = np.concatenate([np.arange(1 << 14), (1 << 23) - 1 - np.arange(1 << 14),
                          rng.integers(0, 1 << 23, (1 << 16) - (1 << 15))]).astype(np.uint32)
    assert sig.size == 1 << 16
    exps = sorted(set(range(-60, 60, 5)) | {59})  # (and 2^60 itself, the guard's last value, below)
    x = np.concatenate([((np.uint32(e + 127) << np.uint32(23)) | sig).view(f32) for e in exps] + [f32([2.0 ** 60, 0.0])])
    x = np.concatenate([x, -x[:-1]])
    assert div_fast_ok(x).all() and x.size >= 2 * len(exps) << 16
    alphas = sorted({f32(hp["w_alpha"]) for hp in HP_SETS.values() if arith_flags(hp)[0]})
    assert len(alphas) >= 7 and f32(2.0 ** -30) in alphas and f32(2.0 ** 30) in alphas
    for a in alphas:
        quick, exact = pyoracle.div_alpha_fast(a, x)
        with np.errstate(all="ignore"):
            assert_bitwise(exact, x / a, "the C divide is numpy's, alpha = %r" % a)
        assert_bitwise(quick, exact, "alpha = %r" % a)
        assert np.isfinite(exact).all()
    for name, (a, v) in DIV_DISCRIMINATORS.items():
        quick, exact = pyoracle.div_alpha_fast(a, np.array([v], f32))
        in_guard = bool(div_fast_ok(v)) and arith_flags(dict(w_alpha=a, w_beta=1.0))[0] == 1
        assert not in_guard, name
        assert bits(quick)[0] != bits(exact)[0] and not (np.isnan(quick[0]) and np.isnan(exact[0])), (
            name, quick, exact)
