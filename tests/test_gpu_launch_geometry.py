"""Forced launch grids, workgroup sizes, LDS parking, range order and stream use (the engine's FFM_*
switches, read when an engine is created) against the oracle, bit for bit.

At the default grids a bitwise test gives each wave of the update launches one or two items, so the
third and later trips of their loops -- and the hot and few-occurrence ranges' list entry requested
two items ahead -- would go unnoticed if they were wrong.  Here the grids are forced down to the
`sized()` floors (engine_step.h) and to uneven values just above them, on blocks long enough that
every targeted loop takes at least three trips per wave (or workgroup): the forced-grid cases
(update grids, wide launch, the row-order walk, compact shards) restate the item counts from the
block and the workgroup counts the engine launches, and assert that first.  The other cases (range
order, serial engine, row kernel, parking, evaluation, staged blocks) pin a switch each on the same
blocks without restating trips.

Every case: logits, loss sum and the whole state bit for bit (NaN positions included) against
oracle.pyoracle.CpuModel from the same start state; the oracle's result is computed once per block
and start state (a module-scoped cache) and every variant is compared with it.
"""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import CpuModel, Csr
from util import (EDGE_COUNTS, STRESS_HP, assert_bitwise, assert_rank_rows, assert_state_bitwise,
                  block_ids_per_field, fast_state, get_bias3, irregular_copy, keep_columns, kept_copy,
                  occurrence_block, run_rank_staged)

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-12  # (test_gpu_parity.py: the loss sum's per-row terms are summed in another order)

def _loss_close(a, b):
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= LOSS_RTOL * max(1.0, abs(b)) * 64


# ---- the engine's launch geometry, restated (engine_step.h, kernels_tile.h, kernels_update.h) -----
SMALL_MAX, HUGE_MIN, GIANT_MIN, SUPER_MIN, RANGE = 10, 128, 257, 2048, 256
UPD_WAVES, WIDE_WAVES, TERMS_CAP = 4, 8, 2048
DEFAULT_GRIDS = dict(hot=2048, small=768, walk=256, giant=1024)
FLOOR = dict(hot=1, small=1, walk=1, giant=1)
# uneven, just above the floors (hot / small 64, walk 16 workgroups; the super pass and the join take
# grid_giant as it is, so 5 = 20 waves): 37 everywhere would be clamped back to the floors of the hot
# and few-occurrence ranges.  (giant = 5 leaves the giant range's workgroups -- ffm_coop_items -- at
# their floor of 32: COOP_UNEVEN gives them 37, the super pass and the join 148 waves.)
UNEVEN = dict(hot=67, small=67, walk=17, giant=5)
COOP_UNEVEN = dict(hot=1, small=1, walk=1, giant=37)


def cdiv(a, b):
    return -(-a // b)


def per_feat(F, k):
    """Chunks of 64 elements per stored record of a whole model (tile_geom)."""
    if k <= 64:
        return cdiv(F, 64 // k)
    return F * cdiv(k, 64)


def serial_features(blk):
    """Per distinct feature (np.unique order): does it have a serial slot?  Its cmask is not 0
    (kernels_group.h) when a row that holds it holds two entries of one field (a whole model owns
    every field pair)."""
    lens = np.diff(blk.row_ptr)
    row_of = np.repeat(np.arange(blk.n_rows), lens)
    F = int(blk.field.max()) + 1
    per_row_field = np.bincount(row_of.astype(np.int64) * F + blk.field, minlength=blk.n_rows * F)
    twice_row = (per_row_field.reshape(blk.n_rows, F) >= 2).any(axis=1)
    u, inv = np.unique(blk.feat, return_inverse=True)
    return np.bincount(inv, weights=twice_row[row_of].astype(np.float64), minlength=u.size) > 0


def classes(blk):
    c = np.unique(blk.feat, return_counts=True)[1]
    serial = serial_features(blk)
    return dict(few=int(((c >= 2) & (c <= SMALL_MAX)).sum()),
                serial_multi=int((serial & (c >= 2)).sum()),
                big=int(((c > SMALL_MAX) & (c <= HUGE_MIN)).sum()),
                huge=int(((c > HUGE_MIN) & (c < GIANT_MIN)).sum()),
                giant=int((c >= GIANT_MIN).sum()),
                ranges=int(sum(cdiv(int(x), RANGE) for x in c if x >= SUPER_MIN)),
                supers=int((c >= SUPER_MIN).sum()))


def update_trips(blk, F, k, grids, wide=False):
    """{loop: (items, waves or workgroups, fewest trips of one)} of a whole model's update launches.
    The row-order walk's items are its 64-feature groups over the multi-occurrence lists that hold a
    feature with a serial slot (the others are an empty ballot): at least cdiv(serial features, 64),
    in whatever order the grouping lists them."""
    nnz = int(blk.row_ptr[-1])
    cl = classes(blk)
    pf = per_feat(F, k)
    wpb = WIDE_WAVES if wide else UPD_WAVES
    scale = wpb // UPD_WAVES

    def sized(grid, per_wg, least):
        return max(least, min(grid, cdiv(nnz, per_wg)))
    nt = cdiv(sized(grids["hot"], 32, 64), scale)
    ns = cdiv(sized(grids["small"], 128, 64), scale)
    nw = cdiv(sized(grids["walk"], 1024, 16), scale)
    ng = sized(grids["giant"], 256, 32)
    gg = grids["giant"]
    loops = {
        "ffm_tile_items (waves)": ((cl["big"] + cl["huge"]) * pf, nt * wpb),
        "ffm_small_body (waves)": (cl["few"], ns * wpb),
        WALK: (cdiv(cl["serial_multi"], 64), nw * wpb),
        "ffm_coop_items (workgroups)": (cl["giant"] * pf, ng),
        "ffm_range_items_b (waves)": (cl["ranges"] * pf, gg * UPD_WAVES),
        "ffm_range_join (waves)": (cl["giant"] * pf, gg * UPD_WAVES),
    }
    return {name: (items, n, items // n) for name, (items, n) in loops.items()}


WALK = "ffm_generic_body walk (waves, 64-feature groups with serial slots)"
RANGES = ("ffm_tile_items (waves)", "ffm_small_body (waves)", "ffm_coop_items (workgroups)",
          "ffm_range_items_b (waves)", "ffm_range_join (waves)")


def assert_three_trips(trips, what, loops=RANGES):
    short = {name: t for name, t in trips.items() if name in loops and t[2] < 3}
    assert not short, "%s: loops under three trips per wave / workgroup (items, waves, trips): %r" % (what, short)


# ---- blocks -----------------------------------------------------------------------------------------
# (18 fields: a partial last chunk at k = 4, 8 and 16 -- lanes past a record's last slot; 39 would make a
# k = 16 state 2.4 GB)
F_BIG, ROWS = 18, 12288


def _cycle(pattern, n):
    return [pattern[i % len(pattern)] for i in range(n)]


def geometry_counts():
    """Occurrence counts of the whole-model blocks: 12900 few-occurrence features (mostly two), 820 hot
    and very hot ones (268 waves x 3), 89 giants and 11 supers (k = 16 at COOP_UNEVEN: 100 giants x 5 chunks for
    three trips of 148 waves; 109 ranges), the class edges among them.  One entry per field and row:
    no serial slots (the walk has its own block)."""
    few = _cycle([2] * 16 + [3, 5, 9, 10], 12900)
    hot = _cycle([11, 11, 12, 12, 13, 15, 16, 17], 812) + [31, 32, 33, 127, 128, 129, 255, 256]
    giant = _cycle([257, 258, 260, 270, 300], 80) + [400, 511, 512, 513, 700, 1000, 1500, 2047, 258]
    supers = [2048, 2049, 2600, 2600, 2600, 2600, 3000, 2100, 2100, 2100, 2100]
    return few + hot + giant + supers


@functools.lru_cache(maxsize=1)
def geometry_block():
    """The irregular copy of the occurrence block (a third of one field's entries gone, some rows in
    reverse field order): the general folds, and the one-launch kind decode over every range."""
    regular, _, _ = occurrence_block(F_BIG, geometry_counts(), ROWS, seed=41)
    return irregular_copy(regular, seed=41)


def test_geometry_block_reaches_three_trips():
    blk = geometry_block()
    for k in (4, 8, 16):
        for grids in (FLOOR, UNEVEN):
            assert_three_trips(update_trips(blk, F_BIG, k, grids), "k=%d %r" % (k, grids))
            assert_three_trips(update_trips(blk, F_BIG, k, grids, wide=True), "k=%d wide %r" % (k, grids))
    assert_three_trips(update_trips(blk, F_BIG, 16, COOP_UNEVEN), "k=16 %r" % COOP_UNEVEN)
    assert classes(blk)["serial_multi"] == 0
    wb = walk_block()
    for grids in (FLOOR, UNEVEN):
        assert_three_trips(update_trips(wb, F_ROW, 16, grids), "walk block %r" % grids, loops=(WALK,))
    # (the default grids give one or two: what the other suites run)
    t = update_trips(blk, F_BIG, 16, DEFAULT_GRIDS)
    assert t["ffm_tile_items (waves)"][2] < 3 and t["ffm_coop_items (workgroups)"][2] < 3


def ragged_block(F, n_rows, n_feats_per_field, seed, uniform=0.0):
    """Rows of 20..40 entries with two or three entries in many fields (serial slots: the row-order
    walk), every 64th row 66..80 entries (more than TERMS_CAP pairs: the row kernel takes several
    passes); ids Zipf-like within their field (a fraction `uniform` of them uniform instead), so
    features repeat across rows (never within one)."""
    rng = np.random.default_rng(seed)
    row_ptr, field, feat, val = [0], [], [], []
    per = n_feats_per_field
    for r in range(n_rows):
        n = int(rng.integers(66, 81)) if r % 64 == 5 else int(rng.integers(20, 41))
        f = np.sort(rng.integers(0, F, n)).astype(np.int32)
        if r % 7 == 3:
            f = f[::-1].copy()
        i = np.minimum((rng.pareto(1.1, n) * 3).astype(np.int64), per - 1)
        if uniform > 0:
            flat = rng.random(n) < uniform
            i[flat] = rng.integers(0, per, int(flat.sum()))
        while True:  # (a feature at most once per row)
            dup = np.ones(n, bool)
            dup[np.unique(f.astype(np.int64) * per + i, return_index=True)[1]] = False
            if not dup.any():
                break
            i[dup] = rng.integers(0, per, int(dup.sum()))
        field.append(f)
        feat.append((f.astype(np.int64) * per + i).astype(np.int32))
        v = (rng.random(n) + 0.25).astype(np.float32)
        v[rng.random(n) < 0.5] = 1.0
        val.append(v)
        row_ptr.append(row_ptr[-1] + n)
    label = (rng.random(n_rows) < 0.4).astype(np.int32)
    return Csr(np.array(row_ptr, np.int32), np.concatenate(field), np.concatenate(feat),
               np.concatenate(val), label)


F_ROW, ROWS_RAGGED, PER_RAGGED, MAX_ROW = 39, 1536, 200, 80


@functools.lru_cache(maxsize=1)
def row_block():
    return ragged_block(F_ROW, ROWS_RAGGED, PER_RAGGED, seed=43)


WALK_ROWS, WALK_PER = 8192, 700


@functools.lru_cache(maxsize=1)
def walk_block():
    """Ragged rows over a small id space (39 fields x 700 ids): nearly every feature occurs several
    times in rows that hold two entries of one field, so the row-order walk has thousands of
    serial-slot features to fold."""
    return ragged_block(F_ROW, WALK_ROWS, WALK_PER, seed=47, uniform=0.6)


def test_ragged_block_has_serial_slots_and_long_rows():
    blk = row_block()
    lens = np.diff(blk.row_ptr)
    assert lens.max() <= MAX_ROW and (lens * (lens - 1) // 2 > TERMS_CAP).sum() >= 20
    # rows touching one field two or three times: the slots the row-order walk folds
    row_of = np.repeat(np.arange(blk.n_rows), lens)
    dup = np.unique(row_of.astype(np.int64) * F_ROW + blk.field, return_counts=True)[1]
    assert (dup >= 2).sum() >= 5000 and (dup >= 3).sum() >= 1000


# ---- the oracle, once per block and start state -------------------------------------------------------
_ORACLE = {}


def _oracle(key, make):
    if key not in _ORACLE:
        if len(_ORACLE) >= 3:  # (host memory: a k = 16 whole-model state is 0.8 GB)
            _ORACLE.pop(next(iter(_ORACLE)))
        _ORACLE[key] = make()
    return _ORACLE[key]


def _whole_model(k):
    """(start state, oracle logits, loss, final state) of the geometry block at k, stress
    hyper-parameters, n near 0 and a fifth of vec_n zero."""
    def make():
        nf = F_BIG * block_ids_per_field(ROWS)
        o = CpuModel("oracle", "FFM", nf, F_BIG, k, **STRESS_HP)
        st = fast_state(np.random.default_rng(600 + k), o, n_hi=0.02, n_zero=0.2)
        o.set_state(st)
        lo, so = o.train_batch(geometry_block())
        fin = o.get_state()
        assert np.isnan(fin["vec_z"]).any(), "the NaNs must reach the folds"
        return st, lo, so, fin
    return _oracle(("whole", k), make)


def _engine_whole(k, **kw):
    nf = F_BIG * block_ids_per_field(ROWS)
    fs = (np.arange(F_BIG + 1) * block_ids_per_field(ROWS)).astype(np.int32)
    return fa.Engine("FFM", nf, F_BIG, k, skip_init=True, max_batch_rows=ROWS, max_batch_nnz=ROWS * F_BIG,
                     max_row_nnz=F_BIG, field_start=fs, **STRESS_HP, **kw)


def _check_train(e, blk, want, what):
    st, lo, so, fin = want
    e.set_state(st)
    lg, sg = e.train_batch(blk)
    assert_bitwise(lg, lo, what + " logits")
    if np.isnan(so):
        assert np.isnan(sg), what
    else:
        assert abs(sg - so) <= 1e-9 * max(1.0, abs(so)), (what, sg, so)
    assert_state_bitwise(e.get_state(), fin, what)


GRID_SWITCHES = dict(hot="FFM_GRID_HOT", small="FFM_GRID_SMALL", walk="FFM_GRID_WALK", giant="FFM_GRID_GIANT")


def _set_grids(monkeypatch, grids):
    for name, v in grids.items():
        monkeypatch.setenv(GRID_SWITCHES[name], str(v))


# ---- update grids -------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
@pytest.mark.parametrize("grids", ["floor", "uneven"])
@pytest.mark.parametrize("k", [4, 8, 16])
def test_forced_update_grids(k, grids, split, monkeypatch):
    """FFM_GRID_HOT / SMALL / WALK / GIANT at the floors (the super pass and the join on ONE
    workgroup) and uneven, k = 4 / 8 / 16 (the three FTRL_LAUNCH_ALL instantiations), the update as
    one launch and as three side by side."""
    g = FLOOR if grids == "floor" else UNEVEN
    blk = geometry_block()
    assert_three_trips(update_trips(blk, F_BIG, k, g), "k=%d %s" % (k, grids))
    _set_grids(monkeypatch, g)
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    e = _engine_whole(k)
    _check_train(e, blk, _whole_model(k), "grids %s k=%d split=%s" % (grids, k, split))
    e.close()


@pytest.mark.parametrize("grids", ["floor", "uneven"])
def test_forced_update_grids_wide_launch(grids, monkeypatch):
    """k = 16 on the eight-wave launch (FFM_WIDE_NNZ above the block: kWideWaves workgroups, their
    sizes halved in workgroups, the giant range's waves fold together eight at a time)."""
    g = FLOOR if grids == "floor" else UNEVEN
    blk = geometry_block()
    assert_three_trips(update_trips(blk, F_BIG, 16, g, wide=True), "wide " + grids)
    _set_grids(monkeypatch, g)
    monkeypatch.setenv("FFM_UPDATE_SPLIT", "0")
    monkeypatch.setenv("FFM_WIDE_NNZ", str(int(blk.row_ptr[-1]) + 1))
    e = _engine_whole(16)
    _check_train(e, blk, _whole_model(16), "wide grids " + grids)
    e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
@pytest.mark.parametrize("order", ["210", "201", "120", "102", "021", "012", "112"])
def test_update_range_order_at_floor_grids(order, split, monkeypatch):
    """Every FFM_UPDATE_ORDER permutation of the giant / hot / few ranges (the one launch's range
    decode), and one invalid value (112: would run the hot range twice) that must act as the
    default."""
    _set_grids(monkeypatch, FLOOR)
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    monkeypatch.setenv("FFM_UPDATE_ORDER", order)
    e = _engine_whole(16)
    _check_train(e, geometry_block(), _whole_model(16), "order %s split=%s" % (order, split))
    e.close()


def test_serial_engine(monkeypatch):
    """FFM_ENGINE_SERIAL=1: every launch on the main stream, at the floor grids."""
    _set_grids(monkeypatch, FLOOR)
    monkeypatch.setenv("FFM_ENGINE_SERIAL", "1")
    monkeypatch.setenv("FFM_UPDATE_SPLIT", "2")
    e = _engine_whole(16)
    _check_train(e, geometry_block(), _whole_model(16), "serial")
    e.close()


def _walk_model():
    def make():
        nf = F_ROW * WALK_PER
        o = CpuModel("oracle", "FFM", nf, F_ROW, 16, **STRESS_HP)
        st = fast_state(np.random.default_rng(650), o, n_hi=0.02, n_zero=0.2)
        o.set_state(st)
        lo, so = o.train_batch(walk_block())
        return st, lo, so, o.get_state()
    return _oracle(("walk",), make)


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
@pytest.mark.parametrize("grids", ["floor", "uneven"])
def test_forced_grids_serial_slot_walk(grids, split, monkeypatch):
    """The row-order walk of serial slots (rows with two or three entries of one field) at the floor
    and the uneven grids: every wave of the walk range takes at least three 64-feature groups that
    hold serial-slot features."""
    g = FLOOR if grids == "floor" else UNEVEN
    blk = walk_block()
    assert_three_trips(update_trips(blk, F_ROW, 16, g), "walk " + grids, loops=(WALK,))
    _set_grids(monkeypatch, g)
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    e = fa.Engine("FFM", F_ROW * WALK_PER, F_ROW, 16, skip_init=True, max_batch_rows=WALK_ROWS,
                  max_row_nnz=MAX_ROW, **STRESS_HP)
    _check_train(e, blk, _walk_model(), "walk grids %s split=%s" % (grids, split))
    e.close()


@pytest.mark.parametrize("split", ["0", "2"], ids=["one_launch", "three_side_by_side"])
def test_forced_update_grids_uneven_coop(split, monkeypatch):
    """k = 16 with the giant range on 37 workgroups (ffm_coop_items uneven; the super pass and the
    join on 148 waves)."""
    blk = geometry_block()
    assert_three_trips(update_trips(blk, F_BIG, 16, COOP_UNEVEN), "coop uneven")
    _set_grids(monkeypatch, COOP_UNEVEN)
    monkeypatch.setenv("FFM_UPDATE_SPLIT", split)
    e = _engine_whole(16)
    _check_train(e, blk, _whole_model(16), "coop uneven split=%s" % split)
    e.close()


# ---- the row kernel: workgroup size, refresh mode, LDS parking ------------------------------------
def _row_model(k):
    def make():
        nf = F_ROW * PER_RAGGED
        o = CpuModel("oracle", "FFM", nf, F_ROW, k, **STRESS_HP)
        st = fast_state(np.random.default_rng(700 + k), o, n_hi=0.02, n_zero=0.2)
        o.set_state(st)
        lo, so = o.train_batch(row_block())
        return st, lo, so, o.get_state()
    return _oracle(("row", k), make)


def _engine_row(k):
    return fa.Engine("FFM", F_ROW * PER_RAGGED, F_ROW, k, skip_init=True, max_batch_rows=ROWS_RAGGED,
                     max_row_nnz=MAX_ROW, **STRESS_HP)


@pytest.mark.parametrize("refresh", ["3", "0"], ids=["parking_on", "refresh_pass"])
@pytest.mark.parametrize("threads", ["64", "128", "192", "256"])
def test_row_kernel_workgroup_size(threads, refresh, monkeypatch):
    """FFM_ROW_THREADS 64 / 128 / 192 / 256 with the once-only features refreshed and updated by their
    row (refresh mode 3, parking on) and with the refresh pass (FFM_ENGINE_ROW_REFRESH=0): ragged rows
    with serial slots, rows of more than TERMS_CAP pairs."""
    monkeypatch.setenv("FFM_ROW_THREADS", threads)
    monkeypatch.setenv("FFM_ENGINE_ROW_REFRESH", refresh)
    e = _engine_row(16)
    _check_train(e, row_block(), _row_model(16), "row threads %s refresh %s" % (threads, refresh))
    e.close()


@pytest.mark.parametrize("park", ["0", "16", "96", "1024", "default", "budget_48k", "96_at_64_threads"])
@pytest.mark.parametrize("k", [8, 16])
def test_row_kernel_parking(k, park, monkeypatch):
    """FFM_ROW_PARK none / one vector / 96 bytes / 1024 / the default, FFM_ROW_PARK_BUDGET=49152 (above
    32 KB: the row kernels' LDS attribute is raised when the engine is created), and 96 bytes at 64
    threads -- each read when the engine is created."""
    monkeypatch.setenv("FFM_ENGINE_ROW_REFRESH", "3")
    if park == "budget_48k":
        monkeypatch.setenv("FFM_ROW_PARK_BUDGET", "49152")
    elif park == "96_at_64_threads":
        monkeypatch.setenv("FFM_ROW_PARK", "96")
        monkeypatch.setenv("FFM_ROW_THREADS", "64")
    elif park != "default":
        monkeypatch.setenv("FFM_ROW_PARK", park)
    e = _engine_row(k)
    _check_train(e, row_block(), _row_model(k), "park %s k=%d" % (park, k))
    e.close()


# ---- evaluation ---------------------------------------------------------------------------------------
def _eval_model():
    def make():
        nf = F_ROW * PER_RAGGED
        o = CpuModel("oracle", "FFM", nf, F_ROW, 16, **STRESS_HP)
        st = fast_state(np.random.default_rng(800), o, n_add=0.05)  # warm: the predictions stay finite
        o.set_state(st)
        blk = row_block()
        o.train_batch(blk.rows(0, 768))
        lo, loss = o.predict_batch(blk)
        po, _ = o.predict_batch(blk, output_prob=True)
        halves = sum(o.predict_batch(blk.rows(a, b))[1] for a, b in ((0, 768), (768, ROWS_RAGGED)))
        return st, lo, po, loss, halves
    return _oracle(("eval",), make)


@pytest.mark.parametrize("switch", ["default", "EVAL_DEFER=0", "PREDICT_WAVE=0", "PREDICT_WAVE=1"])
def test_predict_after_training(switch, monkeypatch):
    """Evaluation after a training block: ffm_engine_predict_batch's logits and probabilities bit for
    bit, and the pipelined evaluation -- predict_batch_async, whose block is launched by the next
    call (deferred) or at once (FFM_EVAL_DEFER=0), its loss summed into train_flush -- within
    LOSS_RTOL of the oracle's; FFM_PREDICT_WAVE 0 / 1: rows through the workgroup-per-row kernel / a
    wave per row."""
    if switch != "default":
        name, v = switch.split("=")
        monkeypatch.setenv({"EVAL_DEFER": "FFM_EVAL_DEFER", "PREDICT_WAVE": "FFM_PREDICT_WAVE"}[name], v)
    st, lo, po, loss, halves = _eval_model()
    blk = row_block()
    e = _engine_row(16)
    e.set_state(st)
    e.train_batch(blk.rows(0, 768))
    lg, lsg = e.predict_batch(blk)
    pg, _ = e.predict_batch(blk, output_prob=True)
    assert_bitwise(lg, lo, switch + " logits")
    assert_bitwise(pg, po, switch + " probabilities")
    assert _loss_close(lsg, loss), (switch, lsg, loss)
    e.predict_batch_async(blk.rows(0, 768))
    e.predict_batch_async(blk.rows(768, ROWS_RAGGED))  # (launches the first when it was deferred)
    got = e.train_flush()
    assert _loss_close(got, halves), (switch, "pipelined", got, halves)
    e.close()


# ---- staged blocks: pull grid, the super count read while possibly pending --------------------------------
def _staged_model():
    """Two staged blocks: the geometry block (supers) and its first 4096 rows (no supers); warm state
    so that the second block stays finite."""
    def make():
        nf = F_BIG * block_ids_per_field(ROWS)
        o = CpuModel("oracle", "FFM", nf, F_BIG, 16, **STRESS_HP)
        st = fast_state(np.random.default_rng(900), o, n_add=0.05)
        o.set_state(st)
        blocks = _staged_blocks()
        logits = [o.train_batch(b)[0] for b in blocks]
        return st, logits, o.get_state()
    return _oracle(("staged",), make)


def _staged_blocks():
    blk = geometry_block()
    return [blk, blk.rows(0, 4096)]


def _own_pages(c):
    def cp(a):
        out = fa.page_aligned(a.size, a.dtype)
        out[:] = a
        return out
    return Csr(cp(c.row_ptr), cp(c.field), cp(c.feat), cp(c.val), cp(c.label))


@pytest.mark.parametrize("switch", ["SUPER_WAIT=0", "GRID_PULL=1", "GRID_PULL=5"])
@pytest.mark.parametrize("zero_copy", [False, True], ids=["copied", "zero_copy"])
def test_staged_blocks(switch, zero_copy, monkeypatch):
    """FFM_SUPER_WAIT=0 (the block's super count read without waiting for its grouping: pending or
    not, the supers must run when there are any) and FFM_GRID_PULL 1 / 5 (the staged block's upload),
    on staged blocks with and without supers, copied and zero-copy."""
    name, v = switch.split("=")
    monkeypatch.setenv({"SUPER_WAIT": "FFM_SUPER_WAIT", "GRID_PULL": "FFM_GRID_PULL"}[name], v)
    st, logits, fin = _staged_model()
    blocks = _staged_blocks()
    assert classes(blocks[0])["supers"] > 0 and classes(blocks[1])["supers"] == 0
    e = _engine_whole(16)
    e.set_state(st)
    if zero_copy:
        blocks = [_own_pages(b) for b in blocks]
        for b in blocks:
            e.pin_block(b)
    out = torch.zeros(ROWS, dtype=torch.float32, device="cuda")
    for b in blocks:
        e.stage_batch(b, zero_copy)
    got = []
    for b in blocks:
        e.train_staged(out.data_ptr())
        e.sync()
        got.append(out[:b.n_rows].cpu().numpy().copy())
    for i, (x, y) in enumerate(zip(got, logits)):
        assert_bitwise(x, y, "%s block %d logits" % (switch, i))
    assert_state_bitwise(e.get_state(), fin, switch)
    e.close()
    if zero_copy:
        for b in blocks:
            e.unpin_block(b)


# ---- compact shards: the flat few-occurrence kernel in many rounds ---------------------------------------
S_F, S_K, S_SHARDS, S_ROWS = 39, 16, 8, 4352


def _shard_counts():
    return list(EDGE_COUNTS) + _cycle([2, 3, 4, 5, 6, 7, 8, 9, 10], 3000)


def _shard_setup():
    def make():
        per = block_ids_per_field(S_ROWS)
        nf = S_F * per
        o = CpuModel("oracle", "FFM", nf, S_F, S_K, **STRESS_HP)
        st = fast_state(np.random.default_rng(400), o, n_add=0.05)
        o.set_state(st)
        blocks = [occurrence_block(S_F, _shard_counts(), S_ROWS, seed=500 + s)[0] for s in range(2)]
        logits = [o.train_batch(b)[0] for b in blocks]
        want = o.get_state()
        return st, blocks, logits, want
    return _oracle(("shards",), make)


@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("which", ["bias_owner", "other"])
def test_compact_shard_flat_kernel_rounds(which, grid, monkeypatch):
    """FFM_GRID_SMALL 1 / 3 on two of the eight ranks of test_every_edge_count_on_eight_compact_shards'
    setup (the bias owner and one other), with 3000 more few-occurrence features: the flat kernel's
    lanes take at least three rounds (its record span is at least k / 4 vectors)."""
    monkeypatch.setenv("FFM_GRID_SMALL", grid)
    st, blocks, logits, want = _shard_setup()
    per = block_ids_per_field(S_ROWS)
    nf = S_F * per
    plan = fa.shard_plan(S_F, S_SHARDS, field_map=True)
    r = plan["bias_owner"] if which == "bias_owner" else (plan["bias_owner"] + 3) % S_SHARDS
    keep = keep_columns(plan, r)
    kept = [kept_copy(b, keep) for b in blocks]
    for b in kept:
        few = classes(b)["few"]
        rounds = cdiv(few * (S_K // 4), int(grid) * 256)
        assert rounds >= 3, (few, rounds)
    fs = (np.arange(S_F + 1) * per).astype(np.int32)
    e = fa.Engine("FFM", nf, S_F, S_K, skip_init=True, max_batch_rows=S_ROWS, max_batch_nnz=S_ROWS * S_F,
                  n_shards=S_SHARDS, shard_rank=r, max_row_nnz=S_F, field_start=fs, **STRESS_HP)
    e.set_state(st)
    run_rank_staged(e, kept, logits)
    ids = np.arange(nf, dtype=np.int32)
    assert_rank_rows(e, r, ids, ids // per, want, plan, S_K, "grid_small %s" % grid)
    if r == plan["bias_owner"]:
        assert_bitwise(get_bias3(e), want["bias3"], "bias3")
    e.close()


def teardown_module():
    _ORACLE.clear()
    for f in (geometry_block, row_block, walk_block):
        f.cache_clear()
