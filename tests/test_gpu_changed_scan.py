"""ffm_engine_changed_features (csrc/kernels_scan.h): the device scan that lists the features which no
longer hold what ffm_engine_create gave them.  Every comparison is of bit patterns and exact: a fresh
engine reports nothing (the scan's draw is create's), a single poked word reports exactly its feature,
and after training the list is the numpy predicate over the oracle's final state."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import CpuModel
from scan_util import expected_changed, fresh_state, without_fields
from util import DEFAULT_HP, STRESS_HP, assert_state_bitwise, bits

gpu = pytest.mark.gpu

# (model type, n_fields, n_factors, n_feats): FFM with 16-byte aligned records and with row_len = 15 (the
# scalar path), FM with four vectors per record and with k = 65 (scalar), LR at the bitmap-word edges of
# either word width
SHAPES = ([("FFM", 5, 4, 97), ("FFM", 5, 3, 97), ("FM", 1, 8, 33), ("FM", 1, 65, 33)]
          + [("LR", 1, 1, n) for n in (1, 31, 32, 33, 63, 64, 65)])
INITS = [(42, 0.0, 0.02), (7, 0.0, 0.02), (7, 0.25, 0.05)]  # (seed, init_mean, init_stddev)


def shape_id(s):
    return "%s-F%d-k%d-n%d" % s


def engine(shape, seed=42, mean=0.0, stddev=0.02, **kw):
    mt, F, k, nf = shape
    return fa.Engine(mt, nf, F, k, seed=seed, init_mean=mean, init_stddev=stddev, max_batch_rows=64,
                     max_batch_nnz=64 * 8, **kw)


def assert_ids(got, want, what):
    assert got.dtype == np.int32, what
    assert np.array_equal(got, np.asarray(want, np.int32)), (what, got[:16], np.asarray(want)[:16])


@gpu
@pytest.mark.parametrize("skip_init", [False, True], ids=["init", "skip_init"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fresh_engine_reports_nothing(shape, skip_init):
    for seed, mean, stddev in INITS:
        e = engine(shape, seed, mean, stddev, skip_init=skip_init)
        what = "%s seed=%d mean=%g" % (shape_id(shape), seed, mean)
        assert_ids(e.changed_features(), [], what)
        # ... and the state it was compared with is the one the helper restates
        assert_state_bitwise(e.get_state(), fresh_state(shape[0], shape[3], e.row_len, seed, mean, stddev, skip_init), what)
        e.close()


@gpu
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=shape_id)
def test_weights_set_to_the_host_draw_are_unchanged(shape):
    seed, mean, stddev = 11, -0.125, 0.03
    e = engine(shape, seed, mean, stddev)
    fr = fresh_state(shape[0], shape[3], e.row_len, seed, mean, stddev)
    zero = {k: np.zeros_like(fr[k]) for k in ("bias3", "lin_w", "vec_w")}
    e.set_state(zero)  # (set_weights: every w is now 0, not its draw)
    assert_ids(e.changed_features(), np.arange(shape[3]), "zeroed weights")
    e.set_state({k: fr[k] for k in ("bias3", "lin_w", "vec_w")})
    assert_ids(e.changed_features(), [], "weights set to init_weights_host's output")
    e.close()
    # the other way round: a skip_init engine given the draws differs everywhere from ITS create-time zeros
    e = engine(shape, seed, mean, stddev, skip_init=True)
    e.set_state({k: fr[k] for k in ("bias3", "lin_w", "vec_w")})
    assert_ids(e.changed_features(), np.arange(shape[3]), "skip_init engine given the draws")
    e.close()


def poke_values(key, init):
    """The patterns poked into one word: 1.0, NaN, and -0.0 for (n, z) / the draw's neighbour for w."""
    f = np.float32
    if key.endswith("_w"):
        return [("1.0", f(1.0)), ("nan", f(np.nan)), ("nextafter(init)", np.nextafter(f(init), f(np.inf)))]
    return [("1.0", f(1.0)), ("-0.0", f(-0.0)), ("nan", f(np.nan))]


@gpu
@pytest.mark.parametrize("skip_init", [False, True], ids=["init", "skip_init"])
@pytest.mark.parametrize("shape", [("FFM", 5, 4, 97), ("FFM", 5, 3, 97), ("FM", 1, 65, 97), ("LR", 1, 1, 97)], ids=shape_id)
def test_single_element_pokes(shape, skip_init):
    nf = shape[3]
    e = engine(shape, skip_init=skip_init)
    L = e.row_len
    for key in fa.Engine.ROW_KEYS:
        if key.startswith("vec") and L == 0:
            continue
        for feat in (0, 31, 32, 63, 64, nf - 1):
            ids = np.array([feat], np.int32)
            orig = e.get_rows(ids)[key]
            for elem in ((0, L - 1) if key.startswith("vec") else (None,)):
                at = (0, elem) if elem is not None else (0,)
                for name, v in poke_values(key, orig[at]):
                    what = "%s[%d][%s] = %s" % (key, feat, elem, name)
                    poked = orig.copy()
                    poked[at] = v
                    assert bits(poked)[at] != bits(orig)[at], what
                    e.set_rows(ids, {key: poked})
                    assert_ids(e.changed_features(), [feat], what)
                    e.set_rows(ids, {key: orig})
                    assert_ids(e.changed_features(), [], what + " poked back")
    if skip_init:  # create-time w is +0 here: -0.0 is another pattern
        e.set_rows(np.array([40], np.int32), {"lin_w": np.array([-0.0], np.float32)})
        assert_ids(e.changed_features(), [40], "lin_w = -0.0 on a skip_init engine")
        e.set_rows(np.array([40], np.int32), {"lin_w": np.array([0.0], np.float32)})
    # two pokes in different bitmap words, given in descending order, come back ascending
    key = "lin_z" if L == 0 else "vec_z"
    two = np.array([70, 3], np.int32)
    rows = e.get_rows(two)[key]
    if L:
        rows[:, -1] = np.float32(-0.0)  # the last element of both records
    else:
        rows[:] = np.float32(-0.0)
    e.set_rows(two, {key: rows})
    assert_ids(e.changed_features(), [3, 70], "two words")
    e.close()


F_TRAIN, NF_TRAIN = 8, 5000
TRAIN_SHAPES = [("FFM", 4, False, DEFAULT_HP), ("FFM", 4, True, STRESS_HP), ("FM", 16, False, DEFAULT_HP),
                ("LR", 1, False, DEFAULT_HP)]


@pytest.fixture(scope="module")
def zipf_blocks():
    gen = synth.Generator(F_TRAIN, NF_TRAIN, seed=5)
    return [gen.block(512) for _ in range(3)]


def oracle_run(mt, k, learn, hp, blocks, seed=42):
    """The oracle started from the engine's create-time state and trained on the blocks."""
    F = F_TRAIN if mt == "FFM" else 1
    o = CpuModel("oracle", mt, NF_TRAIN, F, k, learn=learn, **hp)
    fr = fresh_state(mt, NF_TRAIN, o.row_len, seed, 0.0, 0.02)
    o.set_state(fr)
    for b in blocks:
        o.train_batch(b)
    return o, fr


def occurring_ids(blocks):
    feat = np.concatenate([b.feat for b in blocks])
    return np.unique(feat[(feat >= 0) & (feat < NF_TRAIN)]).astype(np.int32)


@pytest.mark.parametrize("mt,k,learn,hp", TRAIN_SHAPES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_oracle_changes_exactly_the_features_that_occur(zipf_blocks, mt, k, learn, hp):
    """On the CPU: under the reference arithmetic every in-range id of the blocks ends with another
    pattern somewhere in its state (lin_n grows by g * g > 0) and no other id is touched -- what the GPU
    test below relies on.  (It holds for the learning variant on these blocks as well.)"""
    fa.build()
    blocks = zipf_blocks if mt == "FFM" else [without_fields(b) for b in zipf_blocks]
    o, fr = oracle_run(mt, k, learn, hp, blocks)
    want = expected_changed(o.get_state(), fr)
    assert 0 < want.size < NF_TRAIN
    assert np.array_equal(want, occurring_ids(blocks))


@gpu
@pytest.mark.parametrize("pipelined", [False, True], ids=["sync", "async_no_flush"])
@pytest.mark.parametrize("mt,k,learn,hp", TRAIN_SHAPES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_after_training_the_scan_is_the_oracle_predicate(zipf_blocks, mt, k, learn, hp, pipelined):
    blocks = zipf_blocks if mt == "FFM" else [without_fields(b) for b in zipf_blocks]
    o, fr = oracle_run(mt, k, learn, hp, blocks)
    so = o.get_state()
    want = expected_changed(so, fr)
    F = F_TRAIN if mt == "FFM" else 1
    per = NF_TRAIN // F_TRAIN
    fs = (np.arange(F + 1) * per).astype(np.int32) if mt == "FFM" else None
    e = fa.Engine(mt, NF_TRAIN, F, k, max_batch_rows=512, max_batch_nnz=512 * F_TRAIN, field_start=fs, learn=learn, **hp)
    for b in blocks:
        if pipelined:
            e.train_batch_async(b)  # (the last block is staged, not trained, when this returns)
        else:
            e.train_batch(b)
    got = e.changed_features()  # no flush in between
    assert_ids(got, want, "scan vs oracle predicate")
    if not learn:
        assert_ids(got, occurring_ids(blocks), "scan vs the ids that occur")
    if pipelined:
        e.train_flush()
    assert_state_bitwise(e.get_state(), so, "state after the scan")
    e.close()


@gpu
def test_capacity_and_sharded_errors():
    e = engine(("FFM", 5, 4, 97))
    lib = e.lib
    ids = np.array([3, 64, 96], np.int32)
    rows = e.get_rows(ids)["lin_n"]
    rows[:] = 1.0
    e.set_rows(ids, {"lin_n": rows})
    n = ctypes.c_int64(-1)
    buf = np.full(3, -1, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    assert lib.ffm_engine_changed_features(e.h, buf.ctypes.data_as(i32p), 2, ctypes.byref(n)) == -4  # FFM_E_CAPACITY
    assert n.value == 3 and (buf == -1).all()
    n.value = -1
    assert lib.ffm_engine_changed_features(e.h, None, 0, ctypes.byref(n)) == 0 and n.value == 3  # only counts
    assert lib.ffm_engine_changed_features(e.h, buf.ctypes.data_as(i32p), 3, ctypes.byref(n)) == 0
    assert buf.tolist() == [3, 64, 96]
    e.close()
    s = fa.Engine("FFM", 97, 4, 4, n_shards=2, shard_rank=0, max_batch_rows=64, max_batch_nnz=512)
    n.value = -1
    assert lib.ffm_engine_changed_features(s.h, None, 0, ctypes.byref(n)) == -5  # FFM_E_UNSUPPORTED
    assert n.value == 0
    with pytest.raises(fa.EngineError) as err:
        s.changed_features()
    assert err.value.code == -5
    s.close()


def test_null_engine_is_invalid():
    """No device needed: the argument check comes first, and *n_changed is still set."""
    fa.build()
    lib = fa.load_library()
    n = ctypes.c_int64(-1)
    assert lib.ffm_engine_changed_features(None, None, 0, ctypes.byref(n)) == -1  # FFM_E_INVALID
    assert n.value == 0
    assert b"null engine" in lib.ffm_engine_last_error()


@gpu
def test_offsets_past_2_to_31():
    """FFM 39 x 16 with 3 441 481 features: the smallest count whose latent element index (and whose
    draw index) passes 2^31; the record of the last feature starts 25.8 GB into the tensor."""
    F, k, nf = 39, 16, 3441481
    assert (nf - 1) * F * k < 2 ** 31 <= nf * F * k
    e = fa.Engine("FFM", nf, F, k, max_batch_rows=64, max_batch_nnz=64 * F)
    last = np.array([nf - 1], np.int32)
    orig = e.get_rows(last)
    poked = orig["vec_z"].copy()
    poked[0, F * k - 1] = -0.0
    e.set_rows(last, {"vec_z": poked})
    assert_ids(e.changed_features(), [nf - 1], "vec_z of the last record")
    e.set_rows(last, {"vec_z": orig["vec_z"]})
    # back to the create-time state: every w of every record is compared with its draw again, the last
    # record's (draw indices past 2^31) included
    assert_ids(e.changed_features(), [], "restored")
    e.close()


@gpu
def test_a_block_the_device_refused_is_an_error_of_the_scan():
    """A row longer than max_row_nnz reaching train_batch_device is skipped as a whole by the device; the
    scan that follows returns (and clears) that error as ffm_engine_sync would, instead of listing a model
    that silently lacks the block.  The next scan is clean: the model is still the fresh one."""
    from oracle.pyoracle import Csr
    F, k, per = 4, 4, 30
    e = fa.Engine("FFM", F * per, F, k, max_batch_rows=64, max_batch_nnz=4096, max_row_nnz=8, seed=2)
    rows = [[(f, f * per + (r + f) % per, 1.0) for f in range(F)] for r in range(10)]
    rows[6] = [(f % F, (f % F) * per + f % per, 1.0) for f in range(9)]  # 9 entries > 8
    bad = Csr.from_rows(rows, [r % 2 for r in range(10)])
    d = {k_: torch.from_numpy(getattr(bad, k_)).cuda() for k_ in ("row_ptr", "field", "feat", "val", "label")}
    out = torch.zeros(10, device="cuda")
    e.train_batch_device(10, int(bad.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr(),
                         d["feat"].data_ptr(), d["val"].data_ptr(), d["label"].data_ptr(), out.data_ptr())
    with pytest.raises(fa.EngineError) as err:
        e.changed_features()
    assert err.value.code == -4  # FFM_E_CAPACITY
    e.sync()  # the report cleared the flag
    assert_ids(e.changed_features(), [], "the refused block left the model alone")
    e.close()
