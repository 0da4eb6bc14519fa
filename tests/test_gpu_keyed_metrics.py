"""Keyed capture and the grouped AUC on the device (include/ffm_engine.h "Metrics", keyed capture): the capture
kernel, the radix sort and the rank pass of csrc/kernels_keyed.h against fa.keyed_auc_reference -- per-key tables
as integers, gauc bit for bit.  Expected values come from the p the same engine returns (predict_batch(...,
output_prob=True); for the train channel the returned pre-update logits through ffm_engine_eval_sigmoid) and from
the keys read off the block on the host.

One shape throughout: FFM, 4 fields, 4096 features, k = 4, blocks of at most 8192 rows, rows of one entry per
field in field order.  Field f owns ids [1024 f, 1024 (f + 1)); field 0's id is the row's key.  The latent weights
are zero and lin_w is non-zero only on field 1's ids, where it takes five values: every score is one of five, so
ties inside keys are the rule.  The rank pass scans in tiles of TILE = 2048 words (kKeyedTile)."""
import ctypes
import math
import re
import struct

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

pytestmark = pytest.mark.gpu

NF, F, K, PER = 4096, 4, 4, 1024
MAX_ROWS = 8192
TILE = 2048
LEVELS = np.array([-1.5, -0.25, 0.0, 0.5, 2.0], np.float32)
COUNTS = ("n_rows", "n_keys", "n_keys_mixed", "n_rows_mixed", "n_nan", "n_unkeyed", "n_overflow")
E_INVALID, E_CAPACITY, E_UNSUPPORTED = fa.engine.E_INVALID, fa.engine.E_CAPACITY, fa.engine.E_UNSUPPORTED


def bits(x):
    return struct.pack("<d", x)


def level_lin(levels=LEVELS):
    lin = np.zeros(NF, np.float32)
    lin[PER:2 * PER] = np.asarray(levels, np.float32)[np.arange(PER) % len(levels)]
    return lin


def make_engine(lin=None, **kw):
    e = fa.Engine("FFM", NF, F, K, skip_init=True, max_batch_rows=MAX_ROWS, max_batch_nnz=MAX_ROWS * 8, **kw)
    if not kw.get("serve"):
        e.set_state(e.zero_state())
    e.set_weights(bias=np.zeros(1, np.float32), lin_w=level_lin() if lin is None else lin,
                  vec_w=np.zeros((NF, F * K), np.float32))
    return e


def make_block(keys, seed, pos_rate=0.4):
    """One row per key: [field 0: the key, field 1 .. 3: a random id of the field], values 1."""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.int64)
    n = keys.size
    feat = np.empty((n, F), np.int32)
    feat[:, 0] = keys
    for f in range(1, F):
        feat[:, f] = f * PER + rng.integers(0, PER, n)
    field = np.broadcast_to(np.arange(F, dtype=np.int32), (n, F)).copy()
    return Block((np.arange(n + 1) * F).astype(np.int32), field.reshape(-1), feat.reshape(-1), np.ones(n * F, np.float32),
                 (rng.random(n) < pos_rate).astype(np.int32))


def from_rows(rows, labels):
    """rows: lists of (field, feat) -- any shape of row."""
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    flat = [x for r in rows for x in r]
    return Block(ptr, np.array([x[0] for x in flat], np.int32), np.array([x[1] for x in flat], np.int32),
                 np.ones(len(flat), np.float32), np.asarray(labels, np.int32))


def keys_of(b, key_field=0, n_feats=NF, feat=None):
    """The row's key as the header defines it, -1 for none."""
    feat = b.feat if feat is None else feat
    out = np.full(b.n_rows, -1, np.int64)
    for r in range(b.n_rows):
        for j in range(int(b.row_ptr[r]), int(b.row_ptr[r + 1])):
            if b.field[j] == key_field and 0 <= feat[j] < n_feats:
                out[r] = feat[j]
                break
    return out


def cat(blocks):
    return np.concatenate([keys_of(b) for b in blocks]), np.concatenate([b.label for b in blocks])


def probs(e, blocks):
    return np.concatenate([e.predict_batch(b, output_prob=True)[0] for b in blocks]) if blocks else np.zeros(0, np.float32)


def assert_keyed(e, channel, ref, what, overflow=0):
    t = e.metrics_keyed_table(channel)
    for k in ("key", "pos", "neg", "u2"):
        got, want = t[k], ref[k]
        assert got.shape == want.shape, "%s: %d keys, expected %d" % (what, got.size, want.size)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %s differs at %d keys, first key %d: %d, expected %d" % (
            what, k, bad.size, ref["key"][bad[0]], got[bad[0]], want[bad[0]])
    m = e.metrics_read_keyed(channel)
    print("%s: %s" % (what, m))
    for k in COUNTS:
        assert m[k] == (overflow if k == "n_overflow" else ref[k]), (what, k, m, {c: ref[c] for c in COUNTS})
    assert bits(m["gauc"]) == bits(ref["gauc"]) or (math.isnan(m["gauc"]) and math.isnan(ref["gauc"])), (what, m["gauc"], ref["gauc"])
    return m


def run_eval(e, blocks, what, capacity=1 << 16):
    """p first (capture off), then capture on from empty, the blocks once more, and the comparison."""
    e.metrics_key_field(0, capacity, eval=False, train=False)
    p = probs(e, blocks)
    keys, label = cat(blocks)
    ref = fa.keyed_auc_reference(keys, p, label)
    e.metrics_key_field(0, capacity, eval=True)
    for b in blocks:
        e.predict_batch(b)
    return assert_keyed(e, "eval", ref, what), ref, p


@pytest.fixture(scope="module")
def engine():
    e = make_engine()
    yield e
    e.close()


# ---- 1. the edges of the rank pass --------------------------------------------------------------

def edge_keys(case):
    rng = np.random.default_rng(7)
    if case == "every_row_its_own_key":
        return rng.permutation(PER)
    if case == "one_key":
        return np.full(3000, 7)
    if case == "keys_of_1_2_63_64_65_rows":
        return rng.permutation(np.repeat([900, 3, 511, 512, 77], [1, 2, 63, 64, 65]))
    if case == "long_key":  # 3 tiles and a bit of one key: its five tie runs are ~1250 words each and cross every tile boundary
        return rng.permutation(np.concatenate([np.full(3 * TILE + 100, 300), rng.integers(0, 40, 1500)]))
    assert case == "mixed_sizes"
    return rng.integers(0, 200, 5000)


@pytest.mark.parametrize("case", ["every_row_its_own_key", "one_key", "keys_of_1_2_63_64_65_rows", "long_key", "mixed_sizes"])
def test_rank_pass_edges(engine, case):
    keys = edge_keys(case)
    assert keys.size <= MAX_ROWS
    m, ref, p = run_eval(engine, [make_block(keys, 11)], case)
    assert np.unique(p).size <= LEVELS.size and m["n_rows"] == keys.size
    if case == "every_row_its_own_key":
        assert m["n_keys"] == keys.size and m["n_keys_mixed"] == 0 and math.isnan(m["gauc"])
    if case == "one_key":
        assert m["n_keys"] == 1 and m["n_rows_mixed"] == keys.size and 0.0 < m["gauc"] < 1.0
    if case == "keys_of_1_2_63_64_65_rows":
        assert sorted((ref["pos"] + ref["neg"]).tolist()) == [1, 2, 63, 64, 65]
    if case == "long_key":
        g = int(np.flatnonzero(ref["key"] == 300)[0])
        assert ref["pos"][g] + ref["neg"][g] >= 3 * TILE and ref["pos"][g] > 0 and ref["neg"][g] > 0


def test_a_key_that_is_all_positive(engine):
    rng = np.random.default_rng(9)
    b = make_block(rng.integers(0, 30, 4000), 12)
    b.label[b.feat[0::F] == 5] = 1
    b.label[b.feat[0::F] == 6] = 0
    m, ref, _ = run_eval(engine, [b], "all positive")
    g5, g6 = int(np.flatnonzero(ref["key"] == 5)[0]), int(np.flatnonzero(ref["key"] == 6)[0])
    assert ref["neg"][g5] == 0 and ref["u2"][g5] == 0 and ref["pos"][g6] == 0 and m["n_keys_mixed"] == m["n_keys"] - 2


def test_a_fresh_model_scores_every_mixed_key_one_half():
    e = make_engine(lin=np.zeros(NF, np.float32))
    m, ref, p = run_eval(e, [make_block(np.random.default_rng(3).integers(0, 300, 6000), 13)], "fresh model")
    assert (p == np.float32(0.5)).all() and m["n_keys_mixed"] > 100
    assert (ref["u2"] == (ref["pos"] * ref["neg"]).astype(np.uint64)).all() and m["gauc"] == 0.5
    e.close()


def test_saturated_scores():
    """lin_w of +-88 and +-100: p = 1.0 exactly at both positive ones, p = 0.0 exactly at -100 (at -88 expf(88) is
    still finite and the sigmoid's fp32 quotient a tiny non-zero number: whatever it is, it is ranked by its bits)."""
    e = make_engine(lin=level_lin([88.0, -88.0, 100.0, -100.0, 0.25]))
    m, ref, p = run_eval(e, [make_block(np.random.default_rng(4).integers(0, 50, 5000), 14, pos_rate=0.5)], "saturated")
    print("p values:", np.unique(p))
    assert (p == np.float32(1.0)).any() and (p == np.float32(0.0)).any() and m["n_nan"] == 0 and m["n_keys_mixed"] == 50
    e.close()


# ---- 2. rows that are left out ------------------------------------------------------------------

def test_nan_unkeyed_and_erased_entries():
    lin = level_lin()
    lin[PER + 3] = np.nan
    lin[PER + 8] = np.nan
    e = make_engine(lin=lin)
    rng = np.random.default_rng(5)
    rows, labels = [], []
    for r in range(3000):
        key, sid = int(rng.integers(0, 60)), PER + int(rng.integers(0, 40))
        kind = r % 6
        if kind == 0:    # no entry of the key field at all
            row = [(1, sid), (2, 2 * PER + 1)]
        elif kind == 1:  # the key field's only entry is erased (id outside the model): no key
            row = [(0, NF + 5 + key), (1, sid)]
        elif kind == 2:  # an erased entry of the key field, then a valid one: that one is the key
            row = [(0, -3), (1, sid), (0, key), (0, (key + 1) % 60)]
        elif kind == 3:  # the key field last
            row = [(1, sid), (3, 3 * PER + 9), (0, key)]
        else:
            row = [(0, key), (1, sid)]
        rows.append(row)
        labels.append(int(rng.random() < 0.45))
    blocks = [from_rows(rows[:1700], labels[:1700]), from_rows(rows[1700:], labels[1700:])]
    m, ref, p = run_eval(e, blocks, "rows left out")
    assert m["n_unkeyed"] > 0 and m["n_nan"] > 0 and m["n_nan"] == int(np.isnan(p).sum())
    keys, _ = cat(blocks)
    assert m["n_unkeyed"] == int(((keys < 0) & ~np.isnan(p)).sum()) and m["n_rows"] + m["n_nan"] + m["n_unkeyed"] == 3000
    e.close()


def test_capacity_and_empty_block(engine):
    e = engine
    blocks = [make_block(np.random.default_rng(6).integers(0, 100, n), 15 + i) for i, n in enumerate((700, 2000, 300))]
    e.metrics_key_field(0, 1, eval=False, train=False)
    p = probs(e, blocks)
    keys, label = cat(blocks)
    full = fa.keyed_auc_reference(keys, p, label)
    e.metrics_key_field(0, 1000, eval=True)
    for b in blocks:
        e.predict_batch(b)
    m = e.metrics_read_keyed("eval")
    t = e.metrics_keyed_table("eval")
    assert (m["n_rows"], m["n_overflow"], m["n_nan"], m["n_unkeyed"]) == (1000, 2000, 0, 0), m
    # the table is that of the 1000 stored rows, whatever they are: a part of the full table, reduced as always
    assert int(t["pos"].sum() + t["neg"].sum()) == 1000 and np.isin(t["key"], full["key"]).all()
    at = np.searchsorted(full["key"], t["key"])
    assert (t["pos"] <= full["pos"][at]).all() and (t["neg"] <= full["neg"][at]).all()
    again = fa.metrics_from_keyed(t["pos"], t["neg"], t["u2"])
    assert bits(again["gauc"]) == bits(m["gauc"]) and again["n_keys"] == m["n_keys"] == t["key"].size
    # an empty block adds nothing; neither does an unlabelled one
    empty = fa.keyed_auc_reference([], np.zeros(0, np.float32), [])
    e.metrics_key_field(0, 1000, eval=False, train=False)
    e.metrics_key_field(0, 1000, eval=True)
    e.predict_batch(make_block([], 1))
    e.predict_batch(blocks[0], with_loss=False)
    m = assert_keyed(e, "eval", empty, "an empty block")
    assert m["n_rows"] == 0 and math.isnan(m["gauc"])
    # exactly full is not overflow
    e.metrics_key_field(0, 700, eval=True)
    e.predict_batch(blocks[0])
    assert_keyed(e, "eval", fa.keyed_auc_reference(keys[:700], p[:700], label[:700]), "exactly full")


# ---- 3. order independence ----------------------------------------------------------------------

def test_order_and_block_split_do_not_matter(engine):
    e = engine
    base = make_block(np.random.default_rng(8).integers(0, 500, 6000), 21)
    seen = []
    for shuffle in range(3):
        perm = np.random.default_rng(100 + shuffle).permutation(6000)
        feat = base.feat.reshape(6000, F)[perm].reshape(-1).copy()
        whole = Block(base.row_ptr, base.field, feat, base.val, base.label[perm].copy())
        for cuts in ((0, 6000), (0, 1000, 3500, 6000)):
            blocks = [whole.rows(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
            m, ref, _ = run_eval(e, blocks, "shuffle %d, %d blocks" % (shuffle, len(blocks)))
            seen.append((ref["key"].tobytes(), ref["pos"].tobytes(), ref["neg"].tobytes(), ref["u2"].tobytes(), bits(m["gauc"])))
    assert len(set(seen)) == 1 and not math.isnan(struct.unpack("<d", seen[0][4])[0])


# ---- 4. entry points ----------------------------------------------------------------------------

def restart(e, eval=False, train=False, capacity=1 << 16):
    e.metrics_key_field(0, capacity, eval=False, train=False)
    e.metrics_key_field(0, capacity, eval=eval, train=train)


def test_every_labelled_predict_entry_point_feeds_the_eval_capture(engine):
    from test_gpu_metrics import DeviceBlock, pinned, without_field_array
    e = engine
    blocks = [make_block(np.random.default_rng(30 + i).integers(0, 80, n), 40 + i) for i, n in enumerate((300, 257, 64, 1))]
    restart(e)
    p = probs(e, blocks)
    keys, label = cat(blocks)
    once = fa.keyed_auc_reference(keys, p, label)
    twice = fa.keyed_auc_reference(np.tile(keys, 2), np.tile(p, 2), np.tile(label, 2))
    for output_prob in (False, True):
        restart(e, eval=True, train=True)
        for b in blocks:
            e.predict_batch(b, output_prob=output_prob)
        assert_keyed(e, "eval", once, "predict_batch output_prob=%d" % output_prob)
    e.predict_batch(blocks[0], with_loss=False)
    assert_keyed(e, "eval", once, "an unlabelled predict_batch adds nothing")
    for zero_copy in (False, True):
        for bare in (False, True):
            cs = [without_field_array(b) if bare else b for b in blocks]
            if zero_copy:
                cs = [pinned(c) for c in cs]
            restart(e, eval=True, train=True)
            for c in cs:
                e.predict_batch_async(c, zero_copy=zero_copy)
            e.train_flush()
            assert_keyed(e, "eval", once, "predict_batch_async zero_copy=%d bare=%d" % (zero_copy, bare))
    # reading launches the deferred block itself: no flush in between
    restart(e, eval=True)
    for b in blocks:
        e.predict_batch_async(b)
    assert_keyed(e, "eval", once, "read without a flush")
    e.train_flush()
    # the scores going out as well
    restart(e, eval=True)
    bufs = [e.score_buffer(b.n_rows) for b in blocks]
    for b, buf in zip(blocks, bufs):
        e.predict_batch_async(b, scores=buf, output_prob=True)
    e.train_flush()
    assert np.array_equal(np.concatenate(bufs).view(np.uint32), p.view(np.uint32))
    assert_keyed(e, "eval", once, "predict_batch_async with scores")
    for buf in bufs:
        e.free_score_buffer(buf)
    for output_prob in (0, 1):
        restart(e, eval=True, train=True)
        for b in blocks:
            d = DeviceBlock(b)
            d_out = torch.zeros(b.n_rows, dtype=torch.float32, device="cuda")
            e.predict_batch_device(*d.args(), output_prob, d_out.data_ptr(), None)
            e.predict_batch_device(*d.args(), output_prob, None, None)  # out == NULL: the engine's own output array
            e.sync()
        assert_keyed(e, "eval", twice, "predict_batch_device output_prob=%d" % output_prob)
    # predict_finish_device has no rows: it adds nothing
    d_logit = torch.zeros(300, dtype=torch.float32, device="cuda")
    d_label = torch.from_numpy(blocks[0].label).cuda()
    torch.cuda.synchronize()
    e.predict_finish_device(300, d_logit.data_ptr(), d_label.data_ptr(), 0, None)
    e.sync()
    assert_keyed(e, "eval", twice, "predict_finish_device adds nothing")
    assert_keyed(e, "train", fa.keyed_auc_reference([], np.zeros(0, np.float32), []), "predicting leaves the train capture alone")
    restart(e)


def train_state(e):
    """lin_w of five values through (n, z), as training reads them; latent weights stay zero."""
    st = e.zero_state()
    st["lin_n"][:] = 1.0
    st["lin_z"][PER:2 * PER] = np.array([-40.0, -8.0, 3.0, 12.0, 60.0], np.float32)[np.arange(PER) % 5]
    return st


@pytest.mark.parametrize("path", ["train_batch", "train_batch_async", "train_batch_async_pinned", "stage_batch+train_staged",
                                  "train_batch_device", "train_forward_device+train_update_device"])
def test_every_training_path_feeds_the_train_capture(path):
    from test_gpu_metrics import MAX_ROWS as BUF_ROWS, _run_train
    e, twin = make_engine(), make_engine()
    for x in (e, twin):
        x.set_state(train_state(x))
    blocks = [make_block(np.random.default_rng(50 + i).integers(0, 40, n), 60 + i) for i, n in enumerate((256, 300, 65, 129))]
    assert max(b.n_rows for b in blocks) <= BUF_ROWS
    logits = np.concatenate([twin.train_batch(b)[0] for b in blocks])  # the pre-update logits, block after block
    keys, label = cat(blocks)
    ref = fa.keyed_auc_reference(keys, e.eval_sigmoid(logits), label)
    e.metrics_key_field(0, 4096, eval=True, train=True)
    keep = _run_train(e, path, blocks)
    m = assert_keyed(e, "train", ref, path)
    assert m["n_rows"] == 750 and m["n_keys_mixed"] > 0
    assert_keyed(e, "eval", fa.keyed_auc_reference([], np.zeros(0, np.float32), []), "training leaves the eval capture alone")
    a, b = e.get_state(), twin.get_state()
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a), "capture changes no state"
    del keep
    e.close()
    twin.close()


def test_a_serving_engine_and_hashed_ids():
    s = make_engine(serve="f16")
    blocks = [make_block(np.random.default_rng(70 + i).integers(0, 90, n), 80 + i) for i, n in enumerate((2000, 500))]
    m, _, _ = run_eval(s, blocks, "serving engine, f16")
    assert m["n_keys_mixed"] > 0
    s.close()
    # hashed ids: the key is the id the kernels see, the hashed one; raw ids far outside the model
    lin = LEVELS[np.arange(NF) % 5].astype(np.float32)
    h = make_engine(lin=lin, hash_ids=True)
    rng = np.random.default_rng(71)
    raw = make_block(rng.integers(0, 400, 3000) * 7919 + 1000003, 81)
    raw.feat[1::F] += 5000000
    hashed = fa.hash_ids(raw.field, raw.feat, NF, n_fields=F)
    h.metrics_key_field(0, 4096, eval=False, train=False)
    p = probs(h, [raw])
    keys = keys_of(raw, feat=hashed)
    assert (keys >= 0).all() and np.unique(keys).size > 100
    ref = fa.keyed_auc_reference(keys, p, raw.label)
    h.metrics_key_field(0, 4096, eval=True)
    h.predict_batch(raw)
    assert_keyed(h, "eval", ref, "hashed ids")
    h.close()


# ---- 5. bookkeeping -----------------------------------------------------------------------------

def launches(e, name):
    m = re.search(r"%s\s+launches=\s*(\d+)" % re.escape(name), e.profile_dump())
    return int(m.group(1)) if m else 0


def test_bookkeeping():
    e, plain = make_engine(), make_engine()
    for x in (e, plain):
        x.set_state(train_state(x))
    blocks = [make_block(np.random.default_rng(90 + i).integers(0, 50, n), 95 + i) for i, n in enumerate((200, 100, 65))]
    keys, label = cat(blocks)
    # off by default: reading is FFM_E_INVALID and the launches are those of an engine that never heard of capture
    # (its buffers are made by ffm_engine_metrics_key_field alone: the free HBM of a shared device says nothing here)
    for ch in ("eval", "train"):
        with pytest.raises(fa.EngineError) as err:
            e.metrics_read_keyed(ch)
        assert err.value.code == E_INVALID
        with pytest.raises(fa.EngineError):
            e.metrics_keyed_table(ch)
    for x in (e, plain):
        x.profile_enable(True)
        for b in blocks:
            x.predict_batch(b)
        x.train_batch(blocks[0])
    assert "keyed_" not in e.profile_dump()
    count = lambda x: sorted(re.findall(r"^(\S+)\s+launches=\s*(\d+)", x.profile_dump(), re.M))  # noqa: E731
    assert count(e) == count(plain)
    ref = fa.keyed_auc_reference(keys, probs(e, blocks), label)  # (of the weights as that training block left them)
    # on: exactly one launch per labelled block and channel
    cap = 1 << 20
    e.metrics_key_field(0, cap, eval=True)
    e.profile_enable(True)
    for b in blocks:
        e.predict_batch(b)
    e.predict_batch(blocks[0], with_loss=False)
    e.train_batch(blocks[1])
    assert launches(e, "keyed_capture_kernel") == len(blocks)
    assert_keyed(e, "eval", ref, "three blocks")
    with pytest.raises(fa.EngineError):  # the channels are independent: train is still off
        e.metrics_read_keyed("train")
    # a read is the sort and the rank pass, named in the dump
    dump = e.profile_dump()
    for name in ("keyed_sort_hist_kernel", "keyed_sort_scan_kernels", "keyed_sort_scatter_kernel", "keyed_rank_kernels"):
        assert name in dump, dump
    # a second enable keeps a channel that is on, starts the other from empty
    e.metrics_key_field(0, cap, eval=True, train=True)
    assert_keyed(e, "eval", ref, "after a second enable")
    assert e.metrics_read_keyed("train")["n_rows"] == 0
    e.profile_enable(True)
    e.train_batch(blocks[2])
    e.predict_batch(blocks[0])
    assert launches(e, "keyed_capture_kernel") == 2
    assert e.metrics_read_keyed("train")["n_rows"] == blocks[2].n_rows
    # reset returns the numbers and empties
    e.metrics_key_field(0, cap, eval=False, train=False)
    ref = fa.keyed_auc_reference(keys, probs(e, blocks), label)  # (two more blocks have trained)
    e.metrics_key_field(0, cap, eval=True)
    for b in blocks:
        e.predict_batch(b)
    m = e.metrics_read_keyed("eval", reset=True)
    assert m["n_rows"] == sum(b.n_rows for b in blocks) and bits(m["gauc"]) == bits(ref["gauc"])
    assert e.metrics_read_keyed("eval")["n_rows"] == 0 and e.metrics_keyed_table("eval")["key"].size == 0
    e.predict_batch(blocks[1])
    assert e.metrics_read_keyed("eval")["n_rows"] == blocks[1].n_rows
    # off stops the launches and cannot be read; on again starts empty; another key field starts empty too
    e.metrics_key_field(0, cap, eval=False, train=False)
    e.profile_enable(True)
    e.predict_batch(blocks[0])
    assert launches(e, "keyed_capture_kernel") == 0
    with pytest.raises(fa.EngineError):
        e.metrics_read_keyed("eval")
    e.metrics_key_field(0, cap, eval=True)
    assert e.metrics_read_keyed("eval")["n_rows"] == 0
    e.predict_batch(blocks[0])
    e.metrics_key_field(2, cap, eval=True)
    assert e.metrics_read_keyed("eval")["n_rows"] == 0
    e.predict_batch(blocks[0])
    t = e.metrics_keyed_table("eval")
    assert t["key"].min() >= 2 * PER and t["key"].max() < 3 * PER and int(t["pos"].sum() + t["neg"].sum()) == blocks[0].n_rows
    e.profile_enable(False)
    e.close()
    plain.close()
    # the histogram channels' numbers do not change by capture being on
    e, plain = make_engine(), make_engine()
    e.metrics_key_field(0, cap, eval=True, train=True)
    for x in (e, plain):
        x.set_state(train_state(x))
        x.metrics_enable(eval=True, train=True)
        for b in blocks:
            x.predict_batch(b)
        x.train_batch(blocks[2])
    for ch in ("eval", "train"):
        assert e.metrics(ch) == plain.metrics(ch) or (math.isnan(e.metrics(ch)["auc"]) and math.isnan(plain.metrics(ch)["auc"]))
        he, hp = e.metrics_histogram(ch), plain.metrics_histogram(ch)
        assert np.array_equal(he[0], hp[0]) and np.array_equal(he[1], hp[1]) and int(he[0].sum() + he[1].sum()) > 0
    e.close()
    plain.close()


# ---- 6. refusals --------------------------------------------------------------------------------

def code_of(fn):
    with pytest.raises(fa.EngineError) as err:
        fn()
    return err.value.code


def test_refusals_leave_the_engine_usable(engine):
    e = engine
    b = make_block(np.random.default_rng(2).integers(0, 20, 500), 3)
    restart(e)
    before = e.predict_batch(b, output_prob=True)[0]
    assert code_of(lambda: e.metrics_key_field(-1, 100)) == E_INVALID
    assert code_of(lambda: e.metrics_key_field(F, 100)) == E_INVALID
    assert code_of(lambda: e.metrics_key_field(0, 0)) == E_INVALID
    assert code_of(lambda: e.metrics_key_field(0, -7)) == E_INVALID
    assert code_of(lambda: e.metrics_key_field(0, (1 << 30) + 1)) == E_UNSUPPORTED
    assert code_of(lambda: e._check(e.lib.ffm_engine_metrics_key_field(e.h, 4, 0, 100))) == E_INVALID
    assert code_of(lambda: e.metrics_read_keyed("eval")) == E_INVALID
    km = fa.KeyedMetrics()
    assert code_of(lambda: e._check(e.lib.ffm_engine_metrics_read_keyed(e.h, 2, 0, ctypes.byref(km)))) == E_INVALID
    e.metrics_key_field(0, 1000, eval=True)
    e.predict_batch(b)
    assert code_of(lambda: e._check(e.lib.ffm_engine_metrics_read_keyed(e.h, 0, 0, None))) == E_INVALID
    # arrays too short: FFM_E_CAPACITY with the count set; NULL arrays with cap == 0 ask for it
    n = ctypes.c_int64(-1)
    assert e.lib.ffm_engine_metrics_keyed_table(e.h, 0, 0, None, None, None, None, ctypes.byref(n)) == E_CAPACITY and n.value == 20
    key = np.zeros(3, np.int32)
    n = ctypes.c_int64(-1)
    assert e.lib.ffm_engine_metrics_keyed_table(e.h, 0, 3, key.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, None,
                                                ctypes.byref(n)) == E_CAPACITY and n.value == 20
    assert_keyed(e, "eval", fa.keyed_auc_reference(keys_of(b), before, b.label), "after the refusals")
    restart(e)
    # engines keyed capture is not for: refused, and they go on working
    for name, kw in (("LR", dict(n_fields=1, n_factors=1)), ("FM", dict(n_fields=1, n_factors=4))):
        o = fa.Engine(name, 64, max_batch_rows=64, **kw)
        assert code_of(lambda: o.metrics_key_field(0, 100)) == E_UNSUPPORTED
        assert code_of(lambda: o.metrics_read_keyed("eval")) == E_INVALID
        o.metrics_enable(eval=True)
        o.close()
    sh = fa.Engine("FFM", NF, F, K, max_batch_rows=64, n_shards=2, shard_rank=0)
    assert code_of(lambda: sh.metrics_key_field(0, 100)) == E_UNSUPPORTED
    sh.close()
    g = fa.Group([0], "FFM", NF, F, K, max_batch_rows=512, max_batch_nnz=512 * F)
    assert code_of(lambda: g.engines[0].metrics_key_field(0, 100)) == E_UNSUPPORTED
    out, _ = g.predict_batch(b)
    assert out.shape == (500,)
    g.close()
