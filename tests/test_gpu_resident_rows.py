"""Resident rows (include/ffm_engine.h "Resident rows"; csrc/kernels_rows.h, csrc/engine_rows.h): blocks cut out of
device-parsed text in HBM and staged from there, against the same blocks in host memory, bit for bit.  The text, the
blocks and the chunking are those of the CPU test (tests/row_cut_cases.py); parser slots of 4 KB make blocks straddle
chunks; the reference blocks are parse_text_host plus numpy slicing."""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

import row_cut_cases as cases
from util import STRESS_HP, assert_bitwise, assert_state_bitwise

pytestmark = pytest.mark.gpu

SLOT = 4096
SLOT_MIXED = 2048  # (the mixed test wants at least 8 chunks of the 300 rows, about 16 KB of text)
F, NF, K = cases.N_FIELDS, cases.N_FEATS, 4
ROWS, NNZ = 64, 64 * 5  # a block's capacities: the entry budget (five entries a row; the mean row is about six) bites
RAMP = [1, 7, 64]
POISON = 0xAB
BITS = 10


def _lib():
    lib = fa.load_library()
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    lib.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    return lib


def _download(addr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        assert _lib().hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@functools.lru_cache(maxsize=None)
def _data(has_field=True, slow=False, slot=SLOT):
    """(chunks of the text, their host parses, the whole text's host parse).  slow: one row of the text spells its
    first value 1e-3 -- outside the device grammar, the float 0.001 -- and the host parses read 0.001 in its place."""
    slow_row = 150 if slow else None
    text, counts = cases.make_text(300, 5, has_field=has_field, slow_row=slow_row)
    if slow:
        assert counts[slow_row] > 0 and text.count(b"1e-3") == 1
    chunks = cases.chunks(text, slot)
    assert len(chunks) >= 3
    fix = lambda t: t.replace(b"1e-3", b"0.001")  # noqa: E731
    host = [fa.parse_text_host(fix(c), has_field=has_field) for c in chunks]
    whole = fa.parse_text_host(fix(text), has_field=has_field)
    assert whole["n_slow"] == 0 and whole["n_rows"] == 300 == sum(h["n_rows"] for h in host)
    assert np.array_equal(whole["row_ptr"][1:] - whole["row_ptr"][:-1], counts)
    return chunks, host, whole


def _host_block(whole, r0, r1):
    e0, e1 = int(whole["row_ptr"][r0]), int(whole["row_ptr"][r1])
    return synth.Block((whole["row_ptr"][r0:r1 + 1] - e0).astype(np.int32), whole["field"][e0:e1].copy(), whole["feat"][e0:e1].copy(),
                       whole["val"][e0:e1].copy(), whole["label"][r0:r1].copy())


def _ranges(whole, wants=RAMP, max_nnz=NNZ):
    return cases.reference_blocks(whole["row_ptr"], wants, max_nnz)


def _feed(has_field, slow, ranges, cutter, before_block=lambda: None, counts=None, slot=SLOT):
    """Yields the closed RowsBlock of every row range, driving parser and cutter the way host/row_stream.cpp does:
    chunk t + 1 is parsed while chunk t is consumed, a chunk's rows are taken before its slot is parsed into again, a
    chunk the device will not parse goes in through take_host."""
    chunks, host, _ = _data(has_field, slow, slot)
    starts = np.concatenate([[0], np.cumsum([h["n_rows"] for h in host])])
    tp = fa.TextParser(has_field=has_field, max_bytes=slot, max_rows=slot // 2 + 1, max_nnz=slot // 4 + 2)
    counts = {} if counts is None else counts
    counts.update(device=0, host=0, spans=[])
    waited = {}
    try:
        def start(i):
            if i < len(chunks):
                tp.parse(chunks[i], slot=i & 1)

        def get(i, cur):
            while cur[0] < i:  # chunk cur is consumed: its slot takes the chunk after the next
                if cur[0] not in waited:
                    tp.wait(cur[0] & 1)
                    waited[cur[0]] = None
                cur[0] += 1
                start(cur[0] + 1)
            if i not in waited:
                blk = tp.wait(i & 1, rows=True)
                if blk["n_slow"] or blk["overflow"]:
                    assert blk["row_ptr_host"] is None
                    waited[i] = None
                    counts["host"] += 1
                else:
                    assert blk["n_rows"] == host[i]["n_rows"] and np.array_equal(blk["row_ptr_host"], host[i]["row_ptr"]), i
                    waited[i] = blk
                    counts["device"] += 1
            return waited[i]

        cur = [0]
        start(0)
        start(1)
        for r0, r1 in ranges:
            before_block()
            r, first = r0, None
            while r < r1:
                i = int(np.searchsorted(starts, r, side="right")) - 1
                first = i if first is None else first
                lo, hi = r - int(starts[i]), min(r1, int(starts[i + 1])) - int(starts[i])
                src = get(i, cur)
                if src is None:
                    h = host[i]
                    e0 = int(h["row_ptr"][lo])
                    cutter.take_host(hi - lo, h["row_ptr"][lo:hi + 1], h["field"][e0:], h["feat"][e0:], h["val"][e0:], h["label"][lo:])
                else:
                    cutter.take(src, lo, hi)
                r += hi - lo
            counts["spans"].append(1 if first is None else i - first + 1)
            yield cutter.close()
        for i in range(cur[0], min(cur[0] + 2, len(chunks))):
            if i not in waited:
                tp.wait(i & 1)
    finally:
        _lib().hipDeviceSynchronize()
        tp.close()


class Ring:
    """A cutter's buffers in use: released once the engine has pulled the block that lived there."""

    def __init__(self, cutter, engine):
        self.cutter, self.engine, self.held, self.waits = cutter, engine, [], 0

    def before_block(self):
        if len(self.held) == self.cutter.n_blocks:
            blk = self.held.pop(0)
            if self.engine.blocks_pulled() < blk.seq:
                self.waits += 1
            while self.engine.blocks_pulled() < blk.seq:
                pass
            self.cutter.release(blk)

    def handed_over(self, blk):
        assert blk.seq > 0
        self.held.append(blk)


def test_cutter_blocks_equal_the_sliced_host_arrays_and_nothing_behind_them_is_written():
    lib = _lib()
    _, _, whole = _data(True, False)
    ranges = _ranges(whole)
    assert any(r1 - r0 < w for (r0, r1), w in zip(ranges, RAMP + [64] * len(ranges))), "the entry budget ends a block early"
    cutter = fa.RowCutter(ROWS, NNZ, n_blocks=3)
    sizes = dict(row_ptr=ROWS + 1, label=ROWS, field=NNZ, feat=NNZ, val=NNZ)
    try:
        # the buffers' addresses (three blocks of no rows), then every byte of them poisoned
        for _ in range(3):
            blk = cutter.close()
            assert (blk.n_rows, blk.nnz, blk.longest_row) == (0, 0, 0)
            assert lib.hipEventSynchronize(blk.ready) == 0
            assert _download(blk.row_ptr, 1, np.int32)[0] == 0
            for k, n in sizes.items():
                assert getattr(blk, k) % 16 == 0
                assert lib.hipMemset(getattr(blk, k), POISON, 4 * n) == 0
            cutter.release(blk)
        assert lib.hipDeviceSynchronize() == 0
        poison = np.uint32(0x01010101 * POISON)
        counts = {}
        seen_buffers = set()
        for (r0, r1), blk in zip(ranges, _feed(True, False, ranges, cutter, counts=counts)):
            want = _host_block(whole, r0, r1)
            assert (blk.n_rows, blk.nnz) == (r1 - r0, want.nnz)
            assert blk.longest_row == int(np.diff(want.row_ptr).max(initial=0))
            assert lib.hipEventSynchronize(blk.ready) == 0
            for k, n_valid in (("row_ptr", blk.n_rows + 1), ("label", blk.n_rows), ("field", blk.nnz), ("feat", blk.nnz), ("val", blk.nnz)):
                got = _download(getattr(blk, k), sizes[k], np.uint32)
                assert np.array_equal(got[:n_valid], np.ascontiguousarray(getattr(want, k)).view(np.uint32)), (r0, r1, k)
                assert (got[n_valid:] == poison).all(), (r0, r1, k, "bytes behind the block were written")
                # (the next block that lives here starts from poison again)
                assert lib.hipMemset(getattr(blk, k), POISON, 4 * sizes[k]) == 0
            seen_buffers.add(blk.index)
            cutter.release(blk)
        assert seen_buffers == {0, 1, 2} and counts["host"] == 0 and counts["device"] >= 3
        assert 1 in counts["spans"] and max(counts["spans"]) >= 2, counts["spans"]  # inside a chunk, and across chunks
    finally:
        cutter.destroy()


def _engine(kind, **kw):
    """(a) plain FFM; (b) hashed, rare ids folded, one field bucketed, rows normalised; fm / lr: libsvm models."""
    base = dict(max_batch_rows=ROWS, max_batch_nnz=NNZ, max_row_nnz=128, seed=3, **STRESS_HP)
    base.update(kw)
    if kind == "a":
        return fa.Engine("FFM", NF, F, K, **base)
    if kind == "b":
        e = fa.Engine("FFM", NF, F, K, hash_ids=True, normalize=True, **base)
        words = np.random.default_rng(4).integers(0, 1 << 63, size=(1 << BITS) // 64, dtype=np.uint64) * np.uint64(2)
        e.set_rare_fold(BITS, words)
        bins = np.unique(fa.value_bins(np.array([0.25, 0.5, 1.0, 2.0], np.float32))[0])
        e.set_buckets({3: bins})
        return e
    return fa.Engine(kind.upper(), NF, 1, K if kind == "fm" else 1, **base)


def _score_ring(e, n_blocks):
    buf = e.score_buffer(ROWS * n_blocks)
    return buf, [buf[i * ROWS:(i + 1) * ROWS] for i in range(n_blocks)]


def _predict_resident(e, has_field, slow, ranges, output_prob, n_blocks=3, counts=None, slot=SLOT):
    """Every block through predict_async_resident with a score buffer: (scores per block, flush loss, the ring)."""
    cutter = fa.RowCutter(ROWS, NNZ, n_blocks=n_blocks)
    ring = Ring(cutter, e)
    buf, views = _score_ring(e, len(ranges))
    try:
        for i, blk in enumerate(_feed(has_field, slow, ranges, cutter, ring.before_block, counts, slot)):
            before = e.blocks_pulled()
            e.predict_async_resident(blk, scores=views[i], output_prob=output_prob)
            assert blk.seq > before
            ring.handed_over(blk)
        loss = e.train_flush()
        assert e.blocks_scored() == ring.held[-1].seq
        return [views[i][:r1 - r0].copy() for i, (r0, r1) in enumerate(ranges)], loss, ring
    finally:
        e.sync()
        e.free_score_buffer(buf)
        cutter.destroy()


def _check_prediction(e, has_field, slow=False, counts=None, slot=SLOT):
    _, _, whole = _data(has_field, slow, slot)
    ranges = _ranges(whole)
    blocks = [_host_block(whole, r0, r1) for r0, r1 in ranges]
    for prob in (False, True):
        want = [e.predict_batch(c, output_prob=prob) for c in blocks]
        for c in blocks:  # the host form's flush loss
            e.predict_batch_async(c)
        loss_host = e.train_flush()
        got, loss, _ = _predict_resident(e, has_field, slow, ranges, prob, counts=counts, slot=slot)
        for (r0, r1), g, (w, _) in zip(ranges, got, want):
            assert_bitwise(g, w, "rows %d..%d, prob %s" % (r0, r1, prob))
        assert np.float64(loss).tobytes() == np.float64(loss_host).tobytes(), (loss, loss_host)
        assert np.float64(loss).tobytes() == np.float64(sum(ls for _, ls in want)).tobytes()


@pytest.mark.parametrize("kind", ["a", "b", "c_f16", "fm", "lr"])
def test_predict_resident_is_predict_batch_of_the_host_block(kind):
    has_field = kind not in ("fm", "lr")
    if kind == "c_f16":
        t = _engine("a")
        t.fill_state(seed=6)
        e = fa.Engine("FFM", NF, F, K, serve="f16", skip_init=True, max_batch_rows=ROWS, max_batch_nnz=NNZ, max_row_nnz=128, **STRESS_HP)
        e.pack_from(t)
        t.close()
    else:
        e = _engine(kind)
        e.fill_state(seed=6)
    try:
        _check_prediction(e, has_field)
    finally:
        e.close()


def _pinned_blocks(e, blocks):
    out = []
    for c in blocks:
        cb = synth.Block(*(None if a is None else fa.page_aligned(a.size, a.dtype) for a in (c.row_ptr, c.field, c.feat, c.val, c.label)))
        for k in ("row_ptr", "field", "feat", "val", "label"):
            getattr(cb, k)[:] = getattr(c, k)
        e.pin_block(cb)
        out.append(cb)
    return out


def _train_both(kind, has_field, slow=False, counts=None, slot=SLOT):
    """Two engines from one seed: one trained through train_batch_async_pinned on host blocks, the other through
    train_async_resident, block sizes 1, 7 and 64 in a ramp."""
    _, _, whole = _data(has_field, slow, slot)
    ranges = _ranges(whole)
    blocks = [_host_block(whole, r0, r1) for r0, r1 in ranges]
    a, b = _engine(kind), _engine(kind)
    cutter = fa.RowCutter(ROWS, NNZ, n_blocks=4)
    try:
        assert_state_bitwise(a.get_state(), b.get_state(), "twin engines")
        pinned = _pinned_blocks(a, blocks)
        try:
            for cb in pinned:
                a.train_batch_async_pinned(cb)
            loss_a = a.train_flush()
        finally:
            a.sync()
            for cb in pinned:
                a.unpin_block(cb)
        ring = Ring(cutter, b)
        for blk in _feed(has_field, slow, ranges, cutter, ring.before_block, counts, slot):
            b.train_async_resident(blk)
            ring.handed_over(blk)
        loss_b = b.train_flush()
        assert b.blocks_pulled() == len(ranges) == a.blocks_pulled()
        assert np.float64(loss_a).tobytes() == np.float64(loss_b).tobytes(), (loss_a, loss_b)
        assert_state_bitwise(a.get_state(), b.get_state(), "trained state, " + kind)
        wa, wb = a.get_weights(), b.get_weights()
        for k in wa:
            assert_bitwise(np.atleast_1d(wa[k]), np.atleast_1d(wb[k]), "weights " + k)
        assert loss_a > 0 and not np.isnan(loss_a)
    finally:
        b.sync()
        cutter.destroy()
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["a", "b", "fm"])
def test_train_resident_is_train_pinned_of_the_host_blocks(kind):
    _train_both(kind, kind != "fm")


def test_device_and_host_parsed_rows_meet_in_one_block():
    """One line carries 1e-3: its chunk is slow and goes in through take_host, its neighbours through take."""
    chunks, host, whole = _data(True, True, SLOT_MIXED)
    assert len(chunks) >= 8
    counts = {}
    e = _engine("a")
    e.fill_state(seed=6)
    try:
        _check_prediction(e, True, slow=True, counts=counts, slot=SLOT_MIXED)
    finally:
        e.close()
    assert counts["host"] == 1 and counts["device"] == len(chunks) - 1, counts
    slow_chunk = [i for i, c in enumerate(chunks) if b"1e-3" in c]
    assert len(slow_chunk) == 1 and 0 < slow_chunk[0] < len(chunks) - 1
    assert max(counts["spans"]) >= 2  # (a block holds rows of the slow chunk and of a neighbour)
    counts = {}
    _train_both("a", True, slow=True, counts=counts, slot=SLOT_MIXED)
    assert counts["host"] == 1 and counts["device"] == len(chunks) - 1, counts


def _device_block(arrays):
    """(RowsBlock, keep-alive tensors) of host arrays copied to the device by torch."""
    keep = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()}
    torch.cuda.synchronize()
    blk = fa.RowsBlock()
    for k, t in keep.items():
        setattr(blk, k, t.data_ptr())
    return blk, keep


def test_edges_and_refusals():
    e = _engine("a")
    e.fill_state(seed=6)
    cutter = fa.RowCutter(ROWS, NNZ, n_blocks=2)
    try:
        # rows with nnz == 0, and a block of no rows
        _, _, whole = _data(True, False)
        empty_rows = [r for r in range(300) if whole["row_ptr"][r + 1] == whole["row_ptr"][r]]
        assert len(empty_rows) >= 3
        c = synth.Block(np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([1, 0, 1], np.int32))
        want, want_loss = e.predict_batch(c)
        cutter.take_host(3, c.row_ptr, c.field, c.feat, c.val, c.label)
        blk = cutter.close()
        assert (blk.n_rows, blk.nnz, blk.longest_row) == (3, 0, 0)
        buf = e.score_buffer(ROWS)
        e.predict_async_resident(blk, scores=buf)
        none = cutter.close()
        assert (none.n_rows, none.nnz) == (0, 0)
        e.predict_async_resident(none, scores=buf[16:])
        loss = e.train_flush()
        assert_bitwise(buf[:3].copy(), want, "rows without entries")
        assert np.float64(loss).tobytes() == np.float64(want_loss).tobytes()
        assert e.blocks_scored() == none.seq == blk.seq + 1
        # both buffers are held: nothing goes in until one is released
        with pytest.raises(fa.EngineError) as ei:
            cutter.take_host(3, c.row_ptr, c.field, c.feat, c.val, c.label)
        assert ei.value.code == fa.engine.E_CAPACITY and "held" in str(ei.value)
        with pytest.raises(fa.EngineError):
            cutter.close()
        cutter.release(blk)
        cutter.release(none)
        with pytest.raises(fa.EngineError):
            cutter.release(none)
        # a take beyond the cutter's capacities is refused before anything is launched
        big = np.arange(ROWS + 2, dtype=np.int32)
        with pytest.raises(fa.EngineError) as ei:
            cutter.take_host(ROWS + 1, big * 0, None, None, None, np.zeros(ROWS + 1, np.int32))
        assert ei.value.code == fa.engine.E_CAPACITY
        few = np.array([0, NNZ + 1], np.int32)
        with pytest.raises(fa.EngineError) as ei:
            cutter.take_host(1, few, np.zeros(NNZ + 1, np.int32), np.zeros(NNZ + 1, np.int32), np.ones(NNZ + 1, np.float32), np.zeros(1, np.int32))
        assert ei.value.code == fa.engine.E_CAPACITY
        e.free_score_buffer(buf)

        # the host forms' refusals, code and message
        def refusal(call):
            with pytest.raises(fa.EngineError) as ei:
                call()
            return ei.value.code, str(ei.value)

        one = np.zeros(1, np.int32)
        # a longest row of max_row_nnz + 1
        n = 129
        long_row = synth.Block(np.array([0, n], np.int32), (np.arange(n) % F).astype(np.int32), (np.arange(n) % NF).astype(np.int32),
                               np.ones(n, np.float32), one)
        blk, keep = _device_block(dict(row_ptr=long_row.row_ptr, field=long_row.field, feat=long_row.feat, val=long_row.val, label=long_row.label))
        blk.n_rows, blk.nnz, blk.longest_row = 1, n, n
        host_form = refusal(lambda: e.predict_batch_async(long_row))
        assert refusal(lambda: e.predict_async_resident(blk)) == host_form and host_form[0] == fa.engine.E_CAPACITY
        assert refusal(lambda: e.train_async_resident(blk)) == refusal(lambda: e.train_batch_async(long_row))
        assert refusal(lambda: e.stage_resident(blk)) == refusal(lambda: e.stage_batch(long_row))
        # a block over max_batch_rows
        n = ROWS + 1
        many = synth.Block(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(n, np.int32))
        blk, keep2 = _device_block(dict(row_ptr=many.row_ptr, label=many.label))
        blk.n_rows, blk.nnz, blk.longest_row = n, 0, 0
        host_form = refusal(lambda: e.predict_batch_async(many))
        assert refusal(lambda: e.predict_async_resident(blk)) == host_form and host_form[0] == fa.engine.E_CAPACITY
        assert refusal(lambda: e.train_async_resident(blk)) == refusal(lambda: e.train_batch_async(many))
        # ... and over max_batch_nnz
        blk.n_rows, blk.nnz, blk.longest_row = 1, NNZ + 1, 1
        assert refusal(lambda: e.predict_async_resident(blk))[0] == fa.engine.E_CAPACITY
        # a training call on a serving engine
        s = fa.Engine("FFM", NF, F, K, serve="f32", skip_init=True, max_batch_rows=ROWS, max_batch_nnz=NNZ, max_row_nnz=128, **STRESS_HP)
        try:
            s.pack_from(e)
            ok = _host_block(whole, 0, 8)
            blk, keep3 = _device_block(dict(row_ptr=ok.row_ptr, field=ok.field, feat=ok.feat, val=ok.val, label=ok.label))
            blk.n_rows, blk.nnz, blk.longest_row = ok.n_rows, ok.nnz, int(np.diff(ok.row_ptr).max())
            host_form = refusal(lambda: s.train_batch_async(ok))
            assert refusal(lambda: s.train_async_resident(blk)) == host_form and host_form[0] == fa.engine.E_UNSUPPORTED
            assert refusal(lambda: s.stage_resident(blk)) == refusal(lambda: s.stage_batch(ok))
            # ... while it predicts such a block of the caller's own (no cutter, no event)
            buf = s.score_buffer(ROWS)
            s.predict_async_resident(blk, scores=buf)
            s.train_flush()
            assert_bitwise(buf[:ok.n_rows].copy(), s.predict_batch(ok)[0], "a caller's own block on a serving engine")
            s.free_score_buffer(buf)
        finally:
            s.close()
        # nothing refused above was counted as staged
        assert e.blocks_pulled() == none.seq
    finally:
        e.sync()
        cutter.destroy()
        e.close()


def test_a_ring_of_two_buffers_under_ten_blocks_waits_for_blocks_pulled():
    _, _, whole = _data(True, False)
    ranges = cases.reference_blocks(whole["row_ptr"], [30], NNZ)
    assert len(ranges) >= 10
    blocks = [_host_block(whole, r0, r1) for r0, r1 in ranges]
    e = _engine("a")
    e.fill_state(seed=6)
    try:
        want = [e.predict_batch(c)[0] for c in blocks]
        got, _, ring = _predict_resident(e, True, False, ranges, False, n_blocks=2)
        for g, w, r in zip(got, want, ranges):
            assert_bitwise(g, w, "rows %d..%d" % r)
        assert len(ring.held) == 2 and ring.held[-1].seq == e.blocks_pulled()
    finally:
        e.close()
