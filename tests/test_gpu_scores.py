"""Per-row scores out of the pipelined prediction (include/ffm_engine.h:
ffm_engine_predict_batch_async_scores / ffm_engine_blocks_scored; csrc/engine_stage.h:
push_scores_kernel): what lands in the caller's page-locked buffer is, bit for bit, what the
synchronous ffm_engine_predict_batch returns for the same rows and state; nothing is written behind
the block; a block's number is published once its scores are whole; loss sum and eval histogram do
not change; blocks without a buffer publish nothing and launch nothing; the refusals.
Tiny models: FFM 8 fields x k 16, FM k 16 and LR over 10 000 features."""
import time

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth
from oracle.pyoracle import Csr
from util import STRESS_HP, assert_bitwise, rand_state

pytestmark = pytest.mark.gpu

NF, F, K = 10000, 8, 16
MAX_ROWS = 1024
MODELS = {"FFM": ("FFM", NF, F, K), "FM": ("FM", NF, 1, K), "LR": ("LR", NF, 1, 1)}
# the row counts of the issue: n % 4 in {0, 1, 3}, one / two / many workgroups' worth, an empty block;
# 2 and 66 add n % 4 == 2.  Ten of them in a row wrap the four staging slots twice.
ROW_COUNTS = (0, 1, 3, 63, 64, 65, 257, 1000, 2, 66)
CANARY = np.uint32(0xC0FFEE42)
PAD = 8


def make_block(mt, n, seed):
    """n rows of one entry per field (FM / LR: field 0 everywhere); every seventh row (r % 7 == 3) empty."""
    g = synth.Generator(F, NF, "zipf", seed=seed).block(max(n, 1))
    lens = np.diff(g.row_ptr)[:n]
    keep = (np.arange(n) % 7 != 3)
    sel = np.repeat(keep, lens)
    nnz = int(lens.sum())
    field = g.field[:nnz][sel].copy()
    if mt != "FFM":
        field[:] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens * keep)]).astype(np.int32)
    return Csr(row_ptr, field, g.feat[:nnz][sel].copy(), g.val[:nnz][sel].copy(), g.label[:n].copy())


def own_pages(c):
    def cp(a):
        out = fa.page_aligned(a.size, a.dtype)
        out[:] = a
        return out
    return Csr(cp(c.row_ptr), cp(c.field), cp(c.feat), cp(c.val), cp(c.label))


def make_engine(mt, seed=5, **kw):
    name, nf, nfld, k = MODELS[mt]
    e = fa.Engine(name, nf, nfld, k, skip_init=True, max_batch_rows=MAX_ROWS, **dict(STRESS_HP, **kw))
    st = rand_state(np.random.default_rng(seed), e)
    for key in ("vec_n", "lin_n"):
        st[key] += np.float32(0.05)
    e.set_state(st)
    return e


class Buffers:
    """Score buffers of one engine, each PAD floats longer than its block and filled with a canary."""

    def __init__(self, e):
        self.e, self.bufs = e, []

    def new(self, n):
        a = self.e.score_buffer(n + PAD)
        a.view(np.uint32)[:] = CANARY
        self.bufs.append(a)
        return a

    def close(self):
        for a in self.bufs:
            self.e.free_score_buffer(a)


def assert_canaries(buf, n, what):
    tail = buf.view(np.uint32)[n:]
    assert tail.size == PAD and (tail == CANARY).all(), "%s: written behind row %d: %s" % (what, n, tail)


_reference = {}


def reference(mt):
    """(blocks, logits, probabilities, loss sums) of ROW_COUNTS through the synchronous predict_batch:
    computed once per model type, shared by the tests, never written to."""
    if mt not in _reference:
        e = make_engine(mt)
        blocks = [make_block(mt, n, 100 + i) for i, n in enumerate(ROW_COUNTS)]
        logit, prob, loss = [], [], []
        for b in blocks:
            lg, ls = e.predict_batch(b, output_prob=False)
            pr, _ = e.predict_batch(b, output_prob=True)
            for a in (lg, pr):
                a.setflags(write=False)
            logit.append(lg)
            prob.append(pr)
            loss.append(ls)
        e.close()
        _reference[mt] = (blocks, logit, prob, loss)
    return _reference[mt]


@pytest.mark.parametrize("zero_copy", [False, True], ids=["copied", "zero_copy"])
@pytest.mark.parametrize("output_prob", [False, True], ids=["logit", "prob"])
@pytest.mark.parametrize("mt", ["FFM", "FM", "LR"])
def test_scores_match_the_synchronous_call_bit_for_bit(mt, output_prob, zero_copy):
    """Ten scored blocks in a row (more than the four staging slots: numbers and slots wrap), rows of
    0..1000 with empty rows among them: after the flush every buffer holds predict_batch's bits, the
    canaries behind every block are intact, blocks_scored() is the last staging number, and the
    flush returns the loss sum of the synchronous calls."""
    blocks, logit, prob, loss = reference(mt)
    want = prob if output_prob else logit
    e = make_engine(mt)
    bufs = Buffers(e)
    host = [own_pages(b) for b in blocks] if zero_copy else blocks
    if zero_copy:
        for b in host:
            e.pin_block(b)
    assert e.blocks_scored() == 0
    outs = [bufs.new(b.n_rows) for b in blocks]
    seen = [0]
    for b, out in zip(host, outs):
        e.predict_batch_async(b, zero_copy=zero_copy, scores=out, output_prob=output_prob)
        seen.append(e.blocks_scored())
    total = e.train_flush()
    seen.append(e.blocks_scored())
    assert e.blocks_scored() == len(blocks) == e.blocks_pulled()
    assert all(a <= b for a, b in zip(seen, seen[1:])), seen
    for i, (b, out) in enumerate(zip(blocks, outs)):
        what = "%s block %d (%d rows)" % (mt, i, b.n_rows)
        assert_bitwise(out[:b.n_rows], want[i], what)
        assert_canaries(out, b.n_rows, what)
    assert abs(total - sum(loss)) <= 1e-9 * max(1.0, abs(sum(loss))), (total, sum(loss))
    if zero_copy:
        for b in host:
            e.unpin_block(b)
    bufs.close()
    e.close()


def test_nan_logits_arrive_as_nan():
    """NaN logits (what the reference's sqrt(n + g2 * g1) leaves behind when n is near 0 and the sum
    negative, tests/test_gpu_scale.py::test_quirk_nans_flow_through_the_folds -- put into the state
    directly here: a negative n, a NaN w and |z| > l1 in every latent slot of the field-0 features with
    an odd id): the rows that hold such a feature score NaN, the others stay finite, and the buffer has
    the NaNs where the synchronous call has them, as logits and as probabilities."""
    rng = np.random.default_rng(23)
    e = fa.Engine("FFM", NF, F, K, skip_init=True, max_batch_rows=MAX_ROWS, **STRESS_HP)
    st = rand_state(rng, e)
    for key in ("vec_n", "lin_n"):
        st[key] += np.float32(0.05)
    odd = np.arange(1, NF // F, 2)  # field 0 owns ids [0, NF / F)
    st["vec_n"][odd] = np.float32(-0.5)
    st["vec_z"][odd] = np.float32(0.7)
    st["vec_w"][odd] = np.float32(np.nan)
    e.set_state(st)
    score = synth.Generator(F, NF, "zipf", seed=8).block(257)
    expect_nan = score.feat.reshape(257, F)[:, 0] % 2 == 1
    assert expect_nan.any() and not expect_nan.all()
    bufs = Buffers(e)
    for output_prob in (False, True):
        want, _ = e.predict_batch(score, output_prob=output_prob)
        assert np.array_equal(np.isnan(want), expect_nan), "the case must score NaN exactly where a row holds an odd field-0 id"
        out = bufs.new(score.n_rows)
        e.predict_batch_async(score, scores=out, output_prob=output_prob)
        e.sync()
        assert_bitwise(out[:score.n_rows], want, "NaN scores, output_prob=%d" % output_prob)
        assert_canaries(out, score.n_rows, "NaN scores")
    bufs.close()
    e.close()


@pytest.mark.parametrize("grid", ["1", "3", "24", None], ids=["grid1", "grid3", "grid24", "default"])
def test_every_grid_width_moves_the_same_scores(grid, monkeypatch):
    """FFM_GRID_PUSH sets the download kernel's workgroups.  A block of 4099 rows is 1024 lanes of four
    rows and three single rows: one workgroup walks it in four strides, three in two (the second partly
    filled), the default takes four workgroups of one store per lane; then 257 and 3 rows through the
    same engine (fewer lanes than one workgroup: the grid shrinks with the block)."""
    if grid is None:
        monkeypatch.delenv("FFM_GRID_PUSH", raising=False)
    else:
        monkeypatch.setenv("FFM_GRID_PUSH", grid)
    name, nf, nfld, k = MODELS["LR"]
    e = fa.Engine(name, nf, nfld, k, skip_init=True, max_batch_rows=4099, **STRESS_HP)
    e.set_state(rand_state(np.random.default_rng(5), e))
    bufs = Buffers(e)
    blocks = [make_block("LR", n, 300 + n) for n in (4099, 257, 3)]
    want = [e.predict_batch(b, output_prob=True)[0] for b in blocks]
    outs = [bufs.new(b.n_rows) for b in blocks]
    for b, out in zip(blocks, outs):
        e.predict_batch_async(b, scores=out, output_prob=True)
    e.sync()
    assert e.blocks_scored() == 3
    for b, out, w in zip(blocks, outs, want):
        assert_bitwise(out[:b.n_rows], w, "FFM_GRID_PUSH=%s, %d rows" % (grid, b.n_rows))
        assert_canaries(out, b.n_rows, "FFM_GRID_PUSH=%s, %d rows" % (grid, b.n_rows))
    bufs.close()
    e.close()


@pytest.mark.parametrize("mt", ["FFM", "LR"])
def test_scores_are_visible_without_a_flush(mt):
    """sync() after blocks 1..3: blocks_scored() == 3 and all three buffers are whole.  Then, block by
    block: once block t + 1 is handed over, blocks_scored() reaches t within 5 s (the predict launch of
    a block is deferred by one call) and buffer t is whole when it does; the count never goes back."""
    blocks, logit, _, _ = reference(mt)
    order = [7, 6, 5, 4, 3, 7, 1, 0, 2, 6, 7]  # (1000, 257, 65, ... rows; empty and tiny blocks in between)
    e = make_engine(mt)
    bufs = Buffers(e)
    outs = []
    for i in order[:3]:
        outs.append(bufs.new(blocks[i].n_rows))
        e.predict_batch_async(blocks[i], scores=outs[-1])
    e.sync()
    assert e.blocks_scored() == 3
    for j, i in enumerate(order[:3]):
        assert_bitwise(outs[j][:blocks[i].n_rows], logit[i], "after sync, block %d" % (j + 1))
    last = 3
    for n in range(4, len(order) + 1):  # hand over block number n, then wait for number n - 1
        i = order[n - 1]
        outs.append(bufs.new(blocks[i].n_rows))
        e.predict_batch_async(blocks[i], scores=outs[-1])
        deadline = time.monotonic() + 5.0
        while True:
            now = e.blocks_scored()
            assert now >= last, (now, last)
            last = now
            if now >= n - 1 or time.monotonic() > deadline:
                break
        assert last >= n - 1, "block %d was not published within 5 s of handing over block %d" % (n - 1, n)
        # (no engine call in between: the buffer is read the moment the number is seen)
        j = order[n - 2]
        assert_bitwise(outs[n - 2][:blocks[j].n_rows], logit[j], "polled, block %d" % (n - 1))
    e.train_flush()
    assert e.blocks_scored() == len(order)
    for j, i in enumerate(order):
        assert_bitwise(outs[j][:blocks[i].n_rows], logit[i], "after the flush, block %d" % (j + 1))
        assert_canaries(outs[j], blocks[i].n_rows, "block %d" % (j + 1))
    bufs.close()
    e.close()


@pytest.mark.parametrize("mt", ["FFM", "FM", "LR"])
def test_loss_sum_and_eval_histogram_do_not_change(mt):
    """The same labelled blocks once with and once without score buffers (logits and probabilities):
    identical flush sums (the same bits) and identical eval-channel histograms."""
    blocks, _, _, _ = reference(mt)
    got = []
    for mode in ("none", "logit", "prob"):
        e = make_engine(mt)
        e.metrics_enable(eval=True)
        bufs = Buffers(e)
        for b in blocks:
            out = None if mode == "none" else bufs.new(b.n_rows)
            e.predict_batch_async(b, scores=out, output_prob=mode == "prob")
        total = e.train_flush()
        pos, neg = e.metrics_histogram("eval")
        got.append((total, pos, neg, e.metrics("eval")["n_nan"]))
        bufs.close()
        e.close()
    assert got[0][1].sum() + got[0][2].sum() == sum(ROW_COUNTS)
    for other, mode in ((got[1], "logit"), (got[2], "prob")):
        assert np.float64(other[0]).view(np.uint64) == np.float64(got[0][0]).view(np.uint64), (mode, other[0], got[0][0])
        assert np.array_equal(other[1], got[0][1]) and np.array_equal(other[2], got[0][2]), mode
        assert other[3] == got[0][3]


def test_mixed_sequences_publish_only_scored_blocks():
    """Blocks with and without a buffer interleaved: blocks_scored() moves only at the scored ones
    (to their staging numbers), the unscored ones still count in the loss; with scores=None the
    profile lists no push_scores launch, with scores one per scored block."""
    blocks, logit, prob, loss = reference("FFM")
    e = make_engine("FFM")
    bufs = Buffers(e)
    e.profile_enable(True)
    for i in (7, 5, 3):
        e.predict_batch_async(blocks[i])
    first = e.train_flush()
    assert "push_scores" not in e.profile_dump(), e.profile_dump()
    assert "row_kernel<predict>" in e.profile_dump()
    assert e.blocks_scored() == 0 and e.blocks_pulled() == 3
    assert abs(first - (loss[7] + loss[5] + loss[3])) <= 1e-9 * abs(first)
    e.profile_enable(False)
    # numbers 4..10; scored: 5 (prob), 6 (logit), 9 (empty block), 10 (logit)
    plan = [(7, None), (6, True), (5, False), (4, None), (2, None), (0, False), (7, False)]
    outs, want_scored, expect = [], 0, []
    e.profile_enable(True)
    for j, (i, mode) in enumerate(plan):
        out = None if mode is None else bufs.new(blocks[i].n_rows)
        outs.append(out)
        e.predict_batch_async(blocks[i], scores=out, output_prob=bool(mode))
        e.sync()  # (launches the deferred block: everything handed over so far is done)
        if mode is not None:
            want_scored = 4 + j
        assert e.blocks_scored() == want_scored, (j, e.blocks_scored(), want_scored)
        expect.append(want_scored)
    assert expect == [0, 5, 6, 6, 6, 9, 10]
    dump = e.profile_dump()
    line = [ln for ln in dump.splitlines() if ln.startswith("push_scores_kernel")]
    assert len(line) == 1 and "launches=     4" in line[0], dump
    total = e.train_flush()
    assert abs(total - sum(loss[i] for i, _ in plan)) <= 1e-9 * abs(total)
    for (i, mode), out in zip(plan, outs):
        if mode is not None:
            assert_bitwise(out[:blocks[i].n_rows], (prob if mode else logit)[i], "mixed, block of %d rows" % blocks[i].n_rows)
            assert_canaries(out, blocks[i].n_rows, "mixed")
    bufs.close()
    e.close()


def test_refusals():
    """FFM_E_INVALID with its message: a score pointer offset by 4 bytes, a sharded engine, a staged
    training block still waiting.  A refused call stages nothing: the numbering goes on unbroken."""
    blocks, logit, _, _ = reference("FFM")
    blk = blocks[5]
    e = make_engine("FFM")
    bufs = Buffers(e)
    out = bufs.new(blk.n_rows + 4)
    with pytest.raises(fa.EngineError) as ei:
        e.predict_batch_async(blk, scores=out[1:])
    assert ei.value.code == -1 and "16-byte aligned" in str(ei.value)
    assert (out.view(np.uint32) == CANARY).all()
    e.stage_batch(blk)
    with pytest.raises(fa.EngineError) as ei:
        e.predict_batch_async(blk, scores=out)
    assert ei.value.code == -1 and "staged training blocks are still waiting" in str(ei.value)
    e.train_flush()  # (trains the staged block: number 1)
    lg, _ = e.predict_batch(blk)
    e.predict_batch_async(blk, scores=out)
    e.sync()
    assert e.blocks_scored() == 2 == e.blocks_pulled()
    assert_bitwise(out[:blk.n_rows], lg, "after the refusals")
    assert (out.view(np.uint32)[blk.n_rows:] == CANARY).all()
    bufs.close()
    e.close()
    name, nf, nfld, k = MODELS["FFM"]
    s = fa.Engine(name, nf, nfld, k, max_batch_rows=MAX_ROWS, n_shards=2, shard_rank=0, **STRESS_HP)
    buf = s.score_buffer(blk.n_rows)
    with pytest.raises(fa.EngineError) as ei:
        s.predict_batch_async(blk, scores=buf)
    assert ei.value.code == -1 and "sharded engine" in str(ei.value)
    assert s.blocks_scored() == 0
    s.free_score_buffer(buf)
    s.close()
