"""Every row kernel against the oracle on a ladder of row lengths (util.ROW_LENGTHS: each entry count
at which fm_row_wave_kernel, fm_row_kernel, ffm_row_kernel or ffm_row_wave_kernel changes path,
with its neighbours), in blocks built by util.row_length_block: empty rows first and last, once-only
and repeated features at every position of a row, out-of-range entries in a parked position, in a
chunk and on both sides of the 64-entry pass boundary, an id twice in a long row, FFM rows with
repeated fields and in descending field order.

Every case trains two such blocks and predicts a third, from a warm state, on the oracle and on the
engine: logits (and probabilities) bit for bit, the loss sum by util.loss_close, the whole state bit
for bit after each block, the state untouched by predict.  A failure names the length of the rows
that differ.  tests/test_block_semantics.py checks on the CPU that the oracle's results in all of
these cases are finite, so nothing here passes on NaNs.

The same rows run with another LDS carve-up, another terms capacity and, on predict, another number
of launches depending on the row cap the entry point hands the kernels: the longest row of the block
(calls from host memory) or the engine's max_row_nnz (device calls).  The entry-point cases run the
host calls on the whole block (cap 150) and on util.row_cap_prefixes' pieces (caps 1, 3, 5, 64, 65, 128,
129, 150), the device calls and the split step with max_row_nnz = 160.
"""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from oracle.pyoracle import Csr
from util import (HP_SETS, ROW_ENTRY_SHAPES, ROW_FIELDS, ROW_LENGTHS, ROW_SEED, ROW_SHAPES, assert_rows_bitwise,
                  assert_state_bitwise, assert_state_rows_bitwise, loss_close, row_cap_prefixes, row_length_case,
                  row_pieces_shape, row_shape_id, take_rows)

pytestmark = pytest.mark.gpu

DEVICE_ROW_CAP = 160  # max_row_nnz of the engines the device entry points run on: above every row


def _engine(shape, nf, **kw):
    mt, k, hp_name, learn = shape
    return fa.Engine(mt, nf, ROW_FIELDS if mt == "FFM" else 1, k, skip_init=True, max_batch_rows=128,
                     learn=learn, **HP_SETS[hp_name], **kw)


class Host:
    """train_batch / predict_batch from host memory: the row cap is the block's longest row."""
    name = "host"

    def __init__(self, shape, nf):
        self.e = _engine(shape, nf)

    def train(self, blk):
        return self.e.train_batch(blk)

    def predict(self, blk, prob):
        return self.e.predict_batch(blk, output_prob=prob)


class Device:
    """train_batch_device / predict_batch_device: the row cap is the engine's max_row_nnz."""
    name = "device"

    def __init__(self, shape, nf):
        self.e = _engine(shape, nf, max_row_nnz=DEVICE_ROW_CAP)
        self.ffm = shape[0] == "FFM"

    def _upload(self, blk):
        d = {key: torch.from_numpy(np.ascontiguousarray(getattr(blk, key))).cuda()
             for key in ("row_ptr", "field", "feat", "val", "label")}
        out = torch.full((max(blk.n_rows, 1),), float("nan"), dtype=torch.float32, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        csr = (blk.n_rows, int(blk.row_ptr[-1]), d["row_ptr"].data_ptr(), d["field"].data_ptr() if self.ffm else None,
               d["feat"].data_ptr(), d["val"].data_ptr())
        return d, csr, out, loss

    def _result(self, blk, out, loss):
        self.e.sync()
        return out[:blk.n_rows].cpu().numpy(), float(loss.cpu()[0])

    def train(self, blk):
        d, csr, out, loss = self._upload(blk)
        self.e.train_batch_device(*csr, d["label"].data_ptr(), out.data_ptr(), loss.data_ptr())
        return self._result(blk, out, loss)

    def predict(self, blk, prob):
        d, csr, out, loss = self._upload(blk)
        self.e.predict_batch_device(*csr, d["label"].data_ptr(), prob, out.data_ptr(), loss.data_ptr())
        return self._result(blk, out, loss)


class Split(Device):
    """train_forward_device + train_update_device fed the engine's own logits (the row kernel leaves
    tmp_grad and the once-only features to the kernels that follow); predict_batch_device for the
    logits + predict_finish_device."""
    name = "split"

    def train(self, blk):
        d, csr, out, loss = self._upload(blk)
        part = torch.full_like(out, float("nan"))
        torch.cuda.synchronize()
        self.e.train_forward_device(*csr, d["label"].data_ptr(), part.data_ptr())
        self.e.sync()
        self.e.train_update_device(part.data_ptr(), out.data_ptr(), loss.data_ptr())
        return self._result(blk, out, loss)

    def predict(self, blk, prob):
        d, csr, out, loss = self._upload(blk)
        part = torch.full_like(out, float("nan"))
        torch.cuda.synchronize()
        self.e.predict_batch_device(*csr, None, 0, part.data_ptr(), None)
        self.e.predict_finish_device(blk.n_rows, part.data_ptr(), d["label"].data_ptr(), prob, out.data_ptr(),
                                     loss.data_ptr())
        return self._result(blk, out, loss)


DRIVERS = {"host": Host, "device": Device, "split": Split}


@functools.lru_cache(maxsize=2)
def _reference(shape):
    """The oracle's side of a case, computed once per shape: per trained block (logits, loss sum, state
    after it), for the predicted block (logits, probabilities, loss sum); the model stays at the final
    state (predict leaves it alone) for the pieces' references."""
    o, st, blocks, nf = row_length_case(shape, ROW_SEED)
    trained = []
    for blk in blocks[:2]:
        lg, ls = o.train_batch(blk)
        trained.append((lg, ls, o.get_state()))
    po, pls = o.predict_batch(blocks[2])
    pp, _ = o.predict_batch(blocks[2], output_prob=True)
    return dict(o=o, start=st, blocks=blocks, nf=nf, trained=trained, predict=(po, pp, pls))


def _check_loss(got, want, what):
    assert loss_close(got, want), "%s: loss sum %r vs %r" % (what, got, want)


def _check_predict(drv, o, blk, what, want=None):
    if want is None:
        po, pls = o.predict_batch(blk)
        want = (po, o.predict_batch(blk, output_prob=True)[0], pls)
    po, pp, pls = want
    out, ls = drv.predict(blk, False)
    assert_rows_bitwise(out, po, blk, what + " predict logits")
    _check_loss(ls, pls, what + " predict")
    out, _ = drv.predict(blk, True)
    assert_rows_bitwise(out, pp, blk, what + " predict probabilities")


def _check_case(shape, drv, what, predict_pieces=False):
    ref = _reference(shape)
    drv.e.set_state(ref["start"])
    for j, blk in enumerate(ref["blocks"][:2]):
        lg, ls, state = ref["trained"][j]
        got, gls = drv.train(blk)
        assert_rows_bitwise(got, lg, blk, "%s logits of block %d" % (what, j))
        _check_loss(gls, ls, "%s block %d" % (what, j))
        assert_state_rows_bitwise(drv.e.get_state(), state, blk, "%s state after block %d" % (what, j))
    before = drv.e.get_state()
    _check_predict(drv, ref["o"], ref["blocks"][2], what, ref["predict"])
    if predict_pieces:  # (caps 128 / 129: without / with the second predict launch)
        for piece in row_cap_prefixes(ref["blocks"][2]):
            _check_predict(drv, ref["o"], piece, "%s piece with row cap %d" % (what, np.diff(piece.row_ptr).max()))
    assert_state_bitwise(drv.e.get_state(), before, what + " state after predict")
    drv.e.close()


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=row_shape_id)
def test_every_row_length_on_every_model_shape(shape):
    """FM k = 8 (idle lanes), 33, 64 (fm_row_wave_kernel), 65, 128 (fm_row_kernel), LR, FFM k = 4, 16,
    64 (vectorised row kernel, wave predict kernel), 12 (vec4; predict keeps the workgroup kernel), 6
    (generic kernels) under the stress hyper-parameters, FFM k = 16 and FM k = 8 under the default
    ones and under the learning variant (other record words loaded by the FM wave kernel) -- from host
    memory; predict also on the row-cap pieces."""
    nf = _reference(shape)["nf"]
    _check_case(shape, Host(shape, nf), row_shape_id(shape), predict_pieces=True)


@pytest.mark.parametrize("entry", ["device", "split"])
@pytest.mark.parametrize("shape", ROW_ENTRY_SHAPES, ids=row_shape_id)
def test_every_row_length_through_the_device_entry_points(shape, entry):
    """The device calls and the split step on an engine whose max_row_nnz (160) exceeds every row: the
    oracle's bits, and therefore the host calls' (test_every_row_length_on_every_model_shape)."""
    nf = _reference(shape)["nf"]
    _check_case(shape, DRIVERS[entry](shape, nf), "%s %s" % (row_shape_id(shape), entry))


@pytest.mark.parametrize("shape", ROW_ENTRY_SHAPES, ids=row_shape_id)
def test_every_row_cap_from_host_memory(shape):
    """The row-cap pieces of each block chained as consecutive blocks on one engine: the host calls size
    the kernels by the longest row of each piece (1, 3, 5, 64, 65, 128, 129, 150).  (FM under
    util.row_pieces_shape's hyper-parameters, with which the chain's logits stay small.)"""
    shape = row_pieces_shape(shape)
    o, st, blocks, nf = row_length_case(shape, ROW_SEED)
    drv = Host(shape, nf)
    drv.e.set_state(st)
    for j in (0, 1):
        for piece in row_cap_prefixes(blocks[j]):
            what = "%s block %d, piece with row cap %d" % (row_shape_id(shape), j, np.diff(piece.row_ptr).max())
            lg, ls = o.train_batch(piece)
            got, gls = drv.train(piece)
            assert_rows_bitwise(got, lg, piece, what + " logits")
            _check_loss(gls, ls, what)
            assert_state_rows_bitwise(drv.e.get_state(), o.get_state(), piece, what + " state")
    before = drv.e.get_state()
    for piece in row_cap_prefixes(blocks[2]):
        _check_predict(drv, o, piece, "%s predict piece with row cap %d" % (row_shape_id(shape), np.diff(piece.row_ptr).max()))
    assert_state_bitwise(drv.e.get_state(), before, row_shape_id(shape) + " state after predict")
    drv.e.close()


SWITCHES = ([("FFM_PREDICT_WAVE", v, k) for k in (4, 16, 64) for v in ("0", "1")]
            + [("FFM_ENGINE_ROW_REFRESH", v, 16) for v in ("0", "3")]
            + [("FFM_ROW_THREADS", v, 16) for v in ("64", "256")])


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name,value,k", SWITCHES, ids=["%s=%s-k%d" % s for s in SWITCHES])
def test_every_row_length_under_the_row_kernel_switches(name, value, k, entry, monkeypatch):
    """FFM_PREDICT_WAVE 0 / 1 (k = 4, 16, 64), FFM_ENGINE_ROW_REFRESH 0 / 3 and FFM_ROW_THREADS 64 / 256
    (k = 16), read when the engine is created."""
    monkeypatch.setenv(name, value)
    shape = ("FFM", k, "stress_hp", False)
    nf = _reference(shape)["nf"]
    _check_case(shape, DRIVERS[entry](shape, nf), "%s %s=%s %s" % (row_shape_id(shape), name, value, entry),
                predict_pieces=entry == "host")


def _small_blocks(blk):
    """Blocks of 1, 2, 3 and 5 rows cut from the ladder block (a partial last workgroup in the wave
    kernels): the empty row alone, then short and long rows mixed."""
    lens = np.diff(blk.row_ptr)
    first = lambda n: int(np.flatnonzero(lens == n)[0])  # noqa: E731
    last = lambda n: int(np.flatnonzero(lens == n)[-1])  # noqa: E731
    return [take_rows(blk, idx) for idx in (
        [0], [first(65), 0], [first(130), first(3), first(64)], [first(150), last(0), last(1), first(129), first(4)],
        [last(2)], [first(1), last(128)], [last(0), last(92), last(0)])]


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("shape", ROW_ENTRY_SHAPES, ids=row_shape_id)
def test_blocks_of_a_few_rows(shape, entry):
    """Blocks of 1, 2, 3 and 5 rows, one of them the empty row alone (the row that stores the refreshed
    bias), trained one after the other and then predicted."""
    o, st, blocks, nf = row_length_case(shape, ROW_SEED)
    drv = DRIVERS[entry](shape, nf)
    drv.e.set_state(st)
    small = _small_blocks(blocks[0]) + _small_blocks(blocks[1])
    assert [b.n_rows for b in small[:4]] == [1, 2, 3, 5] and small[0].row_ptr[-1] == 0
    for j, blk in enumerate(small):
        what = "%s %s small block %d (rows of %s entries)" % (row_shape_id(shape), entry, j, np.diff(blk.row_ptr).tolist())
        lg, ls = o.train_batch(blk)
        got, gls = drv.train(blk)
        assert_rows_bitwise(got, lg, blk, what + " logits")
        _check_loss(gls, ls, what)
        assert_state_rows_bitwise(drv.e.get_state(), o.get_state(), blk, what + " state")
    before = drv.e.get_state()
    for j, blk in enumerate(_small_blocks(blocks[2])):
        _check_predict(drv, o, blk, "%s %s small block %d (rows of %s entries)" % (
            row_shape_id(shape), entry, j, np.diff(blk.row_ptr).tolist()))
    assert_state_bitwise(drv.e.get_state(), before, "%s %s state after predict" % (row_shape_id(shape), entry))
    drv.e.close()


SIGNED_ZERO = [("LR", 1, None), ("FFM", 4, "1"), ("FFM", 16, "1"), ("FFM", 64, "1"), ("FFM", 16, "0"), ("FFM", 12, None)]


@pytest.mark.parametrize("mt,k,wave", SIGNED_ZERO, ids=["%s-k%d-wave%s" % s for s in SIGNED_ZERO])
def test_predict_keeps_the_sign_of_a_zero_logit(mt, k, wave, monkeypatch):
    """The ordered sums pad their idle lanes, erased entries and the last partial chunk of staged terms
    with -0.0, the one value that leaves every running sum as it is: with +0.0 a running -0.0 turns
    into +0.0.  Stored weights that are signed zeros make every logit of the block -0.0 (the bias is
    -0.0; every linear product is -0.0: lin_w = -0.0 under a positive value, +0.0 under a negative one;
    FFM rows keep two entries in range, one value of each sign, so their only pair term is +0.0 * x1 * x2
    = -0.0) -- on rows of every length of the ladder, the two survivors first and last in the row and,
    from 65 entries on, at positions 63 and 64; LR rows are whole."""
    if wave is not None:
        monkeypatch.setenv("FFM_PREDICT_WAVE", wave)
    shape = (mt, k, "default_hp", False)
    o, st, _, nf = row_length_case(shape, ROW_SEED)
    per = nf // ROW_FIELDS
    rows = []
    for n in ROW_LENGTHS:
        if mt == "LR":
            rows.append([(0, (7 * len(rows) + j) % per, 0.5 + 0.25 * (j % 3)) for j in range(n)])
            continue
        for keep in ((0, n - 1), (63, 64)):
            if n < 2 or keep[1] >= n:
                continue
            r = len(rows)
            row = [((j % ROW_FIELDS, -7, 1.0), (j % ROW_FIELDS, nf + 3, 0.5), (ROW_FIELDS + 2, j, 1.0))[j % 3] for j in range(n)]
            row[keep[0]], row[keep[1]] = (0, r, 0.75), (1, per + r, -0.5)
            rows.append(row)
    blk = Csr.from_rows(rows, [r % 2 for r in range(len(rows))])
    zero = {key: np.zeros_like(a) for key, a in st.items()}
    zero["bias3"][0] = -0.0
    zero["lin_w"][:per] = -0.0
    o.set_state(zero)
    po, pls = o.predict_batch(blk)
    assert (po == 0).all() and np.signbit(po).all(), "every logit of the oracle is -0.0"
    drv = Host(shape, nf)
    drv.e.set_state(zero)
    _check_predict(drv, o, blk, "%s k=%d signed zeros" % (mt, k))
    drv.e.close()
