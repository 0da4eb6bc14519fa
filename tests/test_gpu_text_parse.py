"""The device text parser (include/ffm_engine.h "Text blocks", csrc/kernels_text.h) against its host twin
ffm_engine_textparse_host -- itself held against the CLI's real parser in tests/test_text_parse_host.py --, counts and
arrays bit for bit: both file types, zero_copy on and off, both slots, every boundary the kernels have (the 16-byte
lane, the wave step, the newline tiles, the line tiles, the one-workgroup scans' chunks), slow lines, capacities,
refusals, and the parsed arrays handed straight to an engine's _device entry points."""
import ctypes

import numpy as np
import pytest
import torch  # (first: one HIP runtime per process)

import ftrl_ffm_amd as fa
from ftrl_ffm_amd import synth

import text_parse_cases as cases

pytestmark = pytest.mark.gpu

MAX_BYTES, MAX_ROWS, MAX_NNZ = 5 << 18, 600000, 300000
COUNTS = ("n_lines", "n_rows", "nnz", "n_slow", "first_slow_byte", "overflow")
DTYPES = dict(row_ptr=np.int32, label=np.int32, field=np.int32, feat=np.int32, val=np.uint32)


def _download(addr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        lib = fa.load_library()
        lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert lib.hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


class Pinned:
    """A page-locked copy of a text."""

    def __init__(self, text):
        self.lib = fa.load_library()
        self.a = fa.page_aligned(max(len(text), 1), np.uint8)
        self.a[:len(text)] = np.frombuffer(text, np.uint8)
        assert self.lib.ffm_engine_pin_host(self.a.ctypes.data, self.a.nbytes) == 0
        self.view = self.a[:len(text)]

    def close(self):
        self.lib.ffm_engine_unpin_host(self.a.ctypes.data)


def _check(tp, text, has_field, slot=0, zero_copy=False, what=""):
    """Parses `text` on the device and holds the block against the twin's.  Returns the twin's block."""
    want = fa.parse_text_host(text, has_field=has_field, max_rows=tp.max_rows, max_nnz=tp.max_nnz)
    pin = Pinned(text) if zero_copy else None
    try:
        tp.parse(pin.view if pin else text, slot=slot, zero_copy=zero_copy)
        got = tp.wait(slot)
    finally:
        if pin:
            pin.close()
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    if want["n_slow"] == 0 and want["overflow"] == 0:
        R, E = want["n_rows"], want["nnz"]
        for k, n in (("row_ptr", R + 1), ("label", R), ("field", E), ("feat", E), ("val", E)):
            dev = _download(got[k], n, DTYPES[k])
            assert np.array_equal(dev, want[k].view(DTYPES[k])), (what, k)
    return want


@pytest.fixture(scope="module")
def parsers():
    made = {hf: fa.TextParser(has_field=hf, max_bytes=MAX_BYTES, max_rows=MAX_ROWS, max_nnz=MAX_NNZ) for hf in (True, False)}
    yield made
    for tp in made.values():
        tp.close()


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_fast_texts_both_slots_and_copies(parsers, has_field):
    tp = parsers[has_field]
    for i, (name, text) in enumerate(cases.fast_texts(has_field).items()):
        for slot, zc in ((i & 1, False), (1 - (i & 1), True)):
            want = _check(tp, text, has_field, slot, zc, name)
            assert want["n_slow"] == 0, name


def test_two_slots_in_flight(parsers):
    tp = parsers[True]
    texts = cases.fast_texts(True)
    a, b = texts["synth39"], texts["values"]
    tp.parse(a, slot=0)
    tp.parse(b, slot=1)
    ga, gb = tp.wait(0), tp.wait(1)
    for got, text in ((ga, a), (gb, b)):
        want = fa.parse_text_host(text)
        assert all(got[k] == want[k] for k in COUNTS)
        assert np.array_equal(_download(got["val"], want["nnz"], np.uint32), want["val"].view(np.uint32))
        assert np.array_equal(_download(got["row_ptr"], want["n_rows"] + 1, np.int32), want["row_ptr"])


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_tokens_per_line(parsers, has_field):
    """0 .. 300 entries in a line, short tokens (several start in one lane's 16 bytes) and long ones."""
    rng = np.random.default_rng(3)
    for tok_kind in ("short", "long"):
        lines = []
        for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 5):
            toks = ["1"]
            for j in range(n):
                if tok_kind == "short":
                    toks.append(cases._entry(has_field, j % 10, int(rng.integers(0, 10)), "1"))
                else:
                    toks.append(cases._entry(has_field, int(rng.integers(0, 10 ** 9)), int(rng.integers(0, 10 ** 9)),
                                             "-%d.%06d" % (rng.integers(0, 3), rng.integers(0, 10 ** 6))))
            lines.append(" ".join(toks))
        text = ("\n".join(lines) + "\n").encode()
        want = _check(parsers[has_field], text, has_field, 0, False, tok_kind)
        assert want["n_rows"] == 11 and want["n_slow"] == 0


def _line_of_length(L, lb, has_field):
    """A line of L bytes that begins at text offset lb, with a token across every wave-step boundary it reaches."""
    tok = cases._entry(has_field, 12, 345678, "0.25") if has_field else cases._entry(False, 0, 1234567, "-1.25")
    n = len(tok)
    s = "1"
    first = (lb & ~15) - lb  # where the wave's first step begins, relative to the line
    for k in (1, 2, 3):
        B = first + k * fa.TEXT_TILE_BYTES
        if B + n > L:
            break
        while len(s) + 1 + n < B - n // 2:
            s += " " + tok
        s += " " * (B - n // 2 - len(s)) + tok
        assert len(s) > B > len(s) - n
    while len(s) + 1 + n <= L:
        s += " " + tok
    return s.ljust(L)


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_line_lengths_around_the_wave_step(parsers, has_field):
    T = fa.TEXT_TILE_BYTES
    for lead in (b"", b"0\n", b"0 \n   \n1\n"):  # the line begins on and off a 16-byte boundary
        for L in [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)] + [15, 16, 17, 31, 32, 33]:
            for tail in (b"\n", b"", b"\r\n"):
                text = lead + _line_of_length(L, len(lead), has_field).encode() + tail
                want = _check(parsers[has_field], text, has_field, 0, False, (lead, L, tail))
                assert want["n_slow"] == 0 and want["n_rows"] == lead.count(b"0") + lead.count(b"1") + 1


def test_degenerate_texts(parsers):
    for has_field in (True, False):
        tp = parsers[has_field]
        for text, rows in ((b"", 0), (b"\n", 0), (b"1", 1), (b"\n\n \n\r\n   \n", 0), (b" \n" * 300, 0),
                           (("1 " + cases._entry(has_field, 1, 2, "0.5")).encode(), 1)):
            for slot in (0, 1):
                assert _check(tp, text, has_field, slot, slot == 1, text[:8])["n_rows"] == rows


def test_scan_boundaries(parsers):
    """Line counts around the line tile, the line-tile scan's chunk, the newline tile and the newline scan's chunk."""
    tp = parsers[True]
    lt, ch, sb = fa.TEXT_LINE_TILE, fa.TEXT_SCAN_CHUNK, fa.TEXT_SCAN_BYTES
    counts = {70001}
    for at in (lt, lt * ch, sb // 2, sb * ch // 2):  # ("1\n" is two bytes a line)
        counts |= {at - 1, at, at + 1}
    for n in sorted(counts):
        text = b"1\n" * (n - 1) + b"0"
        want = _check(tp, text, True, n & 1, False, n)
        assert want["n_rows"] == n and want["nnz"] == 0
    mixed = (b"1 1:2:3\n\n" * 40000)
    assert _check(tp, mixed, True)["n_lines"] == 80000


@pytest.mark.parametrize("has_field", [True, False], ids=["libffm", "libsvm"])
def test_slow_lines(parsers, has_field):
    tp = parsers[has_field]
    slow = cases.slow_lines(has_field)
    texts = {name: cases.around(has_field, line) for name, line in slow.items()}
    for name, (text, offset) in texts.items():
        want = _check(tp, text, has_field, 0, False, name)
        assert want["n_slow"] == 1 and want["first_slow_byte"] == offset, name
    two = texts["nan"][0] + texts["exponent"][0]
    want = _check(tp, two, has_field, 1, True, "two")
    assert want["n_slow"] == 2 and want["first_slow_byte"] == texts["nan"][1]
    many = b"".join(t for t, _ in texts.values()) * 10  # slow lines in many workgroups: the smallest offset wins
    want = _check(tp, many, has_field, 0, False, "many")
    assert want["n_slow"] == 10 * len(texts) and want["first_slow_byte"] == texts["exponent"][1]
    eight = b"1 " + b"a " * 40 + b"\n"  # eight token starts in one lane's 16 bytes
    assert _check(tp, b"1\n" + eight, has_field)["first_slow_byte"] == 2
    assert _check(tp, texts["exponent"][0].replace(b"1e-3", b"1.5"), has_field)["n_slow"] == 0  # the slot parses on


def test_capacity_and_refusals():
    text = cases.fast_texts(True)["synth"]
    full = fa.parse_text_host(text)
    R, E = full["n_rows"], full["nnz"]
    small = b"1 0:1:0.5 1:2:1\n0 3:4:2\n"
    for kw in (dict(max_rows=R - 1, max_nnz=E), dict(max_rows=R, max_nnz=E - 1)):
        tp = fa.TextParser(has_field=True, max_bytes=len(text), **kw)
        for slot in (0, 1):
            got = _check(tp, text, True, slot, False, kw)
            assert got["overflow"] == 1 and (got["n_rows"], got["nnz"]) == (R, E)
            assert _check(tp, small, True, slot, False, "after overflow")["n_rows"] == 2
        tp.close()
    tp = fa.TextParser(has_field=True, max_bytes=len(text), max_rows=R, max_nnz=E)
    assert _check(tp, text, True)["overflow"] == 0
    with pytest.raises(fa.EngineError) as ei:
        tp.parse(text + b"\n")
    assert ei.value.code == -1 and "max_bytes" in str(ei.value)
    for slot in (2, -1):
        with pytest.raises(fa.EngineError):
            tp.parse(small, slot=slot)
        with pytest.raises(fa.EngineError):
            tp.wait(slot)
    tp.parse(small, slot=1)
    with pytest.raises(fa.EngineError) as ei:
        tp.parse(small, slot=1)
    assert ei.value.code == -1 and "not waited for" in str(ei.value)
    assert tp.wait(1)["n_rows"] == 2
    with pytest.raises(fa.EngineError):
        tp.wait(1)
    with pytest.raises(fa.EngineError):
        tp.parse(np.zeros(16, np.uint8), slot=0, zero_copy=True)  # not page-locked
    assert _check(tp, small, True)["n_rows"] == 2
    tp.close()
    for bad in (dict(max_bytes=0), dict(max_bytes=1 << 31), dict(max_rows=0), dict(max_nnz=0)):
        with pytest.raises(fa.EngineError):
            fa.TextParser(**{**dict(has_field=True, max_bytes=64, max_rows=4, max_nnz=4), **bad})


def test_parsed_arrays_feed_the_device_entry_points(parsers):
    """train_batch_device / predict_batch_device on the parser's arrays against train_batch / predict_batch on the
    host-parsed block: logits, loss and state bit for bit."""
    F, K, N = 4, 4, 300
    blk = synth.Generator(F, 4000, "zipf", seed=21).block(N)
    text = synth.to_libffm_text(blk).encode()
    host = fa.parse_text_host(text)
    c = synth.Block(host["row_ptr"], host["field"], host["feat"], host["val"], host["label"])
    assert c.n_rows == N
    tp = parsers[True]
    hp = dict(w_alpha=0.05, w_l1=0.001, w_l2=0.1, seed=5, max_batch_rows=N, max_batch_nnz=N * F)
    a, b = fa.Engine("FFM", 4000, F, K, **hp), fa.Engine("FFM", 4000, F, K, **hp)
    out = torch.zeros(N, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for step in range(2):
        tp.parse(text, slot=step)
        d = tp.wait(step)
        assert (d["n_rows"], d["nnz"], d["n_slow"], d["overflow"]) == (N, int(host["nnz"]), 0, 0)
        args = (N, d["nnz"], d["row_ptr"], d["field"], d["feat"], d["val"], d["label"])
        a.predict_batch_device(*args, False, out.data_ptr(), loss.data_ptr())
        a.sync()
        want_out, want_loss = b.predict_batch(c)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out.view(np.uint32)), step
        assert float(loss.cpu()[0]) == want_loss
        a.train_batch_device(*args, out.data_ptr(), loss.data_ptr())
        a.sync()
        want_out, want_loss = b.train_batch(c)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out.view(np.uint32)), step
        assert float(loss.cpu()[0]) == want_loss
    sa, sb = a.get_state(), b.get_state()
    for k in sb:
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
    assert a.changed_features().size > 0
    a.close()
    b.close()
