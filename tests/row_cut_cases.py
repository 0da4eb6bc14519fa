"""Texts for the resident-rows tests (tests/test_row_cut_host.py, tests/test_gpu_resident_rows.py): a few hundred rows
of the device grammar (csrc/text_parse.h "Text blocks") with every row shape a cut can meet, and the cut of a text into
chunks of whole lines that host/text_stream.cpp makes."""
import numpy as np

N_FIELDS, N_FEATS = 5, 200
VALUES = ("1", "1", "1", "0.5", "2", "0.25", "-1.5", "3", "0.125")


def make_text(n_rows=300, seed=0, has_field=True, n_fields=N_FIELDS, n_feats=N_FEATS, slow_row=None):
    """(text, entries per row): n_rows rows of 0, 1, n_fields and 3 * n_fields entries -- a label-only line and a row
    whose every value is 0 (all dropped) among the rows of 0 --, blank lines, `\\r\\n` lines, no final `\\n`.
    slow_row: that row's first value is spelled 1e-3, which the device grammar leaves to the host."""
    rng = np.random.default_rng(seed)
    kinds = [0, 1, n_fields, 3 * n_fields]
    lines, counts = [], []
    for r in range(n_rows):
        n = kinds[r] if r < 4 else int(rng.choice(kinds, p=[0.06, 0.14, 0.6, 0.2]))
        label = "1" if rng.random() < 0.4 else "0"
        toks = [label]
        if n == 0 and r % 2 == 1:  # (every value 0: all dropped)
            toks += ["%s%d:0" % ("%d:" % (j % n_fields) if has_field else "", int(rng.integers(0, n_feats))) for j in range(3)]
        for j in range(n):
            v = VALUES[int(rng.integers(0, len(VALUES)))]
            if slow_row == r and j == 0:
                v = "1e-3"
            f = "%d:" % (j % n_fields) if has_field else ""
            toks.append("%s%d:%s" % (f, int(rng.integers(0, n_feats)), v))
        line = " ".join(toks)
        if r % 37 == 5:
            line += "\r"
        lines.append(line)
        counts.append(n)
        if r % 41 == 7:
            lines.append("")  # a blank line
        if r % 53 == 11:
            lines.append("   ")
    if slow_row is not None:
        assert counts[slow_row] > 0
    return "\n".join(lines).encode(), np.array(counts, np.int64)


def chunks(text, max_bytes):
    """The text cut as host/text_stream.cpp cuts a file into slots of max_bytes: whole lines, at most max_bytes (a
    longer single line goes alone, up to its newline); the last chunk may lack its final newline."""
    out, at = [], 0
    while at < len(text):
        end = min(len(text), at + max_bytes)
        if end < len(text):
            cut = text.rfind(b"\n", at, end)
            if cut < 0:
                cut = text.find(b"\n", end)
                cut = len(text) - 1 if cut < 0 else cut
            end = cut + 1
        out.append(text[at:end])
        at = end
    return out


def reference_blocks(row_ptr, wants, max_nnz):
    """The cut rule of CsrStream::next on one row_ptr: [(r0, r1)] for a sequence of block sizes `wants` (the last one
    repeats), ending a block early rather than exceed max_nnz entries; a single row beyond it goes out alone."""
    out, r, i = [], 0, 0
    n = len(row_ptr) - 1
    while r < n:
        want = wants[min(i, len(wants) - 1)]
        i += 1
        r1 = min(n, r + want)
        while r1 > r + 1 and row_ptr[r1] - row_ptr[r] > max_nnz:
            r1 -= 1
        out.append((r, r1))
        r = r1
    return out
