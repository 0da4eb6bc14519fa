"""The definition of Engine.score_items (include/ffm_engine.h "Scoring a catalogue: items of several entries") without
a GPU: score_items_reference plus a float64 base equals the plain float64 FFM logit of spell_out_items' rows."""
import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

F, K, M, PER = 4, 4, 3, 9


def logit64(w, F, k, row):
    """bias + linear terms + every pair (a < b) of the surviving entries (field, id, value) of one row."""
    n = len(w["lin_w"])
    W = w["vec_w"].reshape(n, F, k)
    ent = [(f, i, x) for f, i, x in row if 0 <= i < n and 0 <= f < F]
    out = float(w["bias"]) + sum(x * w["lin_w"][i] for _, i, x in ent)
    for a in range(len(ent)):
        for b in range(a + 1, len(ent)):
            (fa_, ia, xa), (fb, ib, xb) = ent[a], ent[b]
            out += xa * xb * float(W[ia, fb] @ W[ib, fa_])
    return out


@pytest.mark.parametrize("with_val", (False, True))
def test_reference_is_the_logit_of_the_spelled_out_rows(with_val):
    rng = np.random.default_rng(7)
    n = F * PER
    w = dict(bias=rng.normal(), lin_w=rng.normal(size=n), vec_w=rng.normal(size=n * F * K))
    rows = [[(0, 3, 0.5), (2, 2 * PER + 1, -1.25), (2, 2 * PER + 4, 2.0)], [], [(1, n, 1.0), (3, 3 * PER, 0.75)]]  # (one erased id)
    flat = [e for r in rows for e in r]
    ctx = Block(np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.array([e[0] for e in flat], np.int32),
                np.array([e[1] for e in flat], np.int32), np.array([e[2] for e in flat], np.float32), np.zeros(len(rows), np.int32))
    fld = np.array([3, 0, 2], np.int32)
    feat = (fld[None, :] * PER + rng.integers(PER, size=(5, M))).astype(np.int32)
    feat[1, 1], feat[3, 0], feat[4] = -1, n, feat[0]  # erased slots below and above the range; a repeated item
    val = np.array([1.5, -0.5, 0.25], np.float32) if with_val else None
    ref, scale = fa.score_items_reference(w, ctx, fld, feat, val, n_fields=F)
    sp = fa.spell_out_items(ctx, fld, feat, val)
    assert sp.n_rows == len(rows) * 5 and ref.shape == scale.shape == (len(rows), 5)
    for r in range(len(rows)):
        base = logit64(w, F, K, rows[r])
        for c in range(5):
            q = r * 5 + c
            lo, hi = sp.row_ptr[q], sp.row_ptr[q + 1]
            row = list(zip(sp.field[lo:hi].tolist(), sp.feat[lo:hi].tolist(), sp.val[lo:hi].astype(np.float64).tolist()))
            assert row[:len(rows[r])] == [(f, i, float(np.float32(x))) for f, i, x in rows[r]] and len(row) == len(rows[r]) + M
            want = logit64(w, F, K, row)
            assert abs(base + ref[r, c] - want) <= 1e-12 * max(1.0, abs(want)), (r, c)
            assert scale[r, c] >= 0.0
    assert np.array_equal(ref[:, 4], ref[:, 0])
