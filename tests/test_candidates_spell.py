"""spell_out_candidates (ftrl-ffm_amd/engine.py): the semantics of Engine.score_candidates in executable form --
row c of the result is the context of candidate c's request followed by the candidate's own entries.  Hand-written
cases with the expected arrays written out; needs no GPU.  Also: the header declares both entry points and keeps
the ABI version, and the binding binds them."""
import os

import numpy as np
import pytest

import ftrl_ffm_amd as fa
from ftrl_ffm_amd.synth import Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block(rows, val=True):
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return Block(ptr, np.array([e[0] for e in flat], np.int32), np.array([e[1] for e in flat], np.int32),
                 np.array([e[2] for e in flat], np.float32) if val else None, np.zeros(len(rows), np.int32))


def same(got, row_ptr, field, feat, val):
    assert got.row_ptr.dtype == np.int32 and got.field.dtype == np.int32 and got.feat.dtype == np.int32
    assert got.val.dtype == np.float32 and got.label.dtype == np.int32
    assert got.row_ptr.tolist() == row_ptr
    assert got.field.tolist() == field
    assert got.feat.tolist() == feat
    assert got.val.view(np.uint32).tolist() == np.array(val, np.float32).view(np.uint32).tolist()  # (-0.0 stays -0.0)
    assert got.label.tolist() == [0] * (len(row_ptr) - 1)


def test_two_requests_the_second_without_candidates():
    ctx = block([[(0, 10, 0.5), (1, 20, 2.0)], [(0, 11, 1.0)]])
    cand = block([[(2, 30, 1.5)], [], [(2, 31, -0.0), (3, 40, 3.0)]])
    got = fa.spell_out_candidates(ctx, [0, 3, 3], cand)
    same(got, [0, 3, 5, 9],
         [0, 1, 2, 0, 1, 0, 1, 2, 3],
         [10, 20, 30, 10, 20, 10, 20, 31, 40],
         [0.5, 2.0, 1.5, 0.5, 2.0, 0.5, 2.0, -0.0, 3.0])


def test_first_request_without_candidates_and_an_empty_context():
    ctx = block([[(0, 10, 0.5), (1, 20, 2.0)], []])
    cand = block([[(2, 7, 4.0), (0, 8, 0.25)], []])
    got = fa.spell_out_candidates(ctx, np.array([0, 0, 2], np.int32), cand)
    same(got, [0, 2, 2], [2, 0], [7, 8], [4.0, 0.25])


def test_val_none_reads_as_ones():
    ctx = block([[(0, 10, 0.5), (1, 20, 2.0)], [(1, 21, 3.0)]], val=False)
    cand = block([[(2, 30, 1.5)], [(3, 41, 7.0), (2, 32, 0.5)]])
    got = fa.spell_out_candidates(ctx, [0, 1, 2], cand)
    same(got, [0, 3, 6], [0, 1, 2, 1, 3, 2], [10, 20, 30, 21, 41, 32], [1.0, 1.0, 1.5, 1.0, 7.0, 0.5])
    cand.val = None
    got = fa.spell_out_candidates(ctx, [0, 1, 2], cand)
    same(got, [0, 3, 6], [0, 1, 2, 1, 3, 2], [10, 20, 30, 21, 41, 32], [1.0] * 6)
    ctx = block([[(0, 10, 0.5), (1, 20, 2.0)], [(1, 21, 3.0)]])
    got = fa.spell_out_candidates(ctx, [0, 1, 2], cand)
    same(got, [0, 3, 6], [0, 1, 2, 1, 3, 2], [10, 20, 30, 21, 41, 32], [0.5, 2.0, 1.0, 3.0, 1.0, 1.0])


def test_nothing_at_all_and_a_bad_request_pointer():
    empty = block([])
    got = fa.spell_out_candidates(empty, [0], empty)
    same(got, [0], [], [], [])
    ctx, cand = block([[(0, 1, 1.0)]]), block([[(1, 2, 1.0)], []])
    for bad in ([0, 1], [1, 2], [0, 2, 2], [0]):
        with pytest.raises(ValueError):
            fa.spell_out_candidates(ctx, bad, cand)


def test_header_and_binding_carry_the_entry_points():
    header = open(os.path.join(ROOT, "include", "ffm_engine.h")).read()
    assert "#define FFM_ENGINE_ABI_VERSION 4" in header
    assert "Scoring candidates" in header and "ffm.cpp:51-55" in header
    for word in ("field order", "OUT OF SCOPE", "groups, shards, FM and LR", "rows beyond 128 entries"):
        assert word in header, word
    bound = {name: args for name, _, args in fa.ABI}
    assert len(bound["ffm_engine_score_candidates"]) == 14
    assert len(bound["ffm_engine_score_candidates_device"]) == 17
    fa.build()
    lib = fa.load_library()
    assert lib.ffm_engine_score_candidates(None, 0, None, None, None, None, None, 0, None, None, None, None, 0, None) == -1
    assert lib.ffm_engine_score_candidates_device(None, 0, None, None, None, None, None, 0, None, None, None, None,
                                                  0, 0, 0, 0, None) == -1
    assert callable(fa.Engine.score_candidates) and callable(fa.Engine.score_candidates_device)
