"""The best K of a catalogue (include/ffm_engine.h "Scoring a catalogue: the best K"), what needs no device: the two
symbols, the C error convention, and catalog_topk_reference's total order spelled out on a hand-written matrix."""
import os

import numpy as np

import ftrl_ffm_amd as fa

NAMES = ("ffm_engine_score_catalog_topk", "ffm_engine_score_catalog_topk_device")


def test_symbols_are_declared_bound_and_exported():
    fa.build()
    lib = fa.load_library()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffm_engine.h")).read()
    bound = {n for n, _, _ in fa.ABI}
    for name in NAMES:
        assert name + "(" in header and name in bound and hasattr(lib, name), name
    assert lib.ffm_engine_score_catalog_topk(None, 0, None, None, None, None, 0, 0, 0, 1.0, 8, 0, None, None) == -1
    assert lib.ffm_engine_score_catalog_topk_device(None, 0, None, None, None, None, 0, 0, 0, 1.0, 8, 0, 0, 0, None, None) == -1
    assert b"null engine" in lib.ffm_engine_last_error()


def test_reference_is_the_total_order_with_ties_to_the_lower_id():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    m = np.array([[-0.0, 2.5, 0.0, 2.5, -inf, inf],
                  [1.0, nan, -3.0, inf, 1.0, -0.0]], np.float32)
    assert m.view(np.uint32)[1, 1] >> 31 == 0  # (the NaN's sign bit is clear: it ranks above +inf)
    s, i = fa.catalog_topk_reference(m, 100, 8)
    assert s.dtype == np.float32 and i.dtype == np.int32 and s.shape == i.shape == (2, 8)
    # +inf; the tie 2.5 to the lower id; +0.0 above -0.0; -inf; then the fill
    assert i[0].tolist() == [105, 101, 103, 102, 100, 104, -1, -1]
    # the NaN above +inf; the tie 1.0 to the lower id
    assert i[1].tolist() == [101, 103, 100, 104, 105, 102, -1, -1]
    want = np.full((2, 8), 0x7FC00000, np.uint32)
    want[0, :6] = m.view(np.uint32)[0, [5, 1, 3, 2, 0, 4]]
    want[1, :6] = m.view(np.uint32)[1, [1, 3, 0, 4, 5, 2]]
    assert np.array_equal(s.view(np.uint32), want)
    s2, i2 = fa.catalog_topk_reference(m, 100, 2)
    assert np.array_equal(i2, i[:, :2]) and np.array_equal(s2.view(np.uint32), want[:, :2])
    s0, i0 = fa.catalog_topk_reference(np.zeros((3, 0), np.float32), 7, 2)
    assert (i0 == -1).all() and (s0.view(np.uint32) == 0x7FC00000).all()
