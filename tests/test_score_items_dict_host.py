"""The host side of dictionary slots (include/ffm_engine.h "Scoring a catalogue: dictionary slots"): factor_items and
expand_items are inverses, an out-of-range code expands to an erased id, and the four entry points are bound."""
import numpy as np

import ftrl_ffm_amd as fa

NAMES = ("ffm_engine_score_items_dict", "ffm_engine_score_items_dict_device", "ffm_engine_score_items_dict_topk",
         "ffm_engine_score_items_dict_topk_device")


def test_factor_and_expand_are_inverses():
    rng = np.random.default_rng(3)
    t = np.stack([rng.integers(1000, size=50), 1000 + rng.integers(7, size=50), 2000 + rng.integers(3, size=50)], axis=1).astype(np.int32)
    for g in (1, 2):
        feat, code, dicts = fa.factor_items(t, g)
        assert feat.shape == (50, g) and code.shape == (50, 3 - g) and len(dicts) == 3 - g
        assert all(len(d) == len(np.unique(t[:, g + a])) for a, d in enumerate(dicts))
        assert np.array_equal(fa.expand_items(feat, code, dicts, 5000), t)


def test_a_code_outside_its_dictionary_expands_to_n_feats():
    feat, code, dicts = np.array([[5], [6], [7]], np.int32), np.array([[0], [-1], [2]], np.int32), [np.array([40, 41], np.int32)]
    assert np.array_equal(fa.expand_items(feat, code, dicts, 99), [[5, 40], [6, 99], [7, 99]])


def test_the_entry_points_are_declared_and_exported():
    lib, declared = fa.load_library(), {name for name, _, _ in fa.ABI}
    for name in NAMES:
        assert name in declared and getattr(lib, name) is not None, name
