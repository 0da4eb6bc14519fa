"""The host side of per-request item lists (include/ffm_engine.h "Scoring a catalogue: per-request item lists"): both
entry points are declared in the header's ABI table, exported by the library, bound on Engine, and refuse a null engine."""
import ftrl_ffm_amd as fa

NAMES = ("ffm_engine_score_item_lists", "ffm_engine_score_item_lists_device")


def test_the_entry_points_are_declared_bound_and_exported():
    lib, declared = fa.load_library(), {name for name, _, _ in fa.ABI}
    for name in NAMES:
        assert name in declared and getattr(lib, name) is not None, name
        assert callable(getattr(fa.Engine, name[len("ffm_engine_"):])), name


def test_a_null_engine_is_refused():
    lib = fa.load_library()
    assert fa.engine.E_INVALID == -1
    assert lib.ffm_engine_score_item_lists(None, 1, None, None, None, None, 1, None, None, None, 1, None, None, 0, None) == -1
    assert lib.ffm_engine_score_item_lists_device(None, 1, None, None, None, None, 1, None, None, None, 1, None, None, 0, 0, 0, 0, 0, None) == -1
