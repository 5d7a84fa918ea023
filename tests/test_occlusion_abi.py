"""The occlusion entries of include/racc_hip.h exist, are bound, and check their context before anything else (no GPU needed)."""
import pytest

from rayaccel_amd import engine

ENTRIES = {
    "racc_hip_occluded_device": lambda lib, count: lib.racc_hip_occluded_device(None, None, None, None, count, None),
    "racc_hip_occluded": lambda lib, count: lib.racc_hip_occluded(None, None, None, None, count),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_symbol_is_exported_and_bound(name):
    assert name in engine.ABI
    lib = engine.load_library()
    assert getattr(lib, name).argtypes == engine.ABI[name][1]


@pytest.mark.parametrize("count", [5, 0])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_null_context_is_refused_first(name, count):
    """count == 0 is a successful no-op only for a real context: the context is checked first."""
    lib = engine.load_library()
    assert ENTRIES[name](lib, count) == -1
    assert b"ctx is NULL" in lib.racc_hip_last_error()
