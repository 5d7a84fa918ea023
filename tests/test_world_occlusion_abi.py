"""The world occlusion entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and
refuse a NULL context with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import os
import re

import pytest

from rayaccel_amd import engine

_vp, _u32 = engine._vp, engine._u32
DECLARED = {
    "racc_hip_world_occluded_device": [_vp, _vp, _vp, _vp, _u32, _vp],
    "racc_hip_world_occluded": [_vp, _vp, _vp, _vp, _u32],
}
NULL_CALLS = {
    "racc_hip_world_occluded_device": lambda lib, count: lib.racc_hip_world_occluded_device(None, None, None, None, count, None),
    "racc_hip_world_occluded": lambda lib, count: lib.racc_hip_world_occluded(None, None, None, None, count),
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_exported_bound_and_declared(name):
    assert name in engine.ABI
    lib = engine.load_library()
    assert getattr(lib, name).argtypes == DECLARED[name] == engine.ABI[name][1]
    assert getattr(lib, name).restype is engine._i
    header = open(os.path.join(os.path.dirname(engine._HERE), "include", "racc_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/racc_hip.h" % name
    assert "an instanced occlusion query" not in header, "the header still lists the instanced occlusion query as out of scope"


@pytest.mark.parametrize("count", [5, 0])
@pytest.mark.parametrize("name", sorted(NULL_CALLS))
def test_null_context_is_refused_first(name, count):
    """count == 0 is a successful no-op only for a real context and world: the context is checked first."""
    lib = engine.load_library()
    assert NULL_CALLS[name](lib, count) == -1
    assert b"ctx is NULL" in lib.racc_hip_last_error()


def test_python_interface_is_there():
    for method in ("occluded", "occluded_device"):
        assert callable(getattr(engine.World, method))
