"""The world-refit entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and refuse a
NULL context (the host function: a NULL pointer) with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from rayaccel_amd import engine

_vp, _u32, _P = engine._vp, engine._u32, engine._P
DECLARED = {
    "racc_hip_world_refit_create": [_vp, _vp, _P(_vp)],
    "racc_hip_world_refit_destroy": [_vp, _vp],
    "racc_hip_world_refit_device": [_vp, _vp, _vp, _u32, _vp],
    "racc_hip_world_refit": [_vp, _vp, _vp, _u32],
    "racc_hip_world_refit_check": [_vp, _vp, _P(_u32)],
    "racc_hip_world_download": [_vp, _vp, _vp, _vp, _u32, _vp, _P(C.c_float)],
    "racc_host_world_refit": [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _P(C.c_float), _vp],
}
NULL_CALLS = {
    "racc_hip_world_refit_create": (lambda lib: lib.racc_hip_world_refit_create(None, None, None), b"ctx is NULL"),
    "racc_hip_world_refit_destroy": (lambda lib: lib.racc_hip_world_refit_destroy(None, None), b"ctx is NULL"),
    "racc_hip_world_refit_device": (lambda lib: lib.racc_hip_world_refit_device(None, None, None, 0, None), b"ctx is NULL"),
    "racc_hip_world_refit": (lambda lib: lib.racc_hip_world_refit(None, None, None, 0), b"ctx is NULL"),
    "racc_hip_world_refit_check": (lambda lib: lib.racc_hip_world_refit_check(None, None, None), b"ctx is NULL"),
    "racc_hip_world_download": (lambda lib: lib.racc_hip_world_download(None, None, None, None, 0, None, None), b"ctx is NULL"),
    "racc_host_world_refit": (lambda lib: lib.racc_host_world_refit(None, None, 1, None, 1, None, None, None, None, None), b"racc_host_world_refit: transforms / root boxes pointer is NULL"),
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_exported_bound_and_declared(name):
    assert name in engine.ABI
    lib = engine.load_library()
    assert getattr(lib, name).argtypes == DECLARED[name] == engine.ABI[name][1]
    assert getattr(lib, name).restype is engine._i
    header = open(os.path.join(os.path.dirname(engine._HERE), "include", "racc_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, header), "%s is not declared in include/racc_hip.h" % name


@pytest.mark.parametrize("name", sorted(NULL_CALLS))
def test_null_is_refused_first(name):
    lib = engine.load_library()
    call, message = NULL_CALLS[name]
    assert call(lib) == -1
    assert message in lib.racc_hip_last_error()


def test_python_interface_is_there():
    import rayaccel_amd as ra
    assert callable(ra.host_world_refit) and ra.WorldRefit is engine.WorldRefit
    for method in ("create_refit", "download"):
        assert callable(getattr(engine.World, method))
    for method in ("refit", "refit_device", "check", "destroy"):
        assert callable(getattr(engine.WorldRefit, method))
