"""The world-rebuild entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and refuse a
NULL context (the host function: a NULL pointer) with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

from rayaccel_amd import engine

_vp, _u32, _P = engine._vp, engine._u32, engine._P
DECLARED = {
    "racc_hip_world_rebuild_create": [_vp, _vp, _P(_vp)],
    "racc_hip_world_rebuild_device": [_vp, _vp, _vp, _u32, _vp],
    "racc_hip_world_rebuild": [_vp, _vp, _vp, _u32],
    "racc_hip_world_rebuild_check": [_vp, _vp, _P(_u32), _P(_u32)],
    "racc_host_world_rebuild": [_vp, _vp, _u32, _vp, _vp, _P(C.c_float), _vp, _u32, _P(_u32), _vp, _P(_u32)],
}
NULL_CALLS = {
    "racc_hip_world_rebuild_create": (lambda lib: lib.racc_hip_world_rebuild_create(None, None, None), b"world_rebuild_create: ctx is NULL"),
    "racc_hip_world_rebuild_device": (lambda lib: lib.racc_hip_world_rebuild_device(None, None, None, 0, None), b"world_rebuild_device: ctx is NULL"),
    "racc_hip_world_rebuild": (lambda lib: lib.racc_hip_world_rebuild(None, None, None, 0), b"world_rebuild: ctx is NULL"),
    "racc_hip_world_rebuild_check": (lambda lib: lib.racc_hip_world_rebuild_check(None, None, None, None), b"world_rebuild_check: ctx is NULL"),
    "racc_host_world_rebuild": (lambda lib: lib.racc_host_world_rebuild(None, None, 1, None, None, None, None, 1, None, None, None), b"racc_host_world_rebuild: transforms / root boxes pointer is NULL"),
}
# behind a context that is not NULL the handle is looked at before the device is: a NULL handle is refused without a GPU
_CTX = C.c_void_p(1)
NULL_HANDLE_CALLS = {
    "racc_hip_world_rebuild_create": (lambda lib: lib.racc_hip_world_rebuild_create(_CTX, None, C.byref(C.c_void_p())), b"world_rebuild_create: world is NULL"),
    "racc_hip_world_rebuild_device": (lambda lib: lib.racc_hip_world_rebuild_device(_CTX, None, None, 0, None), b"world_rebuild_device: refit/d_transforms12 is NULL"),
    "racc_hip_world_rebuild": (lambda lib: lib.racc_hip_world_rebuild(_CTX, None, None, 0), b"world_rebuild: refit/transforms is NULL"),
    "racc_hip_world_rebuild_check": (lambda lib: lib.racc_hip_world_rebuild_check(_CTX, None, None, None), b"world_rebuild_check: refit/height/disabled_instances is NULL"),
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


@pytest.mark.parametrize("name", sorted(NULL_HANDLE_CALLS))
def test_null_handle_is_refused_before_the_device_is_touched(name):
    lib = engine.load_library()
    call, message = NULL_HANDLE_CALLS[name]
    assert call(lib) == -1
    assert message in lib.racc_hip_last_error()


def test_the_header_no_longer_lists_the_rebuild_as_out_of_scope():
    root = os.path.dirname(engine._HERE)
    assert "a device-side rebuild" not in open(os.path.join(root, "include", "racc_hip.h")).read()
    assert "a device-side rebuild" not in open(os.path.join(root, "DESIGN.md")).read()


def test_python_interface_is_there():
    import rayaccel_amd as ra
    assert callable(ra.host_world_rebuild)
    assert "rebuild" in inspect.signature(engine.World.create_refit).parameters
    for method in ("rebuild", "rebuild_device", "check_rebuild"):
        assert callable(getattr(engine.WorldRefit, method))
