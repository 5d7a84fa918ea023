"""The scene-rebuild entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and refuse a
NULL context (the host function: a NULL pointer) with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from rayaccel_amd import engine

_vp, _u32, _P = engine._vp, engine._u32, engine._P
DECLARED = {
    "racc_hip_scene_rebuild_create": [_vp, _vp, _u32, _vp, _u32, _P(_vp), _P(_vp)],
    "racc_hip_scene_rebuild_device": [_vp, _vp, _vp, _u32, _vp],
    "racc_hip_scene_rebuild": [_vp, _vp, _vp, _u32],
    "racc_hip_scene_rebuild_check": [_vp, _vp, _P(_u32)],
    "racc_hip_refit_download_remap": [_vp, _vp, _vp, _u32],
    "racc_host_scene_rebuild": [_vp, _u32, _vp, _u32, _vp, _u32, _P(_u32), _vp, _u32, _P(_u32), _vp, _u32, _P(_u32), _P(_u32)],
}
NULL_CALLS = {
    "racc_hip_scene_rebuild_create": (lambda lib: lib.racc_hip_scene_rebuild_create(None, None, 0, None, 0, None, None), b"scene_rebuild_create: ctx is NULL"),
    "racc_hip_scene_rebuild_device": (lambda lib: lib.racc_hip_scene_rebuild_device(None, None, None, 0, None), b"scene_rebuild_device: ctx is NULL"),
    "racc_hip_scene_rebuild": (lambda lib: lib.racc_hip_scene_rebuild(None, None, None, 0), b"scene_rebuild: ctx is NULL"),
    "racc_hip_scene_rebuild_check": (lambda lib: lib.racc_hip_scene_rebuild_check(None, None, None), b"scene_rebuild_check: ctx is NULL"),
    "racc_hip_refit_download_remap": (lambda lib: lib.racc_hip_refit_download_remap(None, None, None, 0), b"refit_download_remap: ctx is NULL"),
    "racc_host_scene_rebuild": (lambda lib: lib.racc_host_scene_rebuild(None, 0, None, 6, None, 1, None, None, 32, None, None, 4, None, None), b"racc_host_scene_rebuild: vertices / indices pointer is NULL"),
}
# behind a context that is not NULL the handle is looked at before the device is: a NULL handle is refused without a GPU
_CTX = C.c_void_p(1)
NULL_HANDLE_CALLS = {
    "racc_hip_scene_rebuild_create": (lambda lib: lib.racc_hip_scene_rebuild_create(_CTX, None, 0, None, 0, None, None), b"scene_rebuild_create: scene_out/out is NULL"),
    "racc_hip_scene_rebuild_device": (lambda lib: lib.racc_hip_scene_rebuild_device(_CTX, None, None, 0, None), b"scene_rebuild_device: refit/d_vertices is NULL"),
    "racc_hip_scene_rebuild": (lambda lib: lib.racc_hip_scene_rebuild(_CTX, None, None, 0), b"scene_rebuild: refit/vertices is NULL"),
    "racc_hip_scene_rebuild_check": (lambda lib: lib.racc_hip_scene_rebuild_check(_CTX, None, None), b"scene_rebuild_check: refit/height is NULL"),
    "racc_hip_refit_download_remap": (lambda lib: lib.racc_hip_refit_download_remap(_CTX, None, None, 0), b"refit_download_remap: refit/remap_out is NULL"),
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


def test_create_hands_back_no_handle_when_it_refuses():
    lib = engine.load_library()
    scene, handle = C.c_void_p(5), C.c_void_p(5)
    assert lib.racc_hip_scene_rebuild_create(_CTX, None, 0, None, 0, C.byref(scene), C.byref(handle)) == -1
    assert b"scene_rebuild_create: vertices/indices is NULL" in lib.racc_hip_last_error()
    assert scene.value is None and handle.value is None


def test_the_refit_section_of_the_header_points_at_the_rebuild():
    header = open(os.path.join(os.path.dirname(engine._HERE), "include", "racc_hip.h")).read()
    assert "build and rebuild of a scene's tree on the device" in header
    assert "every GPU API's BVH update are the usual counterparts." not in header, "the sentence was to be reworded to point at the new section"


def test_python_interface_is_there():
    import rayaccel_amd as ra
    assert callable(ra.host_scene_rebuild) and callable(engine.Context.create_dynamic_scene)
    for method in ("rebuild", "rebuild_device", "check_rebuild"):
        assert callable(getattr(engine.Refit, method))
