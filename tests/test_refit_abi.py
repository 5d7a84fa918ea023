"""The refit entries of include/racc_hip.h exist, are bound with the declared argument types, and refuse a NULL context — the host
function a NULL blob — with -1 and a message before anything else (no GPU needed)."""
import pytest

from rayaccel_amd import engine

_vp, _u32 = engine._vp, engine._u32
DECLARED = {
    "racc_hip_refit_create": [_vp, _vp, _vp, _u32, _u32, engine._P(_vp)],
    "racc_hip_refit_destroy": [_vp, _vp],
    "racc_hip_scene_refit": [_vp, _vp, _vp, _u32],
    "racc_hip_scene_refit_device": [_vp, _vp, _vp, _u32, _vp],
    "racc_hip_refit_download": [_vp, _vp, _vp, _u32, _vp, _u32],
    "racc_host_blobs_refit": [_vp, _u32, _vp, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp],
}
NULL_CALLS = {
    "racc_hip_refit_create": (lambda lib: lib.racc_hip_refit_create(None, None, None, 0, 0, None), b"ctx is NULL"),
    "racc_hip_refit_destroy": (lambda lib: lib.racc_hip_refit_destroy(None, None), b"ctx is NULL"),
    "racc_hip_scene_refit": (lambda lib: lib.racc_hip_scene_refit(None, None, None, 0), b"ctx is NULL"),
    "racc_hip_scene_refit_device": (lambda lib: lib.racc_hip_scene_refit_device(None, None, None, 0, None), b"ctx is NULL"),
    "racc_hip_refit_download": (lambda lib: lib.racc_hip_refit_download(None, None, None, 0, None, 0), b"ctx is NULL"),
    "racc_host_blobs_refit": (lambda lib: lib.racc_host_blobs_refit(None, 0, None, 0, 0, None, 0, None, 0, None, 0, None, None), b"blob pointer is NULL"),
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbol_is_exported_and_bound(name):
    assert name in engine.ABI
    lib = engine.load_library()
    assert getattr(lib, name).argtypes == DECLARED[name] == engine.ABI[name][1]
    assert getattr(lib, name).restype is engine._i


@pytest.mark.parametrize("name", sorted(NULL_CALLS))
def test_null_is_refused_first(name):
    lib = engine.load_library()
    call, message = NULL_CALLS[name]
    assert call(lib) == -1
    assert message in lib.racc_hip_last_error()


def test_python_interface_is_there():
    assert callable(engine.host_refit) and callable(engine.Context.create_refit)
    for method in ("refit", "refit_device", "download", "destroy"):
        assert callable(getattr(engine.Refit, method))
