"""The wide-refit entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and refuse a
NULL context (the host function: a NULL pointer) with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import ctypes as C
import inspect
import os
import re

import pytest

from rayaccel_amd import engine

_vp, _u32, _i, _P = engine._vp, engine._u32, engine._i, engine._P
DECLARED = {
    "racc_hip_refit_create_wide": [_vp, _vp, _vp, _u32, _u32, _P(_vp)],
    "racc_hip_refit_download_wide": [_vp, _vp, _i, _vp, _u32, _P(_u32)],
    "racc_hip_refit_check": [_vp, _vp, _P(_u32)],
    "racc_host_scene_wide_nodes_refit": [_vp, _vp, _u32, _u32, _u32, _i, _vp, _u32, _P(_u32), _P(_u32)],
}
NULL_CALLS = {
    "racc_hip_refit_create_wide": (lambda lib: lib.racc_hip_refit_create_wide(None, None, None, 0, 0, None), b"ctx is NULL"),
    "racc_hip_refit_download_wide": (lambda lib: lib.racc_hip_refit_download_wide(None, None, 45, None, 0, None), b"ctx is NULL"),
    "racc_hip_refit_check": (lambda lib: lib.racc_hip_refit_check(None, None, None), b"ctx is NULL"),
    "racc_host_scene_wide_nodes_refit": (lambda lib: lib.racc_host_scene_wide_nodes_refit(None, None, 1, 1, 2, 45, None, 0, None, None), b"wide_nodes_refit: NULL argument"),
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


def test_host_function_refuses_another_format_and_another_topology(small_host):
    import rayaccel_amd as ra
    h = small_host
    with pytest.raises(ra.RaccError) as e:
        ra.host_wide_refit(h.nodes, h.nodes, len(h.pairs), len(h.remap), 47)
    assert e.value.code == -1 and "format" in str(e.value)
    other = h.nodes.copy()
    other["first"][1], other["last"][1] = h.nodes["last"][1], h.nodes["first"][1]
    assert other["first"][1] != h.nodes["first"][1]
    with pytest.raises(ra.RaccError) as e:
        ra.host_wide_refit(h.nodes, other, len(h.pairs), len(h.remap), 45)
    assert e.value.code == -1 and "child reference" in str(e.value)


def test_options_keep_their_size():
    assert C.sizeof(engine.Options) == 72


def test_python_interface_is_there():
    import rayaccel_amd as ra
    assert callable(ra.host_wide_refit) and ra.host_wide_refit is engine.host_wide_refit
    for method in ("download_wide", "check", "refit", "refit_device", "download", "destroy"):
        assert callable(getattr(engine.Refit, method))
    assert inspect.signature(engine.Context.create_refit).parameters["wide"].default is False
