"""The instancing entries of include/racc_hip.h exist, are declared in the header, are bound with the declared argument types, and refuse
NULL and a bad count with -1 (RACC_HIP_ERR_INVALID) and a message before anything else (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rayaccel_amd import engine

_vp, _u32, _P = engine._vp, engine._u32, engine._P
DECLARED = {
    "racc_hip_world_create": [_vp, _vp, _P(_vp), _u32, _P(_vp)],
    "racc_hip_world_update": [_vp, _vp, _vp, _u32],
    "racc_hip_world_destroy": [_vp, _vp],
    "racc_hip_world_get_info": [_vp, _P(engine.WorldInfo)],
    "racc_hip_world_intersect_device": [_vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "racc_hip_world_intersect": [_vp, _vp, _vp, _vp, _vp, _u32],
    "racc_host_world_prepare": [_vp, _vp, _u32, _vp, _vp, _P(C.c_float), _vp, _u32, _P(_u32), _vp, _P(_u32)],
}
NULL_CALLS = {
    "racc_hip_world_create": (lambda lib: lib.racc_hip_world_create(None, None, None, 0, None), b"ctx is NULL"),
    "racc_hip_world_update": (lambda lib: lib.racc_hip_world_update(None, None, None, 0), b"ctx is NULL"),
    "racc_hip_world_destroy": (lambda lib: lib.racc_hip_world_destroy(None, None), b"ctx is NULL"),
    "racc_hip_world_get_info": (lambda lib: lib.racc_hip_world_get_info(None, None), b"world/info is NULL"),
    "racc_hip_world_intersect_device": (lambda lib: lib.racc_hip_world_intersect_device(None, None, None, None, None, 0, None), b"ctx is NULL"),
    "racc_hip_world_intersect": (lambda lib: lib.racc_hip_world_intersect(None, None, None, None, None, 0), b"ctx is NULL"),
    "racc_host_world_prepare": (lambda lib: lib.racc_host_world_prepare(None, None, 1, None, None, None, None, 0, None, None, None), b"pointer is NULL"),
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


def _prepare_raw(count, capacity=None, t=None):
    """racc_host_world_prepare with real arrays for `alloc` instances and `count` passed as the count."""
    alloc = 2
    t = np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (alloc, 1)) if t is None else t
    rb = np.tile(np.array([0, 0, 0, 1, 1, 1], np.float32), (alloc, 1))
    inv, boxes, nodes, order = np.zeros((alloc, 12), np.float32), np.zeros((alloc, 6), np.float32), np.zeros(alloc, engine.GPU_NODE_DTYPE), np.zeros(alloc, np.uint32)
    pad, nn, h = C.c_float(0), C.c_uint32(0), C.c_uint32(0)
    rc = engine.load_library().racc_host_world_prepare(engine._ptr(t), engine._ptr(rb), count, engine._ptr(inv), engine._ptr(boxes), C.byref(pad),
                                                       engine._ptr(nodes), alloc if capacity is None else capacity, C.byref(nn), engine._ptr(order), C.byref(h))
    return rc, engine.load_library().racc_hip_last_error()


def test_host_prepare_refuses_a_bad_count():
    assert _prepare_raw(2)[0] == 0
    rc, msg = _prepare_raw(0)
    assert rc == -1 and b"count is 0" in msg
    rc, msg = _prepare_raw((1 << 20) + 1)      # (refused before any array is read)
    assert rc == -1 and b"2^20" in msg
    rc, msg = _prepare_raw(2, capacity=0)
    assert rc == -1 and b"node_capacity" in msg


def test_limits_agree_with_the_header():
    header = open(os.path.join(os.path.dirname(engine._HERE), "include", "racc_hip.h")).read()
    assert re.search(r"#define RACC_HIP_WORLD_MAX_INSTANCES \(1u << 20\)", header) and engine.WORLD_MAX_INSTANCES == 1 << 20
    assert C.sizeof(engine.WorldInfo) == 32


def test_python_interface_is_there():
    import rayaccel_amd as ra
    assert callable(ra.host_world_prepare) and callable(engine.Context.create_world) and ra.World is engine.World and ra.NO_INSTANCE == 0xFFFFFFFF
    for method in ("intersect", "intersect_device", "update", "destroy"):
        assert callable(getattr(engine.World, method))
    assert isinstance(engine.World.info, property)
