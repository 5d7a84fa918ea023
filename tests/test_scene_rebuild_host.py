"""racc_host_scene_rebuild (rayaccel_amd/csrc/scene_rebuild.cpp): the host specification of the bottom-level rebuild on the device — the
LBVH of racc_scene_rebuild_rule.h over the triangles of a mesh, one triangle per pair, one pair per leaf.  No GPU needed.

Held byte for byte to a third formulation (tests/scene_rebuild_helpers.py: numpy fields, Python's sort of (field, index) tuples, Karras's
per-node searches); its output refits to itself, is a blob the upload accepts, and traces like the brute force.  The heights the GPU tests
rely on (tests/test_gpu_scene_rebuild.py) are established here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from helpers import MISS, assert_matches_arbiter
from oracle import oracle as orc
from rayaccel_amd import engine
from scene_rebuild_helpers import (NODE_FIELDS, chain, common_centre, duplicated, height_bound, numpy_lbvh, on_one_axis, padded_pairs, rays_at,
                                   soup)

LDS_LEVELS = 13      # the deepest LDS stack of any traversal kernel that takes a binary scene (the default closest-hit kernel: 12 entries + 1)


def shapes():
    out = [("T=%d" % t, soup(t, 500 + t)) for t in (2, 3, 4, 5, 31, 32, 33, 1000)]
    return out + [("all-ties", common_centre(1000)), ("one-axis", on_one_axis(300, 3)), ("duplicated", duplicated(400, 4)), ("chain", chain())]


SHAPES = shapes()


def assert_is_the_rule(blobs, v, idx, what):
    t = idx.size // 3
    want = numpy_lbvh(v, idx)
    assert len(blobs["nodes"]) == t - 1 and len(blobs["pairs"]) == padded_pairs(t) and len(blobs["remap"]) == 2 * t, what
    assert np.array_equal(blobs["remap"], want["remap"]), "%s: remap (the order) differs from the numpy formulation" % what
    for f in NODE_FIELDS:
        assert blobs["nodes"][f].tobytes() == want["nodes"][f].tobytes(), "%s: nodes.%s differs from the numpy formulation" % (what, f)
    assert blobs["pairs"].tobytes() == want["pairs"].tobytes(), "%s: pairs differ from the numpy formulation" % what
    assert blobs["height"] == want["height"] <= height_bound(t), "%s: height %d, numpy %d, bound %d" % (what, blobs["height"], want["height"], height_bound(t))
    return want


@pytest.mark.parametrize("name,mesh", SHAPES, ids=[s[0] for s in SHAPES])
def test_the_host_function_is_the_rule_and_a_scene(name, mesh):
    v, idx = mesh
    t = idx.size // 3
    blobs = ra.host_scene_rebuild(v, idx)
    assert_is_the_rule(blobs, v, idx, name)
    again = ra.host_scene_rebuild(v.copy(), idx.copy())
    assert all(blobs[k].tobytes() == again[k].tobytes() for k in ("nodes", "pairs", "remap")), "two calls differ"
    # a refit of the output to its own vertices is the identity
    refit = ra.host_refit(blobs, v, idx)
    assert refit["nodes"].tobytes() == blobs["nodes"].tobytes() and refit["pairs"].tobytes() == blobs["pairs"].tobytes(), "%s: host_refit is not the identity" % name
    # the upload's validation and re-layout accept the blob
    lib, n = engine.load_library(), C.c_uint32(0)
    assert lib.racc_host_scene_device_nodes(engine._ptr(blobs["nodes"]), t - 1, len(blobs["pairs"]), len(blobs["remap"]), 1, None, 0, C.byref(n)) == 0, lib.racc_hip_last_error()
    assert n.value >= t - 1
    # the oracle's traversal of the blob against the brute-force arbiter
    rays = rays_at(v, idx, 3000, 77)
    res = orc.traverse(blobs, rays)
    assert (res["triangle"] != MISS).mean() > 0.2, "%s: rays must hit for the test to mean anything" % name
    assert_matches_arbiter(res, dict(vertices=v, indices=idx), rays)


def test_all_ties_the_index_alone_decides():
    v, idx = common_centre(1000)
    blobs = ra.host_scene_rebuild(v, idx)
    assert np.array_equal(blobs["remap"][0::2], np.arange(1000)), "equal fields: the order is the index order"
    assert blobs["height"] == 10, "ceil(log2 1000) levels of index bits, found %d" % blobs["height"]


def test_one_axis_leaves_two_axes_without_extent():
    v, idx = on_one_axis(300, 3)
    blobs = ra.host_scene_rebuild(v, idx)
    x = v.reshape(-1, 3, 3)[:, 0, 0]
    assert np.array_equal(blobs["remap"][0::2], np.lexsort((np.arange(300), x))), "hi == lo on y and z: x alone orders the triangles"


def test_chain_is_deeper_than_every_lds_stack():
    """Centres at 2^-k, k = 0 .. 39: under the 21-bit field the first 21 bits of x cut one triangle off each, the triangles of the last
    cell are shared out by their index bits.  tests/test_gpu_scene_rebuild.py traces this mesh through the spilled stack."""
    v, idx = chain()
    blobs = ra.host_scene_rebuild(v, idx)
    want = numpy_lbvh(v, idx)
    print("chain of 40: height %d (bound %d)" % (want["height"], height_bound(40)))
    assert blobs["height"] == want["height"]
    assert want["height"] > LDS_LEVELS, "the chain must spill every kernel's stack: height %d" % want["height"]


def test_refusals_leave_the_outputs_untouched():
    lib, p = engine.load_library(), engine._ptr
    v3, idx = soup(5, 1)
    v = engine._as_verts4(v3)
    nodes, pairs, remap = np.zeros(4, engine.GPU_NODE_DTYPE), np.zeros(32, engine.PAIR_DTYPE), np.full(10, 77, np.uint32)
    nn, npairs, nremap, height = C.c_uint32(77), C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)

    def raw(code, text, v=v, nv=len(v), idx=idx, ni=idx.size, node_cap=4, pair_cap=32, remap_cap=10, null=None):
        a = dict(v=p(v), idx=p(idx), nodes=p(nodes), nn=C.byref(nn), pairs=p(pairs), npairs=C.byref(npairs), remap=p(remap), nremap=C.byref(nremap), height=C.byref(height))
        if null:
            a[null] = None
        rc = lib.racc_host_scene_rebuild(a["v"], nv, a["idx"], ni, a["nodes"], node_cap, a["nn"], a["pairs"], pair_cap, a["npairs"], a["remap"], remap_cap, a["nremap"], a["height"])
        msg = lib.racc_hip_last_error().decode()
        assert rc == code and "racc_host_scene_rebuild" in msg and text in msg, (rc, msg)
        assert not nodes.tobytes().strip(b"\0") and not pairs.tobytes().strip(b"\0") and (remap == 77).all(), "an output was written"
        assert nn.value == npairs.value == nremap.value == height.value == 77, "a count was written"

    for null in ("v", "idx", "nodes", "nn", "pairs", "npairs", "remap", "nremap", "height"):
        raw(-1, "NULL", null=null)
    raw(-1, "multiple of 3", ni=14)
    raw(-1, "fewer than 2 triangles", ni=3)
    raw(-1, "fewer than 2 triangles", ni=0)
    bad = idx.copy(); bad[7] = len(v)
    raw(-1, "not below vertex_count", idx=bad)
    for value in (np.nan, np.inf, -np.inf):
        vv = v.copy(); vv[4, 1] = value
        raw(-1, "not finite", v=vv)
    raw(-1, "node_capacity", node_cap=3)
    raw(-1, "pair_capacity", pair_cap=31)
    raw(-1, "remap_capacity", remap_cap=9)
    # 2^24 triangles: the limit of the format (the indices are never read: the count is refused first)
    huge = np.zeros(3, np.uint32)
    raw(-4, "2^24", idx=huge, ni=3 << 24)
    # ... and the function works with exactly the room it asks for
    assert lib.racc_host_scene_rebuild(p(v), len(v), p(idx), idx.size, p(nodes), 4, C.byref(nn), p(pairs), 32, C.byref(npairs), p(remap), 10, C.byref(nremap), C.byref(height)) == 0
    assert (nn.value, npairs.value, nremap.value) == (4, 32, 10) and 2 <= height.value <= 4


def test_stand_alone_driver_under_asan_and_ubsan():
    """tests/cpp/scene_rebuild_host_check.cpp: racc_host_scene_rebuild on the shapes above, the field function on every special value, and
    the rule header's hierarchy step over sorted, all-equal, reversed and random keys through bounds-checked accessors — built with the
    Makefile's AddressSanitizer + UBSan flags and run as a program of its own."""
    subprocess.check_call(["make", "-s", "-C", engine.CSRC, "../../tests/cpp/scene_rebuild_host_check"])
    exe = os.path.join(os.path.dirname(engine._HERE), "tests", "cpp", "scene_rebuild_host_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "checks passed, 0 failures" in out.stdout
