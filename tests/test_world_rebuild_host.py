"""racc_host_world_rebuild (rayaccel_amd/csrc/world_build.cpp): the host specification of the top-level rebuild on the device — the LBVH
of racc_world_rebuild_rule.h over racc_host_world_prepare's inverses and world boxes.  No GPU needed.

The heights the GPU tests rely on (tests/test_gpu_world_rebuild.py: the chain world on the small scene's root box) are established here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from rayaccel_amd import engine
from test_world_host import random_world
from world_rebuild_helpers import chain_world, common_centre_world, height_bound, numpy_lbvh, walk_height

COUNTS = [1, 2, 3, 64, 65, 1000]
BOX_FIELDS = ("leftMin", "leftMax", "rightMin", "rightMax")
LDS_LEVELS = 8      # kWorldTopLds: the top-level stack levels the world kernels keep in LDS (racc_hip_world_info::lds_levels)


def unit_boxes(n):
    return np.tile(np.float32([-1, -1, -1, 1, 1, 1]), (n, 1))


def assert_is_the_rule(w, t, rb, what):
    """Everything the issue asks of one output: topology and order against the numpy restatement, the per-instance part against prepare,
    the boxes against a refit of the output itself, the structure, the height."""
    n = len(t)
    prepared = ra.host_world_prepare(t, rb)
    assert w["inv"].tobytes() == prepared["inv"].tobytes() and w["world_boxes"].tobytes() == prepared["world_boxes"].tobytes(), what
    assert np.float32(w["ray_pad"]).tobytes() == np.float32(prepared["ray_pad"]).tobytes(), what
    first, last, order = numpy_lbvh(prepared["world_boxes"])
    assert len(w["nodes"]) == max(n - 1, 1), what
    assert np.array_equal(w["order"], order), "%s: order differs from the numpy restatement" % what
    assert np.array_equal(w["nodes"]["first"], first) and np.array_equal(w["nodes"]["last"], last), "%s: topology differs from the numpy restatement" % what
    assert sorted(w["order"].tolist()) == list(range(n)), what
    height = walk_height(w["nodes"]["first"], w["nodes"]["last"], n)      # (also: every record reached once, every position named once)
    assert w["height"] == height, "%s: reported height %d, a walk finds %d" % (what, w["height"], height)
    assert height <= height_bound(n), "%s: height %d above the bound %d" % (what, height, height_bound(n))
    refit = ra.host_world_refit(t, rb, w["nodes"], w["order"])
    for f in BOX_FIELDS:
        assert refit["nodes"][f].tobytes() == w["nodes"][f].tobytes(), "%s: %s is not racc_host_world_refit's fold" % (what, f)
    return height


@pytest.mark.parametrize("count", COUNTS)
def test_random_worlds(count):
    t, rb = random_world(count, 1100 + count)
    w = ra.host_world_rebuild(t, rb)
    assert_is_the_rule(w, t, rb, "%d instances" % count)
    again = ra.host_world_rebuild(t.copy(), rb.copy())
    for k in ("inv", "world_boxes", "nodes", "order"):
        assert w[k].tobytes() == again[k].tobytes(), "two calls differ in %s" % k
    assert w["ray_pad"] == again["ray_pad"] and w["height"] == again["height"]
    if count == 1:      # as racc_host_world_prepare makes it
        assert w["nodes"].tobytes() == ra.host_world_prepare(t, rb)["nodes"].tobytes()


def test_identical_instances_are_ordered_by_index():
    t, rb = random_world(500, 9)
    t[10:20] = t[10]; rb[10:20] = rb[10]
    w = ra.host_world_rebuild(t, rb)
    assert_is_the_rule(w, t, rb, "ten identical instances among 500")
    at = [int(np.nonzero(w["order"] == i)[0][0]) for i in range(10, 20)]
    assert at == list(range(at[0], at[0] + 10)), "equal Morton fields: the index decides"


def test_common_centre_the_index_bits_alone_decide():
    t = common_centre_world(1000)
    w = ra.host_world_rebuild(t, unit_boxes(1000))
    height = assert_is_the_rule(w, t, unit_boxes(1000), "1000 instances with one centre")
    assert np.array_equal(w["order"], np.arange(1000))
    assert height == 10, "ceil(log2 1000) levels of index bits, found %d" % height


def test_morton_chain_is_deeper_than_the_lds_stack(small_host):
    """31 centres at L * 2^-k on one axis: ten field bits cut one instance off each, the index bits share out the rest.  The same world
    on the small scene's root box is what tests/test_gpu_world_rebuild.py traces: its height is established here."""
    for rb, what in ((unit_boxes(31), "unit boxes"), (np.tile(ra.root_box(small_host.nodes), (31, 1)), "the small scene's root box")):
        t = chain_world(4096.0)
        w = ra.host_world_rebuild(t, rb)
        height = assert_is_the_rule(w, t, rb, "chain, " + what)
        print("chain world on %s: height %d (bound %d)" % (what, height, height_bound(31)))
        assert height > LDS_LEVELS + 1, "the chain must spill the top-level stack: height %d" % height


def test_chain_with_a_crowd_at_its_end():
    t = chain_world(4096.0, extra_at_the_end=200)
    w = ra.host_world_rebuild(t, unit_boxes(len(t)))
    height = assert_is_the_rule(w, t, unit_boxes(len(t)), "chain of 31 with 200 more on its last instance")
    print("chain + crowd: height %d (bound %d)" % (height, height_bound(len(t))))
    assert height > 10 + 7, "ten levels of field bits above at least ceil(log2 201) - 1 levels of index bits, found %d" % height


def test_refusals_are_prepares_and_name_the_entry():
    t, rb = random_world(3, 1)
    assert len(ra.host_world_rebuild(t, rb)["nodes"]) == 2

    def refused(tt, bb, text):
        with pytest.raises(ra.RaccError) as e:
            ra.host_world_rebuild(tt, bb)
        assert e.value.code == -1 and text in str(e.value) and "racc_host_world_rebuild" in str(e.value), str(e.value)
        with pytest.raises(ra.RaccError) as p:
            ra.host_world_prepare(tt, bb)
        assert str(p.value).replace("racc_host_world_prepare", "racc_host_world_rebuild") == str(e.value), "prepare refuses differently"

    for bad in (np.nan, np.inf, -np.inf):
        tt = t.copy(); tt[1, 2, 3] = bad
        refused(tt, rb, "not finite")
    tt = t.copy(); tt[2, :, :3] = 0
    refused(tt, rb, "singular")
    tt = t.copy(); tt[0, :, :3] = [[1, 2, 3], [1, 2, 3], [4, 5, 6]]
    refused(tt, rb, "singular")
    tt = t.copy(); tt[0, :, :3] = np.float32(3e38) * np.eye(3, dtype=np.float32)
    refused(tt, rb, "not finite")
    bb = rb.copy(); bb[1, 0] = np.nan
    refused(t, bb, "not finite")
    bb = rb.copy(); bb[1, 0], bb[1, 3] = 2, 1
    refused(t, bb, "min > max")
    refused(np.zeros((0, 3, 4), np.float32), np.zeros((0, 6), np.float32), "count is 0")

    # the raw entry: NULL pointers, too many instances, too little room — and nothing written
    lib, p = engine.load_library(), engine._ptr
    tt = np.ascontiguousarray(t.reshape(3, 12))
    inv, boxes, nodes, order = np.full((3, 12), -7, np.float32), np.full((3, 6), -7, np.float32), np.zeros(2, engine.GPU_NODE_DTYPE), np.full(3, 77, np.uint32)
    pad, nn, height = C.c_float(-7), C.c_uint32(77), C.c_uint32(77)

    def raw(text, t=tt, rb=rb, n=3, cap=2, null=None):
        a = dict(t=p(t), rb=p(rb), inv=p(inv), boxes=p(boxes), pad=C.byref(pad), nodes=p(nodes), nn=C.byref(nn), order=p(order), height=C.byref(height))
        if null:
            a[null] = None
        rc = lib.racc_host_world_rebuild(a["t"], a["rb"], n, a["inv"], a["boxes"], a["pad"], a["nodes"], cap, a["nn"], a["order"], a["height"])
        msg = lib.racc_hip_last_error().decode()
        assert rc == -1 and "racc_host_world_rebuild" in msg and text in msg, (rc, msg)
        assert (inv == -7).all() and (boxes == -7).all() and pad.value == -7 and nn.value == 77 and height.value == 77 and (order == 77).all() and not nodes.tobytes().strip(b"\0")

    for null in ("t", "rb", "inv", "boxes", "pad", "nodes", "nn", "order", "height"):
        raw("NULL", null=null)
    raw("2^20", n=(1 << 20) + 1)
    raw("node_capacity", cap=1)
    bad = tt.copy(); bad[2, 5] = np.nan
    raw("not finite", t=bad)


def test_stand_alone_driver_under_asan_and_ubsan():
    """tests/cpp/world_rebuild_host_check.cpp: racc_host_world_rebuild on random, common-centre and chain worlds and its refusals, built
    with the Makefile's AddressSanitizer + UBSan flags and run as a program of its own."""
    subprocess.check_call(["make", "-s", "-C", engine.CSRC, "../../tests/cpp/world_rebuild_host_check"])
    exe = os.path.join(os.path.dirname(engine._HERE), "tests", "cpp", "world_rebuild_host_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "rebuilds checked, 0 failures" in out.stdout
