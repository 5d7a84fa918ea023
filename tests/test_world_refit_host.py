"""racc_host_world_refit (rayaccel_amd/csrc/world_build.cpp): the host specification of the top-level refit — the tree's topology kept,
inverses / world boxes / ray pad as racc_host_world_prepare computes them, child boxes propagated bottom-up.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from rayaccel_amd import engine
from test_world_host import random_world
from world_helpers import affine, rotation

BOX_FIELDS = ("leftMin", "leftMax", "rightMin", "rightMax")


def moved_world(n, seed):
    """n transforms of the issue's ranges — rotations, non-uniform scales up to 1e3, translations up to 1e5 — for random_world's boxes."""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        scale = 10.0 ** rng.uniform(-1, 3, 3) * rng.choice([-1.0, 1.0], 3)
        t[i] = affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), scale, rng.uniform(-1e5, 1e5, 3))
    return t


def below(nodes, order, boxes, ref):
    """The independent restatement: NumPy min / max over the world boxes of every instance below `ref`, by a recursive walk."""
    if ref & 0x80000000:
        n = nodes[ref & 0x7FFFFFFF]
        parts = [below(nodes, order, boxes, int(n["first"])), below(nodes, order, boxes, int(n["last"]))]
        parts = [p for p in parts if p is not None]
        return np.min([p[0] for p in parts], 0), np.max([p[1] for p in parts], 0)
    if ref >> 24 == 0:
        return None
    b = boxes[order[ref & 0xFFFFFF]]
    return b[:3], b[3:]


def assert_boxes_are_the_union_of_what_is_below(out):
    nodes, order, boxes = out["nodes"], out["order"], out["world_boxes"]
    for i, n in enumerate(nodes):
        for ref, lo, hi in ((int(n["first"]), "leftMin", "leftMax"), (int(n["last"]), "rightMin", "rightMax")):
            want = below(nodes, order, boxes, ref)
            if want is not None:
                assert np.array_equal(n[lo], want[0]) and np.array_equal(n[hi], want[1]), "node %d, child %#x" % (i, ref)


@pytest.mark.parametrize("count", [1, 2, 3, 65, 1000])
def test_refit_at_prepares_own_transforms_reproduces_it(count):
    t, rb = random_world(count, 300 + count)
    w = ra.host_world_prepare(t, rb)
    out = ra.host_world_refit(t, rb, w["nodes"], w["order"])
    assert out["inv"].tobytes() == w["inv"].tobytes() and out["world_boxes"].tobytes() == w["world_boxes"].tobytes()
    assert np.float32(out["ray_pad"]).tobytes() == np.float32(w["ray_pad"]).tobytes()
    for f in ("kind", "parent", "first", "last"):
        assert np.array_equal(out["nodes"][f], w["nodes"][f]), f
    for f in BOX_FIELDS:      # numerically: a zero plane's sign may differ (prepare folds over instances, the refit over the tree)
        assert np.array_equal(out["nodes"][f], w["nodes"][f]), f


@pytest.mark.parametrize("count", [1, 2, 3, 65, 1000])
def test_refit_to_moved_transforms(count):
    t, rb = random_world(count, 300 + count)
    w = ra.host_world_prepare(t, rb)
    moved = moved_world(count, 500 + count)
    fresh = ra.host_world_prepare(moved, rb)
    out = ra.host_world_refit(moved, rb, w["nodes"], w["order"])
    assert out["inv"].tobytes() == fresh["inv"].tobytes() and out["world_boxes"].tobytes() == fresh["world_boxes"].tobytes()
    assert np.float32(out["ray_pad"]).tobytes() == np.float32(fresh["ray_pad"]).tobytes()
    for f in ("kind", "parent", "first", "last"):
        assert np.array_equal(out["nodes"][f], w["nodes"][f]), f
    assert_boxes_are_the_union_of_what_is_below(out)
    if count == 1:      # the empty reference's box is copied from the input
        assert out["nodes"]["rightMin"].tobytes() == w["nodes"]["rightMin"].tobytes() and out["nodes"]["rightMax"].tobytes() == w["nodes"]["rightMax"].tobytes()
    # ... and a second refit, from the refitted tree back to the first transforms, gives the tree prepare made
    back = ra.host_world_refit(t, rb, out["nodes"], out["order"])
    for f in BOX_FIELDS:
        assert np.array_equal(back["nodes"][f], w["nodes"][f]), f


def _raw(t, rb, n, nodes, node_count, order, inv, boxes, pad, out_nodes):
    lib = engine.load_library()
    p = engine._ptr
    rc = lib.racc_host_world_refit(p(t), p(rb), n, p(nodes), node_count, p(order), p(inv), p(boxes), None if pad is None else C.byref(pad), p(out_nodes))
    return rc, lib.racc_hip_last_error().decode()


def test_outputs_may_alias_inputs():
    t, rb = random_world(65, 11)
    w = ra.host_world_prepare(t, rb)
    moved = moved_world(65, 12)
    want = ra.host_world_refit(moved, rb, w["nodes"], w["order"])
    # inv over the transforms, the world boxes over the root boxes, the nodes over themselves
    tt, bb, nodes = np.ascontiguousarray(moved.reshape(65, 12)).copy(), rb.copy(), w["nodes"].copy()
    pad = C.c_float(0)
    rc, msg = _raw(tt, bb, 65, nodes, len(nodes), w["order"], tt, bb, pad, nodes)
    assert rc == 0, msg
    assert tt.tobytes() == want["inv"].tobytes() and bb.tobytes() == want["world_boxes"].tobytes() and nodes.tobytes() == want["nodes"].tobytes()
    assert np.float32(pad.value) == np.float32(want["ray_pad"])


def test_refusals_write_nothing_and_name_the_entry():
    t, rb = random_world(5, 1)
    t = np.ascontiguousarray(t.reshape(5, 12))
    w = ra.host_world_prepare(t, rb)
    assert _raw(t, rb, 5, w["nodes"], 4, w["order"], np.zeros((5, 12), np.float32), np.zeros((5, 6), np.float32), C.c_float(0), np.zeros_like(w["nodes"]))[0] == 0

    def refused(text, t=t, rb=rb, n=5, nodes=w["nodes"], node_count=4, order=w["order"], null=None):
        inv, boxes, out_nodes, pad = np.full((5, 12), -7, np.float32), np.full((5, 6), -7, np.float32), np.zeros(4, engine.GPU_NODE_DTYPE), C.c_float(-7)
        out_nodes["kind"] = 0xABABABAB
        args = dict(t=t, rb=rb, nodes=nodes, order=order, inv=inv, boxes=boxes, pad=pad, out_nodes=out_nodes)
        if null:
            args[null] = None
        rc, msg = _raw(args["t"], args["rb"], n, args["nodes"], node_count, args["order"], args["inv"], args["boxes"], args["pad"], args["out_nodes"])
        assert rc == -1 and "racc_host_world_refit" in msg and text in msg, (rc, msg)
        assert (inv == -7).all() and (boxes == -7).all() and pad.value == -7 and (out_nodes["kind"] == 0xABABABAB).all() and (out_nodes["first"] == 0).all(), "outputs written by a refused call (%s)" % text

    # what racc_host_world_prepare refuses
    for null in ("t", "rb", "nodes", "order", "inv", "boxes", "pad", "out_nodes"):
        refused("NULL", null=null)
    refused("count is 0", n=0)
    refused("2^20", n=(1 << 20) + 1)
    for bad in (np.nan, np.inf, -np.inf):
        tt = t.copy(); tt[1, 11] = bad
        refused("not finite", t=tt)
    bb = rb.copy(); bb[2, 4] = np.nan
    refused("not finite", rb=bb)
    bb = rb.copy(); bb[1, 0], bb[1, 3] = 2, 1
    refused("min > max", rb=bb)
    tt = t.copy(); tt[2, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = 0
    refused("singular", t=tt)
    tt = t.copy(); tt[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = [1, 2, 3, 1, 2, 3, 4, 5, 6]
    refused("singular", t=tt)
    tt = t.copy(); tt[0, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = (np.float32(3e38) * np.eye(3, dtype=np.float32)).reshape(-1)
    refused("not finite", t=tt)
    # a malformed topology
    refused("node_count", node_count=3)
    refused("node_count", node_count=5)
    nodes = w["nodes"].copy(); nodes["first"][0] = 0x80000000 | 4
    refused("child index", nodes=nodes)
    inner = [(i, f) for i in range(4) for f in ("first", "last") if w["nodes"][f][i] & 0x80000000]
    leaves = [(i, f) for i in range(4) for f in ("first", "last") if not w["nodes"][f][i] & 0x80000000]
    i, f = inner[0]
    nodes = w["nodes"].copy(); nodes[f][i] = 0x80000000      # back to the root: reached twice
    refused("reached twice", nodes=nodes)
    (i, f), (j, g) = inner[0], inner[1]
    nodes = w["nodes"].copy(); nodes[g][j] = nodes[f][i]      # one subtree shared
    refused("reached twice", nodes=nodes)
    i, f = inner[-1]
    nodes = w["nodes"].copy(); nodes[f][i] = 0      # a subtree cut off (an empty reference in its place): its node is never reached
    refused("never reached", nodes=nodes)
    i, f = leaves[0]
    nodes = w["nodes"].copy(); nodes[f][i] = (2 << 24) | (int(nodes[f][i]) & 0xFFFFFF)
    refused("more than one instance", nodes=nodes)
    nodes = w["nodes"].copy(); nodes[f][i] = (1 << 24) | 5
    refused("position", nodes=nodes)
    nodes = w["nodes"].copy(); nodes[f][i] = nodes[leaves[1][1]][leaves[1][0]]      # one position in two leaves, another in none
    refused("position", nodes=nodes)
    nodes = w["nodes"].copy(); nodes[f][i] = 0      # an empty reference where an instance belongs
    refused("position", nodes=nodes)
    order = w["order"].copy(); order[0] = order[1]
    refused("permutation", order=order)
    order = w["order"].copy(); order[3] = 5
    refused("permutation", order=order)


def test_stand_alone_driver_under_asan_and_ubsan():
    """tests/cpp/world_refit_host_check.cpp: racc_host_world_refit on worlds of 1 and 257 instances, a refusal and aliasing outputs, built
    with the Makefile's AddressSanitizer + UBSan flags and run as a program of its own."""
    subprocess.check_call(["make", "-s", "-C", engine.CSRC, "../../tests/cpp/world_refit_host_check"])
    exe = os.path.join(os.path.dirname(engine._HERE), "tests", "cpp", "world_refit_host_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "refits checked, 0 failures" in out.stdout
