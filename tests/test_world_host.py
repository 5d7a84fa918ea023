"""racc_host_world_prepare (rayaccel_amd/csrc/world_build.cpp): the host side of instancing — inverse transforms, conservative world boxes,
the top-level BVH2.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from rayaccel_amd import engine
from world_helpers import adjugate_inverse, affine, rotation


def random_world(n, seed, spread=50.0):
    """n general affine transforms (rotation, non-uniform scale of either sign, translation) and object boxes, some of them flat."""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        scale = rng.uniform(0.3, 3.0, 3) * rng.choice([-1.0, 1.0], 3)
        t[i] = affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), scale, rng.uniform(-spread, spread, 3))
    lo = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    ext = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    ext[rng.uniform(size=(n, 3)) < 0.15] = 0      # flat boxes
    return t, np.concatenate([lo, lo + ext], 1).astype(np.float32)


@pytest.fixture(scope="module", params=[1, 2, 3, 7, 64, 1000])
def prepared(request):
    t, rb = random_world(request.param, 100 + request.param)
    return t, rb, ra.host_world_prepare(t, rb)


def test_inverse_is_the_double_inverse_rounded(prepared):
    t, _, w = prepared
    inv64, det = adjugate_inverse(t)
    assert np.array_equal(w["inv"].view(np.uint32), inv64.astype(np.float32).view(np.uint32)), "inv is not the float64 inverse rounded to float32"
    # ... and that expression is the inverse: against numpy's LU-based one to well below a float32 ulp, and inv . M = identity in double
    m4 = np.zeros((len(t), 4, 4))
    m4[:, :3, :] = t
    m4[:, 3, 3] = 1
    lu = np.linalg.inv(m4)[:, :3, :]
    scale = np.abs(lu).max((1, 2), keepdims=True)
    assert (np.abs(inv64 - lu) <= 1e-12 * scale).all()
    assert (np.abs(w["inv"].astype(np.float64) - lu) <= 2.0 ** -23 * scale).all()


def test_world_boxes_contain_the_transformed_corners(prepared):
    t, rb, w = prepared
    t64 = t.astype(np.float64)
    for corner in range(8):
        p = np.stack([rb[:, k + 3 * ((corner >> k) & 1)] for k in range(3)], 1).astype(np.float64)
        q = np.einsum("nrk,nk->nr", t64[:, :, :3], p) + t64[:, :, 3]
        assert (w["world_boxes"][:, :3].astype(np.float64) <= q).all() and (q <= w["world_boxes"][:, 3:].astype(np.float64)).all(), "corner %d outside" % corner
    # conservative, not absurd: the margin is a few 2^-20 of the magnitudes involved
    size = (w["world_boxes"][:, 3:] - w["world_boxes"][:, :3]).astype(np.float64)
    ext = np.einsum("nrk,nk->nr", np.abs(t64[:, :, :3]), (rb[:, 3:] - rb[:, :3]).astype(np.float64))      # the exact world box's size
    mag = np.abs(w["world_boxes"]).max(1, keepdims=True) + np.abs(t64[:, :, 3]).max(1, keepdims=True)
    assert (size >= ext).all() and (size - ext <= 1e-3 * mag).all()
    assert 0 < w["ray_pad"] < 1e-3


def walk(w):
    """Depth-first over the top-level blob: returns (instances per leaf visit, box of everything below every child, height); asserts the
    project's scene validation rules on the way (in-range children, every node reached once, non-empty leaves but for the one-instance root)."""
    nodes, order, boxes = w["nodes"], w["order"], w["world_boxes"]
    n = len(order)
    seen_nodes, seen_inst = np.zeros(len(nodes), int), np.zeros(n, int)
    height = [0]

    def below(ref, depth, parent):
        if ref & 0x80000000:
            i = ref & 0x7FFFFFFF
            assert i < len(nodes), "child index out of range"
            seen_nodes[i] += 1
            assert seen_nodes[i] == 1, "node %d reached twice (a cycle or a shared subtree)" % i
            assert nodes["parent"][i] == parent and 1 <= nodes["kind"][i] <= 3
            height[0] = max(height[0], depth)
            lo_l, hi_l = below(int(nodes["first"][i]), depth + 1, i)
            lo_r, hi_r = below(int(nodes["last"][i]), depth + 1, i)
            if lo_l is not None:
                assert (nodes["leftMin"][i] <= lo_l).all() and (hi_l <= nodes["leftMax"][i]).all(), "node %d: left box does not contain its subtree" % i
            if lo_r is not None:
                assert (nodes["rightMin"][i] <= lo_r).all() and (hi_r <= nodes["rightMax"][i]).all(), "node %d: right box does not contain its subtree" % i
            los = [x for x in (lo_l, lo_r) if x is not None]
            his = [x for x in (hi_l, hi_r) if x is not None]
            return np.min(los, 0), np.max(his, 0)
        first, cnt = ref & 0xFFFFFF, ref >> 24
        if cnt == 0:
            assert n == 1 and ref == 0, "an empty leaf outside a one-instance world"
            return None, None
        assert first + cnt <= n, "leaf range out of bounds"
        ids = order[first:first + cnt]
        seen_inst[ids] += 1
        return boxes[ids, :3].min(0), boxes[ids, 3:].max(0)

    below(0x80000000, 1, 0xFFFFFFFF)
    assert (seen_nodes == 1).all(), "unreachable nodes"
    assert (seen_inst == 1).all(), "an instance is in no leaf or in several"
    return height[0]


def test_top_level_tree_is_valid_and_contains_what_is_below(prepared):
    t, rb, w = prepared
    n = len(t)
    assert sorted(w["order"].tolist()) == list(range(n))
    assert len(w["nodes"]) == max(n - 1, 1)
    assert walk(w) == w["height"]
    assert w["height"] <= int(np.ceil(np.log2(max(n, 2)))), "median splits give a balanced tree"


def test_multi_instance_tree_passes_the_upload_validation():
    """The project's own validator (racc_host_scene_device_nodes runs validateScene) accepts the blob as a scene over `count` pairs."""
    t, rb = random_world(100, 5)
    w = ra.host_world_prepare(t, rb)
    dev = engine.device_nodes(w["nodes"], 100, 200)
    assert len(dev) >= len(w["nodes"])


def test_output_is_deterministic():
    t, rb = random_world(500, 9)
    t[10:20] = t[10]; rb[10:20] = rb[10]      # identical instances: ties in every split
    a, b = ra.host_world_prepare(t, rb), ra.host_world_prepare(t.copy(), rb.copy())
    for k in ("inv", "world_boxes", "nodes", "order"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["ray_pad"] == b["ray_pad"] and a["height"] == b["height"]


def test_refusals():
    t, rb = random_world(3, 1)
    ok = ra.host_world_prepare(t, rb)
    assert len(ok["nodes"]) == 2

    def refused(tt, bb, text):
        with pytest.raises(ra.RaccError) as e:
            ra.host_world_prepare(tt, bb)
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    for bad in (np.nan, np.inf, -np.inf):
        tt = t.copy(); tt[1, 2, 3] = bad
        refused(tt, rb, "not finite")
    tt = t.copy(); tt[2, :, :3] = 0
    refused(tt, rb, "singular")
    tt = t.copy(); tt[0, :, :3] = [[1, 2, 3], [1, 2, 3], [4, 5, 6]]      # two equal rows of small integers: the determinant is exactly zero in double
    refused(tt, rb, "singular")
    tt = t.copy(); tt[0, :, :3] = np.float32(2.0 ** 100) * np.eye(3, dtype=np.float32)      # determinant 2^300: float overflows, double does not — accepted
    assert ra.host_world_prepare(tt, np.zeros_like(rb))["inv"][0, 0, 0] == np.float32(2.0 ** -100)
    tt = t.copy(); tt[0, :, :3] = np.float32(3e38) * np.eye(3, dtype=np.float32)
    refused(tt, rb, "not finite")                     # the world box overflows float
    bb = rb.copy(); bb[1, 0] = np.nan
    refused(t, bb, "not finite")
    bb = rb.copy(); bb[1, 0], bb[1, 3] = 2, 1
    refused(t, bb, "min > max")
    refused(np.zeros((0, 3, 4), np.float32), np.zeros((0, 6), np.float32), "count is 0")


def test_stand_alone_driver_under_asan_and_ubsan():
    """tests/cpp/world_host_check.cpp: racc_host_world_prepare on a few hundred random and degenerate inputs (flat boxes, negative scale,
    mirrors), built with the Makefile's AddressSanitizer + UBSan flags and run as a program of its own."""
    subprocess.check_call(["make", "-s", "-C", engine.CSRC, "../../tests/cpp/world_host_check"])
    exe = os.path.join(os.path.dirname(engine._HERE), "tests", "cpp", "world_host_check")
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "worlds checked" in out.stdout
