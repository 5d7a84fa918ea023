"""racc_host_scene_wide_nodes_refit — the rule by which a refit carries moved boxes into the 4-wide (format 45) and compressed (format 50)
records (include/racc_hip.h, "host wide refit"; rayaccel_amd/csrc/racc_refit_wide.inc).  No GPU.

The function states the collapse and the quantisation a second time (racc_scene_format.inc may not change): with now == built it must
give racc_host_scene_wide_nodes byte for byte, which holds the two statements together — on the small scene's two trees, and on hand-made
frames whose lower planes are +0.0 / -0.0 in every slot order, where the fold of the frame's origin decides a sign bit."""
import itertools

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import engine
from refit_helpers import NEG0, POS0, displaced, scene_size, zero_sign_scene
from wide_refit_helpers import assert_wide_refit_rule, collapsed, flattened, overflowing


def _counts(host):
    return len(host.pairs), len(host.remap)


def _refit_both(blobs, now_nodes):
    pc, rc = len(blobs["pairs"]), len(blobs["remap"])
    built45 = engine.wide_nodes(blobs["nodes"], pc, rc, 45)[0]
    now45, d45 = ra.host_wide_refit(blobs["nodes"], now_nodes, pc, rc, 45)
    now50, d50 = ra.host_wide_refit(blobs["nodes"], now_nodes, pc, rc, 50)
    assert d45 == 0, "format 45 holds any box: it never disables"
    return built45, now45, now50, d50


@pytest.mark.parametrize("fmt", [45, 50])
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_identity(small_host, small_default_host, tree, fmt):
    host = small_host if tree == "quality 0" else small_default_host
    want, _ = engine.wide_nodes(host.nodes, *_counts(host), fmt)
    got, disabled = ra.host_wide_refit(host.nodes, host.nodes, *_counts(host), fmt)
    assert disabled == 0 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "%s, format %d: now == built does not give racc_host_scene_wide_nodes" % (tree, fmt)


@pytest.mark.parametrize("displacement", ["a few units", "as large as the scene"])
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_displaced(small_scene, small_host, small_default_host, tree, displacement):
    host, sc = (small_host if tree == "quality 0" else small_default_host), small_scene
    v = displaced(sc["vertices"], 3.0 if displacement == "a few units" else scene_size(sc["vertices"]), phase=0.5)
    now = ra.host_refit(host.blobs(), v, sc["indices"])
    assert not np.array_equal(now["nodes"]["leftMin"], host.nodes["leftMin"])
    built45, now45, now50, disabled = _refit_both(host.blobs(), now["nodes"])
    assert disabled == 0
    assert_wide_refit_rule(built45, now45, now50, now["nodes"], 0, "%s, displaced %s" % (tree, displacement))
    assert not np.array_equal(now45, built45)


def _four_leaf_blob(lower, upper):
    """Three nodes, four one-pair leaves -> ONE wide record whose slot i holds the box lower[i] .. upper[i] ([4, 3] each)."""
    nodes = np.zeros(3, orc.GPU_NODE_DTYPE)
    nodes["kind"] = 1
    nodes["first"][0], nodes["last"][0] = 0x80000001, 0x80000002
    nodes["parent"][1:] = 0
    for n, (a, b) in ((1, (0, 1)), (2, (2, 3))):
        nodes["first"][n], nodes["last"][n] = (1 << 24) | a, (1 << 24) | b
        nodes["leftMin"][n], nodes["leftMax"][n], nodes["rightMin"][n], nodes["rightMax"][n] = lower[a], upper[a], lower[b], upper[b]
    nodes["leftMin"][0], nodes["leftMax"][0] = np.minimum(lower[0], lower[1]), np.maximum(upper[0], upper[1])
    nodes["rightMin"][0], nodes["rightMax"][0] = np.minimum(lower[2], lower[3]), np.maximum(upper[2], upper[3])
    return nodes


def test_signed_zero_frames_in_every_slot_order():
    """The origin of a frame is the fold of its lower planes; for planes that are all zeros the fold's rule decides the sign bit the record
    stores.  All sixteen sign patterns of four slots, on x with an extent, on y without one (upper planes zeros of the opposite sign), and
    on z with the pattern reversed: racc_host_scene_wide_nodes (quantiseWide's std::fmin fold) and the restated select agree on every
    byte, and the stored origin is the FIRST slot's zero."""
    for signs in itertools.product((POS0, NEG0), repeat=4):
        s = np.array(signs, np.float32)
        lower = np.stack([s, s, s[::-1]], 1)
        upper = np.stack([np.ones(4, np.float32), -s, np.full(4, 2.0, np.float32)], 1)
        nodes = _four_leaf_blob(lower, upper)
        for fmt in (45, 50):
            want, _ = engine.wide_nodes(nodes, 32, 8, fmt)
            got, disabled = ra.host_wide_refit(nodes, nodes, 32, 8, fmt)
            assert len(want) == 1 and disabled == 0
            assert got.tobytes() == want.tobytes(), "format %d, lower planes %s: %s against %s" % (fmt, signs, got, want)
        org = got[0, 4:7].view(np.float32)
        # (on y min < max is false, so the collapse's ordering takes the box's max — the zero of the opposite sign — as the lower plane)
        assert (org == 0).all() and list(np.signbit(org)) == [np.signbit(s[0]), not np.signbit(s[0]), np.signbit(s[3])], "lower planes %s: origin %s" % (signs, org)


@pytest.mark.parametrize("target", ["plane", "point"])
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_frames_without_extent(small_scene, small_host, small_default_host, tree, target):
    host, sc = (small_host if tree == "quality 0" else small_default_host), small_scene
    v = flattened(sc["vertices"]) if target == "plane" else collapsed(sc["vertices"])
    now = ra.host_refit(host.blobs(), v, sc["indices"])
    built45, now45, now50, disabled = _refit_both(host.blobs(), now["nodes"])
    assert disabled == 0
    assert_wide_refit_rule(built45, now45, now50, now["nodes"], 0, "%s, mesh flattened to a %s" % (tree, target))
    tiny = np.finfo(np.float32).tiny
    scale = now50[:, 7:10].view(np.float32)
    assert (scale[:, 1] == tiny).all() and ((scale == tiny).all() if target == "point" else (scale[:, 0] > tiny).any())


def test_zero_sign_scene():
    """refit_helpers.zero_sign_scene: one node, vertex sets A and B differ only in which zeros are negative.  One wide record with two used
    slots; the refitted records are racc_host_scene_wide_nodes of the refitted blob (the collapse of one node has nothing to choose)."""
    blobs, geo, va, vb = zero_sign_scene()
    origins = []
    for v in (va, vb):
        now = ra.host_refit(blobs, v, geo["indices"])
        for fmt in (45, 50):
            want, _ = engine.wide_nodes(now["nodes"], len(now["pairs"]), len(now["remap"]), fmt)
            got, disabled = ra.host_wide_refit(blobs["nodes"], now["nodes"], len(blobs["pairs"]), len(blobs["remap"]), fmt)
            assert disabled == 0 and got.tobytes() == want.tobytes()
        origins.append(got[0, 4:7].copy())
    assert not np.array_equal(origins[0], origins[1]) and (np.array(origins).view(np.float32)[:, [0, 2]] == 0).all()


@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_overflowing_frame_is_disabled(small_scene, small_host, small_default_host, tree):
    """Coordinates of -3e38 and +3e38 are finite and every box holds them exactly; their difference is not: format 50 disables every frame
    that spans both (the root's at least) and counts it, format 45 holds the boxes bit for bit."""
    host, sc = (small_host if tree == "quality 0" else small_default_host), small_scene
    v = overflowing(sc["vertices"])
    now = ra.host_refit(host.blobs(), v, sc["indices"])
    built45, now45, now50, disabled = _refit_both(host.blobs(), now["nodes"])
    assert 0 < disabled < len(now50)
    assert_wide_refit_rule(built45, now45, now50, now["nodes"], disabled, tree + ", +-3e38")
    assert np.isposinf(now50[0, 4:7].view(np.float32)).all(), "the root's frame spans both vertices"
    x = now45[:, 4:12].view(np.float32)
    x = x[np.isfinite(x)]      # (unused slots hold +inf)
    assert x.min() == np.float32(-3e38) and x.max() == np.float32(3e38)
