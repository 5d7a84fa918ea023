"""Host refit (racc_host_blobs_refit, rayaccel_amd/csrc/scene_refit.cpp): the specification of the refit rule.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import engine, synth
from helpers import MISS, assert_matches_arbiter, assert_same_hits_across_trees
from refit_helpers import assert_planes_equal, displaced, hand_refit_zero_sign, numpy_refit, scene_size, zero_sign_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def unsplit_host(small_scene):
    return ra.HostScene(small_scene["vertices"], small_scene["indices"], quality=1, split_percent=-1)


def same_bytes(a, b):
    return a["nodes"].tobytes() == b["nodes"].tobytes() and a["pairs"].tobytes() == b["pairs"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- identity
def test_identity_on_unsplit_trees(small_scene, small_host, unsplit_host):
    for what, host in (("quality 0", small_host), ("quality 1 without splits", unsplit_host)):
        got = ra.host_refit(host.blobs(), small_scene["vertices"], small_scene["indices"])
        same = (got["nodes"].view(np.uint8).reshape(-1, 64) == host.nodes.view(np.uint8).reshape(-1, 64)).all(1)
        assert same.all(), "%s: %d of %d node records differ from the build" % (what, (~same).sum(), len(same))
        assert got["pairs"].tobytes() == host.pairs.tobytes(), what
        assert np.array_equal(got["remap"], host.remap)


def test_identity_on_the_default_split_tree(small_scene, small_default_host):
    host = small_default_host
    got = ra.host_refit(host.blobs(), small_scene["vertices"], small_scene["indices"])
    assert got["pairs"].tobytes() == host.pairs.tobytes()
    for f in ("leftMin", "rightMin"):
        assert (got["nodes"][f] <= host.nodes[f]).all(), "a refit box does not contain the built one (%s)" % f
    for f in ("leftMax", "rightMax"):
        assert (got["nodes"][f] >= host.nodes[f]).all(), "a refit box does not contain the built one (%s)" % f
    same = (got["nodes"].view(np.uint8).reshape(-1, 64) == host.nodes.view(np.uint8).reshape(-1, 64)).all(1)
    print("default tree: %d of %d node records byte-identical after the identity refit" % (same.sum(), len(same)))
    assert same.sum() * 2 >= len(same)
    for f in ("kind", "parent", "first", "last"):
        assert np.array_equal(got["nodes"][f], host.nodes[f])


def test_outputs_may_alias_inputs(small_scene, small_host):
    moved = displaced(small_scene["vertices"], 3.0)
    want = ra.host_refit(small_host.blobs(), moved, small_scene["indices"])
    nodes, pairs = small_host.nodes.copy(), small_host.pairs.copy()
    v, idx = engine._as_verts4(moved), np.ascontiguousarray(small_scene["indices"], np.uint32).reshape(-1)
    p = engine._ptr
    rc = ra.load_library().racc_host_blobs_refit(p(nodes), len(nodes), p(pairs), len(pairs), small_host.pair_count, p(small_host.remap), len(small_host.remap),
                                                 p(v), len(v), p(idx), idx.size, p(nodes), p(pairs))
    assert rc == 0 and nodes.tobytes() == want["nodes"].tobytes() and pairs.tobytes() == want["pairs"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- moved vertices
@pytest.fixture(scope="module", params=["a few units", "as large as the scene"])
def moved(request, small_scene):
    amp = 3.0 if request.param == "a few units" else scene_size(small_scene["vertices"])
    return dict(name=request.param, vertices=displaced(small_scene["vertices"], amp), indices=small_scene["indices"])


def test_moved_vertices_match_the_numpy_restatement(moved, small_host, unsplit_host, small_default_host):
    for what, host in (("quality 0", small_host), ("unsplit quality 1", unsplit_host), ("default tree", small_default_host)):
        got = ra.host_refit(host.blobs(), moved["vertices"], moved["indices"])
        assert_planes_equal(got, numpy_refit(host.blobs(), moved["vertices"], moved["indices"]), "%s, displacement %s" % (what, moved["name"]))


def test_moved_vertices_trace_like_a_fresh_build(moved, small_scene, small_host, small_default_host):
    sc = dict(vertices=moved["vertices"], indices=moved["indices"])
    prim, _ = synth.primary_rays(small_scene["camera"], 96, 96)
    rays = np.concatenate([prim, synth.random_rays(8192, 13)])
    fresh = orc.traverse(ra.HostScene(moved["vertices"], moved["indices"], quality=0).blobs(), rays, threads=8)
    assert 0.05 < (fresh["triangle"] != MISS).mean() < 0.95
    for what, host in (("quality 0", small_host), ("default tree", small_default_host)):
        refitted = ra.host_refit(host.blobs(), moved["vertices"], moved["indices"])
        got = orc.traverse(refitted, rays, threads=8)
        assert_same_hits_across_trees(fresh, got, "%s refitted, displacement %s" % (what, moved["name"]))
        assert_matches_arbiter(got[:2048], sc, rays[:2048])
        assert_matches_arbiter(got[-2048:], sc, rays[-2048:])


def test_signed_zeros_bytes_worked_out_by_hand():
    blobs, geo, va, vb = zero_sign_scene()
    for what, v in (("set A (the identity)", va), ("set B", vb), ("set A again", va)):
        got = ra.host_refit(blobs, v, geo["indices"])
        want = hand_refit_zero_sign(v)
        for f in ("leftMin", "leftMax", "rightMin", "rightMax"):
            assert got["nodes"][f].tobytes() == want["nodes"][f].tobytes(), "%s: %s is %s, by hand %s" % (what, f, got["nodes"][f], want["nodes"][f])
        assert got["pairs"].tobytes() == want["pairs"].tobytes(), what
        blobs = got
    assert np.signbit(got["nodes"]["leftMin"][0][1]) and not np.signbit(got["nodes"]["leftMin"][0][0])      # set A: y of `a` is -0.0, x is +0.0
    assert_planes_equal(got, numpy_refit(blobs, va, geo["indices"]), "signed zeros")


# ---------------------------------------------------------------------------------------------------------------- refusals
def _raw(host, vertices, indices, remap=None):
    nodes, pairs = np.full(len(host.nodes) * 64, 0xAB, np.uint8), np.full(len(host.pairs) * 48, 0xAB, np.uint8)
    v, idx = engine._as_verts4(vertices), np.ascontiguousarray(indices, np.uint32).reshape(-1)
    remap = host.remap if remap is None else remap
    p = engine._ptr
    lib = ra.load_library()
    rc = lib.racc_host_blobs_refit(p(host.nodes), len(host.nodes), p(host.pairs), len(host.pairs), host.pair_count, p(remap), len(remap),
                                   p(v), len(v), p(idx), idx.size, p(nodes), p(pairs))
    return rc, lib.racc_hip_last_error(), bool((nodes == 0xAB).all() and (pairs == 0xAB).all())


def test_refusals_write_nothing(small_scene, small_host):
    v, idx = small_scene["vertices"], np.array(small_scene["indices"], np.uint32)
    rc, _, untouched = _raw(small_host, v, idx)
    assert rc == 0 and not untouched
    bad_idx = idx.copy()
    bad_idx.reshape(-1)[len(bad_idx.reshape(-1)) // 2] = len(v)
    bad_remap = small_host.remap.copy()
    bad_remap[2 * (small_host.pair_count - 1)] = (bad_remap[2 * (small_host.pair_count - 1)] & 0xC0000000) | (idx.size // 3)
    nan_v, inf_v = np.array(v, np.float32, copy=True), np.array(v, np.float32, copy=True)
    nan_v[len(v) // 3, 1] = np.nan
    inf_v[len(v) - 1, 2] = -np.inf
    for what, args in (("an index >= vertex_count", (v, bad_idx, None)), ("a remap id >= the triangle count", (v, idx, bad_remap)),
                       ("a NaN vertex", (nan_v, idx, None)), ("an Inf vertex", (inf_v, idx, None))):
        rc, msg, untouched = _raw(small_host, *args)
        assert rc == -1 and msg.startswith(b"racc_host_blobs_refit:"), (what, rc, msg)
        assert untouched, "%s: refused, but the output arrays were written" % what
    with pytest.raises(ra.RaccError):
        ra.host_refit(small_host.blobs(), nan_v, idx)


def test_blob_rules_agree_with_the_upload(small_host):
    """scene_refit.cpp restates racc_hip_scene_upload's blob rules (validateScene, racc_scene_format.inc: another translation unit).  This
    holds the two together: every malformed blob one refuses, the other refuses (racc_host_scene_device_nodes runs validateScene without a GPU)."""
    lib, p = ra.load_library(), engine._ptr
    v, idx = engine._as_verts4(np.zeros((4, 3), np.float32)), np.zeros(3, np.uint32)

    def both(nodes, npairs, remap):
        n = C.c_uint32(0)
        upload = lib.racc_host_scene_device_nodes(p(nodes), len(nodes), npairs, len(remap), 1, None, 0, C.byref(n))
        pairs = np.zeros(max(npairs, 1), orc.PAIR_DTYPE)
        out_n, out_p = np.zeros_like(nodes), np.zeros_like(pairs)
        refit = lib.racc_host_blobs_refit(p(nodes), len(nodes), p(pairs), npairs, npairs, p(remap), len(remap), p(v), len(v), p(idx), idx.size, p(out_n), p(out_p))
        return upload, refit

    good = np.zeros(2, orc.GPU_NODE_DTYPE)
    good["first"], good["last"] = [0x80000001, (1 << 24) | 0], [(1 << 24) | 1, (1 << 24) | 2]
    remap = np.zeros(6, np.uint32)
    assert both(good, 3, remap) == (0, 0)
    cases = {}
    for name, (node, field, value) in dict(child_out_of_range=(0, "first", 0x80000002), cycle=(1, "first", 0x80000000), twice=(1, "last", 0x80000001),
                                           empty_leaf=(1, "last", 2), leaf_out_of_range=(1, "last", (2 << 24) | 2)).items():
        bad = good.copy()
        bad[field][node] = value
        cases[name] = both(bad, 3, remap)
    cases["remap_too_short"] = both(good, 3, remap[:4])
    for name, (upload, refit) in cases.items():
        assert upload != 0 and refit != 0, "%s: upload says %d, host refit says %d" % (name, upload, refit)


# ---------------------------------------------------------------------------------------------------------------- sanitizers
def test_stand_alone_driver_under_asan_and_ubsan():
    """tests/cpp/refit_host_check.cpp + scene_refit.cpp + scene_build.cpp with -fsanitize=address,undefined (`make asan`), run as a program."""
    subprocess.check_call(["make", "-s", "-C", engine.CSRC, "asan"])
    p = subprocess.run([os.path.join(ROOT, "tests", "cpp", "refit_host_check")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 differences" in p.stdout and "ERROR" not in p.stderr and "runtime error" not in p.stderr
