"""Refit of a device-resident scene to moved vertices — racc_hip_refit_* / racc_hip_scene_refit* (rayaccel_amd/csrc/racc_refit.inc) and
racc::updateScene.  The bar: after every refit the device records, downloaded in blob order, equal racc_host_blobs_refit of the same
vertices BYTE FOR BYTE, and traces on the refitted scene are bit-exact against the oracle on those blobs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, assert_bit_exact, book_rays, book_scene, leaf_rays, leaf_scene, make_rays
from refit_helpers import displaced, scene_size, zero_sign_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "update_scene_check")


def assert_same_records(got, want, what):
    nodes, pairs = got
    a, b = nodes.view(np.uint8).reshape(-1, 64), np.ascontiguousarray(want["nodes"]).view(np.uint8).reshape(-1, 64)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d node records differ, e.g. node %d: device %s, host %s" % (what, len(bad), len(a), bad[0], nodes[bad[0]], want["nodes"][bad[0]])
    a, b = pairs.view(np.uint8).reshape(-1, 48), np.ascontiguousarray(want["pairs"]).view(np.uint8).reshape(-1, 48)
    bad = np.nonzero((a != b).any(1))[0]
    assert len(bad) == 0, "%s: %d of %d pair records differ, e.g. pair %d: device %s, host %s" % (what, len(bad), len(a), bad[0], pairs[bad[0]], want["pairs"][bad[0]])


@pytest.fixture(scope="module")
def rf(small_scene, small_host, small_default_host):
    """A context of this module's own (default options) with the small scene as both builders make it, each with a refit handle."""
    ctx = ra.Context(device=0)
    trees = {}
    for name, host in (("quality 0", small_host), ("default tree", small_default_host)):
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        trees[name] = dict(blobs=host.blobs(), scene=scene, refit=ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"])))
    prim, _ = synth.primary_rays(small_scene["camera"], 256, 256)
    yield dict(ctx=ctx, trees=trees, sc=small_scene, rays=np.concatenate([synth.random_rays(65536, 7), prim]))
    for t in trees.values():
        t["refit"].destroy()
        t["scene"].destroy()
    ctx.destroy()


# ------------------------------------------------------------------------------------------------------------ 1. download without a refit
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_download_without_a_refit_is_the_upload(small_scene, small_host, small_default_host, tree):
    host = small_host if tree == "quality 0" else small_default_host
    with ra.Context(device=0) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        refit = ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"]))
        assert len(host.pairs) > host.pair_count      # padding records are part of the comparison
        assert_same_records(refit.download(), host.blobs(), "%s, download right after create_refit" % tree)
        refit.destroy()
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. A -> B -> A
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_there_and_back(rf, tree):
    t, sc = rf["trees"][tree], rf["sc"]
    a, b = sc["vertices"], displaced(sc["vertices"], 3.0)
    for what, v in (("B", b), ("A again", a)):
        t["refit"].refit(v)
        assert_same_records(t["refit"].download(), ra.host_refit(t["blobs"], v, sc["indices"]), "%s, refit to %s" % (tree, what))
    if tree == "quality 0":
        assert_same_records(t["refit"].download(), t["blobs"], "quality 0, back at A: the original upload")
    assert t["scene"].info["node_count"] == len(t["blobs"]["nodes"])


# ------------------------------------------------------------------------------------------------------------ 3. trace after refit
@pytest.mark.parametrize("displacement", ["a few units", "as large as the scene"])
@pytest.mark.parametrize("tree", ["quality 0", "default tree"])
def test_trace_after_refit(rf, tree, displacement):
    ctx, t, sc, rays = rf["ctx"], rf["trees"][tree], rf["sc"], rf["rays"]
    v = displaced(sc["vertices"], 3.0 if displacement == "a few units" else scene_size(sc["vertices"]), phase=0.5)
    want_blobs = ra.host_refit(t["blobs"], v, sc["indices"])
    ref = orc.traverse(want_blobs, rays, threads=16)
    for what, part in (("random rays", slice(0, 65536)), ("primary rays", slice(65536, None))):
        frac = (ref["triangle"][part] != MISS).mean()
        print("%s, %s, %s: the oracle's hit fraction is %.3f" % (tree, displacement, what, frac))
        assert 0.1 <= frac <= 0.9, "%s, %s: the oracle's hit fraction on the %s is %.3f" % (tree, displacement, what, frac)
    t["refit"].refit(v)
    what = "%s refitted, displacement %s" % (tree, displacement)
    assert_bit_exact(ctx.intersect(t["scene"], None, rays), ref, what + ", host path")
    d_rays, d_res = ctx.alloc(len(rays) * 32), ctx.alloc(len(rays) * 16)
    d_rays.upload(rays)
    ctx.intersect_device(t["scene"], None, d_rays.ptr, d_res.ptr, len(rays), lane=ra.LANE_AUTO)      # the engine's own streams; below this context's chain threshold (786,432 rays) the launch stands alone: the chain is test_chained_batches_after_refit's
    ctx.wait(ra.LANE_AUTO)
    assert_bit_exact(d_res.download(orc.RESULT_DTYPE, len(rays)), ref, what + ", device-resident batch")
    d_rays.free(); d_res.free()
    occ = ctx.occluded(t["scene"], rays)
    assert np.array_equal(occ, (ref["triangle"] != MISS).astype(np.uint8)), what + ": occluded differs from 'the oracle reports a hit'"
    t["refit"].refit(sc["vertices"])


def test_chained_batches_after_refit(small_scene, small_default_host):
    """The chain's kernels on rewritten records.  A default context chains only batches of >= 786,432 rays, so this context chains every
    batch (chain_min_rays=1): three batches back to back after a refit, then a second refit — waited for as the ordering contract asks —
    and three more."""
    sc, host = small_scene, small_default_host
    prim, _ = synth.primary_rays(sc["camera"], 256, 256)
    batches = [synth.random_rays(65536, 7), prim, synth.random_rays(65536, 23)]
    with ra.Context(device=0, chain_min_rays=1) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
        d_rays, d_res = [ctx.alloc(len(r) * 32) for r in batches], [ctx.alloc(len(r) * 16) for r in batches]
        for d, r in zip(d_rays, batches):
            d.upload(r)
        for k, amp in enumerate((3.0, 11.0)):
            v = displaced(sc["vertices"], amp, phase=0.2 + k)
            blobs = ra.host_refit(host.blobs(), v, sc["indices"])
            refit.refit(v)
            for dr, do, r in zip(d_rays, d_res, batches):
                ctx.intersect_device(scene, None, dr.ptr, do.ptr, len(r), lane=ra.LANE_AUTO)
            ctx.wait(ra.LANE_AUTO)
            for i, (do, r) in enumerate(zip(d_res, batches)):
                assert_bit_exact(do.download(orc.RESULT_DTYPE, len(r)), orc.traverse(blobs, r, threads=16), "refit %d, chained batch %d" % (k, i))
        for b in d_rays + d_res:
            b.free()
        refit.destroy()
        scene.destroy()


def test_remap_longer_than_the_pairs(rf, small_host):
    """racc_hip_scene_upload accepts a remap longer than two entries per pair; the device does not hold the unpadded pair count, the handle
    takes it from where the last leaf ends: padding records must still come out as copies of pair 0, as the host refit writes them."""
    sc, ctx = rf["sc"], rf["ctx"]
    blobs = dict(small_host.blobs(), remap=np.concatenate([small_host.remap, np.zeros(10, np.uint32)]))
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
    v = displaced(sc["vertices"], 2.0, phase=0.9)
    refit.refit(v)
    assert_same_records(refit.download(), ra.host_refit(blobs, v, sc["indices"]), "remap with ten spare entries")
    refit.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 4. the hand-off across CUs and XCDs
def test_hand_off_across_xcds():
    """20,000+ triangles: the box kernel has more than 32 workgroups, the two arrivers at a counter sit on different CUs and XCDs, and the
    top of the tree is reached by late arrivers.  A relaxed counter or a missing acquire shows here as a box that misses its sibling's planes."""
    sc = synth.battlefield_synth(grid=100, boxes=32, quads=100)
    assert len(sc["indices"]) >= 20000
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=None)
    assert len(host.nodes) + 1 > 32 * 256      # leaf references = inner nodes + 1: one thread each, 256 per workgroup
    with ra.Context(device=0) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
        st = ctx.create_stream()
        d_v = ctx.alloc(len(sc["vertices"]) * 16)
        size = scene_size(sc["vertices"])
        for k, amp in enumerate((0.5, 3.0, 0.1 * size, size, 7.0)):
            v = np.ascontiguousarray(displaced(sc["vertices"], amp, phase=0.3 * k), np.float32)
            assert v.shape[1] == 4
            d_v.upload(v)
            refit.refit_device(d_v.ptr, len(v), stream=st)
            ctx.stream_synchronize(st)
            assert_same_records(refit.download(), ra.host_refit(host.blobs(), v, sc["indices"]), "refit %d (amplitude %.1f) through refit_device" % (k, amp))
        d_v.free()
        ctx.destroy_stream(st)
        refit.destroy()
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 5. hand-made edge scenes
def _edge_case(ctx, blobs, geometry, moved, rays, what):
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    refit = ctx.create_refit(scene, geometry["indices"], len(geometry["vertices"]))
    assert_same_records(refit.download(), blobs, what + ", before any refit")
    for step, v in (("moved", moved), ("back", geometry["vertices"])):
        refit.refit(v)
        want = ra.host_refit(blobs, v, geometry["indices"])
        assert_same_records(refit.download(), want, "%s, %s" % (what, step))
        ref = orc.traverse(want, rays)
        assert_bit_exact(ctx.intersect(scene, None, rays), ref, "%s, %s" % (what, step))
    refit.destroy()
    scene.destroy()
    return ref


def test_hand_made_edge_scenes(rf):
    ctx = rf["ctx"]
    # a leaf of 127 pairs (the format's limit) beside a lone triangle
    blobs, geo = leaf_scene(127, "row")
    ref = _edge_case(ctx, blobs, geo, displaced(geo["vertices"], 0.2), leaf_rays(127, "row"), "leaf of 127 pairs")
    assert (ref["triangle"] != MISS).any() and (ref["triangle"] == MISS).any()
    # one leaf of 126 lone triangles that all have the same box, deep one-sided levels above the four far triangles
    sc = book_scene(126)
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=0)
    ref = _edge_case(ctx, host.blobs(), sc, displaced(sc["vertices"], 0.05), book_rays(sc, 126), "book of 126 pages")
    assert (ref["triangle"] != MISS).mean() > 0.5
    # +0.0 against -0.0: the select keeps the accumulator, the first vertex folded decides the sign of a zero plane
    blobs, geo, va, vb = zero_sign_scene()
    rays = make_rays([[0.75, 0.25, -1], [0.25, 0.75, -1], [0.5, 0.5, 5], [1.0, 5.3, -3], [-2, -2, -1]], [[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1]])
    ref = _edge_case(ctx, blobs, geo, vb, rays, "signed zeros")
    assert list(ref["triangle"] != MISS) == [True, True, True, True, False]


# ------------------------------------------------------------------------------------------------------------ 6. fast mode is refused
@pytest.mark.skipif(not ra.load_library().racc_hip_variant_available(50), reason="this build has no kernel_variant 50")
def test_fast_mode_is_refused(small_scene, small_default_host):
    host = small_default_host
    rays = synth.random_rays(8192, 3)
    with ra.Context(device=0, kernel_variant=50) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        before = ctx.intersect(scene, None, rays)
        with pytest.raises(ra.RaccError) as e:
            ctx.create_refit(scene, small_scene["indices"], len(small_scene["vertices"]))
        assert e.value.code == -1 and "refit_create" in str(e.value)
        after = ctx.intersect(scene, None, rays)
        assert before.tobytes() == after.tobytes() and (before["triangle"] != MISS).mean() > 0.1
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. destroy gives memory back
def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the engine itself is linked against."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_destroy_gives_the_memory_back():
    """A mesh large enough for the handle's device arrays (16 B per pair, 8 B per leaf, 8 B per device record, 16 B per vertex of staging)
    to be seen in hipMemGetInfo: what create + one refit took must come back but for an eighth (allocation granularity)."""
    sc = synth.battlefield_synth(grid=300, boxes=32, quads=100)
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=0)
    with ra.Context(device=0) as ctx:
        scene = ctx.upload_scene(host.nodes, host.pairs, host.remap)
        before = _free_device_memory()
        refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
        refit.refit(sc["vertices"])
        held = before - _free_device_memory()
        refit.destroy()
        after = _free_device_memory()
        print("refit handle: %d bytes of device memory held, %d not returned by destroy" % (held, before - after))
        assert held >= 2 << 20, "the handle holds %d bytes: too little for this test to see" % held
        assert abs(before - after) <= held // 8
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 8. racc::updateScene
def _run_update(tmp_path, sc, moved, rays, env=None):
    files = [os.path.join(str(tmp_path), n) for n in ("mesh.bin", "moved.bin", "rays.bin", "out.bin")]
    v = np.ascontiguousarray(sc["vertices"], np.float32)
    assert v.shape[1] == 4
    with open(files[0], "wb") as f:
        f.write(np.array([len(v), len(sc["indices"])], np.uint32).tobytes() + v.tobytes() + np.ascontiguousarray(sc["indices"], np.uint32).tobytes())
    with open(files[1], "wb") as f:
        f.write(np.ascontiguousarray(moved, np.float32).tobytes())
    with open(files[2], "wb") as f:
        f.write(np.array([len(rays)], np.uint32).tobytes() + np.ascontiguousarray(rays).tobytes())
    p = subprocess.run([BIN] + files, capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    return p, files[3]


def test_update_scene_through_render(tmp_path, small_scene, small_default_host):
    sc = small_scene
    moved = displaced(sc["vertices"], 3.0, phase=1.0)
    prim, _ = synth.primary_rays(sc["camera"], 256, 256)
    rays = np.concatenate([prim, synth.random_rays(40000, 17)])
    p, out = _run_update(tmp_path, sc, moved, rays)
    assert p.returncode == 0, p.stdout + p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1])["raysTraced"] == len(rays)
    got = np.fromfile(out, orc.RESULT_DTYPE)
    ref = orc.traverse(ra.host_refit(small_default_host.blobs(), moved, sc["indices"]), rays, threads=8)      # racc::createScene builds the default tree
    assert 0.1 <= (ref["triangle"] != MISS).mean() <= 0.9
    assert np.array_equal(got["triangle"], ref["triangle"])
    hit = ref["triangle"] != MISS
    for f in ("t", "u", "v"):
        assert np.array_equal(got[f][hit].view(np.uint32), ref[f][hit].view(np.uint32))
        np.testing.assert_allclose(got[f][~hit], ref[f][~hit], rtol=1e-5, atol=1e-5)
    if ra.load_library().racc_hip_variant_available(50):      # a context in fast-traversal mode: false and one "RayAccelerator: ..." line
        p, _ = _run_update(tmp_path, sc, moved, rays[:64], env=dict(RACC_FAST_TRAVERSAL="1"))
        assert p.returncode == 7 and p.stderr.count("RayAccelerator:") == 1 and "updateScene" in p.stderr, p.stdout + p.stderr
