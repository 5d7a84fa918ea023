"""Occlusion (any-hit) queries on worlds — racc_hip_world_occluded / racc_hip_world_occluded_device, worldOccludedKernel
(rayaccel_amd/csrc/racc_world_occlusion.inc).

The bar, in every test: occluded == (some instance's composed closest-hit result is a hit), for every ray, no allowances.  The expectation
is computed on the CPU — world_helpers.compose(inv, blobs, rays)[2].any(0): the specification's ray transform in numpy.float32 with the
library's own `inv`, the oracle's traversal per instance with the ray's own maxT, the per-instance hit masks ORed together.  Every device
output carries 16 guard bytes behind `count`, which must come back untouched, and every output byte is 0 or 1.  No test asserts a time."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, assert_bit_exact, book_rays, book_scene, comb_scene, leaf_rays, leaf_scene, make_rays
from world_helpers import IDENTITY, NO_INSTANCE, affine, compose, object_rays, rotation

pytestmark = pytest.mark.gpu

GUARD = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prepare(transforms, blobs_list):
    return ra.host_world_prepare(np.array(transforms, np.float32), np.array([ra.root_box(b["nodes"]) for b in blobs_list]))


def expectation(transforms, blobs_list, rays, threads=16):
    """(occluded as uint8 [N], composed closest hit Result[N], per-instance hit masks [I, N]) on the CPU."""
    w = prepare(transforms, blobs_list)
    res, _, hits = compose(w["inv"], blobs_list, rays, threads=threads)
    return hits.any(0).astype(np.uint8), res, hits


def issue(ctx, world, rays, stream=None):
    """One device-resident launch, not waited for: (device rays, device output with its guard, count)."""
    n = len(rays)
    d_r = ctx.alloc(max(n, 1) * 32)
    if n:
        d_r.upload(rays)
    d_o = ctx.alloc(n + GUARD)
    d_o.upload(np.full(n + GUARD, 0xAB, np.uint8))
    world.occluded_device(d_r.ptr, d_o.ptr, n, stream=stream)
    return d_r, d_o, n


def checked(buf, n, what=""):
    assert (buf[n:] == 0xAB).all(), "%s: guard bytes behind the output were written" % what
    assert (buf[:n] <= 1).all(), "%s: output bytes other than 0 and 1: %s" % (what, np.unique(buf[:n]))
    return buf[:n].copy()


def collect(launch, what=""):
    d_r, d_o, n = launch
    buf = d_o.download(np.uint8, n + GUARD)
    d_r.free(); d_o.free()
    return checked(buf, n, what)


def device_path(ctx, world, rays, stream=None, what=""):
    launch = issue(ctx, world, rays, stream)
    ctx.stream_synchronize(stream)
    return collect(launch, what)


def host_path(world, rays, what=""):
    buf = np.full(len(rays) + GUARD, 0xAB, np.uint8)
    world.occluded(rays, out=buf)
    return checked(buf, len(rays), what)


def assert_exact(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0 and np.array_equal(got, want), "%s: %d of %d rays differ from the expectation, e.g. rays %s: got %s want %s" % (
        what, len(bad), len(want), bad[:8], got[bad[:8]], want[bad[:8]])


def check_both_paths(ctx, world, rays, want, what):
    assert_exact(device_path(ctx, world, rays, what=what), want, what + " (device path)")
    assert_exact(host_path(world, rays, what=what), want, what + " (host path)")


def reported_by_intersect(world, rays):
    return (world.intersect(rays)[1] != NO_INSTANCE).astype(np.uint8)


def sole_occluders(hits):
    """Per instance: the number of rays that it alone occludes."""
    alone = hits.sum(0) == 1
    return [int((hits[k] & alone).sum()) for k in range(len(hits))]


@pytest.fixture(scope="module")
def wo(small_scene, small_host, small_default_host):
    """A context of this module's own (default options) with the small scene as both builders make it, and the module's base ray set."""
    ctx = ra.Context(device=0)
    trees = {}
    for name, host in (("reference builder", small_host), ("quality tree", small_default_host)):
        trees[name] = dict(blobs=host.blobs(), scene=ctx.upload_scene(host.nodes, host.pairs, host.remap))
    prim, _ = synth.primary_rays(small_scene["camera"], 256, 256)
    base = np.ascontiguousarray(np.concatenate([synth.random_rays(65536, 7), prim])[::4])
    assert len(base) == 32768
    yield dict(ctx=ctx, trees=trees, sc=small_scene, rays=base, scene=trees["reference builder"]["scene"], blobs=trees["reference builder"]["blobs"])
    for t in trees.values():
        t["scene"].destroy()
    ctx.destroy()


def overlapping_transforms(sc):
    """The five transforms of tests/test_gpu_world.py: rotations, a non-uniform scale, a mirror, translated by less than the scene's
    extent, so the instances overlap in depth."""
    v = sc["vertices"][:, :3]
    ext = float((v.max(0) - v.min(0)).max())
    return [affine(),
            affine(rotation([0, 1, 0], 30.0), translation=(0.15 * ext, 0.05 * ext, -0.1 * ext)),
            affine(rotation([1, 2, 0.5], 75.0), scale=(1.2, 0.7, 0.9), translation=(-0.2 * ext, 0.1 * ext, 0.1 * ext)),
            affine(scale=(-1.0, 1.0, 1.0), translation=(0.05 * ext, -0.04 * ext, 0.12 * ext)),      # a mirror
            affine(rotation([0.3, -1, 0.2], 200.0), scale=(0.8, 0.8, 0.8), translation=(0.1 * ext, 0.02 * ext, 0.2 * ext))]


@pytest.fixture(scope="module")
def five(wo):
    """Test 2's world: five overlapping instances of the small scene (reference builder's tree), with its expectation (computed once)."""
    transforms = overlapping_transforms(wo["sc"])
    world = wo["ctx"].create_world([(m, wo["scene"]) for m in transforms])
    want, res, hits = expectation(transforms, [wo["blobs"]] * 5, wo["rays"])
    want.setflags(write=False)
    yield dict(world=world, transforms=transforms, want=want, res=res, hits=hits)
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("tree", ["reference builder", "quality tree"])
def test_identity(wo, tree):
    ctx, t, rays = wo["ctx"], wo["trees"][tree], wo["rays"]
    world = ctx.create_world([(IDENTITY, t["scene"])])
    got = host_path(world, rays, "identity, %s" % tree)
    plain = ctx.occluded(t["scene"], rays)
    assert np.array_equal(got, plain), "identity instance against Context.occluded, %s: %d rays differ" % (tree, (got != plain).sum())
    assert_exact(got, reported_by_intersect(world, rays), "identity instance against World.intersect, %s" % tree)
    assert_exact(device_path(ctx, world, rays, what="identity, %s" % tree), plain, "identity, %s (device path)" % tree)
    print("identity, %s: occluded fraction %.3f" % (tree, got.mean()))
    assert 0.1 <= got.mean() <= 0.9
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. overlapping instances
def test_five_overlapping_instances(wo, five):
    want, hits = five["want"], five["hits"]
    several = int((hits.sum(0) >= 2).sum())
    sole = sole_occluders(hits)
    print("five overlapping instances: occluded fraction %.4f, %d rays hit two or more instances, sole occluder per instance %s" % (want.mean(), several, sole))
    assert 0.1 <= want.mean() <= 0.9, "the expected occluded fraction is %.3f" % want.mean()
    assert several >= 1000, "only %d rays hit two or more instances" % several
    assert min(sole) >= 100, "an instance is the sole occluder of fewer than 100 rays: %s — nothing shows that the kernel goes on after a miss and reaches it" % sole
    check_both_paths(wo["ctx"], five["world"], wo["rays"], want, "five overlapping instances")
    assert_exact(reported_by_intersect(five["world"], wo["rays"]), want, "World.intersect's instance != NO_INSTANCE")


# ------------------------------------------------------------------------------------------------------------ 3. intervals
def test_intervals(wo, five):
    ctx, world = wo["ctx"], five["world"]
    sel = np.nonzero(five["want"] == 1)[0]
    base = wo["rays"][sel].copy()
    t = five["res"]["t"][sel]
    args = (five["transforms"], [wo["blobs"]] * 5)
    rays = base.copy()
    rays["maxT"] = np.float32(0.5) * t
    want = expectation(*args, rays)[0]
    assert not want.any()
    check_both_paths(ctx, world, rays, want, "maxT = 0.5 t")
    rays["maxT"] = np.float32(1.5) * t
    want = expectation(*args, rays)[0]
    assert want.all()
    check_both_paths(ctx, world, rays, want, "maxT = 1.5 t")
    rays["maxT"] = t      # closed at maxT, but t is a rounded quotient: both outcomes
    want = expectation(*args, rays)[0]
    print("maxT = t: expected occluded fraction %.4f" % want.mean())
    assert want.any() and not want.all()
    got = device_path(ctx, world, rays, what="maxT = t")
    assert_exact(got, want, "maxT = t")
    assert got.any() and not got.all()
    rays["maxT"] = np.inf
    rays["minT"] = t      # open at minT: the nearest hit may go, whatever lies behind stays
    want = expectation(*args, rays)[0]
    print("minT = t, maxT = inf: expected occluded fraction %.4f" % want.mean())
    check_both_paths(ctx, world, rays, want, "minT = t, maxT = inf")


# ------------------------------------------------------------------------------------------------------------ 4. several scenes
def world_rays(m, rays):
    """Object-space rays carried into world space by the [3,4] transform `m` (float64, then rounded): rays that are known to meet an instance."""
    m = np.asarray(m, np.float64)
    out = rays.copy()
    out["origin"] = (rays["origin"].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    out["dir"] = (rays["dir"].astype(np.float64) @ m[:, :3].T).astype(np.float32)
    return out


def test_several_scenes_with_a_bottom_level_spill(wo):
    ctx = wo["ctx"]
    leaf_blobs, _ = leaf_scene(127)
    book = book_scene()
    book_host = ra.HostScene(book["vertices"], book["indices"])
    blobs = dict(small=wo["blobs"], leaf=leaf_blobs, book=book_host.blobs(), comb=comb_scene(40))
    scenes = dict(small=wo["scene"])
    for k in ("leaf", "book", "comb"):
        scenes[k] = ctx.upload_scene(blobs[k]["nodes"], blobs[k]["pairs"], blobs[k]["remap"])
    inst = [("small", affine()),
            ("leaf", affine(rotation([0, 0, 1], 20.0), scale=(0.2, 2.0, 1.0), translation=(-40.0, 25.0, -30.0))),
            ("book", affine(rotation([1, 1, 0], 50.0), scale=(6.0, 6.0, 6.0), translation=(10.0, 30.0, 5.0))),
            ("comb", affine(rotation([0, 1, 0], 90.0), scale=(0.3, 0.3, 0.3), translation=(-60.0, 20.0, 0.0))),
            ("book", affine(scale=(-4.0, 4.0, 4.0), translation=(-15.0, 28.0, 20.0))),
            ("comb", affine(rotation([1, 0, 0], -90.0), scale=(0.25, 0.25, 0.25), translation=(20.0, 60.0, -20.0)))]
    world = ctx.create_world([(m, scenes[k]) for k, m in inst])
    info = world.info
    assert info["instance_count"] == 6 and info["bottom_spill_levels"] > 0, "comb_scene(40) must force a bottom-level stack spill: %s" % info
    comb_rays = make_rays([[x, y, -10.0] for x in (-20.0, 0.0, 15.0) for y in (-20.0, 0.0, 10.0)] * 8, [[0.0, 0.0, 1.0]] * 72)
    aimed = {"leaf": leaf_rays(127, "row"), "book": book_rays(book), "comb": comb_rays}
    rays = np.concatenate([world_rays(m, aimed[k]) for k, m in inst if k != "small"] + [wo["rays"][::2]])
    rays["maxT"] = np.inf
    want, _, hits = expectation([m for _, m in inst], [blobs[k] for k, _ in inst], rays)
    sole = sole_occluders(hits)
    print("several scenes: %d rays, occluded fraction %.3f, sole occluder per instance %s" % (len(rays), want.mean(), sole))
    assert min(sole) >= 1, "an instance is never the sole occluder: %s" % sole
    check_both_paths(ctx, world, rays, want, "several scenes")
    world.destroy()
    for k in ("leaf", "book", "comb"):
        scenes[k].destroy()


# ------------------------------------------------------------------------------------------------------------ 5. deep top level
def test_deep_top_level_spills_its_stack(wo):
    ctx = wo["ctx"]
    blobs, _ = leaf_scene(1)      # one unit quad at z = 10 (and the helper's lone triangle at x = -20 .. -18, z = 30)
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    n = 4096
    transforms = [affine(translation=(3.0 * i, 0.0, 0.0)) for i in range(n)]
    world = ctx.create_world([(m, scene) for m in transforms])
    info = world.info
    assert info["height"] > info["lds_levels"] and info["spill_levels"] > 0, "the top-level stack must spill: %s" % info
    k = np.arange(96)
    along = make_rays(np.stack([-40.0 + 97.0 * k, 0.25 + 0.005 * k, np.full(96, 5.0)], 1),      # along the row, rising slowly through every box
                      np.stack([np.ones(96), np.zeros(96), 0.002 + 0.0001 * k], 1), max_t=np.inf)
    back = make_rays(np.stack([3.0 * n + 10.0 - 50.0 * k, 0.5 + 0.004 * k, np.full(96, 35.0)], 1),
                     np.stack([-np.ones(96), np.zeros(96), -0.003 - 0.0001 * k], 1), max_t=np.inf)
    i = (np.arange(512) * 37) % n
    across = make_rays(np.stack([3.0 * i + 0.1 + 0.0015 * np.arange(512), np.full(512, 0.5), np.zeros(512)], 1), [[0.0, 0.0, 1.0]] * 512)
    slanted = make_rays(np.stack([3.0 * i + 0.5, np.full(512, 0.5), np.zeros(512)], 1), np.stack([0.3 * np.sin(i), np.zeros(512), np.ones(512)], 1))
    rays = np.concatenate([along, back, across, slanted])
    assert len(rays) == 1216
    want, _, _ = expectation(transforms, [blobs] * n, rays, threads=1)
    print("4096 instances in a row: %s; %d rays, occluded fraction %.3f" % (info, len(rays), want.mean()))
    assert want.any() and not want.all()
    check_both_paths(ctx, world, rays, want, "4096 instances in a row")
    world.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 6. edges
def test_edges(wo, small_host):
    ctx, scene, blobs = wo["ctx"], wo["scene"], wo["blobs"]
    rays = wo["rays"][::4].copy()
    m = overlapping_transforms(wo["sc"])[1]
    world = ctx.create_world([(m, scene), (IDENTITY, scene)])
    args = ([m, IDENTITY], [blobs, blobs])
    want = expectation(*args, rays)[0]
    hit = np.nonzero(want == 1)[0]
    # non-finite rays give 0: NaN, +inf, -inf in every field of rays that are occluded when left alone
    bad = rays[hit[:64]].copy()
    for k in range(64):
        field, comp, value = ("origin", "dir", "minT", "maxT")[k % 4], (k // 4) % 3, (np.nan, np.inf, -np.inf)[(k // 12) % 3]
        if field == "maxT":
            bad[field][k] = np.nan
        elif field == "minT":
            bad[field][k] = value
        else:
            bad[field][k, comp] = value
    assert not expectation(*args, bad)[0].any()
    for got in (device_path(ctx, world, bad, what="non-finite rays"), host_path(world, bad, "non-finite rays")):
        assert len(got) == 64 and not got.any(), "non-finite rays: %s" % got
    # count = 0 succeeds with NULL arrays on both entries and touches nothing
    world.occluded_device(None, None, 0)
    assert ra.load_library().racc_hip_world_occluded(ctx._h, world._h, None, None, 0) == 0
    assert len(device_path(ctx, world, rays[:0], what="count 0")) == 0 and len(host_path(world, rays[:0], "count 0")) == 0
    # NULL arrays with a count are refused
    with pytest.raises(ra.RaccError) as e:
        world.occluded_device(None, None, 5)
    assert e.value.code == -1 and "is NULL" in str(e.value)
    # 1 ray and 65 rays (the refill tail), occluded and not
    for n in (1, 65):
        for pick, what in ((hit[:n], "occluded"), (np.nonzero(want == 0)[0][:n], "free"), (np.arange(n), "mixed")):
            check_both_paths(ctx, world, rays[pick], want[pick], "%d-ray batch, %s" % (n, what))
    world.destroy()
    # the transformed ray overflows for some rays: finite world-space rays with components near the largest float, through inv = 2
    half = affine(scale=(0.5, 0.5, 0.5), translation=(3.0, -2.0, 1.0))
    world = ctx.create_world([(half, scene)])
    plain = world_rays(half, rays[:4096])
    far_o, far_d = plain[:256].copy(), plain[256:512].copy()
    far_o["origin"][np.arange(256), np.arange(256) % 3] = np.where(np.arange(256) % 2 == 0, 3e38, -3e38).astype(np.float32)
    far_d["dir"][np.arange(256), np.arange(256) % 3] = np.where(np.arange(256) % 2 == 0, 3e38, -3e38).astype(np.float32)
    mixed = np.concatenate([plain, far_o, far_d])
    inv = prepare([half], [blobs])["inv"]
    seen = object_rays(inv[0], mixed)
    overflow = ~(np.isfinite(seen["origin"]).all(1) & np.isfinite(seen["dir"]).all(1))
    assert np.isfinite(mixed["origin"]).all() and np.isfinite(mixed["dir"]).all() and (overflow[4096:]).all() and not overflow[:4096].any()
    want2 = expectation([half], [blobs], mixed)[0]
    assert not want2[overflow].any() and 0.1 <= want2[:4096].mean() <= 0.9
    check_both_paths(ctx, world, mixed, want2, "transformed ray overflows")
    assert_exact(reported_by_intersect(world, mixed), want2, "transformed ray overflows: World.intersect")
    # a world of another context is refused
    with ra.Context(device=0) as other:
        lib = ra.load_library()
        d = other.alloc(1024)
        assert lib.racc_hip_world_occluded_device(other._h, world._h, d.ptr, d.ptr, 8, None) == -1
        assert b"another context" in lib.racc_hip_last_error()
        out = np.zeros(8, np.uint8)
        assert lib.racc_hip_world_occluded(other._h, world._h, ra.engine._ptr(rays[:8].copy()), ra.engine._ptr(out), 8) == -1
        assert b"another context" in lib.racc_hip_last_error()
        d.free()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. beside other work
@pytest.mark.parametrize("occlusion_first", [False, True])
def test_beside_chained_closest_hit_batches(wo, five, small_host, occlusion_first):
    batches = [synth.random_rays(65536, 7), synth.random_rays(65536, 21), synth.random_rays(65536, 22)]
    refs = [orc.traverse(wo["blobs"], r, threads=16) for r in batches]
    with ra.Context(device=0, chain_min_rays=1) as ctx:
        scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
        world = ctx.create_world([(m, scene) for m in five["transforms"]])
        st = ctx.create_stream()
        d_rays, d_res = [], []
        for r in batches:
            d_rays.append(ctx.alloc(len(r) * 32)); d_rays[-1].upload(r)
            d_res.append(ctx.alloc(len(r) * 16))

        def chain():
            for dr, do, r in zip(d_rays, d_res, batches):
                ctx.intersect_device(scene, None, dr.ptr, do.ptr, len(r), lane=ra.LANE_AUTO)

        if occlusion_first:
            launch = issue(ctx, world, wo["rays"], st)
            chain()
        else:
            chain()
            launch = issue(ctx, world, wo["rays"], st)
        ctx.stream_synchronize(st)
        ctx.wait(ra.LANE_AUTO)
        for k, (do, r, ref) in enumerate(zip(d_res, batches, refs)):
            assert_bit_exact(do.download(orc.RESULT_DTYPE, len(r)), ref, "chained closest-hit batch %d beside a world occlusion launch" % k)
        assert_exact(collect(launch, "beside the chain"), five["want"], "world occlusion launch beside three chained batches")
        for b in d_rays + d_res:
            b.free()
        ctx.destroy_stream(st)
        world.destroy()
        scene.destroy()


def test_two_launches_on_two_streams(wo, five):
    ctx, world = wo["ctx"], five["world"]
    a, b = wo["rays"][:16384], wo["rays"][16384:]
    want_a, want_b = five["want"][:16384], five["want"][16384:]
    assert not np.array_equal(want_a, want_b)
    s1, s2 = ctx.create_stream(), ctx.create_stream()
    la, lb = issue(ctx, world, a, s1), issue(ctx, world, b, s2)      # back to back, nothing waited for in between
    ctx.stream_synchronize(s1); ctx.stream_synchronize(s2)
    assert_exact(collect(la, "stream 1"), want_a, "two streams, launch 1")
    assert_exact(collect(lb, "stream 2"), want_b, "two streams, launch 2")
    ctx.destroy_stream(s1); ctx.destroy_stream(s2)


# ------------------------------------------------------------------------------------------------------------ 8. update
def test_after_world_update(wo, five):
    ctx, blobs, rays = wo["ctx"], wo["blobs"], wo["rays"]
    world = ctx.create_world([(m, wo["scene"]) for m in five["transforms"]])
    moved = [affine(rotation([0, 1, 0], 10.0 * k), translation=(4.0 * k, 1.0 * k, -3.0 * k)) @ np.vstack([m, [0, 0, 0, 1]]).astype(np.float64) for k, m in enumerate(five["transforms"])]
    moved = [np.asarray(m[:3], np.float32) for m in moved]
    world.update(moved)
    want = expectation(moved, [blobs] * 5, rays)[0]
    changed = (want != five["want"]).mean()
    print("after World.update: the expectation differs from the first one at %.2f %% of the rays" % (100.0 * changed))
    assert changed > 0.01, "the update must change the answer for the test to mean anything"
    check_both_paths(ctx, world, rays, want, "after World.update")
    world.update(five["transforms"])
    check_both_paths(ctx, world, rays, five["want"], "updated back to the first transforms")
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 9. nothing left behind
def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the engine itself is linked against (as tests/test_gpu_world.py)."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_nothing_left_behind(wo, five, small_host):
    rays = wo["rays"]
    start = _free_device_memory()
    ctx = ra.Context(device=0)
    scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    world = ctx.create_world([(m, scene) for m in five["transforms"]])
    st = ctx.create_stream()
    for _launch in range(5):
        assert_exact(device_path(ctx, world, rays, st, "memory test"), five["want"], "memory test")
    ctx.destroy_stream(st)
    world.destroy()
    scene.destroy()
    ctx.destroy()
    end = _free_device_memory()
    print("free device memory: %d bytes before the context, %d after Context.destroy (difference %d)" % (start, end, start - end))
    assert abs(start - end) <= 8 << 20


# ------------------------------------------------------------------------------------------------------------ 10. tunables
_TUNABLES_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import rayaccel_amd as ra
d = np.load(sys.argv[2])
with ra.Context(device=0) as ctx:
    scene = ctx.upload_scene(d["nodes"], d["pairs"], d["remap"])
    world = ctx.create_world([(m, scene) for m in d["transforms"]])
    got = world.occluded(d["rays"])
    world.destroy()
    scene.destroy()
np.savez(sys.argv[3], occluded=got)
"""


def test_tunables_do_not_change_results(tmp_path, wo, five, small_host):
    """RACC_WOCC_* are read once per process, hence a child (started fresh): one workgroup per CU, a refill only when the whole wave is
    idle and a pair step as soon as one lane waits return the same bytes for test 2's rays."""
    inputs, outputs = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inputs, nodes=small_host.nodes, pairs=small_host.pairs, remap=small_host.remap, transforms=np.array(five["transforms"], np.float32), rays=wo["rays"])
    p = subprocess.run([sys.executable, "-c", _TUNABLES_CHILD, ROOT, inputs, outputs], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, RACC_WOCC_WAVES="1", RACC_WOCC_REFILL="64", RACC_WOCC_LEAF="1"))
    assert p.returncode == 0, p.stderr[-2000:]
    got = np.load(outputs)["occluded"]
    assert got.dtype == np.uint8
    assert_exact(got, five["want"], "RACC_WOCC_WAVES=1 RACC_WOCC_REFILL=64 RACC_WOCC_LEAF=1")
    assert_exact(got, host_path(five["world"], wo["rays"], "this process"), "the child against this process's defaults")
