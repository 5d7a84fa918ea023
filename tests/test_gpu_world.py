"""Instancing — racc_hip_world_* / worldIntersectKernel (rayaccel_amd/csrc/racc_world.inc).

The bar, in every test but the last: bit-exact on triangle, t, u, v and the instance index against the composed expectation of
world_helpers.compose — the specification's ray transform in numpy.float32 with the library's own `inv`, orc.traverse per instance with
the ray's own maxT, smallest t, then lowest instance index.  Every device output carries guard records behind `count`, which must come
back untouched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, assert_bit_exact, assert_matches_arbiter, book_rays, book_scene, comb_scene, leaf_rays, leaf_scene, make_rays
from refit_helpers import displaced
from world_helpers import IDENTITY, NO_INSTANCE, affine, assert_world_exact, compose, rotation

pytestmark = pytest.mark.gpu

GUARD = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prepare(transforms, blobs_list):
    return ra.host_world_prepare(np.array(transforms, np.float32), np.array([ra.root_box(b["nodes"]) for b in blobs_list]))


def issue(ctx, world, rays, stream=None):
    n = len(rays)
    d_r, d_o, d_i = ctx.alloc(max(n, 1) * 32), ctx.alloc((n + GUARD) * 16), ctx.alloc((n + GUARD) * 4)
    if n:
        d_r.upload(rays)
    d_o.upload(np.full((n + GUARD) * 4, 0xABABABAB, np.uint32))
    d_i.upload(np.full(n + GUARD, 0xCDCDCDCD, np.uint32))
    world.intersect_device(d_r.ptr, d_o.ptr, d_i.ptr, n, stream=stream)
    return d_r, d_o, d_i, n


def collect(launch, what=""):
    d_r, d_o, d_i, n = launch
    res = d_o.download(np.uint32, (n + GUARD) * 4)
    inst = d_i.download(np.uint32, n + GUARD)
    for b in (d_r, d_o, d_i):
        b.free()
    assert (res[n * 4:] == 0xABABABAB).all() and (inst[n:] == 0xCDCDCDCD).all(), "%s: guard records behind the outputs were written" % what
    return res[:n * 4].copy().view(synth.RESULT_DTYPE), inst[:n].copy()


def device_path(ctx, world, rays, stream=None, what=""):
    launch = issue(ctx, world, rays, stream)
    ctx.stream_synchronize(stream)
    return collect(launch, what)


def check_world(ctx, world, transforms, blobs_list, rays, what, threads=16, host_too=True):
    """Device path (and host path) of `world` against the composed expectation; returns (expected results, instances, per-instance hits)."""
    w = prepare(transforms, blobs_list)
    want, want_inst, hits = compose(w["inv"], blobs_list, rays, threads=threads)
    got, got_inst = device_path(ctx, world, rays, what=what)
    assert_world_exact(got, got_inst, want, want_inst, what + " (device path)")
    if host_too:
        got, got_inst = world.intersect(rays)
        assert_world_exact(got, got_inst, want, want_inst, what + " (host path)")
    return want, want_inst, hits


@pytest.fixture(scope="module")
def wd(small_scene, small_host, small_default_host):
    """A context of this module's own (default options) with the small scene as both builders make it, and the module's ray set."""
    ctx = ra.Context(device=0)
    trees = {}
    for name, host in (("reference builder", small_host), ("quality tree", small_default_host)):
        trees[name] = dict(blobs=host.blobs(), scene=ctx.upload_scene(host.nodes, host.pairs, host.remap))
    prim, _ = synth.primary_rays(small_scene["camera"], 256, 256)
    yield dict(ctx=ctx, trees=trees, sc=small_scene, rays=np.concatenate([synth.random_rays(65536, 7), prim]),
               scene=trees["reference builder"]["scene"], blobs=trees["reference builder"]["blobs"])
    for t in trees.values():
        t["scene"].destroy()
    ctx.destroy()


def overlapping_transforms(sc):
    """Five general affine transforms of the small scene — rotations, a non-uniform scale, a mirror — translated by less than the scene's
    extent, so the instances overlap in depth; every coordinate stays at the scene's own magnitude."""
    v = sc["vertices"][:, :3]
    ext = float((v.max(0) - v.min(0)).max())
    return [affine(),
            affine(rotation([0, 1, 0], 30.0), translation=(0.15 * ext, 0.05 * ext, -0.1 * ext)),
            affine(rotation([1, 2, 0.5], 75.0), scale=(1.2, 0.7, 0.9), translation=(-0.2 * ext, 0.1 * ext, 0.1 * ext)),
            affine(scale=(-1.0, 1.0, 1.0), translation=(0.05 * ext, -0.04 * ext, 0.12 * ext)),      # a mirror
            affine(rotation([0.3, -1, 0.2], 200.0), scale=(0.8, 0.8, 0.8), translation=(0.1 * ext, 0.02 * ext, 0.2 * ext))]


@pytest.fixture(scope="module")
def five(wd):
    """Test 2's world: five overlapping instances of the small scene (reference builder's tree), with its expectation."""
    ctx, blobs = wd["ctx"], wd["blobs"]
    transforms = overlapping_transforms(wd["sc"])
    world = ctx.create_world([(m, wd["scene"]) for m in transforms])
    w = prepare(transforms, [blobs] * 5)
    want, want_inst, hits = compose(w["inv"], [blobs] * 5, wd["rays"])
    yield dict(world=world, transforms=transforms, want=want, want_inst=want_inst, hits=hits, inv=w["inv"])
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("tree", ["reference builder", "quality tree"])
def test_identity(wd, tree):
    ctx, t, rays = wd["ctx"], wd["trees"][tree], wd["rays"]
    world = ctx.create_world([(IDENTITY, t["scene"])])
    info = world.info
    assert info["instance_count"] == 1 and info["node_count"] == 1 and info["height"] == 1 and info["device_bytes"] == 148
    want, want_inst, _ = check_world(ctx, world, [IDENTITY], [t["blobs"]], rays, "identity, %s" % tree)
    got, got_inst = world.intersect(rays)
    plain = ctx.intersect(t["scene"], None, rays)
    assert_bit_exact(got, plain, "identity instance against Context.intersect, %s" % tree)
    hit = plain["triangle"] != MISS
    assert 0.1 <= hit.mean() <= 0.9
    assert (got_inst[hit] == 0).all() and (got_inst[~hit] == NO_INSTANCE).all()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. overlapping instances
def test_overlapping_instances_of_one_scene(wd, five):
    frac = (five["want"]["triangle"] != MISS).mean()
    several = int((five["hits"].sum(0) >= 2).sum())
    print("five overlapping instances: composed hit fraction %.3f, %d rays hit two or more instances, winners per instance %s" % (
        frac, several, np.bincount(five["want_inst"][five["want_inst"] != NO_INSTANCE], minlength=5).tolist()))
    assert 0.1 <= frac <= 0.9, "the composed hit fraction is %.3f" % frac
    assert several >= 1000, "only %d rays hit two or more instances: the min logic is untested" % several
    assert len(wd["rays"]) == 65536 + 256 * 256
    got, got_inst = device_path(wd["ctx"], five["world"], wd["rays"], what="five instances")
    assert_world_exact(got, got_inst, five["want"], five["want_inst"], "five overlapping instances (device path)")
    got, got_inst = five["world"].intersect(wd["rays"])
    assert_world_exact(got, got_inst, five["want"], five["want_inst"], "five overlapping instances (host path)")


# ------------------------------------------------------------------------------------------------------------ 3. several scenes
def world_rays(m, rays):
    """Object-space rays carried into world space by the [3,4] transform `m` (float64, then rounded): rays that are known to meet an instance."""
    m = np.asarray(m, np.float64)
    out = rays.copy()
    out["origin"] = (rays["origin"].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    out["dir"] = (rays["dir"].astype(np.float64) @ m[:, :3].T).astype(np.float32)
    return out


def test_several_scenes_in_one_world(wd):
    ctx = wd["ctx"]
    leaf_blobs, _ = leaf_scene(127)
    book = book_scene()
    book_host = ra.HostScene(book["vertices"], book["indices"])
    comb = comb_scene(40)
    blobs = dict(small=wd["blobs"], leaf=leaf_blobs, book=book_host.blobs(), comb=comb)
    scenes = dict(small=wd["scene"])
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
    rays = np.concatenate([wd["rays"][::8]] + [world_rays(m, aimed[k]) for k, m in inst if k != "small"])
    rays["maxT"] = np.inf
    want, want_inst, hits = check_world(ctx, world, [m for _, m in inst], [blobs[k] for k, _ in inst], rays, "several scenes")
    winners = np.bincount(want_inst[want_inst != NO_INSTANCE], minlength=6)
    print("several scenes: %d rays, winners per instance %s" % (len(rays), winners.tolist()))
    assert (winners > 0).all(), "an instance never wins a ray: %s" % winners
    world.destroy()
    for k in ("leaf", "book", "comb"):
        scenes[k].destroy()


# ------------------------------------------------------------------------------------------------------------ 4. ties
def test_ties_go_to_the_lowest_index(wd):
    ctx, rays = wd["ctx"], wd["rays"][::4]
    m = overlapping_transforms(wd["sc"])[2]
    a, b = wd["trees"]["reference builder"], wd["trees"]["quality tree"]
    single = ctx.create_world([(m, a["scene"])])
    one, _ = single.intersect(rays)
    single.destroy()
    hit = one["triangle"] != MISS
    assert hit.sum() > 1000
    a2 = dict(blobs=a["blobs"], scene=ctx.upload_scene(a["blobs"]["nodes"], a["blobs"]["pairs"], a["blobs"]["remap"]))      # the same blobs, a second upload
    # identical transforms: one scene twice, two uploads of it in both orders, and two trees over the same triangles in both orders
    for order in ((a, a), (a, a2), (a2, a), (a, b), (b, a)):
        world = ctx.create_world([(m, order[0]["scene"]), (m, order[1]["scene"])])
        want, want_inst, hits = check_world(ctx, world, [m, m], [order[0]["blobs"], order[1]["blobs"]], rays, "two coincident instances", host_too=False)
        got, got_inst = world.intersect(rays)
        world.destroy()
        if order[0]["blobs"] is order[1]["blobs"]:
            assert (hits[0] == hits[1]).all() and (got_inst[hit] == 0).all() and (got_inst[~hit] == NO_INSTANCE).all(), "identical instances: every hit reports index 0"
            assert_bit_exact(got, one, "identical instances against the single one")
        else:
            assert (hits[0] & hits[1]).sum() > 1000
    a2["scene"].destroy()


# ------------------------------------------------------------------------------------------------------------ 5. deep top level
def test_deep_top_level_spills_its_stack(wd):
    ctx = wd["ctx"]
    blobs, _ = leaf_scene(1)      # one unit quad at z = 10 (and the helper's lone triangle at x = -20 .. -18, z = 30)
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    n = 4096
    transforms = [affine(translation=(3.0 * i, 0.0, 0.0)) for i in range(n)]
    world = ctx.create_world([(m, scene) for m in transforms])
    info = world.info
    print("4096 instances in a row: %s" % info)
    assert info["height"] > info["lds_levels"] and info["spill_levels"] > 0, "the top-level stack must spill: %s" % info
    assert info["node_count"] == n - 1 and info["device_bytes"] == 148 * n - 64
    k = np.arange(96)
    along = make_rays(np.stack([-40.0 + 97.0 * k, 0.25 + 0.005 * k, np.full(96, 5.0)], 1),      # along the row, rising slowly through every box
                      np.stack([np.ones(96), np.zeros(96), 0.002 + 0.0001 * k], 1), max_t=np.inf)
    back = make_rays(np.stack([3.0 * n + 10.0 - 50.0 * k, 0.5 + 0.004 * k, np.full(96, 35.0)], 1),
                     np.stack([-np.ones(96), np.zeros(96), -0.003 - 0.0001 * k], 1), max_t=np.inf)
    i = (np.arange(512) * 37) % n
    across = make_rays(np.stack([3.0 * i + 0.1 + 0.0015 * np.arange(512), np.full(512, 0.5), np.zeros(512)], 1), [[0.0, 0.0, 1.0]] * 512)
    slanted = make_rays(np.stack([3.0 * i + 0.5, np.full(512, 0.5), np.zeros(512)], 1), np.stack([0.3 * np.sin(i), np.zeros(512), np.ones(512)], 1))
    rays = np.concatenate([along, back, across, slanted])
    want, want_inst, hits = check_world(ctx, world, transforms, [blobs] * n, rays, "4096 instances in a row", threads=1)
    print("row: %d rays, %d hits, %d distinct winners, up to %d instances hit by one ray" % (len(rays), (want_inst != NO_INSTANCE).sum(), len(np.unique(want_inst)), hits.sum(0).max()))
    assert (want_inst[192:704] == i).all(), "the rays across the row hit the quad they start under"
    assert (want_inst[:192] != NO_INSTANCE).sum() > 96, "the rays along the row hit something"
    world.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 6. edges
def test_edges(wd):
    ctx, scene, blobs = wd["ctx"], wd["scene"], wd["blobs"]
    rays = wd["rays"][::16].copy()
    plain = ctx.intersect(scene, None, rays)
    hit = np.nonzero(plain["triangle"] != MISS)[0]
    # a uniform scale by 2: origin and direction doubled are exact, inv = 0.5 exact, so the object-space ray is the plain one and t is unchanged
    double = ctx.create_world([(affine(scale=(2.0, 2.0, 2.0)), scene)])
    scaled = rays.copy()
    scaled["origin"] *= np.float32(2); scaled["dir"] *= np.float32(2)
    got, got_inst = double.intersect(scaled)
    assert_bit_exact(got, plain, "uniform scale by 2: t unchanged")
    double.destroy()

    m = overlapping_transforms(wd["sc"])[1]
    world = ctx.create_world([(m, scene), (IDENTITY, scene)])
    args = ([m, IDENTITY], [blobs, blobs])
    want, _, _ = check_world(ctx, world, *args, rays, "edges: plain")
    # clipping: the composed hits again with maxT = 0.5 t / t / 1.5 t and minT = 0 / t / 0.5 t in rotation
    h = np.nonzero(want["triangle"] != MISS)[0]
    again = rays[h].copy()
    t, cls = want["t"][h], np.arange(len(h)) % 3
    again["maxT"] = np.where(cls == 0, np.float32(0.5) * t, np.where(cls == 1, t, np.float32(1.5) * t)).astype(np.float32)
    w2, i2, _ = check_world(ctx, world, *args, again, "edges: maxT = 0.5 t / t / 1.5 t")
    assert (w2["t"][w2["triangle"] != MISS] <= again["maxT"][w2["triangle"] != MISS]).all()
    again["maxT"] = np.inf
    again["minT"] = np.where(cls == 0, np.float32(0), np.where(cls == 1, t, np.float32(0.5) * t)).astype(np.float32)
    w3, i3, _ = check_world(ctx, world, *args, again, "edges: minT = 0 / t / 0.5 t")
    changed = (w3["triangle"] == MISS) | (w3["t"].view(np.uint32) != t.view(np.uint32))
    print("minT = t: %d of %d hits are clipped away (the interval is open at minT; t is a rounded quotient, so not all)" % (changed[cls == 1].sum(), (cls == 1).sum()))
    assert changed[cls == 1].any() and not changed[cls == 0].any() and not changed[cls == 2].any()      # (minT = 0.5 t leaves the hit at t in reach)
    # non-finite rays miss
    bad = rays[hit[:64]].copy()
    for k in range(64):
        field, comp, value = ("origin", "dir", "minT", "maxT")[k % 4], (k // 4) % 3, (np.nan, np.inf, -np.inf)[(k // 12) % 3]
        if field == "maxT":
            bad[field][k] = np.nan
        elif field == "minT":
            bad[field][k] = value
        else:
            bad[field][k, comp] = value
    got, got_inst = device_path(ctx, world, bad, what="non-finite rays")
    assert (got["triangle"] == MISS).all() and (got_inst == NO_INSTANCE).all() and (got["t"] == 0).all() and (got["u"] == 0).all() and (got["v"] == 0).all()
    check_world(ctx, world, *args, bad, "non-finite rays")
    # count = 0 succeeds; 1 ray and 65 rays (the refill tail)
    world.intersect_device(None, None, None, 0)
    r0, i0 = world.intersect(rays[:0])
    assert len(r0) == 0 and len(i0) == 0
    for n in (1, 65):
        check_world(ctx, world, *args, rays[hit[:n]], "%d-ray batch" % n)
    world.destroy()


def test_create_refusals(wd, small_host):
    ctx, scene = wd["ctx"], wd["scene"]
    with pytest.raises(ra.RaccError) as e:
        ctx.create_world([])
    assert e.value.code == -1 and "count is 0" in str(e.value)
    singular = IDENTITY.copy(); singular[2, :3] = 0
    with pytest.raises(ra.RaccError) as e:
        ctx.create_world([(IDENTITY, scene), (singular, scene)])
    assert e.value.code == -1 and "singular" in str(e.value)
    with ra.Context(device=0) as other:
        foreign = other.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
        with pytest.raises(ra.RaccError) as e:
            ctx.create_world([(IDENTITY, scene), (IDENTITY, foreign)])
        assert e.value.code == -1 and "this context" in str(e.value)
        foreign.destroy()
    world = ctx.create_world([(IDENTITY, scene), (IDENTITY, scene)])
    with pytest.raises(ra.RaccError) as e:
        world.update([IDENTITY])
    assert "count differs" in str(e.value)
    nan = IDENTITY.copy(); nan[0, 3] = np.nan
    with pytest.raises(ra.RaccError):
        world.update([IDENTITY, nan])
    got, got_inst = world.intersect(wd["rays"][:4096])      # the refused update left the world as it was
    assert_bit_exact(got, ctx.intersect(scene, None, wd["rays"][:4096]), "after a refused update")
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. update
def test_update_with_new_transforms(wd, five):
    ctx, blobs, rays = wd["ctx"], wd["blobs"], wd["rays"][::4]
    world = ctx.create_world([(m, wd["scene"]) for m in five["transforms"]])
    moved = [affine(rotation([0, 1, 0], 10.0 * k), translation=(4.0 * k, 1.0 * k, -3.0 * k)) @ np.vstack([m, [0, 0, 0, 1]]).astype(np.float64) for k, m in enumerate(five["transforms"])]
    moved = [np.asarray(m[:3], np.float32) for m in moved]
    world.update(moved)
    want, want_inst, _ = check_world(ctx, world, moved, [blobs] * 5, rays, "after World.update")
    base = five["want"][::4]
    assert (want["t"].view(np.uint32) != base["t"].view(np.uint32)).mean() > 0.1, "the update must change the answer for the test to mean anything"
    world.update(five["transforms"])
    got, got_inst = world.intersect(rays)
    assert_world_exact(got, got_inst, base, five["want_inst"][::4], "updated back to the first transforms")
    world.destroy()


def test_update_after_a_member_scene_was_refitted(wd, small_host):
    ctx, sc, rays = wd["ctx"], wd["sc"], wd["rays"][::4]
    scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
    transforms = overlapping_transforms(sc)[:3]
    world = ctx.create_world([(m, scene) for m in transforms])
    v = displaced(sc["vertices"], 11.0, phase=0.3)      # moves the root box as well
    blobs = ra.host_refit(small_host.blobs(), v, sc["indices"])
    assert not np.array_equal(ra.root_box(blobs["nodes"]), ra.root_box(small_host.nodes))
    refit.refit(v)
    world.update(transforms)
    check_world(ctx, world, transforms, [blobs] * 3, rays, "member scene refitted, then World.update")
    world.destroy()
    refit.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ the scene registry
def test_registry_survives_frees_in_between(wd, small_host, small_default_host):
    """Refit and instancing look a scene up in one registry (racc_scene_registry.inc): uploads, frees and both lookups interleaved on one
    context, then the refitted scene C — traced plainly and as a world — against the host refit's blobs uploaded fresh."""
    ctx, sc, rays = wd["ctx"], wd["sc"], wd["rays"][:4096]
    a = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    b = ctx.upload_scene(small_default_host.nodes, small_default_host.pairs, small_default_host.remap)
    c = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    b.destroy()
    refit = ctx.create_refit(c, sc["indices"], len(sc["vertices"]))
    transforms = overlapping_transforms(sc)[:2]
    world = ctx.create_world([(transforms[0], a), (transforms[1], c)])
    check_world(ctx, world, transforms, [small_host.blobs()] * 2, rays, "world of (A, C) after B was freed", host_too=False)
    world.destroy()
    a.destroy()
    v = displaced(sc["vertices"], 3.0, phase=0.2)
    refit.refit(v)
    blobs = ra.host_refit(small_host.blobs(), v, sc["indices"])
    fresh = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    want = ctx.intersect(fresh, None, rays)
    assert (want["t"].view(np.uint32) != ctx.intersect(wd["scene"], None, rays)["t"].view(np.uint32)).any(), "the refit must change the answer for the test to mean anything"
    assert_bit_exact(ctx.intersect(c, None, rays), want, "C refitted after A and B were freed, against the host refit uploaded fresh")
    world = ctx.create_world([(IDENTITY, c)])
    got, got_inst = world.intersect(rays)
    assert_bit_exact(got, want, "world of C, against the host refit uploaded fresh")
    assert np.array_equal(got_inst, np.where(want["triangle"] != MISS, 0, NO_INSTANCE).astype(np.uint32))
    world.destroy()      # the documented order: a world before its scenes, a refit handle before its scene
    refit.destroy()
    fresh.destroy()
    c.destroy()


_NO_TOPOLOGY_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import rayaccel_amd as ra
d = np.load(sys.argv[2])
with ra.Context(device=0) as ctx:
    scene = ctx.upload_scene(d["nodes"], d["pairs"], d["remap"])
    try:
        ctx.create_refit(scene, d["indices"], int(d["vertex_count"])).destroy()
        refusal = ""
    except ra.RaccError as e:
        refusal = str(e)
    plain = ctx.intersect(scene, None, d["rays"])
    world = ctx.create_world([(np.eye(3, 4, dtype=np.float32), scene)])
    got, inst = world.intersect(d["rays"])
    world.destroy()
    scene.destroy()
np.savez(sys.argv[3], refusal=refusal, plain=plain, world=got, inst=inst)
"""


def test_without_kept_topology_only_refit_is_refused(tmp_path, wd, small_host):
    """RACC_REFIT_TOPOLOGY=0 is read once per process, hence a child: create_refit is refused, the scene still traces and still becomes an
    instance (its owner is registered all the same), with this process's records."""
    ctx, sc, rays = wd["ctx"], wd["sc"], wd["rays"][:4096]
    inputs, outputs = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inputs, nodes=small_host.nodes, pairs=small_host.pairs, remap=small_host.remap, indices=sc["indices"], vertex_count=len(sc["vertices"]), rays=rays)
    p = subprocess.run([sys.executable, "-c", _NO_TOPOLOGY_CHILD, ROOT, inputs, outputs], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, RACC_REFIT_TOPOLOGY="0"))
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.load(outputs)
    assert "topology words" in str(out["refusal"]), "create_refit under RACC_REFIT_TOPOLOGY=0: %r" % str(out["refusal"])
    want = ctx.intersect(wd["scene"], None, rays)
    assert 0 < (want["triangle"] != MISS).sum() < len(rays)      # hits and misses
    assert_bit_exact(out["plain"].view(synth.RESULT_DTYPE), want, "intersect under RACC_REFIT_TOPOLOGY=0")
    world = ctx.create_world([(IDENTITY, wd["scene"])])
    got, got_inst = world.intersect(rays)
    world.destroy()
    assert_bit_exact(out["world"].view(synth.RESULT_DTYPE), got, "world of one instance under RACC_REFIT_TOPOLOGY=0")
    assert np.array_equal(out["inst"], got_inst)


@pytest.mark.parametrize("world_first", [False, True])
def test_beside_chained_closest_hit_batches(wd, five, small_host, world_first):
    batches = [wd["rays"][:65536], synth.random_rays(65536, 21), synth.random_rays(65536, 22)]
    refs = [orc.traverse(wd["blobs"], r, threads=16) for r in batches]
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

        if world_first:
            launch = issue(ctx, world, wd["rays"], st)
            chain()
        else:
            chain()
            launch = issue(ctx, world, wd["rays"], st)
        ctx.stream_synchronize(st)
        ctx.wait(ra.LANE_AUTO)
        for k, (do, r, ref) in enumerate(zip(d_res, batches, refs)):
            assert_bit_exact(do.download(orc.RESULT_DTYPE, len(r)), ref, "chained closest-hit batch %d beside a world launch" % k)
        got, got_inst = collect(launch, "beside the chain")
        assert_world_exact(got, got_inst, five["want"], five["want_inst"], "world launch beside three chained batches")
        for b in d_rays + d_res:
            b.free()
        ctx.destroy_stream(st)
        world.destroy()
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 8. memory
def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the engine itself is linked against (as tests/test_gpu_refit.py)."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_destroy_gives_the_memory_back(wd):
    """A world large enough to be seen in hipMemGetInfo (148 B per instance: 2^18 instances hold 37 MB): what create + launches took comes
    back at World.destroy but for an eighth (allocation granularity), and after Context.destroy nothing of either is left."""
    blobs, _ = leaf_scene(1)
    rays = wd["rays"][:4096]
    start = _free_device_memory()
    ctx = ra.Context(device=0)
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    st = ctx.create_stream()
    n = 1 << 18
    t = np.tile(IDENTITY.reshape(1, 12), (n, 1))
    t[:, 3] = 3.0 * (np.arange(n) % 512); t[:, 11] = 3.0 * (np.arange(n) // 512)
    before = _free_device_memory()
    world = ctx.create_world([(m, scene) for m in t])
    for _launch in range(5):
        launch = issue(ctx, world, rays, st)
        ctx.stream_synchronize(st)
        collect(launch, "memory test")
    held = before - _free_device_memory()
    assert world.info["device_bytes"] == 148 * n - 64
    world.destroy()
    after = _free_device_memory()
    print("world of 2^18 instances: %d bytes of device memory held, %d not returned by destroy" % (held, before - after))
    assert held >= 32 << 20, "the world holds %d bytes: too little for this test to see" % held
    assert abs(before - after) <= held // 8
    ctx.destroy_stream(st)
    scene.destroy()
    ctx.destroy()
    end = _free_device_memory()
    print("free device memory: %d bytes before the context, %d after Context.destroy (difference %d)" % (start, end, start - end))
    assert abs(start - end) <= 8 << 20


# ------------------------------------------------------------------------------------------------------------ 9. geometry cross-check
def test_geometry_cross_check_against_the_flattened_scene(wd, five):
    """Independent of the ray-transform rule: every instance's vertices carried into world space in double, one flat triangle list
    (triangle id = instance * T + triangle), the double-precision brute force over all of it.  Every 16th ray of test 2's set (the brute
    force is O(rays x triangles)).  tests/helpers.py::assert_matches_arbiter's rule: same hit/miss except where the arbiter's hit grazes an
    edge, same (instance, triangle) except at exact-distance ties, t within 1e-4 relative."""
    import threading
    sc = wd["sc"]
    v, idx = sc["vertices"][:, :3].astype(np.float64), sc["indices"]
    T = len(idx)
    flat_v, flat_i = [], []
    for k, m in enumerate(five["transforms"]):
        m64 = m.astype(np.float64)
        flat_v.append(v @ m64[:, :3].T + m64[:, 3])
        flat_i.append(idx + k * len(v))
    flat = dict(vertices=np.concatenate([np.concatenate(flat_v).astype(np.float32), np.ones((5 * len(v), 1), np.float32)], 1),
                indices=np.ascontiguousarray(np.concatenate(flat_i).astype(np.uint32)))
    sel = np.arange(0, len(wd["rays"]), 16)
    rays = np.ascontiguousarray(wd["rays"][sel])
    # The rule's tolerance on t is relative (1e-4, no absolute floor).  Both sides round POSITIONS at the coordinates' magnitude — the
    # specification's o' = fl(inv (o, 1)) here, the float32 world-space vertices the arbiter is given there: a few ulp of 100 .. 200, i.e.
    # up to ~1e-4 absolute in t — so a relative 1e-4 can only be asked of hits at t >= ~1: the rays' intervals start at minT = 2 (the random
    # rays start inside the scene, some of them a hair from a surface: with minT = 0 one record of 7,022, a hit at t = 0.006, is off by 6.3e-7
    # absolute = 1.05e-4 relative).  The same rays on both sides; the tolerance itself is the rule's.
    rays["minT"] = 2.0
    want, want_inst, _ = compose(five["inv"], [wd["blobs"]] * 5, rays)
    got, got_inst = five["world"].intersect(rays)
    assert_world_exact(got, got_inst, want, want_inst, "the cross-check's rays")
    res = got.copy()
    hit = got["triangle"] != MISS
    res["triangle"][hit] = got_inst[hit] * np.uint32(T) + got["triangle"][hit]
    # the exception classes, counted before the rule is applied (the brute force in slices on threads: ctypes releases the GIL)
    parts = [None] * 16
    cuts = [len(rays) * k // 16 for k in range(17)]

    def work(k):
        parts[k] = orc.brute_closest(flat["vertices"], flat["indices"], rays[cuts[k]:cuts[k + 1]])

    ts = [threading.Thread(target=work, args=(k,)) for k in range(16)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    tri = np.concatenate([p[0] for p in parts])
    hit_b = tri != MISS
    print("geometry cross-check: %d rays, %d hits; exception classes: %d hit/miss differences (edge grazers), %d other (instance, triangle) at a tie" % (
        len(rays), int(hit.sum()), int((hit != hit_b).sum()), int((hit & hit_b & (res["triangle"] != tri)).sum())))
    assert 0.1 <= hit.mean() <= 0.9
    ties = assert_matches_arbiter(res, flat, rays)
    assert ties <= max(8, len(rays) // 500)
