"""Rebuild of a world's top level on the device — racc_hip_world_rebuild* (rayaccel_amd/csrc/racc_world_rebuild.inc).

Two bars.  The rebuilt world as bytes: World.download() after a device rebuild equals racc_host_world_rebuild (inv, order, the topology
words, the four box fields, ray_pad) and check_rebuild() returns its height.  Its results: byte-equal to a world created with the new
transforms and bit-exact against world_helpers.compose.  Every height relied on here is established by tests/test_world_rebuild_host.py
on the CPU; no test feeds the kernels a tree deeper than the rule's bound.  At most 16k rays per launch."""
import numpy as np
import pytest

import rayaccel_amd as ra
from rayaccel_amd import synth
from refit_helpers import displaced
from test_gpu_world_refit import device_transforms, moved_transforms, overlapping_transforms, trace
from test_world_host import random_world
from world_helpers import NO_INSTANCE, affine, assert_world_exact, compose, rotation
from world_rebuild_helpers import chain_world, common_centre_world, height_bound, walk_height

pytestmark = pytest.mark.gpu

NODE_FIELDS = ("first", "last", "leftMin", "leftMax", "rightMin", "rightMax")


@pytest.fixture(scope="module")
def rw(small_scene, small_host):
    """A context of this module's own with the small scene (reference builder's tree), a stream and the module's 12k rays."""
    ctx = ra.Context(device=0)
    scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    prim, _ = synth.primary_rays(small_scene["camera"], 64, 64)
    st = ctx.create_stream()
    yield dict(ctx=ctx, scene=scene, blobs=small_host.blobs(), sc=small_scene, st=st, rays=np.concatenate([synth.random_rays(8192, 7), prim]),
               root=ra.root_box(small_host.nodes))
    ctx.destroy_stream(st)
    scene.destroy()
    ctx.destroy()


def rebuild_device(rw, handle, transforms):
    """One device rebuild on the module's stream, waited for."""
    d = device_transforms(rw["ctx"], transforms)
    handle.rebuild_device(d.ptr, stream=rw["st"])
    rw["ctx"].stream_synchronize(rw["st"])
    d.free()


def assert_download_is_the_host_rebuild(world, transforms, rb, what):
    want, got = ra.host_world_rebuild(transforms, rb), world.download()
    assert got["inv"].tobytes() == want["inv"].tobytes(), "%s: inv differs from racc_host_world_rebuild" % what
    assert np.array_equal(got["order"], want["order"]), "%s: order differs from racc_host_world_rebuild" % what
    for f in NODE_FIELDS:
        assert got["nodes"][f].tobytes() == want["nodes"][f].tobytes(), "%s: %s differs from racc_host_world_rebuild" % (what, f)
    assert np.float32(got["ray_pad"]).tobytes() == np.float32(want["ray_pad"]).tobytes(), "%s: ray_pad %r, host %r" % (what, got["ray_pad"], want["ray_pad"])
    return want


def grid_transforms(side, pitch):
    t = np.tile(affine(), (side * side, 1, 1))
    t[:, 0, 3] = pitch * (np.arange(side * side) % side)
    t[:, 2, 3] = pitch * (np.arange(side * side) // side)
    return t


def assert_traces_as_a_fresh_world(rw, world, transforms, rays, what, blobs=None, scene=None):
    """intersect_device records and instance indices and occluded_device bytes: byte-equal to a world created with `transforms`, bit-exact
    against compose on the host rule's inverses."""
    n = len(transforms)
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    fresh = rw["ctx"].create_world([(m, scene or rw["scene"]) for m in transforms])
    f, f_inst, f_occ = trace(rw, fresh, rays, rw["st"])
    fresh.destroy()
    assert got.tobytes() == f.tobytes() and got_inst.tobytes() == f_inst.tobytes() and occ.tobytes() == f_occ.tobytes(), "%s: against a world created with the new transforms" % what
    want, want_inst, hits = compose(world.download()["inv"], [blobs or rw["blobs"]] * n, rays)
    assert_world_exact(got, got_inst, want, want_inst, what)
    assert np.array_equal(occ, (want_inst != NO_INSTANCE).astype(np.uint8)), "%s: occluded" % what
    return want_inst, hits


# ------------------------------------------------------------------------------------------------------------ 1. byte parity
def byte_cases():
    cases = [("%d" % n, n) for n in (1, 2, 3, 64, 65, 1000)]
    return cases + [("common-centre", "common"), ("chain", "chain")]


@pytest.mark.parametrize("name,case", byte_cases(), ids=[c[0] for c in byte_cases()])
def test_download_after_a_device_rebuild_is_the_host_rebuild(rw, name, case):
    ctx = rw["ctx"]
    if case == "common":
        built, moved = random_world(1000, 31)[0], [common_centre_world(1000)]
    elif case == "chain":
        built, moved = random_world(31, 32)[0], [chain_world(4096.0)]
    else:      # a world built elsewhere, its instances then permuted and moved — twice on one handle
        built = random_world(case, 1200 + case)[0]
        moved = [moved_transforms(case, seed)[np.random.RandomState(seed).permutation(case)] for seed in (1300 + case, 1400 + case)]
    count = len(built)
    rb = np.tile(rw["root"], (count, 1))
    world = ctx.create_world([(m, rw["scene"]) for m in built])
    handle = world.create_refit(rebuild=True)
    bound = height_bound(count, disabled_possible=True)
    for round_, t in enumerate(moved):
        rebuild_device(rw, handle, t)
        want = assert_download_is_the_host_rebuild(world, t, rb, "%s, rebuild %d" % (name, round_))
        assert handle.check_rebuild() == (want["height"], 0)
        assert want["height"] <= bound and world.info["height"] >= bound and world.info["spill_levels"] >= want["height"] + 1 - world.info["lds_levels"]
        # ... and a refit of the rebuilt tree to the same transforms reproduces it, signs of zeros included
        d = device_transforms(ctx, t)
        handle.refit_device(d.ptr, stream=rw["st"])
        ctx.stream_synchronize(rw["st"])
        d.free()
        assert_download_is_the_host_rebuild(world, t, rb, "%s, refit behind rebuild %d" % (name, round_))
    handle.destroy()
    assert world.info["height"] == want["height"], "destroy sets info.height from the real height"
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. results
def test_results_on_the_five_overlapping_transforms(rw):
    ctx, rays = rw["ctx"], rw["rays"]
    t = overlapping_transforms(rw["sc"])
    moved = [t[(k + 1) % 5] for k in range(5)]
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    base_inst = trace(rw, world, rays, rw["st"])[1]
    handle = world.create_refit(rebuild=True)
    rebuild_device(rw, handle, moved)
    want_inst, hits = assert_traces_as_a_fresh_world(rw, world, moved, rays, "five overlapping instances, rebuilt")
    assert 0.1 <= (want_inst != NO_INSTANCE).mean() <= 0.9 and (hits.sum(0) >= 2).sum() >= 100
    assert (want_inst != base_inst).mean() > 0.1, "the move must change the answer for the test to mean anything"
    host, host_inst = world.intersect(rays)
    assert host_inst.tobytes() == trace(rw, world, rays, rw["st"])[1].tobytes(), "host path on the rebuilt world"
    handle.destroy()
    world.destroy()


def test_results_on_a_permuted_grid(rw):
    ctx, rays = rw["ctx"], rw["rays"][::3]
    v = rw["sc"]["vertices"][:, :3]
    pitch = 1.1 * float((v.max(0) - v.min(0)).max())
    built = grid_transforms(8, pitch)
    moved = np.ascontiguousarray(built[np.random.RandomState(8).permutation(64)])
    rays = rays.copy()
    rays["origin"][:, 0] += np.float32(3.5 * pitch); rays["origin"][:, 2] += np.float32(3.5 * pitch)      # into the middle of the grid
    world = ctx.create_world([(m, rw["scene"]) for m in built])
    handle = world.create_refit(rebuild=True)
    rebuild_device(rw, handle, moved)
    want_inst, _ = assert_traces_as_a_fresh_world(rw, world, moved, rays, "8x8 grid, permuted and rebuilt")
    assert len(np.unique(want_inst)) > 4, "rays must reach several instances for the test to mean anything"
    handle.destroy()
    world.destroy()


def test_results_on_the_chain_world_through_the_spilled_stack(rw):
    """The chain's height on this root box is established by tests/test_world_rebuild_host.py; it is above lds_levels, so the top-level
    stack spills on a tree of known height."""
    ctx, rays = rw["ctx"], rw["rays"][::3]
    moved = chain_world(4096.0)
    world = ctx.create_world([(m, rw["scene"]) for m in random_world(31, 33)[0]])
    handle = world.create_refit(rebuild=True)
    rebuild_device(rw, handle, moved)
    height, disabled = handle.check_rebuild()
    assert disabled == 0 and height == ra.host_world_rebuild(moved, np.tile(rw["root"], (31, 1)))["height"]
    assert height > world.info["lds_levels"] + 1 and world.info["spill_levels"] >= height + 1 - world.info["lds_levels"]
    want_inst, hits = assert_traces_as_a_fresh_world(rw, world, moved, rays, "chain world, rebuilt")
    assert (hits.sum(0) >= 8).sum() >= 100, "rays must pass through the crowded end of the chain"
    handle.destroy()
    info = world.info
    assert info["height"] == height and info["spill_levels"] == max(height + 1 - info["lds_levels"], 0), "destroy sets info from the real height"
    got, got_inst, _ = trace(rw, world, rays, rw["st"])
    want, want_inst2, _ = compose(world.download()["inv"], [rw["blobs"]] * 31, rays)
    assert_world_exact(got, got_inst, want, want_inst2, "chain world after the handle was destroyed")
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 3. stream order
def test_refit_rebuild_refit_trace_on_one_stream_without_host_waits(rw):
    ctx, sc, st = rw["ctx"], rw["sc"], rw["st"]
    rays = rw["rays"][::3]
    n = len(rays)
    base = overlapping_transforms(sc)
    sets = [[base[(i + k) % 5] for i in range(5)] for k in range(1, 4)]      # three different assignments of places
    world = ctx.create_world([(m, rw["scene"]) for m in base])
    handle = world.create_refit(rebuild=True)
    d_t = [device_transforms(ctx, s) for s in sets]
    d_r, d_o, d_i = ctx.alloc(n * 32), ctx.alloc(n * 16), ctx.alloc(n * 4)
    d_r.upload(rays)
    handle.refit_device(d_t[0].ptr, stream=st)      # all in stream order, no host wait in between
    handle.rebuild_device(d_t[1].ptr, stream=st)
    handle.refit_device(d_t[2].ptr, stream=st)
    world.intersect_device(d_r.ptr, d_o.ptr, d_i.ptr, n, stream=st)
    ctx.stream_synchronize(st)
    got, got_inst = d_o.download(synth.RESULT_DTYPE, n), d_i.download(np.uint32, n)
    rb = np.tile(rw["root"], (5, 1))
    want, want_inst, _ = compose(ra.host_world_prepare(np.array(sets[2]), rb)["inv"], [rw["blobs"]] * 5, rays)
    assert_world_exact(got, got_inst, want, want_inst, "refit, rebuild, refit, trace on one stream")
    # the topology is the rebuild's (second set), the boxes the last refit's (third set)
    down = world.download()
    built = ra.host_world_rebuild(np.array(sets[1]), rb)
    refitted = ra.host_world_refit(np.array(sets[2]), rb, built["nodes"], built["order"])
    assert np.array_equal(down["order"], built["order"]) and down["inv"].tobytes() == refitted["inv"].tobytes()
    for f in NODE_FIELDS:
        assert down["nodes"][f].tobytes() == refitted["nodes"][f].tobytes(), f
    _, other_inst, _ = compose(built["inv"], [rw["blobs"]] * 5, rays)
    assert (other_inst != want_inst).mean() > 0.05, "the last refit must change the answer for the test to mean anything"
    for b in d_t + [d_r, d_o, d_i]:
        b.free()
    handle.destroy()
    world.destroy()


def test_a_member_scene_refitted_on_the_same_stream_is_picked_up(rw, small_host):
    ctx, sc, st = rw["ctx"], rw["sc"], rw["st"]
    rays = rw["rays"][::3]
    scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)      # a member scene of this test's own
    scene_refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
    transforms = overlapping_transforms(sc)
    world = ctx.create_world([(m, scene) for m in transforms])
    handle = world.create_refit(rebuild=True)
    v = displaced(sc["vertices"], 11.0, phase=0.3)      # moves the root box as well
    blobs = ra.host_refit(small_host.blobs(), v, sc["indices"])
    rb = np.tile(ra.root_box(blobs["nodes"]), (5, 1))
    assert not np.array_equal(rb[0], rw["root"])
    v4 = ra.engine._as_verts4(v)
    d_v = ctx.alloc(v4.nbytes)
    d_v.upload(v4)
    d_t = device_transforms(ctx, transforms[::-1])
    scene_refit.refit_device(d_v.ptr, len(v4), stream=st)      # the scene's refit and the world's rebuild behind it: stream order alone
    handle.rebuild_device(d_t.ptr, stream=st)
    ctx.stream_synchronize(st)
    assert_download_is_the_host_rebuild(world, np.array(transforms[::-1]), rb, "member scene refitted on the same stream")
    assert_traces_as_a_fresh_world(rw, world, transforms[::-1], rays, "member scene refitted, then the world rebuilt", blobs=blobs, scene=scene)
    d_v.free(); d_t.free()
    handle.destroy()
    world.destroy()
    scene_refit.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 4. handle life
def test_a_plain_refit_handle_cannot_rebuild(rw):
    ctx, lib = rw["ctx"], ra.load_library()
    t = overlapping_transforms(rw["sc"])
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    info = world.info
    handle = world.create_refit()
    assert world.info == info, "a plain handle leaves info alone"
    before = world.download()
    d = device_transforms(ctx, t[::-1])
    with pytest.raises(ra.RaccError) as e:
        handle.rebuild_device(d.ptr, stream=rw["st"])
    assert e.value.code == -1 and "racc_hip_world_refit_create" in str(e.value)
    with pytest.raises(ra.RaccError) as e:
        handle.rebuild(t[::-1])
    assert e.value.code == -1 and "racc_hip_world_refit_create" in str(e.value)
    with pytest.raises(ra.RaccError):
        handle.check_rebuild()
    ctx.stream_synchronize(rw["st"])
    after = world.download()
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("inv", "nodes", "order")) and after["ray_pad"] == before["ray_pad"]
    d.free()
    handle.destroy()
    assert world.info == info
    # ... and on a rebuild handle: one per world, count checked, a refused blocking rebuild leaves the world as it was
    handle = world.create_refit(rebuild=True)
    with pytest.raises(ra.RaccError) as e:
        world.create_refit(rebuild=True)
    assert "already has a refit handle" in str(e.value)
    with pytest.raises(ra.RaccError) as e:
        handle.rebuild(t[:4])
    assert "count differs" in str(e.value)
    singular = [m.copy() for m in t]
    singular[3][2, :3] = 0
    with pytest.raises(ra.RaccError) as e:
        handle.rebuild(singular)
    assert e.value.code == -1 and "singular" in str(e.value) and "racc_hip_world_rebuild" in str(e.value)
    after = world.download()
    assert all(after[k].tobytes() == before[k].tobytes() for k in ("inv", "nodes", "order")), "a refused rebuild left the world as it was"
    handle.rebuild(t[::-1])      # the blocking entry: complete on return
    assert_download_is_the_host_rebuild(world, np.array(t[::-1]), np.tile(rw["root"], (5, 1)), "the blocking rebuild")
    handle.destroy()
    world.destroy()


def test_world_update_with_the_rebuild_handle_alive_then_a_device_rebuild(rw):
    ctx, count = rw["ctx"], 65
    rays = rw["rays"][::6]
    rb = np.tile(rw["root"], (count, 1))
    rng = np.random.RandomState(6)
    t = np.array([affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), rng.uniform(0.5, 1.5, 3), rng.uniform(-60, 60, 3)) for _ in range(count)])
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    lds = world.info["lds_levels"]
    handle = world.create_refit(rebuild=True)
    bound = height_bound(count, disabled_possible=True)
    assert world.info["height"] >= bound and world.info["spill_levels"] >= bound + 1 - lds, "raised at creation"
    updated = np.ascontiguousarray(t[rng.permutation(count)])
    world.update(updated)      # the host rebuild, under the live handle
    assert world.info["height"] >= bound and world.info["spill_levels"] >= bound + 1 - lds, "racc_hip_world_update keeps the raised values"
    host = ra.host_world_prepare(updated, rb)
    assert handle.check_rebuild()[0] == host["height"], "the height word follows the host rebuild"
    moved = np.ascontiguousarray(t[rng.permutation(count)])
    moved[:, :, 3] += np.float32(2.0)
    rebuild_device(rw, handle, moved)
    want = assert_download_is_the_host_rebuild(world, moved, rb, "device rebuild after World.update")
    assert handle.check_rebuild() == (want["height"], 0)
    assert world.info["spill_levels"] >= want["height"] + 1 - lds
    assert_traces_as_a_fresh_world(rw, world, moved, rays, "device rebuild after World.update")
    handle.destroy()
    assert world.info["height"] == want["height"]
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 5. disabled instances
def test_unusable_transforms_disable_their_instances(rw):
    ctx, blobs, count = rw["ctx"], rw["blobs"], 65
    dead = [17, 40]
    rays = rw["rays"][::6]
    rng = np.random.RandomState(5)
    t = np.array([affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), rng.uniform(0.5, 1.5, 3), rng.uniform(-60, 60, 3)) for _ in range(count)])
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    handle = world.create_refit(rebuild=True)
    moved = np.ascontiguousarray(t[rng.permutation(count)])
    moved[:, :, 3] += np.float32(3.0)
    good = moved.copy()
    moved[dead[0]] = 0                   # a zero matrix
    moved[dead[1], 1, 2] = np.nan        # a NaN coefficient
    rebuild_device(rw, handle, moved)
    height, disabled = handle.check_rebuild()
    assert disabled == 2 and handle.check() == 2
    after = world.download()
    assert np.isnan(after["inv"][dead]).all() and np.isfinite(np.delete(after["inv"], dead, 0)).all()
    # every instance is still named once, the disabled ones behind every enabled one; the height is the walk's and inside the bound
    assert walk_height(after["nodes"]["first"], after["nodes"]["last"], count) == height <= height_bound(count, disabled_possible=True)
    assert sorted(after["order"].tolist()) == list(range(count)) and after["order"][-2:].tolist() == dead
    others = np.delete(np.arange(count), dead)
    sub = ra.host_world_prepare(moved[others], np.tile(rw["root"], (count - 2, 1)))
    assert after["inv"][others].tobytes() == sub["inv"].tobytes() and after["ray_pad"] == sub["ray_pad"], "disabled instances do not enter the pad"
    # never reported: the composition over NaN inverses (every transformed ray is rejected), as the refit's test does it
    want, want_inst, _ = compose(after["inv"], [blobs] * count, rays)
    assert (want_inst != NO_INSTANCE).mean() > 0.1 and not np.isin(want_inst, dead).any()
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    assert_world_exact(got, got_inst, want, want_inst, "63 live instances beside two disabled ones")
    assert np.array_equal(occ, (want_inst != NO_INSTANCE).astype(np.uint8))
    # no other record changes: the same world with usable transforms there differs only where those two instances are hit
    rebuild_device(rw, handle, good)
    assert handle.check_rebuild()[1] == 0 and np.isfinite(world.download()["inv"]).all()
    full, full_inst, _ = trace(rw, world, rays, rw["st"])
    keep = ~np.isin(full_inst, dead)
    assert np.isin(full_inst, dead).any(), "the two instances must be hit for the test to mean anything"
    assert got[keep].tobytes() == full[keep].tobytes() and got_inst[keep].tobytes() == full_inst[keep].tobytes()
    handle.destroy()
    world.destroy()
