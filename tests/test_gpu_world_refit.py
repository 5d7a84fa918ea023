"""Refit of a world's top level on the device — racc_hip_world_refit* / worldRefitKernel (rayaccel_amd/csrc/racc_world_refit.inc).

Two bars.  The refitted world as bytes: World.download() after a device refit equals racc_host_world_refit of the download before it (inv,
the top-level records, ray_pad).  Its results: bit-exact on triangle, t, u, v and the instance index against world_helpers.compose on
the new inverses, and byte-equal to a world created with the new transforms.  At most 16k rays per launch."""
import ctypes as C

import numpy as np
import pytest

import rayaccel_amd as ra
from rayaccel_amd import synth
from refit_helpers import displaced
from test_world_host import random_world
from world_helpers import IDENTITY, NO_INSTANCE, affine, assert_world_exact, compose, rotation

pytestmark = pytest.mark.gpu


def overlapping_transforms(sc):
    """tests/test_gpu_world.py's five: general affine transforms of the small scene, translated by less than its extent."""
    v = sc["vertices"][:, :3]
    ext = float((v.max(0) - v.min(0)).max())
    return [affine(),
            affine(rotation([0, 1, 0], 30.0), translation=(0.15 * ext, 0.05 * ext, -0.1 * ext)),
            affine(rotation([1, 2, 0.5], 75.0), scale=(1.2, 0.7, 0.9), translation=(-0.2 * ext, 0.1 * ext, 0.1 * ext)),
            affine(scale=(-1.0, 1.0, 1.0), translation=(0.05 * ext, -0.04 * ext, 0.12 * ext)),      # a mirror
            affine(rotation([0.3, -1, 0.2], 200.0), scale=(0.8, 0.8, 0.8), translation=(0.1 * ext, 0.02 * ext, 0.2 * ext))]


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


@pytest.fixture(scope="module")
def five(rw):
    transforms = overlapping_transforms(rw["sc"])
    world = rw["ctx"].create_world([(m, rw["scene"]) for m in transforms])
    yield dict(world=world, transforms=transforms)
    world.destroy()


def device_transforms(ctx, transforms):
    t = np.ascontiguousarray(np.asarray(transforms, np.float32).reshape(-1, 12))
    d = ctx.alloc(t.nbytes)
    d.upload(t)
    return d


def refit_device(rw, handle, transforms):
    """One device refit on the module's stream, waited for."""
    d = device_transforms(rw["ctx"], transforms)
    handle.refit_device(d.ptr, stream=rw["st"])
    rw["ctx"].stream_synchronize(rw["st"])
    d.free()


def trace(rw, world, rays, stream=None):
    """(results, instances, occluded) of the device entries on `stream`, waited for."""
    ctx, n = rw["ctx"], len(rays)
    d_r, d_o, d_i, d_b = ctx.alloc(n * 32), ctx.alloc(n * 16), ctx.alloc(n * 4), ctx.alloc(n)
    d_r.upload(rays)
    world.intersect_device(d_r.ptr, d_o.ptr, d_i.ptr, n, stream=stream)
    world.occluded_device(d_r.ptr, d_b.ptr, n, stream=stream)
    ctx.stream_synchronize(stream)
    out = d_o.download(synth.RESULT_DTYPE, n), d_i.download(np.uint32, n), d_b.download(np.uint8, n)
    for b in (d_r, d_o, d_i, d_b):
        b.free()
    return out


def assert_download_is_the_host_refit(before, after, transforms, root_boxes, what):
    want = ra.host_world_refit(transforms, root_boxes, before["nodes"], before["order"])
    assert after["inv"].tobytes() == want["inv"].tobytes(), "%s: inv differs from racc_host_world_refit" % what
    assert np.array_equal(after["order"], before["order"]), "%s: order changed" % what
    for f in ("first", "last"):
        assert np.array_equal(after["nodes"][f], want["nodes"][f]), "%s: topology word %s changed" % (what, f)
    for f in ("leftMin", "leftMax", "rightMin", "rightMax"):
        assert after["nodes"][f].tobytes() == want["nodes"][f].tobytes(), "%s: %s differs from racc_host_world_refit" % (what, f)
    assert np.float32(after["ray_pad"]).tobytes() == np.float32(want["ray_pad"]).tobytes(), "%s: ray_pad %r, host %r" % (what, after["ray_pad"], want["ray_pad"])
    return want


def moved_transforms(n, seed):
    """Rotations, non-uniform scales of either sign and translations far from where the tree was built."""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        t[i] = affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), 10.0 ** rng.uniform(-1, 2, 3) * rng.choice([-1.0, 1.0], 3), rng.uniform(-1e4, 1e4, 3))
    return t


# ------------------------------------------------------------------------------------------------------------ 1. byte parity
@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 1000])
def test_download_after_a_device_refit_is_the_host_refit(rw, count):
    ctx = rw["ctx"]
    t, _ = random_world(count, 700 + count)
    rb = np.tile(rw["root"], (count, 1))
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    built = ra.host_world_prepare(t, rb)
    before = world.download()
    assert before["inv"].tobytes() == built["inv"].tobytes() and np.array_equal(before["order"], built["order"]) and before["ray_pad"] == built["ray_pad"]
    for f in ("first", "last", "leftMin", "leftMax", "rightMin", "rightMax"):
        assert before["nodes"][f].tobytes() == built["nodes"][f].tobytes(), "download of a fresh world: %s" % f
    handle = world.create_refit()
    assert world.download()["ray_pad"] == built["ray_pad"], "the pad word of a new handle holds the world's pad"
    for round_, seed in enumerate((800 + count, 900 + count)):      # twice on one handle: the counters are reset
        moved = moved_transforms(count, seed)
        refit_device(rw, handle, moved)
        assert handle.check() == 0
        after = world.download()
        assert_download_is_the_host_refit(before, after, moved, rb, "%d instances, refit %d" % (count, round_))
        fresh = ra.host_world_prepare(moved, rb)
        assert after["inv"].tobytes() == fresh["inv"].tobytes() and after["ray_pad"] == fresh["ray_pad"]
        before = after
    handle.destroy()
    assert world.download()["ray_pad"] == before["ray_pad"], "destroy copies the pad back into the world"
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. results
def test_results_after_instances_swap_places(rw, five):
    ctx, blobs, rays = rw["ctx"], rw["blobs"], rw["rays"]
    moved = [five["transforms"][(k + 1) % 5] for k in range(5)]      # every instance takes its neighbour's place: the worst case for kept topology
    world = ctx.create_world([(m, rw["scene"]) for m in five["transforms"]])
    base, base_inst, _ = trace(rw, world, rays, rw["st"])
    handle = world.create_refit()
    refit_device(rw, handle, moved)
    inv = world.download()["inv"]
    want, want_inst, hits = compose(inv, [blobs] * 5, rays)
    assert 0.1 <= (want_inst != NO_INSTANCE).mean() <= 0.9 and (hits.sum(0) >= 2).sum() >= 100
    assert (want_inst != base_inst).mean() > 0.1, "the move must change the answer for the test to mean anything"
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    assert_world_exact(got, got_inst, want, want_inst, "after the refit (device path)")
    assert np.array_equal(occ, (want_inst != NO_INSTANCE).astype(np.uint8)), "occluded after the refit"
    host, host_inst = world.intersect(rays)
    assert_world_exact(host, host_inst, want, want_inst, "after the refit (host path)")
    assert np.array_equal(world.occluded(rays), occ)
    fresh = ctx.create_world([(m, rw["scene"]) for m in moved])
    f, f_inst, f_occ = trace(rw, fresh, rays, rw["st"])
    assert got.tobytes() == f.tobytes() and got_inst.tobytes() == f_inst.tobytes() and occ.tobytes() == f_occ.tobytes(), "against a world created with the new transforms"
    fresh.destroy()
    handle.destroy()
    got, got_inst, _ = trace(rw, world, rays, rw["st"])      # the world keeps its refitted state without the handle
    assert_world_exact(got, got_inst, want, want_inst, "after the handle was destroyed")
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 3. stream order
def test_twenty_refits_and_launches_on_one_stream_without_host_waits(rw, five):
    ctx, blobs, st, lib = rw["ctx"], rw["blobs"], rw["st"], ra.load_library()
    rays = rw["rays"][::6]
    n, steps = len(rays), 20
    sets = [[(affine(rotation([0, 1, 0], 7.0 * k), translation=(2.0 * k, -1.0 * k, 0.5 * k * i)).astype(np.float64) @ np.vstack([m, [0, 0, 0, 1]]))[:3].astype(np.float32)
             for i, m in enumerate(five["transforms"])] for k in range(steps)]
    world = ctx.create_world([(m, rw["scene"]) for m in five["transforms"]])
    handle = world.create_refit()
    staged = device_transforms(ctx, np.array(sets, np.float32).reshape(steps * 5, 12))      # every step's transforms, uploaded before the first launch
    d_t, d_r = ctx.alloc(5 * 48), ctx.alloc(n * 32)
    d_r.upload(rays)
    outs = [(ctx.alloc(n * 16), ctx.alloc(n * 4)) for _ in range(steps)]
    for k in range(steps):      # upload transforms k, refit, launch into buffer k: all in stream order, no host wait in between
        ra.engine._check(lib.racc_hip_memcpy_d2d_async(ctx._h, d_t.ptr, staged.ptr + k * 5 * 48, 5 * 48, st))
        handle.refit_device(d_t.ptr, stream=st)
        world.intersect_device(d_r.ptr, outs[k][0].ptr, outs[k][1].ptr, n, stream=st)
    ctx.stream_synchronize(st)
    assert handle.check() == 0
    changed = 0
    for k in range(steps):
        inv = ra.host_world_prepare(np.array(sets[k]), np.tile(rw["root"], (5, 1)))["inv"]
        want, want_inst, _ = compose(inv, [blobs] * 5, rays)
        got, got_inst = outs[k][0].download(synth.RESULT_DTYPE, n), outs[k][1].download(np.uint32, n)
        assert_world_exact(got, got_inst, want, want_inst, "step %d of 20 on one stream" % k)
        if k:
            changed += int((got["t"].view(np.uint32) != prev).any())
        prev = got["t"].view(np.uint32).copy()
    assert changed == steps - 1, "every step must change the answer for the test to mean anything"
    for b in [staged, d_t, d_r] + [x for pair in outs for x in pair]:
        b.free()
    handle.destroy()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 4. member scene refit
def test_a_refitted_member_scene_is_picked_up_without_a_world_update(rw, small_host):
    ctx, sc, rays = rw["ctx"], rw["sc"], rw["rays"]
    scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    scene_refit = ctx.create_refit(scene, sc["indices"], len(sc["vertices"]))
    transforms = overlapping_transforms(sc)[:3]
    world = ctx.create_world([(m, scene) for m in transforms])
    handle = world.create_refit()
    v = displaced(sc["vertices"], 11.0, phase=0.3)      # moves the root box as well
    blobs = ra.host_refit(small_host.blobs(), v, sc["indices"])
    assert not np.array_equal(ra.root_box(blobs["nodes"]), ra.root_box(small_host.nodes))
    scene_refit.refit(v)
    before = world.download()
    refit_device(rw, handle, transforms)      # unchanged transforms, no World.update: the root boxes are read on the device
    assert_download_is_the_host_refit(before, world.download(), np.array(transforms), np.tile(ra.root_box(blobs["nodes"]), (3, 1)), "member scene refitted")
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    want, want_inst, _ = compose(world.download()["inv"], [blobs] * 3, rays)
    assert_world_exact(got, got_inst, want, want_inst, "member scene refitted, then the world refit")
    fresh = ctx.create_world([(m, scene) for m in transforms])      # made after the scene refit
    f, f_inst, f_occ = trace(rw, fresh, rays, rw["st"])
    assert got.tobytes() == f.tobytes() and got_inst.tobytes() == f_inst.tobytes() and occ.tobytes() == f_occ.tobytes()
    fresh.destroy()
    handle.destroy()
    world.destroy()
    scene_refit.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 5. ray pad
def test_ray_pad_follows_the_condition_numbers(rw):
    ctx, blobs = rw["ctx"], rw["blobs"]
    rb = np.tile(rw["root"], (3, 1))
    turned = [affine(rotation([0, 1, 0], 40.0 * k), translation=(30.0 * k, 0.0, 0.0)) for k in range(3)]
    squashed = [affine(rotation([1, 0.5, 0], 25.0 * k), scale=(1e3, 1.0, 1e-2), translation=(30.0 * k, 5.0 * k, 0.0)) for k in range(3)]
    world = ctx.create_world([(m, rw["scene"]) for m in turned])
    handle = world.create_refit()
    pad0 = world.download()["ray_pad"]
    refit_device(rw, handle, squashed)
    want = ra.host_world_prepare(np.array(squashed), rb)
    pad1 = world.download()["ray_pad"]
    print("ray_pad: %.9g for pure rotations, %.9g for a scale of (1e3, 1, 1e-2)" % (pad0, pad1))
    assert pad0 == ra.host_world_prepare(np.array(turned), rb)["ray_pad"] and pad1 == want["ray_pad"] and pad1 > 1000 * pad0
    rays = rw["rays"][:8192].copy()
    d = rays["dir"] / np.linalg.norm(rays["dir"], axis=1, keepdims=True)
    rays["origin"] = (rays["origin"].astype(np.float64) - 1e5 * d.astype(np.float64)).astype(np.float32)      # origins at 1e5, aimed at where they were
    rays["maxT"] = np.inf
    exp, exp_inst, _ = compose(want["inv"], [blobs] * 3, rays)
    print("rays from 1e5: %d of %d hit" % ((exp_inst != NO_INSTANCE).sum(), len(rays)))
    assert (exp_inst != NO_INSTANCE).sum() > 0
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    assert_world_exact(got, got_inst, exp, exp_inst, "origins at 1e5 under the refitted pad")
    assert np.array_equal(occ, (exp_inst != NO_INSTANCE).astype(np.uint8))
    handle.destroy()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 6. rebuild in between
def test_world_update_with_a_live_handle_then_refit_again(rw):
    ctx, count = rw["ctx"], 65
    rb = np.tile(rw["root"], (count, 1))
    t, _ = random_world(count, 41)
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    handle = world.create_refit()
    refit_device(rw, handle, moved_transforms(count, 42))
    rebuilt = moved_transforms(count, 43)
    world.update(rebuilt)      # rebuilds the top level and the handle's tables
    want = ra.host_world_prepare(rebuilt, rb)
    before = world.download()
    assert before["inv"].tobytes() == want["inv"].tobytes() and before["ray_pad"] == want["ray_pad"] and np.array_equal(before["order"], want["order"])
    assert np.array_equal(before["nodes"]["first"], want["nodes"]["first"]) and np.array_equal(before["nodes"]["last"], want["nodes"]["last"])
    assert not np.array_equal(want["order"], ra.host_world_prepare(t, rb)["order"]), "the rebuild must change the topology for the test to mean anything"
    moved = moved_transforms(count, 44)
    refit_device(rw, handle, moved)
    assert handle.check() == 0
    assert_download_is_the_host_refit(before, world.download(), moved, rb, "refit after World.update")
    handle.destroy()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. disabled instance
def test_an_unusable_transform_disables_its_instance(rw):
    ctx, blobs, count, dead = rw["ctx"], rw["blobs"], 65, 17
    rays = rw["rays"][::6]
    rng = np.random.RandomState(5)
    t = np.array([affine(rotation(rng.normal(size=3), rng.uniform(0, 360)), rng.uniform(0.5, 1.5, 3), rng.uniform(-60, 60, 3)) for _ in range(count)])
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    handle = world.create_refit()
    moved = t.copy()
    moved[:, :, 3] += np.float32(3.0)
    moved[dead] = 0      # an all-zero transform
    refit_device(rw, handle, moved)
    assert handle.check() == 1
    after = world.download()
    assert np.isnan(after["inv"][dead]).all() and np.isfinite(np.delete(after["inv"], dead, 0)).all()
    others = np.delete(np.arange(count), dead)
    sub = ra.host_world_prepare(moved[others], np.tile(rw["root"], (count - 1, 1)))
    assert after["inv"][others].tobytes() == sub["inv"].tobytes() and after["ray_pad"] == sub["ray_pad"], "the disabled instance does not enter the pad"
    want, want_inst, _ = compose(sub["inv"], [blobs] * (count - 1), rays)      # the 64-instance composition
    hit = want_inst != NO_INSTANCE
    want_inst[hit] = others[want_inst[hit]].astype(np.uint32)
    assert hit.mean() > 0.1
    got, got_inst, occ = trace(rw, world, rays, rw["st"])
    assert (got_inst != dead).all(), "the disabled instance is reported"
    assert_world_exact(got, got_inst, want, want_inst, "64 live instances beside a disabled one")
    assert np.array_equal(occ, hit.astype(np.uint8))
    refit_device(rw, handle, t)      # ... and a usable transform brings it back
    assert handle.check() == 0 and np.isfinite(world.download()["inv"]).all()
    handle.destroy()
    world.destroy()


# ------------------------------------------------------------------------------------------------------------ 8. handle rules
def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the engine itself is linked against (as tests/test_gpu_world.py)."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_handle_rules(rw, five):
    ctx, lib, rays = rw["ctx"], ra.load_library(), rw["rays"][:4096]
    world = ctx.create_world([(m, rw["scene"]) for m in five["transforms"]])
    handle = world.create_refit()
    with pytest.raises(ra.RaccError) as e:
        world.create_refit()
    assert e.value.code == -1 and "already has a refit handle" in str(e.value)
    d = device_transforms(ctx, five["transforms"])
    assert lib.racc_hip_world_refit_device(ctx._h, handle._h, d.ptr, 4, None) == -1 and b"count differs" in lib.racc_hip_last_error()
    with pytest.raises(ra.RaccError) as e:
        handle.refit(five["transforms"][:4])
    assert "count differs" in str(e.value)
    d.free()
    base, base_inst = world.intersect(rays)
    singular = [m.copy() for m in five["transforms"]]
    singular[3][2, :3] = 0
    with pytest.raises(ra.RaccError) as e:
        handle.refit(singular)
    assert e.value.code == -1 and "singular" in str(e.value) and "racc_hip_world_refit" in str(e.value)
    got, got_inst = world.intersect(rays)
    assert got.tobytes() == base.tobytes() and got_inst.tobytes() == base_inst.tobytes(), "a refused refit left the world as it was"
    moved = [five["transforms"][(k + 2) % 5] for k in range(5)]
    handle.refit(moved)      # the blocking entry: complete on return
    want, want_inst, _ = compose(ra.host_world_prepare(np.array(moved), np.tile(rw["root"], (5, 1)))["inv"], [rw["blobs"]] * 5, rays)
    got, got_inst = world.intersect(rays)
    assert_world_exact(got, got_inst, want, want_inst, "after the blocking refit")
    with pytest.raises(ra.RaccError) as e:      # the world is destroyed after its handle
        ra.engine._check(lib.racc_hip_world_destroy(ctx._h, world._h))
    assert "refit handle" in str(e.value)
    handle.destroy()
    world.create_refit().destroy()      # ... and a new handle may follow a destroyed one
    world.destroy()


def test_destroy_gives_the_memory_back(rw):
    """A handle large enough to be seen in hipMemGetInfo (2^18 instances: 3 MB of tables and 12 MB of staging once the blocking entry has
    run): what it took comes back at destroy but for an eighth, and the world's own device_bytes is what it was."""
    ctx = rw["ctx"]
    n = 1 << 18
    t = np.tile(IDENTITY.reshape(1, 12), (n, 1))
    t[:, 3] = 170.0 * (np.arange(n) % 512); t[:, 11] = 170.0 * (np.arange(n) // 512)
    world = ctx.create_world([(m, rw["scene"]) for m in t])
    assert world.info["device_bytes"] == 148 * n - 64
    before = _free_device_memory()
    handle = world.create_refit()
    t[:, 7] = 5.0
    handle.refit(t)
    held = before - _free_device_memory()
    assert world.info["device_bytes"] == 148 * n - 64, "the refit state belongs to the handle, not to the world"
    assert world.download()["inv"][n - 1].tobytes() == ra.host_world_prepare(t[n - 1:], rw["root"][None])["inv"].tobytes()
    handle.destroy()
    after = _free_device_memory()
    print("refit handle of 2^18 instances: %d bytes of device memory held, %d not returned by destroy" % (held, before - after))
    assert held >= 12 << 20, "the handle holds %d bytes: too little for this test to see" % held
    assert abs(before - after) <= held // 8
    world.destroy()
