"""Build and rebuild of a scene's tree on the device — racc_hip_scene_rebuild* (rayaccel_amd/csrc/racc_scene_rebuild.inc).

Two bars.  The scene as bytes: Refit.download() and download_remap() after the creation and after a device rebuild to moved vertices equal
racc_host_scene_rebuild (the four topology words, the four box fields, the padded pairs, remap) and check_rebuild() returns its height.
Its results: what intersect, occluded and a two-instance world report on the device-built scene is bit for bit what they report on
racc_hip_scene_upload of the host function's blobs, and the closest hits are the oracle's traversal of those blobs, bit for bit.  Every
height relied on here is established by tests/test_scene_rebuild_host.py on the CPU; every mesh is finite.  T <= 4,099, 6k rays a launch."""
import ctypes as C

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from scene_rebuild_helpers import NODE_FIELDS, chain, common_centre, height_bound, moved, rays_at, soup
from world_helpers import affine

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
RAYS = 6000


@pytest.fixture(scope="module")
def rb():
    """A context of this module's own (default kernel) and a stream."""
    ctx = ra.Context(device=0)
    st = ctx.create_stream()
    yield dict(ctx=ctx, st=st)
    ctx.destroy_stream(st)
    ctx.destroy()


def mesh_of(case):
    if case == "all-ties":
        return common_centre(1000)
    if case == "chain":
        return chain()
    return soup(case, 900 + case)


def moved_mesh(case, v, seed):
    """The case's mesh for a second build: displaced vertices — but the two special meshes keep what makes them special."""
    if case == "all-ties":
        return (v + np.float32([2, 1, -3])).astype(np.float32)
    if case == "chain":
        return (v * np.float32(0.5)).astype(np.float32)      # exact: the centres stay powers of two
    return moved(v, seed)


def device_vertices(ctx, v):
    v4 = ra.engine._as_verts4(v)
    d = ctx.alloc(v4.nbytes)
    d.upload(v4)
    return d, len(v4)


def rebuild_device(rb, handle, v):
    """One device rebuild on the module's stream, waited for (the bound stays held: no check)."""
    d, n = device_vertices(rb["ctx"], v)
    handle.rebuild_device(d.ptr, n, stream=rb["st"])
    rb["ctx"].stream_synchronize(rb["st"])
    d.free()


def assert_scene_is_the_host_rebuild(handle, v, idx, what):
    want = ra.host_scene_rebuild(v, idx)
    nodes, pairs = handle.download()
    assert len(nodes) == len(want["nodes"]) and len(pairs) == len(want["pairs"]), what
    for f in NODE_FIELDS:
        assert nodes[f].tobytes() == want["nodes"][f].tobytes(), "%s: nodes.%s differs from racc_host_scene_rebuild" % (what, f)
    assert pairs.tobytes() == want["pairs"].tobytes(), "%s: pairs differ from racc_host_scene_rebuild" % what
    assert np.array_equal(handle.download_remap(), want["remap"]), "%s: remap differs from racc_host_scene_rebuild" % what
    return want


def trace_all(rb, scene, rays):
    """(closest hits, occluded, world closest hits, world instances, world occluded) through the default entries."""
    ctx = rb["ctx"]
    got, occ = ctx.intersect(scene, None, rays), ctx.occluded(scene, rays)
    world = ctx.create_world([(affine(), scene), (affine(translation=(0.25, -0.5, 0.125)), scene)])
    w, w_inst = world.intersect(rays)
    w_occ = world.occluded(rays)
    world.destroy()
    return got, occ, w, w_inst, w_occ


def assert_traces_as_the_uploaded_host_blobs(rb, scene, blobs, rays, what):
    ctx = rb["ctx"]
    uploaded = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    want = trace_all(rb, uploaded, rays)
    uploaded.destroy()
    got = trace_all(rb, scene, rays)
    for g, w, name in zip(got, want, ("intersect", "occluded", "world intersect", "world instances", "world occluded")):
        assert g.tobytes() == w.tobytes(), "%s: %s differs from the same entry on racc_hip_scene_upload of the host blobs" % (what, name)
    ref = orc.traverse(blobs, rays)
    hit = ref["triangle"] != MISS
    assert np.array_equal(got[0]["triangle"], ref["triangle"]), "%s: triangles differ from the oracle's traversal" % what
    for f in ("t", "u", "v"):
        assert got[0][f][hit].tobytes() == ref[f][hit].tobytes(), "%s: %s differs from the oracle's traversal" % (what, f)
    assert np.array_equal(got[1], hit.astype(np.uint8)), "%s: occluded against the oracle's hits" % what
    assert 0.2 < hit.mean(), "%s: rays must hit for the test to mean anything" % what
    return ref


# ------------------------------------------------------------------------------------------------------------ 1. byte parity
CASES = [2, 3, 33, 1000, 4099, "all-ties", "chain"]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_download_after_create_and_after_a_device_rebuild_is_the_host_rebuild(rb, case):
    ctx = rb["ctx"]
    v, idx = mesh_of(case)
    t = idx.size // 3
    scene, handle = ctx.create_dynamic_scene(v, idx)
    want = assert_scene_is_the_host_rebuild(handle, v, idx, "%s, created" % case)
    info = scene.info
    assert info["node_count"] == t - 1 and info["remap_count"] == 2 * t and info["max_leaf_pairs"] == 1 and info["inner_height"] == want["height"]
    for round_ in range(2):      # twice on one handle
        v2 = moved_mesh(case, v, 40 + round_)
        rebuild_device(rb, handle, v2)
        assert scene.info["inner_height"] == height_bound(t), "the bound is held behind a device rebuild"
        want = assert_scene_is_the_host_rebuild(handle, v2, idx, "%s, device rebuild %d" % (case, round_))
        assert handle.check_rebuild() == want["height"] == scene.info["inner_height"]
        v = v2
    v3 = moved_mesh(case, v, 50)
    handle.rebuild(v3)      # the blocking entry: complete on return, the real height in info
    want = assert_scene_is_the_host_rebuild(handle, v3, idx, "%s, blocking rebuild" % case)
    assert scene.info["inner_height"] == want["height"]
    handle.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 2. results
@pytest.mark.parametrize("case", [1000, "chain"], ids=["1000", "chain"])
def test_results_under_the_held_bound_and_after_check(rb, case):
    """Once between rebuild_device and check (the bound held: up to 75 spilled levels allocated) and once after check (the real height).
    The chain's height is above every LDS stack (tests/test_scene_rebuild_host.py), so its rays run through the spill."""
    ctx = rb["ctx"]
    v, idx = mesh_of(case)
    t = idx.size // 3
    scene, handle = ctx.create_dynamic_scene(v, idx)
    v2 = moved_mesh(case, v, 60)
    blobs = ra.host_scene_rebuild(v2, idx)
    rays = rays_at(v2, idx, RAYS, 61)
    if case == "chain":      # along the chain, through all forty triangles' boxes
        rays["origin"][::2] = np.float32([2.0, 0.0, 0.0]) + np.random.RandomState(5).uniform(-0.2, 0.2, (len(rays[::2]), 3)).astype(np.float32)
        rays["dir"][::2] = np.float32([-1.0, 0.0, 0.0])
        assert blobs["height"] > 13
    rebuild_device(rb, handle, v2)
    assert scene.info["inner_height"] == height_bound(t) >= blobs["height"]
    ref = assert_traces_as_the_uploaded_host_blobs(rb, scene, blobs, rays, "%s under the held bound" % case)
    assert handle.check_rebuild() == blobs["height"] == scene.info["inner_height"]
    assert_traces_as_the_uploaded_host_blobs(rb, scene, blobs, rays, "%s after check" % case)
    assert len(np.unique(ref["triangle"])) > (10 if case == "chain" else 100)
    handle.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 3. refit after rebuild
def test_a_refit_on_the_same_handle_is_the_host_refit_of_the_host_rebuild(rb):
    ctx = rb["ctx"]
    v, idx = soup(1000, 71)
    scene, handle = ctx.create_dynamic_scene(v, idx)
    v2, v3 = moved(v, 72), moved(v, 73, amount=0.7)
    rebuild_device(rb, handle, v2)
    built = ra.host_scene_rebuild(v2, idx)
    want = ra.host_refit(built, v3, idx)
    for blocking in (False, True):
        if blocking:
            handle.refit(v3)
        else:
            d, n = device_vertices(ctx, v3)
            handle.refit_device(d.ptr, n, stream=rb["st"])
            ctx.stream_synchronize(rb["st"])
            d.free()
        nodes, pairs = handle.download()
        assert nodes.tobytes() == want["nodes"].tobytes() and pairs.tobytes() == want["pairs"].tobytes(), "refit behind a rebuild (blocking=%s)" % blocking
        assert np.array_equal(handle.download_remap(), built["remap"])
        assert handle.check() == 0
        rebuild_device(rb, handle, v2)      # back, for the second round
    handle.check_rebuild()
    rays = rays_at(v3, idx, RAYS, 74)
    handle.refit(v3)
    got = ctx.intersect(scene, None, rays)
    ref = orc.traverse(want, rays)
    hit = ref["triangle"] != MISS
    assert np.array_equal(got["triangle"], ref["triangle"]) and got["t"][hit].tobytes() == ref["t"][hit].tobytes()
    handle.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 4. stream order
def test_rebuild_refit_and_a_world_launch_on_one_stream_without_host_waits(rb):
    ctx, st = rb["ctx"], rb["st"]
    v, idx = soup(1000, 81)
    scene, handle = ctx.create_dynamic_scene(v, idx)
    v2, v3 = moved(v, 82), moved(v, 83, amount=0.7)
    rebuild_device(rb, handle, v)      # the bound is held from here on: the world created now has stack room for every rebuild to come
    transforms = [affine(), affine(translation=(0.25, -0.5, 0.125))]
    world = ctx.create_world([(m, scene) for m in transforms])
    rays = rays_at(v3, idx, RAYS, 84)
    n = len(rays)
    (d2, nv), (d3, _) = device_vertices(ctx, v2), device_vertices(ctx, v3)
    d_r, d_o, d_i = ctx.alloc(n * 32), ctx.alloc(n * 16), ctx.alloc(n * 4)
    d_r.upload(rays)
    handle.rebuild_device(d2.ptr, nv, stream=st)      # all in stream order, no host wait in between
    handle.refit_device(d3.ptr, nv, stream=st)
    world.intersect_device(d_r.ptr, d_o.ptr, d_i.ptr, n, stream=st)
    ctx.stream_synchronize(st)
    got, got_inst = d_o.download(synth.RESULT_DTYPE, n), d_i.download(np.uint32, n)
    # the topology is the rebuild's (second set), the boxes and pairs the refit's (third set)
    built = ra.host_scene_rebuild(v2, idx)
    want = ra.host_refit(built, v3, idx)
    nodes, pairs = handle.download()
    assert nodes.tobytes() == want["nodes"].tobytes() and pairs.tobytes() == want["pairs"].tobytes() and np.array_equal(handle.download_remap(), built["remap"])
    # ... and the launch behind them saw exactly that scene: the same world over an upload of those blobs
    uploaded = ctx.upload_scene(want["nodes"], want["pairs"], want["remap"])
    fresh = ctx.create_world([(m, uploaded) for m in transforms])
    f, f_inst = fresh.intersect(rays)
    assert got.tobytes() == f.tobytes() and got_inst.tobytes() == f_inst.tobytes(), "rebuild, refit, world launch on one stream"
    assert (got_inst != ra.NO_INSTANCE).mean() > 0.2
    unrefitted = ctx.upload_scene(built["nodes"], built["pairs"], built["remap"])
    other = ctx.intersect(unrefitted, None, rays)
    alone = ctx.intersect(uploaded, None, rays)
    assert (other["t"] != alone["t"]).mean() > 0.05, "the refit must change the answer for the test to mean anything"
    for b in (d2, d3, d_r, d_o, d_i):
        b.free()
    fresh.destroy(); world.destroy()
    unrefitted.destroy(); uploaded.destroy()
    handle.destroy()
    scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(rb, small_scene, small_host):
    ctx, lib = rb["ctx"], ra.load_library()
    v, idx = soup(33, 91)
    scene, handle = ctx.create_dynamic_scene(v, idx)
    # the rebuild's handle is the scene's only handle
    for wide in (False, True):
        with pytest.raises(ra.RaccError) as e:
            ctx.create_refit(scene, idx, len(v), wide=wide)
        assert e.value.code == -1 and "racc_hip_scene_rebuild_create" in str(e.value) and "only handle" in str(e.value)
    # vertex_count is the handle's
    d, n = device_vertices(ctx, np.concatenate([v, v[:1]]))
    before = handle.download()
    for call in (lambda: handle.rebuild_device(d.ptr, n, stream=rb["st"]), lambda: handle.rebuild(np.concatenate([v, v[:1]]))):
        with pytest.raises(ra.RaccError) as e:
            call()
        assert e.value.code == -1 and "vertex_count differs" in str(e.value)
    bad = v.copy(); bad[5, 1] = np.inf
    with pytest.raises(ra.RaccError) as e:
        handle.rebuild(bad)
    assert e.value.code == -1 and "not finite" in str(e.value)
    ctx.stream_synchronize(rb["st"])
    after = handle.download()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes(), "a refused rebuild left the scene as it was"
    d.free()
    # the handle is destroyed before the scene
    assert lib.racc_hip_scene_free(ctx._h, scene._h) == -1 and b"racc_hip_refit_destroy comes first" in lib.racc_hip_last_error()
    assert ctx.intersect(scene, None, rays_at(v, idx, 64, 92)).dtype == synth.RESULT_DTYPE      # still there
    handle.destroy()
    with pytest.raises(ra.RaccError):      # the flag outlives the handle: the topology words are gone
        ctx.create_refit(scene, idx, len(v))
    scene.destroy()
    # a plain handle cannot rebuild
    plain_scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
    plain = ctx.create_refit(plain_scene, small_scene["indices"], len(small_scene["vertices"]))
    d, n = device_vertices(ctx, small_scene["vertices"])
    with pytest.raises(ra.RaccError) as e:
        plain.rebuild_device(d.ptr, n, stream=rb["st"])
    assert e.value.code == -1 and "racc_hip_refit_create" in str(e.value)
    with pytest.raises(ra.RaccError) as e:
        plain.rebuild(small_scene["vertices"])
    assert e.value.code == -1 and "racc_hip_refit_create" in str(e.value)
    with pytest.raises(ra.RaccError):
        plain.check_rebuild()
    d.free()
    plain.destroy()
    plain_scene.destroy()
    # what the host function refuses, creation refuses under its name
    with pytest.raises(ra.RaccError) as e:
        ctx.create_dynamic_scene(v[:3], idx[:3])
    assert e.value.code == -1 and "racc_host_scene_rebuild" in str(e.value)


def test_a_context_whose_uploads_carry_other_copies_is_refused():
    v, idx = soup(33, 93)
    ctx = ra.Context(device=0, kernel_variant=50)
    try:
        with pytest.raises(ra.RaccError) as e:
            ctx.create_dynamic_scene(v, idx)
        assert e.value.code == -1 and "would go stale" in str(e.value) and "45-53" in str(e.value)
    finally:
        ctx.destroy()
