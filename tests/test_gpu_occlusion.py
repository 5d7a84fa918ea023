"""Occlusion (any-hit) queries — racc_hip_occluded / racc_hip_occluded_device, occludedKernel (rayaccel_amd/csrc/racc_occlusion.inc).

The bar, in every test: occ == (oracle's closest-hit traversal reports a hit), for every ray, no allowances — the kernel enters the
children the reference's rule enters with the ray's own maxT and accepts a pair exactly where the reference's pair test does.  Every
output buffer carries 64 guard bytes (0xAB) behind `count`, which must come back untouched, and every output byte is 0 or 1."""
import ctypes as C

import numpy as np
import pytest

import rayaccel_amd as ra
from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, assert_bit_exact, book_rays, book_scene, comb_scene, far_scene, leaf_rays, leaf_scene, make_rays, sliver_scene

pytestmark = pytest.mark.gpu

GUARD = 64


def expected(blobs, rays):
    return (orc.traverse(blobs, rays, threads=16)["triangle"] != MISS).astype(np.uint8)


def issue(ctx, scene, rays, stream=None):
    """One device-resident launch, not waited for: (device rays, device output with its guard, count)."""
    n = len(rays)
    d_r = ctx.alloc(max(n, 1) * 32)
    if n:
        d_r.upload(rays)
    d_o = ctx.alloc(n + GUARD)
    d_o.upload(np.full(n + GUARD, 0xAB, np.uint8))
    ctx.occluded_device(scene, d_r.ptr, d_o.ptr, n, stream=stream)
    return d_r, d_o, n


def collect(launch, what=""):
    d_r, d_o, n = launch
    buf = d_o.download(np.uint8, n + GUARD)
    d_r.free(); d_o.free()
    return checked(buf, n, what)


def checked(buf, n, what=""):
    assert (buf[n:] == 0xAB).all(), "%s: guard bytes behind the output were written" % what
    assert (buf[:n] <= 1).all(), "%s: output bytes other than 0 and 1: %s" % (what, np.unique(buf[:n]))
    return buf[:n]


def device_path(ctx, scene, rays, stream=None, what=""):
    launch = issue(ctx, scene, rays, stream)
    ctx.stream_synchronize(stream)
    return collect(launch, what)


def host_path(ctx, scene, rays, what=""):
    buf = np.full(len(rays) + GUARD, 0xAB, np.uint8)
    ctx.occluded(scene, rays, out=buf)
    return checked(buf, len(rays), what)


def assert_exact(occ, want, what):
    bad = np.nonzero(occ != want)[0]
    assert len(bad) == 0 and np.array_equal(occ, want), "%s: %d of %d rays differ from the oracle, e.g. rays %s: got %s want %s" % (
        what, len(bad), len(want), bad[:8], occ[bad[:8]], want[bad[:8]])


@pytest.fixture(scope="module")
def occ(small_scene, small_host, small_default_host):
    """A context of this module's own (default options) with the small scene as both builders make it."""
    ctx = ra.Context(device=0)
    trees = {}
    for name, host in (("reference builder", small_host), ("quality tree", small_default_host)):
        trees[name] = dict(blobs=host.blobs(), scene=ctx.upload_scene(host.nodes, host.pairs, host.remap))
    prim, _ = synth.primary_rays(small_scene["camera"], 256, 256)
    rays = np.concatenate([prim, synth.random_rays(65536, 7)])
    yield dict(ctx=ctx, trees=trees, rays=rays, scene=trees["reference builder"]["scene"], blobs=trees["reference builder"]["blobs"])
    for t in trees.values():
        t["scene"].destroy()
    ctx.destroy()


# ------------------------------------------------------------------------------------------------------------ 1. small scene, both trees
@pytest.mark.parametrize("tree", ["reference builder", "quality tree"])
def test_small_scene_three_intervals(occ, tree):
    ctx, blobs, scene = occ["ctx"], occ["trees"][tree]["blobs"], occ["trees"][tree]["scene"]
    unbounded = occ["rays"].copy()
    unbounded["maxT"] = np.inf
    hits = orc.traverse(blobs, unbounded, threads=16)
    hit = np.nonzero(hits["triangle"] != MISS)[0]
    # the oracle's hits again with maxT = 0.5 t (nothing in reach), exactly t (closed interval, rounding) and 1.5 t, in rotation
    again = unbounded[hit].copy()
    t = hits["t"][hit]
    cls = np.arange(len(hit)) % 3
    again["maxT"] = np.where(cls == 0, np.float32(0.5) * t, np.where(cls == 1, t, np.float32(1.5) * t)).astype(np.float32)
    for what, rays in (("maxT = 1e6", occ["rays"]), ("maxT = +inf", unbounded), ("maxT = 0.5 t / t / 1.5 t", again)):
        want = expected(blobs, rays)
        assert 0.1 <= want.mean() <= 0.9, "%s: the oracle's hit fraction is %.3f" % (what, want.mean())
        if rays is again:
            at_t = want[cls == 1]
            assert at_t.any() and not at_t.all(), "maxT = t: the oracle gives one outcome only"
        got = device_path(ctx, scene, rays, what="%s, %s" % (tree, what))
        print("%s, %s: %d rays, occluded fraction %.3f" % (tree, what, len(rays), got.mean()))
        assert_exact(got, want, "%s, %s" % (tree, what))
        if rays is again:
            assert_exact(got[cls == 1], want[cls == 1], "%s, maxT = t" % tree)


# ------------------------------------------------------------------------------------------------------------ 2. edge cases through scene_upload
def _run_blobs(ctx, blobs, rays, what):
    scene = ctx.upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    want = expected(blobs, rays)
    assert_exact(device_path(ctx, scene, rays, what=what), want, what + " (device path)")
    assert_exact(host_path(ctx, scene, rays, what=what), want, what + " (host path)")
    info = scene.info
    scene.destroy()
    return want, info


def test_quad_kats(occ):
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 9], [6, 5, 9], [5, 6, 9]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.uint32)
    blobs = orc.build_scene(np.concatenate([v, np.ones((len(v), 1), np.float32)], 1), idx)
    rays = make_rays([[0.75, 0.25, -2], [0.25, 0.75, -2], [0.75, 0.25, 3],      # 0-2: both triangles of the quad, a back face
                      [0.75, 0.25, -2],                                         # 3: minT exactly at the hit: open interval
                      [0.75, 0.25, -2],                                         # 4: maxT exactly at a flat axis-aligned quad: the slab sentinel culls the box
                      [0.5, 0.5, -1],                                           # 5: on the shared diagonal
                      [5.25, 5.25, 0], [5.9, 5.9, 0],                           # 6,7: the unpaired triangle and its phantom second half
                      [0.75, 0.25, -2], [0.75, 0.25, -2],                       # 8,9: axis-parallel directions (0 / -0 -> +-1e-10)
                      [0.3, 0.6, -2], [-3, -3, -2]],                            # 10: plain hit; 11: misses everything
                     [[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [-0.0, 0.0, 1], [0, 0, 1], [0, 0, 1]])
    rays["minT"][3] = 2.0
    rays["maxT"][4] = 2.0
    want, _ = _run_blobs(occ["ctx"], blobs, rays, "quad KATs")
    assert list(want) == [1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0]
    # closed at maxT: a slanted triangle hit at exactly t = maxT, just below it, just above it; minT just below the hit
    v = np.array([[0, 0, 0], [2, 0, 2], [0, 2, 2], [5, 5, 9], [6, 5, 9], [5, 6, 9], [7, 7, 9], [8, 7, 9], [7, 8, 9]], np.float32)
    blobs = orc.build_scene(np.concatenate([v, np.ones((9, 1), np.float32)], 1), np.arange(9, dtype=np.uint32).reshape(3, 3))
    rays = make_rays([[0.5, 0.5, -2]] * 4, [[0, 0, 1]] * 4)
    rays["maxT"] = [3.0, 2.999, np.nextafter(np.float32(3.0), np.float32(4.0)), 1e6]
    rays["minT"][3] = np.nextafter(np.float32(3.0), np.float32(0.0))
    want, _ = _run_blobs(occ["ctx"], blobs, rays, "closed at maxT")
    assert list(want) == [1, 0, 1, 1]


@pytest.mark.parametrize("arrangement", ["row", "near_first", "near_last", "coincident"])
def test_hand_made_leaves(occ, arrangement):
    for n in (1, 2, 63, 64, 127):
        blobs, _ = leaf_scene(n, arrangement)
        want, info = _run_blobs(occ["ctx"], blobs, leaf_rays(n, arrangement), "leaf of %d pairs, %s" % (n, arrangement))
        assert info["max_leaf_pairs"] == n and want.any() and not want.all()


def test_book_of_126_pages(occ):
    sc = book_scene(126)
    host = ra.HostScene(sc["vertices"], sc["indices"], quality=0)
    want, info = _run_blobs(occ["ctx"], host.blobs(), book_rays(sc, 126), "book of 126 pages")
    assert info["max_leaf_pairs"] == 126 and want.sum() >= len(want) - 2


def test_comb_spills_the_stack(occ):
    blobs = comb_scene(40)
    n = 300
    o = np.stack([np.linspace(-20, 20, n), np.linspace(-15, 15, n), np.full(n, -10.0)], 1)
    beside = np.stack([np.linspace(52, 58, n), np.linspace(-15, 15, n), np.full(n, -10.0)], 1)      # inside every box, beside every triangle: 40 pushes, 40 pops
    rays = np.concatenate([make_rays(o, [[0, 0, 1]] * n), make_rays(beside, [[0, 0, 1]] * n),
                           make_rays(o, [[0, 0, 1]] * n, max_t=65.0),                               # every triangle lies behind maxT: the whole stack is unwound
                           make_rays(o, [[0, 0, 1]] * n, max_t=90.0)])                              # only the nearer ones are in reach
    _, _, _, depth = orc.traverse(blobs, rays, counters=True)
    assert depth.max() == 40
    scene = occ["ctx"].upload_scene(blobs["nodes"], blobs["pairs"], blobs["remap"])
    assert scene.info["inner_height"] == 40 and scene.info["spill_levels"] > 0      # 12 levels in LDS (the occlusion kernel's count as well), 28 in the spill
    scene.destroy()
    want, _ = _run_blobs(occ["ctx"], blobs, rays, "comb")
    assert want[:n].mean() > 0.9 and not want[n:3 * n].any() and want[3 * n:].mean() > 0.9


def test_slivers_and_far_coordinates(occ):
    sc = sliver_scene()
    rays = synth.random_rays(20000, seed=3, extent=50.0, ymax=50.0)
    rays["origin"][:, 1] -= 25
    want, _ = _run_blobs(occ["ctx"], orc.build_scene(sc["vertices"], sc["indices"]), rays, "slivers")
    assert want.sum() > 100
    sc = far_scene()
    prim, _ = synth.primary_rays(sc["camera"], 128, 128)
    rnd = synth.random_rays(6000, seed=9, extent=100.0, ymax=30.0)
    rnd["origin"] = rnd["origin"] * np.float32(1000.0) + np.array([5e4, 2e4, -7e4], np.float32)
    want, _ = _run_blobs(occ["ctx"], orc.build_scene(sc["vertices"], sc["indices"]), np.concatenate([prim, rnd]), "coordinates at 1e4..1e5")
    assert want.mean() > 0.3


def test_non_finite_rays(occ):
    """NaN, +inf and -inf in every field, one field of one ray at a time, on rays that are occluded when left alone."""
    base = synth.random_rays(4096, 7)
    base = base[expected(occ["blobs"], base) == 1][:32]
    cases = [(field, c, bad) for field, comps in (("origin", 3), ("dir", 3), ("minT", 1), ("maxT", 1)) for c in range(comps) for bad in (np.nan, np.inf, -np.inf)]
    rays = base[np.arange(len(cases)) % len(base)].copy()
    must_be_zero = []
    for i, (field, c, bad) in enumerate(cases):
        if field in ("origin", "dir"):
            rays[field][i, c] = bad
        else:
            rays[field][i] = bad
        must_be_zero.append(field != "maxT" or bool(np.isnan(bad)))
    rays = np.concatenate([rays, base])      # (and the untouched ones: all occluded)
    must_be_zero = np.array(must_be_zero + [False] * len(base))
    want = expected(occ["blobs"], rays)
    assert not want[must_be_zero].any() and want[-len(base):].all()
    for path in (device_path, host_path):
        got = path(occ["ctx"], occ["scene"], rays, what="non-finite rays")
        assert not got[must_be_zero].any()
        assert_exact(got, want, "non-finite rays")      # maxT = +-inf alone: whatever the oracle says


# ------------------------------------------------------------------------------------------------------------ 3. sizes
def test_sizes(occ):
    rays = synth.random_rays(100003, 5)
    want = expected(occ["blobs"], rays)
    for count in (1, 63, 64, 65, 100003):
        assert_exact(device_path(occ["ctx"], occ["scene"], rays[:count], what="count %d" % count), want[:count], "count %d, device path" % count)
        assert_exact(host_path(occ["ctx"], occ["scene"], rays[:count], what="count %d" % count), want[:count], "count %d, host path" % count)
    # count == 0 touches nothing: not the output (device or host), and no argument but the context and the scene is looked at
    assert len(device_path(occ["ctx"], occ["scene"], rays[:0], what="count 0")) == 0
    assert len(host_path(occ["ctx"], occ["scene"], rays[:0], what="count 0")) == 0
    occ["ctx"].occluded_device(occ["scene"], None, None, 0)
    buf = np.full(256, 0xAB, np.uint8)
    d_o = occ["ctx"].alloc(256)
    d_o.upload(buf)
    occ["ctx"].occluded_device(occ["scene"], None, d_o.ptr, 0)
    occ["ctx"].stream_synchronize(None)
    assert (d_o.download(np.uint8, 256) == 0xAB).all()
    d_o.free()


# ------------------------------------------------------------------------------------------------------------ 4. refill
def test_every_lane_is_refilled(occ):
    rays = synth.random_rays((1 << 20) + 37, 11)      # the grid holds 6 workgroups of 256 lanes per CU: every lane is refilled about three times
    want = expected(occ["blobs"], rays)
    assert 0.3 < want.mean() < 0.5
    assert_exact(device_path(occ["ctx"], occ["scene"], rays, what="1M + 37 rays"), want, "1M + 37 random rays")


# ------------------------------------------------------------------------------------------------------------ 5. paths
def test_paths_and_streams(occ):
    ctx, scene = occ["ctx"], occ["scene"]
    a, b = occ["rays"][:65536], occ["rays"][65536:]
    want_a, want_b = expected(occ["blobs"], a), expected(occ["blobs"], b)
    assert not np.array_equal(want_a, want_b)
    host = host_path(ctx, scene, a, what="host path")
    assert_exact(host, want_a, "host path")
    assert np.array_equal(device_path(ctx, scene, a, None, "NULL stream"), host)
    s1, s2 = ctx.create_stream(), ctx.create_stream()
    assert np.array_equal(device_path(ctx, scene, a, s1, "created stream"), host)
    la, lb = issue(ctx, scene, a, s1), issue(ctx, scene, b, s2)      # back to back, nothing waited for in between
    ctx.stream_synchronize(s1); ctx.stream_synchronize(s2)
    assert_exact(collect(la, "stream 1"), want_a, "two streams, launch 1")
    assert_exact(collect(lb, "stream 2"), want_b, "two streams, launch 2")
    ctx.destroy_stream(s1); ctx.destroy_stream(s2)


# ------------------------------------------------------------------------------------------------------------ 6. beside the chain
@pytest.mark.parametrize("occlusion_first", [False, True])
def test_beside_chained_closest_hit_batches(occ, small_host, occlusion_first):
    batches = [occ["rays"][:65536], synth.random_rays(65536, 21), synth.random_rays(65536, 22)]
    other = occ["rays"][65536:]
    refs = [orc.traverse(occ["blobs"], r, threads=16) for r in batches]
    want = expected(occ["blobs"], other)
    with ra.Context(device=0, chain_min_rays=1) as ctx:
        scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
        st = ctx.create_stream()
        d_rays, d_res = [], []
        for r in batches:
            d_rays.append(ctx.alloc(len(r) * 32)); d_rays[-1].upload(r)
            d_res.append(ctx.alloc(len(r) * 16))

        def chain():
            for dr, do, r in zip(d_rays, d_res, batches):
                ctx.intersect_device(scene, None, dr.ptr, do.ptr, len(r), lane=ra.LANE_AUTO)

        if occlusion_first:
            launch = issue(ctx, scene, other, st)
            chain()
        else:
            chain()
            launch = issue(ctx, scene, other, st)
        ctx.stream_synchronize(st)
        ctx.wait(ra.LANE_AUTO)
        for k, (do, r, ref) in enumerate(zip(d_res, batches, refs)):
            assert_bit_exact(do.download(orc.RESULT_DTYPE, len(r)), ref, "chained closest-hit batch %d beside an occlusion launch" % k)
        assert_exact(collect(launch, "beside the chain"), want, "occlusion launch beside three chained batches")
        for b in d_rays + d_res:
            b.free()
        ctx.destroy_stream(st)
        scene.destroy()


# ------------------------------------------------------------------------------------------------------------ 7. no state left behind
def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the engine itself is linked against."""
    ra.load_library()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_no_state_left_behind(occ, small_host):
    rays = occ["rays"][65536:]
    want = expected(occ["blobs"], rays)
    before = _free_device_memory()
    for _ in range(2):
        ctx = ra.Context(device=0)
        scene = ctx.upload_scene(small_host.nodes, small_host.pairs, small_host.remap)
        st = ctx.create_stream()
        d_r = ctx.alloc(len(rays) * 32)
        d_r.upload(rays)
        d_o = ctx.alloc(len(rays) + GUARD)
        d_o.upload(np.full(len(rays) + GUARD, 0xAB, np.uint8))
        for _launch in range(50):
            ctx.occluded_device(scene, d_r.ptr, d_o.ptr, len(rays), stream=st)
        ctx.stream_synchronize(st)
        assert_exact(checked(d_o.download(np.uint8, len(rays) + GUARD), len(rays), "50 launches"), want, "after 50 launches")
        d_r.free(); d_o.free()
        ctx.destroy_stream(st)
        scene.destroy()
        ctx.destroy()
    after = _free_device_memory()
    print("free device memory: %d bytes before the first create, %d after the second destroy (difference %d)" % (before, after, before - after))
    assert abs(before - after) <= 8 << 20
