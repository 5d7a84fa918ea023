"""CPU tests of the product's host-side scene build (rayaccel_amd/csrc/scene_build.cpp) against the
oracle's restatement of Bvh2.cpp / Scene.cpp: index and byte work, so BIT-EXACT."""
import os

import numpy as np
import pytest

import rayaccel_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import oracle as orc
from rayaccel_amd import synth


@pytest.mark.parametrize("kw", [dict(grid=8, boxes=2, quads=5), dict(grid=40, boxes=32, quads=100),
                                dict(grid=96, boxes=200, quads=900), dict(grid=3, boxes=0, quads=0)])
def test_builder_and_packer_match_oracle(kw):
    sc = synth.battlefield_synth(**kw)
    hs = ra.HostScene(sc["vertices"], sc["indices"])
    nodes, tris = orc.bvh2_build(sc["vertices"], sc["indices"])
    assert np.array_equal(hs.bvh_nodes.view(np.uint8), nodes.view(np.uint8))       # tree incl. float bounds
    assert np.array_equal(hs.bvh_triangles, tris)                                   # leaf triangle order
    blobs = orc.scene_pack(nodes, tris, sc["vertices"], sc["indices"])
    assert np.array_equal(hs.nodes.view(np.uint8), blobs["nodes"].view(np.uint8))   # 64 B inner nodes
    assert np.array_equal(hs.pairs.view(np.uint8), blobs["pairs"].view(np.uint8))   # 48 B pairs incl. padding
    assert np.array_equal(hs.remap, blobs["remap"]) and hs.pair_count == blobs["pair_count"]


def test_blob_invariants(small_scene, small_host):
    T = len(small_scene["indices"])
    hs = small_host
    assert (len(hs.pairs) * 3) % 32 == 0 and len(hs.pairs) > hs.pair_count          # Scene.cpp:334-338 (>=1 pad pair)
    assert np.array_equal(hs.pairs[hs.pair_count:].view(np.uint8).reshape(-1, 48), np.tile(hs.pairs[:1].view(np.uint8), (len(hs.pairs) - hs.pair_count, 1)))
    ids = hs.remap & 0x3FFFFFFF
    second_real = (hs.remap[1::2] >> 30) != 0                                       # second slot used iff edge code != 0
    used = np.concatenate([ids[0::2], ids[1::2][second_real]])
    assert np.array_equal(np.sort(used), np.arange(T))                               # every triangle exactly once
    kids = np.concatenate([hs.nodes["first"], hs.nodes["last"]])
    leaves = kids[(kids & 0x80000000) == 0]
    first, cnt = leaves & 0xFFFFFF, leaves >> 24
    order = np.argsort(first)
    assert cnt.min() >= 1 and cnt.max() <= 127
    assert np.array_equal(first[order][1:], (first + cnt)[order][:-1]) and (first + cnt).max() == hs.pair_count   # ranges tile the pairs
    inner = kids[(kids & 0x80000000) != 0] & 0x7FFFFFFF
    assert np.array_equal(np.sort(inner), np.arange(1, len(hs.nodes)))               # a tree: every inner node but the root has one parent


def test_pairing_rate_on_connected_mesh(small_host, small_scene):
    assert small_host.pair_count < 0.56 * len(small_scene["indices"])                # ~0.5 pairs/triangle when well connected


def test_build_is_deterministic(small_scene):
    a = ra.HostScene(small_scene["vertices"], small_scene["indices"])
    b = ra.HostScene(small_scene["vertices"], small_scene["indices"])
    assert np.array_equal(a.nodes.view(np.uint8), b.nodes.view(np.uint8)) and np.array_equal(a.remap, b.remap)


def test_error_behaviour():
    lib = ra.load_library()
    import ctypes as C
    v = np.zeros((8, 4), np.float32)
    h = C.c_void_p()
    idx = np.arange(6, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.racc_host_scene_build(vp(v), 8, vp(idx), 5, C.byref(h)) == -1                 # index_count % 3 (Scene.cpp:186)
    assert b"multiple of 3" in lib.racc_hip_last_error()
    assert lib.racc_host_scene_build(vp(v), 8, vp(idx), 6, C.byref(h)) == -4 and not h      # 2 triangles: root would be a leaf
    bad = np.array([0, 1, 99, 0, 1, 2, 1, 2, 3], np.uint32)
    assert lib.racc_host_scene_build(vp(v), 8, vp(bad), 9, C.byref(h)) == -1                 # vertex index out of range
    mis = np.zeros(64, np.float32)
    off = 1 if mis.ctypes.data % 16 == 0 else 0
    addr = mis.ctypes.data + 4 * off
    assert addr % 16 != 0
    assert lib.racc_host_scene_build(C.c_void_p(addr), 8, vp(np.arange(9, dtype=np.uint32) % 8), 9, C.byref(h)) == -1   # Scene.cpp:187
    with pytest.raises(ra.RaccError):
        ra.HostScene(v, idx[:3])


def test_path_tracer_shared_arithmetic():
    """pt_shade.h (compiled verbatim by the host and the device consumer): the polynomial sin/cos that replaces the two
    math libraries stays within 2e-7 of the true value on [0, 1), is exact at the quadrant boundaries, and the counter RNG
    produces 24-bit uniforms in [0, 1) with a flat histogram."""
    import ctypes as C
    from rayaccel_amd import engine
    engine.load_library()
    lib = C.CDLL(engine.PT_LIB_PATH)
    r = np.concatenate([np.arange(0, 1 << 16, dtype=np.float32) / np.float32(1 << 16),
                        np.random.default_rng(5).random(200000, dtype=np.float32),
                        np.array([0.0, 0.25, 0.5, 0.75, np.nextafter(np.float32(1), np.float32(0))], np.float32)])
    s, c = np.zeros_like(r), np.zeros_like(r)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.racc_pt_test_sincos2pi(vp(r), C.c_uint32(len(r)), vp(s), vp(c))
    ang = 2.0 * np.pi * r.astype(np.float64)
    assert np.abs(s - np.sin(ang)).max() < 2e-7 and np.abs(c - np.cos(ang)).max() < 2e-7
    assert np.abs(s.astype(np.float64) ** 2 + c.astype(np.float64) ** 2 - 1).max() < 5e-7
    assert (s[-5], c[-5]) == (0.0, 1.0) and (s[-4], c[-4]) == (1.0, 0.0) and (s[-3], c[-3]) == (0.0, -1.0) and (s[-2], c[-2]) == (-1.0, 0.0)
    u = np.zeros(1 << 18, np.float32)
    lib.racc_pt_test_uniform(C.c_uint32(12345), C.c_uint32(7), C.c_uint32(2), C.c_uint32(3), C.c_uint32(len(u)), vp(u))
    assert u.min() >= 0.0 and u.max() < 1.0 and np.all(u * (1 << 24) == np.floor(u * (1 << 24)))
    hist = np.bincount((u * 64).astype(int), minlength=64)
    assert hist.min() > 0.9 * len(u) / 64 and hist.max() < 1.1 * len(u) / 64 and abs(u.mean() - 0.5) < 2e-3


def test_build_is_identical_for_any_thread_count(monkeypatch):
    """The thread-pool build allocates provisional node ids in timing-dependent order; the renumber pass must make the
    blobs byte-identical to the single-threaded build (and therefore to the oracle's)."""
    sc = synth.battlefield_synth(grid=96, boxes=300, quads=1500)          # ~26k triangles: several pool tasks
    blobs = {}
    for threads in ("1", "3", "8"):
        monkeypatch.setenv("RACC_BUILD_THREADS", threads)
        h = ra.HostScene(sc["vertices"], sc["indices"])
        blobs[threads] = (h.nodes.tobytes(), h.pairs.tobytes(), h.remap.tobytes())
    assert blobs["1"] == blobs["3"] == blobs["8"]
    ref = orc.build_scene(sc["vertices"], sc["indices"])
    assert blobs["8"][0] == ref["nodes"].tobytes() and blobs["8"][1] == ref["pairs"].tobytes() and blobs["8"][2] == ref["remap"].tobytes()


def test_non_finite_vertices_are_refused(small_scene):
    """A NaN/inf coordinate turns the SAH costs into NaN (the reference would index sorted[-1], Bvh2.cpp:467-485 never sees
    it coming): the host build refuses such input."""
    import rayaccel_amd as ra
    for bad in (np.nan, np.inf, -np.inf, 3e19):
        v = small_scene["vertices"].copy()
        v[17, 1] = bad
        with pytest.raises(ra.RaccError):
            ra.HostScene(v, small_scene["indices"])


def test_material_sampling_matches_the_reference_restatement():
    """the path-tracing consumer's BSDF sampling (pt_shade.h sampleMaterial, a scalar re-derivation) held to the
    oracle's operation-by-operation restatement of the reference's ReflectiveDiffuseMaterial::sample8 (Renderer/Materials.cpp:39-151):
    the same choice between mirror and diffuse direction, the same colour weights, the same mirror direction, the same diffuse
    direction when both use exact sine/cosine — and a diffuse direction within the error of the reference's own parabola
    sine/cosine (Materials.cpp:11-29, up to 0.056) otherwise: that substitution is pt_shade.h's one deliberate deviation."""
    import ctypes as C
    from rayaccel_amd import engine
    from oracle import oracle as orc
    engine.load_library()
    lib = C.CDLL(engine.PT_LIB_PATH)
    rng = np.random.default_rng(17)
    n = 20000
    normal = rng.normal(size=(n, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True).astype(np.float32)
    wo = rng.normal(size=(n, 3)).astype(np.float32)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True).astype(np.float32)
    flip = (normal * wo).sum(1) < 0          # the consumer hands the material a normal on the viewer's side (PathTracingRenderer.cpp:230-260)
    normal[flip] *= -1
    rnd = rng.random((n, 3), dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for ke in ([0.6, 0.5, 0.4, 1.5], [0.9, 0.9, 0.9, 1.0 / 1.5], [0.05, 0.1, 0.7, 2.4]):        # kd + eta (Renderer/main.cpp:165-168 style; eta < 1: total internal reflection occurs)
        ke = np.array(ke, np.float32)
        wi, col, alive = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        lib.racc_pt_test_sample_material(vp(ke), vp(rnd), vp(normal), vp(wo), C.c_uint32(n), vp(wi), vp(col), vp(alive))
        assert alive.all()
        wi_e, col_e, dif_e = orc.pt_sample_material(ke, rnd, normal, wo, exact_trig=True)
        wi_a, col_a, dif_a = orc.pt_sample_material(ke, rnd, normal, wo, exact_trig=False)
        assert np.array_equal(dif_e, dif_a)                              # the choice does not depend on the trig functions
        np.testing.assert_allclose(col, col_e, rtol=2e-4, atol=1e-6)      # colour weights: Materials.cpp:121-141 (Fresnel near grazing incidence cancels: 1e-4)
        np.testing.assert_allclose(wi, wi_e, rtol=0, atol=3e-6)           # mirror direction and exact-trig diffuse direction
        refl = dif_e == 0
        assert 0.02 < refl.mean() < 0.98 or ke[3] < 1.0
        np.testing.assert_allclose(wi[refl], wi_a[refl], rtol=0, atol=3e-6)
        cosang = np.clip((wi[~refl].astype(np.float64) * wi_a[~refl]).sum(1), -1, 1)
        assert np.degrees(np.arccos(cosang)).max() < 4.0                  # the reference's parabola sine/cosine: <= 0.056 off before normalisation


@pytest.fixture(scope="module")
def tsan_builds():
    """`make tsan` on demand (the sanitizer builds are test artefacts, not part of the product's `all`); a host without
    libtsan skips the two tests instead of failing the library build."""
    import subprocess
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rayaccel_amd", "csrc"), "tsan"], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("ThreadSanitizer build not possible here: " + p.stderr[-300:])


def test_group_workers_under_thread_sanitizer(tsan_builds):
    """The device group's persistent per-GPU worker threads (rayaccel_amd/csrc/racc_group_worker.h) in a GPU-free -fsanitize=thread
    harness (`make tsan`, tests/cpp/group_worker_tsan.cpp): four caller threads, three workers, post / drain / collect as
    racc_hip_group_intersect_device + racc_hip_group_wait do.  No race, no lost job, failures collected once."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "group_worker_tsan")
    assert os.path.exists(exe), "make -C rayaccel_amd/csrc tsan"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"))
    assert p.returncode == 0 and "ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]


def test_scene_build_under_thread_sanitizer(tsan_builds):
    """The host scene build — the thread-pool BVH2 build and the quality mode's parallel subtree phases (sibling subtrees share the node
    above them: ADVICE r05) — under -fsanitize=thread (`make tsan`, tests/cpp/scene_build_tsan.cpp): no race, and the blobs of a 6-thread
    build equal those of a 1-thread build."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "scene_build_tsan")
    assert os.path.exists(exe), "make -C rayaccel_amd/csrc tsan"
    p = subprocess.run([exe, "96", "6"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"))
    assert p.returncode == 0 and "ThreadSanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]


def test_the_build_at_the_pair_limit_falls_back_to_one_reference_per_triangle(tmp_path):
    """A leaf reference holds a pair index in 24 bits (Scene.cpp:294-312).  A scene whose pairs fit but not with the extra references of the
    spatial splits (battlefield-synth-XL is 10 % away from that) must come out as the build without splits gives it, not fail: the limit
    lowered to 2,000 pairs in a build of scene_build.cpp of its own (tests/cpp/scene_build_limit.cpp) — library's budget, a caller's budget,
    a caller without options; and the error past the limit."""
    import subprocess
    exe = str(tmp_path / "scene_build_limit")
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wno-subobject-linkage", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "scene_build_limit.cpp"),
                        "-o", exe, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "the blobs of the build without splits" in p.stdout and "rc -4" in p.stdout


def _device_to_reference(dev):
    """64 B device records (racc_host_scene_device_nodes) back into the reference's node format (Scene.cpp:73-78)."""
    out = np.zeros(len(dev), ra.engine.GPU_NODE_DTYPE)
    out["first"], out["last"] = dev[:, 0], dev[:, 1]
    pl = dev[:, 4:16].view(np.float32)
    out["leftMin"], out["leftMax"] = pl[:, 0:6:2], pl[:, 1:6:2]
    out["rightMin"], out["rightMax"] = pl[:, 6:12:2], pl[:, 7:12:2]
    return out


@pytest.mark.parametrize("order", [0, 1])
def test_device_node_order_is_the_same_tree(small_scene, small_host, order):
    """racc_hip_scene_upload re-numbers the nodes (round 4: every 128 B line = a node and the child a ray most likely enters next).
    The re-numbered records, read back as a reference-format blob, must give the oracle the same hits bit for bit — same boxes, same
    first/last roles, same leaves — and the line structure must be what the header promises."""
    dev = small_host.device_nodes(order)
    n = len(small_host.nodes)
    inner = lambda r: (r & 0x80000000) != 0
    used = np.zeros(len(dev), bool)
    used[0] = True
    for col in (0, 1):
        idx = dev[inner(dev[:, col]), col] & 0x7FFFFFFF
        assert idx.max() < len(dev) and not used[idx].any()       # every record referenced once
        used[idx] = True
    assert used.sum() == n and not dev[~used].any()               # the rest is all-zero padding
    assert len(dev) - n <= max(2, n // 50)
    rays = np.concatenate([synth.primary_rays(small_scene["camera"], 128, 128)[0], synth.random_rays(6000, seed=3, ymax=30.0)])
    a = orc.traverse(small_host.blobs(), rays, env=small_scene["env"])
    b = orc.traverse(dict(small_host.blobs(), nodes=_device_to_reference(dev)), rays, env=small_scene["env"])
    assert a.tobytes() == b.tobytes()
    if order == 1:
        ev = np.arange(0, len(dev) - 1, 2)
        child_behind = (dev[ev, 0] == (0x80000000 | (ev + 1))) | (dev[ev, 1] == (0x80000000 | (ev + 1)))
        childless = ~inner(dev[:, 0]) & ~inner(dev[:, 1])
        assert (child_behind | (childless[ev] & (childless[ev + 1] | ~used[ev + 1]))).all()      # a line = parent + child, or two childless nodes
        assert child_behind.mean() > 0.5
        both = inner(dev[ev, 0]) & inner(dev[ev, 1]) & child_behind                                # the larger of two inner children sits behind its parent
        pl = dev[:, 4:16].view(np.float32)
        def area(rows, o):
            x, y, z = (pl[rows, o + 1] - pl[rows, o]).astype(np.float64), (pl[rows, o + 3] - pl[rows, o + 2]).astype(np.float64), (pl[rows, o + 5] - pl[rows, o + 4]).astype(np.float64)
            return x * y + x * z + y * z
        rows = ev[both]
        first_behind = dev[rows, 0] == (0x80000000 | (rows + 1))
        assert ((area(rows, 0) >= area(rows, 6)) == first_behind).all()


def test_eight_wide_shading_is_the_scalar_shading_bit_for_bit():
    """pt_shade.h's AVX2 form of a surface interaction (ptshade::simd::shadeSurface8: what the host path-tracing consumer's shade callback runs,
    eight hits at a time — the reference's shading is 8-wide AVX2 too, PathTracingRenderer.cpp:72-566) against the scalar form it shares with
    the device consumer: alive flag, next ray and next payload of 1.2 million random interactions — all four materials, both tangent frames,
    total internal reflection, dying paths, non-finite origins — identical in every bit."""
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, "rayaccel_amd", "libracc_pathtracer.so"))
    lib.racc_pt_test_shade8.restype = C.c_longlong
    lib.racc_pt_test_shade8.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    for seed in (1, 2, 3):
        alive = C.c_uint32(0)
        bad = lib.racc_pt_test_shade8(400000, seed, C.byref(alive))
        assert bad == 0, "seed %d: %d interactions differ" % (seed, bad)          # (-1: a build without AVX2 — the Makefile compiles with -mavx2 -mfma)
        assert 100000 < alive.value < 300000                                       # both outcomes well represented


@pytest.mark.parametrize("top", [128, 524, 7])
def test_device_node_order_with_a_cached_top_is_the_same_tree(small_scene, small_host, top):
    """Order 2 (kernel variants 60-63, whose workgroups hold device records [0, CACHE) in LDS): the `top` nodes with the largest own boxes
    first — a connected top of the tree, root at 0, areas falling — and the subtrees below it in order 1's line pairs.  Same tree for the
    oracle bit for bit; asked for as racc_host_scene_device_nodes(order = top)."""
    dev = small_host.device_nodes(top)
    n = len(small_host.nodes)
    inner = lambda r: (r & 0x80000000) != 0
    used = np.zeros(len(dev), bool)
    used[0] = True
    parent = np.full(len(dev), -1, np.int64)
    for col in (0, 1):
        rows = np.nonzero(inner(dev[:, col]))[0]
        idx = dev[rows, col] & 0x7FFFFFFF
        assert idx.max() < len(dev) and not used[idx].any()
        used[idx] = True
        parent[idx] = rows
    assert used.sum() == n and not dev[~used].any()
    assert len(dev) - n <= max(3, n // 50)
    rays = np.concatenate([synth.primary_rays(small_scene["camera"], 128, 128)[0], synth.random_rays(6000, seed=3, ymax=30.0)])
    a = orc.traverse(small_host.blobs(), rays, env=small_scene["env"])
    b = orc.traverse(dict(small_host.blobs(), nodes=_device_to_reference(dev)), rays, env=small_scene["env"])
    assert a.tobytes() == b.tobytes()
    k = min(top, n)
    assert used[:k].all() and (parent[1:k] < np.arange(1, k)).all()          # connected: every top node's parent sits before it
    pl = dev[:, 4:16].view(np.float32).astype(np.float64)
    own = lambda r: (np.maximum(pl[r, 1:6:2], pl[r, 7:12:2]) - np.minimum(pl[r, 0:6:2], pl[r, 6:12:2]))
    d = own(np.arange(k))
    area = d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2] + d[:, 1] * d[:, 2]
    assert (np.diff(area) <= 1e-9 * area[:-1]).all()                          # largest boxes first
    rest = np.arange(k, len(dev))
    d = own(rest[used[rest]])
    assert (d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2] + d[:, 1] * d[:, 2]).max() <= area[-1] * (1 + 1e-9)      # ... and nothing below the top is larger than its last node
    start = k + (k & 1)
    ev = np.arange(start, len(dev) - 1, 2)
    child_behind = (dev[ev, 0] == (0x80000000 | (ev + 1))) | (dev[ev, 1] == (0x80000000 | (ev + 1)))
    childless = ~inner(dev[:, 0]) & ~inner(dev[:, 1])
    assert (child_behind | (childless[ev] & (childless[ev + 1] | ~used[ev + 1]))).all()                      # behind the top: a line = parent + child, or two childless nodes


@pytest.mark.parametrize("cfg", [dict(RACC_CPU_THREADS="5", RACC_BATCH="2048", RACC_IN_FLIGHT="60000", RACC_GPU_THREADS="3", RACC_SHADE_BATCH="500"),
                                 dict(RACC_CPU_THREADS="2", RACC_BATCH="16384", RACC_IN_FLIGHT="16384", RACC_GPU_THREADS="4", RACC_DEVICES="0,1"),
                                 dict(RACC_CPU_THREADS="7", RACC_BATCH="700", RACC_IN_FLIGHT="20000", RACC_GPU_THREADS="1", RACC_SHADE_BATCH="64")])
def test_scheduler_under_thread_sanitizer(tmp_path, small_scene, cfg, tsan_builds):
    """SURVEY §5's -fsanitize=thread build of the host scheduler (`make tsan`): rayaccel_amd/csrc/racc_api.cpp — CPU workers, GPU
    submission threads, the four stream lists, the callback contract — and the test driver of tests/test_gpu_render.py, instrumented,
    over tests/cpp/fake_engine.cpp (a stand-in for the C-ABI that traces nothing and sleeps a pseudo-random time per launch; the
    real engine under the same driver is tests/test_gpu_render.py's job on the GPU box).  Starved and multi-device configurations, two
    frames each: no data race, no lock-order inversion, every spawned ray shaded exactly once."""
    import json
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "render_check_tsan")
    assert os.path.exists(exe), "make -C rayaccel_amd/csrc tsan"
    scene_file, out_file = os.path.join(str(tmp_path), "scene.bin"), os.path.join(str(tmp_path), "out.bin")
    synth.write_scene_bin(scene_file, small_scene)
    p = subprocess.run([exe, scene_file, out_file, "256", "256", "3", "2"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", **cfg))
    assert p.returncode == 0 and "ThreadSanitizer" not in p.stderr, p.stdout[-500:] + p.stderr[-4000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["raysTraced"] == info["shaded"] > 4 * 128 * 128       # primaries + two generations of bounces, none lost


def test_device_node_order_on_degenerate_trees():
    """The line-paired order on shapes a SAH build never makes: a 40-deep left-leaning comb (every node has ONE inner child: all lines
    are parent + child), a single inner node, tiny meshes (6 ... 131 unconnected triangles).  Same hits as the blob, record counts within bounds."""
    from helpers import comb_scene, make_rays
    comb = comb_scene(40)
    dev = ra.engine.device_nodes(comb["nodes"], len(comb["pairs"]), len(comb["remap"]), 1)
    assert len(dev) == 40 and dev[0, 0] == (0x80000000 | 1)            # root first, its chain link behind it
    o = np.stack([np.linspace(-20, 20, 64), np.linspace(-15, 15, 64), np.full(64, -10.0)], 1)
    rays = make_rays(o, [[0, 0, 1]] * 64)
    assert orc.traverse(comb, rays).tobytes() == orc.traverse(dict(comb, nodes=_device_to_reference(dev)), rays).tobytes()
    rng = np.random.default_rng(1)
    for tris in (6, 9, 17, 40, 131):
        centres = np.repeat(rng.uniform(-10, 10, (tris, 3)), 3, axis=0)      # small triangles far apart: the SAH splits down to the 2-triangle leaves
        v = np.concatenate([(centres + rng.uniform(-0.3, 0.3, (tris * 3, 3))).astype(np.float32), np.ones((tris * 3, 1), np.float32)], 1)
        idx = np.arange(tris * 3, dtype=np.uint32).reshape(tris, 3)
        host = ra.HostScene(v, idx)
        for order in (0, 1):
            dev = host.device_nodes(order)
            assert len(host.nodes) <= len(dev) <= len(host.nodes) + 1
            r = synth.random_rays(2000, seed=tris, extent=12.0, ymax=10.0)
            assert orc.traverse(host.blobs(), r).tobytes() == orc.traverse(dict(host.blobs(), nodes=_device_to_reference(dev)), r).tobytes()
