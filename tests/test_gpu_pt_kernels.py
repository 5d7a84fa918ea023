"""GPU tests of the two path-tracing kernels (rayaccel_amd/csrc/pt_device.hip: ptGenKernel, ptShadeKernel) on arrays the tests
supply, record by record: against oracle/pt_reference.py (float64, written from the reference's lines), bit for bit against the
host consumer's hooks, and — for a real render — round by round, so that with the traversal oracle the whole device path tracer
is tied to something other than itself.  Inputs, tolerances and the comparison: tests/pt_inputs.py."""
import numpy as np
import pytest

import pt_inputs as pin
from oracle import pt_reference as ref
from rayaccel_amd import engine, synth

pytestmark = pytest.mark.gpu

CAM = np.array([1.5, 20.0, -60.0, 0.0011, 0.0, 0.0002, 0.0, -0.0011, 0.0001, -0.9, 0.55, 0.8], np.float32)      # origin, right, up, view


@pytest.fixture(scope="module")
def table(small_scene):
    return pin.tri_table(small_scene)


@pytest.fixture(scope="module")
def compute_units():
    return engine.pt_device_compute_units(0)      # the device properties' count, through the consumer's own library


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _scatter(dev, rec):
    """The compacted survivors of a device pass put back at their records' places, by the key (pixel, sample): every key must
    be one of the inputs' and appear once.  Returns (alive, rays, paths), entry i belonging to record i."""
    n = len(rec["samples"])
    assert dev["count"] == len(dev["rays"]) == len(dev["paths"]) == len(dev["samples"]) <= n
    key_in = (rec["paths"]["pixelDepth"] & np.uint32(0xFFFFFF)).astype(np.uint64) << np.uint64(32) | rec["samples"].astype(np.uint64)
    assert len(np.unique(key_in)) == n
    key_out = (dev["paths"]["pixelDepth"] & np.uint32(0xFFFFFF)).astype(np.uint64) << np.uint64(32) | dev["samples"].astype(np.uint64)
    assert len(np.unique(key_out)) == len(key_out), "a survivor was written twice (or two slots collided)"
    order = np.argsort(key_in)
    pos = np.searchsorted(key_in[order], key_out)
    assert (pos < n).all() and np.array_equal(key_in[order][np.minimum(pos, n - 1)], key_out), "a survivor carries a key no input has"
    at = order[pos]
    alive = np.zeros(n, bool)
    alive[at] = True
    rays, paths = np.zeros(n, engine.RAY_DTYPE), np.zeros(n, engine.PATH_DTYPE)
    rays[at], paths[at] = dev["rays"], dev["paths"]
    assert np.array_equal(dev["samples"], rec["samples"][at])          # every survivor keeps its sample index
    return alive, rays, paths


def _shade_counts(cus):
    return [1, 64, 1023, 1024, 1025, 3 * 1024 + 5, cus * 2 * 1024 + 1024 + 37]      # the last: a second, partly empty sweep of the grid-stride loop


@pytest.fixture(scope="module")
def passes(table, compute_units):
    """Every batch size once through the device kernel, the host hook and the reference (shared by the tests below)."""
    tris, names = table
    out = {}
    for count in _shade_counts(compute_units):
        rec = pin.make_records(count, tris, names)
        dev = engine.pt_device_shade(tris, pin.MATERIALS, pin.MAX_DEPTH, rec["rays"], rec["hits"], rec["paths"], rec["samples"], pin.FRAME_WORDS)
        host = engine.pt_host_shade(tris, pin.MATERIALS, pin.MAX_DEPTH, rec["rays"], rec["hits"], rec["paths"], rec["samples"])
        out[count] = (rec, dev, host, pin.reference_pass(tris, pin.MATERIALS, pin.MAX_DEPTH, rec))
    return out


def test_shade_kernel_matches_the_reference_record_by_record(passes, compute_units):
    """(a) count, keys, sample indices, next rays and payloads within the tolerances, exact minT / maxT / pixelDepth, and the
    frame = the exact integer sum of the reference's miss contributions, word for word, zero elsewhere.
    (Ranking the ballot prefix with <= fails here on the first batch.  Leaving out the loop's last __syncthreads() does NOT: a
    build without it passed all seven batches, the two-sweep one included — a wave would have to shade a whole next sweep while
    another still sums the per-wave counts.)"""
    assert compute_units * 2 * 1024 < max(passes)
    for count, (rec, dev, host, exp) in passes.items():
        alive, rays, paths = _scatter(dev, rec)
        pin.compare_with_reference("ptShadeKernel, %d records" % count, alive, rays, paths, rec, exp)
        frame = ref.accumulate_misses(pin_daz_hits(rec), pin_daz_paths(rec), pin.FRAME_WORDS)
        assert np.array_equal(dev["frame"], frame), "frame differs from the exact sum at %d words" % (dev["frame"] != frame).sum()
        if count >= 3000:
            p0 = 123 * pin.FRAME_W + 45
            assert (frame[p0 * 3:p0 * 3 + 3] != 0).all() and (rec["paths"]["pixelDepth"] & 0xFFFFFF == p0).sum() >= 1024


def pin_daz_hits(rec):
    h = rec["hits"].copy()
    for f in ("t", "u", "v"):
        h[f] = pin.daz(h[f])
    return h


def pin_daz_paths(rec):
    p = rec["paths"].copy()
    p["weight"] = pin.daz(p["weight"])
    return p


def test_shade_kernel_equals_the_host_consumer_bit_for_bit(passes):
    """(b) the project's own claim, on records instead of constant-environment frames: alive flags, next rays, payloads and
    the accumulated contributions of the device kernel and of the host hook are identical in every bit."""
    for count, (rec, dev, host, exp) in passes.items():
        alive, rays, paths = _scatter(dev, rec)
        assert np.array_equal(alive, host["alive"]), "alive flags differ at records %s" % np.nonzero(alive != host["alive"])[0][:8]
        assert np.array_equal(_bits(rays), _bits(host["rays"])) and np.array_equal(_bits(paths), _bits(host["paths"]))
        frame = np.zeros(pin.FRAME_WORDS, np.int64)
        miss = rec["hits"]["triangle"] == ref.MISS
        pixel = (rec["paths"]["pixelDepth"][miss] & np.uint32(0xFFFFFF)).astype(np.int64)
        for ch in range(3):
            ok = host["valid"][miss][:, ch]
            np.add.at(frame, pixel[ok] * 3 + ch, host["contrib"][miss][ok, ch])
        assert np.array_equal(dev["frame"], frame)


@pytest.mark.parametrize("region", [(128, 128, 1, 128), (256, 128, 3, 300), (256, 256, 9, 256)])
def test_gen_kernel(region, compute_units):
    """(c) every (pixel, sample) of the region once, pixel = y * width + x with the FRAME's width, lanes 0..63 of a wave one
    8x8 pixel block, rays bit-identical to the host hook's and within tolerance of the float64 camera, weights 1, depth 0.
    (256 x 256 x 9 exceeds CUs * 8 * 256 threads: the grid-stride loop wraps.)"""
    w, h, samples, width = region
    first = 5
    n = w * h * samples
    if samples == 9:
        assert n > compute_units * 8 * 256
    rays, paths, sidx = engine.pt_device_gen(CAM, width, w, h, first, samples)
    pixel = paths["pixelDepth"]
    assert (pixel >> 24 == 0).all()
    x, y = pixel % width, pixel // width
    assert (x < w).all() and (y < h).all()
    assert np.array_equal(sidx, first + np.arange(n, dtype=np.uint32) // (w * h))          # sample-major
    key = sidx.astype(np.uint64) * np.uint64(1 << 24) + pixel
    want = (first + np.repeat(np.arange(samples, dtype=np.uint64), w * h)) * np.uint64(1 << 24) + np.tile((np.arange(h, dtype=np.uint64)[:, None] * width + np.arange(w, dtype=np.uint64)[None, :]).ravel(), samples)
    assert np.array_equal(np.sort(key), np.sort(want))                                       # each (pixel, sample) exactly once
    # a wave = 64 consecutive records = one 8x8 block, row-major inside it
    bx, by = x.reshape(-1, 64), y.reshape(-1, 64)
    lane = np.arange(64)
    assert (bx[:, :1] % 8 == 0).all() and (by[:, :1] % 8 == 0).all()
    assert np.array_equal(bx, bx[:, :1] + (lane & 7)[None, :]) and np.array_equal(by, by[:, :1] + (lane >> 3)[None, :])
    h_rays, h_paths = engine.pt_host_primary_rays(CAM, x, y, pixel, sidx)
    assert np.array_equal(_bits(rays), _bits(h_rays)) and np.array_equal(_bits(paths), _bits(h_paths))
    exp = ref.primary_ray(CAM, x, y, pixel, sidx)
    dev = np.abs(rays["dir"].astype(np.float64) - exp["dir"]).max()
    print("ptGenKernel %s: largest direction deviation %.3g (bound %.3g)" % (region, dev, pin.TOL_DIR))
    assert dev <= pin.TOL_DIR
    for f in ("origin", "minT", "maxT"):
        assert np.array_equal(rays[f].view(np.uint32), exp[f].view(np.uint32)), f
    assert (paths["weight"] == 1.0).all() and np.array_equal(pixel, exp["pixelDepth"])


def test_a_render_round_by_round(tmp_path, small_scene, small_default_host):
    """(d) the small scene at 256 x 128, 2 spp (one pipeline: rounds are sequential), depth 4, under an environment that
    varies in both axes and per channel.  Renders are reproducible, so the one-shot capture is armed for one round per render.
    Round k + 1's (ray, payload, sample) set, keyed by (pixel, sample), is what the reference derives from round k's captured
    records; the frame is EXACTLY the sum over all rounds of the captured misses' contributions; each round's hits are the
    traversal oracle's, bit for bit."""
    from oracle import oracle as orc
    from helpers import assert_bit_exact
    W, H, SPP, DEPTH = 256, 128, 2, 4
    sc = dict(small_scene)
    ey, ex = np.meshgrid(np.linspace(0, 1, 16, dtype=np.float32), np.linspace(0, 1, 32, dtype=np.float32), indexing="ij")
    env = np.zeros((16, 32, 4), np.float32)
    env[..., 0], env[..., 1], env[..., 2] = 0.25 + 1.5 * ex, 0.5 + 2.0 * ey * ey, 2.5 - ex - ey
    sc["env"] = env
    path = str(tmp_path / "scene.bin")
    synth.write_scene_bin(path, sc)
    tris = pin.scene_file_tris(path)
    blobs = small_default_host.blobs()
    cap = W * H * SPP
    rounds, frame0 = [], None
    for k in range(DEPTH + 2):
        rays, hits, paths, samples, count = engine.path_trace_capture_round_paths(k, cap)
        img, st = engine.path_trace(path, W, H, 0, SPP, max_depth=DEPTH, shading="gpu")
        if frame0 is None:
            frame0 = img
        assert np.array_equal(img, frame0)                                     # reproducible
        n = int(count.value)
        if n == 0:
            assert k == st["reserved"]                                         # rounds executed
            break
        rounds.append(dict(rays=rays[:n], hits=hits[:n], paths=paths[:n], samples=samples[:n], cls=np.array(["render"] * n, dtype=object)))
    engine.path_trace_capture_round(0, 0)                                      # disarm
    assert len(rounds) == st["reserved"] >= 3 and len(rounds[0]["rays"]) == cap and sum(len(r["rays"]) for r in rounds) == st["rays_traced"]
    total = np.zeros(W * H * 3, np.int64)
    for k, rec in enumerate(rounds):
        assert ((rec["paths"]["pixelDepth"] >> 24) == k).all()
        assert_bit_exact(rec["hits"], orc.traverse(blobs, rec["rays"], env=env), "render round %d (%d rays)" % (k, len(rec["rays"])))
        total += ref.accumulate_misses(rec["hits"], rec["paths"], W * H * 3)
        exp = pin.reference_pass(tris, pin.RENDER_MATERIALS, DEPTH, rec)
        nxt = rounds[k + 1] if k + 1 < len(rounds) else dict(rays=rec["rays"][:0], paths=rec["paths"][:0], samples=rec["samples"][:0])
        alive, nrays, npaths = _scatter(dict(count=len(nxt["rays"]), rays=nxt["rays"], paths=nxt["paths"], samples=nxt["samples"]), rec)
        pin.compare_with_reference("render round %d" % k, alive, nrays, npaths, rec, exp)
    assert np.array_equal(frame0.reshape(-1), total / ref.FIXED) and total.any()      # (the frame leaves the library as fixed point / 2^20: exact in float64)
    assert len(np.unique(frame0.reshape(-1, 3), axis=0)) > 1000                        # nothing like a constant sky
