"""CPU tests (no GPU): the host consumer's per-record arithmetic (rayaccel_amd/csrc/pt_shade.h through the hooks
racc_pt_test_primary_rays / racc_pt_test_shade of pathtracer.cpp) against oracle/pt_reference.py, a float64 restatement of the
reference's lines — record by record, on the inputs of tests/pt_inputs.py.  tests/test_gpu_pt_kernels.py holds the two device
kernels to the same reference and, bit for bit, to these hooks."""
import numpy as np
import pytest

import pt_inputs as pin
from oracle import pt_reference as ref
from rayaccel_amd import engine
from rayaccel_amd.engine import PATH_DTYPE, RAY_DTYPE, RESULT_DTYPE

CAM = np.array([1.5, 20.0, -60.0, 0.0011, 0.0, 0.0002, 0.0, -0.0011, 0.0001, -0.9, 0.55, 0.8], np.float32)      # origin, right, up, view


@pytest.fixture(scope="module")
def table(small_scene):
    return pin.tri_table(small_scene)


def _one(tri_row, material, d, t, u, v, weight=(1, 1, 1), pixel=77, depth=0, sample=3, origin=(0.25, 0.25, 1.0)):
    """One record on a one-triangle table."""
    rays, hits, paths = np.zeros(1, RAY_DTYPE), np.zeros(1, RESULT_DTYPE), np.zeros(1, PATH_DTYPE)
    rays["origin"], rays["dir"], rays["minT"], rays["maxT"] = origin, d, 1e-3, 1e6
    hits["triangle"], hits["t"], hits["u"], hits["v"] = 0, t, u, v
    paths["weight"], paths["pixelDepth"] = weight, pixel | (depth << 24)
    tris = tri_row.copy()
    tris["material"] = material
    return dict(rays=rays, hits=hits, paths=paths, samples=np.array([sample], np.uint32), cls=np.array(["hand"], dtype=object)), tris


def _both(rec, tris, materials=pin.MATERIALS, max_depth=pin.MAX_DEPTH):
    host = engine.pt_host_shade(tris, materials, max_depth, rec["rays"], rec["hits"], rec["paths"], rec["samples"])
    return host, pin.reference_pass(tris, materials, max_depth, rec)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
MIRROR = dict(kd=np.zeros((4, 3), np.float32), eta=np.full(4, 1.5, np.float32))      # kd = 0: only the mirror lobe can be picked


def test_barycentrics_weigh_the_three_corners_in_the_order_w_u_v():
    """The unit right triangle with three different vertex normals, hit at its corners: (u, v) = (1, 0) must shade with n1,
    (0, 1) with n2, (0, 0) with n0 (PathTracingRenderer.cpp:261-274).  With kd = 0 the bounce is the mirror direction
    2 (n.wo) n - wo of THAT normal, known in closed form."""
    hand, names = pin.hand_made_tris()
    row = hand[names["right"]:names["right"] + 1]
    d = np.array([0.0, 0.0, -1.0], np.float32)
    wo = -d.astype(np.float64)
    for (u, v), corner in (((1, 0), "n1"), ((0, 1), "n2"), ((0, 0), "n0")):
        rec, tris = _one(row, 1, d, 1.0, u, v)
        host, exp = _both(rec, tris, MIRROR)
        n = row[corner][0].astype(np.float64)
        mirror = 2 * (n @ wo) * n - wo
        assert host["alive"][0] and exp["alive"][0]
        np.testing.assert_allclose(host["rays"]["dir"][0], mirror, rtol=0, atol=pin.TOL_DIR)
        np.testing.assert_allclose(exp["dir"][0], mirror, rtol=0, atol=pin.TOL_DIR)
        others = [row[c][0].astype(np.float64) for c in ("n0", "n1", "n2") if c != corner]
        assert all(np.abs(2 * (m @ wo) * m - wo - mirror).max() > 0.1 for m in others)          # the three answers are far apart


def test_a_ray_from_the_back_flips_both_normals_and_stays_on_its_side():
    """A ray arriving from below the triangle (z < 0): geometric and shading normal both turn to -z, the next origin is moved to
    the ray's side (hit point - 1e-4 z) and the mirror bounce leaves downward."""
    hand, names = pin.hand_made_tris()
    row = hand[names["right"]:names["right"] + 1]
    d = pin._unit(np.array([0.1, 0.2, 1.0])).astype(np.float32)
    origin = (np.array([0.25, 0.25, 0.0]) - 2.0 * d.astype(np.float64)).astype(np.float32)
    rec, tris = _one(row, 1, d, 2.0, 0.25, 0.25, origin=origin)
    host, exp = _both(rec, tris, MIRROR)
    assert host["alive"][0] and exp["alive"][0]
    hit_point = origin.astype(np.float64) + 2.0 * d.astype(np.float64)
    for o in (host["rays"]["origin"][0].astype(np.float64), exp["origin"][0]):
        np.testing.assert_allclose(o - hit_point, [0, 0, -1e-4], rtol=0, atol=2e-6)
        assert o[2] < hit_point[2]
    n = row["n0"][0] * 0.5 + row["n1"][0] * 0.25 + row["n2"][0] * 0.25
    n = -pin._unit(n.astype(np.float64))
    wo = -d.astype(np.float64)
    mirror = 2 * (n @ wo) * n - wo
    assert mirror[2] < -0.5
    np.testing.assert_allclose(host["rays"]["dir"][0], mirror, rtol=0, atol=pin.TOL_DIR)
    np.testing.assert_allclose(exp["dir"][0], mirror, rtol=0, atol=pin.TOL_DIR)
    pin.compare_with_reference("back side", host["alive"], host["rays"], host["paths"], rec, exp)


def test_the_depth_guard_lets_the_last_bounce_through_and_no_more():
    """depth == maxDepth - 1 continues with depth bits maxDepth (PathTracingRenderer.cpp:120, :414); depth == maxDepth ends."""
    hand, names = pin.hand_made_tris()
    row = hand[names["right"]:names["right"] + 1]
    d = np.array([0.0, 0.0, -1.0], np.float32)
    rec, tris = _one(row, 1, d, 1.0, 0.3, 0.3, pixel=0xFFFFFF, depth=pin.MAX_DEPTH - 1)
    host, exp = _both(rec, tris, MIRROR)
    assert host["alive"][0] and exp["alive"][0]
    assert host["paths"]["pixelDepth"][0] == exp["pixelDepth"][0] == (0xFFFFFF | (pin.MAX_DEPTH << 24))
    rec, tris = _one(row, 1, d, 1.0, 0.3, 0.3, pixel=0xFFFFFF, depth=pin.MAX_DEPTH)
    host, exp = _both(rec, tris, MIRROR)
    assert not host["alive"][0] and not exp["alive"][0]


def test_the_camera_ray_through_pixel_zero_in_closed_form():
    """Pixel (0, 0) with both jitters known (the counter RNG's two numbers, checked to be what racc_pt_test_uniform returns):
    dir = normalize(view + right jx + up jy), origin the camera's, [minT, maxT] = [0, 1e6], weight 1, depth 0."""
    import ctypes as C
    lib = C.CDLL(engine.PT_LIB_PATH)
    sample = 5
    j = np.zeros(2, np.float32)
    for k, stream in enumerate((1, 2)):
        out = np.zeros(1, np.float32)
        lib.racc_pt_test_uniform(C.c_uint32(0), C.c_uint32(sample), C.c_uint32(0), C.c_uint32(stream), C.c_uint32(1), out.ctypes.data_as(C.c_void_p))
        j[k] = out[0]
    key = ref.path_key(np.array([0]), np.array([sample]))
    assert ref.uniform_keyed(key, 0, 1)[0] == float(j[0]) and ref.uniform_keyed(key, 0, 2)[0] == float(j[1])
    assert 0 <= j[0] < 1 and 0 <= j[1] < 1 and j[0] != j[1]
    c = CAM.astype(np.float64).reshape(4, 3)
    want = pin._unit(c[3] + c[1] * float(j[0]) + c[2] * float(j[1]))
    z = np.zeros(1, np.uint32)
    rays, paths = engine.pt_host_primary_rays(CAM, z, z, z, z + sample)
    exp = ref.primary_ray(CAM, z, z, z, z + sample)
    np.testing.assert_allclose(rays["dir"][0], want, rtol=0, atol=pin.TOL_DIR)
    np.testing.assert_allclose(exp["dir"][0], want, rtol=0, atol=1e-15)
    assert np.array_equal(rays["origin"][0], CAM[:3]) and rays["minT"][0] == 0 and rays["maxT"][0] == np.float32(1e6)
    assert np.array_equal(paths["weight"][0], [1, 1, 1]) and paths["pixelDepth"][0] == 0


# ---- the generated classes -------------------------------------------------------------------------------------------------------
def test_host_camera_rays_match_the_reference():
    rng = np.random.default_rng(pin.SEED)
    n = 20000
    x, y = rng.integers(0, 1920, n).astype(np.uint32), rng.integers(0, 1080, n).astype(np.uint32)
    pixel, sample = y * np.uint32(1920) + x, rng.integers(0, 64, n).astype(np.uint32)
    rays, paths = engine.pt_host_primary_rays(CAM, x, y, pixel, sample)
    exp = ref.primary_ray(CAM, x, y, pixel, sample)
    dev = np.abs(rays["dir"].astype(np.float64) - exp["dir"]).max()
    print("camera rays: largest direction deviation %.3g (bound %.3g)" % (dev, pin.TOL_DIR))
    assert dev <= pin.TOL_DIR
    for f in ("origin", "minT", "maxT"):
        assert np.array_equal(rays[f].view(np.uint32), exp[f].view(np.uint32)), f
    assert np.array_equal(paths["weight"], exp["weight"]) and np.array_equal(paths["pixelDepth"], exp["pixelDepth"])
    # neighbouring pixels get different jitter, and the ray moves with the pixel
    assert len(np.unique(rays["dir"], axis=0)) == n


@pytest.mark.parametrize("count", [1, 64, 1025, 3 * 1024 + 5, 40000])
def test_host_shading_matches_the_reference_record_by_record(table, count):
    tris, names = table
    rec = pin.make_records(count, tris, names)
    host = engine.pt_host_shade(tris, pin.MATERIALS, pin.MAX_DEPTH, rec["rays"], rec["hits"], rec["paths"], rec["samples"])
    exp = pin.reference_pass(tris, pin.MATERIALS, pin.MAX_DEPTH, rec)
    pin.compare_with_reference("host hook, %d records" % count, host["alive"], host["rays"], host["paths"], rec, exp)
    # misses: exact
    assert np.array_equal(host["valid"], exp["valid"]) and np.array_equal(host["contrib"], exp["contrib"])
    assert not host["alive"][exp["miss"]].any()


def test_every_class_is_exercised_and_stays_under_the_borderline_cap(table):
    """Per input class: how many records, how many survive, the share inside a decision guard (<= 1 % of the class's surface
    hits) — and the outcomes each class exists for."""
    tris, names = table
    rec = pin.make_records(40000, tris, names)
    host, exp = _both(rec, tris)
    cls = rec["cls"]
    assert set(cls) == set(pin.CLASSES)
    for c in pin.CLASSES:
        k = cls == c
        surf = k & exp["surface"]
        share = (exp["borderline"] & surf).sum() / max(int(surf.sum()), 1)
        print("class %-15s %6d records, %6d surface hits, %6d alive, borderline share %.4f%%" % (c, k.sum(), surf.sum(), (exp["alive"] & k).sum(), 100 * share))
        assert share <= pin.BORDERLINE_CAP, c
    alive = host["alive"]
    for c in ("surface", "edge", "grazing", "nx", "cut", "one_channel", "depth"):
        assert 0 < alive[cls == c].sum() < (cls == c).sum(), c                     # both outcomes occur
    for c in ("guard", "zero_area", "cancelling", "far"):
        assert not alive[cls == c].any() and not exp["alive"][cls == c].any(), c     # these end the path, without a trap
    m = rec["hits"]["triangle"] != ref.MISS
    mat = tris["material"][np.where(rec["hits"]["triangle"] < len(tris), rec["hits"]["triangle"], 0)]
    assert not alive[m & (mat == 2)].any()                                          # kd = 0, eta = 1: the zero denominator
    assert all(alive[m & (mat == i)].any() for i in (0, 1, 3))
    k_neg = exp["margins"]["k"][exp["surface"] & (mat == 1)]
    assert (k_neg < np.inf).any()
    # both tangent frames, both lobes, both sides
    nx = cls == "nx"
    assert alive[nx].any()
    d = cls == "depth"
    depth = rec["paths"]["pixelDepth"] >> 24
    assert alive[d & (depth == pin.MAX_DEPTH - 1)].any() and not alive[d & (depth == pin.MAX_DEPTH)].any()
    assert ((host["paths"]["pixelDepth"][d & alive] & 0xFFFFFF) == 0xFFFFFF).all()
    # misses: zero channels, skipped channels, negative and large contributions, denormals read as zero
    assert (host["contrib"][cls == "miss_negative"] < 0).any() and (np.abs(host["contrib"][cls == "miss_big"]) > 2 ** 38).any()
    assert (~host["valid"][cls == "miss_nonfinite"]).sum() == (cls == "miss_nonfinite").sum()
    assert (host["contrib"][cls == "miss_zero"] == 0).any()
    z = host["contrib"][cls == "miss_denormal"]
    assert ((z == 0).sum(1) == 1).all() and (z > 2 ** 20).any()


def test_miss_contributions_round_half_away_from_zero():
    """Products that land exactly on .5 fixed-point units, both signs: llround, not rint."""
    n = 8
    hits, paths = np.zeros(n, RESULT_DTYPE), np.zeros(n, PATH_DTYPE)
    hits["triangle"] = ref.MISS
    half = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5]) / ref.FIXED          # exact in float32
    hits["t"], hits["u"], hits["v"] = half, -half, half * 3
    paths["weight"], paths["pixelDepth"] = 1.0, np.arange(n)
    tris, _ = pin.hand_made_tris()
    host = engine.pt_host_shade(tris, pin.MATERIALS, pin.MAX_DEPTH, np.zeros(n, RAY_DTYPE), hits, paths, np.zeros(n, np.uint32))
    add, valid = ref.miss_contribution(hits, paths)
    assert valid.all() and np.array_equal(add[:, 0], [1, 2, 3, 4, -1, -2, -3, -4]) and np.array_equal(add[:, 1], -add[:, 0])
    assert np.array_equal(host["contrib"], add) and host["valid"].all()
    frame = ref.accumulate_misses(hits, paths, 3 * n)
    assert np.array_equal(frame.reshape(n, 3), add)
