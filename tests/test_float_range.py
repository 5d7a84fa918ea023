"""The oracle across the whole float range (no GPU): where is DESIGN.md §3's "bit-identical for every finite ray" a statement about one
expression tree, and where does the tree itself leave the normal range?

Multiplying every length by 2^k is exact in binary floating point, so a traversal of the scaled scene must report the same triangle, the
same u and v and exactly 2^k t while nothing overflows, underflows or becomes inf - inf.  tests/float_range_cases.py holds the scenes
(all under 200 triangles, a few hundred rays each) and the scales.  For each scene:

  * the set D of k at which oracle(scale(scene), scale(rays)) == scale(oracle(scene, rays)) bit for bit is established from the oracle
    alone and must contain -16 .. 16 (measured over every k of -50 .. 45 and printed: -41 .. 35 is in D for every scene);
  * outside D every differing record is classified against the double-precision arbiter on the scaled scene (a measurement, printed;
    the table is in DESIGN.md §3);
  * whether a NaN reaches a hit record, the oracle's min / max or its pair test is stated as a test, counted by a build of the oracle with
    -DORC_COUNT_NAN that must give the same records;
  * the scalar oracle, its two SIMD ports and the wide model's calls into it are held to each other on every scene and k;
  * the top-level box test of the world kernels (world_helpers.top_level_enters) removes no composed hit inside D;
  * the admission table (one ray per row, outcome written by hand) is held to the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from rayaccel_amd import engine
import float_range_cases as frc
from float_range_cases import MISS, REJECTED, SCALES, SCENES, TRACED
from helpers import assert_bit_exact, assert_same_bits_nan_aware, scale_blobs, scale_rays, scaled_results

ORACLE_DIR = os.path.dirname(os.path.abspath(orc._LIB_PATH))      # the sources next to the library in use
# oracle/Makefile's CFLAGS: the counting build must be the same arithmetic
ORACLE_CFLAGS = ["-O3", "-fPIC", "-std=c11", "-D_GNU_SOURCE", "-ffp-contract=off", "-fno-math-errno", "-mavx2", "-mfma"]


@pytest.fixture(scope="module")
def counting_oracle(tmp_path_factory):
    """racc_oracle.c compiled with -DORC_COUNT_NAN -> traverse(blobs, rays) = (records, (NaN FIRST operands of omin / omax, NaN SECOND
    operands), pair tests that saw a NaN operand, per-ray flag: some pair test or min / max of this ray saw one)."""
    path = str(tmp_path_factory.mktemp("oracle") / "libracc_oracle_count.so")
    subprocess.check_call(["gcc"] + ORACLE_CFLAGS + ["-DORC_COUNT_NAN", "-shared", "-o", path, os.path.join(ORACLE_DIR, "racc_oracle.c"), "-lm", "-lpthread"])
    lib = C.CDLL(path)
    vp, u32 = C.c_void_p, C.c_uint32
    lib.orc_traverse.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, u32, vp, vp, vp]
    lib.orc_traverse.restype = None
    lib.orc_nan_counts.argtypes = [vp, C.c_int]
    lib.orc_nan_counts.restype = None

    def traverse(blobs, rays):
        rays = np.ascontiguousarray(rays)
        nodes, pairs, remap = (np.ascontiguousarray(blobs[f]) for f in ("nodes", "pairs", "remap"))
        out = np.zeros(len(rays), orc.RESULT_DTYPE)
        counts, total, tainted = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(len(rays), bool)
        lib.orc_nan_counts(orc._p(counts), 1)
        for i in range(len(rays)):      # one ray per call: the counters are global
            lib.orc_traverse(orc._p(nodes), orc._p(pairs), orc._p(remap), None, 0, 0, orc._p(rays), orc._p(out), i, i + 1, None, None, None)
            lib.orc_nan_counts(orc._p(counts), 1)
            total += counts
            tainted[i] = counts.any()
        return out, (int(total[0]), int(total[1])), int(total[2]), tainted
    return traverse


# ----------------------------------------------------------------------------------------------------------------------------- helpers
def test_scaling_helpers_are_exact_and_touch_only_lengths():
    blobs, geo, rays = frc.scene("leaf7 near_last")
    for k in (20, -20, 100, -100):
        sb, sr = scale_blobs(blobs, k), scale_rays(rays, k)
        back = scale_blobs(sb, -k)
        assert back["nodes"].tobytes() == blobs["nodes"].tobytes() and back["pairs"].tobytes() == blobs["pairs"].tobytes()      # exact both ways
        assert np.array_equal(sb["remap"], blobs["remap"]) and np.array_equal(sb["nodes"]["first"], blobs["nodes"]["first"]) and np.array_equal(sb["nodes"]["kind"], blobs["nodes"]["kind"])
        assert np.array_equal(sr["dir"], rays["dir"]) and np.array_equal(scale_rays(sr, -k)["origin"], rays["origin"])
        assert np.array_equal(sr["maxT"][np.isinf(rays["maxT"])], rays["maxT"][np.isinf(rays["maxT"])])
        assert np.array_equal(sb["pairs"]["p0"], blobs["pairs"]["p0"] * np.float32(2.0) ** k)
    res = orc.traverse(blobs, rays)
    s = scaled_results(res, 8)
    hit = res["triangle"] != MISS
    assert hit.any() and (~hit).any() and np.array_equal(s["t"][hit], res["t"][hit] * 256) and np.array_equal(s["t"][~hit], res["t"][~hit])
    assert np.array_equal(s["u"], res["u"]) and np.array_equal(s["triangle"], res["triangle"])


def test_nan_aware_comparison_excuses_only_the_oracles_nans():
    ref = np.zeros(4, orc.RESULT_DTYPE)
    ref["triangle"] = [3, 5, MISS, 7]
    ref["t"] = [1.0, np.nan, 0.25, 2.0]
    ref["u"] = [0.5, np.nan, 0.25, 0.5]
    got = ref.copy()
    got["t"].view(np.uint32)[1] ^= 0x80000000          # the other NaN sign
    assert assert_same_bits_nan_aware(got, ref) == 2
    with pytest.raises(AssertionError):
        assert_bit_exact(got, ref)                      # the plain comparison sees the sign of the NaN
    bad = got.copy(); bad["u"][1] = 0.5                 # a number where the oracle holds a NaN
    with pytest.raises(AssertionError):
        assert_same_bits_nan_aware(bad, ref)
    bad = got.copy(); bad["t"][0] = np.nan              # a NaN where the oracle holds a number
    with pytest.raises(AssertionError):
        assert_same_bits_nan_aware(bad, ref)
    bad = got.copy(); bad["t"][3] = np.nextafter(np.float32(2.0), np.float32(3.0))
    with pytest.raises(AssertionError):
        assert_same_bits_nan_aware(bad, ref)
    bad = got.copy(); bad["triangle"][0] = 4
    with pytest.raises(AssertionError):
        assert_same_bits_nan_aware(bad, ref)


# ------------------------------------------------------------------------------------------------------------------------- the domain D
@pytest.mark.parametrize("name", SCENES)
def test_domain_of_scale_invariance(name):
    """D from the reference alone; D must contain -16 .. 16 (every k of it, not only the listed scales).  Outside D: the class counts per k,
    printed (DESIGN.md §3 holds the table); nothing is asserted about them except that the oracle terminates."""
    blobs, geo, rays = frc.scene(name)
    assert (orc.traverse(blobs, rays)["triangle"] != MISS).sum() >= 10
    for k in frc.IN_DOMAIN:
        assert frc.case(name, k)["in_domain"], "%s: scaling by 2^%d changes the oracle's records" % (name, k)
    D = [k for k in sorted(SCALES) if frc.case(name, k)["in_domain"]]
    every = [k for k in range(-50, 46) if frc.case(name, k)["in_domain"]]
    assert every == list(range(every[0], every[-1] + 1)), "%s: D has a hole between 2^%d and 2^%d" % (name, every[0], every[-1])
    print("%s: D = %s of the listed scales; among every k of -50 .. 45: %d .. %d" % (name, D, every[0], every[-1]))
    for k in sorted(SCALES):
        c = frc.case(name, k)
        if not c["in_domain"]:
            print("%s k = %4d: %s, NaN fields in hit records %d" % (name, k, frc.classify(c["ref"], c["want"], c["geometry"], c["rays"]), c["nan_fields"]))
        assert c["in_domain"] == (c["nan_fields"] == 0 and c["ref"].tobytes() == c["want"].tobytes())
        if c["in_domain"]:
            assert c["nan_fields"] == 0


# ------------------------------------------------------------------------------------------------------------------- NaN reachability
def test_nan_reaches_hit_records_min_max_and_the_pair_test_only_outside_the_domain(counting_oracle):
    """Stated as found: from finite rays and finite scenes
      * inside D (every scene, every k of D) no NaN reaches omin / omax or the pair test, and no hit record holds a NaN or an infinity;
      * outside D, towards LARGE lengths, a hit record can carry an infinity (k >= 42) or a NaN (k >= 63) in t, u, v.  The NaN is born in
        the pair test (C = p0 - o and the products overflow: n . C = inf - inf, and t = T / |det| = inf * 0); an accepted NaN t becomes the
        ray's tFar, and THAT is how a NaN reaches omin / omax: as tFar, the first operand of the slab test's omin(t1, .), or as a child's
        "missed" value (= tFar) in omax(tFirst, tLast).  The slab products themselves never make one: fma(plane, 1 / d, -o / d) with finite
        factors returns an infinite addend unchanged;
      * as the first operand the select a < b ? a : b and minNum agree; as the second (tLast = NaN in omax(tFirst, tLast)) they differ, but
        the result is only compared `!= tRay` with tRay = the same NaN, true either way: no record can tell them apart on finite scenes
        (test_min_max_ignore_a_nan_plane does, with an infinite plane);
      * towards small lengths nothing becomes NaN: the products underflow to zero and the hits are lost (T <= |det| * tNear reads 0 <= 0).
    The counting build gives the same records as the library's."""
    reached = dict(first=0, second=0, pair=0, hit_nan=0, hit_inf=0)
    for name in SCENES:
        for k in SCALES:
            c = frc.case(name, k)
            res, (first, second), pair, tainted = counting_oracle(c["blobs"], c["rays"])
            assert res.tobytes() == c["ref"].tobytes(), "%s k = %d: the counting build computes other records" % (name, k)
            hit = c["ref"]["triangle"] != MISS
            inf = int(sum((hit & np.isinf(c["ref"][f])).sum() for f in ("t", "u", "v")))
            if c["in_domain"] or k < 0:
                assert (first, second, pair, c["nan_fields"], inf) == (0, 0, 0, 0, 0), "%s k = %d (%s): NaN at min/max %d + %d, in the pair test %d, in hit records %d, inf %d" % (
                    name, k, "in D" if c["in_domain"] else "small lengths", first, second, pair, c["nan_fields"], inf)
            if first or second:
                assert pair > 0, "%s k = %d: a NaN at omin / omax although no pair test saw one" % (name, k)
            reached["first"] += first; reached["second"] += second; reached["pair"] += pair; reached["hit_nan"] += c["nan_fields"]; reached["hit_inf"] += inf
    print("NaN at omin / omax as first operand: %(first)d, as second: %(second)d, pair tests with a NaN operand: %(pair)d, NaN fields in hit records: %(hit_nan)d, infinite fields: %(hit_inf)d" % reached)
    assert reached["first"] > 0 and reached["pair"] > 0 and reached["hit_nan"] > 0 and reached["hit_inf"] > 0


def test_min_max_ignore_a_nan_plane(counting_oracle):
    """omin / omax are minNum / maxNum (as OpenCL's fmin / fmax and v_min_f32 / v_max_f32): float_range_cases.nan_plane_case works out by
    hand that the ray misses, with finite planes and with the infinite one that puts a NaN into the SECOND operand — where the select
    a < b ? a : b enters the box and reports triangle 0 at t = 2 (tools/oracle_fault_injection.py: this test fails for that fault).  Both
    SIMD ports alike."""
    for infinite in (False, True):
        blobs, rays, want = frc.nan_plane_case(infinite)
        got = orc.traverse(blobs, rays)
        assert got["triangle"][0] == want and got["t"][0] == 0 and got["u"][0] == 0 and got["v"][0] == 0, "infinite plane: %s, record %s" % (infinite, got[0])
        res, (first, second), pair, _ = counting_oracle(blobs, rays)
        assert res.tobytes() == got.tobytes() and first == 0 and (second > 0) == infinite and pair == 0
        for width in (8, 16):
            if orc.simd_width() >= width:
                assert orc.traverse_simd(blobs, rays, width=width).tobytes() == got.tobytes()


def test_the_pick_keeps_the_first_triangle_on_an_exact_tie():
    """Both triangles of float_range_cases.tie_pair_case accept every ray at equal T |det|: the strict pick (Kernels.h:97) reports the first."""
    blobs, rays, want = frc.tie_pair_case()
    got = orc.traverse(blobs, rays)
    assert np.array_equal(got["triangle"], want) and got["t"][0] == 10.0 and got["t"][1] == 10.0, got
    for width in (8, 16):
        if orc.simd_width() >= width:
            assert orc.traverse_simd(blobs, rays, width=width).tobytes() == got.tobytes()
    for fmt in (45, 50):
        records, _ = engine.wide_nodes(blobs["nodes"], len(blobs["pairs"]), len(blobs["remap"]), fmt)
        assert orc.traverse_wide(records, fmt, blobs, rays)[0].tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------------------------- the ports
@pytest.mark.parametrize("name", SCENES)
def test_oracle_ports_agree_on_every_scale(name, counting_oracle):
    """The scalar oracle, the AVX2 and AVX-512 ports and the threaded entry are byte-identical on every scene and k, for every ray — denormal
    operands (k <= -120), overflowing ones and NaN included.  (Found by this test: with the negations of mad_cross written as -(x) gcc folds
    them into fused multiply-subtracts, which leave the sign of a NaN product alone where the ports' and the GPU's explicit flip changes it;
    the pair test reads sign bits, so eight rays of the comb at 2^120 were a miss in the scalar oracle and a hit in both ports and in every
    kernel.  The oracle now flips the bit, racc_oracle.c oneg.)"""
    excused = 0
    for k in SCALES:
        c = frc.case(name, k)
        _, _, _, tainted = counting_oracle(c["blobs"], c["rays"])
        assert not (tainted.any() and c["in_domain"])
        tainted |= np.isnan(c["ref"]["t"]) | np.isnan(c["ref"]["u"]) | np.isnan(c["ref"]["v"])      # (inf * 0 in t = T / |det| comes after every test)
        assert orc.traverse(c["blobs"], c["rays"], threads=3).tobytes() == c["ref"].tobytes()
        for width in (8, 16):
            if orc.simd_width() < width:
                continue
            got = orc.traverse_simd(c["blobs"], c["rays"], width=width)
            assert got.tobytes() == c["ref"].tobytes(), "%s k = %d: the %d-lane port differs from the scalar oracle at rays %s (%d of them saw a NaN)" % (
                name, k, width, np.nonzero((got.view(np.uint32).reshape(-1, 4) != c["ref"].view(np.uint32).reshape(-1, 4)).any(1))[0][:8], int(tainted.sum()))
            excused += int(tainted.sum())
        for fmt in (45, 50):
            records, _ = engine.wide_nodes(c["blobs"]["nodes"], len(c["blobs"]["pairs"]), len(c["blobs"]["remap"]), fmt)
            a = orc.traverse_wide(records, fmt, c["blobs"], c["rays"], threads=1)[0]
            b = orc.traverse_wide(records, fmt, c["blobs"], c["rays"], threads=4, compare=False)[0]
            assert a.tobytes() == b.tobytes()
            if c["in_domain"] and fmt == 45:
                # the wide model calls the oracle's own pair test and admission: inside D its records are the oracle's but for exact ties
                same = (a["triangle"] == c["ref"]["triangle"])
                assert a[same].tobytes() == c["ref"][same].tobytes()
                assert np.array_equal(a["t"][~same], c["ref"]["t"][~same])
    print("%s: %d ray traversals that saw a NaN compared byte for byte" % (name, excused))


# ------------------------------------------------------------------------------------------------------------- worlds: the top level
def test_top_level_cull_changes_no_record_inside_the_domain():
    """A world tests the ray against the instance's padded world box before it enters the instance — a test the single-scene path does not
    make.  Inside D it removes no hit (world_build.cpp's bound), both for an identity instance of the scaled scene and for the unscaled
    scene under 2^k I; outside D the oracle accepts pairs through infinite and NaN operands on rays that never enter that box (or whose
    entry distance is +inf under maxT = +inf, the slab test's "missed"), and the world reports a miss there: counted and printed."""
    culled_outside = 0
    for name in SCENES:
        blobs0, _, _ = frc.scene(name)
        for k in SCALES:
            c = frc.case(name, k)
            ways = [("identity instance of the scaled scene", np.eye(3, 4, dtype=np.float32), c["blobs"])]
            if frc.scale_transform(k) is not None:
                ways.append(("the unscaled scene under 2^k I", frc.scale_transform(k), blobs0))
            for way, m, blobs in ways:
                exp, code = frc.world_expectation(m, blobs, c["rays"])
                if exp is None:
                    assert not c["in_domain"], "%s, 2^%d, %s: the host preparation refuses (%d) a transform inside D" % (name, k, way, code)
                    continue
                if c["in_domain"]:
                    assert len(exp["culled_hits"]) == 0, "%s, 2^%d, %s: the top level culls rays %s that hit" % (name, k, way, exp["culled_hits"][:8])
                elif len(exp["culled_hits"]):
                    culled_outside += len(exp["culled_hits"])
                    print("%s, 2^%d, %s: %d composed hits never enter the world box, rays %s" % (name, k, way, len(exp["culled_hits"]), exp["culled_hits"][:8]))
    assert culled_outside > 0


# ---------------------------------------------------------------------------------------------------------------- the admission table
def test_admission_table_on_the_oracle():
    """One ray per row on the quad scene, the outcome written by hand (float_range_cases.admission_table): REJECTED rows are misses with
    t = u = v = 0 whatever the probe image; traced rows report the triangle given there, and every traced hit is the double-precision
    arbiter's triangle too on the rows that vary the origin (the arbiter does not clamp directions)."""
    names, rays, expected = frc.admission_table()
    geo = frc.quad_geometry()
    blobs = orc.build_scene(geo["vertices"], geo["indices"])
    env = np.full((4, 8, 4), 0.5, np.float32)
    res = orc.traverse(blobs, rays, env=env)
    tri, t, _, _, _ = orc.brute_closest(geo["vertices"], geo["indices"], rays)
    assert len(names) == len(set(names)) and len(names) > 90
    for i, (name, want) in enumerate(zip(names, expected)):
        r = res[i]
        if want == REJECTED:
            assert r["triangle"] == MISS and r["t"] == 0 and r["u"] == 0 and r["v"] == 0, "%s: %s" % (name, r)
        else:
            assert want[0] == TRACED and r["triangle"] == want[1], "%s: triangle %d, expected %d" % (name, r["triangle"], want[1])
            if name.startswith("origin[") and want[1] != MISS:      # (not the rows that live on the clamp: the arbiter does not clamp)
                assert tri[i] == want[1], "%s: the arbiter reports triangle %d" % (name, tri[i])
            if want[1] == MISS:
                assert r["t"] == 0.5 and r["u"] == 0.5 and r["v"] == 0.5, "%s: a traced miss carries the probe colour, got %s" % (name, r)
            else:
                assert np.isfinite(r["t"]) and (len(want) == 3 or (abs(r["u"] - 0.5) < 1e-6 and abs(r["v"] - 0.25) < 1e-6)), "%s: %s" % (name, r)
    # the clamp: below 1e-10 the component is replaced, at and above it is kept — t = 2 / |d.z| tells them apart
    for sign in "+-":
        below, at, above = (res["t"][names.index("dir.z = %s%s, no limit" % (sign, label))] for label in ("1e-10 - 1 ulp", "1e-10", "1e-10 + 1 ulp"))
        assert below == at and above < at and np.nextafter(above, np.float32(np.inf)) >= np.nextafter(at, np.float32(0)) and abs(at - 2e10) < 1e4, (below, at, above)
    i = names.index("dir = (0, 0, 2^127): 1/d denormal")
    assert res["t"][i] == np.float32(2.0 ** -126)      # 2 * 2^-127: 1/d is a denormal, kept
    i = names.index("dir[2] = largest finite")
    assert 0 < res["t"][i] < np.finfo(np.float32).tiny   # t itself is a denormal
    # every port admits alike
    for width in (8, 16):
        if orc.simd_width() >= width:
            assert orc.traverse_simd(blobs, rays, env=env, width=width).tobytes() == res.tobytes()
    for fmt in (45, 50):
        records, _ = engine.wide_nodes(blobs["nodes"], len(blobs["pairs"]), len(blobs["remap"]), fmt)
        wide = orc.traverse_wide(records, fmt, blobs, rays, env=env)[0]
        assert np.array_equal(wide["triangle"], res["triangle"]) and wide["t"].tobytes() == res["t"].tobytes()
