"""Shared by tests/test_float_range.py (CPU) and tests/test_gpu_float_range.py: the small hand-made scenes, their rays, the scales 2^k at
which every length is multiplied, and the admission table (one ray per row with its outcome written out by hand).

Every scene is built ONCE at k = 0 (the builders never see extreme input); the scaled forms come from helpers.scale_blobs / scale_rays."""
import functools

import numpy as np

from oracle import oracle as orc
from rayaccel_amd import synth
from helpers import MISS, comb_scene, leaf_rays, leaf_scene, make_rays, scale_blobs, scale_geometry, scale_rays, scaled_results, tie_scene

SCALES = (0, 8, -8, 16, -16, 20, -20, 24, -24, 28, -28, 32, -32, 42, -42, 63, -63, 64, -64, 100, -100, 120, -120, -126, -140, -149)
IN_DOMAIN = tuple(range(-16, 17))      # what the fifth-order term T * |det| predicts for lengths of 1 .. 100
SCENES = ("quad", "leaf7 near_last", "leaf2 coincident", "tie", "comb16", "soup, reference builder", "soup, quality builder")
CLASSES = ("same", "wrong_triangle", "missed", "phantom", "nonfinite")


def quad_geometry():
    """_quad_scene of tests/test_gpu_edge_cases.py (and of tests/test_oracle.py): the unit quad in z = 0 and a lone far triangle."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 9], [6, 5, 9], [5, 6, 9]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.uint32)
    return dict(vertices=np.concatenate([v, np.ones((len(v), 1), np.float32)], 1), indices=idx)


def soup_geometry(quads=32, seed=0x51CE):
    """64 triangles: 32 slightly folded quads (two triangles sharing a diagonal, so the packer makes real pairs) of size 0.5 .. 3 with
    random orientation and heavy overlap in a box of +-4."""
    k = np.arange(quads)
    u = lambda s: synth.hash_uniform(k, s, seed).astype(np.float64)
    ctr = np.stack([u(1) * 8 - 4, u(2) * 8 - 4, u(3) * 8 - 4], 1)
    def unit(s0):
        z, ph = u(s0) * 2 - 1, u(s0 + 1) * 2 * np.pi
        r = np.sqrt(np.maximum(0.0, 1 - z * z))
        return np.stack([r * np.cos(ph), z, r * np.sin(ph)], 1)
    a, b = unit(4), unit(6)
    b -= a * (b * a).sum(1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    n = np.cross(a, b)
    size = (0.5 + 2.5 * u(8))[:, None]
    fold = (0.2 * (u(9) - 0.5))[:, None]
    corners = np.stack([ctr - a * size - b * size, ctr + a * size - b * size + n * fold, ctr + a * size + b * size, ctr - a * size + b * size + n * fold], 1)
    v = corners.reshape(-1, 3).astype(np.float32)
    idx = np.stack([np.stack([4 * k, 4 * k + 1, 4 * k + 2], 1), np.stack([4 * k, 4 * k + 2, 4 * k + 3], 1)], 1).reshape(-1, 3).astype(np.uint32)
    return dict(vertices=np.concatenate([v, np.ones((len(v), 1), np.float32)], 1), indices=idx)


def geometry_of_blobs(blobs):
    """The triangles a hand-made blob describes, for the arbiter: pair p holds (p0, p1, p2) under the id of remap[2p] and, unless p3 = p1
    (a lone triangle, Scene.cpp:174-178), (p0, p3, p1) under the id of remap[2p + 1].  The vertex ORDER is the pair's, not the original
    triangle's: good for the id and the distance, not for u and v.  Exact for the hand-made scenes (small integers and halves)."""
    n = int(blobs["pair_count"])
    p = blobs["pairs"][:n]
    p0 = p["p0"].astype(np.float64)
    p1, p2 = p0 - p["e1"], p0 + p["e2"]
    p3 = p0 + np.stack([p["e3x"], p["e3y"], p["e3z"]], 1)
    ids = blobs["remap"] & 0x3FFFFFFF
    count = int(ids[:2 * n].max()) + 1
    verts = np.zeros((3 * count, 4), np.float32)
    verts[:, 3] = 1
    for k in range(n):
        t0 = int(ids[2 * k])
        verts[3 * t0:3 * t0 + 3, :3] = (p0[k], p1[k], p2[k])
        if not np.array_equal(p3[k], p1[k]):
            t1 = int(ids[2 * k + 1])
            verts[3 * t1:3 * t1 + 3, :3] = (p0[k], p3[k], p1[k])
    return dict(vertices=verts, indices=np.arange(3 * count, dtype=np.uint32).reshape(-1, 3))


def _root_box(blobs):
    n = blobs["nodes"][0]
    return np.minimum(n["leftMin"], n["rightMin"]).astype(np.float64), np.maximum(n["leftMax"], n["rightMax"]).astype(np.float64)


def _edge_rays(blobs, limit=24, outer=True):
    """Rays onto the shared diagonal (p0-p1) of a pair, onto its outer edge p0-p2 and into the corner p0, along the pair's normal from both
    sides.  For an axis-aligned pair the normal is an axis and the target exact: the ray lies ON the edge, a tie inside the pair."""
    o, d = [], []
    n = int(blobs["pair_count"])
    for k in np.unique(np.linspace(0, n - 1, min(n, limit)).astype(int)):
        p = blobs["pairs"][k]
        p0, e1, e2 = p["p0"].astype(np.float64), p["e1"].astype(np.float64), p["e2"].astype(np.float64)
        nrm = np.cross(e1, e2)
        if not np.linalg.norm(nrm) > 0:
            continue
        nrm /= np.linalg.norm(nrm)
        for q in (p0 - 0.5 * e1, p0 - 0.25 * e1, p0 + 0.5 * e2, p0)[:4 if outer else 2]:
            o.append(q - 4.0 * nrm); d.append(nrm)
        o.append(p0 - 0.5 * e1 + 4.0 * nrm); d.append(-nrm)
    return make_rays(o, d)


def _box_rays(blobs, count, seed):
    """From points around the root box towards points inside it (seeded), every fifth one along an axis."""
    lo, hi = _root_box(blobs)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo) + 1e-3
    k = np.arange(count)
    u = lambda s: synth.hash_uniform(k, s, seed).astype(np.float64)
    target = ctr + np.stack([u(1) * 2 - 1, u(2) * 2 - 1, u(3) * 2 - 1], 1) * half
    z, ph = u(4) * 2 - 1, u(5) * 2 * np.pi
    r = np.sqrt(np.maximum(0.0, 1 - z * z))
    out = np.stack([r * np.cos(ph), r * np.sin(ph), z], 1)
    axis = (k % 5) == 0
    out[axis] = np.eye(3)[k[axis] % 3] * np.where(u(6)[axis] < 0.5, -1.0, 1.0)[:, None]
    origin = target + out * (2.5 * np.linalg.norm(half))
    return make_rays(origin, -out)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (blobs, geometry for the arbiter, rays) at k = 0.  A few hundred rays: the scene's own generator, rays onto the shared diagonals
    and edges and a seeded set around the root box.  minT = 0 and maxT = +inf, except every fourth ray: that one ends exactly at its hit
    (maxT = the oracle's t, minT = t / 2 on every eighth) or, where it misses, at 1000."""
    import rayaccel_amd as ra
    if name == "quad":
        geo = quad_geometry()
        blobs = orc.build_scene(geo["vertices"], geo["indices"])
        own = make_rays([[0.75, 0.25, -2], [0.25, 0.75, -2], [0.75, 0.25, 3], [0.5, 0.5, -1], [5.25, 5.25, 0], [5.9, 5.9, 0], [0.75, 0.25, -2], [0.3, 0.6, -2], [-3, -3, -2],
                         [1.0, 0.5, -2], [0.0, 0.0, -2], [1.0, 1.0, 5]],
                        [[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [-0.0, 0.0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]])
    elif name.startswith("leaf"):
        n, arrangement = int(name[4]), name.split()[1]
        blobs, geo = leaf_scene(n, arrangement)
        own = leaf_rays(n, arrangement)
    elif name == "tie":
        blobs, own = tie_scene()
        geo = geometry_of_blobs(blobs)
    elif name == "comb16":
        blobs = comb_scene(16)
        geo = geometry_of_blobs(blobs)
        own = make_rays(np.stack([np.linspace(-20, 20, 40), np.linspace(-15, 15, 40), np.full(40, -10.0)], 1), [[0, 0, 1]] * 40)
    else:
        geo = soup_geometry()
        if name == "soup, reference builder":
            blobs = orc.build_scene(geo["vertices"], geo["indices"])
        else:
            blobs = ra.HostScene(geo["vertices"], geo["indices"], quality=1).blobs()
        own = make_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    # (the soup's pairs are not axis-aligned: a ray "onto" an OUTER edge or a corner is a graze within rounding, on which the double-precision
    #  arbiter and binary32 may differ either way; its shared diagonals lie inside the quad, where only the triangle is in question)
    rays = np.concatenate([own, _edge_rays(blobs, outer=not name.startswith("soup")), _box_rays(blobs, 240, seed=len(name))])
    rays["minT"], rays["maxT"] = 0.0, np.inf
    hits = orc.traverse(blobs, rays)
    fourth = np.arange(len(rays)) % 4 == 3
    hit = hits["triangle"] != MISS
    rays["maxT"][fourth & hit] = hits["t"][fourth & hit]
    rays["maxT"][fourth & ~hit] = 1000.0
    eighth = fourth & hit & (np.arange(len(rays)) % 8 == 7)
    rays["minT"][eighth] = np.float32(0.5) * hits["t"][eighth]
    assert 200 <= len(rays) < 1000 and len(geo["indices"]) < 200
    return blobs, geo, rays


@functools.lru_cache(maxsize=None)
def case(name, k):
    """-> dict(blobs, geometry, rays: the scaled forms; ref: the oracle on them; want: the oracle at k = 0 with t scaled; in_domain: the two
    are bit-equal for every ray; nan_fields: the float fields of `ref`'s hit records that hold a NaN).  Cached: the tests leave it unchanged."""
    blobs0, geo0, rays0 = scene(name)
    blobs, rays = scale_blobs(blobs0, k), scale_rays(rays0, k)
    ref = orc.traverse(blobs, rays)
    want = scaled_results(orc.traverse(blobs0, rays0), k)
    hit = ref["triangle"] != MISS
    nan_fields = int(sum((hit & np.isnan(ref[f])).sum() for f in ("t", "u", "v")))
    for a in (ref, want, rays):
        a.flags.writeable = False
    return dict(blobs=blobs, geometry=scale_geometry(geo0, k), rays=rays, ref=ref, want=want, in_domain=ref.tobytes() == want.tobytes(), nan_fields=nan_fields)


def classify(ref, want, geometry, rays):
    """Every record of `ref` that differs from `want`, against the double-precision arbiter on the (scaled) scene -> counts per CLASSES:
    nonfinite (a hit record with a NaN or an infinity in t, u or v), missed (the arbiter hits, the record does not), phantom (the other way
    round), same (a hit at the arbiter's distance to 1e-4: its triangle or an exact tie), wrong_triangle (a hit at another distance: the
    other triangle of a pair, or a farther one)."""
    differ = np.nonzero((ref["triangle"] != want["triangle"]) | (ref["t"].view(np.uint32) != want["t"].view(np.uint32)) |
                        (ref["u"].view(np.uint32) != want["u"].view(np.uint32)) | (ref["v"].view(np.uint32) != want["v"].view(np.uint32)))[0]
    counts = dict.fromkeys(CLASSES, 0)
    if not len(differ):
        return counts
    with np.errstate(all="ignore"):
        tri, t, _, _, _ = orc.brute_closest(geometry["vertices"], geometry["indices"], rays[differ])
    for j, i in enumerate(differ):
        r = ref[i]
        hit, arb = r["triangle"] != MISS, tri[j] != MISS
        if hit and not (np.isfinite(r["t"]) and np.isfinite(r["u"]) and np.isfinite(r["v"])):
            counts["nonfinite"] += 1
        elif arb and not hit:
            counts["missed"] += 1
        elif hit and not arb:
            counts["phantom"] += 1
        elif hit and abs(float(r["t"]) - t[j]) <= 1e-4 * abs(t[j]):
            counts["same"] += 1
        elif hit:
            counts["wrong_triangle"] += 1
        else:
            counts["same"] += 1      # both miss: the records differ in the miss colour only (cannot happen: the direction is not scaled)
    return counts


# -------------------------------------------------------------------------------------------------------------------------------- worlds
def scale_transform(k):
    """2^k I as a [3,4] object-to-world transform, or None where 2^k is not a normal binary32 number."""
    m = np.zeros((3, 4), np.float32)
    with np.errstate(all="ignore"):
        s = np.ldexp(np.float32(1.0), k)
    if not np.isfinite(s) or s < np.finfo(np.float32).tiny:
        return None
    m[0, 0] = m[1, 1] = m[2, 2] = s
    return m


def world_expectation(transform, blobs, rays):
    """What a ONE-instance world must report: world_helpers' composed expectation — the oracle on the transformed ray — for
    every ray that enters the instance's padded world box by the top-level rule (world_helpers.top_level_enters), a miss for every other.
    -> None where the host preparation refuses the transform (with .code of the refusal in the second place), else
    dict(prep, want, want_inst, occluded, culled_hits: rays on which the composition alone hits but the top level never enters)."""
    import rayaccel_amd as ra
    from world_helpers import NO_INSTANCE, compose, top_level_enters
    try:
        prep = ra.host_world_prepare(np.array([transform], np.float32), np.array([ra.root_box(blobs["nodes"])]))
    except ra.RaccError as refusal:
        return None, refusal.code
    want, want_inst, hits = compose(prep["inv"], [blobs], rays, threads=1)
    enters = top_level_enters(prep, rays)
    culled = hits.any(0) & ~enters
    want[culled] = (MISS, 0.0, 0.0, 0.0)
    want_inst[culled] = NO_INSTANCE
    return dict(prep=prep, want=want, want_inst=want_inst, occluded=(hits.any(0) & enters).astype(np.uint8), culled_hits=np.nonzero(culled)[0]), 0


# ------------------------------------------------------------------------------------------------------------------------ admission table
F32 = np.float32
BIG, TINY, DENORMAL = np.finfo(np.float32).max, np.finfo(np.float32).tiny, F32(1e-41)
EPS = F32(1e-10)                    # Kernels.h:149-157: |d| < 1e-10 is replaced by +-1e-10
TRACED, REJECTED = "traced", "rejected"


def admission_table():
    """One ray per row on the quad scene -> (names, rays, expected): expected[i] is REJECTED (the record must be a miss with t = u = v = 0,
    whatever probe image is given) or (TRACED, triangle id or MISS) written out by hand — for a traced miss the record carries the probe
    colour.  The base ray starts at (0.75, 0.25, -2) along +z with (minT, maxT) = (0, 1000): it hits triangle 0 at t = 2."""
    names, rows, expected = [], [], []

    def row(name, outcome, origin=(0.75, 0.25, -2.0), direction=(0.0, 0.0, 1.0), min_t=0.0, max_t=1000.0):
        names.append(name)
        rows.append((origin, direction, min_t, max_t))
        expected.append(outcome)

    hit0 = (TRACED, 0)
    miss = (TRACED, MISS)
    specials = (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("largest finite", BIG), ("smallest normal", TINY), ("denormal", DENORMAL), ("+0", 0.0), ("-0", -0.0))
    # origin x (y) tiny or a zero of either sign: the origin lies on the quad's edge x = 0 (y = 0) within 1e-38.  The zero x and y
    # components of the direction are clamped to +1e-10, so at t = 2 the ray is 2e-10 INSIDE the quad in x and y: (2e-10, 0.25) lies in
    # triangle 1 = (v0, v2, v3), the half with x <= y, and (0.75, 2e-10) in triangle 0 = (v0, v1, v2), the half with y <= x.  The pair test
    # sees the tilt (R = d x C holds d.x = 1e-10 exactly), so the edge barycentric is a small positive number or +0 and its sign bit
    # accepts; reported, it rounds to u = 0 (x rows: P = v0 + u (v2 - v0) + v (v3 - v0), v = 0.25) resp. v = 0 (y rows: u = 0.75).
    # The double-precision arbiter, which does not clamp, sits exactly on the edge and reports the same triangle.
    edge_x, edge_y = (TRACED, 1, "moved"), (TRACED, 0, "moved")
    for axis in range(3):
        for label, value in specials:
            o = [0.75, 0.25, -2.0]
            o[axis] = value
            if label in ("NaN", "+inf", "-inf"):
                out = REJECTED
            elif label == "largest finite":
                out = miss                                       # x, y far off the quad; z beyond it, looking away
            elif axis == 2:
                out = miss                                       # z = 0 (or tiny): the origin lies IN the quad's plane: T <= |det| * minT = 0 rejects (open at minT)
            else:
                out = edge_x if axis == 0 else edge_y            # on the edge x = 0 / y = 0, 2e-10 inside: a hit (see above)
            row("origin[%d] = %s" % (axis, label), out, origin=tuple(o))
    for axis in range(3):
        for label, value in specials:
            d = [0.0, 0.0, 1.0]
            d[axis] = value
            if label in ("NaN", "+inf", "-inf"):
                out = REJECTED
            elif axis == 2:
                # dir.z tiny -> clamped to 1e-10: t = 2e10 > maxT = 1000: a miss; dir.z = 3.4e38: t = 2 / 3.4e38 (denormal), a hit while denormals are kept
                out = hit0 if label == "largest finite" else miss
            else:
                # dir.x / dir.y = 3.4e38 next to dir.z = 1: the ray leaves the quad sideways at once; tiny: the +z ray, a hit
                out = miss if label == "largest finite" else hit0
            row("dir[%d] = %s" % (axis, label), out, direction=tuple(d))
    for label, value in specials:
        if label in ("NaN", "+inf", "-inf"):
            out = REJECTED
        elif label == "largest finite":
            out = miss
        else:
            out = hit0
        row("minT = %s" % label, out, min_t=value)
    for label, value in specials:
        if label == "NaN":
            out = REJECTED
        elif label in ("+inf", "largest finite"):
            out = hit0                                           # maxT = +inf is a valid ray (no limit)
        else:
            out = miss                                           # -inf, tiny, +-0: the interval is empty before the quad
        row("maxT = %s" % label, out, max_t=value)
    # the clamp threshold: |d| < 1e-10 exactly.  Below it the component becomes +-1e-10, at and above it stays.  With dir.z = 1e-10 (either
    # way) t = 2e10: a hit only with maxT beyond it; what tells the rows apart is t itself (asserted in the test from the oracle: 2 / d).
    below, above = np.nextafter(EPS, F32(0)), np.nextafter(EPS, F32(1))
    for label, value in (("1e-10 - 1 ulp", below), ("1e-10", EPS), ("1e-10 + 1 ulp", above)):
        for sign in (1.0, -1.0):
            z = F32(sign) * value
            # (the zero x and y components are clamped to +1e-10 too: the ray runs along (1, 1, +-1) and meets z = 0 two units further in x and y)
            o = (0.75 - 2.0, 0.25 - 2.0, -2.0 if sign > 0 else 2.0)
            row("dir.z = %s%s, no limit" % ("+" if sign > 0 else "-", label), hit0, origin=o, direction=(0.0, 0.0, z), max_t=np.inf)
            row("dir.x = %s%s" % ("+" if sign > 0 else "-", label), hit0, direction=(F32(sign) * value, 0.0, 1.0))
    row("minT > maxT", miss, min_t=3.0, max_t=1.0)
    row("minT == maxT at the hit", miss, min_t=2.0, max_t=2.0)                          # open at minT
    row("maxT = 0", miss, max_t=0.0)
    row("negative minT, the hit behind the origin", hit0, origin=(0.75, 0.25, 2.0), min_t=-5.0, max_t=1000.0)      # t = -2 lies in (-5, 1000]
    row("negative minT and maxT, the hit behind the origin", hit0, origin=(0.75, 0.25, 2.0), min_t=-5.0, max_t=-1.0)
    row("negative minT, the hit behind minT", miss, origin=(0.75, 0.25, 2.0), min_t=-1.0, max_t=1000.0)
    for e in (30, -30, 100, -100, 126):
        # d = (0, 0, 2^e): t = 2 / 2^e, and x, y are clamped to 1e-10: the hit point moves by t * 1e-10 in x and y.  2^30, 2^100, 2^126: not at
        # all, a hit at t = 2^-29, 2^-99, 2^-125; 2^-30: t = 2^31 > 1000 (a miss), without a limit a hit 0.21 further in x and y (still
        # triangle 0, other u and v); 2^-100: t = 2^101, the hit point 2.5e20 off the quad: a miss either way
        s = float(np.ldexp(1.0, e))
        row("dir = (0, 0, 2^%d)" % e, hit0 if e > 0 else miss, direction=(0.0, 0.0, s))
        row("dir = (0, 0, 2^%d), no limit" % e, hit0 if e > 0 else ((TRACED, 0, "moved") if e == -30 else miss), direction=(0.0, 0.0, s), max_t=np.inf)
    row("dir = (0, 0, 2^127): 1/d denormal", hit0, direction=(0.0, 0.0, float(np.ldexp(1.0, 127))), max_t=np.inf)
    rays = np.zeros(len(rows), synth.RAY_DTYPE)
    with np.errstate(all="ignore"):
        for i, (o, d, lo, hi) in enumerate(rows):
            rays["origin"][i], rays["dir"][i], rays["minT"][i], rays["maxT"][i] = o, d, lo, hi
    return names, rays, expected


# ------------------------------------------------------------------------------------------------- known answers with non-finite planes
def nan_plane_case(infinite):
    """A node in which a NaN arrives as the SECOND operand of the oracle's omin / omax — what tells minNum from the select a < b ? a : b.
    One leaf with the quad (1e29, 0, 0) .. (3e29, 1, 0) and the ray from (2e29, 0.25, -2) along +z with maxT = 1000: the zero x component
    of the direction is clamped to 1e-10, 1 / d = 1e10 and -o / d = -2e39 overflows to -inf.
      finite planes:  a = fma(1e29, 1e10, -inf) = b = fma(3e29, 1e10, -inf) = -inf: the x slab ends at -inf, the box is missed, the record
                      a miss (out of the domain: the ray does pass through the quad, at t = 2);
      leftMax.x = +inf (`infinite`):  b = fma(+inf, 1e10, -inf) = NaN, the second operand of omin(a, b) and omax(a, b).
                      minNum / maxNum (OpenCL fmin / fmax, v_min_f32 / v_max_f32): both return a = -inf, the x slab ends at -inf: a MISS;
                      the select returns the NaN for both, it drops out of t0 and t1, y and z admit the ray: a HIT of triangle 0 at t = 2.
    -> (blobs, rays, expected triangle = MISS either way for minNum)."""
    from helpers import quad_pair
    L = 1e29
    blobs, _ = leaf_scene(1, "row")
    blobs["pairs"][0] = quad_pair([L, 0, 0], [3 * L, 0, 0], [3 * L, 1, 0], [L, 1, 0])
    blobs["pairs"][2:] = blobs["pairs"][0]
    n = blobs["nodes"][0]
    n["leftMin"], n["leftMax"] = (L, 0, 0), (np.inf if infinite else 3 * L, 1, 0)
    rays = make_rays([[2 * L, 0.25, -2.0]], [[0, 0, 1]], max_t=1000.0)
    return blobs, rays, MISS


def tie_pair_case():
    """A pair whose two triangles are the SAME triangle (p3 = p2: (a, c, b) under id 0 and (a, b, c) under id 1, opposite windings): both
    accept every ray through it with T1 |det2| == T2 |det1| bit for bit, and the pick `T1 * absDet2 > T2 * absDet1` (Kernels.h:97) keeps
    the FIRST — with >= it would be the second.  Rays from the front and from behind -> (blobs, rays, expected triangle ids)."""
    from helpers import quad_pair
    blobs, _ = leaf_scene(1, "row")
    blobs["pairs"][0] = quad_pair([0, 0, 10], [1, 0, 10], [1, 1, 10], [1, 0, 10])
    blobs["pairs"][2:] = blobs["pairs"][0]
    blobs["remap"][0], blobs["remap"][1] = 0, 1 | (1 << 30)
    rays = make_rays([[0.75, 0.25, 0.0], [0.75, 0.25, 20.0], [0.6, 0.5, 0.0]], [[0, 0, 1], [0, 0, -1], [0.01, -0.02, 1]])
    return blobs, rays, np.array([0, 0, 0], np.uint32)
