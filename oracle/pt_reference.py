"""Float64 restatement of the path-tracing consumer's three per-record operations: one camera ray, one surface
interaction, one miss.  numpy only, no GPU, vectorised over records.

TEST INFRASTRUCTURE ONLY (like oracle.py): imported by tests/, never by anything under rayaccel_amd/.

Written from the reference's source lines (file:line into the reference checkout), NOT from rayaccel_amd/csrc/pt_shade.h:
    camera ray            Renderer/Camera.cpp:55-85, payload Renderer/LightPath.cpp:11-37, Renderer/LightPath.h:14-17
    surface interaction   Renderer/PathTracingRenderer.cpp:113-422 (material: oracle.pt_sample_material, Materials.cpp:39-151)
    miss                  Renderer/PathTracingRenderer.cpp:505-563
Inputs are the float32 / uint32 values exactly as the kernels get them; arithmetic is float64.

Where the project departs from the reference ON PURPOSE this module takes the project's side:
  1. random numbers come from a counter RNG keyed by (pixel, sample, depth, stream) instead of rand()-seeded SimdRandom8
     streams (Camera.cpp:58, PathTracingRenderer.cpp:102): integer arithmetic, restated exactly below (uint32);
  2. exact sine and cosine instead of the parabolas of Materials.cpp:11-29 (pt_sample_material(..., exact_trig=True));
  3. true division and square root where the reference uses rcp / rsqrt (Camera.cpp:79, PathTracingRenderer.cpp:282);
  4. the shading normal is turned to the viewer's side by the sign of ITS OWN dot product with wo; the reference gives it the
     sign bit of dot(rayDir, geometryNormal) (:342-349), which is the same thing only under the orientation convention of the
     per-triangle normals stored in ITS scene files — the project recomputes those normals from the winding (the file's are
     skipped) and cannot rely on that convention.  `sides_disagree` in shade_surface's result marks the records where the two
     normals lie on different sides of the ray, i.e. where the two rules could differ;
  5. a next origin or direction that is infinite ends the path, not only one that is NaN (:416-419 compares x == x);
  6. the frame buffer is 64-bit fixed point (2^20 units) instead of float (:535-547, :562), and a non-finite product is
     skipped per channel: miss_contribution is therefore exact integer arithmetic.
"""
import ctypes as C

import numpy as np

from . import oracle as orc

RAY_DTYPE = orc.RAY_DTYPE
HIT_DTYPE = orc.RESULT_DTYPE
PATH_DTYPE = np.dtype([("weight", "<f4", 3), ("pixelDepth", "<u4")])                       # LightPath.h:14-17
# the device consumer's 64-byte per-triangle shading record: three vertex normals, the geometric normal, the material
SHADE_TRI_DTYPE = np.dtype([("n0", "<f4", 3), ("n1", "<f4", 3), ("n2", "<f4", 3), ("ng", "<f4", 3), ("material", "<u4"), ("pad", "<u4", 3)])
assert PATH_DTYPE.itemsize == 16 and SHADE_TRI_DTYPE.itemsize == 64

MISS = 0xFFFFFFFF
FIXED = 1048576.0                                   # 2^20
F32 = np.float32
MIN_T, MAX_T = F32(1e-3), F32(1e6)                  # PathTracingRenderer.cpp:421-422 (float literals)
OFFSET = float(F32(1e-4))                           # :410-412
CUT = float(F32(0.01))                              # :394-396
WIDE = float(F32(0.1))                              # Materials.cpp:83

# Decision guards: a record whose margin for a decision is inside its guard may legitimately take the other branch in
# float32.  `rel` guards are relative to the threshold, the others absolute.
GUARDS = dict(ng_wo=3e-6, n_wo=3e-6, n_x=2.0 ** -23, k=1e-6, pick=2e-4, cut=2e-4, wi_ng=3e-6)


# ---- the counter RNG (departure 1): uint32 arithmetic, exact ------------------------------------------------------------------
def _u32(a):
    return np.asarray(a).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def pcg(x):
    x = _u32(_u32(x) * np.uint64(747796405) + np.uint64(2891336453))
    w = _u32(((x >> ((x >> np.uint64(28)) + np.uint64(4))) ^ x) * np.uint64(277803737))
    return (w >> np.uint64(22)) ^ w


def path_key(pixel, sample):
    return pcg(pcg(pixel) ^ _u32(_u32(sample) * np.uint64(0x9E3779B9)))


def uniform_keyed(key, depth, stream):
    """24-bit uniform in [0, 1): exact in float32 and float64."""
    h = pcg(key ^ _u32(_u32(depth) * np.uint64(0x85EBCA6B) + np.uint64((stream * 0xC2B2AE35) & 0xFFFFFFFF)))
    return (h >> np.uint64(8)).astype(np.float64) / 16777216.0


# ---- camera ray ---------------------------------------------------------------------------------------------------------------
def primary_ray(cam, x, y, pixel, sample):
    """Camera.cpp:55-85 for one pixel each.  cam: 12 float32 = origin, right, up, view (Camera::lookAt's products, :22-25).
    -> dict(origin[n,3] f32, dir[n,3] f64, minT, maxT f32, weight[n,3] f32, pixelDepth u32)."""
    cam = np.asarray(cam, np.float32).reshape(4, 3).astype(np.float64)
    origin, right, up, view = cam
    x, y, pixel, sample = (np.asarray(a, np.uint32) for a in (x, y, pixel, sample))
    key = path_key(pixel, sample)
    px = x.astype(np.float64) + uniform_keyed(key, 0, 1)                  # :68 (the x jitter is drawn first)
    py = y.astype(np.float64) + uniform_keyed(key, 0, 2)                  # :69
    d = view[None, :] + up[None, :] * py[:, None] + right[None, :] * px[:, None]          # :71-77
    d = d / np.sqrt((d * d).sum(1))[:, None]                                                # :79-83 (true 1/sqrt: departure 3)
    n = len(x)
    return dict(origin=np.broadcast_to(cam[0].astype(np.float32), (n, 3)).copy(), dir=d,
                minT=np.zeros(n, np.float32),                                               # :56
                maxT=np.full(n, MAX_T, np.float32),                                         # :85
                weight=np.ones((n, 3), np.float32), pixelDepth=pixel.copy())                # LightPath.cpp:18-21 (depth bits 0)


# ---- geometry helpers ---------------------------------------------------------------------------------------------------------
def geometric_normal(a, b, c):
    """Unit normal of the winding (a, b, c), float64.  (The reference reads per-triangle normals from its scene file,
    main.cpp:174; the project recomputes them: cross(b - a, c - a), normalised.)"""
    a, b, c = (np.asarray(v, np.float64)[..., :3] for v in (a, b, c))
    n = np.cross(b - a, c - a)
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / np.sqrt((n * n).sum(-1))[..., None]


def pack_shade_tris(n0, n1, n2, ng, material):
    """The 64-byte records `n0 n1 n2 ng material pad` a test hands to the kernels."""
    out = np.zeros(len(material), SHADE_TRI_DTYPE)
    with np.errstate(invalid="ignore"):
        for name, v in (("n0", n0), ("n1", n1), ("n2", n2), ("ng", ng)):
            out[name] = np.asarray(v).astype(np.float32)
    out["material"] = np.asarray(material, np.uint32)
    return out


def shade_tris_of_scene(vertices, indices, normals, triangle_materials):
    """The records of a whole scene (vertices / normals [V, >=3], indices 3 per triangle)."""
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32)[:, :3]
    nrm = np.asarray(normals, np.float32)[:, :3]
    # the edges are float32 differences in the project (the vertices are float32 data); the normalisation is float64 here
    e1 = (v[idx[:, 1]] - v[idx[:, 0]]).astype(np.float64)
    e2 = (v[idx[:, 2]] - v[idx[:, 0]]).astype(np.float64)
    ng = np.cross(e1, e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ng = ng / np.sqrt((ng * ng).sum(1))[:, None]
    return pack_shade_tris(nrm[idx[:, 0]], nrm[idx[:, 1]], nrm[idx[:, 2]], ng, np.asarray(triangle_materials, np.uint32) & 3)


def gather_tris(tris, triangle):
    """Per-record (n0, n1, n2, ng, material) for shade_surface; out-of-range indices read record 0 (the guard drops them)."""
    t = np.asarray(triangle, np.uint32)
    safe = np.where(t < len(tris), t, 0).astype(np.int64)
    r = tris[safe]
    return r["n0"], r["n1"], r["n2"], r["ng"], r["material"]


def _sample_material(ke, rnd, normal, wo):
    """orc.pt_sample_material(..., exact_trig=True) for many samples of ONE material (the oracle's entry takes one lane a call)."""
    lib = orc.lib()
    ke = np.ascontiguousarray(ke, np.float32)
    rnd, normal, wo = (np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (rnd, normal, wo))
    n = len(rnd)
    wi, colour, diffuse = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
    vp, fn = C.c_void_p, lib.orc_pt_sample_material
    pk, pr, pn, pw, pi, pc = (a.ctypes.data for a in (ke, rnd, normal, wo, wi, colour))
    for i in range(n):
        o = 12 * i
        diffuse[i] = fn(vp(pk), vp(pr + o), vp(pn + o), vp(pw + o), 1, vp(pi + o), vp(pc + o)) != 0
    return wi, colour, diffuse


# ---- one surface interaction --------------------------------------------------------------------------------------------------
def shade_surface(materials, ray, hit, path, sample, n0, n1, n2, ng, material, max_depth, triangle_count):
    """PathTracingRenderer.cpp:113-422 for records that are not misses (a miss comes back dead with infinite margins).
    materials: dict(kd=[4,3], eta=[4]) float32.  ray/hit/path: RAY_DTYPE / HIT_DTYPE / PATH_DTYPE arrays; sample u32[n];
    n0, n1, n2, ng: float32 [n,3] of the record's triangle; material u32[n].
    -> dict(alive bool[n]; origin, dir, weight float64 [n,3]; minT, maxT float32; pixelDepth u32; sample u32;
            margins {name: float64[n]} = distance of each decision's quantity from its threshold (inf where the decision was
            not reached or cannot flip), sides_disagree bool[n] (departure 4))."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return _shade_surface(materials, ray, hit, path, sample, n0, n1, n2, ng, material, max_depth, triangle_count)


def _shade_surface(materials, ray, hit, path, sample, n0, n1, n2, ng, material, max_depth, triangle_count):
    n = len(ray)
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    kd, eta = f64(materials["kd"]).reshape(4, 3), f64(materials["eta"]).reshape(4)
    tri = np.asarray(hit["triangle"], np.uint32)
    pd = np.asarray(path["pixelDepth"], np.uint32)
    pixel, depth = pd & np.uint32(0xFFFFFF), pd >> np.uint32(24)                                 # :114-115, :505
    sample = np.asarray(sample, np.uint32)
    go = (tri.astype(np.int64) < int(triangle_count)) & (depth < np.uint32(max_depth))          # :120
    inf = np.full(n, np.inf)
    margins = {k: inf.copy() for k in GUARDS}

    u, v = f64(hit["u"]), f64(hit["v"])
    w = 1.0 - (u + v)                                                                            # :218
    nrm = f64(n0) * w[:, None] + f64(n1) * u[:, None] + f64(n2) * v[:, None]                     # :261-274: w, u, v weigh corners 0, 1, 2
    nrm = nrm / np.sqrt((nrm * nrm).sum(1))[:, None]                                             # :282-286 (departure 3)
    d = f64(ray["dir"])
    wo = -d                                                                                      # :373-375
    gn = f64(ng)
    g_wo = (gn * wo).sum(1)                                                                      # :342-345 (sign of dot(rayDir, Ng))
    n_wo = (nrm * wo).sum(1)
    sides_disagree = go & ((g_wo < 0) != (n_wo < 0))
    margins["ng_wo"] = np.where(go, np.abs(g_wo), np.inf)
    margins["n_wo"] = np.where(go, np.abs(n_wo), np.inf)
    gv = np.where((g_wo < 0)[:, None], -gn, gn)        # Ng on the viewer's side: where wi must lie (:400-402) and where the origin moves (:404-412)
    nrm = np.where((n_wo < 0)[:, None], -nrm, nrm)     # the shading normal on the viewer's side (departure 4)
    margins["n_x"] = np.where(go, np.abs(np.abs(nrm[:, 0]) - WIDE), np.inf)                      # Materials.cpp:82-83

    key = path_key(pixel, sample)
    rnd = np.stack([uniform_keyed(key, depth.astype(np.uint64) + 1, s) for s in (3, 4, 5)], 1)  # :351-353: three numbers per interaction
    m = np.asarray(material, np.uint32) & np.uint32(3)
    # the decisions inside the material, in float64, for their margins (Materials.cpp:57-58, :67-69, :77-79, :123-128)
    cosi = np.maximum(np.where(np.isnan(n_wo), 0.0, np.abs(n_wo)), 0.0)
    e = eta[m]
    k = 1.0 + e * e * (cosi * cosi - 1.0)
    cost = np.sqrt(np.where(k >= 0, k, 0.0))
    rper = (e * cosi - cost) / (e * cosi + cost)
    rpar = -(e * cost - cosi) / (e * cost + cosi)
    fresnel = np.where(k < 0, 1.0, 0.5 * (rpar * rpar + rper * rper))
    s0 = 3.0 * fresnel
    total = s0 + kd[m].sum(1)
    pick = rnd[:, 2] * total
    margins["k"] = np.where(go, np.abs(k), np.inf)
    rel = np.abs(pick - s0) / np.abs(s0)              # relative to the threshold (s0 == 0, eta == 1: nothing is "near" it)
    margins["pick"] = np.where(go & np.isfinite(rel), rel, np.inf)

    wi, colour = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    for mi in range(4):
        sel = np.nonzero(go & (m == mi))[0]
        if len(sel):
            ke = np.array([*materials["kd"][mi], materials["eta"][mi]], np.float32)
            a, b, _ = _sample_material(ke, rnd[sel], nrm[sel], wo[sel])                          # :380
            wi[sel], colour[sel] = a, b
    wgt = f64(path["weight"]) * colour                                                           # :390-392
    big = np.where(np.isnan(wgt), -np.inf, wgt).max(1)
    heavy = big > CUT                                                                            # :394-398 (NaN compares false: a zero denominator dies here)
    alive = go & heavy
    margins["cut"] = np.where(go & np.isfinite(big), np.abs(big - CUT) / CUT, np.inf)
    wi_g = (wi * gv).sum(1)                                                                      # :400
    alive &= wi_g > 0                                                                            # :402: wi on the side the ray came from (no transmission)
    margins["wi_ng"] = np.where(go & heavy & ~np.isnan(wi_g), np.abs(wi_g), np.inf)
    p = f64(ray["origin"]) + d * f64(hit["t"])[:, None] + gv * OFFSET                            # :355-357, :410-412
    alive &= np.isfinite(p.astype(np.float32).sum(1, dtype=np.float32)) & np.isfinite(wi.sum(1))  # :416-419 (departure 5)
    return dict(alive=alive, origin=p, dir=wi, weight=wgt, minT=np.full(n, MIN_T, np.float32), maxT=np.full(n, MAX_T, np.float32),
                pixelDepth=(pd + np.uint32(0x1000000)).astype(np.uint32),                       # :414
                sample=sample, margins=margins, sides_disagree=sides_disagree)


def borderline(margins):
    """Records with a decision inside its guard: the float32 code may take the other branch there."""
    out = None
    for name, guard in GUARDS.items():
        b = margins[name] < guard
        out = b if out is None else (out | b)
    return out


# ---- one miss -----------------------------------------------------------------------------------------------------------------
def miss_contribution(hit, path):
    """PathTracingRenderer.cpp:505-563 in the project's fixed point (departure 6): int64 [n,3] to be ADDED to
    frame[pixel * 3 + ch] and valid[n,3].  EXACT: float32 x float32 is exact in float64, so is the factor 2^20, and llround is
    round-half-away-from-zero."""
    env = np.stack([hit["t"], hit["u"], hit["v"]], 1).astype(np.float32).astype(np.float64)      # :530-533 / :560: radiance rides in t, u, v
    with np.errstate(invalid="ignore", over="ignore"):
        v = env * np.asarray(path["weight"], np.float32).astype(np.float64)
        valid = np.isfinite(v)
        s = np.where(valid, v, 0.0) * FIXED
        r = np.where(s >= 0, np.floor(s + 0.5), np.ceil(s - 0.5))
    return r.astype(np.int64), valid


def accumulate_misses(hit, path, frame_words):
    """The frame (int64 words, pixel * 3 + ch) after adding every miss record of (hit, path): exact integer sums."""
    frame = np.zeros(frame_words, np.int64)
    miss = np.asarray(hit["triangle"]) == MISS
    add, valid = miss_contribution(hit[miss], path[miss])
    pixel = (path["pixelDepth"][miss] & np.uint32(0xFFFFFF)).astype(np.int64)
    for ch in range(3):
        np.add.at(frame, pixel[valid[:, ch]] * 3 + ch, add[valid[:, ch], ch])
    return frame
