"""Inputs shared by tests/test_pt_reference.py (host hooks, no GPU) and tests/test_gpu_pt_kernels.py (the two kernels): ONE
seeded generator of shading records, the comparison of a shading pass with oracle/pt_reference.py, and a reader for the
per-triangle shading records of a scene file.

Every float input is normal or zero, except in the class "denormal" (which exists to check that host and device agree under
flush-to-zero; the float64 reference is given those inputs with the denormals read as zero, as both consumers read them)."""
import struct

import numpy as np

from oracle import pt_reference as ref
from rayaccel_amd.engine import PATH_DTYPE, RAY_DTYPE, RESULT_DTYPE, SHADE_TRI_DTYPE

assert SHADE_TRI_DTYPE == ref.SHADE_TRI_DTYPE and PATH_DTYPE == ref.PATH_DTYPE

SEED = 20240611
MAX_DEPTH = 5
FRAME_W, FRAME_H = 300, 200
FRAME_WORDS = FRAME_W * FRAME_H * 3
# eta < 1, eta > 1 (k < 0 at grazing incidence: the total-internal-reflection branch, Materials.cpp:79), eta = 1 twice — once with
# kd = 0, where Fresnel is 0, the diffuse lobe is always picked and the path dies on the zero denominator (Materials.cpp:138)
MATERIALS = dict(kd=np.array([[0.8, 0.7, 0.6], [0.1, 0.9, 0.2], [0.0, 0.0, 0.0], [0.05, 0.02, 0.6]], np.float32),
                 eta=np.array([1.0 / 1.4, 1.5, 1.0, 1.0], np.float32))
# what the consumers hard-code for a scene file (Renderer/main.cpp:165-168)
RENDER_MATERIALS = dict(kd=np.array([[0.8] * 3, [0.1] * 3, [0.6] * 3, [0.3] * 3], np.float32),
                        eta=np.array([np.float32(1.0) / np.float32(1.4)] * 2 + [np.float32(1.0) / np.float32(1.2)] * 2, np.float32))

# Tolerances (float32 consumers against the float64 reference)
TOL_DIR = 3e-6            # next direction, per component (tests/test_host_build.py holds the same arithmetic to this bound)
TOL_WEIGHT = 2e-4         # colour weights, relative to incoming weight x colour (ditto)
TOL_ORIGIN = 4 * 2.0 ** -24   # next origin: |delta| <= 4 ulp-halves of (|o| + |t d| + 1e-4): three float32 roundings + the normal's own error
BORDERLINE_CAP = 0.01     # share of surface-hit records that may sit inside a decision guard


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def hand_made_tris():
    """A few triangles no scene would hold.  Returns (ShadeTri records, dict name -> index within them)."""
    names, rows = {}, []

    def add(name, n0, n1, n2, ng, material):
        names[name] = len(rows)
        rows.append((n0, n1, n2, ng, material))

    # the unit right triangle (0,0,0) (1,0,0) (0,1,0) with three different vertex normals
    add("right", _unit(np.array([0.2, 0.1, 1.0])), _unit(np.array([-0.3, 0.2, 1.0])), _unit(np.array([0.1, -0.4, 1.0])), np.array([0.0, 0.0, 1.0]), 0)
    add("zero_area", np.array([0.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([np.nan] * 3), 0)      # Ng = 0/0
    add("cancelling", np.array([0.0, 1.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0]), 0)  # N = 0/0 at u = v = 1/4
    for k, a in enumerate((0.0999, 0.1001, -0.0999, -0.1001, 0.05, 0.2, 0.0)):         # flat normals with |x| on both sides of 0.1 (Materials.cpp:83)
        n = np.array([a, np.sqrt(1 - a * a) * 0.6, np.sqrt(1 - a * a) * 0.8])
        add("nx%d" % k, n, n, n, n, k & 3)
    n0, n1, n2, ng, mat = (np.array([r[i] for r in rows]) for i in range(5))
    return ref.pack_shade_tris(n0, n1, n2, ng, mat), names


def tri_table(scene):
    """The small scene's triangles (vertex normals = area-weighted face normals, materials 0..3 in turn) + the hand-made ones."""
    v = scene["vertices"][:, :3].astype(np.float64)
    idx = scene["indices"].reshape(-1, 3)
    fn = np.cross(v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, idx[:, k], fn)
    vn = (vn / np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    tris = ref.shade_tris_of_scene(scene["vertices"], idx, vn, np.arange(len(idx)) & 3)
    hand, names = hand_made_tris()
    return np.concatenate([tris, hand]), {k: len(tris) + i for k, i in names.items()}


CLASSES = ("surface", "edge", "grazing", "nx", "cut", "one_channel", "depth", "guard", "zero_area", "cancelling", "far", "denormal",
           "miss", "miss_zero", "miss_nonfinite", "miss_big", "miss_negative", "miss_denormal")
# which class record i gets (i modulo the pattern); the same-pixel block of misses overrides a stretch of it in large batches
_PATTERN = ("surface", "miss", "surface", "edge", "surface", "grazing", "miss", "surface", "nx", "cut", "surface", "one_channel", "depth", "miss_zero",
            "surface", "guard", "grazing", "miss_nonfinite", "surface", "zero_area", "edge", "miss_big", "surface", "cancelling", "cut", "miss_negative",
            "surface", "far", "depth", "denormal", "surface", "miss_denormal", "grazing", "miss", "surface", "edge", "nx", "surface", "cut", "depth")
SAME_PIXEL = (1100, 1024, 300)      # records [1100, 1100 + 1024) miss into ONE pixel, the next 300 into its two neighbours (batches of >= 3000 records)


def make_records(count, tris, names, seed=SEED):
    """`count` shading records on the triangle table `tris`.  Returns dict(rays, hits, paths, samples, cls [count] class names).
    (pixel, sample) is unique per record: sample = 7 + record index."""
    rng = np.random.default_rng(seed + count)
    n = count
    cls = np.array([_PATTERN[i % len(_PATTERN)] for i in range(n)], dtype=object)
    block = n >= 3000
    if block:
        a, b, c = SAME_PIXEL
        cls[a:a + b + c] = "miss"
    is_miss = np.array([c.startswith("miss") for c in cls])
    T_scene = len(tris) - len(hand_made_tris()[0])

    rays, hits, paths = np.zeros(n, RAY_DTYPE), np.zeros(n, RESULT_DTYPE), np.zeros(n, PATH_DTYPE)
    samples = (np.arange(n, dtype=np.uint32) + np.uint32(7))

    # ---- surface records -----------------------------------------------------------------------------------------------------
    tri = rng.integers(0, T_scene, n).astype(np.uint32)
    nx_names = [k for k in names if k.startswith("nx")]
    tri[cls == "nx"] = np.array([names[nx_names[i % len(nx_names)]] for i in range(int((cls == "nx").sum()))], np.uint32)
    tri[cls == "zero_area"] = names["zero_area"]
    tri[cls == "cancelling"] = names["cancelling"]
    g = np.nonzero(cls == "guard")[0]
    tri[g[0::2]] = len(tris)                      # == triangleCount: dies, nothing gathered
    tri[g[1::2]] = 0xFFFFFFFE
    # barycentrics: interior; the three edges and the three corners in class "edge"
    u = rng.uniform(0.02, 0.96, n)
    v = rng.uniform(0.02, 0.98, n) * (0.98 - u)
    e = np.nonzero(cls == "edge")[0]
    kind = np.arange(len(e)) % 6
    u[e[kind == 0]] = 0.0
    v[e[kind == 1]] = 0.0
    u32 = u.astype(np.float32)
    v32 = v.astype(np.float32)
    v32[e[kind == 2]] = np.float32(1.0) - u32[e[kind == 2]]          # u + v = 1
    u32[e[kind == 3]], v32[e[kind == 3]] = 1.0, 0.0
    u32[e[kind == 4]], v32[e[kind == 4]] = 0.0, 1.0
    u32[e[kind == 5]], v32[e[kind == 5]] = 0.0, 0.0
    c = cls == "cancelling"
    u32[c], v32[c] = 0.25, 0.25
    # directions: from both sides of the triangle; |cos| to the geometric normal in [0.2, 1], or grazing in [5e-3, 2e-2]
    ng = tris["ng"][np.where(tri < len(tris), tri, 0)].astype(np.float64)
    ng = np.where(np.isnan(ng), np.array([0.0, 0.0, 1.0]), ng)
    cosv = rng.uniform(0.2, 1.0, n)
    gz = cls == "grazing"
    cosv[gz] = rng.uniform(5e-3, 2e-2, int(gz.sum()))
    cosv *= np.where(rng.random(n) < 0.4, -1.0, 1.0)
    rnd = _unit(rng.normal(size=(n, 3)))
    tang = _unit(rnd - ng * (rnd * ng).sum(1, keepdims=True))
    wo = ng * cosv[:, None] + tang * np.sqrt(1 - cosv * cosv)[:, None]
    rays["dir"] = (-wo).astype(np.float32)
    rays["origin"] = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    rays["minT"], rays["maxT"] = 1e-3, 1e6
    t = rng.uniform(0.5, 250.0, n).astype(np.float32)
    t[cls == "far"] = np.inf                      # the next origin is not finite: the path ends
    hits["triangle"], hits["t"], hits["u"], hits["v"] = tri, t, u32, v32
    # weights: ordinary; around the 0.01 cut (colour weights are of order 1); one channel alone above it
    w = rng.uniform(0.05, 1.0, (n, 3))
    k = cls == "cut"
    w[k] = rng.uniform(0.002, 0.04, (int(k.sum()), 3))
    k = np.nonzero(cls == "one_channel")[0]
    w[k] = 1e-4
    w[k, np.arange(len(k)) % 3] = rng.uniform(0.3, 1.0, len(k))
    w = w.astype(np.float32)
    k = np.nonzero(cls == "denormal")[0]
    w[k, np.arange(len(k)) % 3] = np.float32(1e-40)          # a denormal channel among normal ones
    depth = rng.integers(0, MAX_DEPTH, n).astype(np.uint32)
    pixel = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    k = np.nonzero(cls == "depth")[0]
    depth[k] = (np.arange(len(k)) % (MAX_DEPTH + 1)).astype(np.uint32)      # 0 .. maxDepth: the last one ends the path
    depth[k[len(k) // 2:]] = np.where(np.arange(len(k) - len(k) // 2) % 2 == 0, MAX_DEPTH - 1, MAX_DEPTH)
    pixel[k] = 0xFFFFFF                                                   # every pixel bit next to the depth bits set

    # ---- misses: the environment's radiance rides in t, u, v ---------------------------------------------------------------------
    m = np.nonzero(is_miss)[0]
    rad = rng.uniform(0.01, 4.0, (n, 3)).astype(np.float32)
    k = np.nonzero(cls == "miss_zero")[0]
    rad[k, np.arange(len(k)) % 3] = 0.0                                   # no atomic is issued for that channel
    k = np.nonzero(cls == "miss_nonfinite")[0]
    rad[k, np.arange(len(k)) % 3] = np.where(np.arange(len(k)) % 2 == 0, np.inf, np.nan).astype(np.float32)      # that channel is skipped, the others added
    k = cls == "miss_big"
    rad[k] = rng.uniform(0.5e6, 1.0e6, (int(k.sum()), 3)).astype(np.float32)      # weight x radiance near 2^40 fixed-point units
    k = np.nonzero(cls == "miss_negative")[0]
    rad[k, np.arange(len(k)) % 3] *= -1.0                                 # a negative long long added as unsigned long long wraps as intended
    k = np.nonzero(cls == "miss_denormal")[0]
    w[k, np.arange(len(k)) % 3] = np.float32(1e-40)                       # a denormal weight times a huge radiance: 0.03 if it were not read as zero
    rad[k] = np.float32(3e38)
    w[k] = np.where(w[k] == np.float32(1e-40), w[k], np.float32(1e-38) * rng.uniform(1.2, 3.0, (len(k), 3)).astype(np.float32))
    pixel[m] = rng.integers(0, FRAME_W * FRAME_H, len(m)).astype(np.uint32)
    depth[m] = rng.integers(0, MAX_DEPTH + 1, len(m)).astype(np.uint32)
    if block:
        a, b, c = SAME_PIXEL
        p0 = 123 * FRAME_W + 45
        pixel[a:a + b] = p0
        pixel[a + b:a + b + c] = p0 + np.where(np.arange(c) % 2 == 0, 1, -1)
    hits["triangle"][m] = 0xFFFFFFFF
    hits["t"][m], hits["u"][m], hits["v"][m] = rad[m, 0], rad[m, 1], rad[m, 2]
    paths["weight"] = w
    paths["pixelDepth"] = pixel | (depth << np.uint32(24))
    assert len(set(zip(pixel.tolist(), samples.tolist()))) == n
    return dict(rays=rays, hits=hits, paths=paths, samples=samples, cls=cls)


def daz(a):
    """A float32 array with its denormals read as zero (what both consumers do with them)."""
    a = np.array(a, np.float32)
    tiny = (np.abs(a) < np.finfo(np.float32).tiny) & (a != 0)
    a[tiny] = 0.0
    return a


def reference_pass(tris, materials, max_depth, rec):
    """oracle/pt_reference.py over one batch of records: shade_surface + miss contributions + the borderline mask."""
    rays, hits, paths = rec["rays"].copy(), rec["hits"].copy(), rec["paths"].copy()
    paths["weight"] = daz(paths["weight"])
    for f in ("t", "u", "v"):
        hits[f] = daz(hits[f])
    n0, n1, n2, ng, mat = ref.gather_tris(tris, hits["triangle"])
    out = ref.shade_surface(materials, rays, hits, paths, rec["samples"], n0, n1, n2, ng, mat, max_depth, len(tris))
    out["borderline"] = ref.borderline(out["margins"])
    miss = hits["triangle"] == ref.MISS
    out["surface"] = ~miss & (hits["triangle"] < len(tris)) & ((paths["pixelDepth"] >> 24) < max_depth)
    out["miss"] = miss
    out["contrib"], out["valid"] = ref.miss_contribution(hits, paths)
    out["contrib"][~miss] = 0
    out["valid"][~miss] = False
    return out


def compare_with_reference(label, got_alive, got_rays, got_paths, rec, expect, worst=None):
    """One shading pass (uncompacted: entry i belongs to record i) against reference_pass's result.  The alive sets may differ
    only at borderline records, whose share of the surface hits is capped; every other survivor's next ray and payload are held
    to the tolerances.  Prints the share and the largest deviations; `worst` (a dict) collects the maxima across calls."""
    surface, border = expect["surface"], expect["borderline"] & expect["surface"]
    share = border.sum() / max(int(surface.sum()), 1)
    print("%s: %d records, %d surface hits, %d alive, borderline share %.4f%% (%d), normals on different sides %d"
          % (label, len(got_alive), surface.sum(), expect["alive"].sum(), 100 * share, border.sum(), expect["sides_disagree"].sum()))
    assert share <= BORDERLINE_CAP, "%s: %.3f%% of the surface hits are inside a decision guard" % (label, 100 * share)
    firm = ~border
    wrong = np.nonzero(firm & (got_alive != expect["alive"]))[0]
    assert len(wrong) == 0, "%s: alive flag differs from the reference at %d records, first %d (class %s): margins %s" % (
        label, len(wrong), wrong[0], rec["cls"][wrong[0]], {k: float(v[wrong[0]]) for k, v in expect["margins"].items()})
    s = np.nonzero(firm & expect["alive"])[0]
    if not len(s):
        return
    r, p = got_rays[s], got_paths[s]
    # exact fields: minT, maxT, pixel | depth + 1
    assert np.array_equal(r["minT"].view(np.uint32), expect["minT"][s].view(np.uint32)), label + ": minT"
    assert np.array_equal(r["maxT"].view(np.uint32), expect["maxT"][s].view(np.uint32)), label + ": maxT"
    assert np.array_equal(p["pixelDepth"], expect["pixelDepth"][s]), label + ": pixelDepth"
    d_dir = np.abs(r["dir"].astype(np.float64) - expect["dir"][s])
    o = rec["rays"]["origin"][s].astype(np.float64)
    td = rec["rays"]["dir"][s].astype(np.float64) * rec["hits"]["t"][s].astype(np.float64)[:, None]
    bound_o = TOL_ORIGIN * (np.abs(o) + np.abs(td) + 1e-4)
    d_org = np.abs(r["origin"].astype(np.float64) - expect["origin"][s]) / bound_o
    w_ref = expect["weight"][s]
    d_w = np.abs(p["weight"].astype(np.float64) - w_ref) / np.maximum(np.abs(w_ref), 1e-300)
    d_w = np.where(w_ref == 0, np.where(p["weight"] == 0, 0.0, np.inf), d_w)
    print("%s: largest deviations: direction %.3g (bound %.3g), origin %.3g of its bound, weight %.3g relative (bound %.3g)"
          % (label, d_dir.max(), TOL_DIR, d_org.max(), d_w.max(), TOL_WEIGHT))
    if worst is not None:
        for k, val in (("dir", d_dir.max()), ("origin", d_org.max()), ("weight", d_w.max()), ("share", share)):
            worst[k] = max(worst.get(k, 0.0), float(val))
    assert d_dir.max() <= TOL_DIR, "%s: next direction off by %.3g at record %d" % (label, d_dir.max(), s[np.argmax(d_dir.max(1))])
    assert d_org.max() <= 1.0, "%s: next origin off by %.3g of its bound at record %d" % (label, d_org.max(), s[np.argmax(d_org.max(1))])
    assert d_w.max() <= TOL_WEIGHT, "%s: weight off by %.3g (relative) at record %d" % (label, d_w.max(), s[np.argmax(d_w.max(1))])


_HEADER = struct.Struct("<3I4H10f")


def scene_file_tris(path):
    """The per-triangle shading records of a scene file in the reference's layout (Renderer/main.cpp:117-191): indices,
    materials, [per-triangle normals skipped], vertices, vertex normals."""
    with open(path, "rb") as f:
        hdr = _HEADER.unpack(f.read(60))
        _, V, T = hdr[:3]
        idx = np.frombuffer(f.read(T * 12), "<u4").reshape(T, 3)
        mats = np.frombuffer(f.read(T * 2), "<u2")
        f.seek(T * 16, 1)
        v = np.frombuffer(f.read(V * 16), "<f4").reshape(V, 4)
        nrm = np.frombuffer(f.read(V * 16), "<f4").reshape(V, 4)
    return ref.shade_tris_of_scene(v, idx, nrm, mats)
