"""Shared by the refit tests (tests/test_refit_host.py, tests/test_gpu_refit.py): displacements, an independent numpy restatement of the
refit rule (include/racc_hip.h, racc_host_blobs_refit) and a hand-made scene whose coordinates are +0.0 and -0.0."""
import numpy as np

from oracle import oracle as orc

NEG0, POS0 = np.float32("-0.0"), np.float32("0.0")


def displaced(vertices, amplitude, phase=0.0):
    """A smooth displacement of every vertex: sines of the position with a wavelength of the scene's size, `amplitude` units high."""
    v = np.array(vertices, np.float32, copy=True)
    p = v[:, :3].astype(np.float64)
    size = float((p.max(0) - p.min(0)).max())
    w = 2.0 * np.pi / size
    d = np.stack([np.sin(w * p[:, 2] + phase), 0.5 * np.sin(w * p[:, 0] + 1.0 + phase), np.cos(w * p[:, 1] + 2.0 * phase)], 1)
    v[:, :3] = (p + amplitude * d).astype(np.float32)
    return v


def scene_size(vertices):
    p = np.asarray(vertices)[:, :3]
    return float((p.max(0) - p.min(0)).max())


def pair_vertex_indices(blobs, indices):
    """[pair_count, 4] vertex indices of every pair: remap[2p] = t0 | ea << 30, remap[2p+1] = t1 | (eb+1) << 30 or 0 (lone: p3 = p1)."""
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    n = int(blobs["pair_count"])
    r0, r1 = blobs["remap"][0:2 * n:2].astype(np.int64), blobs["remap"][1:2 * n:2].astype(np.int64)
    t0, ea = r0 & 0x3FFFFFFF, r0 >> 30
    t1, eb = r1 & 0x3FFFFFFF, (r1 >> 30) - 1
    rows = np.arange(n)
    q = np.stack([idx[t0, ea], idx[t0, (ea + 1) % 3], idx[t0, (ea + 2) % 3], idx[t0, (ea + 1) % 3]], 1)
    paired = r1 != 0
    q[paired, 3] = idx[t1[paired], (eb[paired] + 2) % 3]
    assert len(rows) == len(q)
    return q


def numpy_refit(blobs, vertices, indices):
    """The rule restated with numpy set operations: a pair record from its four vertices; a child box = min / max over ALL vertices below
    that child (so equality with it is also tightness: every plane is attained by a vertex of the subtree).  Float equality, not bytes:
    min / max over a set does not say which zero wins."""
    v = np.asarray(vertices, np.float32)[:, :3]
    q = pair_vertex_indices(blobs, indices)
    p0, p1, p2, p3 = (v[q[:, k]] for k in range(4))
    pairs = np.zeros(len(blobs["pairs"]), orc.PAIR_DTYPE)
    n = len(q)
    pairs["e1"][:n], pairs["e2"][:n], pairs["p0"][:n] = p0 - p1, p2 - p0, p0
    e3 = p3 - p0
    pairs["e3x"][:n], pairs["e3y"][:n], pairs["e3z"][:n] = e3[:, 0], e3[:, 1], e3[:, 2]
    pairs[n:] = pairs[0]
    pmin, pmax = v[q].min(1), v[q].max(1)           # per pair
    nodes = blobs["nodes"].copy()
    done = {}

    def box(ref):
        if ref & 0x80000000:
            i = ref & 0x7FFFFFFF
            if i not in done:
                l, r = box(int(nodes["first"][i])), box(int(nodes["last"][i]))
                nodes["leftMin"][i], nodes["leftMax"][i], nodes["rightMin"][i], nodes["rightMax"][i] = l[0], l[1], r[0], r[1]
                done[i] = (np.minimum(l[0], r[0]), np.maximum(l[1], r[1]))
            return done[i]
        first, cnt = ref & 0xFFFFFF, ref >> 24
        return pmin[first:first + cnt].min(0), pmax[first:first + cnt].max(0)

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    box(0x80000000)
    return dict(nodes=nodes, pairs=pairs, remap=blobs["remap"], pair_count=blobs["pair_count"])


def assert_planes_equal(got, want, what):
    for f in ("leftMin", "leftMax", "rightMin", "rightMax"):
        assert np.array_equal(got["nodes"][f], want["nodes"][f]), "%s: %s differs from the numpy restatement" % (what, f)
    for f in ("kind", "parent", "first", "last"):
        assert np.array_equal(got["nodes"][f], want["nodes"][f]), "%s: topology word %s changed" % (what, f)
    for f in ("e1", "e2", "p0", "e3x", "e3y", "e3z"):
        assert np.array_equal(got["pairs"][f], want["pairs"][f]), "%s: pair field %s differs from the numpy restatement" % (what, f)


def zero_sign_scene():
    """Hand-made blobs: ONE node; left = a leaf of one pair (the quad a, b, c, d as triangles 0 = (a, c, b), 1 = (c, a, d): p0 p1 p2 p3 =
    a c b d), right = the lone triangle 2 = (e, f, g).  Returns (blobs, geometry dict(vertices, indices), vertex sets A and B) — the sets
    differ in which coordinates are +0.0 and which -0.0; `blobs` holds A's records, worked out by hand below."""
    idx = np.array([[0, 2, 1], [2, 0, 3], [4, 5, 6]], np.uint32)

    def verts(s):      # s = -0.0 for set A, +0.0 for set B (and the other way round)
        t = -s
        return np.array([[t, s, 2, 1], [1, t, 2, 1], [1, 1, 2, 1], [s, 1, 2, 1],      # a b c d
                         [s, 5, s, 1], [3, 5, t, 1], [t, 6, s, 1]], np.float32)      # e f g
    va, vb = verts(NEG0), verts(POS0)
    blobs = hand_refit_zero_sign(va)
    blobs["nodes"]["kind"], blobs["nodes"]["first"], blobs["nodes"]["last"] = 1, (1 << 24) | 0, (1 << 24) | 1
    return blobs, dict(vertices=va, indices=idx), va, vb


def hand_refit_zero_sign(v):
    """The records of zero_sign_scene for vertex set `v`, by hand.  With s = v[0,1] (the sign pattern) and t = -s:
      left  fold a c b d:  x: t (a), 1, 1, s  -> min t (s < t is false for zeros), max 1;   y: s (a), 1, t, 1 -> min s, max 1;   z: 2
      right fold e f g f:  x: s (e), 3, t     -> min s, max 3;   y: 5, 5, 6 -> min 5, max 6;   z: s (e), t, s -> min s, max s (t > s is false)
    The select keeps the accumulator on a tie of zeros, so each zero plane carries the sign of the FIRST vertex folded — fmin / fmax
    would give (-0, +0) whatever the order."""
    s, t = v[0, 1], v[0, 0]
    assert s == 0 and t == 0 and np.signbit(s) != np.signbit(t)
    nodes = np.zeros(1, orc.GPU_NODE_DTYPE)
    nodes["leftMin"][0], nodes["leftMax"][0] = (t, s, 2), (1, 1, 2)
    nodes["rightMin"][0], nodes["rightMax"][0] = (s, 5, s), (3, 6, s)
    a, b, c, d, e, f, g = (v[i, :3] for i in range(7))
    pairs = np.zeros(32, orc.PAIR_DTYPE)
    for k, (p0, p1, p2, p3) in enumerate(((a, c, b, d), (e, f, g, f))):
        pairs[k]["e1"], pairs[k]["e2"], pairs[k]["p0"] = p0 - p1, p2 - p0, p0
        pairs[k]["e3x"], pairs[k]["e3y"], pairs[k]["e3z"] = p3 - p0
    pairs[2:] = pairs[0]
    remap = np.array([0 | (0 << 30), 1 | (1 << 30), 2, 0], np.uint32)
    return dict(nodes=nodes, pairs=pairs, remap=remap, pair_count=2)
