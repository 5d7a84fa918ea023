"""Shared by the bottom-level rebuild's tests (tests/test_scene_rebuild_host.py, tests/test_gpu_scene_rebuild.py): the rule of
rayaccel_amd/csrc/racc_scene_rebuild_rule.h restated a third time — numpy.float64 fields, Python's sort of (field, index) tuples, Karras's
per-node searches over arbitrary-precision integers — and the meshes that stress it."""
import numpy as np

from rayaccel_amd import engine

LEAF = 1 << 24
INNER = 0x80000000
ROOT = 0xFFFFFFFF
AXIS_BITS = 21
BOX_FIELDS = ("leftMin", "leftMax", "rightMin", "rightMax")
NODE_FIELDS = ("kind", "parent", "first", "last") + BOX_FIELDS


def height_bound(triangles):
    """Rule 9: one node per bit that can differ between two keys — 63 field bits, ceil(log2 T) index bits — and never more than T - 1."""
    return min(63 + int(np.ceil(np.log2(triangles))), triangles - 1)


def padded_pairs(triangles):
    return (triangles // 32 + 1) * 32


def fold(points):
    """The select of racc_host_blobs_refit folded over `points` [n, 3] in order, from the first: (min[3], max[3]) with its signs of zeros."""
    mn, mx = points[0].copy(), points[0].copy()
    for p in points[1:]:
        lower, higher = p < mn, p > mx
        mn[lower], mx[higher] = p[lower], p[higher]
    return mn, mx


def triangle_boxes(vertices, indices):
    """[T, 6] min, max: rule 1, vectorised over the triangles."""
    tri = np.asarray(vertices, np.float32)[:, :3][np.asarray(indices, np.int64).reshape(-1, 3)]      # [T, 3 vertices, 3 axes]
    mn, mx = tri[:, 0].copy(), tri[:, 0].copy()
    for k in (1, 2):
        p = tri[:, k]
        mn, mx = np.where(p < mn, p, mn), np.where(p > mx, p, mx)
    return np.concatenate([mn, mx], 1)


def numpy_keys(vertices, indices):
    """Rules 1-5: the sorted (field, triangle) tuples, fields as Python integers."""
    b = triangle_boxes(vertices, indices).astype(np.float64)
    c = (0.5 * b[:, :3] + 0.5 * b[:, 3:]).astype(np.float32)
    lo, hi = c.min(0), c.max(0)
    fields = [0] * len(c)
    for axis in range(3):
        if not hi[axis] > lo[axis]:
            continue
        v = (c[:, axis].astype(np.float64) - np.float64(lo[axis])) / (np.float64(hi[axis]) - np.float64(lo[axis])) * float(1 << AXIS_BITS)
        q = np.minimum(np.floor(v), float((1 << AXIS_BITS) - 1)).astype(np.int64)
        for t, qq in enumerate(q.tolist()):
            f = 0
            for bit in range(AXIS_BITS):
                f |= ((qq >> bit) & 1) << (3 * bit + 2 - axis)
            fields[t] |= f
    return sorted((f, t) for t, f in enumerate(fields))


def numpy_lbvh(vertices, indices):
    """Rules 1-8 and the height: dict(nodes, pairs, remap, pair_count, height) as racc_host_scene_rebuild returns them.  The hierarchy by
    Karras's searches, one node at a time, over the 95-bit integers field << 32 | index."""
    vertices = np.asarray(vertices, np.float32)[:, :3]
    tris = np.asarray(indices, np.int64).reshape(-1, 3)
    keys = numpy_keys(vertices, indices)
    n = len(keys)
    big = [(f << 32) | t for f, t in keys]

    def delta(i, j):
        return -1 if j < 0 or j >= n else 95 - (big[i] ^ big[j]).bit_length()

    nodes = np.zeros(n - 1, engine.GPU_NODE_DTYPE)
    nodes["kind"] = 1
    nodes["parent"][0] = ROOT
    span = [None] * (n - 1)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) > delta(i, i - 1) else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        split = i + s * d + min(d, 0)
        a, b = min(i, j), max(i, j)
        span[i] = (a, split, b)
        for field, lo_, hi_, child in (("first", a, split, split), ("last", split + 1, b, split + 1)):
            if lo_ == hi_:
                nodes[field][i] = LEAF | lo_
            else:
                nodes[field][i] = INNER | child
                nodes["parent"][child] = i
    # boxes: children before parents — a node's range lies inside its parent's, so by descending width of the range would do; a walk is plainer
    order, height = [(0, 1)], 0
    for node, depth in order:
        height = max(height, depth)
        for ref in (int(nodes["first"][node]), int(nodes["last"][node])):
            if ref & INNER:
                order.append((ref & 0x7FFFFFFF, depth + 1))
    assert len(order) == n - 1, "a node is reached twice or never"
    leaf_boxes = triangle_boxes(vertices, indices)
    for node, _ in reversed(order):
        for ref, mn, mx in ((int(nodes["first"][node]), "leftMin", "leftMax"), (int(nodes["last"][node]), "rightMin", "rightMax")):
            if ref & INNER:
                c = nodes[ref & 0x7FFFFFFF]
                lo_, hi_ = fold(np.stack([c["leftMin"], c["rightMin"]]))[0], fold(np.stack([c["leftMax"], c["rightMax"]]))[1]
            else:
                box = leaf_boxes[keys[ref & 0xFFFFFF][1]]
                lo_, hi_ = box[:3], box[3:]
            nodes[mn][node], nodes[mx][node] = lo_, hi_
    pairs = np.zeros(padded_pairs(n), engine.PAIR_DTYPE)
    order_t = np.array([t for _, t in keys], np.int64)
    p0, p1, p2 = (vertices[tris[order_t, k]] for k in range(3))
    pairs["e1"][:n], pairs["e2"][:n], pairs["p0"][:n] = p0 - p1, p2 - p0, p0
    e3 = p1 - p0
    pairs["e3x"][:n], pairs["e3y"][:n], pairs["e3z"][:n] = e3[:, 0], e3[:, 1], e3[:, 2]
    pairs[n:] = pairs[0]
    remap = np.zeros(2 * n, np.uint32)
    remap[0::2] = order_t
    return dict(nodes=nodes, pairs=pairs, remap=remap, pair_count=n, height=height)


# ------------------------------------------------------------------------------------------------------------ the meshes
def soup(triangles, seed, extent=4.0, size=1.5):
    """`triangles` random triangles, three vertices of its own each."""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-extent, extent, (triangles, 1, 3))
    v = (centres + rng.uniform(-size, size, (triangles, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * triangles, dtype=np.uint32)


def common_centre(triangles):
    """Triangles of different sizes around one centre: every box is symmetric about (3, -2, 5), so every field ties and the index decides."""
    assert triangles <= 4096
    s = (1.0 + np.arange(triangles, dtype=np.float32) / np.float32(4096))[:, None, None]      # 3 +- s etc. are exact in binary32: the centres are equal as bits
    corners = np.float32([[-1, -1, -1], [1, 1, 1], [1, -1, 0]])[None]      # the box of these three is [-1, 1]^3
    v = (np.float32([3, -2, 5]) + s * corners).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * triangles, dtype=np.uint32)


def on_one_axis(triangles, seed):
    """Congruent triangles translated along x only: hi == lo on two axes."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-50, 50, triangles).astype(np.float32)
    base = np.float32([[0, 0, 0], [0, 1, 0], [0, 0, 1]])
    v = np.tile(base, (triangles, 1, 1))
    v[:, :, 0] = x[:, None]
    return v.reshape(-1, 3), np.arange(3 * triangles, dtype=np.uint32)


def duplicated(triangles, seed):
    """A soup of triangles // 4 whose index triples appear four times each (shuffled): equal keys but for the index."""
    v, idx = soup(max(triangles // 4, 1), seed)
    tri = np.tile(idx.reshape(-1, 3), (4, 1))
    return v, np.ascontiguousarray(tri[np.random.RandomState(seed + 1).permutation(len(tri))]).reshape(-1)


def chain(length=40):
    """Triangles whose centres sit at 2^-k, k = 0 .. length - 1, on the x axis: each of the 21 field bits of x cuts one triangle off the
    rest, the index bits share out those that fall into the last cell — a tree far deeper than any kernel's LDS stack."""
    x = (2.0 ** -np.arange(length)).astype(np.float32)
    v = np.zeros((length, 3, 3), np.float32)
    v[:, :, 0] = x[:, None]                   # flat in x: the centre is the vertices' x exactly
    v[:, 1, 1] = 0.5; v[:, 1, 2] = -0.25
    v[:, 2, 2] = 0.5; v[:, 2, 1] = -0.25
    v[:, 0, 1] = -0.25; v[:, 0, 2] = -0.25     # every triangle covers (y, z) near the origin: a ray along x meets them all
    return v.reshape(-1, 3), np.arange(3 * length, dtype=np.uint32)


def moved(vertices, seed, amount=3.0):
    """The same mesh with every vertex displaced: new centres, a new order."""
    rng = np.random.RandomState(seed)
    return (np.asarray(vertices, np.float32)[:, :3] + rng.uniform(-amount, amount, (len(vertices), 3))).astype(np.float32)


def rays_at(vertices, indices, count, seed):
    """`count` rays towards points on the mesh's triangles (every seventh beside its target), from three quarters of the mesh's diagonal
    away.  Rays whose closest hit — the double-precision brute force's, nothing of the code under test — grazes its triangle (|cos| < 0.1)
    are left out: binary32 t, u, v lose digits with 1 / cos, which is the pair test's rounding and not a tree's doing."""
    from oracle import oracle as orc
    from rayaccel_amd import synth
    rng = np.random.RandomState(seed)
    v = np.asarray(vertices, np.float32)[:, :3].astype(np.float64)
    tri = v[np.asarray(indices, np.int64).reshape(-1, 3)]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-30)
    ext = np.maximum(v.max(0) - v.min(0), 1e-3)
    n = 2 * count
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    which = rng.randint(0, len(tri), n)
    target = (tri[which] * w[:, :, None]).sum(1)
    target[::7] += rng.normal(0, 0.05, (len(target[::7]), 3)) * ext
    direction = normal[which] * rng.choice([-1.0, 1.0], (n, 1)) + 0.6 * rng.normal(size=(n, 3)) / np.sqrt(3.0)
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    origin = target - direction * (0.75 * np.linalg.norm(ext))
    rays = np.zeros(n, synth.RAY_DTYPE)
    rays["origin"], rays["dir"] = origin.astype(np.float32), direction.astype(np.float32)
    rays["minT"], rays["maxT"] = 0.0, np.float32(1e6)
    hit = orc.brute_closest(vertices, indices, rays)[0]
    cos = np.abs((normal[np.minimum(hit, len(tri) - 1)] * rays["dir"].astype(np.float64)).sum(1))
    keep = np.nonzero((hit == 0xFFFFFFFF) | (cos >= 0.1))[0]
    assert len(keep) >= count, "too many grazing rays"
    return np.ascontiguousarray(rays[keep[:count]])
