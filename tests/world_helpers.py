"""Shared by the instancing tests (tests/test_world_host.py, tests/test_gpu_world.py): transforms, the specification's ray transform in
numpy.float32 and the composed expectation — orc.traverse per distinct (instance, scene), smallest t, then lowest instance index."""
import ctypes as C
import ctypes.util

import numpy as np

from oracle import oracle as orc
from rayaccel_amd import synth

MISS = 0xFFFFFFFF
NO_INSTANCE = 0xFFFFFFFF


def affine(rotation=np.eye(3), scale=(1.0, 1.0, 1.0), translation=(0.0, 0.0, 0.0)):
    """[3,4] float32 object-to-world: rotation . diag(scale), then the translation."""
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = np.asarray(rotation, np.float64) @ np.diag(np.asarray(scale, np.float64))
    m[:, 3] = translation
    return m.astype(np.float32)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * k + (1 - c) * (k @ k)


IDENTITY = affine()


def adjugate_inverse(transforms):
    """The inverse of [N,3,4] float32 transforms evaluated in float64 — cofactors over the determinant, translation -(A^-1 b), the same
    expression tree as the library's, so the rounding to float32 is comparable bit for bit — returned in float64."""
    t = np.asarray(transforms, np.float32).astype(np.float64).reshape(-1, 3, 4)
    a, b = t[:, :, :3], t[:, :, 3]
    c = np.zeros_like(a)
    for r in range(3):
        for k in range(3):
            r1, r2, k1, k2 = (r + 1) % 3, (r + 2) % 3, (k + 1) % 3, (k + 2) % 3
            c[:, r, k] = a[:, r1, k1] * a[:, r2, k2] - a[:, r1, k2] * a[:, r2, k1]
    det = a[:, 0, 0] * c[:, 0, 0] + a[:, 0, 1] * c[:, 0, 1] + a[:, 0, 2] * c[:, 0, 2]
    inv = np.zeros_like(t)
    inv[:, :, :3] = np.transpose(c, (0, 2, 1)) / det[:, None, None]
    B = inv[:, :, :3]
    inv[:, :, 3] = -((B[:, :, 0] * b[:, 0:1] + B[:, :, 1] * b[:, 1:2]) + B[:, :, 2] * b[:, 2:3])
    return inv, det


def object_rays(inv, rays):
    """Section 1 of the specification in numpy.float32: o' = inv (o, 1), d' = inv (d, 0), each component ((m0 x + m1 y) + m2 z) + m3
    evaluated left to right (numpy never fuses), the same minT and maxT."""
    m = np.asarray(inv, np.float32).reshape(3, 4)
    o, d = rays["origin"].astype(np.float32), rays["dir"].astype(np.float32)
    out = rays.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            out["origin"][:, r] = ((m[r, 0] * o[:, 0] + m[r, 1] * o[:, 1]) + m[r, 2] * o[:, 2]) + m[r, 3]
            out["dir"][:, r] = (m[r, 0] * d[:, 0] + m[r, 1] * d[:, 1]) + m[r, 2] * d[:, 2]
    return out


def valid_rays(rays):
    return np.isfinite(rays["origin"]).all(1) & np.isfinite(rays["dir"]).all(1) & np.isfinite(rays["minT"]) & ~np.isnan(rays["maxT"])


def compose(inv, blobs_per_instance, rays, threads=16):
    """The expected world result: (Result[N], instance[N], per-instance hit mask [I, N]).  `blobs_per_instance[i]` = the blobs dict of
    instance i's scene (the same dict object for instances of one scene)."""
    n = len(rays)
    res = np.zeros(n, synth.RESULT_DTYPE)
    res["triangle"] = MISS
    inst = np.full(n, NO_INSTANCE, np.uint32)
    best = np.full(n, np.inf, np.float32)
    found = np.zeros(n, bool)
    hits = np.zeros((len(blobs_per_instance), n), bool)
    ok = valid_rays(rays)
    for i, blobs in enumerate(blobs_per_instance):
        h = orc.traverse(blobs, object_rays(inv[i], rays), threads=threads)
        hit = (h["triangle"] != MISS) & ok
        hits[i] = hit
        better = hit & (~found | (h["t"] < best))      # strict: an exact tie stays with the lower index
        res[better] = h[better]
        inst[better] = i
        best[better] = h["t"][better]
        found |= hit
    return res, inst, hits


def assert_world_exact(got, got_inst, want, want_inst, what=""):
    """Bit-exact on triangle, t, u, v and the instance index, misses included (triangle = MISS, t = u = v = 0, instance = NO_INSTANCE)."""
    assert got.dtype == want.dtype == synth.RESULT_DTYPE and got_inst.dtype == np.uint32
    bad = np.nonzero(got_inst != want_inst)[0]
    assert len(bad) == 0, "%s: instance index differs at %d rays, e.g. %s: got %s want %s" % (what, len(bad), bad[:8], got_inst[bad[:8]], want_inst[bad[:8]])
    for f in ("triangle", "t", "u", "v"):
        g, w = got[f].view(np.uint32), want[f].view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %s not bit-exact at %d rays, e.g. %s: got %r want %r" % (what, f, len(bad), bad[:8], got[f][bad[:8]], want[f][bad[:8]])
    miss = want["triangle"] == MISS
    assert (want_inst[miss] == NO_INSTANCE).all() and (want["t"][miss] == 0).all()


_fmaf = None


def _fmaf_elementwise():
    """libm's fmaf as a numpy ufunc (numpy has no fused multiply-add), loaded on first use."""
    global _fmaf
    if _fmaf is None:
        libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.fmaf.argtypes, libm.fmaf.restype = [C.c_float, C.c_float, C.c_float], C.c_float
        _fmaf = np.frompyfunc(lambda a, b, c: libm.fmaf(float(a), float(b), float(c)), 3, 1)
    return _fmaf


def top_level_enters(prep, rays):
    """The top-level rule of the world kernels for a ONE-instance world, in binary32 (racc_world.inc: setWorldRay, worldWidenedEnd,
    worldTopInnerStep over slabPair): does the ray enter the instance's padded world box in [minT, maxT widened by 2^-20 of itself]?
    `prep` = host_world_prepare's output.  The world box is padded by ray_pad (|ox| + |oy| + |oz|) on every side; 1 / d is that of the
    clamped direction; min / max ignore a NaN; the interval's end doubles as "missed" (so an entry distance equal to it — +inf under
    maxT = +inf — reads as missed).  While nothing overflows the box is conservative and every ray that can hit the instance enters it
    (world_build.cpp); this function is for the ends of the float range, where the products overflow.  It is a MODEL OF THE KERNEL's
    rule, not an independent reference: what makes it usable is that inside the domain it is asserted to remove no hit
    (tests/test_float_range.py), so there the expectation is the plain composition.  -> bool [N]."""
    nodes = prep["nodes"]
    assert len(nodes) == 1 and nodes["first"][0] == (1 << 24) and nodes["last"][0] == 0, "a one-instance world: one top-level node, the instance on the left, nothing on the right"
    f = np.float32
    with np.errstate(all="ignore"):
        o, d = rays["origin"].astype(f), rays["dir"].astype(f).copy()
        small = np.abs(d) < f(1e-10)
        d[small] = np.copysign(f(1e-10), d[small])
        inv = f(1.0) / d
        e = -o * inv
        pad = f(prep["ray_pad"]) * ((np.abs(o[:, 0]) + np.abs(o[:, 1])) + np.abs(o[:, 2]))
        t = rays["maxT"].astype(f)
        end = t + np.fmax(np.abs(t) * f(9.5367431640625e-07), f(1e-30))
        lo = nodes["leftMin"][0][None, :] - pad[:, None]
        hi = nodes["leftMax"][0][None, :] + pad[:, None]
        fmaf = _fmaf_elementwise()
        a, b = fmaf(lo, inv, e).astype(f), fmaf(hi, inv, e).astype(f)
        near = np.fmax(np.fmax(rays["minT"].astype(f), np.fmin(a[:, 0], b[:, 0])), np.fmax(np.fmin(a[:, 1], b[:, 1]), np.fmin(a[:, 2], b[:, 2])))
        far = np.fmin(np.fmin(end, np.fmax(a[:, 0], b[:, 0])), np.fmin(np.fmax(a[:, 1], b[:, 1]), np.fmax(a[:, 2], b[:, 2])))
        entry = np.where(near > far, end, near)
        return entry != end
