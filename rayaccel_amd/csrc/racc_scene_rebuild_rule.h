// racc_scene_rebuild_rule.h — the rule of the bottom-level LBVH (an LBVH over the triangles of a mesh, in the scene formats every kernel
// reads), stated once: racc_world_rebuild_rule.h's sibling.  Compiled for the host by scene_rebuild.cpp (racc_host_scene_rebuild, the
// specification) and for the device by racc_scene_rebuild.inc (racc_hip_scene_rebuild*): the same expressions in the same order, in double
// where a rounding could differ, nothing contracted (-ffp-contract=off on both sides), so the two agree bit for bit.  The hierarchy over the
// sorted keys is formulated twice — top-down on the host, by Karras's per-node searches here (hierarchyStep: "Maximizing Parallelism in the
// Construction of BVHs, Octrees, and k-d Trees", HPG 2012), which the device kernel and the sanitised CPU driver
// (tests/cpp/scene_rebuild_host_check.cpp) both run.
//
//  1. Triangle box: the select of racc_host_blobs_refit (min = b < acc ? b : acc, max = b > acc ? b : acc) folded over the triangle's three
//     vertices in index order, the accumulator starting from the first vertex.
//  2. Centre, per axis: c = float(0.5 * double(min) + 0.5 * double(max)) of that box — never 0.5 * (min + max), which overflows.
//  3. Bounds: lo / hi per axis = the smallest / largest centre coordinate.  A minimum and a maximum are exact, so they do not depend on
//     the order of a reduction; -0.0 and +0.0 may stand for each other, everything below uses lo and hi only as numbers.
//  4. Morton field: per axis q = quantise(c, lo, hi) below, 21 bits — floor(2^21 (c - lo) / (hi - lo)) in double, at most 2^21 - 1, 0 where
//     hi > lo does not hold and 0 where the quotient is not a number in range; a value in [0, 2^21) for ANY input bits, NaN and infinities
//     included.  field = x, y, z interleaved into 63 bits with x highest (bit 3k + 2 = bit k of qx, 3k + 1 of qy, 3k of qz).
//  5. Key = the pair (field, triangle index), ordered lexicographically: a 95-bit number, field above index.  Keys are unique, so their
//     sorted order is one order; order[p] = the triangle of the p-th smallest key.
//  6. Pairs: pair p is triangle order[p] alone — remap[2p] = t, remap[2p + 1] = 0, its vertices a[0], a[1], a[2], a[1] of the triangle's
//     index triple a, the record what refitPairsKernel / racc_host_blobs_refit pack from them.  paddedPairs(T) records (the smallest
//     multiple of 32 above T, scene_build.cpp's rule), the padding copies of pair 0.  remap_count = 2T.
//  7. Hierarchy over the sorted keys (positions 0 .. T - 1): node 0 is the root over [0, T - 1].  A node over [a, b], a < b, splits behind
//     s = the last position of [a, b) with a 0 in the highest bit in which key[a] and key[b] differ.  First child = [a, s], last child =
//     [s + 1, b].  A child of one position p is the leaf p | 1 << 24; a wider first child is node s, a wider last child node s + 1
//     (Karras's numbering), referenced as 0x80000000 | node.  kind = 1, parent = the parent's index (0xFFFFFFFF for the root).  T - 1 nodes.
//  8. Boxes: racc_host_blobs_refit's fold over this topology (leaf = the triangle's box, inner = first child's box as accumulator with the
//     last child's), so refitting the output to its own vertices reproduces it, signs of zeros included.
//  9. Height (levels of nodes on the longest root path) <= heightBound(T): a node's split bit — the highest bit in which the two ends of
//     its range differ — is strictly lower than its parent's, since both ends of a child's range agree in the parent's split bit and
//     above.  So a root path has at most one node per bit that can differ between two keys: the 63 bits of the field and the low
//     ceil(log2(T)) bits of the index (indices are below T).  63 + ceil(log2(T)), at most 87 (T < 2^24); and never more than the T - 1
//     nodes there are.
#pragma once

#include <cstdint>

#include "racc_world_rule.h"      // RACC_RULE_FN

namespace racc_scene_rebuild_rule {

constexpr uint32_t kAxisBits = 21;
constexpr uint32_t kFieldBits = 3 * kAxisBits;      // what a sort has to look at: bits [0, 63) of the field
constexpr uint32_t kMaxTriangles = 1u << 24;        // a leaf reference holds a 24-bit position

RACC_RULE_FN float foldMin(float acc, float b) { return b < acc ? b : acc; }
RACC_RULE_FN float foldMax(float acc, float b) { return b > acc ? b : acc; }

RACC_RULE_FN float centre(float mn, float mx) { return float(0.5 * double(mn) + 0.5 * double(mx)); }

// Rules 1-2 for one triangle: v0, v1, v2 point at x, y, z.
RACC_RULE_FN void triangleCentre(const float* v0, const float* v1, const float* v2, float c[3]) {
    for (int k = 0; k < 3; ++k) {
        float mn = v0[k], mx = v0[k];
        mn = foldMin(mn, v1[k]); mx = foldMax(mx, v1[k]);
        mn = foldMin(mn, v2[k]); mx = foldMax(mx, v2[k]);
        c[k] = centre(mn, mx);
    }
}

// One axis.  Every comparison with a NaN is false, so whatever the three floats hold the result is one of the three returns below.
RACC_RULE_FN uint32_t quantise(float c, float lo, float hi) {
    if (!(hi > lo)) return 0u;
    const double q = (double(c) - double(lo)) / (double(hi) - double(lo)) * 2097152.0;
    return q >= 2097151.0 ? 2097151u : (q > 0.0 ? uint32_t(q) : 0u);
}

// 21 bits -> every third bit
RACC_RULE_FN uint64_t spread3(uint32_t q) {
    uint64_t v = q & 0x1FFFFFu;
    v = (v | (v << 32)) & 0x001F00000000FFFFull;
    v = (v | (v << 16)) & 0x001F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

RACC_RULE_FN uint64_t field(const float c[3], const float lo[3], const float hi[3]) {
    return (spread3(quantise(c[0], lo[0], hi[0])) << 2) | (spread3(quantise(c[1], lo[1], hi[1])) << 1) | spread3(quantise(c[2], lo[2], hi[2]));
}

// Leading bits of the 95-bit keys (fa, ia) and (fb, ib) that agree: 95 for equal keys (which a sorted array of keys never holds).
RACC_RULE_FN int commonPrefix(uint64_t fa, uint32_t ia, uint64_t fb, uint32_t ib) {
    const uint64_t x = (fa ^ fb) & 0x7FFFFFFFFFFFFFFFull;
    if (x) return __builtin_clzll(x) - 1;
    const uint32_t y = ia ^ ib;
    return 63 + (y ? __builtin_clz(y) : 32);
}

RACC_RULE_FN uint32_t ceilLog2(uint32_t n) { uint32_t l = 0; while ((1ull << l) < n) ++l; return l; }

// Rule 9.
RACC_RULE_FN uint32_t heightBound(uint32_t triangles) {
    const uint32_t byBits = kFieldBits + ceilLog2(triangles);
    const uint32_t byNodes = triangles > 1u ? triangles - 1u : 1u;
    return byBits < byNodes ? byBits : byNodes;
}

// Rule 6.
RACC_RULE_FN uint32_t paddedPairs(uint32_t triangles) { return (triangles / 32u + 1u) * 32u; }

// Rule 7 for node `i` of `n` >= 2 sorted keys, i in [0, n - 2]: Karras's searches.  `fields[p]`, `indices[p]` = the key at position p.
// word[side] is the child reference of the record; a leaf child is position target[side], whose slot is 2 * i + side; an inner child is
// node target[side], whose parent slot is 2 * i + side.
// In bounds whatever the keys hold (unsorted garbage included): delta is -1 for a position outside [0, n), so no search accepts one and
// every position read lies in [0, n); the split is clamped to [0, n - 2], so target[] lies in [0, n - 1] — tables of n entries hold every
// index this function names.  (On sorted unique keys the clamp changes nothing and an inner target lies in [1, n - 2].)
struct HierarchyStep { uint32_t word[2]; uint32_t target[2]; bool leaf[2]; };

template <class Fields, class Indices>
RACC_RULE_FN HierarchyStep hierarchyStep(const Fields& fields, const Indices& indices, int n, int i) {
    const uint64_t fi = fields[i];
    const uint32_t ii = indices[i];
    auto delta = [&](int j) -> int { return (j < 0 || j >= n) ? -1 : commonPrefix(fi, ii, fields[j], indices[j]); };
    // the direction of the range and a bound of its length
    const int d = delta(i + 1) > delta(i - 1) ? 1 : -1;
    const int deltaMin = delta(i - d);
    int lMax = 2;
    while (lMax < (1 << 26) && delta(i + lMax * d) > deltaMin) lMax <<= 1;      // (n <= 2^24: the first condition never decides)
    // the other end, by binary search
    int l = 0;
    for (int t = lMax >> 1; t >= 1; t >>= 1)
        if (delta(i + (l + t) * d) > deltaMin) l += t;
    const int j = i + l * d;
    // the split: the last position, seen from i, that shares more than the range's common prefix with key[i]
    const int deltaNode = delta(j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(i + (s + t) * d) > deltaNode) s += t;
    } while (t > 1);
    int split = i + s * d + (d < 0 ? -1 : 0);      // first child [a, split], last child [split + 1, b]
    split = split < 0 ? 0 : (split > n - 2 ? n - 2 : split);
    const int a = d > 0 ? i : j, b = d > 0 ? j : i;
    HierarchyStep r;
    r.leaf[0] = a == split;
    r.target[0] = uint32_t(split);
    r.word[0] = (r.leaf[0] ? (1u << 24) : 0x80000000u) | uint32_t(split);
    r.leaf[1] = b == split + 1;
    r.target[1] = uint32_t(split + 1);
    r.word[1] = (r.leaf[1] ? (1u << 24) : 0x80000000u) | uint32_t(split + 1);
    return r;
}

}  // namespace racc_scene_rebuild_rule
