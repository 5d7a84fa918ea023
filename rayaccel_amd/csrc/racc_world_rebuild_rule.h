// racc_world_rebuild_rule.h — the rule of the top-level LBVH, stated once: racc_world_rule.h's sibling.  Compiled for the host by
// world_build.cpp (racc_host_world_rebuild, the specification) and for the device by racc_world_rebuild.inc (racc_hip_world_rebuild*): the
// same expressions in the same order, in double where a rounding could differ, nothing contracted (-ffp-contract=off on both sides), so
// the two agree bit for bit.  What is here is what is evaluated per instance or per pair of keys; the hierarchy over the sorted keys is
// stated in words below and formulated twice — top-down on the host, by Karras's per-node searches on the device ("Maximizing
// Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012) — because that is the point of having a specification.
//
//  1. Per instance: inv, world box and condition number by racc_world_rule::instance, unchanged.
//  2. Centre, per axis: c = float(0.5 * double(min) + 0.5 * double(max)) of the world box — never 0.5 * (min + max), which overflows.
//  3. Bounds: lo / hi per axis = the smallest / largest centre coordinate of the ENABLED instances (the host function has no others).
//     A minimum and a maximum are exact, so they do not depend on the order of a reduction; -0.0 and +0.0 may stand for each other,
//     everything below uses lo and hi only as numbers.
//  4. Morton field: per axis q = quantise(c, lo, hi) below, 10 bits; field = x, y, z interleaved into 30 bits with x highest (bit 3k + 2
//     = bit k of qx, bit 3k + 1 = bit k of qy, bit 3k = bit k of qz).  A disabled instance (device only) has the field kDisabledField =
//     2^30: behind every enabled one.
//  5. Key = (uint64(field) << 32) | instance index.  Keys are unique, so their sorted order is one order; order[p] = the low word of
//     the p-th smallest key.
//  6. Hierarchy over the sorted keys (positions 0 .. count - 1): the root covers [0, count - 1] and is record 0.  A node covering [a, b],
//     a < b, splits at s = the last position of [a, b) whose key shares with key[a] more leading bits than key[b] does — the last one
//     with a 0 in the highest bit in which key[a] and key[b] differ.  First child = [a, s], last child = [s + 1, b].  A child of one
//     position p is the leaf reference p | 1 << 24; a wider first child is record s, a wider last child record s + 1 (Karras's
//     numbering: a record's index is the end of its range that touches its sibling), referenced as 0x80000000 | record.
//     max(count - 1, 1) records.  count == 1: record 0 = {leaf 0, the empty reference 0}, as racc_host_world_prepare makes it.
//  7. Boxes and ray_pad: the fold of racc_host_world_refit over this topology (accumulator = first child, select not fmin).
//  8. Height (levels of records on the longest root path) <= heightBound(count, disabledPossible):
//     a record's split bit — the highest bit in which the two ends of its range differ — is strictly lower than its parent's, since both
//     ends of a child's range agree in the parent's split bit and above.  So a root path has at most one record per bit that can differ
//     between two keys.  Those are: the low ceil(log2(count)) bits of the index (indices are below count <= 2^20 =
//     RACC_HIP_WORLD_MAX_INSTANCES), the 30 bits of the Morton field, and — only where instances can be disabled, which the host function
//     refuses — the one bit of kDisabledField.  30 + ceil(log2(count)) on the host, one more on the device; and never more than the
//     count - 1 records there are (1 for count == 1).
#pragma once

#include <cstdint>

#include "racc_world_rule.h"

namespace racc_world_rebuild_rule {

constexpr uint32_t kAxisBits = 10;
constexpr uint32_t kFieldBits = 3 * kAxisBits;
constexpr uint32_t kDisabledField = 1u << kFieldBits;
constexpr uint32_t kKeyLowBit = 32, kKeyEndBit = 32 + kFieldBits + 1;      // where the field sits in a key: what a sort has to look at

RACC_RULE_FN float centre(float mn, float mx) { return float(0.5 * double(mn) + 0.5 * double(mx)); }

// One axis: floor(1024 (c - lo) / (hi - lo)) in double, at most 1023; 0 on an axis without extent.
RACC_RULE_FN uint32_t quantise(float c, float lo, float hi) {
    if (!(hi > lo)) return 0u;
    const double q = (double(c) - double(lo)) / (double(hi) - double(lo)) * 1024.0;
    return q >= 1023.0 ? 1023u : (q > 0.0 ? uint32_t(q) : 0u);
}

// 10 bits -> every third bit
RACC_RULE_FN uint32_t spread3(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

RACC_RULE_FN uint32_t field(const float c[3], const float lo[3], const float hi[3]) {
    return (spread3(quantise(c[0], lo[0], hi[0])) << 2) | (spread3(quantise(c[1], lo[1], hi[1])) << 1) | spread3(quantise(c[2], lo[2], hi[2]));
}

RACC_RULE_FN uint64_t key(uint32_t fieldValue, uint32_t index) { return (uint64_t(fieldValue) << 32) | index; }

// Leading bits two DIFFERENT keys share.
RACC_RULE_FN int commonPrefix(uint64_t a, uint64_t b) { return __builtin_clzll(a ^ b); }

RACC_RULE_FN uint32_t ceilLog2(uint32_t n) { uint32_t l = 0; while ((1ull << l) < n) ++l; return l; }

// Rule 8.
RACC_RULE_FN uint32_t heightBound(uint32_t count, bool disabledPossible) {
    const uint32_t byBits = kFieldBits + (disabledPossible ? 1u : 0u) + ceilLog2(count);
    const uint32_t byRecords = count > 1u ? count - 1u : 1u;
    return byBits < byRecords ? byBits : byRecords;
}

}  // namespace racc_world_rebuild_rule
