// scene_refit.cpp — host refit of reference-format scene blobs to moved vertices (racc_host_blobs_refit, include/racc_hip.h).
//
// No counterpart in the reference (its scenes are frozen at createScene, Scene.cpp:216-349); Embree's rtcCommitScene on a deformable
// scene is the usual one.  The topology stays — child references, leaf ranges, remap — and only what depends on vertex positions is
// recomputed: the 48 B pair records (packPair's three subtractions, Scene.cpp:149-153) and the child boxes of the 64 B node records.
// This file is the SPECIFICATION of the rule; the device refit (racc_refit.inc) reproduces it bit for bit:
//   pair p      remap[2p] = t0 | ea << 30, remap[2p+1] = t1 | (eb+1) << 30 or 0 for a lone triangle (then p3 = p1); with a / b the index
//               triples of t0 / t1 the vertices are a[ea], a[(ea+1)%3], a[(ea+2)%3], b[(eb+2)%3] — exactly what flatten() packed
//               (scene_build.cpp); padding records [pair_count, pair_count_padded) are copies of the new pair 0 (Scene.cpp:334-338)
//   select      min = b < acc ? b : acc, max = b > acc ? b : acc per component — never fmin/fmax, whose answer for -0.0 against +0.0
//               differs between host and device
//   leaf box    that select folded over the leaf's pairs first .. first+cnt-1 and each pair's vertices p0, p1, p2, p3, the
//               accumulator starting from p0 of the first pair
//   inner box   the node's first-child box (accumulator) with its last-child box, by the same select
// Everything is validated before the first output byte is written, so the outputs may alias the inputs.
#include "racc_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

extern "C" void racc_hip_set_error_(const char* msg);

namespace {

struct Node64 { uint32_t kind, parent, first, last; float box[12]; };      // leftMin[3], leftMax[3], rightMin[3], rightMax[3] (Scene.cpp:73-78)
struct Pair48 { float e1[3], e3x, e2[3], e3y, p0[3], e3z; };               // Scene.cpp:83-87
static_assert(sizeof(Node64) == 64 && sizeof(Pair48) == 48, "reference record sizes");

int refuse(const char* what) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "racc_host_blobs_refit: %s", what);
    racc_hip_set_error_(msg);
    return RACC_HIP_ERR_INVALID;
}

inline void foldPoint(float* mn, float* mx, const float* p) {
    for (int k = 0; k < 3; ++k) {
        mn[k] = p[k] < mn[k] ? p[k] : mn[k];
        mx[k] = p[k] > mx[k] ? p[k] : mx[k];
    }
}

}  // namespace

extern "C" int racc_host_blobs_refit(const void* nodes64, uint32_t node_count,
                                     const void* pairs48, uint32_t pair_count_padded, uint32_t pair_count,
                                     const uint32_t* remap, uint32_t remap_count,
                                     const float* vertices, uint32_t vertex_count,
                                     const uint32_t* indices, uint32_t index_count,
                                     void* nodes64_out, void* pairs48_out) {
    if (!nodes64 || !pairs48 || !remap) return refuse("scene blob pointer is NULL");
    if (!vertices || !indices || !nodes64_out || !pairs48_out) return refuse("vertices / indices / output pointer is NULL");
    if (!node_count) return refuse("scene has no inner node");
    if (node_count > (1u << 26) || pair_count_padded > (1u << 24)) return refuse("node/pair count exceeds the reference format (Scene.cpp:294-312)");
    if (!pair_count || pair_count > pair_count_padded) return refuse("pair_count must lie in [1, pair_count_padded]");
    if (uint64_t(pair_count) * 2 > remap_count) return refuse("remap shorter than the pairs it indexes");
    if (index_count % 3 != 0) return refuse("index_count is not a multiple of 3 (Scene.cpp:186)");
    const Node64* in = static_cast<const Node64*>(nodes64);
    const uint32_t triCount = index_count / 3;

    // the tree: validateScene's rules (racc_scene_format.inc), and on the way the nodes in an order in which a parent precedes its children
    std::vector<uint32_t> order;
    order.reserve(node_count);
    {
        std::vector<uint8_t> seen(node_count, 0);
        order.push_back(0u);
        seen[0] = 1;
        for (size_t head = 0; head < order.size(); ++head) {
            const uint32_t kids[2] = { in[order[head]].first, in[order[head]].last };
            for (uint32_t c : kids) {
                if (c & 0x80000000u) {
                    const uint32_t ci = c & 0x7FFFFFFFu;
                    if (ci >= node_count) return refuse("scene blob: child index out of range");
                    if (seen[ci]) return refuse("scene blob: inner node referenced twice (not a tree)");
                    seen[ci] = 1;
                    order.push_back(ci);
                } else {
                    const uint32_t first = c & 0xFFFFFFu, cnt = c >> 24;
                    if (cnt == 0) return refuse("scene blob: leaf with zero pairs");
                    if (first + cnt > pair_count) return refuse("scene blob: leaf pair range out of bounds");
                }
            }
        }
    }
    // the four vertex indices of every pair
    std::vector<uint32_t> quad(size_t(pair_count) * 4);
    for (uint32_t p = 0; p < pair_count; ++p) {
        const uint32_t r0 = remap[2 * size_t(p)], r1 = remap[2 * size_t(p) + 1];
        const uint32_t t0 = r0 & 0x3FFFFFFFu, ea = r0 >> 30;
        if (t0 >= triCount || ea > 2u) return refuse("remap names a triangle beyond index_count / 3 (or an edge code beyond 2)");
        const uint32_t* a = indices + size_t(t0) * 3;
        uint32_t* q = &quad[size_t(p) * 4];
        q[0] = a[ea]; q[1] = a[(ea + 1) % 3]; q[2] = a[(ea + 2) % 3];
        if (r1 == 0u) q[3] = q[1];                                          // lone triangle: p3 = p1 (Scene.cpp:160-180)
        else {
            const uint32_t t1 = r1 & 0x3FFFFFFFu, eb = (r1 >> 30) - 1u;
            if (t1 >= triCount || (r1 >> 30) == 0u) return refuse("remap names a triangle beyond index_count / 3 (or a second triangle without its edge code)");
            q[3] = indices[size_t(t1) * 3 + (eb + 2) % 3];
        }
    }
    for (uint32_t i = 0; i < index_count; ++i)
        if (indices[i] >= vertex_count) return refuse("an index is not below vertex_count");
    for (size_t i = 0; i < size_t(vertex_count); ++i)
        if (!std::isfinite(vertices[i * 4]) || !std::isfinite(vertices[i * 4 + 1]) || !std::isfinite(vertices[i * 4 + 2])) return refuse("a vertex coordinate is not finite");

    // ---- nothing can fail from here on (but the allocations): results are built apart and copied out at the end (in and out may alias) ----
    std::vector<Pair48> pairs;
    std::vector<Node64> nodes;
    try {
        pairs.resize(pair_count_padded);
        nodes.assign(in, in + node_count);                                 // kind, parent, first, last (and nodes the root does not reach) unchanged
    } catch (const std::bad_alloc&) { racc_hip_set_error_("racc_host_blobs_refit: out of host memory"); return RACC_HIP_ERR_NOMEM; }
    for (uint32_t p = 0; p < pair_count; ++p) {                            // packPair (scene_build.cpp; Scene.cpp:149-153)
        const uint32_t* q = &quad[size_t(p) * 4];
        const float *p0 = vertices + size_t(q[0]) * 4, *p1 = vertices + size_t(q[1]) * 4, *p2 = vertices + size_t(q[2]) * 4, *p3 = vertices + size_t(q[3]) * 4;
        Pair48& r = pairs[p];
        for (int k = 0; k < 3; ++k) { r.e1[k] = p0[k] - p1[k]; r.e2[k] = p2[k] - p0[k]; r.p0[k] = p0[k]; }
        r.e3x = p3[0] - p0[0]; r.e3y = p3[1] - p0[1]; r.e3z = p3[2] - p0[2];
    }
    for (uint32_t p = pair_count; p < pair_count_padded; ++p) pairs[p] = pairs[0];
    for (size_t i = order.size(); i-- > 0;) {                              // children before their parents
        Node64& n = nodes[order[i]];
        const uint32_t kids[2] = { n.first, n.last };
        for (int side = 0; side < 2; ++side) {
            float* mn = n.box + side * 6;
            float* mx = mn + 3;
            const uint32_t c = kids[side];
            if (c & 0x80000000u) {
                const float* cb = nodes[c & 0x7FFFFFFFu].box;              // its boxes are final: it comes behind this node in `order`
                for (int k = 0; k < 3; ++k) {
                    mn[k] = cb[6 + k] < cb[k] ? cb[6 + k] : cb[k];
                    mx[k] = cb[9 + k] > cb[3 + k] ? cb[9 + k] : cb[3 + k];
                }
            } else {
                const uint32_t first = c & 0xFFFFFFu, cnt = c >> 24;
                const float* start = vertices + size_t(quad[size_t(first) * 4]) * 4;
                for (int k = 0; k < 3; ++k) mn[k] = mx[k] = start[k];
                for (uint32_t p = first; p < first + cnt; ++p)
                    for (int v = 0; v < 4; ++v) foldPoint(mn, mx, vertices + size_t(quad[size_t(p) * 4 + v]) * 4);
            }
        }
    }
    std::memcpy(nodes64_out, nodes.data(), size_t(node_count) * sizeof(Node64));
    std::memcpy(pairs48_out, pairs.data(), size_t(pair_count_padded) * sizeof(Pair48));
    return RACC_HIP_OK;
}
