// world_build.cpp — host side of instancing (racc_host_world_prepare, include/racc_hip.h): per-instance inverse transforms, conservative
// world-space boxes and the top-level BVH2 over them.  No GPU code.
//
// No counterpart in the reference (one flattened scene per racc::Scene, Scene.cpp:216-349); the two-level structure of Embree's
// RTC_GEOMETRY_TYPE_INSTANCE and of every GPU ray-tracing API is the usual one.
//
// inv (part of the specification, include/racc_hip.h): the inverse of the 3x4 object-to-world transform evaluated in double — adjugate of
// the 3x3 part over its determinant, translation = -(A^-1 b) — each of the twelve coefficients rounded to float once.
//
// World boxes.  The kernel culls an instance whose box a ray misses, and a cull must never lose a hit the object-space traversal would
// report.  That traversal works on o' = fl(inv (o, 1)), d' = fl(inv (d, 0)); a point o' + t d' of the instance's root box maps to the world
// point A (o' + t d') + b, which differs from o + t d by at most
//     g cond (2 |o| + |b| + |W|),   cond = |A|_inf |A^-1|_inf, |W| = the largest coordinate of the exact world box, g ~ 5 ulp/2
// (one rounding of every inv coefficient plus the four of each transformed component, carried back through |A|).  The instance's part,
// K cond_i (|b_i| + |W_i|) with K = 2^-20 (16 units of 2^-24: three times g, which also covers the rounding of the slab test and of the
// object-space tests at the box's surface), is added to the box here and the box rounded outwards; the ray's part, ray_pad (|ox| + |oy| +
// |oz|) with ray_pad = 2 K max_i cond_i, is added by the kernel to every box it tests (racc_world.inc).
//
// Top level: BVH2 in the scenes' 64-byte node format (Scene.cpp:73-78), one instance per leaf, leaf reference = position in `order` |
// 1 << 24.  Median split of the box centres along the longest axis of their bounds, ties by instance index: deterministic.  A world of
// one instance has a root whose last child is the empty reference 0 (count 0; the kernel never enters it).
#include "racc_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

extern "C" void racc_hip_set_error_(const char* msg);

namespace {

struct Node64 { uint32_t kind, parent, first, last; float box[12]; };      // leftMin[3], leftMax[3], rightMin[3], rightMax[3]
static_assert(sizeof(Node64) == 64, "reference record size");

int refuse(int code, const char* what, long long at = -1) {
    char msg[256];
    if (at >= 0) std::snprintf(msg, sizeof(msg), "racc_host_world_prepare: %s (instance %lld)", what, at);
    else std::snprintf(msg, sizeof(msg), "racc_host_world_prepare: %s", what);
    racc_hip_set_error_(msg);
    return code;
}

inline float roundDown(double x) { const float f = float(x); return double(f) > x ? std::nextafterf(f, -INFINITY) : f; }
inline float roundUp(double x) { const float f = float(x); return double(f) < x ? std::nextafterf(f, INFINITY) : f; }

struct Builder {
    const float* boxes;                 // [count][6] min, max
    std::vector<float> centre;          // [count][3]
    std::vector<uint32_t>& order;
    std::vector<Node64>& nodes;
    uint32_t height = 0;

    void bounds(uint32_t first, uint32_t last, float* out6) const {
        for (int k = 0; k < 3; ++k) { out6[k] = boxes[size_t(order[first]) * 6 + k]; out6[3 + k] = boxes[size_t(order[first]) * 6 + 3 + k]; }
        for (uint32_t i = first + 1; i < last; ++i) {
            const float* b = boxes + size_t(order[i]) * 6;
            for (int k = 0; k < 3; ++k) { out6[k] = b[k] < out6[k] ? b[k] : out6[k]; out6[3 + k] = b[3 + k] > out6[3 + k] ? b[3 + k] : out6[3 + k]; }
        }
    }

    // builds the inner node over order[first, last) (at least two instances) and returns its index
    uint32_t build(uint32_t first, uint32_t last, uint32_t parent, uint32_t depth) {
        const uint32_t self = uint32_t(nodes.size());
        nodes.emplace_back();
        if (depth > height) height = depth;
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = centre[size_t(order[first]) * 3 + k];
        for (uint32_t i = first + 1; i < last; ++i)
            for (int k = 0; k < 3; ++k) {
                const float c = centre[size_t(order[i]) * 3 + k];
                lo[k] = c < lo[k] ? c : lo[k]; hi[k] = c > hi[k] ? c : hi[k];
            }
        int axis = 0;
        if (hi[1] - lo[1] > hi[axis] - lo[axis]) axis = 1;
        if (hi[2] - lo[2] > hi[axis] - lo[axis]) axis = 2;
        const uint32_t mid = first + (last - first) / 2;
        std::sort(order.begin() + first, order.begin() + last, [&](uint32_t a, uint32_t b) {
            const float ca = centre[size_t(a) * 3 + axis], cb = centre[size_t(b) * 3 + axis];
            return ca < cb || (ca == cb && a < b);
        });
        float box[12];
        bounds(first, mid, box);
        bounds(mid, last, box + 6);
        const uint32_t l = mid - first == 1 ? ((1u << 24) | first) : (0x80000000u | build(first, mid, self, depth + 1));
        const uint32_t r = last - mid == 1 ? ((1u << 24) | mid) : (0x80000000u | build(mid, last, self, depth + 1));
        Node64& n = nodes[self];
        n.kind = uint32_t(axis) + 1u; n.parent = parent; n.first = l; n.last = r;
        std::memcpy(n.box, box, sizeof(box));
        return self;
    }
};

}  // namespace

extern "C" int racc_host_world_prepare(const float* transforms12, const float* root_boxes6, uint32_t count,
                                       float* inv12_out, float* world_boxes6_out, float* ray_pad_out,
                                       void* nodes64_out, uint32_t node_capacity, uint32_t* node_count_out,
                                       uint32_t* order_out, uint32_t* height_out) try {
    if (!transforms12 || !root_boxes6) return refuse(RACC_HIP_ERR_INVALID, "transforms / root boxes pointer is NULL");
    if (!inv12_out || !world_boxes6_out || !ray_pad_out || !nodes64_out || !node_count_out || !order_out || !height_out) return refuse(RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    if (!count) return refuse(RACC_HIP_ERR_INVALID, "count is 0: a world has at least one instance");
    if (count > RACC_HIP_WORLD_MAX_INSTANCES) return refuse(RACC_HIP_ERR_INVALID, "more than 2^20 instances");
    const uint32_t nodesNeeded = count > 1u ? count - 1u : 1u;
    if (node_capacity < nodesNeeded) return refuse(RACC_HIP_ERR_INVALID, "node_capacity is below max(count - 1, 1)");

    // everything is validated and computed into buffers of our own before the first output byte is written
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6);
    const double K = 1.0 / 1048576.0;      // 2^-20, see the head of this file
    double maxCond = 0.0;
    for (uint32_t i = 0; i < count; ++i) {
        const float* m = transforms12 + size_t(i) * 12;
        const float* rb = root_boxes6 + size_t(i) * 6;
        for (int k = 0; k < 12; ++k) if (!std::isfinite(m[k])) return refuse(RACC_HIP_ERR_INVALID, "a transform coefficient is not finite", i);
        for (int k = 0; k < 6; ++k) if (!std::isfinite(rb[k])) return refuse(RACC_HIP_ERR_INVALID, "a root box coordinate is not finite", i);
        for (int k = 0; k < 3; ++k) if (rb[k] > rb[3 + k]) return refuse(RACC_HIP_ERR_INVALID, "a root box has min > max", i);
        const double a[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } };
        const double b[3] = { m[3], m[7], m[11] };
        double c[3][3];      // cofactors: c[r][k] = cofactor of a[r][k]
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {
                const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
                c[r][k] = a[r1][k1] * a[r2][k2] - a[r1][k2] * a[r2][k1];
            }
        const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
        if (det == 0.0 || !std::isfinite(det)) return refuse(RACC_HIP_ERR_INVALID, "a transform is singular (its double-precision determinant is zero or not finite)", i);
        double B[3][3], t[3], normA = 0.0, normB = 0.0, normb = 0.0;
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) B[r][k] = c[k][r] / det;      // adjugate = transposed cofactors
        for (int r = 0; r < 3; ++r) t[r] = -((B[r][0] * b[0] + B[r][1] * b[1]) + B[r][2] * b[2]);
        float* o = &inv[size_t(i) * 12];
        for (int r = 0; r < 3; ++r) {
            o[r * 4 + 0] = float(B[r][0]); o[r * 4 + 1] = float(B[r][1]); o[r * 4 + 2] = float(B[r][2]); o[r * 4 + 3] = float(t[r]);
            for (int k = 0; k < 4; ++k) if (!std::isfinite(o[r * 4 + k])) return refuse(RACC_HIP_ERR_INVALID, "a transform is singular in float (a coefficient of its inverse is not finite)", i);
            normA = std::max(normA, std::fabs(a[r][0]) + std::fabs(a[r][1]) + std::fabs(a[r][2]));
            normB = std::max(normB, std::fabs(B[r][0]) + std::fabs(B[r][1]) + std::fabs(B[r][2]));
            normb = std::max(normb, std::fabs(b[r]));
        }
        const double cond = normA * normB;
        maxCond = std::max(maxCond, cond);
        // the eight corners in double: per world axis the extremes are reached by picking min or max per object axis
        double lo[3], hi[3], mag = 0.0;
        for (int r = 0; r < 3; ++r) {
            lo[r] = hi[r] = b[r];
            for (int k = 0; k < 3; ++k) {
                const double p = a[r][k] * double(rb[k]), q = a[r][k] * double(rb[3 + k]);
                lo[r] += std::min(p, q); hi[r] += std::max(p, q);
            }
            mag = std::max(mag, std::max(std::fabs(lo[r]), std::fabs(hi[r])));
        }
        const double margin = K * cond * (normb + mag);
        float* w = &boxes[size_t(i) * 6];
        for (int r = 0; r < 3; ++r) {
            // (the sums above carry a few double roundings of their own: 2^-40 of the magnitudes, far inside the margin)
            w[r] = roundDown(lo[r] - margin); w[3 + r] = roundUp(hi[r] + margin);
            if (!std::isfinite(w[r]) || !std::isfinite(w[3 + r])) return refuse(RACC_HIP_ERR_INVALID, "a world-space box is not finite in float", i);
        }
    }
    const float rayPad = roundUp(2.0 * K * maxCond);
    if (!std::isfinite(rayPad)) return refuse(RACC_HIP_ERR_INVALID, "the transforms' condition numbers overflow float");

    std::vector<uint32_t> order(count);
    for (uint32_t i = 0; i < count; ++i) order[i] = i;
    std::vector<Node64> nodes;
    nodes.reserve(nodesNeeded);
    uint32_t height = 1;
    if (count == 1u) {
        Node64 n{};
        n.kind = 1u; n.parent = 0xFFFFFFFFu; n.first = (1u << 24) | 0u; n.last = 0u;
        std::memcpy(n.box, boxes.data(), 24);
        nodes.push_back(n);
    } else {
        Builder bl{ boxes.data(), std::vector<float>(size_t(count) * 3), order, nodes };
        for (uint32_t i = 0; i < count; ++i)
            for (int k = 0; k < 3; ++k) bl.centre[size_t(i) * 3 + k] = 0.5f * boxes[size_t(i) * 6 + k] + 0.5f * boxes[size_t(i) * 6 + 3 + k];
        bl.build(0u, count, 0xFFFFFFFFu, 1u);
        height = bl.height;
    }

    std::memcpy(inv12_out, inv.data(), inv.size() * sizeof(float));
    std::memcpy(world_boxes6_out, boxes.data(), boxes.size() * sizeof(float));
    *ray_pad_out = rayPad;
    std::memcpy(nodes64_out, nodes.data(), nodes.size() * sizeof(Node64));
    *node_count_out = uint32_t(nodes.size());
    std::memcpy(order_out, order.data(), order.size() * sizeof(uint32_t));
    *height_out = height;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return refuse(RACC_HIP_ERR_NOMEM, "out of host memory");
}
