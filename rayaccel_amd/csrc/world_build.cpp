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
//
// racc_host_world_rebuild builds the other top level: the LBVH of racc_world_rebuild_rule.h over the same inverses and world boxes — the
// specification of the rebuild on the device (racc_world_rebuild.inc), written top-down where the device searches per node.
#include "racc_hip.h"
#include "racc_world_rule.h"
#include "racc_world_rebuild_rule.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

extern "C" void racc_hip_set_error_(const char* msg);

namespace {

struct Node64 { uint32_t kind, parent, first, last; float box[12]; };      // leftMin[3], leftMax[3], rightMin[3], rightMax[3]
static_assert(sizeof(Node64) == 64, "reference record size");

const char* const kPrepare = "racc_host_world_prepare";
const char* const kRefit = "racc_host_world_refit";
const char* const kRebuild = "racc_host_world_rebuild";

// `who` = the entry the message names
int refuse(const char* who, int code, const char* what, long long at = -1) {
    char msg[256];
    if (at >= 0) std::snprintf(msg, sizeof(msg), "%s: %s (instance %lld)", who, what, at);
    else std::snprintf(msg, sizeof(msg), "%s: %s", who, what);
    racc_hip_set_error_(msg);
    return code;
}

// What every entry refuses about its inputs' shape, before anything is read.
int refuseShape(const char* who, const float* transforms12, const float* rootBoxes6, uint32_t count) {
    if (!transforms12 || !rootBoxes6) return refuse(who, RACC_HIP_ERR_INVALID, "transforms / root boxes pointer is NULL");
    if (!count) return refuse(who, RACC_HIP_ERR_INVALID, "count is 0: a world has at least one instance");
    if (count > RACC_HIP_WORLD_MAX_INSTANCES) return refuse(who, RACC_HIP_ERR_INVALID, "more than 2^20 instances");
    return RACC_HIP_OK;
}

// The per-instance part of racc_host_world_prepare and racc_host_world_refit (and what racc_hip_world_refit validates with): inverses,
// world boxes and the ray pad by racc_world_rule.h, into the caller's own buffers; a refusal names `who` and the instance.
int perInstance(const char* who, const float* transforms12, const float* rootBoxes6, uint32_t count, float* inv, float* boxes, float& rayPad) {
    namespace rule = racc_world_rule;
    static const char* const kWhy[] = {
        "",
        "a transform coefficient is not finite",
        "a root box coordinate is not finite",
        "a root box has min > max",
        "a transform is singular (its double-precision determinant is zero or not finite)",
        "a transform is singular in float (a coefficient of its inverse is not finite)",
        "a world-space box is not finite in float",
    };
    double maxCond = 0.0;
    for (uint32_t i = 0; i < count; ++i) {
        double cond = 0.0;
        const rule::Refusal why = rule::instance(transforms12 + size_t(i) * 12, rootBoxes6 + size_t(i) * 6, inv + size_t(i) * 12, boxes + size_t(i) * 6, cond);
        if (why != rule::kOk) return refuse(who, RACC_HIP_ERR_INVALID, kWhy[why], i);
        maxCond = std::max(maxCond, cond);
    }
    rayPad = rule::rayPadOf(maxCond);
    if (!std::isfinite(rayPad)) return refuse(who, RACC_HIP_ERR_INVALID, "the transforms' condition numbers overflow float");
    return RACC_HIP_OK;
}

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

// The hierarchy of racc_world_rebuild_rule.h (rule 6) over sorted keys, top-down: a range is split at the highest bit in which its two
// ends differ.  Boxes on the way back up, by racc_host_world_refit's fold (rule 7).
struct LbvhBuilder {
    const float* boxes;                 // [count][6] min, max
    const std::vector<uint64_t>& keys;  // sorted
    std::vector<Node64>& nodes;         // max(count - 1, 1) records, numbered as the rule says
    uint32_t height = 0;

    // the reference of the child covering [a, b], built if it is a record
    uint32_t child(uint32_t a, uint32_t b, uint32_t record, uint32_t parent, uint32_t depth, float* box) {
        if (a == b) {
            std::memcpy(box, boxes + size_t(uint32_t(keys[a])) * 6, 24);
            return (1u << 24) | a;
        }
        build(record, a, b, parent, depth);
        const float* acc = nodes[record].box;      // the child's first-child box (accumulator), then its last-child box
        const float* o = acc + 6;
        for (int k = 0; k < 3; ++k) { box[k] = o[k] < acc[k] ? o[k] : acc[k]; box[3 + k] = o[3 + k] > acc[3 + k] ? o[3 + k] : acc[3 + k]; }
        return 0x80000000u | record;
    }

    // record `self` over the positions [a, b], a < b
    void build(uint32_t self, uint32_t a, uint32_t b, uint32_t parent, uint32_t depth) {
        if (depth > height) height = depth;
        const int bit = 63 - racc_world_rebuild_rule::commonPrefix(keys[a], keys[b]);
        // every key of [a, b] agrees with both ends above `bit`, so the range is zeros then ones there: the last zero
        const uint32_t s = uint32_t(std::partition_point(keys.begin() + a, keys.begin() + b + 1, [bit](uint64_t k) { return ((k >> bit) & 1u) == 0u; }) - keys.begin()) - 1u;
        float box[12];
        const uint32_t l = child(a, s, s, self, depth + 1, box);
        const uint32_t r = child(s + 1u, b, s + 1u, self, depth + 1, box + 6);
        Node64& n = nodes[self];
        n.kind = 1u; n.parent = parent; n.first = l; n.last = r;
        std::memcpy(n.box, box, sizeof(box));
    }
};

}  // namespace

extern "C" int racc_host_world_prepare(const float* transforms12, const float* root_boxes6, uint32_t count,
                                       float* inv12_out, float* world_boxes6_out, float* ray_pad_out,
                                       void* nodes64_out, uint32_t node_capacity, uint32_t* node_count_out,
                                       uint32_t* order_out, uint32_t* height_out) try {
    if (!transforms12 || !root_boxes6) return refuse(kPrepare, RACC_HIP_ERR_INVALID, "transforms / root boxes pointer is NULL");
    if (!inv12_out || !world_boxes6_out || !ray_pad_out || !nodes64_out || !node_count_out || !order_out || !height_out) return refuse(kPrepare, RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    if (!count) return refuse(kPrepare, RACC_HIP_ERR_INVALID, "count is 0: a world has at least one instance");
    if (count > RACC_HIP_WORLD_MAX_INSTANCES) return refuse(kPrepare, RACC_HIP_ERR_INVALID, "more than 2^20 instances");
    const uint32_t nodesNeeded = count > 1u ? count - 1u : 1u;
    if (node_capacity < nodesNeeded) return refuse(kPrepare, RACC_HIP_ERR_INVALID, "node_capacity is below max(count - 1, 1)");

    // everything is validated and computed into buffers of our own before the first output byte is written
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6);
    float rayPad = 0.0f;
    if (int rc = perInstance(kPrepare, transforms12, root_boxes6, count, inv.data(), boxes.data(), rayPad)) return rc;

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
    return refuse(kPrepare, RACC_HIP_ERR_NOMEM, "out of host memory");
}

// Internal (not in the header): the per-instance rule for racc_hip_world_refit (racc_world_refit.inc), whose refusals name `who`.
// inv12_out / world_boxes6_out are scratch of the caller's; nothing else is written.
extern "C" int racc_host_world_instances_(const char* who, const float* transforms12, const float* root_boxes6, uint32_t count,
                                          float* inv12_out, float* world_boxes6_out, float* ray_pad_out) {
    if (int rc = refuseShape(who, transforms12, root_boxes6, count)) return rc;
    if (!inv12_out || !world_boxes6_out || !ray_pad_out) return refuse(who, RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    return perInstance(who, transforms12, root_boxes6, count, inv12_out, world_boxes6_out, *ray_pad_out);
}

extern "C" int racc_host_world_refit(const float* transforms12, const float* root_boxes6, uint32_t count,
                                     const void* nodes64, uint32_t node_count, const uint32_t* order,
                                     float* inv12_out, float* world_boxes6_out, float* ray_pad_out, void* nodes64_out) try {
    if (int rc = refuseShape(kRefit, transforms12, root_boxes6, count)) return rc;
    if (!nodes64 || !order) return refuse(kRefit, RACC_HIP_ERR_INVALID, "nodes / order pointer is NULL");
    if (!inv12_out || !world_boxes6_out || !ray_pad_out || !nodes64_out) return refuse(kRefit, RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    if (node_count != (count > 1u ? count - 1u : 1u)) return refuse(kRefit, RACC_HIP_ERR_INVALID, "node_count is not max(count - 1, 1)");

    // everything is validated and computed into buffers of our own before the first output byte is written (outputs may alias inputs)
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6);
    float rayPad = 0.0f;
    if (int rc = perInstance(kRefit, transforms12, root_boxes6, count, inv.data(), boxes.data(), rayPad)) return rc;

    std::vector<Node64> nodes(node_count);
    std::memcpy(nodes.data(), nodes64, size_t(node_count) * sizeof(Node64));
    std::vector<uint8_t> seen(count, 0);
    for (uint32_t i = 0; i < count; ++i) {
        if (order[i] >= count || seen[order[i]]) return refuse(kRefit, RACC_HIP_ERR_INVALID, "order is not a permutation of [0, count)");
        seen[order[i]] = 1;
    }
    // the topology, walked from the root: every node reached exactly once, every position of `order` in exactly one leaf
    std::vector<uint8_t> nodeSeen(node_count, 0), posSeen(count, 0);
    std::vector<uint32_t> visit;      // parents before their children
    visit.reserve(node_count);
    visit.push_back(0u);
    nodeSeen[0] = 1;
    for (size_t at = 0; at < visit.size(); ++at) {
        const Node64& n = nodes[visit[at]];
        for (const uint32_t c : { n.first, n.last }) {
            if (c & 0x80000000u) {
                const uint32_t i = c & 0x7FFFFFFFu;
                if (i >= node_count) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a child index is not below node_count");
                if (nodeSeen[i]) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a node is reached twice");
                nodeSeen[i] = 1;
                visit.push_back(i);
            } else {
                const uint32_t first = c & 0xFFFFFFu, cnt = c >> 24;
                if (cnt > 1u) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a leaf names more than one instance");
                if (cnt == 0u) continue;      // the empty reference (a one-instance world's last child): its box is kept
                if (first >= count) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a leaf position is not below count");
                if (posSeen[first]) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a leaf position is named twice");
                posSeen[first] = 1;
            }
        }
    }
    if (visit.size() != node_count) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a node is never reached from the root");
    for (uint32_t i = 0; i < count; ++i) if (!posSeen[i]) return refuse(kRefit, RACC_HIP_ERR_INVALID, "a position of order is in no leaf");

    // boxes bottom-up: children before their parents
    for (size_t at = visit.size(); at-- > 0;) {
        Node64& n = nodes[visit[at]];
        for (int side = 0; side < 2; ++side) {
            const uint32_t c = side ? n.last : n.first;
            float* box = n.box + side * 6;
            if (c & 0x80000000u) {
                const float* acc = nodes[c & 0x7FFFFFFFu].box;      // the child's first-child box (accumulator), then its last-child box
                const float* b = acc + 6;
                for (int k = 0; k < 3; ++k) { box[k] = b[k] < acc[k] ? b[k] : acc[k]; box[3 + k] = b[3 + k] > acc[3 + k] ? b[3 + k] : acc[3 + k]; }
            } else if (c >> 24) {
                std::memcpy(box, &boxes[size_t(order[c & 0xFFFFFFu]) * 6], 24);
            }
        }
    }

    std::memcpy(inv12_out, inv.data(), inv.size() * sizeof(float));
    std::memcpy(world_boxes6_out, boxes.data(), boxes.size() * sizeof(float));
    *ray_pad_out = rayPad;
    std::memcpy(nodes64_out, nodes.data(), nodes.size() * sizeof(Node64));
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return refuse(kRefit, RACC_HIP_ERR_NOMEM, "out of host memory");
}

// The specification of racc_hip_world_rebuild* (racc_world_rebuild.inc): the top-level LBVH of racc_world_rebuild_rule.h.
extern "C" int racc_host_world_rebuild(const float* transforms12, const float* root_boxes6, uint32_t count,
                                       float* inv12_out, float* world_boxes6_out, float* ray_pad_out,
                                       void* nodes64_out, uint32_t node_capacity, uint32_t* node_count_out,
                                       uint32_t* order_out, uint32_t* height_out) try {
    namespace rule = racc_world_rebuild_rule;
    if (!transforms12 || !root_boxes6) return refuse(kRebuild, RACC_HIP_ERR_INVALID, "transforms / root boxes pointer is NULL");
    if (!inv12_out || !world_boxes6_out || !ray_pad_out || !nodes64_out || !node_count_out || !order_out || !height_out) return refuse(kRebuild, RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    if (!count) return refuse(kRebuild, RACC_HIP_ERR_INVALID, "count is 0: a world has at least one instance");
    if (count > RACC_HIP_WORLD_MAX_INSTANCES) return refuse(kRebuild, RACC_HIP_ERR_INVALID, "more than 2^20 instances");
    const uint32_t nodesNeeded = count > 1u ? count - 1u : 1u;
    if (node_capacity < nodesNeeded) return refuse(kRebuild, RACC_HIP_ERR_INVALID, "node_capacity is below max(count - 1, 1)");

    // everything is validated and computed into buffers of our own before the first output byte is written
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6);
    float rayPad = 0.0f;
    if (int rc = perInstance(kRebuild, transforms12, root_boxes6, count, inv.data(), boxes.data(), rayPad)) return rc;

    std::vector<float> centre(size_t(count) * 3);
    float lo[3], hi[3];
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k) {
            const float c = rule::centre(boxes[size_t(i) * 6 + k], boxes[size_t(i) * 6 + 3 + k]);
            centre[size_t(i) * 3 + k] = c;
            if (!i || c < lo[k]) lo[k] = c;
            if (!i || c > hi[k]) hi[k] = c;
        }
    std::vector<uint64_t> keys(count);
    for (uint32_t i = 0; i < count; ++i) keys[i] = rule::key(rule::field(&centre[size_t(i) * 3], lo, hi), i);
    std::sort(keys.begin(), keys.end());

    std::vector<Node64> nodes(nodesNeeded);
    uint32_t height = 1;
    if (count == 1u) {
        Node64 n{};
        n.kind = 1u; n.parent = 0xFFFFFFFFu; n.first = (1u << 24) | 0u; n.last = 0u;
        std::memcpy(n.box, boxes.data(), 24);
        nodes[0] = n;
    } else {
        LbvhBuilder bl{ boxes.data(), keys, nodes };
        bl.build(0u, 0u, count - 1u, 0xFFFFFFFFu, 1u);
        height = bl.height;
    }

    std::memcpy(inv12_out, inv.data(), inv.size() * sizeof(float));
    std::memcpy(world_boxes6_out, boxes.data(), boxes.size() * sizeof(float));
    *ray_pad_out = rayPad;
    std::memcpy(nodes64_out, nodes.data(), nodes.size() * sizeof(Node64));
    *node_count_out = nodesNeeded;
    for (uint32_t p = 0; p < count; ++p) order_out[p] = uint32_t(keys[p]);
    *height_out = height;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return refuse(kRebuild, RACC_HIP_ERR_NOMEM, "out of host memory");
}
