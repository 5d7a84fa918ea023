// scene_rebuild.cpp — racc_host_scene_rebuild (include/racc_hip.h): the host specification of the bottom-level rebuild on the device
// (racc_scene_rebuild.inc), scene_refit.cpp's sibling.  No GPU code.
//
// The rule is racc_scene_rebuild_rule.h's: an LBVH over the triangles of a mesh — one triangle per pair, one pair per leaf — in the
// reference's blob formats.  The formulation here is deliberately not the device's: std::sort over (field, index) and a recursive top-down
// split by partition_point, against rocPRIM's radix sort and Karras's per-node searches there; the device reproduces the bytes.
// Everything is validated and computed into buffers of our own before the first output byte is written.
#include "racc_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "racc_scene_rebuild_rule.h"

extern "C" void racc_hip_set_error_(const char* msg);

namespace {

namespace rule = racc_scene_rebuild_rule;

struct Node64 { uint32_t kind, parent, first, last; float box[12]; };      // leftMin[3], leftMax[3], rightMin[3], rightMax[3] (Scene.cpp:73-78)
struct Pair48 { float e1[3], e3x, e2[3], e3y, p0[3], e3z; };               // Scene.cpp:83-87
static_assert(sizeof(Node64) == 64 && sizeof(Pair48) == 48, "reference record sizes");

struct Key { uint64_t field; uint32_t index; };

int refuse(int code, const char* what) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "racc_host_scene_rebuild: %s", what);
    racc_hip_set_error_(msg);
    return code;
}

// bit `bit` (94 = the highest) of the 95-bit key
inline uint32_t keyBit(const Key& k, int bit) { return bit >= 32 ? uint32_t((k.field >> (bit - 32)) & 1u) : ((k.index >> bit) & 1u); }

struct Builder {
    const float* boxes;                 // [T][6] min, max, by triangle
    const std::vector<Key>& keys;       // sorted
    std::vector<Node64>& nodes;         // T - 1 records, numbered as the rule says
    uint32_t height = 0;

    // the reference of the child covering [a, b], built if it is a node
    uint32_t child(uint32_t a, uint32_t b, uint32_t node, uint32_t parent, uint32_t depth, float* box) {
        if (a == b) {
            std::memcpy(box, boxes + size_t(keys[a].index) * 6, 24);
            return (1u << 24) | a;
        }
        build(node, a, b, parent, depth);
        const float* acc = nodes[node].box;      // the child's first-child box (accumulator), then its last-child box
        const float* o = acc + 6;
        for (int k = 0; k < 3; ++k) { box[k] = rule::foldMin(acc[k], o[k]); box[3 + k] = rule::foldMax(acc[3 + k], o[3 + k]); }
        return 0x80000000u | node;
    }

    // node `self` over the positions [a, b], a < b.  (Depth: one level per key bit at most, rule 9.)
    void build(uint32_t self, uint32_t a, uint32_t b, uint32_t parent, uint32_t depth) {
        if (depth > height) height = depth;
        const int bit = 94 - rule::commonPrefix(keys[a].field, keys[a].index, keys[b].field, keys[b].index);
        // every key of [a, b] agrees with both ends above `bit`, so the range is zeros then ones there: the last zero
        const uint32_t s = uint32_t(std::partition_point(keys.begin() + a, keys.begin() + b + 1, [bit](const Key& k) { return keyBit(k, bit) == 0u; }) - keys.begin()) - 1u;
        float box[12];
        const uint32_t l = child(a, s, s, self, depth + 1, box);
        const uint32_t r = child(s + 1u, b, s + 1u, self, depth + 1, box + 6);
        Node64& n = nodes[self];
        n.kind = 1u; n.parent = parent; n.first = l; n.last = r;
        std::memcpy(n.box, box, sizeof(box));
    }
};

}  // namespace

extern "C" int racc_host_scene_rebuild(const float* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                                       void* nodes64_out, uint32_t node_capacity, uint32_t* node_count,
                                       void* pairs48_out, uint32_t pair_capacity, uint32_t* pair_count_padded,
                                       uint32_t* remap_out, uint32_t remap_capacity, uint32_t* remap_count, uint32_t* height) try {
    if (!vertices || !indices) return refuse(RACC_HIP_ERR_INVALID, "vertices / indices pointer is NULL");
    if (!nodes64_out || !node_count || !pairs48_out || !pair_count_padded || !remap_out || !remap_count || !height) return refuse(RACC_HIP_ERR_INVALID, "an output pointer is NULL");
    if (index_count % 3 != 0) return refuse(RACC_HIP_ERR_INVALID, "index_count is not a multiple of 3 (Scene.cpp:186)");
    const uint32_t T = index_count / 3;
    if (T < 2u) return refuse(RACC_HIP_ERR_INVALID, "fewer than 2 triangles: a scene has at least one inner node");
    if (T >= rule::kMaxTriangles) return refuse(RACC_HIP_ERR_LIMIT, "2^24 triangles or more: a leaf reference holds a 24-bit pair index (Scene.cpp:294-312)");
    const uint32_t padded = rule::paddedPairs(T);
    if (node_capacity < T - 1u) return refuse(RACC_HIP_ERR_INVALID, "node_capacity is below index_count / 3 - 1");
    if (pair_capacity < padded) return refuse(RACC_HIP_ERR_INVALID, "pair_capacity is below the padded pair count (the smallest multiple of 32 above index_count / 3)");
    if (remap_capacity / 2u < T) return refuse(RACC_HIP_ERR_INVALID, "remap_capacity is below 2 * (index_count / 3)");
    for (uint32_t i = 0; i < index_count; ++i)
        if (indices[i] >= vertex_count) return refuse(RACC_HIP_ERR_INVALID, "an index is not below vertex_count");
    for (size_t i = 0; i < size_t(vertex_count); ++i)
        if (!std::isfinite(vertices[i * 4]) || !std::isfinite(vertices[i * 4 + 1]) || !std::isfinite(vertices[i * 4 + 2])) return refuse(RACC_HIP_ERR_INVALID, "a vertex coordinate is not finite");

    // rules 1-3
    std::vector<float> boxes(size_t(T) * 6), centres(size_t(T) * 3);
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t* a = indices + size_t(t) * 3;
        float* box = &boxes[size_t(t) * 6];
        for (int k = 0; k < 3; ++k) box[k] = box[3 + k] = vertices[size_t(a[0]) * 4 + k];
        for (int v = 1; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                const float p = vertices[size_t(a[v]) * 4 + k];
                box[k] = rule::foldMin(box[k], p); box[3 + k] = rule::foldMax(box[3 + k], p);
            }
        for (int k = 0; k < 3; ++k) {
            const float c = rule::centre(box[k], box[3 + k]);
            centres[size_t(t) * 3 + k] = c;
            if (!t || c < lo[k]) lo[k] = c;
            if (!t || c > hi[k]) hi[k] = c;
        }
    }
    // rules 4-5
    std::vector<Key> keys(T);
    for (uint32_t t = 0; t < T; ++t) keys[t] = Key{ rule::field(&centres[size_t(t) * 3], lo, hi), t };
    std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) { return x.field != y.field ? x.field < y.field : x.index < y.index; });
    // rule 6
    std::vector<Pair48> pairs(padded);
    for (uint32_t p = 0; p < T; ++p) {      // packPair (scene_build.cpp; Scene.cpp:149-153) of a[0], a[1], a[2], a[1]
        const uint32_t* a = indices + size_t(keys[p].index) * 3;
        const float *p0 = vertices + size_t(a[0]) * 4, *p1 = vertices + size_t(a[1]) * 4, *p2 = vertices + size_t(a[2]) * 4, *p3 = p1;
        Pair48& r = pairs[p];
        for (int k = 0; k < 3; ++k) { r.e1[k] = p0[k] - p1[k]; r.e2[k] = p2[k] - p0[k]; r.p0[k] = p0[k]; }
        r.e3x = p3[0] - p0[0]; r.e3y = p3[1] - p0[1]; r.e3z = p3[2] - p0[2];
    }
    for (uint32_t p = T; p < padded; ++p) pairs[p] = pairs[0];
    // rules 7-8
    std::vector<Node64> nodes(T - 1u);
    Builder bl{ boxes.data(), keys, nodes };
    bl.build(0u, 0u, T - 1u, 0xFFFFFFFFu, 1u);

    std::memcpy(nodes64_out, nodes.data(), nodes.size() * sizeof(Node64));
    *node_count = T - 1u;
    std::memcpy(pairs48_out, pairs.data(), pairs.size() * sizeof(Pair48));
    *pair_count_padded = padded;
    for (uint32_t p = 0; p < T; ++p) { remap_out[2 * size_t(p)] = keys[p].index; remap_out[2 * size_t(p) + 1] = 0u; }
    *remap_count = 2u * T;
    *height = bl.height;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return refuse(RACC_HIP_ERR_NOMEM, "out of host memory");
}
