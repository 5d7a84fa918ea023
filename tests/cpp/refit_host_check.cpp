// refit_host_check — stand-alone driver of racc_host_blobs_refit (rayaccel_amd/csrc/scene_refit.cpp) for the AddressSanitizer + UBSan
// build (`make asan`): builds a 200-triangle mesh with the reference builder, refits it to moved vertices and back, in place and into
// separate arrays, and compares every box with a recursive fold of its own and every pair record with its own subtractions.
// Exit code 0 = all equal; the sanitizers abort on their own findings.
#include "racc_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Node { uint32_t kind, parent, first, last; float box[12]; };
struct Box { float mn[3], mx[3]; };

struct Mesh {
    std::vector<float> vertices;      // xyzw
    std::vector<uint32_t> indices;
};

const uint32_t* g_remap;
const Mesh* g_mesh;
const Node* g_nodes;

void quadOf(uint32_t p, uint32_t q[4]) {
    const uint32_t r0 = g_remap[2 * p], r1 = g_remap[2 * p + 1];
    const uint32_t* a = &g_mesh->indices[size_t(r0 & 0x3FFFFFFFu) * 3];
    const uint32_t ea = r0 >> 30;
    q[0] = a[ea]; q[1] = a[(ea + 1) % 3]; q[2] = a[(ea + 2) % 3]; q[3] = q[1];
    if (r1) q[3] = g_mesh->indices[size_t(r1 & 0x3FFFFFFFu) * 3 + ((r1 >> 30) - 1 + 2) % 3];
}

Box boxOf(uint32_t ref) {
    Box b;
    if (ref & 0x80000000u) {
        const Node& n = g_nodes[ref & 0x7FFFFFFFu];
        const Box l = boxOf(n.first), r = boxOf(n.last);
        for (int k = 0; k < 3; ++k) { b.mn[k] = r.mn[k] < l.mn[k] ? r.mn[k] : l.mn[k]; b.mx[k] = r.mx[k] > l.mx[k] ? r.mx[k] : l.mx[k]; }
        return b;
    }
    const uint32_t first = ref & 0xFFFFFFu, cnt = ref >> 24;
    uint32_t q[4];
    quadOf(first, q);
    for (int k = 0; k < 3; ++k) b.mn[k] = b.mx[k] = g_mesh->vertices[size_t(q[0]) * 4 + k];
    for (uint32_t p = first; p < first + cnt; ++p) {
        quadOf(p, q);
        for (int v = 0; v < 4; ++v)
            for (int k = 0; k < 3; ++k) {
                const float x = g_mesh->vertices[size_t(q[v]) * 4 + k];
                b.mn[k] = x < b.mn[k] ? x : b.mn[k];
                b.mx[k] = x > b.mx[k] ? x : b.mx[k];
            }
    }
    return b;
}

int check(const Mesh& mesh, const std::vector<Node>& nodes, const std::vector<float>& pairs, uint32_t pairCount, uint32_t padded, const uint32_t* remap, const char* what) {
    g_mesh = &mesh; g_nodes = nodes.data(); g_remap = remap;
    int bad = 0;
    for (size_t n = 0; n < nodes.size(); ++n) {
        const Box l = boxOf(nodes[n].first), r = boxOf(nodes[n].last);
        float want[12];
        std::memcpy(want, l.mn, 12); std::memcpy(want + 3, l.mx, 12); std::memcpy(want + 6, r.mn, 12); std::memcpy(want + 9, r.mx, 12);
        if (std::memcmp(want, nodes[n].box, 48) != 0) ++bad;
    }
    for (uint32_t p = 0; p < padded; ++p) {
        uint32_t q[4];
        quadOf(p < pairCount ? p : 0u, q);
        const float *p0 = &mesh.vertices[size_t(q[0]) * 4], *p1 = &mesh.vertices[size_t(q[1]) * 4], *p2 = &mesh.vertices[size_t(q[2]) * 4], *p3 = &mesh.vertices[size_t(q[3]) * 4];
        const float want[12] = { p0[0] - p1[0], p0[1] - p1[1], p0[2] - p1[2], p3[0] - p0[0], p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], p3[1] - p0[1],
                                 p0[0], p0[1], p0[2], p3[2] - p0[2] };
        if (std::memcmp(want, &pairs[size_t(p) * 12], 48) != 0) ++bad;
    }
    if (bad) std::fprintf(stderr, "refit_host_check: %s: %d records differ from the driver's own fold\n", what, bad);
    return bad;
}

}  // namespace

int main() {
    // a 10 x 10 grid of quads (200 triangles, 121 vertices) over a bumpy height field
    Mesh mesh;
    const int N = 10;
    for (int z = 0; z <= N; ++z)
        for (int x = 0; x <= N; ++x) {
            const float v[4] = { float(x), std::sin(0.7f * float(x)) * std::cos(0.9f * float(z)), float(z), 1.0f };
            mesh.vertices.insert(mesh.vertices.end(), v, v + 4);
        }
    for (int z = 0; z < N; ++z)
        for (int x = 0; x < N; ++x) {
            const uint32_t a = uint32_t(z * (N + 1) + x), b = a + 1, c = a + uint32_t(N + 1), d = c + 1;
            const uint32_t t[6] = { a, c, b, b, c, d };
            mesh.indices.insert(mesh.indices.end(), t, t + 6);
        }
    const uint32_t vertexCount = uint32_t(mesh.vertices.size() / 4), indexCount = uint32_t(mesh.indices.size());

    racc_host_build_options opt;
    std::memset(&opt, 0, sizeof(opt));
    opt.struct_size = sizeof(opt);
    opt.quality = 0;
    racc_host_scene* host = nullptr;
    if (racc_host_scene_build_ex(mesh.vertices.data(), vertexCount, mesh.indices.data(), indexCount, &opt, &host) != RACC_HIP_OK) {
        std::fprintf(stderr, "refit_host_check: build failed: %s\n", racc_hip_last_error());
        return 2;
    }
    const void *pn = nullptr, *pp = nullptr;
    const uint32_t* remap = nullptr;
    uint32_t nodeCount = 0, padded = 0, pairCount = 0, remapCount = 0;
    racc_host_scene_blobs(host, &pn, &nodeCount, &pp, &padded, &pairCount, &remap, &remapCount);
    std::vector<Node> built(static_cast<const Node*>(pn), static_cast<const Node*>(pn) + nodeCount);
    std::vector<float> builtPairs(static_cast<const float*>(pp), static_cast<const float*>(pp) + size_t(padded) * 12);

    int bad = check(mesh, built, builtPairs, pairCount, padded, remap, "the build itself");

    // refit 1: moved vertices, into separate arrays
    Mesh moved = mesh;
    for (uint32_t i = 0; i < vertexCount; ++i) {
        moved.vertices[size_t(i) * 4 + 0] += 0.3f * std::sin(float(i));
        moved.vertices[size_t(i) * 4 + 1] += 2.0f * std::cos(0.37f * float(i));
        moved.vertices[size_t(i) * 4 + 2] -= 0.25f * std::sin(1.3f * float(i));
    }
    std::vector<Node> nodes(nodeCount);
    std::vector<float> pairs(size_t(padded) * 12);
    int rc = racc_host_blobs_refit(built.data(), nodeCount, builtPairs.data(), padded, pairCount, remap, remapCount, moved.vertices.data(), vertexCount,
                                   moved.indices.data(), indexCount, nodes.data(), pairs.data());
    if (rc != RACC_HIP_OK) { std::fprintf(stderr, "refit_host_check: refit 1 failed: %s\n", racc_hip_last_error()); return 3; }
    bad += check(moved, nodes, pairs, pairCount, padded, remap, "refit to moved vertices");

    // refit 2: back to the build's vertices, in place (outputs alias inputs): the reference builder's tree comes back byte for byte
    rc = racc_host_blobs_refit(nodes.data(), nodeCount, pairs.data(), padded, pairCount, remap, remapCount, mesh.vertices.data(), vertexCount,
                               mesh.indices.data(), indexCount, nodes.data(), pairs.data());
    if (rc != RACC_HIP_OK) { std::fprintf(stderr, "refit_host_check: refit 2 failed: %s\n", racc_hip_last_error()); return 3; }
    bad += check(mesh, nodes, pairs, pairCount, padded, remap, "refit back, in place");
    if (std::memcmp(nodes.data(), built.data(), size_t(nodeCount) * 64) != 0 || std::memcmp(pairs.data(), builtPairs.data(), pairs.size() * 4) != 0) {
        std::fprintf(stderr, "refit_host_check: the refit back to the build's vertices differs from the build\n");
        ++bad;
    }

    // a refusal writes nothing: an index beyond the vertices
    std::vector<uint32_t> wrong = mesh.indices;
    wrong[7] = vertexCount;
    const std::vector<Node> before = nodes;
    rc = racc_host_blobs_refit(nodes.data(), nodeCount, pairs.data(), padded, pairCount, remap, remapCount, mesh.vertices.data(), vertexCount,
                               wrong.data(), indexCount, nodes.data(), pairs.data());
    if (rc != RACC_HIP_ERR_INVALID || std::memcmp(before.data(), nodes.data(), size_t(nodeCount) * 64) != 0) { std::fprintf(stderr, "refit_host_check: a bad index was not refused cleanly\n"); ++bad; }

    racc_host_scene_free(host);
    std::printf("refit_host_check: %u nodes, %u pairs (%u padded), %d differences\n", nodeCount, pairCount, padded, bad);
    return bad ? 1 : 0;
}
