// world_refit_host_check — stand-alone driver of racc_host_world_refit (rayaccel_amd/csrc/world_build.cpp) for the AddressSanitizer +
// UBSan build (`make asan`): worlds of 1 and 257 instances prepared, then refitted to moved transforms; inv / world boxes / ray pad against
// racc_host_world_prepare of the moved transforms as bytes, the topology words kept, every child box against a walk of its own over the
// world boxes below it; the same call with its outputs aliasing its inputs; refusals that must leave the outputs untouched.
// Exit code 0 = all good; the sanitizers abort on their own findings.
#include "racc_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Node { uint32_t kind, parent, first, last; float box[12]; };

uint64_t g_state = 0x243F6A8885A308D3ull;
double uniform() {      // xorshift64*, [0, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return double((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
double range(double a, double b) { return a + (b - a) * uniform(); }

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failures < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

void makeTransforms(std::vector<float>& t, uint32_t count, double spread, double maxScale) {
    t.resize(size_t(count) * 12);
    for (uint32_t i = 0; i < count; ++i) {
        double ax[3] = { range(-1, 1), range(-1, 1), range(-1, 1) };
        double len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        if (len < 1e-3) { ax[0] = 1; ax[1] = ax[2] = 0; len = 1; }
        for (double& a : ax) a /= len;
        const double ang = range(0, 6.283185307179586), c = std::cos(ang), s = std::sin(ang);
        double R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) R[r][k] = (r == k ? c : 0.0) + (1 - c) * ax[r] * ax[k];
        R[0][1] -= s * ax[2]; R[0][2] += s * ax[1]; R[1][0] += s * ax[2]; R[1][2] -= s * ax[0]; R[2][0] -= s * ax[1]; R[2][1] += s * ax[0];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) t[size_t(i) * 12 + r * 4 + k] = float(R[r][k] * range(0.2, maxScale) * (uniform() < 0.3 ? -1.0 : 1.0));
            t[size_t(i) * 12 + r * 4 + 3] = float(range(-spread, spread));
        }
    }
}

// the box of everything below `ref`, folded over the instances' world boxes
bool below(const std::vector<Node>& nodes, const std::vector<uint32_t>& order, const std::vector<float>& boxes, uint32_t ref, float out[6]) {
    if (ref & 0x80000000u) {
        const Node& n = nodes[ref & 0x7FFFFFFFu];
        float l[6], r[6];
        const bool hl = below(nodes, order, boxes, n.first, l), hr = below(nodes, order, boxes, n.last, r);
        if (!hl && !hr) return false;
        for (int k = 0; k < 3; ++k) {
            out[k] = !hr ? l[k] : (!hl ? r[k] : std::fmin(l[k], r[k]));
            out[3 + k] = !hr ? l[3 + k] : (!hl ? r[3 + k] : std::fmax(l[3 + k], r[3 + k]));
        }
        return true;
    }
    if ((ref >> 24) == 0u) return false;
    std::memcpy(out, &boxes[size_t(order[ref & 0xFFFFFFu]) * 6], 24);
    return true;
}

void checkCount(uint32_t count) {
    const uint32_t cap = count > 1 ? count - 1 : 1;
    std::vector<float> t, moved, rb(size_t(count) * 6);
    makeTransforms(t, count, 100.0, 4.0);
    makeTransforms(moved, count, 1e5, 1e3);
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k) { rb[size_t(i) * 6 + k] = float(range(-10, 10)); rb[size_t(i) * 6 + 3 + k] = rb[size_t(i) * 6 + k] + (uniform() < 0.1 ? 0.0f : float(range(0, 5))); }
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6), inv2(inv), boxes2(boxes), inv3(inv), boxes3(boxes);
    std::vector<Node> nodes(cap), nodes2(cap), nodes3(cap);
    std::vector<uint32_t> order(count), order2(count);
    uint32_t nodeCount = 0, height = 0;
    float pad = 0, pad2 = 0, pad3 = 0;
    CHECK(racc_host_world_prepare(t.data(), rb.data(), count, inv.data(), boxes.data(), &pad, nodes.data(), cap, &nodeCount, order.data(), &height) == RACC_HIP_OK, "%u: prepare refused: %s", count, racc_hip_last_error());
    CHECK(racc_host_world_prepare(moved.data(), rb.data(), count, inv2.data(), boxes2.data(), &pad2, nodes2.data(), cap, &nodeCount, order2.data(), &height) == RACC_HIP_OK, "%u: prepare(moved) refused: %s", count, racc_hip_last_error());
    const int rc = racc_host_world_refit(moved.data(), rb.data(), count, nodes.data(), cap, order.data(), inv3.data(), boxes3.data(), &pad3, nodes3.data());
    CHECK(rc == RACC_HIP_OK, "%u: refit refused: %s", count, racc_hip_last_error());
    if (rc != RACC_HIP_OK) return;
    CHECK(!std::memcmp(inv3.data(), inv2.data(), inv2.size() * 4) && !std::memcmp(boxes3.data(), boxes2.data(), boxes2.size() * 4) && !std::memcmp(&pad3, &pad2, 4), "%u: inv / world boxes / ray pad differ from prepare(moved)", count);
    for (uint32_t n = 0; n < cap; ++n) {
        CHECK(!std::memcmp(&nodes3[n], &nodes[n], 16), "%u: node %u: topology words changed", count, n);
        for (int side = 0; side < 2; ++side) {
            float want[6];
            const uint32_t ref = side ? nodes3[n].last : nodes3[n].first;
            if (below(nodes3, order, boxes3, ref, want)) {
                for (int k = 0; k < 6; ++k) CHECK(nodes3[n].box[side * 6 + k] == want[k], "%u: node %u side %d plane %d: %g, below it %g", count, n, side, k, nodes3[n].box[side * 6 + k], want[k]);
            } else CHECK(!std::memcmp(nodes3[n].box + side * 6, nodes[n].box + side * 6, 24), "%u: node %u: the empty reference's box was not copied", count, n);
        }
    }
    // outputs aliasing inputs: inv over the transforms, world boxes over the root boxes, nodes over nodes
    std::vector<float> ta(moved), ba(rb);
    std::vector<Node> na(nodes);
    float pad4 = 0;
    CHECK(racc_host_world_refit(ta.data(), ba.data(), count, na.data(), cap, order.data(), ta.data(), ba.data(), &pad4, na.data()) == RACC_HIP_OK, "%u: aliased refit refused: %s", count, racc_hip_last_error());
    CHECK(!std::memcmp(ta.data(), inv3.data(), inv3.size() * 4) && !std::memcmp(ba.data(), boxes3.data(), boxes3.size() * 4) && !std::memcmp(na.data(), nodes3.data(), size_t(cap) * 64) && pad4 == pad3, "%u: aliased outputs differ", count);
    // refusals: nothing is written
    std::vector<float> invr(inv.size(), -7.0f), boxr(boxes.size(), -7.0f);
    std::vector<Node> nr(cap);
    std::memset(nr.data(), 0xAB, size_t(cap) * 64);
    float padr = -7.0f;
    auto untouched = [&]() {
        for (float x : invr) if (x != -7.0f) return false;
        for (float x : boxr) if (x != -7.0f) return false;
        for (size_t b = 0; b < size_t(cap) * 64; ++b) if (reinterpret_cast<const unsigned char*>(nr.data())[b] != 0xAB) return false;
        return padr == -7.0f;
    };
    std::vector<float> bad(moved);
    for (int k = 0; k < 12; ++k) bad[size_t(count - 1) * 12 + k] = 0.0f;
    CHECK(racc_host_world_refit(bad.data(), rb.data(), count, nodes.data(), cap, order.data(), invr.data(), boxr.data(), &padr, nr.data()) == RACC_HIP_ERR_INVALID && untouched(), "%u: zero transform accepted or outputs written", count);
    CHECK(std::strstr(racc_hip_last_error(), "racc_host_world_refit") != nullptr, "the message does not name the entry: %s", racc_hip_last_error());
    bad = moved; bad[5] = NAN;
    CHECK(racc_host_world_refit(bad.data(), rb.data(), count, nodes.data(), cap, order.data(), invr.data(), boxr.data(), &padr, nr.data()) == RACC_HIP_ERR_INVALID && untouched(), "%u: NaN coefficient accepted or outputs written", count);
    std::vector<Node> broken(nodes);
    broken[0].first = 0x80000000u | cap;      // a child index out of range
    CHECK(racc_host_world_refit(moved.data(), rb.data(), count, broken.data(), cap, order.data(), invr.data(), boxr.data(), &padr, nr.data()) == RACC_HIP_ERR_INVALID && untouched(), "%u: child index out of range accepted or outputs written", count);
    std::vector<uint32_t> dup(order);
    dup[0] = count;
    CHECK(racc_host_world_refit(moved.data(), rb.data(), count, nodes.data(), cap, dup.data(), invr.data(), boxr.data(), &padr, nr.data()) == RACC_HIP_ERR_INVALID && untouched(), "%u: order out of range accepted or outputs written", count);
    CHECK(racc_host_world_refit(moved.data(), rb.data(), count, nodes.data(), cap + 1, order.data(), invr.data(), boxr.data(), &padr, nr.data()) == RACC_HIP_ERR_INVALID && untouched(), "%u: wrong node_count accepted or outputs written", count);
}

}  // namespace

int main() {
    int refits = 0;
    for (uint32_t count : { 1u, 257u }) { checkCount(count); ++refits; }
    std::printf("%d refits checked, %d failures\n", refits, g_failures);
    return g_failures ? 1 : 0;
}
