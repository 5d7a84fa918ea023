// world_rebuild_host_check — stand-alone driver of racc_host_world_rebuild (rayaccel_amd/csrc/world_build.cpp) for the AddressSanitizer +
// UBSan build (`make asan`): random worlds of 1, 2, 3, 257 and 1000 instances, 1000 instances in one place, a Morton chain of 31 and the
// chain with a crowd at its end.  Per world: inv / world boxes / ray pad against racc_host_world_prepare as bytes; the keys restated here
// (without the rule's header) ascending along `order`; every record's range split behind the last key with a 0 in the highest bit its two
// end keys differ in, and numbered as the rule says; every record reached once, every position named once; the boxes against
// racc_host_world_refit of the output as bytes; the height against a walk and the bound; two calls byte-equal; refusals that must leave the
// outputs untouched and name the entry.  Exit code 0 = all good; the sanitizers abort on their own findings.
#include "racc_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Node { uint32_t kind, parent, first, last; float box[12]; };

uint64_t g_state = 0x13198A2E03707344ull;
double uniform() {      // xorshift64*, [0, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return double((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
double range(double a, double b) { return a + (b - a) * uniform(); }

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failures < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

void randomTransforms(std::vector<float>& t, uint32_t count, double spread) {
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
            for (int k = 0; k < 3; ++k) t[size_t(i) * 12 + r * 4 + k] = float(R[r][k] * range(0.2, 4.0) * (uniform() < 0.3 ? -1.0 : 1.0));
            t[size_t(i) * 12 + r * 4 + 3] = float(range(-spread, spread));
        }
    }
}

void translations(std::vector<float>& t, const std::vector<double>& x) {
    t.assign(x.size() * 12, 0.0f);
    for (size_t i = 0; i < x.size(); ++i) { t[i * 12 + 0] = t[i * 12 + 5] = t[i * 12 + 10] = 1.0f; t[i * 12 + 3] = float(x[i]); t[i * 12 + 7] = -2.0f; t[i * 12 + 11] = 5.0f; }
}

// the keys of the rule, restated: centres in double rounded to float, 10 bits per axis against the centre bounds, x highest
std::vector<uint64_t> keysOf(const std::vector<float>& boxes, uint32_t count) {
    std::vector<float> c(size_t(count) * 3);
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k) {
            const float v = float(0.5 * double(boxes[size_t(i) * 6 + k]) + 0.5 * double(boxes[size_t(i) * 6 + 3 + k]));
            c[size_t(i) * 3 + k] = v;
            lo[k] = std::fmin(lo[k], v); hi[k] = std::fmax(hi[k], v);
        }
    std::vector<uint64_t> keys(count);
    for (uint32_t i = 0; i < count; ++i) {
        uint64_t field = 0;
        for (int k = 0; k < 3; ++k) {
            uint64_t q = 0;
            if (hi[k] > lo[k]) {
                const double v = std::floor((double(c[size_t(i) * 3 + k]) - double(lo[k])) / (double(hi[k]) - double(lo[k])) * 1024.0);
                q = v > 1023.0 ? 1023u : uint64_t(v);
            }
            for (int bit = 0; bit < 10; ++bit) field |= ((q >> bit) & 1u) << (3 * bit + 2 - k);
        }
        keys[i] = (field << 32) | i;
    }
    return keys;
}

uint32_t boundOf(uint32_t count) {
    uint32_t l = 0;
    while ((1ull << l) < count) ++l;
    const uint32_t byBits = 30 + l, byRecords = count > 1 ? count - 1 : 1;
    return byBits < byRecords ? byBits : byRecords;
}

struct Walk {
    const std::vector<Node>& nodes;
    const std::vector<uint64_t>& sorted;      // the restated keys along `order`
    std::vector<int> recordSeen, positionSeen;
    uint32_t height = 0;
    const char* what;

    // returns the range [a, b] of positions below `ref`
    void below(uint32_t ref, uint32_t expectRecord, uint32_t parent, uint32_t depth, uint32_t& a, uint32_t& b) {
        if (!(ref & 0x80000000u)) {
            const uint32_t p = ref & 0xFFFFFFu;
            CHECK((ref >> 24) == 1u && p < positionSeen.size(), "%s: leaf reference %#x", what, ref);
            if (p < positionSeen.size()) ++positionSeen[p];
            a = b = p;
            return;
        }
        const uint32_t i = ref & 0x7FFFFFFFu;
        CHECK(i < nodes.size() && i == expectRecord, "%s: record %u where the rule numbers %u", what, i, expectRecord);
        if (i >= nodes.size() || recordSeen[i]++) { CHECK(false, "%s: record %u out of range or reached twice", what, i); a = b = 0; return; }
        CHECK(nodes[i].parent == parent && nodes[i].kind == 1u, "%s: record %u: parent %u kind %u", what, i, nodes[i].parent, nodes[i].kind);
        if (depth > height) height = depth;
        // the children's expected records follow from the split, which follows from the first child's range: walk it first
        uint32_t la, lb, ra, rb;
        const uint32_t firstRef = nodes[i].first, lastRef = nodes[i].last;
        const uint32_t split = (firstRef & 0x80000000u) ? (firstRef & 0x7FFFFFFFu) : (firstRef & 0xFFFFFFu);      // record `split` or the leaf of position `split`
        below(firstRef, split, i, depth + 1, la, lb);
        below(lastRef, split + 1, i, depth + 1, ra, rb);
        CHECK(lb == split && ra == split + 1, "%s: record %u: children cover [%u, %u] and [%u, %u]", what, i, la, lb, ra, rb);
        a = la; b = rb;
        if (a < b && b < sorted.size()) {
            const int bit = 63 - __builtin_clzll(sorted[a] ^ sorted[b]);
            CHECK(((sorted[split] >> bit) & 1u) == 0u && ((sorted[split + 1] >> bit) & 1u) == 1u, "%s: record %u over [%u, %u] is not split at bit %d", what, i, a, b, bit);
        }
    }
};

void checkWorld(const char* what, const std::vector<float>& t, const std::vector<float>& rb) {
    const uint32_t count = uint32_t(t.size() / 12), cap = count > 1 ? count - 1 : 1;
    std::vector<float> inv(size_t(count) * 12), boxes(size_t(count) * 6), inv2(inv), boxes2(boxes), inv3(inv), boxes3(boxes);
    std::vector<Node> nodes(cap), nodes2(cap), nodes3(cap);
    std::vector<uint32_t> order(count), order2(count);
    uint32_t nodeCount = 0, height = 0, nodeCount2 = 0, height2 = 0;
    float pad = 0, pad2 = 0, pad3 = 0;
    const int rc = racc_host_world_rebuild(t.data(), rb.data(), count, inv.data(), boxes.data(), &pad, nodes.data(), cap, &nodeCount, order.data(), &height);
    CHECK(rc == RACC_HIP_OK, "%s: rebuild refused: %s", what, racc_hip_last_error());
    if (rc != RACC_HIP_OK) return;
    CHECK(racc_host_world_prepare(t.data(), rb.data(), count, inv2.data(), boxes2.data(), &pad2, nodes2.data(), cap, &nodeCount2, order2.data(), &height2) == RACC_HIP_OK, "%s: prepare refused: %s", what, racc_hip_last_error());
    CHECK(!std::memcmp(inv.data(), inv2.data(), inv.size() * 4) && !std::memcmp(boxes.data(), boxes2.data(), boxes.size() * 4) && !std::memcmp(&pad, &pad2, 4), "%s: inv / world boxes / ray pad differ from prepare", what);
    CHECK(nodeCount == cap, "%s: node_count %u", what, nodeCount);
    if (count == 1) CHECK(!std::memcmp(nodes.data(), nodes2.data(), 64), "%s: a one-instance world is not prepare's", what);

    const std::vector<uint64_t> keys = keysOf(boxes, count);
    std::vector<uint64_t> sorted(count);
    for (uint32_t p = 0; p < count; ++p) sorted[p] = order[p] < count ? keys[order[p]] : 0;
    for (uint32_t p = 0; p + 1 < count; ++p) CHECK(sorted[p] < sorted[p + 1], "%s: keys not ascending at position %u", what, p);
    Walk w{ nodes, sorted, std::vector<int>(cap, 0), std::vector<int>(count, 0), 0, what };
    if (count == 1) {
        CHECK(nodes[0].first == (1u << 24) && nodes[0].last == 0u && height == 1u, "%s: the one-instance root", what);
    } else {
        uint32_t a = 0, b = 0;
        w.below(0x80000000u, 0u, 0xFFFFFFFFu, 1u, a, b);
        CHECK(a == 0 && b == count - 1, "%s: the root covers [%u, %u]", what, a, b);
        for (uint32_t i = 0; i < cap; ++i) CHECK(w.recordSeen[i] == 1, "%s: record %u reached %d times", what, i, w.recordSeen[i]);
        for (uint32_t p = 0; p < count; ++p) CHECK(w.positionSeen[p] == 1, "%s: position %u named %d times", what, p, w.positionSeen[p]);
        CHECK(w.height == height, "%s: reported height %u, walked %u", what, height, w.height);
    }
    CHECK(height <= boundOf(count), "%s: height %u above the bound %u", what, height, boundOf(count));
    std::printf("%s: %u instances, height %u (bound %u)\n", what, count, height, boundOf(count));

    CHECK(racc_host_world_refit(t.data(), rb.data(), count, nodes.data(), cap, order.data(), inv3.data(), boxes3.data(), &pad3, nodes3.data()) == RACC_HIP_OK, "%s: refit of the output refused: %s", what, racc_hip_last_error());
    CHECK(!std::memcmp(nodes3.data(), nodes.data(), size_t(cap) * 64), "%s: the boxes are not racc_host_world_refit's fold", what);
    CHECK(racc_host_world_rebuild(t.data(), rb.data(), count, inv3.data(), boxes3.data(), &pad3, nodes3.data(), cap, &nodeCount2, order2.data(), &height2) == RACC_HIP_OK, "%s: second call refused", what);
    CHECK(!std::memcmp(nodes3.data(), nodes.data(), size_t(cap) * 64) && !std::memcmp(order2.data(), order.data(), size_t(count) * 4) && height2 == height, "%s: two calls differ", what);

    // refusals: nothing is written, the message names the entry
    std::vector<float> invr(inv.size(), -7.0f), boxr(boxes.size(), -7.0f);
    std::vector<Node> nr(cap);
    std::vector<uint32_t> orderr(count, 77u);
    std::memset(nr.data(), 0xAB, size_t(cap) * 64);
    float padr = -7.0f;
    uint32_t ncr = 77, hr = 77;
    auto untouched = [&]() {
        for (float x : invr) if (x != -7.0f) return false;
        for (float x : boxr) if (x != -7.0f) return false;
        for (uint32_t x : orderr) if (x != 77u) return false;
        for (size_t k = 0; k < size_t(cap) * 64; ++k) if (reinterpret_cast<const unsigned char*>(nr.data())[k] != 0xAB) return false;
        return padr == -7.0f && ncr == 77 && hr == 77;
    };
    auto refused = [&](const float* tt, const float* bb, uint32_t n, uint32_t capacity, const char* why) {
        const int r = racc_host_world_rebuild(tt, bb, n, invr.data(), boxr.data(), &padr, nr.data(), capacity, &ncr, orderr.data(), &hr);
        CHECK(r == RACC_HIP_ERR_INVALID && untouched(), "%s: %s accepted or outputs written", what, why);
        CHECK(std::strstr(racc_hip_last_error(), "racc_host_world_rebuild") != nullptr, "%s: the message does not name the entry: %s", why, racc_hip_last_error());
    };
    std::vector<float> bad(t);
    for (int k = 0; k < 12; ++k) bad[size_t(count - 1) * 12 + k] = 0.0f;
    refused(bad.data(), rb.data(), count, cap, "a zero transform");
    bad = t; bad[5] = NAN;
    refused(bad.data(), rb.data(), count, cap, "a NaN coefficient");
    std::vector<float> badBox(rb);
    badBox[0] = 2.0f; badBox[3] = 1.0f;
    refused(t.data(), badBox.data(), count, cap, "an inverted root box");
    refused(t.data(), rb.data(), 0, cap, "count 0");
    refused(nullptr, rb.data(), count, cap, "NULL transforms");
    if (count > 2) refused(t.data(), rb.data(), count, cap - 1, "a short node_capacity");
}

std::vector<float> randomBoxes(uint32_t count) {
    std::vector<float> rb(size_t(count) * 6);
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k) { rb[size_t(i) * 6 + k] = float(range(-10, 10)); rb[size_t(i) * 6 + 3 + k] = rb[size_t(i) * 6 + k] + (uniform() < 0.1 ? 0.0f : float(range(0, 5))); }
    return rb;
}

std::vector<float> unitBoxes(size_t count) {
    std::vector<float> rb(count * 6);
    for (size_t i = 0; i < count; ++i) for (int k = 0; k < 3; ++k) { rb[i * 6 + k] = -1.0f; rb[i * 6 + 3 + k] = 1.0f; }
    return rb;
}

}  // namespace

int main() {
    int rebuilds = 0;
    std::vector<float> t;
    for (uint32_t count : { 1u, 2u, 3u, 257u, 1000u }) { randomTransforms(t, count, 100.0); checkWorld("random", t, randomBoxes(count)); ++rebuilds; }
    translations(t, std::vector<double>(1000, 3.0));
    checkWorld("one centre", t, unitBoxes(1000)); ++rebuilds;
    std::vector<double> x;
    for (int k = 0; k <= 30; ++k) x.push_back(std::ldexp(4096.0, -k));
    translations(t, x);
    checkWorld("chain", t, unitBoxes(x.size())); ++rebuilds;
    x.insert(x.end(), 200, std::ldexp(4096.0, -30));
    translations(t, x);
    checkWorld("chain and crowd", t, unitBoxes(x.size())); ++rebuilds;
    std::printf("%d rebuilds checked, %d failures\n", rebuilds, g_failures);
    return g_failures ? 1 : 0;
}
