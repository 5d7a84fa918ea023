// scene_rebuild_host_check — stand-alone driver of racc_host_scene_rebuild (rayaccel_amd/csrc/scene_rebuild.cpp) and of the rule header's
// device-side text (racc_scene_rebuild_rule.h: field, hierarchyStep) for the AddressSanitizer + UBSan build (`make asan`).
//   1. The host function on random meshes of 2, 3, 4, 5, 31, 32, 33 and 1000 triangles, 1000 triangles with one centre, 300 on one axis,
//      duplicated triangles and the chain of 40.  Per mesh: the counts; remap a permutation with ascending keys; racc_host_blobs_refit of
//      the output to its own vertices as bytes; every node reached once, every position named once, the height against a walk and the
//      bound; and — the device's formulation against the host's — hierarchyStep over the sorted keys reproduces every node's first / last
//      and parent.  Its refusals leave the outputs untouched.
//   2. racc_scene_rebuild_rule::quantise / field on NaN, +-inf, denormals, +-FLT_MAX, zeros in every role: always in [0, 2^21) / [0, 2^63).
//   3. hierarchyStep over sorted, all-equal, reversed and random key arrays of 2 .. 257 entries.  Every array goes through an accessor that
//      checks its index, and every index the step returns is checked against [0, n): the sanitised evidence that the device kernel, which
//      runs the same text, cannot leave its arrays whatever the keys hold.
// Exit code 0 = all good; the sanitizers abort on their own findings.
#include "racc_hip.h"
#include "racc_scene_rebuild_rule.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

namespace rule = racc_scene_rebuild_rule;
struct Node { uint32_t kind, parent, first, last; float box[12]; };

uint64_t g_state = 0x243F6A8885A308D3ull;
uint64_t next64() { g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27; return g_state * 0x2545F4914F6CDD1Dull; }
double uniform() { return double(next64() >> 11) / 9007199254740992.0; }
double range(double a, double b) { return a + (b - a) * uniform(); }

int g_failures = 0, g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_failures < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// an array that checks every index it is asked for
template <class T> struct Checked {
    const std::vector<T>& v;
    T operator[](int i) const {
        if (i < 0 || size_t(i) >= v.size()) { std::printf("FAILED: index %d outside [0, %zu)\n", i, v.size()); std::abort(); }
        return v[size_t(i)];
    }
};

struct Mesh { std::vector<float> v; std::vector<uint32_t> idx; const char* name; };

Mesh soup(uint32_t T, const char* name) {
    Mesh m; m.name = name;
    for (uint32_t t = 0; t < T; ++t) {
        const double c[3] = { range(-4, 4), range(-4, 4), range(-4, 4) };
        for (int k = 0; k < 3; ++k) { for (int a = 0; a < 3; ++a) m.v.push_back(float(c[a] + range(-1.5, 1.5))); m.v.push_back(0.0f); m.idx.push_back(t * 3 + uint32_t(k)); }
    }
    return m;
}
Mesh commonCentre(uint32_t T) {
    Mesh m; m.name = "one centre";
    const float corners[3][3] = { {-1, -1, -1}, {1, 1, 1}, {1, -1, 0} }, c[3] = { 3, -2, 5 };
    for (uint32_t t = 0; t < T; ++t) {
        const float s = 1.0f + float(t) / 4096.0f;
        for (int k = 0; k < 3; ++k) { for (int a = 0; a < 3; ++a) m.v.push_back(c[a] + s * corners[k][a]); m.v.push_back(0.0f); m.idx.push_back(t * 3 + uint32_t(k)); }
    }
    return m;
}
Mesh oneAxis(uint32_t T) {
    Mesh m; m.name = "one axis";
    const float base[3][3] = { {0, 0, 0}, {0, 1, 0}, {0, 0, 1} };
    for (uint32_t t = 0; t < T; ++t) {
        const float x = float(range(-50, 50));
        for (int k = 0; k < 3; ++k) { m.v.push_back(x); m.v.push_back(base[k][1]); m.v.push_back(base[k][2]); m.v.push_back(0.0f); m.idx.push_back(t * 3 + uint32_t(k)); }
    }
    return m;
}
Mesh duplicated(uint32_t quarter) {
    Mesh m = soup(quarter, "duplicated");
    const std::vector<uint32_t> once = m.idx;
    for (int rep = 0; rep < 3; ++rep) m.idx.insert(m.idx.end(), once.begin(), once.end());
    const uint32_t T = uint32_t(m.idx.size() / 3);
    for (uint32_t t = T - 1; t > 0; --t) {      // shuffle the triples
        const uint32_t o = uint32_t(next64() % (t + 1));
        for (int k = 0; k < 3; ++k) std::swap(m.idx[size_t(t) * 3 + k], m.idx[size_t(o) * 3 + k]);
    }
    return m;
}
Mesh chain(uint32_t length) {
    Mesh m; m.name = "chain";
    const float yz[3][2] = { {-0.25f, -0.25f}, {0.5f, -0.25f}, {-0.25f, 0.5f} };
    for (uint32_t t = 0; t < length; ++t)
        for (int k = 0; k < 3; ++k) { m.v.push_back(std::ldexp(1.0f, -int(t))); m.v.push_back(yz[k][0]); m.v.push_back(yz[k][1]); m.v.push_back(0.0f); m.idx.push_back(t * 3 + uint32_t(k)); }
    return m;
}

// the sorted keys by the rule's own functions (what the device forms), in a formulation of its own: fields, then std::stable_sort by field
void keysOf(const Mesh& m, std::vector<uint64_t>& fields, std::vector<uint32_t>& order) {
    const uint32_t T = uint32_t(m.idx.size() / 3);
    std::vector<float> c(size_t(T) * 3);
    float lo[3], hi[3];
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t* a = &m.idx[size_t(t) * 3];
        rule::triangleCentre(&m.v[size_t(a[0]) * 4], &m.v[size_t(a[1]) * 4], &m.v[size_t(a[2]) * 4], &c[size_t(t) * 3]);
        for (int k = 0; k < 3; ++k) { if (!t || c[size_t(t) * 3 + k] < lo[k]) lo[k] = c[size_t(t) * 3 + k]; if (!t || c[size_t(t) * 3 + k] > hi[k]) hi[k] = c[size_t(t) * 3 + k]; }
    }
    std::vector<uint64_t> f(T);
    for (uint32_t t = 0; t < T; ++t) f[t] = rule::field(&c[size_t(t) * 3], lo, hi);
    order.resize(T);
    for (uint32_t t = 0; t < T; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return f[x] < f[y]; });      // (as the radix sort: stable, index order in)
    fields.resize(T);
    for (uint32_t p = 0; p < T; ++p) fields[p] = f[order[p]];
}

uint32_t walk(const std::vector<Node>& nodes, uint32_t T, const char* name) {
    std::vector<int> seenNode(nodes.size(), 0), seenPos(T, 0);
    std::vector<std::pair<uint32_t, uint32_t>> todo{ {0u, 1u} };
    seenNode[0] = 1;
    uint32_t height = 0;
    while (!todo.empty()) {
        const auto [n, depth] = todo.back();
        todo.pop_back();
        height = std::max(height, depth);
        for (uint32_t ref : { nodes[n].first, nodes[n].last }) {
            if (ref & 0x80000000u) {
                const uint32_t c = ref & 0x7FFFFFFFu;
                CHECK(c > 0 && c < nodes.size(), "%s: child %u out of range", name, c);
                if (c >= nodes.size()) continue;
                CHECK(nodes[c].parent == n, "%s: node %u has parent %u, is a child of %u", name, c, nodes[c].parent, n);
                if (!seenNode[c]++) todo.emplace_back(c, depth + 1);
            } else {
                CHECK((ref >> 24) == 1u && (ref & 0xFFFFFFu) < T, "%s: leaf %08x", name, ref);
                if ((ref & 0xFFFFFFu) < T) ++seenPos[ref & 0xFFFFFFu];
            }
        }
    }
    for (int s : seenNode) CHECK(s == 1, "%s: a node is reached %d times", name, s);
    for (int s : seenPos) CHECK(s == 1, "%s: a position is named %d times", name, s);
    return height;
}

void checkMesh(const Mesh& m) {
    const uint32_t T = uint32_t(m.idx.size() / 3), V = uint32_t(m.v.size() / 4), padded = rule::paddedPairs(T);
    std::vector<Node> nodes(T - 1);
    std::vector<float> pairs(size_t(padded) * 12);
    std::vector<uint32_t> remap(size_t(T) * 2);
    uint32_t nn = 0, np = 0, nr = 0, height = 0;
    const int rc = racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), uint32_t(m.idx.size()), nodes.data(), T - 1, &nn, pairs.data(), padded, &np, remap.data(), T * 2, &nr, &height);
    CHECK(rc == 0, "%s: rc %d (%s)", m.name, rc, racc_hip_last_error());
    if (rc) return;
    CHECK(nn == T - 1 && np == padded && nr == 2 * T && padded % 32 == 0 && padded > T && padded - T <= 32, "%s: counts %u %u %u", m.name, nn, np, nr);
    std::vector<uint64_t> fields;
    std::vector<uint32_t> order;
    keysOf(m, fields, order);
    for (uint32_t p = 0; p < T; ++p) CHECK(remap[2 * p] == order[p] && remap[2 * p + 1] == 0u, "%s: remap[%u] = %u, %u; the sorted keys have triangle %u", m.name, 2 * p, remap[2 * p], remap[2 * p + 1], order[p]);
    for (uint32_t p = 0; p + 1 < T; ++p) CHECK(fields[p] < fields[p + 1] || (fields[p] == fields[p + 1] && order[p] < order[p + 1]), "%s: keys not ascending at %u", m.name, p);
    CHECK(std::memcmp(&pairs[size_t(T) * 12], &pairs[0], 48) == 0 && std::memcmp(&pairs[size_t(padded - 1) * 12], &pairs[0], 48) == 0, "%s: padding is not pair 0", m.name);
    const uint32_t walked = walk(nodes, T, m.name);
    CHECK(walked == height && height <= rule::heightBound(T), "%s: height %u, walk %u, bound %u", m.name, height, walked, rule::heightBound(T));
    for (const Node& n : nodes) CHECK(n.kind == 1u, "%s: kind %u", m.name, n.kind);
    CHECK(nodes[0].parent == 0xFFFFFFFFu, "%s: root parent", m.name);
    // the device's formulation over the same keys
    const Checked<uint64_t> cf{ fields };
    const Checked<uint32_t> co{ order };
    for (uint32_t i = 0; i + 1 < T; ++i) {
        const rule::HierarchyStep s = rule::hierarchyStep(cf, co, int(T), int(i));
        CHECK(s.word[0] == nodes[i].first && s.word[1] == nodes[i].last, "%s: node %u is %08x %08x, hierarchyStep gives %08x %08x", m.name, i, nodes[i].first, nodes[i].last, s.word[0], s.word[1]);
        for (int side = 0; side < 2; ++side) {
            CHECK(s.target[side] < T && (s.leaf[side] || (s.target[side] >= 1u && s.target[side] + 1u < T)), "%s: node %u side %d names %u", m.name, i, side, s.target[side]);
            CHECK((s.word[side] & 0xFFFFFFu) == s.target[side] || (s.word[side] & 0x7FFFFFFFu) == s.target[side], "%s: word and target differ", m.name);
        }
    }
    // a refit of the output to its own vertices is the identity
    std::vector<Node> nodes2(T - 1);
    std::vector<float> pairs2(pairs.size());
    const int rr = racc_host_blobs_refit(nodes.data(), T - 1, pairs.data(), padded, T, remap.data(), 2 * T, m.v.data(), V, m.idx.data(), uint32_t(m.idx.size()), nodes2.data(), pairs2.data());
    CHECK(rr == 0, "%s: refit rc %d (%s)", m.name, rr, racc_hip_last_error());
    CHECK(std::memcmp(nodes.data(), nodes2.data(), nodes.size() * 64) == 0, "%s: the refit changes the nodes", m.name);
    CHECK(std::memcmp(pairs.data(), pairs2.data(), pairs.size() * 4) == 0, "%s: the refit changes the pairs", m.name);
    // twice the same
    std::vector<Node> again(T - 1);
    racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), uint32_t(m.idx.size()), again.data(), T - 1, &nn, pairs2.data(), padded, &np, remap.data(), T * 2, &nr, &height);
    CHECK(std::memcmp(nodes.data(), again.data(), nodes.size() * 64) == 0, "%s: two calls differ", m.name);
    std::printf("%-12s T = %4u  height %2u (bound %2u)\n", m.name, T, height, rule::heightBound(T));
}

void checkRefusals() {
    const Mesh m = soup(5, "refusals");
    std::vector<Node> nodes(4);
    std::vector<float> pairs(32 * 12, -7.0f);
    std::vector<uint32_t> remap(10, 77u);
    std::memset(nodes.data(), 0x5A, 4 * 64);
    uint32_t nn = 77, np = 77, nr = 77, h = 77;
    auto untouched = [&](const char* what, int rc, int want) {
        CHECK(rc == want && std::strstr(racc_hip_last_error(), "racc_host_scene_rebuild"), "%s: rc %d (%s)", what, rc, racc_hip_last_error());
        bool clean = nn == 77 && np == 77 && nr == 77 && h == 77;
        for (float f : pairs) clean = clean && f == -7.0f;
        for (uint32_t r : remap) clean = clean && r == 77u;
        for (size_t i = 0; i < 4 * 64; ++i) clean = clean && reinterpret_cast<const unsigned char*>(nodes.data())[i] == 0x5A;
        CHECK(clean, "%s: an output was written", what);
    };
    const uint32_t V = 15, I = 15;
    untouched("NULL vertices", racc_host_scene_rebuild(nullptr, V, m.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    untouched("NULL height", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, nullptr), RACC_HIP_ERR_INVALID);
    untouched("index_count % 3", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), 14, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    untouched("one triangle", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), 3, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    untouched("2^24 triangles", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), 3u << 24, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_LIMIT);
    untouched("index out of range", racc_host_scene_rebuild(m.v.data(), 14, m.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    for (float bad : { NAN, INFINITY, -INFINITY }) {
        Mesh b = m; b.v[4 * 7 + 2] = bad;
        untouched("not finite", racc_host_scene_rebuild(b.v.data(), V, b.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    }
    untouched("node capacity", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), I, nodes.data(), 3, &nn, pairs.data(), 32, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    untouched("pair capacity", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 31, &np, remap.data(), 10, &nr, &h), RACC_HIP_ERR_INVALID);
    untouched("remap capacity", racc_host_scene_rebuild(m.v.data(), V, m.idx.data(), I, nodes.data(), 4, &nn, pairs.data(), 32, &np, remap.data(), 9, &nr, &h), RACC_HIP_ERR_INVALID);
}

void checkField() {
    const float denormal = std::ldexp(1.0f, -149);
    const float special[] = { NAN, -NAN, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX, denormal, -denormal, FLT_MIN, -FLT_MIN, 0.0f, -0.0f, 1.0f, -1.0f, 3.0e38f, 1e-30f };
    const size_t n = sizeof(special) / sizeof(special[0]);
    for (size_t a = 0; a < n; ++a)
        for (size_t b = 0; b < n; ++b)
            for (size_t c = 0; c < n; ++c) {
                const uint32_t q = rule::quantise(special[a], special[b], special[c]);
                CHECK(q < (1u << 21), "quantise(%g, %g, %g) = %u", special[a], special[b], special[c], q);
                const float cc[3] = { special[a], special[b], special[c] }, lo[3] = { special[b], special[c], special[a] }, hi[3] = { special[c], special[a], special[b] };
                CHECK(rule::field(cc, lo, hi) < (1ull << 63), "field out of range");
            }
    for (int i = 0; i < 200000; ++i) {      // any bits whatever
        float f[3];
        for (float& x : f) { const uint32_t bits = uint32_t(next64()); std::memcpy(&x, &bits, 4); }
        CHECK(rule::quantise(f[0], f[1], f[2]) < (1u << 21), "quantise of random bits out of range");
    }
    CHECK(rule::quantise(1.0f, 0.0f, 1.0f) == (1u << 21) - 1u && rule::quantise(0.0f, 0.0f, 1.0f) == 0u && rule::quantise(0.5f, 0.0f, 1.0f) == (1u << 20), "quantise end points");
    CHECK(rule::spread3(0x1FFFFFu) == 0x1249249249249249ull && rule::spread3(1u << 20) == (1ull << 60), "spread3");
}

void checkStepOnArbitraryKeys() {
    for (int n = 2; n <= 257; ++n)
        for (int kind = 0; kind < 6; ++kind) {
            std::vector<uint64_t> f(size_t(n), 0);
            std::vector<uint32_t> o(size_t(n), 0);
            for (int i = 0; i < n; ++i) {
                switch (kind) {
                case 0: f[size_t(i)] = uint64_t(i) * 0x0003000300030003ull & 0x7FFFFFFFFFFFFFFFull; o[size_t(i)] = uint32_t(i); break;      // sorted by field
                case 1: f[size_t(i)] = 42; o[size_t(i)] = uint32_t(i); break;                                                              // sorted by index alone
                case 2: f[size_t(i)] = 42; o[size_t(i)] = 7; break;                                                                        // all equal
                case 3: f[size_t(i)] = uint64_t(n - i) << 20; o[size_t(i)] = uint32_t(n - i); break;                                       // reversed
                case 4: f[size_t(i)] = next64(); o[size_t(i)] = uint32_t(next64()); break;                                                 // random, bit 63 included
                default: f[size_t(i)] = next64() & 3u; o[size_t(i)] = uint32_t(next64() & 3u); break;                                      // random with many duplicates
                }
            }
            const Checked<uint64_t> cf{ f };
            const Checked<uint32_t> co{ o };
            std::vector<uint32_t> parent(size_t(n), 0), slot(size_t(n), 0);      // the device's tables: n entries each
            for (int i = 0; i + 1 < n; ++i) {
                const rule::HierarchyStep s = rule::hierarchyStep(cf, co, n, i);
                for (int side = 0; side < 2; ++side) {
                    CHECK(s.target[side] < uint32_t(n), "n %d kind %d node %d side %d: target %u", n, kind, i, side, s.target[side]);
                    if (s.target[side] >= uint32_t(n)) continue;
                    (s.leaf[side] ? slot : parent).at(s.target[side]) = uint32_t(i) * 2u + uint32_t(side);
                    CHECK((s.word[side] & (s.leaf[side] ? 0xFFFFFFu : 0x7FFFFFFFu)) == s.target[side] && ((s.word[side] >> 31) == (s.leaf[side] ? 0u : 1u)), "n %d kind %d: word %08x", n, kind, s.word[side]);
                }
            }
            if (kind < 2) {      // sorted unique keys: a tree
                std::vector<int> seen(size_t(n), 0);
                for (int i = 0; i + 1 < n; ++i) {
                    const rule::HierarchyStep s = rule::hierarchyStep(cf, co, n, i);
                    for (int side = 0; side < 2; ++side) if (s.leaf[side]) ++seen[s.target[side]];
                }
                for (int s : seen) CHECK(s == 1, "n %d kind %d: a position is a leaf %d times", n, kind, s);
            }
        }
}

}  // namespace

int main() {
    for (uint32_t T : { 2u, 3u, 4u, 5u, 31u, 32u, 33u, 1000u }) checkMesh(soup(T, "random"));
    checkMesh(commonCentre(1000));
    checkMesh(oneAxis(300));
    checkMesh(duplicated(100));
    checkMesh(chain(40));
    checkRefusals();
    checkField();
    checkStepOnArbitraryKeys();
    std::printf("%d checks passed, %d failures\n", g_checks - g_failures, g_failures);
    return g_failures ? 1 : 0;
}
