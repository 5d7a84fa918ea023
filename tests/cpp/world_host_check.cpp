// world_host_check — stand-alone driver of racc_host_world_prepare (rayaccel_amd/csrc/world_build.cpp) for the AddressSanitizer + UBSan
// build (`make asan`): a few hundred random and degenerate worlds — flat boxes, negative scale, mirrors, coincident instances, one
// instance — each checked with code of its own: inv . M = identity in double, every world box contains the eight transformed corners,
// the tree reaches every instance exactly once and every child box contains what is below it; a second run gives the same bytes; the
// refusals refuse and leave the outputs untouched.  Exit code 0 = all good; the sanitizers abort on their own findings.
#include "racc_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Node { uint32_t kind, parent, first, last; float box[12]; };

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform() {      // xorshift64*, [0, 1)
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return double((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
double range(double a, double b) { return a + (b - a) * uniform(); }

struct World {
    uint32_t count = 0;
    std::vector<float> transforms, rootBoxes, inv, boxes;
    std::vector<Node> nodes;
    std::vector<uint32_t> order;
    uint32_t nodeCount = 0, height = 0;
    float rayPad = 0.0f;
};

int prepare(World& w) {
    const uint32_t cap = w.count > 1 ? w.count - 1 : 1;
    w.inv.assign(size_t(w.count) * 12, -7.0f); w.boxes.assign(size_t(w.count) * 6, -7.0f);
    w.nodes.assign(cap, Node{}); w.order.assign(w.count, 0xABABABABu);
    return racc_host_world_prepare(w.transforms.data(), w.rootBoxes.data(), w.count, w.inv.data(), w.boxes.data(), &w.rayPad,
                                   w.nodes.data(), cap, &w.nodeCount, w.order.data(), &w.height);
}

void makeWorld(World& w, uint32_t count, int flavour) {
    w.count = count;
    w.transforms.resize(size_t(count) * 12); w.rootBoxes.resize(size_t(count) * 6);
    for (uint32_t i = 0; i < count; ++i) {
        float* m = &w.transforms[size_t(i) * 12];
        // rotation about a random axis (Rodrigues), then scale per flavour
        double ax[3] = { range(-1, 1), range(-1, 1), range(-1, 1) };
        double len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        if (len < 1e-3) { ax[0] = 1; ax[1] = ax[2] = 0; len = 1; }
        for (double& a : ax) a /= len;
        const double ang = range(0, 6.283185307179586), c = std::cos(ang), s = std::sin(ang);
        double R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) R[r][k] = (r == k ? c : 0.0) + (1 - c) * ax[r] * ax[k];
        R[0][1] -= s * ax[2]; R[0][2] += s * ax[1]; R[1][0] += s * ax[2]; R[1][2] -= s * ax[0]; R[2][0] -= s * ax[1]; R[2][1] += s * ax[0];
        double sc[3] = { range(0.2, 4), range(0.2, 4), range(0.2, 4) };
        if (flavour == 1) for (double& x : sc) x = -x;                                  // negative scale
        if (flavour == 2) sc[int(uniform() * 3) % 3] *= -1;                             // a mirror
        if (flavour == 3) { sc[0] = 1e-4; sc[1] = 1e3; }                                // badly conditioned
        if (flavour == 4) { for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R[r][k] = r == k; sc[0] = sc[1] = sc[2] = 1; }      // identity, coincident
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) m[r * 4 + k] = float(R[r][k] * sc[k]);
            m[r * 4 + 3] = flavour == 4 ? 0.0f : float(range(-100, 100));
        }
        float* b = &w.rootBoxes[size_t(i) * 6];
        for (int k = 0; k < 3; ++k) {
            b[k] = float(range(-10, 10));
            const bool flat = flavour == 5 || uniform() < 0.1;                          // flat boxes (flavour 5: points)
            b[3 + k] = flat ? b[k] : b[k] + float(range(0, 5));
        }
    }
}

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_failures < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// box of everything below `ref`, checked against the parents' child boxes on the way
bool below(const World& w, uint32_t ref, uint32_t parent, uint32_t depth, std::vector<uint32_t>& nodeSeen, std::vector<uint32_t>& instSeen, uint32_t& height, float out[6]) {
    if (ref & 0x80000000u) {
        const uint32_t i = ref & 0x7FFFFFFFu;
        if (i >= w.nodeCount) { CHECK(false, "child %u out of range", i); return false; }
        if (++nodeSeen[i] != 1) { CHECK(false, "node %u reached twice", i); return false; }
        const Node& n = w.nodes[i];
        CHECK(n.parent == parent && n.kind >= 1 && n.kind <= 3, "node %u: kind %u parent %u", i, n.kind, n.parent);
        if (depth > height) height = depth;
        float l[6], r[6];
        const bool hl = below(w, n.first, i, depth + 1, nodeSeen, instSeen, height, l), hr = below(w, n.last, i, depth + 1, nodeSeen, instSeen, height, r);
        for (int k = 0; k < 3; ++k) {
            if (hl) CHECK(n.box[k] <= l[k] && l[3 + k] <= n.box[3 + k], "node %u: left box does not contain its subtree", i);
            if (hr) CHECK(n.box[6 + k] <= r[k] && r[3 + k] <= n.box[9 + k], "node %u: right box does not contain its subtree", i);
        }
        if (!hl && !hr) return false;
        for (int k = 0; k < 3; ++k) {
            out[k] = !hr ? l[k] : (!hl ? r[k] : std::fmin(l[k], r[k]));
            out[3 + k] = !hr ? l[3 + k] : (!hl ? r[3 + k] : std::fmax(l[3 + k], r[3 + k]));
        }
        return true;
    }
    const uint32_t first = ref & 0xFFFFFFu, cnt = ref >> 24;
    if (cnt == 0) { CHECK(w.count == 1 && ref == 0, "an empty leaf outside a one-instance world"); return false; }
    if (first + cnt > w.count) { CHECK(false, "leaf range out of bounds"); return false; }
    for (uint32_t j = first; j < first + cnt; ++j) {
        const uint32_t id = w.order[j];
        if (id >= w.count) { CHECK(false, "order[%u] = %u out of range", j, id); return false; }
        ++instSeen[id];
        const float* b = &w.boxes[size_t(id) * 6];
        for (int k = 0; k < 6; ++k) out[k] = (j == first) ? b[k] : (k < 3 ? std::fmin(out[k], b[k]) : std::fmax(out[k], b[k]));
    }
    return true;
}

void checkWorld(const World& w, const char* what) {
    for (uint32_t i = 0; i < w.count; ++i) {
        const float* m = &w.transforms[size_t(i) * 12];
        const float* v = &w.inv[size_t(i) * 12];
        double worst = 0.0, scale = 0.0;      // inv . M against the identity, relative to |inv| |M|
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 4; ++k) {
                double sum = k == 3 ? double(v[r * 4 + 3]) : 0.0, mag = std::fabs(sum);
                for (int j = 0; j < 3; ++j) { sum += double(v[r * 4 + j]) * double(m[j * 4 + k]); mag += std::fabs(double(v[r * 4 + j]) * double(m[j * 4 + k])); }
                worst = std::fmax(worst, std::fabs(sum - (r == k ? 1.0 : 0.0)));
                scale = std::fmax(scale, mag);
            }
        CHECK(worst <= 4e-7 * std::fmax(scale, 1.0), "%s: instance %u: inv . M is off the identity by %g (scale %g)", what, i, worst, scale);
        const float* rb = &w.rootBoxes[size_t(i) * 6];
        const float* wb = &w.boxes[size_t(i) * 6];
        for (int corner = 0; corner < 8; ++corner)
            for (int r = 0; r < 3; ++r) {
                double q = m[r * 4 + 3];
                for (int k = 0; k < 3; ++k) q += double(m[r * 4 + k]) * double(rb[k + 3 * ((corner >> k) & 1)]);
                CHECK(double(wb[r]) <= q && q <= double(wb[3 + r]), "%s: instance %u: corner %d outside its world box on axis %d", what, i, corner, r);
            }
    }
    CHECK(w.nodeCount == (w.count > 1 ? w.count - 1 : 1), "%s: %u nodes for %u instances", what, w.nodeCount, w.count);
    std::vector<uint32_t> nodeSeen(w.nodeCount, 0), instSeen(w.count, 0);
    uint32_t height = 0;
    float all[6];
    below(w, 0x80000000u, 0xFFFFFFFFu, 1, nodeSeen, instSeen, height, all);
    for (uint32_t s : nodeSeen) CHECK(s == 1, "%s: a node is unreachable", what);
    for (uint32_t s : instSeen) CHECK(s == 1, "%s: an instance is in %u leaves", what, s);
    CHECK(height == w.height, "%s: height %u reported, %u found", what, w.height, height);
    CHECK(w.rayPad > 0.0f && std::isfinite(w.rayPad), "%s: ray pad %g", what, w.rayPad);
}

bool untouched(const World& w) {
    for (float x : w.inv) if (x != -7.0f) return false;
    for (float x : w.boxes) if (x != -7.0f) return false;
    for (uint32_t x : w.order) if (x != 0xABABABABu) return false;
    return true;
}

}  // namespace

int main() {
    const uint32_t sizes[] = { 1, 2, 3, 4, 5, 17, 64, 255, 1000 };
    int worlds = 0;
    for (int round = 0; round < 6; ++round)
        for (int flavour = 0; flavour < 6; ++flavour)
            for (uint32_t count : sizes) {
                if (count == 1000 && round > 0) continue;
                World w;
                makeWorld(w, count, flavour);
                char what[64];
                std::snprintf(what, sizeof(what), "flavour %d, %u instances", flavour, count);
                const int rc = prepare(w);
                CHECK(rc == RACC_HIP_OK, "%s: refused: %s", what, racc_hip_last_error());
                if (rc != RACC_HIP_OK) continue;
                checkWorld(w, what);
                World again = w;
                CHECK(prepare(again) == RACC_HIP_OK, "%s: second run refused", what);
                CHECK(!std::memcmp(again.inv.data(), w.inv.data(), w.inv.size() * 4) && !std::memcmp(again.boxes.data(), w.boxes.data(), w.boxes.size() * 4) &&
                      !std::memcmp(again.nodes.data(), w.nodes.data(), size_t(w.nodeCount) * 64) && !std::memcmp(again.order.data(), w.order.data(), w.order.size() * 4) &&
                      again.rayPad == w.rayPad && again.height == w.height, "%s: two runs differ", what);
                ++worlds;
            }
    // refusals: nothing is written
    {
        World w;
        makeWorld(w, 5, 0);
        const std::vector<float> good = w.transforms;
        w.transforms[12 + 7] = NAN;
        CHECK(prepare(w) == RACC_HIP_ERR_INVALID && untouched(w), "NaN coefficient accepted or outputs written");
        w.transforms = good; w.transforms[24 + 2] = INFINITY;
        CHECK(prepare(w) == RACC_HIP_ERR_INVALID && untouched(w), "infinite coefficient accepted or outputs written");
        w.transforms = good; for (int k = 0; k < 3; ++k) { w.transforms[36 + k] = w.transforms[36 + 4 + k] = float(k + 1); w.transforms[36 + 8 + k] = float(k + 4); }      // two equal rows of small integers: exactly zero
        CHECK(prepare(w) == RACC_HIP_ERR_INVALID && untouched(w), "singular transform accepted or outputs written");
        w.transforms = good; for (int k = 0; k < 12; ++k) w.transforms[48 + k] = 0.0f;
        CHECK(prepare(w) == RACC_HIP_ERR_INVALID && untouched(w), "zero transform accepted or outputs written");
        w.transforms = good;
        const uint32_t keep = w.count;
        w.count = 0;
        CHECK(racc_host_world_prepare(w.transforms.data(), w.rootBoxes.data(), 0, w.inv.data(), w.boxes.data(), &w.rayPad, w.nodes.data(), 4, &w.nodeCount, w.order.data(), &w.height) == RACC_HIP_ERR_INVALID, "count 0 accepted");
        CHECK(racc_host_world_prepare(w.transforms.data(), w.rootBoxes.data(), (1u << 20) + 1u, w.inv.data(), w.boxes.data(), &w.rayPad, w.nodes.data(), 4, &w.nodeCount, w.order.data(), &w.height) == RACC_HIP_ERR_INVALID, "2^20 + 1 instances accepted");
        w.count = keep;
        CHECK(prepare(w) == RACC_HIP_OK, "the good world is refused after the refusals");
    }
    std::printf("%d worlds checked, %d failures\n", worlds, g_failures);
    return g_failures ? 1 : 0;
}
