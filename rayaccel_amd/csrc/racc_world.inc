// racc_world.inc — instancing: two-level scenes with per-instance transforms.  worldIntersectKernel and the C-ABI entries around it
// (racc_hip_world_*); the any-hit query on worlds, worldOccludedKernel, is racc_world_occlusion.inc behind this file, on the helpers
// here.  Textually included by racc_hip_unit.hip BEHIND racc_hip.hip, racc_scene_registry.inc and racc_query.inc, so it sees
// the context, the scenes' device pointers and owners, fail() / HIP_TRY / checkWatchdog, the helpers of racc_device.inc and the query
// scaffold, and changes none of them.  The reference has no instancing (one flattened scene, Scene.cpp:216-349); Embree's
// RTC_GEOMETRY_TYPE_INSTANCE is the usual counterpart.
//
// Contract (include/racc_hip.h): a world is an ordered list of (3x4 object-to-world transform, uploaded scene).  With inv the float-rounded
// double-precision inverse (world_build.cpp), instance i sees the ray o' = inv (o, 1), d' = inv (d, 0) — each component the plain float
// expression ((m0 x + m1 y) + m2 z) + m3, no contraction — with the ray's own minT and maxT, and its result h_i is exactly what the
// closest-hit path reports for that ray on that scene: the reference's visiting order inside the bottom level (node rule as in
// racc_kernel_v8.inc's C++ iteration / oracle/racc_oracle.c, slabPair and pairIntersectData of racc_device.inc, tFar shrinking with every
// accepted pair), started with the ray's own maxT whatever other instances have reported.  The world result is the h_i of smallest t,
// exact ties to the lowest instance index: independent of the order in which instances are visited.
//
// The one optimisation: the top-level tree is walked with the best t so far, and a node or instance whose padded box the ray misses in
// [minT, best] is never entered.  The boxes are conservative by construction (world_build.cpp explains the bound): what the host adds per
// instance, plus rayPad (|ox| + |oy| + |oz|) added here on every side of every box, and the interval's end widened by 2^-20 of itself —
// an instance that could still report t <= best is always entered, so no record can change.
//
// Structure (plain HIP): the wavefront scaffold of racc_query.inc — the same ray feed, lane stack, BVH2 inner step and stream-ordered
// scratch as occludedKernel.  A lane is either at the top level (`inst` = none; `node` = a top-level reference) or inside an instance
// (`inst` = its index; `node` = a reference into that scene's BVH2 records).  Each scheduling iteration the wave votes for ONE of three
// steps: a pair step (every lane at a bottom-level leaf tests one pair), a bottom-level inner step, or a top-level step (inner node: box
// tests; leaf: transform the ray and enter the instance).  Two lane stacks: the top-level one survives an instance's traversal, the
// bottom-level one is empty at every entry.

namespace {

constexpr int kWorldBlock = 256;
constexpr int kWorldTopLds = 8;               // top-level stack levels in LDS (8 KB per workgroup)
constexpr int kWorldBotLds = 12;              // bottom-level stack levels in LDS (12 KB per workgroup), as occludedKernel
constexpr uint32_t kWorldWavesPerSimd = 5;    // grid: this many workgroups of four waves per CU (`make resources`: 84 VGPRs, 20 KB of LDS per workgroup: five fit)
constexpr uint32_t kWorldRefillMin = 16;      // idle lanes that trigger a refill
constexpr uint32_t kWorldLeafMin = 10;        // bottom-level leaf lanes that trigger a pair step
constexpr uint32_t kWorldNoInst = 0xFFFFFFFFu;

struct WorldInstDev {          // one per instance, 32 B: where its scene lives
    const float4* nodes;       // 64 B device records (racc_device.inc, slabPair), root = record 0
    const float4* pairs;
    const uint32_t* remap;
    uint64_t pad;
};
static_assert(sizeof(WorldInstDev) == 32, "one table entry per 32 B");

struct WorldArgs {
    const float4* rays;
    float4* results;
    uint32_t* instances;
    QueryFeedArgs feed;
    const float4* topNodes;    // top-level tree as 64 B device records: words 0-1 child references, then Lx Ly Lz Rx Ry Rz as (min, max)
    const uint32_t* order;     // a top-level leaf (first | cnt << 24) names the instances order[first .. first + cnt)
    const float4* inv;         // three rows per instance
    const WorldInstDev* table;
    float rayPad;
    const float* rayPadDev;    // the device word that holds the pad while the world has a refit handle (racc_world_refit.inc), else NULL
    uint32_t* spillTop;        // [topSpillLevels][gridThreads]
    uint32_t* spillBot;        // [botSpillLevels][gridThreads]
    uint32_t topSpillLevels, botSpillLevels, spillStride;
    uint32_t leafMin;
    uint32_t maxIters;
    uint32_t* trips;
};

// The hit epilogue of the closest-hit kernels (racc_kernel_v8.inc, Kernels.h:223-239: remap gather and edge rotation).  It is inline code
// there, in files this one may not touch, hence restated here: the one piece of bottom-level arithmetic (1 - u - v) that is.
__device__ __forceinline__ float4 worldHitRecord(const uint32_t* remap, int hitIndex, float t, float hitU, float hitV) {
    uint32_t m = remap[hitIndex];
    const uint32_t edge = m >> 30;
    m &= 0x3FFFFFFFu;
    const float bx = hitU, by = hitV, bz = 1.0f - hitU - hitV;
    float u = bx, v = by;
    if (edge == 1u) { u = bz; v = bx; } else if (edge == 2u) { u = by; v = bz; }
    return make_float4(__uint_as_float(m), t, u, v);
}

__device__ __forceinline__ bool worldEmptyRef(uint32_t ref) { return ref < kLeafBase; }      // a leaf reference of count 0 (one-instance worlds)

// ---- what the world kernels share (worldIntersectKernel here, worldOccludedKernel in racc_world_occlusion.inc): the world ray, the
// top-level step and the transform-and-enter rule.  One statement of each; the kernels differ in what they keep per lane, in the interval
// end they hand to the top level and in what an empty stack means.

// The world ray of a lane: origin and direction as given (what the instances transform), 1/d of the clamped direction for the top-level
// boxes (the clamp here only for those box tests), the ray's own interval, and the pad this ray adds to every top-level box.
struct WorldRay {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
    float tNear, tMax, pad;
};

__device__ __forceinline__ void setWorldRay(WorldRay& w, const float4 q0, const float4 q1, float rayPad) {
    w.ox = q0.x; w.oy = q0.y; w.oz = q0.z; w.tNear = q0.w;
    w.dx = q1.x; w.dy = q1.y; w.dz = q1.z; w.tMax = q1.w;
    w.ix = 1.0f / clampDir(w.dx); w.iy = 1.0f / clampDir(w.dy); w.iz = 1.0f / clampDir(w.dz);
    w.pad = rayPad * (fabsf(w.ox) + fabsf(w.oy) + fabsf(w.oz));
}

// The interval end the top level is walked with for a limit t: 2^-20 of itself past it — past every t <= the limit an instance could
// still report (world_build.cpp has the bound).
__device__ __forceinline__ float worldWidenedEnd(float t) { return t + fmaxf(fabsf(t) * 9.5367431640625e-07f, 1e-30f); }

// Top-level inner node: both child boxes, padded, against [tNear, tEnd] (tEnd = worldWidenedEnd of the kernel's limit).  `node` becomes
// the next reference, the farther child goes on the stack if both were entered; if neither was, pop() — the kernel's rule for what comes
// next, and for the empty stack.  (Continuations, not a returned flag: the closest-hit kernel compiles to what it was before the split.)
template <class Stack, class Pop>
__device__ __forceinline__ void worldTopInnerStep(const float4* topNodes, uint32_t& node, const WorldRay& w, float tEnd, Stack& top, Pop&& pop) {
    const float4* np = topNodes + size_t(node & 0x7FFFFFFFu) * 4;
    const uint2 k2 = *reinterpret_cast<const uint2*>(np);
    float4 d1 = np[1], d2 = np[2], d3 = np[3];
    d1.x -= w.pad; d1.y += w.pad; d1.z -= w.pad; d1.w += w.pad;
    d2.x -= w.pad; d2.y += w.pad; d2.z -= w.pad; d2.w += w.pad;
    d3.x -= w.pad; d3.y += w.pad; d3.z -= w.pad; d3.w += w.pad;
    float tFirst, tLast;
    slabPair(d1, d2, d3, w.ix, w.iy, w.iz, -w.ox * w.ix, -w.oy * w.iy, -w.oz * w.iz, w.tNear, tEnd, tFirst, tLast);
    const bool hitFirst = tFirst != tEnd && !worldEmptyRef(k2.x);      // (slabPair: tEnd doubles as "missed")
    const bool hitLast = tLast != tEnd && !worldEmptyRef(k2.y);
    if (hitFirst && hitLast) {
        const bool lastNearer = tLast < tFirst;
        top.push(lastNearer ? k2.x : k2.y);
        node = lastNearer ? k2.y : k2.x;
    } else if (hitFirst) node = k2.x;
    else if (hitLast) node = k2.y;
    else pop();
}

// Top-level leaf `leaf` (first | cnt << 24): its next instance, `id`; the rest of the range waits on the top-level stack.  `r` becomes the
// ray instance `id` sees — o' = inv (o, 1), d' = inv (d, 0): ((m0 x + m1 y) + m2 z) + m3, left to right (-ffp-contract=off: nothing is
// fused), with the ray's own minT and maxT whatever other instances have reported — and enter(id) starts the instance's traversal.  If
// the closest-hit path rejects the transformed ray (not finite), h_id is a miss: reject().
template <class Stack, class Reject, class Enter>
__device__ __forceinline__ void worldEnterNext(const uint32_t* order, const float4* inv, uint32_t leaf, const WorldRay& w, Stack& top, LaneRay& r, Reject&& reject, Enter&& enter) {
    const uint32_t first = leaf & 0xFFFFFFu, cnt = leaf >> 24;
    const uint32_t id = order[first];
    if (cnt > 1u) top.push(((cnt - 1u) << 24) | (first + 1u));
    const float4 m0 = inv[size_t(id) * 3], m1 = inv[size_t(id) * 3 + 1], m2 = inv[size_t(id) * 3 + 2];
    const float ox = ((m0.x * w.ox + m0.y * w.oy) + m0.z * w.oz) + m0.w;
    const float oy = ((m1.x * w.ox + m1.y * w.oy) + m1.z * w.oz) + m1.w;
    const float oz = ((m2.x * w.ox + m2.y * w.oy) + m2.z * w.oz) + m2.w;
    const float dx = (m0.x * w.dx + m0.y * w.dy) + m0.z * w.dz;
    const float dy = (m1.x * w.dx + m1.y * w.dy) + m1.z * w.dz;
    const float dz = (m2.x * w.dx + m2.y * w.dy) + m2.z * w.dz;
    if (!(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz))) reject();
    else {
        setLaneRay(r, ox, oy, oz, dx, dy, dz, w.tNear, w.tMax);
        enter(id);
    }
}

__global__ void __launch_bounds__(kWorldBlock) worldIntersectKernel(const WorldArgs a) {
    __shared__ uint32_t topLds[kWorldTopLds * kWorldBlock];
    __shared__ uint32_t botLds[kWorldBotLds * kWorldBlock];

    const uint32_t tid = threadIdx.x;
    const uint32_t gtid = blockIdx.x * uint32_t(kWorldBlock) + tid;
    const uint32_t lane = tid & 63u;
    const uint32_t gwave = uint32_t(__builtin_amdgcn_readfirstlane(int(gtid >> 6)));

    RayFeed feed;
    feed.start(a.feed, gwave);
    LaneStack<kWorldTopLds, kWorldBlock> top{topLds + tid, a.spillTop, a.topSpillLevels, a.spillStride, gtid, 0u};
    LaneStack<kWorldBotLds, kWorldBlock> bot{botLds + tid, a.spillBot, a.botSpillLevels, a.spillStride, gtid, 0u};

    WorldRay w = {};      // the world ray
    // the best instance result so far (raw: pair index * 2 + which, unrotated barycentrics) and the limit the top level culls with
    float bestT = 0.0f, bestU = 0.0f, bestV = 0.0f, tCull = 0.0f;
    int bestIndex = -1;
    uint32_t bestInst = kWorldNoInst;
    // inside an instance: the object-space ray, {1/d, -o/d}, the shrinking limit, the hit, the scene
    LaneRay r = {};
    const float4* scNodes = nullptr;
    const float4* scPairs = nullptr;
    uint32_t rayIdx = 0u, node = kEmpty, inst = kWorldNoInst;

    // next top-level reference from the stack; a ray that runs out of stack is finished: its record is written and its lane freed
    auto topPop = [&]() {
        if (!top.pop(node)) {
            float4 out = make_float4(__uint_as_float(kInvalidTriangle), 0.0f, 0.0f, 0.0f);
            if (bestInst != kWorldNoInst) out = worldHitRecord(a.table[bestInst].remap, bestIndex, bestT, bestU, bestV);
            a.results[rayIdx] = out;
            a.instances[rayIdx] = bestInst;
            node = kEmpty;
        }
    };
    // next bottom-level reference; an instance whose stack is empty is finished: its result is composed (smallest t, ties to the lowest
    // instance index) and the lane goes back to the top level
    auto botPop = [&]() {
        if (!bot.pop(node)) {
            if (r.hitIndex >= 0 && (bestInst == kWorldNoInst || r.tFar < bestT || (r.tFar == bestT && inst < bestInst))) {
                bestT = r.tFar; bestU = r.hitU; bestV = r.hitV; bestIndex = r.hitIndex; bestInst = inst;
                tCull = bestT;
            }
            inst = kWorldNoInst;
            topPop();
        }
    };

    for (uint32_t iter = 0;; ++iter) {
        if (watchdogTripped(iter, a.maxIters, a.trips, lane)) break;

        // ================= refill: idle lanes take the next rays of the wave's chunk =================
        const bool more = feed.refill(a.feed, node == kEmpty, lane, [&](uint32_t idx) {
            float4 q0, q1;
            if (!admitRay(a.rays, idx, q0, q1)) {
                a.results[idx] = make_float4(__uint_as_float(kInvalidTriangle), 0.0f, 0.0f, 0.0f);
                a.instances[idx] = kWorldNoInst;
            } else {
                setWorldRay(w, q0, q1, a.rayPadDev ? *a.rayPadDev : a.rayPad);
                bestInst = kWorldNoInst; bestIndex = -1; bestT = bestU = bestV = 0.0f;
                tCull = w.tMax;
                rayIdx = idx;
                inst = kWorldNoInst;
                node = 0x80000000u;      // the top-level root
                top.height = 0u; bot.height = 0u;
            }
        });
        if (!more) break;

        // ================= vote: one pair step, one bottom-level inner step or one top-level step =================
        const bool inBot = inst != kWorldNoInst;
        const bool isPair = inBot && int(node) >= int(kLeafBase);
        const bool isBotInner = inBot && int(node) < 0;
        const bool isTop = !inBot && node != kEmpty;
        const uint32_t nPair = uint32_t(__popcll(__ballot(isPair)));
        const uint32_t nBot = uint32_t(__popcll(__ballot(isBotInner)));
        const uint32_t nTop = uint32_t(__popcll(__ballot(isTop)));
        if (nPair != 0u && (nPair >= a.leafMin || (nBot == 0u && nTop == 0u))) {
            if (isPair) {      // Kernels.h:200-205, one pair per step: the leaf's pairs in order, tFar shrinking
                const uint32_t first = node & 0xFFFFFFu, cnt = node >> 24;
                const float4* p = scPairs + size_t(first) * 3;
                const float4 t0 = p[0], t1 = p[1], t2 = p[2];
                r.tFar = pairIntersectData(t0, t1, t2, first, r);
                if (cnt > 1u) node = ((cnt - 1u) << 24) | (first + 1u);
                else botPop();
            }
        } else if (nBot != 0u && nBot >= nTop) {
            if (isBotInner && !bvh2InnerStep(scNodes, node, r, r.tFar, bot)) botPop();      // tRay = the current tFar
        } else if (nTop != 0u) {
            if (isTop) {
                if (int(node) < 0) {      // top-level inner node, against [tNear, widened best t]: past every t that could still win or tie
                    worldTopInnerStep(a.topNodes, node, w, worldWidenedEnd(tCull), top, topPop);
                } else {                  // top-level leaf: enter its next instance
                    worldEnterNext(a.order, a.inv, node, w, top, r, topPop, [&](uint32_t id) {
                        const WorldInstDev e = a.table[id];
                        scNodes = e.nodes; scPairs = e.pairs;
                        inst = id;
                        node = 0x80000000u;     // Kernels.h:164
                        bot.height = 0u;
                    });
                }
            }
        }
    }
}

}  // namespace

struct racc_hip_world {
    racc_hip_ctx* ctx = nullptr;
    uint32_t count = 0;
    std::vector<const racc_hip_scene*> scenes;
    float4* topNodes = nullptr;               // [max(count - 1, 1)] device records
    uint32_t* order = nullptr;                // [count]
    float4* inv = nullptr;                    // [count][3]
    WorldInstDev* table = nullptr;            // [count]
    float rayPad = 0.0f;
    uint32_t maxBottomHeight = 0;
    racc_hip_world_info info{};
    struct racc_hip_world_refit* refit = nullptr;    // the world's refit handle, if it has one (racc_world_refit.inc) ...
    float* rayPadDev = nullptr;               // ... and then the handle's device word that holds the current pad
};

namespace {

// racc_world_refit.inc: the handle's tables rebuilt from a new top level (`dev` = its device records on the host) and its pad word set.
int worldRefitRebuild(racc_hip_world* w, const uint32_t* dev, float rayPad);
// racc_world_rebuild.inc: while the world's handle can rebuild on the device, info.height / spill_levels are held at the LBVH's bound
// and the handle's height word follows a host rebuild.  A no-op for any other world.
int worldRebuildHold(racc_hip_world* w);

// The member scenes' root boxes [count][6], read from the device: record 0's two child boxes combined.
int worldRootBoxes(const racc_hip_world* w, std::vector<float>& rootBoxes) {
    const uint32_t count = w->count;
    rootBoxes.resize(size_t(count) * 6);
    std::vector<std::pair<const racc_hip_scene*, std::array<float, 6>>> seen;
    for (uint32_t i = 0; i < count; ++i) {
        const racc_hip_scene* s = w->scenes[i];
        const std::array<float, 6>* box = nullptr;
        for (const auto& e : seen) if (e.first == s) { box = &e.second; break; }
        if (!box) {
            float rec[16];      // device record 0 = the root: words 4-15 = Lx Ly Lz Rx Ry Rz as (min, max)
            HIP_TRY(hipMemcpy(rec, s->nodes, sizeof(rec), hipMemcpyDeviceToHost), "hipMemcpy(root record)");
            std::array<float, 6> b;
            for (int k = 0; k < 3; ++k) {
                b[k] = rec[4 + 2 * k] < rec[10 + 2 * k] ? rec[4 + 2 * k] : rec[10 + 2 * k];
                b[3 + k] = rec[5 + 2 * k] > rec[11 + 2 * k] ? rec[5 + 2 * k] : rec[11 + 2 * k];
            }
            seen.emplace_back(s, b);
            box = &seen.back().second;
        }
        std::memcpy(&rootBoxes[size_t(i) * 6], box->data(), 24);
    }
    return RACC_HIP_OK;
}

// Reads the member scenes' root boxes from the device, runs racc_host_world_prepare and uploads its products.  Blocking.
int worldCommit(racc_hip_world* w, const float* transforms12) try {
    const uint32_t count = w->count;
    std::vector<float> rootBoxes;
    if (int rc = worldRootBoxes(w, rootBoxes)) return rc;
    const uint32_t capacity = count > 1u ? count - 1u : 1u;
    std::vector<float> inv(size_t(count) * 12), worldBoxes(size_t(count) * 6);
    std::vector<uint32_t> blob(size_t(capacity) * 16), order(count);
    uint32_t nodeCount = 0, height = 0;
    float rayPad = 0.0f;
    if (int rc = racc_host_world_prepare(transforms12, rootBoxes.data(), count, inv.data(), worldBoxes.data(), &rayPad, blob.data(), capacity, &nodeCount, order.data(), &height)) return rc;
    // blob node (Scene.cpp:73-78: leftMin[3], leftMax[3], rightMin[3], rightMax[3]) -> device record (racc_device.inc, slabPair), same numbering
    std::vector<uint32_t> dev(size_t(capacity) * 16, 0u);
    for (uint32_t n = 0; n < nodeCount; ++n) {
        const uint32_t* b = &blob[size_t(n) * 16];
        uint32_t* d = &dev[size_t(n) * 16];
        d[0] = b[2]; d[1] = b[3];
        for (int side = 0; side < 2; ++side)
            for (int k = 0; k < 3; ++k) { d[4 + side * 6 + 2 * k] = b[4 + side * 6 + k]; d[4 + side * 6 + 2 * k + 1] = b[4 + side * 6 + 3 + k]; }
    }
    HIP_TRY(hipMemcpy(w->topNodes, dev.data(), size_t(capacity) * 64, hipMemcpyHostToDevice), "hipMemcpy(top-level nodes)");
    HIP_TRY(hipMemcpy(w->order, order.data(), size_t(count) * 4, hipMemcpyHostToDevice), "hipMemcpy(instance order)");
    HIP_TRY(hipMemcpy(w->inv, inv.data(), size_t(count) * 48, hipMemcpyHostToDevice), "hipMemcpy(inverse transforms)");
    w->rayPad = rayPad;
    w->info.node_count = nodeCount;
    w->info.height = height;
    w->info.spill_levels = height + 1u > uint32_t(kWorldTopLds) ? height + 1u - uint32_t(kWorldTopLds) : 0u;
    if (w->refit) {      // a live refit handle follows the new topology and pad
        if (int rc = worldRefitRebuild(w, dev.data(), rayPad)) return rc;
        return worldRebuildHold(w);
    }
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world: out of host memory");
}

// What a launch of either world kernel does on the host: the grid and the feed, the members the two argument structs share (same names),
// and launch(a, blocks) inside the launch's scratch (racc_query.inc; here the cursor word and both spills).
template <class Args, class Launch>
int launchOnWorld(racc_hip_ctx* ctx, const racc_hip_world* w, const void* dRays, uint32_t count, uint32_t waves, uint32_t refillMin, uint32_t leafMin,
                  const char* limitMsg, const char* launchMsg, hipStream_t st, Args& a, Launch&& launch) {
    QueryGrid g;
    if (int rc = queryGrid(ctx, count, uint32_t(kWorldBlock), waves, limitMsg, g, a.feed)) return rc;
    a.rays = static_cast<const float4*>(dRays);
    a.topNodes = w->topNodes; a.order = w->order; a.inv = w->inv; a.table = w->table;
    a.rayPad = w->rayPad; a.rayPadDev = w->rayPadDev;
    a.topSpillLevels = w->info.spill_levels;
    a.botSpillLevels = w->info.bottom_spill_levels;
    a.spillStride = g.gridThreads;
    a.feed.refillMin = refillMin; a.leafMin = leafMin;
    a.maxIters = ctx->maxIters;
    a.trips = ctx->devTrips;
    return withQueryScratch(size_t(a.topSpillLevels + a.botSpillLevels) * g.gridThreads, st, launchMsg, [&](uint32_t* scratch) {
        a.feed.cursor = scratch;
        a.spillTop = scratch + kQueryScratchHead;
        a.spillBot = a.spillTop + size_t(a.topSpillLevels) * g.gridThreads;
        launch(a, g.blocks);
    });
}

// Enqueues one world launch on `st`.
int launchWorld(racc_hip_ctx* ctx, const racc_hip_world* w, const void* dRays, void* dResults, uint32_t* dInstances, uint32_t count, hipStream_t st) {
    // RACC_WORLD_WAVES / RACC_WORLD_REFILL / RACC_WORLD_LEAF: A/B of the grid size and the two vote thresholds (tools/bench_world.py)
    static const uint32_t envWaves = queryTunable("RACC_WORLD_WAVES", 1, 8, kWorldWavesPerSimd);
    static const uint32_t envRefill = queryTunable("RACC_WORLD_REFILL", 1, 64, kWorldRefillMin);
    static const uint32_t envLeaf = queryTunable("RACC_WORLD_LEAF", 1, 64, kWorldLeafMin);
    WorldArgs a;
    a.results = static_cast<float4*>(dResults);
    a.instances = dInstances;
    return launchOnWorld(ctx, w, dRays, count, envWaves, envRefill, envLeaf, "world_intersect: more than 0xFF000000 rays in one launch", "launch worldIntersectKernel", st, a,
                         [&](const WorldArgs& args, uint32_t blocks) { hipLaunchKernelGGL(worldIntersectKernel, dim3(blocks), dim3(kWorldBlock), 0, st, args); });
}

}  // namespace

extern "C" {

int racc_hip_world_destroy(racc_hip_ctx* ctx, racc_hip_world* w) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_destroy: ctx is NULL");
    if (!w) return RACC_HIP_OK;
    if (w->refit) return fail(RACC_HIP_ERR_INVALID, "world_destroy: the world has a refit handle: racc_hip_world_refit_destroy comes first");
    hipSetDevice(ctx->device);
    if (w->topNodes) hipFree(w->topNodes);
    if (w->order) hipFree(w->order);
    if (w->inv) hipFree(w->inv);
    if (w->table) hipFree(w->table);
    delete w;
    return RACC_HIP_OK;
}

int racc_hip_world_create(racc_hip_ctx* ctx, const float* transforms12, const racc_hip_scene* const* scenes, uint32_t count, racc_hip_world** out) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_create: ctx is NULL");
    if (!out) return fail(RACC_HIP_ERR_INVALID, "world_create: out is NULL");
    *out = nullptr;
    if (!transforms12 || !scenes) return fail(RACC_HIP_ERR_INVALID, "world_create: transforms/scenes is NULL");
    if (!count) return fail(RACC_HIP_ERR_INVALID, "world_create: count is 0: a world has at least one instance");
    if (count > RACC_HIP_WORLD_MAX_INSTANCES) return fail(RACC_HIP_ERR_INVALID, "world_create: more than 2^20 instances");
    uint32_t maxHeight = 0;
    const racc_hip_scene* known = nullptr;      // (runs of one scene are the common case: one registry lookup per run)
    for (uint32_t i = 0; i < count; ++i) {
        const racc_hip_scene* s = scenes[i];
        if (!s) return fail(RACC_HIP_ERR_INVALID, "world_create: a scene is NULL");
        if (s != known) {
            if (sceneOwner(s) != ctx) return fail(RACC_HIP_ERR_INVALID, "world_create: a scene was not uploaded through racc_hip_scene_upload on this context (another context's scene, or a device group's replica)");
            known = s;
        }
        if (s->info.inner_height > maxHeight) maxHeight = s->info.inner_height;
    }
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    racc_hip_world* w = new (std::nothrow) racc_hip_world();
    if (!w) return fail(RACC_HIP_ERR_NOMEM, "out of host memory");
    w->ctx = ctx; w->count = count;
    w->scenes.assign(scenes, scenes + count);
    w->maxBottomHeight = maxHeight;
    std::vector<WorldInstDev> table(count);
    for (uint32_t i = 0; i < count; ++i) { table[i].nodes = scenes[i]->nodes; table[i].pairs = scenes[i]->pairs; table[i].remap = scenes[i]->remap; table[i].pad = 0; }
    const size_t capacity = count > 1u ? count - 1u : 1u;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&w->topNodes), capacity * 64);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&w->order), size_t(count) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&w->inv), size_t(count) * 48);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&w->table), size_t(count) * sizeof(WorldInstDev));
    if (e == hipSuccess) e = hipMemcpy(w->table, table.data(), size_t(count) * sizeof(WorldInstDev), hipMemcpyHostToDevice);
    if (e != hipSuccess) { racc_hip_world_destroy(ctx, w); return fail(RACC_HIP_ERR_DEVICE, "world_create", e); }
    w->info.instance_count = count;
    w->info.lds_levels = uint32_t(kWorldTopLds);
    w->info.bottom_spill_levels = maxHeight > uint32_t(kWorldBotLds) ? maxHeight - uint32_t(kWorldBotLds) : 0u;
    w->info.device_bytes = capacity * 64 + size_t(count) * (4 + 48 + sizeof(WorldInstDev));
    if (int rc = worldCommit(w, transforms12)) { racc_hip_world_destroy(ctx, w); return rc; }
    *out = w;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_create: out of host memory");
}

int racc_hip_world_update(racc_hip_ctx* ctx, racc_hip_world* w, const float* transforms12, uint32_t count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_update: ctx is NULL");
    if (!w || !transforms12) return fail(RACC_HIP_ERR_INVALID, "world_update: world/transforms is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_update: the world belongs to another context");
    if (count != w->count) return fail(RACC_HIP_ERR_INVALID, "world_update: count differs from the world's instance count");
    if (int rc = racc_hip_synchronize(ctx)) return rc;      // no kernel reads the top level or a root box while they change
    // (a transform that is refused leaves the world as it was: racc_host_world_prepare validates before anything is uploaded)
    return worldCommit(w, transforms12);
}

int racc_hip_world_get_info(const racc_hip_world* w, racc_hip_world_info* info) {
    if (!w || !info) return fail(RACC_HIP_ERR_INVALID, "world_get_info: world/info is NULL");
    *info = w->info;
    return RACC_HIP_OK;
}

int racc_hip_world_intersect_device(racc_hip_ctx* ctx, const racc_hip_world* w, const void* d_rays, void* d_results, uint32_t* d_instances, uint32_t count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_intersect_device: ctx is NULL");
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_intersect_device: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_intersect_device: the world belongs to another context");
    if (!count) return RACC_HIP_OK;
    if (!d_rays || !d_results || !d_instances) return fail(RACC_HIP_ERR_INVALID, "world_intersect_device: d_rays/d_results/d_instances is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return launchWorld(ctx, w, d_rays, d_results, d_instances, count, static_cast<hipStream_t>(stream));
}

int racc_hip_world_intersect(racc_hip_ctx* ctx, const racc_hip_world* w, const void* rays, void* results, uint32_t* instances, uint32_t count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_intersect: ctx is NULL");
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_intersect: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_intersect: the world belongs to another context");
    if (!count) return RACC_HIP_OK;
    if (!rays || !results || !instances) return fail(RACC_HIP_ERR_INVALID, "world_intersect: rays/results/instances is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return runStagedQuery(ctx, "world_intersect (host arrays)", rays, count, results, size_t(count) * 16, instances, size_t(count) * 4, [&](void* dRays, void* dOut, void* dInst, hipStream_t st) {
        return launchWorld(ctx, w, dRays, dOut, static_cast<uint32_t*>(dInst), count, st);
    });
}

}  // extern "C"
