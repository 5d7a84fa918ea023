// racc_world_occlusion.inc — occlusion (any-hit) queries on worlds: worldOccludedKernel and the two C-ABI entries around it
// (racc_hip_world_occluded*).  Textually included by racc_hip_unit.hip BEHIND racc_world.inc, so it sees the world, the query scaffold
// (racc_query.inc), pairAccepts (racc_occlusion.inc) and the world helpers (racc_world.inc: WorldRay, worldTopInnerStep, worldEnterNext,
// worldWidenedEnd, launchOnWorld), and changes none of them.  Embree's rtcOccluded on a scene with instances is the usual counterpart.
//
// Contract (include/racc_hip.h): occluded[i] = 1 iff some instance's closest-hit result h_i, as defined for racc_hip_world_intersect*, is a
// hit — i.e. iff racc_hip_world_intersect* reports instance != 0xFFFFFFFF for that ray; for every ray.  Inside an instance the rule is
// occludedKernel's: the transformed ray with the ray's own minT / maxT, tRay never shrunk, the pair test up to `outside1 && outside2`,
// stop at the first accepted pair — which is "h_i is a hit" by that kernel's argument.  Rays the closest-hit path rejects give 0; a
// transformed ray it rejects only skips that instance.
//
// Why it holds.  "Some h_i is a hit" does not depend on the order in which instances, children or pairs are visited, so the order is free
// and a lane stops at the first accepted pair.  What has to be shown is that every instance that could report a hit is entered unless the
// ray is already decided.  The top level is walked with the interval end fixed at the ray's own maxT, widened by 2^-20 of itself exactly
// as worldIntersectKernel widens tCull (worldWidenedEnd, computed once at admission).  The closest-hit kernel's tCull starts at maxT and
// only shrinks, so this end is never smaller than the one that kernel uses; and by the bound in world_build.cpp an instance that could
// report t <= maxT — every h_i that is a hit has t <= maxT — has a padded box the ray meets in [minT, that end], at every level of the
// top-level tree (a parent's box contains its children's).  So the walk here enters every instance the closest-hit walk can enter and
// every instance with a hit; it stops early only with the answer 1.
//
// Lane state: the world ray and its widened end, the object-space ray, the scene's two pointers, whether the lane is inside an instance.
// No best hit, no tCull, no remap pointer, no hit epilogue.  Structure as worldIntersectKernel: the three-way vote (pair step,
// bottom-level inner step, top-level step) over two lane stacks.

namespace {

constexpr uint32_t kWoccWavesPerSimd = 6;     // grid: this many workgroups of four waves per CU (`make resources` has the kernel's occupancy)
constexpr uint32_t kWoccRefillMin = 16;       // idle lanes that trigger a refill
constexpr uint32_t kWoccLeafMin = 10;         // bottom-level leaf lanes that trigger a pair step

struct WorldOccArgs {          // WorldArgs with one byte per ray for its two outputs (launchOnWorld fills the members they share)
    const float4* rays;
    uint8_t* occluded;
    QueryFeedArgs feed;
    const float4* topNodes;
    const uint32_t* order;
    const float4* inv;
    const WorldInstDev* table;
    float rayPad;
    const float* rayPadDev;
    uint32_t* spillTop;        // [topSpillLevels][gridThreads]
    uint32_t* spillBot;        // [botSpillLevels][gridThreads]
    uint32_t topSpillLevels, botSpillLevels, spillStride;
    uint32_t leafMin;
    uint32_t maxIters;
    uint32_t* trips;
};

__global__ void __launch_bounds__(kWorldBlock) worldOccludedKernel(const WorldOccArgs a) {
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

    WorldRay w = {};           // the world ray
    float tEnd = 0.0f;         // its own maxT, widened: the top level's interval end for the ray's whole life
    // inside an instance: the object-space ray (tFar = the ray's own maxT, never shrunk; no hit is kept) and the scene
    LaneRay r = {};
    const float4* scNodes = nullptr;
    const float4* scPairs = nullptr;
    uint32_t rayIdx = 0u, node = kEmpty;
    bool inBot = false;

    // next top-level reference; a ray that runs out of top-level stack is not occluded and frees its lane
    auto topPop = [&]() {
        if (!top.pop(node)) { a.occluded[rayIdx] = uint8_t(0); node = kEmpty; }
    };
    // next bottom-level reference; an instance whose stack is empty has no hit: the lane goes back to the top level
    auto botPop = [&]() {
        if (!bot.pop(node)) { inBot = false; topPop(); }
    };

    for (uint32_t iter = 0;; ++iter) {
        if (watchdogTripped(iter, a.maxIters, a.trips, lane)) break;

        // ================= refill: idle lanes take the next rays of the wave's chunk =================
        const bool more = feed.refill(a.feed, node == kEmpty, lane, [&](uint32_t idx) {
            float4 q0, q1;
            if (!admitRay(a.rays, idx, q0, q1)) a.occluded[idx] = uint8_t(0);
            else {
                setWorldRay(w, q0, q1, a.rayPadDev ? *a.rayPadDev : a.rayPad);
                tEnd = worldWidenedEnd(w.tMax);
                rayIdx = idx;
                inBot = false;
                node = 0x80000000u;      // the top-level root
                top.height = 0u; bot.height = 0u;
            }
        });
        if (!more) break;

        // ================= vote: one pair step, one bottom-level inner step or one top-level step =================
        const bool isPair = inBot && int(node) >= int(kLeafBase);
        const bool isBotInner = inBot && int(node) < 0;
        const bool isTop = !inBot && node != kEmpty;
        const uint32_t nPair = uint32_t(__popcll(__ballot(isPair)));
        const uint32_t nBot = uint32_t(__popcll(__ballot(isBotInner)));
        const uint32_t nTop = uint32_t(__popcll(__ballot(isTop)));
        if (nPair != 0u && (nPair >= a.leafMin || (nBot == 0u && nTop == 0u))) {
            if (isPair) {      // one pair per step; the first accepted pair decides the ray
                const uint32_t first = node & 0xFFFFFFu, cnt = node >> 24;
                const float4* p = scPairs + size_t(first) * 3;
                const float4 t0 = p[0], t1 = p[1], t2 = p[2];
                if (pairAccepts(t0, t1, t2, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.tNear, r.tFar)) { a.occluded[rayIdx] = uint8_t(1); inBot = false; node = kEmpty; }
                else if (cnt > 1u) node = ((cnt - 1u) << 24) | (first + 1u);      // the leaf's remaining pairs
                else botPop();
            }
        } else if (nBot != 0u && nBot >= nTop) {
            if (isBotInner && !bvh2InnerStep(scNodes, node, r, r.tFar, bot)) botPop();      // tRay = the ray's own maxT
        } else if (nTop != 0u) {
            if (isTop) {
                if (int(node) < 0) {      // top-level inner node, against [tNear, widened maxT]
                    worldTopInnerStep(a.topNodes, node, w, tEnd, top, topPop);
                } else {                  // top-level leaf: enter its next instance; a rejected transformed ray only skips it
                    worldEnterNext(a.order, a.inv, node, w, top, r, topPop, [&](uint32_t id) {
                        const WorldInstDev e = a.table[id];
                        scNodes = e.nodes; scPairs = e.pairs;
                        inBot = true;
                        node = 0x80000000u;     // Kernels.h:164
                        bot.height = 0u;
                    });
                }
            }
        }
    }
}

// Enqueues one world occlusion launch on `st`.
int launchWorldOccluded(racc_hip_ctx* ctx, const racc_hip_world* w, const void* dRays, uint8_t* dOccluded, uint32_t count, hipStream_t st) {
    // RACC_WOCC_WAVES / RACC_WOCC_REFILL / RACC_WOCC_LEAF: A/B of the grid size and the two vote thresholds (tools/bench_world_occlusion.py)
    static const uint32_t envWaves = queryTunable("RACC_WOCC_WAVES", 1, 8, kWoccWavesPerSimd);
    static const uint32_t envRefill = queryTunable("RACC_WOCC_REFILL", 1, 64, kWoccRefillMin);
    static const uint32_t envLeaf = queryTunable("RACC_WOCC_LEAF", 1, 64, kWoccLeafMin);
    WorldOccArgs a;
    a.occluded = dOccluded;
    return launchOnWorld(ctx, w, dRays, count, envWaves, envRefill, envLeaf, "world_occluded: more than 0xFF000000 rays in one launch", "launch worldOccludedKernel", st, a,
                         [&](const WorldOccArgs& args, uint32_t blocks) { hipLaunchKernelGGL(worldOccludedKernel, dim3(blocks), dim3(kWorldBlock), 0, st, args); });
}

}  // namespace

extern "C" {

int racc_hip_world_occluded_device(racc_hip_ctx* ctx, const racc_hip_world* w, const void* d_rays, uint8_t* d_occluded, uint32_t count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_occluded_device: ctx is NULL");
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_occluded_device: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_occluded_device: the world belongs to another context");
    if (!count) return RACC_HIP_OK;
    if (!d_rays || !d_occluded) return fail(RACC_HIP_ERR_INVALID, "world_occluded_device: d_rays/d_occluded is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return launchWorldOccluded(ctx, w, d_rays, d_occluded, count, static_cast<hipStream_t>(stream));
}

int racc_hip_world_occluded(racc_hip_ctx* ctx, const racc_hip_world* w, const void* rays, uint8_t* occluded, uint32_t count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_occluded: ctx is NULL");
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_occluded: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_occluded: the world belongs to another context");
    if (!count) return RACC_HIP_OK;
    if (!rays || !occluded) return fail(RACC_HIP_ERR_INVALID, "world_occluded: rays/occluded is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return runStagedQuery(ctx, "world_occluded (host arrays)", rays, count, occluded, size_t(count), nullptr, 0, [&](void* dRays, void* dOut, void*, hipStream_t st) {
        return launchWorldOccluded(ctx, w, dRays, static_cast<uint8_t*>(dOut), count, st);
    });
}

}  // extern "C"
