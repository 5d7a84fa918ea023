// racc_occlusion.inc — occlusion (any-hit) queries: occludedKernel and the two C-ABI entries around it.  Textually included by
// racc_hip_unit.hip BEHIND racc_hip.hip and racc_query.inc, so it sees the context, the scene's device pointers, fail() / HIP_TRY /
// checkWatchdog, the helpers of racc_device.inc and the query scaffold, and changes none of them.  The reference has no such query (its
// scheduler only knows the closest hit); Embree's rtcOccluded is the usual counterpart.
//
// Contract: occluded = 1 iff a triangle pair that the reference traversal rule reaches with tRay = the ray's own maxT (never shrunk)
// passes the reference pair test up to `outside1 && outside2` (racc_device.inc, pairIntersectData) — which is exactly
// "the closest-hit traversal reports a hit": until its first hit that traversal runs with the limit maxT as well, every node decision
// depends only on the ray, the node and that limit, and after a first hit it is a hit whatever follows.  Same expressions as the
// closest-hit kernels (explicit fmaf only, -ffp-contract=off); the order in which children and pairs are visited is free, so a lane
// stops at the first accepted pair.  No hit state, no division per hit, no remap gather, no miss colour: one byte per ray.
//
// Structure (plain HIP, no inline assembly in this version): the wavefront scaffold of racc_query.inc (ray feed, lane stack, BVH2 inner
// step, stream-ordered scratch) over the 64 B BVH2 records of scene->nodes; each scheduling iteration the wave votes for one pair step
// (every lane that holds a leaf tests ONE pair) or one inner step.

namespace {

constexpr int kOccBlock = 256;
constexpr int kOccLdsLevels = 12;           // stack levels in LDS (12 KB per workgroup); a push happens at most once per inner node of the root path
constexpr uint32_t kOccWavesPerSimd = 6;    // grid: this many workgroups of four waves per CU (see `make resources` for the kernel's occupancy)
constexpr uint32_t kOccRefillMin = 16;      // idle lanes that trigger a refill
constexpr uint32_t kOccLeafMin = 10;        // leaf lanes that trigger a pair step

struct OccludeArgs {
    const float4* rays;
    uint8_t* occluded;
    QueryFeedArgs feed;
    const float4* nodes;      // 64 B device records (racc_device.inc, slabPair), root = record 0
    const float4* pairs;
    uint32_t* spill;          // [spillLevels][gridThreads]
    uint32_t spillLevels, spillStride;
    uint32_t leafMin;         // leaf lanes that trigger a pair step
    uint32_t maxIters;
    uint32_t* trips;
};

// pairIntersectData (racc_device.inc) up to its `if (outside1 && outside2)` and nothing after it: same expressions, same order.
__device__ __forceinline__ bool pairAccepts(const float4 t0, const float4 t1, const float4 t2, float ox, float oy, float oz,
                                            float dx, float dy, float dz, float tNear, float tMax) {
    const float n1x = __builtin_fmaf(t0.y, t1.z, -(t0.z * t1.y));
    const float n1y = __builtin_fmaf(t0.z, t1.x, -(t0.x * t1.z));
    const float n1z = __builtin_fmaf(t0.x, t1.y, -(t0.y * t1.x));
    const float n2x = __builtin_fmaf(t1.w, t0.z, -(t2.w * t0.y));
    const float n2y = __builtin_fmaf(t2.w, t0.x, -(t0.w * t0.z));
    const float n2z = __builtin_fmaf(t0.w, t0.y, -(t1.w * t0.x));
    const float cx = t2.x - ox, cy = t2.y - oy, cz = t2.z - oz;
    const float rx = __builtin_fmaf(dy, cz, -(dz * cy));
    const float ry = __builtin_fmaf(dz, cx, -(dx * cz));
    const float rz = __builtin_fmaf(dx, cy, -(dy * cx));

    const float det1 = dot3(n1x, n1y, n1z, dx, dy, dz);
    const float det2 = dot3(n2x, n2y, n2z, dx, dy, dz);
    const uint32_t sgn1 = __float_as_uint(det1) & 0x80000000u;
    const uint32_t sgn2 = __float_as_uint(det2) & 0x80000000u;

    const float re1 = dot3(rx, ry, rz, t0.x, t0.y, t0.z);
    const uint32_t iU1 = __float_as_uint(dot3(rx, ry, rz, t1.x, t1.y, t1.z)) ^ sgn1;
    const uint32_t iV1 = __float_as_uint(re1) ^ sgn1;
    const uint32_t iU2 = __float_as_uint(-re1) ^ sgn2;
    const uint32_t iV2 = __float_as_uint(-dot3(rx, ry, rz, t0.w, t1.w, t2.w)) ^ sgn2;

    bool outside1 = int(iU1 | iV1) < 0;
    bool outside2 = int(iU2 | iV2) < 0;

    const float U1 = __uint_as_float(iU1), V1 = __uint_as_float(iV1);
    const float U2 = __uint_as_float(iU2), V2 = __uint_as_float(iV2);
    const float absDet1 = fabsf(det1);
    const float absDet2 = fabsf(det2);
    const float W1 = absDet1 - U1 - V1;
    const float W2 = absDet2 - U2 - V2;
    const float T1 = __uint_as_float(__float_as_uint(dot3(n1x, n1y, n1z, cx, cy, cz)) ^ sgn1);
    const float T2 = __uint_as_float(__float_as_uint(dot3(n2x, n2y, n2z, cx, cy, cz)) ^ sgn2);

    outside1 = outside1 || (W1 < 0.0f || T1 <= absDet1 * tNear || T1 > absDet1 * tMax);      // open at tNear, closed at tMax
    outside2 = outside2 || (W2 < 0.0f || T2 <= absDet2 * tNear || T2 > absDet2 * tMax);
    return !(outside1 && outside2);
}

__global__ void __launch_bounds__(kOccBlock) occludedKernel(const OccludeArgs a) {
    __shared__ uint32_t stackLds[kOccLdsLevels * kOccBlock];

    const uint32_t tid = threadIdx.x;
    const uint32_t gtid = blockIdx.x * uint32_t(kOccBlock) + tid;
    const uint32_t lane = tid & 63u;
    const uint32_t gwave = uint32_t(__builtin_amdgcn_readfirstlane(int(gtid >> 6)));

    RayFeed feed;
    feed.start(a.feed, gwave);
    LaneStack<kOccLdsLevels, kOccBlock> stack{stackLds + tid, a.spill, a.spillLevels, a.spillStride, gtid, 0u};

    // lane state: the ray (tFar = its own maxT, never shrunk; no hit is kept), its index and the node it holds
    LaneRay r = {};
    uint32_t rayIdx = 0u, node = kEmpty;

    // next node from the stack; a ray that runs out of stack is a miss and frees its lane
    auto pop = [&]() {
        if (!stack.pop(node)) { a.occluded[rayIdx] = uint8_t(0); node = kEmpty; }
    };

    for (uint32_t iter = 0;; ++iter) {
        if (watchdogTripped(iter, a.maxIters, a.trips, lane)) break;

        // ================= refill: idle lanes take the next rays of the wave's chunk =================
        const bool more = feed.refill(a.feed, node == kEmpty, lane, [&](uint32_t idx) {
            float4 q0, q1;
            if (!admitRay(a.rays, idx, q0, q1)) a.occluded[idx] = uint8_t(0);
            else {
                setLaneRay(r, q0.x, q0.y, q0.z, q1.x, q1.y, q1.z, q0.w, q1.w);
                rayIdx = idx;
                node = 0x80000000u;     // Kernels.h:164
                stack.height = 0u;
            }
        });
        if (!more) break;

        // ================= vote: one pair step or one inner step =================
        const bool isLeaf = int(node) >= int(kLeafBase);
        const bool isInner = int(node) < 0;
        const uint32_t nLeaf = uint32_t(__popcll(__ballot(isLeaf)));
        const uint32_t nInner = uint32_t(__popcll(__ballot(isInner)));
        if (nLeaf != 0u && (nLeaf >= a.leafMin || nInner == 0u)) {
            if (isLeaf) {
                const uint32_t first = node & 0xFFFFFFu, cnt = node >> 24;
                const float4* p = a.pairs + size_t(first) * 3;
                const float4 t0 = p[0], t1 = p[1], t2 = p[2];
                if (pairAccepts(t0, t1, t2, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, r.tNear, r.tFar)) { a.occluded[rayIdx] = uint8_t(1); node = kEmpty; }
                else if (cnt > 1u) node = ((cnt - 1u) << 24) | (first + 1u);      // the leaf's remaining pairs
                else pop();
            }
        } else if (nInner != 0u) {
            if (isInner && !bvh2InnerStep(a.nodes, node, r, r.tFar, stack)) pop();
        }
    }
}

// Enqueues one occlusion launch on `st` (scratch: racc_query.inc).
int launchOccluded(racc_hip_ctx* ctx, const racc_hip_scene* scene, const void* dRays, uint8_t* dOccluded, uint32_t count, hipStream_t st) {
    // RACC_OCC_WAVES / RACC_OCC_REFILL / RACC_OCC_LEAF: A/B of the grid size and the two vote thresholds (tools/bench_occlusion.py)
    static const uint32_t envWaves = queryTunable("RACC_OCC_WAVES", 1, 8, kOccWavesPerSimd);
    static const uint32_t envRefill = queryTunable("RACC_OCC_REFILL", 1, 64, kOccRefillMin);
    static const uint32_t envLeaf = queryTunable("RACC_OCC_LEAF", 1, 64, kOccLeafMin);
    QueryGrid g;
    OccludeArgs a;
    if (int rc = queryGrid(ctx, count, uint32_t(kOccBlock), envWaves, "occluded: more than 0xFF000000 rays in one launch", g, a.feed)) return rc;
    const uint32_t height = scene->info.inner_height;
    a.rays = static_cast<const float4*>(dRays);
    a.occluded = dOccluded;
    a.nodes = scene->nodes; a.pairs = scene->pairs;
    a.spillLevels = height > uint32_t(kOccLdsLevels) ? height - uint32_t(kOccLdsLevels) : 0u;
    a.spillStride = g.gridThreads;
    a.feed.refillMin = envRefill; a.leafMin = envLeaf;
    a.maxIters = ctx->maxIters;
    a.trips = ctx->devTrips;
    return withQueryScratch(size_t(a.spillLevels) * g.gridThreads, st, "launch occludedKernel", [&](uint32_t* scratch) {
        a.feed.cursor = scratch;
        a.spill = scratch + kQueryScratchHead;
        hipLaunchKernelGGL(occludedKernel, dim3(g.blocks), dim3(kOccBlock), 0, st, a);
    });
}

}  // namespace

extern "C" {

int racc_hip_occluded_device(racc_hip_ctx* ctx, const racc_hip_scene* scene, const void* d_rays, uint8_t* d_occluded, uint32_t count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "occluded_device: ctx is NULL");
    if (!scene) return fail(RACC_HIP_ERR_INVALID, "occluded_device: scene is NULL");
    if (!count) return RACC_HIP_OK;
    if (!d_rays || !d_occluded) return fail(RACC_HIP_ERR_INVALID, "occluded_device: d_rays/d_occluded is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return launchOccluded(ctx, scene, d_rays, d_occluded, count, static_cast<hipStream_t>(stream));
}

int racc_hip_occluded(racc_hip_ctx* ctx, const racc_hip_scene* scene, const void* rays, uint8_t* occluded, uint32_t count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "occluded: ctx is NULL");
    if (!scene) return fail(RACC_HIP_ERR_INVALID, "occluded: scene is NULL");
    if (!count) return RACC_HIP_OK;
    if (!rays || !occluded) return fail(RACC_HIP_ERR_INVALID, "occluded: rays/occluded is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return runStagedQuery(ctx, "occluded (host arrays)", rays, count, occluded, size_t(count), nullptr, 0, [&](void* dRays, void* dOut, void*, hipStream_t st) {
        return launchOccluded(ctx, scene, dRays, static_cast<uint8_t*>(dOut), count, st);
    });
}

}  // extern "C"
