// racc_occlusion.inc — occlusion (any-hit) queries: occludedKernel and the two C-ABI entries around it.  Textually included by
// racc_hip_unit.hip BEHIND racc_hip.hip, so it sees the context, the scene's device pointers, fail() / HIP_TRY / checkWatchdog and the
// helpers of racc_device.inc, and changes none of them.  The reference has no such query (its scheduler only knows the closest hit);
// Embree's rtcOccluded is the usual counterpart.
//
// Contract: occluded = 1 iff a triangle pair that the reference traversal rule reaches with tRay = the ray's own maxT (never shrunk)
// passes the reference pair test up to `outside1 && outside2` (racc_device.inc, pairIntersectData) — which is exactly
// "the closest-hit traversal reports a hit": until its first hit that traversal runs with the limit maxT as well, every node decision
// depends only on the ray, the node and that limit, and after a first hit it is a hit whatever follows.  Same expressions as the
// closest-hit kernels (explicit fmaf only, -ffp-contract=off); the order in which children and pairs are visited is free, so a lane
// stops at the first accepted pair.  No hit state, no division per hit, no remap gather, no miss colour: one byte per ray.
//
// Structure (plain HIP, no inline assembly in this version): a persistent grid of wave64 waves over the 64 B BVH2 records of
// scene->nodes; rays are handed out in chunks (the first chunk of every wave statically, the rest from one cursor word); finished
// lanes are found by ballot, ranked with laneRank and refilled; each scheduling iteration the wave votes for one pair step (every lane
// that holds a leaf tests ONE pair) or one inner step; the per-lane stack is [level][thread] columns in LDS, deeper levels in a global
// spill.  The launch's scratch (cursor word + spill) is allocated, zeroed and freed in stream order around the kernel: nothing of it
// lives in the context or a lane, so launches on different streams overlap each other and chained closest-hit batches.

namespace {

constexpr int kOccBlock = 256;
constexpr int kOccLdsLevels = 12;           // stack levels in LDS (12 KB per workgroup); a push happens at most once per inner node of the root path
constexpr uint32_t kOccWavesPerSimd = 6;    // grid: this many workgroups of four waves per CU (see `make resources` for the kernel's occupancy)
constexpr uint32_t kOccRefillMin = 16;      // idle lanes that trigger a refill
constexpr uint32_t kOccLeafMin = 10;        // leaf lanes that trigger a pair step
constexpr uint32_t kOccScratchHead = 64;    // words in front of the spill area: word 0 = the ray cursor

struct OccludeArgs {
    const float4* rays;
    uint8_t* occluded;
    uint32_t count;
    const float4* nodes;      // 64 B device records (racc_device.inc, slabPair), root = record 0
    const float4* pairs;
    uint32_t* cursor;         // one zeroed word per launch
    uint32_t dynBase;         // rays handed out statically (grid waves x chunk): the cursor counts from here
    uint32_t chunk;           // rays per dequeue, a multiple of 64
    uint32_t* spill;          // [spillLevels][gridThreads]
    uint32_t spillLevels, spillStride;
    uint32_t refillMin;       // idle lanes that trigger a refill
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
    __shared__ uint32_t stackLds[kOccLdsLevels * kOccBlock];      // [level][thread]: conflict-free columns

    const uint32_t tid = threadIdx.x;
    const uint32_t gtid = blockIdx.x * uint32_t(kOccBlock) + tid;
    const uint32_t lane = tid & 63u;
    const uint32_t gwave = uint32_t(__builtin_amdgcn_readfirstlane(int(gtid >> 6)));

    // the wave's current chunk [wBeg, wEnd): the first one is assigned statically (no start-up stampede on the cursor word)
    uint32_t wBeg = gwave * a.chunk, wEnd;
    if (wBeg >= a.count) { wBeg = 0u; wEnd = 0u; }
    else wEnd = wBeg + min(a.chunk, a.count - wBeg);
    bool exhausted = a.dynBase >= a.count;

    // lane state: the ray, {1/d, -o/d}, its interval, its index, the node it holds and its stack height
    float ox = 0.0f, oy = 0.0f, oz = 0.0f, dx = 0.0f, dy = 0.0f, dz = 0.0f;
    float ix = 0.0f, iy = 0.0f, iz = 0.0f, ex = 0.0f, ey = 0.0f, ez = 0.0f;
    float tNear = 0.0f, tFar = 0.0f;
    uint32_t rayIdx = 0u, node = kEmpty, sp = 0u;

    // next node from the stack; a ray that runs out of stack is a miss and frees its lane
#define RACC_OCC_POP()                                                                                              \
    do {                                                                                                            \
        if (sp == 0u) { a.occluded[rayIdx] = uint8_t(0); node = kEmpty; }                                           \
        else {                                                                                                      \
            --sp;                                                                                                   \
            node = sp < uint32_t(kOccLdsLevels) ? stackLds[sp * uint32_t(kOccBlock) + tid]                          \
                                                : a.spill[size_t(sp - uint32_t(kOccLdsLevels)) * a.spillStride + gtid]; \
        }                                                                                                           \
    } while (0)

    for (uint32_t iter = 0;; ++iter) {
        if (iter >= a.maxIters) {      // watchdog, like the closest-hit kernels: the wave gives up, the host hears about it at the next synchronisation
            if (lane == 0u) __hip_atomic_fetch_add(a.trips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }

        // ================= refill: idle lanes take the next rays of the wave's chunk =================
        const uint64_t emptyMask = __ballot(node == kEmpty);
        const uint32_t nEmpty = uint32_t(__popcll(emptyMask));
        if (nEmpty == 64u || (nEmpty >= a.refillMin && !(exhausted && wBeg == wEnd))) {
            if (wBeg == wEnd && !exhausted) {
                uint32_t b = 0u;
                if (lane == 0u) b = __hip_atomic_fetch_add(a.cursor, a.chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b = uint32_t(__builtin_amdgcn_readfirstlane(int(b)));
                const uint64_t start = uint64_t(a.dynBase) + b;
                if (start >= uint64_t(a.count)) exhausted = true;
                else { wBeg = uint32_t(start); wEnd = wBeg + min(a.chunk, a.count - wBeg); }
            }
            if (wBeg == wEnd) {
                if (nEmpty == 64u) break;      // no ray left to draw and none in flight
            } else {
                const uint32_t take = min(nEmpty, wEnd - wBeg);
                const uint32_t rank = laneRank(emptyMask);
                if (node == kEmpty && rank < take) {
                    const uint32_t idx = wBeg + rank;
                    float4 q0, q1;
                    loadRay(a.rays, idx, false, q0, q1);
                    const bool valid = isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z) && isfinite(q0.w) &&
                                       isfinite(q1.x) && isfinite(q1.y) && isfinite(q1.z) && !isnan(q1.w);
                    if (!valid) a.occluded[idx] = uint8_t(0);      // rays the oracle rejects (racc_oracle.c:183-191)
                    else {
                        const float eps = 1e-10f;   // Kernels.h:149-157
                        ox = q0.x; oy = q0.y; oz = q0.z; tNear = q0.w;
                        dx = (fabsf(q1.x) < eps) ? copysignf(eps, q1.x) : q1.x;
                        dy = (fabsf(q1.y) < eps) ? copysignf(eps, q1.y) : q1.y;
                        dz = (fabsf(q1.z) < eps) ? copysignf(eps, q1.z) : q1.z;
                        tFar = q1.w;
                        ix = 1.0f / dx; iy = 1.0f / dy; iz = 1.0f / dz;      // Kernels.h:159-160
                        ex = -ox * ix; ey = -oy * iy; ez = -oz * iz;
                        rayIdx = idx;
                        node = 0x80000000u;     // Kernels.h:164
                        sp = 0u;
                    }
                }
                wBeg += take;
            }
        }

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
                if (pairAccepts(t0, t1, t2, ox, oy, oz, dx, dy, dz, tNear, tFar)) { a.occluded[rayIdx] = uint8_t(1); node = kEmpty; }
                else if (cnt > 1u) node = ((cnt - 1u) << 24) | (first + 1u);      // the leaf's remaining pairs
                else RACC_OCC_POP();
            }
        } else if (nInner != 0u) {
            if (isInner) {
                const float4* np = a.nodes + size_t(node & 0x7FFFFFFFu) * 4;
                const uint2 k2 = *reinterpret_cast<const uint2*>(np);
                const float4 d1 = np[1], d2 = np[2], d3 = np[3];
                const float tRay = tFar;
                float tFirst, tLast;
                slabPair(d1, d2, d3, ix, iy, iz, ex, ey, ez, tNear, tRay, tFirst, tLast);
                const float firstDiff = tRay - tFirst, lastDiff = tRay - tLast;
                if (firstDiff + lastDiff != 0.0f) {                               // Kernels.h:192 (tRay = +inf: NaN != 0, descends into `first`)
                    const bool lastNearer = tLast < tFirst;                       // signbit(tLast - tFirst), Kernels.h:193
                    if ((tFirst != tRay) & (tLast != tRay)) {                     // fmax(tFirst, tLast) != tRay, Kernels.h:194: both entered
                        const uint32_t farKid = lastNearer ? k2.x : k2.y;
                        if (sp < uint32_t(kOccLdsLevels)) { stackLds[sp * uint32_t(kOccBlock) + tid] = farKid; ++sp; }
                        else if (sp - uint32_t(kOccLdsLevels) < a.spillLevels) { a.spill[size_t(sp - uint32_t(kOccLdsLevels)) * a.spillStride + gtid] = farKid; ++sp; }
                        // (a validated tree cannot push deeper than its height: the spill area is sized from it)
                    }
                    node = lastNearer ? k2.y : k2.x;
                } else RACC_OCC_POP();
            }
        }
    }
#undef RACC_OCC_POP
}

// Enqueues one occlusion launch on `st`: scratch (cursor word + spill) allocated, zeroed and freed in stream order around the kernel.
int launchOccluded(racc_hip_ctx* ctx, const racc_hip_scene* scene, const void* dRays, uint8_t* dOccluded, uint32_t count, hipStream_t st) {
    if (count > 0xFF000000u) return fail(RACC_HIP_ERR_LIMIT, "occluded: more than 0xFF000000 rays in one launch");      // (the cursor word counts past `count` by at most grid waves x chunk)
    // RACC_OCC_WAVES / RACC_OCC_REFILL / RACC_OCC_LEAF: A/B of the grid size and the two vote thresholds (tools/bench_occlusion.py), results do not depend on them
    static const uint32_t envWaves = [] { const char* e = std::getenv("RACC_OCC_WAVES"); return e && std::atoi(e) > 0 && std::atoi(e) <= 8 ? uint32_t(std::atoi(e)) : kOccWavesPerSimd; }();
    static const uint32_t envRefill = [] { const char* e = std::getenv("RACC_OCC_REFILL"); return e && std::atoi(e) > 0 && std::atoi(e) <= 64 ? uint32_t(std::atoi(e)) : kOccRefillMin; }();
    static const uint32_t envLeaf = [] { const char* e = std::getenv("RACC_OCC_LEAF"); return e && std::atoi(e) > 0 && std::atoi(e) <= 64 ? uint32_t(std::atoi(e)) : kOccLeafMin; }();
    uint32_t blocks = uint32_t(ctx->numCUs) * envWaves;
    const uint32_t blocksNeeded = (count + uint32_t(kOccBlock) - 1u) / uint32_t(kOccBlock);
    if (blocks > blocksNeeded) blocks = blocksNeeded;
    const uint32_t gridThreads = blocks * uint32_t(kOccBlock);
    const uint32_t height = scene->info.inner_height;
    const uint32_t spillLevels = height > uint32_t(kOccLdsLevels) ? height - uint32_t(kOccLdsLevels) : 0u;

    OccludeArgs a;
    a.rays = static_cast<const float4*>(dRays);
    a.occluded = dOccluded;
    a.count = count;
    a.nodes = scene->nodes; a.pairs = scene->pairs;
    a.chunk = count >= (1u << 19) ? 128u : 64u;
    a.dynBase = (gridThreads / 64u) * a.chunk;
    a.spillLevels = spillLevels; a.spillStride = gridThreads;
    a.refillMin = envRefill; a.leafMin = envLeaf;
    a.maxIters = ctx->maxIters;
    a.trips = ctx->devTrips;

    uint32_t* scratch = nullptr;
    const size_t bytes = (size_t(kOccScratchHead) + size_t(spillLevels) * gridThreads) * sizeof(uint32_t);
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), bytes, st), "hipMallocAsync(occlusion scratch)");
    hipError_t e = hipMemsetAsync(scratch, 0, size_t(kOccScratchHead) * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        a.cursor = scratch;
        a.spill = scratch + kOccScratchHead;
        hipLaunchKernelGGL(occludedKernel, dim3(blocks), dim3(kOccBlock), 0, st, a);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, "launch occludedKernel", e);
    if (e2 != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, "hipFreeAsync(occlusion scratch)", e2);
    return RACC_HIP_OK;
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
    // everything of the call is its own (stream, staging arrays): several threads may be in here at once
    hipStream_t st = nullptr;
    void* dRays = nullptr;
    void* dOut = nullptr;
    int rc = RACC_HIP_OK;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&dRays, size_t(count) * 32);
    if (e == hipSuccess) e = hipMalloc(&dOut, size_t(count));
    if (e == hipSuccess) e = hipMemcpyAsync(dRays, rays, size_t(count) * 32, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = launchOccluded(ctx, scene, dRays, static_cast<uint8_t*>(dOut), count, st);
    if (e == hipSuccess && rc == RACC_HIP_OK) e = hipMemcpyAsync(occluded, dOut, size_t(count), hipMemcpyDeviceToHost, st);
    if (st) { const hipError_t es = hipStreamSynchronize(st); if (e == hipSuccess) e = es; }
    if (dRays) hipFree(dRays);
    if (dOut) hipFree(dOut);
    if (st) hipStreamDestroy(st);
    if (rc != RACC_HIP_OK) return rc;
    if (e != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, "occluded (host arrays)", e);
    return checkWatchdog(ctx);
}

}  // extern "C"
