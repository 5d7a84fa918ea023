// racc_query.inc — what the plain-HIP query kernels (occludedKernel, worldIntersectKernel) and their entries share: the wavefront scaffold
// on the device — ray feed, ray admission, lane stack, BVH2 inner step, watchdog — and the launch plumbing on the host.  Textually included
// by racc_hip_unit.hip BEHIND racc_hip.hip and racc_scene_registry.inc, so it sees the context, fail() / HIP_TRY / checkWatchdog and the
// helpers of racc_device.inc, and changes none of them.  A new query kernel is assembled from these pieces; what it owns is its vote, its
// leaf step and what an empty stack means.  Arithmetic is expression for expression that of the closest-hit kernels (explicit fmaf only,
// -ffp-contract=off).

namespace {

struct QueryFeedArgs {        // the ray feed's part of a query kernel's arguments (host side: queryGrid, withQueryScratch)
    uint32_t count;
    uint32_t* cursor;         // one zeroed word per launch
    uint32_t dynBase;         // rays handed out statically (grid waves x chunk): the cursor counts from here
    uint32_t chunk;           // rays per dequeue, a multiple of 64
    uint32_t refillMin;       // idle lanes that trigger a refill
};

// Ray feed: the wave's current chunk [wBeg, wEnd) and whether the cursor has run past the last ray.
struct RayFeed {
    uint32_t wBeg, wEnd;
    bool exhausted;

    // the first chunk is assigned statically (no start-up stampede on the cursor word)
    __device__ __forceinline__ void start(const QueryFeedArgs& a, uint32_t gwave) {
        wBeg = gwave * a.chunk;
        if (wBeg >= a.count) { wBeg = 0u; wEnd = 0u; }
        else wEnd = wBeg + min(a.chunk, a.count - wBeg);
        exhausted = a.dynBase >= a.count;
    }

    // One refill round of the wave; `idle` = this lane holds no ray.  Idle lanes take the next rays of the chunk in lane order: admit(idx)
    // runs in every lane that gets ray idx.  False: no ray left to draw and none in flight, the wave leaves.
    template <class Admit>
    __device__ __forceinline__ bool refill(const QueryFeedArgs& a, bool idle, uint32_t lane, Admit&& admit) {
        const uint64_t emptyMask = __ballot(idle);
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
                if (nEmpty == 64u) return false;
            } else {
                const uint32_t take = min(nEmpty, wEnd - wBeg);
                const uint32_t rank = laneRank(emptyMask);
                if (idle && rank < take) admit(wBeg + rank);
                wBeg += take;
            }
        }
        return true;
    }
};

// Ray admission: loads ray `idx`; false for the rays the oracle rejects (racc_oracle.c:183-191).
__device__ __forceinline__ bool admitRay(const float4* rays, uint32_t idx, float4& q0, float4& q1) {
    loadRay(rays, idx, false, q0, q1);
    return isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z) && isfinite(q0.w) &&
           isfinite(q1.x) && isfinite(q1.y) && isfinite(q1.z) && !isnan(q1.w);
}

__device__ __forceinline__ float clampDir(float d) {      // Kernels.h:149-157
    const float eps = 1e-10f;
    return (fabsf(d) < eps) ? copysignf(eps, d) : d;
}

// A lane's ray from an origin and a direction: the clamp, then 1/d, then -o/d, in that order (Kernels.h:149-160).  No hit yet.
__device__ __forceinline__ void setLaneRay(LaneRay& r, float ox, float oy, float oz, float dx, float dy, float dz, float tNear, float tFar) {
    r.ox = ox; r.oy = oy; r.oz = oz; r.tNear = tNear;
    r.dx = clampDir(dx); r.dy = clampDir(dy); r.dz = clampDir(dz);
    r.tFar = tFar;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    r.ex = -r.ox * r.ix; r.ey = -r.oy * r.iy; r.ez = -r.oz * r.iz;
    r.hitIndex = -1; r.hitU = 0.0f; r.hitV = 0.0f;
}

// Per-lane stack of node references: the first kLdsLevels levels are this thread's column of a [level][kBlock] LDS array
// (conflict-free), deeper ones its column of a global spill [spillLevels][stride].
template <int kLdsLevels, int kBlock>
struct LaneStack {
    uint32_t* ldsColumn;      // lds + tid
    uint32_t* spill;
    uint32_t spillLevels, stride, gtid;
    uint32_t height;

    __device__ __forceinline__ void push(uint32_t ref) {
        if (height < uint32_t(kLdsLevels)) { ldsColumn[height * uint32_t(kBlock)] = ref; ++height; }
        else if (height - uint32_t(kLdsLevels) < spillLevels) { spill[size_t(height - uint32_t(kLdsLevels)) * stride + gtid] = ref; ++height; }
        // (a validated tree cannot push deeper than its height, a top-level tree than its height + 1: the spill area is sized from it)
    }
    __device__ __forceinline__ bool pop(uint32_t& ref) {
        if (height == 0u) return false;
        --height;
        ref = height < uint32_t(kLdsLevels) ? ldsColumn[height * uint32_t(kBlock)]
                                            : spill[size_t(height - uint32_t(kLdsLevels)) * stride + gtid];
        return true;
    }
};

// One BVH2 inner step of the closest-hit kernels (racc_kernel_v8.inc's C++ iteration): `node` is an inner reference into the 64 B device
// records `nodes` (racc_device.inc, slabPair), tRay the limit the boxes are tested with.  True: `node` is the next node and the far child
// is on the stack if both were entered.  False: neither was, the caller pops.
template <class Stack>
__device__ __forceinline__ bool bvh2InnerStep(const float4* nodes, uint32_t& node, const LaneRay& r, float tRay, Stack& stack) {
    const float4* np = nodes + size_t(node & 0x7FFFFFFFu) * 4;
    const uint2 k2 = *reinterpret_cast<const uint2*>(np);
    const float4 d1 = np[1], d2 = np[2], d3 = np[3];
    float tFirst, tLast;
    slabPair(d1, d2, d3, r.ix, r.iy, r.iz, r.ex, r.ey, r.ez, r.tNear, tRay, tFirst, tLast);
    const float firstDiff = tRay - tFirst, lastDiff = tRay - tLast;
    if (firstDiff + lastDiff != 0.0f) {                               // Kernels.h:192 (tRay = +inf: NaN != 0, descends into `first`)
        const bool lastNearer = tLast < tFirst;                       // signbit(tLast - tFirst), Kernels.h:193
        if ((tFirst != tRay) & (tLast != tRay))                       // fmax(tFirst, tLast) != tRay, Kernels.h:194: both entered
            stack.push(lastNearer ? k2.x : k2.y);
        node = lastNearer ? k2.y : k2.x;
        return true;
    }
    return false;
}

// Watchdog, like the closest-hit kernels: true = the wave gives up, the host hears about it at the next synchronisation.
__device__ __forceinline__ bool watchdogTripped(uint32_t iter, uint32_t maxIters, uint32_t* trips, uint32_t lane) {
    if (iter < maxIters) return false;
    if (lane == 0u) __hip_atomic_fetch_add(trips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return true;
}

constexpr uint32_t kQueryScratchHead = 64;      // words in front of the spill area: word 0 = the ray cursor

// A/B tunable from the environment (tools/bench_occlusion.py, tools/bench_world.py): an integer in [lo, hi], else the default.  Results
// do not depend on any of them.  Call sites keep the value in a `static const`: the environment is read once per process.
uint32_t queryTunable(const char* name, int lo, int hi, uint32_t fallback) {
    const char* e = std::getenv(name);
    const int v = e ? std::atoi(e) : lo - 1;
    return v >= lo && v <= hi ? uint32_t(v) : fallback;
}

struct QueryGrid { uint32_t blocks, gridThreads; };

// Grid of a query launch — wavesPerSimd workgroups of `block` threads (four waves) per CU, no more than the rays need — and the feed's
// count, chunk and dynBase for it.  `limitMsg` is the refusal of a launch whose cursor word could wrap (it counts past `count` by at most
// grid waves x chunk).
int queryGrid(const racc_hip_ctx* ctx, uint32_t count, uint32_t block, uint32_t wavesPerSimd, const char* limitMsg, QueryGrid& g, QueryFeedArgs& feed) {
    if (count > 0xFF000000u) return fail(RACC_HIP_ERR_LIMIT, limitMsg);
    feed.count = count;
    g.blocks = uint32_t(ctx->numCUs) * wavesPerSimd;
    const uint32_t blocksNeeded = (count + block - 1u) / block;
    if (g.blocks > blocksNeeded) g.blocks = blocksNeeded;
    g.gridThreads = g.blocks * block;
    feed.chunk = count >= (1u << 19) ? 128u : 64u;
    feed.dynBase = (g.gridThreads / 64u) * feed.chunk;
    return RACC_HIP_OK;
}

// The launch's scratch, in stream order on `st`: kQueryScratchHead zeroed words + spillWords allocated, launch(scratch) — which enqueues
// the kernel —, freed.  The free is always issued; a launch error is reported before a free error.
template <class Launch>
int withQueryScratch(size_t spillWords, hipStream_t st, const char* launchMsg, Launch&& launch) {
    uint32_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scratch), (size_t(kQueryScratchHead) + spillWords) * sizeof(uint32_t), st), "hipMallocAsync(query scratch)");
    hipError_t e = hipMemsetAsync(scratch, 0, size_t(kQueryScratchHead) * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        launch(scratch);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, launchMsg, e);
    if (e2 != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, "hipFreeAsync(query scratch)", e2);
    return RACC_HIP_OK;
}

// What a blocking entry owns on the device: a private non-blocking stream, the staged rays and up to two staged output arrays.
// Everything of the call is its own, so several threads may be in such an entry at once; everything is freed on every path.
struct QueryStaging {
    hipStream_t st = nullptr;
    void* dev[3] = {nullptr, nullptr, nullptr};      // rays, outputs
    ~QueryStaging() {
        for (void* p : dev) if (p) hipFree(p);
        if (st) hipStreamDestroy(st);
    }
};

// A blocking entry: copies `rays` in, enqueue(dRays, dOut0, dOut1, stream) -> rc puts the query on the stream, the outputs are copied to
// out0 / out1 (bytes1 may be 0) and the stream is synchronised.  Reports the enqueue's rc first, then the first HIP error (as `what`),
// then the watchdog.
template <class Enqueue>
int runStagedQuery(racc_hip_ctx* ctx, const char* what, const void* rays, uint32_t count, void* out0, size_t bytes0, void* out1, size_t bytes1, Enqueue&& enqueue) {
    void* const host[3] = {nullptr, out0, out1};
    const size_t bytes[3] = {size_t(count) * 32, bytes0, bytes1};
    int rc = RACC_HIP_OK;
    hipError_t e;
    {
        QueryStaging s;
        e = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking);
        for (int i = 0; i < 3; ++i)
            if (e == hipSuccess && bytes[i]) e = hipMalloc(&s.dev[i], bytes[i]);
        if (e == hipSuccess) e = hipMemcpyAsync(s.dev[0], rays, bytes[0], hipMemcpyHostToDevice, s.st);
        if (e == hipSuccess) rc = enqueue(s.dev[0], s.dev[1], s.dev[2], s.st);
        for (int i = 1; i < 3; ++i)
            if (e == hipSuccess && rc == RACC_HIP_OK && bytes[i]) e = hipMemcpyAsync(host[i], s.dev[i], bytes[i], hipMemcpyDeviceToHost, s.st);
        if (s.st) { const hipError_t es = hipStreamSynchronize(s.st); if (e == hipSuccess) e = es; }
    }
    if (rc != RACC_HIP_OK) return rc;
    if (e != hipSuccess) return fail(RACC_HIP_ERR_DEVICE, what, e);
    return checkWatchdog(ctx);
}

}  // namespace
