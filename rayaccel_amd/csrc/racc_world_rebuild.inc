// racc_world_rebuild.inc — rebuild of a world's top level on the device, in stream order: an LBVH (Morton codes of the instance box
// centres, a radix sort, Karras's 2012 hierarchy) written into the world's existing allocations, and the C-ABI entries around it
// (racc_hip_world_rebuild*).  Textually included by racc_hip_unit.hip BEHIND racc_world_refit.inc, so it sees the world, the refit handle,
// worldRefitLaunch and kRefitRoot.  Every GPU API's top-level build (and Embree's rtcCommitScene on a scene of instances that changed
// neighbourhoods) is the usual counterpart: what racc_hip_world_update does on the host, without leaving the stream.
//
// The rule is racc_world_rebuild_rule.h's, which racc_host_world_rebuild (world_build.cpp) states top-down; this file reproduces that
// function's nodes, `order`, inv and ray_pad byte for byte.  Five kernels and one sort, nothing waits on anything except through stream
// order, nobody spins:
//   worldRebuildCentresKernel  one thread per INSTANCE: racc_world_rule::instance on its transform and its scene's root box (read from
//                              the device record, as worldRefitKernel does), the centre of its world box into the scratch, the centre
//                              bounds reduced in the wave and folded into six words by one atomic min / max per wave and axis — floats
//                              as ordered integers.  An instance the host rule would refuse is marked disabled.
//   worldRebuildKeysKernel     one thread per instance: its Morton field against the finished bounds, key = field << 32 | index.
//   rocprim::radix_sort_keys   key-only, over the bits the field occupies (32 .. 62).  The keys are formed in index order and the sort
//                              is stable (rocPRIM documents it), so equal fields stay in index order: the order of the whole keys.
//   worldRebuildTreeKernel     one thread per position: order[p] = the low word of key p; for p < count - 1 the record p by Karras's
//                              searches (direction, range end, split; delta = clzll of the XOR of two keys, -1 outside the array):
//                              words 0-1 of the record, parentSlot of its inner children, slots of its leaf children.
//   worldRebuildHeightKernel   one thread per position: the records on its path to the root, counted along parentSlot; the maximum
//                              into the height word (wave-reduced, one atomic max per wave).
//   worldRefitLaunch           unchanged, behind them: the inverses, the boxes up the new tree at the acq_rel counters, the pad.  (It
//                              evaluates the per-instance rule a second time; tools/bench_world_rebuild.py has what that costs.)
// All indices the tree kernel forms stay inside [0, count) whatever the keys hold: delta is -1 outside the array, so no search leaves it.
//
// A disabled instance has the field 2^30 and sorts behind every enabled one; it remains a leaf, with the NaN inverse and the neutral box
// worldRefitKernel gives it.
//
// Stack room.  The host cannot know a device-built tree's height without leaving the stream, so for as long as a rebuild-capable handle
// lives the world's info.height / spill_levels are held at racc_world_rebuild_rule::heightBound (at least what they were): a launch issued
// behind a rebuild always has the levels it needs.  The handle's height word holds the real height of the current topology — written by
// the height kernel, and by worldRebuildHold after a host rebuild — and racc_hip_world_refit_destroy sets info from it.
#include <rocprim/device/device_radix_sort.hpp>

namespace {

namespace rebuild_rule = racc_world_rebuild_rule;
constexpr int kWorldRebuildBlock = 256;
constexpr uint32_t kWorldRebuildWords = 8;      // lo[3], hi[3], height, unused
constexpr uint32_t kWorldRebuildHeightWord = 6;

// floats as unsigned integers of the same order (-0.0 below +0.0: rule 3 lets them stand for each other)
__device__ __forceinline__ uint32_t orderedOf(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float floatOf(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

__device__ __forceinline__ uint32_t waveMin(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t waveMax(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

__global__ void __launch_bounds__(kWorldRebuildBlock) worldRebuildCentresKernel(const float* __restrict__ transforms, const WorldInstDev* __restrict__ table, uint32_t count,
                                                                                float4* __restrict__ centres, uint32_t* words) {
    const uint32_t id = blockIdx.x * uint32_t(kWorldRebuildBlock) + threadIdx.x;
    uint32_t lo[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, hi[3] = { 0u, 0u, 0u };      // neutral: an idle lane, a disabled instance
    if (id < count) {
        float m[12], rb[6], o[12], w[6];
        const float4* t = reinterpret_cast<const float4*>(transforms) + size_t(id) * 3;
        const float4 t0 = t[0], t1 = t[1], t2 = t[2];
        m[0] = t0.x; m[1] = t0.y; m[2] = t0.z; m[3] = t0.w; m[4] = t1.x; m[5] = t1.y; m[6] = t1.z; m[7] = t1.w; m[8] = t2.x; m[9] = t2.y; m[10] = t2.z; m[11] = t2.w;
        const float4* root = table[id].nodes;      // device record 0 = the root: words 4-15 = Lx Ly Lz Rx Ry Rz as (min, max)
        const float4 r1 = root[1], r2 = root[2], r3 = root[3];
        const float rec[12] = { r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w };
#pragma unroll
        for (int k = 0; k < 3; ++k) {      // as worldCommit and worldRefitKernel form it
            rb[k] = rec[2 * k] < rec[6 + 2 * k] ? rec[2 * k] : rec[6 + 2 * k];
            rb[3 + k] = rec[1 + 2 * k] > rec[7 + 2 * k] ? rec[1 + 2 * k] : rec[7 + 2 * k];
        }
        double cond = 0.0;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 1.0f);      // w != 0: disabled
        if (racc_world_rule::instance(m, rb, o, w, cond) == racc_world_rule::kOk) {
            c = make_float4(rebuild_rule::centre(w[0], w[3]), rebuild_rule::centre(w[1], w[4]), rebuild_rule::centre(w[2], w[5]), 0.0f);
            lo[0] = hi[0] = orderedOf(c.x); lo[1] = hi[1] = orderedOf(c.y); lo[2] = hi[2] = orderedOf(c.z);
        }
        centres[id] = c;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {      // every lane of the wave is here
        const uint32_t mn = waveMin(lo[k]), mx = waveMax(hi[k]);
        if ((threadIdx.x & 63u) == 0u && mn <= mx) {      // (mn > mx: no enabled instance in this wave)
            __hip_atomic_fetch_min(words + k, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(words + 3 + k, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void __launch_bounds__(kWorldRebuildBlock) worldRebuildKeysKernel(const float4* __restrict__ centres, const uint32_t* __restrict__ words, uint32_t count,
                                                                             unsigned long long* __restrict__ keys) {
    const uint32_t id = blockIdx.x * uint32_t(kWorldRebuildBlock) + threadIdx.x;
    if (id >= count) return;
    const float4 c = centres[id];
    uint32_t f = rebuild_rule::kDisabledField;
    if (c.w == 0.0f) {      // (then the bounds hold at least this centre)
        const float cc[3] = { c.x, c.y, c.z };
        const float lo[3] = { floatOf(words[0]), floatOf(words[1]), floatOf(words[2]) }, hi[3] = { floatOf(words[3]), floatOf(words[4]), floatOf(words[5]) };
        f = rebuild_rule::field(cc, lo, hi);
    }
    keys[id] = rebuild_rule::key(f, id);
}

// Karras's delta: the leading bits key[i] and key[j] share, -1 for a j outside the array.  (The keys are unique.)
__device__ __forceinline__ int worldRebuildDelta(const unsigned long long* __restrict__ keys, int n, unsigned long long ki, int j) {
    return (j < 0 || j >= n) ? -1 : rebuild_rule::commonPrefix(ki, keys[j]);
}

__global__ void __launch_bounds__(kWorldRebuildBlock) worldRebuildTreeKernel(const unsigned long long* __restrict__ keys, uint32_t count, float4* __restrict__ topNodes,
                                                                             uint32_t* __restrict__ order, uint32_t* __restrict__ slots, uint32_t* __restrict__ parentSlot) {
    const uint32_t p = blockIdx.x * uint32_t(kWorldRebuildBlock) + threadIdx.x;
    if (p >= count) return;
    const unsigned long long ki = keys[p];
    order[p] = uint32_t(ki);
    if (p == 0u) parentSlot[0] = kRefitRoot;
    if (count == 1u) {      // record 0 = {the leaf, the empty reference}; the empty reference's box is never read and stays what it is
        *reinterpret_cast<uint2*>(topNodes) = make_uint2((1u << 24) | 0u, 0u);
        slots[0] = 0u;
        return;
    }
    if (p + 1u >= count) return;
    const int n = int(count), i = int(p);
    // the direction of the range and a bound of its length
    const int d = worldRebuildDelta(keys, n, ki, i + 1) > worldRebuildDelta(keys, n, ki, i - 1) ? 1 : -1;
    const int deltaMin = worldRebuildDelta(keys, n, ki, i - d);
    int lMax = 2;
    while (worldRebuildDelta(keys, n, ki, i + lMax * d) > deltaMin) lMax <<= 1;      // (at most 2^21: count <= 2^20)
    // the other end, by binary search
    int l = 0;
    for (int t = lMax >> 1; t >= 1; t >>= 1)
        if (worldRebuildDelta(keys, n, ki, i + (l + t) * d) > deltaMin) l += t;
    const int j = i + l * d;
    // the split: the last position, seen from i, that shares more than the range's common prefix with key[i]
    const int deltaNode = worldRebuildDelta(keys, n, ki, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (worldRebuildDelta(keys, n, ki, i + (s + t) * d) > deltaNode) s += t;
    } while (t > 1);
    const int split = i + s * d + (d < 0 ? -1 : 0);      // first child [a, split], last child [split + 1, b]
    const int a = d > 0 ? i : j, b = d > 0 ? j : i;
    uint32_t first, last;
    if (a == split) { first = (1u << 24) | uint32_t(split); slots[split] = p * 2u; }
    else { first = 0x80000000u | uint32_t(split); parentSlot[split] = p * 2u; }
    if (b == split + 1) { last = (1u << 24) | uint32_t(split + 1); slots[split + 1] = p * 2u + 1u; }
    else { last = 0x80000000u | uint32_t(split + 1); parentSlot[split + 1] = p * 2u + 1u; }
    *reinterpret_cast<uint2*>(topNodes + size_t(p) * 4) = make_uint2(first, last);
}

// `maxLevels` = the bound of the rule: no path is longer, so the walk ends whatever the tables hold.
__global__ void __launch_bounds__(kWorldRebuildBlock) worldRebuildHeightKernel(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ parentSlot, uint32_t count,
                                                                               uint32_t maxLevels, uint32_t* heightWord) {
    const uint32_t p = blockIdx.x * uint32_t(kWorldRebuildBlock) + threadIdx.x;
    uint32_t levels = 0u;
    if (p < count) {
        uint32_t rec = slots[p] >> 1;
        levels = 1u;
        while (levels < maxLevels) {
            const uint32_t up = parentSlot[rec];
            if (up == kRefitRoot) break;
            rec = up >> 1;
            ++levels;
        }
    }
    levels = waveMax(levels);
    if ((threadIdx.x & 63u) == 0u && levels) __hip_atomic_fetch_max(heightWord, levels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

uint32_t worldRebuildSpillOf(uint32_t height) { return height + 1u > uint32_t(kWorldTopLds) ? height + 1u - uint32_t(kWorldTopLds) : 0u; }

hipError_t worldRebuildSort(WorldRefit* r, void* temp, size_t& bytes, hipStream_t st) {
    const uint32_t count = r->world->count;
    return rocprim::radix_sort_keys(temp, bytes, r->keys, r->keys + count, size_t(count), rebuild_rule::kKeyLowBit, rebuild_rule::kKeyEndBit, st);
}

int worldRebuildLaunch(WorldRefit* r, const float* dTransforms, hipStream_t st) {
    const racc_hip_world* w = r->world;
    const uint32_t count = w->count;
    const dim3 grid((count + kWorldRebuildBlock - 1) / kWorldRebuildBlock), block(kWorldRebuildBlock);
    HIP_TRY(hipMemsetAsync(r->rebuildWords, 0xFF, 12, st), "hipMemsetAsync(world rebuild bounds)");
    HIP_TRY(hipMemsetAsync(r->rebuildWords + 3, 0, (kWorldRebuildWords - 3) * 4, st), "hipMemsetAsync(world rebuild bounds)");
    hipLaunchKernelGGL(worldRebuildCentresKernel, grid, block, 0, st, dTransforms, w->table, count, r->centres, r->rebuildWords);
    HIP_TRY(hipGetLastError(), "launch worldRebuildCentresKernel");
    hipLaunchKernelGGL(worldRebuildKeysKernel, grid, block, 0, st, r->centres, r->rebuildWords, count, r->keys);
    HIP_TRY(hipGetLastError(), "launch worldRebuildKeysKernel");
    size_t bytes = r->sortTempBytes;
    HIP_TRY(worldRebuildSort(r, r->sortTemp, bytes, st), "radix_sort_keys(world rebuild)");
    hipLaunchKernelGGL(worldRebuildTreeKernel, grid, block, 0, st, r->keys + count, count, w->topNodes, w->order, r->slots, r->parentSlot);
    HIP_TRY(hipGetLastError(), "launch worldRebuildTreeKernel");
    hipLaunchKernelGGL(worldRebuildHeightKernel, grid, block, 0, st, r->slots, r->parentSlot, count, rebuild_rule::heightBound(count, true), r->rebuildWords + kWorldRebuildHeightWord);
    HIP_TRY(hipGetLastError(), "launch worldRebuildHeightKernel");
    return worldRefitLaunch(r, dTransforms, st);
}

void worldRebuildFree(WorldRefit* r) {
    if (r->centres) hipFree(r->centres);
    if (r->keys) hipFree(r->keys);
    if (r->sortTemp) hipFree(r->sortTemp);
    if (r->rebuildWords) hipFree(r->rebuildWords);
}

// racc_world.inc's worldCommit ends here: a host rebuild under a live rebuild-capable handle.  info holds what the host built.
int worldRebuildHold(racc_hip_world* w) {
    WorldRefit* r = w->refit;
    if (!r || !r->rebuildWords) return RACC_HIP_OK;
    HIP_TRY(hipMemcpy(r->rebuildWords + kWorldRebuildHeightWord, &w->info.height, 4, hipMemcpyHostToDevice), "hipMemcpy(world rebuild height)");
    const uint32_t bound = rebuild_rule::heightBound(w->count, true);
    if (w->info.height < bound) w->info.height = bound;
    if (w->info.spill_levels < worldRebuildSpillOf(bound)) w->info.spill_levels = worldRebuildSpillOf(bound);
    return RACC_HIP_OK;
}

// racc_hip_world_refit_destroy, after its device synchronisation: the real height back into the world.
void worldRebuildLeave(WorldRefit* r) {
    if (!r->rebuildWords) return;
    uint32_t height = 0;
    if (hipMemcpy(&height, r->rebuildWords + kWorldRebuildHeightWord, 4, hipMemcpyDeviceToHost) != hipSuccess || !height) return;
    r->world->info.height = height;
    r->world->info.spill_levels = worldRebuildSpillOf(height);
}

}  // namespace

extern "C" {

int racc_hip_world_rebuild_create(racc_hip_ctx* ctx, racc_hip_world* w, WorldRefit** out) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_create: ctx is NULL");
    if (!out) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_create: out is NULL");
    *out = nullptr;
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_create: world is NULL");
    WorldRefit* r = nullptr;
    if (int rc = racc_hip_world_refit_create(ctx, w, &r)) return rc;      // (the plain handle's refusals, under its name)
    const uint32_t count = w->count;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->centres), size_t(count) * 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->keys), size_t(count) * 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rebuildWords), kWorldRebuildWords * 4);
    if (e == hipSuccess) e = hipMemset(r->rebuildWords, 0, kWorldRebuildWords * 4);
    if (e == hipSuccess) e = worldRebuildSort(r, nullptr, r->sortTempBytes, r->stream);      // the size query: nothing runs
    if (e == hipSuccess) e = hipMalloc(&r->sortTemp, r->sortTempBytes ? r->sortTempBytes : 4);
    int rc = e == hipSuccess ? worldRebuildHold(w) : fail(RACC_HIP_ERR_DEVICE, "world_rebuild_create", e);
    if (rc) {      // back to a world without a handle (a plain handle's destroy: the scratch that exists goes with it, info is untouched)
        worldRebuildFree(r);
        r->centres = nullptr; r->keys = nullptr; r->sortTemp = nullptr; r->rebuildWords = nullptr;
        racc_hip_world_refit_destroy(ctx, r);
        return rc;
    }
    *out = r;
    return RACC_HIP_OK;
}

int racc_hip_world_rebuild_device(racc_hip_ctx* ctx, WorldRefit* r, const void* d_transforms12, uint32_t count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_device: ctx is NULL");
    if (!r || !d_transforms12) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_device: refit/d_transforms12 is NULL");
    if (r->world->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_device: the world belongs to another context");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_device: the handle was made by racc_hip_world_refit_create: racc_hip_world_rebuild_create makes one that can rebuild");
    if (count != r->world->count) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_device: count differs from the world's instance count");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return worldRebuildLaunch(r, static_cast<const float*>(d_transforms12), static_cast<hipStream_t>(stream));
}

int racc_hip_world_rebuild(racc_hip_ctx* ctx, WorldRefit* r, const float* transforms12, uint32_t count) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild: ctx is NULL");
    if (!r || !transforms12) return fail(RACC_HIP_ERR_INVALID, "world_rebuild: refit/transforms is NULL");
    racc_hip_world* w = r->world;
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild: the world belongs to another context");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "world_rebuild: the handle was made by racc_hip_world_refit_create: racc_hip_world_rebuild_create makes one that can rebuild");
    if (count != w->count) return fail(RACC_HIP_ERR_INVALID, "world_rebuild: count differs from the world's instance count");
    if (int rc = racc_hip_synchronize(ctx)) return rc;      // no kernel reads the top level or a root box while they change
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    // validated with the host rule before anything changes: a refused transform leaves the world as it was
    std::vector<float> rootBoxes, inv(size_t(count) * 12), boxes(size_t(count) * 6);
    if (int rc = worldRootBoxes(w, rootBoxes)) return rc;
    float pad = 0.0f;
    if (int rc = racc_host_world_instances_("racc_hip_world_rebuild", transforms12, rootBoxes.data(), count, inv.data(), boxes.data(), &pad)) return rc;
    if (!r->transforms) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->transforms), size_t(count) * 48), "hipMalloc(world rebuild transforms)");
    HIP_TRY(hipMemcpyAsync(r->transforms, transforms12, size_t(count) * 48, hipMemcpyHostToDevice, r->stream), "hipMemcpyAsync(world rebuild transforms)");
    if (int rc = worldRebuildLaunch(r, r->transforms, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream), "hipStreamSynchronize(world rebuild)");
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_rebuild: out of host memory");
}

int racc_hip_world_rebuild_check(racc_hip_ctx* ctx, WorldRefit* r, uint32_t* height, uint32_t* disabled_instances) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_check: ctx is NULL");
    if (!r || !height || !disabled_instances) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_check: refit/height/disabled_instances is NULL");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "world_rebuild_check: the handle was made by racc_hip_world_refit_create");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(height, r->rebuildWords + kWorldRebuildHeightWord, 4, hipMemcpyDeviceToHost), "hipMemcpy(height)");
    HIP_TRY(hipMemcpy(disabled_instances, r->state + 1, 4, hipMemcpyDeviceToHost), "hipMemcpy(disabled instances)");
    return RACC_HIP_OK;
}

}  // extern "C"
