// racc_world_refit.inc — refit of a world's top level to moved instances, on the device: worldRefitKernel, worldRefitPadKernel and the
// C-ABI entries around them (racc_hip_world_refit*, racc_hip_world_download).  Textually included by racc_hip_unit.hip BEHIND
// racc_world_occlusion.inc, so it sees the world, refitMin / refitMax and kRefitRoot of racc_refit.inc and fail() / HIP_TRY.  Embree's
// rtcCommitScene on a scene of moved instances and every GPU API's top-level update are the usual counterparts.
//
// The rule is racc_host_world_refit's (world_build.cpp), reproduced bit for bit: topology unchanged; per instance the inverse, the
// conservative world box and the condition number by racc_world_rule.h — the very function the host compiles, in double, nothing
// contracted; a leaf child's box the world box of its instance, an inner child's box the union of that node's first-child box
// (accumulator) with its last-child box by the select of racc_refit.inc; ray_pad from the largest condition number.
//
// All refit state lives in the racc_hip_world_refit handle: per `order` position the slot (2 * device record + side) its box goes to,
// per top-level record its own slot in its parent, one arrival counter per record, a 64-bit word for the largest condition number (as its
// bit pattern: non-negative doubles order like their bits), a counter of disabled instances and the 4-byte word the world kernels read
// the pad from while the handle lives.  The world's own allocations do not change.
//
// worldRefitKernel: one thread per `order` position.  It reads its instance's root box from the member scene's root record on the device
// (a refitted member scene is picked up without a host step), evaluates the rule, writes inv, folds the condition number into the max
// word (one wave-reduced agent-scope atomic max), writes its six planes into the parent's record and climbs exactly as refitBoxesKernel
// does: an agent-scope acq_rel fetch_add on the parent's counter, the first arriver retires, the second one unions first-child-first and
// goes on.  Nobody spins.  An instance the host rule would refuse is disabled: inv = twelve NaNs (every transformed ray is rejected at
// admission), world box = {+inf, +inf, +inf, -inf, -inf, -inf} (neutral under the select), not in the max, counted.  The topology is
// never written.  Counters, the max word and the disabled counter are zeroed in stream order before the kernel; worldRefitPadKernel
// behind it writes the pad word.

struct racc_hip_world_refit {
    racc_hip_world* world = nullptr;
    uint32_t* slots = nullptr;                // [count] per `order` position: 2 * device record + side
    uint32_t* parentSlot = nullptr;           // [capacity] per top-level record: its own slot in its parent, kRefitRoot for the root
    unsigned long long* state = nullptr;      // {max condition number (bits); disabled counter, 4 B unused; arrival counters [capacity]}: zeroed before every refit
    float* rayPad = nullptr;                  // the device word the world kernels read
    float* transforms = nullptr;              // staging of the blocking entry, allocated at its first call
    hipStream_t stream = nullptr;             // ... and its stream
    // the scratch of the device rebuild (racc_world_rebuild.inc): all NULL on a handle racc_hip_world_refit_create made
    float4* centres = nullptr;                // [count] per instance: its box centre, w != 0 for a disabled instance
    unsigned long long* keys = nullptr;       // [2][count]: as formed, then sorted
    void* sortTemp = nullptr;                 // the radix sort's temporary storage, sized at creation ...
    size_t sortTempBytes = 0;                 // ... to this
    uint32_t* rebuildWords = nullptr;         // {centre bounds lo[3], hi[3] as ordered integers; height; unused}
};

namespace {

using WorldRefit = struct racc_hip_world_refit;      // (the bare name is the blocking entry's)
constexpr int kWorldRefitBlock = 256;

__device__ __forceinline__ uint32_t* worldRefitDisabled(unsigned long long* state) { return reinterpret_cast<uint32_t*>(state + 1); }
__device__ __forceinline__ uint32_t* worldRefitCounters(unsigned long long* state) { return reinterpret_cast<uint32_t*>(state + 2); }
size_t worldRefitStateBytes(uint32_t capacity) { return 16 + size_t(capacity) * 4; }

// racc_world_rebuild.inc: frees the rebuild's scratch; at destroy, the real height read back into the world's info.
void worldRebuildFree(struct racc_hip_world_refit* r);
void worldRebuildLeave(struct racc_hip_world_refit* r);

__global__ void __launch_bounds__(kWorldRefitBlock) worldRefitKernel(const float* __restrict__ transforms, const WorldInstDev* __restrict__ table,
                                                                     const uint32_t* __restrict__ order, const uint32_t* __restrict__ slots, uint32_t count,
                                                                     const uint32_t* __restrict__ parentSlot, unsigned long long* state,
                                                                     float4* __restrict__ inv, float* nodes) {
    const uint32_t i = blockIdx.x * uint32_t(kWorldRefitBlock) + threadIdx.x;
    const bool active = i < count;
    float mnx = INFINITY, mny = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxy = -INFINITY, mxz = -INFINITY;
    unsigned long long condBits = 0ull;
    bool isDisabled = false;
    if (active) {
        const uint32_t id = order[i];
        float m[12], rb[6], o[12], w[6];
        const float4* t = reinterpret_cast<const float4*>(transforms) + size_t(id) * 3;
        const float4 t0 = t[0], t1 = t[1], t2 = t[2];
        m[0] = t0.x; m[1] = t0.y; m[2] = t0.z; m[3] = t0.w; m[4] = t1.x; m[5] = t1.y; m[6] = t1.z; m[7] = t1.w; m[8] = t2.x; m[9] = t2.y; m[10] = t2.z; m[11] = t2.w;
        const float4* root = table[id].nodes;      // device record 0 = the root: words 4-15 = Lx Ly Lz Rx Ry Rz as (min, max)
        const float4 r1 = root[1], r2 = root[2], r3 = root[3];
        const float rec[12] = { r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w };
#pragma unroll
        for (int k = 0; k < 3; ++k) {      // as worldCommit forms it
            rb[k] = rec[2 * k] < rec[6 + 2 * k] ? rec[2 * k] : rec[6 + 2 * k];
            rb[3 + k] = rec[1 + 2 * k] > rec[7 + 2 * k] ? rec[1 + 2 * k] : rec[7 + 2 * k];
        }
        double cond = 0.0;
        if (racc_world_rule::instance(m, rb, o, w, cond) == racc_world_rule::kOk) {
            condBits = static_cast<unsigned long long>(__double_as_longlong(cond));
            mnx = w[0]; mny = w[1]; mnz = w[2]; mxx = w[3]; mxy = w[4]; mxz = w[5];
        } else {
            isDisabled = true;
            const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = nan;
        }
        float4* out = inv + size_t(id) * 3;
        out[0] = make_float4(o[0], o[1], o[2], o[3]);
        out[1] = make_float4(o[4], o[5], o[6], o[7]);
        out[2] = make_float4(o[8], o[9], o[10], o[11]);
    }
    // the wave's largest condition number and its disabled instances: one atomic each per wave (every lane of the wave is here)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(condBits, off, 64);
        condBits = other > condBits ? other : condBits;
    }
    const uint32_t nDisabled = uint32_t(__popcll(__ballot(isDisabled)));
    if ((threadIdx.x & 63u) == 0u) {
        if (condBits) __hip_atomic_fetch_max(state, condBits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nDisabled) __hip_atomic_fetch_add(worldRefitDisabled(state), nDisabled, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!active) return;
    uint32_t* counters = worldRefitCounters(state);
    uint32_t slot = slots[i];
    for (;;) {
        const uint32_t rec = slot >> 1;
        float* planes = nodes + size_t(rec) * 16 + 4 + (slot & 1u) * 6;
        planes[0] = mnx; planes[1] = mxx; planes[2] = mny; planes[3] = mxy; planes[4] = mnz; planes[5] = mxz;
        // release: the planes above are visible to whoever reads this counter next; acquire: the sibling's planes are visible to us
        const uint32_t arrived = __hip_atomic_fetch_add(counters + rec, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == 0u) return;                   // the sibling's subtree is not finished: whoever finishes it goes on from here
        const uint32_t up = parentSlot[rec];
        if (up == kRefitRoot) return;
        const float* b = nodes + size_t(rec) * 16 + 4;      // first child's planes (accumulator), then the last child's
        mnx = refitMin(b[0], b[6]); mxx = refitMax(b[1], b[7]);
        mny = refitMin(b[2], b[8]); mxy = refitMax(b[3], b[9]);
        mnz = refitMin(b[4], b[10]); mxz = refitMax(b[5], b[11]);
        slot = up;
    }
}

// One thread, behind worldRefitKernel in stream order: the pad of the largest condition number into the word the world kernels read.
__global__ void worldRefitPadKernel(const unsigned long long* __restrict__ state, float* rayPad) {
    *rayPad = racc_world_rule::rayPadOf(__longlong_as_double(static_cast<long long>(state[0])));
}

int worldRefitLaunch(WorldRefit* r, const float* dTransforms, hipStream_t st) {
    const racc_hip_world* w = r->world;
    const uint32_t capacity = w->count > 1u ? w->count - 1u : 1u;
    HIP_TRY(hipMemsetAsync(r->state, 0, worldRefitStateBytes(capacity), st), "hipMemsetAsync(world refit state)");
    hipLaunchKernelGGL(worldRefitKernel, dim3((w->count + kWorldRefitBlock - 1) / kWorldRefitBlock), dim3(kWorldRefitBlock), 0, st, dTransforms, w->table, w->order, r->slots,
                       w->count, r->parentSlot, r->state, w->inv, reinterpret_cast<float*>(w->topNodes));
    HIP_TRY(hipGetLastError(), "launch worldRefitKernel");
    hipLaunchKernelGGL(worldRefitPadKernel, dim3(1), dim3(1), 0, st, r->state, r->rayPad);
    HIP_TRY(hipGetLastError(), "launch worldRefitPadKernel");
    return RACC_HIP_OK;
}

// The handle's tables from the top level's device records (`dev`, on the host) and the pad into its word.  Blocking copies.
int worldRefitRebuild(racc_hip_world* w, const uint32_t* dev, float rayPad) try {
    WorldRefit* r = w->refit;
    const uint32_t count = w->count, capacity = count > 1u ? count - 1u : 1u;
    std::vector<uint32_t> slots(count, kRefitRoot), parentSlot(capacity, kRefitRoot);
    std::vector<uint32_t> work;
    work.push_back(0u);
    uint32_t reached = 1;
    while (!work.empty()) {
        const uint32_t d = work.back();
        work.pop_back();
        for (uint32_t side = 0; side < 2; ++side) {
            const uint32_t c = dev[size_t(d) * 16 + side];
            if (c & 0x80000000u) {
                const uint32_t ci = c & 0x7FFFFFFFu;
                if (ci >= capacity || ci == 0u || parentSlot[ci] != kRefitRoot) return fail(RACC_HIP_ERR_INVALID, "world_refit: the top-level records are not a tree");
                parentSlot[ci] = d * 2u + side;
                work.push_back(ci);
                ++reached;
            } else if (c >> 24) {
                const uint32_t first = c & 0xFFFFFFu;
                if ((c >> 24) != 1u || first >= count || slots[first] != kRefitRoot) return fail(RACC_HIP_ERR_INVALID, "world_refit: the top-level leaves do not name every instance once");
                slots[first] = d * 2u + side;
            }
        }
    }
    if (reached != capacity) return fail(RACC_HIP_ERR_INVALID, "world_refit: the top-level records are not a tree");
    for (uint32_t s : slots) if (s == kRefitRoot) return fail(RACC_HIP_ERR_INVALID, "world_refit: the top-level leaves do not name every instance once");
    HIP_TRY(hipMemcpy(r->slots, slots.data(), size_t(count) * 4, hipMemcpyHostToDevice), "hipMemcpy(world refit slots)");
    HIP_TRY(hipMemcpy(r->parentSlot, parentSlot.data(), size_t(capacity) * 4, hipMemcpyHostToDevice), "hipMemcpy(world refit parents)");
    HIP_TRY(hipMemcpy(r->rayPad, &rayPad, 4, hipMemcpyHostToDevice), "hipMemcpy(world refit pad)");
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_refit: out of host memory");
}

void worldRefitFree(WorldRefit* r) {
    if (r->stream) { hipStreamSynchronize(r->stream); hipStreamDestroy(r->stream); }
    if (r->slots) hipFree(r->slots);
    if (r->parentSlot) hipFree(r->parentSlot);
    if (r->state) hipFree(r->state);
    if (r->rayPad) hipFree(r->rayPad);
    if (r->transforms) hipFree(r->transforms);
    worldRebuildFree(r);
    delete r;
}

}  // namespace

extern "C" int racc_host_world_instances_(const char* who, const float* transforms12, const float* root_boxes6, uint32_t count,
                                          float* inv12_out, float* world_boxes6_out, float* ray_pad_out);      // world_build.cpp

extern "C" {

int racc_hip_world_refit_create(racc_hip_ctx* ctx, racc_hip_world* w, WorldRefit** out) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_create: ctx is NULL");
    if (!out) return fail(RACC_HIP_ERR_INVALID, "world_refit_create: out is NULL");
    *out = nullptr;
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_refit_create: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_create: the world belongs to another context");
    if (w->refit) return fail(RACC_HIP_ERR_INVALID, "world_refit_create: the world already has a refit handle (at most one per world)");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    const uint32_t count = w->count, capacity = count > 1u ? count - 1u : 1u;
    std::vector<uint32_t> dev(size_t(capacity) * 16);
    HIP_TRY(hipMemcpy(dev.data(), w->topNodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(top-level nodes)");
    WorldRefit* r = new (std::nothrow) WorldRefit();
    if (!r) return fail(RACC_HIP_ERR_NOMEM, "out of host memory");
    r->world = w;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->slots), size_t(count) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->parentSlot), size_t(capacity) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->state), worldRefitStateBytes(capacity));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rayPad), 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { worldRefitFree(r); return fail(RACC_HIP_ERR_DEVICE, "world_refit_create", e); }
    w->refit = r;
    if (int rc = worldRefitRebuild(w, dev.data(), w->rayPad)) { w->refit = nullptr; worldRefitFree(r); return rc; }
    w->rayPadDev = r->rayPad;      // from here on the world kernels read the pad from the word
    *out = r;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_refit_create: out of host memory");
}

int racc_hip_world_refit_destroy(racc_hip_ctx* ctx, WorldRefit* r) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_destroy: ctx is NULL");
    if (!r) return RACC_HIP_OK;
    hipSetDevice(ctx->device);
    racc_hip_world* w = r->world;
    hipDeviceSynchronize();      // no refit and no world launch is alive while the pad moves back into the world
    float pad = w->rayPad;
    if (hipMemcpy(&pad, r->rayPad, 4, hipMemcpyDeviceToHost) == hipSuccess) w->rayPad = pad;
    worldRebuildLeave(r);
    w->rayPadDev = nullptr;
    w->refit = nullptr;
    worldRefitFree(r);
    return RACC_HIP_OK;
}

int racc_hip_world_refit_device(racc_hip_ctx* ctx, WorldRefit* r, const void* d_transforms12, uint32_t count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_device: ctx is NULL");
    if (!r || !d_transforms12) return fail(RACC_HIP_ERR_INVALID, "world_refit_device: refit/d_transforms12 is NULL");
    if (r->world->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_device: the world belongs to another context");
    if (count != r->world->count) return fail(RACC_HIP_ERR_INVALID, "world_refit_device: count differs from the world's instance count");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return worldRefitLaunch(r, static_cast<const float*>(d_transforms12), static_cast<hipStream_t>(stream));
}

int racc_hip_world_refit(racc_hip_ctx* ctx, WorldRefit* r, const float* transforms12, uint32_t count) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit: ctx is NULL");
    if (!r || !transforms12) return fail(RACC_HIP_ERR_INVALID, "world_refit: refit/transforms is NULL");
    racc_hip_world* w = r->world;
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit: the world belongs to another context");
    if (count != w->count) return fail(RACC_HIP_ERR_INVALID, "world_refit: count differs from the world's instance count");
    if (int rc = racc_hip_synchronize(ctx)) return rc;      // no kernel reads the top level or a root box while they change
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    // validated with the host rule before anything changes: a refused transform leaves the world as it was
    std::vector<float> rootBoxes, inv(size_t(count) * 12), boxes(size_t(count) * 6);
    if (int rc = worldRootBoxes(w, rootBoxes)) return rc;
    float pad = 0.0f;
    if (int rc = racc_host_world_instances_("racc_hip_world_refit", transforms12, rootBoxes.data(), count, inv.data(), boxes.data(), &pad)) return rc;
    if (!r->transforms) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->transforms), size_t(count) * 48), "hipMalloc(world refit transforms)");
    HIP_TRY(hipMemcpyAsync(r->transforms, transforms12, size_t(count) * 48, hipMemcpyHostToDevice, r->stream), "hipMemcpyAsync(world refit transforms)");
    if (int rc = worldRefitLaunch(r, r->transforms, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream), "hipStreamSynchronize(world refit)");
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_refit: out of host memory");
}

int racc_hip_world_refit_check(racc_hip_ctx* ctx, WorldRefit* r, uint32_t* disabled_instances) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_refit_check: ctx is NULL");
    if (!r || !disabled_instances) return fail(RACC_HIP_ERR_INVALID, "world_refit_check: refit/disabled_instances is NULL");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(disabled_instances, r->state + 1, 4, hipMemcpyDeviceToHost), "hipMemcpy(disabled instances)");
    return RACC_HIP_OK;
}

int racc_hip_world_download(racc_hip_ctx* ctx, const racc_hip_world* w, float* inv12_out, void* nodes64_out, uint32_t node_capacity,
                            uint32_t* order_out, float* ray_pad_out) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "world_download: ctx is NULL");
    if (!w) return fail(RACC_HIP_ERR_INVALID, "world_download: world is NULL");
    if (w->ctx != ctx) return fail(RACC_HIP_ERR_INVALID, "world_download: the world belongs to another context");
    const uint32_t count = w->count, nodeCount = w->info.node_count;
    if (nodes64_out && node_capacity < nodeCount) return fail(RACC_HIP_ERR_INVALID, "world_download: node_capacity is below the world's node_count");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    if (inv12_out) HIP_TRY(hipMemcpy(inv12_out, w->inv, size_t(count) * 48, hipMemcpyDeviceToHost), "hipMemcpy(inverse transforms)");
    if (order_out) HIP_TRY(hipMemcpy(order_out, w->order, size_t(count) * 4, hipMemcpyDeviceToHost), "hipMemcpy(instance order)");
    if (ray_pad_out) {
        *ray_pad_out = w->rayPad;
        if (w->rayPadDev) HIP_TRY(hipMemcpy(ray_pad_out, w->rayPadDev, 4, hipMemcpyDeviceToHost), "hipMemcpy(ray pad)");
    }
    if (nodes64_out) {
        std::vector<uint32_t> dev(size_t(nodeCount) * 16);
        HIP_TRY(hipMemcpy(dev.data(), w->topNodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(top-level nodes)");
        for (uint32_t n = 0; n < nodeCount; ++n) {      // device record -> blob node (worldCommit's conversion, backwards), same numbering
            const uint32_t* d = &dev[size_t(n) * 16];
            uint32_t b[16];
            b[0] = 0u; b[1] = 0u; b[2] = d[0]; b[3] = d[1];      // kind and parent: the device does not hold them
            for (int side = 0; side < 2; ++side)
                for (int k = 0; k < 3; ++k) { b[4 + side * 6 + k] = d[4 + side * 6 + 2 * k]; b[4 + side * 6 + 3 + k] = d[4 + side * 6 + 2 * k + 1]; }
            std::memcpy(static_cast<char*>(nodes64_out) + size_t(n) * 64, b, 64);
        }
    }
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "world_download: out of host memory");
}

}  // extern "C"
