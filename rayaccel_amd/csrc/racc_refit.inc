// racc_refit.inc — refit of a device-resident scene to moved vertices: refitPairsKernel, refitBoxesKernel and the C-ABI entries around
// them (racc_hip_refit_*, racc_hip_scene_refit*).  Textually included by racc_hip_unit.hip BEHIND racc_hip.hip and
// racc_scene_registry.inc, so it sees the context, the scene's device pointers and kept topology and fail() / HIP_TRY, and changes none of
// them.  The reference has no such operation (its scenes are frozen at createScene); Embree's rtcCommitScene on a deformable scene is the
// usual counterpart.
//
// The rule is racc_host_blobs_refit's (scene_refit.cpp), reproduced bit for bit: topology unchanged, pair records re-packed from the
// pair's four vertices, a leaf's box folded with `b < acc ? b : acc` / `b > acc ? b : acc` over its pairs' vertices in order, an inner
// box the union of the first child's box (accumulator) with the last child's.
//
// All refit state lives in the racc_hip_refit handle.  What a handle needs and the device does not hold is the blob's topology words,
// which the scene registry keeps from the upload (racc_scene_registry.inc: sceneTopology; a scene without them is refused).  The handle
// shares them, so they outlive the scene's free.
//
// Box step: one thread per leaf reference.  It folds its leaf's box from the vertices, writes the six planes of its side into the
// parent's device record and climbs: an agent-scope acq_rel fetch_add on the parent's arrival counter; the first arriver retires, the
// second one — its acquire pairs with the first one's release, which is the only thing that makes the sibling's planes visible across
// CUs and XCDs — reads BOTH child boxes from the record, unions them first-child-first, writes the result into the grandparent's record
// and repeats until the root.  Nobody spins or waits: the kernel terminates whatever the schedule.  Counters are zeroed in stream order
// before the kernel.  Padding device records are never touched (no reference points at them): they stay all-zero.

namespace {

constexpr int kRefitBlock = 256;
constexpr uint32_t kRefitRoot = 0xFFFFFFFFu;      // parent slot of the root record

__device__ __forceinline__ float refitMin(float acc, float b) { return b < acc ? b : acc; }
__device__ __forceinline__ float refitMax(float acc, float b) { return b > acc ? b : acc; }

// One thread per pair record (padding included: those are rewritten from pair 0's vertices, Scene.cpp:334-338).
__global__ void __launch_bounds__(kRefitBlock) refitPairsKernel(const float4* __restrict__ vertices, const uint4* __restrict__ quads,
                                                                float4* __restrict__ pairs, uint32_t pairCount, uint32_t pairCountPadded) {
    const uint32_t p = blockIdx.x * uint32_t(kRefitBlock) + threadIdx.x;
    if (p >= pairCountPadded) return;
    const uint4 q = quads[p < pairCount ? p : 0u];
    const float4 p0 = vertices[q.x], p1 = vertices[q.y], p2 = vertices[q.z], p3 = vertices[q.w];
    float4* out = pairs + size_t(p) * 3;      // {e1.xyz, e3.x} {e2.xyz, e3.y} {p0.xyz, e3.z}: packPair (scene_build.cpp)
    out[0] = make_float4(p0.x - p1.x, p0.y - p1.y, p0.z - p1.z, p3.x - p0.x);
    out[1] = make_float4(p2.x - p0.x, p2.y - p0.y, p2.z - p0.z, p3.y - p0.y);
    out[2] = make_float4(p0.x, p0.y, p0.z, p3.z - p0.z);
}

// One thread per leaf reference.  leaves[i] = {leaf reference (first | cnt << 24), slot}; slot = 2 * device record + side (0 = first
// child) names where a box goes; parentSlot[record] = the slot of that record's own box in ITS parent, kRefitRoot for the root.
// A device record: words 0-1 child references, 2-3 unused, 4-15 the planes Lx Ly Lz Rx Ry Rz as (min, max) pairs (racc_device.inc).
__global__ void __launch_bounds__(kRefitBlock) refitBoxesKernel(const float4* __restrict__ vertices, const uint4* __restrict__ quads,
                                                                const uint2* __restrict__ leaves, uint32_t leafCount,
                                                                const uint32_t* __restrict__ parentSlot, uint32_t* counters, float* nodes) {
    const uint32_t i = blockIdx.x * uint32_t(kRefitBlock) + threadIdx.x;
    if (i >= leafCount) return;
    const uint2 leaf = leaves[i];
    const uint32_t first = leaf.x & 0xFFFFFFu, cnt = leaf.x >> 24;
    float mnx, mny, mnz, mxx, mxy, mxz;
    {
        const float4 s = vertices[quads[first].x];
        mnx = mxx = s.x; mny = mxy = s.y; mnz = mxz = s.z;
    }
    for (uint32_t p = first; p < first + cnt; ++p) {
        const uint4 q = quads[p];
        const uint32_t vi[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = vertices[vi[k]];
            mnx = refitMin(mnx, v.x); mny = refitMin(mny, v.y); mnz = refitMin(mnz, v.z);
            mxx = refitMax(mxx, v.x); mxy = refitMax(mxy, v.y); mxz = refitMax(mxz, v.z);
        }
    }
    uint32_t slot = leaf.y;
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

}  // namespace

struct racc_hip_refit {
    racc_hip_scene* scene = nullptr;
    std::shared_ptr<const RefitTopology> topology;
    std::vector<uint32_t> blobToDevice;       // device record of every blob node (racc_hip_refit_download)
    uint32_t vertexCount = 0, pairCount = 0, leafCount = 0;
    uint4* quads = nullptr;                   // [pairCount] the four vertex indices of every pair
    uint2* leaves = nullptr;                  // [leafCount]
    uint32_t* parentSlot = nullptr;           // [deviceNodes]
    uint32_t* counters = nullptr;             // [deviceNodes] arrival counters
    float4* vertices = nullptr;               // staging of the blocking entry, allocated at its first call
    hipStream_t stream = nullptr;             // ... and its stream
    // a handle of racc_hip_refit_create_wide (racc_refit_wide.inc): every refit also rewrites the scene's 4-wide / compressed records
    bool wideClaimed = false;                 // this handle is the scene's one wide handle (racc_scene_registry.inc)
    uint32_t wideCount = 0;                   // 0: a plain handle
    uint4* wideSources = nullptr;             // [wideCount] per slot 2 * device record + side of the binary child box it copies, kWideNone in an unused slot
    uint32_t* wideDisabled = nullptr;         // [1] compressed frames the last refit disabled (racc_hip_refit_check)
    // a handle of racc_hip_scene_rebuild_create (racc_scene_rebuild.inc): no topology words, device record = node index, the tables above
    // are written by the rebuild's kernels; parentSlot and counters hold max(deviceNodes, triangles) entries
    uint32_t* rebuildWords = nullptr;         // [8] centre bounds lo[3], hi[3] as ordered integers, height, unused; null: not a rebuild handle
    uint32_t triCount = 0;
    uint32_t* rebuildIndices = nullptr;       // [3 * triCount] the mesh's index triples
    unsigned long long* rebuildKeys = nullptr;      // [2 * triCount] Morton fields: as formed, sorted
    uint32_t* rebuildValues = nullptr;        // [2 * triCount] triangle indices: as formed, sorted
    void* sortTemp = nullptr;                 // rocPRIM's temporary storage, sized at creation
    size_t sortTempBytes = 0;
};

namespace {

int refitWideLaunch(racc_hip_refit* r, hipStream_t st);      // racc_refit_wide.inc
int refitWideAttach(racc_hip_refit* r);
void refitWideDetach(racc_hip_refit* r);
void sceneRebuildDetach(racc_hip_refit* r);      // racc_scene_rebuild.inc
int sceneRebuildDownload(racc_hip_refit* r, void* nodes64_out, uint32_t node_capacity, void* pairs48_out, uint32_t pair_capacity);

int refitLaunch(racc_hip_refit* r, const float4* dVertices, hipStream_t st) {
    const racc_hip_scene* s = r->scene;
    HIP_TRY(hipMemsetAsync(r->counters, 0, size_t(s->deviceNodes) * sizeof(uint32_t), st), "hipMemsetAsync(refit counters)");
    const uint32_t padded = s->info.pair_count;
    hipLaunchKernelGGL(refitPairsKernel, dim3((padded + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, dVertices, r->quads, s->pairs, r->pairCount, padded);
    HIP_TRY(hipGetLastError(), "launch refitPairsKernel");
    hipLaunchKernelGGL(refitBoxesKernel, dim3((r->leafCount + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, dVertices, r->quads, r->leaves, r->leafCount,
                       r->parentSlot, r->counters, reinterpret_cast<float*>(s->nodes));
    HIP_TRY(hipGetLastError(), "launch refitBoxesKernel");
    if (r->wideCount) return refitWideLaunch(r, st);      // behind the box kernel on the same stream: the kernel boundary publishes the binary boxes
    return RACC_HIP_OK;
}

}  // namespace

extern "C" {

int racc_hip_refit_destroy(racc_hip_ctx* ctx, racc_hip_refit* r) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_destroy: ctx is NULL");
    if (!r) return RACC_HIP_OK;
    hipSetDevice(ctx->device);
    if (r->stream) { hipStreamSynchronize(r->stream); hipStreamDestroy(r->stream); }
    if (r->quads) hipFree(r->quads);
    if (r->leaves) hipFree(r->leaves);
    if (r->parentSlot) hipFree(r->parentSlot);
    if (r->counters) hipFree(r->counters);
    if (r->vertices) hipFree(r->vertices);
    refitWideDetach(r);
    sceneRebuildDetach(r);
    delete r;
    return RACC_HIP_OK;
}

}  // extern "C"

namespace {

// racc_hip_refit_create and racc_hip_refit_create_wide (racc_refit_wide.inc): the latter also attaches the wide state (refitWideAttach)
int refitCreate(racc_hip_ctx* ctx, racc_hip_scene* scene, const uint32_t* indices, uint32_t index_count, uint32_t vertex_count, bool wide,
                racc_hip_refit** out) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_create: ctx is NULL");
    if (!out) return fail(RACC_HIP_ERR_INVALID, "refit_create: out is NULL");
    *out = nullptr;
    if (!scene || !indices) return fail(RACC_HIP_ERR_INVALID, "refit_create: scene/indices is NULL");
    if (sceneIsRebuilt(scene))
        return fail(RACC_HIP_ERR_INVALID, "refit_create: the scene was made by racc_hip_scene_rebuild_create, whose handle is its only handle: a device rebuild changes the "
                                          "topology, the words a plain handle keeps would go stale and it would write wrong boxes");
    if (!wide && (scene->nodesWide || scene->nodesWideQ || scene->nodesSoa))
        return fail(RACC_HIP_ERR_INVALID, "refit_create: the scene carries a 4-wide, compressed or SoA copy of the tree (kernel_variant 45 / 50, wide_below, the SoA variant); "
                                          "racc_hip_refit_create_wide refits the 4-wide and compressed copies, a stale copy would give wrong hits");
    if (wide && scene->nodesSoa) return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: the scene carries an SoA copy of the tree (the SoA variant), which is not refitted");
    if (wide && !scene->nodesWide && !scene->nodesWideQ)
        return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: the scene carries neither a 4-wide nor a compressed copy of the tree (racc_hip_refit_create is the entry for it)");
    std::shared_ptr<const RefitTopology> topo = sceneTopology(scene);
    if (!topo) return fail(RACC_HIP_ERR_INVALID, "refit_create: the blob's topology words were not kept for this scene (a device group's replica, RACC_REFIT_TOPOLOGY=0, or no host memory at upload)");
    if (index_count % 3 != 0) return fail(RACC_HIP_ERR_INVALID, "refit_create: index_count is not a multiple of 3");
    const uint32_t triCount = index_count / 3, nodeCount = topo->nodeCount, deviceNodes = scene->deviceNodes;
    const uint32_t remapCount = scene->info.remap_count;
    // The device does not hold the unpadded pair count: it is where the last leaf ends (the builder's leaves cover [0, pair_count) without gaps).
    // Records behind that are padding — copies of pair 0 — whatever remap holds for them.  validateScene (upload) guarantees remap covers every leaf.
    uint32_t pairCount = 0;
    for (uint32_t b = 0; b < nodeCount; ++b)
        for (uint32_t side = 0; side < 2; ++side) {
            const uint32_t c = topo->words[size_t(b) * 4 + 2 + side];
            if (!(c & 0x80000000u) && (c & 0xFFFFFFu) + (c >> 24) > pairCount) pairCount = (c & 0xFFFFFFu) + (c >> 24);
        }
    if (!pairCount || pairCount > scene->info.pair_count || uint64_t(pairCount) * 2 > remapCount) return fail(RACC_HIP_ERR_INVALID, "refit_create: the leaves' pair ranges do not fit the scene's pairs and remap");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");

    // what the device holds: the records (words 0-1 = the child references in device numbering) and remap
    std::vector<uint32_t> dev(size_t(deviceNodes) * 16), remap(remapCount);
    HIP_TRY(hipMemcpy(dev.data(), scene->nodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(device nodes)");
    HIP_TRY(hipMemcpy(remap.data(), scene->remap, size_t(remapCount) * 4, hipMemcpyDeviceToHost), "hipMemcpy(remap)");

    // both trees walked together from their roots: blob node <-> device record.  The blob passed validateScene at upload (every child
    // index and pair range in bounds, every inner node reached once); the device words are checked against it as they are met.
    const uint32_t* words = topo->words.data();
    std::vector<uint32_t> blobToDevice(nodeCount, kRefitRoot), parentSlot(deviceNodes, kRefitRoot);
    std::vector<uint2> leaves;
    leaves.reserve(size_t(nodeCount) + 1);
    std::vector<std::pair<uint32_t, uint32_t>> work;      // (blob node, device record)
    work.emplace_back(0u, 0u);
    blobToDevice[0] = 0u;
    while (!work.empty()) {
        const auto [b, d] = work.back();
        work.pop_back();
        for (uint32_t side = 0; side < 2; ++side) {
            const uint32_t bc = words[size_t(b) * 4 + 2 + side], dc = dev[size_t(d) * 16 + side];
            if ((bc ^ dc) & 0x80000000u) return fail(RACC_HIP_ERR_INVALID, "refit_create: the device records do not match the uploaded tree");
            if (bc & 0x80000000u) {
                const uint32_t bi = bc & 0x7FFFFFFFu, di = dc & 0x7FFFFFFFu;
                if (bi >= nodeCount || di >= deviceNodes || di == 0u || parentSlot[di] != kRefitRoot) return fail(RACC_HIP_ERR_INVALID, "refit_create: the device records do not match the uploaded tree");
                blobToDevice[bi] = di;
                parentSlot[di] = d * 2u + side;
                work.emplace_back(bi, di);
            } else {
                const uint32_t first = bc & 0xFFFFFFu, cnt = bc >> 24;
                if (bc != dc || cnt == 0u) return fail(RACC_HIP_ERR_INVALID, "refit_create: the device records do not match the uploaded tree");
                if (first + cnt > pairCount) return fail(RACC_HIP_ERR_INVALID, "refit_create: a leaf reaches into pairs that remap does not cover");
                leaves.push_back(make_uint2(bc, d * 2u + side));
            }
        }
    }
    // the four vertex indices of every pair (scene_refit.cpp), validated like racc_host_blobs_refit validates them
    std::vector<uint4> quads(pairCount);
    for (uint32_t p = 0; p < pairCount; ++p) {
        const uint32_t r0 = remap[2 * size_t(p)], r1 = remap[2 * size_t(p) + 1];
        const uint32_t t0 = r0 & 0x3FFFFFFFu, ea = r0 >> 30;
        if (t0 >= triCount || ea > 2u) return fail(RACC_HIP_ERR_INVALID, "refit_create: remap names a triangle beyond index_count / 3 (or an edge code beyond 2)");
        const uint32_t* a = indices + size_t(t0) * 3;
        uint4 q = make_uint4(a[ea], a[(ea + 1) % 3], a[(ea + 2) % 3], 0u);
        if (r1 == 0u) q.w = q.y;
        else {
            const uint32_t t1 = r1 & 0x3FFFFFFFu, eb = (r1 >> 30) - 1u;
            if (t1 >= triCount || (r1 >> 30) == 0u) return fail(RACC_HIP_ERR_INVALID, "refit_create: remap names a triangle beyond index_count / 3 (or a second triangle without its edge code)");
            q.w = indices[size_t(t1) * 3 + (eb + 2) % 3];
        }
        quads[p] = q;
    }
    for (uint32_t i = 0; i < index_count; ++i)
        if (indices[i] >= vertex_count) return fail(RACC_HIP_ERR_INVALID, "refit_create: an index is not below vertex_count");

    racc_hip_refit* r = new (std::nothrow) racc_hip_refit();
    if (!r) return fail(RACC_HIP_ERR_NOMEM, "out of host memory");
    r->scene = scene; r->topology = topo; r->blobToDevice.swap(blobToDevice);
    r->vertexCount = vertex_count; r->pairCount = pairCount; r->leafCount = uint32_t(leaves.size());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->quads), quads.size() * sizeof(uint4));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->leaves), leaves.size() * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->parentSlot), size_t(deviceNodes) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->counters), size_t(deviceNodes) * 4);
    if (e == hipSuccess) e = hipMemcpy(r->quads, quads.data(), quads.size() * sizeof(uint4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->leaves, leaves.data(), leaves.size() * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->parentSlot, parentSlot.data(), size_t(deviceNodes) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { racc_hip_refit_destroy(ctx, r); return fail(RACC_HIP_ERR_DEVICE, "refit_create", e); }
    if (wide) if (int rc = refitWideAttach(r)) { racc_hip_refit_destroy(ctx, r); return rc; }
    *out = r;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {      // (the host-side tables; the handle itself is allocated after them)
    return fail(RACC_HIP_ERR_NOMEM, "refit_create: out of host memory");
}

}  // namespace

extern "C" {

int racc_hip_refit_create(racc_hip_ctx* ctx, racc_hip_scene* scene, const uint32_t* indices, uint32_t index_count, uint32_t vertex_count,
                          racc_hip_refit** out) {
    return refitCreate(ctx, scene, indices, index_count, vertex_count, false, out);
}

int racc_hip_scene_refit_device(racc_hip_ctx* ctx, racc_hip_refit* r, const void* d_vertices, uint32_t vertex_count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_refit_device: ctx is NULL");
    if (!r || !d_vertices) return fail(RACC_HIP_ERR_INVALID, "scene_refit_device: refit/d_vertices is NULL");
    if (vertex_count != r->vertexCount) return fail(RACC_HIP_ERR_INVALID, "scene_refit_device: vertex_count differs from the one the refit handle was created with");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return refitLaunch(r, static_cast<const float4*>(d_vertices), static_cast<hipStream_t>(stream));
}

int racc_hip_scene_refit(racc_hip_ctx* ctx, racc_hip_refit* r, const float* vertices, uint32_t vertex_count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_refit: ctx is NULL");
    if (!r || !vertices) return fail(RACC_HIP_ERR_INVALID, "scene_refit: refit/vertices is NULL");
    if (vertex_count != r->vertexCount) return fail(RACC_HIP_ERR_INVALID, "scene_refit: vertex_count differs from the one the refit handle was created with");
    for (size_t i = 0; i < size_t(vertex_count); ++i)
        if (!std::isfinite(vertices[i * 4]) || !std::isfinite(vertices[i * 4 + 1]) || !std::isfinite(vertices[i * 4 + 2])) return fail(RACC_HIP_ERR_INVALID, "scene_refit: a vertex coordinate is not finite");
    if (r->wideCount && r->scene->nodesWideQ && vertex_count) {      // no frame of the compressed copy is wider than the mesh: nothing is disabled below
        for (int ax = 0; ax < 3; ++ax) {
            float mn = vertices[ax], mx = mn;
            for (size_t i = 1; i < size_t(vertex_count); ++i) { const float v = vertices[i * 4 + ax]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
            if (!std::isfinite(mx - mn)) return fail(RACC_HIP_ERR_LIMIT, "scene_refit: the vertices' extent on an axis overflows binary32 (the compressed 4-wide format cannot hold such a frame)");
        }
    }
    if (int rc = racc_hip_synchronize(ctx)) return rc;      // no traversal kernel (a chain's included) is alive while the records change
    const size_t bytes = size_t(vertex_count ? vertex_count : 1u) * 16;
    if (!r->vertices) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->vertices), bytes), "hipMalloc(refit vertices)");
    HIP_TRY(hipMemcpyAsync(r->vertices, vertices, size_t(vertex_count) * 16, hipMemcpyHostToDevice, r->stream), "hipMemcpyAsync(refit vertices)");
    if (int rc = refitLaunch(r, r->vertices, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream), "hipStreamSynchronize(refit)");
    return RACC_HIP_OK;
}

int racc_hip_refit_download(racc_hip_ctx* ctx, racc_hip_refit* r, void* nodes64_out, uint32_t node_capacity, void* pairs48_out, uint32_t pair_capacity) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_download: ctx is NULL");
    if (!r) return fail(RACC_HIP_ERR_INVALID, "refit_download: refit is NULL");
    if (r->rebuildWords) { HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice"); return sceneRebuildDownload(r, nodes64_out, node_capacity, pairs48_out, pair_capacity); }
    const racc_hip_scene* s = r->scene;
    const uint32_t nodeCount = r->topology->nodeCount;
    if ((nodes64_out && node_capacity < nodeCount) || (pairs48_out && pair_capacity < s->info.pair_count)) return fail(RACC_HIP_ERR_INVALID, "refit_download: capacity too small");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    if (pairs48_out) HIP_TRY(hipMemcpy(pairs48_out, s->pairs, size_t(s->info.pair_count) * 48, hipMemcpyDeviceToHost), "hipMemcpy(pairs)");
    if (nodes64_out) {
        std::vector<float> dev(size_t(s->deviceNodes) * 16);
        HIP_TRY(hipMemcpy(dev.data(), s->nodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(device nodes)");
        for (uint32_t b = 0; b < nodeCount; ++b) {
            char* rec = static_cast<char*>(nodes64_out) + size_t(b) * 64;
            std::memcpy(rec, &r->topology->words[size_t(b) * 4], 16);
            const uint32_t d = r->blobToDevice[b];
            float box[12] = {};      // (a node the root does not reach has no device record: zeros)
            if (d != kRefitRoot) {
                const float* p = &dev[size_t(d) * 16 + 4];      // Lx Ly Lz Rx Ry Rz as (min, max) -> leftMin[3], leftMax[3], rightMin[3], rightMax[3]
                for (int side = 0; side < 2; ++side)
                    for (int k = 0; k < 3; ++k) { box[side * 6 + k] = p[side * 6 + 2 * k]; box[side * 6 + 3 + k] = p[side * 6 + 2 * k + 1]; }
            }
            std::memcpy(rec + 16, box, 48);
        }
    }
    return RACC_HIP_OK;
}

}  // extern "C"
