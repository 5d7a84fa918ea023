// racc_scene_rebuild.inc — build and rebuild of a scene's tree (the bottom level) on the device, in stream order: an LBVH over the
// triangles of a mesh (Morton codes of the triangle box centres, a radix sort, Karras's 2012 hierarchy) written into a scene's existing
// allocations in the formats every kernel reads, and the C-ABI entries around it (racc_hip_scene_rebuild*).  Textually included by
// racc_hip_unit.hip BEHIND racc_refit.inc and racc_world_rebuild.inc: it sees the scene, the refit handle, refitLaunch and kRefitRoot, and
// the world rebuild's ordered floats, wave reductions and rocPRIM include.  Every GPU API's bottom-level build is the usual counterpart.
//
// The rule is racc_scene_rebuild_rule.h's, which racc_host_scene_rebuild (scene_rebuild.cpp) states top-down; this file reproduces that
// function's nodes, pairs and remap byte for byte.  Four kernels and one sort of its own, nothing waits on anything except through stream
// order, nobody spins:
//   sceneRebuildBoundsKernel   one thread per TRIANGLE: its box and centre, the centre bounds reduced in the wave and folded into six words
//                              by one atomic min / max per wave and axis — floats as ordered integers (worldRebuildCentresKernel's way).
//   sceneRebuildFieldsKernel   one thread per triangle: its centre again (three gathers the L2 still holds, instead of 12 B of scratch per
//                              triangle written and read), its Morton field against the finished bounds, value = its index.
//   rocprim::radix_sort_pairs  over the 63 bits of the field, the triangle index as value.  The input is in index order and the sort is
//                              stable (rocPRIM documents it), so equal fields stay in index order: the order of the 95-bit keys.
//   sceneRebuildTreeKernel     one thread per position p: remap[2p], remap[2p + 1], the pair's four vertex indices (quads[p]); for
//                              p < T - 1 node p by racc_scene_rebuild_rule::hierarchyStep: words 0-1 of device record p, parentSlot of
//                              its inner children, the leaf table entries of its leaf children.
//   sceneRebuildHeightKernel   one thread per position: the records on its path to the root, counted along parentSlot; the maximum into
//                              the height word (wave-reduced, one atomic max per wave).
//   refitLaunch                unchanged, behind them: the pair records, the boxes up the new tree at the acq_rel counters.
// The sort always delivers sorted unique keys whatever the vertices hold (the field is in [0, 2^63) for any bits), and hierarchyStep
// names only positions in [0, T) and nodes in [0, T - 1] even for garbage: no access of the rebuild leaves its arrays.
//
// Layout.  racc_hip_scene_upload (which does all allocation) leaves the records in its line-paired order; the first device rebuild — part
// of racc_hip_scene_rebuild_create — rewrites them as device record = node index, and they stay that way: the upload's padding records lie
// unreferenced behind the T - 1 nodes.  The line-paired order is out of scope (include/racc_hip.h).
//
// Stack room.  The host cannot know a device-built tree's height without leaving the stream, so racc_hip_scene_rebuild_device raises the
// scene's info.inner_height to racc_scene_rebuild_rule::heightBound before it enqueues anything (the launch paths size the spill from it at
// every launch); the blocking rebuild and racc_hip_scene_rebuild_check set it to the real height, which the height kernel leaves in the
// handle's height word.

namespace {

namespace scene_rule = racc_scene_rebuild_rule;
constexpr int kSceneRebuildBlock = 256;
constexpr uint32_t kSceneRebuildWords = 8;      // lo[3], hi[3], height, unused
constexpr uint32_t kSceneRebuildHeightWord = 6;

__device__ __forceinline__ void sceneRebuildCentre(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices, uint32_t t, float c[3]) {
    const uint32_t* a = indices + size_t(t) * 3;
    const float4 p0 = vertices[a[0]], p1 = vertices[a[1]], p2 = vertices[a[2]];
    const float v0[3] = { p0.x, p0.y, p0.z }, v1[3] = { p1.x, p1.y, p1.z }, v2[3] = { p2.x, p2.y, p2.z };
    scene_rule::triangleCentre(v0, v1, v2, c);
}

__global__ void __launch_bounds__(kSceneRebuildBlock) sceneRebuildBoundsKernel(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices, uint32_t triCount,
                                                                               uint32_t* words) {
    const uint32_t t = blockIdx.x * uint32_t(kSceneRebuildBlock) + threadIdx.x;
    uint32_t lo[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, hi[3] = { 0u, 0u, 0u };      // neutral: an idle lane
    if (t < triCount) {
        float c[3];
        sceneRebuildCentre(vertices, indices, t, c);
        lo[0] = hi[0] = orderedOf(c[0]); lo[1] = hi[1] = orderedOf(c[1]); lo[2] = hi[2] = orderedOf(c[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {      // every lane of the wave is here
        const uint32_t mn = waveMin(lo[k]), mx = waveMax(hi[k]);
        if ((threadIdx.x & 63u) == 0u && mn <= mx) {
            __hip_atomic_fetch_min(words + k, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(words + 3 + k, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void __launch_bounds__(kSceneRebuildBlock) sceneRebuildFieldsKernel(const float4* __restrict__ vertices, const uint32_t* __restrict__ indices, uint32_t triCount,
                                                                               const uint32_t* __restrict__ words, unsigned long long* __restrict__ fields,
                                                                               uint32_t* __restrict__ values) {
    const uint32_t t = blockIdx.x * uint32_t(kSceneRebuildBlock) + threadIdx.x;
    if (t >= triCount) return;
    float c[3];
    sceneRebuildCentre(vertices, indices, t, c);
    const float lo[3] = { floatOf(words[0]), floatOf(words[1]), floatOf(words[2]) }, hi[3] = { floatOf(words[3]), floatOf(words[4]), floatOf(words[5]) };
    fields[t] = scene_rule::field(c, lo, hi);
    values[t] = t;
}

// `fields` / `order`: the sorted keys.  Writes only entries [0, T) of remap / 2, quads and leaves, records [0, T - 1) of nodes and entries
// [0, T) of parentSlot (racc_scene_rebuild_rule::hierarchyStep's guarantee; the handle's tables have at least T entries).
__global__ void __launch_bounds__(kSceneRebuildBlock) sceneRebuildTreeKernel(const unsigned long long* __restrict__ fields, const uint32_t* __restrict__ order,
                                                                             const uint32_t* __restrict__ indices, uint32_t triCount, uint32_t indexLimit,
                                                                             float4* __restrict__ nodes, uint32_t* __restrict__ remap, uint4* __restrict__ quads,
                                                                             uint2* __restrict__ leaves, uint32_t* __restrict__ parentSlot) {
    const uint32_t p = blockIdx.x * uint32_t(kSceneRebuildBlock) + threadIdx.x;
    if (p >= triCount) return;
    uint32_t t = order[p];
    t = t < triCount ? t : 0u;      // (the sort's values are a permutation of [0, T): never decides)
    const uint32_t* a = indices + size_t(t) * 3;
    const uint32_t a0 = a[0] < indexLimit ? a[0] : 0u, a1 = a[1] < indexLimit ? a[1] : 0u, a2 = a[2] < indexLimit ? a[2] : 0u;      // (validated at creation: never decides)
    *reinterpret_cast<uint2*>(remap + size_t(p) * 2) = make_uint2(t, 0u);
    quads[p] = make_uint4(a0, a1, a2, a1);
    if (p == 0u) parentSlot[0] = kRefitRoot;
    if (p + 1u >= triCount) return;
    const scene_rule::HierarchyStep s = scene_rule::hierarchyStep(fields, order, int(triCount), int(p));
#pragma unroll
    for (uint32_t side = 0; side < 2u; ++side) {
        if (s.leaf[side]) leaves[s.target[side]] = make_uint2(s.word[side], p * 2u + side);
        else parentSlot[s.target[side]] = p * 2u + side;
    }
    *reinterpret_cast<uint2*>(nodes + size_t(p) * 4) = make_uint2(s.word[0], s.word[1]);
}

// `maxLevels` = the bound of the rule: no path is longer, so the walk ends whatever the tables hold.  `recordLimit` = T - 1.
__global__ void __launch_bounds__(kSceneRebuildBlock) sceneRebuildHeightKernel(const uint2* __restrict__ leaves, const uint32_t* __restrict__ parentSlot, uint32_t triCount,
                                                                               uint32_t recordLimit, uint32_t maxLevels, uint32_t* heightWord) {
    const uint32_t p = blockIdx.x * uint32_t(kSceneRebuildBlock) + threadIdx.x;
    uint32_t levels = 0u;
    if (p < triCount) {
        uint32_t rec = leaves[p].y >> 1;
        levels = 1u;
        while (levels < maxLevels && rec < recordLimit) {
            const uint32_t up = parentSlot[rec];
            if (up == kRefitRoot) break;
            rec = up >> 1;
            ++levels;
        }
    }
    levels = waveMax(levels);
    if ((threadIdx.x & 63u) == 0u && levels) __hip_atomic_fetch_max(heightWord, levels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

hipError_t sceneRebuildSort(racc_hip_refit* r, void* temp, size_t& bytes, hipStream_t st) {
    const uint32_t T = r->triCount;
    return rocprim::radix_sort_pairs(temp, bytes, r->rebuildKeys, r->rebuildKeys + T, r->rebuildValues, r->rebuildValues + T, size_t(T), 0u, scene_rule::kFieldBits, st);
}

// info.inner_height / spill_levels for a tree of `height` levels, as racc_hip_scene_upload fills them
void sceneRebuildSetHeight(racc_hip_ctx* ctx, racc_hip_scene* s, uint32_t height) {
    s->info.inner_height = height;
    const uint32_t lds = uint32_t(pickVariant(ctx, height).stackLevels());
    s->info.spill_levels = height > lds ? height - lds : 0u;
}

int sceneRebuildLaunch(racc_hip_refit* r, const float4* dVertices, hipStream_t st) {
    const racc_hip_scene* s = r->scene;
    const uint32_t T = r->triCount;
    const dim3 grid((T + kSceneRebuildBlock - 1) / kSceneRebuildBlock), block(kSceneRebuildBlock);
    HIP_TRY(hipMemsetAsync(r->rebuildWords, 0xFF, 12, st), "hipMemsetAsync(scene rebuild bounds)");
    HIP_TRY(hipMemsetAsync(r->rebuildWords + 3, 0, (kSceneRebuildWords - 3) * 4, st), "hipMemsetAsync(scene rebuild bounds)");
    hipLaunchKernelGGL(sceneRebuildBoundsKernel, grid, block, 0, st, dVertices, r->rebuildIndices, T, r->rebuildWords);
    HIP_TRY(hipGetLastError(), "launch sceneRebuildBoundsKernel");
    hipLaunchKernelGGL(sceneRebuildFieldsKernel, grid, block, 0, st, dVertices, r->rebuildIndices, T, r->rebuildWords, r->rebuildKeys, r->rebuildValues);
    HIP_TRY(hipGetLastError(), "launch sceneRebuildFieldsKernel");
    size_t bytes = r->sortTempBytes;
    HIP_TRY(sceneRebuildSort(r, r->sortTemp, bytes, st), "radix_sort_pairs(scene rebuild)");
    hipLaunchKernelGGL(sceneRebuildTreeKernel, grid, block, 0, st, r->rebuildKeys + T, r->rebuildValues + T, r->rebuildIndices, T, r->vertexCount, s->nodes, s->remap, r->quads,
                       r->leaves, r->parentSlot);
    HIP_TRY(hipGetLastError(), "launch sceneRebuildTreeKernel");
    hipLaunchKernelGGL(sceneRebuildHeightKernel, grid, block, 0, st, r->leaves, r->parentSlot, T, T - 1u, scene_rule::heightBound(T), r->rebuildWords + kSceneRebuildHeightWord);
    HIP_TRY(hipGetLastError(), "launch sceneRebuildHeightKernel");
    return refitLaunch(r, dVertices, st);
}

// the caller has synchronised: the height word of the tree the scene holds now, into info
int sceneRebuildReadHeight(racc_hip_ctx* ctx, racc_hip_refit* r, uint32_t* height) {
    uint32_t h = 0;
    HIP_TRY(hipMemcpy(&h, r->rebuildWords + kSceneRebuildHeightWord, 4, hipMemcpyDeviceToHost), "hipMemcpy(scene rebuild height)");
    if (!h || h > scene_rule::heightBound(r->triCount)) return fail(RACC_HIP_ERR_DEVICE, "scene_rebuild: the height word is outside the rule's bound (no rebuild has completed on this handle?)");
    sceneRebuildSetHeight(ctx, r->scene, h);
    if (height) *height = h;
    return RACC_HIP_OK;
}

// racc_hip_refit_destroy
void sceneRebuildDetach(racc_hip_refit* r) {
    if (r->rebuildIndices) hipFree(r->rebuildIndices);
    if (r->rebuildKeys) hipFree(r->rebuildKeys);
    if (r->rebuildValues) hipFree(r->rebuildValues);
    if (r->sortTemp) hipFree(r->sortTemp);
    if (r->rebuildWords) { hipFree(r->rebuildWords); sceneReleaseRebuild(r->scene); }
}

// racc_hip_refit_download on a rebuild handle: device record = node index, so the blob is the records themselves — first / last are words
// 0-1, parent comes from parentSlot, kind is 1.
int sceneRebuildDownload(racc_hip_refit* r, void* nodes64_out, uint32_t node_capacity, void* pairs48_out, uint32_t pair_capacity) try {
    const racc_hip_scene* s = r->scene;
    const uint32_t nodeCount = r->triCount - 1u;
    if ((nodes64_out && node_capacity < nodeCount) || (pairs48_out && pair_capacity < s->info.pair_count)) return fail(RACC_HIP_ERR_INVALID, "refit_download: capacity too small");
    if (pairs48_out) HIP_TRY(hipMemcpy(pairs48_out, s->pairs, size_t(s->info.pair_count) * 48, hipMemcpyDeviceToHost), "hipMemcpy(pairs)");
    if (nodes64_out) {
        std::vector<uint32_t> dev(size_t(nodeCount) * 16), parent(nodeCount);
        HIP_TRY(hipMemcpy(dev.data(), s->nodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(device nodes)");
        HIP_TRY(hipMemcpy(parent.data(), r->parentSlot, parent.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(parent slots)");
        for (uint32_t b = 0; b < nodeCount; ++b) {
            const uint32_t* d = &dev[size_t(b) * 16];
            uint32_t rec[16] = { 1u, parent[b] == kRefitRoot ? kRefitRoot : parent[b] >> 1, d[0], d[1] };
            for (int side = 0; side < 2; ++side)      // Lx Ly Lz Rx Ry Rz as (min, max) -> leftMin[3], leftMax[3], rightMin[3], rightMax[3]
                for (int k = 0; k < 3; ++k) { rec[4 + side * 6 + k] = d[4 + side * 6 + 2 * k]; rec[4 + side * 6 + 3 + k] = d[4 + side * 6 + 2 * k + 1]; }
            std::memcpy(static_cast<char*>(nodes64_out) + size_t(b) * 64, rec, 64);
        }
    }
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "refit_download: out of host memory");
}

}  // namespace

extern "C" {

int racc_hip_scene_rebuild_create(racc_hip_ctx* ctx, const float* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                                  racc_hip_scene** scene_out, racc_hip_refit** out) try {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_create: ctx is NULL");
    if (!scene_out || !out) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_create: scene_out/out is NULL");
    *scene_out = nullptr; *out = nullptr;
    if (!vertices || !indices) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_create: vertices/indices is NULL");
    {
        const Variant& own = pickVariant(ctx, 0u);
        if (own.wide || own.cacheNodes > 0 || ctx->opts.wide_below != 0u || ctx->opts.kernel_variant == uint32_t(kSoaVariant))
            return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_create: this context's uploads carry a 4-wide, compressed or SoA copy of the tree or put the top of the tree first "
                                              "(kernel_variant 45-53, wide_below, the SoA variant, 60-63): a device rebuild rewrites the binary records only, the copies and "
                                              "the cached top would go stale");
    }
    // the host function on the given vertices (its refusals, under its name), uploaded through the ordinary entry: all allocation is there
    const uint32_t T = index_count / 3;
    const size_t cap = T < scene_rule::kMaxTriangles ? T : 0u;      // (a count the host function refuses gets no room)
    std::vector<char> nodes((cap ? cap - 1 : 0) * 64 + 64), pairs(size_t(scene_rule::paddedPairs(uint32_t(cap))) * 48);
    std::vector<uint32_t> remap(cap * 2 + 2);
    uint32_t nodeCount = 0, pairCount = 0, remapCount = 0, height = 0;
    if (int rc = racc_host_scene_rebuild(vertices, vertex_count, indices, index_count, nodes.data(), uint32_t(cap ? cap - 1 : 0), &nodeCount, pairs.data(),
                                         scene_rule::paddedPairs(uint32_t(cap)), &pairCount, remap.data(), uint32_t(cap * 2), &remapCount, &height)) return rc;
    racc_hip_scene* scene = nullptr;
    if (int rc = racc_hip_scene_upload(ctx, nodes.data(), nodeCount, pairs.data(), pairCount, remap.data(), remapCount, &scene)) return rc;
    racc_hip_refit* r = new (std::nothrow) racc_hip_refit();
    if (!r) { racc_hip_scene_free(ctx, scene); return fail(RACC_HIP_ERR_NOMEM, "out of host memory"); }
    r->scene = scene; r->vertexCount = vertex_count; r->triCount = T; r->pairCount = T; r->leafCount = T;
    const size_t tables = scene->deviceNodes > T ? scene->deviceNodes : T;      // parentSlot / counters: every index the tree kernel can name, every record refitLaunch zeroes
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->quads), size_t(T) * sizeof(uint4));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->leaves), size_t(T) * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->parentSlot), tables * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->counters), tables * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->vertices), size_t(vertex_count) * 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rebuildIndices), size_t(index_count) * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rebuildKeys), size_t(T) * 2 * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rebuildValues), size_t(T) * 2 * 4);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = sceneRebuildSort(r, nullptr, r->sortTempBytes, r->stream);      // the size query: nothing runs
    if (e == hipSuccess) e = hipMalloc(&r->sortTemp, r->sortTempBytes ? r->sortTempBytes : 4);
    if (e == hipSuccess) e = hipMemcpy(r->rebuildIndices, indices, size_t(index_count) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->vertices, vertices, size_t(vertex_count) * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(r->parentSlot, 0xFF, tables * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->rebuildWords), kSceneRebuildWords * 4);      // last: what makes it a rebuild handle
    if (e == hipSuccess) e = hipMemset(r->rebuildWords, 0, kSceneRebuildWords * 4);
    if (e == hipSuccess) e = hipDeviceSynchronize();      // (hipMemset returns before it has run, and the handle's stream does not wait for the null stream)
    int rc = e == hipSuccess ? RACC_HIP_OK : fail(RACC_HIP_ERR_DEVICE, "scene_rebuild_create", e);
    if (!rc && !sceneClaimRebuild(scene)) rc = fail(RACC_HIP_ERR_NOMEM, "scene_rebuild_create: the scene got no registry record (out of host memory at upload)");
    // one device rebuild: the scene is in the rebuild's own layout from here on
    if (!rc) rc = sceneRebuildLaunch(r, r->vertices, r->stream);
    if (!rc && (e = hipStreamSynchronize(r->stream)) != hipSuccess) rc = fail(RACC_HIP_ERR_DEVICE, "hipStreamSynchronize(scene rebuild)", e);
    uint32_t built = 0;
    if (!rc) rc = sceneRebuildReadHeight(ctx, r, &built);
    if (!rc && built != height) rc = fail(RACC_HIP_ERR_DEVICE, "scene_rebuild_create: the device-built tree's height differs from the host specification's");
    if (rc) { racc_hip_refit_destroy(ctx, r); racc_hip_scene_free(ctx, scene); return rc; }
    scene->info.max_leaf_pairs = 1u;
    *scene_out = scene; *out = r;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "scene_rebuild_create: out of host memory");
}

int racc_hip_scene_rebuild_device(racc_hip_ctx* ctx, racc_hip_refit* r, const void* d_vertices, uint32_t vertex_count, void* stream) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_device: ctx is NULL");
    if (!r || !d_vertices) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_device: refit/d_vertices is NULL");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_device: the handle was made by racc_hip_refit_create*: racc_hip_scene_rebuild_create makes one that can rebuild");
    if (vertex_count != r->vertexCount) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_device: vertex_count differs from the one the handle was created with");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    sceneRebuildSetHeight(ctx, r->scene, scene_rule::heightBound(r->triCount));      // before anything is enqueued: a launch behind the rebuild has the levels it needs
    return sceneRebuildLaunch(r, static_cast<const float4*>(d_vertices), static_cast<hipStream_t>(stream));
}

int racc_hip_scene_rebuild(racc_hip_ctx* ctx, racc_hip_refit* r, const float* vertices, uint32_t vertex_count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild: ctx is NULL");
    if (!r || !vertices) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild: refit/vertices is NULL");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild: the handle was made by racc_hip_refit_create*: racc_hip_scene_rebuild_create makes one that can rebuild");
    if (vertex_count != r->vertexCount) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild: vertex_count differs from the one the handle was created with");
    for (size_t i = 0; i < size_t(vertex_count); ++i)      // the host rule's refusal (indices were validated at creation)
        if (!std::isfinite(vertices[i * 4]) || !std::isfinite(vertices[i * 4 + 1]) || !std::isfinite(vertices[i * 4 + 2])) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild: a vertex coordinate is not finite");
    if (int rc = racc_hip_synchronize(ctx)) return rc;      // no traversal kernel (a chain's included) is alive while the records change
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpyAsync(r->vertices, vertices, size_t(vertex_count) * 16, hipMemcpyHostToDevice, r->stream), "hipMemcpyAsync(rebuild vertices)");
    sceneRebuildSetHeight(ctx, r->scene, scene_rule::heightBound(r->triCount));
    if (int rc = sceneRebuildLaunch(r, r->vertices, r->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(r->stream), "hipStreamSynchronize(scene rebuild)");
    return sceneRebuildReadHeight(ctx, r, nullptr);
}

int racc_hip_refit_download_remap(racc_hip_ctx* ctx, racc_hip_refit* r, uint32_t* remap_out, uint32_t remap_capacity) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_download_remap: ctx is NULL");
    if (!r || !remap_out) return fail(RACC_HIP_ERR_INVALID, "refit_download_remap: refit/remap_out is NULL");
    const racc_hip_scene* s = r->scene;
    if (remap_capacity < s->info.remap_count) return fail(RACC_HIP_ERR_INVALID, "refit_download_remap: capacity too small");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(remap_out, s->remap, size_t(s->info.remap_count) * 4, hipMemcpyDeviceToHost), "hipMemcpy(remap)");
    return RACC_HIP_OK;
}

int racc_hip_scene_rebuild_check(racc_hip_ctx* ctx, racc_hip_refit* r, uint32_t* height) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_check: ctx is NULL");
    if (!r || !height) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_check: refit/height is NULL");
    if (!r->rebuildWords) return fail(RACC_HIP_ERR_INVALID, "scene_rebuild_check: the handle was made by racc_hip_refit_create*");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    return sceneRebuildReadHeight(ctx, r, height);
}

}  // extern "C"
