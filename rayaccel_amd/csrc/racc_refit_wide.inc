// racc_refit_wide.inc — refit of the 4-wide (format 45) and compressed (format 50) copies of a scene: the rule as a host function
// (racc_host_scene_wide_nodes_refit), refitWideKernel and the C-ABI entries around it (racc_hip_refit_create_wide,
// racc_hip_refit_download_wide, racc_hip_refit_check).  Textually included by racc_hip_unit.hip BEHIND racc_refit.inc, whose handle it
// extends (racc_hip_refit::wide*) and whose refitLaunch calls refitWideLaunch behind refitBoxesKernel on the same stream.  Not a hashed
// file (DESIGN.md §3, the fingerprint rule): racc_scene_format.inc's collapseWide / quantiseWide stay as they are, and what a refit
// needs of them is restated here:
//   collapseWideSources  collapseWide's selection rule once more, recording per slot WHICH binary child box it copies.  Held equal to
//                        collapseWide by racc_hip_refit_create_wide (the replayed references must be the device's) and by the
//                        identity test (tests/test_wide_refit_host.py: now == built gives racc_host_scene_wide_nodes byte for byte).
//   wideFrameScale, wideLowerByte, wideUpperByte   quantiseWide's result stated without its starting guess, one __host__ __device__
//                        text for the host rule and the kernel.
// The collapse is decided by the blob the scene was uploaded from and kept, as the binary refit keeps its topology: which boxes share a
// wide record no longer follows the moved boxes' areas, so the wide tree degrades with motion like the binary one does.
//
// The kernel: four lanes per wide record, lane = slot.  Each lane gathers its slot's box (24 B) from the binary device record through
// racc_hip_refit::wideSources.  Format 45: the lane writes its column of the six plane vectors.  Format 50: the quad folds the frame
// with __shfl_xor (width 4), every lane derives the three scales and its own six bytes, the bytes are OR-combined across the quad and
// the record's words 4-15 leave as three 16-byte stores; the references (words 0-3) are never written.

namespace {

constexpr uint32_t kWideNone = 0xFFFFFFFFu;      // source of an unused slot

// The fold of a frame's lower / upper corner keeps the accumulator on a tie: of +0.0 and -0.0 the one met first stays, which is what
// quantiseWide's std::fmin / std::fmax fold returns in this build (tests/test_wide_refit_host.py pins it) and not what a device fmin gives.
__host__ __device__ __forceinline__ float wideMin(float acc, float b) { return b < acc ? b : acc; }
__host__ __device__ __forceinline__ float wideMax(float acc, float b) { return b > acc ? b : acc; }

// scale: the correctly rounded (hi - lo) / 255, FLT_MIN where that is not positive, raised until the last byte reaches the upper corner
__host__ __device__ __forceinline__ float wideFrameScale(float lo, float hi) {
    float scale = (hi - lo) / 255.0f;
    if (!(scale > 0.0f)) scale = 1.17549435e-38f;
    while (__builtin_fmaf(255.0f, scale, lo) < hi) scale = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, scale) + 1u);      // nextafter of a positive float
    return scale;
}

// the largest a in [0, 255] with fmaf(a, scale, org) <= plane (a = 0 satisfies it: org is the fold of the lower planes)
__host__ __device__ __forceinline__ uint32_t wideLowerByte(float plane, float scale, float org) {
    uint32_t a = 0u;
#pragma unroll
    for (uint32_t bit = 128u; bit; bit >>= 1) {
        const uint32_t t = a | bit;
        if (__builtin_fmaf(float(t), scale, org) <= plane) a = t;
    }
    return a;
}

// the smallest b in [0, 255] with fmaf(b, scale, org) >= plane (b = 255 satisfies it: wideFrameScale)
__host__ __device__ __forceinline__ uint32_t wideUpperByte(float plane, float scale, float org) {
    uint32_t x = 0u;      // the largest byte that decodes BELOW the plane, if any does
#pragma unroll
    for (uint32_t bit = 128u; bit; bit >>= 1) {
        const uint32_t t = x | bit;
        if (__builtin_fmaf(float(t), scale, org) < plane) x = t;
    }
    const uint32_t b = __builtin_fmaf(0.0f, scale, org) < plane ? x + 1u : 0u;
    return b > 255u ? 255u : b;
}

__host__ __device__ __forceinline__ bool wideFinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u; }

constexpr int kRefitWideBlock = 256;      // 64 records per workgroup

__global__ void __launch_bounds__(kRefitWideBlock) refitWideKernel(const float* __restrict__ nodes, const uint32_t* __restrict__ sources, uint32_t wideCount,
                                                                   float* wide45, uint4* wide50, uint32_t* disabled) {
    const uint32_t i = blockIdx.x * uint32_t(kRefitWideBlock) + threadIdx.x;
    const uint32_t rec = i >> 2, slot = i & 3u;
    if (rec >= wideCount) return;      // (whole quads leave together)
    const uint32_t src = sources[i];
    const bool used = src != kWideNone;
    float lo[3], hi[3];
    if (used) {
        const float2* b = reinterpret_cast<const float2*>(nodes + size_t(src >> 1) * 16 + 4 + (src & 1u) * 6);      // (min, max) of x, y, z: 8-byte aligned on either side
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float2 p = b[ax];
            lo[ax] = p.x < p.y ? p.x : p.y;      // collapseWide's per-axis ordering
            hi[ax] = p.x < p.y ? p.y : p.x;
        }
    } else {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { lo[ax] = __builtin_inff(); hi[ax] = -__builtin_inff(); }      // neutral in the folds below
    }
    if (wide45 && used) {
        float* w = wide45 + size_t(rec) * 32 + 4 + slot;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { w[8 * ax] = lo[ax]; w[8 * ax + 4] = hi[ax]; }
    }
    if (!wide50) return;
    int bad = used && !(wideFinite(lo[0]) && wideFinite(lo[1]) && wideFinite(lo[2]) && wideFinite(hi[0]) && wideFinite(hi[1]) && wideFinite(hi[2]));
    bad |= __shfl_xor(bad, 1, 4);
    bad |= __shfl_xor(bad, 2, 4);
    float org[3], scl[3];
    uint32_t q[6];
    if (!bad) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            // the fold in slot order — the lower slot's value is the accumulator at either step, and "the first met stays" is associative
            float mn = lo[ax], mx = hi[ax];
            float o = __shfl_xor(mn, 1, 4); mn = (slot & 1u) ? wideMin(o, mn) : wideMin(mn, o);
            o = __shfl_xor(mn, 2, 4);       mn = (slot & 2u) ? wideMin(o, mn) : wideMin(mn, o);
            o = __shfl_xor(mx, 1, 4);       mx = (slot & 1u) ? wideMax(o, mx) : wideMax(mx, o);
            o = __shfl_xor(mx, 2, 4);       mx = (slot & 2u) ? wideMax(o, mx) : wideMax(mx, o);
            const float scale = wideFrameScale(mn, mx);
            if (!wideFinite(scale) || !wideFinite(mn)) bad = 1;      // (the same in all four lanes)
            org[ax] = mn; scl[ax] = scale;
            q[2 * ax] = (used ? wideLowerByte(lo[ax], scale, mn) : 255u) << (8u * slot);
            q[2 * ax + 1] = (used ? wideUpperByte(hi[ax], scale, mn) : 0u) << (8u * slot);
        }
    }
    if (bad) {      // a frame the format cannot hold: every slot unused, every plane decodes to +inf
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) { org[ax] = __builtin_inff(); scl[ax] = 1.17549435e-38f; q[2 * ax] = 255u << (8u * slot); q[2 * ax + 1] = 0u; }
        if (slot == 0u) atomicAdd(disabled, 1u);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        q[k] |= __shfl_xor(q[k], 1, 4);
        q[k] |= __shfl_xor(q[k], 2, 4);
    }
    uint4* out = wide50 + size_t(rec) * 4;      // words 0-3: the references, left alone
    if (slot == 0u) out[1] = make_uint4(__float_as_uint(org[0]), __float_as_uint(org[1]), __float_as_uint(org[2]), __float_as_uint(scl[0]));
    else if (slot == 1u) out[2] = make_uint4(__float_as_uint(scl[1]), __float_as_uint(scl[2]), q[0], q[1]);
    else if (slot == 2u) out[3] = make_uint4(q[2], q[3], q[4], q[5]);
}

// collapseWide (racc_scene_format.inc) with the source of every slot: src = 2 * blob node + side of the child box the slot copies
struct WideSources { uint32_t ref[4], src[4], used; };

void collapseWideSources(const GpuNodeHost* in, uint32_t n, std::vector<WideSources>& out) {
    struct Cand { uint32_t ref, src; };
    auto area = [&](const Cand& c) {
        const float* b = in[c.src >> 1].box + (c.src & 1u) * 6;      // min[3], max[3]
        const double x = double(b[3]) - b[0], y = double(b[4]) - b[1], z = double(b[5]) - b[2];
        return x * y + x * z + y * z;
    };
    std::vector<uint32_t> queue;      // breadth first, blob indices; a wide node's number is its position
    queue.reserve(n); out.clear(); out.reserve(n / 2 + 1);
    queue.push_back(0);
    const uint32_t firstLeaf = (in[0].first & 0x80000000u) ? 0x01000000u : in[0].first;
    for (size_t qh = 0; qh < queue.size(); ++qh) {
        const uint32_t g = queue[qh];
        Cand c[4]; int k = 2;
        c[0] = Cand{in[g].first, g * 2u}; c[1] = Cand{in[g].last, g * 2u + 1u};
        while (k < 4) {
            int best = -1; double bestA = -1.0;
            for (int i = 0; i < k; ++i)
                if ((c[i].ref & 0x80000000u) && area(c[i]) > bestA) { bestA = area(c[i]); best = i; }
            if (best < 0) break;
            const uint32_t m = c[best].ref & 0x7FFFFFFFu;
            for (int i = k; i > best + 1; --i) c[i] = c[i - 1];
            c[best] = Cand{in[m].first, m * 2u}; c[best + 1] = Cand{in[m].last, m * 2u + 1u};
            ++k;
        }
        WideSources w{};
        for (int i = 0; i < 4; ++i) {
            if (i < k) {
                uint32_t r = c[i].ref;
                if (r & 0x80000000u) { const uint32_t t = r & 0x7FFFFFFFu; r = 0x80000000u | uint32_t(queue.size()); queue.push_back(t); }
                w.ref[i] = r; w.src[i] = c[i].src;
            } else { w.ref[i] = firstLeaf; w.src[i] = kWideNone; }
        }
        w.used = uint32_t(k);
        out.push_back(w);
    }
}

int refitWideLaunch(racc_hip_refit* r, hipStream_t st) {
    const racc_hip_scene* s = r->scene;
    HIP_TRY(hipMemsetAsync(r->wideDisabled, 0, sizeof(uint32_t), st), "hipMemsetAsync(wide refit count)");
    const uint32_t threads = r->wideCount * 4u;      // (wideCount <= 2^26: validateScene)
    hipLaunchKernelGGL(refitWideKernel, dim3((threads + kRefitWideBlock - 1) / kRefitWideBlock), dim3(kRefitWideBlock), 0, st, reinterpret_cast<const float*>(s->nodes),
                       reinterpret_cast<const uint32_t*>(r->wideSources), r->wideCount, reinterpret_cast<float*>(s->nodesWide), reinterpret_cast<uint4*>(s->nodesWideQ), r->wideDisabled);
    HIP_TRY(hipGetLastError(), "launch refitWideKernel");
    return RACC_HIP_OK;
}

void refitWideDetach(racc_hip_refit* r) {
    if (r->wideSources) hipFree(r->wideSources);
    if (r->wideDisabled) hipFree(r->wideDisabled);
    if (r->wideClaimed) sceneReleaseWideRefit(r->scene);
    r->wideSources = nullptr; r->wideDisabled = nullptr; r->wideClaimed = false; r->wideCount = 0;
}

// The handle is complete as a plain one.  Replays the collapse on the binary records as the device holds them — no refit can have touched
// them: the plain create refuses this scene and this is its first wide handle — and checks the replayed references against the device's.
int refitWideAttach(racc_hip_refit* r) {
    racc_hip_scene* s = r->scene;
    if (!sceneClaimWideRefit(s)) return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: the scene already has a wide refit handle (at most one per scene)");
    r->wideClaimed = true;
    const uint32_t nodeCount = r->topology->nodeCount, wideCount = s->wideCount;
    std::vector<float> dev(size_t(s->deviceNodes) * 16);
    HIP_TRY(hipMemcpy(dev.data(), s->nodes, dev.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(device nodes)");
    std::vector<GpuNodeHost> blob(nodeCount);
    for (uint32_t b = 0; b < nodeCount; ++b) {
        std::memcpy(&blob[b], &r->topology->words[size_t(b) * 4], 16);
        const uint32_t d = r->blobToDevice[b];
        if (d == kRefitRoot) continue;      // not reached from the root: the collapse does not reach it either
        const float* p = &dev[size_t(d) * 16 + 4];
        for (int side = 0; side < 2; ++side)
            for (int k = 0; k < 3; ++k) { blob[b].box[side * 6 + k] = p[side * 6 + 2 * k]; blob[b].box[side * 6 + 3 + k] = p[side * 6 + 2 * k + 1]; }
    }
    std::vector<WideSources> wide;
    collapseWideSources(blob.data(), nodeCount, wide);
    if (wide.size() != wideCount) return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: the replayed collapse does not give the device's wide records");
    for (const float4* copy : {s->nodesWide, s->nodesWideQ}) {
        if (!copy) continue;
        const size_t words = copy == s->nodesWide ? 32 : 16;      // per record; the references are words 0-3 of either format
        std::vector<uint32_t> records(size_t(wideCount) * words);
        HIP_TRY(hipMemcpy(records.data(), copy, records.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(wide records)");
        for (uint32_t w = 0; w < wideCount; ++w)
            if (std::memcmp(&records[size_t(w) * words], wide[w].ref, 16) != 0) return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: the replayed collapse does not give the device's wide records");
    }
    std::vector<uint32_t> sources(size_t(wideCount) * 4);
    for (uint32_t w = 0; w < wideCount; ++w)
        for (int i = 0; i < 4; ++i) {
            const uint32_t src = wide[w].src[i];
            sources[size_t(w) * 4 + i] = src == kWideNone ? kWideNone : r->blobToDevice[src >> 1] * 2u + (src & 1u);      // (a node the collapse reaches has a device record)
        }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->wideSources), sources.size() * 4), "hipMalloc(wide refit sources)");
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->wideDisabled), sizeof(uint32_t)), "hipMalloc(wide refit count)");
    HIP_TRY(hipMemcpy(r->wideSources, sources.data(), sources.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(wide refit sources)");
    HIP_TRY(hipMemset(r->wideDisabled, 0, sizeof(uint32_t)), "hipMemset(wide refit count)");
    r->wideCount = wideCount;
    return RACC_HIP_OK;
}

}  // namespace

extern "C" {

int racc_hip_refit_create_wide(racc_hip_ctx* ctx, racc_hip_scene* scene, const uint32_t* indices, uint32_t index_count, uint32_t vertex_count,
                               racc_hip_refit** out) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_create_wide: ctx is NULL");
    return refitCreate(ctx, scene, indices, index_count, vertex_count, true, out);
}

int racc_hip_refit_download_wide(racc_hip_ctx* ctx, racc_hip_refit* r, int format, void* out, uint32_t capacity, uint32_t* count) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_download_wide: ctx is NULL");
    if (!r || !count) return fail(RACC_HIP_ERR_INVALID, "refit_download_wide: refit/count is NULL");
    *count = 0;
    if (format != 45 && format != 50) return fail(RACC_HIP_ERR_INVALID, "refit_download_wide: format must be 45 (128 B records) or 50 (64 B compressed records)");
    const racc_hip_scene* s = r->scene;
    const float4* copy = format == 45 ? s->nodesWide : s->nodesWideQ;
    if (!copy) return fail(RACC_HIP_ERR_INVALID, "refit_download_wide: the scene carries no copy of that format");
    *count = s->wideCount;
    if (!out) return RACC_HIP_OK;
    if (capacity < s->wideCount) return fail(RACC_HIP_ERR_INVALID, "refit_download_wide: capacity too small");
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(out, copy, size_t(s->wideCount) * (format == 45 ? 128 : 64), hipMemcpyDeviceToHost), "hipMemcpy(wide records)");
    return RACC_HIP_OK;
}

int racc_hip_refit_check(racc_hip_ctx* ctx, racc_hip_refit* r, uint32_t* disabled_frames) {
    if (!ctx) return fail(RACC_HIP_ERR_INVALID, "refit_check: ctx is NULL");
    if (!r || !disabled_frames) return fail(RACC_HIP_ERR_INVALID, "refit_check: refit/disabled_frames is NULL");
    *disabled_frames = 0;
    if (!r->wideDisabled) return RACC_HIP_OK;      // a plain handle: the binary format holds every finite box
    HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
    HIP_TRY(hipMemcpy(disabled_frames, r->wideDisabled, sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy(disabled frames)");
    return RACC_HIP_OK;
}

int racc_host_scene_wide_nodes_refit(const void* nodes64_built, const void* nodes64_now, uint32_t node_count, uint32_t pair_count, uint32_t remap_count,
                                     int format, void* out, uint32_t capacity, uint32_t* count, uint32_t* disabled_frames) try {
    if (!nodes64_built || !nodes64_now || !count || !disabled_frames) return fail(RACC_HIP_ERR_INVALID, "wide_nodes_refit: NULL argument");
    *count = 0; *disabled_frames = 0;
    if (format != 45 && format != 50) return fail(RACC_HIP_ERR_INVALID, "wide_nodes_refit: format must be 45 (128 B records) or 50 (64 B compressed records)");
    const GpuNodeHost* built = static_cast<const GpuNodeHost*>(nodes64_built);
    const GpuNodeHost* now = static_cast<const GpuNodeHost*>(nodes64_now);
    racc_hip_scene_info info{};
    if (int rc = validateScene(built, node_count, pair_count, remap_count, info)) return rc;
    for (uint32_t b = 0; b < node_count; ++b)
        if (built[b].first != now[b].first || built[b].last != now[b].last) return fail(RACC_HIP_ERR_INVALID, "wide_nodes_refit: the two blobs differ in a child reference (a refit keeps the topology)");
    std::vector<WideSources> wide;
    collapseWideSources(built, node_count, wide);
    *count = uint32_t(wide.size());
    if (!out) {      // the count of disabled frames needs the records: only *count without them
        return RACC_HIP_OK;
    }
    if (capacity < wide.size()) return fail(RACC_HIP_ERR_INVALID, "wide_nodes_refit: capacity too small");
    const float inf = std::numeric_limits<float>::infinity();
    uint32_t disabled = 0;
    for (size_t n = 0; n < wide.size(); ++n) {
        const WideSources& w = wide[n];
        float lo[3][4], hi[3][4];
        bool finite = true;
        for (int i = 0; i < 4; ++i)
            for (int ax = 0; ax < 3; ++ax) {
                if (uint32_t(i) >= w.used) { lo[ax][i] = hi[ax][i] = inf; continue; }
                const float* b = now[w.src[i] >> 1].box + (w.src[i] & 1u) * 6;
                const float mn = b[ax], mx = b[3 + ax];
                lo[ax][i] = mn < mx ? mn : mx; hi[ax][i] = mn < mx ? mx : mn;
                finite = finite && wideFinite(lo[ax][i]) && wideFinite(hi[ax][i]);
            }
        if (format == 45) {
            WideNode r{};
            std::memcpy(r.ref, w.ref, 16);
            for (int ax = 0; ax < 3; ++ax)
                for (int i = 0; i < 4; ++i) { r.plane[2 * ax][i] = lo[ax][i]; r.plane[2 * ax + 1][i] = hi[ax][i]; }
            r.used = w.used;
            std::memcpy(static_cast<char*>(out) + n * sizeof(WideNode), &r, sizeof(WideNode));
            continue;
        }
        WideNodeQ r{};
        std::memcpy(r.ref, w.ref, 16);
        float scl[3] = {};
        bool bad = !finite;
        for (int ax = 0; ax < 3 && !bad; ++ax) {
            float mn = inf, mx = -inf;
            for (uint32_t i = 0; i < w.used; ++i) { mn = wideMin(mn, lo[ax][i]); mx = wideMax(mx, hi[ax][i]); }
            const float scale = wideFrameScale(mn, mx);
            if (!wideFinite(scale) || !wideFinite(mn)) { bad = true; break; }
            r.org[ax] = mn; scl[ax] = scale;
            for (uint32_t i = 0; i < 4; ++i) {
                const bool used = i < w.used;
                r.q[2 * ax] |= (used ? wideLowerByte(lo[ax][i], scale, mn) : 255u) << (8u * i);
                r.q[2 * ax + 1] |= (used ? wideUpperByte(hi[ax][i], scale, mn) : 0u) << (8u * i);
            }
        }
        if (bad) {
            ++disabled;
            for (int ax = 0; ax < 3; ++ax) { r.org[ax] = inf; scl[ax] = std::numeric_limits<float>::min(); r.q[2 * ax] = 0xFFFFFFFFu; r.q[2 * ax + 1] = 0u; }
        }
        r.sclX = scl[0]; r.sclY = scl[1]; r.sclZ = scl[2];
        std::memcpy(static_cast<char*>(out) + n * sizeof(WideNodeQ), &r, sizeof(WideNodeQ));
    }
    *disabled_frames = disabled;
    return RACC_HIP_OK;
} catch (const std::bad_alloc&) {
    return fail(RACC_HIP_ERR_NOMEM, "wide_nodes_refit: out of host memory");
}

}  // extern "C"
