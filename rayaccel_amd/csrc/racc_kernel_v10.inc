// racc_kernel_v10.inc — the compressed 4-wide traversal kernel (traverseKernelV10), textually included by racc_hip.hip after
// racc_device.inc.  DESIGN.md §3 "compressed wide nodes".
//
// Why: the counters of profiles/r02 put the CU's vector-memory data-return path at 86 % busy, proportional to the number of
// vector-memory instructions, and a visit of a 64-byte binary node costs four of them whatever the lanes hold.  The 4-wide
// node of racc_kernel_v9.inc halves the visits but doubles the record (128 B, eight loads).  This format keeps the 4-wide
// node in 64 BYTES — four loads per visit, half the visits: half the vector-memory instructions and bytes per ray —
// and V8's LDS footprint (one 64 B stage slot per lane: five workgroups per CU).
//
// Device record (built at upload by quantiseWide in racc_hip.hip from the collapse of racc_kernel_v9.inc's format):
//     +0   child refs[4]     (bit 31: wide inner node | leaf ref (count << 24 | first pair), as in the reference format)
//     +16  origin.x origin.y origin.z scale.x
//     +32  scale.y scale.z | lower x planes, one BYTE per child | upper x planes
//     +48  lower y | upper y | lower z | upper z
// A plane is decoded as fmaf(float(byte), scale, origin) — one rounding, the same on the host — and the host picks every
// byte so that the decoded box CONTAINS the reference's child box (lower planes rounded down, upper planes up, verified with
// that very fmaf).  The distances are then the reference's expression on the decoded plane (Kernels.h:122-123:
// fma(plane, 1/d, -o/d)), which is monotone in the plane, so entry' <= entry and exit' >= exit hold in binary32: every box
// the reference's ray enters, this ray enters.  It may enter more (+1.7 % visits, +14 % pair tests on the bench batch,
// oracle/wide_sim quant=1); a pair test is the reference's own and tFar only shrinks through real hits, so the closest hit
// is the oracle's, bit for bit, except (a) exact-distance ties, as for V9, and (b) a hit the reference's own box test culled
// although its pair test accepts it (box vs triangle rounding at a box face): then this kernel reports the CLOSER hit.
// tests/helpers.py::assert_same_closest_hit allows exactly these two.  Both are COUNTED by the exact model of this format
// (oracle/racc_oracle_wide.c — the host's records walked by the wideStep rule below), to which every instantiation of this
// kernel is held bit for bit (tests/test_gpu_wide_exact.py, tests/test_gpu_edge_cases.py).  On the small test scene, 22,384
// rays (a tile of primaries + 6000 random ones), records that differ from the binary oracle: (a) ties 0, (b) closer hits 0 on
// both trees, plus 2 aliases on the library-default tree (a triangle that spatial splits put into two leaves, met through its
// other reference); on the 40-deep comb 0 / 0 / 0; on tests/helpers.py::tie_scene every one of the 64 records is a tie, and the
// id reported is the one the rule below dictates (tests/test_wide_format.py).
//
// Structure: V8's (racc_kernel_v8.inc) — persistent waves, chained launches, quad-cooperative LDS-DMA fetch, header, leaf
// step and fused step verbatim — with V9's wide step (nearest hit child next, the others pushed in slot order) behind a
// decode: 6 v_cndmask (the direction's signs pick entry and exit bytes), 24 v_cvt_f32_ubyte, 12 + 12 v_pk_fma_f32.
// ASM = false: the same kernel in plain C++ (A/B and cross-check).
// QUEUE_ENV (round 6; what the lazy chain runs, as V8's: racc_kernel_v8.inc): a miss is stored with its direction parked in the rgb slots and
// its ray index queued; when 64 are queued — and before the wave moves on to another batch or ends — all 64 lanes turn one record each into
// probe-image radiance (Kernels.h:213-222).  The queue lives in global memory (args.missQ: this kernel's LDS is full at five workgroups per CU).
template <int BLOCK, int LDS_LEVELS, bool STATS, bool ASM, bool CHAIN = false, bool QUEUE_ENV = false>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5))) traverseKernelV10(const TraverseArgs a) {
    static_assert(BLOCK == 256, "the assembly block addresses the stack with literal strides (level = 1 KiB)");
    static_assert(LDS_LEVELS >= 6, "a wide step writes up to four levels above the top");
    static_assert(!QUEUE_ENV || CHAIN, "the miss queue is the lazy chain's");
    constexpr bool DEFER_ENV = !QUEUE_ENV;
    constexpr uint32_t kStagePiece = 1040u;
    __shared__ uint32_t lds[LDS_LEVELS * BLOCK];
    __shared__ __attribute__((aligned(16))) unsigned char stageAll[(BLOCK / 64) * 4 * kStagePiece];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6)));
    uint32_t* const myLdsKept = lds + tid;                               // level L < LDS_LEVELS lives at myLds[L * BLOCK]
    uint32_t* const mySpillKept = a.spill + (blockIdx.x * BLOCK + tid);  // level L >= LDS_LEVELS at mySpill[(L - LDS_LEVELS) * spillStride]
    // QUEUE_ENV (the lazy chain's instantiation): the cold code carries the probe-image lookup, and the registers below the block's window are
    // short — the lane number and the two stack columns are re-derived where the cold code needs them instead of being kept alive across the
    // block (a volatile asm is not common-subexpression-eliminated): no scratch in this instantiation either (tests/test_abi.py)
    auto laneNow = [&]() -> uint32_t {
        if constexpr (QUEUE_ENV) { uint32_t l_; asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l_)); return l_; }
        else return lane;
    };
    auto ldsNow = [&]() -> uint32_t* { if constexpr (QUEUE_ENV) return lds + (wave * 64u + laneNow()); else return myLdsKept; };
    auto spillNow = [&]() -> uint32_t* { if constexpr (QUEUE_ENV) return a.spill + (blockIdx.x * BLOCK + wave * 64u + laneNow()); else return mySpillKept; };
#define myLds (ldsNow())
#define mySpill (spillNow())
    unsigned char* const stage = stageAll + wave * 4u * kStagePiece;
    const unsigned char* const myRec = stage + (lane & 3u) * kStagePiece + (lane >> 2) * 64u;
    typedef __attribute__((address_space(3))) unsigned char* lbyte_t;
    const uint32_t ldsCol = uint32_t(reinterpret_cast<uintptr_t>((lbyte_t)(reinterpret_cast<unsigned char*>(myLdsKept))));            // LDS byte address of level 0
    const uint32_t stageAddr = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(reinterpret_cast<uintptr_t>((lbyte_t)stage)))));
    const __amdgpu_buffer_rsrc_t nodeRsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(a.nodes), 16, a.nodeCount * 4u, 0x00020000);
    myLdsKept[0] = kDone;       // the sentinel below every ray's stack (own column: no barrier needed)
    const float4* const pairsArr = a.pairs;      // (locals, so that the lambdas below do not capture the argument block)
    const float4* const nodesArr = a.nodes;
    const size_t spillStride = a.spillStride;
    const uint32_t maxIters = a.maxIters;
    // The batch this wave draws rays from: its launch's, then — chained launches — the ones issued after it (racc_kernel_v8.inc).
    const float4* rays = a.rays;
    float4* res0 = a.results;
    float4* res1 = a.results;
    uint32_t* cursor = a.cursor;
    uint32_t count = a.count;
    const ChainDesc* chainCur = CHAIN ? a.chain : nullptr;
    uint32_t srcTag = 0;
    bool everLoaded = false;
    const uint32_t staticWaves = (CHAIN && a.chain) ? 0u : gridDim.x * uint32_t(BLOCK / 64);
    uint32_t dynBase = staticWaves * a.chunk;
    // QUEUE_ENV: this wave's miss queue (64 ray indices with their batch tag, global memory) and how many it holds (wave-uniform)
#define RACC10_GLOBAL(T, ptr) ((__attribute__((address_space(1))) T*)(ptr))
    uint32_t* const missQG = QUEUE_ENV ? a.missQ + (size_t(blockIdx.x) * BLOCK + wave * 64u) : nullptr;
    uint32_t qCount = 0;
#define RACC10_FLUSH_MISSES()                                                                                                           \
    do {                                                                                                                                \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   /* the parked records and queue entries of earlier refill steps have left the wave */ \
        const uint32_t fl_ = laneNow();                                                                                                 \
        if (fl_ < qCount) {                                                                                                             \
            const uint32_t q_ = __hip_atomic_load(RACC10_GLOBAL(const uint32_t, missQG) + fl_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
            float4* const r_ = ((q_ >> 31) ? res1 : res0) + (q_ & 0x7FFFFFFFu);                                                         \
            /* the parked direction, written by a lane of this wave in an earlier refill step: agent-scope loads (they miss the CU's L1) */ \
            const unsigned long long yz_ = __hip_atomic_load(RACC10_GLOBAL(const unsigned long long, r_) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
            const uint32_t yb_ = __hip_atomic_load(RACC10_GLOBAL(const uint32_t, r_) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
            uint32_t ew_ = a.envW, eh_ = a.envH;                                                                                        \
            const float4* ep_ = a.env;                                                                                                  \
            asm volatile("" : "+s"(ew_), "+s"(eh_), "+s"(ep_));   /* (or float(envW), float(envH) are hoisted out of the kernel's loop and kept in spilled VGPRs) */ \
            const float4 e_ = envSample(ep_, ew_, eh_, __uint_as_float(yb_), __uint_as_float(uint32_t(yz_)), __uint_as_float(uint32_t(yz_ >> 32))); \
            *RACC10_GLOBAL(f32x4, r_) = (f32x4){e_.x, e_.y, e_.z, e_.w};                                                                 \
        }                                                                                                                               \
        qCount = 0;                                                                                                                     \
    } while (0)

    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, tNear = 0.f, tFar = 0.f, hitU = 0.f, hitV = 0.f;
    f32x2 iex = {0.f, 0.f}, iey = iex, iez = iex;      // per axis {1/d, -o/d} (Kernels.h:159-160) in ONE register pair: v_pk_fma_f32 broadcasts either half (op_sel)
    int hitIndex = -1;
    uint32_t rayIdx = 0;
    uint32_t node = kEmpty;     // bit31: inner ref | >= kLeafBase: leaf, pairs pending | kDone: awaiting epilogue | kEmpty
    uint32_t sp = 0;            // level of the top stack entry (0 = only the sentinel)
    uint32_t wBeg = (CHAIN && a.chain) ? 0u : min((blockIdx.x * uint32_t(BLOCK / 64) + wave) * a.chunk, count);
    uint32_t wEnd = (CHAIN && a.chain) ? 0u : min(wBeg + a.chunk, count);
    bool exhausted = false;
    uint32_t iter = 0;
    uint32_t stInner = 0, stInnerLanes = 0, stLeaf = 0, stLeafLanes = 0, stRefill = 0, stLoaded = 0, stDeq = 0;
    unsigned long long cyInner = 0, cyLeaf = 0, cyRefill = 0, cyStart = 0;
    if (STATS) cyStart = __builtin_readcyclecounter();
    uint32_t quadLane = lane & 3u;
    asm volatile("" : "+v"(quadLane));      // in a VGPR, so that v_or can take the DPP operand directly
    // policy words for the assembly block: [refillMin | leafMin << 8 | tailActive << 16], [thinReps | innerReps << 8 | flags | deep level << 20]
    const uint32_t pol0 = uint32_t(__builtin_amdgcn_readfirstlane(int(min(a.refillMin, 255u) | (min(a.leafMin, 255u) << 8) | (min(a.tailActive, 255u) << 16) | (min(a.coopNum, 255u) << 24))));
    const uint32_t pol1 = uint32_t(__builtin_amdgcn_readfirstlane(int(min(max(a.thinReps, 1u), 255u) | (min(max(a.innerReps, 1u), 255u) << 8) |
                                                                      (a.noFusedStep ? 0x80000u : 0u) | (uint32_t(LDS_LEVELS - 4) << 20))));
    const uint64_t polA = uint64_t(pol0) | (uint64_t(pol1) << 32);

    auto stackGet = [&](uint32_t level) -> uint32_t {
        uint32_t v = myLds[min(level, uint32_t(LDS_LEVELS - 1)) * BLOCK];
        if (level >= uint32_t(LDS_LEVELS)) {
            uint32_t s_ = mySpill[size_t(level - LDS_LEVELS) * spillStride];
            asm volatile("" : "+v"(s_));      // keeps the two address spaces apart (no flat_load of a selected pointer)
            v = s_;
        }
        return v;
    };
    auto stackPut = [&](uint32_t level, uint32_t v) {
        if (level < uint32_t(LDS_LEVELS)) myLds[level * BLOCK] = v;
        else mySpill[size_t(level - LDS_LEVELS) * spillStride] = v;
    };
    // one pair of every lane that waits at a leaf (Kernels.h:200-205 + 36-115)
    auto leafStep = [&]() {
        if (int(node) >= int(kLeafBase)) {
            const uint32_t cur = node & 0xFFFFFFu;
            const float4 t0 = pairsArr[cur * 3u], t1 = pairsArr[cur * 3u + 1u], t2 = pairsArr[cur * 3u + 2u];
            const uint32_t popped = stackGet(sp);
            LaneRay r;
            r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz; r.tNear = tNear; r.tFar = tFar;
            r.hitIndex = hitIndex; r.hitU = hitU; r.hitV = hitV;
            tFar = pairIntersectData(t0, t1, t2, cur, r);
            hitIndex = r.hitIndex; hitU = r.hitU; hitV = r.hitV;
            const bool more = node >= 2u * kLeafBase;          // pair count > 1
            node = more ? node - 0xFFFFFFu : popped;           // (count - 1, first + 1) | pop
            sp -= more ? 0u : 1u;
        }
    };
    // the four children's planes of one axis side: fmaf(float(byte), scale, origin), one rounding (the host's quantiseWide checks with the same expression)
    auto decode4 = [](uint32_t q, float scale, float origin) -> float4 {
        return make_float4(__builtin_fmaf(float(q & 255u), scale, origin), __builtin_fmaf(float((q >> 8) & 255u), scale, origin),
                           __builtin_fmaf(float((q >> 16) & 255u), scale, origin), __builtin_fmaf(float(q >> 24), scale, origin));
    };
    // one wide node of every lane that holds one (the record's four 16-byte quarters)
    auto wideStep = [&](const u32x4 refs, const u32x4 w1, const u32x4 w2, const u32x4 w3) {
        const float orgX = __uint_as_float(w1.x), orgY = __uint_as_float(w1.y), orgZ = __uint_as_float(w1.z);
        const float sclX = __uint_as_float(w1.w), sclY = __uint_as_float(w2.x), sclZ = __uint_as_float(w2.y);
        const bool sx = dx < 0.0f, sy = dy < 0.0f, sz = dz < 0.0f;      // the direction's signs pick the entry and the exit plane (fma is monotone)
        const float4 nx = decode4(sx ? w2.w : w2.z, sclX, orgX), fx = decode4(sx ? w2.z : w2.w, sclX, orgX);
        const float4 ny = decode4(sy ? w3.y : w3.x, sclY, orgY), fy = decode4(sy ? w3.x : w3.y, sclY, orgY);
        const float4 nz = decode4(sz ? w3.w : w3.z, sclZ, orgZ), fz = decode4(sz ? w3.z : w3.w, sclZ, orgZ);
        const uint32_t popped = stackGet(sp);
        const float tRay = tFar;
        const f32x2 vix = {iex.x, iex.x}, viy = {iey.x, iey.x}, viz = {iez.x, iez.x}, vex = {iex.y, iex.y}, vey = {iey.y, iey.y}, vez = {iez.y, iez.y};
        const f32x2 nx01 = __builtin_elementwise_fma((f32x2){nx.x, nx.y}, vix, vex), nx23 = __builtin_elementwise_fma((f32x2){nx.z, nx.w}, vix, vex);
        const f32x2 fx01 = __builtin_elementwise_fma((f32x2){fx.x, fx.y}, vix, vex), fx23 = __builtin_elementwise_fma((f32x2){fx.z, fx.w}, vix, vex);
        const f32x2 ny01 = __builtin_elementwise_fma((f32x2){ny.x, ny.y}, viy, vey), ny23 = __builtin_elementwise_fma((f32x2){ny.z, ny.w}, viy, vey);
        const f32x2 fy01 = __builtin_elementwise_fma((f32x2){fy.x, fy.y}, viy, vey), fy23 = __builtin_elementwise_fma((f32x2){fy.z, fy.w}, viy, vey);
        const f32x2 nz01 = __builtin_elementwise_fma((f32x2){nz.x, nz.y}, viz, vez), nz23 = __builtin_elementwise_fma((f32x2){nz.z, nz.w}, viz, vez);
        const f32x2 fz01 = __builtin_elementwise_fma((f32x2){fz.x, fz.y}, viz, vez), fz23 = __builtin_elementwise_fma((f32x2){fz.z, fz.w}, viz, vez);
        const float n0 = fmaxf(fmaxf(tNear, nx01.x), fmaxf(ny01.x, nz01.x)), f0 = fminf(fminf(tRay, fx01.x), fminf(fy01.x, fz01.x));
        const float n1 = fmaxf(fmaxf(tNear, nx01.y), fmaxf(ny01.y, nz01.y)), f1 = fminf(fminf(tRay, fx01.y), fminf(fy01.y, fz01.y));
        const float n2 = fmaxf(fmaxf(tNear, nx23.x), fmaxf(ny23.x, nz23.x)), f2 = fminf(fminf(tRay, fx23.x), fminf(fy23.x, fz23.x));
        const float n3 = fmaxf(fmaxf(tNear, nx23.y), fmaxf(ny23.y, nz23.y)), f3 = fminf(fminf(tRay, fx23.y), fminf(fy23.y, fz23.y));
        const float k0 = n0 > f0 ? tRay : n0;      // tFar doubles as "missed" (Kernels.h:131-134, 192-194)
        const float k1 = n1 > f1 ? tRay : n1;
        const float k2 = n2 > f2 ? tRay : n2;
        const float k3 = n3 > f3 ? tRay : n3;
        // the nearest hit child (lowest slot among equals) is visited next, the other hit children go on the stack in slot order
        const bool A = k1 < k0, B = k3 < k2;
        const float k01 = A ? k1 : k0, k23 = B ? k3 : k2;
        const uint32_t r01 = A ? refs.y : refs.x, r23 = B ? refs.w : refs.z;
        const bool C = k23 < k01;
        const float bestKey = C ? k23 : k01;
        const uint32_t best = C ? r23 : r01;
        const bool any = bestKey != tRay;
        uint32_t level = sp;
        if (k0 != tRay && (A || C)) { ++level; stackPut(level, refs.x); }
        if (k1 != tRay && (!A || C)) { ++level; stackPut(level, refs.y); }
        if (k2 != tRay && (B || !C)) { ++level; stackPut(level, refs.z); }
        if (k3 != tRay && !(B && C)) { ++level; stackPut(level, refs.w); }
        node = any ? best : popped;
        sp = any ? level : sp - 1u;
    };
    auto wideStepGlobal = [&]() {      // the slow iteration's fetch: straight from the node array
        if (int(node) < 0) {
            const u32x4* rec = reinterpret_cast<const u32x4*>(nodesArr) + size_t(node & 0x7FFFFFFFu) * 4;
            wideStep(rec[0], rec[1], rec[2], rec[3]);
        }
    };

    bool tripped = false;
    for (;;) {
        // ================= epilogue of finished rays + refill of empty lanes =================
        unsigned long long cyTop = 0;
        if (STATS) { cyTop = __builtin_readcyclecounter(); ++stRefill; }
        bool parked = false;      // QUEUE_ENV: this lane has just stored a miss that still needs its radiance
        if (node == kDone) {     // Kernels.h:213-241
            float4 out;
            if (hitIndex < 0) {
                // DEFER_ENV: park the (clamped) direction in the rgb slots, envShadeKernel turns it into radiance right after this
                // kernel on the same stream; QUEUE_ENV: the same, the wave itself does it later, 64 records at a time (Kernels.h:213-222)
                out = a.env ? make_float4(__uint_as_float(kInvalidTriangle), dx, dy, dz)
                            : make_float4(__uint_as_float(kInvalidTriangle), 0.0f, 0.0f, 0.0f);
                parked = QUEUE_ENV && a.env != nullptr;
            } else {
                uint32_t m = a.remap[hitIndex];
                const uint32_t edge = m >> 30;
                m &= 0x3FFFFFFFu;
                const float bx = hitU, by = hitV, bz = 1.0f - hitU - hitV;
                float u = bx, v = by;
                if (edge == 1u) { u = bz; v = bx; } else if (edge == 2u) { u = by; v = bz; }
                out = make_float4(__uint_as_float(m), tFar, u, v);
            }
            if (CHAIN) ((rayIdx >> 31) ? res1 : res0)[rayIdx & 0x7FFFFFFFu] = out; else res0[rayIdx] = out;
            node = kEmpty;
        }
        if (QUEUE_ENV) {
            const uint64_t missMask = __ballot(parked);
            const uint32_t nMiss = uint32_t(__popcll(missMask));
            if (nMiss) {
                if (qCount + nMiss > 64u) RACC10_FLUSH_MISSES();
                if (parked) *(RACC10_GLOBAL(uint32_t, missQG) + qCount + laneRank(missMask)) = rayIdx;
                qCount += nMiss;
            }
        }
        {
            const uint64_t emptyMask = __ballot(node == kEmpty);
            const uint32_t need = __popcll(emptyMask);
            if (wBeg == wEnd) {
                for (int tries = 0;; ++tries) {
                    if (!exhausted) {
                        if (STATS) ++stDeq;
                        uint32_t b = 0;
                        if (CHAIN && !everLoaded && chainCur) {      // a wave's first draw: look before taking — the kernel may start after its batch has been
                            if (laneNow() == 0) b = __hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // worked off, and 5120 atomics on one word take 50 us
                            if (uint32_t(__builtin_amdgcn_readfirstlane(int(b))) >= count) { exhausted = true; wBeg = wEnd = count; break; }
                        }
                        if (laneNow() == 0) b = atomicAdd(cursor, a.chunk);
                        const uint32_t r0 = __builtin_amdgcn_readfirstlane(b);
                        b = r0 + dynBase;
                        if (b < r0) b = 0xFFFFFFFFu;      // 32-bit wrap: past any batch
                        exhausted = (b >= count) || (b + a.chunk < b);
                        wBeg = exhausted ? count : b;
                        wEnd = exhausted ? count : min(b + a.chunk, count);
                    }
                    if (!CHAIN || !exhausted || !chainCur || tries) break;
                    if (!everLoaded) break;      // a kernel that starts after its batch has been worked off by its predecessors: nothing to do, no walk down the chain
                    // This batch is handed out.  Chained launches: if the launch issued after it is known by now, go on with
                    // that one's rays (resident and final since it was issued; its cursor is shared with whoever else works on
                    // it, its own kernel included — which may not have a slot yet).  Its results are complete once its kernel
                    // and every kernel issued before it have ended: the host orders that.  Tried again at every refill while
                    // the wave drains; a wave whose lanes still hold rays of the batch BEFORE this one waits for them (two
                    // results arrays is what the tag bit can tell apart).
                    uint32_t nx = 0;
                    if (laneNow() == 0) nx = __hip_atomic_load(&chainCur->next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (no acquire: its cache invalidate would empty the L2 under every other wave; the fields below are read by loads of the same scope, issued after this one has returned)
                    nx = uint32_t(__builtin_amdgcn_readfirstlane(int(nx)));
                    if (!nx) break;
                    const uint32_t newTag = srcTag ^ 1u;
                    if (__ballot(node != kEmpty && (rayIdx >> 31) == newTag) != 0ull) break;
                    const ChainDesc* d = a.chainRing + (nx - 1u);
                    unsigned long long pr = 0, po = 0, pc = 0;
                    uint32_t cnt = 0;
                    if (laneNow() == 0) {
                        pr = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&d->rays), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        po = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&d->results), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pc = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(&d->cursor), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        cnt = __hip_atomic_load(&d->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    auto uni64 = [](unsigned long long v) {
                        const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))));
                        return (static_cast<unsigned long long>(hi) << 32) | lo;
                    };
                    rays = reinterpret_cast<const float4*>(uni64(pr));
                    float4* const nr = reinterpret_cast<float4*>(uni64(po));
                    if (QUEUE_ENV) RACC10_FLUSH_MISSES();      // (queued records may carry the tag that is handed out again now)
                    if (newTag) res1 = nr; else res0 = nr;
                    cursor = reinterpret_cast<uint32_t*>(uni64(pc));
                    count = uint32_t(__builtin_amdgcn_readfirstlane(int(cnt)));
                    dynBase = 0u;          // chained launches have no static chunks
                    chainCur = d;
                    srcTag = newTag;
                    exhausted = false;     // and draw the first chunk at once
                }
            }
            const uint32_t take = min(need, wEnd - wBeg);
            const uint32_t rank = laneRank(emptyMask);
            if (node == kEmpty && rank < take) {
                const uint32_t idx = wBeg + rank;
                float4 q0, q1;
                loadRay(rays, idx, CHAIN && a.raysBypassL1 != 0u, q0, q1);
                const bool valid = isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z) && isfinite(q0.w) &&
                                   isfinite(q1.x) && isfinite(q1.y) && isfinite(q1.z) && !isnan(q1.w);
                if (!valid) {   // NaN in the first slot tells envShadeKernel to leave rgb = 0
                    ((CHAIN && srcTag) ? res1 : res0)[idx] = make_float4(__uint_as_float(kInvalidTriangle), (DEFER_ENV && a.env) ? __uint_as_float(0x7FC00000u) : 0.0f, 0.0f, 0.0f);
                } else {
                    const float eps = 1e-10f;   // Kernels.h:149-157
                    ox = q0.x; oy = q0.y; oz = q0.z; tNear = q0.w;
                    dx = (fabsf(q1.x) < eps) ? copysignf(eps, q1.x) : q1.x;
                    dy = (fabsf(q1.y) < eps) ? copysignf(eps, q1.y) : q1.y;
                    dz = (fabsf(q1.z) < eps) ? copysignf(eps, q1.z) : q1.z;
                    tFar = q1.w;
                    const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;    // Kernels.h:159-160
                    const float ex = -ox * ix, ey = -oy * iy, ez = -oz * iz;
                    iex = (f32x2){ix, ex}; iey = (f32x2){iy, ey}; iez = (f32x2){iz, ez};
                    hitIndex = -1; hitU = 0.0f; hitV = 0.0f;
                    rayIdx = CHAIN ? idx | (srcTag << 31) : idx;
                    node = 0x80000000u;     // Kernels.h:164
                    sp = 0;
                }
            }
            wBeg += take;
            everLoaded = everLoaded || take != 0u;
            if (STATS) { stLoaded += take; cyRefill += __builtin_readcyclecounter() - cyTop; }
            if (exhausted && wBeg == wEnd && __ballot(node != kEmpty) == 0ull) break;      // (a chained wave has just looked for a next batch)
        }

        // ================= traverse until a refill is due =================
        if constexpr (!ASM) {
            for (;;) {
                if (++iter > maxIters) { tripped = true; break; }
                if (STATS) cyTop = __builtin_readcyclecounter();
                const uint32_t nInner = __popcll(__ballot(int(node) < 0));
                const uint32_t nLeaf = __popcll(__ballot(int(node) >= int(kLeafBase)));
                const uint32_t nActive = nInner + nLeaf;
                if (nActive == 0u) break;
                if (!exhausted) { if (64u - nActive >= a.refillMin) break; }
                else if (uint32_t(__popcll(__ballot(node == kDone))) >= a.refillMin) break;
                const bool thin = nActive <= a.tailActive;
                const bool doLeaf = nLeaf >= a.leafMin || nInner == 0u || nLeaf * 4u >= nActive;
                const bool doInner = nInner != 0u && (!doLeaf || thin);
                if (doLeaf) {
                    if (STATS) { ++stLeaf; stLeafLanes += nLeaf; }
                    leafStep();
                    if (STATS) { cyLeaf += __builtin_readcyclecounter() - cyTop; cyTop = __builtin_readcyclecounter(); }
                }
                if (doInner) {
                    const uint32_t reps = thin ? a.thinReps : a.innerReps;
                    for (uint32_t rep = 0;; ++rep) {
                        if (STATS) { ++stInner; stInnerLanes += uint32_t(__popcll(__ballot(int(node) < 0))); }
                        {
                            typedef __attribute__((address_space(3))) void* lptr_t;
                            const uint32_t own = int(node) < 0 ? node << 2 : 0xFFFFFFF0u;      // 16 B element index of the record; out of range for lanes without one
                            const uint32_t e0 = uint32_t(__builtin_amdgcn_update_dpp(0, int(own), 0x00, 0xF, 0xF, true)) | quadLane;
                            const uint32_t e1 = uint32_t(__builtin_amdgcn_update_dpp(0, int(own), 0x55, 0xF, 0xF, true)) | quadLane;
                            const uint32_t e2 = uint32_t(__builtin_amdgcn_update_dpp(0, int(own), 0xAA, 0xF, 0xF, true)) | quadLane;
                            const uint32_t e3 = uint32_t(__builtin_amdgcn_update_dpp(0, int(own), 0xFF, 0xF, 0xF, true)) | quadLane;
                            __builtin_amdgcn_struct_ptr_buffer_load_lds(nodeRsrc, (lptr_t)(stage + 0u * kStagePiece), 16, int(e0), 0, 0, 0, 0);
                            __builtin_amdgcn_struct_ptr_buffer_load_lds(nodeRsrc, (lptr_t)(stage + 1u * kStagePiece), 16, int(e1), 0, 0, 0, 0);
                            __builtin_amdgcn_struct_ptr_buffer_load_lds(nodeRsrc, (lptr_t)(stage + 2u * kStagePiece), 16, int(e2), 0, 0, 0, 0);
                            __builtin_amdgcn_struct_ptr_buffer_load_lds(nodeRsrc, (lptr_t)(stage + 3u * kStagePiece), 16, int(e3), 0, 0, 0, 0);
                            __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): the four pieces have landed in the stage
                        }
                        if (int(node) < 0) {
                            const u32x4* rec = reinterpret_cast<const u32x4*>(myRec);
                            wideStep(rec[0], rec[1], rec[2], rec[3]);
                        }
                        if (rep + 1u >= reps || __ballot(int(node) < 0) == 0ull) break;
                    }
                    if (STATS) cyInner += __builtin_readcyclecounter() - cyTop;
                }
            }
        } else {
        uint32_t afterLeaf = 0;
        for (;;) {
            uint32_t code;
            const uint32_t flags = uint32_t(__builtin_amdgcn_readfirstlane(int((exhausted ? 1u : 0u) | (afterLeaf << 1))));
            const uint64_t polB = uint64_t(flags) | (uint64_t(maxIters) << 32);
            iter = uint32_t(__builtin_amdgcn_readfirstlane(int(iter)));      // (wave-uniform by construction; says so to the register allocator)
            asm volatile(
                // ---- entry: unpack the policy, stage addresses, lane constants, this ray's direction signs
                "s_mov_b64 s[40:41], exec\n\t"
                "s_mov_b64 s[80:81], %[polA]\n\t"              // s80 = pol0, s81 = pol1
                "s_mov_b64 s[82:83], %[polB]\n\t"              // s82 = flags, s83 = watchdog limit
                "s_and_b32 s68, s80, 0xff\n\t"                 // refillMin
                "s_bfe_u32 s69, s80, 0x80008\n\t"              // leafMin
                "s_bfe_u32 s70, s80, 0x80010\n\t"              // tailActive
                "s_lshr_b32 s71, s80, 24\n\t"                  // coopPct
                "s_and_b32 s72, s81, 0xff\n\t"                 // thinReps
                "s_bfe_u32 s73, s81, 0x80008\n\t"              // innerReps
                "s_bfe_u32 s79, s81, 0x60014\n\t"              // a stack this high (LDS levels - 4) no longer fits a wide step's writes
                "s_add_u32 s78, s79, 4\n\t"                    // LDS levels
                "s_and_b32 s74, s82, 1\n\t"                    // exhausted
                "s_lshr_b32 s63, s82, 1\n\t"                   // first header after a leaf step
                "s_mov_b32 s66, 0xffffff\n\t"
                "s_add_u32 s75, %[stage], 1040\n\t"
                "s_add_u32 s76, %[stage], 2080\n\t"
                "s_add_u32 s77, %[stage], 3120\n\t"
                "v_mbcnt_lo_u32_b32 v88, -1, 0\n\t"
                "v_mbcnt_hi_u32_b32 v88, -1, v88\n\t"          // lane
                "v_and_b32_e32 v90, 3, v88\n\t"                // lane in quad
                "v_lshrrev_b32_e32 v87, 2, v88\n\t"
                "v_mul_u32_u24_e32 v89, 0x410, v90\n\t"
                "v_lshl_add_u32 v89, v87, 6, v89\n\t"
                "v_add_u32_e32 v89, %[stage], v89\n\t"         // LDS address of this lane's record in the stage: (lane & 3) * 1040 + (lane >> 2) * 64
                "v_cmp_gt_f32_e64 s[92:93], 0, %[dx]\n\t"      // lanes whose ray runs against the axis: entry plane = the upper one
                "v_cmp_gt_f32_e64 s[94:95], 0, %[dy]\n\t"
                "v_cmp_gt_f32_e64 s[96:97], 0, %[dz]\n\t"
                // ---- scheduling header (V8's)
                "L_top%=:\n\t"
                "s_setprio 2\n\t"                                       // wave priority rises toward the next memory request: racc_kernel_v8_hot.inc
                "s_add_u32 %[iter], %[iter], 1\n\t"
                "s_cmp_gt_u32 %[iter], s83\n\t"
                "s_cbranch_scc1 L_trip%=\n\t"
                "v_cmp_gt_i32_e64 s[42:43], 0, %[node]\n\t"             // lanes at an inner node
                "v_cmp_lt_i32_e64 s[44:45], s66, %[node]\n\t"           // lanes at a leaf
                "v_cmp_le_i32_e64 s[50:51], s79, %[sp]\n\t"        // inner lane whose stack leaves no room for a wide step's four writes ...
                "v_cmp_le_i32_e64 s[52:53], s78, %[sp]\n\t"        // ... leaf lane whose top entry is beyond the LDS part
                "s_bcnt1_i32_b64 s46, s[42:43]\n\t"
                "s_bcnt1_i32_b64 s47, s[44:45]\n\t"
                "s_add_u32 s48, s46, s47\n\t"
                "s_cmp_eq_u32 s48, 0\n\t"
                "s_cbranch_scc1 L_refill%=\n\t"
                "s_cmp_lg_u32 s74, 0\n\t"
                "s_cbranch_scc1 L_exh%=\n\t"
                "s_sub_u32 s49, 64, s48\n\t"
                "s_cmp_ge_u32 s49, s68\n\t"
                "s_cbranch_scc1 L_refill%=\n\t"
                "s_branch L_vote%=\n\t"
                "L_exh%=:\n\t"
                "v_cmp_eq_u32_e32 vcc, 1, %[node]\n\t"                  // finished rays waiting for their epilogue
                "s_bcnt1_i32_b64 s49, vcc\n\t"
                "s_cmp_ge_u32 s49, s68\n\t"
                "s_cbranch_scc1 L_refill%=\n\t"
                "L_vote%=:\n\t"
                "s_and_b64 s[50:51], s[50:51], s[42:43]\n\t"
                "s_and_b64 s[52:53], s[52:53], s[44:45]\n\t"
                "s_or_b64 s[50:51], s[50:51], s[52:53]\n\t"
                "s_cmp_lg_u64 s[50:51], 0\n\t"
                "s_cbranch_scc1 L_deep%=\n\t"
                "s_cmp_le_u32 s48, s70\n\t"
                "s_cselect_b32 s61, 1, 0\n\t"                           // thin wave
                "s_cmp_ge_u32 s47, s69\n\t"
                "s_cbranch_scc1 L_wantleaf%=\n\t"
                "s_cmp_eq_u32 s46, 0\n\t"
                "s_cbranch_scc1 L_wantleaf%=\n\t"
                "s_lshl_b32 s49, s47, 2\n\t"
                "s_cmp_ge_u32 s49, s48\n\t"
                "s_cbranch_scc0 L_inner%=\n\t"
                "L_wantleaf%=:\n\t"                                     // a thin wave just back from its leaf step runs its inner lanes too
                "s_and_b32 s49, s63, s61\n\t"
                "s_cmp_lg_u32 s49, 0\n\t"
                "s_cselect_b32 s49, s46, 0\n\t"
                "s_cmp_eq_u32 s49, 0\n\t"
                "s_cbranch_scc1 L_leaf%=\n\t"
                "L_inner%=:\n\t"
                "s_mov_b32 s63, 0\n\t"
                "s_cmp_lg_u32 s61, 0\n\t"
                "s_cselect_b32 s60, s72, s73\n\t"                       // wide steps this iteration
                // fetch mode (as V8): cooperative unless the wave is coherent (lanes holding the same node as their quad neighbour:
                // the addresser merges their per-lane loads) — primary rays, the top of the tree
                "v_mov_b32_dpp v64, %[node] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_cmp_eq_u32_e32 vcc, v64, %[node]\n\t"
                "s_and_b64 vcc, vcc, s[42:43]\n\t"
                "s_bcnt1_i32_b64 s49, vcc\n\t"
                "s_mul_i32 s49, s49, 100\n\t"
                "s_mul_i32 s62, s46, s71\n\t"
                "s_cmp_lt_u32 s49, s62\n\t"
                "s_cselect_b32 s62, 1, 0\n\t"
                // ---- wide step: fetch (quad-cooperative LDS-DMA, as V8's), decode, four slab tests (Kernels.h:117-135), nearest first
                "L_rep%=:\n\t"
                "s_setprio 3\n\t"
                "s_cmp_lg_u32 s62, 0\n\t"
                "s_cbranch_scc1 L_coop%=\n\t"
                "s_mov_b64 exec, s[42:43]\n\t"                          // coherent wave: every lane loads its own record
                "v_lshlrev_b32_e32 v64, 6, %[node]\n\t"                 // byte offset of the 64 B record (bit 31 falls off)
                "v_lshl_add_u32 v87, %[sp], 10, %[ldscol]\n\t"          // LDS address of the top stack entry
                "global_load_dwordx4 v[52:55], v64, %[nodes] offset:16\n\t"
                "global_load_dwordx4 v[56:59], v64, %[nodes] offset:32\n\t"
                "global_load_dwordx4 v[60:63], v64, %[nodes] offset:48\n\t"
                "global_load_dwordx4 v[48:51], v64, %[nodes]\n\t"
                "s_setprio 0\n\t"
                "ds_read_b32 v86, v87\n\t"
                "s_waitcnt vmcnt(0)\n\t"
                "s_branch L_decode%=\n\t"
                "L_coop%=:\n\t"
                "s_mov_b64 exec, s[40:41]\n\t"                          // all 64 lanes: a quad fetches the record of its lane j, 16 B each
                "v_lshl_add_u32 v87, %[sp], 10, %[ldscol]\n\t"          // LDS address of the top stack entry
                "v_lshlrev_b32_e32 v64, 2, %[node]\n\t"                 // 16 B element index of the record
                "s_mov_b32 m0, %[stage]\n\t"
                "v_cndmask_b32_e64 v64, -1, v64, s[42:43]\n\t"          // lanes without an inner node: out of range, nothing is fetched for them
                "s_nop 1\n\t"
                "v_or_b32_dpp v65, v64, v90 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v66, v64, v90 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v67, v64, v90 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v68, v64, v90 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "buffer_load_dwordx4 v65, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s75\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v66, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s76\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v67, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s77\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v68, %[rsrc], 0 idxen lds\n\t"
                "s_setprio 0\n\t"
                "s_waitcnt vmcnt(0)\n\t"                                // the four pieces have landed in the stage
                "L_coopread%=:\n\t"
                "s_mov_b64 exec, s[42:43]\n\t"
                "ds_read_b128 v[52:55], v89 offset:16\n\t"              // frame: origin.x origin.y origin.z scale.x
                "ds_read_b128 v[56:59], v89 offset:32\n\t"              // scale.y scale.z | lower x planes of the four children (a byte each) | upper x
                "ds_read_b128 v[60:63], v89 offset:48\n\t"              // lower y | upper y | lower z | upper z
                "ds_read_b128 v[48:51], v89\n\t"                        // child refs
                "ds_read_b32 v86, v87\n\t"                              // top of the stack
                "L_decode%=:\n\t"
                "s_waitcnt lgkmcnt(3)\n\t"
                "v_cndmask_b32_e64 v64, v59, v58, s[92:93]\n\t"         // the direction's signs pick the entry and the exit plane of each axis
                "v_cndmask_b32_e64 v58, v58, v59, s[92:93]\n\t"
                "s_waitcnt lgkmcnt(2)\n\t"
                "v_cndmask_b32_e64 v65, v61, v60, s[94:95]\n\t"
                "v_cndmask_b32_e64 v60, v60, v61, s[94:95]\n\t"
                "v_cndmask_b32_e64 v66, v63, v62, s[96:97]\n\t"
                "v_cndmask_b32_e64 v62, v62, v63, s[96:97]\n\t"
                "v_cvt_f32_ubyte0_e32 v68, v58\n\t"      // entry x: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v69, v58\n\t"
                "v_cvt_f32_ubyte2_e32 v70, v58\n\t"
                "v_cvt_f32_ubyte3_e32 v71, v58\n\t"
                "v_pk_fma_f32 v[68:69], v[68:69], v[54:55], v[52:53] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[70:71], v[70:71], v[54:55], v[52:53] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"
                "v_pk_fma_f32 v[68:69], v[68:69], %[iex], %[iex] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[70:71], v[70:71], %[iex], %[iex] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_cvt_f32_ubyte0_e32 v72, v60\n\t"      // entry y: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v73, v60\n\t"
                "v_cvt_f32_ubyte2_e32 v74, v60\n\t"
                "v_cvt_f32_ubyte3_e32 v75, v60\n\t"
                "v_pk_fma_f32 v[72:73], v[72:73], v[56:57], v[52:53] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[74:75], v[74:75], v[56:57], v[52:53] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 v[72:73], v[72:73], %[iey], %[iey] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[74:75], v[74:75], %[iey], %[iey] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_cvt_f32_ubyte0_e32 v76, v62\n\t"      // entry z: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v77, v62\n\t"
                "v_cvt_f32_ubyte2_e32 v78, v62\n\t"
                "v_cvt_f32_ubyte3_e32 v79, v62\n\t"
                "v_pk_fma_f32 v[76:77], v[76:77], v[56:57], v[54:55] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[78:79], v[78:79], v[56:57], v[54:55] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"
                "v_pk_fma_f32 v[76:77], v[76:77], %[iez], %[iez] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[78:79], v[78:79], %[iez], %[iez] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_max_f32_e32 v80, v72, v76\n\t"
                "v_max_f32_e32 v81, v73, v77\n\t"
                "v_max_f32_e32 v82, v74, v78\n\t"
                "v_max_f32_e32 v83, v75, v79\n\t"
                "v_max3_f32 v80, %[tnear], v68, v80\n\t"                // entry distances
                "v_max3_f32 v81, %[tnear], v69, v81\n\t"
                "v_max3_f32 v82, %[tnear], v70, v82\n\t"
                "v_max3_f32 v83, %[tnear], v71, v83\n\t"
                "s_setprio 1\n\t"
                "v_cvt_f32_ubyte0_e32 v68, v64\n\t"      // exit x: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v69, v64\n\t"
                "v_cvt_f32_ubyte2_e32 v70, v64\n\t"
                "v_cvt_f32_ubyte3_e32 v71, v64\n\t"
                "v_pk_fma_f32 v[68:69], v[68:69], v[54:55], v[52:53] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[70:71], v[70:71], v[54:55], v[52:53] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"
                "v_pk_fma_f32 v[68:69], v[68:69], %[iex], %[iex] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[70:71], v[70:71], %[iex], %[iex] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_cvt_f32_ubyte0_e32 v72, v65\n\t"      // exit y: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v73, v65\n\t"
                "v_cvt_f32_ubyte2_e32 v74, v65\n\t"
                "v_cvt_f32_ubyte3_e32 v75, v65\n\t"
                "v_pk_fma_f32 v[72:73], v[72:73], v[56:57], v[52:53] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[74:75], v[74:75], v[56:57], v[52:53] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_pk_fma_f32 v[72:73], v[72:73], %[iey], %[iey] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[74:75], v[74:75], %[iey], %[iey] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_cvt_f32_ubyte0_e32 v76, v66\n\t"      // exit z: the four children's grid coordinates
                "v_cvt_f32_ubyte1_e32 v77, v66\n\t"
                "v_cvt_f32_ubyte2_e32 v78, v66\n\t"
                "v_cvt_f32_ubyte3_e32 v79, v66\n\t"
                "v_pk_fma_f32 v[76:77], v[76:77], v[56:57], v[54:55] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"      // plane = fma(q, scale, origin)
                "v_pk_fma_f32 v[78:79], v[78:79], v[56:57], v[54:55] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"
                "v_pk_fma_f32 v[76:77], v[76:77], %[iez], %[iez] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"      // distance = fma(plane, 1/d, -o/d), Kernels.h:122-123
                "v_pk_fma_f32 v[78:79], v[78:79], %[iez], %[iez] op_sel:[0,0,1] op_sel_hi:[1,0,1]\n\t"
                "v_min_f32_e32 v64, v72, v76\n\t"
                "v_min_f32_e32 v65, v73, v77\n\t"
                "v_min_f32_e32 v66, v74, v78\n\t"
                "v_min_f32_e32 v67, v75, v79\n\t"
                "v_min3_f32 v64, %[tfar], v68, v64\n\t"                 // exit distances
                "v_min3_f32 v65, %[tfar], v69, v65\n\t"
                "v_min3_f32 v66, %[tfar], v70, v66\n\t"
                "v_min3_f32 v67, %[tfar], v71, v67\n\t"
                "v_cmp_gt_f32_e64 s[52:53], v80, v64\n\t"
                "v_cmp_gt_f32_e64 s[54:55], v81, v65\n\t"
                "v_cmp_gt_f32_e64 s[56:57], v82, v66\n\t"
                "v_cmp_gt_f32_e64 s[58:59], v83, v67\n\t"
                "v_cndmask_b32_e64 v80, v80, %[tfar], s[52:53]\n\t"     // keys: tFar doubles as "missed" (Kernels.h:131-134, 192-194)
                "v_cndmask_b32_e64 v81, v81, %[tfar], s[54:55]\n\t"
                "v_cndmask_b32_e64 v82, v82, %[tfar], s[56:57]\n\t"
                "v_cndmask_b32_e64 v83, v83, %[tfar], s[58:59]\n\t"
                "s_waitcnt lgkmcnt(1)\n\t"                              // the refs are in
                "v_cmp_lt_f32_e64 s[52:53], v81, v80\n\t"               // A: slot 1 nearer than slot 0
                "v_cmp_lt_f32_e64 s[54:55], v83, v82\n\t"               // B: slot 3 nearer than slot 2
                "v_cmp_neq_f32_e64 s[58:59], v80, %[tfar]\n\t"          // hit masks
                "v_cmp_neq_f32_e64 s[44:45], v81, %[tfar]\n\t"
                "v_cndmask_b32_e64 v68, v80, v81, s[52:53]\n\t"
                "v_cndmask_b32_e64 v69, v48, v49, s[52:53]\n\t"
                "v_cndmask_b32_e64 v70, v82, v83, s[54:55]\n\t"
                "v_cndmask_b32_e64 v71, v50, v51, s[54:55]\n\t"
                "v_cmp_neq_f32_e64 s[46:47], v82, %[tfar]\n\t"
                "v_cmp_lt_f32_e64 s[56:57], v70, v68\n\t"               // C: the nearest is in slots 2/3
                "v_cmp_neq_f32_e64 s[48:49], v83, %[tfar]\n\t"
                "s_or_b64 s[50:51], s[52:53], s[56:57]\n\t"
                "v_cndmask_b32_e64 v68, v68, v70, s[56:57]\n\t"         // nearest key
                "v_cndmask_b32_e64 v69, v69, v71, s[56:57]\n\t"         // nearest child
                "s_and_b64 s[58:59], s[58:59], s[50:51]\n\t"            // slot 0 goes on the stack: hit and not the nearest (A | C)
                "s_orn2_b64 s[50:51], s[56:57], s[52:53]\n\t"
                "s_and_b64 s[44:45], s[44:45], s[50:51]\n\t"            // slot 1: C | ~A
                "s_orn2_b64 s[50:51], s[54:55], s[56:57]\n\t"
                "s_and_b64 s[46:47], s[46:47], s[50:51]\n\t"            // slot 2: B | ~C
                "s_nand_b64 s[50:51], s[54:55], s[56:57]\n\t"
                "s_and_b64 s[48:49], s[48:49], s[50:51]\n\t"            // slot 3: ~(B & C)
                "v_cmp_neq_f32_e32 vcc, v68, %[tfar]\n\t"               // any child hit
                "ds_write_b32 v87, v48 offset:1024\n\t"                 // above the top; counts only if sp is raised
                "v_addc_co_u32_e64 %[sp], s[50:51], 0, %[sp], s[58:59]\n\t"
                "v_lshl_add_u32 v72, %[sp], 10, %[ldscol]\n\t"
                "ds_write_b32 v72, v49 offset:1024\n\t"
                "v_addc_co_u32_e64 %[sp], s[50:51], 0, %[sp], s[44:45]\n\t"
                "v_lshl_add_u32 v73, %[sp], 10, %[ldscol]\n\t"
                "ds_write_b32 v73, v50 offset:1024\n\t"
                "v_addc_co_u32_e64 %[sp], s[50:51], 0, %[sp], s[46:47]\n\t"
                "v_lshl_add_u32 v74, %[sp], 10, %[ldscol]\n\t"
                "ds_write_b32 v74, v51 offset:1024\n\t"
                "v_addc_co_u32_e64 %[sp], s[50:51], 0, %[sp], s[48:49]\n\t"
                "s_andn2_b64 s[52:53], exec, vcc\n\t"                   // nothing hit: pop
                "s_waitcnt lgkmcnt(4)\n\t"                              // the top of the stack is in (the four writes may still be on their way)
                "v_cndmask_b32_e32 %[node], v86, v69, vcc\n\t"
                "v_subb_co_u32_e64 %[sp], s[50:51], %[sp], 0, s[52:53]\n\t"
                "s_sub_u32 s60, s60, 1\n\t"
                "v_cmp_gt_i32_e64 s[42:43], 0, %[node]\n\t"
                "s_cmp_eq_u32 s60, 0\n\t"
                "s_cbranch_scc1 L_repdone%=\n\t"
                "v_cmp_le_i32_e64 s[50:51], s79, %[sp]\n\t"             // (pushes may have raised a stack too far for another fast step)
                "s_and_b64 s[50:51], s[50:51], s[42:43]\n\t"
                "s_cmp_lg_u64 s[50:51], 0\n\t"
                "s_cbranch_scc1 L_repdone%=\n\t"
                "s_cmp_lg_u64 s[42:43], 0\n\t"
                "s_cbranch_scc1 L_rep%=\n\t"
                "L_repdone%=:\n\t"
                "s_mov_b64 exec, s[40:41]\n\t"
                "s_branch L_top%=\n\t"
                // ---- doors
                "L_refill%=:\n\t"
                "s_mov_b32 %[code], 0\n\t"
                "s_branch L_out%=\n\t"
                "L_deep%=:\n\t"
                "s_mov_b32 %[code], 1\n\t"
                "s_branch L_out%=\n\t"
                "L_trip%=:\n\t"
                "s_mov_b32 %[code], 2\n\t"
                "s_branch L_out%=\n\t"
                // ---- leaf step (Kernels.h:200-205 + 36-115): one pair of every lane that waits at a leaf; V8's sequence.
                // Fused step: when inner lanes exist as well, their node records are requested FIRST (the data waits in the
                // stage, no registers), then the leaf lanes' pairs; both fetches are in flight together, the leaf body runs,
                // then the inner lanes read their records back and take one wide step.
                "L_leaf%=:\n\t"
                "s_setprio 3\n\t"
                "s_mov_b32 s67, 0\n\t"
                "s_cmp_eq_u32 s46, 0\n\t"
                "s_cbranch_scc1 L_leafbody%=\n\t"
                "s_bitcmp1_b32 s81, 19\n\t"
                "s_cbranch_scc1 L_leafbody%=\n\t"
                "s_mov_b32 s67, 1\n\t"
                "v_lshlrev_b32_e32 v64, 2, %[node]\n\t"                 // 16 B element index of the record
                "s_mov_b32 m0, %[stage]\n\t"
                "v_cndmask_b32_e64 v64, -1, v64, s[42:43]\n\t"          // lanes without an inner node: out of range, nothing is fetched for them
                "s_nop 1\n\t"
                "v_or_b32_dpp v65, v64, v90 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v66, v64, v90 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v67, v64, v90 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_or_b32_dpp v68, v64, v90 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "buffer_load_dwordx4 v65, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s75\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v66, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s76\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v67, %[rsrc], 0 idxen lds\n\t"
                "s_mov_b32 m0, s77\n\t"
                "s_nop 0\n\t"
                "buffer_load_dwordx4 v68, %[rsrc], 0 idxen lds\n\t"
                "L_leafbody%=:\n\t"
                "s_mov_b64 exec, s[44:45]\n\t"
                "v_and_b32_e32 v86, s66, %[node]\n\t"                  // current pair
                "v_lshl_add_u32 v85, %[sp], 10, %[ldscol]\n\t"
                "v_mul_u32_u24_e32 v87, 48, v86\n\t"
                "ds_read_b32 v84, v85\n\t"                             // top of the stack: the node after this leaf's last pair
                "global_load_dwordx4 v[48:51], v87, %[pairs]\n\t"      // e1.xyz e3.x
                "global_load_dwordx4 v[52:55], v87, %[pairs] offset:16\n\t"   // e2.xyz e3.y
                "global_load_dwordx4 v[56:59], v87, %[pairs] offset:32\n\t"   // p0.xyz e3.z
                "s_setprio 0\n\t"
                "s_waitcnt vmcnt(0)\n\t"
                "v_mul_f32_e64 v60, v50, -v53\n\t"
                "v_mul_f32_e64 v61, v48, -v54\n\t"
                "v_mul_f32_e64 v62, v49, -v52\n\t"
                "v_mul_f32_e64 v63, v59, -v49\n\t"
                "v_mul_f32_e64 v64, v51, -v50\n\t"
                "v_mul_f32_e64 v65, v55, -v48\n\t"
                "v_fmac_f32_e32 v60, v49, v54\n\t"                     // n1 = e1 x e2
                "v_fmac_f32_e32 v61, v50, v52\n\t"
                "v_fmac_f32_e32 v62, v48, v53\n\t"
                "v_fmac_f32_e32 v63, v55, v50\n\t"                     // n2 = e3 x e1
                "v_fmac_f32_e32 v64, v59, v48\n\t"
                "v_fmac_f32_e32 v65, v51, v49\n\t"
                "v_sub_f32_e32 v66, v56, %[ox]\n\t"                    // C = p0 - o
                "v_sub_f32_e32 v67, v57, %[oy]\n\t"
                "v_sub_f32_e32 v68, v58, %[oz]\n\t"
                "v_mul_f32_e64 v69, %[dz], -v67\n\t"
                "v_mul_f32_e64 v70, %[dx], -v68\n\t"
                "v_mul_f32_e64 v71, %[dy], -v66\n\t"
                "v_fmac_f32_e32 v69, %[dy], v68\n\t"                   // R = d x C
                "v_fmac_f32_e32 v70, %[dz], v66\n\t"
                "v_fmac_f32_e32 v71, %[dx], v67\n\t"
                "v_mul_f32_e32 v72, v60, %[dx]\n\t"
                "v_mul_f32_e32 v73, v63, %[dx]\n\t"
                "v_mul_f32_e32 v76, v69, v48\n\t"
                "v_mul_f32_e32 v77, v69, v52\n\t"
                "v_mul_f32_e32 v80, v69, v51\n\t"
                "v_mul_f32_e32 v85, v60, v66\n\t"
                "v_mul_f32_e32 v87, v63, v66\n\t"
                "v_fmac_f32_e32 v72, v61, %[dy]\n\t"
                "v_fmac_f32_e32 v73, v64, %[dy]\n\t"
                "v_fmac_f32_e32 v76, v70, v49\n\t"
                "v_fmac_f32_e32 v77, v70, v53\n\t"
                "v_fmac_f32_e32 v80, v70, v55\n\t"
                "v_fmac_f32_e32 v85, v61, v67\n\t"
                "v_fmac_f32_e32 v87, v64, v67\n\t"
                "v_fmac_f32_e32 v72, v62, %[dz]\n\t"                   // det1 = n1 . d
                "v_fmac_f32_e32 v73, v65, %[dz]\n\t"                   // det2 = n2 . d
                "v_fmac_f32_e32 v76, v71, v50\n\t"                     // R . e1
                "v_fmac_f32_e32 v77, v71, v54\n\t"                     // R . e2
                "v_fmac_f32_e32 v80, v71, v59\n\t"                     // R . e3
                "v_fmac_f32_e32 v85, v62, v68\n\t"                     // n1 . C
                "v_fmac_f32_e32 v87, v65, v68\n\t"                     // n2 . C
                "v_and_b32_e32 v74, 0x80000000, v72\n\t"
                "v_and_b32_e32 v75, 0x80000000, v73\n\t"
                "v_xor_b32_e32 v77, v77, v74\n\t"                      // U1
                "v_xor_b32_e32 v78, v76, v74\n\t"                      // V1
                "v_xor_b32_e32 v79, v76, v75\n\t"
                "v_xor_b32_e32 v80, v80, v75\n\t"
                "v_xor_b32_e32 v85, v85, v74\n\t"                      // T1
                "v_xor_b32_e32 v87, v87, v75\n\t"                      // T2
                "v_xor_b32_e32 v79, 0x80000000, v79\n\t"               // U2 = -(R . e1) ^ sgn2
                "v_xor_b32_e32 v80, 0x80000000, v80\n\t"               // V2 = -(R . e3) ^ sgn2
                "v_or_b32_e32 v81, v77, v78\n\t"
                "v_sub_f32_e64 v83, |v72|, v77\n\t"
                "v_mul_f32_e64 v61, |v72|, %[tnear]\n\t"
                "v_mul_f32_e64 v62, |v72|, %[tfar]\n\t"
                "v_mul_f32_e64 v63, |v73|, %[tnear]\n\t"
                "v_mul_f32_e64 v64, |v73|, %[tfar]\n\t"
                "v_or_b32_e32 v82, v79, v80\n\t"
                "v_sub_f32_e64 v60, |v73|, v79\n\t"
                "v_sub_f32_e32 v83, v83, v78\n\t"                      // W1
                "v_sub_f32_e32 v60, v60, v80\n\t"                      // W2
                "v_mul_f32_e64 v65, v85, |v73|\n\t"
                "v_mul_f32_e64 v66, v87, |v72|\n\t"
                "v_cmp_gt_i32_e64 s[52:53], 0, v81\n\t"
                "v_cmp_le_f32_e64 s[56:57], v85, v61\n\t"
                "v_cmp_gt_f32_e64 s[58:59], v85, v62\n\t"
                "v_cmp_lt_f32_e64 s[54:55], v83, 0\n\t"
                "s_or_b64 s[52:53], s[52:53], s[56:57]\n\t"
                "s_or_b64 s[52:53], s[52:53], s[58:59]\n\t"
                "s_or_b64 s[52:53], s[52:53], s[54:55]\n\t"            // outside the first triangle
                "v_cmp_gt_i32_e64 s[54:55], 0, v82\n\t"
                "v_cmp_le_f32_e64 s[56:57], v87, v63\n\t"
                "v_cmp_gt_f32_e64 s[58:59], v87, v64\n\t"
                "v_cmp_lt_f32_e64 s[50:51], v60, 0\n\t"
                "s_or_b64 s[54:55], s[54:55], s[56:57]\n\t"
                "s_or_b64 s[54:55], s[54:55], s[58:59]\n\t"
                "s_or_b64 s[54:55], s[54:55], s[50:51]\n\t"            // outside the second triangle
                "v_cmp_gt_f32_e64 s[56:57], v65, v66\n\t"              // T1 * |det2| > T2 * |det1|: the second one is nearer
                "s_and_b64 s[58:59], s[52:53], s[54:55]\n\t"
                "s_or_b64 s[56:57], s[56:57], s[52:53]\n\t"
                "s_andn2_b64 s[58:59], exec, s[58:59]\n\t"             // lanes with a hit
                "s_andn2_b64 s[56:57], s[56:57], s[54:55]\n\t"         // ... in the second triangle
                "v_cndmask_b32_e64 v67, |v72|, |v73|, s[56:57]\n\t"
                "v_cndmask_b32_e64 v68, v85, v87, s[56:57]\n\t"
                "v_cndmask_b32_e64 v69, v77, v79, s[56:57]\n\t"
                "v_cndmask_b32_e64 v70, v78, v80, s[56:57]\n\t"
                "v_div_scale_f32 v71, s[50:51], v67, v67, 1.0\n\t"     // 1 / |det|, correctly rounded (hipcc's expansion)
                "v_rcp_f32_e32 v60, v71\n\t"
                "v_cndmask_b32_e64 v61, 0, 1, s[56:57]\n\t"
                "v_lshl_or_b32 v61, v86, 1, v61\n\t"                   // pair * 2 + which
                "v_fma_f32 v62, -v71, v60, 1.0\n\t"
                "v_fmac_f32_e32 v60, v62, v60\n\t"
                "v_div_scale_f32 v62, vcc, 1.0, v67, 1.0\n\t"
                "v_mul_f32_e32 v63, v62, v60\n\t"
                "v_fma_f32 v64, -v71, v63, v62\n\t"
                "v_fmac_f32_e32 v63, v64, v60\n\t"
                "v_fma_f32 v71, -v71, v63, v62\n\t"
                "v_div_fmas_f32 v71, v71, v60, v63\n\t"
                "v_div_fixup_f32 v67, v71, v67, 1.0\n\t"
                "s_mov_b32 s49, 0x2000000\n\t"
                "v_mul_f32_e32 v68, v68, v67\n\t"                      // t
                "v_mul_f32_e32 v69, v69, v67\n\t"                      // u
                "v_mul_f32_e32 v70, v70, v67\n\t"                      // v
                "v_cmp_le_u32_e64 s[52:53], s49, %[node]\n\t"          // more pairs in this leaf
                "v_cndmask_b32_e64 %[tfar], %[tfar], v68, s[58:59]\n\t"
                "v_cndmask_b32_e64 %[hu], %[hu], v69, s[58:59]\n\t"
                "v_cndmask_b32_e64 %[hv], %[hv], v70, s[58:59]\n\t"
                "v_cndmask_b32_e64 %[hidx], %[hidx], v61, s[58:59]\n\t"
                "v_add_u32_e32 v62, 0xff000001, %[node]\n\t"           // (count - 1, first + 1)
                "s_andn2_b64 s[54:55], exec, s[52:53]\n\t"
                "s_waitcnt lgkmcnt(0)\n\t"
                "v_cndmask_b32_e64 %[node], v84, v62, s[52:53]\n\t"    // next pair, or pop
                "v_subb_co_u32_e64 %[sp], vcc, %[sp], 0, s[54:55]\n\t"
                "s_cmp_lg_u32 s67, 0\n\t"
                "s_cbranch_scc0 L_leafend%=\n\t"
                "s_mov_b64 exec, s[42:43]\n\t"                         // fused: the inner lanes' records are in the stage (the leaf body waited vmcnt(0))
                "s_mov_b32 s60, 1\n\t"                                 // one wide step
                "v_lshl_add_u32 v87, %[sp], 10, %[ldscol]\n\t"
                "s_branch L_coopread%=\n\t"
                "L_leafend%=:\n\t"
                "s_mov_b64 exec, s[40:41]\n\t"
                "s_mov_b32 s63, 1\n\t"                                 // a thin wave now runs its inner lanes too
                "s_branch L_top%=\n\t"
                "L_out%=:\n\t"
                "s_setprio 0\n\t"
                "s_mov_b64 exec, s[40:41]\n\t"
                // (the ray's constants are tied in/out operands although the block never writes them: with plain inputs the register
                //  allocator kept a second copy of them live around the block and spilled it — six scratch dwords per lane per refill,
                //  which is where profiles/r02's 7.7 x write traffic came from)
                : [node] "+v"(node), [sp] "+v"(sp), [tfar] "+v"(tFar), [hidx] "+v"(hitIndex), [hu] "+v"(hitU), [hv] "+v"(hitV), [code] "=s"(code), [iter] "+s"(iter),
                  [tnear] "+v"(tNear), [ox] "+v"(ox), [oy] "+v"(oy), [oz] "+v"(oz), [dx] "+v"(dx), [dy] "+v"(dy), [dz] "+v"(dz),
                  [iex] "+v"(iex), [iey] "+v"(iey), [iez] "+v"(iez)
                : [ldscol] "v"(ldsCol), [pairs] "s"(pairsArr), [nodes] "s"(nodesArr), [rsrc] "s"(nodeRsrc), [stage] "s"(stageAddr),
                  [polA] "s"(polA), [polB] "s"(polB)
                : "memory", "vcc", "scc",
                  "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59",
                  "s60", "s61", "s62", "s63", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83",
                  "s92", "s93", "s94", "s95", "s96", "s97",
                  "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63",
                  "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79",
                  "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90");
            afterLeaf = 0;
            if (code == 0u) break;                                   // REFILL
            if (code == 2u) { tripped = true; break; }               // TRIP
            // DEEP: one spill-aware iteration — a pair for every leaf lane, then a wide step for every inner lane
            if (STATS) { ++stLeaf; stLeafLanes += uint32_t(__popcll(__ballot(int(node) >= int(kLeafBase)))); }
            leafStep();
            wideStepGlobal();
        }
        }
        if (tripped) {
            if (laneNow() == 0) __hip_atomic_fetch_add(a.trips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
    }

    if (QUEUE_ENV) RACC10_FLUSH_MISSES();      // what is still queued when the wave ends
#undef RACC10_FLUSH_MISSES
#undef RACC10_GLOBAL
    if (STATS && lane == 0) {
        atomicAdd(a.stats + 0, (unsigned long long)stInner); atomicAdd(a.stats + 1, (unsigned long long)stInnerLanes);
        atomicAdd(a.stats + 2, (unsigned long long)stLeaf);  atomicAdd(a.stats + 3, (unsigned long long)stLeafLanes);
        atomicAdd(a.stats + 4, (unsigned long long)stRefill); atomicAdd(a.stats + 5, (unsigned long long)stLoaded);
        atomicAdd(a.stats + 6, (unsigned long long)stDeq);   atomicAdd(a.stats + 7, 1ull);
        atomicAdd(a.stats + 8, cyInner); atomicAdd(a.stats + 10, cyLeaf); atomicAdd(a.stats + 12, cyRefill);
        atomicAdd(a.stats + 13, (unsigned long long)(__builtin_readcyclecounter() - cyStart));
    }
#undef myLds
#undef mySpill
    __syncthreads();
    if (QUEUE_ENV ? (wave == 0u && laneNow() == 0u) : tid == 0u) {
        if (a.rearm) {
            const uint32_t prev = atomicInc(a.cursor + 1, gridDim.x - 1);
            if (prev == gridDim.x - 1) atomicExch(a.cursor, 0u);
        }
    }
}

