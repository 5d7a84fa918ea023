/*
 * racc_hip.h — C-ABI of the MI355X (gfx950) intersect-batch engine.
 *
 * This is the boundary the reference's host code would bind instead of its
 * OpenCL calls: plain pointers and sizes, `int` status (0 = ok, <0 = error,
 * text via racc_hip_last_error()), never throws, no torch/HIP types in any
 * signature.  Each entry cites the reference interface it replaces
 * (file:line relative to the reference checkout).  The reference-side stubs a
 * maintainer would add are shown in INTEGRATION.md.
 *
 * Record layouts are the reference's, byte for byte:
 *   Ray     32 B  {origin[3], minT, dir[3], maxT}         RayAccelerator.h:59-64
 *   Result  16 B  {u32 triangle; t,u,v | r,g,b}           RayAccelerator.h:66-76
 *                 triangle == 0xFFFFFFFF => miss, floats = environment rgb
 *   Node    64 B  {kind,parent,first,last, leftMin[3],leftMax[3],
 *                  rightMin[3],rightMax[3]}                Scene.cpp:73-78
 *   Pair    48 B  {e1.xyz,e3.x, e2.xyz,e3.y, p0.xyz,e3.z}  Scene.cpp:83-87
 *   remap   u32   tri | edge<<30, two per pair             Scene.cpp:132-133
 */
#ifndef RACC_HIP_H
#define RACC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RACC_HIP_OK                 0
#define RACC_HIP_ERR_INVALID       -1   /* bad argument / malformed scene blob */
#define RACC_HIP_ERR_DEVICE        -2   /* a HIP call failed */
#define RACC_HIP_ERR_NO_DEVICE     -3   /* no gfx950 device / extension unusable */
#define RACC_HIP_ERR_LIMIT         -4   /* scene exceeds a format limit (Scene.cpp:294-312) */
#define RACC_HIP_ERR_NOMEM         -5

#define RACC_HIP_MAX_LANES          8   /* >= gpuSubmissionThreads (RayAccelerator.cpp:436) */
#define RACC_HIP_LANE_AUTO 0xFFFFFFFFu  /* racc_hip_intersect_device: the engine picks the lane, round robin; racc_hip_wait: all lanes */

typedef struct racc_hip_ctx   racc_hip_ctx;    /* one per (process, GPU) */
typedef struct racc_hip_scene racc_hip_scene;  /* device-resident flattened BVH2 + pairs */
typedef struct racc_hip_env   racc_hip_env;    /* device-resident RGBA32F probe image */
typedef struct racc_host_scene racc_host_scene;/* host-side build product (reference-format blobs) */

typedef struct racc_hip_options {
    uint32_t struct_size;      /* = sizeof(racc_hip_options) */
    uint32_t lanes;            /* concurrent submission lanes, each with its own HIP stream (0 => default, racc_hip_lane_count)
                                  (≙ gpuSubmissionThreads queues, RayAccelerator.cpp:711-717); 0 => 4 */
    uint32_t waves_per_simd;   /* persistent-grid occupancy target, 1..8; 0 => engine default */
    uint32_t kernel_variant;   /* 0 => engine default (V8: reference traversal order, results bit-identical to the oracle);
                                  50 => the compressed 4-wide kernel (V10: 64-byte nodes, child boxes quantised conservatively to
                                  8 bits — half the node bytes and vector-memory instructions per ray; 4-8 % faster on incoherent
                                  batches; same closest hit except exact-distance ties and hits the reference's own box test drops
                                  although its pair test accepts them: there the CLOSER hit, confirmed by the double-precision
                                  arbiter, is reported); 45 => the uncompressed 4-wide kernel (V9, 128-byte nodes); 60-63 => the
                                  default kernel with the top of the tree (524 / 768 / 260 / 128 node records) held in LDS, 16
                                  waves per CU as workgroups of 1024 / 1024 / 512 / 256 threads: bit-identical results, measured
                                  slower, kept for the A/B; others: DESIGN.md §3, racc_hip_variant_available */
    uint32_t refill_min;       /* idle lanes that trigger a wave refill; 0 => default */
    uint32_t leaf_min;         /* leaf-holding lanes that trigger a leaf step; 0 => default */
    uint32_t chunk;            /* rays a wave dequeues per cursor atomic; 0 => default */
    uint32_t tail_active;      /* waves with <= this many live rays ("thin") run both step bodies per iteration;
                                  0 => default (32), > 64 => never */
    uint32_t regroup_period;   /* V3 kernels: scheduling iterations between workgroup-wide regroupings; 0 => default */
    uint32_t thin_reps;        /* V2 kernels: inner steps a thin wave runs per scheduling iteration; 0 => default (8) */
    uint32_t inner_reps;       /* V2 kernels: inner steps any other wave runs per scheduling iteration; 0 => default (3) */
    uint32_t coop_same_pct;    /* V7 kernels: inner steps fetch nodes quad-cooperatively through LDS-DMA while fewer than this
                                  percentage of the inner lanes hold the same node as their quad neighbour (divergent waves);
                                  0 => default (20), > 100 => never, 100 => always */
    uint32_t time_kernels;     /* != 0: an event pair around every traversal kernel (racc_hip_read_kernel_times); costs two
                                  hipEventRecord per launch, so off by default */
    uint32_t drain_prefetch;   /* what a thin wave (few live rays: a launch's drain, a small launch) does about the latency of its node
                                  fetches.  0 => default: nothing.  1: touch both children's records as soon as the child refs arrive
                                  (round 2: -3 % on a 64k-ray batch, +4..10 % on 256k..1M rays).  3: every step also requests the record
                                  BEHIND each lane's node — its likeliest next node in the device order, 46 % of the visits — into the
                                  lane's LDS-DMA slots, and a lane that goes on into that record reads it from LDS (round 5, built at
                                  the round-4 verdict's request; measured slower: 64k rays 0.130 vs 0.113-0.116 ms, 1M 0.345 vs 0.320 —
                                  a wave steps in lockstep, one lane's miss costs the whole step).  Same results in all forms */
    uint32_t leaf_step;        /* 0/1 => the leaf step runs inside the kernel's assembly block and takes the inner lanes' step along
                                  (one memory round trip for both); 2 => in C++ through the block's LEAF door; 3 => in the block,
                                  not fused (A/B; same results) */
    uint32_t wide_below;       /* launches of fewer rays than this use the 4-wide kernel (kernel_variant 45) instead of the
                                  context's kernel: a launch of <= ~200k rays is all dependent chain, and the wide tree halves
                                  it (27k-ray launch, the reference's stream size: 0.10 instead of 0.12 ms).  Results: see
                                  kernel_variant 45.  0 => never (default) */
    uint32_t chain_launches;   /* 0/1 => device-resident batches issued on the engine's own streams (racc_hip_intersect_device with
                                  stream = NULL) are chained: waves that run out of rays in one batch go on with the next one
                                  issued, so a sequence of batches runs like one long launch (no drain between them).  A batch's
                                  arrays belong to the engine until racc_hip_wait on its lane has returned and may be re-issued
                                  at once after that (the exact rule: racc_hip_intersect_device below).  2 => off: every launch
                                  stands alone, the lanes' launches merely overlap (same rule).  Round 5: the chain is LAZY — once
                                  a chain has its kernels (one per lane in rotation), a further batch is only published to them (a
                                  descriptor written by a one-thread kernel): no traversal kernel that would find nothing left, no
                                  miss-shading kernel (the chained kernels sample the probe image in their epilogue).  racc_hip_wait /
                                  racc_hip_synchronize establish completion — the chain's kernels have ended and every published
                                  batch's rays were handed out — and trace whatever the chain did not reach (it had ended before the
                                  batch was linked) with a catch-up kernel; hence results are defined, as before, when the wait
                                  returns.  A caller who waits for every batch gains nothing from a chain and would pay for its start and
                                  end (0.46 against 0.35 ms per 1M-ray batch): with the default threshold (chain_min_rays = 0), after
                                  two waits in a row that found a chain of one batch, a batch issued while nothing else of the
                                  context is in flight is launched stand-alone; the first batch issued while another is in flight
                                  starts a chain again (RACC_CHAIN_SOLO=0 switches that off).  3 => round 4's form: every chained
                                  launch brings its own kernel + miss-shading kernel */
    uint32_t chain_min_rays;   /* only batches of at least this many rays are chained; smaller ones are launched stand-alone on their
                                  lane (they overlap like any two lanes' launches).  A chained launch costs the host more stream
                                  operations, and a batch that is worked off before its successor is linked breaks the chain: 27,648-ray
                                  streams back to back run 126 Mrays/s chained, 657 stand-alone; the crossover is between 512k and 1M
                                  rays.  0 => default (786,432); 1 => chain every batch (tests) */
} racc_hip_options;

typedef struct racc_hip_scene_info {
    uint32_t node_count;       /* inner nodes */
    uint32_t pair_count;       /* pairs incl. padding */
    uint32_t remap_count;
    uint32_t inner_height;     /* levels of inner nodes on the longest root path */
    uint32_t max_leaf_pairs;
    uint32_t spill_levels;     /* stack levels beyond the LDS-resident ones */
    uint64_t device_bytes;
} racc_hip_scene_info;

/* Per-launch counters of the last racc_hip_intersect_device* call on a lane (debug/bench). */
typedef struct racc_hip_launch_info {
    uint32_t grid_blocks, block_threads;
    uint32_t lds_bytes_per_block;
    uint32_t waves_per_simd;
    float    last_kernel_ms;   /* hipEvent time of the traversal kernel alone */
} racc_hip_launch_info;

const char* racc_hip_last_error(void);             /* thread-local, never NULL */
const char* racc_hip_version(void);
/* The lanes a context has (options.lanes, or the default: 4; without chained launches 6 when the HIP runtime was given >= 8
 * hardware queues, GPU_MAX_HW_QUEUES) and how many of them RACC_HIP_LANE_AUTO rotates over (3; without chained launches 6 in
 * that case: kernels of two streams that share a hardware queue do not overlap; RACC_AUTO_LANES overrides).  A caller that rotates result buffers needs at least
 * `auto_lanes` of them.  Either pointer may be NULL. */
int racc_hip_lane_count(const racc_hip_ctx* ctx, uint32_t* lanes, uint32_t* auto_lanes);

/* 1 if racc_hip_options::kernel_variant = n selects a kernel of this build (0 = the default always does; the earlier
 * generations and ablations exist only in a `make EXPERIMENTAL=1` build), else 0.  Needs no GPU. */
int racc_hip_variant_available(uint32_t kernel_variant);

/* ≙ clGetDeviceIDs, RayAccelerator.cpp:467-478 (reference picks devices[0]). */
int racc_hip_device_count(int* count);

/* ≙ racc::createContext's OpenCL half: program build + queues, RayAccelerator.cpp:463-514,700-717.
 * Fails with RACC_HIP_ERR_NO_DEVICE if `device` is not a gfx950 GPU: there is no CPU fallback. */
int racc_hip_create(int device, const racc_hip_options* opts, racc_hip_ctx** out);
int racc_hip_destroy(racc_hip_ctx* ctx);           /* ≙ racc::destroy(Context*), RayAccelerator.cpp:761-788 */

/* ≙ the three clCreateBuffer(COPY_HOST_PTR) calls, Scene.cpp:342-346.  Inputs are the
 * reference-format blobs (copied; caller keeps ownership).  The blob is validated
 * (child indices, pair ranges, no cycles) and re-laid-out for the device. */
int racc_hip_scene_upload(racc_hip_ctx* ctx,
                          const void* nodes64, uint32_t node_count,
                          const void* pairs48, uint32_t pair_count,
                          const uint32_t* remap, uint32_t remap_count,
                          racc_hip_scene** out);
int racc_hip_scene_free(racc_hip_ctx* ctx, racc_hip_scene* scene);   /* ≙ Scene.cpp:362-369 */
int racc_hip_scene_get_info(const racc_hip_scene* scene, racc_hip_scene_info* info);

/* ≙ clCreateImage(RGBA, FLOAT), Environment.cpp:36-50.  rgba is width*height*4 floats, copied. */
int racc_hip_env_upload(racc_hip_ctx* ctx, const float* rgba, uint32_t width, uint32_t height, racc_hip_env** out);
int racc_hip_env_free(racc_hip_ctx* ctx, racc_hip_env* env);         /* ≙ Environment.cpp:63-64 */

/* ≙ clCreateBuffer(CL_MEM_USE_HOST_PTR) per ray stream, RayAccelerator.cpp:635-645: page-locks the
 * stream's host arrays so the copies below run at PCIe rate.  Optional. */
int racc_hip_register_stream(racc_hip_ctx* ctx, void* rays, void* results, uint32_t capacity);
int racc_hip_unregister_stream(racc_hip_ctx* ctx, void* rays, void* results);
/* Same for one block that holds many streams (the reference allocates all of them in one block,
 * RayAccelerator.cpp:547-568). */
int racc_hip_register_host(racc_hip_ctx* ctx, void* ptr, uint64_t bytes);
int racc_hip_unregister_host(racc_hip_ctx* ctx, void* ptr);

/* ≙ clSetKernelArg x7 + clEnqueueNDRangeKernel + clFinish on one submission thread's queue,
 * RayAccelerator.cpp:378-404.  Host Ray[count] in, host Result[count] out, in place and in order
 * (RayStream contract, RayAccelerator.h:78-83).  `lane` in [0, lanes): calls on distinct lanes may
 * run concurrently from different threads.  env may be NULL (miss rgb = 0).  Blocking. */
int racc_hip_intersect(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                       const void* rays, void* results, uint32_t count, uint32_t lane);
/* Same, split into enqueue and wait (≙ clEnqueueNDRangeKernel / clFinish).  The enqueue returns as soon as the batch's three stages
 * — rays in over PCIe, traversal, results out over PCIe — are queued; it blocks only while the SAME lane's previous host batch is
 * still in flight (a lane has one pair of staging arrays).  With page-locked arrays (racc_hip_register_*) the stages of batches
 * issued on different lanes overlap: all copies into the GPU go through one stream, back to back, all copies out through another,
 * the kernels run on the lanes' streams in between — a caller that rotates 3-4 lanes keeps the link busy in both directions
 * (≙ the reference's gpuSubmissionThreads queues, RayAccelerator.cpp:711-717; 1M-ray batches back to back: DESIGN.md §6).
 * The host arrays belong to the engine until racc_hip_wait on the lane (or RACC_HIP_LANE_AUTO: every lane) has returned. */
int racc_hip_intersect_async(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                             const void* rays, void* results, uint32_t count, uint32_t lane);
/* racc_hip_wait(lane): the lane's host batch is copied out / its device-resident launches have ended.  With chained launches (the default
 * for device-resident batches of >= chain_min_rays rays) a batch is complete when its chain is, whichever lane it was issued on: while a
 * chain has batches outstanding, a wait for ONE lane waits for every lane's kernels (a context-wide wait) and holds the chain's mutex
 * meanwhile — threads that each drive a lane of their own and wait often should create the context with chain_launches = 2. */
int racc_hip_wait(racc_hip_ctx* ctx, uint32_t lane);

/* MI355X-sized dispatch: a whole set of ray streams in ONE launch.  The reference launches once per
 * <=27k-ray stream (RayAccelerator.cpp:369-404); 27k rays occupy 5 % of the 524,288 lanes a MI355X keeps
 * resident and every launch pays the latency of its longest ray, so the scheduler (racc::render) hands over
 * everything that is ready.  rays[i]/results[i] are host arrays of counts[i] records; results land in place
 * and in order per stream.  Blocking.  When the arrays are page-locked (racc_hip_register_*) and the launch has
 * >= 512k rays it is cut into 256k-ray slices whose PCIe copies run beside the neighbouring slices' kernels. */
int racc_hip_intersect_streams(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                               uint32_t n_streams, const void* const* rays, void* const* results,
                               const uint32_t* counts, uint32_t lane);
/* The same without the wait (≙ racc_hip_intersect_async for a set of streams): the pointer arrays are read during the call, the
 * ray/result arrays belong to the engine until racc_hip_wait(ctx, lane). */
int racc_hip_intersect_streams_async(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                                     uint32_t n_streams, const void* const* rays, void* const* results,
                                     const uint32_t* counts, uint32_t lane);

/* Device-resident variant: d_rays/d_results are device pointers (e.g. torch tensors' data_ptr()).
 * `stream` is a hipStream_t passed as void* (NULL => the lane's own stream).  Asynchronous.
 * A lane owns one ray cursor and spill area, so its launches never overlap: a launch that goes to another stream than the
 * lane's previous one first waits (on the device) for that one.  Launches on DIFFERENT lanes do overlap — one's drain hides
 * under the next one's bulk — which is how the reference keeps its gpuSubmissionThreads queues busy
 * (RayAccelerator.cpp:711-717).  lane = RACC_HIP_LANE_AUTO rotates over the lanes, so a single-threaded caller that issues
 * batch after batch (stream = NULL) gets that overlap without managing lanes; racc_hip_wait(ctx, RACC_HIP_LANE_AUTO) or
 * racc_hip_synchronize then waits for all of them.  A launch of <= 2M rays issued while ANOTHER lane has a launch the host has not
 * waited for takes a thin grid (2 waves per SIMD instead of 5), so that up to three launches are co-resident; "in flight" is what the
 * caller has issued and not yet waited for — a property of the call sequence, not of the GPU's progress at that instant: wait for a
 * lane (racc_hip_wait) before issuing a launch that should have the machine to itself.
 * With stream = NULL the batch must be resident and final at the call, and — racc_hip_options::chain_launches, the default, for
 * batches of at least racc_hip_options::chain_min_rays rays (786,432) —
 * launches are CHAINED: waves of the launches issued before may start on this batch at once and carry on through it, so that
 * a sequence of batches runs like one long launch (20 batches of 1M rays back to back: 0.28 instead of 0.33 ms each).  A launch
 * on a caller's stream is never chained.
 *
 * Array reuse under chained launches — the exact rule (≙ the in-place, in-order ray-stream contract, RayAccelerator.h:78-83,
 * RayAccelerator.cpp:369-410: the reference recycles a stream's arrays bounce after bounce):
 *   - a batch's ray and result arrays belong to the engine from the call until racc_hip_wait on ITS lane (or
 *     RACC_HIP_LANE_AUTO / racc_hip_synchronize) has returned; a lane's wait returns when its batch is complete, whoever traced it;
 *   - after that wait the arrays may be rewritten and re-issued AT ONCE, by any means that has completed before the next call
 *     (racc_hip_memcpy_h2d, a copy or kernel on another stream that the caller has synchronised), while the batches of the
 *     other lanes are still in flight and their kernels go on to trace the re-issued one.
 * Why a kernel that outlives kernel boundaries reads the NEW contents: every batch is linked into the chain by a kernel that is
 * dispatched after the call (one thread, on the engine's control stream).  The acquire of that dispatch — ROCm gives every kernel
 * dispatch packet an agent-scope acquire fence — makes the command processor invalidate the vector L1 of every CU and the
 * non-coherent lines of every XCD's L2 BEFORE the kernel runs, i.e. before the link can become visible; no wave reads a batch's
 * rays before it has seen the link (a relaxed agent-scope load, served by the L2), and nothing writes the array in between.  The
 * ray records themselves are loaded with system-scope loads (sc0 sc1: they always miss the CU's L1), which takes the L1 out of the
 * argument altogether.  Results travel the other way through kernel ends: a batch is complete when its own kernel and every kernel
 * issued before it have ended (their end-of-kernel release writes the L2s back), which is what the lane's wait waits for.
 * tests/test_gpu_reuse.py recycles three ray and three result buffers through 2,000 chained batches of 64 ... 1M rays, rewritten
 * by host copies and by a copy kernel on another stream, on a scene that thrashes the L2s and on one that leaves them idle:
 * every batch bit-exact.
 * What this rests on: the dispatch-packet acquire is behaviour of the HIP runtime and the command processor, not of this library —
 * established on ROCm 7.2 (HIP 7.2.26015), gfx950 in SPX partition mode, and checked there by the test above, not derived from a
 * specification.  On any other runtime or partition mode the GUARANTEED rule is the stricter one: re-issue an array only after
 * racc_hip_synchronize (no kernel of the chain is alive then), or create the context with chain_launches = 2 (every launch stands
 * alone; a kernel never outlives the boundary that publishes its inputs). */
int racc_hip_intersect_device(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                              const void* d_rays, void* d_results, uint32_t count,
                              uint32_t lane, void* stream);
/* Runs the device variant `iters` times back to back on the lane's stream and writes each launch's
 * traversal-kernel duration in milliseconds (HIP events on that stream) to ms[iters]. Blocking. */
int racc_hip_intersect_device_timed(racc_hip_ctx* ctx, const racc_hip_scene* scene, const racc_hip_env* env,
                                    const void* d_rays, void* d_results, uint32_t count,
                                    uint32_t lane, uint32_t iters, float* ms);
/* ---- occlusion (any-hit) queries ----
 * ≙ nothing in the reference (its scheduler knows the closest hit only); Embree's rtcOccluded is the usual counterpart.  The shadow /
 * visibility ray: is anything in (minT, maxT]?  The answer is exactly "racc_hip_intersect* would report a hit for this ray" — the same
 * traversal rule with the ray's own maxT and the same pair test in the same arithmetic — but the traversal stops at the first accepted
 * triangle pair, keeps no hit state, gathers no remap entry, samples no environment (hence no `env` argument) and writes one byte
 * per ray instead of a 16-byte Result.  Rays the closest-hit path rejects (non-finite origin, direction or minT, NaN maxT) give 0.
 * Its own kernel (occludedKernel, rayaccel_amd/csrc/racc_occlusion.inc) on the BVH2 records every scene carries, whatever
 * kernel_variant the context was created with.  No lane, chain, group or RCCL involvement: a launch owns its scratch memory (one
 * cursor word + stack spill, allocated and freed in stream order around the kernel), so launches on different streams overlap each
 * other and the chained closest-hit batches of racc_hip_intersect_device, and racc_hip_destroy leaves nothing of them behind.
 *
 * occluded[i] = 1 if anything lies in (minT, maxT] of rays[i], else 0.  Device-resident, asynchronous on `stream`
 * (hipStream_t as void*, NULL = the default stream, as racc_hip_memcpy_d2d_async); complete after racc_hip_stream_synchronize,
 * which also reports a watchdog trip.  ctx is checked first, then scene; count == 0 is a successful no-op. */
int racc_hip_occluded_device(racc_hip_ctx*, const racc_hip_scene*, const void* d_rays, uint8_t* d_occluded, uint32_t count, void* stream);
/* Host arrays, blocking, callable from several threads at once (every call brings its own stream and staging arrays). */
int racc_hip_occluded(racc_hip_ctx*, const racc_hip_scene*, const void* rays, uint8_t* occluded, uint32_t count);

/* ---- dynamic scenes: refit of a device-resident scene to moved vertices ----
 * ≙ nothing in the reference (its scenes are frozen at createScene, Scene.cpp:216-349); Embree's rtcCommitScene on a deformable scene and
 * every GPU API's BVH update are the usual counterparts — and their bottom-level BUILD is "dynamic scenes: build and rebuild of a
 * scene's tree on the device" below, for a mesh that has left what a kept topology can bear.  The topology stays (child references, leaf ranges, remap, the device node order,
 * hence inner_height, max_leaf_pairs and every count in racc_hip_scene_info); the 48 B pair records and the child boxes of the 64 B node
 * records are recomputed by the rule of racc_host_blobs_refit (below, "host refit"), bit for bit.  A refitted tree traces the moved mesh
 * correctly; how well it traces it depends on how far the vertices moved from the positions the tree was built for.
 *
 * All refit state lives in the racc_hip_refit handle: the four vertex indices of every pair, every device record's parent, the list of
 * leaf references, one arrival counter per record (device memory), the blob's topology words (host memory, 16 B per inner node, kept
 * from racc_hip_scene_upload on) and the map from blob order to device order.  Destroy the handle before its scene.
 * Those topology words are the one cost refit puts on callers who never use it: racc_hip_scene_upload keeps them for every scene, in the
 * record it registers per scene (the device drops the blob's node order and its kind / parent words, so they cannot be recovered later);
 * RACC_REFIT_TOPOLOGY=0 in the environment switches that off, and racc_hip_refit_create then refuses.  The unpadded pair count is taken to be where the last leaf ends (as in
 * every blob the builder makes); records behind it are padding, rewritten as copies of pair 0.
 * racc_hip_refit_create: indices / index_count as the scene was built from, vertex_count = the length of every vertex array to come.
 * Validates like the host refit (remap's triangle ids < index_count / 3, every index < vertex_count).  RACC_HIP_ERR_INVALID, scene
 * untouched, when the scene carries a 4-wide, compressed or SoA copy of the tree — a context created with kernel_variant 45 or 50,
 * wide_below != 0 or the SoA variant: this entry does not refit those copies and a stale one would give wrong hits (racc_hip_refit_create_wide,
 * below, takes the 4-wide and compressed ones) — or is a device group's replica.
 *
 * Ordering contract: a refit rewrites arrays that traversal kernels read.
 *   racc_hip_scene_refit (host xyzw vertices, validated: finite) calls racc_hip_synchronize(ctx) first, so that no kernel of a chain is
 *   alive, then runs on a stream of the handle's own and has completed when it returns.
 *   racc_hip_scene_refit_device (device xyzw vertices, NOT validated: they must be finite) is asynchronous on `stream` (hipStream_t as
 *   void*, NULL = the default stream).  Before the call the caller guarantees that every batch and occlusion launch issued on this scene
 *   has been waited for; afterwards the caller calls racc_hip_stream_synchronize on that stream before the next launch on the scene.
 * racc_hip_refit_download: the scene's current records back in reference format and blob order (what racc_hip_scene_upload was given,
 * boxes and pair records as the last completed refit left them); either pointer may be NULL; capacities in records (node_count /
 * padded pair_count of racc_hip_scene_info).  The caller has waited for the refit. */
typedef struct racc_hip_refit racc_hip_refit;
int racc_hip_refit_create(racc_hip_ctx*, racc_hip_scene*, const uint32_t* indices, uint32_t index_count, uint32_t vertex_count, racc_hip_refit** out);
int racc_hip_refit_destroy(racc_hip_ctx*, racc_hip_refit*);
int racc_hip_scene_refit(racc_hip_ctx*, racc_hip_refit*, const float* vertices, uint32_t vertex_count);
int racc_hip_scene_refit_device(racc_hip_ctx*, racc_hip_refit*, const void* d_vertices, uint32_t vertex_count, void* stream);
int racc_hip_refit_download(racc_hip_ctx*, racc_hip_refit*, void* nodes64_out, uint32_t node_capacity, void* pairs48_out, uint32_t pair_capacity);

/* ---- dynamic scenes: refit of the 4-wide and compressed copies (fast mode) ----
 * racc_hip_refit_create_wide is racc_hip_refit_create for a scene that carries a 4-wide and / or a compressed copy of the tree — a
 * context created with kernel_variant 45-53 or wide_below != 0.  The handle is an ordinary racc_hip_refit: racc_hip_scene_refit,
 * racc_hip_scene_refit_device, racc_hip_refit_download and racc_hip_refit_destroy work on it with the ordering contract above, and
 * every refit also rewrites whichever wide copies the scene has, by the rule of racc_host_scene_wide_nodes_refit (below, "host wide
 * refit"), bit for bit: the collapse stays as the upload made it, every plane follows the refitted binary boxes.  Quality degrades with
 * motion as the binary tree's does — and in one more way: which four boxes share a record was decided by the areas at upload.
 * RACC_HIP_ERR_INVALID, scene untouched: an SoA copy, a device group's replica, a scene without topology words or without any wide
 * copy, a scene that already has a wide handle (at most one per scene; racc_hip_refit_create refuses these scenes as before), or wide
 * references on the device that are not what the collapse of the device's binary records gives (the handle replays it at creation).
 * Device memory on top of the plain handle's: 16 B per wide record.
 * A compressed frame that cannot hold its boxes — a plane that is not finite, an extent that overflows binary32 — is DISABLED by the
 * refit: references kept, every slot written as an unused one, origin +inf, so that every plane decodes to +inf and rays miss the
 * subtree below it.  racc_hip_refit_check returns how many frames the last refit disabled (0 on a plain handle); the caller has
 * synchronised first.  The blocking racc_hip_scene_refit never gets there: on a handle whose scene has a compressed copy it returns
 * RACC_HIP_ERR_LIMIT, scene untouched, when max - min of all vertices on an axis is not finite in binary32.
 * racc_hip_refit_download_wide: the device's current records of `format` (45: 128 B, 50: 64 B; as racc_host_scene_wide_nodes lays
 * them out); RACC_HIP_ERR_INVALID when the scene has no copy of that format; out may be NULL (then only *count); capacity in records. */
int racc_hip_refit_create_wide(racc_hip_ctx*, racc_hip_scene*, const uint32_t* indices, uint32_t index_count, uint32_t vertex_count, racc_hip_refit** out);
int racc_hip_refit_download_wide(racc_hip_ctx*, racc_hip_refit*, int format, void* out, uint32_t capacity, uint32_t* count);
int racc_hip_refit_check(racc_hip_ctx*, racc_hip_refit*, uint32_t* disabled_frames);

/* ---- dynamic scenes: build and rebuild of a scene's tree on the device, in stream order ----
 * ≙ nothing in the reference; every GPU API's bottom-level build is the usual counterpart.  What racc_host_scene_build plus
 * racc_hip_scene_upload do on the host — a new tree for a mesh that deformed beyond what a refit's kept topology can bear, or for
 * vertices that come from a kernel — without leaving the stream: an LBVH over the triangles (Morton codes of the triangle box centres, a
 * radix sort, Karras's 2012 hierarchy), one triangle per pair and one pair per leaf, written into the scene's existing allocations in the
 * formats every kernel reads.  The rule is stated once, in rayaccel_amd/csrc/racc_scene_rebuild_rule.h; racc_host_scene_rebuild (below,
 * "host scene rebuild") is its specification, and after a device rebuild racc_hip_refit_download plus the scene's remap are that
 * function's nodes, pairs and remap byte for byte.  "Refit per frame, rebuild every N frames" — both on one handle and one stream.
 * Such a tree is expected to trace well below racc_host_scene_build's SAH tree (lone triangles, no line-paired record order, no
 * surface-area heuristic): DESIGN.md §3 has the measured ratio, which is what tells a caller how often a host build is worth its price.
 *
 * racc_hip_scene_rebuild_create (blocking): runs racc_host_scene_rebuild on the given xyzw vertices (its refusals, under its name),
 * uploads the blobs through racc_hip_scene_upload — which does all allocation — makes a refit handle with the rebuild's scratch, and
 * runs one device rebuild, so that the scene is in the rebuild's own layout from then on: device record = node index, the upload's
 * padding records unreferenced behind the T - 1 nodes.  Device memory beyond a plain handle's: 12 B per triangle of indices, 24 B per
 * triangle of keys and values (formed, sorted), 16 B per vertex of staging, 32 B of words (centre bounds, height) and rocPRIM's temporary
 * storage, sized at creation.  The handle is an ordinary racc_hip_refit: racc_hip_scene_refit, racc_hip_scene_refit_device,
 * racc_hip_refit_download (nodes in node order: the identity map), racc_hip_refit_check and racc_hip_refit_destroy work on it, and
 * racc_hip_scene_get_info reports max_leaf_pairs = 1.  It is the scene's ONLY handle: the scene's registry record is flagged and its
 * topology words are dropped, and racc_hip_refit_create / racc_hip_refit_create_wide refuse the scene from then on — a device rebuild
 * changes the topology, the words a plain handle keeps would go stale and it would write wrong boxes.  Destroy the handle before the
 * scene: racc_hip_scene_free returns RACC_HIP_ERR_INVALID while it lives.
 * RACC_HIP_ERR_INVALID, nothing created: a context whose uploads carry a 4-wide, compressed or SoA copy of the tree or put the top of
 * the tree first (kernel_variant 45-53, wide_below != 0, the SoA variant, 60-63) — a rebuild rewrites the binary records only, the copies
 * and the cached top would go stale.
 * racc_hip_scene_rebuild_device: device xyzw vertices, NOT validated — they must be finite; with vertices that are not the results are
 * unspecified, but every access of the rebuild stays inside its arrays (the rule header says why) — asynchronous on `stream`, with the
 * ordering contract of racc_hip_scene_refit_device.  RACC_HIP_ERR_INVALID before anything is enqueued: a handle racc_hip_refit_create*
 * made, a vertex_count that differs from the handle's.
 * racc_hip_scene_rebuild: host vertices, validated by the host rule (finite); calls racc_hip_synchronize(ctx) as racc_hip_scene_refit
 * does, runs on the handle's stream and has completed on return.
 * racc_hip_scene_rebuild_check: the height (levels of nodes on the longest root path) of the tree the scene holds now; the caller has
 * synchronised the stream first.
 *   Stack room: the host cannot know the height of a tree built on the device without leaving the stream.  So
 * racc_hip_scene_rebuild_device raises the scene's info.inner_height (and info.spill_levels) to the rule's bound before it enqueues
 * anything — 63 + ceil(log2 T) levels, at most T - 1 (the rule header derives it) — and every launch sizes its spill from
 * info.inner_height: a launch issued behind a device rebuild always has stack room.  The price of the bound: up to 87 levels against the
 * default kernel's 12 in LDS is up to 75 spilled levels x 4 B x 524,288 grid threads = 157 MB of spill area per lane, allocated at the
 * first launch that needs it and kept.  racc_hip_scene_rebuild (blocking) and racc_hip_scene_rebuild_check set info.inner_height to the
 * real height, and the next launch sizes its spill from that.  (info is read by launches and written by these entries: the ordering
 * contract covers it.)
 *   Worlds: racc_hip_world_create reads its scenes' inner_height once.  A world created after racc_hip_scene_rebuild_check or the
 * blocking rebuild has stack room for the tree the scene holds THEN (create it anew after a rebuild that makes the tree taller); a world
 * created between racc_hip_scene_rebuild_device and the check reads the bound and has room for every rebuild to come, at the bound's
 * price.
 * racc_hip_refit_download_remap: the scene's remap as the device holds it now (remap_count of racc_hip_scene_info words; any refit handle —
 * only a rebuild changes it); the caller has waited for the rebuild.  With racc_hip_refit_download: the whole scene back as blobs.
 * Out of scope: pairing of triangles that share an edge (every pair is a lone triangle), the 128-byte line order of the records, SAH or
 * treelet optimisation of the LBVH, the 4-wide and compressed formats, device groups, the racc:: C++ interface, changing the triangle
 * count on a live handle. */
int racc_hip_scene_rebuild_create(racc_hip_ctx*, const float* vertices, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                                  racc_hip_scene** scene_out, racc_hip_refit** out);
int racc_hip_scene_rebuild_device(racc_hip_ctx*, racc_hip_refit*, const void* d_vertices, uint32_t vertex_count, void* stream);
int racc_hip_scene_rebuild(racc_hip_ctx*, racc_hip_refit*, const float* vertices, uint32_t vertex_count);
int racc_hip_scene_rebuild_check(racc_hip_ctx*, racc_hip_refit*, uint32_t* height);
int racc_hip_refit_download_remap(racc_hip_ctx*, racc_hip_refit*, uint32_t* remap_out, uint32_t remap_capacity);

/* ---- instancing: two-level scenes with per-instance transforms ----
 * ≙ nothing in the reference (one flattened scene per racc::Scene, Scene.cpp:216-349); Embree's RTC_GEOMETRY_TYPE_INSTANCE and the
 * top-level / bottom-level structures of every GPU ray-tracing API are the usual counterparts.  Uploaded scenes are the bottom level; a
 * WORLD is an ordered list of `count` instances, each a 3x4 row-major object-to-world transform (twelve floats, rows of {a0 a1 a2 b}) and a
 * racc_hip_scene of the same context; several instances may name one scene.  Rigid motion costs racc_hip_world_refit_device (below: the
 * top level refitted on the device) or racc_hip_world_update (the top level rebuilt on the host) — no rebuild of a scene, the
 * bottom-level tree keeps its quality; a thousand copies of a mesh cost one scene plus 148 bytes each.
 *
 * Semantics.  inv = the inverse transform evaluated in double precision, every coefficient rounded to float once (racc_host_world_prepare
 * returns it).  Instance i sees the ray o' = inv (o, 1), d' = inv (d, 0), each component the plain float expression
 * ((m0 x + m1 y) + m2 z) + m3 (d': without m3), left to right, nothing fused, with the ray's own minT and maxT; the direction is not
 * normalised, so t means the same in both spaces.  Its result h_i is exactly what racc_hip_intersect* reports for that ray on that scene
 * (the oracle's traversal bit for bit: the reference's visiting order inside the bottom level, hence its tie behaviour).  The world result
 * is the h_i of smallest t, exact ties to the lowest instance index: Result = its triangle, t, u, v unchanged (triangle ids are the
 * scene's own), plus one uint32 instance index per ray.  A miss is triangle = 0xFFFFFFFF, t = u = v = 0, instance = 0xFFFFFFFF: there is no
 * environment argument.  Rays the closest-hit path rejects (non-finite origin, direction or minT, NaN maxT — in world space or after the
 * transform) miss.  Instances are culled by the best t so far against conservative world-space boxes (rayaccel_amd/csrc/world_build.cpp
 * has the bound); an instance's traversal always starts with the ray's own maxT, as defined.
 * Its own kernel (worldIntersectKernel, rayaccel_amd/csrc/racc_world.inc) on the BVH2 records every scene carries, whatever kernel_variant
 * the context was created with.  No lane, chain, group or RCCL involvement: a launch owns its scratch memory, allocated and freed in stream
 * order around the kernel, so launches overlap each other and chained closest-hit batches, and racc_hip_destroy leaves nothing behind.
 *
 * Ownership: a world BORROWS its scenes — destroy the world before freeing any of them.  racc_hip_world_create refuses (RACC_HIP_ERR_INVALID)
 * a scene that was not uploaded through racc_hip_scene_upload on `ctx` (another context's, a device group's replica), count == 0,
 * count > RACC_HIP_WORLD_MAX_INSTANCES and whatever racc_host_world_prepare refuses.
 * racc_hip_world_update: new transforms for the same scenes, `count` = the world's.  Also the call to make after a member scene was
 * refitted (racc_hip_scene_refit*): it re-reads the scenes' root boxes.  Blocking; calls racc_hip_synchronize first, as racc_hip_scene_refit
 * does.  A refused transform leaves the world as it was.
 * racc_hip_world_intersect_device: device-resident Ray[count] in, Result[count] and uint32[count] out, asynchronous on `stream`
 * (hipStream_t as void*, NULL = the default stream); complete after racc_hip_stream_synchronize, which also reports a watchdog trip.
 * ctx is checked first, then world; count == 0 is a successful no-op.
 * racc_hip_world_intersect: host arrays, blocking, callable from several threads at once (every call brings its own stream and staging).
 *
 * Occlusion (any-hit) on a world — the shadow / visibility ray of a caller who uses instancing, as racc_hip_occluded* is for a scene.
 * occluded[i] = 1 iff some instance's closest-hit result h_i, as defined above, is a hit; equivalently, iff racc_hip_world_intersect*
 * reports instance != 0xFFFFFFFF for rays[i].  That holds for every ray: there is no exception class.  Inside an instance the rule is that
 * of racc_hip_occluded*: the transformed ray with the ray's own minT / maxT, the limit never shrunk, the pair test up to its
 * accept / reject decision, stop at the first accepted pair.  Rays the closest-hit path rejects give 0 — in world space, or after every
 * transform; a rejected transformed ray only skips that instance.  The order in which instances are visited is free; the top level is
 * walked with the ray's own maxT (widened as the closest-hit kernel widens its limit), which is never less than the closest-hit kernel's
 * limit, so every instance that could report a hit is entered unless the ray is already decided.  One byte per ray: no Result, no instance
 * index, no remap gather.  Its own kernel (worldOccludedKernel, rayaccel_amd/csrc/racc_world_occlusion.inc), a launch owning its scratch
 * memory like the closest-hit world launch.
 * racc_hip_world_occluded_device: device-resident Ray[count] in, uint8[count] out, asynchronous on `stream`; complete after
 * racc_hip_stream_synchronize, which also reports a watchdog trip.  ctx is checked first, then world, then that the world is this
 * context's; count == 0 is a successful no-op; NULL arrays are refused.  The ordering contract with racc_hip_world_update is that of
 * racc_hip_world_intersect_device (the update synchronises the context first).
 * racc_hip_world_occluded: host arrays, blocking, callable from several threads at once (every call brings its own stream and staging).
 * Out of scope for the occlusion query: reporting which instance occluded, instance or ray masks, device groups, the 4-wide formats,
 * multi-level instancing, wiring into the path tracers or racc::render.
 *
 * Out of scope: environment sampling on a miss, racc::render carrying instance ids (its Result has no room),
 * device groups, the 4-wide kernels, multi-level instancing (an instance of a world). */
#define RACC_HIP_WORLD_MAX_INSTANCES (1u << 20)
typedef struct racc_hip_world racc_hip_world;
typedef struct racc_hip_world_info {
    uint32_t instance_count;
    uint32_t node_count;           /* top-level inner nodes */
    uint32_t height;               /* levels of top-level inner nodes on the longest root path */
    uint32_t lds_levels;           /* top-level stack levels the kernel keeps in LDS */
    uint32_t spill_levels;         /* top-level stack levels beyond those (global memory) */
    uint32_t bottom_spill_levels;  /* bottom-level stack levels beyond the kernel's LDS-resident ones, over all member scenes */
    uint64_t device_bytes;         /* top-level nodes, instance order, inverse transforms, instance table — not the scenes */
} racc_hip_world_info;
int racc_hip_world_create(racc_hip_ctx*, const float* transforms12, const racc_hip_scene* const* scenes, uint32_t count, racc_hip_world** out);
int racc_hip_world_update(racc_hip_ctx*, racc_hip_world*, const float* transforms12, uint32_t count);
int racc_hip_world_destroy(racc_hip_ctx*, racc_hip_world*);
int racc_hip_world_get_info(const racc_hip_world*, racc_hip_world_info* info);
int racc_hip_world_intersect_device(racc_hip_ctx*, const racc_hip_world*, const void* d_rays, void* d_results, uint32_t* d_instances, uint32_t count, void* stream);
int racc_hip_world_intersect(racc_hip_ctx*, const racc_hip_world*, const void* rays, void* results, uint32_t* instances, uint32_t count);
int racc_hip_world_occluded_device(racc_hip_ctx*, const racc_hip_world*, const void* d_rays, uint8_t* d_occluded, uint32_t count, void* stream);
int racc_hip_world_occluded(racc_hip_ctx*, const racc_hip_world*, const void* rays, uint8_t* occluded, uint32_t count);

/* ---- instancing: refit of a world's top level to moved instances, on the device ----
 * ≙ nothing in the reference; Embree's rtcCommitScene on a scene of moved instances and every GPU API's top-level update are the usual
 * counterparts.  What racc_hip_scene_refit* is for a scene: asynchronous, device-resident, for transforms a kernel of the caller's
 * produces (a physics step, a particle system).  The top level's topology stays (child references, `order`, hence node_count, height and
 * spill_levels of racc_hip_world_info); the per-instance inverse transforms, the child boxes of the top-level records and ray_pad are
 * recomputed by the rule of racc_host_world_refit (below, "host world refit"), bit for bit.  A refitted world traces the moved instances
 * correctly — every result is what a world created with the new transforms reports; how FAST it traces them depends on how far the
 * instances moved from where the top level was built: its quality degrades (boxes of one subtree grow and overlap; instances that swap
 * places are the worst case).  racc_hip_world_rebuild_device (next section) rebuilds the top level on the same stream, racc_hip_world_update
 * on the host — "refit per frame, rebuild every N frames".
 *
 * All refit state lives in the racc_hip_world_refit handle (device memory: 8 B per instance plus 36 B): per `order` position the slot
 * (2 * device record + side) its box goes to, every top-level record's own slot in its parent, one arrival counter per record, a 64-bit
 * word for the largest condition number, a counter of disabled instances and the 4-byte word the world kernels read ray_pad from while
 * the handle lives.  The world's own allocations and racc_hip_world_info::device_bytes do not change.  At most one handle per world (a
 * second racc_hip_world_refit_create is RACC_HIP_ERR_INVALID); destroy the handle before its world (racc_hip_world_destroy refuses a
 * world that still has one).  racc_hip_world_update on a world with a live handle works as before and ends by rebuilding the handle's
 * tables from the new topology.
 *
 * racc_hip_world_refit_device: `count` (= the world's) device-resident 3x4 transforms, 16-byte aligned, asynchronous on `stream`
 * (hipStream_t as void*, NULL = the default stream).  The member scenes' root boxes are read from their device records, so a member
 * scene that was refitted (racc_hip_scene_refit*) is picked up with no host step.  The transforms are NOT validated on the host.  An
 * instance whose transform or boxes racc_host_world_prepare would refuse — a coefficient that is not finite, a determinant that is zero
 * or not finite in double, a coefficient of the inverse or of the world box that is not finite in float — is DISABLED: its inv becomes
 * twelve NaNs (every transformed ray is rejected, so it is never reported), its world box {+inf, +inf, +inf, -inf, -inf, -inf}, it does
 * not enter ray_pad and it is counted; the topology is never written, whatever the input.  racc_hip_world_refit_check returns the count
 * of the last refit; the caller has synchronised the stream first.
 * Ordering contract: before the call the caller guarantees that every launch on this world (and every refit of a member scene) issued
 * on ANOTHER stream has been waited for.  Launches issued afterwards on the SAME stream need nothing; on other streams they need
 * racc_hip_stream_synchronize on the refit's stream first.
 * racc_hip_world_refit: host transforms, validated with the host rule (whatever racc_host_world_prepare refuses is refused, and the
 * world is left as it was); calls racc_hip_synchronize(ctx), copies, runs on a stream of the handle's own and has completed on return.
 * racc_hip_world_download (any world, with or without a handle): inv [count][12], the top-level records converted back to the 64-byte
 * blob layout (node_capacity in records, at least node_count of racc_hip_world_info; kind and parent are written as 0 and are
 * unspecified: the device does not hold them), order [count] and the current ray_pad.  Any output pointer may be NULL.  Blocking; the
 * caller has waited for whatever writes the world.
 * Out of scope: device groups, the racc:: C++ interface, instance masks.  (The rebuild of the top level on the device is the next section.) */
struct racc_hip_world_refit;      /* the handle; no typedef, because racc_hip_world_refit is also the name of the blocking entry: write `struct racc_hip_world_refit*` */
int racc_hip_world_refit_create(racc_hip_ctx*, racc_hip_world*, struct racc_hip_world_refit** out);
int racc_hip_world_refit_destroy(racc_hip_ctx*, struct racc_hip_world_refit*);
int racc_hip_world_refit_device(racc_hip_ctx*, struct racc_hip_world_refit*, const void* d_transforms12, uint32_t count, void* stream);
int racc_hip_world_refit(racc_hip_ctx*, struct racc_hip_world_refit*, const float* transforms12, uint32_t count);
int racc_hip_world_refit_check(racc_hip_ctx*, struct racc_hip_world_refit*, uint32_t* disabled_instances);
int racc_hip_world_download(racc_hip_ctx*, const racc_hip_world*, float* inv12_out, void* nodes64_out, uint32_t node_capacity,
                            uint32_t* order_out, float* ray_pad_out);

/* ---- instancing: rebuild of a world's top level on the device, in stream order ----
 * ≙ nothing in the reference; every GPU API's top-level build is the usual counterpart.  What racc_hip_world_update does on the host —
 * a new top-level tree for instances that changed neighbourhoods, where a refit's kept topology traces slowly — without leaving the
 * stream: an LBVH (Morton codes of the instance box centres, a radix sort, Karras's 2012 hierarchy) written into the world's existing
 * allocations.  The rule is stated once, in rayaccel_amd/csrc/racc_world_rebuild_rule.h; racc_host_world_rebuild (below, "host world
 * rebuild") is its specification, and after a device rebuild racc_hip_world_download returns that function's inv, nodes (first, last, the
 * four boxes), order and ray_pad byte for byte.  A rebuilt world answers every ray exactly as racc_hip_world_create with the same
 * transforms does: the world contract (smallest t, ties to the lowest instance index) does not depend on the topology.  "Refit per frame,
 * rebuild every N frames" — both on one handle and one stream.
 *
 * racc_hip_world_rebuild_create: racc_hip_world_refit_create plus the rebuild's scratch.  The handle is an ordinary world refit handle:
 * every racc_hip_world_refit* entry works on it, it is the world's one handle, racc_hip_world_refit_destroy destroys it.  Device memory,
 * beyond the plain handle's 8 B per instance plus 36 B: 32 B per instance (a 16-byte centre record and two 8-byte keys, formed and
 * sorted) plus 32 B of words (centre bounds, height) plus the radix sort's temporary storage, sized at creation by rocPRIM for `count`
 * 64-bit keys (another buffer of keys and its histograms: about 8 B per instance).
 *   Stack room: the host cannot know the height of a tree built on the device without leaving the stream.  So at creation, and for as
 * long as the handle lives, the world's info.height and info.spill_levels are raised to the rule's bound — 31 + ceil(log2(count)) levels,
 * at most count - 1 (racc_world_rebuild_rule.h derives it) — keeping at least their current value: a launch issued after a device rebuild
 * always has stack room.  racc_hip_world_update on such a world keeps the raised values.  racc_hip_world_refit_destroy, which
 * synchronises the device, reads the real height back and sets info.height / spill_levels from it.
 * racc_hip_world_rebuild_device: the arguments, alignment, ordering contract and disable rule of racc_hip_world_refit_device — `count`
 * (= the world's) device-resident 3x4 transforms, 16-byte aligned, asynchronous on `stream`, not validated on the host; the member
 * scenes' root boxes are read from their device records.  An instance the host rule would refuse is DISABLED as a refit disables it (NaN
 * inv, neutral box, not in ray_pad, counted); it sorts behind every enabled instance and remains a leaf of the tree.
 * RACC_HIP_ERR_INVALID on a handle racc_hip_world_refit_create made, before anything is enqueued.
 * racc_hip_world_rebuild: host transforms, validated with the host rule (whatever racc_host_world_prepare refuses is refused, and the
 * world is left as it was); calls racc_hip_synchronize(ctx), copies, runs on the handle's own stream and has completed on return.
 * racc_hip_world_rebuild_check: the height (levels of top-level records on the longest root path) of the tree the world holds now and
 * the disabled instances of the last refit or rebuild; the caller has synchronised the stream first.
 * Out of scope: treelet or SAH optimisation of the LBVH, device groups, the racc:: C++ interface, instance masks, multi-level
 * instancing, the 4-wide formats. */
int racc_hip_world_rebuild_create(racc_hip_ctx*, racc_hip_world*, struct racc_hip_world_refit** out);
int racc_hip_world_rebuild_device(racc_hip_ctx*, struct racc_hip_world_refit*, const void* d_transforms12, uint32_t count, void* stream);
int racc_hip_world_rebuild(racc_hip_ctx*, struct racc_hip_world_refit*, const float* transforms12, uint32_t count);
int racc_hip_world_rebuild_check(racc_hip_ctx*, struct racc_hip_world_refit*, uint32_t* height, uint32_t* disabled_instances);

int racc_hip_get_launch_info(racc_hip_ctx* ctx, uint32_t lane, racc_hip_launch_info* info);
/* With racc_hip_options::time_kernels: durations (ms, HIP events on the stream each launch went to) of the lane's traversal
 * kernels since the last call, oldest first, at most `capacity` (the engine keeps the last 256); *n = how many.  Waits for them. */
int racc_hip_read_kernel_times(racc_hip_ctx* ctx, uint32_t lane, float* ms, uint32_t capacity, uint32_t* n);
/* Scheduling statistics accumulated by the statistics build of the default kernel (kernel_variant 42) on a lane:
 * [0] inner steps (wave-level) [1] lanes live in them [2] leaf steps [3] lanes live in them
 * [4] refill iterations [5] rays loaded [6] cursor dequeues [7] waves; shader-clock cycles summed over waves:
 * [8],[10] unused by variant 42 [12] refill iterations [13] wave lifetime;
 * [14] inner steps in which ALL live inner lanes hold the same node (what a wave-uniform scalar step could serve)
 * [15] inner steps fetched quad-cooperatively.  stats16 has 16 entries.  Waits for the lane. */
int racc_hip_read_stats(racc_hip_ctx* ctx, uint32_t lane, uint64_t* stats16, int reset);

/* Device memory helpers for hosts that do not bring their own allocator. */
int racc_hip_malloc(racc_hip_ctx* ctx, uint64_t bytes, void** d_ptr);
int racc_hip_free(racc_hip_ctx* ctx, void* d_ptr);
int racc_hip_memcpy_h2d(racc_hip_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);
int racc_hip_memcpy_d2h(racc_hip_ctx* ctx, void* dst, const void* d_src, uint64_t bytes);
/* Device-to-device copy on `stream` (a hipStream_t as void*, e.g. from racc_hip_stream_create; NULL = the default stream): the
 * runtime's copy kernel.  For hosts that stage ray batches in HBM and hand the engine a rotating set of arrays. */
int racc_hip_memcpy_d2d_async(racc_hip_ctx* ctx, void* d_dst, const void* d_src, uint64_t bytes, void* stream);
int racc_hip_synchronize(racc_hip_ctx* ctx);
/* HIP streams for hosts that do not bring their own (passed back as the `stream` of racc_hip_intersect_device). */
int racc_hip_stream_create(racc_hip_ctx* ctx, void** stream);
int racc_hip_stream_synchronize(racc_hip_ctx* ctx, void* stream);      /* also reports a watchdog trip */
int racc_hip_stream_destroy(racc_hip_ctx* ctx, void* stream);

/* ---- multi-GPU: device groups ----------------------------------------------------------------------
 * ≙ nothing in the reference (its cl_context drives devices[0], RayAccelerator.cpp:467-478).  A group is one engine context per
 * entry of `devices` (entries may repeat an ordinal: rehearsal on one GPU); the scene and the environment are replicated on
 * every member (read-only data, Scene.cpp:342-346); racc_hip_group_intersect cuts a host batch into contiguous shards of whole
 * 64-ray chunks, traces them concurrently (one persistent host thread and one PCIe link per GPU) and lands the results in place, in order.
 * No exchange between GPUs.  racc_hip_group_ctx gives the members for everything else (lanes, device-resident batches). */
typedef struct racc_hip_group racc_hip_group;
typedef struct racc_hip_group_scene racc_hip_group_scene;
typedef struct racc_hip_group_env racc_hip_group_env;
int racc_hip_group_create(const int* devices, uint32_t n, const racc_hip_options* opts, racc_hip_group** out);
int racc_hip_group_destroy(racc_hip_group* group);
uint32_t racc_hip_group_size(const racc_hip_group* group);
racc_hip_ctx* racc_hip_group_ctx(racc_hip_group* group, uint32_t i);
int racc_hip_group_scene_upload(racc_hip_group* group, const void* nodes64, uint32_t node_count, const void* pairs48, uint32_t pair_count,
                                const uint32_t* remap, uint32_t remap_count, racc_hip_group_scene** out);
int racc_hip_group_scene_free(racc_hip_group* group, racc_hip_group_scene* scene);
int racc_hip_group_env_upload(racc_hip_group* group, const float* rgba, uint32_t width, uint32_t height, racc_hip_group_env** out);
int racc_hip_group_env_free(racc_hip_group* group, racc_hip_group_env* env);
int racc_hip_group_intersect(racc_hip_group* group, const racc_hip_group_scene* scene, const racc_hip_group_env* env,
                             const void* rays, void* results, uint32_t count);
/* Device-resident counterpart (≙ racc_hip_intersect_device per member): d_rays[i] / d_results[i] are device pointers on member i's
 * GPU holding that member's shard of counts[i] rays (racc_hip_malloc on racc_hip_group_ctx(group, i), or the host's own allocator);
 * a member with counts[i] == 0 sits the call out.  Asynchronous: the call hands every shard to its member's worker thread, which
 * issues it on the member's own streams — lanes rotated, launches chained, exactly as racc_hip_intersect_device(lane =
 * RACC_HIP_LANE_AUTO, stream = NULL) — so a caller that issues batch after batch keeps all GPUs full without a host thread of its
 * own per GPU.  The arrays belong to the engine until racc_hip_group_wait returns; it waits for everything issued on every
 * member and reports the first failure (a watchdog trip included).  No exchange between the members; a GPU-side consumer that
 * needs every hit everywhere gathers afterwards (racc_hip_allgather_results, one communicator rank per member). */
int racc_hip_group_intersect_device(racc_hip_group* group, const racc_hip_group_scene* scene, const racc_hip_group_env* env,
                                    const void* const* d_rays, void* const* d_results, const uint32_t* counts);
int racc_hip_group_wait(racc_hip_group* group);

/* ---- multi-GPU: hit-record exchange over RCCL/xGMI ------------------------------------------------
 * The path shards without any exchange: rays never interact, the scene is read-only (Scene.cpp:342-346), so every GPU
 * traces its contiguous shard of a batch (one process per GPU, or one racc::Context over several GPUs).  Only a GPU-side
 * consumer that needs EVERY hit on EVERY GPU needs the step below: one ncclAllGather of the 16-byte Result records, a
 * single message per rank.  librccl is bound at run time (dlopen); these entries fail with RACC_HIP_ERR_DEVICE if it is
 * absent.  No counterpart in the reference (it drives one device, RayAccelerator.cpp:467-478).
 *   rank 0: racc_hip_comm_unique_id(&id); the host program ships the 128 bytes to the other ranks (MPI, torch.distributed,
 *   a file); every rank: racc_hip_comm_init_rank(ctx, &id, rank, nranks, &comm);
 *   per batch: racc_hip_allgather_results(comm, d_shard, d_all, rays_per_rank, stream)  — every rank contributes
 *   rays_per_rank records (pad the last shard); d_all holds nranks * rays_per_rank records, rank r's at r * rays_per_rank;
 *   in place if d_shard == d_all + rank * rays_per_rank.  Asynchronous on `stream` (hipStream_t as void*, NULL = default). */
typedef struct racc_hip_comm racc_hip_comm;
typedef struct racc_hip_comm_id { char bytes[128]; } racc_hip_comm_id;      /* = ncclUniqueId */
int racc_hip_comm_unique_id(racc_hip_comm_id* id);
int racc_hip_comm_init_rank(racc_hip_ctx* ctx, const racc_hip_comm_id* id, int rank, int nranks, racc_hip_comm** out);
int racc_hip_allgather_results(racc_hip_comm* comm, const void* d_send, void* d_recv, uint32_t count_per_rank, void* stream);
int racc_hip_comm_destroy(racc_hip_comm* comm);

/* ---- host-side scene build (no GPU needed) ---------------------------------------------------
 * ≙ the GPU branch of racc::createScene, Scene.cpp:216-339: createBvh2 (Bvh2.cpp:772-907) →
 * leaf pair merge (Scene.cpp:237-261) → 64 B node flatten (Scene.cpp:275-332) → pair padding
 * (Scene.cpp:334-338).  vertices: xyzw floats, 16-byte aligned (Scene.cpp:187); index_count % 3 == 0
 * (Scene.cpp:186).  Deterministic (the reference's node numbering is thread-timing dependent).
 * = racc_host_scene_build_ex with options NULL: the library default, RACC_HOST_BUILD_DEFAULT_QUALITY — the quality-1 tree (below; the
 * same reference-format blobs with fewer node visits per ray; it is the tree bench.py's headline figure is measured on, so a drop-in caller
 * of racc::createScene gets what is benchmarked) — unless the environment variable RACC_BUILD_QUALITY (0, 1, 2) says otherwise; 0 there, or
 * racc_host_build_options.quality = 0, gives the reference's own builder (Bvh2.cpp:257-535), byte-identical to the oracle's restatement. */
#define RACC_HOST_BUILD_DEFAULT_QUALITY 1u
int racc_host_scene_build(const float* vertices, uint32_t vertex_count,
                          const uint32_t* indices, uint32_t index_count,
                          racc_host_scene** out);
/* The same with options.  quality 0 = the reference's builder.  quality 1 (= racc_host_scene_build) / 2 (no
 * counterpart in the reference): the finished tree is post-processed — every leaf cut down to ONE triangle pair (the reference
 * leaves up to six in a leaf, and every pair of a visited leaf is tested, Kernels.h:200-205), then subtrees re-inserted where they
 * enlarge the boxes above them least (Bittner et al. 2013; parallel over fixed subtrees, so still deterministic for any thread
 * count).  The blobs stay in the reference's format (Scene.cpp:73-87) and the reference's traversal order applies unchanged: the
 * oracle and the reference's own OpenCL kernel consume them as they are; only the number of node visits and pair tests per ray
 * drops (battlefield-synth, first-bounce rays: 51.1 -> 43.9 visits, 3.44 -> 2.43 pair tests at quality 1).  Since round 6 the tree is
 * built over REFERENCES to triangles: a triangle whose box is much larger than itself gets several, each with the box of the part of it
 * between two median planes of the scene's box (spatial splits, Karras & Aila 2013; split_percent below), and then sits in several leaves,
 * its pair record written once per leaf — remap[] names a triangle more than once, pair_count grows by up to the budget.  Hit records of a
 * quality tree equal those of the quality-0 tree up to how a triangle happens to be paired (t/u/v within rounding, primId up to
 * exact-distance ties and rays that graze an edge).  threads 0 = RACC_BUILD_THREADS, else the CPUs this process may use. */
typedef struct racc_host_build_options {
    uint32_t struct_size;      /* sizeof(racc_host_build_options): fields a caller's older header lacks read as 0 */
    uint32_t quality;          /* 0, 1, 2 */
    uint32_t threads;
    uint32_t split_percent;    /* quality >= 1: spatial splits, the budget of extra triangle references as a percentage of the triangle count;
                                  0 = the library chooses: RACC_HOST_BUILD_DEFAULT_SPLIT_PERCENT, or three times that where the SAH estimate of the
                                  tree as built drops by more than 7 % with it (scenes of unconnected, overlapping triangles); RACC_BUILD_SPLIT_PERCENT
                                  overrides; RACC_HOST_BUILD_NO_SPLITS = none */
    uint32_t reserved[4];
} racc_host_build_options;
#define RACC_HOST_BUILD_DEFAULT_SPLIT_PERCENT 10u
#define RACC_HOST_BUILD_NO_SPLITS 0xFFFFFFFFu
int racc_host_scene_build_ex(const float* vertices, uint32_t vertex_count,
                             const uint32_t* indices, uint32_t index_count,
                             const racc_host_build_options* options,      /* NULL = all defaults */
                             racc_host_scene** out);
int racc_host_scene_free(racc_host_scene* scene);
/* Borrowed pointers into the build product, valid until racc_host_scene_free. */
int racc_host_scene_blobs(const racc_host_scene* scene,
                          const void** nodes64, uint32_t* node_count,
                          const void** pairs48, uint32_t* pair_count_padded, uint32_t* pair_count,
                          const uint32_t** remap, uint32_t* remap_count);
/* The intermediate BVH2 (Bvh2.h:15-29): 48 B nodes + permuted triangle ids. */
int racc_host_scene_bvh2(const racc_host_scene* scene,
                         const void** nodes48, uint32_t* node_count,
                         const uint32_t** triangles, uint32_t* triangle_count);

/* Host refit: reference-format blobs in, the same blobs for moved vertices out (pure function: no GPU, no scene handle; outputs may alias
 * inputs).  kind, parent, first, last and remap are unchanged.  The rule — the specification racc_hip_scene_refit reproduces bit for bit:
 *   pair record  remap[2p] = t0 | ea << 30, remap[2p+1] = t1 | (eb+1) << 30 or 0 for a lone triangle (then p3 = p1); with a / b the index
 *                triples of t0 / t1 the pair's vertices are a[ea], a[(ea+1)%3], a[(ea+2)%3], b[(eb+2)%3]; the record is e1 = p0 - p1,
 *                e2 = p2 - p0, e3 = p3 - p0, p0 (Scene.cpp:149-153); records [pair_count, pair_count_padded) are copies of the new pair 0
 *   select       min = b < acc ? b : acc, max = b > acc ? b : acc per component (not fmin / fmax: -0.0 against +0.0)
 *   leaf box     the select folded over the leaf's pairs first .. first+cnt-1, each pair's vertices in order p0 p1 p2 p3, from p0 of the first
 *   inner box    the node's first-child box (accumulator) with its last-child box, by the same select
 * Refitting a tree the builder made to the vertices it was built from reproduces it byte for byte unless it has spatial splits (the library
 * default): there a split reference's clipped box becomes its whole pair's box (every refit box contains the built one).
 * RACC_HIP_ERR_INVALID before any output byte is written: a blob racc_hip_scene_upload would refuse, a triangle id in remap[0, 2 * pair_count)
 * >= index_count / 3, an index >= vertex_count, a vertex coordinate (x, y, z) that is not finite. */
int racc_host_blobs_refit(const void* nodes64, uint32_t node_count,
                          const void* pairs48, uint32_t pair_count_padded, uint32_t pair_count,
                          const uint32_t* remap, uint32_t remap_count,
                          const float* vertices /* xyzw */, uint32_t vertex_count,
                          const uint32_t* indices, uint32_t index_count,
                          void* nodes64_out, void* pairs48_out);

/* Host scene rebuild: the specification of racc_hip_scene_rebuild* (pure function: no GPU, no handle) — an LBVH over the triangles of a
 * mesh in the reference's blob formats, by the rule of rayaccel_amd/csrc/racc_scene_rebuild_rule.h.  T = index_count / 3.
 *   triangle box  the select of racc_host_blobs_refit folded over the triangle's three vertices in index order, from the first one
 *   centre     per axis float(0.5 * min + 0.5 * max) of that box, evaluated in double
 *   field      per axis floor(2^21 (c - lo) / (hi - lo)) in double, at most 2^21 - 1, 0 where hi > lo does not hold (lo / hi = the smallest
 *              / largest centre); the three 21-bit values interleaved into 63 bits, x highest
 *   key        the pair (field, triangle index), ordered lexicographically — unique; order[p] = the triangle of the p-th smallest key
 *   pairs48_out  pair p is triangle order[p] alone: vertices a[0], a[1], a[2], a[1], the record as racc_host_blobs_refit packs it;
 *              *pair_count_padded = the smallest multiple of 32 above T, the padding copies of pair 0
 *   remap_out  remap[2p] = order[p], remap[2p + 1] = 0; *remap_count = 2T
 *   nodes64_out  node 0 the root over the positions [0, T - 1]; a node over [a, b] splits behind the last position that has a 0 in the
 *              highest bit in which key[a] and key[b] differ (of the 95-bit concatenation); first child = the lower range; a child of one
 *              position p is the leaf p | 1 << 24, a wider first child is node `split`, a wider last child node `split + 1`
 *              (0x80000000 | node); kind = 1, parent = the parent's index (0xFFFFFFFF for the root); *node_count = T - 1.  Boxes: exactly
 *              racc_host_blobs_refit's fold over this topology, so refitting the output to its own vertices reproduces it, signs of
 *              zeros included.
 *   height     levels of nodes on the longest root path: at most 63 + ceil(log2 T) and at most T - 1.
 * Deterministic.  Before any output byte is written: RACC_HIP_ERR_INVALID for a NULL pointer, index_count % 3 != 0, T < 2, an index >=
 * vertex_count, a vertex coordinate (x, y, z) that is not finite, node_capacity < T - 1, pair_capacity < the padded pair count,
 * remap_capacity < 2T; RACC_HIP_ERR_LIMIT for T >= 2^24. */
int racc_host_scene_rebuild(const float* vertices /* xyzw */, uint32_t vertex_count, const uint32_t* indices, uint32_t index_count,
                            void* nodes64_out, uint32_t node_capacity, uint32_t* node_count,
                            void* pairs48_out, uint32_t pair_capacity, uint32_t* pair_count_padded,
                            uint32_t* remap_out, uint32_t remap_capacity, uint32_t* remap_count, uint32_t* height);

/* Host side of instancing (racc_hip_world_* above; pure function, no GPU, no handle) — ≙ nothing in the reference.  Inputs: `count`
 * 3x4 row-major object-to-world transforms and each instance's object-space root box {min[3], max[3]} (the union of the two child boxes
 * of its scene's root node).  Outputs, all caller-allocated and written only when the call succeeds:
 *   inv12_out         [count][12]  the inverse transforms: evaluated in double (adjugate over determinant, translation -(A^-1 b)), each
 *                                  coefficient rounded to float once — part of the specification of racc_hip_world_intersect*
 *   world_boxes6_out  [count][6]   one conservative world-space box {min[3], max[3]} per instance: contains the eight transformed corners
 *                                  of the root box, plus the instance's share of the margin that makes culling against it lossless
 *   ray_pad_out       the ray's share of that margin: the kernel widens every box by *ray_pad_out * (|ox| + |oy| + |oz|) on every side
 *   nodes64_out       top-level BVH2 over those boxes in the scenes' 64-byte node format (Scene.cpp:73-78), node 0 the root,
 *                     max(count - 1, 1) nodes (node_capacity must be at least that; *node_count_out says how many were written); a leaf
 *                     reference first | cnt << 24 names the instances order_out[first .. first + cnt) — here always one; a world of one
 *                     instance has the empty reference 0 as its root's last child
 *   order_out         [count]      a permutation of the instance indices
 *   height_out        levels of inner nodes on the longest root path
 * Deterministic (median splits of the box centres, ties by instance index).  RACC_HIP_ERR_INVALID: a NULL pointer, count == 0,
 * count > RACC_HIP_WORLD_MAX_INSTANCES, a coefficient or box coordinate that is not finite, a box with min > max, a singular transform (its
 * double-precision determinant is zero or not finite, or a coefficient of the inverse or of a world box is not finite in float). */
int racc_host_world_prepare(const float* transforms12, const float* root_boxes6, uint32_t count,
                            float* inv12_out, float* world_boxes6_out, float* ray_pad_out,
                            void* nodes64_out, uint32_t node_capacity, uint32_t* node_count_out,
                            uint32_t* order_out, uint32_t* height_out);

/* Host world refit: a top-level tree in, the same tree for moved instances out (pure function: no GPU, no handle; outputs may alias
 * inputs) — the specification racc_hip_world_refit* reproduces bit for bit.  nodes64 / order as racc_host_world_prepare or
 * racc_hip_world_download deliver them, node_count = max(count - 1, 1).
 *   inv12_out, world_boxes6_out, *ray_pad_out   exactly what racc_host_world_prepare computes for these transforms and root boxes (one
 *                function serves both entries)
 *   nodes64_out  kind, parent, first and last are copied.  A leaf child's box is the world box of order[first] (cnt is always 1); an empty
 *                reference's box (cnt 0, the one-instance world's last child) is copied from the input; an inner child's box is that child
 *                node's first-child box (accumulator) with its last-child box by the select of racc_host_blobs_refit:
 *                min = b < acc ? b : acc, max = b > acc ? b : acc per component (not fmin / fmax)
 * Refitting a tree racc_host_world_prepare made to the transforms it was made for reproduces it except possibly the sign of a zero
 * plane: prepare folds a child's box over the instances below it in `order`, this folds it over the tree, and the select keeps whichever
 * of -0.0 and +0.0 it meets first.
 * RACC_HIP_ERR_INVALID before any output byte is written: whatever racc_host_world_prepare refuses (a NULL pointer, count == 0,
 * count > RACC_HIP_WORLD_MAX_INSTANCES, an input that is not finite, a box with min > max, a singular transform), and a malformed
 * topology: node_count != max(count - 1, 1), a child index >= node_count, a node reached twice or never, a leaf with cnt > 1, a leaf
 * position >= count (or named twice, or never), `order` not a permutation of [0, count). */
int racc_host_world_refit(const float* transforms12, const float* root_boxes6, uint32_t count,
                          const void* nodes64, uint32_t node_count, const uint32_t* order,
                          float* inv12_out, float* world_boxes6_out, float* ray_pad_out, void* nodes64_out);

/* Host world rebuild: the specification of racc_hip_world_rebuild* (pure function: no GPU, no handle).  The arguments and refusals of
 * racc_host_world_prepare, whose inv12_out, world_boxes6_out and *ray_pad_out it reproduces as bytes; the tree is the LBVH of
 * rayaccel_amd/csrc/racc_world_rebuild_rule.h instead of the median split:
 *   centre     per axis float(0.5 * min + 0.5 * max) of the world box, evaluated in double
 *   field      per axis floor(1024 (c - lo) / (hi - lo)) in double, at most 1023, 0 where hi == lo (lo / hi = the smallest / largest
 *              centre); the three 10-bit values interleaved into 30 bits, x highest
 *   key        (uint64(field) << 32) | instance index — unique; order_out[p] = the low word of the p-th smallest key
 *   nodes64_out  node 0 the root over the positions [0, count - 1]; a node over [a, b] splits behind the last position that has a 0 in
 *              the highest bit in which key[a] and key[b] differ; first child = the lower range; a child of one position p is the leaf
 *              p | 1 << 24, a wider first child is node `split`, a wider last child node `split + 1` (0x80000000 | node); kind = 1,
 *              parent = the parent's index (0xFFFFFFFF for the root); max(count - 1, 1) nodes, a world of one instance as
 *              racc_host_world_prepare makes it.  Boxes: exactly racc_host_world_refit's fold over this topology, so refitting the
 *              output to its own transforms reproduces it, signs of zeros included.
 *   height_out   levels of nodes on the longest root path: at most 30 + ceil(log2(count)) and at most count - 1 (a node's split bit is
 *              below its parent's; 30 field bits and ceil(log2(count)) index bits can differ).
 * Deterministic.  RACC_HIP_ERR_INVALID before any output byte is written, as racc_host_world_prepare; the message names this entry. */
int racc_host_world_rebuild(const float* transforms12, const float* root_boxes6, uint32_t count,
                            float* inv12_out, float* world_boxes6_out, float* ray_pad_out,
                            void* nodes64_out, uint32_t node_capacity, uint32_t* node_count_out,
                            uint32_t* order_out, uint32_t* height_out);

/* The device layout racc_hip_scene_upload gives the node blob (for tools and tests; needs no GPU).  Device record, 64 B: words 0-1 =
 * the two child references (re-numbered), words 2-3 unused, then the child boxes as six (min, max) plane pairs: Lx Ly Lz Rx Ry Rz.
 * order 1 (the default of racc_hip_scene_upload): every 128-byte line holds a node and, behind it, its inner child with the larger
 * box — a ray that goes on into that child finds its record in the line it has just fetched — lines in depth-first order; nodes whose
 * children are both leaves share lines pairwise; all-zero padding records (no reference points at them) fill the rest, so *count may
 * exceed node_count.  order 0: the 4096 nodes with the largest boxes first, the rest in the blob's order (round 1-3 layout).
 * order > 1 (what a context created with kernel_variant 60-63 uploads): the `order` nodes with the largest own boxes first — a
 * connected top of the tree, the records those kernels keep in LDS — and the subtrees below them in order 1's line pairs.
 * out64 may be NULL (then only *count is returned); capacity in records. */
int racc_host_scene_device_nodes(const void* nodes64, uint32_t node_count, uint32_t pair_count, uint32_t remap_count, int order,
                                 void* out64, uint32_t capacity, uint32_t* count);

/* The 4-wide device records racc_hip_scene_upload builds for the wide kernels (for tools and tests; needs no GPU): the very collapse and
 * quantisation that upload runs, with the same refusals.
 *   format 45  the 128 B record of kernel_variant 45-49: words 0-3 the four child references (inner ones re-numbered breadth first),
 *              words 4-27 the planes lo.x hi.x lo.y hi.y lo.z hi.z, four children each — every used box bit-equal to a box of the blob —,
 *              word 28 the number of used slots (slots [0, used); host-side bookkeeping, no kernel reads it), words 29-31 zero.  An unused
 *              slot holds six planes at +inf and the reference of a real leaf.
 *   format 50  the 64 B compressed record of kernel_variant 50-53: words 0-3 the references, 4-6 the frame's origin, 7-9 its scale
 *              (x, y, z), 10-15 one byte per child for lo.x hi.x lo.y hi.y lo.z hi.z; a plane decodes as fmaf(float(byte), scale, origin)
 *              and the decoded box contains the blob's.  An unused slot holds lower bytes 255, upper bytes 0 and the reference of a real
 *              leaf.  RACC_HIP_ERR_INVALID: a child box that is not finite; RACC_HIP_ERR_LIMIT: a frame whose extent overflows binary32.
 * *stack_bound = the number of stack entries a traversal of these records can need at most (what upload sizes the spill area by).
 * out may be NULL (then only *count and *stack_bound are returned); capacity in records. */
int racc_host_scene_wide_nodes(const void* nodes64, uint32_t node_count, uint32_t pair_count, uint32_t remap_count, int format,
                               void* out, uint32_t capacity, uint32_t* count, uint32_t* stack_bound);

/* Host wide refit: the 4-wide records of a refitted scene (pure function: no GPU) — the specification racc_hip_scene_refit* reproduces
 * bit for bit on a handle of racc_hip_refit_create_wide.
 *   nodes64_built  the blob the scene was uploaded from.  It alone decides the collapse: which binary child box every slot copies, the
 *                  slot order, the breadth-first numbering, `used` and the leaf reference in unused slots — racc_host_scene_wide_nodes'
 *                  collapse of that blob, kept as the binary refit keeps its topology.  The wide tree's quality therefore degrades
 *                  with motion like the binary tree's, and the grouping of boxes into records no longer follows their areas.
 *   nodes64_now    the same topology with refitted boxes, as racc_host_blobs_refit delivers them.  It supplies every plane.
 *   format 45      a used slot's six planes are its source child's box in nodes64_now, lower / upper ordered per axis; references, `used`
 *                  and unused slots as built.  Holds any box; never disables.
 *   format 50      the frame of those planes, stated by its result:
 *                    org    per axis the fold of the used lower planes in slot order, `p < acc ? p : acc` from +inf on (of +0.0 and
 *                           -0.0 the one met first stays);
 *                    scale  the correctly rounded binary32 (hi - lo) / 255 with hi the like fold of the upper planes, FLT_MIN if that
 *                           quotient is not positive, then raised by nextafter until fmaf(255, scale, org) >= hi;
 *                    a lower byte is the largest a in [0, 255] with fmaf(a, scale, org) <= plane, an upper byte the smallest b with
 *                    fmaf(b, scale, org) >= plane; unused slots get 255 / 0.
 *                  A frame with a used plane that is not finite, or whose org or scale is not finite on an axis, is DISABLED and
 *                  counted in *disabled_frames: references kept, all four slots 255 / 0, org +inf and scale FLT_MIN on every axis
 *                  (every plane decodes to +inf, format 45's convention for a slot that is never entered: rays miss the subtree).
 * With nodes64_now == nodes64_built the records equal racc_host_scene_wide_nodes' byte for byte.  RACC_HIP_ERR_INVALID: a NULL pointer,
 * another format, a blob racc_hip_scene_upload refuses, blobs that differ in a child reference.  out may be NULL (then only *count is
 * returned; *disabled_frames is 0); capacity in records. */
int racc_host_scene_wide_nodes_refit(const void* nodes64_built, const void* nodes64_now, uint32_t node_count, uint32_t pair_count, uint32_t remap_count,
                                     int format, void* out, uint32_t capacity, uint32_t* count, uint32_t* disabled_frames);

#ifdef __cplusplus
}
#endif
#endif
