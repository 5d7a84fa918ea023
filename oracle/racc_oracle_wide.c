/*
 * racc_oracle_wide.c — exact CPU model of the engine's 4-wide device formats and of their traversal.
 *
 * TEST INFRASTRUCTURE ONLY — never linked into or loaded by the product.  Built into libracc_oracle.so as ONE translation
 * unit with racc_oracle.c (included below): ray admission, the epsilon clamp, the pair test, the order of the pairs within
 * a leaf, the epilogue and the miss radiance are that file's own functions, called here and not restated.  The analysis
 * program oracle/wide_sim.c includes this file and keeps no copy of its own.
 *
 * What is restated, from the statement of the rule in the product's plain C++ (rayaccel_amd/csrc/racc_scene_format.inc:
 * collapseWide, quantiseWide; racc_kernel_v9.inc / racc_kernel_v10.inc: the wideStep lambdas):
 *   collapse    the two children of a BVH2 node are the first candidates; the inner candidate with the largest surface area
 *               (DOUBLE arithmetic, first among equals) is replaced in place by its own two children until there are four
 *               or only leaves are left; nodes numbered breadth first; an unused slot holds six planes at +inf and the ref
 *               of a real leaf; stack bound = 3 * height + 1.
 *   quantise    frame = box around the used children, scale = extent / 255 raised until fmaf(255, scale, origin) reaches
 *               the upper corner; a lower plane takes the largest byte whose decoded value does not exceed it, an upper
 *               plane the smallest byte whose decoded value is not below it; unused slots: lower 255, upper 0.
 *   traverse    reads the DEVICE RECORDS as bytes.  Format 45: the planes.  Format 50: fmaf(float(byte), scale, origin) —
 *               one rounding.  The sign of the (clamped) direction picks the entry and the exit plane; a distance is
 *               fma(plane, 1/d, -o/d); entry = maxNum(tNear, x, y, z), exit = minNum(tFar, x, y, z) (the hardware's
 *               v_max_f32 / v_min_f32: a NaN operand is ignored); key = entry > exit ? tFar : entry, and key == tFar is
 *               "missed"; the nearest hit child — strict <, so the lowest slot among equals — is visited next, the other
 *               hit children are pushed in slot order (the highest slot is popped first).  A slot is NEVER skipped by its
 *               ref: an unused slot is kept out by its planes alone, exactly as on the device.
 * Each lane of the kernels owns its node and its stack, so the sequence of box and pair tests of a ray does not depend on
 * scheduling: this model is exact, record for record (tests/test_gpu_wide_exact.py).
 *
 * The sign of a zero cannot steer anything here: keys are only compared (<, >, !=), never examined bitwise.
 */
#include "racc_oracle.c"

typedef struct { uint32_t ref[4]; float plane[6][4]; uint32_t used; uint32_t pad[3]; } orc_wide_node;      /* 128 B: planes lo.x hi.x lo.y hi.y lo.z hi.z, four children each */
typedef struct { uint32_t ref[4]; float org[3]; float scl[3]; uint32_t q[6]; } orc_wide_node_q;             /* 64 B: q = lo.x hi.x lo.y hi.y lo.z hi.z, byte i = child i */
_Static_assert(sizeof(orc_wide_node) == 128 && sizeof(orc_wide_node_q) == 64, "device record sizes");

typedef struct { uint32_t ref; float mn[3], mx[3]; } wide_cand;

static double wide_area(const wide_cand* c) {
    const double x = (double)c->mx[0] - c->mn[0], y = (double)c->mx[1] - c->mn[1], z = (double)c->mx[2] - c->mn[2];
    return x * y + x * z + y * z;
}

/* out: room for nodeCount records (a wide node absorbs at least one BVH2 node).  Returns the number of wide nodes. */
uint32_t orc_collapse_wide(const orc_gpu_node* nodes, uint32_t nodeCount, orc_wide_node* out, uint32_t* stackBound) {
    uint32_t* map = (uint32_t*)malloc(sizeof(uint32_t) * nodeCount);       /* BVH2 index -> wide index */
    uint32_t* queue = (uint32_t*)malloc(sizeof(uint32_t) * nodeCount);     /* breadth-first queue of BVH2 indices; position = wide index */
    uint32_t* depth = (uint32_t*)malloc(sizeof(uint32_t) * nodeCount);
    memset(map, 0xFF, sizeof(uint32_t) * nodeCount);
    uint32_t qt = 0, height = 0;
    queue[qt] = 0; depth[qt] = 1; map[0] = 0; ++qt;
    const uint32_t firstLeaf = (nodes[0].first & 0x80000000u) ? 0x01000000u : nodes[0].first;      /* a real leaf: pair 0 always exists */
    for (uint32_t qh = 0; qh < qt; ++qh) {
        const orc_gpu_node* n = nodes + queue[qh];
        if (depth[qh] > height) height = depth[qh];
        wide_cand c[4]; int k = 2;
        c[0].ref = n->first; memcpy(c[0].mn, n->leftMin, 12); memcpy(c[0].mx, n->leftMax, 12);
        c[1].ref = n->last;  memcpy(c[1].mn, n->rightMin, 12); memcpy(c[1].mx, n->rightMax, 12);
        while (k < 4) {
            int best = -1; double bestA = -1.0;
            for (int i = 0; i < k; ++i)
                if ((c[i].ref & 0x80000000u) && wide_area(&c[i]) > bestA) { bestA = wide_area(&c[i]); best = i; }
            if (best < 0) break;
            const orc_gpu_node* m = nodes + (c[best].ref & 0x7FFFFFFFu);
            for (int i = k; i > best + 1; --i) c[i] = c[i - 1];
            c[best].ref = m->first; memcpy(c[best].mn, m->leftMin, 12); memcpy(c[best].mx, m->leftMax, 12);
            c[best + 1].ref = m->last; memcpy(c[best + 1].mn, m->rightMin, 12); memcpy(c[best + 1].mx, m->rightMax, 12);
            ++k;
        }
        orc_wide_node* w = out + qh;
        memset(w, 0, sizeof(*w));
        for (int i = 0; i < 4; ++i) {
            if (i < k) {
                uint32_t r = c[i].ref;
                if (r & 0x80000000u) {
                    const uint32_t t = r & 0x7FFFFFFFu;
                    map[t] = qt; queue[qt] = t; depth[qt] = depth[qh] + 1; ++qt;
                    r = 0x80000000u | map[t];
                }
                w->ref[i] = r;
                for (int a = 0; a < 3; ++a) {      /* an inverted box acts as its mirror image in the reference's slab test (min/max of the two distances) */
                    w->plane[2 * a][i] = c[i].mn[a] < c[i].mx[a] ? c[i].mn[a] : c[i].mx[a];
                    w->plane[2 * a + 1][i] = c[i].mn[a] < c[i].mx[a] ? c[i].mx[a] : c[i].mn[a];
                }
            } else {
                w->ref[i] = firstLeaf;
                for (int p = 0; p < 6; ++p) w->plane[p][i] = INFINITY;
            }
        }
        w->used = (uint32_t)k;
    }
    if (stackBound) *stackBound = 3u * height + 1u;      /* at most three entries per level of the path */
    free(map); free(queue); free(depth);
    return qt;
}

/* The kernel's decode: ONE rounding. */
static inline float wide_decode(uint32_t byte, float scale, float origin) { return fmaf((float)byte, scale, origin); }

/* Returns 0, -1 (a used child box is not finite) or -4 (a frame's extent overflows binary32, or a box cannot be held). */
int orc_quantise_wide(const orc_wide_node* in, uint32_t count, orc_wide_node_q* out) {
    for (uint32_t n = 0; n < count; ++n) {
        const orc_wide_node* w = in + n;
        orc_wide_node_q r;
        memset(&r, 0, sizeof(r));
        memcpy(r.ref, w->ref, sizeof(r.ref));
        for (uint32_t i = 0; i < 4 && i < w->used; ++i)
            for (int p = 0; p < 6; ++p)
                if (!isfinite(w->plane[p][i])) return -1;
        for (int a = 0; a < 3; ++a) {
            float lo = INFINITY, hi = -INFINITY;
            for (uint32_t i = 0; i < 4 && i < w->used; ++i) { lo = fminf(lo, w->plane[2 * a][i]); hi = fmaxf(hi, w->plane[2 * a + 1][i]); }
            float scale = (hi - lo) / 255.0f;
            if (!(scale > 0.0f)) scale = 1.17549435e-38f;
            while (wide_decode(255u, scale, lo) < hi) scale = nextafterf(scale, INFINITY);
            if (!isfinite(scale) || !isfinite(lo)) return -4;
            r.org[a] = lo; r.scl[a] = scale;
            uint32_t qlo = 0, qhi = 0;
            for (uint32_t i = 0; i < 4; ++i) {
                int ql = 255, qh = 0;      /* unused slot: inverted */
                if (i < w->used) {
                    const float pl = w->plane[2 * a][i], ph = w->plane[2 * a + 1][i];
                    ql = (int)floorf((pl - lo) / scale); qh = (int)ceilf((ph - lo) / scale);
                    ql = ql < 0 ? 0 : ql > 255 ? 255 : ql; qh = qh < 0 ? 0 : qh > 255 ? 255 : qh;
                    while (ql > 0 && wide_decode((uint32_t)ql, scale, lo) > pl) --ql;
                    while (ql < 255 && wide_decode((uint32_t)(ql + 1), scale, lo) <= pl) ++ql;
                    while (qh < 255 && wide_decode((uint32_t)qh, scale, lo) < ph) ++qh;
                    while (qh > 0 && wide_decode((uint32_t)(qh - 1), scale, lo) >= ph) --qh;
                    if (wide_decode((uint32_t)ql, scale, lo) > pl || wide_decode((uint32_t)qh, scale, lo) < ph) return -4;
                }
                qlo |= (uint32_t)ql << (8 * i); qhi |= (uint32_t)qh << (8 * i);
            }
            r.q[2 * a] = qlo; r.q[2 * a + 1] = qhi;
        }
        out[n] = r;
    }
    return 0;
}

/* The 24 planes the traversal below tests a ray against in a record, as it decodes them: planes[count][6][4]. */
void orc_decode_wide(const void* records, int format, uint32_t count, float* planes) {
    for (uint32_t n = 0; n < count; ++n)
        for (int p = 0; p < 6; ++p)
            for (int i = 0; i < 4; ++i) {
                float v;
                if (format == 50) {
                    const orc_wide_node_q* q = (const orc_wide_node_q*)records + n;
                    v = wide_decode((q->q[p] >> (8 * i)) & 255u, q->scl[p >> 1], q->org[p >> 1]);
                } else v = ((const orc_wide_node*)records + n)->plane[p][i];
                planes[((size_t)n * 6 + (size_t)p) * 4 + (size_t)i] = v;
            }
}

/* v_max_f32 / v_min_f32 (IEEE maxNum / minNum): a NaN operand is ignored */
static inline float wmax(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
static inline float wmin(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }

typedef struct { unsigned long long nv, np, slots[5], depthHist[64], deepVisits[64]; } orc_wide_stats;

enum { ORC_WIDE_ORDER_PRODUCT = 0, ORC_WIDE_ORDER_HIGHEST_AMONG_EQUALS = 1, ORC_WIDE_ORDER_REVERSED_PUSH = 2 };

/* One ray.  `order` is for tests only: 0 = the product's rule; 1 = the HIGHEST slot among equal keys is visited next; 2 = the other
 * hit children are pushed in REVERSED slot order — what the kernels would compute if the rule changed. */
static void traverse_wide_one(const void* records, int format, const orc_pair* pairs, const uint32_t* remap,
                              const float* env, uint32_t envW, uint32_t envH, const orc_ray* in, orc_result* out,
                              int order, uint32_t* depthOut, orc_wide_stats* st) {
    ray_state ray;
    float invDir[3], OoD[3];
    if (depthOut) *depthOut = 0;
    if (!ray_admit(in, &ray, invDir, OoD)) { out->triangle = 0xFFFFFFFFu; out->t = out->u = out->v = 0.0f; return; }
    hit_state hit = { -1, ray.tFar, 0.0f, 0.0f };
    uint32_t node = 0x80000000u, stack[1024], head = 0, maxDepth = 0;
    for (;;) {
        if (node & 0x80000000u) {
            const uint32_t index = node & 0x7FFFFFFFu;
            uint32_t ref[4];
            float nearP[3][4], farP[3][4];      /* entry and exit plane per axis and child: the direction's sign picks */
            if (format == 50) {
                const orc_wide_node_q* q = (const orc_wide_node_q*)records + index;
                memcpy(ref, q->ref, sizeof(ref));
                for (int a = 0; a < 3; ++a) {
                    const int neg = ray.d[a] < 0.0f;
                    const uint32_t qn = neg ? q->q[2 * a + 1] : q->q[2 * a], qf = neg ? q->q[2 * a] : q->q[2 * a + 1];
                    for (int i = 0; i < 4; ++i) {
                        nearP[a][i] = wide_decode((qn >> (8 * i)) & 255u, q->scl[a], q->org[a]);
                        farP[a][i] = wide_decode((qf >> (8 * i)) & 255u, q->scl[a], q->org[a]);
                    }
                }
            } else {
                const orc_wide_node* w = (const orc_wide_node*)records + index;
                memcpy(ref, w->ref, sizeof(ref));
                for (int a = 0; a < 3; ++a) {
                    const int neg = ray.d[a] < 0.0f;
                    for (int i = 0; i < 4; ++i) { nearP[a][i] = w->plane[2 * a + neg][i]; farP[a][i] = w->plane[2 * a + 1 - neg][i]; }
                }
            }
            if (st) { ++st->nv; ++st->deepVisits[head < 63 ? head : 63]; }
            const float tRay = ray.tFar;
            float k[4];
            for (int i = 0; i < 4; ++i) {
                const float nx = fmaf(nearP[0][i], invDir[0], OoD[0]), fx = fmaf(farP[0][i], invDir[0], OoD[0]);
                const float ny = fmaf(nearP[1][i], invDir[1], OoD[1]), fy = fmaf(farP[1][i], invDir[1], OoD[1]);
                const float nz = fmaf(nearP[2][i], invDir[2], OoD[2]), fz = fmaf(farP[2][i], invDir[2], OoD[2]);
                const float n = wmax(wmax(ray.tNear, nx), wmax(ny, nz)), f = wmin(wmin(tRay, fx), wmin(fy, fz));
                k[i] = n > f ? tRay : n;      /* tFar doubles as "missed" (Kernels.h:131-134, 192-194) */
            }
            /* the nearest hit child (lowest slot among equals) is visited next */
            const int hi = order == ORC_WIDE_ORDER_HIGHEST_AMONG_EQUALS;
            const int A = hi ? k[1] <= k[0] : k[1] < k[0], B = hi ? k[3] <= k[2] : k[3] < k[2];
            const float k01 = A ? k[1] : k[0], k23 = B ? k[3] : k[2];
            const int s01 = A ? 1 : 0, s23 = B ? 3 : 2;
            const int Cc = hi ? k23 <= k01 : k23 < k01;
            const float bestKey = Cc ? k23 : k01;
            const int best = Cc ? s23 : s01;
            int hits = 0;
            for (int i = 0; i < 4; ++i) hits += k[i] != tRay;
            if (st) ++st->slots[hits];
            if (bestKey != tRay) {
                /* the other hit children go on the stack in slot order */
                for (int j = 0; j < 4; ++j) {
                    const int i = order == ORC_WIDE_ORDER_REVERSED_PUSH ? 3 - j : j;
                    if (i != best && k[i] != tRay && head < 1024) stack[head++] = ref[i];
                }
                if (head > maxDepth) maxDepth = head;
                node = ref[best];
                continue;
            }
        } else {
            const int32_t first = (int32_t)(node & 0xFFFFFFu);
            const int32_t last = first + (int32_t)(node >> 24);
            for (int32_t i = first; i < last; ++i) { ray.tFar = pair_intersect(pairs, i, &ray, &hit); if (st) ++st->np; }
        }
        if (!head) break;
        node = stack[--head];
    }
    if (st) ++st->depthHist[maxDepth < 63 ? maxDepth : 63];
    if (depthOut) *depthOut = maxDepth;
    ray_epilogue(remap, env, envW, envH, &ray, &hit, out);
}

/* counters (all optional when `counters` is NULL), summed over the batch:
 *   [0] wide node visits   [1] pair tests
 *   with `bvh2` (the reference-format node blob the records were collapsed from) the binary oracle runs next to the model:
 *   [2] records that differ from it in any bit of triangle, t, u, v (a miss record: in the triangle word only), of which
 *   [3] ties     both hit, another triangle, |t - t'| <= 1e-6 |t'|
 *   [4] closer   the model hits where the oracle misses, or at a smaller t (and it is no tie)
 *   [5] aliases  the oracle's triangle through another of its references: t within 2e-6 relative + 2e-5, u and v within 1e-4
 *   [6] others   anything else (must be 0)
 *   [7] the deepest stack of any ray */
enum { ORC_WIDE_COUNTERS = 8 };

typedef struct {
    const void* records; int format; const orc_gpu_node* bvh2; const orc_pair* pairs; const uint32_t* remap;
    const float* env; uint32_t envW, envH;
    const orc_ray* rays; orc_result* results; uint32_t count, slice; int order;
    uint32_t* depth; unsigned long long* counters; uint64_t* cursor;
} wide_job;

static void* wide_worker(void* arg) {
    wide_job* j = (wide_job*)arg;
    const uint64_t slices = ((uint64_t)j->count + j->slice - 1) / j->slice;
    unsigned long long c[ORC_WIDE_COUNTERS] = { 0 };
    orc_wide_stats st;
    memset(&st, 0, sizeof(st));
    for (;;) {
        const uint64_t s = __atomic_fetch_add(j->cursor, 1, __ATOMIC_RELAXED);
        if (s >= slices) break;
        const uint32_t b = (uint32_t)(s * j->slice), e = b + j->slice < j->count ? b + j->slice : j->count;
        for (uint32_t i = b; i < e; ++i) {
            uint32_t dp = 0;
            orc_result* g = j->results + i;
            traverse_wide_one(j->records, j->format, j->pairs, j->remap, j->env, j->envW, j->envH, j->rays + i, g, j->order, &dp, &st);
            if (j->depth) j->depth[i] = dp;
            if (dp > c[7]) c[7] = dp;
            if (!j->bvh2) continue;
            orc_result r;
            traverse_one(j->bvh2, j->pairs, j->remap, j->env, j->envW, j->envH, j->rays + i, &r, 0, 0, 0);
            const int hg = g->triangle != 0xFFFFFFFFu, hr = r.triangle != 0xFFFFFFFFu;
            if (g->triangle == r.triangle && (!hr || (f2u(g->t) == f2u(r.t) && f2u(g->u) == f2u(r.u) && f2u(g->v) == f2u(r.v)))) continue;
            ++c[2];
            if (hg && hr && g->triangle != r.triangle && fabsf(g->t - r.t) <= 1e-6f * fabsf(r.t)) ++c[3];
            else if (hg && hr && g->triangle == r.triangle && fabs((double)g->t - r.t) <= 2e-5 + 2e-6 * fabs((double)r.t) &&
                     fabs((double)g->u - r.u) <= 1e-4 && fabs((double)g->v - r.v) <= 1e-4) ++c[5];
            else if (hg && (!hr || g->t < r.t)) ++c[4];
            else ++c[6];
        }
    }
    c[0] = st.nv; c[1] = st.np;
    if (j->counters) {
        for (int k = 0; k < 7; ++k) __atomic_fetch_add(&j->counters[k], c[k], __ATOMIC_RELAXED);
        unsigned long long seen = __atomic_load_n(&j->counters[7], __ATOMIC_RELAXED);
        while (seen < c[7] && !__atomic_compare_exchange_n(&j->counters[7], &seen, c[7], 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    return 0;
}

void orc_traverse_wide_mt(const void* records, int format, const orc_gpu_node* bvh2, const orc_pair* pairs, const uint32_t* remap,
                          const float* env, uint32_t envW, uint32_t envH,
                          const orc_ray* rays, orc_result* results, uint32_t count, int order, uint32_t threads,
                          uint32_t* maxDepthOut, unsigned long long* counters) {
    if (!threads) threads = 1;
    if (threads > 64) threads = 64;
    if (counters) memset(counters, 0, sizeof(unsigned long long) * ORC_WIDE_COUNTERS);
    uint64_t cursor = 0;
    wide_job job = { records, format, bvh2, pairs, remap, env, envW, envH, rays, results, count, 1024, order, maxDepthOut, counters, &cursor };
    pthread_t tid[64];
    for (uint32_t t = 1; t < threads; ++t) pthread_create(&tid[t], 0, wide_worker, &job);
    wide_worker(&job);
    for (uint32_t t = 1; t < threads; ++t) pthread_join(tid[t], 0);
}
