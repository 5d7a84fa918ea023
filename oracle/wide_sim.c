/*
 * wide_sim.c — CPU model of the engine's 4-wide traversal (analysis tool + checker, test infrastructure).
 *
 * The engine's device format may differ from the reference's as long as the results do not: at upload the
 * reference-format BVH2 (Scene.cpp:73-78) can be collapsed into 4-wide nodes, one 128-byte vector-L1 line each.  This
 * program restates that collapse and the 4-wide traversal on the CPU, runs it next to the reference-order BVH2 traversal
 * (racc_oracle.c, Kernels.h:139-242) on the same buffers and reports
 *   - node visits / pair tests / stack depth per ray for both,
 *   - how many results differ, split into exact-distance ties (same t, other primitive: either answer is a closest hit,
 *     SURVEY.md §8c's arbiter rule) and real differences (must be 0).
 * The per-box test is the reference's (same fma, same "entry distance == tFar counts as missed" rule, Kernels.h:117-135,
 * 192-194); only the ORDER in which the hit children are visited is the wide node's own: nearest entry distance first.
 *
 * The collapse, the quantisation and the traversal are racc_oracle_wide.c's — the exact model that tests/test_wide_format.py holds
 * to the product's records byte for byte and tests/test_gpu_wide_exact.py to the kernels' results bit for bit; this program
 * only reads files, runs it and prints the statistics.
 *
 * Build: gcc -O2 -ffp-contract=off -mavx2 -mfma -o wide_sim wide_sim.c -lm -lpthread   (includes racc_oracle_wide.c, which includes racc_oracle.c)
 * Run:   wide_sim nodes.bin pairs.bin remap.bin rays.bin [order] [maxrays] [quant]
 *        order 0 = the product's visiting rule (default), 1 = highest slot among equals, 2 = reversed push order (the model's test-only variants)
 *        quant 1 = the 64-byte compressed node of racc_kernel_v10.inc: the four child boxes quantised conservatively to 8 bits
 *                  per plane on the box that encloses them (origin + q * scale, decoded with one fmaf exactly as the kernel
 *                  does); every decoded box contains the reference's box, so every box the reference enters is entered.
 */
#include "racc_oracle_wide.c"

#include <stdio.h>

static void* slurp(const char* path, size_t* n) {
    FILE* f = fopen(path, "rb"); if (!f) { perror(path); exit(3); }
    fseek(f, 0, SEEK_END); *n = (size_t)ftell(f); rewind(f);
    void* p = malloc(*n); if (fread(p, 1, *n, f) != *n) exit(3); fclose(f); return p;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: wide_sim nodes.bin pairs.bin remap.bin rays.bin [order] [maxrays] [quant]\n"); return 2; }
    size_t nb, pb, rb, mb;
    orc_gpu_node* nodes = slurp(argv[1], &nb);
    orc_pair* pairs = slurp(argv[2], &pb);
    uint32_t* remap = slurp(argv[3], &mb);
    orc_ray* rays = slurp(argv[4], &rb);
    const int order = argc > 5 ? atoi(argv[5]) : 0;
    const uint32_t nodeCount = (uint32_t)(nb / 64);
    uint32_t count = (uint32_t)(rb / 32);
    if (argc > 6 && (uint32_t)atoi(argv[6]) < count) count = (uint32_t)atoi(argv[6]);
    orc_wide_node* wide = aligned_alloc(128, sizeof(orc_wide_node) * nodeCount);
    uint32_t stackBound = 0;
    const uint32_t wideCount = orc_collapse_wide(nodes, nodeCount, wide, &stackBound);
    const int quant = argc > 7 ? atoi(argv[7]) : 0;
    const void* records = wide;
    if (quant) {
        orc_wide_node_q* packed = aligned_alloc(64, sizeof(orc_wide_node_q) * wideCount);
        const int rc = orc_quantise_wide(wide, wideCount, packed);
        if (rc) { fprintf(stderr, "quantise: refused (%d)\n", rc); return 4; }
        float* planes = malloc(sizeof(float) * 24 * (size_t)wideCount);
        orc_decode_wide(packed, 50, wideCount, planes);
        double growth = 0.0;
        for (uint32_t i = 0; i < wideCount; ++i)
            for (int p = 0; p < 6; ++p)
                for (uint32_t c = 0; c < wide[i].used; ++c) growth += fabs((double)planes[((size_t)i * 6 + p) * 4 + c] - wide[i].plane[p][c]);
        fprintf(stderr, "quantised %u nodes, mean plane displacement %.3g\n", wideCount, growth / (24.0 * wideCount));
        free(planes);
        records = packed;
    }
    unsigned long long full = 0;
    for (uint32_t i = 0; i < wideCount; ++i) full += wide[i].used;
    orc_wide_stats st; memset(&st, 0, sizeof(st));
    unsigned long long nv2 = 0, np2 = 0, d2 = 0, ties = 0, diffs = 0, d2max = 0, closer = 0, depthSum = 0, depthMax = 0;
    for (uint32_t i = 0; i < count; ++i) {
        orc_result a, b; uint32_t nv, np, dp, dw;
        traverse_one(nodes, pairs, remap, 0, 0, 0, rays + i, &a, &nv, &np, &dp);
        nv2 += nv; np2 += np; d2 += dp; if (dp > d2max) d2max = dp;
        traverse_wide_one(records, quant ? 50 : 45, pairs, remap, 0, 0, 0, rays + i, &b, order, &dw, &st);
        depthSum += dw; if (dw > depthMax) depthMax = dw;
        if (a.triangle != b.triangle || f2u(a.t) != f2u(b.t) || f2u(a.u) != f2u(b.u) || f2u(a.v) != f2u(b.v)) {
            if (a.triangle != 0xFFFFFFFFu && b.triangle != 0xFFFFFFFFu && fabsf(a.t - b.t) <= 1e-6f * fabsf(a.t)) ++ties;
            else if (quant && b.triangle != 0xFFFFFFFFu && (a.triangle == 0xFFFFFFFFu || b.t < a.t)) ++closer;      /* the larger boxes let a hit through that the reference's own box test culled (box vs triangle rounding): a closer hit, not a wrong one */
            else { ++diffs; if (diffs < 5) fprintf(stderr, "diff ray %u: %u %g %g %g | %u %g %g %g\n", i, a.triangle, a.t, a.u, a.v, b.triangle, b.t, b.u, b.v); }
        }
    }
    printf("{\"rays\": %u, \"order\": %d, \"bvh2_nodes\": %u, \"wide_nodes\": %u, \"stack_bound\": %u, \"slots_used\": %.2f, \"nv2\": %.2f, \"np2\": %.2f, \"depth2_mean\": %.2f, \"depth2_max\": %llu, "
           "\"nv4\": %.2f, \"np4\": %.2f, \"depth4_mean\": %.2f, \"depth4_max\": %llu, \"hits_per_visit\": [%.3f, %.3f, %.3f, %.3f, %.3f], \"ties\": %llu, \"closer_than_reference\": %llu, \"differences\": %llu}\n",
           count, order, nodeCount, wideCount, stackBound, (double)full / wideCount, (double)nv2 / count, (double)np2 / count, (double)d2 / count, d2max,
           (double)st.nv / count, (double)st.np / count, (double)depthSum / count, depthMax,
           (double)st.slots[0] / st.nv, (double)st.slots[1] / st.nv, (double)st.slots[2] / st.nv, (double)st.slots[3] / st.nv, (double)st.slots[4] / st.nv, ties, closer, diffs);
    if (getenv("WIDE_SIM_HIST")) {
        fprintf(stderr, "rays by deepest stack / visits by stack height at the visit:\n");
        unsigned long long cr = 0, cv = 0;
        for (int d = 0; d < 64; ++d) { cr += st.depthHist[d]; cv += st.deepVisits[d]; if (st.depthHist[d] || st.deepVisits[d]) fprintf(stderr, "  %2d: rays %8llu (cum %.5f)  visits %10llu (cum %.5f)\n", d, st.depthHist[d], (double)cr / count, st.deepVisits[d], (double)cv / st.nv); }
    }
    return diffs ? 1 : 0;
}
