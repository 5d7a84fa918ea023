// racc_world_rule.h — the per-instance rule of instancing, stated once: the float-rounded double-precision inverse of a 3x4 transform, the
// conservative world-space box of its root box and its condition number (world_build.cpp's head has the bound).  Compiled for the host by
// world_build.cpp (racc_host_world_prepare, racc_host_world_refit) and for the device by racc_world_refit.inc (worldRefitKernel): the same
// expressions in the same order, in double, nothing contracted (-ffp-contract=off on both sides), so the two agree bit for bit.
// std::max / std::min / std::fabs are written as the comparisons they are (no fmax / fmin: those differ on NaN and on the device).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RACC_RULE_FN __host__ __device__ inline
#else
#define RACC_RULE_FN inline
#endif

namespace racc_world_rule {

enum Refusal {      // in the order the checks are made
    kOk = 0,
    kTransformNotFinite,
    kRootBoxNotFinite,
    kRootBoxInverted,
    kSingular,
    kInverseNotFinite,
    kWorldBoxNotFinite,
};

RACC_RULE_FN double maxOf(double a, double b) { return a < b ? b : a; }      // std::max
RACC_RULE_FN double minOf(double a, double b) { return b < a ? b : a; }      // std::min
RACC_RULE_FN double absOf(double x) { return __builtin_fabs(x); }
RACC_RULE_FN bool finite(double x) { return __builtin_isfinite(x); }
RACC_RULE_FN bool finite(float x) { return __builtin_isfinite(x); }

RACC_RULE_FN float roundDown(double x) { const float f = float(x); return double(f) > x ? nextafterf(f, -INFINITY) : f; }
RACC_RULE_FN float roundUp(double x) { const float f = float(x); return double(f) < x ? nextafterf(f, INFINITY) : f; }

constexpr double kMarginK = 1.0 / 1048576.0;      // 2^-20, see the head of world_build.cpp

// The ray's share of the margin for the largest condition number of a world.
RACC_RULE_FN float rayPadOf(double maxCond) { return roundUp(2.0 * kMarginK * maxCond); }

// One instance: m = its twelve transform coefficients, rb = its object-space root box {min[3], max[3]}.  Writes the inverse (o, twelve
// floats), the world box (w, {min[3], max[3]}) and the condition number; on a refusal what o, w and cond hold is unspecified.
RACC_RULE_FN Refusal instance(const float* m, const float* rb, float* o, float* w, double& cond) {
    for (int k = 0; k < 12; ++k) if (!finite(m[k])) return kTransformNotFinite;
    for (int k = 0; k < 6; ++k) if (!finite(rb[k])) return kRootBoxNotFinite;
    for (int k = 0; k < 3; ++k) if (rb[k] > rb[3 + k]) return kRootBoxInverted;
    const double a[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } };
    const double b[3] = { m[3], m[7], m[11] };
    double c[3][3];      // cofactors: c[r][k] = cofactor of a[r][k]
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            c[r][k] = a[r1][k1] * a[r2][k2] - a[r1][k2] * a[r2][k1];
        }
    const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
    if (det == 0.0 || !finite(det)) return kSingular;
    double B[3][3], t[3], normA = 0.0, normB = 0.0, normb = 0.0;
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) B[r][k] = c[k][r] / det;      // adjugate = transposed cofactors
    for (int r = 0; r < 3; ++r) t[r] = -((B[r][0] * b[0] + B[r][1] * b[1]) + B[r][2] * b[2]);
    for (int r = 0; r < 3; ++r) {
        o[r * 4 + 0] = float(B[r][0]); o[r * 4 + 1] = float(B[r][1]); o[r * 4 + 2] = float(B[r][2]); o[r * 4 + 3] = float(t[r]);
        for (int k = 0; k < 4; ++k) if (!finite(o[r * 4 + k])) return kInverseNotFinite;
        normA = maxOf(normA, absOf(a[r][0]) + absOf(a[r][1]) + absOf(a[r][2]));
        normB = maxOf(normB, absOf(B[r][0]) + absOf(B[r][1]) + absOf(B[r][2]));
        normb = maxOf(normb, absOf(b[r]));
    }
    cond = normA * normB;
    // the eight corners in double: per world axis the extremes are reached by picking min or max per object axis
    double lo[3], hi[3], mag = 0.0;
    for (int r = 0; r < 3; ++r) {
        lo[r] = hi[r] = b[r];
        for (int k = 0; k < 3; ++k) {
            const double p = a[r][k] * double(rb[k]), q = a[r][k] * double(rb[3 + k]);
            lo[r] += minOf(p, q); hi[r] += maxOf(p, q);
        }
        mag = maxOf(mag, maxOf(absOf(lo[r]), absOf(hi[r])));
    }
    const double margin = kMarginK * cond * (normb + mag);
    for (int r = 0; r < 3; ++r) {
        // (the sums above carry a few double roundings of their own: 2^-40 of the magnitudes, far inside the margin)
        w[r] = roundDown(lo[r] - margin); w[3 + r] = roundUp(hi[r] + margin);
        if (!finite(w[r]) || !finite(w[3 + r])) return kWorldBoxNotFinite;
    }
    return kOk;
}

}  // namespace racc_world_rule
