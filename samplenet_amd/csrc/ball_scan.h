// ball_scan.h -- the ball query's scan of one query by one wave and its launch rule, shared by the units that group behind it
// (ball_query.hip: channel-major grouping; set_abstraction.hip: row-major grouping).  The contract is written out at the top of
// ball_query.hip and in include/samplenet_hip_internal.h; every unit that includes this is built with -ffp-contract=off.
#pragma once
#include <climits>
#include <cmath>

#include "sn_common.h"

#pragma clang fp contract(off)  // the contract's distance is product-then-sum (no FMA)

namespace sn {

constexpr int kBallWaves = 4;               // waves per workgroup
constexpr int kBallMaxQueriesPerWave = 4;   // queries a wave takes in sequence, at most
constexpr int kBallWaveSlots = 256 * 32;    // resident waves of the chip (256 CUs x 32)

// Queries a wave takes in sequence.  With fewer queries than wave slots a second query per wave only empties SIMDs (the fused
// gather and the scatter are latency-bound: at 32 x 128 queries, c = 128, four per wave left one wave per SIMD); beyond, queries
// in sequence save workgroup dispatches.
inline int ball_queries_per_wave(long long queries)
{
    const long long q = (queries + kBallWaveSlots - 1) / kBallWaveSlots;
    return q < 1 ? 1 : (q > kBallMaxQueriesPerWave ? kBallMaxQueriesPerWave : (int)q);
}

template <int RULE>
__device__ __forceinline__ bool ball_pass(float d2, float thr)
{
    if (RULE == SN_BALL_RULE_SQRT) {
        const float s = sqrtf(d2);                   // correctly rounded (the build keeps hipcc's default for sqrt and division)
        const float d = s < 1e-20f ? 1e-20f : s;     // std::max(s, 1e-20f): a NaN stays a NaN
        return d < thr;                              // thr = radius
    }
    return d2 < thr;                                 // thr = fl(radius * radius), or -1 when radius is not > 0
}

// The scan of one query by one wave (all 64 lanes arrive, uniform arguments except `lane`).  Writes row[0 .. nsample) and returns
// min(hits, nsample); the unfilled slots repeat the first hit (0 for an empty ball).
template <int RULE>
__device__ __forceinline__ int ball_scan_row(int n, int nsample, float thr, const float *__restrict__ P, int layout1, float qx, float qy,
                                             float qz, int lane, int *row)
{
    int cnt = 0, first = 0;
    for (int base = 0; base < n; base += kWave) {
        const int k = base + lane;
        bool pass = false;
        if (k < n) {
            const float dx = qx - P[pt_off(layout1, n, k, 0)];
            const float dy = qy - P[pt_off(layout1, n, k, 1)];
            const float dz = qz - P[pt_off(layout1, n, k, 2)];
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            pass = ball_pass<RULE>(d2, thr);
        }
        const sn_u64 mask = __ballot(pass);
        if (mask == 0) continue;
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        const int slot = cnt + below;
        if (pass && slot < nsample) row[slot] = k;
        if (cnt == 0) first = base + (int)__builtin_ctzll(mask);
        cnt += (int)__builtin_popcountll(mask);
        if (cnt >= nsample) break;
    }
    const int hits = cnt < nsample ? cnt : nsample;
    for (int s = hits + lane; s < nsample; s += kWave) row[s] = first;
    return hits;
}

// queries per wave, workgroups per cloud and the grid of a launch in which a wave owns a query
inline int ball_grid(const char *who, int b, int m, int *qpw, int *groups, unsigned *grid)
{
    *qpw = ball_queries_per_wave((long long)b * m);
    const int per_group = kBallWaves * *qpw;
    *groups = (int)(((long long)m + per_group - 1) / per_group);
    const long long g = (long long)b * *groups;
    if (g > INT_MAX) return sn_set_error(SN_ERR_UNSUPPORTED, "%s: the launch needs more than 2^31 - 1 workgroups", who);
    *grid = (unsigned)g;
    return 0;
}

// fl(radius * radius) for the squared rule (-1: nothing passes), the radius itself for the reference's rule (its comparison is
// false for a NaN and for every radius <= 1e-20f without help)
inline float ball_threshold(float radius, int rule)
{
    if (rule == SN_BALL_RULE_SQRT) return radius;
    if (!(radius > 0.f)) return -1.f;
    return radius * radius;  // one fp32 product, rounded once
}

}  // namespace sn
