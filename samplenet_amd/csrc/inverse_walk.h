// inverse_walk.h -- the sum over one destination row's list of sn_gather_invert, and the launch rule of the kernels in which a group
// of lanes owns a row, shared by the row-layout gradients "by inverted index" (set_abstraction.hip: sn_group_rows_backward;
// feature_rows.hip: sn_interp_rows_backward) and stated here once.  include/samplenet_hip_internal.h gives the callers' contracts.
//
// THE WALK.  start points at the row's two words (start[0], start[1]: where its list begins and ends in `order`), ne is the cloud's
// entry count.  The sum is taken over i in [max(start[0], 0), min(start[1], ne)) in ascending i -- list order, which for lists of
// sn_gather_invert is ascending entry number -- from +0, one term and one rounded add per entry e = order[i]:
//     unweighted   g[(e / K) * stride]
//     weighted     fl(g[(e / K) * stride] * w[e])      the product rounded, then added
// K entries share a source row (K = 1: every entry has its own).  Loads go kWalkBatch entries at a time: their entry numbers first
// (-1 past the list's end), then their operands side by side, then the adds, still one by one and in list order, so the batching
// cannot show in the bits.  CLAMP AND SKIP: a start outside [0, ne] or an entry number outside [0, ne) can only come from a caller's
// own buffers; the bounds are clamped and such an entry contributes nothing -- its loads read entry 0's operands and are dropped --
// so foreign lists cannot make the walk read elsewhere.  (gather_bwd_inverted_kernel, feature_propagate.hip, keeps the same rule in
// its channel-major body.)  An empty list gives +0.  Lists are not split: a launch takes as long as its longest list.
//
// The arithmetic RELIES ON THE INCLUDING UNIT'S `#pragma clang fp contract(off)`: with contraction on, the weighted term's product
// and add would fuse and the bits of the ordered route would be lost.
#pragma once
#include <climits>

#include "sn_common.h"

namespace sn {

constexpr int kWalkBatch = 4;     // entries of a list whose loads are in flight together
constexpr int kLaneThreads = 256; // workgroup of a lane-group launch

template <int K, bool WEIGHTED>
__device__ __forceinline__ float inverse_walk_sum(const int *start, const int *order, int ne, const float *g, int stride, const float *w)
{
    const int lo = max(start[0], 0), hi = min(start[1], ne);
    float acc = 0.f;
    for (int i = lo; i < hi; i += kWalkBatch) {
        int e[kWalkBatch];
        float wt[kWalkBatch], gv[kWalkBatch];
#pragma unroll
        for (int t = 0; t < kWalkBatch; ++t) e[t] = i + t < hi ? order[i + t] : -1;
#pragma unroll
        for (int t = 0; t < kWalkBatch; ++t) {
            const unsigned at = (unsigned)e[t] < (unsigned)ne ? (unsigned)e[t] : 0u;   // (an entry that is skipped below reads entry 0's operands)
            wt[t] = WEIGHTED ? w[at] : 0.f;
            gv[t] = g[(size_t)(at / (unsigned)K) * stride];
        }
#pragma unroll
        for (int t = 0; t < kWalkBatch; ++t)
            if ((unsigned)e[t] < (unsigned)ne) acc += WEIGHTED ? gv[t] * wt[t] : gv[t];
    }
    return acc;
}

// THE LAUNCH RULE.  A group of lg lanes, the power of two covering `cols` (64 at most), owns an item; a workgroup of kLaneThreads
// holds kLaneThreads / lg of them.  An item is a row (chunked == false: the group walks the row's columns lg at a time) or a row and
// one chunk of lg of its columns.
inline int sn_too_many_workgroups(const char *who)
{
    return sn_set_error(SN_ERR_UNSUPPORTED, "%s: the launch needs more than 2^31 - 1 workgroups", who);
}

inline int lane_group(long long cols)
{
    int lg = 1;
    while (lg < cols && lg < kWave) lg <<= 1;
    return lg;
}

struct LaneGrid {
    int lg, chunks;
    long long items;
    unsigned grid;
};

inline int lane_grid(const char *who, long long rows, int cols, bool chunked, LaneGrid *l)
{
    l->lg = lane_group(cols);
    l->chunks = chunked ? (int)(((long long)cols + l->lg - 1) / l->lg) : 1;
    l->items = rows * l->chunks;
    const int per = kLaneThreads / l->lg;
    const long long grid = (l->items + per - 1) / per;
    if (grid > INT_MAX) return sn_too_many_workgroups(who);
    l->grid = (unsigned)grid;
    return 0;
}

}  // namespace sn
