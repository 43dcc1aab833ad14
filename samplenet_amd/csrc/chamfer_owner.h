// chamfer_owner.h -- what the units that form a Chamfer gradient share (chamfer_backward.hip, sampler_step_loss.hip,
// progressive_prefix.hip): the implicit upstream gradient, the ordered owner sum of the register-resident kernels, and the one
// launch helper two of them call.  Device code here is __forceinline__ only: every kernel is defined in exactly one unit.
#pragma once
#include "sn_common.h"

namespace sn {

struct sn_xyz3 {
    float x, y, z;
};

constexpr int kMaxPrefixes = 16;  // nested prefixes / grouped evaluations a launch takes by value

// Implicit upstream gradients (fused simplification loss, samplenet.py:171-181): with gL = d loss / d (scalar loss),
//   g(dist of target j)  = gL * (ct + (j == argmax_t[b] ? cmax_t : 0)),   g(dist of source l) = gL * (cs + (l == argmax_s[b] ? cmax_s : 0))
// so no per-point gradient tensors are materialised.  gL == NULL: explicit gT / gS arrays are used.
struct ImplicitGrad {
    const float *gL;
    const int *argmax_t, *argmax_s;
    float ct, cmax_t, cs, cmax_s;
    float gscale = 1.f;  // upstream gradient = *gL * gscale (rounded once, like a separate scaling op in front would)
};

// ------------------------------------------------------------------------------------------------
// Ordered owner sum of the register-resident kernels.  The sources whose nearest target is j ("owners") are met slot
// by slot (slot i = sources i * 64 + lane); the reference adds their contributions one after the other in ascending source
// index, and so does this -- the same fp32 subtractions in the same order -- but as a chain over lanes instead of a scalar
// walk (find the lowest set bit, clear it, three v_readlane, three dependent v_sub: ~10 issue slots per owner on a value
// that is the same in all 64 lanes):
//   1. every owner's rank among the query's owners = popcount of the earlier slots' ballots + mbcnt of its own; the owners
//      store their contributions, compacted in that order, into a list of kOwnerCap entries per wave in LDS;
//   2. the list is read back 16 entries per row of 16 lanes, x / y / z in rows 0 / 1 / 2, and every entry is one link
//      acc = row_ror:1(acc) - c: lane t's link t + 1 takes the running value from lane t - 1 and subtracts entry t, lane 0
//      takes it from lane 15 -- the start value, or the end of the chunk before -- so the chunks follow each other without
//      any hand-over and the sum stands in lane 15 after 16 links (whatever the other lanes hold by then).  Entries past the
//      end of the list subtract +0, which changes no bit of any value; the last chunk stops after its own entries (rounded
//      up to 4 links) and the sum is taken from the lane it has reached.
// The list is drained when the slots are through, not per slot (one owner per slot is the usual case and an LDS round trip
// per slot would cost more than the walk it replaces); a query can own every source, so the list is bounded and the slots are
// passed once more per kOwnerCap owners.
// ------------------------------------------------------------------------------------------------
constexpr int kOwnerCap = 256;            // entries of a wave's list, a multiple of 16 (the headline's busiest queries own ~120 points)
constexpr int kOwnerRow = kOwnerCap + 16;  // one coordinate's row: the entries, then 16 words that take the stores of owners past the
                                           // capacity in the first pass and the (masked-off) read of a chunk behind the last one
struct OwnerList {
    float c[3][kOwnerRow];
};

__device__ __forceinline__ float dpp_row_ror1(float x)  // lane below within the row of 16; the row's lane 0 reads its lane 15
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x121, 0xf, 0xf, true));
}

// (ax, ay, az) -> ((a - c_o0) - c_o1) - ... over the owners o0 < o1 < ... of target j, c_o = gg_o (s_o - t); wave-uniform in and out
template <int PPL>
__device__ __forceinline__ void owner_sum(OwnerList &L, int lane, int j, const int (&is)[PPL], const float (&gg)[PPL],
                                          const float (&sx)[PPL], const float (&sy)[PPL], const float (&sz)[PPL], float tx,
                                          float ty, float tz, float &ax, float &ay, float &az)
{
    const int row = lane >> 4, sub = lane & 15;
    // (row 3 idles along row 2.  min(), not a select: written as row < 3 ? row : 2 the instruction chosen depended on which other
    //  kernels of the unit call this function -- v_min_u32 beside chamfer_soft_bwd_kernel, a compare and a select without it)
    const float *col = &L.c[min(row, 2)][sub];
    float acc = row == 0 ? ax : (row == 1 ? ay : az);
    int at = 15;  // lane of every row that holds the sum
    auto drain = [&](int cnt) {  // the chain over the first cnt entries of the list
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the list: written by other lanes of this wave
        float v = sub < cnt ? col[0] : 0.f;
#pragma nounroll
        for (int c0 = 0; c0 < cnt; c0 += 16) {
            const int e = c0 + 16 + sub;  // the next chunk is on its way while this one's chain runs
            const float vn = e < cnt ? col[c0 + 16] : 0.f;
            const int rem = cnt - c0;
            if (rem >= 16) {
#pragma unroll
                for (int t = 0; t < 16; ++t) acc = dpp_row_ror1(acc) - v;
            } else {  // the last chunk of all
#pragma nounroll
                for (int t = 0; t < rem; t += 4) {
                    acc = dpp_row_ror1(acc) - v;
                    acc = dpp_row_ror1(acc) - v;
                    acc = dpp_row_ror1(acc) - v;
                    acc = dpp_row_ror1(acc) - v;
                }
                at = ((rem + 3) & ~3) - 1;
            }
            v = vn;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // nothing is in flight here, but the compiler counts the masked-off read of a chunk behind the last one as pending and
        // would wait for the LDS queue -- the stores of the slot before -- in every slot of the next pass or query
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
    };
    // the first pass over the slots lists the owners of rank 0 .. kOwnerCap - 1 (those past it store into the row's spare words)
    int total = 0;  // owners in the slots so far
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
        const bool own = is[i] == j;
        const sn_u64 mask = __ballot(own);
        if (mask) {
            // (a product of its own: no fma may absorb it into the chain's subtraction)
            const float cx = gg[i] * (sx[i] - tx), cy = gg[i] * (sy[i] - ty), cz = gg[i] * (sz[i] - tz);
            const unsigned r = total + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            const unsigned rc = r < (unsigned)kOwnerCap ? r : (unsigned)kOwnerCap;
            if (own) L.c[0][rc] = cx, L.c[1][rc] = cy, L.c[2][rc] = cz;
            total += __builtin_popcountll(mask);
        }
    }
    drain(total < kOwnerCap ? total : kOwnerCap);
    // a query with more owners (rare: the mean is ns / nt) takes one further pass and chain per kOwnerCap of them
#pragma nounroll
    for (int base = kOwnerCap; base < total; base += kOwnerCap) {
        // (opaque to the compiler: otherwise it forms the ballots and contributions of ALL slots ahead of this loop and keeps them,
        //  2 PPL scalar and 3 PPL vector registers)
        j = __builtin_amdgcn_readfirstlane(j);  // (wave-uniform already; a scalar register whatever the compiler made of it)
        asm volatile("" : "+v"(tx), "+v"(ty), "+v"(tz), "+s"(j));
        int n = 0;
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const bool own = is[i] == j;
            const sn_u64 mask = __ballot(own);
            if (mask) {
                const int n0 = n;
                n += __builtin_popcountll(mask);
                if (n > base && n0 < base + kOwnerCap) {
                    const float cx = gg[i] * (sx[i] - tx), cy = gg[i] * (sy[i] - ty), cz = gg[i] * (sz[i] - tz);
                    const int r = n0 - base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    if (own && (unsigned)r < (unsigned)kOwnerCap) L.c[0][r] = cx, L.c[1][r] = cy, L.c[2][r] = cz;
                }
            }
        }
        drain(total - base < kOwnerCap ? total - base : kOwnerCap);
    }
    ax = readlane_f(acc, at), ay = readlane_f(acc, 16 + at), az = readlane_f(acc, 32 + at);
}

// workgroups (of 4 waves) the targets of all clouds are spread over: every wave loads the whole source set into registers
// before its first target, so fewer, longer-lived waves amortise that load (1024 groups = one target per wave at the
// sampler's sizes: measured 9 us; swept 64..1024 at B = 32: 1024 is fastest)
constexpr int kChamferBwdGroups = 1024;

// the Chamfer backward of one side, register-resident up to 2048 sources (chamfer_backward.hip); the sampler step's loss backward
// takes it for larger clouds
void launch_chamfer_bwd(int b, int ysplit, int nt, int ns, const float *T, const float *S, const float *gT, const int *idxT,
                        const float *gS, const int *idxS, float *gradT, int own_first, const ImplicitGrad &ig, hipStream_t st,
                        int t_layout = 0);

}  // namespace sn
