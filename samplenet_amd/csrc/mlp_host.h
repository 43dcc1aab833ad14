// mlp_host.h -- host-side launch helpers shared by the forward and backward units of the PointNet MLP (pointnet_mlp.hip,
// pointnet_mlp_backward.hip).  What it holds:
//   * tile shapes, LDS sizing (lds_bytes) and occupancy shaping (shaped_lds), device_cus
//   * operand builders: make_act, make_dz, make_fwd (the backward unit's own argument blocks, DgradArgs / WgradArgs, are declared
//     there and built there: make_dgrad / make_wgrad at the head of its host section), wgrad_rows_per_split
//   * the FULL-tile launch macro SN_LAUNCH_T
//   * the mode dispatch: dispatch_act / dispatch_modes turn (dz_mode, "the layer below has a BatchNorm") into the kernels' template
//     parameters, over the combinations the call site names and no others
//   * launch_lds_twins: the FULLR = true / false pair of a kernel that needs more than 64 KB of dynamic LDS
#pragma once
#include <type_traits>

#include "mlp_device.h"

namespace sn {

using TileBig = Tile<64, 64, 2, 2>;     // R large: 64 rows x 64 cols per 256-thread workgroup -> >= 2 workgroups per CU
                                        // at B*N = 32768 rows, so one workgroup's load latency hides under another's MFMAs
using TileWide = Tile<64, 128, 2, 4>;   // conv layers with 128 output channels: one 512-thread workgroup per 64 rows (Tile<64, 128, 2, 2>,
                                        // 32 x 64 per wave, half the LDS fragment traffic: 17.5 vs 15.8 us on the 128 -> 128 layer)
using TileSmall = Tile<32, 128, 1, 4>;  // R small (FC head at small batch): 32 rows x 128 cols
using TileW = Tile<64, 64, 2, 2>;       // weight gradient: Co x (Ci+1) output tile

template <class T>
static size_t lds_bytes()
{
    return sizeof(float) * std::max(T::LDS_FLOATS, T::WR * 2 * T::BN);
}

}  // namespace sn

using namespace sn;

extern "C" int sn_linear_stats_blocks(int R);

static ActSrc make_act(const float *z, const float *coef, int rows, int ch, int ones_col = -1)
{
    ActSrc a{};
    a.z = z, a.rows = rows, a.ch = ch, a.ones_col = ones_col;
    a.mode = coef ? ACT_BN_RELU : ACT_NONE;
    a.scale = coef, a.shift = coef ? coef + ch : nullptr;
    return a;
}

static DzSrc make_dz(int mode, const float *dy, const float *z, const float *kcoef, const float *gsel, const int *argsel,
                     int rows, int ch, int npts)
{
    DzSrc d{};
    d.mode = mode, d.dy = dy, d.z = z, d.rows = rows, d.ch = ch, d.npts = npts > 0 ? npts : 1;
    d.k1 = kcoef, d.k2 = kcoef ? kcoef + ch : nullptr, d.k3 = kcoef ? kcoef + 2 * ch : nullptr;
    d.gsel = gsel, d.argsel = argsel;
    return d;
}

// the operands every forward entry has; what only some have (bn, pool_*, the statistics chain) is set by the entry
static FwdArgs make_fwd(int R, int Ci, int Co, const float *ain, const float *coef_prev, const float *W, const float *bias, float *z,
                        float *stats)
{
    FwdArgs g{};
    g.a = make_act(ain, coef_prev, R, Ci);
    g.w.w = W, g.w.co = Co, g.w.ci = Ci;
    g.bias = bias, g.z = z, g.stats = stats;
    return g;
}

// rows of one split-K slice of the weight gradient: ceil(R / nsplit), in whole K chunks
static int wgrad_rows_per_split(int R, int nsplit)
{
    const int rps = (R + nsplit - 1) / nsplit;
    return ((rps + BK - 1) / BK) * BK;
}

// Occupancy shaping.  The dispatcher stacks workgroups on a CU up to its resource limit before moving on, so a grid of
// 512 small workgroups can land 4-deep on half of the 256 CUs (measured: SQ_WAIT_INST_ANY 52 % of wave cycles -- four
// waves per SIMD queueing on one matrix pipe) instead of 2-deep on all of them.  Requesting 160 KB / (workgroups per CU
// the grid needs) of LDS makes exactly that many fit, which spreads the grid evenly.
static size_t shaped_lds(size_t needed, dim3 grid)
{
    const size_t nblk = (size_t)grid.x * grid.y * grid.z;
    const size_t per_cu = std::max<size_t>(1, (nblk + 255) / 256);
    const size_t want = std::min<size_t>(64 * 1024, (160 * 1024) / per_cu);
    return std::max(needed, want > 1024 ? want - 1024 : needed);
}

// ---- dispatch helpers: tile x fast-path x operand modes are template parameters (no control flow around loads) ----
#define SN_LAUNCH_T(KERN, T_, FULL_, GRID, ARGS, ...)                                                              \
    do {                                                                                                           \
        const size_t lds_ = shaped_lds(lds_bytes<T_>(), GRID);                                                     \
        if (FULL_)                                                                                                 \
            hipLaunchKernelGGL((KERN<T_, true, __VA_ARGS__>), GRID, dim3(T_::THREADS), lds_, st, ARGS);            \
        else                                                                                                       \
            hipLaunchKernelGGL((KERN<T_, false, __VA_ARGS__>), GRID, dim3(T_::THREADS), lds_, st, ARGS);           \
    } while (0)

// Mode dispatch.  A call site lists the dZ modes (ZModes) and the previous-layer modes (PModes) its kernel is built for; f is a
// generic callable that receives the pair -- and a site's extra two-way switch (vec / full) -- as integral constants, so that
// `decltype(zm)::value` is a template argument.  Only the listed product is instantiated.  A pair outside the list calls nothing:
// every site sits behind the entry's own dz_mode check or behind the route condition that excludes the pair.
template <int... Z>
struct ZModes {};
template <int... P>
struct PModes {};

template <int... P, class F>
static void dispatch_act(PModes<P...>, bool bn_prev, F &&f)
{
    const int pmode = bn_prev ? ACT_BN_RELU : ACT_NONE;
    (void)((pmode == P && (f(std::integral_constant<int, P>{}), true)) || ...);
}

template <int... Z, class PL, class F>
static void dispatch_modes(ZModes<Z...>, PL pl, int dz_mode, bool bn_prev, F &&f)
{
    (void)((dz_mode == Z && (dispatch_act(pl, bn_prev, [&](auto pm) { f(std::integral_constant<int, Z>{}, pm); }), true)) || ...);
}

template <class ZL, class PL, class F>
static void dispatch_modes(ZL zl, PL pl, int dz_mode, bool bn_prev, bool flag, F &&f)
{
    if (flag)
        dispatch_modes(zl, pl, dz_mode, bn_prev, [&](auto zm, auto pm) { f(zm, pm, std::true_type{}); });
    else
        dispatch_modes(zl, pl, dz_mode, bn_prev, [&](auto zm, auto pm) { f(zm, pm, std::false_type{}); });
}

// The FULLR = true / false twins (KT / KF) of a kernel launched with more than 64 KB of dynamic LDS: the size must be requested per
// kernel and per device first -- one SnLdsAttr per kernel instantiation (the statics of this instantiation).  A refused request
// leaves the error text under `who`; the launch below then fails and the entry point's launch check reports it.
template <auto KT, auto KF, class A>
static void launch_lds_twins(bool fullr, dim3 grid, dim3 block, size_t lds, const char *who, hipStream_t st, const A &a)
{
    static SnLdsAttr at, af;
    (void)sn_lds_attr(at, (const void *)KT, lds, who);
    (void)sn_lds_attr(af, (const void *)KF, lds, who);
    if (fullr)
        hipLaunchKernelGGL(KT, grid, block, lds, st, a);
    else
        hipLaunchKernelGGL(KF, grid, block, lds, st, a);
}

static int device_cus()
{
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            n = v;
        else
            n = 256;  // MI355X
        (void)hipGetLastError();
    }
    return n;
}
