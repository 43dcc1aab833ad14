// fps_select.h -- which farthest-point sampling variant sn_furthest_point_sample runs for a shape.  sampling.hip launches it;
// sn_workspace_bytes (capi_common.cpp) sizes the streaming path's temp from the same rule without linking the kernels.
#pragma once

namespace sn {

constexpr int kFpsWaveMaxN = 64 * 32;     // (a) one wave per cloud: 32 points per lane
constexpr int kFpsGroupMaxN = 1024 * 16;  // (b) one workgroup per cloud: 1024 threads x 16 points
// Auto: (a) while a lane holds few points or the clouds alone fill every SIMD, else (b) while the cloud fits in one
// workgroup's registers, else (c).  Thresholds from profiles/fps/fps_bench.txt.
constexpr int kFpsWaveAutoMaxN = 256;
constexpr int kFpsWaveAutoMinB = 1024;

extern int g_fps_variant;  // 0 = auto, 1 / 2 / 3 = force (a) / (b) / (c): sn_fps_set_variant (capi_common.cpp)

inline bool fps_fits(int v, int N)
{
    return v == 3 || (v == 1 && N <= kFpsWaveMaxN) || (v == 2 && N <= kFpsGroupMaxN);
}

// 1 / 2 / 3 = (a) / (b) / (c); 0 = the forced variant cannot take N
inline int fps_choose(int B, int N)
{
    if (g_fps_variant) return fps_fits(g_fps_variant, N) ? g_fps_variant : 0;
    if (N <= kFpsWaveMaxN && (N <= kFpsWaveAutoMaxN || B >= kFpsWaveAutoMinB)) return 1;
    if (N <= kFpsGroupMaxN) return 2;
    return 3;
}

}  // namespace sn
