// The error of the device's expf and logf against fp64, in ulps of their own results, over the arguments sn_classification_terms_*
// (samplenet_amd/csrc/cls_terms.hip) can hand them: the library terms of tests/cls_terms_ref.py's bounds (ULPS).
//   expf(x - m), x - m <= 0:  2^20 uniform over [-104, 0] (below about -103.97 the result is zero), 2^20 at -2^-k u (k = 0 .. 23: dense at
//                             zero, where the terms that carry the sum sit), 2^20 uniform over [-20, 0], and the exact points 0, -0.
//   logf(s), 1 <= s <= C:     2^20 uniform over [1, 1024], 2^20 at 1 + 2^-k u (dense at one: a row dominated by one class), 2^20 uniform
//                             over [1, 2^20], the 2^20 consecutive floats from 1 upwards, and the exact points 1, 2, 1024.
// Compiled like cls_terms.hip (no contraction, no fast math).  Prints the largest error in ulps and where.  Recorded in
// profiles/eval/errors.txt.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o cls_math_error cls_math_error.hip && ./cls_math_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__global__ void __launch_bounds__(256) math_kernel(int n, int which, const float *__restrict__ x, float *__restrict__ y)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = which ? logf(x[i]) : expf(x[i]);
}

static double ulp_of(double v)
{
    if (v == 0.0) return ldexp(1.0, -149);
    int e;
    frexp(fabs(v), &e);  // |v| in [2^(e-1), 2^e)
    return ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
}

static int sweep(const char *name, int which, const std::vector<float> &x)
{
    const int n = (int)x.size();
    std::vector<float> y(n);
    float *dx, *dy;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&dy, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, which, dx, dy);
    CK(hipGetLastError());
    CK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0, worst_abs = 0;
    float at = 0;
    for (int i = 0; i < n; ++i) {
        const double ref = which ? log((double)x[i]) : exp((double)x[i]);
        const double err = fabs((double)y[i] - ref), u = err / ulp_of(ref);
        if (u > worst) worst = u, at = x[i];
        if (err > worst_abs) worst_abs = err;
    }
    printf("%s on %d arguments: max error %.3f ulp of the result (at x = %.9g), max absolute error %.3e\n", name, n, worst, (double)at,
           worst_abs);
    CK(hipFree(dx));
    CK(hipFree(dy));
    return 0;
}

int main()
{
    const int q = 1 << 20;
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13, s ^= s >> 7, s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
    std::vector<float> xe(3 * q + 2), xl(4 * q + 3);
    for (int i = 0; i < q; ++i) {
        xe[i] = (float)(-104.0 * rnd());
        xe[q + i] = (float)(-ldexp(rnd(), -(i % 24)));
        xe[2 * q + i] = (float)(-20.0 * rnd());
        xl[i] = (float)(1.0 + 1023.0 * rnd());
        xl[q + i] = (float)(1.0 + ldexp(rnd(), -(i % 24)));
        xl[2 * q + i] = (float)(1.0 + 1048575.0 * rnd());
        uint32_t one;
        const float f1 = 1.0f;
        memcpy(&one, &f1, 4);
        one += (uint32_t)i;
        memcpy(&xl[3 * q + i], &one, 4);
    }
    xe[3 * q] = 0.0f, xe[3 * q + 1] = -0.0f;
    xl[4 * q] = 1.0f, xl[4 * q + 1] = 2.0f, xl[4 * q + 2] = 1024.0f;
    if (sweep("expf", 0, xe)) return 1;
    if (sweep("logf", 1, xl)) return 1;
    return 0;
}
