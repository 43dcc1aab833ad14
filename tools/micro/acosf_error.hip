// The error of the device's acosf against fp64, in ulps of its own result: the library term of rot_err's bound (tests/pose_ref.py
// ACOSF_ULP; sn_pose_error_forward computes 2 acosf(clamp(2 d^2 - 1))).  2^22 arguments: 2^20 uniform over [-1, 1], 2^20 at
// 1 - 2^-k u and 2^20 at -1 + 2^-k u (k = 0 .. 23, u uniform: dense at both ends, where rot_err's edge cases sit), 2^20 consecutive
// floats below 1, and the exact points -1, -0, 0, 1.  Compiled like the library's geometry files (no contraction, no fast math).
// Prints the largest error in ulps, where it occurs, and the largest absolute error.  Recorded in profiles/pose/errors.txt.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o acosf_error acosf_error.hip && ./acosf_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__global__ void __launch_bounds__(256) acos_kernel(int n, const float *__restrict__ x, float *__restrict__ y)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = acosf(x[i]);
}

static double ulp_of(float v)
{
    if (v == 0.0f) return ldexp(1.0, -149);
    int e;
    frexp((double)fabsf(v), &e);  // |v| in [2^(e-1), 2^e)
    return ldexp(1.0, (e - 1 < -126 ? -126 : e - 1) - 23);
}

int main()
{
    const int q = 1 << 20, n = 4 * q + 4;
    std::vector<float> x(n), y(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13, s ^= s >> 7, s ^= s << 17; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
    for (int i = 0; i < q; ++i) {
        x[i] = (float)(2.0 * rnd() - 1.0);
        const double t = ldexp(rnd(), -(i % 24));
        x[q + i] = (float)(1.0 - t), x[2 * q + i] = (float)(-1.0 + t);
        uint32_t one;
        const float f1 = 1.0f;
        memcpy(&one, &f1, 4);
        one -= (uint32_t)i;
        memcpy(&x[3 * q + i], &one, 4);
    }
    x[4 * q] = -1.0f, x[4 * q + 1] = -0.0f, x[4 * q + 2] = 0.0f, x[4 * q + 3] = 1.0f;
    float *dx, *dy;
    CK(hipMalloc(&dx, n * sizeof(float)));
    CK(hipMalloc(&dy, n * sizeof(float)));
    CK(hipMemcpy(dx, x.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(acos_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, dy);
    CK(hipGetLastError());
    CK(hipMemcpy(y.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0, worst_abs = 0;
    float at = 0, at_abs = 0;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        const double ref = acos((double)x[i]);
        if (!(y[i] >= 0.0f && y[i] <= 3.1415927410125732f)) ++bad;  // (float(pi) rounds above pi)
        const double err = fabs((double)y[i] - ref), u = err / ulp_of((float)ref);
        if (u > worst) worst = u, at = x[i];
        if (err > worst_abs) worst_abs = err, at_abs = x[i];
    }
    printf("acosf on %d arguments: max error %.3f ulp of the result (at x = %.9g), max absolute error %.3e (at x = %.9g), "
           "results outside [0, float(pi)]: %ld\n", n, worst, (double)at, worst_abs, (double)at_abs, bad);
    printf("acosf(1) = %.9g, acosf(-1) = %.9g, 2 acosf(-1) = %.9g\n", (double)y[4 * q + 3], (double)y[4 * q], (double)(2.0f * y[4 * q]));
    CK(hipFree(dx));
    CK(hipFree(dy));
    return bad ? 2 : 0;
}
