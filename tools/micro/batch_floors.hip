// batch_floors.hip -- worst error of the device's logf, sqrtf and sincosf over EVERY input sn_batch_assemble's draws can hand them
// (csrc/batch_assemble.hip: gauss2 and the rotation angle), against the fp64 functions, in ulps of the true result (1 ulp = 2^-23 |true|).
// The sweep is exhaustive (2^24 inputs each), so the figures are exact for this library build.  tools/batch_floors.py builds and runs it:
//     hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/micro/batch_floors.hip -o tools/micro/batch_floors
//   logf     x = (k + 1) 2^-24, k = 0 .. 2^24 - 1                         (u1 of gauss2)
//   sqrtf    x = -2 logf((k + 1) 2^-24)                                   (the radius' argument, as the kernel forms it)
//   sincosf  x = 6.28318530717958647692f * (k 2^-24)                      (gauss2's angle; the rotation angle is the same product)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

constexpr int kBlocks = 1 << 16, kThreads = 256;  // 2^24 threads

__device__ float ulps(float got, double want)
{
    if (want == 0.0) return got == 0.f ? 0.f : INFINITY;
    return (float)(fabs((double)got - want) / (fabs(want) * 0x1p-23));
}

__global__ __launch_bounds__(kThreads) void sweep(float *out)
{
    __shared__ float s[3][kThreads];
    const unsigned k = blockIdx.x * kThreads + threadIdx.x;
    const float u1 = (float)(k + 1u) * 0x1p-24f, u2 = (float)k * 0x1p-24f;
    const float lg = logf(u1), arg = -2.0f * lg, ang = 6.28318530717958647692f * u2;
    float sn, cs;
    sincosf(ang, &sn, &cs);
    s[0][threadIdx.x] = ulps(lg, log((double)u1));
    s[1][threadIdx.x] = ulps(sqrtf(arg), sqrt((double)arg));
    s[2][threadIdx.x] = fmaxf(ulps(sn, sin((double)ang)), ulps(cs, cos((double)ang)));
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int f = 0; f < 3; ++f) s[f][threadIdx.x] = fmaxf(s[f][threadIdx.x], s[f][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x * kBlocks + blockIdx.x] = s[threadIdx.x][0];
}

int main()
{
    float *d = nullptr;
    if (hipMalloc(&d, 3 * kBlocks * sizeof(float)) != hipSuccess) return 1;
    sweep<<<kBlocks, kThreads>>>(d);
    std::vector<float> h(3 * kBlocks);
    if (hipMemcpy(h.data(), d, h.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    const char *names[3] = {"logf", "sqrtf", "sincosf"};
    for (int f = 0; f < 3; ++f) {
        float worst = 0.f;
        for (int b = 0; b < kBlocks; ++b) worst = fmaxf(worst, h[f * kBlocks + b]);
        printf("%s %.6f\n", names[f], worst);
    }
    hipFree(d);
    return 0;
}
