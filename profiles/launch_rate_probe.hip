// launch_rate_probe.hip -- how long a launch of EMPTY workgroups takes, by grid, workgroup size and LDS per workgroup: what the
// dispatcher alone costs a kernel made of many small workgroups (realign_kernel: 12 232 one-wave workgroups of 6 352 B of LDS;
// triage_classify_kernel: 1 172 workgroups of 256 lanes and 25 756 B).  Smallest of 20 launches, HIP events.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 profiles/launch_rate_probe.hip -o launch_rate_probe && ./launch_rate_probe
#include <hip/hip_runtime.h>
#include <cstdio>

#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// touches its LDS so that the allocation is real; writes nothing to memory unless out is set (it never is)
__global__ void empty_kernel(int* out)
{
    extern __shared__ int lds[];
    lds[threadIdx.x] = (int)blockIdx.x;
    if (out) out[0] = lds[threadIdx.x ^ 1];
}

int main()
{
    hipStream_t st; TRY(hipStreamCreate(&st));
    hipEvent_t a, b; TRY(hipEventCreate(&a)); TRY(hipEventCreate(&b));
    const int grids[] = { 1172, 4688, 12232, 73153 };
    const int shapes[][2] = { { 64, 256 }, { 64, 6400 }, { 64, 25756 }, { 256, 1024 }, { 256, 25756 } };
    printf("lanes  lds_B   grid   us_per_launch  ns_per_workgroup\n");
    for (auto& sh : shapes) {
        TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(empty_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, sh[1]));
        for (int g : grids) {
            float best = 1e30f;
            for (int rep = 0; rep < 20; rep++) {
                TRY(hipEventRecord(a, st));
                hipLaunchKernelGGL(empty_kernel, dim3(g), dim3(sh[0]), sh[1], st, nullptr);
                TRY(hipEventRecord(b, st));
                TRY(hipEventSynchronize(b));
                float ms = 0; TRY(hipEventElapsedTime(&ms, a, b));
                if (ms < best) best = ms;
            }
            printf("%5d  %5d  %5d  %13.1f  %16.2f\n", sh[0], sh[1], g, best * 1e3f, best * 1e6f / g);
        }
    }
    return 0;
}
