// ubench_uniform.hip — what does a WAVE-UNIFORM dependent 64-byte fetch cost (the packet walk's node / record fetch,
// csrc/pt_walks.h trav_packet_wide), next to the per-lane gather of tools/ubench_gather.hip?
//   mode 0: per lane: every lane chases its own chain with 4 x global_load_dwordx4 (the per-lane walk; 64 items per wave step)
//   mode 1: uniform, scalar: the wave chases ONE chain; the index is readfirstlane'd and the item read through a constant
//           address-space pointer -> s_load_dwordx16 through the scalar data cache
//   mode 2: uniform, one lane: lane 0 issues the 4 x global_load_dwordx4 of the wave's item, readfirstlane broadcasts it
// Dependent chain: the next index depends on the loaded data.  Resident grid: 8 blocks of 256 per CU (8 waves per SIMD).
// Prints items/s per wave and per CU (mode 0: lane-items, modes 1-2: wave-items).
// Build: hipcc --offload-arch=gfx950 -O3 -o ubench_uniform tools/ubench_uniform.hip
// Usage: ubench_uniform <table MB> <mode> [iters]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

typedef const __attribute__((address_space(4))) float cfloat;

template <int MODE>
__global__ void __launch_bounds__(256, 8) k_uniform(const float4* __restrict__ items, uint32_t n_items, int iters, float* out) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(gid >> 6));
    float acc = 0.f;
    if (MODE == 0) {
        uint32_t idx = mix(gid * 2654435761u + 12345u) % n_items;
        for (int it = 0; it < iters; it++) {
            const float4* p = items + (size_t)idx * 4;
            const float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            acc += q0.x + q0.y + q0.z + q0.w + q1.x + q1.y + q1.z + q1.w + q2.x + q2.y + q2.z + q2.w + q3.x + q3.y + q3.z;
            idx = mix(idx ^ __float_as_uint(q3.w) ^ (uint32_t)it) % n_items;
        }
    } else {
        uint32_t idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mix(wave * 2654435761u + 12345u) % n_items));
        for (int it = 0; it < iters; it++) {
            float v[16];
            if (MODE == 1) {
                cfloat* p = (cfloat*)items + (size_t)idx * 16;
#pragma unroll
                for (int k = 0; k < 16; k++) v[k] = p[k];
            } else {
                float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0, q2 = q0, q3 = q0;
                if ((threadIdx.x & 63) == 0) {
                    uint32_t i4 = idx * 4u;
                    asm volatile("" : "+v"(i4));   // a vector index: left alone, hipcc turns the uniform load into s_load
                    const float4* p = items + i4;
                    q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3];
                }
                const float4 q[4] = {q0, q1, q2, q3};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    v[4 * k + 0] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q[k].x)));
                    v[4 * k + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q[k].y)));
                    v[4 * k + 2] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q[k].z)));
                    v[4 * k + 3] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q[k].w)));
                }
            }
#pragma unroll
            for (int k = 0; k < 15; k++) acc += v[k];
            idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(mix(idx ^ __float_as_uint(v[15]) ^ (uint32_t)it) % n_items));
        }
    }
    out[gid] = acc;
}

int main(int argc, char** argv) {
    const double mb = argc > 1 ? atof(argv[1]) : 100.0;
    const int mode = argc > 2 ? atoi(argv[2]) : 1;
    const int iters = argc > 3 ? atoi(argv[3]) : 2000;
    const uint32_t n_items = (uint32_t)(mb * 1024.0 * 1024.0 / 64.0);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int n_cu = prop.multiProcessorCount;
    const int blocks = n_cu * 8;
    float4* items = nullptr;
    float* out = nullptr;
    if (hipMalloc(&items, (size_t)n_items * 64) != hipSuccess || hipMalloc(&out, (size_t)blocks * 256 * 4) != hipSuccess) return 1;
    std::vector<float4> h((size_t)n_items * 4);
    for (size_t i = 0; i < h.size(); i++) {
        const float f = (float)((i * 2654435761u) & 0xffff) * 1e-6f;
        h[i] = make_float4(f, f, f, f);
    }
    if (hipMemcpy(items, h.data(), h.size() * 16, hipMemcpyHostToDevice) != hipSuccess) return 1;
    auto run = [&](int it) {
        if (mode == 0) hipLaunchKernelGGL(k_uniform<0>, dim3(blocks), dim3(256), 0, 0, items, n_items, it, out);
        else if (mode == 1) hipLaunchKernelGGL(k_uniform<1>, dim3(blocks), dim3(256), 0, 0, items, n_items, it, out);
        else hipLaunchKernelGGL(k_uniform<2>, dim3(blocks), dim3(256), 0, 0, items, n_items, it, out);
    };
    run(100);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    run(iters);
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess) return 1;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    const double waves = (double)blocks * 4, per_wave_items = mode == 0 ? 64.0 * iters : (double)iters;
    const double per_wave = per_wave_items / (ms * 1e-3), per_cu = per_wave * waves / n_cu;
    printf("{\"table_mb\": %.0f, \"mode\": %d, \"iters\": %d, \"ms\": %.3f, \"items_per_s_per_wave\": %.4g, \"items_per_s_per_cu\": %.4g, "
           "\"ns_per_step\": %.1f}\n", mb, mode, iters, ms, per_wave, per_cu, ms * 1e6 / iters);
    (void)hipFree(items);
    (void)hipFree(out);
    return 0;
}
