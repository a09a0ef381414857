// pt_k_mega.hip — the megakernel family (one wave per 8x8 tile, bounce by bounce) and the explicit
// ray-batch kernel, with their launchers.  One translation unit of libptmi.so (pt_ctx.h).
#include "pt_ctx.h"

// trace<<<>>>, tracer.cu:343-400: one lane per pixel, one wave per 8x8 tile, `spp`
// consecutive samples folded in registers.
// OCC = waves per SIMD the register allocator must leave room for (4 / 6 / 8)
// ALG = 0 while-while walk (Aila-Laine), 1 unified-step walk, 2 wide (4-way quantised) walk,
//       3 wide walk over Woop records
// MIS = the shadow rays and bounce rays of PT_FLAG_NEE weighed against each other (PT_FLAG_MIS, path_shade_hit)
// V: the word of pt_variants.h (PV_*; mega_exists: what is instantiated)
template <bool COUNT, uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK, pv_occ(V)) k_trace_mega_bvh2(const KParams P) {
    static_assert(COUNT == pv_count(V), "COUNT repeats the word's bit");
    constexpr int LSTK = pv_lstk(V), ALG = pv_alg(V), ENV = pv_env(V);
    constexpr bool MIS = pv_mis(V);
    float4* s_top = s_dyn;
    lds_load_top<PT_BLOCK>(P.sc, s_top);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    int tile = blockIdx.x * (PT_BLOCK / 64) + (tid >> 6);
    uint32_t s_only = 0;
    if (P.samples) {  // one wave per (sample, tile)
        s_only = (uint32_t)(tile / P.n_tiles);
        tile -= (int)s_only * P.n_tiles;
        if (s_only >= P.spp) return;
    }
    int tx, ty;
    if (!pt_tile_coords(P, tile, tx, ty)) return;
    const int px = tx * PT_TILE + (lane & 7), py = ty * PT_TILE + (lane >> 3);
    if (px >= P.W || py >= P.H) return;  // tracer.cu:358
    const uint64_t pix = (uint64_t)py * (uint64_t)P.W + (uint64_t)px;
    TravOverflow<LSTK> stk_ovf;
    TravStack<LSTK, PT_BLOCK> stk(__builtin_amdgcn_readfirstlane(16 * P.sc.n_top + (tid & ~63)), stk_ovf);

    TravCount tc;
    uint32_t n_rays = 0, n_hits = 0;

    uint32_t n_done = P.spp;
    if (P.samples) {
        const v3 col = pt_get_sample<COUNT, ALG, ENV, MIS>(P, px, py, pix, P.frame + s_only, stk, s_top, tc, n_rays, n_hits);
        float* dst = pt_sample_ptr(P, (uint32_t)s_only, (size_t)pix);
        dst[0] = col.x; dst[1] = col.y; dst[2] = col.z;
        n_done = 1;
    } else {
        float* acc = P.accum + 3 * pix;
        float ax = 0.f, ay = 0.f, az = 0.f;
        if (P.sample_index != 1) { ax = acc[0]; ay = acc[1]; az = acc[2]; }
        for (uint32_t s = 0; s < P.spp; s++) {
            const v3 col = pt_get_sample<COUNT, ALG, ENV, MIS>(P, px, py, pix, P.frame + s, stk, s_top, tc, n_rays, n_hits);
            pt_accumulate(ax, ay, az, col, P.sample_index + s);
        }
        acc[0] = ax; acc[1] = ay; acc[2] = az;
        if ((P.flags & PT_FLAG_WRITE_RGBA) && P.rgba) P.rgba[pix] = pt_pack_rgba(ax, ay, az);
    }
    if (COUNT) {
        const bool booker = __ffsll((long long)__ballot(1)) - 1 == lane;
        const uint32_t e = wave_sum_u32(n_hits), f = wave_sum_u32(n_done);
        pt_book_walk<false>(P, booker, n_rays, tc);   // (no wave statistics: they are the persistent walks')
        if (booker) {
            atomicAdd(&P.counters[PT_CNT_HITS], (unsigned long long)e);
            atomicAdd(&P.counters[PT_CNT_PATHS], (unsigned long long)f);
        }
    }
}

// Closest-hit on an explicit ray batch (pt_trace_rays): rows a5–a7 in isolation.
__global__ void __launch_bounds__(PT_BLOCK_RAYS) k_trace_rays_bvh2(const KScene sc, const float4* __restrict__ rays, size_t n,
                                                                   int cull, float* __restrict__ t_out,
                                                                   int* __restrict__ tri_out, float* __restrict__ n_out) {
    float4* s_top = s_dyn;
    lds_load_top<PT_BLOCK_RAYS>(sc, s_top);
    const size_t i = (size_t)blockIdx.x * PT_BLOCK_RAYS + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    TravCount tc;
    TravOverflow<PT_STACK_CAP> stk_ovf;
    TravStack<PT_STACK_CAP, PT_BLOCK_RAYS> stk(__builtin_amdgcn_readfirstlane(16 * sc.n_top + ((int)threadIdx.x & ~63)), stk_ovf);
    const Hit h = trav_bvh2<TW_TOP>(sc, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), cull != 0, stk, tc, s_top);
    t_out[i] = h.t;
    tri_out[i] = h.tri;
    if (n_out) {
        const v3 hn = h.tri != -1 ? pt_hit_normal(sc, h) : V3(0.f, 0.f, 0.f);
        n_out[3 * i] = hn.x; n_out[3 * i + 1] = hn.y; n_out[3 * i + 2] = hn.z;
    }
}

namespace ptmi {

// Instantiated: mega_exists; the request's word: mega_word (pt_variants.h).
hipError_t launch_mega(const LaunchCfg& L, const KParams& P, hipStream_t st) {
    return with_variant<mega_exists, PV_BITS>(mega_word(L), [&](auto v) {
        const auto kernel = k_trace_mega_bvh2<pv_count(v()), v()>;
        const hipError_t e = allow_lds(kernel, L.lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(PT_BLOCK), L.lds, st, P);
        return hipGetLastError();
    });
}

hipError_t launch_rays(const KScene& sc, size_t lds, const float4* rays, size_t n, int cull, float* t_out, int* tri_out,
                       float* n_out, hipStream_t st) {
    hipError_t e = allow_lds(k_trace_rays_bvh2, lds);
    if (e != hipSuccess) return e;
    const int blocks = (int)((n + PT_BLOCK_RAYS - 1) / PT_BLOCK_RAYS);
    hipLaunchKernelGGL(k_trace_rays_bvh2, dim3(blocks), dim3(PT_BLOCK_RAYS), lds, st, sc, rays, n, cull, t_out, tri_out, n_out);
    return hipGetLastError();
}

}  // namespace ptmi
