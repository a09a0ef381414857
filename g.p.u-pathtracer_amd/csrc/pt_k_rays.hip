// pt_k_rays.hip — pt_render_rays: the path loop over a caller's rays (other cameras, probes, baking), its fold and their launchers.
// One translation unit of libptmi.so (pt_ctx.h); the API function is ptmi.hip's.  DESIGN.md §10 f10.
//
// k_render_rays<V> is the loop of pt_rays_loop.h (k_rays_loop) started from KRays: a slot's path starts at the ray as it stands in the buffer, with
// the RNG of pixel first_index + ray behind the camera's two jitter draws, so a batch that equals a camera's rays gives that camera's
// image bit for bit.  The fold (k_fold_rays) also serves pt_render_camera (pt_k_camera.hip), whose rows it sees as a batch without rays.
// k_fold_pixels is pt_render_pixels' fold of the same sample buffer into full-frame buffers.
#include "pt_ctx.h"
#include "pt_rays_loop.h"

template <uint32_t V>
constexpr auto k_render_rays = &k_rays_loop<V, KRays>;

// Folds the launch's samples [spp][n][3] into the running mean of every ray, in sample order: one lane per ray.
template <bool HDR>
__global__ void __launch_bounds__(256) k_fold_rays(const KParams P, const KRays R) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)R.n) return;
    float* acc = R.out + 3 * i;
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (P.sample_index != 1) { ax = acc[0]; ay = acc[1]; az = acc[2]; }
    for (uint32_t s = 0; s < P.spp; s++) rays_accumulate<HDR>(ax, ay, az, pt_sld3(pt_sample_ptr(P, s, i)), P.sample_index + s);
    acc[0] = ax; acc[1] = ay; acc[2] = az;
}

// pt_render_pixels: folds the launch's samples [spp][n][3] into FULL-FRAME buffers, one lane per row.  Row i is pixel pixels[i] (or i);
// the pixel's own count c says where its running means stand, so sample s enters them with N = c + 1 + s: the accumulator through
// rays_accumulate, the luminance moments through pt_moments (k_fold_samples<MOM>'s).  A listed index past the image is skipped.  Two
// rows with the same pixel would race: the caller lists a pixel once (include/ptmi.h).
struct KPixels {
    const uint32_t* __restrict__ pixels;
    float* __restrict__ accum;
    float2* __restrict__ moments;
    uint32_t* __restrict__ counts;
    uint32_t n, n_pix;
};
template <bool HDR, bool MOMENTS>
__global__ void __launch_bounds__(256) k_fold_pixels(const KParams P, const KPixels X) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)X.n) return;
    const uint32_t pix = X.pixels ? X.pixels[i] : (uint32_t)i;
    if (pix >= X.n_pix) return;
    const uint32_t c = X.counts[pix];
    float* acc = X.accum + 3 * (size_t)pix;
    float ax = 0.f, ay = 0.f, az = 0.f, m1 = 0.f, m2 = 0.f;
    if (c != 0u) {
        ax = acc[0]; ay = acc[1]; az = acc[2];
        if constexpr (MOMENTS) { const float2 m = X.moments[pix]; m1 = m.x; m2 = m.y; }
    }
    for (uint32_t s = 0; s < P.spp; s++) {
        const v3 col = pt_sld3(pt_sample_ptr(P, s, i));
        const uint64_t N = (uint64_t)c + 1u + s;
        rays_accumulate<HDR>(ax, ay, az, col, N);
        if constexpr (MOMENTS) pt_moments(m1, m2, col, N);
    }
    acc[0] = ax; acc[1] = ay; acc[2] = az;
    if constexpr (MOMENTS) X.moments[pix] = make_float2(m1, m2);
    X.counts[pix] = c + P.spp;
}

namespace ptmi {

static KRays rays_args(const RaysCall& r) { return KRays{(const float4*)r.rays, r.out, r.first_index, (uint32_t)r.n, r.hdr}; }

// Instantiated: rays_exists; the request's word: rays_word (pt_variants.h).  A request without an instantiation (PT_FLAG_MIS without
// PT_FLAG_NEE or over Woop records) is none that pt_render_rays lets through.
hipError_t launch_render_rays(const LaunchCfg& L, const KParams& P, const RaysCall& r, hipStream_t st) {
    const KRays R = rays_args(r);
    return with_variant<rays_exists, PV_BITS>(rays_word(L), [&](auto v) {
        return launch_resident(k_render_rays<v()>, L.lds, INT_MAX, L.n_cu, (size_t)std::max(1, L.work_blocks), st, P, R);
    });
}

hipError_t launch_fold_rays(const pt_ctx* c, const KParams& P, const RaysCall& r) {
    const KRays R = rays_args(r);
    with_bool(r.hdr != 0, [&](auto hdr) {
        hipLaunchKernelGGL(k_fold_rays<hdr()>, dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, c->stream, P, R);
    });
    return hipGetLastError();
}

hipError_t launch_fold_pixels(const pt_ctx* c, const KParams& P, const PixelsCall& r) {
    const KPixels X{r.pixels, r.accum, (float2*)r.moments, r.counts, (uint32_t)r.n, r.n_pix};
    with_bool(r.hdr != 0, [&](auto hdr) {
        with_bool(r.moments != nullptr, [&](auto mom) {
            hipLaunchKernelGGL((k_fold_pixels<hdr(), mom()>), dim3((unsigned)((r.n + 255) / 256)), dim3(256), 0, c->stream, P, X);
        });
    });
    return hipGetLastError();
}

}  // namespace ptmi
