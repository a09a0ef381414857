// pt_filter.hip — pt_denoise (the edge-avoiding a-trous wavelet filter, Dammertz et al. 2010) and
// pt_denoise_variance (the same filter steered by each pixel's variance, §10 f15; include/ptmi.h states the arithmetic,
// tests/denoise_ref.py and tests/denoise_var_ref.py restate it).  One translation unit of libptmi.so (pt_ctx.h).
//   k_dn_demod       colour / albedo into ping-pong buffer A as float4 (i, hit) — the hit flag rides in .w, so a tap learns
//                    whether q is a miss from the colour load it makes anyway
//   k_dn_copy        iterations = 0: out = color bit for bit (+ display words)
//   k_dv_seed<COPY>  colour / albedo and the variance of the mean luminance from the moments into ping-pong buffer A as float4
//                    (i, v) — the hit flag rides in the SIGN BIT of v (a miss with variance 0 is -0.0f, so the flag is read as a
//                    bit, never with < 0); COPY is iterations = 0
//   k_dn_iter<LAST>, k_dv_iter<LAST>  one launch per iteration, 16x16 tiles, both atrous_pixel: 25 taps, each one dwordx4 load per
//                    buffer (colour; normal and position only where both ends are hits) and ONE v_exp_f32 (the terms folded into
//                    exp2 with log2(e) in the constants); the last iteration remodulates, clamps, writes out (+ display words).
//                    k_dv_iter adds per PIXEL, not per tap: the 3x3 pre-filter of v (eight dword loads from L1 — no LDS apron,
//                    so no barrier and the lanes outside the image still leave at once) and one division for the luminance
//                    stop 1 / (sigma_l sd + 1e-4); v travels as sum w^2 v / (sum w)^2
// No LDS tile: at step 16 the taps are 64 rows apart, an apron would re-read more than it saves; the packed buffers of a 1080p
// frame (~100 MB) stay in the 256 MB Infinity Cache.
#include <cmath>
#include <cstring>

#include "pt_image.h"

namespace {

struct DnArgs {
    const float* color;                   // [H][W][3] (out may alias it)
    const float4* __restrict__ albedo;
    const float4* __restrict__ normal;
    const float4* __restrict__ position;
    const float4* __restrict__ src;       // ping-pong (i, hit)
    float4* __restrict__ dst;
    float* out;                           // [H][W][3], may alias color
    uint32_t* rgba;                       // may be null
    int W, H;
    int step;                             // 2^l
    float kc, kn, kx;                     // log2(e) / sigma^2 of the three terms (colour: of this iteration), 0 = off
};

struct DvArgs {
    const float* color;                   // [H][W][3] (out may alias it)
    const float2* __restrict__ moments;   // [H][W] (m1, m2)
    const float* __restrict__ length;     // [H][W] frames behind the moments; null = 1
    const float4* __restrict__ albedo;
    const float4* __restrict__ normal;
    const float4* __restrict__ position;
    const float4* __restrict__ src;       // ping-pong (i, v): the sign bit of v set = the pixel is a miss
    float4* __restrict__ dst;
    float* out;                           // [H][W][3], may alias color
    float* __restrict__ out_var;          // [H][W], may be null
    uint32_t* rgba;                       // may be null
    int W, H;
    int step;                             // 2^l
    float spf;                            // samples behind one frame of the moments
    float sl;                             // sigma_luminance, 0 = off
    float kn, kx;                         // log2(e) / sigma^2 of the normal and the position term, 0 = off
};

__device__ __forceinline__ bool dv_is_miss(float v) { return (__float_as_uint(v) >> 31) != 0u; }   // -0.0f is a miss too

__global__ void __launch_bounds__(PTD_BLOCK) k_dn_demod(const DnArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 a = A.albedo[p], n = A.normal[p];
    const float* c = A.color + 3 * p;
    const bool hit = n.x != 0.f || n.y != 0.f || n.z != 0.f;
    A.dst[p] = make_float4(c[0] / ptd_demod_div(a.x), c[1] / ptd_demod_div(a.y), c[2] / ptd_demod_div(a.z), hit ? 1.f : 0.f);
}

__global__ void __launch_bounds__(PTD_BLOCK) k_dn_copy(const DnArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float r = A.color[3 * p], g = A.color[3 * p + 1], b = A.color[3 * p + 2];
    ptd_store(A.out, A.rgba, p, r, g, b);
}

// The seed: (c / a', var_p / L(a')^2) into ping-pong buffer A.  COPY (iterations = 0): out = color bit for bit, out_var = var_p.
template <bool COPY>
__global__ void __launch_bounds__(PTD_BLOCK) k_dv_seed(const DvArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float2 m = A.moments[p];
    const float n = A.spf * (A.length ? A.length[p] : 1.0f);
    const float var = fminf(fmaxf(n >= 2.0f ? fmaxf(0.f, m.y - m.x * m.x) / (n - 1.0f) : m.y, 0.f), 1e30f);   // NaN: 0
    const float r = A.color[3 * p], g = A.color[3 * p + 1], b = A.color[3 * p + 2];
    if (COPY) {
        ptd_store(A.out, A.rgba, p, r, g, b);
        if (A.out_var) A.out_var[p] = var;
    } else {
        const float4 a = A.albedo[p], nr = A.normal[p];
        const float ax = ptd_demod_div(a.x), ay = ptd_demod_div(a.y), az = ptd_demod_div(a.z);
        const float la = ptd_lum(ax, ay, az);
        const float v0 = var / (la * la);
        const bool hit = nr.x != 0.f || nr.y != 0.f || nr.z != 0.f;
        A.dst[p] = make_float4(r / ax, g / ay, b / az, hit ? v0 : __uint_as_float(__float_as_uint(v0) | 0x80000000u));
    }
}

// One pixel of one iteration, of pt_denoise (VAR 0, DnArgs) and of pt_denoise_variance (VAR 1, DvArgs).  The pixel setup, the tap
// loop, the geometric stop, the one v_exp_f32 and the remodulation are the same statements for both; VAR chooses how the hit flag
// rides in .w, the luminance stop (behind the 3x3 pre-filter of v: eight dword loads of adjacent pixels, from L1 — the step-1 taps
// of the same tile touch the same lines — and one division) in place of the colour stop, and the variance's travel into out_var.
template <bool VAR, bool LAST, class Args>
__device__ __forceinline__ void atrous_pixel(const Args& A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 cp = A.src[p];
    bool mp, hp;
    float vp = 0.f;
    if constexpr (VAR) {
        mp = dv_is_miss(cp.w);
        hp = !mp;
        vp = fabsf(cp.w);
    } else {
        hp = cp.w != 0.f;
        mp = !hp;
    }
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), xp = np;
    float kxp = 0.f;
    if (hp) {
        np = A.normal[p];
        xp = A.position[p];
        kxp = fminf(A.kx / (xp.w * xp.w), 1e30f);   // 1 / (sigma_x t_p)^2, finite
    }
    float kl = 0.f, lp = 0.f;
    if constexpr (VAR) {
        // g_p: the (1,2,1)x(1,2,1) mean of v over the adjacent pixels with p's hit flag
        float gs = 4.0f * vp, gw = 4.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const int yq = y + dy;
            if (yq < 0 || yq >= A.H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int xq = x + dx;
                if ((dx == 0 && dy == 0) || xq < 0 || xq >= A.W) continue;
                const float vq = A.src[(size_t)yq * (size_t)A.W + (size_t)xq].w;
                if (dv_is_miss(vq) != mp) continue;
                const float gk = (float)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
                gs = fmaf(gk, fabsf(vq), gs); gw += gk;
            }
        }
        const float sd = sqrtf(fmaxf(gs / gw, 0.f));
        kl = A.sl > 0.f ? 1.44269504f / fmaf(A.sl, sd, 1e-4f) : 0.f;   // log2(e) k_p
        lp = ptd_lum(cp.x, cp.y, cp.z);
    }
    const float hk[5] = {1.f / 16.f, 4.f / 16.f, 6.f / 16.f, 4.f / 16.f, 1.f / 16.f};
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int yq = y + dy * A.step;
        if (yq < 0 || yq >= A.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int xq = x + dx * A.step;
            if (xq < 0 || xq >= A.W) continue;
            const float hh = hk[dy + 2] * hk[dx + 2];
            if (dx == 0 && dy == 0) {   // the centre: e = 0
                sr = fmaf(hh, cp.x, sr); sg = fmaf(hh, cp.y, sg); sb = fmaf(hh, cp.z, sb); sw += hh;
                if constexpr (VAR) sv = fmaf(hh * hh, vp, sv);
                continue;
            }
            const size_t q = (size_t)yq * (size_t)A.W + (size_t)xq;
            const float4 cq = A.src[q];
            float e;
            if constexpr (VAR) {
                if (dv_is_miss(cq.w) != mp) continue;   // exactly one of p, q is a miss
                e = kl * fabsf(lp - ptd_lum(cq.x, cq.y, cq.z));
            } else {
                if ((cq.w != 0.f) != hp) continue;   // exactly one of p, q is a miss
                const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                e = A.kc * fmaf(db, db, fmaf(dg, dg, dr * dr));
            }
            if (hp) {
                const float4 nq = A.normal[q], xq4 = A.position[q];
                const float ax = np.x - nq.x, ay = np.y - nq.y, az = np.z - nq.z;
                const float bx = xp.x - xq4.x, by = xp.y - xq4.y, bz = xp.z - xq4.z;
                e = fmaf(A.kn, fmaf(az, az, fmaf(ay, ay, ax * ax)), e);
                e = fmaf(kxp, fmaf(bz, bz, fmaf(by, by, bx * bx)), e);
            }
            const float w = hh * __builtin_amdgcn_exp2f(-e);   // one v_exp_f32
            sr = fmaf(w, cq.x, sr); sg = fmaf(w, cq.y, sg); sb = fmaf(w, cq.z, sb); sw += w;
            if constexpr (VAR) sv = fmaf(w * w, fabsf(cq.w), sv);
        }
    }
    const float inv = 1.0f / sw;
    const float r = sr * inv, g = sg * inv, b = sb * inv;
    float v = 0.f;
    if constexpr (VAR) v = sv * (inv * inv);
    if (!LAST) {
        if constexpr (VAR) A.dst[p] = make_float4(r, g, b, mp ? __uint_as_float(__float_as_uint(v) | 0x80000000u) : v);
        else A.dst[p] = make_float4(r, g, b, cp.w);
    } else {
        const float4 a = A.albedo[p];
        const float ax = ptd_demod_div(a.x), ay = ptd_demod_div(a.y), az = ptd_demod_div(a.z);
        const float o0 = pt_clamp01(r * ax), o1 = pt_clamp01(g * ay), o2 = pt_clamp01(b * az);
        ptd_store(A.out, A.rgba, p, o0, o1, o2);
        if constexpr (VAR) {
            if (A.out_var) {
                const float la = ptd_lum(ax, ay, az);
                A.out_var[p] = v * (la * la);
            }
        }
    }
}

template <bool LAST>
__global__ void __launch_bounds__(PTD_BLOCK) k_dn_iter(const DnArgs A) {
    atrous_pixel<false, LAST>(A);
}

template <bool LAST>
__global__ void __launch_bounds__(PTD_BLOCK) k_dv_iter(const DvArgs A) {
    atrous_pixel<true, LAST>(A);
}

using namespace ptmi;

// ---- the host side both calls share
// log2(e) * scale / sigma^2, in double; a term with sigma <= 0 is off (0); capped so that 0 x constant stays 0
float k_of(double sigma, double scale = 1.0) {
    if (!(sigma > 0.0)) return 0.f;
    return (float)std::min(1.4426950408889634 * scale / (sigma * sigma), 1e30);
}

// The two ping-pong frames of n_pix pixels in the context's scratch.  PT_OK, or the error already recorded.
int filter_scratch(pt_ctx* c, size_t n_pix, float4* ping[2]) {
    if (2 * n_pix > c->d_denoise.count()) HIP_TRY(c, hipStreamSynchronize(c->stream));   // the old frames may still be read by an earlier call's launches
    HIP_TRY(c, c->d_denoise.reserve(2 * n_pix));
    ping[0] = c->d_denoise.get();
    ping[1] = ping[0] + n_pix;
    return PT_OK;
}

// The L >= 1 iterations behind the seed launch that filled ping[0]: iteration l reads ping[l & 1] at step 2^l and writes the other,
// the last one (`last`, the <true> kernel) the caller's buffers; each(A, l) sets what else an iteration has of its own.
template <class Args, class Each>
void filter_iterations(Args& A, float4* const ping[2], int L, dim3 grid, hipStream_t st, void (*mid)(Args), void (*last)(Args), Each each) {
    for (int l = 0; l < L; l++) {
        A.step = 1 << l;
        each(A, l);
        A.src = ping[l & 1];
        A.dst = ping[(l + 1) & 1];
        hipLaunchKernelGGL(l + 1 < L ? mid : last, grid, dim3(PTD_BLOCK), 0, st, A);
    }
}

}  // namespace

extern "C" int pt_denoise(pt_ctx* c, const pt_denoise_params* dp, const float* color_dev, const float* albedo_dev,
                          const float* normal_dev, const float* position_dev, float* out_dev, uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const Refusal r = check_denoise_call(dp, color_dev && albedo_dev && normal_dev && position_dev && out_dev);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    DnArgs A;
    std::memset(&A, 0, sizeof A);
    A.color = color_dev;
    A.albedo = (const float4*)albedo_dev;
    A.normal = (const float4*)normal_dev;
    A.position = (const float4*)position_dev;
    A.out = out_dev;
    A.rgba = rgba_dev;
    A.W = dp->width; A.H = dp->height;
    const dim3 grid = ptd_grid(dp->width, dp->height);
    const int L = dp->iterations;
    float4* ping[2] = {nullptr, nullptr};
    if (L > 0)
        if (int rc = filter_scratch(c, (size_t)dp->width * (size_t)dp->height, ping)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (L == 0) {
        hipLaunchKernelGGL(k_dn_copy, grid, dim3(PTD_BLOCK), 0, st, A);
    } else {
        A.dst = ping[0];
        hipLaunchKernelGGL(k_dn_demod, grid, dim3(PTD_BLOCK), 0, st, A);
        A.kn = k_of(dp->sigma_normal);
        A.kx = k_of(dp->sigma_position);
        filter_iterations(A, ping, L, grid, st, k_dn_iter<false>, k_dn_iter<true>, [dp](DnArgs& a, int l) {
            a.kc = k_of(dp->sigma_color, std::ldexp(1.0, 2 * l));   // (sigma_c 2^-l)^2 = sigma_c^2 / 4^l
        });
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_denoise_variance(pt_ctx* c, const pt_denoise_variance_params* dp, const float* color_dev, const float* moments_dev,
                                   const float* length_dev, const float* albedo_dev, const float* normal_dev, const float* position_dev,
                                   float* out_dev, float* out_variance_dev, uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const Refusal r = check_denoise_variance_call(dp, {color_dev, moments_dev, length_dev, albedo_dev, normal_dev, position_dev, out_dev, out_variance_dev});   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    DvArgs A;
    std::memset(&A, 0, sizeof A);
    A.color = color_dev;
    A.moments = (const float2*)moments_dev;
    A.length = length_dev;
    A.albedo = (const float4*)albedo_dev;
    A.normal = (const float4*)normal_dev;
    A.position = (const float4*)position_dev;
    A.out = out_dev;
    A.out_var = out_variance_dev;
    A.rgba = rgba_dev;
    A.W = dp->width; A.H = dp->height;
    A.spf = dp->samples_per_frame;
    const dim3 grid = ptd_grid(dp->width, dp->height);
    const int L = dp->iterations;
    float4* ping[2] = {nullptr, nullptr};
    if (L > 0)   // pt_denoise's scratch, by its rule
        if (int rc = filter_scratch(c, (size_t)dp->width * (size_t)dp->height, ping)) return rc;
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (L == 0) {
        hipLaunchKernelGGL(k_dv_seed<true>, grid, dim3(PTD_BLOCK), 0, st, A);
    } else {
        A.dst = ping[0];
        hipLaunchKernelGGL(k_dv_seed<false>, grid, dim3(PTD_BLOCK), 0, st, A);
        A.sl = dp->sigma_luminance > 0.f ? fminf(dp->sigma_luminance, 1e30f) : 0.f;
        A.kn = k_of(dp->sigma_normal);
        A.kx = k_of(dp->sigma_position);
        filter_iterations(A, ping, L, grid, st, k_dv_iter<false>, k_dv_iter<true>, [](DvArgs&, int) {});
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
