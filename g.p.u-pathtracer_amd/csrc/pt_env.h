// pt_env.h — the environment map of pt_upload_environment: what a path that leaves the scene gathers instead of bk_color, and what
// pt_eval_environment answers for a caller's rays.  One lookup for both (include/ptmi.h states it): the kernels
// that shade in the lane that walked call it from path_shade_hit's miss branch (pt_shade.h), k_eval_environment (pt_env.hip) for
// every ray of a batch.  Included by pt_kernels.h in front of KParams (KEnv is its last member) and by pt_shade.h.
// A map uploaded under PT_OPT_ENV_LIGHT carries a sampling distribution too: pt_env_draw turns two uniform
// numbers into a direction and its density, pt_env_pdf answers the density of a given direction — path_shade_hit's NEE branch and
// the batch kernels of pt_sample_environment / pt_environment_pdf (pt_env.hip) share them.
#pragma once
#include "pt_math.h"

// The map as the kernels see it.  texels: float4[H][W] = (r, g, b, 0), scaled at upload; nullptr = no map (bk_color).
// kx = W / 2pi, ky = H / pi, hx = W / 2, hy = H / 2: computed on the host in double, rounded once.
struct KEnv {
    const float4* __restrict__ texels;
    int W, H;
    float front[3], right[3], up[3];
    float kx, ky, hx, hy;
    int filter;   // PT_ENV_NEAREST 0, PT_ENV_BILINEAR 1
    int _pad;
    // PT_OPT_ENV_LIGHT: the distribution the map is sampled by as a light, built on the host at upload (include/ptmi.h states the
    // rule); nullptr = the map is no light.  cx: float[H][W + 1], per row the CDF over the columns; cy: float[H + 1], the CDF over
    // the rows; zs: float[H + 1], sin(latitude) of the row edges.  One allocation, cx its start.
    const float* __restrict__ cx;
    const float* __restrict__ cy;
    const float* __restrict__ zs;
};

__device__ __forceinline__ bool pt_env_finite(float v) { return fabsf(v) <= PT_F32_MAX; }   // false for a NaN

// p + w * (q - p) per component: plain * and +, so that p == q gives p whatever w is
__device__ __forceinline__ v3 pt_env_lerp(float4 p, float4 q, float w) {
    return V3(p.x + w * (q.x - p.x), p.y + w * (q.y - p.y), p.z + w * (q.z - p.z));
}

// The radiance the map sends along direction d (any length).  binary32, plain * and +; the only fused operations are vdot's.
// E lives in a kernel-argument block (constant address space: PT_KARGS in the path kernels, the first argument of
// k_eval_environment), so its fields are fetched here, by the waves that get here and by no other.
// __noinline__: inlined, atan2f's registers are added to the path kernels' shading code and the persistent kernel spills four
// times as many VGPRs at 6 waves per SIMD, as a call three times as many (profiles/r14_environment.txt).  Either way only in the
// ENV instantiations of those kernels, which a context without a map never launches.
typedef const __attribute__((address_space(4))) KEnv pt_kenv;
static __device__ __noinline__ v3 pt_env_lookup(pt_kenv& E, v3 d) {
    // 1. the direction in the map's frame
    const float a = vdot(d, V3(E.front[0], E.front[1], E.front[2]));
    const float b = vdot(d, V3(E.right[0], E.right[1], E.right[2]));
    const float c = vdot(d, V3(E.up[0], E.up[1], E.up[2]));
    if (!(pt_env_finite(a) && pt_env_finite(b) && pt_env_finite(c)) || (a == 0.0f && b == 0.0f && c == 0.0f)) return V3(0.f, 0.f, 0.f);
    // 2. longitude from front towards right, latitude towards up: both independent of |d|
    const float lon = atan2f(b, a);
    const float lat = atan2f(c, sqrtf(a * a + b * b));
    // 3. texel coordinates: an integer fx, fy is a texel (the inverse of the latitude-longitude ray generation)
    const float fx = lon * E.kx + E.hx;
    const float fy = lat * E.ky + E.hy;
    const int W = E.W, H = E.H;
    const float4* tex = E.texels;
    // columns wrap (fx lies in 0 .. W up to rounding: one step either way is all a wrap ever needs), rows clamp; the min / max
    // behind the wrap keeps every index inside the map whatever fx is
    auto col = [&](float x) {
        int i = (int)x;
        if (i >= W) i -= W;
        if (i < 0) i += W;
        return (size_t)min(max(i, 0), W - 1);
    };
    auto row = [&](float y) { return (size_t)min(max((int)y, 0), H - 1); };
    if (E.filter == 0) {   // 4. PT_ENV_NEAREST
        const float4 t = tex[row(floorf(fy + 0.5f)) * (size_t)W + col(floorf(fx + 0.5f))];
        return V3(t.x, t.y, t.z);
    }
    // 5. PT_ENV_BILINEAR: the columns within each row first, then the two rows
    const float x0 = floorf(fx), wx = fx - x0;
    const float y0 = floorf(fy), wy = fy - y0;
    const size_t c0 = col(x0), c1 = col(x0 + 1.0f);
    const size_t r0 = row(y0) * (size_t)W, r1 = row(y0 + 1.0f) * (size_t)W;
    const float4 t00 = tex[r0 + c0], t01 = tex[r0 + c1], t10 = tex[r1 + c0], t11 = tex[r1 + c1];
    const v3 lo = pt_env_lerp(t00, t01, wx), hi = pt_env_lerp(t10, t11, wx);
    return V3(lo.x + wy * (hi.x - lo.x), lo.y + wy * (hi.y - lo.y), lo.z + wy * (hi.z - lo.z));
}

// ---- the map as a light (PT_OPT_ENV_LIGHT).  binary32, plain * and +.

// the largest i in 0 .. n - 1 with cdf[i] <= u (cdf[0] = 0 <= u): an entry of zero width is never the answer
__device__ __forceinline__ int pt_env_search(const float* __restrict__ cdf, int n, float u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cdf[mid] <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the density per steradian of texel (x, y), constant over it: from the CDF differences, so that it is the density of what
// pt_env_draw draws whatever the rounding of the tables.  A texel that is never drawn has density 0 (a row near a pole of a tall
// map can have dz == 0 in binary32; its py is 0 then as well)
__device__ __forceinline__ float pt_env_texel_pdf(float py, float px, float kx, float dz) {
    const float p = py * px;
    return p > 0.0f ? (p * kx) / dz : 0.0f;
}

// (u1, u2) in [0, 1) -> (direction, density): the row by u1, the column within it by u2, a point uniform in solid angle inside
// the texel.  Only called for a map with tables (E.cx != nullptr).  __noinline__ for pt_env_lookup's reason.
static __device__ __noinline__ float4 pt_env_draw(pt_kenv& E, float u1, float u2) {
    const int W = E.W, H = E.H;
    const float* cy = E.cy;
    const float* zs = E.zs;
    const int y = pt_env_search(cy, H, u1);
    const float cy0 = cy[y], py = cy[y + 1] - cy0;
    const float v1 = fminf((u1 - cy0) / py, 0x1.fffffep-1f);
    const float* cx = E.cx + (size_t)y * (size_t)(W + 1);
    const int x = pt_env_search(cx, W, u2);
    const float cx0 = cx[x], px = cx[x + 1] - cx0;
    const float v2 = fminf((u2 - cx0) / px, 0x1.fffffep-1f);
    const float z0 = zs[y], dz = zs[y + 1] - z0;
    const float z = z0 + v1 * dz;
    const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
    const float lon = ((((float)x - 0.5f) + v2) - E.hx) / E.kx;
    const float cl = r * cosf(lon), sl = r * sinf(lon);
    float4 o;
    o.x = (E.front[0] * cl + E.right[0] * sl) + E.up[0] * z;
    o.y = (E.front[1] * cl + E.right[1] * sl) + E.up[1] * z;
    o.z = (E.front[2] * cl + E.right[2] * sl) + E.up[2] * z;
    o.w = pt_env_texel_pdf(py, px, E.kx, dz);
    return o;
}

// the density pt_env_draw has along direction d (any length): the texel a nearest lookup of d picks, the same formula; 0 for a
// direction the lookup calls invalid.  Only called for a map with tables.
static __device__ __noinline__ float pt_env_pdf(pt_kenv& E, v3 d) {
    const float a = vdot(d, V3(E.front[0], E.front[1], E.front[2]));
    const float b = vdot(d, V3(E.right[0], E.right[1], E.right[2]));
    const float c = vdot(d, V3(E.up[0], E.up[1], E.up[2]));
    if (!(pt_env_finite(a) && pt_env_finite(b) && pt_env_finite(c)) || (a == 0.0f && b == 0.0f && c == 0.0f)) return 0.0f;
    const float lon = atan2f(b, a);
    const float lat = atan2f(c, sqrtf(a * a + b * b));
    const float fx = lon * E.kx + E.hx;
    const float fy = lat * E.ky + E.hy;
    const int W = E.W, H = E.H;
    int x = (int)floorf(fx + 0.5f);
    if (x >= W) x -= W;
    if (x < 0) x += W;
    x = min(max(x, 0), W - 1);
    const int y = min(max((int)floorf(fy + 0.5f), 0), H - 1);
    const float* cx = E.cx + (size_t)y * (size_t)(W + 1);
    return pt_env_texel_pdf(E.cy[y + 1] - E.cy[y], cx[x + 1] - cx[x], E.kx, E.zs[y + 1] - E.zs[y]);
}
