// pt_env.hip — the environment map on the context: pt_upload_environment, pt_eval_environment and its kernel; the map as a light
// (PT_OPT_ENV_LIGHT): the sampling tables built at upload, pt_sample_environment, pt_environment_pdf and their kernels.
// One translation unit of libptmi.so (pt_ctx.h).  The lookup, the draw and the density are pt_env.h's, shared with the path kernels.
// DESIGN.md §10 f11, f12.
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_ctx.h"

static_assert(sizeof(pt_environment) == 64, "ABI struct size (tests/test_environment.py)");

// One thread per ray: the lookup along words 4-6 of the ray.  KEnv is the FIRST argument, so that it is read where the path kernels
// read theirs: in the kernel-argument block, through the constant address space.
__global__ void __launch_bounds__(256) k_eval_environment(const KEnv E_arg, const float4* __restrict__ rays, uint32_t n, float* __restrict__ out) {
    pt_kenv& E = *(pt_kenv*)__builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const float4 b = rays[2 * i + 1];
    const v3 r = pt_env_lookup(E, V3(b.x, b.y, b.z));
    out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}

// One thread per draw: (u1, u2) clamped into [0, 1) -> (direction, density), and the lookup along it when the caller wants it.
__global__ void __launch_bounds__(256) k_sample_environment(const KEnv E_arg, const float2* __restrict__ u, uint32_t n, float4* __restrict__ out,
                                                            float* __restrict__ rad) {
    pt_kenv& E = *(pt_kenv*)__builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const float2 v = u[i];
    // fmaxf / fminf return the other operand for a NaN: a NaN becomes 0
    const float4 s = pt_env_draw(E, fminf(fmaxf(v.x, 0.0f), 0x1.fffffep-1f), fminf(fmaxf(v.y, 0.0f), 0x1.fffffep-1f));
    out[i] = s;
    if (rad) {
        const v3 r = pt_env_lookup(E, V3(s.x, s.y, s.z));
        rad[3 * i] = r.x; rad[3 * i + 1] = r.y; rad[3 * i + 2] = r.z;
    }
}

// One thread per ray: the density the draw has along words 4-6 of the ray.
__global__ void __launch_bounds__(256) k_environment_pdf(const KEnv E_arg, const float4* __restrict__ rays, uint32_t n, float* __restrict__ out) {
    pt_kenv& E = *(pt_kenv*)__builtin_amdgcn_kernarg_segment_ptr();
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const float4 b = rays[2 * i + 1];
    out[i] = pt_env_pdf(E, V3(b.x, b.y, b.z));
}

namespace ptmi {

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// PT_OPT_ENV_LIGHT: the sampling tables of a map (include/ptmi.h states the rule; tests/env_light_ref.py restates it), in double,
// every sum sequential in ascending index.  tab = cx [H][W + 1], cy [H + 1], zs [H + 1].  false: the map is no light — its basis
// is not orthonormal (the draw's inverse mapping assumes it) or it is black.
static bool env_tables(const pt_environment* env, const std::vector<float4>& t, std::vector<float>& tab) {
    const float* basis[3] = {env->front, env->right, env->up};
    for (int i = 0; i < 3; i++) {
        const double x = basis[i][0], y = basis[i][1], z = basis[i][2];
        if (!(std::fabs(std::sqrt(x * x + y * y + z * z) - 1.0) <= 1e-4)) return false;
        const float* o = basis[(i + 1) % 3];
        if (!(std::fabs(x * (double)o[0] + y * (double)o[1] + z * (double)o[2]) <= 1e-4)) return false;
    }
    const size_t W = (size_t)env->width, H = (size_t)env->height;
    const bool wide = env->filter == PT_ENV_BILINEAR;
    auto m1 = [&](size_t y, size_t x) {
        const float4 p = t[y * W + x];
        return std::max(p.x, std::max(p.y, p.z));
    };
    // a bilinear lookup inside a texel's cell reads its neighbours too (columns wrap, rows clamp): the density is positive
    // wherever the lookup can be
    auto weight = [&](size_t y, size_t x) {
        if (!wide) return (double)m1(y, x);
        const size_t ys[3] = {y > 0 ? y - 1 : 0, y, y + 1 < H ? y + 1 : H - 1}, xs[3] = {(x + W - 1) % W, x, (x + 1) % W};
        float m = 0.0f;
        for (size_t yy : ys)
            for (size_t xx : xs) m = std::max(m, m1(yy, xx));
        return (double)m;
    };
    tab.assign(H * (W + 1) + 2 * (H + 1), 0.0f);
    float* cx = tab.data();
    float* cy = cx + H * (W + 1);
    float* zs = cy + (H + 1);
    const double pi = 3.14159265358979323846;
    for (size_t i = 1; i < H; i++) zs[i] = (float)std::sin(((double)i - 0.5 - (double)H / 2.0) * pi / (double)H);
    zs[0] = -1.0f; zs[H] = 1.0f;
    std::vector<double> row(W), A(H);
    double T = 0.0;
    for (size_t y = 0; y < H; y++) {
        double S = 0.0;
        for (size_t x = 0; x < W; x++) { row[x] = weight(y, x); S += row[x]; }
        float* c = cx + y * (W + 1);
        double part = 0.0;
        for (size_t i = 0; i < W; i++) {
            c[i] = S > 0.0 ? (float)(part / S) : (float)((double)i / (double)W);   // a row with S == 0 is never picked
            part += row[i];
        }
        c[0] = 0.0f; c[W] = 1.0f;
        A[y] = S * ((double)zs[y + 1] - (double)zs[y]);
        T += A[y];
    }
    if (!(T > 0.0)) return false;
    double part = 0.0;
    for (size_t i = 0; i < H; i++) { cy[i] = (float)(part / T); part += A[i]; }
    cy[0] = 0.0f; cy[H] = 1.0f;
    return true;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" int pt_upload_environment(pt_ctx* c, const pt_environment* env, const float* texels) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!env) {   // clear: bk_color again, and the stage-split pipeline with it
        HIP_TRY(c, quiesce(c));
        c->env = EnvMap();
        c->env_gen++;
        return PT_OK;
    }
    // the struct first: nothing of `texels` is read before the dimensions are known to be sane
    if (!texels) return fail(c, PT_ERR_INVALID, "pt_upload_environment: null texels");
    if (env->width < 1 || env->width > 16384 || env->height < 1 || env->height > 16384 || (uint64_t)env->width * (uint64_t)env->height > (1ull << 26))
        return fail(c, PT_ERR_INVALID, "pt_upload_environment: width and height must be 1..16384 with width * height <= 2^26");
    if (env->filter != PT_ENV_NEAREST && env->filter != PT_ENV_BILINEAR) return fail(c, PT_ERR_INVALID, "pt_upload_environment: filter must be PT_ENV_NEAREST or PT_ENV_BILINEAR");
    const float* basis[3] = {env->front, env->right, env->up};
    for (const float* v : basis)
        if (!finite3(v) || (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f)) return fail(c, PT_ERR_INVALID, "pt_upload_environment: front, right and up must be finite and not zero");
    if (!finite3(env->scale) || env->scale[0] < 0.0f || env->scale[1] < 0.0f || env->scale[2] < 0.0f)
        return fail(c, PT_ERR_INVALID, "pt_upload_environment: scale must be finite and not negative");
    // (r, g, b, 0) per texel, the scale folded in: texel * scale, one rounding
    const size_t n = (size_t)env->width * (size_t)env->height;
    std::vector<float4> host(n);
    for (size_t i = 0; i < n; i++) {
        const float r = texels[3 * i] * env->scale[0], g = texels[3 * i + 1] * env->scale[1], b = texels[3 * i + 2] * env->scale[2];
        if (!(std::isfinite(r) && std::isfinite(g) && std::isfinite(b)) || r < 0.0f || g < 0.0f || b < 0.0f)
            return fail(c, PT_ERR_INVALID, "pt_upload_environment: a texel is not finite or is negative after scaling");
        host[i] = make_float4(r, g, b, 0.0f);
    }
    std::vector<float> tab;   // PT_OPT_ENV_LIGHT: stays empty when the map is no light
    if (c->opt_env_light && !env_tables(env, host, tab)) tab.clear();
    // the new map is complete before anything of the old one is touched: any failure up to the adoption leaves the old map, and its
    // tables, in place
    EnvMap m;
    HIP_TRY(c, m.d_texels.alloc(n));
    HIP_TRY(c, hipMemcpy(m.d_texels.get(), host.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(c, m.d_tables.alloc(tab.size()));
    if (!tab.empty()) HIP_TRY(c, hipMemcpy(m.d_tables.get(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    KEnv& k = m.k;
    k.texels = m.d_texels.get();
    if (const float* dev_tab = m.d_tables.get()) {
        const size_t W = (size_t)env->width, H = (size_t)env->height;
        k.cx = dev_tab; k.cy = dev_tab + H * (W + 1); k.zs = dev_tab + H * (W + 1) + (H + 1);
    }
    k.W = env->width; k.H = env->height;
    for (int i = 0; i < 3; i++) { k.front[i] = env->front[i]; k.right[i] = env->right[i]; k.up[i] = env->up[i]; }
    const double pi = 3.14159265358979323846;
    k.kx = (float)((double)env->width / (2.0 * pi)); k.ky = (float)((double)env->height / pi);
    k.hx = (float)((double)env->width / 2.0); k.hy = (float)((double)env->height / 2.0);
    k.filter = env->filter;
    HIP_TRY(c, quiesce(c));   // a render in flight, on a side stream (PT_OPT_OVERLAP) too, reads the old map to its end
    c->env = std::move(m);
    c->env_gen++;
    return PT_OK;
}

extern "C" int pt_eval_environment(pt_ctx* c, const float* rays_dev, size_t n_rays, float* radiance_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!c->env.k.texels) return fail(c, PT_ERR_NO_SCENE, "pt_eval_environment: no environment map uploaded");
    if (n_rays == 0) return PT_OK;
    if (!rays_dev || !radiance_dev) return fail(c, PT_ERR_INVALID, "pt_eval_environment: null argument");
    if (n_rays >= (1ull << 32)) return fail(c, PT_ERR_INVALID, "pt_eval_environment: more than 2^32 - 1 rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_eval_environment, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, c->stream, c->env.k, (const float4*)rays_dev,
                       (uint32_t)n_rays, radiance_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_environment_is_light(pt_ctx* c, int* out) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!out) return fail(c, PT_ERR_INVALID, "pt_environment_is_light: null argument");
    *out = c->env.k.texels && c->env.k.cx ? 1 : 0;
    return PT_OK;
}

extern "C" int pt_sample_environment(pt_ctx* c, const float* u_dev, size_t n, float* dir_pdf_dev, float* radiance_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!c->env.k.texels) return fail(c, PT_ERR_NO_SCENE, "pt_sample_environment: no environment map uploaded");
    if (!c->env.k.cx) return fail(c, PT_ERR_UNSUPPORTED, "pt_sample_environment: the map is no light (PT_OPT_ENV_LIGHT at its upload, an orthonormal basis, not black)");
    if (n == 0) return PT_OK;
    if (!u_dev || !dir_pdf_dev) return fail(c, PT_ERR_INVALID, "pt_sample_environment: null argument");
    if (n >= (1ull << 32)) return fail(c, PT_ERR_INVALID, "pt_sample_environment: more than 2^32 - 1 draws in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_sample_environment, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->env.k, (const float2*)u_dev, (uint32_t)n,
                       (float4*)dir_pdf_dev, radiance_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_environment_pdf(pt_ctx* c, const float* rays_dev, size_t n, float* pdf_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!c->env.k.texels) return fail(c, PT_ERR_NO_SCENE, "pt_environment_pdf: no environment map uploaded");
    if (!c->env.k.cx) return fail(c, PT_ERR_UNSUPPORTED, "pt_environment_pdf: the map is no light (PT_OPT_ENV_LIGHT at its upload, an orthonormal basis, not black)");
    if (n == 0) return PT_OK;
    if (!rays_dev || !pdf_dev) return fail(c, PT_ERR_INVALID, "pt_environment_pdf: null argument");
    if (n >= (1ull << 32)) return fail(c, PT_ERR_INVALID, "pt_environment_pdf: more than 2^32 - 1 rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_environment_pdf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->env.k, (const float4*)rays_dev, (uint32_t)n, pdf_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
