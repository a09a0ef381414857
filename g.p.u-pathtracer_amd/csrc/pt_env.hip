// pt_env.hip — the environment map on the context: pt_upload_environment, pt_eval_environment and its kernel.
// One translation unit of libptmi.so (pt_ctx.h).  The lookup itself is pt_env.h's, shared with the path kernels.  DESIGN.md §10 f11.
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

namespace ptmi {

// every stream a kernel that reads the map can still be running on
static hipError_t env_quiesce(pt_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && c->own_stream != c->stream) e = hipStreamSynchronize(c->own_stream);
    for (pt_ctx::Side& s : c->side)
        if (e == hipSuccess && s.stream) e = hipStreamSynchronize(s.stream);
    return e;
}

void env_release(pt_ctx* c) {
    (void)hipFree((void*)c->env.texels);
    c->env = KEnv{};
}

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace ptmi

using namespace ptmi;

extern "C" int pt_upload_environment(pt_ctx* c, const pt_environment* env, const float* texels) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!env) {   // clear: bk_color again, and the stage-split pipeline with it
        HIP_TRY(c, env_quiesce(c));
        env_release(c);
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
    // the new copy is complete before anything of the old one is touched: any failure up to here leaves the old map in place
    float4* dev = nullptr;
    HIP_TRY(c, hipMalloc((void**)&dev, n * sizeof(float4)));
    hipError_t e = hipMemcpy(dev, host.data(), n * sizeof(float4), hipMemcpyHostToDevice);
    // a render in flight, on a side stream (PT_OPT_OVERLAP) too, reads the old map to its end
    if (e == hipSuccess) e = env_quiesce(c);
    if (e != hipSuccess) { (void)hipFree(dev); return hip_fail(c, e, "pt_upload_environment"); }
    env_release(c);
    KEnv& k = c->env;
    k.texels = dev;
    k.W = env->width; k.H = env->height;
    for (int i = 0; i < 3; i++) { k.front[i] = env->front[i]; k.right[i] = env->right[i]; k.up[i] = env->up[i]; }
    const double pi = 3.14159265358979323846;
    k.kx = (float)((double)env->width / (2.0 * pi)); k.ky = (float)((double)env->height / pi);
    k.hx = (float)((double)env->width / 2.0); k.hy = (float)((double)env->height / 2.0);
    k.filter = env->filter;
    c->env_gen++;
    return PT_OK;
}

extern "C" int pt_eval_environment(pt_ctx* c, const float* rays_dev, size_t n_rays, float* radiance_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!c->env.texels) return fail(c, PT_ERR_NO_SCENE, "pt_eval_environment: no environment map uploaded");
    if (n_rays == 0) return PT_OK;
    if (!rays_dev || !radiance_dev) return fail(c, PT_ERR_INVALID, "pt_eval_environment: null argument");
    if (n_rays >= (1ull << 32)) return fail(c, PT_ERR_INVALID, "pt_eval_environment: more than 2^32 - 1 rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_eval_environment, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, c->stream, c->env, (const float4*)rays_dev,
                       (uint32_t)n_rays, radiance_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
