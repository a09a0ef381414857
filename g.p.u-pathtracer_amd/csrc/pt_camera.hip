// pt_camera.hip — pt_camera_rays: the jittered rays of five camera models, written on the device into the buffer pt_render_rays
// reads (the contract is include/ptmi.h's).  One translation unit of libptmi.so (pt_ctx.h).
//   k_camera_rays<MODEL, LIST>  one thread per ray, 256-thread blocks; the pixel number from the list (one coalesced dword load) or
//                    first_pixel + i; the two jitter draws of the pixel's stream (none under PT_CAMF_CENTRE), the model's
//                    arithmetic, and the row as two 16-byte stores — a wave writes 2 KiB contiguously.  No LDS, no atomics; the
//                    only device memory touched is the caller's.
// The models' arithmetic is pt_model_ray<MODEL> (pt_camera_model.h), which pt_render_camera's path start (pt_k_camera.hip) calls too.
// The pinhole is pt_camera_ray (pt_shade.h) called with that jitter: what path_begin_hashed computes, so the rows equal the first
// segments of pt_render's samples bit for bit.  The other models share its pixel offsets and are checked against float64.
#include <cmath>

#include "pt_ctx.h"
#include "pt_camera_model.h"

static_assert(sizeof(pt_camera_model) == 32, "ABI struct size (tests/test_camera.py)");
static_assert((PT_CAM_LENS_KEY >> 63) == 1, "the lens stream's key has its top bit set");

namespace {

struct CamArgs {
    pt_camera cam;
    pt_camera_model cm;
    uint64_t frame;
    const uint32_t* __restrict__ pixels;   // LIST: n pixel numbers
    uint32_t first_pixel;                  // !LIST: row i is pixel first_pixel + i (< width * height, checked on the host)
    uint32_t n;
    uint32_t n_pix;                        // width * height
};

template <int MODEL, bool LIST>
__global__ void __launch_bounds__(256) k_camera_rays(const CamArgs A, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t pix = LIST ? A.pixels[i] : A.first_pixel + i;
    v3 o = cam_v3(A.cam.pos), d = V3(0.f, 0.f, 0.f);
    if (!LIST || pix < A.n_pix) {   // a listed index past the image: the zero-direction row
        float jx = 0.0f, jy = 0.0f;
        if (!(A.cm.flags & PT_CAMF_CENTRE)) {   // the two draws of path_begin_hashed
            pt_rng rng = pt_rng_init(pt_wang64(A.frame), (uint64_t)pix);
            const float u0 = pt_rng_next(rng), u1 = pt_rng_next(rng);
            jx = u0 - 0.5f; jy = u1 - 0.5f;
        }
        pt_model_ray<MODEL>(A.cam, A.cm, A.frame, pix, jx, jy, o, d);   // pt_camera_model.h
    }
    rays[2 * (size_t)i] = make_float4(o.x, o.y, o.z, 0.0f);
    rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

template <int MODEL>
void launch_model(const CamArgs& A, float4* rays, hipStream_t st) {
    const dim3 grid((unsigned)(((size_t)A.n + 255) / 256)), block(256);
    if (A.pixels) hipLaunchKernelGGL((k_camera_rays<MODEL, true>), grid, block, 0, st, A, rays);
    else hipLaunchKernelGGL((k_camera_rays<MODEL, false>), grid, block, 0, st, A, rays);
}

}  // namespace

using namespace ptmi;

extern "C" int pt_camera_rays(pt_ctx* c, const pt_camera* cam, const pt_camera_model* cm, uint64_t frame, const uint32_t* pixels_dev,
                              size_t n, uint64_t first_pixel, float* rays_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (n == 0) return PT_OK;
    if (!cam || !cm || !rays_dev) return fail(c, PT_ERR_INVALID, "pt_camera_rays: null argument");
    const Refusal r = check_camera_model("pt_camera_rays", *cm, n, first_pixel, pixels_dev != nullptr);   // pt_plan.h
    if (r.code != PT_OK) return fail(c, r);
    const uint64_t n_pix = (uint64_t)cm->width * (uint64_t)cm->height;
    HIP_TRY(c, hipSetDevice(c->device));
    CamArgs A;
    A.cam = *cam; A.cm = *cm; A.frame = frame; A.pixels = pixels_dev;
    A.first_pixel = pixels_dev ? 0u : (uint32_t)first_pixel;
    A.n = (uint32_t)n; A.n_pix = (uint32_t)n_pix;
    HIP_TRY(c, span_begin(c));
    float4* rays = (float4*)rays_dev;
    switch (cm->model) {
    case PT_CAM_PINHOLE: launch_model<PT_CAM_PINHOLE>(A, rays, c->stream); break;
    case PT_CAM_THIN_LENS: launch_model<PT_CAM_THIN_LENS>(A, rays, c->stream); break;
    case PT_CAM_ORTHO: launch_model<PT_CAM_ORTHO>(A, rays, c->stream); break;
    case PT_CAM_FISHEYE: launch_model<PT_CAM_FISHEYE>(A, rays, c->stream); break;
    default: launch_model<PT_CAM_EQUIRECT>(A, rays, c->stream); break;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
