// pt_camera.hip — pt_camera_rays: the jittered rays of five camera models, written on the device into the buffer pt_render_rays
// reads (the contract is include/ptmi.h's).  One translation unit of libptmi.so (pt_ctx.h).
//   k_camera_rays<MODEL, LIST>  one thread per ray, 256-thread blocks; the pixel number from the list (one coalesced dword load) or
//                    first_pixel + i; the two jitter draws of the pixel's stream (none under PT_CAMF_CENTRE), the model's
//                    arithmetic, and the row as two 16-byte stores — a wave writes 2 KiB contiguously.  No LDS, no atomics; the
//                    only device memory touched is the caller's.
// The pinhole is pt_camera_ray (pt_shade.h) called with that jitter: what path_begin_hashed computes, so the rows equal the first
// segments of pt_render's samples bit for bit.  The other models share its pixel offsets and are checked against float64.
#include <cmath>

#include "pt_ctx.h"

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

__device__ __forceinline__ v3 cam_v3(const float* v) { return V3(v[0], v[1], v[2]); }

template <int MODEL, bool LIST>
__global__ void __launch_bounds__(256) k_camera_rays(const CamArgs A, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t pix = LIST ? A.pixels[i] : A.first_pixel + i;
    const pt_camera& cam = A.cam;
    const int W = A.cm.width, H = A.cm.height;
    const v3 pos = cam_v3(cam.pos);
    v3 o = pos, d = V3(0.f, 0.f, 0.f);
    if (!LIST || pix < A.n_pix) {   // a listed index past the image: the zero-direction row
        const int px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
        float jx = 0.0f, jy = 0.0f;
        if (!(A.cm.flags & PT_CAMF_CENTRE)) {   // the two draws of path_begin_hashed
            pt_rng rng = pt_rng_init(pt_wang64(A.frame), (uint64_t)pix);
            const float u0 = pt_rng_next(rng), u1 = pt_rng_next(rng);
            jx = u0 - 0.5f; jy = u1 - 0.5f;
        }
        const v3 front = cam_v3(cam.front), right = cam_v3(cam.right), up = cam_v3(cam.up);
        // the pixel's offsets from the image centre, as pt_camera_ray forms them
        const float ax = (((float)px - (float)W / 2.0f) + 0.5f) + jx, ay = (((float)py - (float)H / 2.0f) + 0.5f) + jy;
        if constexpr (MODEL == PT_CAM_PINHOLE) {
            pt_camera_ray(cam, W, H, px, py, jx, jy, o, d);
        } else if constexpr (MODEL == PT_CAM_THIN_LENS) {
            const float xs = ax * cam.dist * cam.aspect * cam.fov / (float)(W - 1), ys = ay * cam.dist * cam.fov / (float)(H - 1);
            const v3 dir0 = vmadd(up, ys, vmadd(right, xs, vscale(front, cam.dist)));
            const v3 pf = vmadd(dir0, A.cm.focus_dist / cam.dist, pos);
            const float R = A.cm.lens_radius;
            if (R > 0.0f) {   // R == 0: the origin is pos itself, whatever the sign of its zeros
                pt_rng lens = pt_rng_init(pt_wang64(A.frame ^ PT_CAM_LENS_KEY), (uint64_t)pix);
                const float v0 = pt_rng_next(lens), v1 = pt_rng_next(lens);
                float c, s;
                pt_sincos2pi(v1, c, s);
                const float lr = R * sqrtf(v0);
                o = vmadd(up, lr * s, vmadd(right, lr * c, pos));
            }
            d = vnormalize(vsub(pf, o));
        } else if constexpr (MODEL == PT_CAM_ORTHO) {
            const float sx = ax * A.cm.ortho_height * cam.aspect / (float)W, sy = ay * A.cm.ortho_height / (float)H;
            o = vmadd(up, sy, vmadd(right, sx, pos));
            d = vnormalize(front);
        } else if constexpr (MODEL == PT_CAM_FISHEYE) {
            const float r_px = (float)(W < H ? W : H) / 2.0f, half = A.cm.fisheye_fov / 2.0f;
            const float rho = sqrtf(ax * ax + ay * ay), theta = rho / r_px * half;
            if (rho == 0.0f) {
                d = vnormalize(front);
            } else if (!(theta > half)) {   // inside the image circle
                float st, ct;
                sincosf(theta, &st, &ct);
                const float k = st / rho;
                d = vnormalize(vmadd(up, ay * k, vmadd(right, ax * k, vscale(front, ct))));
            }
        } else {   // PT_CAM_EQUIRECT
            const float fx = (float)px + jx, fy = (float)py + jy;
            const float lon = (fx - (float)W / 2.0f) * (6.28318548f / (float)W);
            const float lat = fminf(fmaxf((fy - (float)H / 2.0f) * (3.14159274f / (float)H), -1.57079637f), 1.57079637f);
            float sl, cl, sa, ca;
            sincosf(lon, &sl, &cl);
            sincosf(lat, &sa, &ca);
            d = vnormalize(vmadd(up, sa, vscale(vmadd(right, sl, vscale(front, cl)), ca)));
        }
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
    if (cm->model < PT_CAM_PINHOLE || cm->model > PT_CAM_EQUIRECT) return fail(c, PT_ERR_INVALID, "pt_camera_rays: unknown camera model");
    if (cm->flags & ~PT_CAMF_CENTRE) return fail(c, PT_ERR_INVALID, "pt_camera_rays: unknown flag bits");
    const uint64_t n_pix = (uint64_t)(cm->width > 0 ? cm->width : 0) * (uint64_t)(cm->height > 0 ? cm->height : 0);
    if (cm->width < 2 || cm->height < 2 || n_pix >= (1ull << 32))
        return fail(c, PT_ERR_INVALID, "pt_camera_rays: width and height must be >= 2 with width * height < 2^32");
    if (n >= (1ull << 32)) return fail(c, PT_ERR_INVALID, "pt_camera_rays: more than 2^32 - 1 rays in one call");
    if (!pixels_dev && (first_pixel > n_pix || (uint64_t)n > n_pix - first_pixel))
        return fail(c, PT_ERR_INVALID, "pt_camera_rays: first_pixel + n exceeds width * height");
    switch (cm->model) {
    case PT_CAM_THIN_LENS:
        if (!std::isfinite(cm->lens_radius) || cm->lens_radius < 0.0f || !std::isfinite(cm->focus_dist) || !(cm->focus_dist > 0.0f))
            return fail(c, PT_ERR_INVALID, "pt_camera_rays: lens_radius must be finite and >= 0, focus_dist finite and > 0");
        break;
    case PT_CAM_ORTHO:
        if (!std::isfinite(cm->ortho_height) || !(cm->ortho_height > 0.0f)) return fail(c, PT_ERR_INVALID, "pt_camera_rays: ortho_height must be finite and > 0");
        break;
    case PT_CAM_FISHEYE:
        if (!std::isfinite(cm->fisheye_fov) || !(cm->fisheye_fov > 0.0f) || cm->fisheye_fov > 6.28318548f)
            return fail(c, PT_ERR_INVALID, "pt_camera_rays: fisheye_fov must be in (0, 2 pi]");
        break;
    default: break;
    }
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
