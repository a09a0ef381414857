// pt_camera_model.h — the arithmetic of the five camera models (include/ptmi.h: PT_CAM_*), written once for the two kernels that make
// camera rays: k_camera_rays (pt_camera.hip) stores the ray, k_render_camera (pt_k_camera.hip) starts a path on it in registers.  Both
// are compiled with -ffp-contract=off, so the one source gives the same bits in both.
#pragma once
#include <cmath>

#include "pt_kernels.h"

__device__ __forceinline__ v3 cam_v3(const float* v) { return V3(v[0], v[1], v[2]); }

// The ray of pixel pix (< W * H) under model MODEL with the sub-pixel jitter (jx, jy); o and d come in as (pos, 0) and a pixel that
// has no ray (outside the fisheye's image circle) leaves them so.  frame keys the lens stream of PT_CAM_THIN_LENS.
template <int MODEL>
__device__ __forceinline__ void pt_model_ray(const pt_camera& cam, const pt_camera_model& cm, uint64_t frame, uint32_t pix, float jx,
                                             float jy, v3& o, v3& d) {
    const int W = cm.width, H = cm.height;
    const int px = (int)(pix % (uint32_t)W), py = (int)(pix / (uint32_t)W);
    const v3 pos = cam_v3(cam.pos);
    const v3 front = cam_v3(cam.front), right = cam_v3(cam.right), up = cam_v3(cam.up);
    // the pixel's offsets from the image centre, as pt_camera_ray forms them
    const float ax = (((float)px - (float)W / 2.0f) + 0.5f) + jx, ay = (((float)py - (float)H / 2.0f) + 0.5f) + jy;
    if constexpr (MODEL == PT_CAM_PINHOLE) {
        pt_camera_ray(cam, W, H, px, py, jx, jy, o, d);
    } else if constexpr (MODEL == PT_CAM_THIN_LENS) {
        const float xs = ax * cam.dist * cam.aspect * cam.fov / (float)(W - 1), ys = ay * cam.dist * cam.fov / (float)(H - 1);
        const v3 dir0 = vmadd(up, ys, vmadd(right, xs, vscale(front, cam.dist)));
        const v3 pf = vmadd(dir0, cm.focus_dist / cam.dist, pos);
        const float R = cm.lens_radius;
        if (R > 0.0f) {   // R == 0: the origin is pos itself, whatever the sign of its zeros
            pt_rng lens = pt_rng_init(pt_wang64(frame ^ PT_CAM_LENS_KEY), (uint64_t)pix);
            const float v0 = pt_rng_next(lens), v1 = pt_rng_next(lens);
            float c, s;
            pt_sincos2pi(v1, c, s);
            const float lr = R * sqrtf(v0);
            o = vmadd(up, lr * s, vmadd(right, lr * c, pos));
        }
        d = vnormalize(vsub(pf, o));
    } else if constexpr (MODEL == PT_CAM_ORTHO) {
        const float sx = ax * cm.ortho_height * cam.aspect / (float)W, sy = ay * cm.ortho_height / (float)H;
        o = vmadd(up, sy, vmadd(right, sx, pos));
        d = vnormalize(front);
    } else if constexpr (MODEL == PT_CAM_FISHEYE) {
        const float r_px = (float)(W < H ? W : H) / 2.0f, half = cm.fisheye_fov / 2.0f;
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

// ... with the model a value the whole launch shares: a scalar branch
__device__ __forceinline__ void pt_model_ray_of(int model, const pt_camera& cam, const pt_camera_model& cm, uint64_t frame, uint32_t pix,
                                                float jx, float jy, v3& o, v3& d) {
    switch (model) {
    case PT_CAM_PINHOLE: pt_model_ray<PT_CAM_PINHOLE>(cam, cm, frame, pix, jx, jy, o, d); break;
    case PT_CAM_THIN_LENS: pt_model_ray<PT_CAM_THIN_LENS>(cam, cm, frame, pix, jx, jy, o, d); break;
    case PT_CAM_ORTHO: pt_model_ray<PT_CAM_ORTHO>(cam, cm, frame, pix, jx, jy, o, d); break;
    case PT_CAM_FISHEYE: pt_model_ray<PT_CAM_FISHEYE>(cam, cm, frame, pix, jx, jy, o, d); break;
    default: pt_model_ray<PT_CAM_EQUIRECT>(cam, cm, frame, pix, jx, jy, o, d); break;
    }
}
