// pt_k_camera.hip — pt_render_camera: the path loop over the pixels of a camera model, each sample's ray made where its path starts.
// One translation unit of libptmi.so (pt_ctx.h); the API function is ptmi.hip's.  DESIGN.md §10 f17.
//
// k_render_camera<V> is the loop of pt_rays_loop.h (k_rays_loop) — k_render_rays' — started from KCamRays: a refilled lane takes its pixel from the
// list (one dword load) or from first_pixel + row, initialises the path's stream from (frame + sample, pixel), spends its first two
// draws on the jitter and computes the model's ray (pt_camera_model.h: the arithmetic k_camera_rays stores) in registers.  So sample s
// of a row starts at the row pt_camera_rays writes for that pixel in frame + s, with the stream pt_render has for the pixel — no ray
// buffer, no 32-byte loads per slot, no launch per sample.  The model is a value of the launch (a scalar branch taken once per path),
// not a template argument: the family has k_render_rays' 19 words (rays_exists).  The camera rides in KParams::cam, which
// pt_render_rays leaves zero; the model and the pixels are the second kernel argument.  The fold is pt_k_rays.hip's.
#include "pt_ctx.h"
#include "pt_camera_model.h"
#include "pt_rays_loop.h"

struct KCamRays {
    pt_camera_model cm;
    const uint32_t* __restrict__ pixels;   // n pixel numbers, or nullptr: row i is pixel first_pixel + i
    float* __restrict__ out;               // [n][3] running mean of the samples' radiance
    uint32_t first_pixel;
    uint32_t n_pix;                        // width * height: a listed index from here on has no ray
    uint32_t n;
    int hdr;                               // PT_RAYS_HDR: the fold does not clamp

    // The camera, the model and the pixels are read HERE, through the kernel-argument pointer (PT_KARGS; this struct lies behind
    // KParams), and not as the members of P and of *this: everything derived from them is uniform float arithmetic, which this
    // target computes in VGPRs, and hoisted out of the persistent loop it would hold registers of every lane for the whole kernel
    // (measured: 21 spilled VGPRs in the (6, 16) kernels instead of at most 1; path_begin_hashed reads its camera the same way).
    template <class PS>
    __device__ __forceinline__ void start(const KParams&, uint32_t s_idx, uint32_t row, PS& ps) const {
        PT_KARGS(K);
        typedef const __attribute__((address_space(4))) KCamRays KArg;
        KArg& C = *(KArg*)((const __attribute__((address_space(4))) char*)K_p + sizeof(KParams));
        pt_camera cam;
        for (int i = 0; i < 3; i++) { cam.pos[i] = K.cam.pos[i]; cam.front[i] = K.cam.front[i]; cam.right[i] = K.cam.right[i]; cam.up[i] = K.cam.up[i]; }
        cam.dist = K.cam.dist; cam.aspect = K.cam.aspect; cam.fov = K.cam.fov; cam._pad = 0.f;
        pt_camera_model m;
        m.model = C.cm.model; m.width = C.cm.width; m.height = C.cm.height; m.flags = C.cm.flags;
        m.lens_radius = C.cm.lens_radius; m.focus_dist = C.cm.focus_dist; m.ortho_height = C.cm.ortho_height; m.fisheye_fov = C.cm.fisheye_fov;
        const uint32_t pix = C.pixels ? C.pixels[row] : C.first_pixel + row;
        const uint64_t frame = K.frame + s_idx;
        // pt_render's stream of this (frame, pixel); its first two draws are the jitter (path_begin_hashed), and under
        // PT_CAMF_CENTRE it stands behind them all the same (k_render_rays)
        ps.rng = pt_rng_init(pt_wang64(frame), (uint64_t)pix);
        float jx = 0.0f, jy = 0.0f;
        if (!(m.flags & PT_CAMF_CENTRE)) {
            const float u0 = pt_rng_next(ps.rng), u1 = pt_rng_next(ps.rng);
            jx = u0 - 0.5f; jy = u1 - 0.5f;
        }
        ps.rng.n = 2;
        v3 o = cam_v3(cam.pos), d = V3(0.f, 0.f, 0.f);
        if (pix < C.n_pix) pt_model_ray_of(m.model, cam, m, frame, pix, jx, jy, o, d);   // else the zero-direction row: a miss
        ps.o = o;
        ps.d = d;
    }
};
static_assert(sizeof(KParams) % alignof(KCamRays) == 0, "the second kernel argument lies right behind KParams (KCamRays::start)");

template <uint32_t V>
constexpr auto k_render_camera = &k_rays_loop<V, KCamRays>;

namespace ptmi {

// Instantiated: camera_exists (= rays_exists); the request's word: rays_word (pt_variants.h), as launch_render_rays.  P.cam holds the camera.
hipError_t launch_render_camera(const LaunchCfg& L, const KParams& P, const CameraCall& r, hipStream_t st) {
    const KCamRays R{*r.cm, r.pixels, r.out, r.pixels ? 0u : (uint32_t)r.first_pixel, (uint32_t)((uint64_t)r.cm->width * (uint64_t)r.cm->height),
                     (uint32_t)r.n, r.hdr};
    return with_variant<camera_exists, PV_BITS>(rays_word(L), [&](auto v) {
        return launch_resident(k_render_camera<v()>, L.lds, INT_MAX, L.n_cu, (size_t)std::max(1, L.work_blocks), st, P, R);
    });
}

}  // namespace ptmi
