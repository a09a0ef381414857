// pt_aux.hip — pt_render_aux and pt_render_aux_camera: the first-hit guide buffers the image stages read (under a
// camera model §10 f20).  One translation unit of libptmi.so (pt_ctx.h).
//   k_render_aux     one lane per pixel, a 256-thread block per 16x16 tile (one wave per 8x8 quadrant): the pixel-centre camera
//                    ray, the binary closest-hit walk of pt_trace_rays, the spheres by pt_closest_sphere; albedo, normal,
//                    position (+ t) as float4 rows, the hit id
//   k_render_aux_camera  the same lane, tile and hit (aux_rows) behind the pixel-centre ray of one of the five camera models
//                    (pt_camera_model.h: the row pt_camera_rays writes under PT_CAMF_CENTRE with lens_radius 0)
#include <cstring>

#include "pt_image.h"
#include "pt_camera_model.h"

namespace {

struct AuxOut {
    float4* __restrict__ albedo;
    float4* __restrict__ normal;
    float4* __restrict__ position;
    int32_t* __restrict__ id;   // may be null
};

// What both kernels do behind the walk of a pixel's ray: the spheres, the rows of the four buffers.  The walk and its stack stay
// written in each kernel: moved in here, k_render_aux no longer compiles to the instructions it had (tools/isa_compare.py).
__device__ __forceinline__ void aux_rows(const KParams& P, const AuxOut& A, const size_t pix, const Hit& h, const v3& o, const v3& d) {
    const SceneHit sh = pt_closest_sphere(P, o, d, h);
    float4 alb = make_float4(0.f, 0.f, 0.f, 0.f), nrm = alb, pos = alb;
    int32_t id = -1;
    if (sh.geom != 3) {
        const v3 hitpos = vmadd(d, sh.t, o);
        v3 n, col;
        if (sh.geom == 1) {
            const pt_sphere_d& s = P.sc.spheres[sh.sph_id];
            n = vnormalize(vsub(hitpos, V3(s.px, s.py, s.pz)));
            col = V3(s.col[0], s.col[1], s.col[2]);
            id = -2 - sh.sph_id;
        } else {
            n = vnormalize(pt_hit_normal(P.sc, h));
            if (P.tri_matid) {
                const float4 m0 = P.mat_table[2 * P.tri_matid[h.tri]];
                col = V3(m0.x, m0.y, m0.z);
            } else {
                col = V3(P.tri_col[0], P.tri_col[1], P.tri_col[2]);
            }
            id = h.tri;
        }
        if (!(vdot(n, d) < 0)) n = vscale(n, -1.0f);
        alb = make_float4(col.x, col.y, col.z, 0.f);
        nrm = make_float4(n.x, n.y, n.z, 0.f);
        pos = make_float4(hitpos.x, hitpos.y, hitpos.z, sh.t);
    }
    A.albedo[pix] = alb;
    A.normal[pix] = nrm;
    A.position[pix] = pos;
    if (A.id) A.id[pix] = id;
}

// KParams first: pt_closest_sphere reads the spheres through the kernel-argument pointer at offset 0 (PT_KARGS)
__global__ void __launch_bounds__(PT_BLOCK_RAYS) k_render_aux(const KParams P, const AuxOut A) {
    float4* s_top = s_dyn;
    lds_load_top<PT_BLOCK_RAYS>(P.sc, s_top);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int px = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const int py = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    if (px >= P.W || py >= P.H) return;
    const size_t pix = (size_t)py * (size_t)P.W + (size_t)px;
    v3 o, d;
    pt_camera_ray(P.cam, P.W, P.H, px, py, 0.0f, 0.0f, o, d);   // u0 = u1 = 0.5: the pixel centre
    TravCount tc;
    TravOverflow<PT_STACK_CAP> stk_ovf;
    TravStack<PT_STACK_CAP, PT_BLOCK_RAYS> stk(__builtin_amdgcn_readfirstlane(16 * P.sc.n_top + (tid & ~63)), stk_ovf);
    const Hit h = trav_bvh2<TW_TOP>(P.sc, o, d, P.cull != 0, stk, tc, s_top);
    aux_rows(P, A, pix, h, o, d);
}

// k_render_aux under a camera model (P.W, P.H = the model's image): the model is a value of the launch, a scalar branch.  A pixel
// without a ray (d = 0, outside the fisheye's circle) writes its miss here: 1 / d is infinite, it must not reach the slab test.
struct AuxCamera {
    AuxOut out;
    pt_camera_model cm;   // lens_radius 0 (the host clears it): the ray through the lens centre, no draw
};
__global__ void __launch_bounds__(PT_BLOCK_RAYS) k_render_aux_camera(const KParams P, const AuxCamera C) {
    float4* s_top = s_dyn;
    lds_load_top<PT_BLOCK_RAYS>(P.sc, s_top);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int px = blockIdx.x * 16 + (wv & 1) * 8 + (lane & 7);
    const int py = blockIdx.y * 16 + (wv >> 1) * 8 + (lane >> 3);
    if (px >= P.W || py >= P.H) return;
    const size_t pix = (size_t)py * (size_t)P.W + (size_t)px;
    v3 o = cam_v3(P.cam.pos), d = V3(0.f, 0.f, 0.f);
    pt_model_ray_of(C.cm.model, P.cam, C.cm, 0, (uint32_t)pix, 0.0f, 0.0f, o, d);   // pt_camera_rays' row under PT_CAMF_CENTRE
    if (d.x == 0.f && d.y == 0.f && d.z == 0.f) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        C.out.albedo[pix] = zero;
        C.out.normal[pix] = zero;
        C.out.position[pix] = zero;
        if (C.out.id) C.out.id[pix] = -1;
        return;
    }
    TravCount tc;
    TravOverflow<PT_STACK_CAP> stk_ovf;
    TravStack<PT_STACK_CAP, PT_BLOCK_RAYS> stk(__builtin_amdgcn_readfirstlane(16 * P.sc.n_top + (tid & ~63)), stk_ovf);
    const Hit h = trav_bvh2<TW_TOP>(P.sc, o, d, P.cull != 0, stk, tc, s_top);
    aux_rows(P, C.out, pix, h, o, d);
}

}  // namespace

using namespace ptmi;

extern "C" int pt_render_aux(pt_ctx* c, const pt_camera* cam, const pt_params* p, float* albedo_dev, float* normal_dev,
                             float* position_dev, int32_t* id_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    const Refusal r = check_aux_call(f, p, cam && albedo_dev && normal_dev && position_dev);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    KParams P;
    std::memset(&P, 0, sizeof P);
    scene_view(c, P.sc, P.ksph);
    const size_t lds = binary_ray_layout(f, P.sc);
    P.cam = *cam;
    P.W = p->width; P.H = p->height;
    P.cull = p->cull_backfaces;
    for (int i = 0; i < 3; i++) P.tri_col[i] = p->tri_col[i];
    P.tri_matid = c->mat.d_tri_matid.get();
    P.mat_table = c->mat.d_mat_table.get();
    AuxOut A;
    A.albedo = (float4*)albedo_dev;
    A.normal = (float4*)normal_dev;
    A.position = (float4*)position_dev;
    A.id = id_dev;
    HIP_TRY(c, allow_lds(k_render_aux, lds));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_render_aux, ptd_grid(p->width, p->height), dim3(PT_BLOCK_RAYS), lds, c->stream, P, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_render_aux_camera(pt_ctx* c, const pt_camera* cam, const pt_camera_model* cm, const pt_params* p, float* albedo_dev,
                                    float* normal_dev, float* position_dev, int32_t* id_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    const Refusal r = check_aux_camera_call(f, cm, p, cam && albedo_dev && normal_dev && position_dev);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    KParams P;
    std::memset(&P, 0, sizeof P);
    scene_view(c, P.sc, P.ksph);
    const size_t lds = binary_ray_layout(f, P.sc);
    P.cam = *cam;
    P.W = cm->width; P.H = cm->height;
    P.cull = p->cull_backfaces;
    for (int i = 0; i < 3; i++) P.tri_col[i] = p->tri_col[i];
    P.tri_matid = c->mat.d_tri_matid.get();
    P.mat_table = c->mat.d_mat_table.get();
    AuxCamera C;
    C.out.albedo = (float4*)albedo_dev;
    C.out.normal = (float4*)normal_dev;
    C.out.position = (float4*)position_dev;
    C.out.id = id_dev;
    C.cm = *cm;
    C.cm.lens_radius = 0.0f;
    HIP_TRY(c, allow_lds(k_render_aux_camera, lds));
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_render_aux_camera, ptd_grid(cm->width, cm->height), dim3(PT_BLOCK_RAYS), lds, c->stream, P, C);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
