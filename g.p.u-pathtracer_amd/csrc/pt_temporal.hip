// pt_temporal.hip — the history of earlier frames reprojected into a new one: pt_temporal (include/ptmi.h states the
// arithmetic, tests/temporal_ref.py restates it), pt_temporal_motion (the same for triangles moved by pt_refit_bvh, §10 f14;
// tests/motion_ref.py), pt_temporal_moments (the luminance moments reprojected as the colour is, §10 f15) and pt_temporal_camera
// (the history of any of the five camera models, §10 f20).  One translation unit of libptmi.so (pt_ctx.h).
//   k_temporal<IDS>  one lane per pixel in 16x16 tiles; the current hit point projected into the previous camera, up to four
//                    bilinear taps of the history — per tap the id (when given) first, then normal and position as one dwordx4
//                    each, colour and length only for a tap that passed every test; no LDS (neighbouring lanes share their taps
//                    through L1 / L2)
//   k_tm_first       no history: out = cur bit for bit, length 1 (+ display words)
//   k_temporal_motion<MOTION>  k_temporal<true>'s pixel (tm_pixel, shared) behind one more step — the pixel's triangle row in the
//                    previous and the current vertex buffer, a dwordx3 per vertex, and for a row that changed the point the
//                    pixel's barycentric coordinates had on the previous triangle; that point, not the pixel's own, is
//                    projected and tested (+ the motion, when asked for)
//   k_temporal_moments<IDS, MOVED>  tm_pixel with the (m1, m2) payload — pt_temporal's rule (MOVED 0) or pt_temporal_motion's
//                    (MOVED 1, also the launch without a history); no length, no display word
//   k_temporal_camera<IDS, MOVED>  tm_pixel with the projection of the previous camera's MODEL (pt_temporal_camera, §10 f20): the
//                    inverses of pt_camera_model.h's five models, the model a value of the launch; rows where the caller gave them
#include <cmath>
#include <cstring>

#include "pt_image.h"

namespace {

struct TmArgs {
    const float* __restrict__ prev_color;      // [H][W][3]; never the out buffers (checked on the host)
    const float* __restrict__ prev_len;        // [H][W]
    const float4* __restrict__ prev_normal;
    const float4* __restrict__ prev_position;
    const int32_t* __restrict__ prev_id;       // null = ids not compared
    const float* cur_color;                    // [H][W][3] (out_color may alias it)
    const float4* __restrict__ cur_normal;
    const float4* __restrict__ cur_position;
    const int32_t* __restrict__ cur_id;
    float* out_color;
    float* __restrict__ out_len;
    uint32_t* __restrict__ rgba;               // may be null
    int W, H;
    float pos[3], front[3], right[3], up[3];   // the previous camera
    float sx, sy, cx, cy;                      // fx = b / a * sx + cx
    float max_history, plane_tol, normal_thr;
};

__global__ void __launch_bounds__(PTD_BLOCK) k_tm_first(const TmArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float r = A.cur_color[3 * p], g = A.cur_color[3 * p + 1], b = A.cur_color[3 * p + 2];
    A.out_color[3 * p] = r; A.out_color[3 * p + 1] = g; A.out_color[3 * p + 2] = b;
    A.out_len[p] = 1.0f;
    if (A.rgba) A.rgba[p] = pt_pack_rgba(r, g, b);
}

// pt_temporal behind one more step, where the pixel's surface point was when the history was rendered
struct TmMotionArgs {
    TmArgs t;                                  // t.prev_color null = no history: out = cur, motion 0
    const float* __restrict__ prev_verts;      // [n_tris][9] by original id; may equal cur_verts
    const float* __restrict__ cur_verts;
    float2* __restrict__ motion;               // [H][W]; null unless the kernel writes it
    uint32_t n_tris;
};

// Vertex k of a 36-byte row that is only 4-byte aligned: one dwordx3 load.  The empty asm keeps the compiler from seeing that the
// three vertices are adjacent, or it joins their nine words into two dwordx4 loads and one dword.
__device__ __forceinline__ v3 tm_vertex(const float* row, int k) {
    const float* r = row + 3 * k;
    asm("" : "+v"(r));
    const __attribute__((address_space(1))) float* q = (const __attribute__((address_space(1))) float*)r;   // global, not flat
    return V3(q[0], q[1], q[2]);
}
__device__ __forceinline__ bool tm_same_bits(const v3& a, const v3& b) {
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) && __float_as_uint(a.z) == __float_as_uint(b.z);
}
__device__ __forceinline__ bool tm_positive_finite(float a) { return a > 0.f && a < INFINITY; }

// Where the previous camera saw a point, v = x' - pos, in the two steps tm_pixel takes: depth(v), which must be > 0 or the history is
// rejected, and at(v, depth), the history coordinates (fx, fy) — not finite where the model rejects behind that.  TmPinhole is step 2
// of pt_temporal, the statements tm_pixel held before its projection became a parameter.
struct TmPinhole {
    __device__ __forceinline__ float depth(const TmArgs& A, const v3& v) const { return vdot(v, V3(A.front[0], A.front[1], A.front[2])); }
    __device__ __forceinline__ float2 at(const TmArgs& A, const v3& v, float a) const {
        const float fx = fmaf(vdot(v, V3(A.right[0], A.right[1], A.right[2])) / a, A.sx, A.cx);
        const float fy = fmaf(vdot(v, V3(A.up[0], A.up[1], A.up[2])) / a, A.sy, A.cy);
        return make_float2(fx, fy);
    }
};
// The inverses of the five camera models (pt_camera_model.h; include/ptmi.h states them under pt_temporal_camera), the model a value
// of the launch: a scalar branch.  sx, sy, cx, cy hold the model's host constants (temporal_args).  The two models of all directions
// have no depth test (1 passes it); what they reject comes back as NaN coordinates.
struct TmModel {
    int model;
    __device__ __forceinline__ bool angular() const { return model == PT_CAM_FISHEYE || model == PT_CAM_EQUIRECT; }
    __device__ __forceinline__ float depth(const TmArgs& A, const v3& v) const { return angular() ? 1.0f : TmPinhole().depth(A, v); }
    __device__ __forceinline__ float2 at(const TmArgs& A, const v3& v, float a) const {
        if (model == PT_CAM_PINHOLE || model == PT_CAM_THIN_LENS) return TmPinhole().at(A, v, a);
        const float b = vdot(v, V3(A.right[0], A.right[1], A.right[2]));
        const float c = vdot(v, V3(A.up[0], A.up[1], A.up[2]));
        if (model == PT_CAM_ORTHO) return make_float2(fmaf(b, A.sx, A.cx), fmaf(c, A.sy, A.cy));   // sx = W / (ortho_height * aspect), sy = H / ortho_height
        a = TmPinhole().depth(A, v);
        const float nan = __uint_as_float(0x7fc00000u);
        if (model == PT_CAM_FISHEYE) {   // sx = (min(W, H) / 2) / half, sy = half = fisheye_fov / 2
            const float s = sqrtf(fmaf(c, c, b * b));
            const float theta = atan2f(s, a);
            if ((a == 0.f && s == 0.f) || theta > A.sy) return make_float2(nan, nan);
            const float rho = theta * A.sx;
            const float k = s > 0.f ? rho / s : 0.f;
            return make_float2(fmaf(b, k, A.cx), fmaf(c, k, A.cy));
        }
        // PT_CAM_EQUIRECT: sx = W / 2 pi, sy = H / pi, cx = W / 2, cy = H / 2 (an integer coordinate is a texel centre)
        const float h = sqrtf(fmaf(b, b, a * a));
        if (h == 0.f && c == 0.f) return make_float2(nan, nan);
        return make_float2(fmaf(atan2f(b, a), A.sx, A.cx), fmaf(atan2f(c, h), A.sy, A.cy));
    }
};

// One pixel of k_temporal (MOVED 0: M unused, and nothing below differs from what the kernel held before the two shared it) and
// of k_temporal_motion (MOVED 1; 2 = the motion is written as well).  The projection, the taps and the blend are the same
// statements for both, so a surface point that did not move gets k_temporal<true>'s bits.
// PAY 3: the payload is the colour.  PAY 2 (pt_temporal_moments): the buffers named *_color hold (m1, m2) rows, the blend runs on
// those two, and neither a length nor a display word is written; every other statement is shared.
// PROJ: where the previous camera saw the point (above).  MOVED 3 (k_temporal_camera only): MOVED 0's static point with MOVED 2's
// motion written — ROWS and MOTION below are what MOVED 0, 1, 2 always meant.
template <bool IDS, int MOVED, int PAY = 3, class PROJ = TmPinhole>
__device__ __forceinline__ void tm_pixel(const TmArgs& A, const TmMotionArgs* M, const PROJ proj = PROJ()) {
    constexpr bool ROWS = MOVED == 1 || MOVED == 2, MOTION = MOVED >= 2;
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float cr = A.cur_color[PAY * p], cg = A.cur_color[PAY * p + 1];
    float cb = 0.f;
    if constexpr (PAY == 3) cb = A.cur_color[3 * p + 2];
    const float4 n4 = (MOVED != 0 && !A.prev_color) ? make_float4(0.f, 0.f, 0.f, 0.f) : A.cur_normal[p];   // no history: every pixel as a miss
    float o0 = cr, o1 = cg, o2 = cb, on = 1.0f;   // no history accepted: the current frame, bit for bit
    float mx = 0.f, my = 0.f;
    if (n4.x != 0.f || n4.y != 0.f || n4.z != 0.f) {
        const float4 x4 = A.cur_position[p];
        v3 np = V3(n4.x, n4.y, n4.z), xp = V3(x4.x, x4.y, x4.z);
        int idm = 0;
        bool was = true;   // the point has a place in the previous frame's scene: (xp, np) become (x', n')
        if constexpr (ROWS) {
            idm = A.cur_id[p];
            if (idm >= 0) {
                was = (uint32_t)idm < M->n_tris;   // past the rows: no history, and no row is read
                if (was && M->prev_verts != M->cur_verts) {
                    const float* cw = M->cur_verts + 9 * (size_t)idm;
                    const float* pw = M->prev_verts + 9 * (size_t)idm;
                    const v3 c0 = tm_vertex(cw, 0), c1 = tm_vertex(cw, 1), c2 = tm_vertex(cw, 2);
                    const v3 p0 = tm_vertex(pw, 0), p1 = tm_vertex(pw, 1), p2 = tm_vertex(pw, 2);
                    if (!(tm_same_bits(c0, p0) && tm_same_bits(c1, p1) && tm_same_bits(c2, p2))) {
                        const v3 e1 = vsub(c1, c0), e2 = vsub(c2, c0), w = vsub(xp, c0);
                        const v3 N = vcross(e1, e2);
                        const float nn = vdot(N, N);
                        const float inv = 1.0f / nn;
                        const float u = vdot(vcross(w, e2), N) * inv, v = vdot(vcross(e1, w), N) * inv;   // barycentric, not clamped
                        const v3 f1 = vsub(p1, p0), f2 = vsub(p2, p0);
                        const v3 N1 = vcross(f1, f2);
                        const float nn1 = vdot(N1, N1);
                        was = tm_positive_finite(nn) && fabsf(u) < INFINITY && fabsf(v) < INFINITY && tm_positive_finite(nn1);
                        xp = vmadd(f2, v, vmadd(f1, u, p0));
                        // the previous triangle's unit normal on the face the current ray sees
                        np = vscale(N1, (vdot(np, N) < 0.f ? -1.0f : 1.0f) * (1.0f / sqrtf(nn1)));
                    }
                }
            }
        }
        const v3 v = vsub(xp, V3(A.pos[0], A.pos[1], A.pos[2]));
        const float a = proj.depth(A, v);
        if (a > 0.f && (!ROWS || was)) {
            const float2 f = proj.at(A, v, a);
            const float fx = f.x, fy = f.y;
            if constexpr (MOTION) {
                if (fabsf(fx) < INFINITY && fabsf(fy) < INFINITY) { mx = fx - (float)x; my = fy - (float)y; }
            }
            // outside (-1, W) x (-1, H) no tap is inside the image; NaN and infinities fail here too, before the conversion to int
            if (fx > -1.0f && fx < (float)A.W && fy > -1.0f && fy < (float)A.H) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float wx = fx - x0f, wy = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float tol = A.plane_tol * x4.w;
                int idp = 0;
                if constexpr (ROWS) idp = idm;
                else if (IDS) idp = A.cur_id[p];
                float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f;
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int xq = x0 + i, yq = y0 + j;
                        const float w = (i ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
                        if (xq < 0 || xq >= A.W || yq < 0 || yq >= A.H || !(w > 0.f)) continue;
                        const size_t q = (size_t)yq * (size_t)A.W + (size_t)xq;
                        if (IDS) {
                            if (A.prev_id[q] != idp) continue;
                        }
                        const float4 nq = A.prev_normal[q], xq4 = A.prev_position[q];
                        if (nq.x == 0.f && nq.y == 0.f && nq.z == 0.f) continue;   // the history pixel is a miss
                        if (!(vdot(np, V3(nq.x, nq.y, nq.z)) >= A.normal_thr)) continue;
                        const v3 dq = vsub(V3(xq4.x, xq4.y, xq4.z), xp);
                        if (!(fabsf(vdot(np, dq)) <= tol)) continue;
                        const float* c = A.prev_color + PAY * q;
                        sr = fmaf(w, c[0], sr); sg = fmaf(w, c[1], sg);
                        if constexpr (PAY == 3) sb = fmaf(w, c[2], sb);
                        sl = fmaf(w, A.prev_len[q], sl);
                        sw += w;
                    }
                }
                if (sw >= 0.01f) {
                    const float inv = 1.0f / sw;
                    const float hr = sr * inv, hg = sg * inv, hb = sb * inv;
                    on = fminf(sl * inv + 1.0f, A.max_history);
                    const float k = 1.0f / on;
                    o0 = fmaf(cr - hr, k, hr); o1 = fmaf(cg - hg, k, hg); o2 = fmaf(cb - hb, k, hb);
                }
            }
        }
    }
    if constexpr (PAY == 2) {
        A.out_color[2 * p] = o0; A.out_color[2 * p + 1] = o1;
        return;
    }
    A.out_color[3 * p] = o0; A.out_color[3 * p + 1] = o1; A.out_color[3 * p + 2] = o2;
    A.out_len[p] = on;
    if (A.rgba) A.rgba[p] = pt_pack_rgba(o0, o1, o2);
    if constexpr (MOTION) M->motion[p] = make_float2(mx, my);
}

template <bool IDS>
__global__ void __launch_bounds__(PTD_BLOCK) k_temporal(const TmArgs A) {
    tm_pixel<IDS, 0>(A, nullptr);
}

// A row of the vertex buffers is 36 bytes and only 4-byte aligned: three dwordx3 loads each.  The lanes of a tile mostly share a
// few triangles, so the rows come from L1 / L2.
template <bool MOTION>
__global__ void __launch_bounds__(PTD_BLOCK) k_temporal_motion(const TmMotionArgs M) {
    tm_pixel<true, MOTION ? 2 : 1>(M.t, &M);
}

// MOVED 0: pt_temporal's rule (IDS as there); MOVED 1: pt_temporal_motion's rule, which is also the launch without a history (every
// pixel as a miss: out = cur).
template <bool IDS, int MOVED>
__global__ void __launch_bounds__(PTD_BLOCK) k_temporal_moments(const TmMotionArgs M) {
    tm_pixel<IDS, MOVED, 2>(M.t, &M);
}

// tm_pixel under the previous camera's model (pt_temporal_camera).  MOVED 0: no rows, IDS as k_temporal; 3: the same with the motion
// written (also the launch without a history: every pixel as a miss, motion 0); 1, 2: k_temporal_motion's rows.
struct TmCameraArgs {
    TmMotionArgs m;
    int model;
};
template <bool IDS, int MOVED>
__global__ void __launch_bounds__(PTD_BLOCK) k_temporal_camera(const TmCameraArgs C) {
    tm_pixel<IDS, MOVED, 3>(C.m.t, &C.m, TmModel{C.model});
}

using namespace ptmi;

// What the four calls share: the argument rules (check_temporal_call, pt_plan.h, under the caller's name `fn`) and the kernel
// arguments of the reprojection, with the vertex rows where the call reads them.  PT_OK with M filled, or the error already recorded.
int temporal_args(pt_ctx* c, const char* fn, const TemporalCall& a, TmMotionArgs& M) {
    const Refusal r = check_temporal_call(fn, a);
    if (r.code != PT_OK) return fail(c, r);
    std::memset(&M, 0, sizeof M);
    TmArgs& A = M.t;
    const pt_temporal_params* tp = a.tp;
    A.cur_color = a.cur_color;
    A.cur_normal = (const float4*)a.cur_normal;
    A.cur_position = (const float4*)a.cur_position;
    A.out_color = a.out_color;
    A.out_len = a.out_length;
    A.rgba = a.rgba;
    A.W = tp->width; A.H = tp->height;
    M.motion = (float2*)a.motion;
    if (!a.prev_color) return PT_OK;
    A.prev_color = a.prev_color;
    A.prev_len = a.prev_length;
    A.prev_normal = (const float4*)a.prev_normal;
    A.prev_position = (const float4*)a.prev_position;
    A.prev_id = a.prev_id;
    A.cur_id = a.cur_id;
    const pt_camera* prev_cam = a.prev_cam;
    for (int i = 0; i < 3; i++) {
        A.pos[i] = prev_cam->pos[i]; A.front[i] = prev_cam->front[i]; A.right[i] = prev_cam->right[i]; A.up[i] = prev_cam->up[i];
    }
    // the inverse of pt_camera_ray's pixel mapping, every step one binary32 rounding
    A.sx = (float)(tp->width - 1) / (prev_cam->aspect * prev_cam->fov);
    A.sy = (float)(tp->height - 1) / prev_cam->fov;
    A.cx = (float)tp->width / 2.0f - 0.5f;
    A.cy = (float)tp->height / 2.0f - 0.5f;
    if (a.kind == TEMPORAL_CAMERA) {   // ... or of pt_model_ray's (TmModel reads these four)
        const pt_camera_model& cm = *a.prev_cm;
        const float W = (float)tp->width, H = (float)tp->height;
        switch (cm.model) {
        case PT_CAM_ORTHO:
            A.sx = W / (cm.ortho_height * prev_cam->aspect);
            A.sy = H / cm.ortho_height;
            break;
        case PT_CAM_FISHEYE:
            A.sy = cm.fisheye_fov / 2.0f;
            A.sx = ((float)std::min(tp->width, tp->height) / 2.0f) / A.sy;
            break;
        case PT_CAM_EQUIRECT:
            A.sx = W / 6.28318548f;
            A.sy = H / 3.14159274f;
            A.cx = W / 2.0f;
            A.cy = H / 2.0f;
            break;
        default: break;   // the pinhole and the thin lens: every guide ray passes through pos along dir0
        }
    }
    A.max_history = tp->max_history;
    A.plane_tol = tp->plane_tolerance;
    A.normal_thr = tp->normal_threshold;
    if (temporal_reads_rows(a)) {
        M.prev_verts = a.prev_verts;
        M.cur_verts = a.cur_verts;
        M.n_tris = (uint32_t)a.n_tris;
    }
    return PT_OK;
}

}  // namespace

extern "C" int pt_temporal(pt_ctx* c, const pt_temporal_params* tp, const pt_camera* prev_cam, const float* prev_color_dev,
                           const float* prev_length_dev, const float* prev_normal_dev, const float* prev_position_dev,
                           const int32_t* prev_id_dev, const float* cur_color_dev, const float* cur_normal_dev,
                           const float* cur_position_dev, const int32_t* cur_id_dev, float* out_color_dev, float* out_length_dev,
                           uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    TemporalCall a = {};
    a.kind = TEMPORAL_COLOUR;
    a.tp = tp; a.prev_cam = prev_cam;
    a.prev_color = prev_color_dev; a.prev_length = prev_length_dev; a.prev_normal = prev_normal_dev; a.prev_position = prev_position_dev; a.prev_id = prev_id_dev;
    a.cur_color = cur_color_dev; a.cur_normal = cur_normal_dev; a.cur_position = cur_position_dev; a.cur_id = cur_id_dev;
    a.out_color = out_color_dev; a.out_length = out_length_dev; a.rgba = rgba_dev;
    TmMotionArgs M;
    if (int rc = temporal_args(c, "pt_temporal", a, M)) return rc;
    const TmArgs& A = M.t;
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid = ptd_grid(tp->width, tp->height);
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (!A.prev_color) hipLaunchKernelGGL(k_tm_first, grid, dim3(PTD_BLOCK), 0, st, A);
    else if (A.prev_id) hipLaunchKernelGGL(k_temporal<true>, grid, dim3(PTD_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(k_temporal<false>, grid, dim3(PTD_BLOCK), 0, st, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_temporal_motion(pt_ctx* c, const pt_temporal_params* tp, const pt_camera* prev_cam, const float* prev_verts_dev,
                                  const float* cur_verts_dev, size_t n_tris, const float* prev_color_dev, const float* prev_length_dev,
                                  const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                                  const float* cur_color_dev, const float* cur_normal_dev, const float* cur_position_dev,
                                  const int32_t* cur_id_dev, float* out_color_dev, float* out_length_dev, uint32_t* rgba_dev,
                                  float* motion_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    TemporalCall a = {};
    a.kind = TEMPORAL_MOTION;
    a.tp = tp; a.prev_cam = prev_cam;
    a.prev_color = prev_color_dev; a.prev_length = prev_length_dev; a.prev_normal = prev_normal_dev; a.prev_position = prev_position_dev; a.prev_id = prev_id_dev;
    a.cur_color = cur_color_dev; a.cur_normal = cur_normal_dev; a.cur_position = cur_position_dev; a.cur_id = cur_id_dev;
    a.out_color = out_color_dev; a.out_length = out_length_dev; a.rgba = rgba_dev;
    a.prev_verts = prev_verts_dev; a.cur_verts = cur_verts_dev; a.n_tris = n_tris; a.motion = motion_dev;
    TmMotionArgs M;
    if (int rc = temporal_args(c, "pt_temporal_motion", a, M)) return rc;
    const bool history = prev_color_dev != nullptr;
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid = ptd_grid(tp->width, tp->height);
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (motion_dev) hipLaunchKernelGGL(k_temporal_motion<true>, grid, dim3(PTD_BLOCK), 0, st, M);   // (without a history: out = cur, motion 0)
    else if (history) hipLaunchKernelGGL(k_temporal_motion<false>, grid, dim3(PTD_BLOCK), 0, st, M);
    else hipLaunchKernelGGL(k_tm_first, grid, dim3(PTD_BLOCK), 0, st, M.t);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_temporal_moments(pt_ctx* c, const pt_temporal_params* tp, const pt_camera* prev_cam, const float* prev_verts_dev,
                                   const float* cur_verts_dev, size_t n_tris, const float* prev_moments_dev, const float* prev_length_dev,
                                   const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                                   const float* cur_moments_dev, const float* cur_normal_dev, const float* cur_position_dev,
                                   const int32_t* cur_id_dev, float* out_moments_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    TemporalCall a = {};
    a.kind = TEMPORAL_MOMENTS;
    a.tp = tp; a.prev_cam = prev_cam;
    a.prev_color = prev_moments_dev; a.prev_length = prev_length_dev; a.prev_normal = prev_normal_dev; a.prev_position = prev_position_dev; a.prev_id = prev_id_dev;
    a.cur_color = cur_moments_dev; a.cur_normal = cur_normal_dev; a.cur_position = cur_position_dev; a.cur_id = cur_id_dev;
    a.out_color = out_moments_dev;
    a.prev_verts = prev_verts_dev; a.cur_verts = cur_verts_dev; a.n_tris = n_tris;
    TmMotionArgs M;
    if (int rc = temporal_args(c, "pt_temporal_moments", a, M)) return rc;
    const bool history = prev_moments_dev != nullptr;
    const bool motion = temporal_reads_rows(a);   // pt_temporal_motion's rule
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid = ptd_grid(tp->width, tp->height);
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (!history || motion) hipLaunchKernelGGL((k_temporal_moments<true, 1>), grid, dim3(PTD_BLOCK), 0, st, M);   // (no history: out = cur)
    else if (M.t.prev_id) hipLaunchKernelGGL((k_temporal_moments<true, 0>), grid, dim3(PTD_BLOCK), 0, st, M);
    else hipLaunchKernelGGL((k_temporal_moments<false, 0>), grid, dim3(PTD_BLOCK), 0, st, M);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_temporal_camera(pt_ctx* c, const pt_temporal_params* tp, const pt_camera* prev_cam, const pt_camera_model* prev_cm,
                                  const float* prev_verts_dev, const float* cur_verts_dev, size_t n_tris, const float* prev_color_dev,
                                  const float* prev_length_dev, const float* prev_normal_dev, const float* prev_position_dev,
                                  const int32_t* prev_id_dev, const float* cur_color_dev, const float* cur_normal_dev,
                                  const float* cur_position_dev, const int32_t* cur_id_dev, float* out_color_dev, float* out_length_dev,
                                  uint32_t* rgba_dev, float* motion_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    TemporalCall a = {};
    a.kind = TEMPORAL_CAMERA;
    a.tp = tp; a.prev_cam = prev_cam; a.prev_cm = prev_cm;
    a.prev_color = prev_color_dev; a.prev_length = prev_length_dev; a.prev_normal = prev_normal_dev; a.prev_position = prev_position_dev; a.prev_id = prev_id_dev;
    a.cur_color = cur_color_dev; a.cur_normal = cur_normal_dev; a.cur_position = cur_position_dev; a.cur_id = cur_id_dev;
    a.out_color = out_color_dev; a.out_length = out_length_dev; a.rgba = rgba_dev;
    a.prev_verts = prev_verts_dev; a.cur_verts = cur_verts_dev; a.n_tris = n_tris; a.motion = motion_dev;
    TmCameraArgs C;
    if (int rc = temporal_args(c, "pt_temporal_camera", a, C.m)) return rc;
    const bool history = prev_color_dev != nullptr, rows = temporal_reads_rows(a), ids = C.m.t.prev_id != nullptr;
    C.model = history ? prev_cm->model : PT_CAM_PINHOLE;
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid = ptd_grid(tp->width, tp->height), block(PTD_BLOCK);
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (!history && !motion_dev) hipLaunchKernelGGL(k_tm_first, grid, block, 0, st, C.m.t);
    else if (!history) hipLaunchKernelGGL((k_temporal_camera<false, 3>), grid, block, 0, st, C);   // out = cur, motion 0
    else if (rows && motion_dev) hipLaunchKernelGGL((k_temporal_camera<true, 2>), grid, block, 0, st, C);
    else if (rows) hipLaunchKernelGGL((k_temporal_camera<true, 1>), grid, block, 0, st, C);
    else if (motion_dev && ids) hipLaunchKernelGGL((k_temporal_camera<true, 3>), grid, block, 0, st, C);
    else if (motion_dev) hipLaunchKernelGGL((k_temporal_camera<false, 3>), grid, block, 0, st, C);
    else if (ids) hipLaunchKernelGGL((k_temporal_camera<true, 0>), grid, block, 0, st, C);
    else hipLaunchKernelGGL((k_temporal_camera<false, 0>), grid, block, 0, st, C);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
