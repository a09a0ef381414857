// pt_denoise.hip — pt_render_aux (first-hit guide buffers), pt_denoise (edge-avoiding a-trous wavelet filter, Dammertz et
// al. 2010), pt_temporal (the history of earlier frames reprojected into a new one, §10 f8),
// pt_temporal_motion (the same for triangles moved by pt_refit_bvh, §10 f14), pt_denoise_variance (the filter steered by each pixel's
// variance), pt_temporal_moments (the moments reprojected as the colour is, §10 f15) and pt_select_pixels (adaptive sampling's pixel
// list, §10 f18), pt_meter and pt_tonemap (the display stage, §10 f19).  One translation unit of libptmi.so (pt_ctx.h).
//   k_render_aux     one lane per pixel, a 256-thread block per 16x16 tile (one wave per 8x8 quadrant): the pixel-centre camera
//                    ray, the binary closest-hit walk of pt_trace_rays, the spheres by pt_closest_sphere; albedo, normal,
//                    position (+ t) as float4 rows, the hit id
//   k_dn_demod       colour / albedo into ping-pong buffer A as float4 (i, hit) — the hit flag rides in .w, so a tap learns
//                    whether q is a miss from the colour load it makes anyway
//   k_dn_iter<LAST>  one launch per iteration, 16x16 tiles: 25 taps, each one dwordx4 load per buffer (colour; normal and
//                    position only where both ends are hits) and ONE v_exp_f32 (the three terms folded into exp2 with log2(e)
//                    in the per-launch constants); the last iteration remodulates, clamps, writes out (+ display words)
//   k_dn_copy        iterations = 0: out = color bit for bit (+ display words)
//   k_temporal<IDS>  pt_temporal: one lane per pixel in the same 16x16 tiles; the current hit point projected
//                    into the previous camera, up to four bilinear taps of the history — per tap the id (when given) first, then
//                    normal and position as one dwordx4 each, colour and length only for a tap that passed every test; no LDS
//                    (neighbouring lanes share their taps through L1 / L2)
//   k_tm_first       pt_temporal without a history: out = cur bit for bit, length 1 (+ display words)
//   k_temporal_motion<MOTION>  pt_temporal_motion: k_temporal<true>'s pixel (tm_pixel, shared) behind one more
//                    step — the pixel's triangle row in the previous and the current vertex buffer, a dwordx3 per vertex, and for
//                    a row that changed the point the pixel's barycentric coordinates had on the previous triangle; that
//                    point, not the pixel's own, is projected and tested (+ the motion, when asked for)
//   k_dv_seed<COPY>  pt_denoise_variance: colour / albedo and the variance of the mean luminance from the
//                    moments into ping-pong buffer A as float4 (i, v) — the hit flag rides in the SIGN BIT of v (a miss with
//                    variance 0 is -0.0f, so the flag is read as a bit, never with < 0); COPY is iterations = 0
//   k_dv_iter<LAST>  k_dn_iter's launch shape and tap budget (one dwordx4 of (i, v); normal and position only where both ends
//                    are hits; one v_exp_f32); per PIXEL, not per tap: the 3x3 pre-filter of v (eight dword loads from L1 —
//                    no LDS apron, so no barrier and the lanes outside the image still leave at once) and one division for the
//                    luminance stop 1 / (sigma_l sd + 1e-4); v travels as sum w^2 v / (sum w)^2
//   k_temporal_moments<IDS, MOVED>  pt_temporal_moments: tm_pixel with the (m1, m2) payload — pt_temporal's rule (MOVED 0) or
//                    pt_temporal_motion's (MOVED 1, also the launch without a history); no length, no display word
//   k_frame_error    pt_frame_error: one lane per pixel, the relative standard error of the mean luminance from the moments
//                    pt_render_moments keeps; a block adds its 256 values up in LDS, in double, and writes
//                    ONE partial sum and ONE count to its own slot — the host adds the slots in block order
//   k_select_count, k_select_scan, k_select_write  pt_select_pixels: k_frame_error's figure with each pixel's own
//                    sample count and the rule "needs more samples", over the same blocks — per block the sum and the number of
//                    selected pixels (wave ballots), one block's exclusive scan of those numbers, then every selected pixel stores
//                    its number at its rank: an ascending list without atomics and without a block that waits for another
//   k_tonemap<TABLE, VEC>  pt_tonemap: exposure, curve and display word of one pixel per thread, or of four (VEC:
//                    three dwordx4 loads, one dwordx4 store of words); TABLE: the transfer's 256 thresholds staged in LDS once per
//                    block and searched in eight branch-free steps per channel — no pow on the device
//   k_meter_hist<VEC>, k_meter_finish  pt_meter: a fixed grid's luminance histograms (257 counters in LDS, integer LDS adds, one row
//                    of plain stores per block), then one block that adds the rows, scans the bins, trims, and leaves the exposure
//                    in the caller's four floats — nothing returns to the host
// No LDS tile: at step 16 the taps are 64 rows apart, an apron would re-read more than it saves; the packed buffers of a 1080p
// frame (~100 MB) stay in the 256 MB Infinity Cache.
#include <cmath>
#include <cstring>

#include "pt_ctx.h"

#define PTD_TILE 16
#define PTD_BLOCK (PTD_TILE * PTD_TILE)

namespace {

struct AuxOut {
    float4* __restrict__ albedo;
    float4* __restrict__ normal;
    float4* __restrict__ position;
    int32_t* __restrict__ id;   // may be null
};

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

__device__ __forceinline__ float ptd_demod_div(float a) { return a > 1e-3f ? a : 1.0f; }
template <class Args>
__device__ __forceinline__ bool ptd_pixel(const Args& A, int& x, int& y) {
    x = blockIdx.x * PTD_TILE + (threadIdx.x & (PTD_TILE - 1));
    y = blockIdx.y * PTD_TILE + (threadIdx.x / PTD_TILE);
    return x < A.W && y < A.H;
}

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
    A.out[3 * p] = r; A.out[3 * p + 1] = g; A.out[3 * p + 2] = b;
    if (A.rgba) A.rgba[p] = pt_pack_rgba(r, g, b);
}

template <bool LAST>
__global__ void __launch_bounds__(PTD_BLOCK) k_dn_iter(const DnArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 cp = A.src[p];
    const bool hp = cp.w != 0.f;
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), xp = np;
    float kxp = 0.f;
    if (hp) {
        np = A.normal[p];
        xp = A.position[p];
        kxp = fminf(A.kx / (xp.w * xp.w), 1e30f);   // 1 / (sigma_x t_p)^2, finite
    }
    const float hk[5] = {1.f / 16.f, 4.f / 16.f, 6.f / 16.f, 4.f / 16.f, 1.f / 16.f};
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
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
                continue;
            }
            const size_t q = (size_t)yq * (size_t)A.W + (size_t)xq;
            const float4 cq = A.src[q];
            if ((cq.w != 0.f) != hp) continue;   // exactly one of p, q is a miss
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            float e = A.kc * fmaf(db, db, fmaf(dg, dg, dr * dr));
            if (hp) {
                const float4 nq = A.normal[q], xq4 = A.position[q];
                const float ax = np.x - nq.x, ay = np.y - nq.y, az = np.z - nq.z;
                const float bx = xp.x - xq4.x, by = xp.y - xq4.y, bz = xp.z - xq4.z;
                e = fmaf(A.kn, fmaf(az, az, fmaf(ay, ay, ax * ax)), e);
                e = fmaf(kxp, fmaf(bz, bz, fmaf(by, by, bx * bx)), e);
            }
            const float w = hh * __builtin_amdgcn_exp2f(-e);   // one v_exp_f32
            sr = fmaf(w, cq.x, sr); sg = fmaf(w, cq.y, sg); sb = fmaf(w, cq.z, sb); sw += w;
        }
    }
    const float inv = 1.0f / sw;
    const float r = sr * inv, g = sg * inv, b = sb * inv;
    if (!LAST) {
        A.dst[p] = make_float4(r, g, b, cp.w);
    } else {
        const float4 a = A.albedo[p];
        const float o0 = pt_clamp01(r * ptd_demod_div(a.x)), o1 = pt_clamp01(g * ptd_demod_div(a.y)), o2 = pt_clamp01(b * ptd_demod_div(a.z));
        A.out[3 * p] = o0; A.out[3 * p + 1] = o1; A.out[3 * p + 2] = o2;
        if (A.rgba) A.rgba[p] = pt_pack_rgba(o0, o1, o2);
    }
}

// pt_denoise_variance (include/ptmi.h states the arithmetic, tests/denoise_var_ref.py restates it)
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

__device__ __forceinline__ float dv_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool dv_is_miss(float v) { return (__float_as_uint(v) >> 31) != 0u; }   // -0.0f is a miss too

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
        A.out[3 * p] = r; A.out[3 * p + 1] = g; A.out[3 * p + 2] = b;
        if (A.rgba) A.rgba[p] = pt_pack_rgba(r, g, b);
        if (A.out_var) A.out_var[p] = var;
    } else {
        const float4 a = A.albedo[p], nr = A.normal[p];
        const float ax = ptd_demod_div(a.x), ay = ptd_demod_div(a.y), az = ptd_demod_div(a.z);
        const float la = dv_lum(ax, ay, az);
        const float v0 = var / (la * la);
        const bool hit = nr.x != 0.f || nr.y != 0.f || nr.z != 0.f;
        A.dst[p] = make_float4(r / ax, g / ay, b / az, hit ? v0 : __uint_as_float(__float_as_uint(v0) | 0x80000000u));
    }
}

// One iteration.  Per pixel: the 3x3 pre-filter of v (eight dword loads of adjacent pixels, from L1: the step-1 taps of the same
// tile touch the same lines) and one division for the luminance stop; per tap k_dn_iter's budget.
template <bool LAST>
__global__ void __launch_bounds__(PTD_BLOCK) k_dv_iter(const DvArgs A) {
    int x, y;
    if (!ptd_pixel(A, x, y)) return;
    const size_t p = (size_t)y * (size_t)A.W + (size_t)x;
    const float4 cp = A.src[p];
    const bool mp = dv_is_miss(cp.w);
    const bool hp = !mp;
    const float vp = fabsf(cp.w);
    float4 np = make_float4(0.f, 0.f, 0.f, 0.f), xp = np;
    float kxp = 0.f;
    if (hp) {
        np = A.normal[p];
        xp = A.position[p];
        kxp = fminf(A.kx / (xp.w * xp.w), 1e30f);   // 1 / (sigma_x t_p)^2, finite
    }
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
    const float kl = A.sl > 0.f ? 1.44269504f / fmaf(A.sl, sd, 1e-4f) : 0.f;   // log2(e) k_p
    const float lp = dv_lum(cp.x, cp.y, cp.z);
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
                sv = fmaf(hh * hh, vp, sv);
                continue;
            }
            const size_t q = (size_t)yq * (size_t)A.W + (size_t)xq;
            const float4 cq = A.src[q];
            if (dv_is_miss(cq.w) != mp) continue;   // exactly one of p, q is a miss
            float e = kl * fabsf(lp - dv_lum(cq.x, cq.y, cq.z));
            if (hp) {
                const float4 nq = A.normal[q], xq4 = A.position[q];
                const float ax = np.x - nq.x, ay = np.y - nq.y, az = np.z - nq.z;
                const float bx = xp.x - xq4.x, by = xp.y - xq4.y, bz = xp.z - xq4.z;
                e = fmaf(A.kn, fmaf(az, az, fmaf(ay, ay, ax * ax)), e);
                e = fmaf(kxp, fmaf(bz, bz, fmaf(by, by, bx * bx)), e);
            }
            const float w = hh * __builtin_amdgcn_exp2f(-e);   // one v_exp_f32
            sr = fmaf(w, cq.x, sr); sg = fmaf(w, cq.y, sg); sb = fmaf(w, cq.z, sb); sw += w;
            sv = fmaf(w * w, fabsf(cq.w), sv);
        }
    }
    const float inv = 1.0f / sw;
    const float r = sr * inv, g = sg * inv, b = sb * inv;
    const float v = sv * (inv * inv);
    if (!LAST) {
        A.dst[p] = make_float4(r, g, b, mp ? __uint_as_float(__float_as_uint(v) | 0x80000000u) : v);
    } else {
        const float4 a = A.albedo[p];
        const float ax = ptd_demod_div(a.x), ay = ptd_demod_div(a.y), az = ptd_demod_div(a.z);
        const float o0 = pt_clamp01(r * ax), o1 = pt_clamp01(g * ay), o2 = pt_clamp01(b * az);
        A.out[3 * p] = o0; A.out[3 * p + 1] = o1; A.out[3 * p + 2] = o2;
        if (A.rgba) A.rgba[p] = pt_pack_rgba(o0, o1, o2);
        if (A.out_var) {
            const float la = dv_lum(ax, ay, az);
            A.out_var[p] = v * (la * la);
        }
    }
}

// pt_temporal (include/ptmi.h states the arithmetic, tests/temporal_ref.py restates it)
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

// pt_temporal_motion (include/ptmi.h states the arithmetic, tests/motion_ref.py restates it): pt_temporal behind one more step,
// where the pixel's surface point was when the history was rendered
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

// One pixel of k_temporal (MOVED 0: M unused, and nothing below differs from what the kernel held before the two shared it) and
// of k_temporal_motion (MOVED 1; 2 = the motion is written as well).  The projection, the taps and the blend are the same
// statements for both, so a surface point that did not move gets k_temporal<true>'s bits.
// PAY 3: the payload is the colour.  PAY 2 (pt_temporal_moments): the buffers named *_color hold (m1, m2) rows, the blend runs on
// those two, and neither a length nor a display word is written; every other statement is shared.
template <bool IDS, int MOVED, int PAY = 3>
__device__ __forceinline__ void tm_pixel(const TmArgs& A, const TmMotionArgs* M) {
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
        if constexpr (MOVED != 0) {
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
        const float a = vdot(v, V3(A.front[0], A.front[1], A.front[2]));
        if (a > 0.f && (MOVED == 0 || was)) {
            const float fx = fmaf(vdot(v, V3(A.right[0], A.right[1], A.right[2])) / a, A.sx, A.cx);
            const float fy = fmaf(vdot(v, V3(A.up[0], A.up[1], A.up[2])) / a, A.sy, A.cy);
            if constexpr (MOVED == 2) {
                if (fabsf(fx) < INFINITY && fabsf(fy) < INFINITY) { mx = fx - (float)x; my = fy - (float)y; }
            }
            // outside (-1, W) x (-1, H) no tap is inside the image; NaN and infinities fail here too, before the conversion to int
            if (fx > -1.0f && fx < (float)A.W && fy > -1.0f && fy < (float)A.H) {
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float wx = fx - x0f, wy = fy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float tol = A.plane_tol * x4.w;
                int idp = 0;
                if constexpr (MOVED != 0) idp = idm;
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
    if constexpr (MOVED == 2) M->motion[p] = make_float2(mx, my);
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

// pt_temporal_moments: tm_pixel with the (m1, m2) payload.  MOVED 0: pt_temporal's rule (IDS as there); MOVED 1: pt_temporal_motion's
// rule, which is also the launch without a history (every pixel as a miss: out = cur).
template <bool IDS, int MOVED>
__global__ void __launch_bounds__(PTD_BLOCK) k_temporal_moments(const TmMotionArgs M) {
    tm_pixel<IDS, MOVED, 2>(M.t, &M);
}

// pt_frame_error: rse of pixel i in binary32 (include/ptmi.h states the formula); per block the sum of rse in double and the
// number of pixels above the threshold, by the tree reduction of k_tree_cost (pt_tree.hip): no atomics, no fences, the same
// figure run after run
__global__ void __launch_bounds__(256) k_frame_error(const float2* __restrict__ moments, uint32_t n_pix, float nm1, float threshold,
                                                     double* __restrict__ sums, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double rse = 0.0;
    uint32_t above = 0u;
    if (i < n_pix) {
        const float2 m = moments[i];
        const float var = fmaxf(0.f, m.y - m.x * m.x);
        const float r = sqrtf(var / nm1) / (m.x + 0.01f);
        rse = (double)r;
        above = r > threshold ? 1u : 0u;
    }
    __shared__ double s_sum[256];
    __shared__ uint32_t s_cnt[256];
    s_sum[threadIdx.x] = rse; s_cnt[threadIdx.x] = above;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s_sum[threadIdx.x] += s_sum[threadIdx.x + off]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[blockIdx.x] = s_sum[0]; counts[blockIdx.x] = s_cnt[0]; }
}

// ---- pt_tonemap and pt_meter (include/ptmi.h states the arithmetic, tests/tonemap_ref.py restates it).  Both are
// bandwidth-bound — 12 bytes read per pixel, 4 or 12 written — so the VEC routes move a thread's four pixels as three dwordx4 loads
// (and three dwordx4 stores, one dwordx4 store of words); the scalar routes serve buffers that are not 16-byte aligned and pixel
// counts that do not come in fours.  Plain *, + and /: one binary32 rounding per step.
struct ToneArgs {
    const float* color;                 // [n_pix][3]; out may alias it: a thread reads all its pixels before it writes one
    const float* __restrict__ exposure; // float[1] on the device (pt_meter's state[0]); may be null
    const float* __restrict__ table;    // the transfer's 256 thresholds; read only by <TABLE>
    float* out;                         // [n_pix][3], may be null
    uint32_t* rgba;                     // [n_pix], may be null
    uint32_t n_items;                   // pixels, or groups of four pixels (VEC)
    int curve;                          // PT_TONE_*
    float e, iw2;                       // tp->exposure; 1 / white^2 (0: plain Reinhard)
};
__device__ __forceinline__ float tone_in(float c, float e) {
    const float x = c * e;
    return x > 0.f ? fminf(x, 65536.0f) : 0.f;   // a NaN and a negative: 0
}
__device__ __forceinline__ float tone_aces(float x) {
    const float a = x * (2.51f * x + 0.03f);
    const float b = x * (2.43f * x + 0.59f) + 0.14f;
    return fminf(a / b, 1.0f);
}
// the curve's output of one pixel, in place
__device__ __forceinline__ void tone_pixel(int curve, float e, float iw2, float& r, float& g, float& b) {
    r = tone_in(r, e); g = tone_in(g, e); b = tone_in(b, e);
    if (curve == PT_TONE_REINHARD) {
        const float L = dv_lum(r, g, b);
        const float s = (1.0f + L * iw2) / (1.0f + L);
        r = fminf(r * s, 1.0f); g = fminf(g * s, 1.0f); b = fminf(b * s, 1.0f);
    } else if (curve == PT_TONE_ACES) {
        r = tone_aces(r); g = tone_aces(g); b = tone_aces(b);
    } else {
        r = fminf(r, 1.0f); g = fminf(g, 1.0f); b = fminf(b, 1.0f);
    }
}
// the number of k in 1..255 with y >= T[k]: T ascends strictly and T[0] = 0 <= y, so it is the largest k with T[k] <= y — eight
// steps, each one LDS read and a conditional add, no branch
__device__ __forceinline__ uint32_t tone_code(const float* T, float y) {
    uint32_t k = 0u;
#pragma unroll
    for (uint32_t step = 128u; step != 0u; step >>= 1) k += T[k + step] <= y ? step : 0u;
    return k;
}
template <bool TABLE>
__device__ __forceinline__ uint32_t tone_word(const float* T, float r, float g, float b) {
    if (!TABLE) return pt_pack_rgba(r, g, b);
    return (tone_code(T, b) << 16) | (tone_code(T, g) << 8) | tone_code(T, r);
}
template <bool TABLE, bool VEC>
__global__ void __launch_bounds__(256) k_tonemap(const ToneArgs A) {
    __shared__ float s_T[256];
    if (TABLE) {   // once per block
        s_T[threadIdx.x] = A.table[threadIdx.x];
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // (blocks * 256 <= 2^32)
    if (i >= A.n_items) return;
    float e = A.e;
    if (A.exposure) {
        const float scaled = A.e * A.exposure[0];
        if (scaled > 0.f && scaled <= PT_F32_MAX) e = scaled;   // (false for a NaN)
    }
    if (VEC) {
        const float4* c4 = (const float4*)A.color + 3 * (size_t)i;
        const float4 q0 = pt_sld4(c4), q1 = pt_sld4(c4 + 1), q2 = pt_sld4(c4 + 2);
        float p[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            tone_pixel(A.curve, e, A.iw2, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            w[k] = tone_word<TABLE>(s_T, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
        }
        if (A.out) {
            float4* o4 = (float4*)A.out + 3 * (size_t)i;
            o4[0] = make_float4(p[0], p[1], p[2], p[3]);
            o4[1] = make_float4(p[4], p[5], p[6], p[7]);
            o4[2] = make_float4(p[8], p[9], p[10], p[11]);
        }
        if (A.rgba) ((uint4*)A.rgba)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const float* c = A.color + 3 * (size_t)i;
        float r = c[0], g = c[1], b = c[2];
        tone_pixel(A.curve, e, A.iw2, r, g, b);
        if (A.out) {
            float* o = A.out + 3 * (size_t)i;
            o[0] = r; o[1] = g; o[2] = b;
        }
        if (A.rgba) A.rgba[i] = tone_word<TABLE>(s_T, r, g, b);
    }
}

// pt_meter's bin of one pixel: ptmi::METER_BINS = not metered
__device__ __forceinline__ uint32_t meter_bin(float r, float g, float b) {
    const float L = dv_lum(r, g, b);
    if (!(fabsf(L) <= PT_F32_MAX) || L < 1.52587890625e-05f) return ptmi::METER_BINS;   // not finite, or below 2^-16
    if (L >= 65536.0f) return ptmi::METER_BINS - 1u;
    return (__float_as_uint(L) >> 20) - ((127u - 16u) << 3);   // 8 bins per octave: the exponent and the mantissa's top three bits
}
// 1: a fixed grid whose threads stride over the pixels; the block's counts in LDS by integer adds (any order gives the same counts),
// then stored whole to the block's own row of the scratch
template <bool VEC>
__global__ void __launch_bounds__(256) k_meter_hist(const float* __restrict__ color, uint32_t n_items, uint32_t* __restrict__ partial) {
    __shared__ uint32_t s_h[ptmi::METER_BINS + 1];
    s_h[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_h[ptmi::METER_BINS] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += stride) {
        if (VEC) {
            const float4* c4 = (const float4*)color + 3 * i;
            const float4 q0 = pt_sld4(c4), q1 = pt_sld4(c4 + 1), q2 = pt_sld4(c4 + 2);
            atomicAdd(&s_h[meter_bin(q0.x, q0.y, q0.z)], 1u);
            atomicAdd(&s_h[meter_bin(q0.w, q1.x, q1.y)], 1u);
            atomicAdd(&s_h[meter_bin(q1.z, q1.w, q2.x)], 1u);
            atomicAdd(&s_h[meter_bin(q2.y, q2.z, q2.w)], 1u);
        } else {
            const float* c = color + 3 * i;
            atomicAdd(&s_h[meter_bin(c[0], c[1], c[2])], 1u);
        }
    }
    __syncthreads();
    uint32_t* row = partial + (size_t)blockIdx.x * (ptmi::METER_BINS + 1);
    row[threadIdx.x] = s_h[threadIdx.x];
    if (threadIdx.x == 0) row[ptmi::METER_BINS] = s_h[ptmi::METER_BINS];
}
struct MeterArgs {
    const uint32_t* __restrict__ partial;   // [n_blocks][METER_BINS + 1]
    float* state;                            // float[4]
    uint32_t n_blocks;
    float key, low_pct, high_pct, min_exposure, max_exposure, adapt;
    int reset;
};
// 2: one block, thread b owns bin b: the bins' totals, their inclusive scan, the trimmed weights and their two integer sums; thread 0
// turns those into the four state floats
__global__ void __launch_bounds__(256) k_meter_finish(const MeterArgs A) {
    __shared__ uint32_t s_scan[2][256];
    __shared__ unsigned long long s_S[256], s_W[256];
    const uint32_t b = threadIdx.x;
    uint32_t count = 0u;
    for (uint32_t k = 0u; k < A.n_blocks; k++) count += A.partial[(size_t)k * (ptmi::METER_BINS + 1) + b];
    int cur = 0;
    s_scan[0][b] = count;
    __syncthreads();
    for (uint32_t off = 1u; off < 256u; off <<= 1) {   // inclusive, Hillis-Steele (the counts add up to < 2^32)
        const uint32_t x = s_scan[cur][b] + (b >= off ? s_scan[cur][b - off] : 0u);
        s_scan[cur ^ 1][b] = x;
        cur ^= 1;
        __syncthreads();
    }
    const long long cum = (long long)s_scan[cur][b], before = cum - (long long)count, n = (long long)s_scan[cur][255];
    long long lo = (long long)(unsigned long long)((double)A.low_pct * (double)n);
    long long hi = (long long)(unsigned long long)((double)A.high_pct * (double)n);
    if (hi <= lo) { lo = 0; hi = n; }
    const long long span = (cum < hi ? cum : hi) - (before > lo ? before : lo);
    const unsigned long long w = span > 0 ? (unsigned long long)span : 0ull;
    s_S[b] = w * (2ull * b + 1ull);
    s_W[b] = w;
    __syncthreads();
    for (uint32_t off = 128u; off > 0u; off >>= 1) {
        if (b < off) { s_S[b] += s_S[b + off]; s_W[b] += s_W[b + off]; }
        __syncthreads();
    }
    if (b != 0u) return;
    const unsigned long long S = s_S[0], Wt = s_W[0];
    const float prev = A.state[0];
    const bool prev_ok = prev > 0.f && prev <= PT_F32_MAX;   // finite and > 0
    float l_avg = 0.f, target = prev_ok ? prev : 1.0f;
    if (Wt != 0ull) {
        const double p = (double)S / (double)(16ull * Wt) - 16.0;
        const double fl = floor(p);
        l_avg = (float)ldexp(1.0 + (p - fl), (int)fl);
        target = A.key / l_avg;
    }
    target = fminf(fmaxf(target, A.min_exposure), A.max_exposure);
    A.state[0] = (A.reset || !prev_ok) ? target : prev + (target - prev) * A.adapt;
    A.state[1] = target;
    A.state[2] = l_avg;
    A.state[3] = (float)(uint32_t)Wt;   // Wt <= n < 2^32
}

// ---- pt_select_pixels: the pixels that need more samples as an ascending list, in three launches over the same 256-pixel blocks.  No
// block waits for another and nothing is added atomically: the list and the figures are the same run after run.
struct SelectArgs {
    const float2* __restrict__ moments;
    const uint32_t* __restrict__ counts;
    uint32_t n_pix, min_n, max_n;   // min_n = max(min_samples, 2)
    float threshold;
};
// k_frame_error's rse with the pixel's own sample count; 0 below two samples and where it is not finite (include/ptmi.h)
__device__ __forceinline__ float select_rse(float2 m, uint32_t n) {
    if (n < 2u) return 0.f;
    const float var = fmaxf(0.f, m.y - m.x * m.x);
    const float r = sqrtf(var / (float)(n - 1u)) / (m.x + 0.01f);
    return fabsf(r) <= PT_F32_MAX ? r : 0.f;   // (false for a NaN)
}
// the rule of pixel i, for both passes over the blocks; rse: its error figure
__device__ __forceinline__ bool select_pixel(const SelectArgs& A, uint32_t i, float& rse) {
    rse = 0.f;
    if (i >= A.n_pix) return false;
    const uint32_t n = A.counts[i];
    rse = select_rse(A.moments[i], n);
    return n < A.max_n && (n < A.min_n || rse > A.threshold);
}
// 1: per block the sum of rse in double — k_frame_error's tree, so uniform counts give pt_frame_error's figure — and the number of
// selected pixels, from the four waves' ballots
__global__ void __launch_bounds__(256) k_select_count(const SelectArgs A, double* __restrict__ sums, uint32_t* __restrict__ n_sel) {
    float rse;
    const bool sel = select_pixel(A, blockIdx.x * 256u + threadIdx.x, rse);
    __shared__ double s_sum[256];
    __shared__ uint32_t s_wave[4];
    s_sum[threadIdx.x] = (double)rse;
    const unsigned long long vote = __ballot(sel);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(vote);
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[blockIdx.x] = s_sum[0]; n_sel[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]); }
}
// 2: one block turns the blocks' counts into their first list positions (an exclusive scan), 256 counts per round with the carry of
// the rounds before
__global__ void __launch_bounds__(256) k_select_scan(const uint32_t* __restrict__ n_sel, uint32_t n_blocks, uint32_t* __restrict__ base) {
    __shared__ uint32_t s_scan[2][256];
    uint32_t carry = 0u;
    for (uint32_t first = 0u; first < n_blocks; first += 256u) {
        const uint32_t b = first + threadIdx.x;
        const uint32_t v = b < n_blocks ? n_sel[b] : 0u;
        int cur = 0;
        s_scan[0][threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {   // inclusive, Hillis-Steele
            const uint32_t x = s_scan[cur][threadIdx.x] + ((int)threadIdx.x >= off ? s_scan[cur][threadIdx.x - off] : 0u);
            s_scan[cur ^ 1][threadIdx.x] = x;
            cur ^= 1;
            __syncthreads();
        }
        if (b < n_blocks) base[b] = carry + (s_scan[cur][threadIdx.x] - v);
        carry += s_scan[cur][255];
        __syncthreads();   // the next round overwrites the rows
    }
}
// 3: every selected pixel stores its number at the block's first position + the selected pixels before it in the block (the waves
// before its own through LDS, the lanes before it in its wave's ballot)
__global__ void __launch_bounds__(256) k_select_write(const SelectArgs A, const uint32_t* __restrict__ base, uint32_t* __restrict__ pixels) {
    float rse;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool sel = select_pixel(A, i, rse);
    __shared__ uint32_t s_wave[4];
    const unsigned long long vote = __ballot(sel);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) s_wave[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    if (!sel) return;
    uint32_t rank = base[blockIdx.x] + __builtin_amdgcn_mbcnt_hi((uint32_t)(vote >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vote, 0u));
    for (uint32_t w = 0; w < wave; w++) rank += s_wave[w];
    pixels[rank] = i;   // rank < the number selected <= n_pix
}

}  // namespace

using namespace ptmi;

extern "C" int pt_render_aux(pt_ctx* c, const pt_camera* cam, const pt_params* p, float* albedo_dev, float* normal_dev,
                             float* position_dev, int32_t* id_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!cam || !p || !albedo_dev || !normal_dev || !position_dev) return fail(c, PT_ERR_INVALID, "pt_render_aux: null argument");
    if (p->width < 1 || p->height < 1) return fail(c, PT_ERR_INVALID, "pt_render_aux: width and height must be >= 1");
    if (!c->tree.has_bvh) return fail(c, PT_ERR_NO_SCENE, "pt_render_aux: no BVH uploaded");
    if (c->tree.records_woop) return fail(c, PT_ERR_UNSUPPORTED, "pt_render_aux: the binary walk reads Moller-Trumbore records (upload with PT_OPT_TRI_TEST 0)");
    HIP_TRY(c, hipSetDevice(c->device));
    KParams P;
    std::memset(&P, 0, sizeof P);
    scene_view(c, P.sc, P.ksph);
    const size_t lds = binary_ray_layout(ctx_facts(c), P.sc);
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
    const dim3 grid((unsigned)((p->width + 15) / 16), (unsigned)((p->height + 15) / 16));
    hipLaunchKernelGGL(k_render_aux, grid, dim3(PT_BLOCK_RAYS), lds, c->stream, P, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_denoise(pt_ctx* c, const pt_denoise_params* dp, const float* color_dev, const float* albedo_dev,
                          const float* normal_dev, const float* position_dev, float* out_dev, uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!dp || !color_dev || !albedo_dev || !normal_dev || !position_dev || !out_dev) return fail(c, PT_ERR_INVALID, "pt_denoise: null argument");
    if (dp->width < 1 || dp->height < 1) return fail(c, PT_ERR_INVALID, "pt_denoise: width and height must be >= 1");
    if (dp->iterations < 0 || dp->iterations > 10) return fail(c, PT_ERR_INVALID, "pt_denoise: iterations must be 0..10");
    if (!std::isfinite(dp->sigma_color) || !std::isfinite(dp->sigma_normal) || !std::isfinite(dp->sigma_position))
        return fail(c, PT_ERR_INVALID, "pt_denoise: a sigma is not finite");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_pix = (size_t)dp->width * (size_t)dp->height;
    DnArgs A;
    std::memset(&A, 0, sizeof A);
    A.color = color_dev;
    A.albedo = (const float4*)albedo_dev;
    A.normal = (const float4*)normal_dev;
    A.position = (const float4*)position_dev;
    A.out = out_dev;
    A.rgba = rgba_dev;
    A.W = dp->width; A.H = dp->height;
    const dim3 grid((unsigned)((dp->width + PTD_TILE - 1) / PTD_TILE), (unsigned)((dp->height + PTD_TILE - 1) / PTD_TILE));
    const int L = dp->iterations;
    float4* ping[2] = {nullptr, nullptr};
    if (L > 0) {
        if (2 * n_pix > c->d_denoise.count()) HIP_TRY(c, hipStreamSynchronize(c->stream));   // the old frames may still be read by an earlier call's launches
        HIP_TRY(c, c->d_denoise.reserve(2 * n_pix));
        ping[0] = c->d_denoise.get();
        ping[1] = ping[0] + n_pix;
    }
    // log2(e) / sigma^2, in double; a term with sigma <= 0 is off (0); capped so that 0 x constant stays 0
    auto k_of = [](double sigma, double scale) -> float {
        if (!(sigma > 0.0)) return 0.f;
        return (float)std::min(1.4426950408889634 * scale / (sigma * sigma), 1e30);
    };
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (L == 0) {
        hipLaunchKernelGGL(k_dn_copy, grid, dim3(PTD_BLOCK), 0, st, A);
    } else {
        A.dst = ping[0];
        hipLaunchKernelGGL(k_dn_demod, grid, dim3(PTD_BLOCK), 0, st, A);
        A.kn = k_of(dp->sigma_normal, 1.0);
        A.kx = k_of(dp->sigma_position, 1.0);
        for (int l = 0; l < L; l++) {
            A.step = 1 << l;
            A.kc = k_of(dp->sigma_color, std::ldexp(1.0, 2 * l));   // (sigma_c 2^-l)^2 = sigma_c^2 / 4^l
            A.src = ping[l & 1];
            A.dst = ping[(l + 1) & 1];
            if (l + 1 < L) hipLaunchKernelGGL(k_dn_iter<false>, grid, dim3(PTD_BLOCK), 0, st, A);
            else hipLaunchKernelGGL(k_dn_iter<true>, grid, dim3(PTD_BLOCK), 0, st, A);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_denoise_variance(pt_ctx* c, const pt_denoise_variance_params* dp, const float* color_dev, const float* moments_dev,
                                   const float* length_dev, const float* albedo_dev, const float* normal_dev, const float* position_dev,
                                   float* out_dev, float* out_variance_dev, uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!dp || !color_dev || !albedo_dev || !normal_dev || !position_dev || !out_dev) return fail(c, PT_ERR_INVALID, "pt_denoise_variance: null argument");
    if (dp->width < 1 || dp->height < 1) return fail(c, PT_ERR_INVALID, "pt_denoise_variance: width and height must be >= 1");
    if (dp->iterations < 0 || dp->iterations > 10) return fail(c, PT_ERR_INVALID, "pt_denoise_variance: iterations must be 0..10");
    if (!std::isfinite(dp->sigma_luminance) || !std::isfinite(dp->sigma_normal) || !std::isfinite(dp->sigma_position))
        return fail(c, PT_ERR_INVALID, "pt_denoise_variance: a sigma is not finite");
    if (!moments_dev) return fail(c, PT_ERR_INVALID, "pt_denoise_variance: null moments");
    if (!std::isfinite(dp->samples_per_frame) || dp->samples_per_frame < 1.f)
        return fail(c, PT_ERR_INVALID, "pt_denoise_variance: samples_per_frame must be finite and >= 1");
    if (out_variance_dev) {
        const void* inputs[] = {color_dev, moments_dev, length_dev, albedo_dev, normal_dev, position_dev};
        for (const void* o : inputs)
            if (o == (const void*)out_variance_dev) return fail(c, PT_ERR_INVALID, "pt_denoise_variance: out_variance_dev may not be one of the inputs");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_pix = (size_t)dp->width * (size_t)dp->height;
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
    const dim3 grid((unsigned)((dp->width + PTD_TILE - 1) / PTD_TILE), (unsigned)((dp->height + PTD_TILE - 1) / PTD_TILE));
    const int L = dp->iterations;
    float4* ping[2] = {nullptr, nullptr};
    if (L > 0) {   // pt_denoise's scratch, by its rule
        if (2 * n_pix > c->d_denoise.count()) HIP_TRY(c, hipStreamSynchronize(c->stream));   // the old frames may still be read by an earlier call's launches
        HIP_TRY(c, c->d_denoise.reserve(2 * n_pix));
        ping[0] = c->d_denoise.get();
        ping[1] = ping[0] + n_pix;
    }
    auto k_of = [](double sigma) -> float {   // log2(e) / sigma^2, as pt_denoise
        if (!(sigma > 0.0)) return 0.f;
        return (float)std::min(1.4426950408889634 / (sigma * sigma), 1e30);
    };
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
        for (int l = 0; l < L; l++) {
            A.step = 1 << l;
            A.src = ping[l & 1];
            A.dst = ping[(l + 1) & 1];
            if (l + 1 < L) hipLaunchKernelGGL(k_dv_iter<false>, grid, dim3(PTD_BLOCK), 0, st, A);
            else hipLaunchKernelGGL(k_dv_iter<true>, grid, dim3(PTD_BLOCK), 0, st, A);
        }
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

namespace {

// What pt_temporal, pt_temporal_motion and pt_temporal_moments (with_length false: its payload writes no length) share: the argument checks (messages under the caller's name `fn`) and the kernel
// arguments of the reprojection.  PT_OK with A filled, or the error already recorded.
int temporal_args(pt_ctx* c, const std::string& fn, const pt_temporal_params* tp, const pt_camera* prev_cam, const float* prev_color_dev,
                  const float* prev_length_dev, const float* prev_normal_dev, const float* prev_position_dev, const int32_t* prev_id_dev,
                  const float* cur_color_dev, const float* cur_normal_dev, const float* cur_position_dev, const int32_t* cur_id_dev,
                  float* out_color_dev, float* out_length_dev, uint32_t* rgba_dev, TmArgs& A, bool with_length = true) {
    if (!tp || !cur_color_dev || !cur_normal_dev || !cur_position_dev || !out_color_dev || (with_length && !out_length_dev))
        return fail(c, PT_ERR_INVALID, fn + ": null argument");
    if (tp->width < 2 || tp->height < 2) return fail(c, PT_ERR_INVALID, fn + ": width and height must be >= 2");
    if (!std::isfinite(tp->max_history) || tp->max_history < 1.f) return fail(c, PT_ERR_INVALID, fn + ": max_history must be finite and >= 1");
    if (!std::isfinite(tp->plane_tolerance) || tp->plane_tolerance < 0.f)
        return fail(c, PT_ERR_INVALID, fn + ": plane_tolerance must be finite and >= 0");
    if (!(tp->normal_threshold >= -1.f && tp->normal_threshold <= 1.f)) return fail(c, PT_ERR_INVALID, fn + ": normal_threshold must be in -1..1");
    const bool history = prev_color_dev != nullptr;
    if (history) {
        if (!prev_cam || !prev_length_dev || !prev_normal_dev || !prev_position_dev)
            return fail(c, PT_ERR_INVALID, fn + ": a history needs its camera, lengths, normals and positions");
        if ((prev_id_dev == nullptr) != (cur_id_dev == nullptr)) return fail(c, PT_ERR_INVALID, fn + ": ids of both frames or of neither");
        if (out_color_dev == prev_color_dev || (with_length && out_length_dev == prev_length_dev))
            return fail(c, PT_ERR_INVALID, fn + ": the new history may not overwrite the old one (ping-pong the buffers)");
    }
    std::memset(&A, 0, sizeof A);
    A.cur_color = cur_color_dev;
    A.cur_normal = (const float4*)cur_normal_dev;
    A.cur_position = (const float4*)cur_position_dev;
    A.out_color = out_color_dev;
    A.out_len = out_length_dev;
    A.rgba = rgba_dev;
    A.W = tp->width; A.H = tp->height;
    if (history) {
        A.prev_color = prev_color_dev;
        A.prev_len = prev_length_dev;
        A.prev_normal = (const float4*)prev_normal_dev;
        A.prev_position = (const float4*)prev_position_dev;
        A.prev_id = prev_id_dev;
        A.cur_id = cur_id_dev;
        for (int i = 0; i < 3; i++) {
            A.pos[i] = prev_cam->pos[i]; A.front[i] = prev_cam->front[i]; A.right[i] = prev_cam->right[i]; A.up[i] = prev_cam->up[i];
        }
        // the inverse of pt_camera_ray's pixel mapping, every step one binary32 rounding
        A.sx = (float)(tp->width - 1) / (prev_cam->aspect * prev_cam->fov);
        A.sy = (float)(tp->height - 1) / prev_cam->fov;
        A.cx = (float)tp->width / 2.0f - 0.5f;
        A.cy = (float)tp->height / 2.0f - 0.5f;
        A.max_history = tp->max_history;
        A.plane_tol = tp->plane_tolerance;
        A.normal_thr = tp->normal_threshold;
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
    TmArgs A;
    if (int rc = temporal_args(c, "pt_temporal", tp, prev_cam, prev_color_dev, prev_length_dev, prev_normal_dev, prev_position_dev, prev_id_dev,
                               cur_color_dev, cur_normal_dev, cur_position_dev, cur_id_dev, out_color_dev, out_length_dev, rgba_dev, A))
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid((unsigned)((tp->width + PTD_TILE - 1) / PTD_TILE), (unsigned)((tp->height + PTD_TILE - 1) / PTD_TILE));
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
    TmMotionArgs M;
    std::memset(&M, 0, sizeof M);
    if (int rc = temporal_args(c, "pt_temporal_motion", tp, prev_cam, prev_color_dev, prev_length_dev, prev_normal_dev, prev_position_dev,
                               prev_id_dev, cur_color_dev, cur_normal_dev, cur_position_dev, cur_id_dev, out_color_dev, out_length_dev,
                               rgba_dev, M.t))
        return rc;
    const bool history = prev_color_dev != nullptr;
    if (history) {
        if (!prev_id_dev || !cur_id_dev) return fail(c, PT_ERR_INVALID, "pt_temporal_motion: the ids of both frames are required (they choose the vertex rows)");
        if (n_tris > 0 && (!prev_verts_dev || !cur_verts_dev)) return fail(c, PT_ERR_INVALID, "pt_temporal_motion: a null vertex buffer with n_tris > 0");
        if (n_tris >= ((size_t)1 << 31)) return fail(c, PT_ERR_INVALID, "pt_temporal_motion: n_tris must be < 2^31 (ids are int32)");
        if (motion_dev) {
            const void* others[] = {prev_verts_dev, cur_verts_dev, prev_color_dev, prev_length_dev, prev_normal_dev, prev_position_dev, prev_id_dev,
                                    cur_color_dev, cur_normal_dev, cur_position_dev, cur_id_dev, out_color_dev, out_length_dev, rgba_dev};
            for (const void* o : others)
                if (o == (const void*)motion_dev) return fail(c, PT_ERR_INVALID, "pt_temporal_motion: motion_dev may not be one of the other buffers");
        }
        M.prev_verts = prev_verts_dev;
        M.cur_verts = cur_verts_dev;
        M.n_tris = (uint32_t)n_tris;
    }
    M.motion = (float2*)motion_dev;
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid((unsigned)((tp->width + PTD_TILE - 1) / PTD_TILE), (unsigned)((tp->height + PTD_TILE - 1) / PTD_TILE));
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
    TmMotionArgs M;
    std::memset(&M, 0, sizeof M);
    if (int rc = temporal_args(c, "pt_temporal_moments", tp, prev_cam, prev_moments_dev, prev_length_dev, prev_normal_dev, prev_position_dev,
                               prev_id_dev, cur_moments_dev, cur_normal_dev, cur_position_dev, cur_id_dev, out_moments_dev, nullptr, nullptr,
                               M.t, false))
        return rc;
    const bool history = prev_moments_dev != nullptr;
    const bool motion = prev_verts_dev != nullptr || cur_verts_dev != nullptr;   // pt_temporal_motion's rule
    if (history && motion) {
        if (!prev_id_dev || !cur_id_dev) return fail(c, PT_ERR_INVALID, "pt_temporal_moments: the ids of both frames are required (they choose the vertex rows)");
        if (n_tris > 0 && (!prev_verts_dev || !cur_verts_dev)) return fail(c, PT_ERR_INVALID, "pt_temporal_moments: a null vertex buffer with n_tris > 0");
        if (n_tris >= ((size_t)1 << 31)) return fail(c, PT_ERR_INVALID, "pt_temporal_moments: n_tris must be < 2^31 (ids are int32)");
        M.prev_verts = prev_verts_dev;
        M.cur_verts = cur_verts_dev;
        M.n_tris = (uint32_t)n_tris;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid((unsigned)((tp->width + PTD_TILE - 1) / PTD_TILE), (unsigned)((tp->height + PTD_TILE - 1) / PTD_TILE));
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (!history || motion) hipLaunchKernelGGL((k_temporal_moments<true, 1>), grid, dim3(PTD_BLOCK), 0, st, M);   // (no history: out = cur)
    else if (M.t.prev_id) hipLaunchKernelGGL((k_temporal_moments<true, 0>), grid, dim3(PTD_BLOCK), 0, st, M);
    else hipLaunchKernelGGL((k_temporal_moments<false, 0>), grid, dim3(PTD_BLOCK), 0, st, M);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_frame_error(pt_ctx* c, const float* moments_dev, int32_t width, int32_t height, uint64_t n_samples, float threshold,
                              double* mean_rse, uint64_t* n_above) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!moments_dev || (!mean_rse && !n_above)) return fail(c, PT_ERR_INVALID, "pt_frame_error: null argument");
    if (width < 1 || height < 1) return fail(c, PT_ERR_INVALID, "pt_frame_error: width and height must be >= 1");
    if (n_samples < 2) return fail(c, PT_ERR_INVALID, "pt_frame_error: the standard error needs n_samples >= 2");
    if (!std::isfinite(threshold) || threshold < 0.f) return fail(c, PT_ERR_INVALID, "pt_frame_error: threshold must be finite and >= 0");
    const size_t n_pix = (size_t)width * (size_t)height;
    if (n_pix > 0xffffffffull) return fail(c, PT_ERR_INVALID, "pt_frame_error: more than 2^32 - 1 pixels");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_blocks = (n_pix + 255) / 256;
    const size_t need = n_blocks * (sizeof(double) + sizeof(uint32_t));
    HIP_TRY(c, c->d_frame_err.reserve(need));   // (no wait: nothing reads the old slots, every earlier call synchronised before it returned)
    double* d_sums = (double*)c->d_frame_err.get();
    uint32_t* d_counts = (uint32_t*)(d_sums + n_blocks);
    hipLaunchKernelGGL(k_frame_error, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, (const float2*)moments_dev, (uint32_t)n_pix,
                       (float)(n_samples - 1), threshold, d_sums, d_counts);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned char> h(need);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_frame_err.get(), need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double* sums = (const double*)h.data();
    const uint32_t* counts = (const uint32_t*)(sums + n_blocks);
    double total = 0.0;
    uint64_t above = 0;
    for (size_t b = 0; b < n_blocks; b++) { total += sums[b]; above += counts[b]; }   // in block order: reproducible
    if (mean_rse) *mean_rse = total / (double)n_pix;
    if (n_above) *n_above = above;
    return PT_OK;
}

extern "C" int pt_select_pixels(pt_ctx* c, const pt_select_params* sp, const float* moments_dev, const uint32_t* counts_dev,
                                uint32_t* pixels_dev, uint64_t* n_selected, double* mean_rse) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    uint64_t n_pix = 0;
    const Refusal r = check_select_call(sp, moments_dev && counts_dev && pixels_dev && n_selected, n_pix);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    const SelectPlan plan = plan_select(n_pix);
    const size_t n_blocks = plan.n_blocks, back = plan.read_back;   // what the host reads: the sums and the counts
    HIP_TRY(c, c->d_select.reserve(plan.scratch));   // (no wait: every earlier call synchronised before it returned)
    double* d_sums = (double*)c->d_select.get();
    uint32_t* d_nsel = (uint32_t*)(d_sums + n_blocks);
    uint32_t* d_base = d_nsel + n_blocks;
    const SelectArgs A{(const float2*)moments_dev, counts_dev, (uint32_t)n_pix, std::max(sp->min_samples, 2u), sp->max_samples, sp->threshold};
    HIP_TRY(c, span_begin(c));
    hipLaunchKernelGGL(k_select_count, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, A, d_sums, d_nsel);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(256), 0, c->stream, (const uint32_t*)d_nsel, (uint32_t)n_blocks, d_base);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_select_write, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, A, (const uint32_t*)d_base, pixels_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    std::vector<unsigned char> h(back);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_select.get(), back, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double* sums = (const double*)h.data();
    const uint32_t* n_sel = (const uint32_t*)(sums + n_blocks);
    double total = 0.0;
    uint64_t selected = 0;
    for (size_t b = 0; b < n_blocks; b++) { total += sums[b]; selected += n_sel[b]; }   // in block order: reproducible
    *n_selected = selected;
    if (mean_rse) *mean_rse = total / (double)n_pix;
    return PT_OK;
}

namespace {

// T[0] = 0, T[k] = eotf((k - 0.5) / 255) in double, rounded once to binary32 (include/ptmi.h)
void tone_thresholds(int transfer, float* T) {
    T[0] = 0.0f;
    for (int k = 1; k < 256; k++) {
        const double v = ((double)k - 0.5) / 255.0;
        const double lin = transfer == PT_XFER_SRGB ? (v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4)) : std::pow(v, 2.2);
        T[k] = (float)lin;
    }
}
struct ToneTables {
    float t[2][256];   // PT_XFER_SRGB, PT_XFER_GAMMA22
    ToneTables() { tone_thresholds(PT_XFER_SRGB, t[0]); tone_thresholds(PT_XFER_GAMMA22, t[1]); }
};
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0u; }   // (a null pointer counts as aligned)

}  // namespace

extern "C" int pt_tonemap_thresholds(int transfer, float* out256) {
    if (!out256) return fail(nullptr, PT_ERR_INVALID, "pt_tonemap_thresholds: null argument");
    if (transfer != PT_XFER_SRGB && transfer != PT_XFER_GAMMA22)
        return fail(nullptr, PT_ERR_INVALID, "pt_tonemap_thresholds: transfer must be PT_XFER_SRGB or PT_XFER_GAMMA22 (PT_XFER_LINEAR has no table)");
    tone_thresholds(transfer, out256);
    return PT_OK;
}

extern "C" int pt_tonemap(pt_ctx* c, const pt_tonemap_params* tp, const float* color_dev, const float* exposure_dev, float* out_dev,
                          uint32_t* rgba_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    uint64_t n_pix = 0;
    const Refusal r = check_tonemap_call(tp, color_dev && (out_dev || rgba_dev), n_pix);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    const bool table = rgba_dev && tp->transfer != PT_XFER_LINEAR;
    if (table && !c->d_tone) {   // once per context, and complete before this returns: later calls on any stream read it
        static const ToneTables tables;
        HIP_TRY(c, c->d_tone.alloc(2 * 256));
        const hipError_t e = hipMemcpy(c->d_tone.get(), tables.t, sizeof tables.t, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            c->d_tone.reset();
            return hip_fail(c, e, "pt_tonemap: uploading the threshold tables");
        }
    }
    const DisplayPlan plan = plan_tonemap(n_pix, aligned16(color_dev) && aligned16(out_dev) && aligned16(rgba_dev));
    ToneArgs A;
    std::memset(&A, 0, sizeof A);
    A.color = color_dev;
    A.exposure = exposure_dev;
    A.table = table ? c->d_tone.get() + (tp->transfer == PT_XFER_SRGB ? 0 : 256) : nullptr;
    A.out = out_dev;
    A.rgba = rgba_dev;
    A.n_items = (uint32_t)plan.items;
    A.curve = tp->curve;
    A.e = tp->exposure;
    A.iw2 = (tp->curve != PT_TONE_REINHARD || tp->white == INFINITY) ? 0.0f : 1.0f / (tp->white * tp->white);
    HIP_TRY(c, span_begin(c));
    with_bool(table, [&](auto T) {
        with_bool(plan.vec, [&](auto V) {
            hipLaunchKernelGGL((k_tonemap<decltype(T)::value, decltype(V)::value>), dim3(plan.n_blocks), dim3(256), 0, c->stream, A);
        });
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

extern "C" int pt_meter(pt_ctx* c, const pt_meter_params* mp, const float* color_dev, float* state_dev, int reset) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    uint64_t n_pix = 0;
    const Refusal r = check_meter_call(mp, color_dev && state_dev, n_pix);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_meter.reserve(METER_SCRATCH_WORDS));   // its one size: no wait, nothing is ever released
    const DisplayPlan plan = plan_meter(n_pix, aligned16(color_dev));
    MeterArgs A;
    std::memset(&A, 0, sizeof A);
    A.partial = c->d_meter.get();
    A.state = state_dev;
    A.n_blocks = plan.n_blocks;
    A.key = mp->key; A.low_pct = mp->low_pct; A.high_pct = mp->high_pct;
    A.min_exposure = mp->min_exposure; A.max_exposure = mp->max_exposure; A.adapt = mp->adapt;
    A.reset = reset != 0;
    HIP_TRY(c, span_begin(c));
    if (plan.vec) hipLaunchKernelGGL(k_meter_hist<true>, dim3(plan.n_blocks), dim3(256), 0, c->stream, color_dev, (uint32_t)plan.items, c->d_meter.get());
    else hipLaunchKernelGGL(k_meter_hist<false>, dim3(plan.n_blocks), dim3(256), 0, c->stream, color_dev, (uint32_t)plan.items, c->d_meter.get());
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_meter_finish, dim3(1), dim3(256), 0, c->stream, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, span_end(c));
    return PT_OK;
}
