// pt_display.hip — the display stage (include/ptmi.h states the arithmetic, tests/tonemap_ref.py restates it):
// pt_tonemap, pt_tonemap_thresholds and pt_meter.  One translation unit of libptmi.so (pt_ctx.h).
//   k_tonemap<TABLE, VEC>  exposure, curve and display word of one pixel per thread, or of four (VEC: three dwordx4 loads, one
//                    dwordx4 store of words); TABLE: the transfer's 256 thresholds staged in LDS once per block and searched in
//                    eight branch-free steps per channel — no pow on the device
//   k_meter_hist<VEC>, k_meter_finish  a fixed grid's luminance histograms (257 counters in LDS, integer LDS adds, one row of
//                    plain stores per block), then one block that adds the rows, scans the bins, trims, and leaves the exposure
//                    in the caller's four floats — nothing returns to the host
// Both are bandwidth-bound — 12 bytes read per pixel, 4 or 12 written — so the VEC routes move a thread's four pixels as three
// dwordx4 loads (and three dwordx4 stores, one dwordx4 store of words); the scalar routes serve buffers that are not 16-byte aligned
// and pixel counts that do not come in fours.  Plain *, + and /: one binary32 rounding per step.
#include <cmath>
#include <cstring>

#include "pt_image.h"

namespace {

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
        const float L = ptd_lum(r, g, b);
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
    const float L = ptd_lum(r, g, b);
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
    const int cur = ptd_block_scan(s_scan, count);   // (the counts add up to < 2^32)
    const long long cum = (long long)s_scan[cur][b], before = cum - (long long)count, n = (long long)s_scan[cur][255];
    long long lo = (long long)(unsigned long long)((double)A.low_pct * (double)n);
    long long hi = (long long)(unsigned long long)((double)A.high_pct * (double)n);
    if (hi <= lo) { lo = 0; hi = n; }
    const long long span = (cum < hi ? cum : hi) - (before > lo ? before : lo);
    const unsigned long long w = span > 0 ? (unsigned long long)span : 0ull;
    s_S[b] = w * (2ull * b + 1ull);
    s_W[b] = w;
    ptd_block_sum(s_S, s_W);
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

}  // namespace

using namespace ptmi;

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
