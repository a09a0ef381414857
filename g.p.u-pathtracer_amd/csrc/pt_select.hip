// pt_select.hip — the error figures of a frame's luminance moments: pt_frame_error and pt_select_pixels, adaptive
// sampling's pixel list (§10 f18); include/ptmi.h states the formulas.  One translation unit of libptmi.so (pt_ctx.h).
//   k_frame_error    one lane per pixel, the relative standard error of the mean luminance from the moments pt_render_moments
//                    keeps; a block adds its 256 values up in LDS, in double, and writes ONE partial sum and ONE count to its own
//                    slot — the host adds the slots in block order
//   k_select_count, k_select_scan, k_select_write  k_frame_error's figure with each pixel's own sample count and the rule "needs
//                    more samples", over the same blocks — per block the sum and the number of selected pixels (wave ballots),
//                    one block's exclusive scan of those numbers, then every selected pixel stores its number at its rank: an
//                    ascending list without atomics and without a block that waits for another
// The sums and the list are the same run after run: no block waits for another and nothing is added atomically.
#include <cmath>
#include <vector>

#include "pt_image.h"

namespace {

// rse of pixel i in binary32; per block the sum of rse in double and the number of pixels above the threshold, by the tree
// reduction of k_tree_cost (pt_tree.hip)
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
    ptd_block_sum(s_sum, s_cnt);
    if (threadIdx.x == 0) { sums[blockIdx.x] = s_sum[0]; counts[blockIdx.x] = s_cnt[0]; }
}

// ---- pt_select_pixels: three launches over the same 256-pixel blocks
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
    ptd_block_sum(s_sum);
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
        const int cur = ptd_block_scan(s_scan, v);
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

using namespace ptmi;

// What both calls end with: the blocks' sums (double) and counts (uint32, behind the sums), the first `back` bytes of `scratch`,
// read back once the stream has run dry and added in block order — reproducible.  PT_OK, or the error already recorded.
int read_back_block_sums(pt_ctx* c, const char* scratch, size_t n_blocks, size_t back, double& total, uint64_t& count) {
    std::vector<unsigned char> h(back);
    HIP_TRY(c, hipMemcpyAsync(h.data(), scratch, back, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double* sums = (const double*)h.data();
    const uint32_t* counts = (const uint32_t*)(sums + n_blocks);
    total = 0.0;
    count = 0;
    for (size_t b = 0; b < n_blocks; b++) { total += sums[b]; count += counts[b]; }
    return PT_OK;
}

}  // namespace

extern "C" int pt_frame_error(pt_ctx* c, const float* moments_dev, int32_t width, int32_t height, uint64_t n_samples, float threshold,
                              double* mean_rse, uint64_t* n_above) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    uint64_t n_pix = 0;
    const Refusal r = check_frame_error_call(moments_dev && (mean_rse || n_above), width, height, n_samples, threshold, n_pix);   // (pt_plan.h)
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_blocks = (n_pix + 255) / 256;
    const size_t need = n_blocks * (sizeof(double) + sizeof(uint32_t));
    HIP_TRY(c, c->d_frame_err.reserve(need));   // (no wait: nothing reads the old slots, every earlier call synchronised before it returned)
    double* d_sums = (double*)c->d_frame_err.get();
    uint32_t* d_counts = (uint32_t*)(d_sums + n_blocks);
    hipLaunchKernelGGL(k_frame_error, dim3((unsigned)n_blocks), dim3(256), 0, c->stream, (const float2*)moments_dev, (uint32_t)n_pix,
                       (float)(n_samples - 1), threshold, d_sums, d_counts);
    HIP_TRY(c, hipGetLastError());
    double total;
    uint64_t above;
    if (int rc = read_back_block_sums(c, c->d_frame_err.get(), n_blocks, need, total, above)) return rc;
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
    const size_t n_blocks = plan.n_blocks;
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
    double total;
    uint64_t selected;
    if (int rc = read_back_block_sums(c, c->d_select.get(), n_blocks, plan.read_back, total, selected)) return rc;
    *n_selected = selected;
    if (mean_rse) *mean_rse = total / (double)n_pix;
    return PT_OK;
}
