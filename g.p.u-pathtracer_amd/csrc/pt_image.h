// pt_image.h — what more than one of the image stages uses (pt_aux.hip, pt_filter.hip, pt_temporal.hip, pt_select.hip,
// pt_display.hip): the 16x16 pixel tile and its grid, the demodulation's divisor, the Rec. 709 luminance, the "store colour and
// optional display word" pair, and a 256-thread block's tree sum and inclusive scan in LDS.  Every device helper is forced inline
// and takes its small arguments by value, so a kernel that calls one compiles to what it held written out.
#pragma once
#include "pt_ctx.h"

#define PTD_TILE 16
#define PTD_BLOCK (PTD_TILE * PTD_TILE)

namespace {

// the launch grid of one lane per pixel in 16x16 tiles
inline dim3 ptd_grid(int w, int h) { return dim3((unsigned)((w + PTD_TILE - 1) / PTD_TILE), (unsigned)((h + PTD_TILE - 1) / PTD_TILE)); }

// the lane's pixel; false outside the image
template <class Args>
__device__ __forceinline__ bool ptd_pixel(const Args& A, int& x, int& y) {
    x = blockIdx.x * PTD_TILE + (threadIdx.x & (PTD_TILE - 1));
    y = blockIdx.y * PTD_TILE + (threadIdx.x / PTD_TILE);
    return x < A.W && y < A.H;
}
__device__ __forceinline__ float ptd_demod_div(float a) { return a > 1e-3f ? a : 1.0f; }
// Rec. 709 luminance, in this order of operations (pt_shade.h's pt_moments states it too)
__device__ __forceinline__ float ptd_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// pixel p of a float[H][W][3] buffer, and its display word where the caller asked for words
__device__ __forceinline__ void ptd_store(float* out, uint32_t* rgba, size_t p, float r, float g, float b) {
    out[3 * p] = r; out[3 * p + 1] = g; out[3 * p + 2] = b;
    if (rgba) rgba[p] = pt_pack_rgba(r, g, b);
}

// The sum of a 256-thread block's values by a tree in LDS: every thread has stored its own at s[threadIdx.x] (no barrier yet);
// afterwards s[0] holds the sum, in the same order of additions run after run.  Several arrays share the barriers.
template <class... T>
__device__ __forceinline__ void ptd_block_sum(T*... s) {
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) ((s[threadIdx.x] += s[threadIdx.x + off]), ...);
        __syncthreads();
    }
}
// The inclusive scan (Hillis-Steele) of a 256-thread block's values v over two LDS rows: returns the row r whose s[r][i] holds
// v_0 + ... + v_i; every thread may read any entry of it at once.
__device__ __forceinline__ int ptd_block_scan(uint32_t (*s)[256], uint32_t v) {
    int cur = 0;
    s[0][threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t x = s[cur][threadIdx.x] + ((int)threadIdx.x >= off ? s[cur][threadIdx.x - off] : 0u);
        s[cur ^ 1][threadIdx.x] = x;
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

}  // namespace
