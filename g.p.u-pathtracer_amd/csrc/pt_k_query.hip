// pt_k_query.hip — bounded closest-hit and any-hit queries on a caller's ray batch: pt_closest_hits, pt_any_hits.
// One translation unit of libptmi.so (pt_ctx.h).  DESIGN.md §10 f9.
//
// k_query_rays is the extend stage of the stage-split pipeline (k_wf_extend, pt_k_wave.hip) without a pipeline around it: persistent
// waves on a resident grid draw regions of PT_REGION consecutive rays from PT_SHARDS counters, idle lanes take the next rays by a
// ballot + prefix count (v_mbcnt), a lane's whole state is one ray and the walk (8 waves per SIMD), and the walk is the pipeline's —
// trav_run_wide over the 4-wide tree with the second record of a leaf requested ahead, as it stands in pt_walks.h.  A ray is
// (o, ignored, d, t_max): the lane starts with h.t = min(t_max, F32_MAX), so the walk's own `t < h.t` is the bound, strict, and
// the boxes beyond it are never opened.  A ray whose t_max is not greater than 0 (0, negative, NaN) writes its miss where it is
// drawn and never becomes live.
//
// A tree too deep for the wide walk's stack (wide_walk_fits, pt_plan.h: the rule of every call) takes k_query_rays_bvh2: the binary walk
// of pt_trace_rays, unbounded, and the bound applied to its answer — the nearest hit inside (0, t_max) is the nearest hit when it
// lies inside and nothing otherwise, so both kernels give the same results.
#include <cstring>

#include "pt_ctx.h"

struct KQuery {
    KScene sc;
    const float4* __restrict__ rays;   // [n][2]: (o.xyz, ignored) (d.xyz, t_max)
    float* __restrict__ t_out;         // closest: t, F32_MAX on a miss
    int* __restrict__ tri_out;         //          original triangle id, -1 on a miss
    float* __restrict__ n_out;         //          [n][3] the winner's un-normalised normal, 0 on a miss; may be null
    uint8_t* __restrict__ hit_out;     // any: 1 = a triangle inside (0, t_max), else 0
    unsigned int* queue;               // PT_SHARDS counters, zero at launch
    uint32_t n, n_regions;
    int cull, batch;
};

template <bool ANY>
__device__ __forceinline__ void query_write_miss(const KQuery& Q, size_t i) {
    if (ANY) {
        Q.hit_out[i] = 0;
    } else {
        float z = 0.f;
        asm volatile("" : "+v"(z));   // made here: as a constant hipcc keeps three zeroed VGPRs (spilled) through the whole kernel
        Q.t_out[i] = PT_F32_MAX;
        Q.tri_out[i] = -1;
        if (Q.n_out) { Q.n_out[3 * i] = z; Q.n_out[3 * i + 1] = z; Q.n_out[3 * i + 2] = z; }
    }
}

// h: the walk's result for a ray that was walked with the bound in h.t (h.tri = -1: nothing inside the bound, h.t still the bound)
__device__ __forceinline__ void query_write_closest(const KQuery& Q, size_t i, const Hit& h) {
    const bool hit = h.tri != -1;
    Q.t_out[i] = hit ? h.t : PT_F32_MAX;
    Q.tri_out[i] = h.tri;
    if (Q.n_out) {
        const v3 hn = hit ? pt_hit_normal(Q.sc, h) : V3(0.f, 0.f, 0.f);
        Q.n_out[3 * i] = hn.x; Q.n_out[3 * i + 1] = hn.y; Q.n_out[3 * i + 2] = hn.z;
    }
}

// The walk prunes a box whose entry distance exceeds h.t, and here h.t is the caller's bound, not a hit's own t.  A box's entry
// distance, fma(plane, 1 / d, -o / d) on quantised planes, is not rounded as Moller-Trumbore's t is: three roundings, each up to
// u = 2^-24 of |plane / d| or |o / d|, and on the axis that decides the entry |plane / d| <= |o / d| + t.  So a hit just below the
// bound, on a face of its box, would be pruned with its box (walls that are the scene's bounds: a few per cent of such rays).
// The ray's box-test terms — idx .. oodz, which only the box tests read — are therefore scaled by 1 - eps,
//     eps = 8 u (2 max|o / d| / bound + 1), at most 1/2,
// which moves every box distance towards 0 by more than its rounding error and the triangle's together (8 u where 3 + 3 are needed),
// keeps every sign and the order of the entry keys, and leaves the triangle tests and their strict `t < bound` exact: a few more
// boxes are opened, no answer changes but those the rounding took.  An unbounded ray gets eps = 8 u.
__device__ __forceinline__ void query_widen_boxes(TravState& ts) {
    const float m = fmaxf(fmaxf(fabsf(ts.oodx), fabsf(ts.oody)), fabsf(ts.oodz));
    const float eps = fminf(4.76837158203125e-07f * (2.0f * m / ts.h.t + 1.0f), 0.5f);   // 8 x 2^-24
    const float k = 1.0f - eps;
    ts.idx *= k; ts.idy *= k; ts.idz *= k;
    ts.oodx *= k; ts.oody *= k; ts.oodz *= k;
}

// ANY: trav_run_wide<.., ANY> — the lane leaves at the first record it accepts, with h.t = 0.
// V: the word of pt_variants.h (QV_*; query_exists: what is instantiated)
template <uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK, budget_occ(qv_budget(V))) k_query_rays(const KQuery Q) {
    constexpr bool ANY = qv_any(V);
    constexpr int LSTK = budget_lstk(qv_budget(V));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    TravOverflow<LSTK> stk_ovf;
    TravStack<LSTK, PT_BLOCK> stk(__builtin_amdgcn_readfirstlane(tid & ~63), stk_ovf);
    const bool cull = Q.cull != 0;
    const uint32_t n_regions = Q.n_regions;
    const uint32_t shard_regions = (n_regions + PT_SHARDS - 1) / PT_SHARDS;
    const int batch = Q.batch;

    uint32_t next = 0, end = 0;   // wave-uniform: the part of the wave's region not handed to lanes yet
    bool empty = false;           // wave-uniform: every shard of the queue is exhausted
    int shard = (int)(blockIdx.x & (PT_SHARDS - 1));

    bool live = false;
    uint32_t idx = 0;
    v3 o = V3(0.f, 0.f, 0.f), d = V3(0.f, 0.f, 0.f);
    TravState ts;
    ts.idx = ts.idy = ts.idz = ts.oodx = ts.oody = ts.oodz = 0.f;
    ts.node = PT_SENTINEL; ts.leaf = 0; ts.sp = 0;
    ts.h = pt_no_hit();
    TravCount tc;

    for (;;) {
        // ---- refill: idle lanes take the next rays of the wave's region(s); lane -> ray by a ballot + prefix count (v_mbcnt) of the
        // idle mask
        const unsigned long long idle = __ballot(!live);
        const int n_idle = __popcll(idle);
        if (!empty && (n_idle >= batch || n_idle == 64)) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            uint32_t served = 0;
            for (int round = 0; round < 8 && served < (uint32_t)n_idle; round++) {
                if (next == end) {
                    // shard s owns regions s, s + 8, ...; an empty shard is left for the next one (as k_wf_extend)
                    bool got = false;
                    for (int tries = 0; tries < PT_SHARDS && !got; tries++) {
                        uint32_t k = 0;
                        if (lane == 0) k = atomicAdd(Q.queue + shard * PT_SHARD_STRIDE, 1u);
                        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
                        const uint32_t r = k * PT_SHARDS + (uint32_t)shard;
                        if (k < shard_regions && r < n_regions) {
                            next = r * PT_REGION;
                            end = (uint32_t)min((unsigned long long)next + PT_REGION, (unsigned long long)Q.n);   // (n < 2^32)
                            got = true;
                        } else {
                            shard = (shard + 1) & (PT_SHARDS - 1);
                        }
                    }
                    if (!got) { empty = true; break; }
                }
                const uint32_t take = min((uint32_t)n_idle - served, end - next);
                if (!live && rank >= served && rank < served + take) {
                    idx = next + (rank - served);
                    const float4 a = pt_sld4(Q.rays + 2 * (size_t)idx), b = pt_sld4(Q.rays + 2 * (size_t)idx + 1);
                    o = V3(a.x, a.y, a.z);
                    d = V3(b.x, b.y, b.z);
                    trav_begin(ts, o, d, stk, Q.sc.wide_root);
                    ts.h.t = fminf(b.w, PT_F32_MAX);
                    query_widen_boxes(ts);
                    // not greater than 0 — 0, negative, NaN — is a miss that never becomes live (t_max itself is tested: the fminf
                    // drops a NaN).  Every drawn lane sets the walk up, so that no value of the walk's state depends on the branch.
                    live = b.w > 0.0f;
                    if (!live) query_write_miss<ANY>(Q, (size_t)idx);
                }
                next += take;
                served += take;
            }
        }
        const unsigned long long busy = __ballot(live);
        if (!busy) {
            if (empty) break;
            continue;
        }
        // ---- walk until `batch` lanes have finished (lanes that can get no more work do not count)
        const int n_dead = empty ? 64 - __popcll(busy) : 0;
        if (live) {
            const bool fin = trav_run_wide<TW_DYN | TW_AHEAD | (ANY ? TW_ANY : 0u)>(ts, Q.sc, o, d, cull, stk, tc, n_dead, batch);
            if (fin) {
                if (ANY) Q.hit_out[idx] = ts.h.t == 0.0f ? 1 : 0;
                else query_write_closest(Q, (size_t)idx, ts.h);
                live = false;
            }
        }
    }
}

// The deep-tree fallback: k_trace_rays_bvh2's walk (one thread per ray, all 72 stack entries and the top of the tree in LDS),
// then the bound.
__global__ void __launch_bounds__(PT_BLOCK_RAYS) k_query_rays_bvh2(const KQuery Q) {
    float4* s_top = s_dyn;
    lds_load_top<PT_BLOCK_RAYS>(Q.sc, s_top);
    const size_t i = (size_t)blockIdx.x * PT_BLOCK_RAYS + threadIdx.x;
    if (i >= (size_t)Q.n) return;
    const float4 ro = Q.rays[2 * i], rd = Q.rays[2 * i + 1];
    Hit h = pt_no_hit();
    if (rd.w > 0.0f) {
        TravCount tc;
        TravOverflow<PT_STACK_CAP> stk_ovf;
        TravStack<PT_STACK_CAP, PT_BLOCK_RAYS> stk(__builtin_amdgcn_readfirstlane(16 * Q.sc.n_top + ((int)threadIdx.x & ~63)), stk_ovf);
        h = trav_bvh2<TW_TOP>(Q.sc, V3(ro.x, ro.y, ro.z), V3(rd.x, rd.y, rd.z), Q.cull != 0, stk, tc, s_top);
        if (!(h.t < fminf(rd.w, PT_F32_MAX))) h = pt_no_hit();   // (a miss holds F32_MAX, never below the bound)
    }
    if (Q.hit_out) Q.hit_out[i] = h.tri != -1 ? 1 : 0;
    else query_write_closest(Q, i, h);
}

namespace ptmi {

hipError_t launch_query(pt_ctx* c, const QueryPlan& plan, const QueryCall& q) {
    KQuery Q;
    std::memset(&Q, 0, sizeof Q);
    scene_view(c, Q.sc);
    Q.rays = (const float4*)q.rays;
    Q.t_out = q.t; Q.tri_out = q.tri; Q.n_out = q.normal; Q.hit_out = q.hit;
    Q.queue = c->d_queue.get();   // the context's counters: every use is on the caller's stream, behind a reset of its own
    Q.n = (uint32_t)q.n;
    Q.n_regions = plan.n_regions;
    Q.cull = q.cull;
    Q.batch = plan.batch;
    hipStream_t st = c->stream;
    if (!plan.wide) {   // pt_trace_rays' launch
        Q.sc.stack_n = PT_STACK_CAP; Q.sc.top_base = 0; Q.sc.n_top = plan.n_top;
        const size_t lds = plan.lds;
        const hipError_t e = allow_lds(k_query_rays_bvh2, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_query_rays_bvh2, dim3((unsigned)((q.n + PT_BLOCK_RAYS - 1) / PT_BLOCK_RAYS)), dim3(PT_BLOCK_RAYS), lds, st, Q);
        return hipGetLastError();
    }
    const hipError_t e = queue_reset(Q.queue, st);
    if (e != hipSuccess) return e;
    return with_variant<query_exists, QV_BITS>(plan.word, [&](auto v) {
        Q.sc.stack_n = budget_lstk(qv_budget(v()));
        return launch_resident(k_query_rays<v()>, plan.lds, plan.blocks_per_cu, plan.n_cu, (size_t)Q.n_regions, st, Q);
    });
}

}  // namespace ptmi
