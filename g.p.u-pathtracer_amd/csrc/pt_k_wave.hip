// pt_k_wave.hip — the stage-split ("wavefront") frame pipeline, PT_KERNEL_WAVEFRONT.
// One translation unit of libptmi.so (pt_ctx.h).
//
// BASELINE.json configs[4] / SURVEY.md §7 step 5e: "ray buffers in SoA, extend / shade / generate
// kernels, ballot + prefix-sum compaction of live rays between bounces".  The reference has nothing
// like it (one thread per pixel, tracer.cu:413-414); the arithmetic of a path is the reference's
// (path_begin / trav_run_wide / path_shade_hit are the functions the other frame kernels call), so the
// images are the same bit for bit — only WHERE a path's state lives between segments differs:
//
//   bounce 0   works on SLOTS, one per (sample, pixel) in the tile order of the other frame kernels: both stages
//              compute the camera ray from the slot number (a few dozen instructions) instead of a generate
//              kernel writing 32-byte ray records for them to read back; the shade stage of bounce 0 WRITES
//              the sample colour (accu = 0 + emission) instead of adding to a zeroed one
//   per bounce
//     extend   persistent waves: a wave draws REGIONS of the ray queue from eight sharded counters,
//              walks the BVH for 64 rays at a time and refills a lane as soon as its ray is done (its whole
//              per-lane state is one ray + the walk: no path state, 8 waves per SIMD); writes (t, record)
//     shade    one lane per live record, every wave full: spheres, shading, BRDF sample (tracer.cu:98-296);
//              emitted light is added to the sample colour in place, a miss writes the background
//              (tracer.cu:140-142), survivors are packed to the front of their region's next generation with
//              a ballot + prefix count (v_mbcnt) — dead paths cost nothing in the next stage; survivors whose new ray
//              the tree's root turns away are packed behind the others and never queued (PT_OPT_ROOT_CULL)
//   PT_OPT_PATH_HISTORY (the default where it holds: path_history_holds, pt_plan.h): the record carries which objects the path has
//              hit instead of its mask, the shade lane rebuilds mask and accu from that word, and the sample colour is written once,
//              by the lane the path ends in — no write at bounce 0 for a path that goes on, no add in place
//   k_fold_samples folds the sample colours into the running mean (tracer.cu:386-391), as for every kernel.
// Which of the kernels below a bounce runs: WavePlan, at the end of the file.  Why the split pays: DESIGN.md §5.2.
#include "pt_ctx.h"

// ------------------------------------------------------------------------------------------------
// block-level compaction: exclusive rank of the calling lane among the block's lanes with keep == true,
// and the block's total.  Four waves: ballot + v_mbcnt inside a wave, one LDS word per wave.
__device__ __forceinline__ int wf_block_rank(bool keep, int& total, int* s_cnt) {
    const unsigned long long m = __ballot(keep);
    const int w = threadIdx.x >> 6;
    const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if ((threadIdx.x & 63) == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < PT_BLOCK / 64; k++) {
        const int c = s_cnt[k];
        if (k < w) base += c;
        tot += c;
    }
    total = tot;
    return base + in_wave;
}

// copies the first PT_KSPHERES spheres' attributes from the kernel arguments into LDS (path_shade's sph_tab = 0)
// HIST (PT_OPT_PATH_HISTORY): one more row behind them, the call's triangle material as code PT_HIST_TRI reads it (wf_history_row)
constexpr int WF_TRI_ROW = 15 * PT_KSPHERES - 4;   // its emission at [4..6] and colour at [7..9], where a sphere's row has them
template <bool HIST = false>
__device__ __forceinline__ void wf_sphere_table() {
    if (threadIdx.x < 11 * PT_KSPHERES) {
        PT_KARGS(K);
        const float v = ((const __attribute__((address_space(4))) float*)&K.ksph[0])[threadIdx.x];
        ((float*)s_dyn)[threadIdx.x] = v;
        if (threadIdx.x % 11 < 4) ((float*)s_dyn)[88 + 4 * (threadIdx.x / 11) + threadIdx.x % 11] = v;
    }
    if (HIST && threadIdx.x >= 128 && threadIdx.x < 134) {   // (another wave than the spheres'; tri_col and tri_emi lie side by side)
        PT_KARGS(K);
        const int k = (int)threadIdx.x - 128;
        ((float*)s_dyn)[WF_TRI_ROW + (k < 3 ? 7 + k : 1 + k)] = ((const __attribute__((address_space(4))) float*)&K.tri_col[0])[k];
    }
    __syncthreads();
}

// PT_OPT_PATH_HISTORY: the row of the object behind a history code (pt_kernels.h) in the table above
__device__ __forceinline__ const float* wf_history_row(uint32_t code) {
    return (const float*)s_dyn + (code == PT_HIST_TRI ? (uint32_t)WF_TRI_ROW : 11u * code);
}
// ... and a path's mask and gathered light in front of bounce n, from the objects its bounces 0 .. n - 1 ended on: the operations,
// operands and order of path_shade_hit (DIFF, SPEC and METAL: accu += mask * emit, then mask *= colour), so both are what the lane
// that carries them from bounce to bounce holds, bit for bit
__device__ __forceinline__ void wf_history_replay(uint32_t word, uint32_t n, v3& mask, v3& accu) {
    mask = V3(1.f, 1.f, 1.f);
    accu = V3(0.f, 0.f, 0.f);
    for (uint32_t k = 0; k < n; k++) {   // (n = the bounce: wave-uniform)
        const float* t = wf_history_row(pt_hist_code(word, k));
        accu = vadd(accu, vmul(mask, V3(t[4], t[5], t[6])));
        mask = vmul(mask, V3(t[7], t[8], t[9]));
    }
}

// ------------------------------------------------------------------------------------------------
// once per call: the frame hashes of the call's samples (uf::hash, utilfun.cpp:380-389) and fresh queue
// counters for every bounce's extend launch
__global__ void __launch_bounds__(256) k_wf_prepare(const KParams P) {
    for (uint32_t i = threadIdx.x; i < P.spp; i += 256) P.wf.hashes[i] = pt_wang64(P.frame + i);
    for (uint32_t i = threadIdx.x; i < P.wf.queues_words; i += 256) P.wf.queues_all[i] = 0u;
}

// ------------------------------------------------------------------------------------------------
// slot = region * 256 + thread; slot >> 6 = a wave's worth of bounce-0 paths, coherent by construction (pt_slot_pixel)
__device__ __forceinline__ bool wf_slot_pixel(const KParams& P, uint32_t slot, uint32_t& s_idx, int& px, int& py) {
    if (slot >= P.wf.n_slots) return false;
    return pt_slot_pixel(P, slot, s_idx, px, py);
}

// the h.t an any-hit lane starts its walk with, for the sphere bound ts of its hit slot: t <= ts as the walk's t < h.t, so one bit up
// (ts > 0.01; PT_F32_MAX = no sphere stays)
__device__ __forceinline__ float wf_anyhit_start(float ts) {
    return ts < PT_F32_MAX ? __uint_as_float(__float_as_uint(ts) + 1u) : ts;
}

// ------------------------------------------------------------------------------------------------
// extend: the closest-hit walk (rows a5-a7) over the ray queue; see the file header.
// FIRST: bounce 0 — a region is 256 consecutive slots and the ray is the slot's camera ray.
// ANY (PT_OPT_LAST_ANYHIT): the path's last segment when no triangle emits — the shade launch before left (ts, sphere) of the
// ray's nearest sphere in the ray's hit slot, and all the picture still needs is whether a triangle is hit at t <= ts.  The
// lane starts the walk bounded by the next float above ts and leaves at the first record it accepts (trav_run_wide<.., ANY>);
// it writes t = 0 over ts when there is one and leaves the slot alone otherwise.
// ENTRY (PT_OPT_ROOT_ENTRY; never FIRST): the record carries what the walk's node step on the root found for its ray (the entry code
// of pt_kernels.h, left by the shade lane that made the ray), so the lane starts BEHIND that step: the far children on the stack, in
// the order the step pushes them, and the nearest one — a node or a leaf — as its item.  Stack, item and h.t are the walk's own after
// its first step, and everything after it is the same bit for bit.
// V: the word of pt_variants.h (WX_*; extend_exists: what is instantiated)
template <bool COUNT, uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK, budget_occ(wx_budget(V))) k_wf_extend(const KParams P) {
    static_assert(COUNT == wx_count(V), "COUNT repeats the word's bit");
    constexpr int LSTK = budget_lstk(wx_budget(V));
    constexpr bool FIRST = wx_first(V), ANY = wx_any(V), ENTRY = wx_entry(V);
    static_assert(!(FIRST && ENTRY), "bounce 0's rays come from the camera: nobody ran their root step");
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    TravOverflow<LSTK> stk_ovf;
    TravStack<LSTK, PT_BLOCK> stk(__builtin_amdgcn_readfirstlane(tid & ~63), stk_ovf);
    const bool cull = P.cull != 0;
    const uint32_t n_regions = (uint32_t)P.wf.n_regions;
    const uint32_t shard_regions = (n_regions + PT_SHARDS - 1) / PT_SHARDS;
    const int batch = P.batch;

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
    uint32_t n_rays = 0, it_begin = 0, act_begin = 0, it_loop = 0;
    int root_l0 = 0, root_l1 = 0, root_l2 = 0, root_l3 = 0;   // ENTRY: the root's four links (wave-uniform: scalar loads, once)
    if (ENTRY) {
        const float4 q2 = pt_uld4(P.sc.nodes, P.sc.wide_root + 2), q3 = pt_uld4(P.sc.nodes, P.sc.wide_root + 3);   // (wide_node_decode)
        root_l0 = __float_as_int(q2.z); root_l1 = __float_as_int(q2.w);
        root_l2 = __float_as_int(q3.x); root_l3 = __float_as_int(q3.y);
    }

    for (;;) {
        if (COUNT) it_loop++;
        // ---- refill: idle lanes take the next records of the wave's region(s); lane -> record by a ballot +
        // prefix count (v_mbcnt) of the idle mask
        const unsigned long long idle = __ballot(!live);
        const int n_idle = __popcll(idle);
        if (!empty && (n_idle >= batch || n_idle == 64)) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            uint32_t served = 0;
            for (int round = 0; round < 8 && served < (uint32_t)n_idle; round++) {
                if (next == end) {
                    // eight counters (blocks b and b + 8 share an XCD under round-robin placement: speed only);
                    // shard s owns regions s, s + 8, ...; an empty shard is left for the next one
                    bool got = false;
                    for (int tries = 0; tries < PT_SHARDS && !got; tries++) {
                        uint32_t k = 0;
                        if (lane == 0) k = atomicAdd(P.wf.queue + shard * PT_SHARD_STRIDE, 1u);
                        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
                        const uint32_t r = k * PT_SHARDS + (uint32_t)shard;
                        if (k < shard_regions && r < n_regions) {
                            next = r * PT_REGION;
                            if (FIRST) end = min(next + (uint32_t)PT_REGION, P.wf.n_slots);
                            else end = next + (uint32_t)__builtin_amdgcn_readfirstlane(P.wf.walk_in[r]);
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
                    float bound = PT_F32_MAX, b_w = 0.f;
                    if (FIRST) {
                        uint32_t s_idx = 0;
                        int px = 0, py = 0;
                        if (wf_slot_pixel(P, idx, s_idx, px, py)) {
                            PathState ps;
                            path_begin_hashed(P, px, py, (uint64_t)((uint32_t)py * (uint32_t)P.W + (uint32_t)px), P.wf.hashes[s_idx], ps);
                            o = ps.o;
                            d = ps.d;
                            live = true;
                        }
                    } else {
                        const float4 a = pt_sld4(P.wf.ray0_in + idx), b = pt_sld4(P.wf.ray1_in + idx);
                        if (ANY) bound = pt_sld1((const float*)(P.wf.hit + idx));
                        o = V3(a.x, a.y, a.z);
                        d = V3(a.w, b.x, b.y);
                        b_w = b.w;
                        live = true;
                    }
                    if (live) trav_begin(ts, o, d, stk, P.sc.wide_root);
                    if (ANY) ts.h.t = wf_anyhit_start(bound);
                    if constexpr (ENTRY) {   // what the root step would leave: trav_run_wide's pushes, far to near, then the nearest child
                        const uint32_t code = __float_as_uint(b_w) >> PT_REC_ENTRY_SHIFT, n = pt_entry_count(code);
                        auto link = [&](uint32_t k) {   // (wide_link of the root)
                            const uint32_t c = pt_entry_child(code, k);
                            return c == 0u ? root_l0 : (c == 1u ? root_l1 : (c == 2u ? root_l2 : root_l3));
                        };
                        if (n == 4u) { ts.sp++; stk.put(ts.sp, link(3)); }
                        if (n >= 3u) { ts.sp++; stk.put(ts.sp, link(2)); }
                        if (n >= 2u) { ts.sp++; stk.put(ts.sp, link(1)); }
                        ts.node = link(0);
                        if (COUNT && ts.node < 0) tc.leaves++;
                    }
                }
                next += take;
                served += take;
            }
            if (COUNT && served) { it_begin++; act_begin += served; }
        }
        const unsigned long long busy = __ballot(live);
        if (!busy) {
            if (empty) break;
            continue;
        }
        // ---- walk until `batch` lanes have finished (lanes that can get no more work do not count)
        const int n_dead = empty ? 64 - __popcll(busy) : 0;
        if (live) {
            const bool fin = trav_run_wide<tw_count(COUNT) | TW_DYN | TW_AHEAD | (ANY ? TW_ANY : 0u)>(ts, P.sc, o, d, cull, stk, tc, n_dead, batch);
            if (fin) {
                if (ANY) { if (ts.h.t == 0.0f) pt_sst1((float*)(P.wf.hit + idx), 0.0f); }
                else pt_sst2(P.wf.hit + idx, make_float2(ts.h.t, __int_as_float(ts.h.rec)));
                live = false;
                if (COUNT) n_rays++;
            }
        }
    }

    if (COUNT) {
        const uint32_t w_ovf = wave_sum_u32(stk.n_ovf), w_rays = ANY ? wave_sum_u32(n_rays) : 0u;
        pt_book_walk<true>(P, lane == 0, n_rays, tc);
        if (lane == 0) {
            if (ANY) atomicAdd(&P.counters[PT_CNT_ANY_RAYS], (unsigned long long)w_rays);
            atomicAdd(&P.counters[PT_CNT_IT_BEGIN], (unsigned long long)it_begin);
            atomicAdd(&P.counters[PT_CNT_ACT_BEGIN], (unsigned long long)act_begin);
            atomicAdd(&P.counters[PT_CNT_IT_LOOP], (unsigned long long)it_loop);
            atomicAdd(&P.counters[PT_CNT_STACK_OVF], (unsigned long long)w_ovf);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// extend of bounce 0 as wave-wide packets (PT_OPT_FIRST_WALK 1; trav_packet_wide): a wave walks 64-slot groups g, g + stride, ...
// (lane i = slot 64 g + i, the camera ray of path_begin_hashed), no queue and no refill.  The product launch is a plain grid of
// one wave per group (the loop runs once); the instrumented one (COUNT) runs a resident grid, so that each wave books its
// counters once for all of its groups instead of 518 400 waves adding to the same nine words.  The hits of a group are one
// coalesced 512-byte row.
template <bool COUNT>
__global__ void __launch_bounds__(PT_BLOCK, 8) k_wf_extend_packet(const KParams P) {
    const uint32_t n_groups = P.wf.n_slots / 64u;   // (n_slots is a multiple of 64)
    const uint32_t stride = gridDim.x * (uint32_t)(PT_BLOCK / 64);
    TravCount tc;
    uint32_t n_rays = 0, n_walked = 0;
    for (uint32_t group = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (PT_BLOCK / 64) + (threadIdx.x >> 6)));
         group < n_groups; group += stride) {   // (wave-uniform)
        const uint32_t slot = group * 64u + (threadIdx.x & 63u);
        uint32_t s_idx = 0;
        int px = 0, py = 0;
        v3 o = V3(0.f, 0.f, 0.f), d = V3(0.f, 0.f, 0.f);
        const bool in = wf_slot_pixel(P, slot, s_idx, px, py);
        if (in) {
            PathState ps;
            path_begin_hashed(P, px, py, (uint64_t)((uint32_t)py * (uint32_t)P.W + (uint32_t)px), P.wf.hashes[s_idx], ps);
            o = ps.o;
            d = ps.d;
        }
        const Hit h = trav_packet_wide<tw_count(COUNT)>(P.sc, o, d, P.cull != 0, in, tc);
        if (in) pt_sst2(P.wf.hit + slot, make_float2(h.t, __int_as_float(h.rec)));
        if (COUNT) { n_rays += in ? 1u : 0u; n_walked++; }
    }
    if (COUNT && n_walked) {   // (wave-uniform) rays .. leaves per lane of the masks; the wave's node / record steps and the lanes
                               // in their masks are lane 0's
        pt_book_walk<true>(P, (threadIdx.x & 63) == 0, n_rays, tc);
        if ((threadIdx.x & 63) == 0) atomicAdd(&P.counters[PT_CNT_PACKET_GROUPS], (unsigned long long)n_walked);
    }
}

// ------------------------------------------------------------------------------------------------
// shade: one bounce of tracer.cu:98-296 for every live record of a region; see the file header.
// FIRST: bounce 0 — lane = slot; the path starts here (camera ray, RNG) and the sample colour is written, not added to.
// LAST: the path's final bounce (without PT_FLAG_NEE): only the hit's emission is still wanted (path_last_emission).
// where a surviving path's record goes inside its region: packed in slot order (experiments splice their own order in here:
// tools/pt_exp_hooks.h, PT_EXP_SORT)
#ifndef PT_SURVIVOR_RANK
#define PT_SURVIVOR_RANK(P, alive, ps, total, s_cnt) wf_block_rank(alive, total, s_cnt)
#endif

// tracer.cu:140-142: a miss makes the sample the background colour; PT_FLAG_MISS_KEEPS_PATH (extension) adds mask * background (FIRST: to 0)
template <bool FIRST>
__device__ __forceinline__ void wf_shade_miss(float* smp, v3 mask) {
    PT_KARGS(K);
    if (FIRST && (K.flags & PT_FLAG_MISS_KEEPS_PATH)) {
        smp[0] = 0.f + mask.x * K.bk[0]; smp[1] = 0.f + mask.y * K.bk[1]; smp[2] = 0.f + mask.z * K.bk[2];
    } else if (K.flags & PT_FLAG_MISS_KEEPS_PATH) {
        smp[0] += mask.x * K.bk[0]; smp[1] += mask.y * K.bk[1]; smp[2] += mask.z * K.bk[2];
    } else {
        smp[0] = K.bk[0]; smp[1] = K.bk[1]; smp[2] = K.bk[2];
    }
}
// PT_OPT_PATH_HISTORY: the same rule for a lane that holds the path's whole accu — the sample's one store (accu is 0 at bounce 0)
__device__ __forceinline__ void wf_shade_miss_history(float* smp, v3 accu, v3 mask) {
    PT_KARGS(K);
    if (K.flags & PT_FLAG_MISS_KEEPS_PATH) pt_sst3(smp, V3(accu.x + mask.x * K.bk[0], accu.y + mask.y * K.bk[1], accu.z + mask.z * K.bk[2]));
    else pt_sst3(smp, V3(K.bk[0], K.bk[1], K.bk[2]));
}
// mask * emission of a later bounce's hit, added to the sample colour in place; nothing is touched when it is all zero
__device__ __forceinline__ void wf_add_emission(float* smp, v3 e) {
    if (!(e.x == 0.f) || !(e.y == 0.f) || !(e.z == 0.f)) {
        smp[0] += e.x; smp[1] += e.y; smp[2] += e.z;   // (as ONE dwordx3 each way: the last bounce's launch +6 %)
    }
}

// one path's segment after the walk: h = its closest triangle hit (h.tri 0, or the triangle's id with P.tri_matid; -1 on a
// miss); the spheres, then the background, the emission alone (LAST) or shading + the BRDF sample, the emission going to the
// sample colour smp (FIRST: written, not added to).  True when the path goes on.
// HIST (PT_OPT_PATH_HISTORY): ps came in with the path's whole mask and accu (wf_history_replay), so smp is written ONCE, here, when
// the path ends with this segment, and not touched when it goes on; `code` = the history code of what the segment ended on.
template <bool NEE, bool FIRST, bool LAST, bool HIST = false>
__device__ __forceinline__ bool wf_shade_segment(const KParams& P, PathState& ps, const Hit& h, bool tri_hit, float* smp, NeeReq* req, uint32_t& code) {
    static_assert(!(NEE && HIST), "k_wf_resolve adds to the sample colour in place");
    v3 tri_n = V3(0.f, 0.f, 0.f);
    if (!LAST && tri_hit) {   // the triangle's un-normalised normal (4th piece)
        const float4 q3 = P.sc.nodes[h.rec + 3];
        tri_n = V3(q3.x, q3.y, q3.z);
    }
    const SceneHit sh = pt_closest_sphere(P, ps.o, ps.d, h, 0);
    if (sh.geom == 3) {
        if (HIST) wf_shade_miss_history(smp, ps.accu, ps.mask);
        else wf_shade_miss<FIRST>(smp, ps.mask);
        return false;
    }
    v3 col;
    if (HIST) {
        code = sh.geom == 1 ? (uint32_t)sh.sph_id : PT_HIST_TRI;
        if (LAST) {   // (tracer.cu:305: accu after the last hit's emission)
            pt_sst3(smp, vadd(ps.accu, path_last_emission(P, ps, h, sh, 0)));
            return false;
        }
        const bool ended = path_shade_hit(P, ps, h, sh, tri_n, col, 0, nullptr);
        if (ended) pt_sst3(smp, FIRST ? V3(0.f + col.x, 0.f + col.y, 0.f + col.z) : col);   // col = accu
        return !ended;
    }
    const bool done = LAST ? true : path_shade_hit(P, ps, h, sh, tri_n, col, 0, NEE ? req : nullptr);
    if (LAST) col = path_last_emission(P, ps, h, sh, 0);
    const v3 e = done ? col : ps.accu;   // mask * emission of this hit (accu entered as 0)
    if (FIRST) {   // accu = 0 (tracer.cu:48) + this hit's emission
        pt_sst3(smp, V3(0.f + e.x, 0.f + e.y, 0.f + e.z));
    } else wf_add_emission(smp, e);
    return !done;
}

// PT_OPT_FUSE_STAGES: the fold of one region inside the last shade launch, when the region's slots hold ALL samples of their
// pixels (sample groups of G = 4 LP = spp samples: 256 / G pixels x G samples).  Wave 0 folds them, LP lanes per pixel, through
// the code k_fold_samples_grouped<LP> runs, so the accumulator and the display words are the same bit for bit.
template <int LP>
__device__ __forceinline__ void wf_fold_region(const KParams& P, uint32_t region) {
    if (threadIdx.x >= 64) return;
    uint32_t s_idx = 0;
    int px = 0, py = 0;
    // sample 0 of the region's pixel threadIdx.x / LP (pt_slot_pixel: the G samples of a pixel are G consecutive slots)
    const bool in = wf_slot_pixel(P, region * PT_REGION + (threadIdx.x / LP) * (4u * LP), s_idx, px, py);
    pt_fold_pixel_grouped<LP>(P, in, in ? (size_t)py * (size_t)P.W + (size_t)px : 0, (int)(threadIdx.x % LP));
}

// PT_OPT_LAST_ANYHIT: the nearest sphere along a survivor's NEW ray, (ts, sphere) — pt_closest_sphere's loop over an empty
// triangle hit, so (PT_F32_MAX, -1) when no sphere qualifies.  With the strict running minimum this is the sphere the loop after
// the walk picks whenever a sphere wins, so the pair is final: the last segment only asks the triangles for a hit at t <= ts.
__device__ __forceinline__ float2 wf_sphere_bound(const KParams& P, const PathState& ps) {
    const SceneHit sh = pt_closest_sphere(P, ps.o, ps.d, pt_no_hit(), 0);
    return make_float2(sh.t, __int_as_float(sh.sph_id));
}

// PT_OPT_LAST_OCCLUDERS: whether one of the tree's occluders — the mesh's largest triangles, their records' first three pieces in the
// table P.wf.s_con, fetched once per wave with scalar loads as trav_packet_wide fetches its items — answers the any-hit query of a
// walker's last segment: the walk's test on the walk's record with trav_run_wide<.., ANY>'s acceptance (t > 0 && t < h.t, h.t the bound
// the lane would start that walk with), so a positive verdict is one the walk reaches at the record's leaf.  The order in which an
// any-hit query tries triangles does not matter.  The loop is wave-uniform: every lane of the wave calls it, `walker` set in the lanes
// that ask, and it ends with the table or when no lane is left undecided.
__device__ __forceinline__ bool wf_occluded(const KParams& P, bool walker, const PathState& ps, float ts) {
    const float4* tab = P.wf.s_con;
    const float t_max = wf_anyhit_start(ts);
    const bool cull = P.cull != 0;
    bool open = walker, hit = false;
    for (int a = 0; a < 3 * PT_OCCLUDERS_MAX && __ballot(open) != 0ull; a += 3) {
        const float4 q0 = pt_uld4(tab, a), q1 = pt_uld4(tab, a + 1), q2 = pt_uld4(tab, a + 2);
        const float t = pt_mt_intersect(V3(q0.x, q0.y, q0.z), V3(q1.x, q1.y, q1.z), V3(q2.x, q2.y, q2.z), ps.o, ps.d, cull);
        if (open && t > 0.0f && t < t_max) { hit = true; open = false; }
        if (__float_as_int(q1.w) != 0) break;   // the list's last record
    }
    return hit;
}

// PT_OPT_ROOT_CULL: where a surviving path's record goes inside its region, in two classes that each keep the slot order — the
// WALKERS at [0, n_walk), then the WALK-FREE records up to `total`: those whose new ray the next extend launch's first node step, on
// the tree's root with the h.t the lane would start with (ts: the sphere bound of a BOUND launch's survivor), would leave without a
// child.  That lane would pop the sentinel and report pt_no_hit(), or leave ts in place; here the lane that made the ray runs the
// step itself — the walk's own functions on the root fetched once per wave with scalar loads, so the verdict is the walk's bit for
// bit — and the extend launch only draws a region's first n_walk records.  Every lane of the block calls it.
// PT_OPT_ROOT_ENTRY: the rest of that step is kept too — the keys sorted as the walk sorts them, so the order is the walk's, ties
// included — as the walker's entry code in `entry`, already at its place in ray1.w (0 without the option, and for the walk-free).
// OCCL (PT_OPT_LAST_OCCLUDERS; BOUND launches with root_cull on): a walker's ray is the path's last segment, an any-hit query, and any
// accepted triangle answers it — so the lane tries the tree's occluder table first (wf_occluded) and a decided lane joins the walk-free
// class with `occluded` set: its hit slot gets the verdict k_wf_extend<.., ANY> would have written.
template <bool BOUND, bool OCCL = false>
__device__ __forceinline__ int wf_survivor_slot(const KParams& P, bool alive, const PathState& ps, float ts, bool& walk_free, int& n_walk,
                                                int& total, int* s_cnt, int* s_cnt_free, uint32_t& entry, bool& occluded) {
    static_assert(BOUND || !OCCL, "only a last segment is an any-hit query");
    walk_free = false;
    occluded = false;
    entry = 0u;
    if (P.wf.root_cull) {   // (wave-uniform)
        const WideNode root = wide_node_load_uniform(P.sc, P.sc.wide_root);
        if (alive) {
            TravState s;
            trav_ray(s, ps.o, ps.d);
            uint32_t key[4];
            wide_node_keys_raw(root, s.idx, s.idy, s.idz, s.oodx, s.oody, s.oodz, BOUND ? wf_anyhit_start(ts) : PT_F32_MAX, key);
            walk_free = (key[0] & key[1] & key[2] & key[3]) == 0xffffffffu;
            if (P.wf.root_entry && !walk_free) {   // (the flag is wave-uniform)
                wide_sort4(key);   // the hit children first, nearest first
                const uint32_t n = 1u + (key[1] != 0xffffffffu ? 1u : 0u) + (key[2] != 0xffffffffu ? 1u : 0u) + (key[3] != 0xffffffffu ? 1u : 0u);
                entry = pt_entry_pack(n, key[0], key[1], key[2]) << PT_REC_ENTRY_SHIFT;
            }
        }
    }
    if constexpr (OCCL) {   // (every lane of the wave; the sort above was for nothing in a lane decided here)
        occluded = wf_occluded(P, alive && !walk_free, ps, ts);
        if (occluded) { walk_free = true; entry = 0u; }
    }
    const int r = PT_SURVIVOR_RANK(P, alive && !walk_free, ps, n_walk, s_cnt);
    total = n_walk;
    if (!P.wf.root_cull) return r;
    int n_free;
    const int rf = PT_SURVIVOR_RANK(P, walk_free, ps, n_free, s_cnt_free);
    total += n_free;
    return walk_free ? n_walk + rf : r;
}

// the counts of a region's next generation; an instrumented launch that classifies (PT_OPT_ROOT_CULL 2) books the rays it kept out
// of the queue, which no extend wave will count
template <bool COUNT>
__device__ __forceinline__ void wf_region_counts(const KParams& P, uint32_t region, int n_walk, int total) {
    if (threadIdx.x != 0) return;
    P.wf.cnt_out[region] = total;
    P.wf.walk_out[region] = n_walk;
    if (COUNT && total != n_walk) {
        atomicAdd(&P.counters[PT_CNT_RAYS], (unsigned long long)(total - n_walk));
        atomicAdd(&P.counters[PT_CNT_WALK_FREE], (unsigned long long)(total - n_walk));
    }
}

// FOLD (PT_OPT_FUSE_STAGES, LAST only): LP of wf_fold_region — this launch also folds the samples, no k_fold_samples follows
// BOUND (PT_OPT_LAST_ANYHIT, the shade launch of bounce depth - 2): the survivors' rays are the paths' last segments; their
// sphere bound goes to the survivor's hit slot for k_wf_extend<.., ANY> and k_wf_shade_last_any
// HIST (PT_OPT_PATH_HISTORY, never NEE): plane 0 of the mask generations holds the path's history word instead of mask.x, the other two
// planes are not touched; the lane rebuilds mask and accu from it, and the sample colour is written by the lane the path ends in
// OCCL (PT_OPT_LAST_OCCLUDERS, BOUND only): the walkers among the survivors are tested against the tree's occluder table first
// (wf_survivor_slot); an instrumented launch books the rays it decided
// V: the word of pt_variants.h (WS_*; shade_exists: what is instantiated)
template <bool COUNT, uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK) k_wf_shade(const KParams P) {
    static_assert(COUNT == ws_count(V), "COUNT repeats the word's bit");
    constexpr bool NEE = ws_nee(V), FIRST = ws_first(V), LAST = ws_last(V), BOUND = ws_bound(V), HIST = ws_hist(V), OCCL = ws_occl(V);
    constexpr int FOLD = ws_fold(V);
    __shared__ int s_cnt[PT_BLOCK / 64];
    __shared__ int s_cnt2[PT_BLOCK / 64];
    __shared__ int s_cnt_free[PT_BLOCK / 64];
    const uint32_t region = blockIdx.x;
    const int n_in = FIRST ? PT_REGION : P.wf.cnt_in[region];
    const bool last = LAST || P.wf.bounce + 1 >= P.depth;
    if (n_in == 0) {   // (the whole block: before anything is set up — in an open scene most regions are empty after the first bounce)
        if (!last) wf_region_counts<false>(P, region, 0, 0);
        if (NEE && threadIdx.x == 0) P.wf.s_cnt[region] = 0;
        if constexpr (FOLD > 0) wf_fold_region<FOLD>(P, region);   // every path of the region ended earlier: its samples are final
        return;
    }
    wf_sphere_table<HIST>();
    const size_t i = (size_t)region * PT_REGION + threadIdx.x;
    bool have = (int)threadIdx.x < n_in;
    bool alive = false, tri_hit = false;
    uint32_t hist = 0, code = 0;
    PathState ps;
    NeeReq req;
    req.want = false;
    uint32_t pix = 0, s_idx = 0;
    int px = 0, py = 0;
    if (FIRST) have = wf_slot_pixel(P, (uint32_t)i, s_idx, px, py);
    if (have) {
        if (FIRST) {
            pix = (uint32_t)py * (uint32_t)P.W + (uint32_t)px;
            path_begin_hashed(P, px, py, (uint64_t)pix, P.wf.hashes[s_idx], ps);
        } else {
            const float4 a = pt_sld4(P.wf.ray0_in + i), b = pt_sld4(P.wf.ray1_in + i);
            ps.o = V3(a.x, a.y, a.z);
            ps.d = V3(a.w, b.x, b.y);
            pix = __float_as_uint(b.z);
            ps.nee_mask = 0;
            uint32_t sn = __float_as_uint(b.w);
            if (NEE) {   // the sphere bits ride above the pixel, the triangle-light bit above the sample number
                ps.nee_mask = (pix >> PT_REC_PIXEL_BITS) | ((sn >> PT_REC_LIGHT_BIT) << 8);
                pix &= (1u << PT_REC_PIXEL_BITS) - 1u;
                sn &= (1u << PT_REC_LIGHT_BIT) - 1u;
            } else if (P.wf.root_entry) sn &= (1u << PT_REC_ENTRY_SHIFT) - 1u;   // (the entry code was the walk's)
            s_idx = sn >> PT_REC_DRAW_BITS;
            if (HIST) {
                hist = __float_as_uint(pt_sld1(P.wf.mask_in + i));
                wf_history_replay(hist, P.wf.bounce, ps.mask, ps.accu);
            } else {
                ps.mask = V3(pt_sld1(P.wf.mask_in + i), pt_sld1(P.wf.mask_in + (size_t)P.wf.cap + i), pt_sld1(P.wf.mask_in + 2 * (size_t)P.wf.cap + i));
                ps.accu = V3(0.f, 0.f, 0.f);   // this segment's emission only: the running sum lives in the sample buffer
            }
            ps.depth = P.wf.bounce;
            ps.rng = pt_rng_init(P.wf.hashes[s_idx], (uint64_t)pix);
            ps.rng.n = sn & (PT_REC_MAX_DRAWS - 1u);
        }
        const float2 hh = pt_sld2(P.wf.hit + i);
        Hit h;
        h.t = hh.x;
        h.rec = __float_as_int(hh.y);
        h.tri = -1;
        tri_hit = h.t < PT_F32_MAX;
        if (tri_hit) {   // a triangle was hit: its id (v0.w)
            h.tri = 0;
            if (P.tri_matid) h.tri = __float_as_int(P.sc.nodes[h.rec].w);
        }
        alive = wf_shade_segment<NEE, FIRST, LAST, HIST>(P, ps, h, tri_hit, pt_sample_ptr(P, s_idx, (size_t)pix), &req, code);
    }
    float2 bound = make_float2(PT_F32_MAX, __int_as_float(-1));
    if (BOUND && alive) bound = wf_sphere_bound(P, ps);
    if (COUNT) {   // all 64 lanes of every wave are here
        const uint32_t nh = wave_sum_u32(tri_hit ? 1u : 0u), np = wave_sum_u32(have && !alive ? 1u : 0u);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&P.counters[PT_CNT_HITS], (unsigned long long)nh);
            atomicAdd(&P.counters[PT_CNT_PATHS], (unsigned long long)np);
        }
    }
    if (NEE) {   // PT_FLAG_NEE: the shadow rays of this bounce's DIFF hits, packed like the survivors
        int n_sh;
        const int rs = wf_block_rank(req.want, n_sh, s_cnt2);
        if (req.want) {
            const size_t j = (size_t)region * PT_REGION + (size_t)rs;
            P.wf.s_ray0[j] = make_float4(req.o.x, req.o.y, req.o.z, req.d.x);
            P.wf.s_ray1[j] = make_float4(req.d.y, req.d.z, __uint_as_float(pix), __uint_as_float(s_idx));
            P.wf.s_con[j] = make_float4(req.contrib.x, req.contrib.y, req.contrib.z, req.t_max);
        }
        if (threadIdx.x == 0) P.wf.s_cnt[region] = n_sh;
    }
    if (last) {   // every path ends with this bounce (tracer.cu:305)
        if constexpr (FOLD > 0) {
            // workgroup-scope release / acquire (vmcnt(0) + s_barrier): the emission adds above (HIST: the samples' stores) reach the
            // folding wave; the block is on one CU, and no other block writes these samples in this launch
            __syncthreads();
            wf_fold_region<FOLD>(P, region);
        }
        return;
    }
    int n_walk, total;
    bool walk_free, occluded;
    uint32_t entry;
    const int r = wf_survivor_slot<BOUND, OCCL>(P, alive, ps, bound.x, walk_free, n_walk, total, s_cnt, s_cnt_free, entry, occluded);
    if constexpr (OCCL) bound.x = occluded ? 0.0f : bound.x;   // k_wf_extend<.., ANY>'s verdict: t = 0 over ts, the sphere stays
    if (COUNT && OCCL) {   // all 64 lanes of every wave are here; wf_region_counts books every walk-free ray as the root's
        const unsigned long long no = (unsigned long long)__popcll(__ballot(occluded));
        if ((threadIdx.x & 63) == 0 && no) {
            atomicAdd(&P.counters[PT_CNT_OCCLUDED], no);
            atomicAdd(&P.counters[PT_CNT_WALK_FREE], 0ull - no);
        }
    }
    if (alive) {
        const size_t j = (size_t)region * PT_REGION + (size_t)r;
        pt_sst4(P.wf.ray0_out + j, make_float4(ps.o.x, ps.o.y, ps.o.z, ps.d.x));
        pt_sst4(P.wf.ray1_out + j, make_float4(ps.d.y, ps.d.z, __uint_as_float(NEE ? (pix | ((ps.nee_mask & 0xffu) << PT_REC_PIXEL_BITS)) : pix),
                                              __uint_as_float((s_idx << PT_REC_DRAW_BITS) | ps.rng.n | (NEE ? (ps.nee_mask >> 8) << PT_REC_LIGHT_BIT : entry))));
        if (HIST) pt_sst1(P.wf.mask_out + j, __uint_as_float(pt_hist_push(hist, P.wf.bounce, code)));
        else {
            pt_sst1(P.wf.mask_out + j, ps.mask.x);
            pt_sst1(P.wf.mask_out + (size_t)P.wf.cap + j, ps.mask.y);
            pt_sst1(P.wf.mask_out + 2 * (size_t)P.wf.cap + j, ps.mask.z);
        }
        // (slot j held another lane's hit of THIS bounce: every lane of the region has read its own before the rank's barrier)
        if (BOUND) pt_sst2(P.wf.hit + j, bound);   // (walk-free: the bound stands, "no triangle at or before the sphere")
        else if (walk_free) pt_sst2(P.wf.hit + j, make_float2(pt_no_hit().t, __int_as_float(pt_no_hit().rec)));   // what its walk would have written
    }
    wf_region_counts<COUNT>(P, region, n_walk, total);
}

// PT_OPT_LAST_ANYHIT: the last shade launch behind k_wf_extend<.., ANY>.  The hit slot holds (ts, sphere) of the segment's nearest
// sphere, t = 0 when a triangle lies at or before it: a triangle emits nothing (the launch is only chosen when none can), a sphere
// adds path_last_emission's 0 + mask * emission, neither is the background rule of wf_shade_segment.  No ray, no sphere tests.
// HIST: as k_wf_shade's — the lane holds the path's accu, and every verdict stores the sample once: accu when a triangle is in the way.
// V: the word of pt_variants.h (WS_*; shade_last_any_exists: what is instantiated)
template <bool COUNT, uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK) k_wf_shade_last_any(const KParams P) {
    static_assert(COUNT == ws_count(V), "COUNT repeats the word's bit");
    constexpr bool HIST = ws_hist(V);
    constexpr int FOLD = ws_fold(V);
    const uint32_t region = blockIdx.x;
    const int n_in = P.wf.cnt_in[region];
    if (n_in == 0) {
        if constexpr (FOLD > 0) wf_fold_region<FOLD>(P, region);
        return;
    }
    wf_sphere_table<HIST>();
    const size_t i = (size_t)region * PT_REGION + threadIdx.x;
    const bool have = (int)threadIdx.x < n_in;
    bool tri_hit = false;
    if (have) {
        const float4 b = pt_sld4(P.wf.ray1_in + i);
        const float2 hh = pt_sld2(P.wf.hit + i);
        v3 mask, accu = V3(0.f, 0.f, 0.f);
        if (HIST) wf_history_replay(__float_as_uint(pt_sld1(P.wf.mask_in + i)), P.wf.bounce, mask, accu);
        else mask = V3(pt_sld1(P.wf.mask_in + i), pt_sld1(P.wf.mask_in + (size_t)P.wf.cap + i), pt_sld1(P.wf.mask_in + 2 * (size_t)P.wf.cap + i));
        const uint32_t pix = __float_as_uint(b.z);
        const uint32_t s_idx = (__float_as_uint(b.w) & (P.wf.root_entry ? (1u << PT_REC_ENTRY_SHIFT) - 1u : ~0u)) >> PT_REC_DRAW_BITS;
        float* smp = pt_sample_ptr(P, s_idx, (size_t)pix);
        const int sph = __float_as_int(hh.y);
        tri_hit = hh.x == 0.0f;
        if (HIST) {
            if (tri_hit) pt_sst3(smp, accu);
            else if (sph >= 0) {
                const float* t = (const float*)s_dyn + 11 * sph;
                pt_sst3(smp, vadd(accu, vadd(V3(0.f, 0.f, 0.f), vmul(mask, V3(t[4], t[5], t[6])))));
            } else wf_shade_miss_history(smp, accu, mask);
        } else if (!tri_hit && sph >= 0) {
            const float* t = (const float*)s_dyn + 11 * sph;
            wf_add_emission(smp, vadd(V3(0.f, 0.f, 0.f), vmul(mask, V3(t[4], t[5], t[6]))));
        } else if (!tri_hit) {
            wf_shade_miss<false>(smp, mask);
        }
    }
    if (COUNT) {   // all 64 lanes of every wave are here
        const uint32_t nh = wave_sum_u32(tri_hit ? 1u : 0u), np = wave_sum_u32(have ? 1u : 0u);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&P.counters[PT_CNT_HITS], (unsigned long long)nh);
            atomicAdd(&P.counters[PT_CNT_PATHS], (unsigned long long)np);
        }
    }
    if constexpr (FOLD > 0) {
        __syncthreads();   // (as in k_wf_shade: the emission adds, or the stores, above reach the folding wave)
        wf_fold_region<FOLD>(P, region);
    }
}

// bounce 0's packet walk and its shade in ONE launch (PT_OPT_FUSE_STAGES 1: the product launch without PT_FLAG_NEE).  One block
// per region, as both launches it replaces run, so lane = slot of k_wf_shade<FIRST>: after trav_packet_wide the lane shades its
// own hit with the camera ray and RNG state it started the walk with — no hit record written and read back, no camera ray
// computed twice — and the survivors are packed as k_wf_shade<FIRST> packs them (same records, same order).
// BOUND: as k_wf_shade's (depth 2: bounce 0's survivors are the last segments).
// HIST: as k_wf_shade's (a path that goes on leaves its first code and no sample colour).
// OCCL: as k_wf_shade's.
// V: the word of pt_variants.h (WS_*; fused_exists: what is instantiated)
template <uint32_t V>
__global__ void __launch_bounds__(PT_BLOCK, 8) k_wf_extend_packet_shade(const KParams P) {
    constexpr bool BOUND = ws_bound(V), HIST = ws_hist(V), OCCL = ws_occl(V);
    __shared__ int s_cnt[PT_BLOCK / 64];
    __shared__ int s_cnt_free[PT_BLOCK / 64];
    wf_sphere_table<HIST>();
    const uint32_t region = blockIdx.x;
    const size_t i = (size_t)region * PT_REGION + threadIdx.x;
    uint32_t s_idx = 0;
    int px = 0, py = 0;
    const bool have = wf_slot_pixel(P, (uint32_t)i, s_idx, px, py);
    const uint32_t pix = (uint32_t)py * (uint32_t)P.W + (uint32_t)px;
    PathState ps;
    ps.o = ps.d = V3(0.f, 0.f, 0.f);
    if (have) path_begin_hashed(P, px, py, (uint64_t)pix, P.wf.hashes[s_idx], ps);
    TravCount tc;
    Hit h = trav_packet_wide<TW_NONE>(P.sc, ps.o, ps.d, P.cull != 0, have, tc);   // (every lane of the wave: EXEC = all 64)
    bool alive = false;
    uint32_t code = 0;
    if (have) {
        const bool tri_hit = h.t < PT_F32_MAX;
        if (tri_hit && !P.tri_matid) h.tri = 0;   // (else the walk's id: the record's v0.w, what k_wf_shade reads back)
        alive = wf_shade_segment<false, true, false, HIST>(P, ps, h, tri_hit, pt_sample_ptr(P, s_idx, (size_t)pix), nullptr, code);
    }
    if (P.wf.bounce + 1 >= P.depth) return;   // depth 1
    float2 bound = make_float2(PT_F32_MAX, __int_as_float(-1));
    if (BOUND && alive) bound = wf_sphere_bound(P, ps);
    int n_walk, total;
    bool walk_free, occluded;
    uint32_t entry;
    const int r = wf_survivor_slot<BOUND, OCCL>(P, alive, ps, bound.x, walk_free, n_walk, total, s_cnt, s_cnt_free, entry, occluded);
    if constexpr (OCCL) bound.x = occluded ? 0.0f : bound.x;   // (as k_wf_shade)
    if (alive) {
        const size_t j = (size_t)region * PT_REGION + (size_t)r;
        pt_sst4(P.wf.ray0_out + j, make_float4(ps.o.x, ps.o.y, ps.o.z, ps.d.x));
        pt_sst4(P.wf.ray1_out + j, make_float4(ps.d.y, ps.d.z, __uint_as_float(pix), __uint_as_float((s_idx << PT_REC_DRAW_BITS) | ps.rng.n | entry)));
        if (HIST) pt_sst1(P.wf.mask_out + j, __uint_as_float(pt_hist_push(0u, 0u, code)));
        else {
            pt_sst1(P.wf.mask_out + j, ps.mask.x);
            pt_sst1(P.wf.mask_out + (size_t)P.wf.cap + j, ps.mask.y);
            pt_sst1(P.wf.mask_out + 2 * (size_t)P.wf.cap + j, ps.mask.z);
        }
        if (BOUND) pt_sst2(P.wf.hit + j, bound);
        else if (walk_free) pt_sst2(P.wf.hit + j, make_float2(pt_no_hit().t, __int_as_float(pt_no_hit().rec)));   // (as k_wf_shade)
    }
    wf_region_counts<false>(P, region, n_walk, total);
}

// PT_FLAG_NEE: adds the contribution of every shadow ray that reached its light (nothing closer than t_max) to its path's
// sample colour — after the emission this bounce's shade launch added, as the oracle orders the two sums.
__global__ void __launch_bounds__(PT_BLOCK) k_wf_resolve(const KParams P) {
    const int n_in = P.wf.s_cnt[blockIdx.x];
    if ((int)threadIdx.x >= n_in) return;
    const size_t i = (size_t)blockIdx.x * PT_REGION + threadIdx.x;
    const float4 c = P.wf.s_con[i];
    const float2 hh = P.wf.s_hit[i];
    if (hh.x < c.w) return;   // a triangle is in the way
    const float4 b = P.wf.s_ray1[i];
    const uint32_t pix = __float_as_uint(b.z), s_idx = __float_as_uint(b.w);
    float* smp = pt_sample_ptr(P, s_idx, (size_t)pix);
    smp[0] += c.x; smp[1] += c.y; smp[2] += c.z;
}

namespace ptmi {

// makes sure the context holds the path records of layout w (plan_wave_layout, pt_plan.h)
int wave_reserve(pt_ctx* c, const WaveLayout& w) {
    if (w.need > c->d_wave.count()) HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, c->d_wave.reserve(w.need));
    return PT_OK;
}

constexpr size_t WF_LDS_SHADE = (15 * PT_KSPHERES + 6) * 4;   // wf_sphere_table, with the triangle material's row
// one block per region of Q
template <class K>
static hipError_t launch_regions(K kernel, size_t n_blocks, size_t lds, const KParams& Q, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_blocks), dim3(PT_BLOCK), lds, s, Q);
    return hipGetLastError();
}
// the extend stage's persistent grid (resident blocks, at most `blocks_per_cu` per CU) over the records of Q.
// Instantiated: extend_exists, fused_exists; the words: extend_word, fused_word (pt_variants.h).
static hipError_t launch_extend(const WavePlan& p, WaveExtend kind, const KParams& Q, const LaunchCfg& L, int blocks_per_cu, hipStream_t s) {
    const size_t n_reg = (size_t)Q.wf.n_regions;
    if (kind == EXT_FUSED)
        return with_variant<fused_exists, WS_BITS>(fused_word(p, Q.depth), [&](auto v) { return launch_regions(k_wf_extend_packet_shade<v()>, n_reg, WF_LDS_SHADE, Q, s); });
    if (kind == EXT_PACKET) {   // one block per region (4 groups); instrumented: the resident grid, 8 blocks per CU
#ifdef PT_PACKET_RESIDENT_GRID   // experiment (tools/build_variant.sh): the product launch on the resident grid too
        const bool resident = true;
#else
        const bool resident = p.count;
#endif
        const size_t n_blk = resident ? std::min<size_t>(n_reg, (size_t)8 * L.n_cu) : n_reg;
        return p.count ? launch_regions(k_wf_extend_packet<true>, n_blk, 0, Q, s) : launch_regions(k_wf_extend_packet<false>, n_blk, 0, Q, s);
    }
    return with_variant<extend_exists, WX_BITS>(extend_word(p, kind), [&](auto v) {
        return launch_resident(k_wf_extend<wx_count(v()), v()>, (size_t)budget_lstk(wx_budget(v())) * PT_BLOCK * 4, blocks_per_cu, L.n_cu, n_reg, s, Q);
    });
}

// the shade stage.  Instantiated: shade_exists, shade_last_any_exists; the word: shade_word (pt_variants.h).
static hipError_t launch_shade(const WavePlan& p, WaveShade kind, bool first, const KParams& Q, hipStream_t s) {
    const size_t n_reg = (size_t)Q.wf.n_regions;
    if (kind == SHADE_LAST_ANY)
        return with_variant<shade_last_any_exists, WS_BITS>(shade_word(p, kind, first), [&](auto v) {
            return launch_regions(k_wf_shade_last_any<ws_count(v()), v()>, n_reg, WF_LDS_SHADE, Q, s);
        });
    return with_variant<shade_exists, WS_BITS>(shade_word(p, kind, first), [&](auto v) { return launch_regions(k_wf_shade<ws_count(v()), v()>, n_reg, WF_LDS_SHADE, Q, s); });
}

int render_wavefront(pt_ctx* c, KParams& P, const CallPlan& call) {
    const WaveLayout& w = call.wl;
    const WavePlan& plan = call.wave;
    const LaunchCfg& L = call.L;
    const int rc = wave_reserve(c, w);
    if (rc != PT_OK) return rc;
    char* const base = c->d_wave.get();   // the pieces of the layout: base + w.off[piece], the second generation of a piece at piece + 1
    P.wf.nee = w.nee ? 1 : 0;
    P.wf.root_cull = plan.root_cull ? 1 : 0;
    P.wf.root_entry = plan.root_entry ? 1 : 0;
    if (w.nee) {
        P.wf.s_ray0 = (float4*)(base + w.off[W_S_RAY0]);
        P.wf.s_ray1 = (float4*)(base + w.off[W_S_RAY1]);
        P.wf.s_con = (float4*)(base + w.off[W_S_CON]);
        P.wf.s_hit = (float2*)(base + w.off[W_S_HIT]);
        P.wf.s_cnt = (int*)(base + w.off[W_S_CNT]);
    } else P.wf.s_con = plan.occluders ? c->d_occ.get() : nullptr;   // (the table of the tree on the context: occluders_collect)
    unsigned int* const queues = (unsigned int*)(base + w.off[W_QUEUES]);

    hipStream_t st = c->stream;
    P.sc.n_top = 0;
    P.sph_tab = 0;
    P.batch = call.wave_batch;
    P.wf.hit = (float2*)(base + w.off[W_HIT]);
    P.wf.hashes = (unsigned long long*)(base + w.off[W_HASHES]);
    P.wf.queues_all = queues;
    P.wf.queues_words = (uint32_t)w.q_words;
    P.wf.cap = (uint32_t)w.cap;
    P.wf.n_regions = (int)w.n_regions;
    P.wf.n_slots = (uint32_t)((size_t)call.work_tiles * 64);
    P.wf.bounce = 0;
    hipLaunchKernelGGL(k_wf_prepare, dim3(1), dim3(256), 0, st, P);
    HIP_TRY(c, hipGetLastError());
    if (stage_mark(c, PT_STAGE_GENERATE) != PT_OK) return PT_ERR_DEVICE;

    for (uint32_t b = 0; b < P.depth; b++) {
        const int g = (int)(b & 1u);
        P.wf.bounce = b;
        const int o = g ^ 1;   // bounce b reads generation g and writes the other
        P.wf.ray0_in = (float4*)(base + w.off[W_RAY0 + g]); P.wf.ray1_in = (float4*)(base + w.off[W_RAY1 + g]); P.wf.mask_in = (float*)(base + w.off[W_MASK + g]);
        P.wf.cnt_in = (int*)(base + w.off[W_CNT + g]); P.wf.walk_in = (int*)(base + w.off[W_WALK + g]);   // (walk: the records at the front of every region that the extend launch walks)
        P.wf.ray0_out = (float4*)(base + w.off[W_RAY0 + o]); P.wf.ray1_out = (float4*)(base + w.off[W_RAY1 + o]); P.wf.mask_out = (float*)(base + w.off[W_MASK + o]);
        P.wf.cnt_out = (int*)(base + w.off[W_CNT + o]); P.wf.walk_out = (int*)(base + w.off[W_WALK + o]);
        P.wf.queue = queues + (size_t)b * PT_SHARDS * PT_SHARD_STRIDE;
        HIP_TRY(c, launch_extend(plan, plan.extend(b, P.depth), P, L, call.wave_blocks, st));   // (EXT_FUSED: walk + shade, booked as extend)
        if (stage_mark(c, PT_STAGE_EXTEND) != PT_OK) return PT_ERR_DEVICE;
        const WaveShade shade = plan.shade(b, P.depth);
        if (shade == SHADE_NONE) continue;
        HIP_TRY(c, launch_shade(plan, shade, b == 0, P, st));
        if (stage_mark(c, PT_STAGE_SHADE) != PT_OK) return PT_ERR_DEVICE;
        if (w.nee) {   // this bounce's shadow rays: the closest-hit extend kernel over the shadow records, then the resolve
            KParams S = P;
            S.wf.ray0_in = P.wf.s_ray0; S.wf.ray1_in = P.wf.s_ray1; S.wf.cnt_in = S.wf.walk_in = P.wf.s_cnt; S.wf.hit = P.wf.s_hit;   // (every shadow ray is walked)
            S.wf.queue = queues + ((size_t)P.depth + b) * PT_SHARDS * PT_SHARD_STRIDE;
            HIP_TRY(c, launch_extend(plan, EXT_CLOSEST, S, L, call.wave_blocks, st));
            if (stage_mark(c, PT_STAGE_EXTEND) != PT_OK) return PT_ERR_DEVICE;
            hipLaunchKernelGGL(k_wf_resolve, dim3((unsigned)w.n_regions), dim3(PT_BLOCK), 0, st, P);
            HIP_TRY(c, hipGetLastError());
            if (stage_mark(c, PT_STAGE_SHADE) != PT_OK) return PT_ERR_DEVICE;
        }
    }
    return PT_OK;
}

}  // namespace ptmi
