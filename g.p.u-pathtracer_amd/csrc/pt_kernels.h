// pt_kernels.h — the path loop as gfx950 kernels.
//
// Reference path:  trace (GpuPathTracer/tracer.cu:343-400) → getSample
// (:27-339) → intersectBVHandTriangles (GpuPathTracer/cudaUtils.h:256-460) +
// intersectAllSpeheres (:221-236) → BRDF block (tracer.cu:156-293) → accumulate + pack
// (:386-398).  Not a translation: wave64 tiles, traversal stack in LDS, re-laid-out
// scene, counter RNG keyed by pixel.
#pragma once
#include "pt_math.h"
#include "pt_env.h"
#include "pt_variants.h"
#include "../../include/ptmi.h"

struct KScene {
    // One buffer of 64-byte items (4 float4 each): inner nodes first, then triangle records
    //   node: [c0.lo.x c0.hi.x c0.lo.y c0.hi.y][c1 ...][c0.lo.z c0.hi.z c1.lo.z c1.hi.z][link0 link1 0 0]
    //   tri : [v0.xyz, id][e1.xyz, last][e2.xyz, 0][cross(v0-v1, v0-v2), 0]
    // links: >= 0 float4 index of an inner node, < 0 ~(float4 index of a leaf's first record)
    const float4* __restrict__ nodes;   // = items
    const float4* __restrict__ tris;    // = items (same base: leaf links index the same buffer)
    const pt_sphere_d* __restrict__ spheres;
    int n_spheres;
    int has_bvh;
    int n_top;     // nodes [top_base/4, top_base/4 + n_top) (breadth-first prefix) are mirrored in LDS
    int stack_n;   // LDS stack entries per lane
    int top_base;  // float4 index of the mirrored tree's root: 0 (binary) or wide_root
    int wide_root; // float4 index of the 4-wide quantised tree's root (= its node 0), 0 if absent
};

// Stage-split (wavefront) pipeline, pt_k_wave.hip: one generation of path records in HBM.  A record lives
// in slot i of its REGION (256 consecutive slots = one block of the generate / shade stages); a region's live
// records are packed at its front and counted in cnt[region], so compaction never leaves the block
// (ballot + prefix count, no global atomics) and the order of the records is deterministic.  PT_OPT_ROOT_CULL: the records whose
// ray the tree's root turns away come last, walk[region] counts the ones before them, and only those are walked.
//   ray0[i] = (o.x, o.y, o.z, d.x)   ray1[i] = (d.y, d.z, bits(pixel), bits(sample << PT_REC_DRAW_BITS | rng draws))
//             (PT_OPT_ROOT_ENTRY: ray1.w = bits(entry code << PT_REC_ENTRY_SHIFT | sample << PT_REC_DRAW_BITS | rng draws), below)
//   mask    = three planes [cap] (x, y, z), not stored for the first bounce (1, 1, 1)
//             (PT_OPT_PATH_HISTORY: plane 0 = the path's history word, below; the sample colour is then written once, where the path ends)
//   hit[i]  = (t, bits(float4 index of the winning record)); t = F32_MAX: no triangle
// PT_FLAG_NEE: the sphere bits of nee_mask ride above the pixel (ray1.z), its triangle-light bit above the sample (ray1.w).
// The stages of pt_k_wave.hip pack and unpack the record with the PT_REC_* field widths of pt_variants.h.
// PT_OPT_ROOT_ENTRY (KWave::root_entry; never with PT_FLAG_NEE): the top PT_REC_ENTRY_BITS of ray1.w hold the walker's ENTRY CODE, what the
// walk's node step on the tree's root found for the record's ray — the shade lane that made the ray ran that step (PT_OPT_ROOT_CULL) —
// and the sample number keeps the bits between.  A call whose spp does not fit them keeps the format above.
// The entry code: the root's hit children nearest first, as wide_sort4 orders them — three 2-bit child numbers below (hit children - 1).
// A walker has 1..4 hit children; with four the last one is the XOR of the other three (0 ^ 1 ^ 2 ^ 3 = 0).  The fields of children
// that are not hit are not read.
constexpr uint32_t pt_entry_pack(uint32_t n, uint32_t c0, uint32_t c1, uint32_t c2) {
    return (c0 & 3u) | ((c1 & 3u) << 2) | ((c2 & 3u) << 4) | ((n - 1u) << 6);
}
constexpr uint32_t pt_entry_count(uint32_t code) { return (code >> 6) + 1u; }
// the k-th nearest hit child, k < pt_entry_count(code)
constexpr uint32_t pt_entry_child(uint32_t code, uint32_t k) {
    return k < 3u ? (code >> (2u * k)) & 3u : (code ^ (code >> 2) ^ (code >> 4)) & 3u;
}
// every ordered selection of 1..4 of the four children (4 + 12 + 24 + 24 = 64) comes back from its code, and the code fits its field
constexpr bool pt_entry_round_trips() {
    uint32_t seen = 0;
    for (uint32_t n = 1; n <= 4; n++)
        for (uint32_t s = 0; s < 256; s++) {   // s: four 2-bit child numbers; the first n must differ
            const uint32_t c[4] = {s & 3u, (s >> 2) & 3u, (s >> 4) & 3u, (s >> 6) & 3u};
            bool distinct = true;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t j = i + 1; j < n; j++) distinct = distinct && c[i] != c[j];
            bool rest_zero = true;   // (one representative per selection)
            for (uint32_t i = n; i < 4; i++) rest_zero = rest_zero && c[i] == 0u;
            if (!distinct || !rest_zero) continue;
            const uint32_t code = pt_entry_pack(n, c[0], c[1], c[2]);
            if (code >= (1u << PT_REC_ENTRY_BITS) || pt_entry_count(code) != n) return false;
            for (uint32_t k = 0; k < n; k++)
                if (pt_entry_child(code, k) != c[k]) return false;
            seen++;
        }
    return seen == 64u;
}
static_assert(pt_entry_round_trips(), "the entry code of PT_OPT_ROOT_ENTRY");
// PT_OPT_PATH_HISTORY (WavePlan::history): plane 0 of `mask` holds the path's HISTORY WORD instead of mask.x, and the other two planes are
// neither read nor written.  The word has PT_HIST_BITS per finished bounce, bounce b's at bits 4b .. 4b + 3: the code of the object that
// bounce ended on, 0-7 = sphere k (of the kernel-argument block), PT_HIST_TRI = a triangle (the call's one triangle material).  32 bits
// hold the 8 bounces a path of depth 9 survives.  Mask and gathered light are functions of it (wf_history_replay, pt_k_wave.hip).
constexpr uint32_t pt_hist_push(uint32_t word, uint32_t bounce, uint32_t code) { return word | (code << (PT_HIST_BITS * bounce)); }
constexpr uint32_t pt_hist_code(uint32_t word, uint32_t bounce) { return (word >> (PT_HIST_BITS * bounce)) & ((1u << PT_HIST_BITS) - 1u); }
// every code comes back from every bounce's field, whatever the other fields hold, and the lower fields stay what they were
constexpr bool pt_hist_round_trips() {
    for (uint32_t b = 0; b + 1 < PT_HIST_MAX_DEPTH; b++)
        for (uint32_t code = 0; code <= PT_HIST_TRI; code++) {
            uint32_t w = 0;
            for (uint32_t k = 0; k < b; k++) w = pt_hist_push(w, k, (code + k) % (PT_HIST_TRI + 1u));
            w = pt_hist_push(w, b, code);
            if (pt_hist_code(w, b) != code) return false;
            for (uint32_t k = 0; k < b; k++)
                if (pt_hist_code(w, k) != (code + k) % (PT_HIST_TRI + 1u)) return false;
        }
    return PT_HIST_TRI >= PT_KSPHERES && PT_HIST_TRI < (1u << PT_HIST_BITS);
}
static_assert(pt_hist_round_trips(), "the history word of PT_OPT_PATH_HISTORY");
struct KWave {
    const float4* __restrict__ ray0_in;
    const float4* __restrict__ ray1_in;
    const float* __restrict__ mask_in;
    float4* __restrict__ ray0_out;
    float4* __restrict__ ray1_out;
    float* __restrict__ mask_out;
    float2* __restrict__ hit;
    const int* __restrict__ walk_in;   // records at the front of a region that the extend launch walks (<= cnt_in); next to `hit`, its other word
    const int* __restrict__ cnt_in;
    int* __restrict__ cnt_out;
    int* __restrict__ walk_out;
    unsigned long long* hashes;   // uf::hash(frame + s), s < spp (written by k_wf_prepare)
    unsigned int* queue;          // region queue of THIS bounce's extend launch (PT_SHARDS counters)
    unsigned int* queues_all;     // k_wf_prepare: every bounce's counters, zeroed
    uint32_t queues_words;
    uint32_t cap;                 // slots per plane (regions * 256)
    int n_regions;
    uint32_t n_slots;             // (sample, pixel) slots of the call: work tiles * 64 (bounce 0 works on slots, not records)
    // PT_FLAG_NEE: the shadow-ray records a shade launch emits (region-compacted like the survivors), traced by another
    // extend launch and resolved by k_wf_resolve: s_ray0/s_ray1 as ray0/ray1, s_con = (contribution rgb, t_max), s_hit
    float4* __restrict__ s_ray0;
    float4* __restrict__ s_ray1;
    float4* __restrict__ s_con;   // without PT_FLAG_NEE: the tree's occluder table when the call tests it (PT_OPT_LAST_OCCLUDERS), read only:
                                  // 3 float4 per occluder = the first three pieces of its record, the last one's `last` flag set
    float2* __restrict__ s_hit;
    int* __restrict__ s_cnt;
    int nee;                      // 1: ray1.z carries pixel | nee_mask << 24
    int root_cull;                // 1: this call's shade launches classify their survivors (PT_OPT_ROOT_CULL)
    int root_entry;               // 1: ... and leave the walkers' entry codes in ray1.w, where the extend launches start from (PT_OPT_ROOT_ENTRY)
    uint32_t bounce;
};

struct KParams {
    KScene sc;
    pt_sphere_d ksph[PT_KSPHERES];
    float* __restrict__ accum;
    uint32_t* __restrict__ rgba;
    unsigned long long* counters;      // PT_CNT_N x u64 when instrumented
    pt_camera cam;
    int W, H;
    uint32_t depth;
    int cull;
    uint64_t frame, sample_index;
    uint32_t spp;
    int tri_mat;
    float tri_col[3], tri_emi[3], bk[3];
    float air_ior, glass_ior, phong;
    // per-triangle materials (pt_upload_tri_materials): NULL = the reference's one global material
    const int* tri_matid;          // [original triangle id] -> row of mat_table
    const float4* mat_table;       // 2 float4 per material: (col, emi.x) (emi.yz, mat bits, phong)
    // PT_FLAG_NEE: the triangles whose material row emits, ascending original id; 3 float4 each:
    // (v0, emi.r) (e1 = v1 - v0, emi.g) (e2 = v2 - v0, emi.b) — copied from the triangle's record
    const float4* tri_lights;
    int n_tri_lights;
    uint32_t flags;
    // tile enumeration: tiles_x tiles per tile-row; this launch covers n_tiles tiles taken
    // from the tile-rows this partition owns (stripes of stripe_tr tile-rows, round-robin)
    int tiles_x, tile_rows, n_tiles;
    int part_index, part_count, stripe_tr;
    // persistent kernel: global work counter over the n_tiles*64 tile-ordered pixel slots,
    // and the number of waiting lanes that makes a wave leave the traversal loop
    unsigned int* queue;
    int batch;
    int refill;   // idle lanes that trigger a refill from the queue
    int sph_tab;              // float index into the dynamic LDS of the sphere table (persistent kernel), -1 = none
    int vote_node, vote_rec;  // postponed-leaf walk: node step when n_node*vote_node >= n_rec*vote_rec
    int chunk;    // tile-ordered pixel slots per queue fetch (<= PT_CHUNK)
    // spp > 1: samples are traced as independent work items into `samples` ([spp][H*W][3] floats)
    // and folded into the running mean afterwards, in order, by k_fold_samples.  The frame's
    // critical path is then ONE path, not spp paths, and a launch has spp x more parallel work.
    float* __restrict__ samples;   // nullptr: fold each sample straight into accum (spp == 1)
    // where (sample s, pixel p) lives: samples + 3 * (s * smp_ss + p * smp_ps) — [spp][H*W][3] (W*H, 1) for the kernels whose
    // waves hold ONE sample of 64 pixels, [H*W][spp][3] (1, spp) for the stage-split pipeline's sample groups
    unsigned long long smp_ss;
    uint32_t smp_ps;
    uint32_t sgroup_log2;          // 64 consecutive (sample, pixel) slots = 2^k samples x (64 >> k) pixels of a tile (pt_slot_pixel)
    KWave wf;
};
// The environment map of pt_upload_environment (KEnv, pt_env.h) rides in KParams WITHOUT making it larger: it is laid over the first
// bytes of `wf`.  A call runs either the stage-split pipeline, which reads wf and never a map (plan_walk, pt_plan.h: a context with a map does
// not choose it), or a kernel that shades in the lane that walked, which reads the map (texels == nullptr: none, bk_color) and
// never wf.  fill_path_params zeroes the block and copies the map in (pt_set_env); only render_wavefront writes wf.  So the size
// of KParams, the offset of every kernel's second argument and the instruction streams of the pipeline's kernels are what they
// were (a union of the two members already reorders two of k_wf_shade's stores).  The block is kernel-argument memory: written
// by the host, only ever read on the device, through PT_KENV.
static_assert(sizeof(KEnv) <= sizeof(KWave) && alignof(KEnv) <= alignof(KWave) && sizeof(KParams) == 872, "KParams must not grow: the map lies over wf");
#define PT_KENV(K) (*(pt_kenv*)&(K).wf)   // K: PT_KARGS' reference to the kernel-argument block
inline void pt_set_env(KParams& P, const KEnv& e) { __builtin_memcpy(&P.wf, &e, sizeof e); }

// the three colour floats of (sample s, pixel pix) in the call's sample buffer
__device__ __forceinline__ float* pt_sample_ptr(const KParams& P, uint32_t s, size_t pix) {
    return P.samples + 3 * ((size_t)s * (size_t)P.smp_ss + pix * (size_t)P.smp_ps);
}

struct Hit {
    float t;   // PT_F32_MAX on miss
    int tri;   // original triangle id, -1 on miss
    int rec;   // float4 index of the winner's record: its 4th piece holds cross(v0-v1, v0-v2),
               // fetched once per segment by pt_hit_normal instead of at every improvement (and two
               // registers less to carry through the walk)
};
__device__ __forceinline__ Hit pt_no_hit() {
    Hit h;
    h.t = PT_F32_MAX; h.tri = -1; h.rec = 0;
    return h;
}

// the un-normalised geometric normal of a hit triangle (4th piece of its record)
__device__ __forceinline__ v3 pt_hit_normal(const KScene& sc, const Hit& h) {
    const float4 q3 = sc.nodes[h.rec + 3];
    return V3(q3.x, q3.y, q3.z);
}

// true in exactly one of the lanes that execute this call together
__device__ __forceinline__ bool pt_first_active_lane() {
    const unsigned long long m = __ballot(true);
    return (__ffsll((long long)m) - 1) == (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
}

struct TravCount {
    uint32_t inner = 0, tris = 0, leaves = 0;
    // wave-level schedule statistics (instrumented launches of the wide walk only; booked by one lane of
    // those in the step): iterations spent in node / record steps and the lanes active in them
    uint32_t it_node = 0, act_node = 0, it_rec = 0, act_rec = 0;
};

// The words of KParams::counters (PT_OPT_COUNTERS): the six of pt_counters, then the PT_WAVE_STATS of pt_get_wave_stats, as include/ptmi.h
// documents them.  Two wave statistics mean another thing in the stage-split pipeline, whose shade stage has no passes to count.
enum {
    PT_CNT_RAYS, PT_CNT_INNER, PT_CNT_TRIS, PT_CNT_LEAVES, PT_CNT_HITS, PT_CNT_PATHS,
    PT_CNT_WAVE, PT_CNT_IT_NODE = PT_CNT_WAVE, PT_CNT_ACT_NODE, PT_CNT_IT_REC, PT_CNT_ACT_REC,   // node / record steps, their lanes
    PT_CNT_IT_SHADE, PT_CNT_ACT_SHADE,   // persistent kernel: shading passes, lanes
    PT_CNT_IT_BEGIN, PT_CNT_ACT_BEGIN,   // path-start (pipeline: refill) passes, lanes
    PT_CNT_IT_LOOP, PT_CNT_STACK_OVF,    // outer-loop iterations, pushes past the LDS window
    PT_CNT_WALK_FREE,                    // pipeline: rays kept out of the extend queue (PT_OPT_ROOT_CULL 2)
    PT_CNT_OCCLUDED,                     // pipeline: last-segment rays an occluder decided in the shade stage (PT_OPT_LAST_OCCLUDERS 2)
    PT_CNT_N,
    PT_CNT_PACKET_GROUPS = PT_CNT_IT_SHADE,   // pipeline: 64-ray groups the bounce-0 packet walk walked
    PT_CNT_ANY_RAYS = PT_CNT_ACT_SHADE        // pipeline: rays of the any-hit launch (PT_OPT_LAST_ANYHIT 2)
};
static_assert(PT_CNT_WAVE == sizeof(pt_counters) / sizeof(uint64_t) && PT_CNT_N - PT_CNT_WAVE == PT_WAVE_STATS, "include/ptmi.h");

#include "pt_walks.h"
#include "pt_shade.h"

template <bool COUNT, int ALG, int ENV, bool MIS, class STK>
__device__ __forceinline__ v3 pt_get_sample(const KParams& P, int px, int py, uint64_t pix, uint64_t frame,
                                            STK& stk, const float4* __restrict__ s_top, TravCount& tc,
                                            uint32_t& n_rays, uint32_t& n_hits) {
    PathStateOf<MIS> ps;
    path_begin(P, px, py, pix, frame, ps);
    const bool cull = P.cull != 0;
    v3 col = V3(0.f, 0.f, 0.f);
    if (P.depth == 0) return col;
    for (;;) {
        Hit h = pt_no_hit();
        if (P.sc.has_bvh) {
            if (ALG >= 2) {
                TravState ts;
                trav_begin(ts, ps.o, ps.d, stk, P.sc.wide_root);
                trav_run_wide<tw_count(COUNT) | (ALG == ALG_WIDE_WOOP ? TW_WOOP : 0u)>(ts, P.sc, ps.o, ps.d, cull, stk, tc, 0, 0);
                h = ts.h;
            } else if (ALG == 1) {
                TravState ts;
                trav_begin(ts, ps.o, ps.d, stk);
                trav_run_unified<tw_count(COUNT)>(ts, P.sc, ps.o, ps.d, cull, stk, tc, 0, 0);
                h = ts.h;
            } else {
                h = trav_bvh2<tw_count(COUNT) | TW_TOP>(P.sc, ps.o, ps.d, cull, stk, tc, s_top);
            }
        }
        if (COUNT) { n_rays++; n_hits += (h.tri != -1); }
        NeeReq req;
        req.want = false;
        const bool done = path_shade<ENV, MIS>(P, ps, h, col, -1, (P.flags & PT_FLAG_NEE) ? &req : nullptr);
        // the loop's exit condition crosses the shadow walk below in a VGPR: kept as a lane mask in SGPRs, hipcc (ROCm 7.2)
        // lost it across the walk's wave-uniform loop and a finished path ran one more bounce
        int done_v = done ? 1 : 0;
        asm volatile("" : "+v"(done_v));
        if (req.want) {   // PT_FLAG_NEE: the shadow ray of this DIFF hit, against the triangles
            Hit h2 = pt_no_hit();
            if (P.sc.has_bvh) {
                TravState ts;
                if (ALG >= 2) {
                    trav_begin(ts, req.o, req.d, stk, P.sc.wide_root);
                    trav_run_wide<tw_count(COUNT) | (ALG == ALG_WIDE_WOOP ? TW_WOOP : 0u)>(ts, P.sc, req.o, req.d, cull, stk, tc, 0, 0);
                } else if (ALG == 1) {
                    trav_begin(ts, req.o, req.d, stk);
                    trav_run_unified<tw_count(COUNT)>(ts, P.sc, req.o, req.d, cull, stk, tc, 0, 0);
                } else {
                    trav_begin(ts, req.o, req.d, stk);
                    trav_run<tw_count(COUNT) | TW_TOP>(ts, P.sc, req.o, req.d, cull, stk, tc, 0, 0, s_top);
                }
                h2 = ts.h;
            }
            if (COUNT) n_rays++;
            if (!(h2.t < req.t_max)) {
                ps.accu = vadd(ps.accu, req.contrib);
                if (done) col = vadd(col, req.contrib);   // the path ended with this bounce: col was the gathered light before it
            }
        }
        if (done_v) break;
    }
    return col;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// books a wave's walk counters: its rays and what their walks fetched, and (STEPS: the kernels whose wave statistics are
// documented) the wide walk's node / record steps, which the walk books in ONE lane of those inside it, so they are summed over
// the lanes too.  Every lane of the wave calls it; the lane with `booker` set adds the sums.
template <bool STEPS>
__device__ __forceinline__ void pt_book_walk(const KParams& P, bool booker, uint32_t n_rays, const TravCount& tc) {
    const uint32_t v[8] = {n_rays, tc.inner, tc.tris, tc.leaves, tc.it_node, tc.act_node, tc.it_rec, tc.act_rec};
    const int word[8] = {PT_CNT_RAYS, PT_CNT_INNER, PT_CNT_TRIS, PT_CNT_LEAVES, PT_CNT_IT_NODE, PT_CNT_ACT_NODE, PT_CNT_IT_REC, PT_CNT_ACT_REC};
    uint32_t sum[8];
#pragma unroll
    for (int k = 0; k < (STEPS ? 8 : 4); k++) sum[k] = wave_sum_u32(v[k]);
    if (!booker) return;
#pragma unroll
    for (int k = 0; k < (STEPS ? 8 : 4); k++) atomicAdd(&P.counters[word[k]], (unsigned long long)sum[k]);
}

// Maps the launch's linear tile number to the global tile coordinates this partition owns.
__device__ __forceinline__ bool pt_tile_coords(const KParams& P, int tile, int& tx, int& ty) {
    if (tile >= P.n_tiles) return false;
    const int lrow = tile / P.tiles_x;
    tx = tile - lrow * P.tiles_x;
    if (P.part_count > 1) {
        const int k = lrow / P.stripe_tr, within = lrow - k * P.stripe_tr;
        ty = (P.part_index + k * P.part_count) * P.stripe_tr + within;
    } else {
        ty = lrow;
    }
    return ty < P.tile_rows;
}

// The call's (sample, pixel) slots, 64 to a work tile, n_tiles * spp work tiles (stage-split pipeline and persistent kernel):
//  * sgroup_log2 = 0: work tile = (sample, tile), slot & 63 = pixel of the 8x8 tile in row order;
//  * sgroup_log2 = k: G = 2^k samples x 64/G pixels of a tile — the G samples of a pixel are the SAME ray but for the sub-pixel
//    jitter, so lanes that start them together walk the same nodes and records in step.  Work tile -> (sample group, tile, j-th
//    share of the tile's pixels); lane -> (pixel number j * 64/G + lane / G in Morton order, sample lane % G).
// Which lane traces which (pixel, sample) changes no result: every path is keyed by (sample's frame hash, pixel).
// False for slots past the call's last and for the pixels of a partial tile that lie outside the image (tracer.cu:358).
__device__ __forceinline__ bool pt_slot_pixel(const KParams& P, uint32_t slot, uint32_t& s_idx, int& px, int& py) {
    const uint32_t lg = P.sgroup_log2;
    int wt = (int)(slot >> 6);
    uint32_t k = slot & 63u, s_in = 0u;
    if (lg) {
        const uint32_t g1 = (1u << lg) - 1u;
        s_in = k & g1;
        k = ((uint32_t)wt & g1) * (64u >> lg) + (k >> lg);
        wt >>= lg;
    }
    const uint32_t grp = (uint32_t)(wt / P.n_tiles);
    wt -= (int)grp * P.n_tiles;
    s_idx = (grp << lg) + s_in;
    int tx = 0, ty = 0;
    if (s_idx >= P.spp || !pt_tile_coords(P, wt, tx, ty)) return false;
    if (lg) {   // Morton order inside the tile: consecutive pixel numbers form 2x2, 4x2, 4x4 ... blocks
        px = tx * PT_TILE + (int)((k & 1u) | ((k >> 1) & 2u) | ((k >> 2) & 4u));
        py = ty * PT_TILE + (int)(((k >> 1) & 1u) | ((k >> 2) & 2u) | ((k >> 3) & 4u));
    } else {
        px = tx * PT_TILE + (int)(k & 7u);
        py = ty * PT_TILE + (int)((k >> 3) & 7u);
    }
    return px < P.W && py < P.H;
}
