// pt_variants.h — which instantiations of the path, walk and query kernels exist, and which one a request runs.
//
// Every kernel family takes ONE flag word (uint32_t) of named bits and small named fields as its template argument (after COUNT, where
// a family has instrumented instantiations).  For each family this header holds the bits and their accessors, <family>_exists(v) — the
// rules for which words are instantiated, with the number of them pinned by a static_assert — and the pure functions that turn a
// request (option values, flags, the plan of a call) into a word.  The launchers (pt_k_*.hip) compute the word and hand it to
// with_variant (pt_ctx.h), which instantiates exactly the words that exist and answers hipErrorInvalidValue for any other; the check
// program (pt_variants_check.cpp, `make variants_check`) walks the whole request domain on the host and shows that every request has
// a kernel and every kernel a request.  Plain constexpr code for host and device: no HIP call, nothing of the context.
#pragma once
#include <cstdint>

#include "../../include/ptmi.h"

// f(v) for how many of the 2^n_bits words
template <class F>
constexpr int variant_count(F exists, int n_bits) {
    int n = 0;
    for (uint32_t v = 0; v < (1u << n_bits); v++) n += exists(v) ? 1 : 0;
    return n;
}
constexpr uint32_t variant_field(uint32_t v, int shift, int bits) { return (v >> shift) & ((1u << bits) - 1u); }

// ---- register / stack budgets: (waves per SIMD the registers leave room for) x (traversal stack entries per lane in LDS; deeper
// entries overflow to scratch).  They are speed knobs, never results: a request for another pair runs the nearest one (*_budget below).
enum Budget : uint32_t { BUDGET_4x16, BUDGET_6x16, BUDGET_8x16, BUDGET_6x24, BUDGET_4x72, BUDGET_N };
constexpr int BUDGET_BITS = 3;
constexpr int budget_occ(uint32_t b) { return b == BUDGET_8x16 ? 8 : (b == BUDGET_6x16 || b == BUDGET_6x24) ? 6 : 4; }
constexpr int budget_lstk(uint32_t b) { return b == BUDGET_4x72 ? 72 : b == BUDGET_6x24 ? 24 : 16; }

// ---- the sizes the kernels and the host's planning (pt_plan.h) share
#define PT_BLOCK 256          // frame kernels: 4 waves; one wave = one 8x8 pixel tile
#define PT_BLOCK_RAYS 256     // ray-batch kernel
#define PT_TILE 8
#define PT_MAX_TOP 1024       // most nodes the LDS copy of the top of the tree may hold
#define PT_STACK_CAP 72       // deepest traversal stack (tree depth <= 64, SplitBVHBuilder MaxDepth)
static_assert(budget_lstk(BUDGET_4x72) == PT_STACK_CAP, "the budget with the whole stack in LDS");
#define PT_SHARDS 8           // work-queue counters (one per XCD worth of blocks)
#define PT_SHARD_STRIDE 32    // uints between counters: one 128-byte line each
#define PT_REGION 256         // stage-split pipeline: path-record slots per region (= one block)
#define PT_KSPHERES 8         // spheres carried in the kernel-argument block (scalar loads); more -> global array
// the packed fields of the pipeline's path record (pt_kernels.h) and the limits plan_wave_layout (pt_plan.h) derives from them
constexpr uint32_t PT_REC_DRAW_BITS = 12;    // ray1.w: RNG draws of the path so far, below the sample number
constexpr uint32_t PT_REC_LIGHT_BIT = 31;    // ray1.w, PT_FLAG_NEE: nee_mask bit 8 (the triangle lights)
constexpr uint32_t PT_REC_PIXEL_BITS = 24;   // ray1.z, PT_FLAG_NEE: the pixel, below nee_mask bits 0-7 (the spheres)
// exclusive limits: draws per path, samples per call without / with PT_FLAG_NEE
constexpr uint32_t PT_REC_MAX_DRAWS = 1u << PT_REC_DRAW_BITS, PT_REC_MAX_SAMPLES = 1u << (32 - PT_REC_DRAW_BITS),
                   PT_REC_MAX_SAMPLES_NEE = 1u << (PT_REC_LIGHT_BIT - PT_REC_DRAW_BITS);
// PT_OPT_ROOT_ENTRY: the top bits of ray1.w hold the walker's entry code (pt_kernels.h), the sample number keeps the bits between
constexpr uint32_t PT_REC_ENTRY_BITS = 8, PT_REC_ENTRY_SHIFT = 32 - PT_REC_ENTRY_BITS;
constexpr uint32_t PT_REC_MAX_SAMPLES_ENTRY = 1u << (PT_REC_ENTRY_SHIFT - PT_REC_DRAW_BITS);   // exclusive, as the limits above
// PT_OPT_PATH_HISTORY: bits per finished bounce in the history word, a triangle's code, the deepest call the word serves (pt_kernels.h)
constexpr uint32_t PT_HIST_BITS = 4, PT_HIST_TRI = 8, PT_HIST_MAX_DEPTH = 32 / PT_HIST_BITS + 1;

// ---- the walk a path kernel runs (LaunchCfg::walk, the kernels' ALG) and what its miss and NEE branches do with the context's map (ENV)
enum { ALG_WHILE = 0, ALG_UNIFIED = 1, ALG_WIDE = 2, ALG_WIDE_WOOP = 3, ALG_WIDE_PEND = 4 };
enum { ENV_NONE = 0, ENV_LOOKUP = 1, ENV_LIGHT = 2 };   // no map; a miss looks the map up; ... and PT_FLAG_NEE draws from its tables
// the map on the context (LaunchCfg::env): ENV_LIGHT when it has sampling tables (PT_OPT_ENV_LIGHT)
constexpr int env_code(bool has_map, bool has_tables) { return has_map ? (has_tables ? ENV_LIGHT : ENV_LOOKUP) : ENV_NONE; }
// ... and the shading instantiation that serves it.  nee_kernel: the kernel can walk a shadow ray at all (the megakernel always, the
// NEE instantiations of k_render_rays); where it cannot, a map that is a light is only looked up.  The MIS instantiations exist without
// a map and with ENV_LIGHT, which serves a map without tables too (path_shade_hit asks for them).
constexpr int shade_env(int map, bool nee_kernel, bool mis) {
    if (map == ENV_LIGHT && !nee_kernel) return ENV_LOOKUP;
    return mis && map == ENV_LOOKUP ? ENV_LIGHT : map;
}

// ---- the walks of pt_walks.h: trav_run<W>, trav_run_unified<W>, trav_run_wide<W>, trav_run_wide_pend<W>, trav_bvh2<W>
enum : uint32_t {
    TW_NONE = 0u,
    TW_COUNT = 1u << 0,   // book the walk's fetches in TravCount
    TW_DYN = 1u << 1,     // resumable: hand the wave back when enough lanes wait for service
    TW_TOP = 1u << 2,     // while-while walk: the top of the tree from its LDS mirror
    TW_WOOP = 1u << 3,    // wide walk: Woop records
    TW_AHEAD = 1u << 4,   // wide walk: a leaf's second record requested with its first
    TW_ANY = 1u << 5,     // wide walk: any-hit query (exact records only)
};
constexpr uint32_t tw_count(bool count) { return count ? (uint32_t)TW_COUNT : 0u; }

// ---- the kernels that shade in the lane that walked: k_trace_mega_bvh2<COUNT, V>, k_trace_persist_bvh2<COUNT, V>, k_render_rays<V>
enum : uint32_t { PV_COUNT = 1u << 0, PV_NEE = 1u << 1, PV_MIS = 1u << 2 };   // instrumented; walks shadow rays (k_render_rays); PT_FLAG_MIS
constexpr int PV_BUDGET_SHIFT = 3, PV_ALG_SHIFT = 6, PV_ALG_BITS = 3, PV_ENV_SHIFT = 9, PV_ENV_BITS = 2, PV_BITS = 11;
constexpr bool pv_count(uint32_t v) { return (v & PV_COUNT) != 0; }
constexpr bool pv_nee(uint32_t v) { return (v & PV_NEE) != 0; }
constexpr bool pv_mis(uint32_t v) { return (v & PV_MIS) != 0; }
constexpr uint32_t pv_budget(uint32_t v) { return variant_field(v, PV_BUDGET_SHIFT, BUDGET_BITS); }
constexpr int pv_occ(uint32_t v) { return budget_occ(pv_budget(v)); }
constexpr int pv_lstk(uint32_t v) { return budget_lstk(pv_budget(v)); }
constexpr int pv_alg(uint32_t v) { return (int)variant_field(v, PV_ALG_SHIFT, PV_ALG_BITS); }
constexpr int pv_env(uint32_t v) { return (int)variant_field(v, PV_ENV_SHIFT, PV_ENV_BITS); }
constexpr uint32_t pv_word(bool count, bool nee, bool mis, uint32_t budget, int alg, int env) {
    return (count ? (uint32_t)PV_COUNT : 0u) | (nee ? (uint32_t)PV_NEE : 0u) | (mis ? (uint32_t)PV_MIS : 0u) | (budget << PV_BUDGET_SHIFT) |
           ((uint32_t)alg << PV_ALG_SHIFT) | ((uint32_t)env << PV_ENV_SHIFT);
}

// The megakernel: the three binary-tree and wide walks over exact records (it does not read Woop records) at (8, 16), (4, 16) and
// (4, all 72 in LDS); without a map, with its lookup and with its draw under NEE; under MIS without a map and with ENV_LIGHT.
constexpr bool mega_exists(uint32_t v) {
    const uint32_t b = pv_budget(v);
    if (pv_nee(v) || !(b == BUDGET_8x16 || b == BUDGET_4x16 || b == BUDGET_4x72) || pv_alg(v) > ALG_WIDE || pv_env(v) > ENV_LIGHT) return false;
    return !pv_mis(v) || pv_env(v) != ENV_LOOKUP;
}
constexpr uint32_t mega_budget(int occ, int lstk) { return lstk >= 72 ? BUDGET_4x72 : occ >= 5 ? BUDGET_8x16 : BUDGET_4x16; }
constexpr uint32_t mega_word(bool count, int occ, int lstk, int walk, int map, bool mis) {
    return pv_word(count, false, mis, mega_budget(occ, lstk), walk < ALG_WIDE ? walk : ALG_WIDE, shade_env(map, true, mis));
}
static_assert(variant_count(mega_exists, PV_BITS) == 90, "k_trace_mega_bvh2: 2 x 3 budgets x 3 walks x (3 maps + 2 under MIS)");

// The persistent kernel: the wide walks (Woop records and the postponed leaf among them) at all five budgets, the two exact binary
// walks (parity variants) at (8, 16) and (4, 72); without and with the map's lookup (it runs no NEE: a light or not), never MIS.
constexpr bool persist_exists(uint32_t v) {
    const uint32_t b = pv_budget(v);
    if (pv_nee(v) || pv_mis(v) || b >= BUDGET_N || pv_alg(v) > ALG_WIDE_PEND || pv_env(v) > ENV_LOOKUP) return false;
    return pv_alg(v) >= ALG_WIDE || b == BUDGET_8x16 || b == BUDGET_4x72;
}
constexpr uint32_t persist_budget(int walk, int occ, int lstk) {
    if (lstk >= 72) return BUDGET_4x72;
    if (walk < ALG_WIDE) return BUDGET_8x16;
    if (lstk == 24) return BUDGET_6x24;
    return occ >= 8 ? BUDGET_8x16 : occ >= 5 ? BUDGET_6x16 : BUDGET_4x16;
}
constexpr uint32_t persist_word(bool count, int occ, int lstk, int walk, int map) {
    const int alg = walk <= ALG_WHILE ? ALG_WHILE : walk > ALG_WIDE_PEND ? ALG_WIDE : walk;
    return pv_word(count, false, false, persist_budget(walk, occ, lstk), alg, shade_env(map, false, false));
}
static_assert(variant_count(persist_exists, PV_BITS) == 76, "k_trace_persist_bvh2: 2 x 2 maps x (3 wide walks x 5 budgets + 2 binary x 2)");

// pt_render_rays' kernel: the wide walk (over either records) and the unified binary walk, at (6, 16) without and (4, 16) with the
// shadow-ray state; each without and with the map's lookup, the NEE ones also with its draw; under MIS (only with NEE, never over Woop
// records) without a map and with ENV_LIGHT.  No instrumented instantiation.
constexpr bool rays_exists(uint32_t v) {
    if (pv_count(v) || pv_alg(v) < ALG_UNIFIED || pv_alg(v) > ALG_WIDE_WOOP || pv_budget(v) != (pv_nee(v) ? BUDGET_4x16 : BUDGET_6x16)) return false;
    if (!pv_nee(v)) return !pv_mis(v) && pv_env(v) <= ENV_LOOKUP;
    if (pv_mis(v)) return pv_alg(v) != ALG_WIDE_WOOP && (pv_env(v) == ENV_NONE || pv_env(v) == ENV_LIGHT);
    return pv_env(v) <= ENV_LIGHT;
}
constexpr uint32_t rays_word(int walk, int map, bool nee, bool mis) {   // (it has no while-while walk: 0 runs as 1)
    const int alg = walk == ALG_WIDE_WOOP || walk == ALG_WIDE ? walk : ALG_UNIFIED;
    return pv_word(false, nee, mis, nee ? BUDGET_4x16 : BUDGET_6x16, alg, shade_env(map, nee, mis));
}
static_assert(variant_count(rays_exists, PV_BITS) == 19, "k_render_rays: 3 walks x (2 + 3 maps) + 2 walks x 2 under MIS");
// pt_render_camera's kernel, k_render_camera<V>, is the same loop with the camera model's ray as the path start: the same walks, budgets
// and NEE / MIS / map rules, so its words ARE rays_exists / rays_word.  The camera model is a value of the launch, not a bit of the word.
constexpr bool camera_exists(uint32_t v) { return rays_exists(v); }
static_assert(variant_count(camera_exists, PV_BITS) == 19, "k_render_camera: one per k_render_rays, none per camera model");

// The kernel family of a path call, from the one the option, PT_FLAG_MIS or PT_KERNEL_AUTO's table asks for (plan_family, pt_plan.h): shadow rays
// have a stage in the pipeline (the pixel rides below nee_mask in the record, so it must fit) and a loop in the megakernel, nothing in
// the persistent kernel; the pipeline runs where it can (wave_ok), the megakernel does not read Woop records.
constexpr int path_kernel(int kernel, int walk, bool wave_ok, bool nee, bool pixels_fit) {
    if (nee && kernel != PT_KERNEL_MEGA_BVH2) kernel = wave_ok && pixels_fit ? PT_KERNEL_WAVEFRONT : PT_KERNEL_MEGA_BVH2;
    if (kernel == PT_KERNEL_WAVEFRONT && !wave_ok) kernel = PT_KERNEL_PERSISTENT;   // same images
    if (kernel == PT_KERNEL_MEGA_BVH2 && walk == ALG_WIDE_WOOP) kernel = PT_KERNEL_PERSISTENT;
    return kernel;
}

// ---- the ray-batch queries: k_query_rays<V>, the extend stage's two budgets
enum : uint32_t { QV_ANY = 1u << 0 };   // any-hit (pt_any_hits)
constexpr int QV_BUDGET_SHIFT = 1, QV_BITS = 4;
constexpr bool qv_any(uint32_t v) { return (v & QV_ANY) != 0; }
constexpr uint32_t qv_budget(uint32_t v) { return variant_field(v, QV_BUDGET_SHIFT, BUDGET_BITS); }
constexpr bool query_exists(uint32_t v) { return qv_budget(v) == BUDGET_8x16 || qv_budget(v) == BUDGET_6x24; }
constexpr uint32_t extend_budget(bool deep_stack) { return deep_stack ? BUDGET_6x24 : BUDGET_8x16; }   // deep_stack: PT_OPT_LDS_STACK 24
constexpr uint32_t query_word(bool any, bool deep_stack) { return (any ? (uint32_t)QV_ANY : 0u) | (extend_budget(deep_stack) << QV_BUDGET_SHIFT); }
static_assert(variant_count(query_exists, QV_BITS) == 4, "k_query_rays: closest and any-hit x 2 budgets");

// ---- the stage-split pipeline (pt_k_wave.hip).  What one call launches, decided once: which extend and which shade kernel every bounce runs.
enum WaveExtend { EXT_CLOSEST, EXT_ANY, EXT_FIRST, EXT_PACKET, EXT_FUSED };   // k_wf_extend<.., FIRST / ANY>, .._packet, .._packet_shade
enum WaveShade { SHADE_PLAIN, SHADE_BOUND, SHADE_LAST, SHADE_LAST_ANY, SHADE_NONE };   // k_wf_shade<..>, k_wf_shade_last_any, in EXT_FUSED
struct WavePlan {
    bool count, nee, deep_stack;   // instrumented kernels; PT_FLAG_NEE; the (6 waves, 24 entries) budget instead of (8, 16)
    bool packet;       // bounce 0 as wave-wide packets (PT_OPT_FIRST_WALK 1): the tree fits the packet stack budget (PT_OPT_PACKET_STACK)
    // PT_OPT_FUSE_STAGES 1, the product launch without PT_FLAG_NEE: bounce 0's shade runs in the packet walk's launch, and the last shade
    // launch folds the samples (fold_lp lanes per pixel) when every region holds all samples of its pixels (groups of spp = 16, 8 or 4)
    bool fuse_first;
    int fold_lp;
    // PT_OPT_LAST_ANYHIT: when no triangle can emit, a path's last segment reaches the picture only through the sphere or the background it
    // ends on.  The shade launch of bounce depth - 2 leaves the nearest sphere of every survivor's new ray in its hit slot, the walk of bounce
    // depth - 1 is an any-hit query bounded by it, the last shade launch reads the verdict.
    bool anyhit;
    // PT_OPT_ROOT_CULL: the shade launches keep the survivors whose new ray the tree's root turns away out of the next extend launch's
    // queue (wf_survivor_slot).
    bool root_cull;
    // PT_OPT_ROOT_ENTRY: ... and leave the rest of that node step in the walkers' records as an entry code, from which the extend launches
    // of bounces >= 1 start below the root (k_wf_extend<.., ENTRY>).  Only with root_cull, without PT_FLAG_NEE (its shadow records carry
    // no code, and ray1.w's top bit is taken) and when spp fits the narrowed sample field; every other call keeps the plain record.
    bool root_entry;
    // PT_OPT_PATH_HISTORY: the records carry the objects the path has hit (the history word of pt_kernels.h) in place of its mask, a
    // shade lane rebuilds mask and accu from it, and a path's sample colour is written once, by the lane it ends in (path_history_holds).
    bool history;
    // PT_OPT_LAST_OCCLUDERS: the launch that bounds the last segments (SHADE_BOUND, or EXT_FUSED at depth 2) tests its walkers against the
    // tree's occluder table and keeps the decided ones out of the any-hit launch's queue (last_occluders_hold).
    bool occluders;
    constexpr WaveExtend extend(uint32_t b, uint32_t depth) const {
        if (b == 0) return fuse_first ? EXT_FUSED : packet ? EXT_PACKET : EXT_FIRST;
        return anyhit && b + 1 == depth ? EXT_ANY : EXT_CLOSEST;
    }
    constexpr WaveShade shade(uint32_t b, uint32_t depth) const {
        if (b == 0 && fuse_first) return SHADE_NONE;
        if (anyhit && b + 1 >= depth) return SHADE_LAST_ANY;   // behind the any-hit walk: the verdict's emission only
        if (anyhit && b + 2 == depth) return SHADE_BOUND;      // its survivors' rays are the last segments: their sphere bound
        if (b != 0 && !nee && !count && b + 1 >= depth) return SHADE_LAST;   // the final bounce: emission only
        return SHADE_PLAIN;
    }
};
// The options with the values 0 / 1 / 2 (PT_OPT_LAST_ANYHIT, _ROOT_CULL, _ROOT_ENTRY, _LAST_OCCLUDERS, _PATH_HISTORY): 1 switches the
// product launches, instrumented launches only follow with 2.
constexpr bool stage_option_on(bool count, int value) { return count ? value == 2 : value >= 1; }
// PT_OPT_LAST_OCCLUDERS: whether the shade launch that bounds the last segments also tests its walkers against the tree's occluder list:
// the any-hit launch runs behind it (that launch's own rule: WavePlan::anyhit), the launch classifies its survivors at all (root cull:
// the decided lanes join the walk-free class), and the tree has a list.
constexpr bool last_occluders_hold(bool tree_has_list, bool anyhit_launch, bool root_cull) { return anyhit_launch && root_cull && tree_has_list; }
// what wave_plan (pt_k_wave.hip) reads off the context, the call and the tree
struct WaveRequest {
    bool count, nee, deep_stack, moments;   // PT_OPT_COUNTERS; PT_FLAG_NEE; PT_OPT_LDS_STACK 24; pt_render_moments
    bool packet;           // PT_OPT_FIRST_WALK 1 and the tree fits the packet stack budget
    bool anyhit_scene;     // no triangle can emit, one triangle material, the spheres fit the kernel arguments, exact records
    bool history_holds;    // path_history_holds (pt_plan.h); never with PT_FLAG_NEE
    bool tree_has_occluders;
    bool spp_fits_entry;   // spp < PT_REC_MAX_SAMPLES_ENTRY
    int fuse_stages, last_anyhit, root_cull, root_entry, path_history, last_occluders;   // the options' values
    uint32_t depth, spp, sgroup_log2;
};
constexpr WavePlan wave_plan_of(const WaveRequest& r) {
    WavePlan p = {};
    p.count = r.count; p.nee = r.nee; p.deep_stack = r.deep_stack;
    p.packet = r.packet;
    const bool fuse = r.fuse_stages != 0 && !r.nee && !r.count;
    p.fuse_first = fuse && p.packet;
    // ... and the call keeps no luminance moments (pt_render_moments): those are the separate fold launch's job
    p.fold_lp = fuse && !r.moments && r.depth >= 2 && r.sgroup_log2 >= 2 && r.sgroup_log2 <= 4 && r.spp == (1u << r.sgroup_log2) ? (int)r.spp / 4 : 0;
    p.anyhit = stage_option_on(r.count, r.last_anyhit) && r.depth >= 2 && !r.nee && r.anyhit_scene;
    p.root_cull = stage_option_on(r.count, r.root_cull);
    p.history = stage_option_on(r.count, r.path_history) && r.history_holds;
    p.occluders = stage_option_on(r.count, r.last_occluders) && last_occluders_hold(r.tree_has_occluders, p.anyhit, p.root_cull);
    p.root_entry = p.root_cull && !r.nee && r.spp_fits_entry && stage_option_on(r.count, r.root_entry);
    return p;
}

// the extend stage: k_wf_extend<COUNT, V> at the two budgets; bounce 0 (FIRST) has neither a bound nor an entry code
enum : uint32_t { WX_COUNT = 1u << 0, WX_FIRST = 1u << 1, WX_ANY = 1u << 2, WX_ENTRY = 1u << 3 };
constexpr int WX_BUDGET_SHIFT = 4, WX_BITS = 7;
constexpr bool wx_count(uint32_t v) { return (v & WX_COUNT) != 0; }
constexpr bool wx_first(uint32_t v) { return (v & WX_FIRST) != 0; }
constexpr bool wx_any(uint32_t v) { return (v & WX_ANY) != 0; }
constexpr bool wx_entry(uint32_t v) { return (v & WX_ENTRY) != 0; }
constexpr uint32_t wx_budget(uint32_t v) { return variant_field(v, WX_BUDGET_SHIFT, BUDGET_BITS); }
constexpr bool extend_exists(uint32_t v) {
    return (wx_budget(v) == BUDGET_8x16 || wx_budget(v) == BUDGET_6x24) && !(wx_first(v) && (wx_any(v) || wx_entry(v)));
}
constexpr uint32_t extend_word(const WavePlan& p, WaveExtend kind) {   // kind: EXT_FIRST, EXT_ANY or EXT_CLOSEST
    const uint32_t v = (p.count ? (uint32_t)WX_COUNT : 0u) | (extend_budget(p.deep_stack) << WX_BUDGET_SHIFT);
    if (kind == EXT_FIRST) return v | WX_FIRST;
    return v | (kind == EXT_ANY ? (uint32_t)WX_ANY : 0u) | (p.root_entry ? (uint32_t)WX_ENTRY : 0u);
}
static_assert(variant_count(extend_exists, WX_BITS) == 20, "k_wf_extend: 2 x 2 budgets x (FIRST + closest / any x entry)");

// the shade stage: k_wf_shade<COUNT, V>, k_wf_shade_last_any<COUNT, V> and k_wf_extend_packet_shade<V> share these bits
enum : uint32_t { WS_COUNT = 1u << 0, WS_NEE = 1u << 1, WS_FIRST = 1u << 2, WS_LAST = 1u << 3, WS_BOUND = 1u << 4, WS_HIST = 1u << 5, WS_OCCL = 1u << 6 };
constexpr int WS_FOLD_SHIFT = 7, WS_FOLD_BITS = 2, WS_BITS = 9;   // the fold field: 0 none, else 1 + log2(lanes per pixel)
constexpr bool ws_count(uint32_t v) { return (v & WS_COUNT) != 0; }
constexpr bool ws_nee(uint32_t v) { return (v & WS_NEE) != 0; }
constexpr bool ws_first(uint32_t v) { return (v & WS_FIRST) != 0; }
constexpr bool ws_last(uint32_t v) { return (v & WS_LAST) != 0; }
constexpr bool ws_bound(uint32_t v) { return (v & WS_BOUND) != 0; }
constexpr bool ws_hist(uint32_t v) { return (v & WS_HIST) != 0; }
constexpr bool ws_occl(uint32_t v) { return (v & WS_OCCL) != 0; }
constexpr int ws_fold(uint32_t v) { return variant_field(v, WS_FOLD_SHIFT, WS_FOLD_BITS) ? 1 << (variant_field(v, WS_FOLD_SHIFT, WS_FOLD_BITS) - 1u) : 0; }   // lanes per pixel: 0, 1, 2, 4
constexpr uint32_t ws_fold_field(int fold_lp) { return (fold_lp == 4 ? 3u : (uint32_t)fold_lp) << WS_FOLD_SHIFT; }
// k_wf_shade: only a launch that bounds the last segments tests occluders; only the emission-only last launch (never bounce 0, never
// bounding) folds; NEE kernels are never LAST, BOUND, HIST or folding (k_wf_resolve adds in place behind them); instrumented ones never
// LAST or folding (they count the last bounce's paths like any other's)
constexpr bool shade_exists(uint32_t v) {
    if (ws_occl(v) && !ws_bound(v)) return false;
    if (ws_fold(v) && !ws_last(v)) return false;
    if (ws_last(v) && (ws_first(v) || ws_bound(v) || ws_nee(v) || ws_count(v))) return false;
    return !ws_nee(v) || !(ws_bound(v) || ws_hist(v));
}
// k_wf_shade_last_any: instrumented, history, fold — an instrumented one never folds
constexpr bool shade_last_any_exists(uint32_t v) {
    return (v & (WS_NEE | WS_FIRST | WS_LAST | WS_BOUND | WS_OCCL)) == 0 && !(ws_count(v) && ws_fold(v));
}
// k_wf_extend_packet_shade: bounce 0's product launch without NEE — bound (with or without occluders) and history
constexpr bool fused_exists(uint32_t v) { return (v & ~(uint32_t)(WS_BOUND | WS_HIST | WS_OCCL)) == 0 && !(ws_occl(v) && !ws_bound(v)); }
// kind: SHADE_PLAIN, SHADE_BOUND, SHADE_LAST (k_wf_shade) or SHADE_LAST_ANY (k_wf_shade_last_any); first: bounce 0
constexpr uint32_t shade_word(const WavePlan& p, WaveShade kind, bool first) {
    uint32_t v = (p.count ? (uint32_t)WS_COUNT : 0u) | (p.nee ? (uint32_t)WS_NEE : 0u) | (p.history ? (uint32_t)WS_HIST : 0u);
    if (kind == SHADE_LAST_ANY) return v | ws_fold_field(p.fold_lp);
    if (first) v |= WS_FIRST;
    if (kind == SHADE_LAST) v |= WS_LAST | ws_fold_field(p.fold_lp);
    if (kind == SHADE_BOUND) v |= WS_BOUND | (p.occluders ? (uint32_t)WS_OCCL : 0u);
    return v;
}
constexpr uint32_t fused_word(const WavePlan& p, uint32_t depth) {   // (BOUND at depth 2: bounce 0's survivors are the last segments)
    return (p.history ? (uint32_t)WS_HIST : 0u) | (p.anyhit && depth == 2 ? WS_BOUND | (p.occluders ? (uint32_t)WS_OCCL : 0u) : 0u);
}
static_assert(variant_count(shade_exists, WS_BITS) == 36, "k_wf_shade: 4 NEE + 2 histories x (6 instrumented + 4 last + 6 others)");
static_assert(variant_count(shade_last_any_exists, WS_BITS) == 10, "k_wf_shade_last_any: 2 histories x (instrumented + 4 folds)");
static_assert(variant_count(fused_exists, WS_BITS) == 6, "k_wf_extend_packet_shade: 2 histories x (plain, bound, bound + occluders)");
