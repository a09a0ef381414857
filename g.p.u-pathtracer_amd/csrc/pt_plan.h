// pt_plan.h — what every call runs, decided in plain C++: the argument rules of the path calls, the walk, the kernel family, the side
// stream, the sample and LDS layouts, the queue and the grids, the stage-split pipeline's records and launches, the plans of
// pt_render_rays, of pt_select_pixels and of the ray-batch queries, the argument rules of every image-stage call.  Every function here is a pure function of plain facts: what the context holds
// (CtxFacts, filled by ctx_facts in ptmi.hip), what the caller passed (CallFacts) and the two answers only the runtime has (whether the
// caller's stream is idle; PT_KERNEL_AUTO's table).  The entry points gather the facts, ask, and apply the answer; the check program
// (pt_variants_check.cpp) asks the same functions over a domain of scenes x options x calls on the host.  No HIP call, no HIP type.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>

#include "../../include/ptmi.h"
#include "pt_variants.h"

namespace ptmi {

// ---- the facts -----------------------------------------------------------------------------------
struct CtxFacts {
    bool has_bvh, records_woop;                                     // the tree on the context
    uint32_t wide_depth, n_top_layout, wide_top_layout, n_occ;
    int n_spheres, sphere_mat[PT_KSPHERES];                         // ... the spheres, the materials of the first ones
    bool mat_table, tri_emits;                                      // pt_upload_tri_materials: a table is set; one of its triangles emits
    int env, n_cu;                                                  // env_code of the map; compute units
    // the options planning reads, by pt_set_option's names
    int kernel, counters, timing, overlap, sph_lds, top, occ, lstk, walk, batch, refill, vote_node, vote_rec;
    int wave_batch, wave_samples, wave_blocks, first_walk, packet_stack, fuse_stages, last_anyhit, root_cull, root_entry, last_occluders, path_history;
};
struct CallFacts {
    bool frame;            // pt_render / pt_render_moments; else pt_render_rays
    const pt_params* p;
    uint32_t spp;
    bool buffers, rgba, moments;   // every required pointer but p is given; rgba_dev; moments_dev (frame)
    uint64_t n_rays;       // pt_render_rays; pt_render_camera: its rows
    int mode;
    // pt_render_camera (else pt_render_rays): buffers counts cam and cm in; whether a pixel list is given; first_pixel without one
    bool camera = false;
    const pt_camera_model* cm = nullptr;
    bool list = false;
    uint64_t first_pixel = 0;
    // pt_render_pixels (a camera call): buffers counts accum_dev and counts_dev in, moments is moments_dev; without a list its rows are the whole image
    bool pixels = false;
};
inline const char* path_call_name(const CallFacts& a) { return a.frame ? "pt_render" : a.pixels ? "pt_render_pixels" : a.camera ? "pt_render_camera" : "pt_render_rays"; }
// A call the rules turn away (code != PT_OK, with pt_last_error's text), or one with nothing to do (nothing: PT_OK at once)
struct Refusal {
    int code = PT_OK;
    std::string msg;
    bool nothing = false;
};

// ---- the rules of a camera model and the pixels asked of it, in pt_camera_rays' order and wording under the caller's name: an unknown
// model or flag bits, the image, n, first_pixel + n without a list (whole: n is the image, pt_render_pixels), the chosen model's own parameter
// (the others are ignored)
inline bool plan_finite(float x) { return x - x == 0.0f; }   // neither an infinity nor a NaN
inline Refusal check_camera_model(const std::string& who, const pt_camera_model& cm, uint64_t n, uint64_t first_pixel, bool list, bool whole = false) {
    if (cm.model < PT_CAM_PINHOLE || cm.model > PT_CAM_EQUIRECT) return {PT_ERR_INVALID, who + ": unknown camera model"};
    if (cm.flags & ~PT_CAMF_CENTRE) return {PT_ERR_INVALID, who + ": unknown flag bits"};
    const uint64_t n_pix = (uint64_t)(cm.width > 0 ? cm.width : 0) * (uint64_t)(cm.height > 0 ? cm.height : 0);
    if (cm.width < 2 || cm.height < 2 || n_pix >= (1ull << 32)) return {PT_ERR_INVALID, who + ": width and height must be >= 2 with width * height < 2^32"};
    if (n >= (1ull << 32)) return {PT_ERR_INVALID, who + ": more than 2^32 - 1 rays in one call"};
    if (!list && whole && n != n_pix) return {PT_ERR_INVALID, who + ": without a pixel list n must equal width * height"};
    if (!list && (first_pixel > n_pix || n > n_pix - first_pixel)) return {PT_ERR_INVALID, who + ": first_pixel + n exceeds width * height"};
    switch (cm.model) {
    case PT_CAM_THIN_LENS:
        if (!plan_finite(cm.lens_radius) || cm.lens_radius < 0.0f || !plan_finite(cm.focus_dist) || !(cm.focus_dist > 0.0f))
            return {PT_ERR_INVALID, who + ": lens_radius must be finite and >= 0, focus_dist finite and > 0"};
        break;
    case PT_CAM_ORTHO:
        if (!plan_finite(cm.ortho_height) || !(cm.ortho_height > 0.0f)) return {PT_ERR_INVALID, who + ": ortho_height must be finite and > 0"};
        break;
    case PT_CAM_FISHEYE:
        if (!plan_finite(cm.fisheye_fov) || !(cm.fisheye_fov > 0.0f) || cm.fisheye_fov > 6.28318548f) return {PT_ERR_INVALID, who + ": fisheye_fov must be in (0, 2 pi]"};
        break;
    default: break;
    }
    return {};
}
// ... asked for the model's whole image: n = width * height from pixel 0 (pt_render_aux_camera, pt_temporal_camera)
inline Refusal check_camera_model_image(const std::string& who, const pt_camera_model& cm) {
    return check_camera_model(who, cm, (uint64_t)(cm.width > 0 ? cm.width : 0) * (uint64_t)(cm.height > 0 ? cm.height : 0), 0, false, true);
}

// ---- the argument rules of pt_render, pt_render_rays, pt_render_camera and pt_render_pixels, each call's in its own order and wording
inline Refusal check_path_call(const CtxFacts& f, const CallFacts& a) {
    const std::string who(path_call_name(a));
    const bool no_scene = !f.has_bvh && f.n_spheres == 0;
    if (!a.frame) {
        if (no_scene) return {PT_ERR_NO_SCENE, who + ": no scene uploaded"};
        if (a.n_rays == 0 || a.spp == 0) return {PT_OK, "", true};
    }
    if (!a.buffers || !a.p) return {PT_ERR_INVALID, who + ": null argument"};
    const pt_params& p = *a.p;
    if (a.frame) {
        if (p.width < 2 || p.height < 2) return {PT_ERR_INVALID, "pt_render: image must be at least 2x2 (the camera divides by w-1, h-1)"};
        if (a.spp == 0) return {PT_ERR_INVALID, "pt_render: spp must be >= 1"};
    } else {
        if (a.mode != PT_RAYS_CLAMPED && a.mode != PT_RAYS_HDR) return {PT_ERR_INVALID, who + ": mode must be PT_RAYS_CLAMPED or PT_RAYS_HDR"};
        if (a.camera) {
            const Refusal r = check_camera_model(who, *a.cm, a.n_rays, a.first_pixel, a.list, a.pixels);
            if (r.code != PT_OK) return r;
        } else if (a.n_rays >= (1ull << 32)) return {PT_ERR_INVALID, who + ": more than 2^32 - 1 rays in one call"};
    }
    if (p.sample_index == 0) return {PT_ERR_INVALID, who + (a.frame ? ": sample_index (constantPdf) starts at 1" : ": sample_index starts at 1")};
    if (p.tri_mat < PT_MAT_DIFF || p.tri_mat > PT_MAT_REFR) return {PT_ERR_INVALID, who + ": bad triangle material"};
    if (a.frame && (p.flags & PT_FLAG_WRITE_RGBA) && !a.rgba) return {PT_ERR_INVALID, "pt_render: PT_FLAG_WRITE_RGBA needs rgba_dev"};
    if ((p.flags & PT_FLAG_NEE) && !(p.flags & PT_FLAG_COSINE_DIFF))
        return {PT_ERR_INVALID, who + ": PT_FLAG_NEE needs PT_FLAG_COSINE_DIFF" + (a.frame ? " (the reference's DIFF lobe has no density to weigh a light sample against)" : "")};
    if ((p.flags & PT_FLAG_MIS) && !(p.flags & PT_FLAG_NEE))
        return {PT_ERR_INVALID, who + ": PT_FLAG_MIS needs PT_FLAG_NEE" + (a.frame ? " (it weighs NEE's shadow rays against the bounce rays)" : "")};
    if (!a.frame) return {};
    if (no_scene) return {PT_ERR_NO_SCENE, "pt_render: no scene uploaded"};
    if (p.part_count > 1) {
        if (p.part_index < 0 || p.part_index >= p.part_count) return {PT_ERR_INVALID, "pt_render: part_index out of range"};
        if (p.part_rows <= 0 || (p.part_rows % PT_TILE) != 0) return {PT_ERR_INVALID, "pt_render: part_rows must be a positive multiple of 8"};
    }
    return {};
}

// ---- the rules every entry point shares, each written here once ----------------
// PT_FLAG_NEE over emissive triangles: the call samples the light list, which is copied out of exact records
inline bool samples_tri_lights(const CtxFacts& f, uint32_t flags) { return (flags & PT_FLAG_NEE) && f.has_bvh && f.tri_emits; }
inline Refusal tri_lights_rule(const CtxFacts& f, uint32_t flags) {
    if (samples_tri_lights(f, flags) && f.records_woop) return {PT_ERR_UNSUPPORTED, "pt_render: PT_FLAG_NEE over emissive triangles needs the exact (Moller-Trumbore) records"};
    return {};
}
// The wide walk pushes up to three entries per level: whether a stack of `cap` entries holds it for this tree.
inline bool wide_walk_fits(const CtxFacts& f, int cap) { return f.has_bvh && 3 * f.wide_depth + 2 <= (uint32_t)cap; }
// The walk a path call runs (LaunchCfg::walk) under PT_OPT_WALK, or PT_ERR_UNSUPPORTED in `who`'s name: Woop records are only
// understood by the wide walk, a tree too deep for it takes the unified binary walk.  postponed: the caller has walk 4, else it runs as 2.
// PT_FLAG_MIS: never over Woop records (the megakernel does not read them, k_render_rays has no such instantiation).
inline Refusal choose_walk(const CtxFacts& f, const char* who, bool postponed, bool mis, int& walk) {
    const bool wide_ok = wide_walk_fits(f, PT_STACK_CAP);
    if (f.has_bvh && f.records_woop) {
        if (!wide_ok) return {PT_ERR_UNSUPPORTED, std::string(who) + ": Woop records need the wide walk and this tree is too deep for it"};
        walk = ALG_WIDE_WOOP;
        if (mis) return {PT_ERR_UNSUPPORTED, std::string(who) + ": PT_FLAG_MIS needs the exact (Moller-Trumbore) records (upload with PT_OPT_TRI_TEST 0)"};
        return {};
    }
    walk = f.walk == ALG_WIDE_PEND && !postponed ? (int)ALG_WIDE : f.walk;
    if (walk >= ALG_WIDE && !wide_ok) walk = ALG_UNIFIED;
    return {};
}
// PT_OPT_PATH_HISTORY: whether a call's masks and gathered light are functions of the objects its paths hit, in path_shade_hit's
// DIFF / SPEC / METAL arithmetic (mask *= colour, accu += mask * emission) — nothing scales the colour (the roulettes), nothing adds in
// place beside the shade lanes (PT_FLAG_NEE: k_wf_resolve), every object has a history code and a row in the shade stage's table (the
// spheres of the kernel-argument block, ONE triangle material), no REFR branch scales the mask, and the word holds the codes.
inline bool path_history_holds(const CtxFacts& f, const pt_params& p) {
    if ((p.flags & (PT_FLAG_NEE | PT_FLAG_RUSSIAN_ROULETTE | PT_FLAG_RR_CPU_TRACER)) || f.mat_table || f.n_spheres > PT_KSPHERES ||
        p.tri_mat == PT_MAT_REFR || p.depth > PT_HIST_MAX_DEPTH)
        return false;
    for (int i = 0; i < f.n_spheres; i++)
        if (f.sphere_mat[i] == PT_MAT_REFR) return false;
    return true;
}
// LDS bytes of a frame-kernel block, top-of-tree planes + stack, with the largest n_top (halved from the one asked for) that fits
// 160 KiB: a deep tree gives the LDS to the stack first
constexpr size_t PT_LDS_BYTES = 160 * 1024;
inline size_t lds_fit(int& n_top, int stack_n, int block) {
    const size_t stack = (size_t)stack_n * block * 4;
    while (n_top > 0 && (size_t)n_top * 64 + stack > PT_LDS_BYTES) n_top /= 2;
    return (size_t)n_top * 64 + stack;
}
// the sphere table of a persistent kernel's block (PT_OPT_SPHERE_LDS) behind what `lds` holds: its first word; `lds` grows by it
inline int lds_sphere_table(size_t& lds) { lds += 15 * PT_KSPHERES * 4; return (int)(lds / 4) - 15 * PT_KSPHERES; }
// The binary walk with one thread per ray (pt_trace_rays, the deep-tree queries, pt_render_aux): all PT_STACK_CAP entries and the top
// of the tree (n_top nodes) in LDS.  Returns the LDS bytes of a block of PT_BLOCK_RAYS.
inline size_t binary_ray_lds(const CtxFacts& f, int& n_top) {
    n_top = (int)std::min<uint32_t>((uint32_t)f.top, f.n_top_layout);
    return lds_fit(n_top, PT_STACK_CAP, PT_BLOCK_RAYS);
}
// queue granularity: 64-slot chunks when the launch has plenty of them per resident wave, smaller ones for small launches (an
// eighth of a 1080p frame per GPU is ~4 000 tiles for ~5 000 waves)
inline int queue_chunk(int n_cu, uint64_t slots) {
    const uint64_t waves = (uint64_t)n_cu * 20;
    return slots / 64 >= 4 * waves ? 64 : (slots / 32 >= 4 * waves ? 32 : 16);
}
// the knobs of a persistent launch's queue.  refill <= batch, or a wave can spin: the walk returns at once because `batch` lanes wait,
// none of them has anything to shade and the idle ones are too few to trigger a refill
struct QueueKnobs { int batch, refill, vote_node, vote_rec; };
inline QueueKnobs queue_knobs(const CtxFacts& f) { return {f.batch, std::min(f.refill, f.batch), f.vote_node, f.vote_rec}; }
// samples of one pixel that share a wave at bounce 0 of the stage-split pipeline, as a power of two (wf_slot_pixel): the largest
// 2^k <= PT_OPT_WAVE_SAMPLES, k >= 2, that divides spp; else 0 (one sample of a whole tile per wave, the other kernels' order)
inline uint32_t wave_sample_group_log2(uint32_t spp, int cap) {
    for (int k = 6; k >= 2; k--)
        if ((1 << k) <= cap && (spp & ((1u << k) - 1u)) == 0u) return (uint32_t)k;
    return 0u;
}
// most RNG draws one bounce can make with these flags (path_shade_hit): DIFF 4, or 2 cosine-weighted (+ 3 for the light
// sample of PT_FLAG_NEE), METAL 2, REFR 1, + 1 per roulette switch
inline uint32_t draws_per_bounce(uint32_t flags) {
    uint32_t k = (flags & PT_FLAG_COSINE_DIFF) ? 2u : 4u;
    if (flags & PT_FLAG_NEE) k += 3u;
    if (flags & PT_FLAG_RUSSIAN_ROULETTE) k += 1u;
    if (flags & PT_FLAG_RR_CPU_TRACER) k += 1u;
    return k;
}

// ---- pt_render ------------------------------------------------------------------------------------
// The tiles of a frame call: tiles_x tiles per tile-row; the call covers n_tiles tiles of the tile-rows its part owns (stripes of
// stripe_tr tile-rows, round-robin).  n_tiles <= 0: the part owns no tile, nothing to render.
struct TileGrid { int tiles_x, tile_rows, part_index, part_count, stripe_tr, n_tiles; };
inline Refusal frame_tiles(const pt_params& p, uint32_t spp, TileGrid& g) {
    g.tiles_x = (p.width + PT_TILE - 1) / PT_TILE;
    g.tile_rows = (p.height + PT_TILE - 1) / PT_TILE;
    if (p.part_count > 1) {
        g.part_index = p.part_index; g.part_count = p.part_count; g.stripe_tr = p.part_rows / PT_TILE;
        const int n_stripes = (g.tile_rows + g.stripe_tr - 1) / g.stripe_tr;
        const int owned = (n_stripes - p.part_index + p.part_count - 1) / p.part_count;  // stripes index, index+count, ...
        g.n_tiles = owned * g.stripe_tr * g.tiles_x;
    } else {
        g.part_index = 0; g.part_count = 1; g.stripe_tr = 1;
        g.n_tiles = g.tile_rows * g.tiles_x;
    }
    if (g.n_tiles <= 0) return {PT_OK, "", true};
    if ((uint64_t)g.n_tiles * 64u * (uint64_t)spp >= (1ull << 31)) return {PT_ERR_INVALID, "pt_render: width*height*spp too large for one call (split the samples over several calls)"};
    return {};
}

struct LaunchCfg {
    bool count;        // instrumented instantiation (PT_OPT_COUNTERS)
    int occ;           // waves per SIMD the registers are budgeted for
    int lstk;          // LDS stack entries per lane (16, 24 or PT_STACK_CAP)
    int walk;          // 0 while-while, 1 unified, 2 wide, 3 wide over Woop records, 4 wide + postponed leaf
    size_t lds;        // dynamic LDS bytes of a block
    int blocks;        // megakernel grid (one wave per work tile)
    int work_blocks;   // persistent grid cap: blocks that have work at all
    int n_cu;
    bool moments;      // the call keeps luminance moments (pt_render_moments): they are the separate fold launch's job
    int env;           // the context's environment map (env_code, pt_variants.h): ENV_NONE, ENV_LOOKUP, or ENV_LIGHT with PT_OPT_ENV_LIGHT's tables
    bool nee, mis;     // the call has PT_FLAG_NEE; PT_FLAG_MIS: the instantiations that weigh shadow rays against bounce rays
};
// the variant words (pt_variants.h) the launchers of the kernels that shade in the lane that walked ask for
inline uint32_t mega_word(const LaunchCfg& L) { return ::mega_word(L.count, L.occ, L.lstk, L.walk, L.env, L.mis); }
inline uint32_t persist_word(const LaunchCfg& L) { return ::persist_word(L.count, L.occ, L.lstk, L.walk, L.env); }
inline uint32_t rays_word(const LaunchCfg& L) { return ::rays_word(L.walk, L.env, L.nee, L.mis); }

// One call's path records in the stage-split pipeline: the pieces in the order they lie in the context's buffer, two generations of
// ray0, ray1, mask (3 planes; PT_OPT_PATH_HISTORY uses the first: the history words), cnt and walk (bounce b reads [b & 1] and writes the
// other), the frame hashes, the queue counters of every extend launch, and under PT_FLAG_NEE the shadow records.
enum WavePiece { W_RAY0, W_RAY1 = 2, W_MASK = 4, W_HIT = 6, W_CNT, W_WALK = 9, W_HASHES = 11, W_QUEUES, W_S_RAY0, W_S_RAY1, W_S_CON, W_S_HIT, W_S_CNT, W_PIECES };
struct WaveLayout {
    size_t n_regions, cap, q_words, need;
    size_t off[W_PIECES + 1];   // byte offset of every piece; piece i ends where i + 1 begins, the last at `need`
    bool nee;
};
// ... or the refusal of a call beyond the limits of the record's packed fields (pt_variants.h): the RNG draw count (2 camera draws +
// draws_per_bounce per bounce), the sample number, the slot
inline Refusal plan_wave_layout(uint32_t flags, uint32_t depth, uint32_t spp, int work_tiles, WaveLayout& w) {
    if ((uint64_t)depth * draws_per_bounce(flags) + 2u >= PT_REC_MAX_DRAWS || spp >= PT_REC_MAX_SAMPLES)
        return {PT_ERR_UNSUPPORTED, "pt_render: PT_KERNEL_WAVEFRONT packs < " + std::to_string(PT_REC_MAX_DRAWS) + " RNG draws per path (2 + depth x 4..9, by flags) and < " +
                                        std::to_string(PT_REC_MAX_SAMPLES) + " samples per call into a path record"};
    w.n_regions = ((size_t)work_tiles + PT_REGION / 64 - 1) / (PT_REGION / 64);
    w.cap = w.n_regions * PT_REGION;
    if (w.cap >= (1ull << 31)) return {PT_ERR_INVALID, "pt_render: too many path records for one call"};
    w.nee = (flags & PT_FLAG_NEE) != 0;
    if (w.nee && spp >= PT_REC_MAX_SAMPLES_NEE)
        return {PT_ERR_UNSUPPORTED, "pt_render: PT_FLAG_NEE in the stage-split pipeline packs < " + std::to_string(PT_REC_MAX_SAMPLES_NEE) + " samples per call into a path record"};
    const size_t b_ray = w.cap * 16, b_mask = w.cap * 12, b_hit = w.cap * 8, b_cnt = ((w.n_regions * 4 + 255) / 256) * 256, b_hash = (((size_t)spp * 8 + 255) / 256) * 256;
    w.q_words = (size_t)depth * (w.nee ? 2 : 1) * PT_SHARDS * PT_SHARD_STRIDE;   // one set of queue counters per extend launch
    const size_t s = w.nee ? 1 : 0;   // the shadow records: s_ray0, s_ray1, s_con as rays, s_hit, s_cnt
    const size_t bytes[W_PIECES] = {b_ray, b_ray, b_ray, b_ray, b_mask, b_mask, b_hit, b_cnt, b_cnt, b_cnt, b_cnt, b_hash, w.q_words * 4,
                                    s * b_ray, s * b_ray, s * b_ray, s * b_hit, s * b_cnt};
    w.off[0] = 0;
    for (int i = 0; i < W_PIECES; i++) w.off[i + 1] = w.off[i] + bytes[i];
    w.need = w.off[W_PIECES];
    return {};
}

// What one call runs and with which buffers, decided once and in steps, split where the runtime has to be asked:
//   plan_walk    the walk, and whether PT_KERNEL_AUTO looks the configuration up at all (lookup)
//   plan_family  given AUTO's answer, the kernel family (path_kernel), and whether the caller's stream is asked if it is idle (idle_query)
//   plan_launch  given that answer, the rest: side stream, samples, LDS, queue, grids, and the pipeline's records and launches
// Nothing after plan_launch changes the plan or refuses the call.
struct CallPlan {
    int kernel;               // PT_KERNEL_MEGA_BVH2, PT_KERNEL_PERSISTENT or PT_KERNEL_WAVEFRONT (before plan_family: what the option asks for)
    bool wave_ok, lookup, idle_query;
    int probe;                // PT_KERNEL_AUTO: this call is timed trial `probe` of its configuration; -1: it is none
    bool side;                // the path kernel runs on a side stream (PT_OPT_OVERLAP)
    bool samples;             // ... into a sample buffer that a fold reads afterwards
    uint32_t sgroup_log2;     // the samples of a pixel side by side in the slot order and in the sample buffer (wave_sample_group_log2)
    int n_top, sph_tab;       // LDS: nodes mirrored, first word of the sphere table (-1: none)
    int chunk, work_tiles;    // queue granularity in slots, 64-slot work items of the call
    LaunchCfg L;              // walk, stack window, LDS bytes, grids
    QueueKnobs q;
    // the pipeline's share (kernel == PT_KERNEL_WAVEFRONT): the records, which kernel every bounce runs, the extend stage's knobs
    WaveLayout wl;
    WavePlan wave;
    int wave_batch, wave_blocks;
};
// PT_KERNEL_AUTO's answer for a call that looks its configuration up: the timed trial this call is (probe 0..3; even: the persistent
// kernel, odd: the pipeline) or -1, and then the decided choice, if there is one yet
struct AutoAnswer { int probe; bool decided; int choice; };

inline Refusal plan_walk(const CtxFacts& f, const CallFacts& a, CallPlan& plan) {
    plan = CallPlan();
    const bool nee = (a.p->flags & PT_FLAG_NEE) != 0, mis = (a.p->flags & PT_FLAG_MIS) != 0;
    const Refusal r = choose_walk(f, "pt_render", true, mis, plan.L.walk);
    // The stage-split pipeline needs a BVH, at least one bounce, the wide walk over exact records and a context without an
    // environment map (its last-segment any-hit launch shades misses without a ray in hand).
    plan.wave_ok = f.has_bvh && a.p->depth > 0 && plan.L.walk == ALG_WIDE && f.env == ENV_NONE;
    // PT_FLAG_MIS: the megakernel whatever the option says, and no trial — the pipeline's path record has no word for the bounce's density
    plan.kernel = mis ? (int)PT_KERNEL_MEGA_BVH2 : f.kernel;
    plan.probe = -1;
    plan.lookup = plan.kernel == PT_KERNEL_AUTO && plan.wave_ok && !f.counters && !nee;   // (an instrumented call is no trial; a call with shadow rays has no choice)
    return r;
}
// the kernel family, every rule once and in this order: the option; PT_KERNEL_AUTO's table; PT_FLAG_NEE and what a family cannot run
inline void plan_family(const CtxFacts& f, const CallFacts& a, const AutoAnswer& au, CallPlan& plan) {
    int kernel = plan.kernel;
    if (kernel == PT_KERNEL_AUTO) {
        kernel = PT_KERNEL_PERSISTENT;
        if (plan.lookup) {
            plan.probe = au.probe;
            if (au.probe >= 0) kernel = (au.probe & 1) ? PT_KERNEL_WAVEFRONT : PT_KERNEL_PERSISTENT;
            else if (au.decided) kernel = au.choice;
        }
    }
    plan.kernel = path_kernel(kernel, plan.L.walk, plan.wave_ok, (a.p->flags & PT_FLAG_NEE) != 0,
                              (uint64_t)a.p->width * (uint64_t)a.p->height <= (1ull << PT_REC_PIXEL_BITS));
    plan.idle_query = f.overlap && plan.kernel != PT_KERNEL_WAVEFRONT;
}
// What the pipeline launches for this call: WavePlan (pt_variants.h), from what the context, the call and the tree say
inline WavePlan wave_plan(const CtxFacts& f, const CallFacts& a, const CallPlan& plan) {
    const pt_params& p = *a.p;
    WaveRequest r = {};
    r.count = plan.L.count; r.nee = plan.L.nee; r.deep_stack = plan.L.lstk == 24; r.moments = a.moments;
    r.packet = f.first_walk == 1 && wide_walk_fits(f, f.packet_stack);
    const bool tri_dark = p.tri_emi[0] == 0.f && p.tri_emi[1] == 0.f && p.tri_emi[2] == 0.f;
    r.anyhit_scene = !f.mat_table && tri_dark && f.n_spheres <= PT_KSPHERES && !f.records_woop;
    r.history_holds = path_history_holds(f, p);
    r.tree_has_occluders = f.n_occ > 0;
    r.spp_fits_entry = a.spp < PT_REC_MAX_SAMPLES_ENTRY;
    r.fuse_stages = f.fuse_stages; r.last_anyhit = f.last_anyhit; r.root_cull = f.root_cull; r.root_entry = f.root_entry;
    r.path_history = f.path_history; r.last_occluders = f.last_occluders;
    r.depth = p.depth; r.spp = a.spp; r.sgroup_log2 = plan.sgroup_log2;
    return wave_plan_of(r);
}
inline Refusal plan_launch(const CtxFacts& f, const CallFacts& a, int n_tiles, bool caller_idle, CallPlan& plan) {
    LaunchCfg& L = plan.L;
    const bool persistent = plan.kernel == PT_KERNEL_PERSISTENT, wavefront = plan.kernel == PT_KERNEL_WAVEFRONT;
    // overlap with the previous call: the path kernel goes to a side stream with its own sample buffer and queue
    // counters, so it can start while the previous call's last paths drain (the tail of a call is as long as its
    // longest path: ~15 % of a one-sample 1080p call); instrumented, timed and trial calls run in line
    // ... and so does a call whose caller's stream is idle: a host that syncs before every launch (BasicScene.cpp:395) leaves nothing to
    // overlap with, and in line the call is two launches shorter (no cross-stream events; one sample folds inside the path kernel)
    plan.side = plan.idle_query && !f.counters && !f.timing && plan.probe < 0 && !caller_idle;
    // spp > 1: trace the samples as independent work items, fold them afterwards (k_fold_samples); the stage-split pipeline always
    // works that way, and the moments are the fold's job
    plan.samples = a.spp > 1 || wavefront || plan.side || a.moments;
    plan.sgroup_log2 = plan.samples && (wavefront || persistent) ? wave_sample_group_log2(a.spp, f.wave_samples) : 0u;
    plan.work_tiles = n_tiles * (plan.samples ? (int)a.spp : 1);

    L.lstk = f.lstk ? f.lstk : PT_STACK_CAP;   // any depth <= 64 works with every LDS window: deeper entries overflow
    plan.n_top = f.has_bvh ? (int)std::min<uint32_t>((uint32_t)f.top, L.walk >= ALG_WIDE ? f.wide_top_layout : f.n_top_layout) : 0;
    if (L.walk >= ALG_UNIFIED) plan.n_top = 0;  // only the while-while walk reads the LDS mirror
    L.lds = lds_fit(plan.n_top, L.lstk, PT_BLOCK);
    plan.sph_tab = persistent && f.sph_lds ? lds_sphere_table(L.lds) : -1;   // behind the stacks (and the LDS mirror)
    const long slots = (long)plan.work_tiles * 64;
    plan.chunk = queue_chunk(f.n_cu, (uint64_t)slots);
    plan.q = queue_knobs(f);
    const int waves_per_block = PT_BLOCK / 64;
    L.count = f.counters != 0;
    L.occ = f.occ;
    L.blocks = (plan.work_tiles + waves_per_block - 1) / waves_per_block;
    L.work_blocks = (int)((slots + plan.chunk * waves_per_block - 1) / (plan.chunk * waves_per_block));
    L.n_cu = f.n_cu;
    L.moments = a.moments;
    L.env = f.env;
    L.nee = (a.p->flags & PT_FLAG_NEE) != 0;
    L.mis = (a.p->flags & PT_FLAG_MIS) != 0;
    if (!wavefront) return {};
    plan.wave = wave_plan(f, a, plan);
    plan.wave_batch = f.wave_batch;
    plan.wave_blocks = f.wave_blocks;
    return plan_wave_layout(a.p->flags, a.p->depth, a.spp, plan.work_tiles, plan.wl);
}

// ---- pt_render_rays, pt_render_camera, pt_render_pixels (the same plan under the call's own name: its rows are the batch) ---
// slots of one launch: what keeps its sample buffer below 768 MiB; more samples than that go out as several launches, which the
// fold's order makes the same thing
constexpr uint64_t RAYS_MAX_SLOTS = 1ull << 26;
struct RaysPlan {
    LaunchCfg L;           // (no instrumented kernel; the register budget is rays_word's: by PT_FLAG_NEE)
    int sph_tab;
    QueueKnobs q;
    uint32_t per_launch;   // samples per launch
    bool samples;          // the launches go through the sample buffer and a fold: more than one sample per launch, or a call whose fold
                           // does more than the kernel's one-sample fold in line (pt_render_pixels: a count per pixel, the moments)
};
inline Refusal plan_rays(const CtxFacts& f, const CallFacts& a, RaysPlan& plan) {
    plan = RaysPlan();
    LaunchCfg& L = plan.L;
    L.nee = (a.p->flags & PT_FLAG_NEE) != 0;
    L.mis = (a.p->flags & PT_FLAG_MIS) != 0;
    const Refusal r = choose_walk(f, path_call_name(a), false, L.mis, L.walk);   // (0 runs as 1: the loop has no while-while walk)
    L.lstk = 16;
    L.lds = (size_t)L.lstk * PT_BLOCK * 4;
    plan.sph_tab = f.sph_lds ? lds_sphere_table(L.lds) : -1;
    L.n_cu = f.n_cu;
    L.env = f.env;
    plan.q = queue_knobs(f);
    plan.per_launch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(a.spp, RAYS_MAX_SLOTS / a.n_rays));
    plan.samples = plan.per_launch > 1 || a.pixels;
    return r;
}
// one launch of `spp_now` samples: its slots' queue chunk (the return value) and the blocks that have work at all
inline int plan_rays_launch(const CtxFacts& f, const CallFacts& a, const RaysPlan& plan, uint32_t spp_now, int& work_blocks) {
    const uint64_t slots = a.n_rays * (plan.samples ? spp_now : 1u);
    const int chunk = queue_chunk(f.n_cu, slots);
    work_blocks = (int)std::min<uint64_t>((slots + (uint64_t)chunk * 4 - 1) / ((uint64_t)chunk * 4), (uint64_t)INT_MAX);
    return chunk;
}

// ---- pt_select_pixels: its argument rules in the header's order (buffers: moments, counts, pixels and n_selected are all given);
// n_pix: width * height of a call that passes
inline Refusal check_select_call(const pt_select_params* sp, bool buffers, uint64_t& n_pix) {
    n_pix = 0;
    if (!sp || !buffers) return {PT_ERR_INVALID, "pt_select_pixels: null argument"};
    n_pix = (uint64_t)(sp->width > 0 ? sp->width : 0) * (uint64_t)(sp->height > 0 ? sp->height : 0);
    if (sp->width < 1 || sp->height < 1 || n_pix >= (1ull << 32)) return {PT_ERR_INVALID, "pt_select_pixels: width and height must be >= 1 with width * height < 2^32"};
    if (!plan_finite(sp->threshold) || sp->threshold < 0.0f) return {PT_ERR_INVALID, "pt_select_pixels: threshold must be finite and >= 0"};
    if (sp->min_samples > sp->max_samples) return {PT_ERR_INVALID, "pt_select_pixels: min_samples must not exceed max_samples"};
    return {};
}
// its launches: 256-pixel blocks, and the context's scratch — per block a double sum and a uint32 count, which the host reads back,
// and a uint32 list offset
struct SelectPlan { size_t n_blocks, read_back, scratch; };
inline SelectPlan plan_select(uint64_t n_pix) {
    SelectPlan s;
    s.n_blocks = (size_t)((n_pix + 255) / 256);
    s.read_back = s.n_blocks * 12;
    s.scratch = s.n_blocks * 16;
    return s;
}

// ---- pt_tonemap / pt_meter: their argument rules in the header's order (buffers: every required pointer but the parameters is given —
// tonemap: color_dev and one of out_dev, rgba_dev; meter: color_dev and state_dev); n_pix: width * height of a call that passes
inline Refusal check_tonemap_call(const pt_tonemap_params* tp, bool buffers, uint64_t& n_pix) {
    n_pix = 0;
    if (!tp || !buffers) return {PT_ERR_INVALID, "pt_tonemap: null argument"};
    n_pix = (uint64_t)(tp->width > 0 ? tp->width : 0) * (uint64_t)(tp->height > 0 ? tp->height : 0);
    if (tp->width < 1 || tp->height < 1 || n_pix >= (1ull << 32)) return {PT_ERR_INVALID, "pt_tonemap: width and height must be >= 1 with width * height < 2^32"};
    if (tp->curve < PT_TONE_CLAMP || tp->curve > PT_TONE_ACES || tp->transfer < PT_XFER_LINEAR || tp->transfer > PT_XFER_GAMMA22)
        return {PT_ERR_INVALID, "pt_tonemap: unknown curve or transfer"};
    if (!plan_finite(tp->exposure) || !(tp->exposure > 0.0f)) return {PT_ERR_INVALID, "pt_tonemap: exposure must be finite and > 0"};
    if (tp->curve == PT_TONE_REINHARD && !(tp->white > 0.0f)) return {PT_ERR_INVALID, "pt_tonemap: white must be > 0 (+inf: plain Reinhard)"};
    return {};
}
inline Refusal check_meter_call(const pt_meter_params* mp, bool buffers, uint64_t& n_pix) {
    n_pix = 0;
    if (!mp || !buffers) return {PT_ERR_INVALID, "pt_meter: null argument"};
    n_pix = (uint64_t)(mp->width > 0 ? mp->width : 0) * (uint64_t)(mp->height > 0 ? mp->height : 0);
    if (mp->width < 1 || mp->height < 1 || n_pix >= (1ull << 32)) return {PT_ERR_INVALID, "pt_meter: width and height must be >= 1 with width * height < 2^32"};
    if (!plan_finite(mp->key) || !(mp->key > 0.0f)) return {PT_ERR_INVALID, "pt_meter: key must be finite and > 0"};
    if (!(mp->low_pct >= 0.0f && mp->low_pct < mp->high_pct && mp->high_pct <= 1.0f)) return {PT_ERR_INVALID, "pt_meter: the percentages must hold 0 <= low_pct < high_pct <= 1"};
    if (!plan_finite(mp->min_exposure) || !plan_finite(mp->max_exposure) || !(mp->min_exposure > 0.0f) || !(mp->min_exposure <= mp->max_exposure))
        return {PT_ERR_INVALID, "pt_meter: the exposure limits must be finite with 0 < min_exposure <= max_exposure"};
    if (!(mp->adapt >= 0.0f && mp->adapt <= 1.0f)) return {PT_ERR_INVALID, "pt_meter: adapt must be in 0..1"};
    return {};
}
// their launches.  Tone map: four pixels per thread (three 16-byte loads, one 16-byte store of words) where the pixels come in fours
// and every buffer given is 16-byte aligned (`aligned16`), else one pixel per thread; 256-thread blocks.  Meter: the histogram pass'
// fixed grid of at most METER_BLOCKS blocks, whose threads stride, and the scratch [blocks][METER_BINS + 1] of uint32 counts (the last
// one: the unmetered pixels), reserved at its largest once
constexpr uint32_t METER_BINS = 256, METER_BLOCKS = 256;
constexpr size_t METER_SCRATCH_WORDS = (size_t)METER_BLOCKS * (METER_BINS + 1);
struct DisplayPlan { bool vec; uint64_t items; uint32_t n_blocks; };   // items: pixels, or groups of four (vec)
inline DisplayPlan plan_tonemap(uint64_t n_pix, bool aligned16) {
    DisplayPlan d;
    d.vec = aligned16 && n_pix % 4 == 0;
    d.items = d.vec ? n_pix / 4 : n_pix;
    d.n_blocks = (uint32_t)((d.items + 255) / 256);
    return d;
}
inline DisplayPlan plan_meter(uint64_t n_pix, bool aligned16) {
    DisplayPlan d;
    d.vec = aligned16 && n_pix % 4 == 0;
    d.items = d.vec ? n_pix / 4 : n_pix;
    d.n_blocks = (uint32_t)std::min<uint64_t>((n_pix + 255) / 256, METER_BLOCKS);
    return d;
}

// ---- pt_render_aux, pt_denoise, pt_denoise_variance, the three reprojections and pt_frame_error: their argument rules in the
// header's order.  Device pointers are compared, never read.
// buffers: cam and the three guide buffers are given
inline Refusal check_aux_call(const CtxFacts& f, const pt_params* p, bool buffers) {
    if (!buffers || !p) return {PT_ERR_INVALID, "pt_render_aux: null argument"};
    if (p->width < 1 || p->height < 1) return {PT_ERR_INVALID, "pt_render_aux: width and height must be >= 1"};
    if (!f.has_bvh) return {PT_ERR_NO_SCENE, "pt_render_aux: no BVH uploaded"};
    if (f.records_woop) return {PT_ERR_UNSUPPORTED, "pt_render_aux: the binary walk reads Moller-Trumbore records (upload with PT_OPT_TRI_TEST 0)"};
    return {};
}
// pt_render_aux_camera; buffers: cam and the three guide buffers are given.  The image is cm's, checked whole as pt_render_pixels' is
inline Refusal check_aux_camera_call(const CtxFacts& f, const pt_camera_model* cm, const pt_params* p, bool buffers) {
    if (!buffers || !cm || !p) return {PT_ERR_INVALID, "pt_render_aux_camera: null argument"};
    const Refusal r = check_camera_model_image("pt_render_aux_camera", *cm);
    if (r.code != PT_OK) return r;
    if (!f.has_bvh) return {PT_ERR_NO_SCENE, "pt_render_aux_camera: no BVH uploaded"};
    if (f.records_woop) return {PT_ERR_UNSUPPORTED, "pt_render_aux_camera: the binary walk reads Moller-Trumbore records (upload with PT_OPT_TRI_TEST 0)"};
    return {};
}
// buffers: the colour, the three guide buffers and out are given
inline Refusal check_denoise_call(const pt_denoise_params* dp, bool buffers) {
    if (!dp || !buffers) return {PT_ERR_INVALID, "pt_denoise: null argument"};
    if (dp->width < 1 || dp->height < 1) return {PT_ERR_INVALID, "pt_denoise: width and height must be >= 1"};
    if (dp->iterations < 0 || dp->iterations > 10) return {PT_ERR_INVALID, "pt_denoise: iterations must be 0..10"};
    if (!plan_finite(dp->sigma_color) || !plan_finite(dp->sigma_normal) || !plan_finite(dp->sigma_position)) return {PT_ERR_INVALID, "pt_denoise: a sigma is not finite"};
    return {};
}
// the caller's buffers as it passed them (length, out_variance and the display words may be null)
struct VarianceBuffers { const void *color, *moments, *length, *albedo, *normal, *position, *out, *out_variance; };
inline Refusal check_denoise_variance_call(const pt_denoise_variance_params* dp, const VarianceBuffers& b) {
    if (!dp || !b.color || !b.albedo || !b.normal || !b.position || !b.out) return {PT_ERR_INVALID, "pt_denoise_variance: null argument"};
    if (dp->width < 1 || dp->height < 1) return {PT_ERR_INVALID, "pt_denoise_variance: width and height must be >= 1"};
    if (dp->iterations < 0 || dp->iterations > 10) return {PT_ERR_INVALID, "pt_denoise_variance: iterations must be 0..10"};
    if (!plan_finite(dp->sigma_luminance) || !plan_finite(dp->sigma_normal) || !plan_finite(dp->sigma_position))
        return {PT_ERR_INVALID, "pt_denoise_variance: a sigma is not finite"};
    if (!b.moments) return {PT_ERR_INVALID, "pt_denoise_variance: null moments"};
    if (!plan_finite(dp->samples_per_frame) || dp->samples_per_frame < 1.f) return {PT_ERR_INVALID, "pt_denoise_variance: samples_per_frame must be finite and >= 1"};
    const void* const inputs[] = {b.color, b.moments, b.length, b.albedo, b.normal, b.position};
    if (b.out_variance)
        for (const void* in : inputs)
            if (in == b.out_variance) return {PT_ERR_INVALID, "pt_denoise_variance: out_variance_dev may not be one of the inputs"};
    return {};
}
// What the caller of pt_temporal, pt_temporal_motion (rows, motion), pt_temporal_moments (rows; the buffers named *_color hold its
// moments, and it has no out_length, no rgba) or pt_temporal_camera (rows where given, motion, the previous camera's model) passed; a
// pointer the call does not have stays null
enum TemporalKind { TEMPORAL_COLOUR, TEMPORAL_MOTION, TEMPORAL_MOMENTS, TEMPORAL_CAMERA };
struct TemporalCall {
    TemporalKind kind;
    const pt_temporal_params* tp;
    const pt_camera* prev_cam;
    const float *prev_color, *prev_length, *prev_normal, *prev_position;
    const int32_t* prev_id;
    const float *cur_color, *cur_normal, *cur_position;
    const int32_t* cur_id;
    float *out_color, *out_length;
    uint32_t* rgba;
    const float *prev_verts, *cur_verts;   // the vertex rows by triangle id
    size_t n_tris;
    float* motion;
    const pt_camera_model* prev_cm;        // pt_temporal_camera
};
// a history: prev_color is given.  rows: the call finds moved triangles' points in the vertex rows (pt_temporal_motion always,
// pt_temporal_moments and pt_temporal_camera where a row buffer is given)
inline bool temporal_reads_rows(const TemporalCall& a) {
    return a.kind == TEMPORAL_MOTION || ((a.kind == TEMPORAL_MOMENTS || a.kind == TEMPORAL_CAMERA) && (a.prev_verts || a.cur_verts));
}
inline Refusal check_temporal_call(const std::string& who, const TemporalCall& a) {
    const bool with_length = a.kind != TEMPORAL_MOMENTS;
    const pt_temporal_params* tp = a.tp;
    if (!tp || !a.cur_color || !a.cur_normal || !a.cur_position || !a.out_color || (with_length && !a.out_length)) return {PT_ERR_INVALID, who + ": null argument"};
    if (tp->width < 2 || tp->height < 2) return {PT_ERR_INVALID, who + ": width and height must be >= 2"};
    if (!plan_finite(tp->max_history) || tp->max_history < 1.f) return {PT_ERR_INVALID, who + ": max_history must be finite and >= 1"};
    if (!plan_finite(tp->plane_tolerance) || tp->plane_tolerance < 0.f) return {PT_ERR_INVALID, who + ": plane_tolerance must be finite and >= 0"};
    if (!(tp->normal_threshold >= -1.f && tp->normal_threshold <= 1.f)) return {PT_ERR_INVALID, who + ": normal_threshold must be in -1..1"};
    if (!a.prev_color) return {};
    if (!a.prev_cam || !a.prev_length || !a.prev_normal || !a.prev_position) return {PT_ERR_INVALID, who + ": a history needs its camera, lengths, normals and positions"};
    if (a.kind == TEMPORAL_CAMERA) {   // the model the history was rendered under: its own rules, and the image of the parameters
        if (!a.prev_cm) return {PT_ERR_INVALID, who + ": a history needs the model of its camera"};
        const pt_camera_model* prev_cm = a.prev_cm;   // (host memory, as tp)
        const pt_camera_model& cm = *prev_cm;
        const Refusal r = check_camera_model_image(who, cm);
        if (r.code != PT_OK) return r;
        if (cm.width != tp->width || cm.height != tp->height) return {PT_ERR_INVALID, who + ": the model's image must be the parameters' (prev_cm->width, height)"};
    }
    if ((a.prev_id == nullptr) != (a.cur_id == nullptr)) return {PT_ERR_INVALID, who + ": ids of both frames or of neither"};
    if (a.out_color == a.prev_color || (with_length && a.out_length == a.prev_length))
        return {PT_ERR_INVALID, who + ": the new history may not overwrite the old one (ping-pong the buffers)"};
    if (temporal_reads_rows(a)) {
        if (!a.prev_id || !a.cur_id) return {PT_ERR_INVALID, who + ": the ids of both frames are required (they choose the vertex rows)"};
        if (a.n_tris > 0 && (!a.prev_verts || !a.cur_verts)) return {PT_ERR_INVALID, who + ": a null vertex buffer with n_tris > 0"};
        if (a.n_tris >= ((size_t)1 << 31)) return {PT_ERR_INVALID, who + ": n_tris must be < 2^31 (ids are int32)"};
    }
    const void* const others[] = {a.prev_verts, a.cur_verts, a.prev_color, a.prev_length, a.prev_normal, a.prev_position, a.prev_id,
                                  a.cur_color, a.cur_normal, a.cur_position, a.cur_id, a.out_color, a.out_length, a.rgba};
    if (a.motion)
        for (const void* o : others)
            if (o == (const void*)a.motion) return {PT_ERR_INVALID, who + ": motion_dev may not be one of the other buffers"};
    return {};
}
// buffers: the moments and one of mean_rse, n_above are given; n_pix: width * height of a call that passes
inline Refusal check_frame_error_call(bool buffers, int32_t width, int32_t height, uint64_t n_samples, float threshold, uint64_t& n_pix) {
    n_pix = 0;
    if (!buffers) return {PT_ERR_INVALID, "pt_frame_error: null argument"};
    if (width < 1 || height < 1) return {PT_ERR_INVALID, "pt_frame_error: width and height must be >= 1"};
    if (n_samples < 2) return {PT_ERR_INVALID, "pt_frame_error: the standard error needs n_samples >= 2"};
    if (!plan_finite(threshold) || threshold < 0.f) return {PT_ERR_INVALID, "pt_frame_error: threshold must be finite and >= 0"};
    n_pix = (uint64_t)width * (uint64_t)height;
    if (n_pix > 0xffffffffull) return {PT_ERR_INVALID, "pt_frame_error: more than 2^32 - 1 pixels"};
    return {};
}

// ---- pt_closest_hits / pt_any_hits: the wide walk on a resident grid over regions of PT_REGION rays at one of the extend stage's two
// budgets ((8 waves per SIMD, 16 stack entries in LDS), or (6, 24) under PT_OPT_LDS_STACK 24), or pt_trace_rays' binary launch with the
// bound applied to its answer when the tree is too deep for the wide one
struct QueryPlan {
    bool wide;
    uint32_t word, n_regions;   // query_word (wide)
    int batch, blocks_per_cu, n_cu;
    int n_top;                  // binary: the LDS mirror
    size_t lds;
};
inline QueryPlan plan_query(const CtxFacts& f, uint64_t n, bool any) {
    QueryPlan q = {};
    q.wide = wide_walk_fits(f, PT_STACK_CAP);
    q.word = query_word(any, f.lstk == 24);
    q.n_regions = (uint32_t)((n + PT_REGION - 1) / PT_REGION);
    q.batch = f.wave_batch; q.blocks_per_cu = f.wave_blocks; q.n_cu = f.n_cu;
    q.lds = q.wide ? (size_t)budget_lstk(qv_budget(q.word)) * PT_BLOCK * 4 : binary_ray_lds(f, q.n_top);
    return q;
}

}  // namespace ptmi
