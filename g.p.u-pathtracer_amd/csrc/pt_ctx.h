// pt_ctx.h — the context behind the C ABI (include/ptmi.h) and the host-side helpers shared by the
// translation units of libptmi.so: ptmi.hip (API), pt_tree.hip (trees: makers, adoption, cost), pt_build.hip (device BVH
// builder), pt_refit.hip (refit), pt_aux.hip, pt_filter.hip, pt_temporal.hip, pt_select.hip, pt_display.hip (the image stages: guide buffers, a-trous filters, reprojection, frame error and pixel selection, display; pt_image.h is what they share), pt_k_*.hip (kernel families +
// their launchers, no API function), pt_env.hip (environment map), pt_camera.hip (camera models).  Host code only.
// Every device buffer, event and stream of the context is a member that owns it (pt_own.h): pt_destroy waits and deletes.  The scene's
// resources — tree, spheres, materials, environment — are values: built in a local, adopted behind quiesce().
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/ptmi.h"
#include "pt_kernels.h"
#include "pt_own.h"
#include "pt_plan.h"

// the bounce-0 walk of a new context (PT_OPT_FIRST_WALK); -DPT_FIRST_WALK_DEFAULT=0 builds the per-lane one for A/B timing
#ifndef PT_FIRST_WALK_DEFAULT
#define PT_FIRST_WALK_DEFAULT 1
#endif
// most triangles a tree's occluder list holds (PT_OPT_LAST_OCCLUDERS; the sweep of profiles/r18_last_occluders.txt chose it)
#ifndef PT_OCCLUDERS_MAX
#define PT_OCCLUDERS_MAX 12
#endif
// ... and the share of the mesh's triangle area one of them has at least, as 1 / N: the walls of a room hold 6-8 % each and decide
// most occluded last segments; the two ground triangles of gto_sixteen hold 3.1 % each and a list of them decides too few to pay
#define PT_OCCLUDER_AREA_DIV 24

// Everything that describes an acceleration structure.  A tree is a VALUE: the makers (pt_tree.hip, pt_build.hip) fill one inside a
// DevTree without touching the context, and adopt_tree (pt_tree.hip) is the only code that writes pt_ctx::tree.  So
//   * a call that fails before adoption leaves the context exactly as it was: tree, build_ms, scene_gen, refit state;
//   * the previous tree lives until the new one is complete: one more tree at the peak of a plain upload, two more for a moment
//     under PT_OPT_REBUILD 2 (3 n items of 64 B: ~150 MB at 800 k triangles);
//   * scene_gen advances by one per successful call (only equality is ever tested on it).
struct TreeState {
    float4* d_nodes = nullptr;   // one item buffer, [binary nodes][records][wide nodes]: links index it directly (KScene::nodes and ::tris); a view of DevTree::items
    bool records_woop = false;   // what the uploaded records are
    bool has_bvh = false;
    uint64_t wide_root = 0;      // float4 index of the 4-wide tree's root, 0 = not built
    uint64_t n_wide = 0, n_inner = 0, n_refs = 0, n_leaves = 0, scene_bytes = 0;
    uint32_t wide_top_layout = 0, wide_depth = 0;
    uint32_t n_top_layout = 0;   // nodes [0, n_top_layout) are in breadth-first order
    uint32_t max_depth = 0;
    int32_t max_tri_id = -1;     // largest original triangle id of the uploaded BVH
    float build_ms = -1.f;       // device time of the build behind this tree, -1: no device build stands behind it
    double opt_cost[2] = {0.0, 0.0};   // PT_OPT_OPTIMIZE: area cost (inner-node areas / root area) before / after, 0 when it did not run
    // PT_OPT_LAST_OCCLUDERS: the ids of the mesh's largest triangles, largest first (select_occluders), chosen where the tree is adopted;
    // the context's table (pt_ctx::d_occ) holds their records as THIS tree's item buffer has them
    int32_t occ_ids[PT_OCCLUDERS_MAX] = {};
    uint32_t n_occ = 0;
};

// A tree with the item buffer it describes: whatever a maker allocated is released on every early return, the loser of
// PT_OPT_REBUILD 2 when it goes out of scope, the context's tree when another is adopted over it.  A moved-from tree is "no tree".
struct DevTree : TreeState {
    ptmi::DevBuf<float4> items;
    DevTree() = default;
    DevTree(DevTree&& o) noexcept : TreeState(o), items(std::move(o.items)) { static_cast<TreeState&>(o) = TreeState(); }
    DevTree& operator=(DevTree&& o) noexcept {
        if (this != &o) {
            TreeState::operator=(o);
            items = std::move(o.items);
            static_cast<TreeState&>(o) = TreeState();
        }
        return *this;
    }
    hipError_t alloc_items(size_t n_float4) {
        const hipError_t e = items.alloc(n_float4);
        d_nodes = items.get();
        return e;
    }
};

// pt_upload_tri_materials' table and the light list it implies, a value like a tree: filled in a local, move-assigned onto the context
// once every allocation and copy has succeeded (the only place mat_gen advances).  Empty: the one global material of pt_params.
struct Materials {
    ptmi::DevBuf<int32_t> d_tri_matid;   // material row of every triangle id
    ptmi::DevBuf<float4> d_mat_table;    // two rows per pt_material
    size_t n_tri_matid = 0;
    // PT_FLAG_NEE over emissive triangles: ids whose material row emits (host, ascending), id -> light slot (device),
    // the light records (device; rebuilt from the triangle records when the scene or the materials changed)
    std::vector<int32_t> emissive_ids;
    ptmi::DevBuf<int32_t> d_light_slot;
    ptmi::DevBuf<float4> d_tri_lights;
};

// pt_upload_environment's map (pt_env.hip), a value too: the context's own device copy of the texels, the sampling tables
// (PT_OPT_ENV_LIGHT; empty: the map is no light) and the map as the kernels get it, computed from them: k.texels == nullptr: no map,
// k.cx == nullptr: no light.
struct EnvMap {
    ptmi::DevBuf<float4> d_texels;
    ptmi::DevBuf<float> d_tables;   // cx, cy, zs
    KEnv k = {};
    int code() const { return env_code(k.texels != nullptr, k.cx != nullptr); }   // LaunchCfg::env
};

struct pt_ctx {
    using Event = ptmi::Event;
    using Stream = ptmi::Stream;
    template <class T> using DevBuf = ptmi::DevBuf<T>;
    int device = 0;
    // the streams first: members go in reverse order, so whatever ran on a stream is released before the stream (pt_destroy has waited
    // for all of them by then)
    Stream own_stream;
    hipStream_t stream = nullptr;      // the caller's (pt_set_stream) or own_stream: borrowed
    // Overlap of consecutive calls (PT_OPT_OVERLAP, persistent / mega kernels): the path kernel of call k + 1 runs on
    // a side stream into its own sample buffer while call k's last paths drain; only the folds (which touch the
    // accumulator, in order) stay on the caller's stream.  side[x]: stream, sample buffer, queue counters of slot x.
    int opt_overlap = 1;
    struct Side {
        Stream stream;
        Event traced, folded;   // path kernel done / the fold that read the buffer done
        bool fold_pending = false;
        DevBuf<float> samples;
        DevBuf<unsigned int> queue;
        uint64_t lights_seen = 0;   // the light list generation this stream has been ordered behind (lights_gen)
        uint64_t geom_seen = 0;     // the refit generation this stream has been ordered behind (geom_gen)
    } side[2];
    int side_next = 0;
    Event switch_ev;                   // pt_set_stream: the new stream waits for what the old one was given (recorded there at the switch)
    std::string err;
    // scene
    DevTree tree;                      // written by adopt_tree (pt_tree.hip) only
    DevBuf<pt_sphere_d> d_spheres;
    Materials mat;                     // pt_upload_tri_materials
    uint64_t mat_gen = 0, lights_key = ~0ull;
    uint64_t lights_geom = 0;          // the refit generation (geom_gen) the light list was collected at
    // the light list is (re)written on the caller's stream; a side stream (PT_OPT_OVERLAP) waits for lights_ev before its
    // first kernel that may read that generation of the list
    Event lights_ev;
    uint64_t lights_gen = 0;
    int n_spheres = 0;
    pt_sphere_d h_spheres[PT_KSPHERES];   // host copy of the first spheres for the kernel-argument block
    // pt_upload_environment (pt_env.hip); env_gen counts the uploads and clears, part of PT_KERNEL_AUTO's key like scene_gen
    EnvMap env;
    uint64_t env_gen = 0;
    // options
    int opt_kernel = PT_KERNEL_AUTO;
    int opt_counters = 0;
    int opt_timing = 0;
    // measurement
    DevBuf<unsigned long long> d_counters;
    DevBuf<unsigned int> d_queue;      // work counters of the persistent kernel, of the ray-batch queries (pt_k_query.hip) and of pt_render_rays (pt_k_rays.hip), on the caller's stream: reset there before every launch
    DevBuf<float> d_samples;           // [spp][H*W][3] sample colours of a multi-sample call; pt_render_rays: [spp][n][3] (both on the caller's stream); grow-only
    int n_cu = 0;
    int opt_batch = 36;
    int opt_presplit = 0;        // pt_build_bvh: 0 off, else the target length in per cent of diag/sqrt(n) (PT_OPT_PRESPLIT)
    int opt_optimize = 0;        // pt_upload_bvh: passes of insertion-based optimisation over the uploaded hierarchy (PT_OPT_OPTIMIZE)
    int opt_rebuild = 0;         // pt_upload_bvh: 1 = re-cluster the uploaded triangles on the device (PT_OPT_REBUILD)
    int opt_build_algo = 1;      // pt_build_bvh: 0 LBVH (Karras), 1 PLOC (PT_OPT_BUILD_ALGO)
    int opt_sph_lds = 1;         // persistent kernel: sphere attributes from an LDS copy (PT_OPT_SPHERE_LDS)
    int opt_vote_node = 1, opt_vote_rec = 1;
    int opt_refill = 8;          // idle lanes that trigger a refill (PT_OPT_REFILL)
    int opt_top = 64;            // nodes mirrored in LDS (PT_OPT_TOP_NODES)
    int opt_occ = 6;             // waves per SIMD the kernel is compiled for (PT_OPT_OCCUPANCY)
    int opt_lstk = 16;           // LDS stack entries per lane (deeper entries overflow to scratch)
    int opt_walk = 2;            // 0 while-while, 1 unified-step, 2 wide, 4 wide + postponed leaf (PT_OPT_WALK)
    int opt_leaf_max = 2;        // leaves with more references are split at upload (PT_OPT_LEAF_MAX)
    int opt_tri_test = 0;        // 0 Moller-Trumbore records, 1 Woop records (next upload; PT_OPT_TRI_TEST)
    // stage-split (wavefront) pipeline: path records of one call, two generations (pt_k_wave.hip)
    DevBuf<char> d_wave;         // grow-only; dropped again once PT_KERNEL_AUTO has decided against the pipeline everywhere (auto_decide)
    int opt_wave_batch = 16;     // extend kernel: finished lanes that make a wave leave the walk to write hits / refill
    int opt_wave_samples = 16;   // bounce 0 of the stage-split pipeline: samples of one pixel per wave (PT_OPT_WAVE_SAMPLES)
    int opt_wave_blocks = 8;     // extend kernel: resident 256-thread blocks per CU the grid is sized for (PT_OPT_WAVE_BLOCKS)
    int opt_first_walk = PT_FIRST_WALK_DEFAULT;   // extend kernel of bounce 0: 0 per-lane walk, 1 wave-wide packets (PT_OPT_FIRST_WALK)
    int opt_packet_stack = PT_PACKET_STACK_MAX;   // (link, mask) entries the packet walk may use per wave (PT_OPT_PACKET_STACK)
    int opt_fuse_stages = 1;     // bounce 0's shade in the packet walk's launch, the fold in the last shade launch (PT_OPT_FUSE_STAGES)
    int opt_last_anyhit = 1;     // the last segment as a sphere-bounded any-hit query: 0 off, 1 product launches, 2 instrumented too (PT_OPT_LAST_ANYHIT)
    int opt_root_cull = 1;       // new rays the root node step turns away stay out of the extend queue: 0 off, 1 product launches, 2 instrumented too (PT_OPT_ROOT_CULL)
    int opt_root_entry = 1;      // ... and the walkers' records carry the root step's result, the extend launches start below the root: 0 off, 1 product launches, 2 instrumented too (PT_OPT_ROOT_ENTRY)
    int opt_env_light = 0;       // the next pt_upload_environment builds the map's sampling tables: under PT_FLAG_NEE it is a light (PT_OPT_ENV_LIGHT)
    int opt_last_occluders = 1;  // last-segment walkers that one of the tree's largest triangles occludes stay out of the any-hit queue: 0 off, 1 product launches, 2 instrumented too (PT_OPT_LAST_OCCLUDERS)
    int opt_path_history = 1;    // the records carry the objects a path has hit instead of its mask, its sample colour is written once: 0 off, 1 product launches, 2 instrumented too (PT_OPT_PATH_HISTORY)
    // PT_KERNEL_AUTO: which stage layout is faster depends on the workload (long paths and many samples per call:
    // the stage-split pipeline; short paths or few samples: the persistent kernel), so the first FOUR calls of a
    // configuration are timed trials, two per layout, alternating (HIP events on the stream, buffers allocated before the
    // timed span; the faster trial of each layout counts) and the following ones run the faster layout.  A small table of configurations (least recently used replaced): a context that cycles through
    // a few configurations — the partitions of a tile split, two image sizes — keeps every decision.
    struct AutoPick {
        static constexpr int TRIALS = 4, PENDING = 4, DECIDED = 5;
        uint64_t key = 0;        // what the choice was made for: image, spp, depth, partition shape, scene generation, material, flags
        int phase = 0;           // 0..3: this call is timed trial `phase` (even: persistent kernel, odd: pipeline)  4: events pending  5: decided
        int choice = PT_KERNEL_PERSISTENT;
        Event e[2 * TRIALS];     // start / end of every trial
        float ms[2] = {0.f, 0.f};   // the faster of each layout's two trials (a context's very first launch is slow: code upload)
        uint64_t used = 0;       // tick of the last pt_render that looked this entry up
    };
    static constexpr int N_PICKS = 8;
    AutoPick picks[N_PICKS];
    int pick_last = -1;          // entry of the last PT_KERNEL_AUTO call (pt_auto_choice), -1 = none
    uint64_t pick_tick = 0;
    uint64_t scene_gen = 0;      // bumped once by every adopted tree (adopt_tree)
    // pt_refit_bvh: the boxes and records of the tree are rewritten on the caller's stream; geom_gen counts the refits and a side
    // stream (PT_OPT_OVERLAP) waits for geom_ev before its first path kernel after one (the light list is re-collected too)
    uint64_t geom_gen = 0;
    Event geom_ev;
    // PT_OPT_LAST_OCCLUDERS: the first three pieces of the records of tree.occ_ids, copied out of the tree's item buffer on the caller's
    // stream by whoever writes those records: adopt_tree and pt_refit_bvh (occluders_collect).  3 float4 each, the last one's `last` set.
    DevBuf<float4> d_occ;
    // what the refit of one tree needs on the device, made by its first refit (pt_refit.hip) and dropped (= Refit()) where the tree is replaced
    struct Refit {
        uint64_t scene_gen = 0;
        const float4* items = nullptr;           // the tree it was made for: (scene_gen, item buffer)
        DevBuf<char> d_mem;                      // one allocation: the lists and scratch below
        int4* bin_list = nullptr;                // binary nodes by height: {node, records of leaf child 0 (0: inner), of child 1, 0}
        int4* wide_list = nullptr;               // wide nodes by height: {slot, children, records of 0 | 1 << 16, of 2 | 3 << 16}
        float* bin_box = nullptr;                // [n_inner][6] exact union of a binary node's triangles (lo > hi: all dropped)
        float* wide_box = nullptr;               // [n_wide][6] the same per wide node
        float* rec_box = nullptr;                // [n_refs][6] triangle box of every record
        uint32_t* first_use = nullptr;           // bit per record: the first record of its triangle (counts a dropped triangle once)
        std::vector<uint32_t> bin_off, wide_off; // list offsets per height (size heights + 1)
    } refit;
    // pt_denoise's two ping-pong colour frames (pt_filter.hip; pt_denoise_variance uses them too): grow-only
    DevBuf<float4> d_denoise;
    // pt_frame_error's per-block partial results (pt_select.hip): [blocks] double sums, then [blocks] uint32 counts; grow-only
    DevBuf<char> d_frame_err;
    // pt_select_pixels' per-block scratch (pt_select.hip): [blocks] double sums, [blocks] uint32 counts, [blocks] uint32 list offsets; grow-only
    DevBuf<char> d_select;
    // pt_meter's partial histograms (pt_display.hip): [METER_BLOCKS][METER_BINS + 1] uint32, reserved whole by the first call
    DevBuf<uint32_t> d_meter;
    // pt_tonemap's threshold tables (pt_display.hip): [2][256] floats, PT_XFER_SRGB then PT_XFER_GAMMA22, uploaded by the first call that needs one
    DevBuf<float> d_tone;
    Event ev0, ev1;
    bool timed = false;
    // PT_OPT_TIMING: events between the stages of the last call (pt_get_stage_ms); stage_kind[i] is the
    // PT_STAGE_* of the work between event i and event i + 1
    std::vector<Event> stage_ev;
    std::vector<int> stage_kind;
    size_t stage_used = 0;
};

namespace ptmi {

extern thread_local std::string g_err;

inline int fail(pt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    g_err = msg;
    return code;
}
inline int fail(pt_ctx* c, const Refusal& r) { return r.code == PT_OK ? PT_OK : fail(c, r.code, r.msg); }   // (nothing to do: PT_OK, the last error stays)
inline int hip_fail(pt_ctx* c, hipError_t e, const char* what) {
    return fail(c, PT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Every stream a launch that reads the scene can still be running on: the caller's, the context's own, both side streams
// (PT_OPT_OVERLAP).  What replaces a scene resource — adopt_tree, pt_upload_spheres, pt_upload_tri_materials, pt_upload_environment —
// and pt_destroy wait here first; the owners themselves never wait.
inline hipError_t quiesce(pt_ctx* c) {
    hipError_t e = c->stream ? hipStreamSynchronize(c->stream) : hipSuccess;
    if (e == hipSuccess && c->own_stream && c->own_stream != c->stream) e = hipStreamSynchronize(c->own_stream);
    for (pt_ctx::Side& s : c->side)
        if (e == hipSuccess && s.stream) e = hipStreamSynchronize(s.stream);
    return e;
}

template <typename K>
hipError_t allow_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// ---- the rules every entry point shares are pt_plan.h's; here is what applies their answers to the context and the kernel arguments
// What planning reads off the context (ptmi.hip): the one place that reads the tree's fields and the options for a plan
CtxFacts ctx_facts(const pt_ctx* c);
// The scene as a kernel sees it: one item buffer for nodes and records, the wide tree's root and, where ksph (KParams::ksph) is
// given, the spheres: a ray-batch query sees none.  Zeroes the rest; the stack and LDS layout is the caller's.
inline void scene_view(const pt_ctx* c, KScene& sc, pt_sphere_d* ksph = nullptr) {
    sc = KScene();
    sc.nodes = sc.tris = c->tree.d_nodes;
    sc.has_bvh = c->tree.has_bvh ? 1 : 0;
    sc.wide_root = (int)c->tree.wide_root;
    if (!ksph) return;
    sc.spheres = c->d_spheres.get(); sc.n_spheres = c->n_spheres;
    std::memcpy(ksph, c->h_spheres, sizeof c->h_spheres);
}
// The binary walk with one thread per ray (binary_ray_lds, pt_plan.h) in a kernel's scene view.  Returns the LDS bytes of a block.
inline size_t binary_ray_layout(const CtxFacts& f, KScene& sc) {
    sc.stack_n = PT_STACK_CAP; sc.top_base = 0;
    return binary_ray_lds(f, sc.n_top);
}
// The work counters of a persistent launch: PT_SHARDS of them, a cache line apart, zero when the launch starts.
constexpr size_t QUEUE_WORDS = PT_SHARDS * PT_SHARD_STRIDE, QUEUE_BYTES = QUEUE_WORDS * sizeof(unsigned int);
inline hipError_t queue_reset(unsigned int* q, hipStream_t st) { return hipMemsetAsync(q, 0, QUEUE_BYTES, st); }
inline void queue_params(const QueueKnobs& q, unsigned int* queue, KParams& P) {
    P.queue = queue; P.batch = q.batch; P.refill = q.refill;
    P.vote_node = q.vote_node; P.vote_rec = q.vote_rec;
}
// PT_OPT_TIMING: the span pt_last_kernel_ms reads, around a call's launches on the caller's stream (HIP_TRY(c, span_begin(c)) ...);
// the context counts as timed only once the end event is recorded
inline hipError_t span_begin(pt_ctx* c) { return c->opt_timing ? hipEventRecord(c->ev0, c->stream) : hipSuccess; }
inline hipError_t span_end(pt_ctx* c) {
    const hipError_t e = c->opt_timing ? hipEventRecord(c->ev1, c->stream) : hipSuccess;
    if (c->opt_timing && e == hipSuccess) c->timed = true;
    return e;
}

// ---- compile-time dispatch: generic lambdas take template arguments as std::integral_constant values; only the combinations a
// lambda is CALLED with are instantiated
template <int V> constexpr std::integral_constant<int, V> int_c{};
template <class F>   // f(true_type) or f(false_type), by v
auto with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// One kernel family's dispatch (pt_variants.h): f(integral_constant<uint32_t, V>) for the word V of N_BITS bits that equals v — instantiated
// for the words with EXISTS(V) and no other — or hipErrorInvalidValue when v is none of them: no request runs another request's kernel.
// (a binary search over the words [LO, LO + N) at compile time: v lies among them)
template <bool (*EXISTS)(uint32_t), uint32_t LO, uint32_t N, class F>
hipError_t with_variant_in(uint32_t v, F& f) {
    if constexpr (N > 1) return v < LO + N / 2 ? with_variant_in<EXISTS, LO, N / 2>(v, f) : with_variant_in<EXISTS, LO + N / 2, N / 2>(v, f);
    else if constexpr (EXISTS(LO)) return f(std::integral_constant<uint32_t, LO>{});
    else return hipErrorInvalidValue;
}
template <bool (*EXISTS)(uint32_t), int N_BITS, class F>
hipError_t with_variant(uint32_t v, F&& f) { return v < (1u << N_BITS) ? with_variant_in<EXISTS, 0u, (1u << N_BITS)>(v, f) : hipErrorInvalidValue; }

// A grid of resident blocks for a kernel whose waves draw work from a queue: what the device holds at once (at most `max_per_cu` per
// CU), never more than `work_cap`.  No grid-wide wait anywhere: an over-estimate only means a few late blocks find the queue empty.
template <class K, class... A>
hipError_t launch_resident(K kernel, size_t lds, int max_per_cu, int n_cu, size_t work_cap, hipStream_t st, const A&... args) {
    int per_cu = 0;
    const hipError_t e = allow_lds(kernel, lds);
    if (e != hipSuccess) return e;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PT_BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    per_cu = std::min(per_cu, max_per_cu);
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<size_t>((size_t)per_cu * n_cu, work_cap)), dim3(PT_BLOCK), lds, st, args...);
    return hipGetLastError();
}

// ---- launchers of the kernel families (one translation unit each) -------------------------------
hipError_t launch_mega(const LaunchCfg& L, const KParams& P, hipStream_t st);        // pt_k_mega.hip
hipError_t launch_rays(const KScene& sc, size_t lds, const float4* rays, size_t n, int cull, float* t_out, int* tri_out,
                       float* n_out, hipStream_t st);                                 // pt_k_mega.hip
hipError_t launch_persist(const LaunchCfg& L, const KParams& P, hipStream_t st);     // pt_k_persist.hip
hipError_t launch_fold(const KParams& P, float2* moments, hipStream_t st);           // pt_k_persist.hip; moments: nullptr = none
// stage-split pipeline (pt_k_wave.hip): generate -> depth x (extend, shade), as plan.wave and plan.wl say; returns PT_* status.  The
// samples are already folded into the accumulator when plan.wave.fold_lp != 0 (PT_OPT_FUSE_STAGES): no launch_fold after it
int render_wavefront(pt_ctx* c, KParams& P, const CallPlan& plan);
int wave_reserve(pt_ctx* c, const WaveLayout& w);   // makes sure the context holds the path records of layout w (a PT_KERNEL_AUTO trial: ahead of its timed span)
// ray-batch queries over the tree on the context (pt_k_query.hip): pt_closest_hits (hit = nullptr) and pt_any_hits (hit given; t, tri and
// normal unused).  Resets the work counters on the stream, then one launch: the wide walk on a resident grid, or the binary walk with
// the bound applied to its answer when the tree is too deep for the wide one
struct QueryCall {
    const float* rays;   // float[n][8] = (o, ignored, d, t_max)
    size_t n;            // 0 < n < 2^32
    int cull;
    float* t;
    int32_t* tri;
    float* normal;       // may be nullptr
    uint8_t* hit;
};
hipError_t launch_query(pt_ctx* c, const QueryPlan& plan, const QueryCall& q);
// the path loop over a caller's rays (pt_k_rays.hip), one launch of pt_render_rays: the persistent grid over the (sample, ray) slots
// that P and the batch describe, on the context's stream, and the fold of a launch's sample buffer into the running means
struct RaysCall {
    const float* rays;      // float[n][8] = (o, ignored, d, ignored)
    float* out;             // float[n][3]
    uint64_t first_index;   // RNG key of ray 0
    size_t n;               // 0 < n < 2^32
    int hdr;                // mode == PT_RAYS_HDR
};
hipError_t launch_render_rays(const LaunchCfg& L, const KParams& P, const RaysCall& r, hipStream_t st);
hipError_t launch_fold_rays(const pt_ctx* c, const KParams& P, const RaysCall& r);
// the same loop over the pixels of a camera model (pt_k_camera.hip), one launch of pt_render_camera; P.cam is the camera.  Its fold
// is launch_fold_rays over RaysCall{nullptr, out, 0, n, hdr}
struct CameraCall {
    const pt_camera_model* cm;   // checked: check_camera_model (pt_plan.h)
    const uint32_t* pixels;      // n pixel numbers on the device, or nullptr
    uint64_t first_pixel;        // without a list: row i is pixel first_pixel + i
    float* out;                  // float[n][3]
    size_t n;                    // 0 < n < 2^32
    int hdr;                     // mode == PT_RAYS_HDR
};
hipError_t launch_render_camera(const LaunchCfg& L, const KParams& P, const CameraCall& r, hipStream_t st);
// pt_render_pixels' fold (pt_k_rays.hip): the launch's sample buffer [P.spp][n][3] scattered into full-frame buffers, every listed
// pixel from its own sample count on
struct PixelsCall {
    const uint32_t* pixels;   // n pixel numbers on the device, or nullptr: row i is pixel i
    float* accum;             // float[n_pix][3]
    float* moments;           // float[n_pix][2], or nullptr
    uint32_t* counts;         // uint32[n_pix]
    size_t n;                 // 0 < n < 2^32
    uint32_t n_pix;           // width * height: a listed index from here on is skipped
    int hdr;                  // mode == PT_RAYS_HDR
};
hipError_t launch_fold_pixels(const pt_ctx* c, const KParams& P, const PixelsCall& r);
// PT_OPT_TIMING: marks the end of a stage of the running call on the context's stream (no-op when timing is off)
int stage_mark(pt_ctx* c, int kind_of_work_since_last_mark);
// device BVH builder (pt_build.hip), a maker: the tree over the mesh into `out` (its build_ms set), the context's own tree untouched.
// PT_OPT_BUILD_ALGO 1 falls back to the LBVH inside when PLOC's tree gets too deep.  id_map: the id triangle t reports (default t)
int build_bvh_impl(pt_ctx* c, const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris, DevTree& out,
                   const int32_t* id_map = nullptr);
// PT_OPT_LAST_OCCLUDERS (pt_tree.hip).  select_occluders: the rule — of the triangles (id, nine vertex floats; a triangle may be listed
// more than once, each time in full) those whose area is at least 1/24 (PT_OCCLUDER_AREA_DIV) of the mesh's, largest first, ties to the smaller id, at most
// `cap`; returns how many ids it wrote.  occluders_collect: copies the records of c->tree.occ_ids into c->d_occ on the context's stream.
struct OccTri { int32_t id; const float *v0, *v1, *v2; };
int select_occluders(std::vector<OccTri>& tris, int32_t* ids, int cap);
int occluders_collect(pt_ctx* c);

}  // namespace ptmi

#define HIP_TRY(ctx, call)                                                \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return ptmi::hip_fail((ctx), e_, #call);    \
    } while (0)
