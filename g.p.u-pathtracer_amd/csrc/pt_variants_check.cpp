// pt_variants_check.cpp — every request has a kernel and every kernel a request, and every plan is sound: a CPU program with its own
// main, no HIP library (`make variants_check`, SAN=1 for the address and undefined-behaviour sanitizers; tests/test_variants.py runs both).
// It RUNS the planner (pt_plan.h: the functions pt_render, pt_render_rays, pt_render_camera, pt_render_pixels, pt_select_pixels, pt_tonemap, pt_meter, the older image-stage calls and the ray-batch queries call) over a domain of scenes x
// options x calls x the runtime's answers, and holds no rule of its own: a call is skipped because the planner refused it, and the
// refusal's code has to be the one REFUSALS lists for its text.  Of every plan it asserts what follows from the project's constants
// (LDS, refill <= batch, grids, the record layout); of every variant word a plan asks a launcher for, that the word is instantiated —
// with_variant (pt_ctx.h) would answer hipErrorInvalidValue for any other — and, the other way round, that every instantiated word
// came out of some plan.
#include <cstdio>
#include <initializer_list>
#include <set>
#include <vector>

#include "pt_plan.h"
using namespace ptmi;

static int n_failed = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (n_failed++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                       \
    } while (0)

struct Family {
    const char* name;
    bool (*exists)(uint32_t);
    int n_bits;
    long requests = 0;
    std::vector<char> seen = std::vector<char>(1u << n_bits, 0);   // by word
    void request(uint32_t v) {
        requests++;
        if (v >= seen.size() || !exists(v)) {
            if (n_failed++ < 20) std::printf("FAILED %s: a request asks for word 0x%x, which is not instantiated\n", name, v);
        } else seen[v] = 1;
    }
    int words() const {
        int n = 0;
        for (uint32_t v = 0; v < seen.size(); v++) {
            n += seen[v];
            if (exists(v) && !seen[v] && n_failed++ < 20) std::printf("FAILED %s: no request runs the instantiated word 0x%x\n", name, v);
        }
        return n;
    }
    void report() const { std::printf("%-26s %9ld requests, %3d distinct words, %3d kernels\n", name, requests, words(), variant_count(exists, n_bits)); }
};
static Family mega{"k_trace_mega_bvh2", mega_exists, PV_BITS}, persist{"k_trace_persist_bvh2", persist_exists, PV_BITS},
    rays{"k_render_rays", rays_exists, PV_BITS}, query{"k_query_rays", query_exists, QV_BITS}, extend{"k_wf_extend", extend_exists, WX_BITS},
    shade{"k_wf_shade", shade_exists, WS_BITS}, last_any{"k_wf_shade_last_any", shade_last_any_exists, WS_BITS},
    fused{"k_wf_extend_packet_shade", fused_exists, WS_BITS},
    camera{"k_render_camera", camera_exists, PV_BITS};   // the camera start of k_render_rays' loop: reported in a line of its own wording

// the refusals the planner knows, by a piece of their text, with the code each one answers; every one of them is met below
static struct { const char* text; int code; long seen; } REFUSALS[] = {
    {": no scene uploaded", PT_ERR_NO_SCENE, 0}, {": null argument", PT_ERR_INVALID, 0}, {"image must be at least 2x2", PT_ERR_INVALID, 0},
    {"spp must be >= 1", PT_ERR_INVALID, 0}, {"mode must be PT_RAYS_CLAMPED or PT_RAYS_HDR", PT_ERR_INVALID, 0}, {"more than 2^32 - 1 rays", PT_ERR_INVALID, 0},
    {" starts at 1", PT_ERR_INVALID, 0}, {": bad triangle material", PT_ERR_INVALID, 0}, {"PT_FLAG_WRITE_RGBA needs rgba_dev", PT_ERR_INVALID, 0},
    {"PT_FLAG_NEE needs PT_FLAG_COSINE_DIFF", PT_ERR_INVALID, 0}, {"PT_FLAG_MIS needs PT_FLAG_NEE", PT_ERR_INVALID, 0},
    {"part_index out of range", PT_ERR_INVALID, 0}, {"part_rows must be a positive multiple of 8", PT_ERR_INVALID, 0},
    {"width*height*spp too large for one call", PT_ERR_INVALID, 0}, {"too many path records for one call", PT_ERR_INVALID, 0},
    {"PT_FLAG_NEE over emissive triangles needs the exact", PT_ERR_UNSUPPORTED, 0}, {"Woop records need the wide walk", PT_ERR_UNSUPPORTED, 0},
    {"PT_FLAG_MIS needs the exact", PT_ERR_UNSUPPORTED, 0}, {"RNG draws per path", PT_ERR_UNSUPPORTED, 0},
    {"PT_FLAG_NEE in the stage-split pipeline packs", PT_ERR_UNSUPPORTED, 0},
    // check_camera_model's (pt_render_camera; pt_camera_rays asks the same function)
    {": unknown camera model", PT_ERR_INVALID, 0}, {": unknown flag bits", PT_ERR_INVALID, 0}, {"width and height must be >= 2", PT_ERR_INVALID, 0},
    {"first_pixel + n exceeds width * height", PT_ERR_INVALID, 0}, {"lens_radius must be finite", PT_ERR_INVALID, 0},
    {"ortho_height must be finite", PT_ERR_INVALID, 0}, {"fisheye_fov must be in", PT_ERR_INVALID, 0},
    // pt_render_pixels' own, and pt_select_pixels' (its null argument is the row above)
    {"without a pixel list n must equal", PT_ERR_INVALID, 0}, {"width and height must be >= 1", PT_ERR_INVALID, 0},
    {"threshold must be finite", PT_ERR_INVALID, 0}, {"min_samples must not exceed", PT_ERR_INVALID, 0},
    // pt_tonemap's and pt_meter's (their null argument and image rows are above)
    {"unknown curve or transfer", PT_ERR_INVALID, 0}, {"exposure must be finite and > 0", PT_ERR_INVALID, 0}, {"white must be > 0", PT_ERR_INVALID, 0},
    {"key must be finite and > 0", PT_ERR_INVALID, 0}, {"0 <= low_pct < high_pct <= 1", PT_ERR_INVALID, 0},
    {"0 < min_exposure <= max_exposure", PT_ERR_INVALID, 0}, {"adapt must be in 0..1", PT_ERR_INVALID, 0},
    // pt_render_aux's, the two filters', the three reprojections' and pt_frame_error's (null argument, image and threshold rows are above)
    {": no BVH uploaded", PT_ERR_NO_SCENE, 0}, {"the binary walk reads Moller-Trumbore records", PT_ERR_UNSUPPORTED, 0},
    {"iterations must be 0..10", PT_ERR_INVALID, 0}, {"a sigma is not finite", PT_ERR_INVALID, 0}, {": null moments", PT_ERR_INVALID, 0},
    {"samples_per_frame must be finite and >= 1", PT_ERR_INVALID, 0}, {"out_variance_dev may not be one of the inputs", PT_ERR_INVALID, 0},
    {"max_history must be finite and >= 1", PT_ERR_INVALID, 0}, {"plane_tolerance must be finite and >= 0", PT_ERR_INVALID, 0},
    {"normal_threshold must be in -1..1", PT_ERR_INVALID, 0}, {"a history needs its camera, lengths, normals and positions", PT_ERR_INVALID, 0},
    {": ids of both frames or of neither", PT_ERR_INVALID, 0}, {"the new history may not overwrite the old one", PT_ERR_INVALID, 0},
    {"the ids of both frames are required", PT_ERR_INVALID, 0}, {"a null vertex buffer with n_tris > 0", PT_ERR_INVALID, 0},
    {"n_tris must be < 2^31", PT_ERR_INVALID, 0}, {"motion_dev may not be one of the other buffers", PT_ERR_INVALID, 0},
    {"the standard error needs n_samples >= 2", PT_ERR_INVALID, 0}, {"more than 2^32 - 1 pixels", PT_ERR_INVALID, 0},
    // pt_temporal_camera's own (pt_render_aux_camera's are pt_render_aux's and check_camera_model's)
    {"a history needs the model of its camera", PT_ERR_INVALID, 0}, {"the model's image must be the parameters'", PT_ERR_INVALID, 0},
};
static long n_refused = 0, n_planned = 0;
// true: the planner refused the call or found nothing to do in it
static bool turned_away(const Refusal& r) {
    if (r.code == PT_OK) return r.nothing;
    n_refused++;
    int rows = 0;
    for (auto& e : REFUSALS)
        if (r.msg.find(e.text) != std::string::npos) { rows++; e.seen++; CHECK(r.code == e.code); }
    if (rows != 1 && n_failed++ < 20) std::printf("FAILED: the refusal \"%s\" matches %d rows of REFUSALS\n", r.msg.c_str(), rows);
    return true;
}

// ---- the domain: scenes
struct Tree { bool has_bvh, woop; uint32_t wide_depth, n_occ; };
static const Tree NO_TREE = {false, false, 0, 0}, TREE = {true, false, 10, 0}, TREE_OCC = {true, false, 10, 3}, TREE_WOOP = {true, true, 10, 0},
                  TREE_23 = {true, false, 23, 0},   // 3 x 23 + 2 = 71 entries: the wide walk's stack holds it, a packet stack of 40 does not
                  TREE_DEEP = {true, false, 24, 2}, TREE_WOOP_DEEP = {true, true, 24, 0};
static const Tree TREES[] = {NO_TREE, TREE, TREE_OCC, TREE_WOOP, TREE_23, TREE_DEEP, TREE_WOOP_DEEP};
struct Spheres { int n; bool refr; };   // refr: one of the first PT_KSPHERES is PT_MAT_REFR
static const Spheres SPHERES[] = {{0, false}, {3, false}, {9, false}, {8, true}, {20, true}};
struct Mats { bool table, emits; };
static const Mats MATS[] = {{false, false}, {true, false}, {true, true}};

// a new context's options (pt_ctx.h) over the scene
static CtxFacts scene(const Tree& t, const Spheres& s, const Mats& m, int env) {
    CtxFacts f = {};
    f.has_bvh = t.has_bvh; f.records_woop = t.woop; f.wide_depth = t.wide_depth; f.n_occ = t.n_occ;
    f.n_top_layout = t.has_bvh ? 100 : 0; f.wide_top_layout = t.has_bvh ? 40 : 0;
    f.n_spheres = s.n;
    for (int i = 0; i < PT_KSPHERES && i < s.n; i++) f.sphere_mat[i] = i == 1 && s.refr ? PT_MAT_REFR : PT_MAT_DIFF + i % 3;
    f.mat_table = m.table; f.tri_emits = m.emits;
    f.env = env; f.n_cu = 256;
    f.kernel = PT_KERNEL_AUTO; f.overlap = 1; f.sph_lds = 1; f.top = 64; f.occ = 6; f.lstk = 16; f.walk = 2; f.batch = 36; f.refill = 8;
    f.vote_node = f.vote_rec = 1; f.wave_batch = 16; f.wave_samples = 16; f.wave_blocks = 8; f.first_walk = 1; f.packet_stack = 72;
    f.fuse_stages = f.last_anyhit = f.root_cull = f.root_entry = f.last_occluders = f.path_history = 1;
    return f;
}
static pt_params params(int w, int h, uint32_t depth, uint32_t flags) {
    pt_params p = {};
    p.width = w; p.height = h; p.depth = depth; p.flags = flags;
    p.sample_index = 1; p.tri_mat = PT_MAT_DIFF;
    return p;
}
static CallFacts frame(const pt_params& p, uint32_t spp, bool moments = false) { return {true, &p, spp, true, true, moments, 0, 0}; }

// ---- pt_render: the steps in pt_render_moments' order.  One frame call under given answers of the runtime; false: turned away
static bool frame_call(const CtxFacts& f, const CallFacts& a, const AutoAnswer& au, bool caller_idle, CallPlan& plan) {
    if (turned_away(check_path_call(f, a)) || turned_away(tri_lights_rule(f, a.p->flags))) return false;
    TileGrid g;
    if (turned_away(frame_tiles(*a.p, a.spp, g)) || turned_away(plan_walk(f, a, plan))) return false;
    plan_family(f, a, au, plan);
    return !turned_away(plan_launch(f, a, g.n_tiles, caller_idle, plan));
}
static std::set<int> wave_calls;   // (count, nee, deep stack, moments) of the calls that run the pipeline
// what holds of every plan, and the words its launches ask for
static void frame_plan(const CtxFacts& f, const CallFacts& a, const CallPlan& plan) {
    const LaunchCfg& L = plan.L;
    n_planned++;
    CHECK(L.lds <= PT_LDS_BYTES && plan.q.refill <= plan.q.batch && L.work_blocks >= 1 && L.blocks >= 1 && plan.work_tiles >= 1);
    CHECK(plan.chunk == 16 || plan.chunk == 32 || plan.chunk == 64);
    CHECK(plan.sph_tab < 0 || (size_t)(plan.sph_tab + 15 * PT_KSPHERES) * 4 == L.lds);
    CHECK(!plan.side || (plan.samples && plan.probe < 0));
    if (plan.kernel == PT_KERNEL_MEGA_BVH2) mega.request(mega_word(L));
    else if (plan.kernel == PT_KERNEL_PERSISTENT) persist.request(persist_word(L));
    if (plan.kernel != PT_KERNEL_WAVEFRONT) {
        CHECK(plan.kernel == PT_KERNEL_MEGA_BVH2 || plan.kernel == PT_KERNEL_PERSISTENT);
        return;
    }
    CHECK(f.env == ENV_NONE && !L.mis && plan.samples && !plan.side);   // a pipeline plan never coexists with a map
    wave_calls.insert((L.count ? 1 : 0) | (L.nee ? 2 : 0) | (L.lstk == 24 ? 4 : 0) | (a.moments ? 8 : 0));
    const WaveLayout& w = plan.wl;
    CHECK(w.cap < (1ull << 31) && w.cap >= (size_t)plan.work_tiles * 64 && w.off[0] == 0 && w.off[W_PIECES] == w.need && w.nee == L.nee);
    for (int i = 0; i < W_PIECES; i++) CHECK(w.off[i] <= w.off[i + 1] && w.off[i] % 16 == 0);   // in order, none over the next; float4 pieces aligned
    CHECK(w.off[W_RAY0 + 1] - w.off[W_RAY0] == w.cap * 16 && w.off[W_QUEUES + 1] - w.off[W_QUEUES] == w.q_words * 4);
    CHECK((w.off[W_S_RAY0] == w.need) == !w.nee);   // the shadow records only under PT_FLAG_NEE
    const WavePlan& p = plan.wave;
    const uint32_t depth = a.p->depth;
    for (uint32_t b = 0; b < depth; b++) {   // render_wavefront's launches, bounce by bounce
        const WaveExtend e = p.extend(b, depth);
        if (e == EXT_FUSED) fused.request(fused_word(p, depth));
        else if (e != EXT_PACKET) extend.request(extend_word(p, e));   // (k_wf_extend_packet has COUNT alone)
        const WaveShade s = p.shade(b, depth);
        CHECK((s == SHADE_NONE) == (e == EXT_FUSED));
        if (s == SHADE_LAST_ANY) last_any.request(shade_word(p, s, b == 0));
        else if (s != SHADE_NONE) shade.request(shade_word(p, s, b == 0));
        if (L.nee) extend.request(extend_word(p, EXT_CLOSEST));   // the bounce's shadow rays
    }
}
// the call under every answer the runtime can give it: PT_KERNEL_AUTO's table where the plan looks it up (no trial and nothing decided, the
// four trials, either choice), the caller's stream idle or busy where the plan asks
static void frame_calls(const CtxFacts& f, const CallFacts& a) {
    static const AutoAnswer AUTO[] = {{-1, false, PT_KERNEL_PERSISTENT}, {0, false, PT_KERNEL_PERSISTENT}, {1, false, PT_KERNEL_PERSISTENT}, {2, false, PT_KERNEL_PERSISTENT},
                                      {3, false, PT_KERNEL_PERSISTENT}, {-1, true, PT_KERNEL_PERSISTENT}, {-1, true, PT_KERNEL_WAVEFRONT}};
    CallPlan plan;
    for (const AutoAnswer& au : AUTO) {
        for (int idle = 0; idle < 2; idle++) {
            if (!frame_call(f, a, au, idle != 0, plan)) return;   // (the refusals do not depend on the runtime's answers)
            frame_plan(f, a, plan);
            if (!plan.idle_query) break;
        }
        if (!plan.lookup) break;
    }
}

int main() {
    const uint32_t COS = PT_FLAG_COSINE_DIFF, NEE = PT_FLAG_NEE | COS, MIS = PT_FLAG_MIS | NEE;
    const int KERNELS[] = {PT_KERNEL_AUTO, PT_KERNEL_MEGA_BVH2, PT_KERNEL_PERSISTENT, PT_KERNEL_WAVEFRONT};

    // (a) which family, which budget: every tree x map x material table, the options that choose among the frame kernels, the flags that do
    for (const Tree& t : TREES)
        for (int env = ENV_NONE; env <= ENV_LIGHT; env++)
            for (const Mats& m : {MATS[0], MATS[2]})
                for (int kernel : KERNELS)
                    for (int count = 0; count < 2; count++)
                        for (int walk : {0, 1, 2, 4})
                            for (int lstk : {0, 16, 24})
                                for (int occ : {4, 5, 6, 8}) {
                                    CtxFacts f = scene(t, SPHERES[t.has_bvh ? 1 : 0], m, env);
                                    f.kernel = kernel; f.counters = count; f.walk = walk; f.lstk = lstk; f.occ = occ;
                                    for (uint32_t flags : {0u, COS, NEE, MIS, (uint32_t)PT_FLAG_NEE, (uint32_t)(PT_FLAG_MIS | COS)})
                                        for (uint32_t depth : {0u, 3u})
                                            for (uint32_t spp : {1u, 4u})
                                                for (int moments = 0; moments < 2; moments++) {
                                                    const pt_params p = params(100, 60, depth, flags);
                                                    frame_calls(f, frame(p, spp, moments != 0));
                                                }
                                }
    CHECK(wave_calls.size() == 16);   // every (count, nee, deep stack, moments)

    // (b) what the pipeline launches: the scenes that decide the last segment's any-hit query, the path history, the occluder test and
    // the packet walk; every value of the stage options; depths 1 .. 4; (spp): one sample, the groups of 4, 8 and 16 that a fused fold
    // needs, a group that is not the whole call
    struct { Tree t; Spheres s; Mats m; } const WAVE_SCENES[] = {{TREE_OCC, SPHERES[1], MATS[0]}, {TREE, SPHERES[3], MATS[0]}, {TREE_OCC, SPHERES[4], MATS[0]},
                                                               {TREE, SPHERES[0], MATS[2]}, {TREE_23, SPHERES[0], MATS[0]}, {TREE_OCC, SPHERES[2], MATS[1]}};
    for (const auto& s : WAVE_SCENES)
        for (int bits = 0; bits < 32; bits++)
            for (int opts = 0; opts < 243; opts++) {
                CtxFacts f = scene(s.t, s.s, s.m, ENV_NONE);
                f.kernel = PT_KERNEL_WAVEFRONT;
                f.counters = bits & 1; f.lstk = bits & 2 ? 24 : 16; f.first_walk = bits & 4 ? 1 : 0; f.packet_stack = bits & 8 ? 72 : 40; f.fuse_stages = bits & 16 ? 1 : 0;
                f.last_anyhit = opts % 3; f.root_cull = opts / 3 % 3; f.root_entry = opts / 9 % 3; f.path_history = opts / 27 % 3; f.last_occluders = opts / 81 % 3;
                for (uint32_t flags : {0u, NEE})
                    for (uint32_t depth = 1; depth <= 4; depth++)
                        for (uint32_t spp : {1u, 4u, 8u, 16u, 32u})
                            for (int call = 0; call < 4; call++) {   // moments; a triangle material that emits
                                pt_params p = params(100, 60, depth, flags);
                                p.tri_emi[1] = call & 2 ? 1.f : 0.f;
                                frame_calls(f, frame(p, spp, (call & 1) != 0));
                            }
            }

    // (c) every other option planning reads, at the ends of its range and between, one at a time over a new context's values
    struct { int CtxFacts::*opt; std::vector<int> values; } const KNOBS[] = {
        {&CtxFacts::timing, {0, 1}}, {&CtxFacts::overlap, {0, 1}}, {&CtxFacts::sph_lds, {0, 1}}, {&CtxFacts::top, {0, 1, 64, 100, 1024}},
        {&CtxFacts::batch, {1, 7, 36, 64}}, {&CtxFacts::refill, {1, 8, 37, 64}}, {&CtxFacts::vote_node, {1, 64}}, {&CtxFacts::vote_rec, {1, 64}},
        {&CtxFacts::wave_batch, {1, 16, 64}}, {&CtxFacts::wave_samples, {1, 2, 4, 7, 8, 16, 32, 64}}, {&CtxFacts::wave_blocks, {1, 8}},
        {&CtxFacts::packet_stack, {2, 31, 32, 72}}, {&CtxFacts::n_cu, {1, 256, 304}}};
    for (const auto& knob : KNOBS)
        for (int value : knob.values)
            for (int kernel : KERNELS)
                for (int walk : {0, 2})
                    for (const Spheres& s : SPHERES)
                        for (const Tree& t : {NO_TREE, TREE, TREE_OCC})
                            for (uint32_t spp : {1u, 3u, 4u, 16u, 64u, 4096u}) {
                                CtxFacts f = scene(t, s, MATS[0], ENV_NONE);
                                f.*knob.opt = value; f.kernel = kernel; f.walk = walk;
                                for (int side : {2, 100, 1920}) {   // one tile .. enough slots for 64-slot chunks
                                    const pt_params p = params(side, side > 100 ? 1080 : side, 5, 0);
                                    frame_calls(f, frame(p, spp));
                                }
                            }

    // (d) the argument rules of pt_render, one broken at a time and several together (the first in the rules' order answers)
    {
        const CtxFacts f = scene(TREE, SPHERES[1], MATS[0], ENV_NONE), empty = scene(NO_TREE, SPHERES[0], MATS[0], ENV_NONE);
        CallPlan plan;
        const AutoAnswer none = {-1, false, PT_KERNEL_PERSISTENT};
        for (int broken = 0; broken < (1 << 11); broken++) {
            pt_params p = params(broken & 1 ? 1 : 64, 64, 3, broken & 2 ? (uint32_t)PT_FLAG_NEE : broken & 4 ? (uint32_t)(PT_FLAG_MIS | COS) : 0u);
            if (broken & 8) p.sample_index = 0;
            if (broken & 16) p.tri_mat = PT_MAT_REFR + 1;
            if (broken & 32) p.flags |= PT_FLAG_WRITE_RGBA;
            p.part_count = broken & 64 ? 4 : 0; p.part_rows = broken & 128 ? 12 : 8; p.part_index = broken & 256 ? 4 : 1;
            CallFacts a = frame(p, broken & 512 ? 0 : 1);
            a.rgba = false;
            a.buffers = !(broken & 1024);
            const bool ran = frame_call(f, a, none, false, plan);
            const bool bad = (broken & ~(64 | 128 | 256)) || ((broken & 64) && (broken & (128 | 256)));   // (the part's fields count with part_count > 1)
            CHECK(ran == !bad);
            (void)frame_call(empty, a, none, false, plan);
        }
        const CallFacts null_params = {true, nullptr, 1, true, true, false, 0, 0};
        CHECK(!frame_call(f, null_params, none, false, plan));
        pt_params p = params(64, 8, 3, 0);   // one tile-row in stripes of 8 rows: part 1 of 2 owns no tile, nothing to render
        p.part_count = 2; p.part_rows = 8; p.part_index = 1;
        CHECK(check_path_call(f, frame(p, 1)).code == PT_OK && !frame_call(f, frame(p, 1), none, false, plan));
    }

    // (e) tests/test_gpu_call_plan.py::CASES, worked by hand: the family each call runs on a new context with a tree and nine spheres
    {
        struct { const char* id; int kernel; Tree tree; int walk, counters; uint32_t flags, depth; int family; bool lookup; } const CASES[] = {
            {"wavefront", PT_KERNEL_WAVEFRONT, TREE, 2, 0, 0, 3, PT_KERNEL_WAVEFRONT, false},
            {"wavefront-depth0", PT_KERNEL_WAVEFRONT, TREE, 2, 0, 0, 0, PT_KERNEL_PERSISTENT, false},
            {"wavefront-walk0", PT_KERNEL_WAVEFRONT, TREE, 0, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"wavefront-walk1", PT_KERNEL_WAVEFRONT, TREE, 1, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"wavefront-walk4", PT_KERNEL_WAVEFRONT, TREE, 4, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"wavefront-no-tree", PT_KERNEL_WAVEFRONT, NO_TREE, 2, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"wavefront-woop", PT_KERNEL_WAVEFRONT, TREE_WOOP, 2, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"persistent", PT_KERNEL_PERSISTENT, TREE, 2, 0, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"persistent-nee", PT_KERNEL_PERSISTENT, TREE, 2, 0, NEE, 3, PT_KERNEL_WAVEFRONT, false},
            {"persistent-nee-walk0", PT_KERNEL_PERSISTENT, TREE, 0, 0, NEE, 3, PT_KERNEL_MEGA_BVH2, false},
            {"auto", PT_KERNEL_AUTO, TREE, 2, 0, 0, 3, PT_KERNEL_WAVEFRONT, true},   // (under the answer below: trial 1, the pipeline's)
            {"auto-counters", PT_KERNEL_AUTO, TREE, 2, 1, 0, 3, PT_KERNEL_PERSISTENT, false},
            {"auto-nee", PT_KERNEL_AUTO, TREE, 2, 0, NEE, 3, PT_KERNEL_WAVEFRONT, false},
            {"mis", PT_KERNEL_WAVEFRONT, TREE, 2, 0, MIS, 3, PT_KERNEL_MEGA_BVH2, false},
            {"auto-mis", PT_KERNEL_AUTO, TREE, 2, 0, MIS, 3, PT_KERNEL_MEGA_BVH2, false},
        };
        for (const auto& k : CASES) {
            CtxFacts f = scene(k.tree, SPHERES[2], MATS[0], ENV_NONE);
            f.kernel = k.kernel; f.walk = k.walk; f.counters = k.counters;
            const pt_params p = params(96, 64, k.depth, k.flags);
            CallPlan plan;
            const bool ran = frame_call(f, frame(p, 1), AutoAnswer{1, false, PT_KERNEL_PERSISTENT}, true, plan);
            if ((!ran || plan.kernel != k.family || plan.lookup != k.lookup) && n_failed++ < 20) std::printf("FAILED: case %s plans family %d\n", k.id, ran ? plan.kernel : -1);
        }
    }

    // (f) the pipeline's refusals at their edges: the last call that runs and the first that does not
    {
        CtxFacts f = scene(TREE, SPHERES[1], MATS[0], ENV_NONE);
        f.kernel = PT_KERNEL_WAVEFRONT;
        CallPlan plan;
        const AutoAnswer none = {-1, false, PT_KERNEL_PERSISTENT};
        auto runs = [&](int w, int h, uint32_t depth, uint32_t flags, uint32_t spp) {
            const pt_params p = params(w, h, depth, flags);
            const bool ran = frame_call(f, frame(p, spp), none, false, plan);
            if (ran) frame_plan(f, frame(p, spp), plan);
            return ran;
        };
        static_assert(2047 * 2 + 2 == PT_REC_MAX_DRAWS, "two draws per cosine-weighted bounce, two for the camera");
        CHECK(runs(8, 8, 2046, COS, 1) && !runs(8, 8, 2047, COS, 1));                                       // depth * draws + 2 == PT_REC_MAX_DRAWS
        CHECK(runs(8, 8, 3, 0, PT_REC_MAX_SAMPLES - 1) && !runs(8, 8, 3, 0, PT_REC_MAX_SAMPLES));         // spp == 2^20
        CHECK(runs(8, 8, 3, NEE, PT_REC_MAX_SAMPLES_NEE - 1) && !runs(8, 8, 3, NEE, PT_REC_MAX_SAMPLES_NEE));
        CHECK(runs(64, 64, 3, 0, (1u << 19) - 1) && !runs(64, 64, 3, 0, 1u << 19));                       // n_tiles * 64 * spp == 2^31: 64 tiles
        // 2^25 - 1 = 31 * 601 * 1801 tiles are 2^23 regions, 2^31 records: one too many
        CHECK(!runs(8 * 31 * 601, 8 * 1801, 3, 0, 1) && runs(8 * 31 * 601, 8 * 1800, 3, 0, 1));
        f.kernel = PT_KERNEL_PERSISTENT;   // the frame kernels have no such limits
        CHECK(runs(8, 8, 2047, COS, 1) && runs(8, 8, 3, 0, PT_REC_MAX_SAMPLES) && runs(8 * 31 * 601, 8 * 1801, 3, 0, 1));
    }

    // (g) pt_render_rays: every scene and map, the options its plan reads, the flags, batches around RAYS_MAX_SLOTS, every launch of a call
    for (const Tree& t : TREES)
        for (int env = ENV_NONE; env <= ENV_LIGHT; env++)
            for (const Mats& m : {MATS[0], MATS[2]})
                for (int walk : {0, 1, 2, 4})
                    for (int knobs = 0; knobs < 4; knobs++)
                        for (uint32_t flags : {0u, COS, NEE, MIS, (uint32_t)PT_FLAG_NEE, (uint32_t)(PT_FLAG_MIS | COS)})
                            for (uint64_t n : {0ull, 1ull, 1000ull, (1ull << 26) / 3, 1ull << 26, (1ull << 32) - 1, 1ull << 32})
                                for (uint32_t spp : {0u, 1u, 3u, 64u})
                                    for (int mode : {(int)PT_RAYS_CLAMPED, (int)PT_RAYS_HDR, 7}) {
                                        CtxFacts f = scene(t, SPHERES[t.has_bvh ? 2 : knobs & 1], m, env);
                                        f.walk = walk; f.sph_lds = knobs & 1; f.n_cu = knobs & 2 ? 256 : 8;
                                        pt_params p = params(0, 0, 4, flags);
                                        const CallFacts a = {false, &p, spp, true, false, false, n, mode};
                                        RaysPlan plan = {};
                                        if (turned_away(check_path_call(f, a)) || turned_away(tri_lights_rule(f, flags)) || turned_away(plan_rays(f, a, plan))) continue;
                                        n_planned++;
                                        rays.request(rays_word(plan.L));
                                        CHECK(plan.L.lds <= PT_LDS_BYTES && plan.q.refill <= plan.q.batch && plan.per_launch >= 1 && plan.per_launch <= spp);
                                        CHECK(plan.per_launch == 1 || plan.per_launch * n <= RAYS_MAX_SLOTS);
                                        for (uint32_t s0 = 0; s0 < spp; s0 += plan.per_launch) {
                                            int work_blocks = 0;
                                            const int chunk = plan_rays_launch(f, a, plan, std::min(plan.per_launch, spp - s0), work_blocks);
                                            CHECK(work_blocks >= 1 && (chunk == 16 || chunk == 32 || chunk == 64));
                                        }
                                    }
    {   // ... and its own argument rules
        const CtxFacts f = scene(TREE, SPHERES[1], MATS[0], ENV_NONE);
        pt_params p = params(0, 0, 4, 0);
        CHECK(turned_away(check_path_call(f, CallFacts{false, &p, 1, false, false, false, 10, PT_RAYS_HDR})));
        CHECK(turned_away(check_path_call(f, CallFacts{false, nullptr, 1, true, false, false, 10, PT_RAYS_HDR})));
        CHECK(check_path_call(f, CallFacts{false, nullptr, 0, false, false, false, 10, 7}).nothing);   // nothing to do comes first
        p.sample_index = 0;
        CHECK(turned_away(check_path_call(f, CallFacts{false, &p, 1, true, false, false, 10, PT_RAYS_HDR})));
        p.sample_index = 1; p.tri_mat = -1;
        CHECK(turned_away(check_path_call(f, CallFacts{false, &p, 1, true, false, false, 10, PT_RAYS_HDR})));
    }

    // (g') pt_render_camera: (g)'s domain — its plan is plan_rays under its own name — over the five models, without and with a pixel
    // list; the image holds every n of the domain but 2^32 - 1 and 2^32 (65536 x 65535 pixels), which a list alone can ask for
    auto model = [](int kind, int w, int h) {
        pt_camera_model cm = {};
        cm.model = kind; cm.width = w; cm.height = h;
        cm.lens_radius = 0.1f; cm.focus_dist = 3.0f; cm.ortho_height = 4.0f; cm.fisheye_fov = 3.0f;
        return cm;
    };
    for (const Tree& t : TREES)
        for (int env = ENV_NONE; env <= ENV_LIGHT; env++)
            for (const Mats& m : {MATS[0], MATS[2]})
                for (int walk : {0, 1, 2, 4})
                    for (int knobs = 0; knobs < 4; knobs++)
                        for (uint32_t flags : {0u, COS, NEE, MIS, (uint32_t)PT_FLAG_NEE, (uint32_t)(PT_FLAG_MIS | COS)})
                            for (uint64_t n : {0ull, 1ull, 1000ull, (1ull << 26) / 3, 1ull << 26, (1ull << 32) - 1, 1ull << 32})
                                for (uint32_t spp : {0u, 1u, 3u, 64u})
                                    for (int call = 0; call < 10; call++) {   // model x list
                                        CtxFacts f = scene(t, SPHERES[t.has_bvh ? 2 : knobs & 1], m, env);
                                        f.walk = walk; f.sph_lds = knobs & 1; f.n_cu = knobs & 2 ? 256 : 8;
                                        pt_params p = params(0, 0, 4, flags);
                                        const pt_camera_model cm = model(call % 5, 65536, 65535);
                                        const bool list = call >= 5;
                                        const CallFacts a = {false, &p, spp, true, false, false, n, call == 3 ? (int)PT_RAYS_HDR : (int)PT_RAYS_CLAMPED, true, &cm, list, list ? 0u : 5u};
                                        RaysPlan plan = {};
                                        const Refusal r = check_path_call(f, a);
                                        // the rows the image cannot hold, or 2^32 of them, are turned away in the call's own name
                                        if (r.code != PT_OK) CHECK(r.msg.rfind("pt_render_camera: ", 0) == 0);
                                        if (turned_away(r) || turned_away(tri_lights_rule(f, flags)) || turned_away(plan_rays(f, a, plan))) continue;
                                        CHECK(n < (1ull << 32) && (list || n + 5 <= 65536ull * 65535ull));
                                        n_planned++;
                                        camera.request(rays_word(plan.L));
                                        CHECK(plan.L.lds <= PT_LDS_BYTES && plan.q.refill <= plan.q.batch && plan.per_launch >= 1 && plan.per_launch <= spp);
                                        CHECK(plan.per_launch == 1 || plan.per_launch * n <= RAYS_MAX_SLOTS);
                                        for (uint32_t s0 = 0; s0 < spp; s0 += plan.per_launch) {
                                            int work_blocks = 0;
                                            const int chunk = plan_rays_launch(f, a, plan, std::min(plan.per_launch, spp - s0), work_blocks);
                                            CHECK(work_blocks >= 1 && (chunk == 16 || chunk == 32 || chunk == 64));
                                        }
                                    }
    {   // ... and its argument rules, each broken alone and the order in which they answer (include/ptmi.h)
        const CtxFacts f = scene(TREE, SPHERES[1], MATS[0], ENV_NONE), empty = scene(NO_TREE, SPHERES[0], MATS[0], ENV_NONE), woop = scene(TREE_WOOP, SPHERES[1], MATS[0], ENV_NONE);
        pt_params p = params(0, 0, 4, 0);
        pt_camera_model cm = model(PT_CAM_PINHOLE, 37, 23);
        auto call = [&](const CtxFacts& ctx, const pt_params* pp, uint32_t spp, bool buffers, uint64_t n, int mode, bool list, uint64_t first) {
            const CallFacts a = {false, pp, spp, buffers, false, false, n, mode, true, &cm, list, first};
            Refusal r = check_path_call(ctx, a);
            RaysPlan plan = {};
            if (r.code == PT_OK && !r.nothing) r = plan_rays(ctx, a, plan);
            if (r.code != PT_OK) { CHECK(turned_away(r)); CHECK(r.msg.rfind("pt_render_camera: ", 0) == 0); }
            return r;
        };
        auto says = [](const Refusal& r, const char* text) { return r.code != PT_OK && r.msg.find(text) != std::string::npos; };
        CHECK(call(f, &p, 3, true, 37 * 23, PT_RAYS_CLAMPED, false, 0).code == PT_OK);
        CHECK(says(call(empty, nullptr, 0, false, 0, 7, false, 0), "no scene uploaded"));        // no scene comes before nothing to do
        CHECK(call(f, nullptr, 0, false, 10, 7, false, 0).nothing && call(f, nullptr, 3, false, 0, 7, false, 0).nothing);   // ... which comes before NULLs
        CHECK(says(call(f, &p, 1, false, 10, 7, false, 0), "null argument") && says(call(f, nullptr, 1, true, 10, 7, false, 0), "null argument"));
        cm.model = 9;
        CHECK(says(call(f, &p, 1, true, 10, 7, false, 0), "mode must be"));                        // the mode before the model
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "unknown camera model"));
        cm.model = -1;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "unknown camera model"));
        cm = model(PT_CAM_FISHEYE, 37, 23); cm.flags = 2; cm.width = 1;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "unknown flag bits"));       // the flags before the image
        cm.flags = PT_CAMF_CENTRE;
        CHECK(says(call(f, &p, 1, true, 1ull << 32, PT_RAYS_HDR, false, 0), "width and height"));  // the image before n
        cm.width = 65536; cm.height = 65536;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, true, 0), "width and height"));
        cm.width = 37; cm.height = 23;
        CHECK(says(call(f, &p, 1, true, 1ull << 32, PT_RAYS_HDR, true, 0), "more than 2^32 - 1 rays"));
        CHECK(says(call(f, &p, 1, true, 1ull << 32, PT_RAYS_HDR, false, 0), "more than 2^32 - 1 rays"));   // n before first_pixel + n
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false, 1), "first_pixel + n exceeds") && says(call(f, &p, 1, true, 1, PT_RAYS_HDR, false, 37 * 23 + 1), "first_pixel + n exceeds"));
        CHECK(call(f, &p, 1, true, 37 * 23 - 1, PT_RAYS_HDR, false, 1).code == PT_OK && call(f, &p, 1, true, 5000, PT_RAYS_HDR, true, 1ull << 40).code == PT_OK);   // a list: first_pixel is not read
        cm.fisheye_fov = 7.0f; p.sample_index = 0;
        CHECK(says(call(f, &p, 1, true, 37 * 23 + 1, PT_RAYS_HDR, false, 0), "first_pixel + n exceeds"));   // ... before the model's parameter
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "fisheye_fov must be"));       // the model's parameter before pt_render_rays' own rules
        cm.fisheye_fov = 0.0f;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "fisheye_fov must be"));
        cm.model = PT_CAM_ORTHO;   // another model's parameter is ignored
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), " starts at 1"));
        const float inf = 1.0f / 0.0f * (float)(p.depth != 0), nan = inf - inf;
        for (float bad : {0.0f, -1.0f, inf, nan}) { cm.ortho_height = bad; CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "ortho_height must be")); }
        cm = model(PT_CAM_THIN_LENS, 37, 23);
        for (float bad : {-0.5f, inf, nan}) { cm.lens_radius = bad; CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "lens_radius must be")); }
        cm.lens_radius = 0.0f;
        for (float bad : {0.0f, -1.0f, inf, nan}) { cm.focus_dist = bad; CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "lens_radius must be")); }
        cm.focus_dist = 1.0f;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), " starts at 1"));
        p.sample_index = 1; p.tri_mat = -1; p.flags = PT_FLAG_NEE;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "bad triangle material"));
        p.tri_mat = PT_MAT_DIFF;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "PT_FLAG_NEE needs PT_FLAG_COSINE_DIFF"));
        p.flags = PT_FLAG_MIS | COS;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "PT_FLAG_MIS needs PT_FLAG_NEE"));
        p.flags = MIS;
        CHECK(call(f, &p, 1, true, 10, PT_RAYS_HDR, false, 0).code == PT_OK && says(call(woop, &p, 1, true, 10, PT_RAYS_HDR, false, 0), "PT_FLAG_MIS needs the exact"));
    }

    // (g'') pt_render_pixels: pt_render_camera's kernels over a list or over the whole image (n = W * H then, so the image is the n of the
    // domain where it can be one), with and without moments; every launch goes through the sample buffer, a one-sample launch too
    for (const Tree& t : TREES)
        for (int env = ENV_NONE; env <= ENV_LIGHT; env++)
            for (const Mats& m : {MATS[0], MATS[2]})
                for (int walk : {0, 1, 2, 4})
                    for (int knobs = 0; knobs < 4; knobs++)
                        for (uint32_t flags : {0u, COS, NEE, MIS, (uint32_t)PT_FLAG_NEE, (uint32_t)(PT_FLAG_MIS | COS)})
                            for (uint64_t n : {0ull, 1ull, 1000ull, (1ull << 26) / 3, 1ull << 26, (1ull << 32) - 1, 1ull << 32})
                                for (uint32_t spp : {0u, 1u, 3u, 64u})
                                    for (int call = 0; call < 10; call++) {   // model x list
                                        CtxFacts f = scene(t, SPHERES[t.has_bvh ? 2 : knobs & 1], m, env);
                                        f.walk = walk; f.sph_lds = knobs & 1; f.n_cu = knobs & 2 ? 256 : 8;
                                        pt_params p = params(0, 0, 4, flags);
                                        const bool list = call >= 5;
                                        // without a list the image has n pixels where two factors >= 2 give it: 1000, 2^26
                                        const pt_camera_model cm = list ? model(call % 5, 65536, 65535) : n == 1000 ? model(call % 5, 40, 25) : model(call % 5, 8192, 8192);
                                        CallFacts a = {false, &p, spp, true, false, (call & 1) != 0, n, call == 3 ? (int)PT_RAYS_HDR : (int)PT_RAYS_CLAMPED, true, &cm, list, 0};
                                        a.pixels = true;
                                        RaysPlan plan = {};
                                        const Refusal r = check_path_call(f, a);
                                        if (r.code != PT_OK) CHECK(r.msg.rfind("pt_render_pixels: ", 0) == 0);
                                        if (turned_away(r) || turned_away(tri_lights_rule(f, flags)) || turned_away(plan_rays(f, a, plan))) continue;
                                        CHECK(n < (1ull << 32) && (list || n == (uint64_t)cm.width * (uint64_t)cm.height));
                                        n_planned++;
                                        camera.request(rays_word(plan.L));
                                        CHECK(plan.samples);   // never the kernel's fold in line
                                        CHECK(plan.L.lds <= PT_LDS_BYTES && plan.q.refill <= plan.q.batch && plan.per_launch >= 1 && plan.per_launch <= spp);
                                        CHECK(plan.per_launch == 1 || plan.per_launch * n <= RAYS_MAX_SLOTS);
                                        for (uint32_t s0 = 0; s0 < spp; s0 += plan.per_launch) {
                                            int work_blocks = 0;
                                            const int chunk = plan_rays_launch(f, a, plan, std::min(plan.per_launch, spp - s0), work_blocks);
                                            CHECK(work_blocks >= 1 && (chunk == 16 || chunk == 32 || chunk == 64));
                                        }
                                    }
    {   // ... its argument rules are pt_render_camera's under its own name, with one of its own where first_pixel's stands
        const CtxFacts f = scene(TREE, SPHERES[1], MATS[0], ENV_NONE), empty = scene(NO_TREE, SPHERES[0], MATS[0], ENV_NONE), woop = scene(TREE_WOOP, SPHERES[1], MATS[0], ENV_NONE);
        pt_params p = params(0, 0, 4, 0);
        pt_camera_model cm = model(PT_CAM_PINHOLE, 37, 23);
        auto call = [&](const CtxFacts& ctx, const pt_params* pp, uint32_t spp, bool buffers, uint64_t n, int mode, bool list) {
            CallFacts a = {false, pp, spp, buffers, false, true, n, mode, true, &cm, list, 0};
            a.pixels = true;
            Refusal r = check_path_call(ctx, a);
            RaysPlan plan = {};
            if (r.code == PT_OK && !r.nothing) { r = plan_rays(ctx, a, plan); CHECK(plan.samples); }
            if (r.code != PT_OK) { CHECK(turned_away(r)); CHECK(r.msg.rfind("pt_render_pixels: ", 0) == 0); }
            return r;
        };
        auto says = [](const Refusal& r, const char* text) { return r.code != PT_OK && r.msg.find(text) != std::string::npos; };
        CHECK(call(f, &p, 1, true, 37 * 23, PT_RAYS_CLAMPED, false).code == PT_OK && call(f, &p, 3, true, 5, PT_RAYS_HDR, true).code == PT_OK);
        CHECK(says(call(empty, nullptr, 0, false, 0, 7, false), "no scene uploaded"));           // no scene comes before nothing to do
        CHECK(call(f, nullptr, 0, false, 10, 7, false).nothing && call(f, nullptr, 3, false, 0, 7, true).nothing);   // ... which comes before NULLs
        CHECK(says(call(f, &p, 1, false, 10, 7, false), "null argument") && says(call(f, nullptr, 1, true, 10, 7, false), "null argument"));
        cm.model = 9;
        CHECK(says(call(f, &p, 1, true, 10, 7, false), "mode must be"));                           // the mode before the model
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false), "unknown camera model"));       // the model before n against the image
        cm = model(PT_CAM_FISHEYE, 37, 23); cm.flags = 2; cm.width = 1;
        CHECK(says(call(f, &p, 1, true, 10, PT_RAYS_HDR, false), "unknown flag bits"));
        cm.flags = 0;
        CHECK(says(call(f, &p, 1, true, 1ull << 32, PT_RAYS_HDR, false), "width and height"));     // the image before n
        cm.width = 37;
        CHECK(says(call(f, &p, 1, true, 1ull << 32, PT_RAYS_HDR, false), "more than 2^32 - 1 rays"));   // n < 2^32 before n against the image
        cm.fisheye_fov = 7.0f; p.sample_index = 0;
        for (uint64_t n : {1ull, 37ull * 23 - 1, 37ull * 23 + 1}) CHECK(says(call(f, &p, 1, true, n, PT_RAYS_HDR, false), "without a pixel list n must equal"));
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), "fisheye_fov must be"));     // ... before the model's parameter
        CHECK(says(call(f, &p, 1, true, 5000, PT_RAYS_HDR, true), "fisheye_fov must be"));         // a list may be longer than the image
        cm.fisheye_fov = 3.0f;
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), " starts at 1"));            // then pt_render_rays' own rules
        p.sample_index = 1; p.tri_mat = -1; p.flags = PT_FLAG_NEE;
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), "bad triangle material"));
        p.tri_mat = PT_MAT_DIFF;
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), "PT_FLAG_NEE needs PT_FLAG_COSINE_DIFF"));
        p.flags = PT_FLAG_MIS | COS;
        CHECK(says(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), "PT_FLAG_MIS needs PT_FLAG_NEE"));
        p.flags = MIS;
        CHECK(call(f, &p, 1, true, 37 * 23, PT_RAYS_HDR, false).code == PT_OK && says(call(woop, &p, 1, true, 37 * 23, PT_RAYS_HDR, false), "PT_FLAG_MIS needs the exact"));
    }

    // (g3) pt_select_pixels: every rule broken alone and together (the first in the header's order answers), and the scratch of a call that passes
    {
        const float inf = 1.0f / 0.0f * (float)(KERNELS[1] != 0), nan = inf - inf;
        auto says = [](const Refusal& r, const char* text) { return r.code != PT_OK && r.msg.find(text) != std::string::npos; };
        for (int broken = 0; broken < 32; broken++) {
            pt_select_params sp = {};
            sp.width = broken & 2 ? 0 : 1920; sp.height = 1080; sp.threshold = broken & 4 ? -0.5f : 0.05f;
            sp.min_samples = broken & 8 ? 65u : 4u; sp.max_samples = 64u;
            uint64_t n_pix = 0;
            const Refusal r = check_select_call(broken & 16 ? nullptr : &sp, !(broken & 1), n_pix);
            CHECK((r.code == PT_OK) == !broken);
            if (broken) CHECK(turned_away(r));
            CHECK(says(r, broken & 17 ? "null argument" : broken & 2 ? "width and height must be >= 1" : broken & 4 ? "threshold must be finite" : "min_samples must not exceed") == (broken != 0));
            if (!broken) {
                n_planned++;
                const SelectPlan s = plan_select(n_pix);
                CHECK(n_pix == 1920ull * 1080 && s.n_blocks == 8100 && s.read_back == 8100 * 12 && s.scratch == 8100 * 16);
            }
        }
        pt_select_params sp = {};
        sp.width = sp.height = 65536; sp.max_samples = 1;
        uint64_t n_pix = 0;
        CHECK(says(check_select_call(&sp, true, n_pix), "width and height must be >= 1"));   // 2^32 pixels
        sp.height = 65535; sp.min_samples = 1;
        CHECK(check_select_call(&sp, true, n_pix).code == PT_OK && plan_select(n_pix).n_blocks == (1u << 24) - 256);
        sp.height = -3;
        CHECK(says(check_select_call(&sp, true, n_pix), "width and height must be >= 1"));
        sp.height = 1;
        for (float bad : {-1.0f, inf, -inf, nan}) { sp.threshold = bad; CHECK(says(check_select_call(&sp, true, n_pix), "threshold must be finite")); }
        sp.threshold = 0.0f;
        CHECK(check_select_call(&sp, true, n_pix).code == PT_OK && n_pix == 65536 && plan_select(1).n_blocks == 1 && plan_select(257).n_blocks == 2);
    }

    // (g4) pt_tonemap and pt_meter: every rule broken alone and together (the first in the header's order answers), and the launches of calls that pass
    {
        const float inf = 1.0f / 0.0f * (float)(KERNELS[1] != 0), nan = inf - inf;
        auto says = [](const Refusal& r, const char* text) { return r.code != PT_OK && r.msg.find(text) != std::string::npos; };
        for (int broken = 0; broken < 64; broken++) {
            pt_tonemap_params tp = {};
            tp.width = 1920; tp.height = broken & 2 ? 0 : 1080; tp.curve = broken & 4 ? 3 : PT_TONE_REINHARD; tp.transfer = PT_XFER_SRGB;
            tp.exposure = broken & 8 ? 0.0f : 1.5f; tp.white = broken & 16 ? -1.0f : 4.0f;
            uint64_t n_pix = 0;
            const Refusal r = check_tonemap_call(broken & 32 ? nullptr : &tp, !(broken & 1), n_pix);
            CHECK((r.code == PT_OK) == !broken);
            if (broken) CHECK(turned_away(r));
            CHECK(says(r, broken & 33 ? "pt_tonemap: null argument" : broken & 2 ? "width and height must be >= 1" : broken & 4 ? "unknown curve or transfer"
                          : broken & 8 ? "exposure must be finite and > 0" : "white must be > 0") == (broken != 0));
            if (!broken) {
                n_planned++;
                const DisplayPlan v = plan_tonemap(n_pix, true), s = plan_tonemap(n_pix, false);
                CHECK(n_pix == 1920ull * 1080 && v.vec && v.items == n_pix / 4 && v.n_blocks == 2025 && !s.vec && s.items == n_pix && s.n_blocks == 8100);
            }
        }
        for (int broken = 0; broken < 128; broken++) {
            pt_meter_params mp = {};
            mp.width = broken & 2 ? -1 : 1920; mp.height = 1080; mp.key = broken & 4 ? 0.0f : 0.18f;
            mp.low_pct = 0.1f; mp.high_pct = broken & 8 ? 0.1f : 0.9f;
            mp.min_exposure = broken & 16 ? 4.0f : 0.25f; mp.max_exposure = 2.0f; mp.adapt = broken & 32 ? 1.5f : 0.25f;
            uint64_t n_pix = 0;
            const Refusal r = check_meter_call(broken & 64 ? nullptr : &mp, !(broken & 1), n_pix);
            CHECK((r.code == PT_OK) == !broken);
            if (broken) CHECK(turned_away(r));
            CHECK(says(r, broken & 65 ? "pt_meter: null argument" : broken & 2 ? "width and height must be >= 1" : broken & 4 ? "key must be finite and > 0"
                          : broken & 8 ? "0 <= low_pct < high_pct <= 1" : broken & 16 ? "0 < min_exposure <= max_exposure" : "adapt must be in 0..1") == (broken != 0));
            if (!broken) {
                n_planned++;
                const DisplayPlan v = plan_meter(n_pix, true), s = plan_meter(n_pix, false);
                CHECK(v.vec && v.items == n_pix / 4 && v.n_blocks == METER_BLOCKS && !s.vec && s.items == n_pix && s.n_blocks == METER_BLOCKS);
            }
        }
        // the values each rule turns away, and the ones at its edge that pass
        pt_tonemap_params tp = {};
        tp.width = tp.height = 65536; tp.curve = PT_TONE_CLAMP; tp.transfer = PT_XFER_LINEAR; tp.exposure = 1.0f; tp.white = nan;   // (white: not read under CLAMP)
        uint64_t n_pix = 0;
        CHECK(says(check_tonemap_call(&tp, true, n_pix), "width and height must be >= 1"));   // 2^32 pixels
        tp.height = 65535;
        CHECK(check_tonemap_call(&tp, true, n_pix).code == PT_OK && plan_tonemap(n_pix, true).n_blocks == (1u << 22) - 64 && plan_tonemap(n_pix, false).n_blocks == (1u << 24) - 256);
        tp.width = 37; tp.height = 23;
        CHECK(check_tonemap_call(&tp, true, n_pix).code == PT_OK && !plan_tonemap(n_pix, true).vec && plan_tonemap(n_pix, true).n_blocks == 4);
        for (int bad : {-1, 3}) {
            tp.curve = bad; CHECK(says(check_tonemap_call(&tp, true, n_pix), "unknown curve or transfer"));
            tp.curve = PT_TONE_ACES; tp.transfer = bad; CHECK(says(check_tonemap_call(&tp, true, n_pix), "unknown curve or transfer"));
            tp.transfer = PT_XFER_GAMMA22;
        }
        for (float bad : {0.0f, -1.0f, inf, -inf, nan}) { tp.exposure = bad; CHECK(says(check_tonemap_call(&tp, true, n_pix), "exposure must be finite and > 0")); }
        tp.exposure = 1e-30f; tp.curve = PT_TONE_REINHARD;
        for (float bad : {0.0f, -2.0f, -inf, nan}) { tp.white = bad; CHECK(says(check_tonemap_call(&tp, true, n_pix), "white must be > 0")); }
        tp.white = inf;
        CHECK(check_tonemap_call(&tp, true, n_pix).code == PT_OK && n_pix == 37 * 23);
        pt_meter_params mp = {};
        mp.width = 1; mp.height = 1; mp.key = 0.18f; mp.low_pct = 0.0f; mp.high_pct = 1.0f; mp.min_exposure = mp.max_exposure = 1.0f; mp.adapt = 0.0f;
        CHECK(check_meter_call(&mp, true, n_pix).code == PT_OK && n_pix == 1 && plan_meter(1, true).n_blocks == 1 && !plan_meter(1, true).vec);
        CHECK(plan_meter(257, false).n_blocks == 2 && plan_meter(65536, true).n_blocks == 256 && plan_meter(66000, false).n_blocks == 256 && plan_meter((1ull << 32) - 1, true).n_blocks == 256);
        CHECK(METER_SCRATCH_WORDS * 4 == 263168);
        for (float bad : {0.0f, -1.0f, inf, nan}) { mp.key = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "key must be finite and > 0")); }
        mp.key = 0.18f;
        for (float bad : {-0.1f, 1.0f, nan}) { mp.low_pct = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "0 <= low_pct < high_pct <= 1")); }
        mp.low_pct = 0.0f;
        for (float bad : {0.0f, 1.5f, nan}) { mp.high_pct = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "0 <= low_pct < high_pct <= 1")); }
        mp.high_pct = 1.0f;
        for (float bad : {0.0f, -1.0f, 2.0f, inf, nan}) { mp.min_exposure = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "0 < min_exposure <= max_exposure")); }
        mp.min_exposure = 1.0f;
        for (float bad : {0.5f, inf, nan}) { mp.max_exposure = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "0 < min_exposure <= max_exposure")); }
        mp.max_exposure = 1.0f;
        for (float bad : {-0.5f, 1.5f, nan}) { mp.adapt = bad; CHECK(says(check_meter_call(&mp, true, n_pix), "adapt must be in 0..1")); }
    }

    // (g5) pt_render_aux, pt_render_aux_camera, pt_denoise, pt_denoise_variance, the four reprojections and pt_frame_error: every rule broken alone and together
    // (the first in the header's order answers), a well-formed call passes, and the values each rule names.  The "device" pointers
    // are addresses of host words that nothing reads.
    {
        const float inf = 1.0f / 0.0f * (float)(KERNELS[1] != 0), nan = inf - inf;
        auto says = [](const Refusal& r, const char* text) { return r.code != PT_OK && r.msg.find(text) != std::string::npos; };
        // `rules`: (broken, text) in the header's order; the call must answer with the first broken one, or pass
        struct Rule { bool broken; const char* text; };
        auto first_answers = [&](const Refusal& r, std::initializer_list<Rule> rules) {
            for (const Rule& k : rules)
                if (k.broken) {
                    CHECK(turned_away(r));
                    CHECK(says(r, k.text));
                    return;
                }
            CHECK(r.code == PT_OK && !r.nothing && r.msg.empty());
        };
        static float mem[24];
        static int32_t ids[2];
        static uint32_t words[1];

        for (int broken = 0; broken < 32; broken++) {
            pt_params p = {};
            p.width = broken & 2 ? 0 : 37; p.height = 23;
            const CtxFacts f = scene(broken & 4 ? NO_TREE : broken & 8 ? TREE_WOOP : TREE, SPHERES[1], MATS[0], ENV_NONE);
            first_answers(check_aux_call(f, broken & 16 ? nullptr : &p, !(broken & 1)),
                          {{(broken & 17) != 0, "pt_render_aux: null argument"}, {(broken & 2) != 0, "pt_render_aux: width and height must be >= 1"},
                           {(broken & 4) != 0, "pt_render_aux: no BVH uploaded"}, {(broken & 8) != 0, "the binary walk reads Moller-Trumbore records"}});
        }
        // pt_render_aux_camera: the model's rules (the image is cm's; p's width and height are not read) between the pointers and the scene
        for (int broken = 0; broken < 512; broken++) {
            pt_params p = {};
            pt_camera_model cm = {};
            cm.model = broken & 2 ? 5 : PT_CAM_FISHEYE; cm.flags = broken & 4 ? 2 : PT_CAMF_CENTRE;
            cm.width = broken & 8 ? 1 : 37; cm.height = 23;
            cm.fisheye_fov = broken & 16 ? 7.0f : 3.0f;
            cm.lens_radius = -1.0f;   // another model's parameter: ignored
            const CtxFacts f = scene(broken & 32 ? NO_TREE : broken & 64 ? TREE_WOOP : TREE, SPHERES[1], MATS[0], ENV_NONE);
            first_answers(check_aux_camera_call(f, broken & 128 ? nullptr : &cm, broken & 256 ? nullptr : &p, !(broken & 1)),
                          {{(broken & (1 | 128 | 256)) != 0, "pt_render_aux_camera: null argument"}, {(broken & 2) != 0, "pt_render_aux_camera: unknown camera model"},
                           {(broken & 4) != 0, "pt_render_aux_camera: unknown flag bits"}, {(broken & 8) != 0, "pt_render_aux_camera: width and height must be >= 2"},
                           {(broken & 16) != 0, "pt_render_aux_camera: fisheye_fov must be in"}, {(broken & 32) != 0, "pt_render_aux_camera: no BVH uploaded"},
                           {(broken & 64) != 0, "pt_render_aux_camera: the binary walk reads Moller-Trumbore records"}});
        }
        for (int broken = 0; broken < 32; broken++) {
            pt_denoise_params dp = {};
            dp.width = broken & 2 ? 0 : 37; dp.height = 23; dp.iterations = broken & 4 ? 11 : 4;
            dp.sigma_color = 0.0f; dp.sigma_normal = broken & 8 ? nan : 1.0f; dp.sigma_position = 0.03f;
            first_answers(check_denoise_call(broken & 16 ? nullptr : &dp, !(broken & 1)),
                          {{(broken & 17) != 0, "pt_denoise: null argument"}, {(broken & 2) != 0, "pt_denoise: width and height must be >= 1"},
                           {(broken & 4) != 0, "pt_denoise: iterations must be 0..10"}, {(broken & 8) != 0, "pt_denoise: a sigma is not finite"}});
        }
        for (int broken = 0; broken < 256; broken++) {
            pt_denoise_variance_params dp = {};
            dp.width = 37; dp.height = broken & 2 ? 0 : 23; dp.iterations = broken & 4 ? -1 : 4;
            dp.sigma_luminance = broken & 8 ? inf : 4.0f; dp.sigma_normal = 1.0f; dp.sigma_position = 0.03f; dp.samples_per_frame = broken & 32 ? 0.5f : 4.0f;
            const VarianceBuffers b = {broken & 1 ? nullptr : &mem[0], broken & 16 ? nullptr : &mem[1], &mem[2], &mem[3], &mem[4], &mem[5], &mem[6], broken & 64 ? &mem[2] : &mem[7]};
            first_answers(check_denoise_variance_call(broken & 128 ? nullptr : &dp, b),
                          {{(broken & 129) != 0, "pt_denoise_variance: null argument"}, {(broken & 2) != 0, "pt_denoise_variance: width and height must be >= 1"},
                           {(broken & 4) != 0, "pt_denoise_variance: iterations must be 0..10"}, {(broken & 8) != 0, "pt_denoise_variance: a sigma is not finite"},
                           {(broken & 16) != 0, "pt_denoise_variance: null moments"}, {(broken & 32) != 0, "samples_per_frame must be finite and >= 1"},
                           {(broken & 64) != 0, "out_variance_dev may not be one of the inputs"}});
        }
        // the reprojections: bit 8192 takes the history away, and with it every rule behind the parameters'
        const struct { TemporalKind kind; const char* who; } CALLS[] = {{TEMPORAL_COLOUR, "pt_temporal"}, {TEMPORAL_MOTION, "pt_temporal_motion"}, {TEMPORAL_MOMENTS, "pt_temporal_moments"},
                                                                        {TEMPORAL_CAMERA, "pt_temporal_camera"}};
        static pt_camera_model model;   // pt_temporal_camera's: an equirectangular 37 x 23 image, as the parameters'
        auto well_formed = [&](TemporalKind kind, pt_temporal_params* tp, pt_camera* cam) {
            model = {};
            model.model = PT_CAM_EQUIRECT; model.width = 37; model.height = 23;
            tp->width = 37; tp->height = 23; tp->max_history = 32.0f; tp->plane_tolerance = 0.02f; tp->normal_threshold = 0.9f;
            TemporalCall a = {};
            a.kind = kind; a.tp = tp; a.prev_cam = cam;
            a.prev_color = &mem[0]; a.prev_length = &mem[1]; a.prev_normal = &mem[2]; a.prev_position = &mem[3]; a.prev_id = &ids[0];
            a.cur_color = &mem[4]; a.cur_normal = &mem[5]; a.cur_position = &mem[6]; a.cur_id = &ids[1];
            a.out_color = &mem[7];
            if (kind != TEMPORAL_MOMENTS) { a.out_length = &mem[8]; a.rgba = &words[0]; }
            if (kind != TEMPORAL_COLOUR) { a.prev_verts = &mem[9]; a.cur_verts = &mem[10]; a.n_tris = 5; }
            if (kind == TEMPORAL_MOTION || kind == TEMPORAL_CAMERA) a.motion = &mem[11];
            if (kind == TEMPORAL_CAMERA) a.prev_cm = &model;
            return a;
        };
        for (const auto& call : CALLS)
            for (int broken = 0; broken < 16384; broken++) {
                pt_temporal_params tp = {};
                pt_camera cam = {};
                TemporalCall a = well_formed(call.kind, &tp, &cam);
                const bool rows = call.kind != TEMPORAL_COLOUR, history = !(broken & 8192);
                if (broken & 1) a.cur_normal = nullptr;
                if (broken & 2) tp.width = 1;
                if (broken & 4) tp.max_history = 0.5f;
                if (broken & 8) tp.plane_tolerance = -1.0f;
                if (broken & 16) tp.normal_threshold = 2.0f;
                if (broken & 32) a.prev_normal = nullptr;
                if (broken & (64 | 256)) a.prev_id = nullptr;   // 64 alone: the ids of one frame; 256: of neither
                if (broken & 256) a.cur_id = nullptr;
                if (broken & 128) a.out_color = (float*)a.prev_color;
                if (broken & 512) a.prev_verts = nullptr;        // (the colour call has no rows: these three change nothing there)
                if (broken & 1024) a.n_tris = (size_t)1 << 31;
                const bool has_motion = call.kind == TEMPORAL_MOTION || call.kind == TEMPORAL_CAMERA;
                if (broken & 2048 && has_motion) a.motion = (float*)a.rgba;
                if (broken & 4096) a.tp = nullptr;
                if (!history) a.prev_color = nullptr;
                const std::string who = std::string(call.who) + ": ";
                const std::string t0 = who + "null argument", t1 = who + "width and height must be >= 2", t2 = who + "max_history must be finite and >= 1",
                                  t3 = who + "plane_tolerance must be finite and >= 0", t4 = who + "normal_threshold must be in -1..1",
                                  t5 = who + "a history needs its camera", t6 = who + "ids of both frames or of neither", t7 = who + "the new history may not overwrite",
                                  t8 = who + "the ids of both frames are required", t9 = who + "a null vertex buffer with n_tris > 0", t10 = who + "n_tris must be < 2^31",
                                  t11 = who + "motion_dev may not be one of the other buffers";
                first_answers(check_temporal_call(call.who, a),
                              {{(broken & (1 | 4096)) != 0, t0.c_str()}, {(broken & 2) != 0, t1.c_str()}, {(broken & 4) != 0, t2.c_str()}, {(broken & 8) != 0, t3.c_str()},
                               {(broken & 16) != 0, t4.c_str()}, {history && (broken & 32), t5.c_str()}, {history && (broken & 64) && !(broken & 256), t6.c_str()},
                               {history && (broken & 128), t7.c_str()}, {history && rows && (broken & 256), t8.c_str()}, {history && rows && (broken & 512), t9.c_str()},
                               {history && rows && (broken & 1024), t10.c_str()}, {history && has_motion && (broken & 2048), t11.c_str()}});
            }
        // pt_temporal_camera's own rules, between the history's pointers and the ids: a model, the model's rules, the parameters' image; without
        // rows the ids of neither frame pass and the motion buffer is still compared
        for (int broken = 0; broken < 512; broken++) {
            pt_temporal_params tp = {};
            pt_camera cam = {};
            TemporalCall a = well_formed(TEMPORAL_CAMERA, &tp, &cam);
            const bool history = !(broken & 256);
            if (broken & 1) a.prev_position = nullptr;
            if (broken & 2) a.prev_cm = nullptr;
            if (broken & 8) { model.model = PT_CAM_ORTHO; model.ortho_height = 0.0f; }
            if (broken & 4) model.model = -1;
            if (broken & 16) model.height = 24;
            if (broken & 32) a.prev_id = nullptr;
            if (broken & 64) { a.prev_verts = a.cur_verts = nullptr; a.n_tris = (size_t)1 << 40; }   // no rows: n_tris is ignored
            if (broken & 128) a.motion = (float*)a.cur_normal;
            if (!history) a.prev_color = nullptr;
            first_answers(check_temporal_call("pt_temporal_camera", a),
                          {{history && (broken & 1), "pt_temporal_camera: a history needs its camera, lengths"}, {history && (broken & 2), "pt_temporal_camera: a history needs the model of its camera"},
                           {history && (broken & 4), "pt_temporal_camera: unknown camera model"}, {history && (broken & 8) && !(broken & 4), "pt_temporal_camera: ortho_height must be finite"},
                           {history && (broken & 16), "pt_temporal_camera: the model's image must be the parameters'"}, {history && (broken & 32), "pt_temporal_camera: ids of both frames or of neither"},
                           {history && (broken & 128), "pt_temporal_camera: motion_dev may not be one of the other buffers"}});
        }
        {   // without rows the ids of neither frame pass; with rows they are required
            pt_temporal_params tp = {};
            pt_camera cam = {};
            TemporalCall a = well_formed(TEMPORAL_CAMERA, &tp, &cam);
            a.prev_id = a.cur_id = nullptr;
            CHECK(temporal_reads_rows(a) && says(check_temporal_call("pt_temporal_camera", a), "the ids of both frames are required"));
            a.prev_verts = a.cur_verts = nullptr;
            CHECK(!temporal_reads_rows(a) && check_temporal_call("pt_temporal_camera", a).code == PT_OK);
            a.cur_verts = &mem[10];   // one row buffer: rows are read, and both are needed
            a.prev_id = &ids[0]; a.cur_id = &ids[1];
            CHECK(temporal_reads_rows(a) && says(check_temporal_call("pt_temporal_camera", a), "a null vertex buffer with n_tris > 0"));
            for (int m = PT_CAM_PINHOLE; m <= PT_CAM_EQUIRECT; m++) {   // every model, with the parameters of the others out of range
                a = well_formed(TEMPORAL_CAMERA, &tp, &cam);
                model.model = m;
                model.lens_radius = m == PT_CAM_THIN_LENS ? 0.5f : -1.0f; model.focus_dist = m == PT_CAM_THIN_LENS ? 35.0f : 0.0f;
                model.ortho_height = m == PT_CAM_ORTHO ? 30.0f : -1.0f; model.fisheye_fov = m == PT_CAM_FISHEYE ? 6.28318548f : 9.0f;
                CHECK(check_temporal_call("pt_temporal_camera", a).code == PT_OK);
            }
        }
        for (int broken = 0; broken < 32; broken++) {
            uint64_t n_pix = 77;
            const Refusal r = check_frame_error_call(!(broken & 1), broken & 16 ? 65536 : 37, broken & 2 ? 0 : broken & 16 ? 65536 : 23, broken & 4 ? 1 : 16, broken & 8 ? nan : 0.1f, n_pix);
            first_answers(r, {{(broken & 1) != 0, "pt_frame_error: null argument"}, {(broken & 2) != 0, "pt_frame_error: width and height must be >= 1"},
                              {(broken & 4) != 0, "the standard error needs n_samples >= 2"}, {(broken & 8) != 0, "pt_frame_error: threshold must be finite and >= 0"},
                              {(broken & 16) != 0, "more than 2^32 - 1 pixels"}});
            if (!broken) CHECK(n_pix == 37 * 23);
        }
        // the values each rule turns away, and the ones at its edge that pass
        {
            pt_denoise_params dp = {};
            dp.width = dp.height = 1; dp.sigma_normal = -1.0f;   // (a sigma <= 0 switches its term off)
            for (int ok : {0, 10}) { dp.iterations = ok; CHECK(check_denoise_call(&dp, true).code == PT_OK); }
            for (int bad : {-1, 11}) { dp.iterations = bad; CHECK(says(check_denoise_call(&dp, true), "iterations must be 0..10")); }
            dp.iterations = 4;
            for (float bad : {inf, -inf, nan}) {
                for (float* s : {&dp.sigma_color, &dp.sigma_normal, &dp.sigma_position}) {
                    const float keep = *s;
                    *s = bad; CHECK(says(check_denoise_call(&dp, true), "a sigma is not finite"));
                    *s = keep;
                }
            }
            pt_denoise_variance_params dv = {};
            dv.width = dv.height = 1; dv.iterations = 10; dv.samples_per_frame = 1.0f;
            const VarianceBuffers b = {&mem[0], &mem[1], nullptr, &mem[3], &mem[4], &mem[5], &mem[0], nullptr};   // no length, no out_variance, out = color
            CHECK(check_denoise_variance_call(&dv, b).code == PT_OK);
            for (float bad : {inf, -inf, nan}) {
                for (float* s : {&dv.sigma_luminance, &dv.sigma_normal, &dv.sigma_position}) {
                    const float keep = *s;
                    *s = bad; CHECK(says(check_denoise_variance_call(&dv, b), "a sigma is not finite"));
                    *s = keep;
                }
            }
            for (float bad : {0.0f, 0.5f, -1.0f, inf, nan}) { dv.samples_per_frame = bad; CHECK(says(check_denoise_variance_call(&dv, b), "samples_per_frame must be finite and >= 1")); }
            dv.samples_per_frame = 1.0f;
            for (int k = 0; k < 6; k++) {   // out_variance on each input in turn; on out it is none of them
                VarianceBuffers v = {&mem[0], &mem[1], &mem[2], &mem[3], &mem[4], &mem[5], &mem[6], &mem[k]};
                CHECK(says(check_denoise_variance_call(&dv, v), "out_variance_dev may not be one of the inputs"));
                v.out_variance = v.out;
                CHECK(check_denoise_variance_call(&dv, v).code == PT_OK);
            }
            pt_temporal_params tp = {};
            pt_camera cam = {};
            for (const auto& call : CALLS) {
                TemporalCall a = well_formed(call.kind, &tp, &cam);
                tp.width = tp.height = 2; tp.max_history = 1.0f; tp.plane_tolerance = 0.0f;
                model.width = model.height = 2;
                for (float ok : {-1.0f, 1.0f}) { tp.normal_threshold = ok; CHECK(check_temporal_call(call.who, a).code == PT_OK); }
                for (float bad : {0.5f, -1.0f, inf, -inf, nan}) { tp.max_history = bad; CHECK(says(check_temporal_call(call.who, a), "max_history must be finite and >= 1")); }
                tp.max_history = 1.0f;
                for (float bad : {-0.5f, inf, -inf, nan}) { tp.plane_tolerance = bad; CHECK(says(check_temporal_call(call.who, a), "plane_tolerance must be finite and >= 0")); }
                tp.plane_tolerance = 0.0f;
                for (float bad : {-1.5f, 1.5f, inf, -inf, nan}) { tp.normal_threshold = bad; CHECK(says(check_temporal_call(call.who, a), "normal_threshold must be in -1..1")); }
                tp.normal_threshold = 0.9f;
                a.prev_cam = nullptr;
                CHECK(says(check_temporal_call(call.who, a), "a history needs its camera"));
                a.prev_cam = &cam;
                a.out_color = (float*)a.cur_color;   // in place over the current frame is allowed
                CHECK(check_temporal_call(call.who, a).code == PT_OK);
                if (call.kind != TEMPORAL_MOMENTS) {
                    a.out_length = (float*)a.prev_length;
                    CHECK(says(check_temporal_call(call.who, a), "the new history may not overwrite"));
                    a.out_length = &mem[8];
                }
                if (call.kind == TEMPORAL_COLOUR) {
                    a.prev_id = a.cur_id = nullptr;   // ids of neither frame
                    CHECK(check_temporal_call(call.who, a).code == PT_OK);
                    continue;
                }
                a.n_tris = ((size_t)1 << 31) - 1;
                CHECK(check_temporal_call(call.who, a).code == PT_OK);
                a.n_tris = 0; a.prev_verts = a.cur_verts;   // no rows at all, and one buffer for both
                CHECK(check_temporal_call(call.who, a).code == PT_OK);
                if (call.kind == TEMPORAL_MOMENTS) {
                    a.prev_verts = a.cur_verts = nullptr; a.prev_id = a.cur_id = nullptr;   // pt_temporal's rule: no rows, ids of neither
                    CHECK(!temporal_reads_rows(a) && check_temporal_call(call.who, a).code == PT_OK);
                    continue;
                }
                const void* const others[] = {a.prev_verts, a.prev_color, a.prev_length, a.prev_normal, a.prev_position, a.prev_id,
                                              a.cur_color, a.cur_normal, a.cur_position, a.cur_id, a.out_color, a.out_length, a.rgba};
                for (const void* o : others) { a.motion = (float*)o; CHECK(says(check_temporal_call(call.who, a), "motion_dev may not be one of the other buffers")); }
                a.prev_color = nullptr;   // without a history the motion buffer is not compared
                CHECK(check_temporal_call(call.who, a).code == PT_OK);
            }
            uint64_t n_pix = 0;
            for (float bad : {-1.0f, inf, -inf, nan}) CHECK(says(check_frame_error_call(true, 37, 23, 2, bad, n_pix), "threshold must be finite and >= 0"));
            CHECK(check_frame_error_call(true, 65537, 65535, 2, 0.0f, n_pix).code == PT_OK && n_pix == 0xffffffffull);   // 2^32 - 1 pixels
            CHECK(says(check_frame_error_call(true, 65536, 65536, 2, 0.0f, n_pix), "more than 2^32 - 1 pixels"));
            CHECK(says(check_frame_error_call(true, 37, -23, 2, 0.0f, n_pix), "width and height must be >= 1"));
        }
    }

    // (h) pt_closest_hits / pt_any_hits: the wide walk's two budgets, the binary walk for a tree too deep
    for (const Tree& t : {TREE, TREE_OCC, TREE_23, TREE_DEEP})
        for (int lstk : {0, 16, 24})
            for (int top : {0, 64, 1024})
                for (int any = 0; any < 2; any++)
                    for (uint64_t n : {1ull, 256ull, 257ull, (1ull << 32) - 1}) {
                        CtxFacts f = scene(t, SPHERES[0], MATS[0], ENV_NONE);
                        f.lstk = lstk; f.top = top;
                        const QueryPlan q = plan_query(f, n, any != 0);
                        n_planned++;
                        CHECK(q.lds <= PT_LDS_BYTES && q.n_regions >= 1 && (uint64_t)q.n_regions * PT_REGION >= n && q.wide == (t.wide_depth < 24));
                        if (q.wide) query.request(q.word);
                        else CHECK(q.n_top <= top && q.lds == (size_t)q.n_top * 64 + (size_t)PT_STACK_CAP * PT_BLOCK_RAYS * 4);
                    }

    for (const Family* fam : {&mega, &persist, &rays, &query, &extend, &shade, &last_any, &fused}) fam->report();
    std::printf("camera family %s: requests=%ld words=%d kernels=%d\n", camera.name, camera.requests, camera.words(), variant_count(camera.exists, camera.n_bits));
    std::printf("%ld plans, %ld refusals\n", n_planned, n_refused);
    for (const auto& e : REFUSALS)
        if (!e.seen && n_failed++ < 20) std::printf("FAILED: no call of the domain is refused with \"%s\"\n", e.text);
    // the budgets the words carry are the ones the requests asked for, or the nearest
    CHECK(budget_occ(mega_budget(6, 16)) == 8 && budget_occ(mega_budget(4, 16)) == 4 && budget_lstk(mega_budget(8, 72)) == 72);
    CHECK(persist_budget(ALG_WIDE, 5, 16) == BUDGET_6x16 && persist_budget(ALG_WIDE, 8, 24) == BUDGET_6x24 && persist_budget(ALG_UNIFIED, 4, 24) == BUDGET_8x16);
    CHECK(shade_env(ENV_LIGHT, false, false) == ENV_LOOKUP && shade_env(ENV_LOOKUP, true, true) == ENV_LIGHT && shade_env(ENV_LIGHT, true, false) == ENV_LIGHT);
    CHECK(env_code(false, false) == ENV_NONE && env_code(true, false) == ENV_LOOKUP && env_code(true, true) == ENV_LIGHT);
    for (int lp : {0, 1, 2, 4}) CHECK(ws_fold(ws_fold_field(lp)) == lp);
    if (n_failed) {
        std::printf("%d checks FAILED\n", n_failed);
        return 1;
    }
    std::printf("all checks hold\n");
    return 0;
}
