// ptmi.hip — C ABI of libptmi.so (include/ptmi.h): context, materials and spheres, launches.
// The kernels are in pt_kernels.h; the tree (pt_upload_bvh, pt_build_bvh) is pt_tree.hip's.
//
// Replaces BasicScene::launchKernel (GpuPathTracer/tracer.cu:405-415) and the device
// buffer set-up of GpuPathTracer/BasicScene.cpp:138-149,:214-215,:297-313.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pt_ctx.h"

static_assert(sizeof(pt_sphere) == 44, "pt_sphere must match the reference Sphere (44 B)");
static_assert(sizeof(pt_sphere_d) == sizeof(pt_sphere), "device sphere mirror");
static_assert(sizeof(pt_params) == 104 && sizeof(pt_camera) == 64 && sizeof(pt_counters) == 48, "ABI struct sizes (tests/test_host_and_abi.py)");

namespace ptmi {
thread_local std::string g_err;
}
using namespace ptmi;

namespace ptmi {
// PT_KERNEL_AUTO: reads the trials' events once they have all completed (wait = false: only if that needs no waiting) and decides
static bool auto_decide(pt_ctx* c, pt_ctx::AutoPick& a, bool wait) {
    using AP = pt_ctx::AutoPick;
    if (a.phase != AP::PENDING) return a.phase == AP::DECIDED;
    for (int t = 0; t < AP::TRIALS; t++) {
        const hipError_t e = wait ? hipEventSynchronize(a.e[2 * t + 1]) : hipEventQuery(a.e[2 * t + 1]);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }   // hipErrorNotReady is not an error of the call
    }
    float best[2] = {3.0e38f, 3.0e38f};
    bool ok = true;
    for (int t = 0; t < AP::TRIALS; t++) {
        float ms = 0.f;
        ok = ok && hipEventElapsedTime(&ms, a.e[2 * t], a.e[2 * t + 1]) == hipSuccess;
        best[t & 1] = std::min(best[t & 1], ms);
    }
    a.ms[0] = best[0]; a.ms[1] = best[1];
    a.choice = ok && a.ms[1] < a.ms[0] ? PT_KERNEL_WAVEFRONT : PT_KERNEL_PERSISTENT;
    a.phase = AP::DECIDED;
    bool wave_wanted = false;   // by any remembered configuration
    for (const AP& o : c->picks)
        if (o.key && (o.phase < AP::DECIDED || o.choice == PT_KERNEL_WAVEFRONT)) wave_wanted = true;
    if (!wave_wanted) c->d_wave.reset();   // the pipeline's path records (3 GB at 1080p x 16 spp) are not needed; the trials that used them are done
    return true;
}

int stage_mark(pt_ctx* c, int kind) {
    if (!c->opt_timing) return PT_OK;
    if (c->stage_used == c->stage_ev.size()) {
        Event e;
        HIP_TRY(c, e.ensure());
        c->stage_ev.push_back(std::move(e));
        c->stage_kind.push_back(0);
    }
    HIP_TRY(c, hipEventRecord(c->stage_ev[c->stage_used], c->stream));
    c->stage_kind[c->stage_used] = kind;   // kind of the work that ENDS at this event
    c->stage_used++;
    return PT_OK;
}

// What planning reads off the context: the one place that reads the tree's fields and the options for a plan (pt_plan.h)
CtxFacts ctx_facts(const pt_ctx* c) {
    const TreeState& t = c->tree;
    CtxFacts f = {};
    f.has_bvh = t.has_bvh; f.records_woop = t.records_woop;
    f.wide_depth = t.wide_depth; f.n_top_layout = t.n_top_layout; f.wide_top_layout = t.wide_top_layout; f.n_occ = t.n_occ;
    f.n_spheres = c->n_spheres;
    for (int i = 0; i < PT_KSPHERES; i++) f.sphere_mat[i] = c->h_spheres[i].mat;
    f.mat_table = c->mat.d_tri_matid.get() != nullptr; f.tri_emits = !c->mat.emissive_ids.empty();
    f.env = c->env.code(); f.n_cu = c->n_cu;
    f.kernel = c->opt_kernel; f.counters = c->opt_counters; f.timing = c->opt_timing; f.overlap = c->opt_overlap; f.sph_lds = c->opt_sph_lds;
    f.top = c->opt_top; f.occ = c->opt_occ; f.lstk = c->opt_lstk; f.walk = c->opt_walk; f.batch = c->opt_batch; f.refill = c->opt_refill;
    f.vote_node = c->opt_vote_node; f.vote_rec = c->opt_vote_rec; f.wave_batch = c->opt_wave_batch; f.wave_samples = c->opt_wave_samples;
    f.wave_blocks = c->opt_wave_blocks; f.first_walk = c->opt_first_walk; f.packet_stack = c->opt_packet_stack; f.fuse_stages = c->opt_fuse_stages;
    f.last_anyhit = c->opt_last_anyhit; f.root_cull = c->opt_root_cull; f.root_entry = c->opt_root_entry;
    f.last_occluders = c->opt_last_occluders; f.path_history = c->opt_path_history;
    return f;
}

// pt_set_option's table, one row per option: the member it sets, the values it takes and what a refused value is answered with.
// TRI_TEST, LEAF_MAX and OPTIMIZE take effect at the next pt_upload_bvh, ENV_LIGHT at the next pt_upload_environment.
struct OptionRow {
    enum Rule { FLAG, RANGE, SET };   // any value, kept as 0 / 1;  v[0]..v[1];  one of v[0..3] (a shorter set repeats its last value)
    int id;
    int pt_ctx::*field;
    Rule rule;
    int v[4];
    int code;
    const char* msg;
};
static const OptionRow OPTIONS[] = {
    {PT_OPT_KERNEL, &pt_ctx::opt_kernel, OptionRow::SET, {PT_KERNEL_AUTO, PT_KERNEL_MEGA_BVH2, PT_KERNEL_PERSISTENT, PT_KERNEL_WAVEFRONT}, PT_ERR_UNSUPPORTED, "pt_set_option: kernel variant not available in this build"},
    {PT_OPT_COUNTERS, &pt_ctx::opt_counters, OptionRow::FLAG, {}, PT_OK, ""},
    {PT_OPT_TIMING, &pt_ctx::opt_timing, OptionRow::FLAG, {}, PT_OK, ""},
    {PT_OPT_SPHERE_LDS, &pt_ctx::opt_sph_lds, OptionRow::FLAG, {}, PT_OK, ""},
    {PT_OPT_OVERLAP, &pt_ctx::opt_overlap, OptionRow::FLAG, {}, PT_OK, ""},
    {PT_OPT_TOP_NODES, &pt_ctx::opt_top, OptionRow::RANGE, {0, PT_MAX_TOP}, PT_ERR_INVALID, "pt_set_option: top nodes must be 0..1024"},
    {PT_OPT_OCCUPANCY, &pt_ctx::opt_occ, OptionRow::SET, {4, 5, 6, 8}, PT_ERR_INVALID, "pt_set_option: occupancy must be 4, 5 (runs as 6), 6 or 8 waves per SIMD"},
    {PT_OPT_TRI_TEST, &pt_ctx::opt_tri_test, OptionRow::RANGE, {0, 1}, PT_ERR_INVALID, "pt_set_option: tri test must be 0 (Moller-Trumbore) or 1 (Woop)"},
    {PT_OPT_LEAF_MAX, &pt_ctx::opt_leaf_max, OptionRow::RANGE, {0, 1024}, PT_ERR_INVALID, "pt_set_option: leaf_max must be 0 (keep) .. 1024"},
    {PT_OPT_WALK, &pt_ctx::opt_walk, OptionRow::SET, {0, 1, 2, 4}, PT_ERR_INVALID, "pt_set_option: walk must be 0 (while-while), 1 (unified-step), 2 (wide) or 4 (wide, postponed leaf)"},
    {PT_OPT_REBUILD, &pt_ctx::opt_rebuild, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: rebuild must be 0 (keep the hierarchy), 1 (re-cluster) or 2 (keep the cheaper tree)"},
    {PT_OPT_PRESPLIT, &pt_ctx::opt_presplit, OptionRow::RANGE, {0, 100000}, PT_ERR_INVALID, "pt_set_option: presplit must be 0 (off) .. 100000 (per cent of diag/sqrt(n))"},
    {PT_OPT_BUILD_ALGO, &pt_ctx::opt_build_algo, OptionRow::RANGE, {0, 1}, PT_ERR_INVALID, "pt_set_option: build algorithm must be 0 (LBVH) or 1 (PLOC)"},
    {PT_OPT_WAVE_BATCH, &pt_ctx::opt_wave_batch, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: wave batch must be 1..64"},
    {PT_OPT_VOTE_NODE, &pt_ctx::opt_vote_node, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: vote weight must be 1..64"},
    {PT_OPT_VOTE_REC, &pt_ctx::opt_vote_rec, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: vote weight must be 1..64"},
    {PT_OPT_OPTIMIZE, &pt_ctx::opt_optimize, OptionRow::RANGE, {0, 16}, PT_ERR_INVALID, "pt_set_option: optimize passes must be 0 (off) .. 16"},
    {PT_OPT_WAVE_SAMPLES, &pt_ctx::opt_wave_samples, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: wave samples must be 1 (one sample of a tile per wave) .. 64"},
    {PT_OPT_WAVE_BLOCKS, &pt_ctx::opt_wave_blocks, OptionRow::RANGE, {1, 8}, PT_ERR_INVALID, "pt_set_option: wave blocks must be 1..8 per CU"},
    {PT_OPT_LDS_STACK, &pt_ctx::opt_lstk, OptionRow::SET, {0, 16, 24, 24}, PT_ERR_INVALID, "pt_set_option: LDS stack must be 0 (all 72 entries in LDS), 16 or 24 entries"},
    {PT_OPT_REFILL, &pt_ctx::opt_refill, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: refill must be 1..64"},
    {PT_OPT_BATCH, &pt_ctx::opt_batch, OptionRow::RANGE, {1, 64}, PT_ERR_INVALID, "pt_set_option: batch must be 1..64"},
    {PT_OPT_FIRST_WALK, &pt_ctx::opt_first_walk, OptionRow::RANGE, {0, 1}, PT_ERR_INVALID, "pt_set_option: first walk must be 0 (per lane) or 1 (wave-wide packets)"},
    {PT_OPT_PACKET_STACK, &pt_ctx::opt_packet_stack, OptionRow::RANGE, {2, PT_PACKET_STACK_MAX}, PT_ERR_INVALID, "pt_set_option: packet stack must be 2..72 entries"},
    {PT_OPT_FUSE_STAGES, &pt_ctx::opt_fuse_stages, OptionRow::RANGE, {0, 1}, PT_ERR_INVALID, "pt_set_option: fuse stages must be 0 (separate launches) or 1"},
    {PT_OPT_LAST_ANYHIT, &pt_ctx::opt_last_anyhit, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: last any-hit must be 0 (off), 1 (product launches) or 2 (instrumented launches too)"},
    {PT_OPT_ROOT_CULL, &pt_ctx::opt_root_cull, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: root cull must be 0 (off), 1 (product launches) or 2 (instrumented launches too)"},
    {PT_OPT_ROOT_ENTRY, &pt_ctx::opt_root_entry, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: root entry must be 0 (off), 1 (product launches) or 2 (instrumented launches too)"},
    {PT_OPT_LAST_OCCLUDERS, &pt_ctx::opt_last_occluders, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: last occluders must be 0 (off), 1 (product launches) or 2 (instrumented launches too)"},
    {PT_OPT_ENV_LIGHT, &pt_ctx::opt_env_light, OptionRow::RANGE, {0, 1}, PT_ERR_INVALID, "pt_set_option: env light must be 0 (the map is no light) or 1 (sampled under PT_FLAG_NEE)"},
    {PT_OPT_PATH_HISTORY, &pt_ctx::opt_path_history, OptionRow::RANGE, {0, 2}, PT_ERR_INVALID, "pt_set_option: path history must be 0 (off), 1 (product launches) or 2 (instrumented launches too)"},
};
}  // namespace ptmi

extern "C" {

int pt_abi_version(void) { return PTMI_ABI_VERSION; }

int pt_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return PT_ERR_DEVICE; }
    return n;
}

const char* pt_last_error(const pt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int pt_create(int device, pt_ctx** out) {
    if (!out) return fail(nullptr, PT_ERR_INVALID, "pt_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceCount");
    if (device < 0 || device >= n) return fail(nullptr, PT_ERR_INVALID, "pt_create: no such device");
    if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");
    std::unique_ptr<pt_ctx> c(new pt_ctx());   // a failure below releases whatever the context holds by then
    c->device = device;
    if ((e = c->own_stream.create(hipStreamNonBlocking)) != hipSuccess) return hip_fail(nullptr, e, "pt_create: the context's own stream");
    c->stream = c->own_stream;
    if ((e = c->d_counters.alloc(PT_CNT_N)) != hipSuccess) return hip_fail(nullptr, e, "pt_create: counters");
    if ((e = hipMemset(c->d_counters.get(), 0, c->d_counters.bytes())) != hipSuccess) return hip_fail(nullptr, e, "hipMemset");
    if ((e = c->d_queue.alloc(QUEUE_WORDS)) != hipSuccess) return hip_fail(nullptr, e, "pt_create: work counters");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    c->n_cu = prop.multiProcessorCount;
    if ((e = c->ev0.ensure()) != hipSuccess || (e = c->ev1.ensure()) != hipSuccess) return hip_fail(nullptr, e, "pt_create: timing events");
    *out = c.release();
    return PT_OK;
}

int pt_destroy(pt_ctx* c) {
    if (!c) return PT_OK;
    (void)hipSetDevice(c->device);
    (void)quiesce(c);   // every stream is idle before the first free
    delete c;           // the members release what they own (pt_own.h)
    return PT_OK;
}

int pt_set_stream(pt_ctx* c, void* s) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    hipStream_t next = s ? (hipStream_t)s : c->own_stream;
    if (next != c->stream) {
        // The context's scratch (sample buffers, path records, queue and work counters, the light list, a refit tree) is written by the
        // calls on whichever stream is current, and a side stream's fold waits on the stream it was issued on: what the new stream is
        // given starts behind everything the old one has been given.  No host synchronisation.
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->switch_ev.ensure(hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->switch_ev, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(next, c->switch_ev, 0));
    }
    c->stream = next;
    return PT_OK;
}

int pt_set_option(pt_ctx* c, int option, int value) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    for (const OptionRow& o : OPTIONS) {
        if (o.id != option) continue;
        bool ok = true;
        if (o.rule == OptionRow::RANGE) ok = value >= o.v[0] && value <= o.v[1];
        if (o.rule == OptionRow::SET) ok = std::find(o.v, o.v + 4, value) != o.v + 4;
        if (!ok) return fail(c, o.code, o.msg);
        c->*o.field = o.rule == OptionRow::FLAG ? value != 0 : value;
        return PT_OK;
    }
    return fail(c, PT_ERR_INVALID, "pt_set_option: unknown option");
}

int pt_sync(pt_ctx* c) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

int pt_malloc(pt_ctx* c, size_t bytes, void** out) {
    if (!c || !out || bytes == 0) return fail(c, PT_ERR_INVALID, "pt_malloc: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, device_alloc(out, bytes));
    return PT_OK;
}
int pt_free(pt_ctx* c, void* p) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, device_free(p));
    return PT_OK;
}
int pt_memset(pt_ctx* c, void* p, int v, size_t bytes) {
    if (!c || !p) return fail(c, PT_ERR_INVALID, "pt_memset: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(p, v, bytes, c->stream));
    return PT_OK;
}
int pt_download(pt_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(c, PT_ERR_INVALID, "pt_download: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}
int pt_upload(pt_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(c, PT_ERR_INVALID, "pt_upload: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// the table and the light list of a pt_upload_tri_materials call (n_materials > 0) into `m`, the context untouched
static int make_materials(pt_ctx* c, const pt_material* table, size_t n_materials, const int32_t* tri_material, size_t n_tris, Materials& m) {
    if (!table || !tri_material) return fail(c, PT_ERR_INVALID, "pt_upload_tri_materials: null array");
    if (n_materials > (1u << 24) || n_tris >= (size_t)0x7fffffff) return fail(c, PT_ERR_INVALID, "pt_upload_tri_materials: table too large");
    if (c->tree.has_bvh && (size_t)c->tree.max_tri_id >= n_tris && c->tree.max_tri_id >= 0)
        return fail(c, PT_ERR_INVALID, "pt_upload_tri_materials: n_tris does not cover the triangle ids of the uploaded BVH");
    for (size_t i = 0; i < n_materials; i++)
        if (table[i].mat < PT_MAT_DIFF || table[i].mat > PT_MAT_REFR) return fail(c, PT_ERR_INVALID, "pt_upload_tri_materials: bad material type");
    for (size_t i = 0; i < n_tris; i++)
        if (tri_material[i] < 0 || (size_t)tri_material[i] >= n_materials) return fail(c, PT_ERR_INVALID, "pt_upload_tri_materials: material index out of range");
    static_assert(sizeof(pt_material) == 32, "pt_material is two float4 rows");
    HIP_TRY(c, m.d_tri_matid.alloc(n_tris));
    HIP_TRY(c, m.d_mat_table.alloc(2 * n_materials));
    HIP_TRY(c, hipMemcpy(m.d_tri_matid.get(), tri_material, n_tris * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(m.d_mat_table.get(), table, n_materials * sizeof(pt_material), hipMemcpyHostToDevice));
    m.n_tri_matid = n_tris;
    // PT_FLAG_NEE: the triangles that emit, in id order, and where each one's light record goes
    std::vector<int32_t> slot(n_tris, -1);
    for (size_t i = 0; i < n_tris; i++) {
        const pt_material& row = table[tri_material[i]];
        if (!(row.emi[0] == 0.0f && row.emi[1] == 0.0f && row.emi[2] == 0.0f)) {
            slot[i] = (int32_t)m.emissive_ids.size();
            m.emissive_ids.push_back((int32_t)i);
        }
    }
    if (!m.emissive_ids.empty()) {
        HIP_TRY(c, m.d_light_slot.alloc(n_tris));
        HIP_TRY(c, m.d_tri_lights.alloc(m.emissive_ids.size() * 3));
        HIP_TRY(c, hipMemcpy(m.d_light_slot.get(), slot.data(), n_tris * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return PT_OK;
}

int pt_upload_tri_materials(pt_ctx* c, const pt_material* table, size_t n_materials, const int32_t* tri_material, size_t n_tris) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    HIP_TRY(c, hipSetDevice(c->device));
    Materials m;   // filled here, adopted at the end: a failure on the way leaves the context's table, light list and mat_gen as they were
    if (n_materials > 0) {
        const int rc = make_materials(c, table, n_materials, tri_material, n_tris, m);
        if (rc != PT_OK) return rc;
    }   // (else empty: back to the one global material of pt_params)
    HIP_TRY(c, quiesce(c));   // nothing in flight reads the old table or light list
    c->mat = std::move(m);
    c->mat_gen++;
    return PT_OK;
}

// PT_FLAG_NEE: copies (v0, e1, e2) of every emissive triangle from its record into its light slot (a triangle a spatial
// split lists more than once is listed in full each time: the copies write the same values)
__global__ void __launch_bounds__(256) k_collect_tri_lights(const float4* __restrict__ rec, uint32_t n_rec, const int32_t* __restrict__ slot,
                                                            uint32_t n_ids, const int* __restrict__ tri_matid, const float4* __restrict__ mat_table,
                                                            float4* __restrict__ lights) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rec) return;
    const float4 q0 = rec[4 * (size_t)i];
    const int id = __float_as_int(q0.w);
    if (id < 0 || (uint32_t)id >= n_ids) return;
    const int s = slot[id];
    if (s < 0) return;
    const float4 q1 = rec[4 * (size_t)i + 1], q2 = rec[4 * (size_t)i + 2];
    const int row = tri_matid[id];
    const float4 m0 = mat_table[2 * row], m1 = mat_table[2 * row + 1];
    lights[3 * (size_t)s + 0] = make_float4(q0.x, q0.y, q0.z, m0.w);
    lights[3 * (size_t)s + 1] = make_float4(q1.x, q1.y, q1.z, m1.x);
    lights[3 * (size_t)s + 2] = make_float4(q2.x, q2.y, q2.z, m1.y);
}

int pt_upload_spheres(pt_ctx* c, const pt_sphere* spheres, size_t n) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (n > 0 && !spheres) return fail(c, PT_ERR_INVALID, "pt_upload_spheres: null array");
    if (n > 4096) return fail(c, PT_ERR_INVALID, "pt_upload_spheres: too many spheres");
    for (size_t i = 0; i < n; i++)
        if (spheres[i].mat < PT_MAT_DIFF || spheres[i].mat > PT_MAT_REFR) return fail(c, PT_ERR_INVALID, "pt_upload_spheres: bad material");
    HIP_TRY(c, hipSetDevice(c->device));
    pt_ctx::DevBuf<pt_sphere_d> fresh;   // complete before the old set is touched
    HIP_TRY(c, fresh.alloc(n));
    if (n) HIP_TRY(c, hipMemcpy(fresh.get(), spheres, n * sizeof(pt_sphere), hipMemcpyHostToDevice));
    HIP_TRY(c, quiesce(c));   // nothing in flight reads the old spheres
    c->d_spheres = std::move(fresh);
    c->n_spheres = (int)n;
    if (n) std::memcpy(c->h_spheres, spheres, std::min<size_t>(n, PT_KSPHERES) * sizeof(pt_sphere));
    return PT_OK;
}

// ---------------------------------------------------------------------------------------
// pt_render in steps, in the order pt_render_moments runs them: gather the facts (ctx_facts, CallFacts), check the arguments, bring the
// light list up to date, fill the kernel arguments, PLAN the call (pt_plan.h: every decision about what runs and with which buffers,
// made once; plan_call asks the runtime what the plan's steps need to know), take the buffers the plan asks for, launch.
namespace ptmi {
// the scene, its geometry (pt_refit_bvh) or the materials changed: copies the lights' vertices out of the records again
static int refresh_tri_lights(pt_ctx* c, const CtxFacts& f, const pt_params* p) {
    if (!samples_tri_lights(f, p->flags)) return PT_OK;
    const Refusal r = tri_lights_rule(f, p->flags);
    if (r.code != PT_OK) return fail(c, r);
    const uint64_t key = (c->scene_gen << 32) ^ c->mat_gen;
    if (c->lights_key == key && c->lights_geom == c->geom_gen) return PT_OK;
    const uint32_t n_rec = (uint32_t)c->tree.n_refs;
    HIP_TRY(c, hipMemsetAsync(c->mat.d_tri_lights.get(), 0, c->mat.d_tri_lights.bytes(), c->stream));
    hipLaunchKernelGGL(k_collect_tri_lights, dim3((n_rec + 255) / 256), dim3(256), 0, c->stream, c->tree.d_nodes + 4 * (size_t)c->tree.n_inner, n_rec,
                       c->mat.d_light_slot.get(), (uint32_t)c->mat.n_tri_matid, c->mat.d_tri_matid.get(), c->mat.d_mat_table.get(), c->mat.d_tri_lights.get());
    HIP_TRY(c, hipGetLastError());
    c->lights_key = key;
    c->lights_geom = c->geom_gen;
    // a path kernel on a side stream (PT_OPT_OVERLAP) must not read the list before it is written
    HIP_TRY(c, c->lights_ev.ensure(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->lights_ev, c->stream));
    c->lights_gen++;
    return PT_OK;
}

// the kernel arguments that the context and pt_params give to any path kernel, a frame's or a ray batch's; zeroes the rest
static void fill_path_params(const pt_ctx* c, const CtxFacts& f, const pt_params* p, uint32_t spp, KParams& P) {
    std::memset(&P, 0, sizeof P);
    scene_view(c, P.sc, P.ksph);
    P.counters = c->d_counters.get();
    P.W = p->width; P.H = p->height;
    P.depth = p->depth;
    P.cull = p->cull_backfaces;
    P.frame = p->frame; P.sample_index = p->sample_index; P.spp = spp;
    P.tri_mat = p->tri_mat;
    for (int i = 0; i < 3; i++) { P.tri_col[i] = p->tri_col[i]; P.tri_emi[i] = p->tri_emi[i]; P.bk[i] = p->bk_color[i]; }
    P.air_ior = p->air_ior; P.glass_ior = p->glass_ior; P.phong = p->phong_expo;
    P.tri_matid = c->mat.d_tri_matid.get();
    P.mat_table = c->mat.d_mat_table.get();
    P.flags = p->flags;
    if (samples_tri_lights(f, p->flags)) {
        P.tri_lights = c->mat.d_tri_lights.get();
        P.n_tri_lights = (int)c->mat.emissive_ids.size();
    }
    pt_set_env(P, c->env.k);   // (all zero without a map; with one the stage-split pipeline, which writes wf over these bytes, is never chosen)
}

// the kernel arguments that the context and the call's arguments give; what the plan decides (samples, LDS layout, queue) is added
// by apply_plan
static void fill_params(const pt_ctx* c, const CtxFacts& f, float* accum_dev, uint32_t* rgba_dev, const pt_camera* cam, const pt_params* p, uint32_t spp, const TileGrid& g, KParams& P) {
    fill_path_params(c, f, p, spp, P);
    P.accum = accum_dev;
    P.rgba = rgba_dev;
    P.cam = *cam;
    P.smp_ss = (unsigned long long)p->width * (unsigned long long)p->height;   // one sample per pixel, or sample planes (plan.sgroup_log2 = 0)
    P.smp_ps = 1u;
    P.tiles_x = g.tiles_x; P.tile_rows = g.tile_rows; P.n_tiles = g.n_tiles;
    P.part_index = g.part_index; P.part_count = g.part_count; P.stripe_tr = g.stripe_tr;
}

// PT_KERNEL_AUTO: the entry of the call's configuration in the table of picks (a new configuration takes the least recently used one) and
// what this call is to it.  probe = 0..3: the timed trial of that number (even: the persistent kernel, odd: the pipeline), and the trial is
// consumed here; -1: no trial, the call runs pick->choice once the trials' events have been read and the persistent kernel until then.
static int auto_lookup(pt_ctx* c, const pt_params* p, uint32_t spp, bool moments, pt_ctx::AutoPick*& pick, int& probe) {
    using AP = pt_ctx::AutoPick;
    // the key holds the SHAPE of the partition, not which part this call renders: the parts of a tile split cost alike
    // mat_gen: a material table decides what the pipeline launches (the last segment's any-hit query and the path history need "no table")
    uint64_t key = 0xcbf29ce484222325ull;
    const uint64_t parts[] = {(uint64_t)p->width, (uint64_t)p->height, (uint64_t)spp, (uint64_t)p->depth,
                              (uint64_t)(p->part_count > 1 ? p->part_count : 1), (uint64_t)(p->part_count > 1 ? p->part_rows : 0), c->scene_gen,
                              (uint64_t)c->n_spheres, (uint64_t)p->tri_mat, (uint64_t)(p->flags & ~(uint32_t)PT_FLAG_WRITE_RGBA),
                              (uint64_t)moments, c->env_gen, c->mat_gen};   // with moments the pipeline keeps its separate fold and one sample goes through the sample buffer: other trial times
    for (uint64_t v : parts) { key ^= v; key *= 0x100000001b3ull; }
    if (key == 0) key = 1;
    int slot = -1, lru = 0;
    for (int i = 0; i < pt_ctx::N_PICKS; i++) {
        if (c->picks[i].key == key) { slot = i; break; }
        if (c->picks[i].used < c->picks[lru].used) lru = i;
    }
    if (slot < 0) {
        slot = lru;
        AP& n = c->picks[slot];
        if (n.phase > 0 && n.phase < AP::DECIDED)   // trials of the configuration it held may still be in flight: its events must be idle
            for (const Event& e : n.e) if (e) (void)hipEventSynchronize(e);
        n.key = key; n.phase = 0; n.choice = PT_KERNEL_PERSISTENT; n.ms[0] = n.ms[1] = 0.f;
    }
    AP& a = c->picks[slot];
    a.used = ++c->pick_tick;
    c->pick_last = slot;
    pick = &a;
    probe = -1;
    (void)auto_decide(c, a, false);   // all trials queued: decide once their events have completed, never wait for them
    if (a.phase < AP::TRIALS) {
        for (Event& e : a.e) HIP_TRY(c, e.ensure());
        probe = a.phase++;   // (counted here, before the call's later steps, which can still fail: a trial that never ran stays counted)
    }
    return PT_OK;
}

// The plan of a frame call (CallPlan, pt_plan.h), its steps in order with the runtime's answers between them: PT_KERNEL_AUTO's table
// where the plan looks the configuration up, whether the caller's stream is idle where the plan wants to know
static int plan_call(pt_ctx* c, const CtxFacts& f, const CallFacts& a, int n_tiles, CallPlan& plan, pt_ctx::AutoPick*& pick) {
    Refusal r = plan_walk(f, a, plan);
    if (r.code != PT_OK) return fail(c, r);
    AutoAnswer au = {-1, false, PT_KERNEL_PERSISTENT};
    pick = nullptr;
    if (plan.lookup) {
        const int rc = auto_lookup(c, a.p, a.spp, a.moments, pick, au.probe);
        if (rc != PT_OK) return rc;
        au.decided = pick->phase == pt_ctx::AutoPick::DECIDED;
        au.choice = pick->choice;
    }
    plan_family(f, a, au, plan);
    bool caller_idle = false;
    if (plan.idle_query) {
        caller_idle = hipStreamQuery(c->stream) == hipSuccess;
        if (!caller_idle) (void)hipGetLastError();   // hipErrorNotReady is not an error of this call
    }
    r = plan_launch(f, a, n_tiles, caller_idle, plan);
    return r.code != PT_OK ? fail(c, r) : PT_OK;
}

// the next side slot; its stream, events and queue counters are made on first use
static int side_acquire(pt_ctx* c, pt_ctx::Side*& sd) {
    sd = &c->side[c->side_next];
    c->side_next ^= 1;   // (flipped before the creations below can fail: the slot's next turn makes what is still missing)
    // a priority of its own: ROCm maps the streams of one priority onto a few hardware queues round-robin (four
    // by default, GPU_MAX_HW_QUEUES), and a side stream that shares a hardware queue with the caller's stream or
    // with the other side stream runs in order behind it — no overlap and a 5-9 % LOSS (measured with a second
    // context alive).  The high-priority class has queues of its own.
    if (!sd->stream) {
        int prio_lo = 0, prio_hi = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIP_TRY(c, sd->stream.create(hipStreamNonBlocking, prio_hi));
    }
    HIP_TRY(c, sd->traced.ensure(hipEventDisableTiming));
    HIP_TRY(c, sd->folded.ensure(hipEventDisableTiming));
    HIP_TRY(c, sd->queue.reserve(QUEUE_WORDS));
    return PT_OK;
}

// the sample buffer of the call, the side slot's own or the context's, grown to `need` floats
static int samples_reserve(pt_ctx* c, pt_ctx::Side* sd, size_t need, KParams& P) {
    pt_ctx::DevBuf<float>& buf = sd ? sd->samples : c->d_samples;
    if (need > buf.count()) HIP_TRY(c, hipStreamSynchronize(c->stream));   // every path kernel has a fold behind it on this stream
    HIP_TRY(c, buf.reserve(need));
    P.samples = buf.get();
    return PT_OK;
}

// the side stream's path kernel may start once the caller's earlier work has been SUBMITTED and needs the scene only, but it must not
// overwrite its sample buffer before the fold that last read it is done, nor read a light list or a refit tree still being written
static int side_order(pt_ctx* c, pt_ctx::Side* sd, bool reads_lights) {
    if (sd->fold_pending) HIP_TRY(c, hipStreamWaitEvent(sd->stream, sd->folded, 0));
    if (reads_lights && sd->lights_seen != c->lights_gen) {   // the light list was (re)written on the caller's stream
        HIP_TRY(c, hipStreamWaitEvent(sd->stream, c->lights_ev, 0));
        sd->lights_seen = c->lights_gen;
    }
    if (sd->geom_seen != c->geom_gen) {   // the tree was refit on the caller's stream (pt_refit_bvh)
        HIP_TRY(c, hipStreamWaitEvent(sd->stream, c->geom_ev, 0));
        sd->geom_seen = c->geom_gen;
    }
    return PT_OK;
}

// the plan's share of the kernel arguments: where the samples go, the LDS layout, the persistent kernel's queue
static void apply_plan(const pt_ctx* c, const CallPlan& plan, const pt_ctx::Side* sd, KParams& P) {
    P.sgroup_log2 = plan.sgroup_log2;
    if (plan.sgroup_log2) {
        P.smp_ss = 1ull;
        P.smp_ps = P.spp;
    }
    P.sc.stack_n = plan.L.lstk;
    P.sc.top_base = plan.L.walk >= 2 ? P.sc.wide_root : 0;
    P.sc.n_top = plan.n_top;
    P.sph_tab = plan.sph_tab;
    P.chunk = plan.chunk;
    if (plan.kernel == PT_KERNEL_PERSISTENT) queue_params(plan.q, sd ? sd->queue.get() : c->d_queue.get(), P);
}
}  // namespace ptmi

int pt_render(pt_ctx* c, float* accum_dev, uint32_t* rgba_dev, const pt_camera* cam, const pt_params* p, uint32_t spp) {
    return pt_render_moments(c, accum_dev, rgba_dev, nullptr, cam, p, spp);
}

// pt_render's body; moments_dev != NULL: the fold also keeps the luminance moments of the samples
int pt_render_moments(pt_ctx* c, float* accum_dev, uint32_t* rgba_dev, float* moments_dev, const pt_camera* cam, const pt_params* p,
                      uint32_t spp) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    const CallFacts a = {true, p, spp, accum_dev && cam, rgba_dev != nullptr, moments_dev != nullptr, 0, 0};
    Refusal r = check_path_call(f, a);
    if (r.code != PT_OK) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = refresh_tri_lights(c, f, p);
    if (rc != PT_OK) return rc;
    TileGrid g;
    r = frame_tiles(*p, spp, g);
    if (r.code != PT_OK || r.nothing) return fail(c, r);
    KParams P;
    fill_params(c, f, accum_dev, rgba_dev, cam, p, spp, g, P);
    CallPlan plan;
    pt_ctx::AutoPick* pick = nullptr;
    if ((rc = plan_call(c, f, a, g.n_tiles, plan, pick)) != PT_OK) return rc;
    const int probe = plan.probe;

    // the buffers the plan asks for
    pt_ctx::Side* sd = nullptr;
    if (plan.side && (rc = side_acquire(c, sd)) != PT_OK) return rc;
    if (plan.samples && (rc = samples_reserve(c, sd, (size_t)spp * (size_t)p->width * (size_t)p->height * 3, P)) != PT_OK) return rc;
    if (sd && (rc = side_order(c, sd, P.tri_lights != nullptr)) != PT_OK) return rc;
    hipStream_t trace_stream = sd ? (hipStream_t)sd->stream : c->stream;   // the stream the path kernel runs on
    apply_plan(c, plan, sd, P);

    if (plan.L.count) HIP_TRY(c, hipMemsetAsync(c->d_counters.get(), 0, c->d_counters.bytes(), c->stream));
    if (probe >= 0 && (probe & 1) && (rc = wave_reserve(c, plan.wl)) != PT_OK) return rc;   // a trial of the pipeline: its path records are allocated BEFORE the timed span
    if (probe >= 0) HIP_TRY(c, hipEventRecord(pick->e[2 * probe], c->stream));
    HIP_TRY(c, span_begin(c));
    if (f.timing) {
        c->stage_used = 0;
        if (stage_mark(c, PT_STAGE_NONE) != PT_OK) return PT_ERR_DEVICE;
    }
    const bool folded = plan.kernel == PT_KERNEL_WAVEFRONT && plan.wave.fold_lp != 0;   // (PT_OPT_FUSE_STAGES: in the last shade launch)
    if (plan.kernel == PT_KERNEL_WAVEFRONT) {
        if ((rc = render_wavefront(c, P, plan)) != PT_OK) return rc;
    } else if (plan.kernel == PT_KERNEL_PERSISTENT) {
        HIP_TRY(c, queue_reset(P.queue, trace_stream));
        HIP_TRY(c, launch_persist(plan.L, P, trace_stream));
        if (stage_mark(c, PT_STAGE_FRAME) != PT_OK) return PT_ERR_DEVICE;
    } else {
        HIP_TRY(c, launch_mega(plan.L, P, trace_stream));
        if (stage_mark(c, PT_STAGE_FRAME) != PT_OK) return PT_ERR_DEVICE;
    }
    if (sd) {   // the fold (accumulator, display words) waits for the path kernel on the caller's stream
        HIP_TRY(c, hipEventRecord(sd->traced, sd->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, sd->traced, 0));
    }
    if (P.samples && !folded) {
        HIP_TRY(c, launch_fold(P, (float2*)moments_dev, c->stream));
        if (stage_mark(c, PT_STAGE_FOLD) != PT_OK) return PT_ERR_DEVICE;
    }
    if (sd) {
        HIP_TRY(c, hipEventRecord(sd->folded, c->stream));
        sd->fold_pending = true;
    }
    if (probe >= 0) HIP_TRY(c, hipEventRecord(pick->e[2 * probe + 1], c->stream));
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

int pt_auto_choice(pt_ctx* c, int* kernel, float* ms_persistent, float* ms_wavefront) {
    if (!c || !kernel) return fail(c, PT_ERR_INVALID, "pt_auto_choice: null argument");
    *kernel = PT_KERNEL_AUTO;
    if (ms_persistent) *ms_persistent = 0.f;
    if (ms_wavefront) *ms_wavefront = 0.f;
    if (c->pick_last < 0) return PT_OK;
    pt_ctx::AutoPick& a = c->picks[c->pick_last];
    if (auto_decide(c, a, true)) *kernel = a.choice;   // the caller asks: waiting for the trials is fine here
    if (ms_persistent) *ms_persistent = a.ms[0];
    if (ms_wavefront) *ms_wavefront = a.ms[1];
    return PT_OK;
}

int pt_trace_rays(pt_ctx* c, const float* rays_dev, size_t n, int cull, float* t_dev, int32_t* tri_dev, float* normal_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    if (!f.has_bvh) return fail(c, PT_ERR_NO_SCENE, "pt_trace_rays: no BVH uploaded");
    if (f.records_woop) return fail(c, PT_ERR_UNSUPPORTED, "pt_trace_rays: the ray-batch kernel reads Moller-Trumbore records (upload with PT_OPT_TRI_TEST 0)");
    if (n == 0) return PT_OK;
    if (!rays_dev || !t_dev || !tri_dev) return fail(c, PT_ERR_INVALID, "pt_trace_rays: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    KScene sc;
    scene_view(c, sc);
    HIP_TRY(c, span_begin(c));
    const size_t lds = binary_ray_layout(f, sc);
    HIP_TRY(c, launch_rays(sc, lds, (const float4*)rays_dev, n, cull, t_dev, tri_dev, normal_dev, c->stream));
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

// the checks pt_closest_hits and pt_any_hits share, in pt_trace_rays' order; `outputs`: every required output pointer is given
static int query_call(pt_ctx* c, const char* who, bool outputs, const ptmi::QueryCall& q) {
    const std::string name(who);
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    if (!f.has_bvh) return fail(c, PT_ERR_NO_SCENE, name + ": no BVH uploaded");
    if (f.records_woop) return fail(c, PT_ERR_UNSUPPORTED, name + ": ray-batch queries read Moller-Trumbore records (upload with PT_OPT_TRI_TEST 0)");
    if (q.n == 0) return PT_OK;
    if (!q.rays || !outputs) return fail(c, PT_ERR_INVALID, name + ": null argument");
    if (q.n >= (1ull << 32)) return fail(c, PT_ERR_INVALID, name + ": more than 2^32 - 1 rays in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, span_begin(c));
    HIP_TRY(c, launch_query(c, plan_query(f, q.n, q.hit != nullptr), q));
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

int pt_closest_hits(pt_ctx* c, const float* rays_dev, size_t n, int cull, float* t_dev, int32_t* tri_dev, float* normal_dev) {
    return query_call(c, "pt_closest_hits", t_dev && tri_dev, ptmi::QueryCall{rays_dev, n, cull, t_dev, tri_dev, normal_dev, nullptr});
}

int pt_any_hits(pt_ctx* c, const float* rays_dev, size_t n, int cull, uint8_t* hit_dev) {
    return query_call(c, "pt_any_hits", hit_dev != nullptr, ptmi::QueryCall{rays_dev, n, cull, nullptr, nullptr, nullptr, hit_dev});
}

int pt_render_rays(pt_ctx* c, const float* rays_dev, size_t n_rays, uint64_t first_index, float* radiance_dev, const pt_params* p,
                   uint32_t spp, int mode) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    const CallFacts a = {false, p, spp, rays_dev && radiance_dev, false, false, n_rays, mode};
    Refusal r = check_path_call(f, a);
    if (r.code != PT_OK || r.nothing) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = refresh_tri_lights(c, f, p);
    if (rc != PT_OK) return rc;
    RaysPlan plan;
    r = plan_rays(f, a, plan);
    if (r.code != PT_OK) return fail(c, r);
    KParams P;
    fill_path_params(c, f, p, spp, P);
    P.sc.stack_n = plan.L.lstk;
    P.sc.top_base = plan.L.walk >= 2 ? P.sc.wide_root : 0;
    P.sph_tab = plan.sph_tab;
    queue_params(plan.q, c->d_queue.get(), P);   // the context's counters: every use is on the caller's stream, behind a reset of its own
    const ptmi::RaysCall R{rays_dev, radiance_dev, first_index, n_rays, mode == PT_RAYS_HDR};
    const uint32_t per_launch = plan.per_launch;
    if (plan.samples && (rc = samples_reserve(c, nullptr, (size_t)per_launch * n_rays * 3, P)) != PT_OK) return rc;
    P.smp_ss = n_rays;
    P.smp_ps = 1u;
    HIP_TRY(c, span_begin(c));
    for (uint32_t s0 = 0; s0 < spp; s0 += per_launch) {
        P.spp = std::min(per_launch, spp - s0);
        P.frame = p->frame + s0;
        P.sample_index = p->sample_index + s0;
        P.chunk = plan_rays_launch(f, a, plan, P.spp, plan.L.work_blocks);
        HIP_TRY(c, queue_reset(P.queue, c->stream));
        HIP_TRY(c, launch_render_rays(plan.L, P, R, c->stream));
        if (plan.samples) HIP_TRY(c, launch_fold_rays(c, P, R));
    }
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

// pt_render_rays with the rays made in the kernel: the same plan, sample buffer, launches and fold over the call's rows
int pt_render_camera(pt_ctx* c, const pt_camera* cam, const pt_camera_model* cm, const uint32_t* pixels_dev, size_t n, uint64_t first_pixel,
                     float* radiance_dev, const pt_params* p, uint32_t spp, int mode) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    const CallFacts a = {false, p, spp, cam && cm && radiance_dev, false, false, n, mode, true, cm, pixels_dev != nullptr, first_pixel};
    Refusal r = check_path_call(f, a);
    if (r.code != PT_OK || r.nothing) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = refresh_tri_lights(c, f, p);
    if (rc != PT_OK) return rc;
    RaysPlan plan;
    r = plan_rays(f, a, plan);
    if (r.code != PT_OK) return fail(c, r);
    KParams P;
    fill_path_params(c, f, p, spp, P);
    P.cam = *cam;
    P.sc.stack_n = plan.L.lstk;
    P.sc.top_base = plan.L.walk >= 2 ? P.sc.wide_root : 0;
    P.sph_tab = plan.sph_tab;
    queue_params(plan.q, c->d_queue.get(), P);
    const ptmi::CameraCall R{cm, pixels_dev, first_pixel, radiance_dev, n, mode == PT_RAYS_HDR};
    const ptmi::RaysCall fold{nullptr, radiance_dev, 0, n, mode == PT_RAYS_HDR};
    const uint32_t per_launch = plan.per_launch;
    if (plan.samples && (rc = samples_reserve(c, nullptr, (size_t)per_launch * n * 3, P)) != PT_OK) return rc;
    P.smp_ss = n;
    P.smp_ps = 1u;
    HIP_TRY(c, span_begin(c));
    for (uint32_t s0 = 0; s0 < spp; s0 += per_launch) {
        P.spp = std::min(per_launch, spp - s0);
        P.frame = p->frame + s0;
        P.sample_index = p->sample_index + s0;
        P.chunk = plan_rays_launch(f, a, plan, P.spp, plan.L.work_blocks);
        HIP_TRY(c, queue_reset(P.queue, c->stream));
        HIP_TRY(c, launch_render_camera(plan.L, P, R, c->stream));
        if (plan.samples) HIP_TRY(c, launch_fold_rays(c, P, fold));
    }
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

// pt_render_camera's launches over the listed pixels (or the whole image), always through the sample buffer (plan.samples), each
// followed by the fold into the full-frame accumulator, moments and counts: every pixel from its own count on
int pt_render_pixels(pt_ctx* c, const pt_camera* cam, const pt_camera_model* cm, const uint32_t* pixels_dev, size_t n, float* accum_dev,
                     float* moments_dev, uint32_t* counts_dev, const pt_params* p, uint32_t spp, int mode) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    const CtxFacts f = ctx_facts(c);
    CallFacts a = {false, p, spp, cam && cm && accum_dev && counts_dev, false, moments_dev != nullptr, n, mode, true, cm, pixels_dev != nullptr, 0};
    a.pixels = true;
    Refusal r = check_path_call(f, a);
    if (r.code != PT_OK || r.nothing) return fail(c, r);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = refresh_tri_lights(c, f, p);
    if (rc != PT_OK) return rc;
    RaysPlan plan;
    r = plan_rays(f, a, plan);
    if (r.code != PT_OK) return fail(c, r);
    KParams P;
    fill_path_params(c, f, p, spp, P);
    P.cam = *cam;
    P.sc.stack_n = plan.L.lstk;
    P.sc.top_base = plan.L.walk >= 2 ? P.sc.wide_root : 0;
    P.sph_tab = plan.sph_tab;
    queue_params(plan.q, c->d_queue.get(), P);
    const ptmi::CameraCall R{cm, pixels_dev, 0, nullptr, n, mode == PT_RAYS_HDR};   // no rows of running means: the kernel never folds in line
    const ptmi::PixelsCall fold{pixels_dev, accum_dev, moments_dev, counts_dev, n, (uint32_t)((uint64_t)cm->width * (uint64_t)cm->height), mode == PT_RAYS_HDR};
    const uint32_t per_launch = plan.per_launch;
    if ((rc = samples_reserve(c, nullptr, (size_t)per_launch * n * 3, P)) != PT_OK) return rc;
    P.smp_ss = n;
    P.smp_ps = 1u;
    HIP_TRY(c, span_begin(c));
    if (f.timing) {   // pt_get_stage_ms: the path launches as PT_STAGE_FRAME, the folds as PT_STAGE_FOLD
        c->stage_used = 0;
        if (stage_mark(c, PT_STAGE_NONE) != PT_OK) return PT_ERR_DEVICE;
    }
    for (uint32_t s0 = 0; s0 < spp; s0 += per_launch) {
        P.spp = std::min(per_launch, spp - s0);
        P.frame = p->frame + s0;   // (sample_index is not read: the counts carry N)
        P.chunk = plan_rays_launch(f, a, plan, P.spp, plan.L.work_blocks);
        HIP_TRY(c, queue_reset(P.queue, c->stream));
        HIP_TRY(c, launch_render_camera(plan.L, P, R, c->stream));
        if (stage_mark(c, PT_STAGE_FRAME) != PT_OK) return PT_ERR_DEVICE;
        HIP_TRY(c, launch_fold_pixels(c, P, fold));
        if (stage_mark(c, PT_STAGE_FOLD) != PT_OK) return PT_ERR_DEVICE;
    }
    HIP_TRY(c, span_end(c));
    return PT_OK;
}

int pt_get_counters(pt_ctx* c, pt_counters* out) {
    if (!c || !out) return fail(c, PT_ERR_INVALID, "pt_get_counters: null argument");
    unsigned long long h[PT_CNT_WAVE];
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h, c->d_counters.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->rays = h[PT_CNT_RAYS]; out->inner = h[PT_CNT_INNER]; out->tris = h[PT_CNT_TRIS]; out->leaves = h[PT_CNT_LEAVES];
    out->hits = h[PT_CNT_HITS]; out->paths = h[PT_CNT_PATHS];
    return PT_OK;
}

int pt_get_wave_stats(pt_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n < 0) return fail(c, PT_ERR_INVALID, "pt_get_wave_stats: bad argument");
    unsigned long long h[PT_CNT_N];
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h, c->d_counters.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n && i < PT_WAVE_STATS; i++) out[i] = h[PT_CNT_WAVE + i];
    return PT_OK;
}

int pt_get_stage_ms(pt_ctx* c, float* out, int n) {
    if (!c || !out || n < 0) return fail(c, PT_ERR_INVALID, "pt_get_stage_ms: bad argument");
    if (!c->timed || c->stage_used < 2) return fail(c, PT_ERR_INVALID, "pt_get_stage_ms: no timed pt_render (set PT_OPT_TIMING=1 first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->stage_ev[c->stage_used - 1]));
    for (int i = 0; i < n; i++) out[i] = 0.f;
    for (size_t i = 1; i < c->stage_used; i++) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->stage_ev[i - 1], c->stage_ev[i]));
        const int k = c->stage_kind[i];
        if (k >= 0 && k < n) out[k] += ms;
    }
    return PT_OK;
}

int pt_last_kernel_ms(pt_ctx* c, float* ms) {
    if (!c || !ms) return fail(c, PT_ERR_INVALID, "pt_last_kernel_ms: null argument");
    if (!c->timed) return fail(c, PT_ERR_INVALID, "pt_last_kernel_ms: no timed launch (set PT_OPT_TIMING=1 first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return PT_OK;
}

}  // extern "C"
