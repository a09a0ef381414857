// pt_build.hip — pt_build_bvh's driver: the launches of the device BVH builder (kernels in pt_build.h).
// One translation unit of libptmi.so (pt_ctx.h).  build_bvh_impl checks the mesh once on the host (check_mesh), then runs an
// ATTEMPT: the stages inputs, arrays, order, hierarchy (PLOC or LBVH), emit, finish over one Job.  When PLOC gives up, a second
// attempt runs the same stages with the Karras hierarchy.
#include <cmath>
#include <utility>

#include "pt_ctx.h"
#include "pt_build.h"

namespace ptmi {

// the caller's mesh, checked: what an attempt reads on the host.  Lives in build_bvh_impl, longer than every attempt.
struct Mesh {
    const float* verts; size_t n_verts;
    const int32_t* tris; size_t n_tris;
    const int32_t* id_map;
    float lo[3], hi[3];       // bounds of the vertices
    int32_t max_tri_id;
    int32_t two[6];           // a lone triangle is doubled: the hierarchy needs two leaves (both report id 0)
    const int32_t* rows() const { return n_tris == 1 ? two : tris; }
};

static int check_mesh(pt_ctx* c, Mesh& m) {
    if (!m.verts || !m.tris || m.n_verts == 0 || m.n_tris == 0) return fail(c, PT_ERR_INVALID, "pt_build_bvh: empty mesh or null array");
    if (m.n_tris > (1u << 27) || m.n_verts > (1u << 30)) return fail(c, PT_ERR_INVALID, "pt_build_bvh: mesh too large for 32-bit links");
    if (c->opt_tri_test == 1) return fail(c, PT_ERR_UNSUPPORTED, "pt_build_bvh: Woop records are made by the host path only (pt_upload_bvh)");
    for (size_t i = 0; i < 3 * m.n_tris; i++)
        if (m.tris[i] < 0 || (size_t)m.tris[i] >= m.n_verts) return fail(c, PT_ERR_INVALID, "pt_build_bvh: vertex index out of range");
    for (size_t i = 0; i < 3 * m.n_verts; i++)
        if (!(std::fabs(m.verts[i]) <= 3.0e38f)) return fail(c, PT_ERR_INVALID, "pt_build_bvh: non-finite vertex");
    // the extent of the mesh must be a finite binary32 on every axis: the 4-wide encoder's grid step is ext / 255 (pt_items.h)
    for (int a = 0; a < 3; a++) m.lo[a] = m.hi[a] = m.verts[a];
    for (size_t i = 0; i < 3 * m.n_verts; i++) { m.lo[i % 3] = std::min(m.lo[i % 3], m.verts[i]); m.hi[i % 3] = std::max(m.hi[i % 3], m.verts[i]); }
    for (int a = 0; a < 3; a++)
        if (!(m.hi[a] - m.lo[a] <= 3.402823466e+38f)) return fail(c, PT_ERR_INVALID, "pt_build_bvh: the mesh's extent overflows binary32");
    if (c->mat.d_tri_matid && m.n_tris > c->mat.n_tri_matid)
        return fail(c, PT_ERR_INVALID, "pt_build_bvh: the triangle-material array on this context does not cover this mesh (clear or re-upload it first)");
    for (int k = 0; k < 6; k++) m.two[k] = m.tris[k % 3];
    m.max_tri_id = (int32_t)m.n_tris - 1;
    if (m.id_map) for (size_t i = 0; i < m.n_tris; i++) m.max_tri_id = std::max(m.max_tri_id, m.id_map[i]);
    return PT_OK;
}

// One attempt.  Whatever a launch or an asynchronous copy may still read is the mesh or lives here, until the attempt's last
// synchronise: the stages keep nothing of that kind in their own scope (a read-back is synchronised where it is made).
struct Job {
    const Mesh& m;
    DevTemp tmp;
    BuildArrays B{};
    int n = 0;                        // primitives: max(triangles, 2), more after pre-splitting
    size_t n_items = 0;
    unsigned int n_levels_max = 64;   // binary levels of the hierarchy: what the collapse has to cover
    Event e0, e1;   // the attempt's device time: between the uploads and the last emit launch
    DevTree made;
    explicit Job(const Mesh& mesh) : m(mesh) {}
    dim3 grid() const { return dim3((unsigned)((n + PTB_BLOCK - 1) / PTB_BLOCK)); }
};
static const dim3 blk(PTB_BLOCK);

// what a hierarchy returns besides the PT_* codes: PLOC gave up and the Karras hierarchy can still do it.  Never leaves this file.
constexpr int PLOC_GAVE_UP = INT_MIN;
static int gave_up(pt_ctx* c, int code, const char* why) { (void)fail(c, code, why); return PLOC_GAVE_UP; }

// uploads, the start event, pre-splitting, id_map
static int stage_inputs(pt_ctx* c, Job& j) {
    const Mesh& m = j.m;
    BuildArrays& B = j.B;
    hipStream_t st = c->stream;
    const size_t n_tris = m.n_tris;
    j.n = (int)std::max<size_t>(n_tris, 2);
    B.n_orig = (int)n_tris;
    B.leaf_max = std::max(1, c->opt_leaf_max);
    float* d_verts = nullptr;
    int* d_tris_idx = nullptr;
    HIP_TRY(c, j.tmp.get(&d_verts, 3 * m.n_verts));
    HIP_TRY(c, j.tmp.get(&d_tris_idx, 3 * (size_t)j.n));
    HIP_TRY(c, hipMemcpyAsync(d_verts, m.verts, 3 * m.n_verts * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_tris_idx, m.rows(), 3 * (size_t)j.n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    B.verts = d_verts;
    B.tris = d_tris_idx;
    HIP_TRY(c, j.e0.ensure());
    HIP_TRY(c, j.e1.ensure());
    HIP_TRY(c, hipEventRecord(j.e0, st));
    if (c->opt_presplit && n_tris >= 64) {
        // pre-splitting: long triangles enter as several primitives (pt_build.h); the target length is a
        // multiple of the edge a triangle would have if the n of them tiled a square of the scene's diagonal
        const float *lo = m.lo, *hi = m.hi;
        const float diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
        const float target = 0.01f * (float)c->opt_presplit * diag / std::sqrt((float)n_tris);
        int *d_cnt = nullptr, *d_off = nullptr;
        HIP_TRY(c, j.tmp.get(&d_cnt, n_tris));
        HIP_TRY(c, j.tmp.get(&d_off, n_tris));
        hipLaunchKernelGGL(k_split_count, j.grid(), blk, 0, st, d_verts, d_tris_idx, (int)n_tris, target, d_cnt);
        size_t sb = 0;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, sb, d_cnt, d_off, (int)n_tris, st));
        char* stmp = nullptr;
        HIP_TRY(c, j.tmp.get(&stmp, sb));
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(stmp, sb, d_cnt, d_off, (int)n_tris, st));
        int last_off = 0, last_cnt = 0;
        HIP_TRY(c, hipMemcpyAsync(&last_off, d_off + (n_tris - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&last_cnt, d_cnt + (n_tris - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const long n_ref = (long)last_off + last_cnt;
        if (n_ref > (long)n_tris && n_ref < (1l << 27)) {
            int* d_ref = nullptr;
            HIP_TRY(c, j.tmp.get(&B.tbox, 6 * (size_t)n_ref));
            HIP_TRY(c, j.tmp.get(&d_ref, (size_t)n_ref));
            hipLaunchKernelGGL(k_split_emit, j.grid(), blk, 0, st, d_verts, d_tris_idx, (int)n_tris, target, d_off, B.tbox, d_ref);
            HIP_TRY(c, hipGetLastError());
            B.ref_tri = d_ref;
            j.n = (int)n_ref;
        }
    }
    B.n = j.n;
    if (m.id_map) {
        int* d_map = nullptr;
        HIP_TRY(c, j.tmp.get(&d_map, n_tris));
        HIP_TRY(c, hipMemcpyAsync(d_map, m.id_map, n_tris * sizeof(int32_t), hipMemcpyHostToDevice, st));
        B.id_map = d_map;
    }
    return PT_OK;
}

// the temporaries, the item buffer (zeroed) and the counters' initial values (k_build_reset: no copy from the host)
static int stage_arrays(pt_ctx* c, Job& j) {
    BuildArrays& B = j.B;
    const size_t n = (size_t)j.n;
    if (!B.tbox) HIP_TRY(c, j.tmp.get(&B.tbox, 6 * n));
    HIP_TRY(c, j.tmp.get(&B.cbounds, 6));
    HIP_TRY(c, j.tmp.get(&B.key_in, n));
    HIP_TRY(c, j.tmp.get(&B.key, n));
    HIP_TRY(c, j.tmp.get(&B.val_in, n));
    HIP_TRY(c, j.tmp.get(&B.val, n));
    HIP_TRY(c, j.tmp.get(&B.left, n));
    HIP_TRY(c, j.tmp.get(&B.right, n));
    HIP_TRY(c, j.tmp.get(&B.first, n));
    HIP_TRY(c, j.tmp.get(&B.last, n));
    HIP_TRY(c, j.tmp.get(&B.parent_i, n));
    HIP_TRY(c, j.tmp.get(&B.parent_l, n));
    HIP_TRY(c, j.tmp.get(&B.nbox, 6 * n));
    HIP_TRY(c, j.tmp.get(&B.arrive, n));
    HIP_TRY(c, j.tmp.get(&B.stats, 4));
    HIP_TRY(c, j.tmp.get(&B.level_cnt, PTB_LEVEL_CNT));
    HIP_TRY(c, j.tmp.get(&B.frontier_a, n));
    HIP_TRY(c, j.tmp.get(&B.frontier_b, n));
    j.n_items = (n - 1) + n + (n - 1);   // binary, records, wide (upper bound)
    if (j.n_items * 4 >= (size_t)PT_SENTINEL) return fail(c, PT_ERR_INVALID, "pt_build_bvh: scene too large for 32-bit links");
    HIP_TRY(c, j.made.alloc_items(j.n_items * 4));
    B.items = j.made.d_nodes;
    hipLaunchKernelGGL(k_build_reset, dim3(1), dim3(PTB_LEVEL_CNT), 0, c->stream, B);
    HIP_TRY(c, hipMemsetAsync(B.items, 0, j.n_items * 64, c->stream));
    return PT_OK;
}

// triangle boxes, Morton keys, the sort
static int stage_order(pt_ctx* c, Job& j) {
    const BuildArrays& B = j.B;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_tri_bounds, j.grid(), blk, 0, st, B);
    hipLaunchKernelGGL(k_morton, j.grid(), blk, 0, st, B);
    size_t cub_bytes = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, cub_bytes, B.key_in, B.key, B.val_in, B.val, j.n, 0, 63, st));
    char* cub_tmp = nullptr;
    HIP_TRY(c, j.tmp.get(&cub_tmp, cub_bytes));
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, B.key_in, B.key, B.val_in, B.val, j.n, 0, 63, st));
    return PT_OK;
}

// PLOC: rounds of nearest-neighbour search + mutual merges + ordered compaction.  PLOC_GAVE_UP on degenerate input (hundreds of
// identical boxes: one merge per round, a chain): the Karras hierarchy separates equal keys by position and stays balanced
static int hierarchy_ploc(pt_ctx* c, Job& j) {
    const BuildArrays& B = j.B;
    hipStream_t st = c->stream;
    const int n = j.n;
    PlocArrays Q{};
    HIP_TRY(c, j.tmp.get(&Q.cl, (size_t)n));
    HIP_TRY(c, j.tmp.get(&Q.cl_next, (size_t)n));
    HIP_TRY(c, j.tmp.get(&Q.cbox, 6 * (size_t)n));
    HIP_TRY(c, j.tmp.get(&Q.nn, (size_t)n));
    HIP_TRY(c, j.tmp.get(&Q.keep, (size_t)n));
    HIP_TRY(c, j.tmp.get(&Q.pos, (size_t)n + 1));
    HIP_TRY(c, j.tmp.get(&Q.ref, (size_t)n));
    size_t scan_bytes = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, Q.keep, Q.pos, n, st));
    char* scan_tmp = nullptr;
    HIP_TRY(c, j.tmp.get(&scan_tmp, scan_bytes));
    Q.n_c = n;
    hipLaunchKernelGGL(k_ploc_init, j.grid(), blk, 0, st, B, Q);
    int rounds = 0;
    while (Q.n_c > 1) {
        if (++rounds > 192) return gave_up(c, PT_ERR_UNSUPPORTED, "pt_build_bvh: PLOC needs too many rounds (degenerate input)");
        const dim3 g((unsigned)((Q.n_c + PTB_BLOCK - 1) / PTB_BLOCK));
        hipLaunchKernelGGL(k_ploc_gather, g, blk, 0, st, B, Q);
        hipLaunchKernelGGL(k_ploc_nn, g, blk, 0, st, Q);
        hipLaunchKernelGGL(k_ploc_merge, g, blk, 0, st, B, Q);
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, Q.keep, Q.pos, Q.n_c, st));
        hipLaunchKernelGGL(k_ploc_scatter, g, blk, 0, st, Q);
        HIP_TRY(c, hipGetLastError());
        int last_pos = 0, last_keep = 0;
        HIP_TRY(c, hipMemcpyAsync(&last_pos, Q.pos + (Q.n_c - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&last_keep, Q.keep + (Q.n_c - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const int next = last_pos + last_keep;
        // no pair chose each other: every union's area overflowed binary32 (coordinates near 1e30) — the Karras hierarchy needs no areas
        if (next >= Q.n_c || next < 1) return gave_up(c, PT_ERR_DEVICE, "pt_build_bvh: PLOC round made no progress");
        Q.n_c = next;
        std::swap(Q.cl, Q.cl_next);
    }
    hipLaunchKernelGGL(k_ploc_parents, j.grid(), blk, 0, st, B);
    hipLaunchKernelGGL(k_node_depth, j.grid(), blk, 0, st, B);
    unsigned int deepest = 0;
    HIP_TRY(c, hipMemcpyAsync(&deepest, B.stats + 3, sizeof deepest, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (deepest + 1 > 64) return gave_up(c, PT_ERR_UNSUPPORTED, "pt_build_bvh: PLOC tree deeper than 64 levels");
    j.n_levels_max = deepest + 1;
    // depth-first leaf order: subtrees become contiguous record ranges, so small ones can be cut into
    // multi-triangle leaves (PT_OPT_LEAF_MAX) exactly as in the LBVH
    int* newpos = nullptr;
    HIP_TRY(c, j.tmp.get(&newpos, (size_t)n));
    for (unsigned int level = deepest + 1; level-- > 0;) hipLaunchKernelGGL(k_ploc_size, j.grid(), blk, 0, st, B, level);
    for (unsigned int level = 0; level <= deepest; level++) hipLaunchKernelGGL(k_ploc_first, j.grid(), blk, 0, st, B, level, newpos);
    HIP_TRY(c, hipMemcpyAsync(B.val_in, B.val, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_ploc_reorder, j.grid(), blk, 0, st, B, newpos, B.val_in);
    HIP_TRY(c, hipGetLastError());
    return PT_OK;
}

// Karras' hierarchy, then the bottom-up fit, one launch per level, deepest first
static int hierarchy_lbvh(pt_ctx* c, Job& j) {
    const BuildArrays& B = j.B;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_hierarchy, j.grid(), blk, 0, st, B);
    hipLaunchKernelGGL(k_node_depth, j.grid(), blk, 0, st, B);
    HIP_TRY(c, hipGetLastError());
    unsigned int deepest = 0;
    HIP_TRY(c, hipMemcpyAsync(&deepest, B.stats + 3, sizeof deepest, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (deepest + 1 > 64) return fail(c, PT_ERR_UNSUPPORTED, "pt_build_bvh: tree deeper than 64 levels (degenerate input); use the host builder");
    for (unsigned int level = deepest + 1; level-- > 0;) hipLaunchKernelGGL(k_fit_level, j.grid(), blk, 0, st, B, level);
    j.n_levels_max = deepest + 1;
    return PT_OK;
}

// records, binary nodes, the 4-wide collapse, the end event
static int stage_emit(pt_ctx* c, Job& j) {
    const BuildArrays& B = j.B;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_depth, j.grid(), blk, 0, st, B);
    hipLaunchKernelGGL(k_records, j.grid(), blk, 0, st, B);
    hipLaunchKernelGGL(k_binary, j.grid(), blk, 0, st, B);
    HIP_TRY(c, hipGetLastError());
    // 4-wide collapse, one launch per level of the wide tree; frontier sizes stay on the device, so
    // nothing is read back between levels (a wide level spans at least one binary level: `deepest + 1`
    // launches cover every tree; the empty ones at the end cost a few microseconds each)
    int2 *fin = B.frontier_a, *fout = B.frontier_b;
    const unsigned cgrid = (unsigned)std::min<int>((j.n + PTB_BLOCK - 1) / PTB_BLOCK, 2048);
    for (unsigned int level = 0; level <= j.n_levels_max; level++) {
        hipLaunchKernelGGL(k_collapse, dim3(cgrid), blk, 0, st, B, fin, fout, (int)level);
        std::swap(fin, fout);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(j.e1, st));
    return PT_OK;
}

// the read-back (the attempt's last synchronise), the checks on it, the TreeState
static int stage_finish(pt_ctx* c, Job& j) {
    unsigned int stats[4], level_cnt[PTB_LEVEL_CNT];
    HIP_TRY(c, hipMemcpyAsync(stats, j.B.stats, sizeof stats, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(level_cnt, j.B.level_cnt, sizeof level_cnt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t levels = 0;
    while (levels < 66 && level_cnt[levels] > 0) levels++;
    if (level_cnt[std::min<unsigned int>(j.n_levels_max + 1, 67)] != 0) return fail(c, PT_ERR_DEVICE, "pt_build_bvh: wide collapse did not finish");
    TreeState& t = j.made;
    HIP_TRY(c, hipEventElapsedTime(&t.build_ms, j.e0, j.e1));
    if (stats[3] > 64) return fail(c, PT_ERR_UNSUPPORTED, "pt_build_bvh: tree deeper than 64 levels (degenerate input); use the host builder");
    t.wide_root = 4 * ((uint64_t)(j.n - 1) + (uint64_t)j.n);
    t.wide_top_layout = 1;      // level order below the root, not a breadth-first prefix of fixed size
    t.n_top_layout = 1;
    t.wide_depth = levels;
    t.n_wide = stats[0];
    t.n_inner = (uint64_t)(j.n - 1);
    t.n_refs = (uint64_t)j.n;
    t.n_leaves = stats[2];
    t.max_depth = stats[3];
    t.scene_bytes = j.n_items * 64;
    t.max_tri_id = j.m.max_tri_id;
    t.has_bvh = true;
    return PT_OK;
}

// the device stages from the uploads, with fresh events: build_ms is the device time of the attempt that made the tree
static int attempt(pt_ctx* c, const Mesh& m, int algo, DevTree& out) {
    Job j(m);
    int rc = stage_inputs(c, j);
    if (rc == PT_OK) rc = stage_arrays(c, j);
    if (rc == PT_OK) rc = stage_order(c, j);
    if (rc == PT_OK) rc = algo == 1 && j.n > 2 ? hierarchy_ploc(c, j) : hierarchy_lbvh(c, j);
    if (rc == PT_OK) rc = stage_emit(c, j);
    if (rc == PT_OK) rc = stage_finish(c, j);
    if (rc == PT_OK) out = std::move(j.made);
    return rc;
}

int build_bvh_impl(pt_ctx* c, const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris, DevTree& out, const int32_t* id_map) {
    Mesh m{verts, n_verts, tris, n_tris, id_map, {}, {}, -1, {}};
    if (const int rc = check_mesh(c, m)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int rc = attempt(c, m, c->opt_build_algo, out);
    return rc == PLOC_GAVE_UP ? attempt(c, m, 0, out) : rc;
}

}  // namespace ptmi
