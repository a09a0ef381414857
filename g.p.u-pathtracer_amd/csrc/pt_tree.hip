// pt_tree.hip — the acceleration structure of a context: the makers that produce a tree as a value (DevTree, pt_ctx.h) from the
// caller's hierarchy, from the device builder (pt_build.hip) or from a device-built tree run through the host optimiser; its
// area cost; adopt_tree, the one place that puts a tree on the context; and the entry points made of them (pt_upload_bvh,
// pt_build_bvh, pt_last_build_ms, pt_scene_info, pt_tree_cost, pt_tree_items).  One translation unit of libptmi.so (pt_ctx.h).
#include <cstring>
#include <utility>

#include "pt_ctx.h"
#include "pt_scene_build.h"

using namespace ptmi;

// pt_tree_cost: one lane per wide node; out[0] = root area, out[1] = sum of inner-child areas, out[2] = sum of leaf area x records
// (per-block partial sums, added up on the host in block order: the figure is reproducible, so a choice made on it is too)
extern "C" __global__ void __launch_bounds__(256) k_tree_cost(const float4* __restrict__ items, uint64_t wide_root, uint32_t n_wide, double* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    double inner = 0.0, leaf = 0.0, root = 0.0;
    if (i < n_wide) {
        const float4* nd = items + wide_root + 4 * (size_t)i;
        const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        const float sc[3] = {q0.w, q3.z, q3.w};
        const uint32_t ql[3] = {__float_as_uint(q1.x), __float_as_uint(q1.y), __float_as_uint(q1.z)};
        const uint32_t qh[3] = {__float_as_uint(q1.w), __float_as_uint(q2.x), __float_as_uint(q2.y)};
        const int link[4] = {__float_as_int(q2.z), __float_as_int(q2.w), __float_as_int(q3.x), __float_as_int(q3.y)};
        float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        for (int k = 0; k < 4; k++) {
            float d[3];
            bool used = true;
            for (int a = 0; a < 3; a++) {
                const int l = (int)((ql[a] >> (8 * k)) & 0xffu), h = (int)((qh[a] >> (8 * k)) & 0xffu);
                if (l > h) used = false;   // an unused slot holds an inverted box
                d[a] = (float)(h - l) * sc[a];
                if (l <= h) { lo[a] = fminf(lo[a], (float)l * sc[a]); hi[a] = fmaxf(hi[a], (float)h * sc[a]); }
            }
            if (!used) continue;
            const double area = 2.0 * ((double)d[0] * d[1] + (double)d[1] * d[2] + (double)d[2] * d[0]);
            if (link[k] >= 0) {
                inner += area;
            } else {
                int n = 0;
                for (size_t r = (size_t)(~link[k] & ~3);; r += 4) {
                    n++;
                    if (__float_as_int(items[r + 1].w) != 0 || n >= 64) break;   // the record's `last` flag
                }
                leaf += area * (double)n;
            }
        }
        if (i == 0) {
            const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
            root = 2.0 * (dx * dy + dy * dz + dz * dx);
        }
    }
    // block reduction through LDS: one partial sum per block and term, no atomics
    __shared__ double s_in[256], s_lf[256];
    s_in[threadIdx.x] = inner; s_lf[threadIdx.x] = leaf;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { s_in[threadIdx.x] += s_in[threadIdx.x + off]; s_lf[threadIdx.x] += s_lf[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[1 + 2 * (size_t)blockIdx.x] = s_in[0]; out[2 + 2 * (size_t)blockIdx.x] = s_lf[0]; }
    if (i == 0) out[0] = root;
}

// PT_OPT_LAST_OCCLUDERS: one lane per record; a record of listed triangle k goes to slot k of the table as its first three pieces, the
// `last` flag set on the list's final slot alone (the shade lanes' loop ends there, as a leaf's does).  A triangle a spatial split lists
// more than once is listed in full each time: the copies write the same values.
struct OccList { int32_t id[PT_OCCLUDERS_MAX]; uint32_t n = 0; };
__global__ void __launch_bounds__(256) k_collect_occluders(const float4* __restrict__ rec, uint32_t n_rec, const OccList L, float4* __restrict__ table) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rec) return;
    const float4 q0 = rec[4 * (size_t)i];
    const int id = __float_as_int(q0.w);
    for (uint32_t k = 0; k < L.n; k++) {
        if (L.id[k] != id) continue;
        const float4 q1 = rec[4 * (size_t)i + 1], q2 = rec[4 * (size_t)i + 2];
        table[3 * k + 0] = q0;
        table[3 * k + 1] = make_float4(q1.x, q1.y, q1.z, __int_as_float(k + 1 == L.n ? 1 : 0));
        table[3 * k + 2] = q2;
    }
}

namespace ptmi {
int select_occluders(std::vector<OccTri>& tris, int32_t* ids, int cap) {
    std::stable_sort(tris.begin(), tris.end(), [](const OccTri& a, const OccTri& b) { return a.id < b.id; });
    tris.erase(std::unique(tris.begin(), tris.end(), [](const OccTri& a, const OccTri& b) { return a.id == b.id; }), tris.end());
    // half the length of e1 x e2 in binary64, from the binary32 vertices; the mesh's area summed in id order: reproducible
    std::vector<double> area(tris.size());
    double total = 0.0;
    for (size_t i = 0; i < tris.size(); i++) {
        const OccTri& t = tris[i];
        const double a[3] = {(double)t.v1[0] - t.v0[0], (double)t.v1[1] - t.v0[1], (double)t.v1[2] - t.v0[2]};
        const double b[3] = {(double)t.v2[0] - t.v0[0], (double)t.v2[1] - t.v0[1], (double)t.v2[2] - t.v0[2]};
        const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
        area[i] = 0.5 * std::sqrt(x * x + y * y + z * z);
        total += area[i];
    }
    std::vector<size_t> big;   // (at most PT_OCCLUDER_AREA_DIV can qualify)
    for (size_t i = 0; i < tris.size(); i++)
        if (area[i] * (double)PT_OCCLUDER_AREA_DIV >= total && area[i] > 0.0) big.push_back(i);
    std::stable_sort(big.begin(), big.end(), [&](size_t a, size_t b) { return area[a] > area[b]; });   // (stable: ties keep the id order)
    const int n = (int)std::min<size_t>(big.size(), (size_t)std::max(cap, 0));
    for (int k = 0; k < n; k++) ids[k] = tris[big[(size_t)k]].id;
    return n;
}

int occluders_collect(pt_ctx* c) {
    const TreeState& t = c->tree;
    if (t.n_occ == 0 || !t.has_bvh || t.records_woop) return PT_OK;
    HIP_TRY(c, c->d_occ.reserve(3 * PT_OCCLUDERS_MAX));   // (made once; nothing to wait for)
    OccList L;
    L.n = t.n_occ;
    std::memcpy(L.id, t.occ_ids, sizeof L.id);
    const uint32_t n_rec = (uint32_t)t.n_refs;
    // (a slot whose triangle the tree holds no record of stays all zero: a record no ray hits)
    HIP_TRY(c, hipMemsetAsync(c->d_occ.get(), 0, c->d_occ.bytes(), c->stream));
    hipLaunchKernelGGL(k_collect_occluders, dim3((n_rec + 255) / 256), dim3(256), 0, c->stream, t.d_nodes + 4 * (size_t)t.n_inner, n_rec, L, c->d_occ.get());
    HIP_TRY(c, hipGetLastError());
    return PT_OK;
}

// ---- makers: none reads or writes the context's tree, refit state or generations ------------------------------------------------

// the area cost of the 4-wide tree of `t` (Moller-Trumbore records), in expected node visits / triangle tests of a random ray
static int tree_cost(pt_ctx* c, const TreeState& t, double* node_visits, double* tri_tests) {
    const unsigned n_blocks = (unsigned)((t.n_wide + 255) / 256);
    const size_t n_out = 1 + 2 * (size_t)n_blocks;
    DevBuf<double> d_out;
    HIP_TRY(c, d_out.alloc(n_out));
    hipLaunchKernelGGL(k_tree_cost, dim3(n_blocks), dim3(256), 0, c->stream, t.d_nodes, t.wide_root, (uint32_t)t.n_wide, d_out.get());
    HIP_TRY(c, hipGetLastError());
    std::vector<double> h(n_out, 0.0);
    HIP_TRY(c, hipMemcpyAsync(h.data(), d_out.get(), d_out.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!(h[0] > 0.0)) return fail(c, PT_ERR_INVALID, "tree cost: degenerate root box");
    double inner = 0.0, leaf = 0.0;
    for (unsigned b = 0; b < n_blocks; b++) { inner += h[1 + 2 * (size_t)b]; leaf += h[2 + 2 * (size_t)b]; }
    *node_visits = (h[0] + inner) / h[0];
    *tri_tests = leaf / h[0];
    return PT_OK;
}

// host hierarchy -> device tree: refine (leaves of at most PT_OPT_LEAF_MAX references), optimise (PT_OPT_OPTIMIZE), emit, upload
static int tree_from_host(pt_ctx* c, ptscene::Tree& X, int32_t max_id, DevTree& out) {
    DevTree made;
    DevTree& t = made;
    ptscene::refine(X, (uint32_t)c->opt_leaf_max);
    if (c->opt_optimize > 0 && c->opt_tri_test == 0) {   // every node re-inserted where the area cost grows least (pt_tree_opt.h)
        double before = 0.0, after = 0.0;
        if (ptscene::optimize(X, c->opt_optimize, 64, before, after)) { t.opt_cost[0] = before; t.opt_cost[1] = after; }
    }
    ptscene::Output O;
    ptscene::emit(X, PT_MAX_TOP, O, c->opt_tri_test == 1);
    const size_t nb = O.bin.size() * sizeof(float), tb = O.rec.size() * sizeof(float), wb = O.wide.size() * sizeof(float);
    if ((nb + tb + wb) / 16 >= (size_t)PT_SENTINEL) return fail(c, PT_ERR_INVALID, "tree from a host hierarchy: too large for 32-bit links");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, t.alloc_items((nb + tb + wb) / sizeof(float4)));   // (whole 64-byte items)
    HIP_TRY(c, hipMemcpy(t.d_nodes, O.bin.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy((char*)t.d_nodes + nb, O.rec.data(), tb, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy((char*)t.d_nodes + nb + tb, O.wide.data(), wb, hipMemcpyHostToDevice));
    t.records_woop = c->opt_tri_test == 1;
    t.wide_root = O.wide_root_f4;
    t.wide_top_layout = O.n_top_wide;
    t.wide_depth = O.depth_wide;
    t.n_wide = O.wide.size() / 16;
    t.n_top_layout = O.n_top_bin;
    t.n_inner = O.bin.size() / 16;
    t.n_refs = O.n_refs;
    t.n_leaves = O.n_leaves;
    t.max_depth = O.depth_bin;
    t.scene_bytes = nb + tb + wb;
    t.max_tri_id = max_id;
    t.has_bvh = true;
    out = std::move(made);
    return PT_OK;
}

// device tree -> optimised device tree (PT_OPT_OPTIMIZE on a tree the DEVICE built): binary nodes + the records' ids come back to
// the host, the hierarchy is optimised like an uploaded one and replaces `tree`, which keeps its build_ms.  A no-op without
// PT_OPT_OPTIMIZE and for Woop records.  soup: the nine vertex floats of the n triangles it was built from (the caller's own: records
// are re-encoded from them bit for bit), triangle k reporting ids[k] (nullptr: k).
static int optimise_device_tree(pt_ctx* c, DevTree& tree, const float* soup, const int32_t* ids, size_t n) {
    const TreeState& in = tree;
    if (c->opt_optimize <= 0 || in.records_woop) return PT_OK;
    std::vector<const float*> by_id((size_t)in.max_tri_id + 1, nullptr);
    for (size_t k = 0; k < n; k++) by_id[ids ? (size_t)ids[k] : k] = soup + 9 * k;
    std::vector<float> bin(16 * (size_t)in.n_inner), rec(16 * (size_t)in.n_refs);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(bin.data(), in.d_nodes, bin.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(rec.data(), (const char*)in.d_nodes + bin.size() * sizeof(float), rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    ptscene::Tree X;
    std::string why;
    if (!ptscene::from_items(bin.data(), (size_t)in.n_inner, rec.data(), (size_t)in.n_refs, by_id, X, why))
        return fail(c, PT_ERR_DEVICE, "device-built tree: " + why);
    const float device_ms = in.build_ms;
    const int rc = tree_from_host(c, X, in.max_tri_id, tree);   // replaces `tree` when it succeeds
    if (rc == PT_OK) tree.build_ms = device_ms;
    return rc;
}

// ---- adoption: the only writer of pt_ctx::tree ---------------------------------------------------------------------------------------
// `occ`: the occluder list of the mesh the tree was made of (PT_OPT_LAST_OCCLUDERS; Woop records are not what the list's test reads).
// The list and its table change with the tree and scene_gen: the old tree's table is overwritten behind the wait below, on the stream
// every later launch of the context is ordered behind.  Should the copy fail the tree stands without a list.
static int adopt_tree(pt_ctx* c, DevTree&& t, const OccList& occ) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, quiesce(c));   // nothing in flight reads the old tree
    c->refit = pt_ctx::Refit();   // made for the old tree (pt_refit_bvh makes it again for this one)
    c->tree = std::move(t);
    c->scene_gen++;
    c->tree.n_occ = c->tree.records_woop ? 0u : occ.n;
    std::memcpy(c->tree.occ_ids, occ.id, sizeof occ.id);
    const int rc = occluders_collect(c);
    if (rc != PT_OK) c->tree.n_occ = 0;
    return rc;
}
}  // namespace ptmi

extern "C" {

// ---------------------------------------------------------------------------------------
// Scene upload: validate the reference Compact arrays (CudaBVH.cpp:121-270), then re-lay
// them out for the gfx950 kernels:
//   nodes  : same 64-byte record; the top PT_MAX_TOP nodes in breadth-first order (any prefix
//            of them can be mirrored in LDS), the rest depth-first (a parent next to its first
//            inner child); links rewritten from byte offsets to float4 indices
//   tris   : 48-byte records {v0.xyz, id | e1.xyz, last | e2.xyz, 0}: the edge subtraction
//            of cudaUtils.h:177-178 is hoisted to upload (same IEEE result), the index
//            remap of :452-456 and the 16-byte terminator fetch of :410-413 disappear
int pt_upload_bvh(pt_ctx* c, const float* nodes, size_t n_node_vec4, const float* tri_verts, size_t n_tri_vec4,
                  const int32_t* tri_index, size_t n_index) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!nodes || !tri_verts || !tri_index) return fail(c, PT_ERR_INVALID, "pt_upload_bvh: null array");
    if (n_node_vec4 < 4 || (n_node_vec4 % 4) != 0) return fail(c, PT_ERR_INVALID, "pt_upload_bvh: node array must hold whole 4-vec4 nodes");
    if (n_index != n_tri_vec4) return fail(c, PT_ERR_INVALID, "pt_upload_bvh: index array must parallel the triangle array");
    if (n_node_vec4 * 16 >= (size_t)PT_SENTINEL || n_tri_vec4 >= (size_t)0x7fffffff)
        return fail(c, PT_ERR_INVALID, "pt_upload_bvh: scene too large for 32-bit links");

    ptscene::Tree T;
    std::string perr;
    if (!ptscene::parse(nodes, n_node_vec4, tri_verts, n_tri_vec4, tri_index, T, perr))
        return fail(c, PT_ERR_INVALID, "pt_upload_bvh: " + perr);
    int32_t max_id = -1;
    for (const ptscene::Ref& r : T.refs) max_id = std::max(max_id, r.id);
    if (c->mat.d_tri_matid && (size_t)max_id >= c->mat.n_tri_matid)
        return fail(c, PT_ERR_INVALID, "pt_upload_bvh: the triangle-material array on this context does not cover this BVH's triangle ids (clear or re-upload it first)");
    OccList occ;   // (from the parsed tree too, before a maker re-arranges its references)
    {
        std::vector<OccTri> soup;
        soup.reserve(T.refs.size());
        for (const ptscene::Ref& r : T.refs) soup.push_back({r.id, r.v, r.v + 3, r.v + 6});
        occ.n = (uint32_t)select_occluders(soup, occ.id, PT_OCCLUDERS_MAX);
    }
    const int rebuild = c->opt_tri_test == 0 ? c->opt_rebuild : 0;
    // PT_OPT_REBUILD: keep the caller's TRIANGLES, not its hierarchy — the distinct triangles of the
    // Compact arrays (a spatial-split builder lists some more than once, each time in full), in id order,
    // are clustered again on the device (pt_build.h).  The closest hit does not depend on the tree, so the
    // images are the same bit for bit; whether the new tree is faster depends on the scene.
    // Taken from the parsed tree here, before a maker re-arranges its references.
    std::vector<int32_t> ids;
    std::vector<float> verts;
    if (rebuild) {
        std::vector<const ptscene::Ref*> sorted;
        sorted.reserve(T.refs.size());
        for (const ptscene::Ref& r : T.refs) sorted.push_back(&r);
        std::sort(sorted.begin(), sorted.end(), [](const ptscene::Ref* a, const ptscene::Ref* b) { return a->id < b->id; });
        for (const ptscene::Ref* r : sorted) {
            if (!ids.empty() && ids.back() == r->id) continue;
            ids.push_back(r->id);
            verts.insert(verts.end(), r->v, r->v + 9);
        }
    }
    auto reclustered = [&](DevTree& out) -> int {   // device build over those triangles, then PT_OPT_OPTIMIZE
        std::vector<int32_t> tri_rows(3 * ids.size());
        for (size_t i = 0; i < tri_rows.size(); i++) tri_rows[i] = (int32_t)i;
        const int rc = build_bvh_impl(c, verts.data(), verts.size() / 3, tri_rows.data(), ids.size(), out, ids.data());
        return rc == PT_OK ? optimise_device_tree(c, out, verts.data(), ids.data(), ids.size()) : rc;
    };
    DevTree a;
    int rc = rebuild == 1 ? reclustered(a) : tree_from_host(c, T, max_id, a);
    if (rc != PT_OK) return rc;
    // PT_OPT_REBUILD 2: the re-clustered tree beside the caller's; the one that costs a random ray fewer wide-node visits stays.
    // Without a wide tree or a cost for the caller's, or with a failure on the re-clustered side (no error of the call), the caller's.
    double cost_a = 0.0, cost_b = 0.0, unused = 0.0;
    if (rebuild == 2 && a.n_wide > 0 && tree_cost(c, a, &cost_a, &unused) == PT_OK) {
        DevTree b;
        if (reclustered(b) == PT_OK && tree_cost(c, b, &cost_b, &unused) == PT_OK && cost_b < cost_a) a = std::move(b);
        else c->err.clear();
    }
    return adopt_tree(c, std::move(a), occ);
}

// ---- pt_build_bvh: the BVH built on the device (pt_build.h) ---------------------------------
int pt_build_bvh(pt_ctx* c, const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    DevTree t;
    int rc = build_bvh_impl(c, verts, n_verts, tris, n_tris, t);
    if (rc == PT_OK && c->opt_optimize > 0 && c->opt_presplit == 0) {   // PT_OPT_OPTIMIZE: the built hierarchy goes through the host optimiser
        std::vector<float> flat(9 * n_tris);
        for (size_t i = 0; i < 3 * n_tris; i++) std::memcpy(&flat[3 * i], verts + 3 * (size_t)tris[i], 3 * sizeof(float));
        rc = optimise_device_tree(c, t, flat.data(), nullptr, n_tris);
    }
    if (rc != PT_OK) return rc;
    OccList occ;   // (the build checked the indices)
    {
        std::vector<OccTri> soup(n_tris);
        for (size_t i = 0; i < n_tris; i++)
            soup[i] = {(int32_t)i, verts + 3 * (size_t)tris[3 * i], verts + 3 * (size_t)tris[3 * i + 1], verts + 3 * (size_t)tris[3 * i + 2]};
        occ.n = (uint32_t)select_occluders(soup, occ.id, PT_OCCLUDERS_MAX);
    }
    return adopt_tree(c, std::move(t), occ);
}

int pt_occluder_ids(const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris, int32_t* ids_out, int cap) {
    if (!verts || !tris || !ids_out || cap < 0) return fail(nullptr, PT_ERR_INVALID, "pt_occluder_ids: null array or negative cap");
    std::vector<OccTri> soup(n_tris);
    for (size_t i = 0; i < n_tris; i++) {
        for (int k = 0; k < 3; k++)
            if (tris[3 * i + k] < 0 || (size_t)tris[3 * i + k] >= n_verts) return fail(nullptr, PT_ERR_INVALID, "pt_occluder_ids: vertex index out of range");
        soup[i] = {(int32_t)i, verts + 3 * (size_t)tris[3 * i], verts + 3 * (size_t)tris[3 * i + 1], verts + 3 * (size_t)tris[3 * i + 2]};
    }
    return select_occluders(soup, ids_out, std::min(cap, PT_OCCLUDERS_MAX));
}

int pt_last_build_ms(pt_ctx* c, float* ms) {
    if (!c || !ms) return fail(c, PT_ERR_INVALID, "pt_last_build_ms: null argument");
    if (c->tree.build_ms < 0.f) return fail(c, PT_ERR_INVALID, "pt_last_build_ms: the tree on this context was not built on the device");
    *ms = c->tree.build_ms;
    return PT_OK;
}

int pt_scene_info(pt_ctx* c, uint64_t* n_inner, uint64_t* n_refs, uint64_t* n_leaves, uint32_t* max_depth, uint64_t* bytes) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!c->tree.has_bvh) return fail(c, PT_ERR_NO_SCENE, "pt_scene_info: no BVH uploaded");
    if (n_inner) *n_inner = c->tree.n_inner;
    if (n_refs) *n_refs = c->tree.n_refs;
    if (n_leaves) *n_leaves = c->tree.n_leaves;
    if (max_depth) *max_depth = c->tree.max_depth;
    if (bytes) *bytes = c->tree.scene_bytes;
    return PT_OK;
}

int pt_tree_cost(pt_ctx* c, double* node_visits, double* tri_tests) {
    if (!c || !node_visits || !tri_tests) return fail(c, PT_ERR_INVALID, "pt_tree_cost: null argument");
    if (!c->tree.has_bvh || c->tree.wide_root == 0 || c->tree.n_wide == 0) return fail(c, PT_ERR_NO_SCENE, "pt_tree_cost: no 4-wide tree on this context");
    if (c->tree.records_woop) return fail(c, PT_ERR_UNSUPPORTED, "pt_tree_cost: reads the Moller-Trumbore records' leaf terminators");
    HIP_TRY(c, hipSetDevice(c->device));
    return tree_cost(c, c->tree, node_visits, tri_tests);
}

// read-only view of the item buffer: what an audit of the tree downloads
int pt_tree_items(pt_ctx* c, const void** items_dev, uint64_t* n_binary, uint64_t* n_records, uint64_t* n_wide, uint32_t* wide_depth) {
    if (!c || !items_dev) return fail(c, PT_ERR_INVALID, "pt_tree_items: null argument");
    if (!c->tree.has_bvh || !c->tree.d_nodes) return fail(c, PT_ERR_NO_SCENE, "pt_tree_items: no BVH on this context");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // a pending pt_refit_bvh has written its boxes
    *items_dev = c->tree.d_nodes;
    if (n_binary) *n_binary = c->tree.n_inner;
    if (n_records) *n_records = c->tree.n_refs;
    if (n_wide) *n_wide = c->tree.n_wide;
    if (wide_depth) *wide_depth = c->tree.wide_depth;
    return PT_OK;
}

}  // extern "C"
