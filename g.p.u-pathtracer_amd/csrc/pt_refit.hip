// pt_refit.hip — pt_refit_bvh: the triangles of the tree on the context move, its topology stays, every box is refit on the
// device.  One translation unit of libptmi.so (pt_ctx.h).
//   1. k_refit_records   one lane per record: the caller's nine floats re-encoded (pt_encode_record, `last` kept), the
//                        triangle's box (min / max of its vertices, as pt_build_bvh computes it) into rec_box
//   2. k_refit_level     one launch per node height, both trees in it: a binary node writes its two child boxes into itself,
//                        a wide node is re-encoded (pt_encode_wide_node, its original child count and links); each writes
//                        the exact union of its triangles into its scratch box for its parent to read
// Heights, child counts and leaf ranges come from the first refit of a tree (refit_prepare: the only synchronous step); the
// kernels read no link they have to follow and loop over no data-dependent count that the host did not bound.
// A dropped triangle (a coordinate that is not finite or above 3.0e38 in magnitude) gets zero edges — Moller-Trumbore
// rejects it (det < EPS) with and without culling — and an empty box (lo > hi) that no union takes in.  The encoders never
// see an empty box: an empty child is given a point box at a sibling's lower corner (the origin when all are empty).
#include <cstring>
#include <vector>

#include "pt_ctx.h"
#include "pt_items.h"

#define PTR_BLOCK 256
#define PTR_LEAF_CAP 65535   // records of one leaf (16-bit counts in the wide list)

namespace {

struct RefitArgs {
    float4* items;
    const float* verts;          // [n_tris][9] by original triangle id
    uint32_t n_rec;
    uint64_t rec_base;           // float4 index of record 0
    uint64_t wide_root;          // float4 index of wide node 0
    float* rec_box;
    float* bin_box;
    float* wide_box;
    const uint32_t* first_use;
    uint32_t* n_dropped;
};

__device__ __forceinline__ void ptr_set_empty(float* b) {
    for (int a = 0; a < 3; a++) { b[a] = 3.402823466e+38f; b[3 + a] = -3.402823466e+38f; }
}
__device__ __forceinline__ bool ptr_empty(const float* b) { return !(b[0] <= b[3]); }
__device__ __forceinline__ void ptr_grow(float* u, const float* b) {
    for (int a = 0; a < 3; a++) { u[a] = fminf(u[a], b[a]); u[3 + a] = fmaxf(u[3 + a], b[3 + a]); }
}
// union of the triangle boxes of records [j0, j0 + n) (n <= PTR_LEAF_CAP, from the host)
__device__ __forceinline__ void ptr_leaf_box(const float* __restrict__ rec_box, uint64_t j0, int n, float* b) {
    ptr_set_empty(b);
    for (int r = 0; r < n; r++) ptr_grow(b, rec_box + 6 * (j0 + (uint64_t)r));
}
// the empty children of a node get a point box at the first non-empty one's lower corner (the origin if there is none)
template <int N>
__device__ __forceinline__ void ptr_fill_empty(float (*b)[6], int n) {
    float p[3] = {0.f, 0.f, 0.f};
    bool found = false;
#pragma unroll
    for (int k = 0; k < N; k++)
        if (k < n && !found && !ptr_empty(b[k])) { p[0] = b[k][0]; p[1] = b[k][1]; p[2] = b[k][2]; found = true; }
#pragma unroll
    for (int k = 0; k < N; k++)
        if (k < n && ptr_empty(b[k]))
            for (int a = 0; a < 3; a++) b[k][a] = b[k][3 + a] = p[a];
}

__global__ void __launch_bounds__(PTR_BLOCK) k_refit_records(const RefitArgs A) {
    const uint32_t i = blockIdx.x * PTR_BLOCK + threadIdx.x;
    bool count = false;
    if (i < A.n_rec) {
        float4* r = A.items + A.rec_base + 4 * (size_t)i;
        const int32_t id = __float_as_int(r[0].w), last = __float_as_int(r[1].w);
        float box[6];
        ptr_set_empty(box);
        if (id >= 0) {   // (-1: the dummy record of an empty leaf stays as it is)
            float v[9];
            bool finite = true;
            for (int k = 0; k < 9; k++) {
                v[k] = A.verts[9 * (size_t)id + k];
                finite = finite && fabsf(v[k]) <= 3.0e38f;
            }
            float rec[16];
            if (finite) {
                for (int a = 0; a < 3; a++) {
                    box[a] = fminf(v[a], fminf(v[3 + a], v[6 + a]));
                    box[3 + a] = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
                }
                if (v[0] == 0.f) v[0] = 0.f;   // -0.0f -> +0.0f, as pt_build_bvh's records (k_records)
                pt_encode_record(v, v + 3, v + 6, id, last, rec);
            } else {
                const float z[3] = {0.f, 0.f, 0.f};
                pt_encode_record(z, z, z, id, last, rec);
                count = (A.first_use[i >> 5] >> (i & 31)) & 1u;
            }
            for (int k = 0; k < 4; k++) r[k] = make_float4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
        }
        for (int a = 0; a < 6; a++) A.rec_box[6 * (size_t)i + a] = box[a];
    }
    if (A.n_dropped) {
        const unsigned long long m = __ballot(count);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.n_dropped, (uint32_t)__popcll(m));
    }
}

__device__ __forceinline__ void ptr_binary_node(const RefitArgs& A, const int4 e) {
    float4* nd = A.items + 4 * (size_t)e.x;
    const float4 q3 = nd[3];
    const int32_t link[2] = {__float_as_int(q3.x), __float_as_int(q3.y)};
    const int cnt[2] = {e.y, e.z};
    float b[2][6], u[6];
    ptr_set_empty(u);
    for (int k = 0; k < 2; k++) {
        if (link[k] < 0) {
            ptr_leaf_box(A.rec_box, ((uint64_t)(uint32_t)~link[k] - A.rec_base) >> 2, cnt[k], b[k]);
        } else {
            const float* s = A.bin_box + 6 * (size_t)(link[k] >> 2);
            for (int a = 0; a < 6; a++) b[k][a] = s[a];
        }
        if (!ptr_empty(b[k])) ptr_grow(u, b[k]);
    }
    ptr_fill_empty<2>(b, 2);
    // Compact layout: [c0.lo.x c0.hi.x c0.lo.y c0.hi.y] [c1 ...] [c0.lo.z c0.hi.z c1.lo.z c1.hi.z] [links: kept]
    nd[0] = make_float4(b[0][0], b[0][3], b[0][1], b[0][4]);
    nd[1] = make_float4(b[1][0], b[1][3], b[1][1], b[1][4]);
    nd[2] = make_float4(b[0][2], b[0][5], b[1][2], b[1][5]);
    for (int a = 0; a < 6; a++) A.bin_box[6 * (size_t)e.x + a] = u[a];
}

__device__ __forceinline__ void ptr_wide_node(const RefitArgs& A, const int4 e) {
    float4* nd = A.items + A.wide_root + 4 * (size_t)e.x;
    const float4 q2 = nd[2], q3 = nd[3];
    const int32_t link[4] = {__float_as_int(q2.z), __float_as_int(q2.w), __float_as_int(q3.x), __float_as_int(q3.y)};
    const int n = e.y;
    const int cnt[4] = {e.z & 0xffff, (int)((uint32_t)e.z >> 16), e.w & 0xffff, (int)((uint32_t)e.w >> 16)};
    float b[4][6], u[6];
    ptr_set_empty(u);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k >= n) continue;
        if (link[k] < 0) {
            ptr_leaf_box(A.rec_box, ((uint64_t)(uint32_t)(~link[k] & ~3) - A.rec_base) >> 2, cnt[k], b[k]);
        } else {
            const float* s = A.wide_box + 6 * (size_t)(((uint64_t)(uint32_t)link[k] - A.wide_root) >> 2);
            for (int a = 0; a < 6; a++) b[k][a] = s[a];
        }
        if (!ptr_empty(b[k])) ptr_grow(u, b[k]);
    }
    ptr_fill_empty<4>(b, n);
    PtBox cb[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int a = 0; a < 3; a++) { cb[k].lo[a] = b[k][a]; cb[k].hi[a] = b[k][3 + a]; }
    // unused slots: the inverted box and link 0 again, as before.  The child count as a constant: the encoder's loops unroll
    // and cb stays in registers (with a run-time count the boxes went to scratch)
    float d[16];
    switch (n) {
        case 1: pt_encode_wide_node(cb, 1, link, d); break;
        case 2: pt_encode_wide_node(cb, 2, link, d); break;
        case 3: pt_encode_wide_node(cb, 3, link, d); break;
        default: pt_encode_wide_node(cb, 4, link, d); break;
    }
    for (int k = 0; k < 4; k++) nd[k] = make_float4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
    for (int a = 0; a < 6; a++) A.wide_box[6 * (size_t)e.x + a] = u[a];
}

// what the host needs of the tree to schedule a refit, packed: [binary nodes: links 0, 1][records: id, last][wide nodes: links 0..3]
// (8 + 8 + 16 bytes instead of the 64-byte items)
__global__ void __launch_bounds__(PTR_BLOCK) k_refit_shape(const float4* __restrict__ items, uint64_t n_bin, uint64_t n_rec, uint64_t n_wide,
                                                           int32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * PTR_BLOCK + threadIdx.x;
    if (i < n_bin) {
        const float4 q3 = items[4 * i + 3];
        out[2 * i] = __float_as_int(q3.x);
        out[2 * i + 1] = __float_as_int(q3.y);
    } else if (i < n_bin + n_rec) {
        const uint64_t j = i - n_bin;
        const float4* r = items + 4 * n_bin + 4 * j;
        out[2 * i] = __float_as_int(r[0].w);
        out[2 * i + 1] = __float_as_int(r[1].w);
    } else if (i < n_bin + n_rec + n_wide) {
        const uint64_t k = i - n_bin - n_rec;
        const float4* w = items + 4 * (n_bin + n_rec) + 4 * k;
        const float4 q2 = w[2], q3 = w[3];
        int32_t* o = out + 2 * (n_bin + n_rec) + 4 * k;
        o[0] = __float_as_int(q2.z); o[1] = __float_as_int(q2.w); o[2] = __float_as_int(q3.x); o[3] = __float_as_int(q3.y);
    }
}

// the binary and wide nodes of one height: their children are leaves or nodes of lower heights (earlier launches)
__global__ void __launch_bounds__(PTR_BLOCK) k_refit_level(const RefitArgs A, const int4* __restrict__ bin, uint32_t n_bin,
                                                           const int4* __restrict__ wide, uint32_t n_wide) {
    const uint32_t i = blockIdx.x * PTR_BLOCK + threadIdx.x;
    if (i < n_bin) ptr_binary_node(A, bin[i]);
    else if (i - n_bin < n_wide) ptr_wide_node(A, wide[i - n_bin]);
}

}  // namespace

namespace ptmi {

// The schedule of the tree on the context: its item buffer comes back once, the reachable nodes of both trees get a height
// (0: only leaf children), a child count (wide) and the record count of every leaf child, sorted by height.
static int refit_prepare(pt_ctx* c) {
    c->refit = pt_ctx::Refit();
    const uint64_t n_bin = c->tree.n_inner, n_rec = c->tree.n_refs, n_wide = c->tree.n_wide;
    const uint64_t rec_base = 4 * n_bin, wide_root = c->tree.wide_root;
    if (n_bin == 0 || n_rec == 0 || n_wide == 0 || wide_root != rec_base + 4 * n_rec || n_rec >= (1ull << 31))
        // (every tree pt_upload_bvh and pt_build_bvh install has an inner root, a lone triangle is doubled: not met in practice)
        return fail(c, PT_ERR_UNSUPPORTED, "pt_refit_bvh: the tree on this context lacks the [binary nodes][records][wide nodes] layout");
    // the links, ids and `last` flags come back packed (k_refit_shape), not the item buffer
    std::vector<int32_t> h(2 * (n_bin + n_rec) + 4 * n_wide);
    {
        DevBuf<int32_t> d_shape;
        HIP_TRY(c, d_shape.alloc(h.size()));
        const uint64_t n_all = n_bin + n_rec + n_wide;
        hipLaunchKernelGGL(k_refit_shape, dim3((unsigned)((n_all + PTR_BLOCK - 1) / PTR_BLOCK)), dim3(PTR_BLOCK), 0, c->stream, c->tree.d_nodes, n_bin,
                           n_rec, n_wide, d_shape.get());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h.data(), d_shape.get(), d_shape.bytes(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const int32_t* bl_links = h.data();                       // [n_bin][2]
    const int32_t* rec_w = h.data() + 2 * n_bin;              // [n_rec] id, last
    const int32_t* wl_links = h.data() + 2 * (n_bin + n_rec); // [n_wide][4]
    auto bad = [&](const char* why) { return fail(c, PT_ERR_DEVICE, std::string("pt_refit_bvh: malformed tree: ") + why); };
    // records of the leaf whose first record sits at float4 index r (0 = bad link)
    auto leaf_count = [&](int64_t r) -> int {
        if (r < (int64_t)rec_base || ((r - (int64_t)rec_base) & 3) != 0 || (uint64_t)(r - (int64_t)rec_base) / 4 >= n_rec) return 0;
        uint64_t j = (uint64_t)(r - (int64_t)rec_base) / 4;
        for (int n = 1; n <= PTR_LEAF_CAP && j < n_rec; n++, j++)
            if (rec_w[2 * j + 1] != 0) return n;
        return 0;
    };

    // binary tree (walks 0/1): breadth-first from node 0, heights in reverse order
    std::vector<int32_t> order{0}, hb(n_bin, -1);
    std::vector<int4> ent{make_int4(0, 0, 0, 0)};
    std::vector<uint8_t> seen(n_bin, 0);
    seen[0] = 1;
    for (size_t k = 0; k < order.size(); k++) {
        const int32_t link[2] = {bl_links[2 * (size_t)order[k]], bl_links[2 * (size_t)order[k] + 1]};
        int cnt[2] = {0, 0};
        for (int i = 0; i < 2; i++) {
            if (link[i] < 0) {
                if (!(cnt[i] = leaf_count((int64_t)(uint32_t)~link[i]))) return bad("binary leaf link");
            } else {
                const uint64_t ch = (uint64_t)link[i] / 4;
                if ((link[i] & 3) || ch >= n_bin || seen[ch]) return bad("binary inner link");
                seen[ch] = 1;
                order.push_back((int32_t)ch);
                ent.push_back(make_int4((int32_t)ch, 0, 0, 0));
            }
        }
        ent[k] = make_int4(order[k], cnt[0], cnt[1], 0);
    }
    int max_h = 0;
    for (size_t k = order.size(); k-- > 0;) {
        int ht = 0;
        for (int32_t l : {bl_links[2 * (size_t)order[k]], bl_links[2 * (size_t)order[k] + 1]})
            if (l >= 0) ht = std::max(ht, hb[(size_t)l / 4] + 1);
        hb[(size_t)order[k]] = ht;
        max_h = std::max(max_h, ht);
    }

    // 4-wide tree (walks 2/4, the stage-split pipeline): breadth-first from slot 0
    std::vector<int32_t> worder{0}, hw(n_wide, -1);
    std::vector<int4> went;
    std::vector<uint8_t> wseen(n_wide, 0);
    wseen[0] = 1;
    for (size_t k = 0; k < worder.size(); k++) {
        const int32_t* link = wl_links + 4 * (size_t)worder[k];
        int n = 1;
        while (n < 4 && link[n] != link[0]) n++;   // the encoder repeats link 0 in the unused slots
        int cnt[4] = {0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            if (link[i] < 0) {
                if (!(cnt[i] = leaf_count((int64_t)(uint32_t)(~link[i] & ~3)))) return bad("wide leaf link");
            } else {
                const int64_t off = (int64_t)link[i] - (int64_t)wide_root;
                if (off < 0 || (off & 3) || (uint64_t)off / 4 >= n_wide || wseen[(size_t)off / 4]) return bad("wide inner link");
                wseen[(size_t)off / 4] = 1;
                worder.push_back((int32_t)(off / 4));
            }
        }
        went.push_back(make_int4(worder[k], n, (int32_t)((uint32_t)cnt[0] | (uint32_t)cnt[1] << 16), (int32_t)((uint32_t)cnt[2] | (uint32_t)cnt[3] << 16)));
    }
    for (size_t k = worder.size(); k-- > 0;) {
        const int32_t* link = wl_links + 4 * (size_t)worder[k];
        int ht = 0;
        for (int32_t l : {link[0], link[1], link[2], link[3]})
            if (l >= 0) ht = std::max(ht, hw[(size_t)(((int64_t)l - (int64_t)wide_root) / 4)] + 1);
        hw[(size_t)worder[k]] = ht;
        max_h = std::max(max_h, ht);
    }

    // the lists, sorted by height (counting sort)
    pt_ctx::Refit& R = c->refit;
    auto by_height = [&](const std::vector<int4>& in, const std::vector<int32_t>& ht, std::vector<uint32_t>& off) {
        off.assign((size_t)max_h + 2, 0);
        for (const int4& e : in) off[(size_t)ht[(size_t)e.x] + 1]++;
        for (size_t i = 1; i < off.size(); i++) off[i] += off[i - 1];
        std::vector<uint32_t> pos(off.begin(), off.end() - 1);
        std::vector<int4> out(in.size());
        for (const int4& e : in) out[pos[(size_t)ht[(size_t)e.x]]++] = e;
        return out;
    };
    const std::vector<int4> bl = by_height(ent, hb, R.bin_off), wl = by_height(went, hw, R.wide_off);
    // first record of every triangle id: a dropped triangle is counted once however many references it has
    std::vector<uint32_t> first((n_rec + 31) / 32, 0u);
    {
        std::vector<uint8_t> id_seen((size_t)std::max<int32_t>(c->tree.max_tri_id, 0) + 1, 0);
        for (uint64_t j = 0; j < n_rec; j++) {
            const int32_t id = rec_w[2 * j];
            if (id < 0 || id > c->tree.max_tri_id || id_seen[(size_t)id]) continue;
            id_seen[(size_t)id] = 1;
            first[j >> 5] |= 1u << (j & 31);
        }
    }
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_bl = up16(bl.size() * sizeof(int4)), b_wl = up16(wl.size() * sizeof(int4));
    const size_t b_bb = up16(6 * n_bin * sizeof(float)), b_wb = up16(6 * n_wide * sizeof(float)), b_rb = up16(6 * n_rec * sizeof(float));
    const size_t b_fu = up16(first.size() * sizeof(uint32_t));
    HIP_TRY(c, R.d_mem.alloc(b_bl + b_wl + b_bb + b_wb + b_rb + b_fu));
    char* m = R.d_mem.get();
    R.bin_list = (int4*)m; m += b_bl;
    R.wide_list = (int4*)m; m += b_wl;
    R.bin_box = (float*)m; m += b_bb;
    R.wide_box = (float*)m; m += b_wb;
    R.rec_box = (float*)m; m += b_rb;
    R.first_use = (uint32_t*)m;
    HIP_TRY(c, hipMemcpy(R.bin_list, bl.data(), bl.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(R.wide_list, wl.data(), wl.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(R.first_use, first.data(), first.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    R.scene_gen = c->scene_gen;
    R.items = c->tree.d_nodes;
    return PT_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" int pt_refit_bvh(pt_ctx* c, const float* tri_verts_dev, size_t n_tris, uint32_t* n_dropped_dev) {
    if (!c) return fail(nullptr, PT_ERR_INVALID, "null ctx");
    if (!tri_verts_dev) return fail(c, PT_ERR_INVALID, "pt_refit_bvh: null vertex array");
    if (!c->tree.has_bvh) return fail(c, PT_ERR_NO_SCENE, "pt_refit_bvh: no BVH on this context");
    if (c->tree.records_woop) return fail(c, PT_ERR_UNSUPPORTED, "pt_refit_bvh: Woop records are made on the host only (PT_OPT_TRI_TEST 0)");
    if (c->tree.max_tri_id < 0 || n_tris <= (size_t)c->tree.max_tri_id)
        return fail(c, PT_ERR_INVALID, "pt_refit_bvh: n_tris does not cover the triangle ids of the tree");
    HIP_TRY(c, hipSetDevice(c->device));
    pt_ctx::Refit& R = c->refit;
    if (!R.d_mem || R.scene_gen != c->scene_gen || R.items != c->tree.d_nodes) {
        const int rc = refit_prepare(c);
        if (rc != PT_OK) { c->refit = pt_ctx::Refit(); return rc; }
    }
    RefitArgs A;
    A.items = c->tree.d_nodes;
    A.verts = tri_verts_dev;
    A.n_rec = (uint32_t)c->tree.n_refs;
    A.rec_base = 4 * c->tree.n_inner;
    A.wide_root = c->tree.wide_root;
    A.rec_box = R.rec_box;
    A.bin_box = R.bin_box;
    A.wide_box = R.wide_box;
    A.first_use = R.first_use;
    A.n_dropped = n_dropped_dev;
    hipStream_t st = c->stream;
    HIP_TRY(c, span_begin(c));
    if (n_dropped_dev) HIP_TRY(c, hipMemsetAsync(n_dropped_dev, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_refit_records, dim3((A.n_rec + PTR_BLOCK - 1) / PTR_BLOCK), dim3(PTR_BLOCK), 0, st, A);
    for (size_t ht = 0; ht + 1 < R.bin_off.size(); ht++) {
        const uint32_t nb = R.bin_off[ht + 1] - R.bin_off[ht], nw = R.wide_off[ht + 1] - R.wide_off[ht];
        if (nb + nw == 0) continue;
        hipLaunchKernelGGL(k_refit_level, dim3((nb + nw + PTR_BLOCK - 1) / PTR_BLOCK), dim3(PTR_BLOCK), 0, st, A, R.bin_list + R.bin_off[ht], nb,
                           R.wide_list + R.wide_off[ht], nw);
    }
    HIP_TRY(c, hipGetLastError());
    // PT_OPT_LAST_OCCLUDERS: the listed triangles' records moved with the rest; their copies follow on the same stream, so no call
    // behind this one tests the old vertices (the list keeps its ids: it is the mesh's by area at adoption)
    if (const int rc = occluders_collect(c); rc != PT_OK) { c->tree.n_occ = 0; return rc; }
    HIP_TRY(c, span_end(c));
    // a path kernel on a side stream (PT_OPT_OVERLAP) waits for this before it reads the tree; the light list is collected again
    HIP_TRY(c, c->geom_ev.ensure(hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->geom_ev, st));
    c->geom_gen++;
    return PT_OK;
}
