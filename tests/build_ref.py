"""build_ref — what pt_build_bvh builds, restated sequentially: the kernels of csrc/pt_build.h and the decisions of their driver
(csrc/pt_build.hip), stage by stage in numpy.  numpy only: no GPU, no library of the project.  tests/test_build_ref.py holds this
module to account (hand-worked answers, tree_audit's strict audit); tests/test_gpu_build_ref.py holds the device to it, tree for tree.

    build(verts, tris, algo, leaf_max, presplit=0) -> (binary, records, wide, info, wide_depth)
    tree_cost(wide, n_binary, n_records, records=None) -> (node_visits, tri_tests)

The builder is deterministic apart from the NUMBERING of inner nodes and wide slots, which the device takes from atomic counters;
tree_audit.canonical_form removes it, so the comparison is exact.  Arithmetic: numpy's binary32 operators wherever the C has float
* + - / and sqrtf (the library is compiled without contraction; / and sqrtf are correctly rounded), tree_audit.fma32_fast where fmaf is
written (the edge crossings of k_split_emit), tree_audit's _min32 / _max32 for fminf / fmaxf, tree_audit's encoders for the items.

The rules the documents leave to the code, as the code has them (the builder's section, names this module):
  - equal keys are told apart by their sorted position (ptb_delta); the sort is stable, the value is the primitive's row
  - PLOC: a cluster's neighbour is the one with the smallest union area within +-8 positions, strict <, so a tie goes to the smaller
    position; only pairs that chose each other merge, the smaller position is the left child; survivors keep their order
  - the root is never cut into a leaf; an inner node with last - first + 1 <= leaf_max is
  - the collapse opens the non-leaf entry with the largest area first (strict >, the first wins), puts the last entry in its place
    and appends left, then right
  - -0.0f becomes +0.0f in v0.x of a record and nowhere else

Inputs on which binary32 behaviour could depend on the device are refused (OutOfRange): every product of box extents and every area
computed here must be zero or a normal, finite binary32.
"""
import numpy as np

import tree_audit as ta
from tree_audit import _max32, _min32, encode_records, encode_wide_node

F32 = np.float32
FLT_MAX = F32(3.402823466e+38)
PLOC_RADIUS = 8
PLOC_MAX_ROUNDS = 192
MAX_LEVELS = 64
SPLIT_MAX = 8
SPLIT_MIN_TRIS = 64


class OutOfRange(ValueError):
    """A product of extents or an area is subnormal, infinite or NaN: the mesh is no input for this reference."""


def _normal(x, what):
    x = np.asarray(x)
    bad = ~np.isfinite(x) | ((x != 0) & (np.abs(x) < ta.F32_MIN_NORMAL))
    if np.any(bad):
        raise OutOfRange(f"{what}: {np.asarray(x)[bad][:4].tolist()} is not zero or a normal binary32")
    return x


def area32(b, what="area"):
    """ptb_area over boxes float32 [...][6]: 2 * (dx * dy + dy * dz + dz * dx), every step in binary32, checked."""
    b = np.asarray(b, F32)
    with np.errstate(all="ignore"):
        dx, dy, dz = b[..., 3] - b[..., 0], b[..., 4] - b[..., 1], b[..., 5] - b[..., 2]
        p0, p1, p2 = dx * dy, dy * dz, dz * dx
        ar = F32(2.0) * ((p0 + p1) + p2)
    for p in (p0, p1, p2, ar):
        _normal(p, what)
    return ar


def union32(a, b):
    """fminf of the lower corners, fmaxf of the upper ones (first argument = the left child)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.concatenate([_min32(a[..., :3], b[..., :3]), _max32(a[..., 3:], b[..., 3:])], axis=-1)


# ------------------------------------------------------------------------------------------------------------ boxes, keys
def tri_boxes(verts, tris):
    """k_tri_bounds: float32 [n][6] lo xyz, hi xyz of every triangle row."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    return ta.tri_boxes(v[np.asarray(tris, np.int64).reshape(-1, 3)].reshape(-1, 9))


def centres(tbox):
    """c = 0.5f * lo + 0.5f * hi."""
    tbox = np.asarray(tbox, F32)
    return (F32(0.5) * tbox[:, :3] + F32(0.5) * tbox[:, 3:]).astype(F32)


def centre_bounds(c):
    """The bounds of the box centres (k_tri_bounds' reduction; the order of a reduction by min / max does not matter)."""
    return c.min(0), c.max(0)


def _spread21(v):
    x = v & np.uint64(0x1fffff)
    for sh, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(sh))) & np.uint64(mask)
    return x


def quantise(tbox, size_bits=9):
    """The integers k_morton interleaves: (q uint64 [n][3], qs uint64 [n]); qs is zero at size_bits 0."""
    tbox = np.asarray(tbox, F32)
    c = centres(tbox)
    lo, hi = centre_bounds(c)
    ab = 21 if size_bits == 0 else (63 - size_bits) // 3
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(F32)
        u = np.zeros_like(c)
        for a in range(3):
            if ext[a] > 0:
                u[:, a] = _min32(_max32((c[:, a] - lo[a]) / ext[a], F32(0.0)), F32(1.0))
        q = np.minimum((u * F32(1 << ab)).astype(np.uint64), np.uint64((1 << ab) - 1))
        diag2, sdiag2 = np.zeros(len(tbox), F32), F32(0.0)
        for a in range(3):
            d = tbox[:, 3 + a] - tbox[:, a]
            diag2 = diag2 + _normal(d * d, "squared box extent")
            sdiag2 = F32(sdiag2 + _normal(ext[a] * ext[a], "squared scene extent"))
        _normal(diag2, "squared box diagonal")
        qs = np.zeros(len(tbox), np.uint64)
        if size_bits:
            rel = np.sqrt(diag2 / sdiag2) if sdiag2 > 0 else np.zeros(len(tbox), F32)
            qs = np.minimum((np.minimum(rel, F32(1.0)) * F32(1 << size_bits)).astype(np.uint64), np.uint64((1 << size_bits) - 1))
    return q, qs


def interleave(q, qs, size_bits=9):
    """k_morton's bit loop, most significant first: x y z x y z s, x y z x y z s, ... (plain Morton order at size_bits 0)."""
    q, qs = np.asarray(q, np.uint64).reshape(-1, 3), np.asarray(qs, np.uint64).reshape(-1)
    one = np.uint64(1)
    if size_bits == 0:
        return (_spread21(q[:, 0]) << np.uint64(2)) | (_spread21(q[:, 1]) << one) | _spread21(q[:, 2])
    ab = (63 - size_bits) // 3
    key = np.zeros(len(q), np.uint64)
    bx, bs, phase, ax = ab - 1, size_bits - 1, 0, 0
    for _ in range(3 * ab + size_bits):
        if phase == 6 and bs >= 0:
            bit = (qs >> np.uint64(bs)) & one
            bs -= 1
            phase = 0
        else:
            bit = (q[:, ax] >> np.uint64(bx)) & one
            ax += 1
            if ax == 3:
                ax = 0
                bx -= 1
            phase += 1
            if bx < 0:
                phase = 6      # axes exhausted: the rest are size bits
        key = (key << one) | bit
    return key


def morton_keys(tbox, size_bits=9):
    """The sort key of every primitive box (uint64 [n])."""
    return interleave(*quantise(tbox, size_bits), size_bits)


def sort_keys(keys):
    """hipcub's radix sort of (key, row): stable.  Returns (rows in sorted order, sorted keys)."""
    order = np.argsort(np.asarray(keys, np.uint64), kind="stable")
    return order, np.asarray(keys, np.uint64)[order]


# --------------------------------------------------------------------------------------------------------------- Karras
def delta(key, i, j):
    """ptb_delta: common-prefix length of sorted positions i and j, -1 outside; equal keys go on into the positions."""
    n = len(key)
    if j < 0 or j >= n:
        return -1
    x = int(key[i]) ^ int(key[j])
    if x == 0:
        return 64 + (32 - (i ^ j).bit_length())
    return 64 - x.bit_length()


def karras(key):
    """k_hierarchy over sorted keys: (left, right, first, last) of the n - 1 inner nodes; a child >= 0 is an inner node, < 0 is
    ~position of a leaf.  Node 0 is the root."""
    key = [int(k) for k in key]
    n = len(key)
    left, right, first, last = (np.zeros(n - 1, np.int64) for _ in range(4))
    for i in range(n - 1):
        d = 1 if delta(key, i, i + 1) - delta(key, i, i - 1) >= 0 else -1
        dmin = delta(key, i, i - d)
        lmax = 2
        while delta(key, i, i + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(key, i, i + (l + t) * d) > dmin:
                l += t
            t >>= 1
        j = i + l * d
        dnode = delta(key, i, j)
        s, t = 0, (l + 1) >> 1
        while True:
            if delta(key, i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            t = (t + 1) >> 1
        gamma = i + s * d + min(d, 0)
        lo, hi = min(i, j), max(i, j)
        left[i] = ~gamma if lo == gamma else gamma
        right[i] = ~(gamma + 1) if hi == gamma + 1 else gamma + 1
        first[i], last[i] = lo, hi
    return left, right, first, last


def parents_and_depths(left, right):
    """(parent_i, parent_l, depth of every inner node, depth of every leaf position) — k_hierarchy / k_ploc_parents, k_node_depth,
    k_depth.  Depths are edges to the root."""
    n = len(left) + 1
    parent_i, parent_l = np.full(n - 1, -1, np.int64), np.full(n, -1, np.int64)
    depth, leaf_depth = np.zeros(n - 1, np.int64), np.zeros(n, np.int64)
    stack, seen = [0], 0
    while stack:
        i = stack.pop()
        seen += 1
        for c in (int(left[i]), int(right[i])):
            if c >= 0:
                parent_i[c], depth[c] = i, depth[i] + 1
                stack.append(c)
            else:
                parent_l[~c], leaf_depth[~c] = i, depth[i] + 1
    if seen != n - 1 or np.any(parent_l < 0):
        raise AssertionError("the hierarchy is not a tree over every leaf")
    return parent_i, parent_l, depth, leaf_depth


def fit(left, right, depth, leaf_box):
    """k_fit_level: the box of every inner node bottom-up, left child first in fminf / fmaxf."""
    nbox = np.zeros((len(left), 6), F32)

    def box(c):
        return nbox[c] if c >= 0 else leaf_box[~c]
    for i in np.argsort(-depth, kind="stable"):
        nbox[i] = union32(box(int(left[i])), box(int(right[i])))
    return nbox


# ----------------------------------------------------------------------------------------------------------------- PLOC
def ploc_neighbours(cbox, radius=PLOC_RADIUS):
    """k_ploc_nn: for every cluster the position within +-radius whose union with it has the smallest area; strict <, positions in
    ascending order, so a tie goes to the smaller position.  -1 where no area is below FLT_MAX."""
    cbox = np.asarray(cbox, F32)
    n = len(cbox)
    best, best_area = np.full(n, -1, np.int64), np.full(n, FLT_MAX, F32)
    idx = np.arange(n)
    for off in [o for o in range(-radius, radius + 1) if o != 0]:
        i0, i1 = max(0, -off), min(n, n - off)
        if i1 <= i0:
            continue
        ar = area32(union32(cbox[i0:i1], cbox[i0 + off:i1 + off]), "union area")
        better = ar < best_area[i0:i1]
        best[i0:i1] = np.where(better, idx[i0:i1] + off, best[i0:i1])
        best_area[i0:i1] = np.where(better, ar, best_area[i0:i1])
    return best


def ploc_pairs(nn):
    """k_ploc_merge's decision: the positions i < j that chose each other, as (i, j) arrays in ascending i."""
    nn = np.asarray(nn, np.int64)
    i = np.arange(len(nn))
    j = nn
    mutual = (j >= 0) & (nn[np.maximum(j, 0)] == i) & (i < j)
    return i[mutual], j[mutual]


def ploc(leaf_box, radius=PLOC_RADIUS):
    """hierarchy_ploc up to the complete tree: (left, right, nbox), or None when PLOC gives up (more than 192 rounds, a round without
    a merge, a tree deeper than 64 levels) and the Karras hierarchy takes over.  Node numbers are handed out from n - 2 down, so the
    last merge is node 0."""
    leaf_box = np.asarray(leaf_box, F32)
    n = len(leaf_box)
    left, right, nbox = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64), np.zeros((n - 1, 6), F32)
    cl = ~np.arange(n, dtype=np.int64)
    merges = rounds = 0
    while len(cl) > 1:
        rounds += 1
        if rounds > PLOC_MAX_ROUNDS:
            return None
        cbox = np.where((cl >= 0)[:, None], nbox[np.maximum(cl, 0)], leaf_box[np.maximum(~cl, 0)])
        pi, pj = ploc_pairs(ploc_neighbours(cbox, radius))
        if len(pi) == 0:
            return None
        ids = (n - 2) - merges - np.arange(len(pi))
        merges += len(pi)
        left[ids], right[ids] = cl[pi], cl[pj]
        nbox[ids] = union32(cbox[pi], cbox[pj])
        ref, keep = cl.copy(), np.ones(len(cl), bool)
        ref[pi] = ids
        keep[pj] = False
        cl = ref[keep]
    _, _, depth, _ = parents_and_depths(left, right)
    if int(depth.max()) + 1 > MAX_LEVELS:
        return None
    return left, right, nbox


def ploc_leaf_order(left, right):
    """k_ploc_size / k_ploc_first: the depth-first position of every leaf (left subtree first) and the range of every inner node:
    (newpos by old position, first, last)."""
    n = len(left) + 1
    size = np.zeros(n - 1, np.int64)
    _, _, depth, _ = parents_and_depths(left, right)
    for i in np.argsort(-depth, kind="stable"):
        size[i] = sum(int(size[c]) if c >= 0 else 1 for c in (int(left[i]), int(right[i])))
    first, newpos = np.zeros(n - 1, np.int64), np.zeros(n, np.int64)
    for i in np.argsort(depth, kind="stable"):
        f = int(first[i])
        cl, cr = int(left[i]), int(right[i])
        nl = int(size[cl]) if cl >= 0 else 1
        for c, at in ((cl, f), (cr, f + nl)):
            if c >= 0:
                first[c] = at
            else:
                newpos[~c] = at
    return newpos, first, first + size - 1


# ------------------------------------------------------------------------------------------------------------ pre-split
def split_target(verts, n_tris, presplit):
    """stage_inputs' target length in binary32, from the bounds of ALL vertices."""
    v = np.asarray(verts, F32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    with np.errstate(all="ignore"):
        e = (hi - lo).astype(F32)
        diag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        return F32(F32(0.01) * F32(presplit) * diag / np.sqrt(F32(n_tris)))


def split_count(v9, target):
    """ptb_split_count over rows float32 [n][9]: (count, axis).  1 when the longest extent is not above the target, when the target
    is not positive, and when it is above 4 * 8 targets (a wall stays whole); else min(8, ceil(extent / target))."""
    v = np.asarray(v9, F32).reshape(-1, 3, 3)
    target = F32(target)
    box = ta.tri_boxes(v.reshape(-1, 9))
    with np.errstate(all="ignore"):
        ext = (box[:, 3:] - box[:, :3]).astype(F32)
        axis = np.where(ext[:, 0] >= ext[:, 1], np.where(ext[:, 0] >= ext[:, 2], 0, 2), np.where(ext[:, 1] >= ext[:, 2], 1, 2))
        e = ext[np.arange(len(ext)), axis]
        whole = ~(e > target) | ~(target > 0) | (e > F32(4.0) * F32(SPLIT_MAX) * target)
        k = np.minimum(SPLIT_MAX, np.ceil(np.where(whole, F32(1.0), e / target)).astype(np.int64))
    return np.where(whole, 1, k), axis


def split_slabs_of(v9, k, ax):
    """k_split_emit for m triangles that are ALL cut into the same k > 1 slabs of their boxes, triangle i along ax[i]:
    float32 [m][k][6].  Per slab: the vertices inside it and the edge crossings of its two planes (fmaf), padded, never beyond the
    triangle's own box or the padded slab; the whole box where nothing is found."""
    v = np.asarray(v9, F32).reshape(-1, 3, 3)
    m, row = len(v), np.arange(len(v))
    ax = np.asarray(ax, np.int64).reshape(-1)
    box = ta.tri_boxes(v.reshape(-1, 9))
    lo, hi = box[:, :3], box[:, 3:]
    lo_ax, hi_ax = lo[row, ax], hi[row, ax]
    out = np.zeros((m, k, 6), F32)
    tiny, eps = F32(1e-30), F32(1e-5)
    with np.errstate(all="ignore"):
        pad = (eps * _max32(hi - lo, _max32(np.abs(lo), np.abs(hi))) + tiny).astype(F32)
        padx = pad[row, ax]
        for s in range(k):
            x0 = lo_ax if s == 0 else (lo_ax + (hi_ax - lo_ax) * (F32(s) / F32(k))).astype(F32)
            x1 = hi_ax if s == k - 1 else (lo_ax + (hi_ax - lo_ax) * (F32(s + 1) / F32(k))).astype(F32)
            plo, phi = np.full((m, 3), FLT_MAX, F32), np.full((m, 3), -FLT_MAX, F32)
            for e in range(3):
                a, b = v[:, e], v[:, (e + 1) % 3]
                a_ax, b_ax = a[row, ax], b[row, ax]
                inside = ((a_ax >= x0) & (a_ax <= x1))[:, None]
                plo, phi = np.where(inside, _min32(plo, a), plo), np.where(inside, _max32(phi, a), phi)
                for x in (x0, x1):
                    cross = ((a_ax < x) & (b_ax > x)) | ((a_ax > x) & (b_ax < x))
                    t = np.where(cross, (x - a_ax) / np.where(cross, b_ax - a_ax, F32(1.0)), F32(0.0)).astype(F32)
                    pc = ta.fma32_fast(t[:, None], (b - a).astype(F32), a)
                    pc[row, ax] = x
                    plo = np.where(cross[:, None], _min32(plo, pc), plo)
                    phi = np.where(cross[:, None], _max32(phi, pc), phi)
            blo, bhi = _max32(lo, (plo - pad).astype(F32)), _min32(hi, (phi + pad).astype(F32))
            none = ~(blo <= bhi)
            blo, bhi = np.where(none, lo, blo), np.where(none, hi, bhi)
            slab_lo, slab_hi = _max32(lo_ax, (x0 - padx).astype(F32)), _min32(hi_ax, (x1 + padx).astype(F32))
            blo_ax, bhi_ax = _max32(blo[row, ax], slab_lo), _min32(bhi[row, ax], slab_hi)
            none = ~(blo_ax <= bhi_ax)
            blo[row, ax], bhi[row, ax] = np.where(none, slab_lo, blo_ax), np.where(none, slab_hi, bhi_ax)
            out[:, s, :3], out[:, s, 3:] = blo, bhi
    return out


def split_slabs(v9, k, ax):
    """k_split_emit for ONE triangle cut into k > 1 slabs of its box along ax: float32 [k][6]."""
    return split_slabs_of(np.asarray(v9, F32).reshape(1, 9), k, [ax])[0]


def presplit_boxes(verts, tris, presplit):
    """The pre-split of stage_inputs: (tbox float32 [n_ref][6], ref_tri int [n_ref]) in triangle order, or None when the option is
    off, the mesh has fewer than 64 triangles or no triangle is cut."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(tris)
    if not presplit or n < SPLIT_MIN_TRIS:
        return None
    v9 = np.asarray(verts, F32).reshape(-1, 3)[tris].reshape(-1, 9)
    target = split_target(verts, n, presplit)
    k, axis = split_count(v9, target)
    if int(k.sum()) <= n:
        return None
    off = np.concatenate([[0], np.cumsum(k)])
    tbox = np.zeros((int(off[-1]), 6), F32)
    tbox[off[:-1][k == 1]] = ta.tri_boxes(v9)[k == 1]
    for kk in range(2, SPLIT_MAX + 1):
        rows = np.nonzero(k == kk)[0]
        if len(rows):
            tbox[(off[rows][:, None] + np.arange(kk)[None, :]).reshape(-1)] = split_slabs_of(v9[rows], kk, axis[rows]).reshape(-1, 6)
    return tbox, np.repeat(np.arange(n), k)


# ------------------------------------------------------------------------------------------------------------ hierarchy
class Hierarchy:
    """What the hierarchy stage hands to the emit stage: the primitive boxes, the primitive of every sorted position (val), the
    binary tree over the positions with its ranges, boxes and depths, and which algorithm made it."""


def prepare(verts, tris, algo, presplit=0, size_bits=9, radius=PLOC_RADIUS):
    """Everything of an attempt that does not depend on leaf_max: inputs, order, hierarchy (PLOC, or Karras when asked for, when
    there are two primitives, or when PLOC gives up)."""
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int64).reshape(-1, 3)
    if np.any(~np.isfinite(verts)) or len(tris) == 0:
        raise ValueError("empty mesh or non-finite vertex")
    H = Hierarchy()
    H.verts, H.n_orig = verts, len(tris)
    H.tris = np.concatenate([tris, tris]) if len(tris) == 1 else tris      # a lone triangle is doubled: the tree needs two leaves
    split = presplit_boxes(verts, tris, presplit)
    H.ref_tri = None if split is None else split[1]
    H.tbox = tri_boxes(verts, H.tris) if split is None else split[0]
    n = H.n = len(H.tbox)
    area32(H.tbox, "primitive box")
    H.keys = morton_keys(H.tbox, size_bits)
    H.val, H.sorted_keys = sort_keys(H.keys)
    leaf_box = H.tbox[H.val]
    made = ploc(leaf_box, radius) if algo == 1 and n > 2 else None
    H.ploc = made is not None
    if made is not None:
        H.left, H.right, H.nbox = made
        newpos, H.first, H.last = ploc_leaf_order(H.left, H.right)
        val = np.zeros(n, np.int64)
        val[newpos] = H.val
        H.val = val
        H.left = np.where(H.left < 0, ~newpos[np.maximum(~H.left, 0)], H.left)
        H.right = np.where(H.right < 0, ~newpos[np.maximum(~H.right, 0)], H.right)
        H.parent_i, H.parent_l, H.depth, H.leaf_depth = parents_and_depths(H.left, H.right)
    else:
        H.left, H.right, H.first, H.last = karras(H.sorted_keys)
        H.parent_i, H.parent_l, H.depth, H.leaf_depth = parents_and_depths(H.left, H.right)
        if int(H.depth.max()) + 1 > MAX_LEVELS:
            raise ValueError("tree deeper than 64 levels: pt_build_bvh refuses this mesh")
        H.nbox = fit(H.left, H.right, H.depth, leaf_box)
    H.max_depth = int(max(H.depth.max(), H.leaf_depth.max()))
    if H.max_depth > MAX_LEVELS:
        raise ValueError("tree deeper than 64 levels: pt_build_bvh refuses this mesh")
    return H


# ----------------------------------------------------------------------------------------------------------------- emit
def is_cut(H, c, leaf_max):
    """ptb_is_cut: inner node c becomes ONE leaf.  Never the root."""
    return c > 0 and int(H.last[c]) - int(H.first[c]) + 1 <= leaf_max


def last_flags(H, leaf_max):
    """k_records: record j ends a leaf when it is the last position of its topmost cut ancestor, or stands alone."""
    out = np.zeros(H.n, np.int32)
    for j in range(H.n):
        end, p = j, int(H.parent_l[j])
        while p > 0 and is_cut(H, p, leaf_max):
            end, p = int(H.last[p]), int(H.parent_i[p])
        out[j] = 1 if j == end else 0
    return out


def records(H, leaf_max):
    """The record section in sorted order: the triangle of every position (through ref_tri after a pre-split), its id
    min(t, n_orig - 1), the `last` flags; -0.0f -> +0.0f in v0.x only (encode_records)."""
    t = H.val if H.ref_tri is None else H.ref_tri[H.val]
    v9 = H.verts[H.tris[t]].reshape(-1, 9)
    return encode_records(v9, np.minimum(t, H.n_orig - 1).astype(np.int32), last_flags(H, leaf_max))


def child_box(H, c):
    return H.nbox[c] if c >= 0 else H.tbox[H.val[~c]]


def leaf_link(H, c, leaf_max):
    """(is a leaf, first position): ptb_child_is_leaf."""
    if c < 0:
        return True, ~c
    if is_cut(H, c, leaf_max):
        return True, int(H.first[c])
    return False, 0


def binary_nodes(H, leaf_max):
    """k_binary: one Compact node per inner node, the ones below a cut included."""
    n = H.n
    out = np.zeros((n - 1, 16), F32)
    oi = out.view(np.int32)
    rec_base = 4 * (n - 1)
    for i in range(n - 1):
        for k, c in enumerate((int(H.left[i]), int(H.right[i]))):
            b = child_box(H, c)
            out[i, 4 * k:4 * k + 4] = (b[0], b[3], b[1], b[4])
            out[i, 8 + 2 * k:10 + 2 * k] = (b[2], b[5])
            leaf, fp = leaf_link(H, c, leaf_max)
            oi[i, 12 + k] = ~(rec_base + 4 * fp) if leaf else 4 * c
    return out


def collapse_children(H, node, leaf_max):
    """k_collapse's choice for one inner node: the ordered list of up to four references it adopts."""
    ref = [int(H.left[node]), int(H.right[node])]
    while len(ref) < 4:
        best, ba = -1, F32(-1.0)
        for k, c in enumerate(ref):
            if leaf_link(H, c, leaf_max)[0]:
                continue
            ar = area32(child_box(H, c), "area in the collapse")
            if ar > ba:
                ba, best = ar, k
        if best < 0:
            break
        v = ref[best]
        ref[best] = ref[-1]
        ref.pop()
        ref += [int(H.left[v]), int(H.right[v])]
    return ref


def wide_nodes(H, leaf_max):
    """The 4-wide section level by level from (node 0, slot 0): (float32 [n_wide][16], wide depth).  Slots are handed out in the
    order the levels are walked."""
    n = H.n
    rec_base = 4 * (n - 1)
    wide_base = rec_base + 4 * n
    rows, frontier, levels = {}, [(0, 0)], 0
    n_slots = 1
    while frontier:
        levels += 1
        nxt = []
        for node, slot in frontier:
            ref = collapse_children(H, node, leaf_max)
            links = []
            for c in ref:
                leaf, fp = leaf_link(H, c, leaf_max)
                if leaf:
                    n_rec = 1 if c < 0 else int(H.last[c]) - int(H.first[c]) + 1
                    links.append(~((rec_base + 4 * fp) | (min(n_rec, 4) - 1)))
                else:
                    links.append(wide_base + 4 * n_slots)
                    nxt.append((c, n_slots))
                    n_slots += 1
            rows[slot] = encode_wide_node(np.array([child_box(H, c) for c in ref], F32), links)
        frontier = nxt
    return np.array([rows[s] for s in range(n_slots)], F32), levels


def emit(H, leaf_max):
    """(binary, records, wide, info, wide_depth) of a prepared hierarchy."""
    leaf_max = max(1, int(leaf_max))
    R = records(H, leaf_max)
    W, wide_depth = wide_nodes(H, leaf_max)
    info = dict(n_inner=H.n - 1, n_tri_refs=H.n, n_leaves=int(R.view(np.int32)[:, 7].sum()), max_depth=H.max_depth)
    return binary_nodes(H, leaf_max), R, W, info, wide_depth


def build(verts, tris, algo, leaf_max, presplit=0):
    """pt_build_bvh with PT_OPT_BUILD_ALGO algo, PT_OPT_LEAF_MAX leaf_max and PT_OPT_PRESPLIT presplit: three float32 [n][16]
    sections in the layout of pt_tree_items, info as pt_scene_info reports it (without device_bytes), the depth of the wide tree."""
    return emit(prepare(verts, tris, algo, presplit), leaf_max)


_prepared, _built = {}, {}


def cached_build(name, mesh_arrays, algo, leaf_max, presplit=0):
    """build() once per (name, options) for the whole run; mesh_arrays() -> (verts, tris) is called on a miss only."""
    hk = (name, algo, presplit)
    key = hk + (leaf_max,)
    if key not in _built:
        if hk not in _prepared:
            _prepared[hk] = prepare(*mesh_arrays(), algo, presplit)
        _built[key] = emit(_prepared[hk], leaf_max)
    return _built[key]


# ------------------------------------------------------------------------------------------------------------ tree cost
def tree_cost(wide, n_binary, n_records, records=None):
    """pt_tree_cost (include/ptmi.h) as k_tree_cost computes it: (node_visits, tri_tests).

    The definition is taken over the quantised boxes the walk decodes.  k_tree_cost does NOT decode the planes with the walk's
    fma(q, step, origin) and subtract: it takes every extent as (float)(hi byte - lo byte) * step, ONE binary32 product, and the
    root's box as the fminf / fmaxf of (float)byte * step over the axes that are not inverted.  That is restated here exactly; the
    areas 2 * (dx dy + dy dz + dz dx) and all sums are binary64, as in the kernel.  A leaf counts the records up to its `last` flag
    (at most 64); without `records` the count is the link's low two bits, refused where they say "four or more"."""
    W = np.ascontiguousarray(wide, F32).reshape(-1, 16)
    Wi = W.view(np.int32)
    rec_base = 4 * n_binary
    step = np.stack([W[:, 3], W[:, 14], W[:, 15]], 1)                                    # [node][axis]
    k8 = 8 * np.arange(4)
    ql = (Wi[:, 4:7].astype(np.int64)[:, None, :] >> k8[None, :, None]) & 255            # [node][slot][axis]
    qh = (Wi[:, 7:10].astype(np.int64)[:, None, :] >> k8[None, :, None]) & 255
    used = np.all(ql <= qh, axis=2)
    with np.errstate(all="ignore"):
        d = ((qh - ql).astype(F32) * step[:, None, :]).astype(np.float64)
    area = 2.0 * ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0])
    links = Wi[:, 10:14]
    inner_terms = area[used & (links >= 0)]
    counts = np.zeros(links.shape, np.int64)
    leaf = used & (links < 0)
    r = ~links.astype(np.int64)
    if records is None:
        if np.any((r & 3)[leaf] == 3):
            raise ValueError("tree_cost: a leaf of four or more records; pass the records")
        counts[leaf] = (r & 3)[leaf] + 1
    else:
        last = np.ascontiguousarray(records, F32).reshape(-1, 16).view(np.int32)[:, 7]
        for w, k in zip(*np.nonzero(leaf)):
            j, c = ((int(r[w, k]) & ~3) - rec_base) // 4, 0
            while True:
                c += 1
                if last[j + c - 1] != 0 or c >= 64:
                    break
            counts[w, k] = c
    leaf_terms = area[leaf] * counts[leaf].astype(np.float64)
    # the root: node 0, over every axis of every slot that is not inverted on that axis
    ok = ql[0] <= qh[0]
    lo = np.where(ok, ql[0].astype(F32) * step[0][None, :], F32(3.0e38)).astype(F32).min(0)
    hi = np.where(ok, qh[0].astype(F32) * step[0][None, :], F32(-3.0e38)).astype(F32).max(0)
    e = (hi - lo).astype(F32).astype(np.float64)
    root = 2.0 * ((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0])
    if not root > 0:
        raise ValueError("tree_cost: degenerate root box")
    return (root + float(np.sum(inner_terms))) / root, float(np.sum(leaf_terms)) / root


def cost_terms(wide):
    """How many area terms tree_cost adds for (node_visits, tri_tests): the sizes of the rounding bound of a reordered sum."""
    Wi = np.ascontiguousarray(wide, F32).reshape(-1, 16).view(np.int32)
    k8 = 8 * np.arange(4)
    ql = (Wi[:, 4:7].astype(np.int64)[:, None, :] >> k8[None, :, None]) & 255
    qh = (Wi[:, 7:10].astype(np.int64)[:, None, :] >> k8[None, :, None]) & 255
    used = np.all(ql <= qh, axis=2)
    return int((used & (Wi[:, 10:14] >= 0)).sum()) + 1, int((used & (Wi[:, 10:14] < 0)).sum())


# ------------------------------------------------------------------------------------------------- where two trees differ
def first_difference(got, want):
    """The first stage at which two (binary, records, wide) triples differ, as one line; None when their canonical forms are equal.
    Stages in the builder's order: record order, `last` flags, record words, binary topology, binary boxes, wide nodes."""
    if ta.canonical_form(*got) == ta.canonical_form(*want):
        return None
    (gb, gr, gw), (wb, wr, ww) = ([np.ascontiguousarray(x, F32).reshape(-1, 16) for x in t] for t in (got, want))
    if len(gr) != len(wr) or len(gb) != len(wb):
        return f"sizes: {len(gb)} binary nodes / {len(gr)} records, expected {len(wb)} / {len(wr)}"
    gi, wi = gr.view(np.int32), wr.view(np.int32)
    for what, col in (("record order (triangle ids)", 3), ("`last` flags (the cut rule)", 7)):
        off = np.nonzero(gi[:, col] != wi[:, col])[0]
        if len(off):
            j = int(off[0])
            return f"{what}: {len(off)} of {len(gr)} records differ, first record {j}: {gi[j, col]}, expected {wi[j, col]}"
    if not np.array_equal(gi, wi):
        j = int(np.nonzero(np.any(gi != wi, axis=1))[0][0])
        return f"record words: record {j} (id {gi[j, 3]}) differs in words {np.nonzero(gi[j] != wi[j])[0].tolist()}"
    cg = ta._renumbered(gb, (12, 13), 0, lambda row: 2)
    cw = ta._renumbered(wb, (12, 13), 0, lambda row: 2)
    if len(cg) != len(cw) or not np.array_equal(cg.view(np.int32)[:, 12:14], cw.view(np.int32)[:, 12:14]):
        m = min(len(cg), len(cw))
        off = np.nonzero(np.any(cg.view(np.int32)[:m, 12:14] != cw.view(np.int32)[:m, 12:14], axis=1))[0]
        at = int(off[0]) if len(off) else m
        return f"binary topology: {len(cg)} reachable nodes, expected {len(cw)}; first difference at depth-first node {at}"
    if not np.array_equal(cg.view(np.int32), cw.view(np.int32)):
        off = np.nonzero(np.any(cg.view(np.int32) != cw.view(np.int32), axis=1))[0]
        i = int(off[0])
        return f"binary boxes: {len(off)} of {len(cg)} nodes differ, first depth-first node {i}: {cg[i, :12].tolist()}, expected {cw[i, :12].tolist()}"
    base = 4 * (len(gb) + len(gr))
    cg, cw = ta._renumbered(gw, (10, 11, 12, 13), base, ta._wide_children), ta._renumbered(ww, (10, 11, 12, 13), base, ta._wide_children)
    m = min(len(cg), len(cw))
    off = np.nonzero(np.any(cg.view(np.int32)[:m] != cw.view(np.int32)[:m], axis=1))[0]
    at = int(off[0]) if len(off) else m
    words = np.nonzero(cg.view(np.int32)[at] != cw.view(np.int32)[at])[0].tolist() if at < m else []
    return f"wide nodes: {len(cg)} reachable, expected {len(cw)}; first difference at depth-first node {at}, words {words}"


# ---------------------------------------------------------------------------------------------------------------- cases
SOUP_SIZES = (1, 2, 3, 4, 5, 16, 17, 18, 255, 256, 257, 1000)


def _tri_cloud(rng, n, size, lo=0.0, hi=1.0):
    c = rng.uniform(lo, hi, (n, 1, 3))
    return c + rng.uniform(-size, size, (n, 3, 3))


def case_soup(name):
    """The synthetic meshes of the builder tests as float32 [n][9] soups (read-only), each the smallest at which a rule can go
    wrong; see tests/test_gpu_build_ref.py for what each one reaches."""
    if name not in _CASES:
        _CASES[name] = np.ascontiguousarray(_make_case(name), F32).reshape(-1, 9)
        _CASES[name].setflags(write=False)
    return _CASES[name]


_CASES = {}


def _make_case(name):
    if name.startswith("soup-"):
        n = int(name[5:])
        s = _tri_cloud(np.random.default_rng(1000 + n), n, 0.08)
        if n >= 255:
            # the extreme centres sit in the last, partly filled block of k_tri_bounds' reduction (rows n - 2 and n - 1)
            s[n - 1] = s[n - 1] - s[n - 1].mean(0) + [1.25, 1.25, -0.25]
            s[n - 2] = s[n - 2] - s[n - 2].mean(0) + [-0.25, -0.25, 1.25]
        return s
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "pairs":
        s = _tri_cloud(rng, 400, 0.05)
        return np.concatenate([s, s[::5]])                       # every fifth triangle again, exactly, 400 rows and more away
    if name == "flat":
        s = _tri_cloud(rng, 120, 0.06)
        s[:, :, 1] = 0.375
        return s
    if name in ("co-centred", "co-centred-far"):
        # lo / hi are 0.5 -+ r on every axis with r a multiple of 2^-9: exact in binary32, so every box centre is 0.5 exactly.
        # Forty such triangles alone have no centre extent: rel is 0 and all keys are EQUAL (told apart by position only);
        # "-far" adds one distant triangle, which gives the centres an extent, and then only the size bits differ among the forty.
        r = ((1 + np.arange(40)) / 512.0)[:, None, None]
        d = np.array([[1.0, 1.0, 1.0], [-1.0, 0.5, -1.0], [0.25, -1.0, 0.5]])[None]
        s = 0.5 + r * d
        far = np.array([[[3.0, 3.0, 3.0], [3.0625, 3.0, 3.0], [3.0, 3.0625, 3.03125]]])
        return s if name == "co-centred" else np.concatenate([s, far])
    if name == "two-scales":
        walls = _tri_cloud(rng, 24, 0.9, 0.3, 0.7)
        size = 0.0004 * 2.0 ** rng.uniform(0, 9.5, (2000, 1, 1))
        tiny = rng.uniform(0.2, 0.8, (2000, 1, 3)) + size * rng.uniform(-1, 1, (2000, 3, 3))
        return np.concatenate([walls, tiny])
    if name == "window":
        # Eighteen boxes whose centres lie on the x axis in row order (no centre extent on y and z, every size clamped: the key is x
        # alone).  Rows 0, 8 and 17 are thin sticks along x, the others plates 16 x 16 across: a stick's union with a plate is huge,
        # with another stick small.  Stick 8 is 8 places from stick 0 and 9 from stick 17, which is nearer in x: a window of 8 merges
        # (0, 8) in the first round, a window of 7 merges neither, a window of 9 merges (8, 17).
        cx = np.array([0] + list(range(32, 39)) + [48] + list(range(49, 57)) + [57]) / 64.0
        s = np.zeros((18, 3, 3))
        for k, c in enumerate(cx):
            h = 2.0 ** -11 if k in (0, 8, 17) else 8.0
            s[k] = [[c - 0.625, -h, -h], [c + 0.625, h, h], [c, h, -h]]
        return s
    if name == "at-the-max":
        s = _tri_cloud(rng, 90, 0.05)
        for a in range(3):                                       # one triangle per axis holds the largest centre coordinate
            s[7 + 31 * a, :, a] += 1.5
        return s
    if name == "minus-zero":
        s = _tri_cloud(rng, 60, 0.5, -0.5, 0.5)
        s[::3, 0, 0] = -0.0
        s[1::3, :, 2] = -0.0
        s[2::5, 1, :] = -0.0
        s[5] = [[-0.0, -0.0, -0.0], [0.0, 1.0, 0.0], [-0.0, 0.0, 1.0]]
        s[6] = [[0.5, -0.0, 0.25], [-0.0, -0.0, -0.5], [-0.0, 0.25, -0.0]]
        return s
    raise KeyError(name)


SYNTHETIC = tuple(f"soup-{n}" for n in SOUP_SIZES) + ("window", "pairs", "flat", "co-centred", "co-centred-far", "two-scales", "at-the-max", "minus-zero")


def soup_arrays(soup):
    """(verts, tris) of a soup, as gpu_support.soup_mesh lays them out: triangle t is vertices 3t, 3t + 1, 3t + 2."""
    s = np.ascontiguousarray(soup, F32).reshape(-1, 9)
    return s.reshape(-1, 3), np.arange(3 * len(s), dtype=np.int32).reshape(-1, 3)
