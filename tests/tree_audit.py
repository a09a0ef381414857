"""tree_audit — reads the item buffer of an acceleration structure ([binary nodes][records][wide nodes]) item by
item and checks it against the exact geometry.  numpy only: no GPU, no library of the project.

    audit(binary, records, wide, info, soup, wide_depth=..., ...) -> [Violation(kind, item, what), ...]      ([] = pass)
    canonical_form(binary, records, wide) -> bytes         (equal for two trees that differ only in how their nodes are numbered)

Everything is exact: the trees are deterministic data.  fma32 is the one piece of arithmetic numpy lacks — a fused multiply-add
rounded ONCE to binary32; it is computed in rational arithmetic.  fma32_fast runs a vector through binary64 and sends to fma32
every element whose binary64 sum sits exactly on a binary32 tie (or below the normal range, or is not finite): ties are binary64
numbers and rounding is monotonic, so a binary64 sum that is NOT a tie lies on the same side of every tie as the exact sum and
rounds to the same binary32.  The fast path therefore returns fma32's bits for every input, at any triangle count.

The encoders of csrc/pt_items.h are restated here (encode_records, encode_wide_node), and emit()'s Woop record of
csrc/pt_scene_build.h (encode_woop_records): float64 where the C uses double, fma32
where it uses fmaf, numpy's binary32 operators (one IEEE rounding each) for the rest.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

Violation = namedtuple("Violation", "kind item what")

F32_MIN_NORMAL = np.float32(2.0 ** -126)
_EMPTY = np.array([3.402823466e+38] * 3 + [-3.402823466e+38] * 3, np.float32)


# ------------------------------------------------------------------------------------------------------------ arithmetic
def round_f32(x):
    """A rational number rounded once to the nearest binary32, ties to even (overflow: infinity; zero: +0)."""
    x = Fraction(x)
    if x == 0:
        return np.float32(0.0)
    sign = -1.0 if x < 0 else 1.0
    n, d = abs(x).numerator, abs(x).denominator
    e = n.bit_length() - d.bit_length()            # floor(log2 |x|) is e or e - 1
    if (n < (d << e)) if e >= 0 else ((n << -e) < d):
        e -= 1
    eq = max(e, -126) - 23                         # exponent of the last place (subnormals share -149)
    num, den = (n, d << eq) if eq >= 0 else (n << -eq, d)
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    if q.bit_length() + eq > 128:
        return np.float32(sign * math.inf)
    return np.float32(sign * math.ldexp(q, eq))     # q < 2^25: exact in binary64 and, being a binary32 value, in the cast


def fma32(a, b, c):
    """a * b + c with ONE rounding to binary32 (fmaf).  Finite inputs; an exact zero is +0 unless the product and c are both -0."""
    a, b, c = float(np.float32(a)), float(np.float32(b)), float(np.float32(c))
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))   # infinities and NaN need no rounding
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
        return np.float32(-0.0 if neg and a * b == 0 and c == 0 else 0.0)
    return round_f32(s)


def fma32_fast(a, b, c):
    """fma32 over arrays (broadcast): binary64 where that is provably the same, fma32 for the rest (module docstring)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    if a.ndim == 0:
        return fma32_fast(a[None], b[None], c[None])[0]
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)   # the product is exact (48 bits), the sum rounds once
        out = s.astype(np.float32)
    bits = np.ascontiguousarray(s).view(np.int64)
    # (an exact zero needs no second look: the product is exact and a binary64 sum is zero only when the exact sum is, with IEEE's sign)
    redo = ((bits & ((1 << 29) - 1)) == (1 << 28)) | ~np.isfinite(s) | ((np.abs(s) < 2.0 ** -125) & (s != 0)) | ~np.isfinite(out)
    out = np.array(out, np.float32)
    for i in zip(*np.nonzero(redo)):
        out[i] = fma32(a[i], b[i], c[i])
    return out


def _min32(a, b):
    """fminf / fmaxf on the device order -0 below +0 (IEEE 754-2019 minimum); numpy does not promise it."""
    r = np.minimum(a, b)
    z = (a == 0) & (b == 0)
    return np.where(z & (np.signbit(a) | np.signbit(b)), np.float32(-0.0), r).astype(np.float32)


def _max32(a, b):
    r = np.maximum(a, b)
    z = (a == 0) & (b == 0)
    return np.where(z & ~(np.signbit(a) & np.signbit(b)), np.float32(0.0), r).astype(np.float32)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# -------------------------------------------------------------------------------------------------------------- encoders
def encode_records(v, ids, last):
    """pt_encode_record over rows v (float32 [n][9]) with k_records' -0.0 -> +0.0 in v0.x: float32 [n][16]."""
    v = np.array(v, np.float32).reshape(-1, 9)
    v[:, 0] = np.where(v[:, 0] == 0, np.float32(0.0), v[:, 0])
    v0, v1, v2 = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    out = np.zeros((len(v), 16), np.float32)
    with np.errstate(all="ignore"):
        a, b = v0 - v1, v0 - v2
        out[:, 0:3], out[:, 4:7], out[:, 8:11] = v0, v1 - v0, v2 - v0
        for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            out[:, 12 + k] = fma32_fast(a[:, i], b[:, j], -(a[:, j] * b[:, i]))
    o = out.view(np.int32)
    o[:, 3], o[:, 7] = ids, last
    return out


def encode_woop_records(v, ids, last):
    """emit()'s Woop record (csrc/pt_scene_build.h, PT_OPT_TRI_TEST 1) over rows v (float32 [n][9], v0.x's -0.0 -> +0.0 as the host
    tree stores it): float32 [n][16] = [row z, -translation z][row x, translation x][row y, translation y][N, id << 1 | last].
    The rows are those of M^-1, M = columns (a, b, n, v2), a = v0 - v2, b = v1 - v2, n = a x b: (b x n, n x a, n) / |n|^2, every
    step in binary64 in emit()'s own order (its translation unit is compiled without contraction), rounded once to binary32; a
    triangle with |n|^2 == 0 gets zero rows.  N = cross(v0 - v1, v0 - v2) in the kernels' vcross arithmetic, as in encode_records."""
    v = np.array(v, np.float32).reshape(-1, 9)
    v[:, 0] = np.where(v[:, 0] == 0, np.float32(0.0), v[:, 0])
    out = np.zeros((len(v), 16), np.float32)
    out[:, 12:15] = encode_records(v, 0, 0)[:, 12:15]
    d = v.astype(np.float64)
    v0, v1, v2 = d[:, 0:3], d[:, 3:6], d[:, 6:9]

    def cross(p, q):
        return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)

    with np.errstate(all="ignore"):
        A, B = v0 - v2, v1 - v2
        n = cross(A, B)
        nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        ok = (nn > 0.0)[:, None]
        den = np.where(ok, nn[:, None], 1.0)
        rows = [np.where(ok, r / den, 0.0) for r in (cross(B, n), cross(n, A), n)]
        tr = [-(r[:, 0] * v2[:, 0] + r[:, 1] * v2[:, 1] + r[:, 2] * v2[:, 2]) for r in rows]
        out[:, 0:3], out[:, 3] = rows[2], -tr[2]
        out[:, 4:7], out[:, 7] = rows[0], tr[0]
        out[:, 8:11], out[:, 11] = rows[1], tr[1]
    out.view(np.int32)[:, 15] = (np.asarray(ids, np.int64) << 1 | np.asarray(last, np.int64)).astype(np.int32)
    return out


def _ordered_bits(x):
    i = _bits(x).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def tri_boxes(v):
    """min / max of the three vertices, as k_tri_bounds and k_refit_records take them: float32 [n][6] lo xyz, hi xyz."""
    v = np.asarray(v, np.float32).reshape(-1, 3, 3)
    return np.concatenate([_min32(v[:, 0], _min32(v[:, 1], v[:, 2])), _max32(v[:, 0], _max32(v[:, 1], v[:, 2]))], 1)


def encode_wide_node(boxes, links):
    """pt_encode_wide_node: boxes float32 [n][6] (lo xyz, hi xyz) of the n = 1..4 children, their links -> 16 words (float32)."""
    cb = np.asarray(boxes, np.float32).reshape(-1, 6)
    n = len(cb)
    lo, hi = cb[0, :3].copy(), cb[0, 3:].copy()
    for k in range(1, n):
        for a in range(3):
            if cb[k, a] < lo[a]:
                lo[a] = cb[k, a]
            if cb[k, 3 + a] > hi[a]:
                hi[a] = cb[k, 3 + a]
    tiny = F32_MIN_NORMAL
    one16 = np.float32(1.0) + np.float32(1.0 / 65536.0)
    q = [0] * 6
    scales = []
    with np.errstate(all="ignore"):
        for a in range(3):
            origin, ext = lo[a], np.float32(hi[a] - lo[a])
            scale = tiny
            if ext > 0:
                scale = np.float32((float(ext) / 255.0) * (1.0 + 1.0 / 262144.0))
                if not scale >= tiny:
                    scale = tiny
                guard = 0
                while fma32(255.0, scale, origin) < hi[a]:
                    scale = np.float32(scale * one16)
                    guard += 1
                    if guard > 4096:
                        raise ArithmeticError("encode_wide_node: the grid step does not reach the upper bound")
            scales.append(scale)
            for k in range(4):
                qlo, qhi = 255, 0
                if k < n:
                    fl = math.floor((float(cb[k, a]) - float(origin)) / float(scale))
                    ce = math.ceil((float(cb[k, 3 + a]) - float(origin)) / float(scale))
                    qlo, qhi = int(min(max(fl, 0), 255)), int(min(max(ce, 0), 255))
                    while qlo > 0 and fma32(qlo, scale, origin) > cb[k, a]:
                        qlo -= 1
                    while qhi < 255 and fma32(qhi, scale, origin) < cb[k, 3 + a]:
                        qhi += 1
                q[a] |= qlo << (8 * k)
                q[3 + a] |= qhi << (8 * k)
    d = np.zeros(16, np.float32)
    di = d.view(np.uint32)
    d[0:3], d[3], d[14], d[15] = lo, scales[0], scales[1], scales[2]
    di[4:10] = q
    d.view(np.int32)[10:14] = [links[k] if k < n else links[0] for k in range(4)]
    return d


# ----------------------------------------------------------------------------------------------------------- test points
# s / k of every slab plane, in binary64 and as k_split_emit computes it in binary32
_SLAB_FRACTIONS = np.array(sorted({f for k in range(2, 9) for s in range(1, k) for f in (s / k, float(np.float32(s) / np.float32(k)))}))
def triangle_points(v9):
    """The fixed points of one triangle that coverage asks for (float64 [m][3], clamped to the triangle's float32 box):
    vertices, edge midpoints, centroid, a 6 x 6 barycentric lattice and the edge crossings of every pre-split slab plane
    lo + ext * s / k (k = 2..8, the longest axis: ptb_split_count)."""
    v = np.asarray(v9, np.float32).reshape(3, 3).astype(np.float64)
    pts = [v[0], v[1], v[2], (v[0] + v[1]) / 2, (v[1] + v[2]) / 2, (v[2] + v[0]) / 2, (v[0] + v[1] + v[2]) / 3]
    for i in range(6):
        for j in range(6):
            u, w = (i + 0.5) / 6, (j + 0.5) / 6
            if u + w > 1:
                u, w = 1 - u, 1 - w
            pts.append(v[0] + u * (v[1] - v[0]) + w * (v[2] - v[0]))
    lo, hi = v.min(0), v.max(0)
    ax = int(np.argmax(hi - lo))
    pts = np.array(pts)
    if hi[ax] > lo[ax]:
        X = lo[ax] + (hi[ax] - lo[ax]) * _SLAB_FRACTIONS
        for e in range(3):
            a, b = v[e], v[(e + 1) % 3]
            x = X[(X > min(a[ax], b[ax])) & (X < max(a[ax], b[ax]))]
            if len(x):
                p = a + ((x - a[ax]) / (b[ax] - a[ax]))[:, None] * (b - a)
                p[:, ax] = x
                pts = np.concatenate([pts, p])
    return np.clip(pts, lo, hi)


# ------------------------------------------------------------------------------------------------------- canonical form
def _renumbered(A, link_words, base, n_children):
    """The rows of A reachable from row 0 in depth-first order (children in the order of link_words), every inner link
    (>= 0: base + 4 * row) rewritten to the new numbers; leaf links (< 0) untouched."""
    Ai = A.view(np.int32)
    new, order, stack = {}, [], [0]
    while stack:
        i = stack.pop()
        if i in new:
            raise ValueError(f"row {i} is reached twice")
        new[i] = len(order)
        order.append(i)
        kids = [(int(Ai[i, w]) - base) // 4 for w in link_words[:n_children(Ai[i])] if Ai[i, w] >= 0]
        stack.extend(reversed(kids))
    out = A[order].copy()
    Oi = out.view(np.int32)
    for w in link_words:
        inner = Oi[:, w] >= 0
        Oi[inner, w] = [base + 4 * new[(int(x) - base) // 4] for x in Oi[inner, w]]
    return out


def _wide_children(row):
    n = 1
    while n < 4 and row[10 + n] != row[10]:
        n += 1
    return n


def canonical_form(binary, records, wide):
    """The bytes of a tree up to the numbering of its nodes.  The device builder hands out inner-node numbers (k_ploc_merge) and
    wide slots (k_collapse) from atomic counters, so they depend on scheduling; topology, child order and record order do not.
    The form is the record section as it is, the binary nodes renumbered depth-first from node 0 (child 0 before child 1), the
    wide nodes renumbered depth-first from slot 0 (children in slot order), every node link rewritten to the new numbers and
    every leaf link untouched.  Nodes that no link reaches (below the multi-record leaves of a device-built tree: ptb_is_cut)
    have no place in that order and are left out."""
    B, R, W = (np.ascontiguousarray(x, np.float32).reshape(-1, 16) for x in (binary, records, wide))
    return (R.tobytes() + _renumbered(B, (12, 13), 0, lambda row: 2).tobytes()
            + _renumbered(W, (10, 11, 12, 13), 4 * (len(B) + len(R)), _wide_children).tobytes())


# ---------------------------------------------------------------------------------------------------------------- audit
def _bin_child_box(node, k):
    return np.array([node[4 * k], node[4 * k + 2], node[8 + 2 * k], node[4 * k + 1], node[4 * k + 3], node[9 + 2 * k]], np.float32)


def _empty(b):
    return not b[0] <= b[3]


def _union(a, b):
    if _empty(a):
        return b.copy()
    if _empty(b):
        return a.copy()
    return np.concatenate([_min32(a[:3], b[:3]), _max32(a[3:], b[3:])])


def _fill_empty(boxes):
    """The refit's rule (ptr_fill_empty): an empty child becomes a point box at the first non-empty sibling's lower corner."""
    p = np.zeros(3, np.float32)
    for b in boxes:
        if not _empty(b):
            p = b[:3]
            break
    return [np.concatenate([p, p]) if _empty(b) else b for b in boxes]


def _inside(outer, inner):
    return _empty(inner) or bool(np.all(outer[:3] <= inner[:3]) and np.all(outer[3:] >= inner[3:]))


def audit(binary, records, wide, info, soup, wide_depth, leaf_max=0, split_refs=False, strict=False, coverage=False,
          cut_subtrees=False, depth_exact=True, woop=False, dropped=None, max_violations=40, stats=None):
    """binary / records / wide: float32 [n][16] (PathTracer.tree_items); info: pt_scene_info's dict (n_inner, n_tri_refs, n_leaves,
    max_depth); soup: float32 [n][9] by original id; wide_depth: the accessor's.
      split_refs    a triangle may be listed by several leaves whose boxes hold only a part of it (host SBVH, PT_OPT_PRESPLIT):
                    ids may repeat and a leaf's box need not hold its triangles — `coverage` checks what such a tree owes
      strict        every binary child box and every wide node equal the restated encoders over the exact boxes, bit for bit
      cut_subtrees  a device-built tree: the binary section keeps the nodes below its multi-record leaves (ptb_is_cut, pt_build.h),
                    unreachable, and n_inner is the size of the section
      depth_exact   max_depth equals the walked depth (False: it bounds it — k_depth, pt_build.h, counts the cut-off levels too)
      woop          Woop records (PT_OPT_TRI_TEST 1): the records are audited against encode_woop_records and against the triangle's
                    own vertices (below); the node part as for any tree; no coverage
      stats         a dict that receives counts which are recorded, not judged (woop_floats, woop_floats_differ)
      dropped       bool [n] by id: triangles a refit dropped (zero vertices in the record, nothing in any box)
    """
    V = []

    def bad(kind, item, what):
        if len(V) < max_violations:
            V.append(Violation(kind, item, what))

    B, R, W = (np.ascontiguousarray(x, np.float32).reshape(-1, 16) for x in (binary, records, wide))
    Bi, Ri, Wi = B.view(np.int32), R.view(np.int32), W.view(np.int32)
    nb, nr, nw = len(B), len(R), len(W)
    soup = np.asarray(soup, np.float32).reshape(-1, 9)
    rec_base, wide_base = 4 * nb, 4 * (nb + nr)
    if nb == 0 or nr == 0 or nw == 0:
        return [Violation("shape", "tree", "an empty section")]
    dropped = np.zeros(len(soup), bool) if dropped is None else np.asarray(dropped, bool)

    # ---- record runs: what the `last` flags delimit
    last = (Ri[:, 15] & 1) if woop else Ri[:, 7]
    if not woop and not np.all((last == 0) | (last == 1)):
        bad("record", "records", "a `last` word that is neither 0 nor 1")
    ends = np.nonzero(last != 0)[0]
    if len(ends) == 0 or ends[-1] != nr - 1:
        bad("partition", f"record {nr - 1}", "the last record does not end a leaf")
    starts = np.concatenate([[0], ends[:-1] + 1]) if len(ends) else np.array([0])
    run_len = dict(zip(starts.tolist(), (ends - starts + 1).tolist())) if len(ends) else {0: nr}

    def leaf_of(r, item):
        """float4 index of a leaf's first record -> record number, or None."""
        off = r - rec_base
        if off < 0 or off % 4 or off // 4 >= nr:
            bad("shape", item, f"leaf link {r} does not point at a record")
            return None
        if off // 4 not in run_len:
            bad("partition", item, f"leaf link points at record {off // 4}, inside the run of another leaf")
            return None
        return off // 4

    # ---- records against the soup
    ids = Ri[:, 15] >> 1 if woop else Ri[:, 3]
    live = ids >= 0
    if np.any(ids[live] >= len(soup)):
        bad("ids", "records", "an id beyond the caller's triangles")
        return V
    tbox = np.tile(_EMPTY, (nr, 1))
    if not woop:
        vv = soup[np.maximum(ids, 0)].copy()
        vv[dropped[np.maximum(ids, 0)]] = 0
        want = encode_records(vv, ids, last)
        want[~live] = 0
        want.view(np.int32)[~live, 3], want.view(np.int32)[~live, 7] = -1, 1
        for j in np.nonzero(np.any(_bits(want) != Ri, axis=1))[0]:
            w = np.nonzero(_bits(want[j]) != Ri[j])[0]
            bad("record", f"record {j}", f"id {ids[j]}: words {w.tolist()} are {R[j, w].tolist()}, pt_encode_record gives {want[j, w].tolist()}")
    else:
        # Woop records.  (1) The stored rows, taken in binary64, send the triangle's own vertices to (1,0,0), (0,1,0), (0,0,0).
        # Each stored entry is its exact value within 2^-24 relative (one rounding of a binary64 value to binary32), and the exact rows
        # satisfy the identity exactly, so |row . v + translation - target| <= 2^-24 * (sum |row_i v_i| + |translation|).
        # (2) Every float is within 1 ulp of the restated encoder's (bit-equality is the expectation: stats["woop_floats_differ"]
        # counts the floats that are not); N and the id / last word are equal bit for bit; an empty leaf's record is zero rows with
        # the word -1.
        vv = soup[np.maximum(ids, 0)].copy()
        vv[:, 0] = np.where(vv[:, 0] == 0, np.float32(0.0), vv[:, 0])
        want = encode_woop_records(vv, ids, last)
        want[~live, :15] = 0
        R64, v64 = R.astype(np.float64), vv.astype(np.float64).reshape(-1, 3, 3)
        target = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])     # [vertex][row x, row y, row z]
        flat = ~np.any(want[:, 0:12].view(np.int32) & 0x7FFFFFFF, axis=1)         # zero rows: a triangle without area
        for k, (c, sign) in enumerate(((4, 1.0), (8, 1.0), (0, -1.0))):
            prod = R64[:, None, c:c + 3] * v64                                      # [record][vertex][axis]
            val = prod.sum(2) + sign * R64[:, None, c + 3]
            bound = 2.0 ** -24 * (np.abs(prod).sum(2) + np.abs(R64[:, None, c + 3]))
            off = live[:, None] & ~flat[:, None] & ~(np.abs(val - target[None, :, k]) <= bound)
            for j, i in zip(*np.nonzero(off)):
                bad("woop-rows", f"record {j}", f"id {ids[j]}: row {'xyz'[k]} sends vertex {i} to {val[j, i]!r}, not to {target[i, k]} within {bound[j, i]:.3e}")
        ulps = np.abs(_ordered_bits(want[:, :12]) - _ordered_bits(R[:, :12]))
        if stats is not None:
            stats["woop_floats"] = stats.get("woop_floats", 0) + int(ulps.size)
            stats["woop_floats_differ"] = stats.get("woop_floats_differ", 0) + int((_bits(want[:, :12]) != Ri[:, :12]).sum())
        for j in np.nonzero(np.any((ulps > 1) | ~np.isfinite(R[:, :12]), axis=1))[0]:
            w = np.nonzero((ulps[j] > 1) | ~np.isfinite(R[j, :12]))[0]
            bad("woop-record", f"record {j}", f"id {ids[j]}: floats {w.tolist()} are {R[j, w].tolist()}, emit()'s rows give {want[j, w].tolist()}")
        for j in np.nonzero(np.any(_bits(want[:, 12:16]) != Ri[:, 12:16], axis=1))[0]:
            bad("woop-record", f"record {j}", f"id {ids[j]}: N / id << 1 | last are {Ri[j, 12:16].tolist()}, expected {_bits(want[j, 12:16]).tolist()}")
    geo = live & ~dropped[np.maximum(ids, 0)]
    tbox[geo] = tri_boxes(soup[ids[geo]])
    seen_ids = np.bincount(ids[live], minlength=len(soup))
    if np.any(seen_ids == 0):
        bad("ids", "records", f"triangles {np.nonzero(seen_ids == 0)[0][:8].tolist()} are in no leaf")
    if not split_refs and np.any(seen_ids > 1) and not (len(soup) == 1 and nr == 2):   # (pt_build_bvh doubles a lone triangle)
        bad("ids", "records", f"triangles {np.nonzero(seen_ids > 1)[0][:8].tolist()} are listed more than once")

    def run_box(j):
        b = _EMPTY.copy()
        for r in range(j, j + run_len[j]):
            b = _union(b, tbox[r])
        return b

    # ---- binary tree
    inf6 = np.array([-np.inf] * 3 + [np.inf] * 3)
    seen = np.zeros(nb, bool)
    seen[0] = True
    leaves = {}            # first record -> dict(depth, stored box, path box of the binary tree)
    kids = {}              # node -> [(is_leaf, index, stored box)]
    order = []
    stack = [(0, 0, inf6)]
    depth_bin = 0
    while stack:
        i, d, path = stack.pop()
        order.append(i)
        kids[i] = []
        for k in range(2):
            link, item = int(Bi[i, 12 + k]), f"binary node {i} child {k}"
            box = _bin_child_box(B[i], k)
            p = np.concatenate([np.maximum(path[:3], box[:3]), np.minimum(path[3:], box[3:])])
            if link >= 0:
                if link % 4 or link // 4 >= nb:
                    bad("shape", item, f"inner link {link} is out of range or not aligned")
                elif seen[link // 4]:
                    bad("shape", item, f"node {link // 4} is reached twice")
                else:
                    seen[link // 4] = True
                    kids[i].append((False, link // 4, box))
                    stack.append((link // 4, d + 1, p))
            else:
                j = leaf_of(~link, item)
                if j is None:
                    continue
                if j in leaves:
                    bad("partition", item, f"the leaf at record {j} is linked twice")
                    continue
                leaves[j] = dict(depth=d + 1, box=box, path=p)
                kids[i].append((True, j, box))
                depth_bin = max(depth_bin, d + 1)
                if leaf_max and run_len[j] > leaf_max:
                    bad("leaf-size", item, f"{run_len[j]} records in a leaf, PT_OPT_LEAF_MAX is {leaf_max}")
    for j in sorted(set(run_len) - set(leaves)):
        bad("partition", f"record {j}", f"the run of {run_len[j]} records is in no leaf of the binary tree (orphan)")
    n_reached = int(seen.sum())
    if not cut_subtrees and n_reached != nb:
        bad("shape", "binary nodes", f"{nb - n_reached} nodes are not reachable, first {np.nonzero(~seen)[0][:4].tolist()}")
    if info["n_inner"] != (nb if cut_subtrees else n_reached):
        bad("counts", "n_inner", f"reported {info['n_inner']}, the tree has {nb if cut_subtrees else n_reached}")
    if info["n_tri_refs"] != nr:
        bad("counts", "n_tri_refs", f"reported {info['n_tri_refs']}, the tree has {nr}")
    if info["n_leaves"] != len(leaves):
        bad("counts", "n_leaves", f"reported {info['n_leaves']}, the walk counts {len(leaves)}")
    if depth_bin > 64 or info["max_depth"] > 64:
        bad("depth", "max_depth", f"depth {depth_bin} / reported {info['max_depth']} exceeds 64")
    if (info["max_depth"] != depth_bin) if depth_exact else (info["max_depth"] < depth_bin):
        bad("depth", "max_depth", f"reported {info['max_depth']}, the walk finds {depth_bin}")

    # exact boxes bottom-up; containment and the strict rule
    exact_bin = {}
    for i in reversed(order):
        ex, stored = [], []
        for is_leaf, c, box in kids[i]:
            if is_leaf:
                e = run_box(c)
                leaves[c]["exact"] = e
                inner = e if not split_refs else _EMPTY
            else:
                e = exact_bin[c]
                inner = _EMPTY.copy()
                if not _empty(e):       # (below a subtree a refit dropped entirely the boxes are unrelated points: ptr_fill_empty)
                    for _, _, cbox in kids[c]:
                        inner = _union(inner, cbox)
            what = f"records {c}.." if is_leaf else f"node {c}"
            if not _inside(box, inner):
                bad("containment", f"binary node {i}", f"the box stored for {what} {box.tolist()} does not contain {inner.tolist()}")
            ex.append(e)
            stored.append(box)
        u = _EMPTY.copy()
        for e in ex:
            u = _union(u, e)
        exact_bin[i] = u
        if strict:
            for (is_leaf, c, _), e, box in zip(kids[i], _fill_empty(ex), stored):
                if not _same(e, box):
                    bad("strict-box", f"binary node {i}", f"the box stored for {'records' if is_leaf else 'node'} {c} is {box.tolist()}, min / max of the vertices beneath is {e.tolist()}")

    # ---- 4-wide tree
    wseen = np.zeros(nw, bool)
    wseen[0] = True
    wleaves = {}
    wkids, worder = {}, []
    stack = [(0, 0, inf6)]
    depth_wide = 0
    while stack:
        w, d, path = stack.pop()
        worder.append(w)
        wkids[w] = []
        depth_wide = max(depth_wide, d + 1)
        links = [int(x) for x in Wi[w, 10:14]]
        n = 1
        while n < 4 and links[n] != links[0]:
            n += 1
        qlo = np.array([[(int(Wi[w, 4 + a]) >> (8 * k)) & 255 for a in range(3)] for k in range(4)])
        qhi = np.array([[(int(Wi[w, 7 + a]) >> (8 * k)) & 255 for a in range(3)] for k in range(4)])
        step, origin = np.array([W[w, 3], W[w, 14], W[w, 15]], np.float32), W[w, 0:3]
        if not (np.all(np.isfinite(step)) and np.all(step >= F32_MIN_NORMAL) and np.all(np.isfinite(origin))):
            bad("step", f"wide node {w}", f"grid steps {step.tolist()} at origin {origin.tolist()}: not normal numbers >= 2^-126")
            continue
        plo, phi = fma32_fast(qlo, step[None, :], origin[None, :]), fma32_fast(qhi, step[None, :], origin[None, :])
        for k in range(n, 4):
            if np.any(qlo[k] != 255) or np.any(qhi[k] != 0) or links[k] != links[0]:
                bad("unused-slot", f"wide node {w} slot {k}", f"lo bytes {qlo[k].tolist()}, hi bytes {qhi[k].tolist()}, link {links[k]}: not inverted with link 0 repeated")
        for k in range(n):
            item, link = f"wide node {w} slot {k}", links[k]
            box = np.concatenate([plo[k], phi[k]])
            # (a slot in use may hold an inverted box: the empty leaf of a caller's hierarchy, never entered; over anything that
            # has geometry such a box fails containment below)
            p = np.concatenate([np.maximum(path[:3], box[:3]), np.minimum(path[3:], box[3:])])
            if link >= 0:
                off = link - wide_base
                if off < 0 or off % 4 or off // 4 >= nw:
                    bad("shape", item, f"inner link {link} is out of range or not aligned")
                elif wseen[off // 4]:
                    bad("shape", item, f"wide node {off // 4} is reached twice")
                else:
                    wseen[off // 4] = True
                    wkids[w].append((False, off // 4, box, k))
                    stack.append((off // 4, d + 1, p))
            else:
                r = ~link
                j = leaf_of(r & ~3, item)
                if j is None:
                    continue
                if j in wleaves:
                    bad("partition", item, f"the leaf at record {j} is linked twice")
                    continue
                if (r & 3) != min(run_len[j], 4) - 1:
                    bad("hint", item, f"the link's low bits say {(r & 3) + 1} records, the leaf at record {j} holds {run_len[j]}")
                wleaves[j] = dict(path=p)
                wkids[w].append((True, j, box, k))
    if int(wseen.sum()) != nw:
        bad("shape", "wide nodes", f"{nw - int(wseen.sum())} wide nodes are not reachable")
    if depth_wide != wide_depth:
        bad("depth", "wide_depth", f"reported {wide_depth}, the walk finds {depth_wide}")
    if set(wleaves) != set(leaves):
        odd = sorted(set(wleaves) ^ set(leaves))
        bad("leaves-differ", f"record {odd[0]}", f"{len(odd)} leaves are in one tree only")

    exact_w, geo_w = {}, {}
    for w in reversed(worder):
        ex, ge = [], []
        for is_leaf, c, box, k in wkids[w]:
            if is_leaf:
                lf = leaves.get(c)
                g = lf["exact"] if lf and "exact" in lf else run_box(c)
                e = _EMPTY.copy() if lf is None or _empty(g) else lf["box"]   # the binary tree's leaf box (clipped for a split reference)
            else:
                e, g = exact_w[c], geo_w[c]
            if not _inside(box, e):
                bad("containment", f"wide node {w} slot {k}", f"the decoded box {box.tolist()} does not contain {e.tolist()}")
            ex.append(e)
            ge.append(g)
        u, ug = _EMPTY.copy(), _EMPTY.copy()
        for e, g in zip(ex, ge):
            u, ug = _union(u, e), _union(ug, g)
        exact_w[w], geo_w[w] = u, ug
        step, origin = np.array([W[w, 3], W[w, 14], W[w, 15]], np.float32), W[w, 0:3]
        if not _empty(u):
            top = fma32_fast(np.float32(255.0), step, origin)
            if np.any(top < u[3:]):
                bad("step", f"wide node {w}", f"plane 255 {top.tolist()} falls short of the node's upper bound {u[3:].tolist()}")
        links = [int(x) for x in Wi[w, 10:14]]
        n = 1
        while n < 4 and links[n] != links[0]:
            n += 1
        if strict and len(wkids[w]) == n:
            want = encode_wide_node(_fill_empty(ge), links)
            if not _same(want, W[w]):
                words = np.nonzero(_bits(want) != Wi[w])[0]
                bad("strict-wide", f"wide node {w}", f"words {words.tolist()} are {Wi[w, words].tolist()}, pt_encode_wide_node over the exact child boxes gives {_bits(want)[words].tolist()}")

    # ---- coverage: every test point of every triangle lies in a leaf that lists it and in every box on that leaf's path
    if coverage and not woop:
        by_id = {}
        for j, lf in leaves.items():
            if j not in wleaves:
                continue
            c = np.concatenate([np.maximum(lf["path"][:3], wleaves[j]["path"][:3]), np.minimum(lf["path"][3:], wleaves[j]["path"][3:])])
            for r in range(j, j + run_len[j]):
                if ids[r] >= 0:
                    by_id.setdefault(int(ids[r]), []).append(c)
        for t in range(len(soup)):
            if dropped[t] or t not in by_id:
                continue
            P = triangle_points(soup[t])
            C = np.array(by_id[t])
            ok = np.any(np.all((P[None, :, :] >= C[:, None, :3]) & (P[None, :, :] <= C[:, None, 3:]), axis=2), axis=0)
            if not np.all(ok):
                m = int(np.nonzero(~ok)[0][0])
                bad("coverage", f"triangle {t}", f"{int((~ok).sum())} of {len(P)} points are in no leaf path that lists it, first {P[m].tolist()}")
    return V
