"""Hand-built deep trees for the traversal stack (tests/test_deep_trees.py, tests/test_gpu_deep_stack.py): Compact arrays written
by hand, in the layout pt_upload_bvh parses (csrc/pt_scene_build.h, `parse`), with exactly the shape that fills a walk's stack, and
ray sets in which every stack entry decides some ray's answer.  Pure numpy; the upload keeps the caller's boxes as they are
(parse -> emit copies them), so the loose boxes below reach the walks unchanged and no second triangle per leaf is needed.

Geometry shared by every fixture: an 8 x 8 grid of unit cells, the FOOTPRINT [0, 8]^2; level k has its plane z = k / 8, deeper
levels HIGHER, that is nearer to rays that come from above along -z.  A target triangle covers one half of one cell, split along the
(i, j)-(i + 1, j + 1) diagonal: half A below the diagonal, half B above it.  Every coordinate is a small dyadic number, exact in
binary32.  Declared boxes span the footprint inflated by MARGIN in x and y, so a ray that stays above the footprint enters every
box, and the exact z range of their subtree, so the child that holds the deeper levels is always entered first.

comb(D)    a chain of D inner nodes, node k = {leaf k, node k + 1}, the last one two leaves; D + 1 leaves of one triangle each, leaf k
           on half A of cell k (k < 64) or half B of cell k - 64.  The binary walks push one entry per level, depth D; the 4-wide
           collapse packs three chain nodes into a wide node that pushes three entries: wide depth ceil(D / 3).
           mirror=True: the root becomes {a leaf of two triangles facing down high above the comb, the comb}: one level more.
stair(W)   a chain in which every wide level consumes ONE binary level: chain node k = {A_k, B = chain node k + 1}, A_k an inner node
           with two inner children of two leaves each.  A_k and A1_k are declared larger than B, so the collapse turns chain node k
           into {B, A2, A11, A12}: wide depth W with W - 1 chain nodes, and a wide walk that pushes three entries at every level.
           Three of A_k's four leaves hold a triangle outside the footprint; the fourth, A11, holds the target of cell k, so that
           every level of the stair, too, decides some ray's answer (A's boxes are declared, loosely, over both).
"""
import numpy as np

import gpu_pathtracer_amd as g

MARGIN = 0.5
DZ = 0.125
RAY_DIR = (1.0 / 64.0, -1.0 / 128.0, -1.0)


class Fixture:
    """.nodes, .tris, .index as g.Bvh has them; .mesh the matching g.Mesh (triangle ids = the order of the mesh); the tree as
    written (.inner: [(box0, child0, box1, child1)], child = int node number or a tuple of triangle ids), what it intends
    (.max_depth of pt_scene_info, .wide_depth of the 4-wide collapse) and the planes of its rays (.z_top, .targets: id -> (x, y, z))."""


def _box(x0, x1, y0, y1, z0, z1):
    return (np.array([x0, y0, z0], np.float64), np.array([x1, y1, z1], np.float64))


def _foot(z0, z1, x1=8.0):
    return _box(-MARGIN, x1 + MARGIN, -MARGIN, 8.0 + MARGIN, z0, z1)


def _half(cell, half, z):
    """the triangle on half A (0) or B (1) of `cell` in the plane z, counter-clockwise seen from +z"""
    i, j = float(cell % 8), float(cell // 8)
    if half == 0:
        return [(i, j, z), (i + 1, j, z), (i + 1, j + 1, z)]
    return [(i, j, z), (i + 1, j + 1, z), (i, j + 1, z)]


def _target(cell, half, z):
    i, j = cell % 8, cell // 8
    return (i + 0.75, j + 0.25, z) if half == 0 else (i + 0.25, j + 0.75, z)


def _area(b):
    d = b[1] - b[0]
    return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])


def _encode(inner, tri_verts):
    """Compact arrays (CudaBVH::createCompact's layout) of the tree `inner` (node 0 = root) over the triangles tri_verts[id]"""
    nodes = np.zeros((len(inner), 16), np.float32)
    tris, index, ends = [], [], []
    links = nodes.view(np.int32)
    for k, (b0, c0, b1, c1) in enumerate(inner):
        for i, (b, c) in enumerate(((b0, c0), (b1, c1))):
            nodes[k, 4 * i: 4 * i + 4] = (b[0][0], b[1][0], b[0][1], b[1][1])
            nodes[k, 8 + 2 * i: 10 + 2 * i] = (b[0][2], b[1][2])
            if isinstance(c, tuple):
                links[k, 12 + i] = ~len(tris)
                for tid in c:
                    for v in tri_verts[tid]:
                        tris.append((v[0], v[1], v[2], 0.0))
                        index.append(tid)
                ends.append(len(tris))          # the leaf's terminator
                tris.append((0.0, 0.0, 0.0, 0.0))
                index.append(0)
            else:
                links[k, 12 + i] = 64 * c
    tris = np.array(tris, np.float32)
    tris.view(np.uint32)[ends, 0] = 0x80000000
    return nodes.reshape(-1, 4), tris, np.array(index, np.int32)


def _finish(inner, tri_verts, targets, z_top):
    fx = Fixture()
    fx.inner, fx.targets, fx.z_top = inner, targets, z_top
    fx.nodes, fx.tris, fx.index = _encode(inner, tri_verts)
    v = np.array(tri_verts, np.float32).reshape(-1, 3)
    fx.mesh = g.Mesh.from_arrays(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3))
    fx.n_tris = len(tri_verts)
    fx.max_depth = tree_depth(fx)
    fx.wide_depth = collapse_depth(fx)
    return fx


def comb(D, mirror=False):
    assert 2 <= D <= 127
    tri_verts, targets, inner = [], {}, []
    for k in range(D + 1):
        z = k * DZ
        cell, half = (k, 0) if k < 64 else (k - 64, 1)
        tri_verts.append(_half(cell, half, z))
        targets[k] = _target(cell, half, z)
    z_top = D * DZ
    base = 1 if mirror else 0
    for k in range(D):
        leaf = (_foot(k * DZ, k * DZ), (k,))
        if k + 1 < D:
            chain = (_foot((k + 1) * DZ, z_top), base + k + 1)
        else:
            chain = (_foot(z_top, z_top), (D,))
        # the chain child alternates between the two slots, so both "nearer child" branches of the walks are taken
        inner.append(leaf + chain if k % 2 == 0 else chain + leaf)
    if mirror:
        zm = z_top + 33.0
        tri_verts += [[(-2.0, -2.0, zm), (-2.0, 10.0, zm), (10.0, 10.0, zm)], [(-2.0, -2.0, zm), (10.0, 10.0, zm), (10.0, -2.0, zm)]]
        inner.insert(0, (_box(-2.0, 10.0, -2.0, 10.0, zm, zm), (D + 1, D + 2), _foot(0.0, z_top), 1))
    fx = _finish(inner, tri_verts, targets, z_top)
    fx.D, fx.mirror_ids = D, (D + 1, D + 2) if mirror else ()
    return fx


def stair(W):
    n = W - 1                       # chain nodes
    assert 1 <= n <= 62
    tri_verts, targets, inner = [], {}, [None] * n
    z_top = n * DZ

    def outside(k, m):              # a triangle beside the footprint (x in 9..10), never met by a ray above the footprint
        y, z = float(3 * (k % 2) + m), k * DZ
        tri_verts.append([(9.0, y, z), (10.0, y, z), (10.0, y + 1.0, z)])
        return (len(tri_verts) - 1,)

    for k in range(n):
        z = k * DZ
        tri_verts.append(_half(k, 0, z))
        a11 = (len(tri_verts) - 1,)
        targets[a11[0]] = _target(k, 0, z)
        big, mid, flat = _foot(z - 4.0, z, 10.0), _foot(z - 3.0, z, 10.0), _foot(z, z, 10.0)
        a, a1, a2 = len(inner), len(inner) + 1, len(inner) + 2
        inner += [(big, a1, mid, a2), (flat, a11, flat, outside(k, 0)), (flat, outside(k, 1), flat, outside(k, 2))]
        if k + 1 < n:
            b = (_foot((k + 1) * DZ, z_top), k + 1)
        else:
            tri_verts.append(_half(n, 0, z_top))
            targets[len(tri_verts) - 1] = _target(n, 0, z_top)
            b = (_foot(z_top, z_top), (len(tri_verts) - 1,))
        inner[k] = (big, a) + b if k % 2 == 0 else b + (big, a)
        assert _area(big) > _area(b[0]) and _area(mid) > _area(b[0])
    fx = _finish(inner, tri_verts, targets, z_top)
    fx.W = W
    return fx


def cell_rays(fx, rise=1.0):
    """for every cell one ray through the interior of each half, (0.75, 0.25) and (0.25, 0.75) of the cell, aimed at the half's
    own target plane where it has one (else at plane 0); direction RAY_DIR, origin `rise` above the top plane.  Over the whole
    z range a ray drifts by less than 0.13 in x and 0.07 in y: it stays inside its half, so it meets at most that half's triangle."""
    plane = {(round(x * 4), round(y * 4)): z for (x, y, z) in fx.targets.values()}
    rays = []
    d = np.array(RAY_DIR)
    for cell in range(64):
        for half in (0, 1):
            x, y, _ = _target(cell, half, 0.0)
            z = plane.get((round(x * 4), round(y * 4)), 0.0)
            s = fx.z_top + rise - z
            o = np.array([x, y, z]) - s * d
            rays.append([*o, 0.0, *d, 0.0])
    return np.array(rays, np.float32)


def expected_ids(fx, rays):
    """the id every ray of cell_rays must report: its half's target triangle, or -1"""
    by_xy = {(round(x * 4), round(y * 4)): tid for tid, (x, y, z) in fx.targets.items()}
    out = []
    for r in np.asarray(rays, np.float64):
        s = (r[2] - 0.0) / -r[6]                       # down to plane 0, then back along the drift to the half's own interior point
        x, y = r[0] + s * r[4], r[1] + s * r[5]
        cx, cy = np.floor(x), np.floor(y)
        half = 0 if (y - cy) < (x - cx) else 1
        tx, ty, _ = _target(int(cx) + 8 * int(cy), half, 0.0)
        out.append(by_xy.get((round(tx * 4), round(ty * 4)), -1))
    return np.array(out, np.int32)


# ------------------------------------------------------------------------------------------------ models (evidence, not oracles)
def tree_depth(fx):
    """pt_scene_info's max_depth: the deepest leaf, the root's children at depth 1"""
    best, st = 0, [(0, 0)]
    while st:
        u, d = st.pop()
        for c in (fx.inner[u][1], fx.inner[u][3]):
            if isinstance(c, tuple):
                best = max(best, d + 1)
            else:
                st.append((c, d + 1))
    return best


def collapse_depth(fx):
    """depth of the 4-wide tree `emit` makes (csrc/pt_scene_build.h): a wide node starts as a binary node's two children and, while it
    has room, replaces its inner child of the largest area (the first one on a tie) by that child's two children"""
    def grow(u):
        kids = [(fx.inner[u][0], fx.inner[u][1]), (fx.inner[u][2], fx.inner[u][3])]
        while len(kids) < 4:
            best, ba = -1, -1.0
            for i, (b, c) in enumerate(kids):
                if not isinstance(c, tuple) and np.float32(_area(b)) > ba:
                    best, ba = i, np.float32(_area(b))
            if best < 0:
                break
            v = kids[best][1]
            kids[best] = kids[-1]
            kids.pop()
            kids += [(fx.inner[v][0], fx.inner[v][1]), (fx.inner[v][2], fx.inner[v][3])]
        return [c for _, c in kids]

    depth, level = 0, [0]
    while level:
        depth += 1
        level = [c for u in level for c in grow(u) if not isinstance(c, tuple)]
    return depth


def binary_stack_depth(fx, rays):
    """The binary walk's order restated (trav_run / the oracle's bvh_intersect): slab test of both children, the nearer one first,
    the farther one pushed, the first leaf met postponed.  Returns the largest stack index written per ray (entry 0 is the
    bottom marker).  Boxes only, no triangle is tested: every fixture's rays meet their one triangle after the deepest push."""
    out = []
    for r in np.asarray(rays, np.float64):
        o, inv = r[0:3], 1.0 / r[4:7]

        def slab(b):
            t0, t1 = (b[0] - o) * inv, (b[1] - o) * inv
            lo, hi = max(np.minimum(t0, t1).max(), 0.0), np.maximum(t0, t1).min()
            return lo <= hi, lo

        sp = deepest = 0
        stack = {0: None}
        node, leaf = 0, None
        while node is not None:
            while node is not None and not isinstance(node, tuple):
                b0, c0, b1, c1 = fx.inner[node]
                (h0, d0), (h1, d1) = slab(b0), slab(b1)
                if not h0 and not h1:
                    node, sp = stack[sp], sp - 1
                else:
                    node = c0 if h0 else c1
                    if h0 and h1:
                        far = c1
                        if d1 < d0:
                            node, far = c1, c0
                        sp += 1
                        stack[sp] = far
                        deepest = max(deepest, sp)
                if isinstance(node, tuple) and leaf is None:
                    leaf = node
                    node, sp = stack[sp], sp - 1
                if leaf is not None:
                    break
            while leaf is not None:
                leaf = node if isinstance(node, tuple) else None
                if isinstance(node, tuple):
                    node, sp = stack[sp], sp - 1
        out.append(deepest)
    return np.array(out, np.int32)


ORACLE_LAST_ENTRY = 63          # the oracle's walk keeps ORC_STACK_SIZE = 64 entries (oracle/pt_oracle.h): index 63 is its last


def oracle_may_walk(fx, rays=None):
    """whether the oracle's own walk may be run over the fixture: its stack must hold the modelled depth"""
    return int(binary_stack_depth(fx, cell_rays(fx) if rays is None else rays).max()) <= ORACLE_LAST_ENTRY


# ------------------------------------------------------------------------------------------------ a mesh whose Morton keys chain
CHAIN_SCALE = 1024.0
AXIS_BITS, SIZE_BITS = 18, 9     # csrc/pt_build.h, k_morton: 18 bits per axis of the box centre + 9 bits of the box diagonal = 63


def _about(p, h):
    """a triangle whose box is p +- h in every axis (so its centre is p, exactly)"""
    p = np.asarray(p, np.float64)
    return [p + (-h, -h, -h), p + (h, h, h), p + (h, -h, h)]


def morton_chain_mesh(n_equal=8):
    """Triangles at geometrically shrinking positions and of geometrically shrinking sizes, so that the device builders' sort keys
    have their leading one at 63 different bit positions: the linear BVH (Karras) then peels one key range off per level, a chain
    of 63 inner nodes (depths 0 .. 62), and the n_equal identical keys at its end hang log2(n_equal) inner levels below it.  The box centres span [0, 1]^3:
      - 3 x 18 tiny triangles at 1.5 * 2^-j on one axis each (j = 1 .. 18): coordinate bit 18 - j of that axis leads the key;
      - 9 triangles about the origin with a box diagonal of 0.75 * 2^-i of the scene's (i = 0 .. 8): size bit 8 - i leads;
      - 3 tiny triangles at 1 on each axis (they give the centres their extent), n_equal tiny ones about the origin (key 0).
    1.5 and 0.75 keep every quantised value half a step away from the next power of two, whatever the last bit of the division
    or the square root.  The whole is scaled by CHAIN_SCALE, a power of two (the keys are relative): the tiny triangles, 2^-15 of the
    scene, then stand clear of Moller-Trumbore's determinant threshold.  Returns the g.Mesh."""
    tiny = 2.0 ** -16
    tris = []
    for a in range(3):
        for j in range(1, AXIS_BITS + 1):
            p = [0.0, 0.0, 0.0]
            p[a] = 1.5 * 2.0 ** -j
            tris.append(_about(p, tiny))
    for i in range(SIZE_BITS):
        tris.append(_about((0.0, 0.0, 0.0), 0.375 * 2.0 ** -i))
    for a in range(3):
        p = [0.0, 0.0, 0.0]
        p[a] = 1.0
        tris.append(_about(p, tiny))
    for _ in range(n_equal):
        tris.append(_about((0.0, 0.0, 0.0), tiny))
    tris = CHAIN_SCALE * np.array(tris).reshape(-1, 3)
    v = tris.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), tris)          # every coordinate is exact in binary32
    return g.Mesh.from_arrays(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3))


def morton_keys(mesh):
    """k_morton restated in binary32: the 63-bit extended Morton key of every triangle (most significant first x y z x y z s ...)"""
    f = np.float32
    v = np.asarray(mesh.verts, f)[np.asarray(mesh.tris)]
    lo, hi = v.min(axis=1), v.max(axis=1)
    c = f(0.5) * lo + f(0.5) * hi
    clo, chi = c.min(axis=0), c.max(axis=0)
    ext = chi - clo
    keys = []
    for k in range(len(v)):
        u = [min(max((c[k, a] - clo[a]) / ext[a], f(0)), f(1)) if ext[a] > 0 else f(0) for a in range(3)]
        q = [min(int(f(u[a]) * f(1 << AXIS_BITS)), (1 << AXIS_BITS) - 1) for a in range(3)]
        diag2 = f(0)
        sdiag2 = f(0)
        for a in range(3):
            diag2 = f(diag2 + (hi[k, a] - lo[k, a]) * (hi[k, a] - lo[k, a]))
            sdiag2 = f(sdiag2 + ext[a] * ext[a])
        rel = np.sqrt(f(diag2 / sdiag2)) if sdiag2 > 0 else f(0)
        qs = min(int(min(rel, f(1)) * f(1 << SIZE_BITS)), (1 << SIZE_BITS) - 1)
        key, bx, bs, phase, ax = 0, AXIS_BITS - 1, SIZE_BITS - 1, 0, 0
        for _ in range(3 * AXIS_BITS + SIZE_BITS):
            if phase == 6 and bs >= 0:
                bit = (qs >> bs) & 1
                bs -= 1
                phase = 0
            else:
                bit = (q[ax] >> bx) & 1
                ax += 1
                if ax == 3:
                    ax, bx = 0, bx - 1
                phase += 1
                if bx < 0:
                    phase = 6
            key = (key << 1) | bit
        keys.append(key)
    return keys


def lbvh_depth(keys):
    """depth (edges to the root) of the deepest INNER node of the Karras hierarchy over the sorted keys, equal keys told apart by
    their position (ptb_delta): what pt_build_bvh compares with 64 before it fits a box"""
    keys = sorted(keys)

    def delta(i, j):
        x = keys[i] ^ keys[j]
        return 64 - x.bit_length() if x else 64 + (32 - (i ^ j).bit_length())

    deepest, st = 0, [(0, len(keys) - 1, 0)]
    while st:
        lo, hi, d = st.pop()
        deepest = max(deepest, d)
        dn = delta(lo, hi)
        split = max(s for s in range(lo, hi) if s == lo or delta(lo, s) > dn)
        for a, b in ((lo, split), (split + 1, hi)):
            if a < b:
                st.append((a, b, d + 1))
    return deepest
