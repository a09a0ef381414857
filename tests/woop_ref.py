"""woop_ref — the Woop triangle records (PT_OPT_TRI_TEST 1) ray by ray against exact geometry.  numpy only: no GPU, no library of
the project (the ray families at the end read meshes through gpu_pathtracer_amd's host side, as scene_matrix does).

    records(soup)                 the 16-float record of every triangle, as emit() (csrc/pt_scene_build.h) builds it
    intersect32(rec, o, d, cull)  pt_woop_intersect (csrc/pt_math.h) operation for operation in binary32
    exact(soup, o, d, cull)       t, u, v, det per (ray, triangle) in binary64, straight from the vertices
    margins(rec, o, d, soup)      how far intersect32's u, v, det, t may lie from exact's
    verdict(soup, rays, cull)     the set of acceptable answers per ray

u is the weight of v0 and v the weight of v1 (Woop's M has the columns v0 - v2, v1 - v2): exact() names them the same way, so its
u, v are Moller-Trumbore's (1 - u - v, u).  The accept region is the same triangle.

The margins (K is counted here, from the routine's rounding steps, and tuned on nothing: tests/test_woop.py checks that it holds)
---------------------------------------------------------------------------------------------------------------------------------
eps = 2^-24 is the unit roundoff of binary32, g(k) = k eps / (1 - k eps) the usual bound of k stacked roundings.
vdot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)) rounds three times: |vdot - a.b| <= g(3) sum |a_i b_i|.

  Dx = vdot(d, rx)                      3 roundings + 1, the record's own (each stored entry is a binary64 value rounded once to
                                        binary32)                                                   -> g(4) sum |d_i rx_i|
  Cx = rx.w + vdot(o, rx)               3 + 1 (the add) + 1 (the record)                            -> g(5) (|rx.w| + sum |o_i rx_i|)
  u  = fmaf(t, Dx, Cx)                  one more rounding on everything                             -> K = 6
       du = g(6) (|rx.w| + sum |o_i rx_i| + |t| sum |d_i rx_i|)  +  dt sum |d_i rx_i|
       where dt is t's own absolute error (t's relative error times |t|), which feeds the fma.  v alike with ry.
  u + v > 1                             one rounding of the sum                                     -> du + dv + g(1) (|u| + |v|)
  Oz = rz.w - vdot(o, rz)               3 + 1 + 1                                                   -> eO = g(5) (|rz.w| + sum |o_i rz_i|)
  Dz = vdot(d, rz)                      3 + 1                                                       -> eD = g(4) sum |d_i rz_i|
  t  = Oz * (1.0f / Dz)                 two roundings (the reciprocal is rounded before the multiply)
       dt = (eO + |t| eD) / (|Dz| - eD)  +  g(2) |t|         (infinite when eD >= |Dz|: the ray lies in the plane within rounding)
  det = -vdot(d, N)                     3 roundings over the stored N                               -> g(3) sum |d_i N_i|
       N = vcross(v0 - v1, v0 - v2) in binary32 is itself rounded (each difference once, the product once, the fma once: up to
       g(4) (|a_y b_z| + |a_z b_y|) per component).  The stored N and the vertices are both known, so dN_i is taken as the
       distance |N_i - exact N_i| itself, not as that bound, which on a large axis-aligned wall (whose N is exact) would exceed
       EPS and leave every ray in the wall's plane undecided; this part needs the vertices, hence `soup`.
       ddet = g(3) sum |d_i N_i| + sum |d_i| dN_i

The magnitudes are taken from the stored record in binary64; what that leaves out is of second order in eps and sits inside g(k)'s
denominators.  The binary64 steps of emit() and of exact() are taken as exact: their error is 2^-53 times the same sums of
magnitudes divided by the sine of the triangle's smallest angle (the cancellation in n = a x b), so below eps / 16 for aspect
ratios up to 2^25; the slivers of family e beyond that have dyadic vertices of few bits, whose n binary64 holds exactly.
Woop's known weakness shows in the first sum: far from the origin |rx.w| and |o_i rx_i| are ~ |v2| / edge length each and cancel
to a number in [0, 1], so du grows with |v2| / edge length (family f measures it).
"""
import functools
from collections import namedtuple

import numpy as np

import tree_audit as ta

F32_MAX = np.float32(3.402823466e+38)
EPS = float(np.float32(0.00001))      # the kernel's constant, a binary32 number
U = 2.0 ** -24
K_UV, K_C, K_D, K_T, K_DET = 6, 5, 4, 2, 3    # the counts derived in the module docstring
CHUNK_PAIRS = 1 << 20                 # (ray, triangle) pairs analysed at a time


def g_(k):
    return k * U / (1.0 - k * U)


def _clean(soup):
    s = np.array(soup, np.float32).reshape(-1, 9)
    s[:, 0] = np.where(s[:, 0] == 0, np.float32(0.0), s[:, 0])     # the host tree stores +0.0 for a v0.x of -0.0
    return s


# ---------------------------------------------------------------------------------------------------------------- records
def records(soup):
    """float32 [n][16]: triangle t's record with the word t << 1 | 1 (a leaf of its own).  tree_audit.encode_woop_records is the
    encoder; tree_audit.audit(woop=True) holds the device's records against the same function."""
    s = _clean(soup)
    return ta.encode_woop_records(s, np.arange(len(s)), np.ones(len(s), np.int64))


# ------------------------------------------------------------------------------------------------------------ intersect32
def _vdot32(ax, ay, az, bx, by, bz):
    return ta.fma32_fast(az, bz, ta.fma32_fast(ay, by, ax * bx))


Parts = namedtuple("Parts", "t u v det")


def intersect32_parts(rec, o, d):
    """pt_woop_intersect's numbers over every (ray, triangle) pair: o, d float32 [n][3], rec float32 [m][16] -> Parts of [n][m]
    arrays, all binary32 as the kernel holds them, before the accept rules (`hits`)."""
    rec = np.asarray(rec, np.float32).reshape(-1, 16)
    o, d = (np.asarray(x, np.float32).reshape(-1, 3) for x in (o, d))
    ox, oy, oz = (o[:, k, None] for k in range(3))
    dx, dy, dz = (d[:, k, None] for k in range(3))
    c = [rec[None, :, k] for k in range(16)]
    with np.errstate(all="ignore"):
        Oz = c[3] - _vdot32(ox, oy, oz, c[0], c[1], c[2])
        Dz = _vdot32(dx, dy, dz, c[0], c[1], c[2])
        t = (Oz * (np.float32(1.0) / Dz)).astype(np.float32)      # 1.0f / Dz is rounded to binary32 before the multiply
        u = ta.fma32_fast(t, _vdot32(dx, dy, dz, c[4], c[5], c[6]), c[7] + _vdot32(ox, oy, oz, c[4], c[5], c[6]))
        v = ta.fma32_fast(t, _vdot32(dx, dy, dz, c[8], c[9], c[10]), c[11] + _vdot32(ox, oy, oz, c[8], c[9], c[10]))
        det = -_vdot32(dx, dy, dz, c[12], c[13], c[14])
    return Parts(t, u, v, det)


def hits(p, cull, edge_ge=False):
    """The accept rules of pt_woop_intersect over its numbers: bool [n][m].  edge_ge: the sensitivity test's wrong edge rule,
    u + v >= 1 where the kernel has u + v > 1."""
    one, eps = np.float32(1.0), np.float32(0.00001)
    with np.errstate(all="ignore"):
        miss = np.where(p.det < -eps, bool(cull), p.det < eps)
        uv = p.u + p.v
        miss = miss | (p.u < 0) | (p.v < 0) | ((uv >= one) if edge_ge else (uv > one))
        miss = miss | ~((p.t > 0) & (p.t < F32_MAX))
    return ~miss


def intersect32(rec, o, d, cull, edge_ge=False):
    """t as pt_woop_intersect returns it, F32_MAX for a miss: float32 [n][m]."""
    p = intersect32_parts(rec, o, d)
    return np.where(hits(p, cull, edge_ge), p.t, F32_MAX).astype(np.float32)


def winner(t):
    """The brute-force closest hit of t [n][m] (column = id) under the walk's rule (pt_hit_update: nearer wins, an equal t goes to the
    smaller id): the id per ray, -1 for a miss."""
    j = np.argmin(t, axis=1)      # the first of equal minima = the smallest id
    return np.where(t[np.arange(len(t)), j] < F32_MAX, j, -1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ exact
Exact = namedtuple("Exact", "t u v det accept")


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def _accept_det(det, cull):
    return (det >= EPS) | ((det < -EPS) & (not cull))


def exact(soup, o, d, cull):
    """The ray / triangle test in binary64 straight from the vertices, [n][m] each: with a = v0 - v2, b = v1 - v2, n = a x b,
    det = -d . n (Moller-Trumbore's determinant), t = (v2 - o) . n / d . n, and with q = o + t d - v2 the barycentrics
    u = q . (b x n) / |n|^2 (weight of v0), v = q . (n x a) / |n|^2 (weight of v1).  This form loses nothing to cancellation that the
    triangle itself does not lose: its error is 2^-53 times the sums of magnitudes that margins() multiplies by 2^-24, once n is
    right, and n is exact for vertices of few bits (module docstring).  (Moller-Trumbore's own formulas in binary64 subtract
    products of the ray direction that cancel on a sliver, and were off by 6e-8 in u on the thinnest of family e.)
    accept: the rules of cudaUtils.h:151-166 as the kernel states them: det >= EPS, or det < -EPS without cull; u, v >= 0;
    u + v <= 1; 0 < t < F32_MAX.  EPS is the kernel's binary32 constant 0.00001f."""
    s = _clean(soup).astype(np.float64).reshape(-1, 3, 3)
    o, d = (np.asarray(x, np.float32).reshape(-1, 3).astype(np.float64) for x in (o, d))
    A, B, v2 = s[:, 0] - s[:, 2], s[:, 1] - s[:, 2], s[:, 2]
    n = _cross(A, B)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        dn = d @ n.T
        det = -dn
        t = ((v2 * n).sum(-1)[None, :] - o @ n.T) / dn
        bn, na = _cross(B, n), _cross(n, A)
        # q . r = (o - v2) . r + t (d . r)
        u = ((o @ bn.T - (v2 * bn).sum(-1)[None, :]) + t * (d @ bn.T)) / nn[None, :]
        v = ((o @ na.T - (v2 * na).sum(-1)[None, :]) + t * (d @ na.T)) / nn[None, :]
        acc = _accept_det(det, cull) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < float(F32_MAX))
    return Exact(t, u, v, det, acc)


# ---------------------------------------------------------------------------------------------------------------- margins
Margins = namedtuple("Margins", "u v uv det t t_rel t_lo")


def margins(rec, o, d, soup):
    """The bounds on |u32 - u|, |v32 - v|, |(u + v)32 - (u + v)|, |det32 - det|, |t32 - t| and t's relative one, [n][m] each, by the
    count of the module docstring (K = 6 for u and v), and t_lo <= |t32|.  Infinite where the ray lies in the triangle's plane
    within rounding."""
    rec = np.asarray(rec, np.float32).reshape(-1, 16).astype(np.float64)
    s = _clean(soup).astype(np.float64).reshape(-1, 3, 3)
    so, sd = (np.asarray(x, np.float32).reshape(-1, 3).astype(np.float64) for x in (o, d))
    o, d = np.abs(so), np.abs(sd)
    R = np.abs(rec)
    with np.errstate(all="ignore"):
        mag = lambda a, c: a @ R[:, c:c + 3].T                       # sum |a_i r_i|, [n][m]
        Oz = rec[None, :, 3] - so @ rec[:, 0:3].T
        sDz = sd @ rec[:, 0:3].T
        Dz = np.abs(sDz)
        eO = g_(K_C) * (R[None, :, 3] + mag(o, 0))
        eD = g_(K_D) * mag(d, 0)
        t = np.abs(Oz) / Dz
        dt = np.where(eD < Dz, (eO + t * eD) / (Dz - eD) + g_(K_T) * t, np.inf)
        dt = np.where(np.isnan(dt), np.inf, dt)
        tt = np.where(np.isfinite(t), t, np.inf)
        out, size = [], 0.0
        for c in (4, 8):
            m_d = mag(d, c)
            du = g_(K_UV) * (R[None, :, c + 3] + mag(o, c) + (tt + dt) * m_d) + dt * m_d
            out.append(np.where(np.isnan(du), np.inf, du))
            size = size + np.abs(rec[None, :, c + 3] + so @ rec[:, c:c + 3].T + (Oz / sDz) * (sd @ rec[:, c:c + 3].T))   # |u|, |v|
        du, dv = out
        duv = du + dv + g_(1) * (size + du + dv)           # the sum's own rounding
        duv = np.where(np.isnan(duv), np.inf, duv)
        # the stored N against the exact one: a number, not a bound (both are known); binary64's own cross product is right
        # within 2^-52 of the two products it subtracts
        a, b = s[:, 0] - s[:, 1], s[:, 0] - s[:, 2]
        a_, b_ = np.abs(a), np.abs(b)
        dN = np.abs(rec[:, 12:15] - _cross(a, b)) + 2.0 ** -52 * np.stack(
            [a_[:, 1] * b_[:, 2] + a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] + a_[:, 0] * b_[:, 2], a_[:, 0] * b_[:, 1] + a_[:, 1] * b_[:, 0]], 1)
        ddet = g_(K_DET) * (d @ R[:, 12:15].T) + d @ dN.T
        t_rel = dt / tt
        # the least |t| the kernel can hold, whatever the sign its Dz comes out with: where dt is infinite (a ray within rounding
        # of the triangle's plane) a t the kernel accepts still lies beyond this
        t_lo = np.maximum(np.abs(Oz) - eO, 0.0) / (Dz + eD) / (1.0 + g_(K_T))
        t_lo = np.where(np.isnan(t_lo), 0.0, t_lo)
    return Margins(du, dv, duv, ddet, dt, t_rel, t_lo)


# ---------------------------------------------------------------------------------------------------------------- verdict
class Verdict:
    """ok [n][m + 1] bool: the acceptable answers per ray (column m: a miss); decided [n]: exactly one; certain, maybe [n][m];
    T [n]: the exact t of the nearest certain triangle (inf: none) and `nearest` its id (-1); du_max: the largest finite du seen."""

    def __init__(self, n, m):
        self.ok = np.zeros((n, m + 1), bool)
        self.certain, self.maybe = np.zeros((n, m), bool), np.zeros((n, m), bool)
        self.T, self.nearest = np.full(n, np.inf), np.full(n, -1, np.int64)
        self.decided = np.zeros(n, bool)
        self.du_max = 0.0

    def accepts(self, ids):
        """per ray: is the answer `ids` (-1 = miss) acceptable"""
        ids = np.asarray(ids, np.int64)
        return self.ok[np.arange(len(ids)), np.where(ids < 0, self.ok.shape[1] - 1, ids)]


def classify(ex, mg, cull):
    """(certain, excluded) of every pair from exact's numbers and the margins: certain = the exact test accepts with every
    inequality clear of its margin, excluded = some inequality fails by more than its margin.  A comparison with a NaN is false on
    both sides, which leaves the pair `maybe`."""
    big = float(F32_MAX)
    with np.errstate(all="ignore"):
        det_c = (ex.det - mg.det >= EPS) | ((ex.det + mg.det < -EPS) & (not cull))
        det_x = (ex.det + mg.det < EPS) & ((ex.det - mg.det >= -EPS) | bool(cull))
        s = ex.u + ex.v
        certain = det_c & (ex.u - mg.u >= 0) & (ex.v - mg.v >= 0) & (s + mg.uv <= 1) & (ex.t - mg.t > 0) & (ex.t + mg.t < big)
        excluded = det_x | (ex.u + mg.u < 0) | (ex.v + mg.v < 0) | (s - mg.uv > 1) | (ex.t + mg.t <= 0) | (ex.t - mg.t >= big)
    return certain, excluded


def _chunks(n, m):
    step = max(1, CHUNK_PAIRS // max(m, 1))
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def verdicts(soup, rays, culls=(0, 1), rec=None):
    """verdict() under several cull settings from one pass over the pairs (the setting enters the det rule only): {cull: Verdict}."""
    s = _clean(soup)
    rec = records(s) if rec is None else rec
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    n, m = len(rays), len(s)
    out = {c: Verdict(n, m) for c in culls}
    for a, b in _chunks(n, m):
        o, d = rays[a:b, 0:3], rays[a:b, 4:7]
        ex, mg = exact(s, o, d, True), margins(rec, o, d, s)
        for cull, V in out.items():
            certain, excluded = classify(ex, mg, cull)
            maybe = ~certain & ~excluded
            with np.errstate(all="ignore"):
                tc = np.where(certain, ex.t, np.inf)
                near = np.argmin(tc, axis=1)
                rows = np.arange(b - a)
                T = tc[rows, near]
                has = np.isfinite(T)
                reach = T + np.where(has, mg.t[rows, near], 0.0)
                ok = (certain | maybe) & ~(mg.t_lo > reach[:, None])
            V.ok[a:b, :m], V.ok[a:b, m] = ok, ~has
            V.certain[a:b], V.maybe[a:b] = certain, maybe
            V.T[a:b], V.nearest[a:b] = T, np.where(has, near, -1)
            V.du_max = max(V.du_max, float(mg.u[np.isfinite(mg.u) & ~excluded].max(initial=0.0)))
    for V in out.values():
        V.decided = V.ok.sum(1) == 1
    return out


def verdict(soup, rays, cull, rec=None):
    """The acceptable answers per ray (rays float32 [n][8]: o, -, d, -).  A triangle is certain for a ray when the exact test accepts
    it with every inequality clear of its margin, excluded when some inequality fails by more than its margin, maybe otherwise.
    T = the exact t of the nearest certain triangle.  Acceptable are that triangle, any certain triangle whose t lies within the t
    margins of T, any maybe triangle with t <= T plus the margins (t taken at the least value the kernel can hold, Margins.t_lo);
    a miss only when no triangle is certain."""
    return verdicts(soup, rays, (cull,), rec)[cull]


# ------------------------------------------------------------------------------------------------------------ ray families
def mesh_soup(name):
    """(soup, mesh) of a named mesh: grid (family a), tilted_grid, bunny_low, cornell."""
    import gpu_pathtracer_amd as g
    import scene_matrix as sm
    mesh = sm.grid_mesh(8) if name == "grid" else sm.tilted_grid(8)[0] if name == "tilted_grid" else g.scene_mesh(name)
    return mesh.triangle_soup(), mesh


def reversed_winding(soup):
    """every second triangle's winding reversed (v1 and v2 exchanged)"""
    s = np.array(soup, np.float32).reshape(-1, 9)
    s[1::2] = s[1::2][:, [0, 1, 2, 6, 7, 8, 3, 4, 5]]
    return s


def _rays(o, d):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 4:7] = o, d
    return r


INCIDENCES = (0.0, 60.0, 85.0)                 # degrees from the normal
OFFSETS = (0, 1, -1, 4, -4, 64, -64)           # times the ray's own du
# offset: the multiple of du (None: the two fixed points); edge: the aimed edge's two vertex numbers (None: a vertex, or off the
# edge); du: of (ray, aimed triangle); dist: t at the target
Aimed = namedtuple("Aimed", "rays tri offset edge du dist")


def aimed_rays(soup, n_tris, seed):
    """Family b.  For a seeded sample of triangles: rays at the points with barycentrics (1/2, 1/2, 0) (the midpoint of the edge
    v0 v1) and (1, 0, 0) (the vertex v0), and at a point of the edge u = 0 (v1 v2), drawn 0.3 to 0.7 along it (the midpoints of a
    box's diagonals lie over one another), moved into the triangle (+) or out of it (-) by 0, 1, 4, 64 times du.  From both sides
    of the triangle, at 0, 60 and 85 degrees from its normal, tilted towards a direction in the triangle's plane drawn 20 to 70
    degrees off the edge (a ray tilted along the edge of an axis-aligned mesh lies in the planes of other walls within rounding,
    and each of those is one more acceptable answer), from a distance of half the triangle's shortest edge (near, so that little
    else lies on the way).  du is that ray's own: margins() of the ray with the same direction and origin offset aimed at the
    unmoved point of the edge, for the aimed triangle."""
    s = _clean(soup)
    rng = np.random.default_rng(seed)
    v = s.astype(np.float64).reshape(-1, 3, 3)
    area2 = np.linalg.norm(_cross(v[:, 0] - v[:, 1], v[:, 0] - v[:, 2]), axis=1)
    pick = rng.choice(np.nonzero(area2 > 0)[0], size=min(n_tris, int((area2 > 0).sum())), replace=False)
    rec = records(s)
    O, D, tri, off, edge, dus, dists = [], [], [], [], [], [], []
    for k in pick:
        v0, v1, v2 = v[k]
        A = v0 - v2
        nrm = _cross(v0 - v1, v0 - v2)
        nrm /= np.linalg.norm(nrm)
        tang = (v1 - v2) / np.linalg.norm(v1 - v2)
        turn = np.radians(rng.uniform(20.0, 70.0))
        tang = np.cos(turn) * tang + np.sin(turn) * _cross(nrm, tang)
        dist = 0.5 * min(np.linalg.norm(v0 - v1), np.linalg.norm(v1 - v2), np.linalg.norm(v2 - v0))
        for side in (1.0, -1.0):
            for inc in INCIDENCES:
                c, sn = np.cos(np.radians(inc)), np.sin(np.radians(inc))
                dirn = np.float32(-side * c * nrm + sn * tang).astype(np.float64)    # the direction the ray will carry
                back = dist * dirn
                mid = v2 + rng.uniform(0.3, 0.7) * (v1 - v2)
                du = float(margins(rec[k:k + 1], np.float32(mid - back)[None], np.float32(dirn)[None], s[k:k + 1]).u[0, 0])
                for p, f, e in [(0.5 * (v0 + v1), None, (0, 1)), (v0, None, None)] + [(mid + f * du * A, f, (1, 2) if f == 0 else None) for f in OFFSETS]:
                    O.append(p - back)
                    D.append(dirn)
                    tri.append(k)
                    off.append(f)
                    edge.append(e)
                    dus.append(du)
                    dists.append(dist)
    return Aimed(_rays(np.array(O), np.array(D)), np.array(tri), off, edge, np.array(dus), np.array(dists))


def sliver_soup():
    """Family e: (soup, rays, kinds).  Thin and small triangles in planes z = const in front of ordinary ones; kinds[t] is
    "ordinary", "thin" (|N| >= 1.5 EPS), "small" (|N| <= 0.77 EPS: never to be reported, never to hide anything) or "flat" (no area).
    Every thin or small triangle is v2 = (x, y, z), v0 = v2 + L e, v1 = v2 + w f with e, f orthogonal lattice directions and L, w powers
    of two, so its aspect ratio and |N| = L w |e| |f| are exact and binary64 makes its rows without error; the thinnest ones sit
    at x = y = 0, where a binary32 coordinate still holds w."""
    T, kinds = [], []

    def add(kind, v0, v1, v2):
        T.append([*v0, *v1, *v2])
        kinds.append(kind)

    # the ordinary triangles: a floor of two large ones at z = -9 under everything, wound to face +z
    add("ordinary", (-16, -16, -9), (272, -16, -9), (272, 272, -9))
    add("ordinary", (-16, -16, -9), (272, 272, -9), (-16, 272, -9))
    z = -3.0
    specs = []
    where = {0: (2.0, 2.0), 5: (4.0, 2.0), 10: (6.0, 2.0), 15: (2.0, 4.0), 20: (0.0, 0.0)}
    for a in (0, 5, 10, 15, 20):                       # aspect 2^a, L = 1: |N| = 2^-a ... thin down to 2^-15 (3e-5), small at 2^-20
        specs.append((1.0, 2.0 ** -a, where[a], (1, 0), (0, 1)))
    specs.append((1.0, 2.0 ** -16, (0.0, 0.0), (0, 1), (-1, 0)))        # |N| = 1.53e-5 > EPS
    specs.append((1.0, 2.0 ** -17, (0.0, 0.0), (0, 1), (-1, 0)))        # |N| = 7.6e-6 < EPS
    specs.append((128.0, 2.0 ** -22, (0.0, 0.0), (1, 0), (0, 1)))       # aspect 2^29, |N| = 3.05e-5
    specs.append((128.0, 2.0 ** -23, (0.0, 0.0), (1, 1), (-1, 1)))      # aspect 2^30, |N| = 2 * 1.53e-5
    specs.append((256.0, 2.0 ** -26, (0.0, 0.0), (1, 0), (0, 1)))       # aspect 2^34, |N| = 3.8e-6 < EPS
    specs.append((2.0 ** -8, 2.0 ** -7, (6.0, 6.0), (1, 0), (0, 1)))    # small and fat: |N| = 3.05e-5
    specs.append((2.0 ** -9, 2.0 ** -9, (6.0, 3.0), (1, 0), (0, 1)))    # small and fat: |N| = 3.8e-6 < EPS
    for L, w, (x, y), e, f in specs:
        v2 = (x, y, z)
        nn = L * w * abs(e[0] * f[1] - e[1] * f[0])
        add("thin" if nn > EPS else "small", (x + L * e[0], y + L * e[1], z), (x + w * f[0], y + w * f[1], z), v2)
        assert nn >= 1.5 * EPS or nn <= 0.77 * EPS
        z -= 0.25
    add("flat", (1, 1, z), (2, 2, z), (3, 3, z))               # exactly collinear
    add("flat", (5, 1, z - 0.25), (5, 1, z - 0.25), (6, 3, z - 0.25))   # two coincident vertices
    soup = np.array(T, np.float32)
    assert np.array_equal(soup.astype(np.float64), np.array(T, np.float64)), "a sliver's vertex is not a binary32 number"
    v = soup.astype(np.float64).reshape(-1, 3, 3)
    cen = v.mean(1)
    O, D = [], []
    for dirn in ((0.03, -0.02, -1.0), (-0.05, 0.04, 1.0), (0.6, 0.3, -1.0)):
        dn = np.array(dirn) / np.linalg.norm(dirn)
        for c in cen[2:]:
            O.append(c - 8.0 * dn)
            D.append(dn)
        for k in range(64):      # and at the floor behind them, on a lattice that passes under every sliver
            p = np.array([-2.0 + 1.25 * (k % 8), -2.0 + 1.25 * (k // 8), -9.0])
            O.append(p - 12.0 * dn)
            D.append(dn)
    return soup, _rays(np.array(O), np.array(D)), kinds


MOVES = {"moved": ((2.0 ** 10, -2.0 ** 12, 2.0 ** 8), 1.0), "small": ((0.0, 0.0, 0.0), 2.0 ** -6), "large": ((0.0, 0.0, 0.0), 2.0 ** 6)}


def moved_soup(soup, how):
    """Family f: the soup moved by (2^10, -2^12, 2^8) (every vertex rounded to binary32 where it lands), or scaled by 2^-6 or 2^6
    (exact).  The rays are family b's, aimed anew at the triangles where they now are."""
    shift, scale = MOVES[how]
    v = np.asarray(soup, np.float32).reshape(-1, 3).astype(np.float64) * scale + np.asarray(shift)
    return v.astype(np.float32).reshape(-1, 9)


N_AIMED = {"bunny_low": 10, "cornell": 16}
N_RANDOM = {"bunny_low": 2000, "cornell": 3000, "tilted_grid": 3000}


_aimed = {}


def aim(name):
    """the Aimed of a family of aimed rays (b, f)"""
    family(name)
    return _aimed[name]


@functools.lru_cache(maxsize=None)
def family(name):
    """(soup, rays) of a named family, built once: "a", "b-<mesh>", "c-<mesh>", "e", "f-<move>"; "d" is b and c with both cull
    settings, and with a "~" in front of the name the soup's every second winding reversed."""
    flip = name.startswith("~")
    key = name[1:] if flip else name
    if key == "a":
        import scene_matrix as sm
        soup, rays = mesh_soup("grid")[0], sm.grid_rays(8)
    elif key == "e":
        soup, rays, _ = sliver_soup()
    else:
        kind, what = key.split("-")
        if kind == "f":
            soup = moved_soup(mesh_soup("bunny_low")[0], what)
        else:
            soup = mesh_soup(what)[0]
        if flip:
            soup = reversed_winding(soup)
        if kind == "c":
            from gpu_support import rays_for
            rays = rays_for(soup, N_RANDOM[what], seed=20 + len(what))
        else:
            # tilted_grid's |n|^2 = 21/16 makes its rows inexact: it belongs here, under the margins, not in the exact class of a
            _aimed[name] = aimed_rays(soup, N_AIMED.get(what, 10) if kind == "b" else N_AIMED["bunny_low"], seed=7)
            rays = _aimed[name].rays
    if flip and key in ("a", "e"):
        soup = reversed_winding(soup)
    soup = np.ascontiguousarray(soup, np.float32)
    soup.setflags(write=False)
    rays = np.ascontiguousarray(rays, np.float32)
    rays.setflags(write=False)
    return soup, rays


FAMILIES = ("a", "b-bunny_low", "b-cornell", "b-tilted_grid", "c-bunny_low", "c-cornell", "c-tilted_grid", "e",
            "f-moved", "f-small", "f-large")
REVERSED = ("~b-bunny_low", "~b-cornell", "~b-tilted_grid", "~c-bunny_low", "~c-cornell", "~c-tilted_grid")       # family d's second half


@functools.lru_cache(maxsize=None)
def _family_verdicts(name):
    return verdicts(*family(name))


def family_verdict(name, cull):
    return _family_verdicts(name)[int(bool(cull))]


# ------------------------------------------------------------------------------------------- intersect32 over a whole family
MUTATIONS = ("rows", "sign", "edge", "cull", "N")


def mutate(rec, how):
    """The sensitivity test's wrong records: "rows" = the record's first two rows exchanged (the z row, which makes t, and the x
    row; exchanging the x and y rows would only rename u and v, whose rules are symmetric), "sign" = the x row's translation
    negated, "N" = the normal negated.  "edge" and "cull" change the rules, not the record."""
    r = np.array(rec, np.float32)
    if how == "rows":
        r[:, 0:8] = r[:, [4, 5, 6, 7, 0, 1, 2, 3]]
    elif how == "sign":
        r[:, 7] = -r[:, 7]
    elif how == "N":
        r[:, 12:15] = -r[:, 12:15]
    return r


Check = namedtuple("Check", "worst over winners")     # worst / over: key -> largest error / margin, pairs beyond the margin


def check_family(name, how=None):
    """intersect32 over records() for every (ray, triangle) pair of a family: the errors of u, v, det, t against exact() in units of
    margins(), and the brute-force winner per ray under both cull settings (winners[cull]).  how: one of MUTATIONS."""
    soup, rays = family(name)
    rec = mutate(records(soup), how) if how else records(soup)
    n, m = len(rays), len(soup)
    worst, over = dict(u=0.0, v=0.0, det=0.0, t=0.0), dict(u=0, v=0, det=0, t=0)
    win = {0: np.zeros(n, np.int64), 1: np.zeros(n, np.int64)}
    for a, b in _chunks(n, m):
        o, d = rays[a:b, 0:3], rays[a:b, 4:7]
        p = intersect32_parts(rec, o, d)
        for cull in (0, 1):
            h = hits(p, False if how == "cull" else cull, edge_ge=how == "edge")
            win[cull][a:b] = winner(np.where(h, p.t, F32_MAX))
        if how is None:
            ex, mg = exact(soup, o, d, True), margins(rec, o, d, soup)
            with np.errstate(all="ignore"):
                for key in worst:
                    got, want, bound = getattr(p, key).astype(np.float64), getattr(ex, key), getattr(mg, key)
                    judge = np.isfinite(bound) & np.isfinite(want)
                    err = np.abs(got - want)
                    bad = judge & ~(err <= bound)
                    over[key] += int(bad.sum())
                    ratio = err[judge & (bound > 0)] / bound[judge & (bound > 0)]
                    worst[key] = max(worst[key], float(ratio.max(initial=0.0)))
    return Check(worst, over, win)


@functools.lru_cache(maxsize=None)
def family_check(name):
    return check_family(name)
