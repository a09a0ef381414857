"""numpy restatement of PT_FLAG_MIS (include/ptmi.h "Multiple importance sampling"; csrc/pt_shade.h) in float64, for ONE diffuse
point on the ground quad of estimator_ref (P, normal UP, albedo RHO), depth 2, nothing in the way: per sample the uniform pick,
the draw on the light (sphere cone, uniform triangle point, env_light_ref.draw), w_l, the cosine-lobe bounce, what it lands on
(a sphere, a triangle, the map) and w_b — and from them the per-sample radiance of the three estimators: plain gathering,
exclusive next-event estimation and MIS.  Neither the oracle nor the kernels are consulted.  The scenes of the two cases MIS is
for (S-near, S-sun), S-sky and the case list of tests/test_gpu_mis.py live here too.  A plain module found through tests/ on
sys.path, like estimator_ref; no test in it, no GPU."""
import copy
import functools

import numpy as np

import gpu_pathtracer_amd as g
import env_light_ref
import estimator_ref as ref
from estimator_ref import P, RHO, UP, f32

MIS = ref.NEE | g.FLAG_MIS
# the shading point: path_shade_hit lifts a hit 0.001 along the normal before it tests eligibility, draws and bounces
X = P + 0.001 * UP


# ---------------------------------------------------------------------------------------------------- densities and weights
def pk_sphere(centre, radius, x=X):
    """per-steradian density of the cone draw towards a sphere seen from x: 1 / (2 pi (1 - cos_max))"""
    w = np.asarray(centre, np.float64) - x
    cos_max = np.sqrt(max(0.0, 1.0 - radius * radius / (w @ w)))
    return 1.0 / (2.0 * np.pi * (1.0 - cos_max))


def pk_triangle_from_light(verts, point, x=X):
    """... of a uniform point on a triangle, from the LIGHT's side: 2 d2 / proj with d2 = |point - x|^2, proj = |cross(e1, e2) . l|"""
    v0, v1, v2 = (np.asarray(v, np.float64) for v in verts)
    w = np.asarray(point, np.float64) - x
    d2 = np.einsum("...i,...i->...", w, w)
    l = w / np.sqrt(d2)[..., None]
    return 2.0 * d2 / np.abs(l @ np.cross(v1 - v0, v2 - v0))


def pk_triangle_from_hit(N, d, t):
    """... from the HIT's side: 2 t^2 / |N . d|, N the un-normalised normal (|N| = 2 area), t the distance along the unit d"""
    return 2.0 * t * t / np.abs(d @ np.asarray(N, np.float64))


def light_weight(pk, n_all, cosl):
    """w_l = q / (q + p_b), q = pk / n_all, p_b = cosl / pi"""
    q = pk / n_all
    return q / (q + cosl / np.pi)


def bounce_weight(pk, n_all, pb):
    """w_b = p_b' / (p_b' + q'), 1 where q' is not greater than 0"""
    q = np.asarray(pk, np.float64) / n_all
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(q > 0, pb / (pb + q), 1.0)


# ---------------------------------------------------------------------------------------------------- geometry
def frame(axis):
    """(t, b) as path_shade_hit builds them about a unit axis [.., 3]"""
    a = np.asarray(axis, np.float64)
    big_x = np.abs(a[..., 0]) > np.abs(a[..., 1])
    t = np.where(big_x[..., None], np.stack([a[..., 2], 0 * a[..., 0], -a[..., 0]], -1), np.stack([0 * a[..., 0], -a[..., 2], a[..., 1]], -1))
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    b = np.cross(a, t)
    return t, b / np.linalg.norm(b, axis=-1, keepdims=True)


def hit_sphere(o, d, centre, radius):
    """distance along unit d [n][3] from o to the sphere (the nearer root above 0.01, else the farther), inf where none"""
    w = np.asarray(centre, np.float64) - o
    b = d @ w
    disc = b * b - (w @ w - radius * radius)
    s = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(b - s > 0.01, b - s, b + s)
    return np.where((disc >= 0) & (t > 0.01), t, np.inf)


def hit_triangle(o, d, verts):
    """Moller-Trumbore, both faces: distance along d [n][3], inf where none"""
    v0, v1, v2 = (np.asarray(v, np.float64) for v in verts)
    e1, e2 = v1 - v0, v2 - v0
    pv = np.cross(d, e2)
    det = pv @ e1
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / det
        tv = o - v0
        u = (pv @ tv) * inv
        qv = np.cross(tv, e1)
        v = (d @ qv) * inv
        t = (qv @ e2) * inv
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return np.where(ok, t, np.inf)


# ---------------------------------------------------------------------------------------------------- the restatement
class Scene:
    """spheres: rows of estimator_ref.light (the first 8 that emit and that x is outside of are pickable); triangles: (three
    vertices, emission), every one a light, both faces; texels: a nearest-filtered map in the world frame that is a light, or None."""

    def __init__(self, spheres=(), triangles=(), texels=None, albedo=RHO):
        self.spheres = [(np.array(pr[:3], np.float64), float(pr[3]), np.array(emi, np.float64)) for pr, emi, _, _ in spheres]
        self.triangles = [([f32(v) for v in verts], np.array(emi, np.float64)) for verts, emi in triangles]
        self.texels = None if texels is None else np.asarray(texels, np.float32)
        self.tab = None if texels is None else env_light_ref.Tables(self.texels, False)
        self.albedo = np.asarray(albedo, np.float64)


def estimate(scene, log2_n=16, seed=1, x=X, n=UP):
    """{"plain", "nee", "mis"}: per-sample radiance [2^log2_n][3] of the three estimators at x, float64"""
    N = 1 << log2_n
    u = np.random.default_rng(seed).random((N, 5))
    rho = scene.albedo
    pick_sph = [i for i, (c, r, le) in enumerate(scene.spheres) if i < 8 and le.any() and (c - x) @ (c - x) > r * r * 1.001]
    n_tri = len(scene.triangles)
    n_all = len(pick_sph) + n_tri + (1 if scene.tab is not None else 0)

    # ---- the shadow ray: contribution and w_l
    con, wl = np.zeros((N, 3)), np.ones(N)
    if n_all > 0:
        pick = np.minimum((u[:, 0] * n_all).astype(np.int64), n_all - 1)
        for k, i in enumerate(pick_sph):
            sel = pick == k
            c, r, le = scene.spheres[i]
            w = c - x
            d2 = w @ w
            wn = w / np.sqrt(d2)
            cos_max = np.sqrt(max(0.0, 1.0 - r * r / d2))
            cos_t = 1.0 - u[sel, 1] * (1.0 - cos_max)
            sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
            t1, b1 = frame(wn)
            ph = 2.0 * np.pi * u[sel, 2]
            l = (np.sin(ph) * sin_t)[:, None] * t1 + cos_t[:, None] * wn + (np.cos(ph) * sin_t)[:, None] * b1
            cosl = l @ n
            ok = (cosl > 0) & np.isfinite(hit_sphere(x, l, c, r))
            con[sel] = np.where(ok[:, None], rho * le * (cosl * 2.0 * (1.0 - cos_max) * n_all)[:, None], 0.0)
            wl[sel] = light_weight(pk_sphere(c, r, x), n_all, np.maximum(cosl, 0.0))
        for k, (verts, le) in enumerate(scene.triangles):
            sel = pick == len(pick_sph) + k
            v0, v1, v2 = verts
            su = np.sqrt(u[sel, 1])
            pl = v0 + (1.0 - su)[:, None] * (v1 - v0) + (u[sel, 2] * su)[:, None] * (v2 - v0)
            w = pl - x
            d2 = np.einsum("ij,ij->i", w, w)
            l = w / np.sqrt(d2)[:, None]
            cosl = l @ n
            proj = np.abs(l @ np.cross(v1 - v0, v2 - v0))
            ok = (cosl > 0) & (proj > 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                con[sel] = np.where(ok[:, None], rho * le * (cosl * 0.5 * proj * n_all / (np.pi * d2))[:, None], 0.0)
                wl[sel] = np.where(ok, light_weight(pk_triangle_from_light(verts, pl, x), n_all, np.maximum(cosl, 0.0)), 1.0)
        if scene.tab is not None:
            sel = pick == n_all - 1
            s = env_light_ref.draw(scene.tab, u[sel, 1:3].astype(np.float32))
            l, pdf = s["d"], s["pdf"].astype(np.float64)
            cosl = l @ n
            ok = (cosl > 0) & (pdf > 0)
            L = scene.texels[s["y"], s["x"]].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                con[sel] = np.where(ok[:, None], rho * L * (cosl * n_all / (np.pi * pdf))[:, None], 0.0)
                wl[sel] = np.where(ok, light_weight(pdf, n_all, np.maximum(cosl, 0.0)), 1.0)

    # ---- the bounce ray: the cosine lobe about n, what it lands on, w_b
    nt, nb = frame(n)
    ph, r2s = 2.0 * np.pi * u[:, 3], np.sqrt(u[:, 4])
    d = (np.cos(ph) * r2s)[:, None] * nb + np.sqrt(1.0 - u[:, 4])[:, None] * n + (np.sin(ph) * r2s)[:, None] * nt
    pb = np.maximum(d @ n, 0.0) / np.pi
    best = np.full(N, np.inf)
    Le, pickable, pk = np.zeros((N, 3)), np.zeros(N, bool), np.zeros(N)
    for i, (c, r, le) in enumerate(scene.spheres):
        t = hit_sphere(x, d, c, r)
        win = t < best
        best = np.where(win, t, best)
        Le[win], pickable[win] = le, i in pick_sph
        pk[win] = pk_sphere(c, r, x) if i in pick_sph else 0.0
    for verts, le in scene.triangles:
        t = hit_triangle(x, d, verts)
        win = t < best
        best = np.where(win, t, best)
        Le[win], pickable[win] = le, True
        with np.errstate(invalid="ignore"):
            pk[win] = pk_triangle_from_hit(np.cross(verts[1] - verts[0], verts[2] - verts[0]), d[win], t[win])
    if scene.tab is not None:
        miss = ~np.isfinite(best)
        y, xx, valid = env_light_ref.texel_of(d[miss], scene.tab.W, scene.tab.H)
        Le[miss] = np.where(valid[:, None], scene.texels[y, xx].astype(np.float64), 0.0)
        pickable[miss] = True
        pk[miss] = env_light_ref.pdf_of(scene.tab, d[miss]).astype(np.float64)
    wb = np.where(pickable, bounce_weight(pk, max(n_all, 1), pb), 1.0)
    gathered = rho * Le
    return {"plain": gathered, "nee": con + gathered * (~pickable)[:, None], "mis": con * wl[:, None] + gathered * wb[:, None]}


@functools.lru_cache(maxsize=None)
def standard_error(name, log2_n):
    """per channel, the MIS restatement's standard error of the mean over 2^log2_n samples of a scene of SCENES"""
    return ref.mean_and_se(estimate(SCENES[name](), log2_n)["mis"])[1]


# ---------------------------------------------------------------------------------------------------- scenes
def _la():
    return ref.light(ref.A_C, ref.A_R, ref.A_LE)


def _ls():
    return ref.light(ref.S_C, ref.S_R, ref.S_LE)


# the scenes of estimator_ref whose GPU standard error is held against the restatement's
SCENES = {
    "A": lambda: Scene(spheres=[_la()]),
    "A2": lambda: Scene(spheres=[_la(), _ls()]),
    "B": lambda: Scene(triangles=[(ref.TRI, ref.TRI_LE)]),
    "BA": lambda: Scene(spheres=[_ls()], triangles=[(ref.TRI, ref.TRI_LE)]),
}

# S-near: where LIGHT sampling is poor.  An emissive triangle of side ~8 in the plane y = 0.25 above P, P below its interior and off
# its centroid: a uniform point on it has cos cos' / d^2 between ~(0.25 / 6)^2 / 36 and 1 / 0.0625, five orders of magnitude; the
# cosine lobe samples exactly the numerator that is left.  Its front faces down (cross(e1, e2) . UP < 0), as estimator_ref.TRI's.
NEAR_TRI = [P + (-3.0, 0.25, -2.5), P + (5.0, 0.25, -2.0), P + (0.5, 0.25, 5.0)]
NEAR_LE = np.array([0.9, 0.6, 0.3])
# the rays of the S scenes start here, straight down: below the triangle of S-near, above the ground
S_ORIGIN = P + (0.0, 0.125, 0.0)
# S-sun: where the BOUNCE is poor — test_a_small_sun_over_a_diffuse_plane's map: one texel of 1000 at latitude 40 degrees
SUN_MAP = (64, 32, 23, 10)


def near_scene():
    return Scene(triangles=[(NEAR_TRI, NEAR_LE)])


def near_E(x=X):
    return RHO * NEAR_LE * ref.polygon_form_factor([f32(v) for v in NEAR_TRI], p=x)


def near_mesh():
    """(mesh, material table, row per triangle): the ground and the emissive triangle, estimator_ref's table"""
    return ref.ground_with(NEAR_TRI), ref.TABLE, np.array([0, 0, 1], np.int32)


def sun_texels(sky=False):
    """S-sun's map, or S-sky's: the same sun in a sky of 0.5, where the bounce samples most of the light better"""
    return env_light_ref.hot_map(*SUN_MAP, value=1000.0, ambient=0.5) if sky else env_light_ref.hot_map(*SUN_MAP)


def sun_scene(sky=False):
    return Scene(texels=sun_texels(sky))


def sun_E(sky=False):
    tex = sun_texels(sky)
    return env_light_ref.plane_radiance(env_light_ref.Tables(tex, False), tex, RHO)


def s_rays(n):
    """n identical rays (o, 0, d, 0) from S_ORIGIN straight down"""
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = S_ORIGIN, (0.0, -1.0, 0.0)
    return rays


# ---------------------------------------------------------------------------------------------------- the GPU test's cases
def cases():
    """Every scene estimator_ref builds on two routes (its NEE route at depth 1), plus G and H, as a call with PT_FLAG_NEE |
    PT_FLAG_MIS at depth 2 and the expectation of its NEE route: every light has col 0 and the ground cannot see itself, so the
    second bounce adds nothing — except what it is for in G (the shell the point is inside of) and H (the sphere past the first 8),
    whose NEE routes at depth 2 already count it."""
    out = []
    for c in ref.cases():
        if not (c.name.endswith("-nee1") and c.name != "H-nee1") and c.name not in ("G-nee2", "H-nee2"):
            continue
        m = copy.copy(c)
        m.name, m.flags, m.depth, m.nee = c.name.rsplit("-", 1)[0] + "-mis2", MIS, 2, True
        out.append(m)
    return out
