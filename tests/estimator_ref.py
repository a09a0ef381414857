"""Closed-form radiance for every estimator of the path loop, in float64, and the tiny scenes that isolate each of them: the
inputs of tests/test_estimators.py (the oracle, CPU) and tests/test_gpu_estimators.py (every kernel).  Neither the oracle nor
pt_shade.h is consulted here: every expectation is geometry and the rendering equation.

All scenes share the ground quad (two triangles in y = 0, facing up), the point P = (7, 0, -3) on it, albedo RHO, a black
background and a camera that looks at P from 1.5 units away through a field of view of 1e-5: every pixel and every jitter is
the same path start up to 1e-5 relative, so a frame is as many samples of ONE path integral as it has pixels x samples.  Every
light has col = 0 (a path ends on it) and every emission is chosen so that no single sample colour reaches 1: the fold's clamp
never acts.

The closed forms are computed on the binary32 values the renderers get (sphere rows, vertices and directions are rounded first).
"""
import numpy as np

import gpu_pathtracer_amd as g

RHO = np.array([0.5, 0.6, 0.7])
P = np.array([7.0, 0.0, -3.0])
UP = np.array([0.0, 1.0, 0.0])
BLACK = (0.0, 0.0, 0.0)
BASE = g.FLAG_FACE_FORWARD | g.FLAG_COSINE_DIFF | g.FLAG_MISS_KEEPS_PATH
NEE = BASE | g.FLAG_NEE
FRAME = 77


def f32(x):
    """the binary32 value a renderer reads, as float64"""
    return np.asarray(x, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- closed forms
def sphere_form_factor(centre, radius, p=P, n=UP):
    """Irradiance fraction of a uniform sphere wholly above the horizon of (p, n): F = (r / d)^2 cos(theta)."""
    w = np.asarray(centre, np.float64) - p
    d = np.linalg.norm(w)
    assert (w @ n) >= radius, "the sphere must lie wholly above the horizon"
    return (radius / d) ** 2 * (w @ n) / d


def polygon_form_factor(verts, p=P, n=UP):
    """Lambert's formula for a polygon wholly above the horizon: F = |sum_i gamma_i (n . Gamma_i)| / (2 pi), gamma_i the angle the
    edge i subtends at p and Gamma_i the unit normal of the plane through p and that edge."""
    v = [np.asarray(x, np.float64) - p for x in verts]
    assert all(x @ n > 0 for x in v)
    v = [x / np.linalg.norm(x) for x in v]
    total = 0.0
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        gamma = np.cross(a, b)
        total += np.arccos(np.clip(a @ b, -1.0, 1.0)) * (n @ (gamma / np.linalg.norm(gamma)))
    return abs(total) / (2.0 * np.pi)


def basis(axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 0.0, 1.0])
    t /= np.linalg.norm(t)
    return a, t, np.cross(a, t)


def cone_integral(density, axis, half_angle, N=400):
    """Integral of density(w [.., 3]) over the cone of `half_angle` about `axis`: midpoint rule on an N x N grid in (cos, phi)."""
    a, b1, b2 = basis(axis)
    k = (np.arange(N) + 0.5) / N
    ct, ph = np.meshgrid(1.0 - k * (1.0 - np.cos(half_angle)), 2.0 * np.pi * k, indexing="ij")
    st = np.sqrt(1.0 - ct * ct)
    w = ct[..., None] * a + (st * np.cos(ph))[..., None] * b1 + (st * np.sin(ph))[..., None] * b2
    return float(density(w).mean() * 2.0 * np.pi * (1.0 - np.cos(half_angle)))


def sphere_cone(centre, radius, p=P):
    """(axis, half angle) of the cone a sphere fills as seen from p"""
    w = np.asarray(centre, np.float64) - p
    return w, float(np.arcsin(radius / np.linalg.norm(w)))


def lambert_density(n=UP):
    """cos / pi: what a DIFF surface of albedo 1 turns radiance into"""
    return lambda w: np.clip(w @ n, 0.0, None) / np.pi


def phong_density(expo, mirror):
    """(n + 1) / (2 pi) cos^n about the mirror direction: the METAL lobe's draw, weight 1"""
    m = np.asarray(mirror, np.float64)
    return lambda w: (expo + 1.0) / (2.0 * np.pi) * np.clip(w @ m, 0.0, None) ** expo


def default_lobe_density(n=UP):
    """The DIFF lobe without PT_FLAG_COSINE_DIFF: rv = (c f2, sqrt(1 - f2^2), s f2) draws sin(theta) = f2 uniformly, so
    p(w) = p(sin) |d sin / d theta| / (2 pi sin) = cos / (2 pi sin) per steradian; the weight is 1."""
    def p(w):
        c = np.clip(w @ n, 0.0, 1.0)
        return c / (2.0 * np.pi * np.sqrt(1.0 - c * c))
    return p


def uniform_density():
    """1 / (2 pi): what "uniform hemisphere" would mean; case F tells it from default_lobe_density"""
    return lambda w: np.full(w.shape[:-1], 1.0 / (2.0 * np.pi))


def triangle_area_form_factor(verts, p=P, n=UP, N=600):
    """The form factor of a triangle by quadrature over its AREA, cos cos' / (pi d^2): midpoint rule over N^2 sub-triangles
    (independent of Lambert's contour formula)."""
    a, b, c = (np.asarray(x, np.float64) for x in verts)
    nl = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(nl)
    nl /= np.linalg.norm(nl)
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    total = 0.0
    for off, keep in ((1.0 / 3.0, i + j < N), (2.0 / 3.0, i + j < N - 1)):   # upright and inverted cells, by centroid
        u, v = (i[keep] + off) / N, (j[keep] + off) / N
        w = a + u[:, None] * (b - a) + v[:, None] * (c - a) - p
        d2 = np.einsum("ij,ij->i", w, w)
        total += np.sum((w @ n) * np.abs(w @ nl) / (np.pi * d2 * d2))
    return float(total * area / (N * N))


def schlick(c, nc=1.0, nt=1.5):
    """R0 = ((nt - nc) / (nt + nc))^2, Re = R0 + (1 - R0) (1 - c)^5, c the cosine on the air side"""
    r0 = ((nt - nc) / (nt + nc)) ** 2
    return r0 + (1.0 - r0) * (1.0 - c) ** 5


# ---------------------------------------------------------------------------------------------------- scenes
GROUND_V = [[-50.0, 0.0, -50.0], [50.0, 0.0, -50.0], [50.0, 0.0, 50.0], [-50.0, 0.0, 50.0]]
GROUND_T = [[0, 2, 1], [0, 3, 2]]


def ground_with(*triangles):
    """The ground quad (ids 0, 1) and the given triangles (3 vertices each; ids 2, 3, ..)"""
    v, t = list(GROUND_V), list(GROUND_T)
    for tri in triangles:
        k = len(v)
        v += [list(map(float, x)) for x in tri]
        t.append([k, k + 1, k + 2])
    return g.Mesh.from_arrays(np.array(v, np.float32), np.array(t, np.int32))


def row(col, emi=BLACK, mat=g.MAT_DIFF, phong=0.0):
    m = g.Material()
    m.col[:], m.emi[:], m.mat, m.phong_expo = [float(x) for x in col], [float(x) for x in emi], mat, phong
    return m


def light(centre, radius, emi, col=BLACK):
    """a sphere row: (centre, radius) rounded to binary32, emission, colour, DIFF"""
    return (tuple(f32(centre)) + (float(f32(radius)),), tuple(emi), tuple(col), g.MAT_DIFF)


def sphere_array(rows):
    arr = (g.Sphere * len(rows))()
    for s, (pr, emi, col, mat) in zip(arr, rows):
        s.pos_rad[:], s.emi[:], s.col[:], s.mat = pr, emi, col, mat
    return arr


class Case:
    """One path integral with its answer.  kind: "mc" (the mean is E within 5 standard errors), "fixed" (zero variance: every sample
    is E within 1e-5 E) or "zero" (every sample is exactly 0).  nee: the call has PT_FLAG_NEE (the tighter standard-error bound,
    the smaller frame on the GPU).  alt: an expectation the estimate must REJECT (case F)."""

    def __init__(self, name, E, kind="mc", flags=BASE, depth=2, mesh=None, spheres=(), toward=(0.0, -1.0, 0.0), target=P, cull=0,
                 tri_mat=g.MAT_DIFF, col=RHO, phong=30.0, materials=None, tri_material=None, log2_n=16, alt=None):
        self.name, self.E, self.kind, self.flags, self.depth = name, np.asarray(E, np.float64) * np.ones(3), kind, flags, depth
        self.mesh = mesh if mesh is not None else ground_with()
        self.rows, self.cull, self.tri_mat, self.col, self.phong = list(spheres), cull, tri_mat, tuple(col), phong
        self.materials, self.tri_material = materials, None if tri_material is None else np.asarray(tri_material, np.int32)
        self.toward, self.target = view_direction(toward), np.asarray(target, np.float64)
        self.log2_n, self.alt = log2_n, alt
        self.nee = bool(flags & g.FLAG_NEE)

    def __repr__(self):
        return self.name

    def spheres(self):
        return sphere_array(self.rows) if self.rows else None

    def camera(self, W, H):
        d = self.toward
        a = np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
        r = np.cross(d, a)
        r /= np.linalg.norm(r)
        cam = g.default_camera(W, H)
        cam.pos[:], cam.front[:], cam.right[:], cam.up[:] = tuple(self.target - 1.5 * d), tuple(d), tuple(r), tuple(np.cross(r, d))
        cam.dist, cam.aspect, cam.fov = 1.0, 1.0, 1e-5
        return cam

    def ray(self):
        """the camera's central ray (o, 0, d, 0): it starts on the image plane, one `dist` in front of the camera"""
        cam = self.camera(4, 4)
        o = np.array(cam.pos[:], np.float32) + np.array(cam.front[:], np.float32) * np.float32(cam.dist)
        return np.array([*o, 0.0, *cam.front[:], 0.0], np.float32)

    def params(self, W, H):
        p = g.default_params(W, H, depth=self.depth, tri_mat=self.tri_mat)
        p.tri_col[:], p.tri_emi[:], p.bk_color[:] = self.col, BLACK, BLACK
        p.flags, p.frame, p.sample_index, p.cull_backfaces = self.flags, FRAME, 1, self.cull
        p.phong_expo, p.air_ior, p.glass_ior = self.phong, 1.0, 1.5
        return p


def view_direction(toward):
    """a unit direction as the camera stores it: normalised in float64, rounded to binary32"""
    d = np.asarray(toward, np.float64)
    return f32(d / np.linalg.norm(d))


# the lights
A_C, A_R, A_LE = P + (3.0, 4.0, 1.0), 1.0, np.array([1.6, 1.2, 0.8])
S_C, S_R, S_LE = P + (-2.0, 3.0, -2.0), 0.5, np.array([1.0, 1.5, 1.2])          # the "small light" of A2, BA, G
TRI = [P + (1.0, 3.0, -1.0), P + (4.0, 3.5, 0.5), P + (2.0, 2.5, 3.0)]         # its front (cross(e1, e2) points down) faces P
TRI_LE = np.array([0.9, 0.6, 0.3])
TABLE = [row(RHO), row(BLACK, emi=TRI_LE), row(BLACK)]                       # ground, the emissive triangle, a black occluder


def E_sphere(c, r, le):
    return RHO * le * sphere_form_factor(f32(c), float(f32(r)))


def occluder(dy):
    """a large black triangle in the plane y = 2.75 + dy: from P it covers the whole light triangle (dy < 0) or lies behind it"""
    y = 2.75 + dy
    return [P + (-6.0, y, -6.0), P + (14.0, y, -6.0), P + (2.0, y, 14.0)]


def both(name, E, nee_depth=1, kind="mc", **kw):
    """a scene on its two routes of equal expectation: NEE at depth d and plain gathering at depth d + 1 (the first hit is the
    only DIFF surface: every light has col 0)"""
    return [Case(f"{name}-nee{nee_depth}", E, kind, flags=NEE, depth=nee_depth, **kw),
            Case(f"{name}-plain{nee_depth + 1}", E, kind, flags=BASE, depth=nee_depth + 1, **kw)]


def cases():
    out = []
    E_A, E_S = E_sphere(A_C, A_R, A_LE), E_sphere(S_C, S_R, S_LE)
    E_B = RHO * TRI_LE * polygon_form_factor([f32(v) for v in TRI])
    la, ls = light(A_C, A_R, A_LE), light(S_C, S_R, S_LE)
    tri = dict(mesh=ground_with(TRI), materials=TABLE, tri_material=[0, 0, 1])

    # A, A2: sphere lights — the cone draw, its 2 (1 - cos_max) * n_all weight, the uniform pick
    out += both("A", E_A, spheres=[la]) + [Case("A-nee2", E_A, flags=NEE, depth=2, spheres=[la])]
    out += both("A2", E_A + E_S, spheres=[la, ls])
    # B, BA: a triangle light from a material table — cosl * area * cos_light / (pi d^2); the mixed pick
    out += both("B", E_B, **tri)
    out += both("BA", E_B + E_S, spheres=[ls], **tri)
    # G: inside a black emitting shell — the shell is not eligible and is gathered by the bounce, the small light is not counted twice
    lb = np.array([0.1, 0.2, 0.3])
    shell = light((0.0, 0.0, 0.0), 1000.0, lb)
    F_S = sphere_form_factor(f32(S_C), S_R)
    E_G = RHO * (lb * (1.0 - F_S) + S_LE * F_S)
    out += [Case("G-nee2", E_G, flags=NEE, depth=2, spheres=[shell, ls]), Case("G-plain2", E_G, spheres=[shell, ls])]
    # H: ten spheres, lights at index 2 and index 9 — the sphere past the first 8 is never a pick and never masked: NEE at depth 2
    # gathers it by the bounce, NEE at depth 1 does not see it.  It is large (F = 0.17) and dim, so that the bounce's Bernoulli
    # noise, sqrt((1 - F) / (F n)) E9 / E, stays below half the standard-error bound of the NEE routes at 2^18 samples.
    h_c, h_r, h_le = P + (3.0, 3.0, 2.0), 2.4, np.array([0.1, 0.1, 0.1])
    rows = [light((100.0 + 5.0 * i, 50.0, 100.0), 0.5, BLACK) for i in range(10)]
    rows[2], rows[9] = ls, light(h_c, h_r, h_le)
    out += [Case("H-nee2", E_S + E_sphere(h_c, h_r, h_le), flags=NEE, depth=2, spheres=rows),
            Case("H-nee1", E_S, flags=NEE, depth=1, spheres=rows)]
    # I: the triangle light's winding and cull_backfaces — only the front of a culled triangle emits (B is "as given, cull 0")
    flipped = dict(tri, mesh=ground_with([TRI[0], TRI[2], TRI[1]]))
    out += both("I-given-cull1", E_B, cull=1, **tri) + both("I-flipped-cull0", E_B, **flipped)
    out += both("I-flipped-cull1", 0.0, kind="zero", cull=1, **flipped)
    # J: a black triangle below the light (hides all of it) and above it (hides nothing) — the shadow ray and its t_max
    for name, dy, E, kind in (("J-below", -0.8, 0.0, "zero"), ("J-above", 0.8, E_B, "mc")):
        out += both(name, E, kind=kind, mesh=ground_with(TRI, occluder(dy)), materials=TABLE, tri_material=[0, 0, 1, 2])
    # J2: a black sphere between P and the sphere light, and behind it
    to_a = A_C - P
    out += both("J2-between", 0.0, kind="zero", spheres=[la, light(P + 0.5 * to_a, 0.8, BLACK)])
    out += both("J2-behind", E_A, spheres=[la, light(P + 1.6 * to_a, 0.8, BLACK)])
    # C: the Phong lobe (METAL, through pt_pow01) into a probe sphere at angle alpha from the mirror direction (= the normal)
    col_m, le_m = np.array([0.9, 0.7, 0.5]), np.array([1.0, 0.8, 0.6])
    for expo, alpha in ((20.0, 0.2), (5.0, 0.6)):
        probe = light(P + 6.0 * np.array([np.sin(alpha), np.cos(alpha), 0.0]), 1.0, le_m)
        E = col_m * le_m * cone_integral(phong_density(expo, UP), *sphere_cone(probe[0][:3], probe[0][3]))
        out.append(Case(f"C-phong{expo:g}", E, spheres=[probe], tri_mat=g.MAT_METAL, col=col_m, phong=expo))
    # F: the default DIFF lobe (no PT_FLAG_COSINE_DIFF, no PT_FLAG_FACE_FORWARD)
    probe = light(P + 6.0 * np.array([np.sin(0.7), np.cos(0.7), 0.0]), 1.0, le_m)
    cone = sphere_cone(probe[0][:3], probe[0][3])
    out.append(Case("F-default-lobe", RHO * le_m * cone_integral(default_lobe_density(), *cone), flags=g.FLAG_MISS_KEEPS_PATH,
                    spheres=[probe], log2_n=19, alt=RHO * le_m * cone_integral(uniform_density(), *cone)))
    # D: PT_FLAG_GLASS_FIX — Schlick and the P = .25 + .5 Re split; a sphere above the plane emits Lu, one below Ld
    lu, ld = np.array([0.3, 0.5, 0.7]), np.array([0.6, 0.4, 0.2])
    sky = [light((0.0, 1020.0, 0.0), 1000.0, lu), light((0.0, -1020.0, 0.0), 1000.0, ld)]
    glass = dict(flags=BASE | g.FLAG_GLASS_FIX, spheres=sky, tri_mat=g.MAT_REFR, col=(1.0, 1.0, 1.0))
    for name, deg, up in (("D-above60", 60.0, False), ("D-below30", 30.0, True), ("D-below70", 70.0, True)):
        th = np.radians(deg)
        toward = (np.sin(th), np.cos(th) if up else -np.cos(th), 0.0)
        c_in = abs(view_direction(toward)[1])
        if not up:
            E, kind = schlick(c_in) * lu + (1.0 - schlick(c_in)) * ld, "mc"
        else:
            cos2t = 1.0 - 1.5 * 1.5 * (1.0 - c_in * c_in)
            if cos2t < 0:
                E, kind = ld, "fixed"            # total reflection: back down, every sample
            else:
                re = schlick(np.sqrt(cos2t))     # the cosine on the air side is the transmitted ray's
                E, kind = re * ld + (1.0 - re) * lu, "mc"
        out.append(Case(name, E, kind, toward=toward, **glass))
    # E: a closed sphere — the plain loop and both roulettes
    far = g.Mesh.from_arrays(np.array([[0, -500, 0], [1, -500, 0], [0, -500, 1]], np.float32), np.array([[0, 1, 2]], np.int32))
    le_e = np.array([0.05, 0.04, 0.03])
    room = dict(mesh=far, spheres=[light((0.0, 0.0, 0.0), 100.0, le_e, RHO)], toward=(0.3, -0.5, 0.2), target=(0.0, 0.0, 0.0))
    for depth in (3, 12):
        E = le_e * sum(RHO ** k for k in range(depth))
        E_cpu = le_e * sum(RHO ** k * 0.81 ** max(0, k - 5) for k in range(depth))
        # a roulette played at hit k changes what hits k + 1 .. gather: the unbiased one starts at hit 3 and the CPU tracer's at
        # hit 6, so at depth 3 neither can change a sample and both are as deterministic as the plain loop
        played = "fixed" if depth == 3 else "mc"
        out += [Case(f"E-plain-depth{depth}", E, "fixed", depth=depth, **room),
                Case(f"E-roulette-depth{depth}", E, played, flags=BASE | g.FLAG_RUSSIAN_ROULETTE, depth=depth, **room),
                Case(f"E-cpu-roulette-depth{depth}", E_cpu, played, flags=BASE | g.FLAG_RR_CPU_TRACER, depth=depth, **room)]
    return out


# ---------------------------------------------------------------------------------------------------- acceptance
def mean_and_se(x):
    """(mean, standard error of the mean) per channel of samples [n][3]"""
    x = np.asarray(x, np.float64)
    return x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(len(x))


def verdict(case, x):
    """What is wrong with the samples (or pixel means) x [n][3] of `case`, as a list of sentences; empty when they hold it.  Returns
    (problems, z, se / E): z the error of the mean in standard errors (mc), in units of the 1e-5 E bound (fixed), or the largest
    sample (zero)."""
    x = np.asarray(x, np.float64)
    E = case.E
    if case.kind == "zero":
        worst = np.abs(x).max(axis=0)
        return (["a sample is not exactly 0"] if worst.any() else []), worst, np.zeros(3)
    if case.kind == "fixed":
        worst = (np.abs(x - E) / (1e-5 * E)).max(axis=0)
        return ([f"a sample leaves E by {worst.max() * 1e-5:.2e} relative"] if (worst > 1).any() else []), worst, np.zeros(3)
    m, se = mean_and_se(x)
    z = (m - E) / se
    bad = [f"mean {m} is {z} standard errors from E {E}"] if not (np.abs(z) <= 5).all() else []
    return bad, z, se / E
