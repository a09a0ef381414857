"""The reference of pt_closest_hits / pt_any_hits (tests/test_query.py, tests/test_gpu_query.py): incoherent rays, brute force
filtered by the bound, and the eight bound classes.  Numpy + orc; needs the built host library and no GPU.

A triangle is hit when 0 < t < t_max in binary32, strict on both sides.  The nearest hit inside that interval is brute force's
nearest hit when it lies inside and nothing otherwise, so
  closest(ray) = brute force's (t, id, normal) where 0 < t < t_max, else (FLT_MAX, -1, 0)
  any(ray)     = that predicate.
A NaN t_max fails both comparisons: a miss, like 0 and a negative one."""
import numpy as np

import gpu_pathtracer_amd as g
import orc

FLT_MAX = np.float32(3.402823466e+38)
N_CLASSES = 8
NEVER_OCCLUDED, OCCLUDED_WHERE_HIT = (0, 1, 5, 6, 7), (2, 3, 4)


def random_rays(mesh, n, seed):
    """Rays from around the mesh towards points of its bounding box (the generator of test_gpu_build, restated); words 3 and 7 zero."""
    rng = np.random.default_rng(seed)
    lo, hi = mesh.bounds()
    c, r = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    o = c + rng.normal(size=(n, 3)) * r * 1.2
    tgt = lo + rng.random((n, 3)) * (hi - lo)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 4:7] = o, d
    return rays


def diagonal(mesh):
    lo, hi = mesh.bounds()
    return np.float32(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))


def class_bounds(t_brute, diag):
    """t_max of ray i by its class i % 8, from its own brute-force t (the scene's diagonal where it misses):
    0: 0.5 t   1: t exactly (a miss: the bound is strict)   2: the next float above t (a hit)   3: 2 t   4: +inf   5: 0   6: -1   7: NaN"""
    t = np.asarray(t_brute, np.float32)
    base = np.where(t < FLT_MAX, t, np.float32(diag)).astype(np.float32)
    cls = np.arange(len(t)) % N_CLASSES
    inf = np.float32(np.inf)
    choices = [np.float32(0.5) * base, base, np.nextafter(base, inf), np.float32(2.0) * base, np.full_like(base, inf),
               np.zeros_like(base), np.full_like(base, -1.0), np.full_like(base, np.nan)]
    return np.choose(cls, choices).astype(np.float32), cls


def with_bounds(rays, t_max):
    out = np.array(rays, np.float32)
    out[:, 7] = t_max
    return out


def filter_by_bound(brute, t_max):
    """(t, id, normal, any) of the bounded queries from brute force's unbounded (t, id, normal)"""
    t, tri, nrm = brute
    with np.errstate(invalid="ignore"):
        inside = (tri >= 0) & (t > 0) & (t < np.asarray(t_max, np.float32))
    return (np.where(inside, t, FLT_MAX).astype(np.float32), np.where(inside, tri, -1).astype(np.int32),
            np.where(inside[:, None], nrm, np.float32(0)).astype(np.float32), inside)


_cache = {}


def brute(name, mesh, rays_key, rays, cull):
    """orc.trace_brute, once per (scene name, ray set, cull) for the whole run; the result is shared: leave it unchanged"""
    key = (name, rays_key, bool(cull))
    if key not in _cache:
        _cache[key] = orc.trace_brute(mesh, rays, cull)
    return _cache[key]


def case(name, n, seed, cull):
    """The inputs and the reference of one scene: (mesh, rays with the eight classes in word 7, class of every ray,
    brute force's unbounded (t, id, normal), the bounded reference (t, id, normal, any))."""
    key = ("case", name, n, seed, bool(cull))
    if key not in _cache:
        mesh = g.scene_mesh(name)
        rays = random_rays(mesh, n, seed)
        b = brute(name, mesh, (n, seed), rays, cull)
        t_max, cls = class_bounds(b[0], diagonal(mesh))
        _cache[key] = (mesh, with_bounds(rays, t_max), cls, b, filter_by_bound(b, t_max))
    return _cache[key]


def shares(cls, brute_tri, occluded):
    """(hit share of the unbounded rays, occluded share of the bounded ones), and the per-class rules as a list of failures"""
    hit = brute_tri >= 0
    bad = []
    for c in NEVER_OCCLUDED:
        if occluded[cls == c].any():
            bad.append(f"class {c} has occluded rays")
    for c in OCCLUDED_WHERE_HIT:
        if not np.array_equal(occluded[cls == c], hit[cls == c]):
            bad.append(f"class {c} is not occluded exactly where the ray hits")
    return float(hit.mean()), float(occluded.mean()), bad
