#!/usr/bin/env python3
"""pt_closest_hits / pt_any_hits measured against pt_trace_rays of the same build, same rays, same process: device time
(PT_OPT_TIMING, pt_last_kernel_ms; the median of --reps calls after --warmup) on the bench scene and tree (cornell_dragon, the host
tree, golden camera at 1920x1080).  Three ray sets:
  (a) the pixel-centre camera rays, unbounded                                      pt_trace_rays, pt_closest_hits
  (b) their diffuse bounce, built on the host from (a)'s hits: origin = hit point + 1e-3 x the unit normal facing the ray, a uniformly
      random direction in that hemisphere (fixed seed), unbounded                  pt_trace_rays, pt_closest_hits
  (c) set (b) with t_max = a quarter of the scene's diagonal (ambient occlusion)   pt_closest_hits, pt_any_hits
Usage: python tools/query_bench.py [--out FILE] [--reps 20] [--warmup 3]"""
import argparse
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import gpu_pathtracer_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report here")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--scene", default="cornell_dragon")
ap.add_argument("--seed", type=int, default=9)
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def camera_rays(cam):
    """the pixel-centre ray of every pixel, row-major (pt_camera_ray with zero jitter, in binary32)"""
    f = np.float32
    px, py = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    xs = ((px - f(W) / f(2)) + f(0.5)) * f(cam.dist) * f(cam.aspect) * f(cam.fov) / f(W - 1)
    ys = ((py - f(H) / f(2)) + f(0.5)) * f(cam.dist) * f(cam.fov) / f(H - 1)
    front, right, up, pos = (np.array(list(v), f) for v in (cam.front, cam.right, cam.up, cam.pos))
    dir0 = (front * f(cam.dist))[None, None, :] + xs[..., None] * right + ys[..., None] * up
    rays = np.zeros((H * W, 8), f)
    rays[:, 0:3] = (pos + dir0).reshape(-1, 3)
    rays[:, 4:7] = (dir0 / np.linalg.norm(dir0, axis=-1, keepdims=True)).reshape(-1, 3)
    rays[:, 7] = np.inf                                        # unbounded
    return rays


def bounce_rays(rays, t, tri, nrm, seed):
    """set (b) from set (a)'s hits; rays that hit nothing have no bounce"""
    hit = tri >= 0
    o, d, t, n = rays[hit, 0:3].astype(np.float64), rays[hit, 4:7].astype(np.float64), t[hit].astype(np.float64), nrm[hit].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[np.sum(n * d, axis=1) > 0] *= -1.0                       # facing the ray
    rng = np.random.default_rng(seed)
    v = rng.normal(size=n.shape)
    v /= np.linalg.norm(v, axis=1, keepdims=True)              # uniform on the sphere
    v[np.sum(v * n, axis=1) < 0] *= -1.0                       # ... folded into the normal's hemisphere
    out = np.zeros((len(o), 8), np.float32)
    out[:, 0:3] = o + t[:, None] * d + 1e-3 * n
    out[:, 4:7] = v
    out[:, 7] = np.inf
    return out


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
t.upload_bvh(g.Bvh(mesh))
cam = g.default_camera(W, H)
cam.dist = 18.0 * H / 1080.0
lo, hi = mesh.bounds()
diag = float(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles), host tree, {W}x{H} golden camera; device ms (PT_OPT_TIMING), median / min of {a.reps} calls "
    f"after {a.warmup}; diagonal {diag:.2f}")


class Batch:
    def __init__(self, rays):
        self.n = len(rays)
        self.rays = t.malloc(rays.nbytes)
        self.rays.upload(rays)
        self.d_t, self.d_i, self.d_n, self.d_b = t.malloc(4 * self.n), t.malloc(4 * self.n), t.malloc(12 * self.n), t.malloc(self.n)

    def timed(self, name, fn):
        ms = []
        for _ in range(a.warmup + a.reps):
            fn()
            ms.append(t.last_kernel_ms())
        med, mn = float(np.median(ms[a.warmup:])), float(np.min(ms[a.warmup:]))
        say(f"  {name:<16} {med:8.3f} / {mn:8.3f} ms   {self.n / med / 1e3:9.1f} Mrays/s")
        return med

    def trace(self):
        return self.timed("pt_trace_rays", lambda: t.trace_rays(self.rays.ptr, self.n, True, self.d_t.ptr, self.d_i.ptr, self.d_n.ptr))

    def closest(self):
        return self.timed("pt_closest_hits", lambda: t.closest_hits(self.rays.ptr, self.n, True, self.d_t.ptr, self.d_i.ptr, self.d_n.ptr))

    def any(self):
        return self.timed("pt_any_hits", lambda: t.any_hits(self.rays.ptr, self.n, True, self.d_b.ptr))

    def hits(self):
        t.sync()
        return self.d_t.download(np.float32, (self.n,)), self.d_i.download(np.int32, (self.n,)), self.d_n.download(np.float32, (self.n, 3))

    def free(self):
        for b in (self.rays, self.d_t, self.d_i, self.d_n, self.d_b):
            b.free()


rays_a = camera_rays(cam)
A = Batch(rays_a)
say(f"(a) {A.n} pixel-centre camera rays, unbounded")
ms_trace_a, ms_closest_a = A.trace(), A.closest()
ht, hi_, hn = A.hits()
say(f"  hit share {float((hi_ >= 0).mean()):.4f}; pt_trace_rays / pt_closest_hits = {ms_trace_a / ms_closest_a:.2f}")
rays_b = bounce_rays(rays_a, ht, hi_, hn, a.seed)
A.free()

B = Batch(rays_b)
say(f"(b) {B.n} diffuse bounce rays of (a)'s hits, unbounded")
ms_trace_b, ms_closest_b = B.trace(), B.closest()
_, bi, _ = B.hits()
say(f"  hit share {float((bi >= 0).mean()):.4f}; pt_trace_rays / pt_closest_hits = {ms_trace_b / ms_closest_b:.2f}")
B.free()

rays_c = rays_b.copy()
rays_c[:, 7] = np.float32(0.25 * diag)
Cb = Batch(rays_c)
say(f"(c) set (b) with t_max = {0.25 * diag:.2f} (a quarter of the diagonal): ambient-occlusion rays")
ms_closest_c, ms_any_c = Cb.closest(), Cb.any()
_, ci, _ = Cb.hits()
occ = Cb.d_b.download(np.uint8, (Cb.n,))
say(f"  occluded share {float((occ != 0).mean()):.4f} (closest hits inside the bound: {float((ci >= 0).mean()):.4f}); "
    f"pt_closest_hits / pt_any_hits = {ms_closest_c / ms_any_c:.2f}")
Cb.free()
t.set_option(g.OPT_TIMING, 0)
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
