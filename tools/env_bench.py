#!/usr/bin/env python3
"""What an environment map (pt_upload_environment) costs, against bk_color in the same build, scene and process: device time
(PT_OPT_TIMING, pt_last_kernel_ms; the median of --reps calls after --warmup) of pt_render with PT_KERNEL_PERSISTENT on an OPEN
scene — the dragon alone, no spheres, the tree built on the device, a camera in front of it that it fills ~45 % of, 1920x1080,
16 samples per call, depth 4, PT_FLAGS_SMALLPT:
  (a) bk_color                              the constant every path that leaves the scene gathered before
  (b) a 64 x 32 map, nearest / bilinear     fits the caches: the cost of the lookup's arithmetic
  (c) a 4096 x 2048 map, nearest / bilinear 128 MiB of texels: the cost of its gathers too
  (d) pt_eval_environment over 2 M random directions, both map sizes, bilinear
and the share of the call's segments that hit nothing, from one instrumented call (PT_OPT_COUNTERS).  The figures to read are
(b) / (a) and (c) / (a).
Usage: python tools/env_bench.py [--out FILE] [--reps 9] [--warmup 2] [--scene dragon]"""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scene", default="dragon")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=4)
ap.add_argument("--eval-rays", type=int, default=2_000_000)
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sky(w, h):
    """a smooth sky with a bright patch, float32 [h][w][3]"""
    y, x = np.meshgrid(np.linspace(-0.5, 0.5, h, dtype=np.float32), np.linspace(-1.0, 1.0, w, dtype=np.float32), indexing="ij")
    base = np.stack([0.4 + 0.3 * y, 0.5 + 0.4 * y, 0.7 + 0.5 * y], -1)
    sun = 8.0 * np.exp(-((x - 0.3) ** 2 + (y - 0.25) ** 2) / 0.002)
    return (base + sun[..., None]).astype(np.float32)


def timed(name, fn, unit, count):
    ms = []
    for _ in range(a.warmup + a.reps):
        fn()
        ms.append(t.last_kernel_ms())
    med, mn = float(np.median(ms[a.warmup:])), float(np.min(ms[a.warmup:]))
    say(f"  {name:<44} {med:9.3f} / {mn:9.3f} ms   {count / med / 1e3:8.1f} M{unit}/s")
    return med


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
build_ms = t.build_bvh(mesh)
lo, hi = mesh.bounds()
cam = g.default_camera(W, H)
ext = float(np.max(hi - lo))
cam.dist = 1.0   # the image plane one unit in front of pos (the default's 18 units would start the rays on a plane wider than the mesh)
cam.pos[:] = (0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), float(hi[2]) + 0.35 * ext)   # looks along -z: the mesh fills ~45 % of the frame
p = g.default_params(W, H, depth=a.depth)
p.frame, p.sample_index, p.flags = 0, 1, g.FLAGS_SMALLPT
p.bk_color[:] = (0.5, 0.6, 0.8)
t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
acc, rgba = t.alloc_frame(W, H)
say(f"{a.scene} ({mesh.n_tris} triangles) alone, no spheres, tree built on the device ({build_ms:.1f} ms), {W}x{H}, {a.spp} samples per call, "
    f"depth {a.depth}, PT_FLAGS_SMALLPT, PT_KERNEL_PERSISTENT; device ms (PT_OPT_TIMING), median / min of {a.reps} calls after {a.warmup}")

t.set_option(g.OPT_COUNTERS, 1)
t.launch_kernel(acc.ptr, rgba.ptr, cam, p, a.spp)
t.sync()
c = t.counters()
t.set_option(g.OPT_COUNTERS, 0)
say(f"  segments {c['rays']}, of them ending on a triangle {c['hits']}: {100.0 * (1.0 - c['hits'] / max(c['rays'], 1)):.1f} % of the segments hit nothing "
    f"({c['paths']} paths, {c['rays'] / max(c['paths'], 1):.2f} segments each)")

t.set_option(g.OPT_TIMING, 1)
paths = W * H * a.spp
render = lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, a.spp)   # noqa: E731
ms_bk = timed("(a) bk_color", render, "paths", paths)
rng = np.random.default_rng(6)
d = rng.normal(size=(a.eval_rays, 3))
rays = np.zeros((a.eval_rays, 8), np.float32)
rays[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
d_rays, d_out = t.malloc(rays.nbytes), t.malloc(12 * a.eval_rays)
d_rays.upload(rays)
for tag, (w, h) in (("(b)", (64, 32)), ("(c)", (4096, 2048))):
    tex = sky(w, h)
    for fname, filt in (("nearest", g.ENV_NEAREST), ("bilinear", g.ENV_BILINEAR)):
        t.upload_environment(tex, filter=filt)
        ms = timed(f"{tag} {w} x {h} map, {fname}", render, "paths", paths)
        say(f"      / (a) = {ms / ms_bk:.3f}")
    timed(f"(d) pt_eval_environment, {w} x {h}, bilinear", lambda: t.eval_environment(d_rays.ptr, a.eval_rays, d_out.ptr), "rays", a.eval_rays)
t.clear_environment()
ms_again = timed("(a) bk_color again, the map cleared", render, "paths", paths)
say(f"      / (a) = {ms_again / ms_bk:.3f}")
for b in (d_rays, d_out, acc, rgba):
    b.free()
t.set_option(g.OPT_TIMING, 0)
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
