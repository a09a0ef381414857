#!/usr/bin/env python3
"""pt_render_aux and pt_denoise measured: device time (PT_OPT_TIMING, pt_last_kernel_ms) at 1920x1080 on the bench scene
(cornell_dragon + the sphere room, golden camera), the median of repeated timed calls, for the guide buffers and for the filter
at 1..5 iterations (the default sigmas).
Usage: python tools/denoise_bench.py [--out FILE] [--reps 20]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import gpu_pathtracer_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report here")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--scene", default="cornell_dragon")
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
t.upload_bvh(g.Bvh(mesh))
t.upload_spheres(g.reference_spheres())
cam = g.default_camera(W, H)
cam.dist = 18.0 * H / 1080.0
p = g.default_params(W, H)
p.flags = g.FLAG_WRITE_RGBA
alb, nrm, pos = (t.malloc(W * H * 16) for _ in range(3))
ids = t.malloc(W * H * 4)
acc, rgba = t.alloc_frame(W, H)
out, orgba = t.malloc(W * H * 12), t.malloc(W * H * 4)
t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 4)   # a 4-spp accumulator to filter
t.sync()


def timed(fn):
    ms = []
    for _ in range(a.reps + 2):
        fn()
        ms.append(t.last_kernel_ms())
    return float(np.median(ms[2:])), float(np.min(ms[2:]))


t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}; device ms (PT_OPT_TIMING), median / min of {a.reps} calls")
med, mn = timed(lambda: t.render_aux(cam, p, alb.ptr, nrm.ptr, pos.ptr, ids.ptr))
say(f"pt_render_aux                       {med:7.3f} / {mn:7.3f} ms  ({W * H / med / 1e3:.0f} M primary rays/s)")
dflt = {k: v for k, v in g.DENOISE_DEFAULTS.items() if k != "iterations"}
say(f"pt_denoise, sigmas {dflt}, out + display words:")
for it in range(0, 6):
    med, mn = timed(lambda: t.denoise(acc.ptr, alb.ptr, nrm.ptr, pos.ptr, W, H, out.ptr, orgba.ptr, iterations=it, **dflt))
    say(f"  iterations {it}                      {med:7.3f} / {mn:7.3f} ms")
med, mn = timed(lambda: t.denoise(acc.ptr, alb.ptr, nrm.ptr, pos.ptr, W, H, out.ptr, None, iterations=5, sigma_color=0.0,
                                  sigma_normal=0.0, sigma_position=0.0))
say(f"  iterations 5, every term off        {med:7.3f} / {mn:7.3f} ms")
t.set_option(g.OPT_TIMING, 0)
for b in (alb, nrm, pos, ids, acc, rgba, out, orgba):
    b.free()
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
