#!/usr/bin/env python3
"""pt_render_aux_camera and pt_temporal_camera measured: device time (PT_OPT_TIMING, pt_last_kernel_ms) at 1920x1080 on the bench
scene (cornell_dragon + the sphere room, golden camera), the median of repeated timed calls, in one session: pt_render_aux beside
pt_render_aux_camera under each of the five models, and pt_temporal beside pt_temporal_camera under each model (no rows, with ids;
the history is the model's own guides one degree of pan earlier, colours random), with and without the motion buffer.
Usage: python tools/camera_guides_bench.py [--out FILE] [--reps 20]"""
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
N = W * H
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def panned(cam, deg):
    """A copy of cam turned by deg about its up (pt_app's --pan-deg)."""
    c = g.Camera.from_buffer_copy(cam)
    up, th = np.array(list(cam.up), np.float64), np.deg2rad(deg)
    for name in ("front", "right"):
        v = np.array(list(getattr(cam, name)), np.float64)
        getattr(c, name)[:] = [float(x) for x in v * np.cos(th) + np.cross(up, v) * np.sin(th) + up * np.dot(up, v) * (1.0 - np.cos(th))]
    return c


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
t.upload_bvh(g.Bvh(mesh))
t.upload_spheres(g.reference_spheres())
cam = g.default_camera(W, H)
cam.dist = 18.0 * H / 1080.0
cam1 = panned(cam, 1.0)
p = g.default_params(W, H)
MODELS = (("pinhole", {}), ("thinlens", dict(lens_radius=0.5, focus_dist=35.0)), ("ortho", dict(ortho_height=30.0)),
          ("fisheye", dict(fisheye_fov=float(np.pi))), ("equirect", {}))
prev_g = [t.malloc(N * 16) for _ in range(3)] + [t.malloc(N * 4)]
cur_g = [t.malloc(N * 16) for _ in range(3)] + [t.malloc(N * 4)]
rng = np.random.default_rng(1)
prev_c, cur_c, out_c = t.malloc(N * 12), t.malloc(N * 12), t.malloc(N * 12)
prev_l, out_l, words, motion = t.malloc(N * 4), t.malloc(N * 4), t.malloc(N * 4), t.malloc(N * 8)
prev_c.upload(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
cur_c.upload(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
prev_l.upload(rng.integers(1, 41, (H, W)).astype(np.float32))


def timed(fn):
    ms = []
    for _ in range(a.reps + 2):
        fn()
        ms.append(t.last_kernel_ms())
    return float(np.median(ms[2:])), float(np.min(ms[2:])), float(np.max(ms[2:]))


def row(name, fn):
    med, mn, mx = timed(fn)
    say(f"  {name:<58s} {med * 1e3:8.1f} / {mn * 1e3:8.1f} / {mx * 1e3:8.1f} us")
    return med


def ptrs(bufs):
    return [b.ptr for b in bufs]


t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}; device time (PT_OPT_TIMING), median / min / max of {a.reps} calls")
say("guide buffers (four outputs)")
base_aux = row("pt_render_aux", lambda: t.render_aux(cam, p, *ptrs(cur_g)))
aux = {}
for name, kw in MODELS:
    cm = g.camera_model(name, W, H, centre=True, **kw)
    aux[name] = row(f"pt_render_aux_camera {name}", lambda: t.render_aux_camera(cam, cm, p, *ptrs(cur_g)))
say("reprojection (history: the same model one degree of pan earlier; ids, display words)")
t.render_aux(cam, p, *ptrs(prev_g))
t.render_aux(cam1, p, *ptrs(cur_g))
base_tm = row("pt_temporal", lambda: t.temporal(W, H, cam, prev_c.ptr, prev_l.ptr, *ptrs(prev_g)[1:], cur_c.ptr, *ptrs(cur_g)[1:], out_c.ptr, out_l.ptr, words.ptr))
tm = {}
for name, kw in MODELS:
    cm = g.camera_model(name, W, H, centre=True, **kw)
    t.render_aux_camera(cam, cm, p, *ptrs(prev_g))
    t.render_aux_camera(cam1, cm, p, *ptrs(cur_g))
    for with_motion in (False, True):
        tm[name, with_motion] = row(f"pt_temporal_camera {name}{' + motion' if with_motion else ''}",
                                    lambda: t.temporal_camera(W, H, cam, cm, prev_c.ptr, prev_l.ptr, *ptrs(prev_g)[1:], cur_c.ptr, *ptrs(cur_g)[1:],
                                                              out_c.ptr, out_l.ptr, words.ptr, motion.ptr if with_motion else None))
    t.sync()
    say(f"    history taken on {float((out_l.download(np.float32, (H, W)) > 1).mean()):.3f} of the pixels")
t.set_option(g.OPT_TIMING, 0)
say("ratios to the pinhole calls: " + ", ".join(f"aux {n} {aux[n] / base_aux:.2f}" for n, _ in MODELS) + "; "
    + ", ".join(f"temporal {n} {tm[n, False] / base_tm:.2f}" for n, _ in MODELS))
for b in prev_g + cur_g + [prev_c, cur_c, out_c, prev_l, out_l, words, motion]:
    b.free()
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
