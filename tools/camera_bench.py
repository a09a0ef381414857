#!/usr/bin/env python3
"""pt_camera_rays measured on the bench scene (cornell_dragon_800k with the sphere room, the tree built on the device, bench.py's
camera at 1920x1080, depth 4), device time by PT_OPT_TIMING (pt_last_kernel_ms; the median of --reps after --warmup):
  (a) the generator alone, per camera model: one call writes the 2 073 600 rays of a frame (66 MB)
  (b) a 16-sample frame through PathTracer.render_camera's loop — 16 x (pt_camera_rays, one-sample pt_render_rays), a fresh
      jittered ray per sample — against ONE pt_render_rays(spp = 16) call over fixed rays (the pinhole's centre rays, made by the
      generator once): what anti-aliasing costs.  The loop's device time is the sum over its 32 calls, split into the generator's
      share and the one-sample traces'; the wall clock from sync to sync of both is printed beside it (the loop untimed there).
  (c) the same frame three ways, per model, each as the span of ONE timed region on the stream (wall clock from sync to sync with
      PT_OPT_TIMING off, so the loop's launches queue up as they do in a host's frame loop) and, for the single calls, the device
      time of pt_last_kernel_ms beside it: (i) the loop, (ii) pt_render_camera(spp = 16) — PathTracer.render_model, the rays made
      in the path kernel — and (iii) pt_render_rays(spp = 16) over fixed rays.  Median and min .. max of --reps after --warmup;
      the three are interleaved rep by rep so that drift hits them alike.
Usage: python tools/camera_bench.py [--out FILE] [--reps 7] [--warmup 2]"""
import argparse
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import gpu_pathtracer_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report here")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scene", default="cornell_dragon_800k")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=4)
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return float(np.median(v[a.warmup:]))


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
build_ms = t.build_bvh(mesh)
t.upload_spheres(g.reference_spheres())
cam = g.default_camera(W, H)
p = g.default_params(W, H, depth=a.depth)
p.frame, p.sample_index = 0, 1
say(f"{a.scene} ({mesh.n_tris} triangles) + sphere room, tree built on the device ({build_ms:.1f} ms), {W}x{H}, depth {a.depth}; "
    f"medians of {a.reps} after {a.warmup}")
rays = t.malloc(32 * W * H)
out = t.malloc(12 * W * H)
MODELS = [("pinhole", {}), ("thinlens", dict(lens_radius=0.5, focus_dist=35.0)), ("ortho", dict(ortho_height=30.0)),
          ("fisheye", dict(fisheye_fov=np.pi)), ("equirect", {})]

say("(a) pt_camera_rays, one frame of rays, device ms (and GB/s of the 66 MB written)")
t.set_option(g.OPT_TIMING, 1)
for name, kw in MODELS:
    for centre in (False, True):
        cm = g.camera_model(name, W, H, centre=centre, **kw)
        ms = []
        for k in range(a.warmup + a.reps):
            t.camera_rays(cam, cm, k, rays.ptr)
            ms.append(t.last_kernel_ms())
        say(f"  {name:<9} {'centred ' if centre else 'jittered'} {med(ms):8.4f} ms   {32.0 * W * H / med(ms) / 1e6:7.0f} GB/s")

say(f"(b) a {a.spp}-sample frame: the generate-then-trace loop against one pt_render_rays(spp = {a.spp}) over fixed rays")
for name, kw in MODELS:
    cm = g.camera_model(name, W, H, **kw)
    fixed = g.camera_model(name, W, H, centre=True, **kw)
    gen, trace, one, wall_loop, wall_one = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        # the loop, timed call by call (reading a call's time waits for it: the sums are device time, not the loop's wall clock)
        q = g.Params.from_buffer_copy(p)
        g_ms = r_ms = 0.0
        for s in range(a.spp):
            q.frame, q.sample_index = p.frame + s, p.sample_index + s
            t.camera_rays(cam, cm, q.frame, rays.ptr)
            g_ms += t.last_kernel_ms()
            t.render_rays(rays.ptr, W * H, out.ptr, q, 1)
            r_ms += t.last_kernel_ms()
        gen.append(g_ms)
        trace.append(r_ms)
        # the fixed-ray call
        t.camera_rays(cam, fixed, 0, rays.ptr)
        t.render_rays(rays.ptr, W * H, out.ptr, p, a.spp)
        one.append(t.last_kernel_ms())
        # wall clock, sync to sync
        t.set_option(g.OPT_TIMING, 0)
        t.sync()
        t0 = time.perf_counter()
        t.render_rays(rays.ptr, W * H, out.ptr, p, a.spp)
        t.sync()
        wall_one.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        t.render_camera(cam, cm, p, out.ptr, rays.ptr, spp=a.spp)
        t.sync()
        wall_loop.append((time.perf_counter() - t0) * 1e3)
        t.set_option(g.OPT_TIMING, 1)
    loop = med(gen) + med(trace)
    say(f"  {name:<9} loop {loop:8.3f} ms = generator {med(gen):6.3f} + {a.spp} one-sample traces {med(trace):8.3f};  fixed rays, one call {med(one):8.3f} ms;"
        f"  loop / one call = {loop / med(one):.3f}   (wall clock {med(wall_loop):8.3f} / {med(wall_one):8.3f} = {med(wall_loop) / med(wall_one):.3f})")
say(f"(c) a {a.spp}-sample frame, wall clock sync to sync in ms, median [min .. max]: (i) the loop, (ii) pt_render_camera(spp = {a.spp}), "
    f"(iii) pt_render_rays(spp = {a.spp}) over fixed rays; device ms of (ii) and (iii) by PT_OPT_TIMING")


def wall(fn):
    t.sync()
    t0 = time.perf_counter()
    fn()
    t.sync()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    v = v[a.warmup:]
    return f"{np.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"


for name, kw in MODELS:
    cm = g.camera_model(name, W, H, **kw)
    fixed = g.camera_model(name, W, H, centre=True, **kw)
    w_loop, w_fused, w_fixed, d_fused, d_fixed = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        t.set_option(g.OPT_TIMING, 0)
        w_loop.append(wall(lambda: t.render_camera(cam, cm, p, out.ptr, rays.ptr, spp=a.spp)))
        w_fused.append(wall(lambda: t.render_model(cam, cm, p, out.ptr, spp=a.spp)))
        t.camera_rays(cam, fixed, 0, rays.ptr)
        w_fixed.append(wall(lambda: t.render_rays(rays.ptr, W * H, out.ptr, p, a.spp)))
        t.set_option(g.OPT_TIMING, 1)
        t.render_model(cam, cm, p, out.ptr, spp=a.spp)
        d_fused.append(t.last_kernel_ms())
        t.render_rays(rays.ptr, W * H, out.ptr, p, a.spp)
        d_fixed.append(t.last_kernel_ms())
    say(f"  {name:<9} (i) {spread(w_loop)}  (ii) {spread(w_fused)}  (iii) {spread(w_fixed)}   (i) / (ii) = {med(w_loop) / med(w_fused):.3f}, "
        f"(ii) - (iii) = {med(w_fused) - med(w_fixed):+.3f} ms;  device (ii) {spread(d_fused)}  (iii) {spread(d_fixed)}")
rays.free()
out.free()
t.set_option(g.OPT_TIMING, 0)
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
