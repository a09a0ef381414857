#!/usr/bin/env python3
"""pt_render_rays measured against pt_render of the same build, same scene, same process: device time (PT_OPT_TIMING,
pt_last_kernel_ms; the median of --reps calls after --warmup) on the bench scene (cornell_dragon_800k with the sphere room, the tree
built on the device, bench.py's camera at 1920x1080, 16 samples per call, depth 4):
  (a) pt_render with PT_KERNEL_PERSISTENT                       the frame kernel the ray kernel is modelled on
  (b) pt_render_rays over that camera's own pixel-centre rays   one 32-byte read per path instead of the camera, no jitter
  (c) pt_render_rays over a probe: 4 096 rays x 256 samples     few rays, many samples: uniformly random directions from the
                                                                camera position, HDR mode
The figure to read is (b) / (a): the two trace the same number of paths of the same length through the same loop.
Usage: python tools/rays_bench.py [--out FILE] [--reps 9] [--warmup 2]"""
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
ap.add_argument("--scene", default="cornell_dragon_800k")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--depth", type=int, default=4)
ap.add_argument("--probe-rays", type=int, default=4096)
ap.add_argument("--probe-spp", type=int, default=256)
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
    return rays


def timed(name, paths, fn):
    ms = []
    for _ in range(a.warmup + a.reps):
        fn()
        ms.append(t.last_kernel_ms())
    med, mn = float(np.median(ms[a.warmup:])), float(np.min(ms[a.warmup:]))
    say(f"  {name:<44} {med:9.3f} / {mn:9.3f} ms   {paths / med / 1e3:8.1f} Mpaths/s")
    return med


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
build_ms = t.build_bvh(mesh)
t.upload_spheres(g.reference_spheres())
cam = g.default_camera(W, H)
p = g.default_params(W, H, depth=a.depth)
p.frame, p.sample_index = 0, 1
t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + sphere room, tree built on the device ({build_ms:.1f} ms), {W}x{H}, {a.spp} samples per call, "
    f"depth {a.depth}; device ms (PT_OPT_TIMING), median / min of {a.reps} calls after {a.warmup}")

acc, rgba = t.alloc_frame(W, H)
t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
ms_render = timed("(a) pt_render, PT_KERNEL_PERSISTENT", W * H * a.spp, lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, a.spp))

rays = camera_rays(cam)
d_rays = t.malloc(rays.nbytes)
d_rays.upload(rays)
ms_rays = timed("(b) pt_render_rays, the camera's centre rays", W * H * a.spp, lambda: t.render_rays(d_rays.ptr, W * H, acc.ptr, p, a.spp))
say(f"  (b) / (a) = {ms_rays / ms_render:.3f}")
ms_one = timed("    the same, 1 sample per call (folds in line)", W * H, lambda: t.render_rays(d_rays.ptr, W * H, acc.ptr, p, 1))
ms_one_r = timed("    pt_render, 1 sample per call", W * H, lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 1))
say(f"  1 sample per call: pt_render_rays / pt_render = {ms_one / ms_one_r:.3f}")
d_rays.free()

rng = np.random.default_rng(4)
d = rng.normal(size=(a.probe_rays, 3))
probe = np.zeros((a.probe_rays, 8), np.float32)
probe[:, 0:3] = np.array(list(cam.pos), np.float32) + np.array([0.0, 0.0, -20.0], np.float32)   # the middle of the room
probe[:, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
d_probe = t.malloc(probe.nbytes)
d_probe.upload(probe)
say(f"(c) a probe in the middle of the room: {a.probe_rays} rays x {a.probe_spp} samples, HDR")
ms_probe = timed("(c) pt_render_rays, one call", a.probe_rays * a.probe_spp,
                 lambda: t.render_rays(d_probe.ptr, a.probe_rays, acc.ptr, p, a.probe_spp, hdr=True))
say(f"  paths per ms: probe {a.probe_rays * a.probe_spp / ms_probe:.0f}, frame batch {W * H * a.spp / ms_rays:.0f} "
    f"(ratio {a.probe_rays * a.probe_spp / ms_probe / (W * H * a.spp / ms_rays):.2f}: incoherent first segments against a camera's)")
d_probe.free()
acc.free()
rgba.free()
t.set_option(g.OPT_TIMING, 0)
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
