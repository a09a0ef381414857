#!/usr/bin/env python3
"""What asking pt_render for luminance moments costs, measured: device time (PT_OPT_TIMING: pt_last_kernel_ms for the whole call,
pt_get_stage_ms[PT_STAGE_FOLD] for the fold) at 1920x1080 on bench.py's scene and tree (cornell_dragon_800k, the host SAH tree without spatial splits, + the sphere room,
golden camera),
the median of repeated timed calls, the same call with and without a moments buffer — 16 / 4 / 1 samples per call on the
stage-split pipeline, 1 on the persistent kernel — and the wall time of pt_frame_error on the frame's moments.
Usage: python tools/moments_bench.py [--out FILE] [--reps 20]"""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import gpu_pathtracer_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report here")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--scene", default="cornell_dragon_800k")
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
t.upload_bvh(g.Bvh(mesh, split_alpha=-1.0))   # bench.py's tree
t.upload_spheres(g.reference_spheres())
cam = g.default_camera(W, H)
cam.dist = 18.0 * H / 1080.0
p = g.default_params(W, H)
p.flags = g.FLAG_WRITE_RGBA
acc, rgba = t.alloc_frame(W, H)
mom = t.malloc(W * H * 8)


def timed(spp, moments_ptr):
    """(median whole-call ms, median fold ms) of a.reps timed calls after two warm-up calls; a running mean, as a viewer drives it."""
    call, fold = [], []
    for k in range(a.reps + 2):
        p.frame, p.sample_index = k * spp, k * spp + 1
        t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp, moments_ptr=moments_ptr)
        call.append(t.last_kernel_ms())
        fold.append(t.stage_ms()["fold"])
    return float(np.median(call[2:])), float(np.median(fold[2:]))


t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}; device ms (PT_OPT_TIMING), medians of {a.reps} calls")
say("kernel      spp | call ms: plain  moments  (+)      | fold ms: plain  moments  (+)")
for name, kernel, spp in (("pipeline", g.KERNEL_WAVEFRONT, 16), ("pipeline", g.KERNEL_WAVEFRONT, 4), ("pipeline", g.KERNEL_WAVEFRONT, 1),
                          ("persistent", g.KERNEL_PERSISTENT, 1)):
    t.set_option(g.OPT_KERNEL, kernel)
    c0, f0 = timed(spp, None)
    c1, f1 = timed(spp, mom.ptr)
    say(f"{name:<11} {spp:3d} |         {c0:7.3f} {c1:7.3f} ({c1 - c0:+.3f}) |         {f0:6.3f} {f1:7.3f} ({f1 - f0:+.3f})")
say("(fold ms 0: the call has no fold launch — the pipeline's last shade launch folds 16 / 8 / 4 samples per call, the persistent")
say(" kernel folds one sample in line; with moments such a call always runs the separate fold over its sample buffer)")
t.set_option(g.OPT_TIMING, 0)
t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
t.sync()
n = (a.reps + 2)   # the moments hold the last series: (reps + 2) one-sample calls
wall = []
for _ in range(a.reps + 2):
    t0 = time.perf_counter()
    mean_rse, above = t.frame_error(mom.ptr, W, H, n, 0.05)
    wall.append((time.perf_counter() - t0) * 1e3)
say(f"pt_frame_error {W}x{H} (launch + {(W * H + 255) // 256 * 12} bytes back + host sum), wall: median {np.median(wall[2:]):.3f} ms, "
    f"min {min(wall[2:]):.3f} ms; mean_rse {mean_rse:.6f}, {above} pixels above 0.05 after {n} samples")
for b in (acc, rgba, mom):
    b.free()
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
