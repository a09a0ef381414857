#!/usr/bin/env python3
"""pt_meter and pt_tonemap measured: device time (PT_OPT_TIMING, pt_last_kernel_ms) at 1920x1080 on the bench scene's accumulator
(cornell_dragon + the sphere room, golden camera, 4 spp), the median of repeated timed calls: the meter, the tone map per curve and
transfer, with and without out_dev, on the four-pixel route (aligned buffers) and on the one-pixel route (bases 12 bytes past a
16-byte boundary).  Beside them two baselines of the same session: pt_denoise(iterations = 0, rgba_dev), a copy plus pack over the
same bytes, and the host route pt_app takes without the display flags — the download of the accumulator plus a clamp-and-pack on
the CPU (here numpy's, wall clock).
Usage: python tools/tonemap_bench.py [--out FILE] [--reps 20]"""
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
ap.add_argument("--scene", default="cornell_dragon")
a = ap.parse_args()
W, H = 1920, 1080
N = W * H
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
acc, rgba = t.alloc_frame(W, H)
t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 4)
t.sync()
frame = acc.download(np.float32, (H, W, 3))
out, words, state = t.malloc(N * 12), t.malloc(N * 4), t.malloc(16)
state.zero()
# the same frame and outputs 12 bytes past a 16-byte boundary: the one-pixel route
acc_o, out_o, words_o = t.malloc(N * 12 + 16), t.malloc(N * 12 + 16), t.malloc(N * 4 + 16)
t._check(t._lib.pt_upload(t._ctx, acc_o.ptr + 12, frame.ctypes.data, frame.nbytes))
guides = [t.malloc(N * 16) for _ in range(3)]   # pt_denoise(iterations = 0) reads none of them
for b in guides:
    b.zero()


def timed(fn):
    ms = []
    for _ in range(a.reps + 2):
        fn()
        ms.append(t.last_kernel_ms())
    return float(np.median(ms[2:])), float(np.min(ms[2:])), float(np.max(ms[2:]))


def row(name, fn, bytes_moved):
    med, mn, mx = timed(fn)
    say(f"  {name:<52s} {med * 1e3:8.1f} / {mn * 1e3:8.1f} / {mx * 1e3:8.1f} us   {bytes_moved / med / 1e6:7.1f} GB/s")
    return med


t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}, 4 spp accumulator; device time (PT_OPT_TIMING), median / min / max of {a.reps} calls; "
    f"GB/s = bytes the call must move / median")
say("baseline on the device: pt_denoise(iterations = 0), out + display words (a copy plus the truncating pack; unchanged by this commit)")
base = row("pt_denoise iterations 0, out + rgba", lambda: t.denoise(acc.ptr, guides[0].ptr, guides[1].ptr, guides[2].ptr, W, H, out.ptr, words.ptr, iterations=0), N * 28)
say("pt_meter (two launches: histograms, finish)")
row("pt_meter, aligned", lambda: t.meter(acc.ptr, W, H, state.ptr), N * 12)
row("pt_meter, base + 12 bytes (one pixel per thread)", lambda: t.meter(acc_o.ptr + 12, W, H, state.ptr), N * 12)
say("pt_tonemap, rgba_dev only, aligned (four pixels per thread)")
lin = None
for cname, curve in (("clamp", g.TONE_CLAMP), ("reinhard white 4", g.TONE_REINHARD), ("aces", g.TONE_ACES)):
    for xname, xfer in (("linear", g.XFER_LINEAR), ("srgb", g.XFER_SRGB), ("gamma22", g.XFER_GAMMA22)):
        med = row(f"{cname} + {xname}", lambda: t.tonemap(acc.ptr, W, H, rgba_ptr=words.ptr, curve=curve, transfer=xfer, white=4.0), N * 16)
        if lin is None:
            lin = med
say("pt_tonemap with out_dev")
both = row("clamp + linear, out + rgba (the baseline's bytes)", lambda: t.tonemap(acc.ptr, W, H, rgba_ptr=words.ptr, out_ptr=out.ptr), N * 28)
row("aces + srgb, out + rgba", lambda: t.tonemap(acc.ptr, W, H, rgba_ptr=words.ptr, out_ptr=out.ptr, curve=g.TONE_ACES, transfer=g.XFER_SRGB), N * 28)
row("aces + srgb, out only", lambda: t.tonemap(acc.ptr, W, H, out_ptr=out.ptr, curve=g.TONE_ACES, transfer=g.XFER_SRGB), N * 24)
row("aces + srgb, exposure from pt_meter's state", lambda: t.tonemap(acc.ptr, W, H, rgba_ptr=words.ptr, curve=g.TONE_ACES, transfer=g.XFER_SRGB, exposure_ptr=state.ptr), N * 16)
say("pt_tonemap, bases + 12 bytes (one pixel per thread)")
row("clamp + linear, rgba", lambda: t.tonemap(acc_o.ptr + 12, W, H, rgba_ptr=words_o.ptr + 12), N * 16)
row("clamp + linear, out + rgba", lambda: t.tonemap(acc_o.ptr + 12, W, H, rgba_ptr=words_o.ptr + 12, out_ptr=out_o.ptr + 12), N * 28)
row("aces + srgb, rgba", lambda: t.tonemap(acc_o.ptr + 12, W, H, rgba_ptr=words_o.ptr + 12, curve=g.TONE_ACES, transfer=g.XFER_SRGB), N * 16)
t.set_option(g.OPT_TIMING, 0)
say(f"ratios: tone map clamp + linear, out + rgba / pt_denoise(0) = {both / base:.2f}; rgba only / pt_denoise(0) = {lin / base:.2f}")

# the host route: what pt_app does without the display flags for the routes that have no display words
wall = []
for _ in range(5):
    t.sync()
    t0 = time.perf_counter()
    host = acc.download(np.float32, (H, W, 3))
    t1 = time.perf_counter()
    q = (np.clip(host, 0.0, 1.0) * np.float32(255.0)).astype(np.uint32)
    packed = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16)
    t2 = time.perf_counter()
    wall.append((t1 - t0, t2 - t1))
dl, pk = np.median([w[0] for w in wall]), np.median([w[1] for w in wall])
say(f"baseline on the host (wall clock, median of 5): download of {N * 12 / 1e6:.1f} MB {dl * 1e3:.2f} ms + clamp-and-pack on the CPU (numpy) {pk * 1e3:.2f} ms "
    f"= {(dl + pk) * 1e3:.2f} ms, {(dl + pk) * 1e3 / lin:.0f} x the device tone map (rgba only); the words alone would still be a {N * 4 / 1e6:.1f} MB download")
for b in [acc, rgba, out, words, state, acc_o, out_o, words_o] + guides:
    b.free()
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
