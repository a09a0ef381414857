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

--mode light: what sampling the map as a light (PT_OPT_ENV_LIGHT, upload_environment(light=True)) buys on the same scene and
camera under next-event estimation (PT_FLAGS_SMALLPT | PT_FLAG_NEE; the megakernel renders): a 4096 x 2048 bilinear map, dim sky
with a sun of a few texels (radiance 20 000, 3 x 3 texels, 45 degrees up behind the camera's right shoulder),
  (e) the step time with the light off, on, and on with PT_FLAG_MIS (the shadow rays weighed against the bounce rays)
  (f) pt_frame_error's mean relative standard error of the frame after equal TIME: --budget-ms of device time each, whole calls,
      with the frame's mean luminance and the number of pixels the sun has reached beside it: the error is estimated from the
      samples, so a pixel whose bounce rays never found the sun reports a small error around the wrong mean; and the firefly
      pixels: those whose own relative standard error is still above 0.5
  (g) pt_sample_environment: 2 M draws, with and without the radiance
--skip-light runs (e) and (f) with the light off only and nothing that needs the option: the same file run in a checkout of an
earlier commit gives that commit's time for the same frame.
Usage: python tools/env_bench.py [--mode map|light] [--out FILE] [--reps 9] [--warmup 2] [--scene dragon]"""
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
ap.add_argument("--mode", choices=("map", "light"), default="map")
ap.add_argument("--skip-light", action="store_true", help="--mode light: the light-off figures only (for a checkout without PT_OPT_ENV_LIGHT)")
ap.add_argument("--budget-ms", type=float, default=400.0, help="--mode light: device time per equal-time comparison")
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


def sun_map(w, h):
    """a dim sky and a sun of 3 x 3 texels, float32 [h][w][3]: 45 degrees up, 135 degrees from `front` towards `right`"""
    y = np.linspace(0.0, 1.0, h, dtype=np.float32)[:, None, None]
    tex = np.broadcast_to(np.array([0.05, 0.07, 0.1], np.float32) * (0.5 + y), (h, w, 3)).copy()
    r, c = int(h * 0.75), int(w * (0.5 + 135.0 / 360.0))
    tex[r - 1:r + 2, c - 1:c + 2] = (20000.0, 19000.0, 17000.0)
    return tex


def light_mode():
    """(e) - (g) of the module's text"""
    p.flags = g.FLAGS_SMALLPT | g.FLAG_NEE
    t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    tex = sun_map(4096, 2048)
    mom = t.malloc(W * H * 8)
    say(f"--mode light: PT_FLAGS_SMALLPT | PT_FLAG_NEE, 4096 x 2048 bilinear map with a 3 x 3 texel sun; equal time = {a.budget_ms:.0f} ms of device time")
    for light, mis in (((False, False),) if a.skip_light else ((False, False), (True, False), (True, True))):
        t.upload_environment(tex, **({"light": True} if light else {}))
        p.flags = g.FLAGS_SMALLPT | g.FLAG_NEE | (g.FLAG_MIS if mis else 0)
        tag = "on + PT_FLAG_MIS" if mis else "on " if light else "off"
        ms = timed(f"(e) light {tag}: step", lambda: t.launch_kernel(acc.ptr, rgba.ptr, cam, p, a.spp), "paths", W * H * a.spp)
        calls = max(1, int(a.budget_ms / ms))
        q = g.Params.from_buffer_copy(p)
        spent = 0.0
        for k in range(calls):
            q.frame, q.sample_index = k * a.spp, 1 + k * a.spp
            t.launch_kernel(acc.ptr, rgba.ptr, cam, q, a.spp, mom.ptr)
            spent += t.last_kernel_ms()
        rse, fireflies = t.frame_error(mom.ptr, W, H, calls * a.spp, 0.5)
        m1 = mom.download(np.float32, (H, W, 2))[..., 0].astype(np.float64)
        say(f"  (f) light {tag}: {calls} calls = {calls * a.spp} samples per pixel in {spent:.1f} ms: mean relative standard error {rse:.5f}, "
            f"mean luminance of the frame {m1.mean():.4f}, pixels brighter than 0.3 (three times the brightest sky texel: the sun reached them) {int((m1 > 0.3).sum())}, "
            f"firefly pixels (relative standard error above 0.5) {fireflies}")
    if not a.skip_light:
        n = a.eval_rays
        u = np.random.default_rng(7).random((n, 2), dtype=np.float32)
        d_u, d_o, d_r = t.malloc(u.nbytes), t.malloc(16 * n), t.malloc(12 * n)
        d_u.upload(u)
        timed("(g) pt_sample_environment, directions and densities", lambda: t.sample_environment(d_u.ptr, n, d_o.ptr), "draws", n)
        timed("(g) pt_sample_environment, with the radiance", lambda: t.sample_environment(d_u.ptr, n, d_o.ptr, d_r.ptr), "draws", n)
        for b in (d_u, d_o, d_r):
            b.free()
    mom.free()
    t.clear_environment()


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
if a.mode == "light":
    light_mode()
    acc.free()
    rgba.free()
    t.set_option(g.OPT_TIMING, 0)
    t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)
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
