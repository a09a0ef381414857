#!/usr/bin/env python3
"""What adaptive sampling (pt_select_pixels + pt_render_pixels) costs and buys on the bench scene:
cornell_dragon_800k in the sphere room, 1920x1080, depth 4, the default camera, the tree built on the device.  Device times are
PT_OPT_TIMING's (pt_last_kernel_ms, pt_get_stage_ms): the median of --reps calls after --warmup.
  (a) one pass of --pass-spp samples as a function of the share of pixels selected: pt_select_pixels' three launches, the path
      launch and the fold of pt_render_pixels over the list, beside a pt_render_moments call of the same samples over every pixel.
      The lists are pt_select_pixels' own, at the thresholds that select about that share after a first pass over every pixel.
  (b) the mean squared error, against a uniform frame of --ref-spp samples per pixel from other frame numbers, of the adaptive
      result and of a uniform frame with the same total number of samples (rounded up to whole samples per pixel), with the
      device time of both.
Usage: python tools/adaptive_bench.py [--out FILE] [--reps 7] [--warmup 2] [--scene cornell_dragon_800k] [--ref-spp 4096]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--scene", default="cornell_dragon_800k")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--depth", type=int, default=4)
ap.add_argument("--pass-spp", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--thresholds", default="0.1,0.05,0.025", help="(b): the relative standard errors to sample down to")
ap.add_argument("--min-spp", type=int, default=8)
ap.add_argument("--max-spp", type=int, default=256)
a = ap.parse_args()
W, H, K = a.width, a.height, a.pass_spp
N = W * H
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def rse_host(mom, cnt):
    """pt_select_pixels' per-pixel figure (tests/adaptive_ref.py has the same arithmetic), for choosing thresholds only"""
    m1, m2 = mom[:, 0], mom[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(np.maximum(np.float32(0), m2 - m1 * m1) / np.maximum(cnt.astype(np.float32) - 1, 1)) / (m1 + np.float32(0.01))
    return np.where((cnt >= 2) & np.isfinite(r), r, 0).astype(np.float32)


t = g.PathTracer(0)
t.build_bvh(g.scene_mesh(a.scene))
t.upload_spheres(g.reference_spheres())
t.set_option(g.OPT_TIMING, 1)
cam, cm = g.default_camera(W, H), g.camera_model("pinhole", W, H)
p = g.default_params(W, H, depth=a.depth)
p.frame, p.sample_index = 0, 1
acc, rgba = t.alloc_frame(W, H)
mom, cnt, lst = t.malloc(N * 8), t.malloc(N * 4), t.malloc(N * 4)
say(f"adaptive sampling on {a.scene} {W}x{H} depth {a.depth}, sphere room, tree built on the device; passes of {K} samples; "
    f"median of {a.reps} after {a.warmup}")


def params(frame):
    q = g.Params.from_buffer_copy(p)
    q.frame = frame
    return q


def median(fn):
    """fn() -> a tuple of figures; the medians over the repetitions"""
    rows = [fn() for _ in range(a.warmup + a.reps)][a.warmup:]
    return [float(np.median([r[i] for r in rows])) for i in range(len(rows[0]))]


def uniform(buf, first_frame, spp):
    """spp samples per pixel into buf from sample_index 1, in calls of 16 (the bench's step); the device ms of the calls"""
    ms, done = 0.0, 0
    while done < spp:
        n = min(16, spp - done)
        q = params(first_frame + done)
        q.sample_index = done + 1
        t.launch_kernel(buf.ptr, rgba.ptr, cam, q, n)
        ms += t.last_kernel_ms()
        done += n
    return ms


# ---- (a) the cost of a pass by the share of pixels selected
def uniform_pass():
    t.launch_kernel(acc.ptr, rgba.ptr, cam, params(0), K, moments_ptr=mom.ptr)
    return (t.last_kernel_ms(),)


say(f"(a) pt_render_moments, {K} samples over every pixel: {median(uniform_pass)[0]:.3f} ms")
cnt.zero()
t.render_pixels(cam, cm, params(0), acc.ptr, cnt.ptr, mom.ptr, spp=K)
t.sync()
r0 = rse_host(mom.download(np.float32, (N, 2)), cnt.download(np.uint32, (N,)))
mom0, acc0 = mom.download(np.float32, (N, 2)), acc.download(np.float32, (N, 3))
say(f"    {'share asked':>11} {'threshold':>10} {'selected':>9} {'share':>7} | {'select ms':>9} | {'pass ms':>8} = {'path':>8} + {'fold':>7} | {'Msamples/s':>10}")
for share in (1.0, 0.5, 0.25, 0.1, 0.05, 0.01):
    thr = 0.0 if share >= 1.0 else float(np.quantile(r0, 1.0 - share))

    def one_pass():
        # from the same state every time: the moments and counts of the first pass
        mom.upload(mom0)
        acc.upload(acc0)
        cnt.upload(np.full(N, K, np.uint32))
        n, _ = t.select_pixels(mom.ptr, cnt.ptr, lst.ptr, W, H, thr, K if share < 1.0 else 2 * K, 1 << 30)
        sel_ms = t.last_kernel_ms()
        if n == 0:
            return n, sel_ms, 0.0, 0.0, 0.0
        t.render_pixels(cam, cm, params(K), acc.ptr, cnt.ptr, mom.ptr, spp=K, n=n, pixels_ptr=lst.ptr)
        ms, st = t.last_kernel_ms(), t.stage_ms()
        return n, sel_ms, ms, st["frame"], st["fold"]

    n, sel_ms, ms, path_ms, fold_ms = median(one_pass)
    say(f"    {share:11.2f} {thr:10.4g} {int(n):9d} {n / N:7.3f} | {sel_ms:9.3f} | {ms:8.3f} = {path_ms:8.3f} + {fold_ms:7.3f} | {n * K / max(ms, 1e-9) / 1e3:10.1f}")

# ---- (b) error against a converged frame at equal samples
REF_FRAME = 1 << 20
ref = t.malloc(N * 12)
uniform(ref, REF_FRAME, a.ref_spp)
ref_img = ref.download(np.float32, (N, 3)).astype(np.float64)
say(f"(b) mean squared error against a uniform frame of {a.ref_spp} samples per pixel (frames {REF_FRAME} ..); min {a.min_spp}, max {a.max_spp} samples")
say(f"    {'threshold':>9} | {'passes':>6} {'samples/px':>10} {'at max':>7} {'ms':>9} {'of it select':>12} {'MSE':>11} | {'uniform spp':>11} {'ms':>9} {'MSE':>11} | {'MSE ratio':>9}")
for thr in [float(x) for x in a.thresholds.split(",")]:
    cnt.zero()
    total_ms = sel_total = 0.0
    t.render_pixels(cam, cm, params(0), acc.ptr, cnt.ptr, mom.ptr, spp=K)
    total_ms += t.last_kernel_ms()
    passes, samples, k = 1, N * K, 1
    while True:
        n, _ = t.select_pixels(mom.ptr, cnt.ptr, lst.ptr, W, H, thr, a.min_spp, a.max_spp)
        sel_total += t.last_kernel_ms()
        if n == 0:
            break
        t.render_pixels(cam, cm, params(k * K), acc.ptr, cnt.ptr, mom.ptr, spp=K, n=n, pixels_ptr=lst.ptr)
        total_ms += t.last_kernel_ms()
        passes, samples, k = passes + 1, samples + n * K, k + 1
    total_ms += sel_total
    counts = cnt.download(np.uint32, (N,))
    mse_ad = float(np.mean((acc.download(np.float32, (N, 3)).astype(np.float64) - ref_img) ** 2))
    u = -(-samples // N)
    u_ms = uniform(acc, 0, u)
    mse_u = float(np.mean((acc.download(np.float32, (N, 3)).astype(np.float64) - ref_img) ** 2))
    say(f"    {thr:9.4g} | {passes:6d} {samples / N:10.2f} {float(np.mean(counts == a.max_spp)):7.3f} {total_ms:9.2f} {sel_total:12.2f} {mse_ad:11.4e} | "
        f"{u:11d} {u_ms:9.2f} {mse_u:11.4e} | {mse_ad / mse_u:9.3f}")
t.close()
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
