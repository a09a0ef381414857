#!/usr/bin/env python3
"""pt_refit_bvh measured: device time of a refit (PT_OPT_TIMING) and wall time of a tree's first, synchronising refit on
three scene sizes; the bench step (1920x1080, depth 4, 16 spp, sphere room, the bench's tree: host SAH + PT_OPT_OPTIMIZE 4 +
PT_OPT_REBUILD 2) at rest and after 30 refits that turn each dragon copy of cornell_dragon_800k a few degrees per frame;
against that, pt_build_bvh of the final positions with and without PT_OPT_OPTIMIZE (build time + step time).
Usage: python tools/refit_bench.py [--out FILE] [--big cornell_dragon_6400k] [--frames 30] [--steps 8]"""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import gpu_pathtracer_amd as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report here")
ap.add_argument("--big", default="cornell_dragon_6400k", help="the large scene (device-built tree; '' = skip)")
ap.add_argument("--frames", type=int, default=30)
ap.add_argument("--deg", type=float, default=3.0, help="degrees each dragon copy turns per frame")
ap.add_argument("--steps", type=int, default=8, help="timed bench steps per measurement")
a = ap.parse_args()
W, H, SPP, DEPTH, PASSES = 1920, 1080, 16, 4, 4
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench_tree(pt, mesh):
    pt.set_option(g.OPT_OPTIMIZE, PASSES)
    pt.set_option(g.OPT_REBUILD, 2)
    t0 = time.perf_counter()
    pt.upload_bvh(g.Bvh(mesh, split_alpha=-1.0))
    pt.sync()
    pt.set_option(g.OPT_OPTIMIZE, 0)
    pt.set_option(g.OPT_REBUILD, 0)
    return time.perf_counter() - t0


def refit_ms(pt, buf, n, reps=5):
    """(wall ms of the first call incl. sync, best device ms of `reps` timed refits)"""
    pt.set_option(g.OPT_TIMING, 1)
    t0 = time.perf_counter()
    pt.refit_bvh(buf, n)
    pt.sync()
    first = 1e3 * (time.perf_counter() - t0)
    dev = []
    for _ in range(reps):
        pt.refit_bvh(buf, n)
        dev.append(pt.last_kernel_ms())
    pt.set_option(g.OPT_TIMING, 0)
    return first, min(dev), float(np.median(dev))


def step_ms(pt, acc, rgba, cam, p, steps):
    for i in range(2):   # warm-up (PT_KERNEL_AUTO trials, buffers)
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = i * SPP, 1 + i * SPP
        pt.launch_kernel(acc.ptr, rgba.ptr, cam, q, SPP)
    for i in range(4):
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = (2 + i) * SPP, 1 + (2 + i) * SPP
        pt.launch_kernel(acc.ptr, rgba.ptr, cam, q, SPP)
    pt.sync()
    t0 = time.perf_counter()
    for i in range(steps):
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = (10 + i) * SPP, 1 + (10 + i) * SPP
        pt.launch_kernel(acc.ptr, rgba.ptr, cam, q, SPP)
    pt.sync()
    return 1e3 * (time.perf_counter() - t0) / steps


def turned(soup, copies, deg):
    """every copy (a row range) turned by `deg` about the vertical axis through its own centre"""
    out = soup.copy()
    a_ = np.radians(deg)
    R = np.array([[np.cos(a_), 0, np.sin(a_)], [0, 1, 0], [-np.sin(a_), 0, np.cos(a_)]])
    for lo, hi in copies:
        v = soup[lo:hi].reshape(-1, 3).astype(np.float64)
        c = 0.5 * (v.min(0) + v.max(0))
        out[lo:hi] = ((v - c) @ R.T + c).astype(np.float32).reshape(-1, 9)
    return out


def soup_mesh(soup):
    return g.Mesh.from_arrays(soup.reshape(-1, 3), np.arange(3 * len(soup), dtype=np.int32).reshape(-1, 3))


say(f"pt_refit_bvh, {time.strftime('%Y-%m-%d')}; device ms = PT_OPT_TIMING (best / median of 5), first = wall ms of a tree's first refit "
    "(reads the tree back, uploads the schedule)")
cam = g.default_camera(W, H)
p = g.default_params(W, H, depth=DEPTH)
p.flags = g.FLAG_WRITE_RGBA
sph = g.reference_spheres()

# ---- refit cost on three sizes
for name in ("cornell_dragon", "cornell_dragon_800k", a.big):
    if not name:
        continue
    mesh = g.scene_mesh(name)
    soup = mesh.triangle_soup()
    pt = g.PathTracer(0)
    try:
        if name == a.big:
            pt.build_bvh(mesh)
            tree = "device-built tree (PLOC)"
        else:
            up = bench_tree(pt, mesh)
            tree = f"bench tree (host SAH + OPTIMIZE {PASSES} + REBUILD 2, upload {up:.1f} s)"
        info = pt.scene_info()
        buf = pt.malloc(soup.nbytes)
        buf.upload(soup)
        first, best, med = refit_ms(pt, buf, len(soup))
        say(f"{name}: {mesh.n_tris} tris, {tree}: {info['n_inner']} binary nodes, {info['n_tri_refs']} records, depth {info['max_depth']}; "
            f"refit device {best:.3f} ms (median {med:.3f}), first refit {first:.1f} ms wall")
        buf.free()
    finally:
        pt.close()

# ---- the bench scene in motion
mesh = g.scene_mesh("cornell_dragon_800k")
soup = mesh.triangle_soup()
n_box, n_dragon = g.Mesh.asset("cornell").n_tris, g.Mesh.asset("dragon").n_tris
copies = [(n_box + k * n_dragon, n_box + (k + 1) * n_dragon) for k in range(8)]
assert copies[-1][1] == len(soup)
pt = g.PathTracer(0)
try:
    bench_tree(pt, mesh)
    pt.upload_spheres(sph)
    acc, rgba = pt.alloc_frame(W, H)
    rest = step_ms(pt, acc, rgba, cam, p, a.steps)
    cost_rest = pt.tree_cost()
    buf = pt.malloc(soup.nbytes)
    dev = []
    final = soup
    for f in range(1, a.frames + 1):
        final = turned(soup, copies, a.deg * f)
        buf.upload(final)
        pt.set_option(g.OPT_TIMING, 1)
        pt.refit_bvh(buf, len(soup))
        dev.append(pt.last_kernel_ms())
        pt.set_option(g.OPT_TIMING, 0)
    moved = step_ms(pt, acc, rgba, cam, p, a.steps)
    cost_moved = pt.tree_cost()
    say(f"cornell_dragon_800k bench step ({W}x{H}, depth {DEPTH}, {SPP} spp, sphere room, bench tree): at rest {rest:.2f} ms, "
        f"after {a.frames} refits ({a.deg:g} deg per frame per dragon copy, {a.deg * a.frames:g} deg in all) {moved:.2f} ms; "
        f"refit device ms over the frames: median {np.median(dev):.3f}, max {max(dev):.3f}; "
        f"tree cost (node visits, tri tests) {cost_rest[0]:.2f}/{cost_rest[1]:.2f} -> {cost_moved[0]:.2f}/{cost_moved[1]:.2f}")
    buf.free()
    acc.free()
    rgba.free()
finally:
    pt.close()

# ---- against building the final positions again
fm = soup_mesh(final)
for passes in (0, PASSES):
    pt = g.PathTracer(0)
    try:
        pt.upload_spheres(sph)
        pt.set_option(g.OPT_OPTIMIZE, passes)
        t0 = time.perf_counter()
        build_dev = pt.build_bvh(fm)
        wall = 1e3 * (time.perf_counter() - t0)
        pt.set_option(g.OPT_OPTIMIZE, 0)
        acc, rgba = pt.alloc_frame(W, H)
        st = step_ms(pt, acc, rgba, cam, p, a.steps)
        c = pt.tree_cost()
        say(f"pt_build_bvh of the final positions, OPTIMIZE {passes}: device build {build_dev:.2f} ms, call {wall:.0f} ms wall "
            f"(host copy{' + host optimisation' if passes else ''}), step {st:.2f} ms, tree cost {c[0]:.2f}/{c[1]:.2f}")
        acc.free()
        rgba.free()
    finally:
        pt.close()

if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
