#!/usr/bin/env python3
"""pt_temporal measured: device time (PT_OPT_TIMING, pt_last_kernel_ms) at 1920x1080 on the bench scene (cornell_dragon + the
sphere room, golden camera), the camera panning 1 degree between frames, the median of repeated timed calls — with and without
ids, the first frame's copy path, and beside them the guide pass and pt_denoise at 4 iterations from the same run.
--motion measures pt_temporal_motion instead: the dragon of the bench scene turned and moved between the two frames
(tests/gpu_support.cornell_dragon_moved, applied with pt_refit_bvh), the camera still; pt_temporal_motion with and without its
motion buffer and pt_temporal on the same guides, the three alternating call by call in one process.
--variance measures pt_denoise_variance beside pt_denoise (the same iterations on the same 1080p frame: 4 spp of the bench scene
with its moments) and pt_temporal_moments beside pt_temporal (the camera panned between the frames), each pair alternating call by
call in one process.
Usage: python tools/temporal_bench.py [--out FILE] [--reps 20] [--motion [--turn-deg 3]] [--variance]"""
import argparse
import math
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
ap.add_argument("--pan-deg", type=float, default=1.0)
ap.add_argument("--motion", action="store_true", help="measure pt_temporal_motion on a moved dragon")
ap.add_argument("--variance", action="store_true", help="measure pt_denoise_variance and pt_temporal_moments beside their colour calls")
ap.add_argument("--turn-deg", type=float, default=3.0, help="--motion: the dragon's turn between the two frames")
a = ap.parse_args()
W, H = 1920, 1080
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def panned(cam, deg):
    """front and right turned by deg about up = (0, 1, 0) of the default camera."""
    c = g.Camera.from_buffer_copy(cam)
    th = math.radians(deg)
    for name in ("front", "right"):
        x, y, z = getattr(cam, name)
        getattr(c, name)[:] = (x * math.cos(th) + z * math.sin(th), y, -x * math.sin(th) + z * math.cos(th))
    return c


def motion_bench():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_support import cornell_dragon_moved
    mesh, rest, moved = cornell_dragon_moved(deg=a.turn_deg, shift=(0.3, 0.0, -0.2))
    n = len(rest)
    t = g.PathTracer(0)
    t.upload_bvh(g.Bvh(mesh))
    t.upload_spheres(g.reference_spheres())
    cam = g.default_camera(W, H)
    cam.dist = 18.0 * H / 1080.0
    p = g.default_params(W, H)
    p.flags = g.FLAG_WRITE_RGBA
    acc, rgba = t.alloc_frame(W, H)
    orgba, mo = t.malloc(W * H * 4), t.malloc(W * H * 8)
    verts = [t.malloc(rest.nbytes) for _ in range(2)]
    verts[0].upload(rest)
    verts[1].upload(moved)
    th = g.TemporalHistory(t, W, H)
    p.frame, p.sample_index = 0, 1
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 4)
    th.push(cam, p, acc.ptr)                      # the rest pose becomes the history
    t.refit_bvh(verts[1], n)
    p.frame = 4
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 4)
    prev, cur = 1 - th.cur, th.cur
    alb, nrm, pos, ids = th._ptrs(cur)
    _, pn, pp, pi = th._ptrs(prev)
    t.render_aux(cam, p, alb, nrm, pos, ids)      # the guides of the moved pose
    t.sync()

    def motion(with_motion):
        t.temporal_motion(W, H, cam, verts[0], verts[1], n, th.color[prev].ptr, th.length[prev].ptr, pn, pp, pi, acc.ptr, nrm, pos, ids,
                          th.color[cur].ptr, th.length[cur].ptr, orgba.ptr, mo.ptr if with_motion else None)

    def static():
        t.temporal(W, H, cam, th.color[prev].ptr, th.length[prev].ptr, pn, pp, pi, acc.ptr, nrm, pos, ids, th.color[cur].ptr, th.length[cur].ptr,
                   orgba.ptr)

    calls = (("pt_temporal_motion, motion buffer   ", lambda: motion(True)), ("pt_temporal_motion, no motion buffer", lambda: motion(False)),
             ("pt_temporal, ids (same guides)      ", static))
    t.set_option(g.OPT_TIMING, 1)
    ms = {name: [] for name, _ in calls}
    for _ in range(a.reps + 2):                   # alternating: every call sees the same clocks and caches as its neighbours
        for name, fn in calls:
            fn()
            ms[name].append(t.last_kernel_ms())
    say(f"{a.scene}-moved ({n} triangles, the dragon turned {a.turn_deg} deg and shifted) + 8 spheres, {W}x{H}, camera still; device ms "
        f"(PT_OPT_TIMING), median / min of {a.reps} calls, alternating")
    for name, _ in calls:
        say(f"{name}  {float(np.median(ms[name][2:])):7.3f} / {float(np.min(ms[name][2:])):7.3f} ms")
    t.set_option(g.OPT_TIMING, 0)
    id_cur = th.guides[cur][3].download(np.int32, (H, W))
    dragon = id_cur >= g.Mesh.asset("cornell").n_tris
    for name, fn in calls[1:]:
        fn()
        t.sync()
        length = th.length[cur].download(np.float32, (H, W))
        say(f"  {name.strip()}: history accepted at {(length > 1).mean() * 100:.1f} % of the pixels, {(length > 1)[dragon].mean() * 100:.1f} % of the "
            f"dragon's ({dragon.mean() * 100:.1f} % of the frame)")
    for b in [acc, rgba, orgba, mo] + verts:
        b.free()
    th.free()
    t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def variance_bench():
    t = g.PathTracer(0)
    mesh = g.scene_mesh(a.scene)
    t.upload_bvh(g.Bvh(mesh))
    t.upload_spheres(g.reference_spheres())
    cam0 = g.default_camera(W, H)
    cam0.dist = 18.0 * H / 1080.0
    cam1 = panned(cam0, a.pan_deg)
    p = g.default_params(W, H)
    p.flags = g.FLAG_WRITE_RGBA
    acc, rgba = t.alloc_frame(W, H)
    mom = t.malloc(W * H * 8)
    out, var, orgba, omom = t.malloc(W * H * 12), t.malloc(W * H * 4), t.malloc(W * H * 4), t.malloc(W * H * 8)
    th = g.TemporalHistory(t, W, H, with_moments=True)
    p.frame, p.sample_index = 0, 1
    t.launch_kernel(acc.ptr, rgba.ptr, cam0, p, 4, moments_ptr=mom.ptr)
    th.push(cam0, p, acc.ptr, moments_ptr=mom.ptr)          # frame 0 at cam0 becomes the history
    p.frame = 4
    t.launch_kernel(acc.ptr, rgba.ptr, cam1, p, 4, moments_ptr=mom.ptr)
    prev, cur = 1 - th.cur, th.cur
    alb, nrm, pos, ids = th._ptrs(cur)
    _, pn, pp, pi = th._ptrs(prev)
    t.render_aux(cam1, p, alb, nrm, pos, ids)
    t.sync()
    dflt = {k: v for k, v in g.DENOISE_DEFAULTS.items() if k != "iterations"}
    vdflt = {k: v for k, v in g.DENOISE_VARIANCE_DEFAULTS.items() if k != "iterations"}

    def alternate(calls):
        ms = {name: [] for name, _ in calls}
        for _ in range(a.reps + 2):                   # alternating: every call sees the same clocks and caches as its neighbours
            for name, fn in calls:
                fn()
                ms[name].append(t.last_kernel_ms())
        return {name: (float(np.median(v[2:])), float(np.min(v[2:]))) for name, v in ms.items()}

    t.set_option(g.OPT_TIMING, 1)
    say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}, 4 spp with moments, pan {a.pan_deg} deg between the frames; device ms "
        f"(PT_OPT_TIMING), median / min of {a.reps} calls, each pair alternating")
    for it in (1, 4, 5):
        r = alternate((("dn", lambda: t.denoise(acc.ptr, alb, nrm, pos, W, H, out.ptr, orgba.ptr, iterations=it, **dflt)),
                       ("dv", lambda: t.denoise_variance(acc.ptr, mom.ptr, None, alb, nrm, pos, W, H, out.ptr, var.ptr, orgba.ptr,
                                                         samples_per_frame=4, iterations=it, **vdflt))))
        say(f"{it} iteration{'s' if it > 1 else ' '}: pt_denoise {r['dn'][0]:7.3f} / {r['dn'][1]:7.3f} ms   pt_denoise_variance {r['dv'][0]:7.3f} / "
            f"{r['dv'][1]:7.3f} ms   ratio of the medians {r['dv'][0] / r['dn'][0]:.3f}")
    r = alternate((("tc", lambda: t.temporal(W, H, cam0, th.color[prev].ptr, th.length[prev].ptr, pn, pp, pi, acc.ptr, nrm, pos, ids,
                                             th.color[cur].ptr, th.length[cur].ptr, orgba.ptr)),
                   ("tm", lambda: t.temporal_moments(W, H, cam0, None, None, 0, th.moment[prev].ptr, th.length[prev].ptr, pn, pp, pi, mom.ptr, nrm, pos,
                                                     ids, omom.ptr))))
    say(f"pt_temporal, ids, display words {r['tc'][0]:7.3f} / {r['tc'][1]:7.3f} ms   pt_temporal_moments, ids {r['tm'][0]:7.3f} / {r['tm'][1]:7.3f} ms   "
        f"ratio of the medians {r['tm'][0] / r['tc'][0]:.3f}")
    t.set_option(g.OPT_TIMING, 0)
    for b in (acc, rgba, mom, out, var, orgba, omom):
        b.free()
    th.free()
    t.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if a.motion:
    motion_bench()
    sys.exit(0)
if a.variance:
    variance_bench()
    sys.exit(0)

t = g.PathTracer(0)
mesh = g.scene_mesh(a.scene)
t.upload_bvh(g.Bvh(mesh))
t.upload_spheres(g.reference_spheres())
cam0 = g.default_camera(W, H)
cam0.dist = 18.0 * H / 1080.0
cam1 = panned(cam0, a.pan_deg)
p = g.default_params(W, H)
p.flags = g.FLAG_WRITE_RGBA
acc, rgba = t.alloc_frame(W, H)
out, orgba = t.malloc(W * H * 12), t.malloc(W * H * 4)
th = g.TemporalHistory(t, W, H)
# frame 0 at cam0 becomes the history, frame 1 at cam1 is the current frame
p.frame, p.sample_index = 0, 1
t.launch_kernel(acc.ptr, rgba.ptr, cam0, p, 4)
th.push(cam0, p, acc.ptr)
p.frame = 4
t.launch_kernel(acc.ptr, rgba.ptr, cam1, p, 4)
prev, cur = 1 - th.cur, th.cur
alb, nrm, pos, ids = th._ptrs(cur)
_, pn, pp, pi = th._ptrs(prev)
t.sync()


def timed(fn):
    ms = []
    for _ in range(a.reps + 2):
        fn()
        ms.append(t.last_kernel_ms())
    return float(np.median(ms[2:])), float(np.min(ms[2:]))


t.set_option(g.OPT_TIMING, 1)
say(f"{a.scene} ({mesh.n_tris} triangles) + 8 spheres, {W}x{H}, pan {a.pan_deg} deg between the frames; device ms (PT_OPT_TIMING), "
    f"median / min of {a.reps} calls")
med, mn = timed(lambda: t.render_aux(cam1, p, alb, nrm, pos, ids))
say(f"pt_render_aux                        {med:7.3f} / {mn:7.3f} ms")


def temporal(with_ids, history=True, with_rgba=True):
    t.temporal(W, H, cam0 if history else None, th.color[prev].ptr if history else None, th.length[prev].ptr, pn, pp, pi if with_ids else None,
               acc.ptr, nrm, pos, ids if with_ids else None, th.color[cur].ptr, th.length[cur].ptr, orgba.ptr if with_rgba else None)


for name, fn in (("pt_temporal, ids, display words    ", lambda: temporal(True)),
                 ("pt_temporal, no ids, display words ", lambda: temporal(False)),
                 ("pt_temporal, ids, no display words ", lambda: temporal(True, with_rgba=False)),
                 ("pt_temporal, no history (the copy) ", lambda: temporal(True, history=False))):
    med, mn = timed(fn)
    say(f"{name}  {med:7.3f} / {mn:7.3f} ms")
temporal(True)
t.sync()
length = th.length[cur].download(np.float32, (H, W))
say(f"  history accepted at {(length > 1).mean() * 100:.1f} % of the pixels")
dflt = {k: v for k, v in g.DENOISE_DEFAULTS.items() if k != "iterations"}
for it in (1, 4):
    med, mn = timed(lambda: t.denoise(th.color[cur].ptr, alb, nrm, pos, W, H, out.ptr, orgba.ptr, iterations=it, **dflt))
    say(f"pt_denoise of the history, {it} iteration{'s' if it > 1 else ' '}  {med:7.3f} / {mn:7.3f} ms")
t.set_option(g.OPT_TIMING, 0)
for b in (acc, rgba, out, orgba):
    b.free()
th.free()
t.close()
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
