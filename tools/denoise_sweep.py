#!/usr/bin/env python3
"""The sweep behind pt_denoise's defaults, on the CPU: the oracle renders cornell_box (its material table,
lit by the ceiling quad, black background) at a few small sizes with 4 samples per pixel and with 1024, the reference filter
(tests/denoise_ref.py) runs every setting of the grid on the 4-sample image and gains = MSE(noisy) / MSE(filtered), both
against the 1024-sample image.  Prints the best settings by the geometric mean of the gains over the sizes.
Usage: python tools/denoise_sweep.py [--sizes 80x60,128x96,160x120] [--spp 4] [--ref-spp 1024] [--out FILE]"""
import argparse
import itertools
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import orc  # noqa: E402
import denoise_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="80x60,128x96,160x120")
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--ref-spp", type=int, default=1024)
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ITER = [1, 2, 3, 4, 5, 6]
SC = [0.25, 0.5, 1.0, 2.0, 4.0, 0.0]
SN = [0.1, 0.25, 0.5, 1.0, 0.0]
SX = [0.01, 0.03, 0.1, 0.3, 0.0]
grid = list(itertools.product(ITER, SC, SN, SX))
sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
gains = np.zeros((len(sizes), len(grid)))
for k, (W, H) in enumerate(sizes):
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    ref, _, _ = orc.render(bvh, None, cam, p, a.ref_spp, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)
    p.frame = 1 << 20   # frames the reference did not use
    noisy, _, _ = orc.render(bvh, None, cam, p, a.spp, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)
    alb, nrm, pos, _, _, _ = R.guides(bvh, None, cam, p, mesh.materials, mesh.tri_material)
    m0 = R.mse(noisy, ref)
    say(f"{W}x{H}: MSE of the {a.spp}-spp image vs {a.ref_spp} spp {m0:.3e}")
    for j, (it, sc, sn, sx) in enumerate(grid):
        gains[k, j] = m0 / R.mse(R.atrous(noisy, alb, nrm, pos, it, sc, sn, sx), ref)
score = np.exp(np.mean(np.log(gains), axis=0))
order = np.argsort(-score)
say("gain = MSE(noisy) / MSE(filtered); sigma 0 = term off")
say("iterations sigma_c sigma_n sigma_x | gain per size | geometric mean")
for j in order[:15]:
    it, sc, sn, sx = grid[j]
    say(f"{it:10d} {sc:7.2f} {sn:7.2f} {sx:7.2f} | " + " ".join(f"{g_:6.2f}" for g_ in gains[:, j]) + f" | {score[j]:6.2f}")
for name, pick in (("best per iteration count", lambda it: [j for j in order if grid[j][0] == it][0]),):
    say(name + ":")
    for it in ITER:
        j = pick(it)
        say(f"  {it}: sigma {grid[j][1]:.2f} {grid[j][2]:.2f} {grid[j][3]:.2f}  gains " + " ".join(f"{g_:6.2f}" for g_ in gains[:, j]))
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
