"""The oracle's self-checks (CPU only) on the inputs of tests/test_gpu_scene_matrix.py, which tests/scene_matrix.py defines: the
GPU module compares the kernels with the oracle on these inputs, so the oracle must first be shown to give non-trivial frames
there, to agree with brute force on the coincident triangles and the grid ties, and to be blind to spheres that no ray can
reach."""
import numpy as np

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
from scene_matrix import (PINHOLE_SIDES, POSES, SPHERES_ONLY, duplicated, grid_mesh, grid_rays, make_camera, pinhole_camera,
                          pinhole_params, pose_camera, pose_spheres, red_copies_table, tilted_grid, tilted_grid_table,
                          unreachable_spheres)


# ---------------------------------------------------------------------------------------------------- oracle self-checks
def first_hit_fractions(bvh, sph, cam, W, H, cull=1):
    p = g.default_params(W, H)
    p.cull_backfaces = cull
    ids = R.guides(bvh, sph, cam, p)[3]
    return float((ids >= 0).mean()), float((ids <= -2).mean())


def test_every_pose_gives_a_non_trivial_frame():
    mesh = g.scene_mesh("cornell_dragon")
    bvh = g.Bvh(mesh)
    W, H = 160, 90
    for name in POSES:
        cam, sph = pose_camera(name, W, H), pose_spheres(name)
        tri, sp = first_hit_fractions(bvh, sph, cam, W, H)
        print(f"{name}: triangle first hits {tri:.3f}, sphere first hits {sp:.3f}")
        if name == "away":
            assert tri == 0.0 and sp == 0.0
            continue
        assert tri > 0.05, name
        if sph is not None:
            assert sp > 0.0, name
        p = g.default_params(W, H)
        acc, _, _ = orc.render(bvh, sph, cam, p, 1, want_rgba=False)
        assert np.isfinite(acc).all() and acc.std() > 0, name


def test_oracle_walk_equals_brute_force_on_coincident_triangles():
    mesh = g.scene_mesh("cornell_dragon")
    for reverse in (False, True):
        dup, n0 = duplicated(mesh, reverse)
        bvh = g.Bvh(dup)
        lo, hi = dup.bounds()
        cam = make_camera(320, 180, **POSES["control"][0])
        rays = np.concatenate([orc.random_rays(20000, lo, hi, seed=3), orc.primary_rays(cam, 320, 180, frame=1)])
        for cull in (True, False):
            t0, i0, n0_, _ = orc.trace_bvh(bvh, rays, cull)
            tb, ib, nb = orc.trace_brute(dup, rays, cull)
            assert np.array_equal(t0, tb) and np.array_equal(i0, ib)
            hit = ib >= 0
            assert hit.mean() > 0.2 and np.array_equal(n0_[hit], nb[hit])
            if not reverse:
                assert i0.max() < n0, cull     # the original (the smaller id) wins every exact tie
    # and so the red copies never show: the frame equals the one of the plain mesh under the global material
    dup, n0 = duplicated(mesh)
    W, H = 96, 54
    cam, p = make_camera(W, H, **POSES["control"][0]), g.default_params(W, H)
    tab, ids = red_copies_table(n0, dup.n_tris, p)
    a, _, _ = orc.render(g.Bvh(dup), g.reference_spheres(), cam, p, 2, materials=tab, tri_material=ids)
    bvh0 = g.Bvh(mesh)
    b, _, _ = orc.render(bvh0, g.reference_spheres(), cam, p, 2)
    assert np.array_equal(a, b)


def test_oracle_grid_ties():
    mesh = grid_mesh()
    bvh = g.Bvh(mesh)
    rays = grid_rays()
    for cull in (True, False):
        t0, i0, n0, _ = orc.trace_bvh(bvh, rays, cull)
        tb, ib, nb = orc.trace_brute(mesh, rays, cull)
        assert np.array_equal(t0, tb) and np.array_equal(i0, ib) and np.array_equal(n0, nb)
        assert (ib >= 0).mean() > (0.4 if cull else 0.9)
        assert np.all(t0[ib >= 0] == 4.0)


def test_oracle_tilted_grid_ties_in_frames():
    """every fov-0 frame of the tilted grid: both triangles of the square really meet the ray at the same t, and the frame shows
    the smaller id's colour in every pixel, through the oracle's walk and through brute force alike"""
    mesh, mids = tilted_grid()
    bvh = g.Bvh(mesh)
    tab, tm = tilted_grid_table(mesh.n_tris)
    for side, (below, cull) in PINHOLE_SIDES.items():
        p = pinhole_params(cull)
        for k, (x, y) in enumerate(mids):
            cam = pinhole_camera(x, y, below)
            ray = orc.primary_rays(cam, 2, 2)[:1]
            ts = [orc.trace_brute(g.Mesh.from_arrays(mesh.verts, mesh.tris[[2 * k + q]]), ray, bool(cull))[0][0] for q in (0, 1)]
            assert ts[0] == ts[1] < 1e30, (side, k, ts)
            acc, _, _ = orc.render(bvh, None, cam, p, 1, materials=tab, tri_material=tm)
            col, _, _ = orc.sample_pixels([(0, 0), (1, 1)], None, cam, p, 1, mesh=mesh, materials=tab, tri_material=tm)
            want = np.array(tab[2 * k].emi, np.float32)
            assert (acc == want).all() and (col == want).all(), (side, k)


def test_oracle_is_blind_to_unreachable_spheres():
    bvh = g.Bvh(g.scene_mesh("cornell_dragon"))
    W, H = 64, 48
    cam, p = make_camera(W, H, **POSES["control"][0]), g.default_params(W, H)
    a, ra, _ = orc.render(bvh, g.reference_spheres(), cam, p, 4)
    b, rb, _ = orc.render(bvh, unreachable_spheres(), cam, p, 4)
    assert len(unreachable_spheres()) == 32
    assert np.array_equal(a, b) and np.array_equal(ra, rb)


def test_spheres_only_oracle_frame():
    W, H = 96, 64
    cam, p = make_camera(W, H, **POSES["control"][0]), g.default_params(W, H)
    sph = SPHERES_ONLY()
    acc, _, cnt = orc.render(None, sph, cam, p, 4)
    assert np.isfinite(acc).all() and acc.std() > 0.01 and cnt["rays"] > W * H * 4
