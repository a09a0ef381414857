"""PT_OPT_LAST_OCCLUDERS on the CPU: the selection rule of the occluder list (pt_occluder_ids, restated in numpy from the mesh) and
the predicate behind the direct test — for a last segment whose nearest sphere hit is ts, "a listed triangle is hit at
0 < t < nextafter(ts)" implies "the closest triangle hit of the whole mesh lies at t <= ts", the verdict the any-hit walk writes.
The distances come from the oracle's brute-force loop over one-triangle meshes, as in tests/test_last_anyhit_predicate.py."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc

F32_MAX = np.float32(np.finfo(np.float32).max)
CAP, AREA_DIV = g._abi.OCCLUDERS_MAX, 24.0   # PT_OCCLUDERS_MAX, PT_OCCLUDER_AREA_DIV


def library_ids(verts, tris, cap=CAP):
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32)
    ids = (C.c_int32 * max(cap, 1))()
    n = g._abi.ptmi().pt_occluder_ids(v.ctypes.data, len(v), f.ctypes.data, len(f), ids, cap)
    assert n >= 0, n
    return list(ids[:n])


def areas(verts, tris):
    t = np.asarray(verts, np.float32)[np.asarray(tris)].astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)


def numpy_ids(verts, tris, cap=CAP):
    a = areas(verts, tris)
    total = np.cumsum(a)[-1]   # (summed in id order, as the library sums)
    big = np.nonzero((a * AREA_DIV >= total) & (a > 0))[0]
    order = sorted(big.tolist(), key=lambda i: (-a[i], i))   # largest first, equal areas by the smaller id
    return order[:cap]


@pytest.mark.parametrize("name,expect", [("cornell", 10), ("cornell_dragon", 10), ("gto_sixteen", 0), ("dragon", 0)])
def test_selection_rule(name, expect):
    m = g.scene_mesh(name)
    v, f = np.asarray(m.verts, np.float32), np.asarray(m.tris, np.int32)
    ids = library_ids(v, f)
    assert ids == numpy_ids(v, f) and len(ids) == expect
    a = areas(v, f)
    if ids:
        assert all(a[i] >= a[j] for i, j in zip(ids, ids[1:])), "largest first"
        assert all(i < j for i, j in zip(ids, ids[1:]) if a[i] == a[j]), "equal areas by the smaller id"
        assert any(a[i] == a[j] for i, j in zip(ids, ids[1:])), "the walls are quads: the scene has ties"
        assert a[ids[-1]] * AREA_DIV >= a.sum() > np.delete(a, ids).max() * AREA_DIV, "the threshold"
    for cap in (0, 1, 4):
        assert library_ids(v, f, cap) == ids[:cap]
    # the triangles of the Cornell box are those of the box with the dragon in it: the same ids lead both lists
    if name == "cornell_dragon":
        box = g.scene_mesh("cornell")
        assert ids == library_ids(np.asarray(box.verts, np.float32), np.asarray(box.tris, np.int32))


def test_ties_threshold_and_cap_on_a_hand_built_mesh():
    """28 right triangles in a row (every coordinate exact in binary32): ids 3 and 17 of area 8, eleven of area 4 (ties: one more
    than the list holds), the rest of area 0.25, below the threshold of 63.75 / 24"""
    la, lb = np.full(28, 0.5), np.full(28, 1.0)
    fours = [1, 5, 6, 9, 12, 13, 20, 21, 24, 26, 27]
    la[fours], lb[fours] = 2.0, 4.0
    la[[3, 17]], lb[[3, 17]] = 4.0, 4.0
    x = 16.0 * np.arange(28)
    v = np.stack([np.stack([x, 0 * x, 0 * x], 1), np.stack([x + la, 0 * x, 0 * x], 1), np.stack([x, lb, 0 * x], 1)], 1).astype(np.float32)
    f = np.arange(84, dtype=np.int32).reshape(-1, 3)
    a = areas(v.reshape(-1, 3), f)
    assert a[3] == a[17] == 8.0 and a[1] == a[27] == 4.0 and a.sum() == 63.75 and a[1] * AREA_DIV >= a.sum() > a[0] * AREA_DIV
    want = [3, 17] + fours[:CAP - 2]
    assert library_ids(v.reshape(-1, 3), f) == want == numpy_ids(v.reshape(-1, 3), f)
    assert library_ids(v.reshape(-1, 3), f, 100) == want, "never more than PT_OCCLUDERS_MAX"
    assert library_ids(v.reshape(-1, 3), f, 5) == want[:5]
    # the same triangles under other ids: the two largest lead, then the area-4 triangles with the ten smallest NEW ids
    perm = np.random.default_rng(5).permutation(28)
    got = library_ids(v[perm].reshape(-1, 3), f)
    new_fours = sorted(j for j in range(28) if perm[j] in fours)
    assert got == numpy_ids(v[perm].reshape(-1, 3), f) == sorted(j for j in range(28) if perm[j] in (3, 17)) + new_fours[:CAP - 2]
    # bad arguments are refused
    lib = g._abi.ptmi()
    ids = (C.c_int32 * 4)()
    bad = np.array([[0, 1, 84]], np.int32)
    assert lib.pt_occluder_ids(v.ctypes.data, 84, bad.ctypes.data, 1, ids, 4) < 0
    assert lib.pt_occluder_ids(None, 84, f.ctypes.data, 28, ids, 4) < 0 and lib.pt_occluder_ids(v.ctypes.data, 84, f.ctypes.data, 28, ids, -1) < 0


def sphere_ts(rays, spheres):
    """nearest valid sphere hit per ray (pt_sphere_intersect + the 0.01 rule, float32 steps), F32_MAX when none"""
    o, d = rays[:, 0:3], rays[:, 4:7]
    best = np.full(len(rays), F32_MAX, np.float32)
    for s in spheres:
        c, rad = np.array(s.pos_rad[:3], np.float32), np.float32(s.pos_rad[3])
        op = c - o
        b = np.einsum("ij,ij->i", op, d).astype(np.float32)
        disc = (b * b - np.einsum("ij,ij->i", op, op).astype(np.float32)) + rad * rad
        ok = disc >= 0
        r = np.sqrt(np.where(ok, disc, 0)).astype(np.float32)
        t = np.where(b - r > np.float32(0.01), b - r, np.where(b + r > np.float32(0.01), b + r, np.float32(0)))
        t = np.where(ok, t, np.float32(0)).astype(np.float32)
        best = np.where((t != 0) & (t < best) & (t > np.float32(0.01)), t, best)
    return best


@pytest.mark.parametrize("cull", [True, False])
def test_direct_test_implies_the_anyhit_verdict(cull):
    """2 048 rays per listed triangle of the Cornell box, half of them aimed at it from inside the room"""
    mesh = g.scene_mesh("cornell")
    v, f = np.asarray(mesh.verts, np.float32), np.asarray(mesh.tris, np.int32)
    ids = library_ids(v, f)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(31)
    n_decided = 0
    for k, tri in enumerate(ids):
        rays = orc.random_rays(2048, lo, hi, seed=100 + k)
        w = rng.dirichlet((1.0, 1.0, 1.0), 1024).astype(np.float32)
        aim = w @ v[f[tri]] - rays[::2, 0:3]
        rays[::2, 4:7] = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(np.float32)
        t_min, tri_min, _ = orc.trace_brute(mesh, rays, cull)
        hit = tri_min >= 0
        t_k, tri_k, _ = orc.trace_brute(g.Mesh.from_arrays(v, f[tri:tri + 1]), rays, cull)
        t_k = np.where(tri_k >= 0, t_k, np.inf).astype(np.float32)
        assert np.all(t_k[hit] >= t_min[hit]) and not np.any(np.isfinite(t_k) & ~hit)
        mine = np.isfinite(t_k)
        ts_room = sphere_ts(rays, g.reference_spheres())
        down = np.nextafter(t_k, np.float32(0)).astype(np.float32)
        bounds = {"room": ts_room, "none": np.full(len(rays), F32_MAX, np.float32),
                  "t == ts": np.where(mine, t_k, ts_room).astype(np.float32),               # the tie: the triangle stands
                  "ts one bit below t": np.where(mine, down, ts_room).astype(np.float32)}   # the sphere wins over THIS triangle
        for what, ts in bounds.items():
            start = np.where(ts < F32_MAX, np.nextafter(np.minimum(ts, np.float32(1e38)), np.float32(np.inf)), ts).astype(np.float32)
            direct = (t_k > 0) & (t_k < start)                 # wf_occluded's acceptance on this record
            verdict = hit & ~(ts < t_min)                      # what the closest-hit rule, and so the any-hit walk, decides
            assert np.all(verdict[direct]), (tri, what)
            if what in ("none", "t == ts"):
                assert np.array_equal(direct, mine), (tri, what)
            if what == "ts one bit below t":
                assert not direct.any(), (tri, what)
            n_decided += int(direct.sum()) if what == "room" else 0
        assert mine.sum() > 256, tri
    assert n_decided > 1000
