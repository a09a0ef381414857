"""PT_OPT_LAST_OCCLUDERS: the shade launch that makes a path's last segment tests it against the mesh's largest triangles (the tree's
occluder list, pt_occluder_ids) before it is queued for the any-hit walk; a ray one of them occludes gets that walk's verdict and
stays out of the queue (1, default; 2 = instrumented launches too; 0 = off).  The test is the walk's on the walk's records, so the
accumulator and the display words must be the same bit for bit under every value; a mesh without such triangles and every call the
any-hit launch does not run for must run the launches they ran before (wave stat "occluded" counts the rays decided); and where
the list is used, the rays it decides are exactly the ones missing from the any-hit launch ("act_shade")."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import COUNTERS, bvh_of, dark_table, golden_camera, judge, pipeline_render, same, soup_mesh

pytestmark = pytest.mark.gpu

OCCL = g._abi.OPT_LAST_OCCLUDERS
# the counters that do not depend on how the waves shared the queue: the work, the any-hit launch's rays, the rays kept out
STABLE = COUNTERS + ("act_shade", "walk_free", "occluded")
# what lets the value 2 reach an instrumented launch: the any-hit launch and the classification run there too
INSTRUMENTED = ((g.OPT_LAST_ANYHIT, 2), (g.OPT_ROOT_CULL, 2), (g._abi.OPT_ROOT_ENTRY, 2), (g._abi.OPT_PATH_HISTORY, 2))


def render(v, *args, options=(), **kw):
    return pipeline_render(((OCCL, v),) + tuple(options), *args, **kw)


def counted(v, *args, options=(), **kw):
    return render(v, *args, options=INSTRUMENTED + tuple(options), counters=True, **kw)


def stable(k):
    return {name: k[name] for name in STABLE}


def test_option_number_and_values():
    assert OCCL == 36
    t = g.PathTracer(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.PtError):
                t.set_option(OCCL, bad)
        for ok in (0, 2, 1):
            t.set_option(OCCL, ok)
    finally:
        t.close()


# (W, H, spp, depth, cull_backfaces, triangle material, tile-split parts); depth 2: the fused packet launch classifies
CASES = {
    "257x131-spp16-d4": (257, 131, 16, 4, 1, g.MAT_DIFF, 1),
    "257x131-spp4-d2-nocull-metal": (257, 131, 4, 2, 0, g.MAT_METAL, 1),
    "257x131-spp1-d2": (257, 131, 1, 2, 1, g.MAT_DIFF, 1),
    "64x64-spp1-d4-metal-3parts": (64, 64, 1, 4, 1, g.MAT_METAL, 3),
    "64x64-spp16-d2-3parts": (64, 64, 16, 2, 1, g.MAT_DIFF, 3),
    "64x64-spp4-d4-nocull": (64, 64, 4, 4, 0, g.MAT_DIFF, 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_frames_and_counters(case):
    W, H, spp, depth, cull, mat, parts = CASES[case]
    kw = dict(depth=depth, cull=cull, tri_mat=mat, parts=parts)
    a, b, c = (render(v, "cornell_dragon", W, H, spp, **kw) for v in (0, 1, 2))
    same(b, a, f"{case}: 1")
    same(c, a, f"{case}: 2")
    c0, c1, c2 = (counted(v, "cornell_dragon", W, H, spp, **kw) for v in (0, 1, 2))
    same(c0, a, f"{case}: instrumented, 0")
    same(c1, a, f"{case}: instrumented, 1")
    same(c2, a, f"{case}: instrumented, 2")
    k0, k1, k2 = c0[2], c1[2], c2[2]
    assert stable(k1) == stable(k0), f"{case}: the value 1 changes an instrumented launch"
    print(f"{case}: last-segment walkers {k0['act_shade']}, decided by the list {k2['occluded']}, walked {k2['act_shade']}; "
          f"items {k0['inner'] + k0['tris']} -> {k2['inner'] + k2['tris']}")
    assert k0["occluded"] == 0 and k2["occluded"] > 0
    assert k2["occluded"] + k2["act_shade"] == k0["act_shade"]
    for k in ("rays", "hits", "paths", "walk_free"):
        assert k2[k] == k0[k], k
    for k in ("inner", "tris", "leaves"):
        assert k2[k] < k0[k], k


@pytest.mark.parametrize("scene", ["gto_sixteen", "dragon"])
def test_mesh_without_large_triangles_has_no_list(scene):
    a, b = (render(v, scene, 257, 131, 4) for v in (0, 1))
    same(b, a, scene)
    c0, c2 = (counted(v, scene, 257, 131, 4) for v in (0, 2))
    same(c2, a, f"{scene}, instrumented")
    assert stable(c2[2]) == stable(c0[2]) and c2[2]["occluded"] == 0 and c2[2]["act_shade"] > 0


@pytest.mark.parametrize("depth", [2, 4])
def test_cornell_without_spheres(depth):
    """no bound: ts = PT_F32_MAX, and an occluder at any distance answers the query"""
    a, b, c = (render(v, "cornell", 257, 131, 4, depth=depth, spheres=False) for v in (0, 1, 2))
    same(b, a, f"open scene, depth {depth}: 1")
    same(c, a, f"open scene, depth {depth}: 2")
    c0, c2 = (counted(v, "cornell", 257, 131, 4, depth=depth, spheres=False) for v in (0, 2))
    same(c2, a, f"open scene, depth {depth}, instrumented")
    assert c2[2]["occluded"] > 0 and c2[2]["occluded"] + c2[2]["act_shade"] == c0[2]["act_shade"]


def two_quads():
    """two large quads in front of the sphere room's back wall, facing each other: all four triangles hold a quarter of the area"""
    def quad(z, lo, hi, flip):
        p = [(lo[0], lo[1], z), (hi[0], lo[1], z), (hi[0], hi[1], z), (lo[0], hi[1], z)]
        t = [p[0], p[1], p[2], p[0], p[2], p[3]]
        return t[::-1] if flip else t
    soup = np.array(quad(-40.0, (-12.0, -9.0), (4.0, 9.0), False) + quad(-22.0, (-4.0, -9.0), (12.0, 9.0), True), np.float32)
    return soup_mesh(soup.reshape(-1, 9))


@pytest.mark.parametrize("cull", [0, 1])
def test_two_quads_every_occluded_ray_is_decided_by_the_list(cull):
    """The whole mesh is its own occluder list (ids 0-3), so the occlusion of every last segment is known without a walk: the list
    decides exactly the last segments that hit a triangle, which is the `hits` a depth-2 call counts beyond the same call at depth 1
    (the same bounce-0 rays), and the any-hit walk that follows finds nothing: both calls report the same triangle hits as option 0."""
    mesh = two_quads()
    v, f = np.ascontiguousarray(mesh.verts, np.float32), np.ascontiguousarray(mesh.tris, np.int32)
    ids = (g._abi.C.c_int32 * 12)()
    assert g._abi.ptmi().pt_occluder_ids(v.ctypes.data, len(v), f.ctypes.data, len(f), ids, 12) == 4 and sorted(ids[:4]) == [0, 1, 2, 3]
    bvh = g.Bvh(mesh)
    install = lambda t: t.upload_bvh(bvh)
    W, H, spp = 128, 96, 4
    a, b = (render(x, install, W, H, spp, depth=2, cull=cull) for x in (0, 1))
    same(b, a, f"two quads, cull {cull}")
    d1 = counted(0, install, W, H, spp, depth=1, cull=cull)[2]
    c0, c2 = (counted(x, install, W, H, spp, depth=2, cull=cull) for x in (0, 2))
    same(c2, a, f"two quads, cull {cull}, instrumented")
    last_hits = c0[2]["hits"] - d1["hits"]
    print(f"two quads, cull {cull}: {last_hits} last segments end on a triangle, the list decided {c2[2]['occluded']}")
    assert last_hits > 0 and c2[2]["occluded"] == last_hits and c2[2]["hits"] == c0[2]["hits"]


def nine_spheres(v, counters):
    """the reference room and a ninth sphere: more than the kernel-argument block holds, so no sphere bound and no any-hit launch"""
    t = g.PathTracer(0)
    try:
        for o, x in ((g.OPT_KERNEL, g.KERNEL_WAVEFRONT), (OCCL, v)) + (INSTRUMENTED + ((g.OPT_COUNTERS, 1),) if counters else ()):
            t.set_option(o, x)
        t.upload_bvh(bvh_of("cornell_dragon")[1])
        sph = list(g.reference_spheres())
        extra = g.Sphere()
        extra.pos_rad[:] = (-9.0, -11.0, -30.0, 3.0)
        extra.col[:] = (0.8, 0.8, 0.8)
        extra.mat = g.MAT_DIFF
        t.upload_spheres((g.Sphere * 9)(*(sph + [extra])))
        W, H = 257, 131
        acc, rgba = t.alloc_frame(W, H)
        p = g.default_params(W, H)
        p.flags, p.frame, p.sample_index = g.FLAG_WRITE_RGBA, 7, 1
        t.launch_kernel(acc.ptr, rgba.ptr, golden_camera(W, H), p, 4)
        t.sync()
        out = (acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W)))
        if counters:
            out += ({**t.counters(), **t.wave_stats()},)
        acc.free()
        rgba.free()
        return out
    finally:
        t.close()


FALLBACKS = {
    "nee": dict(flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF),
    "material-table": dict(table=dark_table),
    "emitting-triangles": dict(tri_emi=(0.0, 0.25, 0.0)),
    "depth-1": dict(depth=1),
    "last-anyhit-0": dict(options=((g.OPT_LAST_ANYHIT, 0),)),
    "root-cull-0": dict(options=((g.OPT_ROOT_CULL, 0),)),
}


@pytest.mark.parametrize("case", list(FALLBACKS) + ["nine-spheres"])
def test_fallbacks_run_the_launches_they_ran(case):
    if case == "nine-spheres":
        a, b = (nine_spheres(v, False) for v in (0, 1))
        c0, c2 = (nine_spheres(v, True) for v in (0, 2))
    else:
        kw = dict(FALLBACKS[case])
        late = kw.pop("options", ())   # (set after INSTRUMENTED: the later value of an option stands)
        a, b = (render(v, "cornell_dragon", 257, 131, 4, options=late, **kw) for v in (0, 1))
        c0, c2 = (counted(v, "cornell_dragon", 257, 131, 4, options=late, **kw) for v in (0, 2))
    same(b, a, case)
    same(c2, a, f"{case}, instrumented")
    assert c2[2]["occluded"] == 0, f"{case}: the occluder test ran"
    assert stable(c2[2]) == stable(c0[2]), case


def frame_of(t, W, H, spp):
    acc, rgba = t.alloc_frame(W, H)
    p = g.default_params(W, H)
    p.flags, p.frame, p.sample_index = g.FLAG_WRITE_RGBA, 7, 1
    t.launch_kernel(acc.ptr, rgba.ptr, golden_camera(W, H), p, spp)
    t.sync()
    out = (acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W)))
    acc.free()
    rgba.free()
    return out


def test_long_lived_context_equals_fresh_ones():
    """upload, render, refit with a listed wall moved, render, another mesh (no list), render, the first mesh again, render: every
    frame is the one a fresh context without the option renders of that scene — no call tests the vertices of an earlier state"""
    W, H, spp = 129, 67, 4
    mesh, bvh = bvh_of("cornell_dragon")
    soup = mesh.triangle_soup()
    v, f = np.ascontiguousarray(mesh.verts, np.float32), np.ascontiguousarray(mesh.tris, np.int32)
    ids = (g._abi.C.c_int32 * 12)()
    n = g._abi.ptmi().pt_occluder_ids(v.ctypes.data, len(v), f.ctypes.data, len(f), ids, 12)
    assert n >= 2
    wall = [ids[0], ids[1]]   # the largest quad: equal areas, consecutive ids
    moved = soup.copy()
    centre = 0.5 * (v.min(0) + v.max(0))
    rows = moved[wall].reshape(-1, 3)
    moved[wall] = (rows + 0.25 * (centre - rows.mean(0))).astype(np.float32).reshape(-1, 9)   # a quarter of the way into the room
    steps = [("upload", lambda t: t.upload_bvh(bvh)), ("refit", lambda t: t.refit_bvh(moved)),
             ("other mesh", lambda t: t.upload_bvh(bvh_of("gto_sixteen")[1])), ("upload again", lambda t: t.upload_bvh(bvh))]

    def context(v):
        t = g.PathTracer(0)
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.set_option(OCCL, v)
        t.upload_spheres(g.reference_spheres())
        return t

    long_lived, got = context(1), []
    try:
        for _, step in steps:
            step(long_lived)
            got.append(frame_of(long_lived, W, H, spp))
    finally:
        long_lived.close()
    for k, (what, _) in enumerate(steps):
        fresh = context(0)
        try:
            for _, step in (steps[:2] if k == 1 else [steps[k]]):   # (a refit needs the tree it moves)
                step(fresh)
            same(got[k], frame_of(fresh, W, H, spp), f"long-lived context, {what}")
        finally:
            fresh.close()
    assert not np.array_equal(got[0][0], got[1][0]), "the moved wall changed nothing"
    same(got[3], got[0], "the first mesh again")


def test_persistent_kernel_and_oracle():
    W, H, spp = 64, 64, 4
    b = render(1, "cornell_dragon", W, H, spp)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
        t.upload_bvh(bvh_of("cornell_dragon")[1])
        t.upload_spheres(g.reference_spheres())
        same(b, frame_of(t, W, H, spp), "the persistent kernel's frame")
    finally:
        t.close()
    mesh, bvh = bvh_of("cornell_dragon")
    sph, cam = g.reference_spheres(), golden_camera(W, H)
    p = g.default_params(W, H)
    p.frame, p.sample_index, p.flags = 7, 1, g.FLAG_WRITE_RGBA
    ref = orc.render(bvh, sph, cam, p, spp)[:2]

    class T:
        name, exact = "wavefront-last-occluders", False
    judge(T, "cornell_dragon 64x64", b[:2], ref, mesh, sph, cam, p, spp)
