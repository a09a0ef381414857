"""Oracle parity on inputs the rest of the suite never varies: camera poses other than the default one, sphere sets other
than the 8 reference spheres (more than the kernel-argument block holds, stale rows, METAL / REFR, no BVH at all), and
triangles that tie exactly in t (the smaller id must win in every walk, builder, optimiser and refit).  pt_trace_rays and
pt_render_aux always run the binary walk, so their checks run once; the ties reach the other walks through rendered frames
(red-emitting copies, and a grid whose triangles each emit their own colour seen through exact ties at its shared edges).

Bars, as elsewhere in the suite: walks 0 / 1 equal the oracle bit for bit (accumulator and display words); the wide walks
(the stage-split pipeline included) stay under per-pixel L2 1e-3 with at most MAX_DIFF differing pixels per frame, each of
which must hold the brute-force renderer's colour sample by sample; and the three stage-split variants agree bit for bit.
The inputs are defined in scene_matrix.py; test_scene_matrix_oracle.py checks the oracle on them."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
from gpu_support import MAX_DIFF, STAGE_SPLIT, arbitrate, bvh_of, compare_guides, gpu_trace, judge, n_diff_seen, oracle, setup_scene, turn_rows
from scene_matrix import (N_ROOM, PINHOLE_SIDES, POSES, SPHERE_SETS, SPHERES_ONLY, STALE_THREE, axis_rays, copy_rows, duplicated,
                          grid_mesh, grid_rays, many_spheres, pinhole_camera, pinhole_params, pose_camera, pose_spheres,
                          red_copies_table, tilted_grid, tilted_grid_table, unreachable_spheres)

pytestmark = pytest.mark.gpu

VARIANTS = {
    # id: (kernel, walk, other options)
    "mega-unified": (g.KERNEL_MEGA_BVH2, 1, ()),
    "persistent-whilewhile": (g.KERNEL_PERSISTENT, 0, ()),
    "persistent-wide": (g.KERNEL_PERSISTENT, 2, ()),
    "persistent-postponed": (g.KERNEL_PERSISTENT, 4, ()),
    "wavefront": (g.KERNEL_WAVEFRONT, 2, ()),
    "wavefront-per-lane": (g.KERNEL_WAVEFRONT, 2, ((g.OPT_FIRST_WALK, 0),)),
    "wavefront-unfused": (g.KERNEL_WAVEFRONT, 2, ((g.OPT_FUSE_STAGES, 0),)),
}
WAVEFRONT = [v for v in VARIANTS if v.startswith("wavefront")]
assert tuple(WAVEFRONT) == STAGE_SPLIT   # the variants gpu_support.judge holds to one another


def make_tracer(name):
    kernel, walk, opts = VARIANTS[name]
    t = g.PathTracer(0)
    t.set_option(g.OPT_KERNEL, kernel)
    t.set_option(g.OPT_WALK, walk)
    for o, v in opts:
        t.set_option(o, v)
    t.name, t.exact = name, walk in (0, 1)
    return t


@pytest.fixture(scope="module", params=list(VARIANTS), ids=list(VARIANTS))
def pt(request):
    t = make_tracer(request.param)
    yield t
    print(f"[{t.name}] differing pixels against the oracle, all equal to brute force: {n_diff_seen.get(t.name, 0)}")
    t.close()


def frame_of(t, cam, p, spp, prev=None):
    W, H = p.width, p.height
    acc, rgba = t.alloc_frame(W, H)
    if prev is not None:
        acc.upload(prev)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
    t.sync()
    out = acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W))
    acc.free()
    rgba.free()
    return out


def render_case(t, case, mesh, bvh, sph, cam, p, spp, prev=None, materials=None, tri_material=None, upload=True):
    """one call on the context against the cached oracle frame of `case`"""
    if upload:
        t.upload_tri_materials(None, None)
        t.upload_bvh(bvh)
        t.upload_spheres(sph)
        if materials is not None:
            t.upload_tri_materials(materials, tri_material)
    mk = dict(materials=materials, tri_material=tri_material)
    ref = oracle(("matrix", case), lambda: orc.render(bvh, sph, cam, p, spp, accum=None if prev is None else prev.copy(), **mk)[:2])
    got = frame_of(t, cam, p, spp, prev)
    judge(t, case, got, ref, mesh, sph, cam, p, spp, prev, **mk)
    return got


def params(W, H, depth=4, frame=7, first=1, flags=0):
    p = g.default_params(W, H, depth=depth)
    p.frame, p.sample_index, p.flags = frame, first, flags | g.FLAG_WRITE_RGBA
    return p


# ---------------------------------------------------------------------------------------------------- A. camera poses
# (W, H, spp, depth, prefilled accumulator): the ragged frame and the running mean on the reversed view, 8 spp at depth 2 on
# the narrow one, 16 spp at depth 4 (the fused fold) everywhere else
POSE_CFG = {name: (320, 180, 16, 4, False) for name in POSES}
POSE_CFG["reversed"] = (257, 131, 16, 4, True)
POSE_CFG["narrow"] = (320, 180, 8, 2, False)


@pytest.mark.parametrize("pose", list(POSES))
def test_camera_pose(pt, pose):
    W, H, spp, depth, prefill = POSE_CFG[pose]
    mesh, bvh = bvh_of("cornell_dragon")
    sph, cam = pose_spheres(pose), pose_camera(pose, W, H)
    prev = np.random.default_rng(11).random((H, W, 3), dtype=np.float32) if prefill else None
    p = params(W, H, depth, frame=40, first=17 if prefill else 1)
    acc, _ = render_case(pt, f"pose {pose}", mesh, bvh, sph, cam, p, spp, prev)
    assert np.isfinite(acc).all()


@pytest.mark.parametrize("pose", list(POSES))
def test_camera_pose_guides(pose):
    """pt_render_aux against denoise_ref.guides from every pose, on the denoise tests' scenes (cull on and off); the oracle's
    first hits are non-trivial except where the view sees nothing"""
    W, H = 257, 131
    t = g.PathTracer(0)
    try:
        for scene, mats in (("cornell_dragon", False), ("room", False), ("cornell_box", True)):
            bvh, sph, tab, tm = setup_scene(t, scene, mats)
            if scene != "cornell_box" and not POSES[pose][1]:
                sph = None
                t.upload_spheres(None)
            cam = pose_camera(pose, W, H)
            bufs = [t.malloc(W * H * 16) for _ in range(3)] + [t.malloc(W * H * 4)]
            for cull in (1, 0):
                p = g.default_params(W, H)
                p.cull_backfaces = cull
                t.render_aux(cam, p, *(b.ptr for b in bufs))
                t.sync()
                got = tuple(b.download(np.float32, (H, W, 4)) for b in bufs[:3]) + (bufs[3].download(np.int32, (H, W)),)
                ref = R.guides(bvh, sph, cam, p, tab, tm)
                compare_guides(got, ref, f"{pose} {scene} cull {cull}")
                if scene == "cornell_dragon" and cull:
                    if pose == "away":
                        assert (ref[3] == -1).all()
                    else:
                        assert (ref[3] >= 0).mean() > 0.05, pose
                        assert sph is None or (ref[3] <= -2).any(), pose
            for b in bufs:
                b.free()
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- B. sphere sets
@pytest.mark.parametrize("case", list(SPHERE_SETS))
def test_sphere_set(pt, case):
    W, H = (257, 131) if case == "forty" else (320, 180)
    mesh, bvh = bvh_of("cornell_dragon")
    sph = SPHERE_SETS[case]()
    cam = pose_camera("control", W, H)
    spp, depth = (8, 2) if case == "one-emitter" else (16, 4)
    p = params(W, H, depth, frame=3)
    acc, _ = render_case(pt, f"spheres {case}", mesh, bvh, sph, cam, p, spp)
    assert np.isfinite(acc).all() and acc.any()


def test_stale_sphere_rows(pt):
    """8 spheres, then 3 on the same context: rows 3..7 of the first upload stay behind in the kernel-argument copy"""
    W, H = 320, 180
    mesh, bvh = bvh_of("cornell_dragon")
    cam, p = pose_camera("control", W, H), params(W, H, frame=9)
    render_case(pt, "stale: eight first", mesh, bvh, g.reference_spheres(), cam, p, 16)
    pt.upload_spheres(STALE_THREE())
    render_case(pt, "stale: three after eight", mesh, bvh, STALE_THREE(), cam, p, 16, upload=False)


def test_unreachable_spheres_change_nothing(pt):
    """the reference set and 24 spheres no ray can reach (the global-array path): bit-identical to the 8-sphere frame of the
    same variant, whatever the oracle says"""
    W, H = 320, 180
    _, bvh = bvh_of("cornell_dragon")
    cam, p = pose_camera("control", W, H), params(W, H, frame=21)
    frames = []
    for sph in (g.reference_spheres(), unreachable_spheres()):
        pt.upload_bvh(bvh)
        pt.upload_spheres(sph)
        frames.append(frame_of(pt, cam, p, 16))
    assert len(unreachable_spheres()) > 8
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])
    assert frames[0][0].any()


@pytest.mark.parametrize("name", ["mega-unified"] + WAVEFRONT)
def test_nee_with_forty_spheres(name):
    """PT_FLAG_NEE | PT_FLAG_COSINE_DIFF: light samples among the first 8 spheres, shadow rays against all 40"""
    W, H = 320, 180
    mesh, bvh = bvh_of("cornell_dragon")
    sph = many_spheres()
    cam = pose_camera("control", W, H)
    p = params(W, H, frame=5, flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF)
    t = make_tracer(name)
    try:
        render_case(t, "nee forty", mesh, bvh, sph, cam, p, 16)
    finally:
        t.close()


def test_spheres_only_every_kernel():
    """no BVH ever uploaded on the context: every kernel request (the stage-split pipeline falls back to the persistent
    kernel) equals the oracle bit for bit; no triangle walk runs, so no tolerance applies"""
    W, H = 257, 131
    sph = SPHERES_ONLY()
    cam = pose_camera("control", W, H)
    for spp, depth, prefill in ((16, 4, False), (8, 2, True)):
        prev = np.random.default_rng(4).random((H, W, 3), dtype=np.float32) if prefill else None
        p = params(W, H, depth, frame=2, first=9 if prefill else 1)
        ref = orc.render(None, sph, cam, p, spp, accum=None if prev is None else prev.copy())[:2]
        for kernel, walk in ((g.KERNEL_MEGA_BVH2, 1), (g.KERNEL_MEGA_BVH2, 0), (g.KERNEL_PERSISTENT, 0), (g.KERNEL_PERSISTENT, 2),
                             (g.KERNEL_PERSISTENT, 4), (g.KERNEL_WAVEFRONT, 2), (g.KERNEL_AUTO, 2)):
            t = g.PathTracer(0)
            try:
                t.set_option(g.OPT_KERNEL, kernel)
                t.set_option(g.OPT_WALK, walk)
                t.upload_spheres(sph)
                acc, rgba = frame_of(t, cam, p, spp, prev)
            finally:
                t.close()
            assert np.array_equal(acc, ref[0]) and np.array_equal(rgba, ref[1]), (kernel, walk, spp)
        assert ref[0].std() > 0.01


# ---------------------------------------------------------------------------------------------------- C. coincident triangles
# pt_trace_rays (k_trace_rays_bvh2) and pt_render_aux run the binary walk whatever PT_OPT_KERNEL / PT_OPT_WALK say, so their
# checks run once per tree, not once per variant; the frames below carry the ties into every variant's own walk.
_dup_cache = {}
_brute_cache = {}


def dup_scene(reverse=False):
    if reverse not in _dup_cache:
        mesh, n0 = duplicated(g.scene_mesh("cornell_dragon"), reverse)
        _dup_cache[reverse] = (mesh, g.Bvh(mesh), n0)
    return _dup_cache[reverse]


def check_ids(t, mesh, n0, what, copies_lose=True, seed=5, key=None):
    """pt_trace_rays on the tree on the context against brute force over `mesh` (cached under `key`): t and id bit for bit,
    normals of the hits; with copies_lose no id may be a copy's"""
    lo, hi = mesh.bounds()
    rays = orc.random_rays(60000, lo, hi, seed=seed)
    for cull in (True, False):
        tg, ig, ng = gpu_trace(t, rays, cull)
        ck = (key, seed, cull)
        tb, ib, nb = _brute_cache[ck] if key and ck in _brute_cache else orc.trace_brute(mesh, rays, cull)
        if key:
            _brute_cache[ck] = (tb, ib, nb)
        bad = np.nonzero((ig != ib) | (tg.view(np.int32) != tb.view(np.int32)))[0]
        assert len(bad) == 0, f"{what} cull {cull}: {len(bad)} rays differ from brute force, first {bad[:4]}: {ig[bad[:4]]} vs {ib[bad[:4]]}"
        hit = ib >= 0
        assert hit.mean() > 0.1 and np.array_equal(ng[hit], nb[hit]), what
        if copies_lose:
            assert ig.max() < n0, f"{what} cull {cull}: a copy won a tie"


def test_coincident_triangles(pt):
    """cornell_dragon + identical copies (32 room triangles, every 7th dragon triangle) at higher ids that emit red: each
    variant's frame must show the originals only"""
    mesh, bvh, n0 = dup_scene()
    W, H = 320, 180
    cam = pose_camera("control", W, H)
    p = params(W, H, frame=13)
    tab, tm = red_copies_table(n0, mesh.n_tris, p)
    render_case(pt, "coincident", mesh, bvh, g.reference_spheres(), cam, p, 16, materials=tab, tri_material=tm)


@pytest.mark.parametrize("cull", [1, 0])
def test_coincident_reversed_copies(pt, cull):
    """copies with reversed winding: culled where the original faces the ray (cull on), a near-tie otherwise"""
    mesh, bvh, _ = dup_scene(reverse=True)
    W, H = 257, 131
    cam = pose_camera("oblique", W, H)
    p = params(W, H, frame=17)
    p.cull_backfaces = cull
    render_case(pt, f"reversed copies cull {cull}", mesh, bvh, g.reference_spheres(), cam, p, 8)


def test_coincident_ray_batch_and_guide_ids():
    """the binary walk of pt_trace_rays and pt_render_aux on the duplicated meshes: ids equal brute force and no copy wins"""
    t = g.PathTracer(0)
    try:
        for reverse in (False, True):
            mesh, bvh, n0 = dup_scene(reverse)
            t.upload_bvh(bvh)
            check_ids(t, mesh, n0, f"coincident, reversed {reverse}", copies_lose=not reverse, seed=6 if reverse else 5,
                      key="dup-reversed" if reverse else "dup")
        mesh, bvh, n0 = dup_scene()
        t.upload_bvh(bvh)
        t.upload_spheres(g.reference_spheres())
        W, H = 320, 180
        cam, q = pose_camera("control", W, H), g.default_params(W, H)
        tab, tm = red_copies_table(n0, mesh.n_tris, q)
        t.upload_tri_materials(tab, tm)
        bufs = [t.malloc(W * H * 16) for _ in range(3)] + [t.malloc(W * H * 4)]
        t.render_aux(cam, q, *(b.ptr for b in bufs))
        t.sync()
        got = tuple(b.download(np.float32, (H, W, 4)) for b in bufs[:3]) + (bufs[3].download(np.int32, (H, W)),)
        for b in bufs:
            b.free()
        compare_guides(got, R.guides(bvh, g.reference_spheres(), cam, q, tab, tm), "coincident guides")
        assert got[3].max() < n0 and (got[3] >= N_ROOM).mean() > 0.01
    finally:
        t.close()


def test_grid_ray_batch():
    """integer grids through pt_trace_rays (the binary walk): exact rays through the shared edges and vertices equal the
    oracle's walk and brute force in t, id and normal; axis-aligned rays that lie IN bounding planes equal the oracle's walk
    over the same boxes bit for bit (the producer's own leaves, PT_OPT_LEAF_MAX 0)"""
    mesh = grid_mesh()
    bvh = g.Bvh(mesh)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_LEAF_MAX, 0)
        t.upload_bvh(bvh)
        for cull in (True, False):
            rays = grid_rays()
            tg, ig, ng = gpu_trace(t, rays, cull)
            t0, i0, n0, _ = orc.trace_bvh(bvh, rays, cull)
            tb, ib, nb = orc.trace_brute(mesh, rays, cull)
            assert np.array_equal(t0, tb) and np.array_equal(i0, ib)
            assert np.array_equal(tg, tb) and np.array_equal(ig, ib), f"cull {cull}"
            assert np.array_equal(ng, n0) and np.array_equal(ng[ib >= 0], nb[ib >= 0])
            assert (ib >= 0).mean() > 0.4
            rays = axis_rays()
            tg, ig, ng = gpu_trace(t, rays, cull)
            t0, i0, n0, _ = orc.trace_bvh(bvh, rays, cull)
            assert np.array_equal(tg.view(np.int32), t0.view(np.int32)) and np.array_equal(ig, i0) and np.array_equal(ng, n0), f"axis rays, cull {cull}"
            assert (i0 >= 0).mean() > 0.2
    finally:
        t.close()


def test_grid_ties_in_frames(pt):
    """every variant's own walk on exact edge ties: a tilted grid whose triangles each emit a colour of their own, seen by a
    fov-0 camera whose every ray passes exactly through one square's shared diagonal (both triangles at the same t, the
    smaller id must win), from above with culling and from below without"""
    mesh, mids = tilted_grid()
    bvh = g.Bvh(mesh)
    tab, tm = tilted_grid_table(mesh.n_tris)
    pt.upload_tri_materials(None, None)
    pt.upload_bvh(bvh)
    pt.upload_spheres(None)
    pt.upload_tri_materials(tab, tm)
    try:
        for side, (below, cull) in PINHOLE_SIDES.items():
            p = pinhole_params(cull)
            for k, (x, y) in enumerate(mids):
                cam = pinhole_camera(x, y, below)
                acc, _ = render_case(pt, f"grid tie {side} {k}", mesh, bvh, None, cam, p, 1, materials=tab, tri_material=tm,
                                     upload=False)
                assert np.array_equal(acc[0, 0], np.array(tab[2 * k].emi, np.float32)), f"[{pt.name}] {side} square {k}"
    finally:
        pt.upload_tri_materials(None, None)


@pytest.mark.parametrize("tree", ["lbvh", "ploc", "rebuild2-optimize3", "refit"])
def test_coincident_through_builders(tree):
    """the duplicated mesh through the device builders, the upload-time optimiser with re-clustering, and a refit that moves
    each original and its copy alike: ids against brute force, frames against the oracle with arbitration"""
    mesh, bvh, n0 = dup_scene()
    W, H = 320, 180
    cam = pose_camera("control", W, H)
    p = g.default_params(W, H)
    tab, tm = red_copies_table(n0, mesh.n_tris, p)
    t = g.PathTracer(0)
    try:
        if tree in ("lbvh", "ploc"):
            t.set_option(g.OPT_BUILD_ALGO, 0 if tree == "lbvh" else 1)
            t.build_bvh(mesh)
        elif tree == "rebuild2-optimize3":
            t.set_option(g.OPT_REBUILD, 2)
            t.set_option(g.OPT_OPTIMIZE, 3)
            t.upload_bvh(bvh)
            t.set_option(g.OPT_REBUILD, 0)
            t.set_option(g.OPT_OPTIMIZE, 0)
        else:
            t.upload_bvh(bvh)
            soup = mesh.triangle_soup()
            dragon = np.concatenate([np.arange(N_ROOM, n0), np.arange(n0 + N_ROOM, mesh.n_tris)])   # originals and copies alike
            moved = turn_rows(soup, dragon, 20.0, (1.0, 0.5, -1.0))
            assert np.array_equal(moved[n0:], moved[copy_rows(mesh)[: mesh.n_tris - n0]])
            t.refit_bvh(moved)
            mesh = g.Mesh.from_arrays(moved.reshape(-1, 3), np.arange(3 * len(moved), dtype=np.int32).reshape(-1, 3))
            bvh = g.Bvh(mesh)
        assert t.scene_info()["n_tri_refs"] >= mesh.n_tris
        check_ids(t, mesh, n0, f"{tree} tree", key="moved" if tree == "refit" else "dup")
        t.upload_spheres(g.reference_spheres())
        t.upload_tri_materials(tab, tm)
        n_diff, _ = arbitrate(t, mesh, bvh, g.reference_spheres(), cam, p, range(30, 34), f"coincident, {tree} tree", 4 * MAX_DIFF,
                              materials=tab, tri_material=tm)
        print(f"{tree}: {n_diff} differing (frame, pixel) pairs, all brute force's")
    finally:
        t.close()
