"""pt_refit_bvh — the triangles move, the tree keeps its topology and its boxes are refit on the device.

What pins it is the invariant the device builder's tests use: the closest hit (exact Moller-Trumbore, equal-t ties to the
smaller id) does not depend on the tree, so after a refit
  * ray batches give the brute-force oracle's (t, id, normal) over the MOVED mesh, bit for bit,
  * frames equal the oracle's over a host tree built from the moved mesh (binary walks bit for bit, wide walks within the
    grazing-pixel bar of the existing tests, every differing pixel arbitrated against brute force),
and a refit to the vertices a device tree was built from reproduces that tree exactly."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import arbitrate, cornell_dragon_moved, golden_camera, gpu_trace, rays_for, soup_mesh, twist

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_NO_SCENE, PT_ERR_UNSUPPORTED = -1, -3, -5
WALKS = {"mega-0": (g.KERNEL_MEGA_BVH2, 0), "mega-2": (g.KERNEL_MEGA_BVH2, 2), "persistent-1": (g.KERNEL_PERSISTENT, 1),
         "persistent-4": (g.KERNEL_PERSISTENT, 4), "wavefront": (g.KERNEL_WAVEFRONT, 2), "auto": (g.KERNEL_AUTO, 2)}


TREES = ("device", "lbvh", "host", "optimize", "rebuild2", "presplit")


def install(t, mesh, kind):
    """Put a tree of `kind` over `mesh` on the context."""
    for opt, val in ((g.OPT_OPTIMIZE, 0), (g.OPT_REBUILD, 0), (g.OPT_PRESPLIT, 0), (g.OPT_BUILD_ALGO, 1), (g.OPT_LEAF_MAX, 2)):
        t.set_option(opt, val)
    if kind in ("device", "lbvh", "presplit"):
        t.set_option(g.OPT_BUILD_ALGO, 0 if kind == "lbvh" else 1)
        t.set_option(g.OPT_PRESPLIT, 100 if kind == "presplit" else 0)
        t.build_bvh(mesh)
    else:
        t.set_option(g.OPT_OPTIMIZE, 2 if kind in ("optimize", "rebuild2") else 0)
        t.set_option(g.OPT_REBUILD, 2 if kind == "rebuild2" else 0)
        t.upload_bvh(g.Bvh(mesh))
    for opt, val in ((g.OPT_OPTIMIZE, 0), (g.OPT_REBUILD, 0), (g.OPT_PRESPLIT, 0)):
        t.set_option(opt, val)


def check_hits(t, mesh, rays, what, min_hit=0.05):
    for cull in (True, False):
        tg, ig, ng = gpu_trace(t, rays, cull)
        tb, ib, nb = orc.trace_brute(mesh, rays, cull)
        bad = np.nonzero((ig != ib) | (tg.view(np.int32) != tb.view(np.int32)))[0]
        assert len(bad) == 0, f"{what} cull {cull}: {len(bad)} rays differ from brute force, first {bad[:5]}: {ig[bad[:5]]} vs {ib[bad[:5]]}"
        hit = ib >= 0
        assert hit.mean() >= min_hit and np.array_equal(ng[hit], nb[hit]), what


def render(t, cam, p, kernel, walk, frame=3):
    t.set_option(g.OPT_KERNEL, kernel)
    t.set_option(g.OPT_WALK, walk)
    W, H = p.width, p.height
    acc, rgba = t.alloc_frame(W, H)
    q = g.Params.from_buffer_copy(p)
    q.frame, q.sample_index = frame, 1
    t.launch_kernel(acc.ptr, rgba.ptr, cam, q, 1)
    t.sync()
    a = acc.download(np.float32, (H, W, 3))
    acc.free()
    rgba.free()
    return a


# ------------------------------------------------------------------------------------------------- 1. exact round trip
@pytest.mark.parametrize("algo,leaf_max", [(1, 1), (1, 2), (0, 1), (0, 2)], ids=["ploc-1", "ploc-2", "lbvh-1", "lbvh-2"])
def test_round_trip_reproduces_the_device_tree(algo, leaf_max):
    mesh, soup, moved = cornell_dragon_moved()
    W, H = 320, 180
    cam, p = golden_camera(W, H), g.default_params(W, H)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_BUILD_ALGO, algo)
        t.set_option(g.OPT_LEAF_MAX, leaf_max)
        t.build_bvh(mesh)
        t.upload_spheres(g.reference_spheres())
        info, build_ms = t.scene_info(), t.last_build_ms()
        cost = t.tree_cost()
        frames = {k: render(t, cam, p, *kw) for k, kw in WALKS.items()}
        for step, verts in (("own vertices", soup), ("deformed", moved), ("back", soup)):
            t.refit_bvh(verts)
            if step == "deformed":
                assert t.tree_cost() != cost
                continue
            assert t.tree_cost() == cost, step
            for k, kw in WALKS.items():
                a = render(t, cam, p, *kw)
                assert np.array_equal(a.view(np.int32), frames[k].view(np.int32)), f"{step}, {k}: {int(np.any(a != frames[k], axis=-1).sum())} pixels"
        assert t.scene_info() == info and t.last_build_ms() == build_ms   # a refit is no build
    finally:
        t.close()


# ------------------------------------------------------------------------------- 2. hits equal brute force after motion
@pytest.mark.parametrize("kind", TREES)
@pytest.mark.parametrize("name", ["bunny_low", "gto_sixteen", "cornell_dragon"])
def test_hits_after_motion_equal_brute_force(name, kind):
    if name == "cornell_dragon":
        mesh, soup, moved = cornell_dragon_moved()
    else:
        mesh = g.scene_mesh(name)
        soup = mesh.triangle_soup()
        moved = twist(soup, 0.8, np.array([0.05, -0.02, 0.03]))
    moved_mesh = soup_mesh(moved)
    t = g.PathTracer(0)
    try:
        install(t, mesh, kind)
        t.refit_bvh(moved)
        n = 30000 if name == "cornell_dragon" else 60000
        check_hits(t, moved_mesh, rays_for(moved, n, 5), f"{name} {kind} random")
        W, H = 160, 90
        check_hits(t, moved_mesh, orc.primary_rays(golden_camera(W, H), W, H, frame=2), f"{name} {kind} primary", 0.0)
    finally:
        t.close()


# --------------------------------------------------------------------------------- 3. frames equal the oracle after motion
@pytest.mark.parametrize("kind", ["device", "rebuild2"])
def test_frames_after_motion_equal_oracle(kind):
    mesh, soup, moved = cornell_dragon_moved(-40.0, (-2.0, 0.0, 1.5))
    moved_mesh = soup_mesh(moved)
    oracle_bvh = g.Bvh(moved_mesh)
    sph = g.reference_spheres()
    W, H = 640, 360
    cam, p = golden_camera(W, H), g.default_params(W, H)
    t = g.PathTracer(0)
    try:
        install(t, mesh, kind)
        t.upload_spheres(sph)
        t.refit_bvh(moved)
        for k, (kernel, walk) in WALKS.items():
            if k == "auto":
                continue
            t.set_option(g.OPT_KERNEL, kernel)
            t.set_option(g.OPT_WALK, walk)
            arbitrate(t, moved_mesh, oracle_bvh, sph, cam, p, [6], f"{kind} {k}", 0 if walk < 2 else 4)
    finally:
        t.close()


# ----------------------------------------------------------------------------------------------------- 4. moved lights
def test_moved_triangle_light_gives_the_oracle_image():
    mesh = g.scene_mesh("cornell_box")
    table, ids = mesh.materials, mesh.tri_material
    soup = mesh.triangle_soup()
    emi = np.array([[m.emi[0], m.emi[1], m.emi[2]] for m in table], np.float32)
    quad = np.nonzero(np.any(emi[ids] != 0, axis=1))[0]
    assert len(quad) == 2
    v = soup.reshape(-1, 3)
    ext = v.max(0) - v.min(0)
    moved = soup.copy()
    moved[quad] = (soup[quad].reshape(-1, 3) + np.array([0.15, -0.2, 0.1], np.float32) * ext).reshape(-1, 9)
    W, H, spp = 160, 120, 2
    cam, p = g.default_camera(W, H), g.default_params(W, H)
    p.depth, p.frame, p.flags = 4, 9, g.FLAG_NEE | g.FLAGS_SMALLPT
    p.bk_color[:] = (0, 0, 0)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_MEGA_BVH2)
        t.set_option(g.OPT_WALK, 1)
        t.upload_bvh(g.Bvh(mesh))
        t.upload_tri_materials(table, ids)
        acc, rgba = t.alloc_frame(W, H)
        for verts in (soup, moved, soup, moved):
            m = soup_mesh(verts)
            ref, _, _ = orc.render(g.Bvh(m), None, cam, p, spp, materials=table, tri_material=ids, lights=orc.tri_lights(m, table, ids))
            t.refit_bvh(verts)
            acc.zero()
            t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
            t.sync()
            a = acc.download(np.float32, (H, W, 3))
            assert a.mean() > 0.01
            assert np.array_equal(a, ref), int(np.any(a != ref, axis=-1).sum())
    finally:
        t.close()


# ------------------------------------------------------------------------------------------ 5. ordering without host syncs
@pytest.mark.parametrize("kernel", [g.KERNEL_PERSISTENT, g.KERNEL_MEGA_BVH2])
def test_refits_between_overlapped_renders_need_no_host_sync(kernel):
    mesh, soup, moved = cornell_dragon_moved(60.0, (0.0, 3.0, 0.0))
    W, H = 400, 225
    cam, p = golden_camera(W, H), g.default_params(W, H)
    p.frame, p.sample_index = 11, 1
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, kernel)
        t.set_option(g.OPT_WALK, 2)
        t.set_option(g.OPT_OVERLAP, 1)
        t.build_bvh(mesh)
        t.upload_spheres(g.reference_spheres())
        v0, v1 = t.malloc(soup.nbytes), t.malloc(moved.nbytes)
        v0.upload(soup)
        v1.upload(moved)
        ref = {}
        for name, buf in (("V1", v1), ("V0", v0)):    # reference frames, one at a time
            t.refit_bvh(buf)
            ref[name] = render(t, cam, p, kernel, 2, frame=11)
        assert not np.array_equal(ref["V0"], ref["V1"])
        BW, BH = 1920, 1080
        big_acc, big_rgba = t.alloc_frame(BW, BH)
        bcam, bp = golden_camera(BW, BH), g.default_params(BW, BH)
        bp.depth = 6
        bufs = [t.alloc_frame(W, H) for _ in range(4)]
        for rep in range(2):                         # keep the caller's stream busy (the first round allocates the side buffers)
            t.sync()
            for k in range(3):
                bp.frame = 100 + k
                t.launch_kernel(big_acc.ptr, big_rgba.ptr, bcam, bp, 4)
        seq = [("V0", None), ("V0", None), ("V1", v1), ("V0", v0)]
        for (name, refit_to), (acc, rgba) in zip(seq, bufs):
            if refit_to is not None:
                t.refit_bvh(refit_to)
            t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 1)
        t.sync()
        for i, ((name, _), (acc, _)) in enumerate(zip(seq, bufs)):
            a = acc.download(np.float32, (H, W, 3))
            assert np.array_equal(a, ref[name]), f"call {i} ({name}): {int(np.any(a != ref[name], axis=-1).sum())} pixels differ"
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------- 6. dropped triangles
@pytest.mark.parametrize("kind", ["device", "host"])
def test_dropped_triangles_are_never_hit_and_counted_once(kind):
    mesh = g.scene_mesh("gto_sixteen")
    soup = mesh.triangle_soup()
    rng = np.random.default_rng(3)
    drop = np.sort(rng.choice(len(soup), len(soup) // 20, replace=False))
    bad = soup.copy()
    for i, r in enumerate(drop):
        bad[r, rng.integers(9)] = (np.nan, np.inf, -np.inf, np.float32(3.2e38), np.float32(-3.2e38))[i % 5]
    keep = np.setdiff1d(np.arange(len(soup)), drop)
    kept_mesh = soup_mesh(soup[keep])
    t = g.PathTracer(0)
    try:
        install(t, mesh, kind)
        cnt = t.malloc(4)
        t.refit_bvh(bad, n_dropped=cnt)
        t.sync()
        assert int(cnt.download(np.uint32, (1,))[0]) == len(drop)
        rays = rays_for(soup, 60000, 9)
        for cull in (True, False):
            tg, ig, _ = gpu_trace(t, rays, cull)
            tb, ib, _ = orc.trace_brute(kept_mesh, rays, cull)
            ib = np.where(ib >= 0, keep[np.maximum(ib, 0)], -1)
            assert not np.isin(ig, drop).any()
            assert np.array_equal(ig, ib) and np.array_equal(tg, tb)
        t.refit_bvh(soup, n_dropped=cnt)                  # back: every triangle again
        t.sync()
        assert int(cnt.download(np.uint32, (1,))[0]) == 0
        check_hits(t, mesh, rays, f"{kind} restored")
    finally:
        t.close()


# ----------------------------------------------------------------------------------------- 7. stale state + error codes
def test_stale_state_and_errors():
    a, b = g.scene_mesh("bunny_low"), g.scene_mesh("gto_sixteen")
    t = g.PathTracer(0)
    lib = t._lib
    try:
        sa = a.triangle_soup()
        buf = t.malloc(sa.nbytes)
        buf.upload(sa)
        assert lib.pt_refit_bvh(t._ctx, buf.ptr, len(sa), None) == PT_ERR_NO_SCENE
        t.upload_bvh(g.Bvh(a))
        t.refit_bvh(twist(sa, 0.5, 0.0))
        sb = b.triangle_soup()
        assert len(sb) != len(sa)
        t.upload_bvh(g.Bvh(b))
        mb = twist(sb, -0.6, np.array([0.1, 0.0, 0.0]))
        t.refit_bvh(mb)
        check_hits(t, soup_mesh(mb), rays_for(mb, 40000, 13), "after a new upload")
        t.build_bvh(a)
        ma = twist(sa, 0.7, 0.0)
        t.refit_bvh(ma)
        check_hits(t, soup_mesh(ma), rays_for(ma, 40000, 14), "after a device build")
        # PT_OPT_TIMING brackets the refit: nothing else on this context was timed, so pt_last_kernel_ms is the refit's time
        with pytest.raises(g.PtError):
            t.last_kernel_ms()
        t.set_option(g.OPT_TIMING, 1)
        t.refit_bvh(ma)
        ms = t.last_kernel_ms()
        t.set_option(g.OPT_TIMING, 0)
        assert np.isfinite(ms) and 0.0 < ms < 1000.0, ms
        # errors
        assert lib.pt_refit_bvh(t._ctx, None, len(sa), None) == PT_ERR_INVALID
        assert lib.pt_refit_bvh(t._ctx, buf.ptr, len(sa) - 1, None) == PT_ERR_INVALID
        assert lib.pt_refit_bvh(t._ctx, buf.ptr, 0, None) == PT_ERR_INVALID
        t.set_option(g.OPT_TRI_TEST, 1)
        t.upload_bvh(g.Bvh(a))
        assert lib.pt_refit_bvh(t._ctx, buf.ptr, len(sa), None) == PT_ERR_UNSUPPORTED
        buf.free()
    finally:
        t.close()


# -------------------------------------------------------------------------------------------------------- 8. scale check
def test_scaling_by_two_doubles_t_exactly():
    mesh = g.scene_mesh("dragon")
    soup = mesh.triangle_soup()
    t = g.PathTracer(0)
    try:
        t.build_bvh(mesh)
        rays = rays_for(soup, 60000, 17)
        t0, i0, _ = gpu_trace(t, rays, True)
        t.refit_bvh(soup * np.float32(2.0))
        r2 = rays.copy()
        r2[:, :3] *= np.float32(2.0)
        t2, i2, _ = gpu_trace(t, r2, True)
        hit = i0 >= 0
        assert hit.mean() > 0.1
        assert np.array_equal(i2, i0)
        assert np.array_equal(t2[hit], np.float32(2.0) * t0[hit])
    finally:
        t.close()


@pytest.mark.parametrize("kind", ["device", "host"])
def test_one_triangle_tree_refits(kind):
    """The smallest tree: pt_build_bvh doubles a lone triangle, the host builder's root has one leaf; both have an inner root."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    mesh = g.Mesh.from_arrays(tri, np.array([[0, 1, 2]], np.int32))
    moved = (tri + np.array([0.5, 0.25, 2.0], np.float32)).reshape(1, 9)
    rng = np.random.default_rng(23)
    n = 4000
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    target = w @ moved.reshape(3, 3)
    o = target + rng.normal(size=(n, 3)).astype(np.float32) * 3.0
    d = target - o
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 4:7] = o, d / np.linalg.norm(d, axis=1, keepdims=True)
    t = g.PathTracer(0)
    try:
        install(t, mesh, kind)
        t.refit_bvh(moved)
        check_hits(t, soup_mesh(moved), rays, f"one triangle, {kind}", 0.3)
    finally:
        t.close()
