"""Trees are made as values and adopted on the context in one place (csrc/pt_tree.hip).

What a caller can see of that: a call that fails leaves the context as it was; whichever route adopted the tree, pt_refit_bvh gets
a schedule made for THAT tree; the light list and PT_KERNEL_AUTO's picks follow the adopted tree.  The scenes are the 32-triangle
cornell and gto_sixteen: PT_OPT_REBUILD 2 keeps the re-clustered tree on the first and the caller's on the second."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import golden_camera, gpu_trace, material, rays_for, soup_mesh

pytestmark = pytest.mark.gpu

W, H = 64, 48


def frame(t, cam, p, spp):
    acc, rgba = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
    t.sync()
    a = acc.download(np.float32, (H, W, 3))
    acc.free()
    rgba.free()
    return a


def upload(t, bvh, rebuild, optimize=0):
    t.set_option(g.OPT_REBUILD, rebuild)
    t.set_option(g.OPT_OPTIMIZE, optimize)
    try:
        t.upload_bvh(bvh)
    finally:
        t.set_option(g.OPT_REBUILD, 0)
        t.set_option(g.OPT_OPTIMIZE, 0)


# ---------------------------------------------------------------------------------------------- 1. a failed call changes nothing
@pytest.mark.parametrize("tree", ["uploaded", "device-built"])
def test_a_failed_call_changes_nothing(tree):
    mesh = g.scene_mesh("cornell")
    bvh = g.Bvh(mesh)
    rays = orc.random_rays(2000, *mesh.bounds(), seed=31)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    t = g.PathTracer(0)
    lib = t._lib
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
        t.upload_spheres(g.reference_spheres())
        if tree == "uploaded":
            t.upload_bvh(bvh)
            assert t.last_build_ms() == -1.0
        else:
            t.build_bvh(mesh)
            assert t.last_build_ms() > 0

        def state():
            return t.scene_info(), t.tree_cost(), t.last_build_ms(), gpu_trace(t, rays), frame(t, cam, p, 1)

        before = state()
        assert (before[3][1] >= 0).mean() > 0.05 and before[4].any()
        v, f = np.ascontiguousarray(mesh.verts, np.float32), np.ascontiguousarray(mesh.tris, np.int32)
        v_nan = v.copy()
        v_nan[5, 1] = np.nan
        f_bad = f.copy()
        f_bad[7, 2] = len(v)
        n, tr, ix = (np.ascontiguousarray(bvh.nodes, np.float32), np.ascontiguousarray(bvh.tris, np.float32),
                     np.ascontiguousarray(bvh.index, np.int32))
        for rebuild in (0, 1, 2):
            t.set_option(g.OPT_REBUILD, rebuild)
            assert lib.pt_build_bvh(t._ctx, v_nan.ctypes.data, len(v), f.ctypes.data, len(f)) != 0
            assert lib.pt_build_bvh(t._ctx, v.ctypes.data, len(v), f_bad.ctypes.data, len(f)) != 0
            assert lib.pt_upload_bvh(t._ctx, n.ctypes.data, n.size // 4 - 1, tr.ctypes.data, tr.size // 4, ix.ctypes.data, ix.size) != 0
            assert lib.pt_upload_bvh(t._ctx, n.ctypes.data, n.size // 4, tr.ctypes.data, tr.size // 4, ix.ctypes.data, ix.size - 1) != 0
        t.set_option(g.OPT_REBUILD, 0)
        after = state()
        assert after[:3] == before[:3]
        hit = before[3][1] >= 0                      # (a miss writes no normal)
        for a, b in zip((after[3][0], after[3][1], after[3][2][hit], after[4]), (before[3][0], before[3][1], before[3][2][hit], before[4])):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        t.close()


def test_a_tree_deeper_than_64_is_refused_and_changes_nothing():
    """comb(66) of tests/deep_trees.py: its last inner node is 65 edges below the root, one more than pt_upload_bvh parses, so the
    call answers PT_ERR_INVALID under every PT_OPT_REBUILD; comb(65), the deepest tree it takes (stack depth 65), is still on the
    context afterwards and still traces every half-cell ray as brute force does"""
    import deep_trees as dt
    held, deeper = dt.comb(65), dt.comb(66)
    assert (held.max_depth, deeper.max_depth) == (65, 66)
    rays = dt.cell_rays(held)
    assert dt.binary_stack_depth(held, rays).min() == 65
    t0, tri0, nrm0 = orc.trace_brute(held.mesh, rays, True)
    t = g.PathTracer(0)
    try:
        t.upload_bvh(held)
        before = t.scene_info(), t.tree_items()[3]
        assert before[0]["max_depth"] == 65 and before[1] == 22
        n, tr, ix = (np.ascontiguousarray(deeper.nodes, np.float32), np.ascontiguousarray(deeper.tris, np.float32),
                     np.ascontiguousarray(deeper.index, np.int32))
        for rebuild in (0, 1, 2):
            t.set_option(g.OPT_REBUILD, rebuild)
            rc = t._lib.pt_upload_bvh(t._ctx, n.ctypes.data, n.size // 4, tr.ctypes.data, tr.size // 4, ix.ctypes.data, ix.size)
            assert rc == -1, rebuild                 # PT_ERR_INVALID
        t.set_option(g.OPT_REBUILD, 0)
        assert (t.scene_info(), t.tree_items()[3]) == before and t.last_build_ms() == -1.0
        tg, ig, ng = gpu_trace(t, rays)
        assert np.array_equal(ig, tri0) and np.array_equal(tg.view(np.int32), t0.view(np.int32))
        assert np.array_equal(ng[tri0 >= 0], nrm0[tri0 >= 0]) and (tri0 >= 0).sum() == 66
    finally:
        t.close()


# --------------------------------------------------------------------------------------- 2. every route hands refit a fresh tree
@pytest.mark.parametrize("scene", ["cornell", "gto_sixteen"])
def test_every_route_hands_refit_a_fresh_tree(scene):
    mesh = g.scene_mesh(scene)
    bvh = g.Bvh(mesh)
    lo, hi = mesh.bounds()
    shift = np.array([0.11, -0.07, 0.05], np.float32) * (hi - lo)
    moved = (mesh.triangle_soup().reshape(-1, 3) + shift).astype(np.float32).reshape(-1, 9)
    moved_mesh = soup_mesh(moved)
    rays = rays_for(moved, 2000, 41)
    brute = {cull: orc.trace_brute(moved_mesh, rays, cull) for cull in (True, False)}
    assert (brute[False][1] >= 0).mean() >= 0.05
    t = g.PathTracer(0)
    try:
        def tree():
            return t.tree_cost(), t.scene_info()

        # the two candidates of PT_OPT_REBUILD 2, without and with PT_OPT_OPTIMIZE: which one a later upload kept shows in (cost, info)
        cand = {}
        for optimize in (0, 1):
            for rebuild in (0, 1):
                upload(t, bvh, rebuild, optimize)
                cand[(rebuild, optimize)] = tree()
            assert cand[(0, optimize)] != cand[(1, optimize)]

        def by_upload(rebuild, optimize):      # -> a device build stands behind the tree now on the context
            upload(t, bvh, rebuild, optimize)
            now = tree()
            if rebuild < 2:
                assert now == cand[(rebuild, optimize)]
            else:                                  # PT_OPT_REBUILD 2 kept one of the two candidates (asserted distinct above)
                assert now in (cand[(0, optimize)], cand[(1, optimize)])
            return now == cand[(1, optimize)]      # ... and the re-clustered one is the one a device build stands behind

        def by_build(optimize):
            t.set_option(g.OPT_OPTIMIZE, optimize)
            try:
                t.build_bvh(mesh)
            finally:
                t.set_option(g.OPT_OPTIMIZE, 0)
            return True

        routes = [("upload", lambda: by_upload(0, 0)), ("build", lambda: by_build(0)),
                  ("upload, rebuild 1, optimize 1", lambda: by_upload(1, 1)), ("upload, rebuild 2", lambda: by_upload(2, 0)),
                  ("upload, rebuild 2, optimize 1", lambda: by_upload(2, 1)), ("build, optimize 1", lambda: by_build(1))]
        kept = {}
        for what, adopt in routes:
            device_built = adopt()
            kept[what] = device_built
            assert (t.last_build_ms() > 0) == device_built, what
            t.refit_bvh(moved)
            for cull, (tb, ib, nb) in brute.items():
                tg, ig, ng = gpu_trace(t, rays, cull)
                bad = np.nonzero((ig != ib) | (tg.view(np.int32) != tb.view(np.int32)))[0]
                assert len(bad) == 0, f"{scene}, {what}, cull {cull}: {len(bad)} rays differ from brute force, first {bad[:5]}"
                hit = ib >= 0
                assert np.array_equal(ng[hit], nb[hit]), what
        print(f"{scene}: PT_OPT_REBUILD 2 kept the re-clustered tree: {kept['upload, rebuild 2']}, optimised: {kept['upload, rebuild 2, optimize 1']}")
        assert kept["upload, rebuild 2"] == (scene == "cornell")      # both outcomes occur (test_rebuild_2_keeps_the_cheaper_tree)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------ 3. the light list follows the tree
def test_the_light_list_follows_the_tree():
    mesh = g.scene_mesh("cornell")
    bvh = g.Bvh(mesh)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    p.depth, p.frame, p.flags = 3, 5, g.FLAG_NEE | g.FLAG_COSINE_DIFF
    p.bk_color[:] = (0, 0, 0)                 # the emitting triangle is the only light
    # the triangle most pixels look at emits; its neighbourhood: those pixels and the ones within 3 of them
    _, first, _ = orc.trace_brute(mesh, orc.primary_rays(cam, W, H, frame=p.frame, jitter=False), bool(p.cull_backfaces))
    first = first.reshape(H, W)
    emitter = int(np.bincount(first[first >= 0]).argmax())
    seen = np.pad(first == emitter, 3)
    near = np.zeros((H, W), bool)
    for dy in range(7):
        for dx in range(7):
            near |= seen[dy:dy + H, dx:dx + W]
    assert 50 < near.sum() < W * H
    table = [material((0.75, 0.75, 0.75)), material((0.78, 0.78, 0.78), emi=(17, 12, 4))]
    ids = np.zeros(mesh.n_tris, np.int32)
    ids[emitter] = 1
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.set_option(g.OPT_OVERLAP, 0)
        frames = []
        for rebuild in (0, 1, 0):
            upload(t, bvh, rebuild)
            if not frames:
                t.upload_tri_materials(table, ids)
            frames.append(frame(t, cam, p, 2))
            assert frames[-1][near].any(), f"frame {len(frames)}"
        assert np.array_equal(frames[2].view(np.int32), frames[0].view(np.int32))
        assert int(np.any(frames[1] != frames[0], axis=-1).sum()) <= 2
    finally:
        t.close()


# -------------------------------------------------------------------- 4. an adoption is a new scene to PT_KERNEL_AUTO's picks
def test_adoption_invalidates_the_auto_picks():
    bvh = g.Bvh(g.scene_mesh("cornell"))
    cam, p = golden_camera(W, H), g.default_params(W, H)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
        t.upload_bvh(bvh)
        t.upload_spheres(g.reference_spheres())
        acc, rgba = t.alloc_frame(W, H)
        for tree in ("first", "re-uploaded"):
            for trial in range(4):
                assert trial == 0 or t.auto_choice()[0] == g.KERNEL_AUTO, (tree, trial)   # trials again, not the earlier tree's pick
                t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 1)
            assert t.auto_choice()[0] in (g.KERNEL_PERSISTENT, g.KERNEL_WAVEFRONT)
            upload(t, bvh, 2)
    finally:
        t.close()
