"""GPU tests of pt_temporal_motion (temporal reprojection for triangles moved by pt_refit_bvh) against the CPU reference of
tests/motion_ref.py: random colour over real guides of a mesh at rest and after its refit, pt_temporal's bits wherever nothing
moved, the row bound, aliasing, call ordering, the quality of a sequence with moving blocks, errors, freedom from side effects
and pt_app --spin-deg."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import motion_ref as M
import temporal_ref as T
from gpu_support import Guides, bits, golden_camera, setup_scene, soup_mesh, twist
from temporal_ref import FRAGILE_MAX, PARAM_SETS, QUALITY_FRAMES, QUALITY_SPP, params, random_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


def motion_gpu(t, W, H, prev_cam, verts, prev, cur, out_alias=False, with_rgba=True, with_motion=True, same_verts=False, **kw):
    """pt_temporal_motion over host arrays: verts = (prev soup, cur soup, n_tris) — uploaded as two buffers, or as one when
    same_verts — or None (no history), prev = (color, length, normal, position, id) or None, cur = (color, normal, position,
    id).  Returns (out, length, rgba or None, motion or None)."""
    bufs = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = t.malloc(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
        return b

    dprev = [up(a) for a in prev] if prev is not None else [None] * 5
    dcur = [up(a) for a in cur]
    pv = cv = None
    n = 0
    if verts is not None:
        n = verts[2]
        pv = up(np.asarray(verts[0], np.float32))
        cv = pv if same_verts else up(np.asarray(verts[1], np.float32))
    do = dcur[0] if out_alias else t.malloc(W * H * 12)
    dl = t.malloc(W * H * 4)
    dr = t.malloc(W * H * 4) if with_rgba else None
    dm = t.malloc(W * H * 8) if with_motion else None
    bufs += [b for b in (None if out_alias else do, dl, dr, dm) if b is not None]
    if dm is not None:
        dm.upload(np.full((H, W, 2), 77.0, np.float32))   # every pixel must be written
    ptr = lambda b: b.ptr if b is not None else None   # noqa: E731
    t.temporal_motion(W, H, prev_cam, ptr(pv), ptr(cv), n, *[ptr(b) for b in dprev], *[ptr(b) for b in dcur], do.ptr, dl.ptr, ptr(dr), ptr(dm),
                      **params(**kw))
    t.sync()
    out, length = do.download(np.float32, (H, W, 3)), dl.download(np.float32, (H, W))
    rgba = dr.download(np.uint32, (H, W)) if dr else None
    motion = dm.download(np.float32, (H, W, 2)) if dm else None
    for b in bufs:
        b.free()
    return out, length, rgba, motion


def temporal_gpu(t, W, H, prev_cam, prev, cur, **kw):
    """pt_temporal over the same host arrays: (out, length, rgba)."""
    bufs = [t.malloc(max(np.ascontiguousarray(a).nbytes, 4)) for a in list(prev) + list(cur)]
    for b, a in zip(bufs, list(prev) + list(cur)):
        b.upload(np.ascontiguousarray(a))
    do, dl, dr = t.malloc(W * H * 12), t.malloc(W * H * 4), t.malloc(W * H * 4)
    t.temporal(W, H, prev_cam, *[b.ptr for b in bufs], do.ptr, dl.ptr, dr.ptr, **params(**kw))
    t.sync()
    got = do.download(np.float32, (H, W, 3)), dl.download(np.float32, (H, W)), dr.download(np.uint32, (H, W))
    for b in bufs + [do, dl, dr]:
        b.free()
    return got


# ---------------------------------------------------------------------------------------------------- against the reference
_cases = {}


def case_guides(t, name, W, H, move):
    """(prev_cam, rest soup, moved soup, guides at rest from prev_cam, guides after the refit from the moved camera): the mesh
    built on the device from its soup (ids = rows), both sides of the triangles drawn."""
    key = (name, W, H, move)
    if key not in _cases:
        rest, moved = M.case_soups(name)
        prev_cam = M.case_camera(name, rest, W, H)
        p = g.default_params(W, H)
        p.cull_backfaces = 0
        t.upload_tri_materials(None, None)
        t.upload_spheres([])
        t.build_bvh(soup_mesh(rest))
        gb = Guides(t, W, H)
        gb.render(prev_cam, p)
        gp = gb.download()[1:4]
        t.refit_bvh(moved)
        gb.render(T.moved(prev_cam, **M.CAMERA_MOVES[move]), p)
        gc = gb.download()[1:4]
        gb.free()
        _cases[key] = (prev_cam, rest, moved, gp, gc)
    return _cases[key]


# The bounds on out and length are pt_temporal's, for the same arithmetic class (binary32 against binary64 tap sums).  Motion: both
# sides perform the same binary32 operations, and 4 ulp of the largest coordinate leave room for last-place differences in the
# division and the square root.  Every case prints its figures.
@pytest.mark.parametrize("name,W,H", M.CASES)
@pytest.mark.parametrize("move", list(M.CAMERA_MOVES))
@pytest.mark.parametrize("pset", list(PARAM_SETS))
def test_equals_the_reference(t, name, W, H, move, pset):
    prev_cam, rest, moved, gp, gc = case_guides(t, name, W, H, move)
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    n = len(rest)
    out, length, rgba, motion = motion_gpu(t, W, H, prev_cam, (rest, moved, n), (prev, ln, *gp), (cur, *gc), **PARAM_SETS[pset])
    ref, ref_len, ref_motion, fragile, acc = M.temporal_motion(W, H, prev_cam, rest, moved, n, prev, ln, *gp, cur, *gc, **params(**PARAM_SETS[pset]))
    was_moved = M.where_it_was(rest, moved, n, *gc)[3]
    ok = ~fragile
    d_out, d_len = float(np.abs(out - ref)[ok].max(initial=0)), float(np.abs(length - ref_len)[ok].max(initial=0))
    d_mo = float(np.abs(motion - ref_motion)[ok].max(initial=0))
    share = float(acc[was_moved].mean()) if was_moved.any() else 0.0
    print(f"motion {name} {W}x{H} {move} {pset}: |out-ref| {d_out:.3g} |len-ref| {d_len:.3g} |motion-ref| {d_mo:.3g} fragile {fragile.mean():.4f} "
          f"moved pixels {was_moved.mean():.3f}, accepted of them {share:.3f}")
    assert d_out <= 1e-4, d_out
    assert d_len <= 1e-3, d_len
    assert d_mo <= 4 * 2.0 ** -23 * max(W, H), d_mo
    assert np.array_equal(rgba, R.pack_rgba(out))
    assert fragile.mean() <= FRAGILE_MAX, float(fragile.mean())
    if pset == "history1":
        assert np.all(length == 1)
    if W >= 37 and pset != "plane0":
        assert was_moved.mean() > 0.1 and share > 0.5, (float(was_moved.mean()), share)   # else the case tests nothing


# ---------------------------------------------------------------------------------------------------- the room: spheres, unmoved mesh
_room = {}


def room_guides(t, W, H, twisted):
    """The sphere room from the golden camera and from a camera panned 2 degrees: (prev_cam, soup, soup of the current frame,
    previous guides, current guides).  twisted: the mesh is refit to its twist before the current guides are rendered."""
    key = (W, H, twisted)
    if key not in _room:
        setup_scene(t, "room", False)
        soup = g.scene_mesh("cornell").triangle_soup()
        cur_soup = twist(soup, 0.2, (0.01, 0.0, 0.0)) if twisted else soup
        prev_cam, p = golden_camera(W, H), g.default_params(W, H)
        gb = Guides(t, W, H)
        gb.render(prev_cam, p)
        gp = gb.download()[1:4]
        if twisted:
            t.refit_bvh(cur_soup)
        gb.render(T.moved(prev_cam, pan_deg=2.0), p)
        gc = gb.download()[1:4]
        gb.free()
        _room[key] = (prev_cam, soup, cur_soup, gp, gc)
    return _room[key]


@pytest.mark.parametrize("W,H", [(37, 23), (257, 131)])
def test_an_unmoved_mesh_is_pt_temporal_bit_for_bit(t, W, H):
    prev_cam, soup, _, gp, gc = room_guides(t, W, H, False)
    cur, prev, ln = random_frames(W, H, 31)
    ref = temporal_gpu(t, W, H, prev_cam, (prev, ln, *gp), (cur, *gc))
    assert (gc[2] <= -2).any() and (gc[2] >= 0).any() and (ref[1] > 1).mean() > 0.3
    for same in (True, False):   # one pointer for both vertex buffers, then two equal copies
        out, length, rgba, motion = motion_gpu(t, W, H, prev_cam, (soup, soup.copy(), len(soup)), (prev, ln, *gp), (cur, *gc), same_verts=same)
        assert np.array_equal(bits(out), bits(ref[0])) and np.array_equal(bits(length), bits(ref[1])) and np.array_equal(rgba, ref[2]), same
        assert np.abs(motion).max() > 0.5


def test_spheres_keep_pt_temporal_s_bits_beside_a_twisted_mesh(t):
    W, H = 257, 131
    prev_cam, soup, cur_soup, gp, gc = room_guides(t, W, H, True)
    cur, prev, ln = random_frames(W, H, 32)
    ref = temporal_gpu(t, W, H, prev_cam, (prev, ln, *gp), (cur, *gc))
    out, length, rgba, motion = motion_gpu(t, W, H, prev_cam, (soup, cur_soup, len(soup)), (prev, ln, *gp), (cur, *gc))
    sph = gc[2] <= -2
    assert sph.mean() > 0.05 and (length[sph] > 1).mean() > 0.3
    assert np.array_equal(bits(out[sph]), bits(ref[0][sph])) and np.array_equal(bits(length[sph]), bits(ref[1][sph]))
    assert np.array_equal(rgba[sph], ref[2][sph])
    tri = gc[2] >= 0
    assert tri.any() and not np.array_equal(bits(out[tri]), bits(ref[0][tri]))   # (the mesh did move)


# ---------------------------------------------------------------------------------------------------- rows, buffers
def test_rows_past_n_tris_are_not_read_and_take_no_history(t):
    """n_tris = half the real count, the full vertex buffers behind it: pixels whose id >= n_tris are bit copies of cur with
    length 1 and motion 0, the others equal the full-count call.  (No id points outside the allocations.)"""
    name, W, H = "bunny_low", 257, 131
    prev_cam, rest, moved, gp, gc = case_guides(t, name, W, H, "static")
    cur, prev, ln = random_frames(W, H, 33)
    n = len(rest)
    full = motion_gpu(t, W, H, prev_cam, (rest, moved, n), (prev, ln, *gp), (cur, *gc))
    half = motion_gpu(t, W, H, prev_cam, (rest, moved, n // 2), (prev, ln, *gp), (cur, *gc))
    past = gc[2] >= n // 2
    # (both kinds of pixel are there by the hundred, and the full-count call did give the pixels past the bound a history)
    assert past.sum() > 100 and (~past & (gc[2] >= 0)).sum() > 100 and (full[1][past] > 1).mean() > 0.5
    assert np.array_equal(bits(half[0][past]), bits(cur[past])) and np.all(half[1][past] == 1) and np.all(half[3][past] == 0)
    assert np.array_equal(half[2][past], R.pack_rgba(cur)[past])
    for a, b in zip(half, full):
        assert np.array_equal(bits(a[~past]), bits(b[~past]))
    none = motion_gpu(t, W, H, prev_cam, (rest, moved, 0), (prev, ln, *gp), (cur, *gc))   # n_tris = 0: no triangle has a history
    tri = gc[2] >= 0
    assert np.array_equal(bits(none[0][tri]), bits(cur[tri])) and np.all(none[1][tri] == 1)


@pytest.mark.parametrize("history", [True, False])
def test_aliasing_no_history_and_the_motion_buffer(t, history):
    name, W, H = "cube", 37, 23
    prev_cam, rest, moved, gp, gc = case_guides(t, name, W, H, "pan")
    cur, prev, ln = random_frames(W, H, 34)
    verts = (rest, moved, len(rest)) if history else None
    pv = (prev, ln, *gp) if history else None
    cam = prev_cam if history else None
    a = motion_gpu(t, W, H, cam, verts, pv, (cur, *gc))
    b = motion_gpu(t, W, H, cam, verts, pv, (cur, *gc), out_alias=True)
    c = motion_gpu(t, W, H, cam, verts, pv, (cur, *gc), with_motion=False, with_rgba=False)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[3]), bits(b[3]))
    assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(bits(a[1]), bits(c[1]))   # motion_dev NULL: the same out bits
    if history:
        assert not np.array_equal(a[0], cur) and np.abs(a[3]).max() > 0.5
    else:
        assert np.array_equal(bits(a[0]), bits(cur)) and np.all(a[1] == 1) and np.array_equal(a[2], R.pack_rgba(cur))
        assert np.all(a[3] == 0)


# ---------------------------------------------------------------------------------------------------- with pt_render
def blocks_scene(t, W, H):
    """cornell_box with its materials on the context; (mesh, camera, params, the soups of the quality sequence's poses)."""
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    soup0, blocks = mesh.triangle_soup(), M.block_rows(mesh)
    return mesh, cam, p, [M.quality_pose(soup0, blocks, k) for k in range(QUALITY_FRAMES)]


def test_chain_needs_no_host_sync(t):
    """refit_bvh -> launch_kernel -> render_aux -> temporal_motion -> denoise back to back, twice (the second frame has a
    history and moved blocks), equals the same calls with a host sync between every two."""
    W, H = 320, 240
    mesh, cam, p, soups = blocks_scene(t, W, H)
    n = len(soups[0])
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    t.set_option(g.OPT_OVERLAP, 1)
    results = []
    try:
        for sync in (False, True):
            acc, rg = t.alloc_frame(W, H)
            out, orgba, mo = t.malloc(W * H * 12), t.malloc(W * H * 4), t.malloc(W * H * 8)
            verts = [t.malloc(soups[0].nbytes) for _ in range(2)]
            verts[0].upload(soups[0])
            verts[1].upload(soups[3])   # the blocks 6 degrees on
            th = g.TemporalHistory(t, W, H)
            t.sync()
            maybe = t.sync if sync else (lambda: None)
            for k in range(2):
                t.refit_bvh(verts[k], n)
                maybe()
                for s in range(3):   # several calls in a row: the later ones run their path kernels on a side stream
                    q = g.Params.from_buffer_copy(p)
                    q.frame, q.sample_index, q.flags = 40 + 3 * k + s, 1 + s, g.FLAG_WRITE_RGBA
                    t.launch_kernel(acc.ptr, rg.ptr, cam, q, 1)
                    maybe()
                alb, nrm, pos, ids = th._ptrs(th.cur)
                hk = th.cur
                t.render_aux(cam, p, alb, nrm, pos, ids)
                maybe()
                if k == 0:
                    t.temporal_motion(W, H, None, None, None, 0, None, None, None, None, None, acc.ptr, nrm, pos, ids, th.color[hk].ptr,
                                      th.length[hk].ptr, None, mo.ptr)
                else:
                    _, pn, pp, pi = th._ptrs(1 - hk)
                    t.temporal_motion(W, H, cam, verts[0], verts[1], n, th.color[1 - hk].ptr, th.length[1 - hk].ptr, pn, pp, pi, acc.ptr, nrm,
                                      pos, ids, th.color[hk].ptr, th.length[hk].ptr, None, mo.ptr)
                th.cur = 1 - hk
                maybe()
                t.denoise(th.color[hk].ptr, alb, nrm, pos, W, H, out.ptr, orgba.ptr)
                maybe()
            t.sync()
            results.append((out.download(np.float32, (H, W, 3)), orgba.download(np.uint32, (H, W)),
                            th.color[hk].download(np.float32, (H, W, 3)), th.length[hk].download(np.float32, (H, W)),
                            acc.download(np.float32, (H, W, 3)), mo.download(np.float32, (H, W, 2))))
            for b in [acc, rg, out, orgba, mo] + verts:
                b.free()
            th.free()
    finally:
        t.upload_tri_materials(None, None)
        t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    a, b = results
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert (a[3] > 1).mean() > 0.5 and not np.array_equal(a[2], a[4]) and not np.array_equal(a[0], a[2])   # history taken, filtered
    assert np.abs(a[5]).max() > 1.0   # the blocks' pixels moved


def test_quality_on_a_moving_mesh(t):
    """cornell_box 320x240, 8 frames of 4 spp from one camera while the two blocks turn 2 degrees a frame, through
    TemporalHistory.push(moved=...): the history is at least M.QUALITY_K_MOTION times closer (MSE) to 1024 spp of the last pose
    than the last frame alone, 0.8 x the gain of the numpy reference over oracle renders at 80x60 (tests/test_motion.py;
    DESIGN.md §10 f14).  Prints the gain and the accepted share."""
    W, H = 320, 240
    mesh, cam, p, soups = blocks_scene(t, W, H)
    n = len(soups[0])
    verts = [t.malloc(soups[0].nbytes) for _ in range(2)]
    ref_acc, rg = t.alloc_frame(W, H)
    q = g.Params.from_buffer_copy(p)
    verts[0].upload(soups[-1])
    t.refit_bvh(verts[0], n)
    for k in range(0, 1024, 64):
        q.frame, q.sample_index = k, 1 + k
        t.launch_kernel(ref_acc.ptr, rg.ptr, cam, q, 64)
    t.sync()
    acc, _rg = t.alloc_frame(W, H)
    th = g.TemporalHistory(t, W, H)
    for k in range(QUALITY_FRAMES):
        t.sync()   # (the upload below is a host copy: the push that read this buffer two frames ago has run)
        verts[k & 1].upload(soups[k])
        t.refit_bvh(verts[k & 1], n)
        q.frame, q.sample_index = (1 << 20) + QUALITY_SPP * k, 1
        t.launch_kernel(acc.ptr, rg.ptr, cam, q, QUALITY_SPP)
        th.push(cam, q, acc.ptr, moved=(verts[1 - (k & 1)].ptr, verts[k & 1].ptr, n) if k else (None, None, 0))
    t.sync()
    hk = 1 - th.cur
    ref, last = ref_acc.download(np.float32, (H, W, 3)), acc.download(np.float32, (H, W, 3))
    hist, length = th.color[hk].download(np.float32, (H, W, 3)), th.length[hk].download(np.float32, (H, W))
    ids = th.guides[hk][3].download(np.int32, (H, W))
    for b in [ref_acc, rg, acc, _rg] + verts:
        b.free()
    th.free()
    t.upload_tri_materials(None, None)
    on_blocks = np.isin(ids, np.concatenate(M.block_rows(mesh)))
    gain, accepted = R.mse(last, ref) / R.mse(hist, ref), float((length > 1)[on_blocks].mean())
    print(f"motion quality 320x240, {QUALITY_FRAMES} x {QUALITY_SPP} spp, blocks turning {M.QUALITY_TURN} deg: gain {gain:.2f}, "
          f"accepted on the blocks {accepted:.3f} ({on_blocks.mean():.3f} of the frame)")
    assert on_blocks.mean() > 0.1 and accepted > 0.9, accepted
    assert gain >= M.QUALITY_K_MOTION, gain


# ---------------------------------------------------------------------------------------------------- errors, side effects
def test_temporal_motion_errors():
    lib = g._abi.ptmi()
    W, H = 8, 8
    fresh = g.PathTracer(0)   # no scene needed
    try:
        bufs = [fresh.malloc(W * H * 16) for _ in range(14)]
        for b in bufs:
            b.zero()
        pv, cv, pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, mo = (b.ptr for b in bufs)
        cam = golden_camera(W, H)
        tp = g.TemporalParams(W, H, 32.0, 0.02, 0.9, 0)
        #      0             1              2   3   4  5   6   7   8   9   10  11  12  13  14  15  16    17
        ok = [C.byref(tp), C.byref(cam), pv, cv, 4, pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, None, mo]

        def call(args):
            return lib.pt_temporal_motion(fresh._ctx, *args)

        def bad(k, v=None):
            args = list(ok)
            args[k] = v
            return call(args)

        assert call(ok) == 0
        # everything pt_temporal refuses, in its order
        for k in (0, 10, 11, 12, 14, 15):        # params, cur colour / normal / position, out colour / length
            assert bad(k) == PT_ERR_INVALID, k
        nan, inf = float("nan"), float("inf")
        for wrong in ((1, H, 32, .02, .9), (W, 1, 32, .02, .9), (0, H, 32, .02, .9), (W, -4, 32, .02, .9), (W, H, 0.5, .02, .9), (W, H, nan, .02, .9),
                      (W, H, inf, .02, .9), (W, H, 32, -1e-3, .9), (W, H, 32, nan, .9), (W, H, 32, inf, .9), (W, H, 32, .02, 1.5),
                      (W, H, 32, .02, -1.5), (W, H, 32, .02, nan)):
            assert call([C.byref(g.TemporalParams(*wrong, 0))] + ok[1:]) == PT_ERR_INVALID, wrong
        for k in (1, 6, 7, 8):                   # with a history: its camera, lengths, normals, positions
            assert bad(k) == PT_ERR_INVALID, k
        assert bad(14, pc) == PT_ERR_INVALID     # the new history over the old one
        assert bad(15, pl) == PT_ERR_INVALID
        # what this call refuses beyond that
        for k in (9, 13):                        # either id pointer
            assert bad(k) == PT_ERR_INVALID, k
        args = list(ok)
        args[9] = args[13] = None                # ... or both: the ids choose the rows
        assert call(args) == PT_ERR_INVALID
        for k in (2, 3):                         # a vertex pointer, while n_tris > 0
            assert bad(k) == PT_ERR_INVALID, k
        assert bad(4, 1 << 31) == PT_ERR_INVALID and bad(4, (1 << 40) + 3) == PT_ERR_INVALID
        for k in (2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):   # motion over any input or output buffer
            assert bad(17, ok[k]) == PT_ERR_INVALID, k
        args = list(ok)
        args[16] = args[17] = mo                 # ... the display words included
        assert call(args) == PT_ERR_INVALID
        assert b"pt_temporal_motion" in lib.pt_last_error(fresh._ctx)
        # valid: no rows at all (with or without vertex pointers), one buffer for both poses, out over cur, no motion buffer
        args = list(ok)
        args[2] = args[3] = None
        args[4] = 0
        assert call(args) == 0 and bad(4, 0) == 0 and bad(3, pv) == 0 and bad(14, cc) == 0 and bad(17) == 0
        # no history: prev_cam, every prev_*, the vertex pointers and n_tris are ignored
        assert call([C.byref(tp), None, None, None, 1 << 40, None, None, None, None, None, cc, cn, cp, ci, oc, ol, None, mo]) == 0
        assert call([C.byref(tp), None, None, cv, 4, None, pl, None, None, pi, cc, cn, cp, None, oc, ol, None, None]) == 0
        for edge in ((2, 2, 1.0, 0.0, -1.0), (W, H, 32, .02, 1.0)):
            assert call([C.byref(g.TemporalParams(*edge, 0))] + ok[1:]) == 0, edge
        fresh.sync()
        for b in bufs:
            b.free()
        # the context still renders correctly
        W, H = 64, 64
        bvh, sph, _, _ = setup_scene(fresh, "room", False)
        cam, p = golden_camera(W, H), g.default_params(W, H)
        acc, rg = fresh.alloc_frame(W, H)
        fresh.launch_kernel(acc.ptr, rg.ptr, cam, p, 2)
        fresh.sync()
        ref, _, _ = orc.render(bvh, sph, cam, p, spp=2)
        assert np.array_equal(acc.download(np.float32, (H, W, 3)), ref)
        acc.free()
        rg.free()
    finally:
        fresh.close()


def test_pushes_with_moved_leave_no_trace_in_render(t):
    W, H = 257, 131
    bvh, sph, _, _ = setup_scene(t, "room", False)
    soup = g.scene_mesh("cornell").triangle_soup()
    cam, p = golden_camera(W, H), g.default_params(W, H)
    p.flags = g.FLAG_WRITE_RGBA

    def frame(tr):
        acc, rg = tr.alloc_frame(W, H)
        tr.launch_kernel(acc.ptr, rg.ptr, cam, p, 3)
        tr.sync()
        out = acc.download(np.float32, (H, W, 3)), rg.download(np.uint32, (H, W))
        acc.free()
        rg.free()
        return out

    th = g.TemporalHistory(t, W, H)
    acc, rg = t.alloc_frame(W, H)
    mo = t.malloc(W * H * 8)
    verts = [t.malloc(soup.nbytes) for _ in range(2)]
    verts[0].upload(soup)
    verts[1].upload(soup)   # (the vertex buffers are inputs of the history alone: the tree stays at rest)
    for k in range(2):
        c2 = T.moved(cam, pan_deg=2.0 * k)
        t.launch_kernel(acc.ptr, rg.ptr, c2, p, 3)
        th.push(c2, p, acc.ptr, rg.ptr, moved=(verts[1 - k].ptr, verts[k].ptr, len(soup)), motion_ptr=mo.ptr)
    t.sync()
    assert (th.length[1 - th.cur].download(np.float32, (H, W)) > 1).mean() > 0.5
    assert np.abs(mo.download(np.float32, (H, W, 2))).max() > 0.5
    for b in [acc, rg, mo] + verts:
        b.free()
    th.free()
    after = frame(t)
    clean = g.PathTracer(0)
    try:
        clean.upload_bvh(bvh)
        clean.upload_spheres(sph)
        b = frame(clean)
    finally:
        clean.close()
    assert np.array_equal(bits(after[0]), bits(b[0])) and np.array_equal(after[1], b[1])


def test_temporal_motion_timing(t):
    name, W, H = "bunny_low", 257, 131
    prev_cam, rest, moved, gp, gc = case_guides(t, name, W, H, "pan")
    t.set_option(g.OPT_TIMING, 1)
    try:
        cur, prev, ln = random_frames(W, H, 8)
        motion_gpu(t, W, H, prev_cam, (rest, moved, len(rest)), (prev, ln, *gp), (cur, *gc))
        assert 0 < t.last_kernel_ms() < 5.0
    finally:
        t.set_option(g.OPT_TIMING, 0)


def test_pt_app_spin_deg(tmp_path):
    """--spin-deg 0 issues no refit: --out is byte-identical to a plain run.  --spin-deg 3 with --temporal-out writes both
    files, which differ from each other and from the plain run.  The combinations --pan-deg refuses are refused."""
    app = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
    base = [app, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "120", "--frames", "8", "--spp", "2"]

    def run(name, extra):
        img = tmp_path / f"{name}.png"
        r = subprocess.run(base + ["--out", str(img)] + extra, capture_output=True, text=True, timeout=300)
        return r, img

    r, plain = run("plain", [])
    assert r.returncode == 0, r.stderr[-500:]
    r, still = run("still", ["--spin-deg", "0"])
    assert r.returncode == 0, r.stderr[-500:]
    assert still.read_bytes() == plain.read_bytes()
    r, spin = run("spin", ["--spin-deg", "3", "--temporal-out", str(tmp_path / "t_spin.png")])
    assert r.returncode == 0, r.stderr[-500:]
    tspin = (tmp_path / "t_spin.png").read_bytes()
    assert tspin[:8] == b"\x89PNG\r\n\x1a\n" and tspin != spin.read_bytes() and spin.read_bytes() != plain.read_bytes()
    assert tspin != plain.read_bytes()
    r, alone = run("alone", ["--spin-deg", "3"])   # motion alone: the last frame, the same with or without --temporal-out
    assert r.returncode == 0 and alone.read_bytes() == spin.read_bytes()
    for extra in (["--resume", str(tmp_path / "none.ckpt")], ["--checkpoint", str(tmp_path / "c.ckpt")],
                  ["--until-error", "0.1", "--max-frames", "16"], ["--equirect"]):
        r, _ = run("refused", ["--spin-deg", "3"] + extra)
        assert r.returncode != 0 and "--spin-deg" in r.stderr, extra
    r, _ = run("refused", ["--spin-deg", "nan"])
    assert r.returncode != 0
    assert not (tmp_path / "c.ckpt").exists()
