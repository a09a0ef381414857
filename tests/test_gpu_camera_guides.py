"""GPU tests of pt_render_aux_camera and pt_temporal_camera (contract in include/ptmi.h): the guide buffers and
the temporal reprojection of the five camera models.

The pinhole is pinned bit for bit to pt_render_aux, the pinhole and the thin lens to pt_temporal / pt_temporal_motion.  The guides of
every model are judged by the oracle's walk over the rows pt_camera_rays writes (tests/camera_guides_ref.py); the projections by the
float64 inverses of tests/camera_ref.py, within the pixel bound of tests/test_gpu_camera.py; the blend by steps 3 to 5 of pt_temporal
restated over the device's own coordinates.  tests/test_camera_guides.py checks the premises on the CPU."""
import ctypes as C

import numpy as np
import pytest

import camera_guides_ref as G
import camera_ref as cr
import denoise_ref as R
import gpu_pathtracer_amd as g
import motion_ref as M
import temporal_ref as T
from camera_guides_ref import PIXEL_BOUND
from gpu_support import bits, compare_guides, cornell_dragon_moved, golden_camera, setup_scene, soup_mesh
from scene_matrix import make_camera
from temporal_ref import FRAGILE_MAX, MOVES, QUALITY_FRAMES, QUALITY_PAN, QUALITY_SPP, params, random_frames

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_NO_SCENE, PT_ERR_UNSUPPORTED = -1, -3, -5
# the two calls under test: every test of this file, the premises included, stands on them (a library without them fails here)
CALLS = (g._abi.ptmi().pt_render_aux_camera, g._abi.ptmi().pt_temporal_camera)


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


def test_error_codes_are_the_headers():
    src = open(__file__.replace("tests/test_gpu_camera_guides.py", "include/ptmi.h")).read()
    for name, code in (("PT_ERR_INVALID", PT_ERR_INVALID), ("PT_ERR_NO_SCENE", PT_ERR_NO_SCENE), ("PT_ERR_UNSUPPORTED", PT_ERR_UNSUPPORTED)):
        assert f"{name} = {code}" in src.replace("  ", " "), name


# ---------------------------------------------------------------------------------------------------- launches over host arrays
class Bufs:
    """Device buffers of one call, freed together."""

    def __init__(self, t):
        self.t, self.all = t, []

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = self.t.malloc(max(a.nbytes, 4))
        b.upload(a)
        self.all.append(b)
        return b.ptr

    def new(self, nbytes, fill=None):
        b = self.t.malloc(nbytes)
        if fill is not None:
            b.upload(np.full(nbytes // 4, fill, np.float32))
        self.all.append(b)
        return b

    def free(self):
        for b in self.all:
            b.free()


def aux_gpu(t, cam, cm, p, which="camera", with_ids=True):
    """pt_render_aux_camera (or pt_render_aux) into fresh buffers: (albedo, normal, position, id); without ids the id buffer keeps
    the pattern it was filled with."""
    W, H = cm.width, cm.height
    B = Bufs(t)
    alb, nrm, pos = (B.new(W * H * 16, 7.0) for _ in range(3))
    ids = B.new(W * H * 4)
    ids.upload(np.full(W * H, 0x5A5A5A5A, np.int32))
    if which == "camera":
        t.render_aux_camera(cam, cm, p, alb.ptr, nrm.ptr, pos.ptr, ids.ptr if with_ids else None)
    else:
        t.render_aux(cam, p, alb.ptr, nrm.ptr, pos.ptr, ids.ptr if with_ids else None)
    t.sync()
    out = (alb.download(np.float32, (H, W, 4)), nrm.download(np.float32, (H, W, 4)), pos.download(np.float32, (H, W, 4)),
           ids.download(np.int32, (H, W)))
    B.free()
    return out


def centre_rows(t, cam, cm):
    """The rows of pt_camera_rays(PT_CAMF_CENTRE, lens_radius 0) for the model's whole image."""
    c = g._abi.CameraModel.from_buffer_copy(cm)
    c.flags, c.lens_radius = g.CAMF_CENTRE, 0.0
    n = c.width * c.height
    buf = t.malloc(32 * n)
    t.camera_rays(cam, c, 7, buf.ptr, n)
    t.sync()
    rows = buf.download(np.float32, (n, 8))
    buf.free()
    return rows


def temporal_camera_gpu(t, W, H, prev_cam, prev_cm, prev, cur, verts=None, with_motion=True, call="camera", **kw):
    """pt_temporal_camera over host arrays — or, for the comparisons, pt_temporal (call="temporal") / pt_temporal_motion
    (call="motion") over the same ones.  prev = (color, length, normal, position, id or None) or None, cur = (color, normal, position,
    id or None), verts = (prev soup, cur soup, n_tris) or None.  Returns (out, length, rgba, motion or None)."""
    B = Bufs(t)
    dprev = [B.up(a) for a in prev] if prev is not None else [None] * 5
    dcur = [B.up(a) for a in cur]
    pv = cv = None
    n = 0
    if verts is not None:
        pv, cv, n = B.up(np.asarray(verts[0], np.float32)), B.up(np.asarray(verts[1], np.float32)), verts[2]
    do, dl, dr = B.new(W * H * 12, 77.0), B.new(W * H * 4, 77.0), B.new(W * H * 4, 77.0)
    dm = B.new(W * H * 8, 77.0) if with_motion else None   # every pixel must be written
    mp = dm.ptr if dm else None
    if call == "camera":
        t.temporal_camera(W, H, prev_cam, prev_cm, *dprev, *dcur, do.ptr, dl.ptr, dr.ptr, mp, prev_verts=pv, cur_verts=cv, n_tris=n, **params(**kw))
    elif call == "motion":
        t.temporal_motion(W, H, prev_cam, pv, cv, n, *dprev, *dcur, do.ptr, dl.ptr, dr.ptr, mp, **params(**kw))
    else:
        t.temporal(W, H, prev_cam, *dprev, *dcur, do.ptr, dl.ptr, dr.ptr, **params(**kw))
    t.sync()
    out = (do.download(np.float32, (H, W, 3)), dl.download(np.float32, (H, W)), dr.download(np.uint32, (H, W)),
           dm.download(np.float32, (H, W, 2)) if dm else None)
    B.free()
    return out


_scene = [None]
_guides = {}


def scene(t, name, materials):
    """setup_scene once per (scene, table) in a row: (bvh, spheres, materials, tri_material)."""
    if _scene[0] is None or _scene[0][0] != (name, materials):
        _scene[0] = ((name, materials), setup_scene(t, name, materials))
    return _scene[0][1]


def model_guides(t, scene_name, materials, name, W, H, cam, cull=None):
    """The guides pt_render_aux_camera writes for a model of camera_guides_ref.MODELS, downloaded once per case."""
    key = (scene_name, materials, name, W, H, tuple(cam.pos), tuple(cam.front), cull)
    if key not in _guides:
        scene(t, scene_name, materials)
        p = g.default_params(W, H)
        if cull is not None:
            p.cull_backfaces = cull
        _guides[key] = aux_gpu(t, cam, G.camera_model(name, W, H), p)
    return _guides[key]


def same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None and y is None:
            continue
        assert np.array_equal(bits(x), bits(y)), f"{what}: output {k} differs in {int((bits(x) != bits(y)).sum())} words"


# ---------------------------------------------------------------------------------------------------- 1: the pinhole pin
@pytest.mark.parametrize("size", G.SIZES, ids=["64x48", "33x17"])
@pytest.mark.parametrize("cull", [0, 1], ids=["two-sided", "cull"])
@pytest.mark.parametrize("scene_name,materials", [("room", False), ("cornell_box", False), ("cornell_box", True)], ids=["room", "box", "box-table"])
def test_pinhole_is_pt_render_aux(t, scene_name, materials, cull, size):
    W, H = size
    scene(t, scene_name, materials)
    cam, p, cm = G.guide_camera(W, H), g.default_params(W, H), G.camera_model("pinhole", W, H)
    p.cull_backfaces = cull
    p.width, p.height = 5, 3   # not read: the image is the model's
    got = aux_gpu(t, cam, cm, p)
    p.width, p.height = W, H
    want = aux_gpu(t, cam, cm, p, which="aux")
    same_bits(got, want, f"pinhole {scene_name} {W}x{H}")
    assert (want[3] >= 0).any() and np.any(want[1] != 0)
    noid = aux_gpu(t, cam, cm, p, with_ids=False)
    same_bits(noid[:3], want[:3], "without ids")
    assert np.all(noid[3] == 0x5A5A5A5A), "id_dev NULL: no id is written"


# ---------------------------------------------------------------------------------------------------- 2: every model against the oracle
@pytest.mark.parametrize("scene_name,materials", [("room", False), ("cornell_box", True)], ids=["room", "box-table"])
@pytest.mark.parametrize("name,k", G.MODEL_CASES)
def test_models_against_the_oracle(t, name, scene_name, materials, k):
    W, H = G.size_of(name, k)
    bvh, sph, mats, tm = scene(t, scene_name, materials)
    cam, p, cm = G.guide_camera(W, H), g.default_params(W, H), G.camera_model(name, W, H)
    got = model_guides(t, scene_name, materials, name, W, H, cam)
    rows = centre_rows(t, cam, cm)
    ref = G.guides_from_rays(rows, bvh, sph, p, (H, W), mats, tm)
    du_p, du_n, ties = compare_guides(got, ref, f"{name} {scene_name} {W}x{H}")
    ids = got[3]
    print(f"{name} {scene_name} {W}x{H}: position {du_p} ulp, normal {du_n} ulp, ties {ties}, triangles {(ids >= 0).mean():.3f}, spheres {(ids <= -2).mean():.3f}")
    assert (ids >= 0).mean() > 0.05
    if scene_name == "room":
        assert (ids <= -2).any(), "the room shows sphere ids"
    has = np.any(rows[:, 4:7] != 0, axis=1).reshape(H, W)
    if G.MODELS[name][0] == cr.FISHEYE:
        assert 0 < (~has).sum() and np.all(ids[~has] == -1) and (ids[has] != -1).any()
        for b in got[:3]:
            assert not np.any(b[~has]), "a pixel outside the circle is a miss"
    else:
        assert has.all()
    if name == "thinlens":   # the aperture is range-checked and otherwise ignored; flags too
        for over in (dict(lens_radius=0.0), dict(lens_radius=0.5, centre=False)):
            cm0 = g.camera_model(cr.THIN_LENS, W, H, **{**dict(centre=True, focus_dist=35.0), **over})
            same_bits(aux_gpu(t, cam, cm0, p), got, f"thin lens {over}")


# ---------------------------------------------------------------------------------------------------- 3: pinhole and thin lens are pt_temporal
@pytest.mark.parametrize("ids", [True, False], ids=["ids", "no-ids"])
@pytest.mark.parametrize("name", ["pinhole", "thinlens"])
@pytest.mark.parametrize("size", G.SIZES, ids=["64x48", "33x17"])
def test_pinhole_and_thin_lens_reproject_as_pt_temporal(t, size, name, ids):
    W, H = size
    prev_cam = G.guide_camera(W, H)
    gp = model_guides(t, "room", False, name, W, H, prev_cam)
    gc = model_guides(t, "room", False, name, W, H, T.moved(prev_cam, **MOVES["pan"]))
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    pi, ci = (gp[3], gc[3]) if ids else (None, None)
    pv, cv = (prev, ln, gp[1], gp[2], pi), (cur, gc[1], gc[2], ci)
    cm = G.camera_model(name, W, H)
    want = temporal_camera_gpu(t, W, H, prev_cam, None, pv, cv, with_motion=False, call="temporal")
    got = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv, with_motion=False)
    same_bits(got, want, f"{name} {W}x{H}")
    assert (want[1] > 1).mean() > 0.3, "the history is taken"
    withm = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv)   # the motion buffer changes nothing else
    same_bits(withm[:3], want[:3], f"{name} {W}x{H} with motion")
    assert np.any(withm[3] != 0) and not np.any(withm[3] == 77.0)
    first = temporal_camera_gpu(t, W, H, None, None, None, cv)   # no history: out = cur, motion 0
    assert np.array_equal(bits(first[0]), bits(cur)) and np.all(first[1] == 1) and not np.any(first[3])


_dragon = {}


def dragon_camera(rest, W, H):
    """A camera 0.6 of the dragon's extent in front of it and a little above, looking at its centre: the dragon (the rows behind the
    box's) covers a tenth of a 180 degree fisheye's image and over half of the pinhole's."""
    n_box = g.Mesh.asset("cornell").n_tris
    v = rest[n_box:].reshape(-1, 3).astype(np.float64)
    c, ext = 0.5 * (v.min(0) + v.max(0)), float((v.max(0) - v.min(0)).max())
    pos = c + np.array([0.0, 0.2 * ext, 0.6 * ext])
    return make_camera(W, H, pos=tuple(pos), front=tuple(c - pos))


def dragon_guides(t, name, W, H):
    """(prev_cam, rest soup, moved soup, guides at rest, guides after the refit seen from a panned camera) of cornell_dragon built
    on the device from its soup (ids = rows), under a model."""
    if name not in _dragon:
        _, rest, moved = cornell_dragon_moved()
        prev_cam, p, cm = dragon_camera(rest, W, H), g.default_params(W, H), G.camera_model(name, W, H)
        t.upload_tri_materials(None, None)
        t.upload_spheres([])
        t.build_bvh(soup_mesh(rest))
        _scene[0] = None
        gp = aux_gpu(t, prev_cam, cm, p)
        t.refit_bvh(moved)
        gc = aux_gpu(t, T.moved(prev_cam, **MOVES["pan"]), cm, p)
        _dragon[name] = (prev_cam, rest, moved, gp, gc)
    return _dragon[name]


@pytest.mark.parametrize("name", ["pinhole", "thinlens"])
def test_pinhole_and_thin_lens_follow_rows_as_pt_temporal_motion(t, name):
    W, H = 64, 48
    prev_cam, rest, moved, gp, gc = dragon_guides(t, name, W, H)
    cur, prev, ln = random_frames(W, H, 9)
    pv, cv, n = (prev, ln, gp[1], gp[2], gp[3]), (cur, gc[1], gc[2], gc[3]), len(rest)
    cm = G.camera_model(name, W, H)
    for with_motion in (True, False):
        want = temporal_camera_gpu(t, W, H, prev_cam, None, pv, cv, verts=(rest, moved, n), with_motion=with_motion, call="motion")
        got = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv, verts=(rest, moved, n), with_motion=with_motion)
        same_bits(got, want, f"{name} rows motion={with_motion}")
    assert (want[1] > 1).mean() > 0.1, "the history is taken (the dragon fills half the frame and has moved far)"
    static = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv, with_motion=False)
    assert not np.array_equal(bits(static[0]), bits(want[0])), "the rows matter"


# ---------------------------------------------------------------------------------------------------- 4: a pixel projects onto itself
@pytest.mark.parametrize("name,k", G.MODEL_CASES)
def test_every_model_projects_a_pixel_onto_itself(t, name, k):
    """The guides' own camera and model as the previous ones: the motion of every hit pixel is 0 within PIXEL_BOUND per axis — the
    half-pixel conventions of the five inverses against the five forward models, no reference in between."""
    W, H = G.size_of(name, k)
    cam, cm = G.guide_camera(W, H), G.camera_model(name, W, H)
    gd = model_guides(t, "room", False, name, W, H, cam)
    cur, prev, ln = random_frames(W, H, 3)
    out, length, _, motion = temporal_camera_gpu(t, W, H, cam, cm, (prev, ln, gd[1], gd[2], gd[3]), (cur, gd[1], gd[2], gd[3]))
    hit = gd[3] != -1
    ys, xs = np.nonzero(hit)
    m = cr.Model.of(cam, cm)
    ex, ey = G.coord_error(m, xs + motion[ys, xs, 0].astype(np.float64), ys + motion[ys, xs, 1].astype(np.float64), xs.astype(np.float64), ys.astype(np.float64))
    print(f"{name} {W}x{H}: |mx| {ex.max():.3g} |my| {ey.max():.3g} over {hit.sum()} hit pixels, history on {(length[hit] > 1).mean():.3f}")
    assert ex.max() <= PIXEL_BOUND and ey.max() <= PIXEL_BOUND
    assert not np.any(motion[~hit]) and np.all(length[~hit] == 1)
    assert (length[hit] > 1).mean() > 0.9, "a surface seen from the same place keeps its history"


# ---------------------------------------------------------------------------------------------------- 5: a moved camera
@pytest.mark.parametrize("move", list(MOVES))
@pytest.mark.parametrize("name", G.MOVED_MODELS)
def test_moved_camera_against_the_reference(t, name, move):
    W, H = G.size_of(name)
    prev_cam = golden_camera(W, H)
    cur_cam = T.moved(prev_cam, **G.move_of(name, move))
    cm = G.camera_model(name, W, H)
    gp, gc = model_guides(t, "room", False, name, W, H, prev_cam), model_guides(t, "room", False, name, W, H, cur_cam)
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    out, length, rgba, motion = temporal_camera_gpu(t, W, H, prev_cam, cm, (prev, ln, gp[1], gp[2], gp[3]), (cur, gc[1], gc[2], gc[3]))
    m = cr.Model.of(prev_cam, cm)
    hit = gc[3] != -1
    pts = gc[2][..., 0:3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        rx, ry = (v.reshape(H, W) for v in G.project(m, pts))
    rejected, frag = (v.reshape(H, W) for v in G.rejects(m, pts))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy = (xs.astype(np.float32) + motion[..., 0]).astype(np.float32), (ys.astype(np.float32) + motion[..., 1]).astype(np.float32)
    # (a) the coordinates, wherever the reference does not reject; a rejected pixel is the current frame with motion 0
    seen = hit & ~rejected & ~frag
    ex, ey = G.coord_error(m, fx[seen], fy[seen], rx[seen], ry[seen])
    gone = hit & rejected & ~frag
    print(f"{name} {move}: |fx-ref| {ex.max(initial=0):.3g} |fy-ref| {ey.max(initial=0):.3g} over {seen.sum()} pixels, {gone.sum()} rejected, {frag.sum()} near a threshold")
    assert ex.max(initial=0) <= PIXEL_BOUND and ey.max(initial=0) <= PIXEL_BOUND
    assert not np.any(motion[gone]) and np.all(length[gone] == 1) and np.array_equal(bits(out[gone]), bits(cur[gone]))
    assert not np.any(motion[~hit]) and np.array_equal(bits(out[~hit]), bits(cur[~hit]))
    # (b) the blend over the device's own coordinates
    ref, ref_len, fragile, accepted = G.blend_from_coords(W, H, fx, fy, hit & ~rejected, prev, ln, gp[1], gp[2], gp[3], cur, gc[1], gc[2], gc[3], **params())
    fragile |= frag & hit
    ok = ~fragile
    d_out, d_len = float(np.abs(out - ref)[ok].max(initial=0)), float(np.abs(length - ref_len)[ok].max(initial=0))
    print(f"{name} {move}: |out-ref| {d_out:.3g} |len-ref| {d_len:.3g} fragile {fragile.mean():.4f} accepted {accepted.sum() / hit.sum():.3f} of the hit pixels")
    assert d_out <= 1e-4, d_out
    assert d_len <= 1e-3, d_len
    assert np.array_equal(rgba, R.pack_rgba(out))
    # (c) the two conditions of tests/test_camera_guides.py
    assert accepted.sum() >= 0.5 * hit.sum()
    assert fragile.mean() <= FRAGILE_MAX


# ---------------------------------------------------------------------------------------------------- 6: moved triangles, a fisheye
def test_moved_triangles_under_a_fisheye(t):
    W, H, name = 64, 48, "fisheye180"
    prev_cam, rest, moved, gp, gc = dragon_guides(t, name, W, H)
    cm, n = G.camera_model(name, W, H), len(rest)
    cur, prev, ln = random_frames(W, H, 10)
    pv, cv = (prev, ln, gp[1], gp[2], gp[3]), (cur, gc[1], gc[2], gc[3])
    rows = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv, verts=(rest, moved, n))
    static = temporal_camera_gpu(t, W, H, prev_cam, cm, pv, cv)
    ids = gc[3]
    same_row = np.ones(ids.shape, bool)
    tri = ids >= 0
    same_row[tri] = np.all(rest[ids[tri]].view(np.uint32) == moved[ids[tri]].view(np.uint32), axis=-1)
    assert 0.05 < (~same_row).mean() and 0.05 < (same_row & tri).mean(), "both kinds of pixels are in the frame"
    for k in range(4):
        assert np.array_equal(bits(rows[k][same_row]), bits(static[k][same_row])), f"an unmoved row has the bits of the call without rows (output {k})"
    x1, n1, was, mv, frag = M.where_it_was(rest, moved, n, gc[1], gc[2], ids)
    assert np.array_equal(mv, ~same_row)
    m = cr.Model.of(prev_cam, cm)
    rejected, frag2 = (v.reshape(H, W) for v in G.rejects(m, x1.reshape(-1, 3)))
    with np.errstate(all="ignore"):
        rx, ry = (v.reshape(H, W) for v in G.project(m, x1.reshape(-1, 3)))
    seen = mv & was & ~rejected & ~frag & ~frag2
    ys, xs = np.nonzero(seen)
    ex, ey = G.coord_error(m, xs + rows[3][ys, xs, 0].astype(np.float64), ys + rows[3][ys, xs, 1].astype(np.float64), rx[seen], ry[seen])
    print(f"fisheye rows: |fx-ref| {ex.max():.3g} |fy-ref| {ey.max():.3g} over {seen.sum()} moved pixels; history on {(rows[1][seen] > 1).mean():.3f} of them, "
          f"{(static[1][seen] > 1).mean():.3f} without rows")
    assert seen.sum() > 50 and ex.max() <= PIXEL_BOUND and ey.max() <= PIXEL_BOUND
    assert (rows[1][seen] > 1).mean() > (static[1][seen] > 1).mean(), "following the rows keeps more history on what moved"


# ---------------------------------------------------------------------------------------------------- 7: errors and order
def test_errors_of_both_calls():
    lib = g._abi.ptmi()
    W, H = 8, 8
    fresh = g.PathTracer(0)
    try:
        n = W * H
        bufs = [fresh.malloc(n * 16) for _ in range(14)]
        pattern = np.full(n * 4, 0x5A5A5A5A, np.uint32)

        def fill():
            for b in bufs:
                b.upload(pattern)

        def untouched():
            fresh.sync()
            return all(np.array_equal(b.download(np.uint32, (n * 4,)), pattern) for b in bufs)

        def refused(rc, code, word):
            msg = lib.pt_last_error(fresh._ctx)
            assert rc == code and word in msg, (rc, msg)
            assert untouched(), msg

        fill()
        cam, p = golden_camera(W, H), g.default_params(W, H)
        cm = G.camera_model("fisheye180", W, H)
        alb, nrm, pos, ids = (b.ptr for b in bufs[:4])

        def aux(cam_=cam, cm_=cm, p_=p, bufs_=(alb, nrm, pos, ids)):
            ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
            return lib.pt_render_aux_camera(fresh._ctx, ref(cam_), ref(cm_), ref(p_), *bufs_)

        # pt_render_aux_camera: the pointers and the model before the scene (there is none yet), then the scene
        refused(aux(cam_=None), PT_ERR_INVALID, b"null argument")
        refused(aux(cm_=None), PT_ERR_INVALID, b"null argument")
        refused(aux(p_=None), PT_ERR_INVALID, b"null argument")
        for k in range(3):
            refused(aux(bufs_=tuple(None if i == k else x for i, x in enumerate((alb, nrm, pos, ids)))), PT_ERR_INVALID, b"null argument")
        for over, word in ((dict(model=7), b"unknown camera model"), (dict(flags=6), b"unknown flag bits"), (dict(width=1), b"width and height must be >= 2"),
                           (dict(fisheye_fov=7.0), b"fisheye_fov"), (dict(model=cr.ORTHO, ortho_height=0.0), b"ortho_height"),
                           (dict(model=cr.THIN_LENS, lens_radius=-1.0, focus_dist=2.0), b"lens_radius")):
            bad = g._abi.CameraModel.from_buffer_copy(cm)
            for f, v in over.items():
                setattr(bad, f, v)
            refused(aux(cm_=bad), PT_ERR_INVALID, b"pt_render_aux_camera: " + word)
        refused(aux(), PT_ERR_NO_SCENE, b"pt_render_aux_camera: no BVH uploaded")
        fresh.upload_spheres(g.reference_spheres())
        refused(aux(), PT_ERR_NO_SCENE, b"no BVH uploaded")      # spheres alone are no scene for the walk
        fresh.set_option(g.OPT_TRI_TEST, 1)
        fresh.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        refused(aux(), PT_ERR_UNSUPPORTED, b"Moller-Trumbore")
        refused(aux(cm_=None), PT_ERR_INVALID, b"null argument")  # the order: pointers first
        fresh.set_option(g.OPT_TRI_TEST, 0)
        fresh.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        assert aux() == 0 and aux(bufs_=(alb, nrm, pos, None)) == 0
        fresh.sync()
        assert not untouched()

        # pt_temporal_camera
        fill()
        pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, rg, mo, vb = (b.ptr for b in bufs)
        tp = g.TemporalParams(W, H, 32.0, 0.02, 0.9, 0)
        ok = [C.byref(tp), C.byref(cam), C.byref(cm), None, None, 0, pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, rg, mo]

        def call(args):
            return lib.pt_temporal_camera(fresh._ctx, *args)

        def with_(**at):
            args = list(ok)
            for k, v in at.items():
                args[int(k[1:])] = v
            return args

        for k in (0, 11, 12, 13, 15, 16):        # params, cur colour / normal / position, out colour / length
            refused(call(with_(**{f"a{k}": None})), PT_ERR_INVALID, b"pt_temporal_camera: null argument")
        for k in (1, 7, 8, 9):                   # with a history: its camera, lengths, normals, positions
            refused(call(with_(**{f"a{k}": None})), PT_ERR_INVALID, b"a history needs its camera")
        refused(call(with_(a2=None)), PT_ERR_INVALID, b"a history needs the model of its camera")
        for over, word in ((dict(model=-1), b"unknown camera model"), (dict(model=5), b"unknown camera model"), (dict(flags=2), b"unknown flag bits"),
                           (dict(fisheye_fov=0.0), b"fisheye_fov"), (dict(width=W + 1), b"the model's image must be the parameters'"),
                           (dict(height=H - 1), b"the model's image must be the parameters'")):
            bad = g._abi.CameraModel.from_buffer_copy(cm)
            for f, v in over.items():
                setattr(bad, f, v)
            refused(call(with_(a2=C.byref(bad))), PT_ERR_INVALID, b"pt_temporal_camera: " + word)
        refused(call(with_(a10=None)), PT_ERR_INVALID, b"ids of both frames or of neither")
        refused(call(with_(a15=pc)), PT_ERR_INVALID, b"may not overwrite")
        refused(call(with_(a18=cn)), PT_ERR_INVALID, b"motion_dev may not be one of the other buffers")
        refused(call(with_(a3=vb, a4=vb, a5=4, a10=None, a14=None)), PT_ERR_INVALID, b"the ids of both frames are required")
        refused(call(with_(a3=vb, a5=4)), PT_ERR_INVALID, b"a null vertex buffer with n_tris > 0")
        refused(call(with_(a3=vb, a4=vb, a5=1 << 31)), PT_ERR_INVALID, b"n_tris must be < 2^31")
        refused(call(with_(a2=None, a0=None)), PT_ERR_INVALID, b"null argument")   # the order: the parameters before the history
        refused(call([C.byref(g.TemporalParams(W, 1, 32.0, 0.02, 0.9, 0))] + ok[1:]), PT_ERR_INVALID, b"width and height must be >= 2")
        assert untouched()
        # calls that pass: a history with and without ids, rows, no rows with an n_tris that is ignored, no history without a model
        for args in (ok, with_(a10=None, a14=None), with_(a3=vb, a4=vb, a5=4), with_(a5=1 << 40), with_(a18=None), with_(a15=cc),
                     with_(a1=None, a2=None, a6=None), with_(a1=None, a2=None, a6=None, a18=None)):
            fill()
            assert call(args) == 0, lib.pt_last_error(fresh._ctx)
            fresh.sync()
            assert not np.array_equal(bufs[10].download(np.uint32, (n * 4,)), pattern), "out_length is written"
        for b in bufs:
            b.free()
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------- 8: no trace
def test_the_two_calls_leave_no_trace_in_render(t):
    W, H = 257, 131
    bvh, sph, _, _ = scene(t, "room", False)
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

    before = frame(t)
    cm = G.camera_model("fisheye220", W, H)
    th = g.TemporalHistory(t, W, H)
    acc, rg = t.alloc_frame(W, H)
    mo = t.malloc(W * H * 8)
    for k in range(3):
        c2 = T.moved(cam, pan_deg=2.0 * k)
        t.render_model(c2, cm, p, acc.ptr, spp=2)
        th.push(c2, p, acc.ptr, rg.ptr, motion_ptr=mo.ptr, model=cm)
    t.sync()
    assert (th.length[1 - th.cur].download(np.float32, (H, W)) > 1).mean() > 0.3
    for b in (acc, rg, mo):
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
    for a in (before, after):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_timing_covers_both_calls(t):
    W, H = 64, 48
    scene(t, "room", False)
    cam, cm, p = G.guide_camera(W, H), G.camera_model("equirect", W, H), g.default_params(W, H)
    gd = model_guides(t, "room", False, "equirect", W, H, cam)
    t.set_option(g.OPT_TIMING, 1)
    try:
        aux_gpu(t, cam, cm, p)
        assert t.last_kernel_ms() > 0
        cur, prev, ln = random_frames(W, H, 8)
        temporal_camera_gpu(t, W, H, cam, cm, (prev, ln, gd[1], gd[2], gd[3]), (cur, gd[1], gd[2], gd[3]))
        assert t.last_kernel_ms() > 0
    finally:
        t.set_option(g.OPT_TIMING, 0)


# ---------------------------------------------------------------------------------------------------- 9: it does its job
def test_a_fisheye_frame_is_denoised_and_carried(t):
    """cornell_box 160x120 under a 180 degree fisheye, rendered by pt_render_camera in HDR.  (a) pt_denoise of a 4-spp frame with the
    new guides is closer (MSE) to 1024 spp than the frame itself; the three frames are compared in pt_denoise's output range [0, 1].
    (b) TemporalHistory.push(model=) over QUALITY_FRAMES frames of QUALITY_SPP samples panning QUALITY_PAN degrees is closer to 1024 spp
    at the last camera than the last frame alone.  Both bars are "better than doing nothing": gain > 1.  Measured: DESIGN.md §10 f20."""
    W, H = 160, 120
    mesh, bvh, cam0, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    _scene[0] = None
    cm = g.camera_model("fisheye", W, H, fisheye_fov=float(np.pi))
    cams = [T.moved(cam0, pan_deg=QUALITY_PAN * k) for k in range(QUALITY_FRAMES)]
    n = W * H
    ref_b, acc, den = t.malloc(n * 12), t.malloc(n * 12), t.malloc(n * 12)
    q = g.Params.from_buffer_copy(p)
    for k in range(0, 1024, 64):
        q.frame, q.sample_index = k, 1 + k
        t.render_model(cams[-1], cm, q, ref_b.ptr, spp=64, hdr=True)
    th = g.TemporalHistory(t, W, H)
    for k, cam in enumerate(cams):
        q.frame, q.sample_index = (1 << 20) + QUALITY_SPP * k, 1
        t.render_model(cam, cm, q, acc.ptr, spp=QUALITY_SPP, hdr=True)
        _, _, (alb, nrm, pos, _ids) = th.push(cam, q, acc.ptr, model=cm)
    t.denoise(acc.ptr, alb, nrm, pos, W, H, den.ptr)
    t.sync()
    hk = 1 - th.cur
    ref, last, dn = (b.download(np.float32, (H, W, 3)) for b in (ref_b, acc, den))
    hist, length = th.color[hk].download(np.float32, (H, W, 3)), th.length[hk].download(np.float32, (H, W))
    for b in (ref_b, acc, den):
        b.free()
    th.free()
    t.upload_tri_materials(None, None)
    clip = lambda a: np.clip(a, 0.0, 1.0)   # noqa: E731
    gain_d = R.mse(clip(last), clip(ref)) / R.mse(dn, clip(ref))
    gain_t, accepted = R.mse(last, ref) / R.mse(hist, ref), float((length > 1).mean())
    print(f"fisheye quality 160x120: denoise gain {gain_d:.2f} (4 spp against 1024); temporal gain {gain_t:.2f} over {QUALITY_FRAMES} x {QUALITY_SPP} spp, "
          f"pan {QUALITY_PAN} deg, history on {accepted:.3f} of the pixels")
    assert gain_d > 1.0, gain_d
    assert gain_t > 1.0, gain_t
