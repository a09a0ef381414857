"""CPU tests (no GPU) of pt_temporal_motion, the temporal reprojection for triangles moved by pt_refit_bvh: the call is declared,
bound and exported, and the CPU reference (tests/motion_ref.py) has the properties its contract promises — it is pt_temporal
where nothing moved, it follows a quad that slides, approaches or turns where pt_temporal drops or mistakes the history, it
rejects rows it cannot use, few pixels of a twisted mesh are fragile, and on a moving mesh its history is worth what
motion_ref.QUALITY_GAIN_MOTION_CPU says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import motion_ref as M
import temporal_ref as T
from gpu_support import bits, soup_mesh, turn_rows, twist
from scene_matrix import make_camera
from temporal_ref import FRAGILE_MAX, PARAM_SETS, QUALITY_FRAMES, QUALITY_SPP, params, random_frames

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ---------------------------------------------------------------------------------------------------- the ABI
def test_temporal_motion_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_temporal_motion\(pt_ctx\* ctx, const pt_temporal_params\* tp, const pt_camera\* prev_cam,\s+"
                     r"const float\* prev_verts_dev, const float\* cur_verts_dev, size_t n_tris,\s+"
                     r"const float\* prev_color_dev, const float\* prev_length_dev,\s+"
                     r"const float\* prev_normal_dev, const float\* prev_position_dev, const int32_t\* prev_id_dev,\s+"
                     r"const float\* cur_color_dev,\s+"
                     r"const float\* cur_normal_dev, const float\* cur_position_dev, const int32_t\* cur_id_dev,\s+"
                     r"float\* out_color_dev, float\* out_length_dev, uint32_t\* rgba_dev,\s+"
                     r"float\* motion_dev /\* float\[h\]\[w\]\[2\], may be NULL \*/\);", hdr)
    assert "#define PTMI_ABI_VERSION 3" in hdr
    names = {n for n, _, _ in g._abi.PTMI_SYMBOLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    assert "pt_temporal_motion" in names and hasattr(g._abi.ptmi(), "pt_temporal_motion")
    assert re.search(r" T pt_temporal_motion$", out, re.M)
    lib = g._abi.ptmi()
    assert lib.pt_abi_version() == 3     # functions are only added
    tp = g.TemporalParams(8, 8, 32.0, 0.02, 0.9, 0)
    assert lib.pt_temporal_motion(None, C.byref(tp), None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None,
                                  None, None) == -1
    assert b"null ctx" in lib.pt_last_error(None)
    assert hasattr(g.PathTracer, "temporal_motion")


# ---------------------------------------------------------------------------------------------------- a quad facing the camera
QUAD_D = 10.0


def quad_camera(W, H):
    cam = g.default_camera(W, H)
    cam.dist = 1.0
    return cam


def quad(x0, x1, y0, y1, z=-QUAD_D):
    """Two triangles, front towards +z (the camera at the origin looks along -z)."""
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return np.array([a + b + c, a + c + d], np.float32)


def run_both(W, H, cam, prev_soup, cur_soup, cur, prev, ln, n_tris=None, **kw):
    """(guides of the previous pose, guides of the current pose, motion_ref's result, temporal_ref's result) of one camera."""
    gp, gc = M.brute_guides(prev_soup, cam, W, H), M.brute_guides(cur_soup, cam, W, H)
    n = len(cur_soup) if n_tris is None else n_tris
    mo = M.temporal_motion(W, H, cam, prev_soup, cur_soup, n, prev, ln, *gp, cur, *gc, **params(**kw))
    st = T.temporal(W, H, cam, prev, ln, *gp, cur, *gc, **params(**kw))
    return gp, gc, mo, st


@pytest.mark.parametrize("W,H", [(37, 23), (33, 21)])
def test_equal_vertex_buffers_are_pt_temporal(W, H):
    """Nothing moved: motion_ref equals temporal_ref bit for bit, under a camera that moved as well as under one that did not."""
    prev_cam = quad_camera(W, H)
    soup = np.concatenate([quad(-4, 4, -3, 3), quad(-9, 0, -5, 1, -14.0)])
    cur, prev, ln = random_frames(W, H, 21)
    gp = M.brute_guides(soup, prev_cam, W, H)
    for cur_cam in (prev_cam, T.moved(prev_cam, pan_deg=2.0, side=0.3)):
        gc = M.brute_guides(soup, cur_cam, W, H)
        for kw in PARAM_SETS.values():
            for cv in (soup, soup.copy()):
                out, length, motion, fragile, acc = M.temporal_motion(W, H, prev_cam, soup, cv, len(soup), prev, ln, *gp, cur, *gc, **params(**kw))
                ref, ref_len, ref_fragile, ref_acc = T.temporal(W, H, prev_cam, prev, ln, *gp, cur, *gc, **params(**kw))
                assert np.array_equal(bits(out), bits(ref)) and np.array_equal(bits(length), bits(ref_len))
                assert np.array_equal(acc, ref_acc) and np.array_equal(fragile, ref_fragile)
    assert acc.mean() > 0.1 and np.abs(motion).max() > 0.5   # (the panned camera: history taken, and the pixels did move)


@pytest.mark.parametrize("k", [1, 3])
def test_a_quad_moved_by_k_pixel_footprints_shifts_the_history_by_k_pixels(k):
    """The sideways-camera test of test_temporal with the camera still and the surface moving: the quad slides along `right`
    by k footprints of a pixel, inside its own plane, so pt_temporal passes every test and takes the history of the surface
    point k pixels away; pt_temporal_motion takes the point's own."""
    W, H = 33, 21
    cam = quad_camera(W, H)
    foot = QUAD_D * cam.aspect * cam.fov / (W - 1)
    # larger than the view: every pixel lies on it in both frames; lopsided, so that its diagonal passes through no pixel centre
    prev_soup = quad(-20.3, 21.1, -12.7, 13.9)
    cur_soup = prev_soup.copy()
    cur_soup[:, 0::3] += np.float32(k * foot)
    rng = np.random.default_rng(5)
    cur, prev = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2))
    ln = np.ones((H, W), np.float32)
    gp, gc, (out, length, motion, fragile, acc), (s_out, s_len, _, s_acc) = run_both(W, H, cam, prev_soup, cur_soup, cur, prev, ln)
    xs = np.arange(W)
    inside = xs - k >= 0
    # the current pixel x shows the surface point the previous pixel x - k showed; the diagonal between the two triangles moved
    # with the quad, so a pixel's triangle is the triangle of its point in the previous frame as well
    assert acc[:, inside].all()
    want = 0.5 * (prev[:, np.clip(xs - k, 0, W - 1)].astype(np.float64) + cur)
    assert np.abs(out - want)[:, inside].max() <= 1e-3      # fx is k off an integer by ~1e-5: the neighbour's share
    assert np.abs(length[:, inside] - 2).max() == 0
    assert np.abs(motion[..., 0] + k).max() <= 1e-3 and np.abs(motion[..., 1]).max() <= 1e-3
    gone = xs - k < -1
    assert np.array_equal(bits(out[:, gone]), bits(cur[:, gone])) and np.all(length[:, gone] == 1)
    # pt_temporal on the same inputs: accepted wherever the ids agree, with the history of the WRONG point (the pixel's own)
    same_id = gp[2] == gc[2]
    assert s_acc[same_id].all() and same_id.mean() > 0.7
    assert np.abs(s_out - 0.5 * (prev.astype(np.float64) + cur))[same_id].max() <= 1e-3


def test_a_quad_that_approaches_keeps_its_history():
    """The quad moves 10 % of its distance towards the camera: every point leaves its old tangent plane by half the distance it
    is seen from times 0.1 / 0.9, far more than plane_tolerance, so pt_temporal drops all of it; pt_temporal_motion keeps at least
    0.9 of the pixels that lie on the quad in both frames."""
    W, H = 33, 21
    cam = quad_camera(W, H)
    prev_soup = quad(-4, 4, -3, 3)
    cur_soup = prev_soup.copy()
    cur_soup[:, 2::3] += np.float32(0.1 * QUAD_D)
    cur, prev, ln = random_frames(W, H, 22)
    gp, gc, (out, length, motion, fragile, acc), (s_out, s_len, _, s_acc) = run_both(W, H, cam, prev_soup, cur_soup, cur, prev, ln)
    both = (gp[2] >= 0) & (gc[2] >= 0)
    cols, rows = int(both.any(0).sum()), int(both.any(1).sum())
    # at least 12 pixels across, so that the pixels along the border and the diagonal — the only ones whose taps can all fall on a
    # miss or on the other triangle — cannot add up to the 10 % the bar below allows
    assert cols >= 12 and rows >= 12, (cols, rows)
    assert not s_acc[both].any()
    share = float(acc[both].mean())
    print(f"approaching quad: {int(both.sum())} pixels on it in both frames ({cols} x {rows}), motion accepts {share:.3f}, temporal 0")
    assert share >= 0.9, share
    assert np.array_equal(bits(s_out[both]), bits(cur[both]))
    # a point moves towards the image centre when seen from further away
    xs = np.arange(W) - (W - 1) / 2.0
    m = both & acc
    assert np.all((motion[..., 0] * xs)[m] <= 0) and np.abs(motion[m]).max() > 0.3


def turned(tri, deg):
    return turn_rows(tri, np.arange(len(tri)), deg, (0.0, 0.0, 0.0))


def test_a_turned_triangle_keeps_its_history_unless_it_showed_its_other_face():
    W, H = 33, 21
    cam = quad_camera(W, H)
    rest = np.array([[-5, -4, -QUAD_D, 5, -4, -QUAD_D, 0, 5, -QUAD_D]], np.float32)
    cur, prev, ln = random_frames(W, H, 23)
    # 30 degrees about `up`: the normals are cos 30 = 0.866 < 0.9 apart, pt_temporal sees another surface
    gp, gc, (out, length, motion, fragile, acc), (_, _, _, s_acc) = run_both(W, H, cam, rest, turned(rest, 30.0), cur, prev, ln, normal_threshold=0.9)
    both = (gp[2] >= 0) & (gc[2] >= 0)
    assert both.sum() > 40 and acc[both].mean() > 0.8, (int(both.sum()), float(acc[both].mean()))
    assert not s_acc[both].any()
    assert np.all(length[both & acc] > 1)
    # 150 degrees: the previous frame saw the triangle's other face, whose normal looks the other way — no history for either
    gp, gc, (out, length, motion, fragile, acc), (s_out, _, _, s_acc) = run_both(W, H, cam, turned(rest, 150.0), rest, cur, prev, ln, normal_threshold=0.9)
    both = (gp[2] >= 0) & (gc[2] >= 0)
    assert both.sum() > 40 and not acc.any() and not s_acc[both].any()
    assert np.array_equal(bits(out), bits(cur)) and np.all(length == 1)
    assert np.abs(motion[both]).max() > 0   # the projection itself did not reject: the motion is still reported


def test_rows_that_cannot_be_used_reject_the_history():
    """A previous row of zero area, a previous row holding a NaN, an id >= n_tris: out = cur bit for bit, length 1, on every pixel
    of that triangle; the other triangle of the quad keeps its history."""
    W, H = 33, 21
    cam = quad_camera(W, H)
    cur_soup = quad(-4, 4, -3, 3)
    cur, prev, ln = random_frames(W, H, 24)
    shifted = cur_soup.copy()
    shifted[:, 0::3] += np.float32(0.25)
    flat, nan = shifted.copy(), shifted.copy()
    flat[1, 3:6] = flat[1, 0:3]                    # v1 = v0: no area
    nan[1, 4] = np.nan
    gp = M.brute_guides(shifted, cam, W, H)        # what the previous frame showed (the bad row was drawn from its good twin)
    gc = M.brute_guides(cur_soup, cam, W, H)
    on0, on1 = gc[2] == 0, gc[2] == 1
    assert on0.sum() > 20 and on1.sum() > 20
    for name, pv, n in (("zero area", flat, 2), ("nan", nan, 2), ("id >= n_tris", shifted, 1)):
        out, length, motion, fragile, acc = M.temporal_motion(W, H, cam, pv, cur_soup, n, prev, ln, *gp, cur, *gc, **params())
        assert not acc[on1].any() and np.all(length[on1] == 1) and np.array_equal(bits(out[on1]), bits(cur[on1])), name
        assert np.all(motion[on1] == 0), name
        assert acc[on0].mean() > 0.8, name
    # a current row of zero area cannot be hit, but a caller's stale buffer may hold one: rejected just the same
    flat_cur = cur_soup.copy()
    flat_cur[1, 6:9] = flat_cur[1, 0:3]
    out, length, motion, fragile, acc = M.temporal_motion(W, H, cam, shifted, flat_cur, 2, prev, ln, *gp, cur, *gc, **params())
    assert not acc[on1].any() and np.array_equal(bits(out[on1]), bits(cur[on1]))


# ---------------------------------------------------------------------------------------------------- a real mesh, twisted
TWIST = (0.35, (0.01, 0.0, 0.005))    # gpu_support.twist's amount and shift (x the extent) for bunny_low


def bunny_camera(W, H):
    return make_camera(W, H, pos=(-1.0, 5.0, 19.0), front=(0.0, 0.0, -1.0), fov=0.75, dist=1.0)


_bunny = {}


def bunny_inputs(W, H):
    if (W, H) not in _bunny:
        soup = g.scene_mesh("bunny_low").triangle_soup()
        moved = twist(soup, *TWIST)
        cam = bunny_camera(W, H)
        _bunny[(W, H)] = (cam, soup, moved, M.brute_guides(soup, cam, W, H), M.brute_guides(moved, cam, W, H))
    return _bunny[(W, H)]


@pytest.mark.parametrize("W,H", [(37, 23), (257, 131)])
def test_few_pixels_of_a_twisted_mesh_are_fragile(W, H):
    cam, soup, moved, gp, gc = bunny_inputs(W, H)
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    on_mesh = gc[2] >= 0
    assert on_mesh.mean() > 0.15
    for name, kw in PARAM_SETS.items():
        out, length, motion, fragile, acc = M.temporal_motion(W, H, cam, soup, moved, len(soup), prev, ln, *gp, cur, *gc, **params(**kw))
        print(f"twisted bunny_low {W}x{H} {name}: fragile {fragile.mean():.4f}, accepted on the mesh {acc[on_mesh].mean():.3f}")
        assert fragile.mean() <= FRAGILE_MAX, (name, float(fragile.mean()))
        if name != "plane0" and W > 100:   # (at 37x23 a triangle of this mesh is smaller than a pixel: few taps share the pixel's id)
            assert acc[on_mesh].mean() > 0.5, (name, float(acc[on_mesh].mean()))


# ---------------------------------------------------------------------------------------------------- quality
def quality_sequence(W, H, render, guides, temporal):
    """QUALITY_FRAMES frames of QUALITY_SPP samples of cornell_box from one camera while its two blocks turn M.QUALITY_TURN degrees
    a frame.  render(k, params, spp) -> colour of pose k, guides(k, params) -> (normal, position, id),
    temporal(k, prev, cur) -> (history, length, accepted) with prev = (history, length, guides) or None.  Returns (gain, accepted
    share of the last frame on the blocks' pixels)."""
    mesh, _, cam, p = R.cornell_box_scene(W, H)
    blocks = np.concatenate(M.block_rows(mesh))
    last = QUALITY_FRAMES - 1
    p.frame = 0
    ref = render(last, p, 1024)
    prev = None
    for k in range(QUALITY_FRAMES):
        p.frame = (1 << 20) + QUALITY_SPP * k
        cur = render(k, p, QUALITY_SPP)
        gc = guides(k, p)
        hist, ln, acc = temporal(k, prev, (cur, gc))
        prev = (hist, ln, gc)
    on_blocks = np.isin(gc[2], blocks)
    return R.mse(cur, ref) / R.mse(hist, ref), float(acc[on_blocks].mean())


def test_reference_gains_on_a_moving_mesh():
    """8 frames of 4 spp of cornell_box at 80x60, the blocks turning 2 degrees a frame (oracle renders over a host tree per
    frame): the gain of motion_ref's history and of temporal_ref's over the same frames, both against 1024 spp of the last pose,
    are the constants of motion_ref within 2 %."""
    W, H = 80, 60
    mesh, _, cam, _ = R.cornell_box_scene(W, H)
    soup0, blocks = mesh.triangle_soup(), M.block_rows(mesh)
    soups = [M.quality_pose(soup0, blocks, k) for k in range(QUALITY_FRAMES)]
    bvhs = [g.Bvh(soup_mesh(s)) for s in soups]
    renders, guide_sets = {}, {}

    def render(k, p, spp):
        key = (k, spp)
        if key not in renders:
            renders[key] = orc.render(bvhs[k], None, cam, p, spp, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)[0]
        return renders[key]

    def guides(k, p):
        if k not in guide_sets:
            guide_sets[k] = R.guides(bvhs[k], None, cam, p, mesh.materials, mesh.tri_material)[1:4]
        return guide_sets[k]

    def with_motion(k, prev, cur):
        if prev is None:
            out, ln, _, _, acc = M.temporal_motion(W, H, None, None, None, 0, None, None, None, None, None, cur[0], *cur[1], **g.TEMPORAL_DEFAULTS)
        else:
            out, ln, _, _, acc = M.temporal_motion(W, H, cam, soups[k - 1], soups[k], len(soup0), prev[0], prev[1], *prev[2], cur[0], *cur[1],
                                                   **g.TEMPORAL_DEFAULTS)
        return out, ln, acc

    def static(k, prev, cur):
        if prev is None:
            out, ln, _, acc = T.temporal(W, H, None, None, None, None, None, None, cur[0], *cur[1], **g.TEMPORAL_DEFAULTS)
        else:
            out, ln, _, acc = T.temporal(W, H, cam, prev[0], prev[1], *prev[2], cur[0], *cur[1], **g.TEMPORAL_DEFAULTS)
        return out, ln, acc

    gain_m, acc_m = quality_sequence(W, H, render, guides, with_motion)
    gain_s, acc_s = quality_sequence(W, H, render, guides, static)
    print(f"moving blocks 80x60: motion gain {gain_m:.3f} (accepted on the blocks {acc_m:.3f}), temporal gain {gain_s:.3f} (accepted {acc_s:.3f})")
    assert abs(gain_m - M.QUALITY_GAIN_MOTION_CPU) <= 0.02 * M.QUALITY_GAIN_MOTION_CPU, gain_m
    assert abs(gain_s - M.QUALITY_GAIN_STATIC_CPU) <= 0.02 * M.QUALITY_GAIN_STATIC_CPU, gain_s
    assert acc_m > acc_s
