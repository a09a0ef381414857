"""CPU tests (no GPU) of the temporal reprojection extension: pt_temporal is declared, bound and exported with the header's struct
layout, argument checks come before any device call, and the CPU reference (tests/temporal_ref.py) has the properties its
contract promises — analytically on a plane facing the camera, on the real inputs the GPU tests use (how many pixels are
fragile), and as a quality gain on oracle renders of a panning camera."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import temporal_ref as T
from gpu_support import golden_camera
from temporal_ref import (ACCEPTED_MIN, FRAGILE_MAX, MOVES, PARAM_SETS, QUALITY_FRAMES, QUALITY_GAIN_CPU, QUALITY_PAN, QUALITY_SPP, params,
                          random_frames)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ---------------------------------------------------------------------------------------------------- the ABI
def test_temporal_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_temporal\(pt_ctx\* ctx, const pt_temporal_params\* tp, const pt_camera\* prev_cam,\s+"
                     r"const float\* prev_color_dev, const float\* prev_length_dev,\s+"
                     r"const float\* prev_normal_dev, const float\* prev_position_dev, const int32_t\* prev_id_dev,\s+"
                     r"const float\* cur_color_dev,\s+"
                     r"const float\* cur_normal_dev, const float\* cur_position_dev, const int32_t\* cur_id_dev,\s+"
                     r"float\* out_color_dev, float\* out_length_dev, uint32_t\* rgba_dev\);", hdr)
    assert "#define PTMI_ABI_VERSION 3" in hdr
    names = {n for n, _, _ in g._abi.PTMI_SYMBOLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    assert "pt_temporal" in names and hasattr(g._abi.ptmi(), "pt_temporal")
    assert re.search(r" T pt_temporal$", out, re.M)
    assert g._abi.ptmi().pt_abi_version() == 3     # functions are only added


def test_temporal_params_layout_matches_the_header():
    D = g.TemporalParams
    assert C.sizeof(D) == 24
    assert [(f, getattr(D, f).offset) for f, _ in D._fields_] == [
        ("width", 0), ("height", 4), ("max_history", 8), ("plane_tolerance", 12), ("normal_threshold", 16), ("_pad", 20)]
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct pt_temporal_params \{(.*?)\} pt_temporal_params;", hdr, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["width", "height", "max_history", "plane_tolerance", "normal_threshold", "_pad"]


def test_null_context_is_invalid():
    lib = g._abi.ptmi()
    tp = g.TemporalParams(8, 8, 32.0, 0.02, 0.9, 0)
    assert lib.pt_temporal(None, C.byref(tp), None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"null ctx" in lib.pt_last_error(None)


def test_defaults_are_the_issue_s_starting_values():
    assert g.TEMPORAL_DEFAULTS == dict(max_history=32.0, plane_tolerance=0.02, normal_threshold=0.9)
    src = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read()   # the app uses the same values
    m = re.search(r"pt_temporal_params tpar = \{[^,]+, [^,]+, ([\d.e+-]+)f, ([\d.e+-]+)f, ([\d.e+-]+)f, 0\}", src)
    assert m and tuple(float(m.group(k)) for k in (1, 2, 3)) == (32.0, 0.02, 0.9)


# ---------------------------------------------------------------------------------------------------- a plane facing the camera
PLANE_D = 10.0


def plane_guides(cam, W, H):
    """(normal, position, id) of the plane z = -PLANE_D seen through the pixel centres of `cam` (pt_render_aux's layout; the
    camera ray of pt_camera_ray in double, rounded once)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx = (xs - W / 2.0 + 0.5) * cam.dist * cam.aspect * cam.fov / (W - 1)
    sy = (ys - H / 2.0 + 0.5) * cam.dist * cam.fov / (H - 1)
    f, r, u, pos = (np.array(list(v), np.float64) for v in (cam.front, cam.right, cam.up, cam.pos))
    d0 = f * cam.dist + sx[..., None] * r + sy[..., None] * u
    o = pos + d0
    d = d0 / np.linalg.norm(d0, axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        t = (-PLANE_D - o[..., 2]) / d[..., 2]
    hit = np.isfinite(t) & (t > 0) & (d[..., 2] < 0)
    normal, position = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    normal[hit, 2] = 1.0
    position[hit, 0:3] = (o + t[..., None] * d)[hit]
    position[hit, 3] = t[hit]
    return normal, position, np.where(hit, 7, -1).astype(np.int32)


def plane_camera(W, H):
    cam = g.default_camera(W, H)
    cam.dist = 1.0
    return cam


@pytest.mark.parametrize("with_ids", [True, False])
def test_static_camera_keeps_every_pixel_and_lengths_grow_to_the_cap(with_ids):
    W, H = 33, 21
    cam = plane_camera(W, H)
    nrm, pos, ids = plane_guides(cam, W, H)
    ids = ids if with_ids else None
    rng = np.random.default_rng(3)
    hist = ln = None
    frames = []
    for k in range(1, 7):
        cur = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
        frames.append(cur)
        if hist is None:
            hist, ln, fragile, acc = T.temporal(W, H, None, None, None, None, None, None, cur, nrm, pos, ids, **params(max_history=4.0))
            assert not acc.any()
        else:
            new, ln, fragile, acc = T.temporal(W, H, cam, hist, ln, nrm, pos, ids, cur, nrm, pos, ids, **params(max_history=4.0))
            assert acc.all() and not fragile.any()
            n = min(k, 4)
            # the four weights are (1, 0, 0, 0) up to the rounding of fx (~ W 2^-22): random neighbours would show otherwise
            assert np.abs(new - (hist + (cur - hist) / n)).max() <= 1e-4
            hist = new
        assert np.abs(ln - min(k, 4)).max() <= 1e-4, k
        if k <= 4:   # below the cap the history is the mean of the frames
            assert np.abs(hist - np.mean(frames, axis=0)).max() <= 1e-4


def test_a_camera_turned_by_120_degrees_rejects_everything():
    W, H = 33, 21
    cam = plane_camera(W, H)
    nrm, pos, ids = plane_guides(cam, W, H)
    rng = np.random.default_rng(4)
    cur, prev = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2))
    ln = np.full((H, W), 9.0, np.float32)
    for deg in (120.0, -120.0, 180.0):
        out, length, fragile, acc = T.temporal(W, H, T.moved(cam, pan_deg=deg), prev, ln, nrm, pos, ids, cur, nrm, pos, ids, **params())
        assert not acc.any() and not fragile.any()
        assert np.array_equal(out.view(np.int32), cur.view(np.int32)) and np.all(length == 1)


@pytest.mark.parametrize("k", [1, 3, -2])
def test_a_sideways_move_of_k_pixel_footprints_shifts_the_history_by_k_pixels(k):
    W, H = 33, 21
    prev_cam = plane_camera(W, H)
    # one pixel's footprint on the plane: its distance from the camera point x the pixel pitch of the image plane at distance 1
    foot = PLANE_D * prev_cam.aspect * prev_cam.fov / (W - 1)
    cur_cam = T.moved(prev_cam, side=k * foot)
    pn, pp, pi = plane_guides(prev_cam, W, H)
    cn, cp, ci = plane_guides(cur_cam, W, H)
    rng = np.random.default_rng(5)
    cur, prev = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2))
    ln = np.ones((H, W), np.float32)
    out, length, fragile, acc = T.temporal(W, H, prev_cam, prev, ln, pn, pp, pi, cur, cn, cp, ci, **params())
    xs = np.arange(W)
    inside = (xs + k >= 0) & (xs + k <= W - 1)
    # the current pixel x sees what the previous pixel x + k saw
    assert acc[:, inside].all() and not acc[:, ~inside & ((xs + k < -1) | (xs + k > W))].any()
    src = np.clip(xs + k, 0, W - 1)
    want = 0.5 * (prev[:, src].astype(np.float64) + cur)
    assert np.abs(out - want)[:, inside].max() <= 1e-3      # fx is k off an integer by ~1e-5: the neighbour's share
    assert np.abs(length[:, inside] - 2).max() == 0
    gone = ~inside & ((xs + k < -1) | (xs + k > W))
    assert np.array_equal(out[:, gone].view(np.int32), cur[:, gone].view(np.int32))


def test_no_history_is_a_bit_copy():
    W, H = 9, 5
    cam = plane_camera(W, H)
    nrm, pos, ids = plane_guides(cam, W, H)
    cur = np.random.default_rng(6).uniform(0, 2, (H, W, 3)).astype(np.float32)
    out, length, fragile, acc = T.temporal(W, H, None, None, None, None, None, None, cur, nrm, pos, ids, **params())
    assert np.array_equal(out.view(np.int32), cur.view(np.int32)) and np.all(length == 1) and not fragile.any() and not acc.any()


def test_a_current_miss_and_a_history_miss_take_no_history():
    W, H = 17, 9
    cam = plane_camera(W, H)
    nrm, pos, ids = plane_guides(cam, W, H)
    cn, cp, pn, pp = nrm.copy(), pos.copy(), nrm.copy(), pos.copy()
    cn[2, 3], cp[2, 3] = 0, 0          # a current miss
    pn[5, 8], pp[5, 8] = 0, 0          # a miss in the history
    rng = np.random.default_rng(7)
    cur, prev = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2))
    ln = np.full((H, W), 3.0, np.float32)
    out, length, _, acc = T.temporal(W, H, cam, prev, ln, pn, pp, None, cur, cn, cp, None, **params())
    for y, x in ((2, 3), (5, 8)):
        assert not acc[y, x] and length[y, x] == 1 and np.array_equal(out[y, x], cur[y, x])
    assert acc.sum() == W * H - 2


# ---------------------------------------------------------------------------------------------------- the real inputs
_room = {}


def room_inputs(W, H, move):
    """The sphere room (cornell + the reference's spheres) from the golden camera (the history) and from the moved camera (the
    current frame): (prev_cam, prev guides, cur guides) with guides = (normal, position, id) of denoise_ref.guides."""
    if "bvh" not in _room:
        _room["bvh"], _room["sph"] = g.Bvh(g.scene_mesh("cornell")), g.reference_spheres()
    key = (W, H, move)
    if key not in _room:
        prev_cam, p = golden_camera(W, H), g.default_params(W, H)
        gp = R.guides(_room["bvh"], _room["sph"], prev_cam, p)[1:4]
        gc = gp if move == "static" else R.guides(_room["bvh"], _room["sph"], T.moved(prev_cam, **MOVES[move]), p)[1:4]
        _room[key] = (prev_cam, gp, gc)
    return _room[key]


@pytest.mark.parametrize("W,H", [(37, 23), (257, 131)])
@pytest.mark.parametrize("move", ["pan", "dolly", "side"])
def test_few_pixels_of_the_real_inputs_are_fragile(W, H, move):
    prev_cam, gp, gc = room_inputs(W, H, move)
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    for name, kw in PARAM_SETS.items():
        for ids in (True, False):
            out, length, fragile, acc = T.temporal(W, H, prev_cam, prev, ln, gp[0], gp[1], gp[2] if ids else None,
                                                   cur, gc[0], gc[1], gc[2] if ids else None, **params(**kw))
            assert fragile.mean() <= FRAGILE_MAX, (name, ids, float(fragile.mean()))
            if name != "plane0":
                assert acc.mean() > 0.3, (name, ids, float(acc.mean()))   # the move leaves most of the frame its history


# ---------------------------------------------------------------------------------------------------- quality
def quality_sequence(W, H, render, guides):
    """The quality measure: QUALITY_FRAMES frames of QUALITY_SPP samples of cornell_box, the camera panning QUALITY_PAN degrees
    a frame, carried through `T.temporal` with the defaults; render(cam, params, spp) -> colour, guides(cam, params) -> (normal,
    position, id).  Returns (gain, accepted share of the last frame)."""
    mesh, bvh, cam0, p = R.cornell_box_scene(W, H)
    cams = [T.moved(cam0, pan_deg=QUALITY_PAN * k) for k in range(QUALITY_FRAMES)]
    p.frame = 0
    ref = render(cams[-1], p, 1024)
    hist = ln = None
    for k, cam in enumerate(cams):
        p.frame = (1 << 20) + QUALITY_SPP * k
        cur = render(cam, p, QUALITY_SPP)
        gc = guides(cam, p)
        if hist is None:
            hist, ln, _, acc = T.temporal(W, H, None, None, None, None, None, None, cur, *gc, **g.TEMPORAL_DEFAULTS)
        else:
            hist, ln, _, acc = T.temporal(W, H, cams[k - 1], hist, ln, *gp, cur, *gc, **g.TEMPORAL_DEFAULTS)
        gp = gc
    return R.mse(cur, ref) / R.mse(hist, ref), float(acc.mean())


def test_reference_gain_on_oracle_renders():
    """8 frames of 4 spp of cornell_box at 80x60 under a 1 degree pan per frame: the history is QUALITY_GAIN_CPU times closer
    (MSE) to 1024 spp than the last frame alone, and at least ACCEPTED_MIN of the last frame's pixels took their history."""
    W, H = 80, 60
    mesh, bvh, _, _ = R.cornell_box_scene(W, H)

    def render(cam, p, spp):
        return orc.render(bvh, None, cam, p, spp, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)[0]

    def guides(cam, p):
        return R.guides(bvh, None, cam, p, mesh.materials, mesh.tri_material)[1:4]

    gain, accepted = quality_sequence(W, H, render, guides)
    print(f"temporal gain 80x60: {gain:.3f}, accepted {accepted:.3f}")
    assert accepted >= ACCEPTED_MIN, accepted
    assert abs(gain - QUALITY_GAIN_CPU) <= 0.01, gain      # the figure QUALITY_K is derived from (deterministic renders)
