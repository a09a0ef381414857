"""Guide buffers and reprojection for the camera models without a GPU: pt_render_aux_camera and
pt_temporal_camera in the header, the binding and the library; the float64 projection of tests/camera_guides_ref.py against the
forward models of tests/camera_ref.py; the check program's walk over both calls' rules (csrc/pt_variants_check.cpp); and the premises
of tests/test_gpu_camera_guides.py, on guides made here from camera_ref.Model.rays through the oracle's walk."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import camera_guides_ref as G
import camera_ref as cr
import gpu_pathtracer_amd as g
import temporal_ref as T
from gpu_support import bvh_of, golden_camera

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")
PT_ERR_INVALID = -1
# the two calls under test: every test of this file, the premises included, stands on them (a library without them fails here)
CALLS = (g._abi.ptmi().pt_render_aux_camera, g._abi.ptmi().pt_temporal_camera)


def flat(text):
    return re.sub(r"\s+\*?\s*", " ", text)


# ---------------------------------------------------------------------------------------------------- the surface
def test_symbols_bindings_and_null_context():
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_render_aux_camera"][2]) == 8 and len(rows["pt_temporal_camera"][2]) == 20
    lib = g._abi.ptmi()
    assert lib.pt_render_aux_camera.argtypes[2]._type_ is g._abi.CameraModel and lib.pt_temporal_camera.argtypes[3]._type_ is g._abi.CameraModel
    assert lib.pt_temporal_camera.argtypes[6] is C.c_size_t
    cam, cm, p = golden_camera(8, 8), g.camera_model("fisheye", 8, 8), g.default_params(8, 8)
    tp = g.TemporalParams(8, 8, 32.0, 0.02, 0.9, 0)
    assert lib.pt_render_aux_camera(None, C.byref(cam), C.byref(cm), C.byref(p), None, None, None, None) == PT_ERR_INVALID
    assert lib.pt_last_error(None) == b"null ctx"
    assert lib.pt_temporal_camera(None, C.byref(tp), C.byref(cam), C.byref(cm), None, None, 0, *([None] * 13)) == PT_ERR_INVALID
    assert lib.pt_last_error(None) == b"null ctx"
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libptmi.so")], capture_output=True, text=True)
    assert nm.returncode == 0
    for name in ("pt_render_aux_camera", "pt_temporal_camera"):
        assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"libptmi.so does not export {name}"
    blob = open(os.path.join(CSRC, "libptmi.so"), "rb").read()
    assert b"k_render_aux_camera" in blob and b"k_temporal_camera" in blob
    assert list(inspect.signature(g.PathTracer.render_aux_camera).parameters) == ["self", "cam", "model", "params", "albedo_ptr", "normal_ptr",
                                                                                 "position_ptr", "id_ptr"]
    assert list(inspect.signature(g.PathTracer.temporal_camera).parameters)[:6] == ["self", "width", "height", "prev_cam", "prev_model", "prev_color_ptr"]
    assert inspect.signature(g.TemporalHistory.push).parameters["model"].default is None


def test_header_states_the_two_calls():
    src = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "#define PTMI_ABI_VERSION 3" in src
    assert re.search(r"int\s+pt_render_aux_camera\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_camera\s*\*\s*cam,\s*const\s+pt_camera_model\s*\*\s*cm,"
                     r"\s*const\s+pt_params\s*\*\s*params,", src)
    assert re.search(r"int\s+pt_temporal_camera\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_temporal_params\s*\*\s*tp,\s*const\s+pt_camera\s*\*\s*prev_cam,"
                     r"\s*const\s+pt_camera_model\s*\*\s*prev_cm,\s*const\s+float\s*\*\s*prev_verts_dev,", src)
    text = flat(src[src.index("guide buffers and reprojection for the camera models"):src.index("display: exposure metering and tone mapping")])
    for piece in ("DESIGN.md §10 f20", "under PT_CAMF_CENTRE with lens_radius taken as 0", "is not walked and writes a miss",
                  "kx = (float)W / (ortho_height * aspect)", "fx = fmaf(b, kx, cx), fy = fmaf(c, ky, cy)", "s = sqrtf(fmaf(c, c, b * b))",
                  "theta = atan2f(s, a)", "kf = ((float)min(W, H) / 2.0f) / half", "k = s > 0 ? rho / s : 0", "There is no a > 0 test",
                  "h = sqrtf(fmaf(b, b, a * a))", "lon = atan2f(b, a), lat = atan2f(c, h)", "(float)W / 6.28318548f", "(float)H / 3.14159274f",
                  "rejected when fx or fy is not finite", "Horizontal wrap".lower(), "a moments variant", "pt_app --camera"):
        assert flat(piece) in text, piece
    # the guide-buffer item of the two older calls' "Left out" lists (tests/test_camera.py and tests/test_render_camera.py pin its
    # words) now names the call that makes the guides
    for call in ("int pt_camera_rays(", "int pt_render_camera("):
        doc = src[:src.index(call)]
        left = doc[doc.rindex("Left out:"):]
        assert "pt_render_aux_camera" in left and "do not serve them yet" not in flat(left), call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    f20 = design[design.index("f20"):]
    for piece in ("pt_render_aux_camera", "pt_temporal_camera", "pt_app", "seam", "moments"):
        assert piece in f20, piece
    assert "pt_render_aux_camera" in open(os.path.join(ROOT, "README.md")).read()


# ---------------------------------------------------------------------------------------------------- the projection
def orthonormal_model(kind, W, H, seed, **kw):
    """A camera_ref.Model at a tilted position whose basis is orthonormal in float64."""
    m = cr.Model(golden_camera(W, H), kind, W, H, **kw)
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    m.front, m.right, m.up = q[:, 0], q[:, 1], q[:, 2]
    m.pos = np.array([0.5, -0.25, 1.0])
    return m


@pytest.mark.parametrize("name", list(G.MODELS))
@pytest.mark.parametrize("size", [(64, 48), (33, 17), (64, 32)], ids=["64x48", "33x17", "64x32"])
def test_project_inverts_the_forward_models(name, size):
    """project(m, o + t d) returns the coordinates m.rays was given, to 1e-9 pixel, at random t — and at integer coordinates (a pixel
    centre of the forward model is an integer coordinate of the inverse: the half-pixel conventions)."""
    W, H = size
    kind, kw = G.MODELS[name]
    m = orthonormal_model(kind, W, H, 5, **kw)
    rng = np.random.default_rng(W + H)
    n = 4000
    fx, fy = rng.uniform(-0.5, W - 0.5, n), rng.uniform(-0.5, H - 0.5, n)
    _, px, py = cr.pixel_grid(W, H)
    fx, fy = np.concatenate([fx, px.astype(np.float64)]), np.concatenate([fy, py.astype(np.float64)])
    if kind == cr.EQUIRECT:   # the poles have no longitude
        keep = np.abs((fy - H / 2.0) * (np.pi / H)) < np.pi / 2 - 1e-3
        fx, fy = fx[keep], fy[keep]
    o, d, has = m.rays(fx, fy)
    assert has.sum() > 0.3 * len(fx)
    t = rng.uniform(0.5, 60.0, len(fx))
    gx, gy = G.project(m, (o + t[:, None] * d)[has])
    ex, ey = G.coord_error(m, gx, gy, fx[has], fy[has])
    print(f"{name} {W}x{H}: |fx| {ex.max():.3g} |fy| {ey.max():.3g}")
    assert ex.max() <= 1e-9 and ey.max() <= 1e-9
    rejected, fragile = G.rejects(m, (o + t[:, None] * d)[has])
    assert not np.any(rejected & ~fragile), "a point a pixel sees is not turned away"
    if kind == cr.FISHEYE:   # points outside the image circle are
        out = m.pos + 3.0 * (np.cos(m.ffov / 2 + 0.05) * m.front + np.sin(m.ffov / 2 + 0.05) * m.up)
        assert G.rejects(m, out[None])[0][0]
    if kind in (cr.PINHOLE, cr.THIN_LENS, cr.ORTHO):
        assert G.rejects(m, (m.pos - 2.0 * m.front + 0.3 * m.up)[None])[0][0]


# ---------------------------------------------------------------------------------------------------- the rules
@pytest.mark.parametrize("san", ["", "SAN=1"], ids=["plain", "sanitized"])
def test_check_program_walks_both_calls_rules(san):
    """The error order of pt_render_aux_camera and of pt_temporal_camera — every rule broken alone and together, the first in the
    header's order answering with its own text — as the check program walks it; the entry points ask the functions it runs."""
    src = open(os.path.join(CSRC, "pt_variants_check.cpp")).read()
    assert "first_answers(check_aux_camera_call(f," in src and '{TEMPORAL_CAMERA, "pt_temporal_camera"}' in src
    for text in ("pt_render_aux_camera: unknown camera model", "pt_render_aux_camera: no BVH uploaded", "pt_temporal_camera: a history needs the model of its camera",
                 "pt_temporal_camera: the model's image must be the parameters'", "pt_temporal_camera: ortho_height must be finite"):
        assert text in src, text
    aux = open(os.path.join(CSRC, "pt_aux.hip")).read()
    body = aux[aux.index('extern "C" int pt_render_aux_camera('):]
    assert "check_aux_camera_call(f, cm, p," in body and body.index('"null ctx"') < body.index("check_aux_camera_call(")
    assert len(re.findall(r"PT_ERR_INVALID|PT_ERR_UNSUPPORTED|PT_ERR_NO_SCENE", body)) == 1, "no rule of its own but null ctx"
    tmp = open(os.path.join(CSRC, "pt_temporal.hip")).read()
    body = tmp[tmp.index('extern "C" int pt_temporal_camera('):]
    assert 'temporal_args(c, "pt_temporal_camera", a, C.m)' in body and len(re.findall(r"PT_ERR_INVALID|PT_ERR_UNSUPPORTED|PT_ERR_NO_SCENE", body)) == 1
    exe = os.path.join(CSRC, "pt_variants_check")
    build = subprocess.run(["make", "-B", "-C", PKG, "variants_check"] + ([san] if san else []), capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout


def test_history_class_checks_its_model():
    class Stub:
        def malloc(self, n):
            return type("B", (), {"ptr": 1, "free": lambda self: None})()
    th = g.TemporalHistory(Stub(), 8, 8, with_moments=True)
    with pytest.raises(ValueError):
        th.push(golden_camera(8, 8), g.default_params(8, 8), 1, moments_ptr=1, model=g.camera_model("fisheye", 8, 8))
    th = g.TemporalHistory(Stub(), 8, 8)
    with pytest.raises(ValueError):
        th.push(golden_camera(8, 8), g.default_params(8, 8), 1, model=g.camera_model("fisheye", 16, 8))


# ---------------------------------------------------------------------------------------------------- premises of the GPU tests
_cpu_guides = {}


def cpu_guides(name, W, H, cam):
    """The room's guides under a model, made on the CPU: the six-tuple of guides_from_rays."""
    key = (name, W, H, tuple(cam.pos), tuple(cam.front))
    if key not in _cpu_guides:
        _, bvh = bvh_of("cornell")
        cm = G.camera_model(name, W, H)
        _cpu_guides[key] = G.guides_from_rays(G.centre_rays(cam, cm), bvh, g.reference_spheres(), g.default_params(W, H), (H, W))
    return _cpu_guides[key]


@pytest.mark.parametrize("name", list(G.MODELS))
def test_premises_of_the_guides(name):
    """Every model's room at both sizes from the guide camera: more than 5 % of the pixels hit triangles, sphere ids show; a fisheye
    has pixels outside its circle, all misses, and hits inside; a pixel subtends at least 0.05 rad under the two angular models."""
    for k in (k for n, k in G.MODEL_CASES if n == name):
        guides_premises(name, *G.size_of(name, k))


def guides_premises(name, W, H):
    cam = G.guide_camera(W, H)
    alb, nrm, pos, ids, _, _ = cpu_guides(name, W, H, cam)
    assert (ids >= 0).mean() > 0.05 and (ids <= -2).any(), ((ids >= 0).mean(), (ids <= -2).any())
    kind, kw = G.MODELS[name]
    if kind == cr.FISHEYE:
        m = cr.Model.of(cam, G.camera_model(name, W, H))
        _, px, py = cr.pixel_grid(W, H)
        _, _, has = m.rays(px.astype(np.float64), py.astype(np.float64))
        has = has.reshape(H, W)
        assert 0 < (~has).sum() and np.all(ids[~has] == -1) and (ids[has] != -1).any()
        for w, h in G.SIZES:
            assert kw["fisheye_fov"] / min(w, h) >= 0.05
    if kind == cr.EQUIRECT:
        assert 2 * np.pi / W >= 0.05 and np.pi / H >= 0.05


@pytest.mark.parametrize("move", list(T.MOVES))
@pytest.mark.parametrize("name", G.MOVED_MODELS)
def test_premises_of_the_moved_camera(name, move):
    """The two conditions of the GPU suite's moved-camera test, on the reference alone: the history is accepted on at least half
    of the hit pixels, and the fragile share stays within temporal_ref.FRAGILE_MAX."""
    W, H = G.size_of(name)
    prev_cam = golden_camera(W, H)
    cur_cam = T.moved(prev_cam, **G.move_of(name, move))
    gp, gc = cpu_guides(name, W, H, prev_cam), cpu_guides(name, W, H, cur_cam)
    m = cr.Model.of(prev_cam, G.camera_model(name, W, H))
    pts = gc[2][..., 0:3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        fx, fy = (v.reshape(H, W) for v in G.project(m, pts))
    rejected, frag = (v.reshape(H, W) for v in G.rejects(m, pts))
    cur, prev, ln = T.random_frames(W, H, W + 31 * H)
    _, length, fragile, accepted = G.blend_from_coords(W, H, fx.astype(np.float32), fy.astype(np.float32), ~rejected, prev, ln, gp[1], gp[2], gp[3],
                                                       cur, gc[1], gc[2], gc[3], **T.params())
    hit = gc[3] != -1
    fragile |= frag & hit
    print(f"{name} {move}: accepted {accepted.sum() / hit.sum():.3f} of the hit pixels, fragile {fragile.mean():.4f}")
    assert accepted.sum() >= 0.5 * hit.sum(), accepted.sum() / hit.sum()
    assert fragile.mean() <= T.FRAGILE_MAX, fragile.mean()
