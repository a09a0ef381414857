"""pt_camera_rays without a GPU: the declarations, the bindings, the NULL-context error, and the premises of the GPU tests — the
restated random stream (tests/camera_ref.py) gives the jitter of the oracle's camera rays exactly, and each float64 camera model
has its defining property and is undone by its inverse mapping."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import camera_ref as cr
import env_ref
import orc
from scene_matrix import make_camera

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
W, H = 37, 23


def golden(W, H):
    cam = g.default_camera(W, H)
    cam.dist = 18.0 * H / 1080.0
    return cam


def tilted(W, H, pos=(0.0, 0.0, 0.0)):
    return make_camera(W, H, pos=pos, front=(0.3, -0.2, -1.0), roll=0.4, fov=0.9)


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_header_declares_the_call():
    src = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int\s+pt_camera_rays\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_camera\s*\*\s*cam,\s*const\s+pt_camera_model\s*\*\s*cm,\s*uint64_t\s+frame,"
                     r"\s*const\s+uint32_t\s*\*\s*pixels_dev[^,)]*,\s*size_t\s+n,\s*uint64_t\s+first_pixel,\s*float\s*\*\s*rays_dev[^,)]*\)\s*;", src)
    assert re.search(r"PT_CAM_PINHOLE\s*=\s*0\s*,\s*PT_CAM_THIN_LENS\s*=\s*1\s*,\s*PT_CAM_ORTHO\s*=\s*2\s*,\s*PT_CAM_FISHEYE\s*=\s*3\s*,\s*PT_CAM_EQUIRECT\s*=\s*4", src)
    assert re.search(r"PT_CAMF_CENTRE\s*=\s*1\b", src)
    key = re.search(r"#define\s+PT_CAM_LENS_KEY\s+(0x[0-9A-Fa-f]+)ull", src)
    assert key and int(key.group(1), 16) == g.CAM_LENS_KEY == cr.LENS_KEY and g.CAM_LENS_KEY >> 63 == 1
    body = re.search(r"typedef\s+struct\s+pt_camera_model\s*\{(.*?)\}\s*pt_camera_model\s*;", src, re.S)
    assert body
    fields = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", fields).strip() == ("int32_t model; int32_t width, height; int32_t flags; float lens_radius; float focus_dist; "
                                                    "float ortho_height; float fisheye_fov;")
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src)


def test_left_out_items_are_in_the_header():
    src = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "ptmi.h")).read())
    section = src[src.index("pt_camera_rays writes"):src.index("enum { PT_CAM_PINHOLE")]
    left = section[section.index("Left out:"):]
    for item in ("guide buffers for these cameras", "pt_render_aux stays pinhole", "stereo pairs", "lens shapes other than a disk",
                 "RNG keys for pt_render_rays by pixel", "the generator fused into the path kernel"):
        assert item in left, item


def test_struct_mirror_is_32_bytes():
    M = g.CameraModel
    assert C.sizeof(M) == 32
    assert [(n, getattr(M, n).offset) for n, _ in M._fields_] == [("model", 0), ("width", 4), ("height", 8), ("flags", 12), ("lens_radius", 16),
                                                                    ("focus_dist", 20), ("ortho_height", 24), ("fisheye_fov", 28)]
    src = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "csrc", "pt_camera.hip")).read()
    assert "static_assert(sizeof(pt_camera_model) == 32" in src


def test_abi_binds_and_the_package_exports():
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_camera_rays"][2]) == 8
    lib = g._abi.ptmi()
    assert lib.pt_camera_rays.argtypes[3] is C.c_uint64 and lib.pt_camera_rays.argtypes[5] is C.c_size_t and lib.pt_camera_rays.argtypes[6] is C.c_uint64
    assert (g.CAM_PINHOLE, g.CAM_THIN_LENS, g.CAM_ORTHO, g.CAM_FISHEYE, g.CAM_EQUIRECT) == (0, 1, 2, 3, 4) == \
        (g._abi.CAM_PINHOLE, g._abi.CAM_THIN_LENS, g._abi.CAM_ORTHO, g._abi.CAM_FISHEYE, g._abi.CAM_EQUIRECT) == \
        (cr.PINHOLE, cr.THIN_LENS, cr.ORTHO, cr.FISHEYE, cr.EQUIRECT)
    assert g.CAMF_CENTRE == g._abi.CAMF_CENTRE == 1
    assert lib.pt_abi_version() == 3
    for name in ("camera_rays", "render_camera"):
        assert callable(getattr(g.PathTracer, name))
    for kind, value in (("pinhole", 0), ("thinlens", 1), ("ortho", 2), ("fisheye", 3), ("equirect", 4)):
        cm = g.camera_model(kind, 64, 32)
        assert isinstance(cm, g.CameraModel) and (cm.model, cm.width, cm.height, cm.flags) == (value, 64, 32, 0)
        assert cm.lens_radius == 0 and cm.focus_dist > 0 and cm.ortho_height > 0 and 0 < cm.fisheye_fov <= 2 * np.pi
    cm = g.camera_model(g.CAM_FISHEYE, 16, 8, centre=True, fisheye_fov=2.0)
    assert (cm.model, cm.flags, cm.fisheye_fov) == (3, g.CAMF_CENTRE, 2.0)


def test_pt_app_has_the_camera_option():
    src = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read()
    head = src[:src.index("#include")]
    for word in ("--camera", "--aperture", "--focus", "--ortho-height", "--fisheye-deg"):
        assert f'"{word}"' in src and word in head, word
    assert "pt_camera_rays(" in src
    mk = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "Makefile")).read()
    assert "csrc/pt_camera.o" in mk.split("OBJS =")[1].split("\n")[0] and "csrc/pt_camera.o: csrc/pt_camera.hip $(KHDR)" in mk


def test_null_context_is_refused():
    lib = g._abi.ptmi()
    cam, cm = golden(W, H), g.camera_model("pinhole", W, H)
    assert lib.pt_camera_rays(None, C.byref(cam), C.byref(cm), 7, None, 4, 0, None) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()
    assert lib.pt_camera_rays(None, None, None, 0, None, 0, 0, None) == -1   # before n == 0


# ---------------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize("frame", [7, 8])
def test_the_restated_stream_gives_the_oracles_jitter(frame):
    """The draws equal the oracle's, bit for bit; the oracle's camera function fed them gives orc.primary_rays' rows, bit for bit
    (so they ARE the jitter of those rays); and the float64 pinhole fed that jitter is undone by its inverse within 1e-6 pixel.
    The oracle's binary32 rays themselves invert to within 1e-3 pixel, the bound of the GPU tests."""
    cam = golden(W, H)
    pix, px, py = cr.pixel_grid(W, H)
    u0, u1 = cr.draws(frame, pix)
    L = orc.lib()
    want = np.array([[L.orc_rng_draw(frame, int(p), 0), L.orc_rng_draw(frame, int(p), 1)] for p in pix], np.float32)
    assert np.array_equal(u0.view(np.uint32), want[:, 0].view(np.uint32)) and np.array_equal(u1.view(np.uint32), want[:, 1].view(np.uint32))
    assert u0.min() > 0 and u0.max() <= 1 and len(np.unique(u0)) > 800
    rays = orc.primary_rays(cam, W, H, frame=frame)
    made = np.zeros_like(rays)
    for p in pix:
        o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
        L.orc_camera_ray(C.byref(cam), int(px[p]), int(py[p]), W, H, u0[p], u1[p], o.ctypes.data, d.ctypes.data)
        made[p, 0:3], made[p, 4:7] = o, d
    assert np.array_equal(made.view(np.uint32), rays.view(np.uint32))
    jx, jy = cr.jitter(frame, pix)
    assert np.array_equal(jx, u0 - np.float32(0.5)) and np.abs(jx).max() <= 0.5
    m = cr.Model(cam, cr.PINHOLE, W, H)
    fx, fy = px + jx.astype(np.float64), py + jy.astype(np.float64)
    o, d, has = m.rays(fx, fy)
    gx, gy = m.pixel_coords(o, d)
    assert has.all() and np.abs(gx - fx).max() <= 1e-6 and np.abs(gy - fy).max() <= 1e-6
    gx, gy = m.pixel_coords(rays[:, 0:3], rays[:, 4:7])
    assert np.abs(gx - fx).max() <= 1e-3 and np.abs(gy - fy).max() <= 1e-3
    # the origin lies ON the image plane: `dist` in front of pos
    assert np.abs((o - m.pos) @ m.front - m.dist).max() <= 1e-12
    assert not np.array_equal(cr.draws(frame, pix, cr.LENS_KEY)[0], u0), "the lens stream is another stream"


def test_centre_jitter_is_zero():
    jx, jy = cr.jitter(7, np.arange(10), centre=True)
    assert not jx.any() and not jy.any() and jx.dtype == np.float32


# ---------------------------------------------------------------------------------------------------- the models' defining properties
def coords(frame=7):
    pix, px, py = cr.pixel_grid(W, H)
    jx, jy = cr.jitter(frame, pix)
    return px + jx.astype(np.float64), py + jy.astype(np.float64)


def test_fisheye_centre_looks_along_front_and_the_rim_at_half_the_angle():
    # an exactly orthonormal basis: towards theta = pi the image-plane direction is (b, c) / sin(theta), which magnifies the 6e-8 by
    # which a rounded binary32 basis is skew (the inverse assumes it orthonormal, as the model does)
    cam = make_camera(W, H, pos=(1.0, 2.0, 3.0), front=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    for fov in (np.pi, 2.0, 2 * np.pi):
        m = cr.Model(cam, cr.FISHEYE, W, H, fisheye_fov=fov)
        c = np.array([W / 2.0 - 0.5]), np.array([H / 2.0 - 0.5])          # the image centre: ax = ay = 0
        o, d, has = m.rays(*c)
        f = m.front / np.linalg.norm(m.front)
        assert has.all() and np.allclose(d[0], f, atol=1e-12) and np.array_equal(o[0], m.pos)
        rim = min(W, H) / 2.0
        for ang in np.linspace(0, 2 * np.pi, 7):
            o, d, has = m.rays(c[0] + rim * (1 - 1e-9) * np.cos(ang), c[1] + rim * (1 - 1e-9) * np.sin(ang))
            assert has.all() and abs(np.arccos(np.clip(d[0] @ f, -1, 1)) - m.ffov / 2) <= 1e-6
            _, d2, has2 = m.rays(c[0] + 1.001 * rim * np.cos(ang), c[1] + 1.001 * rim * np.sin(ang))
            assert not has2.any() and not d2.any(), "outside the image circle there is no ray"
        fx, fy = coords()
        o, d, has = m.rays(fx, fy)
        gx, gy = m.pixel_coords(o, d)
        assert has.sum() > 300 and np.abs(gx - fx)[has].max() <= 1e-6 and np.abs(gy - fy)[has].max() <= 1e-6
        assert np.isnan(gx[~has]).all()


def test_thin_lens_rays_of_a_pixel_meet_in_the_plane_in_focus():
    cam = tilted(W, H)
    m = cr.Model(cam, cr.THIN_LENS, W, H, lens_radius=0.2, focus_dist=3.0)
    fx, fy = coords()
    pf = m.focus_point(fx, fy)
    f = m.front / np.linalg.norm(m.front)
    assert np.abs((pf - m.pos) @ f - 3.0).max() <= 1e-5, "pf lies in the plane `focus_dist` along front (the basis is binary32)"
    rng = np.random.default_rng(4)
    origins = []
    for _ in range(3):
        v0, v1 = rng.random(len(fx)), rng.random(len(fx))
        o, d, _ = m.rays(fx, fy, v0, v1)
        t = np.einsum("ij,ij->i", pf - o, d)
        assert np.linalg.norm(o + t[:, None] * d - pf, axis=1).max() <= 1e-9, "every lens point's ray passes through pf"
        assert np.linalg.norm(o - m.pos, axis=1).max() <= 0.2 * (1 + 1e-9) and np.abs((o - m.pos) @ f).max() <= 1e-7
        gx, gy = m.pixel_coords(o, d)
        assert np.abs(gx - fx).max() <= 1e-6 and np.abs(gy - fy).max() <= 1e-6
        origins.append(o)
    assert not np.allclose(origins[0], origins[1])
    # a closed aperture is the pinhole seen from pos
    m0 = cr.Model(cam, cr.THIN_LENS, W, H, lens_radius=0.0, focus_dist=3.0)
    o, d, _ = m0.rays(fx, fy, rng.random(len(fx)), rng.random(len(fx)))
    _, dp, _ = cr.Model(cam, cr.PINHOLE, W, H).rays(fx, fy)
    assert np.array_equal(o, np.tile(m0.pos, (len(fx), 1))) and np.abs(d - dp).max() <= 1e-12


def test_ortho_rays_are_parallel_and_evenly_spaced():
    cam = tilted(W, H, pos=(1.0, 2.0, 3.0))
    m = cr.Model(cam, cr.ORTHO, W, H, ortho_height=10.0)
    pix, px, py = cr.pixel_grid(W, H)
    o, d, has = m.rays(px.astype(np.float64), py.astype(np.float64))
    assert has.all() and np.abs(d - d[0]).max() == 0 and np.allclose(d[0], m.front / np.linalg.norm(m.front), atol=1e-12)
    o = o.reshape(H, W, 3)
    assert np.allclose(np.linalg.norm(o[1:] - o[:-1], axis=-1), 10.0 / H * np.linalg.norm(m.up), rtol=1e-12)
    assert np.allclose(np.linalg.norm(o[:, 1:] - o[:, :-1], axis=-1), 10.0 * m.aspect / W * np.linalg.norm(m.right), rtol=1e-12)
    fx, fy = coords()
    o, d, _ = m.rays(fx, fy)
    gx, gy = m.pixel_coords(o, d)
    assert np.abs(gx - fx).max() <= 1e-6 and np.abs(gy - fy).max() <= 1e-6


def test_equirect_inverts_to_env_refs_positions():
    """The inverse is env_ref.positions — the lookup's own (fx, fy) — and the centred rays are the directions pt_app --equirect
    renders."""
    cam = tilted(16, 8)
    m = cr.Model(cam, cr.EQUIRECT, 16, 8)
    basis = dict(front=tuple(cam.front), right=tuple(cam.right), up=tuple(cam.up))
    pix, px, py = cr.pixel_grid(16, 8)
    o, d, has = m.rays(px.astype(np.float64), py.astype(np.float64))
    assert has.all() and np.abs(d - env_ref.equirect_dirs(16, 8, **basis)).max() <= 1e-7
    jx, jy = cr.jitter(7, pix)
    fx, fy = px + jx.astype(np.float64), py + jy.astype(np.float64)
    o, d, _ = m.rays(fx, fy)
    ex, ey, valid = env_ref.positions(d.astype(np.float32), 16, 8, **basis)
    gx, gy = m.pixel_coords(o, d.astype(np.float32))
    assert valid.all() and np.array_equal(gx, ex) and np.array_equal(gy, ey)
    free = fy > 0   # row 0 with a negative jitter lies past the pole: its latitude is clamped, its longitude is lost
    assert (~free).sum() > 0 and free.sum() > 100
    assert np.abs(ey - np.maximum(fy, 0)).max() <= 1e-5
    dx = np.abs(ex - fx)[free]
    assert np.minimum(dx, 16 - dx).max() <= 1e-4
