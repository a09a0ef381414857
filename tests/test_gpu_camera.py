"""pt_camera_rays — jittered rays of five camera models made on the device (extension; contract in
include/ptmi.h).

The pinhole is pinned bit for bit: its rows are orc.primary_rays', and the generate-then-trace loop (PathTracer.render_camera)
folds pt_render's frame.  The other models are judged through the float64 inverse mappings of tests/camera_ref.py: the ray the
device made, taken back to continuous pixel coordinates, must land within 1e-3 pixel of the pixel plus its restated jitter.  At the
sizes used here a pixel subtends at least 0.05 rad, so the bound is about 5e-5 rad: fifty times binary32's rounding through such a
chain, and five hundred times smaller than a half-pixel convention error.  tests/test_camera.py checks the premises on the CPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref as cr
import gpu_pathtracer_amd as g
import orc
from gpu_support import bits, golden_camera, setup_scene
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
SIZES = [(37, 23), (16, 8)]
PIXEL_BOUND = 1e-3
UNIT_BOUND = 2.0 ** -20
CANARY = -7.0
BK = (0.125, 0.75, 0.375)


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)   # what pt_render runs beside it; pt_camera_rays and pt_render_rays do not read the option
    yield tr
    tr.close()


def tilted(W, H, pos=(0.5, -0.25, 1.0)):
    """An orthonormal basis that is no permutation of the axes: a model that mixed up front, right and up would show."""
    return make_camera(W, H, pos=pos, front=(0.3, -0.2, -1.0), roll=0.4, fov=0.9)


def generate(t, cam, cm, frame, n=None, first_pixel=0, pixels=None):
    """pt_camera_rays into a fresh buffer pre-filled with CANARY, one spare row behind it: (rows [n][8], the spare row)."""
    if n is None:
        n = len(pixels) if pixels is not None else cm.width * cm.height - first_pixel
    buf = t.malloc(32 * (n + 1))
    buf.upload(np.full((n + 1, 8), CANARY, np.float32))
    lst = None
    if pixels is not None:
        lst = t.malloc(4 * max(len(pixels), 1))
        lst.upload(np.asarray(pixels, np.uint32))
    t.camera_rays(cam, cm, frame, buf.ptr, n, first_pixel, lst.ptr if lst else None)
    t.sync()
    out = buf.download(np.float32, (n + 1, 8))
    buf.free()
    if lst:
        lst.free()
    assert np.all(out[n] == CANARY), "the row behind the buffer was written"
    return out[:n]


def model_kwargs(kind):
    return {cr.THIN_LENS: dict(lens_radius=0.2, focus_dist=3.0), cr.ORTHO: dict(ortho_height=10.0), cr.FISHEYE: dict(fisheye_fov=2.5)}.get(kind, {})


# ---------------------------------------------------------------------------------------------------- 1: the pinhole, bit for bit
@pytest.mark.parametrize("size", SIZES, ids=["37x23", "16x8"])
def test_pinhole_rows_are_the_oracles(t, size):
    W, H = size
    cam = golden_camera(W, H)
    for frame in (7, 8):
        want = orc.primary_rays(cam, W, H, frame=frame)
        got = generate(t, cam, g.camera_model("pinhole", W, H), frame)
        assert np.array_equal(bits(got), bits(want)), f"frame {frame}: {int(np.any(bits(got) != bits(want), axis=1).sum())} rows differ"
        # a batch split by first_pixel
        k = (W * H) // 2 - 3
        parts = np.concatenate([generate(t, cam, g.camera_model("pinhole", W, H), frame, n=k),
                                generate(t, cam, g.camera_model("pinhole", W, H), frame, first_pixel=k)])
        assert np.array_equal(bits(parts), bits(want))
    assert not np.array_equal(orc.primary_rays(cam, W, H, frame=7), orc.primary_rays(cam, W, H, frame=8))
    centre = generate(t, cam, g.camera_model("pinhole", W, H, centre=True), 7)
    assert np.array_equal(bits(centre), bits(orc.primary_rays(cam, W, H, frame=7, jitter=False)))
    assert np.array_equal(bits(centre), bits(generate(t, cam, g.camera_model("pinhole", W, H, centre=True), 8))), "no draw under PT_CAMF_CENTRE"


# ---------------------------------------------------------------------------------------------------- 2: the whole loop
@pytest.mark.parametrize("flags", [0, g.FLAGS_SMALLPT], ids=["default", "smallpt"])
def test_render_camera_is_pt_render(t, flags):
    """render_camera(pinhole, spp = 3) — three times (pt_camera_rays, one-sample pt_render_rays) on one stream, no sync — equals
    pt_render(spp = 3) on the same context bit for bit: the generator spends exactly the two draws pt_render_rays' stream stands
    behind, and each sample gets its own frame number and running-mean index."""
    W, H = 37, 23
    setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    p.frame, p.sample_index, p.flags = 7, 1, flags
    acc, rgba = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 3)
    t.sync()
    ref = acc.download(np.float32, (H, W, 3))
    rays, out = t.malloc(32 * W * H), t.malloc(12 * W * H)
    out.upload(np.full((H, W, 3), CANARY, np.float32))
    t.render_camera(cam, g.camera_model("pinhole", W, H), p, out.ptr, rays.ptr, spp=3)
    t.sync()
    got = out.download(np.float32, (H, W, 3))
    for b in (acc, rgba, rays, out):
        b.free()
    assert ref.any() and len(np.unique(ref.reshape(-1, 3), axis=0)) > 100
    assert np.array_equal(bits(got), bits(ref)), f"{int(np.any(bits(got) != bits(ref), axis=-1).sum())} pixels differ"


# ---------------------------------------------------------------------------------------------------- 3: the pixel list
def test_pixel_list(t):
    W, H = 37, 23
    cam, cm = tilted(W, H), g.camera_model("pinhole", W, H)
    full = generate(t, cam, cm, 7)
    perm = np.random.default_rng(11).permutation(W * H).astype(np.uint32)
    got = generate(t, cam, cm, 7, pixels=perm)
    assert np.array_equal(bits(got), bits(full[perm])) and not np.array_equal(bits(got), bits(full))
    # indices past the image among valid ones: o = pos, d = 0
    lst = np.array([5, W * H, 17, W * H + 5, 2 ** 32 - 1, W * H - 1], np.uint32)
    past = lst >= W * H
    pos = np.array(list(cam.pos), np.float32)
    for kind in range(5):
        cmk = g.camera_model(kind, W, H, **model_kwargs(kind))
        rows = generate(t, cam, cmk, 7, pixels=lst)
        assert np.array_equal(bits(rows[past]), bits(np.tile(np.concatenate([pos, [0], [0, 0, 0], [0]]).astype(np.float32), (3, 1)))), kind
        assert np.array_equal(bits(rows[~past]), bits(generate(t, cam, cmk, 7)[lst[~past]])), kind
    # such a row renders as bk_color
    setup_scene(t, "room", False)
    rows = generate(t, golden_camera(W, H), cm, 7, pixels=lst)
    p = g.default_params(W, H)
    p.frame, p.bk_color[:] = 7, BK
    rays, out = t.malloc(rows.nbytes), t.malloc(12 * len(rows))
    rays.upload(rows)
    t.render_rays(rays.ptr, len(rows), out.ptr, p, 1)
    t.sync()
    rad = out.download(np.float32, (len(rows), 3))
    rays.free()
    out.free()
    assert np.array_equal(rad[past], np.tile(np.array(BK, np.float32), (3, 1))) and not np.any(np.all(rad[~past] == np.array(BK, np.float32), axis=1))


# ---------------------------------------------------------------------------------------------------- 4: every other model
@pytest.mark.parametrize("size", SIZES, ids=["37x23", "16x8"])
@pytest.mark.parametrize("centre", [False, True], ids=["jittered", "centred"])
@pytest.mark.parametrize("kind", [cr.THIN_LENS, cr.ORTHO, cr.FISHEYE, cr.EQUIRECT], ids=["thinlens", "ortho", "fisheye", "equirect"])
def test_models_invert_to_the_jittered_pixel(t, kind, centre, size):
    W, H = size
    cam = tilted(W, H)
    cm = g.camera_model(kind, W, H, centre=centre, **model_kwargs(kind))
    m = cr.Model.of(cam, cm)
    pix, px, py = cr.pixel_grid(W, H)
    for frame in (7, 8):
        rows = generate(t, cam, cm, frame)
        jx, jy = cr.jitter(frame, pix, centre)
        fx, fy = px + jx.astype(np.float64), py + jy.astype(np.float64)
        o, d = rows[:, 0:3], rows[:, 4:7]
        assert not rows[:, 3].any() and not rows[:, 7].any(), "words 3 and 7 are zero"
        _, _, has = m.rays(fx, fy)
        assert np.array_equal(np.any(d != 0, axis=1), has), "which pixels have a ray"
        if kind == cr.FISHEYE:
            assert 0 < has.sum() < W * H and np.array_equal(bits(o[~has]), bits(np.tile(np.array(list(cam.pos), np.float32), ((~has).sum(), 1))))
        else:
            assert has.all()
        length = np.linalg.norm(d[has].astype(np.float64), axis=1)
        assert np.abs(length - 1).max() <= UNIT_BOUND, np.abs(length - 1).max()
        gx, gy = m.pixel_coords(o, d)
        ex, ey = np.abs(gx - fx), np.abs(gy - fy)
        if kind == cr.EQUIRECT:
            ex = np.minimum(ex, W - ex)              # column 0 meets column W - 1
            past_pole = fy <= 0                      # the latitude is clamped at the pole, where the longitude is lost
            ey = np.where(past_pole, np.abs(gy), ey)
            ex = np.where(past_pole, 0.0, ex)
            assert centre or past_pole.sum() > 0
        print(f"model {kind} {W}x{H} frame {frame} centre {centre}: {ex[has].max():.2e}, {ey[has].max():.2e} pixel off")
        assert ex[has].max() <= PIXEL_BOUND and ey[has].max() <= PIXEL_BOUND
    if not centre:
        assert not np.array_equal(rows, generate(t, cam, cm, 7)), "frames 7 and 8 draw different jitter"


# ---------------------------------------------------------------------------------------------------- 5: thin lens
def test_thin_lens_closed_aperture(t):
    W, H = 37, 23
    cam = tilted(W, H)
    cm = g.camera_model("thinlens", W, H, lens_radius=0.0, focus_dist=3.0)
    rows = generate(t, cam, cm, 7)
    pix, px, py = cr.pixel_grid(W, H)
    jx, jy = cr.jitter(7, pix)
    fx, fy = px + jx.astype(np.float64), py + jy.astype(np.float64)
    assert np.array_equal(bits(rows[:, 0:3]), bits(np.tile(np.array(list(cam.pos), np.float32), (W * H, 1)))), "o == pos as bits"
    pin = cr.Model(cam, cr.PINHOLE, W, H)
    gx, gy = pin.pixel_coords(rows[:, 0:3], rows[:, 4:7])
    assert np.abs(gx - fx).max() <= PIXEL_BOUND and np.abs(gy - fy).max() <= PIXEL_BOUND
    hole = generate(t, cam, g.camera_model("pinhole", W, H), 7)
    hx, hy = pin.pixel_coords(hole[:, 0:3], hole[:, 4:7])
    assert np.abs(gx - hx).max() <= PIXEL_BOUND and np.abs(gy - hy).max() <= PIXEL_BOUND


def test_thin_lens_open_aperture(t):
    W, H, R, F = 37, 23, 0.2, 3.0
    cam = tilted(W, H, pos=(0.0, 0.0, 0.0))
    cm = g.camera_model("thinlens", W, H, lens_radius=R, focus_dist=F)
    m = cr.Model.of(cam, cm)
    pix, px, py = cr.pixel_grid(W, H)
    offsets = {}
    for frame in (7, 8):
        rows = generate(t, cam, cm, frame)
        o, d = rows[:, 0:3].astype(np.float64), rows[:, 4:7].astype(np.float64)
        jx, jy = cr.jitter(frame, pix)
        pf = m.focus_point(px + jx.astype(np.float64), py + jy.astype(np.float64))
        rel = o - m.pos
        assert np.linalg.norm(rel, axis=1).max() <= R * (1 + 2.0 ** -20)
        assert np.abs(rel @ m.front).max() <= 2.0 ** -20 * R
        tt = np.einsum("ij,ij->i", pf - o, d) / np.einsum("ij,ij->i", d, d)
        miss = np.linalg.norm(o + tt[:, None] * d - pf, axis=1)
        print(f"frame {frame}: the lines pass pf at {miss.max():.2e}")
        assert miss.max() <= 1e-5 * F
        lx, ly = rel @ m.right, rel @ m.up
        assert abs(lx.mean()) <= 5 * R / (2 * np.sqrt(W * H)) and abs(ly.mean()) <= 5 * R / (2 * np.sqrt(W * H))
        assert np.hypot(lx, ly).max() > 0.9 * R, "the disk is filled to its edge"
        # the lens stream: draws 0 and 1 of (frame ^ PT_CAM_LENS_KEY, pixel)
        wx, wy = m.lens_offset(*cr.draws(frame, pix, cr.LENS_KEY))
        assert np.abs(lx - wx).max() <= 1e-5 * R and np.abs(ly - wy).max() <= 1e-5 * R
        offsets[frame] = np.stack([lx, ly], 1)
    assert not np.allclose(offsets[7], offsets[8], atol=1e-3)


# ---------------------------------------------------------------------------------------------------- 6: equirect through the environment lookup
def test_equirect_round_trip_through_the_environment_lookup():
    """A 16x8 map whose texel (x, y) is (x, y, 1), laid out in the camera's basis and looked up with PT_ENV_NEAREST along the
    generated rays: every pixel of rows 1..7 gets its own texel back, through code that shares nothing with the generator (atan2f
    against sincosf).  A jitter draw of exactly 1.0 would sit on the texel edge; the restatement says the frame has none."""
    W, H, frame = 16, 8, 7
    cam = tilted(W, H)
    pix, px, py = cr.pixel_grid(W, H)
    u0, u1 = cr.draws(frame, pix)
    assert int((u0 == 1).sum() + (u1 == 1).sum()) == 0, "a draw on the texel edge: choose another frame"
    tex = np.zeros((H, W, 3), np.float32)
    tex[..., 0], tex[..., 1], tex[..., 2] = px.reshape(H, W), py.reshape(H, W), 1.0
    tr = g.PathTracer(0)
    try:
        tr.upload_environment(tex, front=tuple(cam.front), right=tuple(cam.right), up=tuple(cam.up), filter=g.ENV_NEAREST)
        rays, out = tr.malloc(32 * W * H), tr.malloc(12 * W * H)
        for centre in (False, True):
            tr.camera_rays(cam, g.camera_model("equirect", W, H, centre=centre), frame, rays.ptr)
            tr.eval_environment(rays.ptr, W * H, out.ptr)   # no sync in between: ordered on the stream
            tr.sync()
            got = out.download(np.float32, (H, W, 3))
            assert np.array_equal(got[1:], tex[1:]), f"centre {centre}: {np.argwhere(np.any(got[1:] != tex[1:], axis=-1))[:6].tolist()}"
        rays.free()
        out.free()
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------- 7: fisheye
def test_fisheye_circle(t):
    W, H = 16, 8
    cam = tilted(W, H)
    f = np.array(list(cam.front), np.float64)
    pixel_angle = (np.pi / 2) / (min(W, H) / 2.0)   # what one pixel subtends: (fov / 2) / Rpx
    for centre in (True, False):
        rows = generate(t, cam, g.camera_model("fisheye", W, H, centre=centre, fisheye_fov=np.pi), 7).reshape(H, W, 8)
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert np.array_equal(bits(rows[y, x]), bits(np.array(list(cam.pos) + [0, 0, 0, 0, 0], np.float32))), (x, y)
        d = rows[H // 2, W // 2, 4:7].astype(np.float64)   # offsets (0.5, 0.5) + jitter from the centre
        angle = np.arccos(np.clip(d @ f / np.linalg.norm(f), -1, 1))
        assert 0 < angle <= pixel_angle * (1.0 if centre else np.sqrt(2.0)), angle
        # the image circle has radius min(W, H) / 2 = 4 pixels about the image centre
        inside = np.any(rows[..., 4:7] != 0, axis=-1)
        pix, px, py = cr.pixel_grid(W, H)
        jx, jy = cr.jitter(7, pix, centre)
        rho = np.hypot(px + jx - 7.5, py + jy - 3.5).reshape(H, W)
        assert np.array_equal(inside, rho <= 4.0) and inside[3:5, 5:11].all() and 32 < inside.sum() < W * H


# ---------------------------------------------------------------------------------------------------- 8: errors, nothing written
def test_errors_in_order_and_nothing_written(t):
    W, H = 37, 23
    lib, cam = g._abi.ptmi(), golden_camera(W, H)
    n = 64
    buf = t.malloc(32 * (n + 1))
    fill = np.full((n + 1, 8), CANARY, np.float32)
    buf.upload(fill)

    def call(cam_=cam, n_=n, first=0, rays=buf.ptr, pixels=None, **fields):
        cm = g.camera_model(fields.pop("model", g.CAM_PINHOLE), fields.pop("width", W), fields.pop("height", H))
        for k, v in fields.items():
            setattr(cm, k, v)
        rc = lib.pt_camera_rays(t._ctx, C.byref(cam_) if cam_ is not None else None, C.byref(cm), 7, pixels, n_, first, rays)
        return rc, lib.pt_last_error(t._ctx).decode()

    def untouched():
        t.sync()
        return np.array_equal(bits(buf.download(np.float32, (n + 1, 8))), bits(fill))

    assert lib.pt_camera_rays(None, None, None, 7, None, 0, 0, None) == -1                                 # 1: NULL ctx, even with n == 0
    assert lib.pt_camera_rays(t._ctx, None, None, 7, None, 0, 0, None) == 0                                 # 2: n == 0 before the pointers
    assert call(n_=0, model=99)[0] == 0 and call(n_=0, width=0)[0] == 0 and untouched()
    assert call(cam_=None, model=99)[0] == -1 and "null" in call(cam_=None, model=99)[1]                   # 3 before 4
    assert lib.pt_camera_rays(t._ctx, C.byref(cam), None, 7, None, n, 0, buf.ptr) == -1
    assert call(rays=None, model=99)[0] == -1 and "null" in call(rays=None, model=99)[1]
    for model in (-1, 5, 99):                                                                              # 4 before 5
        rc, msg = call(model=model, width=1)
        assert rc == -1 and "model" in msg, msg
    rc, msg = call(flags=2, width=1)
    assert rc == -1 and "flag" in msg, msg
    for wh in (dict(width=1), dict(height=1), dict(width=-4), dict(width=65536, height=65536)):            # 5 before 6
        rc, msg = call(n_=2 ** 32, **wh)
        assert rc == -1 and "width" in msg, (wh, msg)
    rc, msg = call(n_=2 ** 32, first=5)                                                                    # 6 before 7
    assert rc == -1 and "2^32" in msg, msg
    for first, n_ in ((W * H - n + 1, n), (W * H, 1), (2 ** 64 - 1, 2), (0, W * H + 1)):                   # 7 before 8
        rc, msg = call(first=first, n_=n_, model=g.CAM_ORTHO, ortho_height=-1.0)
        assert rc == -1 and "first_pixel" in msg, (first, n_, msg)
    nan, inf = float("nan"), float("inf")
    bad = [(g.CAM_THIN_LENS, dict(lens_radius=-0.1, focus_dist=1.0)), (g.CAM_THIN_LENS, dict(lens_radius=nan, focus_dist=1.0)),
           (g.CAM_THIN_LENS, dict(lens_radius=inf, focus_dist=1.0)), (g.CAM_THIN_LENS, dict(lens_radius=0.1, focus_dist=0.0)),
           (g.CAM_THIN_LENS, dict(lens_radius=0.1, focus_dist=inf)), (g.CAM_THIN_LENS, dict(lens_radius=0.1, focus_dist=nan)),
           (g.CAM_ORTHO, dict(ortho_height=0.0)), (g.CAM_ORTHO, dict(ortho_height=-2.0)), (g.CAM_ORTHO, dict(ortho_height=nan)), (g.CAM_ORTHO, dict(ortho_height=inf)),
           (g.CAM_FISHEYE, dict(fisheye_fov=0.0)), (g.CAM_FISHEYE, dict(fisheye_fov=-1.0)), (g.CAM_FISHEYE, dict(fisheye_fov=6.2832)),
           (g.CAM_FISHEYE, dict(fisheye_fov=nan)), (g.CAM_FISHEYE, dict(fisheye_fov=inf))]
    for model, fields in bad:                                                                              # 8
        rc, msg = call(model=model, **fields)
        assert rc == -1 and msg.startswith("pt_camera_rays:"), (model, fields, msg)
    assert untouched()
    # the parameters of the other models are ignored; the ends of the ranges are valid
    junk = dict(lens_radius=nan, focus_dist=-1.0, ortho_height=nan, fisheye_fov=-3.0)
    for model in (g.CAM_PINHOLE, g.CAM_EQUIRECT):
        assert call(model=model, **junk)[0] == 0
    assert call(model=g.CAM_FISHEYE, fisheye_fov=float(np.float32(2 * np.pi)), lens_radius=nan, focus_dist=nan, ortho_height=nan)[0] == 0
    assert call(model=g.CAM_THIN_LENS, lens_radius=0.0, focus_dist=1e-3, ortho_height=nan, fisheye_fov=nan)[0] == 0
    assert call(first=W * H - n, model=g.CAM_ORTHO, ortho_height=1e-3, lens_radius=nan, focus_dist=nan, fisheye_fov=nan)[0] == 0
    # a list lifts rule 7 (its indices are checked on the device)
    lst = t.malloc(4 * n)
    lst.upload(np.arange(n, dtype=np.uint32))
    assert call(first=2 ** 40, pixels=lst.ptr)[0] == 0
    t.sync()
    got = buf.download(np.float32, (n + 1, 8))
    assert np.all(got[n] == CANARY) and np.array_equal(bits(got[:n]), bits(orc.primary_rays(cam, W, H, frame=7)[:n]))
    lst.free()
    buf.free()


def test_camera_rays_timing(t):
    W, H = 37, 23
    buf = t.malloc(32 * W * H)
    t.set_option(g.OPT_TIMING, 1)
    try:
        t.camera_rays(golden_camera(W, H), g.camera_model("fisheye", W, H), 7, buf.ptr)
        assert 0 < t.last_kernel_ms() < 50
    finally:
        t.set_option(g.OPT_TIMING, 0)
        buf.free()


# ---------------------------------------------------------------------------------------------------- 9: pt_app --camera
def read_pfm(path, W, H):
    raw = open(path, "rb").read()
    assert raw[:2] == b"PF"
    return np.frombuffer(raw[-W * H * 12:], "<f4").reshape(H, W, 3)


def run_app(args):
    r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh")] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]


def test_pt_app_camera(tmp_path):
    """--camera pinhole writes the bytes a run without --camera writes; --camera fisheye runs and leaves --bk outside its circle.
    A .pfm takes pt_render_rays' HDR mode, while pt_render's accumulator is a clamped mean, so equal bytes need samples that never
    exceed 1.  The 37x23 pair has that for a plain reason: the app's camera has dist = H / 60 = 0 there, no ray has a direction
    and every pixel is --bk on both sides.  The 160x120 pair is the one that looks at something: without the sphere room no
    surface emits, a path returns black or, where it leaves the open box, the bare --bk = 1, and the mean of three such samples
    stays within 0..1 whatever the clamp."""
    W, H = 37, 23
    a, b = tmp_path / "a.pfm", tmp_path / "b.pfm"
    run_app(["--camera", "pinhole", "--width", W, "--height", H, "--frames", 3, "--out", a])
    run_app(["--width", W, "--height", H, "--frames", 3, "--out", b])
    assert a.read_bytes() == b.read_bytes()
    W2, H2 = 160, 120
    c, d = tmp_path / "c.pfm", tmp_path / "d.pfm"
    run_app(["--camera", "pinhole", "--width", W2, "--height", H2, "--frames", 3, "--no-spheres", "--out", c])
    run_app(["--width", W2, "--height", H2, "--frames", 3, "--no-spheres", "--out", d])
    img = read_pfm(d, W2, H2)
    assert img.max() <= 1.0 and len(np.unique(img)) >= 4, "the pair must look at something, and never above 1"
    assert c.read_bytes() == d.read_bytes()
    # fisheye: the corners lie outside the image circle
    bk = (0.25, 0.5, 0.75)
    e = tmp_path / "e.pfm"
    run_app(["--camera", "fisheye", "--fisheye-deg", 180, "--width", W, "--height", H, "--frames", 3, "--bk", *bk, "--out", e])
    img = read_pfm(e, W, H)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert np.array_equal(img[y, x], np.array(bk, np.float32)), (x, y, img[y, x])
    assert np.any(np.any(img != np.array(bk, np.float32), axis=-1)), "inside the circle the room is seen"
    # the refusals of --equirect
    for extra in (["--equirect"], ["--gpus", 2], ["--denoise-out", tmp_path / "x.png"], ["--pan-deg", 1]):
        r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--camera", "ortho"] + [str(v) for v in extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--camera does not combine" in r.stderr, (extra, r.stderr[-300:])
    r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--camera", "wide"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--camera" in r.stderr
