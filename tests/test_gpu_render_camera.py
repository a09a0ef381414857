"""pt_render_camera — a camera model's frame in one call: each sample's jittered ray is made in the path kernel (extension,
DESIGN.md §10 f17; contract in include/ptmi.h).

The reference is the loop the call replaces, PathTracer.render_camera: per sample one pt_camera_rays and a one-sample
pt_render_rays.  Every comparison is bitwise (gpu_support.bits), every output buffer is pre-filled with a canary and has one
spare row that must stay untouched.  Sizes are those of test_gpu_camera.py: odd, no multiple of 64 lanes, fewer slots than one
queue chunk of a busy device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
from gpu_support import bits, golden_camera, setup_scene
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
W, H = 37, 23
SPP = 3
CANARY = -7.0
BK = (0.125, 0.75, 0.375)
KINDS = ["pinhole", "thinlens", "ortho", "fisheye", "equirect"]
INVALID, NO_SCENE, UNSUPPORTED = -1, -3, -5


def model_kwargs(kind):
    """The model parameters test_gpu_camera.py judges the generator with."""
    return {"thinlens": dict(lens_radius=0.2, focus_dist=3.0), "ortho": dict(ortho_height=10.0), "fisheye": dict(fisheye_fov=2.5)}.get(kind, {})


def tilted(w, h, pos=(0.5, -0.25, 1.0)):
    """An orthonormal basis that is no permutation of the axes, looking into the room."""
    return make_camera(w, h, pos=pos, front=(0.3, -0.2, -1.0), roll=0.4, fov=0.9)


def params(w=W, h=H, flags=0, frame=7, sample_index=1, depth=4):
    p = g.default_params(w, h, depth=depth)
    p.frame, p.sample_index, p.flags = frame, sample_index, flags
    p.bk_color[:] = BK
    return p


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)   # what pt_render runs beside the call; the call itself does not read the option
    setup_scene(tr, "room", False)
    yield tr
    tr.close()


def fused(t, cam, cm, p, spp=SPP, hdr=False, n=None, first_pixel=0, pixels=None, init=None):
    """render_model into a buffer of n + 1 rows pre-filled with CANARY (or `init` in its first n): the n rows."""
    if n is None:
        n = len(pixels) if pixels is not None else cm.width * cm.height - first_pixel
    out = t.malloc(12 * (n + 1))
    fill = np.full((n + 1, 3), CANARY, np.float32)
    if init is not None:
        fill[:n] = init
    out.upload(fill)
    lst = None
    if pixels is not None:
        lst = t.malloc(4 * max(len(pixels), 1))
        lst.upload(np.asarray(pixels, np.uint32))
    t.render_model(cam, cm, p, out.ptr, spp=spp, hdr=hdr, n=n, first_pixel=first_pixel, pixels_ptr=lst.ptr if lst else None)
    t.sync()
    got = out.download(np.float32, (n + 1, 3))
    out.free()
    if lst:
        lst.free()
    assert np.all(got[n] == CANARY), "the row behind the buffer was written"
    return got[:n]


def loop(t, cam, cm, p, spp=SPP, hdr=False):
    """render_camera, the loop of (pt_camera_rays, one-sample pt_render_rays): the whole frame's rows."""
    n = cm.width * cm.height
    rays, out = t.malloc(32 * n), t.malloc(12 * (n + 1))
    out.upload(np.full((n + 1, 3), CANARY, np.float32))
    t.render_camera(cam, cm, p, out.ptr, rays.ptr, spp=spp, hdr=hdr)
    t.sync()
    got = out.download(np.float32, (n + 1, 3))
    rays.free()
    out.free()
    assert np.all(got[n] == CANARY)
    return got[:n]


def same(got, want, what):
    diff = np.any(bits(got) != bits(want), axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {len(diff)} rows differ, first {np.flatnonzero(diff)[:5].tolist()}"


def miss_sample(p, spp, hdr):
    """What spp samples of bk_color fold to from sample_index on, in the fold's binary32 arithmetic (include/ptmi.h)."""
    a = np.zeros(3, np.float32)
    bk = np.array(list(p.bk_color), np.float32)
    for s in range(spp):
        N = p.sample_index + s
        a = (a * np.float32(N - 1) + bk) * (np.float32(1.0) / np.float32(N)) if N > 1 else bk.copy()
        if not hdr:
            a = np.clip(a, np.float32(0), np.float32(1))
    return a


# ---------------------------------------------------------------------------------------------------- 1: the fused call is the loop
@pytest.mark.parametrize("size", [(37, 23), (16, 8)], ids=["37x23", "16x8"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_call_equals_the_loop(t, kind, size):
    """(a) of the header, for the five models, under the default flags and FLAGS_SMALLPT, clamped and HDR."""
    w, h = size
    cam, cm = tilted(w, h), g.camera_model(kind, w, h, **model_kwargs(kind))
    for flags in (0, g.FLAGS_SMALLPT):
        for hdr in (False, True):
            p = params(w, h, flags)
            want = loop(t, cam, cm, p, hdr=hdr)
            got = fused(t, cam, cm, p, hdr=hdr)
            assert len(np.unique(want, axis=0)) > 20, "the frame must look at something"
            same(got, want, f"{kind} {w}x{h} flags {flags:#x} hdr {hdr}")
    centred = g.camera_model(kind, w, h, centre=True, **model_kwargs(kind))
    same(fused(t, cam, centred, params(w, h)), loop(t, cam, centred, params(w, h)), f"{kind} under CAMF_CENTRE")


# ---------------------------------------------------------------------------------------------------- 2: the pinhole is pt_render
@pytest.mark.parametrize("flags", [0, g.FLAGS_SMALLPT], ids=["default", "smallpt"])
def test_pinhole_equals_pt_render(t, flags):
    """(b): pinhole, first_pixel 0, n = W * H, clamped, is launch_kernel(spp = 3)'s accumulator on the same context."""
    cam, p = golden_camera(W, H), params(flags=flags)
    acc, rgba = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, SPP)
    t.sync()
    ref = acc.download(np.float32, (W * H, 3))
    acc.free()
    rgba.free()
    assert len(np.unique(ref, axis=0)) > 100
    same(fused(t, cam, g.camera_model("pinhole", W, H), p), ref, "pinhole against pt_render")


# ---------------------------------------------------------------------------------------------------- 3: NEE, MIS, a map, Woop records
def test_nee_mis_environment_woop(t):
    """Thin lens against the loop under FLAG_NEE | FLAG_COSINE_DIFF and with FLAG_MIS on the room (every sphere of it emits), on a
    context whose environment map is a light (with FLAG_MISS_KEEPS_PATH; without NEE its lookup), and over Woop records.  With a
    tree that the wide walk holds these calls run the words (wide, none), (wide, none, NEE), (wide, none, NEE, MIS), (wide, lookup),
    (wide, light, NEE), (wide, light, NEE, MIS), (Woop, none) and (Woop, none, NEE) of rays_exists.  Not reached by a small scene:
    the seven words of the unified binary walk (PT_OPT_WALK 0 / 1 or a tree too deep for the wide walk; the loop itself is the one
    tests/test_gpu_render_rays.py runs over those walks), (wide, lookup, NEE), and the three Woop words with a map: 11 of 19."""
    cam, cm = tilted(W, H), g.camera_model("thinlens", W, H, **model_kwargs("thinlens"))
    nee = g.FLAG_NEE | g.FLAG_COSINE_DIFF
    for flags in (nee, nee | g.FLAG_MIS):
        for hdr in (False, True):
            p = params(flags=flags)
            want = loop(t, cam, cm, p, hdr=hdr)
            assert len(np.unique(want, axis=0)) > 20
            same(fused(t, cam, cm, p, hdr=hdr), want, f"flags {flags:#x} hdr {hdr}")
    sky = g.PathTracer(0)
    try:
        setup_scene(sky, "box", False)   # the open box alone: paths leave it
        yy, xx = np.mgrid[0:8, 0:16].astype(np.float32)
        tex = np.stack([0.2 + xx / 16, 0.1 + yy / 8, 0.5 + 0 * xx], -1).astype(np.float32)
        tex[2, 5] = (30.0, 25.0, 20.0)   # a small sun
        sky.upload_environment(tex, light=True)
        assert sky.environment_is_light()
        for flags in (0, g.FLAG_MISS_KEEPS_PATH, nee | g.FLAG_MISS_KEEPS_PATH, nee | g.FLAG_MIS | g.FLAG_MISS_KEEPS_PATH):
            p = params(flags=flags)
            want = loop(sky, cam, cm, p, hdr=True)
            assert len(np.unique(want, axis=0)) > 20
            same(fused(sky, cam, cm, p, hdr=True), want, f"environment light, flags {flags:#x}")
    finally:
        sky.close()
    woop = g.PathTracer(0)
    try:
        woop.set_option(g.OPT_TRI_TEST, 1)
        setup_scene(woop, "room", False)
        for flags in (0, nee):
            p = params(flags=flags)
            want = loop(woop, cam, cm, p)
            assert len(np.unique(want, axis=0)) > 20
            same(fused(woop, cam, cm, p), want, f"Woop records, flags {flags:#x}")
        # PT_FLAG_MIS over Woop records: pt_render_rays' refusal, in this call's name, nothing written
        lib = g._abi.ptmi()
        out = woop.malloc(12 * 8)
        out.upload(np.full((8, 3), CANARY, np.float32))
        p = params(flags=nee | g.FLAG_MIS)
        rc = lib.pt_render_camera(woop._ctx, C.byref(cam), C.byref(cm), None, 8, 0, out.ptr, C.byref(p), 1, g._abi.RAYS_CLAMPED)
        msg = lib.pt_last_error(woop._ctx).decode()
        woop.sync()
        assert rc == UNSUPPORTED and msg.startswith("pt_render_camera:") and "PT_FLAG_MIS" in msg, (rc, msg)
        assert np.all(out.download(np.float32, (8, 3)) == CANARY)
        out.free()
    finally:
        woop.close()


# ---------------------------------------------------------------------------------------------------- 4: the pixel list
@pytest.mark.parametrize("kind", ["fisheye", "thinlens"])
def test_pixel_list(t, kind):
    """(c): a listed pixel has the bits it has in the full frame — the path's stream is the pixel's, not the row's."""
    cam, cm, p = tilted(W, H), g.camera_model(kind, W, H, **model_kwargs(kind)), params()
    full = fused(t, cam, cm, p)
    perm = np.random.default_rng(11).permutation(W * H).astype(np.uint32)
    got = fused(t, cam, cm, p, pixels=perm)
    same(got, full[perm], f"{kind}: a permutation of all pixels")
    assert not np.array_equal(bits(got), bits(full))
    # repeats, and indices past the image among valid ones
    seen = [8 * W + 15, 11 * W + 18, 14 * W + 20]   # near the image centre: inside the fisheye's circle too
    lst = np.array([seen[0], W * H, seen[1], seen[0], W * H + 5, 2 ** 32 - 1, W * H - 1, seen[2], seen[2], seen[1]], np.uint32)
    past = lst >= W * H
    for hdr in (False, True):
        whole = fused(t, cam, cm, p, hdr=hdr)
        rows = fused(t, cam, cm, p, hdr=hdr, pixels=lst)
        same(rows[~past], whole[lst[~past]], f"{kind}: listed pixels, hdr {hdr}")
        same(rows[past], np.tile(miss_sample(p, SPP, hdr), (int(past.sum()), 1)), f"{kind}: indices past the image, hdr {hdr}")
    assert np.array_equal(miss_sample(p, 1, False), np.array(BK, np.float32))
    assert not np.any(np.all(whole[seen] == miss_sample(p, SPP, True), axis=1)), "the valid pixels see the room"


# ---------------------------------------------------------------------------------------------------- 5: splits
@pytest.mark.parametrize("kind", ["thinlens", "equirect"])
def test_splits(t, kind):
    cam, cm, p = tilted(W, H), g.camera_model(kind, W, H, **model_kwargs(kind)), params()
    for hdr in (False, True):
        whole = fused(t, cam, cm, p, hdr=hdr)
        # 2 + 1 samples over two calls, frame and sample_index advanced alike
        first = fused(t, cam, cm, p, spp=2, hdr=hdr)
        q = params(frame=p.frame + 2, sample_index=p.sample_index + 2)
        same(fused(t, cam, cm, q, spp=1, hdr=hdr, init=first), whole, f"{kind}: 2 + 1 samples, hdr {hdr}")
        # the rows in two parts by first_pixel
        k = (W * H) // 2 - 3
        parts = np.concatenate([fused(t, cam, cm, p, hdr=hdr, n=k), fused(t, cam, cm, p, hdr=hdr, first_pixel=k)])
        same(parts, whole, f"{kind}: parts by first_pixel, hdr {hdr}")
    # a running mean under way: N = 5 .. 7 over a given accumulator
    init = np.random.default_rng(3).random((W * H, 3), dtype=np.float32)
    q = params(sample_index=5)
    a = fused(t, cam, cm, q, init=init)
    b = fused(t, cam, cm, params(frame=8, sample_index=6), spp=2, init=fused(t, cam, cm, q, spp=1, init=init))
    same(b, a, f"{kind}: 1 + 2 samples from N = 5")
    assert not np.array_equal(a, fused(t, cam, cm, p))
    black = fused(t, cam, cm, params(depth=0))
    assert not black.any(), "depth 0 folds black samples"


# ---------------------------------------------------------------------------------------------------- 6: fisheye, outside the circle
def test_fisheye_outside_the_circle(t):
    w, h = 16, 8
    cam = tilted(w, h)
    cm = g.camera_model("fisheye", w, h, centre=True, fisheye_fov=np.pi)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (np.hypot(xx - 7.5, yy - 3.5) <= 4.0).reshape(-1)   # the circle of radius min(W, H) / 2 about the image centre
    assert 32 < inside.sum() < w * h
    for flags in (0, g.FLAGS_SMALLPT):
        for hdr in (False, True):
            p = params(w, h, flags)
            got = fused(t, cam, cm, p, hdr=hdr)
            same(got[~inside], np.tile(miss_sample(p, SPP, hdr), (int((~inside).sum()), 1)), f"outside the circle, flags {flags:#x}")
            assert not np.any(np.all(got[inside] == miss_sample(p, SPP, hdr), axis=1)), "inside the circle the room is seen"
    one = fused(t, cam, cm, params(w, h), spp=1)
    assert np.array_equal(one[~inside], np.tile(np.array(BK, np.float32), (int((~inside).sum()), 1))), "exactly bk_color"


# ---------------------------------------------------------------------------------------------------- 7: call history
def test_between_two_pt_render_calls(t):
    """The call shares the context's sample buffer and queue counters with pt_render: issued between two pt_render calls of a
    larger frame, without a sync, it changes neither their bits nor its own."""
    W2, H2 = 96, 64
    cam2, p2 = golden_camera(W2, H2), params(W2, H2)
    cam, cm, p = tilted(W, H), g.camera_model("thinlens", W, H, **model_kwargs("thinlens")), params()
    acc, rgba = t.alloc_frame(W2, H2)
    t.launch_kernel(acc.ptr, rgba.ptr, cam2, p2, 4)
    t.sync()
    frame = acc.download(np.float32, (H2, W2, 3))
    own = fused(t, cam, cm, p)
    acc2, rgba2 = t.alloc_frame(W2, H2)
    out = t.malloc(12 * (W * H + 1))
    out.upload(np.full((W * H + 1, 3), CANARY, np.float32))
    acc.zero()
    t.launch_kernel(acc.ptr, rgba.ptr, cam2, p2, 4)
    t.render_model(cam, cm, p, out.ptr, spp=SPP)
    t.launch_kernel(acc2.ptr, rgba2.ptr, cam2, p2, 4)
    t.sync()
    a, b, mid = acc.download(np.float32, (H2, W2, 3)), acc2.download(np.float32, (H2, W2, 3)), out.download(np.float32, (W * H + 1, 3))
    for buf in (acc, rgba, acc2, rgba2, out):
        buf.free()
    assert frame.any() and np.array_equal(bits(a), bits(frame)) and np.array_equal(bits(b), bits(frame))
    same(mid[:-1], own, "between two pt_render calls")
    assert np.all(mid[-1] == CANARY)


# ---------------------------------------------------------------------------------------------------- 8: the argument rules, in order
def test_errors_in_order_and_nothing_written(t):
    lib, cam = g._abi.ptmi(), golden_camera(W, H)
    n = 64
    buf = t.malloc(12 * (n + 1))
    fill = np.full((n + 1, 3), CANARY, np.float32)
    buf.upload(fill)
    good = params()

    def call(ctx=t, cam_=cam, n_=n, first=0, out=buf.ptr, pixels=None, p=good, spp=1, mode=g._abi.RAYS_HDR, no_cm=False, **fields):
        cm = g.camera_model(fields.pop("model", g.CAM_PINHOLE), fields.pop("width", W), fields.pop("height", H))
        for k, v in fields.items():
            setattr(cm, k, v)
        rc = lib.pt_render_camera(ctx._ctx, C.byref(cam_) if cam_ is not None else None, None if no_cm else C.byref(cm), pixels, n_, first, out,
                                  C.byref(p) if p is not None else None, spp, mode)
        return rc, lib.pt_last_error(ctx._ctx).decode()

    def refused(result, code, word):
        rc, msg = result
        assert rc == code and msg.startswith("pt_render_camera:") and word in msg, (rc, msg, word)

    def broken(**fields):
        q = params()
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    # 1: NULL ctx, whatever else
    assert lib.pt_render_camera(None, None, None, None, 0, 0, None, None, 0, 7) == INVALID and "null ctx" in lib.pt_last_error(None).decode()
    # 2: no scene, before "nothing to do" and before the pointers
    empty = g.PathTracer(0)
    try:
        refused(call(ctx=empty, n_=0, spp=0, cam_=None, out=None, p=None, mode=7), NO_SCENE, "no scene")
    finally:
        empty.close()
    # 3: n == 0 or spp == 0: PT_OK before the pointers, the mode and the model
    assert call(n_=0, cam_=None, out=None, p=None, mode=7, model=99)[0] == 0 and call(spp=0, cam_=None, no_cm=True, out=None, p=None, mode=7)[0] == 0
    # 4: the pointers, before the mode
    for null in (dict(cam_=None), dict(no_cm=True), dict(out=None), dict(p=None)):
        refused(call(mode=7, **null), INVALID, "null argument")
    # 5: the mode, before the model
    refused(call(mode=7, model=99), INVALID, "mode")
    refused(call(mode=-1), INVALID, "mode")
    # 6: pt_camera_rays' checks, in its order
    for model in (-1, 5, 99):
        refused(call(model=model, flags=2), INVALID, "unknown camera model")
    refused(call(flags=2, width=1), INVALID, "flag")
    for wh in (dict(width=1), dict(height=1), dict(width=-4), dict(width=65536, height=65536)):
        refused(call(n_=2 ** 32, **wh), INVALID, "width")
    refused(call(n_=2 ** 32, first=5), INVALID, "2^32")
    for first, n_ in ((W * H - n + 1, n), (W * H, 1), (2 ** 64 - 1, 2), (0, W * H + 1)):
        refused(call(first=first, n_=n_, model=g.CAM_ORTHO, ortho_height=-1.0), INVALID, "first_pixel")
    nan, inf = float("nan"), float("inf")
    zero_index = broken(sample_index=0)
    for model, fields in ((g.CAM_THIN_LENS, dict(lens_radius=-0.1, focus_dist=1.0)), (g.CAM_THIN_LENS, dict(lens_radius=0.1, focus_dist=nan)),
                          (g.CAM_ORTHO, dict(ortho_height=0.0)), (g.CAM_ORTHO, dict(ortho_height=inf)),
                          (g.CAM_FISHEYE, dict(fisheye_fov=6.2832)), (g.CAM_FISHEYE, dict(fisheye_fov=nan))):
        rc, msg = call(model=model, p=zero_index, **fields)                     # ... before pt_render_rays' own rules
        assert rc == INVALID and msg.startswith("pt_render_camera:") and "sample_index" not in msg, msg
    # 7: pt_render_rays' remaining rules
    refused(call(p=zero_index, model=g.CAM_ORTHO, ortho_height=1.0, lens_radius=nan, fisheye_fov=-3.0), INVALID, "sample_index")   # other models' parameters are ignored
    refused(call(p=broken(tri_mat=9, flags=g.FLAG_NEE)), INVALID, "triangle material")
    refused(call(p=broken(flags=g.FLAG_NEE)), INVALID, "PT_FLAG_NEE needs PT_FLAG_COSINE_DIFF")
    refused(call(p=broken(flags=g.FLAG_MIS | g.FLAG_COSINE_DIFF)), INVALID, "PT_FLAG_MIS needs PT_FLAG_NEE")
    t.sync()
    assert np.array_equal(bits(buf.download(np.float32, (n + 1, 3))), bits(fill)), "a refused call wrote"
    # a list lifts the rule on first_pixel; the call then runs
    lst = t.malloc(4 * n)
    lst.upload(np.arange(n, dtype=np.uint32))
    assert call(first=2 ** 40, pixels=lst.ptr, mode=g._abi.RAYS_CLAMPED)[0] == 0
    t.sync()
    got = buf.download(np.float32, (n + 1, 3))
    assert np.all(got[n] == CANARY)
    same(got[:n], fused(t, cam, g.camera_model("pinhole", W, H), good, spp=1)[:n], "the call after the refusals")
    lst.free()
    buf.free()


def test_timing_covers_the_call(t):
    out = t.malloc(12 * W * H)
    t.set_option(g.OPT_TIMING, 1)
    try:
        t.render_model(tilted(W, H), g.camera_model("fisheye", W, H), params(), out.ptr, spp=SPP)
        assert 0 < t.last_kernel_ms() < 200
    finally:
        t.set_option(g.OPT_TIMING, 0)
        out.free()


# ---------------------------------------------------------------------------------------------------- 9: pt_app --camera
def run_app(args):
    r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh")] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]


@pytest.mark.parametrize("args", [["--camera", "fisheye"], ["--camera", "thinlens", "--aperture", 0.5, "--focus", 30]], ids=["fisheye", "thinlens"])
def test_pt_app_fused_and_loop_write_the_same_file(tmp_path, args):
    """--camera renders through pt_render_camera, --camera-loop through the two-call loop: byte-identical files, HDR and clamped."""
    for ext in ("pfm", "ppm"):
        a, b = tmp_path / f"a.{ext}", tmp_path / f"b.{ext}"
        common = args + ["--width", W, "--height", H, "--frames", 4, "--spp", 3, "--bk", *BK]
        run_app(common + ["--out", a])
        run_app(common + ["--camera-loop", "--out", b])
        assert a.read_bytes() == b.read_bytes(), ext
    if args[1] == "fisheye":
        img = np.frombuffer(a.read_bytes()[-W * H * 3:], np.uint8)
        assert len(np.unique(img)) > 8, "the fisheye frame looks at the room"
    r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--camera-loop"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--camera-loop needs --camera" in r.stderr
