"""GPU tests of pt_render_moments (per-pixel luminance moments kept by the fold) and pt_frame_error against the numpy
restatement of tests/moments_ref.py over the oracle's per-sample colours: bit for bit over scenes, sizes, samples per call and
kernel families; the accumulator untouched; continuation, partitions, overlapped calls, the frame figure, freedom from side
effects and the pt_app options."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import moments_ref as M
from gpu_support import bits, golden_camera

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1
# pixels where the ACCUMULATOR differs from the oracle are the grazing cases of DESIGN.md §4: tests/test_gpu_wide.py allows 40 per
# 2 M pixels, which is 0 at the sizes here
GRAZING_PER_PIXEL = 40 / 2_000_000


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


_scenes = {}


def scene(name, W, H):
    """(mesh, bvh, spheres, camera, params, materials, tri_material): the sphere room over cornell, or cornell_box with its
    material table."""
    if name not in _scenes:
        mesh = g.scene_mesh("cornell" if name == "room" else "cornell_box")
        _scenes[name] = (mesh, g.Bvh(mesh))
    mesh, bvh = _scenes[name]
    if name == "room":
        return mesh, bvh, g.reference_spheres(), golden_camera(W, H), g.default_params(W, H), None, None
    if name == "box-defaults":   # the asset as the library renders it when nothing is changed: default camera and parameters
        return mesh, bvh, None, g.default_camera(W, H), g.default_params(W, H), mesh.materials, mesh.tri_material
    _, _, cam, p = R.cornell_box_scene(W, H)
    return mesh, bvh, None, cam, p, mesh.materials, mesh.tri_material


def install(t, name, W, H):
    mesh, bvh, sph, cam, p, mats, tm = scene(name, W, H)
    t.upload_tri_materials(None, None)
    t.upload_bvh(bvh)           # the oracle walks this very tree
    t.upload_spheres(sph or [])
    if mats is not None:
        t.upload_tri_materials(mats, tm)
    return bvh, sph, cam, p, mats, tm


_refs = {}


def reference(name, W, H, spp, frame, flags=0):
    """(moments, accumulator, display words) of one call from sample_index 1, by the oracle."""
    key = (name, W, H, spp, frame, flags)
    if key not in _refs:
        _, bvh, sph, cam, p, mats, tm = scene(name, W, H)
        p.frame, p.sample_index, p.flags = frame, 1, flags | g.FLAG_WRITE_RGBA
        m, _ = M.oracle_moments(bvh, sph, cam, p, spp, mats, tm)
        acc, rgba, _ = orc.render(bvh, sph, cam, p, spp=spp, materials=mats, tri_material=tm)
        _refs[key] = (m, acc, rgba)
    return _refs[key]


class Frame:
    """accumulator, display words and moments of one frame on the device; the moments start as NaN."""

    def __init__(self, t, W, H):
        self.t, self.W, self.H = t, W, H
        self.acc, self.rgba = t.alloc_frame(W, H)
        self.mom = t.malloc(W * H * 8)
        self.poison()

    def poison(self):
        self.mom.upload(np.full((self.H, self.W, 2), np.nan, np.float32))

    def get(self):
        self.t.sync()
        W, H = self.W, self.H
        return (self.mom.download(np.float32, (H, W, 2)), self.acc.download(np.float32, (H, W, 3)), self.rgba.download(np.uint32, (H, W)))

    def free(self):
        for b in (self.acc, self.rgba, self.mom):
            b.free()


def options(t, kernel, walk):
    t.set_option(g.OPT_KERNEL, kernel)
    t.set_option(g.OPT_WALK, walk)


def restore(t):
    options(t, g.KERNEL_AUTO, 2)


CONFIGS = {"mega": (g.KERNEL_MEGA_BVH2, 2), "persistent": (g.KERNEL_PERSISTENT, 2), "wavefront": (g.KERNEL_WAVEFRONT, 2),
           "persistent-walk0": (g.KERNEL_PERSISTENT, 0)}
SPPS = [1, 3, 4, 8, 16]   # the plain fold (1, 3) and the grouped one with 1, 2 and 4 lanes per pixel (4, 8, 16)
SIZES = [(64, 64), (257, 131)]
FRAME = 7


def render_both(t, name, W, H, spp, flags=0):
    """One call through pt_render_moments, one through pt_render and one through pt_render_moments with a NULL buffer, on the
    context as configured: ((moments, acc, rgba), (acc, rgba) of pt_render, (acc, rgba) of the NULL call)."""
    _, _, cam, p, _, _ = install(t, name, W, H)
    p.frame, p.sample_index, p.flags = FRAME, 1, flags | g.FLAG_WRITE_RGBA
    lib = g._abi.ptmi()
    out = []
    for mode in ("moments", "plain", "null"):
        f = Frame(t, W, H)
        if mode == "moments":
            t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp, moments_ptr=f.mom.ptr)
        elif mode == "plain":
            t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp)
        else:
            assert lib.pt_render_moments(t._ctx, f.acc.ptr, f.rgba.ptr, None, C.byref(cam), C.byref(p), spp) == 0
        out.append(f.get())
        f.free()
    return out


def check_against_reference(got, ref, what):
    gm, ga, gr = got
    rm, ra, rr = ref
    differ = np.any(ga != ra, axis=-1)
    cap = int(GRAZING_PER_PIXEL * differ.size)
    print(f"{what}: {int(differ.sum())} grazing pixels (cap {cap})")
    assert differ.sum() <= cap, f"{what}: the accumulator differs from the oracle in {int(differ.sum())} pixels"
    ok = ~differ
    assert np.array_equal(gr[ok], rr[ok]), what
    bad = np.argwhere(np.any(bits(gm) != bits(rm), axis=-1) & ok)
    assert len(bad) == 0, f"{what}: moments differ in {len(bad)} pixels, first {bad[:3].tolist()}: {gm[tuple(bad[0])]} vs {rm[tuple(bad[0])]}"


# ---------------------------------------------------------------------------------------------------- 1, 2: the moments, the frame
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["room", "box"])
def test_moments_equal_the_reference_and_the_frame_is_pt_renders(t, name, W, H, spp, config):
    options(t, *CONFIGS[config])
    try:
        with_m, plain, null = render_both(t, name, W, H, spp)
    finally:
        restore(t)
    what = f"{name} {W}x{H} spp {spp} {config}"
    check_against_reference(with_m, reference(name, W, H, spp, FRAME), what)
    for other, label in ((plain, "pt_render"), (null, "moments_dev = NULL")):
        assert np.array_equal(bits(with_m[1]), bits(other[1])), f"{what}: accumulator vs {label}"
        assert np.array_equal(with_m[2], other[2]), f"{what}: display words vs {label}"
    assert np.isnan(null[0]).all() and np.isnan(plain[0]).all()   # nobody wrote a buffer that was not passed


@pytest.mark.parametrize("spp", [4, 3])
def test_moments_with_next_event_estimation(t, spp):
    W, H, flags = 64, 64, g.FLAG_NEE | g.FLAG_COSINE_DIFF
    restore(t)
    with_m, plain, null = render_both(t, "room", W, H, spp, flags)
    check_against_reference(with_m, reference("room", W, H, spp, FRAME, flags), f"room NEE spp {spp}")
    assert np.array_equal(bits(with_m[1]), bits(plain[1])) and np.array_equal(with_m[2], plain[2])
    assert np.array_equal(bits(with_m[1]), bits(null[1])) and np.array_equal(with_m[2], null[2])


def test_auto_kernel_with_moments(t):
    """PT_KERNEL_AUTO: the timed trials and the calls after them keep the moments like any other call."""
    W, H, spp = 64, 64, 4
    restore(t)
    _, _, cam, p, _, _ = install(t, "room", W, H)
    ref = reference("room", W, H, spp, FRAME)
    p.frame, p.sample_index, p.flags = FRAME, 1, g.FLAG_WRITE_RGBA
    f = Frame(t, W, H)
    for k in range(7):   # four trials, then the decided layout
        f.poison()
        t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp, moments_ptr=f.mom.ptr)
        check_against_reference(f.get(), ref, f"auto call {k}")
    f.free()


# ---------------------------------------------------------------------------------------------------- 3: continuation
@pytest.mark.parametrize("config", ["persistent", "wavefront", "mega"])
def test_five_plus_seven_samples_equal_twelve(t, config):
    W, H = 64, 64
    options(t, *CONFIGS[config])
    try:
        _, _, cam, p, _, _ = install(t, "room", W, H)
        p.flags = g.FLAG_WRITE_RGBA
        whole, split = Frame(t, W, H), Frame(t, W, H)
        p.frame, p.sample_index = FRAME, 1
        t.launch_kernel(whole.acc.ptr, whole.rgba.ptr, cam, p, 12, moments_ptr=whole.mom.ptr)
        t.launch_kernel(split.acc.ptr, split.rgba.ptr, cam, p, 5, moments_ptr=split.mom.ptr)
        p.frame, p.sample_index = FRAME + 5, 6
        t.launch_kernel(split.acc.ptr, split.rgba.ptr, cam, p, 7, moments_ptr=split.mom.ptr)
        a, b = whole.get(), split.get()
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y))
        check_against_reference(a, reference("room", W, H, 12, FRAME), f"12 samples {config}")
        # a second series from sample_index 1 overwrites what the buffer holds (here: the first series' result)
        p.frame, p.sample_index = FRAME, 1
        t.launch_kernel(split.acc.ptr, split.rgba.ptr, cam, p, 5, moments_ptr=split.mom.ptr)
        p.frame, p.sample_index = FRAME + 5, 6
        t.launch_kernel(split.acc.ptr, split.rgba.ptr, cam, p, 7, moments_ptr=split.mom.ptr)
        c = split.get()
        assert np.array_equal(bits(c[0]), bits(a[0])) and np.array_equal(bits(c[1]), bits(a[1]))
        whole.free()
        split.free()
    finally:
        restore(t)


# ---------------------------------------------------------------------------------------------------- 4: partitions
@pytest.mark.parametrize("config,spp", [("persistent", 3), ("wavefront", 4), ("mega", 1)])
def test_partitions_own_their_pixels_only(t, config, spp):
    W, H = 64, 64
    options(t, *CONFIGS[config])
    try:
        _, _, cam, p, _, _ = install(t, "room", W, H)
        p.frame, p.sample_index, p.flags = FRAME, 1, g.FLAG_WRITE_RGBA
        whole = Frame(t, W, H)
        t.launch_kernel(whole.acc.ptr, whole.rgba.ptr, cam, p, spp, moments_ptr=whole.mom.ptr)
        wm = whole.get()[0]
        whole.free()
        check = np.zeros((H, W), bool)
        p.part_count, p.part_rows = 3, 8
        for part in range(3):
            p.part_index = part
            f = Frame(t, W, H)
            t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp, moments_ptr=f.mom.ptr)
            m = f.get()[0]
            f.free()
            owned = np.repeat(((np.arange(H) // 8) % 3 == part)[:, None], W, axis=1)
            assert np.array_equal(bits(m)[owned], bits(wm)[owned]), part
            assert np.isnan(m[~owned]).all(), part   # the other parts' pixels were not touched
            check |= owned
        assert check.all()
    finally:
        restore(t)


# ---------------------------------------------------------------------------------------------------- 5: overlapped calls
def test_back_to_back_calls_without_host_sync(t):
    W, H = 320, 240
    options(t, g.KERNEL_PERSISTENT, 2)
    t.set_option(g.OPT_OVERLAP, 1)
    try:
        _, _, cam, p, _, _ = install(t, "box", W, H)
        f = Frame(t, W, H)
        t.sync()
        # several calls in a row: the later ones run their path kernels on a side stream (the caller's stream is busy)
        for k in range(4):
            q = g.Params.from_buffer_copy(p)
            q.frame, q.sample_index, q.flags = 40 + k, 1 + k, g.FLAG_WRITE_RGBA
            t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, q, 1, moments_ptr=f.mom.ptr)
        got = f.get()
        f.free()
    finally:
        restore(t)
    check_against_reference(got, reference("box", W, H, 4, 40), "four one-sample calls back to back")


# ---------------------------------------------------------------------------------------------------- 6: pt_frame_error
def off_every_pixel(r, thr):
    """thr, moved up until no pixel's rse lies within 1e-4 relative of it (0 stays: rse >= 0, and 0 is exact on both sides)."""
    while thr > 0 and np.any(np.abs(r - thr) <= 1e-4 * thr):
        thr *= 1.0005
    return thr


@pytest.fixture(scope="module")
def rendered_moments(t):
    W, H, spp = 257, 131, 8
    restore(t)
    _, _, cam, p, _, _ = install(t, "room", W, H)
    p.frame, p.sample_index = FRAME, 1
    f = Frame(t, W, H)
    t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp, moments_ptr=f.mom.ptr)
    m = f.get()[0]
    f.free()
    assert np.isfinite(m).all()
    return m, spp


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (257, 131), (1920, 1080)])
def test_frame_error_equals_the_reference(t, rendered_moments, W, H):
    src, n = rendered_moments
    flat = src.reshape(-1, 2)
    m = np.ascontiguousarray(flat[(np.arange(W * H) * 7 + 1000) % len(flat)].reshape(H, W, 2))   # downloaded moments, re-dealt to the size
    buf = t.malloc(m.nbytes)
    buf.upload(m)
    r = M.rse(m, n).astype(np.float64)
    for thr0 in (0.0, 0.05, 0.5):
        thr = off_every_pixel(r, thr0)
        ref_mean, ref_above = M.frame_error(m, n, thr)
        mean, above = t.frame_error(buf.ptr, W, H, n, thr)
        mean2, above2 = t.frame_error(buf.ptr, W, H, n, thr)
        print(f"{W}x{H} threshold {thr:.6g}: mean_rse {mean!r} (reference {ref_mean!r}), above {above} ({ref_above})")
        assert above == ref_above
        assert abs(mean - ref_mean) <= 1e-5 * ref_mean
        assert (mean, above) == (mean2, above2)   # bit for bit, run to run
    # either output alone
    lib, mean, above = g._abi.ptmi(), C.c_double(), C.c_uint64()
    assert lib.pt_frame_error(t._ctx, buf.ptr, W, H, n, 0.0, C.byref(mean), None) == 0
    assert lib.pt_frame_error(t._ctx, buf.ptr, W, H, n, 0.0, None, C.byref(above)) == 0
    assert (mean.value, above.value) == t.frame_error(buf.ptr, W, H, n, 0.0)
    buf.free()


def test_frame_error_errors():
    lib = g._abi.ptmi()
    fresh = g.PathTracer(0)   # no scene needed
    try:
        buf = fresh.malloc(8 * 8 * 8)
        buf.zero()
        mean, above = C.c_double(), C.c_uint64()
        ok = dict(m=buf.ptr, w=8, h=8, n=2, thr=0.0, mean=C.byref(mean), above=C.byref(above))

        def call(**kw):
            a = dict(ok, **kw)
            return lib.pt_frame_error(fresh._ctx, a["m"], a["w"], a["h"], a["n"], a["thr"], a["mean"], a["above"])

        assert call() == 0 and mean.value == 0.0 and above.value == 0
        assert lib.pt_frame_error(None, buf.ptr, 8, 8, 2, 0.0, C.byref(mean), C.byref(above)) == PT_ERR_INVALID
        for bad in (dict(m=None), dict(mean=None, above=None), dict(w=0), dict(h=0), dict(w=-3), dict(n=1), dict(n=0),
                    dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=-0.5)):
            assert call(**bad) == PT_ERR_INVALID, bad
        with pytest.raises(g.PtError):
            fresh.frame_error(buf.ptr, 8, 8, 1)
        assert call() == 0
        buf.free()
    finally:
        fresh.close()


def test_render_moments_errors_are_pt_renders(t):
    W, H = 16, 16
    lib = g._abi.ptmi()
    _, _, cam, p, _, _ = install(t, "room", W, H)
    f = Frame(t, W, H)
    for change, spp in ((dict(sample_index=0), 1), (dict(width=1), 1), (dict(tri_mat=9), 1), (dict(flags=g.FLAG_NEE), 1), ({}, 0),
                        (dict(part_count=3, part_rows=5), 1)):
        q = g.Params.from_buffer_copy(p)
        for k, v in change.items():
            setattr(q, k, v)
        a = lib.pt_render(t._ctx, f.acc.ptr, f.rgba.ptr, C.byref(cam), C.byref(q), spp)
        b = lib.pt_render_moments(t._ctx, f.acc.ptr, f.rgba.ptr, f.mom.ptr, C.byref(cam), C.byref(q), spp)
        assert a == b == PT_ERR_INVALID, change
    assert lib.pt_render_moments(t._ctx, None, f.rgba.ptr, f.mom.ptr, C.byref(cam), C.byref(p), 1) == PT_ERR_INVALID
    assert np.isnan(f.get()[0]).all()
    f.free()


# ---------------------------------------------------------------------------------------------------- 7: the figure means something
def progressive_errors(t, name, W, H):
    restore(t)
    _, _, cam, p, _, _ = install(t, name, W, H)
    f = Frame(t, W, H)
    out, done = [], 0
    for total in (4, 16, 64):
        p.frame, p.sample_index = done, done + 1
        t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, total - done, moments_ptr=f.mom.ptr)
        done = total
        out.append(t.frame_error(f.mom.ptr, W, H, done)[0])
    f.free()
    print(f"{name} {W}x{H}: mean_rse after 4 / 16 / 64 samples {out}")
    return out


def test_frame_error_falls_with_samples_on_cornell_box(t):
    """mean_rse after 64 samples below that after 16, below that after 4, on cornell_box 160x120 with its material table, the
    library's default camera and default parameters (nothing of pt_params changed: the box is open towards the camera and the
    default background is white, so a path that leaves the box carries light).  Strict order only, no ratio.

    The parameters are the defaults on purpose.  The figure is a statement about pixels that HAVE seen light: a pixel whose
    samples are all black has m1 = m2 = 0 and, by the floor of the definition, rse 0.  With the background set to black (the
    denoiser tests' cornell_box_scene: one small ceiling quad, no next-event estimation) only 4.6 % of the pixels have a lit
    sample after 4 samples, 15 % after 16, 43 % after 64, each newly lit pixel enters with rse ~ 1, and the frame's figure
    RISES, 0.04127 / 0.13298 / 0.30253 (numpy reference and device alike) — a property of the definition on a frame that is
    mostly unlit, written down in DESIGN.md §10 f7 with what it means for a stop rule; it is not what this test is about."""
    e4, e16, e64 = progressive_errors(t, "box-defaults", 160, 120)
    assert e64 < e16 < e4, (e4, e16, e64)


def test_frame_error_falls_with_samples_in_the_sphere_room(t):
    """The same strict order where the premise of the figure holds — in the sphere room every wall glows, so (nearly) every
    sample carries light and every pixel's estimate has a finite relative variance: the standard error of its mean falls with
    the number of samples.  Strict order only, no ratio."""
    e4, e16, e64 = progressive_errors(t, "room", 160, 120)
    assert e64 < e16 < e4, (e4, e16, e64)


# ---------------------------------------------------------------------------------------------------- 8: no trace
def test_moments_and_frame_error_leave_no_trace_in_render(t):
    W, H = 257, 131
    restore(t)
    bvh, sph, cam, p, _, _ = install(t, "room", W, H)
    p.flags = g.FLAG_WRITE_RGBA

    def frame(tr):
        acc, rg = tr.alloc_frame(W, H)
        tr.launch_kernel(acc.ptr, rg.ptr, cam, p, 3)
        tr.sync()
        out = acc.download(np.float32, (H, W, 3)), rg.download(np.uint32, (H, W))
        acc.free()
        rg.free()
        return out

    f = Frame(t, W, H)
    for spp in (1, 3, 16):
        t.launch_kernel(f.acc.ptr, f.rgba.ptr, cam, p, spp, moments_ptr=f.mom.ptr)
    t.frame_error(f.mom.ptr, W, H, 16, 0.1)
    f.free()
    a = frame(t)
    clean = g.PathTracer(0)
    try:
        clean.upload_bvh(bvh)
        clean.upload_spheres(sph)
        b = frame(clean)
    finally:
        clean.close()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- 9: pt_app
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
BASE = [APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "120", "--spp", "2"]


def run_app(args):
    r = subprocess.run(BASE + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout


def test_pt_app_variance_out(tmp_path):
    outs = {}
    for k, extra in (("plain", []), ("var", ["--variance-out", str(tmp_path / "var.pfm")]), ("plain2", ["--gpus", "2"]),
                     ("var2", ["--gpus", "2", "--variance-out", str(tmp_path / "var2.pfm")])):
        img = tmp_path / f"{k}.png"
        run_app(["--frames", "4", "--out", str(img)] + extra)
        outs[k] = img.read_bytes()
    assert outs["var"] == outs["plain"] and outs["var2"] == outs["plain2"]
    for name in ("var.pfm", "var2.pfm"):
        blob = (tmp_path / name).read_bytes()
        head = blob.split(b"\n", 3)
        assert head[0] == b"PF" and head[1].split() == [b"160", b"120"]
        data = np.frombuffer(head[3], np.float32)
        assert data.size == 160 * 120 * 3
        assert np.isfinite(data).all() and (data >= 0).all() and data.any()
        assert np.array_equal(data[0::3], data[1::3]) and np.array_equal(data[0::3], data[2::3])   # grey
    if outs["plain2"] == outs["plain"]:   # the gathered frame is the one-context frame: so are its moments
        assert (tmp_path / "var2.pfm").read_bytes() == (tmp_path / "var.pfm").read_bytes()


@pytest.mark.parametrize("gpus", [1, 2])
def test_pt_app_until_error(tmp_path, gpus):
    more = ["--gpus", str(gpus)]
    loose = run_app(["--frames", "4", "--until-error", "1e9", "--max-frames", "12", "--out", str(tmp_path / "loose.png")] + more)
    assert "until-error 1e+09: 4 frames rendered" in loose, loose
    run_app(["--frames", "4", "--out", str(tmp_path / "four.png")] + more)
    assert (tmp_path / "loose.png").read_bytes() == (tmp_path / "four.png").read_bytes()
    tight = run_app(["--frames", "4", "--until-error", "0", "--max-frames", "12", "--out", str(tmp_path / "tight.png")] + more)
    assert "until-error 0: 12 frames rendered" in tight, tight
    run_app(["--frames", "12", "--out", str(tmp_path / "twelve.png")] + more)
    assert (tmp_path / "tight.png").read_bytes() == (tmp_path / "twelve.png").read_bytes()
    r = subprocess.run(BASE + ["--frames", "4", "--until-error", "0.1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--max-frames" in r.stderr
