"""Adaptive sampling on the GPU (extension; contract in include/ptmi.h): pt_render_pixels, pt_select_pixels and the
host loop AdaptiveSampler.

The references are the existing calls — render_model (pt_render_camera), launch_kernel (pt_render / pt_render_moments), frame_error —
and tests/adaptive_ref.py, the numpy restatement of the fold and of the selection rule.  Every comparison of rendered values is
bitwise (gpu_support.bits); every buffer a test hands in is pre-filled with a canary and has one spare trailing element that must
stay untouched.  37 x 23 = 851 pixels are a multiple of neither 64 lanes nor 256-pixel blocks; 768 pixels are exactly three blocks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import gpu_pathtracer_amd as g
from gpu_support import bits, golden_camera, setup_scene
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu
W, H = 37, 23
NPIX = W * H
FRAME = 7
CANARY = -7.0
CANARY_U32 = 0xDEADBEEF
KINDS = ["pinhole", "thinlens", "ortho", "fisheye", "equirect"]
F = np.float32
INVALID, NO_SCENE = -1, -3


def model_kwargs(kind):
    return {"thinlens": dict(lens_radius=0.2, focus_dist=3.0), "ortho": dict(ortho_height=10.0), "fisheye": dict(fisheye_fov=2.5)}.get(kind, {})


def tilted(w, h):
    """An orthonormal basis that is no permutation of the axes, looking into the room."""
    return make_camera(w, h, pos=(0.5, -0.25, 1.0), front=(0.3, -0.2, -1.0), roll=0.4, fov=0.9)


def params(frame=FRAME, sample_index=1, flags=0):
    p = g.default_params(W, H, depth=4)
    p.frame, p.sample_index, p.flags = frame, sample_index, flags
    return p


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)   # what pt_render runs beside the calls; the calls themselves do not read the option
    setup_scene(tr, "room", False)
    yield tr
    tr.close()


class Frame:
    """Full-frame accumulator, moments and counts on the device, each with one spare element behind the image."""

    def __init__(self, t, accum=None, moments=None, counts=None, n_pix=NPIX):
        self.t, self.n = t, n_pix
        self.host = [np.full((n_pix + 1, 3), CANARY, F), np.full((n_pix + 1, 2), CANARY, F), np.full(n_pix + 1, CANARY_U32, np.uint32)]
        for h, init in zip(self.host, (accum, moments, counts)):
            if init is not None:
                h[:n_pix] = init
        self.dev = [t.malloc(h.nbytes) for h in self.host]
        for d, h in zip(self.dev, self.host):
            d.upload(h)
        self.accum, self.moments, self.counts = self.dev

    def get(self):
        """(accum, moments, counts) of the image; asserts the spare elements."""
        self.t.sync()
        out = [d.download(h.dtype, h.shape) for d, h in zip(self.dev, self.host)]
        assert np.all(out[0][self.n] == CANARY) and np.all(out[1][self.n] == CANARY) and out[2][self.n] == CANARY_U32, "an element behind a buffer was written"
        return out[0][:self.n], out[1][:self.n], out[2][:self.n]

    def free(self):
        for d in self.dev:
            d.free()


def full_frame(t, cam, cm, p, spp, hdr):
    """render_model over the whole image: float[NPIX][3]."""
    out = t.malloc(12 * NPIX)
    out.upload(np.full((NPIX, 3), CANARY, F))
    t.render_model(cam, cm, p, out.ptr, spp=spp, hdr=hdr)
    t.sync()
    got = out.download(F, (NPIX, 3))
    out.free()
    return got


def same(got, want, what):
    diff = bits(got).reshape(len(got), -1) != bits(want).reshape(len(want), -1)
    rows = np.flatnonzero(diff.any(axis=-1))
    assert len(rows) == 0, f"{what}: {len(rows)} of {len(got)} rows differ, first {rows[:5].tolist()}: {got[rows[0]]} vs {want[rows[0]]}"


# ---------------------------------------------------------------------------------------------------- 1: guarantee (a)
@pytest.mark.parametrize("kind", KINDS)
def test_whole_image_equals_render_camera(t, kind):
    """From zero counts and without a list, 3 samples and then 2 more are render_model(spp=5) bit for bit, clamped and HDR; all
    counts are 5; for the pinhole, clamped, it is launch_kernel(spp=5)'s accumulator and its moments."""
    cam = golden_camera(W, H) if kind == "pinhole" else tilted(W, H)
    cm = g.camera_model(kind, W, H, **model_kwargs(kind))
    for hdr in (False, True):
        fr = Frame(t, counts=0)
        t.render_pixels(cam, cm, params(FRAME), fr.accum.ptr, fr.counts.ptr, fr.moments.ptr, spp=3, hdr=hdr)
        t.render_pixels(cam, cm, params(FRAME + 3, sample_index=9), fr.accum.ptr, fr.counts.ptr, fr.moments.ptr, spp=2, hdr=hdr)   # (sample_index is not read)
        acc, mom, cnt = fr.get()
        fr.free()
        want = full_frame(t, cam, cm, params(FRAME), 5, hdr)
        assert len(np.unique(want, axis=0)) > 20, "the frame must look at something"
        same(acc, want, f"{kind} hdr {hdr}")
        assert np.all(cnt == 5)
        if kind == "pinhole" and not hdr:
            ref_acc, rgba = t.alloc_frame(W, H)
            ref_mom = t.malloc(NPIX * 8)
            t.launch_kernel(ref_acc.ptr, rgba.ptr, cam, params(FRAME), 5, moments_ptr=ref_mom.ptr)
            t.sync()
            same(acc, ref_acc.download(F, (NPIX, 3)), "pinhole against pt_render")
            same(mom, ref_mom.download(F, (NPIX, 2)), "pinhole moments against pt_render_moments")
            for b in (ref_acc, rgba, ref_mom):
                b.free()


# ---------------------------------------------------------------------------------------------------- 2: guarantee (b)
@pytest.mark.parametrize("hdr", [False, True], ids=["clamped", "hdr"])
def test_listed_pixels_get_their_own_count_and_the_rest_keeps_its_bits(t, hdr):
    """Random counts 0..5 and random buffer contents; a shuffled list of 211 distinct pixels and two indices past the image; 3
    samples.  The sample colours come from render_model (HDR, sample_index 1, one sample: the colour itself), folded by
    adaptive_ref; every element that is not a listed pixel's keeps the uploaded bits."""
    kind = "thinlens" if hdr else "pinhole"
    cam, cm = tilted(W, H), g.camera_model(kind, W, H, **model_kwargs(kind))
    rng = np.random.default_rng(23 + hdr)
    counts0 = rng.integers(0, 6, NPIX).astype(np.uint32)
    acc0, mom0 = rng.random((NPIX, 3), dtype=F), rng.random((NPIX, 2), dtype=F)
    fresh = np.flatnonzero(counts0 == 0)
    acc0[fresh[::2]] = np.nan      # N == 1 overwrites whatever was there
    mom0[fresh[::2]] = np.nan
    listed = rng.permutation(NPIX)[:211].astype(np.uint32)
    assert (counts0[listed] == 0).any() and (counts0[listed] == 5).any()
    rows = np.insert(listed, [17, 200], [NPIX, 0xFFFFFFF0]).astype(np.uint32)
    assert len(rows) == 213 and rows[17] == NPIX
    spp = 3
    col = np.stack([full_frame(t, cam, cm, params(FRAME + s), 1, True) for s in range(spp)], axis=1)   # [NPIX][spp][3]
    want_acc, want_mom, want_cnt = A.fold(col[listed], counts0[listed], acc0[listed], mom0[listed], hdr=hdr)

    lst = t.malloc(4 * (len(rows) + 1))
    lst.upload(np.append(rows, np.uint32(5)))
    for with_moments in (True, False):
        fr = Frame(t, acc0, mom0, counts0)
        t.render_pixels(cam, cm, params(FRAME), fr.accum.ptr, fr.counts.ptr, fr.moments.ptr if with_moments else None, spp=spp, hdr=hdr,
                        n=len(rows), pixels_ptr=lst.ptr)
        acc, mom, cnt = fr.get()
        fr.free()
        same(acc[listed], want_acc, "listed accumulators")
        assert np.array_equal(cnt[listed], want_cnt) and np.array_equal(cnt[listed], counts0[listed] + 3)
        rest = np.ones(NPIX, bool)
        rest[listed] = False
        same(acc[rest], acc0[rest], "unlisted accumulators")
        assert np.array_equal(cnt[rest], counts0[rest]), "unlisted counts"
        if with_moments:
            same(mom[listed], want_mom, "listed moments")
            same(mom[rest], mom0[rest], "unlisted moments")
        else:
            same(mom, mom0, "moments of a call without a moments buffer")
    lst.free()


# ---------------------------------------------------------------------------------------------------- 3: select, synthetic
def synthetic(n_pix, threshold, min_s, max_s, seed):
    """(moments, counts) with every count class, NaN / inf moments, m2 < m1^2 and an exact-zero error, the rest drawn so that the
    reference's rse lies a relative 1e-4 away from the threshold."""
    rng = np.random.default_rng(seed)
    classes = np.array([0, 1, max(min_s, 1) - 1, min_s, max(max_s, 1) - 1, max_s, 2, 3, 7], np.int64)
    cnt = np.where(rng.random(n_pix) < 0.5, rng.choice(classes, n_pix), rng.integers(0, max_s + 3, n_pix)).astype(np.uint32)
    m1 = (rng.random(n_pix, dtype=F) * F(0.9) + F(0.05)).astype(F)
    # the error about the threshold: var = (q * threshold * (m1 + 0.01))^2 * (n - 1) with q spread over 0 .. 3
    q = (rng.random(n_pix) * 3.0).astype(F)
    sd = q * F(max(threshold, 0.02)) * (m1 + F(0.01)) * np.sqrt(np.maximum(cnt.astype(F) - F(1), F(1)))
    mom = np.stack([m1, m1 * m1 + sd * sd], axis=-1).astype(F)
    special = rng.permutation(n_pix)[:40]
    mom[special[0:4], 0] = np.nan
    mom[special[4:8], 1] = np.nan
    mom[special[8:12], 0] = np.inf
    mom[special[12:16], 1] = np.inf
    mom[special[16:20], 0] = -np.inf
    mom[special[20:28], 1] = mom[special[20:28], 0] ** 2 * F(0.5)     # m2 < m1^2: var clamps to 0
    mom[special[28:34]] = (0.5, 0.25)                                 # exactly zero
    cnt[special[[0, 4, 8, 12, 20, 28]]] = [5, 2, 3, 6, 4, 2][:6]
    cnt[special[28:34]] = np.maximum(cnt[special[28:34]], 2)
    for _ in range(50):   # move the pixels whose figure is too close to the threshold
        r = A.rse(mom, cnt)
        near = (cnt >= 2) & np.isfinite(mom).all(axis=-1) & (r != 0) & (np.abs(r.astype(np.float64) - threshold) < 2e-4 * max(threshold, 1e-30))
        if not near.any():
            break
        mom[near, 1] *= F(1.5)
    return mom, cnt


def decided_clear_of_rounding(mom, cnt, threshold):
    """Every pixel's figure is either decided without rounding (fewer than two samples; not finite; var exactly 0) or lies a
    relative 1e-4 away from the threshold: a last-bit difference in sqrtf or the division cannot decide a case."""
    r = A.rse(mom, cnt).astype(np.float64)
    m = mom.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        var = np.fmax(F(0), m[:, 1] - m[:, 0] * m[:, 0])
        raw = np.sqrt(var / np.maximum(cnt.astype(F) - F(1), F(1))) / (m[:, 0] + F(0.01))
    exact = (cnt < 2) | ~np.isfinite(raw) | (var == 0)
    return bool(np.all(exact | (np.abs(r - threshold) >= 1e-4 * np.maximum(r, threshold))))


def run_select(t, mom, cnt, w, h, threshold, min_s, max_s):
    """(n, mean_rse, the whole list buffer of w * h entries) of one pt_select_pixels call over uploaded moments and counts."""
    n_pix = w * h
    fr = Frame(t, None, mom, cnt, n_pix=n_pix)
    lst = t.malloc(4 * (n_pix + 1))
    lst.upload(np.full(n_pix + 1, CANARY_U32, np.uint32))
    n, mean = t.select_pixels(fr.moments.ptr, fr.counts.ptr, lst.ptr, w, h, threshold, min_s, max_s)
    out = lst.download(np.uint32, (n_pix + 1,))
    _, mom_after, cnt_after = fr.get()
    fr.free()
    lst.free()
    assert out[n_pix] == CANARY_U32, "the element behind the list was written"
    assert np.array_equal(bits(mom_after), bits(np.asarray(mom, F))) and np.array_equal(cnt_after, cnt), "the inputs were written"
    return n, mean, out[:n_pix]


@pytest.mark.parametrize("shape", [(W, H), (32, 24)], ids=["851", "768-three-blocks"])
def test_select_on_synthetic_moments(t, shape):
    w, h = shape
    n_pix = w * h
    cases = [("mixed", 0.05, 4, 16), ("strict-at-zero", 0.0, 0, 0xFFFFFFFF), ("min-equals-max", 0.05, 8, 8), ("two-is-the-floor", 0.2, 0, 40)]
    for k, (what, threshold, min_s, max_s) in enumerate(cases):
        mom, cnt = synthetic(n_pix, threshold, min_s, min(max_s, 40), seed=100 + k)
        assert decided_clear_of_rounding(mom, cnt, threshold), what
        ref, r = A.select(mom, cnt, threshold, min_s, max_s)
        for c in {0, 1, max(min_s, 1) - 1, min_s, min(max_s, 40) - 1, min(max_s, 40)}:
            assert (cnt == c).any(), (what, c)
        assert ref.any() and not ref.all() and (~np.isfinite(mom)).any() and (mom[:, 1] < mom[:, 0] ** 2).any()
        zero = np.flatnonzero((mom[:, 0] == F(0.5)) & (mom[:, 1] == F(0.25)))
        assert len(zero) >= 6 and np.all(r[zero] == 0)
        if threshold == 0.0:
            assert not ref[zero].any(), "rse exactly 0 is not above a threshold of 0"
        n, mean, lst = run_select(t, mom, cnt, w, h, threshold, min_s, max_s)
        want = np.flatnonzero(ref).astype(np.uint32)
        print(f"{what} {n_pix}: selected {n} (reference {len(want)}), mean rse {mean!r} (reference {A.mean_rse(r)!r})")
        assert n == len(want), what
        assert np.array_equal(lst[:n], want), f"{what}: the list differs from the reference's"
        assert np.all(np.diff(lst[:n].astype(np.int64)) > 0), "ascending"
        assert np.all(lst[n:] == CANARY_U32), "written beyond the last entry"
        # sqrtf and the division are correctly rounded or within an ulp each (the figure is a sum of such values, all >= 0)
        assert abs(mean - A.mean_rse(r)) <= 4 * 2.0 ** -23 * A.mean_rse(r), what
    # all selected: nobody has reached min_samples; none: max_samples 0 — n == 0 and the list untouched
    mom, cnt = synthetic(n_pix, 0.05, 4, 16, seed=7)
    n, _, lst = run_select(t, mom, cnt, w, h, 0.05, 100, 100)
    assert n == n_pix and np.array_equal(lst, np.arange(n_pix, dtype=np.uint32))
    n, _, lst = run_select(t, mom, cnt, w, h, 0.05, 0, 0)
    assert n == 0 and np.all(lst == CANARY_U32)
    n, _, lst = run_select(t, mom, np.full(n_pix, 16, np.uint32), w, h, 1e30, 4, 99)
    assert n == 0 and np.all(lst == CANARY_U32), "nothing above a huge threshold"


# ---------------------------------------------------------------------------------------------------- 4: against pt_frame_error
def test_select_agrees_with_frame_error(t):
    """The moments of a real 8-sample frame with uniform counts: the mean is pt_frame_error's exactly and, with min_samples 0 and
    max_samples UINT32_MAX, the number selected its n_above."""
    cam = golden_camera(W, H)
    acc, rgba = t.alloc_frame(W, H)
    mom, cnt, lst = t.malloc(NPIX * 8), t.malloc(NPIX * 4), t.malloc(NPIX * 4)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, params(FRAME), 8, moments_ptr=mom.ptr)
    cnt.upload(np.full(NPIX, 8, np.uint32))
    for threshold in (0.0, 0.05, 0.3):
        mean, above = t.frame_error(mom.ptr, W, H, 8, threshold)
        n, mean_sel = t.select_pixels(mom.ptr, cnt.ptr, lst.ptr, W, H, threshold)
        print(f"threshold {threshold}: frame_error ({mean!r}, {above}), select_pixels ({mean_sel!r}, {n})")
        assert mean > 0 and mean_sel == mean, threshold
        assert n == above, threshold
        got = lst.download(np.uint32, (NPIX,))[:n]
        assert np.all(np.diff(got.astype(np.int64)) > 0) and (n == 0 or got[-1] < NPIX)
    assert 0 < t.frame_error(mom.ptr, W, H, 8, 0.05)[1] < NPIX, "the thresholds must decide something"
    for b in (acc, rgba, mom, cnt, lst):
        b.free()


# ---------------------------------------------------------------------------------------------------- 5: guarantee (d), the loop
def test_adaptive_sampler_end_to_end(t):
    cam, cm = golden_camera(W, H), g.camera_model("pinhole", W, H)
    # the threshold: the median of the positive per-pixel errors of the uniform 32-sample frame — pixels well above it run to the
    # maximum, pixels that see the background (error 0) stop at the minimum
    acc, rgba = t.alloc_frame(W, H)
    mom = t.malloc(NPIX * 8)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, params(FRAME), 32, moments_ptr=mom.ptr)
    t.sync()
    r32 = A.rse(mom.download(F, (NPIX, 2)), np.full(NPIX, 32, np.uint32))
    threshold = float(np.median(r32[r32 > 0]))
    ad = g.AdaptiveSampler(t, cm, threshold, 4, 32, 4)
    total, mean = ad.run(cam, params(FRAME))
    t.sync()
    cnt = ad.counts.download(np.uint32, (NPIX,))
    got_acc, got_mom = ad.accum.download(F, (NPIX, 3)), ad.moments.download(F, (NPIX, 2))
    print(f"threshold {threshold!r}: {len(ad.passes)} passes {[m for m, _ in ad.passes]}, {total} samples, mean rse {mean!r}, counts {np.bincount(cnt)[::4].tolist()}")
    assert len(ad.passes) <= 8 and total == int(cnt.sum()) and ad.passes[0][0] == NPIX
    assert np.all(np.diff([m for m, _ in ad.passes]) <= 0), "selection is monotone: a pixel that stopped stays stopped"
    assert cnt.min() >= 4 and cnt.max() <= 32 and np.all(cnt % 4 == 0)
    assert (cnt < 32).any() and (cnt == 32).any(), "both early-stopped pixels and pixels at the maximum must occur"
    ref_sel, r = A.select(got_mom, cnt, threshold, 4, 32)
    assert not ref_sel.any() and np.all(r[cnt < 32] <= F(threshold)), "a pixel below the maximum has an error at most the threshold"
    for c in np.unique(cnt):
        t.launch_kernel(acc.ptr, rgba.ptr, cam, params(FRAME), int(c), moments_ptr=mom.ptr)
        t.sync()
        rows = np.flatnonzero(cnt == c)
        same(got_acc[rows], acc.download(F, (NPIX, 3))[rows], f"accumulators of the pixels with {c} samples")
        same(got_mom[rows], mom.download(F, (NPIX, 2))[rows], f"moments of the pixels with {c} samples")
    ad.free()
    for b in (acc, rgba, mom):
        b.free()


# ---------------------------------------------------------------------------------------------------- 6: errors write nothing
def test_refusals_on_a_context(t):
    lib, ctx = g._abi.ptmi(), t._ctx
    cam, cm, p = golden_camera(W, H), g.camera_model("pinhole", W, H), params()
    fr = Frame(t, counts=0)
    lst = t.malloc(4 * NPIX)
    lst.upload(np.arange(NPIX, dtype=np.uint32))

    def call(cam_=cam, cm_=cm, pixels=None, n=NPIX, accum=fr.accum.ptr, counts=fr.counts.ptr, p_=p, spp=1, mode=g._abi.RAYS_CLAMPED):
        rc = lib.pt_render_pixels(ctx, C.byref(cam_) if cam_ else None, C.byref(cm_) if cm_ else None, pixels, n, accum, fr.moments.ptr, counts,
                                  C.byref(p_) if p_ else None, spp, mode)
        return rc, lib.pt_last_error(ctx).decode()

    assert call(n=0)[0] == 0 and call(spp=0, cam_=None)[0] == 0                       # nothing to do comes before the NULLs
    for kw in (dict(cam_=None), dict(cm_=None), dict(accum=None), dict(counts=None), dict(p_=None)):
        rc, msg = call(**kw)
        assert rc == INVALID and msg == "pt_render_pixels: null argument", kw
    assert call(mode=7) == (INVALID, "pt_render_pixels: mode must be PT_RAYS_CLAMPED or PT_RAYS_HDR")
    for n in (NPIX - 1, NPIX + 1, 1):
        assert call(n=n) == (INVALID, "pt_render_pixels: without a pixel list n must equal width * height")
    assert call(pixels=lst.ptr, n=5)[0] == 0 and call(pixels=lst.ptr, n=NPIX + 1 - 1)[0] == 0   # a list of any length
    bad = params(sample_index=0)
    assert call(p_=bad) == (INVALID, "pt_render_pixels: sample_index starts at 1")
    _, _, cnt = fr.get()
    assert np.array_equal(np.flatnonzero(cnt), np.arange(NPIX)) and np.all(cnt[:5] == 2) and np.all(cnt[5:] == 1), "only the two calls that ran counted"

    sp = g.SelectParams(W, H, 0.1, 4, 32, 0)
    n_sel = C.c_uint64(77)

    def select(sp_=sp, mom=fr.moments.ptr, counts=fr.counts.ptr, pixels=lst.ptr, n=n_sel):
        rc = lib.pt_select_pixels(ctx, C.byref(sp_) if sp_ else None, mom, counts, pixels, C.byref(n) if n else None, None)
        return rc, lib.pt_last_error(ctx).decode()

    for kw in (dict(sp_=None), dict(mom=None), dict(counts=None), dict(pixels=None), dict(n=None)):
        assert select(**kw) == (INVALID, "pt_select_pixels: null argument"), kw
    assert select(sp_=g.SelectParams(0, H, float("nan"), 9, 1, 0))[1].startswith("pt_select_pixels: width and height")
    assert select(sp_=g.SelectParams(W, H, float("nan"), 9, 1, 0))[1] == "pt_select_pixels: threshold must be finite and >= 0"
    assert select(sp_=g.SelectParams(W, H, -0.0 - 1e-9, 9, 1, 0))[0] == INVALID
    assert select(sp_=g.SelectParams(W, H, 0.0, 9, 1, 0)) == (INVALID, "pt_select_pixels: min_samples must not exceed max_samples")
    assert n_sel.value == 77 and np.array_equal(lst.download(np.uint32, (NPIX,)), np.arange(NPIX, dtype=np.uint32)), "a refused call writes nothing"
    assert select()[0] == 0 and n_sel.value == NPIX                                       # every pixel is below min_samples
    fr.free()
    lst.free()
    empty = g.PathTracer(0)
    try:
        rc = lib.pt_render_pixels(empty._ctx, None, None, None, 0, None, None, None, None, 0, 7)
        assert rc == NO_SCENE and lib.pt_last_error(empty._ctx).decode() == "pt_render_pixels: no scene uploaded"
    finally:
        empty.close()


# ---------------------------------------------------------------------------------------------------- 7: pt_app --adaptive
def test_pt_app_adaptive_holds_each_pixels_plain_run(tmp_path):
    """pt_app --adaptive: a pixel that ends with c samples holds what a plain run of c samples gives it (--camera pinhole, one call),
    for every count that occurs; the counts come from --samples-out.  Also with a fisheye model, and the usage refusals."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    app = os.path.join(root, "g.p.u-pathtracer_amd", "host", "pt_app")
    # 96 x 64: pt_app's camera stands H / 60 (an integer division) in front of its image plane
    base = [app, "--mesh", os.path.join(root, "assets", "cornell.ptmesh"), "--width", "96", "--height", "64"]

    def run(args, code=0):
        r = subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == code, r.stderr[-500:]
        return r

    for model in ([], ["--camera", "fisheye"]):
        out, cnt_path = tmp_path / "a.pfm", tmp_path / "c.pfm"
        for threshold in (0.05, 0.02, 0.1, 0.01, 0.2, 0.005):   # the first at which some pixels stop early and others go on
            r = run(model + ["--adaptive", threshold, "--min-spp", 4, "--max-spp", 12, "--samples-out", cnt_path, "--out", out])
            assert f"adaptive {threshold:g}: " in r.stdout and "mean_rse" in r.stdout, r.stdout
            img, cnt = g.read_pfm(str(out)), g.read_pfm(str(cnt_path))[..., 0]
            values = np.unique(cnt)
            print(f"{model} threshold {threshold}: counts {[(int(v), int((cnt == v).sum())) for v in values]}")
            assert set(values.tolist()) <= {4.0, 8.0, 12.0}
            if len(values) >= 2:
                break
        assert len(values) >= 2, "no threshold of the ladder gives pixels with different counts"
        for c in values:
            plain = tmp_path / f"p{int(c)}.pfm"
            run((model or ["--camera", "pinhole"]) + ["--frames", int(c), "--spp", int(c), "--out", plain])
            ref = g.read_pfm(str(plain))
            rows = cnt == c
            assert np.array_equal(bits(img[rows]), bits(ref[rows])), f"{model}: the pixels with {int(c)} samples"
    assert "multiples of --pass-spp" in run(["--adaptive", 0.1, "--min-spp", 6, "--max-spp", 12], 1).stderr
    assert "go with --adaptive" in run(["--min-spp", 4], 1).stderr
    assert "does not combine" in run(["--adaptive", 0.1, "--min-spp", 4, "--max-spp", 8, "--until-error", 0.1, "--max-frames", 32], 1).stderr
