"""GPU tests of pt_denoise_variance (variance-guided a-trous filter) and pt_temporal_moments (the moments reprojected as the
colour is) against the CPU references of tests/denoise_var_ref.py: the filter over random colour and moments with real guides,
aliasing, errors, the scratch it shares with pt_denoise, call ordering after pt_render_moments, the quality of the defaults at
4, 64 and 1024 spp, the moments payload against the colour calls bit for bit, TemporalHistory with moments, timing and
pt_app --denoise-variance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import denoise_ref as R
import denoise_var_ref as V
import motion_ref as M
import temporal_ref as T
from denoise_var_ref import VAR_QUALITY_K
from gpu_support import Guides, bits, golden_camera, setup_scene, soup_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1

# out_variance against the float64 reference: |got - ref| <= VAR_RTOL * max(ref, VAR_FLOOR).  The weights enter squared and
# v_exp_f32 is an approximation, so the bound is MEASURED, not derived: the largest relative deviation on an MI355X over the 216
# cases of test_filter_equals_the_reference (it prints the figure of every case) was 1.31e-5 (37x23, 5 iterations, no position term,
# no lengths; the next two 9.4e-6 and 7.8e-6, the last one at a variance of 2.6e-15), and the bound is 8 x that.  VAR_FLOOR only
# keeps the ratio defined where the reference is exactly 0 (a zero-variance pixel all of whose taps are zero-variance pixels).
# The colour's largest deviation over the same cases was 1.0e-6, a hundredth of its 1e-4 bound.
VAR_RTOL = 8 * 1.31e-5
VAR_FLOOR = 1e-30


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


# ---------------------------------------------------------------------------------------------------- inputs
_guide_cache = {}


def real_guides(t, W, H):
    """Real guides (the sphere room + cornell, pt_render_aux; frames under 64 pixels a side cut from the middle of a 64-pixel one)
    with 5 % forced misses, and colour uniform in [0, 1]: test_gpu_denoise's inputs, restated."""
    if (W, H) not in _guide_cache:
        setup_scene(t, "room", False)
        WW, HH = max(W, 64), max(H, 64)
        gb = Guides(t, WW, HH)
        gb.render(golden_camera(WW, HH), g.default_params(WW, HH))
        alb, nrm, pos, _ = gb.download()
        gb.free()
        y0, x0 = (HH - H) // 2, (WW - W) // 2
        alb, nrm, pos = (np.ascontiguousarray(a[y0:y0 + H, x0:x0 + W]) for a in (alb, nrm, pos))
        miss = np.random.default_rng(W * 7919 + H).uniform(size=(H, W)) < 0.05
        for a in (alb, nrm, pos):
            a[miss] = 0
        _guide_cache[(W, H)] = (alb, nrm, pos)
    alb, nrm, pos = _guide_cache[(W, H)]
    col = np.random.default_rng(W + 31 * H).uniform(0, 1, (H, W, 3)).astype(np.float32)
    return col, alb, nrm, pos


def random_moments(W, H, lengths):
    """(moments, length or None, samples_per_frame): the seed variance is exactly 0 on a tenth of the pixels (misses next to hits
    among them) and uniform in [1e-3, 1e-1] elsewhere.  With lengths (1..6 frames of ONE sample, so the pixels of length 1 take
    the n < 2 branch, var = m2); without, 8 samples everywhere."""
    rng = np.random.default_rng(97 * W + H + (1 if lengths else 0))
    m1 = rng.uniform(0.1, 1.0, (H, W)).astype(np.float32)
    tv = np.where(rng.uniform(size=(H, W)) < 0.1, 0.0, rng.uniform(1e-3, 1e-1, (H, W)))
    ln = rng.integers(1, 7, (H, W)).astype(np.float32) if lengths else None
    spf = 1.0 if lengths else 8.0
    n = spf * (ln.astype(np.float64) if lengths else np.ones((H, W)))
    sq = (m1 * m1).astype(np.float32).astype(np.float64)          # m2 = fl(m1 * m1) exactly where the variance is 0
    m2 = np.where(n >= 2, sq + tv * (n - 1), tv).astype(np.float32)
    m2 = np.where((tv == 0) & (n >= 2), (m1 * m1).astype(np.float32), m2)
    return np.stack([m1, m2], -1), ln, spf


def dv_gpu(t, color, moments, length, albedo, normal, position, out_alias=False, with_rgba=True, with_var=True, **kw):
    """pt_denoise_variance over host arrays: (out, out_variance or None, rgba or None)."""
    H, W = color.shape[:2]
    host = (color, moments, length, albedo, normal, position)
    dev = [t.malloc(max(a.nbytes, 4)) if a is not None else None for a in host]
    for d, a in zip(dev, host):
        if d is not None:
            d.upload(np.ascontiguousarray(a))
    do = dev[0] if out_alias else t.malloc(W * H * 12)
    dvar = t.malloc(W * H * 4) if with_var else None
    dr = t.malloc(W * H * 4) if with_rgba else None
    ptr = lambda b: b.ptr if b is not None else None   # noqa: E731
    t.denoise_variance(*[ptr(d) for d in dev], W, H, do.ptr, ptr(dvar), ptr(dr), **kw)
    t.sync()
    out = do.download(np.float32, (H, W, 3))
    var = dvar.download(np.float32, (H, W)) if dvar else None
    rgba = dr.download(np.uint32, (H, W)) if dr else None
    for b in {id(x): x for x in dev + [do, dvar, dr] if x is not None}.values():
        b.free()
    return out, var, rgba


def var_deviation(got, ref, floor=VAR_FLOOR):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(ref.astype(np.float64), floor)).max())


# test_gpu_denoise.SIGMAS with sigma_color mapped to sigma_luminance: (sigma_luminance, sigma_normal, sigma_position)
SIGMAS = {"all": (1.0, 0.5, 0.05), "no_luminance": (0.0, 0.5, 0.05), "no_normal": (1.0, -1.0, 0.05), "no_position": (1.0, 0.5, 0.0),
          "none": (0.0, 0.0, 0.0), "tight": (0.2, 0.1, 0.01)}


# ---------------------------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (37, 23)])
@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("sig", list(SIGMAS))
@pytest.mark.parametrize("lengths", [True, False], ids=["lengths", "no_lengths"])
def test_filter_equals_the_reference(t, W, H, iterations, sig, lengths):
    col, alb, nrm, pos = real_guides(t, W, H)
    mom, ln, spf = random_moments(W, H, lengths)
    sl, sn, sx = SIGMAS[sig]
    kw = dict(iterations=iterations, sigma_luminance=sl, sigma_normal=sn, sigma_position=sx, samples_per_frame=spf)
    out, var, rgba = dv_gpu(t, col, mom, ln, alb, nrm, pos, **kw)
    ref, ref_var = V.atrous_variance(col, mom, ln, alb, nrm, pos, iterations, sl, sn, sx, samples_per_frame=spf)
    d_out, d_var = float(np.abs(out - ref).max()), var_deviation(var, ref_var)
    print(f"dv {W}x{H} it={iterations} {sig} lengths={lengths}: |out-ref| {d_out:.3g} variance rel {d_var:.3g}")
    assert d_out <= 1e-4, d_out
    assert np.array_equal(rgba, R.pack_rgba(out))
    assert d_var <= VAR_RTOL, d_var
    if iterations == 0:
        assert np.array_equal(bits(out), bits(col))
        assert np.array_equal(bits(var), bits(ref_var))     # the seed is binary32 on both sides
        assert (var == 0).mean() > 0.02 or W == 1


def test_filter_1080p_sampled_pixels(t):
    """The variance is judged relative to max(ref, 1e-12).  Measured on an MI355X: 2999 of the 3000 pixels deviate by at most
    6.3e-6 of their value (median 2.6e-7); one, a miss whose variance and whose neighbours' variance are exactly 0, holds 1.9e-27 and
    deviates by 1.45e-4 of that.  Its luminance stop sits at its floor, k_p = 1 / 1e-4, so what little it gathers comes through
    weights near 1e-12 whose exponent is 1e4 x a luminance difference — a last-place rounding of that difference in binary32 moves
    the weight by 1e-4 of itself.  The smallest variance these inputs seed is 1e-3 / 5 before demodulation; 1e-12 is far below anything
    a filter of it returns and far above what such a pixel holds."""
    W, H = 1920, 1080
    col, alb, nrm, pos = real_guides(t, W, H)
    mom, ln, spf = random_moments(W, H, True)
    rng = np.random.default_rng(11)
    ys, xs = rng.integers(0, H, 3000), rng.integers(0, W, 3000)
    ys[:4], xs[:4] = (0, H - 1, 0, H - 1), (0, 0, W - 1, W - 1)   # the corners
    it, sig = 2, SIGMAS["all"]     # (the reference runs every iteration but the last over the whole frame, in float64)
    out, var, rgba = dv_gpu(t, col, mom, ln, alb, nrm, pos, iterations=it, sigma_luminance=sig[0], sigma_normal=sig[1],
                            sigma_position=sig[2], samples_per_frame=spf)
    ref, ref_var = V.atrous_variance(col, mom, ln, alb, nrm, pos, it, *sig, samples_per_frame=spf, pixels=(ys, xs))
    assert np.abs(out[ys, xs] - ref).max() <= 1e-4
    d_var = var_deviation(var[ys, xs], ref_var, floor=1e-12)
    print(f"dv 1080p: |out-ref| {float(np.abs(out[ys, xs] - ref).max()):.3g} variance rel {d_var:.3g} (no floor: {var_deviation(var[ys, xs], ref_var):.3g})")
    assert d_var <= VAR_RTOL, d_var
    assert np.array_equal(rgba, R.pack_rgba(out))


@pytest.mark.parametrize("iterations", [0, 3])
def test_out_may_alias_color(t, iterations):
    col, alb, nrm, pos = real_guides(t, 37, 23)
    mom, ln, spf = random_moments(37, 23, True)
    a, va, ra = dv_gpu(t, col, mom, ln, alb, nrm, pos, iterations=iterations, samples_per_frame=spf)
    b, vb, rb = dv_gpu(t, col, mom, ln, alb, nrm, pos, out_alias=True, iterations=iterations, samples_per_frame=spf)
    c, vc, _ = dv_gpu(t, col, mom, ln, alb, nrm, pos, with_rgba=False, with_var=False, iterations=iterations, samples_per_frame=spf)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ra, rb) and np.array_equal(bits(va), bits(vb))
    assert np.array_equal(bits(a), bits(c)) and vc is None


def test_errors(t):
    """In the header's order: pt_denoise's, NULL moments, samples_per_frame, out_variance equal to an input."""
    lib = g._abi.ptmi()
    W, H = 8, 8
    bufs = [t.malloc(W * H * 16) for _ in range(9)]
    color, mom, ln, alb, nrm, pos, out, var, rgba = [b.ptr for b in bufs]

    def call(dp=(W, H, 2, 4.0, 0.5, 0.05, 1.0, 0), **over):
        a = dict(color=color, mom=mom, ln=ln, alb=alb, nrm=nrm, pos=pos, out=out, var=var, rgba=rgba)
        a.update(over)
        return lib.pt_denoise_variance(t._ctx, C.byref(g.DenoiseVarianceParams(*dp)) if dp is not None else None, a["color"], a["mom"], a["ln"],
                                       a["alb"], a["nrm"], a["pos"], a["out"], a["var"], a["rgba"])

    try:
        assert call() == 0 and call(ln=None, var=None, rgba=None) == 0
        assert call(dp=None) == PT_ERR_INVALID
        for k in ("color", "alb", "nrm", "pos", "out"):
            assert call(**{k: None}) == PT_ERR_INVALID, k
        nan, inf = float("nan"), float("inf")
        for dp in ((0, H, 2, 1, 1, 1, 1, 0), (W, 0, 2, 1, 1, 1, 1, 0), (W, H, -1, 1, 1, 1, 1, 0), (W, H, 11, 1, 1, 1, 1, 0),
                   (W, H, 2, nan, 1, 1, 1, 0), (W, H, 2, 1, inf, 1, 1, 0), (W, H, 2, 1, 1, -inf, 1, 0)):
            assert call(dp=dp) == PT_ERR_INVALID, dp
        assert call(mom=None) == PT_ERR_INVALID
        assert b"moments" in lib.pt_last_error(t._ctx)
        for spf in (0.5, 0.0, -1.0, nan, inf):
            assert call(dp=(W, H, 2, 4.0, 0.5, 0.05, spf, 0)) == PT_ERR_INVALID, spf
            assert b"samples_per_frame" in lib.pt_last_error(t._ctx)
        for k in ("color", "mom", "ln", "alb", "nrm", "pos"):
            assert call(var={"color": color, "mom": mom, "ln": ln, "alb": alb, "nrm": nrm, "pos": pos}[k]) == PT_ERR_INVALID, k
            assert b"out_variance_dev" in lib.pt_last_error(t._ctx)
        assert call() == 0     # the context still works
        t.sync()
    finally:
        for b in bufs:
            b.free()


def test_scratch_is_shared_with_pt_denoise(t):
    """pt_denoise 7x5, pt_denoise_variance 37x23 (grows the shared scratch), pt_denoise 7x5 on one context: each result equals a
    fresh context's, bit for bit."""
    small, large = real_guides(t, 7, 5), real_guides(t, 37, 23)
    mom, ln, spf = random_moments(37, 23, True)

    def dn(tr):
        col, alb, nrm, pos = small
        bufs = [tr.malloc(a.nbytes) for a in small] + [tr.malloc(7 * 5 * 12)]
        for b, a in zip(bufs, small):
            b.upload(np.ascontiguousarray(a))
        tr.denoise(*[b.ptr for b in bufs[:4]], 7, 5, bufs[4].ptr, iterations=3, sigma_color=1.0)
        tr.sync()
        out = bufs[4].download(np.float32, (5, 7, 3))
        for b in bufs:
            b.free()
        return out

    def dv(tr):
        return dv_gpu(tr, large[0], mom, ln, *large[1:], iterations=3, samples_per_frame=spf)

    got = [dn(t), dv(t), dn(t)]
    fresh = []
    for fn in (dn, dv, dn):
        tr = g.PathTracer(0)
        try:
            fresh.append(fn(tr))
        finally:
            tr.close()
    assert np.array_equal(bits(got[0]), bits(fresh[0])) and np.array_equal(bits(got[2]), bits(fresh[2]))
    assert np.array_equal(bits(got[1][0]), bits(fresh[1][0])) and np.array_equal(bits(got[1][1]), bits(fresh[1][1]))
    assert np.array_equal(got[1][2], fresh[1][2])


# ---------------------------------------------------------------------------------------------------- with pt_render_moments
def box_scene(t, W, H):
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    return cam, p


def test_straight_after_render_moments_needs_no_host_sync(t):
    W, H = 320, 240
    cam, p = box_scene(t, W, H)
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    t.set_option(g.OPT_OVERLAP, 1)
    results = []
    try:
        for sync in (False, True):
            gb = Guides(t, W, H)
            gb.render(cam, p)
            acc, rg = t.alloc_frame(W, H)
            mom, out, var, orgba = t.malloc(W * H * 8), t.malloc(W * H * 12), t.malloc(W * H * 4), t.malloc(W * H * 4)
            t.sync()
            for k in range(4):     # several calls in a row: the later ones run their path kernels on a side stream
                q = g.Params.from_buffer_copy(p)
                q.frame, q.sample_index, q.flags = 40 + k, 1 + k, g.FLAG_WRITE_RGBA
                t.launch_kernel(acc.ptr, rg.ptr, cam, q, 1, moments_ptr=mom.ptr)
            if sync:
                t.sync()
            t.denoise_variance(acc.ptr, mom.ptr, None, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr, var.ptr, orgba.ptr, samples_per_frame=4)
            t.sync()
            results.append((out.download(np.float32, (H, W, 3)), var.download(np.float32, (H, W)), orgba.download(np.uint32, (H, W)),
                            acc.download(np.float32, (H, W, 3)), mom.download(np.float32, (H, W, 2))))
            for b in (acc, rg, mom, out, var, orgba):
                b.free()
            gb.free()
    finally:
        t.upload_tri_materials(None, None)
        t.set_option(g.OPT_OVERLAP, 0)
        t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    a, b = results
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert not np.array_equal(a[0], a[3]) and a[1].any()   # it filtered something, and there is variance


def test_quality_of_the_defaults_on_the_gpu(t):
    """cornell_box 320x240 against 8192 spp (64-sample calls): gain >= VAR_QUALITY_K at 4, 64 and 1024 spp; at 1024 spp
    pt_denoise's defaults make the frame worse (gain < 1) and the variance-guided filter improves it (gain > 1).
    Measured on oracle frames with the float64 reference: 2.91 / 8.68 / 4.54, and 0.53 for the defaults."""
    W, H = 320, 240
    cam, p = box_scene(t, W, H)

    def render(spp, frame, mom):
        acc, rg = t.alloc_frame(W, H)
        q = g.Params.from_buffer_copy(p)
        for k in range(0, spp, 64):
            q.frame, q.sample_index = frame + k, 1 + k
            t.launch_kernel(acc.ptr, rg.ptr, cam, q, min(64, spp - k), moments_ptr=mom.ptr if mom else None)
        rg.free()
        return acc

    try:
        gb = Guides(t, W, H)
        gb.render(cam, p)
        dref = render(V.QUALITY_REF_SPP, 0, None)
        t.sync()
        ref = dref.download(np.float32, (H, W, 3))
        dref.free()
        out, mom = t.malloc(W * H * 12), t.malloc(W * H * 8)
        gains = {}
        for spp in V.QUALITY_SPP:
            acc = render(spp, V.QUALITY_NOISY_FRAME, mom)
            t.denoise_variance(acc.ptr, mom.ptr, None, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr, samples_per_frame=spp)
            t.sync()
            noisy, den = acc.download(np.float32, (H, W, 3)), out.download(np.float32, (H, W, 3))
            t.denoise(acc.ptr, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr)
            t.sync()
            plain = out.download(np.float32, (H, W, 3))
            acc.free()
            gains[spp] = (R.mse(noisy, ref) / R.mse(den, ref), R.mse(noisy, ref) / R.mse(plain, ref))
            print(f"quality 320x240 {spp} spp vs {V.QUALITY_REF_SPP}: variance-guided gain {gains[spp][0]:.2f}, pt_denoise defaults {gains[spp][1]:.2f}")
        for b in (out, mom):
            b.free()
        gb.free()
    finally:
        t.upload_tri_materials(None, None)
    for spp in V.QUALITY_SPP:
        assert gains[spp][0] >= VAR_QUALITY_K, (spp, gains[spp])
    assert gains[1024][1] < 1.0 < gains[1024][0], gains[1024]


# ---------------------------------------------------------------------------------------------------- pt_temporal_moments
_two = {}


def two_camera_guides(t, W, H, move):
    """(prev_cam, (normal, position, id) of the golden camera, the same of the moved camera) over the sphere room."""
    key = (W, H, tuple(sorted(move.items())))
    if key not in _two:
        setup_scene(t, "room", False)
        prev_cam, p = golden_camera(W, H), g.default_params(W, H)
        got = []
        gb = Guides(t, W, H)
        for cam in (prev_cam, T.moved(prev_cam, **move)):
            gb.render(cam, p)
            got.append(gb.download()[1:4])
        gb.free()
        _two[key] = (prev_cam, got[0], got[1])
    return _two[key]


def moments_frames(W, H, seed):
    rng = np.random.default_rng(seed)
    cur, prev = (rng.uniform(0, 1, (H, W, 2)).astype(np.float32) for _ in range(2))
    return cur, prev, rng.integers(1, 41, (H, W)).astype(np.float32)


def pad3(m):
    return np.ascontiguousarray(np.concatenate([m, np.zeros(m.shape[:2] + (1,), np.float32)], -1))


def tm_gpu(t, W, H, prev_cam, verts, prev, cur, colour, out_alias=False, **kw):
    """verts = (prev soup, cur soup, n) or None; prev = (payload, length, normal, position, id or None) or None; cur = (payload,
    normal, position, id or None).  colour False: pt_temporal_moments on the (m1, m2) payloads -> out [H][W][2].  colour True: the
    colour call of the same rule (pt_temporal / pt_temporal_motion) on the payloads padded to (m1, m2, 0) -> out [H][W][3]."""
    bufs = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = t.malloc(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
        return b

    ptr = lambda b: b.ptr if b is not None else None   # noqa: E731
    if colour:
        prev = None if prev is None else (pad3(prev[0]),) + tuple(prev[1:])
        cur = (pad3(cur[0]),) + tuple(cur[1:])
    dprev = [up(a) for a in prev] if prev is not None else [None] * 5
    dcur = [up(a) for a in cur]
    pv, cv, n = (up(np.asarray(verts[0], np.float32)), up(np.asarray(verts[1], np.float32)), verts[2]) if verts is not None else (None, None, 0)
    ch = 3 if colour else 2
    do = dcur[0] if out_alias else up(np.full((H, W, ch), 77.0, np.float32))     # every pixel must be written
    kw = T.params(**kw)
    if not colour:
        t.temporal_moments(W, H, prev_cam, ptr(pv), ptr(cv), n, *[ptr(b) for b in dprev], *[ptr(b) for b in dcur], do.ptr, **kw)
    else:
        dl = up(np.zeros((H, W), np.float32))
        if verts is not None:
            t.temporal_motion(W, H, prev_cam, ptr(pv), ptr(cv), n, *[ptr(b) for b in dprev], *[ptr(b) for b in dcur], do.ptr, dl.ptr, **kw)
        else:
            t.temporal(W, H, prev_cam, *[ptr(b) for b in dprev], *[ptr(b) for b in dcur], do.ptr, dl.ptr, **kw)
    t.sync()
    out = do.download(np.float32, (H, W, ch))
    for b in bufs:
        b.free()
    return out


@pytest.mark.parametrize("W,H", [(2, 2), (7, 5), (37, 23)])
@pytest.mark.parametrize("ids", [True, False])
@pytest.mark.parametrize("max_history", [1.0, 32.0])
def test_moments_under_a_camera_move(t, W, H, ids, max_history):
    prev_cam, gp, gc = two_camera_guides(t, W, H, dict(pan_deg=2.0))
    cur, prev, ln = moments_frames(W, H, W + 31 * H)
    pi, ci = (gp[2], gc[2]) if ids else (None, None)
    args = (prev_cam, None, (prev, ln, gp[0], gp[1], pi), (cur, gc[0], gc[1], ci))
    out = tm_gpu(t, W, H, *args, colour=False, max_history=max_history)
    col = tm_gpu(t, W, H, *args, colour=True, max_history=max_history)
    assert np.array_equal(bits(out), bits(col[..., :2])) and not col[..., 2].any()
    ref, fragile, acc = V.temporal_moments(W, H, prev_cam, None, None, 0, prev, ln, gp[0], gp[1], pi, cur, gc[0], gc[1], ci,
                                           **T.params(max_history=max_history))
    d = float(np.abs(out - ref)[~fragile].max(initial=0))
    print(f"temporal_moments {W}x{H} ids={ids} max_history={max_history}: |out-ref| {d:.3g} fragile {fragile.mean():.4f} accepted {acc.mean():.3f}")
    assert d <= 1e-4 and fragile.mean() <= T.FRAGILE_MAX
    if max_history > 1.0 and W > 2:
        assert acc.mean() > 0.5 and not np.array_equal(out, cur)
    alias = tm_gpu(t, W, H, *args, colour=False, out_alias=True, max_history=max_history)
    assert np.array_equal(bits(alias), bits(out))


def test_moments_under_moved_triangles(t):
    W, H = 37, 23
    rest, moved = M.case_soups("cube")
    prev_cam = M.case_camera("cube", rest, W, H)
    p = g.default_params(W, H)
    p.cull_backfaces = 0
    t.upload_tri_materials(None, None)
    t.upload_spheres([])
    t.build_bvh(soup_mesh(rest))
    gb = Guides(t, W, H)
    gb.render(prev_cam, p)
    gp = gb.download()[1:4]
    t.refit_bvh(moved)
    gb.render(T.moved(prev_cam, pan_deg=2.0), p)
    gc = gb.download()[1:4]
    gb.free()
    cur, prev, ln = moments_frames(W, H, 3)
    n = len(rest)
    args = (prev_cam, (rest, moved, n), (prev, ln, *gp), (cur, *gc))
    out = tm_gpu(t, W, H, *args, colour=False)
    col = tm_gpu(t, W, H, *args, colour=True)
    assert np.array_equal(bits(out), bits(col[..., :2]))
    ref, fragile, acc = V.temporal_moments(W, H, prev_cam, rest, moved, n, prev, ln, *gp, cur, *gc, **T.params())
    was_moved = M.where_it_was(rest, moved, n, *gc)[3]
    assert np.abs(out - ref)[~fragile].max(initial=0) <= 1e-4 and fragile.mean() <= T.FRAGILE_MAX
    assert was_moved.mean() > 0.1 and acc[was_moved].mean() > 0.5       # moved pixels kept their history
    # pt_temporal's rule on the same frames loses it where the triangles moved: the two rules are really two
    static = tm_gpu(t, W, H, prev_cam, None, (prev, ln, *gp), (cur, *gc), colour=False)
    assert not np.array_equal(static, out)


def test_moments_rejected_history_and_no_history_are_bit_copies(t):
    W, H = 37, 23
    prev_cam, gp, gc = two_camera_guides(t, W, H, {})
    cur, prev, ln = moments_frames(W, H, 5)
    out = tm_gpu(t, W, H, None, None, None, (cur, gc[0], gc[1], gc[2]), colour=False)
    assert np.array_equal(bits(out), bits(cur))
    turned = T.moved(prev_cam, pan_deg=120.0)     # a history that looked 120 degrees away: nothing projects into it
    _, _, gt = two_camera_guides(t, W, H, dict(pan_deg=120.0))
    for ids in (True, False):
        out = tm_gpu(t, W, H, turned, None, (prev, ln, gt[0], gt[1], gt[2] if ids else None), (cur, gc[0], gc[1], gc[2] if ids else None),
                     colour=False)
        assert np.array_equal(bits(out), bits(cur))


def test_temporal_moments_errors(t):
    lib = g._abi.ptmi()
    W, H = 8, 8
    bufs = [t.malloc(W * H * 16) for _ in range(11)]
    pm, pl, pn, pp, pi, cm, cn, cp, ci, om, vb = [b.ptr for b in bufs]
    cam = golden_camera(W, H)

    def call(tp=(W, H, 32.0, 0.02, 0.9, 0), cam=cam, pv=None, cv=None, n=0, **over):
        a = dict(pm=pm, pl=pl, pn=pn, pp=pp, pi=pi, cm=cm, cn=cn, cp=cp, ci=ci, om=om)
        a.update(over)
        return lib.pt_temporal_moments(t._ctx, C.byref(g.TemporalParams(*tp)) if tp else None, C.byref(cam) if cam is not None else None, pv, cv, n,
                                       a["pm"], a["pl"], a["pn"], a["pp"], a["pi"], a["cm"], a["cn"], a["cp"], a["ci"], a["om"])

    try:
        assert call() == 0 and call(pi=None, ci=None) == 0 and call(pv=vb, cv=vb, n=1) == 0 and call(om=cm) == 0
        assert call(tp=None) == PT_ERR_INVALID
        for k in ("cm", "cn", "cp", "om"):
            assert call(**{k: None}) == PT_ERR_INVALID, k
        for tp in ((1, H, 32.0, 0.02, 0.9, 0), (W, H, 0.5, 0.02, 0.9, 0), (W, H, 32.0, -1.0, 0.9, 0), (W, H, 32.0, 0.02, 1.5, 0)):
            assert call(tp=tp) == PT_ERR_INVALID, tp
        for k in ("pl", "pn", "pp"):
            assert call(**{k: None}) == PT_ERR_INVALID, k
        assert call(cam=None) == PT_ERR_INVALID
        assert call(pi=None) == PT_ERR_INVALID and call(ci=None) == PT_ERR_INVALID     # ids of both frames or of neither
        assert call(om=pm) == PT_ERR_INVALID                                            # ping-pong the moment histories
        # pt_temporal_motion's requirements once a vertex pointer is given
        assert call(pv=vb, cv=vb, n=1, pi=None, ci=None) == PT_ERR_INVALID
        assert call(pv=vb, cv=None, n=1) == PT_ERR_INVALID and call(pv=None, cv=vb, n=1) == PT_ERR_INVALID
        assert call(pv=vb, cv=vb, n=1 << 31) == PT_ERR_INVALID
        # no history: the prev_* pointers, the camera and the vertex pointers are ignored
        assert call(pm=None, pl=None, pn=None, pp=None, pi=None, cam=None) == 0
        t.sync()
    finally:
        for b in bufs:
            b.free()


def test_history_push_with_moments_equals_the_hand_issued_calls(t):
    """Three frames of a panning camera through TemporalHistory(with_moments=True) against the same calls issued by hand, bit for
    bit; self.moments and the returned lengths then go straight into denoise_variance."""
    W, H = 80, 60                                         # (the default camera's dist is H / 60, integer divide: H >= 60)
    cam0, p = box_scene(t, W, H)
    frames = 3
    try:
        acc, rg = t.alloc_frame(W, H)
        mom = t.malloc(W * H * 8)
        cams = [T.moved(cam0, pan_deg=1.0 * k) for k in range(frames)]

        def render(k):
            q = g.Params.from_buffer_copy(p)
            q.frame, q.sample_index = 100 + 4 * k, 1
            t.launch_kernel(acc.ptr, rg.ptr, cams[k], q, 4, moments_ptr=mom.ptr)

        hist = g.TemporalHistory(t, W, H, with_moments=True)
        assert hist.moments is None
        for k in range(frames):
            render(k)
            color_ptr, length_ptr, guides = hist.push(cams[k], p, acc.ptr, moments_ptr=mom.ptr)
        assert hist.moments is not None
        out, var = t.malloc(W * H * 12), t.malloc(W * H * 4)
        t.denoise_variance(color_ptr, hist.moments, length_ptr, *guides[:3], W, H, out.ptr, var.ptr, samples_per_frame=4)
        t.sync()
        n_pix = W * H
        h_color = hist.color[1 - hist.cur].download(np.float32, (H, W, 3))
        h_len = hist.length[1 - hist.cur].download(np.float32, (H, W))
        h_mom = hist.moment[1 - hist.cur].download(np.float32, (H, W, 2))
        h_out, h_var = out.download(np.float32, (H, W, 3)), var.download(np.float32, (H, W))
        with pytest.raises(ValueError):
            hist.push(cams[0], p, acc.ptr)                       # a history with moments needs the frame's moments
        hist.free()
        plain = g.TemporalHistory(t, W, H)
        with pytest.raises(ValueError):
            plain.push(cams[0], p, acc.ptr, moments_ptr=mom.ptr)
        plain.free()

        # by hand: guides, colour call, moments call with the SAME previous lengths, swap
        col = [t.malloc(n_pix * 12) for _ in range(2)]
        ln = [t.malloc(n_pix * 4) for _ in range(2)]
        mm = [t.malloc(n_pix * 8) for _ in range(2)]
        gbs = [Guides(t, W, H) for _ in range(2)]
        for k in range(frames):
            render(k)
            c, o = k & 1, 1 - (k & 1)
            gbs[c].render(cams[k], p)
            if k == 0:
                t.temporal(W, H, None, None, None, None, None, None, acc.ptr, gbs[c].nrm.ptr, gbs[c].pos.ptr, gbs[c].ids.ptr, col[c].ptr, ln[c].ptr)
                t.temporal_moments(W, H, None, None, None, 0, None, None, None, None, None, mom.ptr, gbs[c].nrm.ptr, gbs[c].pos.ptr, gbs[c].ids.ptr,
                                   mm[c].ptr)
            else:
                prev = (cams[k - 1], col[o].ptr, ln[o].ptr, gbs[o].nrm.ptr, gbs[o].pos.ptr, gbs[o].ids.ptr)
                t.temporal(W, H, *prev, acc.ptr, gbs[c].nrm.ptr, gbs[c].pos.ptr, gbs[c].ids.ptr, col[c].ptr, ln[c].ptr)
                t.temporal_moments(W, H, prev[0], None, None, 0, mm[o].ptr, *prev[2:], mom.ptr, gbs[c].nrm.ptr, gbs[c].pos.ptr, gbs[c].ids.ptr,
                                   mm[c].ptr)
        c = (frames - 1) & 1
        t.denoise_variance(col[c].ptr, mm[c].ptr, ln[c].ptr, gbs[c].alb.ptr, gbs[c].nrm.ptr, gbs[c].pos.ptr, W, H, out.ptr, var.ptr, samples_per_frame=4)
        t.sync()
        assert np.array_equal(bits(h_color), bits(col[c].download(np.float32, (H, W, 3))))
        assert np.array_equal(bits(h_len), bits(ln[c].download(np.float32, (H, W))))
        assert np.array_equal(bits(h_mom), bits(mm[c].download(np.float32, (H, W, 2))))
        assert np.array_equal(bits(h_out), bits(out.download(np.float32, (H, W, 3))))
        assert np.array_equal(bits(h_var), bits(var.download(np.float32, (H, W))))
        assert h_len.max() == frames and h_var.any() and not np.array_equal(h_out, h_color)
        for b in col + ln + mm + [acc, rg, mom, out, var]:
            b.free()
        for gb in gbs:
            gb.free()
    finally:
        t.upload_tri_materials(None, None)


# ---------------------------------------------------------------------------------------------------- timing, the app
def test_timing_1080p_five_iterations(t):
    """Under the 5 ms cap of test_gpu_denoise; the ratio to pt_denoise is measured by tools/temporal_bench.py --variance
    (profiles/r19_denoise_variance.txt), not asserted."""
    W, H = 1920, 1080
    setup_scene(t, "cornell_dragon", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    gb = Guides(t, W, H)
    acc, rg = t.alloc_frame(W, H)
    out, mom = t.malloc(W * H * 12), t.malloc(W * H * 8)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 2, moments_ptr=mom.ptr)
    gb.render(cam, p)
    t.set_option(g.OPT_TIMING, 1)
    try:
        ms = []
        for _ in range(5):
            t.denoise_variance(acc.ptr, mom.ptr, None, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr, None, rg.ptr, samples_per_frame=2,
                               iterations=5)
            ms.append(t.last_kernel_ms())
    finally:
        t.set_option(g.OPT_TIMING, 0)
    for b in (acc, rg, out, mom):
        b.free()
    gb.free()
    print(f"1080p: denoise_variance x5 {sorted(ms)}")
    assert 0 < min(ms) < 5.0


def test_pt_app_denoise_variance(tmp_path):
    """--denoise-variance: the --out image is byte-identical to a plain run (one context, and a tile split over two whose
    moments are gathered), the denoised image differs from --denoise-out's own; the flag is refused without --denoise-out, with
    --temporal-out and with --resume."""
    app = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
    base = [app, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "120", "--frames", "4", "--spp", "2"]
    outs = {}
    for k, extra in (("plain", []), ("dn", ["--denoise-out", str(tmp_path / "den.png")]),
                     ("dv", ["--denoise-out", str(tmp_path / "denv.png"), "--denoise-variance"]), ("plain2", ["--gpus", "2"]),
                     ("dv2", ["--gpus", "2", "--denoise-out", str(tmp_path / "denv2.png"), "--denoise-variance"])):
        img = tmp_path / f"{k}.png"
        r = subprocess.run(base + ["--out", str(img)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        outs[k] = img.read_bytes()
    assert outs["dn"] == outs["plain"] and outs["dv"] == outs["plain"]
    dn, dv = (tmp_path / "den.png").read_bytes(), (tmp_path / "denv.png").read_bytes()
    assert dv[:8] == b"\x89PNG\r\n\x1a\n" and dv != dn and dv != outs["plain"]
    assert outs["dv2"] == outs["plain2"]
    if outs["plain2"] == outs["plain"]:   # the gathered frame is the one-context frame: so are its moments and its denoised image
        assert (tmp_path / "denv2.png").read_bytes() == dv
    for extra in (["--denoise-variance"], ["--denoise-variance", "--denoise-out", str(tmp_path / "x.png"), "--temporal-out", str(tmp_path / "t.png")],
                  ["--denoise-variance", "--denoise-out", str(tmp_path / "x.png"), "--resume", str(tmp_path / "none.ckpt")]):
        r = subprocess.run(base + ["--out", str(tmp_path / "y.png")] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--denoise-variance" in r.stderr + r.stdout
