"""GPU tests of pt_temporal (temporal reprojection) against the CPU reference of tests/temporal_ref.py: random colour over real
guides of two cameras, bit copies where no history is taken, aliasing, a static camera, call ordering, the quality of a panning
sequence, errors, freedom from side effects and pt_app --temporal-out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import temporal_ref as T
from gpu_support import Guides, bits, golden_camera, setup_scene
from temporal_ref import (ACCEPTED_MIN, FRAGILE_MAX, MOVES, PARAM_SETS, QUALITY_FRAMES, QUALITY_K, QUALITY_PAN, QUALITY_SPP, params,
                          random_frames)

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


_guides = {}


def real_guides(t, W, H, move, scene="room"):
    """(prev_cam, (normal, position, id) of the golden camera, the same of the moved camera): pt_render_aux over `scene`,
    rendered at W x H directly."""
    kw = move if isinstance(move, dict) else MOVES[move]   # a name of MOVES or the keywords of T.moved
    key = (W, H, tuple(sorted(kw.items())), scene)
    if key not in _guides:
        setup_scene(t, scene, False)
        prev_cam, p = golden_camera(W, H), g.default_params(W, H)
        cams = [prev_cam, T.moved(prev_cam, **kw)]
        got = []
        gb = Guides(t, W, H)
        for cam in cams:
            gb.render(cam, p)
            got.append(gb.download()[1:4])
        gb.free()
        _guides[key] = (prev_cam, got[0], got[1])
    return _guides[key]


def temporal_gpu(t, W, H, prev_cam, prev, cur, out_alias=False, with_rgba=True, **kw):
    """pt_temporal over host arrays: prev = (color, length, normal, position, id or None) or None, cur = (color, normal,
    position, id or None).  Returns (out, length, rgba or None)."""
    bufs = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = t.malloc(max(a.nbytes, 4))
        b.upload(a)
        bufs.append(b)
        return b

    dprev = [up(a) for a in prev] if prev is not None else [None] * 5
    dcur = [up(a) for a in cur]
    do = dcur[0] if out_alias else t.malloc(W * H * 12)
    dl = t.malloc(W * H * 4)
    dr = t.malloc(W * H * 4) if with_rgba else None
    bufs += [b for b in (None if out_alias else do, dl, dr) if b is not None]
    ptr = lambda b: b.ptr if b is not None else None   # noqa: E731
    t.temporal(W, H, prev_cam, *[ptr(b) for b in dprev], *[ptr(b) for b in dcur], do.ptr, dl.ptr, ptr(dr), **params(**kw))
    t.sync()
    out, length = do.download(np.float32, (H, W, 3)), dl.download(np.float32, (H, W))
    rgba = dr.download(np.uint32, (H, W)) if dr else None
    for b in bufs:
        b.free()
    return out, length, rgba


# ---------------------------------------------------------------------------------------------------- against the reference
# The bounds are pt_denoise's tolerance class; the projection is restated in binary32 and only the tap sums differ (binary32
# against binary64), so differences near 1e-6 are expected.  Every case prints its figures.
@pytest.mark.parametrize("W,H", [(2, 2), (7, 5), (37, 23), (257, 131)])
@pytest.mark.parametrize("move", list(MOVES))
@pytest.mark.parametrize("ids", [True, False])
@pytest.mark.parametrize("pset", list(PARAM_SETS))
def test_equals_the_reference(t, W, H, move, ids, pset):
    prev_cam, gp, gc = real_guides(t, W, H, move)
    cur, prev, ln = random_frames(W, H, W + 31 * H)
    pi, ci = (gp[2], gc[2]) if ids else (None, None)
    out, length, rgba = temporal_gpu(t, W, H, prev_cam, (prev, ln, gp[0], gp[1], pi), (cur, gc[0], gc[1], ci), **PARAM_SETS[pset])
    ref, ref_len, fragile, acc = T.temporal(W, H, prev_cam, prev, ln, gp[0], gp[1], pi, cur, gc[0], gc[1], ci, **params(**PARAM_SETS[pset]))
    ok = ~fragile
    d_out, d_len = float(np.abs(out - ref)[ok].max(initial=0)), float(np.abs(length - ref_len)[ok].max(initial=0))
    print(f"temporal {W}x{H} {move} ids={ids} {pset}: |out-ref| {d_out:.3g} |len-ref| {d_len:.3g} fragile {fragile.mean():.4f} accepted {acc.mean():.3f}")
    assert d_out <= 1e-4, d_out
    assert d_len <= 1e-3, d_len
    assert np.array_equal(rgba, R.pack_rgba(out))
    assert fragile.mean() <= FRAGILE_MAX, float(fragile.mean())
    if pset == "history1":
        assert np.all(length == 1)
    if move == "static" and pset != "plane0" and W > 2:
        assert acc.mean() > 0.5   # (the history is really taken)


def test_no_history_and_rejected_history_are_bit_copies(t):
    W, H = 37, 23
    prev_cam, gp, gc = real_guides(t, W, H, "static")
    cur, prev, ln = random_frames(W, H, 5)
    out, length, rgba = temporal_gpu(t, W, H, None, None, (cur, gc[0], gc[1], gc[2]))
    assert np.array_equal(bits(out), bits(cur)) and np.all(length == 1) and np.array_equal(rgba, R.pack_rgba(cur))
    # the history of a camera that looked 120 degrees away: nothing of the current frame projects into it
    turned = T.moved(prev_cam, pan_deg=120.0)
    _, _, gt = real_guides(t, W, H, dict(pan_deg=120.0))   # what the turned camera saw
    for ids in (True, False):
        out, length, rgba = temporal_gpu(t, W, H, turned, (prev, ln, gt[0], gt[1], gt[2] if ids else None),
                                         (cur, gc[0], gc[1], gc[2] if ids else None))
        assert np.array_equal(bits(out), bits(cur)) and np.all(length == 1) and np.array_equal(rgba, R.pack_rgba(cur))


@pytest.mark.parametrize("history", [True, False])
def test_out_may_alias_cur(t, history):
    W, H = 37, 23
    prev_cam, gp, gc = real_guides(t, W, H, "pan")
    cur, prev, ln = random_frames(W, H, 6)
    pv = (prev, ln, gp[0], gp[1], gp[2]) if history else None
    cam = prev_cam if history else None
    a, la, ra = temporal_gpu(t, W, H, cam, pv, (cur, gc[0], gc[1], gc[2]))
    b, lb, rb = temporal_gpu(t, W, H, cam, pv, (cur, gc[0], gc[1], gc[2]), out_alias=True)
    c, lc, _ = temporal_gpu(t, W, H, cam, pv, (cur, gc[0], gc[1], gc[2]), with_rgba=False)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(la), bits(lb)) and np.array_equal(ra, rb)
    assert np.array_equal(bits(a), bits(c)) and np.array_equal(bits(la), bits(lc))
    if history:
        assert not np.array_equal(a, cur)   # it blended something


def test_static_camera_is_the_mean_of_the_frames(t):
    """K one-sample frames from one viewpoint through TemporalHistory with max_history >= K: the history is their mean.  The
    bound is twice what the numpy reference itself deviates from np.mean on the same frames (the bilinear weights are (1, 0, 0,
    0) only up to the rounding of fx, so a neighbour leaks in with a weight of ~W 2^-22).  The reference's own deviation over
    oracle renders of the same eight frames, which equal the GPU's bit for bit, is 1.4e-5: the bound is 2.9e-5."""
    W, H, K = 64, 64, 8
    bvh, sph, _, _ = setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    acc, rg = t.alloc_frame(W, H)
    th = g.TemporalHistory(t, W, H)
    frames = []
    for k in range(K):
        p.frame, p.sample_index = 100 + k, 1
        t.launch_kernel(acc.ptr, rg.ptr, cam, p, 1)
        color_ptr, length_ptr, gptrs = th.push(cam, p, acc.ptr, max_history=64.0)
        t.sync()
        frames.append(acc.download(np.float32, (H, W, 3)))
    k_last = 1 - th.cur
    hist = th.color[k_last].download(np.float32, (H, W, 3))
    length = th.length[k_last].download(np.float32, (H, W))
    nrm, pos, ids = (th.guides[k_last][1].download(np.float32, (H, W, 4)), th.guides[k_last][2].download(np.float32, (H, W, 4)),
                     th.guides[k_last][3].download(np.int32, (H, W)))
    assert color_ptr == th.color[k_last].ptr and length_ptr == th.length[k_last].ptr and gptrs[1] == th.guides[k_last][1].ptr
    th.free()
    acc.free()
    rg.free()
    # the reference over the same frames
    ref = ref_len = None
    fragile = np.zeros((H, W), bool)
    for k in range(K):
        if ref is None:
            ref, ref_len, f, _ = T.temporal(W, H, None, None, None, None, None, None, frames[k], nrm, pos, ids, **params(max_history=64.0))
        else:
            ref, ref_len, f, _ = T.temporal(W, H, cam, ref, ref_len, nrm, pos, ids, frames[k], nrm, pos, ids, **params(max_history=64.0))
        fragile |= f
    mean = np.mean(np.asarray(frames, np.float64), axis=0)
    hitm = np.any(nrm[..., :3] != 0, -1)
    ok = ~fragile & hitm
    dev_ref = float(np.abs(ref - mean)[ok].max())
    dev_gpu = float(np.abs(hist - mean)[ok].max())
    print(f"static camera, {K} frames {W}x{H}: reference deviates {dev_ref:.3g} from the mean, the GPU {dev_gpu:.3g}; fragile {fragile.mean():.4f}")
    assert fragile.mean() <= FRAGILE_MAX and ok.mean() > 0.9
    assert dev_ref <= 1e-3                       # the reference itself is the mean (else the bound below says nothing)
    assert dev_gpu <= 2.0 * dev_ref, (dev_gpu, dev_ref)
    assert np.abs(length - K)[ok].max() <= 1e-3
    assert np.all(length[~hitm] == 1)            # a miss keeps no history


def test_1080p_sampled_pixels(t):
    W, H = 1920, 1080
    prev_cam, gp, gc = real_guides(t, W, H, dict(pan_deg=1.0), scene="cornell_dragon")
    cur, prev, ln = random_frames(W, H, 12)
    rng = np.random.default_rng(11)
    ys, xs = rng.integers(0, H, 3004), rng.integers(0, W, 3004)
    ys[:4], xs[:4] = (0, H - 1, 0, H - 1), (0, 0, W - 1, W - 1)   # the corners
    out, length, rgba = temporal_gpu(t, W, H, prev_cam, (prev, ln, gp[0], gp[1], gp[2]), (cur, gc[0], gc[1], gc[2]))
    ref, ref_len, fragile, acc = T.temporal(W, H, prev_cam, prev, ln, gp[0], gp[1], gp[2], cur, gc[0], gc[1], gc[2], pixels=(ys, xs), **params())
    ok = ~fragile
    assert fragile.mean() <= FRAGILE_MAX and acc.mean() > 0.5
    assert np.abs(out[ys, xs] - ref)[ok].max() <= 1e-4
    assert np.abs(length[ys, xs] - ref_len)[ok].max() <= 1e-3
    assert np.array_equal(rgba, R.pack_rgba(out))
    del _guides[(W, H, (("pan_deg", 1.0),), "cornell_dragon")]   # (large)


# ---------------------------------------------------------------------------------------------------- with pt_render
def test_chain_needs_no_host_sync(t):
    """launch_kernel -> render_aux -> temporal -> denoise back to back, twice (the second frame has a history), equals the same
    calls with a host sync between every two."""
    W, H = 320, 240
    mesh, bvh, cam0, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    t.set_option(g.OPT_OVERLAP, 1)
    results = []
    try:
        for sync in (False, True):
            acc, rg = t.alloc_frame(W, H)
            out, orgba = t.malloc(W * H * 12), t.malloc(W * H * 4)
            th = g.TemporalHistory(t, W, H)
            t.sync()
            maybe = t.sync if sync else (lambda: None)
            for k in range(2):
                cam = T.moved(cam0, pan_deg=1.0 * k)
                for s in range(3):   # several calls in a row: the later ones run their path kernels on a side stream
                    q = g.Params.from_buffer_copy(p)
                    q.frame, q.sample_index, q.flags = 40 + 3 * k + s, 1 + s, g.FLAG_WRITE_RGBA
                    t.launch_kernel(acc.ptr, rg.ptr, cam, q, 1)
                    maybe()
                alb, nrm, pos, ids = th._ptrs(th.cur)
                hk = th.cur
                t.render_aux(cam, p, alb, nrm, pos, ids)
                maybe()
                if k == 0:
                    t.temporal(W, H, None, None, None, None, None, None, acc.ptr, nrm, pos, ids, th.color[hk].ptr, th.length[hk].ptr)
                else:
                    _, pn, pp, pi = th._ptrs(1 - hk)
                    t.temporal(W, H, T.moved(cam0), th.color[1 - hk].ptr, th.length[1 - hk].ptr, pn, pp, pi, acc.ptr, nrm, pos, ids,
                               th.color[hk].ptr, th.length[hk].ptr)
                th.cur = 1 - hk
                maybe()
                t.denoise(th.color[hk].ptr, alb, nrm, pos, W, H, out.ptr, orgba.ptr)
                maybe()
            t.sync()
            results.append((out.download(np.float32, (H, W, 3)), orgba.download(np.uint32, (H, W)),
                            th.color[hk].download(np.float32, (H, W, 3)), th.length[hk].download(np.float32, (H, W)),
                            acc.download(np.float32, (H, W, 3))))
            for b in (acc, rg, out, orgba):
                b.free()
            th.free()
    finally:
        t.upload_tri_materials(None, None)
        t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    a, b = results
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert (a[3] > 1).mean() > 0.5 and not np.array_equal(a[2], a[4]) and not np.array_equal(a[0], a[2])   # history taken, filtered


def test_quality_on_a_moving_camera(t):
    """cornell_box 320x240, 8 frames of 4 spp under a 1 degree pan per frame: the history is at least QUALITY_K times closer (MSE)
    to 1024 spp at the last camera than the last frame alone, QUALITY_K = 0.8 x the gain of the numpy reference over oracle
    renders at 80x60 (tests/test_temporal.py).  Prints the gain."""
    W, H = 320, 240
    mesh, bvh, cam0, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    cams = [T.moved(cam0, pan_deg=QUALITY_PAN * k) for k in range(QUALITY_FRAMES)]
    ref_acc, rg = t.alloc_frame(W, H)
    q = g.Params.from_buffer_copy(p)
    for k in range(0, 1024, 64):
        q.frame, q.sample_index = k, 1 + k
        t.launch_kernel(ref_acc.ptr, rg.ptr, cams[-1], q, 64)
    acc, _rg = t.alloc_frame(W, H)
    th = g.TemporalHistory(t, W, H)
    for k, cam in enumerate(cams):
        q.frame, q.sample_index = (1 << 20) + QUALITY_SPP * k, 1
        t.launch_kernel(acc.ptr, rg.ptr, cam, q, QUALITY_SPP)
        th.push(cam, q, acc.ptr)
    t.sync()
    hk = 1 - th.cur
    ref, last = ref_acc.download(np.float32, (H, W, 3)), acc.download(np.float32, (H, W, 3))
    hist, length = th.color[hk].download(np.float32, (H, W, 3)), th.length[hk].download(np.float32, (H, W))
    for b in (ref_acc, rg, acc, _rg):
        b.free()
    th.free()
    t.upload_tri_materials(None, None)
    gain, accepted = R.mse(last, ref) / R.mse(hist, ref), float((length > 1).mean())
    print(f"temporal quality 320x240, {QUALITY_FRAMES} x {QUALITY_SPP} spp, pan {QUALITY_PAN} deg: gain {gain:.2f}, accepted {accepted:.3f}")
    assert accepted >= ACCEPTED_MIN, accepted
    assert gain >= QUALITY_K, gain


# ---------------------------------------------------------------------------------------------------- errors, side effects
def test_temporal_errors():
    lib = g._abi.ptmi()
    W, H = 8, 8
    fresh = g.PathTracer(0)   # no scene needed
    try:
        bufs = [fresh.malloc(W * H * 16) for _ in range(11)]
        for b in bufs:
            b.zero()
        pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol = (b.ptr for b in bufs)
        cam = golden_camera(W, H)
        tp = g.TemporalParams(W, H, 32.0, 0.02, 0.9, 0)
        ok = [C.byref(tp), C.byref(cam), pc, pl, pn, pp, pi, cc, cn, cp, ci, oc, ol, None]

        def call(args):
            return lib.pt_temporal(fresh._ctx, *args)

        assert call(ok) == 0
        for k in (0, 7, 8, 9, 11, 12):          # params, cur colour / normal / position, out colour / length
            args = list(ok)
            args[k] = None
            assert call(args) == PT_ERR_INVALID, k
        for k in (1, 3, 4, 5):                  # with a history: its camera, lengths, normals, positions
            args = list(ok)
            args[k] = None
            assert call(args) == PT_ERR_INVALID, k
        for k in (6, 10):                       # exactly one of the two id pointers
            args = list(ok)
            args[k] = None
            assert call(args) == PT_ERR_INVALID, k
        args = list(ok)
        args[6] = args[10] = None               # neither: fine
        assert call(args) == 0
        args = list(ok)
        args[11] = pc                           # the new history over the old one
        assert call(args) == PT_ERR_INVALID
        args = list(ok)
        args[12] = pl
        assert call(args) == PT_ERR_INVALID
        args = list(ok)
        args[11] = cc                           # out over cur: allowed
        assert call(args) == 0
        # no history: prev_cam and every prev_* are ignored, a lone id pointer included
        assert call([C.byref(tp), None, None, None, None, None, None, cc, cn, cp, ci, oc, ol, None]) == 0
        assert call([C.byref(tp), None, None, pl, None, None, pi, cc, cn, cp, None, oc, ol, None]) == 0
        nan, inf = float("nan"), float("inf")
        for bad in ((1, H, 32, .02, .9), (W, 1, 32, .02, .9), (0, H, 32, .02, .9), (W, -4, 32, .02, .9), (W, H, 0.5, .02, .9), (W, H, nan, .02, .9),
                    (W, H, inf, .02, .9), (W, H, 32, -1e-3, .9), (W, H, 32, nan, .9), (W, H, 32, inf, .9), (W, H, 32, .02, 1.5),
                    (W, H, 32, .02, -1.5), (W, H, 32, .02, nan)):
            assert call([C.byref(g.TemporalParams(*bad, 0))] + ok[1:]) == PT_ERR_INVALID, bad
        assert b"pt_temporal" in lib.pt_last_error(fresh._ctx)
        for edge in ((2, 2, 1.0, 0.0, -1.0), (W, H, 32, .02, 1.0)):
            assert call([C.byref(g.TemporalParams(*edge, 0))] + ok[1:]) == 0, edge
        fresh.sync()
        for b in bufs:
            b.free()
        # the context still renders correctly
        W, H = 64, 64
        bvh, sph, _, _ = setup_scene(fresh, "room", False)
        cam, p = golden_camera(W, H), g.default_params(W, H)
        acc, rg = fresh.alloc_frame(W, H)
        fresh.launch_kernel(acc.ptr, rg.ptr, cam, p, 2)
        fresh.sync()
        ref, _, _ = orc.render(bvh, sph, cam, p, spp=2)
        assert np.array_equal(acc.download(np.float32, (H, W, 3)), ref)
        acc.free()
        rg.free()
    finally:
        fresh.close()


def test_temporal_leaves_no_trace_in_render(t):
    W, H = 257, 131
    bvh, sph, _, _ = setup_scene(t, "room", False)
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
    th = g.TemporalHistory(t, W, H)
    acc, rg = t.alloc_frame(W, H)
    for k in range(2):
        c2 = T.moved(cam, pan_deg=2.0 * k)
        t.launch_kernel(acc.ptr, rg.ptr, c2, p, 3)
        th.push(c2, p, acc.ptr, rg.ptr)
    t.sync()
    assert (th.length[1 - th.cur].download(np.float32, (H, W)) > 1).mean() > 0.5
    acc.free()
    rg.free()
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


def test_temporal_timing(t):
    W, H = 257, 131
    prev_cam, gp, gc = real_guides(t, W, H, "pan")
    t.set_option(g.OPT_TIMING, 1)
    try:
        cur, prev, ln = random_frames(W, H, 8)
        temporal_gpu(t, W, H, prev_cam, (prev, ln, gp[0], gp[1], gp[2]), (cur, gc[0], gc[1], gc[2]))
        assert 0 < t.last_kernel_ms() < 5.0
    finally:
        t.set_option(g.OPT_TIMING, 0)


def test_pt_app_temporal_out(tmp_path):
    """A camera that stands still: --out is byte-identical with and without --temporal-out, which is a PNG.  A panning camera:
    both files are written and differ.  The combinations --temporal-out does not support are refused."""
    app = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
    base = [app, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "120", "--frames", "8", "--spp", "2"]

    def run(name, extra):
        img = tmp_path / f"{name}.png"
        r = subprocess.run(base + ["--out", str(img)] + extra, capture_output=True, text=True, timeout=300)
        return r, img

    r, plain = run("plain", [])
    assert r.returncode == 0, r.stderr[-500:]
    r, still = run("still", ["--pan-deg", "0", "--dolly", "0", "--temporal-out", str(tmp_path / "t_still.png")])
    assert r.returncode == 0, r.stderr[-500:]
    assert still.read_bytes() == plain.read_bytes()
    ts = (tmp_path / "t_still.png").read_bytes()
    assert ts[:8] == b"\x89PNG\r\n\x1a\n"
    r, pan = run("pan", ["--pan-deg", "1", "--temporal-out", str(tmp_path / "t_pan.png"), "--denoise-out", str(tmp_path / "d_pan.pfm")])
    assert r.returncode == 0, r.stderr[-500:]
    tpan = (tmp_path / "t_pan.png").read_bytes()
    assert tpan[:8] == b"\x89PNG\r\n\x1a\n" and tpan != pan.read_bytes() and pan.read_bytes() != plain.read_bytes()
    assert (tmp_path / "d_pan.pfm").read_bytes()[:2] == b"PF"
    r, moving = run("moving", ["--pan-deg", "1", "--dolly", "0.1"])   # motion alone: the last frame
    assert r.returncode == 0 and moving.read_bytes() != plain.read_bytes()
    tout = ["--temporal-out", str(tmp_path / "x.png")]
    for extra in (["--gpus", "2"], ["--resume", str(tmp_path / "none.ckpt")], ["--checkpoint", str(tmp_path / "c.ckpt")],
                  ["--variance-out", str(tmp_path / "v.pfm")], ["--until-error", "0.1", "--max-frames", "16"]):
        r, _ = run("refused", tout + extra)
        assert r.returncode != 0 and "--temporal-out" in r.stderr, extra
    assert not (tmp_path / "x.png").exists()
