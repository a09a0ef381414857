"""GPU tests of pt_render_aux (first-hit guide buffers) and pt_denoise (edge-avoiding a-trous filter) against the CPU reference
of tests/denoise_ref.py: guides over the test scenes and after a refit, the filter over random colour with real guides, call
ordering, the quality of the defaults, errors, freedom from side effects, timing and pt_app --denoise-out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
from denoise_ref import QUALITY_K
from gpu_support import Guides, compare_guides, cornell_dragon_moved, golden_camera, setup_scene, soup_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID, PT_ERR_NO_SCENE, PT_ERR_UNSUPPORTED = -1, -3, -5


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


# ---------------------------------------------------------------------------------------------------- guide buffers
@pytest.mark.parametrize("W,H", [(64, 64), (257, 131)])
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("scene,materials", [("room", False), ("cornell_box", True), ("cornell_box", False)])
def test_guides_equal_the_reference(t, scene, materials, cull, W, H):
    bvh, sph, mats, tm = setup_scene(t, scene, materials)
    cam = golden_camera(W, H) if scene == "room" else g.default_camera(W, H)
    p = g.default_params(W, H)
    p.cull_backfaces = cull
    p.part_count, p.part_index, p.flags = 3, 1, g.FLAG_NEE   # ignored: always the full frame
    gb = Guides(t, W, H)
    gb.render(cam, p)
    got = gb.download()
    gb.free()
    ref = R.guides(bvh, sph, cam, p, mats, tm)
    compare_guides(got, ref, f"{scene} mat={materials} cull={cull} {W}x{H}")
    assert (got[3] >= 0).mean() > 0.05
    if scene == "room":
        assert (got[3] <= -2).any()   # spheres too


def test_guides_1080p_bench_scene(t):
    W, H = 1920, 1080
    bvh, sph, _, _ = setup_scene(t, "cornell_dragon", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    gb = Guides(t, W, H)
    gb.render(cam, p)
    got = gb.download()
    gb.free()
    compare_guides(got, R.guides(bvh, sph, cam, p), "cornell_dragon 1080p")
    assert (got[3] >= 100).mean() > 0.01   # the dragon is in the frame


def test_guides_without_ids_and_timing(t):
    W, H = 96, 64
    setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    gb = Guides(t, W, H)
    gb.render(cam, p)
    a = gb.download()
    t.set_option(g.OPT_TIMING, 1)
    try:
        gb.ids.zero()
        gb.render(cam, p, with_ids=False)
        b = gb.download()
        assert t.last_kernel_ms() > 0
    finally:
        t.set_option(g.OPT_TIMING, 0)
    gb.free()
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert not b[3].any()   # id_dev = NULL: nothing written


def test_guides_after_a_refit_without_host_sync(t):
    W, H = 320, 180
    mesh, soup, moved = cornell_dragon_moved()
    t.upload_tri_materials(None, None)
    t.upload_spheres(g.reference_spheres())
    t.build_bvh(mesh)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    dv = t.malloc(moved.nbytes)
    dv.upload(moved)                       # staged before: the refit and the guides below run back to back
    gb = Guides(t, W, H)
    t.refit_bvh(dv)
    gb.render(cam, p)
    got = gb.download()
    gb.free()
    dv.free()
    mm = soup_mesh(moved)
    ref = list(R.guides(g.Bvh(mm), g.reference_spheres(), cam, p))
    # a host tree over the moved triangles may differ from the refit one on rays that graze a box: brute force decides
    diff = np.argwhere(got[3] != ref[3])
    assert len(diff) <= 8, len(diff)
    if len(diff):
        rays = orc.primary_rays(cam, W, H, jitter=False).reshape(H, W, 8)[diff[:, 0], diff[:, 1]]
        _, ib, _ = orc.trace_brute(mm, rays, True)
        gi = got[3][diff[:, 0], diff[:, 1]]
        assert np.array_equal(gi[gi >= 0], ib[gi >= 0])
        for k in range(4):   # those pixels are settled: out of the comparison below
            ref[k] = ref[k].copy()
            ref[k][diff[:, 0], diff[:, 1]] = got[k][diff[:, 0], diff[:, 1]]
    compare_guides(got, ref, "after refit")
    moved_ids = np.unique(got[3][got[3] >= g.Mesh.asset("cornell").n_tris])
    assert len(moved_ids) > 100


def test_aux_errors(t):
    W, H = 16, 16
    cam, p = g.default_camera(W, H), g.default_params(W, H)
    lib = g._abi.ptmi()
    fresh = g.PathTracer(0)
    try:
        gb = Guides(fresh, W, H)
        assert lib.pt_render_aux(fresh._ctx, C.byref(cam), C.byref(p), gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, None) == PT_ERR_NO_SCENE
        fresh.set_option(g.OPT_TRI_TEST, 1)
        fresh.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        assert lib.pt_render_aux(fresh._ctx, C.byref(cam), C.byref(p), gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, None) == PT_ERR_UNSUPPORTED
        fresh.set_option(g.OPT_TRI_TEST, 0)
        fresh.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        ok = (C.byref(cam), C.byref(p), gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, None)
        for k in range(5):
            args = list(ok)
            args[k] = None
            assert lib.pt_render_aux(fresh._ctx, *args) == PT_ERR_INVALID, k
        for w, h in ((0, 16), (16, 0), (-3, 16)):
            q = g.default_params(W, H)
            q.width, q.height = w, h
            assert lib.pt_render_aux(fresh._ctx, C.byref(cam), C.byref(q), gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, None) == PT_ERR_INVALID
        gb.render(cam, p)
        got = gb.download()
        gb.free()
        compare_guides(got, R.guides(g.Bvh(g.scene_mesh("cornell")), None, cam, p), "after errors")
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------- the filter
def denoise_gpu(t, color, albedo, normal, position, out_alias=False, with_rgba=True, **kw):
    H, W = color.shape[:2]
    dc, da, dn, dp = (t.malloc(max(a.nbytes, 4)) for a in (color, albedo, normal, position))
    for d, a in ((dc, color), (da, albedo), (dn, normal), (dp, position)):
        d.upload(np.ascontiguousarray(a))
    do = dc if out_alias else t.malloc(W * H * 12)
    dr = t.malloc(W * H * 4) if with_rgba else None
    t.denoise(dc.ptr, da.ptr, dn.ptr, dp.ptr, W, H, do.ptr, dr.ptr if dr else None, **kw)
    t.sync()
    out = do.download(np.float32, (H, W, 3))
    rgba = dr.download(np.uint32, (H, W)) if dr else None
    for b in {id(x): x for x in (dc, da, dn, dp, do, dr) if x is not None}.values():
        b.free()
    return out, rgba


_guide_cache = {}


def real_guides(t, W, H):
    """Real guides (the sphere room + cornell, pt_render_aux; frames under 64 pixels a side cut from the middle of a 64-pixel one)
    with a few forced misses, and random colour."""
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


SIGMAS = {"all": (1.0, 0.5, 0.05), "no_color": (0.0, 0.5, 0.05), "no_normal": (1.0, -1.0, 0.05), "no_position": (1.0, 0.5, 0.0),
          "none": (0.0, 0.0, 0.0), "tight": (0.2, 0.1, 0.01)}


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (37, 23)])
@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("sig", list(SIGMAS))
def test_filter_equals_the_reference(t, W, H, iterations, sig):
    col, alb, nrm, pos = real_guides(t, W, H)
    sc, sn, sx = SIGMAS[sig]
    out, rgba = denoise_gpu(t, col, alb, nrm, pos, iterations=iterations, sigma_color=sc, sigma_normal=sn, sigma_position=sx)
    ref = R.atrous(col, alb, nrm, pos, iterations, sc, sn, sx)
    assert np.abs(out - ref).max() <= 1e-4, float(np.abs(out - ref).max())
    assert np.array_equal(rgba, R.pack_rgba(out))
    if iterations == 0:
        assert np.array_equal(out.view(np.int32), col.view(np.int32))


def test_filter_1080p_sampled_pixels(t):
    W, H = 1920, 1080
    col, alb, nrm, pos = real_guides(t, W, H)
    rng = np.random.default_rng(11)
    ys, xs = rng.integers(0, H, 3000), rng.integers(0, W, 3000)
    ys[:4], xs[:4] = (0, H - 1, 0, H - 1), (0, 0, W - 1, W - 1)   # the corners
    for it, sig in ((2, SIGMAS["all"]), (4, SIGMAS["tight"])):
        out, rgba = denoise_gpu(t, col, alb, nrm, pos, iterations=it, sigma_color=sig[0], sigma_normal=sig[1], sigma_position=sig[2])
        ref = R.atrous(col, alb, nrm, pos, it, *sig, pixels=(ys, xs))
        assert np.abs(out[ys, xs] - ref).max() <= 1e-4
        assert np.array_equal(rgba, R.pack_rgba(out))


@pytest.mark.parametrize("iterations", [0, 3])
def test_out_may_alias_color(t, iterations):
    col, alb, nrm, pos = real_guides(t, 37, 23)
    a, ra = denoise_gpu(t, col, alb, nrm, pos, iterations=iterations)
    b, rb = denoise_gpu(t, col, alb, nrm, pos, out_alias=True, iterations=iterations)
    c, _ = denoise_gpu(t, col, alb, nrm, pos, with_rgba=False, iterations=iterations)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(ra, rb)
    assert np.array_equal(a.view(np.int32), c.view(np.int32))


def test_scratch_grows_and_is_reused(t):
    """Small, large, small again: every call equals the reference (the scratch is grown once and reused)."""
    for W, H in ((7, 5), (37, 23), (7, 5)):
        col, alb, nrm, pos = real_guides(t, W, H)
        out, _ = denoise_gpu(t, col, alb, nrm, pos, iterations=2)
        assert np.abs(out - R.atrous(col, alb, nrm, pos, 2, **{k: v for k, v in g.DENOISE_DEFAULTS.items() if k != "iterations"})).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------- with pt_render
def box_frame(t, W, H, spp, frame, rgba=True):
    """cornell_box (materials, black background) rendered with the context's default kernel; accum, rgba buffers."""
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    p.frame, p.sample_index = frame, 1
    p.flags = g.FLAG_WRITE_RGBA
    acc, rg = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, spp)
    return acc, rg, cam, p


def test_denoise_after_render_needs_no_host_sync(t):
    W, H = 320, 240
    mesh, bvh, _, _ = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    t.set_option(g.OPT_OVERLAP, 1)
    results = []
    for sync in (False, True):
        _, _, cam, p = R.cornell_box_scene(W, H)
        gb = Guides(t, W, H)
        gb.render(cam, p)
        acc, rg = t.alloc_frame(W, H)
        out, orgba = t.malloc(W * H * 12), t.malloc(W * H * 4)
        t.sync()
        # several calls in a row: the later ones run their path kernels on a side stream (the caller's stream is busy)
        for k in range(4):
            q = g.Params.from_buffer_copy(p)
            q.frame, q.sample_index, q.flags = 40 + k, 1 + k, g.FLAG_WRITE_RGBA
            t.launch_kernel(acc.ptr, rg.ptr, cam, q, 1)
        if sync:
            t.sync()
        t.denoise(acc.ptr, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr, orgba.ptr)
        t.sync()
        results.append((out.download(np.float32, (H, W, 3)), orgba.download(np.uint32, (H, W)), acc.download(np.float32, (H, W, 3))))
        for b in (acc, rg, out, orgba):
            b.free()
        gb.free()
    t.upload_tri_materials(None, None)
    t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    (a, ra, acc_a), (b, rb, acc_b) = results
    assert np.array_equal(acc_a.view(np.int32), acc_b.view(np.int32))
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(ra, rb)
    assert not np.array_equal(a, acc_a)   # it filtered something


def test_quality_of_the_defaults_on_the_gpu(t):
    W, H = 320, 240
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    t.upload_bvh(bvh)
    t.upload_spheres([])
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    frames = {}
    for name, spp, frame in (("ref", 1024, 0), ("noisy", 4, 1 << 20)):
        acc, rg = t.alloc_frame(W, H)
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = frame, 1
        for k in range(0, spp, 64):   # 64 samples per call
            q.frame, q.sample_index = frame + k, 1 + k
            t.launch_kernel(acc.ptr, rg.ptr, cam, q, min(64, spp - k))
        frames[name] = acc
    gb = Guides(t, W, H)
    gb.render(cam, p)
    out = t.malloc(W * H * 12)
    t.denoise(frames["noisy"].ptr, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr)
    t.sync()
    ref, noisy = frames["ref"].download(np.float32, (H, W, 3)), frames["noisy"].download(np.float32, (H, W, 3))
    den = out.download(np.float32, (H, W, 3))
    for b in (out, frames["ref"], frames["noisy"]):
        b.free()
    gb.free()
    t.upload_tri_materials(None, None)
    gain = R.mse(noisy, ref) / R.mse(den, ref)
    print(f"quality 320x240 4 spp vs 1024 spp: gain {gain:.2f}")
    assert gain >= QUALITY_K, gain


def test_denoise_errors(t):
    lib = g._abi.ptmi()
    W, H = 8, 8
    bufs = [t.malloc(W * H * 16) for _ in range(5)]
    ok = [C.byref(g.DenoiseParams(W, H, 2, 1.0, 0.5, 0.05))] + [b.ptr for b in bufs]
    fresh = g.PathTracer(0)   # no scene needed
    try:
        for k in range(6):    # dp, color, albedo, normal, position, out
            args = list(ok)
            args[k] = None
            assert lib.pt_denoise(t._ctx, *args, None) == PT_ERR_INVALID, k
        for dp in ((0, H, 2, 1, 1, 1), (W, 0, 2, 1, 1, 1), (W, H, -1, 1, 1, 1), (W, H, 11, 1, 1, 1),
                   (W, H, 2, float("nan"), 1, 1), (W, H, 2, 1, float("inf"), 1), (W, H, 2, 1, 1, float("-inf"))):
            assert lib.pt_denoise(t._ctx, C.byref(g.DenoiseParams(*dp)), *ok[1:], None) == PT_ERR_INVALID, dp
        _, alb, nrm, pos = real_guides(t, 37, 23)
        c2 = np.random.default_rng(4).uniform(0, 1, (23, 37, 3)).astype(np.float32)
        out, _ = denoise_gpu(fresh, c2, alb, nrm, pos, iterations=10, sigma_color=1.0, sigma_normal=0.5, sigma_position=0.05)
        assert np.abs(out - R.atrous(c2, alb, nrm, pos, 10, 1.0, 0.5, 0.05)).max() <= 1e-4
    finally:
        fresh.close()
        for b in bufs:
            b.free()
    # the context still renders correctly
    W, H = 64, 64
    bvh, sph, _, _ = setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    acc, rg = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 2)
    t.sync()
    ref, _, _ = orc.render(bvh, sph, cam, p, spp=2)
    assert np.array_equal(acc.download(np.float32, (H, W, 3)), ref)
    acc.free()
    rg.free()


def test_aux_and_denoise_leave_no_trace_in_render(t):
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

    gb = Guides(t, W, H)
    gb.render(cam, p)
    acc, rg = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 3)
    t.denoise(acc.ptr, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, acc.ptr, rg.ptr)   # in place, on purpose
    t.sync()
    acc.free()
    rg.free()
    gb.free()
    a = frame(t)
    clean = g.PathTracer(0)
    try:
        clean.upload_bvh(bvh)
        clean.upload_spheres(sph)
        b = frame(clean)
    finally:
        clean.close()
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_timing_1080p_five_iterations(t):
    W, H = 1920, 1080
    setup_scene(t, "cornell_dragon", False)
    cam, p = golden_camera(W, H), g.default_params(W, H)
    gb = Guides(t, W, H)
    acc, rg = t.alloc_frame(W, H)
    out = t.malloc(W * H * 12)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 1)
    t.set_option(g.OPT_TIMING, 1)
    try:
        gb.render(cam, p)
        aux_ms = t.last_kernel_ms()
        ms = []
        for _ in range(5):
            t.denoise(acc.ptr, gb.alb.ptr, gb.nrm.ptr, gb.pos.ptr, W, H, out.ptr, rg.ptr, iterations=5)
            ms.append(t.last_kernel_ms())
    finally:
        t.set_option(g.OPT_TIMING, 0)
    for b in (acc, rg, out):
        b.free()
    gb.free()
    print(f"1080p: aux {aux_ms:.3f} ms, denoise x5 {sorted(ms)}")
    assert 0 < min(ms) < 5.0 and 0 < aux_ms < 50.0


def test_pt_app_denoise_out(tmp_path):
    """--denoise-out writes an image; the --out image is byte-identical to a run without the flag (one context and a tile
    split over two)."""
    app = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
    base = [app, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "120", "--frames", "4", "--spp", "2"]
    outs = {}
    for k, extra in (("plain", []), ("dn", ["--denoise-out", str(tmp_path / "den.png")]), ("dn_pfm", ["--denoise-out", str(tmp_path / "den.pfm")]),
                     ("plain2", ["--gpus", "2"]), ("dn2", ["--gpus", "2", "--denoise-out", str(tmp_path / "den2.png")])):
        img = tmp_path / f"{k}.png"
        r = subprocess.run(base + ["--out", str(img)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        outs[k] = img.read_bytes()
    same = {k: outs[k] == outs["plain"] for k in outs}
    assert same["dn"] and same["dn_pfm"], same
    assert outs["dn2"] == outs["plain2"], same
    dn = (tmp_path / "den.png").read_bytes()
    assert dn[:8] == b"\x89PNG\r\n\x1a\n" and dn != outs["plain"]
    assert (tmp_path / "den.pfm").read_bytes()[:2] == b"PF"
    if same["plain2"]:   # the gathered frame is the one-context frame: so is its denoised image
        assert (tmp_path / "den2.png").read_bytes() == dn
