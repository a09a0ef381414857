"""pt_upload_environment / pt_eval_environment on the device (extension; contract in include/ptmi.h).

Three references, none of them the code under test: the map itself (a nearest lookup along the directions of a latitude-longitude
frame must return it texel by texel — tests/test_environment.py checks that premise on the CPU), tests/env_ref.py (float64
positions from the definition) and the renderer without a map (a constant map equal to bk_color must give its oracle-checked
images bit for bit).  Images are 37 x 23: no multiple of the 8 x 8 tile or of a wave."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_ref
import orc
from gpu_support import bits, golden_camera, gpu_trace

pytestmark = pytest.mark.gpu
W, H = 37, 23
SIZES = [(1, 1), (5, 3), (16, 8)]
BK = (0.25, 0.5, 0.75)


# ---------------------------------------------------------------------------------------------------- scene and launches
def spheres(rows):
    arr = (g.Sphere * len(rows))()
    for s, (pr, emi, col, mat) in zip(arr, rows):
        s.pos_rad[:], s.emi[:], s.col[:], s.mat = pr, emi, col, mat
    return arr


IN_VIEW = [((5.5, 3.0, 0.0, 1.5), (2.0, 1.5, 1.0), (0.8, 0.8, 0.8), g.MAT_DIFF), ((-8.0, 7.0, 0.0, 1.2), (0, 0, 0), (0.9, 0.9, 0.9), g.MAT_SPEC)]
BEHIND = [((5.5, 3.0, 40.0, 1.5), (2.0, 1.5, 1.0), (0.8, 0.8, 0.8), g.MAT_DIFF), ((-8.0, 7.0, 45.0, 1.2), (0, 0, 0), (0.9, 0.9, 0.9), g.MAT_SPEC)]


def bunny_camera():
    cam = golden_camera(W, H)
    cam.pos[:] = (-1.0, 5.0, 11.0)   # in front of the bunny, looking along -z past it
    return cam


def bunny_params(flags=0, depth=4):
    p = g.default_params(W, H, depth=depth)
    p.bk_color[:] = BK
    p.tri_emi[:] = (0.125, 0.25, 0.0625)
    p.flags = flags
    p.frame = 5
    return p


@pytest.fixture(scope="module")
def t():
    """bunny_low built on the device, two small spheres in view, no map."""
    tr = g.PathTracer(0)
    tr.build_bvh(g.scene_mesh("bunny_low"))
    tr.upload_spheres(spheres(IN_VIEW))
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def sky():
    """A context with no scene worth the name: pt_eval_environment needs none."""
    tr = g.PathTracer(0)
    yield tr
    tr.close()


def fresh_bunny():
    tr = g.PathTracer(0)
    tr.build_bvh(g.scene_mesh("bunny_low"))
    tr.upload_spheres(spheres(IN_VIEW))
    return tr


def render(t, p, spp=4, calls=1, moments=False, parts=1, cam=None):
    """`calls` pt_render calls of spp samples each: the accumulator (and the moments)."""
    cam = bunny_camera() if cam is None else cam
    acc, rgba = t.alloc_frame(W, H)
    mom = t.malloc(W * H * 8) if moments else None
    q = g.Params.from_buffer_copy(p)
    for k in range(calls):
        q.frame, q.sample_index = p.frame + k * spp, 1 + k * spp
        for part in range(parts):
            if parts > 1:
                q.part_index, q.part_count, q.part_rows = part, parts, 8
            t.launch_kernel(acc.ptr, rgba.ptr, cam, q, spp, mom.ptr if moments else None)
    t.sync()
    out = acc.download(np.float32, (H, W, 3))
    m = mom.download(np.float32, (H, W, 2)) if moments else None
    for b in (acc, rgba, mom):
        if b is not None:
            b.free()
    return (out, m) if moments else out


def on_device(t, arr):
    b = t.malloc(max(arr.nbytes, 32))
    b.upload(np.ascontiguousarray(arr))
    return b


def eval_env(t, dirs):
    """pt_eval_environment over directions [n][3]."""
    n = len(dirs)
    r, out = on_device(t, env_ref.rays_of(dirs)), t.malloc(12 * n)
    t.eval_environment(r.ptr, n, out.ptr)
    t.sync()
    got = out.download(np.float32, (n, 3))
    r.free()
    out.free()
    return got


def render_rays(t, rays, p, spp=1, hdr=True):
    n = len(rays)
    r, out = on_device(t, rays), t.malloc(12 * n)
    t.render_rays(r.ptr, n, out.ptr, p, spp, 0, hdr)
    t.sync()
    got = out.download(np.float32, (n, 3))
    r.free()
    out.free()
    return got


def index_map(Wm, Hm):
    """Every texel different, and exactly representable."""
    return np.arange(Wm * Hm * 3, dtype=np.float32).reshape(Hm, Wm, 3)


# ---------------------------------------------------------------------------------------------------- 1: round trip
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_nearest_lookup_over_the_equirect_directions_returns_the_map(sky, size):
    """... bit for bit, for unit directions and for the same directions 1000 times shorter and longer; column 0 from both sides of the
    +-pi seam (the frame's own column 0 looks at longitude -pi with right-component -1.2e-16; the same rays with that component
    +1e-7 arrive from +pi) and the pole row (row 0 looks at latitude -pi/2)."""
    Wm, Hm = size
    tex = index_map(Wm, Hm)
    sky.upload_environment(tex, filter=g.ENV_NEAREST, **env_ref.WORLD)
    d = env_ref.equirect_dirs(Wm, Hm)
    for k in (1.0, 1e-3, 1e3):
        got = eval_env(sky, d * np.float32(k))
        assert np.array_equal(bits(got), bits(tex.reshape(-1, 3))), f"scale {k}: {int(np.any(got != tex.reshape(-1, 3), axis=-1).sum())} texels differ"
    seam = d.reshape(Hm, Wm, 3)[1:, 0].copy()   # column 0 of the rows that are no pole
    if len(seam):
        assert (seam[:, 0] <= 0).all() and np.abs(seam[:, 0]).max() < 1e-6   # right-component: -0 or just below
        seam[:, 0] = 1e-7
        assert np.array_equal(eval_env(sky, seam), tex[1:, 0])
    sky.clear_environment()


# ---------------------------------------------------------------------------------------------------- 2: random directions
def test_random_directions_against_the_reference(sky):
    """4 096 random directions on a 16 x 8 gradient-plus-noise map.  Nearest: the reference's texel exactly wherever the float64
    position is further than 2^-10 from a texel border (at most 1 % are set aside; tests/test_environment.py counts 0.4 %).
    Bilinear: within g * 2^-12 + 4 ulp of the float64 value at the float64 position, g the largest step between adjacent texels.
    A map whose texels hold their own column and row numbers then reads the device's positions back (bilinear, away from the seam and
    the clamped rows, returns fx and fy themselves): the largest error is printed (profiles/r14_environment.txt records it)."""
    Wm, Hm = 16, 8
    tex = env_ref.gradient_map(Wm, Hm)
    d = env_ref.random_dirs(4096)
    fx, fy, valid = env_ref.positions(d, Wm, Hm)
    assert valid.all()
    sky.upload_environment(tex, filter=g.ENV_NEAREST)
    got = eval_env(sky, d)
    near = (np.abs(fx + 0.5 - np.round(fx + 0.5)) <= 2.0 ** -10) | (np.abs(fy + 0.5 - np.round(fy + 0.5)) <= 2.0 ** -10)
    print(f"nearest: {int(near.sum())} of {len(d)} directions set aside")
    assert near.mean() <= 0.01
    ref = env_ref.nearest(tex, fx, fy)
    assert np.array_equal(bits(got[~near]), bits(ref[~near])), f"{int(np.any(got[~near] != ref[~near], axis=-1).sum())} directions pick another texel"

    sky.upload_environment(tex, filter=g.ENV_BILINEAR)
    got = eval_env(sky, d).astype(np.float64)
    err, bound = np.abs(got - env_ref.bilinear(tex, fx, fy)).max(), env_ref.bilinear_bound(tex)
    print(f"bilinear: largest error {err:.3e}, bound {bound:.3e} (g = {env_ref.max_step(tex):.4f})")
    assert err <= bound

    y, x = np.meshgrid(np.arange(Hm, dtype=np.float32), np.arange(Wm, dtype=np.float32), indexing="ij")
    sky.upload_environment(np.stack([x, y, np.zeros_like(x)], -1), filter=g.ENV_BILINEAR)
    got = eval_env(sky, d).astype(np.float64)
    inner = (fx > 0.01) & (fx < Wm - 1.01) & (fy > 0.01) & (fy < Hm - 1.01)   # no wrapped column, no clamped row
    ex, ey = np.abs(got[inner, 0] - fx[inner]).max(), np.abs(got[inner, 1] - fy[inner]).max()
    print(f"position error read back over {int(inner.sum())} directions: fx {ex:.3e} = 2^{np.log2(ex):.1f}, fy {ey:.3e} = 2^{np.log2(ey):.1f} texels")
    assert max(ex, ey) <= 2.0 ** -12   # the margin the bilinear bound grants
    sky.clear_environment()


# ---------------------------------------------------------------------------------------------------- 3: invalid directions
@pytest.mark.parametrize("filt", [g.ENV_NEAREST, g.ENV_BILINEAR], ids=["nearest", "bilinear"])
def test_invalid_directions_are_black(sky, filt):
    sky.upload_environment(env_ref.gradient_map(16, 8), filter=filt)
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 0], [0, 0, 0], [-np.inf, 1, 1], [1, np.nan, np.nan], [-0.0, 0.0, -0.0], [3e38, 3e38, 3e38]], np.float32)
    good = np.array([[0, 0, -1], [1e-30, 0, 0]], np.float32)
    got = eval_env(sky, np.concatenate([bad[:6], good]))
    assert not got[:6].any() and np.array_equal(bits(got[:6]), np.zeros((6, 3), np.int32))
    assert (got[6:] > 0).all()
    # (3e38, 3e38, 3e38) in a frame whose front is (1, 1, 0) / sqrt(2)-ish: the dot product overflows -> black as well
    sky.upload_environment(env_ref.gradient_map(16, 8), front=(1, 1, 0), right=(1, -1, 0), up=(0, 0, 1), filter=filt)
    assert not eval_env(sky, bad[6:]).any()
    sky.clear_environment()


# ---------------------------------------------------------------------------------------------------- 4: constant map = background
def const_map():
    return np.broadcast_to(np.asarray(BK, np.float32), (3, 5, 3)).copy()


def test_the_camera_sees_past_the_mesh(t):
    _, tri, _ = gpu_trace(t, orc.primary_rays(bunny_camera(), W, H, jitter=False))
    share = float((tri < 0).mean())
    print(f"pixel-centre rays that miss the triangles: {100 * share:.1f} %")
    assert 0.2 <= share <= 0.8


FLAGS = [("default", 0), ("smallpt", g.FLAGS_SMALLPT), ("smallpt-nee", g.FLAGS_SMALLPT | g.FLAG_NEE)]
KERNELS = [("mega", g.KERNEL_MEGA_BVH2), ("persistent", g.KERNEL_PERSISTENT), ("wavefront", g.KERNEL_WAVEFRONT)]


@pytest.mark.parametrize("fname,flags", FLAGS, ids=[f[0] for f in FLAGS])
@pytest.mark.parametrize("kname,kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_constant_map_equals_the_background(t, kname, kernel, fname, flags):
    """A 5 x 3 map whose every texel is bk_color: pt_render, 4 spp, depth 4, bit-identical to the same context without a map."""
    t.set_option(g.OPT_KERNEL, kernel)
    p = bunny_params(flags)
    t.clear_environment()
    ref = render(t, p)
    for filt in (g.ENV_BILINEAR, g.ENV_NEAREST):
        t.upload_environment(const_map(), filter=filt)
        got = render(t, p)
        assert np.array_equal(bits(got), bits(ref)), f"{kname} {fname}: {int(np.any(bits(got) != bits(ref), axis=-1).sum())} pixels differ"
    t.clear_environment()
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 1   # (with the default flags most paths end on the bare background: few colours)


def test_constant_map_moments_partition_and_rays(t):
    """... and so do pt_render_moments, a 3-way partition, and pt_render_rays over the camera's own rays."""
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    p, cam = bunny_params(g.FLAGS_SMALLPT), bunny_camera()
    t.clear_environment()
    ref, ref_m = render(t, p, moments=True)
    ref_rays = [render_rays(t, orc.primary_rays(cam, W, H, frame=p.frame + k), frame_of(p, k), hdr=False) for k in range(2)]
    assert np.array_equal(bits(ref_rays[0].reshape(H, W, 3)), bits(render(t, p, spp=1))), "the premise: the camera's rays give its image"
    t.upload_environment(const_map())
    got, got_m = render(t, p, moments=True)
    assert np.array_equal(bits(got), bits(ref)) and np.array_equal(bits(got_m), bits(ref_m))
    assert np.array_equal(bits(render(t, p, parts=3)), bits(ref))
    for k in range(2):
        assert np.array_equal(bits(render_rays(t, orc.primary_rays(cam, W, H, frame=p.frame + k), frame_of(p, k), hdr=False)), bits(ref_rays[k]))
    t.clear_environment()


def frame_of(p, k):
    q = g.Params.from_buffer_copy(p)
    q.frame = p.frame + k
    return q


# ---------------------------------------------------------------------------------------------------- 5: a real map along rays
@pytest.mark.parametrize("filt", [g.ENV_NEAREST, g.ENV_BILINEAR], ids=["nearest", "bilinear"])
def test_rays_that_miss_carry_the_map_and_rays_that_hit_carry_the_emission(t, filt):
    """pt_render_rays, HDR, depth 1, one sample, on a 16 x 8 gradient map; the spheres stand behind the rays' origins.  A ray that
    pt_trace_rays reports as a miss carries pt_eval_environment of the same ray bit for bit, a ray that hits carries tri_emi."""
    t.upload_spheres(spheres(BEHIND))
    t.upload_environment(env_ref.gradient_map(16, 8), filter=filt)
    p = bunny_params(depth=1)
    rays = orc.primary_rays(bunny_camera(), W, H, jitter=False)
    extra = orc.random_rays(1000, *g.scene_mesh("bunny_low").bounds(), seed=4)   # all around the bunny: every latitude of the map
    extra = extra[extra[:, 6] < 0.0]   # ... heading away from the spheres at z = +40
    rays = np.concatenate([rays, extra])
    _, tri, _ = gpu_trace(t, rays)
    miss = tri < 0
    assert 100 < miss.sum() < len(rays) - 100
    got = render_rays(t, rays, p)
    sky = eval_env(t, rays[:, 4:7])
    assert np.array_equal(bits(got[miss]), bits(sky[miss])), f"{int(np.any(bits(got[miss]) != bits(sky[miss]), axis=-1).sum())} missing rays differ"
    assert np.array_equal(got[~miss], np.broadcast_to(np.asarray(p.tri_emi[:], np.float32), (int((~miss).sum()), 3)))
    assert len(np.unique(sky[miss], axis=0)) > 50   # a real map: the rays see many texels
    t.clear_environment()
    t.upload_spheres(spheres(IN_VIEW))


# ---------------------------------------------------------------------------------------------------- 6: one mirror bounce
def test_one_mirror_bounce():
    """A two-triangle mirror quad in the plane z = 0, depth 2: with PT_FLAG_MISS_KEEPS_PATH the radiance is tri_col * env(reflect(d, n)),
    without it the bare env(...) — the reference's unmasked miss.  Against env_ref at the float64 reflection, within test 2's bound
    (tri_col < 1 shrinks the lookup's error by more than the product's one rounding adds)."""
    tr = g.PathTracer(0)
    quad = np.array([[-50, -50, 0], [50, -50, 0], [50, 50, 0], [-50, 50, 0]], np.float32)
    tr.build_bvh(g.Mesh.from_arrays(quad, np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
    tex = env_ref.gradient_map(16, 8)
    tr.upload_environment(tex, filter=g.ENV_BILINEAR)
    rng = np.random.default_rng(9)
    n = 600
    d = np.concatenate([rng.uniform(-2, 2, (n, 2)), -np.ones((n, 1))], 1)   # downwards, at most 71 degrees off the normal: onto the quad
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = env_ref.rays_of(d)
    rays[:, 0:3] = rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.array([0, 0, 5], np.float32)
    _, tri, _ = gpu_trace(tr, rays)
    assert (tri >= 0).all()
    refl = d.astype(np.float64) * np.array([1, 1, -1.0])
    fx, fy, valid = env_ref.positions(refl, 16, 8)   # (float64 directions pass through float32 inside: 1e-7 of a turn, far below the margin)
    ref = env_ref.bilinear(tex, fx, fy, valid)
    bound = env_ref.bilinear_bound(tex)
    p = g.default_params(W, H, depth=2, tri_mat=g.MAT_SPEC)
    p.tri_col[:] = (0.5, 0.25, 0.75)
    p.bk_color[:] = (9, 9, 9)
    col = np.asarray(p.tri_col[:], np.float32).astype(np.float64)
    p.flags = g.FLAG_MISS_KEEPS_PATH
    got = render_rays(tr, rays, p).astype(np.float64)
    print(f"masked: largest error {np.abs(got - col * ref).max():.3e}, bound {bound:.3e}")
    assert np.abs(got - col * ref).max() <= bound
    p.flags = 0
    got = render_rays(tr, rays, p).astype(np.float64)
    print(f"bare: largest error {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= bound
    tr.close()


# ---------------------------------------------------------------------------------------------------- 7: the fall-back
def test_with_a_map_the_pipeline_falls_back_to_the_persistent_kernel(t):
    p = bunny_params(g.FLAGS_SMALLPT)
    t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
    t.clear_environment()
    plain = render(t, p)
    t.upload_environment(env_ref.gradient_map(16, 8))
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    ref = render(t, p)
    assert np.any(bits(ref) != bits(plain))
    t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
    assert np.array_equal(bits(render(t, p)), bits(ref))
    t.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    for k in range(6):
        assert np.array_equal(bits(render(t, p)), bits(ref)), f"PT_KERNEL_AUTO, call {k}"
    assert t.auto_choice()[0] in (g.KERNEL_AUTO, g.KERNEL_PERSISTENT)   # no trial ran: nothing was decided, or the fall-back
    t.set_option(g.OPT_TIMING, 1)
    try:
        for kernel in (g.KERNEL_WAVEFRONT, g.KERNEL_AUTO):
            t.set_option(g.OPT_KERNEL, kernel)
            render(t, p)
            ms = t.stage_ms()
            assert ms["extend"] == 0 and ms["frame"] > 0, ms
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.clear_environment()
        again = render(t, p)
        ms = t.stage_ms()
        assert ms["extend"] > 0 and ms["frame"] == 0, ms
        assert np.array_equal(bits(again), bits(plain))
    finally:
        t.set_option(g.OPT_TIMING, 0)


# ---------------------------------------------------------------------------------------------------- 8: order and replacement
def test_a_render_reads_the_map_that_was_there_when_it_was_issued(t):
    """Render with map A, upload B without syncing, render again: the first image is a fresh context's with A, the second a fresh
    context's with B.  And four samples in one call equal four calls of one."""
    A, B = env_ref.gradient_map(16, 8, seed=1), env_ref.gradient_map(5, 3, seed=2) * np.float32(2.0)
    p, cam = bunny_params(g.FLAGS_SMALLPT), bunny_camera()
    t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    t.upload_environment(A)
    acc = [t.alloc_frame(W, H) for _ in range(2)]
    t.sync()
    t.launch_kernel(acc[0][0].ptr, acc[0][1].ptr, cam, p, 4)
    t.launch_kernel(acc[0][0].ptr, acc[0][1].ptr, cam, p, 4)   # a second call in flight: the side stream of PT_OPT_OVERLAP
    t.upload_environment(B)                                    # no sync from the caller
    t.launch_kernel(acc[1][0].ptr, acc[1][1].ptr, cam, p, 4)
    t.sync()
    got = [a.download(np.float32, (H, W, 3)) for a, _ in acc]
    for a, r in acc:
        a.free()
        r.free()
    one_by_one = render(t, p, spp=1, calls=4)
    t.clear_environment()
    fresh = fresh_bunny()
    fresh.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
    fresh.upload_environment(B)
    ref_b = render(fresh, p)
    fresh.upload_environment(A)
    ref_a = render(fresh, p)
    fresh.close()
    assert np.any(bits(ref_a) != bits(ref_b))
    assert np.array_equal(bits(got[0]), bits(ref_a)), "the render issued before the upload"
    assert np.array_equal(bits(got[1]), bits(ref_b)), "the render issued after the upload"
    assert np.array_equal(bits(one_by_one), bits(ref_b)), "four calls of one sample"


# ---------------------------------------------------------------------------------------------------- 9: errors
def test_errors_come_in_the_documented_order(sky):
    lib, ctx = sky._lib, sky._ctx
    INVALID, NO_SCENE = -1, -3

    def env(w=5, h=3, filt=g.ENV_BILINEAR, front=(0, 0, -1), right=(1, 0, 0), up=(0, 1, 0), scale=(1, 1, 1)):
        e = g.Environment()
        e.width, e.height, e.filter = w, h, filt
        e.front[:], e.right[:], e.up[:], e.scale[:] = front, right, up, scale
        return e

    def upload(e, tex):
        a = None if tex is None else np.ascontiguousarray(tex, np.float32)
        return lib.pt_upload_environment(ctx, C.byref(e), None if a is None else a.ctypes.data)

    rays = on_device(sky, env_ref.rays_of(env_ref.equirect_dirs(5, 3)))
    out = sky.malloc(12 * 15)
    sky.clear_environment()
    assert lib.pt_eval_environment(ctx, rays.ptr, 15, out.ptr) == NO_SCENE
    good = index_map(5, 3) + 1
    assert upload(env(filt=g.ENV_NEAREST), good) == 0
    one = np.ones((1, 1, 3), np.float32)
    # the struct is checked before the texels are touched: a one-texel buffer behind a 16385-wide header is never read
    assert upload(env(), None) == INVALID and "texels" in sky._lib.pt_last_error(ctx).decode()
    assert upload(env(w=16385, h=1), one) == INVALID and "width" in sky._lib.pt_last_error(ctx).decode()
    assert upload(env(w=0), one) == INVALID and upload(env(w=16384, h=8192), one) == INVALID   # 2^27 texels
    assert upload(env(w=16384, h=16384, filt=2), one) == INVALID and "width" in sky._lib.pt_last_error(ctx).decode()   # the dimension first
    assert upload(env(w=1, h=1, filt=2), one) == INVALID and "filter" in sky._lib.pt_last_error(ctx).decode()
    assert upload(env(w=16384, h=4096, front=(np.nan, 0, 0)), one) == INVALID and "front" in sky._lib.pt_last_error(ctx).decode()   # 2^26 texels never read
    assert upload(env(w=16384, h=4096, up=(0, 0, 0)), one) == INVALID
    assert upload(env(w=16384, h=4096, scale=(1, -1, 1)), one) == INVALID and "scale" in sky._lib.pt_last_error(ctx).decode()
    assert upload(env(w=16384, h=4096, scale=(1, np.inf, 1)), one) == INVALID
    bad = good.copy()
    bad[2, 4, 1] = -1.0
    assert upload(env(), bad) == INVALID and "texel" in sky._lib.pt_last_error(ctx).decode()
    bad[2, 4, 1] = np.nan
    assert upload(env(), bad) == INVALID
    assert upload(env(scale=(1, 1, 3e38)), good) == INVALID   # finite texels, not finite once scaled
    with pytest.raises(g.PtError):
        sky.upload_environment(bad)
    # the old map survived every refusal
    sky.set_option(g.OPT_TIMING, 1)
    assert lib.pt_eval_environment(ctx, rays.ptr, 0, None) == 0
    assert lib.pt_eval_environment(ctx, None, 15, out.ptr) == INVALID and lib.pt_eval_environment(ctx, rays.ptr, 15, None) == INVALID
    assert lib.pt_eval_environment(ctx, rays.ptr, 1 << 32, out.ptr) == INVALID
    sky.eval_environment(rays.ptr, 15, out.ptr)
    sky.sync()
    assert sky.last_kernel_ms() > 0
    sky.set_option(g.OPT_TIMING, 0)
    assert np.array_equal(out.download(np.float32, (15, 3)), env_ref.nearest(good, *env_ref.positions(env_ref.equirect_dirs(5, 3), 5, 3)[:2]))
    sky.clear_environment()
    assert lib.pt_eval_environment(ctx, rays.ptr, 15, out.ptr) == NO_SCENE
    rays.free()
    out.free()
