"""The environment map as a light on the device (PT_OPT_ENV_LIGHT; contract in include/ptmi.h).

References, none of them the code under test: tests/env_light_ref.py (the tables in float64 and the draw in float32, from the
definition; tests/test_env_light.py checks its properties on the CPU), closed forms in float64 (the map's integral, the radiance of
a diffuse plane under a nearest map), the same call without the tables (same expectation, by bounce rays), and the renderer
itself (pt_render against pt_render_rays).  Maps and scenes are tiny; the estimator tests draw 2^16 - 2^18 one-sample paths."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_light_ref as ref
import env_ref
import orc
from gpu_support import bits, golden_camera, gpu_trace

pytestmark = pytest.mark.gpu
OPT_ENV_LIGHT = g._abi.OPT_ENV_LIGHT
NEE_FLAGS = g.FLAG_FACE_FORWARD | g.FLAG_COSINE_DIFF | g.FLAG_MISS_KEEPS_PATH | g.FLAG_NEE   # FLAGS_SMALLPT without the roulette, + NEE
ALBEDO = (0.5, 0.6, 0.7)
TILTED = dict(front=(0.6, 0.0, -0.8), right=(0.8, 0.0, 0.6), up=(0.0, 1.0, 0.0))   # orthonormal, no axis of the world but up


@pytest.fixture(scope="module")
def sky():
    """A context with no scene: the batch calls need none."""
    tr = g.PathTracer(0)
    yield tr
    tr.close()


def on_device(t, arr):
    b = t.malloc(max(arr.nbytes, 32))
    b.upload(np.ascontiguousarray(arr))
    return b


def sample(t, u):
    """pt_sample_environment over u [n][2]: (dir_pdf [n][4], radiance [n][3])."""
    n = len(u)
    d_u, d_o, d_r = on_device(t, np.asarray(u, np.float32)), t.malloc(16 * n), t.malloc(12 * n)
    t.sample_environment(d_u.ptr, n, d_o.ptr, d_r.ptr)
    t.sync()
    out = d_o.download(np.float32, (n, 4)), d_r.download(np.float32, (n, 3))
    for b in (d_u, d_o, d_r):
        b.free()
    return out


def batch(t, call, dirs, width):
    """call(rays, n, out) over directions [n][3]: float32 [n][width] (pt_eval_environment, pt_environment_pdf)."""
    n = len(dirs)
    r, out = on_device(t, env_ref.rays_of(dirs)), t.malloc(4 * width * n)
    call(r.ptr, n, out.ptr)
    t.sync()
    got = out.download(np.float32, (n, width) if width > 1 else (n,))
    r.free()
    out.free()
    return got


def render_rays(t, rays, p, spp=1, hdr=True, out=None):
    n = len(rays)
    r = on_device(t, rays)
    o = t.malloc(12 * n) if out is None else out
    t.render_rays(r.ptr, n, o.ptr, p, spp, 0, hdr)
    t.sync()
    got = o.download(np.float32, (n, 3))
    r.free()
    if out is None:
        o.free()
    return got


def params(W, H, depth, flags=NEE_FLAGS, frame=5):
    p = g.default_params(W, H, depth=depth)
    p.tri_col[:] = ALBEDO
    p.tri_emi[:] = (0, 0, 0)
    p.bk_color[:] = (0.25, 0.5, 0.75)
    p.flags, p.frame = flags, frame
    return p


def ground(y=0.0, half=50.0):
    """Two triangles in the plane y = `y`, facing up."""
    v = np.array([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]], np.float32)
    return g.Mesh.from_arrays(v, np.array([[0, 2, 1], [0, 3, 2]], np.int32))


# ---------------------------------------------------------------------------------------------------- 1: draws against the reference
CASES = ref.draw_cases() + [("16x8-gradient-bilinear-tilted", env_ref.gradient_map(16, 8), True)]


@pytest.mark.parametrize("name,tex,bil", CASES, ids=[c[0] for c in CASES])
def test_draws_against_the_reference(sky, name, tex, bil):
    """A 64 x 64 stratified grid of u plus the corners 0 and 1 - 2^-24: every draw lands in the reference's texel (read back from the
    device's direction through env_ref.positions, on the draws at least 1 % of the texel away from its edges, where the direction's
    rounding cannot cross one), its direction within 1e-5 and its density within 1e-5 relative of the reference's; the radiance is
    pt_eval_environment of the returned directions and the density pt_environment_pdf of them, bit for bit (the latter on the
    interior draws, which are at least 95 %)."""
    H, W = tex.shape[:2]
    basis = TILTED if name.endswith("tilted") else env_ref.WORLD
    sky.upload_environment(tex, filter=g.ENV_BILINEAR if bil else g.ENV_NEAREST, light=True, **basis)
    assert sky.environment_is_light()
    u = ref.stratified(64)
    s = ref.draw(ref.Tables(tex, bil), u, **basis)
    got, rad = sample(sky, u)
    d, pdf = got[:, :3], got[:, 3]
    inner = ref.interior(s)
    print(f"{name}: {100 * inner.mean():.2f} % interior, direction error {np.abs(d - s['d']).max():.2e}, "
          f"density error {np.abs(pdf / s['pdf'] - 1).max():.2e} relative")
    assert inner.mean() >= 0.95
    y, x, valid = ref.texel_of(d[inner], W, H, **basis)
    assert valid.all() and np.array_equal(y, s["y"][inner]) and np.array_equal(x, s["x"][inner]), "a draw landed in another texel"
    assert np.abs(d - s["d"]).max() <= 1e-5
    assert (np.abs(pdf.astype(np.float64) - s["pdf"]) <= 1e-5 * s["pdf"]).all()
    assert np.array_equal(bits(rad), bits(batch(sky, sky.eval_environment, d, 3)))
    back = batch(sky, sky.environment_pdf, d, 1)
    assert np.array_equal(bits(back[inner]), bits(pdf[inner]))
    sky.clear_environment()


def test_u_outside_the_unit_square_is_clamped(sky):
    tex = env_ref.gradient_map(16, 8)
    sky.upload_environment(tex, filter=g.ENV_NEAREST, light=True)
    u = np.array([[-1, 0.5], [0.5, 2], [np.nan, np.nan], [np.inf, -np.inf], [1.0, 1.0], [0.25, 0.75]], np.float32)
    got, _ = sample(sky, u)
    want, _ = sample(sky, ref.clamp_u(u))
    assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).all() and (got[:, 3] > 0).all()
    bad = np.array([[np.nan, 0, 1], [0, 0, 0], [np.inf, 0, 0]], np.float32)
    assert np.array_equal(batch(sky, sky.environment_pdf, bad, 1), np.zeros(3, np.float32))
    sky.clear_environment()


# ---------------------------------------------------------------------------------------------------- 2: the estimator's identity
def test_radiance_over_density_is_the_maps_integral(sky):
    """A grey, strictly positive 8 x 4 nearest map: every draw has L / pdf = I = sum L_t Omega_t (float64, from the reference) up to
    the rounding of the two CDF differences the density is made of: |L / pdf - I| <= I * 4 * 2^-24 / min(px, py).  u: the stratified
    grid and the corner 1 - 2^-24, not the corner 0: u1 = 0 draws the pole itself (z = -1, r = 0), the one direction where the
    columns of row 0 meet and the lookup's longitude is atan2f(0, 0) = 0 — column W / 2 whatever column was drawn (include/ptmi.h
    says so; a path draws it once in 2^24 visits of row 0)."""
    grey = np.repeat(env_ref.gradient_map(8, 4)[:, :, :1], 3, axis=2)
    assert (grey > 0).all()
    sky.upload_environment(grey, filter=g.ENV_NEAREST, light=True)
    u = np.delete(ref.stratified(64), -2, axis=0)
    tab = ref.Tables(grey, False)
    s = ref.draw(tab, u)
    got, rad = sample(sky, u)
    I = ref.integral(tab, grey)[0]
    est = rad[:, 0].astype(np.float64) / got[:, 3].astype(np.float64)
    bound = I * 4 * 2.0 ** -24 / np.minimum(s["px"], s["py"]).astype(np.float64)
    print(f"I = {I:.6f}; largest |L / pdf - I| / bound = {(np.abs(est - I) / bound).max():.3f}")
    assert (np.abs(est - I) <= bound).all()
    sky.clear_environment()


# ---------------------------------------------------------------------------------------------------- 3: closed form, variance
def mean_and_se(x):
    x = x.astype(np.float64)
    return x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(len(x))


def test_a_small_sun_over_a_diffuse_plane():
    """A ground quad of albedo (0.5, 0.6, 0.7) under a black 64 x 32 nearest map with one texel of radiance 1000 at latitude 40
    degrees; 2^16 identical rays straight down, one sample each with its own random stream, depth 2: every ray is one sample of
    E = rho / pi * L * (2 pi / W) * (zs[y+1]^2 - zs[y]^2) / 2.  With the map as a light the mean is E within 5 standard errors and
    the standard error is below 2 % of E (the contribution varies by the cosine across one texel only); without, the mean is E
    within 5 of its own standard errors (a Bernoulli of p ~ 1.5e-3 per sample) — and the light's standard error is at least 4
    times smaller (measured: profiles/r15_env_light.txt)."""
    t = g.PathTracer(0)
    t.build_bvh(ground())
    tex = ref.hot_map(64, 32, 23, 10)
    E = ref.plane_radiance(ref.Tables(tex, False), tex, ALBEDO)
    n = 1 << 16
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7] = (7.0, 5.0, -3.0), (0.0, -1.0, 0.0)   # near the quad's centre, off the edge its triangles share
    p = params(64, 64, depth=2)
    stats = {}
    for light in (True, False):
        t.upload_environment(tex, filter=g.ENV_NEAREST, light=light)
        assert t.environment_is_light() == light
        stats[light] = mean_and_se(render_rays(t, rays, p))
    t.close()
    (m1, se1), (m0, se0) = stats[True], stats[False]
    print(f"E = {E}\nlight:  mean {m1}, SE {se1} ({(se1 / E).max():.2e} of E), (mean - E) / SE {(m1 - E) / se1}\n"
          f"bounce: mean {m0}, SE {se0}, (mean - E) / SE {(m0 - E) / se0}\nSE ratio bounce / light: {se0 / se1}")
    assert (E > 0).all()
    assert (np.abs(m1 - E) <= 5 * se1).all() and (se1 <= 0.02 * E).all()
    assert (np.abs(m0 - E) <= 5 * se0).all()
    assert (se1 <= se0 / 4).all()


# ---------------------------------------------------------------------------------------------------- 4: occlusion, further bounces
W, H = 37, 23


def bunny_camera():
    cam = golden_camera(W, H)
    cam.pos[:] = (-1.0, 5.0, 11.0)   # test_gpu_environment's: in front of the bunny, looking along -z past it
    return cam


@pytest.fixture(scope="module")
def bunny():
    """bunny_low standing on the ground quad (the quad's two triangles are the last two ids), built on the device; the 8 x 4 map."""
    mesh = g.scene_mesh("bunny_low")
    lo, hi = (np.asarray(v, np.float64) for v in mesh.bounds())
    n_bunny = mesh.n_tris
    mesh.append(ground(y=float(lo[1])))
    tr = g.PathTracer(0)
    tr.build_bvh(mesh)
    tex = ref.hot_map(8, 4, 3, 2, value=20.0, ambient=0.2)
    yield tr, n_bunny, (lo + hi) / 2.0, tex
    tr.close()


def test_light_and_bounce_agree_behind_occluders(bunny):
    """Depth 4, bilinear: 16 camera pixels — 8 on the bunny, the 8 on the ground nearest to it, where its shadow falls — 2^14
    identical rays each: the means with and without the tables agree per pixel and channel within 5 combined standard errors."""
    t, n_bunny, centre, tex = bunny
    rays = orc.primary_rays(bunny_camera(), W, H, jitter=False)
    dist, tri, _ = gpu_trace(t, rays)
    on_mesh = np.flatnonzero((tri >= 0) & (tri < n_bunny))
    on_ground = np.flatnonzero(tri >= n_bunny)
    assert len(on_mesh) >= 8 and len(on_ground) >= 8
    hit = rays[on_ground, 0:3] + dist[on_ground, None] * rays[on_ground, 4:7]
    near = on_ground[np.argsort(np.hypot(hit[:, 0] - centre[0], hit[:, 2] - centre[2]))[:8]]
    pick = np.concatenate([on_mesh[np.linspace(0, len(on_mesh) - 1, 8).astype(int)], near])
    per = 1 << 14
    batch_rays = np.repeat(rays[pick], per, axis=0)
    p = params(W, H, depth=4)
    stats = {}
    for light in (True, False):
        t.upload_environment(tex, filter=g.ENV_BILINEAR, light=light)
        assert t.environment_is_light() == light
        got = render_rays(t, batch_rays, p).reshape(16, per, 3).astype(np.float64)
        stats[light] = got.mean(axis=1), got.std(axis=1, ddof=1) / np.sqrt(per)
    t.clear_environment()
    (m1, se1), (m0, se0) = stats[True], stats[False]
    z = (m1 - m0) / np.sqrt(se1 ** 2 + se0 ** 2)
    print(f"means (light) {m1[:, 0]}\nmeans (bounce) {m0[:, 0]}\nlargest |difference| in combined standard errors: {np.abs(z).max():.2f}; SE ratio {np.median(se0 / se1):.2f}")
    assert (m1 > 0).all() and (np.abs(z) <= 5).all()


# ---------------------------------------------------------------------------------------------------- 5: both kernels
def test_the_megakernel_and_the_rays_kernel_agree(bunny):
    """pt_render, 32 x 32, 4 samples, the map a light: the image equals pt_render_rays over that camera's own jittered rays, sample by
    sample, bit for bit."""
    t, _, _, tex = bunny
    w = h = 32
    cam = golden_camera(w, h)
    cam.pos[:] = (-1.0, 5.0, 11.0)
    t.upload_environment(tex, filter=g.ENV_BILINEAR, light=True)
    p = params(w, h, depth=4)
    acc, rgba = t.alloc_frame(w, h)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 4)
    t.sync()
    image = acc.download(np.float32, (h, w, 3))
    out = t.malloc(12 * w * h)
    for k in range(4):
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = p.frame + k, 1 + k
        got = render_rays(t, orc.primary_rays(cam, w, h, frame=p.frame + k), q, hdr=False, out=out)
    plain = render_frame(t, cam, p, 4, light_map=(tex, False))
    for b in (acc, rgba, out):
        b.free()
    t.clear_environment()
    assert np.array_equal(bits(got.reshape(h, w, 3)), bits(image)), f"{int(np.any(bits(got.reshape(h, w, 3)) != bits(image), axis=-1).sum())} pixels differ"
    assert np.any(bits(plain) != bits(image)), "the tables changed nothing: the light was never sampled"


def render_frame(t, cam, p, spp, light_map=None, **kw):
    """One pt_render call into a fresh accumulator, after uploading light_map = (texels, light) when given."""
    if light_map is not None:
        t.upload_environment(light_map[0], filter=kw.pop("filter", g.ENV_BILINEAR), light=light_map[1], **kw)
    acc, rgba = t.alloc_frame(p.width, p.height)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
    t.sync()
    out = acc.download(np.float32, (p.height, p.width, 3))
    acc.free()
    rgba.free()
    return out


# ---------------------------------------------------------------------------------------------------- 6: what must not move
def test_what_the_tables_must_not_change(bunny):
    t, _, _, tex = bunny
    cam = bunny_camera()
    sheared = dict(front=(0.0, 0.0, -1.0), right=(1.0, 0.01, 0.0), up=(0.0, 1.0, 0.0))
    black = np.zeros((4, 8, 3), np.float32)
    cases = [("no NEE", params(W, H, 4, flags=g.FLAGS_SMALLPT), tex, {}, True),
             ("NEE without MISS_KEEPS_PATH", params(W, H, 4, flags=g.FLAG_FACE_FORWARD | g.FLAG_COSINE_DIFF | g.FLAG_NEE), tex, {}, True),
             ("a sheared basis", params(W, H, 4), tex, sheared, False),
             ("a black map", params(W, H, 4), black, {}, False)]
    for name, p, m, basis, is_light in cases:
        ref_frame = render_frame(t, cam, p, 4, light_map=(m, False), **basis)
        got = render_frame(t, cam, p, 4, light_map=(m, True), **basis)
        assert t.environment_is_light() == is_light, name
        assert np.array_equal(bits(got), bits(ref_frame)), f"{name}: {int(np.any(bits(got) != bits(ref_frame), axis=-1).sum())} pixels differ"
    # and where it applies, it does change the frame
    assert np.any(bits(render_frame(t, cam, params(W, H, 4), 4, light_map=(tex, True))) != bits(render_frame(t, cam, params(W, H, 4), 4, light_map=(tex, False))))
    # the option is read by the upload: a clear and an upload with it back at 0 drop the tables
    t.upload_environment(tex, light=True)
    assert t.environment_is_light()
    t.clear_environment()
    assert not t.environment_is_light()
    t.upload_environment(tex)
    assert not t.environment_is_light()
    assert t._lib.pt_sample_environment(t._ctx, None, 0, None, None) == -5   # PT_ERR_UNSUPPORTED, before n or any pointer is looked at
    t.clear_environment()


# ---------------------------------------------------------------------------------------------------- 7: errors
def test_errors_come_in_the_documented_order(sky):
    lib, ctx = sky._lib, sky._ctx
    INVALID, UNSUPPORTED, NO_SCENE = -1, -5, -3
    tex = env_ref.gradient_map(5, 3)
    u = on_device(sky, ref.stratified(4))
    n = 18
    out, rad, pdf = sky.malloc(16 * n), sky.malloc(12 * n), sky.malloc(4 * n)
    rays = on_device(sky, env_ref.rays_of(env_ref.equirect_dirs(5, 3)))
    for v in (-1, 2, 7):
        assert lib.pt_set_option(ctx, OPT_ENV_LIGHT, v) == INVALID
    is_light = C.c_int(5)
    assert lib.pt_environment_is_light(ctx, None) == INVALID
    sky.clear_environment()
    assert lib.pt_environment_is_light(ctx, C.byref(is_light)) == 0 and is_light.value == 0
    assert lib.pt_sample_environment(ctx, None, 0, None, None) == NO_SCENE and lib.pt_environment_pdf(ctx, None, 0, None) == NO_SCENE
    sky.upload_environment(tex, filter=g.ENV_NEAREST)
    assert lib.pt_sample_environment(ctx, None, 0, None, None) == UNSUPPORTED and lib.pt_environment_pdf(ctx, None, 0, None) == UNSUPPORTED
    assert "no light" in lib.pt_last_error(ctx).decode()
    sky.upload_environment(tex, filter=g.ENV_NEAREST, light=True)
    sky.set_option(g.OPT_TIMING, 1)
    assert lib.pt_sample_environment(ctx, None, 0, None, None) == 0 and lib.pt_environment_pdf(ctx, None, 0, None) == 0
    assert lib.pt_sample_environment(ctx, None, n, out.ptr, None) == INVALID and lib.pt_sample_environment(ctx, u.ptr, n, None, rad.ptr) == INVALID
    assert lib.pt_sample_environment(ctx, None, 1 << 32, out.ptr, None) == INVALID and "null" in lib.pt_last_error(ctx).decode()   # the pointer first
    assert lib.pt_sample_environment(ctx, u.ptr, 1 << 32, out.ptr, None) == INVALID and "2^32" in lib.pt_last_error(ctx).decode()
    assert lib.pt_environment_pdf(ctx, None, 15, pdf.ptr) == INVALID and lib.pt_environment_pdf(ctx, rays.ptr, 15, None) == INVALID
    assert lib.pt_environment_pdf(ctx, rays.ptr, 1 << 32, pdf.ptr) == INVALID
    # a refused upload leaves the old map and its tables in place: the same draws before and after
    sky.sample_environment(u.ptr, n, out.ptr, None)   # radiance may be NULL
    sky.sync()
    assert sky.last_kernel_ms() > 0
    before = out.download(np.float32, (n, 4))
    bad = tex.copy()
    bad[1, 1, 1] = -1.0
    sky.set_option(OPT_ENV_LIGHT, 1)
    e = g.Environment()
    e.width, e.height, e.filter = 5, 3, 2   # an unknown filter
    e.front[:], e.right[:], e.up[:], e.scale[:] = (0, 0, -1), (1, 0, 0), (0, 1, 0), (1, 1, 1)
    assert lib.pt_upload_environment(ctx, C.byref(e), bad.ctypes.data) == INVALID
    e.filter = g.ENV_NEAREST
    assert lib.pt_upload_environment(ctx, C.byref(e), bad.ctypes.data) == INVALID and "texel" in lib.pt_last_error(ctx).decode()
    sky.set_option(OPT_ENV_LIGHT, 0)
    assert sky.environment_is_light()
    sky.sample_environment(u.ptr, n, out.ptr, rad.ptr)
    sky.environment_pdf(rays.ptr, 15, pdf.ptr)
    sky.sync()
    assert sky.last_kernel_ms() > 0
    assert np.array_equal(bits(out.download(np.float32, (n, 4))), bits(before))
    s = ref.draw(ref.Tables(tex, False), ref.stratified(4))
    assert np.abs(before[:, :3] - s["d"]).max() <= 1e-5
    want = ref.pdf_of(ref.Tables(tex, False), env_ref.equirect_dirs(5, 3))
    assert len(np.unique(want)) == 15 and np.allclose(pdf.download(np.float32, (15,)), want, rtol=1e-5, atol=0)   # every texel its own density
    sky.set_option(g.OPT_TIMING, 0)
    sky.clear_environment()
    for b in (u, out, rad, pdf, rays):
        b.free()
