"""pt_render_rays — the path loop over a caller's rays (extension; contract in include/ptmi.h).

The reference of every case is the CPU oracle or pt_render itself: orc.primary_rays(cam, W, H, frame=f) are exactly the jittered
first segments of the samples with frame f (tests/test_render_rays.py checks that premise on the CPU), so a batch made of them
must reproduce the camera's image bit for bit; rays no camera makes are checked at depth 1, where no random draw decides
anything."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_trees as dt
import gpu_pathtracer_amd as g
import orc
from denoise_ref import sphere_intersect
from gpu_support import MAX_DIFF, bits, golden_camera, setup_scene, soup_mesh, twist
from scene_matrix import make_camera, tilted_grid_table

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")
F0 = 7   # first frame number of the multi-call cases


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)   # what pt_render runs beside it; pt_render_rays does not read the option
    yield tr
    tr.close()


class Batch:
    """A ray batch and its radiance on the device."""

    def __init__(self, t, rays, init=None):
        self.t, self.n = t, len(rays)
        self.rays = t.malloc(max(rays.nbytes, 32))
        self.rays.upload(np.ascontiguousarray(rays, np.float32))
        self.out = t.malloc(12 * self.n + 12)   # one spare row: the canary of the nothing-written cases
        self.out.upload(np.full((self.n + 1, 3), -7.0, np.float32) if init is None else init)

    def set_rays(self, rays):
        self.rays.upload(np.ascontiguousarray(rays, np.float32))

    def render(self, p, spp=1, first_index=0, hdr=False, first=0, n=None):
        n = self.n - first if n is None else n
        self.t.render_rays(self.rays.ptr + 32 * first, n, self.out.ptr + 12 * first, p, spp, first_index, hdr)

    def get(self):
        self.t.sync()
        return self.out.download(np.float32, (self.n, 3))

    def free(self):
        self.rays.free()
        self.out.free()


def params(W, H, frame=F0, sample_index=1, **kw):
    p = g.default_params(W, H, **kw)
    p.frame, p.sample_index = frame, sample_index
    return p


def camera_frames(t, cam, p, frames, hdr=False):
    """`frames` calls of one sample: the camera's jittered rays of frame F0 + k folded with N = 1 + k."""
    W, H = p.width, p.height
    b = Batch(t, orc.primary_rays(cam, W, H, frame=F0))
    for k in range(frames):
        if k:
            b.set_rays(orc.primary_rays(cam, W, H, frame=F0 + k))
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = F0 + k, 1 + k
        b.render(q, 1, hdr=hdr)
        t.sync()   # the next upload must not overtake the launch
    out = b.get().reshape(H, W, 3)
    b.free()
    return out


def scene_mesh_of(scene):
    return g.scene_mesh("cornell" if scene == "room" else scene)


# ---------------------------------------------------------------------------------------------------- 1: a camera's rays, its image
@pytest.mark.parametrize("size", [(64, 64), (37, 23)], ids=["64x64", "37x23"])
@pytest.mark.parametrize("scene", ["room", "cornell_box"])
def test_camera_rays_give_the_oracles_image(t, scene, size):
    """Three one-sample calls over the camera's rays of frames F0 .. F0 + 2 equal orc.render(spp = 3) bit for bit.  A pixel that
    differs is replayed with the brute-force closest hit and must hold its colour (the grazing cases of the wide walk); on these
    scenes none is expected, and the oracle's own walk agrees with brute force everywhere (checked here, on the CPU)."""
    W, H = size
    bvh, sph, mats, tm = setup_scene(t, scene, scene == "cornell_box")
    mesh = scene_mesh_of(scene)
    cam, p = golden_camera(W, H), params(W, H)
    mk = dict(materials=mats, tri_material=tm)
    ref, _, _ = orc.render(bvh, sph, cam, p, 3, want_rgba=False, **mk)
    pixels = [(x, y) for y in range(H) for x in range(W)]
    col, _, _ = orc.sample_pixels(pixels, sph, cam, p, 3, mesh=mesh, **mk)
    brute = orc.fold_samples(col, 1).reshape(H, W, 3)
    assert np.array_equal(bits(ref), bits(brute)), "the reference itself: the oracle's walk against brute force"
    got = camera_frames(t, cam, p, 3)
    diff = np.argwhere(np.any(bits(got) != bits(ref), axis=-1))
    print(f"{scene} {W}x{H}: {len(diff)} pixels differ from the oracle")
    for y, x in diff:
        assert np.array_equal(bits(got[y, x]), bits(brute[y, x])), f"pixel ({x},{y}): {got[y, x]} oracle {ref[y, x]} brute force {brute[y, x]}"
    assert len(diff) == 0


FLAG_SETS = [("default", "room", 0, g.MAT_DIFF, 1), ("metal-literal-w", "room", g.FLAG_METAL_LITERAL_W, g.MAT_METAL, 1),
             ("smallpt", "room", g.FLAGS_SMALLPT, g.MAT_REFR, 1), ("nee-table", "cornell_box", g.FLAG_COSINE_DIFF | g.FLAG_NEE, g.MAT_DIFF, 1),
             ("no-cull", "room", 0, g.MAT_SPEC, 0), ("nee-spheres", "room", g.FLAG_COSINE_DIFF | g.FLAG_NEE | g.FLAG_MISS_KEEPS_PATH, g.MAT_DIFF, 1)]


@pytest.mark.parametrize("name,scene,flags,tri_mat,cull", FLAG_SETS, ids=[f[0] for f in FLAG_SETS])
def test_camera_rays_give_pt_renders_image(t, name, scene, flags, tri_mat, cull):
    """The same three calls against pt_render(spp = 3) on the same context, for the estimator switches, both cull settings and
    the material table with next-event estimation (pt_render then runs the stage-split pipeline or the megakernel): bit for bit."""
    W, H = 37, 23
    setup_scene(t, scene, scene == "cornell_box")
    cam, p = golden_camera(W, H), params(W, H, tri_mat=tri_mat)
    p.flags, p.cull_backfaces = flags, cull
    acc, rgba = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 3)
    t.sync()
    ref = acc.download(np.float32, (H, W, 3))
    acc.free()
    rgba.free()
    got = camera_frames(t, cam, p, 3)
    assert ref.any()
    assert np.array_equal(bits(got), bits(ref)), f"{name}: {int(np.any(bits(got) != bits(ref), axis=-1).sum())} pixels differ"


# ---------------------------------------------------------------------------------------------------- 2: HDR
def hdr_fold(col, first_n=1, acc=None):
    """The running mean of PT_RAYS_HDR in numpy float32: a = (a * (N - 1) + col) * (1 / N), a = 0 in front of the sum when N == 1."""
    acc = np.zeros(col.shape[:-2] + (3,), np.float32) if acc is None else acc.astype(np.float32)
    for s in range(col.shape[-2]):
        N = first_n + s
        a = np.zeros_like(acc) if N == 1 else acc * np.float32(N - 1)
        acc = ((a + col[..., s, :]) * (np.float32(1.0) / np.float32(N))).astype(np.float32)
    return acc


def test_hdr_mode_is_the_unclamped_mean(t):
    W, H = 37, 23
    bvh, sph, _, _ = setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), params(W, H)
    pixels = [(x, y) for y in range(H) for x in range(W)]
    col, _, _ = orc.sample_pixels(pixels, sph, cam, p, 3, bvh=bvh)
    want = hdr_fold(col).reshape(H, W, 3)
    got = camera_frames(t, cam, p, 3, hdr=True)
    assert want.max() > 1.0, "no value above 1: the clamp would not have shown"
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got, camera_frames(t, cam, p, 3))


# ---------------------------------------------------------------------------------------------------- 3: splits
def test_samples_in_one_call_equal_one_call_each(t):
    W, H = 37, 23
    setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), params(W, H)
    rays = orc.primary_rays(cam, W, H, frame=F0)
    for hdr in (False, True):
        one, many = Batch(t, rays), Batch(t, rays)
        one.render(p, 4, hdr=hdr)
        for s in range(4):
            many.render(params(W, H, frame=F0 + s, sample_index=1 + s), 1, hdr=hdr)
        a, b = one.get(), many.get()
        assert a.any() and np.array_equal(bits(a), bits(b))
        one.free()
        many.free()


def test_many_samples_of_few_rays(t):
    """130 rays x 64 samples: every wave holds slots of several samples, a running mean continued from N = 3."""
    W, H = 37, 23
    setup_scene(t, "room", False)
    cam = golden_camera(W, H)
    rays = orc.primary_rays(cam, W, H, frame=F0)[300:430]
    init = np.random.default_rng(5).random((131, 3), dtype=np.float32)
    one, many = Batch(t, rays, init), Batch(t, rays, init)
    one.render(params(W, H, sample_index=3), 64, first_index=300)
    for s in range(64):
        many.render(params(W, H, frame=F0 + s, sample_index=3 + s), 1, first_index=300)
    a, b = one.get(), many.get()
    assert np.array_equal(bits(a), bits(b)) and len(np.unique(a, axis=0)) > 100
    one.free()
    many.free()


def test_a_batch_split_by_first_index(t):
    W, H = 37, 23
    setup_scene(t, "room", False)
    cam, p = golden_camera(W, H), params(W, H)
    rays = orc.primary_rays(cam, W, H, frame=F0)
    whole, parts = Batch(t, rays), Batch(t, rays)
    whole.render(p, 2)
    parts.render(p, 2, first_index=0, first=0, n=400)
    parts.render(p, 2, first_index=400, first=400, n=451)
    a, b = whole.get(), parts.get()
    assert a.any() and np.array_equal(bits(a), bits(b))
    whole.free()
    parts.free()


def test_first_index_beyond_32_bits(t):
    """Keys 2^32 + 5 + i: the pixels (i, 3) of a frame 1431655767 wide (3 x 1431655767 = 2^32 + 5), whose rays the oracle's camera
    function gives with the jitter of those keys; orc.sample_pixels renders exactly these pixels."""
    Wb, Hb, n = 1431655767, 4, 70
    bvh, sph, _, _ = setup_scene(t, "room", False)
    cam, p = golden_camera(64, 64), params(Wb, Hb)
    L = orc.lib()
    rays = np.zeros((n, 8), np.float32)
    for i in range(n):
        key = 3 * Wb + i
        u0, u1 = L.orc_rng_draw(F0, key, 0), L.orc_rng_draw(F0, key, 1)
        o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
        L.orc_camera_ray(C.byref(cam), i, 3, Wb, Hb, u0, u1, o.ctypes.data, d.ctypes.data)
        rays[i, 0:3], rays[i, 4:7] = o, d
    col, _, _ = orc.sample_pixels([(i, 3) for i in range(n)], sph, cam, p, 1, bvh=bvh)
    b = Batch(t, rays)
    b.render(p, 1, first_index=2 ** 32 + 5)
    got1 = b.get()
    assert np.array_equal(bits(got1), bits(orc.fold_samples(col, 1)))
    low = Batch(t, rays)
    low.render(p, 1, first_index=5)
    assert not np.array_equal(low.get(), got1), "the upper word of first_index is part of the key"
    low.free()
    b.free()


# ---------------------------------------------------------------------------------------------------- 3b: the schedule knobs
# include/ptmi.h: "PT_OPT_BATCH, PT_OPT_REFILL and PT_OPT_SPHERE_LDS apply: speed, never results".  k_render_rays carries its own copy
# of the persistent kernel's refill loop (ballot / mbcnt lane -> slot map, sharded chunk counter, refill <= batch clamp), so the copy
# is rendered at the same corners as tests/test_gpu_schedule_knobs.py renders the original (which also says why no setting can spin).
KNOB_SETTINGS = [((g.OPT_BATCH, b), (g.OPT_REFILL, r)) for b, r in ((1, 1), (1, 64), (64, 1), (64, 64), (36, 8), (2, 64))] + \
                [((g.OPT_SPHERE_LDS, 0),), ((g.OPT_SPHERE_LDS, 1),)]
POISON = 1000


FIXED_FRONTS = ((0.3, -0.4, -1.0), (-0.5, 0.2, -1.0), (0.0, -1.0, -0.9), (0.8, 0.1, -1.0), (-0.2, 0.7, -1.0), (0.1, -0.3, -1.0), (-0.9, -0.6, -1.0))


def fixed_ray_camera(W, H, front):
    """A camera with fov 0: every pixel's ray is pos + dist * front along front whatever the jitter, so ALL samples of orc.render
    start from the ray pt_render_rays is given once — its spp samples of one ray are then the oracle's samples of that pixel."""
    return make_camera(W, H, pos=(0.0, 0.0, 0.0), front=front, fov=0.0)


def knob_cases():
    """name -> (W, H, rays, calls, spp per call): the camera's rays of one frame, three one-sample calls (camera_frames: each
    frame's own jitter), and 7 rays x 512 samples in one call — few rays and many samples, so almost every slot of a wave is the
    same ray and the samples go through the sample buffer ([spp][n][3]) and the fold.  The seven rays are seven different
    ones, ray i that of a zero-fov camera looking along FIXED_FRONTS[i]: a slot that read another ray's origin or direction,
    or another ray's random stream, would show."""
    return {"129x71x3": (129, 71, 129 * 71, 3, 1), "7x512": (7, 2, 7, 1, 512)}


def knob_rays(name, k):
    """The rays of call k of the case."""
    W, H, n, calls, spp = knob_cases()[name]
    if name == "7x512":
        return np.stack([orc.primary_rays(fixed_ray_camera(W, H, f), W, H, frame=F0)[i] for i, f in enumerate(FIXED_FRONTS)])
    return orc.primary_rays(golden_camera(W, H), W, H, frame=F0 + k)[:n]


_knob_ref = {}


def knob_reference(name):
    """orc.render's accumulator for the case, one row per ray, once per run.  The 7-ray case: row i is pixel i (the random stream
    of key i, which first_index = 0 gives ray i) of the oracle's frame through camera i, after its premise is checked."""
    if name not in _knob_ref:
        W, H, n, calls, spp = knob_cases()[name]
        bvh, sph = g.Bvh(g.scene_mesh("cornell")), g.reference_spheres()
        if name == "7x512":
            ref = np.zeros((n, 3), np.float32)
            for i, f in enumerate(FIXED_FRONTS):
                cam = fixed_ray_camera(W, H, f)
                r0, r1 = orc.primary_rays(cam, W, H, frame=F0), orc.primary_rays(cam, W, H, frame=F0 + 5)
                assert np.isfinite(r0).all() and np.array_equal(bits(r0), bits(r1)) and len(np.unique(r0, axis=0)) == 1, "the ray depends on the jitter"
                ref[i] = orc.render(bvh, sph, cam, params(W, H), spp, want_rgba=False)[0][0, i]
            assert len(np.unique(knob_rays(name, 0)[:, 4:7], axis=0)) == n and len(np.unique(ref, axis=0)) == n
        else:
            ref = orc.render(bvh, sph, golden_camera(W, H), params(W, H), calls * spp, want_rgba=False)[0].reshape(-1, 3)[:n]
        _knob_ref[name] = ref
    return _knob_ref[name]


def knob_render(name, walk, options):
    """The case on a fresh context with `options`, behind a poison call: the same buffers rendered with other frame numbers
    first, so a slot that is never traced leaves a value of the wrong frame in the sample buffer or the output."""
    W, H, n, calls, spp = knob_cases()[name]
    tr = g.PathTracer(0)
    try:
        tr.set_option(g.OPT_WALK, walk)
        for o, v in options:
            tr.set_option(o, v)
        setup_scene(tr, "room", False)
        b = Batch(tr, knob_rays(name, 0))
        b.render(params(W, H, frame=F0 + POISON), spp)
        poison = b.get().copy()
        for k in range(calls):
            if k:
                tr.sync()   # the next upload must not overtake the launch
                b.set_rays(knob_rays(name, k))
            b.render(params(W, H, frame=F0 + k * spp, sample_index=1 + k * spp), spp)
        got = b.get()
        b.free()
        assert got.any() and not np.array_equal(got, poison), f"{name} walk {walk} {options}: empty, or the poison call's result"
        return got
    finally:
        tr.close()


@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("name", list(knob_cases()))
def test_schedule_knobs_change_no_radiance(name, walk):
    """PT_OPT_BATCH x PT_OPT_REFILL at the corners of their ranges (in (1, 64) and (2, 64) the clamp works) and PT_OPT_SPHERE_LDS
    0 / 1.  Walk 1 (the unified binary walk, exact): the radiance equals orc.render's accumulator bit for bit at every setting.
    Walk 2 (wide): it equals the default-knob result bit for bit, which may leave the oracle at no more than MAX_DIFF grazing rays."""
    ref = knob_reference(name)
    if walk == 2:
        base = knob_render(name, walk, ())
        n_off = int(np.any(bits(base) != bits(ref), axis=1).sum())
        print(f"{name}: the wide walk's default-knob result differs from the oracle at {n_off} rays")
        assert n_off <= MAX_DIFF
        ref = base
    for options in KNOB_SETTINGS:
        got = knob_render(name, walk, options)
        bad = np.nonzero(np.any(bits(got) != bits(ref), axis=1))[0]
        assert len(bad) == 0, f"{name} walk {walk} {options}: {len(bad)} rays differ, first {bad[:6]}"


# ---------------------------------------------------------------------------------------------------- 4: rays no camera makes
def first_hit_radiance(bvh, sph, rays, p, tri_emi=None):
    """depth 1 under the default flags: the emission of the first hit — the nearest triangle (oracle walk), or a sphere at
    t > 0.01 closer than it — or bk_color."""
    t_tri, tri, _, _ = orc.trace_bvh(bvh, rays, cull=bool(p.cull_backfaces))
    o, d = rays[:, 0:3].copy(), rays[:, 4:7].copy()
    out = np.tile(np.array(list(p.bk_color), np.float32), (len(rays), 1))
    out[tri >= 0] = np.array(list(p.tri_emi), np.float32) if tri_emi is None else tri_emi[tri[tri >= 0]]
    best = t_tri.copy()
    for s in sph or []:
        ts = sphere_intersect(s, o, d)
        m = (ts != 0) & (ts < best) & (ts > np.float32(0.01))
        best[m] = ts[m]
        out[m] = np.array(list(s.emi), np.float32)
    return out, tri


def test_incoherent_rays_at_depth_one(t):
    bvh, sph, _, _ = setup_scene(t, "room", False)
    v = np.asarray(scene_mesh_of("room").verts, np.float32)
    rays = orc.random_rays(2000, v.min(0), v.max(0))
    p = params(64, 64, depth=1)
    p.tri_emi[:] = (0.25, 0.5, 2.0)
    p.bk_color[:] = (0.125, 0.75, 0.375)
    want, tri = first_hit_radiance(bvh, sph, rays, p)
    b = Batch(t, rays)
    b.render(p, 1, hdr=True)
    got = b.get()
    b.free()
    assert (tri >= 0).sum() > 100 and len(np.unique(want, axis=0)) >= 4
    assert np.array_equal(bits(got), bits(want)), f"{int(np.any(got != want, axis=1).sum())} rays differ"


# ---------------------------------------------------------------------------------------------------- 5: bad rays
def test_bad_rays_end_as_misses(t):
    W, H = 37, 23
    setup_scene(t, "room", False)
    cam = golden_camera(W, H)
    good = orc.primary_rays(cam, W, H, frame=F0)[100:300]
    bad = np.repeat(good[:1], 8, axis=0)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad[0, 4] = nan
    bad[1, 6] = inf
    bad[2, 5] = -inf
    bad[3, 4:7] = 0.0
    bad[4, 4:7] = (-0.0, 0.0, -0.0)
    bad[5, 0] = nan
    bad[6, 2] = inf
    bad[7, 0:3], bad[7, 4:7] = nan, nan
    at = [0, 13, 64, 65, 127, 128, 199, 200]   # where the bad rays go: positions in the spliced batch
    rays = np.zeros((208, 8), np.float32)
    is_bad = np.zeros(208, bool)
    is_bad[at] = True
    rays[is_bad], rays[~is_bad] = bad, good
    for flags in (0, g.FLAG_MISS_KEEPS_PATH):
        p = params(W, H)
        p.flags = flags
        p.bk_color[:] = (0.125, 0.75, 0.375)
        spliced, plain = Batch(t, rays), Batch(t, good)
        spliced.render(p, 2)
        # the keys of the good rays in the spliced batch, one call per run between two bad rays
        keys = np.nonzero(~is_bad)[0]
        for k0 in np.nonzero(np.diff(np.concatenate(([-2], keys))) != 1)[0]:
            k1 = k0
            while k1 + 1 < len(keys) and keys[k1 + 1] == keys[k1] + 1:
                k1 += 1
            plain.render(p, 2, first_index=int(keys[k0]), first=int(k0), n=int(k1 - k0 + 1))
        a, b = spliced.get(), plain.get()
        assert np.array_equal(bits(a[~is_bad]), bits(b))
        assert np.array_equal(a[is_bad], np.tile(np.array([0.125, 0.75, 0.375], np.float32), (8, 1)))
        spliced.free()
        plain.free()


# ---------------------------------------------------------------------------------------------------- 6: errors, nothing written
def test_errors_in_order_and_nothing_written(t):
    W, H = 37, 23
    lib, p = g._abi.ptmi(), params(W, H)
    empty = g.PathTracer(0)
    try:
        assert lib.pt_render_rays(empty._ctx, None, 4, 0, None, None, 1, 9) == -3        # no scene comes before every argument check
    finally:
        empty.close()
    setup_scene(t, "room", False)
    rays = orc.primary_rays(golden_camera(W, H), W, H, frame=F0)[:64]
    b = Batch(t, rays)
    canary = b.get().copy()
    call = lambda r, n, o, pp, spp, mode: lib.pt_render_rays(t._ctx, r, n, 0, o, pp, spp, mode)
    assert call(None, 0, None, None, 1, 9) == 0 and call(None, 4, None, None, 0, 9) == 0   # nothing to do comes before the pointers
    assert call(b.rays.ptr, 0, b.out.ptr, C.byref(p), 1, 0) == 0 and call(b.rays.ptr, 64, b.out.ptr, C.byref(p), 0, 0) == 0
    assert np.array_equal(b.get(), canary)
    assert call(None, 4, b.out.ptr, C.byref(p), 1, 9) == -1 and call(b.rays.ptr, 4, None, C.byref(p), 1, 9) == -1
    assert call(b.rays.ptr, 4, b.out.ptr, None, 1, 9) == -1
    assert call(b.rays.ptr, 4, b.out.ptr, C.byref(p), 1, 2) == -1 and "mode" in lib.pt_last_error(t._ctx).decode()
    assert call(b.rays.ptr, 2 ** 32, b.out.ptr, C.byref(p), 1, 0) == -1 and "2^32" in lib.pt_last_error(t._ctx).decode()
    assert np.array_equal(b.get(), canary)
    # depth 0: black samples, folded as pt_render folds them
    p0 = params(W, H, depth=0, sample_index=2)
    b.out.upload(np.full((65, 3), 0.5, np.float32))
    b.render(p0, 1)
    got = b.get()
    assert np.array_equal(got[:64], np.full((64, 3), 0.25, np.float32))
    b.free()


# ---------------------------------------------------------------------------------------------------- 7: ordering, side effects
def test_render_rays_after_refit_sees_the_moved_triangles():
    """A device-built tree over the Cornell box, twisted by pt_refit_bvh: depth-1 radiance by the per-triangle material table's
    emission, compared over the refit vertices."""
    mesh = g.scene_mesh("cornell_box")
    soup = mesh.triangle_soup()
    moved = twist(soup, 0.6, (0.05, 0.0, -0.03))
    n = len(soup)
    tab = [g.Material() for _ in range(n)]
    emi = np.random.default_rng(9).random((n, 3), dtype=np.float32)
    for i, m in enumerate(tab):
        m.col[:], m.emi[:], m.mat = (0.5, 0.5, 0.5), emi[i], g.MAT_DIFF
    tr = g.PathTracer(0)
    try:
        tr.build_bvh(soup_mesh(soup))
        tr.upload_spheres(None)
        tr.upload_tri_materials(tab, np.arange(n, dtype=np.int32))
        v = moved.reshape(-1, 3)
        rays = orc.random_rays(1500, v.min(0), v.max(0), seed=77)
        p = params(64, 64, depth=1)
        p.bk_color[:] = (0.125, 0.75, 0.375)
        b = Batch(tr, rays)
        b.render(p, 1, hdr=True)
        before = b.get().copy()
        tr.refit_bvh(moved)
        b.render(p, 1, hdr=True)   # no sync in between: ordered on the stream
        got = b.get()
        b.free()
    finally:
        tr.close()
    t_m, tri_m, _ = orc.trace_brute(soup_mesh(moved), rays, cull=True)
    want = np.tile(np.array([0.125, 0.75, 0.375], np.float32), (len(rays), 1))
    want[tri_m >= 0] = emi[tri_m[tri_m >= 0]]
    assert (tri_m >= 0).sum() > 100 and not np.array_equal(before, got)
    assert np.array_equal(bits(got), bits(want)), f"{int(np.any(got != want, axis=1).sum())} rays differ"


def test_render_rays_leaves_no_trace_in_render(t):
    W, H = 129, 67
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
    b = Batch(t, orc.primary_rays(cam, W, H, frame=3))
    acc, rg = t.alloc_frame(W, H)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 3)
    b.render(p, 5, hdr=True)
    t.launch_kernel(acc.ptr, rg.ptr, cam, p, 3)
    t.sync()
    between = acc.download(np.float32, (H, W, 3))
    assert b.get().any()
    b.free()
    acc.free()
    rg.free()
    after = frame(t)
    clean = g.PathTracer(0)
    try:
        clean.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
        clean.upload_bvh(bvh)
        clean.upload_spheres(sph)
        c = frame(clean)
    finally:
        clean.close()
    for a in (before, after):
        assert np.array_equal(bits(a[0]), bits(c[0])) and np.array_equal(a[1], c[1])
    assert np.array_equal(bits(between), bits(c[0]))


def test_render_rays_timing(t):
    W, H = 129, 67
    setup_scene(t, "room", False)
    b = Batch(t, orc.primary_rays(golden_camera(W, H), W, H, frame=F0))
    t.set_option(g.OPT_TIMING, 1)
    try:
        b.render(params(W, H), 4)
        assert 0 < t.last_kernel_ms() < 50
    finally:
        t.set_option(g.OPT_TIMING, 0)
        b.free()


# ---------------------------------------------------------------------------------------------------- 8: pt_app --equirect
def test_pt_app_equirect(tmp_path):
    """160x80, 2 samples: a PNG and a PFM are written; the PNG differs from the pinhole frame; the PFM's centre pixel is the HDR
    radiance of the one ray along `front` with that pixel's key and the app's frame numbers (0, 1)."""
    W, H = 160, 80
    base = [APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", str(W), "--height", str(H), "--frames", "2"]
    png, pfm, pin = tmp_path / "e.png", tmp_path / "e.pfm", tmp_path / "p.png"
    for extra in (["--equirect", "--out", str(png)], ["--equirect", "--out", str(pfm)], ["--out", str(pin)]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
    assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and png.read_bytes() != pin.read_bytes()
    raw = pfm.read_bytes()
    assert raw[:2] == b"PF"
    img = np.frombuffer(raw[-W * H * 12:], "<f4").reshape(H, W, 3)
    tr = g.PathTracer(0)
    try:
        tr.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        tr.upload_spheres(g.reference_spheres())
        ray = np.zeros((1, 8), np.float32)
        ray[0, 4:7] = (0.0, 0.0, -1.0)   # the app's camera: at the origin, front = -z
        b = Batch(tr, ray)
        p = g.default_params(W, H)   # the app's parameters are the package's defaults
        p.frame, p.sample_index = 0, 1
        b.render(p, 2, first_index=(H // 2) * W + W // 2, hdr=True)
        want = b.get()[0]
        b.free()
    finally:
        tr.close()
    rows = [img[H // 2, W // 2], img[H - 1 - H // 2, W // 2]]   # (whichever way the writer orders the rows)
    assert any(np.array_equal(bits(r), bits(want)) for r in rows), (rows, want)


# ---------------------------------------------------------------------------------------------------- 9: deep trees
DEEP_BK = (0.125, 0.75, 0.375)
_deep = {}


def deep_case(name):
    """(fixture, its 128 half-cell rays, the radiance every ray must return at depth 1 under tilted_grid_table) of a tree of
    tests/deep_trees.py: the emission of the triangle deep_trees.expected_ids names, which brute force confirms, or DEEP_BK."""
    if name not in _deep:
        kind, n = name.split("-")
        fx = dt.stair(int(n)) if kind == "stair" else dt.comb(int(n))
        rays = dt.cell_rays(fx)
        ids = dt.expected_ids(fx, rays)
        assert np.array_equal(orc.trace_brute(fx.mesh, rays, True)[1], ids) and 16 < (ids >= 0).sum() < 128
        want = np.tile(np.array(DEEP_BK, np.float32), (len(rays), 1))
        want[ids >= 0] = np.stack([(ids[ids >= 0] + 1) / 256.0, np.full((ids >= 0).sum(), 0.5), np.full((ids >= 0).sum(), 0.25)], 1)
        _deep[name] = fx, rays, ids, want
    return _deep[name]


def deep_context(fx, woop=False):
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_TRI_TEST, int(woop))
    tr.upload_bvh(fx)
    tr.upload_spheres(None)
    tr.upload_tri_materials(*tilted_grid_table(fx.n_tris))
    return tr


def deep_params():
    p = params(64, 64, depth=1)
    p.bk_color[:] = DEEP_BK
    return p


# stair(23): 3 * 23 + 2 = 71 entries, the last tree the wide walk takes; stair(24): 74 > 72, the unified binary walk takes over;
# comb(17): stack depth 17, the first overflow of the 16-entry LDS window this call always uses
DEEP_TREES = {"stair-23": (24, 23), "stair-24": (25, 24), "comb-17": (17, 6)}   # name -> (max_depth, wide depth)


@pytest.mark.parametrize("name", list(DEEP_TREES))
def test_deep_trees_under_every_walk(name):
    """pt_render_rays over the trees on both sides of the wide walk's stack rule and past the LDS window, under the default walk and
    PT_OPT_WALK 0, 1 (both run the unified binary walk here) and 4 (runs as 2): depth 1, every triangle emitting its id, so a ray's
    radiance names the triangle it hit.  Equal to the brute-force answer bit for bit."""
    fx, rays, ids, want = deep_case(name)
    assert (fx.max_depth, fx.wide_depth) == DEEP_TREES[name]
    if name == "comb-17":
        depth = dt.binary_stack_depth(fx, rays)
        assert depth.min() == depth.max() == 17
    tr = deep_context(fx)
    try:
        assert tr.scene_info()["max_depth"] == fx.max_depth and tr.tree_items()[3] == fx.wide_depth
        for walk in (2, 0, 1, 4):
            tr.set_option(g.OPT_WALK, walk)
            for hdr in (True, False):
                b = Batch(tr, rays)
                b.render(deep_params(), 1, hdr=hdr)
                got = b.get()
                b.free()
                bad = np.nonzero(np.any(bits(got) != bits(want), axis=1))[0]
                assert len(bad) == 0, f"{name} walk {walk} hdr {hdr}: rays {bad[:8]} return {got[bad[:4]]}, brute force {want[bad[:4]]}"
    finally:
        tr.close()


def test_deep_trees_with_woop_records():
    """Woop records (PT_OPT_TRI_TEST 1 before the upload) are read by the wide walk only.  stair(24) is too deep for it: the call
    answers PT_ERR_UNSUPPORTED, names itself in the message and writes nothing.  stair(23) renders: which triangle a ray hits, or
    that it hits none, equals brute force for every ray (Woop's t differs in its last bits; the ids, and with them the emission
    returned at depth 1, do not)."""
    lib = g._abi.ptmi()
    fx, rays, ids, want = deep_case("stair-24")
    tr = deep_context(fx, woop=True)
    try:
        assert tr.tree_items()[3] == 24
        b, p = Batch(tr, rays), deep_params()
        canary = b.get().copy()
        for walk in (2, 1):
            tr.set_option(g.OPT_WALK, walk)
            assert lib.pt_render_rays(tr._ctx, b.rays.ptr, b.n, 0, b.out.ptr, C.byref(p), 1, 0) == -5
            msg = lib.pt_last_error(tr._ctx).decode()
            assert msg.startswith("pt_render_rays:") and "Woop" in msg, msg
        assert np.array_equal(b.get(), canary)
        b.free()
    finally:
        tr.close()
    fx, rays, ids, want = deep_case("stair-23")
    tr = deep_context(fx, woop=True)
    try:
        assert tr.tree_items()[3] == 23
        for walk in (2, 1):     # (the option does not choose the walk of Woop records)
            tr.set_option(g.OPT_WALK, walk)
            b = Batch(tr, rays)
            b.render(deep_params(), 1, hdr=True)
            got = b.get()
            b.free()
            hit = np.any(bits(got) != bits(np.array(DEEP_BK, np.float32)), axis=1)
            assert np.array_equal(hit, ids >= 0), f"walk {walk}: hit / miss differs for rays {np.nonzero(hit != (ids >= 0))[0][:8]}"
            assert np.array_equal(bits(got), bits(want)), f"walk {walk}: rays {np.nonzero(np.any(got != want, axis=1))[0][:8]} name another triangle"
    finally:
        tr.close()
