"""PT_FLAG_MIS on the device (contract in include/ptmi.h "Multiple importance sampling").

References, none of them the code under test: closed-form radiance (tests/estimator_ref.py, tests/env_light_ref.py), the float64
restatement of the estimator (tests/mis_ref.py, held against geometry on the CPU by tests/test_mis.py), the same call without the
flag (same expectation; the same bits where no bounce ray follows), and the renderer itself (pt_render against pt_render_rays).
Measured on an MI355X: profiles/r17_mis.txt."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_light_ref
import estimator_ref as ref
import mis_ref
import orc
from gpu_support import bits, golden_camera, gpu_trace, is_frame_kernel

pytestmark = pytest.mark.gpu
NEE, MIS = ref.NEE, mis_ref.MIS
KERNELS = {"mega": g.KERNEL_MEGA_BVH2, "persistent": g.KERNEL_PERSISTENT, "wavefront": g.KERNEL_WAVEFRONT}
INVALID, NO_SCENE, UNSUPPORTED = -1, -3, -5


def on_device(t, arr):
    b = t.malloc(max(arr.nbytes, 32))
    b.upload(np.ascontiguousarray(arr))
    return b


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


def render_frame(t, cam, p, spp, moments=False):
    """one pt_render (or pt_render_moments) call into a fresh accumulator"""
    acc, rgba = t.alloc_frame(p.width, p.height)
    mom = t.malloc(8 * p.width * p.height) if moments else None
    t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp, moments_ptr=mom.ptr if moments else None)
    t.sync()
    out = acc.download(np.float32, (p.height, p.width, 3))
    for b in (acc, rgba) + ((mom,) if moments else ()):
        b.free()
    return out


def with_flags(p, flags, **fields):
    q = g.Params.from_buffer_copy(p)
    q.flags = flags
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def context(case, timing=True):
    t = g.PathTracer(0)
    if timing:
        t.set_option(g.OPT_TIMING, 1)
    t.upload_bvh(g.Bvh(case.mesh))
    t.upload_spheres(case.spheres())
    if case.materials is not None:
        t.upload_tri_materials(case.materials, case.tri_material)
    return t


# ---------------------------------------------------------------------------------------------------- 1: closed forms, every route
CASES = mis_ref.cases()
SPP, SIDE = 64, 64


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_route_holds_the_closed_form(case):
    """The four routes of test_gpu_estimators at 2^18 samples: |mean - E| <= 5 SE (a dark case exactly 0), SE <= 0.02 E, nothing
    reaches 1, every pt_render route ran the frame kernel — and on A, A2, B, BA the standard error is at most 1.25 x the
    restatement's at the same sample count (the 1.25: the sampling noise of a standard error at 2^18 samples, binary32 against
    float64)."""
    n = SIDE * SIDE * SPP
    held = case.name.rsplit("-", 1)[0]
    se_ref = mis_ref.standard_error(held, 18) if held in mis_ref.SCENES else None
    failures = []
    t = context(case)
    try:
        for route in ("rays",) + tuple(KERNELS):
            if route == "rays":
                rays = np.ascontiguousarray(np.tile(case.ray(), (n, 1)))
                x, framed = render_rays(t, rays, case.params(SIDE, SIDE)), True
            else:
                t.set_option(g.OPT_KERNEL, KERNELS[route])
                x = render_frame(t, case.camera(SIDE, SIDE), case.params(SIDE, SIDE), SPP).reshape(-1, 3)
                framed = is_frame_kernel(t.stage_ms())
            problems, z, rel = ref.verdict(case, x)
            print(f"MIS {case.name:24s} {route:10s} {case.kind:5s} z {z[0]:+7.2f} {z[1]:+7.2f} {z[2]:+7.2f}  "
                  f"SE/E {rel[0]:.5f} {rel[1]:.5f} {rel[2]:.5f}  max {x.max():.4f}")
            if not framed:
                problems.append("did not run the frame kernel")
            if case.kind == "mc" and not (rel <= 0.02).all():
                problems.append(f"SE / E {rel} above 0.02")
            if not x.max() < 1.0:
                problems.append(f"a sample or pixel reached {x.max()}")
            if se_ref is not None:
                se = ref.mean_and_se(x)[1]
                print(f"MIS {case.name:24s} {route:10s} SE {se}  restatement {se_ref}  ratio {se / se_ref}")
                if not (se <= 1.25 * se_ref).all():
                    problems.append(f"SE {se} above 1.25 x the restatement's {se_ref}")
            failures += [f"{route}: {p}" for p in problems]
    finally:
        t.close()
    assert not failures, (case.name, failures)


# ---------------------------------------------------------------------------------------------------- 2: the two wins
N_WIN = 1 << 16


def three_estimators(t, case):
    """{estimator: (mean, SE)} of 2^16 identical rays from mis_ref.S_ORIGIN, one sample each, depth 2"""
    rays = mis_ref.s_rays(N_WIN)
    out = {}
    for name, flags in (("plain", ref.BASE), ("nee", NEE), ("mis", MIS)):
        out[name] = ref.mean_and_se(render_rays(t, rays, with_flags(case.params(64, 64), flags)))
        print(f"{case.name:7s} {name:5s} mean {out[name][0]} SE {out[name][1]} z {(out[name][0] - case.E) / out[name][1]}")
    return out


def restated(scene):
    est = mis_ref.estimate(scene, 16)
    return {k: ref.mean_and_se(v)[1] for k, v in est.items()}


def test_s_near_mis_beats_the_area_sampler():
    mesh, table, rows = mis_ref.near_mesh()
    case = ref.Case("S-near", mis_ref.near_E(), depth=2, mesh=mesh, materials=table, tri_material=rows)
    t = context(case, timing=False)
    try:
        st = three_estimators(t, case)
    finally:
        t.close()
    want = restated(mis_ref.near_scene())
    print(f"S-near SE_mis / SE_nee: device {st['mis'][1] / st['nee'][1]}, restatement {want['mis'] / want['nee']}")
    for k, (m, se) in st.items():
        assert (np.abs(m - case.E) <= 5 * se).all(), k
    assert (st["mis"][1] <= 0.5 * st["nee"][1]).all()


@pytest.fixture(scope="module")
def plane():
    """the ground quad alone: the scene of test_a_small_sun_over_a_diffuse_plane"""
    t = g.PathTracer(0)
    t.upload_bvh(g.Bvh(ref.ground_with()))
    yield t
    t.close()


def test_s_sun_mis_beats_the_bounce(plane):
    case = ref.Case("S-sun", mis_ref.sun_E(), depth=2)
    plane.upload_environment(mis_ref.sun_texels(), filter=g.ENV_NEAREST, light=True)
    assert plane.environment_is_light()
    st = three_estimators(plane, case)
    plane.clear_environment()
    want = restated(mis_ref.sun_scene())
    print(f"S-sun SE_mis / SE_bounce: device {st['mis'][1] / st['plain'][1]}, restatement {want['mis'] / want['plain']}")
    for k, (m, se) in st.items():
        assert (np.abs(m - case.E) <= 5 * se).all(), k
    assert (st["mis"][1] <= 0.5 * st["plain"][1]).all()


def test_s_sky_holds_the_closed_form_and_the_restatements_noise(plane):
    case = ref.Case("S-sky", mis_ref.sun_E(sky=True), depth=2)
    plane.upload_environment(mis_ref.sun_texels(sky=True), filter=g.ENV_NEAREST, light=True)
    st = three_estimators(plane, case)
    plane.clear_environment()
    want = restated(mis_ref.sun_scene(sky=True))
    print(f"S-sky SE device {[st[k][1][0] for k in ('plain', 'nee', 'mis')]}, restatement {[want[k][0] for k in ('plain', 'nee', 'mis')]}")
    for k, (m, se) in st.items():
        assert (np.abs(m - case.E) <= 5 * se).all(), k
    assert (st["mis"][1] <= 1.25 * want["mis"]).all()


# ---------------------------------------------------------------------------------------------------- 3: depth 1 is plain NEE
def box_params(w, h, depth, flags, frame=5):
    p = g.default_params(w, h, depth=depth)
    p.flags, p.frame = flags, frame
    return p


def rays_frame(t, cam, p, spp):
    """pt_render_rays over the camera's own jittered rays, sample by sample, clamped: what pt_render folds"""
    w, h = p.width, p.height
    out = t.malloc(12 * w * h)
    for k in range(spp):
        q = with_flags(p, p.flags, frame=p.frame + k, sample_index=1 + k)
        got = render_rays(t, orc.primary_rays(cam, w, h, frame=p.frame + k), q, hdr=False, out=out)
    out.free()
    return got.reshape(h, w, 3)


def both_ways(t, cam, p_nee, p_mis, spp, what):
    t.set_option(g.OPT_KERNEL, g.KERNEL_MEGA_BVH2)   # the same kernel family for both flags: this is about the estimator
    a, b = render_frame(t, cam, p_nee, spp), render_frame(t, cam, p_mis, spp)
    assert a.any() and np.array_equal(bits(a), bits(b)), f"{what}, pt_render: {int(np.any(bits(a) != bits(b), axis=-1).sum())} pixels differ"
    c, d = rays_frame(t, cam, p_nee, spp), rays_frame(t, cam, p_mis, spp)
    assert c.any() and np.array_equal(bits(c), bits(d)), f"{what}, pt_render_rays: {int(np.any(bits(c) != bits(d), axis=-1).sum())} rays differ"


def test_depth_one_is_plain_nee():
    w = h = 32
    cam = golden_camera(w, h)
    t = g.PathTracer(0)
    try:
        mesh = g.scene_mesh("cornell_box")
        t.upload_bvh(g.Bvh(mesh))
        t.upload_spheres(g.reference_spheres())
        t.upload_tri_materials(mesh.materials, mesh.tri_material)
        both_ways(t, cam, box_params(w, h, 1, NEE), box_params(w, h, 1, MIS), 4, "cornell_box, depth 1")
        # no pickable light at all: the path is inside the one emitting sphere, no material table — estimator_ref's closed room
        # (case E).  Not the reference room: its glowing walls are spheres of radius 600 centred 615 and more from the room's middle,
        # so a path is OUTSIDE every wall but the one it stands on, and picks them.
        room = next(c for c in ref.cases() if c.name == "E-plain-depth3")
        t.upload_bvh(g.Bvh(room.mesh))
        t.upload_spheres(room.spheres())
        t.upload_tri_materials(None, None)
        p_nee, p_mis = with_flags(room.params(w, h), NEE, depth=4), with_flags(room.params(w, h), MIS, depth=4)
        both_ways(t, golden_camera(w, h), p_nee, p_mis, 4, "inside the only emitter, depth 4")
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------- 4, 5: every kind of light at once
W, H = 37, 23
ALBEDO = (0.5, 0.6, 0.7)


def bunny_camera(w=W, h=H):
    cam = golden_camera(w, h)
    cam.pos[:] = (-1.0, 5.0, 11.0)
    return cam


def bunny_params(w, h, flags, depth=4, frame=5):
    p = g.default_params(w, h, depth=depth)
    p.tri_col[:], p.tri_emi[:], p.bk_color[:] = ALBEDO, (0, 0, 0), (0.25, 0.5, 0.75)
    p.flags, p.frame = flags, frame
    return p


@pytest.fixture(scope="module")
def bunny():
    """bunny_low on the ground quad under the 8 x 4 bilinear map as a light, an emissive sphere beside the mesh, a mirror sphere on
    its other side, and a material table whose one emissive triangle hangs above it, facing down."""
    mesh = g.scene_mesh("bunny_low")
    lo, hi = (np.asarray(v, np.float64) for v in mesh.bounds())
    mid = (lo + hi) / 2.0
    n_bunny = mesh.n_tris
    half = 50.0
    gv = np.array([[-half, lo[1], -half], [half, lo[1], -half], [half, lo[1], half], [-half, lo[1], half]], np.float32)
    mesh.append(g.Mesh.from_arrays(gv, np.array([[0, 2, 1], [0, 3, 2]], np.int32)))
    y = hi[1] + 3.0
    lamp = np.array([[mid[0] - 1.0, y, mid[2] - 1.0], [mid[0] + 1.0, y, mid[2] - 1.0], [mid[0], y, mid[2] + 1.0]], np.float32)
    mesh.append(g.Mesh.from_arrays(lamp, np.array([[0, 1, 2]], np.int32)))
    rows = np.zeros(mesh.n_tris, np.int32)
    rows[-1] = 1
    table = [ref.row(ALBEDO), ref.row(ref.BLACK, emi=(6.0, 5.0, 4.0))]
    spheres = ref.sphere_array([ref.light((hi[0] + 3.0, hi[1] + 2.0, mid[2]), 1.0, (4.0, 3.0, 2.0)),
                                ((float(lo[0] - 3.0), float(lo[1] + 1.5), float(mid[2]), 1.5), ref.BLACK, (0.9, 0.9, 0.9), g.MAT_SPEC)])
    tr = g.PathTracer(0)
    tr.build_bvh(mesh)
    tr.upload_spheres(spheres)
    tr.upload_tri_materials(table, rows)
    tr.upload_environment(env_light_ref.hot_map(8, 4, 3, 2, value=20.0, ambient=0.2), filter=g.ENV_BILINEAR, light=True)
    assert tr.environment_is_light()
    yield tr, n_bunny, mid
    tr.close()


def test_the_megakernel_and_the_rays_kernel_agree(bunny):
    t = bunny[0]
    w = h = 32
    cam, p = bunny_camera(w, h), bunny_params(w, h, MIS)
    image = render_frame(t, cam, p, 4)
    got = rays_frame(t, cam, p, 4)
    plain = render_frame(t, cam, bunny_params(w, h, NEE), 4)
    assert np.array_equal(bits(got), bits(image)), f"{int(np.any(bits(got) != bits(image), axis=-1).sum())} pixels differ"
    assert np.isfinite(image).all() and np.any(bits(plain) != bits(image)), "the flag changed nothing"


def test_long_paths_keep_the_expectation(bunny):
    t, n_bunny, centre = bunny
    rays = orc.primary_rays(bunny_camera(), W, H, jitter=False)
    dist, tri, _ = gpu_trace(t, rays)
    on_mesh = np.flatnonzero((tri >= 0) & (tri < n_bunny))
    on_ground = np.flatnonzero((tri >= n_bunny) & (tri < n_bunny + 2))
    assert len(on_mesh) >= 8 and len(on_ground) >= 8
    hit = rays[on_ground, 0:3] + dist[on_ground, None] * rays[on_ground, 4:7]
    near = on_ground[np.argsort(np.hypot(hit[:, 0] - centre[0], hit[:, 2] - centre[2]))[:8]]
    pick = np.concatenate([on_mesh[np.linspace(0, len(on_mesh) - 1, 8).astype(int)], near])
    per = 1 << 14
    batch = np.repeat(rays[pick], per, axis=0)
    stats = {}
    for name, flags in (("nee", NEE), ("mis", MIS)):
        got = render_rays(t, batch, bunny_params(W, H, flags)).reshape(16, per, 3).astype(np.float64)
        stats[name] = got.mean(axis=1), got.std(axis=1, ddof=1) / np.sqrt(per)
    (m1, se1), (m0, se0) = stats["mis"], stats["nee"]
    z = (m1 - m0) / np.sqrt(se1 ** 2 + se0 ** 2)
    print(f"means (mis) {m1[:, 0]}\nmeans (nee) {m0[:, 0]}\nlargest |difference| in combined standard errors: {np.abs(z).max():.2f}; "
          f"SE_mis / SE_nee per pixel {(se1 / se0)[:, 0]}")
    assert (m1 > 0).all() and (m0 > 0).all() and (np.abs(z) <= 5).all()


# ---------------------------------------------------------------------------------------------------- 6: call rules
@pytest.fixture(scope="module")
def box():
    """cornell_box with its emissive material table and the default spheres; PT_OPT_TIMING on"""
    t = g.PathTracer(0)
    t.set_option(g.OPT_TIMING, 1)
    mesh = g.scene_mesh("cornell_box")
    t.upload_bvh(g.Bvh(mesh))
    t.upload_spheres(g.reference_spheres())
    t.upload_tri_materials(mesh.materials, mesh.tri_material)
    yield t
    t.close()


def test_every_kernel_option_runs_the_frame_kernel(box):
    w = h = 32
    cam, p = golden_camera(w, h), box_params(w, h, 4, MIS)
    frames = {}
    for name, k in (("auto", g.KERNEL_AUTO),) + tuple(KERNELS.items()):
        box.set_option(g.OPT_KERNEL, k)
        frames[name] = render_frame(box, cam, p, 4)
        assert is_frame_kernel(box.stage_ms()), (name, box.stage_ms())
    for name, f in frames.items():
        assert f.any() and np.array_equal(bits(f), bits(frames["mega"])), name
    assert np.any(bits(frames["mega"]) != bits(render_frame(box, cam, box_params(w, h, 4, NEE), 4))), "the flag changed nothing"


def test_flagged_calls_leave_the_auto_table_alone(box):
    w = h = 32
    cam, plain, flagged = golden_camera(w, h), box_params(w, h, 4, 0), box_params(w, h, 4, MIS)
    box.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    for _ in range(5):
        render_frame(box, cam, plain, 4)
    before = box.auto_choice()
    assert before[0] in (g.KERNEL_PERSISTENT, g.KERNEL_WAVEFRONT)
    for _ in range(2):
        render_frame(box, cam, flagged, 4)
        assert box.auto_choice() == before
    render_frame(box, cam, plain, 4)
    assert box.auto_choice() == before


def test_moments_samples_and_stripes(box):
    w = h = 32
    cam, p = golden_camera(w, h), box_params(w, h, 4, MIS)
    box.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    whole = render_frame(box, cam, p, 8)
    assert np.array_equal(bits(render_frame(box, cam, p, 8, moments=True)), bits(whole)), "pt_render_moments wrote another accumulator"
    acc, rgba = box.alloc_frame(w, h)
    box.launch_kernel(acc.ptr, rgba.ptr, cam, p, 3)
    box.launch_kernel(acc.ptr, rgba.ptr, cam, with_flags(p, MIS, frame=p.frame + 3, sample_index=4), 5)
    box.sync()
    assert np.array_equal(bits(acc.download(np.float32, (h, w, 3))), bits(whole)), "3 + 5 samples differ from 8"
    acc.zero()
    for part in range(3):
        box.launch_kernel(acc.ptr, rgba.ptr, cam, with_flags(p, MIS, part_index=part, part_count=3, part_rows=8), 8)
    box.sync()
    assert np.array_equal(bits(acc.download(np.float32, (h, w, 3))), bits(whole)), "three stripes differ from the full frame"
    acc.free()
    rgba.free()


# ---------------------------------------------------------------------------------------------------- 7: errors
def raw_calls(t, cam, p, acc, rgba, mom, rays, out, n):
    """the status of the three entry points for one pt_params"""
    lib, ctx = t._lib, t._ctx
    return (lib.pt_render(ctx, acc.ptr, rgba.ptr, C.byref(cam), C.byref(p), 1),
            lib.pt_render_moments(ctx, acc.ptr, rgba.ptr, mom.ptr, C.byref(cam), C.byref(p), 1),
            lib.pt_render_rays(ctx, rays.ptr, n, 0, out.ptr, C.byref(p), 1, g._abi.RAYS_HDR))


def test_errors(box):
    w = h = 32
    cam = golden_camera(w, h)
    host_rays = orc.primary_rays(cam, w, h, jitter=False)
    n = len(host_rays)
    no_nee = box_params(w, h, 4, ref.BASE | g.FLAG_MIS)
    bare = box_params(w, h, 4, g.FLAG_MIS)
    # a context without a scene: PT_FLAG_MIS without PT_FLAG_NEE is refused before the scene is asked for (pt_render,
    # pt_render_moments; pt_render_rays looks for the scene first, as documented)
    empty = g.PathTracer(0)
    try:
        bufs = [empty.malloc(12 * w * h), empty.malloc(4 * w * h), empty.malloc(8 * w * h), on_device(empty, host_rays), empty.malloc(12 * n)]
        assert raw_calls(empty, cam, no_nee, *bufs, n) == (INVALID, INVALID, NO_SCENE)
        assert raw_calls(empty, cam, box_params(w, h, 4, MIS), *bufs, n) == (NO_SCENE, NO_SCENE, NO_SCENE)
        # ... and behind the PT_FLAG_NEE-needs-PT_FLAG_COSINE_DIFF check: both fail, the message is the earlier one's
        assert empty._lib.pt_render(empty._ctx, bufs[0].ptr, bufs[1].ptr, C.byref(cam), C.byref(box_params(w, h, 4, g.FLAG_NEE | g.FLAG_MIS)), 1) == INVALID
        assert b"PT_FLAG_COSINE_DIFF" in empty._lib.pt_last_error(empty._ctx)
    finally:
        empty.close()
    # with a scene: all three refuse it, and the context renders what it rendered
    box.set_option(g.OPT_KERNEL, g.KERNEL_AUTO)
    before = render_frame(box, cam, box_params(w, h, 4, MIS), 2)
    bufs = [box.malloc(12 * w * h), box.malloc(4 * w * h), box.malloc(8 * w * h), on_device(box, host_rays), box.malloc(12 * n)]
    assert raw_calls(box, cam, no_nee, *bufs, n) == (INVALID, INVALID, INVALID)
    assert raw_calls(box, cam, bare, *bufs, n) == (INVALID, INVALID, INVALID)
    assert b"PT_FLAG_MIS" in box._lib.pt_last_error(box._ctx)
    for b in bufs:
        b.free()
    assert np.array_equal(bits(render_frame(box, cam, box_params(w, h, 4, MIS), 2)), bits(before))
    # Woop records: unsupported from all three; a call without the flag renders
    woop = g.PathTracer(0)
    try:
        woop.set_option(g.OPT_TRI_TEST, 1)
        woop.upload_bvh(g.Bvh(g.scene_mesh("cornell")))
        woop.upload_spheres(g.reference_spheres())
        bufs = [woop.malloc(12 * w * h), woop.malloc(4 * w * h), woop.malloc(8 * w * h), on_device(woop, host_rays), woop.malloc(12 * n)]
        assert raw_calls(woop, cam, box_params(w, h, 4, MIS), *bufs, n) == (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)
        assert raw_calls(woop, cam, no_nee, *bufs, n) == (INVALID, INVALID, INVALID)
        assert raw_calls(woop, cam, box_params(w, h, 4, ref.BASE), *bufs, n) == (0, 0, 0)
        woop.sync()
        assert bufs[0].download(np.float32, (h, w, 3)).any()
    finally:
        woop.close()
