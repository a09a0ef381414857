"""The traversal stack at full depth (TravStack in csrc/pt_walks.h: the LDS window of 16, 24 or all 72 entries, the private overflow
array behind it; the packet walk's per-wave stack; the planner's `3 * wide_depth + 2 <= PT_STACK_CAP` rule) on the hand-built trees of
tests/deep_trees.py, whose CPU side tests/test_deep_trees.py checks.

The scenes are tiny (at most a few hundred triangles, 64 x 64 pixels, 128 rays) and every stack entry decides some ray's answer:
comb(D) makes the binary walks push exactly D entries and the wide walks as many in groups of three, stair(W) makes the wide walks
push three entries at each of W levels.  Every comparison is exact: with brute force (orc.trace_brute) always, with the oracle's own
walk (orc.render) wherever its 64-entry stack holds the tree, that is for a modelled depth of at most 63.  The one tolerance is
Woop's t (test_gpu_wide.test_woop_records_within_tolerance).  Every test asserts the depth its fixture was built for: pt_scene_info's
max_depth, pt_tree_items' wide depth and the stack model's depth for the rays at hand.

The stage-split pipeline has two extend instantiations, (8 waves, 16 entries) and (6, 24); PT_OPT_LDS_STACK 0 runs the first one there
(launch_extend: "the nearest one"), so its LDS-only cases are the frame kernels'.  The megakernel and the persistent kernel's binary
walks likewise run their 16-entry window for a request of 24."""
import math

import numpy as np
import pytest

import deep_trees as dt
import gpu_pathtracer_amd as g
import orc
from scene_matrix import make_camera, spheres, tilted_grid_table
from gpu_support import gpu_trace, is_frame_kernel, is_pipeline, l2, material

pytestmark = pytest.mark.gpu

W = H = 64
DEPTHS = (15, 16, 17, 23, 24, 25, 33, 63, 65)
PT_STACK_CAP = 72
PT_ERR_UNSUPPORTED = -5
OPT_ROOT_ENTRY = g._abi.OPT_ROOT_ENTRY
NEE = g.FLAG_NEE | g.FLAG_COSINE_DIFF
MEGA, PERSIST, WAVE = g.KERNEL_MEGA_BVH2, g.KERNEL_PERSISTENT, g.KERNEL_WAVEFRONT
# every option a case of this module may change, with the value a new context has
BASE = {g.OPT_KERNEL: PERSIST, g.OPT_WALK: 2, g.OPT_LDS_STACK: 16, g.OPT_OCCUPANCY: 6, g.OPT_FIRST_WALK: 1, g.OPT_PACKET_STACK: 72,
        g.OPT_FUSE_STAGES: 1, g.OPT_LAST_ANYHIT: 1, g.OPT_ROOT_CULL: 1, OPT_ROOT_ENTRY: 1, g.OPT_COUNTERS: 0, g.OPT_TIMING: 0}


# ------------------------------------------------------------------------------------------------ fixtures, cameras, references
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixture(name):
    kind, n = name.split("-")[0], int(name.split("-")[1])
    return cached(name, lambda: dt.stair(n) if kind == "stair" else dt.comb(n, mirror=kind == "mirror"))


def camera_down(fx):
    """above the fixture, looking along -z, framing the footprint with a margin of a quarter cell at plane 0"""
    L = fx.z_top + 64.0
    return make_camera(W, H, pos=(4.0, 4.0, L), front=(0, 0, -1), fov=8.5 * 63.0 / (64.0 * L), dist=1.0)


def camera_up(fx):
    """between the comb and the mirror, looking up: the reflected rays come down over the footprint as camera_down's do"""
    L = fx.z_top + 64.0
    return make_camera(W, H, pos=(4.0, 4.0, fx.z_top + 2.0), front=(0, 0, 1), fov=8.5 * 63.0 / (64.0 * L), dist=1.0)


def params(depth, flags=0, cull=1):
    p = g.default_params(W, H, depth=depth)
    p.flags = flags | g.FLAG_WRITE_RGBA
    p.cull_backfaces = cull
    p.frame, p.sample_index = 7, 1
    p.bk_color[:] = (0, 0, 0)
    return p


def id_table(fx):
    """tilted_grid_table's emission ((id + 1) / 256, 0.5, 0.25) per triangle; a mirror's two triangles get a PT_MAT_SPEC row"""
    rows, ids = tilted_grid_table(fx.n_tris)
    for k in getattr(fx, "mirror_ids", ()):
        rows[k] = material((1.0, 1.0, 1.0), mat=g.MAT_SPEC)
    return rows, ids


def decode_ids(acc):
    """the triangle a depth-1, 1-spp pixel of an id-coded frame saw (-1: the black background)"""
    assert np.array_equal(acc[..., 1][acc[..., 0] > 0], np.full((acc[..., 0] > 0).sum(), 0.5, np.float32))
    return (np.rint(acc[..., 0].astype(np.float64) * 256.0).astype(np.int32) - 1).reshape(-1)


def model_depth(fx, rays):
    """the stack model's depth over a sample of `rays` (every 61st: the model is plain Python)"""
    return int(dt.binary_stack_depth(fx, rays[::61]).max())


def oracle_frame(name, cam_of, depth, spp, flags=0, table=True, sph=None):
    fx = fixture(name)
    assert fx.max_depth <= dt.ORACLE_LAST_ENTRY, "the oracle's 64-entry stack does not hold this tree"

    def make():
        tab = id_table(fx) if table else (None, None)
        return orc.render(fx, sph() if sph else None, cam_of(fx), params(depth, flags), spp, materials=tab[0], tri_material=tab[1])[:2]
    return cached(("oracle", name, cam_of.__name__, depth, spp, flags, table, sph), make)


# ------------------------------------------------------------------------------------------------ one context per tree
class Scene:
    """a context with one fixture uploaded; options are set back to BASE before every case"""

    def __init__(self, name, table=True, sph=None, before_upload=()):
        self.fx = fixture(name)
        self.t = g.PathTracer(0)
        for o, v in before_upload:
            self.t.set_option(o, v)
        self.t.upload_bvh(self.fx)
        self.t.upload_spheres(sph() if sph else None)
        if table:
            self.t.upload_tri_materials(*id_table(self.fx))

    def check_tree(self, max_depth, wide_depth):
        """the two preconditions every test asserts: the uploaded tree has the depths the fixture was built for"""
        assert self.fx.max_depth == max_depth and self.fx.wide_depth == wide_depth
        assert self.t.scene_info()["max_depth"] == max_depth
        assert self.t.tree_items()[3] == wide_depth

    def render(self, cam, p, spp=1, **options):
        """(accumulator, display words[, counters + wave stats, stage times]) of one pt_render call under BASE + options"""
        t = self.t
        for o, v in {**BASE, **options_by_id(options)}.items():
            t.set_option(o, v)
        acc, rgba = t.alloc_frame(W, H)
        try:
            t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
            t.sync()
            out = [acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W))]
        finally:
            acc.free()
            rgba.free()
        out.append({**t.counters(), **t.wave_stats()} if options.get("counters") else None)
        out.append(t.stage_ms() if options.get("timing") else None)
        return out

    def close(self):
        self.t.close()


NAMES = {"kernel": g.OPT_KERNEL, "walk": g.OPT_WALK, "lstk": g.OPT_LDS_STACK, "occ": g.OPT_OCCUPANCY, "first_walk": g.OPT_FIRST_WALK,
         "packet_stack": g.OPT_PACKET_STACK, "fuse": g.OPT_FUSE_STAGES, "anyhit": g.OPT_LAST_ANYHIT, "root_cull": g.OPT_ROOT_CULL,
         "root_entry": OPT_ROOT_ENTRY, "counters": g.OPT_COUNTERS, "timing": g.OPT_TIMING}


def options_by_id(options):
    return {NAMES[k]: v for k, v in options.items()}


_scene = {}


def scene(name, **kw):
    """the context of the fixture `name` (and of what else is uploaded with it), kept until the module is done"""
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _scene:
        _scene[key] = Scene(name, **kw)
    return _scene[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for s in _scene.values():
        s.close()
    _scene.clear()


def same_frame(got, ref, what):
    assert np.array_equal(got[0].view(np.int32), ref[0].view(np.int32)), f"{what}: accumulator differs in {int(np.any(got[0] != ref[0], axis=-1).sum())} pixels"
    assert np.array_equal(got[1], ref[1]), f"{what}: display words differ"
    assert got[0].any(), what


# ------------------------------------------------------------------------------------------------ a. ray batches
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("D", DEPTHS)
def test_ray_batch_over_comb(D, cull):
    """stack depth D (every one of the 128 rays pushes D entries; pt_trace_rays keeps all 72 in LDS): t, id and normal of every
    half-cell ray equal brute force, no mismatch allowed.  The first case also reads pt_trace_rays' timed span (PT_OPT_TIMING)."""
    s = scene(f"comb-{D}")
    s.check_tree(D, math.ceil(D / 3))
    rays = dt.cell_rays(s.fx)
    depth = dt.binary_stack_depth(s.fx, rays)
    assert depth.min() == depth.max() == D
    timed = D == DEPTHS[0] and cull
    s.t.set_option(g.OPT_TIMING, int(timed))
    t, tri, nrm = gpu_trace(s.t, rays, cull)
    if timed:
        assert s.t.last_kernel_ms() > 0
        s.t.set_option(g.OPT_TIMING, 0)
    t0, tri0, nrm0 = orc.trace_brute(s.fx.mesh, rays, cull)
    assert np.array_equal(tri0, dt.expected_ids(s.fx, rays)) and (tri0 >= 0).sum() == D + 1
    assert np.array_equal(tri, tri0), f"ids differ for rays {np.nonzero(tri != tri0)[0][:8]}"
    assert np.array_equal(t.view(np.int32), t0.view(np.int32))
    assert np.array_equal(nrm[tri0 >= 0], nrm0[tri0 >= 0])


@pytest.mark.parametrize("D", DEPTHS)
def test_first_hit_ids_over_comb(D):
    """stack depth D: pt_render_aux's ids for the pixel-centre rays of the depth-1 camera equal brute force exactly"""
    s = scene(f"comb-{D}")
    s.check_tree(D, math.ceil(D / 3))
    cam, p = camera_down(s.fx), params(1)
    rays = orc.primary_rays(cam, W, H, p.frame, jitter=False)
    assert model_depth(s.fx, rays) == D
    bufs = [s.t.malloc(W * H * 16) for _ in range(3)] + [s.t.malloc(W * H * 4)]
    try:
        s.t.render_aux(cam, p, *[b.ptr for b in bufs])
        s.t.sync()
        ids = bufs[3].download(np.int32, (H * W,))
    finally:
        for b in bufs:
            b.free()
    _, tri0, _ = orc.trace_brute(s.fx.mesh, rays, True)
    assert len(set(tri0[tri0 >= 0])) == D + 1            # every leaf is seen by some pixel
    assert np.array_equal(ids[tri0 >= 0], tri0[tri0 >= 0]) and (ids[tri0 < 0] < 0).all()


# ------------------------------------------------------------------------------------------------ b. id-coded frame at depth 1
def frame_configs():
    """id -> options: every kernel x walk, every LDS window, and the occupancies that pick another instantiation (launch_mega,
    launch_persist, launch_extend)"""
    cfg = {}
    for walk in (0, 1, 2):
        for occ, lstk in ((8, 16), (4, 16), (6, 24), (6, 0)):
            cfg[f"mega-walk{walk}-occ{occ}-lstk{lstk}"] = dict(kernel=MEGA, walk=walk, occ=occ, lstk=lstk)
    for walk in (0, 1):
        for lstk in (16, 24, 0):
            cfg[f"persistent-walk{walk}-lstk{lstk}"] = dict(kernel=PERSIST, walk=walk, lstk=lstk)
    for walk in (2, 4):
        for occ, lstk in ((4, 16), (6, 16), (8, 16), (6, 24), (6, 0)):
            cfg[f"persistent-walk{walk}-occ{occ}-lstk{lstk}"] = dict(kernel=PERSIST, walk=walk, occ=occ, lstk=lstk)
    for first_walk in (0, 1):
        for lstk in (16, 24):
            cfg[f"pipeline-first{first_walk}-lstk{lstk}"] = dict(kernel=WAVE, first_walk=first_walk, lstk=lstk)
    for lstk in (16, 24):
        cfg[f"pipeline-packet-short-lstk{lstk}"] = dict(kernel=WAVE, first_walk=1, lstk=lstk, packet_stack="short")
    return cfg


FRAME_CONFIGS = frame_configs()


def lds_window(o):
    """the LDS window a configuration's walks really run with (see the module docstring)"""
    lstk = o["lstk"]
    if o["kernel"] == WAVE:
        return 24 if lstk == 24 else 16
    if lstk == 0:
        return PT_STACK_CAP
    if o["kernel"] == MEGA or o["walk"] <= 1:
        return 16
    return lstk


@pytest.mark.parametrize("D,config", [(D, c) for D in DEPTHS for c in FRAME_CONFIGS])
def test_id_coded_frame(D, config):
    """stack depth D (binary walks; the wide walks push the same D entries three at a time): the depth-1 frame of a camera above
    comb(D), every triangle emitting its own id.  The ids decoded from the colours equal brute force on the same primary rays
    for every D, 65 included; the accumulator and the display words equal the oracle's bit for bit where D <= 63.  Instrumented
    (PT_OPT_COUNTERS) the same frame again, and the overflow counter says which side of the LDS window the run was on: > 0
    where D exceeds the window, 0 where all 72 entries are in LDS; the packet kernel books its groups exactly when
    3 * wide_depth + 2 fits PT_OPT_PACKET_STACK."""
    s = scene(f"comb-{D}")
    wide = math.ceil(D / 3)
    s.check_tree(D, wide)
    o = dict(FRAME_CONFIGS[config])
    need = 3 * wide + 2
    if o.get("packet_stack") == "short":
        o["packet_stack"] = need - 1
    cam, p = camera_down(s.fx), params(1)
    rays = orc.primary_rays(cam, W, H, p.frame)
    assert cached(("model", D), lambda: model_depth(s.fx, rays)) == D
    _, tri0, _ = cached(("brute", D), lambda: orc.trace_brute(s.fx.mesh, rays, True))
    assert len(set(tri0[tri0 >= 0])) == D + 1
    for counters in (0, 1):
        acc, rgba, cnt, _ = s.render(cam, p, 1, counters=counters, **o)
        ids = decode_ids(acc)
        bad = np.nonzero(ids != tri0)[0]
        assert len(bad) == 0, f"{config}, counters {counters}: {len(bad)} pixels show another triangle than brute force, first {bad[:6]}: {ids[bad[:6]]} for {tri0[bad[:6]]}"
        if D <= dt.ORACLE_LAST_ENTRY:
            same_frame((acc, rgba), oracle_frame(f"comb-{D}", camera_down, 1, 1), f"{config}, counters {counters}")
    print(f"comb({D}) {config}: stack_overflows {cnt['stack_overflows']}, it_shade {cnt['it_shade']}")
    groups = (W // 8) * (H // 8)
    packet = o["kernel"] == WAVE and o["first_walk"] == 1 and need <= o.get("packet_stack", 72)
    if o["kernel"] == WAVE:
        assert cnt["it_shade"] == (groups if packet else 0)
    window = lds_window(o)
    if o["kernel"] == MEGA:
        return                      # pt_get_wave_stats is the persistent kernel's and the pipeline's (include/ptmi.h): nothing booked
    if window >= PT_STACK_CAP or packet:     # (the packet walk keeps its own per-wave stack; at depth 1 it is the call's only walk)
        assert cnt["stack_overflows"] == 0
    elif D > window:
        assert cnt["stack_overflows"] > 0


# ------------------------------------------------------------------------------------------------ c. later bounces
MIRROR_D = 33          # tree depth 34: past both LDS windows, and within the oracle's stack
LATER = [dict(kernel=WAVE, root_cull=rc, root_entry=re, fuse=fu, lstk=ls) for rc in (0, 1) for re in (0, 1) for fu in (0, 1) for ls in (16, 24)]
LATER += [dict(kernel=k, lstk=ls) for k in (PERSIST, MEGA) for ls in (16, 24)]


def later_id(o):
    return "-".join(f"{k}{v}" for k, v in o.items())


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("o", LATER, ids=later_id)
def test_later_bounces_through_the_comb(o, depth):
    """stack depth 33 below a root that also holds a mirror leaf (tree depth 34, wide depth 12): the camera looks up at the mirror,
    the reflected rays come down through the comb, so the deep walks are those of bounce 1 (queued walks, root-entry starts that
    pre-load the stack with the root's other children) and, at depth 3, bounce 2.  4 spp inside a dark sphere that closes the scene;
    equal to the oracle bit for bit.  A
    material table is on the context, so the last segment stays a closest-hit walk."""
    name = f"mirror-{MIRROR_D}"
    s = scene(name, sph=room)
    s.check_tree(MIRROR_D + 1, 1 + math.ceil((MIRROR_D - 2) / 3))
    down = dt.cell_rays(s.fx, rise=34.0)            # from above the mirror's height: what a reflected ray is to the tree
    assert int(dt.binary_stack_depth(s.fx, down[::8]).max()) == MIRROR_D
    cam, p = camera_up(s.fx), params(depth)
    ref = oracle_frame(name, camera_up, depth, 4, sph=room)
    assert len(np.unique(ref[0][..., 0])) > MIRROR_D // 2          # the comb's ids show in the mirror
    got = s.render(cam, p, 4, **o)
    same_frame(got, ref, f"{later_id(o)} depth {depth}")


# ------------------------------------------------------------------------------------------------ d. any-hit last segment
ROOM = (4.0, 4.0, 0.0, 300.0, (0, 0, 0), (0.75, 0.75, 0.75), g.MAT_DIFF)     # encloses everything: no path ends on a miss


def room():
    return spheres([ROOM])


def lamp_below():
    return spheres([(4.0, 4.0, -30.0, 20.0, (4.0, 3.0, 2.0), (0.5, 0.5, 0.5), g.MAT_DIFF), ROOM])


@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("lstk", [16, 24])
def test_anyhit_last_segment_through_the_comb(depth, lstk):
    """stack depth 33 (tree depth 34) for the segments that come down from the now diffuse plate above the camera: no table, a dark
    DIFF material, one emissive sphere below the comb, so a path's last segment is an any-hit query (PT_OPT_LAST_ANYHIT 1) that a
    half-cell's triangle blocks or not.  It must equal the closest-hit walk (0), both must equal the oracle, and instrumented with
    the value 2 the any-hit launch reports its rays ("act_shade") and its overflows."""
    name = f"mirror-{MIRROR_D}"
    s = scene(name, table=False, sph=lamp_below)
    s.check_tree(MIRROR_D + 1, 1 + math.ceil((MIRROR_D - 2) / 3))
    down = dt.cell_rays(s.fx, rise=34.0)
    assert int(dt.binary_stack_depth(s.fx, down[::8]).max()) == MIRROR_D
    cam, p = camera_up(s.fx), params(depth)
    ref = oracle_frame(name, camera_up, depth, 4, table=False, sph=lamp_below)
    lit = np.any(ref[0] > 0, axis=-1).mean()
    assert 0.05 < lit < 0.95                                     # some paths reach the lamp, some are blocked
    for fuse in (0, 1):
        closest = s.render(cam, p, 4, kernel=WAVE, anyhit=0, lstk=lstk, fuse=fuse)
        anyhit = s.render(cam, p, 4, kernel=WAVE, anyhit=1, lstk=lstk, fuse=fuse)
        same_frame(closest, ref, f"closest hit, fuse {fuse}")
        same_frame(anyhit, ref, f"any hit, fuse {fuse}")
    counted = s.render(cam, p, 4, kernel=WAVE, anyhit=2, lstk=lstk, counters=1)
    same_frame(counted, ref, "any hit, instrumented")
    assert counted[2]["act_shade"] > 0 and counted[2]["stack_overflows"] > 0
    for kernel in (PERSIST, MEGA):
        same_frame(s.render(cam, p, 4, kernel=kernel, lstk=lstk), ref, f"kernel {kernel}")


@pytest.mark.parametrize("kernel", [WAVE, MEGA], ids=["shadow-stage", "mega-loop"])
def test_shadow_rays_through_the_comb(kernel):
    """stack depth 33: PT_FLAG_NEE | PT_FLAG_COSINE_DIFF over the same scene, so shadow rays run from the plate down through the comb
    to the lamp: the pipeline's shadow-ray stage and the megakernel's loop, against the oracle with the same flags"""
    name = f"mirror-{MIRROR_D}"
    s = scene(name, table=False, sph=lamp_below)
    s.check_tree(MIRROR_D + 1, 1 + math.ceil((MIRROR_D - 2) / 3))
    assert int(dt.binary_stack_depth(s.fx, dt.cell_rays(s.fx, rise=34.0)[::8]).max()) == MIRROR_D
    cam, p = camera_up(s.fx), params(3, flags=NEE)
    ref = oracle_frame(name, camera_up, 3, 4, flags=NEE, table=False, sph=lamp_below)
    for lstk in (16, 24):
        same_frame(s.render(cam, p, 4, kernel=kernel, lstk=lstk), ref, f"lstk {lstk}")


# ------------------------------------------------------------------------------------------------ e. Woop records
@pytest.mark.parametrize("D", DEPTHS)
def test_woop_records_over_comb(D):
    """stack depth D under the persistent kernel's Woop walk (PT_OPT_TRI_TEST 1; the ray-batch kernel refuses these records, so the
    rays are the depth-1 camera's).  The pixels' ids equal brute force exactly: ids do not depend on t's last bits, and no ray of
    this camera grazes an edge closer than brute force itself resolves.  t feeds the next bounce, so a depth-2 frame (inside a dark
    sphere that closes the scene) is held to
    test_woop_records_within_tolerance's bars: per-pixel L2 < 1e-3 from a few spp on, at most 1e-4 of the pixels off by 1e-2."""
    s = scene(f"comb-{D}", before_upload=((g.OPT_TRI_TEST, 1),), sph=room)
    try:
        assert s.t.scene_info()["max_depth"] == D and s.fx.wide_depth == math.ceil(D / 3)     # (pt_tree_items reads exact records' layout too)
        assert s.t.tree_items()[3] == math.ceil(D / 3)
        cam, p = camera_down(s.fx), params(1)
        rays = orc.primary_rays(cam, W, H, p.frame)
        assert cached(("model", D), lambda: model_depth(s.fx, rays)) == D
        _, tri0, _ = cached(("brute", D), lambda: orc.trace_brute(s.fx.mesh, rays, True))
        for lstk, occ in ((16, 8), (16, 4), (24, 6), (0, 6)):
            acc = s.render(cam, p, 1, kernel=PERSIST, lstk=lstk, occ=occ)[0]
            assert np.array_equal(decode_ids(acc), tri0), f"lstk {lstk} occ {occ}"
        if D <= dt.ORACLE_LAST_ENTRY:
            ref = oracle_frame(f"comb-{D}", camera_down, 2, 8, sph=room)
            acc = s.render(cam, params(2), 8, kernel=PERSIST)[0]
            err, big = l2(acc, ref[0]), int((np.abs(acc - ref[0]).max(axis=-1) > 1e-2).sum())
            print(f"woop comb({D}) depth 2, 8 spp: L2 {err:.3e}, pixels off by > 1e-2: {big}")
            assert err < 1e-3 and big <= W * H // 10000
    finally:
        s.t.set_option(g.OPT_TRI_TEST, 0)


# ------------------------------------------------------------------------------------------------ f. the wide / binary boundary
@pytest.mark.parametrize("Wd", [23, 24])
def test_wide_walk_gives_way_to_the_binary_walk(Wd):
    """stair(23): wide depth 23, 3 * 23 + 2 = 71 entries, the last tree the wide walk takes (three pushes at each level);
    stair(24) needs 74 > PT_STACK_CAP: the binary walk runs (stack depth 24) and a requested pipeline becomes the persistent kernel.
    What ran is read as test_gpu_call_plan reads it (stage times) and from the wide walks' own step counters; the frames of all
    three kernel requests equal the oracle's bit for bit, at depth 1 (id-coded) and depth 3."""
    name = f"stair-{Wd}"
    s = scene(name, sph=room)
    s.check_tree(Wd + 1, Wd)
    wide_ok = 3 * Wd + 2 <= PT_STACK_CAP
    assert wide_ok == (Wd == 23)
    cam = camera_down(s.fx)
    rays = orc.primary_rays(cam, W, H, 7)
    assert model_depth(s.fx, rays) == Wd
    _, tri0, _ = orc.trace_brute(s.fx.mesh, rays, True)
    assert len(set(tri0[tri0 >= 0])) == Wd
    for depth, spp in ((1, 1), (3, 4)):
        p = params(depth)
        ref = oracle_frame(name, camera_down, depth, spp, sph=room)
        for kernel in (MEGA, PERSIST, WAVE):
            for lstk in (16, 24, 0):
                got = s.render(cam, p, spp, kernel=kernel, lstk=lstk, timing=1)
                same_frame(got, ref, f"kernel {kernel} lstk {lstk} depth {depth}")
                if depth == 1:
                    assert np.array_equal(decode_ids(got[0]), tri0)
                ms = got[3]
                assert is_pipeline(ms) if kernel == WAVE and wide_ok else is_frame_kernel(ms), (kernel, ms)
    p = params(1)
    for kernel, first_walk in ((MEGA, 1), (PERSIST, 1), (WAVE, 0), (WAVE, 1)):
        got = s.render(cam, p, 1, kernel=kernel, first_walk=first_walk, counters=1)
        same_frame(got, oracle_frame(name, camera_down, 1, 1, sph=room), f"instrumented, kernel {kernel}, first walk {first_walk}")
        c = got[2]
        print(f"stair({Wd}) kernel {kernel} first walk {first_walk}: {c}")
        if kernel == MEGA:                                    # (pt_get_wave_stats is the other two families')
            continue
        packet = kernel == WAVE and first_walk == 1 and wide_ok
        assert (c["it_node"] > 0) == wide_ok                  # the wide walks' node steps: none when the binary walk ran
        assert (c["stack_overflows"] > 0) == (not packet)     # three entries per level, or 24, against a window of 16
        if kernel == WAVE and wide_ok:                        # the packet kernel's groups: the pipeline's own stat
            assert c["it_shade"] == ((W // 8) * (H // 8) if packet else 0)


def test_woop_records_on_a_tree_too_deep_for_the_wide_walk():
    """stair(24), stack depth 24 for the binary walk, which cannot read Woop records: pt_render answers PT_ERR_UNSUPPORTED, and with
    the option set back and the tree uploaded again the context renders the oracle's frame"""
    name = "stair-24"
    s = scene(name, before_upload=((g.OPT_TRI_TEST, 1),))
    try:
        assert s.t.scene_info()["max_depth"] == 25 and s.t.tree_items()[3] == 24
        cam, p = camera_down(s.fx), params(1)
        assert model_depth(s.fx, orc.primary_rays(cam, W, H, 7)) == 24
        for kernel in (MEGA, PERSIST, WAVE):
            with pytest.raises(g.PtError) as e:
                s.render(cam, p, 1, kernel=kernel)
            assert e.value.code == PT_ERR_UNSUPPORTED
    finally:
        s.t.set_option(g.OPT_TRI_TEST, 0)
    s.t.upload_bvh(s.fx)
    s.t.upload_tri_materials(*id_table(s.fx))
    s.check_tree(25, 24)
    for kernel in (MEGA, PERSIST, WAVE):
        same_frame(s.render(cam, p, 1, kernel=kernel), oracle_frame(name, camera_down, 1, 1), f"kernel {kernel}")


# ------------------------------------------------------------------------------------------------ g. the device builders' limit
def chain_rays(mesh):
    """one ray at every triangle's centroid from 2^-10 of the scene away, direction (-1/4, 1/8, 1): onto the front of the (1, 0, -1) normals"""
    c = np.asarray(mesh.verts, np.float64)[np.asarray(mesh.tris)].mean(axis=1)
    d = np.array([-0.25, 0.125, 1.0])
    rays = np.zeros((len(c), 8), np.float32)
    rays[:, 0:3] = c - d * (dt.CHAIN_SCALE / 1024.0)
    rays[:, 4:7] = d
    return rays


@pytest.mark.parametrize("n_equal", [8, 2])
@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
def test_device_builders_at_their_depth_limit(algo, n_equal):
    """stack depth at most 64, the builders' limit: morton_chain_mesh's keys chain (found on the CPU from the keys:
    tests/test_deep_trees.py), so the linear BVH is 66 levels deep with eight equal keys at the chain's end and exactly 64 with two.
    Whichever builder runs (PLOC, PLOC falling back to the LBVH, the LBVH), the result is a tree of at most 64 levels whose hits
    equal brute force, or the documented PT_ERR_UNSUPPORTED with the context, and the tree it held, usable afterwards."""
    mesh = dt.morton_chain_mesh(n_equal)
    assert dt.lbvh_depth(dt.morton_keys(mesh)) == (65 if n_equal == 8 else 63)
    rays = chain_rays(mesh)
    brute = {cull: orc.trace_brute(mesh, rays, cull) for cull in (True, False)}
    assert (brute[True][1] >= 0).mean() > 0.9 and len(set(brute[True][1])) > mesh.n_tris // 2
    held = fixture("comb-17")
    held_rays = dt.cell_rays(held)
    t = g.PathTracer(0)
    try:
        t.upload_bvh(held)
        t.set_option(g.OPT_BUILD_ALGO, algo)
        v, f = np.ascontiguousarray(mesh.verts, np.float32), np.ascontiguousarray(mesh.tris, np.int32)
        rc = t._lib.pt_build_bvh(t._ctx, v.ctypes.data, len(v), f.ctypes.data, len(f))
        print(f"algo {algo}, {n_equal} equal keys: pt_build_bvh -> {rc}" + (f", max_depth {t.scene_info()['max_depth']}, wide depth {t.tree_items()[3]}" if rc == 0 else ""))
        assert rc in (0, PT_ERR_UNSUPPORTED)
        if algo == 0:      # the linear BVH is the hierarchy modelled on the CPU: 65 edges to its deepest inner node is too deep, 63 is not
            assert (rc == 0) == (n_equal == 2) and (rc != 0 or t.scene_info()["max_depth"] == 64)
        if rc == 0:
            assert t.last_build_ms() > 0 and t.scene_info()["max_depth"] <= 64
            for cull, (t0, tri0, nrm0) in brute.items():
                tg, ig, ng = gpu_trace(t, rays, cull)
                assert np.array_equal(ig, tri0) and np.array_equal(tg.view(np.int32), t0.view(np.int32)), f"cull {cull}"
                assert np.array_equal(ng[tri0 >= 0], nrm0[tri0 >= 0])
            p = params(1, cull=0)
            p.tri_emi[:] = (0.5, 0.25, 0.125)
            cam = make_camera(W, H, pos=(0.4 * dt.CHAIN_SCALE, 0.1 * dt.CHAIN_SCALE, 3.0 * dt.CHAIN_SCALE), front=(0, 0, -1), dist=1.0)
            acc, rgba = t.alloc_frame(W, H)
            for kernel in (MEGA, PERSIST, WAVE):         # the walks of the three families take the tree too, and agree
                t.set_option(g.OPT_KERNEL, kernel)
                acc.zero()
                t.launch_kernel(acc.ptr, rgba.ptr, cam, p, 1)
                t.sync()
                frame = acc.download(np.float32, (H, W, 3))
                if kernel == MEGA:
                    first = frame
                assert np.array_equal(frame.view(np.int32), first.view(np.int32)) and frame.any(), f"kernel {kernel}"
        else:
            assert t.last_build_ms() == -1.0 and t.scene_info()["max_depth"] == 17      # the uploaded comb is still the tree
            tg, ig, _ = gpu_trace(t, held_rays, True)
            t0, tri0, _ = orc.trace_brute(held.mesh, held_rays, True)
            assert np.array_equal(ig, tri0) and np.array_equal(tg.view(np.int32), t0.view(np.int32))
    finally:
        t.close()
