"""What the GPU test modules share: cameras, cached trees, launches through the C ABI, moved geometry, the A/B renderer of the
stage-split pipeline's options, the arbitration of a frame against the oracle, and the guide buffers.  A plain module found
through tests/ on sys.path, like orc, scene_matrix and tree_audit; importing it needs the built host library and no GPU.

A helper lives here when two or more test modules use it; each has one definition, and its docstring names the suites that rely
on it.  No test module imports another test module (tests/test_support_layout.py).  pytest does not rewrite the asserts of a
plain module, so every helper that asserts states its own message."""
import numpy as np

import gpu_pathtracer_amd as g
import orc
from scene_matrix import make_camera, red_copies_table


# ---------------------------------------------------------------------------------------------------- cameras, trees, launches
def golden_camera(W, H):
    """The default camera with the 1080p field of view at any test resolution: the camera of the committed oracle images
    (tests/golden/make_golden.py) and of nearly every suite, the CPU ones test_oracle and test_temporal included."""
    cam = g.default_camera(W, H)
    cam.dist = 18.0 * H / 1080.0
    return cam


def l2(a, b):
    """Per-pixel L2 of two accumulators, the measure of the north-star bar (< 1e-3): test_gpu_parity, test_gpu_wide,
    test_gpu_bench_configs, test_gpu_scene_matrix, test_gpu_deep_stack, and `check` / `judge` below."""
    return float(np.sqrt(np.mean(np.sum((a.astype(np.float64) - b) ** 2, axis=-1))))


_bvh_cache = {}


def bvh_of(name, **kw):
    """(mesh, host tree) of a named scene, built once per (name, builder keywords) for the whole run: every suite that renders a
    named scene, and test_reference_radiance."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _bvh_cache:
        mesh = g.scene_mesh(name)
        _bvh_cache[key] = (mesh, g.Bvh(mesh, **kw))
    return _bvh_cache[key]


def gpu_render(pt, bvh, spheres, cam, p, spp=1, accum_init=None):
    """One pt_render call on the context `pt` after uploading the scene: (accumulator, display words).  test_gpu_parity,
    test_gpu_wide, test_gpu_bench_configs."""
    W, H = p.width, p.height
    if bvh is not None:
        pt.upload_bvh(bvh)
    pt.upload_spheres(spheres)
    acc, rgba = pt.alloc_frame(W, H)
    if accum_init is not None:
        acc.upload(accum_init)
    pt.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
    pt.sync()
    a = acc.download(np.float32, (H, W, 3))
    r = rgba.download(np.uint32, (H, W))
    acc.free()
    rgba.free()
    return a, r


def gpu_trace(pt, rays, cull=True):
    """pt_trace_rays over host rays: (t, triangle id, normal).  test_gpu_parity, test_gpu_build, test_gpu_refit,
    test_gpu_tree_adopt, test_gpu_scene_matrix, test_gpu_deep_stack, test_gpu_bench_configs."""
    n = len(rays)
    d_r = pt.malloc(rays.nbytes)
    d_r.upload(rays)
    d_t, d_i, d_n = pt.malloc(4 * n), pt.malloc(4 * n), pt.malloc(12 * n)
    pt.trace_rays(d_r.ptr, n, cull, d_t.ptr, d_i.ptr, d_n.ptr)
    pt.sync()
    out = d_t.download(np.float32, (n,)), d_i.download(np.int32, (n,)), d_n.download(np.float32, (n, 3))
    for b in (d_r, d_t, d_i, d_n):
        b.free()
    return out


def bits(a):
    """An array's words, for comparisons that must not treat NaNs or signed zeros specially: test_gpu_moments, test_gpu_temporal."""
    return np.ascontiguousarray(a).view(np.int32)


def is_pipeline(ms):
    """PathTracer.stage_ms() of a call that ran the stage-split launches and no frame kernel: test_gpu_call_plan,
    test_gpu_deep_stack."""
    return ms["generate"] > 0 and ms["extend"] > 0 and ms["frame"] == 0


def is_frame_kernel(ms):
    """PathTracer.stage_ms() of a call that ran the persistent kernel or the megakernel and none of generate / extend / shade:
    test_gpu_call_plan, test_gpu_deep_stack."""
    return ms["frame"] > 0 and ms["generate"] == 0 and ms["extend"] == 0 and ms["shade"] == 0


def material(col, emi=(0, 0, 0), mat=g.MAT_DIFF, phong=0.0):
    """A row of a per-triangle material table: test_materials, test_gpu_deep_stack, test_gpu_tree_adopt."""
    m = g.Material()
    m.col[:] = col
    m.emi[:] = emi
    m.mat, m.phong_expo = mat, phong
    return m


# ---------------------------------------------------------------------------------------------------- moved geometry
def soup_mesh(soup):
    """A Mesh whose triangle t is row t of the soup (the ids a refit tree reports): test_gpu_refit, test_gpu_tree_audit,
    test_gpu_tree_adopt, test_gpu_denoise."""
    s = np.ascontiguousarray(soup, np.float32).reshape(-1, 9)
    return g.Mesh.from_arrays(s.reshape(-1, 3), np.arange(3 * len(s), dtype=np.int32).reshape(-1, 3))


def needles():
    """A 16 x 16 patch of small triangles beside needles 1000 x longer than wide, at 45 degrees to the axes, of lengths that
    ask the pre-split for 2..8 slabs (float32 [560][9], the 48 needles last).  test_gpu_tree_audit, test_build_ref,
    test_gpu_build_ref."""
    tris = []
    h = 0.05
    for i in range(16):
        for j in range(16):
            p = np.array([i * h, j * h, 0.0])
            tris.append([p, p + [h, 0, 0], p + [0, h, 0.01]])
            tris.append([p + [h, 0, 0], p + [h, h, 0.02], p + [0, h, 0.01]])
    dirs = [np.array(d) / np.sqrt(2.0) for d in ([1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0])]
    for k in range(48):
        L = 0.08 * 1.09 ** k
        d = dirs[k % 4]
        side = np.cross(d, [0.3, 0.5, 0.8])
        side = side / np.linalg.norm(side) * (L / 1000.0)
        o = np.array([1.0 + 0.03 * k, 0.02 * k, 0.1 + 0.01 * k])
        tris.append([o, o + L * d, o + 0.5 * L * d + side])
    return np.array(tris, np.float32).reshape(-1, 9)


BUILDER_ASSETS = ("cube", "cornell", "bunny_low", "gto_sixteen")
_builder_meshes = {}


def builder_mesh(name):
    """(Mesh, verts, tris, soup) of a mesh of the builder tests, made once: a committed asset, "needles", "needles-63" / "needles-64"
    (the first 63 / 64 rows of needles() with its 48 long triangles moved to the front: either side of the pre-split's triangle
    threshold) or a synthetic case of build_ref.case_soup.  verts / tris are the arrays pt_build_bvh receives.  test_build_ref,
    test_gpu_build_ref."""
    if name not in _builder_meshes:
        import build_ref
        if name in BUILDER_ASSETS:
            mesh = g.scene_mesh(name)
        elif name.startswith("needles"):
            s = needles()
            mesh = soup_mesh(s if name == "needles" else np.concatenate([s[-48:], s[:-48]])[:int(name[8:])])
        else:
            mesh = soup_mesh(build_ref.case_soup(name))
        verts, tris = np.ascontiguousarray(mesh.verts, np.float32), np.ascontiguousarray(mesh.tris, np.int32)
        soup = mesh.triangle_soup()
        for a in (verts, tris, soup):
            a.setflags(write=False)
        _builder_meshes[name] = (mesh, verts, tris, soup)
    return _builder_meshes[name]


def twist(soup, amount, shift):
    """Non-rigid: every vertex turns about the vertical axis through the mesh centre by an angle that grows with its height,
    then moves by `shift` (a number, a tuple or an array) x the extent.  A function of the vertex alone, so shared vertices stay
    shared.  test_gpu_refit, test_gpu_tree_audit."""
    v = soup.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    a = amount * (v[:, 1] - c[1]) / ext
    x, z = v[:, 0] - c[0], v[:, 2] - c[2]
    out = np.stack([c[0] + np.cos(a) * x - np.sin(a) * z, v[:, 1], c[2] + np.sin(a) * x + np.cos(a) * z], 1) + np.asarray(shift, np.float64) * ext
    return out.astype(np.float32).reshape(soup.shape)


def turn_rows(soup, rows, deg, shift):
    """Rigid: rows `rows` turn by `deg` about the vertical axis through their centre and move by `shift`.  test_gpu_refit,
    test_gpu_scene_matrix, and cornell_dragon_moved below."""
    out = soup.copy()
    v = soup[rows].reshape(-1, 3).astype(np.float64)
    c = 0.5 * (v.min(0) + v.max(0))
    a = np.radians(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    out[rows] = ((v - c) @ R.T + c + np.asarray(shift)).astype(np.float32).reshape(-1, 9)
    return out


def cornell_dragon_moved(deg=25.0, shift=(1.5, 0.5, -1.0)):
    """(mesh, its soup, the soup with the dragon turned and moved inside the box): test_gpu_refit, test_gpu_denoise,
    test_gpu_root_entry."""
    mesh = g.scene_mesh("cornell_dragon")
    n_box = g.Mesh.asset("cornell").n_tris
    soup = mesh.triangle_soup()
    return mesh, soup, turn_rows(soup, np.arange(n_box, len(soup)), deg, shift)


def rays_for(soup, n, seed):
    """Incoherent rays through the bounds of a soup: test_gpu_refit, test_gpu_tree_adopt."""
    v = soup.reshape(-1, 3)
    return orc.random_rays(n, v.min(0), v.max(0), seed=seed)


# ---------------------------------------------------------------------------------------------------- pipeline options, A / B
COUNTERS = ("rays", "inner", "tris", "leaves", "hits", "paths")   # the work counters: test_gpu_root_cull, test_gpu_root_entry


def set_options(t, pairs):
    """The (option, value) pairs on a context that has no scene yet, in the order given.  The one ordering rule: an option is set
    BEFORE the upload that reads it — PT_OPT_TRI_TEST, PT_OPT_LEAF_MAX, PT_OPT_REBUILD, PT_OPT_OPTIMIZE and PT_OPT_PRESPLIT before
    pt_upload_bvh, PT_OPT_BUILD_ALGO and PT_OPT_LEAF_MAX before pt_build_bvh, PT_OPT_ENV_LIGHT before pt_upload_environment (which
    PathTracer.upload_environment's `light` does itself) — and every other option is read by the calls, so all of them go on first and
    the scene afterwards.  `pipeline_render` below and call_sequences.install."""
    for o, v in pairs:
        t.set_option(o, v)


def pipeline_render(options, scene, W, H, spp, depth=4, flags=0, spheres=True, calls=1, prefill=False, counters=False, cam=None,
                    tri_emi=(0, 0, 0), tri_mat=g.MAT_DIFF, table=None, parts=1, cull=None, before_upload=()):
    """(accumulator, display words) after `calls` pt_render calls on a fresh context with PT_KERNEL_WAVEFRONT asked for and the
    (option, value) pairs of `options`, then of `before_upload`, set before the scene goes up.  test_gpu_fused_stages,
    test_gpu_last_anyhit, test_gpu_root_cull, test_gpu_packet_first and test_gpu_root_entry each render the same call with one
    option at two or three values and compare the results with `same`.
    scene: a name of bvh_of, None for no tree on the context, or a callable install(t) that puts a tree there; spheres: the
    reference's, or none; table(mesh) -> the arguments of pt_upload_tri_materials (named scenes only); cam: the golden camera
    unless given; prefill: the accumulator starts as a fixed frame and the first call's sample_index is 5 (a running mean under
    way); parts > 1: every call as that many tile-split parts of 8 rows; cull: cull_backfaces, when not the default.
    counters: PT_OPT_COUNTERS is set and a third item is returned, one dict of counters() and wave_stats() summed over every
    launch (both report the last launch only; their keys do not collide)."""
    t = g.PathTracer(0)
    try:
        set_options(t, ((g.OPT_KERNEL, g.KERNEL_WAVEFRONT),) + tuple(options) + tuple(before_upload) + (((g.OPT_COUNTERS, 1),) if counters else ()))
        mesh = None
        if callable(scene):
            scene(t)
        elif scene is not None:
            mesh, bvh = bvh_of(scene)
            t.upload_bvh(bvh)
        t.upload_spheres(g.reference_spheres() if spheres else None)
        if table is not None:
            t.upload_tri_materials(*table(mesh))
        cam = golden_camera(W, H) if cam is None else cam
        acc, rgba = t.alloc_frame(W, H)
        first = 1
        if prefill:
            acc.upload(np.random.default_rng(3).random((H, W, 3), dtype=np.float32))
            first = 5
        total = {}
        for call in range(calls):
            for part in range(parts):
                p = g.default_params(W, H, depth=depth, tri_mat=tri_mat)
                p.flags = flags | g.FLAG_WRITE_RGBA
                p.tri_emi[:] = tri_emi
                if cull is not None:
                    p.cull_backfaces = cull
                p.frame, p.sample_index = 7 + call * spp, first + call * spp
                if parts > 1:
                    p.part_index, p.part_count, p.part_rows = part, parts, 8
                t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
                if counters:
                    for k, v in {**t.counters(), **t.wave_stats()}.items():
                        total[k] = total.get(k, 0) + v
        t.sync()
        out = (acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W)))
        if counters:
            out += (total,)
        acc.free()
        rgba.free()
        return out
    finally:
        t.close()


def same(a, b, what):
    """Two results of pipeline_render (or any (accumulator, display words, ...)) hold the same non-empty frame bit for bit: the
    five suites of pipeline_render."""
    assert np.array_equal(a[0], b[0]), f"{what}: accumulator differs"
    assert np.array_equal(a[1], b[1]), f"{what}: display words differ"
    assert a[0].any(), f"{what}: the frame is empty"


def upload(bvh):
    """The install(t) that uploads a host tree, for pipeline_render's callable scene: test_gpu_packet_first."""
    return lambda t: t.upload_bvh(bvh)


def dark_table(mesh):
    """A per-triangle material table whose rows emit nothing: a table is on the context, so a call is not eligible for what
    needs "no triangle emits".  test_gpu_last_anyhit, test_gpu_root_cull, test_gpu_root_entry."""
    p = g.default_params(8, 8)
    n = len(np.asarray(mesh.tris))
    table, ids = red_copies_table(n, n, p)
    return table, ids


# the Cornell floor (y = -15) touches the floor sphere's top at (0, -15, -20): t and ts agree to the last bits for segments that
# land near that point.  test_gpu_last_anyhit, test_gpu_root_cull.
TIE_W, TIE_H, TIE_SPP = 96, 64, 16


def tie_camera():
    """A camera that looks at the floor / floor-sphere contact, for TIE_W x TIE_H frames."""
    return make_camera(TIE_W, TIE_H, pos=(0.0, -9.0, -12.0), front=(0.0, -6.0, -8.0), fov=1.2)


# ---------------------------------------------------------------------------------------------------- arbitration by the oracle
_oracle_cache = {}


def oracle(key, fn):
    """One oracle render per configuration for the whole run, shared by the kernel variants and by the suites that render the
    same configuration: test_gpu_bench_configs, test_gpu_scene_matrix, and `arbitrate` below."""
    if key not in _oracle_cache:
        _oracle_cache[key] = fn()
    return _oracle_cache[key]


def check(acc, ref, what, max_diff):
    """The bar of the benchmarked configurations: per-pixel L2 < 1e-3 and at most max_diff differing pixels.
    test_gpu_bench_configs."""
    n_diff = int(np.any(acc != ref, axis=-1).sum())
    err = l2(acc, ref)
    print(f"{what}: L2 {err:.3e}, differing pixels {n_diff} of {acc.shape[0] * acc.shape[1]}")
    assert err < 1e-3, f"{what}: L2 {err:.3e}"
    assert n_diff <= max_diff, f"{what}: {n_diff} differing pixels, more than {max_diff}"


def emitters(mesh, materials, tri_material):
    """orc.tri_lights of a material table with emitters, None without one: the light list PT_FLAG_NEE samples, which both oracle
    renderers need to restate such a call.  `arbitrate` and `judge` below."""
    if materials is None or not any(any(m.emi) for m in materials):
        return None
    return orc.tri_lights(mesh, materials, tri_material)


def arbitrate(pt, mesh, bvh, sph, cam, p, frames, what, max_diff, oracle_key=None, materials=None, tri_material=None):
    """Sample by sample (one pt_render per frame, N = 1) against the oracle's walk over `bvh`; every (frame, pixel) where the
    two differ is replayed with the BRUTE-FORCE closest hit (orc.sample_pixels over the raw triangles: no tree, so no box
    can cull anything) and the GPU must hold brute force's colour.  Returns (differing, of which the oracle's walk was off).
    materials / tri_material: the per-triangle material table on the context, handed to both oracle renderers.
    test_gpu_bench_configs, test_gpu_refit, test_gpu_scene_matrix."""
    mk = dict(materials=materials, tri_material=tri_material, lights=emitters(mesh, materials, tri_material))
    W, H = p.width, p.height
    acc, rgba = pt.alloc_frame(W, H)
    diffs = []
    for f in frames:
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = f, 1
        pt.launch_kernel(acc.ptr, rgba.ptr, cam, q, 1)
        pt.sync()
        got = acc.download(np.float32, (H, W, 3))
        ref = oracle((oracle_key, f), lambda: orc.render(bvh, sph, cam, q, 1, want_rgba=False, **mk)[0]) if oracle_key else \
            orc.render(bvh, sph, cam, q, 1, want_rgba=False, **mk)[0]
        ys, xs = np.nonzero(np.any(got != ref, axis=-1))
        diffs += [(f, int(x), int(y), got[y, x].copy(), ref[y, x].copy()) for x, y in zip(xs, ys)]
    acc.free()
    rgba.free()
    n_oracle_off = 0
    for f, x, y, got, ref in diffs:
        q = g.Params.from_buffer_copy(p)
        q.frame, q.sample_index = f, 1
        col, t_b, id_b = orc.sample_pixels([(x, y)], sph, cam, q, 1, mesh=mesh, **mk)
        _, t_o, id_o = orc.sample_pixels([(x, y)], sph, cam, q, 1, bvh=bvh, **mk)
        brute = orc.fold_samples(col, 1)[0]
        seg = int(np.argmax((t_b[0, 0] != t_o[0, 0]) | (id_b[0, 0] != id_o[0, 0]))) if (np.any(t_b != t_o) or np.any(id_b != id_o)) else -1
        print(f"  {what}: frame {f} pixel ({x},{y}) gpu {got} oracle {ref} brute {brute}; oracle's walk leaves brute force at segment {seg}: "
              f"t {t_o[0, 0, seg] if seg >= 0 else None} id {id_o[0, 0, seg] if seg >= 0 else None} vs t {t_b[0, 0, seg] if seg >= 0 else None} id {id_b[0, 0, seg] if seg >= 0 else None}")
        assert np.array_equal(got, brute), f"{what}: GPU differs from the brute-force arbiter at frame {f} pixel ({x},{y})"
        n_oracle_off += int(not np.array_equal(ref, brute))
    print(f"{what}: {len(diffs)} differing (frame, pixel) pairs of {len(frames) * W * H}, all equal to brute force on the GPU side; "
          f"the oracle's binary walk was the one off in {n_oracle_off}")
    assert len(diffs) <= max_diff, f"{what}: {len(diffs)} differing (frame, pixel) pairs, more than {max_diff}"
    return len(diffs), n_oracle_off


MAX_DIFF = 2   # judge's cap for the wide walks at the suites' sizes: the cap of test_materials.py / test_gpu_build.py
# the stage-split variants of test_gpu_scene_matrix: whichever of them judges a case must hold the frame the first one held
STAGE_SPLIT = ("wavefront", "wavefront-per-lane", "wavefront-unfused")
_wf_frames = {}     # case -> (variant, accumulator, display words) of the first stage-split variant that ran it
n_diff_seen = {}    # variant -> differing pixels seen by judge, all arbitrated


def judge(t, case, got, ref, mesh, sph, cam, p, spp, prev=None, materials=None, tri_material=None):
    """One frame against the oracle's, at the bars of test_gpu_scene_matrix: a variant with t.exact (binary walks) equals the
    oracle bit for bit, accumulator and display words; any other stays under per-pixel L2 1e-3 with at most MAX_DIFF differing
    pixels, each of which must hold the brute-force renderer's colour; and the STAGE_SPLIT variants (by t.name) agree with one
    another bit for bit.  `got`, `ref`: (accumulator, display words) of the same call.  test_gpu_scene_matrix,
    test_gpu_last_anyhit, test_gpu_root_cull."""
    acc, rgba = got
    ref_acc, ref_rgba = ref
    diff = np.any(acc != ref_acc, axis=-1)
    n_diff = int(diff.sum())
    err = l2(acc, ref_acc)
    assert err < 1e-3, f"[{t.name}] {case}: L2 {err:.3e}"
    if t.exact:
        assert n_diff == 0, f"[{t.name}] {case}: {n_diff} pixels differ from the oracle"
        assert np.array_equal(rgba, ref_rgba), f"[{t.name}] {case}: display words differ from the oracle"
    else:
        assert n_diff <= MAX_DIFF, f"[{t.name}] {case}: {n_diff} pixels differ from the oracle"
        assert not np.any((rgba != ref_rgba) & ~diff), f"[{t.name}] {case}: display words differ where the accumulator does not"
        for y, x in zip(*np.nonzero(diff)):
            col, _, _ = orc.sample_pixels([(int(x), int(y))], sph, cam, p, spp, mesh=mesh, materials=materials, tri_material=tri_material,
                                          lights=emitters(mesh, materials, tri_material))
            brute = orc.fold_samples(col, p.sample_index, None if prev is None else prev[y, x][None])[0]
            print(f"  [{t.name}] {case}: pixel ({x},{y}) gpu {acc[y, x]} oracle {ref_acc[y, x]} brute {brute}")
            assert np.array_equal(acc[y, x], brute), f"[{t.name}] {case}: pixel ({x},{y}) is neither the oracle's nor brute force's"
        n_diff_seen[t.name] = n_diff_seen.get(t.name, 0) + n_diff
    if t.name in STAGE_SPLIT:
        first = _wf_frames.setdefault(case, (t.name, acc, rgba))
        assert np.array_equal(acc, first[1]) and np.array_equal(rgba, first[2]), f"[{t.name}] {case}: differs from [{first[0]}]"


# ---------------------------------------------------------------------------------------------------- guide buffers
class Guides:
    """Device guide buffers of one frame (pt_render_aux): test_gpu_denoise, test_gpu_temporal."""

    def __init__(self, t, W, H):
        self.t, self.W, self.H = t, W, H
        self.alb, self.nrm, self.pos = (t.malloc(W * H * 16) for _ in range(3))
        self.ids = t.malloc(W * H * 4)

    def render(self, cam, p, with_ids=True):
        self.t.render_aux(cam, p, self.alb.ptr, self.nrm.ptr, self.pos.ptr, self.ids.ptr if with_ids else None)

    def download(self):
        self.t.sync()
        W, H = self.W, self.H
        return (self.alb.download(np.float32, (H, W, 4)), self.nrm.download(np.float32, (H, W, 4)),
                self.pos.download(np.float32, (H, W, 4)), self.ids.download(np.int32, (H, W)))

    def free(self):
        for b in (self.alb, self.nrm, self.pos, self.ids):
            b.free()


def setup_scene(t, scene, materials):
    """(bvh, spheres, materials, tri_material) of a guide test scene ("room", "cornell_dragon", else cornell_box), installed on
    the context: test_gpu_denoise, test_gpu_temporal, test_gpu_scene_matrix."""
    t.upload_tri_materials(None, None)
    if scene == "room":
        mesh, sph = g.scene_mesh("cornell"), g.reference_spheres()
    elif scene == "cornell_dragon":
        mesh, sph = g.scene_mesh("cornell_dragon"), g.reference_spheres()
    else:
        mesh, sph = g.scene_mesh("cornell_box"), None
    bvh = g.Bvh(mesh)
    t.upload_bvh(bvh)
    t.upload_spheres(sph or [])
    mats = tm = None
    if materials:
        mats, tm = mesh.materials, mesh.tri_material
        t.upload_tri_materials(mats, tm)
    return bvh, sph, mats, tm


def _ordered(x):
    i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulp_distance(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def compare_guides(got, ref, what):
    """pt_render_aux's buffers against denoise_ref.guides: ids equal except at sphere / triangle ties (1e-6 relative in t); albedo
    exact; triangle t exact; positions and normals within 2 ulp.  Returns the largest position / normal ulp distances seen and
    the number of ties.  test_gpu_denoise, test_gpu_scene_matrix."""
    ga, gn, gp, gi = got
    ra, rn, rp, ri, t_tri, t_sph = ref
    tie = (ri != -1) & np.isfinite(t_sph) & (t_tri < 3e38) & (np.abs(t_tri.astype(np.float64) - t_sph) <= 1e-6 * np.abs(t_tri))
    ok = ~tie
    bad = np.argwhere(ok & (gi != ri))
    assert len(bad) == 0, f"{what}: {len(bad)} ids differ, first {bad[:4].tolist()}: {gi[tuple(bad[0])]} vs {ri[tuple(bad[0])]}"
    assert np.array_equal(ga[ok].view(np.int32), ra[ok].view(np.int32)), f"{what}: albedo"
    tri = ok & (ri >= 0)
    assert np.array_equal(gp[tri][:, 3].view(np.int32), rp[tri][:, 3].view(np.int32)), f"{what}: triangle t"
    miss = ok & (ri == -1)
    for b in (ga, gn, gp):
        assert not np.any(b[miss]), f"{what}: a miss must be all zero"
    assert np.array_equal(np.any(gn[..., :3] != 0, -1), gi != -1), f"{what}: miss <=> normal (0, 0, 0)"
    hit = ok & (ri != -1)
    du_p, du_n = int(_ulp_distance(gp[hit], rp[hit]).max(initial=0)), int(_ulp_distance(gn[hit], rn[hit]).max(initial=0))
    assert du_p <= 2 and du_n <= 2, f"{what}: position {du_p} ulp, normal {du_n} ulp"
    return du_p, du_n, int(tie.sum())
