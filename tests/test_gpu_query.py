"""pt_closest_hits / pt_any_hits — bounded closest-hit and any-hit queries on a caller's rays (extension, DESIGN.md §10 f9;
csrc/pt_k_query.hip).

Every answer has an exact reference: brute force filtered by the bound (tests/query_ref.py, whose inputs tests/test_query.py checks
on the CPU).  The records and the triangle arithmetic are pt_trace_rays', so t, id and normal are compared bit for bit; the 4-wide
tree's quantised boxes are not the binary tree's, so on the mesh scenes at most gpu_support.MAX_DIFF grazing rays per case may
differ, each printed.  The hand-built deep trees (tests/deep_trees.py) allow none."""
import math

import numpy as np
import pytest

import deep_trees as dt
import gpu_pathtracer_amd as g
import orc
import query_ref as qr
from gpu_support import MAX_DIFF, bits, cornell_dragon_moved, golden_camera, gpu_trace, rays_for, setup_scene, soup_mesh

pytestmark = pytest.mark.gpu

N, SEED = 20000, 5
PAD = 64
PT_OK, PT_ERR_INVALID, PT_ERR_NO_SCENE, PT_ERR_UNSUPPORTED = 0, -1, -3, -5
PT_STACK_CAP = 72
SCENES = ("cornell", "bunny_low", "gto_sixteen")
TREES = ("host", "device", "optimize")
T_FILL, I_FILL, N_FILL, B_FILL = np.float32(-7.5), np.int32(-77), np.float32(-3.25), np.uint8(0xA5)


# ------------------------------------------------------------------------------------------------ contexts, launches
_ctx = {}


def context(name, tree):
    """one context per (scene, tree kind), kept until the module is done"""
    if (name, tree) not in _ctx:
        mesh = g.scene_mesh(name)
        t = g.PathTracer(0)
        if tree == "device":
            t.build_bvh(mesh)
        else:
            t.set_option(g.OPT_OPTIMIZE, 1 if tree == "optimize" else 0)
            t.upload_bvh(g.Bvh(mesh))
            t.set_option(g.OPT_OPTIMIZE, 0)
        _ctx[(name, tree)] = t
    return _ctx[(name, tree)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for t in _ctx.values():
        t.close()
    _ctx.clear()


class Buffers:
    """the device side of a batch: the rays, and outputs PAD elements longer than the batch, pre-filled with a pattern"""

    def __init__(self, t, rays):
        self.t, self.n = t, len(rays)
        m = self.n + PAD
        self.rays = t.malloc(max(rays.nbytes, 32))
        if self.n:
            self.rays.upload(rays)
        self.d_t, self.d_i, self.d_n, self.d_b = t.malloc(4 * m), t.malloc(4 * m), t.malloc(12 * m), t.malloc(m)
        self.d_t.upload(np.full(m, T_FILL, np.float32))
        self.d_i.upload(np.full(m, I_FILL, np.int32))
        self.d_n.upload(np.full((m, 3), N_FILL, np.float32))
        self.d_b.upload(np.full(m, B_FILL, np.uint8))

    def closest(self, cull, normal=True):
        self.t.closest_hits(self.rays.ptr, self.n, cull, self.d_t.ptr, self.d_i.ptr, self.d_n.ptr if normal else None)

    def any(self, cull):
        self.t.any_hits(self.rays.ptr, self.n, cull, self.d_b.ptr)

    def download(self):
        """(t, id, normal, bytes) of the batch after a sync; the padding of all four must still hold the pattern"""
        self.t.sync()
        n, m = self.n, self.n + PAD
        t, i = self.d_t.download(np.float32, (m,)), self.d_i.download(np.int32, (m,))
        nr, b = self.d_n.download(np.float32, (m, 3)), self.d_b.download(np.uint8, (m,))
        assert np.all(t[n:] == T_FILL) and np.all(i[n:] == I_FILL) and np.all(nr[n:] == N_FILL) and np.all(b[n:] == B_FILL), \
            "a query wrote past the end of its outputs"
        return t[:n], i[:n], nr[:n], b[:n]

    def free(self):
        for b in (self.rays, self.d_t, self.d_i, self.d_n, self.d_b):
            b.free()


def query(t, rays, cull):
    """both calls over host rays: (t, id, normal, bytes)"""
    buf = Buffers(t, rays)
    try:
        buf.closest(cull)
        buf.any(cull)
        return buf.download()
    finally:
        buf.free()


def compare(what, got, ref, rays, cap):
    """t (bits), id, normal and the any-hit bytes against the reference; every differing ray is printed with its t, the count
    always, and at most `cap` rays may differ.  Every byte is 0 or 1."""
    gt, gi, gn, gb = got
    rt, ri, rn, ra = ref
    assert np.all(gb <= 1), f"{what}: a byte that is neither 0 nor 1"
    off_c = (bits(gt) != bits(rt)) | (gi != ri) | np.any(gn != rn, axis=1)
    off_a = (gb != 0) != np.asarray(ra, bool)
    for k in np.nonzero(off_c | off_a)[0]:
        print(f"  {what}: ray {k} t_max {rays[k, 7]!r}: closest t {gt[k]!r} id {gi[k]} normal {gn[k]}, reference t {rt[k]!r} id {ri[k]} normal {rn[k]}; "
              f"any {gb[k]}, reference {int(ra[k])}")
    n_c, n_a = int(off_c.sum()), int(off_a.sum())
    print(f"{what}: {n_c} closest and {n_a} any-hit answers of {len(rays)} differ from the reference")
    assert n_c <= cap, f"{what}: {n_c} closest-hit answers differ from the reference, more than {cap}"
    assert n_a <= cap, f"{what}: {n_a} any-hit answers differ from the reference, more than {cap}"


# ------------------------------------------------------------------------------------------------ 1. against brute force, with bounds
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name", SCENES)
def test_bounded_queries_equal_brute_force(name, tree, cull):
    """20 000 rays with the eight bound classes: t (bits), id, normal and the any-hit bytes equal brute force filtered by the bound,
    at most MAX_DIFF rays apart.
    MEASURED ON THE MI355X: 0 differing rays in all eighteen cases.  (Without the widened box tests of query_widen_boxes the six
    cornell cases lost 29 to 156 class-2 rays, t_max = the next float above t, on walls that lie on the faces of their boxes.)"""
    mesh, rays, cls, b, ref = qr.case(name, N, SEED, cull)
    hit, occ, bad = qr.shares(cls, b[1], ref[3])
    assert not bad, bad
    assert hit > 0.5 and 0.15 <= occ <= 0.5, (hit, occ)       # both answers are exercised
    compare(f"{name} {tree} cull {cull}", query(context(name, tree), rays, cull), ref, rays, MAX_DIFF)


# ------------------------------------------------------------------------------------------------ 2. unbounded = pt_trace_rays
@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", SCENES)
def test_unbounded_closest_equals_trace_rays(name, cull):
    mesh, rays, cls, b, _ = qr.case(name, N, SEED, cull)
    t = context(name, "host")
    tt, ti, tn = gpu_trace(t, rays, cull)
    tn = np.where((ti >= 0)[:, None], tn, np.float32(0))
    for t_max in (np.float32(np.inf), qr.FLT_MAX):
        r = qr.with_bounds(rays, t_max)
        compare(f"{name} cull {cull} t_max {t_max!r} against pt_trace_rays", query(t, r, cull), (tt, ti, tn, ti >= 0), r, MAX_DIFF)


# ------------------------------------------------------------------------------------------------ 3. sizes and edges of the refill
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, N])
def test_batch_sizes(n):
    mesh, rays, cls, b, ref = qr.case("bunny_low", N, SEED, True)
    got = query(context("bunny_low", "host"), rays[:n], True)       # (download checks the padding)
    compare(f"bunny_low n {n}", got, tuple(x[:n] for x in ref), rays[:n], MAX_DIFF)
    if n >= 63:
        assert got[3].any() and not got[3].all()


def test_empty_batch_writes_nothing():
    t = context("bunny_low", "host")
    lib = g._abi.ptmi()
    buf = Buffers(t, np.zeros((0, 8), np.float32))
    try:
        assert lib.pt_closest_hits(t._ctx, buf.rays.ptr, 0, 1, buf.d_t.ptr, buf.d_i.ptr, buf.d_n.ptr) == PT_OK
        assert lib.pt_any_hits(t._ctx, buf.rays.ptr, 0, 1, buf.d_b.ptr) == PT_OK
        assert lib.pt_closest_hits(t._ctx, None, 0, 1, None, None, None) == PT_OK and lib.pt_any_hits(t._ctx, None, 0, 1, None) == PT_OK
        buf.download()
    finally:
        buf.free()


@pytest.mark.parametrize("n", [1, 300])
def test_rays_that_are_never_live(n):
    """every ray has t_max = 0: all misses, written where the rays are drawn, with an empty walk"""
    mesh, rays, *_ = qr.case("bunny_low", N, SEED, True)
    r = qr.with_bounds(rays[:n], np.float32(0))
    gt, gi, gn, gb = query(context("bunny_low", "host"), r, True)
    assert np.all(gt == qr.FLT_MAX) and np.all(gi == -1) and not gn.any() and not gb.any()


def test_back_to_back_calls_need_no_host_sync():
    mesh, rays, cls, b, ref = qr.case("bunny_low", N, SEED, True)
    t = context("bunny_low", "host")
    parts = (rays[:5000], rays[5000:5257], rays[7000:])

    def run(sync):
        bufs = [Buffers(t, r) for r in parts]
        try:
            for buf in bufs:
                buf.closest(True, normal=buf is not bufs[1])
                if sync:
                    t.sync()
                buf.any(True)
                if sync:
                    t.sync()
            return [buf.download() for buf in bufs]
        finally:
            for buf in bufs:
                buf.free()

    a, s = run(False), run(True)
    for k, (x, y) in enumerate(zip(a, s)):
        assert all(np.array_equal(bits(u) if u.dtype == np.float32 else u, bits(v) if v.dtype == np.float32 else v) for u, v in zip(x, y)), k
    assert np.all(a[1][2] == N_FILL)                             # no normal asked for: the buffer is left alone
    assert a[0][3].any() and a[2][3].any()


# ------------------------------------------------------------------------------------------------ 4. the stack at full depth
DEEP = [f"comb-{D}" for D in (15, 16, 17, 23, 24, 25, 33, 63, 65)] + ["stair-23", "stair-24"]
_deep = {}


def deep_scene(name):
    if name not in _deep:
        kind, n = name.split("-")
        fx = dt.stair(int(n)) if kind == "stair" else dt.comb(int(n))
        t = g.PathTracer(0)
        t.upload_bvh(fx)
        _deep[name] = (fx, t)
    return _deep[name]


@pytest.fixture(scope="module", autouse=True)
def _close_deep():
    yield
    for _, t in _deep.values():
        t.close()
    _deep.clear()


@pytest.mark.parametrize("lstk", [16, 24])
@pytest.mark.parametrize("name", DEEP)
def test_deep_trees_exact(name, lstk):
    """comb(D) fills the stack to depth D three entries at a time, stair(23) pushes three entries at each of 23 levels; stair(24) is
    the tree the wide walk cannot take, so both calls run the binary walk and apply the bound.  Every answer equals brute force."""
    fx, t = deep_scene(name)
    kind, n = name.split("-")
    wide_depth = t.tree_items()[3]
    assert wide_depth == fx.wide_depth == (int(n) if kind == "stair" else math.ceil(int(n) / 3))
    assert (3 * wide_depth + 2 > PT_STACK_CAP) == (name == "stair-24")
    t.set_option(g.OPT_LDS_STACK, lstk)
    rays = dt.cell_rays(fx)
    diag = qr.diagonal(fx.mesh)
    for cull in (True, False):
        b = orc.trace_brute(fx.mesh, rays, cull)
        assert np.array_equal(b[1], dt.expected_ids(fx, rays)) and (b[1] >= 0).sum() == len(fx.targets)
        base = np.where(b[1] >= 0, b[0], diag).astype(np.float32)
        for cls, t_max in ((2, np.nextafter(base, np.float32(np.inf))), (1, base)):
            r = qr.with_bounds(rays, t_max)
            ref = qr.filter_by_bound(b, t_max)
            assert np.array_equal(ref[3], (b[1] >= 0) if cls == 2 else np.zeros(len(rays), bool))
            compare(f"{name} lstk {lstk} cull {cull} class {cls}", query(t, r, cull), ref, r, 0)


# ------------------------------------------------------------------------------------------------ 5. after a refit
def test_queries_after_refit():
    """cornell_dragon's dragon turned and moved by pt_refit_bvh, 6 000 rays with the eight classes against brute force on the moved mesh.
    MEASURED ON THE MI355X: 0 differing rays (17 class-2 rays on the box's walls before the box tests were widened)."""
    mesh, soup, moved = cornell_dragon_moved()
    moved_mesh = soup_mesh(moved)
    t = g.PathTracer(0)
    try:
        t.build_bvh(mesh)
        t.refit_bvh(moved)
        rays = rays_for(moved, 6000, 5)
        b = orc.trace_brute(moved_mesh, rays, True)
        t_max, cls = qr.class_bounds(b[0], qr.diagonal(moved_mesh))
        r = qr.with_bounds(rays, t_max)
        ref = qr.filter_by_bound(b, t_max)
        assert ref[3].mean() > 0.1
        compare("cornell_dragon moved by pt_refit_bvh", query(t, r, True), ref, r, MAX_DIFF)
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 6. torch tensors
def test_torch_tensors_on_torchs_stream():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch reports no device")
    mesh, rays, cls, b, ref = qr.case("bunny_low", N, SEED, True)
    t = g.PathTracer(0)
    before = torch.cuda.current_stream()
    try:
        t.upload_bvh(g.Bvh(mesh))
        plain = query(t, rays, True)
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)
        assert stream.cuda_stream != 0
        t.set_stream(stream.cuda_stream)
        d_r = torch.from_numpy(rays).to(dev)
        d_t = torch.empty(N, dtype=torch.float32, device=dev)
        d_i = torch.empty(N, dtype=torch.int32, device=dev)
        d_n = torch.empty((N, 3), dtype=torch.float32, device=dev)
        d_b = torch.ones(N + PAD, dtype=torch.bool, device=dev)
        t.closest_hits(d_r.data_ptr(), N, True, d_t.data_ptr(), d_i.data_ptr(), d_n.data_ptr())
        t.any_hits(d_r.data_ptr(), N, True, d_b.data_ptr())
        n_occ = int(d_b[:N].sum().item())                      # torch's own kernel, ordered behind the query on the shared stream
        got = (d_t.cpu().numpy(), d_i.cpu().numpy(), d_n.cpu().numpy(), d_b.cpu().numpy())
        assert got[3][N:].all()
        assert n_occ == int(plain[3].sum())
        assert np.array_equal(bits(got[0]), bits(plain[0])) and np.array_equal(got[1], plain[1])
        assert np.array_equal(bits(got[2]), bits(plain[2])) and np.array_equal(got[3][:N], plain[3] != 0)
        compare("bunny_low through torch tensors", plain, ref, rays, MAX_DIFF)
        stream.synchronize()
    finally:
        torch.cuda.set_stream(before)
        t.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors_in_order():
    lib = g._abi.ptmi()
    t = g.PathTracer(0)
    try:
        buf = t.malloc(4096)
        p = buf.ptr

        def closest(ctx, rays=p, n=4, t_=p, tri=p, nrm=p):
            return lib.pt_closest_hits(ctx, rays, n, 1, t_, tri, nrm)

        def any_(ctx, rays=p, n=4, hit=p):
            return lib.pt_any_hits(ctx, rays, n, 1, hit)

        def named(who):
            return lib.pt_last_error(t._ctx).startswith(who)

        # a NULL context, whatever else is wrong
        assert closest(None, None, 1 << 32, None, None) == PT_ERR_INVALID and b"null ctx" in lib.pt_last_error(None)
        assert any_(None, None, 1 << 32, None) == PT_ERR_INVALID and b"null ctx" in lib.pt_last_error(None)
        # no tree: before the empty batch and before the pointers
        assert closest(t._ctx, None, 0, None, None) == PT_ERR_NO_SCENE and named(b"pt_closest_hits")
        assert any_(t._ctx, None, 0, None) == PT_ERR_NO_SCENE and named(b"pt_any_hits")
        # Woop records: before the empty batch and before the pointers
        mesh = g.scene_mesh("cornell")
        t.set_option(g.OPT_TRI_TEST, 1)
        t.upload_bvh(g.Bvh(mesh))
        t.set_option(g.OPT_TRI_TEST, 0)
        assert closest(t._ctx, None, 0, None, None) == PT_ERR_UNSUPPORTED and named(b"pt_closest_hits")
        assert any_(t._ctx, None, 0, None) == PT_ERR_UNSUPPORTED and named(b"pt_any_hits")
        t.upload_bvh(g.Bvh(mesh))
        # an empty batch is fine, whatever the pointers
        assert closest(t._ctx, None, 0, None, None, None) == PT_OK and any_(t._ctx, None, 0, None) == PT_OK
        # NULL pointers (the normal buffer may be NULL), before the size
        for n in (4, 1 << 32):
            assert closest(t._ctx, rays=None, n=n) == PT_ERR_INVALID and named(b"pt_closest_hits")
            assert closest(t._ctx, t_=None, n=n) == PT_ERR_INVALID and named(b"pt_closest_hits")
            assert closest(t._ctx, tri=None, n=n) == PT_ERR_INVALID and named(b"pt_closest_hits")
            assert any_(t._ctx, rays=None, n=n) == PT_ERR_INVALID and named(b"pt_any_hits")
            assert any_(t._ctx, hit=None, n=n) == PT_ERR_INVALID and named(b"pt_any_hits")
        # 2^32 rays or more (nothing is launched)
        for n in (1 << 32, (1 << 32) + 5, 1 << 40):
            assert closest(t._ctx, n=n) == PT_ERR_INVALID and named(b"pt_closest_hits")
            assert any_(t._ctx, n=n) == PT_ERR_INVALID and named(b"pt_any_hits")
        buf.zero()
        assert closest(t._ctx, n=4, t_=p + 1024, tri=p + 2048, nrm=None) == PT_OK and any_(t._ctx, n=4, hit=p + 3072) == PT_OK
        t.sync()
        buf.free()
        # the context still renders correctly
        W, H = 64, 64
        bvh, sph, _, _ = setup_scene(t, "room", False)
        cam, pr = golden_camera(W, H), g.default_params(W, H)
        acc, rg = t.alloc_frame(W, H)
        t.launch_kernel(acc.ptr, rg.ptr, cam, pr, 2)
        t.sync()
        ref, _, _ = orc.render(bvh, sph, cam, pr, spp=2)
        assert np.array_equal(acc.download(np.float32, (H, W, 3)), ref)
        acc.free()
        rg.free()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 8. no trace in pt_render
def test_queries_leave_no_trace_in_render():
    W, H = 257, 131
    t = g.PathTracer(0)
    try:
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
        mesh, rays, cls, b, ref = qr.case("cornell", N, SEED, True)      # the room's mesh
        # the answers at every setting are compared, not looked at: both range ends of the two schedule knobs of the refill
        # loop of k_query_rays, each stack window, against brute force filtered by the bound (as the parity tests above)
        for lstk, batch, blocks in ((16, 16, 8), (24, 5, 8), (16, 64, 8), (16, 1, 8), (24, 1, 1), (16, 64, 1), (16, 16, 1)):
            t.set_option(g.OPT_LDS_STACK, lstk)
            t.set_option(g.OPT_WAVE_BATCH, batch)
            t.set_option(g.OPT_WAVE_BLOCKS, blocks)
            got = query(t, rays, True)
            compare(f"room, PT_OPT_LDS_STACK {lstk} PT_OPT_WAVE_BATCH {batch} PT_OPT_WAVE_BLOCKS {blocks}", got, ref, rays, MAX_DIFF)
            assert got[3].any() and not got[3].all()
        t.set_option(g.OPT_LDS_STACK, 16)
        t.set_option(g.OPT_WAVE_BATCH, 16)
        t.set_option(g.OPT_WAVE_BLOCKS, 8)
        after = frame(t)
        clean = g.PathTracer(0)
        try:
            clean.upload_bvh(bvh)
            clean.upload_spheres(sph)
            fresh = frame(clean)
        finally:
            clean.close()
        for a in (before, after):
            assert np.array_equal(bits(a[0]), bits(fresh[0])) and np.array_equal(a[1], fresh[1])
        assert fresh[0].any()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------------ 9. timing
def test_timing_covers_the_call():
    mesh, rays, *_ = qr.case("bunny_low", N, SEED, True)
    t = context("bunny_low", "host")
    buf = Buffers(t, rays)
    t.set_option(g.OPT_TIMING, 1)
    try:
        buf.closest(True)
        ms_c = t.last_kernel_ms()
        buf.any(True)
        ms_a = t.last_kernel_ms()
        print(f"{N} rays on bunny_low: pt_closest_hits {ms_c:.3f} ms, pt_any_hits {ms_a:.3f} ms")
        assert 0 < ms_c < 5.0 and 0 < ms_a < 5.0
        buf.download()
    finally:
        t.set_option(g.OPT_TIMING, 0)
        buf.free()
