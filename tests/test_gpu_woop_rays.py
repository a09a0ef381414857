"""Woop records (PT_OPT_TRI_TEST 1) on the device, ray by ray against exact geometry: the records in device memory against
tests/woop_ref.py's restatement of emit() and against the triangles' own vertices (tree_audit.audit(woop=True)), and the two
routes that walk them — pt_render_rays and pt_render's persistent kernel — against woop_ref.verdict's acceptable answers on the
ray families of woop_ref (tests/test_woop.py checks the reference itself on the CPU).  At depth 1 with one emissive material row
per triangle a ray's radiance names the triangle it hit; the id is coded in two colour channels.

Printed per family (lines "woop-rays |"): rays, decided share, rays whose answer is a `maybe` triangle, and the cracks — rays
aimed exactly at an edge that two triangles share which come back with neither of them nor anything nearer — next to the same count
for the default Moller-Trumbore records on the same rays.  The crack count is recorded, not asserted."""
import numpy as np
import pytest

import deep_trees as dt
import gpu_pathtracer_amd as g
import orc
import tree_audit as ta
import woop_ref as wr
from gpu_support import bits, soup_mesh
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu

BK = (0.0, 0.0, 0.75)      # apart from every code: a code's blue is 0.25, its red and green are odd multiples of 1 / 512


# ------------------------------------------------------------------------------------------------------------- id <-> colour
def id_table(n):
    """one emissive DIFF row per triangle: emission ((2 (id & 255) + 1) / 512, (2 (id >> 8) + 1) / 512, 1 / 4), exact in binary32 and
    below the accumulator's clamp, so 65536 triangles fit"""
    rows = []
    for k in range(n):
        m = g.Material()
        m.col[:], m.emi[:], m.mat, m.phong_expo = (0.5, 0.5, 0.5), ((2 * (k & 255) + 1) / 512.0, (2 * (k >> 8) + 1) / 512.0, 0.25), g.MAT_DIFF, 0.0
        rows.append(m)
    return rows, np.arange(n, dtype=np.int32)


def decode(rgb, n, what):
    """colours [..., 3] -> ids (-1: the background); anything that is neither a code nor the background fails"""
    rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    miss = np.all(bits(rgb) == bits(np.array(BK, np.float32)), axis=1)
    lo, hi = (rgb[:, 0].astype(np.float64) * 512.0 - 1.0) / 2.0, (rgb[:, 1].astype(np.float64) * 512.0 - 1.0) / 2.0
    code = ~miss & (rgb[:, 2] == 0.25) & (lo == np.round(lo)) & (hi == np.round(hi)) & (lo >= 0) & (lo < 256) & (hi >= 0)
    assert np.all(miss | code), f"{what}: rays {np.nonzero(~(miss | code))[0][:8]} return {rgb[~(miss | code)][:4]}, neither a triangle's code nor the background"
    ids = np.where(miss, -1, (hi * 256 + lo)).astype(np.int64)
    assert ids.max(initial=-1) < n, f"{what}: id {ids.max()} of {n} triangles"
    return ids


# ------------------------------------------------------------------------------------------------------------------ contexts
def context(soup, tri_test=1, leaf_max=None):
    tr = g.PathTracer(0)
    tr.set_option(g.OPT_TRI_TEST, tri_test)
    if leaf_max is not None:
        tr.set_option(g.OPT_LEAF_MAX, leaf_max)
    tr.upload_bvh(g.Bvh(soup_mesh(soup)))
    tr.upload_spheres(None)
    tr.upload_tri_materials(*id_table(len(soup)))
    return tr


def ray_params(cull):
    p = g.default_params(64, 64, depth=1)
    p.frame, p.sample_index, p.cull_backfaces = 7, 1, cull
    p.bk_color[:] = BK
    return p


def ray_ids(tr, rays, cull, hdr, what, n_tris):
    n = len(rays)
    d_r, d_o = tr.malloc(rays.nbytes), tr.malloc(12 * n)
    d_r.upload(np.ascontiguousarray(rays, np.float32))
    d_o.upload(np.full((n, 3), -7.0, np.float32))
    tr.render_rays(d_r.ptr, n, d_o.ptr, ray_params(cull), 1, 0, hdr)
    tr.sync()
    out = d_o.download(np.float32, (n, 3))
    d_r.free()
    d_o.free()
    return decode(out, n_tris, what)


def held(V, ids, what):
    off = np.nonzero(~V.accepts(ids))[0]
    assert len(off) == 0, (f"{what}: rays {off[:8]} answer {ids[off[:8]]}; acceptable "
                           f"{[np.nonzero(V.ok[i])[0].tolist() for i in off[:4]]} (the last column stands for a miss), decided {V.decided[off[:8]]}")


# -------------------------------------------------------------------------------------------------------------------- records
def audit_records(tr, soup, what, leaf_max):
    B, R, W, wd = tr.tree_items()
    stats = {}
    v = ta.audit(B, R, W, tr.scene_info(), soup, wide_depth=wd, woop=True, split_refs=True, leaf_max=leaf_max, stats=stats)
    print(f"woop-records | {what}: {len(R)} records, {stats['woop_floats_differ']} of {stats['woop_floats']} row floats differ from the reference's")
    assert v == [], what + "\n" + "\n".join(f"{x.kind} | {x.item} | {x.what}" for x in v[:12])
    return R


RECORD_MESHES = ("a", "b-bunny_low", "b-cornell", "b-tilted_grid", "e", "f-moved", "f-small", "f-large", "~b-bunny_low", "~b-cornell", "~b-tilted_grid")


@pytest.mark.parametrize("leaf_max", [2, 0])
@pytest.mark.parametrize("name", RECORD_MESHES)
def test_records(name, leaf_max):
    """Every mesh of the families, uploaded with PT_OPT_TRI_TEST 1 and read back through pt_tree_items: the rows map the triangle's
    own vertices to (1,0,0), (0,1,0), (0,0,0) within 2^-24 per entry times the magnitudes summed, every float is within 1 ulp of
    woop_ref.records' (tree_audit.encode_woop_records; the count of floats that are not bit-equal is printed), N is the vcross
    value bit for bit, and the id / last word is right, with the producer's leaves (PT_OPT_LEAF_MAX 0) and split ones (2)."""
    soup = wr.family(name)[0]
    tr = context(soup, leaf_max=leaf_max)
    try:
        R = audit_records(tr, soup, f"{name} leaf_max {leaf_max}", leaf_max)
        # the same records by id, against records(): the function the verdicts are computed from
        want = wr.records(soup)
        ids = R.view(np.int32)[:, 15] >> 1
        assert np.array_equal(bits(R[:, 12:15]), bits(want[ids, 12:15]))
        assert np.all(np.abs(ta._ordered_bits(R[:, :12]) - ta._ordered_bits(want[ids, :12])) <= 1)
    finally:
        tr.close()


def test_empty_leaf_record():
    """A caller's hierarchy with a leaf that holds nothing: its Woop record is zero rows under the word -1 (id -1, last), the rays
    that cross its place hit what lies there or nothing"""
    tri = [[(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (2.0, 2.0, 0.0)], [(4.0, 0.0, 0.5), (6.0, 0.0, 0.5), (6.0, 2.0, 0.5)]]
    big = 3.0e38
    inverted = (np.array([big] * 3), np.array([-big] * 3))
    box = lambda t: (np.min(np.array(tri[t]), 0), np.max(np.array(tri[t]), 0))
    rest = (np.array([4.0, 0.0, 0.5]), np.array([6.0, 2.0, 0.5]))
    fx = dt._finish([(box(0), (0,), rest, 1), (box(1), (1,), inverted, ())], tri, {}, 0.5)
    soup = np.array(tri, np.float32).reshape(-1, 9)
    tr = g.PathTracer(0)
    try:
        tr.set_option(g.OPT_TRI_TEST, 1)
        tr.set_option(g.OPT_LEAF_MAX, 0)
        tr.upload_bvh(fx)
        tr.upload_spheres(None)
        tr.upload_tri_materials(*id_table(2))
        R = audit_records(tr, soup, "empty leaf", 0)
        words = R.view(np.int32)[:, 15]
        assert sorted(words.tolist()) == [-1, 1, 3] and not np.any(R.view(np.int32)[words == -1, :15])
        rays = np.array([[1.5, 0.5, 3, 0, 0, 0, -1, 0], [5.5, 0.5, 3, 0, 0, 0, -1, 0], [3.0, 1.0, 3, 0, 0, 0, -1, 0]], np.float32)
        assert ray_ids(tr, rays, 1, True, "empty leaf", 2).tolist() == [0, 1, -1]
    finally:
        tr.close()


# ------------------------------------------------------------------------------------------------------------- pt_render_rays
def shared_edge_rays(name, soup):
    """(rows, sharers [rows][m] bool, distance) of the rays of an aimed family that are aimed exactly at an edge two or more
    triangles share"""
    A = wr.aim(name)
    v = np.asarray(soup, np.float32).reshape(-1, 3, 3)
    rows, share = [], []
    for i, e in enumerate(A.edge):
        if e is None:
            continue
        p, q = v[A.tri[i], e[0]], v[A.tri[i], e[1]]
        has = lambda x: np.any(np.all(v == x[None, None, :], axis=2), axis=1)
        s = has(p) & has(q)
        if s.sum() >= 2:
            rows.append(i)
            share.append(s)
    return np.array(rows, np.int64), np.array(share, bool).reshape(len(rows), len(v))


def cracks(name, soup, V, ids):
    """(cracks, edge rays): of the rays aimed at an edge that two or more triangles share, with at least two of the sharers not
    excluded for the ray (facing it, or no cull) and nothing certain nearer than the edge, those whose answer is none of the sharers"""
    rows, share = shared_edge_rays(name, soup)
    if len(rows) == 0:
        return 0, 0
    open_ = (share & (V.certain[rows] | V.maybe[rows])).sum(1) >= 2
    open_ &= ~(V.T[rows] < wr.aim(name).dist[rows] * (1.0 - 1e-4))
    through = np.array([a < 0 or not share[k, a] for k, a in enumerate(ids[rows])])
    return int((through & open_).sum()), int(open_.sum())


GPU_FAMILIES = wr.FAMILIES + wr.REVERSED


@pytest.mark.parametrize("name", GPU_FAMILIES)
def test_render_rays(name):
    """pt_render_rays at depth 1 over a family, both cull settings (family d), PT_OPT_WALK 2 and 1 (the option does not choose the
    walk of Woop records) and both hdr settings, schedule knobs at default: every ray's decoded id lies in the verdict's
    acceptable set; family a equals brute force on every ray."""
    soup, rays = wr.family(name)
    tr = context(soup)
    mt = context(soup, tri_test=0)
    try:
        for cull in (1, 0):
            V = wr.family_verdict(name, cull)
            first = None
            for walk in (2, 1):
                tr.set_option(g.OPT_WALK, walk)
                for hdr in (True, False):
                    what = f"{name} cull {cull} walk {walk} hdr {hdr}"
                    ids = ray_ids(tr, rays, cull, hdr, what, len(soup))
                    held(V, ids, what)
                    first = ids if first is None else first
                    assert np.array_equal(ids, first), f"{what}: differs from walk 2, hdr, at rays {np.nonzero(ids != first)[0][:8]}"
            ids, ids_mt = first, ray_ids(mt, rays, cull, True, f"{name} cull {cull} Moller-Trumbore", len(soup))
            if name == "a":
                id_b = orc.trace_brute(wr.mesh_soup("grid")[1], rays, bool(cull))[1]
                assert np.array_equal(ids, id_b), f"family a cull {cull}: rays {np.nonzero(ids != id_b)[0][:8]} leave brute force"
                n_crack, n_crack_mt, n_edge = int(((ids < 0) & (id_b >= 0)).sum()), int(((ids_mt < 0) & (id_b >= 0)).sum()), len(rays)
            elif name.lstrip("~")[0] in "bf":
                (n_crack, n_edge), (n_crack_mt, _) = cracks(name, soup, V, ids), cracks(name, soup, V, ids_mt)
            else:
                n_crack = n_crack_mt = n_edge = 0
            is_maybe = (ids >= 0) & V.maybe[np.arange(len(ids)), np.maximum(ids, 0)]
            print(f"woop-rays | {name} cull {cull} | rays {len(rays)} | decided {V.decided.mean():.4f} | answer is a maybe triangle {int(is_maybe.sum())} | "
                  f"differs from Moller-Trumbore {int((ids != ids_mt).sum())} | edge rays {n_edge}: cracks {n_crack}, Moller-Trumbore {n_crack_mt} | largest du {V.du_max:.3e}")
    finally:
        tr.close()
        mt.close()


# -------------------------------------------------------------------------------------------------- pt_render, persistent kernel
def frame_scene(which):
    """(soup, camera) of a 64 x 48 frame: the dyadic grids, the sliver soup, the bunny far from the origin"""
    W, H = 64, 48
    if which == "grid":
        return wr.family("a")[0], make_camera(W, H, pos=(3.7, 4.3, 6.0), front=(0.05, -0.03, -1.0), fov=0.7)
    if which == "slivers":
        return wr.family("e")[0], make_camera(W, H, pos=(3.2, 2.9, 5.0), front=(0.02, 0.03, -1.0), fov=0.8)
    soup = wr.family("f-moved")[0]
    v = soup.reshape(-1, 3).astype(np.float64)
    c = 0.5 * (v.min(0) + v.max(0))
    return soup, make_camera(W, H, pos=tuple(c + (0.0, 0.5, 14.0)), front=(0.0, -0.03, -1.0), fov=0.7)


_frame_verdicts = {}


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("which", ["grid", "slivers", "moved-bunny"])
def test_persistent_kernel_frame(which, cull):
    """pt_render on the persistent kernel, 64 x 48 at depth 1, PT_OPT_LDS_STACK 16 / 0 x PT_OPT_OCCUPANCY 4 / 8: every pixel's id lies
    in the verdict's set for its primary ray (orc.primary_rays), and the four settings agree bit for bit."""
    W, H = 64, 48
    soup, cam = frame_scene(which)
    p = g.default_params(W, H, depth=1)
    p.frame, p.sample_index, p.cull_backfaces = 11, 1, cull
    p.bk_color[:] = BK
    rays = orc.primary_rays(cam, W, H, frame=11)
    if which not in _frame_verdicts:
        _frame_verdicts[which] = wr.verdicts(soup, rays)
    V = _frame_verdicts[which][cull]
    tr = context(soup)
    try:
        tr.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
        acc, rgba = tr.alloc_frame(W, H)
        first = None
        for lds in (16, 0):
            for occ in (4, 8):
                tr.set_option(g.OPT_LDS_STACK, lds)
                tr.set_option(g.OPT_OCCUPANCY, occ)
                acc.zero()
                tr.launch_kernel(acc.ptr, rgba.ptr, cam, p, 1)
                tr.sync()
                got = acc.download(np.float32, (H, W, 3))
                what = f"{which} cull {cull} lds {lds} occupancy {occ}"
                ids = decode(got, len(soup), what)
                held(V, ids, what)
                first = got if first is None else first
                assert np.array_equal(bits(got), bits(first)), f"{what}: the frame differs from the first setting's"
        acc.free()
        rgba.free()
        hit = ids >= 0
        is_maybe = hit & V.maybe[np.arange(len(ids)), np.maximum(ids, 0)]
        print(f"woop-rays | frame {which} cull {cull} | rays {len(rays)} | decided {V.decided.mean():.4f} | hit {int(hit.sum())} | "
              f"answer is a maybe triangle {int(is_maybe.sum())} | largest du {V.du_max:.3e}")
        assert hit.sum() > W * H // 8, "the camera hardly sees the mesh"
    finally:
        tr.close()
