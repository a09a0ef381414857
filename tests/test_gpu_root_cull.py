"""PT_OPT_ROOT_CULL: a surviving path's new ray that the next walk's first node step — on the 4-wide tree's root, with the h.t the
lane would start with — leaves without a child is classified by the shade lane that made it, packed behind its region's walkers and
kept out of the extend queue (1, default: product launches; 2: instrumented launches too; 0: every survivor is queued).  That walk
would have reported "no triangle", which is what the shade lane writes, so the accumulator and the display words must be the same
bit for bit; with 0 and 1 an instrumented call must count what it always counted, and with 2 it must lack exactly one node visit
per ray it kept out (wave stat "walk_free")."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import COUNTERS, TIE_H, TIE_SPP, TIE_W, bvh_of, dark_table, golden_camera, judge, pipeline_render, same, tie_camera

pytestmark = pytest.mark.gpu


def render(cull, *args, options=(), **kw):
    return pipeline_render(((g.OPT_ROOT_CULL, cull),) + tuple(options), *args, **kw)


@pytest.mark.parametrize("size", [(640, 360), (257, 131)], ids=["640x360", "257x131"])
@pytest.mark.parametrize("spp", [16, 8, 4, 32, 1])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_cull_equals_full_queue(size, spp, depth):
    W, H = size
    a, b = (render(v, "cornell_dragon", W, H, spp, depth=depth) for v in (0, 1))
    same(b, a, f"{W}x{H} spp {spp} depth {depth}")


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("first_walk", [0, 1])
@pytest.mark.parametrize("anyhit", [0, 1])
@pytest.mark.parametrize("depth", [2, 4])
def test_cull_under_every_stage_layout(fuse, first_walk, anyhit, depth):
    """bounce 0's survivors are classified by the fused packet launch or by k_wf_shade<FIRST> behind either walk; with
    PT_OPT_LAST_ANYHIT the survivors of bounce depth - 2 against their sphere bound"""
    opts = ((g.OPT_FUSE_STAGES, fuse), (g.OPT_FIRST_WALK, first_walk), (g.OPT_LAST_ANYHIT, anyhit))
    a, b = (render(v, "cornell_dragon", 257, 131, 16, depth=depth, options=opts) for v in (0, 1))
    same(b, a, f"fuse {fuse} first walk {first_walk} any-hit {anyhit} depth {depth}")


@pytest.mark.parametrize("depth", [2, 4])
def test_cull_tile_split_parts(depth):
    a, b = (render(v, "cornell_dragon", 257, 131, 16, depth=depth, parts=3) for v in (0, 1))
    same(b, a, f"3 parts, depth {depth}")
    whole = render(1, "cornell_dragon", 257, 131, 16, depth=depth)
    same(b, whole, f"3 parts against the whole frame, depth {depth}")


@pytest.mark.parametrize("spp", [16, 8])
def test_cull_running_mean(spp):
    """sample_index 5 over a pre-filled accumulator, then a second call on top"""
    a, b = (render(v, "cornell_dragon", 257, 131, spp, calls=2, prefill=True) for v in (0, 1))
    same(b, a, f"running mean, spp {spp}")


@pytest.mark.parametrize("flags", [0, g.FLAG_MISS_KEEPS_PATH], ids=["plain", "miss-keeps-path"])
@pytest.mark.parametrize("depth", [2, 4])
def test_cull_open_scene(flags, depth):
    """no spheres: a ray that misses the root misses everything and takes the background rule in the next shade launch"""
    a, b = (render(v, "cornell", 320, 180, 16, depth=depth, flags=flags, spheres=False) for v in (0, 1))
    same(b, a, f"open scene, flags {flags}, depth {depth}")


def test_cull_miss_keeps_path():
    a, b = (render(v, "cornell_dragon", 320, 180, 16, flags=g.FLAG_MISS_KEEPS_PATH) for v in (0, 1))
    same(b, a, "PT_FLAG_MISS_KEEPS_PATH")


OTHER_PACKINGS = {
    "nee": dict(flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF),   # the survivors are classified, the shadow records are all walked
    "material-table": dict(table=dark_table),
    "metal": dict(tri_mat=g.MAT_METAL),
    "specular": dict(tri_mat=g.MAT_SPEC),
}


@pytest.mark.parametrize("case", list(OTHER_PACKINGS))
def test_cull_with_nee_and_materials(case):
    kw = OTHER_PACKINGS[case]
    a, b = (render(v, "cornell_dragon", 257, 131, 16, **kw) for v in (0, 1))
    same(b, a, case)
    c0, c2 = (render(v, "cornell_dragon", 257, 131, 16, counters=True, **kw) for v in (0, 2))
    same(c2, c0, f"{case}, instrumented")
    assert c2[2]["rays"] == c0[2]["rays"] and c2[2]["walk_free"] > 0
    assert c2[2]["inner"] == c0[2]["inner"] - c2[2]["walk_free"]


@pytest.mark.parametrize("anyhit", [0, 2])
@pytest.mark.parametrize("depth", [2, 4])
def test_counters(anyhit, depth):
    """0 and 1: an instrumented call counts the full queue, exactly.  2: the same rays, hits and paths — the shade stage still sees
    every segment — the same records and leaves, and one node visit less per ray kept out: the root visit of the walk the
    classification replaces (closest hit, and with PT_OPT_LAST_ANYHIT 2 the any-hit walk of the last segment)."""
    opts = ((g.OPT_LAST_ANYHIT, anyhit),)
    c0, c1, c2 = (render(v, "cornell_dragon", 320, 180, 16, depth=depth, counters=True, options=opts) for v in (0, 1, 2))
    same(c1, c0, "instrumented, 1")
    same(c2, c0, "instrumented, 2")
    k0, k1, k2 = c0[2], c1[2], c2[2]
    for k in COUNTERS + ("act_shade", "walk_free"):
        assert k1[k] == k0[k], k
    assert k0["walk_free"] == 0
    assert k0["rays"] == 320 * 180 * 16 * depth   # the closed room: every path runs its `depth` segments
    print(f"any-hit {anyhit} depth {depth}: rays {k2['rays']}, walk-free {k2['walk_free']}, inner {k0['inner']} -> {k2['inner']}")
    assert 0 < k2["walk_free"] < k2["rays"]
    for k in ("rays", "tris", "leaves", "hits", "paths"):
        assert k2[k] == k0[k], k
    assert k2["inner"] == k0["inner"] - k2["walk_free"]
    if anyhit == 2:   # "act_shade": the rays the any-hit launch walked
        assert k2["act_shade"] <= k0["act_shade"]


# ---- rays in or next to the planes of the mesh's bounds.  A camera whose `right` (or `up`) is the zero vector sends every ray of
# the frame through one plane x = const (y = const) with that direction component exactly 0 — trav_ray's ooeps case, the last ray of
# test_edge_case_rays — and mirror triangles keep it there over the bounces; diffuse ones add directions at every angle to the plane,
# grazing ones included, from vertices in it.
def plane_camera(W, H, axis, coord, z, flat):
    """a camera at `coord` on `axis` (0: x, 1: y); flat: the basis vector along that axis is zero, so the whole frame lies in the plane"""
    cam = golden_camera(W, H)
    cam.pos[:] = [np.float32(coord) if axis == 0 else np.float32(2.0), np.float32(coord) if axis == 1 else np.float32(-3.0), np.float32(z)]
    cam.front[:] = [0.0, 0.0, -1.0]
    cam.right[:] = [0.0, 0.0, 0.0] if flat and axis == 0 else [1.0, 0.0, 0.0]
    cam.up[:] = [0.0, 0.0, 0.0] if flat and axis == 1 else [0.0, 1.0, 0.0]
    return cam


def ulps(x, n):
    x = np.float32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.float32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return x


GW, GH, GSPP = 64, 48, 8
PLANES = dict(argnames="axis,side", argvalues=[(0, 0), (0, 1), (1, 0), (1, 1)], ids=["x-lo", "x-hi", "y-lo", "y-hi"])


@pytest.mark.parametrize("tri_mat", [g.MAT_DIFF, g.MAT_SPEC], ids=["diffuse", "mirror"])
@pytest.mark.parametrize(**PLANES)
def test_rays_in_the_bounding_planes(axis, side, tri_mat):
    """every ray of the frame in, or 1 / 3 ulps beside, a plane of the mesh's bounds: the frame with the option on is the frame
    with it off, also against the sphere bound of PT_OPT_LAST_ANYHIT"""
    mesh, _ = bvh_of("cornell_dragon")
    bound = mesh.bounds()[side][axis]
    for n in (0, 1, -1, 3, -3):
        for z in (0.0, -40.0):   # from the room in front of the mesh, and from between its walls
            cam = plane_camera(GW, GH, axis, ulps(bound, n), z, flat=True)
            for anyhit in (0, 1):
                opts = ((g.OPT_LAST_ANYHIT, anyhit),)
                a, b = (render(v, "cornell_dragon", GW, GH, GSPP, cam=cam, tri_mat=tri_mat, options=opts) for v in (0, 1))
                same(b, a, f"plane {'xy'[axis]} = {bound} {n:+d} ulps, camera z {z}, material {tri_mat}, any-hit {anyhit}")


@pytest.mark.parametrize("tri_mat", [g.MAT_DIFF, g.MAT_SPEC], ids=["diffuse", "mirror"])
@pytest.mark.parametrize(**PLANES)
def test_camera_in_a_bounding_plane_against_the_oracle(axis, side, tri_mat):
    """The oracle walks the binary tree, whose exact root box drops a ray that lies IN one of its faces with a zero direction
    component (the slab test is not watertight: test_edge_case_rays, tests/test_oracle.py), while the wide root is rounded outward
    and keeps it — with the option on or off.  A frame made of nothing but such rays is therefore not what the wide walk's bars
    (gpu_support.judge) were set for; they are set for frames in which a grazing ray is the exception.  So this
    comparison takes an ordinary camera basis with the camera IN the plane (or 1 / 3 ulps beside it): every camera ray starts on
    the face of the root box, half of them leave it at once, the frame's middle column (row) runs along it."""
    mesh, bvh = bvh_of("cornell_dragon")
    bound = mesh.bounds()[side][axis]
    sph = g.reference_spheres()

    class T:
        name, exact = "wavefront-root-cull", False
    for n in (0, 1, -3):
        for z in (0.0, -40.0):
            cam = plane_camera(GW, GH, axis, ulps(bound, n), z, flat=False)
            what = f"camera at {'xy'[axis]} = {bound} {n:+d} ulps, z {z}, material {tri_mat}"
            a, b = (render(v, "cornell_dragon", GW, GH, GSPP, cam=cam, tri_mat=tri_mat) for v in (0, 1))
            same(b, a, what)
            p = g.default_params(GW, GH, depth=4, tri_mat=tri_mat)
            p.frame, p.sample_index, p.flags = 7, 1, g.FLAG_WRITE_RGBA
            ref = orc.render(bvh, sph, cam, p, GSPP)[:2]
            print(f"{what}: {int(np.any(b[0] != ref[0], axis=-1).sum())} pixels differ from the oracle")
            judge(T, what, b[:2], ref, mesh, sph, cam, p, GSPP)


@pytest.mark.parametrize("depth", [2, 4])
def test_floor_sphere_contact(depth):
    """the floor (the plane y = lo of the bounds) touches the floor sphere: vertices in the plane from both kinds of surface"""
    cam = tie_camera()
    a, b = (render(v, "cornell_dragon", TIE_W, TIE_H, TIE_SPP, depth=depth, cam=cam) for v in (0, 1))
    same(b, a, f"floor / sphere contact, depth {depth}")


def test_context_without_a_tree():
    """spheres only: the call runs the persistent kernel (the pipeline needs the wide tree) and nothing is classified"""
    a, b = (render(v, None, 257, 131, 16) for v in (0, 1))
    same(b, a, "no tree")
    c0, c2 = (render(v, None, 257, 131, 4, counters=True) for v in (0, 2))
    same(c2, c0, "no tree, instrumented")
    for k in COUNTERS:
        assert c2[2][k] == c0[2][k], k
    assert c2[2]["walk_free"] == 0


def test_root_cull_option_values():
    t = g.PathTracer(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.PtError):
                t.set_option(g.OPT_ROOT_CULL, bad)
        for ok in (0, 2, 1):
            t.set_option(g.OPT_ROOT_CULL, ok)
    finally:
        t.close()
