"""PT_OPT_LAST_ANYHIT: when no triangle can emit, the stage-split pipeline walks a path's last segment as an any-hit query bounded
by the segment's nearest sphere hit (1, default; 2 = instrumented launches too) instead of finding the closest triangle (0).  The
picture only needs to know whether a triangle lies at or before the sphere, so the accumulator and the display words must be the
same bit for bit, calls that are not eligible must not run the any-hit launch at all (wave stat "act_shade" counts its rays), and
where it runs it must visit fewer items."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from scene_matrix import make_camera, red_copies_table
from test_gpu_parity import golden_camera, bvh_of
from test_gpu_scene_matrix import judge

pytestmark = pytest.mark.gpu


def render(anyhit, scene, W, H, spp, depth=4, flags=0, spheres=True, calls=1, prefill=False, counters=False, options=(), cam=None,
           tri_emi=(0, 0, 0), table=None, parts=1, before_upload=()):
    """accumulator + display words after `calls` pt_render calls of the stage-split pipeline with PT_OPT_LAST_ANYHIT = anyhit; with
    prefill the accumulator starts as a fixed frame and the first call's sample_index is 5; parts > 1 renders every call as that
    many tile-split parts of 8 rows"""
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.set_option(g.OPT_LAST_ANYHIT, anyhit)
        for o, v in tuple(options) + tuple(before_upload):
            t.set_option(o, v)
        if counters:
            t.set_option(g.OPT_COUNTERS, 1)
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
                p = g.default_params(W, H)
                p.flags = flags | g.FLAG_WRITE_RGBA
                p.depth = depth
                p.tri_emi[:] = tri_emi
                p.frame, p.sample_index = 7 + call * spp, first + call * spp
                if parts > 1:
                    p.part_index, p.part_count, p.part_rows = part, parts, 8
                t.launch_kernel(acc.ptr, rgba.ptr, cam, p, spp)
                if counters:   # (the counters are those of the last launch: add the parts up)
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
    assert np.array_equal(a[0], b[0]), f"{what}: accumulator differs"
    assert np.array_equal(a[1], b[1]), f"{what}: display words differ"
    assert a[0].any(), what


@pytest.mark.parametrize("size", [(640, 360), (257, 131)], ids=["640x360", "257x131"])
@pytest.mark.parametrize("spp", [16, 8, 4, 32, 1])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_anyhit_equals_closest(size, spp, depth):
    W, H = size
    a, b = (render(v, "cornell_dragon", W, H, spp, depth=depth) for v in (0, 1))
    same(b, a, f"{W}x{H} spp {spp} depth {depth}")


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("first_walk", [0, 1])
@pytest.mark.parametrize("depth", [2, 4])
def test_anyhit_under_every_stage_layout(fuse, first_walk, depth):
    """depth 2: the bound comes from bounce 0's shade — the fused packet launch, k_wf_shade<FIRST> behind either walk"""
    opts = ((g.OPT_FUSE_STAGES, fuse), (g.OPT_FIRST_WALK, first_walk))
    a, b = (render(v, "cornell_dragon", 257, 131, 16, depth=depth, options=opts) for v in (0, 1))
    same(b, a, f"fuse {fuse} first walk {first_walk} depth {depth}")


@pytest.mark.parametrize("depth", [2, 4])
def test_anyhit_tile_split_parts(depth):
    a, b = (render(v, "cornell_dragon", 257, 131, 16, depth=depth, parts=3) for v in (0, 1))
    same(b, a, f"3 parts, depth {depth}")
    whole = render(1, "cornell_dragon", 257, 131, 16, depth=depth)
    same(b, whole, f"3 parts against the whole frame, depth {depth}")


@pytest.mark.parametrize("flags", [0, g.FLAG_MISS_KEEPS_PATH], ids=["plain", "miss-keeps-path"])
@pytest.mark.parametrize("depth", [2, 4])
def test_anyhit_open_scene(flags, depth):
    """no spheres at all: the bound is PT_F32_MAX and a last segment that finds no triangle takes the background rule"""
    a, b = (render(v, "cornell", 320, 180, 16, depth=depth, flags=flags, spheres=False) for v in (0, 1))
    same(b, a, f"open scene, flags {flags}, depth {depth}")


def test_anyhit_miss_keeps_path():
    a, b = (render(v, "cornell_dragon", 320, 180, 16, flags=g.FLAG_MISS_KEEPS_PATH) for v in (0, 1))
    same(b, a, "PT_FLAG_MISS_KEEPS_PATH")


@pytest.mark.parametrize("spp", [16, 8])
def test_anyhit_running_mean(spp):
    """sample_index 5 over a pre-filled accumulator, then a second call on top"""
    a, b = (render(v, "cornell_dragon", 257, 131, spp, calls=2, prefill=True) for v in (0, 1))
    same(b, a, f"running mean, spp {spp}")


# the Cornell floor (y = -15) touches the floor sphere's top at (0, -15, -20): t and ts agree to the last bits for segments that
# land near that point
TIE_W, TIE_H, TIE_SPP = 96, 64, 16


def tie_camera():
    return make_camera(TIE_W, TIE_H, pos=(0.0, -9.0, -12.0), front=(0.0, -6.0, -8.0), fov=1.2)


@pytest.mark.parametrize("depth", [2, 4])
def test_anyhit_floor_sphere_tie(depth):
    cam = tie_camera()
    a, b, c = (render(v, "cornell_dragon", TIE_W, TIE_H, TIE_SPP, depth=depth, cam=cam, counters=v == 2) for v in (0, 1, 2))
    same(b, a, f"floor / sphere tie, depth {depth}")
    same(c, a, f"floor / sphere tie, instrumented, depth {depth}")
    assert c[2]["act_shade"] > 0
    # parity with the oracle for that frame, at the bars of test_gpu_scene_matrix.judge
    mesh, bvh = bvh_of("cornell_dragon")
    sph = g.reference_spheres()
    p = g.default_params(TIE_W, TIE_H, depth=depth)
    p.frame, p.sample_index, p.flags = 7, 1, g.FLAG_WRITE_RGBA
    ref = orc.render(bvh, sph, cam, p, TIE_SPP)[:2]

    class T:
        name, exact = "wavefront-last-anyhit", False
    judge(T, f"floor / sphere tie depth {depth}", b[:2], ref, mesh, sph, cam, p, TIE_SPP)


def dark_table(mesh):
    """a per-triangle material table whose rows emit nothing: a table is on the context, so the call is not eligible"""
    p = g.default_params(8, 8)
    n = len(np.asarray(mesh.tris))
    table, ids = red_copies_table(n, n, p)
    return table, ids


INELIGIBLE = {
    "nee": dict(flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF),
    "material-table": dict(table=dark_table),
    "emitting-triangles": dict(tri_emi=(0.0, 0.25, 0.0)),
    "depth-1": dict(depth=1),
    "woop-records": dict(before_upload=((g.OPT_TRI_TEST, 1),)),
}


@pytest.mark.parametrize("case", list(INELIGIBLE))
def test_ineligible_calls_keep_the_closest_hit_walk(case):
    kw = INELIGIBLE[case]
    a, b = (render(v, "cornell_dragon", 257, 131, 16, **kw) for v in (0, 1))
    same(b, a, case)
    c0, c2 = (render(v, "cornell_dragon", 257, 131, 16, counters=True, **kw) for v in (0, 2))
    same(c2, a, f"{case}, instrumented")
    if case != "woop-records":   # (Woop records run the persistent kernel, whose "act_shade" counts its shading lanes)
        assert c2[2]["act_shade"] == 0, f"{case}: the any-hit launch ran"
    for k in ("rays", "inner", "tris", "leaves", "hits", "paths", "act_shade"):
        assert c2[2][k] == c0[2][k], (case, k)


@pytest.mark.parametrize("depth", [2, 4])
def test_counted_anyhit_visits_fewer_items(depth):
    """option 2 under PT_OPT_COUNTERS runs the any-hit launch: same rays, strictly fewer item visits; option 1 keeps the
    closest-hit walk's counters"""
    c0, c1, c2 = (render(v, "cornell_dragon", 320, 180, 16, depth=depth, counters=True) for v in (0, 1, 2))
    same(c1, c0, "instrumented, 1")
    same(c2, c0, "instrumented, 2")
    k0, k1, k2 = c0[2], c1[2], c2[2]
    for k in ("rays", "inner", "tris", "leaves", "hits", "paths"):
        assert k1[k] == k0[k], k
    assert k0["act_shade"] == 0 and k1["act_shade"] == 0 and k2["act_shade"] > 0
    assert k2["rays"] == k0["rays"] and k2["paths"] == k0["paths"]
    print(f"depth {depth}: items closest {k0['inner'] + k0['tris']} any-hit {k2['inner'] + k2['tris']}, any-hit rays {k2['act_shade']}")
    assert k2["inner"] + k2["tris"] < k0["inner"] + k0["tris"]


def test_last_anyhit_option_values():
    t = g.PathTracer(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.PtError):
                t.set_option(g.OPT_LAST_ANYHIT, bad)
        for ok in (0, 2, 1):
            t.set_option(g.OPT_LAST_ANYHIT, ok)
    finally:
        t.close()
