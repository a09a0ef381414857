"""PT_OPT_LAST_ANYHIT: when no triangle can emit, the stage-split pipeline walks a path's last segment as an any-hit query bounded
by the segment's nearest sphere hit (1, default; 2 = instrumented launches too) instead of finding the closest triangle (0).  The
picture only needs to know whether a triangle lies at or before the sphere, so the accumulator and the display words must be the
same bit for bit, calls that are not eligible must not run the any-hit launch at all (wave stat "act_shade" counts its rays), and
where it runs it must visit fewer items."""
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import TIE_H, TIE_SPP, TIE_W, bvh_of, dark_table, judge, pipeline_render, same, tie_camera

pytestmark = pytest.mark.gpu


def render(anyhit, *args, options=(), **kw):
    return pipeline_render(((g.OPT_LAST_ANYHIT, anyhit),) + tuple(options), *args, **kw)


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


@pytest.mark.parametrize("depth", [2, 4])
def test_anyhit_floor_sphere_tie(depth):
    cam = tie_camera()
    a, b, c = (render(v, "cornell_dragon", TIE_W, TIE_H, TIE_SPP, depth=depth, cam=cam, counters=v == 2) for v in (0, 1, 2))
    same(b, a, f"floor / sphere tie, depth {depth}")
    same(c, a, f"floor / sphere tie, instrumented, depth {depth}")
    assert c[2]["act_shade"] > 0
    # parity with the oracle for that frame, at the bars of gpu_support.judge
    mesh, bvh = bvh_of("cornell_dragon")
    sph = g.reference_spheres()
    p = g.default_params(TIE_W, TIE_H, depth=depth)
    p.frame, p.sample_index, p.flags = 7, 1, g.FLAG_WRITE_RGBA
    ref = orc.render(bvh, sph, cam, p, TIE_SPP)[:2]

    class T:
        name, exact = "wavefront-last-anyhit", False
    judge(T, f"floor / sphere tie depth {depth}", b[:2], ref, mesh, sph, cam, p, TIE_SPP)


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
