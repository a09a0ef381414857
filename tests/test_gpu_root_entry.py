"""PT_OPT_ROOT_ENTRY: the shade lane that classifies a survivor's new ray (PT_OPT_ROOT_CULL) keeps the whole result of the walk's
node step on the tree's root — which of the four children the ray enters, nearest first — as an 8-bit code above a narrowed sample
field in the record, and the extend launches of the later bounces start every walk behind the root (1, default: product launches;
2: instrumented launches too; 0: every walk starts at the root).  Stack, first item and h.t are the walk's own after its first
step, so the accumulator and the display words must be the same bit for bit; with 0 and 1 an instrumented call counts what it
always counted, with 2 it lacks exactly one node visit per ray the extend launches drew (wave stat "act_begin").  Calls the option
does not apply to (PT_FLAG_NEE, no root cull, spp beyond the narrowed field) keep the plain record whatever its value."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
from scene_matrix import make_camera
from gpu_support import COUNTERS, cornell_dragon_moved, dark_table, golden_camera, pipeline_render, same

pytestmark = pytest.mark.gpu
ENTRY = g._abi.OPT_ROOT_ENTRY   # 33 (kept out of the package's exported OPT_* names)
MAX_SPP = (1 << 12) - 1           # the largest spp the narrowed sample field holds: 32 - 8 code bits - 12 draw bits, exclusive limit


def pair(scene, W, H, spp, values=(0, 1), cull=1, options=(), **kw):
    """the frames (and counters) of the same call with PT_OPT_ROOT_ENTRY at each of `values`"""
    return [pipeline_render(((g.OPT_ROOT_CULL, cull),) + tuple(options) + ((ENTRY, v),), scene, W, H, spp, **kw) for v in values]


def test_option_number_and_values():
    assert ENTRY == 33 and not hasattr(g, "OPT_ROOT_ENTRY")
    t = g.PathTracer(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.PtError):
                t.set_option(ENTRY, bad)
        for ok in (0, 2, 1):
            t.set_option(ENTRY, ok)
    finally:
        t.close()


@pytest.mark.parametrize("size", [(257, 131), (64, 64)], ids=["257x131", "64x64"])
@pytest.mark.parametrize("spp", [16, 4, 1])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_entry_equals_root_start(size, spp, depth):
    W, H = size
    a, b = pair("cornell_dragon", W, H, spp, depth=depth)
    same(b, a, f"{W}x{H} spp {spp} depth {depth}")


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("first_walk", [0, 1])
@pytest.mark.parametrize("anyhit", [0, 1])
def test_entry_under_every_stage_layout(fuse, first_walk, anyhit):
    """the code is made by the fused packet launch, by k_wf_shade<FIRST> behind either walk, and (any-hit 1) by the BOUND launch
    against the sphere bound the any-hit lane starts with; depth 2: bounce 0's launch is the BOUND one"""
    opts = ((g.OPT_FUSE_STAGES, fuse), (g.OPT_FIRST_WALK, first_walk), (g.OPT_LAST_ANYHIT, anyhit))
    for depth in (2, 4):
        a, b = pair("cornell_dragon", 257, 131, 4, depth=depth, options=opts)
        same(b, a, f"fuse {fuse} first walk {first_walk} any-hit {anyhit} depth {depth}")


CALLS = {
    "three-parts": dict(parts=3),
    "running-mean": dict(calls=2, prefill=True),
    "metal": dict(tri_mat=g.MAT_METAL),
    "mirror": dict(tri_mat=g.MAT_SPEC),
    "material-table": dict(table=dark_table),
}


@pytest.mark.parametrize("case", list(CALLS))
def test_entry_call_shapes_and_materials(case):
    a, b = pair("cornell_dragon", 257, 131, 4, **CALLS[case])
    same(b, a, case)


def around(scene, W, H, inside):
    """a camera looking at the middle of the mesh's bounds from outside them, or placed inside them"""
    lo, hi = (np.asarray(x, np.float64) for x in g.scene_mesh(scene).bounds())
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    if inside:
        return make_camera(W, H, pos=c + np.array([0.11, 0.07, 0.13]) * ext, front=(0.2, -0.1, -1.0))
    pos = c + np.array([0.4, 0.3, 1.6]) * ext
    return make_camera(W, H, pos=pos, front=c - pos)


SMALL = {   # (scene, spheres, camera inside the bounds); the cube lies around the origin, outside the lit room: looked at from outside only
    "cube": ("cube", True, False), "cube-open": ("cube", False, False),
    "cornell": ("cornell", True, False), "cornell-open": ("cornell", False, False), "cornell-inside": ("cornell", True, True),
}


@pytest.mark.parametrize("case", list(SMALL))
def test_entry_small_roots(case):
    """12 and 32 triangles: the root's children are leaves (the nearest child's link is a leaf link) or fewer than four"""
    scene, spheres, inside = SMALL[case]
    cam = around(scene, 96, 64, inside)
    for anyhit in (0, 1):
        a, b = pair(scene, 96, 64, 4, spheres=spheres, cam=cam, options=((g.OPT_LAST_ANYHIT, anyhit),))
        same(b, a, f"{case}, any-hit {anyhit}")


def test_entry_camera_inside_the_mesh():
    """from inside the bounds most rays enter several of the root's children: the four-hit code with its implied last index (the
    golden camera outside covers one and two)"""
    cam = around("cornell_dragon", 257, 131, True)
    a, b = pair("cornell_dragon", 257, 131, 4, cam=cam)
    same(b, a, "camera inside")
    c0, c2 = pair("cornell_dragon", 257, 131, 4, values=(0, 2), cull=2, cam=cam, counters=True)
    same(c2, c0, "camera inside, instrumented")
    assert c2[2]["inner"] == c0[2]["inner"] - c2[2]["act_begin"] and c2[2]["act_begin"] > 0
    for k in ("rays", "tris", "leaves", "hits", "paths"):
        assert c2[2][k] == c0[2][k], k


def test_entry_deep_stack_instantiation():
    """PT_OPT_LDS_STACK 24: the 6-wave instantiations"""
    a, b = pair("cornell_dragon", 257, 131, 4, options=((g.OPT_LDS_STACK, 24),))
    same(b, a, "LDS stack 24")
    whole = pair("cornell_dragon", 257, 131, 4, values=(1,))[0]
    same(b, whole, "LDS stack 24 against 16")


def other_tree(v, kind, W=257, H=131, spp=4):
    """frames of cornell_dragon with PT_OPT_ROOT_ENTRY = v over a tree that is not the uploaded host tree: `device`: pt_build_bvh;
    `refit`: the same after pt_refit_bvh turned and moved the dragon (the root's boxes change, its links stay)"""
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.set_option(ENTRY, v)
        mesh, _, moved = cornell_dragon_moved()
        t.build_bvh(mesh)
        if kind == "refit":
            t.refit_bvh(moved)
        t.upload_spheres(g.reference_spheres())
        acc, rgba = t.alloc_frame(W, H)
        p = g.default_params(W, H)
        p.flags, p.frame, p.sample_index = g.FLAG_WRITE_RGBA, 7, 1
        t.launch_kernel(acc.ptr, rgba.ptr, golden_camera(W, H), p, spp)
        t.sync()
        out = (acc.download(np.float32, (H, W, 3)), rgba.download(np.uint32, (H, W)))
        acc.free()
        rgba.free()
        return out
    finally:
        t.close()


@pytest.mark.parametrize("kind", ["device", "refit"])
def test_entry_device_built_and_refit_trees(kind):
    a, b = (other_tree(v, kind) for v in (0, 1))
    same(b, a, kind)
    if kind == "refit":   # the refit did move something
        assert not np.array_equal(b[0], other_tree(1, "device")[0])


def test_entry_reclustered_tree():
    a, b = pair("cornell_dragon", 257, 131, 4, options=((g.OPT_REBUILD, 1),))
    same(b, a, "PT_OPT_REBUILD 1")


# ---- calls the option does not apply to: the same frame whatever its value
def test_fallback_nee():
    a, b, c = pair("cornell_dragon", 257, 131, 4, values=(0, 1, 2), flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF)
    same(b, a, "NEE, 1")
    same(c, a, "NEE, 2")


def test_fallback_without_root_cull():
    a, b = pair("cornell_dragon", 257, 131, 4, cull=0)
    same(b, a, "root cull 0")
    same(b, pair("cornell_dragon", 257, 131, 4, values=(1,))[0], "root cull 0 against 1")
    c0, c2 = pair("cornell_dragon", 64, 64, 4, values=(0, 2), cull=0, counters=True)   # no classification, so no code to start from
    same(c2, c0, "root cull 0, instrumented")
    for k in COUNTERS:
        assert c2[2][k] == c0[2][k], k


@pytest.mark.parametrize("spp", [MAX_SPP, MAX_SPP + 1], ids=["largest-spp", "one-more"])
def test_fallback_spp_at_the_narrowed_field(spp):
    """sample numbers up to the field's last value, then the first call that keeps the plain record"""
    a, b = pair("cornell_dragon", 16, 8, spp)
    same(b, a, f"spp {spp}")


# ---- counters
def test_counters_unchanged_with_0_and_1():
    for cull in (1, 2):
        c0, c1 = pair("cornell_dragon", 257, 131, 4, cull=cull, counters=True)
        same(c1, c0, f"instrumented, root cull {cull}")
        assert c1[2] == c0[2], {k: (c0[2][k], c1[2][k]) for k in c0[2] if c0[2][k] != c1[2][k]}


@pytest.mark.parametrize("anyhit", [0, 2])
@pytest.mark.parametrize("depth", [2, 4])
def test_counters_with_2(anyhit, depth):
    """PT_OPT_ROOT_CULL 2: the same rays, records, leaves, hits and paths, and one node visit less per ray k_wf_extend drew — the
    root's ("act_begin": the lanes its refills served; bounce 0 is the packet walk, which draws none)"""
    opts = ((g.OPT_LAST_ANYHIT, anyhit),)
    c0, c2 = pair("cornell_dragon", 257, 131, 4, values=(0, 2), cull=2, depth=depth, counters=True, options=opts)
    same(c2, c0, "instrumented, 2")
    k0, k2 = c0[2], c2[2]
    print(f"any-hit {anyhit} depth {depth}: rays {k2['rays']}, drawn {k2['act_begin']}, inner {k0['inner']} -> {k2['inner']}")
    for k in ("rays", "tris", "leaves", "hits", "paths", "act_begin", "walk_free"):
        assert k2[k] == k0[k], k
    assert 0 < k2["act_begin"] < k2["rays"]
    assert k2["inner"] == k0["inner"] - k2["act_begin"]
