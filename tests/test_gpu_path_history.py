"""PT_OPT_PATH_HISTORY: the stage-split pipeline's path records carry WHICH objects a path has hit — four bits per bounce in one
word — instead of its mask as three floats; a shade lane rebuilds the mask and the gathered light from that word with the path's own
arithmetic, and the sample colour is written once, by the lane the path ends in (1, default: product launches; 2: instrumented
launches too; 0: the three mask planes and the in-place adds).  Both vectors are rebuilt bit for bit, so the accumulator and the
display words must be the same bit for bit under every value, no counter may change, and a call the mode does not hold for (NEE, a
roulette, a material table, refraction, nine spheres, depth 10) renders what it rendered.  A path that ended without its one store
would show the previous call's sample: the stale-sample test renders two different frames on one context."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import bits, bvh_of, dark_table, golden_camera, judge, pipeline_render, same

pytestmark = pytest.mark.gpu
HISTORY = g._abi.OPT_PATH_HISTORY   # 34 (kept out of the package's exported OPT_* names)
W, H = 257, 131                     # partial tiles, a partial last region


def render(v, *args, options=(), **kw):
    return pipeline_render(tuple(options) + ((HISTORY, v),), *args, **kw)


def all_values(what, *args, **kw):
    """the same call with the option off, on for product launches, and on for an instrumented call too: one frame"""
    a, b = (render(v, *args, **kw) for v in (0, 1))
    c = render(2, *args, counters=True, **kw)
    same(b, a, f"{what}: 1 against 0")
    same(c, a, f"{what}: 2 with counters against 0")
    return a


def test_option_number_and_values():
    assert HISTORY == 34 and not hasattr(g, "OPT_PATH_HISTORY")
    t = g.PathTracer(0)
    try:
        for bad in (-1, 3):
            with pytest.raises(g.PtError):
                t.set_option(HISTORY, bad)
        for ok in (0, 2, 1):
            t.set_option(HISTORY, ok)
    finally:
        t.close()


@pytest.mark.parametrize("size", [(W, H), (64, 64)], ids=["257x131", "64x64"])
@pytest.mark.parametrize("spp", [16, 4, 1])   # the fold in the last launch, the separate fold, no sample groups
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 9])   # 1: the first launch is the last; 9: all eight fields of the word
def test_history_equals_mask_planes(size, spp, depth):
    all_values(f"{size[0]}x{size[1]} spp {spp} depth {depth}", "cornell_dragon", size[0], size[1], spp, depth=depth)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("first_walk", [0, 1])
@pytest.mark.parametrize("anyhit", [0, 1])
def test_history_under_every_stage_layout(fuse, first_walk, anyhit):
    """the first code is written by the fused packet launch or by k_wf_shade<FIRST> behind either walk; the sample by the LAST
    launch, by the launch behind the any-hit walk, or (depth 2) straight after the launch that made the first code"""
    opts = ((g.OPT_FUSE_STAGES, fuse), (g.OPT_FIRST_WALK, first_walk), (g.OPT_LAST_ANYHIT, anyhit))
    for depth in (2, 4):
        a, b = (render(v, "cornell_dragon", W, H, 4, depth=depth, options=opts) for v in (0, 1))
        same(b, a, f"fuse {fuse} first walk {first_walk} any-hit {anyhit} depth {depth}")


@pytest.mark.parametrize("cull", [0, 1])
def test_history_with_and_without_root_cull(cull):
    all_values(f"root cull {cull}", "cornell_dragon", W, H, 4, options=((g.OPT_ROOT_CULL, cull),))


CALLS = {
    "metal": dict(tri_mat=g.MAT_METAL),
    "mirror": dict(tri_mat=g.MAT_SPEC),
    "emitting-triangles": dict(tri_emi=(0.25, 0.5, 0.125)),   # the triangle row's emission; no any-hit last segment
    "three-parts": dict(parts=3),
    "running-mean": dict(calls=2, prefill=True),
    # paths die on misses at every bounce: the miss rule on the rebuilt accu and mask is their one store
    "open": dict(spheres=False),
    "open-miss-keeps-path": dict(spheres=False, flags=g.FLAG_MISS_KEEPS_PATH),
    "open-depth-9": dict(spheres=False, flags=g.FLAG_MISS_KEEPS_PATH, depth=9),
}


@pytest.mark.parametrize("case", list(CALLS))
def test_history_call_shapes_materials_open_scenes(case):
    all_values(case, "cornell_dragon", W, H, 4, **CALLS[case])


# ---- calls the mode does not hold for: the same frame whatever the option's value
FALLBACKS = {
    "depth-10": dict(depth=10),
    "nee": dict(flags=g.FLAG_NEE | g.FLAG_COSINE_DIFF),
    "russian-roulette": dict(flags=g.FLAG_RUSSIAN_ROULETTE),
    "cpu-tracer-roulette": dict(flags=g.FLAG_RR_CPU_TRACER, depth=8),   # (it plays from the sixth hit on)
    "material-table": dict(table=dark_table),
    "glass-triangles": dict(tri_mat=g.MAT_REFR),
}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallback(case):
    all_values(case, "cornell_dragon", W, H, 4, **FALLBACKS[case])


def sphere_set(kind):
    ref = g.reference_spheres()
    if kind == "one-glass":   # the small mirror sphere refracts instead
        ref[6].mat = g.MAT_REFR
        return ref
    arr = (g.Sphere * 9)()   # nine: beyond the kernel-argument block, so beyond the codes
    for k in range(8):
        C.memmove(C.byref(arr[k]), C.byref(ref[k]), C.sizeof(g.Sphere))
    arr[8].pos_rad[:] = (-12.0, -9.0, -40.0, 5.0)
    arr[8].emi[:] = (0.5, 0.25, 0.0)
    arr[8].col[:] = (0.75, 0.75, 0.25)
    arr[8].mat = g.MAT_DIFF
    return arr


def frames(v, spheres=None, first_frames=(7,), spp=4, depth=4, moments=False, size=(W, H), counters=False):
    """the frames of one pt_render call per entry of `first_frames`, all on ONE context with PT_OPT_PATH_HISTORY = v, each from an
    empty accumulator: [(accumulator, display words[, moments])]"""
    w, h = size
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)
        t.set_option(HISTORY, v)
        if counters:
            t.set_option(g.OPT_COUNTERS, 1)
        t.upload_bvh(bvh_of("cornell_dragon")[1])
        t.upload_spheres(g.reference_spheres() if spheres is None else spheres)
        acc, rgba = t.alloc_frame(w, h)
        mom = t.malloc(w * h * 8) if moments else None
        out = []
        for f in first_frames:
            p = g.default_params(w, h, depth=depth)
            p.flags, p.frame, p.sample_index = g.FLAG_WRITE_RGBA, f, 1
            t.launch_kernel(acc.ptr, rgba.ptr, golden_camera(w, h), p, spp, moments_ptr=mom.ptr if moments else None)
            t.sync()
            out.append((acc.download(np.float32, (h, w, 3)), rgba.download(np.uint32, (h, w))) +
                       ((mom.download(np.float32, (h, w, 2)),) if moments else ()))
        for b in (acc, rgba) + ((mom,) if moments else ()):
            b.free()
        return out
    finally:
        t.close()


@pytest.mark.parametrize("kind", ["one-glass", "nine"])
def test_fallback_sphere_sets(kind):
    a, b, c = (frames(v, spheres=sphere_set(kind), counters=v == 2)[0] for v in (0, 1, 2))
    same(b, a, f"{kind}: 1 against 0")
    same(c, a, f"{kind}: 2 with counters against 0")
    assert not np.array_equal(a[0], frames(0)[0][0]), f"{kind}: the sphere set changed nothing"


@pytest.mark.parametrize("spp", [16, 4, 1])
def test_no_stale_samples(spp):
    """Two calls with different frames on ONE context: the second must be what a fresh context renders for that frame.  Bounce 0 no
    longer writes every sample, so a path that ended without its store would keep the first call's colour."""
    for depth in (1, 4):
        second = frames(1, first_frames=(7, 1007), spp=spp, depth=depth)[1]
        fresh = frames(1, first_frames=(1007,), spp=spp, depth=depth)[0]
        same(second, fresh, f"spp {spp} depth {depth}: second call against a fresh context")
        same(second, frames(0, first_frames=(1007,), spp=spp, depth=depth)[0], f"spp {spp} depth {depth}: against the mask planes")


def test_moments_call():
    """pt_render_moments: the separate fold launch reads the samples for the moments too"""
    a, b = (frames(v, spp=16, moments=True)[0] for v in (0, 1))
    same(b, a, "moments call")
    assert np.array_equal(bits(a[2]), bits(b[2])) and a[2].any(), "moments differ"


@pytest.mark.parametrize("anyhit", [0, 2])
@pytest.mark.parametrize("depth", [2, 4])
def test_counters_unchanged(anyhit, depth):
    opts = ((g.OPT_LAST_ANYHIT, anyhit), (g.OPT_ROOT_CULL, anyhit), (g._abi.OPT_ROOT_ENTRY, anyhit))
    c0, c1, c2 = (render(v, "cornell_dragon", W, H, 4, depth=depth, counters=True, options=opts) for v in (0, 1, 2))
    same(c1, c0, "instrumented, 1")
    same(c2, c0, "instrumented, 2")
    assert c0[2]["rays"] > 0
    for c in (c1, c2):
        assert c[2] == c0[2], {k: (c0[2][k], c[2][k]) for k in c0[2] if c0[2][k] != c[2][k]}


# ---- against the other renderers
def test_against_the_oracle():
    mesh, bvh = bvh_of("cornell_dragon")
    sph, cam = g.reference_spheres(), golden_camera(W, H)

    class T:
        name, exact = "wavefront-path-history", False
    b = render(1, "cornell_dragon", W, H, 4, depth=4)
    p = g.default_params(W, H, depth=4)
    p.frame, p.sample_index, p.flags = 7, 1, g.FLAG_WRITE_RGBA
    ref = orc.render(bvh, sph, cam, p, 4)[:2]
    print(f"{int(np.any(b[0] != ref[0], axis=-1).sum())} pixels differ from the oracle")
    judge(T, "257x131, 4 spp, depth 4", b[:2], ref, mesh, sph, cam, p, 4)


def test_against_the_persistent_kernel():
    """the persistent kernel carries mask and accu in registers from bounce to bounce: what the history word rebuilds"""
    persist = pipeline_render(((g.OPT_KERNEL, g.KERNEL_PERSISTENT),), "cornell_dragon", W, H, 4, depth=4)
    same(render(1, "cornell_dragon", W, H, 4, depth=4), persist, "against the persistent kernel")
