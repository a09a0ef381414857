"""What the host layer of libptmi.so decides, pinned: which kernel family a pt_render call launches and which values
pt_set_option accepts.  The images are equal across the families by design, so a fallback rule that stopped firing would pass
every parity test and only show as a slowdown; and the options' ranges are written nowhere else.

(a) PathTracer.stage_ms() is the observable: a stage that ran reports a time above 0, one that did not reports exactly 0.0.
    "pipeline": the stage-split launches (generate, extend) ran and no frame kernel; "frame kernel": the persistent kernel or the
    megakernel ran and none of generate / extend / shade.  Every expectation is derived from the rules of the render call:
    the option, then PT_KERNEL_AUTO's trials, then the PT_FLAG_NEE override, then the fallbacks (no tree, depth 0, a walk other
    than the wide one, Woop records).
(b) every option id 0..32 and 99 against a probe set that straddles every range's ends."""
import pytest

import gpu_pathtracer_amd as g
from gpu_support import bvh_of, golden_camera, is_frame_kernel, is_pipeline

pytestmark = pytest.mark.gpu
W, H = 64, 32
NEE = g.FLAG_NEE | g.FLAG_COSINE_DIFF
PT_OK, PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 0, -1, -5


def context(kernel, options=(), tree=True, spheres=True):
    t = g.PathTracer(0)
    t.set_option(g.OPT_KERNEL, kernel)
    t.set_option(g.OPT_TIMING, 1)
    for o, v in options:   # (before the upload: PT_OPT_TRI_TEST decides the records it makes)
        t.set_option(o, v)
    if tree:
        t.upload_bvh(bvh_of("cornell")[1])
    t.upload_spheres(g.reference_spheres() if spheres else None)
    return t


def call(t, frame, depth=4, spp=1, flags=0, moments=None, call_no=0):
    """one pt_render call; returns its stage times"""
    acc, rgba = frame
    p = g.default_params(W, H, depth=depth)
    p.flags = flags | g.FLAG_WRITE_RGBA
    p.frame, p.sample_index = 7 + call_no * spp, 1 + call_no * spp
    t.launch_kernel(acc.ptr, rgba.ptr, golden_camera(W, H), p, spp, moments_ptr=None if moments is None else moments.ptr)
    t.sync()
    ms = t.stage_ms()
    print(ms)
    return ms


# id: (kernel, context arguments, call arguments, moments buffer, pipeline?, {stage: ran?})
CASES = {
    "wavefront": (g.KERNEL_WAVEFRONT, {}, {}, False, True, {"shade": True, "fold": True}),
    "wavefront-spp4": (g.KERNEL_WAVEFRONT, {}, dict(spp=4), False, True, {"shade": True, "fold": False}),   # folded in the last shade launch
    "wavefront-spp4-depth1": (g.KERNEL_WAVEFRONT, {}, dict(spp=4, depth=1), False, True, {"shade": False, "fold": True}),   # bounce 0 shaded in the fused launch
    "wavefront-spp4-unfused": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_FUSE_STAGES, 0),)), dict(spp=4), False, True, {"fold": True}),
    "wavefront-spp4-moments": (g.KERNEL_WAVEFRONT, {}, dict(spp=4), True, True, {"fold": True}),
    "wavefront-spp4-counters": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_COUNTERS, 1),)), dict(spp=4), False, True, {"fold": True}),
    "wavefront-depth0": (g.KERNEL_WAVEFRONT, {}, dict(depth=0), False, False, {"fold": False}),
    "wavefront-walk0": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_WALK, 0),)), {}, False, False, {}),
    "wavefront-walk1": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_WALK, 1),)), {}, False, False, {}),
    "wavefront-walk4": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_WALK, 4),)), {}, False, False, {}),
    "wavefront-no-tree": (g.KERNEL_WAVEFRONT, dict(tree=False), {}, False, False, {}),
    "wavefront-woop": (g.KERNEL_WAVEFRONT, dict(options=((g.OPT_TRI_TEST, 1),)), {}, False, False, {}),
    "persistent-nee": (g.KERNEL_PERSISTENT, {}, dict(flags=NEE), False, True, {}),
    "persistent-nee-walk0": (g.KERNEL_PERSISTENT, dict(options=((g.OPT_WALK, 0),)), dict(flags=NEE), False, False, {}),   # the megakernel's loop
    "persistent": (g.KERNEL_PERSISTENT, {}, {}, False, False, {"fold": False}),
    "persistent-spp4": (g.KERNEL_PERSISTENT, {}, dict(spp=4), False, False, {"fold": True}),
    "persistent-moments": (g.KERNEL_PERSISTENT, {}, {}, True, False, {"fold": True}),
    "auto-counters": (g.KERNEL_AUTO, dict(options=((g.OPT_COUNTERS, 1),)), {}, False, False, {}),
    "auto-nee": (g.KERNEL_AUTO, {}, dict(flags=NEE), False, True, {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_what_a_call_launches(case):
    kernel, ctx_kw, call_kw, with_moments, pipeline, stages = CASES[case]
    t = context(kernel, **ctx_kw)
    try:
        frame = t.alloc_frame(W, H)
        moments = None
        if with_moments:
            moments = t.malloc(W * H * 8)
            moments.zero()
        ms = call(t, frame, moments=moments, **call_kw)
        assert is_pipeline(ms) if pipeline else is_frame_kernel(ms), (case, ms)
        for stage, ran in stages.items():
            assert (ms[stage] > 0) == ran and (ran or ms[stage] == 0.0), (case, stage, ms)
        if case == "auto-counters":   # an instrumented call is no trial: nothing was looked up
            assert t.auto_choice()[0] == g.KERNEL_AUTO
    finally:
        t.close()


def test_auto_trials_then_the_choice():
    """the first four calls of a configuration are the timed trials, persistent kernel and pipeline in turn; once their times are
    read the following calls run the family chosen"""
    t = context(g.KERNEL_AUTO)
    try:
        frame = t.alloc_frame(W, H)
        for n, pipeline in enumerate((False, True, False, True)):
            ms = call(t, frame, call_no=n)
            assert is_pipeline(ms) if pipeline else is_frame_kernel(ms), (n, ms)
        k = t.auto_choice()[0]
        assert k in (g.KERNEL_PERSISTENT, g.KERNEL_WAVEFRONT)
        for n in (4, 5):
            ms = call(t, frame, call_no=n)
            assert is_pipeline(ms) if k == g.KERNEL_WAVEFRONT else is_frame_kernel(ms), (n, k, ms)
            assert t.auto_choice()[0] == k
    finally:
        t.close()


# ---- (b) pt_set_option
PROBES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 24, 25, 36, 64, 65, 72, 73, 1024, 1025, 100000, 100001)
ANY = None   # any int is taken (as a flag)


def between(lo, hi):
    return set(range(lo, hi + 1))


ACCEPTS = {
    g.OPT_KERNEL: {0, 1, 3, 5},
    g.OPT_COUNTERS: ANY, g.OPT_TIMING: ANY, g.OPT_SPHERE_LDS: ANY, g.OPT_OVERLAP: ANY,
    g.OPT_TOP_NODES: between(0, 1024),
    g.OPT_OCCUPANCY: {4, 5, 6, 8},
    g.OPT_LDS_STACK: {0, 16, 24},
    g.OPT_WALK: {0, 1, 2, 4},
    g.OPT_LEAF_MAX: between(0, 1024),
    g.OPT_TRI_TEST: {0, 1}, g.OPT_BUILD_ALGO: {0, 1}, g.OPT_FIRST_WALK: {0, 1}, g.OPT_FUSE_STAGES: {0, 1},
    g.OPT_REBUILD: between(0, 2), g.OPT_LAST_ANYHIT: between(0, 2), g.OPT_ROOT_CULL: between(0, 2),
    g.OPT_PRESPLIT: between(0, 100000),
    g.OPT_OPTIMIZE: between(0, 16),
    g.OPT_WAVE_BLOCKS: between(1, 8),
    g.OPT_PACKET_STACK: between(2, 72),
    g.OPT_BATCH: between(1, 64), g.OPT_REFILL: between(1, 64), g.OPT_VOTE_NODE: between(1, 64), g.OPT_VOTE_REC: between(1, 64),
    g.OPT_WAVE_BATCH: between(1, 64), g.OPT_WAVE_SAMPLES: between(1, 64),
}


def test_the_table_names_every_option():
    assert sorted(ACCEPTS) == sorted(v for k, v in vars(g).items() if k.startswith("OPT_"))


@pytest.mark.parametrize("option", list(range(33)) + [99])
def test_what_set_option_accepts(option):
    t = g.PathTracer(0)
    try:
        for v in PROBES:
            rc = t._lib.pt_set_option(t._ctx, option, v)
            if option not in ACCEPTS:
                want = PT_ERR_INVALID
            elif ACCEPTS[option] is ANY or v in ACCEPTS[option]:
                want = PT_OK
            else:
                want = PT_ERR_UNSUPPORTED if option == g.OPT_KERNEL else PT_ERR_INVALID
            assert rc == want, (option, v, rc, want)
    finally:
        t.close()
