"""PT_OPT_FUSE_STAGES: bounce 0's shade inside the packet walk's launch and the fold inside the last shade launch (1, default)
against one launch per stage (0).  The fused launches run the same arithmetic on the same paths, so the accumulator and the display
words must be the same bit for bit, and the instrumented counters (which always run the separate launches) must agree."""
import pytest

import gpu_pathtracer_amd as g
from gpu_support import COUNTERS, pipeline_render, same

pytestmark = pytest.mark.gpu


def render(fuse, *args, options=(), **kw):
    return pipeline_render(((g.OPT_FUSE_STAGES, fuse),) + tuple(options), *args, **kw)


@pytest.mark.parametrize("size", [(640, 360), (257, 131)], ids=["640x360", "257x131"])
@pytest.mark.parametrize("spp", [16, 8, 4, 32])
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_fused_equals_separate(size, spp, depth):
    """spp 16 / 8 / 4 fold in the last shade launch (depth >= 2), 32 keeps the separate fold; depth 1 fuses bounce 0 only"""
    W, H = size
    a, b = (render(f, "cornell_dragon", W, H, spp, depth=depth) for f in (0, 1))
    same(b, a, f"{W}x{H} spp {spp} depth {depth}")


@pytest.mark.parametrize("flags", [0, g.FLAG_MISS_KEEPS_PATH], ids=["plain", "miss-keeps-path"])
def test_fused_equals_separate_open_scene(flags):
    """cornell without the sphere room: most regions are empty after bounce 0 and must still fold at the last bounce"""
    a, b = (render(f, "cornell", 320, 180, 16, flags=flags, spheres=False) for f in (0, 1))
    same(b, a, f"open scene, flags {flags}")


def test_fused_equals_separate_miss_keeps_path():
    a, b = (render(f, "cornell_dragon", 320, 180, 16, flags=g.FLAG_MISS_KEEPS_PATH) for f in (0, 1))
    same(b, a, "PT_FLAG_MISS_KEEPS_PATH")


@pytest.mark.parametrize("spp", [16, 8])
def test_fused_running_mean(spp):
    """sample_index > 1 over a pre-filled accumulator, then a second call on top"""
    a, b = (render(f, "cornell_dragon", 257, 131, spp, calls=2, prefill=True) for f in (0, 1))
    same(b, a, f"running mean, spp {spp}")


def test_nee_unfused_matches():
    flags = g.FLAG_NEE | g.FLAG_COSINE_DIFF
    a, b = (render(f, "cornell_dragon", 320, 180, 16, flags=flags) for f in (0, 1))
    same(b, a, "NEE")


def test_wave_samples_cap_keeps_separate_fold():
    """PT_OPT_WAVE_SAMPLES 4 with 16 spp: a region holds 4 of a pixel's 16 samples, so the fold stays a launch of its own"""
    opts = ((g.OPT_WAVE_SAMPLES, 4),)
    a, b = (render(f, "cornell_dragon", 257, 131, 16, options=opts) for f in (0, 1))
    same(b, a, "wave samples 4")


def test_counters_equal():
    """the work counters and the packet walk's group count; the per-lane extend's schedule statistics (which wave took which
    region) vary from run to run whatever the option, so they are not compared"""
    a, b = (render(f, "cornell_dragon", 320, 180, 16, counters=True) for f in (0, 1))
    same(b, a, "instrumented")
    for k in COUNTERS:
        assert a[2][k] == b[2][k], k
    assert a[2]["it_shade"] == b[2]["it_shade"] > 0


def test_fuse_option_values():
    t = g.PathTracer(0)
    try:
        for bad in (-1, 2):
            with pytest.raises(g.PtError):
                t.set_option(g.OPT_FUSE_STAGES, bad)
    finally:
        t.close()
