"""PT_OPT_FIRST_WALK: the stage-split pipeline's bounce-0 extend as wave-wide packets (1) against the per-lane walk (0).

The packet walk tests, for every lane, exactly the boxes and records the lane's own box tests lead to, in another order; the
closest hit does not depend on the order, so the accumulator and the display words must be bit for bit the same.  Where the
bench configuration differs at all, the pixel is arbitrated by the brute-force closest hit, as test_gpu_bench_configs does.
"""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import bvh_of, golden_camera, pipeline_render, same, upload

pytestmark = pytest.mark.gpu


def render(walk, install, W, H, spp, flags=0, parts=1, calls=2, options=(), **kw):
    opts = ((g.OPT_FIRST_WALK, walk),) + tuple(options)
    return pipeline_render(opts, install, W, H, spp, flags=flags, parts=parts, calls=calls, **kw)


@pytest.mark.parametrize("cfg", [((333, 187), 16, 0, 1), ((640, 360), 8, 0, 3), ((640, 360), 12, g.FLAG_NEE | g.FLAG_COSINE_DIFF, 1),
                                 ((333, 187), 5, 0, 1), ((256, 256), 64, 0, 1)],
                         ids=["ragged-16spp", "split3-8spp", "nee-12spp", "ragged-5spp", "64spp"])
def test_packet_equals_per_lane(cfg):
    """the configurations of test_wave_sample_groups_change_no_pixel: ragged image, a tile split, spp that 16 / 8 / 4 divide and one
    that nothing does, next-event estimation, a second call on top of the first"""
    (W, H), spp, flags, parts = cfg
    _, bvh = bvh_of("cornell_dragon")
    frames = [render(walk, upload(bvh), W, H, spp, flags, parts) for walk in (0, 1)]
    same(frames[1], frames[0], str(cfg))


@pytest.mark.parametrize("cull", [0, 1])
def test_packet_equals_per_lane_cull(cull):
    _, bvh = bvh_of("cornell_dragon")
    frames = [render(walk, upload(bvh), 320, 180, 8, cull=cull) for walk in (0, 1)]
    same(frames[1], frames[0], f"cull {cull}")


def test_packet_equals_per_lane_after_refit():
    mesh, bvh = bvh_of("cornell_dragon")
    soup = mesh.triangle_soup().reshape(-1, 3, 3)
    c = soup.reshape(-1, 3).mean(axis=0)
    a = 0.3   # turn every vertex about the vertical axis through the centre, and lift it a little
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]], np.float32)
    moved = np.ascontiguousarray(((soup - c) @ rot.T + c + np.array([0.0, 0.05, 0.0], np.float32)).astype(np.float32).reshape(-1, 9))

    def install(t):
        t.upload_bvh(bvh)
        t.refit_bvh(moved)

    frames = [render(walk, install, 320, 180, 8) for walk in (0, 1)]
    same(frames[1], frames[0], "refit tree")


def test_packet_equals_per_lane_device_tree():
    mesh, _ = bvh_of("cornell_dragon")
    frames = [render(walk, lambda t: t.build_bvh(mesh), 320, 180, 8) for walk in (0, 1)]
    same(frames[1], frames[0], "device-built tree")


def test_packet_equals_per_lane_woop_records():
    """Woop records never reach the stage-split pipeline (they run the persistent kernel): the option changes nothing"""
    _, bvh = bvh_of("cornell_dragon")
    frames = [render(walk, upload(bvh), 320, 180, 8, options=((g.OPT_TRI_TEST, 1),)) for walk in (0, 1)]
    same(frames[1], frames[0], "Woop records")


def test_packet_stack_budget_falls_back_to_per_lane():
    """a tree deeper than the packet stack budget (PT_OPT_PACKET_STACK) runs the per-lane walk: same frames, and the packet
    kernel's group counter (wave stat 4, counter 10, which the stage-split pipeline books nowhere else) stays at zero"""
    _, bvh = bvh_of("cornell_dragon")
    W, H, spp = 320, 180, 8
    base = render(0, upload(bvh), W, H, spp, calls=1, counters=True)
    pkt = render(1, upload(bvh), W, H, spp, calls=1, counters=True)
    low = render(1, upload(bvh), W, H, spp, calls=1, counters=True, options=((g.OPT_PACKET_STACK, 2),))
    for f, what in ((pkt, "packet"), (low, "fallback")):
        same(f, base, what)
    groups = (W + 7) // 8 * ((H + 7) // 8) * spp
    assert pkt[2]["it_shade"] == groups
    assert low[2]["it_shade"] == 0 and base[2]["it_shade"] == 0
    t = g.PathTracer(0)
    try:
        for bad in (1, 73):
            with pytest.raises(g.PtError):
                t.set_option(g.OPT_PACKET_STACK, bad)
        with pytest.raises(g.PtError):
            t.set_option(g.OPT_FIRST_WALK, 2)
    finally:
        t.close()


def test_packet_counters_keep_per_ray_meaning():
    """depth 1 (bounce 0 only): rays are the same, every lane tests the same kind of candidates, and the wave steps of the packet
    walk are reported (union inflation = wave node steps per group over per-lane node visits per ray)"""
    _, bvh = bvh_of("cornell_dragon")
    W, H, spp = 640, 360, 16
    a = render(0, upload(bvh), W, H, spp, calls=1, depth=1, counters=True)
    b = render(1, upload(bvh), W, H, spp, calls=1, depth=1, counters=True)
    same(b, a, "depth 1")
    ca, cb = a[2], b[2]
    wb = cb   # (one dict holds the work counters and the wave statistics)
    assert ca["rays"] == cb["rays"] == W * H * spp
    assert cb["inner"] > 0 and cb["tris"] > 0 and cb["leaves"] > 0
    assert wb["act_node"] == cb["inner"] and wb["act_rec"] == cb["tris"]
    groups = wb["it_shade"]
    infl = (wb["it_node"] / groups) / (ca["inner"] / ca["rays"])
    print(f"per lane: {ca['inner'] / ca['rays']:.2f} nodes, {ca['tris'] / ca['rays']:.2f} records per ray; packet: {cb['inner'] / cb['rays']:.2f} "
          f"nodes, {cb['tris'] / cb['rays']:.2f} records per ray, {wb['it_node'] / groups:.2f} node steps and {wb['it_rec'] / groups:.2f} "
          f"record steps per group, {wb['act_node'] / max(wb['it_node'], 1):.1f} lanes per node step; union inflation {infl:.2f}")
    assert wb["it_node"] <= wb["act_node"] and wb["it_rec"] <= wb["act_rec"]


def test_bench_configuration_packet_equals_per_lane():
    """the bench step (1920x1080, 16 spp, depth 4, the 800k scene and bench.py's tree): the two walks' frames; any pixel that
    differs must hold the brute-force renderer's colour"""
    W, H, spp = 1920, 1080, 16
    mesh, _ = bvh_of("cornell_dragon_800k")
    tree = bvh_of("cornell_dragon_800k", split_alpha=-1.0)[1]
    opts = ((g.OPT_OPTIMIZE, 4), (g.OPT_REBUILD, 2))
    frames = [render(walk, upload(tree), W, H, spp, calls=1, options=opts) for walk in (0, 1)]
    ys, xs = np.nonzero(np.any(frames[0][0] != frames[1][0], axis=-1))
    print(f"bench configuration: {len(xs)} differing pixels of {W * H}")
    sph = g.reference_spheres()
    cam = golden_camera(W, H)
    for x, y in zip(xs, ys):
        q = g.default_params(W, H)
        q.frame, q.sample_index = 7, 1
        col, _, _ = orc.sample_pixels([(int(x), int(y))], sph, cam, q, spp, mesh=mesh)
        brute = orc.fold_samples(col, 1)[0]
        assert np.array_equal(frames[1][0][y, x], brute), f"packet walk differs from brute force at ({x},{y})"
    assert frames[1][0].any()
