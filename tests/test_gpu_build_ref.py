"""pt_build_bvh against the sequential restatement of its builders (tests/build_ref.py), tree for tree: the item buffer the device
builds equals the reference's up to the numbering of its nodes (tree_audit.canonical_form), byte for byte, and so do the counts.
No ray, no frame, no tolerance.  The other builder suites prove that whatever is built is a VALID tree; this one that it is the
tree the builder describes: the key, the sort, Karras' ranges, PLOC's window, ties and merges, the cut rule, the collapse order,
the pre-split's slabs.

What each mesh is there for (build_ref.case_soup, gpu_support.builder_mesh):
  cube, cornell, bunny_low, gto_sixteen, needles   the meshes of test_gpu_tree_audit's strict audit
  soup-1 .. soup-5        the doubled lone triangle, the two-leaf Karras tree, wide roots with fewer than four children
  soup-16 .. soup-18      PLOC's +-8 window clipped at both ends, and for the first time not clipped
  soup-255 .. soup-257    the `live` masks of k_tri_bounds' block reduction: the extreme centres are in the last, partly filled block
  soup-1000               several blocks
  window                  PLOC's window by design: a pair exactly 8 places apart merges, one 9 apart (and nearer) does not
  pairs                   every fifth triangle twice: equal keys told apart by position, PLOC area ties
  flat                    no centre extent on one axis
  co-centred              forty boxes around one centre: no centre extent at all, every key equal, PLOC one merge per round
  co-centred-far          the same and one distant triangle: among the forty only the size bits differ
  two-scales              wall-sized triangles around tiny ones: rel over the nine size bits, some clamped
  at-the-max              one triangle per axis holds the largest centre coordinate (u == 1)
  minus-zero              -0.0f in v0.x and elsewhere
pt_tree_cost is held to build_ref.tree_cost over the downloaded items: both add the same binary64 terms in different orders.
"""
import numpy as np
import pytest

import build_ref as br
import gpu_pathtracer_amd as g
import tree_audit as ta
from gpu_support import BUILDER_ASSETS, builder_mesh

pytestmark = pytest.mark.gpu

MESHES = BUILDER_ASSETS + ("needles",) + br.SYNTHETIC
PRESPLIT = [(name, ps) for name in ("needles", "gto_sixteen", "two-scales", "needles-63", "needles-64") for ps in (50, 200)]


@pytest.fixture(scope="module")
def ctx():
    tr = g.PathTracer(0)
    try:
        yield tr
    finally:
        tr.close()


def device_tree(t, name, algo, leaf_max, presplit=0):
    for opt, val in ((g.OPT_OPTIMIZE, 0), (g.OPT_REBUILD, 0), (g.OPT_TRI_TEST, 0), (g.OPT_PRESPLIT, presplit), (g.OPT_BUILD_ALGO, algo),
                     (g.OPT_LEAF_MAX, leaf_max)):
        t.set_option(opt, val)
    t.build_bvh(builder_mesh(name)[0])
    return t.tree_items()


def reference_tree(name, algo, leaf_max, presplit=0):
    return br.cached_build(name, lambda: builder_mesh(name)[1:3], algo, leaf_max, presplit)


def same_tree(t, name, algo, leaf_max, presplit=0):
    B, R, W, wd = device_tree(t, name, algo, leaf_max, presplit)
    rB, rR, rW, rinfo, rwd = reference_tree(name, algo, leaf_max, presplit)
    what = f"{name} algo {algo} leaf_max {leaf_max} presplit {presplit}"
    diff = br.first_difference((B, R, W), (rB, rR, rW))
    assert diff is None, f"{what}: the device tree is not the reference's; first stage that differs: {diff}"
    assert ta.canonical_form(B, R, W) == ta.canonical_form(rB, rR, rW), what
    info = {k: v for k, v in t.scene_info().items() if k != "device_bytes"}
    assert info == rinfo, f"{what}: pt_scene_info {info}, the reference {rinfo}"
    assert (wd, len(W)) == (rwd, len(rW)), f"{what}: wide depth / nodes {(wd, len(W))}, the reference {(rwd, len(rW))}"


@pytest.mark.parametrize("leaf_max", [1, 2, 4, 8])
@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name", MESHES)
def test_device_builds_the_reference_tree(ctx, name, algo, leaf_max):
    same_tree(ctx, name, algo, leaf_max)


@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name,presplit", PRESPLIT)
def test_presplit_builds_the_reference_tree(ctx, name, presplit, algo):
    same_tree(ctx, name, algo, 2, presplit)


# ------------------------------------------------------------------------------------------------------------ tree cost
def cost_matches(t, what):
    """Both figures are binary64 sums of the same positive terms (build_ref.tree_cost restates k_tree_cost's terms exactly) in
    different orders: each sum is within (terms) x 2^-53 of the exact one, relative; a factor 4 for the final divisions."""
    B, R, W, _ = t.tree_items()
    got = t.tree_cost()
    want = br.tree_cost(W, len(B), len(R), records=R)
    for fig, g_, w_, terms in zip(("node_visits", "tri_tests"), got, want, br.cost_terms(W)):
        bound = 4.0 * terms * 2.0 ** -53
        print(f"{what}: {fig} {g_!r} / reference {w_!r}, relative difference {abs(g_ - w_) / w_:.3e}, bound {bound:.3e} ({terms} terms)")
        assert abs(g_ - w_) <= bound * w_, f"{what}: {fig} {g_!r}, the reference {w_!r}: more than {bound:.3e} apart"


@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name", MESHES)
def test_tree_cost_of_device_trees(ctx, name, algo):
    device_tree(ctx, name, algo, 2)
    cost_matches(ctx, f"{name} algo {algo}")


@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name,presplit", PRESPLIT)
def test_tree_cost_of_presplit_trees(ctx, name, presplit, algo):
    device_tree(ctx, name, algo, 2, presplit)
    cost_matches(ctx, f"{name} algo {algo} presplit {presplit}")


_host = {}


@pytest.mark.parametrize("rebuild", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "gto_sixteen"])
def test_tree_cost_of_host_route_trees(ctx, name, rebuild):
    for opt, val in ((g.OPT_OPTIMIZE, 0), (g.OPT_REBUILD, rebuild), (g.OPT_TRI_TEST, 0), (g.OPT_PRESPLIT, 0), (g.OPT_BUILD_ALGO, 1), (g.OPT_LEAF_MAX, 2)):
        ctx.set_option(opt, val)
    if name not in _host:
        _host[name] = g.Bvh(builder_mesh(name)[0])
    ctx.upload_bvh(_host[name])
    assert (ctx.last_build_ms() >= 0) == (rebuild == 1)
    cost_matches(ctx, f"{name} uploaded, PT_OPT_REBUILD {rebuild}")
