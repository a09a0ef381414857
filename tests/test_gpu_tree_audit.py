"""The trees in device memory, item by item, against exact geometry (tests/tree_audit.py): every writer of the
[binary nodes][records][wide nodes] buffer — host re-layout, host optimiser, device builder, pre-split, refit and the options
that chain them — is built / uploaded / refit, downloaded through pt_tree_items and audited.  No ray, no frame, no tolerance.

Audit level per tree kind (README of the checks: tree_audit.audit):
  pt_build_bvh, PT_OPT_REBUILD 1 (device-built)      strict: boxes = min / max of the vertices beneath, wide nodes = the restated encoder
  ... optimised on the host (PT_OPT_OPTIMIZE)        shape, records, containment, coverage
  pt_upload_bvh of the host builder's hierarchy      shape, records, containment, coverage (its spatial splits clip leaf boxes)
  PT_OPT_PRESPLIT                                    shape, records, containment, coverage; n_tri_refs > n_tris
  Woop records (PT_OPT_TRI_TEST 1)                   shape and containment of the node part; the records against the restated encoder
                                                     (1 ulp per row float, N and the id word exact) and against their own vertices
  any tree after pt_refit_bvh                        strict against the moved soup (+ coverage after the twist)
Two checks are narrower on device-built trees, for reasons in the builder's code: with PT_OPT_LEAF_MAX > 1 the binary section keeps
the nodes below its multi-record leaves (ptb_is_cut, pt_build.h: unreachable, n_inner is the section's size) and max_depth counts
those cut-off levels too (k_depth, pt_build.h), so it bounds the walked depth instead of equalling it; with PT_OPT_LEAF_MAX 1 both
are exact.  The plane checks use tree_audit.fma32_fast at every triangle count: it re-decides every possible double rounding
exactly, so there is no count above which the audit is less exact.
"""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import tree_audit as ta
from gpu_support import needles, soup_mesh, twist

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_NO_SCENE = -1, -3


# ---------------------------------------------------------------------------------------------------------------- meshes
_SOUPS = {}


def soup_of(name):
    if name not in _SOUPS:
        s = needles() if name == "needles" else g.scene_mesh(name).triangle_soup()
        s.setflags(write=False)
        _SOUPS[name] = s
    return _SOUPS[name]


def mesh_of(name):
    return soup_mesh(soup_of(name)) if name == "needles" else g.scene_mesh(name)


TWIST = (0.8, (0.05, -0.02, 0.03))   # gpu_support.twist's amount and shift for every refit of this module


# --------------------------------------------------------------------------------------------------------------- helpers
def reset(t):
    for opt, val in ((g.OPT_OPTIMIZE, 0), (g.OPT_REBUILD, 0), (g.OPT_PRESPLIT, 0), (g.OPT_BUILD_ALGO, 1), (g.OPT_LEAF_MAX, 2), (g.OPT_TRI_TEST, 0)):
        t.set_option(opt, val)


def items(t):
    B, R, W, wd = t.tree_items()
    return B.copy(), R.copy(), W.copy(), wd


def check(t, soup, what, **kw):
    B, R, W, wd = t.tree_items()
    v = ta.audit(B, R, W, t.scene_info(), soup, wide_depth=wd, **kw)
    print(f"{what}: {len(B)} binary, {len(R)} records, {len(W)} wide nodes, depth {t.scene_info()['max_depth']} / {wd}: {len(v)} violations")
    assert v == [], what + "\n" + "\n".join(f"{x.kind} | {x.item} | {x.what}" for x in v[:12])


def same_items(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.fixture()
def t():
    tr = g.PathTracer(0)
    try:
        reset(tr)
        yield tr
    finally:
        tr.close()


def device_kw(leaf_max):
    return dict(leaf_max=max(leaf_max, 1), cut_subtrees=True, depth_exact=leaf_max <= 1)


# -------------------------------------------------------------------------------------------------------------- accessor
def test_accessor_errors_and_counts(t):
    import ctypes as C
    lib, p = t._lib, C.c_void_p()
    assert lib.pt_tree_items(t._ctx, C.byref(p), None, None, None, None) == PT_ERR_NO_SCENE
    assert lib.pt_tree_items(None, C.byref(p), None, None, None, None) == PT_ERR_INVALID
    t.build_bvh(mesh_of("cube"))
    assert lib.pt_tree_items(t._ctx, None, None, None, None, None) == PT_ERR_INVALID
    assert lib.pt_tree_items(t._ctx, C.byref(p), None, None, None, None) == 0 and p.value
    B, R, W, wd = t.tree_items()
    info = t.scene_info()
    assert (len(B), len(R)) == (info["n_inner"], info["n_tri_refs"]) and len(W) >= 1 and wd >= 1
    assert B.shape[1] == R.shape[1] == W.shape[1] == 16


# -------------------------------------------------------------------------------------------------------------- builders
@pytest.mark.parametrize("leaf_max", [1, 2, 4, 8])
@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("name", ["cube", "cornell", "bunny_low", "gto_sixteen", "needles"])
def test_device_builders_are_strict(t, name, algo, leaf_max):
    t.set_option(g.OPT_BUILD_ALGO, algo)
    t.set_option(g.OPT_LEAF_MAX, leaf_max)
    t.build_bvh(mesh_of(name))
    check(t, soup_of(name), f"{name} algo {algo} leaf_max {leaf_max}", strict=True, **device_kw(leaf_max))


# ------------------------------------------------------------------------------------------------------------ host route
_BVHS = {}


def host_bvh(name):
    if name not in _BVHS:
        _BVHS[name] = g.Bvh(mesh_of(name))
    return _BVHS[name]


@pytest.mark.parametrize("rebuild", [0, 1, 2])
@pytest.mark.parametrize("optimize", [0, 2])
@pytest.mark.parametrize("leaf_max", [0, 2])
@pytest.mark.parametrize("name", ["cube", "cornell", "bunny_low", "gto_sixteen"])
def test_host_route(t, name, leaf_max, optimize, rebuild):
    t.set_option(g.OPT_LEAF_MAX, leaf_max)
    t.set_option(g.OPT_OPTIMIZE, optimize)
    t.set_option(g.OPT_REBUILD, rebuild)
    t.upload_bvh(host_bvh(name))
    what = f"{name} leaf_max {leaf_max} optimize {optimize} rebuild {rebuild}"
    device_built = t.last_build_ms() >= 0
    assert device_built if rebuild == 1 else (rebuild == 2 or not device_built)
    if device_built and optimize == 0:
        check(t, soup_of(name), what + " (device-built)", strict=True, **device_kw(leaf_max))
    elif device_built:      # re-clustered, then through the host optimiser and emit: unique ids, unions as boxes
        check(t, soup_of(name), what + " (device-built, optimised)", coverage=True, leaf_max=max(leaf_max, 1))
    else:
        check(t, soup_of(name), what + " (host hierarchy)", split_refs=True, coverage=True, leaf_max=leaf_max)


@pytest.mark.parametrize("name", ["cornell", "gto_sixteen"])
def test_woop_records(t, name):
    """Woop rows are made in binary64 on the host.  The node part: shape, counts and containment (the wide boxes against the binary
    tree's leaf boxes).  The record part (tree_audit.audit, woop=True): every row float within 1 ulp of the restated encoder's
    (tree_audit.encode_woop_records), N and the id << 1 | last word bit for bit, and the stored rows, taken in binary64, send the
    triangle's own vertices to (1,0,0), (0,1,0), (0,0,0) within 2^-24 per entry times the magnitudes summed.  No coverage."""
    t.set_option(g.OPT_TRI_TEST, 1)
    t.upload_bvh(host_bvh(name))
    check(t, soup_of(name), f"{name} woop", woop=True, split_refs=True, leaf_max=2)


# ------------------------------------------------------------------------------------------------------------- pre-split
@pytest.mark.parametrize("presplit", [50, 100, 200])
@pytest.mark.parametrize("name", ["gto_sixteen", "bunny_low", "needles"])
def test_presplit_covers_every_triangle(t, name, presplit):
    t.set_option(g.OPT_PRESPLIT, presplit)
    t.build_bvh(mesh_of(name))
    info = t.scene_info()
    print(f"{name} presplit {presplit}: {info['n_tri_refs']} references of {len(soup_of(name))} triangles")
    check(t, soup_of(name), f"{name} presplit {presplit}", split_refs=True, coverage=True, **device_kw(2))
    assert info["n_tri_refs"] > len(soup_of(name))


# ----------------------------------------------------------------------------------------------------------------- refit
TREES = ("device", "lbvh", "host", "optimize", "rebuild2", "presplit")


def install(t, name, kind):
    reset(t)
    if kind in ("device", "lbvh", "presplit"):
        t.set_option(g.OPT_BUILD_ALGO, 0 if kind == "lbvh" else 1)
        t.set_option(g.OPT_PRESPLIT, 100 if kind == "presplit" else 0)
        t.build_bvh(mesh_of(name))
    else:
        t.set_option(g.OPT_OPTIMIZE, 2 if kind in ("optimize", "rebuild2") else 0)
        t.set_option(g.OPT_REBUILD, 2 if kind == "rebuild2" else 0)
        t.upload_bvh(host_bvh(name))
    device_made = kind in ("device", "lbvh", "presplit") or (kind == "rebuild2" and t.last_build_ms() >= 0)
    cut = kind in ("device", "lbvh", "presplit")     # (an optimised tree went through emit: no cut-off nodes, exact depth)
    return dict(leaf_max=2, split_refs=kind in ("host", "optimize", "rebuild2", "presplit") and not (kind == "rebuild2" and device_made),
                cut_subtrees=cut, depth_exact=not cut)


def refit_mesh(kind):
    return "gto_sixteen" if kind in ("host", "presplit") else "bunny_low"


@pytest.mark.parametrize("kind", TREES)
def test_refit_round_trip_is_byte_exact(t, kind):
    name = refit_mesh(kind)
    soup = soup_of(name)
    install(t, name, kind)
    built = items(t)
    t.refit_bvh(np.array(soup))
    own = items(t)
    if kind in ("device", "lbvh"):
        assert same_items(own, built), "a refit to the vertices the device tree was built from changed it"
    t.refit_bvh(twist(soup, *TWIST))
    assert not same_items(items(t), own)
    t.refit_bvh(np.array(soup))
    assert same_items(items(t), own), "a refit back does not reproduce the refit to the own vertices"
    assert np.array_equal(built[1].view(np.int32), own[1].view(np.int32)), "records changed under a refit to their own vertices"


@pytest.mark.parametrize("kind", TREES)
def test_refit_to_twisted_vertices_is_strict_and_covers(t, kind):
    name = refit_mesh(kind)
    kw = install(t, name, kind)
    moved = twist(soup_of(name), *TWIST)
    t.refit_bvh(moved)
    check(t, moved, f"{name} {kind} twisted", strict=True, coverage=True, **kw)


def leaves_of_one_wide_node(t):
    """ids of every record below a wide node whose children are all leaves, and of one more leaf elsewhere."""
    B, R, W, _ = t.tree_items()
    Wi, Ri, base = W.view(np.int32), R.view(np.int32), 4 * len(B)
    out = []
    for w in range(len(W) - 1, -1, -1):
        if np.all(Wi[w, 10:14] < 0):
            for link in set(Wi[w, 10:14].tolist()):
                j = ((~link & ~3) - base) // 4
                while True:
                    out.append(int(Ri[j, 3]))
                    if Ri[j, 7]:
                        break
                    j += 1
            break
    j = 0
    while True:
        out.append(int(Ri[j, 3]))
        if Ri[j, 7]:
            break
        j += 1
    return [i for i in out if i >= 0]


@pytest.mark.parametrize("kind", TREES)
def test_refit_with_dropped_triangles(t, kind):
    name = refit_mesh(kind)
    soup = soup_of(name)
    kw = install(t, name, kind)
    rng = np.random.default_rng(3)
    drop = np.union1d(rng.choice(len(soup), len(soup) // 20, replace=False), leaves_of_one_wide_node(t)).astype(np.int64)
    bad = np.array(soup)
    for i, r in enumerate(drop):
        bad[r, rng.integers(9)] = (np.nan, np.inf, -np.inf, np.float32(3.2e38), np.float32(-3.2e38))[i % 5]
    mask = np.zeros(len(soup), bool)
    mask[drop] = True
    cnt = t.malloc(4)
    t.refit_bvh(bad, n_dropped=cnt)
    t.sync()
    assert int(cnt.download(np.uint32, (1,))[0]) == len(drop)
    check(t, soup, f"{name} {kind} with {len(drop)} dropped", strict=True, dropped=mask, **kw)
    cnt.free()


# -------------------------------------------------------------------------------------------------- edges of the encoder
def edge_soups():
    rng = np.random.default_rng(17)
    small = rng.uniform(-1, 1, (60, 3, 3))
    flat = small.copy()
    flat[:, :, 1] = 0.25
    one = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float64)
    near_big = np.float32(1.0e30).astype(np.float64) + rng.integers(0, 6, (40, 3, 3)) * float(np.spacing(np.float32(1.0e30)))
    cluster = rng.uniform(0, 1.0e-4, (80, 3, 3)) + 5.0
    huge = np.array([[[-4.0e3, 0, 0], [6.0e3, 1.0e3, 0], [0, -2.0e3, 8.0e3]]])
    zeros = small.copy()
    zeros[::3, 0, 0] = -0.0
    zeros[1::3, :, 2] = -0.0
    zeros[2::5, 1, :] = -0.0
    zeros[5] = [[-0.0, -0.0, -0.0], [0.0, 1.0, 0.0], [-0.0, 0.0, 1.0]]
    ints = rng.integers(0, 256, (90, 3, 3)).astype(np.float64)
    ints[0, 0], ints[0, 1] = 0, 255
    return {
        "flat": flat, "identical-300": np.repeat(small[:1], 300, 0), "one": one.reshape(1, 3, 3), "two": small[:2],
        "near-1e30": near_big, "near-1e-30": small * 1.0e-30, "eight-orders": np.concatenate([huge, cluster]),
        "negative-zero": zeros, "on-grid-planes": ints,
    }


EDGES = ("flat", "identical-300", "one", "two", "near-1e30", "near-1e-30", "eight-orders", "negative-zero", "on-grid-planes")


@pytest.mark.parametrize("algo", [0, 1], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("case", EDGES)
def test_encoder_edges_built_then_refit(t, case, algo):
    soup = np.ascontiguousarray(edge_soups()[case], np.float32).reshape(-1, 9)
    t.set_option(g.OPT_BUILD_ALGO, algo)
    t.build_bvh(soup_mesh(soup))
    check(t, soup, f"{case} built", strict=True, **device_kw(2))
    built = items(t)
    if case == "flat":
        assert np.any(built[2][:, 14] == ta.F32_MIN_NORMAL), "a flat node takes the smallest normal step"
    t.refit_bvh(soup)
    assert same_items(items(t), built), f"{case}: a refit to the own vertices changed the tree"
    moved = (soup * np.float32(0.75)).astype(np.float32)
    t.refit_bvh(moved)
    check(t, moved, f"{case} refit", strict=True, **device_kw(2))


def test_an_extent_that_overflows_binary32_is_refused(t):
    """|x| <= 3.0e38 holds, hi - lo does not fit binary32: pt_encode_wide_node's step would be infinite.  pt_build_bvh refuses
    (include/ptmi.h) and the tree on the context stays.  Built only: nothing is traced over such coordinates."""
    t.build_bvh(mesh_of("cube"))
    before = items(t)
    soup = np.array([[-2e38, 0, 0, -2e38, 1, 0, -2e38, 0, 1], [2e38, 0, 0, 2e38, 1, 0, 2e38, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    with pytest.raises(g.PtError) as e:
        t.build_bvh(soup_mesh(soup))
    assert e.value.code == PT_ERR_INVALID
    assert same_items(items(t), before)
