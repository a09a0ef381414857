"""The Woop triangle test on the CPU: tests/woop_ref.py's restatement of pt_woop_intersect over its restatement of emit()'s records,
pair by pair against exact geometry, on the ray families a-f of woop_ref (dyadic grids, edge- and vertex-aimed rays, random rays,
both cull settings and reversed windings, slivers, a mesh far from the origin).  No GPU: tests/test_gpu_woop_rays.py holds the
device's records and its walks against the same verdicts.

Stated here, where they are checked: K = 6 (woop_ref.K_UV: the roundings between a record's row and u, counted in woop_ref's
docstring, tuned on nothing); at most 1 % of family c's rays may be undecided (measured: none)."""
import numpy as np
import pytest

import orc
import woop_ref as wr

ALL = wr.FAMILIES + wr.REVERSED
UNDECIDED_MAX = 0.01


def outside(name, cull, winners):
    """the rays whose answer is outside the acceptable set, and those of them that are decided"""
    V = wr.family_verdict(name, cull)
    off = ~V.accepts(winners)
    return np.nonzero(off)[0], np.nonzero(off & V.decided)[0]


@pytest.mark.parametrize("name", ALL)
def test_bound(name):
    """intersect32 over records() agrees with exact() in u, v, det and t within margins(), for every (ray, triangle) pair"""
    soup, rays = wr.family(name)
    C = wr.family_check(name)
    print(f"woop {name}: {len(rays)} rays x {len(soup)} triangles, largest error / margin: "
          + ", ".join(f"{k} {v:.3f}" for k, v in C.worst.items()))
    assert C.over == dict(u=0, v=0, det=0, t=0), f"{name}: pairs beyond the margin {C.over}, largest error / margin {C.worst}"
    if name == "a":     # every Woop quantity is exact on the dyadic grids
        assert C.worst == dict(u=0.0, v=0.0, det=0.0, t=0.0), C.worst


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ALL)
def test_consequence(name, cull):
    """intersect32's brute-force winner, with the walk's tie rule, lies in verdict's acceptable set for every ray"""
    V = wr.family_verdict(name, cull)
    off, _ = outside(name, cull, wr.family_check(name).winners[cull])
    print(f"woop {name} cull {cull}: decided {V.decided.mean():.4f}, largest du {V.du_max:.3e}")
    assert len(off) == 0, f"{name} cull {cull}: rays {off[:8]} answer {wr.family_check(name).winners[cull][off[:8]]}"


@pytest.mark.parametrize("cull", [1, 0])
def test_dyadic_grids_equal_brute_force(cull):
    """Family a: edges are unit axis vectors, |n|^2 = 1, rows in {0, +-1}, integer translations, t = 4, so Woop's answer is
    Moller-Trumbore's brute force exactly, ties to the smaller id.  No margin: one wrong ray fails."""
    soup, rays = wr.family("a")
    rec = wr.records(soup)
    assert set(np.unique(rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])) <= {-1.0, 0.0, 1.0} and np.array_equal(rec[:, [3, 7, 11]], np.round(rec[:, [3, 7, 11]]))
    t_b, id_b, _ = orc.trace_brute(wr.mesh_soup("grid")[1], rays, bool(cull))
    win = wr.family_check("a").winners[cull]
    assert np.array_equal(win, id_b), f"rays {np.nonzero(win != id_b)[0][:8]}"
    p = wr.intersect32_parts(rec, rays[:, 0:3], rays[:, 4:7])
    hit = win >= 0
    assert hit.sum() > 500 and np.all(p.t[np.nonzero(hit)[0], win[hit]] == 4.0) and np.all(t_b[hit] == 4.0)


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", [f for f in ALL if f.lstrip("~").startswith("c-")])
def test_random_rays_are_decided(name, cull):
    """the 1 % condition of family c: at most that share of the rays has more than one acceptable answer"""
    V = wr.family_verdict(name, cull)
    share = 1.0 - V.decided.mean()
    print(f"woop {name} cull {cull}: undecided {share:.4f}")
    assert share <= UNDECIDED_MAX


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", [f for f in ALL if f.lstrip("~")[0] == "b"] + ["f-small", "f-large"])
def test_sixty_four_du_decides(name, cull):
    """Family b (and its scaled copies; on the moved copy 64 du is as large as the triangles themselves, the cancellation that
    test_margin_follows_the_distance_from_the_origin measures, and only the rule of the verdict holds there): the aimed rays 64 du inside the edge are decided and hit the aimed triangle or a nearer certain one (or, the aimed triangle
    being culled or below EPS in area, whatever lies behind it: still one answer); those 64 du outside are decided and do not hit it"""
    A, V = wr.aim(name), wr.family_verdict(name, cull)
    win = wr.family_check(name).winners[cull]
    off = np.array([np.nan if f is None else f for f in A.offset])
    rows = np.arange(len(off))
    for f in (64, -64):
        m = off == f
        assert m.sum() > 0 and np.all(V.decided[m]), f"{name} cull {cull}: rays {rows[m & ~V.decided][:8]} at {f} du are undecided"
    inside = off == 64
    aimed_certain = V.certain[rows, A.tri]
    assert np.all(~aimed_certain[inside] | (win[inside] == A.tri[inside]) | (V.nearest[inside] == win[inside]))
    assert not np.any(win[off == -64] == A.tri[off == -64])
    if cull == 0 and name != "f-small":      # (scaled by 2^-6 the bunny's triangles fall below EPS in area: none is ever hit)
        assert np.all(aimed_certain[inside])


def test_slivers():
    """Family e: a triangle whose exact det is below EPS by more than the margin (|N| <= 0.77 EPS, or no area) is excluded for every
    ray, is never reported, and never hides what lies behind it (the consequence test: the winner is an acceptable answer, and
    these are none)."""
    soup, rays, kinds = wr.sliver_soup()
    gone = np.array([k in ("small", "flat") for k in kinds])
    v = soup.astype(np.float64).reshape(-1, 3, 3)
    e = np.sort(np.stack([np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=1) for i in range(3)], 1), 1)
    aspect = e[:, 2] / np.where(e[:, 0] > 0, e[:, 0], np.inf)
    assert aspect[2:].max() >= 2.0 ** 30 and np.isclose(aspect[2], np.sqrt(2.0)) and kinds.count("flat") == 2
    for cull in (1, 0):
        V = wr.family_verdict("e", cull)
        assert not np.any(V.certain[:, gone] | V.maybe[:, gone]), "a triangle below EPS is not excluded"
        win = wr.family_check("e").winners[cull]
        assert not np.any(gone[win[win >= 0]])
        thin = np.array([k == "thin" for k in kinds])
        print(f"woop e cull {cull}: winners by kind: ordinary {(win >= 0).sum() - thin[win[win >= 0]].sum()}, thin {thin[win[win >= 0]].sum()}, miss {(win < 0).sum()}")
        assert (win >= 0).sum() - thin[win[win >= 0]].sum() > 30, "the ordinary triangles behind the slivers are hardly ever reached"


@pytest.mark.parametrize("how", wr.MUTATIONS)
def test_sensitivity(how):
    """Each wrong record or rule puts at least one DECIDED ray outside its acceptable set: on family a, whose acceptable answer is
    brute force's for every ray, and (the record errors and the cull rule) on the aimed rays of the Cornell mesh."""
    soup, rays = wr.family("a")
    n_a = 0
    for cull in (1, 0):
        id_b = orc.trace_brute(wr.mesh_soup("grid")[1], rays, bool(cull))[1]
        n_a += int((wr.check_family("a", how).winners[cull] != id_b).sum())
    n_b = 0
    if how != "edge":
        win = wr.check_family("b-cornell", how).winners
        n_b = sum(len(outside("b-cornell", cull, win[cull])[1]) for cull in (1, 0))
    print(f"woop sensitivity {how}: family a {n_a} rays leave brute force, b-cornell {n_b} decided rays leave their sets")
    assert n_a > 0 and (how == "edge" or n_b > 0)


def test_margin_follows_the_distance_from_the_origin():
    """Family f.  Scaling by a power of two scales rows and rays exactly: every aimed ray's du is unchanged.  Moving the mesh by
    (2^10, -2^12, 2^8) leaves the edges as they were and takes |v2| from ~7 to ~4300: |rx.w| and sum |o_i rx_i| grow by that factor
    (rx.w = -rx . v2), and du with them — Woop's cancellation.  The derived margin must show it: the median du of the aimed rays
    grows by at least a quarter of the growth of the median |v2|, and by no more than four times that growth."""
    base = wr.aim("b-bunny_low")
    for how in ("small", "large"):
        A = wr.aim("f-" + how)
        assert np.array_equal(A.tri, base.tri) and np.allclose(A.du, base.du, rtol=1e-6, atol=0)
    A = wr.aim("f-moved")
    v2 = lambda name: np.median(np.linalg.norm(wr.family(name)[0].astype(np.float64)[:, 6:9], axis=1))
    growth, moved = np.median(A.du) / np.median(base.du), v2("f-moved") / v2("b-bunny_low")
    for name in ("b-bunny_low", "f-small", "f-large", "f-moved"):
        print(f"woop {name}: du of the aimed triangles: median {np.median(wr.aim(name).du):.3e}, largest {wr.aim(name).du.max():.3e}")
    print(f"woop f-moved: median |v2| grows {moved:.0f} x, median du {growth:.0f} x")
    assert moved / 4 <= growth <= 4 * moved
