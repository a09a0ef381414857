"""The oracle's estimators against closed-form radiance (tests/estimator_ref.py), on the CPU.

The GPU suites pin the kernels to oracle/pt_oracle.c bit for bit, and both were written from one header: a weight, a density or
an eligibility rule that both share would pass every parity test.  Here each of them — sphere- and triangle-light NEE, the
shadow ray's t_max, the spheres past the first 8, "inside the light", the Phong lobe, Schlick and the glass split, both roulettes,
the default DIFF lobe — has to produce the radiance geometry says it must.  Every case runs twice: closest hits from the walk
over g.Bvh(mesh), and from the brute-force loop over the raw triangles (the arbiter of gpu_support.arbitrate / judge), which
has to trace the shadow rays and know the triangle lights too."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import estimator_ref as ref
import orc

CASES = ref.cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------------- the closed forms
def test_sphere_form_factor_against_the_cone_quadrature():
    """(r / d)^2 cos(theta) is the integral of cos / pi over the sphere's cone"""
    for c, r in ((ref.A_C, ref.A_R), (ref.S_C, ref.S_R), (ref.P + (3.0, 3.0, 2.0), 2.4)):
        F = ref.sphere_form_factor(c, r)
        Q = ref.cone_integral(ref.lambert_density(), *ref.sphere_cone(c, r))
        assert abs(Q - F) <= 1e-6 * F, (c, r, F, Q)


def test_lamberts_formula_against_the_area_quadrature():
    """the contour formula is the integral of cos cos' / (pi d^2) over the triangle, whatever the winding; and a triangle that
    fills the whole sky above a point has F -> 1"""
    F = ref.polygon_form_factor(ref.TRI)
    assert F == pytest.approx(ref.polygon_form_factor([ref.TRI[0], ref.TRI[2], ref.TRI[1]]), rel=1e-12)
    Q = ref.triangle_area_form_factor(ref.TRI)
    assert abs(Q - F) <= 1e-5 * F, (F, Q)
    huge = [ref.P + (-1e4, 1.0, -1e4), ref.P + (3e4, 1.0, -1e4), ref.P + (-1e4, 1.0, 3e4)]
    assert ref.polygon_form_factor(huge) == pytest.approx(1.0, abs=1e-3)


def test_the_lobe_quadratures_have_converged():
    """400 x 400 against 800 x 800 midpoints: 1e-6 relative, for every lobe and probe of cases C and F; each density integrates
    to 1 over the hemisphere"""
    for name in ("C-phong20", "C-phong5", "F-default-lobe"):
        c = BY_NAME[name]
        cone = ref.sphere_cone(c.rows[0][0][:3], c.rows[0][0][3])
        dens = ref.default_lobe_density() if name.startswith("F") else ref.phong_density(c.phong, ref.UP)
        a, b = ref.cone_integral(dens, *cone, N=400), ref.cone_integral(dens, *cone, N=800)
        assert abs(a - b) <= 1e-6 * b, (name, a, b)
    for dens in (ref.phong_density(20.0, ref.UP), ref.phong_density(5.0, ref.UP), ref.lambert_density(), ref.uniform_density()):
        # (the midpoint rule's own error over the whole hemisphere: h^2 / 24 * f'(1) = 21 * 20 / (24 * 800^2) = 2.7e-5 for cos^20)
        assert ref.cone_integral(dens, ref.UP, np.pi / 2, N=800) == pytest.approx(1.0, rel=1e-4)
    # the default lobe's density is singular (integrably) at the normal: leave a 1e-3 cap out, which holds sin = 1e-3 of the mass
    k = (np.arange(4000) + 0.5) / 4000
    th = 1e-3 + k * (np.pi / 2 - 1e-3)
    w = np.stack([np.sin(th), np.cos(th), np.zeros_like(th)], -1)
    mass = (ref.default_lobe_density()(w) * 2 * np.pi * np.sin(th)).mean() * (np.pi / 2 - 1e-3)
    assert mass == pytest.approx(1.0 - np.sin(1e-3), rel=1e-6)


def test_schlick_at_its_ends():
    assert ref.schlick(1.0) == pytest.approx(0.04) and ref.schlick(0.0) == pytest.approx(1.0)
    assert 0.04 < ref.schlick(0.5) < ref.schlick(0.3) < 1.0


def test_no_sample_can_reach_the_clamp():
    """every case's expectation lies in [0, 1), and the zero and fixed cases are the ones the table says"""
    assert len(CASES) == len(BY_NAME)
    for c in CASES:
        assert (c.E >= 0).all() and (c.E < 1).all(), c
        assert (c.kind == "zero") == (not c.E.any()), c
    assert {c.name for c in CASES if c.kind == "fixed"} == {"D-below70", "E-plain-depth3", "E-plain-depth12", "E-roulette-depth3",
                                                            "E-cpu-roulette-depth3"}


# ---------------------------------------------------------------------------------------------------- the oracle
def oracle_samples(case, hits):
    """2^log2_n one-sample paths of one pixel, through the tree or the brute-force loop: the colours before the fold [n][3]"""
    p = case.params(3, 3)
    scene = dict(bvh=g.Bvh(case.mesh)) if hits == "tree" else dict(mesh=case.mesh)
    lights = orc.tri_lights(case.mesh, case.materials, case.tri_material) if case.materials is not None else None
    col, _, _ = orc.sample_pixels([(1, 1)], case.spheres(), case.camera(3, 3), p, 1 << case.log2_n, materials=case.materials,
                                  tri_material=case.tri_material, lights=lights, **scene)
    return col[0]


@pytest.mark.parametrize("hits", ("tree", "brute"))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_oracle_holds_the_closed_form(case, hits):
    """|mean - E| <= 5 standard errors per channel at 2^16 samples (2^19 for F); a zero-variance case holds E within 1e-5 E in
    every sample (at most about a dozen binary32 roundings, with a margin of five), a dark one is exactly 0; no sample reaches 1.
    In brute-force mode the triangle-light and occluder cases (B, BA, I, J, J2 under NEE) fail unless the arbiter traces its
    shadow rays and is given the light list."""
    x = oracle_samples(case, hits)
    problems, z, rel = ref.verdict(case, x)
    print(f"{case.name} [{hits}]: E {case.E}, {case.kind} z {np.round(z, 2)}, SE / E {np.round(rel, 4)}, largest sample {x.max():.3f}")
    assert not problems, (case.name, hits, problems)
    assert x.max() < 1.0


def test_the_default_lobe_is_not_a_uniform_hemisphere():
    """Case F at 2^19 samples, judged against the integral of 1 / (2 pi) over the probe: off by more than 10 standard errors in
    every channel, while cos / (2 pi sin) holds (above).  So the test tells the two densities apart."""
    case = BY_NAME["F-default-lobe"]
    m, se = ref.mean_and_se(oracle_samples(case, "tree"))
    z_alt = (m - case.alt) / se
    print(f"against 1 / (2 pi): {z_alt} standard errors; against cos / (2 pi sin): {(m - case.E) / se}")
    assert (np.abs(z_alt) > 10).all()


def test_the_arbiter_sees_a_shadow():
    """J-below, NEE at depth 1: the black triangle hides the light from P, so every sample is 0 — with the tree and in
    brute-force mode, bit for bit the same samples; and with the occluder above the light both modes agree sample by sample too"""
    for name in ("J-below-nee1", "J-above-nee1", "BA-nee1"):
        tree, brute = oracle_samples(BY_NAME[name], "tree"), oracle_samples(BY_NAME[name], "brute")
        assert np.array_equal(tree.view(np.int32), brute.view(np.int32)), name
        assert tree.any() == (name != "J-below-nee1")
