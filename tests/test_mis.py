"""PT_FLAG_MIS on the CPU: the flag and its contract are there, and the float64 restatement tests/mis_ref.py — the reference of
tests/test_gpu_mis.py — is itself held against geometry: the two weights of one direction sum to one, computed from the two
sides' own formulas; the MIS estimator is unbiased against the closed forms of estimator_ref and env_light_ref; and the two scenes
MIS is for show its win with margin (a standard-error ratio of at most 0.35 where the GPU test asserts 0.5)."""
import os

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_light_ref
import estimator_ref as ref
import mis_ref
from mis_ref import X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_flag_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert "PT_FLAG_MIS = 1u << 9" in header and "#define PTMI_ABI_VERSION 3" in header
    assert g.FLAG_MIS == 1 << 9 and g._abi.FLAG_MIS == g.FLAG_MIS
    for left_out in ("power heuristic", "one-sample MIS", "Phong lobe"):
        assert left_out in header, left_out
    assert "--mis" in open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read()


# ---------------------------------------------------------------------------------------------------- weights
def test_sphere_weights_sum_to_one():
    """1000 seeded directions inside the cone of sphere A: w_l from the light's centre and radius, w_b from the direction that
    hits it — the same density by construction (the cone's), so this pins bounce_weight against light_weight"""
    rng = np.random.default_rng(5)
    c, r = ref.f32(ref.A_C), float(ref.f32(ref.A_R))
    w = c - X
    wn = w / np.linalg.norm(w)
    cos_max = np.sqrt(1.0 - r * r / (w @ w))
    cos_t = 1.0 - rng.random(1000) * (1.0 - cos_max) * 0.999
    t1, b1 = mis_ref.frame(wn)
    ph = 2.0 * np.pi * rng.random(1000)
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    d = (np.sin(ph) * sin_t)[:, None] * t1 + cos_t[:, None] * wn + (np.cos(ph) * sin_t)[:, None] * b1
    assert np.isfinite(mis_ref.hit_sphere(X, d, c, r)).all()
    cosl = d @ ref.UP
    for n_all in (1, 3):
        wl = mis_ref.light_weight(mis_ref.pk_sphere(c, r), n_all, cosl)
        wb = mis_ref.bounce_weight(mis_ref.pk_sphere(c, r), n_all, cosl / np.pi)
        assert np.abs(wl + wb - 1.0).max() <= 1e-12 and (wl > 0).all() and (wb > 0).all()


@pytest.mark.parametrize("verts", [ref.TRI, mis_ref.NEAR_TRI], ids=["TRI", "S-near"])
def test_triangle_weights_sum_to_one(verts):
    """1000 seeded points on the triangle: w_l from d2 / proj of the light's vertices, w_b from t^2 / |N . d| of the ray that hits it"""
    rng = np.random.default_rng(6)
    v0, v1, v2 = (ref.f32(v) for v in verts)
    su, u2 = np.sqrt(rng.random(1000)), rng.random(1000)
    pl = v0 + (1.0 - su)[:, None] * (v1 - v0) + (u2 * su)[:, None] * (v2 - v0)
    d = pl - X
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = mis_ref.hit_triangle(X, d, (v0, v1, v2))
    inside = np.isfinite(t)
    assert inside.mean() > 0.99   # (a point drawn on an edge can miss by rounding)
    cosl = d @ ref.UP
    for n_all in (1, 2):
        wl = mis_ref.light_weight(mis_ref.pk_triangle_from_light((v0, v1, v2), pl), n_all, cosl)
        wb = mis_ref.bounce_weight(mis_ref.pk_triangle_from_hit(np.cross(v0 - v1, v0 - v2), d, t), n_all, cosl / np.pi)
        err = np.abs(wl + wb - 1.0)[inside]
        print(f"n_all {n_all}: largest |w_l + w_b - 1| = {err.max():.2e}; w_l in {wl[inside].min():.4f} .. {wl[inside].max():.4f}")
        assert err.max() <= 1e-12


def test_map_weights_sum_to_one():
    """1000 seeded draws from the tables of a gradient map, interior to their texel: w_l from the draw's density, w_b from the
    density of the drawn direction"""
    import env_ref
    tex = env_ref.gradient_map(16, 8)
    tab = env_light_ref.Tables(tex, False)
    u = np.random.default_rng(7).random((3000, 2)).astype(np.float32)
    s = env_light_ref.draw(tab, u)
    keep = np.flatnonzero(env_light_ref.interior(s) & (s["d"] @ ref.UP > 0))[:1000]
    assert len(keep) == 1000
    d, pdf = s["d"][keep], s["pdf"][keep].astype(np.float64)
    back = env_light_ref.pdf_of(tab, d).astype(np.float64)
    cosl = d @ ref.UP
    wl, wb = mis_ref.light_weight(pdf, 2, cosl), mis_ref.bounce_weight(back, 2, cosl / np.pi)
    assert np.abs(wl + wb - 1.0).max() <= 1e-12
    assert (mis_ref.bounce_weight(np.zeros(3), 2, 0.2) == 1.0).all()   # a direction the tables never draw is the bounce's alone


# ---------------------------------------------------------------------------------------------------- unbiased
def report(name, est, E):
    out = {}
    for k in ("plain", "nee", "mis"):
        m, se = ref.mean_and_se(est[k])
        out[k] = (m, se)
        print(f"{name:8s} {k:5s} mean {m} SE {se} z {(m - E) / np.where(se > 0, se, 1)}")
    return out


@pytest.mark.parametrize("name", list(mis_ref.SCENES))
def test_the_restatement_is_unbiased_on_the_closed_form_scenes(name):
    E = next(c.E for c in ref.cases() if c.name == f"{name}-nee1")
    st = report(name, mis_ref.estimate(mis_ref.SCENES[name](), 16), E)
    for k, (m, se) in st.items():
        assert (np.abs(m - E) <= 5 * se).all(), k


def test_the_restatement_is_unbiased_under_the_one_texel_sun():
    E = mis_ref.sun_E()
    st = report("S-sun", mis_ref.estimate(mis_ref.sun_scene(), 16), E)
    for k, (m, se) in st.items():
        assert (np.abs(m - E) <= 5 * se).all(), k


# ---------------------------------------------------------------------------------------------------- the two wins
def test_s_near_light_sampling_is_poor_and_mis_wins():
    v = [ref.f32(p) for p in mis_ref.NEAR_TRI]
    side = [np.linalg.norm(v[i] - v[(i + 1) % 3]) for i in range(3)]
    centroid = sum(v) / 3.0
    assert 7.0 <= min(side) and max(side) <= 9.0 and all(abs(p[1] - 0.25) < 1e-6 for p in v)
    assert np.isfinite(mis_ref.hit_triangle(X, ref.UP[None, :] * np.ones((1, 3)), v)).all(), "P lies below the triangle's interior"
    assert np.hypot(centroid[0] - ref.P[0], centroid[2] - ref.P[2]) > 0.5, "... and off its centroid"
    E = mis_ref.near_E()
    print(f"E at the lifted point {E}, at P {mis_ref.near_E(ref.P)}")
    st = report("S-near", mis_ref.estimate(mis_ref.near_scene(), 16), E)
    for k, (m, se) in st.items():
        assert (np.abs(m - E) <= 5 * se).all(), k
    ratio = st["mis"][1] / st["nee"][1]
    print(f"SE_mis / SE_nee = {ratio}")
    assert (ratio <= 0.35).all()


def test_s_sun_the_bounce_is_poor_and_mis_wins():
    st = report("S-sun", mis_ref.estimate(mis_ref.sun_scene(), 16), mis_ref.sun_E())
    ratio = st["mis"][1] / st["plain"][1]
    print(f"SE_mis / SE_bounce = {ratio}")
    assert (ratio <= 0.35).all()


def test_s_sky_all_three_agree_with_the_closed_form():
    """a sun in a sky of 0.5: the figures are printed (profiles/r17_mis.txt), only the means are asserted"""
    E = mis_ref.sun_E(sky=True)
    st = report("S-sky", mis_ref.estimate(mis_ref.sun_scene(sky=True), 16), E)
    for k, (m, se) in st.items():
        assert (np.abs(m - E) <= 5 * se).all(), k


def test_the_case_list():
    names = [c.name for c in mis_ref.cases()]
    assert names == ["A-mis2", "A2-mis2", "B-mis2", "BA-mis2", "G-mis2", "H-mis2", "I-given-cull1-mis2", "I-flipped-cull0-mis2",
                     "I-flipped-cull1-mis2", "J-below-mis2", "J-above-mis2", "J2-between-mis2", "J2-behind-mis2"]
    by = {c.name: c for c in ref.cases()}
    for c in mis_ref.cases():
        assert c.flags == ref.NEE | g.FLAG_MIS and c.depth == 2 and c.nee
    got = {c.name: c.E for c in mis_ref.cases()}
    assert np.array_equal(got["H-mis2"], by["H-nee2"].E) and np.array_equal(got["G-mis2"], by["G-nee2"].E)
    assert np.array_equal(got["BA-mis2"], by["BA-nee1"].E)
