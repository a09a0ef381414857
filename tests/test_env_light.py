"""The environment map as a light (PT_OPT_ENV_LIGHT) without a GPU: the declarations, the bindings, the
NULL-context errors, pt_app --env-light's refusal, and the properties of the numpy reference (tests/env_light_ref.py) that the GPU
tests (tests/test_gpu_env_light.py) lean on."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_light_ref as ref
import env_ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")


# ---------------------------------------------------------------------------------------------------- header, ABI, errors
def test_header_declares_the_option_and_the_calls():
    src = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"PT_OPT_ENV_LIGHT\s*=\s*35\b", src)
    assert re.search(r"int\s+pt_environment_is_light\s*\(\s*pt_ctx\s*\*\s*ctx,\s*int\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"int\s+pt_sample_environment\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+float\s*\*\s*u_dev,\s*size_t\s+n,\s*float\s*\*\s*dir_pdf_dev,"
                     r"\s*float\s*\*\s*radiance_dev\s*\)\s*;", src)
    assert re.search(r"int\s+pt_environment_pdf\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+float\s*\*\s*rays_dev,\s*size_t\s+n,\s*float\s*\*\s*pdf_dev\s*\)\s*;", src)
    assert "sampling the map as a light under PT_FLAG_NEE" not in src   # no longer left out
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src)


def test_abi_binds_the_calls():
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_environment_is_light"][2]) == 2 and len(rows["pt_sample_environment"][2]) == 5 and len(rows["pt_environment_pdf"][2]) == 4
    lib = g._abi.ptmi()
    assert lib.pt_sample_environment.argtypes[2] is C.c_size_t and lib.pt_environment_pdf.argtypes[2] is C.c_size_t
    assert g._abi.OPT_ENV_LIGHT == 35
    for name in ("environment_is_light", "sample_environment", "environment_pdf"):
        assert callable(getattr(g.PathTracer, name))
    assert inspect.signature(g.PathTracer.upload_environment).parameters["light"].default is False


def test_null_context_is_refused():
    lib = g._abi.ptmi()
    out = C.c_int(7)
    assert lib.pt_environment_is_light(None, C.byref(out)) == -1 and out.value == 7
    assert "null ctx" in lib.pt_last_error(None).decode()
    assert lib.pt_sample_environment(None, None, 4, None, None) == -1
    assert lib.pt_environment_pdf(None, None, 4, None) == -1
    assert lib.pt_set_option(None, g._abi.OPT_ENV_LIGHT, 1) == -1


def test_pt_app_env_light_goes_with_env(tmp_path):
    out = tmp_path / "x.png"
    r = subprocess.run([APP, "--mesh", os.path.join(ROOT, "assets", "cube.ptmesh"), "--width", "32", "--height", "16", "--frames", "1", "--out", str(out),
                        "--env-light"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--env-light" in r.stderr, r.stderr[-300:]
    assert "mesh" not in r.stdout and not out.exists()   # refused before the scene was built
    assert "--env-light" in open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read().split("#include")[0]   # the usage text


# ---------------------------------------------------------------------------------------------------- the reference's properties
CASES = ref.draw_cases()   # the maps of the GPU draw test


@pytest.mark.parametrize("tex,bil", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_reference_tables_and_draws(tex, bil):
    H, W = tex.shape[:2]
    tab = ref.Tables(tex, bil)
    # the CDFs: non-decreasing, exact ends
    assert tab.cx.shape == (H, W + 1) and tab.cy.shape == (H + 1,) and tab.zs.shape == (H + 1,)
    assert (np.diff(tab.cx, axis=1) >= 0).all() and (np.diff(tab.cy) >= 0).all() and (np.diff(tab.zs) > 0).all()   # (no row of these maps is so near a pole that its edges round together)
    assert (tab.cx[:, 0] == 0).all() and (tab.cx[:, W] == 1).all() and tab.cy[0] == 0 and tab.cy[H] == 1 and tab.zs[0] == -1 and tab.zs[H] == 1
    # the density integrates to one over the sphere
    total = (tab.texel_pdf().astype(np.float64) * tab.omega()[:, None]).sum()
    assert abs(total - 1.0) <= 1e-6, total
    assert abs(tab.omega().sum() * W - 4.0 * np.pi) <= 1e-6
    # draws: the direction looks up the texel that was drawn, its density is the drawn one, no texel of weight 0 is ever drawn
    u = ref.stratified(64)
    s = ref.draw(tab, u)
    assert (tab.m[s["y"], s["x"]] > 0).all()
    assert (s["pdf"] > 0).all() and (s["v1"] >= 0).all() and (s["v1"] < 1).all() and (s["v2"] >= 0).all() and (s["v2"] < 1).all()
    assert np.abs(np.linalg.norm(s["d"], axis=1) - 1.0).max() <= 1e-6
    inner = ref.interior(s)
    y, x, valid = ref.texel_of(s["d"][inner], W, H)
    assert valid.all() and np.array_equal(y, s["y"][inner]) and np.array_equal(x, s["x"][inner])
    assert np.array_equal(ref.pdf_of(tab, s["d"][inner]), s["pdf"][inner])
    idx = np.arange(W * H, dtype=np.float32).reshape(H, W, 1) * np.ones(3, np.float32)
    assert np.array_equal(env_ref.nearest(idx, *env_ref.positions(s["d"][inner], W, H)[:2])[:, 0], (s["y"][inner] * W + s["x"][inner]).astype(np.float32))


def test_bilinear_weights_cover_the_neighbours():
    """One hot texel: nearest gives weight to that texel alone, bilinear to its 3 x 3 neighbourhood, columns wrapped."""
    tex = ref.hot_map(5, 3, 1, 0)
    near, wide = ref.Tables(tex, False).m, ref.Tables(tex, True).m
    assert (near > 0).sum() == 1 and near[1, 0] == 1000
    assert (wide > 0).sum() == 9 and (wide[:, [4, 0, 1]] == 1000).all() and not wide[:, 2:4].any()


def test_share_of_interior_draws():
    """The GPU test compares pt_environment_pdf bit for bit on the draws with v1, v2 in [0.01, 0.99] and asserts that they are at
    least 95 % of all: with a uniform residual the expected share is 0.98^2 = 96 %.  The reference alone, on that test's maps."""
    for name, tex, bil in CASES:
        s = ref.draw(ref.Tables(tex, bil), ref.stratified(64))
        share = ref.interior(s).mean()
        print(f"{name}: {100 * share:.2f} % interior")
        assert share >= 0.95, name


def test_zero_rows_are_never_drawn_and_the_integral_is_the_estimate():
    tex = ref.black_rows_map()
    tab = ref.Tables(tex, False)
    s = ref.draw(tab, ref.stratified(64))
    assert not np.isin(s["y"], [0, 1, 2, 3, 10, 11, 31]).any()
    # L / pdf is the map's integral for a grey nearest map (GPU test 2's identity), here in the reference's own arithmetic
    grey = np.repeat(env_ref.gradient_map(8, 4)[:, :, :1], 3, axis=2)
    tab = ref.Tables(grey, False)
    s = ref.draw(tab, ref.stratified(64))
    I = ref.integral(tab, grey)[0]
    L = grey[s["y"], s["x"], 0].astype(np.float64)
    bound = I * 4 * 2.0 ** -24 / np.minimum(s["px"], s["py"]).astype(np.float64)
    assert (np.abs(L / s["pdf"].astype(np.float64) - I) <= bound).all()


def test_plane_radiance_of_a_constant_map():
    """A constant map of radiance L over a diffuse plane: the upper hemisphere's cosine integral is pi, so E = rho * L."""
    tex = np.full((8, 16, 3), 0.75, np.float32)
    E = ref.plane_radiance(ref.Tables(tex, False), tex, (0.5, 0.6, 0.7))
    assert np.allclose(E, np.array([0.5, 0.6, 0.7]) * 0.75, rtol=1e-6)


def test_clamp_of_u():
    u = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert np.array_equal(ref.clamp_u(u), np.array([0, 0, 0.5, ref.ONE_BELOW, ref.ONE_BELOW, 0, ref.ONE_BELOW, 0], np.float32))


def test_tile_split_passes_light_through():
    """tile_split.upload_environment hands its keywords to every context's upload_environment: light=True reaches each rank."""
    from gpu_pathtracer_amd import tile_split

    class Rank:
        def __init__(self):
            self.calls = []

        def upload_environment(self, texels, **kw):
            self.calls.append(("upload", kw))

        def clear_environment(self):
            self.calls.append(("clear", {}))

    ranks = [Rank(), Rank()]
    tile_split.upload_environment(ranks, np.ones((2, 4, 3), np.float32), light=True, filter=g.ENV_NEAREST)
    tile_split.upload_environment(ranks, None)
    for r in ranks:
        assert r.calls == [("upload", {"light": True, "filter": g.ENV_NEAREST}), ("clear", {})]
