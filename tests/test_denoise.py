"""CPU tests (no GPU) of the guide buffers + denoiser extension: pt_render_aux / pt_denoise are declared, bound and exported with
the header's struct layout, argument checks come before any device call, and the CPU reference filter (tests/denoise_ref.py)
has the properties its contract promises — including the gain of pt_denoise's defaults on oracle renders."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
from denoise_ref import QUALITY_K

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_aux_and_denoise_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_render_aux\(pt_ctx\* ctx, const pt_camera\* cam, const pt_params\* params,\s+float\* albedo_dev, "
                     r"float\* normal_dev, float\* position_dev, int32_t\* id_dev\);", hdr)
    assert re.search(r"int pt_denoise\(pt_ctx\* ctx, const pt_denoise_params\* dp, const float\* color_dev,\s+const float\* albedo_dev, "
                     r"const float\* normal_dev, const float\* position_dev,\s+float\* out_dev, uint32_t\* rgba_dev\);", hdr)
    names = {n for n, _, _ in g._abi.PTMI_SYMBOLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    for fn in ("pt_render_aux", "pt_denoise"):
        assert fn in names and hasattr(g._abi.ptmi(), fn)
        assert re.search(rf" T {fn}$", out, re.M)
    assert g._abi.ptmi().pt_abi_version() == 3     # functions are only added


def test_denoise_params_layout_matches_the_header():
    D = g.DenoiseParams
    assert C.sizeof(D) == 24
    assert [(f, getattr(D, f).offset) for f, _ in D._fields_] == [
        ("width", 0), ("height", 4), ("iterations", 8), ("sigma_color", 12), ("sigma_normal", 16), ("sigma_position", 20)]
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct pt_denoise_params \{(.*?)\} pt_denoise_params;", hdr, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["width", "height", "iterations", "sigma_color", "sigma_normal", "sigma_position"]


def test_null_context_is_invalid():
    lib = g._abi.ptmi()
    dp = g.DenoiseParams(8, 8, 2, 1.0, 0.5, 0.1)
    assert lib.pt_render_aux(None, None, None, None, None, None, None) == -1   # PT_ERR_INVALID, no crash
    assert b"null ctx" in lib.pt_last_error(None)
    assert lib.pt_denoise(None, C.byref(dp), None, None, None, None, None, None) == -1
    assert b"null ctx" in lib.pt_last_error(None)


def test_defaults_are_in_range():
    d = g.DENOISE_DEFAULTS
    assert set(d) == {"iterations", "sigma_color", "sigma_normal", "sigma_position"}
    assert 0 <= d["iterations"] <= 10 and all(np.isfinite(d[k]) for k in d)
    src = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read()   # the app uses the same values
    m = re.search(r"pt_denoise_params dn = \{[^,]+, [^,]+, (\d+), ([\d.e+-]+)f, ([\d.e+-]+)f, ([\d.e+-]+)f\}", src)
    assert m and (int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))) == (
        d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_position"])


# ---------------------------------------------------------------------------------------------------- the reference filter
def random_guides(H, W, seed, miss_frac=0.0):
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normal = np.zeros((H, W, 4), np.float32)
    normal[..., :3] = n
    position = np.zeros((H, W, 4), np.float32)
    position[..., :3] = rng.uniform(-5, 5, (H, W, 3))
    position[..., 3] = rng.uniform(1, 20, (H, W))
    albedo = np.zeros((H, W, 4), np.float32)
    albedo[..., :3] = rng.uniform(0.05, 1.0, (H, W, 3))
    miss = rng.uniform(size=(H, W)) < miss_frac
    for a in (normal, position, albedo):
        a[miss] = 0
    return albedo, normal, position


def test_zero_iterations_is_the_identity():
    rng = np.random.default_rng(1)
    c = rng.uniform(0, 2, (9, 13, 3)).astype(np.float32)
    out = R.atrous(c, *random_guides(9, 13, 2, 0.3), 0, 1.0, 0.5, 0.1)
    assert np.array_equal(out.view(np.int32), c.view(np.int32))


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_constant_image_stays_constant(iterations):
    albedo, normal, position = random_guides(23, 17, 3)
    albedo[..., :3] = 0.5
    c = np.full((23, 17, 3), 0.3, np.float32)
    out = R.atrous(c, albedo, normal, position, iterations, 0.5, 0.3, 0.05)
    assert np.allclose(out, 0.3, rtol=0, atol=1e-6)


def test_no_weight_crosses_a_hit_miss_border():
    H, W = 20, 24
    albedo, normal, position = random_guides(H, W, 4)
    albedo[..., :3] = 1.0
    miss = np.zeros((H, W), bool)
    miss[:, : W // 2] = True
    miss[3:7, 15:18] = True                         # an island of misses among hits
    for a in (albedo, normal, position):
        a[miss] = 0
    c = np.where(miss[..., None], 0.0, 1.0).astype(np.float32)
    for it in (1, 4):
        for sig in ((1.0, 0.5, 0.1), (0.0, 0.0, 0.0)):
            out = R.atrous(c, albedo, normal, position, it, *sig)
            assert np.array_equal(out[miss], np.zeros_like(out[miss])) and np.array_equal(out[~miss], np.ones_like(out[~miss]))


def b3_atrous(img, iterations):
    """Separable B3-spline a-trous blur, taps outside the image dropped and the weights renormalised (an independent
    restatement: 1-D passes over zero-padded arrays, divided by the same passes over an image of ones)."""
    h = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    x = np.asarray(img, np.float64)
    H, W = x.shape[:2]

    def conv(a, s, axis):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (2 * s, 2 * s)
        p = np.pad(a, pad)
        n = a.shape[axis]
        return sum(h[k] * np.take(p, np.arange(k * s, k * s + n), axis=axis) for k in range(5))

    for lvl in range(iterations):
        s = 1 << lvl
        num = conv(conv(x, s, 1), s, 0)
        den = conv(conv(np.ones((H, W, 1)), s, 1), s, 0)
        x = num / den
    return x


@pytest.mark.parametrize("shape,iterations", [((7, 5), 2), ((37, 23), 4), ((16, 64), 6)])
def test_all_terms_off_is_the_b3_spline_blur(shape, iterations):
    H, W = shape
    rng = np.random.default_rng(5)
    albedo, normal, position = random_guides(H, W, 6)
    c = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    out = R.atrous(c, albedo, normal, position, iterations, 0.0, -1.0, 0.0)
    a = R.demod_albedo(albedo).astype(np.float64)
    ref = np.clip(b3_atrous((c / R.demod_albedo(albedo)).astype(np.float32), iterations) * a, 0, 1)
    assert np.allclose(out, ref, rtol=0, atol=1e-6)


def test_defaults_gain_on_oracle_renders():
    """4 spp of cornell_box at 80x60, filtered with the defaults, is at least QUALITY_K times closer (MSE) to 512 spp."""
    W, H = 80, 60                                         # (the default camera's dist is H / 60, integer divide: H >= 60)
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    ref, _, _ = orc.render(bvh, None, cam, p, 512, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)
    p.frame = 1 << 20
    noisy, _, _ = orc.render(bvh, None, cam, p, 4, materials=mesh.materials, tri_material=mesh.tri_material, want_rgba=False)
    alb, nrm, pos, ids, _, _ = R.guides(bvh, None, cam, p, mesh.materials, mesh.tri_material)
    assert 0.5 < (ids >= 0).mean() < 1.0                  # both hits and misses in the frame
    out = R.atrous(noisy, alb, nrm, pos, **g.DENOISE_DEFAULTS)
    gain = R.mse(noisy, ref) / R.mse(out, ref)
    assert gain >= QUALITY_K, gain
