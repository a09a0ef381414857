"""CPU tests (no GPU) of the variance-guided denoiser: pt_denoise_variance / pt_temporal_moments are declared, bound and exported
with the header's struct layout, argument checks come before any device call, and the CPU reference (tests/denoise_var_ref.py) has
the properties its contract promises — including the gain of the defaults on oracle renders at every sample count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import denoise_var_ref as V
import moments_ref
from denoise_var_ref import VAR_QUALITY_K

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_denoise_variance\(pt_ctx\* ctx, const pt_denoise_variance_params\* dp, const float\* color_dev,\s+"
                     r"const float\* moments_dev, const float\* length_dev /\* may be NULL \*/,\s+"
                     r"const float\* albedo_dev, const float\* normal_dev, const float\* position_dev,\s+"
                     r"float\* out_dev, float\* out_variance_dev /\* may be NULL \*/, uint32_t\* rgba_dev\);", hdr)
    assert re.search(r"int pt_temporal_moments\(pt_ctx\* ctx, const pt_temporal_params\* tp, const pt_camera\* prev_cam,\s+"
                     r"const float\* prev_verts_dev, const float\* cur_verts_dev, size_t n_tris,\s+"
                     r"const float\* prev_moments_dev, const float\* prev_length_dev,\s+"
                     r"const float\* prev_normal_dev, const float\* prev_position_dev, const int32_t\* prev_id_dev,\s+"
                     r"const float\* cur_moments_dev,\s+"
                     r"const float\* cur_normal_dev, const float\* cur_position_dev, const int32_t\* cur_id_dev,\s+"
                     r"float\* out_moments_dev\);", hdr)
    assert "reprojecting pt_render_moments' moments" not in hdr     # no longer out of scope
    names = {n: a for n, _, a in g._abi.PTMI_SYMBOLS}
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    for fn, n_args in (("pt_denoise_variance", 11), ("pt_temporal_moments", 16)):
        assert fn in names and len(names[fn]) == n_args and hasattr(g._abi.ptmi(), fn)
        assert re.search(rf" T {fn}$", out, re.M)
    assert g._abi.ptmi().pt_abi_version() == 3     # functions are only added
    assert re.search(r"#define PTMI_ABI_VERSION 3\b", hdr)


def test_params_layout_matches_the_header():
    D = g.DenoiseVarianceParams
    assert C.sizeof(D) == 32
    assert [(f, getattr(D, f).offset) for f, _ in D._fields_] == [
        ("width", 0), ("height", 4), ("iterations", 8), ("sigma_luminance", 12), ("sigma_normal", 16), ("sigma_position", 20),
        ("samples_per_frame", 24), ("_pad", 28)]
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    body = re.search(r"typedef struct pt_denoise_variance_params \{(.*?)\} pt_denoise_variance_params;", hdr, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in D._fields_]


def test_null_context_is_invalid():
    lib = g._abi.ptmi()
    dp = g.DenoiseVarianceParams(8, 8, 2, 4.0, 0.5, 0.1, 1.0, 0)
    assert lib.pt_denoise_variance(None, C.byref(dp), *([None] * 9)) == -1   # PT_ERR_INVALID, no crash
    assert b"null ctx" in lib.pt_last_error(None)
    tp = g.TemporalParams(8, 8, 32.0, 0.02, 0.9, 0)
    assert lib.pt_temporal_moments(None, C.byref(tp), None, None, None, 0, *([None] * 10)) == -1
    assert b"null ctx" in lib.pt_last_error(None)


def test_defaults_equal_the_apps():
    d = g.DENOISE_VARIANCE_DEFAULTS
    assert d == dict(iterations=4, sigma_luminance=4.0, sigma_normal=1.0, sigma_position=0.03)
    assert {k: d[k] for k in ("iterations", "sigma_normal", "sigma_position")} == {
        k: g.DENOISE_DEFAULTS[k] for k in ("iterations", "sigma_normal", "sigma_position")}   # the geometry stops are pt_denoise's
    src = open(os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app.cpp")).read()
    m = re.search(r"pt_denoise_variance_params dv = \{W, H, (\d+), ([\d.e+-]+)f, ([\d.e+-]+)f, ([\d.e+-]+)f, ", src)
    assert m and (int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))) == (
        d["iterations"], d["sigma_luminance"], d["sigma_normal"], d["sigma_position"])
    for refused in ("--denoise-variance goes with --denoise-out", "--denoise-variance does not combine with --temporal-out or --resume"):
        assert refused in src


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


def random_moments(H, W, seed, n):
    """Moments whose seed variance (n samples) is uniform in [1e-3, 1e-1]."""
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.1, 1.0, (H, W)).astype(np.float32)
    var = rng.uniform(1e-3, 1e-1, (H, W))
    return np.stack([m1, (m1.astype(np.float64) ** 2 + var * (n - 1)).astype(np.float32)], -1)


def test_zero_iterations_is_the_identity_and_returns_the_seed():
    rng = np.random.default_rng(1)
    c = rng.uniform(0, 2, (9, 13, 3)).astype(np.float32)
    mom = random_moments(9, 13, 2, 8)
    ln = rng.integers(1, 5, (9, 13)).astype(np.float32)
    alb, nrm, pos = random_guides(9, 13, 2, 0.3)
    out, var = V.atrous_variance(c, mom, ln, alb, nrm, pos, 0, 4.0, 0.5, 0.1, samples_per_frame=2.0)
    assert np.array_equal(out.view(np.int32), c.view(np.int32))
    n = 2.0 * ln.astype(np.float64)
    want = np.maximum(0.0, mom[..., 1].astype(np.float64) - mom[..., 0].astype(np.float64) ** 2) / (n - 1)
    assert np.allclose(var, want, rtol=1e-4, atol=0)
    assert np.array_equal(var, V.seed(c, mom, ln, alb, 2.0)[0])
    # fewer than two samples: as uncertain as it is bright; a NaN counts as 0; the result is finite
    mom[0, 0], mom[0, 1], mom[0, 2] = (0.5, 0.7), (np.nan, np.nan), (1.0, np.inf)
    var1 = V.seed(c, mom, None, alb, 1.0)[0]
    assert var1[0, 0] == np.float32(0.7) and var1[0, 1] == 0 and var1[0, 2] == np.float32(1e30)
    assert np.array_equal(var1[1:], mom[1:, :, 1])


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_constant_image_stays_constant(iterations):
    albedo, normal, position = random_guides(23, 17, 3)
    albedo[..., :3] = 0.5
    c = np.full((23, 17, 3), 0.3, np.float32)
    out, var = V.atrous_variance(c, random_moments(23, 17, 4, 16), None, albedo, normal, position, iterations, 4.0, 0.3, 0.05, samples_per_frame=16)
    assert np.allclose(out, 0.3, rtol=0, atol=1e-6)
    assert np.all(var >= 0) and np.all(np.isfinite(var))


def test_no_weight_and_no_prefilter_tap_crosses_a_hit_miss_border():
    H, W = 20, 24
    albedo, normal, position = random_guides(H, W, 4)
    albedo[..., :3] = 1.0
    miss = np.zeros((H, W), bool)
    miss[:, : W // 2] = True
    miss[3:7, 15:18] = True                         # an island of misses among hits ...
    for a in (albedo, normal, position):
        a[miss] = 0
    c = np.where(miss[..., None], 0.0, 1.0).astype(np.float32)
    mom = random_moments(H, W, 5, 8)
    mom[3:7, 15:18] = (0.25, 0.0625)                # ... whose variance is exactly 0 (in the packed buffer: -0.0f)
    assert not V.seed(c, mom, None, albedo, 8.0)[0][3:7, 15:18].any()
    for it in (1, 4):
        for sig in ((4.0, 0.5, 0.1), (0.0, 0.0, 0.0)):
            taps = []
            out, var = V.atrous_variance(c, mom, None, albedo, normal, position, it, *sig, samples_per_frame=8.0, weights_out=taps)
            assert np.array_equal(out[miss], np.zeros_like(out[miss])) and np.array_equal(out[~miss], np.ones_like(out[~miss]))
            if it == 1:                             # (from step 4 on the island's taps reach the misses of the left half)
                assert not var[3:7, 15:18].any()    # nothing of the hits' variance leaks into the island
            assert np.all(var[~miss] > 0)
            ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            for l, level in enumerate(taps):
                for (dy, dx), w in level.items():
                    yq, xq = ys + (dy << l), xs + (dx << l)
                    inside = (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
                    crosses = inside & (miss[np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)] != miss)
                    assert not w[crosses].any() and not w[~inside].any()
    # the pre-filter: a field that is 1 on the hits and 0 on the misses comes back unchanged — no tap crossed
    v = np.where(miss, 0.0, 1.0)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    assert np.array_equal(V.prefilter(v, ~miss, ys, xs), v)


@pytest.mark.parametrize("shape,iterations", [((7, 5), 2), ((37, 23), 4)])
def test_sigma_luminance_zero_is_pt_denoise_without_its_colour_term(shape, iterations):
    H, W = shape
    rng = np.random.default_rng(5)
    albedo, normal, position = random_guides(H, W, 6, 0.1)
    c = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    out, _ = V.atrous_variance(c, random_moments(H, W, 7, 4), None, albedo, normal, position, iterations, 0.0, 0.5, 0.05, samples_per_frame=4)
    ref = R.atrous(c, albedo, normal, position, iterations, 0.0, 0.5, 0.05)
    assert np.abs(out - ref).max() <= 1e-6


def test_variance_after_one_iteration_with_all_terms_off():
    """v(1) = sum h^2 v / (sum h)^2 over the taps inside the image, restated with separable passes."""
    H, W = 11, 9
    rng = np.random.default_rng(8)
    albedo, normal, position = random_guides(H, W, 9)
    c = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    mom = random_moments(H, W, 10, 4)
    _, var = V.atrous_variance(c, mom, None, albedo, normal, position, 1, 0.0, 0.0, 0.0, samples_per_frame=4)
    _, _, v0 = V.seed(c, mom, None, albedo, 4.0)
    h = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0

    def conv(a, k, axis):
        pad = [(0, 0)] * 2
        pad[axis] = (2, 2)
        p = np.pad(a, pad)
        return sum(k[i] * np.take(p, np.arange(i, i + a.shape[axis]), axis=axis) for i in range(5))

    num = conv(conv(v0.astype(np.float64), h ** 2, 1), h ** 2, 0)
    den = conv(conv(np.ones((H, W)), h, 1), h, 0)
    la = V.luminance64(R.demod_albedo(albedo))
    assert np.allclose(var, num / den ** 2 * la ** 2, rtol=1e-6, atol=0)


def test_moments_blend_reference_equals_the_colour_reference():
    """denoise_var_ref.temporal_moments against temporal_ref.temporal run on the colour (m1, m2, 0): the same taps, the blend in
    binary32 instead of binary64."""
    import temporal_ref as T
    W, H = 16, 12
    rng = np.random.default_rng(12)
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., 2] = -1.0
    pos = np.zeros((H, W, 4), np.float32)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cam = g.default_camera(W, H)
    # a wall at distance 10 in front of the camera, seen again from 0.3 to the side
    f, r, u, o = (np.array(list(v), np.float64) for v in (cam.front, cam.right, cam.up, cam.pos))
    sx, sy = (xs - W / 2.0 + 0.5) * cam.aspect * cam.fov / (W - 1), (ys - H / 2.0 + 0.5) * cam.fov / (H - 1)
    d = f + sx[..., None] * r + sy[..., None] * u
    pos[..., :3] = o + 10.0 * d
    pos[..., 3] = 10.0 * np.linalg.norm(d, axis=-1)
    nrm[..., :3] = -f
    prev_cam = T.moved(cam, side=0.3)
    prev_pos = pos.copy()
    dp = np.array(list(prev_cam.front), np.float64) + sx[..., None] * np.array(list(prev_cam.right), np.float64) + sy[..., None] * u
    op = np.array(list(prev_cam.pos), np.float64)
    tt = (10.0 - (op - o) @ f) / (dp @ f)
    prev_pos[..., :3] = op + tt[..., None] * dp
    prev_pos[..., 3] = tt * np.linalg.norm(dp, axis=-1)
    pm, cm = (rng.uniform(0, 1, (H, W, 2)).astype(np.float32) for _ in range(2))
    ln = rng.integers(1, 20, (H, W)).astype(np.float32)
    kw = dict(max_history=8.0, plane_tolerance=0.02, normal_threshold=0.9)
    pn = nrm.copy()
    pn[2:7, 3:10] = 0                               # a block of history misses: the pixels that land there are rejected
    out, fragile, acc = V.temporal_moments(W, H, prev_cam, None, None, 0, pm, ln, pn, prev_pos, None, cm, nrm, pos, None, **kw)
    pad = lambda m: np.concatenate([m, np.zeros((H, W, 1), np.float32)], -1)
    ref, _, _, acc2 = T.temporal(W, H, prev_cam, pad(pm), ln, pn, prev_pos, None, pad(cm), nrm, pos, None, **kw)
    assert np.array_equal(acc, acc2) and 0.5 < acc.mean() < 1.0
    assert np.abs(out - ref[..., :2]).max() <= 2e-7 and not np.array_equal(out, cm)
    assert np.array_equal(out[~acc], cm[~acc])
    none, _, acc0 = V.temporal_moments(W, H, None, None, None, 0, None, None, None, None, None, cm, nrm, pos, None, **kw)
    assert np.array_equal(none, cm) and not acc0.any()


# ---------------------------------------------------------------------------------------------------- quality
def test_quality_on_oracle_renders():
    """cornell_box at 80x60 against 8192 spp: DENOISE_VARIANCE_DEFAULTS gain at least VAR_QUALITY_K at 4, 64 and 1024 spp, and at
    1024 spp more than pt_denoise's defaults (which lose there).  Measured: 2.68 / 3.82 / 2.05, the defaults 0.96 at 1024."""
    W, H = 80, 60
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    mk = dict(materials=mesh.materials, tri_material=mesh.tri_material)
    ref, _, _ = orc.render(bvh, None, cam, p, V.QUALITY_REF_SPP, want_rgba=False, **mk)
    alb, nrm, pos, ids, _, _ = R.guides(bvh, None, cam, p, mesh.materials, mesh.tri_material)
    assert 0.5 < (ids >= 0).mean() < 1.0                  # both hits and misses in the frame
    p.frame = V.QUALITY_NOISY_FRAME
    for spp in V.QUALITY_SPP:
        mom, col = moments_ref.oracle_moments(bvh, None, cam, p, spp, **mk)
        noisy = orc.fold_samples(col.reshape(-1, spp, 3), 1).reshape(H, W, 3)     # = orc.render of the same call, bit for bit
        out, _ = V.atrous_variance(noisy, mom, None, alb, nrm, pos, samples_per_frame=spp, **g.DENOISE_VARIANCE_DEFAULTS)
        gain = R.mse(noisy, ref) / R.mse(out, ref)
        plain = R.mse(noisy, ref) / R.mse(R.atrous(noisy, alb, nrm, pos, **g.DENOISE_DEFAULTS), ref)
        print(f"80x60 {spp} spp: variance-guided gain {gain:.2f}, pt_denoise defaults {plain:.2f}")
        assert gain >= VAR_QUALITY_K, (spp, gain)
        if spp == 1024:
            assert gain > plain, (gain, plain)
