"""CPU tests of the luminance-moment interface (pt_render_moments, pt_frame_error): the C ABI surface without a device, and
the properties of the numpy reference (tests/moments_ref.py) the GPU tests compare against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import gpu_pathtracer_amd as g
import orc
import denoise_ref as R
import moments_ref as M

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1

DECL_RENDER = ("int pt_render_moments(pt_ctx* ctx, float* accum_dev, uint32_t* rgba_dev, float* moments_dev, "
               "const pt_camera* cam, const pt_params* params, uint32_t spp);")
DECL_ERROR = ("int pt_frame_error(pt_ctx* ctx, const float* moments_dev, int32_t width, int32_t height, "
              "uint64_t n_samples, float threshold, double* mean_rse, uint64_t* n_above);")


def test_header_declares_both_functions_and_abi_stays_3():
    hdr = " ".join(open(os.path.join(ROOT, "include", "ptmi.h")).read().split())
    assert DECL_RENDER in hdr
    assert DECL_ERROR in hdr
    assert re.search(r"#define PTMI_ABI_VERSION 3\b", hdr)
    assert g._abi.ptmi().pt_abi_version() == 3


def test_symbols_are_bound_and_exported():
    _vp = C.c_void_p
    bound = {n: (res, args) for n, res, args in g._abi.PTMI_SYMBOLS}
    assert bound["pt_render_moments"] == (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(g.Camera), C.POINTER(g.Params), C.c_uint32])
    assert bound["pt_frame_error"] == (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_uint64, C.c_float, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_uint64)])
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    exported = set(re.findall(r" T (pt_[a-z_0-9]+)", out))
    assert {"pt_render_moments", "pt_frame_error", "pt_render"} <= exported
    assert hasattr(g.PathTracer, "frame_error")


def test_null_context_is_an_error_code_not_a_crash():
    lib = g._abi.ptmi()
    assert lib.pt_render_moments(None, None, None, None, None, None, 1) == PT_ERR_INVALID
    assert lib.pt_last_error(None) == b"null ctx"
    mean = C.c_double()
    assert lib.pt_frame_error(None, None, 4, 4, 2, 0.0, C.byref(mean), None) == PT_ERR_INVALID
    assert lib.pt_last_error(None) == b"null ctx"


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_constant_stream_has_no_variance():
    """One or two equal samples: m1 = L and m2 = L * L exactly ((L + L) * 0.5 has no rounding), so m2 == m1 * m1 to the one
    rounding of the product and rse is 0.  From N = 3 on a step rounds (3 L, and 1 / 3 is not a binary32 number): each of the N
    steps adds at most four roundings of 2^-24 relative (the product with N - 1, the sum, the rounded 1 / N, the product with
    it) and earlier errors only shrink by (N - 1) / N, so |m1 - L| <= 4 N 2^-24 L, the same for m2 against L * L, and m2
    against m1 * m1 three times that plus the product's rounding."""
    rng = np.random.default_rng(5)
    c = rng.uniform(0, 30, (200, 1, 3)).astype(np.float32)
    L = M.luminance(c[:, 0])
    for n in (1, 2):
        m = M.update(np.repeat(c, n, axis=1), 1)
        assert np.array_equal(m[:, 0], L) and np.array_equal(m[:, 1], L * L)
        assert np.array_equal(m[:, 1], m[:, 0] * m[:, 0])
        assert not M.rse(m, 2).any()
    N, u = 12, 2.0 ** -24
    m = M.update(np.repeat(c, N, axis=1), 1)
    L64 = L.astype(np.float64)
    assert np.all(np.abs(m[:, 0] - L64) <= 4 * N * u * L64)
    assert np.all(np.abs(m[:, 1] - m[:, 0].astype(np.float64) ** 2) <= (12 * N + 1) * u * L64 ** 2)
    black = np.zeros((4, 2), np.float32)
    assert not M.rse(black, 2).any()                                  # the floor keeps a black pixel at 0, not 0 / 0
    exact = np.stack([L, L * L], -1)
    mean, above = M.frame_error(exact, N, 0.0)
    assert mean == 0.0 and above == 0


def test_split_equals_at_once_bit_for_bit():
    rng = np.random.default_rng(6)
    col = rng.uniform(0, 4, (37, 23, 12, 3)).astype(np.float32)
    col[3, 4, 7] = (26.0, 19.0, 31.0)   # a firefly: no clamp anywhere
    whole = M.update(col, 1)
    first = M.update(col[..., :5, :], 1, moments=np.full((37, 23, 2), np.nan, np.float32))   # N == 1 overwrites
    both = M.update(col[..., 5:, :], 6, moments=first)
    assert np.array_equal(whole.view(np.int32), both.view(np.int32))
    assert whole[3, 4, 1] > 30.0                                      # the firefly shows in m2
    later = M.update(col[..., 5:, :], 18, moments=M.update(col[..., :5, :], 13, moments=whole))
    assert np.array_equal(later.view(np.int32), M.update(col, 13, moments=whole).view(np.int32))


def test_oracle_samples_fold_to_the_render_and_m1_is_their_mean():
    """The colours the reference is computed from are the ones before the fold: folding them gives orc.render bit for bit, some
    exceed 1, and the float32 running m1 of their luminance equals the float64 mean within 1e-6 relative (four samples: at
    most four roundings of 6e-8 per step, each diluted by the later steps — below 6e-7 in the worst case)."""
    W, H, spp = 80, 60, 4
    mesh, bvh, cam, p = R.cornell_box_scene(W, H)
    p.frame, p.sample_index = 3, 1
    m, col = M.oracle_moments(bvh, None, cam, p, spp, mesh.materials, mesh.tri_material)
    acc, _, _ = orc.render(bvh, None, cam, p, spp=spp, materials=mesh.materials, tri_material=mesh.tri_material)
    assert np.array_equal(orc.fold_samples(col, 1).view(np.int32), acc.view(np.int32))
    assert col.max() > 1.0
    L = M.luminance(col).astype(np.float64)
    mean = L.mean(axis=-1)
    lit = mean > 0
    assert lit.mean() > 0.01   # a small ceiling light and no next-event estimation: most four-sample pixels are black
    assert np.all(np.abs(m[..., 0][lit] - mean[lit]) <= 1e-6 * mean[lit])
    assert not m[..., 0][~lit].any()
    mean_rse, above = M.frame_error(m, spp, 0.0)
    assert 0.0 < mean_rse < 10.0 and 0 < above <= W * H
