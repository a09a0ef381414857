"""numpy restatement of pt_render_moments' per-pixel update and of pt_frame_error (include/ptmi.h), for the tests.

The device code uses plain binary32 * and + (the library is built with -ffp-contract=off and writes no fmaf there), so every
step is one rounding and numpy's float32 arithmetic gives the same bits.  The sample colours come from the oracle:
orc.sample_pixels(...)[0] is [n][spp][3], the colours BEFORE the fold's clamp — orc.fold_samples of them equals orc.render bit
for bit (checked on cornell_box 80x60, where their maximum is 26.6: unclamped values do occur)."""
import numpy as np

import orc

F = np.float32
KR, KG, KB = F(0.2126), F(0.7152), F(0.0722)
RSE_FLOOR = F(0.01)


def luminance(col):
    """L = (0.2126 r + 0.7152 g) + 0.0722 b in float32, one rounding per operation."""
    col = np.asarray(col, F)
    return (KR * col[..., 0] + KG * col[..., 1]) + KB * col[..., 2]


def update(col, first_n, moments=None):
    """The moments after the samples col[..., spp, 3] entered in order with N = first_n, first_n + 1, ...; `moments`
    [..., 2] = (m1, m2) before them (ignored by N == 1, which overwrites).  Returns a new [..., 2] float32 array."""
    col = np.asarray(col, F)
    L = luminance(col)
    shape = col.shape[:-2]
    if moments is None:
        m1, m2 = np.zeros(shape, F), np.zeros(shape, F)
    else:
        m1, m2 = np.array(moments[..., 0], F), np.array(moments[..., 1], F)
    for s in range(col.shape[-2]):
        N = first_n + s
        l = L[..., s]
        if N == 1:
            m1, m2 = l.copy(), l * l
        else:
            fm1, inv = F(N - 1), F(1.0) / F(N)
            m1 = (m1 * fm1 + l) * inv
            m2 = (m2 * fm1 + l * l) * inv
    assert m1.dtype == F and m2.dtype == F
    return np.stack([m1, m2], axis=-1)


def rse(moments, n_samples):
    """Per-pixel relative standard error of the mean luminance, float32."""
    m = np.asarray(moments, F)
    m1, m2 = m[..., 0], m[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.maximum(F(0), m2 - m1 * m1)
        out = np.sqrt(var / F(n_samples - 1)) / (m1 + RSE_FLOOR)
    assert out.dtype == F
    return out


def frame_error(moments, n_samples, threshold):
    """(mean_rse, n_above) as pt_frame_error defines them: rse in float32 per pixel, summed in float64."""
    r = rse(moments, n_samples).reshape(-1)
    return float(np.sum(r.astype(np.float64)) / r.size), int(np.count_nonzero(r > F(threshold)))


def oracle_moments(bvh, spheres, cam, params, spp, materials=None, tri_material=None, pixels=None):
    """The reference moments of a whole frame (or of `pixels` [n][2] = (x, y)) rendered with `params` (frame, sample_index,
    flags as given) and spp samples, from the oracle's per-sample colours over the host tree `bvh`.  Returns (moments
    [H][W][2] or [n][2], colours [.., spp, 3])."""
    W, H = params.width, params.height
    if pixels is None:
        ys, xs = np.mgrid[0:H, 0:W]
        px = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=-1)
    else:
        px = np.asarray(pixels, np.int32).reshape(-1, 2)
    col, _, _ = orc.sample_pixels(px, spheres, cam, params, spp, bvh=bvh, materials=materials, tri_material=tri_material)
    m = update(col, int(params.sample_index))
    if pixels is None:
        return m.reshape(H, W, 2), col.reshape(H, W, spp, 3)
    return m, col
