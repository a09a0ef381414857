"""numpy restatement of adaptive sampling's arithmetic (include/ptmi.h): pt_render_pixels' fold of sample colours into a pixel's
running mean and luminance moments from the pixel's own sample count on, and pt_select_pixels' rule.

binary32 throughout, one rounding per operation, as the device code (plain * and +, no fused multiply-add): numpy's float32
arithmetic gives the same bits for +, *, / and sqrt.  The moments are moments_ref's formula with N = count + 1 + s."""
import numpy as np

import moments_ref as M

F = np.float32
UINT32_MAX = 0xFFFFFFFF


def fold(col, counts, accum, moments=None, hdr=False):
    """The buffers after the samples col[n][spp][3] of n pixels entered in order, pixel i from its count counts[i] on
    (N = counts[i] + 1 + s; N == 1 overwrites whatever the buffers held).  accum [n][3], moments [n][2] or None.  Returns new
    (accum, moments, counts); hdr: no clamp of the mean to 0..1 after each sample."""
    col = np.asarray(col, F)
    n, spp = col.shape[0], col.shape[1]
    counts = np.asarray(counts, np.uint32)
    a = np.array(accum, F).reshape(n, 3)
    m = None if moments is None else np.array(moments, F).reshape(n, 2)
    for s in range(spp):
        N = counts.astype(np.int64) + 1 + s
        first = N == 1
        fm1 = (N - 1).astype(F)[:, None]          # exact below 2^24; (float)(N - 1) rounds the same way above
        inv = (F(1.0) / N.astype(F))[:, None]
        c = col[:, s, :]
        cont = (a * fm1 + c) * inv
        a = np.where(first[:, None], (F(0.0) + c) * F(1.0), cont)
        if not hdr:
            a = np.minimum(np.maximum(a, F(0.0)), F(1.0))
        if m is not None:
            L = M.luminance(c)
            m1 = np.where(first, L, (m[:, 0] * fm1[:, 0] + L) * inv[:, 0])
            m2 = np.where(first, L * L, (m[:, 1] * fm1[:, 0] + L * L) * inv[:, 0])
            m = np.stack([m1, m2], axis=-1)
        assert a.dtype == F and (m is None or m.dtype == F)
    return a, m, (counts + np.uint32(spp)).astype(np.uint32)


def rse(moments, counts):
    """Per-pixel relative standard error of the mean luminance with each pixel's own sample count: 0 below two samples and where
    the figure is not finite.  float32."""
    m = np.asarray(moments, F).reshape(-1, 2)
    n = np.asarray(counts, np.uint32).reshape(-1)
    m1, m2 = m[:, 0], m[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = np.fmax(F(0), m2 - m1 * m1)                              # fmaxf: a NaN difference gives 0
        nm1 = np.maximum(n.astype(np.int64) - 1, 1).astype(F)
        r = np.sqrt(var / nm1) / (m1 + M.RSE_FLOOR)
    assert r.dtype == F
    return np.where((n >= 2) & np.isfinite(r), r, F(0)).astype(F)


def select(moments, counts, threshold, min_samples=0, max_samples=UINT32_MAX):
    """(selected [n] bool, rse [n] float32): a pixel is selected when its count is below max_samples and it is below
    max(min_samples, 2) or its rse is strictly above the threshold."""
    n = np.asarray(counts, np.uint32).reshape(-1).astype(np.int64)
    r = rse(moments, counts)
    return (n < int(max_samples)) & ((n < max(int(min_samples), 2)) | (r > F(threshold))), r


def mean_rse(r):
    """pt_select_pixels' *mean_rse: per 256-pixel block the sum of rse in double by pt_frame_error's tree (pairs 128 apart, then 64,
    ...), the blocks added in order, divided by the number of pixels."""
    r = np.asarray(r, F).reshape(-1)
    n_blocks = (len(r) + 255) // 256
    v = np.zeros(n_blocks * 256, np.float64)
    v[:len(r)] = r
    v = v.reshape(n_blocks, 256)
    off = 128
    while off > 0:
        v = v[:, :off] + v[:, off:2 * off]
        off //= 2
    total = 0.0
    for b in range(n_blocks):
        total += float(v[b, 0])
    return total / len(r)
