"""CPU reference of pt_denoise_variance and pt_temporal_moments — TEST INFRASTRUCTURE ONLY (numpy).

seed():              the seed of include/ptmi.h (pt_denoise_variance) in binary32, one rounding per operation as the header
                     states it: (var_p, i0, v0).
atrous_variance():   the filter contract in numpy: the binary32 seed, then float64 throughout, in the style of
                     denoise_ref.atrous (its `pixels=` option included).
temporal_moments():  pt_temporal_moments: the taps, the acceptance and n are temporal_ref.temporal's / motion_ref's own code run
                     on the payload (m1, m2, 0); the blend restated in binary32, out = fmaf(cur - hist, 1 / n, hist).
Also the inputs and bars that the CPU tests (test_denoise_variance) and the GPU tests (test_gpu_denoise_variance) share.
"""
import numpy as np

import denoise_ref as R
import moments_ref
import motion_ref
import temporal_ref
from denoise_ref import F32, H5, fma

# gain = MSE(noisy) / MSE(filtered), both against 8192 spp of cornell_box, that DENOISE_VARIANCE_DEFAULTS must reach at EVERY
# sample count (4, 64, 1024 spp); at 1024 spp the gain must also exceed 1 where pt_denoise's defaults fall below 1.
# Re-measured with this module over oracle frames at 80x60 (test_denoise_variance.test_quality_on_oracle_renders prints them):
#   variance-guided 2.68 / 3.82 / 2.05 at 4 / 64 / 1024 spp; pt_denoise's defaults 2.97 / 4.71 / 0.96.
VAR_QUALITY_K = 1.5
QUALITY_SPP = (4, 64, 1024)
QUALITY_REF_SPP = 8192
QUALITY_NOISY_FRAME = 1 << 20

G3 = np.array([1.0, 2.0, 1.0])
KR, KG, KB = 0.2126, 0.7152, 0.0722


def luminance64(c):
    """L(c) in float64 with the binary32 constants of the header."""
    c = np.asarray(c, np.float64)
    return (float(F32(KR)) * c[..., 0] + float(F32(KG)) * c[..., 1]) + float(F32(KB)) * c[..., 2]


# ---------------------------------------------------------------------------------------------------- the seed
def seed(color, moments, length, albedo, samples_per_frame):
    """(var_p float32[H][W], i0 float32[H][W][3], v0 float32[H][W]) in binary32, operation for operation."""
    color = np.asarray(color, F32)
    m = np.asarray(moments, F32)
    m1, m2 = m[..., 0], m[..., 1]
    ln = np.ones(m1.shape, F32) if length is None else np.asarray(length, F32)
    with np.errstate(all="ignore"):
        n = (F32(samples_per_frame) * ln).astype(F32)
        many = n >= F32(2)
        var = np.where(many, np.fmax(F32(0), (m2 - (m1 * m1).astype(F32)).astype(F32)) / np.where(many, n - F32(1), F32(1)), m2).astype(F32)
        var = np.fmin(np.fmax(var, F32(0)), F32(1e30)).astype(F32)     # fmaxf / fminf: a NaN counts as 0
        a = R.demod_albedo(albedo)
        la = moments_ref.luminance(a)
        v0 = (var / (la * la).astype(F32)).astype(F32)
        i0 = (color / a).astype(F32)
    return var, i0, v0


# ---------------------------------------------------------------------------------------------------- the filter
def prefilter(v, hit, ys, xs):
    """g_p at the pixels (ys, xs): the (1,2,1)x(1,2,1) mean of v over the adjacent pixels inside the image with p's hit flag."""
    H, W = v.shape
    num = np.zeros(ys.shape, np.float64)
    den = np.zeros(ys.shape, np.float64)
    hp = hit[ys, xs]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yq, xq = ys + dy, xs + dx
            ok = (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
            yc, xc = np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)
            w = np.where(ok & (hit[yc, xc] == hp), G3[dy + 1] * G3[dx + 1], 0.0)
            num += w * v[yc, xc]
            den += w
    return num / den


def atrous_variance(color, moments, length, albedo, normal, position, iterations, sigma_luminance, sigma_normal, sigma_position,
                    samples_per_frame=1.0, pixels=None, weights_out=None):
    """pt_denoise_variance's arithmetic.  color float[H][W][3]; moments float[H][W][2]; length float[H][W] or None; guides
    float[H][W][4].  Returns (out float32[H][W][3], out_variance float32[H][W]), or, with pixels = (ys, xs), both at those pixels
    only (the last iteration is evaluated there alone).  weights_out: a list that receives, per iteration, the dict
    {(dy, dx): w} of the full-frame tap weights (for the tests of the weights)."""
    color = np.asarray(color, F32)
    H, W = color.shape[:2]
    var, i0, v0 = seed(color, moments, length, albedo, samples_per_frame)
    if iterations == 0:
        out = color.copy()
        return (out, var) if pixels is None else (out[pixels], var[pixels])
    a = R.demod_albedo(albedo)
    la = luminance64(a)
    hit = np.any(np.asarray(normal, F32)[..., 0:3] != 0, axis=-1)
    nrm = np.asarray(normal, np.float64)[..., 0:3]
    pos = np.asarray(position, np.float64)[..., 0:3]
    tp = np.asarray(position, np.float64)[..., 3]
    img, v = i0.astype(np.float64), v0.astype(np.float64)
    for l in range(iterations):
        last = l == iterations - 1
        if last and pixels is not None:
            ys, xs = (np.asarray(t, np.int64) for t in pixels)
        else:
            ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        s = 1 << l
        ip, hp = img[ys, xs], hit[ys, xs]
        lp = luminance64(ip)
        k = np.zeros(ys.shape, np.float64)
        if sigma_luminance > 0:
            sd = np.sqrt(np.maximum(prefilter(v, hit, ys, xs), 0.0))
            k = 1.0 / (float(F32(sigma_luminance)) * sd + 1e-4)
        num = np.zeros(ip.shape, np.float64)
        numv = np.zeros(ip.shape[:-1], np.float64)
        den = np.zeros(ip.shape[:-1], np.float64)
        taps = {}
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yq, xq = ys + s * dy, xs + s * dx
                ok = (yq >= 0) & (yq < H) & (xq >= 0) & (xq < W)
                yc, xc = np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)
                iq, hq = img[yc, xc], hit[yc, xc]
                e = np.abs(lp - luminance64(iq)) * k
                both = hp & hq
                if sigma_normal > 0:
                    e = e + np.where(both, np.sum((nrm[ys, xs] - nrm[yc, xc]) ** 2, -1), 0.0) / sigma_normal ** 2
                if sigma_position > 0:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ex = np.sum((pos[ys, xs] - pos[yc, xc]) ** 2, -1) / (sigma_position * tp[ys, xs]) ** 2
                    e = e + np.where(both, ex, 0.0)
                w = np.where(ok & (hp == hq), H5[dy + 2] * H5[dx + 2] * np.exp(-e), 0.0)
                taps[(dy, dx)] = w
                num += w[..., None] * iq
                numv += w * w * v[yc, xc]
                den += w
        if weights_out is not None:
            weights_out.append(taps)
        nxt, nv = num / den[..., None], numv / den ** 2
        if last:
            return np.clip(nxt * a[ys, xs], 0.0, 1.0).astype(F32), (nv * la[ys, xs] ** 2).astype(F32)
        img, v = nxt, nv


# ---------------------------------------------------------------------------------------------------- the moments reprojection
def temporal_moments(W, H, prev_cam, prev_verts, cur_verts, n_tris, prev_moments, prev_length, prev_normal, prev_position, prev_id,
                     cur_moments, cur_normal, cur_position, cur_id, max_history, plane_tolerance, normal_threshold):
    """pt_temporal_moments over whole frames: (out float32[H][W][2], fragile bool[H][W], accepted bool[H][W]).  Both vertex
    arrays None: temporal_ref.temporal decides the taps; otherwise motion_ref.temporal_motion does.  The history value and n come
    from those functions' float64 sums, through their own outputs; the blend is binary32."""
    cur = np.asarray(cur_moments, F32)
    if prev_moments is None:
        return cur.copy(), np.zeros((H, W), bool), np.zeros((H, W), bool)

    def pad(m):
        return np.concatenate([np.asarray(m, F32), np.zeros(np.shape(m)[:2] + (1,), F32)], -1)

    pm, cm = pad(prev_moments), pad(cur)

    def run(lengths, cc, mh):
        if prev_verts is None and cur_verts is None:
            return temporal_ref.temporal(W, H, prev_cam, pm, lengths, prev_normal, prev_position, prev_id, cc, cur_normal,
                                         cur_position, cur_id, mh, plane_tolerance, normal_threshold)
        o, ln, _, fr, ac = motion_ref.temporal_motion(W, H, prev_cam, prev_verts, cur_verts, n_tris, pm, lengths, prev_normal,
                                                      prev_position, prev_id, cc, cur_normal, cur_position, cur_id, mh,
                                                      plane_tolerance, normal_threshold)
        return o, ln, fr, ac

    _, n, fragile, accepted = run(prev_length, cm, max_history)     # n = fminf(sl / sw + 1, max_history): the colour call's out_length
    # the history value itself: those functions blend hist + (cur - hist) / n in float64, so an unbounded max_history, lengths of
    # 1e30 and cur = 0 leave hist (1 - 1e-30) = hist, rounded once
    h = run(np.full((H, W), 1e30, F32), np.zeros_like(cm), 3.0e38)[0][..., 0:2]
    inv = (F32(1.0) / n).astype(F32)
    out = fma((cur - h).astype(F32), inv[..., None], h)     # the blend in binary32: fmaf(cur - hist, 1.0f / n, hist)
    return np.where(accepted[..., None], out, cur).astype(F32), fragile, accepted
