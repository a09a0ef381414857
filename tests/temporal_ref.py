"""CPU reference of pt_temporal — TEST INFRASTRUCTURE ONLY (numpy).

temporal():  the contract of include/ptmi.h (pt_temporal): the projection into the previous camera (v, a, b, c, fx, fy and the
             bilinear weights) and every test of a tap in float32, in the stated order; the tap sums in float64.  Also returns
             the mask of FRAGILE pixels, where one rounding of difference between two float32 restatements could flip a decision.
moved():     a camera panned about its `up`, moved along its `front` (dolly) or along its `right` (sideways).
Also the inputs and bars that the CPU tests (test_temporal) and the GPU tests (test_gpu_temporal) of the feature share.
"""
import numpy as np

import gpu_pathtracer_amd as g
from denoise_ref import F32, fma, vdot

# The camera moves of the GPU comparison, applied to the golden camera (previous frame) to get the current one
MOVES = {"static": {}, "pan": dict(pan_deg=2.0), "dolly": dict(dolly=0.5), "side": dict(side=0.3)}
# The parameter sets of the GPU comparison
PARAM_SETS = {"defaults": {}, "history1": dict(max_history=1.0), "plane0": dict(plane_tolerance=0.0), "normal-1": dict(normal_threshold=-1.0)}
FRAGILE_MAX = 0.02
# The quality sequence: cornell_box, QUALITY_FRAMES frames of QUALITY_SPP samples, the camera panning QUALITY_PAN degrees a frame.
QUALITY_FRAMES, QUALITY_SPP, QUALITY_PAN = 8, 4, 1.0
# gain = MSE(last frame alone) / MSE(history), both against 1024 spp at the last camera.  The numpy reference over oracle renders
# at 80x60 measures 3.48 (test_reference_gain_on_oracle_renders asserts it); the bar for the GPU at 320x240 is 0.8 x that figure,
# the margin for the other sample sets at the other resolution.
QUALITY_GAIN_CPU = 3.48
QUALITY_K = 0.8 * QUALITY_GAIN_CPU
ACCEPTED_MIN = 0.70


def params(**kw):
    d = dict(g.TEMPORAL_DEFAULTS)
    d.update(kw)
    return d


def random_frames(W, H, seed):
    rng = np.random.default_rng(seed)
    cur, prev = (rng.uniform(0, 1, (H, W, 3)).astype(np.float32) for _ in range(2))
    ln = rng.integers(1, 41, (H, W)).astype(np.float32)
    return cur, prev, ln


def moved(cam, pan_deg=0.0, dolly=0.0, side=0.0):
    """A copy of `cam`: front and right turned by pan_deg about up (Rodrigues, in double), then pos moved along the new front
    (dolly) and the new right (side).  Same mapping as pt_app's --pan-deg / --dolly."""
    c = g.Camera.from_buffer_copy(cam)
    up = np.array(list(cam.up), np.float64)
    th = np.deg2rad(pan_deg)

    def rot(v):
        v = np.array(list(v), np.float64)
        return v * np.cos(th) + np.cross(up, v) * np.sin(th) + up * np.dot(up, v) * (1.0 - np.cos(th))

    f, r = rot(cam.front), rot(cam.right)
    pos = np.array(list(cam.pos), np.float64) + dolly * f + side * r
    c.front[:], c.right[:], c.pos[:] = [float(x) for x in f], [float(x) for x in r], [float(x) for x in pos]
    return c


def temporal(W, H, prev_cam, prev_color, prev_length, prev_normal, prev_position, prev_id,
             cur_color, cur_normal, cur_position, cur_id, max_history, plane_tolerance, normal_threshold, pixels=None):
    """pt_temporal's arithmetic.  Colours float[H][W][3], lengths float[H][W], guides float[H][W][4], ids int32[H][W] or None
    (both or neither).  prev_color None = no history.  With pixels = (ys, xs) the outputs are those pixels only.
    Returns (out float32[...][3], length float32[...], fragile bool[...], accepted bool[...])."""
    cur_color = np.asarray(cur_color, F32)
    if pixels is None:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    else:
        ys, xs = (np.asarray(v, np.int64) for v in pixels)
    cur = cur_color[ys, xs]
    shp = ys.shape
    out, length = cur.copy(), np.ones(shp, F32)
    fragile, accepted = np.zeros(shp, bool), np.zeros(shp, bool)
    if prev_color is None:
        return out, length, fragile, accepted
    assert (prev_id is None) == (cur_id is None)
    prev_color, prev_length = np.asarray(prev_color, F32), np.asarray(prev_length, F32)
    prev_normal, prev_position = np.asarray(prev_normal, F32), np.asarray(prev_position, F32)
    n_p = np.asarray(cur_normal, F32)[ys, xs][..., 0:3]
    x_p = np.asarray(cur_position, F32)[ys, xs][..., 0:3]
    t_p = np.asarray(cur_position, F32)[ys, xs][..., 3]
    hit = np.any(n_p != 0, axis=-1)

    def vec(a):
        return np.array(list(a), F32)

    with np.errstate(all="ignore"):
        v = (x_p - vec(prev_cam.pos)).astype(F32)
        a, b, c = vdot(v, vec(prev_cam.front)), vdot(v, vec(prev_cam.right)), vdot(v, vec(prev_cam.up))
        sx = F32(F32(W - 1) / F32(F32(prev_cam.aspect) * F32(prev_cam.fov)))
        sy = F32(F32(H - 1) / F32(prev_cam.fov))
        cx, cy = F32(F32(W) / F32(2.0) - F32(0.5)), F32(F32(H) / F32(2.0) - F32(0.5))
        fx = fma((b / a).astype(F32), sx, cx)
        fy = fma((c / a).astype(F32), sy, cy)
        front_ok = hit & (a > 0)
        ok = front_ok & np.isfinite(fx) & np.isfinite(fy)
        # a within 1e-5 (relative to |v|) of 0: the side of the previous camera's plane is not certain
        fragile |= hit & (np.abs(a.astype(np.float64)) <= 1e-5 * np.sqrt(np.sum(v.astype(np.float64) ** 2, -1)))
        fxs, fys = np.where(ok, fx, F32(-8)), np.where(ok, fy, F32(-8))
        fxs, fys = np.clip(fxs, F32(-8), F32(W + 8)), np.clip(fys, F32(-8), F32(H + 8))   # far outside stays outside, and converts
        x0f, y0f = np.floor(fxs), np.floor(fys)
        wx, wy = (fxs - x0f).astype(F32), (fys - y0f).astype(F32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = (F32(plane_tolerance) * t_p).astype(F32)
        sw = np.zeros(shp, np.float64)
        sc = np.zeros(shp + (3,), np.float64)
        sl = np.zeros(shp, np.float64)
        for j in (0, 1):
            for i in (0, 1):
                xq, yq = x0 + i, y0 + j
                w = ((wx if i else (F32(1.0) - wx).astype(F32)) * (wy if j else (F32(1.0) - wy).astype(F32))).astype(F32)
                cand = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H) & (w > 0)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                n_q, x_q = prev_normal[yc, xc][..., 0:3], prev_position[yc, xc][..., 0:3]
                cand &= np.any(n_q != 0, axis=-1)
                if prev_id is not None:
                    cand &= np.asarray(prev_id)[yc, xc] == np.asarray(cur_id)[ys, xs]
                nd = vdot(n_p, n_q)
                pd = np.abs(vdot(n_p, (x_q - x_p).astype(F32)))
                fragile |= cand & (np.abs(nd.astype(np.float64) - normal_threshold) <= 1e-4)
                # (strictly inside the band: at plane_tolerance = 0 it is empty — the test is then pd == 0, an exact cancellation
                # that every binary32 restatement of the same operations reproduces)
                fragile |= cand & (nd >= F32(normal_threshold)) & (np.abs(pd.astype(np.float64) - tol) < 1e-3 * tol)
                good = cand & (nd >= F32(normal_threshold)) & (pd <= tol)
                wq = np.where(good, w, F32(0)).astype(np.float64)
                sw += wq
                sc += wq[..., None] * prev_color[yc, xc]
                sl += wq * prev_length[yc, xc]
        fragile |= ok & (np.abs(sw - 0.01) <= 1e-3)
        accepted = ok & (sw.astype(F32) >= F32(0.01))
        swd = np.where(accepted, sw, 1.0)
        hist = sc / swd[..., None]
        n = np.minimum(sl / swd + 1.0, float(F32(max_history)))
        blend = hist + (cur.astype(np.float64) - hist) / n[..., None]
    out = np.where(accepted[..., None], blend.astype(F32), cur)
    length = np.where(accepted, n.astype(F32), F32(1.0))
    return out, length, fragile, accepted
