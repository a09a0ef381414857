"""numpy restatement of the environment-map lookup (pt_upload_environment, include/ptmi.h; csrc/pt_env.h): the texel positions in
float64 from the definition, the nearest pick, and the bilinear value in two precisions.  A plain module found through tests/ on
sys.path, like orc and query_ref; no GPU, no library.

Positions are float64 on purpose: the device computes them in binary32 through atan2f, and the tests give that a stated margin
(tests/test_gpu_environment.py) instead of restating a libm."""
import numpy as np

WORLD = dict(front=(0.0, 0.0, -1.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))   # pt_app's camera frame, the default of upload_environment


def equirect_dirs(W, H, front=WORLD["front"], right=WORLD["right"], up=WORLD["up"]):
    """The unit directions `pt_app --equirect` renders, float32 [H * W][3], pixel y * W + x: column x looks at longitude
    (x - W/2) 2 pi / W from front towards right, row y at latitude (y - H/2) pi / H towards up; float64, normalised, rounded once."""
    f, r, u = (np.asarray(v, np.float64) for v in (front, right, up))
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    lon, lat = (x - W / 2.0) * 2.0 * np.pi / W, (y - H / 2.0) * np.pi / H
    d = np.cos(lat)[..., None] * (np.cos(lon)[..., None] * f + np.sin(lon)[..., None] * r) + np.sin(lat)[..., None] * u
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(H * W, 3).astype(np.float32)


def rays_of(dirs, origin=(0.0, 0.0, 0.0)):
    """float32 [n][8] ray rows (o, 0, d, 0) for directions [n][3]."""
    rays = np.zeros((len(dirs), 8), np.float32)
    rays[:, 0:3] = origin
    rays[:, 4:7] = dirs
    return rays


def positions(d, W, H, front=WORLD["front"], right=WORLD["right"], up=WORLD["up"]):
    """(fx, fy, valid) in float64 for directions [n][3] (taken as the float32 values they are): steps 1-3 of the definition.
    valid is False where a component of (a, b, c) is not finite or all are 0: the lookup is (0, 0, 0) there."""
    d = np.asarray(d, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = (d @ np.asarray(v, np.float32).astype(np.float64) for v in (front, right, up))
        valid = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & ~((a == 0) & (b == 0) & (c == 0))
        a, b, c = (np.where(valid, v, 1.0) for v in (a, b, c))
        lon, lat = np.arctan2(b, a), np.arctan2(c, np.sqrt(a * a + b * b))
    return lon * (W / (2.0 * np.pi)) + W / 2.0, lat * (H / np.pi) + H / 2.0, valid


def nearest(texels, fx, fy, valid=None):
    """Step 4: column floor(fx + 0.5) wrapped, row floor(fy + 0.5) clamped; texels [H][W][3] -> [n][3]."""
    H, W = texels.shape[:2]
    col = np.mod(np.floor(fx + 0.5).astype(np.int64), W)
    row = np.clip(np.floor(fy + 0.5).astype(np.int64), 0, H - 1)
    out = texels[row, col].copy()
    if valid is not None:
        out[~valid] = 0
    return out


def bilinear(texels, fx, fy, valid=None, dtype=np.float64):
    """Step 5 at positions (fx, fy): columns x0, x0 + 1 wrapped, rows y0, y0 + 1 clamped, lerp(p, q, w) = p + w * (q - p), the
    columns within each row first, then the rows.  dtype float64: the exact value at that position; float32: the device's
    arithmetic, every step one binary32 rounding, given the weights it computed."""
    H, W = texels.shape[:2]
    x0, y0 = np.floor(fx), np.floor(fy)
    wx, wy = (fx - x0).astype(dtype)[:, None], (fy - y0).astype(dtype)[:, None]
    c0, c1 = np.mod(x0.astype(np.int64), W), np.mod(x0.astype(np.int64) + 1, W)
    r0, r1 = np.clip(y0.astype(np.int64), 0, H - 1), np.clip(y0.astype(np.int64) + 1, 0, H - 1)
    t = texels.astype(dtype)
    lo = t[r0, c0] + wx * (t[r0, c1] - t[r0, c0])
    hi = t[r1, c0] + wx * (t[r1, c1] - t[r1, c0])
    out = lo + wy * (hi - lo)
    if valid is not None:
        out[~valid] = 0
    return out


def max_step(texels):
    """g: the largest difference between adjacent texels of the map (columns wrap, rows do not), over the channels."""
    t = texels.astype(np.float64)
    g = np.abs(t - np.roll(t, 1, axis=1)).max()
    if t.shape[0] > 1:
        g = max(g, np.abs(t[1:] - t[:-1]).max())
    return float(g)


def bilinear_bound(texels):
    """What a bilinear lookup may differ by from the float64 value at the float64 position: g * 2^-12 + 4 ulp.  2^-12 texel is
    the margin given to atan2f's few-ulp error at W = 16 plus the rounding of fx (the value moves by at most g per texel); the
    ulps, of the largest texel, are for the roundings of the three lerps."""
    return max_step(texels) * 2.0 ** -12 + 4 * float(np.spacing(np.float32(texels.max())))


def gradient_map(W, H, seed=5):
    """A smooth gradient plus noise, float32 [H][W][3], positive: every texel differs from its neighbours."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * x / W), 0.3 + 0.6 * y / max(H - 1, 1), 0.6 + 0.3 * np.cos(2 * np.pi * x / W) * (y + 1) / H], -1)
    return (base + 0.05 * rng.random((H, W, 3))).astype(np.float32)


def random_dirs(n, seed=3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
