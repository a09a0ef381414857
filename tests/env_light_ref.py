"""numpy restatement of the environment map as a light (PT_OPT_ENV_LIGHT, include/ptmi.h "The map as a light"; csrc/pt_env.h,
pt_env.hip): the sampling tables from the definition in float64, the draw and the density in float32 as the device computes them,
and what the tests compare against in float64 — the texels' solid angles, the map's integral and the radiance a horizontal diffuse
plane gathers from a nearest-filtered map.  A plain module found through tests/ on sys.path, like env_ref; no GPU, no library."""
import numpy as np

import env_ref

F32, F64 = np.float32, np.float64
ONE_BELOW = F32(1.0) - F32(2.0 ** -24)   # 0x1.fffffep-1f


class Tables:
    """cx float32 [H][W + 1], cy float32 [H + 1], zs float32 [H + 1]; m float64 [H][W] the texel weights, T their total."""

    def __init__(self, texels, bilinear):
        t = np.asarray(texels, F32)
        H, W = t.shape[:2]
        m = t.max(axis=2).astype(F64)
        if bilinear:   # the maximum over the 3 x 3 neighbourhood, columns wrapped, rows clamped
            rows = np.stack([m[np.clip(np.arange(H) + dy, 0, H - 1)] for dy in (-1, 0, 1)]).max(axis=0)
            m = np.stack([np.roll(rows, dx, axis=1) for dx in (-1, 0, 1)]).max(axis=0)
        e = (np.arange(H + 1, dtype=F64) - 0.5 - H / 2.0) * np.pi / H
        zs = np.sin(e).astype(F32)
        zs[0], zs[H] = -1.0, 1.0
        # np.cumsum adds in ascending index, one at a time: the sequential sums of the definition
        part = np.concatenate([np.zeros((H, 1)), np.cumsum(m, axis=1)], axis=1)
        S = part[:, W]
        with np.errstate(invalid="ignore", divide="ignore"):
            cx = np.where(S[:, None] > 0, part / S[:, None], np.arange(W + 1, dtype=F64)[None, :] / W).astype(F32)
        cx[:, 0], cx[:, W] = 0.0, 1.0
        A = S * (zs[1:].astype(F64) - zs[:-1].astype(F64))
        party = np.concatenate([[0.0], np.cumsum(A)])
        self.T = float(party[H])
        assert self.T > 0, "a black map carries no tables"
        cy = (party / self.T).astype(F32)
        cy[0], cy[H] = 0.0, 1.0
        self.W, self.H, self.m, self.cx, self.cy, self.zs = W, H, m, cx, cy, zs
        self.kx, self.hx = F32(W / (2.0 * np.pi)), F32(W / 2.0)

    def omega(self):
        """The solid angle of every texel's nearest cell, float64 [H]: 2 pi / W * (zs[y + 1] - zs[y])."""
        return 2.0 * np.pi / self.W * (self.zs[1:].astype(F64) - self.zs[:-1].astype(F64))

    def texel_pdf(self):
        """The density of every texel as the device computes it, float32 [H][W]: ((py * px) * kx) / dz, 0 where py * px is 0."""
        py = (self.cy[1:] - self.cy[:-1])[:, None]
        px = self.cx[:, 1:] - self.cx[:, :-1]
        dz = (self.zs[1:] - self.zs[:-1])[:, None]
        p = py * px
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(p > 0, (p * self.kx) / dz, F32(0)).astype(F32)


def clamp_u(u):
    """pt_sample_environment's clamp: into [0, 0x1.fffffep-1], a NaN to 0."""
    u = np.asarray(u, F32)
    return np.where(np.isnan(u), F32(0), np.minimum(np.maximum(u, F32(0)), ONE_BELOW)).astype(F32)


def draw(tab, u, front=env_ref.WORLD["front"], right=env_ref.WORLD["right"], up=env_ref.WORLD["up"]):
    """The draw for u float32 [n][2] in [0, 1): a dict of y, x (the texel), py, px, v1, v2, pdf (float32, the device's arithmetic)
    and d (float64 [n][3]: the direction from the float32 z, r and lon with float64 cos / sin — the device's cosf / sinf and its
    three products differ from it by a few 1e-7)."""
    u = np.asarray(u, F32)
    u1, u2 = u[:, 0], u[:, 1]
    W, H = tab.W, tab.H
    y = np.searchsorted(tab.cy[:H], u1, side="right") - 1   # the largest i in 0 .. H - 1 with cy[i] <= u1
    x = np.empty(len(u), np.int64)
    for row in np.unique(y):
        k = y == row
        x[k] = np.searchsorted(tab.cx[row, :W], u2[k], side="right") - 1
    cy0, cx0 = tab.cy[y], tab.cx[y, x]
    py, px = tab.cy[y + 1] - cy0, tab.cx[y, x + 1] - cx0
    v1 = np.minimum((u1 - cy0) / py, ONE_BELOW)
    v2 = np.minimum((u2 - cx0) / px, ONE_BELOW)
    z0 = tab.zs[y]
    dz = tab.zs[y + 1] - z0
    z = z0 + v1 * dz
    r = np.sqrt(np.maximum(F32(0), F32(1) - z * z))
    lon = (((x.astype(F32) - F32(0.5)) + v2) - tab.hx) / tab.kx
    f, rt, upv = (np.asarray(v, F32).astype(F64) for v in (front, right, up))
    r64, z64, lon64 = r.astype(F64), z.astype(F64), lon.astype(F64)
    d = (r64 * np.cos(lon64))[:, None] * f + (r64 * np.sin(lon64))[:, None] * rt + z64[:, None] * upv
    p = py * px
    pdf = np.where(p > 0, (p * tab.kx) / dz, F32(0)).astype(F32)
    assert all(a.dtype == F32 for a in (py, px, v1, v2, z, r, lon, pdf))
    return dict(y=y, x=x, py=py, px=px, v1=v1, v2=v2, d=d, pdf=pdf)


def texel_of(d, W, H, **basis):
    """(y, x, valid): the texel a nearest lookup of directions [n][3] picks (env_ref.positions, float64)."""
    fx, fy, valid = env_ref.positions(d, W, H, **basis)
    return np.clip(np.floor(fy + 0.5).astype(np.int64), 0, H - 1), np.mod(np.floor(fx + 0.5).astype(np.int64), W), valid


def pdf_of(tab, d, **basis):
    """The density of directions [n][3]: the nearest texel's, 0 for an invalid direction."""
    y, x, valid = texel_of(d, tab.W, tab.H, **basis)
    return np.where(valid, tab.texel_pdf()[y, x], F32(0)).astype(F32)


def interior(s, margin=0.01):
    """The draws that lie at least `margin` of their texel away from its edges in both coordinates."""
    return (s["v1"] >= margin) & (s["v1"] <= 1 - margin) & (s["v2"] >= margin) & (s["v2"] <= 1 - margin)


def integral(tab, texels):
    """I = sum over the texels of L * Omega for a nearest-filtered map, float64 [3]."""
    return (np.asarray(texels, F32).astype(F64) * tab.omega()[:, None, None]).sum(axis=(0, 1))


def plane_radiance(tab, texels, albedo):
    """E: what a diffuse plane whose normal is the map's `up` sends back under a nearest-filtered map, float64 [3]:
    rho / pi * sum_t L_t * (2 pi / W) * (max(0, zs[y + 1])^2 - max(0, zs[y])^2) / 2  (the integral of cos over a texel's cell)."""
    zs = np.maximum(tab.zs.astype(F64), 0.0)
    cosw = 2.0 * np.pi / tab.W * (zs[1:] ** 2 - zs[:-1] ** 2) / 2.0
    return np.asarray(albedo, F64) / np.pi * (np.asarray(texels, F32).astype(F64) * cosw[:, None, None]).sum(axis=(0, 1))


def stratified(n=64, seed=11):
    """u: an n x n stratified grid — one point uniform in every cell, so that the position inside whatever texel a point falls in
    is uniform too — plus the corners 0 and 1 - 2^-24, float32 [n * n + 2][2].  (Cell centres would not do: on a map with one hot
    texel they are the residuals themselves, a regular lattice.)"""
    rng = np.random.default_rng(seed)
    i = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    g = np.minimum((i + rng.random((n * n, 2))) / n, 1.0 - 2.0 ** -24)
    return np.concatenate([g, [[0.0, 0.0], [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]]]).astype(F32)


def black_rows_map():
    """64 x 32, gradient, with whole rows black: rows 0-3 (a pole and its neighbours), 10-11 and 31 (the other pole's row)."""
    t = env_ref.gradient_map(64, 32)
    t[[0, 1, 2, 3, 10, 11, 31]] = 0
    return t


def draw_cases():
    """(id, texels, bilinear) of the draw tests, CPU and GPU: 1 x 1, 2 x 1, 5 x 3 and 16 x 8 maps, a gradient and one hot texel in
    a black map, nearest and bilinear; 64 x 32 with one hot texel and with whole black rows."""
    out = []
    for W, H in [(1, 1), (2, 1), (5, 3), (16, 8)]:
        for kind, tex in (("gradient", env_ref.gradient_map(W, H)), ("hot", hot_map(W, H, H // 2, W // 3, 50.0))):
            for bil in (False, True):
                out.append((f"{W}x{H}-{kind}-{'bilinear' if bil else 'nearest'}", tex, bil))
    out.append(("64x32-hot-nearest", hot_map(64, 32, 23, 10), False))
    out.append(("64x32-hot-bilinear", hot_map(64, 32, 23, 10), True))
    out.append(("64x32-black-rows-nearest", black_rows_map(), False))
    out.append(("64x32-black-rows-bilinear", black_rows_map(), True))
    return out


def hot_map(W, H, y, x, value=1000.0, ambient=0.0):
    """ambient everywhere, `value` in one texel; float32 [H][W][3]."""
    t = np.full((H, W, 3), ambient, F32)
    t[y, x] = value
    return t
