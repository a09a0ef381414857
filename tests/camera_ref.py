"""Reference of pt_camera_rays (include/ptmi.h; csrc/pt_camera.hip): the random stream restated exactly, and the five camera
models in float64 with their inverse mappings.  A plain module found through tests/ on sys.path, like orc and env_ref; no GPU, no
library.

The stream — pt_wang64, pt_rng_init, pt_rng_next of csrc/pt_math.h — is integer arithmetic and one exact conversion, so numpy's
uint64 / uint32 restate it bit for bit.  The models are float64 on purpose: the device computes them in binary32, and the tests
give that a stated margin in pixels (tests/test_gpu_camera.py) instead of restating a libm.  An inverse takes a ray (origin,
direction) back to the continuous pixel coordinates (px + jx, py + jy) it was made for, an integer being a pixel centre; every
model but the pinhole assumes an orthonormal basis, as the device does."""
import numpy as np

PINHOLE, THIN_LENS, ORTHO, FISHEYE, EQUIRECT = range(5)
LENS_KEY = 0xC3A5C85C97CB3127   # PT_CAM_LENS_KEY
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------- the stream, exact
def wang64(key):
    """pt_wang64 (uf::hash) of a Python int, as a Python int."""
    k = int(key) & _M64
    k = ((~k) + (k << 21)) & _M64
    k ^= k >> 24
    k = ((k + (k << 3)) + (k << 8)) & _M64
    k ^= k >> 14
    k = ((k + (k << 2)) + (k << 4)) & _M64
    k ^= k >> 28
    k = (k + (k << 31)) & _M64
    return k


def rng_init(frame_hash, pixels):
    """pt_rng_init for an array of pixel numbers: (s0, s1) as uint32 arrays."""
    with np.errstate(over="ignore"):
        z = np.uint64(frame_hash) + np.asarray(pixels).astype(np.uint64)
        z ^= z >> np.uint64(33)
        z *= np.uint64(0xff51afd7ed558ccd)
        z ^= z >> np.uint64(33)
        z *= np.uint64(0xc4ceb9fe1a85ec53)
        z ^= z >> np.uint64(33)
    return (z & np.uint64(0xFFFFFFFF)).astype(np.uint32), (z >> np.uint64(32)).astype(np.uint32)


def _fmix32(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x85EBCA6B)
        x = x ^ (x >> np.uint32(13))
        x = x * np.uint32(0xC2B2AE35)
        x = x ^ (x >> np.uint32(16))
    return x


def rng_next(s0, s1, n):
    """Draw number n (0, 1, ...) of the streams (s0, s1): float32 in (0, 1], pt_rng_next."""
    with np.errstate(over="ignore"):
        x = _fmix32(s0 + np.uint32((n * 0x9E3779B9) & 0xFFFFFFFF))
    x = _fmix32(x ^ s1)
    return ((x >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)


def draws(frame, pixels, key=0):
    """The first two draws (float32) of the stream of (frame ^ key, pixel): key 0 the jitter stream, LENS_KEY the lens stream."""
    s0, s1 = rng_init(wang64(int(frame) ^ key), pixels)
    return rng_next(s0, s1, 0), rng_next(s0, s1, 1)


def jitter(frame, pixels, centre=False):
    """(jx, jy) float32 as pt_camera_rays forms them: draw - 0.5f, or 0 under PT_CAMF_CENTRE."""
    if centre:
        z = np.zeros(len(np.asarray(pixels)), np.float32)
        return z, z.copy()
    u0, u1 = draws(frame, pixels)
    return u0 - np.float32(0.5), u1 - np.float32(0.5)


# ---------------------------------------------------------------------------------------------------- the models, float64
class Model:
    """What a pt_camera and a pt_camera_model say, as float64 (the binary32 values they hold)."""

    def __init__(self, cam, kind, W, H, lens_radius=0.0, focus_dist=1.0, ortho_height=1.0, fisheye_fov=np.pi):
        self.kind, self.W, self.H = int(kind), int(W), int(H)
        self.pos, self.front, self.right, self.up = (np.array(list(v), np.float64) for v in (cam.pos, cam.front, cam.right, cam.up))
        self.dist, self.aspect, self.fov = float(cam.dist), float(cam.aspect), float(cam.fov)
        self.R, self.focus = float(np.float32(lens_radius)), float(np.float32(focus_dist))
        self.oh, self.ffov = float(np.float32(ortho_height)), float(np.float32(fisheye_fov))

    @classmethod
    def of(cls, cam, cm):
        """From the ctypes pair the library is given."""
        return cls(cam, cm.model, cm.width, cm.height, cm.lens_radius, cm.focus_dist, cm.ortho_height, cm.fisheye_fov)

    # -- helpers
    def _offsets(self, fx, fy):
        """(ax, ay): offsets from the image centre of the continuous pixel coordinates (fx, fy) = (px + jx, py + jy)."""
        return (np.asarray(fx, np.float64) - self.W / 2.0) + 0.5, (np.asarray(fy, np.float64) - self.H / 2.0) + 0.5

    def _dir0(self, fx, fy):
        ax, ay = self._offsets(fx, fy)
        xs = ax * self.dist * self.aspect * self.fov / (self.W - 1)
        ys = ay * self.dist * self.fov / (self.H - 1)
        return self.front * self.dist + xs[:, None] * self.right + ys[:, None] * self.up

    def focus_point(self, fx, fy):
        """THIN_LENS: the point in focus of the pixel coordinates, pf = pos + dir0 * (focus_dist / dist)."""
        return self.pos + self._dir0(fx, fy) * (self.focus / self.dist)

    def lens_offset(self, v0, v1):
        """THIN_LENS: the lens point's coordinates along (right, up) for the lens draws."""
        r, phi = self.R * np.sqrt(np.asarray(v0, np.float64)), 2.0 * np.pi * np.asarray(v1, np.float64)
        return r * np.cos(phi), r * np.sin(phi)

    # -- forward: continuous pixel coordinates -> (o, d, has_ray)
    def rays(self, fx, fy, v0=None, v1=None):
        fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
        n = len(fx)
        o = np.tile(self.pos, (n, 1))
        has = np.ones(n, bool)
        if self.kind == PINHOLE:
            dir0 = self._dir0(fx, fy)
            o, d = self.pos + dir0, dir0
        elif self.kind == THIN_LENS:
            lx, ly = self.lens_offset(np.zeros(n) if v0 is None else v0, np.zeros(n) if v1 is None else v1)
            o = self.pos + lx[:, None] * self.right + ly[:, None] * self.up
            d = self.focus_point(fx, fy) - o
        elif self.kind == ORTHO:
            ax, ay = self._offsets(fx, fy)
            o = self.pos + (ax * self.oh * self.aspect / self.W)[:, None] * self.right + (ay * self.oh / self.H)[:, None] * self.up
            d = np.tile(self.front, (n, 1))
        elif self.kind == FISHEYE:
            ax, ay = self._offsets(fx, fy)
            rho = np.hypot(ax, ay)
            theta = rho / (min(self.W, self.H) / 2.0) * (self.ffov / 2.0)
            has = theta <= self.ffov / 2.0
            k = np.where(rho > 0, np.sin(theta) / np.where(rho > 0, rho, 1.0), 0.0)
            d = np.cos(theta)[:, None] * self.front + (ax * k)[:, None] * self.right + (ay * k)[:, None] * self.up
        else:
            lon = (fx - self.W / 2.0) * (2.0 * np.pi / self.W)
            lat = np.clip((fy - self.H / 2.0) * (np.pi / self.H), -np.pi / 2, np.pi / 2)
            d = np.cos(lat)[:, None] * (np.cos(lon)[:, None] * self.front + np.sin(lon)[:, None] * self.right) + np.sin(lat)[:, None] * self.up
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        d[~has] = 0.0
        return o, d, has

    # -- inverse: (o, d) -> continuous pixel coordinates
    def _pinhole_coords(self, v):
        """The pixel coordinates of the pinhole ray through pos along v."""
        a, b, c = v @ self.front, v @ self.right, v @ self.up
        ax = (b / a) * (self.W - 1) / (self.aspect * self.fov)
        ay = (c / a) * (self.H - 1) / self.fov
        return ax + self.W / 2.0 - 0.5, ay + self.H / 2.0 - 0.5

    def pixel_coords(self, o, d):
        """(fx, fy) float64 of rays (o [n][3], d [n][3], taken as the values they are).  Rows without a direction give NaN."""
        o, d = np.asarray(o).astype(np.float64), np.asarray(d).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.kind == PINHOLE:
                return self._pinhole_coords(d)
            if self.kind == THIN_LENS:   # where the line meets the plane in focus, seen from pos
                t = (self.focus - (o - self.pos) @ self.front) / (d @ self.front)
                return self._pinhole_coords(o + t[:, None] * d - self.pos)
            if self.kind == ORTHO:
                ax = ((o - self.pos) @ self.right) * self.W / (self.oh * self.aspect)
                ay = ((o - self.pos) @ self.up) * self.H / self.oh
                return ax + self.W / 2.0 - 0.5, ay + self.H / 2.0 - 0.5
            a, b, c = d @ self.front, d @ self.right, d @ self.up
            if self.kind == FISHEYE:
                s = np.hypot(b, c)
                rho = np.arctan2(s, a) / (self.ffov / 2.0) * (min(self.W, self.H) / 2.0)
                k = np.where(s > 0, rho / np.where(s > 0, s, 1.0), 0.0)
                k = np.where((a == 0) & (s == 0), np.nan, k)
                return b * k + self.W / 2.0 - 0.5, c * k + self.H / 2.0 - 0.5
            lon, lat = np.arctan2(b, a), np.arctan2(c, np.sqrt(a * a + b * b))   # env_ref.positions' statements
            none = (a == 0) & (b == 0) & (c == 0)
            return np.where(none, np.nan, lon * (self.W / (2.0 * np.pi)) + self.W / 2.0), np.where(none, np.nan, lat * (self.H / np.pi) + self.H / 2.0)


def pixel_grid(W, H):
    """(pix, px, py) of every pixel, row-major."""
    pix = np.arange(W * H, dtype=np.int64)
    return pix, pix % W, pix // W
