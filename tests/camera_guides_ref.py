"""CPU reference of pt_render_aux_camera and pt_temporal_camera — TEST INFRASTRUCTURE ONLY (numpy over the oracle).

guides_from_rays():   denoise_ref.guides from the oracle's walk on, over given ray rows (the rows pt_camera_rays writes under
                      PT_CAMF_CENTRE, or camera_ref.Model.rays on the CPU); a row without a direction is a miss and is never walked.
project():            where a camera model sees world points, in float64, through camera_ref.Model.pixel_coords.
rejects():            the points a model's projection turns away (include/ptmi.h, pt_temporal_camera), in float64, and the ones
                      within 1e-5 relative of such a decision (fragile).
blend_from_coords():  steps 3 to 5 of pt_temporal as temporal_ref.temporal states them — float32 tests, float64 sums, the same
                      FRAGILE rules — over given history coordinates (the device's own) instead of computing them.
Also the cases that the CPU tests (test_camera_guides) and the GPU tests (test_gpu_camera_guides) of the feature share."""
import numpy as np

import camera_ref as cr
import gpu_pathtracer_amd as g
import orc
import temporal_ref as T
from denoise_ref import F32, fma, sphere_intersect, vdot, vnormalize
from gpu_support import golden_camera

FLT_MAX = np.finfo(np.float32).max
PIXEL_BOUND = 1e-3   # tests/test_gpu_camera.py's bound, under its premise: at these sizes a pixel subtends at least 0.05 rad

# the models of the tests: name -> (kind, the model's parameters)
MODELS = {"pinhole": (cr.PINHOLE, {}), "thinlens": (cr.THIN_LENS, dict(lens_radius=0.5, focus_dist=35.0)),
          "ortho": (cr.ORTHO, dict(ortho_height=30.0)), "fisheye180": (cr.FISHEYE, dict(fisheye_fov=float(np.pi))),
          "fisheye220": (cr.FISHEYE, dict(fisheye_fov=float(np.radians(220.0)))), "equirect": (cr.EQUIRECT, {})}
SIZES = [(64, 48), (33, 17)]   # 33x17: partial tiles in both axes, an odd width
MOVED_MODELS = ("ortho", "fisheye180", "fisheye220", "equirect")
# The camera moves of the moved-camera test: temporal_ref.MOVES, scaled per model where the reference alone would miss the two
# conditions of test_camera_guides (accepted on half of the hit pixels, fragile within temporal_ref.FRAGILE_MAX); 1 = as they are.
MOVE_SCALE = {"ortho": 1.0, "fisheye180": 1.0, "fisheye220": 1.0, "equirect": 1.0}


def guide_camera(W, H):
    """The camera of the guide tests: the golden camera moved 15 units towards the box, where the mesh covers more than 5 % of the
    image of every model at every size (from the golden camera's own place the room's wall spheres leave the two widest models
    3 to 4 %; tests/test_camera_guides.py checks the share)."""
    return T.moved(golden_camera(W, H), dolly=15.0)


def size_of(name, k=0):
    """The image of a model's case: 64x32 for the equirectangular one (2:1, as its layout), else SIZES[k]."""
    return (64, 32) if name == "equirect" else SIZES[k]


MODEL_CASES = [(name, k) for name in MODELS for k in (0, 1) if (name, k) != ("equirect", 1)]   # (model, index of its size)


def camera_model(name, W, H, **over):
    kind, kw = MODELS[name]
    return g.camera_model(kind, W, H, centre=True, **{**kw, **over})


def move_of(name, move):
    return {k: v * MOVE_SCALE[name] for k, v in T.MOVES[move].items()}


def centre_rays(cam, cm):
    """The rows of pt_camera_rays(PT_CAMF_CENTRE, lens_radius 0) from the float64 model, rounded once: float32 [W * H][8]."""
    m = cr.Model.of(cam, cm)
    m.R = 0.0
    _, px, py = cr.pixel_grid(cm.width, cm.height)
    o, d, _ = m.rays(px.astype(np.float64), py.astype(np.float64))
    rows = np.zeros((len(px), 8), F32)
    rows[:, 0:3], rows[:, 4:7] = o, d
    return rows


# ---------------------------------------------------------------------------------------------------- guide buffers
def guides_from_rays(rays, bvh, spheres, params, shape, materials=None, tri_material=None):
    """The six-tuple gpu_support.compare_guides takes — (albedo, normal, position) float32[H][W][4], id int32[H][W], the triangle t
    and the sphere t of every pixel — for the rays float32[H * W][8]; shape = (H, W).  Reads cull_backfaces and tri_col of params."""
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 8)
    n = len(rays)
    o, d = rays[:, 0:3].copy(), rays[:, 4:7].copy()
    has = np.any(d != 0, axis=1)
    t_tri, tri, nrm = np.full(n, FLT_MAX, F32), np.full(n, -1, np.int32), np.zeros((n, 3), F32)
    if has.any():
        t_tri[has], tri[has], nrm[has], _ = orc.trace_bvh(bvh, rays[has], cull=bool(params.cull_backfaces))
    t = t_tri.copy()
    sph = np.full(n, -1, np.int32)
    t_sph = np.full(n, np.inf, F32)   # the nearest sphere regardless of the triangle
    with np.errstate(all="ignore"):
        for i, s in enumerate(spheres or []):
            ts = np.where(has, sphere_intersect(s, o, d), F32(0))
            m = (ts != 0) & (ts < t) & (ts > F32(0.01))
            t[m], sph[m] = ts[m], i
            near = (ts > F32(0.01)) & (ts < t_sph)
            t_sph[near] = ts[near]
        hit_s, hit_t = sph >= 0, (sph < 0) & (tri >= 0)
        hitpos = fma(d, t[:, None], o)
    nn = np.zeros((n, 3), F32)
    if hit_t.any():
        nn[hit_t] = vnormalize(nrm[hit_t])
    if hit_s.any():
        cen = np.array([spheres[i].pos_rad[0:3] for i in range(len(spheres))], F32)
        nn[hit_s] = vnormalize((hitpos[hit_s] - cen[sph[hit_s]]).astype(F32))
    hit = hit_s | hit_t
    flip = hit & ~(vdot(nn, d) < 0)
    nn[flip] = -nn[flip]
    col = np.zeros((n, 3), F32)
    if hit_t.any():
        if materials is not None:
            tab = np.array([list(m.col) for m in materials], F32)
            col[hit_t] = tab[np.asarray(tri_material, np.int64)[tri[hit_t]]]
        else:
            col[hit_t] = np.array(list(params.tri_col), F32)
    if hit_s.any():
        scol = np.array([list(s.col) for s in spheres], F32)
        col[hit_s] = scol[sph[hit_s]]
    albedo, normal, position = (np.zeros((n, 4), F32) for _ in range(3))
    albedo[hit, 0:3] = col[hit]
    normal[hit, 0:3] = nn[hit]
    position[hit, 0:3] = hitpos[hit]
    position[hit, 3] = t[hit]
    ids = np.full(n, -1, np.int32)
    ids[hit_t] = tri[hit_t]
    ids[hit_s] = -2 - sph[hit_s]
    shp = tuple(shape)
    return (albedo.reshape(shp + (4,)), normal.reshape(shp + (4,)), position.reshape(shp + (4,)), ids.reshape(shp),
            t_tri.reshape(shp), t_sph.reshape(shp))


# ---------------------------------------------------------------------------------------------------- the projection
def project(model, points):
    """(fx, fy) float64 of world points [n][3] under a camera_ref.Model: the orthographic ray of a point starts there along front,
    every other model's passes through pos."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    if model.kind == cr.ORTHO:
        return model.pixel_coords(pts, np.tile(model.front, (len(pts), 1)))
    return model.pixel_coords(np.tile(model.pos, (len(pts), 1)), pts - model.pos)


def rejects(model, points):
    """(rejected, fragile) bool[n]: what pt_temporal_camera's projection turns away before the footprint — behind the camera (a <= 0;
    the pinhole, the thin lens, the orthographic model), outside the image circle (theta > fisheye_fov / 2), no direction at all —
    and the points within 1e-5 relative of such a threshold, where a binary32 restatement may decide otherwise."""
    v = np.asarray(points, np.float64).reshape(-1, 3) - model.pos
    a, b, c = v @ model.front, v @ model.right, v @ model.up
    r = np.sqrt(np.sum(v * v, -1))
    if model.kind == cr.FISHEYE:
        s, half = np.hypot(b, c), model.ffov / 2.0
        theta = np.arctan2(s, a)
        return (theta > half) | (r == 0), np.abs(theta - half) <= 1e-5 * half
    if model.kind == cr.EQUIRECT:
        return r == 0, r <= 1e-5 * np.maximum(np.abs(model.pos).max(), 1.0)
    return ~(a > 0), np.abs(a) <= 1e-5 * r


def coord_error(model, fx, fy, rx, ry):
    """Per-axis distance in pixels of device coordinates (fx, fy) from the reference's (rx, ry).  Equirectangular: fx modulo W and
    scaled by cos(latitude) — longitude is not defined at a pole, and a pixel's width on the sphere shrinks with it."""
    dx, dy = np.abs(np.asarray(fx, np.float64) - rx), np.abs(np.asarray(fy, np.float64) - ry)
    if model.kind == cr.EQUIRECT:
        dx = np.minimum(dx, model.W - dx) * np.cos((ry - model.H / 2.0) * (np.pi / model.H))
    return dx, dy


# ---------------------------------------------------------------------------------------------------- steps 3 to 5
def blend_from_coords(W, H, fx, fy, ok, prev_color, prev_length, prev_normal, prev_position, prev_id,
                      cur_color, cur_normal, cur_position, cur_id, max_history, plane_tolerance, normal_threshold, x1=None, n1=None):
    """Steps 3 to 5 of pt_temporal for every pixel: fx, fy float32[H][W] the history coordinates, ok bool[H][W] where the projection
    did not reject; x1, n1 (float32[H][W][3], optional) the point and normal in the previous scene where triangles moved.
    Returns (out float32[H][W][3], length float32[H][W], fragile bool[H][W], accepted bool[H][W])."""
    cur = np.asarray(cur_color, F32)
    prev_color, prev_length = np.asarray(prev_color, F32), np.asarray(prev_length, F32)
    prev_normal, prev_position = np.asarray(prev_normal, F32), np.asarray(prev_position, F32)
    n_p = np.asarray(cur_normal, F32)[..., 0:3] if n1 is None else np.asarray(n1, F32)
    x_p = np.asarray(cur_position, F32)[..., 0:3] if x1 is None else np.asarray(x1, F32)
    t_p = np.asarray(cur_position, F32)[..., 3]
    shp = (H, W)
    hit = np.any(np.asarray(cur_normal, F32)[..., 0:3] != 0, axis=-1)
    fragile = np.zeros(shp, bool)
    with np.errstate(all="ignore"):
        fx, fy = np.asarray(fx, F32), np.asarray(fy, F32)
        ok = np.asarray(ok, bool) & hit & np.isfinite(fx) & np.isfinite(fy)
        fxs, fys = np.where(ok, fx, F32(-8)), np.where(ok, fy, F32(-8))
        fxs, fys = np.clip(fxs, F32(-8), F32(W + 8)), np.clip(fys, F32(-8), F32(H + 8))   # far outside stays outside, and converts
        x0f, y0f = np.floor(fxs), np.floor(fys)
        wx, wy = (fxs - x0f).astype(F32), (fys - y0f).astype(F32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = (F32(plane_tolerance) * t_p).astype(F32)
        sw, sc, sl = np.zeros(shp, np.float64), np.zeros(shp + (3,), np.float64), np.zeros(shp, np.float64)
        for j in (0, 1):
            for i in (0, 1):
                xq, yq = x0 + i, y0 + j
                w = ((wx if i else (F32(1.0) - wx).astype(F32)) * (wy if j else (F32(1.0) - wy).astype(F32))).astype(F32)
                cand = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H) & (w > 0)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                n_q, x_q = prev_normal[yc, xc][..., 0:3], prev_position[yc, xc][..., 0:3]
                cand &= np.any(n_q != 0, axis=-1)
                if prev_id is not None:
                    cand &= np.asarray(prev_id)[yc, xc] == np.asarray(cur_id)
                nd = vdot(n_p, n_q)
                pd = np.abs(vdot(n_p, (x_q - x_p).astype(F32)))
                fragile |= cand & (np.abs(nd.astype(np.float64) - normal_threshold) <= 1e-4)
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
