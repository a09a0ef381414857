"""CPU reference of pt_temporal_motion — TEST INFRASTRUCTURE ONLY (numpy).

where_it_was():     step 2 of the contract of include/ptmi.h (pt_temporal_motion) in float32, in the stated order: for every pixel
                    the point (x', n') its surface point had in the previous frame's scene, or a rejection.
temporal_motion():  the whole call: (x', n') handed to temporal_ref.temporal as the pixel's position and normal, so the
                    projection, every test of a tap, the float64 sums and the FRAGILE conditions are that function's own code,
                    evaluated on (x', n'); the motion restated beside it.
brute_guides():     (normal, position, id) of a small triangle soup in pt_render_aux's layout, every ray against every triangle in
                    double: no tree, two-sided, the nearest hit.
Also the inputs and bars that the CPU tests (test_motion) and the GPU tests (test_gpu_motion) of the feature share.
"""
import numpy as np

import gpu_pathtracer_amd as g
import temporal_ref as T
from denoise_ref import F32, fma, vdot

FLT_MAX = float(np.finfo(np.float32).max)
# The quality sequence: cornell_box, T.QUALITY_FRAMES frames of T.QUALITY_SPP samples from one camera, the two blocks turning
# QUALITY_TURN degrees a frame about the vertical axis through their own centre.  gain = MSE(last frame alone) / MSE(history), both
# against 1024 spp of the last pose.  The numpy references over oracle renders at 80x60 measure these two figures
# (test_motion.test_reference_gains_on_a_moving_mesh asserts them within 2 %); the GPU bar at 320x240 is 0.8 x the motion figure, the
# margin temporal_ref.QUALITY_K uses for the other resolution and sample set.
QUALITY_TURN = 2.0
QUALITY_GAIN_MOTION_CPU = 2.81    # pt_temporal_motion's arithmetic: 2.806 measured, every pixel of the blocks accepted
QUALITY_GAIN_STATIC_CPU = 2.68    # pt_temporal's arithmetic on the same frames: 2.677 measured, 0.957 of the blocks accepted
QUALITY_K_MOTION = 0.8 * QUALITY_GAIN_MOTION_CPU


# ---------------------------------------------------------------------------------------------------- float32 arithmetic
def vcross(a, b):
    """pt_math.h's vcross: fmaf(a.y, b.z, -(a.z * b.y)), ..."""
    def comp(i, j):
        return fma(a[..., i], b[..., j], -(a[..., j] * b[..., i]).astype(F32))
    return np.stack([comp(1, 2), comp(2, 0), comp(0, 1)], -1)


def vmadd(a, s, b):
    return fma(a, s[..., None], b)


# ---------------------------------------------------------------------------------------------------- step 2
def where_it_was(prev_verts, cur_verts, n_tris, cur_normal, cur_position, cur_id):
    """(x' float32[...][3], n' float32[...][3], was bool[...], moved bool[...], fragile bool[...]) for every pixel of the guides.
    was = the history is not rejected in step 2 (a miss counts as `was`: step 1 deals with it); moved = the arithmetic of a
    moved triangle ran."""
    n_p = np.asarray(cur_normal, F32)[..., 0:3]
    x_p = np.asarray(cur_position, F32)[..., 0:3]
    ids = np.asarray(cur_id, np.int64)
    shp = ids.shape
    x1, n1 = x_p.copy(), n_p.copy()
    was = np.ones(shp, bool)
    fragile = np.zeros(shp, bool)
    moved = np.zeros(shp, bool)
    tri = ids >= 0
    was[tri & (ids >= n_tris)] = False
    rows = tri & (ids < n_tris)
    if not rows.any():
        return x1, n1, was, moved, fragile
    pv = np.ascontiguousarray(prev_verts, F32).reshape(-1, 9)
    cv = np.ascontiguousarray(cur_verts, F32).reshape(-1, 9)
    r = ids[rows]
    c, p = cv[r], pv[r]
    same = np.all(c.view(np.uint32) == p.view(np.uint32), axis=-1)   # equal as 32-bit patterns
    m = ~same
    if m.any():
        c, p, xp, npv = c[m], p[m], x_p[rows][m], n_p[rows][m]
        c0, c1, c2, p0, p1, p2 = c[:, 0:3], c[:, 3:6], c[:, 6:9], p[:, 0:3], p[:, 3:6], p[:, 6:9]
        with np.errstate(all="ignore"):
            e1, e2, w = (c1 - c0).astype(F32), (c2 - c0).astype(F32), (xp - c0).astype(F32)
            N = vcross(e1, e2)
            nn = vdot(N, N)
            ok = (nn > 0) & np.isfinite(nn)
            inv = (F32(1.0) / nn).astype(F32)
            u = (vdot(vcross(w, e2), N) * inv).astype(F32)
            v = (vdot(vcross(e1, w), N) * inv).astype(F32)
            ok &= np.isfinite(u) & np.isfinite(v)
            f1, f2 = (p1 - p0).astype(F32), (p2 - p0).astype(F32)
            xq = vmadd(f2, v, vmadd(f1, u, p0))
            N1 = vcross(f1, f2)
            nn1 = vdot(N1, N1)
            ok &= (nn1 > 0) & np.isfinite(nn1)
            k = (np.where(vdot(npv, N) < 0, F32(-1.0), F32(1.0)) * (F32(1.0) / np.sqrt(nn1)).astype(F32)).astype(F32)
            nq = (N1 * k[..., None]).astype(F32)
            # nn or nn' within a relative 1e-5 of the zero decision (against the squared edge lengths, in double) or of the
            # not-finite one (against the largest binary32): another rounding could decide otherwise
            frag = np.zeros(len(c), bool)
            for a1, a2, s in ((e1, e2, nn), (f1, f2, nn1)):
                d1, d2 = a1.astype(np.float64), a2.astype(np.float64)
                exact = np.sum(np.cross(d1, d2) ** 2, -1)
                scale = np.sum(d1 ** 2, -1) * np.sum(d2 ** 2, -1)
                frag |= ~np.isfinite(exact) | (exact <= 1e-5 * scale) | (exact >= (1.0 - 1e-5) * FLT_MAX)
                frag |= np.isfinite(s) & (s.astype(np.float64) >= (1.0 - 1e-5) * FLT_MAX)
            for s in (u, v):
                frag |= np.isfinite(s) & (np.abs(s.astype(np.float64)) >= (1.0 - 1e-5) * FLT_MAX)
        sel = np.zeros(int(rows.sum()), bool)
        sel[m] = True
        full = np.zeros(shp, bool)
        full[rows] = sel
        x1[full], n1[full] = xq, nq
        was[full] = ok
        fragile[full] = frag
        moved = full
    return x1, n1, was, moved, fragile


# ---------------------------------------------------------------------------------------------------- the call
def temporal_motion(W, H, prev_cam, prev_verts, cur_verts, n_tris, prev_color, prev_length, prev_normal, prev_position, prev_id,
                    cur_color, cur_normal, cur_position, cur_id, max_history, plane_tolerance, normal_threshold):
    """pt_temporal_motion's arithmetic over whole frames.  prev_color None = no history (the vertex arrays are not looked at).
    Returns (out float32[H][W][3], length float32[H][W], motion float32[H][W][2], fragile bool[H][W], accepted bool[H][W])."""
    cur_color = np.asarray(cur_color, F32)
    motion = np.zeros((H, W, 2), F32)
    if prev_color is None:
        out, length, fragile, accepted = T.temporal(W, H, None, None, None, None, None, None, cur_color, cur_normal, cur_position, cur_id,
                                                    max_history, plane_tolerance, normal_threshold)
        return out, length, motion, fragile, accepted
    assert prev_id is not None and cur_id is not None
    x1, n1, was, _, frag2 = where_it_was(prev_verts, cur_verts, n_tris, cur_normal, cur_position, cur_id)
    hit = np.any(np.asarray(cur_normal, F32)[..., 0:3] != 0, axis=-1)
    nrm = np.zeros((H, W, 4), F32)
    pos = np.zeros((H, W, 4), F32)
    go = hit & was
    nrm[go, 0:3] = n1[go]     # a pixel rejected in step 2 goes in as a miss: out = cur, length 1 (n' itself is a unit normal, never all zero)
    pos[..., 0:3] = x1
    pos[..., 3] = np.asarray(cur_position, F32)[..., 3]
    out, length, fragile, accepted = T.temporal(W, H, prev_cam, prev_color, prev_length, prev_normal, prev_position, prev_id,
                                                cur_color, nrm, pos, cur_id, max_history, plane_tolerance, normal_threshold)
    fragile = (fragile | frag2) & hit

    def vec(a):
        return np.array(list(a), F32)

    with np.errstate(all="ignore"):   # pt_temporal's step 2 once more, for the motion: the same operations as T.temporal's
        v = (x1 - vec(prev_cam.pos)).astype(F32)
        a, b, c = vdot(v, vec(prev_cam.front)), vdot(v, vec(prev_cam.right)), vdot(v, vec(prev_cam.up))
        sx = F32(F32(W - 1) / F32(F32(prev_cam.aspect) * F32(prev_cam.fov)))
        sy = F32(F32(H - 1) / F32(prev_cam.fov))
        cx, cy = F32(F32(W) / F32(2.0) - F32(0.5)), F32(F32(H) / F32(2.0) - F32(0.5))
        fx, fy = fma((b / a).astype(F32), sx, cx), fma((c / a).astype(F32), sy, cy)
        ok = go & (a > 0) & np.isfinite(fx) & np.isfinite(fy)
        ys, xs = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
        motion[..., 0] = np.where(ok, (fx - xs).astype(F32), F32(0))
        motion[..., 1] = np.where(ok, (fy - ys).astype(F32), F32(0))
    return out, length, motion, fragile, accepted


# ---------------------------------------------------------------------------------------------------- brute-force guides
def camera_rays(cam, W, H):
    """pt_camera_ray through the pixel centres, in double: (origins on the image plane, unit directions), float64[H][W][3]."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx = (xs - W / 2.0 + 0.5) * cam.dist * cam.aspect * cam.fov / (W - 1)
    sy = (ys - H / 2.0 + 0.5) * cam.dist * cam.fov / (H - 1)
    f, r, u, pos = (np.array(list(v), np.float64) for v in (cam.front, cam.right, cam.up, cam.pos))
    d0 = f * cam.dist + sx[..., None] * r + sy[..., None] * u
    return pos + d0, d0 / np.linalg.norm(d0, axis=-1, keepdims=True)


def brute_guides(soup, cam, W, H):
    """(normal, position, id) of the triangle soup float[n][9] seen through the pixel centres of `cam`, in pt_render_aux's
    layout: the unit normal on the side the ray comes from, the hit point with t in .w, the row of the triangle; a miss is all
    zero with id -1.  No tree: every triangle (Moller-Trumbore in double, two-sided) against every pixel inside the box of its
    three projected vertices, widened by a pixel — the whole frame for a triangle that reaches behind the camera point; the
    nearest hit wins, the lower row on a tie; rounded once."""
    o, d = camera_rays(cam, W, H)
    f, r, u, pos = (np.array(list(v), np.float64) for v in (cam.front, cam.right, cam.up, cam.pos))
    tri = np.asarray(soup, np.float64).reshape(-1, 3, 3)
    best_t = np.full((H, W), np.inf)
    best_i = np.full((H, W), -1, np.int64)
    sx, sy = (W - 1) / (cam.aspect * cam.fov), (H - 1) / cam.fov
    with np.errstate(all="ignore"):
        for k, (v0, v1, v2) in enumerate(tri):
            if not np.all(np.isfinite(tri[k])):
                continue
            rel = tri[k] - pos
            a = rel @ f
            xa, xb, ya, yb = 0, W - 1, 0, H - 1
            if np.all(a > 1e-9):
                px, py = (rel @ r) / a * sx + W / 2.0 - 0.5, (rel @ u) / a * sy + H / 2.0 - 0.5
                xa, xb = max(0, int(np.floor(px.min())) - 1), min(W - 1, int(np.ceil(px.max())) + 1)
                ya, yb = max(0, int(np.floor(py.min())) - 1), min(H - 1, int(np.ceil(py.max())) + 1)
                if xa > xb or ya > yb:
                    continue
            oo, dd = o[ya:yb + 1, xa:xb + 1], d[ya:yb + 1, xa:xb + 1]
            e1, e2 = v1 - v0, v2 - v0
            pvec = np.cross(dd, e2)
            det = pvec @ e1
            tvec = oo - v0
            uu = np.sum(tvec * pvec, -1) / det
            qvec = np.cross(tvec, e1)
            vv = np.sum(dd * qvec, -1) / det
            t = (qvec @ e2) / det
            ok = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 1e-9) & np.isfinite(t)
            bt, bi = best_t[ya:yb + 1, xa:xb + 1], best_i[ya:yb + 1, xa:xb + 1]
            better = ok & (t < bt)
            bt[better], bi[better] = t[better], k
    hit = best_i >= 0
    normal, position = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    ti = tri[best_i[hit]]
    n = np.cross(ti[:, 1] - ti[:, 0], ti[:, 2] - ti[:, 0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[np.sum(n * d[hit], -1) > 0] *= -1.0
    normal[hit, 0:3] = n
    position[hit, 0:3] = o[hit] + best_t[hit, None] * d[hit]
    position[hit, 3] = best_t[hit]
    return normal, position, np.where(hit, best_i, -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- the quality sequence
BLOCK_MATERIALS = (5, 6)   # cornell_box's material rows of the short and of the tall block (twelve triangles each)


def block_rows(mesh):
    """The triangles of cornell_box's two blocks, picked by material row: one index array per block."""
    tm = np.asarray(mesh.tri_material, np.int64)
    return [np.nonzero(tm == m)[0] for m in BLOCK_MATERIALS]


def quality_pose(soup, blocks, k):
    """The soup of frame k: every block turned k x QUALITY_TURN degrees about the vertical axis through its own centre, each
    frame from the rest pose (no drift)."""
    from gpu_support import turn_rows
    out = soup
    if k:
        for rows in blocks:
            out = turn_rows(out, rows, QUALITY_TURN * k, (0.0, 0.0, 0.0))
    return out


# ---------------------------------------------------------------------------------------------------- the GPU comparison's cases
# (mesh, W, H): a mesh built by pt_build_bvh from its soup, seen at rest (the history) and after pt_refit_bvh of its move (the
# current frame).  The moves keep more than half of the moved triangles' pixels their history in the numpy reference alone at
# 37x23 and 257x131 (test_gpu_motion asserts it case by case); bunny_low's triangles are smaller than a pixel at 37x23, where few
# taps share the pixel's id, so it runs at 257x131 only.
CASES = [("cube", 2, 2), ("needles", 7, 5), ("cube", 37, 23), ("needles", 37, 23), ("cube", 257, 131), ("needles", 257, 131),
         ("bunny_low", 257, 131)]
CAMERA_MOVES = {"static": {}, "pan": dict(pan_deg=2.0)}


def case_soups(name):
    """(rest soup, moved soup) of a case's mesh: the cube turns rigidly and shifts (gpu_support.turn_rows), the others twist
    (gpu_support.twist)."""
    from gpu_support import builder_mesh, turn_rows, twist
    soup = np.array(builder_mesh(name)[3])
    if name == "cube":
        return soup, turn_rows(soup, np.arange(len(soup)), 9.0, (0.6, -0.4, 0.5))
    return soup, twist(soup, 0.35 if name == "bunny_low" else 0.25, (0.01, 0.0, 0.005))


def case_camera(name, soup, W, H):
    """A camera that frames the case's mesh from above its front right (of needles: its patch of small triangles, the first 512
    rows, so that those are a few pixels each), built in double and stored as float32; below 37 pixels across it looks at the
    middle of that view through a field narrowed in proportion (needles: below 74, its patch triangles being small)."""
    from scene_matrix import make_camera
    v = np.asarray(soup[:512] if name == "needles" else soup, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    pos = c + ext * np.array([0.35, 0.45, 1.7])
    return make_camera(W, H, pos=pos, front=c - pos, fov=0.8 * min(1.0, W / (74.0 if name == "needles" else 37.0)), dist=1.0)
