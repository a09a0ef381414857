"""The image-stage calls pinned bit for bit: every output buffer of pt_render_aux, pt_denoise, pt_denoise_variance, pt_temporal,
pt_temporal_motion, pt_temporal_moments, pt_frame_error, pt_select_pixels, pt_tonemap and pt_meter (pt_tonemap_thresholds through
the tables pt_tonemap uploads and as a digest of its own) as the SHA-256 of its raw bytes, the figures that return to the host as
exact hex floats or ints.  The suites of these calls compare against float64 references with a tolerance; a last-bit change of a
kernel passes them and fails here.  tests/test_gpu_image_pins.py holds the library to tests/golden/image_stage_digests.json, which

    python tests/image_pins.py --record

wrote on an MI355X before the image stages were split into one translation unit each.  A plain module found through tests/ on
sys.path, like scene_matrix; importing it needs no GPU, digests() does.

Inputs come from fixed numpy seeds and are finite: colours in [0, 2), some miss pixels (zero normal), some albedo channels below
1e-3, lengths between 1 and 8.  The filters run on made-up guides, the reprojections on pt_render_aux's own of assets/cube.ptmesh in
the sphere room (a history only survives guides that agree with its camera).  37 x 23 is odd, no multiple of the 16-pixel tile or
of four pixels, and its far taps fall off the image; 48 x 32 is whole tiles and takes the four-pixel routes; 300 x 220 = 66 000
pixels are 258 blocks of 256, so the selection's scan runs a second round with a carry and the meter's 256 blocks stride.  Every
output buffer starts as 0xCD bytes, so what a call leaves unwritten is pinned as well."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "image_stage_digests.json")
PIXEL_SIZES = [(37, 23), (48, 32)]
BLOCK_SIZE = (300, 220)
F = np.float32
CALLS = ["pt_render_aux", "pt_denoise", "pt_denoise_variance", "pt_temporal", "pt_temporal_motion", "pt_temporal_moments",
         "pt_frame_error", "pt_select_pixels", "pt_tonemap_thresholds", "pt_tonemap", "pt_meter"]


class Dev:
    """The device buffers of a group of cases, freed together."""

    def __init__(self, t):
        self.t, self.bufs = t, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        b = self.t.malloc(a.nbytes)
        b.upload(a)
        self.bufs.append(b)
        return b

    def out(self, nbytes):
        return self.up(np.full(nbytes, 0xCD, np.uint8))

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def sha(t, buf):
    t.sync()
    return hashlib.sha256(buf.download(np.uint8, (buf.nbytes,)).tobytes()).hexdigest()


def ptr(b):
    return b.ptr if b is not None else None


# ---------------------------------------------------------------------------------------------------- inputs
def made_up_guides(W, H, seed):
    """(albedo, normal, position) float32 [H][W][4]: normals of three directions in patches, a tenth of the pixels and one block
    misses; positions on a rough plane, t in [1, 8]; a tenth of the albedo channels at 5e-4 or 0."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    dirs = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0.8, 0.6]], F)
    nrm = np.zeros((H, W, 4), F)
    nrm[..., :3] = dirs[((x // 7) + (y // 5)) % 3]
    miss = r.random((H, W)) < 0.1
    miss[H // 3:H // 3 + 4, W // 2:W // 2 + 6] = True
    nrm[miss] = 0
    pos = np.zeros((H, W, 4), F)
    pos[..., 0], pos[..., 1] = x * 0.1, y * 0.1
    pos[..., 2] = r.random((H, W)) * 0.05
    pos[..., 3] = 1.0 + 7.0 * r.random((H, W))
    pos[miss] = 0
    alb = np.zeros((H, W, 4), F)
    alb[..., :3] = r.random((H, W, 3))
    low = r.random((H, W, 3))
    alb[..., :3][low < 0.05] = 5e-4
    alb[..., :3][low > 0.95] = 0
    alb[miss] = 0
    return alb, nrm, pos


def colour(W, H, seed):
    return (2.0 * np.random.default_rng(seed).random((H, W, 3))).astype(F)


def moments(W, H, seed):
    """(m1, m2) of a luminance with a spread of its own per pixel: m2 >= m1^2 but for a few pixels (the variance clamps at 0)."""
    r = np.random.default_rng(seed)
    m1 = r.random((H, W)) * 1.5
    m2 = m1 * m1 + r.random((H, W)) ** 4
    m2[r.random((H, W)) < 0.03] *= 0.9
    return np.stack([m1, m2], -1).astype(F)


def lengths(W, H, seed):
    return (1.0 + 7.0 * np.random.default_rng(seed).random((H, W))).astype(F)


def hdr(W, H, seed):
    """2^-8 .. 2^8 in every channel, a few zeros and negatives."""
    r = np.random.default_rng(seed)
    img = np.exp2(r.uniform(-8, 8, (H, W, 3)))
    k = r.random((H, W, 3))
    img[k < 0.02] = 0
    img[k > 0.98] *= -1
    return img.astype(F)


# ---------------------------------------------------------------------------------------------------- the cases
def aux_cases(t, g, res):
    """pt_render_aux, and what the reprojections below read: per size (camera, panned camera, the guides at both, the vertex
    rows)."""
    from scene_matrix import make_camera
    mesh = g.scene_mesh("cube")
    rows = np.asarray(mesh.verts, F)[np.asarray(mesh.tris)].reshape(-1, 9)
    t.upload_tri_materials(None, None)
    t.upload_bvh(g.Bvh(mesh))
    t.upload_spheres(g.reference_spheres())
    pos = np.array([3.0, 4.0, 30.0])
    front = np.array([0.0, 0.0, -5.0]) - pos
    front /= np.linalg.norm(front)
    right = np.cross(front, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    scenes = {}
    for W, H in PIXEL_SIZES:
        cams = [make_camera(W, H, pos, front), make_camera(W, H, pos, front + 0.04 * right + 0.01 * np.cross(right, front))]
        p = g.default_params(W, H)
        d = Dev(t)
        got = []
        for k, cam in enumerate(cams):
            for with_ids in (True, False):
                a, n, x, i = d.out(W * H * 16), d.out(W * H * 16), d.out(W * H * 16), d.out(W * H * 4)
                t.render_aux(cam, p, a.ptr, n.ptr, x.ptr, i.ptr if with_ids else None)
                res[f"pt_render_aux/{W}x{H}/cam{k}/{'ids' if with_ids else 'no-ids'}"] = {
                    "albedo": sha(t, a), "normal": sha(t, n), "position": sha(t, x), "id": sha(t, i)}
                if with_ids:
                    got.append((n.download(F, (H, W, 4)), x.download(F, (H, W, 4)), i.download(np.int32, (H, W))))
        d.free()
        scenes[(W, H)] = (cams, got, rows)
    return scenes


def denoise_cases(t, g, res):
    for W, H in PIXEL_SIZES:
        d = Dev(t)
        alb, nrm, pos = (d.up(a) for a in made_up_guides(W, H, 11))
        col = colour(W, H, 12)
        dc = d.up(col)
        sig = dict(sigma_color=1.0, sigma_normal=0.5, sigma_position=0.5)
        for it in (0, 1, 3, 5):
            for words in (True, False):
                out, rgba = d.out(col.nbytes), d.out(W * H * 4)
                t.denoise(dc.ptr, alb.ptr, nrm.ptr, pos.ptr, W, H, out.ptr, rgba.ptr if words else None, iterations=it, **sig)
                res[f"pt_denoise/{W}x{H}/it{it}/{'words' if words else 'no-words'}"] = {"out": sha(t, out), "rgba": sha(t, rgba)}
        alias, rgba = d.up(col), d.out(W * H * 4)
        t.denoise(alias.ptr, alb.ptr, nrm.ptr, pos.ptr, W, H, alias.ptr, rgba.ptr, iterations=3, **sig)
        res[f"pt_denoise/{W}x{H}/it3/out-is-color"] = {"out": sha(t, alias), "rgba": sha(t, rgba)}
        d.free()


def denoise_variance_cases(t, g, res):
    for W, H in PIXEL_SIZES:
        d = Dev(t)
        alb, nrm, pos = (d.up(a) for a in made_up_guides(W, H, 21))
        col = colour(W, H, 22)
        dc, dm, dl = d.up(col), d.up(moments(W, H, 23)), d.up(lengths(W, H, 24))

        def run(name, it, with_len, with_var, **kw):
            out, var, rgba = d.out(col.nbytes), d.out(W * H * 4), d.out(W * H * 4)
            t.denoise_variance(dc.ptr, dm.ptr, dl.ptr if with_len else None, alb.ptr, nrm.ptr, pos.ptr, W, H, out.ptr,
                               var.ptr if with_var else None, rgba.ptr, samples_per_frame=4.0, iterations=it, **kw)
            res[name] = {"out": sha(t, out), "variance": sha(t, var), "rgba": sha(t, rgba)}

        sig = dict(sigma_luminance=2.0, sigma_normal=0.5, sigma_position=0.5)
        for it in (0, 1, 3, 5):
            for with_len in (True, False):
                for with_var in (True, False):
                    run(f"pt_denoise_variance/{W}x{H}/it{it}/{'len' if with_len else 'no-len'}/{'var' if with_var else 'no-var'}",
                        it, with_len, with_var, **sig)
        run(f"pt_denoise_variance/{W}x{H}/it3/sigma-luminance-0", 3, True, True, **dict(sig, sigma_luminance=0.0))
        d.free()


def with_misses(normal, seed):
    """A copy of pt_render_aux's normals with a twentieth of the pixels turned into misses."""
    n = normal.copy()
    n[np.random.default_rng(seed).random(n.shape[:2]) < 0.05] = 0
    return n


def temporal_cases(t, g, res, scenes):
    """pt_temporal, pt_temporal_motion and pt_temporal_moments over the same frames: the current one at cam0, the history at cam0
    (the projection is the identity) or at the panned cam1."""
    for W, H in PIXEL_SIZES:
        cams, guides, rows = scenes[(W, H)]
        d = Dev(t)
        cn, cx, ci = d.up(with_misses(guides[0][0], 31)), d.up(guides[0][1]), d.up(guides[0][2])
        prev = [(d.up(with_misses(n, 32 + k)), d.up(x), d.up(i)) for k, (n, x, i) in enumerate(guides)]
        ccol, pcol = d.up(colour(W, H, 34)), d.up(colour(W, H, 35))
        cmom, pmom = d.up(moments(W, H, 36)), d.up(moments(W, H, 37))
        plen = d.up(lengths(W, H, 38))
        moved = rows.copy()
        moved[[1, 4, 5, 9]] += np.array([0.3, -0.2, 0.1] * 3, F)   # the history's rows: four triangles stood elsewhere
        cur_rows, prev_rows = d.up(rows), d.up(moved)
        n_tris = len(rows)

        def colour_call(name, fn, k, ids, verts=None, motion=None, history=True):
            pn, px, pi = prev[k]
            out, ln, rgba, mo = d.out(W * H * 12), d.out(W * H * 4), d.out(W * H * 4), d.out(W * H * 8)
            head = (W, H, cams[k] if history else None) + (() if verts is None else (ptr(verts[0]), ptr(verts[1]), n_tris if history else 0))
            hist = (pcol.ptr, plen.ptr, pn.ptr, px.ptr, pi.ptr if ids else None) if history else (None,) * 5
            tail = (ccol.ptr, cn.ptr, cx.ptr, ci.ptr if ids else None, out.ptr, ln.ptr, rgba.ptr)
            if verts is None:
                fn(*head, *hist, *tail)
            else:
                fn(*head, *hist, *tail, mo.ptr if motion else None)
            res[name] = {"out": sha(t, out), "length": sha(t, ln), "rgba": sha(t, rgba), "motion": sha(t, mo)}

        tag = f"{W}x{H}"
        colour_call(f"pt_temporal/{tag}/no-history", t.temporal, 0, True, history=False)
        colour_call(f"pt_temporal/{tag}/ids", t.temporal, 0, True)
        colour_call(f"pt_temporal/{tag}/no-ids", t.temporal, 0, False)
        colour_call(f"pt_temporal/{tag}/panned", t.temporal, 1, True)
        none = (None, None)
        colour_call(f"pt_temporal_motion/{tag}/no-history", t.temporal_motion, 0, True, verts=none, history=False)
        colour_call(f"pt_temporal_motion/{tag}/no-history/motion", t.temporal_motion, 0, True, verts=none, motion=True, history=False)
        colour_call(f"pt_temporal_motion/{tag}/same-verts", t.temporal_motion, 1, True, verts=(cur_rows, cur_rows), motion=True)
        colour_call(f"pt_temporal_motion/{tag}/moved", t.temporal_motion, 1, True, verts=(prev_rows, cur_rows))
        colour_call(f"pt_temporal_motion/{tag}/moved/motion", t.temporal_motion, 1, True, verts=(prev_rows, cur_rows), motion=True)

        def moments_call(name, k, ids, verts, history=True):
            pn, px, pi = prev[k]
            out = d.out(W * H * 8)
            hist = (pmom.ptr, plen.ptr, pn.ptr, px.ptr, pi.ptr if ids else None) if history else (None,) * 5
            t.temporal_moments(W, H, cams[k] if history else None, ptr(verts[0]), ptr(verts[1]), n_tris if verts[0] is not None else 0,
                               *hist, cmom.ptr, cn.ptr, cx.ptr, ci.ptr if ids else None, out.ptr)
            res[name] = {"out": sha(t, out)}

        moments_call(f"pt_temporal_moments/{tag}/no-history", 0, True, none, history=False)
        moments_call(f"pt_temporal_moments/{tag}/moved", 1, True, (prev_rows, cur_rows))
        moments_call(f"pt_temporal_moments/{tag}/ids", 1, True, none)
        moments_call(f"pt_temporal_moments/{tag}/no-ids", 1, False, none)
        d.free()


def selection_cases(t, g, res):
    W, H = BLOCK_SIZE
    d = Dev(t)
    dm = d.up(moments(W, H, 41))
    mean, above = t.frame_error(dm.ptr, W, H, 16, 0.1)
    res[f"pt_frame_error/{W}x{H}"] = {"mean_rse": float(mean).hex(), "n_above": int(above)}
    r = np.random.default_rng(42)
    mixed = r.integers(0, 41, (H, W)).astype(np.uint32)
    for name, counts in (("uniform", np.full((H, W), 16, np.uint32)), ("mixed", mixed)):
        dc, px = d.up(counts), d.out(W * H * 4)
        n, mean = t.select_pixels(dm.ptr, dc.ptr, px.ptr, W, H, 0.1, min_samples=4, max_samples=32)
        res[f"pt_select_pixels/{W}x{H}/{name}"] = {"pixels": sha(t, px), "n_selected": int(n), "mean_rse": float(mean).hex()}
    d.free()


def display_cases(t, g, res):
    for name, xfer in (("srgb", g.XFER_SRGB), ("gamma22", g.XFER_GAMMA22)):
        res[f"pt_tonemap_thresholds/{name}"] = {"table": hashlib.sha256(np.ascontiguousarray(g.tone_thresholds(xfer), F).tobytes()).hexdigest()}
    curves = [("clamp", g.TONE_CLAMP, 1.0, np.inf), ("reinhard", g.TONE_REINHARD, 2.5, 4.0), ("aces", g.TONE_ACES, 0.37, np.inf)]
    xfers = [("linear", g.XFER_LINEAR), ("srgb", g.XFER_SRGB), ("gamma22", g.XFER_GAMMA22)]
    for W, H in PIXEL_SIZES:
        d = Dev(t)
        img = hdr(W, H, 51)
        dc, de = d.up(img), d.up(np.array([0.75], F))
        for cn, curve, e, white in curves:
            for xn, xfer in xfers:
                out, rgba = d.out(img.nbytes), d.out(W * H * 4)
                t.tonemap(dc.ptr, W, H, rgba.ptr, out.ptr, curve=curve, transfer=xfer, exposure=e, white=white)
                res[f"pt_tonemap/{W}x{H}/{cn}/{xn}"] = {"out": sha(t, out), "rgba": sha(t, rgba)}
        out, rgba = d.out(img.nbytes), d.out(W * H * 4)
        t.tonemap(dc.ptr, W, H, rgba.ptr, out.ptr, curve=g.TONE_REINHARD, transfer=g.XFER_SRGB, exposure=2.5, white=4.0, exposure_ptr=de.ptr)
        res[f"pt_tonemap/{W}x{H}/reinhard/srgb/exposure-dev"] = {"out": sha(t, out), "rgba": sha(t, rgba)}
        d.free()
    for W, H in PIXEL_SIZES + [BLOCK_SIZE]:
        d = Dev(t)
        dc, st = d.up(hdr(W, H, 52)), d.up(np.zeros(4, F))
        for k, reset in enumerate((True, False)):
            t.meter(dc.ptr, W, H, st.ptr, key=0.18, low_pct=0.1, high_pct=0.9, adapt=0.5, reset=reset)
            res[f"pt_meter/{W}x{H}/call{k}-reset{int(reset)}"] = {"state": sha(t, st)}
        d.free()


def digests():
    """{case: {output: SHA-256 or figure}} of every case, on cuda:0."""
    import gpu_pathtracer_amd as g
    t = g.PathTracer(0)
    res = {}
    try:
        scenes = aux_cases(t, g, res)
        denoise_cases(t, g, res)
        denoise_variance_cases(t, g, res)
        temporal_cases(t, g, res, scenes)
        selection_cases(t, g, res)
        display_cases(t, g, res)
    finally:
        t.close()
    return res


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


if __name__ == "__main__":
    import argparse
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="write the digests (else compare them with the committed ones)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    got = digests()
    if a.record:
        with open(a.out, "w") as fh:
            json.dump(got, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print(f"{len(got)} cases -> {a.out}")
    else:
        with open(a.out) as fh:
            want = json.load(fh)
        bad = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        print(f"{len(got)} cases, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
        sys.exit(1 if bad else 0)
