"""PathTracer — Python mirror of the reference's device-facing surface, over the C ABI.

Reference interface mirrored (same names / argument meaning where one exists):
  BasicScene::launchKernel(const kernelInfo&)   tracer.cu:405-415  → PathTracer.launch_kernel(cam, params, spp)
  cudaMalloc/cudaMemcpy of the CudaBVH arrays  BasicScene.cpp:297-306 → PathTracer.upload_bvh(bvh)
  cudaMalloc/cudaMemcpy of the sphere array     BasicScene.cpp:214-215 → PathTracer.upload_spheres(spheres)
  accumBuffer / dev_drawRes allocation          BasicScene.cpp:138-149 → PathTracer.alloc_frame(w, h)
Errors: the reference prints and exit(1)s (utilfun.hpp:81-90); here every failure raises
PtError carrying pt_last_error().  There is no CPU fallback of any kind.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import Camera, CameraModel, Counters, DenoiseParams, DenoiseVarianceParams, Environment, Material, MeterParams, Params, SelectParams, Sphere, TemporalParams, TonemapParams

# pt_denoise defaults (iterations, sigma_color, sigma_normal, sigma_position): chosen by the CPU sweep of DESIGN.md §10 f6;
# host/pt_app.cpp uses the same values
DENOISE_DEFAULTS = dict(iterations=4, sigma_color=0.0, sigma_normal=1.0, sigma_position=0.03)
# pt_denoise_variance defaults: the geometry stops of DENOISE_DEFAULTS and SVGF's luminance stop of 4 standard errors (DESIGN.md §10
# f15); host/pt_app.cpp uses the same values
DENOISE_VARIANCE_DEFAULTS = dict(iterations=4, sigma_luminance=4.0, sigma_normal=1.0, sigma_position=0.03)
# pt_temporal defaults: starting values by definition, not tuned figures; host/pt_app.cpp uses the same values
TEMPORAL_DEFAULTS = dict(max_history=32.0, plane_tolerance=0.02, normal_threshold=0.9)


def tone_thresholds(transfer):
    """The 256 thresholds T of tonemap()'s transfer XFER_SRGB or XFER_GAMMA22 (pt_tonemap_thresholds; host only): the display code of
    a curve output y is the number of k in 1..255 with y >= T[k]."""
    out = np.empty(256, np.float32)
    lib = _abi.ptmi()
    rc = lib.pt_tonemap_thresholds(int(transfer), out.ctypes.data)
    if rc != 0:
        raise PtError(rc, lib.pt_last_error(None).decode())
    return out


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptmi error {code}: {msg}")
        self.code = code


class DeviceBuffer:
    """A raw device allocation owned by a PathTracer (pt_malloc / pt_free)."""

    def __init__(self, owner, nbytes):
        self.owner, self.nbytes = owner, nbytes
        p = C.c_void_p()
        owner._check(owner._lib.pt_malloc(owner._ctx, nbytes, C.byref(p)))
        self.ptr = p.value

    def zero(self):
        self.owner._check(self.owner._lib.pt_memset(self.owner._ctx, self.ptr, 0, self.nbytes))

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.owner._check(self.owner._lib.pt_download(self.owner._ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        self.owner._check(self.owner._lib.pt_upload(self.owner._ctx, self.ptr, a.ctypes.data, a.nbytes))

    def free(self):
        if self.ptr:
            self.owner._lib.pt_free(self.owner._ctx, self.ptr)
            self.ptr = None


class PathTracer:
    def __init__(self, device=0):
        self._lib = _abi.ptmi()
        ctx = C.c_void_p()
        rc = self._lib.pt_create(device, C.byref(ctx))
        if rc != 0:
            raise PtError(rc, self._lib.pt_last_error(None).decode())
        self._ctx = ctx
        self.device = device

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise PtError(rc, self._lib.pt_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            if getattr(self, "_refit_buf", None) is not None:
                self._refit_buf.free()
                self._refit_buf = None
            self._lib.pt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.pt_set_stream(self._ctx, hip_stream_ptr))

    def set_option(self, opt, value):
        self._check(self._lib.pt_set_option(self._ctx, opt, int(value)))

    def sync(self):
        self._check(self._lib.pt_sync(self._ctx))

    def malloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # ------------------------------------------------------------------ scene
    def upload_bvh(self, bvh):
        n, t, i = (np.ascontiguousarray(bvh.nodes, np.float32), np.ascontiguousarray(bvh.tris, np.float32),
                   np.ascontiguousarray(bvh.index, np.int32))
        self._check(self._lib.pt_upload_bvh(self._ctx, n.ctypes.data, n.size // 4, t.ctypes.data, t.size // 4,
                                            i.ctypes.data, i.size))

    def upload_bvh_arrays(self, nodes, n_node_vec4, tris, n_tri_vec4, index, n_index):
        self._check(self._lib.pt_upload_bvh(self._ctx, nodes, n_node_vec4, tris, n_tri_vec4, index, n_index))

    def upload_spheres(self, spheres):
        n = len(spheres) if spheres is not None else 0
        self._check(self._lib.pt_upload_spheres(self._ctx, spheres if n else None, n))

    def build_bvh(self, mesh):
        """Build the BVH on the device from a Mesh (pt_build_bvh; extension).  Returns the device
        build time in ms."""
        v = np.ascontiguousarray(mesh.verts, np.float32)
        t = np.ascontiguousarray(mesh.tris, np.int32)
        self._check(self._lib.pt_build_bvh(self._ctx, v.ctypes.data, len(v), t.ctypes.data, len(t)))
        ms = C.c_float()
        self._check(self._lib.pt_last_build_ms(self._ctx, C.byref(ms)))
        return ms.value

    def refit_bvh(self, tri_verts, n_tris=None, n_dropped=None):
        """Move the triangles of the tree on the context (pt_refit_bvh; extension): the hierarchy keeps its topology, every
        box is refit on the device.  tri_verts: float32 rows v0, v1, v2 by original triangle id, as a DeviceBuffer or a raw
        device pointer (n_tris rows; a DeviceBuffer's size gives it when omitted), or a host numpy array of shape (n, 9) or
        (n, 3, 3), staged through a device buffer the tracer owns.  n_dropped: a DeviceBuffer or device pointer that
        receives the uint32 count of dropped (non-finite) triangles.  Asynchronous like launch_kernel."""
        if isinstance(tri_verts, np.ndarray):
            a = np.ascontiguousarray(tri_verts)
            if a.dtype != np.float32 or a.ndim not in (2, 3) or a.shape[1:] not in ((9,), (3, 3)):
                raise ValueError("refit_bvh: a float32 array of shape (n, 9) or (n, 3, 3) expected")
            if getattr(self, "_refit_buf", None) is None or self._refit_buf.nbytes < a.nbytes:
                if getattr(self, "_refit_buf", None) is not None:
                    self._refit_buf.free()
                self._refit_buf = DeviceBuffer(self, max(a.nbytes, 36))
            self._refit_buf.upload(a)
            ptr, n = self._refit_buf.ptr, len(a)
        elif isinstance(tri_verts, DeviceBuffer):
            ptr, n = tri_verts.ptr, tri_verts.nbytes // 36 if n_tris is None else n_tris
        else:
            if n_tris is None:
                raise ValueError("refit_bvh: a raw device pointer needs n_tris")
            ptr, n = tri_verts, n_tris
        nd = n_dropped.ptr if isinstance(n_dropped, DeviceBuffer) else n_dropped
        self._check(self._lib.pt_refit_bvh(self._ctx, ptr, int(n), nd))

    def upload_tri_materials(self, table, tri_material):
        """Per-triangle materials (extension): `table` = sequence of Material, `tri_material` =
        int32 row per ORIGINAL triangle id.  table=None clears (one global material again)."""
        if table is None or len(table) == 0:
            self._check(self._lib.pt_upload_tri_materials(self._ctx, None, 0, None, 0))
            return
        arr = (Material * len(table))(*table)
        ids = np.ascontiguousarray(tri_material, np.int32)
        self._check(self._lib.pt_upload_tri_materials(self._ctx, arr, len(table), ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids)))

    def scene_info(self):
        a, b, c_, e = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        d = C.c_uint32()
        self._check(self._lib.pt_scene_info(self._ctx, C.byref(a), C.byref(b), C.byref(c_), C.byref(d), C.byref(e)))
        return {"n_inner": a.value, "n_tri_refs": b.value, "n_leaves": c_.value, "max_depth": d.value,
                "device_bytes": e.value}

    # ------------------------------------------------------------------ hot path
    def alloc_frame(self, width, height):
        """accumBuffer (vec3[W*H], zeroed) and dev_drawRes (uint[W*H]), BasicScene.cpp:138-149."""
        acc = self.malloc(width * height * 12)
        acc.zero()
        rgba = self.malloc(width * height * 4)
        rgba.zero()
        return acc, rgba

    def launch_kernel(self, accum_ptr, rgba_ptr, cam, params, spp=1, moments_ptr=None):
        """render(accum, bvh, camera, spp): asynchronous until sync().  moments_ptr: float[H][W][2] device memory that also
        receives the running (m1, m2) of the samples' luminance (pt_render_moments).  params.flags with FLAG_NEE (needs
        FLAG_COSINE_DIFF): a shadow ray per diffuse hit towards one of the lights; with FLAG_MIS as well (needs FLAG_NEE) the shadow
        ray and the bounce ray are weighed against each other by the balance heuristic — the megakernel renders such a call whatever
        OPT_KERNEL says, and it is refused over Woop records."""
        if moments_ptr is None:
            self._check(self._lib.pt_render(self._ctx, accum_ptr, rgba_ptr, C.byref(cam), C.byref(params), spp))
        else:
            self._check(self._lib.pt_render_moments(self._ctx, accum_ptr, rgba_ptr, moments_ptr, C.byref(cam), C.byref(params), spp))

    def frame_error(self, moments_ptr, width, height, n_samples, threshold=0.0):
        """(mean relative standard error of the pixels' mean luminance, pixels whose own exceeds `threshold`) from the moments
        of n_samples samples per pixel (pt_frame_error).  Synchronises."""
        mean, above = C.c_double(), C.c_uint64()
        self._check(self._lib.pt_frame_error(self._ctx, moments_ptr, int(width), int(height), int(n_samples), float(threshold),
                                             C.byref(mean), C.byref(above)))
        return mean.value, above.value

    def trace_rays(self, rays_ptr, n, cull, t_ptr, tri_ptr, normal_ptr=None):
        self._check(self._lib.pt_trace_rays(self._ctx, rays_ptr, n, int(cull), t_ptr, tri_ptr, normal_ptr))

    def closest_hits(self, rays_ptr, n, cull, t_ptr, tri_ptr, normal_ptr=None):
        """The nearest triangle inside (0, t_max) of every ray (pt_closest_hits): rays float[n][8] = (o, ignored, d, t_max);
        t float[n] (FLT_MAX on a miss), the original id int32[n] (-1), the un-normalised normal float[n][3] (optional).
        Asynchronous until sync()."""
        self._check(self._lib.pt_closest_hits(self._ctx, rays_ptr, n, int(cull), t_ptr, tri_ptr, normal_ptr))

    def any_hits(self, rays_ptr, n, cull, hit_ptr):
        """Whether any triangle lies inside (0, t_max) of every ray (pt_any_hits): one byte per ray, 1 or 0 — a torch.bool
        tensor's data_ptr() will do.  Asynchronous until sync()."""
        self._check(self._lib.pt_any_hits(self._ctx, rays_ptr, n, int(cull), hit_ptr))

    def render_rays(self, rays_ptr, n, out_ptr, params, spp=1, first_index=0, hdr=False):
        """Path-trace a caller's rays (pt_render_rays): rays float[n][8] = (o, ignored, d, ignored) with unit d; out float[n][3], the
        running mean of the radiance per ray, N = params.sample_index ..; ray i draws the random numbers of pixel first_index + i.
        hdr: the mean is not clamped to 0..1.  FLAG_NEE and FLAG_MIS in params.flags as in launch_kernel.  Asynchronous until sync()."""
        self._check(self._lib.pt_render_rays(self._ctx, rays_ptr, int(n), int(first_index), out_ptr, C.byref(params), int(spp),
                                             _abi.RAYS_HDR if hdr else _abi.RAYS_CLAMPED))

    def camera_rays(self, cam, model, frame, rays_ptr, n=None, first_pixel=0, pixels_ptr=None):
        """The jittered rays of frame `frame` under a camera model (pt_camera_rays; model: host.camera_model) into rays float[n][8],
        the layout render_rays reads: row i is pixel first_pixel + i, or pixels_ptr[i] (uint32 on the device; n is then required,
        and an index past the image gives a ray without direction, which renders as a miss).  n defaults to the pixels from
        first_pixel to the end of the image.  Asynchronous on the context's stream: a render_rays issued next reads these rays."""
        if n is None:
            if pixels_ptr is not None:
                raise ValueError("camera_rays: a pixel list needs n")
            n = model.width * model.height - int(first_pixel)
        self._check(self._lib.pt_camera_rays(self._ctx, C.byref(cam), C.byref(model), int(frame), pixels_ptr, int(n), int(first_pixel), rays_ptr))

    def render_camera(self, cam, model, params, out_ptr, rays_ptr, spp=1, hdr=False):
        """spp samples of the whole image of a camera model into out float[H][W][3] (the running mean of render_rays, N =
        params.sample_index ..): per sample s one camera_rays of frame params.frame + s into rays float[H * W][8] and one one-sample
        render_rays of that frame over them — a fresh jittered ray per sample (anti-aliasing; depth of field for a thin lens), all
        on the context's stream, with no upload and no sync.  With a pinhole model this is launch_kernel's frame bit for bit
        (hdr=False).  Asynchronous until sync()."""
        n = model.width * model.height
        q = Params.from_buffer_copy(params)
        for s in range(int(spp)):
            q.frame, q.sample_index = params.frame + s, params.sample_index + s
            self.camera_rays(cam, model, q.frame, rays_ptr)
            self.render_rays(rays_ptr, n, out_ptr, q, 1, 0, hdr)

    def render_model(self, cam, model, params, out_ptr, spp=1, hdr=False, n=None, first_pixel=0, pixels_ptr=None):
        """spp samples of pixels of a camera model's image in ONE call (pt_render_camera): what render_camera's loop computes, bit
        for bit, without a ray buffer and without a launch per sample — each sample's jittered ray is made in the path kernel.
        out float[n][3], the running mean of render_rays (N = params.sample_index ..); row i is pixel first_pixel + i, or
        pixels_ptr[i] (uint32 on the device; n is then required): a listed pixel gets the bits it has in the full frame, an index
        past the image the miss sample.  n defaults to the pixels from first_pixel to the end of the image.  Asynchronous until
        sync()."""
        if n is None:
            if pixels_ptr is not None:
                raise ValueError("render_model: a pixel list needs n")
            n = model.width * model.height - int(first_pixel)
        self._check(self._lib.pt_render_camera(self._ctx, C.byref(cam), C.byref(model), pixels_ptr, int(n), int(first_pixel), out_ptr,
                                               C.byref(params), int(spp), _abi.RAYS_HDR if hdr else _abi.RAYS_CLAMPED))

    def render_pixels(self, cam, model, params, accum_ptr, counts_ptr, moments_ptr=None, spp=1, hdr=False, n=None, pixels_ptr=None):
        """spp more samples of listed pixels folded into FULL-FRAME buffers, every pixel from its own sample count on
        (pt_render_pixels): accum float[H*W][3], counts uint32[H*W], moments float[H*W][2] (optional), the image being the model's.
        pixels_ptr: n pixel numbers (uint32 on the device; n is then required, a pixel listed once at most), or None: every pixel.
        Sample s of a pixel is render_model's for that pixel in frame params.frame + s; the pixel's count gives N, so only the counts
        need zeroing before the first pass and params.sample_index is not read.  Unlisted pixels keep their bits.  Asynchronous
        until sync()."""
        if n is None:
            if pixels_ptr is not None:
                raise ValueError("render_pixels: a pixel list needs n")
            n = model.width * model.height
        self._check(self._lib.pt_render_pixels(self._ctx, C.byref(cam), C.byref(model), pixels_ptr, int(n), accum_ptr, moments_ptr, counts_ptr,
                                               C.byref(params), int(spp), _abi.RAYS_HDR if hdr else _abi.RAYS_CLAMPED))

    def select_pixels(self, moments_ptr, counts_ptr, pixels_ptr, width, height, threshold, min_samples=0, max_samples=0xFFFFFFFF):
        """(n, mean relative standard error): the n pixels that need more samples, as an ascending list in pixels uint32[H*W]
        (pt_select_pixels) — those below max_samples that are below max(min_samples, 2) or whose relative standard error, from the
        moments and the pixel's own count, exceeds `threshold`.  Synchronises."""
        sp = SelectParams(int(width), int(height), float(threshold), int(min_samples), int(max_samples), 0)
        n, mean = C.c_uint64(), C.c_double()
        self._check(self._lib.pt_select_pixels(self._ctx, C.byref(sp), moments_ptr, counts_ptr, pixels_ptr, C.byref(n), C.byref(mean)))
        return n.value, mean.value

    def tonemap(self, color_ptr, width, height, rgba_ptr=None, out_ptr=None, curve=_abi.TONE_CLAMP, transfer=_abi.XFER_LINEAR, exposure=1.0,
                white=float("inf"), exposure_ptr=None):
        """A float[H][W][3] buffer into display words (pt_tonemap): colour x exposure (x exposure_ptr[0] on the device, e.g. the
        state meter() keeps), the curve TONE_CLAMP / TONE_REINHARD (white: the scaled luminance shown as white) / TONE_ACES, then the
        transfer XFER_LINEAR / XFER_SRGB / XFER_GAMMA22 into rgba uint32[H][W]; out float[H][W][3] (optional, may be color) receives
        the curve's output before the transfer.  At least one of rgba_ptr, out_ptr.  Asynchronous until sync()."""
        tp = TonemapParams(int(width), int(height), int(curve), int(transfer), float(exposure), float(white))
        self._check(self._lib.pt_tonemap(self._ctx, C.byref(tp), color_ptr, exposure_ptr, out_ptr, rgba_ptr))

    def meter(self, color_ptr, width, height, state_ptr, key=0.18, low_pct=0.0, high_pct=1.0, min_exposure=2.0 ** -16, max_exposure=2.0 ** 16,
              adapt=1.0, reset=False):
        """The exposure that shows a float[H][W][3] buffer's average luminance at `key`, found and kept on the device (pt_meter):
        state float[4] = (exposure in use, this frame's target, metered luminance, pixels that took part); the average is the
        log-average of the pixels between the low_pct and high_pct shares of the luminance histogram; adapt < 1 moves the exposure
        in use only part of the way to the target, reset jumps.  Pass state_ptr as tonemap(exposure_ptr=).  Asynchronous until
        sync(); nothing comes back to the host."""
        mp = MeterParams(int(width), int(height), float(key), float(low_pct), float(high_pct), float(min_exposure), float(max_exposure), float(adapt))
        self._check(self._lib.pt_meter(self._ctx, C.byref(mp), color_ptr, state_ptr, 1 if reset else 0))

    def upload_environment(self, texels, front=(0, 0, -1), right=(1, 0, 0), up=(0, 1, 0), scale=(1, 1, 1), filter=_abi.ENV_BILINEAR, light=False):
        """Light the paths that leave the scene with a latitude-longitude map (pt_upload_environment) instead of bk_color: texels
        float32 [H][W][3] on the host, in the layout `pt_app --equirect` writes for a camera with this front / right / up (the
        defaults: the default camera's, i.e. the world frame); scale multiplies the texels per channel; filter ENV_BILINEAR or
        ENV_NEAREST.  Waits for renders in flight; a render issued afterwards sees the new map.  With a map the stage-split
        pipeline is not chosen.  light: the map also gets a sampling distribution (PT_OPT_ENV_LIGHT for this upload; the option is
        0 again afterwards) and is one of FLAG_NEE's lights in calls that have FLAG_MISS_KEEPS_PATH too — what a map with a small,
        bright sun needs (FLAG_MIS weighs those shadow rays against the bounce rays, which sample the dim sky around it better);
        environment_is_light() tells whether it took (an orthonormal basis, a map that is not black)."""
        a = np.ascontiguousarray(texels, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("upload_environment: a float32 array of shape (H, W, 3) expected")
        ev = Environment()
        ev.width, ev.height = a.shape[1], a.shape[0]
        ev.front[:], ev.right[:], ev.up[:], ev.scale[:] = front, right, up, scale
        ev.filter = int(filter)
        self.set_option(_abi.OPT_ENV_LIGHT, 1 if light else 0)
        try:
            self._check(self._lib.pt_upload_environment(self._ctx, C.byref(ev), a.ctypes.data))
        finally:
            self.set_option(_abi.OPT_ENV_LIGHT, 0)

    def clear_environment(self):
        """Back to bk_color (and to the stage-split pipeline): pt_upload_environment with no map."""
        self._check(self._lib.pt_upload_environment(self._ctx, None, None))

    def eval_environment(self, rays_ptr, n, out_ptr):
        """What the map sends along the directions of a ray batch (pt_eval_environment): rays float[n][8], words 4-6 read (any
        length); out float[n][3].  Asynchronous until sync()."""
        self._check(self._lib.pt_eval_environment(self._ctx, rays_ptr, int(n), out_ptr))

    def environment_is_light(self):
        """Whether the context's map carries a sampling distribution (pt_environment_is_light): uploaded with light=True, basis
        orthonormal, not black.  False without a map."""
        out = C.c_int(0)
        self._check(self._lib.pt_environment_is_light(self._ctx, C.byref(out)))
        return bool(out.value)

    def sample_environment(self, u_ptr, n, dir_pdf_ptr, radiance_ptr=None):
        """Draw directions from the map's distribution (pt_sample_environment): u float[n][2] in [0, 1); dir_pdf float[n][4] =
        (d.xyz, density per steradian); radiance float[n][3], the lookup along d (optional).  Asynchronous until sync()."""
        self._check(self._lib.pt_sample_environment(self._ctx, u_ptr, int(n), dir_pdf_ptr, radiance_ptr))

    def environment_pdf(self, rays_ptr, n, pdf_ptr):
        """The density sample_environment has along the directions of a ray batch (pt_environment_pdf): rays float[n][8], words 4-6
        read (any length); pdf float[n].  Asynchronous until sync()."""
        self._check(self._lib.pt_environment_pdf(self._ctx, rays_ptr, int(n), pdf_ptr))

    def render_aux(self, cam, params, albedo_ptr, normal_ptr, position_ptr, id_ptr=None):
        """First-hit guide buffers of the pixel-centre rays (pt_render_aux): albedo, normal, position as float[H][W][4], the hit
        id as int32[H][W] (optional).  Asynchronous until sync()."""
        self._check(self._lib.pt_render_aux(self._ctx, C.byref(cam), C.byref(params), albedo_ptr, normal_ptr, position_ptr, id_ptr))

    def render_aux_camera(self, cam, model, params, albedo_ptr, normal_ptr, position_ptr, id_ptr=None):
        """render_aux() under a camera model (pt_render_aux_camera): the image is model.width x model.height, the ray of a pixel
        the one camera_rays() writes for it with centre=True and no aperture; of params only cull_backfaces and tri_col are read.
        The guides of a frame made by render_camera() / render_pixels(), for denoise(), denoise_variance() and
        temporal_camera().  Asynchronous until sync()."""
        self._check(self._lib.pt_render_aux_camera(self._ctx, C.byref(cam), C.byref(model), C.byref(params), albedo_ptr, normal_ptr,
                                                   position_ptr, id_ptr))

    def denoise(self, color_ptr, albedo_ptr, normal_ptr, position_ptr, width, height, out_ptr, rgba_ptr=None,
                iterations=DENOISE_DEFAULTS["iterations"], sigma_color=DENOISE_DEFAULTS["sigma_color"],
                sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_position=DENOISE_DEFAULTS["sigma_position"]):
        """Edge-avoiding a-trous filter of an accumulator (pt_denoise): color / out float[H][W][3] (out may be color), the
        guides of render_aux, the display words into rgba (optional).  A sigma <= 0 switches its term off."""
        dp = DenoiseParams(int(width), int(height), int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position))
        self._check(self._lib.pt_denoise(self._ctx, C.byref(dp), color_ptr, albedo_ptr, normal_ptr, position_ptr, out_ptr, rgba_ptr))

    def denoise_variance(self, color_ptr, moments_ptr, length_ptr, albedo_ptr, normal_ptr, position_ptr, width, height, out_ptr,
                         out_variance_ptr=None, rgba_ptr=None, samples_per_frame=1.0,
                         iterations=DENOISE_VARIANCE_DEFAULTS["iterations"], sigma_luminance=DENOISE_VARIANCE_DEFAULTS["sigma_luminance"],
                         sigma_normal=DENOISE_VARIANCE_DEFAULTS["sigma_normal"], sigma_position=DENOISE_VARIANCE_DEFAULTS["sigma_position"]):
        """Variance-guided a-trous filter (pt_denoise_variance): denoise() with a luminance stop scaled by each pixel's standard
        error.  moments float[H][W][2] as launch_kernel(moments_ptr=) keeps them, samples_per_frame the samples behind one frame
        of them, length (optional) float[H][W] the frames behind each pixel as temporal() writes it; out_variance (optional)
        float[H][W] receives the variance of the filtered mean luminance.  Asynchronous until sync()."""
        dp = DenoiseVarianceParams(int(width), int(height), int(iterations), float(sigma_luminance), float(sigma_normal),
                                   float(sigma_position), float(samples_per_frame), 0)
        self._check(self._lib.pt_denoise_variance(self._ctx, C.byref(dp), color_ptr, moments_ptr, length_ptr, albedo_ptr, normal_ptr,
                                                  position_ptr, out_ptr, out_variance_ptr, rgba_ptr))

    def temporal(self, width, height, prev_cam, prev_color_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr, prev_id_ptr,
                 cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr, out_length_ptr, rgba_ptr=None,
                 max_history=TEMPORAL_DEFAULTS["max_history"], plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"],
                 normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"]):
        """Temporal reprojection (pt_temporal): the history (colour float[H][W][3], length float[H][W], the guides of render_aux
        at prev_cam) carried into the current frame (cur colour and guides); the new history into out colour / length, its
        display words into rgba (optional).  prev_color_ptr=None: no history yet (prev_cam and the other prev_* are ignored).
        out colour may be cur colour, never prev colour.  Asynchronous until sync()."""
        tp = TemporalParams(int(width), int(height), float(max_history), float(plane_tolerance), float(normal_threshold), 0)
        self._check(self._lib.pt_temporal(self._ctx, C.byref(tp), C.byref(prev_cam) if prev_cam is not None else None,
                                          prev_color_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr, prev_id_ptr,
                                          cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr, out_length_ptr, rgba_ptr))

    def temporal_motion(self, width, height, prev_cam, prev_verts, cur_verts, n_tris, prev_color_ptr, prev_length_ptr, prev_normal_ptr,
                        prev_position_ptr, prev_id_ptr, cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr,
                        out_length_ptr, rgba_ptr=None, motion_ptr=None, max_history=TEMPORAL_DEFAULTS["max_history"],
                        plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"], normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"]):
        """temporal() for a scene whose triangles moved between the two frames (pt_temporal_motion): prev_verts / cur_verts are
        the float32 rows v0, v1, v2 by original triangle id that refit_bvh took for the previous and for the current frame (a
        DeviceBuffer or a raw device pointer each; they may be the same buffer), n_tris their number of rows.  Both id pointers are
        required.  motion_ptr (optional): float[H][W][2], where in the previous frame each pixel's surface point was, relative
        to the pixel.  Asynchronous until sync()."""
        pv, cv = (v.ptr if isinstance(v, DeviceBuffer) else v for v in (prev_verts, cur_verts))
        tp = TemporalParams(int(width), int(height), float(max_history), float(plane_tolerance), float(normal_threshold), 0)
        self._check(self._lib.pt_temporal_motion(self._ctx, C.byref(tp), C.byref(prev_cam) if prev_cam is not None else None, pv, cv, int(n_tris),
                                                 prev_color_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr, prev_id_ptr,
                                                 cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr, out_length_ptr,
                                                 rgba_ptr, motion_ptr))

    def temporal_moments(self, width, height, prev_cam, prev_verts, cur_verts, n_tris, prev_moments_ptr, prev_length_ptr, prev_normal_ptr,
                         prev_position_ptr, prev_id_ptr, cur_moments_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_moments_ptr,
                         max_history=TEMPORAL_DEFAULTS["max_history"], plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"],
                         normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"]):
        """The luminance moments float[H][W][2] reprojected as temporal() (prev_verts = cur_verts = None) or temporal_motion()
        reprojects the colour (pt_temporal_moments).  prev_length_ptr is the one the colour call of the same frame reads; no
        length is written.  prev_moments_ptr=None: no history, out = cur.  Asynchronous until sync()."""
        pv, cv = (v.ptr if isinstance(v, DeviceBuffer) else v for v in (prev_verts, cur_verts))
        tp = TemporalParams(int(width), int(height), float(max_history), float(plane_tolerance), float(normal_threshold), 0)
        self._check(self._lib.pt_temporal_moments(self._ctx, C.byref(tp), C.byref(prev_cam) if prev_cam is not None else None, pv, cv, int(n_tris),
                                                  prev_moments_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr, prev_id_ptr,
                                                  cur_moments_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_moments_ptr))

    def temporal_camera(self, width, height, prev_cam, prev_model, prev_color_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr,
                        prev_id_ptr, cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr, out_length_ptr,
                        rgba_ptr=None, motion_ptr=None, prev_verts=None, cur_verts=None, n_tris=0,
                        max_history=TEMPORAL_DEFAULTS["max_history"], plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"],
                        normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"]):
        """temporal() for a history rendered under a camera model (pt_temporal_camera): prev_cam and prev_model are the camera
        and the CameraModel of the prev_* buffers (the guides of render_aux_camera()); the current camera is not needed.  With
        prev_verts / cur_verts (and n_tris) it follows moved triangles as temporal_motion() does and needs both id pointers;
        without them the ids are optional.  motion_ptr (optional, either way): float[H][W][2].  Asynchronous until sync()."""
        pv, cv = (v.ptr if isinstance(v, DeviceBuffer) else v for v in (prev_verts, cur_verts))
        tp = TemporalParams(int(width), int(height), float(max_history), float(plane_tolerance), float(normal_threshold), 0)
        self._check(self._lib.pt_temporal_camera(self._ctx, C.byref(tp), C.byref(prev_cam) if prev_cam is not None else None,
                                                 C.byref(prev_model) if prev_model is not None else None, pv, cv, int(n_tris),
                                                 prev_color_ptr, prev_length_ptr, prev_normal_ptr, prev_position_ptr, prev_id_ptr,
                                                 cur_color_ptr, cur_normal_ptr, cur_position_ptr, cur_id_ptr, out_color_ptr, out_length_ptr,
                                                 rgba_ptr, motion_ptr))

    # ------------------------------------------------------------------ measurement
    def counters(self):
        c = Counters()
        self._check(self._lib.pt_get_counters(self._ctx, C.byref(c)))
        return {f: getattr(c, f) for f, _ in Counters._fields_}

    def stage_ms(self):
        """Device ms of the last timed launch_kernel (PT_OPT_TIMING=1) by stage (pt_get_stage_ms)."""
        out = (C.c_float * 6)()
        self._check(self._lib.pt_get_stage_ms(self._ctx, out, 6))
        return dict(zip(("none", "frame", "generate", "extend", "shade", "fold"), [float(v) for v in out]))

    def auto_choice(self):
        """PT_KERNEL_AUTO's pick for the last configuration: (kernel or KERNEL_AUTO while undecided, ms persistent, ms wavefront)."""
        k, a, b = C.c_int(), C.c_float(), C.c_float()
        self._check(self._lib.pt_auto_choice(self._ctx, C.byref(k), C.byref(a), C.byref(b)))
        return k.value, a.value, b.value

    def tree_cost(self):
        """(expected wide-node visits, expected triangle tests) of a random ray: surface-area cost of the 4-wide tree."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.pt_tree_cost(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def tree_items(self):
        """The item buffer of the tree on the context, downloaded (pt_tree_items; layout: DESIGN.md 3.5): three float32 arrays of
        shape (n, 16) — binary nodes, records, wide nodes (views of one buffer; integer words through .view(np.int32)) — and the
        depth of the 4-wide tree.  Synchronises."""
        p, nb, nr, nw, d = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self._lib.pt_tree_items(self._ctx, C.byref(p), C.byref(nb), C.byref(nr), C.byref(nw), C.byref(d)))
        n = nb.value + nr.value + nw.value
        buf = np.empty((n, 16), np.float32)
        self._check(self._lib.pt_download(self._ctx, buf.ctypes.data, p.value, buf.nbytes))
        return buf[:nb.value], buf[nb.value:nb.value + nr.value], buf[nb.value + nr.value:], d.value

    def wave_stats(self):
        """pt_get_wave_stats of the last instrumented launch.  Under PT_KERNEL_WAVEFRONT "it_shade" holds the 64-ray groups walked by
        the bounce-0 packet walk (PT_OPT_FIRST_WALK 1; include/ptmi.h), not shading passes; "walk_free" the rays PT_OPT_ROOT_CULL 2 kept
        out of the extend queue, "occluded" the last-segment rays PT_OPT_LAST_OCCLUDERS 2 decided in the shade stage."""
        out = (C.c_uint64 * 12)()
        self._check(self._lib.pt_get_wave_stats(self._ctx, out, 12))
        names = ("it_node", "act_node", "it_rec", "act_rec", "it_shade", "act_shade", "it_begin", "act_begin", "it_loop", "stack_overflows",
                 "walk_free", "occluded")
        return dict(zip(names, [int(v) for v in out]))

    def last_build_ms(self):
        """Device time of the build behind the tree on the context; -1 when it is an uploaded hierarchy."""
        ms = C.c_float()
        if self._lib.pt_last_build_ms(self._ctx, C.byref(ms)) != 0:
            return -1.0
        return ms.value

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(self._lib.pt_last_kernel_ms(self._ctx, C.byref(ms)))
        return ms.value


class TemporalHistory:
    """The ping-pong buffers of a host's temporal accumulation: two history colours, two lengths, two sets of guide buffers and the
    camera (with its model, for a frame pushed with one) of the frame pushed last.  push() is one displayed frame of the loop: guides,
    reprojection, swap."""

    def __init__(self, tracer, width, height, with_ids=True, with_moments=False):
        self.t, self.W, self.H = tracer, int(width), int(height)
        n = self.W * self.H
        # with_moments: two moment histories beside the colours; self.moments = the one the last push wrote (None before it)
        self.moment = [tracer.malloc(n * 8) for _ in range(2)] if with_moments else []
        self.moments = None
        self.color = [tracer.malloc(n * 12) for _ in range(2)]
        self.length = [tracer.malloc(n * 4) for _ in range(2)]
        self.guides = [[tracer.malloc(n * 16) for _ in range(3)] + [tracer.malloc(n * 4) if with_ids else None] for _ in range(2)]
        self.cam = None     # the camera of the history; None = nothing pushed yet
        self.model = None   # ... and its CameraModel, when that frame was pushed with one
        self.cur = 0        # the set the NEXT push writes

    def reset(self):
        """Forget the history (a cut: the next push starts over)."""
        self.cam = self.model = None

    def _ptrs(self, k):
        return [b.ptr if b is not None else None for b in self.guides[k]]

    def push(self, cam, params, color_ptr, rgba_ptr=None, moved=None, motion_ptr=None, moments_ptr=None, model=None, **temporal):
        """One frame: render_aux for `cam` (params: the frame's pt_params), then temporal() of the frame in color_ptr (rendered
        with sample_index = 1; never written) against the stored history — or with no history the first time — then the swap.
        Returns (color_ptr, length_ptr, (albedo, normal, position, id) ptrs) of the new history; the colour and the guides can be
        passed to denoise() directly.  **temporal: max_history, plane_tolerance, normal_threshold.  Asynchronous.
        moved = (prev_verts_ptr, cur_verts_ptr, n_tris): the triangles moved since the last push (refit_bvh), so the frame goes
        through temporal_motion() (the history needs ids), with motion_ptr as its motion buffer.  The caller owns and ping-pongs
        the two vertex buffers: the previous one stays unchanged until the push that reads it has been issued.
        moments_ptr (a history made with_moments=True needs it, no other takes it): the frame's moments, as launch_kernel(moments_ptr=)
        kept them (never written); they are reprojected with the same history and the same lengths by temporal_moments(), and
        self.moments is the new moment history, to go into denoise_variance() with the returned lengths.
        model (a CameraModel of this history's size; every push of one history with it, or none): the frame was rendered under
        that camera model (render_camera, render_pixels), so its guides come from render_aux_camera() and the reprojection goes
        through temporal_camera() with the model of the frame pushed before; motion_ptr then needs no moved=.  Not with
        with_moments=True (there is no moments call for the camera models)."""
        if (moments_ptr is not None) != bool(self.moment):
            raise ValueError("TemporalHistory.push: moments_ptr goes with with_moments=True")
        k, o = self.cur, 1 - self.cur
        alb, nrm, pos, ids = self._ptrs(k)
        if model is not None:
            if self.moment:
                raise ValueError("TemporalHistory.push: model= does not go with with_moments=True")
            if (model.width, model.height) != (self.W, self.H):
                raise ValueError("TemporalHistory.push: the model's image is not the history's")
            if self.cam is not None and self.model is None:
                raise ValueError("TemporalHistory.push: the history was pushed without a model (reset() first)")
            self.t.render_aux_camera(cam, model, params, alb, nrm, pos, ids)
            _, pn, pp, pi = self._ptrs(o)
            prev = (None,) * 7 if self.cam is None else (self.cam, self.model, self.color[o].ptr, self.length[o].ptr, pn, pp, pi)
            rows = dict(zip(("prev_verts", "cur_verts", "n_tris"), moved)) if moved is not None else {}
            self.t.temporal_camera(self.W, self.H, *prev, color_ptr, nrm, pos, ids, self.color[k].ptr, self.length[k].ptr, rgba_ptr, motion_ptr,
                                   **rows, **temporal)
            self.cam, self.model = Camera.from_buffer_copy(cam), CameraModel.from_buffer_copy(model)
            self.cur = o
            return self.color[k].ptr, self.length[k].ptr, (alb, nrm, pos, ids)
        if self.model is not None:
            raise ValueError("TemporalHistory.push: the history was pushed with a model (reset() first)")
        self.t.render_aux(cam, params, alb, nrm, pos, ids)
        if self.cam is None:
            prev = (None,) * 6
        else:
            _, pn, pp, pi = self._ptrs(o)
            prev = (self.cam, self.color[o].ptr, self.length[o].ptr, pn, pp, pi)
        if moved is not None:
            self.t.temporal_motion(self.W, self.H, prev[0], *moved, *prev[1:], color_ptr, nrm, pos, ids, self.color[k].ptr, self.length[k].ptr,
                                   rgba_ptr, motion_ptr, **temporal)
        else:
            if motion_ptr is not None:
                raise ValueError("TemporalHistory.push: motion_ptr goes with moved=")
            self.t.temporal(self.W, self.H, *prev, color_ptr, nrm, pos, ids, self.color[k].ptr, self.length[k].ptr, rgba_ptr, **temporal)
        if self.moment:
            pm = None if self.cam is None else self.moment[o].ptr
            self.t.temporal_moments(self.W, self.H, prev[0], *(moved if moved is not None else (None, None, 0)), pm, *prev[2:],
                                    moments_ptr, nrm, pos, ids, self.moment[k].ptr, **temporal)
            self.moments = self.moment[k].ptr
        self.cam = Camera.from_buffer_copy(cam)
        self.cur = o
        return self.color[k].ptr, self.length[k].ptr, (alb, nrm, pos, ids)

    def free(self):
        for b in self.color + self.length + self.moment + [x for gset in self.guides for x in gset if x is not None]:
            b.free()
        self.color, self.length, self.guides, self.cam, self.model = [], [], [], None, None
        self.moment, self.moments = [], None


class AdaptiveSampler:
    """The buffers and the loop of adaptive sampling for one image of a camera model: accumulator, luminance moments, sample counts
    and the pixel list.  run() renders one pass over every pixel, then select_pixels -> render_pixels over the list until nothing
    is selected: every pixel gets samples until its relative standard error is at most `threshold` (never fewer than min_spp, never
    more than max_spp, pass_spp per pass)."""

    def __init__(self, tracer, model, threshold, min_spp, max_spp, pass_spp):
        min_spp, max_spp, pass_spp = int(min_spp), int(max_spp), int(pass_spp)
        if pass_spp < 1 or min_spp < pass_spp or max_spp < min_spp or min_spp % pass_spp or max_spp % pass_spp:
            raise ValueError("AdaptiveSampler: min_spp and max_spp must be multiples of pass_spp with pass_spp <= min_spp <= max_spp")
        self.t, self.model, self.W, self.H = tracer, model, model.width, model.height
        self.threshold, self.min_spp, self.max_spp, self.pass_spp = float(threshold), min_spp, max_spp, pass_spp
        n = self.W * self.H
        self.accum, self.moments, self.counts, self.pixels = tracer.malloc(n * 12), tracer.malloc(n * 8), tracer.malloc(n * 4), tracer.malloc(n * 4)
        self.passes = []    # of the last run: (pixels rendered, mean relative standard error before the pass; None for the first)

    def run(self, cam, params, hdr=False):
        """The whole loop for `cam` from frame params.frame on; pass k renders frames params.frame + k * pass_spp ..: a pixel that
        ends with count c holds exactly the frames params.frame .. + c - 1, i.e. launch_kernel(spp=c)'s accumulator and moments for
        a pinhole model.  Returns (samples rendered in all, mean relative standard error at the end); accum, moments and counts hold
        the result.  Synchronises once per pass."""
        t, n = self.t, self.W * self.H
        self.counts.zero()
        q = Params.from_buffer_copy(params)
        q.sample_index = 1
        t.render_pixels(cam, self.model, q, self.accum.ptr, self.counts.ptr, self.moments.ptr, spp=self.pass_spp, hdr=hdr)
        self.passes = [(n, None)]
        k = 1
        while True:
            m, mean = t.select_pixels(self.moments.ptr, self.counts.ptr, self.pixels.ptr, self.W, self.H, self.threshold, self.min_spp, self.max_spp)
            if m == 0:
                return sum(c for c, _ in self.passes) * self.pass_spp, mean
            q.frame = params.frame + k * self.pass_spp
            t.render_pixels(cam, self.model, q, self.accum.ptr, self.counts.ptr, self.moments.ptr, spp=self.pass_spp, hdr=hdr, n=m, pixels_ptr=self.pixels.ptr)
            self.passes.append((m, mean))
            k += 1

    def free(self):
        for b in (self.accum, self.moments, self.counts, self.pixels):
            b.free()
        self.accum = self.moments = self.counts = self.pixels = None


def algorithmic_bytes(counters, n_spheres):
    """B = sum(64*N_inner + 48*N_tri + 16*N_leaf + 4*[hit]) + 44*n_spheres per
    segment + 28 B per pixel-sample (12 accum read + 12 accum write + 4 RGBA8 write)."""
    return (64 * counters["inner"] + 48 * counters["tris"] + 16 * counters["leaves"] + 4 * counters["hits"]
            + 44 * n_spheres * counters["rays"] + 28 * counters["paths"])
