"""Every estimator against closed-form radiance on every kernel (cases and closed forms: tests/estimator_ref.py; the oracle
passes the same cases on the CPU in tests/test_estimators.py).

The parity suites pin the kernels to the oracle bit for bit, and the two share their estimators' arithmetic by design; here the
reference is geometry.  Each case runs on four routes with every option at its default:
  rays        pt_render_rays, HDR: n identical rays (the camera's central ray), one sample each
  mega        pt_render under PT_KERNEL_MEGA_BVH2
  persistent  pt_render under PT_KERNEL_PERSISTENT (a call with PT_FLAG_NEE is rerouted to the stage-split pipeline)
  wavefront   pt_render under PT_KERNEL_WAVEFRONT
A pt_render route renders the 1e-5 field of view at 64 samples per pixel, 64 x 64 for the calls with PT_FLAG_NEE (2^18 samples)
and 128 x 128 for the others (2^20); its estimate is the mean of the accumulator over the pixels and its standard error the
standard deviation of the pixel means / sqrt(pixels).  The rays route draws as many samples.  PT_OPT_TIMING and stage_ms tell
which kernel family ran, and the expectation is that of tests/test_gpu_call_plan.py.

Accepted, per case, route and channel: |mean - E| <= 5 SE; SE <= 0.005 E with PT_FLAG_NEE and <= 0.02 E without (what gives the
5 SE its power: the oracle's SE / E at 2^16 samples is at most 0.0053 with NEE and 0.022 without, so a half and a quarter of
that leave a margin of about 2 and 3); a zero-variance case holds E within 1e-5 E in every sample or pixel (the fold of 64 equal
samples adds at most 1.5 ulp per step weighted k / 64: below 48 ulp = 2.9e-6); a dark case is exactly 0; no HDR sample and no
pixel reaches 1, so the fold's clamp never acted.  Measured on an MI355X: profiles/r16_estimators.txt."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
import estimator_ref as ref
from gpu_support import is_frame_kernel, is_pipeline

pytestmark = pytest.mark.gpu
CASES = ref.cases()
KERNELS = {"mega": g.KERNEL_MEGA_BVH2, "persistent": g.KERNEL_PERSISTENT, "wavefront": g.KERNEL_WAVEFRONT}
SPP = 64


def context(case):
    t = g.PathTracer(0)
    t.set_option(g.OPT_TIMING, 1)
    t.upload_bvh(g.Bvh(case.mesh))
    t.upload_spheres(case.spheres())
    if case.materials is not None:
        t.upload_tri_materials(case.materials, case.tri_material)
    return t


def rays_route(t, case, n):
    """n copies of the camera's central ray, one sample each with the stream of pixel i: the HDR samples [n][3]"""
    rays = np.ascontiguousarray(np.tile(case.ray(), (n, 1)))
    d_r, d_o = t.malloc(rays.nbytes), t.malloc(12 * n)
    d_r.upload(rays)
    t.render_rays(d_r.ptr, n, d_o.ptr, case.params(64, 64), 1, 0, True)
    t.sync()
    out = d_o.download(np.float32, (n, 3))
    d_r.free()
    d_o.free()
    return out


def frame_route(t, case, kernel, side):
    """one pt_render call of SPP samples into a fresh side x side accumulator: (pixel means [side^2][3], stage times)"""
    t.set_option(g.OPT_KERNEL, kernel)
    acc, rgba = t.alloc_frame(side, side)
    t.launch_kernel(acc.ptr, rgba.ptr, case.camera(side, side), case.params(side, side), SPP)
    t.sync()
    ms = t.stage_ms()
    out = acc.download(np.float32, (side * side, 3))
    acc.free()
    rgba.free()
    return out, ms


def family(route, case, ms):
    """(what ran, whether that is what the render call's rules say): the megakernel is a frame kernel; the persistent kernel has no
    room for a shadow ray, so a call with PT_FLAG_NEE runs the pipeline (test_gpu_call_plan's persistent-nee), any other its frame
    kernel; PT_KERNEL_WAVEFRONT runs the pipeline wherever there is a tree, a bounce and the wide walk — every case here."""
    ran = "pipeline" if is_pipeline(ms) else "frame kernel" if is_frame_kernel(ms) else f"neither ({ms})"
    want = "pipeline" if route == "wavefront" or (route == "persistent" and case.nee) else "frame kernel"
    return ran, ran == want


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_route_holds_the_closed_form(case):
    side = 64 if case.nee else 128
    n = side * side * SPP
    bound = 0.005 if case.nee else 0.02
    failures = []
    t = context(case)
    try:
        for route in ("rays",) + tuple(KERNELS):
            if route == "rays":
                x, ran, as_planned = rays_route(t, case, n), "rays kernel", True
            else:
                x, ms = frame_route(t, case, KERNELS[route], side)
                ran, as_planned = family(route, case, ms)
            problems, z, rel = ref.verdict(case, x)
            print(f"EST {case.name:24s} {route:10s} {ran:12s} {case.kind:5s} z {z[0]:+7.2f} {z[1]:+7.2f} {z[2]:+7.2f}  "
                  f"SE/E {rel[0]:.5f} {rel[1]:.5f} {rel[2]:.5f}  max {x.max():.4f}")
            if not as_planned:
                problems.append(f"ran the {ran}")
            if case.kind == "mc" and not (rel <= bound).all():
                problems.append(f"SE / E {rel} above {bound}")
            if not x.max() < 1.0:
                problems.append(f"a sample or pixel reached {x.max()}")
            failures += [f"{route}: {p}" for p in problems]
    finally:
        t.close()
    assert not failures, (case.name, failures)
