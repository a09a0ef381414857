"""Adaptive sampling without a GPU: pt_render_pixels and pt_select_pixels in the header, the binding and the library, the numpy
restatement (tests/adaptive_ref.py) against hand-computed cases, the check program's walk over the new call's request domain and
over both calls' argument rules (csrc/pt_variants_check.cpp), and the host loop class's argument rule."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import gpu_pathtracer_amd as g
import moments_ref as M

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")
F = np.float32


def header():
    return open(os.path.join(ROOT, "include", "ptmi.h")).read()


def flat(text):
    return re.sub(r"\s+\*?\s*", " ", text)


# ---------------------------------------------------------------------------------------------------- the surface
def test_struct_size_and_symbols():
    assert C.sizeof(g.SelectParams) == 24 and C.sizeof(g._abi.SelectParams) == 24
    assert [f for f, _ in g.SelectParams._fields_] == ["width", "height", "threshold", "min_samples", "max_samples", "_pad"]
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_render_pixels"][2]) == 11 and len(rows["pt_select_pixels"][2]) == 7
    lib = g._abi.ptmi()
    at = lib.pt_render_pixels.argtypes
    assert at[1]._type_ is g.Camera and at[2]._type_ is g.CameraModel and at[4] is C.c_size_t and at[8]._type_ is g.Params
    assert at[9] is C.c_uint32 and at[10] is C.c_int and lib.pt_render_pixels.restype is C.c_int
    at = lib.pt_select_pixels.argtypes
    assert at[1]._type_ is g.SelectParams and at[5]._type_ is C.c_uint64 and at[6]._type_ is C.c_double
    assert lib.pt_abi_version() == 3
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libptmi.so")], capture_output=True, text=True)
    assert nm.returncode == 0
    for name in ("pt_render_pixels", "pt_select_pixels"):
        assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"libptmi.so does not export {name}"
    blob = open(os.path.join(CSRC, "libptmi.so"), "rb").read()
    for kernel in (b"k_fold_pixels", b"k_select_count", b"k_select_scan", b"k_select_write"):
        assert kernel in blob, kernel
    assert list(inspect.signature(g.PathTracer.render_pixels).parameters) == ["self", "cam", "model", "params", "accum_ptr", "counts_ptr", "moments_ptr", "spp", "hdr", "n", "pixels_ptr"]
    assert list(inspect.signature(g.PathTracer.select_pixels).parameters)[:6] == ["self", "moments_ptr", "counts_ptr", "pixels_ptr", "width", "height"]
    assert list(inspect.signature(g.AdaptiveSampler.__init__).parameters) == ["self", "tracer", "model", "threshold", "min_spp", "max_spp", "pass_spp"]


def test_header_declares_the_calls_and_states_the_contract():
    src = header()
    assert re.search(r"int\s+pt_render_pixels\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_camera\s*\*\s*cam,\s*const\s+pt_camera_model\s*\*\s*cm,"
                     r"\s*const\s+uint32_t\s*\*\s*pixels_dev[^,)]*,\s*size_t\s+n,\s*float\s*\*\s*accum_dev[^,)]*,\s*float\s*\*\s*moments_dev[^,)]*,"
                     r"\s*uint32_t\s*\*\s*counts_dev[^,)]*,\s*const\s+pt_params\s*\*\s*params,\s*uint32_t\s+spp,\s*int\s+mode\s*\)\s*;", src)
    assert re.search(r"int\s+pt_select_pixels\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_select_params\s*\*\s*sp,\s*const\s+float\s*\*\s*moments_dev,"
                     r"\s*const\s+uint32_t\s*\*\s*counts_dev,\s*uint32_t\s*\*\s*pixels_dev[^,)]*,\s*uint64_t\s*\*\s*n_selected,\s*double\s*\*\s*mean_rse[^,)]*\)\s*;", src)
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src), "additions: the ABI version stays"
    assert src.index("int pt_render_camera(") < src.index("int pt_render_pixels(") < src.index("int pt_select_pixels(")
    text = flat(src[src.index("adaptive sampling: more samples only where"):src.index("int pt_select_pixels(")])
    for piece in ("N = c + 1 + s", "only counts_dev needs zeroing", "A pixel listed twice in one call is the caller's error",
                  "A count that would pass 2^32 - 1", "for all five models and both modes", "every unlisted pixel keeps its bits in all three buffers",
                  "the counts carry N", "prefixed pt_render_pixels:", "also at spp == 1", "in ASCENDING order",
                  "nothing is written beyond entry *n_selected - 1", "(strictly above)", "never selected", "SYNCHRONISES the context's stream",
                  "16 bytes per block", "no block waits for another and nothing is added atomically", "min_samples is the guard",
                  "Errors, in this order", "n_selected equals its n_above"):
        assert flat(piece) in text, piece
    camera = flat(src[src.index("pt_render_camera path-traces"):src.index("int pt_render_camera(")])
    assert "pt_render_pixels below keeps them" in camera[camera.index("Left out:"):]


def test_null_context_is_refused_first():
    lib = g._abi.ptmi()
    cam, cm, p = g.default_camera(37, 23), g.camera_model("pinhole", 37, 23), g.default_params(37, 23)
    assert lib.pt_render_pixels(None, C.byref(cam), C.byref(cm), None, 851, None, None, None, C.byref(p), 1, g._abi.RAYS_CLAMPED) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()
    assert lib.pt_render_pixels(None, None, None, None, 0, None, None, None, None, 0, 0) == -1   # before n == 0 and spp == 0
    sp = g.SelectParams(37, 23, 0.1, 4, 32, 0)
    n = C.c_uint64(77)
    assert lib.pt_select_pixels(None, C.byref(sp), None, None, None, C.byref(n), None) == -1 and n.value == 77
    assert "null ctx" in lib.pt_last_error(None).decode()


def test_the_kernels_live_beside_their_neighbours_and_restate_nothing():
    rays, den, api, plan = (open(os.path.join(CSRC, f)).read() for f in ("pt_k_rays.hip", "pt_select.hip", "ptmi.hip", "pt_plan.h"))
    fold = rays[rays.index("k_fold_pixels(const KParams"):rays.index("namespace ptmi")]
    assert "rays_accumulate<HDR>(" in fold and "pt_moments(" in fold and "0.2126f" not in fold, "the fold reuses the accumulator's and the moments' device functions"
    sel = den[den.index("namespace {"):den.index("}  // namespace")]   # the file's kernels, k_frame_error among them, and what its two calls share
    assert "atomic" not in sel and "__threadfence" not in sel and "while" not in sel, "no atomics, no fences, no waiting"
    assert sel.count("__global__") == 4 and "__builtin_amdgcn_mbcnt_hi" in sel and "__ballot(" in sel
    for k in ("k_select_count(const SelectArgs", "k_select_scan(const uint32_t*", "k_select_write(const SelectArgs"):
        assert "__global__ void __launch_bounds__(256) " + k in sel, k
    body = api[api.index("int pt_render_pixels("):api.index("int pt_get_counters(")]
    assert "launch_render_camera(" in body and "launch_fold_pixels(" in body and "launch_fold_rays" not in body
    assert "plan.samples = plan.per_launch > 1 || a.pixels;" in plan
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert len(mk.split("OBJS =")[1].split("\n")[0].split()) == 17, "no new translation unit"


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def test_reference_fold_by_hand():
    # one pixel, count 0: N = 1 overwrites the garbage, N = 2 averages; every value exact in binary32
    col = np.array([[[0.5, 0.25, 2.0], [0.25, 0.75, 1.0]]], F)
    a, m, c = A.fold(col, [0], np.full((1, 3), np.nan, F), np.full((1, 2), np.nan, F))
    assert c.tolist() == [2] and c.dtype == np.uint32
    assert a.tolist() == [[0.375, 0.5, 1.0]]            # blue: clamp(2) = 1, then clamp((1 * 1 + 1) * 0.5) = 1
    a_hdr, _, _ = A.fold(col, [0], np.zeros((1, 3), F), None, hdr=True)
    assert a_hdr.tolist() == [[0.375, 0.5, 1.5]]
    L = M.luminance(col[0])
    want1 = (L[0] * F(1) + L[1]) * F(0.5)
    want2 = (L[0] * L[0] * F(1) + L[1] * L[1]) * F(0.5)
    assert m[0, 0] == want1 and m[0, 1] == want2
    # a pixel that holds 3 samples: N = 4 and 5, with the rounding of 1 / 5 as the device has it
    a0, m0 = np.array([[0.5, 0.5, 0.5]], F), np.array([[0.5, 0.375]], F)
    col = np.array([[[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]], F)
    a, m, c = A.fold(col, [3], a0, m0)
    step = (F(0.5) * F(3) + F(1)) * (F(1) / F(4))
    assert step == F(0.625)
    want = (step * F(4) + F(0)) * (F(1) / F(5))
    assert c.tolist() == [5] and np.all(a[0] == want)
    one = (F(0.2126) + F(0.7152)) + F(0.0722)                          # the luminance of white, not exactly 1
    assert m[0, 0] == (((F(0.5) * F(3) + one) * F(0.25)) * F(4) + F(0)) * (F(1) / F(5))
    # the moments are moments_ref's with N = count + 1 + s, and any split over calls gives the same bits
    rng = np.random.default_rng(5)
    col = rng.random((7, 6, 3), dtype=F) * F(3)
    counts = np.array([0, 1, 2, 5, 0, 3, 9], np.uint32)
    a0, m0 = rng.random((7, 3), dtype=F), rng.random((7, 2), dtype=F)
    a, m, c = A.fold(col, counts, a0, m0)
    for i in range(7):
        want = M.update(col[i], int(counts[i]) + 1, m0[i])
        assert np.array_equal(m[i].view(np.int32), want.view(np.int32))
    a1, m1, c1 = A.fold(col[:, :2], counts, a0, m0)
    a2, m2, c2 = A.fold(col[:, 2:], c1, a1, m1)
    assert np.array_equal(a2.view(np.int32), a.view(np.int32)) and np.array_equal(m2.view(np.int32), m.view(np.int32)) and np.array_equal(c2, c)


def test_reference_rule_by_hand():
    #            n < 2          exact 0        var = 0.75, n = 4: sqrt(0.25) / 1.01      m2 < m1^2      NaN            inf
    mom = np.array([[9, 99], [0.5, 0.25], [1.0, 1.75], [1.0, 0.5], [np.nan, 1.0], [1.0, np.inf], [-0.01, 1.0]], F)
    cnt = np.array([1, 4, 4, 4, 4, 4, 2], np.uint32)
    r = A.rse(mom, cnt)
    assert r.dtype == F and r.tolist()[:2] == [0.0, 0.0] and r[2] == F(0.5) / (F(1.0) + F(0.01)) and r[3:].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert A.rse(mom[2:3], [2])[0] == np.sqrt(F(0.75)) / (F(1.0) + F(0.01))
    sel, _ = A.select(mom, cnt, 0.0)
    assert sel.tolist() == [True, False, True, False, False, False, False]      # n < 2 always; rse 0 is not > 0; NaN and inf never
    sel, _ = A.select(mom, cnt, 0.0, 0, 4)
    assert sel.tolist() == [True, False, False, False, False, False, False]     # at max_samples nothing; below it n < 2 still counts, rse 0 does not
    sel, _ = A.select(mom, cnt, 10.0, 5, 5)
    assert sel.tolist() == [True] * 7                                             # below min_samples whatever the error
    sel, _ = A.select(mom, cnt, float(r[2]), 0, 99)
    assert not sel[2]                                                             # strictly above
    sel, _ = A.select(mom, cnt, float(np.nextafter(r[2], F(0))), 0, 99)
    assert sel[2]
    sel, _ = A.select(mom, np.zeros(7, np.uint32), 0.0, 0, 0)
    assert not sel.any()                                                          # max_samples 0: nothing, not even n = 0


def test_reference_mean_is_frame_errors_for_uniform_counts():
    rng = np.random.default_rng(11)
    m1 = rng.random(851, dtype=F)
    mom = np.stack([m1, m1 * m1 + rng.random(851, dtype=F) * F(0.3)], axis=-1)
    r = A.rse(mom, np.full(851, 8, np.uint32))
    assert np.array_equal(r.view(np.int32), M.rse(mom, 8).view(np.int32))
    sel, _ = A.select(mom, np.full(851, 8, np.uint32), 0.125)
    assert int(sel.sum()) == M.frame_error(mom, 8, 0.125)[1]
    # the tree of 256-pixel blocks: every partial sum of three exactly representable values, by hand
    v = np.zeros(600, F)
    v[[0, 128, 255, 256, 599]] = [1.0, 2.0, 4.0, 8.0, 16.0]
    assert A.mean_rse(v) == 31.0 / 600
    assert abs(A.mean_rse(r) - M.frame_error(mom, 8, 0.0)[0]) < 1e-12


# ---------------------------------------------------------------------------------------------------- the planner
@pytest.mark.parametrize("san", ["", "SAN=1"], ids=["plain", "sanitized"])
def test_check_program_walks_the_new_calls(san):
    """The request domain of pt_render_pixels — every plan goes through the sample buffer — and the error order of both calls."""
    src = open(os.path.join(CSRC, "pt_variants_check.cpp")).read()
    assert "a.pixels = true;" in src and "CHECK(plan.samples);" in src and "check_select_call(" in src
    exe = os.path.join(CSRC, "pt_variants_check")
    build = subprocess.run(["make", "-B", "-C", PKG, "variants_check"] + ([san] if san else []), capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    assert ("-fsanitize=address,undefined" in build.stdout) == bool(san), build.stdout
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout
    m = re.search(r"^camera family k_render_camera: requests=(\d+) words=(\d+) kernels=(\d+)$", run.stdout, re.M)
    assert m and int(m.group(2)) == 19 and int(m.group(3)) == 19, run.stdout   # the new call asks for no new kernel of the family


def test_sampler_refuses_counts_that_are_no_multiples():
    model = g.camera_model("pinhole", 37, 23)
    for bad in ((4, 30, 4), (6, 32, 4), (4, 32, 0), (8, 4, 4), (0, 32, 4)):
        with pytest.raises(ValueError):
            g.AdaptiveSampler(None, model, 0.1, *bad)
