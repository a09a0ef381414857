"""pt_render_camera without a GPU: the declaration, the binding, the export, the NULL-context error, the new translation unit in
the Makefile, the contract in the header, and the check program's walk over the call's request domain (csrc/pt_variants_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import gpu_pathtracer_amd as g

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")


def header():
    return open(os.path.join(ROOT, "include", "ptmi.h")).read()


def test_header_declares_the_call():
    src = header()
    assert re.search(r"int\s+pt_render_camera\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_camera\s*\*\s*cam,\s*const\s+pt_camera_model\s*\*\s*cm,"
                     r"\s*const\s+uint32_t\s*\*\s*pixels_dev[^,)]*,\s*size_t\s+n,\s*uint64_t\s+first_pixel,\s*float\s*\*\s*radiance_dev[^,)]*,"
                     r"\s*const\s+pt_params\s*\*\s*params,\s*uint32_t\s+spp,\s*int\s+mode\s*\)\s*;", src)
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src), "an addition: the ABI version stays"
    assert src.index("int pt_camera_rays(") < src.index("pt_render_camera path-traces") < src.index("int pt_render_camera(")


def test_header_states_the_guarantees_and_what_is_left_out():
    src = re.sub(r"\s+\*?\s*", " ", header())
    section = src[src.index("pt_render_camera path-traces"):src.index("int pt_render_camera(")]
    for text in ("(a) without a list the result equals, bit for bit, the loop", "for all five models",
                 "(b) hence with PT_CAM_PINHOLE, first_pixel 0, n = W * H and PT_RAYS_CLAMPED it is pt_render's accumulator bit for bit",
                 "(c) with a list, row i equals row pixels_dev[i] of the full-frame call bit for bit", "repeated indices repeat the value",
                 "an index past the image gives the miss sample (bk_color)", "not of the row number", "frame ^ PT_CAM_LENS_KEY",
                 "prefixed pt_render_camera:", "at most 2^26 slots per launch"):
        assert re.sub(r"\s+\*?\s*", " ", text) in section, text   # (the comment's leading stars go the same way as a product's)
    left = section[section.index("Left out:"):]
    for item in ("luminance moments", "display words", "guide buffers for these cameras", "the stage-split pipeline"):
        assert item in left, item


def test_abi_binds_and_the_library_exports():
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_render_camera"][2]) == 10
    lib = g._abi.ptmi()
    at = lib.pt_render_camera.argtypes
    assert at[4] is C.c_size_t and at[5] is C.c_uint64 and at[8] is C.c_uint32 and at[9] is C.c_int and lib.pt_render_camera.restype is C.c_int
    assert at[1]._type_ is g.Camera and at[2]._type_ is g.CameraModel and at[7]._type_ is g.Params
    assert lib.pt_abi_version() == 3
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libptmi.so")], capture_output=True, text=True)
    assert nm.returncode == 0 and re.search(r"\bT pt_render_camera$", nm.stdout, re.M), "libptmi.so does not export pt_render_camera"
    assert callable(g.PathTracer.render_model) and callable(g.PathTracer.render_camera)
    import inspect
    assert list(inspect.signature(g.PathTracer.render_model).parameters) == ["self", "cam", "model", "params", "out_ptr", "spp", "hdr", "n", "first_pixel", "pixels_ptr"]


def test_null_context_is_refused():
    lib = g._abi.ptmi()
    cam, cm, p = g.default_camera(37, 23), g.camera_model("fisheye", 37, 23), g.default_params(37, 23)
    assert lib.pt_render_camera(None, C.byref(cam), C.byref(cm), None, 4, 0, None, C.byref(p), 1, g._abi.RAYS_CLAMPED) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()
    assert lib.pt_render_camera(None, None, None, None, 0, 0, None, None, 0, 0) == -1   # before n == 0 and spp == 0


def test_the_family_is_a_translation_unit_of_its_own():
    mk = open(os.path.join(PKG, "Makefile")).read()
    objs = mk.split("OBJS =")[1].split("\n")[0]
    assert "csrc/pt_k_camera.o" in objs and "csrc/pt_k_rays.o" in objs and "csrc/pt_camera.o" in objs
    assert "csrc/pt_k_camera.o: csrc/pt_k_camera.hip $(KHDR)" in mk
    khdr = re.search(r"^KHDR = (.*)$", mk, re.M).group(1)
    assert "csrc/pt_rays_loop.h" in khdr and "csrc/pt_camera_model.h" in khdr, "the shared loop and the shared model arithmetic are dependencies"
    # the loop and the models' arithmetic exist once: both kernels of each pair come from the one header
    rays, camk, gen = (open(os.path.join(CSRC, f)).read() for f in ("pt_k_rays.hip", "pt_k_camera.hip", "pt_camera.hip"))
    assert "k_rays_loop<V, KRays>" in rays and "k_rays_loop<V, KCamRays>" in camk
    assert "trav_run_wide" not in rays + camk and "path_shade" not in rays + camk, "the loop body lives in pt_rays_loop.h alone"
    assert "pt_model_ray<MODEL>" in gen and "pt_model_ray_of(" in camk and "sincosf" not in gen + camk, "the models' arithmetic lives in pt_camera_model.h alone"


@pytest.mark.parametrize("san", ["", "SAN=1"], ids=["plain", "sanitized"])
def test_check_program_walks_the_calls_domain(san):
    exe = os.path.join(CSRC, "pt_variants_check")
    build = subprocess.run(["make", "-B", "-C", PKG, "variants_check"] + ([san] if san else []), capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    assert ("-fsanitize=address,undefined" in build.stdout) == bool(san), build.stdout
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout
    m = re.search(r"^camera family k_render_camera: requests=(\d+) words=(\d+) kernels=(\d+)$", run.stdout, re.M)
    assert m, run.stdout
    requests, words, kernels = map(int, m.groups())
    assert kernels == 19 and words == 19 and requests >= words
    rays = re.search(r"^k_render_rays\s+(\d+) requests,\s+(\d+) distinct words,\s+(\d+) kernels$", run.stdout, re.M)
    assert rays and int(rays.group(3)) == kernels, "one k_render_camera per k_render_rays"
