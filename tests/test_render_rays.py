"""pt_render_rays without a GPU: the declaration, the binding, the NULL-context error, the oracle-side premise the GPU tests rest
on (a camera's jittered rays, traced as a batch, are segment 0 of that camera's paths), and pt_app --equirect's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
from gpu_support import bvh_of, golden_camera

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")


def test_header_declares_render_rays():
    src = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int\s+pt_render_rays\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+float\s*\*\s*rays_dev,\s*size_t\s+n_rays,\s*uint64_t\s+first_index,"
                     r"\s*float\s*\*\s*radiance_dev,\s*const\s+pt_params\s*\*\s*params,\s*uint32_t\s+spp,\s*int\s+mode\s*\)\s*;", src)
    assert re.search(r"PT_RAYS_CLAMPED\s*=\s*0\s*,\s*PT_RAYS_HDR\s*=\s*1", src)
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src)


def test_abi_binds_render_rays():
    row = [r for r in g._abi.PTMI_SYMBOLS if r[0] == "pt_render_rays"]
    assert len(row) == 1 and len(row[0][2]) == 8
    lib = g._abi.ptmi()
    assert lib.pt_render_rays.argtypes[3] is C.c_uint64   # first_index is 64 bits wide
    assert (g._abi.RAYS_CLAMPED, g._abi.RAYS_HDR) == (0, 1)
    assert lib.pt_abi_version() == 3
    assert callable(g.PathTracer.render_rays)


def test_null_context_is_refused():
    lib = g._abi.ptmi()
    p = g.default_params(8, 8)
    assert lib.pt_render_rays(None, None, 4, 0, None, C.byref(p), 1, 0) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()


@pytest.mark.parametrize("frame", [0, 12])
def test_a_cameras_rays_are_segment_zero_of_its_paths(frame):
    """orc.primary_rays(cam, W, H, frame=f) are the jittered first segments of the samples with frame f: traced as a batch they
    give the (t, id) that orc.sample_pixels logs for segment 0 of every pixel."""
    W, H = 37, 23
    _, bvh = bvh_of("cornell")
    sph, cam, p = g.reference_spheres(), golden_camera(W, H), g.default_params(W, H)
    p.frame = frame
    t, tri, _, _ = orc.trace_bvh(bvh, orc.primary_rays(cam, W, H, frame=frame), cull=bool(p.cull_backfaces))
    pixels = [(x, y) for y in range(H) for x in range(W)]
    _, t_seg, id_seg = orc.sample_pixels(pixels, sph, cam, p, 1, bvh=bvh)
    assert np.array_equal(t.view(np.int32), t_seg[:, 0, 0].view(np.int32))
    assert np.array_equal(tri, id_seg[:, 0, 0])
    assert (tri >= 0).any() and (tri < 0).any()


def test_pt_app_equirect_refusals(tmp_path):
    """--equirect has no pinhole frame: the options that need one are refused before anything is loaded, by name."""
    base = [APP, "--mesh", os.path.join(ROOT, "assets", "cornell.ptmesh"), "--width", "160", "--height", "80", "--frames", "2",
            "--equirect", "--out", str(tmp_path / "x.png")]
    for extra in (["--denoise-out", str(tmp_path / "d.png")], ["--temporal-out", str(tmp_path / "t.png")],
                  ["--variance-out", str(tmp_path / "v.pfm")], ["--until-error", "0.1", "--max-frames", "16"], ["--gpus", "2"],
                  ["--checkpoint", str(tmp_path / "c.ckpt")], ["--resume", str(tmp_path / "none.ckpt")]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--equirect" in r.stderr, (extra, r.stderr[-300:])
    assert not (tmp_path / "x.png").exists()
