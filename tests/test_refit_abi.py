"""CPU tests (no GPU) of pt_refit_bvh's surface: declared, bound, exported, argument checks before any device call, and the
triangle-soup rows the Python side hands it."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_refit_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_refit_bvh\(pt_ctx\* ctx, const float\* tri_verts_dev, size_t n_tris, uint32_t\* n_dropped_dev\);", hdr)
    assert "pt_refit_bvh" in {n for n, _, _ in g._abi.PTMI_SYMBOLS}
    assert hasattr(g._abi.ptmi(), "pt_refit_bvh")
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    assert re.search(r" T pt_refit_bvh$", out, re.M)
    assert g._abi.ptmi().pt_abi_version() == 3     # a new symbol is backward compatible


def test_refit_null_context_is_invalid():
    lib = g._abi.ptmi()
    assert lib.pt_refit_bvh(None, None, 0, None) == -1   # PT_ERR_INVALID, no crash
    assert b"null ctx" in lib.pt_last_error(None)


@pytest.mark.parametrize("name", ["bunny_low", "cornell_dragon"])
def test_triangle_soup_rows_are_the_triangles_by_id(name):
    mesh = g.scene_mesh(name)
    soup = mesh.triangle_soup()
    assert soup.dtype == np.float32 and soup.shape == (mesh.n_tris, 9) and soup.flags.c_contiguous
    ref = mesh.verts[mesh.tris].reshape(mesh.n_tris, 9)
    assert np.array_equal(soup.view(np.int32), ref.view(np.int32))   # bit for bit, row for row
