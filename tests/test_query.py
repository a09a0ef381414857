"""CPU tests (no GPU) of pt_closest_hits / pt_any_hits' surface — declared, bound, exported, the NULL-context answer, the kernel in
the code object — and of the reference the GPU tests compare with (tests/query_ref.py): on the GPU tests' scenes its inputs meet
the conditions those tests state."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import orc
import query_ref as qr

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PT_ERR_INVALID = -1


def test_queries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int pt_closest_hits\(pt_ctx\* ctx, const float\* rays_dev, size_t n_rays, int cull_backfaces,\s*"
                     r"float\* t_dev, int32_t\* tri_dev, float\* normal_dev\);", hdr)
    assert re.search(r"int pt_any_hits\(pt_ctx\* ctx, const float\* rays_dev, size_t n_rays, int cull_backfaces,\s*uint8_t\* hit_dev\);", hdr)
    bound = {n: (r, a) for n, r, a in g._abi.PTMI_SYMBOLS}
    assert len(bound["pt_closest_hits"][1]) == 7 and len(bound["pt_any_hits"][1]) == 5
    lib = g._abi.ptmi()
    out = subprocess.check_output(["nm", "-D", "--defined-only", g._abi.PTMI_PATH]).decode()
    for name in ("pt_closest_hits", "pt_any_hits"):
        assert hasattr(lib, name)
        assert re.search(rf" T {name}$", out, re.M)
    assert hasattr(g.PathTracer, "closest_hits") and hasattr(g.PathTracer, "any_hits")
    assert lib.pt_abi_version() == 3     # new symbols are backward compatible


def test_null_context_is_invalid():
    lib = g._abi.ptmi()
    assert lib.pt_closest_hits(None, None, 0, 1, None, None, None) == PT_ERR_INVALID   # no crash
    assert b"null ctx" in lib.pt_last_error(None)
    assert lib.pt_any_hits(None, None, 5, 0, None) == PT_ERR_INVALID
    assert b"null ctx" in lib.pt_last_error(None)


def test_query_kernel_is_in_the_code_object():
    blob = open(g._abi.PTMI_PATH, "rb").read()
    assert b"k_query_rays" in blob and b"k_query_rays_bvh2" in blob
    assert b"k_trace_rays_bvh2" in blob


def test_class_bounds_by_hand():
    t = np.array([2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, qr.FLT_MAX], np.float32)
    tm, cls = qr.class_bounds(t, 10.0)
    assert list(cls) == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert tm[0] == 1.0 and tm[1] == 3.0 and tm[2] == np.nextafter(np.float32(4.0), np.float32(np.inf)) and tm[3] == 10.0
    assert np.isinf(tm[4]) and tm[5] == 0.0 and tm[6] == -1.0 and np.isnan(tm[7]) and tm[8] == 5.0
    tri = np.arange(9, dtype=np.int32)
    tri[8] = -1
    nrm = np.ones((9, 3), np.float32)
    rt, ri, rn, ra = qr.filter_by_bound((t, tri, nrm), tm)
    assert list(ra) == [False, False, True, True, True, False, False, False, False]
    assert list(ri) == [-1, -1, 2, 3, 4, -1, -1, -1, -1]
    assert np.array_equal(rt[ra], t[ra]) and np.all(rt[~ra] == qr.FLT_MAX) and not rn[~ra].any() and rn[ra].all()


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("name", ["cornell", "bunny_low"])
def test_reference_inputs_meet_the_gpu_tests_conditions(name, cull):
    """20 000 rays, seed 5: the tree walk of the CPU restatement equals brute force on every ray (so no ray of the GPU tests is one
    on which the references themselves disagree), most rays hit, and the eight classes exercise both answers."""
    mesh, rays, cls, b, (rt, ri, rn, ra) = qr.case(name, 20000, 5, cull)
    t1, i1, n1, _ = orc.trace_bvh(g.Bvh(mesh), rays, cull)
    assert np.array_equal(t1.view(np.int32), b[0].view(np.int32)) and np.array_equal(i1, b[1])
    assert np.array_equal(n1[b[1] >= 0], b[2][b[1] >= 0])
    hit, occ, bad = qr.shares(cls, b[1], ra)
    print(f"{name} cull {cull}: hit share {hit:.3f}, occluded share {occ:.3f}")
    assert not bad, bad
    # the shares as stated for these inputs, to the two decimals they are stated with: hit 0.55 to 0.99, occluded 0.20 to 0.37
    # (cornell without culling: 0.9936 of the rays hit)
    assert 0.55 <= round(hit, 2) <= 0.99
    assert 0.20 <= round(occ, 2) <= 0.37
    assert np.array_equal(ri >= 0, ra) and np.all(rt[~ra] == qr.FLT_MAX)
