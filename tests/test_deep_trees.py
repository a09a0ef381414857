"""The hand-built deep trees of tests/deep_trees.py, checked on the CPU: the stack model reaches the depth each fixture claims, brute
force sees one hit per blocked half-cell, and, where its 64-entry stack allows, the oracle's own walk over the hand-written Compact
arrays agrees with brute force bit for bit.  tests/test_gpu_deep_stack.py runs the same fixtures through the kernels."""
import math

import numpy as np
import pytest

import deep_trees as dt
import orc

DEPTHS = (15, 16, 17, 23, 24, 25, 33, 63, 65)


@pytest.fixture(scope="module")
def combs():
    return {D: dt.comb(D) for D in DEPTHS}


@pytest.mark.parametrize("D", DEPTHS)
def test_comb_reaches_its_depth(combs, D):
    """every ray of cell_rays pushes one entry per level of comb(D): the deepest stack index written is exactly D"""
    fx = combs[D]
    rays = dt.cell_rays(fx)
    assert len(rays) == 128
    depth = dt.binary_stack_depth(fx, rays)
    assert depth.min() == depth.max() == D
    assert fx.max_depth == D and fx.wide_depth == math.ceil(D / 3) and fx.n_tris == D + 1
    assert dt.oracle_may_walk(fx) == (D <= 63)


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("D", DEPTHS)
def test_brute_force_sees_one_hit_per_blocked_half(combs, D, cull):
    """stack depth D (the model's; brute force keeps no stack): leaf k's triangle is met by the ray through its half-cell alone,
    at the exact distance of its plane"""
    fx = combs[D]
    rays = dt.cell_rays(fx)
    t, tri, nrm = orc.trace_brute(fx.mesh, rays, cull)
    want = dt.expected_ids(fx, rays)
    assert np.array_equal(tri, want)
    assert sorted(tri[tri >= 0]) == list(range(D + 1))
    z = np.array([fx.targets[i][2] for i in tri[tri >= 0]])
    assert np.array_equal(t[tri >= 0], (fx.z_top + 1.0 - z).astype(np.float32))      # direction z = -1, unnormalised
    assert (nrm[tri >= 0] == (0.0, 0.0, 1.0)).all()


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("D", [D for D in DEPTHS if D <= 63])
def test_oracle_walk_equals_brute_force(combs, D, cull):
    """stack depth D <= 63, the oracle's last entry: its walk over the hand-written arrays gives brute force's t, id and normal"""
    fx = combs[D]
    rays = dt.cell_rays(fx)
    assert dt.oracle_may_walk(fx, rays)
    t, tri, nrm, cnt = orc.trace_bvh(fx, rays, cull)
    t0, tri0, nrm0 = orc.trace_brute(fx.mesh, rays, cull)
    assert np.array_equal(t.view(np.int32), t0.view(np.int32)) and np.array_equal(tri, tri0)
    assert np.array_equal(nrm[tri0 >= 0], nrm0[tri0 >= 0])
    assert cnt["inner"] == 128 * D            # every ray visits every node of the chain


def test_comb_with_mirror_is_one_level_deeper():
    """comb(D, mirror=True): stack depth D + 1 for rays from above (the root pushes the mirror leaf or the comb), tree depth D + 1,
    and a 4-wide tree whose root holds the mirror leaf and two comb leaves"""
    for D in (22, 30, 61):
        fx = dt.comb(D, mirror=True)
        rays = dt.cell_rays(fx)
        assert fx.max_depth == D + 1 and fx.n_tris == D + 3 and fx.wide_depth == 1 + math.ceil((D - 2) / 3)
        depth = dt.binary_stack_depth(fx, rays)
        assert depth.min() == depth.max() == D        # from below the mirror its box is behind the ray: the root pushes nothing
        t, tri, _, _ = orc.trace_bvh(fx, rays, True)
        t0, tri0, _ = orc.trace_brute(fx.mesh, rays, True)
        assert np.array_equal(tri, tri0) and np.array_equal(t.view(np.int32), t0.view(np.int32))
        assert np.array_equal(tri0, dt.expected_ids(fx, rays))


@pytest.mark.parametrize("W", [2, 5, 23, 24])
def test_stair_is_as_designed(W):
    """stair(W): W - 1 chain nodes, each with a four-leaf side tree: 4 W - 3 triangles, tree depth W + 1, a 4-wide tree of depth W
    (one binary chain level per wide level) and a binary stack depth of W"""
    fx = dt.stair(W)
    rays = dt.cell_rays(fx)
    assert fx.n_tris == 4 * W - 3 and fx.max_depth == W + 1 and fx.wide_depth == W
    depth = dt.binary_stack_depth(fx, rays)
    assert depth.min() == depth.max() == W
    t, tri, nrm, _ = orc.trace_bvh(fx, rays, True)
    t0, tri0, nrm0 = orc.trace_brute(fx.mesh, rays, True)
    assert np.array_equal(tri, tri0) and np.array_equal(t.view(np.int32), t0.view(np.int32))
    assert np.array_equal(tri0, dt.expected_ids(fx, rays)) and (tri0 >= 0).sum() == W
    assert np.array_equal(nrm[tri0 >= 0], nrm0[tri0 >= 0])


def test_morton_chain_mesh_chains():
    """the mesh for the device builders' depth limit: its sort keys lead with 63 different bits, so the linear BVH over them has
    an inner node 62 + log2(8) = 65 edges below the root, past the 64 levels the builders accept (deepest + 1 <= 64); with two equal keys
    instead of eight the deepest inner node is 63 edges down and its leaves 64: the deepest tree they take"""
    mesh = dt.morton_chain_mesh()
    keys = dt.morton_keys(mesh)
    assert mesh.n_tris == 3 * 18 + 9 + 3 + 8 == len(keys)
    assert len({k.bit_length() for k in keys}) == 64          # 63 leading positions, and 0
    assert keys.count(0) == 8
    assert dt.lbvh_depth(keys) == 65
    assert dt.lbvh_depth(dt.morton_keys(dt.morton_chain_mesh(2))) == 63
