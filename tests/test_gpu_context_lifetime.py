"""A context owns its device buffers, events and streams by type (csrc/pt_own.h): what a caller can see of that.
pt_destroy with work in flight on every stream the context has, contexts created and destroyed in a row and side by side, and a
material table replaced, cleared and put back.  Valid use only.  The scenes are the 32-triangle cornell with the reference spheres,
cube, and — where the cornell_box table's emissive rows must name triangles of the tree — cornell_box, as in
call_sequences.DIRECTED["lights"]."""
import numpy as np
import pytest

import gpu_pathtracer_amd as g
from gpu_support import bits, bvh_of, dark_table, golden_camera
from scene_matrix import make_camera

pytestmark = pytest.mark.gpu

NEE = g.FLAGS_SMALLPT | g.FLAG_NEE


def params(W, H, flags, first=1, depth=4):
    p = g.default_params(W, H, depth=depth)
    p.flags = flags | g.FLAG_WRITE_RGBA
    p.frame, p.sample_index = 6 + first, first
    return p


def frame(t, W, H, spp, flags, depth=4, cam=None):
    """One call into a fresh accumulator: its words."""
    acc, rgba = t.alloc_frame(W, H)
    try:
        t.launch_kernel(acc.ptr, rgba.ptr, cam or golden_camera(W, H), params(W, H, flags, depth=depth), spp)
        t.sync()
        return bits(acc.download(np.float32, (H, W, 3)))
    finally:
        acc.free()
        rgba.free()


def destroy(t):
    """pt_destroy's own return code (PathTracer.close drops it)."""
    if getattr(t, "_refit_buf", None) is not None:
        t._refit_buf.free()
        t._refit_buf = None
    rc = t._lib.pt_destroy(t._ctx)
    t._ctx = None
    return rc


def cornell(t, build=False):
    mesh, bvh = bvh_of("cornell")
    if build:
        t.build_bvh(mesh)
    else:
        t.upload_bvh(bvh)
    t.upload_spheres(g.reference_spheres())


# ---------------------------------------------------------------------------------------------- 1. destroyed with work in flight
def test_close_with_work_in_flight():
    import torch
    dev = torch.device("cuda", 0)
    W, H = 96, 64
    # the caller's buffers are torch's: they outlive the context, and no pt_free (which waits for the stream) stands before pt_destroy
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    rgba = torch.zeros((H, W), dtype=torch.int32, device=dev)
    guides = [torch.zeros((H, W, 4), dtype=torch.float32, device=dev) for _ in range(3)]
    ids = torch.zeros((H, W), dtype=torch.int32, device=dev)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()   # (the context's own stream does not wait for torch's)
    cam = golden_camera(W, H)
    t = g.PathTracer(0)
    try:
        t.set_option(g.OPT_KERNEL, g.KERNEL_PERSISTENT)
        t.set_option(g.OPT_OVERLAP, 1)
        cornell(t)
        first = 1
        for spp in (16, 4, 16, 4):   # in line on the idle stream, side slot 0, side slot 1, slot 0 again behind its pending fold
            t.launch_kernel(acc.data_ptr(), rgba.data_ptr(), cam, params(W, H, 0, first), spp)
            first += spp
        t.set_option(g.OPT_KERNEL, g.KERNEL_WAVEFRONT)   # the path records
        t.launch_kernel(acc.data_ptr(), rgba.data_ptr(), cam, params(W, H, 0, first), 16)
        t.render_aux(cam, params(W, H, 0), guides[0].data_ptr(), guides[1].data_ptr(), guides[2].data_ptr(), ids.data_ptr())
        t.denoise(acc.data_ptr(), guides[0].data_ptr(), guides[1].data_ptr(), guides[2].data_ptr(), W, H, out.data_ptr(), iterations=2)
        assert destroy(t) == 0   # no sync in front
    finally:
        t.close()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and float(out.abs().sum()) > 0   # the queued work ran to its end
    after = []
    for _ in range(2):
        f = g.PathTracer(0)
        try:
            cornell(f)
            after.append(frame(f, 37, 23, 4, 0))
        finally:
            f.close()
    assert after[0].any() and np.array_equal(after[0], after[1])


# ---------------------------------------------------------------------------------------------- 2. created and destroyed in a row
def env_5x3():
    tex = np.random.default_rng(503).uniform(0.05, 1.0, (3, 5, 3)).astype(np.float32)
    tex[1, 3] = (90.0, 80.0, 60.0)
    return tex


def test_create_destroy_cycles():
    mesh, _ = bvh_of("cornell")
    box = g.scene_mesh("cornell_box")   # its table covers cornell's 32 ids too
    frames = []
    for k in range(12):
        t = g.PathTracer(0)
        try:
            if k % 2:   # every resource a context can hold; even ones hold what pt_create made
                cornell(t, build=(k // 2) % 2 == 1)
                t.upload_tri_materials(box.materials, box.tri_material)
                t.upload_environment(env_5x3(), filter=g.ENV_NEAREST, light=True)
                assert t.environment_is_light()
                t.refit_bvh(mesh.triangle_soup())
                frames.append(frame(t, 8, 8, 4, 0, depth=2))   # PT_KERNEL_AUTO, the default
            assert destroy(t) == 0
        finally:
            t.close()
    assert len(frames) == 6 and frames[0].any()
    assert np.array_equal(frames[-1], frames[0])

    # the cube from outside, as call_sequences.camera_of looks at a mesh (the golden camera stands inside it); a miss returns bk_color
    cube = g.scene_mesh("cube")
    lo, hi = cube.bounds()
    off = np.array([0.35, 0.25, 1.4])
    outside = make_camera(8, 8, pos=tuple(0.5 * (lo + hi) + off * float(np.max(hi - lo))), front=tuple(-off))

    def pair(reverse):
        a, b = g.PathTracer(0), g.PathTracer(0)
        try:
            cornell(a)
            b.build_bvh(cube)
            got = frame(a, 8, 8, 4, 0), frame(b, 8, 8, 4, g.FLAG_MISS_KEEPS_PATH, cam=outside)
            for t in ((b, a) if reverse else (a, b)):
                assert destroy(t) == 0
            return got
        finally:
            a.close()
            b.close()

    in_order, reversed_ = pair(False), pair(True)
    assert in_order[0].any() and in_order[1].any()
    assert np.array_equal(in_order[0], reversed_[0]) and np.array_equal(in_order[1], reversed_[1])


# ---------------------------------------------------------------------------------------------- 3. a table replaced, cleared, put back
def test_replaced_materials_leave_nothing_behind():
    mesh, bvh = bvh_of("cornell_box")
    tables = {"cornell_box": (mesh.materials, mesh.tri_material), "dark": dark_table(mesh), None: (None, None)}
    history = (("cornell_box", NEE), (None, g.FLAGS_SMALLPT), ("dark", NEE), ("cornell_box", NEE))

    def scene(t):
        t.upload_bvh(bvh)
        t.upload_spheres(g.reference_spheres())

    got = []
    t = g.PathTracer(0)
    try:
        scene(t)
        for table, flags in history:
            t.upload_tri_materials(*tables[table])
            got.append(frame(t, 37, 23, 4, flags))
    finally:
        t.close()
    for (table, flags), have in zip(history, got):
        f = g.PathTracer(0)
        try:
            scene(f)
            if table is not None:
                f.upload_tri_materials(*tables[table])
            want = frame(f, 37, 23, 4, flags)
        finally:
            f.close()
        assert want.any()
        assert np.array_equal(have, want), f"table {table!r}: the long-lived context differs from a fresh one"
    assert np.array_equal(got[0], got[3])
    assert not np.array_equal(got[0], got[2])   # (the emitter is seen: the dark table's frame is another)
