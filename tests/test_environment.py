"""pt_upload_environment / pt_eval_environment without a GPU: the declarations, the bindings, the NULL-context errors, the PFM reader,
pt_app --env's refusals, and the premise of the GPU round-trip test — the reference lookup (tests/env_ref.py) over the directions
`pt_app --equirect` renders returns the map texel by texel."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import env_ref

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
APP = os.path.join(ROOT, "g.p.u-pathtracer_amd", "host", "pt_app")


def test_header_declares_the_environment_calls():
    src = open(os.path.join(ROOT, "include", "ptmi.h")).read()
    assert re.search(r"int\s+pt_upload_environment\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_environment\s*\*\s*env,\s*const\s+float\s*\*\s*texels[^,)]*\)\s*;", src)
    assert re.search(r"int\s+pt_eval_environment\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+float\s*\*\s*rays_dev,\s*size_t\s+n_rays,\s*float\s*\*\s*radiance_dev[^,)]*\)\s*;", src)
    assert re.search(r"PT_ENV_NEAREST\s*=\s*0\s*,\s*PT_ENV_BILINEAR\s*=\s*1", src)
    body = re.search(r"typedef\s+struct\s+pt_environment\s*\{(.*?)\}\s*pt_environment\s*;", src, re.S)
    assert body
    fields = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", fields).strip() == "int32_t width, height; float front[3], right[3], up[3]; float scale[3]; int32_t filter; int32_t _pad;"
    assert re.search(r"#define\s+PTMI_ABI_VERSION\s+3\b", src)


def test_struct_mirror_is_64_bytes():
    E = g.Environment
    assert C.sizeof(E) == 64
    assert [(n, getattr(E, n).offset) for n, _ in E._fields_] == [("width", 0), ("height", 4), ("front", 8), ("right", 20), ("up", 32),
                                                                    ("scale", 44), ("filter", 56), ("_pad", 60)]


def test_abi_binds_the_environment_calls():
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_upload_environment"][2]) == 3 and len(rows["pt_eval_environment"][2]) == 4
    lib = g._abi.ptmi()
    assert lib.pt_eval_environment.argtypes[2] is C.c_size_t
    assert (g.ENV_NEAREST, g.ENV_BILINEAR) == (0, 1) == (g._abi.ENV_NEAREST, g._abi.ENV_BILINEAR)
    assert lib.pt_abi_version() == 3
    for name in ("upload_environment", "clear_environment", "eval_environment"):
        assert callable(getattr(g.PathTracer, name))
    hrows = {r[0] for r in g._abi.PTHOST_SYMBOLS}
    assert {"pth_read_pfm", "pth_free_pfm"} <= hrows and callable(g.read_pfm)


def test_null_context_is_refused():
    lib = g._abi.ptmi()
    ev = g.Environment()
    ev.width = ev.height = 1
    px = (C.c_float * 3)(1, 1, 1)
    assert lib.pt_upload_environment(None, C.byref(ev), px) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()
    assert lib.pt_upload_environment(None, None, None) == -1
    assert lib.pt_eval_environment(None, None, 4, None) == -1
    assert "null ctx" in lib.pt_last_error(None).decode()


# ---------------------------------------------------------------------------------------------------- PFM
def test_read_pfm_round_trips_bit_for_bit(tmp_path):
    rng = np.random.default_rng(1)
    a = rng.normal(size=(3, 5, 3)).astype(np.float32) * 100
    a[0, 0] = (np.float32(-0.0), np.float32(np.inf), np.float32(1e-42))   # signed zero, infinity, a subnormal: bits, not values
    path = str(tmp_path / "a.pfm")
    g.write_image(path, a)
    b = g.read_pfm(path)
    assert b.shape == (3, 5, 3) and b.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_read_pfm_reads_big_endian(tmp_path):
    rng = np.random.default_rng(2)
    a = rng.random((3, 5, 3)).astype(np.float32)
    path = tmp_path / "be.pfm"
    path.write_bytes(b"PF\n5 3\n1.0\n" + a.astype(">f4").tobytes())
    assert np.array_equal(g.read_pfm(str(path)).view(np.uint32), a.view(np.uint32))
    # the scale's size is ignored, its sign is the byte order
    path.write_bytes(b"PF\n5 3\n-2.5\n" + a.astype("<f4").tobytes())
    assert np.array_equal(g.read_pfm(str(path)).view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("blob", [b"Pf\n5 3\n-1.0\n" + bytes(60), b"PF\n5 3\n-1.0\n" + bytes(179), b"PF\n0 3\n-1.0\n", b"PF\n5 3\n0.0\n" + bytes(180), b""],
                         ids=["grey", "truncated", "zero-width", "zero-scale", "empty"])
def test_read_pfm_refuses_malformed_files(tmp_path, blob):
    path = tmp_path / "bad.pfm"
    path.write_bytes(blob)
    with pytest.raises(RuntimeError, match="PFM"):
        g.read_pfm(str(path))


# ---------------------------------------------------------------------------------------------------- pt_app
def test_pt_app_env_refusals(tmp_path):
    """A missing or malformed map, or a map option without --env, ends the run with the option's name before anything is rendered
    (or a device asked for: this runs without one)."""
    out = tmp_path / "x.png"
    base = [APP, "--mesh", os.path.join(ROOT, "assets", "cube.ptmesh"), "--width", "32", "--height", "16", "--frames", "1", "--out", str(out)]
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"PF\n4 2\n-1.0\n" + bytes(10))
    good = tmp_path / "good.pfm"
    good.write_bytes(b"PF\n4 2\n-1.0\n" + struct.pack("<24f", *([0.5] * 24)))
    cases = [(["--env", str(tmp_path / "none.pfm")], "--env:"), (["--env", str(bad)], "--env:"), (["--env-scale", "2"], "--env-scale"),
             (["--env-nearest"], "--env-nearest"), (["--env", str(good), "--env-scale", "-1"], "--env-scale"),
             (["--env", str(good), "--env-scale", "nan"], "--env-scale")]
    for extra, name in cases:
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and name in r.stderr, (extra, r.stderr[-300:])
        assert "mesh" not in r.stdout, (extra, r.stdout[-300:])   # refused before the scene was built
    assert not out.exists()


# ---------------------------------------------------------------------------------------------------- the reference's premise
@pytest.mark.parametrize("size", [(16, 8), (5, 3), (1, 1)], ids=["16x8", "5x3", "1x1"])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
def test_reference_lookup_over_the_equirect_directions_returns_the_grid(size, scale):
    """Nearest lookup along the direction of every pixel of a W x H latitude-longitude frame picks that pixel's texel: the lookup
    is the inverse of --equirect's ray generation, whatever the length of the direction."""
    W, H = size
    tex = np.arange(W * H * 3, dtype=np.float32).reshape(H, W, 3)
    d = env_ref.equirect_dirs(W, H) * np.float32(scale)
    fx, fy, valid = env_ref.positions(d, W, H)
    assert valid.all()
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    poles = (y.ravel() == 0)   # row 0 looks at the pole itself (latitude -pi/2): its longitude is only as good as cos(lat) ~ 6e-17 lets it be
    assert np.abs(fy - y.ravel()).max() < 1e-5
    err_x = np.abs(np.mod(fx - x.ravel() + W / 2.0, W) - W / 2.0)
    assert err_x[~poles].max(initial=0.0) < 1e-5 and err_x.max() < 0.25, (err_x[~poles].max(initial=0.0), err_x.max())
    assert np.array_equal(env_ref.nearest(tex, fx, fy, valid), tex.reshape(-1, 3))


def test_reference_bilinear_returns_a_constant_and_the_texels():
    """p + w * (q - p) returns p when q == p whatever w is, and an integer position returns its texel."""
    tex = np.full((3, 5, 3), np.float32(0.3), np.float32) * np.array([1, 2, 3], np.float32)
    d = env_ref.random_dirs(500)
    fx, fy, valid = env_ref.positions(d, 5, 3)
    for dt in (np.float32, np.float64):
        assert np.array_equal(env_ref.bilinear(tex, fx, fy, valid, dt).astype(np.float32), np.broadcast_to(tex[0, 0], (500, 3)))
    tex = env_ref.gradient_map(16, 8)
    x, y = np.meshgrid(np.arange(16.0), np.arange(8.0))
    assert np.array_equal(env_ref.bilinear(tex, x.ravel(), y.ravel()), tex.reshape(-1, 3).astype(np.float64))


def test_reference_invalid_directions_are_black():
    d = np.array([[np.nan, 0, 1], [0, np.inf, 0], [0, 0, 0], [-np.inf, 1, 1], [0, 0, 1]], np.float32)
    fx, fy, valid = env_ref.positions(d, 16, 8)
    assert valid.tolist() == [False, False, False, False, True]
    tex = env_ref.gradient_map(16, 8)
    assert not env_ref.nearest(tex, fx, fy, valid)[:4].any() and not env_ref.bilinear(tex, fx, fy, valid)[:4].any()


def test_share_of_random_directions_near_a_texel_border():
    """The GPU test sets aside the directions whose float64 fx + 0.5 or fy + 0.5 lies within 2^-10 of an integer and asserts that
    they are at most 1 %.  For uniform directions on a 16 x 8 map the expected share is about 4 x 2^-10 = 0.4 %: fx + 0.5 is uniform
    (2 x 2^-10 of every unit interval), fy + 0.5 is not quite (the latitude density is cos(lat)), but as near."""
    d = env_ref.random_dirs(4096)
    fx, fy, _ = env_ref.positions(d, 16, 8)
    near = (np.abs(fx + 0.5 - np.round(fx + 0.5)) <= 2.0 ** -10) | (np.abs(fy + 0.5 - np.round(fy + 0.5)) <= 2.0 ** -10)
    print(f"set aside: {near.sum()} of 4096 = {100.0 * near.mean():.2f} %")
    assert near.mean() <= 0.01
