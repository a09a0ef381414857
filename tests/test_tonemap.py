"""The display stage without a GPU: pt_tonemap, pt_meter and pt_tonemap_thresholds in the header, the binding and the library, the
threshold tables against numpy's double evaluation, the numpy restatement (tests/tonemap_ref.py) against values worked out by hand,
the check program's walk over both calls' argument rules (csrc/pt_variants_check.cpp), and the oracle's committed frames: CLAMP +
LINEAR + exposure 1 over an oracle accumulator gives that frame's oracle display words."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import tonemap_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


def header():
    return open(os.path.join(ROOT, "include", "ptmi.h")).read()


def flat(text):
    return re.sub(r"\s+\*?\s*", " ", text)


# ---------------------------------------------------------------------------------------------------- the surface
def test_structs_constants_and_symbols():
    assert C.sizeof(g.TonemapParams) == 24 and C.sizeof(g.MeterParams) == 32
    assert [f for f, _ in g.TonemapParams._fields_] == ["width", "height", "curve", "transfer", "exposure", "white"]
    assert [f for f, _ in g.MeterParams._fields_] == ["width", "height", "key", "low_pct", "high_pct", "min_exposure", "max_exposure", "adapt"]
    assert (g.TONE_CLAMP, g.TONE_REINHARD, g.TONE_ACES) == (0, 1, 2) and (g.XFER_LINEAR, g.XFER_SRGB, g.XFER_GAMMA22) == (0, 1, 2)
    src = header()
    assert re.search(r"enum\s*\{\s*PT_TONE_CLAMP = 0, PT_TONE_REINHARD = 1, PT_TONE_ACES = 2\s*\};", src)
    assert re.search(r"enum\s*\{\s*PT_XFER_LINEAR = 0, PT_XFER_SRGB = 1, PT_XFER_GAMMA22 = 2\s*\};", src)
    rows = {r[0]: r for r in g._abi.PTMI_SYMBOLS}
    assert len(rows["pt_tonemap"][2]) == 6 and len(rows["pt_meter"][2]) == 5 and len(rows["pt_tonemap_thresholds"][2]) == 2
    lib = g._abi.ptmi()
    assert lib.pt_tonemap.argtypes[1]._type_ is g.TonemapParams and lib.pt_meter.argtypes[1]._type_ is g.MeterParams
    assert lib.pt_meter.argtypes[4] is C.c_int and lib.pt_tonemap.restype is C.c_int
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(CSRC, "libptmi.so")], capture_output=True, text=True)
    assert nm.returncode == 0
    for name in ("pt_tonemap", "pt_meter", "pt_tonemap_thresholds"):
        assert re.search(r"\bT %s$" % name, nm.stdout, re.M), f"libptmi.so does not export {name}"
    blob = open(os.path.join(CSRC, "libptmi.so"), "rb").read()
    for kernel in (b"k_tonemap", b"k_meter_hist", b"k_meter_finish"):
        assert kernel in blob, kernel
    assert list(inspect.signature(g.PathTracer.tonemap).parameters) == ["self", "color_ptr", "width", "height", "rgba_ptr", "out_ptr", "curve", "transfer",
                                                                       "exposure", "white", "exposure_ptr"]
    assert list(inspect.signature(g.PathTracer.meter).parameters) == ["self", "color_ptr", "width", "height", "state_ptr", "key", "low_pct", "high_pct",
                                                                     "min_exposure", "max_exposure", "adapt", "reset"]
    d = {k: v.default for k, v in inspect.signature(g.PathTracer.meter).parameters.items()}
    assert (d["key"], d["low_pct"], d["high_pct"], d["min_exposure"], d["max_exposure"], d["adapt"], d["reset"]) == (0.18, 0.0, 1.0, 2.0 ** -16, 2.0 ** 16, 1.0, False)
    d = {k: v.default for k, v in inspect.signature(g.PathTracer.tonemap).parameters.items()}
    assert (d["curve"], d["transfer"], d["exposure"], d["white"]) == (g.TONE_CLAMP, g.XFER_LINEAR, 1.0, float("inf"))
    assert callable(g.tone_thresholds)


def test_header_declares_the_calls_and_states_the_contract():
    src = header()
    assert re.search(r"int\s+pt_tonemap\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_tonemap_params\s*\*\s*tp,\s*const\s+float\s*\*\s*color_dev,"
                     r"\s*const\s+float\s*\*\s*exposure_dev(?:\s*/\*.*?\*/)?,\s*float\s*\*\s*out_dev(?:\s*/\*.*?\*/)?,\s*uint32_t\s*\*\s*rgba_dev(?:\s*/\*.*?\*/)?\)\s*;", src)
    assert re.search(r"int\s+pt_meter\s*\(\s*pt_ctx\s*\*\s*ctx,\s*const\s+pt_meter_params\s*\*\s*mp,\s*const\s+float\s*\*\s*color_dev,"
                     r"\s*float\s*\*\s*state_dev(?:\s*/\*.*?\*/)?,\s*int\s+reset\s*\)\s*;", src)
    assert re.search(r"int\s+pt_tonemap_thresholds\s*\(\s*int\s+transfer,\s*float\s*\*\s*out256\s*\)\s*;", src)
    text = flat(src[src.index("display: exposure metering and tone mapping, an EXTENSION (DESIGN.md §10 f19)"):src.index("int pt_tonemap_thresholds(")])
    for piece in ("x = x > 0 ? fminf(x, 65536.0f) : 0", "s = (1.0f + L * iw2) / (1.0f + L)", "a = x * (2.51f * x + 0.03f)", "b = x * (2.43f * x + 0.59f) + 0.14f",
                  "the number of k in 1..255 with y >= T[k]", "T[k] = eotf((k - 0.5) / 255)", "(127 - 16) << 3", "w_b = max(0, min(cum_b, hi) - max(cum_(b-1), lo))",
                  "Lavg = (float)ldexp(1.0 + (p - i), i)", "bin 107, Lavg = 0.1796875", "prev + (target - prev) * adapt", "no global atomics",
                  "Two launches", "No copy back, no synchronisation, no allocation after the first call", "out_dev may alias color_dev",
                  "Nothing is written by a refused call, the state included"):
        assert flat(piece) in text, piece
    # the errors, stated in one order
    tm = text[text.index("Errors, in this order"):]
    order = ["NULL ctx", "a NULL tp or color_dev, or out_dev and rgba_dev both NULL", "width or height < 1", "a curve or a transfer", "an exposure that is not finite",
             "a white that is not > 0"]
    at = [tm.index(p) for p in order]
    assert at == sorted(at)
    mt = tm[tm.index("Errors, in this order", 10):]
    order = ["NULL ctx", "a NULL mp, color_dev or state_dev", "width or height < 1", "a key that is not finite", "percentages outside", "exposure limits", "an adapt outside"]
    at = [mt.index(p) for p in order]
    assert at == sorted(at)


def test_null_context_and_the_host_only_call():
    lib = g._abi.ptmi()
    tp = g.TonemapParams(4, 4, g.TONE_CLAMP, g.XFER_LINEAR, 1.0, float("inf"))
    mp = g.MeterParams(4, 4, 0.18, 0.0, 1.0, 0.5, 2.0, 1.0)
    assert lib.pt_tonemap(None, C.byref(tp), None, None, None, None) == -1
    assert lib.pt_last_error(None) == b"null ctx"
    assert lib.pt_tonemap_thresholds(g.XFER_LINEAR, np.empty(256, F).ctypes.data) == -1
    assert b"PT_XFER_LINEAR has no table" in lib.pt_last_error(None)
    assert lib.pt_meter(None, C.byref(mp), None, None, 0) == -1
    assert lib.pt_last_error(None) == b"null ctx"
    assert lib.pt_tonemap_thresholds(g.XFER_SRGB, None) == -1 and lib.pt_tonemap_thresholds(7, np.empty(256, F).ctypes.data) == -1
    with pytest.raises(g.PtError):
        g.tone_thresholds(g.XFER_LINEAR)


@pytest.mark.parametrize("san", ["", "SAN=1"], ids=["plain", "sanitized"])
def test_check_program_walks_both_calls_rules(san):
    """The error order of pt_tonemap and pt_meter — every rule broken alone and together — and the launches of calls that pass."""
    src = open(os.path.join(CSRC, "pt_variants_check.cpp")).read()
    assert "check_tonemap_call(" in src and "check_meter_call(" in src and "plan_tonemap(" in src and "plan_meter(" in src
    den = open(os.path.join(CSRC, "pt_display.hip")).read()
    assert "check_tonemap_call(tp," in den and "check_meter_call(mp," in den, "the entry points ask the rules the check program runs"
    exe = os.path.join(CSRC, "pt_variants_check")
    build = subprocess.run(["make", "-B", "-C", PKG, "variants_check"] + ([san] if san else []), capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout


def test_kernels_use_no_transcendental_and_stage_the_table():
    den = open(os.path.join(CSRC, "pt_display.hip")).read()
    body = den[den.index("struct ToneArgs"):den.index("}  // namespace")]   # the device part: every kernel of the file
    assert "k_tonemap(const ToneArgs" in body and "k_meter_finish(const MeterArgs" in body
    assert "pt_pack_rgba(r, g, b)" in body, "LINEAR calls the pack of pt_render's words"
    assert "powf" not in body and "exp2" not in body and "log2" not in body and "fmaf" not in body
    assert "__shared__ float s_T[256]" in body and "pt_sld4(" in body and "make_uint4(" in body
    hist = body[body.index("k_meter_hist("):body.index("struct MeterArgs")]
    assert "atomicAdd(&s_h[" in hist and "atomicAdd(partial" not in hist and "atomicAdd(&partial" not in hist


# ---------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("transfer", [R.SRGB, R.GAMMA22], ids=["srgb", "gamma22"])
def test_thresholds(transfer):
    T = g.tone_thresholds(transfer)
    assert T.dtype == F and T.shape == (256,) and T[0] == 0.0
    assert np.all(np.diff(T.astype(np.float64)) > 0), "strictly increasing"
    want = R.thresholds64(transfer)
    ulp = np.spacing(np.abs(want).astype(F)).astype(np.float64)
    assert np.all(np.abs(T.astype(np.float64) - want) <= ulp), "within 1 ulp of numpy's double evaluation"
    gaps = np.diff(T[1:].view(np.int32).astype(np.int64))
    print(f"transfer {transfer}: differs from numpy's rounding at {int((T != R.thresholds(transfer)).sum())} entries; neighbouring entries at least {gaps.min()} ulps apart")
    assert gaps.min() > 1000
    # the count rule is round-to-nearest of the encoded value: floor(255 * oetf(y) + 0.5), away from the ties
    rng = np.random.default_rng(11)
    y = np.concatenate([rng.random(200000).astype(F), np.array([0.0, 1.0], F), np.exp2(rng.uniform(-20, 0, 50000)).astype(F)])
    enc = 255.0 * R.oetf(transfer, y.astype(np.float64))
    # rounding T[k] to binary32 moves it by at most 2^-24 of its value, which is at most 255 x 2^-24 < 2e-5 codes (the encodings' slopes in
    # log-log are <= 1): a y within 1e-4 codes of a tie may fall on either side of the rounded threshold and is left out
    clear = np.abs(enc - np.floor(enc) - 0.5) > 1e-4
    assert clear.mean() > 0.999
    assert np.array_equal(R.codes(T, y)[clear], np.floor(enc + 0.5).astype(np.uint32)[clear])
    assert R.codes(T, F(0.0)) == 0 and R.codes(T, F(1.0)) == 255 and R.codes(T, T[1]) == 1 and R.codes(T, np.nextafter(T[1], F(0))) == 0
    assert R.codes(T, T[255]) == 255 and R.codes(T, np.nextafter(T[255], F(0))) == 254


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def one(rgb, **kw):
    out, word = R.tonemap(np.array([rgb], F), **kw)
    return out[0], int(word[0])


def test_curves_by_hand():
    # CLAMP: 0, 1, the cap
    for curve in (R.CLAMP, R.REINHARD, R.ACES):
        y, w = one((0.0, 0.0, 0.0), curve=curve)
        assert np.array_equal(y, [0, 0, 0]) and w == 0, curve          # ACES: 0 / 0.14
    y, w = one((1.0, 0.5, 0.25))
    assert np.array_equal(y, F([1.0, 0.5, 0.25])) and w == (63 << 16) | (127 << 8) | 255
    y, w = one((1e30, 65536.0, 70000.0))
    assert np.array_equal(y, [1, 1, 1]) and w == 0x00FFFFFF
    # NaN, negative, infinite: 0, 0, the cap
    y, w = one((np.nan, -3.0, np.inf), exposure=0.5)
    assert np.array_equal(y, [0, 0, 1]) and w == 0x00FF0000
    y, _ = one((-np.inf, 1e-42, 0.5), exposure=2.0)                   # a denormal stays a positive value
    assert y[0] == 0 and y[1] == F(1e-42) * F(2.0) and y[2] == 1.0
    # exposure scales before the curve
    y, _ = one((0.25, 0.5, 2.0), exposure=0.5)
    assert np.array_equal(y, F([0.125, 0.25, 1.0]))
    # plain Reinhard on a grey 1: the luminance weights add up to 1 within an ulp, so y = x / (1 + L)
    L1 = (F(0.2126) * F(1) + F(0.7152) * F(1)) + F(0.0722) * F(1)
    y, _ = one((1.0, 1.0, 1.0), curve=R.REINHARD)
    assert np.array_equal(y, np.full(3, F(1) * (F(1) / (F(1) + L1)), F)) and abs(float(y[0]) - 0.5) < 1e-7
    # a pure green 3, white 2: L = 0.7152f * 3, s = (1 + L / 4) / (1 + L); red and blue stay 0: the hue is kept
    L = (F(0.2126) * F(0) + F(0.7152) * F(3)) + F(0.0722) * F(0)
    s = (F(1) + L * F(0.25)) / (F(1) + L)
    y, _ = one((0.0, 3.0, 0.0), curve=R.REINHARD, white=2.0)
    assert np.array_equal(y, F([0, min(F(3) * s, F(1)), 0])) and 0.9 < float(F(3) * s) < 1.5
    # white = 2 shows a grey 2 as white (s = (1 + L / 4) / (1 + L), 2 s = 1 within rounding), plain Reinhard as 2 / 3
    y, _ = one((2.0, 2.0, 2.0), curve=R.REINHARD, white=2.0)
    assert abs(float(y[0]) - 1.0) < 2e-7
    y, _ = one((2.0, 2.0, 2.0), curve=R.REINHARD)
    assert abs(float(y[0]) - 2.0 / 3.0) < 2e-7
    # at the cap: plain Reinhard L / (1 + L) stays below 1; ACES saturates
    y, w = one((np.inf, np.inf, np.inf), curve=R.REINHARD)
    Lc = (F(0.2126) * R.CAP + F(0.7152) * R.CAP) + F(0.0722) * R.CAP
    assert np.array_equal(y, np.full(3, np.fmin(R.CAP * (F(1) / (F(1) + Lc)), F(1)), F)) and 0.9999 < float(y[0]) <= 1.0
    y, w = one((65536.0, 1e9, np.inf), curve=R.ACES)
    assert np.array_equal(y, [1, 1, 1]) and w == 0x00FFFFFF
    # ACES at 1: a = 2.54, b = 3.16, stated in binary32
    a = F(1) * (F(2.51) * F(1) + F(0.03))
    b = F(1) * (F(2.43) * F(1) + F(0.59)) + F(0.14)
    y, _ = one((1.0, 1.0, 1.0), curve=R.ACES)
    assert np.array_equal(y, np.full(3, a / b, F)) and abs(float(y[0]) - 2.54 / 3.16) < 1e-6
    # ACES at 0.5: (0.5 * 1.285) / (0.5 * 1.805 + 0.14)
    y, _ = one((0.5, 0.5, 0.5), curve=R.ACES)
    assert abs(float(y[0]) - 0.6425 / 1.0425) < 1e-6


def test_transfer_words_by_hand():
    # sRGB: linear 0.5 encodes to 0.7354 -> 187.5..: code 188; linear 0.0031308 (the knee) encodes to 0.04045 -> 10.3: code 10
    y, w = one((0.5, 0.0031308, 1.0), transfer=R.SRGB)
    assert w == (255 << 16) | (10 << 8) | 188
    # gamma 2.2: 0.5^(1/2.2) = 0.7297 -> 186.08: code 186; 0.218 -> 0.5004 * 255 = 127.6: code 128
    y, w = one((0.5, 0.218, 0.0), transfer=R.GAMMA22)
    assert w == (0 << 16) | (128 << 8) | 186
    # the transfer does not touch out
    y2, _ = one((0.5, 0.218, 0.0))
    assert np.array_equal(y, y2)
    # LINEAR truncates: 0.999 -> 254, and the word is 0x00BBGGRR
    _, w = one((0.999, 0.0, 0.5))
    assert w == (127 << 16) | 254


def test_exposure_from_the_device_state():
    c = np.array([[0.25, 0.5, 1.0]], F)
    assert np.array_equal(R.curve_out(c, exposure=2.0, state0=0.25), c * F(0.5))
    for bad in (np.nan, 0.0, -1.0, np.inf, -np.inf):
        assert np.array_equal(R.curve_out(c, exposure=2.0, state0=bad), R.curve_out(c, exposure=2.0)), bad
    assert np.array_equal(R.curve_out(c, exposure=3e38, state0=3e38), R.curve_out(c, exposure=3e38))   # the product overflows


def test_meter_by_hand():
    grey = np.full((5, 7, 3), 0.18, F)
    assert set(R.bins(grey).reshape(-1)) == {107}
    s = R.meter(grey)
    assert s[2] == F(0.1796875) and s[3] == 35 and s[1] == F(0.18) / F(0.1796875) and s[0] == s[1]
    # the bins: eight per octave from 2^-16, from the float's own bits
    vals = np.array([2.0 ** -16, np.nextafter(F(2.0 ** -16), F(0)), 1.0, 1.125, np.nextafter(F(1.125), F(0)), 65535.0, 65536.0, 1e30], F)
    with np.errstate(all="ignore"):
        got = R.bins(np.stack([np.zeros_like(vals), vals / F(0.7152), np.zeros_like(vals)], -1))
    L = R.luminance(np.stack([np.zeros_like(vals), vals / F(0.7152), np.zeros_like(vals)], -1))
    want = [0 if L[0] >= F(2.0 ** -16) else 256, 256, None, None, None, 255, None, 255]
    for k, wnt in enumerate(want):
        if wnt is not None:
            assert got[k] == wnt, (k, got[k])
    assert R.bins(np.array([[1.0, 1.0, 1.0]], F))[0] in (127, 128)     # 1.0 is the edge of bin 128; the weights add up to 1 -+ an ulp
    assert R.bins(np.array([[np.nan, 1, 1], [np.inf, 0, 0], [-1, 0, 0], [0, 0, 0], [3e38, 3e38, 3e38]], F)).tolist() == [256, 256, 256, 256, 255]
    # a trimmed two-level image: 30 pixels of 2^-4 grey-ish (bin b0) and 10 pixels 64 x brighter (bin b0 + 48)
    dark, bright = F(0.07), F(0.07 * 64)
    img = np.concatenate([np.full((30, 3), dark, F), np.full((10, 3), bright, F)])
    b0 = int(R.bins(img[:1])[0])
    assert int(R.bins(img[-1:])[0]) == b0 + 48
    full = R.meter(img)
    p = (30 * (2 * b0 + 1) + 10 * (2 * (b0 + 48) + 1)) / (16.0 * 40) - 16.0
    assert full[3] == 40 and full[2] == F(np.ldexp(1.0 + (p - np.floor(p)), int(np.floor(p))))
    # keep the shares 0.5 .. 1.0: lo = 20, hi = 40 -> 10 dark pixels and the 10 bright ones
    half = R.meter(img, low_pct=0.5, high_pct=1.0)
    p = (10 * (2 * b0 + 1) + 10 * (2 * (b0 + 48) + 1)) / (16.0 * 20) - 16.0
    assert half[3] == 20 and half[2] == F(np.ldexp(1.0 + (p - np.floor(p)), int(np.floor(p))))
    # keep 0 .. 0.75: only dark pixels, the centre of their bin
    low = R.meter(img, high_pct=0.75)
    assert low[3] == 30 and low[2] == F(np.ldexp(1.0 + ((2 * b0 + 1) / 16.0 - np.floor((2 * b0 + 1) / 16.0)), int(np.floor((2 * b0 + 1) / 16.0)) - 16))
    # percentages that leave nothing (hi <= lo after the truncation): everything is metered
    tiny = R.meter(img[:3], low_pct=0.1, high_pct=0.2)
    assert tiny[3] == 3
    # the clamp of the target
    assert R.meter(grey, min_exposure=2.0, max_exposure=4.0)[1] == 2.0 and R.meter(grey, min_exposure=0.25, max_exposure=0.5)[1] == 0.5


def test_meter_black_image_and_adaptation():
    black = np.zeros((4, 4, 3), F)
    s = R.meter(black)
    assert s.tolist() == [1.0, 1.0, 0.0, 0.0]                         # no state: 1
    s = R.meter(black, state=[3.0, 9.0, 9.0, 9.0], adapt=0.5)
    assert s.tolist() == [3.0, 3.0, 0.0, 0.0]                         # the exposure in use stays
    s = R.meter(black, state=[3.0, 0, 0, 0], max_exposure=2.0, reset=True)
    assert s.tolist() == [2.0, 2.0, 0.0, 0.0]                         # ... clamped alike
    for bad in (np.nan, 0.0, -2.0, np.inf):
        assert R.meter(black, state=[bad, 0, 0, 0]).tolist() == [1.0, 1.0, 0.0, 0.0]
    # three frames with adapt = 0.25 towards a grey whose target is 4 (Lavg of 0.045 is 0.044921875 = key 0.1796875 / 4), from exposure 1
    grey = np.full((3, 3, 3), 0.045, F)
    assert R.meter(grey)[2] == F(0.044921875)
    st = np.array([1.0, 0, 0, 0], F)
    seen = []
    for _ in range(3):
        st = R.meter(grey, state=st, key=0.1796875, adapt=0.25)
        seen.append(float(st[0]))
        assert st[1] == 4.0
    assert seen == [1.75, 2.3125, 2.734375]
    st = R.meter(grey, state=st, key=0.1796875, adapt=0.25, reset=True)
    assert st[0] == 4.0
    # an invalid exposure in use jumps, whatever adapt says
    assert R.meter(grey, state=[np.nan, 0, 0, 0], key=0.1796875, adapt=0.25)[0] == 4.0
    assert R.meter(grey, state=[0.0, 0, 0, 0], key=0.1796875, adapt=0.0)[0] == 4.0
    assert R.meter(grey, state=[2.0, 0, 0, 0], key=0.1796875, adapt=0.0)[0] == 2.0


def test_inputs_cover_the_edges():
    img = R.hdr_image(300, 220, 5)
    flat_img = img.reshape(-1, 3)
    grey = flat_img[(flat_img[:, 0] == flat_img[:, 1]) & (flat_img[:, 1] == flat_img[:, 2])][:, 0]
    for tr in (R.SRGB, R.GAMMA22):
        assert np.isin(R.neighbours(R.thresholds(tr)), grey).all()
    L = R.luminance(flat_img)
    e = R.bin_edges()
    print(f"bin edges and lower neighbours met exactly by a pixel's luminance: {int(np.isin(e, L).sum())} of {len(e)}")
    assert np.isin(e, L).mean() > 0.9
    assert np.isnan(flat_img).any() and np.isposinf(flat_img).any() and np.isneginf(flat_img).any() and (flat_img == F(1e-42)).any() and (flat_img < 0).any()
    b = R.bins(img)
    assert len(np.unique(b)) == 257, "every bin and the unmetered count are met"


# ---------------------------------------------------------------------------------------------------- the oracle's frames
@pytest.mark.parametrize("name", ["diff_1", "diff_16", "metal_4", "spec_4", "refr_16"])
def test_clamp_linear_gives_the_oracle_display_words(name):
    z = np.load(os.path.join(GOLD, "oracle_images.npz"))
    acc, rgba = z[name], z[name + "_rgba"]
    out, words = R.tonemap(acc, curve=R.CLAMP, transfer=R.LINEAR, exposure=1.0)
    assert np.array_equal(words, rgba)
    assert np.array_equal(out, acc), "the oracle's accumulator is clamped already"
    assert len(np.unique(rgba)) > 100
