"""The display stage on the GPU (extension; contract in include/ptmi.h): pt_tonemap and pt_meter, bit for bit
against tests/tonemap_ref.py throughout.

Every buffer a test hands in lies between canaries that must stay untouched, and may start 4, 8 or 12 bytes past a 16-byte boundary:
then the one-pixel-per-thread route runs instead of the four-pixel one.  37 x 23 = 851 pixels are a multiple of neither 4 nor 256;
300 x 220 = 66000 pixels are more than the meter's whole grid of 256 blocks x 256 threads, so a thread strides twice; 64 x 4 is
aligned.  The images are tonemap_ref.hdr_image's: HDR values over 2^-20 .. 2^20, the special values, every threshold of both tables
and every meter bin edge with their neighbours."""
import ctypes as C

import numpy as np
import pytest

import gpu_pathtracer_amd as g
import tonemap_ref as R
from gpu_support import golden_camera, setup_scene

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1
PAD = 32          # canary bytes in front of and behind every buffer
CANARY = 0xAB
# (curve, exposure, white): exposure 1 under CLAMP, so that the thresholds in the images reach the search as they are
CURVES = [(R.CLAMP, 1.0, np.inf), (R.REINHARD, 2.5, 4.0), (R.ACES, 0.37, np.inf)]
TRANSFERS = [R.LINEAR, R.SRGB, R.GAMMA22]
_tables = {}


def table(transfer):
    """The library's own table (tests/test_tonemap.py holds it to numpy's), fetched once."""
    if transfer != R.LINEAR and transfer not in _tables:
        _tables[transfer] = g.tone_thresholds(transfer)
    return _tables.get(transfer)


_images = {}


def image(W, H, seed=3):
    if (W, H, seed) not in _images:
        img = R.hdr_image(W, H, seed)
        img.setflags(write=False)
        _images[(W, H, seed)] = img
    return _images[(W, H, seed)]


@pytest.fixture(scope="module")
def t():
    tr = g.PathTracer(0)
    yield tr
    tr.close()


class Buf:
    """`nbytes` of device memory `off` bytes past a 16-byte boundary, between canaries; data: what it holds at first (else canaries)."""

    def __init__(self, t, nbytes, off=0, data=None):
        self.t, self.nbytes, self.off = t, nbytes, off
        self.dev = t.malloc(PAD + 16 + nbytes + PAD)
        assert self.dev.ptr % 16 == 0
        self.start = PAD + off
        self.ptr = self.dev.ptr + self.start
        self.host = np.full(self.dev.nbytes, CANARY, np.uint8)
        if data is not None:
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert raw.nbytes == nbytes
            self.host[self.start:self.start + nbytes] = raw
        self.dev.upload(self.host)

    def get(self, dtype, shape):
        """The contents; asserts the canaries on both sides."""
        got = self.dev.download(np.uint8, (self.dev.nbytes,))
        assert np.all(got[:self.start] == CANARY) and np.all(got[self.start + self.nbytes:] == CANARY), "written outside the buffer"
        return got[self.start:self.start + self.nbytes].copy().view(dtype).reshape(shape)

    def free(self):
        self.dev.free()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_tonemap(t, img, mode, offs=(0, 0, 0), **kw):
    """pt_tonemap over img [H][W][3] with out_dev alone ("out"), rgba_dev alone ("rgba"), both ("both") or out_dev == color_dev
    ("alias", with the words): (out or None, rgba or None, the colour buffer afterwards)."""
    H, W = img.shape[:2]
    col = Buf(t, img.nbytes, offs[0], img)
    out = Buf(t, img.nbytes, offs[1]) if mode in ("out", "both") else None
    rgba = Buf(t, 4 * W * H, offs[2]) if mode != "out" else None
    t.tonemap(col.ptr, W, H, rgba_ptr=rgba.ptr if rgba else None, out_ptr=col.ptr if mode == "alias" else out.ptr if out else None, **kw)
    t.sync()
    res = (out.get(F, img.shape) if out else None, rgba.get(np.uint32, (H, W)) if rgba else None, col.get(F, img.shape))
    for b in (col, out, rgba):
        if b:
            b.free()
    return res


def check_all_pairs(t, img, offs=(0, 0, 0), modes=("out", "rgba", "both", "alias")):
    for curve, exposure, white in CURVES:
        want_out = R.curve_out(img, curve, exposure, white)
        for transfer in TRANSFERS:
            want_rgba = R.words(want_out, transfer, table(transfer))
            for mode in modes:
                out, rgba, col = run_tonemap(t, img, mode, offs, curve=curve, transfer=transfer, exposure=exposure, white=white)
                what = f"curve {curve} transfer {transfer} {mode} offsets {offs}"
                if out is not None:
                    assert same_bits(out, want_out), what
                if rgba is not None:
                    bad = np.argwhere(rgba != want_rgba)
                    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: {int(rgba[tuple(bad[0])]):#x} vs {int(want_rgba[tuple(bad[0])]):#x}"
                assert same_bits(col, want_out if mode == "alias" else img), f"{what}: the colour buffer"


# ---------------------------------------------------------------------------------------------------- 1: pt_tonemap against the reference
@pytest.mark.parametrize("W,H", [(37, 23), (257, 1), (300, 220)])
def test_tonemap_all_pairs(t, W, H):
    check_all_pairs(t, image(W, H))


def test_tonemap_single_pixels(t):
    for rgb in ((0, 0, 0), (0.3, 2.0, 0.01), (np.nan, np.inf, -1.0), (1e-42, 65536.0, 1.0), (0.18, 0.18, 0.18)):
        check_all_pairs(t, np.array([[rgb]], F), modes=("both", "alias"))


@pytest.mark.parametrize("offs", [(0, 0, 0), (12, 12, 12), (0, 0, 4), (0, 8, 0), (4, 0, 0)], ids=lambda o: "+".join(map(str, o)))
def test_tonemap_aligned_and_offset_bases(t, offs):
    """64 x 4: the four-pixel route from aligned bases, the one-pixel route as soon as one buffer given is not 16-byte aligned."""
    check_all_pairs(t, image(64, 4), offs, modes=("both", "alias", "rgba") if offs == (0, 0, 0) or offs == (12, 12, 12) else ("both",))


def test_tonemap_plain_reinhard_and_defaults(t):
    img = image(37, 23)
    out, rgba, _ = run_tonemap(t, img, "both", curve=g.TONE_REINHARD, transfer=g.XFER_SRGB, exposure=0.5)   # white: +inf
    want = R.curve_out(img, R.REINHARD, 0.5, np.inf)
    assert same_bits(out, want) and np.array_equal(rgba, R.words(want, R.SRGB, table(R.SRGB)))
    out, rgba, _ = run_tonemap(t, img, "both")                                                                  # CLAMP, LINEAR, 1
    want = R.curve_out(img)
    assert same_bits(out, want) and np.array_equal(rgba, R.words(want))


def test_tonemap_of_a_rendered_accumulator_gives_pt_renders_words():
    W, H = 64, 36
    tr = g.PathTracer(0)
    try:
        setup_scene(tr, "room", False)
        p = g.default_params(W, H, depth=4)
        p.flags = g.FLAG_WRITE_RGBA
        acc, rgba = tr.alloc_frame(W, H)
        tr.launch_kernel(acc.ptr, rgba.ptr, golden_camera(W, H), p, 3)
        words = tr.malloc(4 * W * H)
        tr.tonemap(acc.ptr, W, H, rgba_ptr=words.ptr)   # no sync in between: the same stream
        tr.sync()
        a, want, got = acc.download(F, (H, W, 3)), rgba.download(np.uint32, (H, W)), words.download(np.uint32, (H, W))
        assert np.array_equal(got, want) and len(np.unique(want)) > 100
        assert np.array_equal(got, R.tonemap(a)[1])
        for b in (acc, rgba, words):
            b.free()
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------- 2: pt_meter against the reference
def run_meter(t, img, state=None, off=0, **kw):
    H, W = img.shape[:2]
    col = Buf(t, img.nbytes, off, img)
    st = Buf(t, 16, 0, np.zeros(4, F) if state is None else np.asarray(state, F))
    t.meter(col.ptr, W, H, st.ptr, **kw)
    t.sync()
    got = st.get(F, (4,))
    assert same_bits(col.get(F, img.shape), img)
    col.free()
    st.free()
    return got


@pytest.mark.parametrize("W,H,off", [(37, 23, 0), (1, 1, 0), (257, 1, 0), (300, 220, 0), (300, 220, 12), (64, 4, 0), (64, 4, 12)])
def test_meter_state(t, W, H, off):
    img = image(W, H) if (W, H) != (1, 1) else np.array([[[0.3, 2.0, 0.01]]], F)
    for kw in (dict(), dict(low_pct=0.1, high_pct=0.9), dict(low_pct=0.5, high_pct=1.0, key=0.5), dict(low_pct=0.0, high_pct=0.3, min_exposure=0.5, max_exposure=8.0),
               dict(low_pct=0.999, high_pct=0.9995)):
        got, want = run_meter(t, img, off=off, **kw), R.meter(img, **kw)
        assert same_bits(got, want), f"{kw}: {got.tolist()} vs {want.tolist()}"
    if (W, H) == (300, 220):
        h, unmetered = R.histogram(img)
        assert np.all(h > 0) and unmetered > 0 and R.meter(img)[3] == h.sum()


def test_meter_grey_black_and_invalid_states(t):
    grey = np.full((5, 8, 3), 0.18, F)
    got = run_meter(t, grey)
    assert got[2] == F(0.1796875) and got[3] == 40 and same_bits(got, R.meter(grey))
    black = np.zeros((23, 37, 3), F)
    for state in ([0, 0, 0, 0], [3.0, 9, 9, 9], [np.nan, 0, 0, 0], [-1.0, 0, 0, 0], [np.inf, 0, 0, 0]):
        for kw in (dict(), dict(reset=True, max_exposure=2.0), dict(adapt=0.5)):
            got, want = run_meter(t, black, state, **kw), R.meter(black, state, **kw)
            assert same_bits(got, want), (state, kw, got.tolist(), want.tolist())
    img = image(37, 23)
    for bad in (np.nan, 0.0, -2.0, np.inf, -np.inf):        # an invalid exposure in use: the target, whatever adapt says
        got = run_meter(t, img, [bad, 1, 2, 3], adapt=0.25)
        assert same_bits(got, R.meter(img, [bad, 1, 2, 3], adapt=0.25)) and got[0] == got[1]


def test_meter_adapts_over_three_frames_then_resets(t):
    W, H = 37, 23
    frames = [image(W, H, seed) * F(scale) for seed, scale in ((3, 1.0), (4, 8.0), (5, 0.05))]
    st = Buf(t, 16, 0, np.array([1.0, 0, 0, 0], F))
    want = np.array([1.0, 0, 0, 0], F)
    cols = [Buf(t, f.nbytes, 0, f) for f in frames]
    seen = []
    for k in range(3):
        t.meter(cols[k].ptr, W, H, st.ptr, adapt=0.25, low_pct=0.05, high_pct=0.95)
        want = R.meter(frames[k], want, adapt=0.25, low_pct=0.05, high_pct=0.95)
        t.sync()
        got = st.get(F, (4,))
        assert same_bits(got, want), (k, got.tolist(), want.tolist())
        assert got[0] != got[1], "the exposure in use moves only part of the way to the target"
        seen.append(float(got[0]))
    assert len(set(seen)) == 3
    t.meter(cols[0].ptr, W, H, st.ptr, adapt=0.25, reset=True)
    t.sync()
    got, want = st.get(F, (4,)), R.meter(frames[0], want, adapt=0.25, reset=True)
    assert same_bits(got, want) and got[0] == got[1]
    for b in cols + [st]:
        b.free()


# ---------------------------------------------------------------------------------------------------- 3: the chain
def chain(t, img, state, curve, transfer, exposure, **mk):
    """pt_meter then pt_tonemap(exposure_ptr = the state) with no synchronisation between them: (state, out, rgba)."""
    H, W = img.shape[:2]
    col, st = Buf(t, img.nbytes, 0, img), Buf(t, 16, 0, np.asarray(state, F))
    out, rgba = Buf(t, img.nbytes), Buf(t, 4 * W * H)
    t.meter(col.ptr, W, H, st.ptr, **mk)
    t.tonemap(col.ptr, W, H, rgba_ptr=rgba.ptr, out_ptr=out.ptr, curve=curve, transfer=transfer, exposure=exposure, exposure_ptr=st.ptr)
    t.sync()
    res = st.get(F, (4,)), out.get(F, img.shape), rgba.get(np.uint32, (H, W))
    for b in (col, st, out, rgba):
        b.free()
    return res


def chain_ref(img, state, curve, transfer, exposure, **mk):
    s = R.meter(img, state, **mk)
    y = R.curve_out(img, curve, exposure, np.inf, state0=s[0])
    return s, y, R.words(y, transfer, table(transfer))


def assert_chain(got, want, what):
    assert same_bits(got[0], want[0]), f"{what}: state {got[0].tolist()} vs {want[0].tolist()}"
    assert same_bits(got[1], want[1]), f"{what}: out"
    assert np.array_equal(got[2], want[2]), f"{what}: words"


@pytest.mark.parametrize("W,H", [(37, 23), (300, 220)])
def test_meter_then_tonemap_without_a_sync(t, W, H):
    img = image(W, H)
    for curve, transfer, exposure, mk in ((R.ACES, R.SRGB, 1.0, dict()), (R.REINHARD, R.GAMMA22, 0.5, dict(low_pct=0.1, high_pct=0.9, adapt=0.5)),
                                          (R.CLAMP, R.LINEAR, 2.0, dict(key=0.5))):
        args = (img, [2.0, 0, 0, 0], curve, transfer, exposure)
        assert_chain(chain(t, *args, **mk), chain_ref(*args, **mk), f"{W}x{H} curve {curve}")


def test_tonemap_ignores_an_invalid_device_exposure(t):
    img = image(37, 23)
    want = R.curve_out(img, R.ACES, 0.75)
    for bad in (np.nan, 0.0, -1.0, np.inf, -np.inf):
        col, st, out = Buf(t, img.nbytes, 0, img), Buf(t, 16, 0, np.array([bad, 2, 2, 2], F)), Buf(t, img.nbytes)
        t.tonemap(col.ptr, 37, 23, out_ptr=out.ptr, curve=g.TONE_ACES, exposure=0.75, exposure_ptr=st.ptr)
        t.sync()
        assert same_bits(out.get(F, img.shape), want), bad
        assert same_bits(st.get(F, (4,)), np.array([bad, 2, 2, 2], F))
        for b in (col, st, out):
            b.free()
    # a valid one scales; a product that overflows falls back
    col, st, out = Buf(t, img.nbytes, 0, img), Buf(t, 16, 0, np.array([0.125, 0, 0, 0], F)), Buf(t, img.nbytes)
    t.tonemap(col.ptr, 37, 23, out_ptr=out.ptr, curve=g.TONE_ACES, exposure=0.75, exposure_ptr=st.ptr)
    t.sync()
    assert same_bits(out.get(F, img.shape), R.curve_out(img, R.ACES, 0.75, state0=0.125))
    st2 = Buf(t, 16, 0, np.array([3e38, 0, 0, 0], F))
    t.tonemap(col.ptr, 37, 23, out_ptr=out.ptr, curve=g.TONE_ACES, exposure=4.0, exposure_ptr=st2.ptr)
    t.sync()
    assert same_bits(out.get(F, img.shape), R.curve_out(img, R.ACES, 4.0))
    for b in (col, st, st2, out):
        b.free()


def test_timing_covers_both_calls(t):
    img = image(64, 4)
    col, st, rgba = Buf(t, img.nbytes, 0, img), Buf(t, 16, 0, np.zeros(4, F)), Buf(t, 4 * 256)
    t.set_option(g.OPT_TIMING, 1)
    try:
        t.meter(col.ptr, 64, 4, st.ptr)
        t.sync()
        assert t.last_kernel_ms() > 0
        t.tonemap(col.ptr, 64, 4, rgba_ptr=rgba.ptr, transfer=g.XFER_SRGB)
        t.sync()
        assert t.last_kernel_ms() > 0
    finally:
        t.set_option(g.OPT_TIMING, 0)
    for b in (col, st, rgba):
        b.free()


# ---------------------------------------------------------------------------------------------------- 4: call history
def test_call_history_changes_nothing():
    """meter + tonemap at 37 x 23, at 300 x 220, then at 37 x 23 again on one context equal a fresh context's results, before and after
    a pt_denoise and a pt_select_pixels on the same context, whose results do not change either."""
    small, big = image(37, 23), image(300, 220)
    args = ([1.5, 0, 0, 0], R.REINHARD, R.SRGB, 0.8)
    mk = dict(low_pct=0.05, high_pct=0.95, adapt=0.5)
    fresh = {}
    for name, img in (("small", small), ("big", big)):
        tr = g.PathTracer(0)
        try:
            fresh[name] = chain(tr, img, *args, **mk)
        finally:
            tr.close()
        assert_chain(fresh[name], chain_ref(img, *args, **mk), f"fresh {name}")

    W, H = 37, 23
    rng = np.random.default_rng(9)
    colour = rng.random((H, W, 3), dtype=F)
    guides = [np.concatenate([rng.random((H, W, 3), dtype=F), np.zeros((H, W, 1), F)], -1) for _ in range(2)]
    guides.append(np.concatenate([rng.random((H, W, 3), dtype=F), np.full((H, W, 1), 3.0, F)], -1))
    moments = rng.random((H, W, 2), dtype=F)
    counts = rng.integers(0, 9, (H, W)).astype(np.uint32)

    def others(tr):
        bufs = [Buf(tr, a.nbytes, 0, a) for a in [colour] + guides + [moments, counts]]
        out, lst = Buf(tr, colour.nbytes), Buf(tr, 4 * W * H)
        tr.denoise(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, W, H, out.ptr, iterations=2, sigma_color=0.5)
        n, mean = tr.select_pixels(bufs[4].ptr, bufs[5].ptr, lst.ptr, W, H, 0.2, 2, 8)
        res = out.get(F, colour.shape), n, mean, lst.get(np.uint32, (W * H,))[:n]
        for b in bufs + [out, lst]:
            b.free()
        return res

    def same_others(a, b):
        return same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])

    tr = g.PathTracer(0)
    try:
        for name, img in (("small", small), ("big", big), ("small", small)):
            assert_chain(chain(tr, img, *args, **mk), fresh[name], f"before the other calls, {name}")
        first = others(tr)
        assert first[1] > 0 and first[0].any()
        for name, img in (("small", small), ("big", big), ("small", small)):
            assert_chain(chain(tr, img, *args, **mk), fresh[name], f"after the other calls, {name}")
        assert same_others(others(tr), first), "pt_denoise / pt_select_pixels after the display calls"
    finally:
        tr.close()
    tr = g.PathTracer(0)
    try:
        assert same_others(others(tr), first), "pt_denoise / pt_select_pixels on a context that never ran the display calls"
    finally:
        tr.close()


# ---------------------------------------------------------------------------------------------------- 5: errors write nothing
def test_refusals_in_the_headers_order_write_nothing(t):
    lib, ctx = g._abi.ptmi(), t._ctx
    W, H = 37, 23
    img = image(W, H)
    col, out, rgba, st = Buf(t, img.nbytes, 0, img), Buf(t, img.nbytes), Buf(t, 4 * W * H), Buf(t, 16, 0, np.array([5, 6, 7, 8], F))
    nan, inf = float("nan"), float("inf")

    def tone(tp=(W, H, g.TONE_REINHARD, g.XFER_SRGB, 1.0, 2.0), color=col.ptr, o=out.ptr, r=rgba.ptr):
        rc = lib.pt_tonemap(ctx, C.byref(g.TonemapParams(*tp)) if tp else None, color, st.ptr, o, r)
        return rc, lib.pt_last_error(ctx).decode()

    # each rule alone, and with every later rule broken too: the first in the header's order answers
    assert tone(tp=None) == (INVALID, "pt_tonemap: null argument") and tone(color=None, tp=(0, H, 9, 9, nan, nan)) == (INVALID, "pt_tonemap: null argument")
    assert tone(o=None, r=None, tp=(0, 0, 9, 9, 0.0, 0.0)) == (INVALID, "pt_tonemap: null argument")
    for tp in ((0, H, 9, 9, nan, nan), (W, -1, g.TONE_REINHARD, g.XFER_SRGB, 1.0, 2.0), (65536, 65536, 0, 0, 1.0, 1.0)):
        assert tone(tp=tp) == (INVALID, "pt_tonemap: width and height must be >= 1 with width * height < 2^32"), tp
    for tp in ((W, H, 3, 0, nan, nan), (W, H, -1, 0, 1.0, 1.0), (W, H, g.TONE_REINHARD, 3, 0.0, -1.0), (W, H, 0, -1, 1.0, 1.0)):
        assert tone(tp=tp) == (INVALID, "pt_tonemap: unknown curve or transfer"), tp
    for e in (0.0, -1.0, nan, inf, -inf):
        assert tone(tp=(W, H, g.TONE_REINHARD, g.XFER_SRGB, e, -1.0)) == (INVALID, "pt_tonemap: exposure must be finite and > 0"), e
    for w in (0.0, -1.0, nan, -inf):
        assert tone(tp=(W, H, g.TONE_REINHARD, g.XFER_SRGB, 1.0, w)) == (INVALID, "pt_tonemap: white must be > 0 (+inf: plain Reinhard)"), w

    def meter(mp=(W, H, 0.18, 0.0, 1.0, 0.5, 2.0, 1.0), color=col.ptr, state=st.ptr):
        rc = lib.pt_meter(ctx, C.byref(g.MeterParams(*mp)) if mp else None, color, state, 1)
        return rc, lib.pt_last_error(ctx).decode()

    assert meter(mp=None) == (INVALID, "pt_meter: null argument") and meter(color=None, mp=(0, 0, nan, 2.0, -1.0, nan, nan, nan)) == (INVALID, "pt_meter: null argument")
    assert meter(state=None) == (INVALID, "pt_meter: null argument")
    for mp in ((0, H, nan, 2.0, -1.0, nan, nan, nan), (W, 0, 0.18, 0.0, 1.0, 0.5, 2.0, 1.0), (65536, 65536, 0.18, 0.0, 1.0, 0.5, 2.0, 1.0)):
        assert meter(mp=mp) == (INVALID, "pt_meter: width and height must be >= 1 with width * height < 2^32"), mp
    for key in (0.0, -1.0, nan, inf):
        assert meter(mp=(W, H, key, 2.0, -1.0, nan, nan, nan)) == (INVALID, "pt_meter: key must be finite and > 0"), key
    for lo, hi in ((-0.1, 1.0), (0.5, 0.5), (0.6, 0.5), (0.0, 1.5), (nan, 1.0), (0.0, nan)):
        assert meter(mp=(W, H, 0.18, lo, hi, nan, nan, nan)) == (INVALID, "pt_meter: the percentages must hold 0 <= low_pct < high_pct <= 1"), (lo, hi)
    for mn, mx in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (nan, 1.0), (1.0, nan), (1.0, inf), (inf, inf)):
        assert meter(mp=(W, H, 0.18, 0.0, 1.0, mn, mx, nan)) == (INVALID, "pt_meter: the exposure limits must be finite with 0 < min_exposure <= max_exposure"), (mn, mx)
    for a in (-0.1, 1.5, nan, inf):
        assert meter(mp=(W, H, 0.18, 0.0, 1.0, 0.5, 2.0, a)) == (INVALID, "pt_meter: adapt must be in 0..1"), a
    t.sync()
    assert same_bits(st.get(F, (4,)), np.array([5, 6, 7, 8], F)), "a refused call leaves the state alone"
    assert np.all(out.get(np.uint8, (img.nbytes,)) == CANARY) and np.all(rgba.get(np.uint8, (4 * W * H,)) == CANARY), "a refused call writes nothing"
    assert same_bits(col.get(F, img.shape), img)
    # the edges that pass: white +inf, white ignored outside REINHARD, adapt 0 and 1, min == max
    assert tone(tp=(W, H, g.TONE_REINHARD, g.XFER_SRGB, 1.0, inf))[0] == 0 and tone(tp=(W, H, g.TONE_ACES, g.XFER_LINEAR, 1.0, nan))[0] == 0
    assert meter(mp=(W, H, 0.18, 0.0, 1.0, 1.0, 1.0, 0.0))[0] == 0 and meter(mp=(1, 1, 0.18, 0.0, 1.0, 1.0, 1.0, 1.0))[0] == 0
    t.sync()
    for b in (col, out, rgba, st):
        b.free()


# ---------------------------------------------------------------------------------------------------- 6: pt_app's display flags
def test_pt_app_display_flags(tmp_path):
    """pt_app --tonemap / --transfer / --exposure / --white: the .ppm is the reference chain over the run's own accumulator (its .pfm),
    on pt_render's route and on a --camera route, which packs on the host without the flags and with them accumulates as for a .pfm
    (PT_RAYS_HDR); on pt_render's route clamp + linear + 1 gives today's bytes."""
    import os
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    app = os.path.join(root, "g.p.u-pathtracer_amd", "host", "pt_app")
    base = [app, "--mesh", os.path.join(root, "assets", "cornell.ptmesh"), "--width", "96", "--height", "64", "--frames", "4", "--spp", "4"]

    def run(args, code=0):
        r = subprocess.run(base + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == code, r.stderr[-500:]
        return r

    def file_of(words, name):
        path = str(tmp_path / name)
        g.write_image(path, words)
        return open(path, "rb").read()

    for route in ([], ["--camera", "fisheye"]):
        pfm, plain, tone = tmp_path / "a.pfm", tmp_path / "plain.ppm", tmp_path / "tone.ppm"
        run(route + ["--out", pfm])
        acc = g.read_pfm(str(pfm))
        run(route + ["--tonemap", "clamp", "--out", tone])
        assert open(tone, "rb").read() == file_of(R.tonemap(acc)[1], "ref.ppm"), f"{route}: clamp + linear + exposure 1"
        if not route:
            run(["--out", plain])
            assert open(tone, "rb").read() == open(plain, "rb").read(), "clamp + linear + exposure 1 is what pt_render's route writes without the flags"
        else:
            assert acc.max() > 1.0, "the --camera route's .pfm is unclamped"
        run(route + ["--tonemap", "aces", "--transfer", "srgb", "--exposure", "auto", "--out", tone])
        state = R.meter(acc, np.zeros(4, F), reset=True)
        y = R.curve_out(acc, R.ACES, 1.0, np.inf, state0=state[0])
        assert open(tone, "rb").read() == file_of(R.words(y, R.SRGB, table(R.SRGB)), "ref.ppm"), f"{route}: aces + srgb + auto"
        assert state[3] > 0 and state[0] != 1.0
        run(route + ["--tonemap", "reinhard", "--white", 4, "--transfer", "gamma22", "--exposure", 2.5, "--out", tone])
        y = R.curve_out(acc, R.REINHARD, 2.5, 4.0)
        assert open(tone, "rb").read() == file_of(R.words(y, R.GAMMA22, table(R.GAMMA22)), "ref.ppm"), f"{route}: reinhard + gamma22"
    assert "one of clamp, reinhard, aces" in run(["--tonemap", "filmic"], 1).stderr
    assert "one of linear, srgb, gamma22" in run(["--transfer", "rec709"], 1).stderr
    assert "a finite number > 0, or auto" in run(["--exposure", "-1"], 1).stderr
    assert "must be > 0" in run(["--white", "0"], 1).stderr
