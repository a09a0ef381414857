"""numpy restatement of the display stage's arithmetic (include/ptmi.h): pt_tonemap's exposure, curves and display words, the
threshold tables of pt_tonemap_thresholds, and pt_meter's histogram, trim, average and adaptation.

binary32 throughout, one rounding per operation, as the device code (plain *, + and the correctly rounded /, no fused
multiply-add): numpy's float32 arithmetic gives the same bits.  The meter's histogram is integer arithmetic on the floats' own
bits; its average is a handful of double operations.  Also the inputs both test modules draw from: HDR values, the special values,
the neighbours of every threshold and of every bin edge."""
import numpy as np

F = np.float32
CLAMP, REINHARD, ACES = 0, 1, 2
LINEAR, SRGB, GAMMA22 = 0, 1, 2
CAP = F(65536.0)
BINS = 256
BIN0 = (127 - 16) << 3


# ---------------------------------------------------------------------------------------------------- the tables
def eotf(transfer, v):
    """Encoded value -> linear, in double."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):   # (a negative v: thresholds64's entry 0, which it overwrites)
        if transfer == SRGB:
            return np.where(v <= 0.04045, v / 12.92, np.power((v + 0.055) / 1.055, 2.4))
        return np.power(v, 2.2)


def oetf(transfer, y):
    """Linear -> encoded value, in double: the inverse of eotf."""
    y = np.asarray(y, np.float64)
    if transfer == SRGB:
        return np.where(y <= 0.04045 / 12.92, y * 12.92, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)
    return np.power(y, 1.0 / 2.2)


def thresholds64(transfer):
    """T in double: T[0] = 0, T[k] = eotf((k - 0.5) / 255)."""
    t = eotf(transfer, (np.arange(256, dtype=np.float64) - 0.5) / 255.0)
    t[0] = 0.0
    return t


def thresholds(transfer):
    """T rounded once to binary32."""
    return thresholds64(transfer).astype(F)


def codes(T, y):
    """The number of k in 1..255 with y >= T[k] (T ascends, so a search), as uint32."""
    return np.searchsorted(np.asarray(T, F)[1:], np.asarray(y, F), side="right").astype(np.uint32)


def pack_linear(y):
    """(unsigned char)(255.0f * y) of a value in 0..1: the truncating pack of pt_render's display words."""
    return (F(255.0) * np.asarray(y, F)).astype(np.uint32) & np.uint32(0xFF)


# ---------------------------------------------------------------------------------------------------- pt_tonemap
def luminance(c):
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def exposure_in_use(exposure, state0=None):
    """tp->exposure, or its product with exposure_dev[0] where that is finite and > 0."""
    e = F(exposure)
    if state0 is None:
        return e
    with np.errstate(all="ignore"):
        p = e * F(state0)
    return p if np.isfinite(p) and p > 0 else e


def curve_out(color, curve=CLAMP, exposure=1.0, white=np.inf, state0=None):
    """What out_dev receives: float32 of color's shape."""
    c = np.asarray(color, F)
    e = exposure_in_use(exposure, state0)
    with np.errstate(all="ignore"):
        x = c * e
        x = np.where(x > 0, np.fmin(x, CAP), F(0)).astype(F)
        if curve == CLAMP:
            y = np.fmin(x, F(1))
        elif curve == REINHARD:
            w = F(white)
            iw2 = F(0) if np.isposinf(w) else F(1.0) / (w * w)
            L = luminance(x)
            s = (F(1.0) + L * iw2) / (F(1.0) + L)
            y = np.fmin(x * s[..., None], F(1))
        else:
            a = x * (F(2.51) * x + F(0.03))
            b = x * (F(2.43) * x + F(0.59)) + F(0.14)
            y = np.fmin(a / b, F(1))
    assert y.dtype == F
    return y


def words(y, transfer=LINEAR, T=None):
    """0x00BBGGRR of the curve's output y [...][3]; T: the table to count against (thresholds(transfer) unless given)."""
    y = np.asarray(y, F)
    if transfer == LINEAR:
        k = pack_linear(y)
    else:
        k = codes(thresholds(transfer) if T is None else T, y)
    return (k[..., 2] << np.uint32(16)) | (k[..., 1] << np.uint32(8)) | k[..., 0]


def tonemap(color, curve=CLAMP, transfer=LINEAR, exposure=1.0, white=np.inf, state0=None, T=None):
    """(out, rgba) of pt_tonemap."""
    y = curve_out(color, curve, exposure, white, state0)
    return y, words(y, transfer, T)


# ---------------------------------------------------------------------------------------------------- pt_meter
def bins(color):
    """The histogram bin of every pixel of color [...][3]; BINS = not metered."""
    with np.errstate(all="ignore"):
        L = luminance(color)
        raw = (np.ascontiguousarray(L).view(np.uint32) >> np.uint32(20)).astype(np.int64) - BIN0
        out = np.where(L >= F(65536.0), BINS - 1, raw)
        out = np.where(~np.isfinite(L) | (L < F(2.0 ** -16)), BINS, out)
    return out


def histogram(color):
    """(counts of the 256 bins, the number of unmetered pixels)."""
    h = np.bincount(bins(color).reshape(-1), minlength=BINS + 1)
    return h[:BINS].astype(np.int64), int(h[BINS])


def _finite_positive(v):
    return bool(np.isfinite(v) and v > 0)


def meter(color, state=None, key=0.18, low_pct=0.0, high_pct=1.0, min_exposure=2.0 ** -16, max_exposure=2.0 ** 16, adapt=1.0, reset=False):
    """The four state floats after pt_meter over color [...][3]; state: the four floats before (None: zeros)."""
    prev = F(0) if state is None else F(np.asarray(state, F)[0])
    h, _ = histogram(color)
    cum = np.cumsum(h)
    n = int(cum[-1])
    lo = int(float(F(low_pct)) * float(n))
    hi = int(float(F(high_pct)) * float(n))
    if hi <= lo:
        lo, hi = 0, n
    before = cum - h
    w = np.maximum(0, np.minimum(cum, hi) - np.maximum(before, lo))
    S = int(np.sum(w * (2 * np.arange(BINS, dtype=np.int64) + 1)))
    Wt = int(np.sum(w))
    prev_ok = _finite_positive(prev)
    if Wt:
        p = float(S) / float(16 * Wt) - 16.0
        i = np.floor(p)
        l_avg = F(np.ldexp(1.0 + (p - i), int(i)))
        with np.errstate(all="ignore"):
            target = F(key) / l_avg
    else:
        l_avg = F(0)
        target = prev if prev_ok else F(1)
    target = np.fmin(np.fmax(target, F(min_exposure)), F(max_exposure))
    with np.errstate(all="ignore"):
        use = target if (reset or not prev_ok) else prev + (target - prev) * F(adapt)
    out = np.array([use, target, l_avg, F(Wt)], F)
    return out


# ---------------------------------------------------------------------------------------------------- inputs
def neighbours(v):
    """Every value of v with the floats just below and just above it."""
    v = np.asarray(v, F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]).astype(F)


SPECIALS = np.array([0.0, -1.0, np.nan, np.inf, -np.inf, 1e-42, 1.0, 65536.0, 0.18], F)   # 1e-42: a denormal


def bin_edges():
    """Every bin edge in 2^-16 .. 2^16 (the floats whose low 20 bits are zero there, 2^16 included) with its lower neighbour."""
    e = ((np.arange(BINS + 1, dtype=np.uint32) + np.uint32(BIN0)) << np.uint32(20)).view(F)
    return np.concatenate([e, np.nextafter(e, F(0))]).astype(F)


def colours_with_luminance(L):
    """For every value of L a colour whose luminance, as the device adds it up, is that value exactly where a candidate has it:
    the nine grey levels around L, then the nine pure greens around L / 0.7152f (one multiplication, so most values are met);
    else the grey level L itself, still within an ulp or two."""
    L = np.asarray(L, F)
    step = np.arange(-4, 5, dtype=np.int32)[None, :]
    grey = (L.view(np.int32)[:, None] + step).view(F)
    green = ((L / F(0.7152)).view(np.int32)[:, None] + step).view(F)
    cand = np.concatenate([np.repeat(grey[..., None], 3, -1), np.stack([np.zeros_like(green), green, np.zeros_like(green)], -1)], 1)
    hit = luminance(cand) == L[:, None]
    pick = np.where(hit.any(1), hit.argmax(1), 4)
    return cand[np.arange(len(L)), pick]


def hdr_image(W, H, seed):
    """A seeded float32 [H][W][3] image: HDR values over 2^-20 .. 2^20, then — as far as the pixels go — the special values (each in
    one channel of a grey pixel and as a whole pixel), every threshold of both tables with its two neighbours, and every meter bin
    edge with its lower neighbour as the luminance of a grey or a green pixel (colours_with_luminance)."""
    rng = np.random.default_rng(seed)
    n = W * H
    img = np.exp2(rng.uniform(-20.0, 20.0, (n, 3))).astype(F)
    extra = [np.repeat(SPECIALS[:, None], 3, 1)]
    one = np.full((len(SPECIALS), 3), F(0.5))
    one[np.arange(len(SPECIALS)), np.arange(len(SPECIALS)) % 3] = SPECIALS
    extra.append(one)
    for tr in (SRGB, GAMMA22):
        extra.append(np.repeat(neighbours(thresholds(tr))[:, None], 3, 1))
    extra.append(colours_with_luminance(bin_edges()))
    extra = np.concatenate(extra).astype(F)
    n_special = 2 * len(SPECIALS)
    # an image too small for all of them gets the special values and a seeded choice of the rest, and keeps a quarter of its HDR values
    order = np.concatenate([np.arange(n_special), n_special + rng.permutation(len(extra) - n_special)])
    k = min(len(extra), n - n // 4)
    at = np.arange(k) * (n // k)   # spread over the image, so that every block of a grid meets some
    img[at] = extra[order[:k]]
    return img.reshape(H, W, 3)
