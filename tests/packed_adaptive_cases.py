"""Content-adaptive gain maps for packed RGBA inputs (include/uhdr_hip.h, "content-adaptive gain maps for packed RGBA inputs";
DESIGN.md section 4.1.9): the model and the inputs, not a test file.

The model restates nothing of its own: tests/packed_cases.py's linear_nits gives the two linear colours and the two luminances in
nits, tests/adaptive_cases.py's gains, rule and encode the rest.  One plane takes the luminances; RGB takes the colours per channel
with one range from the extremes over all three channels.  ~40 us per map pixel: the inputs are small and every result is cached.

The inputs are built in numpy for the three HDR forms of packed_cases.FORMS from a linear-light description: an SDR colour s in
[0, 1] and a gain field g, the HDR colour s * 203 * g nits, both quantised to their formats.  tests/test_packed_adaptive_cpu.py holds
each input's condition on the model's range, so that the GPU test cannot pass for the wrong reason."""
import functools

import numpy as np

from oracle import oracle as O
from tests import adaptive_cases as A
from tests import packed_cases as P

F = np.float32
GAMUTS = (P.CG_709, P.CG_2100)
TINT = np.array([1.0, 0.97, 0.94])


# ------------------------------------------------------------------ formats

def _srgb_oetf(x):
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 1e-12), 1 / 2.4) - 0.055)


def _pq_oetf(x):
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    p = np.power(np.maximum(x, 0.0), m1)
    return np.power((c1 + c2 * p) / (1 + c3 * p), m2)


def _hlg_oetf(x):
    a, b, c = 0.17883277, 0.28466892, 0.55991073
    return np.where(x <= 1 / 12, np.sqrt(3 * np.maximum(x, 0.0)), a * np.log(np.maximum(12 * x - b, 1e-12)) + c)


def sdr_from_linear(lin):
    """(h, w, 3) linear [0, 1] -> (h, w, 4) uint8 RGBA8888, alpha 0xFF"""
    out = np.full(lin.shape[:2] + (4,), 0xFF, np.uint8)
    out[:, :, :3] = np.clip(np.rint(_srgb_oetf(lin) * 255), 0, 255).astype(np.uint8)
    return out


def hdr_from_nits(nits, fmt, tf):
    """(h, w, 3) nits -> the HDR image of `fmt`: (h, w) uint32 RGBA1010102 (alpha 3) or (h, w, 4) uint16 halves (alpha 1.0)"""
    if fmt == P.FMT_F16:
        out = np.full(nits.shape[:2] + (4,), 0x3C00, np.uint16)
        out[:, :, :3] = (nits / 1000.0).astype(np.float16).view(np.uint16)
        return out
    v = _pq_oetf(nits / 10000.0) if tf == P.TF_PQ else _hlg_oetf(nits / 1000.0)
    c = np.clip(np.rint(v * 1023), 0, 1023).astype(np.uint32)
    return (c[:, :, 0] | (c[:, :, 1] << 10) | (c[:, :, 2] << 20) | np.uint32(3 << 30)).astype(np.uint32)


# ------------------------------------------------------------------ inputs: fn(w, h, fmt, tf) -> (sdr, hdr)

def _fields(w, h, g0, g1):
    """the SDR ramp (left to right, tinted) and the gain ramp (top to bottom, g0 .. g1)"""
    x, y = np.meshgrid(np.arange(w) / max(w - 1, 1), np.arange(h) / max(h - 1, 1))
    s = (0.1 + 0.7 * x)[:, :, None] * TINT
    return s, (g0 + (g1 - g0) * y)[:, :, None]


def _from_fields(s, g, fmt, tf):
    return sdr_from_linear(s), hdr_from_nits(s * 203.0 * g, fmt, tf)


def interior(w, h, fmt, tf):
    """a smooth HDR ramp over an SDR rendition that is brighter at the top (gain 0.5) and darker at the bottom (gain 3)"""
    return _from_fields(*_fields(w, h, 0.5, 3.0), fmt, tf)


def clamped(w, h, fmt, tf):
    return P.pair(w, h, fmt, P.seed_of(w, fmt, tf))


# which ends of the range rule the LCG pair reaches at 64 x 64, by (transfer function, rgb): (lo == 0.25, hi == cap).  The mean of
# sixteen random pixels pulls a block's luminance towards the middle, so the one-plane PQ map stays inside both ends and no one-plane
# map reaches 0.25; per channel the gamut conversion leaves negative HDR channels and every form reaches 0.25.  both_clamps below
# reaches both ends in every form.
CLAMPED_ENDS = {(P.TF_PQ, False): (False, False), (P.TF_PQ, True): (True, False), (P.TF_HLG, False): (False, True),
                (P.TF_HLG, True): (True, True), (P.TF_LINEAR, False): (False, True), (P.TF_LINEAR, True): (True, True)}


def both_clamps(w, h, fmt, tf):
    """the interior ramp with gains from 0.1 to 1.3 times the transfer function's cap, a geometric ramp so that whole block rows lie
    beyond either end: g_min < 0.25 and g_max > cap"""
    s, g = _fields(w, h, 0.0, 1.0)
    return _from_fields(s, 0.1 * np.power(13.0 * float(A.cap(tf)), g), fmt, tf)


def flat(w, h, fmt, tf):
    """every gain exactly 1: no exact equality of two luminances survives the formats' quantisation, so the SDR image is code 0 --
    encodeGain's `y_sdr <= 0 -> 1` -- under an HDR ramp that is not"""
    sdr, hdr = interior(w, h, fmt, tf)
    sdr = sdr.copy()
    sdr[:, :, :3] = 0
    return sdr, hdr


def all_above_one(w, h, fmt, tf):
    return _from_fields(*_fields(w, h, 2.0, 3.0), fmt, tf)


def black(w, h, fmt, tf):
    """interior with SDR code 0 over the map blocks of rows 0-1, columns 0-3 (all channels: y_sdr = 0), and with the red channel
    alone 0 over the blocks of rows 2-3, columns 2-5 (RGB: gain 1 in one channel of a pixel whose other two have their own)"""
    sdr, hdr = interior(w, h, fmt, tf)
    sdr = sdr.copy()
    sdr[0:8, 0:16, :3] = 0
    sdr[8:16, 8:24, 0] = 0
    return sdr, hdr


def _lone(w, h, fmt, tf, factor):
    s, g = _fields(w, h, 0.5, 3.0)
    g = np.broadcast_to(g, s.shape[:2] + (1,)).copy()
    mw, mh = w // 4, h // 4
    g[4 * (mh - 1):4 * mh, 4 * (mw - 1):4 * mw] *= factor
    return _from_fields(s, g, fmt, tf)


def lone_max(w, h, fmt, tf):
    """interior with the 4 x 4 block of the last map pixel of the last row 1.4 times as bright in HDR: the image's maximum"""
    return _lone(w, h, fmt, tf, 1.4)


def lone_min(w, h, fmt, tf):
    """... and 0.1 times as bright: the image's minimum"""
    return _lone(w, h, fmt, tf, 0.1)


INPUTS = {"interior": interior, "clamped": clamped, "both_clamps": both_clamps, "flat": flat, "all_above_one": all_above_one, "black": black,
          "lone_max": lone_max, "lone_min": lone_min}
# the size each input is used at: 68 x 36 (map 17 x 9, a lone last pixel in every row) where the condition is about that pixel
SIZES = {"interior": (64, 64), "clamped": (64, 64), "both_clamps": (64, 64), "flat": (64, 64), "all_above_one": (68, 36), "black": (64, 64),
         "lone_max": (68, 36), "lone_min": (68, 36)}


@functools.lru_cache(maxsize=None)
def images(name, w, h, fmt, tf):
    sdr, hdr = INPUTS[name](w, h, fmt, tf)
    sdr, hdr = np.ascontiguousarray(sdr), np.ascontiguousarray(hdr)
    sdr.setflags(write=False)
    hdr.setflags(write=False)
    return sdr, hdr


# ------------------------------------------------------------------ the model

@functools.lru_cache(maxsize=None)
def nits(name, w, h, fmt, tf, gamuts=GAMUTS):
    """packed_cases.linear_nits of the input: (sl, hl, ys, yh), read-only, computed once"""
    sdr, hdr = images(name, w, h, fmt, tf)
    out = P.linear_nits(sdr, hdr, fmt, tf, *gamuts)
    for a in out:
        a.setflags(write=False)
    return out


def operands(lin, rgb):
    """what encodeGain sees: the colours per channel (RGB) or the luminances"""
    sl, hl, ys, yh = lin
    return (sl, hl) if rgb else (ys, yh)


def minmax(lin, rgb):
    """(g_min, g_max) as np.float32: over all map pixels, for RGB over all three channels of all map pixels"""
    return A.minmax(*operands(lin, rgb))


def encode(lin, rgb, lo, hi):
    """the map against (lo, hi): (mh, mw) uint8, or (mh, mw, 4) RGBA with A = 0xFF"""
    s, hh = operands(lin, rgb)
    b = A.encode(O, s, hh, lo, hi)
    if not rgb:
        return b
    out = np.full(b.shape[:2] + (4,), 0xFF, np.uint8)
    out[:, :, :3] = b
    return out


@functools.lru_cache(maxsize=None)
def expected(name, w, h, fmt, tf, rgb, gamuts=GAMUTS):
    """PER_IMAGE: (map, (g_min, g_max), (lo, hi)) of the input"""
    lin = nits(name, w, h, fmt, tf, gamuts)
    mm = minmax(lin, rgb)
    rng = A.rule(tf, *mm)
    m = encode(lin, rgb, *rng)
    m.setflags(write=False)
    return m, mm, rng


def recovery_error(lin, rgb, gmap, lo, hi):
    """adaptive_cases.recovery_error over the map pixels whose gain is positive and finite (log2 of the others means nothing)"""
    g = A.gains(*operands(lin, rgb))
    b = gmap[:, :, :3] if rgb else gmap
    ok = np.isfinite(g) & (g > 0)
    return A.recovery_error(b[ok], lo, hi, g[ok])
