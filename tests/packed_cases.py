"""Gain maps and JPEG/R files from packed RGBA inputs (include/uhdr_hip.h, "packed RGBA inputs"): the model
and the cases, not a test file.  There is no reference code for this entry: the header's arithmetic is the contract, restated here
from the oracle's existing primitives.

A pixel value is np.float32(code) * (1 / 255.0f) (RGBA8888), np.float32(code10) * (1 / 1023.0f) (RGBA1010102) or the exact float32 of
a half (RGBA F16).  A map pixel's sample is samplePixels per channel: one running np.float32 sum over its 4 x 4 block, dy outer, dx
inner, then / 16.  From the two sampled colours on it is generateGainMap without yuvToRgb: the oracle's srgbInvOetf, hlgInvOetf /
pqInvOetf, gamutConv, luminance and encodeGain through ctypes, ~40 us per map pixel: keep the images small and share the results.
"""
import ctypes as C
import functools
import os

import numpy as np

from oracle import oracle as O

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = 0, 1, 2
CG_709, CG_P3, CG_2100 = 0, 1, 2
FMT_8888, FMT_1010102, FMT_F16 = 6, 7, 8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "packed")
# the RGBA8888 -> 4:2:0 corpus (scripts/make_packed_fixtures.py): (width, height, quality); the last one's scan exceeds 16 KiB
JPEG_CASES = [(1, 1, 90), (16, 16, 75), (40, 24, 85), (34, 18, 95), (17, 9, 60), (120, 104, 100)]

# (HDR format, transfer function) pairs the packed calls accept
FORMS = [(FMT_1010102, TF_PQ), (FMT_1010102, TF_HLG), (FMT_F16, TF_LINEAR)]


# ------------------------------------------------------------------ images

def _lcg(n, seed):
    s, out = seed & 0xFFFFFFFF, np.empty(n, np.uint32)
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = s >> 8
    return out


def lcg_rgba8888(w, h, seed):
    """(h, w, 4) uint8: full-range codes in every channel, alpha included (it is ignored)"""
    return (_lcg(w * h * 4, seed) & 255).astype(np.uint8).reshape(h, w, 4)


def lcg_rgba1010102(w, h, seed):
    """(h, w) uint32, R | G << 10 | B << 20 | A << 30: full-range 10-bit codes, 0 and 1023 present, any alpha"""
    v = _lcg(w * h * 4, seed).reshape(h, w, 4)
    c = (v[:, :, :3] % 1024).astype(np.uint32)
    c[0, 0, 0], c[-1, -1, 2] = 0, 1023
    return (c[:, :, 0] | (c[:, :, 1] << 10) | (c[:, :, 2] << 20) | ((v[:, :, 3] & 3).astype(np.uint32) << 30)).astype(np.uint32)


def lcg_rgba_f16(w, h, seed):
    """(h, w, 4) uint16 half-precision patterns: finite values in [0, 4] (patterns 0 .. 0x4400, so every exponent is as likely as
    any other and a sixteenth of the draws is subnormal); 0, a subnormal and 3.0 are present"""
    v = (_lcg(w * h * 4, seed) % 0x4401).astype(np.uint16).reshape(h, w, 4)
    v[0, 0, 0], v[0, 1, 1], v[-1, -1, 2] = 0, 0x0155, 0x4200
    return v


def hdr_image(fmt, w, h, seed):
    return lcg_rgba_f16(w, h, seed) if fmt == FMT_F16 else lcg_rgba1010102(w, h, seed)


# ------------------------------------------------------------------ the model

def pixel_values(img, fmt):
    """(h, w, 3) float32: what the header calls a pixel value"""
    if fmt == FMT_8888:
        return (img[:, :, :3].astype(F) * (F(1) / F(255))).astype(F)
    if fmt == FMT_1010102:
        c = np.stack([img & 1023, (img >> 10) & 1023, (img >> 20) & 1023], axis=2)
        return (c.astype(F) * (F(1) / F(1023))).astype(F)
    return img[:, :, :3].view(np.float16).astype(F)


def sample(values):
    """samplePixels per channel at scale 4: (h, w, 3) float32 -> (h / 4, w / 4, 3) float32; the trailing columns and rows are not read"""
    h, w, _ = values.shape
    mh, mw = h // 4, w // 4
    e = np.zeros((mh, mw, 3), F)
    for dy in range(4):
        for dx in range(4):
            e = (e + values[dy:4 * mh:4, dx:4 * mw:4]).astype(F)
    return (e / F(16)).astype(F)


def linear_nits(sdr, hdr, fmt, tf, sdr_gamut, hdr_gamut):
    """the model up to encodeGain's inputs: (sdr rgb, hdr rgb) as (mh, mw, 3) float32 and (sdr y, hdr y) as (mh, mw) float32, in nits"""
    L = O.load()
    s, hh = sample(pixel_values(sdr, FMT_8888)), sample(pixel_values(hdr, fmt))
    mh, mw, _ = s.shape
    inv = {TF_LINEAR: None, TF_HLG: L.orc_hlgInvOetf, TF_PQ: L.orc_pqInvOetf}[tf]
    white = F(10000.0 if tf == TF_PQ else 1000.0)
    srgb = L.orc_srgbInvOetf
    sl, hl = np.empty((mh, mw, 3), F), np.empty((mh, mw, 3), F)
    ys, yh = np.empty((mh, mw), F), np.empty((mh, mw), F)
    for y in range(mh):
        for x in range(mw):
            a = O.Color(*(srgb(float(v)) for v in s[y, x]))
            e = O.Color(*(float(v) if inv is None else inv(float(v)) for v in hh[y, x]))
            b = L.orc_gamutConv(sdr_gamut, hdr_gamut, e, None)
            sl[y, x], hl[y, x] = a.tup(), b.tup()
            ys[y, x], yh[y, x] = L.orc_luminance(sdr_gamut, a), L.orc_luminance(sdr_gamut, b)
    return (sl * F(203.0)).astype(F), (hl * white).astype(F), (ys * F(203.0)).astype(F), (yh * white).astype(F)


def default_range(tf):
    """the reference's constants (ultrahdr.cpp:250-257): (minContentBoost, maxContentBoost)"""
    return 1.0, float(F(10000.0 if tf == TF_PQ else 1000.0) / F(203.0))


def encode_default(ys, yh, tf):
    """the oracle's three-argument encodeGain against the reference's constants, elementwise -> uint8 of the same shape"""
    lo, hi = default_range(tf)
    enc = O.load().orc_encodeGain3
    out = np.empty(ys.shape, np.uint8)
    flat_s, flat_h, flat_o = ys.reshape(-1), yh.reshape(-1), out.reshape(-1)
    for i in range(flat_s.size):
        flat_o[i] = enc(float(flat_s[i]), float(flat_h[i]), lo, hi)
    return out


@functools.lru_cache(maxsize=None)
def pair(w, h, fmt, seed):
    """the LCG pair of this size: (RGBA8888 image, HDR image of `fmt`), read-only, computed once"""
    sdr, hdr = lcg_rgba8888(w, h, seed), hdr_image(fmt, w, h, seed + 1)
    sdr.setflags(write=False)
    hdr.setflags(write=False)
    return sdr, hdr


@functools.lru_cache(maxsize=None)
def model(w, h, fmt, tf, seed, sdr_gamut=CG_709, hdr_gamut=CG_2100):
    """linear_nits of pair(w, h, fmt, seed), computed once"""
    sdr, hdr = pair(w, h, fmt, seed)
    out = linear_nits(sdr, hdr, fmt, tf, sdr_gamut, hdr_gamut)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_default(w, h, fmt, tf, seed, rgb, sdr_gamut=CG_709, hdr_gamut=CG_2100):
    """the map of metadata_in = NULL: (mh, mw) uint8, or (mh, mw, 4) RGBA with A = 0xFF"""
    sl, hl, ys, yh = model(w, h, fmt, tf, seed, sdr_gamut, hdr_gamut)
    if not rgb:
        return encode_default(ys, yh, tf)
    out = np.full(sl.shape[:2] + (4,), 0xFF, np.uint8)
    out[:, :, :3] = encode_default(sl, hl, tf)
    return out


def seed_of(w, fmt, tf):
    """seeds of the pairs, chosen so that the input condition of tests/test_packed_cpu.py holds"""
    return 9000 + 16 * w + 4 * (fmt - FMT_8888) + tf


# ------------------------------------------------------------------ the RGBA8888 -> 4:2:0 corpus

def jpeg_image(w, h):
    """the generator of scripts/make_packed_fixtures.py: a smooth field with LCG noise on top, (h, w, 4) uint8, alpha random.  The
    largest image is all noise, so that its scan exceeds 16 KiB"""
    n = _lcg(w * h * 4, 31 * w + h).reshape(h, w, 4)
    if w * h > 10000:
        return (n & 255).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 9 + 60) % 256, (255 - xx * 5 - yy * 4) % 256, np.zeros_like(xx)], axis=2)
    out = (base + (n & 31)) % 256
    out[:, :, 3] = n[:, :, 3] & 255
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def golden_rgba(w, h):
    a = np.load(os.path.join(DIR, "rgba_%dx%d.npy" % (w, h)))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def golden_jpeg_420(w, h, q):
    """Pillow's quality=q, subsampling=2 file of golden_rgba(w, h)'s R, G, B"""
    return open(os.path.join(DIR, "rgba_%dx%d_q%d_s2.jpg" % (w, h, q)), "rb").read()


def pillow_420(rgba, q):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgba[:, :, :3]), "RGB").save(buf, "JPEG", quality=q, subsampling=2)
    return buf.getvalue()
