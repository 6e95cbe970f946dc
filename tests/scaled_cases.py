"""Gain maps at any scale factor (include/uhdr_hip.h, "gain maps at any scale factor"): the model and the
images, not a test file.

A map pixel is generateGainMap's loop body (ultrahdr.cpp:316-334) with the scale factor s in place of kMapDimensionScaleFactor: the
oracle's sampleYuv420 / sampleP010 -- they take the scale --, yuvToRgb, the inverse OETFs, gamutConv and luminance through ctypes,
then the reference's three-argument encodeGain (the reference's metadata) or tests/gainmap_md_cases.py's rule (the caller's), on the
luminances or per channel.  ~40 us per map pixel: keep a case under about 6000 map pixels; `expected` caches per case.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from tests import gainmap_md_cases as MD

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = 0, 1, 2
CG_709, CG_P3, CG_2100 = 0, 1, 2

# gamma 2.2, both offsets 1 / 64 and a range of [0.5, 6] (the capacity range takes no part in a map)
MD_CASE = (2.2, 1 / 64, 1 / 64, 0.5, 6.0, 0.5, 6.0)


def nits(yuv_img, p010_img, tf, s, sdr_is_601=False):
    """(sdr rgb, hdr rgb, sdr y, hdr y) in nits, float32, of the (height / s) x (width / s) map: what encodeGain receives"""
    L = O.load()
    mw, mh = yuv_img.width // s, yuv_img.height // s
    sdr_gamut, hdr_gamut = yuv_img.colorGamut, p010_img.colorGamut
    sdr_yuv_gamut = CG_P3 if sdr_is_601 else sdr_gamut
    inv = {TF_LINEAR: None, TF_HLG: L.orc_hlgInvOetf, TF_PQ: L.orc_pqInvOetf}[tf]
    white = F(10000.0 if tf == TF_PQ else 1000.0)
    sl, hl = np.empty((mh, mw, 3), F), np.empty((mh, mw, 3), F)
    ys, yh = np.empty((mh, mw), F), np.empty((mh, mw), F)
    yi, pi = C.byref(yuv_img), C.byref(p010_img)
    Color, srgb = O.Color, L.orc_srgbInvOetf
    for y in range(mh):
        for x in range(mw):
            e = L.orc_yuvToRgb(sdr_yuv_gamut, L.orc_sampleYuv420(yi, s, x, y))
            a = Color(srgb(e.r), srgb(e.g), srgb(e.b))
            e = L.orc_yuvToRgb(hdr_gamut, L.orc_sampleP010(pi, s, x, y))
            if inv is not None:
                e = Color(inv(e.r), inv(e.g), inv(e.b))
            b = L.orc_gamutConv(sdr_gamut, hdr_gamut, e, None)
            sl[y, x], hl[y, x] = a.tup(), b.tup()
            ys[y, x], yh[y, x] = L.orc_luminance(sdr_gamut, a), L.orc_luminance(sdr_gamut, b)
    return (sl * F(203.0)).astype(F), (hl * white).astype(F), (ys * F(203.0)).astype(F), (yh * white).astype(F)


def encode_default(a, b, tf):
    """the oracle's three-argument encodeGain against the reference's constants (ultrahdr.cpp:250-257), elementwise"""
    lo, hi = 1.0, float(F(10000.0 if tf == TF_PQ else 1000.0) / F(203.0))
    enc = O.load().orc_encodeGain3
    out = np.empty(a.shape, np.uint8)
    fa, fb, fo = a.reshape(-1), b.reshape(-1), out.reshape(-1)
    for i in range(fa.size):
        fo[i] = enc(float(fa[i]), float(fb[i]), lo, hi)
    return out


def map_of(yuv_img, p010_img, tf, s, rgb=False, case=None, sdr_is_601=False):
    """the expected map: (mh, mw) uint8, or (mh, mw, 4) RGBA with A = 0xFF; case: a tests/gainmap_md_cases.py tuple, or None for the
    reference's metadata.  With a case, also the values in front of the truncation (None without)"""
    sl, hl, ys, yh = nits(yuv_img, p010_img, tf, s, sdr_is_601)
    a, b = (sl, hl) if rgb else (ys, yh)
    if case is None:
        by, v = encode_default(a, b, tf), None
    else:
        by, v = MD.encode(a, b, case)
    if not rgb:
        return by, v
    out = np.full(by.shape[:2] + (4,), 0xFF, np.uint8)
    out[:, :, :3] = by
    return out, v


# ------------------------------------------------------------------ images

class Pair:
    """an LCG pair as planes, optionally with rows longer than the width (pad) and a black SDR rectangle.  Planes: y (h, ls) uint8,
    uv (h, cs) uint8 -- U rows, then V rows at chroma_stride * (h / 2) --, hy (h, ls) uint16, huv (h / 2, ls) uint16"""

    def __init__(self, w, h, seed, sdr_gamut=CG_709, hdr_gamut=CG_2100, pad=0, black=None):
        p010, yuv = O.lcg_frame(w, h, seed)
        self.w, self.h, self.sdr_gamut, self.hdr_gamut = w, h, sdr_gamut, hdr_gamut
        self.ls, self.cs = w + pad, w // 2 + pad // 2
        self.y = np.full((h, self.ls), 0xEE, np.uint8)
        self.y[:, :w] = yuv[:w * h].reshape(h, w)
        self.uv = np.full((h, self.cs), 0xEE, np.uint8)
        self.uv[:, :w // 2] = yuv[w * h:].reshape(h, w // 2)
        self.hy = np.full((h, self.ls), 0xEEEE, np.uint16)
        self.hy[:, :w] = p010[:w * h].reshape(h, w)
        self.huv = np.full((h // 2, self.ls), 0xEEEE, np.uint16)
        self.huv[:, :w] = p010[w * h:].reshape(h // 2, w)
        if black is not None:   # (x0, y0, x1, y1) in pixels, even: Y = 0, U = V = 128 -- every map pixel inside is in doubt
            x0, y0, x1, y1 = black
            self.y[y0:y1, x0:x1] = 0
            self.uv[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = 128
            self.uv[h // 2 + y0 // 2:h // 2 + y1 // 2, x0 // 2:x1 // 2] = 128
        for a in (self.y, self.uv, self.hy, self.huv):
            a.setflags(write=False)

    def oracle_images(self):
        yi = O.yuv420_image(self.y, self.w, self.h, self.sdr_gamut, luma_stride=self.ls, chroma_stride=self.cs, chroma=self.uv)
        pi = O.p010_image(self.hy, self.w, self.h, self.hdr_gamut, luma_stride=self.ls, chroma_stride=self.ls, chroma=self.huv)
        return yi, pi


@functools.lru_cache(maxsize=None)
def pair(w, h, seed, sdr_gamut=CG_709, hdr_gamut=CG_2100, pad=0, black=None):
    return Pair(w, h, seed, sdr_gamut, hdr_gamut, pad, black)


@functools.lru_cache(maxsize=None)
def expected(w, h, seed, tf, s, rgb=False, case=None, sdr_is_601=False, sdr_gamut=CG_709, hdr_gamut=CG_2100, pad=0, black=None):
    """map_of for pair(...), computed once, read-only: (map, v)"""
    yi, pi = pair(w, h, seed, sdr_gamut, hdr_gamut, pad, black).oracle_images()
    m, v = map_of(yi, pi, tf, s, rgb, case, sdr_is_601)
    m.setflags(write=False)
    return m, v
