"""Per-channel (RGB) gain maps: the expected values, restated from the oracle's existing primitives, and the committed corpus
(tests/golden/rgbmap/, scripts/make_rgbmap_fixtures.py).

`channel_bytes` is generate's loop body up to the two linear colours (ultrahdr.cpp:316-330 without the luminances): sampleYuv420 /
sampleP010 at scale 4, yuvToRgb, the inverse OETFs, gamutConv -- then the reference's three-argument encodeGain per CHANNEL on the
np.float32 products channel x 203 / channel x white.  `composite_apply` is the separability argument as a program: every operation
of applyGainMap behind the gain is per channel, so channel c of the per-channel rendition is channel c of the single-channel
rendition with plane c of the map.  ~30 us per map pixel: keep the images small and share the results.
"""
import ctypes as C
import functools
import os

import numpy as np

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = 0, 1, 2
CG_709, CG_P3, CG_2100 = 0, 1, 2
FMT_F16, FMT_PQ, FMT_HLG, FMT_RGB10 = 1, 2, 3, 4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "rgbmap")
SIZES = [(1, 1), (8, 8), (17, 9), (45, 37), (264, 200)]
QUALITIES = [85, 95]
WITH_420 = [(45, 37), (264, 200)]


def channel_bytes(orc, yuv_img, p010_img, tf, sdr_is_601=False):
    """(map_h, map_w, 3) uint8: byte c of a map pixel is encodeGain(sdr_rgb.c * 203, hdr_rgb.c * white, the reference's constants)"""
    L = orc.load()
    mw, mh = yuv_img.width // 4, yuv_img.height // 4
    sdr_gamut, hdr_gamut = yuv_img.colorGamut, p010_img.colorGamut
    sdr_yuv_gamut = CG_P3 if sdr_is_601 else sdr_gamut
    inv = {TF_LINEAR: None, TF_HLG: L.orc_hlgInvOetf, TF_PQ: L.orc_pqInvOetf}[tf]
    white = F(10000.0 if tf == TF_PQ else 1000.0)
    lo, hi = 1.0, float(white / F(203.0))   # ultrahdr.cpp:250-257
    out = np.empty((mh, mw, 3), np.uint8)
    yi, pi = C.byref(yuv_img), C.byref(p010_img)
    Color, srgb, enc = orc.Color, L.orc_srgbInvOetf, L.orc_encodeGain3
    for y in range(mh):
        for x in range(mw):
            e = L.orc_yuvToRgb(sdr_yuv_gamut, L.orc_sampleYuv420(yi, 4, x, y))
            s = (srgb(e.r), srgb(e.g), srgb(e.b))
            e = L.orc_yuvToRgb(hdr_gamut, L.orc_sampleP010(pi, 4, x, y))
            if inv is not None:
                e = Color(inv(e.r), inv(e.g), inv(e.b))
            hh = L.orc_gamutConv(sdr_gamut, hdr_gamut, e, None).tup()
            for c in range(3):
                out[y, x, c] = enc(float(F(s[c]) * F(203.0)), float(F(hh[c]) * white), lo, hi)
    return out


def composite_apply(orc, yuv_img, rgba_map, md, fmt, boost):
    """the per-channel rendition as bytes: three runs of the oracle's applyGainMap with planes R, G, B of rgba_map ((mh, mw, 4) or
    (mh, mw, 3) uint8), channel c taken from run c; the alpha of RGBA1010102 / F16 from run 0 (every run writes the same)"""
    w, h = yuv_img.width, yuv_img.height
    runs = []
    for c in range(3):
        st, out, _ = orc.apply("orc_", yuv_img, np.ascontiguousarray(rgba_map[:, :, c]), md, fmt, boost, threads=2)
        assert st == 0, st
        runs.append(out[:orc.out_bytes_per_image(fmt, w, h)].copy())
    if fmt in (FMT_PQ, FMT_HLG):
        r = [a.view(np.uint32) for a in runs]
        out = (r[0] & np.uint32(0x3ff)) | (r[1] & np.uint32(0x3ff << 10)) | (r[2] & np.uint32(0x3ff << 20)) | (r[0] & np.uint32(0xC0000000))
        return out.view(np.uint8)
    if fmt == FMT_F16:
        r = [a.view(np.uint16).reshape(-1, 4) for a in runs]
        out = r[0].copy()
        out[:, 1] = r[1][:, 1]
        out[:, 2] = r[2][:, 2]
        return out.reshape(-1).view(np.uint8)
    r = [a.view(np.uint16).reshape(3, -1) for a in runs]
    return np.stack([r[0][0], r[1][1], r[2][2]]).reshape(-1).view(np.uint8)


def lcg_pair(orc, w, h, seed, sdr_gamut, hdr_gamut, pad=0):
    """an LCG pair as oracle images; pad > 0: luma rows `pad` samples longer and chroma rows pad / 2 (8-bit) / pad (P010) longer, the
    planes apart.  Returns (yuv image, p010 image, the arrays that back them)"""
    p010, yuv = orc.lcg_frame(w, h, seed)
    if pad == 0:
        return orc.yuv420_image(yuv, w, h, sdr_gamut), orc.p010_image(p010, w, h, hdr_gamut), (p010, yuv)
    ls, cs = w + pad, w // 2 + pad // 2
    y = np.full((h, ls), 0xEE, np.uint8)
    y[:, :w] = yuv[:w * h].reshape(h, w)
    uv = np.full((h, cs), 0xEE, np.uint8)     # U rows then V rows, V at chroma_stride * (h / 2)
    uv[:, :w // 2] = yuv[w * h:].reshape(h, w // 2)
    hy = np.full((h, ls), 0xEEEE, np.uint16)
    hy[:, :w] = p010[:w * h].reshape(h, w)
    huv = np.full((h // 2, ls), 0xEEEE, np.uint16)
    huv[:, :w] = p010[w * h:].reshape(h // 2, w)
    yi = orc.yuv420_image(y, w, h, sdr_gamut, luma_stride=ls, chroma_stride=cs, chroma=uv)
    pi = orc.p010_image(hy, w, h, hdr_gamut, luma_stride=ls, chroma_stride=ls, chroma=huv)
    return yi, pi, (y, uv, hy, huv)


def orc_metadata(orc, max_boost):
    return orc.Metadata(max_boost, 1.0, 1.0, 0.0, 0.0, 1.0, max_boost, 1)


@functools.lru_cache(maxsize=None)
def golden_rgb(w, h):
    a = np.load(os.path.join(DIR, "rgb_%dx%d.npy" % (w, h)))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def golden_jpeg(w, h, q):
    """Pillow's subsampling=0 file of golden_rgb(w, h) at quality q"""
    return open(os.path.join(DIR, "rgb_%dx%d_q%d.jpg" % (w, h, q)), "rb").read()


@functools.lru_cache(maxsize=None)
def golden_jpeg_420(w, h):
    return open(os.path.join(DIR, "rgb_%dx%d_s2.jpg" % (w, h)), "rb").read()


def from_first_dqt(data):
    """the JPEG from its first DQT marker on: what is left of a file when the segments in front (JFIF, ICC, EXIF, XMP, MPF) are set aside"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    i = 2
    while data[i + 1] != 0xDB:   # marker segments: FF xx, 16-bit length
        assert data[i] == 0xFF and data[i + 1] not in (0xDA, 0xD9), "no DQT in front of the scan"
        i += 2 + int.from_bytes(data[i + 2:i + 4], "big")
    return data[i:]
