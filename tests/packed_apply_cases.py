"""Packed apply (include/uhdr_hip.h, uhdr_hip_apply_gainmap_packed_batch): the expected values and the
inputs, not a test file.

Degenerate metadata.  The contract is separability: every step of applyGainMap behind the pixel value is per channel, and a grey
pixel (Y, 128, 128) passes yuvToRgb as (Y / 255, Y / 255, Y / 255) -- the chroma terms are products with 0.0f.  So channel c of the
packed rendition is channel c of the oracle's applyGainMap run on the grey image whose Y plane is plane c of the RGBA image (an RGBA
map: with plane c of the map), which `composite` does the way rgbmap_cases.composite_apply does it for maps.  `from_primitives`
is the same value composed per pixel from the oracle's scalar functions; tests/test_packed_apply_cpu.py holds the two together.

General metadata reuses gainmap_md_cases' float64 model with srgbInvOetf(code / 255) as the linear SDR value (`linear_sdr`).
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from tests import gainmap_md_cases as M

F = np.float32
FMT_F16, FMT_PQ, FMT_HLG, FMT_RGB10 = 1, 2, 3, 4
FORMATS = (FMT_F16, FMT_PQ, FMT_HLG, FMT_RGB10)
FLT_MAX = M.FLT_MAX
CONTENT_BOOST = 4.0
BOOSTS = (FLT_MAX, 2.0, 1.0)
K255 = F(1.0) / F(255.0)   # the C constant 1 / 255.0f


def orc_metadata(max_boost=CONTENT_BOOST, min_boost=1.0):
    return O.Metadata(max_boost, min_boost, 1.0, 0.0, 0.0, min_boost, max_boost, 1)


def lcg_rgba(w, h, seed):
    """(h, w, 4) uint8 from the oracle's LCG: the luma plane of a 4 w x h frame, full-range bytes"""
    _, yuv = O.lcg_frame(4 * w, h, seed)
    return yuv[:4 * w * h].reshape(h, w, 4).copy()


def lcg_map(mw, mh, seed, channels=1):
    m = M.lcg_bytes((mh, mw, channels), seed)
    return m[:, :, 0].copy() if channels == 1 else m


def all_codes_rgba():
    """64 x 64: each of the three channels takes all 256 codes (every entry of the table is read by every channel)"""
    i = np.arange(64 * 64)
    px = np.stack([i % 256, (i * 7 + 3) % 256, 255 - (i * 13) % 256, (i * 5) % 256], axis=1).astype(np.uint8)
    return px.reshape(64, 64, 4)


def all_codes_map():
    """16 x 16: all 256 bytes"""
    return ((np.arange(256) * 37 + 11) % 256).astype(np.uint8).reshape(16, 16)


def _grey_image(plane, w, h):
    """the oracle's 4:2:0 image of one plane as Y with chroma planes of 128s: rounded-up strides, and rows to spare behind the
    height / 2 the reference assumes, so that the last row and column of an odd size read 128 too"""
    cs = (w + 1) // 2
    chroma = np.full(cs * (2 * ((h + 1) // 2) + 2), 128, np.uint8)
    y = np.ascontiguousarray(plane)
    return O.yuv420_image(y, w, h, O.CG_BT709, luma_stride=w, chroma_stride=cs, chroma=chroma), (y, chroma)


def merge_channels(runs, fmt):
    """channel c of run c as one output (the alpha of RGBA1010102 / F16 from run 0: every run writes the same)"""
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


def composite(rgba, gmap, fmt, boost, md=None):
    """the packed rendition's bytes: three runs of the oracle's applyGainMap on grey images, channel c from run c; gmap (mh, mw) or
    (mh, mw, >= 3) uint8"""
    md = md or orc_metadata()
    h, w = rgba.shape[:2]
    runs = []
    for c in range(3):
        img, keep = _grey_image(rgba[:, :, c], w, h)
        plane = np.ascontiguousarray(gmap if gmap.ndim == 2 else gmap[:, :, c])
        st, out, _ = O.apply("orc_", img, plane, md, fmt, boost, threads=2)
        assert st == 0, st
        runs.append(out.copy())
        del keep
    out = merge_channels(runs, fmt)
    out.setflags(write=False)
    return out


def from_primitives(rgba, gmap, fmt, boost, max_boost=CONTENT_BOOST, min_boost=1.0):
    """the same bytes from the oracle's scalar functions, pixel by pixel: ultrahdr.cpp:429-489 with the packed pixel's codes in place
    of lines 429-431"""
    L = O.load()
    h, w = rgba.shape[:2]
    planes = [np.ascontiguousarray(gmap if gmap.ndim == 2 else gmap[:, :, c]) for c in range(3)]
    mh, mw = planes[0].shape
    maps = [O.map_image(p, mw, mh) for p in planes]
    scale = w // mw
    db = float(min(F(boost), F(max_boost)))
    oetf = {FMT_HLG: L.orc_hlgOetf, FMT_PQ: L.orc_pqOetf}.get(fmt)
    words = np.zeros((h, w), np.uint64)
    for y in range(h):
        for x in range(w):
            ch = []
            for c in range(3):
                e = L.orc_srgbInvOetf(float(F(rgba[y, x, c]) * K255))
                g = L.orc_sampleMapIdw(C.byref(maps[c]), scale, x, y)
                v = L.orc_applyGain4(O.Color(e, e, e), g, min_boost, max_boost, db).tup()[c]
                v = float(F(v) / F(db))
                ch.append(oetf(v) if oetf else v)
            col = O.Color(*ch)
            words[y, x] = L.orc_colorToRgbaF16(col) if fmt == FMT_F16 else L.orc_colorToRgba1010102(col)
    if fmt == FMT_F16:
        return words.reshape(-1).view(np.uint8)
    if fmt == FMT_RGB10:
        p = words.astype(np.uint32)
        return np.stack([p & 0x3ff, (p >> 10) & 0x3ff, (p >> 20) & 0x3ff]).astype(np.uint16).reshape(-1).view(np.uint8)
    return words.astype(np.uint32).reshape(-1).view(np.uint8)


@functools.lru_cache(maxsize=None)
def srgb_table():
    """srgbInvOetf((float)code * (1 / 255.0f)) of the oracle for the 256 codes"""
    fn = O.load().orc_srgbInvOetf
    t = np.array([fn(float(F(c) * K255)) for c in range(256)], F)
    t.setflags(write=False)
    return t


def linear_sdr(rgba):
    """(h, w, 3) float32: the linear SDR colour of a packed image, what gainmap_md_cases' model starts from"""
    return srgb_table()[rgba[:, :, :3]]


def fast_distance(got, want, fmt, w, h, wrap):
    """the largest distance between two outputs in FAST's units: 10-bit codes (modulo 1024 where the call's boost lies below the
    content's: only then can a channel pass 1.0 and wrap through the reference's & 0x3ff) or half-precision bit patterns"""
    a, b = M.codes_of(got, fmt, w, h), M.codes_of(want, fmt, w, h)
    d = np.abs(a - b)
    if fmt != FMT_F16 and wrap:
        d = np.minimum(d, 1024 - d)
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0
