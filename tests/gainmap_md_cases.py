"""Gain maps with gamma, offsets and an HDR capacity range (include/uhdr_hip.h): the model and the cases, not
a test file.  There is no reference code for this arithmetic; the header's formula is the contract and this is it in numpy float64.

Apply.  Per pixel the linear SDR colour e comes from the oracle's getYuv420Pixel, yuvToRgb (BT.601) and srgbInvOetf -- evaluated once
per distinct (Y, U, V) code triple, so every chroma sampling goes through the same three functions -- and the gain g from the
oracle's sampleMapIdw; the formula, the OETF and the scaling to codes are float64.  The model keeps v, the value in front of the
truncation, per channel: OETF(out) * 1023 for the 10-bit formats, out itself for F16.

Generate.  The luminances (tests/adaptive_cases.py) or linear colours (as tests/rgbmap_cases.py forms them) carry the f32 values the
device carries; the offsets, the division and the clamp are np.float32 as the header writes them; log2 and pow are float64.

Images.  The shape tests run on plain LCG pairs: full-range codes, a good share of channels clamped by yuvToRgb at 0 or 1.  Such a
channel is exactly 0 whenever offsetSdr is 0 or the exponent is (W = 0), i.e. an exact integer in front of the truncation.  The input
condition of tests/test_gainmap_md_cpu.py and the differing shares of tests/test_gpu_gainmap_md.py therefore use the 264 x 200 LCG
pair with its SDR codes FOLDED into the range where yuvToRgb clamps nothing (folded_pair): no channel is an integer by construction.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = 0, 1, 2
CG_709, CG_P3, CG_2100 = 0, 1, 2
FMT_F16, FMT_PQ, FMT_HLG, FMT_RGB10 = 1, 2, 3, 4
FLT_MAX = 3.4028234663852886e38
DOUBT = 1.0 / 256.0          # apply: a channel whose v lies this close to an integer may come out one code off
GEN_DOUBT = 2.0 ** -30       # generate: the same for a map byte

# (gamma, offsetSdr, offsetHdr, minContentBoost, maxContentBoost, hdrCapacityMin, hdrCapacityMax)
CASES = {
    "default": (1.0, 1 / 64, 1 / 64, 1.0, 4.926, 1.0, 4.926),      # what current libultrahdr writes
    "gamma22": (2.2, 1 / 64, 1 / 64, 1.0, 4.926, 1.0, 4.926),
    "black": (0.5, 0.0, 1 / 32, 0.5, 8.0, 1.5, 6.0),               # results that clamp at black, log2 min < 0, capacity != content
    "flatcap": (1.0, 1 / 64, 0.0, 1.0, 49.26, 2.0, 2.0),           # hdrCapacityMin == hdrCapacityMax
}
# display boosts per case: W = 0, strictly inside (0, 1) where the case has an inside, 1, and one capped above hdrCapacityMax
BOOSTS = {
    "default": (1.0, 2.0, 4.926, 100.0),
    "gamma22": (1.0, 2.0, 4.926, FLT_MAX),
    "black": (1.0, 3.0, 6.0, FLT_MAX),
    "flatcap": (1.5, 2.0, 8.0),
}
DEGENERATE = (1.0, 0.0, 0.0, 1.0, 4.926, 1.0, 4.926)
# seeds of the 264 x 200 pair and of its map, chosen so that the input conditions of tests/test_gainmap_md_cpu.py hold
SHARE_SEED, SHARE_MAP_SEED = 1234, 77


def fields(case):
    """the seven numbers as np.float32, what a uhdr_hip_metadata_t holds"""
    return tuple(F(v) for v in case)


def api_metadata(api, case, version=b"1.0"):
    g, os_, oh, lo, hi, hmin, hmax = case
    return api.Metadata(version, hi, lo, g, os_, oh, hmin, hmax)


def orc_metadata(case):
    g, os_, oh, lo, hi, hmin, hmax = case
    return O.Metadata(hi, lo, g, os_, oh, hmin, hmax, 1)


def is_degenerate(case):
    g, os_, oh, lo, hi, hmin, hmax = fields(case)
    return bool(g == 1 and os_ == 0 and oh == 0 and hmin == lo and hmax == hi)


def weight(case, boost):
    """(W, d) in float64 from the float32 fields"""
    g, os_, oh, lo, hi, hmin, hmax = (float(v) for v in fields(case))
    D = float(F(boost))
    if hmax == hmin:
        w = 1.0 if D >= hmax else 0.0
    else:
        w = min(max((np.log2(D) - np.log2(hmin)) / (np.log2(hmax) - np.log2(hmin)), 0.0), 1.0)
    return float(w), min(D, hmax)


# ------------------------------------------------------------------ images

def lcg_yuv(w, h, seed):
    """the SDR half of an LCG pair as planes: Y (h, w), U, V (h / 2, w / 2)"""
    _, yuv = O.lcg_frame(w, h, seed)
    return (yuv[:w * h].reshape(h, w).copy(), yuv[w * h:w * h * 5 // 4].reshape(h // 2, w // 2).copy(),
            yuv[w * h * 5 // 4:].reshape(h // 2, w // 2).copy())


def folded_pair(w, h, seed):
    """the LCG pair (p010, yuv) with the SDR codes folded into Y in [96, 223], Cb / Cr in [116, 139]: yuvToRgb clamps no channel, and the
    darkest one (75 / 255, linear 0.07) stays above the black clamp of every case (`black`: 0.07 x minContentBoost 0.5 > offsetHdr 1 / 32)"""
    p010, yuv = O.lcg_frame(w, h, seed)
    yuv = yuv.copy()
    yuv[:w * h] = 96 + yuv[:w * h] % 128
    yuv[w * h:] = 116 + yuv[w * h:] % 24
    return p010, yuv


def planes_of(yuv, w, h):
    return (yuv[:w * h].reshape(h, w), yuv[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), yuv[w * h * 5 // 4:].reshape(h // 2, w // 2))


def lcg_bytes(shape, seed):
    """map bytes from the same generator, with 0 and 255 present"""
    n = int(np.prod(shape))
    s, out = seed & 0xFFFFFFFF, np.empty(n, np.uint8)
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (s >> 16) & 255
    out[0], out[-1] = 0, 255
    return out.reshape(shape)


def chroma_planes(w, h, sampling, seed):
    """(Y, U, V, csx, csy) with chroma planes of the sampling's size: '420', '444', '422', '440' (libjpeg's rounded-up sizes)"""
    csx, csy = {"420": (1, 1), "444": (0, 0), "422": (1, 0), "440": (0, 1)}[sampling]
    cw = w // 2 if sampling == "420" else (w + (1 << csx) - 1) >> csx
    ch = h // 2 if sampling == "420" else (h + (1 << csy) - 1) >> csy
    return lcg_bytes((h, w), seed), lcg_bytes((ch, cw), seed + 1), lcg_bytes((ch, cw), seed + 2), csx, csy


# ------------------------------------------------------------------ the apply model

def _linear_sdr(codes):
    """srgbInvOetf(yuvToRgb_601(getYuv420Pixel)) of the oracle for (n, 3) uint8 (Y, U, V) triples -> (n, 3) float32"""
    n = codes.shape[0]
    luma = np.zeros((2 * n, 2), np.uint8)
    luma[0::2, 0] = codes[:, 0]
    chroma = np.zeros((2 * n, 1), np.uint8)   # U rows, then V rows at chroma_stride * (height / 2)
    chroma[:n, 0] = codes[:, 1]
    chroma[n:, 0] = codes[:, 2]
    img = O.yuv420_image(luma, 2, 2 * n, CG_709, luma_stride=2, chroma_stride=1, chroma=chroma)
    L = O.load()
    get, rgb, srgb = L.orc_getYuv420Pixel, L.orc_yuvToRgb, L.orc_srgbInvOetf
    out = np.empty((n, 3), F)
    ref = C.byref(img)
    for i in range(n):
        c = rgb(CG_P3, get(ref, 0, 2 * i))
        out[i] = (srgb(c.r), srgb(c.g), srgb(c.b))
    return out


def linear_sdr(Y, U, V, csx=1, csy=1):
    """(h, w, 3) float32: the linear SDR colour of every pixel, pixel (x, y) taking the chroma sample (x >> csx, y >> csy)"""
    h, w = Y.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = U[yy >> csy, xx >> csx], V[yy >> csy, xx >> csx]
    key = (Y.astype(np.uint32) << 16) | (u.astype(np.uint32) << 8) | v.astype(np.uint32)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    codes = np.stack([(uniq >> 16) & 255, (uniq >> 8) & 255, uniq & 255], axis=1).astype(np.uint8)
    return _linear_sdr(codes)[inv.reshape(-1)].reshape(h, w, 3)


def sampled_gain(gmap, w, h):
    """(h, w, C) float32: sampleMapIdw of the oracle per pixel and map plane; gmap (mh, mw) or (mh, mw, C) uint8"""
    if gmap.ndim == 2:
        gmap = gmap[:, :, None]
    mh, mw, nc = gmap.shape
    scale = w // mw
    fn = O.load().orc_sampleMapIdw
    out = np.empty((h, w, nc), F)
    for c in range(nc):
        plane = np.ascontiguousarray(gmap[:, :, c])
        ref = C.byref(O.map_image(plane, mw, mh))
        for y in range(h):
            for x in range(w):
                out[y, x, c] = fn(ref, scale, x, y)
    return out


def sampled_gain_by_tables(gmap, w, h):
    """sampled_gain without a call per pixel, for the factors at which orc_sampleMapIdw -- it builds its four weight tables on every
    call -- takes minutes: the oracle's tables (orc_fillShepardsIDW), then sampleMap's tap choice and its float32 sum
    (gainmapmath.cpp:686-720) in numpy.  Bit-identical to sampled_gain (tests/test_gainmap_md_cpu.py holds it to that)"""
    if gmap.ndim == 2:
        gmap = gmap[:, :, None]
    mh, mw, nc = gmap.shape
    s = w // mw
    fill = O.load().orc_fillShepardsIDW
    tables = np.empty((4, s, s, 4), F)   # all taps, no right tap, no bottom tap, the corner
    for t, (inc_r, inc_b) in enumerate(((1, 1), (0, 1), (1, 0), (0, 0))):
        fill(tables[t].ctypes.data_as(C.POINTER(C.c_float)), s, inc_r, inc_b)
    x, y = np.arange(w), np.arange(h)
    xl, yl = np.minimum(x // s, mw - 1), np.minimum(y // s, mh - 1)
    xu, yu = np.minimum(x // s + 1, mw - 1), np.minimum(y // s + 1, mh - 1)
    same_x, same_y = (xl == xu)[None, :], (yl == yu)[:, None]
    tbl = np.where(same_x & same_y, 3, np.where(same_x, 1, np.where(same_y, 2, 0)))
    wt = tables[tbl, (y % s)[:, None], (x % s)[None, :]]                       # (h, w, 4)
    e = gmap.astype(F) / F(255.0)                                              # mapUintToFloat
    out = np.empty((h, w, nc), F)
    for c in range(nc):
        p = e[:, :, c]
        e1, e2 = p[yl[:, None], xl[None, :]], p[yu[:, None], xl[None, :]]
        e3, e4 = p[yl[:, None], xu[None, :]], p[yu[:, None], xu[None, :]]
        out[:, :, c] = e1 * wt[:, :, 0] + e2 * wt[:, :, 1] + e3 * wt[:, :, 2] + e4 * wt[:, :, 3]
    return out


def _oetf(fmt, x):
    """the reference's OETFs in float64 (its float constants, as doubles); x >= 0"""
    x = np.asarray(x, np.float64)
    if fmt == FMT_HLG:
        a, b, c = float(F(0.17883277)), float(F(0.28466892)), float(F(0.55991073))
        return np.where(x <= 1.0 / 12.0, np.sqrt(3.0 * x), a * np.log(np.maximum(12.0 * x - b, 1e-300)) + c)
    if fmt == FMT_PQ:
        m1, m2 = float(F(2610.0) / F(16384.0)), float(F(2523.0) / F(4096.0) * F(128.0))
        c1, c2, c3 = float(F(3424.0) / F(4096.0)), float(F(2413.0) / F(4096.0) * F(32.0)), float(F(2392.0) / F(4096.0) * F(32.0))
        p = np.power(x, m1)
        return np.where(x <= 0.0, 0.0, np.power((c1 + c2 * p) / (1.0 + c3 * p), m2))
    return x


def linear_out(e, g, case, boost):
    """the header's out_c in float64: e (h, w, 3), g (h, w, 1 or 3)"""
    gamma, os_, oh, lo, hi, _, _ = (float(v) for v in fields(case))
    W, d = weight(case, boost)
    g = g.astype(np.float64)
    gp = g if gamma == 1.0 else np.power(g, 1.0 / gamma)
    ex = (np.log2(lo) * (1.0 - gp) + np.log2(hi) * gp) * W
    return np.maximum(0.0, (e.astype(np.float64) + os_) * np.exp2(ex) - oh) / d


def pre_truncation(e, g, case, boost, fmt):
    """v per channel (h, w, 3) float64: OETF(out) * 1023 for the 10-bit formats, out for F16"""
    out = linear_out(e, g, case, boost)
    return out if fmt == FMT_F16 else _oetf(fmt, out) * 1023.0


def codes_of(raw, fmt, w, h):
    """the device's (or the oracle's) output bytes as (h, w, 3) integers: 10-bit codes, or half-precision bit patterns (F16)"""
    if fmt in (FMT_PQ, FMT_HLG):
        p = np.ascontiguousarray(raw).view(np.uint32)[:w * h].reshape(h, w)
        return np.stack([p & 0x3ff, (p >> 10) & 0x3ff, (p >> 20) & 0x3ff], axis=2).astype(np.int64)
    if fmt == FMT_F16:
        return np.ascontiguousarray(raw).view(np.uint16)[:w * h * 4].reshape(h, w, 4)[:, :, :3].astype(np.int64)
    return np.ascontiguousarray(raw).view(np.uint16)[:3 * w * h].reshape(3, h, w).transpose(1, 2, 0).astype(np.int64)


def code_distance(codes, v):
    """|code - floor(v)| per channel under the formats' `& 0x3ff`"""
    d = (codes - np.floor(v).astype(np.int64)) & 0x3ff
    return np.minimum(d, 1024 - d)


def half_ulp_distance(bits, v):
    """how many half-precision ULPs the pattern `bits` lies from the float64 value v (both >= 0): positive halves order as integers"""
    with np.errstate(over="ignore"):
        want = np.asarray(v, np.float64).astype(np.float16)
    got = bits.astype(np.uint16).view(np.float16).astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    return np.abs(got - np.asarray(v, np.float64)) / ulp


def near_integer(v, doubt=DOUBT):
    return np.abs(v - np.rint(v)) < doubt


# ------------------------------------------------------------------ the generate model

def encode(ys, yh, case):
    """(bytes uint8, v float64): the header's rule on two float32 arrays of SDR / HDR values in nits"""
    gamma, os_, oh, lo, hi, _, _ = fields(case)
    a = (ys.astype(F) + os_ * F(203.0)).astype(F)
    b = (yh.astype(F) + oh * F(203.0)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = np.where(a > 0, b / np.where(a > 0, a, F(1.0)), F(1.0)).astype(F)
    gain = np.minimum(np.maximum(gain, lo), hi)   # (gain < min -> min; gain > max -> max, as encodeGain)
    l2lo, l2hi = F(np.log2(np.float64(lo))), F(np.log2(np.float64(hi)))
    t = (np.log2(gain.astype(np.float64)) - np.float64(l2lo)) / np.float64(l2hi - l2lo)
    if gamma == 1:
        v = t * 255.0
    else:
        v = np.power(np.maximum(t, 0.0), np.float64(gamma)) * 255.0
    return np.minimum(np.trunc(v), 255).astype(np.int64).astype(np.uint8), v


def linear_colours(orc, yuv_img, p010_img, tf, sdr_is_601=False):
    """(sdr, hdr): two (mh, mw, 3) float32 arrays, the linear colours generate encodes per channel, in nits"""
    L = orc.load()
    mw, mh = yuv_img.width // 4, yuv_img.height // 4
    sdr_gamut, hdr_gamut = yuv_img.colorGamut, p010_img.colorGamut
    sdr_yuv_gamut = CG_P3 if sdr_is_601 else sdr_gamut
    inv = {TF_LINEAR: None, TF_HLG: L.orc_hlgInvOetf, TF_PQ: L.orc_pqInvOetf}[tf]
    white = F(10000.0 if tf == TF_PQ else 1000.0)
    s, hh = np.empty((mh, mw, 3), F), np.empty((mh, mw, 3), F)
    yi, pi = C.byref(yuv_img), C.byref(p010_img)
    Color, srgb = orc.Color, L.orc_srgbInvOetf
    for y in range(mh):
        for x in range(mw):
            e = L.orc_yuvToRgb(sdr_yuv_gamut, L.orc_sampleYuv420(yi, 4, x, y))
            s[y, x] = (srgb(e.r), srgb(e.g), srgb(e.b))
            e = L.orc_yuvToRgb(hdr_gamut, L.orc_sampleP010(pi, 4, x, y))
            if inv is not None:
                e = Color(inv(e.r), inv(e.g), inv(e.b))
            hh[y, x] = L.orc_gamutConv(sdr_gamut, hdr_gamut, e, None).tup()
    return (s * F(203.0)).astype(F), (hh * white).astype(F)


def generate_seed(w, tf):
    """seeds of the generate pairs, chosen so that the input condition of tests/test_gainmap_md_cpu.py holds"""
    return {712: 1300}.get(w, 500 + w) + tf   # (712: 500 + w leaves one luminance byte 3e-10 from an integer under `gamma22`)


@functools.lru_cache(maxsize=None)
def generate_inputs(w, h, tf):
    """the plain LCG pair of this size and transfer function (BT.709 SDR, BT.2100 HDR) and what the model encodes: computed once"""
    from tests import adaptive_cases as A
    p010, yuv = O.lcg_frame(w, h, generate_seed(w, tf))
    yi, pi = O.yuv420_image(yuv, w, h, CG_709), O.p010_image(p010, w, h, CG_2100)
    ys, yh = A.luminances(O, yi, pi, tf)
    sdr, hdr = linear_colours(O, yi, pi, tf)
    for a in (p010, yuv, ys, yh, sdr, hdr):
        a.setflags(write=False)
    return dict(p010=p010, yuv=yuv, ys=ys, yh=yh, sdr=sdr, hdr=hdr)


def in_doubt(v):
    """generate: the map pixels whose byte may differ by one -- the value in front of the truncation within 2^-30 of an integer.  A gain
    on either clamp is not among them: its byte is computed on the host by the rule itself (v is 0 or 255 to the last bit there, an
    integer by construction, and plain LCG pairs clamp a good share of their gains)."""
    return near_integer(v, GEN_DOUBT) & (v > 0) & (v < 255)


@functools.lru_cache(maxsize=None)
def share_inputs():
    """the 264 x 200 folded pair, its map and the model's per-pixel inputs (e, g one plane, g three planes), computed once"""
    w, h = 264, 200
    p010, yuv = folded_pair(w, h, SHARE_SEED)
    gmap = lcg_bytes((h // 4, w // 4, 3), SHARE_MAP_SEED)
    Y, U, V = planes_of(yuv, w, h)
    e = linear_sdr(Y, U, V)
    g3 = sampled_gain(gmap, w, h)
    return dict(w=w, h=h, p010=p010, yuv=yuv, gmap=gmap, e=e, g1=g3[:, :, :1].copy(), g3=g3)
