"""Content-adaptive gain maps: the expected values, restated per map pixel from the oracle's existing primitives.

`luminances` is generate's loop body up to encodeGain (ultrahdr.cpp:316-330): sampleYuv420 / sampleP010 at scale 4, yuvToRgb, the
inverse OETFs, gamutConv, luminance, x 203 / x white in np.float32.  `encode` is the reference's three-argument encodeGain on those
luminances; `gains` the unclamped f32 gain of gainmapmath.cpp:531-534; `rule` the range rule of include/uhdr_hip.h in np.float32.
At the reference's constants this reproduces orc_generateGainMap byte for byte and orc_generateGainMapStats' pair bit for bit
(tests/test_adaptive_cpu.py checks that first).  ~20 us per map pixel: keep the images small and share the results.
"""
import ctypes as C

import numpy as np

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = 0, 1, 2
CG_709, CG_P3, CG_2100 = 0, 1, 2


def cap(tf):
    return F(10000.0 if tf == TF_PQ else 1000.0) / F(203.0)


def rule(tf, g_min, g_max):
    """(lo, hi) as np.float32: fminf(fmaxf(g_min, 0.25), 1), fminf(fmaxf(g_max, 1.0625), cap) -- fmax / fmin drop a NaN operand"""
    with np.errstate(invalid="ignore"):
        lo = np.fmin(np.fmax(F(g_min), F(0.25)), F(1.0))
        hi = np.fmin(np.fmax(F(g_max), F(1.0625)), cap(tf))
    return F(lo), F(hi)


def luminances(orc, yuv_img, p010_img, tf, sdr_is_601=False):
    """(y_sdr, y_hdr): two float32 arrays of the map's shape, exactly the luminances generateGainMap hands to encodeGain"""
    L = orc.load()
    mw, mh = yuv_img.width // 4, yuv_img.height // 4
    sdr_gamut, hdr_gamut = yuv_img.colorGamut, p010_img.colorGamut
    sdr_yuv_gamut = CG_P3 if sdr_is_601 else sdr_gamut
    inv = {TF_LINEAR: None, TF_HLG: L.orc_hlgInvOetf, TF_PQ: L.orc_pqInvOetf}[tf]
    white = F(10000.0 if tf == TF_PQ else 1000.0)
    ys, yh = np.empty((mh, mw), F), np.empty((mh, mw), F)
    yi, pi = C.byref(yuv_img), C.byref(p010_img)
    Color, srgb = orc.Color, L.orc_srgbInvOetf
    for y in range(mh):
        for x in range(mw):
            e = L.orc_yuvToRgb(sdr_yuv_gamut, L.orc_sampleYuv420(yi, 4, x, y))
            e = Color(srgb(e.r), srgb(e.g), srgb(e.b))
            ys[y, x] = F(L.orc_luminance(sdr_gamut, e)) * F(203.0)
            e = L.orc_yuvToRgb(hdr_gamut, L.orc_sampleP010(pi, 4, x, y))
            if inv is not None:
                e = Color(inv(e.r), inv(e.g), inv(e.b))
            e = L.orc_gamutConv(sdr_gamut, hdr_gamut, e, None)
            yh[y, x] = F(L.orc_luminance(sdr_gamut, e)) * white
    return ys, yh


def gains(ys, yh):
    """gainmapmath.cpp:531-534: 1 where y_sdr <= 0, else y_hdr / y_sdr, in f32"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ys > 0, yh / np.where(ys > 0, ys, F(1.0)), F(1.0)).astype(F)


def minmax(ys, yh):
    g = gains(ys, yh)
    return F(g.min()), F(g.max())


def encode(orc, ys, yh, lo, hi):
    """encodeGain(y_sdr, y_hdr, metadata) with minContentBoost = lo, maxContentBoost = hi, per pixel"""
    fn = orc.load().orc_encodeGain3
    lo, hi = float(lo), float(hi)
    out = np.empty(ys.shape, np.uint8)
    flat_s, flat_h, flat_o = ys.reshape(-1), yh.reshape(-1), out.reshape(-1)
    for i in range(flat_s.size):
        flat_o[i] = fn(float(flat_s[i]), float(flat_h[i]), lo, hi)
    return out


def recovery_error(gmap, lo, hi, g):
    """mean and max of |log2(recovered gain) - log2(gain)| over the map; recovered = 2^(log2 lo + (log2 hi - log2 lo) byte / 255)"""
    l0, l1 = np.log2(np.float64(lo)), np.log2(np.float64(hi))
    rec = l0 + (l1 - l0) * gmap.astype(np.float64) / 255.0
    d = np.abs(rec - np.log2(g.astype(np.float64)))
    return float(d.mean()), float(d.max())


def graded_pair(orc, w, h):
    """a P010 luma ramp 64 + 200 + ((5 x + 3 y) mod 400), chroma 512, and SDR = toneMap of it: (p010 uint16, yuv uint8), packed"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    p010 = np.empty(w * h * 3 // 2, np.uint16)
    p010[:w * h] = ((64 + 200 + ((5 * x + 3 * y) % 400)) << 6).reshape(-1)
    p010[w * h:] = 512 << 6
    yuv = np.zeros(w * h * 3 // 2, np.uint8)
    src = orc.p010_image(p010, w, h, CG_2100)
    dst = orc.yuv420_image(yuv, w, h, CG_2100)
    assert orc.load().orc_toneMap(C.byref(src), C.byref(dst)) == 0
    return p010, yuv


def flat_pair(w, h, p_luma, y_luma):
    """every sample the same: P010 luma code p_luma (10 bit) over chroma 512, 8-bit luma y_luma over chroma 128"""
    p010 = np.empty(w * h * 3 // 2, np.uint16)
    p010[:w * h] = p_luma << 6
    p010[w * h:] = 512 << 6
    yuv = np.empty(w * h * 3 // 2, np.uint8)
    yuv[:w * h] = y_luma
    yuv[w * h:] = 128
    return p010, yuv


def metadata_tuple(md):
    return (md.version, md.maxContentBoost, md.minContentBoost, md.gamma, md.offsetSdr, md.offsetHdr, md.hdrCapacityMin, md.hdrCapacityMax)


def xmp_round_trip(orc, api, md):
    """md after what a file can carry of it: written into a gain map's XMP (log2 of the boosts with %g) and parsed back.  Through the
    product's host code -- uhdr_hip_jpegr_encode_api4, then uhdr_hip_jpegr_metadata -- wherever API-4 takes the metadata.  Like the
    reference's appendGainMap (jpegr.cpp:971) it refuses hdrCapacityMin < 1, which an adaptive range with lo < 1 has (applyGainMap,
    ultrahdr.cpp:381, wants hdrCapacityMin == minContentBoost): those go through the restatement's writer and parser
    (oracle/jpegr_oracle.py, pinned to the reference's by tests/test_ref_container.py)."""
    from oracle import jpegr_oracle as J
    d = dict(version=md.version.decode(), max=F(md.maxContentBoost), min=F(md.minContentBoost), gamma=F(md.gamma), off_sdr=F(md.offsetSdr),
             off_hdr=F(md.offsetHdr), capmin=F(md.hdrCapacityMin), capmax=F(md.hdrCapacityMax))
    back = J.metadata_from_xmp(J.XMP_NS + J.xmp_secondary(d).encode())
    want = api.Metadata(back["version"].encode(), back["max"], back["min"], back["gamma"], back["off_sdr"], back["off_hdr"], back["capmin"],
                        back["capmax"])
    lib = api.load()
    y, uv = np.full(16 * 16, 100, np.uint8), np.full(16 * 8, 128, np.uint8)
    p = np.frombuffer(orc.jpeg_encode("orc", y, uv, 16, 16, 90), np.uint8)
    g = np.frombuffer(orc.jpeg_encode("orc", y[:16], None, 4, 4, 85), np.uint8)
    out, n, got = np.zeros(1 << 16, np.uint8), C.c_size_t(), api.Metadata()
    rc = lib.uhdr_hip_jpegr_encode_api4(C.c_void_p(p.ctypes.data), p.size, api.CG_BT709, C.c_void_p(g.ctypes.data), g.size, C.byref(md),
                                        C.c_void_p(out.ctypes.data), out.size, C.byref(n))
    if md.hdrCapacityMin < 1.0:
        assert rc == api.ERROR_BAD_METADATA, rc
        return want
    assert rc == 0, rc
    assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(out.ctypes.data), n.value, C.byref(got)) == 0
    assert metadata_tuple(got) == metadata_tuple(want)
    return got
