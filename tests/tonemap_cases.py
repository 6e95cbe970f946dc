"""The tone-mapped SDR base image of include/uhdr_hip.h as a model (not a test file): what tests/test_tonemap_cpu.py and
tests/test_gpu_tonemap.py hold uhdr_hip_tonemap_headroom and the device's planes to.

Steps 1-2 and 7 of the operator go through the CPU oracle's getP010Pixel, yuvToRgb, hlgInvOetf / pqInvOetf and rgbToYuv, so they carry
the f32 values the device carries; steps 4-6 and 8 are numpy float64, except H, which is formed in float32 exactly as the header
writes it.  The oracle is called once per distinct (Y, U, V) code triple of a frame, not once per pixel.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = O.TF_LINEAR, O.TF_HLG, O.TF_PQ
CG_709, CG_P3, CG_2100 = O.CG_BT709, O.CG_P3, O.CG_BT2100
SHIFT, REINHARD = 0, 1
SWING8 = 184.0   # (see planes())
DOUBT = 1.0 / 256.0   # a sample whose pre-truncation value lies this close to an integer may differ by one code


def white(tf):
    return F(10000.0) if tf == TF_PQ else F(1000.0)


def k_of(tf):
    return white(tf) / F(203.0)


def inv_oetf(tf, x):
    """the oracle's inverse OETF of hdr_tf over a float32 array (LINEAR: the identity)"""
    x = np.ascontiguousarray(x, F)
    if tf == TF_LINEAR:
        return x.copy()
    return O.eval_transfer(1 if tf == TF_HLG else 2, x.reshape(-1)).reshape(x.shape)


def headroom(tf, gamma_max, peak_nits=0.0):
    """step 4 in float32, as written: given when peak_nits > 0, else measured from m' = gamma_max"""
    k = k_of(tf)
    cap = k
    if peak_nits > 0:
        return np.minimum(np.maximum(F(peak_nits) / F(203.0), F(1.0)), cap)
    lin = inv_oetf(tf, np.array([gamma_max], F))[0]
    return np.minimum(np.maximum(lin * k, F(1.0)), cap)


# ------------------------------------------------------------------ frames: (luma (h, w) uint16, chroma (h / 2, w) uint16), P010 words

def lcg_planes(w, h, seed):
    p010, _ = O.lcg_frame(w, h, seed)
    return p010[:w * h].reshape(h, w).copy(), p010[w * h:].reshape(h // 2, w).copy()


def ramp_planes(w, h, grey=False, swing=120.0, top=876.0):
    """a smooth ramp over the legal code range (up to `top` codes above black): luma rises along the diagonal (along x alone when grey), chroma drifts slowly around
    the neutral code by `swing` codes end to end -- not at all when grey"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    t = x / max(w - 1, 1) if grey else (x + y) / max(w + h - 2, 1)
    luma = (64 + np.round(t * top)).astype(np.uint16) << 6
    cx, cy = np.meshgrid(np.arange(w // 2), np.arange(h // 2))
    u = 512 + (0 if grey else 1) * np.round(swing * (cx / max(w // 2 - 1, 1) - 0.5))
    v = 512 + (0 if grey else 1) * np.round(swing * (cy / max(h // 2 - 1, 1) - 0.5))
    chroma = np.empty((h // 2, w), np.uint16)
    chroma[:, 0::2] = u.astype(np.uint16) << 6
    chroma[:, 1::2] = v.astype(np.uint16) << 6
    return luma.astype(np.uint16), chroma


def tiled_lcg_planes(w, h, tw, th, seed):
    """LCG noise of tw x th repeated over w x h: a large frame with few distinct code triples"""
    l, c = lcg_planes(tw, th, seed)
    luma = np.tile(l, ((h + th - 1) // th, (w + tw - 1) // tw))[:h, :w]
    chroma = np.tile(c, ((h // 2 + th // 2 - 1) // (th // 2), (w + tw - 1) // tw))[:h // 2, :w]
    return np.ascontiguousarray(luma), np.ascontiguousarray(chroma)


def set_pixel(luma, chroma, x, y, ycode, ucode=512, vcode=512):
    luma[y, x] = ycode << 6
    chroma[y // 2, (x & ~1)] = ucode << 6
    chroma[y // 2, (x & ~1) + 1] = vcode << 6


# ------------------------------------------------------------------ the model

def _color_array(fn, gamut, a):
    """fn(gamut, Color) of the oracle over the rows of a float32 (n, 3) array"""
    out = np.empty_like(a)
    for i in range(a.shape[0]):
        r = fn(gamut, O.Color(a[i, 0], a[i, 1], a[i, 2]))
        out[i] = (r.r, r.g, r.b)
    return out


def _p010_yuv(codes):
    """getP010Pixel of the oracle for (n, 3) 10-bit code triples: a P010 image two pixels wide with one triple per 2x2 block"""
    n = codes.shape[0]
    luma = np.zeros((2 * n, 2), np.uint16)
    luma[0::2, 0] = codes[:, 0] << 6
    chroma = np.zeros((n, 2), np.uint16)
    chroma[:, 0] = codes[:, 1] << 6
    chroma[:, 1] = codes[:, 2] << 6
    img = O.p010_image(luma, 2, 2 * n, CG_709, 2, 2, chroma=chroma)
    fn = O.load().orc_getP010Pixel
    out = np.empty((n, 3), F)
    for i in range(n):
        r = fn(C.byref(img), 0, 2 * i)
        out[i] = (r.r, r.g, r.b)
    return out


def srgb_oetf(o):
    o = np.asarray(o, np.float64)
    return np.where(o <= 0.0031308, 12.92 * o, 1.055 * np.power(np.maximum(o, 1e-300), 1.0 / 2.4) - 0.055)


def model(luma, chroma, gamut, tf, peak_nits=0.0, identity=False):
    """-> dict: Y (h, w), U, V (h / 2, w / 2) uint8; vy, vu, vv: the values of step 8 before truncation (float64);
    H, m (float32): the headroom and the gamma-domain maximum; o (h, w, 3): step 5's output.
    identity: step 5 skipped (s = 1), for the property tests."""
    lib = O.load()
    h, w = luma.shape
    y10 = (luma >> 6).astype(np.uint32)
    u10 = np.repeat(np.repeat((chroma[:, 0::2] >> 6).astype(np.uint32), 2, axis=0), 2, axis=1)
    v10 = np.repeat(np.repeat((chroma[:, 1::2] >> 6).astype(np.uint32), 2, axis=0), 2, axis=1)
    key = y10 | (u10 << 10) | (v10 << 20)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    inv = inv.reshape(h, w)
    codes = np.stack([uniq & 1023, (uniq >> 10) & 1023, (uniq >> 20) & 1023], axis=1).astype(np.uint16)
    # steps 1, 2
    rgbp = np.clip(_color_array(lib.orc_yuvToRgb, gamut, _p010_yuv(codes)), F(0.0), F(1.0)).astype(F)
    lin = inv_oetf(tf, rgbp)
    # steps 3, 4
    k = k_of(tf)
    m = F(rgbp.max())
    H = headroom(tf, m, peak_nits)
    # steps 5, 6
    v = lin.astype(np.float64) * float(k)
    M = v.max(axis=1, keepdims=True)
    Hd = float(H)
    s = np.where(M > 0, (1.0 + M / (Hd * Hd)) / (1.0 + M), 1.0)
    if identity:
        s = np.ones_like(s)
    o = np.clip(v * s, 0.0, 1.0)
    e = srgb_oetf(o)
    # step 7
    yuv = _color_array(lib.orc_rgbToYuv, gamut, e.astype(F)).astype(np.float64)
    # step 8
    py, pu, pv = yuv[:, 0][inv], yuv[:, 1][inv], yuv[:, 2][inv]
    vy = py * 255.0 + 0.5
    blk = lambda a: (((a[0::2, 0::2] + a[0::2, 1::2]) + a[1::2, 0::2]) + a[1::2, 1::2]) * 0.25
    vu, vv = blk(pu) * 255.0 + 128.0 + 0.5, blk(pv) * 255.0 + 128.0 + 0.5
    q = lambda a: np.clip(a, 0.0, 255.0).astype(np.uint8)
    return {"Y": q(vy), "U": q(vu), "V": q(vv), "vy": vy, "vu": vu, "vv": vv, "H": F(H), "m": m, "o": o[inv]}


def in_doubt(v):
    """samples whose pre-truncation value lies within DOUBT of an integer (values the clip flattens are not: they are 0 or 255 on
    either side)"""
    v = np.asarray(v)
    return (np.abs(v - np.round(v)) < DOUBT) & (v > -DOUBT) & (v < 255.0 + DOUBT)


def compare(got, want_plane, want_v):
    """-> (samples that differ, samples in doubt, worst difference, differing samples that are NOT in doubt)"""
    d = np.abs(got.astype(np.int32) - want_plane.astype(np.int32))
    doubt = in_doubt(want_v)
    return int((d != 0).sum()), int(doubt.sum()), int(d.max()) if d.size else 0, int(((d != 0) & ~doubt).sum())


# ------------------------------------------------------------------ the inputs of the GPU tests

class Case:
    def __init__(self, name, w, h, tf, gamut, content, luma_stride=None, chroma_stride=None, dst_luma_stride=None, dst_chroma_stride=None,
                 offset=0):
        self.name, self.w, self.h, self.tf, self.gamut, self.content = name, w, h, tf, gamut, content
        self.luma_stride, self.chroma_stride = luma_stride or w, chroma_stride or w
        self.dst_luma_stride, self.dst_chroma_stride = dst_luma_stride or w, dst_chroma_stride or w // 2
        self.offset = offset   # bytes: the separate chroma pointers sit this far off their natural alignment

    def __repr__(self):
        return self.name


_TF = {TF_HLG: "hlg", TF_PQ: "pq", TF_LINEAR: "lin"}
_CG = {CG_709: "709", CG_P3: "p3", CG_2100: "2100"}


def peak_xy(w, h):
    """where the large frame's brightest pixel sits: the last block row, off the last column"""
    return w - 3, h - 2


@functools.lru_cache(maxsize=None)
def planes(content, w, h):
    # (8 x 8: a chroma plane has 16 samples, one in doubt would be 6 % of it -- seed and swing are chosen so that there is none)
    if content == "lcg":
        return lcg_planes(w, h, 142 if w == 8 else 7 + w)
    if content == "ramp":
        return ramp_planes(w, h, swing=SWING8 if w == 8 else 120.0, top=700.0)   # signal up to 0.8: a headroom inside the rule's clamps
    # the large frame: DIM noise -- the LCG tile's luma halved towards black, its chroma pulled to 15 % of its distance from neutral,
    # so that no channel comes near the clamp -- repeated over the frame, and ONE brighter, neutral pixel in block row (h - 2) / 2:
    # 539 of 540 at 1920 x 1080, which the measuring pass (at most 512 workgroup rows) reaches only by striding.  That pixel alone
    # decides m' and H; "lcg_tiled_flat" is the same frame without it.
    if content in ("lcg_tiled", "lcg_tiled_flat"):
        luma, chroma = tiled_lcg_planes(w, h, 128, 72, 5)
        luma = ((64 + ((luma >> 6).astype(np.int64) - 64) // 2).astype(np.uint16) << 6).astype(np.uint16)
        chroma = ((512 + np.round(((chroma >> 6).astype(np.int64) - 512) * 0.15)).astype(np.uint16) << 6).astype(np.uint16)
        if content == "lcg_tiled":
            set_pixel(luma, chroma, *peak_xy(w, h), 850)
        return luma, chroma
    raise KeyError(content)


def cases():
    """sizes and layouts of the issue: all three gamuts at the small sizes, one each (rotating) at 258 x 130 and 1920 x 1080"""
    out = []
    for tf in (TF_HLG, TF_PQ, TF_LINEAR):
        for content in ("lcg", "ramp"):
            for gamut in (CG_709, CG_P3, CG_2100):
                tag = "%s-%s-%s" % (_TF[tf], _CG[gamut], content)
                out.append(Case("8x8-" + tag, 8, 8, tf, gamut, content))
                out.append(Case("66x34-" + tag, 66, 34, tf, gamut, content, luma_stride=80, chroma_stride=70, dst_luma_stride=80, dst_chroma_stride=37))
                out.append(Case("64x64-" + tag, 64, 64, tf, gamut, content))
            gamut = (CG_2100, CG_709, CG_P3)[tf]
            tag = "%s-%s-%s" % (_TF[tf], _CG[gamut], content)
            out.append(Case("258x130-" + tag, 258, 130, tf, gamut, content, luma_stride=258, chroma_stride=260, dst_luma_stride=264, dst_chroma_stride=131,
                            offset=2))
        gamut = (CG_709, CG_P3, CG_2100)[tf]
        out.append(Case("1920x1080-%s-%s-lcg_tiled" % (_TF[tf], _CG[gamut]), 1920, 1080, tf, gamut, "lcg_tiled"))
    return out


@functools.lru_cache(maxsize=None)
def _expected(content, w, h, gamut, tf, peak_nits):
    luma, chroma = planes(content, w, h)
    return model(luma, chroma, gamut, tf, peak_nits)


def expected(case, peak_nits=0.0):
    """the model's answer for a case: computed once per (content, size, gamut, tf, peak), shared and left unchanged"""
    return _expected(case.content, case.w, case.h, case.gamut, case.tf, float(peak_nits))
