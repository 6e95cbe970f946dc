"""The tone-mapped SDR image of a packed HDR image (include/uhdr_hip.h, "tone-mapped SDR image from a packed HDR image"; DESIGN.md
section 4.1.7) as a model, and the cases of its tests: not a test file.  There is no reference code for this entry: the header's steps
are the contract.

Step 1 is tests/packed_cases.py::pixel_values plus the clamp; step 2 goes through the oracle's eval_transfer, once per distinct
value (an RGBA1010102 channel has 1024 of them: table()); H is formed in float32 as tests/tonemap_cases.py::headroom forms it; the
steps behind it are numpy float64.  The doubt rule is tonemap_cases.DOUBT: a sample whose value before truncation lies within 1/256
of an integer may differ by one code, every other sample equals the model -- argued there for a longer f32 chain (matrix, chroma
average) of which this one is a prefix.
"""
import functools

import numpy as np

from tests import packed_cases as P
from tests import tonemap_cases as T

F = np.float32
TF_LINEAR, TF_HLG, TF_PQ = P.TF_LINEAR, P.TF_HLG, P.TF_PQ
FMT_1010102, FMT_F16 = P.FMT_1010102, P.FMT_F16
FORMS = P.FORMS
FORM_IDS = ["pq1010102", "hlg1010102", "f16"]
REINHARD, SHIFT = T.REINHARD, T.SHIFT
DOUBT = T.DOUBT
PEAK_GROUPS = 128   # kTonePackedPeakGroups: the measuring pass spends at most this many workgroup rows, of 4 image rows each, per image


# ------------------------------------------------------------------ the model

def values(img, fmt):
    """step 1: (h, w, 3) float32 in [0, 1]"""
    v = P.pixel_values(img, fmt)
    return np.minimum(np.maximum(v, F(0.0)), F(1.0)).astype(F)   # (what fminf(fmaxf(x, 0), 1) gives; NaN is not among the cases)


@functools.lru_cache(maxsize=None)
def table(tf):
    """the 1024 values of step 2 for RGBA1010102: the oracle's inverse OETF of (float)c * (1 / 1023.0f)"""
    t = T.inv_oetf(tf, (np.arange(1024).astype(F) * (F(1) / F(1023))).astype(F))
    t.setflags(write=False)
    return t


def linear(img, fmt, tf):
    """steps 1 and 2: (values, lin), both (h, w, 3) float32"""
    v = values(img, fmt)
    if fmt == FMT_F16:
        return v, v.copy()
    codes = np.stack([img & 1023, (img >> 10) & 1023, (img >> 20) & 1023], axis=2)
    return v, table(tf)[codes]


def model(img, fmt, tf, peak_nits=0.0, identity=False):
    """-> dict: rgba (h, w, 4) uint8; v (h, w, 3) float64, the values of step 7 before truncation; H, m (float32).
    identity: step 5 skipped (s = 1), for the property tests"""
    val, lin = linear(img, fmt, tf)
    k = T.k_of(tf)
    m = F(val.max())
    H = T.headroom(tf, m, peak_nits)
    v = lin.astype(np.float64) * float(k)
    M = v.max(axis=2, keepdims=True)
    Hd = float(H)
    s = np.where(M > 0, (1.0 + M / (Hd * Hd)) / (1.0 + M), 1.0)
    if identity:
        s = np.ones_like(s)
    e = T.srgb_oetf(np.clip(v * s, 0.0, 1.0))
    pre = e * 255.0 + 0.5
    rgba = np.full(img.shape[:2] + (4,), 0xFF, np.uint8)
    rgba[:, :, :3] = np.clip(pre, 0.0, 255.0).astype(np.uint8)
    return {"rgba": rgba, "v": pre, "H": F(H), "m": m}


def compare(got_rgba, want):
    """-> (samples that differ, samples in doubt, worst difference, differing samples that are NOT in doubt) over R, G, B"""
    return T.compare(got_rgba[:, :, :3], want["rgba"][:, :, :3], want["v"])


def doubt_share(want):
    return float(T.in_doubt(want["v"]).mean())


# ------------------------------------------------------------------ contents

def lcg_f16_signed(w, h, seed):
    """packed_cases.lcg_rgba_f16 with a sign bit mixed into one draw in eight, and the values the issue names: 0, a subnormal, -0, a
    negative value, 1.0, 3.0 and 4.0"""
    v = P.lcg_rgba_f16(w, h, seed).copy()
    neg = (P._lcg(w * h * 4, seed ^ 0x5A5A) & 7).reshape(h, w, 4) == 0
    v[neg] |= 0x8000
    v[0, 0, 0], v[0, 1, 1], v[0, 2, 0], v[0, 3, 1], v[1, 0, 2], v[1, 1, 0], v[-1, -1, 2] = 0, 0x0155, 0x8000, 0xBC00, 0x3C00, 0x4400, 0x4200
    return v


def ramp(fmt, w, h):
    """a smooth ramp up to 0.8 of the signal range: R along x, G along y, B along the diagonal; alpha arbitrary"""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    t = np.stack([x / max(w - 1, 1), y / max(h - 1, 1), (x + y) / max(w + h - 2, 1)], axis=2) * 0.8
    if fmt == FMT_F16:
        out = np.zeros((h, w, 4), np.uint16)
        out[:, :, :3] = t.astype(np.float16).view(np.uint16)
        out[:, :, 3] = 0x3C00
        return out
    c = np.round(t * 1023).astype(np.uint32)
    return (c[:, :, 0] | (c[:, :, 1] << 10) | (c[:, :, 2] << 20) | ((x.astype(np.uint32) & 3) << 30)).astype(np.uint32)


def peak_xy(w, h):
    """where the large frame's brightest pixel sits: the last but one row, off the last column"""
    return w - 3, h - 2


def tiled(fmt, w, h, bright):
    """the large frame: DIM noise of 128 x 72 -- codes up to 255 of 1023, halves up to 0.1 -- repeated over the frame, whose
    headroom is 1 by itself, and (bright) ONE brighter pixel in row h - 2.  That pixel alone decides m' and H, and the measuring pass
    reaches its row only by striding: a trip of its grid covers 4 * PEAK_GROUPS = 512 rows"""
    if fmt == FMT_F16:
        tile = (P._lcg(128 * 72 * 4, 77) % 0x2E67).astype(np.uint16).reshape(72, 128, 4)
        img = np.ascontiguousarray(np.tile(tile, ((h + 71) // 72, (w + 127) // 128, 1))[:h, :w])
        if bright:
            x, y = peak_xy(w, h)
            img[y, x, 1] = 0x3800   # 0.5
        return img
    v = P._lcg(128 * 72 * 4, 78).reshape(72, 128, 4)
    c = (v[:, :, :3] % 256).astype(np.uint32)
    tile = (c[:, :, 0] | (c[:, :, 1] << 10) | (c[:, :, 2] << 20) | ((v[:, :, 3] & 3).astype(np.uint32) << 30)).astype(np.uint32)
    img = np.ascontiguousarray(np.tile(tile, ((h + 71) // 72, (w + 127) // 128))[:h, :w])
    if bright:
        x, y = peak_xy(w, h)
        img[y, x] = (img[y, x] & ~np.uint32(1023 << 10)) | np.uint32(900 << 10)
    return img


def seed_of(w, fmt, tf):
    """seeds of the LCG cases: the 2 % condition of tests/test_packed_tonemap_cpu.py holds for them"""
    return 7000 + 16 * w + 4 * (fmt - FMT_1010102) + tf


@functools.lru_cache(maxsize=None)
def image(content, fmt, tf, w, h):
    if content == "lcg":
        img = lcg_f16_signed(w, h, seed_of(w, fmt, tf)) if fmt == FMT_F16 else P.lcg_rgba1010102(w, h, seed_of(w, fmt, tf))
    elif content == "ramp":
        img = ramp(fmt, w, h)
    elif content in ("tiled", "tiled_flat"):
        img = tiled(fmt, w, h, content == "tiled")
    else:
        raise KeyError(content)
    img.setflags(write=False)
    return img


class Case:
    """src_stride / dst_stride in pixels; offset: bytes between a 256-byte boundary and either data pointer; aligned: the layout
    meets what the ALIGNED kernel instance asks (16-byte row starts on both sides, width % 4 == 0)"""

    def __init__(self, name, fmt, tf, w, h, content, src_stride=None, dst_stride=None, offset=0):
        self.name, self.fmt, self.tf, self.w, self.h, self.content = name, fmt, tf, w, h, content
        self.src_stride, self.dst_stride, self.offset = src_stride or w, dst_stride or w, offset
        pieces = 2 if fmt == FMT_F16 else 4
        self.aligned = w % 4 == 0 and offset % 16 == 0 and self.src_stride % pieces == 0 and self.dst_stride % 4 == 0

    def __repr__(self):
        return self.name


def cases():
    """the smallest shapes at which each route can go wrong, per form:
      8x8        one partly filled wave
      64x64      ALIGNED: 16 pieces of 4 pixels per row, 16 groups of 4 rows
      66x34      strides 80 behind data 4 bytes (F16: 8) off: a ragged width, no row 16-byte aligned, a last group of 2 rows:
                 element by element
      258x130    data 4 bytes (F16: 8) past a 256-byte boundary, odd strides: element by element, 5 blocks across
      264x10     ALIGNED past one block across: 66 pieces per row, the second block holds 2; a last group of 2 rows.  (The ALIGNED
                 instance has no partial piece: it is chosen only for widths of whole pieces.)
      1920x1080  the large frame (tiled())"""
    out = []
    for (fmt, tf), tag in zip(FORMS, FORM_IDS):
        off = 8 if fmt == FMT_F16 else 4
        out.append(Case("8x8-%s-lcg" % tag, fmt, tf, 8, 8, "lcg"))
        out.append(Case("64x64-%s-lcg" % tag, fmt, tf, 64, 64, "lcg"))
        out.append(Case("66x34-%s-lcg" % tag, fmt, tf, 66, 34, "lcg", 80, 80, off))
        out.append(Case("258x130-%s-lcg" % tag, fmt, tf, 258, 130, "lcg", 261, 259, off))
        out.append(Case("264x10-%s-ramp" % tag, fmt, tf, 264, 10, "ramp", 272, 268))
        out.append(Case("1920x1080-%s-tiled" % tag, fmt, tf, 1920, 1080, "tiled"))
    return out


@functools.lru_cache(maxsize=None)
def _expected(content, fmt, tf, w, h, peak_nits):
    out = model(image(content, fmt, tf, w, h), fmt, tf, peak_nits)
    for a in (out["rgba"], out["v"]):
        a.setflags(write=False)
    return out


def expected(case, peak_nits=0.0):
    """the model's answer for a case: computed once per (content, form, size, peak), shared and left unchanged"""
    return _expected(case.content, case.fmt, case.tf, case.w, case.h, float(peak_nits))
