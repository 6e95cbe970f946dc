"""applyGainMap at map scale factors other than 4: the cases, their images and the oracle's bytes, not a
test file.

A case is (name, width, height, map width, map height, chroma format).  The 4:2:0 images are LCG frames (oracle.lcg_frame); the maps
are seeded random bytes with 0 and 255 present.  The expected bytes are the oracle's applyGainMap, computed once per
(case, output format, display boost, boost range, lut) and left read-only.

4:4:4, 4:2:2 and 4:4:0 images have no oracle path of their own.  As tests/test_gpu_jpeg_sampling.py does, such an image is split
into 4:2:0 images that hold one chroma phase each: pixel (x, y) reads the chroma sample (x >> csx, y >> csy), which the 4:2:0 image
of phase (x & 1, y & 1) -- its chroma planes are the samples [dy::2, dx::2] in a direction that is not subsampled -- holds at
(x >> 1, y >> 1).  Output pixel (x, y) is taken from the run on its phase image.  An image of odd height needs one run more per
phase: the oracle places Cr chroma_stride * (height / 2) behind Cb, where row height / 2 of Cb -- which only the last row of
pixels reads -- would lie.  A second buffer holds that row of Cb and of Cr where the last row of pixels looks for them, and the last
row of pixels is taken from the run on it.
"""
import functools

import numpy as np

from oracle import oracle as O

F = np.float32
FLT_MAX = 3.4028234663852886e38
FORMATS = (1, 2, 3, 4)                      # F16, PQ 1010102, HLG 1010102, planar 10-bit
BPP = {1: 8, 2: 4, 3: 4, 4: 6}
MAX_BOOST = float(F(1000.0) / F(203.0))
RANGE = (1.0, MAX_BOOST)                    # (minContentBoost, maxContentBoost) of every test but the one below
RANGE_WIDE = (0.5, 6.0)                     # log2 min < 0: the (1 - gain) term of applyGain
CAPPED = 2.0                                # a display boost below maxContentBoost: values pass 1.0, the 0x3ff mask wraps
CHROMA_SHIFTS = {"420": (1, 1), "444": (0, 0), "422": (1, 0), "440": (0, 1)}

CASES = [
    # the division branch of the tap arithmetic: factors that are no power of two, with interior pixels and all three edge tables
    ("s3_300x12", 300, 12, 100, 4, "420"),       # two blocks of 256 columns
    ("s7_70x42", 70, 42, 10, 6, "420"),          # odd: a cell's columns straddle chroma samples
    ("s6_60x36", 60, 36, 10, 6, "420"),
    # every pixel on a tap; the smallest shift
    ("s1_34x18", 34, 18, 34, 18, "420"),
    ("s2_48x20", 48, 20, 24, 10, "420"),
    # powers of two up to the largest table the library keeps
    ("s16_96x48", 96, 48, 6, 3, "420"),
    ("s32_128x64", 128, 64, 4, 2, "420"),
    ("s64_256x128", 256, 128, 4, 2, "420"),
    ("s128_384x256", 384, 256, 3, 2, "420"),
    # tables that live for the call: the first factor past the cache (division branch) and a 4 MiB table (shift branch)
    ("s129_258x258", 258, 258, 2, 2, "420"),
    ("s256_512x256", 512, 256, 2, 1, "420"),
    # maps one pixel wide, one pixel high, one pixel: the no-right, no-bottom and corner tables for every pixel
    ("onewide_2x40", 2, 40, 1, 20, "420"),
    ("onehigh_48x2", 48, 2, 24, 1, "420"),
    ("onepixel_2x2", 2, 2, 1, 1, "420"),
    ("onepixel_130x130", 130, 130, 1, 1, "420"),
    # more than two blocks of 256 columns with a ragged tail of 8, not factor 4
    ("s2_520x6", 520, 6, 260, 3, "420"),
    # the other chroma formats off factor 4, odd sizes among them
    ("s5_45x35_444", 45, 35, 9, 7, "444"),
    ("s3_30x21_422", 30, 21, 10, 7, "422"),
    ("s3_30x21_444", 30, 21, 10, 7, "444"),
    ("s2_20x18_440", 20, 18, 10, 9, "440"),
]
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
# what a case is in the list for (tests/test_apply_scales_cpu.py holds the list to it)
GENERAL = ["s3_300x12", "s7_70x42", "s6_60x36", "s2_48x20", "s16_96x48"]
ONLY_TABLES = {"onewide_2x40": {1, 3}, "onehigh_48x2": {2, 3}, "onepixel_2x2": {3}, "onepixel_130x130": {3}}
# test_capped_display_boost_off_factor_4's subset: factors 3, 16, 129 and the 1x1 map
CAPPED_NAMES = ["s3_300x12", "s16_96x48", "s129_258x258", "onepixel_130x130"]
WIDE_NAME = "s7_70x42"


def factor(case):
    return case[1] // case[3]


def is_420(case):
    return case[5] == "420"


def chroma_shape(case):
    """(rows, columns) of a chroma plane: the reference's halves for 4:2:0, libjpeg's rounded-up sizes otherwise"""
    _, w, h, _, _, chroma = case
    if chroma == "420":
        return h // 2, w // 2
    csx, csy = CHROMA_SHIFTS[chroma]
    return (h + csy) >> csy, (w + csx) >> csx


@functools.lru_cache(maxsize=None)
def planes(name):
    """(Y (h, w), Cb, Cr) uint8, read-only.  4:2:0: an LCG frame; otherwise seeded luma and chroma that differs at every sample"""
    case = BY_NAME[name]
    _, w, h, _, _, chroma = case
    seed = 7000 + NAMES.index(name)
    ch, cw = chroma_shape(case)
    if chroma == "420":
        _, yuv = O.lcg_frame(w, h, seed)
        y = yuv[:w * h].reshape(h, w).copy()
        cb = yuv[w * h:w * h + cw * ch].reshape(ch, cw).copy()
        cr = yuv[w * h + cw * ch:].reshape(ch, cw).copy()
    else:
        y = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)
        cb = ((np.arange(ch)[:, None] * 7 + np.arange(cw)[None, :] * 3) % 251).astype(np.uint8)
        cr = ((np.arange(ch)[:, None] * 5 + np.arange(cw)[None, :] * 11 + 17) % 241).astype(np.uint8)
    for a in (y, cb, cr):
        a.setflags(write=False)
    return y, cb, cr


def packed(name):
    """the planes as one buffer: Y, then Cb, then Cr -- what the yuv420 / ycbcr descriptors of libultrahdr_dev_amd.api describe"""
    return np.concatenate([p.reshape(-1) for p in planes(name)])


@functools.lru_cache(maxsize=None)
def gain_map(name):
    """(map height, map width) uint8, seeded, with 0 and 255 present wherever the map has two pixels"""
    _, _, _, mw, mh, _ = BY_NAME[name]
    m = np.random.RandomState(9000 + NAMES.index(name)).randint(0, 256, (mh, mw)).astype(np.uint8)
    if m.size >= 2:
        m.reshape(-1)[0], m.reshape(-1)[-1] = 0, 255
    m.setflags(write=False)
    return m


def oracle_metadata(boost_range):
    lo, hi = boost_range
    return O.Metadata(float(F(hi)), float(F(lo)), 1.0, 0.0, 0.0, float(F(lo)), float(F(hi)), 1)


def api_metadata(api, boost_range):
    return api.metadata(F(boost_range[1]), F(boost_range[0]))


def _phases(case):
    csx, csy = CHROMA_SHIFTS[case[5]]
    return [(dx, dy) for dy in range(1 if csy else 2) for dx in range(1 if csx else 2)]


def _phase_chroma(case, plane, dx, dy):
    """the samples of `plane` that the pixels of phase (dx, dy) read, where a 4:2:0 image holds them"""
    csx, csy = CHROMA_SHIFTS[case[5]]
    return plane[(slice(None) if csy else slice(dy, None, 2)), (slice(None) if csx else slice(dx, None, 2))]


def _runs(case, prefix, fmt, boost, boost_range, lut):
    """{phase: output bytes of applyGainMap on that phase's 4:2:0 image}; prefix: "orc_" or "ref_" """
    name, w, h, _, _, _ = case
    y, cb, cr = planes(name)
    luma = np.ascontiguousarray(y)
    gmap = np.ascontiguousarray(gain_map(name))
    md = oracle_metadata(boost_range)
    nbytes = BPP[fmt] * w * h
    half, cs = h // 2, (w + 1) // 2
    threads = 2 if prefix == "orc_" else 1
    out = {}
    for dx, dy in _phases(case):
        u, v = _phase_chroma(case, cb, dx, dy), _phase_chroma(case, cr, dx, dy)
        buf = np.zeros((2 * half + 2, cs), np.uint8)
        rows, cols = min(half, u.shape[0]), u.shape[1]
        buf[:rows, :cols] = u[:rows]
        buf[half:half + rows, :cols] = v[:rows]
        st, run, dest = O.apply(prefix, O.yuv420_image(luma, w, h, O.CG_BT709, w, cs, buf), gmap, md, fmt, boost, threads=threads, lut=lut)
        assert st == 0 and (dest.width, dest.height) == (w, h), (name, st)
        run = run[:nbytes].copy()
        if h % 2 and u.shape[0] > half:   # the last row of pixels: row `half` of Cb and of Cr where the oracle reads them
            buf[:] = 0
            buf[half, :cols] = u[half]
            buf[2 * half, :cols] = v[half]
            st, last, _ = O.apply(prefix, O.yuv420_image(luma, w, h, O.CG_BT709, w, cs, buf), gmap, md, fmt, boost, threads=threads, lut=lut)
            assert st == 0
            _rows(run, fmt, w, h)[..., h - 1, :] = _rows(last[:nbytes], fmt, w, h)[..., h - 1, :]
        out[(dx, dy)] = run
    return out


def _rows(raw, fmt, w, h):
    """a view of output bytes with the image's rows and columns as the last two axes"""
    if fmt == 4:
        return raw.view(np.uint16).reshape(3, h, w)
    return raw.view(np.uint64 if fmt == 1 else np.uint32).reshape(h, w)


def apply_of(name, prefix, fmt, boost, boost_range=RANGE, lut=False):
    """applyGainMap of the case through `prefix`'s code: the output bytes, pixel (x, y) from the run on its phase image"""
    case = BY_NAME[name]
    _, w, h, _, _, chroma = case
    runs = _runs(case, prefix, fmt, boost, boost_range, lut)
    if len(runs) == 1:
        return runs[(0, 0)]
    csx, csy = CHROMA_SHIFTS[chroma]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    px = np.zeros_like(xs) if csx else xs & 1
    py = np.zeros_like(ys) if csy else ys & 1
    want = np.zeros(BPP[fmt] * w * h, np.uint8)
    dst = _rows(want, fmt, w, h)
    for (dx, dy), run in runs.items():
        sel = (px == dx) & (py == dy)
        dst[..., sel] = _rows(run, fmt, w, h)[..., sel]
    return want


@functools.lru_cache(maxsize=None)
def expected(name, fmt, boost=FLT_MAX, boost_range=RANGE, lut=False):
    """the oracle's bytes, computed once and read-only; lut: its LUT pipeline (what UHDR_HIP_APPLY_LUT reproduces)"""
    want = apply_of(name, "orc_", fmt, boost, boost_range, lut)
    want.setflags(write=False)
    return want


# ------------------------------------------------------------------ sampleMap's tap choice

def tap_routes(case):
    """gainmapmath.cpp:686-720 for every pixel of the case, in numpy: (table (h, w) -- 0 all four taps, 1 no right tap, 2 no bottom
    tap, 3 the corner --, offset_x (w,), offset_y (h,))"""
    _, w, h, mw, mh, _ = case
    s = factor(case)
    x, y = np.arange(w), np.arange(h)
    xl, yl = x // s, y // s
    xu, yu = xl + 1, yl + 1
    xl, xu = np.minimum(xl, mw - 1), np.minimum(xu, mw - 1)
    yl, yu = np.minimum(yl, mh - 1), np.minimum(yu, mh - 1)
    same_x, same_y = (xl == xu)[None, :], (yl == yu)[:, None]
    table = np.where(same_x & same_y, 3, np.where(same_x, 1, np.where(same_y, 2, 0)))
    return table, x % s, y % s
