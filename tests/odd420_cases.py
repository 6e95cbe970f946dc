"""Odd-sized 4:2:0 images in front of applyGainMap and of the JPEG/R decode (DESIGN.md sections 4.2.4 and 7.3.1): the cases, their
buffers and the oracle's bytes, not a test file.

For such an image the reference's addressing is no longer tidy.  getYuv420Pixel reads chroma sample (y >> 1) * chroma_stride +
(x >> 1), Cb from chroma_data and Cr chroma_stride * (height / 2) behind it.  With an odd width the last column's index is w / 2, one
past its row: the first sample of the next row.  With an odd height the last row of pixels reads row h / 2 of Cb, which lies in Cr, and
row h / 2 of Cr, which lies behind it.  What comes out depends on every byte of the buffer, so a case is a BUFFER, in one of three
layouts:
  "ref"     the reference decoder's (jpegdecoderhelper.cpp:291, :360-362): Y, Cb at w h, Cr at w h + w h / 4, every other byte of
            floor(3 w h / 2) zero -- a gap of w h / 4 - (w / 2)(h / 2) bytes lies between Cb's end and Cr's start, and Cr is read shifted;
  "tight"   what a caller makes with api.yuv420_image: Cr directly behind Cb, zeros up to floor(3 w h / 2);
  "strided" luma_stride above w and chroma_stride above w / 2, noise in the row padding too, as long as the reference reads.
Content is seeded noise in all three planes: a shifted or clamped chroma index changes bytes.  Maps are seeded bytes with 0 and 255
present.  The expected bytes are the oracle's applyGainMap over that very buffer, computed once and left read-only.

The file cases are JPEG/R files with odd-sized 4:2:0 primaries (Pillow's, subsampling=2), maps of the primary's size.
Sizes with w < 2 or h < 2 are out of scope: there the reference itself reads outside its buffer.
"""
import collections
import functools

import numpy as np

from oracle import oracle as O
from tests import apply_scale_cases as A

F = np.float32
FLT_MAX = A.FLT_MAX
FORMATS = A.FORMATS
BPP = A.BPP
RANGE = A.RANGE
CAPPED = A.CAPPED

Case = collections.namedtuple("Case", "name w h mw mh layout reads_need")
# (w, h, map w, map h), the layout, and the fact of the reference layout that tests/test_odd420_cpu.py holds the list to: whether
# applyGainMap reads the byte at need = w h + 2 (w h / 4), one past what a decode call returns (w = 2 mod 4 with an odd h)
CASES = [
    Case("f1_17x9", 17, 9, 17, 9, "ref", False),
    Case("f5_45x35", 45, 35, 9, 7, "tight", False),
    Case("f3_63x45", 63, 45, 21, 15, "strided", False),
    Case("f7_49x35", 49, 35, 7, 5, "ref", False),
    Case("f7_259x301", 259, 301, 37, 43, "tight", False),     # two column blocks of 256, the second one three pixels wide
    Case("f1_17x8", 17, 8, 17, 8, "tight", False),             # odd width alone
    Case("f1_16x9", 16, 9, 16, 9, "ref", False),               # odd height alone
    Case("f3_3x3", 3, 3, 1, 1, "ref", False),                  # a 1 x 1 map, one chroma sample
    Case("f1_18x9", 18, 9, 18, 9, "ref", True),
    Case("f1_518x3", 518, 3, 518, 3, "tight", True),           # three column blocks of 256
    Case("f1_2x3", 2, 3, 2, 3, "ref", True),                   # no gap: w h / 4 = (w / 2)(h / 2) = 1
]
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
CAPPED_NAMES = ["f7_259x301", "f1_518x3"]
RGB_NAMES = ["f1_17x9", "f3_63x45", "f7_259x301"]
MD_NAMES = ["f5_45x35", "f3_63x45"]
MD_CASE = "black"      # tests/gainmap_md_cases.CASES: gamma 0.5, an HDR offset, log2 min < 0, a capacity range that is not the content's
STRIDE_PAD = (5, 3)    # samples added to the luma and to the chroma rows of the "strided" case


def factor(case):
    return case.w // case.mw


def strides(case, layout=None):
    """(luma_stride, chroma_stride)"""
    if (layout or case.layout) == "strided":
        return case.w + STRIDE_PAD[0], case.w // 2 + STRIDE_PAD[1]
    return case.w, case.w // 2


def gap(case):
    """[first, last) of the bytes between Cb's end and Cr's start in the reference's layout"""
    return case.w * case.h + (case.w // 2) * (case.h // 2), case.w * case.h + case.w * case.h // 4


def need(case):
    """what uhdr_hip_jpeg_decode returns for the image"""
    return case.w * case.h + 2 * (case.w * case.h // 4)


def read_offsets(case, layout=None):
    """(luma, Cb, Cr): the byte offsets getYuv420Pixel reads for every pixel, (h, w) each"""
    ls, cs = strides(case, layout)
    y, x = np.mgrid[0:case.h, 0:case.w]
    cb = ls * case.h + (y >> 1) * cs + (x >> 1)
    return y * ls + x, cb, cb + cs * (case.h // 2)


def extent(case, layout=None):
    """bytes of the buffer: floor(3 w h / 2), the reference's, for the packed layouts; as far as the reference reads for the strided one"""
    if (layout or case.layout) == "strided":
        return int(max(o.max() for o in read_offsets(case, layout))) + 1
    return case.w * case.h * 3 // 2


@functools.lru_cache(maxsize=None)
def buffer(name, layout=None):
    """the case's image as one read-only buffer in `layout` (default: the case's own)"""
    case = BY_NAME[name]
    layout = layout or case.layout
    w, h, cw, ch = case.w, case.h, case.w // 2, case.h // 2
    rng = np.random.default_rng(4200 + NAMES.index(name))
    if layout == "strided":
        buf = rng.integers(0, 256, extent(case, layout)).astype(np.uint8)
    else:
        buf = np.zeros(extent(case, layout), np.uint8)
        buf[:w * h] = rng.integers(0, 256, w * h)
        cr = w * h + (w * h // 4 if layout == "ref" else cw * ch)
        buf[w * h:w * h + cw * ch] = rng.integers(0, 256, cw * ch)
        buf[cr:cr + cw * ch] = rng.integers(0, 256, cw * ch)
    buf.setflags(write=False)
    return buf


def image(case, buf, layout=None):
    """the oracle's descriptor over buf: chroma_data follows the luma"""
    ls, cs = strides(case, layout)
    return O.yuv420_image(buf, case.w, case.h, O.CG_BT709, ls, cs)


def seen_chroma(case, buf, layout=None):
    """(Y, U, V), (h, w) each: the samples every pixel reads, chroma at full resolution -- what a model with csx = csy = 0 takes"""
    yo, uo, vo = read_offsets(case, layout)
    return buf[yo], buf[uo], buf[vo]


@functools.lru_cache(maxsize=None)
def gain_map(name, planes=1):
    """(mh, mw) or (mh, mw, 3) uint8, seeded, with 0 and 255 present wherever a plane has two pixels"""
    case = BY_NAME[name]
    shape = (case.mh, case.mw) if planes == 1 else (case.mh, case.mw, planes)
    m = np.random.RandomState(9400 + 10 * NAMES.index(name) + planes).randint(0, 256, shape).astype(np.uint8)
    if case.mw * case.mh >= 2:
        m.reshape(case.mw * case.mh, -1)[0], m.reshape(case.mw * case.mh, -1)[-1] = 0, 255
    m.setflags(write=False)
    return m


def apply_of(case, buf, prefix, fmt, boost=FLT_MAX, lut=False, layout=None):
    """applyGainMap of `prefix`'s code ("orc_" / "ref_") over buf with the case's map"""
    gmap = np.ascontiguousarray(gain_map(case.name))
    st, out, dest = O.apply(prefix, image(case, buf, layout), gmap, A.oracle_metadata(RANGE), fmt, boost, threads=2 if prefix == "orc_" else 1, lut=lut)
    assert st == 0 and (dest.width, dest.height) == (case.w, case.h), (case.name, st)
    return out[:BPP[fmt] * case.w * case.h].copy()


@functools.lru_cache(maxsize=None)
def expected(name, fmt, boost=FLT_MAX, lut=False):
    """the oracle's bytes, computed once and read-only; lut: its LUT pipeline"""
    want = apply_of(BY_NAME[name], buffer(name), "orc_", fmt, boost, lut)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def expected_rgb(name, fmt, boost=FLT_MAX):
    """a three-component map: the oracle's applyGainMap per channel (tests/rgbmap_cases.composite_apply)"""
    from tests import rgbmap_cases as R
    case = BY_NAME[name]
    want = R.composite_apply(O, image(case, buffer(name)), gain_map(name, 3), A.oracle_metadata(RANGE), fmt, boost).copy()
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def md_inputs(name):
    """the per-pixel inputs (e, g) of tests/gainmap_md_cases' model, as tests/test_gpu_gainmap_md.py takes them: the linear SDR colour
    of the samples each pixel reads, and the sampled gain"""
    from tests import gainmap_md_cases as M
    case = BY_NAME[name]
    Y, U, V = seen_chroma(case, buffer(name))
    return M.linear_sdr(Y, U, V, 0, 0), M.sampled_gain_by_tables(gain_map(name), case.w, case.h)


# ------------------------------------------------------------------ files

File = collections.namedtuple("File", "name data primary gmap w h rgb")
FILE_NAMES = ["o17", "o45", "o18", "o17x8", "o16x9", "og17", "og45"]


@functools.lru_cache(maxsize=None)
def files():
    """{name: File}: 4:2:0 primaries of 17x9, 45x37, 18x9, 17x8 and 16x9 with a one-component map of the same size each, 17x9 and 45x37
    with the three-component golden maps too"""
    from oracle import jpegr_oracle as J
    from tests import rgbmap_cases as R
    from tests.jpeg_scaled_cases import JPEGR_MD, gray_jpeg, pillow_jpeg
    out = {}

    def made(name, w, h, seed, rgb=False):
        primary = pillow_jpeg(w, h, seed, subsampling=2)
        gmap = R.golden_jpeg(w, h, 85) if rgb else gray_jpeg(w, h, seed + 10, quality=85)
        data = J.append_gainmap(primary, gmap, JPEGR_MD)
        assert isinstance(data, bytes)
        out[name] = File(name, data, primary, gmap, w, h, rgb)
    made("o17", 17, 9, 132)
    made("o45", 45, 37, 133)
    made("o18", 18, 9, 134)
    made("o17x8", 17, 8, 135)
    made("o16x9", 16, 9, 136)
    made("og17", 17, 9, 137, rgb=True)
    made("og45", 45, 37, 138, rgb=True)
    assert list(out) == FILE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def primary_buffer(name):
    """the oracle's decode of the file's primary image in the reference's buffer: floor(3 w h / 2) bytes, zero where the decoder writes
    nothing; the first `need` bytes are what a decode call returns"""
    from oracle import jpegr_oracle as J
    f = files()[name]
    st, planes, w, h, gray = O.jpeg_decode("orc", f.primary)
    assert st == f.w * f.h + 2 * (f.w * f.h // 4) and not gray and (w, h) == (f.w, f.h)
    buf = J.reference_buffer(planes, w, h)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def file_expected(name, fmt, boost=FLT_MAX):
    """the HDR rendition of the file: oracle/jpegr_oracle.decode (one-component map), or the oracle's applyGainMap per channel over the
    oracle's decode of the primary image in the reference's buffer and Pillow's RGB of the map (three components)"""
    import io

    from PIL import Image

    from oracle import jpegr_oracle as J
    from tests import rgbmap_cases as R
    f = files()[name]
    if not f.rgb:
        st, out, w, h, _, _ = J.decode(f.data, fmt, boost, threads=2)
        assert st == 0 and (w, h) == (f.w, f.h)
        want = out[:BPP[fmt] * w * h].copy()
    else:
        imgs = J.find_images(f.data)
        md = J.metadata_from_xmp(J.app_segment(f.data[imgs[1][0]:imgs[1][0] + imgs[1][1]], 0xE1, J.XMP_NS))
        omd = O.Metadata(float(md["max"]), float(md["min"]), float(md["gamma"]), float(md["off_sdr"]), float(md["off_hdr"]), float(md["capmin"]),
                         float(md["capmax"]), 1 if md["version"] == "1.0" else 0)
        rgb = np.asarray(Image.open(io.BytesIO(f.gmap)).convert("RGB"))
        gamut = J.gamut_from_icc(J.app_segment(f.primary, 0xE2, J.ICC_ID))
        want = R.composite_apply(O, O.yuv420_image(primary_buffer(name), f.w, f.h, gamut), rgb, omd, fmt, boost)[:BPP[fmt] * f.w * f.h].copy()
    want.setflags(write=False)
    return want
