"""Packed RGBA inputs: what needs no device -- the header and the binding, every call-level and per-image status of the three new
calls that returns before the device is touched, in the stated order, the committed corpus against its generator (and Pillow where
Pillow is present), and the input condition of the gamma != 1 comparison of tests/test_gpu_packed.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests import gainmap_md_cases as M
from tests import packed_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
SHIM_HEADER = open(os.path.join(ROOT, "include", "ultrahdr_hip", "ultrahdr_hip.h")).read()
NEW_CALLS = ("uhdr_hip_generate_gainmap_packed_batch", "uhdr_hip_jpeg_encode_rgba420_batch", "uhdr_hip_jpegr_encode_packed_batch")


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.fixture(scope="module")
def mem():
    """16-byte aligned host memory: the checks look at pointers, never at what they point to"""
    buf = np.zeros(4096, np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16


def test_header_and_binding_name_the_new_interface(lib):
    for name, value in (("RGBA8888", 6), ("RGBA1010102", 7), ("RGBA_F16", 8)):
        m = re.search(r"#define UHDR_HIP_PIX_FMT_%s\s+(-?\d+)" % name, HEADER)
        assert m and int(m.group(1)) == value and getattr(api, "PIX_FMT_" + name) == value, name
    m = re.search(r"#define UHDR_HIP_ABI_VERSION\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == 3 and api.ABI_VERSION == 3 and lib.uhdr_hip_abi_version() == 3
    for fn in NEW_CALLS:
        assert re.search(r"\bint %s\(" % fn, HEADER), fn
        assert fn in api.SIGNATURES and getattr(lib, fn) is not None, fn
    # the 4:2:0 encode keeps uhdr_hip_jpeg_encode_batch's signature; the JPEG/R encode is the rgbmap call's with one more int
    assert api.SIGNATURES["uhdr_hip_jpeg_encode_rgba420_batch"] == api.SIGNATURES["uhdr_hip_jpeg_encode_batch"]
    sig = api.SIGNATURES["uhdr_hip_jpegr_encode_rgbmap_batch"][1]
    assert api.SIGNATURES["uhdr_hip_jpegr_encode_packed_batch"][1] == sig[:-2] + [C.c_int] + sig[-2:]
    for helper, fmt in ((api.rgba8888_image, 6), (api.rgba1010102_image, 7), (api.rgba_f16_image, 8)):
        im = helper(4096, 5, 3, api.CG_P3)
        assert (im.data, im.width, im.height, im.colorGamut, im.luma_stride, im.chroma_data, im.pixelFormat) == (4096, 5, 3, 1, 5, None, fmt)
        assert helper(4096, 5, 3, api.CG_P3, 8).luma_stride == 8
    assert "encodeJPEGRPacked(" in SHIM_HEADER and "generateGainMapPacked(" in SHIM_HEADER


# ------------------------------------------------------------------ uhdr_hip_generate_gainmap_packed_batch

def test_generate_statuses_in_their_order(lib, mem):
    _, base = mem
    f = lib.uhdr_hip_generate_gainmap_packed_batch
    img = (api.Image * 1)()
    assert f(-1, img, img, api.TF_HLG, None, None, img, 0, None) == api.ERROR_BAD_PTR
    for k in range(3):
        args = [img, img, img]
        args[k] = None
        assert f(1, args[0], args[1], api.TF_HLG, None, None, args[2], 0, None) == api.ERROR_BAD_PTR, k
    # n == 0: nothing to look at but the transfer function
    assert f(0, None, None, 7, None, None, None, 0, None) == api.ERROR_INVALID_TRANS_FUNC

    def call(sdr, hdr, tf=api.TF_HLG, md=None, dest=None, rgb=0):
        d = api.out_image(base + 1024) if dest is None else dest
        return f(1, C.byref(sdr), C.byref(hdr), tf, None if md is None else C.byref(md), None, C.byref(d), rgb, None)
    sdr = api.rgba8888_image(base, 8, 8, api.CG_BT709)
    h10 = api.rgba1010102_image(base + 256, 8, 8, api.CG_BT2100)
    h16 = api.rgba_f16_image(base + 256, 8, 8, api.CG_BT2100)
    bad_md = M.api_metadata(api, M.CASES["default"], version=b"1.1")
    # pixel formats first: in front of NULL data, bad metadata, a mismatch, a bad transfer function
    assert call(api.yuv420_image(base, 8, 8, api.CG_BT709), h10, md=bad_md) == api.ERROR_UNSUPPORTED_FEATURE
    assert call(sdr, api.p010_image(base, 8, 4, api.CG_BT2100), tf=9) == api.ERROR_UNSUPPORTED_FEATURE
    assert call(sdr, api.rgba8888_image(base, 8, 8, api.CG_BT2100)) == api.ERROR_UNSUPPORTED_FEATURE
    # one HDR format per call (the second image differs from the first)
    two_s, two_h = api.image_array([sdr, sdr]), api.image_array([h10, h16])
    dests = api.image_array([api.out_image(base + 1024), api.out_image(base + 1100)])
    assert f(2, two_s, two_h, api.TF_HLG, None, None, dests, 0, None) == api.ERROR_UNSUPPORTED_FEATURE
    # pointers: NULL, alignment by format (4; 8 for F16), the RGBA dest's
    assert call(api.rgba8888_image(None, 8, 8, api.CG_BT709), h10, md=bad_md) == api.ERROR_BAD_PTR
    assert call(sdr, api.rgba1010102_image(None, 8, 8, api.CG_BT2100)) == api.ERROR_BAD_PTR
    assert call(sdr, h10, dest=api.out_image(None)) == api.ERROR_BAD_PTR
    assert call(api.rgba8888_image(base + 2, 8, 8, api.CG_BT709), h10) == api.ERROR_BAD_PTR
    assert call(sdr, api.rgba1010102_image(base + 258, 8, 8, api.CG_BT2100)) == api.ERROR_BAD_PTR
    assert call(sdr, api.rgba_f16_image(base + 260, 8, 8, api.CG_BT2100), tf=api.TF_LINEAR) == api.ERROR_BAD_PTR
    assert call(sdr, h10, dest=api.out_image(base + 1026), rgb=1) == api.ERROR_BAD_PTR
    # the metadata, uhdr_hip_generate_gainmap_md_batch's validation: in front of stride, size, gamut and transfer function
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 4, api.CG_BT2100, 7), tf=9, md=bad_md) == api.ERROR_BAD_METADATA
    neg = M.api_metadata(api, (1.0, -0.5, 0.0, 1.0, 4.0, 1.0, 4.0))
    assert call(sdr, h10, md=neg) == api.ERROR_BAD_METADATA
    # per image: stride, size, unspecified gamut, transfer function against the format, any other gamut
    assert call(api.rgba8888_image(base, 8, 8, api.CG_BT709, 7), api.rgba1010102_image(base + 256, 8, 4, -1), tf=9) == api.ERROR_INVALID_STRIDE
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 4, -1, 7), tf=9) == api.ERROR_INVALID_STRIDE
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 4, -1), tf=9) == api.ERROR_RESOLUTION_MISMATCH
    assert call(sdr, api.rgba1010102_image(base + 256, 4, 8, -1), tf=9) == api.ERROR_RESOLUTION_MISMATCH
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 8, -1), tf=9) == api.ERROR_INVALID_COLORGAMUT
    assert call(api.rgba8888_image(base, 8, 8, -1), h10, tf=9) == api.ERROR_INVALID_COLORGAMUT
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 8, 5), tf=api.TF_LINEAR) == api.ERROR_INVALID_TRANS_FUNC
    for tf in (api.TF_LINEAR, api.TF_SRGB, -1):
        assert call(sdr, h10, tf=tf) == api.ERROR_INVALID_TRANS_FUNC, tf
    for tf in (api.TF_HLG, api.TF_PQ, api.TF_SRGB, -1):
        assert call(sdr, h16, tf=tf) == api.ERROR_INVALID_TRANS_FUNC, tf
    assert call(sdr, api.rgba1010102_image(base + 256, 8, 8, 5)) == api.ERROR_INVALID_COLORGAMUT
    assert call(api.rgba8888_image(base, 8, 8, 3), h16, tf=api.TF_LINEAR) == api.ERROR_INVALID_COLORGAMUT


# ------------------------------------------------------------------ uhdr_hip_jpeg_encode_rgba420_batch

def test_rgba420_statuses(lib, mem):
    _, base = mem
    img = (api.Image * 1)()
    q, out, cap, size, stat = (C.c_int * 1)(85), (C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_size_t * 1)(0), (C.c_int * 1)(7)
    f = lib.uhdr_hip_jpeg_encode_rgba420_batch
    assert f(-1, img, q, None, None, out, cap, size, stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    for k in range(5):
        args = [img, q, out, cap, size]
        args[k] = None
        assert f(1, args[0], args[1], None, None, args[2], args[3], args[4], stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR, k
    assert f(1, img, q, (C.c_void_p * 1)(None), None, out, cap, size, stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR   # icc without sizes
    for bad in (-1, 101):
        assert f(1, img, (C.c_int * 1)(bad), None, None, out, cap, size, stat, api.MEM_HOST, None) == api.ERROR_INVALID_QUALITY_FACTOR
    assert list(stat) == [7]   # call-level errors leave the statuses alone
    # per file, before any device work; a batch whose every file fails touches no device (there is none here)
    cases = [(api.rgba8888_image(None, 2, 2, 0), api.ERROR_BAD_PTR), (api.mono_image(base, 2, 2), api.ERROR_UNSUPPORTED_FEATURE),
             (api.rgba1010102_image(base, 2, 2, 0), api.ERROR_UNSUPPORTED_FEATURE),
             (api.rgba8888_image(base, 0, 2, 0), api.ERROR_RESOLUTION_MISMATCH), (api.rgba8888_image(base, 65501, 1, 0), api.ERROR_RESOLUTION_MISMATCH),
             (api.rgba8888_image(base, 1, 65501, 0), api.ERROR_RESOLUTION_MISMATCH),
             (api.rgba8888_image(base, 4, 2, 0, 3), api.ERROR_RESOLUTION_MISMATCH), (api.rgba8888_image(base, 4, 2, 0, 1 << 29), api.ERROR_RESOLUTION_MISMATCH),
             (api.rgba8888_image(base + 2, 2, 2, 0), api.ERROR_BAD_PTR)]
    n = len(cases)
    imgs = api.image_array([c[0] for c in cases])
    stat = (C.c_int * n)(*([7] * n))
    rc = f(n, imgs, (C.c_int * n)(*([85] * n)), None, None, (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_size_t * n)(), stat, api.MEM_DEVICE, None)
    assert list(stat) == [c[1] for c in cases] and rc == cases[0][1]
    # host memory: no alignment rule; an output pointer missing beside a capacity
    one = api.image_array([api.rgba8888_image(base + 2, 2, 2, 0, 1)])
    stat = (C.c_int * 1)(7)
    assert f(1, one, q, None, None, out, cap, size, stat, api.MEM_HOST, None) == api.ERROR_RESOLUTION_MISMATCH and list(stat) == [api.ERROR_RESOLUTION_MISMATCH]
    one = api.image_array([api.rgba8888_image(base, 2, 2, 0)])
    assert f(1, one, q, None, None, out, (C.c_size_t * 1)(9), size, stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR and list(stat) == [api.ERROR_BAD_PTR]


# ------------------------------------------------------------------ uhdr_hip_jpegr_encode_packed_batch

def test_jpegr_encode_packed_statuses(lib, mem):
    buf, base = mem
    img = (api.Image * 1)()
    out, cap, size, stat = (C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_size_t * 1)(0), (C.c_int * 1)(7)
    f = lib.uhdr_hip_jpegr_encode_packed_batch
    assert f(-1, img, img, api.TF_HLG, 90, None, None, out, cap, size, stat, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    for k in range(5):
        args = [img, img, out, cap, size]
        args[k] = None
        assert f(1, args[0], args[1], api.TF_HLG, 90, None, None, args[2], args[3], args[4], stat, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR, k
    assert f(1, img, img, api.TF_HLG, 90, (C.c_void_p * 1)(None), None, out, cap, size, stat, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    for bad in (-1, 101):
        assert f(1, img, img, api.TF_HLG, bad, None, None, out, cap, size, stat, 0, api.MEM_HOST, None) == api.ERROR_INVALID_QUALITY_FACTOR
    assert list(stat) == [7]
    # per file, in API-1's order, then the packed generate's own; every file fails, so no device is touched
    H = lambda *a, **k: api.rgba1010102_image(*a, **k)   # noqa: E731
    S = lambda *a, **k: api.rgba8888_image(*a, **k)      # noqa: E731
    hb, sb, ob = base + 1024, base, base + 3000
    good_h, good_s = H(hb, 8, 8, api.CG_BT2100), S(sb, 8, 8, api.CG_BT709)
    cases = [
        (H(None, 7, 8, -1), good_s, ob, api.ERROR_BAD_PTR),
        (H(hb, 7, 8, -1, 3), good_s, None, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (H(hb, 8, 6, -1, 3), good_s, None, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (H(hb, 8194, 8, -1), good_s, None, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (H(hb, 8, 8, -1, 3), good_s, None, api.ERROR_INVALID_COLORGAMUT),
        (H(hb, 8, 8, 3, 3), good_s, None, api.ERROR_INVALID_COLORGAMUT),
        (H(hb, 8, 8, api.CG_BT2100, 7), good_s, None, api.ERROR_INVALID_STRIDE),
        (good_h, S(None, 8, 8, -1), None, api.ERROR_BAD_PTR),
        (good_h, S(None, 8, 8, -1), ob, api.ERROR_BAD_PTR),
        (good_h, S(sb, 16, 8, -1, 7), ob, api.ERROR_INVALID_STRIDE),
        (good_h, S(sb, 16, 8, -1), ob, api.ERROR_RESOLUTION_MISMATCH),
        (good_h, S(sb, 8, 8, -1), ob, api.ERROR_INVALID_COLORGAMUT),
        (good_h, api.yuv420_image(sb, 8, 8, api.CG_BT709), ob, api.ERROR_UNSUPPORTED_FEATURE),
        (api.p010_image(hb, 8, 8, api.CG_BT2100), good_s, ob, api.ERROR_UNSUPPORTED_FEATURE),
        (H(hb + 2, 8, 8, api.CG_BT2100), good_s, ob, api.ERROR_BAD_PTR),
        (good_h, S(sb + 1, 8, 8, api.CG_BT709), ob, api.ERROR_BAD_PTR),
        (api.rgba_f16_image(hb, 8, 8, api.CG_BT2100), good_s, ob, api.ERROR_INVALID_TRANS_FUNC),
    ]
    n = len(cases)
    hs, ss = api.image_array([c[0] for c in cases]), api.image_array([c[1] for c in cases])
    outs = (C.c_void_p * n)(*[c[2] for c in cases])
    stat = (C.c_int * n)(*([7] * n))
    rc = f(n, hs, ss, api.TF_HLG, 90, None, None, outs, (C.c_size_t * n)(*([64] * n)), (C.c_size_t * n)(), stat, 0, api.MEM_DEVICE, None)
    assert list(stat) == [c[3] for c in cases] and rc == cases[0][3]
    # the shared transfer function: none of the three, in API-1's place (behind the HDR image's checks and out[i]); a known one that
    # does not go with the format last; F16 passes with LINEAR only
    one_h, one_s, one_o = api.image_array([good_h]), api.image_array([S(None, 8, 8, -1)]), (C.c_void_p * 1)(ob)
    stat = (C.c_int * 1)(7)
    assert f(1, one_h, one_s, 9, 90, None, None, one_o, (C.c_size_t * 1)(64), size, stat, 0, api.MEM_HOST, None) == api.ERROR_INVALID_TRANS_FUNC
    assert f(1, one_h, one_s, api.TF_LINEAR, 90, None, None, one_o, (C.c_size_t * 1)(64), size, stat, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    one_s = api.image_array([good_s])
    assert f(1, one_h, one_s, api.TF_LINEAR, 90, None, None, one_o, (C.c_size_t * 1)(64), size, stat, 0, api.MEM_HOST, None) == api.ERROR_INVALID_TRANS_FUNC
    # a NULL EXIF payload with a size: behind the SDR image's checks, in front of the pixel formats
    ex, exn = (C.c_void_p * 1)(None), (C.c_size_t * 1)(4)
    yuv = api.image_array([api.yuv420_image(sb, 8, 8, api.CG_BT709)])
    assert f(1, one_h, yuv, api.TF_HLG, 90, ex, exn, one_o, (C.c_size_t * 1)(64), size, stat, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    # host memory has no alignment rule: a misaligned pair gets as far as the transfer function
    odd_h, odd_s = api.image_array([api.rgba_f16_image(hb + 2, 8, 8, api.CG_BT2100)]), api.image_array([S(sb + 1, 8, 8, api.CG_BT709)])
    assert f(1, odd_h, odd_s, api.TF_PQ, 90, None, None, one_o, (C.c_size_t * 1)(64), size, stat, 0, api.MEM_HOST, None) == api.ERROR_INVALID_TRANS_FUNC
    assert buf.max() == 0   # nothing was written


# ------------------------------------------------------------------ the corpus

def test_the_corpus_reproduces_from_its_generator():
    names = set(os.listdir(P.DIR))
    want = set()
    for w, h, q in P.JPEG_CASES:
        want |= {"rgba_%dx%d.npy" % (w, h), "rgba_%dx%d_q%d_s2.jpg" % (w, h, q)}
        img = P.golden_rgba(w, h)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8 and np.array_equal(img, P.jpeg_image(w, h)), (w, h)
    assert names == want
    assert all(os.path.getsize(os.path.join(P.DIR, n)) < (1 << 17) for n in names)
    w, h, q = P.JPEG_CASES[-1]
    big = P.golden_jpeg_420(w, h, q)
    assert len(big) - big.index(b"\xff\xda") > 16384      # a scan of more than 16 KiB


def test_the_corpus_is_pillows():
    pytest.importorskip("PIL.Image")
    import io

    from PIL import Image
    for w, h, q in P.JPEG_CASES:
        data = P.golden_jpeg_420(w, h, q)
        assert data == P.pillow_420(P.golden_rgba(w, h), q), (w, h, q)
        im = Image.open(io.BytesIO(data))
        assert im.size == (w, h) and im.mode == "RGB" and im.layer[0][1:3] == (2, 2) and im.layer[1][1:3] == (1, 1) and not im.info.get("progressive")


# ------------------------------------------------------------------ the model and its input condition

def test_the_generators_hold_what_they_promise():
    a = P.lcg_rgba8888(40, 24, 1)
    assert a.min() == 0 and a.max() == 255
    b = P.lcg_rgba1010102(40, 24, 2)
    codes = np.stack([b & 1023, (b >> 10) & 1023, (b >> 20) & 1023])
    assert codes.min() == 0 and codes.max() == 1023 and len(np.unique(b >> 30)) == 4
    c = P.lcg_rgba_f16(40, 24, 3)
    v = c.view(np.float16).astype(np.float64)
    assert np.isfinite(v).all() and v.min() == 0 and v.max() <= 4 and (v > 1).any()
    assert ((c > 0) & (c < 0x0400)).any()   # subnormal halves
    assert np.array_equal(P.pixel_values(c, P.FMT_F16).astype(np.float16).view(np.uint16), c[:, :, :3])   # exact, subnormals included


def test_sampling_is_sequential_float32():
    """the sum the model forms is the reference's loop, not numpy's pairwise one: a block of one large value and fifteen small ones"""
    v = np.zeros((4, 4, 3), np.float32)
    v[0, 0] = 1.0
    v.reshape(-1, 3)[1:] = 2.0 ** -25
    assert P.sample(v)[0, 0, 0] == np.float32(1.0) / np.float32(16)   # every small addend is rounded away, one after the other
    vals = P.pixel_values(P.lcg_rgba8888(8, 4, 5), P.FMT_8888)
    e = np.float32(0)
    for dy in range(4):
        for dx in range(4):
            e = np.float32(e + vals[dy, 4 + dx, 1])
    assert P.sample(vals)[0, 1, 1] == np.float32(e / np.float32(16))
    assert P.sample(np.ones((6, 11, 3), np.float32)).shape == (1, 2, 3)


@pytest.mark.parametrize("fmt,tf", P.FORMS)
@pytest.mark.parametrize("rgb", [0, 1])
def test_gamma_case_has_no_byte_in_doubt(fmt, tf, rgb):
    """Input condition of the gamma != 1 comparison in tests/test_gpu_packed.py: on the chosen seeds no model value in front of the
    truncation lies within GEN_DOUBT of an integer (a gain on either clamp is the host's byte by the rule itself: M.in_doubt)"""
    sl, hl, ys, yh = P.model(40, 24, fmt, tf, P.seed_of(40, fmt, tf))
    _, v = M.encode(sl, hl, M.CASES["gamma22"]) if rgb else M.encode(ys, yh, M.CASES["gamma22"])
    assert not M.in_doubt(v).any()
    assert ((v > 0) & (v < 255)).mean() > 0.1   # and the comparison is about something: a share of the gains is off the clamps
