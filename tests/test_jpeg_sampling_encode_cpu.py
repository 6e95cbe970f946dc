"""No GPU: what the expected files of tests/test_gpu_jpeg_sampling_encode.py rest on.

tests/jpeg_sampling_encode_oracle.py's interleaver -- each plane's blocks from a Pillow single-plane file, emitted again in the MCU
order of (hs, vs) -- is pinned, with the same code for every sampling, to Pillow's direct files for (1,1), (2,1) and (2,2) at every
size, quality and setting of the GPU matrix, and to IJG libjpeg's raw-data files of tests/golden/encode_sampling/ for (1,2), which
Pillow cannot write.  The pixel-doubling identity behind Pillow's direct 4:2:2 and 4:2:0 files is thereby checked at odd widths too.
"""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests import jpeg_optimize_oracle as JO
from tests import jpeg_restart_oracle as RO
from tests import jpeg_sampling_encode_cases as EC
from tests import jpeg_sampling_encode_oracle as SO
from tests import sampling_cases as SC

PIL = pytest.importorskip("PIL")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (2, 2)])
def test_interleaver_equals_pillows_direct_file(hs, vs):
    for k, (w, h, q) in enumerate(EC.matrix_sizes()):
        y, cb, cr = EC.planes(w, h, hs, vs, 50 + k)
        assert SO.encode_planes(y, cb, cr, hs, vs, q) == SO.pillow_ycbcr(y, cb, cr, hs, vs, q), (w, h, q)


@pytest.mark.parametrize("hs,vs", [(1, 1), (2, 1), (2, 2)])
def test_optimise_and_restart_on_top_equal_pillows(hs, vs):
    """transcode_restart of the interleaver's file is Pillow's file with the same settings: the settings of the GPU matrix"""
    for k, (w, h, q) in enumerate([(17, 9, 90), (45, 37, 50), (130, 70, 100)]):
        y, cb, cr = EC.planes(w, h, hs, vs, 70 + k)
        base = SO.encode_planes(y, cb, cr, hs, vs, q)
        for opt in (False, True):
            for ri, rows in EC.SETTINGS:
                if (ri, rows, opt) == (0, 0, False):
                    continue
                want = SO.pillow_ycbcr(y, cb, cr, hs, vs, q, optimize=opt, restart_marker_blocks=ri, restart_marker_rows=rows)
                assert RO.transcode_restart(base, ri, rows, opt) == want, (w, h, q, opt, ri, rows)


@pytest.mark.parametrize("case", EC.GOLDEN_CASES, ids=lambda c: "s%d%d_%dx%d_q%d" % (c[2], c[3], c[0], c[1], c[4]))
def test_interleaver_equals_ijg_libjpegs_raw_data_file(case):
    w, h, hs, vs, q = case
    y, cb, cr, want = EC.golden(*case)
    assert SO.encode_planes(y, cb, cr, hs, vs, q) == want


def test_440_files_open_in_pillow():
    from PIL import Image
    for k, (w, h, q) in enumerate(EC.matrix_sizes()[::4]):
        y, cb, cr = EC.planes(w, h, 1, 2, 90 + k)
        for ri, rows, opt in ((0, 0, False), (2, 0, True)):
            data = EC.expected(EC.item(y, cb, cr, 1, 2, q), ri, rows, opt)
            im = Image.open(io.BytesIO(data))
            im.draft("YCbCr", (w, h))
            assert im.size == (w, h) and im.mode == "YCbCr"
            a = JO.first_segment(data, 0xC0)
            assert data[a + 11] == 0x12 and data[a + 14] == data[a + 17] == 0x11
            assert np.asarray(im).shape == (h, w, 3)


# ---- the dummy-block rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,vs,w,h", [(2, 1, 17, 9), (2, 1, 40, 8), (2, 1, 264, 200), (1, 2, 9, 17), (1, 2, 16, 24), (1, 2, 45, 37)])
def test_dummy_blocks_have_zero_ac_and_the_dc_in_front(hs, vs, w, h):
    """an odd luma width in blocks (2x1) leaves the right-hand block of the last MCU column without samples, an odd luma height in
    blocks (1x2) the bottom block of the last MCU row: zero AC (one EOB) and a DC difference of 0 to the block before it in the MCU"""
    ybw, ybh = (w + 7) // 8, (h + 7) // 8
    assert (ybw if hs == 2 else ybh) % 2 == 1
    y, cb, cr = EC.planes(w, h, hs, vs, 3)
    jpg = EC.expected(EC.item(y, cb, cr, hs, vs, 90))
    dummies = SO.dummy_blocks(jpg)
    assert len(dummies) == (ybh if hs == 2 else ybw)
    for i, dc, before, ac in dummies:
        assert dc == before and ac == [(0, 0, 0)] and i % 4 == 1
    if (hs, vs) == (2, 1):
        assert jpg == SO.pillow_ycbcr(y, cb, cr, hs, vs, 90)


def test_restart_rows_use_the_samplings_mcus_per_row():
    y, cb, cr = EC.planes(45, 37, 1, 2, 4)
    it = EC.item(y, cb, cr, 1, 2, 90)
    jpg = EC.expected(it, 0, 1)
    a = JO.first_segment(jpg, 0xDD)
    assert (jpg[a + 4] << 8 | jpg[a + 5]) == 6          # ceil(45 / 8) MCUs of 8 x 16 pixels
    y, cb, cr = EC.planes(45, 37, 2, 1, 4)
    jpg = EC.expected(EC.item(y, cb, cr, 2, 1, 90), 0, 1)
    a = JO.first_segment(jpg, 0xDD)
    assert (jpg[a + 4] << 8 | jpg[a + 5]) == 3          # ceil(45 / 16) MCUs of 16 x 8 pixels


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_abi_stays():
    for name in ("uhdr_hip_jpeg_encode_planes_batch_opts", "uhdr_hip_jpeg_encode_rgba_batch_opts", "uhdr_hip_jpegr_encode_packed_sampling_batch"):
        assert re.search(r"\bint %s\(" % name, HEADER), name
        assert name in api.SIGNATURES
    m = re.search(r"#define UHDR_HIP_ABI_VERSION\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == 3 and api.ABI_VERSION == 3
    shim = open(os.path.join(ROOT, "include", "ultrahdr_hip", "ultrahdr_hip.h")).read()
    assert "setPrimarySampling" in shim


def test_calls_refuse_before_the_device():
    """no GPU here: what these calls answer, they answer without one"""
    lib = api.load()
    assert lib.uhdr_hip_abi_version() == 3
    n1 = (C.c_int * 1)(90)
    img = api.image_array([api.rgba8888_image(0x1000, 8, 8, api.CG_BT709, 8)])
    outp, cap, size, stat = (C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_size_t * 1)(0), (C.c_int * 1)(7)
    bad = api.encode_opts()
    bad.struct_size = 12
    U = api.ERROR_UNSUPPORTED_FEATURE
    for sampling in (api.PIX_FMT_YUV440, api.PIX_FMT_MONOCHROME, api.PIX_FMT_RGBA8888, -1, 99):
        assert lib.uhdr_hip_jpeg_encode_rgba_batch_opts(1, img, n1, None, None, outp, cap, size, stat, sampling, None, api.MEM_DEVICE, None) == U
    for sampling in (api.PIX_FMT_YUV444, api.PIX_FMT_YUV422, api.PIX_FMT_YUV420):
        assert lib.uhdr_hip_jpeg_encode_rgba_batch_opts(1, img, n1, None, None, outp, cap, size, stat, sampling, C.byref(bad), api.MEM_DEVICE, None) == U
        assert lib.uhdr_hip_jpeg_encode_rgba_batch_opts(1, None, n1, None, None, outp, cap, size, stat, sampling, None, api.MEM_DEVICE, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_encode_planes_batch_opts(1, img, n1, None, None, outp, cap, size, stat, C.byref(bad), api.MEM_DEVICE, None) == U
    assert lib.uhdr_hip_jpeg_encode_planes_batch_opts(1, None, n1, None, None, outp, cap, size, stat, None, api.MEM_DEVICE, None) == api.ERROR_BAD_PTR
    # per-file checks that end the call before the device: NULL chroma, a chroma stride below the chroma width, a size of 0
    y = np.zeros(64 * 3, np.uint8)
    for fmt in (api.PIX_FMT_YUV444, api.PIX_FMT_YUV422, api.PIX_FMT_YUV440):
        cw = api.chroma_size(fmt, 17, 9)[0]
        d = api.ycbcr_image(y.ctypes.data, 17, 9, api.CG_UNSPECIFIED, fmt)
        d.chroma_data = None
        e = api.ycbcr_image(y.ctypes.data, 17, 9, api.CG_UNSPECIFIED, fmt, chroma_stride=cw - 1)
        f = api.ycbcr_image(y.ctypes.data, 17, 9, api.CG_UNSPECIFIED, fmt, luma_stride=16)
        g = api.ycbcr_image(y.ctypes.data, 0, 9, api.CG_UNSPECIFIED, fmt)
        h = api.ycbcr_image(y.ctypes.data, 65501, 9, api.CG_UNSPECIFIED, fmt)
        imgs = api.image_array([d, e, f, g, h])
        q5, o5, c5, s5, t5 = (C.c_int * 5)(*[90] * 5), (C.c_void_p * 5)(), (C.c_size_t * 5)(), (C.c_size_t * 5)(), (C.c_int * 5)(*[7] * 5)
        rc = lib.uhdr_hip_jpeg_encode_planes_batch_opts(5, imgs, q5, None, None, o5, c5, s5, t5, None, api.MEM_HOST, None)
        want = [api.ERROR_BAD_PTR, api.ERROR_INVALID_STRIDE, api.ERROR_INVALID_STRIDE, api.ERROR_RESOLUTION_MISMATCH, api.ERROR_RESOLUTION_MISMATCH]
        assert list(t5) == want and rc == want[0], (fmt, rc, list(t5))
    hdr = api.image_array([api.rgba1010102_image(0x1000, 8, 8, api.CG_BT2100, 8)])
    for ps in (api.PIX_FMT_YUV440, api.PIX_FMT_MONOCHROME, 77):
        assert lib.uhdr_hip_jpegr_encode_packed_sampling_batch(1, hdr, img, api.TF_HLG, 90, None, None, outp, cap, size, stat, 0, ps, None, api.MEM_DEVICE, None) == U
    assert lib.uhdr_hip_jpegr_encode_packed_sampling_batch(1, hdr, img, api.TF_HLG, 90, None, None, outp, cap, size, stat, 0, api.PIX_FMT_YUV444, C.byref(bad),
                                                           api.MEM_DEVICE, None) == U


def test_restart_mcus_helper_covers_every_sampling():
    lib = api.load()
    out = C.c_uint32(0)
    o = api.encode_opts(0, 0, 2)
    for w, mcu_w, want in ((45, 16, 6), (45, 8, 12), (264, 16, 34)):     # 4:2:0 and 4:2:2: 16; 4:4:4, 4:4:0 and one plane: 8
        assert lib.uhdr_hip_jpeg_restart_mcus(C.byref(o), w, mcu_w, C.byref(out)) == 0 and out.value == want
