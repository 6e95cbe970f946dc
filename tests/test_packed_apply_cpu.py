"""Packed apply without a GPU: the separability argument behind its expected values, pinned to the oracle's scalar functions, and
the order of uhdr_hip_apply_gainmap_packed_batch's argument checks through the C-ABI (every check runs in front of the device)."""
import ctypes as C

import numpy as np
import pytest

from tests import gainmap_md_cases as M
from tests import packed_apply_cases as P


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


# ------------------------------------------------------------------ the composite against the primitives

@pytest.fixture(scope="module")
def small():
    """10 x 6 over a 5 x 3 map and over a 5 x 3 RGBA map (scale 2): interior cells and all three clamped-tap tables"""
    return P.lcg_rgba(10, 6, 91), P.lcg_map(5, 3, 92), P.lcg_map(5, 3, 93, 3)


@pytest.mark.parametrize("fmt", P.FORMATS)
@pytest.mark.parametrize("boost", P.BOOSTS)
def test_composite_equals_the_primitives(small, fmt, boost):
    rgba, plane, rgbmap = small
    for gmap in (plane, rgbmap):
        want = P.from_primitives(rgba, gmap, fmt, boost)
        got = P.composite(rgba, gmap, fmt, boost)
        assert np.array_equal(got, want), (fmt, boost, gmap.ndim)


def test_composite_on_an_odd_size():
    """15 x 5 at scale 5: the grey images carry chroma planes with rounded-up strides"""
    rgba, gmap = P.lcg_rgba(15, 5, 94), P.lcg_map(3, 1, 95)
    for fmt in (P.FMT_HLG, P.FMT_F16):
        assert np.array_equal(P.composite(rgba, gmap, fmt, 2.0), P.from_primitives(rgba, gmap, fmt, 2.0))


def test_table_is_the_grey_pixel():
    """what replaces ultrahdr.cpp:429-431: yuvToRgb of (Y, 128, 128) is (Y / 255, Y / 255, Y / 255) bit for bit, so the model's linear
    SDR value of a packed code is the planar model's of that grey pixel"""
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    grey = M.linear_sdr(y, np.full((8, 8), 128, np.uint8), np.full((8, 8), 128, np.uint8))
    t = P.srgb_table()
    for c in range(3):
        assert np.array_equal(grey[:, :, c].reshape(-1), t)


# ------------------------------------------------------------------ the order of the checks

W, H = 16, 8
ADDR = 0x10000   # never dereferenced: every check of the call runs on the host, in front of the device


def _args(api, n=1, sdr_fmt=None, map_fmt=None, sdr_ptr=ADDR, map_ptr=ADDR + 0x1000, dst_ptr=ADDR + 0x2000, stride=None, map_w=W // 4,
          map_h=H // 4, map_stride=None):
    sdr = [api.rgba8888_image(sdr_ptr, W, H, api.CG_BT709, stride) for _ in range(n)]
    maps = [api.mono_image(map_ptr, map_w, map_h) if map_fmt != api.PIX_FMT_RGBA8888 else api.rgba_map_image(map_ptr, map_w, map_h, map_stride)
            for _ in range(n)]
    for s in sdr:
        if sdr_fmt is not None:
            s.pixelFormat = sdr_fmt
    for m in maps:
        if map_fmt is not None:
            m.pixelFormat = map_fmt
    return sdr, maps, [api.out_image(dst_ptr) for _ in range(n)]


def _call(api, sdr, maps, dests, md, fmt=None, boost=4.0, mode=None, null_md=False):
    fmt = api.OUTPUT_HDR_HLG if fmt is None else fmt
    mode = api.APPLY_FAST if mode is None else mode
    n = len(sdr)
    return api.load().uhdr_hip_apply_gainmap_packed_batch(n, api.image_array(sdr) if n else None, api.image_array(maps) if n else None,
                                                          None if null_md else C.byref(md), fmt, boost, api.image_array(dests) if n else None,
                                                          mode, None)


def test_symbol_is_exported_and_bound(api):
    assert hasattr(C.CDLL(api.LIB_PATH), "uhdr_hip_apply_gainmap_packed_batch")
    assert "uhdr_hip_apply_gainmap_packed_batch" in api.SIGNATURES and callable(api.apply_gainmap_packed)


def test_check_order(api):
    good = api.metadata(4.0)
    bad_md = api.metadata(1.0, 2.0)   # max < min
    general = M.api_metadata(api, M.CASES["default"])
    lib = api.load()
    # 1. call level, in front of a wrong pixel format
    sdr, maps, dests = _args(api, sdr_fmt=api.PIX_FMT_YUV420)
    assert _call(api, sdr, maps, dests, good, null_md=True) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_apply_gainmap_packed_batch(-1, None, None, C.byref(good), 3, 4.0, None, 0, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_apply_gainmap_packed_batch(1, None, None, C.byref(good), 3, 4.0, None, 0, None) == api.ERROR_BAD_PTR
    # 2. pixel formats of EVERY image in front of anything else: image 0 has a NULL pointer, image 1 a wrong format
    sdr, maps, dests = _args(api, n=2)
    sdr[0].data = None
    sdr[1].pixelFormat = api.PIX_FMT_RGBA1010102
    assert _call(api, sdr, maps, dests, bad_md) == api.ERROR_UNSUPPORTED_FEATURE
    sdr, maps, dests = _args(api, n=2)
    sdr[0].data = None
    maps[1].pixelFormat = api.PIX_FMT_YUV420
    assert _call(api, sdr, maps, dests, bad_md) == api.ERROR_UNSUPPORTED_FEATURE
    sdr, maps, dests = _args(api, n=2)          # a map whose form differs from the first map's
    sdr[0].data = None
    maps[1].pixelFormat = api.PIX_FMT_RGBA8888
    assert _call(api, sdr, maps, dests, bad_md) == api.ERROR_UNSUPPORTED_FEATURE
    sdr, maps, dests = _args(api, n=2)          # MONOCHROME and UNSPECIFIED are one form
    maps[1].pixelFormat = -1   # UHDR_HIP_PIX_FMT_UNSPECIFIED
    sdr[0].data = None
    assert _call(api, sdr, maps, dests, bad_md) == api.ERROR_BAD_PTR
    # 3. pointers and alignment in front of the metadata
    for kw in (dict(sdr_ptr=None), dict(map_ptr=None), dict(dst_ptr=None), dict(sdr_ptr=ADDR + 2),
               dict(map_ptr=ADDR + 0x1002, map_fmt=api.PIX_FMT_RGBA8888), dict(dst_ptr=ADDR + 0x2002)):
        sdr, maps, dests = _args(api, **kw)
        assert _call(api, sdr, maps, dests, bad_md) == api.ERROR_BAD_PTR, kw
    sdr, maps, dests = _args(api, dst_ptr=ADDR + 0x2004)   # RGBA F16 stores 8 bytes per pixel, RGBA1010102 4
    assert _call(api, sdr, maps, dests, bad_md, fmt=api.OUTPUT_HDR_LINEAR) == api.ERROR_BAD_PTR
    assert _call(api, sdr, maps, dests, bad_md, fmt=api.OUTPUT_HDR_PQ) == api.ERROR_BAD_METADATA
    # 4. the metadata in front of the display boost
    sdr, maps, dests = _args(api)
    assert _call(api, sdr, maps, dests, bad_md, boost=0.5) == api.ERROR_BAD_METADATA
    assert _call(api, sdr, maps, dests, api.metadata(4.0, version=b"1.1"), boost=0.5) == api.ERROR_BAD_METADATA
    # 5. the display boost in front of the output format
    assert _call(api, sdr, maps, dests, good, boost=0.5, fmt=9) == api.ERROR_INVALID_DISPLAY_BOOST
    assert _call(api, sdr, maps, dests, good, boost=float("nan"), fmt=9) == api.ERROR_INVALID_DISPLAY_BOOST
    # 6. the output format in front of the mode
    for fmt in (api.OUTPUT_SDR, 5, -1):
        assert _call(api, sdr, maps, dests, good, fmt=fmt, mode=api.APPLY_LUT) == api.ERROR_INVALID_OUTPUT_FORMAT
    # 7. the mode in front of the per-image checks
    sdr, maps, dests = _args(api, stride=W - 1)
    assert _call(api, sdr, maps, dests, good, mode=api.APPLY_LUT) == api.ERROR_UNSUPPORTED_FEATURE
    assert _call(api, sdr, maps, dests, good, mode=7) == api.ERROR_UNSUPPORTED_FEATURE
    assert _call(api, sdr, maps, dests, general, mode=api.APPLY_EXACT_UNFILTERED) == api.ERROR_UNSUPPORTED_FEATURE
    assert _call(api, sdr, maps, dests, general, mode=api.APPLY_LUT) == api.ERROR_UNSUPPORTED_FEATURE
    assert _call(api, sdr, maps, dests, good, mode=api.APPLY_EXACT_UNFILTERED) == api.ERROR_INVALID_STRIDE
    # 8. per image: the stride in front of the scale factor
    sdr, maps, dests = _args(api, stride=W - 1, map_w=3)
    assert _call(api, sdr, maps, dests, good) == api.ERROR_INVALID_STRIDE
    sdr, maps, dests = _args(api, map_fmt=api.PIX_FMT_RGBA8888, map_stride=W // 4 - 1, map_h=3)
    assert _call(api, sdr, maps, dests, good) == api.ERROR_INVALID_STRIDE
    for kw in (dict(map_w=3), dict(map_w=0), dict(map_h=1), dict(map_w=W // 2)):   # no divisor; empty; factors 4 and 8; 2 and 4
        sdr, maps, dests = _args(api, **kw)
        assert _call(api, sdr, maps, dests, good) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, kw
    sdr, maps, dests = _args(api, n=2)   # image 0 passes everything, image 1 fails
    maps[1].width = 3
    assert _call(api, sdr, maps, dests, good) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR


def test_no_images_is_a_no_op_after_the_call_level_checks(api):
    good = api.metadata(4.0)
    assert _call(api, [], [], [], good) == api.NO_ERROR
    assert _call(api, [], [], [], api.metadata(1.0, 2.0)) == api.ERROR_BAD_METADATA
    assert _call(api, [], [], [], good, boost=0.0) == api.ERROR_INVALID_DISPLAY_BOOST
    assert _call(api, [], [], [], good, fmt=0) == api.ERROR_INVALID_OUTPUT_FORMAT
    assert _call(api, [], [], [], good, mode=api.APPLY_LUT) == api.ERROR_UNSUPPORTED_FEATURE


def test_valid_arguments_reach_the_device(api):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the CPU-only container")
    sdr, maps, dests = _args(api)
    assert _call(api, sdr, maps, dests, api.metadata(4.0)) == api.ERROR_INSUFFICIENT_RESOURCE
    with pytest.raises(api.UhdrHipError):
        api.apply_gainmap_packed(sdr, maps, api.metadata(4.0), api.OUTPUT_HDR_HLG, 4.0, [ADDR + 0x2000])


def test_shim_declares_and_exports_the_packed_apply():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "applyGainMapPacked(" in open(os.path.join(root, "include", "ultrahdr_hip", "ultrahdr_hip.h")).read()
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(root, "libultrahdr_dev_amd", "libultrahdr_shim.so")]).decode()
    assert "ultrahdr::applyGainMapPacked(" in out
