"""Gain maps at any scale factor, what runs without a GPU: the model of tests/scaled_cases.py against the
oracle at factor 4, the interface, and the statuses the two calls answer before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from oracle import oracle as O
from tests import gainmap_md_cases as M
from tests import rgbmap_cases as R
from tests import scaled_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()
NEW_CALLS = ("uhdr_hip_generate_gainmap_scaled_batch", "uhdr_hip_jpegr_encode_scaled_batch", "uhdr_hip_generate_gainmap_scaled_probe")


@pytest.fixture(scope="module")
def lib():
    return api.load()


@pytest.fixture(scope="module")
def mem():
    """16-byte aligned host memory: the checks look at pointers, never at what they point to"""
    buf = np.zeros(1 << 16, np.uint8)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16


# ------------------------------------------------------------------ the model, pinned at factor 4

@pytest.mark.parametrize("w,h,seed,tf,gamuts", [(40, 24, 11, S.TF_HLG, (S.CG_709, S.CG_2100)), (36, 20, 12, S.TF_PQ, (S.CG_P3, S.CG_P3))])
def test_model_at_factor_4_is_the_oracle(w, h, seed, tf, gamuts):
    p = S.pair(w, h, seed, gamuts[0], gamuts[1])
    yi, pi = p.oracle_images()
    st, want, _ = O.generate("orc_", yi, pi, tf)
    assert st == 0
    mono, _ = S.map_of(yi, pi, tf, 4)
    assert np.array_equal(mono, want)
    rgb, _ = S.map_of(yi, pi, tf, 4, rgb=True)
    assert np.array_equal(rgb[:, :, :3], R.channel_bytes(O, yi, pi, tf)) and (rgb[:, :, 3] == 0xFF).all()


# ------------------------------------------------------------------ the interface

def test_header_and_binding_name_the_new_interface(lib):
    m = re.search(r"#define UHDR_HIP_ABI_VERSION\s+(\d+)", HEADER)
    assert m and int(m.group(1)) == 3 and api.ABI_VERSION == 3 and lib.uhdr_hip_abi_version() == 3
    for fn in NEW_CALLS:
        assert re.search(r"\bint %s\(" % fn, HEADER), fn
        assert fn in api.SIGNATURES and getattr(lib, fn) is not None, fn
    # the packed generate's signature with sdr_is_601 and the factor; the rgbmap encode's with rgb_map and the factor
    sig = api.SIGNATURES["uhdr_hip_generate_gainmap_packed_batch"][1]
    assert api.SIGNATURES["uhdr_hip_generate_gainmap_scaled_batch"][1] == sig[:-2] + [C.c_int, C.c_int, C.c_int] + sig[-1:]
    sig = api.SIGNATURES["uhdr_hip_jpegr_encode_rgbmap_batch"][1]
    assert api.SIGNATURES["uhdr_hip_jpegr_encode_scaled_batch"][1] == sig[:-2] + [C.c_int, C.c_int] + sig[-2:]


# ------------------------------------------------------------------ statuses, no device

def test_generate_statuses_in_their_order(lib, mem):
    buf, base = mem
    f = lib.uhdr_hip_generate_gainmap_scaled_batch
    img = (api.Image * 1)()
    assert f(-1, img, img, api.TF_HLG, None, None, img, 0, 0, 1, None) == api.ERROR_BAD_PTR
    for k in range(3):
        args = [img, img, img]
        args[k] = None
        # (a bad factor as well: the call-level BAD_PTR comes first)
        assert f(1, args[0], args[1], api.TF_HLG, None, None, args[2], 0, 0, 0, None) == api.ERROR_BAD_PTR, k

    def call(yuv, p010, s, tf=api.TF_HLG, md=None, dest=None, rgb=0):
        d = api.out_image(base + 32768) if dest is None else dest
        return f(1, C.byref(yuv), C.byref(p010), tf, None if md is None else C.byref(md), None, C.byref(d), 0, rgb, s, None)
    yuv = api.yuv420_image(base, 16, 16, api.CG_BT709)
    p010 = api.p010_image(base + 1024, 16, 16, api.CG_BT2100)
    bad_md = M.api_metadata(api, M.CASES["default"], version=b"1.1")
    good_md = M.api_metadata(api, S.MD_CASE)
    # the factor, directly after the call-level BAD_PTR: in front of NULL data, bad metadata, a mismatch, a bad transfer function
    for s in (0, -1, 129):
        assert call(yuv, p010, s) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, s
        assert call(api.yuv420_image(None, 16, 16, -1, chroma_ptr=base), api.p010_image(base, 16, 8, 7), s, tf=9, md=bad_md, rgb=1) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, s
        assert f(0, None, None, 9, None, None, None, 0, 0, s, None) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, s
    # the metadata behind it, in the md call's place: behind the images' pointers, in front of their other checks
    assert call(yuv, p010, 2, md=bad_md) == api.ERROR_BAD_METADATA
    assert call(yuv, api.p010_image(base + 1024, 16, 8, api.CG_BT2100), 2, tf=9, md=bad_md) == api.ERROR_BAD_METADATA
    assert call(api.yuv420_image(None, 16, 16, api.CG_BT709, chroma_ptr=base), p010, 2, md=bad_md) == api.ERROR_BAD_PTR
    # per image, the selected call's checks first, then the image against the factor
    small_y, small_p = api.yuv420_image(base, 6, 6, api.CG_BT709), api.p010_image(base + 1024, 6, 6, api.CG_BT2100)
    for md in (None, good_md):
        for rgb in (0, 1):
            assert call(small_y, small_p, 8, md=md, rgb=rgb) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, (md, rgb)
            assert call(small_y, api.p010_image(base + 1024, 6, 8, api.CG_BT2100), 8, md=md, rgb=rgb) == api.ERROR_RESOLUTION_MISMATCH
            assert call(small_y, api.p010_image(base + 1024, 6, 6, -1), 8, md=md, rgb=rgb) == api.ERROR_INVALID_COLORGAMUT
            assert call(small_y, small_p, 8, tf=9, md=md, rgb=rgb) == api.ERROR_INVALID_TRANS_FUNC
            assert call(small_y, small_p, 8, md=md, rgb=rgb, dest=api.out_image(None)) == api.ERROR_BAD_PTR
        assert call(small_y, small_p, 8, md=md, rgb=1, dest=api.out_image(base + 32770)) == api.ERROR_BAD_PTR
    assert call(api.yuv420_image(base, 16, 6, api.CG_BT709), api.p010_image(base + 1024, 16, 6, api.CG_BT2100), 8) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR
    assert call(api.yuv420_image(base, 128, 2, api.CG_BT709), api.p010_image(base + 1024, 128, 2, api.CG_BT2100), 128) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR
    # n == 0: nothing to look at but the factor and the transfer function
    assert f(0, None, None, 7, None, None, None, 0, 0, 3, None) == api.ERROR_INVALID_TRANS_FUNC
    assert buf.max() == 0   # nothing was written


def test_encode_statuses_in_their_order(lib, mem):
    buf, base = mem
    f = lib.uhdr_hip_jpegr_encode_scaled_batch
    img = (api.Image * 1)()
    out, cap, size, stat = (C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_size_t * 1)(0), (C.c_int * 1)(7)
    assert f(-1, img, img, api.TF_HLG, 90, None, None, out, cap, size, stat, 0, 2, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    for k in range(4):
        args = [img, out, cap, size]
        args[k] = None
        assert f(1, args[0], img, api.TF_HLG, 90, None, None, args[1], args[2], args[3], stat, 0, 0, api.MEM_HOST, None) == api.ERROR_BAD_PTR, k
    # the quality in front of the factor, the factor in front of every file
    for bad in (-1, 101):
        assert f(1, img, img, api.TF_HLG, bad, None, None, out, cap, size, stat, 0, 0, api.MEM_HOST, None) == api.ERROR_INVALID_QUALITY_FACTOR
    for s in (0, -1, 129):
        assert f(1, img, img, api.TF_HLG, 90, None, None, out, cap, size, stat, 1, s, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR, s
    assert list(stat) == [7]
    # per file, behind API-1's own checks: a size the factor does not divide.  Every file fails, so no device is touched
    yb, pb, ob = base, base + 16384, base + 49152
    P = lambda w, h, g=api.CG_BT2100: api.p010_image(pb, w, h, g)        # noqa: E731
    Y = lambda w, h, g=api.CG_BT709: api.yuv420_image(yb, w, h, g)       # noqa: E731
    cases = [
        (P(64, 50), Y(64, 50), ob, 8, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (P(60, 48), Y(60, 48), ob, 8, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (P(64, 50), Y(64, 50), ob, 3, api.ERROR_UNSUPPORTED_WIDTH_HEIGHT),
        (P(64, 50, -1), Y(64, 50), ob, 8, api.ERROR_INVALID_COLORGAMUT),
        (P(64, 50), Y(64, 48), ob, 8, api.ERROR_RESOLUTION_MISMATCH),
        (P(64, 50), Y(64, 50), None, 8, api.ERROR_BAD_PTR),
    ]
    for p, y, o, s, want in cases:
        for rgb in (0, 1):
            stat = (C.c_int * 1)(7)
            rc = f(1, C.byref(p), C.byref(y), api.TF_HLG, 90, None, None, (C.c_void_p * 1)(o), (C.c_size_t * 1)(4096), (C.c_size_t * 1)(), stat, rgb, s,
                   api.MEM_HOST, None)
            assert rc == want and list(stat) == [want], (p.width, p.height, s, want)
    # API-0 as well (no SDR image), and a transfer function none of the three in API-1's place, in front of the size
    stat = (C.c_int * 1)(7)
    one_p = P(64, 50)
    assert f(1, C.byref(one_p), None, api.TF_PQ, 90, None, None, (C.c_void_p * 1)(ob), (C.c_size_t * 1)(4096), (C.c_size_t * 1)(), stat, 0, 8,
             api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT
    one_y = Y(64, 50)
    assert f(1, C.byref(one_p), C.byref(one_y), 9, 90, None, None, (C.c_void_p * 1)(ob), (C.c_size_t * 1)(4096), (C.c_size_t * 1)(), stat, 0, 8,
             api.MEM_HOST, None) == api.ERROR_INVALID_TRANS_FUNC
    assert buf.max() == 0   # nothing was written
