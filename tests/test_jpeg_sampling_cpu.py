"""Opt-in decode of 4:4:4, 4:2:2 and 4:4:0 JPEGs (UHDR_HIP_DECODE_ANY_SAMPLING): what needs no device -- the header and the binding,
size probes through the *_ex calls for every file of tests/golden/sampling/, flags == 0 against the calls without flags, and the
samplings that stay refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests.sampling_cases import FIXTURES, FORMATS, chroma_size, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "uhdr_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    return api.load()


def _probe(lib, data, decode_to, flags, ex=True):
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    d = api.Image()
    if ex:
        rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, None, 0, C.byref(d), api.MEM_HOST, None, flags)
    elif decode_to == api.DECODE_TO_RGBA:
        rc = lib.uhdr_hip_jpeg_decode_rgba(buf.ctypes.data, len(data), None, 0, C.byref(d), api.MEM_HOST, None)
    else:
        rc = lib.uhdr_hip_jpeg_decode(buf.ctypes.data, len(data), None, 0, C.byref(d), api.MEM_HOST, None)
    return rc, (d.data, d.width, d.height, d.colorGamut, d.chroma_data, d.luma_stride, d.chroma_stride, d.pixelFormat)


def test_header_and_binding_name_the_new_interface():
    for name, value in (("UHDR_HIP_PIX_FMT_YUV444", 3), ("UHDR_HIP_PIX_FMT_YUV422", 4), ("UHDR_HIP_PIX_FMT_YUV440", 5),
                        ("UHDR_HIP_DECODE_ANY_SAMPLING", 1), ("UHDR_HIP_ABI_VERSION", 3)):
        m = re.search(r"#define %s\s+(-?\d+)" % name, HEADER)
        assert m and int(m.group(1)) == value, name
    assert (api.PIX_FMT_YUV444, api.PIX_FMT_YUV422, api.PIX_FMT_YUV440, api.DECODE_ANY_SAMPLING, api.ABI_VERSION) == (3, 4, 5, 1, 3)
    for fn in ("uhdr_hip_jpeg_decode_batch_ex", "uhdr_hip_jpegr_decode_batch_ex", "uhdr_hip_jpeg_decode_ex", "uhdr_hip_jpegr_decode_ex"):
        assert re.search(r"\bint %s\(" % fn, HEADER), fn
        assert fn in api.SIGNATURES and api.SIGNATURES[fn][1][-1] is C.c_int, fn
    assert api.load().uhdr_hip_abi_version() == 3


def test_descriptor_helper_lays_planes_out_as_the_decoder_does():
    for fmt, (cw, ch) in ((api.PIX_FMT_YUV444, (45, 37)), (api.PIX_FMT_YUV422, (23, 37)), (api.PIX_FMT_YUV440, (45, 19))):
        assert api.chroma_size(fmt, 45, 37) == (cw, ch)
        im = api.ycbcr_image(4096, 45, 37, api.CG_BT709, fmt)
        assert (im.chroma_data, im.luma_stride, im.chroma_stride, im.pixelFormat) == (4096 + 45 * 37, 45, cw, fmt)
    assert api.chroma_size(api.PIX_FMT_YUV420, 46, 38) == (23, 19)


@pytest.mark.parametrize("name", FIXTURES)
def test_size_probe_of_every_fixture(lib, name):
    """out == NULL: ERROR_INSUFFICIENT_RESOURCE and a filled descriptor, without a device"""
    hs, vs, w, h = fixture(name)[:4]
    data = fixture(name)[4]
    cw, ch = chroma_size(hs, vs, w, h)
    rc, d = _probe(lib, data, api.DECODE_TO_YCBCR, api.DECODE_ANY_SAMPLING)
    assert rc == api.ERROR_INSUFFICIENT_RESOURCE
    assert d == (None, w, h, api.CG_UNSPECIFIED, w * h, w, cw, FORMATS[(hs, vs)])   # chroma_data = out + w * h with out == NULL
    # the batch: the same statuses and descriptors, and what a capacity one byte short gives
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    jp, js = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data), (C.c_size_t * 2)(len(data), len(data))
    need = w * h + 2 * cw * ch
    host = np.zeros(need, np.uint8)
    outs, caps = (C.c_void_p * 2)(None, host.ctypes.data), (C.c_size_t * 2)(0, need - 1)
    descs, stat = (api.Image * 2)(), (C.c_int * 2)(7, 7)
    rc = lib.uhdr_hip_jpeg_decode_batch_ex(2, jp, js, api.DECODE_TO_YCBCR, outs, caps, descs, stat, api.MEM_HOST, None, api.DECODE_ANY_SAMPLING)
    assert rc == api.ERROR_INSUFFICIENT_RESOURCE and list(stat) == [api.ERROR_INSUFFICIENT_RESOURCE] * 2
    assert (descs[1].data, descs[1].chroma_data - descs[1].data, descs[1].chroma_stride, descs[1].pixelFormat) == (host.ctypes.data, w * h, cw, FORMATS[(hs, vs)])
    # RGBA: w * h * 4 bytes whatever the sampling
    rc, d = _probe(lib, data, api.DECODE_TO_RGBA, api.DECODE_ANY_SAMPLING)
    assert rc == api.ERROR_INSUFFICIENT_RESOURCE and d[1:3] == (w, h) and d[5] == w


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("decode_to", [api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA])
def test_without_the_flag_nothing_changes(lib, name, decode_to):
    """flags == 0: the status and the descriptor of today's call -- UNKNOWN_ERROR, as the reference's decoder refuses these samplings"""
    data = fixture(name)[4]
    old = _probe(lib, data, decode_to, 0, ex=False)
    assert _probe(lib, data, decode_to, 0) == old
    assert old[0] == api.UNKNOWN_ERROR


def test_a_420_file_is_the_same_call_with_or_without_the_flag(lib):
    data = open(os.path.join(ROOT, "tests", "golden", "jpeg_image.jpg"), "rb").read()
    for decode_to in (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA):
        old = _probe(lib, data, decode_to, 0, ex=False)
        assert old[0] == api.ERROR_INSUFFICIENT_RESOURCE
        assert _probe(lib, data, decode_to, 0) == old and _probe(lib, data, decode_to, api.DECODE_ANY_SAMPLING) == old


def _with_sampling(data, comp, factors):
    """the sampling byte of component `comp` in the frame header of a baseline file replaced"""
    b = bytearray(data)
    at = bytes(b).find(b"\xff\xc0")
    assert at > 0 and b[at + 9] == 3
    b[at + 11 + 3 * comp] = factors
    return bytes(b)


def test_still_refused_with_the_flag(lib):
    data = fixture("s11_base_45x37")[4]
    for decode_to in (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA):
        for bits in (2, 4, 0x40000000, -2):   # an unknown flag bit (with or without the known one): the call itself is refused
            buf = np.frombuffer(data + b"\0" * 8, np.uint8)
            d = api.Image()
            assert lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, None, 0, C.byref(d), api.MEM_HOST, None, bits) == api.ERROR_UNSUPPORTED_FEATURE
            jp, js, st = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(data)), (C.c_int * 1)(7)
            descs = (api.Image * 1)()
            assert lib.uhdr_hip_jpeg_decode_batch_ex(1, jp, js, decode_to, None, None, descs, st, api.MEM_HOST, None, bits) == api.ERROR_UNSUPPORTED_FEATURE
            assert st[0] == 7   # a call-level error touches no per-file status
        # 4:1:1 (luma 4x1), luma 1x4, a chroma factor of 2 on either chroma component
        for comp, factors in ((0, 0x41), (0, 0x14), (1, 0x21), (2, 0x12), (1, 0x22)):
            rc, d = _probe(lib, _with_sampling(data, comp, factors), decode_to, api.DECODE_ANY_SAMPLING)
            assert rc == api.UNKNOWN_ERROR, (comp, hex(factors))
    # JPEG/R entry points: the same call-level refusal
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    d = api.Image()
    assert lib.uhdr_hip_jpegr_decode_ex(buf.ctypes.data, len(data), api.OUTPUT_SDR, 1.0, None, 0, C.byref(d), None, api.APPLY_EXACT, api.MEM_HOST, None,
                                        2) == api.ERROR_UNSUPPORTED_FEATURE
    jp, js = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(data))
    descs = (api.Image * 1)()
    assert lib.uhdr_hip_jpegr_decode_batch_ex(1, jp, js, api.OUTPUT_SDR, 1.0, None, None, descs, None, None, api.APPLY_EXACT, api.MEM_HOST, None,
                                              8) == api.ERROR_UNSUPPORTED_FEATURE


def test_fixture_corpus_is_small_and_complete():
    d = os.path.join(ROOT, "tests", "golden", "sampling")
    sizes = [os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)]
    assert max(sizes) < 200 * 1000 and sum(sizes) < 1500 * 1000
    assert len(FIXTURES) == 3 * (3 * 5 + 1)
    for name in FIXTURES:
        hs, vs, w, h, data, planes = fixture(name)
        cw, ch = chroma_size(hs, vs, w, h)
        assert planes.size == w * h + 2 * cw * ch
        if "big" in name:   # more than 256 subsequences of 512 bits: the decode crosses a workgroup
            assert len(data) > 16 * 1024 + 1024


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_planes_through_the_upsampling_formulas_are_pillows_rgb(name):
    """ties the corpus (IJG libjpeg's planes) to libjpeg-turbo's decode, which is what the device's RGBA is compared with"""
    import io

    from PIL import Image

    from tests.sampling_cases import upsampled_rgb
    hs, vs, w, h, data, planes = fixture(name)
    want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(upsampled_rgb(hs, vs, w, h, planes), want)


def test_host_parsers_with_the_flag_under_sanitizers(tmp_path):
    """the header parser and the progressive decoder with any_sampling on, built with AddressSanitizer + UBSan on the CPU as a
    stand-alone program (tests/cpp/fuzz_sampling_parsers.cpp): the small fixtures as they are, then mutated"""
    import subprocess
    csrc = os.path.join(ROOT, "libultrahdr_dev_amd", "csrc")
    exe = str(tmp_path / "fuzz_sampling")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "fuzz_sampling_parsers.cpp"), os.path.join(csrc, "uhdr_jpeg_hdr.cpp"),
                           os.path.join(csrc, "uhdr_jpeg_prog.cpp"), "-o", exe])
    seeds = [os.path.join(ROOT, "tests", "golden", "sampling", n + ".jpg") for n in FIXTURES if "big" not in n and "130x70" not in n]
    r = subprocess.run([exe] + seeds + ["20000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
