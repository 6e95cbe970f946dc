"""-m gpu: uhdr_hip_jpegr_edit_batch -- n JPEG/R files in, n edited JPEG/R files out, nothing uncompressed crossing PCIe -- against
the oracle's own composition: decode both JPEGs, addEffects on both, encodeJPEGR API-x with the parsed metadata, the ICC gamut and
the extracted EXIF.  Byte for byte."""
import ctypes as C

import numpy as np
import pytest

from tests import effects_chain_cases as K

pytestmark = pytest.mark.gpu
QUALITY = 90


@pytest.fixture(scope="module")
def J():
    from oracle import jpegr_oracle
    return jpegr_oracle


@pytest.fixture(scope="module")
def inputs(orc, J):
    """{(w, h): [file with an EXIF payload, file without]}"""
    out = {}
    for k, (w, h) in enumerate(((64, 48), (96, 64), (48, 80))):
        p010, yuv = orc.lcg_frame(w, h, 300 + k)
        out[(w, h)] = [J.encode_api1(p010, yuv, w, h, orc.CG_BT709, orc.CG_BT2100, orc.TF_HLG, 90, exif=e) for e in (b"Exif\0\0II*\0edit-batch", None)]
    return out


def _expected(orc, J, data, sdr_chain, gm_chain, sdr_gamut=-1):
    """-> (status, bytes): the per-file order of the header"""
    imgs = J.find_images(data)
    if len(imgs) < 2:
        return (-20006 if not imgs else -20003), None
    pj, gj = data[imgs[0][0]:imgs[0][0] + imgs[0][1]], data[imgs[1][0]:imgs[1][0] + imgs[1][1]]
    st, planes, w, h, gray = orc.jpeg_decode("orc", pj)
    gst, gplanes, gw, gh, _ = orc.jpeg_decode("orc", gj)
    if st <= 0 or gray or gst <= 0:
        return -20002, None
    md = J.metadata_from_xmp(J.app_segment(gj, 0xE1, J.XMP_NS))
    if md is None:
        return -20005, None
    gamut = J.gamut_from_icc(J.app_segment(pj, 0xE2, J.ICC_ID))
    if gamut == orc.CG_UNSPECIFIED:
        gamut = sdr_gamut
    ok, _, exif = J.extract_exif(pj)
    rc, buf, desc, _ = K.oracle_run(orc, np.ascontiguousarray(planes[:w * h * 3 // 2]), w, h, False, sdr_chain, gamut=gamut)
    if rc != 0:
        return rc, None
    grc, gbuf, gdesc, _ = K.oracle_run(orc, np.ascontiguousarray(gplanes[:gw * gh]), gw, gh, True, gm_chain)
    if grc != 0:
        return grc, None
    ow, oh, mw, mh = desc[0], desc[1], gdesc[0], gdesc[1]
    return 0, J.encode_apix(buf[:ow * oh * 3 // 2].copy(), ow, oh, gamut, gbuf[:mw * mh].copy().reshape(mh, mw), md, QUALITY, exif=exif if ok else None)


def _call(hip, files, sdr_chain, gm_chain, caps=None, probe=(), quality=QUALITY, stream=None):
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    n = len(files)
    keep = [np.frombuffer(f, np.uint8) for f in files]
    jp = (C.c_void_p * n)(*[k.ctypes.data for k in keep])
    jn = (C.c_size_t * n)(*[k.size for k in keep])
    caps = caps or [1 << 18] * n
    bufs = [np.full(max(c, 1) + 32, 0xEE, np.uint8) for c in caps]
    out = (C.c_void_p * n)(*[None if i in probe else b.ctypes.data for i, b in enumerate(bufs)])
    cap = (C.c_size_t * n)(*[0 if i in probe else c for i, c in enumerate(caps)])
    size, status = (C.c_size_t * n)(), (C.c_int * n)(*([99] * n))
    rc = lib.uhdr_hip_jpegr_edit_batch(n, jp, jn, K.effect_array(hip, sdr_chain), len(sdr_chain), K.effect_array(hip, gm_chain), len(gm_chain), None, quality,
                                       out, cap, size, status, stream_ptr())
    return rc, list(status), list(size), bufs


def _chain_pairs(w, h):
    return [([K.rot(90)], [K.rot(90)]),
            ([K.resize(w // 2, h // 2)], [K.resize(w // 8, h // 8)]),
            ([K.crop(8, w - 9, 4, h - 5), K.mirror(1)], [K.crop(2, w // 4 - 3, 1, h // 4 - 2), K.mirror(1)]),
            ([K.resize(40, 24), K.rot(270), K.mirror(0)], [K.resize(40, 24), K.rot(270), K.mirror(0)])]


@pytest.mark.parametrize("size", [(64, 48), (96, 64), (48, 80)])
def test_edited_files_equal_the_oracles_composition(hip, orc, J, inputs, size):
    files = inputs[size]
    for sdr_chain, gm_chain in _chain_pairs(*size):
        rc, st, sizes, bufs = _call(hip, files, sdr_chain, gm_chain)
        assert rc == 0 and st == [0, 0], (size, sdr_chain, st)
        for k, f in enumerate(files):
            est, want = _expected(orc, J, f, sdr_chain, gm_chain)
            assert est == 0
            assert sizes[k] == len(want) and bufs[k][:sizes[k]].tobytes() == want, (size, sdr_chain, k)
            assert (bufs[k][sizes[k]:] == 0xEE).all()
            assert J.decode(want, orc.OUT_HDR_HLG, 3.4028234663852886e38)[0] == 0


def test_failing_files_do_not_disturb_the_others(hip, orc, J, inputs):
    a, b = inputs[(64, 48)]
    c = inputs[(48, 80)][0]
    imgs = J.find_images(a)
    truncated = a[:imgs[0][0] + imgs[0][1] // 2]
    plain = a[imgs[0][0]:imgs[0][0] + imgs[0][1]]
    sdr_chain, gm_chain = [K.mirror(1)], [K.crop(2, 13, 1, 10)]          # the crop fits a 16x12 map, not the 12x20 one of file c
    files = [a, truncated, plain, c, b, a, b]
    want = [_expected(orc, J, f, sdr_chain, gm_chain) for f in files]
    assert [w[0] for w in want] == [0, want[1][0], hip.ERROR_GAIN_MAP_IMAGE_NOT_FOUND, hip.ERROR_INVALID_CROPPING_PARAMETERS, 0, 0, 0]
    assert want[1][0] in (hip.ERROR_NO_IMAGES_FOUND, hip.ERROR_GAIN_MAP_IMAGE_NOT_FOUND, hip.ERROR_DECODE_ERROR)
    caps = [1 << 18] * 7
    caps[5] = len(want[5][1]) - 1                                        # one byte short
    rc, st, sizes, bufs = _call(hip, files, sdr_chain, gm_chain, caps=caps, probe=(6,))
    R = hip.ERROR_INSUFFICIENT_RESOURCE
    assert st == [0, want[1][0], want[2][0], want[3][0], 0, R, R], st
    assert rc == want[1][0]
    for k in (0, 4):
        assert sizes[k] == len(want[k][1]) and bufs[k][:sizes[k]].tobytes() == want[k][1]
    assert sizes[5] == len(want[5][1]) and sizes[6] == len(want[6][1])   # the exact size, also for the probe
    for k in (1, 2, 3, 6):
        assert (bufs[k] == 0xEE).all()
    assert (bufs[5][caps[5]:] == 0xEE).all()


def test_call_level_errors(hip, inputs):
    files = inputs[(64, 48)]
    rc, st, _, _ = _call(hip, files, [K.rot(90)], [K.rot(90)], quality=101)
    assert rc == hip.ERROR_INVALID_QUALITY_FACTOR and st == [99, 99]
    lib = hip.load()
    assert lib.uhdr_hip_jpegr_edit_batch(-1, None, None, None, 0, None, 0, None, 90, None, None, None, None, None) == hip.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpegr_edit_batch(1, None, None, None, 0, None, 0, None, 90, None, None, None, None, None) == hip.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpegr_edit_batch(0, None, None, None, 1, None, 0, None, 90, None, None, None, None, None) == hip.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpegr_edit_batch(0, None, None, None, 0, None, 0, None, 90, None, None, None, None, None) == 0
