"""-m gpu: odd-sized 4:2:0 JPEGs and JPEG/R files through the decode calls, against the oracle (the files
and their expected bytes: tests/odd420_cases.py, held to one answer by tests/test_odd420_cpu.py).

The reference decodes such an image into a zeroed buffer of floor(3 w h / 2) bytes with Cr w h / 4 bytes behind Cb, and applyGainMap
reads Cr chroma_stride (h / 2) behind Cb: shifted, with zeros from the gap in front.  decode_images zeroes the bytes the decoder does not
write, so every pixel of the HDR rendition is the oracle's -- whatever the pool or the caller's buffer held before.  To make that show,
every call on pooled planes is made behind a decode of larger files full of colour (the same process, the same context), every
caller's buffer is prefilled, and the odd files sit between even-sized ones.

Bars: the decoded planes and the EXACT renditions bit for bit, over all bytes and all pixels; FAST through tests/test_gpu_parity.py's
_check_apply."""
import ctypes as C

import numpy as np
import pytest

from tests import odd420_cases as D
from tests.jpeg_scaled_cases import jpegr_file
from tests.test_gpu_jpegr_decode_rounds import ENTRIES, HOOK, TINY, round_bound  # noqa: F401  (round_bound: a fixture)
from tests.test_gpu_parity import _check_apply

pytestmark = pytest.mark.gpu
FLT_MAX = D.FLT_MAX
ONE_PLANE = [n for n in D.FILE_NAMES if not n.startswith("og")]


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class Even:
    """an even-sized file of tests/jpeg_scaled_cases.jpegr_file, shaped like odd420_cases.File"""

    def __init__(self, w, h, factor):
        self.name, self.data, self.w, self.h, self.rgb = "e%dx%d" % (w, h), jpegr_file(w, h, factor), w, h, False


_EVEN_WANT = {}


def _want(f, fmt):
    if not isinstance(f, Even):
        return D.file_expected(f.name, fmt)
    if (f.name, fmt) not in _EVEN_WANT:
        from oracle import jpegr_oracle as J
        st, out, w, h, _, _ = J.decode(f.data, fmt, FLT_MAX, threads=2)
        assert st == 0
        _EVEN_WANT[(f.name, fmt)] = out[:D.BPP[fmt] * w * h].copy()
    return _EVEN_WANT[(f.name, fmt)]


def _between_even_ones(names):
    """the odd files of `names` in a call with even-sized ones in front, between and behind"""
    files = [Even(130, 70, 2)]
    for k, n in enumerate(names):
        files.append(D.files()[n])
        if k % 2 == 1:
            files.append(Even(136, 72, 4))
    return files + [Even(130, 70, 2)]


def _batch(hip, entry, files, fmt, mode, device):
    """one call of a JPEG/R decode batch entry point into prefilled buffers: (rc, statuses, outputs, descriptors)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    n = len(files)
    bufs = [np.frombuffer(f.data, np.uint8) for f in files]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests, mds, stat = (hip.Image * n)(), (hip.Metadata * n)(), _arr(C.c_int, [7] * n)
    needs = [hip.output_bytes(fmt, f.w, f.h) for f in files]
    outs = [dev_empty(k, 0xCD) if device else np.full(k, 0xCD, np.uint8) for k in needs]
    optr = _arr(C.c_void_p, [o.data_ptr() if device else o.ctypes.data for o in outs])
    tail = () if entry == ENTRIES[0] else (hip.DECODE_ANY_SAMPLING,)
    rc = getattr(lib, entry)(n, ptrs, sizes, fmt, FLT_MAX, optr, _arr(C.c_size_t, needs), dests, mds, stat, mode,
                             hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr(), *tail)
    got = [to_host(o, k).copy() if device else o for o, k in zip(outs, needs)]
    return rc, list(stat), got, dests


def _dirty(hip):
    """fills the context's pooled planes with colour: four 264x200 files with maps of their own size, 132 KiB of planes each -- more
    than any call of this module holds, so the slices its files get afterwards lie in bytes this call wrote"""
    files = [Even(264, 200, 1)] * 4
    rc, stat, _, _ = _batch(hip, ENTRIES[0], files, hip.OUTPUT_HDR_HLG, hip.APPLY_FAST, True)
    assert rc == 0 and stat == [0] * 4


def test_the_dirtying_call_covers_every_other_call():
    pooled = lambda f: 2 * (-(-(f.w * f.h * 3 // 2 + 64 + 1) // 256) * 256)      # noqa: E731  (primary and map, each at most this)
    most = sum(pooled(f) for f in _between_even_ones(D.FILE_NAMES))
    assert most < 4 * 264 * 200 * 3 // 2


# ---- 1. the whole decode buffer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("call", ["single", "single_ex", "batch", "batch_ex"])
def test_whole_decode_buffer(hip, orc, call, device):
    """all `need` bytes of every odd file's primary image are orc.jpeg_decode's: the gap between Cb and Cr is zero although the
    destination held 0xCD (a device caller) or the pool held colour (a host caller); nothing is written behind `need`"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    files = [D.files()[n] for n in D.FILE_NAMES]
    wants = []
    for f in files:
        st, planes, w, h, gray = orc.jpeg_decode("orc", f.primary)
        assert st == f.w * f.h + 2 * (f.w * f.h // 4) and np.array_equal(planes, D.primary_buffer(f.name)[:st])
        g0 = w * h + (w // 2) * (h // 2)
        assert not planes[g0:w * h + w * h // 4].any()
        wants.append(planes)
    needs = [p.size for p in wants]
    bufs = [np.frombuffer(f.primary, np.uint8) for f in files]
    outs = [dev_empty(k + 64, 0xCD) if device else np.full(k + 64, 0xCD, np.uint8) for k in needs]
    addr = [o.data_ptr() if device else o.ctypes.data for o in outs]
    space = hip.MEM_DEVICE if device else hip.MEM_HOST
    n = len(files)
    descs = (hip.Image * n)()
    _dirty(hip)
    if call.startswith("batch"):
        ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
        stat = _arr(C.c_int, [7] * n)
        args = (n, ptrs, sizes, hip.DECODE_TO_YCBCR, _arr(C.c_void_p, addr), _arr(C.c_size_t, needs), descs, stat, space, stream_ptr())
        rc = lib.uhdr_hip_jpeg_decode_batch(*args) if call == "batch" else lib.uhdr_hip_jpeg_decode_batch_ex(*args, hip.DECODE_ANY_SAMPLING)
        assert rc == 0 and list(stat) == [0] * n
    else:
        for k in range(n):
            if call == "single":
                rc = lib.uhdr_hip_jpeg_decode(bufs[k].ctypes.data, bufs[k].size, C.c_void_p(addr[k]), needs[k], C.byref(descs[k]), space, stream_ptr())
            else:
                rc = lib.uhdr_hip_jpeg_decode_ex(bufs[k].ctypes.data, bufs[k].size, hip.DECODE_TO_YCBCR, C.c_void_p(addr[k]), needs[k], C.byref(descs[k]), space,
                                                 stream_ptr(), hip.DECODE_ANY_SAMPLING)
            assert rc == 0, (files[k].name, rc)
    for k, f in enumerate(files):
        got = to_host(outs[k]).copy() if device else outs[k]
        assert (descs[k].width, descs[k].height, descs[k].chroma_stride, descs[k].pixelFormat) == (f.w, f.h, f.w // 2, hip.PIX_FMT_YUV420)
        assert np.array_equal(got[:needs[k]], wants[k]), (call, f.name, np.flatnonzero(got[:needs[k]] != wants[k])[:8])
        assert (got[needs[k]:needs[k] + 64] == 0xCD).all(), (call, f.name)


# ---- 2. JPEG/R decode against the oracle ---------------------------------------------------------------------------------------------
def _names(entry):
    # no flag, and the flag alone: one-component maps (a three-component map contributes its luma there: tests/test_gpu_jpeg_sampling.py)
    return ONE_PLANE if entry in ENTRIES[:2] else D.FILE_NAMES


@pytest.mark.parametrize("tiny", [False, True], ids=["one_round", "round_per_file"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("entry", ENTRIES[:4], ids=lambda e: e[len("uhdr_hip_jpegr_decode_"):])
def test_jpegr_batches(hip, round_bound, entry, device, tiny):
    files = _between_even_ones(_names(entry))
    assert isinstance(files[0], Even) and isinstance(files[-1], Even) and sum(not isinstance(f, Even) for f in files) == len(_names(entry))
    for fmt in D.FORMATS:
        for mode in (hip.APPLY_EXACT, hip.APPLY_FAST):
            _dirty(hip)
            if tiny:
                round_bound(TINY)
            rc, stat, got, dests = _batch(hip, entry, files, fmt, mode, device)
            if tiny:
                assert round_bound(0) == TINY      # the bound that call ran under
            assert rc == 0 and stat == [0] * len(files), (entry, fmt, mode, rc, stat)
            for i, f in enumerate(files):
                want = _want(f, fmt)
                assert (dests[i].width, dests[i].height) == (f.w, f.h), f.name
                if mode == hip.APPLY_EXACT:
                    assert np.array_equal(got[i], want), (entry, f.name, fmt, "%d bytes differ, first at %d" % (int((got[i] != want).sum()), int(np.argmax(got[i] != want))))
                else:
                    _check_apply(hip, fmt, got[i], want, f.w, f.h)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_jpegr_single_call(hip, device):
    """uhdr_hip_jpegr_decode, file by file, EXACT, every format"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    for name in ONE_PLANE:
        f = D.files()[name]
        buf = np.frombuffer(f.data, np.uint8)
        for fmt in D.FORMATS:
            k = hip.output_bytes(fmt, f.w, f.h)
            out = dev_empty(k, 0xCD) if device else np.full(k, 0xCD, np.uint8)
            d, md = hip.Image(), hip.Metadata()
            _dirty(hip)
            rc = lib.uhdr_hip_jpegr_decode(buf.ctypes.data, buf.size, fmt, FLT_MAX, C.c_void_p(out.data_ptr() if device else out.ctypes.data), k, C.byref(d),
                                           C.byref(md), hip.APPLY_EXACT, hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
            got = to_host(out, k).copy() if device else out
            want = D.file_expected(name, fmt)
            assert rc == 0 and (d.width, d.height) == (f.w, f.h)
            assert np.array_equal(got, want), (name, fmt, "%d bytes differ, first at %d" % (int((got != want).sum()), int(np.argmax(got != want))))


# ---- 3. the two-call route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_PLANE)
def test_decode_then_apply(hip, name):
    """uhdr_hip_jpeg_decode of the primary image and of the map into device buffers, then uhdr_hip_apply_gainmap on the descriptors it
    returned: oracle/jpegr_oracle.decode's bytes.  The primary's buffer is the `need` bytes the decode call asks for, 0xFF behind them
    -- except where include/uhdr_hip.h says that applyGainMap reads one byte more (w = 2 mod 4 with an odd h: 18x9): there it is
    need + 1 bytes with the last one zero, as in the reference's buffer"""
    from oracle import jpegr_oracle as J
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    f = D.files()[name]
    need, end = f.w * f.h + 2 * (f.w * f.h // 4), f.w * f.h * 3 // 2
    assert (end - need == 1) == (name == "o18")
    primary = dev_empty(end + 64, 0xFF)
    primary[need:end] = 0
    gplane = dev_empty(f.w * f.h + 64, 0xFF)
    pd, gd = hip.Image(), hip.Image()
    pbuf, gbuf = np.frombuffer(f.primary, np.uint8), np.frombuffer(f.gmap, np.uint8)
    assert lib.uhdr_hip_jpeg_decode(pbuf.ctypes.data, pbuf.size, C.c_void_p(primary.data_ptr()), need, C.byref(pd), hip.MEM_DEVICE, stream_ptr()) == 0
    assert lib.uhdr_hip_jpeg_decode(gbuf.ctypes.data, gbuf.size, C.c_void_p(gplane.data_ptr()), f.w * f.h, C.byref(gd), hip.MEM_DEVICE, stream_ptr()) == 0
    assert (gd.width, gd.height, gd.pixelFormat) == (f.w, f.h, hip.PIX_FMT_MONOCHROME) and pd.chroma_data == primary.data_ptr() + f.w * f.h
    assert bool((primary[end:] == 0xFF).all())
    imgs = J.find_images(f.data)
    x = J.metadata_from_xmp(J.app_segment(f.data[imgs[1][0]:imgs[1][0] + imgs[1][1]], 0xE1, J.XMP_NS))
    md = hip.Metadata(x["version"].encode(), float(x["max"]), float(x["min"]), float(x["gamma"]), float(x["off_sdr"]), float(x["off_hdr"]), float(x["capmin"]),
                      float(x["capmax"]))
    pd.colorGamut = J.gamut_from_icc(J.app_segment(f.primary, 0xE2, J.ICC_ID))
    for fmt in D.FORMATS:
        k = hip.output_bytes(fmt, f.w, f.h)
        out = dev_empty(k, 0xCD)
        dest = hip.out_image(out.data_ptr())
        for mode in (hip.APPLY_EXACT, hip.APPLY_FAST):
            rc = lib.uhdr_hip_apply_gainmap(C.byref(pd), C.byref(gd), C.byref(md), fmt, FLT_MAX, C.byref(dest), mode, hip.MEM_DEVICE, stream_ptr())
            assert rc == 0, (name, fmt, mode, rc)
            got, want = to_host(out, k).copy(), D.file_expected(name, fmt)
            if mode == hip.APPLY_EXACT:
                assert np.array_equal(got, want), (name, fmt, int((got != want).sum()))
            else:
                _check_apply(hip, fmt, got, want, f.w, f.h)


# ---- 5. the SDR rendition is still refused -------------------------------------------------------------------------------------------
def test_sdr_rendition_is_refused(hip):
    """libjpeg-turbo's RGBA of an odd-sized 4:2:0 image is outside the conversion kernels: UNSUPPORTED_FEATURE for the odd files, the
    even-sized neighbours are decoded"""
    files = _between_even_ones(ONE_PLANE)
    rc, stat, _, _ = _batch(hip, ENTRIES[0], files, hip.OUTPUT_SDR, hip.APPLY_EXACT, True)
    want = [0 if isinstance(f, Even) else hip.ERROR_UNSUPPORTED_FEATURE for f in files]
    assert stat == want and rc == hip.ERROR_UNSUPPORTED_FEATURE
