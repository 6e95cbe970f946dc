"""-m gpu: scaled JPEG and JPEG/R decode ("Scaled decode") on the device against the restatement of
tests/jpeg_scaled_oracle.py and against Pillow (libjpeg-turbo), which tests/test_jpeg_scaled_cpu.py holds equal.

Every output is carved between guard bytes and placed 0, 1 and 4 bytes behind a 256-byte boundary in turn: whole N-byte stores, byte
stores of an unaligned plane and the clipped stores of edge blocks all run, and the guards must survive.  The IDCT grid: workgroups of
128 blocks per component (of 16 where the component's size is 8); 130x66 4:2:0 has 180 luma blocks -- a second workgroup -- and 45
chroma blocks each, three workgroups of the eight-lane 8x8 at 1/2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import jpeg_scaled_oracle as S
from tests import jpeg_stream_cases as K
from tests.jpeg_scaled_cases import DENOMS, gray_jpeg, pillow_jpeg, pillow_scaled, pillow_scaled_rgba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = 3.4028234663852886e38
GUARD = 512
OFFSETS = (0, 1, 4)
pytestmark = pytest.mark.gpu


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


class _Carved:
    """`need` bytes `off` bytes behind a 256-byte boundary, GUARD bytes of 0xCD on both sides, in device or host memory"""

    def __init__(self, need, off, device):
        from tests.gpu_util import dev_empty
        self.need, self.device = need, device
        total = need + 2 * GUARD + 256 + 8
        if device:
            self.t = dev_empty(total, 0xCD)
            base = self.t.data_ptr()
        else:
            self.t = np.full(total, 0xCD, np.uint8)
            base = self.t.ctypes.data
        self.lo = (-(base + GUARD)) % 256 + GUARD + off
        self.ptr = base + self.lo
        assert (self.ptr - off) % 256 == 0

    def result(self):
        """(the bytes, guards intact)"""
        from tests.gpu_util import to_host
        full = to_host(self.t).copy() if self.device else self.t
        body = full[self.lo:self.lo + self.need]
        rest = np.concatenate([full[:self.lo], full[self.lo + self.need:]])
        return body.copy(), bool((rest == 0xCD).all())


def _need(hip, d, decode_to):
    if decode_to == hip.DECODE_TO_RGBA:
        return d.width * d.height * 4
    if d.pixelFormat == hip.PIX_FMT_MONOCHROME:
        return d.width * d.height
    if d.pixelFormat == hip.PIX_FMT_YUV420:
        return d.width * d.height + 2 * (d.width * d.height // 4)
    cw, ch = hip.chroma_size(d.pixelFormat, d.width, d.height)
    return d.width * d.height + 2 * cw * ch


def _decode_batch(hip, files, decode_to, s, device, off=0, flags=None, ex=False):
    """probe, then one uhdr_hip_jpeg_decode_batch_scaled call (ex: uhdr_hip_jpeg_decode_batch_ex, s ignored):
    (status, statuses, outputs or None, descriptors)"""
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    flags = hip.DECODE_ANY_SAMPLING if flags is None else flags
    n = len(files)
    bufs = [np.frombuffer(f + b"\0" * 8, np.uint8) for f in files]
    jp, js = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [len(f) for f in files])
    descs, stat = (hip.Image * n)(), _arr(C.c_int, [7] * n)

    def call(outs, caps, mem, stream):
        if ex:
            return lib.uhdr_hip_jpeg_decode_batch_ex(n, jp, js, decode_to, outs, caps, descs, stat, mem, stream, flags)
        return lib.uhdr_hip_jpeg_decode_batch_scaled(n, jp, js, decode_to, outs, caps, descs, stat, mem, stream, flags, s)
    call(None, None, hip.MEM_HOST, None)
    probe = list(stat)
    needs = [_need(hip, descs[i], decode_to) if probe[i] == hip.ERROR_INSUFFICIENT_RESOURCE else 64 for i in range(n)]
    outs = [_Carved(k, off, device) for k in needs]
    rc = call(_arr(C.c_void_p, [o.ptr for o in outs]), _arr(C.c_size_t, needs), hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr() if device else None)
    got = []
    for i, o in enumerate(outs):
        body, intact = o.result()
        assert intact, ("guard bytes", i, s, off, device)
        got.append(body if stat[i] == 0 else None)
    return rc, list(stat), got, descs, probe


_FMT_NAME = None


def _check_against_the_restatement(hip, data, flags, device, pillow_mode):
    """planes and RGBA of one baseline file at every denominator and offset"""
    global _FMT_NAME
    _FMT_NAME = _FMT_NAME or {hip.PIX_FMT_MONOCHROME: "MONOCHROME", hip.PIX_FMT_YUV444: "YUV444", hip.PIX_FMT_YUV422: "YUV422", hip.PIX_FMT_YUV440: "YUV440"}
    f = S.read_baseline(data)
    w, h = f["w"], f["h"]
    for k, s in enumerate(DENOMS):
        ow, oh, fmt, pl = S.decode_scaled(data, s)
        want = S.packed(pl)
        for off in OFFSETS:
            rc, stat, got, descs, _ = _decode_batch(hip, [data], hip.DECODE_TO_YCBCR, s, device, off, flags)
            assert rc == 0 and stat == [0], (s, off, stat)
            d = descs[0]
            assert (d.width, d.height, d.luma_stride, _FMT_NAME[d.pixelFormat]) == (ow, oh, ow, fmt)
            assert f["gray"] or (d.chroma_data - d.data == ow * oh and d.chroma_stride == pl[1].shape[1])
            assert np.array_equal(got[0], want), (w, h, s, off, int((got[0] != want).sum()), np.nonzero(got[0] != want)[0][:8])
        if w >= s and h >= s and pillow_mode is not None:   # ... and Pillow's own planes
            raw = pillow_scaled(data, pillow_mode, w, h, s)
            assert np.array_equal(want, raw.reshape(-1) if f["gray"] else np.concatenate([raw[:, :, c].reshape(-1) for c in range(3)]))
        if f["gray"]:
            continue
        off = OFFSETS[k % 3]
        rc, stat, got, descs, _ = _decode_batch(hip, [data], hip.DECODE_TO_RGBA, s, device, off, flags)
        assert rc == 0 and stat == [0] and (descs[0].width, descs[0].height) == (ow, oh)
        want = S.rgba(pl, fmt, fancy=s != 8)
        assert np.array_equal(got[0], want), ("rgba", w, h, s, int((got[0] != want).sum()))
        if w >= s and h >= s:
            assert np.array_equal(want, pillow_scaled_rgba(data, w, h, s))


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("size", [(8, 8), (3, 5)])
def test_gray(hip, size, device):
    """8x8: one block.  3x5: the output at 1/8 is 1 x 1, at 1/4 1 x 2"""
    _check_against_the_restatement(hip, gray_jpeg(size[0], size[1], 31), 0, device, "L")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("size", [(16, 16), (18, 34), (130, 66)])
def test_420(hip, size, device):
    """18x34: dummy blocks and partial MCUs.  130x66: 270 blocks, a second workgroup of the luma range.  Without the any-sampling flag"""
    _check_against_the_restatement(hip, pillow_jpeg(size[0], size[1], 32, subsampling=2, quality=92), 0, device, "YCbCr")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["444", "422", "440"])
def test_other_samplings(hip, kind, device):
    """4:4:4 37x29, 4:2:2 33x17, 4:4:0 17x33 (the 4:2:2 file mirrored at its diagonal) under UHDR_HIP_DECODE_ANY_SAMPLING"""
    data = {"444": lambda: pillow_jpeg(37, 29, 33, subsampling=0), "422": lambda: pillow_jpeg(33, 17, 34, subsampling=1),
            "440": lambda: S.transposed_file(pillow_jpeg(33, 17, 34, subsampling=1))}[kind]()
    assert hip.load() and S.read_baseline(data)["w"] == {"444": 37, "422": 33, "440": 17}[kind]
    _check_against_the_restatement(hip, data, hip.DECODE_ANY_SAMPLING, device, "YCbCr" if kind == "444" else None)
    # without the flag the file is refused as at full size
    rc, stat, _, _, probe = _decode_batch(hip, [data], hip.DECODE_TO_YCBCR, 2, device, 0, 0)
    full = _decode_batch(hip, [data], hip.DECODE_TO_YCBCR, 1, device, 0, 0, ex=True)
    assert probe == full[4] and rc == full[0] and rc != 0


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_progressive_and_restart_interval_files(hip, device):
    """a progressive 4:2:0 file (its coefficients come from the host) against Pillow and against the restatement of its baseline twin,
    a restart-interval file against both"""
    w, h = 50, 38
    prog = pillow_jpeg(w, h, 35, subsampling=2, progressive=True)
    twin = pillow_jpeg(w, h, 35, subsampling=2)
    _check_against_the_restatement(hip, pillow_jpeg(w, h, 36, subsampling=2, restart_marker_rows=1), 0, device, "YCbCr")
    for s in DENOMS:
        ow, oh, fmt, pl = S.decode_scaled(twin, s)
        raw = pillow_scaled(prog, "YCbCr", w, h, s)
        assert np.array_equal(S.packed(pl), np.concatenate([raw[:, :, c].reshape(-1) for c in range(3)]))
        rc, stat, got, descs, _ = _decode_batch(hip, [prog], hip.DECODE_TO_YCBCR, s, device, 1, 0)
        assert rc == 0 and np.array_equal(got[0], S.packed(pl)), s
        rc, stat, got, descs, _ = _decode_batch(hip, [prog], hip.DECODE_TO_RGBA, s, device, 4, 0)
        assert rc == 0 and np.array_equal(got[0], pillow_scaled_rgba(prog, w, h, s)), s


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", ["range_limit_gray", "range_limit_420", "range_limit_wide", "range_limit_max"])
def test_constructed_streams(hip, name, device):
    """both sides of the 64-bit switch of the reduced passes and every range_limit band (tests/test_jpeg_scaled_cpu.py)"""
    data = K.case(name)[0]
    for k, s in enumerate(DENOMS):
        ow, oh, fmt, pl = S.decode_scaled(data, s)
        for off in (OFFSETS[k % 3], OFFSETS[(k + 1) % 3]):
            rc, stat, got, descs, _ = _decode_batch(hip, [data], hip.DECODE_TO_YCBCR, s, device, off, 0)
            assert rc == 0 and (descs[0].width, descs[0].height) == (ow, oh)
            want = S.packed(pl)
            assert np.array_equal(got[0], want), (name, s, off, int((got[0] != want).sum()), np.nonzero(got[0] != want)[0][:8])


def _dims(d):
    return (d.width, d.height, d.luma_stride, d.chroma_stride, d.pixelFormat, d.colorGamut)


def _truncated():
    good = pillow_jpeg(64, 48, 37, subsampling=2)
    return good[:len(good) - 200] + b"\xff\xd9"


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_batch_equals_the_single_calls(hip, device):
    """gray, 4:2:0, 4:4:4 and progressive files in one call, a truncated file between them: every file as its single call, the failing
    one UNKNOWN_ERROR with its buffer untouched"""
    files = [gray_jpeg(50, 34, 38), pillow_jpeg(130, 66, 32, subsampling=2, quality=92), _truncated(), pillow_jpeg(37, 29, 33, subsampling=0),
             pillow_jpeg(50, 38, 35, subsampling=2, progressive=True), gray_jpeg(3, 5, 31)]
    for s in DENOMS:
        for decode_to in (hip.DECODE_TO_YCBCR, hip.DECODE_TO_RGBA):
            rc, stat, got, descs, _ = _decode_batch(hip, files, decode_to, s, device, 1)
            for i, f in enumerate(files):
                r1, s1, g1, d1, _ = _decode_batch(hip, [f], decode_to, s, device, 4)
                assert stat[i] == s1[0], (i, s, stat[i], s1)
                if s1[0] == 0:
                    assert np.array_equal(got[i], g1[0]) and _dims(descs[i]) == _dims(d1[0]), (i, s)
            gray_rc = hip.UNKNOWN_ERROR if decode_to == hip.DECODE_TO_RGBA else 0
            assert stat == [gray_rc, 0, hip.UNKNOWN_ERROR, 0, 0, gray_rc] and rc == (gray_rc or hip.UNKNOWN_ERROR), (s, stat)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_denominator_1_is_the_ex_call(hip, device):
    files = [gray_jpeg(50, 34, 38), pillow_jpeg(64, 48, 32, subsampling=2), _truncated(), pillow_jpeg(37, 29, 33, subsampling=0), b"\xff\xd8\xff\xd9",
             pillow_jpeg(45, 37, 39, subsampling=2)]
    for decode_to in (hip.DECODE_TO_YCBCR, hip.DECODE_TO_RGBA):
        for flags in (0, hip.DECODE_ANY_SAMPLING):
            a = _decode_batch(hip, files, decode_to, 1, device, 0, flags)
            b = _decode_batch(hip, files, decode_to, 1, device, 0, flags, ex=True)
            assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
            for i in range(len(files)):
                assert (a[2][i] is None) == (b[2][i] is None) and (a[2][i] is None or np.array_equal(a[2][i], b[2][i])), i
                assert (a[3][i].width, a[3][i].height, a[3][i].pixelFormat, a[3][i].chroma_stride) == (b[3][i].width, b[3][i].height, b[3][i].pixelFormat,
                                                                                                    b[3][i].chroma_stride)


# ---- JPEG/R ---------------------------------------------------------------------------------------------------------------------------
_FILES = {}


def _jpegr(hip, w, h, factor, rgb_map):
    """a file of the library's own encoder (uhdr_hip_jpegr_encode_scaled_batch), once per process"""
    key = (w, h, factor, rgb_map)
    if key not in _FILES:
        from tests import scaled_cases as SC
        from tests import test_gpu_scaled as GS
        rc, stat, _, files = GS._encode(hip, hip.load().uhdr_hip_jpegr_encode_scaled_batch, [SC.pair(w, h, 700 + w + factor)], False, SC.TF_HLG, 90,
                                        (rgb_map, factor))
        assert rc == 0 and stat == [0]
        _FILES[key] = files[0]
    return _FILES[key]


def _jpegr_batch(hip, files, out_fmt, mode, s, device, off=0):
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests, mds, stat = (hip.Image * n)(), (hip.Metadata * n)(), _arr(C.c_int, [7] * n)

    def call(optr, ocap, mem, stream):
        return lib.uhdr_hip_jpegr_decode_scaled_batch(n, ptrs, sizes, out_fmt, FLT_MAX, optr, ocap, dests, mds, stat, mode, mem, stream, 0, s)
    call(None, None, hip.MEM_HOST, None)
    probe = list(stat)
    needs = [hip.output_bytes(out_fmt, dests[i].width, dests[i].height) if probe[i] == hip.ERROR_INSUFFICIENT_RESOURCE else 64 for i in range(n)]
    outs = [_Carved(k, off, device) for k in needs]
    rc = call(_arr(C.c_void_p, [o.ptr for o in outs]), _arr(C.c_size_t, needs), hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr() if device else None)
    got = []
    for i, o in enumerate(outs):
        body, intact = o.result()
        assert intact, ("guard bytes", i, s, off)
        got.append(body if stat[i] == 0 else None)
    return rc, probe, list(stat), got, dests, mds


def _apply_of_the_pieces(hip, primary, gm_jpeg, md, out_fmt, mode, s, ms, factor, gamut):
    """uhdr_hip_apply_gainmap_md_batch on what uhdr_hip_jpeg_decode_batch_scaled returns for the two JPEGs"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    rc, stat, got, d, _ = _decode_batch(hip, [primary], hip.DECODE_TO_YCBCR, s, True)
    assert rc == 0
    rgb = False
    rcm, statm, gotm, dm, _ = _decode_batch(hip, [gm_jpeg], hip.DECODE_TO_YCBCR, ms, True)
    assert rcm == 0
    if dm[0].pixelFormat != hip.PIX_FMT_MONOCHROME:   # a per-channel map: its RGBA
        rcm, statm, gotm, dm, _ = _decode_batch(hip, [gm_jpeg], hip.DECODE_TO_RGBA, ms, True)
        assert rcm == 0
        rgb = True
    w, h, mw, mh = d[0].width, d[0].height, dm[0].width, dm[0].height
    assert w == mw * factor and h == mh * factor, (w, h, mw, mh, factor)
    dev, dmap = to_dev(got[0]), to_dev(gotm[0])
    img = hip.ycbcr_image(dev.data_ptr(), w, h, gamut, d[0].pixelFormat)
    mimg = hip.rgba_map_image(dmap.data_ptr(), mw, mh) if rgb else hip.mono_image(dmap.data_ptr(), mw, mh)
    nbytes = hip.output_bytes(out_fmt, w, h)
    dout = dev_empty(nbytes, 0xCD)
    dest = hip.out_image(dout.data_ptr())
    assert lib.uhdr_hip_apply_gainmap_md_batch(1, C.byref(img), C.byref(mimg), C.byref(md), out_fmt, FLT_MAX, C.byref(dest), mode, stream_ptr()) == 0
    return to_host(dout, nbytes).copy(), got[0], gotm[0], (w, h, mw, mh)


def _map_denominator(factor, s):
    return (1, factor // s) if factor % s == 0 else (s // factor, 1)


JPEGR_CASES = [(64, 48, 4, 0), (136, 72, 4, 0), (64, 48, 1, 0), (64, 48, 4, 1)]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("case", JPEGR_CASES, ids=lambda c: "%dx%d_f%d_%s" % (c[0], c[1], c[2], "rgb" if c[3] else "mono"))
def test_jpegr_scaled(hip, case, device):
    """SDR: Pillow's scaled RGB of the primary image plus alpha.  Every HDR format, FAST and EXACT: the apply call on the planes the
    scaled JPEG decode returns for the two JPEGs.  At s = 8 a factor-4 file carries two denominators in one launch (primary 1/8, map 1/2)"""
    from tests import test_gpu_rgbmap as G
    w, h, factor, rgb_map = case
    data = _jpegr(hip, w, h, factor, rgb_map)
    primary, gm_jpeg = G._info(hip, data)
    for k, s in enumerate(DENOMS):
        ms, af = _map_denominator(factor, s)
        off = OFFSETS[k % 3]
        rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], hip.OUTPUT_SDR, hip.APPLY_EXACT, s, device, off)
        assert rc == 0 and (dests[0].width, dests[0].height) == (S.ceil_div(w, s), S.ceil_div(h, s))
        assert np.array_equal(got[0], pillow_scaled_rgba(primary, w, h, s)), ("sdr", s)
        formats = (hip.OUTPUT_HDR_LINEAR, hip.OUTPUT_HDR_PQ, hip.OUTPUT_HDR_HLG, hip.OUTPUT_HDR_LINEAR_RGB_10BIT) if (w, device) == (64, True) else (hip.OUTPUT_HDR_PQ,)
        for out_fmt in formats:
            for mode in (hip.APPLY_FAST, hip.APPLY_EXACT):
                rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], out_fmt, mode, s, device, off)
                assert rc == 0 and stat == [0], (s, out_fmt, mode, stat)
                want, _, _, dims = _apply_of_the_pieces(hip, primary, gm_jpeg, mds[0], out_fmt, mode, s, ms, af, dests[0].colorGamut)
                assert (dests[0].width, dests[0].height) == dims[:2]
                assert np.array_equal(got[0], want), (s, out_fmt, mode, int((got[0] != want).sum()))


def test_jpegr_batch_with_a_refused_and_a_failing_file(hip):
    """factor 4 and factor 1 files, a container cut short and a factor-3 file (refused at s = 2) in one call"""
    from tests.jpeg_scaled_cases import jpegr_file
    good = [_jpegr(hip, 64, 48, 4, 0), _jpegr(hip, 64, 48, 1, 0)]
    files = [good[0], jpegr_file(48, 96, 3), good[1], good[0][:300]]
    rc, probe, stat, got, dests, mds = _jpegr_batch(hip, files, hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, 2, True)
    assert stat[0] == 0 and stat[2] == 0 and stat[1] == hip.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR and stat[3] not in (0, hip.ERROR_INSUFFICIENT_RESOURCE)
    assert rc == hip.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR
    for i, k in ((0, 0), (2, 1)):
        alone = _jpegr_batch(hip, [good[k]], hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, 2, True)
        assert np.array_equal(got[i], alone[3][0])
    # scale_denom 1 is uhdr_hip_jpegr_decode_md_batch
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    one = _jpegr_batch(hip, good, hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, 1, True)
    bufs = [np.frombuffer(f, np.uint8) for f in good]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests2, stat2 = (hip.Image * 2)(), _arr(C.c_int, [7, 7])
    outs = [np.full(64 * 48 * 4, 0xCD, np.uint8) for _ in good]
    assert lib.uhdr_hip_jpegr_decode_md_batch(2, ptrs, sizes, hip.OUTPUT_HDR_PQ, FLT_MAX, _arr(C.c_void_p, [o.ctypes.data for o in outs]),
                                              _arr(C.c_size_t, [o.size for o in outs]), dests2, None, stat2, hip.APPLY_EXACT, hip.MEM_HOST, None, 0) == 0
    assert one[0] == 0 and all(np.array_equal(a, b) for a, b in zip(one[3], outs))


def test_jpegr_exact_against_the_oracle_on_pillows_planes(hip, orc):
    """EXACT at s = 2 of the 64x48 factor-4 file: the oracle's applyGainMap over Pillow's scaled planes of the primary image (4:4:4:
    four 4:2:0 images, one per chroma phase, as tests/test_gpu_jpeg_sampling.py builds them) and the oracle's decode of the map"""
    from tests import test_gpu_rgbmap as G
    w, h, s = 64, 48, 2
    data = _jpegr(hip, w, h, 4, 0)
    primary, gm_jpeg = G._info(hip, data)
    ow, oh = w // s, h // s
    ycc = pillow_scaled(primary, "YCbCr", w, h, s)
    st, gplane, gw, gh, ggray = orc.jpeg_decode("orc", gm_jpeg)
    assert st > 0 and (gw, gh) == (w // 4, h // 4)
    gmap = np.ascontiguousarray(gplane[:gw * gh].reshape(gh, gw))
    rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, s, True)
    assert rc == 0
    md = mds[0]
    omd = orc.Metadata(md.maxContentBoost, md.minContentBoost, md.gamma, md.offsetSdr, md.offsetHdr, md.hdrCapacityMin, md.hdrCapacityMax, 1)
    want = np.zeros((oh, ow), np.uint32)
    for dy in range(2):
        for dx in range(2):
            img = np.concatenate([ycc[:, :, 0].reshape(-1), ycc[dy::2, dx::2, 1].reshape(-1), ycc[dy::2, dx::2, 2].reshape(-1)])
            st, out, _ = orc.apply("orc_", orc.yuv420_image(np.ascontiguousarray(img), ow, oh, dests[0].colorGamut), gmap, omd, hip.OUTPUT_HDR_PQ, FLT_MAX, threads=2)
            assert st == 0
            v = out[:ow * oh * 4].view(np.uint32).reshape(oh, ow)
            want[dy::2, dx::2] = v[dy::2, dx::2]
    assert np.array_equal(got[0].view(np.uint32).reshape(oh, ow), want), int((got[0].view(np.uint32).reshape(oh, ow) != want).sum())


def test_the_shims_setter_and_helper(hip, tmp_path):
    """ultrahdr::JpegRHip::setDecodeScaleDenom and JpegDecoderHelperHip::decompressImage(..., scaleDenom)"""
    from tests import test_gpu_rgbmap as G
    exe = str(tmp_path / "shim_decode_scaled_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_decode_scaled_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    data = _jpegr(hip, 64, 48, 4, 0)
    primary, _ = G._info(hip, data)
    src = str(tmp_path / "in.jpg")
    open(src, "wb").write(data)
    outs = [str(tmp_path / n) for n in ("out.rgba", "out.pq", "out.planes")]
    r = subprocess.run([exe, src, "4"] + outs, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(outs[0], np.uint8), pillow_scaled_rgba(primary, 64, 48, 4))
    want = _jpegr_batch(hip, [data], hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, 4, False)[3][0]   # (the shim's default apply mode)
    assert np.array_equal(np.fromfile(outs[1], np.uint8), want)
    assert np.array_equal(np.fromfile(outs[2], np.uint8), S.packed(S.decode_scaled(primary, 4)[3]))
