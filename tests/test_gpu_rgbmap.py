"""-m gpu: per-channel (RGB) gain maps -- generate against the per-channel restatement of the oracle's primitives, apply against the
composite of three single-channel oracle runs, the 4:4:4 JPEG encoder against Pillow's (libjpeg-turbo's) files of tests/golden/rgbmap/,
JPEG/R files with such maps written and read, and the C++ shim's setter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import rgbmap_cases as R
from tests.sampling_cases import JPEGR_MD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = 3.4028234663852886e38
LSB_TOL, HALF_ULP_TOL = 1, 1     # the FAST bar of tests/test_gpu_parity.py
pytestmark = pytest.mark.gpu
HDR_FORMATS = (R.FMT_F16, R.FMT_PQ, R.FMT_HLG, R.FMT_RGB10)


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


# ---- generate ---------------------------------------------------------------------------------------------------------------------
def _dev_pair(hip, yi, pi, arrays):
    """the oracle pair of R.lcg_pair in device memory: (api yuv image, api p010 image, tensors to keep alive)"""
    from tests.gpu_util import to_dev
    w, h = yi.width, yi.height
    if len(arrays) == 2:
        dp, dy = to_dev(arrays[0]), to_dev(arrays[1])
        return hip.yuv420_image(dy.data_ptr(), w, h, yi.colorGamut), hip.p010_image(dp.data_ptr(), w, h, pi.colorGamut), (dp, dy)
    t = [to_dev(a) for a in arrays]   # y, uv, hy, huv with padded rows
    y = hip.yuv420_image(t[0].data_ptr(), w, h, yi.colorGamut, luma_stride=yi.luma_stride, chroma_stride=yi.chroma_stride, chroma_ptr=t[1].data_ptr())
    p = hip.p010_image(t[2].data_ptr(), w, h, pi.colorGamut, luma_stride=pi.luma_stride, chroma_stride=pi.chroma_stride, chroma_ptr=t[3].data_ptr())
    return y, p, t


def _gpu_generate_rgb(hip, pairs, tf, sdr_is_601=False, offset=0):
    """one uhdr_hip_generate_gainmap_rgb_batch call over `pairs` (tuples of R.lcg_pair): (status, [(mh, mw, 4) uint8], metadata, dests);
    offset: bytes the map pointers sit behind an 8-byte boundary (4: the unpaired stores)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    keep, ys, ps, outs = [], [], [], []
    for yi, pi, arrays in pairs:
        y, p, t = _dev_pair(hip, yi, pi, arrays)
        keep.append(t)
        ys.append(y)
        ps.append(p)
        outs.append(dev_empty(4 * (yi.width // 4) * (yi.height // 4) + 16 + offset, 0xCD))
    dests = hip.image_array([hip.out_image(t.data_ptr() + offset) for t in outs])
    md = hip.Metadata()
    rc = lib.uhdr_hip_generate_gainmap_rgb_batch(len(pairs), hip.image_array(ys), hip.image_array(ps), tf, C.byref(md), dests, int(sdr_is_601), stream_ptr())
    maps = []
    for (yi, _, _), t in zip(pairs, outs):
        mw, mh = yi.width // 4, yi.height // 4
        full = to_host(t).copy()
        assert (full[offset + 4 * mw * mh:] == 0xCD).all() and (full[:offset] == 0xCD).all()   # nothing written outside the map
        maps.append(full[offset:offset + 4 * mw * mh].reshape(mh, mw, 4))
    return rc, maps, md, dests


def _check_map(got, want):
    assert (got[:, :, 3] == 0xFF).all()
    assert np.array_equal(got[:, :, :3], want), int((got[:, :, :3] != want).sum())


GEN_SMALL = [
    # (w, h, sdr gamut, hdr gamut, pad, map offset): the smallest map; an odd map width with an unpaired last pixel; strided planes on
    # the aligned path (rows 8 longer) and on the ragged one (rows 6 longer)
    (4, 4, R.CG_709, R.CG_2100, 0, 0),
    (20, 12, R.CG_P3, R.CG_P3, 0, 4),
    (72, 40, R.CG_2100, R.CG_709, 8, 0),
    (72, 40, R.CG_709, R.CG_2100, 6, 4),
]


@pytest.mark.parametrize("tf", [R.TF_HLG, R.TF_PQ, R.TF_LINEAR])
@pytest.mark.parametrize("case", GEN_SMALL, ids=lambda c: "%dx%d_%d%d_pad%d" % c[:5])
def test_generate_small_maps(hip, orc, case, tf):
    w, h, sg, hg, pad, off = case
    pair = R.lcg_pair(orc, w, h, 300 + w + tf, sg, hg, pad)
    rc, maps, md, dests = _gpu_generate_rgb(hip, [pair], tf, offset=off)
    assert rc == 0
    _check_map(maps[0], R.channel_bytes(orc, pair[0], pair[1], tf))
    d = dests[0]
    assert (d.width, d.height, d.luma_stride, d.chroma_data, d.pixelFormat) == (w // 4, h // 4, w // 4, None, hip.PIX_FMT_RGBA8888)
    # the metadata is the single-channel call's
    st, _, omd = orc.generate("orc_", pair[0], pair[1], tf)
    assert st == 0 and (md.version, md.maxContentBoost, md.minContentBoost, md.gamma, md.offsetSdr, md.offsetHdr, md.hdrCapacityMin, md.hdrCapacityMax) == \
        (b"1.0", omd.maxContentBoost, omd.minContentBoost, omd.gamma, omd.offsetSdr, omd.offsetHdr, omd.hdrCapacityMin, omd.hdrCapacityMax)


def test_generate_with_the_601_matrix(hip, orc):
    pair = R.lcg_pair(orc, 20, 12, 41, R.CG_709, R.CG_2100)
    rc, maps, _, _ = _gpu_generate_rgb(hip, [pair], R.TF_HLG, sdr_is_601=True)
    want = R.channel_bytes(orc, pair[0], pair[1], R.TF_HLG, sdr_is_601=True)
    assert rc == 0 and not np.array_equal(want, R.channel_bytes(orc, pair[0], pair[1], R.TF_HLG))
    _check_map(maps[0], want)


@pytest.fixture(scope="module")
def big_pair(orc):
    """1056x800 -> a 264x200 map: more than one block per image and more than one tile per block; expected values computed once"""
    pair = R.lcg_pair(orc, 1056, 800, 4242, R.CG_709, R.CG_2100)
    want = R.channel_bytes(orc, pair[0], pair[1], R.TF_HLG)
    want.setflags(write=False)
    return pair, want


def test_generate_large_map(hip, big_pair):
    pair, want = big_pair
    for off in (0, 4):   # the 8-byte pair stores, and the ragged kernel on the same image
        rc, maps, _, _ = _gpu_generate_rgb(hip, [pair], R.TF_HLG, offset=off)
        assert rc == 0
        _check_map(maps[0], want)
    assert len({tuple(p) for p in want.reshape(-1, 3)[:2000]}) > 100 and (want[:, :, 0] != want[:, :, 1]).mean() > 0.5   # the planes differ


def test_generate_batch_of_two_sizes(hip, orc):
    a = R.lcg_pair(orc, 72, 40, 51, R.CG_709, R.CG_2100)
    b = R.lcg_pair(orc, 20, 12, 52, R.CG_709, R.CG_2100)
    c = R.lcg_pair(orc, 72, 40, 53, R.CG_709, R.CG_2100)
    rc, maps, _, _ = _gpu_generate_rgb(hip, [a, b, c], R.TF_PQ)
    assert rc == 0
    for pair, got in zip((a, b, c), maps):
        _check_map(got, R.channel_bytes(orc, pair[0], pair[1], R.TF_PQ))


# ---- apply ------------------------------------------------------------------------------------------------------------------------
def _gpu_apply_rgb(hip, img, rgba, md, fmt, boost, mode, stride=None):
    """img: api image over device planes; rgba: (mh, mw, 4) uint8 -> (status, output bytes)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    mh, mw = rgba.shape[:2]
    st = mw if stride is None else stride
    padded = np.full((mh, st, 4), 0x5A, np.uint8)
    padded[:, :mw] = rgba
    dmap = to_dev(padded)
    nbytes = hip.output_bytes(fmt, img.width, img.height)
    dout = dev_empty(nbytes + 16, 0xCD)
    mimg, dest = hip.rgba_map_image(dmap.data_ptr(), mw, mh, stride), hip.out_image(dout.data_ptr())
    rc = lib.uhdr_hip_apply_gainmap_rgb_batch(1, C.byref(img), C.byref(mimg), C.byref(md), fmt, boost, C.byref(dest), mode, stream_ptr())
    full = to_host(dout).copy()
    assert (full[nbytes:] == 0xCD).all()
    return rc, full[:nbytes]


def _check_fast(fmt, fast, ref, wrap, what):
    from tests.gpu_util import diff_1010102, half_ulp_diff
    if fmt == R.FMT_F16:
        worst, frac = half_ulp_diff(fast.view(np.uint16), ref.view(np.uint16))
        assert worst <= HALF_ULP_TOL, (what, worst)
    elif fmt == R.FMT_RGB10:
        d = np.abs(fast.view(np.uint16).astype(np.int32) - ref.view(np.uint16).astype(np.int32))
        if wrap:
            d = np.minimum(d, 1024 - d)
        worst, frac = int(d.max()), float((d != 0).mean())
        assert worst <= LSB_TOL, (what, worst)
    else:
        worst, frac, alpha_ok = diff_1010102(fast.view(np.uint32), ref.view(np.uint32), wrap)
        assert alpha_ok and worst <= LSB_TOL, (what, worst)
    print("%s FAST: worst=%d, differing fraction=%.5f" % (what, worst, frac))


APPLY_CASES = [
    # (w, h, map w, map h, map stride or None)
    (8, 8, 2, 2, None),        # scale 4
    (20, 12, 5, 3, None),      # scale 4, odd map
    (24, 10, 24, 10, None),    # scale 1
    (12, 20, 6, 10, None),     # scale 2
    (30, 18, 10, 6, None),     # scale 3
    # width 300 at scale 4: two column blocks of 256 and a ragged tail of 44.  (Asked for at height 6, which has no scale-4 map -- 1.5
    # rows; applyGainMap's checks refuse it, see the test below.  8 is the smallest height above it that has one.)
    (300, 8, 75, 2, None),
    (20, 12, 5, 3, 8),         # a map luma_stride of width + 3
    # k_apply_px_rgb's taps and weight tables off the factors above: an odd factor on another shape, a larger power of two, the first
    # factor whose table lives for the call only (uhdr_capi.hip: kIdwCacheMaxScale = 128), and maps one pixel wide / one pixel high
    # (no right tap / no bottom tap for every pixel)
    (42, 30, 14, 10, None),    # scale 3
    (96, 48, 6, 3, None),      # scale 16
    (258, 258, 2, 2, None),    # scale 129
    (2, 40, 1, 20, None),      # scale 2, a 1 x 20 map
    (48, 2, 24, 1, None),      # scale 2, a 24 x 1 map
]


@pytest.mark.parametrize("boost", [FLT_MAX, 2.0])
@pytest.mark.parametrize("case", APPLY_CASES, ids=lambda c: "%dx%d_map%dx%d_%s" % c)
def test_apply_against_the_composite(hip, orc, case, boost):
    from tests.gpu_util import to_dev
    w, h, mw, mh, stride = case
    _, yuv = orc.lcg_frame(w, h, 700 + w)
    rng = np.random.default_rng(w * 100 + h)
    rgba = rng.integers(0, 256, (mh, mw, 4)).astype(np.uint8)
    md, omd = hip.metadata(4.0), R.orc_metadata(orc, 4.0)
    oyi = orc.yuv420_image(yuv, w, h, orc.CG_BT709)
    dyuv = to_dev(yuv)
    img = hip.yuv420_image(dyuv.data_ptr(), w, h, hip.CG_BT709)
    for fmt in HDR_FORMATS:
        want = R.composite_apply(orc, oyi, rgba, omd, fmt, boost)
        rc, exact = _gpu_apply_rgb(hip, img, rgba, md, fmt, boost, hip.APPLY_EXACT, stride)
        assert rc == 0 and np.array_equal(exact, want), (fmt, int((exact != want).sum()))
        rc, fast = _gpu_apply_rgb(hip, img, rgba, md, fmt, boost, hip.APPLY_FAST, stride)
        assert rc == 0
        _check_fast(fmt, fast, want, boost < 4.0, "apply-rgb %dx%d fmt %d boost %g" % (w, h, fmt, min(boost, 4.0)))


def test_apply_issue_case_300x6_is_refused_like_the_single_channel_call(hip, orc):
    """300 x 6 at scale 4 has no integer map height: both calls answer UNSUPPORTED_MAP_SCALE_FACTOR before the device is touched"""
    lib = hip.load()
    buf = np.zeros(4096, np.uint8)
    y = hip.yuv420_image(buf.ctypes.data, 300, 6, hip.CG_BT709)
    md, dest = hip.metadata(4.0), hip.out_image(buf.ctypes.data)
    for mh in (1, 2):
        m = hip.rgba_map_image(buf.ctypes.data, 75, mh)
        assert lib.uhdr_hip_apply_gainmap_rgb_batch(1, C.byref(y), C.byref(m), C.byref(md), R.FMT_HLG, FLT_MAX, C.byref(dest), hip.APPLY_FAST,
                                                    None) == hip.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR
        assert lib.uhdr_hip_apply_gainmap_batch(1, C.byref(y), C.byref(m), C.byref(md), R.FMT_HLG, FLT_MAX, C.byref(dest), hip.APPLY_FAST,
                                                None) == hip.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR


def test_apply_yuv444_primary(hip, orc):
    """a 4:4:4 primary whose chroma planes repeat every 4:2:0 sample 2 x 2: each pixel reads the sample the 4:2:0 image gives it, so the
    composite over the 4:2:0 image is the expected rendition"""
    from tests.gpu_util import to_dev
    w, h, mw, mh = 24, 16, 6, 4
    _, yuv = orc.lcg_frame(w, h, 808)
    y = yuv[:w * h]
    cb, cr = (yuv[w * h + k * (w * h // 4):w * h + (k + 1) * (w * h // 4)].reshape(h // 2, w // 2) for k in range(2))
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1).reshape(-1)
    planes = np.concatenate([y, up(cb), up(cr)])
    rgba = np.random.default_rng(9).integers(0, 256, (mh, mw, 4)).astype(np.uint8)
    md, omd = hip.metadata(4.0), R.orc_metadata(orc, 4.0)
    dev = to_dev(planes)
    img = hip.ycbcr_image(dev.data_ptr(), w, h, hip.CG_BT709, hip.PIX_FMT_YUV444)
    for fmt in HDR_FORMATS:
        want = R.composite_apply(orc, orc.yuv420_image(yuv, w, h, orc.CG_BT709), rgba, omd, fmt, FLT_MAX)
        rc, exact = _gpu_apply_rgb(hip, img, rgba, md, fmt, FLT_MAX, hip.APPLY_EXACT)
        assert rc == 0 and np.array_equal(exact, want), fmt
        rc, fast = _gpu_apply_rgb(hip, img, rgba, md, fmt, FLT_MAX, hip.APPLY_FAST)
        assert rc == 0
        _check_fast(fmt, fast, want, False, "apply-rgb 4:4:4 primary fmt %d" % fmt)


@pytest.mark.parametrize("size", [(20, 12, 5, 3), (64, 32, 16, 8), (30, 18, 10, 6)])
def test_apply_with_three_equal_planes_is_the_single_channel_call(hip, orc, size):
    from tests.gpu_util import gpu_apply, to_dev
    lib = hip.load()
    w, h, mw, mh = size
    _, yuv = orc.lcg_frame(w, h, 900 + w)
    plane = np.random.default_rng(w).integers(0, 256, (mh, mw)).astype(np.uint8)
    rgba = np.stack([plane, plane, plane, 255 - plane], axis=2)
    md = hip.metadata(4.0)
    dyuv, dplane = to_dev(yuv), to_dev(plane)
    img = hip.yuv420_image(dyuv.data_ptr(), w, h, hip.CG_BT709)
    for fmt in HDR_FORMATS:
        for boost in (FLT_MAX, 2.0):
            st, want, _ = gpu_apply(lib, img, dplane, mw, mh, md, fmt, boost, hip.APPLY_EXACT)
            rc, got = _gpu_apply_rgb(hip, img, rgba, md, fmt, boost, hip.APPLY_EXACT)
            assert st == 0 and rc == 0 and np.array_equal(got, want), (fmt, boost)


def test_apply_batch_mixes_sizes_and_strides(hip, orc):
    """one call over three images (two sizes, one strided map) equals the single calls"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    md = hip.metadata(4.0)
    keep, imgs, maps, singles = [], [], [], []
    for k, (w, h, mw, mh, stride) in enumerate(((20, 12, 5, 3, None), (20, 12, 5, 3, 8), (24, 10, 24, 10, None))):
        _, yuv = orc.lcg_frame(w, h, 950 + k)
        rgba = np.random.default_rng(k).integers(0, 256, (mh, mw, 4)).astype(np.uint8)
        padded = np.zeros((mh, stride or mw, 4), np.uint8)
        padded[:, :mw] = rgba
        dy, dm = to_dev(yuv), to_dev(padded)
        keep += [dy, dm]
        imgs.append(hip.yuv420_image(dy.data_ptr(), w, h, hip.CG_BT709))
        maps.append(hip.rgba_map_image(dm.data_ptr(), mw, mh, stride))
        singles.append(_gpu_apply_rgb(hip, imgs[-1], rgba, md, R.FMT_PQ, FLT_MAX, hip.APPLY_EXACT, stride)[1])
    outs = [dev_empty(s.size, 0xCD) for s in singles]
    dests = hip.image_array([hip.out_image(t.data_ptr()) for t in outs])
    rc = lib.uhdr_hip_apply_gainmap_rgb_batch(3, hip.image_array(imgs), hip.image_array(maps), C.byref(md), R.FMT_PQ, FLT_MAX, dests, hip.APPLY_EXACT,
                                              stream_ptr())
    assert rc == 0
    for t, want in zip(outs, singles):
        assert np.array_equal(to_host(t, want.size), want)
    assert (dests[2].width, dests[2].height) == (24, 10)


# ---- the 4:4:4 encoder --------------------------------------------------------------------------------------------------------------
def _rgba_of(rgb, seed):
    h, w = rgb.shape[:2]
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 1)).astype(np.uint8)   # alpha is ignored
    return np.ascontiguousarray(np.concatenate([rgb, a], axis=2))


def _encode_rgb(hip, images, qualities, device, caps=None, strides=None):
    """one uhdr_hip_jpeg_encode_rgb_batch call: (status, statuses, sizes, files)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    n = len(images)
    caps = [im.shape[0] * im.shape[1] * 4 + 4096 for im in images] if caps is None else caps
    keep, descs = [], []
    for k, im in enumerate(images):
        h, w = im.shape[:2]
        st = w if strides is None else strides[k]
        src = np.full((h, st, 4), 0x77, np.uint8)
        src[:, :w] = im
        if device:
            t = to_dev(src)
            keep.append(t)
            descs.append(hip.rgba_map_image(t.data_ptr(), w, h, st))
        else:
            keep.append(src)
            descs.append(hip.rgba_map_image(src.ctypes.data, w, h, st))
    if device:
        outs = [dev_empty(c + 16, 0xCD) for c in caps]
        optr = _arr(C.c_void_p, [t.data_ptr() if c else None for t, c in zip(outs, caps)])
    else:
        outs = [np.full(c + 16, 0xCD, np.uint8) for c in caps]
        optr = _arr(C.c_void_p, [a.ctypes.data if c else None for a, c in zip(outs, caps)])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpeg_encode_rgb_batch(n, hip.image_array(descs), _arr(C.c_int, qualities), optr, _arr(C.c_size_t, caps), sizes, stat,
                                            hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
    files = []
    for k in range(n):
        full = to_host(outs[k]).copy() if device else outs[k]
        if stat[k] == 0:
            assert (full[sizes[k]:] == 0xCD).all()
        files.append(full[:sizes[k]].tobytes() if stat[k] == 0 else None)
    return rc, list(stat), list(sizes), files


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("q", R.QUALITIES)
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_encode_rgb_writes_pillows_file(hip, size, q, device):
    w, h = size
    rc, stat, sizes, files = _encode_rgb(hip, [_rgba_of(R.golden_rgb(w, h), w)], [q], device)
    want = R.golden_jpeg(w, h, q)
    assert rc == 0 and stat == [0] and sizes == [len(want)]
    assert files[0] == want, "first difference at byte %d of %d" % (next(i for i in range(len(want)) if files[0][i] != want[i]), len(want))


@pytest.mark.parametrize("device", [True, False])
def test_encode_rgb_batch_of_all_sizes_and_size_probe(hip, device):
    images = [_rgba_of(R.golden_rgb(w, h), 3 * w) for w, h in R.SIZES]
    want = [R.golden_jpeg(w, h, 85) for w, h in R.SIZES]
    # rows 5 pixels longer than the image: the stride is honoured
    rc, stat, sizes, files = _encode_rgb(hip, images, [85] * 5, device, strides=[im.shape[1] + 5 for im in images])
    assert rc == 0 and stat == [0] * 5 and files == want
    # mixed qualities in one call, and the probe: no buffer / one byte short -> INSUFFICIENT_RESOURCE with the exact size, the others unharmed
    want = [R.golden_jpeg(w, h, q) for (w, h), q in zip(R.SIZES, (85, 95, 85, 95, 95))]
    caps = [len(f) + 64 for f in want]
    caps[1], caps[3] = 0, len(want[3]) - 1
    rc, stat, sizes, files = _encode_rgb(hip, images, [85, 95, 85, 95, 95], device, caps=caps)
    ir = hip.ERROR_INSUFFICIENT_RESOURCE
    assert rc == ir and stat == [0, ir, 0, ir, 0] and sizes == [len(f) for f in want]
    assert [files[k] for k in (0, 2, 4)] == [want[k] for k in (0, 2, 4)]


def test_the_planar_encode_calls_do_not_read_the_new_pixel_format(hip, orc):
    """uhdr_hip_jpeg_encode[_batch] never looked at pixelFormat beyond MONOCHROME: a planar descriptor that says RGBA8888 is still
    compressed as the 4:2:0 image its planes are"""
    lib = hip.load()
    w, h = 40, 24
    _, yuv = orc.lcg_frame(w, h, 5)
    want = orc.jpeg_encode("orc", yuv[:w * h], yuv[w * h:], w, h, 90)
    img = hip.yuv420_image(yuv.ctypes.data, w, h, hip.CG_BT709)
    img.pixelFormat = hip.PIX_FMT_RGBA8888
    out, n = np.zeros(w * h * 3 + 4096, np.uint8), C.c_size_t()
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), 90, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(n), hip.MEM_HOST, None) == 0
    assert out[:n.value].tobytes() == want
    out2, sizes, stat = np.zeros(out.size, np.uint8), _arr(C.c_size_t, [0]), _arr(C.c_int, [7])
    rc = lib.uhdr_hip_jpeg_encode_batch(1, C.byref(img), _arr(C.c_int, [90]), None, None, _arr(C.c_void_p, [out2.ctypes.data]), _arr(C.c_size_t, [out2.size]),
                                        sizes, stat, hip.MEM_HOST, None)
    assert rc == 0 and list(stat) == [0] and out2[:sizes[0]].tobytes() == want


# ---- JPEG/R files -------------------------------------------------------------------------------------------------------------------
def _info(hip, data):
    lib = hip.load()
    buf = np.frombuffer(data, np.uint8)
    a, g = hip.JpegInfo(), hip.JpegInfo()
    assert lib.uhdr_hip_jpegr_info(buf.ctypes.data, buf.size, C.byref(a), C.byref(g)) == 0
    return data[a.offset:a.offset + a.size], data[g.offset:g.offset + g.size]


def _metadata_of(hip, data):
    buf = np.frombuffer(data, np.uint8)
    md = hip.Metadata()
    assert hip.load().uhdr_hip_jpegr_metadata(buf.ctypes.data, buf.size, C.byref(md)) == 0
    return (md.version, md.maxContentBoost, md.minContentBoost, md.gamma, md.offsetSdr, md.offsetHdr, md.hdrCapacityMin, md.hdrCapacityMax)


def _jpegr_encode(hip, fn, pairs, api0, tf, q, exifs, device):
    """pairs: R.lcg_pair tuples (packed) -> (status, statuses, files) of one call of `fn` (either JPEG/R batch encoder)"""
    from tests.gpu_util import stream_ptr
    n = len(pairs)
    keep, ys, ps = [], [], []
    for yi, pi, arrays in pairs:
        if device:
            y, p, t = _dev_pair(hip, yi, pi, arrays)
            keep.append(t)
        else:
            y = hip.yuv420_image(arrays[1].ctypes.data, yi.width, yi.height, yi.colorGamut)
            p = hip.p010_image(arrays[0].ctypes.data, pi.width, pi.height, pi.colorGamut)
        ys.append(y)
        ps.append(p)
    caps = [yi.width * yi.height * 6 + 65536 for yi, _, _ in pairs]
    outs = [np.zeros(c, np.uint8) for c in caps]
    ex = exn = None
    if exifs is not None:
        eb = [np.frombuffer(e, np.uint8) if e else None for e in exifs]
        keep.append(eb)
        ex, exn = _arr(C.c_void_p, [e.ctypes.data if e is not None else None for e in eb]), _arr(C.c_size_t, [len(e) if e else 0 for e in exifs])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = fn(n, hip.image_array(ps), None if api0 else hip.image_array(ys), tf, q, ex, exn, _arr(C.c_void_p, [o.ctypes.data for o in outs]),
            _arr(C.c_size_t, caps), sizes, stat, hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
    return rc, list(stat), [outs[k][:sizes[k]].tobytes() for k in range(n)]


EXIF = b"Exif\0\0MM\0*\0\0\0\x08\0\0"


@pytest.mark.parametrize("api0", [False, True])
@pytest.mark.parametrize("tf", [R.TF_HLG, R.TF_PQ])
def test_jpegr_encode_rgbmap(hip, orc, tf, api0):
    """the new call and uhdr_hip_jpegr_encode_batch on the same pairs: the same primary image and metadata, and the gain-map JPEG is the
    stand-alone 4:4:4 encode at quality 85 of the map uhdr_hip_generate_gainmap_rgb_batch returns"""
    lib = hip.load()
    pairs = [R.lcg_pair(orc, 72, 40, 61, R.CG_709, R.CG_2100), R.lcg_pair(orc, 264, 136, 62, R.CG_P3, R.CG_2100), R.lcg_pair(orc, 72, 40, 63, R.CG_709, R.CG_2100)]
    exifs = [None, EXIF, EXIF]
    rc, stat, new = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_rgbmap_batch, pairs, api0, tf, 90, exifs, True)
    assert rc == 0 and stat == [0, 0, 0]
    rc, stat, old = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_batch, pairs, api0, tf, 90, exifs, True)
    assert rc == 0 and stat == [0, 0, 0]
    rc, stat, host = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_rgbmap_batch, pairs, api0, tf, 90, exifs, False)
    assert rc == 0 and host == new                      # planes in host memory: the same files
    for k, pair in enumerate(pairs):
        (np_, ng), (op, og) = _info(hip, new[k]), _info(hip, old[k])
        assert R.from_first_dqt(np_) == R.from_first_dqt(op)
        assert _metadata_of(hip, new[k]) == _metadata_of(hip, old[k])
        assert (EXIF in new[k]) == (exifs[k] is not None)
        if api0:   # the SDR planes API-0 derives: toneMap of the P010 image (the oracle's), in the P010 image's gamut
            p010 = pair[2][0]
            w, h, gamut = pair[1].width, pair[1].height, pair[1].colorGamut
            yuv = np.zeros(w * h * 3 // 2, np.uint8)
            src, dst = orc.p010_image(p010, w, h, gamut), orc.yuv420_image(yuv, w, h, gamut)
            assert orc.load().orc_toneMap(C.byref(src), C.byref(dst)) == 0
            pair = (dst, src, (p010, yuv))
        rc, maps, _, _ = _gpu_generate_rgb(hip, [pair], tf)
        assert rc == 0
        rc, stat, _, files = _encode_rgb(hip, [maps[0]], [85], True)
        assert rc == 0 and R.from_first_dqt(ng) == R.from_first_dqt(files[0]), k
        assert R.from_first_dqt(ng) != R.from_first_dqt(og)


def _jpegr_decode(hip, fn, files, out_fmt, mode, device, flags=0, boost=FLT_MAX):
    """probe, then decode, through `fn` (uhdr_hip_jpegr_decode_rgbmap_batch or _decode_batch_ex): (status, statuses, outputs, dests, mds)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests, mds, stat = (hip.Image * n)(), (hip.Metadata * n)(), _arr(C.c_int, [7] * n)
    fn(n, ptrs, sizes, out_fmt, boost, None, None, dests, mds, stat, mode, hip.MEM_HOST, stream_ptr(), flags)
    needs = [hip.output_bytes(out_fmt, dests[i].width, dests[i].height) if stat[i] == hip.ERROR_INSUFFICIENT_RESOURCE else 16 for i in range(n)]
    if device:
        outs = [dev_empty(k, 0xCD) for k in needs]
        optr = _arr(C.c_void_p, [t.data_ptr() for t in outs])
    else:
        outs = [np.full(k, 0xCD, np.uint8) for k in needs]
        optr = _arr(C.c_void_p, [a.ctypes.data for a in outs])
    rc = fn(n, ptrs, sizes, out_fmt, boost, optr, _arr(C.c_size_t, needs), dests, mds, stat, mode, hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr(), flags)
    got = [to_host(t, k).copy() for t, k in zip(outs, needs)] if device else outs
    return rc, list(stat), got, dests, mds


def _jpeg_decode(hip, data, decode_to, flags):
    """uhdr_hip_jpeg_decode_ex into device memory: (status, bytes, descriptor)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    d = hip.Image()
    rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, None, 0, C.byref(d), hip.MEM_HOST, None, flags)
    if rc != hip.ERROR_INSUFFICIENT_RESOURCE:
        return rc, None, d
    need = d.width * d.height * 4 if decode_to == hip.DECODE_TO_RGBA else d.width * d.height * 3 // 2
    t = dev_empty(need, 0xCD)
    rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, C.c_void_p(t.data_ptr()), need, C.byref(d), hip.MEM_DEVICE, stream_ptr(), flags)
    return rc, (to_host(t, need).copy() if rc == 0 else None), d


def _primary_jpeg(hip, orc, w, h, seed):
    """an LCG frame through the existing encoder: a 4:2:0 primary image"""
    lib = hip.load()
    _, yuv = orc.lcg_frame(w, h, seed)
    out, n = np.zeros(w * h * 3 + 4096, np.uint8), C.c_size_t()
    img = hip.yuv420_image(yuv.ctypes.data, w, h, hip.CG_BT709)
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), 90, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(n), hip.MEM_HOST, None) == 0
    return out[:n.value].tobytes()


def _apply_of_the_pieces(hip, primary, gm_jpeg, md, out_fmt, mode, boost=FLT_MAX):
    """uhdr_hip_apply_gainmap_rgb_batch on the primary's planes (uhdr_hip_jpeg_decode) and the map's RGBA (the existing RGBA decode)"""
    from tests.gpu_util import to_dev
    rc1, planes, d = _jpeg_decode(hip, primary, hip.DECODE_TO_YCBCR, 0)
    rc2, rgba, gd = _jpeg_decode(hip, gm_jpeg, hip.DECODE_TO_RGBA, hip.DECODE_ANY_SAMPLING)
    assert rc1 == 0 and rc2 == 0, (rc1, rc2)
    dev = to_dev(planes)
    img = hip.yuv420_image(dev.data_ptr(), d.width, d.height, hip.CG_UNSPECIFIED)
    rc, out = _gpu_apply_rgb(hip, img, rgba.reshape(gd.height, gd.width, 4), md, out_fmt, boost, mode)
    assert rc == 0
    return out


def _container(primary, gm_jpeg):
    from oracle import jpegr_oracle as J
    data = J.append_gainmap(primary, gm_jpeg, JPEGR_MD)
    assert isinstance(data, bytes)
    return data


# (map size, scale of the primary): every three-component golden that has an RGBA rendition; the largest at scale 2 to stay quick
DECODE_MAPS = [((1, 1), 4), ((8, 8), 4), ((17, 9), 4), ((45, 37), 4), ((264, 200), 2)]


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("mapcase", DECODE_MAPS, ids=lambda c: "%dx%d" % c[0])
def test_jpegr_decode_rgbmap_of_the_goldens(hip, orc, mapcase, device):
    lib = hip.load()
    (mw, mh), scale = mapcase
    primary = _primary_jpeg(hip, orc, mw * scale, mh * scale, 70 + mw)
    maps = [R.golden_jpeg(mw, mh, 85), R.golden_jpeg(mw, mh, 95)]
    if (mw, mh) == (264, 200):
        maps.append(R.golden_jpeg_420(mw, mh))          # 4:2:0, even sizes: the RGBA decode has a rendition of it
    files = [_container(primary, g) for g in maps]
    for out_fmt, modes in ((R.FMT_HLG, (hip.APPLY_EXACT, hip.APPLY_FAST)), (R.FMT_F16, (hip.APPLY_EXACT,)), (R.FMT_RGB10, (hip.APPLY_FAST,))):
        for mode in modes:
            rc, stat, got, dests, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, out_fmt, mode, device)
            assert rc == 0 and stat == [0] * len(files), (out_fmt, mode, stat)
            for k, g in enumerate(maps):
                assert (dests[k].width, dests[k].height) == (mw * scale, mh * scale) and abs(mds[k].maxContentBoost - 10.0) < 1e-3   # (the XMP carries log2 of the boost with six digits)
                want = _apply_of_the_pieces(hip, primary, g, mds[k], out_fmt, mode)
                if mode == hip.APPLY_EXACT:
                    assert np.array_equal(got[k], want), (out_fmt, k, int((got[k] != want).sum()))
                else:    # the same kernel on the same inputs: inside the FAST bar with room to spare
                    _check_fast(out_fmt, got[k], want, False, "decode-rgbmap %dx%d file %d fmt %d" % (mw, mh, k, out_fmt))


def test_jpegr_decode_rgbmap_odd_420_map_is_refused_like_its_rgba_decode(hip, orc):
    """the 45x37 4:2:0 golden: libjpeg-turbo's RGBA of an odd-sized 4:2:0 file is outside uhdr_hip_jpeg_decode_rgba
    (ERROR_UNSUPPORTED_FEATURE), so there is no RGBA to apply: the file gets that status and its neighbour in the batch is unharmed"""
    lib = hip.load()
    g = R.golden_jpeg_420(45, 37)
    assert _jpeg_decode(hip, g, hip.DECODE_TO_RGBA, hip.DECODE_ANY_SAMPLING)[0] == hip.ERROR_UNSUPPORTED_FEATURE
    primary = _primary_jpeg(hip, orc, 180, 148, 115)
    files = [_container(primary, g), _container(primary, R.golden_jpeg(45, 37, 85))]
    rc, stat, got, dests, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, R.FMT_HLG, hip.APPLY_EXACT, True)
    assert rc == hip.ERROR_UNSUPPORTED_FEATURE and stat == [hip.ERROR_UNSUPPORTED_FEATURE, 0]
    assert np.array_equal(got[1], _apply_of_the_pieces(hip, primary, R.golden_jpeg(45, 37, 85), mds[1], R.FMT_HLG, hip.APPLY_EXACT))


def test_jpegr_decode_rgbmap_differs_from_the_luma_rendition(hip, orc):
    """what the feature is for: on the 45x37 golden, whose planes differ by construction, the per-channel rendition differs from the
    one uhdr_hip_jpegr_decode_batch_ex gives (the map's luma on all three channels) in at least one channel of at least 10 % of the
    pixels"""
    lib = hip.load()
    primary = _primary_jpeg(hip, orc, 180, 148, 115)
    data = _container(primary, R.golden_jpeg(45, 37, 85))
    rc, stat, new, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, [data], R.FMT_HLG, hip.APPLY_EXACT, True)
    assert rc == 0
    rc, stat, luma, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_batch_ex, [data], R.FMT_HLG, hip.APPLY_EXACT, True, flags=hip.DECODE_ANY_SAMPLING)
    assert rc == 0
    a, b = new[0].view(np.uint32), luma[0].view(np.uint32)
    frac = float(((a & 0x3FFFFFFF) != (b & 0x3FFFFFFF)).mean())
    print("pixels whose rendition differs from the luma rendition: %.3f" % frac)
    assert frac >= 0.10


def test_jpegr_decode_rgbmap_of_one_component_maps_and_sdr(hip, orc):
    """a file with a one-component map: the bytes of uhdr_hip_jpegr_decode_batch_ex in every mode; UHDR_HIP_OUTPUT_SDR unchanged for both"""
    lib = hip.load()
    sample = open(os.path.join(ROOT, "tests", "golden", "sample_jpegr.jpeg"), "rb").read()
    pair = R.lcg_pair(orc, 72, 40, 64, R.CG_709, R.CG_2100)
    rc, stat, made = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_batch, [pair], False, R.TF_HLG, 90, None, True)
    assert rc == 0
    rgbfile = _container(_primary_jpeg(hip, orc, 68, 36, 3), R.golden_jpeg(17, 9, 85))
    files = [made[0], sample, rgbfile]
    for out_fmt in (hip.OUTPUT_SDR, R.FMT_HLG, R.FMT_PQ):
        for mode in (hip.APPLY_EXACT, hip.APPLY_FAST, hip.APPLY_LUT, hip.APPLY_EXACT_UNFILTERED):
            for device in ((True, False) if mode == hip.APPLY_EXACT else (True,)):
                a = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files[:2], out_fmt, mode, device)
                b = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_batch_ex, files[:2], out_fmt, mode, device)
                assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == [0, 0]
                assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), (out_fmt, mode, device)
        if out_fmt == hip.OUTPUT_SDR:   # the map is not decompressed: the primary's RGBA either way
            a = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, [rgbfile], out_fmt, hip.APPLY_EXACT, True)
            b = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_batch_ex, [rgbfile], out_fmt, hip.APPLY_EXACT, True, flags=hip.DECODE_ANY_SAMPLING)
            assert a[0] == 0 and b[0] == 0 and np.array_equal(a[2][0], b[2][0])
    # the two modes that stay single-channel refuse a file with an RGB map and leave its neighbours alone
    for mode in (hip.APPLY_LUT, hip.APPLY_EXACT_UNFILTERED):
        rc, stat, got, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, R.FMT_HLG, mode, True)
        assert rc == hip.ERROR_UNSUPPORTED_FEATURE and stat == [0, 0, hip.ERROR_UNSUPPORTED_FEATURE]


@pytest.mark.parametrize("api0", [False, True])
def test_jpegr_round_trip(hip, orc, api0):
    """a file from the new encode, read by the new decode: apply-RGB on the decoded pieces"""
    lib = hip.load()
    pairs = [R.lcg_pair(orc, 72, 40, 65, R.CG_709, R.CG_2100), R.lcg_pair(orc, 264, 136, 66, R.CG_P3, R.CG_2100)]
    rc, stat, files = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_rgbmap_batch, pairs, api0, R.TF_HLG, 90, None, True)
    assert rc == 0
    for out_fmt, mode, boost in ((R.FMT_HLG, hip.APPLY_EXACT, FLT_MAX), (R.FMT_PQ, hip.APPLY_EXACT, 2.0), (R.FMT_F16, hip.APPLY_FAST, FLT_MAX)):
        rc, stat, got, dests, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, out_fmt, mode, True, boost=boost)
        assert rc == 0 and stat == [0, 0]
        for k, f in enumerate(files):
            primary, gm = _info(hip, f)
            want = _apply_of_the_pieces(hip, primary, gm, mds[k], out_fmt, mode, boost)
            if mode == hip.APPLY_EXACT:
                assert np.array_equal(got[k], want), (out_fmt, k)
            else:
                _check_fast(out_fmt, got[k], want, False, "round trip file %d fmt %d" % (k, out_fmt))


# ---- the C++ shim -------------------------------------------------------------------------------------------------------------------
def test_the_shims_setter(hip, orc, tmp_path):
    """ultrahdr::JpegRHip::setMultiChannelGainMap: on, encodeJPEGR API-1 writes the new call's bytes and decodeJPEGR returns the new
    call's; off, both return what they did"""
    lib = hip.load()
    exe = str(tmp_path / "shim_rgbmap_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_rgbmap_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    w, h = 72, 40
    pair = R.lcg_pair(orc, w, h, 67, R.CG_709, R.CG_2100)
    pair[2][0].tofile(str(tmp_path / "in.p010"))
    pair[2][1].tofile(str(tmp_path / "in.yuv"))
    r = subprocess.run([exe, str(tmp_path / "in.p010"), str(tmp_path / "in.yuv"), str(w), str(h), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n: open(tmp_path / n, "rb").read()
    rc, stat, new = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_rgbmap_batch, [pair], False, R.TF_HLG, 90, None, False)
    assert rc == 0 and rd("on.jpgr") == new[0]
    rc, stat, old = _jpegr_encode(hip, lib.uhdr_hip_jpegr_encode_batch, [pair], False, R.TF_HLG, 90, None, False)
    assert rc == 0 and rd("off.jpgr") == old[0] and old[0] != new[0]
    got = lambda n: np.frombuffer(rd(n), np.uint8)
    dec = lambda fn, f, flags=0: _jpegr_decode(hip, fn, [f], R.FMT_HLG, hip.APPLY_EXACT, False, flags=flags)[2][0]
    assert np.array_equal(got("on_dec_on.bin"), dec(lib.uhdr_hip_jpegr_decode_rgbmap_batch, new[0]))
    assert np.array_equal(got("on_dec_luma.bin"), dec(lib.uhdr_hip_jpegr_decode_batch_ex, new[0], hip.DECODE_ANY_SAMPLING))
    assert not np.array_equal(got("on_dec_on.bin"), got("on_dec_luma.bin"))
    assert np.array_equal(got("off_dec_off.bin"), dec(lib.uhdr_hip_jpegr_decode_batch_ex, old[0]))
    assert np.array_equal(got("off_dec_on.bin"), got("off_dec_off.bin"))
