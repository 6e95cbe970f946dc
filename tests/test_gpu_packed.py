"""-m gpu: packed RGBA inputs -- uhdr_hip_generate_gainmap_packed_batch against the model of
tests/packed_cases.py, bit for bit; uhdr_hip_jpeg_encode_rgba420_batch against Pillow's files, byte for byte;
uhdr_hip_jpegr_encode_packed_batch against the container of its parts; the C++ shim against the C call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gainmap_md_cases as M
from tests import packed_cases as P
from tests import rgbmap_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FORM_IDS = ["pq1010102", "hlg1010102", "f16"]
GAMUTS = [(P.CG_709, P.CG_2100), (P.CG_P3, P.CG_P3)]   # a conversion, and the identity
EXIF = b"Exif\0\0MM\0*\0\0\0\x08\0\0"


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _bpp(fmt):
    return 8 if fmt == P.FMT_F16 else 4


def _desc(hip, fmt, ptr, w, h, gamut, stride):
    make = {P.FMT_8888: hip.rgba8888_image, P.FMT_1010102: hip.rgba1010102_image, P.FMT_F16: hip.rgba_f16_image}[fmt]
    return make(ptr, w, h, gamut, stride)


def _laid_out(img, fmt, pad, shift):
    """the image's bytes with rows `pad` pixels longer and `shift` pixels in front of pixel (0, 0), all of it poison: (bytes, byte
    offset of pixel (0, 0), stride in pixels)"""
    h, w = img.shape[:2]
    bpp = _bpp(fmt)
    rows = np.full((h, (w + pad) * bpp), 0xEE, np.uint8)
    rows[:, :w * bpp] = np.ascontiguousarray(img).view(np.uint8).reshape(h, w * bpp)
    return np.concatenate([np.full(shift * bpp, 0xEE, np.uint8), rows.reshape(-1)]), shift * bpp, w + pad


class Pair:
    def __init__(self, sdr, hdr, fmt, gamuts=GAMUTS[0], pad=0, shift=0):
        self.sdr, self.hdr, self.fmt, self.gamuts, self.pad, self.shift = sdr, hdr, fmt, gamuts, pad, shift
        self.h, self.w = sdr.shape[:2]

    def on_device(self, hip):
        from tests.gpu_util import to_dev
        out = []
        for img, fmt, gamut in ((self.sdr, P.FMT_8888, self.gamuts[0]), (self.hdr, self.fmt, self.gamuts[1])):
            raw, off, stride = _laid_out(img, fmt, self.pad, self.shift)
            t = to_dev(raw)
            out += [_desc(hip, fmt, t.data_ptr() + off, self.w, self.h, gamut, stride), t]
        return out[0], out[2], (out[1], out[3])


def _generate(hip, pairs, tf, md, rgb, offset=0, shared=None):
    """one uhdr_hip_generate_gainmap_packed_batch call: (status, maps, dests, metadata_out).  md None: metadata_in = NULL.  shared:
    the descriptors of pairs[0] for every image of the call (its inputs are uploaded once)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    bpp = 4 if rgb else 1
    keep, ss, hs, outs = [], [], [], []
    for k, p in enumerate(pairs):
        if shared is None or k == 0:
            s, h, t = p.on_device(hip)
            keep.append(t)
        ss.append(s)
        hs.append(h)
        outs.append(dev_empty(bpp * (p.w // 4) * (p.h // 4) + 16 + offset, 0xCD))
    dests = hip.image_array([hip.out_image(t.data_ptr() + offset) for t in outs])
    md_out = hip.Metadata()
    rc = lib.uhdr_hip_generate_gainmap_packed_batch(len(pairs), hip.image_array(ss), hip.image_array(hs), tf, None if md is None else C.byref(md),
                                                    C.byref(md_out), dests, int(rgb), stream_ptr())
    maps = []
    for p, t in zip(pairs, outs):
        mw, mh = p.w // 4, p.h // 4
        full = to_host(t).copy()
        assert (full[offset + bpp * mw * mh:] == 0xCD).all() and (full[:offset] == 0xCD).all()   # the 16 guard bytes, and what lies in front
        m = full[offset:offset + bpp * mw * mh]
        maps.append(m.reshape(mh, mw, 4) if rgb else m.reshape(mh, mw))
    return rc, maps, dests, md_out


def _lcg_pair(w, h, fmt, tf, gamuts=GAMUTS[0], pad=0, shift=0):
    sdr, hdr = P.pair(w, h, fmt, P.seed_of(w, fmt, tf))
    return Pair(sdr, hdr, fmt, gamuts, pad, shift)


def _want(w, h, fmt, tf, rgb, gamuts=GAMUTS[0]):
    return P.expected_default(w, h, fmt, tf, P.seed_of(w, fmt, tf), bool(rgb), gamuts[0], gamuts[1])


def _md_tuple(md):
    return (md.version, md.maxContentBoost, md.minContentBoost, md.gamma, md.offsetSdr, md.offsetHdr, md.hdrCapacityMin, md.hdrCapacityMax)


def _reference_md(tf):
    lo, hi = P.default_range(tf)
    return (b"1.0", hi, lo, 1.0, 0.0, 0.0, lo, hi)


# ---- generate against the model, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("size", [(40, 24), (44, 20), (46, 22)], ids=lambda s: "%dx%d" % s)
def test_generate_against_the_model(hip, size, form):
    """40x24: map 10x6, one block, the 16-byte loads.  44x20: map 11x5, a thread with a lone pixel.  46x22: the same map, two
    trailing columns and rows that no sum may see.  metadata_in = NULL: the reference's constants, which metadata_out reports"""
    (w, h), (fmt, tf) = size, form
    for gamuts in GAMUTS:
        for rgb in (0, 1):
            rc, maps, dests, md = _generate(hip, [_lcg_pair(w, h, fmt, tf, gamuts)], tf, None, rgb, offset=8 * rgb)
            assert rc == 0, rc
            want = _want(w, h, fmt, tf, rgb, gamuts)
            assert np.array_equal(maps[0], want), (gamuts, rgb, np.argwhere(maps[0] != want)[:4])
            d = dests[0]
            assert (d.width, d.height, d.luma_stride, d.chroma_data, d.pixelFormat) == (w // 4, h // 4, w // 4, None,
                                                                                      hip.PIX_FMT_RGBA8888 if rgb else hip.PIX_FMT_MONOCHROME)
            assert _md_tuple(md) == _reference_md(tf)
    # the bytes are about something: a good share of the one-plane map is off both clamps
    one = _want(w, h, fmt, tf, 0)
    assert ((one > 0) & (one < 255)).mean() > 0.1


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_generate_padded_and_shifted(hip, form):
    """both strides padded with poison and data one pixel into its buffer -- 4-byte (F16: 8-byte) but not 16-byte aligned: the dword
    loads, and the same bytes as the aligned form.  Also: padded strides that keep the 16-byte rows, and each of the other ways out
    of the aligned form by itself (a stride, the dest)"""
    fmt, tf = form
    for rgb in (0, 1):
        aligned, odd = 8 * rgb, 4 * rgb + (1 - rgb)   # dest offsets: 8-byte (2-byte) aligned, and not
        for pad, shift, offset in ((5, 1, aligned), (4, 1, aligned), (4, 0, aligned), (3, 0, aligned), (0, 0, odd), (5, 1, odd)):
            rc, maps, _, _ = _generate(hip, [_lcg_pair(40, 24, fmt, tf, pad=pad, shift=shift)], tf, None, rgb, offset=offset)
            assert rc == 0 and np.array_equal(maps[0], _want(40, 24, fmt, tf, rgb)), (rgb, pad, shift, offset)


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_generate_two_sizes_in_one_call(hip, form):
    fmt, tf = form
    sizes = [(40, 24), (44, 20), (40, 24), (46, 22)]
    for rgb in (0, 1):
        rc, maps, _, _ = _generate(hip, [_lcg_pair(w, h, fmt, tf) for w, h in sizes], tf, None, rgb)
        assert rc == 0
        for (w, h), got in zip(sizes, maps):
            assert np.array_equal(got, _want(w, h, fmt, tf, rgb)), (w, h, rgb)


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_generate_with_metadata(hip, form):
    """metadata_in: the `default` and `gamma22` cases against the model of tests/gainmap_md_cases.py -- exact equality, nothing left out
    (tests/test_packed_cpu.py holds the input condition); explicit degenerate metadata is metadata_in = NULL"""
    fmt, tf = form
    w, h = 40, 24
    sl, hl, ys, yh = P.model(w, h, fmt, tf, P.seed_of(w, fmt, tf))
    for name in ("default", "gamma22"):
        md = M.api_metadata(hip, M.CASES[name])
        rc, maps, _, md_out = _generate(hip, [_lcg_pair(w, h, fmt, tf)], tf, md, 0)
        want, _ = M.encode(ys, yh, M.CASES[name])
        assert rc == 0 and np.array_equal(maps[0], want), (name, np.argwhere(maps[0] != want)[:4])
        assert _md_tuple(md_out) == _md_tuple(md)
        rc, maps, _, _ = _generate(hip, [_lcg_pair(w, h, fmt, tf)], tf, md, 1)
        want, _ = M.encode(sl, hl, M.CASES[name])
        assert rc == 0 and np.array_equal(maps[0][:, :, :3], want) and (maps[0][:, :, 3] == 0xFF).all(), name
    lo, hi = P.default_range(tf)
    for rgb in (0, 1):
        rc, maps, _, _ = _generate(hip, [_lcg_pair(w, h, fmt, tf)], tf, M.api_metadata(hip, (1.0, 0.0, 0.0, lo, hi, lo, hi)), rgb)
        assert rc == 0 and np.array_equal(maps[0], _want(w, h, fmt, tf, rgb))


@pytest.fixture(scope="module")
def big_pairs():
    """one 1024x512 pair per HDR format, numpy-random contents (halves: patterns up to 4.0)"""
    rng = np.random.default_rng(2024)
    w, h = 1024, 512
    sdr = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    out = {P.FMT_1010102: (sdr, rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)),
           P.FMT_F16: (sdr, rng.integers(0, 0x4401, (h, w, 4)).astype(np.uint16))}
    return out


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_generate_past_one_block_one_tile_and_the_large_launch(hip, form, big_pairs):
    """64 descriptors of one 1024x512 pair, each with its own dest: 64 x 16 spans of kGenBlock * kGenTiles pairs, the large-launch
    form (four spans per block).  Every dest equals the n = 1 call's bytes -- the small form, one span per block, 64 blocks -- and a
    256x160 crop of that equals the model"""
    fmt, tf = form
    sdr, hdr = big_pairs[fmt]
    pair = Pair(sdr, hdr, fmt)
    for rgb in (0, 1):
        rc, one, _, _ = _generate(hip, [pair], tf, None, rgb)
        assert rc == 0
        rc, many, _, _ = _generate(hip, [pair] * 64, tf, None, rgb, shared=True)
        assert rc == 0
        for k, got in enumerate(many):
            assert np.array_equal(got, one[0]), (rgb, k)
        cw, ch = 256, 160
        sl, hl, ys, yh = P.linear_nits(sdr[:ch, :cw], hdr[:ch, :cw], fmt, tf, *GAMUTS[0])
        if rgb:
            assert np.array_equal(one[0][:ch // 4, :cw // 4, :3], P.encode_default(sl, hl, tf)) and (one[0][:, :, 3] == 0xFF).all()
        else:
            assert np.array_equal(one[0][:ch // 4, :cw // 4], P.encode_default(ys, yh, tf))


# ---- RGBA8888 -> 4:2:0 files ----------------------------------------------------------------------------------------------------------
def _encode_420(hip, images, qualities, device, caps=None, strides=None, iccs=None, spoil=None):
    """one uhdr_hip_jpeg_encode_rgba420_batch call: (status, statuses, sizes, files); spoil: {index: function that edits the descriptor}"""
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
        t = to_dev(src) if device else src
        keep.append(t)
        descs.append(hip.rgba8888_image(t.data_ptr() if device else src.ctypes.data, w, h, hip.CG_BT709, st))
        if spoil and k in spoil:
            spoil[k](descs[-1])
    if device:
        outs = [dev_empty(c + 16, 0xCD) for c in caps]
        optr = _arr(C.c_void_p, [t.data_ptr() if c else None for t, c in zip(outs, caps)])
    else:
        outs = [np.full(c + 16, 0xCD, np.uint8) for c in caps]
        optr = _arr(C.c_void_p, [a.ctypes.data if c else None for a, c in zip(outs, caps)])
    ip = isz = None
    if iccs is not None:
        ib = [np.frombuffer(i, np.uint8) if i else None for i in iccs]
        keep.append(ib)
        ip, isz = _arr(C.c_void_p, [b.ctypes.data if b is not None else None for b in ib]), _arr(C.c_size_t, [len(i) if i else 0 for i in iccs])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpeg_encode_rgba420_batch(n, hip.image_array(descs), _arr(C.c_int, qualities), ip, isz, optr, _arr(C.c_size_t, caps), sizes, stat,
                                                hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
    files = []
    for k in range(n):
        full = to_host(outs[k]).copy() if device else outs[k]
        if stat[k] == 0:
            assert (full[sizes[k]:] == 0xCD).all()
        files.append(full[:sizes[k]].tobytes() if stat[k] == 0 else None)
    return rc, list(stat), list(sizes), files


def _with_alpha(rgb, seed):
    h, w = rgb.shape[:2]
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 1)).astype(np.uint8)   # alpha is ignored
    return np.ascontiguousarray(np.concatenate([rgb, a], axis=2))


def _corpus():
    """(image (h, w, 4), quality, Pillow's file): the new fixtures and the two committed 4:2:0 files of the per-channel corpus"""
    items = [(P.golden_rgba(w, h), q, P.golden_jpeg_420(w, h, q)) for w, h, q in P.JPEG_CASES]
    items += [(_with_alpha(R.golden_rgb(w, h), w), 85, R.golden_jpeg_420(w, h)) for w, h in R.WITH_420]
    return items


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("k", range(8), ids=["1x1", "16x16", "40x24", "34x18", "17x9", "120x104", "45x37", "264x200"])
def test_rgba420_writes_pillows_file(hip, k, device):
    img, q, want = _corpus()[k]
    rc, stat, sizes, files = _encode_420(hip, [img], [q], device)
    assert rc == 0 and stat == [0] and sizes == [len(want)], (rc, stat, sizes, len(want))
    assert files[0] == want, "first difference at byte %d of %d" % (_first_diff(files[0], want), len(want))


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_rgba420_batch_strides_icc_probe_and_a_failing_file(hip, device):
    lib = hip.load()
    corpus = _corpus()
    images, quals, want = [c[0] for c in corpus], [c[1] for c in corpus], [c[2] for c in corpus]
    n = len(images)
    # one call for every size and quality, rows 5 pixels longer than the image: the stride is honoured
    rc, stat, sizes, files = _encode_420(hip, images, quals, device, strides=[im.shape[1] + 5 for im in images])
    assert rc == 0 and stat == [0] * n and files == want
    # an ICC profile per file: the no-ICC file plus the APP2 segment behind the JFIF header, where uhdr_hip_jpeg_encode puts it
    iccs = []
    for gamut in (hip.CG_BT709, hip.CG_P3, None):
        if gamut is None:
            iccs.append(None)
            continue
        buf, sz = np.zeros(4096, np.uint8), C.c_size_t()
        assert lib.uhdr_hip_icc_profile(hip.TF_SRGB, gamut, C.c_void_p(buf.ctypes.data), buf.size, C.byref(sz)) == 0
        iccs.append(buf[:sz.value].tobytes())
    rc, stat, sizes, files = _encode_420(hip, images[2:5], quals[2:5], device, iccs=iccs, caps=[8192] * 3)
    assert rc == 0 and stat == [0, 0, 0]
    for got, plain, icc in zip(files, want[2:5], iccs):
        seg = b"" if icc is None else b"\xff\xe2" + (len(icc) + 2).to_bytes(2, "big") + icc
        assert got == plain[:20] + seg + plain[20:]
    # the planar encoder puts the same segment in the same place
    w, h = 16, 16
    yuv = np.full(w * h * 3 // 2, 128, np.uint8)
    out, sz = np.zeros(8192, np.uint8), C.c_size_t()
    icc = np.frombuffer(iccs[0], np.uint8)
    y = hip.yuv420_image(yuv.ctypes.data, w, h, hip.CG_BT709)
    assert lib.uhdr_hip_jpeg_encode(C.byref(y), 90, C.c_void_p(icc.ctypes.data), icc.size, C.c_void_p(out.ctypes.data), out.size, C.byref(sz), hip.MEM_HOST, None) == 0
    assert out[:sz.value].tobytes()[20:24 + len(iccs[0])] == files[0][20:24 + len(iccs[0])]
    # the probe: no buffer / one byte short -> INSUFFICIENT_RESOURCE with the exact size; a failing file (a stride below its width)
    # beside good ones leaves their bytes alone
    caps = [len(f) + 64 for f in want]
    caps[1], caps[3] = 0, len(want[3]) - 1

    def short_stride(d):
        d.luma_stride = d.width - 1
    rc, stat, sizes, files = _encode_420(hip, images, quals, device, caps=caps, spoil={4: short_stride})
    ir, mm = hip.ERROR_INSUFFICIENT_RESOURCE, hip.ERROR_RESOLUTION_MISMATCH
    assert rc == ir and stat == [0, ir, 0, ir, mm, 0, 0, 0], stat
    assert [sizes[k] for k in (0, 1, 2, 3, 5, 6, 7)] == [len(want[k]) for k in (0, 1, 2, 3, 5, 6, 7)]
    assert [files[k] for k in (0, 2, 5, 6, 7)] == [want[k] for k in (0, 2, 5, 6, 7)]


# ---- JPEG/R files ---------------------------------------------------------------------------------------------------------------------
def _random_pair(w, h, fmt, seed, gamuts=GAMUTS[0]):
    rng = np.random.default_rng(seed)
    sdr = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    if fmt == P.FMT_F16:
        hdr = rng.integers(0, 0x4401, (h, w, 4)).astype(np.uint16)
    else:
        hdr = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    return Pair(sdr, hdr, fmt, gamuts)


def _jpegr_encode_packed(hip, pairs, tf, q, rgb_map, exifs, device, descs=None):
    """one uhdr_hip_jpegr_encode_packed_batch call: (status, statuses, files); descs: (hdr, sdr) descriptors to use instead"""
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    n = len(pairs)
    keep, ss, hs = [], [], []
    for p in pairs:
        if device:
            s, h, t = p.on_device(hip)
            keep.append(t)
        else:
            sa, ha = np.ascontiguousarray(p.sdr), np.ascontiguousarray(p.hdr)
            keep.append((sa, ha))
            s = _desc(hip, P.FMT_8888, sa.ctypes.data, p.w, p.h, p.gamuts[0], p.w)
            h = _desc(hip, p.fmt, ha.ctypes.data, p.w, p.h, p.gamuts[1], p.w)
        ss.append(s)
        hs.append(h)
    if descs is not None:
        for k, d in descs.items():
            hs[k], ss[k] = d(hs[k], ss[k])
    caps = [p.w * p.h * 6 + 65536 for p in pairs]
    outs = [np.zeros(c, np.uint8) for c in caps]
    ex = exn = None
    if exifs is not None:
        eb = [np.frombuffer(e, np.uint8) if e else None for e in exifs]
        keep.append(eb)
        ex, exn = _arr(C.c_void_p, [e.ctypes.data if e is not None else None for e in eb]), _arr(C.c_size_t, [len(e) if e else 0 for e in exifs])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpegr_encode_packed_batch(n, hip.image_array(hs), hip.image_array(ss), tf, q, ex, exn, _arr(C.c_void_p, [o.ctypes.data for o in outs]),
                                                _arr(C.c_size_t, caps), sizes, stat, int(rgb_map), hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
    return rc, list(stat), [outs[k][:sizes[k]].tobytes() if stat[k] == 0 else None for k in range(n)]


def _file_of_the_parts(hip, pair, tf, q, rgb_map, exif):
    """uhdr_hip_jpegr_append_gainmap of the parts: the map of the packed generate through the existing map encoders at quality 85, the
    primary of uhdr_hip_jpeg_encode_rgba420_batch at q with the SDR gamut's ICC profile, the metadata the generate reports"""
    from tests.test_gpu_rgbmap import _encode_rgb
    lib = hip.load()
    rc, maps, _, md = _generate(hip, [pair], tf, None, rgb_map)
    assert rc == 0
    if rgb_map:
        rc, stat, _, files = _encode_rgb(hip, [maps[0]], [85], True)
        assert rc == 0
        gm = files[0]
    else:
        plane = np.ascontiguousarray(maps[0])
        out, sz = np.zeros(plane.size * 2 + 4096, np.uint8), C.c_size_t()
        img = hip.mono_image(plane.ctypes.data, plane.shape[1], plane.shape[0])
        assert lib.uhdr_hip_jpeg_encode(C.byref(img), 85, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(sz), hip.MEM_HOST, None) == 0
        gm = out[:sz.value].tobytes()
    buf, sz = np.zeros(4096, np.uint8), C.c_size_t()
    assert lib.uhdr_hip_icc_profile(hip.TF_SRGB, pair.gamuts[0], C.c_void_p(buf.ctypes.data), buf.size, C.byref(sz)) == 0
    rc, stat, _, files = _encode_420(hip, [pair.sdr], [q], True, iccs=[buf[:sz.value].tobytes()], caps=[pair.w * pair.h * 4 + 8192])
    assert rc == 0
    primary = files[0]
    pb, gb = np.frombuffer(primary, np.uint8), np.frombuffer(gm, np.uint8)
    eb = np.frombuffer(exif, np.uint8) if exif else None
    out, sz = np.zeros(len(primary) + len(gm) + 8192, np.uint8), C.c_size_t()
    rc = lib.uhdr_hip_jpegr_append_gainmap(pb.ctypes.data, pb.size, gb.ctypes.data, gb.size, eb.ctypes.data if exif else None, len(exif) if exif else 0, None, 0,
                                           C.byref(md), C.c_void_p(out.ctypes.data), out.size, C.byref(sz))
    assert rc == 0
    return out[:sz.value].tobytes(), primary


@pytest.mark.parametrize("form", P.FORMS[1:], ids=FORM_IDS[1:])
@pytest.mark.parametrize("rgb_map", [0, 1], ids=["oneplane", "rgbmap"])
@pytest.mark.parametrize("size", [(48, 32), (264, 200)], ids=lambda s: "%dx%d" % s)
def test_jpegr_encode_packed_is_the_container_of_its_parts(hip, size, rgb_map, form):
    from tests.test_gpu_rgbmap import _jpeg_decode, _jpegr_decode
    lib = hip.load()
    (w, h), (fmt, tf) = size, form
    pair = _random_pair(w, h, fmt, 100 + w + fmt, gamuts=(P.CG_P3, P.CG_2100))
    exif = EXIF if rgb_map else None
    rc, stat, files = _jpegr_encode_packed(hip, [pair], tf, 92, rgb_map, [exif], True)
    assert rc == 0 and stat == [0]
    want, primary = _file_of_the_parts(hip, pair, tf, 92, rgb_map, exif)
    assert files[0] == want, "first difference at byte %d of %d / %d" % (_first_diff(files[0], want), len(files[0]), len(want))
    rc, stat, host = _jpegr_encode_packed(hip, [pair], tf, 92, rgb_map, [exif], False)
    assert rc == 0 and host == files                       # images in host memory: the same file
    # the file reads back: status 0, the primary's RGBA rendition, the reference's constants
    rc, stat, got, dests, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, hip.OUTPUT_SDR, hip.APPLY_EXACT, True)
    assert rc == 0 and stat == [0] and (dests[0].width, dests[0].height) == (w, h)
    rc, rgba, _ = _jpeg_decode(hip, primary, hip.DECODE_TO_RGBA, 0)
    assert rc == 0 and np.array_equal(got[0], rgba)
    # the container's XMP carries log2 of the two upper boosts as "%g" text, six significant digits of 2.3 or 5.6: the value read back
    # is within 2^(5e-6) - 1 < 4e-6 of the constant; every other field is exact
    got_md, ref_md = _md_tuple(mds[0]), _reference_md(tf)
    assert [got_md[k] for k in (0, 2, 3, 4, 5, 6)] == [ref_md[k] for k in (0, 2, 3, 4, 5, 6)]
    assert abs(got_md[1] / ref_md[1] - 1) <= 4e-6 and abs(got_md[7] / ref_md[7] - 1) <= 4e-6, got_md
    rc, stat, got, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, hip.OUTPUT_HDR_HLG, hip.APPLY_EXACT, True)
    assert rc == 0 and stat == [0]


def test_jpegr_encode_packed_three_files_one_bad_in_the_middle(hip):
    fmt, tf = P.FMT_1010102, P.TF_HLG
    pairs = [_random_pair(48, 32, fmt, 7), _random_pair(40, 24, fmt, 8), _random_pair(264, 200, fmt, 9, gamuts=(P.CG_P3, P.CG_P3))]

    def spoil(hd, sd):
        sd.colorGamut = -1
        return hd, sd
    for rgb_map in (0, 1):
        rc, stat, files = _jpegr_encode_packed(hip, pairs, tf, 80, rgb_map, [None, EXIF, EXIF], True, descs={1: spoil})
        assert rc == hip.ERROR_INVALID_COLORGAMUT and stat == [0, hip.ERROR_INVALID_COLORGAMUT, 0]
        for k in (0, 2):
            want, _ = _file_of_the_parts(hip, pairs[k], tf, 80, rgb_map, [None, EXIF, EXIF][k])
            assert files[k] == want, (rgb_map, k)


# ---- the C++ shim -----------------------------------------------------------------------------------------------------------------------
def test_the_shim_gives_the_c_calls_bytes(hip, tmp_path):
    """ultrahdr::JpegRHip::encodeJPEGRPacked (with and without setMultiChannelGainMap) and the free generateGainMapPacked"""
    exe = str(tmp_path / "shim_packed_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # generateGainMapPacked takes device memory: the HIP runtime's C API, no device code
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_packed_test.cpp"), "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip",
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    w, h = 72, 40
    for fmt, tf, name in ((P.FMT_1010102, P.TF_PQ, "pq"), (P.FMT_F16, P.TF_LINEAR, "f16")):
        pair = _random_pair(w, h, fmt, 55 + fmt)
        pair.sdr.tofile(str(tmp_path / "in.rgba"))
        pair.hdr.tofile(str(tmp_path / "in.hdr"))
        r = subprocess.run([exe, str(tmp_path / "in.rgba"), str(tmp_path / "in.hdr"), str(w), str(h), "f16" if fmt == P.FMT_F16 else "1010102", str(tf),
                            str(tmp_path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        rd = lambda n: open(tmp_path / n, "rb").read()   # noqa: E731
        for rgb_map, stem in ((0, "one"), (1, "rgb")):
            rc, stat, files = _jpegr_encode_packed(hip, [pair], tf, 90, rgb_map, None, False)
            assert rc == 0 and rd(stem + ".jpgr") == files[0], (name, stem)
            rc, maps, _, _ = _generate(hip, [pair], tf, None, rgb_map)
            assert rc == 0 and rd(stem + ".map") == maps[0].tobytes(), (name, stem)
