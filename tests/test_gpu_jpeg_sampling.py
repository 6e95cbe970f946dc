"""Opt-in decode of 4:4:4, 4:2:2 and 4:4:0 JPEGs on the device (UHDR_HIP_DECODE_ANY_SAMPLING), their RGBA, applyGainMap over such
planes and JPEG/R files with such primaries.  Expected values: IJG libjpeg's raw_data_out planes (tests/golden/sampling/), Pillow's
(libjpeg-turbo's) decode, and the CPU oracle's applyGainMap on the 4:2:0 images that hold one chroma phase each."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests.sampling_cases import FIXTURES, FORMATS, JPEGR_MD, chroma_size, fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLT_MAX = 3.4028234663852886e38
pytestmark = pytest.mark.gpu


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _need(hip, d, decode_to):
    if decode_to == hip.DECODE_TO_RGBA:
        return d.width * d.height * 4
    if d.pixelFormat == hip.PIX_FMT_MONOCHROME:
        return d.width * d.height
    if d.pixelFormat == hip.PIX_FMT_YUV420:
        return d.width * d.height + 2 * (d.width * d.height // 4)
    cw, ch = hip.chroma_size(d.pixelFormat, d.width, d.height)
    return d.width * d.height + 2 * cw * ch


def _decode(hip, data, decode_to, device, flags=None):
    """probe, then decode: (status, bytes or None, descriptor).  flags None: the calls without flags"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    flags = hip.DECODE_ANY_SAMPLING if flags is None else flags
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    d = hip.Image()
    rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, None, 0, C.byref(d), hip.MEM_HOST, None, flags)
    if rc != hip.ERROR_INSUFFICIENT_RESOURCE:
        return rc, None, d
    need = _need(hip, d, decode_to)
    if device:
        t = dev_empty(need, 0xCD)
        rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, C.c_void_p(t.data_ptr()), need, C.byref(d), hip.MEM_DEVICE, stream_ptr(), flags)
        return rc, (to_host(t, need).copy() if rc == 0 else None), d
    out = np.full(need, 0xCD, np.uint8)
    rc = lib.uhdr_hip_jpeg_decode_ex(buf.ctypes.data, len(data), decode_to, C.c_void_p(out.ctypes.data), need, C.byref(d), hip.MEM_HOST, None, flags)
    return rc, (out if rc == 0 else None), d


def _decode_batch(hip, files, decode_to, device):
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    n = len(files)
    bufs = [np.frombuffer(f + b"\0" * 8, np.uint8) for f in files]
    jp, js = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [len(f) for f in files])
    descs, stat = (hip.Image * n)(), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpeg_decode_batch_ex(n, jp, js, decode_to, None, None, descs, stat, hip.MEM_HOST, None, hip.DECODE_ANY_SAMPLING)
    assert rc == hip.ERROR_INSUFFICIENT_RESOURCE and set(stat) == {hip.ERROR_INSUFFICIENT_RESOURCE}
    needs = [_need(hip, descs[i], decode_to) for i in range(n)]
    if device:
        outs = [dev_empty(k, 0xCD) for k in needs]
        ptrs = [t.data_ptr() for t in outs]
    else:
        outs = [np.full(k, 0xCD, np.uint8) for k in needs]
        ptrs = [a.ctypes.data for a in outs]
    rc = lib.uhdr_hip_jpeg_decode_batch_ex(n, jp, js, decode_to, _arr(C.c_void_p, ptrs), _arr(C.c_size_t, needs), descs, stat,
                                           hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr(), hip.DECODE_ANY_SAMPLING)
    got = [to_host(t, k).copy() for t, k in zip(outs, needs)] if device else outs
    return rc, list(stat), got, descs


def _pillow_jpeg(rgb, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", **kw)
    return b.getvalue()


def _pillow_rgba(data):
    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2).reshape(-1)


def _content(w, h, seed):
    """flat blocks of colour plus noise"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 5) // 6, (w + 5) // 6, 3))
    img = np.repeat(np.repeat(base, 6, axis=0), 6, axis=1)[:h, :w] + rng.integers(-24, 25, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def other_files():
    """files of the samplings the default calls read: Pillow-written 4:2:0 (two sizes) and grayscale, the committed 4:2:0 file"""
    from PIL import Image
    gray = io.BytesIO()
    Image.fromarray(_content(50, 34, 5)[:, :, 0]).save(gray, "JPEG", quality=90)
    return [_pillow_jpeg(_content(64, 48, 6), quality=90, subsampling=2), gray.getvalue(), _pillow_jpeg(_content(272, 200, 7), quality=95, subsampling=2),
            open(os.path.join(GOLDEN, "jpeg_image.jpg"), "rb").read()]


@pytest.mark.parametrize("device", [True, False])
def test_planes_of_every_fixture_are_libjpegs(hip, device):
    for name in FIXTURES:
        hs, vs, w, h, data, planes = fixture(name)
        rc, got, d = _decode(hip, data, hip.DECODE_TO_YCBCR, device)
        cw, ch = chroma_size(hs, vs, w, h)
        assert rc == 0 and (d.width, d.height, d.luma_stride, d.chroma_stride, d.pixelFormat) == (w, h, w, cw, FORMATS[(hs, vs)]), name
        assert d.chroma_data - d.data == w * h
        assert np.array_equal(got, planes), (name, int((got != planes).sum()))


@pytest.mark.parametrize("device", [True, False])
def test_a_batch_mixes_every_sampling(hip, other_files, device):
    """all samplings, baseline / restart-interval / progressive, with 4:2:0 and grayscale files in one call: every file as its single call"""
    files = []
    for k, name in enumerate(FIXTURES):   # (the other files spread through the batch)
        files.append(fixture(name)[4])
        if k % 12 == 5:
            files.append(other_files[k // 12])
    singles = [_decode(hip, f, hip.DECODE_TO_YCBCR, True) for f in files]
    plain = [_decode(hip, f, hip.DECODE_TO_YCBCR, True, flags=0) for f in other_files]
    assert all(rc == 0 for rc, _, _ in singles + plain)
    rc, stat, got, descs = _decode_batch(hip, files, hip.DECODE_TO_YCBCR, device)
    assert rc == 0 and stat == [0] * len(files)
    for i, (_, want, d) in enumerate(singles):
        assert (descs[i].width, descs[i].height, descs[i].chroma_stride, descs[i].pixelFormat) == (d.width, d.height, d.chroma_stride, d.pixelFormat)
        assert np.array_equal(got[i], want), i
    # a 4:2:0 / grayscale file with the flag is the file without it
    for f, (_, want, d) in zip(other_files, plain):
        i = files.index(f)
        assert np.array_equal(got[i], want) and descs[i].pixelFormat == d.pixelFormat


PILLOW_444 = [dict(size=(272, 200), quality=95), dict(size=(45, 37), quality=90), dict(size=(45, 37), quality=90, optimize=True),
              dict(size=(130, 70), quality=90, restart_marker_rows=1), dict(size=(45, 37), quality=90, progressive=True)]


def test_pillow_written_444_decodes_to_pillows_planes(hip):
    from PIL import Image
    for k, case in enumerate(PILLOW_444):
        kw = dict(case)
        w, h = kw.pop("size")
        data = _pillow_jpeg(_content(w, h, 40 + k), subsampling=0, **kw)
        im = Image.open(io.BytesIO(data))
        im.draft("YCbCr", (w, h))
        assert im.mode == "YCbCr"
        ycc = np.asarray(im)   # 4:4:4: libjpeg-turbo hands the samples over as decoded
        want = np.concatenate([ycc[:, :, c].reshape(-1) for c in range(3)])
        for device in (True, False):
            rc, got, d = _decode(hip, data, hip.DECODE_TO_YCBCR, device)
            assert rc == 0 and d.pixelFormat == hip.PIX_FMT_YUV444 and np.array_equal(got, want), (case, device)


def test_rgba_is_libjpeg_turbos(hip, other_files):
    files = [fixture(name)[4] for name in FIXTURES]
    for k, case in enumerate(PILLOW_444):
        kw = dict(case)
        w, h = kw.pop("size")
        files.append(_pillow_jpeg(_content(w, h, 40 + k), subsampling=0, **kw))
        files.append(_pillow_jpeg(_content(w, h, 60 + k), subsampling=1, **kw))   # 4:2:2
    for k, (w, h) in enumerate(((4, 8), (3, 5), (5, 3), (6, 4))):   # 4:2:2 rows of exactly 2 samples are replicated, of 3 filtered (jinit_upsampler)
        files.append(_pillow_jpeg(_content(w, h, 70 + k), quality=90, subsampling=1))
    files += [other_files[0], other_files[2]]   # 4:2:0, once: the old path against the same library
    want = [_pillow_rgba(f) for f in files]
    for device in (True, False):
        rc, stat, got, descs = _decode_batch(hip, files, hip.DECODE_TO_RGBA, device)
        assert rc == 0 and stat == [0] * len(files)
        for i in range(len(files)):
            assert np.array_equal(got[i], want[i]), (i, device, int((got[i] != want[i]).sum()))
    for i in (0, 20, 47, len(files) - 3, len(files) - 1):   # single calls, a few
        rc, got1, _ = _decode(hip, files[i], hip.DECODE_TO_RGBA, True)
        assert rc == 0 and np.array_equal(got1, want[i]), i


# ---- applyGainMap over the new formats --------------------------------------------------------------------------------------------
AW, AH, MW, MH = 64, 48, 16, 12


def _apply_inputs(fmt_pair):
    """a 64x48 image with chroma different at every sample, a 16x12 map"""
    hs, vs = fmt_pair
    rng = np.random.default_rng(100 + 10 * hs + vs)
    cw, ch = chroma_size(hs, vs, AW, AH)
    y = rng.integers(0, 256, (AH, AW)).astype(np.uint8)
    cb = ((np.arange(ch)[:, None] * 7 + np.arange(cw)[None, :] * 3) % 251).astype(np.uint8)
    cr = ((np.arange(ch)[:, None] * 5 + np.arange(cw)[None, :] * 11 + 17) % 241).astype(np.uint8)
    gmap = rng.integers(0, 256, (MH, MW)).astype(np.uint8)
    return y, cb, cr, gmap


def _phase_images(fmt_pair, y, cb, cr):
    """{(dx, dy): packed 4:2:0 image whose chroma is the samples the pixels of that phase read}"""
    hs, vs = fmt_pair
    out = {}
    for dy in range(2 if vs == 1 else 1):
        for dx in range(2 if hs == 1 else 1):
            sel = (slice(dy, None, 2) if vs == 1 else slice(None), slice(dx, None, 2) if hs == 1 else slice(None))
            out[(dx, dy)] = np.concatenate([y.reshape(-1), cb[sel].reshape(-1), cr[sel].reshape(-1)])
            assert out[(dx, dy)].size == AW * AH * 3 // 2
    return out


def _by_phase(fmt_pair, per_phase, out_fmt, hip):
    """output pixel (x, y) from the phase image (x & 1, y & 1) (a subsampled direction has one phase)"""
    hs, vs = fmt_pair
    xs, ys = np.meshgrid(np.arange(AW), np.arange(AH))
    px = (xs & 1) if hs == 1 else np.zeros_like(xs)
    py = (ys & 1) if vs == 1 else np.zeros_like(ys)
    if out_fmt == hip.OUTPUT_HDR_LINEAR_RGB_10BIT:
        planes = {k: v.view(np.uint16).reshape(3, AH, AW) for k, v in per_phase.items()}
        want = np.zeros((3, AH, AW), np.uint16)
        for (dx, dy), v in planes.items():
            sel = (px == dx) & (py == dy)
            want[:, sel] = v[:, sel]
        return want.reshape(-1).view(np.uint8)
    dt = np.uint64 if out_fmt == hip.OUTPUT_HDR_LINEAR else np.uint32
    want = np.zeros((AH, AW), dt)
    for (dx, dy), v in per_phase.items():
        sel = (px == dx) & (py == dy)
        want[sel] = v.view(dt).reshape(AH, AW)[sel]
    return want.reshape(-1).view(np.uint8)


def _gpu_apply_image(hip, img_desc_of, planes, gmap, out_fmt, mode, md, offset=0, size=(AW, AH, MW, MH)):
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    w, h, mw, mh = size
    dev = to_dev(np.concatenate([np.zeros(offset, np.uint8), planes]))
    dmap = to_dev(gmap)
    nbytes = hip.output_bytes(out_fmt, w, h)
    dout = dev_empty(nbytes, 0xCD)
    img = img_desc_of(dev.data_ptr() + offset)
    mimg, dest = hip.mono_image(dmap.data_ptr(), mw, mh), hip.out_image(dout.data_ptr())
    rc = lib.uhdr_hip_apply_gainmap(C.byref(img), C.byref(mimg), C.byref(md), out_fmt, FLT_MAX, C.byref(dest), mode, hip.MEM_DEVICE, stream_ptr())
    assert rc == 0
    return to_host(dout, nbytes).copy()


@pytest.mark.parametrize("fmt_pair", [(1, 1), (2, 1), (1, 2)])
def test_apply_exact_reads_the_chroma_sample_of_the_downsampled_grid(hip, orc, fmt_pair):
    """bit-identical to the oracle's applyGainMap on the 4:2:0 image that holds the pixel's chroma phase; device and host memory"""
    lib = hip.load()
    y, cb, cr, gmap = _apply_inputs(fmt_pair)
    planes = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    phases = _phase_images(fmt_pair, y, cb, cr)
    md, omd = hip.metadata(4.0), orc.Metadata(4.0, 1.0, 1.0, 0.0, 0.0, 1.0, 4.0, 1)
    pix_fmt = FORMATS[fmt_pair]
    for out_fmt in (hip.OUTPUT_HDR_LINEAR, hip.OUTPUT_HDR_PQ, hip.OUTPUT_HDR_HLG, hip.OUTPUT_HDR_LINEAR_RGB_10BIT):
        per_phase = {}
        for k, img in phases.items():
            st, out, _ = orc.apply("orc_", orc.yuv420_image(img, AW, AH, orc.CG_BT709), gmap, omd, out_fmt, FLT_MAX, threads=2)
            assert st == 0
            per_phase[k] = out[:hip.output_bytes(out_fmt, AW, AH)].copy()
        want = _by_phase(fmt_pair, per_phase, out_fmt, hip)
        for mode in (hip.APPLY_EXACT, hip.APPLY_EXACT_UNFILTERED):
            got = _gpu_apply_image(hip, lambda p: hip.ycbcr_image(p, AW, AH, hip.CG_BT709, pix_fmt), planes, gmap, out_fmt, mode, md)
            assert np.array_equal(got, want), (out_fmt, mode, int((got != want).sum()))
        # host memory: the staging copies the format's own chroma extent
        host_out = np.full(hip.output_bytes(out_fmt, AW, AH), 0xCD, np.uint8)
        himg, hmap, hdest = hip.ycbcr_image(planes.ctypes.data, AW, AH, hip.CG_BT709, pix_fmt), hip.mono_image(gmap.ctypes.data, MW, MH), hip.out_image(host_out.ctypes.data)
        assert lib.uhdr_hip_apply_gainmap(C.byref(himg), C.byref(hmap), C.byref(md), out_fmt, FLT_MAX, C.byref(hdest), hip.APPLY_EXACT, hip.MEM_HOST, None) == 0
        assert np.array_equal(host_out, want), out_fmt


@pytest.mark.parametrize("fmt_pair", [(1, 1), (2, 1), (1, 2)])
def test_apply_fast_and_lut_equal_the_general_path_on_the_phase_images(hip, fmt_pair):
    """FAST and LUT: what the same library returns for the 4:2:0 phase images through the per-pixel kernels -- their luma sits at an
    odd address, which the scale-4 fast kernels do not take, so both sides run the same kernel"""
    y, cb, cr, gmap = _apply_inputs(fmt_pair)
    planes = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    phases = _phase_images(fmt_pair, y, cb, cr)
    md = hip.metadata(4.0)
    pix_fmt = FORMATS[fmt_pair]
    for mode in (hip.APPLY_FAST, hip.APPLY_LUT):
        for out_fmt in (hip.OUTPUT_HDR_LINEAR, hip.OUTPUT_HDR_PQ, hip.OUTPUT_HDR_HLG):
            per_phase = {k: _gpu_apply_image(hip, lambda p: hip.yuv420_image(p, AW, AH, hip.CG_BT709), img, gmap, out_fmt, mode, md, offset=1)
                         for k, img in phases.items()}
            want = _by_phase(fmt_pair, per_phase, out_fmt, hip)
            got = _gpu_apply_image(hip, lambda p: hip.ycbcr_image(p, AW, AH, hip.CG_BT709, pix_fmt), planes, gmap, out_fmt, mode, md)
            assert np.array_equal(got, want), (mode, out_fmt, int((got != want).sum()))


def test_apply_batch_mixes_formats(hip):
    """one uhdr_hip_apply_gainmap_batch call over a 4:4:4, a 4:2:0, a 4:2:2 and a 4:4:0 image: each as its single call"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    md = hip.metadata(4.0)
    keep, imgs, maps, singles = [], [], [], []
    for fmt_pair in ((1, 1), (2, 2), (2, 1), (1, 2)):
        y, cb, cr, gmap = _apply_inputs(fmt_pair)
        planes = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
        dev, dmap = to_dev(planes), to_dev(gmap)
        keep += [dev, dmap]
        mk = (lambda p: hip.yuv420_image(p, AW, AH, hip.CG_BT709)) if fmt_pair == (2, 2) else (lambda p, f=FORMATS[fmt_pair]: hip.ycbcr_image(p, AW, AH, hip.CG_BT709, f))
        imgs.append(mk(dev.data_ptr()))
        maps.append(hip.mono_image(dmap.data_ptr(), MW, MH))
        singles.append(_gpu_apply_image(hip, mk, planes, gmap, hip.OUTPUT_HDR_HLG, hip.APPLY_EXACT, md))
    nbytes = hip.output_bytes(hip.OUTPUT_HDR_HLG, AW, AH)
    outs = [dev_empty(nbytes, 0xCD) for _ in imgs]
    dests = hip.image_array([hip.out_image(t.data_ptr()) for t in outs])
    rc = lib.uhdr_hip_apply_gainmap_batch(len(imgs), hip.image_array(imgs), hip.image_array(maps), C.byref(md), hip.OUTPUT_HDR_HLG, FLT_MAX, dests,
                                          hip.APPLY_EXACT, stream_ptr())
    assert rc == 0
    for t, want in zip(outs, singles):
        assert np.array_equal(to_host(t, nbytes), want)


# ---- JPEG/R files with such primaries -----------------------------------------------------------------------------------------------
def _jpegr_files():
    """(file, primary JPEG, gain map plane) for a Pillow 4:4:4 and a Pillow 4:2:2 primary of 64x48 with a grayscale 16x12 map JPEG"""
    from PIL import Image

    from oracle import jpegr_oracle as J
    out = []
    for k, sub in enumerate((0, 1)):
        primary = _pillow_jpeg(_content(AW, AH, 80 + k), quality=92, subsampling=sub)
        g = io.BytesIO()
        Image.fromarray(_content(MW, MH, 90 + k)[:, :, 0]).save(g, "JPEG", quality=85)
        data = J.append_gainmap(primary, g.getvalue(), JPEGR_MD)
        assert isinstance(data, bytes)
        out.append((data, primary, g.getvalue()))
    return out


def _jpegr_batch(hip, files, out_fmt, flags, device, ex=True):
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests, mds, stat = (hip.Image * n)(), (hip.Metadata * n)(), _arr(C.c_int, [7] * n)

    def call(optr, ocap, mem):
        if ex:
            return lib.uhdr_hip_jpegr_decode_batch_ex(n, ptrs, sizes, out_fmt, FLT_MAX, optr, ocap, dests, mds, stat, hip.APPLY_EXACT, mem, stream_ptr(), flags)
        return lib.uhdr_hip_jpegr_decode_batch(n, ptrs, sizes, out_fmt, FLT_MAX, optr, ocap, dests, mds, stat, hip.APPLY_EXACT, mem, stream_ptr())
    call(None, None, hip.MEM_HOST)
    probe = list(stat)
    live = [i for i in range(n) if probe[i] == hip.ERROR_INSUFFICIENT_RESOURCE]
    needs = [hip.output_bytes(out_fmt, dests[i].width, dests[i].height) if i in live else 16 for i in range(n)]
    if device:
        outs = [dev_empty(k, 0xCD) for k in needs]
        optr = _arr(C.c_void_p, [t.data_ptr() for t in outs])
    else:
        outs = [np.full(k, 0xCD, np.uint8) for k in needs]
        optr = _arr(C.c_void_p, [a.ctypes.data for a in outs])
    rc = call(optr, _arr(C.c_size_t, needs), hip.MEM_DEVICE if device else hip.MEM_HOST)
    got = [to_host(t, k).copy() for t, k in zip(outs, needs)] if device else outs
    return rc, probe, list(stat), got, dests, mds


@pytest.mark.parametrize("device", [True, False])
def test_jpegr_files_with_444_and_422_primaries(hip, device):
    sample = open(os.path.join(GOLDEN, "sample_jpegr.jpeg"), "rb").read()
    made = _jpegr_files()
    files = [made[0][0], sample, made[1][0]]
    # without the flag: as today, through either entry point
    for ex in (True, False):
        rc, probe, stat = _jpegr_batch(hip, files, hip.OUTPUT_HDR_HLG, 0, device, ex=ex)[:3]
        assert rc == hip.ERROR_DECODE_ERROR and stat == [hip.ERROR_DECODE_ERROR, 0, hip.ERROR_DECODE_ERROR] and probe[1] == hip.ERROR_INSUFFICIENT_RESOURCE
    for out_fmt in (hip.OUTPUT_SDR, hip.OUTPUT_HDR_HLG, hip.OUTPUT_HDR_PQ, hip.OUTPUT_HDR_LINEAR):
        rc, probe, stat, got, dests, mds = _jpegr_batch(hip, files, out_fmt, hip.DECODE_ANY_SAMPLING, device)
        assert rc == 0 and stat == [0, 0, 0], (out_fmt, stat)
        plain = _jpegr_batch(hip, [sample], out_fmt, 0, device, ex=False)
        assert plain[0] == 0 and np.array_equal(got[1], plain[3][0])   # the sample file: the existing call's bytes
        for k, i in ((0, 0), (1, 2)):
            data, primary, gm_jpeg = made[k]
            assert (dests[i].width, dests[i].height) == (AW, AH)
            if out_fmt == hip.OUTPUT_SDR:
                assert np.array_equal(got[i], _pillow_rgba(primary)), (k, out_fmt)
                continue
            # the HDR outputs: applyGainMap over the planes the decoder returns for the two JPEGs (checked above against libjpeg / Pillow)
            rc1, planes, d = _decode(hip, primary, hip.DECODE_TO_YCBCR, True)
            rc2, gplane, gd = _decode(hip, gm_jpeg, hip.DECODE_TO_YCBCR, True)
            assert rc1 == 0 and rc2 == 0 and gd.pixelFormat == hip.PIX_FMT_MONOCHROME and d.pixelFormat == (hip.PIX_FMT_YUV444, hip.PIX_FMT_YUV422)[k]
            want = _gpu_apply_image(hip, lambda p: hip.ycbcr_image(p, AW, AH, hip.CG_UNSPECIFIED, d.pixelFormat), planes, gplane.reshape(MH, MW), out_fmt,
                                    hip.APPLY_EXACT, mds[i])
            assert np.array_equal(got[i], want), (k, out_fmt)
    # the single call
    lib = hip.load()
    buf = np.frombuffer(made[1][0], np.uint8)
    out, dest = np.full(AW * AH * 4, 0xCD, np.uint8), hip.Image()
    args = (buf.ctypes.data, buf.size, hip.OUTPUT_SDR, FLT_MAX, C.c_void_p(out.ctypes.data), out.size, C.byref(dest), None, hip.APPLY_EXACT, hip.MEM_HOST, None)
    assert lib.uhdr_hip_jpegr_decode_ex(*args, 0) == hip.ERROR_DECODE_ERROR == lib.uhdr_hip_jpegr_decode(*args)
    assert lib.uhdr_hip_jpegr_decode_ex(*args, hip.DECODE_ANY_SAMPLING) == 0 and np.array_equal(out, _pillow_rgba(made[1][1]))


def test_a_gain_map_jpeg_with_chroma_contributes_its_luma(hip):
    """the gain map as a 4:4:4 colour JPEG: the rendition is that of the map's luma plane"""
    from oracle import jpegr_oracle as J
    primary = _pillow_jpeg(_content(AW, AH, 81), quality=92, subsampling=1)
    gm_jpeg = _pillow_jpeg(_content(MW, MH, 91), quality=85, subsampling=0)
    data = J.append_gainmap(primary, gm_jpeg, JPEGR_MD)
    rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], hip.OUTPUT_HDR_PQ, hip.DECODE_ANY_SAMPLING, True)
    assert rc == 0
    _, planes, d = _decode(hip, primary, hip.DECODE_TO_YCBCR, True)
    _, gplanes, gd = _decode(hip, gm_jpeg, hip.DECODE_TO_YCBCR, True)
    assert gd.pixelFormat == hip.PIX_FMT_YUV444
    want = _gpu_apply_image(hip, lambda p: hip.ycbcr_image(p, AW, AH, hip.CG_UNSPECIFIED, d.pixelFormat), planes, gplanes[:MW * MH].reshape(MH, MW),
                            hip.OUTPUT_HDR_PQ, hip.APPLY_EXACT, mds[0])
    assert np.array_equal(got[0], want)


def test_the_shims_setter_passes_the_flag(hip, tmp_path):
    """ultrahdr::JpegRHip::setDecodeAnySampling: off by default (ERROR_DECODE_ERROR, as the reference), on: the SDR rendition is Pillow's"""
    exe = str(tmp_path / "shim_sampling_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_sampling_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    data, primary, _ = _jpegr_files()[0]
    src, dst = str(tmp_path / "in.jpg"), str(tmp_path / "out.rgba")
    open(src, "wb").write(data)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(dst, np.uint8), _pillow_rgba(primary))


def test_jpegr_files_with_odd_sized_primaries(hip):
    """45x35 4:4:4 and 4:2:2 primaries (odd chroma extent) with a 9x7 map, scale 5: SDR is Pillow's RGB, HLG the apply of the decoded planes"""
    from PIL import Image

    from oracle import jpegr_oracle as J
    w, h, mw, mh = 45, 35, 9, 7
    for k, sub in enumerate((0, 1)):
        primary = _pillow_jpeg(_content(w, h, 85 + k), quality=92, subsampling=sub)
        g = io.BytesIO()
        Image.fromarray(_content(mw, mh, 95 + k)[:, :, 0]).save(g, "JPEG", quality=85)
        data = J.append_gainmap(primary, g.getvalue(), JPEGR_MD)
        rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], hip.OUTPUT_SDR, hip.DECODE_ANY_SAMPLING, True)
        assert rc == 0 and (dests[0].width, dests[0].height) == (w, h) and np.array_equal(got[0], _pillow_rgba(primary)), k
        rc, probe, stat, got, dests, mds = _jpegr_batch(hip, [data], hip.OUTPUT_HDR_HLG, hip.DECODE_ANY_SAMPLING, False)
        assert rc == 0, (k, stat)
        _, planes, d = _decode(hip, primary, hip.DECODE_TO_YCBCR, True)
        _, gplane, _ = _decode(hip, g.getvalue(), hip.DECODE_TO_YCBCR, True)
        assert d.pixelFormat == (hip.PIX_FMT_YUV444, hip.PIX_FMT_YUV422)[k]
        want = _gpu_apply_image(hip, lambda p: hip.ycbcr_image(p, w, h, hip.CG_UNSPECIFIED, d.pixelFormat), planes, gplane.reshape(mh, mw), hip.OUTPUT_HDR_HLG,
                                hip.APPLY_EXACT, mds[0], size=(w, h, mw, mh))
        assert np.array_equal(got[0], want), k
