"""-m gpu: the run and slot bookkeeping of the tone-map and convertYuv batch calls (DESIGN.md sections 4, 4.1.3 and 4.1.7), on the
layouts of tests/tone_run_cases.py: a run that ends at the cap of 32 with its size run going on, a class break inside a size run, a
gamut break, a run with no measured member, sparse measured subsets, and more headroom slots than one chunk of 512.

The rule is the one of tests/test_gpu_tonemap.py and tests/test_gpu_packed_tonemap.py, through their helpers: H equals the model's
bit for bit, samples not in doubt equal the model, samples in doubt differ by at most one code, guard bytes and padding columns as
those tests require, dests[i] filled as they require.  tests/test_tone_runs_cpu.py holds the conditions on the inputs (distinct
measured H values strictly between 1 and k, the pooled doubt share, the runs each layout takes).  The shift and convertYuv are
compared with the oracle byte for byte."""
import ctypes as C

import numpy as np
import pytest

from tests import packed_tonemap_cases as K
from tests import tone_run_cases as R
from tests import tonemap_cases as T
from tests.gpu_util import stream_ptr
from tests.test_gpu_packed_tonemap import Frame as PackedFrame
from tests.test_gpu_packed_tonemap import check_pixels
from tests.test_gpu_packed_tonemap import run_batch as run_packed_batch
from tests.test_gpu_tonemap import GUARD, Frame, check_planes, run_batch

pytestmark = pytest.mark.gpu
F = np.float32
TFS = [T.TF_HLG, T.TF_PQ, T.TF_LINEAR]


# ------------------------------------------------------------------ frames of a layout, and the class each one really got
def planar_frames(hip, images, tf):
    return [Frame(hip, *R.planar_planes(im.w, im.h, im.content, tf), im.gamut, *(im.strides or (None,) * 4), offset=im.off) for im in images]


def packed_frames(hip, images, form):
    mul = 2 if form[0] == K.FMT_F16 else 1      # (an F16 source lies on 8 bytes)
    return [PackedFrame(hip, R.packed_image(form, im.w, im.h, im.content), form[0], im.gamut, *(im.strides or (None, None)), offset=im.off * mul)
            for im in images]


def _v(d):
    return d.chroma_data + d.chroma_stride * d.height // 2


def sdr_aligned(f):
    s, d = f.src, f.dst
    return (s.width % 16 == 0 and s.data % 16 == 0 and s.luma_stride % 8 == 0 and s.chroma_data % 16 == 0 and s.chroma_stride % 8 == 0 and
            d.data % 16 == 0 and d.luma_stride % 16 == 0 and d.chroma_data % 8 == 0 and _v(d) % 8 == 0 and d.chroma_stride % 8 == 0)


def shift_aligned(f):
    s, d = f.src, f.dst
    return (s.width % 16 == 0 and s.data % 16 == 0 and s.luma_stride % 8 == 0 and s.chroma_data % 16 == 0 and s.chroma_stride % 8 == 0 and
            d.data % 8 == 0 and d.luma_stride % 8 == 0 and d.chroma_data % 8 == 0 and _v(d) % 8 == 0 and d.chroma_stride % 8 == 0)


def convert_aligned(f):
    d = f.dst
    return d.width % 8 == 0 and d.data % 8 == 0 and d.luma_stride % 8 == 0 and d.chroma_data % 4 == 0 and _v(d) % 4 == 0 and d.chroma_stride % 4 == 0


def packed_aligned(f):
    s, d = f.src, f.dst
    return s.width % 4 == 0 and s.data % 16 == 0 and s.luma_stride % (2 if f.fmt == K.FMT_F16 else 4) == 0 and d.data % 16 == 0 and d.luma_stride % 4 == 0


def _reset(frames):
    for f in frames:
        f.dy.fill_(0xCD)
        f.dc.fill_(0xCD)


# ------------------------------------------------------------------ the two operators
def _check_planar(hip, name, images, frames, tf, null):
    rc, head, ok, da = run_batch(hip, frames, tf, R.peaks(images, null))
    wants = [R.planar_expected(im, tf, measured=null) for im in images]
    wrong = [i for i, w in enumerate(wants) if head[i].tobytes() != w["H"].tobytes()]
    print("tone-runs-observed %s: status %d, %d of %d headrooms differ from the model%s" % (name, rc, len(wrong), len(images),
          "".join(" [%d: device %r model %r]" % (i, head[i], wants[i]["H"]) for i in wrong[:8])))
    assert rc == 0 and ok and not wrong
    for i, (im, f, w) in enumerate(zip(images, frames, wants)):
        check_planes("%s[%d]" % (name, i), f, w)
        d = da[i]
        assert (d.colorGamut, d.data, d.chroma_data, d.width, d.height, d.luma_stride, d.chroma_stride) == (
            im.gamut, f.dst.data, f.dst.chroma_data, im.w, im.h, f.dst.luma_stride, f.dst.chroma_stride), i


@pytest.mark.parametrize("tf", TFS)
def test_planar_operator_over_the_run_layout(hip, tf):
    images = R.layout(False)
    frames = planar_frames(hip, images, tf)
    assert [sdr_aligned(f) for f in frames] == [im.aligned for im in images]      # every image got the class its layout names
    _check_planar(hip, "planar-tf%d-peaks" % tf, images, frames, tf, False)
    _reset(frames)
    _check_planar(hip, "planar-tf%d-null" % tf, images, frames, tf, True)


@pytest.mark.parametrize("tf", TFS)
def test_planar_operator_over_more_slots_than_a_head_chunk(hip, tf):
    images = R.many(False)
    frames = planar_frames(hip, images, tf)
    assert all(sdr_aligned(f) for f in frames)
    _check_planar(hip, "planar-many-tf%d" % tf, images, frames, tf, False)


def _check_packed(hip, name, images, frames, form, null):
    rc, head, ok, da = run_packed_batch(hip, frames, form[1], R.peaks(images, null))
    wants = [R.packed_expected(im, form, measured=null) for im in images]
    wrong = [i for i, w in enumerate(wants) if head[i].tobytes() != w["H"].tobytes()]
    print("tone-runs-observed %s: status %d, %d of %d headrooms differ from the model%s" % (name, rc, len(wrong), len(images),
          "".join(" [%d: device %r model %r]" % (i, head[i], wants[i]["H"]) for i in wrong[:8])))
    assert rc == 0 and ok and not wrong
    for i, (im, f, w) in enumerate(zip(images, frames, wants)):
        check_pixels("%s[%d]" % (name, i), f, w)
        d = da[i]
        assert (d.width, d.height, d.luma_stride, d.colorGamut, d.pixelFormat, d.data) == (im.w, im.h, f.ds, im.gamut, hip.PIX_FMT_RGBA8888, f.dst.data), i


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
def test_packed_operator_over_the_run_layout(hip, form):
    images = R.layout(True)
    frames = packed_frames(hip, images, form)
    assert [packed_aligned(f) for f in frames] == [im.aligned for im in images]
    _check_packed(hip, "packed-%s-peaks" % K.FORM_IDS[K.FORMS.index(form)], images, frames, form, False)
    for f in frames:
        f.reset()
    _check_packed(hip, "packed-%s-null" % K.FORM_IDS[K.FORMS.index(form)], images, frames, form, True)


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
def test_packed_operator_over_more_slots_than_a_head_chunk(hip, form):
    images = R.many(True)
    frames = packed_frames(hip, images, form)
    assert all(packed_aligned(f) for f in frames)
    _check_packed(hip, "packed-many-%s" % K.FORM_IDS[K.FORMS.index(form)], images, frames, form, False)


# ------------------------------------------------------------------ the shift and convertYuv against the oracle
def _oracle_planes(orc, f, luma, chroma):
    """the oracle's toneMap of a frame's image into planes laid out (and pre-filled) like the frame's destination"""
    pad = lambda a, s: np.ascontiguousarray(np.pad(a, ((0, 0), (0, s - a.shape[1]))))      # noqa: E731
    pl, pc = pad(luma, f.ls), pad(chroma, f.cs)
    oy, oc = np.full(f.ny, 0xCD, np.uint8), np.full(f.nc, 0xCD, np.uint8)
    osrc = orc.p010_image(pl, f.w, f.h, f.gamut, f.ls, f.cs, pc)
    odst = orc.yuv420_image(oy, f.w, f.h, -1, f.dls, f.dcs, oc)
    assert orc.load().orc_toneMap(C.byref(osrc), C.byref(odst)) == 0
    return oy, oc


def _equal_planes(f, oy, oc):
    y, u, v, ok = f.result()
    half = f.dcs * f.h // 2
    return ok and np.array_equal(y.reshape(-1), oy) and np.array_equal(u.reshape(-1), oc[:half]) and np.array_equal(v.reshape(-1), oc[half:2 * half])


def test_shift_and_convert_yuv_over_the_run_layout(hip, orc):
    """uhdr_hip_tonemap_batch, uhdr_hip_tonemap_sdr_batch with TONEMAP_SHIFT and uhdr_hip_convert_yuv_batch (in place on the planes
    just written) equal orc_toneMap and orc_convertYuv byte for byte, padding columns and guard bytes included"""
    lib = hip.load()
    images = R.layout(False)
    frames = planar_frames(hip, images, T.TF_PQ)
    assert [shift_aligned(f) for f in frames] == [im.aligned for im in images] == [convert_aligned(f) for f in frames]
    want = [_oracle_planes(orc, f, *R.planar_planes(im.w, im.h, im.content, T.TF_PQ)) for im, f in zip(images, frames)]
    n = len(frames)
    sa, da = hip.image_array([f.src for f in frames]), hip.image_array([f.dst for f in frames])
    assert lib.uhdr_hip_tonemap_batch(n, sa, da, stream_ptr()) == 0
    assert all(_equal_planes(f, *w) for f, w in zip(frames, want))
    assert [d.colorGamut for d in da] == [im.gamut for im in images]
    _reset(frames)
    rc, head, ok, db = run_batch(hip, frames, T.TF_PQ, None, op=T.SHIFT)      # the same launches through the operator's call
    assert rc == 0 and ok and (head.view(np.uint8) == 0xCD).all() and all(_equal_planes(f, *w) for f, w in zip(frames, want))
    assert [d.colorGamut for d in db] == [im.gamut for im in images]
    assert lib.uhdr_hip_convert_yuv_batch(n, da, hip.CG_BT2100, hip.CG_P3, stream_ptr()) == 0
    for f, (oy, oc) in zip(frames, want):
        oimg = orc.yuv420_image(oy, f.w, f.h, orc.CG_BT2100, f.dls, f.dcs, oc)
        assert orc.load().orc_convertYuv(C.byref(oimg), orc.CG_BT2100, orc.CG_P3) == 0
    assert all(_equal_planes(f, *w) for f, w in zip(frames, want))


# ------------------------------------------------------------------ the two reference calls in either memory space
@pytest.mark.parametrize("w,h,strides", [(18, 6, (21, 20, 23, 11)), (66, 34, (80, 70, 77, 37))], ids=["18x6", "66x34"])
def test_tonemap_and_convert_yuv_give_equal_bytes_in_host_and_device_memory(hip, orc, w, h, strides):
    """uhdr_hip_tonemap and uhdr_hip_convert_yuv at a ragged layout, planes between guard bytes: MEM_HOST writes what MEM_DEVICE
    writes (which is the oracle's) and nothing else"""
    lib = hip.load()
    luma, chroma = T.lcg_planes(w, h, 31 + w)
    f = Frame(hip, luma, chroma, T.CG_709, *strides)
    assert lib.uhdr_hip_tonemap(C.byref(f.src), C.byref(f.dst), hip.MEM_DEVICE, stream_ptr()) == 0
    oy, oc = _oracle_planes(orc, f, luma, chroma)
    assert _equal_planes(f, oy, oc) and f.dst.colorGamut == T.CG_709
    pad = lambda a, s: np.ascontiguousarray(np.pad(a, ((0, 0), (0, s - a.shape[1]))))      # noqa: E731
    hl, hc = pad(luma, f.ls), pad(chroma, f.cs)
    hy, huv = np.full(f.ny + 2 * GUARD + 1, 0xCD, np.uint8), np.full(f.nc + 2 * GUARD + 1, 0xCD, np.uint8)
    lo = GUARD + 1
    src = hip.p010_image(hl.ctypes.data, w, h, T.CG_709, f.ls, f.cs, chroma_ptr=hc.ctypes.data)
    dst = hip.yuv420_image(hy.ctypes.data + lo, w, h, hip.CG_UNSPECIFIED, f.dls, f.dcs, chroma_ptr=huv.ctypes.data + lo)
    assert lib.uhdr_hip_tonemap(C.byref(src), C.byref(dst), hip.MEM_HOST, stream_ptr()) == 0
    half = f.dcs * h // 2
    assert dst.colorGamut == T.CG_709 and np.array_equal(hy[lo:lo + f.ny], oy) and np.array_equal(huv[lo:lo + 2 * half], oc[:2 * half])
    for a, nb in ((hy, f.ny), (huv, f.nc)):
        assert (a[:lo] == 0xCD).all() and (a[lo + nb:] == 0xCD).all()
    # convertYuv in place: the device's planes, the host's planes and the oracle's go through the same matrix
    for se, de in ((hip.CG_BT709, hip.CG_P3), (hip.CG_BT2100, hip.CG_BT709)):
        assert lib.uhdr_hip_convert_yuv(C.byref(f.dst), se, de, hip.MEM_DEVICE, stream_ptr()) == 0
        assert lib.uhdr_hip_convert_yuv(C.byref(dst), se, de, hip.MEM_HOST, stream_ptr()) == 0
        oimg = orc.yuv420_image(oy, w, h, se, f.dls, f.dcs, oc)
        assert orc.load().orc_convertYuv(C.byref(oimg), se, de) == 0
        assert _equal_planes(f, oy, oc)
        assert np.array_equal(hy[lo:lo + f.ny], oy) and np.array_equal(huv[lo:lo + 2 * half], oc[:2 * half])
        for a, nb in ((hy, f.ny), (huv, f.nc)):
            assert (a[:lo] == 0xCD).all() and (a[lo + nb:] == 0xCD).all()
