"""uhdr_hip_apply_gainmap_packed_batch on the device (include/uhdr_hip.h).

Degenerate metadata: EXACT and EXACT_UNFILTERED give the bytes of tests/packed_apply_cases.composite -- the oracle's applyGainMap on
grey images, channel by channel -- and FAST holds every 10-bit channel within 1 code and every F16 channel within 1 half-precision
ULP of them, no channel excluded.  Every output lies between guard bytes.  The shapes are the smallest that reach each route of the
table in DESIGN.md section 4.2.5; the expected values of a shape are computed once per (format, boost).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import gainmap_md_cases as M
from tests import packed_apply_cases as P
from tests.gpu_util import dev_empty, to_dev, to_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
FILL = 0xCD

# name: (width, height, scale factor, options).  src_off / dst_off: bytes past a 16-byte boundary; pad: luma_stride = width + pad
SHAPES = {
    "4x4_s4": (4, 4, 4, {}),                        # a 1 x 1 map: every tap clamped
    "8x4_s4": (8, 4, 4, {}),
    "64x64_s4": (64, 64, 4, {}),                    # strip form
    "1032x8_s4": (1032, 8, 4, {}),                  # strip form, a second block across (258 strips)
    "64x64_s4_stride": (64, 64, 4, {"pad": 1}),     # generic form at scale 4
    "64x64_s4_src": (64, 64, 4, {"src_off": 4}),
    "64x64_s4_dst": (64, 64, 4, {"dst_off": 4}),
    "6x6_s3": (6, 6, 3, {}),
    "15x10_s5": (15, 10, 5, {}),
    "8x6_s1": (8, 6, 1, {}),
    "8x6_s2": (8, 6, 2, {}),
    "4x65540_s4": (4, 65540, 4, {}),                # both forms stride over rows beyond the grid's 65535: the second trip
}


@functools.lru_cache(maxsize=None)
def _inputs(name, channels=1):
    w, h, s, _ = SHAPES[name]
    seed = 1000 + 17 * sorted(SHAPES).index(name)
    rgba, gmap = P.lcg_rgba(w, h, seed), P.lcg_map(w // s, h // s, seed + 1, channels)
    rgba.setflags(write=False)
    gmap.setflags(write=False)
    return rgba, gmap


@functools.lru_cache(maxsize=None)
def _want(name, channels, fmt, boost):
    rgba, gmap = _inputs(name, channels)
    return P.composite(rgba, gmap, fmt, boost)


def _run(hip, items, md, fmt, boost, mode, src_off=0, dst_off=0, pad=0, map_pad=0, stream=None):
    """one call over items = [(rgba (h, w, 4), gmap (mh, mw) or (mh, mw, 3))]; -> (status, the outputs' bytes, the dests as filled).
    Every output sits GUARD bytes inside its buffer; the bytes around it must come back untouched."""
    if fmt == P.FMT_F16 and dst_off % 8:
        dst_off *= 2    # (an RGBA F16 pixel is one 8-byte store: 8 bytes past the boundary)
    keep, sdrs, maps, outs = [], [], [], []
    for rgba, gmap in items:
        h, w = rgba.shape[:2]
        src = np.full((h, w + pad, 4), 0xEE, np.uint8)
        src[:, :w] = rgba
        ds = to_dev(np.concatenate([np.full(src_off, 0xEE, np.uint8), src.reshape(-1)]))
        sdrs.append(hip.rgba8888_image(ds.data_ptr() + src_off, w, h, hip.CG_P3, w + pad))
        if gmap.ndim == 2:
            dm = to_dev(gmap)
            maps.append(hip.mono_image(dm.data_ptr(), gmap.shape[1], gmap.shape[0]))
        else:
            mh, mw = gmap.shape[:2]
            m4 = np.full((mh, mw + map_pad, 4), 0xEE, np.uint8)
            m4[:, :mw, :3] = gmap[:, :, :3]
            dm = to_dev(m4)
            maps.append(hip.rgba_map_image(dm.data_ptr(), mw, mh, mw + map_pad))
        nbytes = hip.output_bytes(fmt, w, h)
        do = dev_empty(GUARD + dst_off + nbytes + GUARD, FILL)
        outs.append((do, nbytes))
        keep += [ds, dm]
    n = len(items)
    dests = hip.image_array([hip.out_image(do.data_ptr() + GUARD + dst_off) for do, _ in outs]) if n else None
    s = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    rc = hip.load().uhdr_hip_apply_gainmap_packed_batch(n, hip.image_array(sdrs) if n else None, hip.image_array(maps) if n else None, C.byref(md), fmt,
                                                        boost, dests, mode, s)
    got = []
    for do, nbytes in outs:
        raw = to_host(do)
        lo = GUARD + dst_off
        assert (raw[:lo] == FILL).all() and (raw[lo + nbytes:] == FILL).all(), "bytes outside the output were written"
        got.append(raw[lo:lo + nbytes].copy())
    del keep
    return rc, got, dests


def _check_degenerate(hip, name, channels, rgba, gmap, want_of, opts):
    md = hip.metadata(P.CONTENT_BOOST)
    for fmt in P.FORMATS:
        for boost in P.BOOSTS:
            want = want_of(fmt, boost)
            for mode in (hip.APPLY_EXACT, hip.APPLY_EXACT_UNFILTERED):
                rc, got, dests = _run(hip, [(rgba, gmap)], md, fmt, boost, mode, **opts)
                assert rc == 0, (name, fmt, boost, mode, rc)
                assert np.array_equal(got[0], want), (name, channels, fmt, boost, mode, int((got[0] != want).sum()))
                assert (dests[0].width, dests[0].height, dests[0].colorGamut) == (rgba.shape[1], rgba.shape[0], hip.CG_P3)
            rc, got, _ = _run(hip, [(rgba, gmap)], md, fmt, boost, hip.APPLY_FAST, **opts)
            assert rc == 0
            worst, share = P.fast_distance(got[0], want, fmt, rgba.shape[1], rgba.shape[0], wrap=boost < P.CONTENT_BOOST)
            print("%s maps=%d fmt=%d boost=%g: FAST worst %d, differing share %.2e" % (name, channels, fmt, boost, worst, share))
            assert worst <= 1, (name, channels, fmt, boost, worst)
            if fmt in (P.FMT_PQ, P.FMT_HLG):
                assert (got[0].view(np.uint32) >> 30 == 3).all()
            elif fmt == P.FMT_F16:
                assert (got[0].view(np.uint16).reshape(-1, 4)[:, 3] == 0x3C00).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_one_plane_map(hip, name):
    rgba, gmap = _inputs(name)
    _check_degenerate(hip, name, 1, rgba, gmap, lambda fmt, boost: _want(name, 1, fmt, boost), SHAPES[name][3])


@pytest.mark.parametrize("name", ["64x64_s4", "15x10_s5"])
def test_rgba_maps(hip, name):
    rgba, gmap = _inputs(name, 3)
    _check_degenerate(hip, name, 3, rgba, gmap, lambda fmt, boost: _want(name, 3, fmt, boost), SHAPES[name][3])


def test_rgba_map_with_a_padded_stride(hip):
    rgba, gmap = _inputs("64x64_s4", 3)
    _check_degenerate(hip, "64x64_s4", 3, rgba, gmap, lambda fmt, boost: _want("64x64_s4", 3, fmt, boost), {"map_pad": 3})


@pytest.mark.parametrize("opts", [{}, {"pad": 1}], ids=["strip", "generic"])
def test_every_code_and_every_map_byte(hip, opts):
    """64 x 64 whose three channels each take all 256 codes over a 16 x 16 map that takes all 256 bytes: the whole table"""
    rgba, gmap = P.all_codes_rgba(), P.all_codes_map()
    assert all(len(np.unique(rgba[:, :, c])) == 256 for c in range(3)) and len(np.unique(gmap)) == 256
    want = functools.lru_cache(maxsize=None)(lambda fmt, boost: P.composite(rgba, gmap, fmt, boost))
    _check_degenerate(hip, "all codes", 1, rgba, gmap, want, opts)


def test_three_different_images_in_one_call(hip):
    names = ["64x64_s4", "15x10_s5", "8x6_s2"]
    items = [_inputs(n) for n in names]
    md = hip.metadata(P.CONTENT_BOOST)
    for fmt in P.FORMATS:
        for boost in P.BOOSTS:
            rc, got, dests = _run(hip, items, md, fmt, boost, hip.APPLY_EXACT)
            assert rc == 0
            for k, n in enumerate(names):
                assert np.array_equal(got[k], _want(n, 1, fmt, boost)), (n, fmt, boost)
                assert (dests[k].width, dests[k].height) == SHAPES[n][:2]
            rc, got, _ = _run(hip, items, md, fmt, boost, hip.APPLY_FAST)
            assert rc == 0
            for k, n in enumerate(names):
                assert P.fast_distance(got[k], _want(n, 1, fmt, boost), fmt, SHAPES[n][0], SHAPES[n][1], boost < P.CONTENT_BOOST)[0] <= 1


def test_no_images(hip):
    rc, got, _ = _run(hip, [], hip.metadata(P.CONTENT_BOOST), hip.OUTPUT_HDR_HLG, 2.0, hip.APPLY_FAST)
    assert rc == 0 and got == []


@pytest.mark.parametrize("case", ["gamma22", "flatcap"])     # gamma != 1; offsets with a capacity range that is not the content's
@pytest.mark.parametrize("name", ["64x64_s4", "15x10_s5"])   # the strip form and the generic one
def test_general_metadata(hip, case, name):
    w, h = SHAPES[name][:2]
    md = M.api_metadata(hip, M.CASES[case])
    for channels in (1, 3):
        rgba, gmap = _inputs(name, channels)
        e, g = P.linear_sdr(rgba), M.sampled_gain_by_tables(gmap, w, h)
        for fmt in P.FORMATS:
            for boost in M.BOOSTS[case]:
                rc, fast, _ = _run(hip, [(rgba, gmap)], md, fmt, boost, hip.APPLY_FAST)
                rc2, exact, _ = _run(hip, [(rgba, gmap)], md, fmt, boost, hip.APPLY_EXACT)
                assert rc == 0 and rc2 == 0 and np.array_equal(fast[0], exact[0])
                v = M.pre_truncation(e, g, M.CASES[case], boost, fmt)
                codes = M.codes_of(fast[0], fmt, w, h)
                if fmt == P.FMT_F16:
                    worst = float(M.half_ulp_distance(codes, v).max())
                    assert worst <= 1.0, (case, name, channels, boost, worst)
                    assert (fast[0].view(np.uint16).reshape(-1, 4)[:, 3] == 0x3C00).all()
                else:
                    d = M.code_distance(codes, v)
                    assert d.max() <= 1, (case, name, channels, fmt, boost, int(d.max()))
    rc, _, _ = _run(hip, [_inputs(name)], md, hip.OUTPUT_HDR_HLG, 2.0, hip.APPLY_EXACT_UNFILTERED)
    assert rc == hip.ERROR_UNSUPPORTED_FEATURE


def test_decode_once_render_at_any_boost(hip):
    """a JPEG/R file's layers, decoded once with the existing calls, through the packed apply: byte for byte what uhdr_hip_jpegr_decode
    writes for the file in EXACT mode.  The SDR frame is grey (chroma 128), so its primary decodes to (Y, Y, Y) exactly and the planar
    path's yuvToRgb gives the packed path's pixel values"""
    from oracle import oracle as O
    lib = hip.load()
    w, h = 64, 48
    p010, yuv = O.lcg_frame(w, h, 4242)
    yuv = yuv.copy()
    yuv[w * h:] = 128
    dp, dy = to_dev(p010), to_dev(yuv)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pi, yi = hip.p010_image(dp.data_ptr(), w, h, hip.CG_BT2100), hip.yuv420_image(dy.data_ptr(), w, h, hip.CG_BT709)
    fbuf, fn = np.zeros(w * h * 3 + 65536, np.uint8), C.c_size_t()
    assert lib.uhdr_hip_jpegr_encode_api1(C.byref(pi), C.byref(yi), hip.TF_HLG, 95, None, 0, C.c_void_p(fbuf.ctypes.data), fbuf.size, C.byref(fn),
                                          hip.MEM_DEVICE, s) == 0
    data = fbuf[:fn.value].copy()
    prim, gm, md = hip.JpegInfo(), hip.JpegInfo(), hip.Metadata()
    assert lib.uhdr_hip_jpegr_info(C.c_void_p(data.ctypes.data), data.size, C.byref(prim), C.byref(gm)) == 0
    assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(data.ctypes.data), data.size, C.byref(md)) == 0
    assert (prim.width, prim.height, gm.width, gm.height) == (w, h, w // 4, h // 4)
    d_rgba, d_map = dev_empty(w * h * 4, 0), dev_empty(gm.width * gm.height, 0)
    for info, to, dst in ((prim, 1, d_rgba), (gm, 2, d_map)):    # UHDR_HIP_DECODE_TO_RGBA, UHDR_HIP_DECODE_TO_YCBCR
        jp, jn = (C.c_void_p * 1)(data.ctypes.data + info.offset), (C.c_size_t * 1)(info.size)
        op, on = (C.c_void_p * 1)(dst.data_ptr()), (C.c_size_t * 1)(dst.numel())
        desc = hip.image_array([hip.out_image(0)])
        assert lib.uhdr_hip_jpeg_decode_batch_ex(1, jp, jn, to, op, on, desc, None, hip.MEM_DEVICE, s, 0) == 0
    rgba = to_host(d_rgba, w * h * 4).reshape(h, w, 4)
    assert (rgba[:, :, 0] == rgba[:, :, 1]).all() and (rgba[:, :, 0] == rgba[:, :, 2]).all()
    sdr, mp = hip.rgba8888_image(d_rgba.data_ptr(), w, h, hip.CG_BT709), hip.mono_image(d_map.data_ptr(), gm.width, gm.height)
    for fmt in (hip.OUTPUT_HDR_HLG, hip.OUTPUT_HDR_LINEAR):
        for boost in (hip.FLT_MAX, 2.0):
            nbytes = hip.output_bytes(fmt, w, h)
            ref, ddesc, dmd = dev_empty(nbytes, 0), hip.Image(), hip.Metadata()
            assert lib.uhdr_hip_jpegr_decode(C.c_void_p(data.ctypes.data), data.size, fmt, boost, C.c_void_p(ref.data_ptr()), ref.numel(), C.byref(ddesc),
                                             C.byref(dmd), hip.APPLY_EXACT, hip.MEM_DEVICE, s) == 0
            out = dev_empty(nbytes, FILL)
            dests = hip.apply_gainmap_packed([sdr], [mp], md, fmt, boost, [out.data_ptr()], hip.APPLY_EXACT, s.value)
            assert np.array_equal(to_host(out, nbytes), to_host(ref, nbytes)), (fmt, boost)
            assert (dests[0].width, dests[0].height) == (w, h)


def test_captured_into_a_graph_after_stream_reserve(hip):
    """a scale factor no call has seen (6: its weight table is uploaded by uhdr_hip_stream_reserve), then the call inside a captured
    graph on that stream, replayed once"""
    lib = hip.load()
    w, h, sf = 36, 24, 6
    rgba, gmap = P.lcg_rgba(w, h, 77), P.lcg_map(w // sf, h // sf, 78)
    md = hip.metadata(P.CONTENT_BOOST)
    ds, dm = to_dev(rgba), to_dev(gmap)
    nbytes = hip.output_bytes(hip.OUTPUT_HDR_HLG, w, h)
    out = dev_empty(GUARD + nbytes + GUARD, FILL)
    side = torch.cuda.Stream()
    s = C.c_void_p(side.cuda_stream)
    assert lib.uhdr_hip_stream_reserve(s, 0, w, h, sf) == 0
    sdr, mp = hip.rgba8888_image(ds.data_ptr(), w, h, hip.CG_BT709), hip.mono_image(dm.data_ptr(), w // sf, h // sf)
    # (torch captures in the "global" error mode: an allocation, a blocking copy or a synchronisation inside the call would end the
    # capture with an error, so a capture that succeeds is the check that the call only enqueues)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        hip.apply_gainmap_packed([sdr], [mp], md, hip.OUTPUT_HDR_HLG, 2.0, [out.data_ptr() + GUARD], hip.APPLY_EXACT,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (to_host(out) == FILL).all(), "capture must not execute the kernel"
    g.replay()
    raw = to_host(out)
    assert np.array_equal(raw[GUARD:GUARD + nbytes], P.composite(rgba, gmap, P.FMT_HLG, 2.0))
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + nbytes:] == FILL).all()
    assert lib.uhdr_hip_stream_release(s) == 0


def test_the_shim_gives_the_c_calls_bytes(hip, tmp_path):
    """ultrahdr::applyGainMapPacked (device images): one-plane and RGBA maps, EXACT and FAST"""
    exe = str(tmp_path / "shim_packed_apply_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # the HIP runtime's C API, no device code
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_packed_apply_test.cpp"), "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip",
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    w, h, sf = 64, 64, 4
    md = hip.metadata(P.CONTENT_BOOST)
    for channels in (1, 3):
        rgba, gmap = _inputs("64x64_s4", channels)
        rgba.tofile(str(tmp_path / "in.rgba"))
        m = gmap
        if channels == 3:
            m = np.full((h // sf, w // sf, 4), 0xFF, np.uint8)
            m[:, :, :3] = gmap
        m.tofile(str(tmp_path / "in.map"))
        r = subprocess.run([exe, str(tmp_path / "in.rgba"), str(tmp_path / "in.map"), str(w), str(h), str(w // sf), str(h // sf),
                            "1" if channels == 1 else "4", repr(P.CONTENT_BOOST), str(tmp_path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        for stem, fmt, mode in (("hlg_exact", P.FMT_HLG, hip.APPLY_EXACT), ("hlg_fast", P.FMT_HLG, hip.APPLY_FAST), ("f16_exact", P.FMT_F16, hip.APPLY_EXACT)):
            rc, got, _ = _run(hip, [(rgba, gmap)], md, fmt, 2.0, mode)
            assert rc == 0 and open(tmp_path / (stem + ".bin"), "rb").read() == got[0].tobytes(), (channels, stem)
        assert np.array_equal(np.fromfile(str(tmp_path / "hlg_exact.bin"), np.uint8), _want("64x64_s4", channels, P.FMT_HLG, 2.0))
