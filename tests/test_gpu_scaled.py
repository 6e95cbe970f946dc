"""-m gpu: gain maps at any scale factor -- uhdr_hip_generate_gainmap_scaled_batch against the model of
tests/scaled_cases.py, byte for byte, and uhdr_hip_jpegr_encode_scaled_batch against the existing encode and decode calls.

The kernel's geometry (k_generate_scaled): blocks of 256 threads, one unit per thread, units in row-major order, one tile of 256
units per block (a block walks no further tiles).  A unit of the aligned forms is a strip of 8 luma columns and s rows -- 8 map
pixels at s = 1, 4 at s = 2, 1 at s = 8 --; a unit of the generic form (every other factor, every other layout) is a pair of map
pixels.  136 x 40 at s = 1 is 17 x 40 = 680 strips, three blocks; 272 x 80 is 34 x 40 = 1360 strips at s = 2, six blocks, and
34 x 10 = 340 strips at s = 8, two blocks.  A wave's doubt list covers its 64 units.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import scaled_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = 3.4028234663852886e38
GUARD = 64
pytestmark = pytest.mark.gpu


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _dev_pair(hip, p, shift=0):
    """a tests/scaled_cases.py Pair in device memory, every plane `shift` elements behind its allocation's start: (yuv, p010, keep)"""
    from tests.gpu_util import to_dev
    keep, ptr = [], []
    for a in (p.y, p.uv, p.hy, p.huv):
        flat = np.concatenate([np.full(shift, 0xA5, a.dtype), a.reshape(-1)])
        t = to_dev(flat)
        keep.append(t)
        ptr.append(t.data_ptr() + shift * a.dtype.itemsize)
    y = hip.yuv420_image(ptr[0], p.w, p.h, p.sdr_gamut, luma_stride=p.ls, chroma_stride=p.cs, chroma_ptr=ptr[1])
    q = hip.p010_image(ptr[2], p.w, p.h, p.hdr_gamut, luma_stride=p.ls, chroma_stride=p.ls, chroma_ptr=ptr[3])
    return y, q, keep


def _generate(hip, pairs, tf, s, rgb=False, case=None, sdr_is_601=False, shift=0, map_shift=0, stream=None):
    """one uhdr_hip_generate_gainmap_scaled_batch call: (status, maps, metadata used, dests).  The maps are carved between GUARD bytes
    that must survive"""
    from tests import gainmap_md_cases as MD
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    bpp = 4 if rgb else 1
    keep, ys, ps, outs = [], [], [], []
    for p in pairs:
        y, q, t = _dev_pair(hip, p, shift)
        keep.append(t)
        ys.append(y)
        ps.append(q)
        outs.append(dev_empty(bpp * (p.w // s) * (p.h // s) + 2 * GUARD + map_shift, 0xCD))
    dests = hip.image_array([hip.out_image(t.data_ptr() + GUARD + map_shift) for t in outs])
    md_in = None if case is None else MD.api_metadata(hip, case)
    md_out = hip.Metadata()
    rc = lib.uhdr_hip_generate_gainmap_scaled_batch(len(pairs), hip.image_array(ys), hip.image_array(ps), tf, None if md_in is None else C.byref(md_in),
                                                    C.byref(md_out), dests, int(sdr_is_601), int(rgb), s, stream_ptr() if stream is None else stream)
    maps = []
    for p, t in zip(pairs, outs):
        mw, mh = p.w // s, p.h // s
        full = to_host(t).copy()
        lo = GUARD + map_shift
        if rc == 0:
            assert (full[:lo] == 0xCD).all() and (full[lo + bpp * mw * mh:] == 0xCD).all()   # nothing written outside the map
        else:
            assert (full == 0xCD).all()                                                       # a failing call writes nothing
        m = full[lo:lo + bpp * mw * mh]
        maps.append(m.reshape(mh, mw, 4) if rgb else m.reshape(mh, mw))
    return rc, maps, md_out, dests


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


G1, G2 = (S.CG_709, S.CG_2100), (S.CG_P3, S.CG_P3)   # with a gamut matrix; without
# (w, h, s, tf, gamuts, sdr_is_601, pad, shift, map_shift)
FORMS = [
    # aligned: the 16-byte forms, at least two blocks each
    (136, 40, 1, S.TF_HLG, G1, False, 0, 0, 0),
    (272, 80, 2, S.TF_PQ, G2, False, 0, 0, 0),
    (272, 80, 8, S.TF_LINEAR, G1, False, 16, 0, 0),
    # ragged: pointers moved by one or two elements, strides above the width, an odd map width, a width the factor does not divide
    (70, 22, 1, S.TF_LINEAR, G2, False, 6, 1, 1),
    (70, 22, 2, S.TF_HLG, G1, True, 6, 2, 1),
    (86, 22, 8, S.TF_PQ, G1, False, 2, 1, 3),
    # every other factor: the generic form (odd factors straddle chroma samples)
    (50, 20, 3, S.TF_HLG, G1, False, 0, 0, 0),
    (50, 20, 5, S.TF_PQ, G2, False, 4, 1, 0),
    (64, 32, 16, S.TF_LINEAR, G1, False, 0, 0, 0),
    (256, 128, 128, S.TF_HLG, G1, False, 0, 0, 0),
]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%dx%d_s%d_tf%d_pad%d_shift%d" % (f[0], f[1], f[2], f[3], f[6], f[7]))
def test_factors_and_forms(hip, form):
    w, h, s, tf, gamuts, is601, pad, shift, map_shift = form
    seed = 100 + w + s
    p = S.pair(w, h, seed, gamuts[0], gamuts[1], pad)
    rc, maps, md, dests = _generate(hip, [p], tf, s, sdr_is_601=is601, shift=shift, map_shift=map_shift)
    assert rc == 0
    want, _ = S.expected(w, h, seed, tf, s, False, None, is601, gamuts[0], gamuts[1], pad)
    _same(maps[0], want, form)
    d = dests[0]
    assert (d.width, d.height, d.luma_stride, d.pixelFormat, d.colorGamut, d.chroma_data) == (w // s, h // s, w // s, hip.PIX_FMT_MONOCHROME, hip.CG_UNSPECIFIED, None)
    assert abs(md.maxContentBoost - (10000.0 if tf == S.TF_PQ else 1000.0) / 203.0) < 1e-4 and md.minContentBoost == 1.0 and md.gamma == 1.0


def test_three_images_of_two_sizes_in_one_call(hip):
    """two equal images share a launch (grid.x is the image), the third is a chunk of its own"""
    pairs = [S.pair(136, 40, 237), S.pair(136, 40, 31), S.pair(72, 24, 32)]
    rc, maps, _, dests = _generate(hip, pairs, S.TF_HLG, 1)
    assert rc == 0
    for k, (w, h, seed) in enumerate([(136, 40, 237), (136, 40, 31), (72, 24, 32)]):
        _same(maps[k], S.expected(w, h, seed, S.TF_HLG, 1)[0], k)
        assert (dests[k].width, dests[k].height) == (w, h)


# (w, h, s, tf, rgb, case, pad, shift, map_shift): the exact forms -- per channel, and against the caller's metadata
SELECT = [
    (72, 24, 1, S.TF_HLG, True, None, 0, 0, 0),
    (72, 24, 2, S.TF_PQ, True, None, 0, 0, 0),
    (50, 20, 3, S.TF_LINEAR, True, None, 2, 1, 4),
    (72, 24, 1, S.TF_PQ, False, S.MD_CASE, 0, 0, 0),
    (50, 20, 3, S.TF_HLG, True, S.MD_CASE, 0, 0, 0),
    (50, 20, 3, S.TF_HLG, False, S.MD_CASE, 2, 1, 1),
    (144, 32, 8, S.TF_HLG, True, S.MD_CASE, 0, 0, 0),
]


@pytest.mark.parametrize("sel", SELECT, ids=lambda c: "%dx%d_s%d_tf%d_rgb%d_md%d_shift%d" % (c[0], c[1], c[2], c[3], c[4], c[5] is not None, c[7]))
def test_arithmetic_selection(hip, sel):
    w, h, s, tf, rgb, case, pad, shift, map_shift = sel
    seed = 300 + w + s
    p = S.pair(w, h, seed, S.CG_709, S.CG_2100, pad)
    rc, maps, md, dests = _generate(hip, [p], tf, s, rgb=rgb, case=case, shift=shift, map_shift=map_shift)
    assert rc == 0
    want, v = S.expected(w, h, seed, tf, s, rgb, case, False, S.CG_709, S.CG_2100, pad)
    _same(maps[0], want, sel)
    assert dests[0].pixelFormat == (hip.PIX_FMT_RGBA8888 if rgb else hip.PIX_FMT_MONOCHROME) and (dests[0].width, dests[0].height) == (w // s, h // s)
    if case is not None:
        assert (md.gamma, md.minContentBoost, md.maxContentBoost) == (np.float32(2.2), 0.5, 6.0)


def test_misaligned_rgb_dest_is_bad_ptr(hip):
    for case in (None, S.MD_CASE):
        rc, _, _, _ = _generate(hip, [S.pair(72, 24, 5)], S.TF_HLG, 2, rgb=True, case=case, map_shift=2)
        assert rc == hip.ERROR_BAD_PTR


@pytest.mark.parametrize("w,h,s", [(136, 40, 1), (272, 80, 2)])
def test_black_sdr_frame_every_pixel_in_doubt(hip, w, h, s):
    """Y = 0, U = V = 128: the filter can decide no pixel, every wave's list holds its whole tile"""
    black = (0, 0, w, h)
    p = S.pair(w, h, 41 + s, S.CG_709, S.CG_2100, 0, black)
    rc, maps, _, _ = _generate(hip, [p], S.TF_HLG, s)
    assert rc == 0
    _same(maps[0], S.expected(w, h, 41 + s, S.TF_HLG, s, black=black)[0], (w, h, s))


@pytest.mark.parametrize("tf", [S.TF_HLG, S.TF_PQ])
def test_black_rectangle_in_noise(hip, tf):
    """136 x 40 at s = 1: rows 0 .. 5 are units 0 .. 101 -- the whole first wave and 38 units of the second"""
    black = (0, 0, 136, 6)
    p = S.pair(136, 40, 47, S.CG_709, S.CG_2100, 0, black)
    rc, maps, _, _ = _generate(hip, [p], tf, 1)
    assert rc == 0
    _same(maps[0], S.expected(136, 40, 47, tf, 1, black=black)[0], tf)


def test_probe_counts_the_pixels_in_doubt(hip):
    """uhdr_hip_generate_gainmap_scaled_probe: the call's map, and on a black SDR frame a count of every map pixel"""
    import torch
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    w, h = 136, 40
    for black, seed in (((0, 0, w, h), 42), (None, 237)):
        p = S.pair(w, h, seed, S.CG_709, S.CG_2100, 0, black)
        y, q, keep = _dev_pair(hip, p)
        t, count = dev_empty(w * h, 0xCD), torch.zeros(1, dtype=torch.int32, device="cuda")
        d = hip.out_image(t.data_ptr())
        assert lib.uhdr_hip_generate_gainmap_scaled_probe(1, C.byref(y), C.byref(q), S.TF_HLG, C.byref(d), 0, 1, None, stream_ptr()) == hip.ERROR_BAD_PTR
        assert lib.uhdr_hip_generate_gainmap_scaled_probe(1, C.byref(y), C.byref(q), S.TF_HLG, C.byref(d), 0, 4, C.c_void_p(count.data_ptr()),
                                                          stream_ptr()) == hip.ERROR_UNSUPPORTED_FEATURE
        assert lib.uhdr_hip_generate_gainmap_scaled_probe(1, C.byref(y), C.byref(q), S.TF_HLG, C.byref(d), 0, 1, C.c_void_p(count.data_ptr()), stream_ptr()) == 0
        _same(to_host(t, w * h).reshape(h, w), S.expected(w, h, seed, S.TF_HLG, 1, black=black)[0], black)
        k = int(count.item())
        # (black: gain := 1 is code value 0.0 exactly, inside the filter's band around an integer, for every pixel)
        assert (k == w * h) if black else (0 <= k <= w * h), k


def test_factor_4_is_the_three_existing_calls(hip):
    from tests import gainmap_md_cases as MD
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    w, h = 72, 40
    p = S.pair(w, h, 77)
    y, q, keep = _dev_pair(hip, p)
    mw, mh = w // 4, h // 4

    def old(fn, bpp, *tail):
        t = dev_empty(bpp * mw * mh, 0xCD)
        d = hip.out_image(t.data_ptr())
        assert fn(1, C.byref(y), C.byref(q), S.TF_HLG, *[a(d) if callable(a) else a for a in tail]) == 0
        return to_host(t, bpp * mw * mh).copy(), d
    md = hip.Metadata()
    mono, d0 = old(lib.uhdr_hip_generate_gainmap_batch, 1, C.byref(md), lambda d: C.byref(d), 0, None, stream_ptr())
    rgb, d1 = old(lib.uhdr_hip_generate_gainmap_rgb_batch, 4, C.byref(md), lambda d: C.byref(d), 0, stream_ptr())
    case = MD.api_metadata(hip, S.MD_CASE)
    mdm, d2 = old(lib.uhdr_hip_generate_gainmap_md_batch, 1, C.byref(case), lambda d: C.byref(d), 0, 0, stream_ptr())
    for want, wd, kw in ((mono, d0, {}), (rgb, d1, dict(rgb=True)), (mdm, d2, dict(case=S.MD_CASE))):
        rc, maps, _, dests = _generate(hip, [p], S.TF_HLG, 4, **kw)
        assert rc == 0 and np.array_equal(maps[0].reshape(-1), want), kw
        assert (dests[0].width, dests[0].height, dests[0].luma_stride, dests[0].pixelFormat) == (wd.width, wd.height, wd.luma_stride, wd.pixelFormat)


def test_graph_capture_and_replay(hip):
    import torch
    from tests.gpu_util import dev_empty, to_host
    lib = hip.load()
    w, h = 136, 40
    p = S.pair(w, h, 237)
    y, q, keep = _dev_pair(hip, p)
    t = dev_empty(w * h, 0xCD)
    d = hip.out_image(t.data_ptr())
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.uhdr_hip_generate_gainmap_scaled_batch(1, C.byref(y), C.byref(q), S.TF_HLG, None, None, C.byref(d), 0, 0, 1, s) == 0
    t.fill_(0xCD)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _same(to_host(t, w * h).reshape(h, w), S.expected(w, h, 237, S.TF_HLG, 1)[0], "replay")


# ---- JPEG/R files -------------------------------------------------------------------------------------------------------------------

def _encode(hip, fn, pairs, api0, tf, q, tail, caps=None):
    """one call of a JPEG/R batch encoder over device planes: (status, statuses, sizes, files); tail: the arguments between status
    and mem_space"""
    from tests.gpu_util import stream_ptr
    n = len(pairs)
    keep, ys, ps = [], [], []
    for p in pairs:
        y, p10, t = _dev_pair(hip, p)
        keep.append(t)
        ys.append(y)
        ps.append(p10)
    caps = [p.w * p.h * 8 + 65536 for p in pairs] if caps is None else caps
    outs = [np.zeros(max(c, 16), np.uint8) for c in caps]
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = fn(n, hip.image_array(ps), None if api0 else hip.image_array(ys), tf, q, None, None, _arr(C.c_void_p, [o.ctypes.data for o in outs]),
            _arr(C.c_size_t, caps), sizes, stat, *tail, hip.MEM_DEVICE, stream_ptr())
    return rc, list(stat), list(sizes), [outs[k][:sizes[k]].tobytes() if stat[k] == 0 else None for k in range(n)]


def _api0_pair(orc, p):
    """the pair API-0 generates from: the SDR planes are toneMap of the P010 image (the oracle's), in the P010 image's gamut"""
    w, h = p.w, p.h
    p010 = np.concatenate([p.hy.reshape(-1), p.huv.reshape(-1)])
    yuv = np.zeros(w * h * 3 // 2, np.uint8)
    src, dst = orc.p010_image(p010, w, h, p.hdr_gamut), orc.yuv420_image(yuv, w, h, p.hdr_gamut)
    assert orc.load().orc_toneMap(C.byref(src), C.byref(dst)) == 0
    t = S.Pair.__new__(S.Pair)
    t.w, t.h, t.sdr_gamut, t.hdr_gamut, t.ls, t.cs = w, h, p.hdr_gamut, p.hdr_gamut, w, w // 2
    t.y, t.uv, t.hy, t.huv = yuv[:w * h].reshape(h, w), yuv[w * h:].reshape(h, w // 2), p.hy, p.huv
    return t


def _mono_jpeg(hip, plane, q):
    lib = hip.load()
    mh, mw = plane.shape
    src = np.ascontiguousarray(plane)
    out, n = np.zeros(mw * mh * 3 + 4096, np.uint8), C.c_size_t()
    img = hip.mono_image(src.ctypes.data, mw, mh)
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), q, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(n), hip.MEM_HOST, None) == 0
    return out[:n.value].tobytes()


@pytest.mark.parametrize("api0", [False, True])
@pytest.mark.parametrize("rgb_map", [0, 1])
@pytest.mark.parametrize("s", [1, 2, 8, 16])
def test_jpegr_encode_scaled(hip, orc, s, rgb_map, api0):
    """the scaled call and the existing one on the same pairs: the same primary image; the gain-map JPEG is the stand-alone encode at
    quality 85 of the scaled generate call's map; the existing decode calls read the file, and what they return is the apply call's
    output on the decoded pieces"""
    from tests import rgbmap_cases as R
    from tests import test_gpu_rgbmap as G
    from tests.gpu_util import to_dev
    lib = hip.load()
    tf = S.TF_PQ if s == 2 else S.TF_HLG
    pairs = [S.pair(64, 48, 500 + s), S.pair(128, 64, 510 + s, S.CG_P3, S.CG_2100)]
    rc, stat, _, new = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, pairs, api0, tf, 90, (rgb_map, s))
    assert rc == 0 and stat == [0, 0]
    old_fn = lib.uhdr_hip_jpegr_encode_rgbmap_batch if rgb_map else lib.uhdr_hip_jpegr_encode_batch
    rc, stat, _, old = _encode(hip, old_fn, pairs, api0, tf, 90, ())
    assert rc == 0 and stat == [0, 0]
    rc, stat, _, four = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, pairs, api0, tf, 90, (rgb_map, 4))
    assert rc == 0 and four == old                       # factor 4 IS the existing call
    dec = lib.uhdr_hip_jpegr_decode_rgbmap_batch if rgb_map else lib.uhdr_hip_jpegr_decode_batch_ex
    rc, dstat, got, ddests, mds = G._jpegr_decode(hip, dec, new, R.FMT_HLG, hip.APPLY_EXACT, True)
    assert rc == 0 and dstat == [0, 0]
    for k, p in enumerate(pairs):
        (np_, ng), (op, og) = G._info(hip, new[k]), G._info(hip, old[k])
        # (the primary's XMP and MPF segments hold the gain-map JPEG's length and offset: the image is compared from its first DQT on)
        assert R.from_first_dqt(np_) == R.from_first_dqt(op) and G._metadata_of(hip, new[k]) == G._metadata_of(hip, old[k])
        buf = np.frombuffer(new[k], np.uint8)
        a, g = hip.JpegInfo(), hip.JpegInfo()
        assert lib.uhdr_hip_jpegr_info(buf.ctypes.data, buf.size, C.byref(a), C.byref(g)) == 0
        assert (a.width, a.height, g.width, g.height) == (p.w, p.h, p.w // s, p.h // s)
        src = _api0_pair(orc, p) if api0 else p
        rc, maps, _, _ = _generate(hip, [src], tf, s, rgb=bool(rgb_map))
        assert rc == 0
        if rgb_map:
            rc, st, _, files = G._encode_rgb(hip, [maps[0]], [85], True)
            assert rc == 0 and R.from_first_dqt(ng) == R.from_first_dqt(files[0]), k
        else:
            assert R.from_first_dqt(ng) == R.from_first_dqt(_mono_jpeg(hip, maps[0], 85)), k
        # the decode call's HDR output: the apply call on the decoded primary planes and the decoded map
        assert (ddests[k].width, ddests[k].height) == (p.w, p.h)
        if rgb_map:
            want = G._apply_of_the_pieces(hip, np_, ng, mds[k], R.FMT_HLG, hip.APPLY_EXACT)
        else:
            rc1, planes, d = G._jpeg_decode(hip, np_, hip.DECODE_TO_YCBCR, 0)
            rc2, mono, gd = G._jpeg_decode(hip, ng, hip.DECODE_TO_YCBCR, 0)
            assert rc1 == 0 and rc2 == 0 and (gd.width, gd.height) == (p.w // s, p.h // s)
            dev, dmap = to_dev(planes), to_dev(mono[:gd.width * gd.height])
            img = hip.yuv420_image(dev.data_ptr(), d.width, d.height, hip.CG_UNSPECIFIED)
            from tests.gpu_util import dev_empty, stream_ptr, to_host
            nbytes = hip.output_bytes(R.FMT_HLG, p.w, p.h)
            dout = dev_empty(nbytes, 0xCD)
            mimg, dest = hip.mono_image(dmap.data_ptr(), gd.width, gd.height), hip.out_image(dout.data_ptr())
            assert lib.uhdr_hip_apply_gainmap_batch(1, C.byref(img), C.byref(mimg), C.byref(mds[k]), R.FMT_HLG, FLT_MAX, C.byref(dest), hip.APPLY_EXACT,
                                                    stream_ptr()) == 0
            want = to_host(dout, nbytes).copy()
        assert np.array_equal(got[k], want), (k, int((got[k] != want).sum()))
        # ... and, beside the library's own apply call, the reference's path: the oracle's applyGainMap on the oracle's decode
        # (orc.jpeg_decode) of the file's two JPEGs under the metadata the oracle reads from the file's XMP (oracle/jpegr_oracle.py:
        # decode).  The file's metadata is the reference's degenerate form in every parametrization.  A per-channel map
        # (rgb_map = 1) is a three-component 4:4:4 JPEG, which the reference's decoder -- and orc.jpeg_decode with it -- refuses:
        # there is no reference path for those files, they stay compared with the apply call on the decoded pieces only.
        if not rgb_map:
            from oracle import jpegr_oracle as J
            ost, ref, ow, oh, _, omd = J.decode(new[k], orc.OUT_HDR_HLG, FLT_MAX)
            assert ost == 0 and (ow, oh) == (p.w, p.h) and float(np.float32(omd["max"])) == mds[k].maxContentBoost
            assert np.array_equal(got[k], ref[:got[k].size]), (k, s, "decode differs from the oracle's", int((got[k] != ref[:got[k].size]).sum()))


def test_jpegr_encode_scaled_size_probe_and_a_failing_file(hip):
    lib = hip.load()
    pairs = [S.pair(64, 48, 501)]
    rc, stat, sizes, files = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, pairs, False, S.TF_HLG, 90, (0, 2))
    assert rc == 0
    rc, stat, probe, _ = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, pairs, False, S.TF_HLG, 90, (0, 2), caps=[0])
    assert rc == hip.ERROR_INSUFFICIENT_RESOURCE and stat == [hip.ERROR_INSUFFICIENT_RESOURCE] and probe == sizes
    # 64 x 50 at s = 8 fails by itself; its neighbour's file is the one a call of its own writes
    mixed = [S.pair(64, 50, 502), S.pair(64, 48, 508)]
    rc, stat, _, files = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, mixed, False, S.TF_HLG, 90, (0, 8))
    assert rc == hip.ERROR_UNSUPPORTED_WIDTH_HEIGHT and stat == [hip.ERROR_UNSUPPORTED_WIDTH_HEIGHT, 0]
    rc, stat, _, alone = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, mixed[1:], False, S.TF_HLG, 90, (0, 8))
    assert rc == 0 and files[1] == alone[0]


# ---- the C++ shim -------------------------------------------------------------------------------------------------------------------

def test_the_shims_setter(hip, tmp_path):
    """ultrahdr::JpegRHip::setGainMapScaleFactor(2): encodeJPEGR API-1 writes the scaled call's bytes; with the factor set, an API-3
    overload answers ERROR_UNSUPPORTED_FEATURE instead of writing a factor-4 map"""
    lib = hip.load()
    exe = str(tmp_path / "shim_scaled_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_scaled_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    w, h = 72, 40
    p = S.pair(w, h, 67)
    np.concatenate([p.hy.reshape(-1), p.huv.reshape(-1)]).tofile(str(tmp_path / "in.p010"))
    np.concatenate([p.y.reshape(-1), p.uv.reshape(-1)]).tofile(str(tmp_path / "in.yuv"))
    r = subprocess.run([exe, str(tmp_path / "in.p010"), str(tmp_path / "in.yuv"), str(w), str(h), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n: open(tmp_path / n, "rb").read()   # noqa: E731
    rc, stat, _, new = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, [p], False, S.TF_HLG, 90, (0, 2))
    assert rc == 0 and rd("s2.jpgr") == new[0]
    rc, stat, _, rgb = _encode(hip, lib.uhdr_hip_jpegr_encode_scaled_batch, [p], False, S.TF_HLG, 90, (1, 2))
    assert rc == 0 and rd("s2_rgb.jpgr") == rgb[0]
    rc, stat, _, old = _encode(hip, lib.uhdr_hip_jpegr_encode_batch, [p], False, S.TF_HLG, 90, ())
    assert rc == 0 and rd("s4.jpgr") == old[0] and old[0] != new[0]
