"""-m gpu: content-adaptive gain maps for packed RGBA inputs -- uhdr_hip_generate_gainmap_packed_adaptive_batch
and uhdr_hip_jpegr_encode_packed_adaptive_batch against the model of tests/packed_adaptive_cases.py: maps byte for byte,
content_minmax and boost_range bit for bit, guard bytes around every dest, the workspace and the two float arrays; the constant-range
packed generate given the measured metadata as a cross-check; the C++ shim against the C calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import adaptive_cases as A
from tests import packed_adaptive_cases as PA
from tests import packed_cases as P
from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
from tests.test_gpu_packed import Pair, _generate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLT_MAX = 3.4028234663852886e38
GUARD = 256
FORM_IDS = ["pq1010102", "hlg1010102", "f16"]


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _guarded(nbytes, offset=0):
    t = dev_empty(nbytes + 2 * GUARD + offset, 0xCD)
    return t, t.data_ptr() + GUARD + offset


def _inside(t, nbytes, offset=0):
    """(the bytes between the guards, guards intact)"""
    a = to_host(t)
    lo = GUARD + offset
    return a[lo:lo + nbytes].copy(), bool((a[:lo] == 0xCD).all() and (a[lo + nbytes:] == 0xCD).all())


def _pair(name, w, h, fmt, tf, pad=0, shift=0):
    sdr, hdr = PA.images(name, w, h, fmt, tf)
    return Pair(sdr, hdr, fmt, PA.GAMUTS, pad, shift)


def run(hip, pairs, tf, rgb, scope, want_minmax=True, short=0, offset=0, shared=False):
    """one uhdr_hip_generate_gainmap_packed_adaptive_batch over `pairs`, every output between guard bytes -> (status, maps,
    content_minmax, boost_range, dests, guards intact).  offset: bytes the dests lie off their 256-byte alignment.  shared: the
    descriptors of pairs[0] for every image (its inputs are uploaded once)"""
    lib, n, bpp = hip.load(), len(pairs), 4 if rgb else 1
    keep, ss, hs = [], [], []
    for k, p in enumerate(pairs):
        if not shared or k == 0:
            s, h, t = p.on_device(hip)
            keep.append(t)
        ss.append(s)
        hs.append(h)
    sizes = [bpp * (p.w // 4) * (p.h // 4) for p in pairs]
    maps = [_guarded(s, offset) for s in sizes]
    da = hip.image_array([hip.out_image(m[1]) for m in maps])
    mm, rng = _guarded(8 * n), _guarded(8 * n)
    nb = hip.packed_adaptive_workspace_bytes(ss, rgb)
    ws = _guarded(nb)
    rc = lib.uhdr_hip_generate_gainmap_packed_adaptive_batch(n, hip.image_array(ss), hip.image_array(hs), tf, da, int(rgb), scope,
                                                             C.c_void_p(mm[1]) if want_minmax else None, C.c_void_p(rng[1]), C.c_void_p(ws[1]), nb - short,
                                                             stream_ptr())
    torch.cuda.synchronize()
    out, ok = [], True
    for m, s, p in zip(maps, sizes, pairs):
        b, intact = _inside(m[0], s, offset)
        ok = ok and intact
        out.append(b.reshape(p.h // 4, p.w // 4, 4) if rgb else b.reshape(p.h // 4, p.w // 4))
    (mmb, ok1), (rngb, ok2), (_, ok3) = _inside(mm[0], 8 * n), _inside(rng[0], 8 * n), _inside(ws[0], nb)
    return rc, out, mmb.view(F), rngb.view(F), da, ok and ok1 and ok2 and ok3


def _bits(a):
    return np.asarray(a, F).tobytes()


def check(hip, named, tf, fmt, rgb, scope, **kw):
    """a call over [(input name, w, h, pad, shift)] against the model"""
    pairs = [_pair(name, w, h, fmt, tf, pad, shift) for name, w, h, pad, shift in named]
    rc, maps, mm, rng, da, ok = run(hip, pairs, tf, rgb, scope, **kw)
    assert rc == 0 and ok, (rc, ok)
    lins = [PA.nits(name, w, h, fmt, tf) for name, w, h, _, _ in named]
    stats = [PA.minmax(lin, rgb) for lin in lins]
    pooled = A.rule(tf, min(s[0] for s in stats), max(s[1] for s in stats))
    for i, ((name, w, h, _, _), lin) in enumerate(zip(named, lins)):
        lo, hi = pooled if scope == hip.BOOST_PER_CALL else A.rule(tf, *stats[i])
        assert _bits(mm[2 * i:2 * i + 2]) == _bits(stats[i]), (name, i, mm[2 * i:2 * i + 2], stats[i])
        assert _bits(rng[2 * i:2 * i + 2]) == _bits([lo, hi]), (name, i, rng[2 * i:2 * i + 2], lo, hi)
        want = PA.expected(name, w, h, fmt, tf, bool(rgb))[0] if scope == hip.BOOST_PER_IMAGE else PA.encode(lin, rgb, lo, hi)
        assert np.array_equal(maps[i], want), (name, i, int((maps[i] != want).sum()), np.argwhere(maps[i] != want)[:4])
        d = da[i]
        assert (d.width, d.height, d.luma_stride, d.colorGamut, d.pixelFormat, d.chroma_data, d.chroma_stride) == \
            (w // 4, h // 4, w // 4, hip.CG_UNSPECIFIED, hip.PIX_FMT_RGBA8888 if rgb else hip.PIX_FMT_MONOCHROME, None, 0)
    return maps, mm, rng


# ---- the batch call against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_shapes(hip, form, rgb):
    """8x8: a 2x2 map, one partial wave.  64x64 tight: the aligned form.  68x36 with data one pixel into its buffer and rows five pixels
    longer, the dest off its alignment: the element-wise form, map 17x9, a lone last pixel in every row -- which holds the image's
    maximum in its last row.  264x12: the aligned form past one block across (33 pairs a row)"""
    fmt, tf = form
    odd = 4 if rgb else 1
    check(hip, [("interior", 8, 8, 0, 0)], tf, fmt, rgb, hip.BOOST_PER_IMAGE)
    check(hip, [("interior", 64, 64, 0, 0)], tf, fmt, rgb, hip.BOOST_PER_IMAGE)
    check(hip, [("lone_max", 68, 36, 5, 1)], tf, fmt, rgb, hip.BOOST_PER_IMAGE, offset=odd)
    check(hip, [("interior", 264, 12, 0, 0)], tf, fmt, rgb, hip.BOOST_PER_IMAGE)
    check(hip, [("interior", 264, 12, 4, 0)], tf, fmt, rgb, hip.BOOST_PER_IMAGE, offset=odd)   # aligned rows, a dest that is not


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_every_input(hip, form, rgb):
    """every input of tests/packed_adaptive_cases.py in one call (two sizes: two launches of each pass); the conditions that make
    them inputs are tests/test_packed_adaptive_cpu.py's"""
    fmt, tf = form
    named = [(name,) + PA.SIZES[name] + (0, 0) for name in PA.INPUTS]
    maps, mm, rng = check(hip, named, tf, fmt, rgb, hip.BOOST_PER_IMAGE)
    i = list(PA.INPUTS).index("all_above_one")
    assert mm[2 * i] > 1.5   # no gain of 1 from the absent second pixel of a row's last pair
    # the element-wise form of the same inputs gives the same bytes
    check(hip, [(n, w, h, 3, 1) for n, w, h, _, _ in named], tf, fmt, rgb, hip.BOOST_PER_IMAGE, offset=4 if rgb else 1)


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_the_large_launch(hip, form):
    """64 descriptors of one 1024x512 interior pair, each with its own dest: the large-launch form, four spans per block.  Every dest
    and every range equals the n = 1 call's -- the small form, one span per block -- and that equals the model"""
    fmt, tf = form
    w, h = 1024, 512
    pair = _pair("interior", w, h, fmt, tf)
    for rgb in (0, 1):
        one, mm1, rng1 = check(hip, [("interior", w, h, 0, 0)], tf, fmt, rgb, hip.BOOST_PER_IMAGE)
        rc, many, mm, rng, _, ok = run(hip, [pair] * 64, tf, rgb, hip.BOOST_PER_IMAGE, shared=True)
        assert rc == 0 and ok
        for k, got in enumerate(many):
            assert np.array_equal(got, one[0]), (rgb, k)
            assert _bits(mm[2 * k:2 * k + 2]) == _bits(mm1) and _bits(rng[2 * k:2 * k + 2]) == _bits(rng1), (rgb, k)


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_per_call_scope(hip, form, rgb):
    """images of different sizes and contents in one call: one range, the rule applied to (min of minima, max of maxima), n equal
    pairs in boost_range; content_minmax stays per image.  Then a call that spans a chunk boundary: 65 images of 8x8, the last one
    -- alone in its launch -- holding both extremes of the call"""
    fmt, tf = form
    named = [("interior", 64, 64, 0, 0), ("all_above_one", 68, 36, 0, 0), ("lone_min", 68, 36, 1, 1), ("interior", 8, 8, 0, 0)]
    maps, mm, rng = check(hip, named, tf, fmt, rgb, hip.BOOST_PER_CALL)
    assert all(_bits(rng[2 * i:2 * i + 2]) == _bits(rng[0:2]) for i in range(len(named)))
    assert len({_bits(mm[2 * i:2 * i + 2]) for i in range(len(named))}) == len(named)
    # without content_minmax the call gives the same maps
    rc, maps2, _, rng2, _, ok = run(hip, [_pair(*a[:3], fmt, tf, a[3], a[4]) for a in named], tf, rgb, hip.BOOST_PER_CALL, want_minmax=False)
    assert rc == 0 and ok and all(np.array_equal(a, b) for a, b in zip(maps, maps2)) and _bits(rng2) == _bits(rng)
    for scope in (hip.BOOST_PER_IMAGE, hip.BOOST_PER_CALL):
        named = [("interior" if k % 2 else "all_above_one", 8, 8, 0, 0) for k in range(64)] + [("both_clamps", 8, 8, 0, 0)]
        _, mm, rng = check(hip, named, tf, fmt, rgb, scope)
        if scope == hip.BOOST_PER_CALL:
            assert mm[128] < mm[0:128:2].min() and rng[0] == A.rule(tf, mm[128], mm[129])[0]   # the call's lo comes from the second launch


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_cross_check_with_the_constant_range_generate(hip, form, rgb):
    """the map is what uhdr_hip_generate_gainmap_packed_batch writes when given uhdr_hip_adaptive_metadata(g_min, g_max) as metadata_in,
    both calls run here on the same inputs"""
    fmt, tf = form
    lib = hip.load()
    for name in PA.INPUTS:
        w, h = PA.SIZES[name]
        pair = _pair(name, w, h, fmt, tf)
        rc, maps, mm, rng, _, ok = run(hip, [pair], tf, rgb, hip.BOOST_PER_IMAGE)
        assert rc == 0 and ok
        md = hip.Metadata()
        assert lib.uhdr_hip_adaptive_metadata(tf, mm[0], mm[1], C.byref(md)) == 0
        assert _bits([md.minContentBoost, md.maxContentBoost]) == _bits(rng[0:2])
        rc, other, _, _ = _generate(hip, [pair], tf, md, rgb)
        assert rc == 0
        want = PA.expected(name, w, h, fmt, tf, bool(rgb))[0]
        assert np.array_equal(maps[0], want), name          # the model is the bar
        assert np.array_equal(other[0], maps[0]), (name, int((other[0] != maps[0]).sum()))


# ---- failures and capture ---------------------------------------------------------------------------------------------------------------
def test_failures_write_nothing_and_the_empty_call(hip):
    lib = hip.load()
    fmt, tf = P.FORMS[0]
    pairs = [_pair("interior", 64, 64, fmt, tf), _pair("lone_max", 68, 36, fmt, tf)]
    for rgb in (0, 1):
        for kw, want in ((dict(short=1), hip.ERROR_INSUFFICIENT_RESOURCE), (dict(scope=2), hip.ERROR_UNSUPPORTED_FEATURE), (dict(scope=-1), hip.ERROR_UNSUPPORTED_FEATURE)):
            rc, maps, mm, rng, _, ok = run(hip, pairs, tf, rgb, kw.get("scope", hip.BOOST_PER_IMAGE), short=kw.get("short", 0))
            assert rc == want and ok, (rgb, kw, rc)
            assert all((m == 0xCD).all() for m in maps) and (mm.view(np.uint8) == 0xCD).all() and (rng.view(np.uint8) == 0xCD).all()
    assert lib.uhdr_hip_generate_gainmap_packed_adaptive_batch(0, None, None, tf, None, 1, 0, None, None, None, 0, stream_ptr()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_graph_capture_and_replay_on_new_inputs(hip, rgb):
    lib = hip.load()
    fmt, tf = P.FORMS[0]
    first = [("interior", 64, 64), ("all_above_one", 64, 64), ("interior", 68, 36)]
    second = [("black", 64, 64), ("both_clamps", 64, 64), ("lone_min", 68, 36)]
    n, bpp = len(first), 4 if rgb else 1
    pairs = [_pair(nm, w, h, fmt, tf) for nm, w, h in first]
    dev = [p.on_device(hip) for p in pairs]
    ss, hs = [d[0] for d in dev], [d[1] for d in dev]
    sizes = [bpp * (w // 4) * (h // 4) for _, w, h in first]
    dmaps = [dev_empty(s, 0) for s in sizes]
    da = hip.image_array([hip.out_image(t.data_ptr()) for t in dmaps])
    rng, mm = torch.zeros(2 * n, dtype=torch.float32, device="cuda"), torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    nb = hip.packed_adaptive_workspace_bytes(ss, rgb)
    ws = dev_empty(nb, 0)
    sa, ha = hip.image_array(ss), hip.image_array(hs)
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.uhdr_hip_generate_gainmap_packed_adaptive_batch(n, sa, ha, tf, da, rgb, hip.BOOST_PER_IMAGE, C.c_void_p(mm.data_ptr()),
                                                                   C.c_void_p(rng.data_ptr()), C.c_void_p(ws.data_ptr()), nb, s) == 0
    # other content in the same buffers, then a replay: the captured chain is all there is to the call
    for d, (nm, w, h) in zip(dev, second):
        sdr, hdr = PA.images(nm, w, h, fmt, tf)
        d[2][0].copy_(to_dev(sdr))
        d[2][1].copy_(to_dev(hdr))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    r, m = rng.cpu().numpy(), mm.cpu().numpy()
    for i, (nm, w, h) in enumerate(second):
        want, stats, (lo, hi) = PA.expected(nm, w, h, fmt, tf, bool(rgb))
        assert _bits(r[2 * i:2 * i + 2]) == _bits([lo, hi]) and _bits(m[2 * i:2 * i + 2]) == _bits(stats), nm
        got = to_host(dmaps[i], sizes[i])
        assert np.array_equal(got.reshape(want.shape), want), nm


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def _tonemapped(hip, pair, tf, peak=0.0):
    """the pair of the packed API-0: the HDR image with uhdr_hip_tonemap_packed's SDR rendition of it (in the HDR image's gamut)"""
    lib = hip.load()
    hdr = np.ascontiguousarray(pair.hdr)
    sdr = np.zeros((pair.h, pair.w, 4), np.uint8)
    make = hip.rgba_f16_image if pair.fmt == P.FMT_F16 else hip.rgba1010102_image
    src = make(hdr.ctypes.data, pair.w, pair.h, pair.gamuts[1])
    dst = hip.rgba8888_image(sdr.ctypes.data, pair.w, pair.h, pair.gamuts[1])
    assert lib.uhdr_hip_tonemap_packed(C.byref(src), C.byref(dst), tf, hip.TONEMAP_REINHARD_MAXRGB, peak, None, hip.MEM_HOST, stream_ptr()) == 0
    return Pair(sdr, pair.hdr, pair.fmt, (pair.gamuts[1], pair.gamuts[1]))


def _encode_files(hip, fn_adaptive, pairs, tf, q, rgb, scope, api0, host, spoil=None, peaks=None):
    """uhdr_hip_jpegr_encode_packed_adaptive_batch (fn_adaptive) or the constant-range call of the same form over `pairs`:
    (status, statuses, files, metadata)"""
    lib, n = hip.load(), len(pairs)
    keep, ss, hs = [], [], []
    for p in pairs:
        if host:
            sa, ha = np.ascontiguousarray(p.sdr), np.ascontiguousarray(p.hdr)
            keep.append((sa, ha))
            make = hip.rgba_f16_image if p.fmt == P.FMT_F16 else hip.rgba1010102_image
            s, h = hip.rgba8888_image(sa.ctypes.data, p.w, p.h, p.gamuts[0]), make(ha.ctypes.data, p.w, p.h, p.gamuts[1])
        else:
            s, h, t = p.on_device(hip)
            keep.append(t)
        ss.append(s)
        hs.append(h)
    for k in (spoil or ()):
        hs[k].colorGamut = 7
    caps = [p.w * p.h * 6 + 65536 for p in pairs]
    outs = [np.full(c, 0xCD, np.uint8) for c in caps]
    sizes, stat, mds = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n), (hip.Metadata * n)()
    optr, cptr = _arr(C.c_void_p, [o.ctypes.data for o in outs]), _arr(C.c_size_t, caps)
    mem = hip.MEM_HOST if host else hip.MEM_DEVICE
    pk = None if peaks is None else _arr(C.c_float, peaks)
    ha, sa = hip.image_array(hs), hip.image_array(ss)
    if fn_adaptive:
        rc = lib.uhdr_hip_jpegr_encode_packed_adaptive_batch(n, ha, None if api0 else sa, tf, q, None, None, optr, cptr, sizes, mds, stat, pk, int(rgb), scope, mem,
                                                             stream_ptr())
    elif api0:
        rc = lib.uhdr_hip_jpegr_encode_packed_api0_batch(n, ha, tf, q, None, None, optr, cptr, sizes, mds, stat, hip.TONEMAP_REINHARD_MAXRGB, pk, int(rgb), mem,
                                                         stream_ptr())
    else:
        rc = lib.uhdr_hip_jpegr_encode_packed_batch(n, ha, sa, tf, q, None, None, optr, cptr, sizes, stat, int(rgb), mem, stream_ptr())
    files = [outs[k][:sizes[k]].tobytes() if stat[k] == 0 else None for k in range(n)]
    untouched = [bool((outs[k] == 0xCD).all()) for k in range(n)]
    return rc, list(stat), files, mds, untouched


def _parts(hip, data):
    """(primary JPEG, its ICC profile, the gain-map JPEG) of a JPEG/R file, both JPEGs from their first DQT on: the segments in front
    -- EXIF, XMP, ICC, MPF; the map's XMP with the range -- are the container's"""
    lib = hip.load()
    b = np.frombuffer(data, np.uint8)
    pi, gi = hip.JpegInfo(), hip.JpegInfo()
    assert lib.uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(pi), C.byref(gi)) == 0
    primary = data[pi.offset:pi.offset + pi.size]
    gm = data[gi.offset:gi.offset + gi.size]
    return primary[primary.index(b"\xff\xdb"):], data[pi.icc_offset:pi.icc_offset + pi.icc_size], gm[gm.index(b"\xff\xdb"):]


def _map_jpeg(hip, gmap, rgb):
    """the gain-map JPEG of a map, from its first DQT on: quality 85 through the plain encoders, as the JPEG/R calls compress it"""
    lib = hip.load()
    if rgb:
        from tests.test_gpu_rgbmap import _encode_rgb
        rc, _, _, files = _encode_rgb(hip, [gmap], [85], True)
        assert rc == 0
        return files[0][files[0].index(b"\xff\xdb"):]
    plane = np.ascontiguousarray(gmap)
    out, sz = np.zeros(plane.size * 2 + 4096, np.uint8), C.c_size_t()
    img = hip.mono_image(plane.ctypes.data, plane.shape[1], plane.shape[0])
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), 85, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(sz), hip.MEM_HOST, None) == 0
    jpg = out[:sz.value].tobytes()
    return jpg[jpg.index(b"\xff\xdb"):]


@pytest.mark.parametrize("api0", [False, True], ids=["pair", "api0"])
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("scope", [0, 1], ids=["per_image", "per_call"])
@pytest.mark.parametrize("rgb", [0, 1], ids=["oneplane", "rgbmap"])
def test_files(hip, orc, api0, host, scope, rgb):
    """two files of 64x64 and 72x40 around one that fails its checks: the primary JPEG and the ICC profile are the constant-range
    call's, the gain-map JPEG is the batch call's map through the plain encoder, the XMP and metadata[i] carry the range, the failing
    file leaves its slot alone"""
    lib = hip.load()
    fmt, tf = P.FORMS[0] if rgb == scope else P.FORMS[2]   # PQ RGBA1010102 and F16, each in both forms of the map and both scopes
    pairs = [_pair("interior", 64, 64, fmt, tf), _pair("clamped", 64, 64, fmt, tf), _pair("lone_max", 72, 40, fmt, tf)]
    peaks = [0.0, 0.0, 700.0] if api0 else None
    rc, stat, files, mds, untouched = _encode_files(hip, True, pairs, tf, 90, rgb, scope, api0, host, spoil=[1], peaks=peaks)
    assert rc == hip.ERROR_INVALID_COLORGAMUT and stat == [0, hip.ERROR_INVALID_COLORGAMUT, 0] and untouched[1] and mds[1].maxContentBoost == 0
    crc, cstat, cfiles, _, _ = _encode_files(hip, False, pairs, tf, 90, rgb, scope, api0, host, spoil=[1], peaks=peaks)
    assert (crc, cstat) == (rc, stat)
    good = [0, 2]
    gen = [_tonemapped(hip, pairs[k], tf, peaks[k]) if api0 else pairs[k] for k in good]
    rc, maps, mm, rng, _, ok = run(hip, gen, tf, rgb, scope)
    assert rc == 0 and ok
    for j, k in enumerate(good):
        primary, icc, gm = _parts(hip, files[k])
        cprimary, cicc, _ = _parts(hip, cfiles[k])
        assert primary == cprimary and icc == cicc and len(icc) > 0, k
        assert gm == _map_jpeg(hip, maps[j], rgb), k
        md = mds[k]
        assert _bits([md.minContentBoost, md.maxContentBoost]) == _bits(rng[2 * j:2 * j + 2]), (k, md.minContentBoost, md.maxContentBoost, rng)
        assert A.metadata_tuple(md) == (b"1.0", md.maxContentBoost, md.minContentBoost, 1.0, 0.0, 0.0, md.minContentBoost, md.maxContentBoost)
        got, b = hip.Metadata(), np.frombuffer(files[k], np.uint8)
        assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(b.ctypes.data), b.size, C.byref(got)) == 0
        assert A.metadata_tuple(got) == A.metadata_tuple(A.xmp_round_trip(orc, hip, md))
    if scope == hip.BOOST_PER_CALL:
        assert _bits(rng[0:2]) == _bits(rng[2:4])


@pytest.mark.parametrize("api0", [False, True], ids=["pair", "api0"])
def test_per_call_over_more_than_one_round(hip, api0):
    """65 files of 8x8, PER_CALL: two rounds, so every round is measured before any map is encoded -- one range, the one the batch
    call gives for the 65 pairs at once; the last file, alone in the second round, holds both extremes"""
    fmt, tf = P.FORMS[0]
    pairs = [_pair("interior" if k % 2 else "all_above_one", 8, 8, fmt, tf) for k in range(64)] + [_pair("both_clamps", 8, 8, fmt, tf)]
    rc, stat, files, mds, _ = _encode_files(hip, True, pairs, tf, 90, 0, hip.BOOST_PER_CALL, api0, False)
    assert rc == 0 and stat == [0] * 65
    uniq = {}
    for p in pairs:   # (three distinct contents: tone-map each once)
        uniq.setdefault(id(p.sdr), _tonemapped(hip, p, tf) if api0 else p)
    gen = [uniq[id(p.sdr)] for p in pairs]
    rc, maps, mm, rng, _, ok = run(hip, gen, tf, 0, hip.BOOST_PER_CALL)
    assert rc == 0 and ok
    assert api0 or mm[128] < mm[0:128:2].min()   # the call's lo comes from the second round (a tone-mapped SDR image leaves every minimum near 1)
    for k in range(65):
        assert _bits([mds[k].minContentBoost, mds[k].maxContentBoost]) == _bits(rng[0:2]), k
    for k in (0, 1, 64):
        assert _parts(hip, files[k])[2] == _map_jpeg(hip, maps[k], 0), k


def test_a_decoded_adaptive_file_is_closer_to_the_source(hip):
    """uhdr_hip_jpegr_decode_md_batch on an interior file: mean |log2(recovered HDR luminance / source HDR luminance)| over the map's
    pixels, the recovered luminance the 4x4 block mean of the decoded linear image times the file's display boost times 203"""
    from tests.test_gpu_rgbmap import _jpegr_decode
    lib = hip.load()
    fmt, tf = P.FORMS[0]
    w, h = PA.SIZES["interior"]
    pair = _pair("interior", w, h, fmt, tf)
    _, _, ys, yh = PA.nits("interior", w, h, fmt, tf)
    err = {}
    for name, adaptive in (("adaptive", True), ("constant", False)):
        rc, stat, files, mds, _ = _encode_files(hip, adaptive, [pair], tf, 95, 0, hip.BOOST_PER_IMAGE, False, False)
        assert rc == 0 and stat == [0]
        rc, stat, got, dests, dmd = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, files, hip.OUTPUT_HDR_LINEAR, hip.APPLY_FAST, True)
        assert rc == 0 and stat == [0] and (dests[0].width, dests[0].height) == (w, h)
        lin = got[0].view(np.float16).reshape(h, w, 4)[:, :, :3].astype(np.float64) * float(dmd[0].maxContentBoost)
        lum = (0.2126 * lin[:, :, 0] + 0.7152 * lin[:, :, 1] + 0.0722 * lin[:, :, 2]) * 203.0
        rec = lum.reshape(h // 4, 4, w // 4, 4).mean(axis=(1, 3))
        err[name] = float(np.abs(np.log2(rec / yh.astype(np.float64))).mean())
    print("interior PQ file, mean |log2 error| of the decoded HDR luminance: adaptive %.5f, constant range %.5f" % (err["adaptive"], err["constant"]))
    assert err["adaptive"] < err["constant"]


# ---- the C++ shim -----------------------------------------------------------------------------------------------------------------------
def test_the_shim_gives_the_c_calls_bytes(hip, tmp_path):
    """JpegRHip::encodeJPEGRPacked with setContentBoost(PER_IMAGE) is the C call's file, with -1 today's; the free
    generateGainMapPackedAdaptive gives the batch call's map and range (tests/cpp/shim_packed_adaptive_test.cpp)"""
    exe = str(tmp_path / "shim_packed_adaptive_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # device memory for the free function: the HIP runtime's C API, no device code
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_packed_adaptive_test.cpp"), "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip",
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    w, h = 72, 40
    for (fmt, tf), name in ((P.FORMS[0], "pq"), (P.FORMS[2], "f16")):
        pair = _pair("interior", w, h, fmt, tf)
        np.ascontiguousarray(pair.sdr).tofile(str(tmp_path / "in.rgba"))
        np.ascontiguousarray(pair.hdr).tofile(str(tmp_path / "in.hdr"))
        r = subprocess.run([exe, str(tmp_path / "in.rgba"), str(tmp_path / "in.hdr"), str(w), str(h), "f16" if fmt == P.FMT_F16 else "1010102", str(tf),
                            str(tmp_path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        rd = lambda n: open(tmp_path / n, "rb").read()   # noqa: E731
        per_image = hip.BOOST_PER_IMAGE
        assert rd("const.jpgr") == _encode_files(hip, False, [pair], tf, 90, 0, 0, False, True)[2][0], name
        assert rd("const0.jpgr") == _encode_files(hip, False, [pair], tf, 90, 0, 0, True, True, peaks=[0.0])[2][0], name
        assert rd("img.jpgr") == _encode_files(hip, True, [pair], tf, 90, 0, per_image, False, True)[2][0], name
        assert rd("img_rgb.jpgr") == _encode_files(hip, True, [pair], tf, 90, 1, per_image, False, True)[2][0], name
        assert rd("api0.jpgr") == _encode_files(hip, True, [pair], tf, 90, 0, per_image, True, True, peaks=[600.0])[2][0], name
        assert rd("img.jpgr") != rd("const.jpgr")
        for rgb, stem in ((0, "one"), (1, "rgb")):
            rc, maps, mm, rng, _, ok = run(hip, [pair], tf, rgb, per_image)
            assert rc == 0 and ok and rd(stem + ".map") == maps[0].tobytes() and rd(stem + ".range") == _bits(rng[0:2]), (name, stem)
