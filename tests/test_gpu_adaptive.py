"""-m gpu: content-adaptive gain maps on the device (uhdr_hip_generate_gainmap_adaptive_batch, uhdr_hip_jpegr_encode_adaptive_batch,
uhdr_hip_eval_transfer fn 60, the shim's two additions) against tests/adaptive_cases.py -- the reference's per-pixel primitives and
three-argument encodeGain through the CPU oracle.  Maps byte for byte, statistics and ranges bit for bit."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import adaptive_cases as A
from tests.gpu_util import dev_empty, diff_1010102, stream_ptr, to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLT_MAX = 3.4028234663852886e38
GUARD = 256


class Pair:
    """one (P010, YUV420) pair in a given memory layout, on the host (for the oracle) and on the device"""

    def __init__(self, orc, hip, p010, yuv, w, h, sdr_gamut, hdr_gamut, stride=None, offset=0):
        ls = stride or w
        self.w, self.h, self.sdr_gamut, self.hdr_gamut = w, h, sdr_gamut, hdr_gamut
        plane = lambda a, rows, cols, st: np.pad(a.reshape(rows, cols), ((0, 0), (0, st - cols))).reshape(-1)
        # P010: luma rows of ls words, the interleaved chroma plane apart; YUV: luma rows of ls bytes, U then V rows of ls / 2
        self.hy, self.huv = plane(p010[:w * h], h, w, ls), plane(p010[w * h:], h // 2, w, ls)
        self.y = plane(yuv[:w * h], h, w, ls)
        self.uv = np.concatenate([plane(yuv[w * h:w * h * 5 // 4], h // 2, w // 2, ls // 2), plane(yuv[w * h * 5 // 4:], h // 2, w // 2, ls // 2)])
        self.oyuv = orc.yuv420_image(self.y, w, h, sdr_gamut, ls, ls // 2, chroma=self.uv)
        self.op010 = orc.p010_image(self.hy, w, h, hdr_gamut, ls, ls, chroma=self.huv)
        dev = lambda a: to_dev(np.concatenate([np.zeros(offset, np.uint8), a.view(np.uint8)]))
        self.keep = [dev(self.hy), dev(self.huv), dev(self.y), dev(self.uv)]
        ptr = [t.data_ptr() + offset for t in self.keep]
        self.dyuv = hip.yuv420_image(ptr[2], w, h, sdr_gamut, ls, ls // 2, chroma_ptr=ptr[3])
        self.dp010 = hip.p010_image(ptr[0], w, h, hdr_gamut, ls, ls, chroma_ptr=ptr[1])
        self._lum = {}

    def lum(self, orc, tf, sdr601):
        if (tf, sdr601) not in self._lum:
            self._lum[tf, sdr601] = A.luminances(orc, self.oyuv, self.op010, tf, sdr601)
        return self._lum[tf, sdr601]


def _guarded(nbytes):
    t = dev_empty(nbytes + 2 * GUARD, 0xCD)
    return t, t.data_ptr() + GUARD


def _guards_intact(t, nbytes):
    a = to_host(t)
    return bool((a[:GUARD] == 0xCD).all() and (a[GUARD + nbytes:] == 0xCD).all())


def run_adaptive(hip, pairs, tf, sdr601, scope, want_minmax=True, short=0):
    """one uhdr_hip_generate_gainmap_adaptive_batch over `pairs`, every output between guard bytes -> (status, maps, content_minmax,
    boost_range, dests, guards intact)"""
    lib, n = hip.load(), len(pairs)
    ya, pa = hip.image_array([p.dyuv for p in pairs]), hip.image_array([p.dp010 for p in pairs])
    sizes = [(p.w // 4) * (p.h // 4) for p in pairs]
    maps = [_guarded(s) for s in sizes]
    da = hip.image_array([hip.out_image(m[1]) for m in maps])
    mm, rng = _guarded(8 * n), _guarded(8 * n)
    nb = hip.adaptive_workspace_bytes([p.dyuv for p in pairs])
    ws = _guarded(nb)
    rc = lib.uhdr_hip_generate_gainmap_adaptive_batch(n, ya, pa, tf, da, int(sdr601), scope, C.c_void_p(mm[1]) if want_minmax else None,
                                                      C.c_void_p(rng[1]), C.c_void_p(ws[1]), nb - short, stream_ptr())
    torch.cuda.synchronize()
    ok = all(_guards_intact(m[0], s) for m, s in zip(maps, sizes)) and _guards_intact(mm[0], 8 * n) and _guards_intact(rng[0], 8 * n) and \
        _guards_intact(ws[0], nb)
    out = [to_host(m[0])[GUARD:GUARD + s].reshape(p.h // 4, p.w // 4) for m, s, p in zip(maps, sizes, pairs)]
    return rc, out, to_host(mm[0])[GUARD:GUARD + 8 * n].view(F).copy(), to_host(rng[0])[GUARD:GUARD + 8 * n].view(F).copy(), da, ok


def check_call(orc, hip, pairs, tf, sdr601, scope):
    rc, maps, mm, rng, da, ok = run_adaptive(hip, pairs, tf, sdr601, scope)
    assert rc == 0 and ok, (rc, ok)
    stats = [A.minmax(*p.lum(orc, tf, sdr601)) for p in pairs]
    pooled = A.rule(tf, min(s[0] for s in stats), max(s[1] for s in stats))
    for i, p in enumerate(pairs):
        ys, yh = p.lum(orc, tf, sdr601)
        lo, hi = pooled if scope == hip.BOOST_PER_CALL else A.rule(tf, *stats[i])
        assert (mm[2 * i].tobytes(), mm[2 * i + 1].tobytes()) == (stats[i][0].tobytes(), stats[i][1].tobytes()), (i, mm[2 * i:2 * i + 2], stats[i])
        assert (rng[2 * i].tobytes(), rng[2 * i + 1].tobytes()) == (lo.tobytes(), hi.tobytes()), (i, rng[2 * i:2 * i + 2], lo, hi)
        want = A.encode(orc, ys, yh, lo, hi)
        assert np.array_equal(maps[i], want), (i, int((maps[i] != want).sum()))
        d = da[i]
        assert (d.width, d.height, d.luma_stride, d.colorGamut, d.pixelFormat, d.chroma_data, d.chroma_stride) == \
            (p.w // 4, p.h // 4, p.w // 4, hip.CG_UNSPECIFIED, hip.PIX_FMT_MONOCHROME, None, 0)
    return maps, mm, rng


def _contents(orc, hip, seed):
    """the content classes of the issue at 136 x 72 and smaller, in the three gamut pairs; the 260 x 132 pair in the unaligned class
    (luma stride 272, chroma planes apart, every base pointer 2 bytes off)"""
    lcg = lambda w, h, s: orc.lcg_frame(w, h, s)
    black_sdr = lcg(136, 72, seed + 3)
    black_sdr[1][:136 * 72] = 0
    black_sdr[1][136 * 72:] = 128
    return [
        Pair(orc, hip, *lcg(8, 8, seed), 8, 8, A.CG_709, A.CG_709),
        Pair(orc, hip, *lcg(136, 72, seed + 1), 136, 72, A.CG_709, A.CG_2100),
        Pair(orc, hip, *A.graded_pair(orc, 136, 72), 136, 72, A.CG_2100, A.CG_2100),
        Pair(orc, hip, *lcg(260, 132, seed + 2), 260, 132, A.CG_P3, A.CG_2100, stride=272, offset=2),
        Pair(orc, hip, *A.flat_pair(136, 72, 500, 128), 136, 72, A.CG_709, A.CG_709),          # flat grey: every pixel on a clamp
        Pair(orc, hip, *A.flat_pair(136, 72, 64, 128), 136, 72, A.CG_709, A.CG_2100),          # HDR black over mid-grey SDR: g = 0
        Pair(orc, hip, *black_sdr, 136, 72, A.CG_709, A.CG_2100),                              # y_sdr = 0: gain := 1
        Pair(orc, hip, *lcg(136, 72, seed + 4), 136, 72, A.CG_P3, A.CG_2100),
    ]


@pytest.fixture(scope="module")
def contents(orc, hip):
    return _contents(orc, hip, 11)


@pytest.mark.parametrize("tf,sdr601", [(A.TF_HLG, False), (A.TF_PQ, False), (A.TF_LINEAR, True), (A.TF_PQ, True), (A.TF_HLG, True)])
def test_maps_statistics_and_ranges_equal_the_helper(orc, hip, contents, tf, sdr601):
    maps, mm, rng = check_call(orc, hip, contents, tf, sdr601, hip.BOOST_PER_IMAGE)
    if tf == A.TF_PQ and not sdr601:
        assert rng[2] == F(0.25) and rng[3] == A.cap(tf) and mm[2] < 0.25 and mm[3] > A.cap(tf)   # the LCG pair hits both clamps of the rule
        assert maps[1].min() == 0 and maps[1].max() >= 254
    if tf == A.TF_HLG and not sdr601:
        assert rng[4] == F(1.0)                          # graded: lo clamps to 1
        assert len(np.unique(maps[4])) == 1              # flat grey: one byte
        assert mm[10] == 0.0 and rng[10] == F(0.25) and (maps[5] == 0).all()    # HDR black
        assert mm[12] == 1.0 and mm[13] == 1.0 and rng[12] == F(1.0) and rng[13] == F(1.0625) and (maps[6] == 0).all()   # black SDR


def test_several_images_per_launch_and_a_chunk_boundary_inside_the_call(orc, hip):
    pairs = [Pair(orc, hip, *orc.lcg_frame(1024, 512, 21 + i), 1024, 512, A.CG_709, A.CG_2100) for i in range(3)]
    pairs.append(Pair(orc, hip, *orc.lcg_frame(512, 256, 25), 512, 256, A.CG_709, A.CG_2100))
    check_call(orc, hip, pairs, A.TF_HLG, False, hip.BOOST_PER_IMAGE)


def test_per_call_scope_pools_the_statistic(orc, hip, contents):
    four = [contents[1], contents[2], contents[4], contents[5]]
    maps, mm, rng = check_call(orc, hip, four, A.TF_PQ, False, hip.BOOST_PER_CALL)
    assert all(rng[2 * i].tobytes() == rng[0].tobytes() and rng[2 * i + 1].tobytes() == rng[1].tobytes() for i in range(4))
    assert len({mm[2 * i].tobytes() for i in range(4)}) > 1          # content_minmax stays per image
    # without content_minmax the call gives the same maps
    rc, maps2, _, rng2, _, ok = run_adaptive(hip, four, A.TF_PQ, False, hip.BOOST_PER_CALL, want_minmax=False)
    assert rc == 0 and ok and all(np.array_equal(a, b) for a, b in zip(maps, maps2)) and rng2.tobytes() == rng.tobytes()


def test_fn60_is_the_log2_constant(hip):
    lib = hip.load()
    rs = np.random.RandomState(5)
    one = (np.arange(1 << 13, dtype=np.uint32) + F(1.0).view(np.uint32)).view(F)        # every float of [1, 1 + 2^-10)
    quarter = (np.arange(1 << 13, dtype=np.uint32) + F(0.25).view(np.uint32)).view(F)   # ... and of [0.25, 0.25 (1 + 2^-10))
    x = np.concatenate([rs.uniform(0.25, 49.27, 1 << 20).astype(F), one, quarter, [A.cap(A.TF_HLG), A.cap(A.TF_PQ)]]).astype(F)
    assert one[-1] < F(1.0) + F(2.0 ** -10) and quarter[-1] < F(0.25) * (F(1.0) + F(2.0 ** -10))
    dx, dy = to_dev(x), dev_empty(4 * x.size, 0)
    assert lib.uhdr_hip_eval_transfer(60, C.c_void_p(dx.data_ptr()), C.c_void_p(dy.data_ptr()), x.size, 1.0, 4.0, stream_ptr()) == 0
    got = to_host(dy, 4 * x.size, F)
    want = np.array([math.log2(float(v)) for v in x], np.float64).astype(F)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, x[bad[:4]], got[bad[:4]], want[bad[:4]])


def test_workspace_too_small_and_empty_call(hip, contents):
    lib = hip.load()
    rc, maps, mm, rng, _, ok = run_adaptive(hip, contents[:2], A.TF_HLG, False, hip.BOOST_PER_IMAGE, short=1)
    assert rc == hip.ERROR_INSUFFICIENT_RESOURCE and ok
    assert all((m == 0xCD).all() for m in maps) and (mm.view(np.uint8) == 0xCD).all() and (rng.view(np.uint8) == 0xCD).all()
    n = C.c_size_t(5)
    assert lib.uhdr_hip_generate_adaptive_workspace_bytes(0, None, C.byref(n)) == 0 and n.value == 0
    assert hip.adaptive_workspace_bytes([p.dyuv for p in contents[:2]]) >= 4 * (2 * 2 + 34 * 18)
    assert lib.uhdr_hip_generate_gainmap_adaptive_batch(0, None, None, 1, None, 0, 0, None, None, None, 0, stream_ptr()) == 0


def test_graph_capture_and_replay_on_new_inputs(orc, hip):
    lib, w, h, n = hip.load(), 136, 72, 3
    first = [Pair(orc, hip, *orc.lcg_frame(w, h, 40 + i), w, h, A.CG_709, A.CG_2100) for i in range(n)]
    ya, pa = hip.image_array([p.dyuv for p in first]), hip.image_array([p.dp010 for p in first])
    msz = (w // 4) * (h // 4)
    dmaps = [dev_empty(msz, 0) for _ in range(n)]
    da = hip.image_array([hip.out_image(t.data_ptr()) for t in dmaps])
    rng, mm = torch.zeros(2 * n, dtype=torch.float32, device="cuda"), torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    nb = hip.adaptive_workspace_bytes([p.dyuv for p in first])
    ws = dev_empty(nb, 0)
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.uhdr_hip_generate_gainmap_adaptive_batch(n, ya, pa, A.TF_PQ, da, 0, hip.BOOST_PER_IMAGE, C.c_void_p(mm.data_ptr()),
                                                            C.c_void_p(rng.data_ptr()), C.c_void_p(ws.data_ptr()), nb, s) == 0
    # other content in the same buffers, then a replay: the captured chain is all there is to the call
    second = [Pair(orc, hip, *orc.lcg_frame(w, h, 50 + i), w, h, A.CG_709, A.CG_2100) for i in range(n)]
    for a, b in zip(first, second):
        for ta, tb in zip(a.keep, b.keep):
            ta.copy_(tb)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    r = rng.cpu().numpy()
    for i, p in enumerate(second):
        ys, yh = p.lum(orc, A.TF_PQ, False)
        lo, hi = A.rule(A.TF_PQ, *A.minmax(ys, yh))
        assert (r[2 * i], r[2 * i + 1]) == (lo, hi)
        assert np.array_equal(to_host(dmaps[i], msz).reshape(h // 4, w // 4), A.encode(orc, ys, yh, lo, hi))


@pytest.mark.parametrize("tf", [A.TF_HLG, A.TF_PQ])
def test_apply_of_an_adaptive_map_with_its_metadata(orc, hip, contents, tf):
    lib, p = hip.load(), contents[1]
    rc, maps, mm, rng, _, ok = run_adaptive(hip, [p], tf, False, hip.BOOST_PER_IMAGE)
    assert rc == 0 and ok
    md = hip.Metadata()
    assert lib.uhdr_hip_adaptive_metadata(tf, mm[0], mm[1], C.byref(md)) == 0
    assert (F(md.minContentBoost), F(md.maxContentBoost)) == (rng[0], rng[1])
    omd = orc.Metadata(md.maxContentBoost, md.minContentBoost, 1.0, 0.0, 0.0, md.hdrCapacityMin, md.hdrCapacityMax, 1)
    gmap = np.ascontiguousarray(maps[0])
    st, ref, _ = orc.apply("orc_", p.oyuv, gmap, omd, orc.OUT_HDR_HLG, FLT_MAX)
    assert st == 0
    dmap = to_dev(gmap)
    from tests.gpu_util import gpu_apply
    # (apply's fast path wants packed planes: the pair is packed, 136 x 72)
    st, out, _ = gpu_apply(lib, p.dyuv, dmap, p.w // 4, p.h // 4, md, hip.OUTPUT_HDR_HLG, FLT_MAX, hip.APPLY_EXACT)
    assert st == 0 and np.array_equal(out, ref)
    st, out, _ = gpu_apply(lib, p.dyuv, dmap, p.w // 4, p.h // 4, md, hip.OUTPUT_HDR_HLG, FLT_MAX, hip.APPLY_FAST)
    worst, _, alpha_ok = diff_1010102(out.view(np.uint32), ref.view(np.uint32))
    assert st == 0 and alpha_ok and worst <= 1, worst


# ---- files -------------------------------------------------------------------------------------------------------------------

def _packed(orc, w, h, seed, graded=False):
    return A.graded_pair(orc, w, h) if graded else orc.lcg_frame(w, h, seed)


def _jpeg_decode(lib, hip, data):
    b = np.frombuffer(data, np.uint8)
    out, desc = np.zeros(1 << 20, np.uint8), hip.Image()
    assert lib.uhdr_hip_jpeg_decode(C.c_void_p(b.ctypes.data), b.size, C.c_void_p(out.ctypes.data), out.size, C.byref(desc), hip.MEM_HOST, None) == 0
    return out[:desc.width * desc.height].copy(), desc.width, desc.height


def _after_container_segments(jpg):
    """a primary JPEG from its first DQT on: the segments in front (EXIF, the XMP with the gain map's length, ICC, MPF with its offsets)
    name the second image, whose size is not the same in the two files"""
    return jpg[jpg.index(b"\xff\xdb"):]


@pytest.mark.parametrize("api0", [False, True])
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("scope", [0, 1])
def test_adaptive_files(orc, hip, api0, host, scope):
    lib, tf, q = hip.load(), A.TF_PQ, 90
    shapes = [(64, 48, 61, False), (136, 72, 0, True), (64, 48, 63, False)]
    raw = [_packed(orc, w, h, s, g) for (w, h, s, g) in shapes]
    n = len(raw)
    sdr_gamut, hdr_gamut = (A.CG_2100 if api0 else A.CG_709), A.CG_2100
    keep = [(to_dev(p), to_dev(y)) for p, y in raw]
    ptr = lambda i, k: (raw[i][k].ctypes.data if host else keep[i][k].data_ptr())
    pimgs = [hip.p010_image(ptr(i, 0), w, h, hdr_gamut) for i, (w, h, _, _) in enumerate(shapes)]
    yimgs = [hip.yuv420_image(ptr(i, 1), w, h, sdr_gamut) for i, (w, h, _, _) in enumerate(shapes)]
    # a fourth file that fails its checks (odd width) sits between the others
    order = [0, 1, None, 2]
    bad = hip.p010_image(ptr(0, 0), 63, 48, hdr_gamut)
    pa = hip.image_array([bad if i is None else pimgs[i] for i in order])
    ya = None if api0 else hip.image_array([yimgs[0] if i is None else yimgs[i] for i in order])
    m = len(order)
    cap = 1 << 18
    bufs = [np.zeros(cap, np.uint8) for _ in range(m)]
    outs, caps = (C.c_void_p * m)(*[b.ctypes.data for b in bufs]), (C.c_size_t * m)(*([cap] * m))
    sizes, status, mds = (C.c_size_t * m)(), (C.c_int * m)(), (hip.Metadata * m)()
    mem = hip.MEM_HOST if host else hip.MEM_DEVICE
    rc = lib.uhdr_hip_jpegr_encode_adaptive_batch(m, pa, ya, tf, q, None, None, outs, caps, sizes, mds, status, scope, mem, stream_ptr())
    assert rc == hip.ERROR_UNSUPPORTED_WIDTH_HEIGHT and list(status) == [0, 0, hip.ERROR_UNSUPPORTED_WIDTH_HEIGHT, 0]
    # the constant-range batch on the same inputs
    cbufs = [np.zeros(cap, np.uint8) for _ in range(m)]
    couts, csizes, cstatus = (C.c_void_p * m)(*[b.ctypes.data for b in cbufs]), (C.c_size_t * m)(), (C.c_int * m)()
    lib.uhdr_hip_jpegr_encode_batch(m, pa, ya, tf, q, None, None, couts, caps, csizes, cstatus, mem, stream_ptr())
    assert list(cstatus) == list(status)
    # the maps and ranges the device-level call gives for the same pairs (API-0: on toneMap's SDR rendition)
    pairs = []
    for i, (w, h, _, _) in enumerate(shapes):
        p010, yuv = raw[i]
        if api0:
            yuv = np.zeros_like(yuv)
            assert orc.load().orc_toneMap(C.byref(orc.p010_image(p010, w, h, hdr_gamut)), C.byref(orc.yuv420_image(yuv, w, h, hdr_gamut))) == 0
        pairs.append(Pair(orc, hip, p010, yuv, w, h, sdr_gamut, hdr_gamut))
    rc, maps, mm, rng, _, ok = run_adaptive(hip, pairs, tf, False, scope)
    assert rc == 0 and ok
    for slot, i in enumerate(order):
        if i is None:
            continue
        data = bufs[slot][:sizes[slot]].tobytes()
        b = np.frombuffer(data, np.uint8)
        w, h = shapes[i][0], shapes[i][1]
        md = mds[slot]
        assert (F(md.minContentBoost), F(md.maxContentBoost)) == (rng[2 * i], rng[2 * i + 1]), (slot, md.minContentBoost, md.maxContentBoost, rng)
        assert A.metadata_tuple(md) == (b"1.0", md.maxContentBoost, md.minContentBoost, 1.0, 0.0, 0.0, md.minContentBoost, md.maxContentBoost)
        got = hip.Metadata()
        assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(b.ctypes.data), b.size, C.byref(got)) == 0
        assert A.metadata_tuple(got) == A.metadata_tuple(A.xmp_round_trip(orc, hip, md))
        pi, gi, cpi = hip.JpegInfo(), hip.JpegInfo(), hip.JpegInfo()
        assert lib.uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(pi), C.byref(gi)) == 0
        cdata = cbufs[slot][:csizes[slot]].tobytes()
        cb = np.frombuffer(cdata, np.uint8)
        assert lib.uhdr_hip_jpegr_info(C.c_void_p(cb.ctypes.data), cb.size, C.byref(cpi), None) == 0
        assert _after_container_segments(data[pi.offset:pi.offset + pi.size]) == _after_container_segments(cdata[cpi.offset:cpi.offset + cpi.size])
        assert data[pi.icc_offset:pi.icc_offset + pi.icc_size] == cdata[cpi.icc_offset:cpi.icc_offset + cpi.icc_size] and pi.icc_size > 0
        # the gain-map JPEG against the device-level map through the plain encoder at quality 85
        gm = np.ascontiguousarray(maps[i]).reshape(-1)
        jbuf, jn = np.zeros(1 << 16, np.uint8), C.c_size_t()
        img = hip.mono_image(gm.ctypes.data, w // 4, h // 4)
        assert lib.uhdr_hip_jpeg_encode(C.byref(img), 85, None, 0, C.c_void_p(jbuf.ctypes.data), jbuf.size, C.byref(jn), hip.MEM_HOST, None) == 0
        want_plane = _jpeg_decode(lib, hip, jbuf[:jn.value].tobytes())
        got_plane = _jpeg_decode(lib, hip, data[gi.offset:gi.offset + gi.size])
        assert got_plane[1:] == want_plane[1:] == (w // 4, h // 4) and np.array_equal(got_plane[0], want_plane[0])
        # decodeJPEGR reports the file's metadata
        dout, ddesc, dmd = np.zeros(w * h * 8, np.uint8), hip.Image(), hip.Metadata()
        assert lib.uhdr_hip_jpegr_decode(C.c_void_p(b.ctypes.data), b.size, hip.OUTPUT_HDR_LINEAR, FLT_MAX, C.c_void_p(dout.ctypes.data), dout.size,
                                         C.byref(ddesc), C.byref(dmd), hip.APPLY_EXACT, hip.MEM_HOST, stream_ptr()) == 0
        assert A.metadata_tuple(dmd) == A.metadata_tuple(got) and (ddesc.width, ddesc.height) == (w, h)
    if scope == 1:
        assert len({(mds[s].minContentBoost, mds[s].maxContentBoost) for s in (0, 1, 3)}) == 1
    if api0 or host or scope:
        return
    # the size probe and a buffer one byte short, as in the existing batch: the size is reported, the other files are written
    caps2 = (C.c_size_t * m)(cap, 0, cap, sizes[3] - 1)
    outs2 = (C.c_void_p * m)(bufs[0].ctypes.data, None, bufs[2].ctypes.data, bufs[3].ctypes.data)
    sizes2, status2 = (C.c_size_t * m)(), (C.c_int * m)()
    first = bufs[0][:sizes[0]].copy()
    rc = lib.uhdr_hip_jpegr_encode_adaptive_batch(m, pa, ya, tf, q, None, None, outs2, caps2, sizes2, None, status2, scope, mem, stream_ptr())
    cs2, cst2 = (C.c_size_t * m)(), (C.c_int * m)()
    lib.uhdr_hip_jpegr_encode_batch(m, pa, ya, tf, q, None, None, outs2, caps2, cs2, cst2, mem, stream_ptr())
    assert status2[0] == 0 and status2[1] == cst2[1] and status2[2] == cst2[2] and status2[3] == hip.ERROR_INSUFFICIENT_RESOURCE
    assert sizes2[3] == sizes[3] and sizes2[0] == sizes[0]
    assert status2[1] != 0 and (status2[1] != hip.ERROR_INSUFFICIENT_RESOURCE or sizes2[1] == sizes[1])


def test_per_call_over_more_than_one_round(orc, hip):
    """66 small files, PER_CALL: more than one round of 64, so the statistic of both rounds is taken before any map is encoded --
    every file carries the range of the pooled extremes, which is what the device-level call gives for the 66 pairs at once"""
    lib, tf, w, h, n = hip.load(), A.TF_PQ, 16, 8, 66
    raw = [orc.lcg_frame(w, h, 200 + i) for i in range(n)]
    raw[65] = A.flat_pair(w, h, 64, 200)          # the last file, alone in the second round, holds the call's minimum (g = 0)
    pairs = [Pair(orc, hip, p, y, w, h, A.CG_709, A.CG_2100) for p, y in raw]
    pa, ya = hip.image_array([p.dp010 for p in pairs]), hip.image_array([p.dyuv for p in pairs])
    cap = 1 << 14
    bufs = [np.zeros(cap, np.uint8) for _ in range(n)]
    outs, caps = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*([cap] * n))
    sizes, status, mds = (C.c_size_t * n)(), (C.c_int * n)(), (hip.Metadata * n)()
    assert lib.uhdr_hip_jpegr_encode_adaptive_batch(n, pa, ya, tf, 90, None, None, outs, caps, sizes, mds, status, hip.BOOST_PER_CALL, hip.MEM_DEVICE,
                                                    stream_ptr()) == 0
    rc, maps, mm, rng, _, ok = run_adaptive(hip, pairs, tf, False, hip.BOOST_PER_CALL)
    assert rc == 0 and ok and rng[0] == F(0.25) and mm[2 * 65] == 0.0
    for i in range(n):
        assert status[i] == 0 and (F(mds[i].minContentBoost), F(mds[i].maxContentBoost)) == (rng[0], rng[1]), i
    # the maps too: file 0's gain-map JPEG is the plain encoder's of the device-level map
    b = np.frombuffer(bufs[0][:sizes[0]].tobytes(), np.uint8)
    pi, gi = hip.JpegInfo(), hip.JpegInfo()
    assert lib.uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(pi), C.byref(gi)) == 0
    gm = np.ascontiguousarray(maps[0]).reshape(-1)
    jbuf, jn = np.zeros(1 << 14, np.uint8), C.c_size_t()
    img = hip.mono_image(gm.ctypes.data, w // 4, h // 4)
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), 85, None, 0, C.c_void_p(jbuf.ctypes.data), jbuf.size, C.byref(jn), hip.MEM_HOST, None) == 0
    assert np.array_equal(_jpeg_decode(lib, hip, bufs[0][gi.offset:gi.offset + gi.size].tobytes())[0], _jpeg_decode(lib, hip, jbuf[:jn.value].tobytes())[0])


def test_shim_additions(hip, tmp_path):
    """UltraHdrHip::generateGainMapAdaptive and JpegRHip::setContentBoost from a C++ program (tests/cpp/shim_adaptive_test.cpp), on
    the reference's 1280x720 fixture pair; the program checks its results against the C-ABI calls itself"""
    exe = str(tmp_path / "shim_adaptive_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_adaptive_test.cpp"), "-o", exe,
                           "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    g = os.path.join(ROOT, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "raw_p010_image.p010"), os.path.join(g, "raw_yuv420_image.yuv420")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
