"""-m gpu: the chunks of the gain-map batch calls.  A batch call cuts its image list into chunks -- up to 64 consecutive images of
equal size, gamuts and alignment class (apply over RGBA maps: and equal map stride) share a launch -- and every entry point forms its
chunks by the same rule.  One call per entry point whose list crosses every break rule the call has; the assertion is that every
image's output bytes and returned descriptor are those of the same image passed alone (n == 1) to the same entry point, between
sentinel bytes that survive.  The single calls are pinned to the oracle by the suites of their features; this carries that pin to
every position in a chunk.

The lists (16 x 8 and 24 x 16 images: maps of 4 x 2 and 6 x 4 pixels):
  generate   65 equal images (chunks of 64 and 1; image 64 is a chunk of its own, its statistics land at index 64), a size change,
             an SDR gamut change, an HDR gamut change, a size change back, then aligned -> unaligned -> aligned at equal size (a plane
             pointer moved by 4 bytes: the 16-byte forms of the kernels do not apply)
  apply      65 equal images, a size change and back, then for the one-plane call aligned -> unaligned -> aligned (the destination
             moved by 8 bytes), for the calls over RGBA maps map rows of width, width + 2 and width pixels
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
SLOT = 256          # every plane and every output starts at a multiple of SLOT (plus its shift) in one device allocation
SENTINEL = 0xCD
TF_HLG = 1
# gamma 2.2, both offsets 1 / 64, a range of [0.5, 6] and a capacity range of [1, 4]: nothing of it is what the reference accepts
MD_CASE = (2.2, 1 / 64, 1 / 64, 0.5, 6.0, 1.0, 4.0)
LIMIT = 65          # one image more than a chunk holds


class Arena:
    """byte ranges in one device allocation: reserve() hands out offsets, upload() moves the bytes in one copy"""

    def __init__(self):
        self.size, self.parts = 0, []

    def reserve(self, nbytes, shift=0, data=None):
        """nbytes at a SLOT-aligned offset + shift, GUARD bytes free on both sides; returns the offset"""
        off = self.size + SLOT + shift
        self.size = (off + nbytes + GUARD + SLOT - 1) // SLOT * SLOT
        if data is not None:
            self.parts.append((off, np.ascontiguousarray(data).view(np.uint8).reshape(-1)))
        return off

    def upload(self):
        from tests.gpu_util import to_dev
        host = np.full(self.size + SLOT, SENTINEL, np.uint8)
        for off, b in self.parts:
            host[off:off + b.size] = b
        self.dev = to_dev(host)
        self.base = self.dev.data_ptr()
        assert self.base % SLOT == 0
        return self


def _fields(d):
    return (d.width, d.height, d.colorGamut, d.chroma_data, d.luma_stride, d.chroma_stride, d.pixelFormat)


class Outputs:
    """the outputs of one list, laid out once and allocated twice -- for the batch call and for the single calls --, so that an
    output has the same alignment in both"""

    def __init__(self, sizes, shifts):
        self.arena = Arena()
        self.sizes = sizes
        self.offs = [self.arena.reserve(n, s) for n, s in zip(sizes, shifts)]

    def alloc(self):
        from tests.gpu_util import dev_empty
        t = dev_empty(self.arena.size + SLOT, SENTINEL)
        assert t.data_ptr() % SLOT == 0
        return t

    def check(self, batch, single, what):
        from tests.gpu_util import to_host
        b, s = to_host(batch), to_host(single)
        keep = np.ones(b.size, bool)
        for k, (off, n) in enumerate(zip(self.offs, self.sizes)):
            keep[off:off + n] = False
            assert np.array_equal(b[off:off + n], s[off:off + n]), (what, "image", k, int((b[off:off + n] != s[off:off + n]).sum()))
            assert (s[off:off + n] != SENTINEL).any(), (what, "image", k, "nothing written")
        assert (b[keep] == SENTINEL).all() and (s[keep] == SENTINEL).all(), (what, "bytes outside the outputs were written")


def _descriptors_agree(hip, outs, tb, ts, dests, singles, what):
    for k, (d, e) in enumerate(zip(dests, singles)):
        assert _fields(d) == _fields(e), (what, "image", k, _fields(d), _fields(e))
        assert d.data == tb.data_ptr() + outs.offs[k] and e.data == ts.data_ptr() + outs.offs[k], (what, "image", k)


# ---- generate ------------------------------------------------------------------------------------------------------------------------

def _generate_list():
    """(w, h, sdr gamut, hdr gamut, shift of the first plane in bytes)"""
    a, b = (16, 8, 0, 2, 0), (24, 16, 0, 2, 0)
    return [a] * LIMIT + [b, (24, 16, 1, 2, 0), (24, 16, 1, 1, 0), a, (16, 8, 0, 2, 4), a]


@pytest.fixture(scope="module")
def planar(hip):
    """the generate list as 4:2:0 + P010 pairs in device memory: (list, yuv descriptors, p010 descriptors, arena)"""
    rng = np.random.default_rng(2024)
    ar, spec, ys, ps = Arena(), _generate_list(), [], []
    offs = []
    for w, h, sg, hg, shift in spec:
        y = rng.integers(0, 256, w * h, dtype=np.uint8)
        uv = rng.integers(0, 256, w * h // 2, dtype=np.uint8)
        hy = (rng.integers(0, 1024, w * h, dtype=np.uint16) << 6).astype(np.uint16)
        huv = (rng.integers(0, 1024, w * h // 2, dtype=np.uint16) << 6).astype(np.uint16)
        offs.append((ar.reserve(y.size, shift, y), ar.reserve(uv.size, 0, uv), ar.reserve(hy.size * 2, 0, hy), ar.reserve(huv.size * 2, 0, huv)))
    ar.upload()
    for (w, h, sg, hg, shift), (oy, ou, ohy, ohuv) in zip(spec, offs):
        ys.append(hip.yuv420_image(ar.base + oy, w, h, sg, chroma_ptr=ar.base + ou))
        ps.append(hip.p010_image(ar.base + ohy, w, h, hg, chroma_ptr=ar.base + ohuv))
    return spec, ys, ps, ar


@pytest.fixture(scope="module")
def packed(hip):
    """the generate list as RGBA8888 + RGBA1010102 pairs"""
    rng = np.random.default_rng(2025)
    ar, spec, sd, hd, offs = Arena(), _generate_list(), [], [], []
    for w, h, sg, hg, shift in spec:
        offs.append((ar.reserve(4 * w * h, shift, rng.integers(0, 1 << 32, w * h, dtype=np.uint32)),
                     ar.reserve(4 * w * h, 0, rng.integers(0, 1 << 32, w * h, dtype=np.uint32))))
    ar.upload()
    for (w, h, sg, hg, shift), (os_, oh) in zip(spec, offs):
        sd.append(hip.rgba8888_image(ar.base + os_, w, h, sg))
        hd.append(hip.rgba1010102_image(ar.base + oh, w, h, hg))
    return spec, sd, hd, ar


def _run_generate(hip, spec, first, second, call, scale=4, bpp=1, extra=None):
    """call(n, firsts, seconds, dests, k, extra pointers) over the whole list and over every image alone.  extra: the bytes per image
    of the call's further device outputs (statistics): runs of n records between SLOT sentinel bytes; the single call of image k
    receives the address of record k"""
    from tests.gpu_util import dev_empty, to_host
    n = len(spec)
    outs = Outputs([bpp * (w // scale) * (h // scale) for w, h, _, _, _ in spec], [0] * n)
    tb, ts = outs.alloc(), outs.alloc()
    eb = [(nb, dev_empty(2 * SLOT + n * nb, SENTINEL), dev_empty(2 * SLOT + n * nb, SENTINEL)) for nb in (extra or [])]
    dests = hip.image_array([hip.out_image(tb.data_ptr() + o) for o in outs.offs])
    assert call(n, hip.image_array(first), hip.image_array(second), dests, 0, [C.c_void_p(t.data_ptr() + SLOT) for _, t, _ in eb]) == 0
    singles = []
    for k in range(n):
        d = hip.image_array([hip.out_image(ts.data_ptr() + outs.offs[k])])
        ptrs = [C.c_void_p(t.data_ptr() + SLOT + k * nb) for nb, _, t in eb]
        assert call(1, hip.image_array(first[k:k + 1]), hip.image_array(second[k:k + 1]), d, k, ptrs) == 0, k
        singles.append(d[0])
    return outs, tb, ts, dests, singles, [(nb, to_host(b, 2 * SLOT + n * nb).copy(), to_host(s, 2 * SLOT + n * nb).copy()) for nb, b, s in eb]


def _runs_agree(n, runs, what):
    """a run of n records behind SLOT bytes of sentinel: equal in both allocations, nothing written around it"""
    for nb, b, s in runs:
        lo, hi = SLOT, SLOT + n * nb
        assert np.array_equal(b[lo:hi], s[lo:hi]), (what, np.flatnonzero(b[lo:hi] != s[lo:hi])[:8] // nb)
        for k in range(n):
            assert (b[lo + k * nb:lo + (k + 1) * nb] != SENTINEL).any(), (what, "record", k, "not written")
        assert (b[:lo] == SENTINEL).all() and (b[hi:] == SENTINEL).all() and (s[:lo] == SENTINEL).all() and (s[hi:] == SENTINEL).all(), what


def test_generate_batch_ex_with_statistics(hip, planar):
    spec, ys, ps, _ = planar
    lib = hip.load()
    from tests.gpu_util import stream_ptr

    def call(n, y, p, d, k, ex):
        md = hip.Metadata()
        return lib.uhdr_hip_generate_gainmap_batch_ex(n, y, p, TF_HLG, C.byref(md), d, 0, hip.GENERATE_EXACT, ex[0], stream_ptr())
    outs, tb, ts, dests, singles, runs = _run_generate(hip, spec, ys, ps, call, extra=[8])
    outs.check(tb, ts, "batch_ex")
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "batch_ex")
    _runs_agree(len(spec), runs, "content_minmax")   # (image 64's pair at index 64: the second chunk's statistics start there)
    assert _fields(dests[0]) == (4, 2, hip.CG_UNSPECIFIED, None, 4, 0, hip.PIX_FMT_MONOCHROME)


def test_generate_rgb_batch(hip, planar):
    spec, ys, ps, _ = planar
    lib = hip.load()
    from tests.gpu_util import stream_ptr

    def call(n, y, p, d, k, ex):
        md = hip.Metadata()
        return lib.uhdr_hip_generate_gainmap_rgb_batch(n, y, p, TF_HLG, C.byref(md), d, 0, stream_ptr())
    outs, tb, ts, dests, singles, _ = _run_generate(hip, spec, ys, ps, call, bpp=4)
    outs.check(tb, ts, "rgb_batch")
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "rgb_batch")
    assert _fields(dests[0]) == (4, 2, hip.CG_UNSPECIFIED, None, 4, 0, hip.PIX_FMT_RGBA8888)


@pytest.mark.parametrize("rgb", [0, 1])
def test_generate_md_batch(hip, planar, rgb):
    spec, ys, ps, _ = planar
    lib = hip.load()
    from tests.gpu_util import stream_ptr
    g, os_, oh, lo, hi, hmin, hmax = MD_CASE
    md = hip.Metadata(b"1.0", hi, lo, g, os_, oh, hmin, hmax)

    def call(n, y, p, d, k, ex):
        return lib.uhdr_hip_generate_gainmap_md_batch(n, y, p, TF_HLG, C.byref(md), d, 0, rgb, stream_ptr())
    outs, tb, ts, dests, singles, _ = _run_generate(hip, spec, ys, ps, call, bpp=4 if rgb else 1)
    outs.check(tb, ts, "md_batch rgb=%d" % rgb)
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "md_batch")
    assert _fields(dests[0])[-1] == (hip.PIX_FMT_RGBA8888 if rgb else hip.PIX_FMT_MONOCHROME)


def test_generate_packed_batch(hip, packed):
    spec, sd, hd, _ = packed
    lib = hip.load()
    from tests.gpu_util import stream_ptr

    def call(n, a, b, d, k, ex):
        md = hip.Metadata()
        return lib.uhdr_hip_generate_gainmap_packed_batch(n, a, b, TF_HLG, None, C.byref(md), d, 0, stream_ptr())
    outs, tb, ts, dests, singles, _ = _run_generate(hip, spec, sd, hd, call)
    outs.check(tb, ts, "packed_batch")
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "packed_batch")
    assert _fields(dests[0]) == (4, 2, hip.CG_UNSPECIFIED, None, 4, 0, hip.PIX_FMT_MONOCHROME)


def test_generate_scaled_batch_factor_2(hip, planar):
    spec, ys, ps, _ = planar
    lib = hip.load()
    from tests.gpu_util import stream_ptr

    def call(n, y, p, d, k, ex):
        return lib.uhdr_hip_generate_gainmap_scaled_batch(n, y, p, TF_HLG, None, None, d, 0, 0, 2, stream_ptr())
    outs, tb, ts, dests, singles, _ = _run_generate(hip, spec, ys, ps, call, scale=2)
    outs.check(tb, ts, "scaled_batch")
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "scaled_batch")
    assert _fields(dests[0]) == (8, 4, hip.CG_UNSPECIFIED, None, 8, 0, hip.PIX_FMT_MONOCHROME)
    assert _fields(dests[LIMIT])[:2] == (12, 8)


def test_generate_adaptive_batch_per_image(hip, planar):
    spec, ys, ps, _ = planar
    lib = hip.load()
    from tests.gpu_util import dev_empty, stream_ptr
    keep = []

    def call(n, y, p, d, k, ex):
        nb = hip.adaptive_workspace_bytes(list(y))
        ws = dev_empty(nb + 256, SENTINEL)
        keep.append(ws)
        assert ws.data_ptr() % 16 == 0
        return lib.uhdr_hip_generate_gainmap_adaptive_batch(n, y, p, TF_HLG, d, 0, hip.BOOST_PER_IMAGE, ex[0], ex[1], C.c_void_p(ws.data_ptr()), nb, stream_ptr())
    outs, tb, ts, dests, singles, runs = _run_generate(hip, spec, ys, ps, call, extra=[8, 8])
    outs.check(tb, ts, "adaptive_batch")
    _descriptors_agree(hip, outs, tb, ts, dests, singles, "adaptive_batch")
    _runs_agree(len(spec), runs, "content_minmax / boost_range")


# ---- apply ---------------------------------------------------------------------------------------------------------------------------

FMT_HLG = 3   # UHDR_HIP_OUTPUT_HDR_HLG: RGBA1010102, 4 bytes per pixel


def _apply_list(rgba):
    """(w, h, map stride in pixels, shift of the destination in bytes)"""
    a, b = (16, 8, 4, 0), (24, 16, 6, 0)
    tail = [(16, 8, 4, 0), (16, 8, 6, 0), (16, 8, 4, 0)] if rgba else [a, (16, 8, 4, 8), a]
    return [a] * LIMIT + [b, a] + tail


def _apply_inputs(hip, rgba):
    rng = np.random.default_rng(2026 + int(rgba))
    ar, spec, offs, ys, ms = Arena(), _apply_list(rgba), [], [], []
    for w, h, mstride, _ in spec:
        mh = h // 4
        offs.append((ar.reserve(w * h, 0, rng.integers(0, 256, w * h, dtype=np.uint8)), ar.reserve(w * h // 2, 0, rng.integers(0, 256, w * h // 2, dtype=np.uint8)),
                     ar.reserve(mstride * mh * (4 if rgba else 1), 0, rng.integers(0, 256, mstride * mh * (4 if rgba else 1), dtype=np.uint8))))
    ar.upload()
    for (w, h, mstride, _), (oy, ou, om) in zip(spec, offs):
        ys.append(hip.yuv420_image(ar.base + oy, w, h, hip.CG_BT709, chroma_ptr=ar.base + ou))
        ms.append(hip.rgba_map_image(ar.base + om, w // 4, h // 4, mstride) if rgba else hip.mono_image(ar.base + om, w // 4, h // 4))
    return spec, ys, ms, ar


@pytest.fixture(scope="module")
def mono_maps(hip):
    return _apply_inputs(hip, False)


@pytest.fixture(scope="module")
def rgba_maps(hip):
    return _apply_inputs(hip, True)


def _run_apply(hip, inputs, fn, md, mode, what):
    from tests.gpu_util import stream_ptr
    spec, ys, ms, _ = inputs
    n = len(spec)
    outs = Outputs([4 * w * h for w, h, _, _ in spec], [s for _, _, _, s in spec])
    tb, ts = outs.alloc(), outs.alloc()
    dests = hip.image_array([hip.out_image(tb.data_ptr() + o) for o in outs.offs])
    assert fn(n, hip.image_array(ys), hip.image_array(ms), C.byref(md), FMT_HLG, 4.0, dests, mode, stream_ptr()) == 0
    singles = []
    for k in range(n):
        d = hip.image_array([hip.out_image(ts.data_ptr() + outs.offs[k])])
        assert fn(1, hip.image_array(ys[k:k + 1]), hip.image_array(ms[k:k + 1]), C.byref(md), FMT_HLG, 4.0, d, mode, stream_ptr()) == 0, k
        singles.append(d[0])
    outs.check(tb, ts, what)
    _descriptors_agree(hip, outs, tb, ts, dests, singles, what)
    assert _fields(dests[0])[:3] == (16, 8, hip.CG_BT709) and _fields(dests[LIMIT])[:2] == (24, 16)


def test_apply_batch_fast(hip, mono_maps):
    _run_apply(hip, mono_maps, hip.load().uhdr_hip_apply_gainmap_batch, hip.metadata(6.0, 0.5), hip.APPLY_FAST, "apply_batch")


def test_apply_rgb_batch(hip, rgba_maps):
    _run_apply(hip, rgba_maps, hip.load().uhdr_hip_apply_gainmap_rgb_batch, hip.metadata(6.0, 0.5), hip.APPLY_FAST, "apply_rgb_batch")


def test_apply_md_batch_general_metadata(hip, rgba_maps):
    g, os_, oh, lo, hi, hmin, hmax = MD_CASE
    md = hip.Metadata(b"1.0", hi, lo, g, os_, oh, hmin, hmax)
    _run_apply(hip, rgba_maps, hip.load().uhdr_hip_apply_gainmap_md_batch, md, hip.APPLY_FAST, "apply_md_batch")
