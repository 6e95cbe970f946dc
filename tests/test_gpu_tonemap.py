"""-m gpu: the tone-mapped SDR base image on the device (uhdr_hip_tonemap_sdr_batch, uhdr_hip_tonemap_sdr,
uhdr_hip_jpegr_encode_api0_tonemapped_batch, the shim's two additions) against the model of tests/tonemap_cases.py.

Planes: a sample is in doubt when the model's pre-truncation value lies within 1/256 of an integer (about 60 f32 ulps at full scale;
behind the bit-exact linearisation the device rounds under 20 times and evaluates one power -- an argued margin, not a measured one).
Samples not in doubt equal the model, samples in doubt may differ by one code, none by more.  The headroom equals the model's bit
for bit.  Guard bytes surround every destination plane; the ragged layouts carve their planes at odd addresses, the aligned layouts
(64 x 64, 1920 x 1080, the file tests) at aligned ones, which is what sends them to the ALIGNED kernel instance.  Every test prints
what it observed ("tonemap-observed ...") before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import tonemap_cases as T
from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 256


def _pad(a, stride):
    return np.pad(a, ((0, 0), (0, stride - a.shape[1])))


class Frame:
    """one P010 image on the device in a case's layout, and destination planes between guard bytes"""

    def __init__(self, hip, luma, chroma, gamut, luma_stride=None, chroma_stride=None, dst_luma_stride=None, dst_chroma_stride=None, offset=0):
        self.h, self.w = luma.shape
        w, h = self.w, self.h
        self.ls, self.cs = luma_stride or w, chroma_stride or w
        self.dls, self.dcs = dst_luma_stride or w, dst_chroma_stride or w // 2
        self.gamut, self.offset = gamut, offset
        lead = np.zeros(offset, np.uint8)
        self.keep = [to_dev(np.concatenate([lead, _pad(luma, self.ls).reshape(-1).view(np.uint8)])),
                     to_dev(np.concatenate([lead, _pad(chroma, self.cs).reshape(-1).view(np.uint8)]))]
        self.src = hip.p010_image(self.keep[0].data_ptr() + offset, w, h, gamut, self.ls, self.cs, chroma_ptr=self.keep[1].data_ptr() + offset)
        # a ragged layout has its destination planes at odd addresses; an aligned one keeps the alignment its kernel needs
        self.odd = 1 if (offset or w % 16) else 0
        self.ny, self.nc = self.dls * h, self.dcs * h   # (U rows, then V chroma_stride * height / 2 behind U)
        self.dy, self.dc = dev_empty(self.ny + 2 * GUARD + 1, 0xCD), dev_empty(self.nc + 2 * GUARD + 1, 0xCD)
        self.dst = hip.yuv420_image(self.dy.data_ptr() + GUARD + self.odd, w, h, hip.CG_UNSPECIFIED, self.dls, self.dcs,
                                    chroma_ptr=self.dc.data_ptr() + GUARD + self.odd)

    def result(self):
        """-> (Y (h, dls), U (h / 2, dcs), V, guards intact)"""
        y, c = to_host(self.dy), to_host(self.dc)
        lo, h = GUARD + self.odd, self.h
        ok = all((a[:lo] == 0xCD).all() and (a[lo + n:] == 0xCD).all() for a, n in ((y, self.ny), (c, self.nc)))
        half = self.dcs * h // 2
        return (y[lo:lo + self.ny].reshape(h, self.dls).copy(), c[lo:lo + half].reshape(h // 2, self.dcs).copy(),
                c[lo + half:lo + 2 * half].reshape(h // 2, self.dcs).copy(), bool(ok))


def frame_of(hip, case):
    luma, chroma = T.planes(case.content, case.w, case.h)
    return Frame(hip, luma, chroma, case.gamut, case.luma_stride, case.chroma_stride, case.dst_luma_stride, case.dst_chroma_stride, case.offset)


def run_batch(hip, frames, tf, peaks=None, op=T.REINHARD):
    """one uhdr_hip_tonemap_sdr_batch -> (status, headroom float32[n], its guards intact, dests)"""
    n = len(frames)
    head = dev_empty(4 * n + 2 * GUARD, 0xCD)
    sa, da = hip.image_array([f.src for f in frames]), hip.image_array([f.dst for f in frames])
    pk = None if peaks is None else (C.c_float * n)(*peaks)
    rc = hip.load().uhdr_hip_tonemap_sdr_batch(n, sa, da, tf, op, pk, C.c_void_p(head.data_ptr() + GUARD), stream_ptr())
    torch.cuda.synchronize()
    hb = to_host(head)
    ok = bool((hb[:GUARD] == 0xCD).all() and (hb[GUARD + 4 * n:] == 0xCD).all())
    return rc, hb[GUARD:GUARD + 4 * n].view(F).copy(), ok, da


def check_planes(name, frame, want):
    """the rule of the module's docstring, the zeroed padding and the guards; -> samples that differ, per plane"""
    y, u, v, ok = frame.result()
    w, h = frame.w, frame.h
    out = []
    for tag, got, plane, val, cols in (("Y", y, want["Y"], want["vy"], w), ("U", u, want["U"], want["vu"], w // 2), ("V", v, want["V"], want["vv"], w // 2)):
        differ, doubt, worst, hard = T.compare(got[:, :cols], plane, val)
        print("tonemap-observed %s %s: %d of %d samples differ (%d in doubt), worst %d, %d outside the band" % (name, tag, differ, plane.size, doubt,
                                                                                                              worst, hard))
        out.append((tag, differ, doubt, worst, hard, bool((got[:, cols:] == 0).all())))
    assert ok, "guard bytes around the destination planes were written"
    for tag, differ, doubt, worst, hard, pad_zero in out:
        assert hard == 0 and worst <= 1, (name, tag, differ, doubt, worst, hard)
        assert pad_zero, (name, tag, "padding columns not zeroed")
    return [o[1] for o in out]


@pytest.mark.parametrize("case", T.cases(), ids=repr)
def test_planes_and_headroom_equal_the_model(hip, case):
    fr = frame_of(hip, case)
    want = T.expected(case)
    if case.content == "lcg_tiled":
        # the large frame: ONE pixel decides m' and H, and it sits in a block row the measuring pass reaches only by striding (its
        # grid holds at most 512 workgroup rows) -- a pass that lost workgroups or strided rows would return the flat frame's H
        flat = T.model(*T.planes("lcg_tiled_flat", case.w, case.h), case.gamut, case.tf)
        assert want["m"] > flat["m"] and T.k_of(case.tf) > want["H"] > flat["H"] and T.peak_xy(case.w, case.h)[1] // 2 >= 512
    rc, head, ok, da = run_batch(hip, [fr], case.tf)
    print("tonemap-observed %s H: device %r model %r" % (case.name, head[0], want["H"]))
    assert rc == 0 and ok
    assert head[0].tobytes() == want["H"].tobytes(), (head[0], want["H"], want["m"])
    check_planes(case.name, fr, want)
    assert da[0].colorGamut == case.gamut


@pytest.mark.parametrize("tf", [T.TF_HLG, T.TF_PQ, T.TF_LINEAR])
def test_given_and_measured_headroom_share_a_batch(hip, tf):
    """three images of two sizes, peaks [0, 600, 0]: every image its own slot -- the brightest pixel of image 2 sits in its last row
    and column, so the measuring pass reaches the edge of its grid"""
    l0, c0 = T.planes("ramp", 64, 64)
    l1, c1 = T.planes("lcg", 64, 64)
    l2, c2 = (a.copy() for a in T.planes("ramp", 66, 34))
    T.set_pixel(l2, c2, 65, 33, 940)
    frames = [Frame(hip, l0, c0, T.CG_2100), Frame(hip, l1, c1, T.CG_2100), Frame(hip, l2, c2, T.CG_2100, 80, 70, 80, 37)]
    peaks = [0.0, 600.0, 0.0]
    wants = [T.model(l0, c0, T.CG_2100, tf), T.model(l1, c1, T.CG_2100, tf, 600.0), T.model(l2, c2, T.CG_2100, tf)]
    assert wants[2]["m"] > T.model(*T.planes("ramp", 66, 34), T.CG_2100, tf)["m"]   # the pixel set above IS the maximum
    rc, head, ok, _ = run_batch(hip, frames, tf, peaks)
    print("tonemap-observed mixed batch tf %d H: device %r model %r" % (tf, list(head), [w["H"] for w in wants]))
    assert rc == 0 and ok
    for i in range(3):
        assert head[i].tobytes() == wants[i]["H"].tobytes(), (i, head[i], wants[i]["H"])
        check_planes("mixed[%d]-tf%d" % (i, tf), frames[i], wants[i])
    assert head[1] == T.headroom(tf, F(0.0), 600.0) and head[0] != head[2]
    # peaks == NULL measures every image; a given peak of a measured value reproduces the measured planes
    rc, head_all, ok, _ = run_batch(hip, frames, tf, None)
    assert rc == 0 and ok and head_all[0] == head[0] and head_all[2] == head[2]
    assert head_all[1].tobytes() == T.model(l1, c1, T.CG_2100, tf)["H"].tobytes()


def test_shift_operator_is_tonemap_batch(hip):
    case = next(c for c in T.cases() if c.name.startswith("66x34-hlg-709-lcg"))
    a, b = frame_of(hip, case), frame_of(hip, case)
    rc, _, ok, _ = run_batch(hip, [a], case.tf, op=T.SHIFT)
    assert rc == 0 and ok
    assert hip.load().uhdr_hip_tonemap_batch(1, C.byref(b.src), C.byref(b.dst), stream_ptr()) == 0
    ra, rb = a.result(), b.result()
    assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3])) and ra[3] and rb[3]
    luma, _ = T.planes(case.content, case.w, case.h)
    assert np.array_equal(ra[0][:, :case.w], (luma >> 8).astype(np.uint8))


def test_a_failing_call_writes_nothing(hip):
    case = next(c for c in T.cases() if c.name.startswith("64x64-pq-2100-lcg"))
    frames = [frame_of(hip, case), frame_of(hip, case)]
    rc, head, ok, _ = run_batch(hip, frames, case.tf, [0.0, float("nan")])
    assert rc == hip.ERROR_UNSUPPORTED_FEATURE and ok and (head.view(np.uint8) == 0xCD).all()
    for f in frames:
        y, u, v, g = f.result()
        assert g and (y == 0xCD).all() and (u == 0xCD).all() and (v == 0xCD).all()


@pytest.mark.parametrize("name", ["66x34-pq-p3-lcg", "64x64-hlg-2100-ramp"])
def test_host_and_device_memory_give_equal_bytes(hip, name):
    """uhdr_hip_tonemap_sdr: planes in either memory space, H returned to the host"""
    case = next(c for c in T.cases() if c.name == name)
    lib, want = hip.load(), T.expected(case)
    fr = frame_of(hip, case)
    h_dev = C.c_float(-1.0)
    assert lib.uhdr_hip_tonemap_sdr(C.byref(fr.src), C.byref(fr.dst), case.tf, T.REINHARD, 0.0, C.byref(h_dev), hip.MEM_DEVICE, stream_ptr()) == 0
    y, u, v, ok = fr.result()
    assert ok and fr.dst.colorGamut == case.gamut
    luma, chroma = T.planes(case.content, case.w, case.h)
    hl, hc = _pad(luma, case.luma_stride).copy(), _pad(chroma, case.chroma_stride).copy()
    hy = np.full(case.dst_luma_stride * case.h + 2 * GUARD, 0xCD, np.uint8)
    huv = np.full(case.dst_chroma_stride * case.h + 2 * GUARD, 0xCD, np.uint8)
    src = hip.p010_image(hl.ctypes.data, case.w, case.h, case.gamut, case.luma_stride, case.chroma_stride, chroma_ptr=hc.ctypes.data)
    dst = hip.yuv420_image(hy.ctypes.data + GUARD, case.w, case.h, hip.CG_UNSPECIFIED, case.dst_luma_stride, case.dst_chroma_stride,
                           chroma_ptr=huv.ctypes.data + GUARD)
    h_host = C.c_float(-1.0)
    assert lib.uhdr_hip_tonemap_sdr(C.byref(src), C.byref(dst), case.tf, T.REINHARD, 0.0, C.byref(h_host), hip.MEM_HOST, stream_ptr()) == 0
    assert F(h_host.value).tobytes() == F(h_dev.value).tobytes() == want["H"].tobytes() and dst.colorGamut == case.gamut
    half = case.dst_chroma_stride * case.h // 2
    assert np.array_equal(hy[GUARD:-GUARD].reshape(y.shape), y)
    assert np.array_equal(huv[GUARD:GUARD + half].reshape(u.shape), u) and np.array_equal(huv[GUARD + half:GUARD + 2 * half].reshape(v.shape), v)
    assert (hy[:GUARD] == 0xCD).all() and (hy[-GUARD:] == 0xCD).all() and (huv[:GUARD] == 0xCD).all() and (huv[-GUARD:] == 0xCD).all()
    # a given peak through the single call
    assert lib.uhdr_hip_tonemap_sdr(C.byref(fr.src), C.byref(fr.dst), case.tf, T.REINHARD, 450.0, C.byref(h_dev), hip.MEM_DEVICE, stream_ptr()) == 0
    assert F(h_dev.value) == T.headroom(case.tf, F(0.0), 450.0)
    check_planes(name + "-peak450", fr, T.expected(case, 450.0))


# ------------------------------------------------------------------ files

class Files:
    """n output buffers of a batched encode"""

    def __init__(self, n, cap=1 << 18):
        self.bufs = [np.zeros(cap, np.uint8) for _ in range(n)]
        self.outs, self.caps = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs]), (C.c_size_t * n)(*([cap] * n))
        self.sizes, self.status = (C.c_size_t * n)(), (C.c_int * n)()

    def file(self, i):
        return self.bufs[i][:self.sizes[i]].tobytes()


def _packed(hip, luma, chroma, gamut):
    return Frame(hip, luma, chroma, gamut)


def _tonemapped(hip, frames, tf, q, op, peaks, scope, mds=None):
    n = len(frames)
    f = Files(n)
    pa = hip.image_array([fr.src for fr in frames])
    pk = None if peaks is None else (C.c_float * n)(*peaks)
    rc = hip.load().uhdr_hip_jpegr_encode_api0_tonemapped_batch(n, pa, tf, q, None, None, f.outs, f.caps, f.sizes, mds, f.status, op, pk, scope,
                                                                hip.MEM_DEVICE, stream_ptr())
    return rc, f


def _api1_on_tonemapped_planes(hip, frames, tf, q, peaks, scope):
    """the planes uhdr_hip_tonemap_sdr_batch wrote, given to API-1 (scope -1) or to the adaptive API-1 as the SDR images"""
    n, lib = len(frames), hip.load()
    rc, _, ok, da = run_batch(hip, frames, tf, peaks)
    assert rc == 0 and ok
    f = Files(n)
    pa = hip.image_array([fr.src for fr in frames])
    if scope < 0:
        rc = lib.uhdr_hip_jpegr_encode_batch(n, pa, da, tf, q, None, None, f.outs, f.caps, f.sizes, f.status, hip.MEM_DEVICE, stream_ptr())
    else:
        rc = lib.uhdr_hip_jpegr_encode_adaptive_batch(n, pa, da, tf, q, None, None, f.outs, f.caps, f.sizes, None, f.status, scope, hip.MEM_DEVICE,
                                                      stream_ptr())
    return rc, f


def _split(hip, data):
    b = np.frombuffer(data, np.uint8)
    pi, gi = hip.JpegInfo(), hip.JpegInfo()
    assert hip.load().uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(pi), C.byref(gi)) == 0
    return data[pi.offset:pi.offset + pi.size], data[gi.offset:gi.offset + gi.size]


def _jpeg_planes(hip, data):
    b = np.frombuffer(data, np.uint8)
    out, desc = np.zeros(1 << 20, np.uint8), hip.Image()
    assert hip.load().uhdr_hip_jpeg_decode(C.c_void_p(b.ctypes.data), b.size, C.c_void_p(out.ctypes.data), out.size, C.byref(desc), hip.MEM_HOST, None) == 0
    n = desc.width * desc.height
    return out[:n if desc.pixelFormat == hip.PIX_FMT_MONOCHROME else n * 3 // 2].copy(), desc.width, desc.height


@pytest.mark.parametrize("tf,gamut", [(T.TF_PQ, T.CG_2100), (T.TF_HLG, T.CG_P3)])
def test_files_equal_api1_on_the_tonemapped_planes(hip, tf, gamut):
    """64 x 64 and 256 x 144 (whole 16-column batches: the encoder pads nothing) in one call: byte for byte the files API-1 writes
    for the same P010 images and the planes uhdr_hip_tonemap_sdr_batch derives from them; PER_IMAGE: the adaptive API-1's files"""
    frames = [_packed(hip, *T.planes("lcg", 64, 64), gamut), _packed(hip, *T.planes("ramp", 256, 144), gamut)]
    peaks = [0.0, 800.0]
    for scope in (-1, hip.BOOST_PER_IMAGE):
        mds = (hip.Metadata * 2)()
        rc, got = _tonemapped(hip, frames, tf, 90, T.REINHARD, peaks, scope, mds)
        rc1, want = _api1_on_tonemapped_planes(hip, frames, tf, 90, peaks, scope)
        assert rc == 0 and rc1 == 0 and list(got.status) == [0, 0] == list(want.status)
        for i in range(2):
            assert got.file(i) == want.file(i), (scope, i, got.sizes[i], want.sizes[i])
            parsed = hip.Metadata()
            b = np.frombuffer(got.file(i), np.uint8)
            assert hip.load().uhdr_hip_jpegr_metadata(C.c_void_p(b.ctypes.data), b.size, C.byref(parsed)) == 0
            # (the XMP carries the boosts as decimal text: equal to a few units of f32's last place)
            assert (parsed.minContentBoost, parsed.maxContentBoost) == pytest.approx((mds[i].minContentBoost, mds[i].maxContentBoost), rel=1e-5)
        if scope < 0:
            assert mds[0].minContentBoost == 1.0 and F(mds[0].maxContentBoost) == T.k_of(tf)


def test_ragged_file_decodes_to_api1s_planes(hip):
    """66 x 34: the encoder's column padding differs between the two paths' strides, so the primaries are compared decoded; the
    gain-map JPEGs are byte-equal"""
    l, c = T.planes("lcg", 66, 34)
    frames = [Frame(hip, l, c, T.CG_709, 80, 70, 66, 33)]
    rc, got = _tonemapped(hip, frames, T.TF_HLG, 95, T.REINHARD, None, -1)
    rc1, want = _api1_on_tonemapped_planes(hip, frames, T.TF_HLG, 95, None, -1)
    assert rc == 0 and rc1 == 0
    (gp, gg), (wp, wg) = _split(hip, got.file(0)), _split(hip, want.file(0))
    assert gg == wg
    a, b = _jpeg_planes(hip, gp), _jpeg_planes(hip, wp)
    assert a[1:] == b[1:] == (66, 34) and np.array_equal(a[0], b[0])


def test_shift_file_is_todays_api0_file_and_a_bad_peak_stays_isolated(hip):
    tf = T.TF_HLG
    frames = [_packed(hip, *T.planes("lcg", 64, 64), T.CG_2100), _packed(hip, *T.planes("ramp", 64, 64), T.CG_2100),
              _packed(hip, *T.planes("ramp", 256, 144), T.CG_2100)]
    n, lib = len(frames), hip.load()
    rc, shift = _tonemapped(hip, frames, tf, 90, T.SHIFT, None, -1)
    today = Files(n)
    rc0 = lib.uhdr_hip_jpegr_encode_batch(n, hip.image_array([f.src for f in frames]), None, tf, 90, None, None, today.outs, today.caps, today.sizes,
                                          today.status, hip.MEM_DEVICE, stream_ptr())
    assert rc == 0 and rc0 == 0 and all(shift.file(i) == today.file(i) for i in range(n))
    rc, good = _tonemapped(hip, frames, tf, 90, T.REINHARD, [0.0, 500.0, 0.0], -1)
    assert rc == 0 and all(good.file(i) != today.file(i) for i in range(n))
    rc, bad = _tonemapped(hip, frames, tf, 90, T.REINHARD, [0.0, float("nan"), 0.0], -1)
    assert rc == hip.ERROR_UNSUPPORTED_FEATURE and list(bad.status) == [0, hip.ERROR_UNSUPPORTED_FEATURE, 0]
    assert bad.file(0) == good.file(0) and bad.file(2) == good.file(2) and not bad.bufs[1].any()


def test_the_gain_map_of_a_tonemapped_file_is_not_pinned_to_one_code(hip):
    """64 x 64 PQ noise: the shift path's pseudo-SDR pins most of the map at one code; the tone-mapped file's map holds a range"""
    frames = [_packed(hip, *T.planes("lcg", 64, 64), T.CG_2100)]
    rc, tm = _tonemapped(hip, frames, T.TF_PQ, 90, T.REINHARD, None, -1)
    rc0, sh = _tonemapped(hip, frames, T.TF_PQ, 90, T.SHIFT, None, -1)
    assert rc == 0 and rc0 == 0
    gm, w, h = _jpeg_planes(hip, _split(hip, tm.file(0))[1])
    gs, _, _ = _jpeg_planes(hip, _split(hip, sh.file(0))[1])
    top = lambda a: int(np.bincount(a).max())
    print("tonemap-observed gain map 64x64 PQ noise: tone-mapped %d distinct values (commonest holds %d of %d), shift %d distinct (commonest %d)"
          % (len(np.unique(gm)), top(gm), gm.size, len(np.unique(gs)), top(gs)))
    assert (w, h) == (16, 16) and len(np.unique(gm)) > 2


def test_shim_additions(hip, tmp_path):
    """toneMapSdr and JpegRHip::setToneMap from a C++ program (tests/cpp/shim_tonemap_test.cpp), which checks its results against the
    C-ABI calls they stand on"""
    exe = str(tmp_path / "shim_tonemap_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_tonemap_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
