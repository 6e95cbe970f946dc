"""-m gpu: the packed API-0 -- uhdr_hip_tonemap_packed_batch, uhdr_hip_tonemap_packed,
uhdr_hip_jpegr_encode_packed_api0_batch and the shim's two additions against the model of tests/packed_tonemap_cases.py.

Pixels: a sample is in doubt when the model's value before truncation lies within 1/256 of an integer (tonemap_cases.DOUBT); samples
not in doubt equal the model, samples in doubt may differ by one code, none by more.  The headroom equals the model's bit for bit,
A is 0xFF, and the bytes around every destination and in its padding columns keep their fill: destinations whose case is `aligned`
lie on 256-byte boundaries, which sends them to the ALIGNED kernel instance, the others 4 (F16 cases: 8) bytes behind one.  Every
test prints what it observed ("packed-tonemap-observed ...") before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import packed_tonemap_cases as K
from tests import tonemap_cases as T
from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 256
GAMUT = 2   # BT.2100


def _bpp(fmt):
    return 8 if fmt == K.FMT_F16 else 4


def _desc(hip, fmt, ptr, w, h, gamut, stride):
    return (hip.rgba_f16_image if fmt == K.FMT_F16 else hip.rgba1010102_image)(ptr, w, h, gamut, stride)


def _src_bytes(img, fmt, stride, offset):
    """the image at `stride` pixels per row behind GUARD + offset bytes, all else poison"""
    h, w = img.shape[:2]
    bpp = _bpp(fmt)
    rows = np.full((h, stride * bpp), 0xEE, np.uint8)
    rows[:, :w * bpp] = np.ascontiguousarray(img).view(np.uint8).reshape(h, w * bpp)
    return np.concatenate([np.full(GUARD + offset, 0xEE, np.uint8), rows.reshape(-1)])


class Frame:
    """one packed HDR image on the device in a layout, and an RGBA8888 destination between guard bytes"""

    def __init__(self, hip, img, fmt, gamut=GAMUT, src_stride=None, dst_stride=None, offset=0):
        self.h, self.w = img.shape[:2]
        self.fmt, self.gamut, self.offset = fmt, gamut, offset
        self.ss, self.ds = src_stride or self.w, dst_stride or self.w
        self.keep = to_dev(_src_bytes(img, fmt, self.ss, offset))
        assert self.keep.data_ptr() % 256 == 0
        self.src = _desc(hip, fmt, self.keep.data_ptr() + GUARD + offset, self.w, self.h, gamut, self.ss)
        self.n = self.ds * self.h * 4
        self.out = dev_empty(self.n + 2 * GUARD + 16, 0xCD)
        assert self.out.data_ptr() % 256 == 0
        # (the stride travels in the descriptor; width, height, gamut and format are the call's to fill in)
        self.dst = hip.Image(self.out.data_ptr() + GUARD + offset, 0, 0, hip.CG_UNSPECIFIED, None, self.ds, 0, -1)

    def reset(self):
        self.out.fill_(0xCD)

    def result(self):
        """-> (pixels (h, ds, 4), the bytes around them intact)"""
        a = to_host(self.out)
        lo = GUARD + self.offset
        return a[lo:lo + self.n].reshape(self.h, self.ds, 4).copy(), bool((a[:lo] == 0xCD).all() and (a[lo + self.n:] == 0xCD).all())


def frame_of(hip, case):
    return Frame(hip, K.image(case.content, case.fmt, case.tf, case.w, case.h), case.fmt, GAMUT, case.src_stride, case.dst_stride, case.offset)


def run_batch(hip, frames, tf, peaks=None, op=K.REINHARD, stream=None):
    """one uhdr_hip_tonemap_packed_batch -> (status, headroom float32[n], its guards intact, dests)"""
    n = len(frames)
    head = dev_empty(4 * n + 2 * GUARD, 0xCD)
    sa, da = hip.image_array([f.src for f in frames]), hip.image_array([f.dst for f in frames])
    pk = None if peaks is None else (C.c_float * n)(*peaks)
    rc = hip.load().uhdr_hip_tonemap_packed_batch(n, sa, da, tf, op, pk, C.c_void_p(head.data_ptr() + GUARD), stream or stream_ptr())
    torch.cuda.synchronize()
    hb = to_host(head)
    ok = bool((hb[:GUARD] == 0xCD).all() and (hb[GUARD + 4 * n:] == 0xCD).all())
    return rc, hb[GUARD:GUARD + 4 * n].view(F).copy(), ok, da


def check_pixels(name, frame, want):
    got, ok = frame.result()
    w = frame.w
    differ, doubt, worst, hard = K.compare(got[:, :w], want)
    print("packed-tonemap-observed %s: %d of %d samples differ (%d in doubt), worst %d, %d outside the band" % (name, differ, want["v"].size, doubt,
                                                                                                               worst, hard))
    assert ok, "bytes around the destination were written"
    assert (got[:, w:] == 0xCD).all(), (name, "padding columns were written")
    assert hard == 0 and worst <= 1, (name, differ, doubt, worst, hard)
    assert (got[:, :w, 3] == 0xFF).all(), (name, "alpha")
    return got[:, :w].copy()


@pytest.mark.parametrize("case", K.cases(), ids=repr)
def test_pixels_and_headroom_equal_the_model(hip, case):
    fr = frame_of(hip, case)
    assert (fr.src.data % 16 == 0 and fr.dst.data % 16 == 0) == case.aligned   # the layout takes the instance the case names
    want = K.expected(case)
    rc, head, ok, da = run_batch(hip, [fr], case.tf)
    print("packed-tonemap-observed %s H: device %r model %r" % (case.name, head[0], want["H"]))
    assert rc == 0 and ok
    assert head[0].tobytes() == want["H"].tobytes(), (head[0], want["H"], want["m"])
    check_pixels(case.name, fr, want)
    d = da[0]
    assert (d.width, d.height, d.luma_stride, d.colorGamut, d.pixelFormat, d.data) == (case.w, case.h, case.dst_stride, GAMUT, hip.PIX_FMT_RGBA8888,
                                                                                      fr.dst.data)


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
def test_given_and_measured_headroom_share_a_batch(hip, form):
    """five images of three sizes and both alignment classes, peaks [0, 600, 0, 450, 0]: every image its own slot, four launch groups"""
    fmt, tf = form
    by = {c.name.split("-")[0]: c for c in K.cases() if (c.fmt, c.tf) == form}
    picks = [by["64x64"], by["64x64"], by["66x34"], by["264x10"], by["8x8"]]
    peaks = [0.0, 600.0, 0.0, 450.0, 0.0]
    frames = [frame_of(hip, c) for c in picks]
    wants = [K.expected(c, p) for c, p in zip(picks, peaks)]
    rc, head, ok, _ = run_batch(hip, frames, tf, peaks)
    print("packed-tonemap-observed mixed batch tf %d H: device %r model %r" % (tf, list(head), [w["H"] for w in wants]))
    assert rc == 0 and ok
    for i in range(len(picks)):
        assert head[i].tobytes() == wants[i]["H"].tobytes(), (i, head[i], wants[i]["H"])
        check_pixels("mixed[%d]-%s" % (i, picks[i].name), frames[i], wants[i])
    assert head[1] == T.headroom(tf, F(0.0), 600.0) and head[3] == T.headroom(tf, F(0.0), 450.0)
    # peaks == NULL measures every image
    for f in frames:
        f.reset()
    rc, head_all, ok, _ = run_batch(hip, frames, tf, None)
    assert rc == 0 and ok
    for i, c in enumerate(picks):
        assert head_all[i].tobytes() == K.expected(c)["H"].tobytes(), i
        check_pixels("measured[%d]-%s" % (i, c.name), frames[i], K.expected(c))


def test_a_failing_call_writes_nothing(hip):
    case = next(c for c in K.cases() if c.name == "64x64-pq1010102-lcg")
    frames = [frame_of(hip, case), frame_of(hip, case)]
    for peaks, op, want in (([0.0, float("nan")], K.REINHARD, hip.ERROR_UNSUPPORTED_FEATURE), ([0.0, 0.0], K.SHIFT, hip.ERROR_UNSUPPORTED_FEATURE)):
        rc, head, ok, da = run_batch(hip, frames, case.tf, peaks, op)
        assert rc == want and ok and (head.view(np.uint8) == 0xCD).all()
        for f, d in zip(frames, da):
            got, g = f.result()
            assert g and (got == 0xCD).all() and (d.width, d.height, d.pixelFormat) == (0, 0, -1)
    frames[1].src.colorGamut = 7   # the LAST image's last check
    rc, head, ok, _ = run_batch(hip, frames, case.tf)
    assert rc == hip.ERROR_INVALID_COLORGAMUT and ok and (head.view(np.uint8) == 0xCD).all() and (frames[0].result()[0] == 0xCD).all()


@pytest.mark.parametrize("name", ["66x34-pq1010102-lcg", "64x64-hlg1010102-lcg", "66x34-f16-lcg", "264x10-f16-ramp"])
def test_host_and_device_memory_give_equal_bytes(hip, name):
    """uhdr_hip_tonemap_packed: the image in either memory space, H returned to the host; a host destination's padding stays"""
    case = next(c for c in K.cases() if c.name == name)
    lib, want = hip.load(), K.expected(case)
    fr = frame_of(hip, case)
    h_dev = C.c_float(-1.0)
    assert lib.uhdr_hip_tonemap_packed(C.byref(fr.src), C.byref(fr.dst), case.tf, K.REINHARD, 0.0, C.byref(h_dev), hip.MEM_DEVICE, stream_ptr()) == 0
    dev_px = check_pixels(name + "-device", fr, want)
    assert (fr.dst.width, fr.dst.height, fr.dst.colorGamut, fr.dst.pixelFormat) == (case.w, case.h, GAMUT, hip.PIX_FMT_RGBA8888)
    # host memory, at an address no device call would take: one byte off (the staging copies do not care)
    src = _src_bytes(K.image(case.content, case.fmt, case.tf, case.w, case.h), case.fmt, case.src_stride, 1)
    out = np.full(case.dst_stride * case.h * 4 + 2 * GUARD + 1, 0xCD, np.uint8)
    hs = _desc(hip, case.fmt, src.ctypes.data + GUARD + 1, case.w, case.h, GAMUT, case.src_stride)
    hd = hip.Image(out.ctypes.data + GUARD + 1, 0, 0, hip.CG_UNSPECIFIED, None, case.dst_stride, 0, -1)
    h_host = C.c_float(-1.0)
    assert lib.uhdr_hip_tonemap_packed(C.byref(hs), C.byref(hd), case.tf, K.REINHARD, 0.0, C.byref(h_host), hip.MEM_HOST, stream_ptr()) == 0
    assert F(h_host.value).tobytes() == F(h_dev.value).tobytes() == want["H"].tobytes()
    assert (hd.width, hd.height, hd.luma_stride, hd.colorGamut, hd.pixelFormat) == (case.w, case.h, case.dst_stride, GAMUT, hip.PIX_FMT_RGBA8888)
    px = out[GUARD + 1:-GUARD].reshape(case.h, case.dst_stride, 4)
    assert np.array_equal(px[:, :case.w], dev_px) and (px[:, case.w:] == 0xCD).all()
    assert (out[:GUARD + 1] == 0xCD).all() and (out[-GUARD:] == 0xCD).all()
    # a given peak through the single call, no headroom asked for
    fr.reset()
    assert lib.uhdr_hip_tonemap_packed(C.byref(fr.src), C.byref(fr.dst), case.tf, K.REINHARD, 600.0, None, hip.MEM_DEVICE, stream_ptr()) == 0
    check_pixels(name + "-peak600", fr, K.expected(case, 600.0))


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
def test_the_batch_call_replays_from_a_graph(hip, form):
    """captured on a fresh stream, nothing reserved for it: the replay writes the bytes of the plain call, given and measured H"""
    fmt, tf = form
    by = {c.name.split("-")[0]: c for c in K.cases() if (c.fmt, c.tf) == form}
    picks, peaks = [by["64x64"], by["66x34"], by["64x64"]], [0.0, 0.0, 600.0]
    frames = [frame_of(hip, c) for c in picks]
    rc, head, ok, _ = run_batch(hip, frames, tf, peaks)
    assert rc == 0 and ok
    plain = [f.result()[0] for f in frames]
    for f in frames:
        f.reset()
    n = len(frames)
    dh = torch.zeros(n, dtype=torch.float32, device="cuda")
    sa, da = hip.image_array([f.src for f in frames]), hip.image_array([f.dst for f in frames])
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert hip.load().uhdr_hip_tonemap_packed_batch(n, sa, da, tf, K.REINHARD, (C.c_float * n)(*peaks), C.c_void_p(dh.data_ptr()), s) == 0
    torch.cuda.synchronize()
    assert all((f.result()[0] == 0xCD).all() for f in frames), "capture must not execute the kernels"
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert dh.cpu().numpy().tobytes() == head.tobytes()
    for f, want in zip(frames, plain):
        got, ok = f.result()
        assert ok and np.array_equal(got, want)


# ------------------------------------------------------------------ files

class Files:
    """n output buffers of a batched encode"""

    def __init__(self, n, cap=1 << 19):
        self.bufs = [np.zeros(cap, np.uint8) for _ in range(n)]
        self.outs, self.caps = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs]), (C.c_size_t * n)(*([cap] * n))
        self.sizes, self.status = (C.c_size_t * n)(), (C.c_int * n)(*([7] * n))

    def file(self, i):
        return self.bufs[i][:self.sizes[i]].tobytes()


def _api0(hip, frames, tf, q, peaks, rgb_map, mds=None, op=K.REINHARD):
    n = len(frames)
    f = Files(n)
    pk = None if peaks is None else (C.c_float * n)(*peaks)
    rc = hip.load().uhdr_hip_jpegr_encode_packed_api0_batch(n, hip.image_array([fr.src for fr in frames]), tf, q, None, None, f.outs, f.caps, f.sizes, mds,
                                                            f.status, op, pk, rgb_map, hip.MEM_DEVICE, stream_ptr())
    return rc, f


def _packed_on_tonemapped_images(hip, frames, tf, q, peaks, rgb_map):
    """the RGBA8888 images uhdr_hip_tonemap_packed_batch wrote, given to uhdr_hip_jpegr_encode_packed_batch as the SDR images"""
    n = len(frames)
    rc, _, ok, da = run_batch(hip, frames, tf, peaks)
    assert rc == 0 and ok
    f = Files(n)
    rc = hip.load().uhdr_hip_jpegr_encode_packed_batch(n, hip.image_array([fr.src for fr in frames]), da, tf, q, None, None, f.outs, f.caps, f.sizes, f.status,
                                                       rgb_map, hip.MEM_DEVICE, stream_ptr())
    return rc, f


def _split(hip, data):
    b = np.frombuffer(data, np.uint8)
    pi, gi = hip.JpegInfo(), hip.JpegInfo()
    assert hip.load().uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(pi), C.byref(gi)) == 0
    return data[pi.offset:pi.offset + pi.size], data[gi.offset:gi.offset + gi.size]


def _decode(hip, data, rgb_map):
    """the file through uhdr_hip_jpegr_decode_batch (a per-channel map: its rgbmap sibling) -> (status, descriptor, metadata)"""
    lib = hip.load()
    b = np.frombuffer(data, np.uint8)
    ptrs, sizes = (C.c_void_p * 1)(b.ctypes.data), (C.c_size_t * 1)(b.size)
    dests, mds, stat = (hip.Image * 1)(), (hip.Metadata * 1)(), (C.c_int * 1)(7)
    tail = (0,) if rgb_map else ()
    fn = lib.uhdr_hip_jpegr_decode_rgbmap_batch if rgb_map else lib.uhdr_hip_jpegr_decode_batch
    fn(1, ptrs, sizes, hip.OUTPUT_HDR_PQ, hip.FLT_MAX, None, None, dests, mds, stat, hip.APPLY_EXACT, hip.MEM_HOST, stream_ptr(), *tail)
    assert stat[0] == hip.ERROR_INSUFFICIENT_RESOURCE
    need = hip.output_bytes(hip.OUTPUT_HDR_PQ, dests[0].width, dests[0].height)
    out = np.zeros(need, np.uint8)
    rc = fn(1, ptrs, sizes, hip.OUTPUT_HDR_PQ, hip.FLT_MAX, (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(need), dests, mds, stat, hip.APPLY_EXACT,
            hip.MEM_HOST, stream_ptr(), *tail)
    assert out.any()
    return rc or stat[0], dests[0], mds[0]


def _map_plane(hip, gm_jpeg):
    b = np.frombuffer(gm_jpeg, np.uint8)
    out, desc = np.zeros(1 << 20, np.uint8), hip.Image()
    assert hip.load().uhdr_hip_jpeg_decode(C.c_void_p(b.ctypes.data), b.size, C.c_void_p(out.ctypes.data), out.size, C.byref(desc), hip.MEM_HOST, None) == 0
    return out[:desc.width * desc.height].copy(), desc.width, desc.height


@pytest.mark.parametrize("form", K.FORMS, ids=K.FORM_IDS)
@pytest.mark.parametrize("rgb_map", [0, 1], ids=["oneplane", "rgbmap"])
def test_files_equal_the_packed_call_on_the_tonemapped_images(hip, form, rgb_map):
    """64 x 64, 72 x 40 (rows 3 pixels longer, data off by 4 / 8 bytes) and 64 x 64 again in one call -- two sizes, two alignment
    classes, three launch groups of the tone map: byte for byte the files uhdr_hip_jpegr_encode_packed_batch writes for the same HDR
    images and the images uhdr_hip_tonemap_packed_batch derives from them.  A bad peak fails its own file and no other"""
    fmt, tf = form
    off = _bpp(fmt)
    frames = [Frame(hip, K.ramp(fmt, 64, 64), fmt), Frame(hip, K.ramp(fmt, 72, 40), fmt, GAMUT, 75, 75, off),
              Frame(hip, K.image("lcg", fmt, tf, 64, 64), fmt, 1)]
    peaks = [0.0, 500.0, 0.0]
    n = len(frames)
    mds = (hip.Metadata * n)()
    rc, got = _api0(hip, frames, tf, 90, peaks, rgb_map, mds)
    rc1, want = _packed_on_tonemapped_images(hip, frames, tf, 90, peaks, rgb_map)
    assert rc == 0 and rc1 == 0 and list(got.status) == [0] * n == list(want.status)
    for i in range(n):
        assert got.file(i) == want.file(i), (rgb_map, i, got.sizes[i], want.sizes[i])
        assert mds[i].minContentBoost == 1.0 and F(mds[i].maxContentBoost) == T.k_of(tf) and mds[i].version == b"1.0"
        rcd, d, md = _decode(hip, got.file(i), rgb_map)
        assert rcd == 0 and (d.width, d.height) == (frames[i].w, frames[i].h)
        assert (md.minContentBoost, md.maxContentBoost) == pytest.approx((1.0, float(T.k_of(tf))), rel=1e-5)
    if not rgb_map:   # the ramp's map holds a range, not one code
        gm, w, h = _map_plane(hip, _split(hip, got.file(0))[1])
        print("packed-tonemap-observed gain map of the 64x64 ramp, tf %d: %d distinct values, commonest holds %d of %d"
              % (tf, len(np.unique(gm)), int(np.bincount(gm).max()), gm.size))
        assert (w, h) == (16, 16) and len(np.unique(gm)) > 2
    rc, bad = _api0(hip, frames, tf, 90, [0.0, float("nan"), 0.0], rgb_map)
    assert rc == hip.ERROR_UNSUPPORTED_FEATURE and list(bad.status) == [0, hip.ERROR_UNSUPPORTED_FEATURE, 0]
    assert bad.file(0) == got.file(0) and bad.file(2) == got.file(2) and not bad.bufs[1].any()


def test_files_from_host_memory_and_a_measured_default(hip):
    """images in host memory give the device call's files; hdr_peak_nits == NULL measures every file"""
    fmt, tf = K.FMT_1010102, K.TF_HLG
    imgs = [K.ramp(fmt, 64, 64), K.image("lcg", fmt, tf, 66, 34)]
    frames = [Frame(hip, im, fmt) for im in imgs]
    rc, dev = _api0(hip, frames, tf, 85, None, 0)
    rc0, dev0 = _api0(hip, frames, tf, 85, [0.0, 0.0], 0)
    assert rc == 0 and rc0 == 0 and all(dev.file(i) == dev0.file(i) for i in range(2))
    keep = [np.ascontiguousarray(im) for im in imgs]
    descs = hip.image_array([_desc(hip, fmt, a.ctypes.data, a.shape[1], a.shape[0], GAMUT, a.shape[1]) for a in keep])
    f = Files(2)
    rc = hip.load().uhdr_hip_jpegr_encode_packed_api0_batch(2, descs, tf, 85, None, None, f.outs, f.caps, f.sizes, None, f.status, K.REINHARD, None, 0,
                                                            hip.MEM_HOST, stream_ptr())
    assert rc == 0 and all(f.file(i) == dev.file(i) for i in range(2))


# ------------------------------------------------------------------ the C++ shim

def test_the_shim_gives_the_c_calls_bytes(hip, tmp_path):
    """ultrahdr::JpegRHip::encodeJPEGRPacked from the HDR image alone (setMultiChannelGainMap, setToneMap's peak) and toneMapPacked"""
    exe = str(tmp_path / "shim_packed_tonemap_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_packed_tonemap_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    w, h, peak = 72, 40, 550.0
    lib = hip.load()
    for (fmt, tf), name in zip((K.FORMS[0], K.FORMS[2]), ("1010102", "f16")):
        img = np.ascontiguousarray(K.ramp(fmt, w, h))
        img.tofile(str(tmp_path / "in.hdr"))
        r = subprocess.run([exe, str(tmp_path / "in.hdr"), str(w), str(h), name, str(tf), str(peak), str(tmp_path)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        rd = lambda n: open(tmp_path / n, "rb").read()   # noqa: E731
        desc = hip.image_array([_desc(hip, fmt, img.ctypes.data, w, h, GAMUT, w)])
        for stem, rgb_map, pk in (("one", 0, 0.0), ("rgb", 1, 0.0), ("peak", 0, peak)):
            f = Files(1)
            rc = lib.uhdr_hip_jpegr_encode_packed_api0_batch(1, desc, tf, 90, None, None, f.outs, f.caps, f.sizes, None, f.status, K.REINHARD,
                                                             (C.c_float * 1)(pk), rgb_map, hip.MEM_HOST, stream_ptr())
            assert rc == 0 and rd(stem + ".jpgr") == f.file(0), (name, stem)
        heads = np.frombuffer(rd("heads.f32"), F)
        for k, (stem, pk) in enumerate((("sdr", 0.0), ("peak", peak))):
            out = np.full((h, w + 3, 4), 0xAB, np.uint8)
            hd = hip.Image(out.ctypes.data, 0, 0, hip.CG_UNSPECIFIED, None, w + 3, 0, -1)
            hh = C.c_float()
            assert lib.uhdr_hip_tonemap_packed(desc, C.byref(hd), tf, K.REINHARD, pk, C.byref(hh), hip.MEM_HOST, stream_ptr()) == 0
            assert rd(stem + ".rgba") == out.tobytes() and F(hh.value) == heads[k], (name, stem)
