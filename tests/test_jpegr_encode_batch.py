"""uhdr_hip_jpegr_encode_batch: encodeJPEGR API-1 / API-0 for n files per call.  Every file equals the single call with the same
arguments (status, size, bytes) and the CPU restatement (oracle/jpegr_oracle.py); invalid files fail alone.  The CPU tests need
no GPU: argument checks come before any device state is touched."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from libultrahdr_dev_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    return api.load()


class Batch:
    """one call's arrays; keeps every buffer it points to alive"""

    def __init__(self, p010s, yuvs, caps, exifs=None):
        n = len(p010s)
        self.n = n
        self.P = api.image_array(p010s) if n else None
        self.Y = api.image_array(yuvs) if yuvs is not None else None
        self.outs = [np.zeros(max(int(c), 1), np.uint8) for c in caps]
        self.optr = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in self.outs])
        self.cap = (C.c_size_t * max(n, 1))(*caps)
        self.size = (C.c_size_t * max(n, 1))()
        self.stat = (C.c_int * max(n, 1))()
        self.ex = self.exn = None
        if exifs is not None:
            self._ex = [np.frombuffer(e, np.uint8) if e else None for e in exifs]
            self.ex = (C.c_void_p * n)(*[e.ctypes.data if e is not None else None for e in self._ex])
            self.exn = (C.c_size_t * n)(*[len(e) if e else 0 for e in exifs])

    def run(self, lib, tf, q, mem, stream=None):
        return lib.uhdr_hip_jpegr_encode_batch(self.n, self.P, self.Y, tf, q, self.ex, self.exn, self.optr, self.cap, self.size, self.stat,
                                               mem, stream)

    def file(self, i):
        return self.outs[i][:self.size[i]].tobytes()


def single(lib, p, y, tf, q, exif, cap, mem, stream=None):
    """-> (status, bytes or None, size) of uhdr_hip_jpegr_encode_api1 (y given) or _api0"""
    buf = np.zeros(max(cap, 1), np.uint8)
    n = C.c_size_t()
    eb = np.frombuffer(exif, np.uint8) if exif else None
    ep = C.c_void_p(eb.ctypes.data) if eb is not None else None
    en = len(exif) if exif else 0
    if y is None:
        rc = lib.uhdr_hip_jpegr_encode_api0(C.byref(p), tf, q, ep, en, C.c_void_p(buf.ctypes.data), cap, C.byref(n), mem, stream)
    else:
        rc = lib.uhdr_hip_jpegr_encode_api1(C.byref(p), C.byref(y), tf, q, ep, en, C.c_void_p(buf.ctypes.data), cap, C.byref(n), mem, stream)
    return rc, (buf[:n.value].tobytes() if rc == 0 else None), n.value


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_call_level_arguments(lib):
    p = np.zeros(64 * 64 * 3 // 2, np.uint16)
    y = np.zeros(64 * 64 * 3 // 2, np.uint8)
    pi = api.p010_image(p.ctypes.data, 64, 64, api.CG_BT2100)
    yi = api.yuv420_image(y.ctypes.data, 64, 64, api.CG_BT709)
    b = Batch([pi], [yi], [1 << 16])
    f = lib.uhdr_hip_jpegr_encode_batch
    assert f(-1, b.P, b.Y, api.TF_HLG, 95, None, None, b.optr, b.cap, b.size, b.stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert f(0, None, None, api.TF_HLG, 95, None, None, None, None, None, None, api.MEM_HOST, None) == 0
    assert f(1, None, b.Y, api.TF_HLG, 95, None, None, b.optr, b.cap, b.size, b.stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert f(1, b.P, b.Y, api.TF_HLG, 95, None, None, None, b.cap, b.size, b.stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert f(1, b.P, b.Y, api.TF_HLG, 95, None, None, b.optr, None, b.size, b.stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert f(1, b.P, b.Y, api.TF_HLG, 95, None, None, b.optr, b.cap, None, b.stat, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    b.stat[0] = 12345
    for q in (-1, 101):
        assert f(1, b.P, b.Y, api.TF_HLG, q, None, None, b.optr, b.cap, b.size, b.stat, api.MEM_HOST, None) == api.ERROR_INVALID_QUALITY_FACTOR
    assert b.stat[0] == 12345   # call-level errors leave the per-file statuses alone


def _files_for_validation():
    """(p010 image, yuv image, exif, note): valid and invalid host-memory pairs, buffers kept alive by the returned list"""
    keep, out = [], []

    def pair(w, h, sdr=api.CG_BT709, hdr=api.CG_BT2100, ls=None, yls=None):
        p = np.zeros((ls or w) * h * 3 // 2 + 64, np.uint16)
        y = np.zeros((yls or w) * h * 3 // 2 + 64, np.uint8)
        keep.extend([p, y])
        return api.p010_image(p.ctypes.data, w, h, hdr, ls), api.yuv420_image(y.ctypes.data, w, h, sdr, yls)

    out.append(pair(64, 64) + (None, "valid"))
    out.append(pair(66, 64) + (None, "odd width / 2"))
    out.append(pair(63, 64) + (None, "odd width"))
    p, y = pair(64, 64)
    p.colorGamut = 7
    out.append((p, y, None, "bad hdr gamut"))
    p, y = pair(64, 64)
    y.colorGamut = -1
    out.append((p, y, None, "bad sdr gamut"))
    p, y = pair(64, 64)
    p.luma_stride = 32
    out.append((p, y, None, "bad p010 stride"))
    p, y = pair(64, 64)
    y.luma_stride = 32
    out.append((p, y, None, "bad yuv stride"))
    out.append(pair(64, 64) + (b"", "exif NULL with a size"))
    out.append(pair(96, 48, api.CG_P3, api.CG_BT709) + (b"Exif\0\0abc", "valid with exif"))
    return out, keep


@pytest.mark.parametrize("api0", [False, True])
def test_per_file_validation_matches_single_calls(lib, api0):
    files, keep = _files_for_validation()
    n = len(files)
    exifs = [f[2] for f in files]
    b = Batch([f[0] for f in files], None if api0 else [f[1] for f in files], [1 << 20] * n, exifs)
    # exif NULL with a non-zero size: the array entry is NULL, the size is not
    k = [f[3] for f in files].index("exif NULL with a size")
    b.ex[k] = None
    b.exn[k] = 12
    rc = b.run(lib, api.TF_HLG, 95, api.MEM_HOST)
    want = []
    for i, (p, y, ex, note) in enumerate(files):
        buf = np.zeros(1 << 20, np.uint8)
        sz = C.c_size_t()
        en = 12 if i == k else (len(ex) if ex else 0)
        eb = np.frombuffer(ex, np.uint8) if ex else None
        ep = None if (i == k or eb is None) else C.c_void_p(eb.ctypes.data)
        if api0:
            s = lib.uhdr_hip_jpegr_encode_api0(C.byref(p), api.TF_HLG, 95, ep, en, C.c_void_p(buf.ctypes.data), buf.size, C.byref(sz), api.MEM_HOST, None)
        else:
            s = lib.uhdr_hip_jpegr_encode_api1(C.byref(p), C.byref(y), api.TF_HLG, 95, ep, en, C.c_void_p(buf.ctypes.data), buf.size, C.byref(sz),
                                               api.MEM_HOST, None)
        want.append(s)
    assert list(b.stat[:n]) == want, [(f[3], s, w) for f, s, w in zip(files, b.stat[:n], want)]
    first = next((s for s in want if s != 0), 0)
    assert rc == first
    # an invalid hdr_tf: every file reports what its single call would, no special case
    b2 = Batch([f[0] for f in files], None if api0 else [f[1] for f in files], [1 << 20] * n)
    b2.run(lib, 9, 95, api.MEM_HOST)
    for i, (p, y, ex, note) in enumerate(files):
        buf = np.zeros(16, np.uint8)
        sz = C.c_size_t()
        if api0:
            s = lib.uhdr_hip_jpegr_encode_api0(C.byref(p), 9, 95, None, 0, C.c_void_p(buf.ctypes.data), 16, C.byref(sz), api.MEM_HOST, None)
        else:
            s = lib.uhdr_hip_jpegr_encode_api1(C.byref(p), C.byref(y), 9, 95, None, 0, C.c_void_p(buf.ctypes.data), 16, C.byref(sz), api.MEM_HOST, None)
        assert b2.stat[i] == s, (note, b2.stat[i], s)


def test_batched_encoder_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    if not os.path.exists(kernel_resources.HIPCC):
        pytest.skip("hipcc not present")
    t = kernel_resources.resources(src=os.path.join(ROOT, "libultrahdr_dev_amd", "csrc", "uhdr_jpeg.hip"))
    multi = {k: v for k, v in t.items() if k.split("(")[0].endswith("_multi")}
    names = {k.split("(")[0].split("::")[-1] for k in multi}
    assert names == {"k_jpeg_fdct_quant_count_multi", "k_jpeg_clear_multi", "k_jpeg_emit_multi", "k_jpeg_stuff_count_multi",
                     "k_jpeg_stuff_copy_multi"}, names
    bad = {k: v for k, v in multi.items() if v.get("scratch", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert not bad, bad


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _gpu():
    import torch
    from oracle import jpegr_oracle as J
    from oracle import oracle as O
    return torch, O, J


def _padded(p010, yuv, w, h, pls, yls):
    """tight planes -> planes with luma strides pls (P010 elements) / yls (bytes), chroma strides to match; -> (p, y, p_cs, y_cs)"""
    P = np.zeros(pls * h * 3 // 2, np.uint16)
    P[:pls * h].reshape(h, pls)[:, :w] = p010[:w * h].reshape(h, w)
    P[pls * h:].reshape(h // 2, pls)[:, :w] = p010[w * h:].reshape(h // 2, w)
    ycs = yls // 2
    Y = np.zeros(yls * h + ycs * h, np.uint8)
    Y[:yls * h].reshape(h, yls)[:, :w] = yuv[:w * h].reshape(h, w)
    cw, ch = w // 2, h // 2
    Y[yls * h:yls * h + ycs * ch].reshape(ch, ycs)[:, :cw] = yuv[w * h:w * h + cw * ch].reshape(ch, cw)
    Y[yls * h + ycs * ch:].reshape(ch, ycs)[:, :cw] = yuv[w * h + cw * ch:].reshape(ch, cw)
    return P, Y, pls, ycs


class Case:
    """one file: tight planes (for the oracle), the planes handed to the library in host memory and on the device"""

    def __init__(self, O, torch, w, h, sdr, hdr, seed, exif=None, pad=0, frame=None):
        self.w, self.h, self.sdr, self.hdr, self.exif = w, h, sdr, hdr, exif
        self.p010, self.yuv = frame if frame is not None else O.lcg_frame(w, h, seed)
        if pad:
            P, Y, pcs, ycs = _padded(self.p010, self.yuv, w, h, w + pad, w + 2 * pad)
            self.strides = (w + pad, pcs, w + 2 * pad, ycs)
        else:
            P, Y = self.p010.copy(), self.yuv.copy()
            self.strides = (None, None, None, None)
        self.hp, self.hy = P, Y
        self.dp = torch.from_numpy(P.view(np.uint8).copy()).cuda()
        self.dy = torch.from_numpy(Y.copy()).cuda()

    def images(self, mem):
        pls, pcs, yls, ycs = self.strides
        pp = self.dp.data_ptr() if mem == api.MEM_DEVICE else self.hp.ctypes.data
        yp = self.dy.data_ptr() if mem == api.MEM_DEVICE else self.hy.ctypes.data
        pi = api.p010_image(pp, self.w, self.h, self.hdr, pls)
        yi = api.yuv420_image(yp, self.w, self.h, self.sdr, yls)
        if pls is not None:
            pi.chroma_data = pp + pls * self.h * 2
            pi.chroma_stride = pcs
            yi.chroma_data = yp + yls * self.h
            yi.chroma_stride = ycs
        return pi, yi

    def oracle(self, J, api0, tf, q):
        if api0:
            return J.encode_api0(self.p010, self.w, self.h, self.hdr, tf, q, exif=self.exif)
        return J.encode_api1(self.p010, self.yuv, self.w, self.h, self.sdr, self.hdr, tf, q, exif=self.exif)


def _mixed(O, torch):
    p = np.fromfile(os.path.join(GOLDEN, "raw_p010_image.p010"), np.uint16)
    y = np.fromfile(os.path.join(GOLDEN, "raw_yuv420_image.yuv420"), np.uint8)
    spec = [(640, 480, api.CG_BT709, api.CG_BT2100, None, 0), (200, 120, api.CG_P3, api.CG_BT709, b"Exif\0\0batch-1", 0),
            (72, 40, api.CG_BT2100, api.CG_P3, None, 0), (64, 64, api.CG_BT709, api.CG_BT2100, None, 0),
            (136, 72, api.CG_P3, api.CG_BT2100, b"Exif\0\0batch-2" * 7, 0), (100, 50, api.CG_BT709, api.CG_BT709, None, 16),
            (64, 64, api.CG_P3, api.CG_BT2100, None, 0), (200, 120, api.CG_BT709, api.CG_P3, None, 0)]
    cases = [Case(O, torch, w, h, s, d, 100 + i, e, pad) for i, (w, h, s, d, e, pad) in enumerate(spec)]
    cases.insert(4, Case(O, torch, 1280, 720, api.CG_BT709, api.CG_BT2100, 0, None, 0, frame=(p[:1280 * 720 * 3 // 2], y[:1280 * 720 * 3 // 2])))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("api0", [False, True])
def test_mixed_batch_equals_oracle_and_single_calls(lib, api0):
    torch, O, J = _gpu()
    api.init(0)
    cases = _mixed(O, torch)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tf in (api.TF_LINEAR, api.TF_HLG, api.TF_PQ):
        want = [c.oracle(J, api0, tf, 90) for c in cases]
        for mem in (api.MEM_DEVICE, api.MEM_HOST):
            imgs = [c.images(mem) for c in cases]
            caps = [c.w * c.h * 4 + 65536 for c in cases]
            b = Batch([i[0] for i in imgs], None if api0 else [i[1] for i in imgs], caps, [c.exif for c in cases])
            torch.cuda.synchronize()
            rc = b.run(lib, tf, 90, mem, stream)
            assert rc == 0 and list(b.stat[:b.n]) == [0] * b.n, (tf, mem, list(b.stat[:b.n]))
            for k, c in enumerate(cases):
                s_rc, s_bytes, _ = single(lib, imgs[k][0], None if api0 else imgs[k][1], tf, 90, c.exif, caps[k], mem, stream)
                assert s_rc == 0
                got = b.file(k)
                assert got == s_bytes, (tf, mem, k, c.w, c.h, len(got), len(s_bytes))
                assert got == want[k], (tf, mem, k, c.w, c.h)


@pytest.mark.gpu
def test_invalid_files_and_a_short_buffer_stay_isolated(lib):
    torch, O, J = _gpu()
    api.init(0)
    cases = [Case(O, torch, 64 + 16 * (k % 3), 64, [api.CG_BT709, api.CG_P3, api.CG_BT2100][k % 3], api.CG_BT2100, 300 + k) for k in range(7)]
    imgs = [c.images(api.MEM_DEVICE) for c in cases]
    imgs[2][0].width = 63                   # odd width
    imgs[3][1].colorGamut = 9               # bad SDR gamut
    imgs[5][1].luma_stride = 8              # bad stride
    caps = [1 << 20] * len(cases)
    caps[4] = 1000                          # too small: INSUFFICIENT_RESOURCE with the exact size
    b = Batch([i[0] for i in imgs], [i[1] for i in imgs], caps)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = b.run(lib, api.TF_PQ, 85, api.MEM_DEVICE, stream)
    for k in range(len(cases)):
        s_rc, s_bytes, s_n = single(lib, imgs[k][0], imgs[k][1], api.TF_PQ, 85, None, caps[k], api.MEM_DEVICE, stream)
        assert b.stat[k] == s_rc, (k, b.stat[k], s_rc)
        if s_rc == 0:
            assert b.file(k) == s_bytes == cases[k].oracle(J, False, api.TF_PQ, 85)
    assert b.stat[2] == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT and b.stat[3] == api.ERROR_INVALID_COLORGAMUT
    assert b.stat[5] == api.ERROR_INVALID_STRIDE and b.stat[4] == api.ERROR_INSUFFICIENT_RESOURCE
    assert b.size[4] == len(cases[4].oracle(J, False, api.TF_PQ, 85)) > 1000
    assert rc == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT


@pytest.mark.gpu
def test_more_files_than_one_round(lib):
    torch, O, J = _gpu()
    api.init(0)
    cases = [Case(O, torch, 64, 64, api.CG_BT709 if k % 5 else api.CG_P3, api.CG_BT2100, 500 + k) for k in range(70)]
    imgs = [c.images(api.MEM_DEVICE) for c in cases]
    b = Batch([i[0] for i in imgs], [i[1] for i in imgs], [1 << 16] * len(cases))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert b.run(lib, api.TF_HLG, 95, api.MEM_DEVICE, stream) == 0
    for k in range(len(cases)):
        s_rc, s_bytes, _ = single(lib, imgs[k][0], imgs[k][1], api.TF_HLG, 95, None, 1 << 16, api.MEM_DEVICE, stream)
        assert s_rc == 0 and b.file(k) == s_bytes, k
    for k in (0, 1, 64, 69):
        assert b.file(k) == cases[k].oracle(J, False, api.TF_HLG, 95), k


@pytest.mark.gpu
@pytest.mark.parametrize("mem", [api.MEM_DEVICE, api.MEM_HOST])
def test_stream_larger_than_its_staging_is_compressed_again(lib, mem):
    torch, O, J = _gpu()
    api.init(0)
    w = h = 512   # LCG noise at q100: ~2.3 bytes per pixel against the first guess of w*h + 64 KiB
    cases = [Case(O, torch, w, h, api.CG_P3, api.CG_BT2100, 900), Case(O, torch, w, h, api.CG_BT709, api.CG_BT2100, 901),
             Case(O, torch, 64, 64, api.CG_BT709, api.CG_BT2100, 902)]
    imgs = [c.images(mem) for c in cases]
    caps = [w * h * 6] * 3
    for api0 in (False, True):
        b = Batch([i[0] for i in imgs], None if api0 else [i[1] for i in imgs], caps)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert b.run(lib, api.TF_HLG, 100, mem, stream) == 0
        for k, c in enumerate(cases):
            want = c.oracle(J, api0, api.TF_HLG, 100)
            assert b.file(k) == want, (api0, k)
        assert b.size[0] > w * h + 65536 and b.size[1] > w * h + 65536


@pytest.mark.gpu
def test_two_host_threads_on_their_own_streams(lib):
    torch, O, J = _gpu()
    api.init(0)
    groups = [[Case(O, torch, 96 + 32 * (k % 2), 64 + 16 * t, [api.CG_BT709, api.CG_P3][k % 2], api.CG_BT2100, 700 + 10 * t + k) for k in range(5)]
              for t in range(2)]
    want = [[c.oracle(J, False, api.TF_HLG, 90) for c in g] for g in groups]
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(4):
                    imgs = [c.images(api.MEM_DEVICE) for c in groups[t]]
                    b = Batch([i[0] for i in imgs], [i[1] for i in imgs], [1 << 17] * len(imgs))
                    rc = b.run(lib, api.TF_HLG, 90, api.MEM_DEVICE, C.c_void_p(s.cuda_stream))
                    if rc != 0 or [b.file(k) for k in range(b.n)] != want[t]:
                        errors.append((t, rc, list(b.stat[:b.n])))
        except Exception as e:   # noqa: BLE001 (reported by the main thread)
            errors.append((t, repr(e)))

    torch.cuda.synchronize()
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors


@pytest.mark.gpu
def test_4k_batch_equals_single_calls_and_decodes_alike(lib):
    torch, O, J = _gpu()
    from libultrahdr_dev_amd import synth
    api.init(0)
    w, h, n = 3840, 2160, 8
    frames = [synth.smooth_frame(w, h, 40 + k) for k in range(n)]
    imgs = [(api.p010_image(p.data_ptr(), w, h, api.CG_BT2100), api.yuv420_image(y.data_ptr(), w, h, [api.CG_BT709, api.CG_P3][k % 2]))
            for k, (p, y) in enumerate(frames)]
    cap = w * h * 3
    b = Batch([i[0] for i in imgs], [i[1] for i in imgs], [cap] * n)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert b.run(lib, api.TF_HLG, 95, api.MEM_DEVICE, stream) == 0
    singles = []
    for k in range(n):
        s_rc, s_bytes, _ = single(lib, imgs[k][0], imgs[k][1], api.TF_HLG, 95, None, cap, api.MEM_DEVICE, stream)
        assert s_rc == 0 and b.file(k) == s_bytes, k
        singles.append(s_bytes)

    def decode(files):
        bufs = [np.frombuffer(f, np.uint8) for f in files]
        ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in bufs])
        sizes = (C.c_size_t * n)(*[x.size for x in bufs])
        outs = [torch.empty(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(n)]
        optr = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        ocap = (C.c_size_t * n)(*[w * h * 4] * n)
        dests = (api.Image * n)()
        st = (C.c_int * n)()
        rc = lib.uhdr_hip_jpegr_decode_batch(n, ptrs, sizes, api.OUTPUT_HDR_HLG, api.FLT_MAX, optr, ocap, dests, None, st, api.APPLY_EXACT,
                                             api.MEM_DEVICE, stream)
        assert rc == 0, list(st)
        torch.cuda.synchronize()
        return outs

    for a, c in zip(decode([b.file(k) for k in range(n)]), decode(singles)):
        assert torch.equal(a, c)
