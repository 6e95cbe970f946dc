"""GPU: the single-file codec calls that bench.py, time_jpeg.py, time_jpeg_dec.py and time_jpegr.py do not time, on one smooth 4K frame:
uhdr_hip_jpeg_encode from host planes into host memory, uhdr_hip_jpeg_decode into host memory, uhdr_hip_jpeg_decode_rgba, API-2 / API-3 /
API-x from device and from host planes, and uhdr_hip_jpegr_decode to the SDR rendition (profiles/r06_single_calls.txt)."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from libultrahdr_dev_amd import api, synth

lib = api.init(0)
W, H = 3840, 2160
p, y = synth.smooth_frame(W, H, 77)
hy = y.cpu().numpy().copy()
hp = p.cpu().numpy().copy()
n = C.c_size_t()


def timed(fn, iters=20):
    for _ in range(3):
        rc = fn()
        assert rc == 0, rc
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


res = {}
dimg = api.Image(y.data_ptr(), W, H, api.CG_BT709, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420)
himg = api.Image(hy.ctypes.data, W, H, api.CG_BT709, hy.ctypes.data + W * H, W, W // 2, api.PIX_FMT_YUV420)
dout = torch.zeros(W * H * 2, dtype=torch.uint8, device="cuda")
hout = np.zeros(W * H * 2, np.uint8)
for q in (95, 85):
    res["jpeg_encode host planes -> host file q%d" % q] = timed(lambda: lib.uhdr_hip_jpeg_encode(C.byref(himg), q, None, 0, C.c_void_p(hout.ctypes.data), hout.size, C.byref(n), api.MEM_HOST, None))
    res["jpeg_encode device planes -> device file q%d" % q] = timed(lambda: lib.uhdr_hip_jpeg_encode(C.byref(dimg), q, None, 0, C.c_void_p(dout.data_ptr()), dout.numel(), C.byref(n), api.MEM_DEVICE, None))
assert lib.uhdr_hip_jpeg_encode(C.byref(himg), 95, None, 0, C.c_void_p(hout.ctypes.data), hout.size, C.byref(n), api.MEM_HOST, None) == 0
jpg = hout[:n.value].copy()
jp = C.c_void_p(jpg.ctypes.data)
desc = api.Image()
dpl = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
hpl = np.zeros(W * H * 4, np.uint8)
res["jpeg_decode -> device planes"] = timed(lambda: lib.uhdr_hip_jpeg_decode(jp, jpg.size, C.c_void_p(dpl.data_ptr()), dpl.numel(), C.byref(desc), api.MEM_DEVICE, None))
res["jpeg_decode -> host planes"] = timed(lambda: lib.uhdr_hip_jpeg_decode(jp, jpg.size, C.c_void_p(hpl.ctypes.data), hpl.size, C.byref(desc), api.MEM_HOST, None))
res["jpeg_decode_rgba -> device"] = timed(lambda: lib.uhdr_hip_jpeg_decode_rgba(jp, jpg.size, C.c_void_p(dpl.data_ptr()), dpl.numel(), C.byref(desc), api.MEM_DEVICE, None))
res["jpeg_decode_rgba -> host"] = timed(lambda: lib.uhdr_hip_jpeg_decode_rgba(jp, jpg.size, C.c_void_p(hpl.ctypes.data), hpl.size, C.byref(desc), api.MEM_HOST, None))

fout = np.zeros(W * H * 3, np.uint8)
fo = C.c_void_p(fout.ctypes.data)
for mem, name, pp, yp in ((api.MEM_DEVICE, "device", p.data_ptr(), y.data_ptr()), (api.MEM_HOST, "host", hp.ctypes.data, hy.ctypes.data)):
    pi = api.p010_image(pp, W, H, api.CG_BT2100)
    yi = api.yuv420_image(yp, W, H, api.CG_BT709)
    res["jpegr_encode_api2 %s planes" % name] = timed(lambda: lib.uhdr_hip_jpegr_encode_api2(C.byref(pi), C.byref(yi), jp, jpg.size, api.CG_BT709, api.TF_HLG, fo, fout.size, C.byref(n), mem, None), 10)
    res["jpegr_encode_api3 %s planes" % name] = timed(lambda: lib.uhdr_hip_jpegr_encode_api3(C.byref(pi), jp, jpg.size, api.CG_BT709, api.TF_HLG, fo, fout.size, C.byref(n), mem, None), 10)
    gm = torch.zeros((W // 4) * (H // 4), dtype=torch.uint8, device="cuda")
    hgm = np.zeros((W // 4) * (H // 4), np.uint8)
    gi = api.Image(gm.data_ptr() if mem == api.MEM_DEVICE else hgm.ctypes.data, W // 4, H // 4, api.CG_UNSPECIFIED, None, W // 4, 0, api.PIX_FMT_MONOCHROME)
    md = api.metadata(4.0, 1.0)
    md.hdrCapacityMin, md.hdrCapacityMax = 1.0, 4.0
    res["jpegr_encode_apix %s planes" % name] = timed(lambda: lib.uhdr_hip_jpegr_encode_apix(C.byref(yi), C.byref(gi), C.byref(md), 95, None, 0, fo, fout.size, C.byref(n), mem, None), 10)
fm = api.Image()
fmd = api.Metadata()
assert lib.uhdr_hip_jpegr_encode_api2(C.byref(api.p010_image(p.data_ptr(), W, H, api.CG_BT2100)), C.byref(api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709)), jp, jpg.size, api.CG_BT709, api.TF_HLG, fo, fout.size, C.byref(n), api.MEM_DEVICE, None) == 0
jr = fout[:n.value].copy()
res["jpegr_decode SDR -> device"] = timed(lambda: lib.uhdr_hip_jpegr_decode(C.c_void_p(jr.ctypes.data), jr.size, api.OUTPUT_SDR, api.FLT_MAX, C.c_void_p(dpl.data_ptr()), dpl.numel(), C.byref(fm), C.byref(fmd), api.APPLY_FAST, api.MEM_DEVICE, None))
for k, v in res.items():
    print("SINGLE %-48s %9.3f ms" % (k, v), flush=True)
