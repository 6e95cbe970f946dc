"""GPU: uhdr_hip_jpeg_decode_batch and uhdr_hip_jpeg_encode_batch against loops of single calls in the same process: smooth 4K frames,
q95, n in {1, 4, 16, 64} (or the n given with --n), a distinct frame per file.  Four forms, wall ms per file (every call returns with
its outputs in place):
  decode YCBCR, device outputs    uhdr_hip_jpeg_decode_batch       against uhdr_hip_jpeg_decode
  decode RGBA, device outputs     uhdr_hip_jpeg_decode_batch       against uhdr_hip_jpeg_decode_rgba
  encode, device planes -> host   uhdr_hip_jpeg_encode_batch       against uhdr_hip_jpeg_encode into device memory + the copy down
  encode, device planes -> device uhdr_hip_jpeg_encode_batch       against uhdr_hip_jpeg_encode
Run under rocprofv3 --kernel-trace --stats (with --n 16) for the kernels' split."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from libultrahdr_dev_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[1, 4, 16, 64])
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

lib = api.init(0)
W, H = 3840, 2160
NMAX = max(args.n)
YCC = W * H * 3 // 2
frames = [synth.smooth_frame(W, H, 300 + i)[1] for i in range(NMAX)]
imgs = [api.Image(y.data_ptr(), W, H, api.CG_UNSPECIFIED, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420) for y in frames]
CAP = W * H * 2
host_out = [torch.empty(CAP, dtype=torch.uint8, pin_memory=True) for _ in range(NMAX)]
dev_out = [torch.empty(CAP, dtype=torch.uint8, device="cuda") for _ in range(NMAX)]
torch.cuda.synchronize()
S = C.c_void_p(torch.cuda.current_stream().cuda_stream)

# the files: each frame compressed once at q95
files = []
for i in range(NMAX):
    n = C.c_size_t()
    assert lib.uhdr_hip_jpeg_encode(C.byref(imgs[i]), 95, None, 0, C.c_void_p(dev_out[i].data_ptr()), CAP, C.byref(n), api.MEM_DEVICE, S) == 0
    files.append(np.frombuffer(dev_out[i][:n.value].cpu().numpy().tobytes() + b"\0" * 8, np.uint8))
dec_out = [torch.empty(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(NMAX)]


def timed(fn, iters):
    for _ in range(2):
        assert fn() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


print("4K smooth frames, q95, %d bytes per file (first)" % (files[0].size - 8), flush=True)
for n in args.n:
    iters = max(2, args.iters * 4 // max(n, 4))
    jp = (C.c_void_p * n)(*[f.ctypes.data for f in files[:n]])
    js = (C.c_size_t * n)(*[f.size - 8 for f in files[:n]])
    status = (C.c_int * n)()
    descs = (api.Image * n)()
    d = api.Image()
    for rgba in (False, True):
        need = W * H * 4 if rgba else YCC
        optr = (C.c_void_p * n)(*[t.data_ptr() for t in dec_out[:n]])
        ocap = (C.c_size_t * n)(*[need] * n)
        single = lib.uhdr_hip_jpeg_decode_rgba if rgba else lib.uhdr_hip_jpeg_decode

        def batch():
            return lib.uhdr_hip_jpeg_decode_batch(n, jp, js, api.DECODE_TO_RGBA if rgba else api.DECODE_TO_YCBCR, optr, ocap, descs, status,
                                                  api.MEM_DEVICE, S)

        def singles():
            for i in range(n):
                rc = single(C.c_void_p(files[i].ctypes.data), files[i].size - 8, C.c_void_p(dec_out[i].data_ptr()), need, C.byref(d), api.MEM_DEVICE, S)
                if rc != 0:
                    return rc
            return 0

        ts, tb = timed(singles, iters), timed(batch, iters)
        print("decode %-5s n=%2d: batch %.3f ms per file (%.3f ms per call), single-call loop %.3f ms per file, speed-up %.2fx"
              % ("RGBA" if rgba else "YCBCR", n, tb / n, tb, ts / n, ts / tb), flush=True)
    for to_host in (True, False):
        outs = host_out if to_host else dev_out
        optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs[:n]])
        ocap = (C.c_size_t * n)(*[CAP] * n)
        size = (C.c_size_t * n)()
        q = (C.c_int * n)(*[95] * n)
        I = api.image_array(imgs[:n])
        sz = C.c_size_t()

        def batch():
            return lib.uhdr_hip_jpeg_encode_batch(n, I, q, None, None, optr, ocap, size, status, api.MEM_DEVICE_TO_HOST if to_host else api.MEM_DEVICE, S)

        def singles():
            for i in range(n):
                rc = lib.uhdr_hip_jpeg_encode(C.byref(imgs[i]), 95, None, 0, C.c_void_p(dev_out[i].data_ptr()), CAP, C.byref(sz), api.MEM_DEVICE, S)
                if rc != 0:
                    return rc
                if to_host:   # the single call's host form needs host planes: device memory, then the file down
                    host_out[i][:sz.value].copy_(dev_out[i][:sz.value])
            return 0

        ts, tb = timed(singles, iters), timed(batch, iters)
        print("encode %-6s n=%2d: batch %.3f ms per file (%.3f ms per call), single-call loop %.3f ms per file, speed-up %.2fx"
              % ("host" if to_host else "device", n, tb / n, tb, ts / n, ts / tb), flush=True)
