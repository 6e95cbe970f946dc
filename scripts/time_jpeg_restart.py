"""GPU: what restart intervals cost the encoder and what the files they make give this library's decoder, in one process: 64 smooth
3840x2160 frames (a distinct frame per file) at quality 95, device planes into device memory, one call for all 64.
Encode, wall ms per file (median and spread of --repeats timed loops, every call returning with its outputs in place):
  no intervals     through uhdr_hip_jpeg_encode_batch_ex and through uhdr_hip_jpeg_encode_batch_opts with zero options
  restart_in_rows = 1, restart_interval = 8, restart_interval = 1, each with and without UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN
and the mean file size.  Decode (uhdr_hip_jpeg_decode_batch to YCbCr in device memory, the files in host memory), ms per file, of
the files each setting wrote: the first one alone, and the first 16 as one batch."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from libultrahdr_dev_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

lib = api.init(0)
W, H, Q = 3840, 2160, 95
N = args.n
S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
frames = [synth.smooth_frame(W, H, 300 + i)[1] for i in range(N)]
torch.cuda.synchronize()
imgs = api.image_array([api.Image(y.data_ptr(), W, H, api.CG_UNSPECIFIED, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420) for y in frames])
cap = W * H * 2
outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
q = (C.c_int * N)(*[Q] * N)
optr = (C.c_void_p * N)(*[t.data_ptr() for t in outs])
ocap = (C.c_size_t * N)(*[cap] * N)
size, status = (C.c_size_t * N)(), (C.c_int * N)()


def timed(fn, iters):
    for _ in range(2):
        assert fn() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def spread(fn, iters, per):
    t = [timed(fn, iters) / per for _ in range(args.repeats)]
    return "%.3f (%.3f .. %.3f)" % (statistics.median(t), min(t), max(t)), statistics.median(t)


def decode_times(files):
    """ms per file: files[0] alone, and all of them as one batch"""
    res = []
    for group in (files[:1], files):
        n = len(group)
        bufs = [torch.frombuffer(bytearray(f + b"\0" * 8), dtype=torch.uint8) for f in group]
        jp = (C.c_void_p * n)(*[b.data_ptr() for b in bufs])
        js = (C.c_size_t * n)(*[len(f) for f in group])
        dst = [torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(n)]
        dp = (C.c_void_p * n)(*[t.data_ptr() for t in dst])
        dc = (C.c_size_t * n)(*[W * H * 3 // 2] * n)
        descs, st = (api.Image * n)(), (C.c_int * n)()

        def call():
            return lib.uhdr_hip_jpeg_decode_batch(n, jp, js, api.DECODE_TO_YCBCR, dp, dc, descs, st, api.MEM_DEVICE, S)
        res.append(spread(call, max(2, 16 // n), n))
    return res


SETTINGS = [("ex, flags 0", None, 0), ("opts, zero", (0, 0), 0), ("ex, OPTIMIZE", None, 1), ("opts, zero, OPTIMIZE", (0, 0), 1)]
for opt in (0, 1):
    SETTINGS += [("rows = 1%s" % (", OPTIMIZE" if opt else ""), (0, 1), opt), ("interval = 8%s" % (", OPTIMIZE" if opt else ""), (8, 0), opt),
                 ("interval = 1%s" % (", OPTIMIZE" if opt else ""), (1, 0), opt)]
print("%d x %dx%d q%d, one call; ms per file, median (min .. max) of %d loops of %d calls" % (N, W, H, Q, args.repeats, args.iters))
print("%-26s %-28s %10s   %-28s %-28s" % ("setting", "encode", "bytes/file", "decode, 1 file", "decode, 16 files"))
base = {}
for name, rst, opt in SETTINGS:
    flags = api.ENCODE_OPTIMIZE_HUFFMAN if opt else 0
    if rst is None:
        def call():
            return lib.uhdr_hip_jpeg_encode_batch_ex(N, imgs, q, None, None, optr, ocap, size, status, flags, api.MEM_DEVICE, S)
    else:
        o = api.encode_opts(flags, rst[0], rst[1])

        def call():
            return lib.uhdr_hip_jpeg_encode_batch_opts(N, imgs, q, None, None, optr, ocap, size, status, C.byref(o), api.MEM_DEVICE, S)
    enc, med = spread(call, args.iters, N)
    assert all(status[k] == 0 for k in range(N))
    torch.cuda.synchronize()
    nbytes = sum(size[k] for k in range(N)) // N
    files = [outs[k][:size[k]].cpu().numpy().tobytes() for k in range(min(16, N))]
    (d1, m1), (d16, m16) = decode_times(files)
    base.setdefault(opt, (med, m1, m16))
    e0, a0, b0 = base[opt]
    print("%-26s %-28s %10d   %-28s %-28s  encode %+.3f, decode %+.3f / %+.3f ms per file against no intervals" % (
        name, enc, nbytes, d1, d16, med - e0, m1 - a0, m16 - b0), flush=True)
