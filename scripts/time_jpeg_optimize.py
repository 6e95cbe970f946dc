"""GPU: what UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN costs and what it saves, on the benchmark's own frames: the smooth 3840x2160 frame at
quality 95 and its 960x540 gain map at quality 85, one file per call and 16 per call (a distinct frame per file), device planes
into device memory.  Per form: wall ms per file with and without the flag (median and spread of --repeats timed loops, every
call returning with its outputs in place), their ratio, and the bytes of both files.
Run under rocprofv3 --kernel-trace --stats (with --repeats 1) for the split over the k_jpeg_opt_* launches."""
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
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

lib = api.init(0)
W, H = 3840, 2160
N = 16
S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
frames, maps = [], []
for i in range(N):
    p010, yuv = synth.smooth_frame(W, H, 300 + i)
    gm = torch.empty((W // 4) * (H // 4), dtype=torch.uint8, device="cuda")
    md = api.Metadata()
    dest = api.out_image(gm.data_ptr())
    yi = api.yuv420_image(yuv.data_ptr(), W, H, api.CG_BT709)
    pi = api.p010_image(p010.data_ptr(), W, H, api.CG_BT2100)
    assert lib.uhdr_hip_generate_gainmap(C.byref(yi), C.byref(pi), api.TF_HLG, C.byref(md), C.byref(dest), 0, api.MEM_DEVICE, S) == 0
    frames.append(yuv)
    maps.append(gm)
torch.cuda.synchronize()
FORMS = {
    "4K frame q95": ([api.Image(y.data_ptr(), W, H, api.CG_UNSPECIFIED, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420) for y in frames], 95, W * H * 2),
    "960x540 map q85": ([api.mono_image(m.data_ptr(), W // 4, H // 4) for m in maps], 85, W * H // 4),
}


def timed(fn, iters):
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


for name, (imgs, quality, cap) in FORMS.items():
    outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
    for n in (1, N):
        I = api.image_array(imgs[:n])
        q = (C.c_int * n)(*[quality] * n)
        optr = (C.c_void_p * n)(*[t.data_ptr() for t in outs[:n]])
        ocap = (C.c_size_t * n)(*[cap] * n)
        size, status = (C.c_size_t * n)(), (C.c_int * n)()
        res = {}
        for flags in (0, api.ENCODE_OPTIMIZE_HUFFMAN):
            def call():
                return lib.uhdr_hip_jpeg_encode_batch_ex(n, I, q, None, None, optr, ocap, size, status, flags, api.MEM_DEVICE, S)
            iters = max(3, args.iters // n)
            t = [timed(call, iters) / n for _ in range(args.repeats)]
            res[flags] = (statistics.median(t), min(t), max(t), sum(size[k] for k in range(n)) // n)
        (t0, lo0, hi0, b0), (t1, lo1, hi1, b1) = res[0], res[api.ENCODE_OPTIMIZE_HUFFMAN]
        print("%-16s n=%2d: default %.3f ms per file (%.3f .. %.3f), optimised %.3f ms per file (%.3f .. %.3f), ratio %.2f; "
              "%d -> %d bytes per file (-%d, %.1f %%)" % (name, n, t0, lo0, hi0, t1, lo1, hi1, t1 / t0, b0, b1, b0 - b1, 100.0 * (b0 - b1) / b0), flush=True)
