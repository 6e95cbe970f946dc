"""GPU: what progressive files cost the encoder, in one process: smooth 3840x2160 frames at quality 95 (4:2:0) and smooth 960x540
single planes at quality 85 (a gain map's size), a distinct image per file, device planes into device memory, 1 and 16 files per call.
Wall ms per file (median and spread of --repeats timed loops, every call returning with its outputs in place) and the mean file size of
  default       uhdr_hip_jpeg_encode_planes_batch_scans, UHDR_HIP_SCANS_BASELINE, no options (the existing default path)
  optimised     the same with UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN (the existing optimised path)
  progressive   UHDR_HIP_SCANS_PROGRESSIVE
and, for scale, Pillow's progressive write of the first image of each kind on one host core (from decoded pixels; its colour conversion
is part of its time).  --only NAME times one row alone.  --lib PATH times the default and optimised rows through another build of the library in the same process (the
A/B against the parent commit: its _opts call)."""
import argparse
import ctypes as C
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from libultrahdr_dev_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--lib", default=None)
ap.add_argument("--no-pillow", action="store_true")
ap.add_argument("--only", default=None, help="time this row alone (a kernel trace of one path)")
args = ap.parse_args()

lib = api.init(0)
S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
PROG, BASE = api.SCANS_PROGRESSIVE, api.SCANS_BASELINE


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


other = None
if args.lib:
    other = C.CDLL(args.lib)
    other.uhdr_hip_init.restype = C.c_int
    assert other.uhdr_hip_init(0) == 0
    other.uhdr_hip_jpeg_encode_planes_batch_opts.restype = C.c_int
    other.uhdr_hip_jpeg_encode_planes_batch_opts.argtypes = api.SIGNATURES["uhdr_hip_jpeg_encode_planes_batch_opts"][1]

print("ms per file, median (min .. max) of %d loops of %d calls; device planes into device memory" % (args.repeats, args.iters))
for kind, (W, H, Q, gray) in (("4K 4:2:0 q95", (3840, 2160, 95, False)), ("960x540 one plane q85", (960, 540, 85, True))):
    frames = [synth.smooth_frame(W, H, 300 + i)[1] for i in range(16)]
    torch.cuda.synchronize()
    if gray:
        descs = [api.Image(y.data_ptr(), W, H, api.CG_UNSPECIFIED, None, W, 0, api.PIX_FMT_MONOCHROME) for y in frames]
    else:
        descs = [api.Image(y.data_ptr(), W, H, api.CG_UNSPECIFIED, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420) for y in frames]
    cap = W * H * 2
    outs = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(16)]
    for N in (1, 16):
        imgs = api.image_array(descs[:N])
        q = (C.c_int * N)(*[Q] * N)
        optr = (C.c_void_p * N)(*[t.data_ptr() for t in outs[:N]])
        ocap = (C.c_size_t * N)(*[cap] * N)
        size, status = (C.c_size_t * N)(), (C.c_int * N)()
        opt = api.encode_opts(api.ENCODE_OPTIMIZE_HUFFMAN)
        rows = [("default", lambda: lib.uhdr_hip_jpeg_encode_planes_batch_scans(N, imgs, q, None, None, optr, ocap, size, status, None, BASE, api.MEM_DEVICE, S)),
                ("optimised", lambda: lib.uhdr_hip_jpeg_encode_planes_batch_scans(N, imgs, q, None, None, optr, ocap, size, status, C.byref(opt), BASE,
                                                                                   api.MEM_DEVICE, S)),
                ("progressive", lambda: lib.uhdr_hip_jpeg_encode_planes_batch_scans(N, imgs, q, None, None, optr, ocap, size, status, None, PROG,
                                                                                     api.MEM_DEVICE, S))]
        if other is not None:
            rows += [("default, --lib", lambda: other.uhdr_hip_jpeg_encode_planes_batch_opts(N, imgs, q, None, None, optr, ocap, size, status, None,
                                                                                              api.MEM_DEVICE, S)),
                     ("optimised, --lib", lambda: other.uhdr_hip_jpeg_encode_planes_batch_opts(N, imgs, q, None, None, optr, ocap, size, status, C.byref(opt),
                                                                                                api.MEM_DEVICE, S))]
        sizes = {}
        if args.only:
            rows = [r for r in rows if r[0] == args.only]
        for name, call in rows:
            txt, med = spread(call, args.iters, N)
            assert all(status[k] == 0 for k in range(N)), list(status)
            sizes[name] = sum(size[k] for k in range(N)) // N
            extra = ""
            if name == "progressive" and "optimised" in sizes:
                extra = "  %+.2f %% bytes against optimised" % (100.0 * (sizes[name] - sizes["optimised"]) / sizes["optimised"])
            print("%-22s %2d per call  %-18s %-28s %10d bytes/file%s" % (kind, N, name, txt, sizes[name], extra), flush=True)
    if not args.no_pillow:
        from PIL import Image
        torch.cuda.synchronize()
        f = outs[0][:size[0]].cpu().numpy().tobytes()
        im = Image.open(io.BytesIO(f))
        im.load()
        t = []
        for _ in range(3):
            b = io.BytesIO()
            t0 = time.perf_counter()
            im.save(b, "JPEG", quality=Q, progressive=True, subsampling=-1 if gray else 2)
            t.append((time.perf_counter() - t0) * 1e3)
        print("%-22s Pillow progressive=True on one host core: %.1f ms, %d bytes" % (kind, statistics.median(t), len(b.getvalue())), flush=True)
