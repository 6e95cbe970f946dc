"""GPU: what the encoder's samplings cost, in one process: 16 smooth frames (a distinct frame per file) at quality 95, device inputs into
device memory, one call for all 16; wall ms per file, median and spread of --repeats timed loops.

    (default)      3840x2160 and 1920x1080: planes as 4:2:0 (uhdr_hip_jpeg_encode_batch), 4:4:4, 4:2:2, 4:4:0
                   (uhdr_hip_jpeg_encode_planes_batch_opts); RGBA8888 as 4:2:0 (uhdr_hip_jpeg_encode_rgba420_batch), 4:4:4, 4:2:2
                   (uhdr_hip_jpeg_encode_rgba_batch_opts); blocks per file and mean file size beside each
    --regression   the calls that existed before, at 3840x2160: uhdr_hip_jpeg_encode_batch_opts and uhdr_hip_jpeg_encode_rgba420_batch_opts
                   with default tables, optimised tables and restart_in_rows = 1.  --lib FILE times another build of the library (the
                   parent commit's) with the same code: run the two alternately and compare the series.
"""
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
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--regression", action="store_true")
ap.add_argument("--lib", default=None, help="a libuhdr_hip.so to time instead of the package's (entry points it lacks are not bound)")
ap.add_argument("--tag", default="this build")
args = ap.parse_args()

if args.lib:
    probe = C.CDLL(args.lib)
    api.SIGNATURES = {k: v for k, v in api.SIGNATURES.items() if hasattr(probe, k)}
    api.LIB_PATH = args.lib
lib = api.init(0)
N, Q = args.n, 95
S = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, iters):
    for _ in range(2):
        assert fn() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def spread(fn, per):
    t = [timed(fn, args.iters) / per for _ in range(args.repeats)]
    return statistics.median(t), min(t), max(t)


class Inputs:
    """N frames of w x h in device memory: 4:2:0 planes, the same content as planes of the other samplings, and as RGBA8888 pixels"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.keep = []
        self.desc = {k: [] for k in ("420", "444", "422", "440", "rgba")}
        for i in range(N):
            yuv = synth.smooth_frame(w, h, 300 + i)[1]
            y = yuv[:w * h].view(h, w)
            u, v = yuv[w * h:w * h + w * h // 4].view(h // 2, w // 2), yuv[w * h + w * h // 4:].view(h // 2, w // 2)
            self.keep.append(yuv)
            self.desc["420"].append(api.Image(yuv.data_ptr(), w, h, api.CG_UNSPECIFIED, yuv.data_ptr() + w * h, w, w // 2, api.PIX_FMT_YUV420))
            for name, fmt, rx, ry in (("444", api.PIX_FMT_YUV444, 2, 2), ("422", api.PIX_FMT_YUV422, 1, 2), ("440", api.PIX_FMT_YUV440, 2, 1)):
                up = lambda c: c.repeat_interleave(ry, 0).repeat_interleave(rx, 1).contiguous().view(-1)   # noqa: E731
                t = torch.cat([y.reshape(-1), up(u), up(v)])
                self.keep.append(t)
                self.desc[name].append(api.ycbcr_image(t.data_ptr(), w, h, api.CG_UNSPECIFIED, fmt))
            up2 = lambda c: c.repeat_interleave(2, 0).repeat_interleave(2, 1)   # noqa: E731
            px = torch.stack([y, up2(u), up2(v), torch.full_like(y, 255)], dim=2).contiguous()
            self.keep.append(px)
            self.desc["rgba"].append(api.rgba8888_image(px.data_ptr(), w, h, api.CG_BT709, w))
        torch.cuda.synchronize()
        self.cap = w * h * 3
        self.outs = [torch.empty(self.cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        self.q = (C.c_int * N)(*[Q] * N)
        self.optr = (C.c_void_p * N)(*[t.data_ptr() for t in self.outs])
        self.ocap = (C.c_size_t * N)(*[self.cap] * N)
        self.size, self.status = (C.c_size_t * N)(), (C.c_int * N)()

    def call(self, kind, sampling=None, opts=None):
        imgs = api.image_array(self.desc[kind])
        o = None if opts is None else C.byref(opts)
        a = (N, imgs, self.q, None, None, self.optr, self.ocap, self.size, self.status)
        if kind == "rgba" and sampling is None:
            return lambda: lib.uhdr_hip_jpeg_encode_rgba420_batch_opts(*a, o, api.MEM_DEVICE, S)
        if kind == "rgba":
            return lambda: lib.uhdr_hip_jpeg_encode_rgba_batch_opts(*a, sampling, o, api.MEM_DEVICE, S)
        if kind == "420":
            return lambda: lib.uhdr_hip_jpeg_encode_batch_opts(*a, o, api.MEM_DEVICE, S)
        return lambda: lib.uhdr_hip_jpeg_encode_planes_batch_opts(*a, o, api.MEM_DEVICE, S)

    def mean_size(self):
        assert all(self.status[k] == 0 for k in range(N))
        return sum(self.size[k] for k in range(N)) // N


def blocks(w, h, hs, vs):
    return ((w + 8 * hs - 1) // (8 * hs)) * ((h + 8 * vs - 1) // (8 * vs)) * (hs * vs + 2)


if args.regression:
    inp = Inputs(3840, 2160)
    for kind in ("420", "rgba"):
        for name, o in (("default tables", None), ("optimised tables", api.encode_opts(api.ENCODE_OPTIMIZE_HUFFMAN)), ("restart rows = 1", api.encode_opts(0, 0, 1))):
            med, lo, hi = spread(inp.call(kind, None, o), N)
            print("REG %-12s %-34s %-18s %.4f (%.4f .. %.4f) ms per file, %d bytes" % (
                args.tag, "uhdr_hip_jpeg_encode_batch" if kind == "420" else "uhdr_hip_jpeg_encode_rgba420_batch", name, med, lo, hi, inp.mean_size()), flush=True)
    sys.exit(0)

print("%d files per call, q%d, device to device; ms per file, median (min .. max) of %d loops of %d calls" % (N, Q, args.repeats, args.iters))
for w, h in ((3840, 2160), (1920, 1080)):
    inp = Inputs(w, h)
    base = None
    rows = [("planes 4:2:0 (encode_batch)", "420", None, (2, 2)), ("planes 4:4:4", "444", None, (1, 1)), ("planes 4:2:2", "422", None, (2, 1)),
            ("planes 4:4:0", "440", None, (1, 2)), ("RGBA -> 4:2:0 (rgba420_batch)", "rgba", None, (2, 2)),
            ("RGBA -> 4:4:4", "rgba", api.PIX_FMT_YUV444, (1, 1)), ("RGBA -> 4:2:2", "rgba", api.PIX_FMT_YUV422, (2, 1))]
    for name, kind, sampling, (hs, vs) in rows:
        med, lo, hi = spread(inp.call(kind, sampling), N)
        nb = blocks(w, h, hs, vs)
        if base is None:
            base = (med, nb)
        print("%dx%d %-30s %.3f (%.3f .. %.3f)  %8d blocks (%.2fx)  time %.2fx of planes 4:2:0  %9d bytes/file" % (
            w, h, name, med, lo, hi, nb, nb / base[1], med / base[0], inp.mean_size()), flush=True)
    del inp
    torch.cuda.empty_cache()
