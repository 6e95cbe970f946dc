"""GPU: what a decode at 1/2, 1/4 and 1/8 costs beside the full-size decode (profiles/r19_jpeg_scaled.txt).

    python scripts/time_jpeg_scaled.py [--parent path/to/parent/libuhdr_hip.so] [--runs 3] [--out profiles/r19_jpeg_scaled.txt]

One process, one box.  A run is the median of `calls` calls; every line gives the median of the runs and their spread (min .. max).
  1. a 4K quality-95 4:2:0 file (scripts/time_jpeg_dec.py's) through uhdr_hip_jpeg_decode_batch_scaled at 1, 1/2, 1/4, 1/8: planes
     and RGBA into device memory;
  2. the same for a UHDR_HIP_MEM_HOST caller;
  3. a batch of 16 4K JPEG/R files (API-1, quality 95) to HDR_PQ through uhdr_hip_jpegr_decode_scaled_batch at the four denominators,
     device memory, APPLY_FAST.
With --parent (the library built from the parent commit, loaded next to this one): its uhdr_hip_jpeg_decode_batch_ex and
uhdr_hip_jpegr_decode_md_batch on the same inputs, alternating with this commit's calls at denominator 1."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from libultrahdr_dev_amd import api, synth

W, H = 3840, 2160
FLT_MAX = 3.4028234663852886e38
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def bind(path):
    lib = C.CDLL(path)
    for name in ("uhdr_hip_init", "uhdr_hip_jpeg_decode_batch_ex", "uhdr_hip_jpegr_decode_md_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = api.SIGNATURES[name]
    assert lib.uhdr_hip_init(0) == 0
    return lib


def median_us(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        assert fn() == 0
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def measure(label, fns, runs, calls):
    """fns: [(name, callable)] measured alternately, `runs` runs each"""
    for _, fn in fns:
        for _ in range(3):
            assert fn() == 0
    res = {name: [] for name, _ in fns}
    for _ in range(runs):
        for name, fn in fns:
            res[name].append(median_us(fn, calls))
    for name, _ in fns:
        r = res[name]
        say("%-34s %-16s median %9.1f us   spread %9.1f .. %9.1f us   runs %s" % (label, name, statistics.median(r), min(r), max(r), " ".join("%.0f" % x for x in r)))
    return {name: statistics.median(r) for name, r in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = api.init(0)
    parent = bind(args.parent) if args.parent else None
    say("device: %s; %d runs per line" % (torch.cuda.get_device_name(0), args.runs))

    # ---- 1, 2: one 4K file
    out = torch.zeros(W * H * 2, dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    _, y = synth.smooth_frame(W, H, 77)
    img = api.Image(y.data_ptr(), W, H, api.CG_BT709, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420)
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), 95, None, 0, C.c_void_p(out.data_ptr()), out.numel(), C.byref(n), api.MEM_DEVICE, None) == 0
    data = out[:n.value].cpu().numpy().copy()
    say("file: %d x %d 4:2:0 quality 95, %d bytes" % (W, H, data.size))
    jp, js = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(data.size)
    descs, stat = (api.Image * 1)(), (C.c_int * 1)()
    dev = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    host = np.zeros(W * H * 4, np.uint8)
    for mem, buf, ptr, where in ((api.MEM_DEVICE, dev, dev.data_ptr(), "device memory"), (api.MEM_HOST, host, host.ctypes.data, "host memory")):
        op, oc = (C.c_void_p * 1)(ptr), (C.c_size_t * 1)(W * H * 4)
        for to, what in ((api.DECODE_TO_YCBCR, "planes"), (api.DECODE_TO_RGBA, "RGBA")):
            base = None
            for s in (1, 2, 4, 8):
                fns = [("this commit", lambda s=s, to=to: lib.uhdr_hip_jpeg_decode_batch_scaled(1, jp, js, to, op, oc, descs, stat, mem, None, 0, s))]
                if parent is not None and s == 1:
                    fns.insert(0, ("parent commit", lambda to=to: parent.uhdr_hip_jpeg_decode_batch_ex(1, jp, js, to, op, oc, descs, stat, mem, None, 0)))
                m = measure("4K %s, %s, 1/%d" % (what, where, s), fns, args.runs, 10)["this commit"]
                base = m if s == 1 else base
                if s != 1:
                    say("%-34s %-16s %.2f x the full-size call" % ("", "", m / base))

    # ---- 3: 16 JPEG/R files to HDR_PQ
    nfiles = 16
    blobs = []
    for i in range(nfiles):
        p, y = synth.smooth_frame(W, H, 100 + i)
        pi = api.p010_image(p.data_ptr(), W, H, api.CG_BT2100)
        yi = api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709)
        o = np.zeros(W * H * 3, np.uint8)
        assert lib.uhdr_hip_jpegr_encode_api1(C.byref(pi), C.byref(yi), api.TF_HLG, 95, None, 0, C.c_void_p(o.ctypes.data), o.size, C.byref(n), api.MEM_DEVICE, None) == 0
        blobs.append(o[:n.value].copy())
    del p, y
    ptrs = (C.c_void_p * nfiles)(*[b.ctypes.data for b in blobs])
    sizes = (C.c_size_t * nfiles)(*[b.size for b in blobs])
    outs = [torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda") for _ in range(nfiles)]
    optr = (C.c_void_p * nfiles)(*[o.data_ptr() for o in outs])
    ocap = (C.c_size_t * nfiles)(*[o.numel() for o in outs])
    dests, mds, status = (api.Image * nfiles)(), (api.Metadata * nfiles)(), (C.c_int * nfiles)()
    base = None
    for s in (1, 2, 4, 8):
        fns = [("this commit", lambda s=s: lib.uhdr_hip_jpegr_decode_scaled_batch(nfiles, ptrs, sizes, api.OUTPUT_HDR_PQ, FLT_MAX, optr, ocap, dests, mds, status,
                                                                                 api.APPLY_FAST, api.MEM_DEVICE, None, 0, s))]
        if parent is not None and s == 1:
            fns.insert(0, ("parent commit", lambda: parent.uhdr_hip_jpegr_decode_md_batch(nfiles, ptrs, sizes, api.OUTPUT_HDR_PQ, FLT_MAX, optr, ocap, dests, mds, status,
                                                                                          api.APPLY_FAST, api.MEM_DEVICE, None, 0)))
        m = measure("16 JPEG/R -> HDR_PQ, device, 1/%d" % s, fns, args.runs, 5)["this commit"]
        base = m if s == 1 else base
        if s != 1:
            say("%-34s %-16s %.2f x the full-size call (%.1f us per file)" % ("", "", m / base, m / nfiles))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
