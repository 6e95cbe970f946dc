"""GPU: what the per-image MCU shape costs the 4:2:0 decode, and what the other samplings cost (profiles/r06_jpeg_sampling.txt).

    python scripts/time_jpeg_sampling.py [--parent path/to/parent/libuhdr_hip.so] [--runs 7]

A/B (with --parent: the library built from the parent commit, loaded next to this one in the same process): uhdr_hip_jpeg_decode of
the 4K quality-95 file of scripts/time_jpeg_dec.py and uhdr_hip_jpeg_decode_batch of 16 such files, the two libraries alternating,
`runs` runs each (a run: the median of 10 calls, resp. of 5 batch calls); medians and the spread (min .. max) of the runs.
For information: 4K decode of Pillow-written 4:4:4, 4:2:2 and 4:2:0 files (Pillow writes no 4:4:0) at quality 75 and 95
through uhdr_hip_jpeg_decode_ex, and a 4K applyGainMap over 4:4:4 planes (general per-pixel kernel) beside 4:2:0 (scale-4 kernel)."""
import argparse
import ctypes as C
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from libultrahdr_dev_amd import api, synth

W, H = 3840, 2160


def bind(path):
    """the decode calls of a library of either commit (the parent's has no *_ex symbols: api.load() would refuse it)"""
    lib = C.CDLL(path)
    for name in ("uhdr_hip_init", "uhdr_hip_jpeg_decode", "uhdr_hip_jpeg_decode_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = api.SIGNATURES[name]
    assert lib.uhdr_hip_init(0) == 0
    return lib


def median_us(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def report(label, runs):
    print("%-44s median %9.1f us   spread %9.1f .. %9.1f us   runs %s" % (label, statistics.median(runs), min(runs), max(runs), " ".join("%.0f" % r for r in runs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--ab-only", action="store_true", help="stop after the 4:2:0 A/B (pass this commit's own library as --parent for an A/A)")
    args = ap.parse_args()
    lib = api.init(0)
    libs = [("this commit", lib)]
    if args.parent:
        libs.insert(0, ("parent commit", bind(args.parent)))
    print("device: %s" % torch.cuda.get_device_name(0))

    # the files: 16 smooth 4K frames, quality 95, from the device encoder (the first is scripts/time_jpeg_dec.py's)
    out = torch.zeros(W * H * 2, dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    files, frames = [], []
    for k in range(16):
        _, y = synth.smooth_frame(W, H, 77 + k)
        img = api.Image(y.data_ptr(), W, H, api.CG_BT709, y.data_ptr() + W * H, W, W // 2, api.PIX_FMT_YUV420)
        assert lib.uhdr_hip_jpeg_encode(C.byref(img), 95, None, 0, C.c_void_p(out.data_ptr()), out.numel(), C.byref(n), api.MEM_DEVICE, None) == 0
        files.append(out[:n.value].cpu().numpy().copy())
        if k == 0:
            frames.append(y.cpu().numpy())
    planes = [torch.zeros(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(16)]
    desc = api.Image()

    def single(L):
        return lambda: L.uhdr_hip_jpeg_decode(C.c_void_p(files[0].ctypes.data), files[0].size, C.c_void_p(planes[0].data_ptr()), planes[0].numel(), C.byref(desc),
                                              api.MEM_DEVICE, None)
    jp = (C.c_void_p * 16)(*[f.ctypes.data for f in files])
    js = (C.c_size_t * 16)(*[f.size for f in files])
    op = (C.c_void_p * 16)(*[p.data_ptr() for p in planes])
    oc = (C.c_size_t * 16)(*[p.numel() for p in planes])
    descs, stat = (api.Image * 16)(), (C.c_int * 16)()

    def batch(L):
        return lambda: L.uhdr_hip_jpeg_decode_batch(16, jp, js, api.DECODE_TO_YCBCR, op, oc, descs, stat, api.MEM_DEVICE, None)
    print("\n== no regression on 4:2:0: 4K quality-95 file (%d bytes), alternating libraries, %d runs each ==" % (files[0].size, args.runs))
    want = None
    for label, L in libs:   # warm-up, and both libraries decode the same bytes
        for _ in range(3):
            assert single(L)() == 0 and batch(L)() == 0
        got = planes[0].cpu().numpy().copy()
        assert want is None or np.array_equal(got, want)
        want = got
    res = {(label, kind): [] for label, _ in libs for kind in ("single", "batch")}
    for _ in range(args.runs):
        for label, L in libs:
            res[(label, "single")].append(median_us(single(L), 10))
        for label, L in libs:
            res[(label, "batch")].append(median_us(batch(L), 5))
    for kind, what in (("single", "uhdr_hip_jpeg_decode, one file"), ("batch", "uhdr_hip_jpeg_decode_batch, 16 files")):
        for label, _ in libs:
            report("%s [%s]" % (what, label), res[(label, kind)])
        if len(libs) == 2:
            a, b = statistics.median(res[(libs[0][0], kind)]), statistics.median(res[(libs[1][0], kind)])
            pr = res[(libs[0][0], kind)]
            print("  this / parent = %.4f   (parent's own spread: %.4f .. %.4f of its median)" % (b / a, min(pr) / a, max(pr) / a))

    if args.ab_only:
        return 0

    # the other samplings, for information: the same frame written by Pillow (libjpeg-turbo)
    from PIL import Image
    hy = frames[0]
    Y = hy[:W * H].reshape(H, W)
    U = np.repeat(np.repeat(hy[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), 2, 0), 2, 1)
    V = np.repeat(np.repeat(hy[W * H * 5 // 4:].reshape(H // 2, W // 2), 2, 0), 2, 1)
    ycc = Image.fromarray(np.stack([Y, U, V], -1), mode="YCbCr")
    big = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
    print("\n== 4K decode by sampling (Pillow-written files of the same frame; uhdr_hip_jpeg_decode_ex, device memory, median of 10) ==")
    kept = {}
    for q in (75, 95):
        for sub, name in ((2, "4:2:0"), (1, "4:2:2"), (0, "4:4:4")):
            b = io.BytesIO()
            ycc.save(b, "JPEG", quality=q, subsampling=sub)
            data = np.frombuffer(b.getvalue(), np.uint8).copy()

            def dec():
                return lib.uhdr_hip_jpeg_decode_ex(C.c_void_p(data.ctypes.data), data.size, api.DECODE_TO_YCBCR, C.c_void_p(big.data_ptr()), big.numel(), C.byref(desc),
                                                   api.MEM_DEVICE, None, api.DECODE_ANY_SAMPLING)
            for _ in range(3):
                assert dec() == 0
            if sub == 0:   # the whole 4K frame is there: 4:4:4 planes are what libjpeg-turbo hands Pillow undecoded
                im = Image.open(io.BytesIO(b.getvalue()))
                im.draft("YCbCr", (W, H))
                want = np.asarray(im)
                got = big[:W * H * 3].cpu().numpy().reshape(3, H, W)
                assert all(np.array_equal(got[c], want[:, :, c]) for c in range(3)), "4K 4:4:4 planes differ from Pillow's"
            print("quality %d  %s  %9d bytes   %9.1f us%s" % (q, name, data.size, median_us(dec, 10), "   (planes equal Pillow's)" if sub == 0 else ""))
            if q == 95:
                kept[name] = big[:W * H * 3].clone()

    print("\n== 4K applyGainMap, APPLY_FAST, HLG 1010102, device memory (median of 20, stream synchronised) ==")
    gmap = torch.randint(0, 256, ((W // 4) * (H // 4),), dtype=torch.uint8, device="cuda")
    dout = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    md = api.metadata(4.0)
    mimg, dest = api.mono_image(gmap.data_ptr(), W // 4, H // 4), api.out_image(dout.data_ptr())
    for name, img in (("4:2:0 (scale-4 kernel)", api.yuv420_image(kept["4:2:0"].data_ptr(), W, H, api.CG_BT709)),
                      ("4:4:4 (general per-pixel kernel)", api.ycbcr_image(kept["4:4:4"].data_ptr(), W, H, api.CG_BT709, api.PIX_FMT_YUV444)),
                      ("4:2:2 (general per-pixel kernel)", api.ycbcr_image(kept["4:2:2"].data_ptr(), W, H, api.CG_BT709, api.PIX_FMT_YUV422))):
        def app():
            rc = lib.uhdr_hip_apply_gainmap(C.byref(img), C.byref(mimg), C.byref(md), api.OUTPUT_HDR_HLG, api.FLT_MAX, C.byref(dest), api.APPLY_FAST, api.MEM_DEVICE, None)
            torch.cuda.synchronize()
            return rc
        for _ in range(3):
            assert app() == 0
        print("%-36s %9.1f us" % (name, median_us(app, 20)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
