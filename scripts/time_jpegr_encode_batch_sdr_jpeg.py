"""GPU: uhdr_hip_jpegr_encode_sdr_jpeg_batch (API-2, API-3) and uhdr_hip_jpegr_encode_apix_batch (API-x) against loops of their single
calls (uhdr_hip_jpegr_encode_api2 / _api3 / _apix) in the same process: smooth 4K frames on the device, HLG, a distinct frame per file,
the SDR JPEGs made by uhdr_hip_jpeg_encode at q95 (API-x: the SDR image at q95, the gain map a subsampled luma plane), n in
{1, 4, 16, 64} (or the n given with --n).  Wall ms per file (the call returns once the files are on the host).  Run under
rocprofv3 --kernel-trace --stats (with --n 16) for the kernels' split."""
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
ap.add_argument("--forms", nargs="*", default=["API-3", "API-2", "API-x"])
args = ap.parse_args()

lib = api.init(0)
W, H = 3840, 2160
NMAX = max(args.n)
frames = [synth.smooth_frame(W, H, 200 + i) for i in range(NMAX)]
pis = [api.p010_image(p.data_ptr(), W, H, api.CG_BT2100) for p, _ in frames]
yis = [api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709) for _, y in frames]
maps = [y[:W * H].view(H, W)[::4, ::4].contiguous() for _, y in frames]
gis = [api.Image(m.data_ptr(), W // 4, H // 4, api.CG_UNSPECIFIED, None, 0, 0, api.PIX_FMT_MONOCHROME) for m in maps]
CAP = W * H * 3
sdr = []
dbuf, sz = torch.empty(CAP, dtype=torch.uint8, device="cuda"), C.c_size_t()
for yi in yis:   # the SDR JPEGs an ISP would have written
    assert lib.uhdr_hip_jpeg_encode(C.byref(yi), 95, None, 0, C.c_void_p(dbuf.data_ptr()), CAP, C.byref(sz), api.MEM_DEVICE, None) == 0
    sdr.append(dbuf[:sz.value].cpu().numpy().copy())
outs = [np.zeros(CAP, np.uint8) for _ in range(NMAX)]
md = api.metadata(4.0)
torch.cuda.synchronize()


def timed(fn, iters):
    for _ in range(2):
        assert fn() == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


for form in args.forms:
    for n in args.n:
        P = api.image_array(pis[:n])
        Y = api.image_array(yis[:n])
        G = api.image_array(gis[:n])
        MD = (api.Metadata * n)(*[md] * n)
        J = (C.c_void_p * n)(*[j.ctypes.data for j in sdr[:n]])
        JN = (C.c_size_t * n)(*[j.size for j in sdr[:n]])
        JG = (C.c_int * n)(*[api.CG_BT709] * n)
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs[:n]])
        cap = (C.c_size_t * n)(*[CAP] * n)
        size = (C.c_size_t * n)()
        status = (C.c_int * n)()
        sz = C.c_size_t()

        def batch():
            if form == "API-x":
                return lib.uhdr_hip_jpegr_encode_apix_batch(n, Y, G, MD, 95, None, None, optr, cap, size, status, api.MEM_DEVICE, None)
            return lib.uhdr_hip_jpegr_encode_sdr_jpeg_batch(n, P, Y if form == "API-2" else None, J, JN, JG, api.TF_HLG, optr, cap, size, status,
                                                            api.MEM_DEVICE, None)

        def singles():
            for i in range(n):
                o = C.c_void_p(outs[i].ctypes.data)
                j = C.c_void_p(sdr[i].ctypes.data)
                if form == "API-3":
                    rc = lib.uhdr_hip_jpegr_encode_api3(C.byref(pis[i]), j, sdr[i].size, api.CG_BT709, api.TF_HLG, o, CAP, C.byref(sz), api.MEM_DEVICE, None)
                elif form == "API-2":
                    rc = lib.uhdr_hip_jpegr_encode_api2(C.byref(pis[i]), C.byref(yis[i]), j, sdr[i].size, api.CG_BT709, api.TF_HLG, o, CAP, C.byref(sz),
                                                        api.MEM_DEVICE, None)
                else:
                    rc = lib.uhdr_hip_jpegr_encode_apix(C.byref(yis[i]), C.byref(gis[i]), C.byref(md), 95, None, 0, o, CAP, C.byref(sz), api.MEM_DEVICE, None)
                if rc != 0:
                    return rc
            return 0

        iters = max(2, args.iters * 4 // max(n, 4))
        ts = timed(singles, iters)
        tb = timed(batch, iters)
        print("%s n=%2d 4K: batch %.3f ms per file (%.3f ms per call), single-call loop %.3f ms per file, speed-up %.2fx (%d bytes per file)"
              % (form, n, tb / n, tb, ts / n, ts / tb, size[0]), flush=True)
