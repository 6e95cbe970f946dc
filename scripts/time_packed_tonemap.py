"""Times the packed tone map on one GPU and writes profiles/r11_packed_tonemap.txt.

    python scripts/time_packed_tonemap.py [--out FILE]

In one process:
    tone map   uhdr_hip_tonemap_packed_batch on 64 x 3840x2160 images per call -- RGBA1010102 (PQ, HLG) and RGBA F16 (linear), noise, with a
               given and with a measured headroom -- beside uhdr_hip_tonemap_sdr_batch on P010 frames of the same size (the planar
               operator: the parent's code), and beside a plain device copy that moves the same bytes: 8 B/pixel for RGBA1010102 (4
               read, 4 written), 12 for RGBA F16 -- a copy reads what it writes, so 4 and 6 B/pixel are copied.  PQ RGBA1010102 is
               also timed on a smooth ramp, where neighbouring lanes read neighbouring table entries: the table gather's bank
               conflicts are the only thing that differs from the noise line.
    encode     uhdr_hip_jpegr_encode_packed_api0_batch on 16 x 3840x2160 HDR images in device memory, files to host memory, beside
               uhdr_hip_jpegr_encode_packed_batch given the same HDR images and the RGBA8888 images the tone map wrote for them.
The tone-map calls rotate over SETS resident sets, so that no launch finds its input in a cache the launch before it filled.
Tone-map times are device events around one call each, encode times a host clock around the call (it synchronises); milliseconds
per call, median [min .. max] of REPS.  GB/s are the algorithmic bytes of the given-headroom call -- every input pixel once, every
output pixel once; a measured headroom reads the input a second time, which the x-copy column does not count -- over the median."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

W, H = 3840, 2160
N, N_ENC = 64, 16
SETS, WARMUP, REPS = 3, 2, 9
HBM = 8.0e12
OP = api.TONEMAP_REINHARD_MAXRGB


def arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class Set:
    """N resident 4K frames of every layout and their destinations; every layout one allocation, so that a copy is one call"""

    def __init__(self, lib, seed, s):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        px = W * H
        self.h10 = torch.randint(-2 ** 31, 2 ** 31 - 1, (N * px,), dtype=torch.int32, device="cuda", generator=g)
        self.h16 = torch.randint(0, 0x4401, (N * px * 4,), dtype=torch.int16, device="cuda", generator=g)   # finite halves in [0, 4]
        x = torch.arange(W, device="cuda", dtype=torch.int32).repeat(H, 1)
        y = torch.arange(H, device="cuda", dtype=torch.int32).unsqueeze(1).repeat(1, W)
        ramp = (x * 1023 // (W - 1)) | ((y * 1023 // (H - 1)) << 10) | (((x + y) * 1023 // (W + H - 2)) << 20)
        self.smooth = ramp.reshape(-1).repeat(N).contiguous()
        self.rgba = torch.empty(N * px, dtype=torch.int32, device="cuda")
        self.six = torch.empty(N * px * 6, dtype=torch.uint8, device="cuda")   # the F16 line's copy: 6 B/pixel read, 6 written
        self.six_dst = torch.empty_like(self.six)
        self.p010 = torch.empty(N * px * 3, dtype=torch.uint8, device="cuda")
        self.yuv = torch.empty(N * px * 3 // 2, dtype=torch.uint8, device="cuda")
        for i in range(N):
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(self.p010.data_ptr() + i * px * 3), C.c_void_p(self.yuv.data_ptr() + i * px * 3 // 2), s) == 0
        self.head = torch.zeros(N, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        at = lambda t, i, bpp: t.data_ptr() + i * px * bpp   # noqa: E731
        self.d10 = api.image_array([api.rgba1010102_image(at(self.h10, i, 4), W, H, api.CG_BT2100) for i in range(N)])
        self.dsm = api.image_array([api.rgba1010102_image(at(self.smooth, i, 4), W, H, api.CG_BT2100) for i in range(N)])
        self.d16 = api.image_array([api.rgba_f16_image(at(self.h16, i, 8), W, H, api.CG_BT2100) for i in range(N)])
        self.dp = api.image_array([api.p010_image(self.p010.data_ptr() + i * px * 3, W, H, api.CG_BT2100) for i in range(N)])
        self.dst =api.image_array([api.out_image(at(self.rgba, i, 4)) for i in range(N)])
        self.dst_yuv = api.image_array([api.yuv420_image(self.yuv.data_ptr() + i * px * 3 // 2, W, H, api.CG_UNSPECIFIED) for i in range(N)])


def timed(fn, events=True):
    ts = []
    for r in range(WARMUP + REPS):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(r)
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(r)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
        if r >= WARMUP:
            ts.append(t)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def tonemap_figures(lib, sets, s, out):
    given, measured = arr(C.c_float, [600.0] * N), None
    copies = {}
    for name, src, dst, bpp in (("copy    4 B/pixel read + 4 written (the RGBA1010102 lines' bytes)", "h10", "rgba", 8.0),
                                ("copy    6 B/pixel read + 6 written (the RGBA F16 line's bytes)", "six", "six_dst", 12.0)):
        med, lo, hi = timed(lambda r: getattr(sets[r % SETS], dst).copy_(getattr(sets[r % SETS], src)))
        copies[bpp] = med
        nbytes = N * W * H * bpp
        out("tone map  %-66s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB, %6.0f GB/s (%4.1f %% of 8 TB/s)" % (name, med, lo, hi, nbytes / 1e6, nbytes / med / 1e6,
                                                                                                    100.0 * nbytes / HBM * 1e3 / med))
    rows = [("planar  PQ    P010 -> YUV 4:2:0 (uhdr_hip_tonemap_sdr_batch)", api.TF_PQ, "dp", 4.5, None),
            ("planar  HLG   P010 -> YUV 4:2:0 (uhdr_hip_tonemap_sdr_batch)", api.TF_HLG, "dp", 4.5, None),
            ("packed  PQ    RGBA1010102 noise", api.TF_PQ, "d10", 8.0, 8.0),
            ("packed  PQ    RGBA1010102 smooth ramp", api.TF_PQ, "dsm", 8.0, 8.0),
            ("packed  HLG   RGBA1010102 noise", api.TF_HLG, "d10", 8.0, 8.0),
            ("packed  LINEAR RGBA F16 noise", api.TF_LINEAR, "d16", 12.0, 12.0)]
    for name, tf, src, bpp, copy_of in rows:
        for how, peaks in (("given H", given), ("measured H", measured)):
            def call(r):
                st = sets[r % SETS]
                if src == "dp":
                    rc = lib.uhdr_hip_tonemap_sdr_batch(N, st.dp, st.dst_yuv, tf, OP, peaks, C.c_void_p(st.head.data_ptr()), s)
                else:
                    rc = lib.uhdr_hip_tonemap_packed_batch(N, getattr(st, src), st.dst, tf, OP, peaks, C.c_void_p(st.head.data_ptr()), s)
                assert rc == 0, (name, rc, lib.uhdr_hip_last_error())
            med, lo, hi = timed(call)
            nbytes = N * W * H * bpp
            tail = "" if copy_of is None else "; x%.2f of the copy" % (med / copies[copy_of])
            out("tone map  %-54s %-10s  %8.3f ms [%8.3f .. %8.3f]  %7.1f MB, %6.0f GB/s (%4.1f %% of 8 TB/s)%s" %
                (name, how, med, lo, hi, nbytes / 1e6, nbytes / med / 1e6, 100.0 * nbytes / HBM * 1e3 / med, tail))


def encode_figures(lib, st, s, out):
    caps = [W * H * 3] * N_ENC
    bufs = [np.zeros(c, np.uint8) for c in caps]
    optr, capa = arr(C.c_void_p, [b.ctypes.data for b in bufs]), arr(C.c_size_t, caps)
    sizes, stat = arr(C.c_size_t, [0] * N_ENC), arr(C.c_int, [0] * N_ENC)
    for name, tf, src in (("HLG  RGBA1010102", api.TF_HLG, "d10"), ("LINEAR RGBA F16", api.TF_LINEAR, "d16")):
        hdr = getattr(st, src)
        sdr = st.dst
        assert lib.uhdr_hip_tonemap_packed_batch(N_ENC, hdr, sdr, tf, OP, None, C.c_void_p(st.head.data_ptr()), s) == 0
        torch.cuda.synchronize()

        def both(r):
            assert lib.uhdr_hip_jpegr_encode_packed_batch(N_ENC, hdr, sdr, tf, 90, None, None, optr, capa, sizes, stat, 0, api.MEM_DEVICE, s) == 0, list(stat)

        def alone(r):
            assert lib.uhdr_hip_jpegr_encode_packed_api0_batch(N_ENC, hdr, tf, 90, None, None, optr, capa, sizes, None, stat, OP, None, 0, api.MEM_DEVICE,
                                                               s) == 0, list(stat)
        for label, fn in (("uhdr_hip_jpegr_encode_packed_batch, both images given", both), ("uhdr_hip_jpegr_encode_packed_api0_batch, HDR image alone", alone)):
            med, lo, hi = timed(fn, events=False)
            mb = sum(sizes[k] for k in range(N_ENC)) / 1e6
            out("encode    %-18s %-58s %8.2f ms [%8.2f .. %8.2f]  %6.2f ms per file; %7.1f MB of files (noise, quality 90)" % (name, label, med, lo, hi,
                                                                                                                           med / N_ENC, mb))


def main():
    path = os.path.join(ROOT, "profiles", "r11_packed_tonemap.txt")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    lines = []

    def out(text):
        print(text, flush=True)
        lines.append(text)
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out("command: python scripts/time_packed_tonemap.py")
    out("device: %s; tone map: %d x %dx%d per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
        (torch.cuda.get_device_name(0), N, W, H, SETS, WARMUP, REPS))
    sets = [Set(lib, 1000 * (b + 1), s) for b in range(SETS)]
    tonemap_figures(lib, sets, s, out)
    encode_figures(lib, sets[0], s, out)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
