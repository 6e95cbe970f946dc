"""Times the content-adaptive packed entry points against the constant-range packed ones on one GPU and writes
profiles/r16_packed_adaptive.txt.

    python scripts/time_packed_adaptive.py [--out FILE]

In one process:
    generate   uhdr_hip_generate_gainmap_packed_adaptive_batch on 64 x 3840x2160 pairs -- RGBA8888 with RGBA1010102 (HLG, PQ) and with
               RGBA F16 (linear), one plane and RGB -- beside uhdr_hip_generate_gainmap_packed_batch (metadata_in = NULL) on the same
               sets: the same sampling and the same exact path, so the difference is the gains' write and read (4 or 12 bytes per
               map pixel, each way), the second pass's arithmetic and three small launches.
    encode     uhdr_hip_jpegr_encode_packed_adaptive_batch on 16 x 3840x2160 files in device memory, files to host memory, beside
               uhdr_hip_jpegr_encode_packed_batch (the pair) and uhdr_hip_jpegr_encode_packed_api0_batch (the HDR image alone).
The generate calls rotate over BATCHES resident sets, so that no launch finds its input in a cache the launch before it filled.
Generate times are device events around one call each, encode times a host clock around the call (it synchronises); milliseconds
per call, median [min .. max] of REPS.  The byte model beside each ratio: every input pixel once and every map byte once for the
constant-range call; the adaptive call adds the gains once written and once read."""
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
MW, MH = W // 4, H // 4
N, N_ENC = 64, 16
BATCHES, WARMUP, REPS = 3, 2, 9


def arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class Set:
    """N resident 4K frames of the three packed layouts (noise), the maps (RGBA-sized) and the ranges"""

    def __init__(self, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        self.keep = []
        keep = lambda t: self.keep.append(t) or t   # noqa: E731
        sdr, h10, h16, maps = [], [], [], []
        for i in range(N):
            sdr.append(keep(torch.randint(0, 256, (H * W * 4,), dtype=torch.uint8, device="cuda", generator=g)))
            h10.append(keep(torch.randint(-2 ** 31, 2 ** 31 - 1, (H * W,), dtype=torch.int32, device="cuda", generator=g)))
            h16.append(keep(torch.randint(0, 0x4401, (H * W * 4,), dtype=torch.int16, device="cuda", generator=g)))   # finite halves in [0, 4]
            maps.append(keep(torch.empty(4 * MW * MH, dtype=torch.uint8, device="cuda")))
        torch.cuda.synchronize()
        self.sdr_list = [api.rgba8888_image(t.data_ptr(), W, H, api.CG_BT709) for t in sdr]
        self.sdr = api.image_array(self.sdr_list)
        self.h10 = api.image_array([api.rgba1010102_image(t.data_ptr(), W, H, api.CG_BT2100) for t in h10])
        self.h16 = api.image_array([api.rgba_f16_image(t.data_ptr(), W, H, api.CG_BT2100) for t in h16])
        self.dst = api.image_array([api.out_image(t.data_ptr()) for t in maps])
        self.range = keep(torch.zeros(2 * N, dtype=torch.float32, device="cuda"))


GEN_CASES = [
    # (name, transfer function, HDR images, bytes read per pixel)
    ("HLG    RGBA8888 + RGBA1010102", api.TF_HLG, "h10", 8.0),
    ("PQ     RGBA8888 + RGBA1010102", api.TF_PQ, "h10", 8.0),
    ("LINEAR RGBA8888 + RGBA F16", api.TF_LINEAR, "h16", 12.0),
]


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


def generate_figures(lib, sets, s, out):
    for rgb in (0, 1):
        nb = api.packed_adaptive_workspace_bytes(sets[0].sdr_list, rgb)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        for name, tf, hdr, bpp in GEN_CASES:
            def constant(r):
                st = sets[r % BATCHES]
                assert lib.uhdr_hip_generate_gainmap_packed_batch(N, st.sdr, getattr(st, hdr), tf, None, None, st.dst, rgb, s) == 0

            def adaptive(r):
                st = sets[r % BATCHES]
                assert lib.uhdr_hip_generate_gainmap_packed_adaptive_batch(N, st.sdr, getattr(st, hdr), tf, st.dst, rgb, api.BOOST_PER_IMAGE, None,
                                                                           C.c_void_p(st.range.data_ptr()), C.c_void_p(ws.data_ptr()), nb, s) == 0
            c, clo, chi = timed(constant)
            a, alo, ahi = timed(adaptive)
            map_b, gain_b = (4 if rgb else 1) * MW * MH, (12 if rgb else 4) * MW * MH
            base, more = N * (W * H * bpp + map_b), N * 2 * gain_b
            out("generate  %-30s %-9s constant %7.3f ms [%7.3f .. %7.3f]  adaptive %7.3f ms [%7.3f .. %7.3f]  x%.3f; by bytes x%.3f (%.1f + %.1f MB)" %
                (name, "RGB map" if rgb else "one plane", c, clo, chi, a, alo, ahi, a / c, (base + more) / base, base / 1e6, more / 1e6))
        del ws


def encode_figures(lib, st, s, out):
    caps = [W * H * 3] * N_ENC
    bufs = [np.zeros(c, np.uint8) for c in caps]
    optr, capa = arr(C.c_void_p, [b.ctypes.data for b in bufs]), arr(C.c_size_t, caps)
    sizes, stat = arr(C.c_size_t, [0] * N_ENC), arr(C.c_int, [0] * N_ENC)
    for rgb in (0, 1):
        for api0 in (False, True):
            def constant(r):
                if api0:
                    rc = lib.uhdr_hip_jpegr_encode_packed_api0_batch(N_ENC, st.h10, api.TF_HLG, 90, None, None, optr, capa, sizes, None, stat,
                                                                     api.TONEMAP_REINHARD_MAXRGB, None, rgb, api.MEM_DEVICE, s)
                else:
                    rc = lib.uhdr_hip_jpegr_encode_packed_batch(N_ENC, st.h10, st.sdr, api.TF_HLG, 90, None, None, optr, capa, sizes, stat, rgb, api.MEM_DEVICE, s)
                assert rc == 0, list(stat)

            def adaptive(r):
                assert lib.uhdr_hip_jpegr_encode_packed_adaptive_batch(N_ENC, st.h10, None if api0 else st.sdr, api.TF_HLG, 90, None, None, optr, capa, sizes, None,
                                                                       stat, None, rgb, api.BOOST_PER_IMAGE, api.MEM_DEVICE, s) == 0, list(stat)
            c, clo, chi = timed(constant, events=False)
            a, alo, ahi = timed(adaptive, events=False)
            out("encode    HLG RGBA1010102 %-18s %-9s constant %8.2f ms [%8.2f .. %8.2f]  adaptive %8.2f ms [%8.2f .. %8.2f]  x%.3f; %.2f ms per file" %
                ("alone (API-0)" if api0 else "+ RGBA8888", "RGB map" if rgb else "one plane", c, clo, chi, a, alo, ahi, a / c, a / N_ENC))


def main():
    path = os.path.join(ROOT, "profiles", "r16_packed_adaptive.txt")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    if "--lib" in sys.argv:   # another build of the library (the parent commit's), as in scripts/time_jpeg_sampling_encode.py
        api.LIB_PATH = sys.argv[sys.argv.index("--lib") + 1]
        probe = C.CDLL(api.LIB_PATH)
        api.SIGNATURES = {k: v for k, v in api.SIGNATURES.items() if hasattr(probe, k)}
    lines = []

    def out(text):
        print(text, flush=True)
        lines.append(text)
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out("command: python scripts/time_packed_adaptive.py")
    out("device: %s; generate: %d x %dx%d per call, %d resident sets rotated, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
        (torch.cuda.get_device_name(0), N, W, H, BATCHES, WARMUP, REPS))
    sets = [Set(1000 * (b + 1)) for b in range(BATCHES)]
    generate_figures(lib, sets, s, out)
    encode_figures(lib, sets[0], s, out)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
