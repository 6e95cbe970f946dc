"""Times the packed-RGBA entry points against their planar counterparts on one GPU and writes profiles/r10_packed.txt.

    python scripts/time_packed.py [--out FILE]

In one process:
    generate   uhdr_hip_generate_gainmap_packed_batch on 64 x 3840x2160 pairs -- RGBA8888 with RGBA1010102 (PQ, HLG) and with RGBA F16
               (linear) -- beside uhdr_hip_generate_gainmap_md_batch on planar pairs of the same size: the same exact path behind the
               sampling, so the difference is the bytes read (8 or 12 B/pixel against 4.5) and the sampling's arithmetic.  The planar
               call gets the reference's constants as its metadata, the packed calls metadata_in = NULL: the same encodeGain.
    encode     uhdr_hip_jpegr_encode_packed_batch on 16 x 3840x2160 pairs in device memory, files to host memory, beside
               uhdr_hip_jpegr_encode_batch (API-1) on planar pairs.
    round trip one 1280x720 JPEG/R file (API-1, HLG, the reference's test frames) decoded to RGBA8888 and to HLG RGBA1010102, the map generated again from those
               two: mean absolute byte difference to the map the file carries.  A report, not a test.
The generate calls rotate over BATCHES resident sets, so that no launch finds its input in a cache the launch before it filled.
Generate times are device events around one call each, encode times a host clock around the call (it synchronises); milliseconds
per call, median [min .. max] of REPS.  GB/s are the algorithmic bytes -- every input pixel once, every map byte once -- over the
median."""
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
BATCHES, WARMUP, REPS = 2, 2, 9
FLT_MAX = 3.4028234663852886e38
HBM = 8.0e12


def arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class Set:
    """N resident 4K frames of every layout (noise), and the maps"""

    def __init__(self, lib, seed, s):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        self.keep = []
        keep = lambda t: self.keep.append(t) or t   # noqa: E731
        p010, yuv, sdr, h10, h16, mono = [], [], [], [], [], []
        for i in range(N):
            p, y = keep(torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")), keep(torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda"))
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), s) == 0
            p010.append(p)
            yuv.append(y)
            sdr.append(keep(torch.randint(0, 256, (H * W * 4,), dtype=torch.uint8, device="cuda", generator=g)))
            h10.append(keep(torch.randint(-2 ** 31, 2 ** 31 - 1, (H * W,), dtype=torch.int32, device="cuda", generator=g)))
            h16.append(keep(torch.randint(0, 0x4401, (H * W * 4,), dtype=torch.int16, device="cuda", generator=g)))   # finite halves in [0, 4]
            mono.append(keep(torch.empty(MW * MH, dtype=torch.uint8, device="cuda")))
        torch.cuda.synchronize()
        self.p = api.image_array([api.p010_image(t.data_ptr(), W, H, api.CG_BT2100) for t in p010])
        self.y = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_BT709) for t in yuv])
        self.sdr = api.image_array([api.rgba8888_image(t.data_ptr(), W, H, api.CG_BT709) for t in sdr])
        self.h10 = api.image_array([api.rgba1010102_image(t.data_ptr(), W, H, api.CG_BT2100) for t in h10])
        self.h16 = api.image_array([api.rgba_f16_image(t.data_ptr(), W, H, api.CG_BT2100) for t in h16])
        self.dst = api.image_array([api.out_image(t.data_ptr()) for t in mono])


GEN_CASES = [
    # (name, transfer function, HDR images, bytes read per pixel)
    ("planar  HLG   P010 + YUV 4:2:0 (md call)", api.TF_HLG, "p", 4.5),
    ("planar  PQ    P010 + YUV 4:2:0 (md call)", api.TF_PQ, "p", 4.5),
    ("packed  PQ    RGBA8888 + RGBA1010102", api.TF_PQ, "h10", 8.0),
    ("packed  HLG   RGBA8888 + RGBA1010102", api.TF_HLG, "h10", 8.0),
    ("packed  LINEAR RGBA8888 + RGBA F16", api.TF_LINEAR, "h16", 12.0),
]


def gen_call(lib, st, case, s):
    name, tf, hdr, _ = case
    if hdr == "p":
        hi = (10000.0 if tf == api.TF_PQ else 1000.0) / 203.0
        md = api.metadata(hi)
        rc = lib.uhdr_hip_generate_gainmap_md_batch(N, st.y, st.p, tf, C.byref(md), st.dst, 0, 0, s)
    else:
        rc = lib.uhdr_hip_generate_gainmap_packed_batch(N, st.sdr, getattr(st, hdr), tf, None, None, st.dst, 0, s)
    assert rc == 0, (name, rc, lib.uhdr_hip_last_error())


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


def encode_figures(lib, st, s, out):
    caps = [W * H * 3] * N_ENC
    bufs = [np.zeros(c, np.uint8) for c in caps]
    optr, capa = arr(C.c_void_p, [b.ctypes.data for b in bufs]), arr(C.c_size_t, caps)
    sizes, stat = arr(C.c_size_t, [0] * N_ENC), arr(C.c_int, [0] * N_ENC)

    def planar(r):
        assert lib.uhdr_hip_jpegr_encode_batch(N_ENC, st.p, st.y, api.TF_HLG, 90, None, None, optr, capa, sizes, stat, api.MEM_DEVICE, s) == 0, list(stat)

    def packed(hdr, tf, rgb_map):
        def run(r):
            assert lib.uhdr_hip_jpegr_encode_packed_batch(N_ENC, getattr(st, hdr), st.sdr, tf, 90, None, None, optr, capa, sizes, stat, rgb_map, api.MEM_DEVICE,
                                                          s) == 0, list(stat)
        return run
    rows = [("planar  HLG  uhdr_hip_jpegr_encode_batch (API-1)", planar),
            ("packed  HLG  RGBA8888 + RGBA1010102, one-plane map", packed("h10", api.TF_HLG, 0)),
            ("packed  HLG  RGBA8888 + RGBA1010102, RGB map", packed("h10", api.TF_HLG, 1)),
            ("packed  LINEAR RGBA8888 + RGBA F16, one-plane map", packed("h16", api.TF_LINEAR, 0))]
    for name, fn in rows:
        med, lo, hi = timed(fn, events=False)
        mb = sum(sizes[k] for k in range(N_ENC)) / 1e6
        out("encode    %-52s %8.2f ms [%8.2f .. %8.2f]  %6.2f ms per file; %7.1f MB of files (noise images at quality 90)" % (name, med, lo, hi, med / N_ENC, mb))


def round_trip(lib, s, out):
    w, h = 1280, 720   # the reference's own test frames (tests/golden/, as the parity tests read them: HLG BT.2100 over BT.709)
    g = os.path.join(ROOT, "tests", "golden")
    p = torch.from_numpy(np.fromfile(os.path.join(g, "raw_p010_image.p010"), np.uint8)).cuda()
    y = torch.from_numpy(np.fromfile(os.path.join(g, "raw_yuv420_image.yuv420"), np.uint8)).cuda()
    pi, yi = api.p010_image(p.data_ptr(), w, h, api.CG_BT2100), api.yuv420_image(y.data_ptr(), w, h, api.CG_BT709)
    buf, n = np.zeros(w * h * 3, np.uint8), C.c_size_t()
    assert lib.uhdr_hip_jpegr_encode_api1(C.byref(pi), C.byref(yi), api.TF_HLG, 95, None, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n), api.MEM_DEVICE, s) == 0
    renditions = {}
    for fmt in (api.OUTPUT_SDR, api.OUTPUT_HDR_HLG):
        t = torch.empty(w * h * 4, dtype=torch.uint8, device="cuda")
        d, md = api.Image(), api.Metadata()
        assert lib.uhdr_hip_jpegr_decode(C.c_void_p(buf.ctypes.data), n.value, fmt, FLT_MAX, C.c_void_p(t.data_ptr()), t.numel(), C.byref(d), C.byref(md), api.APPLY_EXACT,
                                         api.MEM_DEVICE, s) == 0
        renditions[fmt] = t
    a, g = api.JpegInfo(), api.JpegInfo()
    assert lib.uhdr_hip_jpegr_info(C.c_void_p(buf.ctypes.data), n.value, C.byref(a), C.byref(g)) == 0
    mw, mh = w // 4, h // 4
    have, d = np.zeros(mw * mh, np.uint8), api.Image()
    assert lib.uhdr_hip_jpeg_decode(C.c_void_p(buf.ctypes.data + g.offset), g.size, C.c_void_p(have.ctypes.data), have.size, C.byref(d), api.MEM_HOST, s) == 0
    # the decoded renditions are both in the primary image's gamut (apply converts none)
    sd = api.rgba8888_image(renditions[api.OUTPUT_SDR].data_ptr(), w, h, api.CG_BT709)
    hd = api.rgba1010102_image(renditions[api.OUTPUT_HDR_HLG].data_ptr(), w, h, api.CG_BT709)
    again = torch.empty(mw * mh, dtype=torch.uint8, device="cuda")
    dst = api.out_image(again.data_ptr())
    assert lib.uhdr_hip_generate_gainmap_packed_batch(1, C.byref(sd), C.byref(hd), api.TF_HLG, None, None, C.byref(dst), 0, s) == 0
    torch.cuda.synchronize()
    diff = np.abs(again.cpu().numpy().astype(np.int32) - have.astype(np.int32))
    out("round trip  %dx%d camera pair (tests/golden/raw_*) -> JPEG/R (API-1, HLG, quality 95) -> RGBA8888 + HLG RGBA1010102 (APPLY_EXACT) -> packed generate:" % (w, h))
    out("            mean |byte difference| to the map the file carries (decoded from its quality-85 JPEG) %.3f, max %d, %.1f %% of the bytes equal"
        % (float(diff.mean()), int(diff.max()), 100.0 * float((diff == 0).mean())))


def main():
    path = os.path.join(ROOT, "profiles", "r10_packed.txt")
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
    out("command: python scripts/time_packed.py")
    out("device: %s; generate: %d x %dx%d per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
        (torch.cuda.get_device_name(0), N, W, H, BATCHES, WARMUP, REPS))
    sets = [Set(lib, 1000 * (b + 1), s) for b in range(BATCHES)]
    base = None
    for case in GEN_CASES:
        med, lo, hi = timed(lambda r: gen_call(lib, sets[r % BATCHES], case, s))
        base = base or med
        nbytes = N * (W * H * case[3] + MW * MH)
        out("generate  %-44s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB, %6.0f GB/s (%4.1f %% of 8 TB/s); x%.2f of the first line" %
            (case[0], med, lo, hi, nbytes / 1e6, nbytes / med / 1e6, 100.0 * nbytes / HBM * 1e3 / med, med / base))
    encode_figures(lib, sets[0], s, out)
    round_trip(lib, s, out)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
