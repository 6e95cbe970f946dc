"""Times uhdr_hip_apply_gainmap_packed_batch against its two yardsticks on one GPU (profiles/r15_packed_apply.txt).

    python scripts/time_packed_apply.py          # 64 x 3840x2160 per call
    python scripts/time_packed_apply.py --quick  # FAST and EXACT at HLG only (a short session)

In one process, on resident images:
    packed     FAST and EXACT; each output format; one-plane and RGBA maps; scale factors 4 (k_apply_packed_s4, the strip form)
               and 2 (k_apply_packed_px, one pixel per lane)
    planar     uhdr_hip_apply_gainmap_batch FAST on 4:2:0 images of the same size with the one-plane map at factor 4 (k_apply_s4)
    copy       a device-to-device copy that reads plus writes as many bytes as the packed call does (DESIGN.md 4.1.7's yardstick)
The images are uniform random codes (torch.randint, fixed seeds), the maps random bytes.  The calls rotate over SETS resident sets so
that no launch finds its input in a cache the launch before it filled.  Times are device events around one call each, in
milliseconds per call: median [min .. max] of REPS.  Last, on the first set: the share of 10-bit channels (HLG) in which FAST differs
from EXACT, for the packed call and -- FAST against EXACT -- for the planar one.
The kernel names are the ones the dispatch rules select for these frames; they are not read from a trace."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

W, H = 3840, 2160
N = 64
SETS, WARMUP, REPS = 2, 2, 7
FLT_MAX = 3.4028234663852886e38
MD = api.Metadata(b"1.0", 4.926, 1.0, 1.0, 0.0, 0.0, 1.0, 4.926)
FORMATS = [(api.OUTPUT_HDR_HLG, "HLG 1010102", 4), (api.OUTPUT_HDR_PQ, "PQ 1010102", 4), (api.OUTPUT_HDR_LINEAR, "linear F16", 8),
           (api.OUTPUT_HDR_LINEAR_RGB_10BIT, "planar 10 bit", 6)]


class Set:
    """N resident images of every kind: RGBA8888 and 4:2:0 SDR, one-plane and RGBA maps at factors 4 and 2, one output each"""

    def __init__(self, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        rnd = lambda nbytes: torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
        self.rgba = [rnd(W * H * 4) for _ in range(N)]
        self.yuv = [rnd(W * H * 3 // 2) for _ in range(N)]
        self.maps = {(s, ch): [rnd((W // s) * (H // s) * ch) for _ in range(N)] for s in (4, 2) for ch in (1, 4)}
        self.out = [torch.empty(W * H * 8, dtype=torch.uint8, device="cuda") for _ in range(N)]
        self.out2 = torch.empty(W * H * 8, dtype=torch.uint8, device="cuda")
        self.sdr = api.image_array([api.rgba8888_image(t.data_ptr(), W, H, api.CG_BT709) for t in self.rgba])
        self.y = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_BT709) for t in self.yuv])
        self.map_desc = {}
        for (s, ch), ts in self.maps.items():
            mk = api.mono_image if ch == 1 else api.rgba_map_image
            self.map_desc[(s, ch)] = api.image_array([mk(t.data_ptr(), W // s, H // s) for t in ts])
        self.dst = api.image_array([api.out_image(t.data_ptr()) for t in self.out])


def packed(lib, st, fmt, mode, s, ch, stream, n=N):
    rc = lib.uhdr_hip_apply_gainmap_packed_batch(n, st.sdr, st.map_desc[(s, ch)], C.byref(MD), fmt, FLT_MAX, st.dst, mode, stream)
    assert rc == 0, (rc, lib.uhdr_hip_last_error())


def planar(lib, st, fmt, mode, stream, n=N):
    rc = lib.uhdr_hip_apply_gainmap_batch(n, st.y, st.map_desc[(4, 1)], C.byref(MD), fmt, FLT_MAX, st.dst, mode, stream)
    assert rc == 0, (rc, lib.uhdr_hip_last_error())


def measure(sets, fn):
    for r in range(WARMUP):
        fn(sets[r % len(sets)])
    torch.cuda.synchronize()
    ts = []
    for r in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(sets[r % len(sets)])
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def differing_share(a, b):
    """share of 10-bit channels in which two RGBA1010102 outputs differ"""
    x, y = a.view(torch.int32), b.view(torch.int32)
    n = 0
    for sh in (0, 10, 20):
        n += int((((x >> sh) & 0x3ff) != ((y >> sh) & 0x3ff)).sum())
    return n / (3.0 * x.numel())


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    quick = "--quick" in sys.argv
    print("device: %s; %d x %dx%d per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
          (torch.cuda.get_device_name(0), N, W, H, SETS, WARMUP, REPS))
    sets = [Set(1000 * (b + 1)) for b in range(SETS)]
    torch.cuda.synchronize()
    line = "%-8s %-14s %-10s s=%d %-6s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB read + written  x%.3f of the copy, x%.3f of planar FAST"
    for fmt, fname, bpp in FORMATS[:1] if quick else FORMATS:
        pl = measure(sets, lambda st: planar(lib, st, fmt, api.APPLY_FAST, stream))
        nb = N * (W * H * (1.5 + bpp) + (W // 4) * (H // 4))
        print("%-8s %-14s %-10s s=4 %-6s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB read + written  (k_apply_s4, 4:2:0 planes)" %
              ("planar", fname, "one plane", "FAST", pl[0], pl[1], pl[2], nb / 1e6))
        for s in (4, 2):
            for ch in (1, 4):
                nb = N * (W * H * (4 + bpp) + (W // s) * (H // s) * ch)
                half = nb // 2
                src = torch.empty(half, dtype=torch.uint8, device="cuda")
                dst = torch.empty(half, dtype=torch.uint8, device="cuda")
                cp = measure(sets, lambda st: dst.copy_(src))
                print("%-8s %-14s %-10s s=%d %-6s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB read + written" %
                      ("copy", fname, "", s, "", cp[0], cp[1], cp[2], 2 * half / 1e6))
                del src, dst
                for mode, mname in ((api.APPLY_FAST, "FAST"), (api.APPLY_EXACT, "EXACT")):
                    t = measure(sets, lambda st: packed(lib, st, fmt, mode, s, ch, stream))
                    print(line % ("packed", fname, "one plane" if ch == 1 else "RGBA map", s, mname, t[0], t[1], t[2], nb / 1e6, t[0] / cp[0], t[0] / pl[0]))
    # FAST against EXACT on 8 images of the first set, HLG
    st, k = sets[0], 8
    for name, fn in (("packed, one plane, s=4", lambda mode: packed(lib, st, api.OUTPUT_HDR_HLG, mode, 4, 1, stream, k)),
                     ("packed, RGBA map, s=4", lambda mode: packed(lib, st, api.OUTPUT_HDR_HLG, mode, 4, 4, stream, k)),
                     ("packed, one plane, s=2", lambda mode: packed(lib, st, api.OUTPUT_HDR_HLG, mode, 2, 1, stream, k)),
                     ("planar, one plane, s=4", lambda mode: planar(lib, st, api.OUTPUT_HDR_HLG, mode, stream, k))):
        fn(api.APPLY_EXACT)
        torch.cuda.synchronize()
        exact = [t[:W * H * 4].clone() for t in st.out[:k]]
        fn(api.APPLY_FAST)
        torch.cuda.synchronize()
        share = sum(differing_share(st.out[i][:W * H * 4], exact[i]) for i in range(k)) / k
        print("share of 10-bit channels where FAST differs from EXACT (HLG, %d images, random codes): %-24s %.3e" % (k, name, share))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
