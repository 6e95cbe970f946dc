"""Times uhdr_hip_generate_gainmap_scaled_batch at several scale factors on one GPU and writes profiles/r13_generate_scales.txt.

    python scripts/time_generate_scales.py [--out FILE]

In one process, on 64 x 3840x2160 planar pairs (noise) in device memory, per factor and transfer function:
    new       the scaled call: one-plane map of the reference's metadata (the filtered kernel), or rgb = 1 (the exact path)
    factor 4  uhdr_hip_generate_gainmap_batch on the same pairs: the yardstick for the same input bytes
    copy      a device-to-device copy that moves the call's algorithmic bytes -- every input byte read once, every map byte written
              once: B bytes of traffic, i.e. a copy of B / 2 bytes, read and written -- as the floor
and the two ratios new / factor 4 and new / copy.  The calls rotate over BATCHES resident sets, so that no launch finds its input in
a cache the launch before it filled.  Times are device events around one call each, milliseconds per call, median [min .. max] of
REPS after WARMUP calls."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

W, H = 3840, 2160
N = 64
BATCHES, WARMUP, REPS = 2, 2, 9
HBM = 8.0e12


class Set:
    """N resident 4K pairs (noise) and room for the largest maps (factor 1, RGBA)"""

    def __init__(self, lib, seed, s):
        self.keep, p010, yuv, maps = [], [], [], []
        for i in range(N):
            p = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
            y = torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda")
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), s) == 0
            m = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
            p010.append(p), yuv.append(y), maps.append(m)
        self.keep = [p010, yuv, maps]
        torch.cuda.synchronize()
        self.p = api.image_array([api.p010_image(t.data_ptr(), W, H, api.CG_BT2100) for t in p010])
        self.y = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_BT709) for t in yuv])
        self.ptrs = [t.data_ptr() for t in maps]

    def dests(self):
        return api.image_array([api.out_image(p) for p in self.ptrs])   # (a call rewrites its descriptors: fresh ones per call)


def timed(fn):
    ts = []
    for r in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(r)
        b.record()
        b.synchronize()
        if r >= WARMUP:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    path = os.path.join(ROOT, "profiles", "r13_generate_scales.txt")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    lines = []

    def out(text):
        print(text, flush=True)
        lines.append(text)
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out("command: python scripts/time_generate_scales.py")
    out("device: %s; %d x %dx%d pairs per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
        (torch.cuda.get_device_name(0), N, W, H, BATCHES, WARMUP, REPS))
    sets = [Set(lib, 1000 * (b + 1), s) for b in range(BATCHES)]
    in_bytes = N * W * H * 4.5
    half_max = int((in_bytes + N * W * H * 4) / 2) + 256
    src = [torch.empty(half_max, dtype=torch.uint8, device="cuda") for _ in range(BATCHES)]
    dst = torch.empty(half_max, dtype=torch.uint8, device="cuda")
    md = api.Metadata()

    def four(tf):
        def run(r):
            st = sets[r % BATCHES]
            assert lib.uhdr_hip_generate_gainmap_batch(N, st.y, st.p, tf, C.byref(md), st.dests(), 0, None, s) == 0
        return run

    def scaled(tf, f, rgb):
        def run(r):
            st = sets[r % BATCHES]
            assert lib.uhdr_hip_generate_gainmap_scaled_batch(N, st.y, st.p, tf, None, None, st.dests(), 0, rgb, f, s) == 0
        return run

    def copy(nbytes):
        def run(r):
            dst[:nbytes].copy_(src[r % BATCHES][:nbytes])
        return run
    cases = [(f, tf, 0) for f in (1, 2, 3, 8) for tf in (api.TF_HLG, api.TF_PQ)] + [(1, api.TF_HLG, 1), (2, api.TF_HLG, 1)]
    names = {api.TF_HLG: "HLG", api.TF_PQ: "PQ"}
    base = {}
    for f, tf, rgb in cases:
        if tf not in base:
            base[tf] = timed(four(tf))
            b = in_bytes + N * (W // 4) * (H // 4)
            out("factor 4  %-3s one-plane map (uhdr_hip_generate_gainmap_batch)      %8.3f ms [%8.3f .. %8.3f]  %7.1f MB, %6.0f GB/s" %
                (names[tf], base[tf][0], base[tf][1], base[tf][2], b / 1e6, b / base[tf][0] / 1e6))
        mpx = (W // f) * (H // f)
        b = in_bytes + N * mpx * (4 if rgb else 1)
        new = timed(scaled(tf, f, rgb))
        flo = timed(copy(int(b / 2)))
        out("factor %-2d %-3s %-14s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB, %6.0f GB/s (%4.1f %% of 8 TB/s), %5.1f ps per map pixel;"
            " copy of the same bytes %7.3f ms [%7.3f .. %7.3f]; x%.2f of factor 4, x%.2f of the copy" %
            (f, names[tf], "RGB map" if rgb else "one-plane map", new[0], new[1], new[2], b / 1e6, b / new[0] / 1e6, 100.0 * b / HBM * 1e3 / new[0],
             new[0] * 1e9 / (N * mpx), flo[0], flo[1], flo[2], new[0] / base[tf][0], new[0] / flo[0]))
    # the share of map pixels the filter leaves in doubt on these noise frames (uhdr_hip_generate_gainmap_scaled_probe, untimed)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for f in (1, 2, 8):
        for tf in (api.TF_HLG, api.TF_PQ):
            count.zero_()
            assert lib.uhdr_hip_generate_gainmap_scaled_probe(N, sets[0].y, sets[0].p, tf, sets[0].dests(), 0, f, C.c_void_p(count.data_ptr()), s) == 0
            torch.cuda.synchronize()
            k, mpx = int(count.item()) & 0xFFFFFFFF, N * (W // f) * (H // f)
            out("in doubt  factor %-2d %-3s %10d of %10d map pixels, %.4f %%" % (f, names[tf], k, mpx, 100.0 * k / mpx))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
