"""Times the per-channel (RGB) gain-map kernels against their single-channel counterparts on one GPU (profiles/r08_rgbmap.txt).

    python scripts/time_rgbmap.py              # 64 x 3840x2160 per call
    python scripts/time_rgbmap.py --once       # one untimed pass of every case, for rocprofv3 --kernel-trace --stats

In one process, on the same frames:
    generate   uhdr_hip_generate_gainmap_rgb_batch against uhdr_hip_generate_gainmap_batch_ex in GENERATE_UNFILTERED mode -- the exact
               path without the f32 pre-filter, which is what the RGB kernel runs: the same front end, three encodeGains for one
    apply      uhdr_hip_apply_gainmap_rgb_batch FAST and EXACT against uhdr_hip_apply_gainmap_batch FAST and EXACT_UNFILTERED on a
               YUV444 primary, which takes the per-pixel kernel k_apply_px in every mode (the scale-4 streaming kernels are
               4:2:0's): the same grid and loads, two more exponentials and 0.19 more map bytes per pixel.  (EXACT behind its f32
               pre-filter, which the RGB path does not have, is printed beside them.)
    encode     uhdr_hip_jpeg_encode_rgb_batch of the 960x540 RGBA maps against uhdr_hip_jpeg_encode_batch of one plane of each:
               three times the blocks.  Both calls end with a synchronisation and bring the sizes to the host.
The calls rotate over BATCHES resident sets of frames, as bench.py does, so that no launch finds its input in a cache the launch
before it filled.  Times are device events around one call each, in milliseconds per call: median [min .. max] of REPS.
The kernel names are the ones the dispatch rules select for these frames; they are not read from a trace --
`rocprofv3 --kernel-trace --stats -- python scripts/time_rgbmap.py --once` shows what ran."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

W, H = 3840, 2160
MW, MH = W // 4, H // 4
N = 64
BATCHES, WARMUP, REPS = 3, 2, 9
FLT_MAX = 3.4028234663852886e38
HBM = 8.0e12


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class Set:
    """N resident 4K pairs (LCG noise, distinct seeds), a YUV444 primary per pair, maps of both kinds and the outputs"""

    def __init__(self, lib, seed, s):
        self.keep = []
        new = lambda nbytes: self.keep.append(torch.empty(nbytes, dtype=torch.uint8, device="cuda")) or self.keep[-1]
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        p010, yuv, y444, mono, rgba, out, jpg = [], [], [], [], [], [], []
        for i in range(N):
            p, y = new(W * H * 3), new(W * H * 3 // 2)
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), s) == 0
            p010.append(p)
            yuv.append(y)
            t = new(W * H * 3)
            t.copy_(torch.randint(0, 256, (W * H * 3,), dtype=torch.uint8, device="cuda", generator=g))
            y444.append(t)
            mono.append(new(MW * MH))
            rgba.append(new(MW * MH * 4))
            out.append(new(W * H * 4))
            jpg.append(new(MW * MH * 4 + 65536))
        torch.cuda.synchronize()
        self.p = api.image_array([api.p010_image(t.data_ptr(), W, H, api.CG_BT2100) for t in p010])
        self.y = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_BT709) for t in yuv])
        self.y444 = api.image_array([api.ycbcr_image(t.data_ptr(), W, H, api.CG_BT709, api.PIX_FMT_YUV444) for t in y444])
        self.mono = api.image_array([api.mono_image(t.data_ptr(), MW, MH) for t in mono])
        self.rgba = api.image_array([api.rgba_map_image(t.data_ptr(), MW, MH) for t in rgba])
        self.mono_dst = api.image_array([api.out_image(t.data_ptr()) for t in mono])
        self.rgba_dst = api.image_array([api.out_image(t.data_ptr()) for t in rgba])
        self.out = api.image_array([api.out_image(t.data_ptr()) for t in out])
        self.jpg = _arr(C.c_void_p, [t.data_ptr() for t in jpg])
        self.jpg_cap = _arr(C.c_size_t, [MW * MH * 4 + 65536] * N)
        self.jpg_size, self.stat, self.q = _arr(C.c_size_t, [0] * N), _arr(C.c_int, [0] * N), _arr(C.c_int, [85] * N)
        self.md = api.Metadata()


CASES = [
    # (group, name, kernels the dispatch rule selects)
    ("generate", "single-channel UNFILTERED", "k_generate<HLG, aligned, no LUT, no filter>"),
    ("generate", "RGB", "k_generate_rgb<HLG, aligned, 4 tiles>"),
    ("apply FAST", "single-channel", "k_apply_px<3, false>"),
    ("apply FAST", "RGB", "k_apply_px_rgb<3, false>"),
    ("apply EXACT", "single-channel EXACT_UNFILTERED", "k_apply_px<3, true>"),
    ("apply EXACT", "RGB", "k_apply_px_rgb<3, true>"),
    ("apply EXACT", "single-channel EXACT (pre-filtered)", "k_apply_px_est<3>, k_apply_resolve<3>"),
    ("encode", "monochrome, one plane", "k_jpeg_fdct_quant_count_multi, k_jpeg_clear_multi, k_jpeg_emit_multi, k_jpeg_stuff_count_multi, k_jpeg_stuff_copy_multi"),
    ("encode", "RGB 4:4:4", "k_jpeg_fdct_quant_count_multi_rgb and the same four"),
]


def call(lib, st, k, s):
    group, name, _ = CASES[k]
    md = C.byref(st.md)
    if group == "generate":
        if name == "RGB":
            rc = lib.uhdr_hip_generate_gainmap_rgb_batch(N, st.y, st.p, api.TF_HLG, md, st.rgba_dst, 0, s)
        else:
            rc = lib.uhdr_hip_generate_gainmap_batch_ex(N, st.y, st.p, api.TF_HLG, md, st.mono_dst, 0, api.GENERATE_UNFILTERED, None, s)
    elif group.startswith("apply"):
        if name == "RGB":
            mode = api.APPLY_FAST if group == "apply FAST" else api.APPLY_EXACT
            rc = lib.uhdr_hip_apply_gainmap_rgb_batch(N, st.y444, st.rgba, md, api.OUTPUT_HDR_HLG, FLT_MAX, st.out, mode, s)
        else:
            mode = api.APPLY_FAST if group == "apply FAST" else api.APPLY_EXACT if "pre-filtered" in name else api.APPLY_EXACT_UNFILTERED
            rc = lib.uhdr_hip_apply_gainmap_batch(N, st.y444, st.mono, md, api.OUTPUT_HDR_HLG, FLT_MAX, st.out, mode, s)
    elif name.startswith("RGB"):
        rc = lib.uhdr_hip_jpeg_encode_rgb_batch(N, st.rgba, st.q, st.jpg, st.jpg_cap, st.jpg_size, st.stat, api.MEM_DEVICE, s)
    else:
        rc = lib.uhdr_hip_jpeg_encode_batch(N, st.mono, st.q, None, None, st.jpg, st.jpg_cap, st.jpg_size, st.stat, api.MEM_DEVICE, s)
    assert rc == 0, (CASES[k], rc, lib.uhdr_hip_last_error())


def measure(lib, sets, k, s):
    for r in range(WARMUP):
        call(lib, sets[r % len(sets)], k, s)
    torch.cuda.synchronize()
    ts = []
    for r in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(lib, sets[r % len(sets)], k, s)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def bytes_moved(k):
    group, name, _ = CASES[k]
    rgb = name.startswith("RGB")
    if group == "generate":
        return N * (W * H * 4.5 + MW * MH * (4 if rgb else 1))
    if group.startswith("apply"):
        return N * (W * H * (3 + 4) + MW * MH * (4 if rgb else 1))
    return N * MW * MH * (4 if rgb else 1)   # the pixels read; the files written are not known before the call


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    once = "--once" in sys.argv
    print("device: %s; %d x %dx%d per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
          (torch.cuda.get_device_name(0), N, W, H, BATCHES, WARMUP, REPS))
    sets = [Set(lib, 1000 * (b + 1), s) for b in range(BATCHES)]
    # the maps the apply and encode cases read are real ones: generate's, of both kinds (the first two cases below rewrite the same bytes)
    for st in sets:
        call(lib, st, 0, s)
        call(lib, st, 1, s)
    torch.cuda.synchronize()
    base = {}
    for k, (group, name, kernels) in enumerate(CASES):
        if once:
            call(lib, sets[0], k, s)
            continue
        med, lo, hi = measure(lib, sets, k, s)
        base.setdefault(group, med)
        nbytes = bytes_moved(k)
        print("%-12s %-36s %8.3f ms [%8.3f .. %8.3f]  x%.2f of the group's first line;  %7.1f MB read + written (encode: read), memory bound %.3f ms (%4.1f %% of 8 TB/s)" %
              (group, name, med, lo, hi, med / base[group], nbytes / 1e6, nbytes / HBM * 1e3, 100.0 * nbytes / HBM * 1e3 / med))
        print("             kernels expected from the dispatch rule (not traced): %s" % kernels)
    if not once:
        st = sets[0]
        print("encode: bytes of the first file of each kind in the last call: %d (the stat array: %s)" % (st.jpg_size[0], sorted(set(st.stat))))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
