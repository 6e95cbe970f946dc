"""Times the general-metadata gain-map kernels against the existing ones on one GPU (profiles/r09_gainmap_metadata.txt).

    python scripts/time_gainmap_metadata.py          # 64 x 3840x2160 per call
    python scripts/time_gainmap_metadata.py --once   # one untimed pass of every case, for rocprofv3 --kernel-trace --stats

In one process, on the same planes:
    apply      uhdr_hip_apply_gainmap_md_batch with gamma 1 and offsets 1/64, and with gamma 2.2, against uhdr_hip_apply_gainmap_batch
               FAST through the per-pixel kernel k_apply_px at scale 4.  The outputs sit 4 bytes behind a 16-byte boundary, which keeps
               the existing call off its scale-4 streaming kernel (app_fast_s4 wants 16-byte aligned rows): the same grid, the same
               loads and stores for all three.  The streaming kernel k_apply_s4 on aligned outputs is printed beside them.
    generate   uhdr_hip_generate_gainmap_md_batch (one plane, and RGB; gamma 1 and gamma 2.2) against
               uhdr_hip_generate_gainmap_rgb_batch: the same front end on the exact path.
The calls rotate over BATCHES resident sets of frames, as bench.py does, so that no launch finds its input in a cache the launch
before it filled.  Times are device events around one call each, in milliseconds per call: median [min .. max] of REPS.
The kernel names are the ones the dispatch rules select for these frames; they are not read from a trace."""
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
OFF = 4   # bytes the unaligned outputs sit behind a 16-byte boundary

DEGENERATE = api.Metadata(b"1.0", 4.926, 1.0, 1.0, 0.0, 0.0, 1.0, 4.926)
OFFSETS = api.Metadata(b"1.0", 4.926, 1.0, 1.0, 1 / 64, 1 / 64, 1.0, 4.926)
GAMMA = api.Metadata(b"1.0", 4.926, 1.0, 2.2, 1 / 64, 1 / 64, 1.0, 4.926)


class Set:
    """N resident 4K pairs (LCG noise, distinct seeds), maps of both kinds and the outputs"""

    def __init__(self, lib, seed, s):
        self.keep = []
        new = lambda nbytes: self.keep.append(torch.empty(nbytes, dtype=torch.uint8, device="cuda")) or self.keep[-1]
        p010, yuv, mono, rgba, out = [], [], [], [], []
        for i in range(N):
            p, y = new(W * H * 3), new(W * H * 3 // 2)
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), s) == 0
            p010.append(p)
            yuv.append(y)
            mono.append(new(MW * MH))
            rgba.append(new(MW * MH * 4))
            out.append(new(W * H * 4 + 16))
        torch.cuda.synchronize()
        self.p = api.image_array([api.p010_image(t.data_ptr(), W, H, api.CG_BT2100) for t in p010])
        self.y = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_BT709) for t in yuv])
        self.mono = api.image_array([api.mono_image(t.data_ptr(), MW, MH) for t in mono])
        self.mono_dst = api.image_array([api.out_image(t.data_ptr()) for t in mono])
        self.rgba_dst = api.image_array([api.out_image(t.data_ptr()) for t in rgba])
        self.out = api.image_array([api.out_image(t.data_ptr()) for t in out])
        self.out_off = api.image_array([api.out_image(t.data_ptr() + OFF) for t in out])
        self.md = api.Metadata()


CASES = [
    # (group, name, kernels the dispatch rule selects)
    ("apply", "existing FAST, per-pixel kernel", "k_apply_px<3, false>"),
    ("apply", "md: gamma 1, offsets 1/64", "k_apply_px_md<3, one plane, no gamma>"),
    ("apply", "md: gamma 2.2, offsets 1/64", "k_apply_px_md<3, one plane, gamma>"),
    ("apply", "existing FAST, aligned outputs", "k_apply_s4<3>"),
    ("generate", "existing RGB", "k_generate_rgb<HLG, aligned, 4 tiles>"),
    ("generate", "md RGB: gamma 1, offsets 1/64", "k_generate_md<HLG, aligned, 4 tiles, RGB>"),
    ("generate", "md RGB: gamma 2.2, offsets 1/64", "k_generate_md<HLG, aligned, 4 tiles, RGB>"),
    ("generate", "md one plane: gamma 1, offsets 1/64", "k_generate_md<HLG, aligned, 4 tiles, one plane>"),
    ("generate", "md one plane: gamma 2.2, offsets 1/64", "k_generate_md<HLG, aligned, 4 tiles, one plane>"),
]


def call(lib, st, k, s):
    group, name, _ = CASES[k]
    md = GAMMA if "2.2" in name else OFFSETS
    if group == "apply":
        if name.startswith("md"):
            rc = lib.uhdr_hip_apply_gainmap_md_batch(N, st.y, st.mono, C.byref(md), api.OUTPUT_HDR_HLG, FLT_MAX, st.out_off, api.APPLY_FAST, s)
        else:
            dst = st.out if "aligned" in name else st.out_off
            rc = lib.uhdr_hip_apply_gainmap_batch(N, st.y, st.mono, C.byref(DEGENERATE), api.OUTPUT_HDR_HLG, FLT_MAX, dst, api.APPLY_FAST, s)
    elif name == "existing RGB":
        rc = lib.uhdr_hip_generate_gainmap_rgb_batch(N, st.y, st.p, api.TF_HLG, C.byref(st.md), st.rgba_dst, 0, s)
    else:
        rgb = "RGB" in name
        rc = lib.uhdr_hip_generate_gainmap_md_batch(N, st.y, st.p, api.TF_HLG, C.byref(md), st.rgba_dst if rgb else st.mono_dst, 0, int(rgb), s)
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
    if group == "generate":
        return N * (W * H * 4.5 + MW * MH * (4 if "RGB" in name else 1))
    return N * (W * H * (1.5 + 4) + MW * MH)


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    once = "--once" in sys.argv
    print("device: %s; %d x %dx%d per call, %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
          (torch.cuda.get_device_name(0), N, W, H, BATCHES, WARMUP, REPS))
    sets = [Set(lib, 1000 * (b + 1), s) for b in range(BATCHES)]
    for st in sets:   # the maps the apply cases read are real ones (the last generate case rewrites the same kind of bytes)
        call(lib, st, len(CASES) - 2, s)
    torch.cuda.synchronize()
    order = [k for k, c in enumerate(CASES) if c[0] == "apply"] + [k for k, c in enumerate(CASES) if c[0] == "generate"]
    base = {}
    for k in order:
        group, name, kernels = CASES[k]
        if once:
            call(lib, sets[0], k, s)
            continue
        med, lo, hi = measure(lib, sets, k, s)
        base.setdefault(group, med)
        nbytes = bytes_moved(k)
        print("%-9s %-38s %8.3f ms [%8.3f .. %8.3f]  x%.3f of the group's first line;  %7.1f MB read + written, memory bound %.3f ms (%4.1f %% of 8 TB/s)" %
              (group, name, med, lo, hi, med / base[group], nbytes / 1e6, nbytes / HBM * 1e3, 100.0 * nbytes / HBM * 1e3 / med))
        print("          kernels expected from the dispatch rule (not traced): %s" % kernels)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
