"""Times the tone-mapped SDR base image on one GPU (profiles/r07_tonemap.txt).

    python scripts/time_tonemap.py              # one 3840x2160 frame and 64 of them; HLG and PQ; measured and given headroom
    python scripts/time_tonemap.py --once       # one untimed pass of every case, for rocprofv3 --kernel-trace --stats

uhdr_hip_tonemap_sdr_batch (REINHARD_MAXRGB) against uhdr_hip_tonemap_batch -- the bit shift it replaces in API-0 -- in the same
process on the same frames.  The calls rotate over BATCHES resident sets of frames, as bench.py does, so that no launch finds its
input in a cache the launch before it filled.  Times are device events around REPS calls, in milliseconds per call.

Bytes moved per pixel: the shift and a given headroom read the P010 planes once (3 B) and write 1.5 B; a measured headroom reads
them twice (k_tonemap_peak, then k_tonemap_sdr).  The bounds printed beside the time:
    memory      bytes / 8 TB/s
    arithmetic  the f64 polynomial work of the exact inverse OETFs (lean log2 / exp2: ~19 f64 operations each; PQ takes two of each
                per channel, HLG one exp2) at the f64 vector rate, 39.3e12 operations/s, plus the f32 special-function
                instructions (3 v_log_f32, 3 v_exp_f32, 1 v_rcp_f32 per pixel for step 5 and the sRGB OETF) at a quarter of
                the f32 rate, 19.7e12/s.  Counts are read off csrc/uhdr_device_math.h, not measured.
The kernel names beside each figure are the ones the dispatch rule selects for these frames (aligned, 16-column multiples); they
are not read from a trace -- `rocprofv3 --kernel-trace --stats -- python scripts/time_tonemap.py --once` shows what ran."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

W, H = 3840, 2160
BATCHES, WARMUP, REPS = 3, 3, 12
HBM = 8.0e12
F64_RATE, SFU_RATE = 39.3e12, 19.7e12
F64_OPS_PER_CHANNEL = {api.TF_HLG: 19 + 6, api.TF_PQ: 4 * 19 + 12, api.TF_LINEAR: 0}
KERNELS = {"shift": "k_tonemap_luma<true>, k_tonemap_chroma<true>",
           "measured": "k_tonemap_head_init, k_tonemap_peak<true>, k_tonemap_head_finish<TF>, k_tonemap_sdr<TF, true>",
           "given": "k_tonemap_head_init, k_tonemap_sdr<TF, true>"}


class Set:
    """n resident 4K frames (LCG noise, distinct seeds) and their destination planes"""

    def __init__(self, lib, n, seed, s):
        self.n = n
        self.src = [torch.empty(W * H * 3, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.dst = [torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda") for _ in range(n)]
        scratch = torch.empty(W * H * 3 // 2, dtype=torch.uint8, device="cuda")
        for i, t in enumerate(self.src):
            assert lib.uhdr_hip_synth_lcg_frame(W, H, seed + i, C.c_void_p(t.data_ptr()), C.c_void_p(scratch.data_ptr()), s) == 0
        torch.cuda.synchronize()
        self.p = api.image_array([api.p010_image(t.data_ptr(), W, H, api.CG_BT2100) for t in self.src])
        self.d = api.image_array([api.yuv420_image(t.data_ptr(), W, H, api.CG_UNSPECIFIED) for t in self.dst])
        self.head = torch.zeros(max(n, 64), dtype=torch.float32, device="cuda")
        self.peaks = (C.c_float * n)(*([1000.0] * n))


def call(lib, st, tf, mode, s):
    if mode == "shift":
        rc = lib.uhdr_hip_tonemap_batch(st.n, st.p, st.d, s)
    else:
        rc = lib.uhdr_hip_tonemap_sdr_batch(st.n, st.p, st.d, tf, api.TONEMAP_REINHARD_MAXRGB, st.peaks if mode == "given" else None,
                                            C.c_void_p(st.head.data_ptr()), s)
    assert rc == 0, (rc, lib.uhdr_hip_last_error())


def measure(lib, sets, tf, mode, s):
    for k in range(WARMUP):
        call(lib, sets[k % len(sets)], tf, mode, s)
    torch.cuda.synchronize()
    ts = []
    for k in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(lib, sets[k % len(sets)], tf, mode, s)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def bounds(n, tf, mode):
    px = n * W * H
    nbytes = px * (7.5 if mode == "measured" else 4.5)
    arith = 0.0 if mode == "shift" else px * 3 * F64_OPS_PER_CHANNEL[tf] / F64_RATE + px * 7 / SFU_RATE
    return nbytes, nbytes / HBM * 1e3, arith * 1e3


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    once = "--once" in sys.argv
    print("device: %s; %d resident sets, %d warm-up + %d timed calls per figure; ms per call: median [min .. max]" %
          (torch.cuda.get_device_name(0), BATCHES, WARMUP, REPS))
    for n in (1, 64):
        sets = [Set(lib, n, 100 * (k + 1), s) for k in range(BATCHES)]
        for tf, tfname in ((api.TF_HLG, "HLG"), (api.TF_PQ, "PQ")):
            for mode in ("shift", "measured", "given"):
                if mode == "shift" and tf != api.TF_HLG:
                    continue   # (the shift does not look at the transfer function)
                if once:
                    call(lib, sets[0], tf, mode, s)
                    continue
                med, lo, hi = measure(lib, sets, tf, mode, s)
                nbytes, t_mem, t_arith = bounds(n, tf, mode)
                nearer = "memory" if abs(med - t_mem) <= abs(med - t_arith) or t_arith == 0.0 else "arithmetic issue"
                print("%2d x 4K  %-3s %-8s %8.3f ms [%8.3f .. %8.3f]  %7.1f MB moved, %5.1f %% of 8 TB/s;  bounds: memory %.3f ms, arithmetic %.3f ms "
                      "-> nearer to the %s bound" % (n, tfname if mode != "shift" else "-", mode, med, lo, hi, nbytes / 1e6, 100.0 * t_mem / med,
                                                     t_mem, t_arith, nearer))
                print("         kernels expected from the dispatch rule (not traced): %s" % KERNELS[mode].replace("TF", "1" if tf == api.TF_HLG else "2"))
        del sets
        torch.cuda.empty_cache()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
