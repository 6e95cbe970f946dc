"""Times the content-adaptive generate against the constant-range one on one GPU (profiles/r05_adaptive.txt).

    python scripts/time_adaptive.py               # (a) and (b) below
    python scripts/time_adaptive.py --once        # one untimed pass of both device-level calls, for rocprofv3 --kernel-trace --stats

(a) 64 x 4K LCG frames, HLG and PQ, rotating over 3 resident batches as bench.py does: uhdr_hip_generate_gainmap_adaptive_batch
    (PER_IMAGE and PER_CALL) against uhdr_hip_generate_gainmap_batch with content_minmax, one process, alternating windows of
    CALLS calls each, device events around every window.  Figures: ms per call, median [min .. max] over the windows, and the ratio
    of the medians.
(b) uhdr_hip_jpegr_encode_adaptive_batch against uhdr_hip_jpegr_encode_batch, 16 smooth 4K files, API-1, device planes, HLG,
    quality 90: wall time of the call (it synchronises), median [min .. max] of REPS.
Pass 1 of the adaptive call evaluates every pixel on the exact path: there is no estimate and therefore no pixel
"in doubt" in pass 2; the script says so where a filtered design would print that fraction."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch         # noqa: E402

from libultrahdr_dev_amd import api, synth   # noqa: E402

W, H, N, BATCHES = 3840, 2160, 64, 3
WINDOWS, CALLS = 7, 6
FILES, REPS = 16, 7


def stat(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


class Batch:
    def __init__(self, seed):
        self.keep = [synth.lcg_frame(W, H, seed + i) for i in range(N)]
        self.ya = api.image_array([api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709) for _, y in self.keep])
        self.pa = api.image_array([api.p010_image(p.data_ptr(), W, H, api.CG_BT2100) for p, _ in self.keep])
        self.maps = torch.empty(N * (W // 4) * (H // 4), dtype=torch.uint8, device="cuda")
        self.da = api.image_array([api.out_image(self.maps.data_ptr() + i * (W // 4) * (H // 4)) for i in range(N)])
        self.yuv_images = [api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709) for _, y in self.keep]


def device_level(lib, once):
    batches = [Batch(1000 + 100 * b) for b in range(BATCHES)]
    mm = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
    rng = torch.zeros(2 * N, dtype=torch.float32, device="cuda")
    nb = api.adaptive_workspace_bytes(batches[0].yuv_images)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    md = api.Metadata()
    print("workspace of the adaptive call: %.1f MiB for %d x %dx%d" % (nb / 2 ** 20, N, W, H))

    def const(b, tf):
        assert lib.uhdr_hip_generate_gainmap_batch(N, b.ya, b.pa, tf, C.byref(md), b.da, 0, C.c_void_p(mm.data_ptr()), s) == 0

    def adaptive(scope):
        def call(b, tf):
            assert lib.uhdr_hip_generate_gainmap_adaptive_batch(N, b.ya, b.pa, tf, b.da, 0, scope, C.c_void_p(mm.data_ptr()), C.c_void_p(rng.data_ptr()),
                                                                C.c_void_p(ws.data_ptr()), nb, s) == 0
        return call
    variants = [("constant range + content_minmax", const), ("adaptive PER_IMAGE", adaptive(api.BOOST_PER_IMAGE)),
                ("adaptive PER_CALL", adaptive(api.BOOST_PER_CALL))]
    if once:
        for tf in (api.TF_HLG, api.TF_PQ):
            for _, fn in variants[:2]:
                fn(batches[0], tf)
        torch.cuda.synchronize()
        return
    for tf, name in ((api.TF_HLG, "HLG"), (api.TF_PQ, "PQ")):
        times = {v[0]: [] for v in variants}
        k = 0
        for w in range(WINDOWS + 1):   # (the first window warms up)
            for vname, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    fn(batches[k % BATCHES], tf)
                    k += 1
                e1.record()
                e1.synchronize()
                if w > 0:
                    times[vname].append(e0.elapsed_time(e1) / CALLS)
        base = stat(times[variants[0][0]])
        for vname, _ in variants:
            t = stat(times[vname])
            print("(a) %-3s %-34s %7.3f ms per call  [%7.3f .. %7.3f]   x %.2f" % (name, vname, *t, t[0] / base[0]))
    print("(a) pass 2 pixels in doubt: none by construction (pass 1 stores exact gains; no estimate is made)")


def file_level(lib):
    frames = [synth.smooth_frame(W, H, 300 + i) for i in range(FILES)]
    pa = api.image_array([api.p010_image(p.data_ptr(), W, H, api.CG_BT2100) for p, _ in frames])
    ya = api.image_array([api.yuv420_image(y.data_ptr(), W, H, api.CG_BT709) for _, y in frames])
    cap = W * H * 2
    import numpy as np
    bufs = [np.empty(cap, np.uint8) for _ in range(FILES)]
    outs, caps = (C.c_void_p * FILES)(*[b.ctypes.data for b in bufs]), (C.c_size_t * FILES)(*([cap] * FILES))
    sizes, status = (C.c_size_t * FILES)(), (C.c_int * FILES)()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def const():
        assert lib.uhdr_hip_jpegr_encode_batch(FILES, pa, ya, api.TF_HLG, 90, None, None, outs, caps, sizes, status, api.MEM_DEVICE, s) == 0

    def adaptive():
        assert lib.uhdr_hip_jpegr_encode_adaptive_batch(FILES, pa, ya, api.TF_HLG, 90, None, None, outs, caps, sizes, None, status, api.BOOST_PER_IMAGE,
                                                        api.MEM_DEVICE, s) == 0
    res = {}
    for name, fn in (("uhdr_hip_jpegr_encode_batch", const), ("uhdr_hip_jpegr_encode_adaptive_batch", adaptive)) * 2:
        fn()
        ts = res.setdefault(name, [])
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    base = stat(res["uhdr_hip_jpegr_encode_batch"])
    for name, ts in res.items():
        t = stat(ts)
        print("(b) %-40s %8.2f ms per %d files  [%8.2f .. %8.2f]   x %.2f" % (name, t[0], FILES, t[1], t[2], t[0] / base[0]))


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    once = "--once" in sys.argv
    device_level(lib, once)
    if not once:
        file_level(lib)


if __name__ == "__main__":
    main()
