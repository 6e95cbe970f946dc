"""Times the batched edit effects on one GPU (profiles/r05_effects_batch.txt).

    python scripts/time_effects_batch.py               # cases (a), (b), (c): warm-up, then REPS timed repetitions each
    python scripts/time_effects_batch.py --once a      # one untimed pass of case (a), for rocprofv3 --kernel-trace --stats

(a) 32 x 1920x1080 YUV420 + 32 x 480x270 monochrome through resize(960,540), mirror(1), rotate 90, crop(10,499,20,899):
    uhdr_hip_add_effects_batch against a loop of uhdr_hip_add_effects over the same 64 images.
(b) the same images through the one-step chains rotate 90, mirror(1), resize(960,540), the same two ways.
(c) uhdr_hip_jpegr_edit_batch, n = 1, 4, 16 4K files, rotate 90 on both images, against its composition from the calls that were
    there before it: uhdr_hip_jpeg_decode_batch x2, 2n x uhdr_hip_add_effects, uhdr_hip_jpegr_encode_apix_batch.
Every figure is wall time of the call(s) plus the stream's synchronisation, in microseconds: median [min .. max] of REPS."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from libultrahdr_dev_amd import api   # noqa: E402

WARMUP, REPS = 5, 30
CHAIN_A = [(3, 960, 540, 0, 0), (1, 1, 0, 0, 0), (2, 90, 0, 0, 0), (0, 10, 499, 20, 899)]
ONE_STEP = {"rotate 90": [(2, 90, 0, 0, 0)], "mirror(1)": [(1, 1, 0, 0, 0)], "resize(960,540)": [(3, 960, 540, 0, 0)]}


def effects(chain):
    arr = (api.Effect * max(len(chain), 1))()
    for i, e in enumerate(chain):
        arr[i] = api.Effect(*e)
    return arr


def measure(fn, reps=REPS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t):
    return "%9.1f us  [%9.1f .. %9.1f]" % t


class Images:
    """32 x 1080p YUV420 + 32 x 480x270 monochrome in device memory, and room for every result"""

    def __init__(self):
        g = torch.Generator(device="cuda").manual_seed(5)
        self.n = 64
        self.src, self.dst, self.imgs = [], [], (api.Image * 64)()
        for i in range(64):
            mono = i >= 32
            w, h = (480, 270) if mono else (1920, 1080)
            nbytes = w * h if mono else w * h * 3 // 2
            t = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
            self.src.append(t)
            self.dst.append(torch.empty(1920 * 1080 * 3 // 2 + 64, dtype=torch.uint8, device="cuda"))
            self.imgs[i] = api.Image(t.data_ptr(), w, h, 1, None, 0, 0, api.PIX_FMT_MONOCHROME if mono else api.PIX_FMT_YUV420)
        self.out = (C.c_void_p * 64)(*[d.data_ptr() for d in self.dst])
        self.cap = (C.c_size_t * 64)(*[d.numel() for d in self.dst])
        self.descs, self.status = (api.Image * 64)(), (C.c_int * 64)()

    def batch(self, lib, fx, n_fx, s):
        rc = lib.uhdr_hip_add_effects_batch(64, self.imgs, fx, n_fx, self.out, self.cap, self.descs, self.status, s)
        assert rc == 0, rc

    def loop(self, lib, fx, n_fx, s):
        for i in range(64):
            o = api.out_image(self.dst[i].data_ptr())
            rc = lib.uhdr_hip_add_effects(C.byref(self.imgs[i]), fx, n_fx, C.byref(o), api.MEM_DEVICE, s)
            assert rc == 0, rc


def jpegr_4k(lib, s):
    """one 3840x2160 JPEG/R file (API-1 of a synthetic frame pair, quality 90)"""
    w, h = 3840, 2160
    p = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
    y = torch.empty(w * h * 3 // 2, dtype=torch.uint8, device="cuda")
    assert lib.uhdr_hip_synth_lcg_frame(w, h, 11, C.c_void_p(p.data_ptr()), C.c_void_p(y.data_ptr()), s) == 0
    torch.cuda.synchronize()
    pi, yi = api.p010_image(p.data_ptr(), w, h, api.CG_BT2100), api.yuv420_image(y.data_ptr(), w, h, api.CG_BT709)
    buf, n = np.zeros(w * h * 3, np.uint8), C.c_size_t()
    rc = lib.uhdr_hip_jpegr_encode_api1(C.byref(pi), C.byref(yi), api.TF_HLG, 90, None, 0, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n), api.MEM_DEVICE, s)
    assert rc == 0, rc
    return buf[:n.value].copy()


class EditCase:
    def __init__(self, lib, data, n, s):
        self.lib, self.n, self.s, self.data = lib, n, s, data
        self.jp = (C.c_void_p * n)(*[data.ctypes.data] * n)
        self.jn = (C.c_size_t * n)(*[data.size] * n)
        self.bufs = [np.zeros(data.size * 2, np.uint8) for _ in range(n)]
        self.out = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.cap = (C.c_size_t * n)(*[b.size for b in self.bufs])
        self.size, self.status = (C.c_size_t * n)(), (C.c_int * n)()
        self.fx = effects([(2, 90, 0, 0, 0)])
        pr, gm = api.JpegInfo(), api.JpegInfo()
        assert lib.uhdr_hip_jpegr_info(C.c_void_p(data.ctypes.data), data.size, C.byref(pr), C.byref(gm)) == 0
        self.md = api.Metadata()
        assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(data.ctypes.data), data.size, C.byref(self.md)) == 0
        w, h, mw, mh = pr.width, pr.height, gm.width, gm.height
        self.pj = (C.c_void_p * n)(*[data.ctypes.data + pr.offset] * n)
        self.pn = (C.c_size_t * n)(*[pr.size] * n)
        self.gj = (C.c_void_p * n)(*[data.ctypes.data + gm.offset] * n)
        self.gn = (C.c_size_t * n)(*[gm.size] * n)
        mk = lambda nb: [torch.empty(nb, dtype=torch.uint8, device="cuda") for _ in range(n)]
        self.dy, self.dg, self.ey, self.eg = mk(w * h * 3 // 2), mk(mw * mh * 3 // 2), mk(w * h * 3 // 2 + 64), mk(mw * mh + 64)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        cap = lambda ts: (C.c_size_t * n)(*[t.numel() for t in ts])
        self.dyp, self.dyc, self.dgp, self.dgc = arr(self.dy), cap(self.dy), arr(self.dg), cap(self.dg)
        self.ydesc, self.gdesc = (api.Image * n)(), (api.Image * n)()
        self.mds = (api.Metadata * n)(*[self.md] * n)

    def edit(self):
        rc = self.lib.uhdr_hip_jpegr_edit_batch(self.n, self.jp, self.jn, self.fx, 1, self.fx, 1, None, 90, self.out, self.cap, self.size, self.status, self.s)
        assert rc == 0, (rc, list(self.status))

    def composed(self):
        lib, n, s = self.lib, self.n, self.s
        assert lib.uhdr_hip_jpeg_decode_batch(n, self.pj, self.pn, api.DECODE_TO_YCBCR, self.dyp, self.dyc, self.ydesc, None, api.MEM_DEVICE, s) == 0
        assert lib.uhdr_hip_jpeg_decode_batch(n, self.gj, self.gn, api.DECODE_TO_YCBCR, self.dgp, self.dgc, self.gdesc, None, api.MEM_DEVICE, s) == 0
        yo, go = (api.Image * n)(), (api.Image * n)()
        for i in range(n):
            self.ydesc[i].colorGamut = api.CG_BT709
            yo[i], go[i] = api.out_image(self.ey[i].data_ptr()), api.out_image(self.eg[i].data_ptr())
            g = self.gdesc[i]
            gi = api.mono_image(g.data, g.width, g.height)
            assert lib.uhdr_hip_add_effects(C.byref(self.ydesc[i]), self.fx, 1, C.byref(yo[i]), api.MEM_DEVICE, s) == 0
            assert lib.uhdr_hip_add_effects(C.byref(gi), self.fx, 1, C.byref(go[i]), api.MEM_DEVICE, s) == 0
        rc = lib.uhdr_hip_jpegr_encode_apix_batch(n, yo, go, self.mds, 90, None, None, self.out, self.cap, self.size, self.status, api.MEM_DEVICE, s)
        assert rc == 0, (rc, list(self.status))


def main():
    torch.cuda.set_device(0)
    lib = api.init(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    im = Images()
    if "--once" in sys.argv:
        fx = effects(CHAIN_A)
        for _ in range(3):
            im.batch(lib, fx, len(CHAIN_A), s)
            im.loop(lib, fx, len(CHAIN_A), s)
        torch.cuda.synchronize()
        return
    print("device: %s; %d warm-up + %d timed repetitions per figure; median [min .. max]" % (torch.cuda.get_device_name(0), WARMUP, REPS))
    fx = effects(CHAIN_A)
    print("(a) 4-step chain, 64 images")
    print("    uhdr_hip_add_effects_batch        %s" % fmt(measure(lambda: im.batch(lib, fx, 4, s))))
    print("    64 x uhdr_hip_add_effects         %s" % fmt(measure(lambda: im.loop(lib, fx, 4, s))))
    print("    64 x uhdr_hip_add_effects (again) %s" % fmt(measure(lambda: im.loop(lib, fx, 4, s))))
    print("(b) one-step chains, 64 images")
    for name, chain in ONE_STEP.items():
        f1 = effects(chain)
        print("    %-16s batch             %s" % (name, fmt(measure(lambda: im.batch(lib, f1, 1, s)))))
        print("    %-16s 64 x single call  %s" % (name, fmt(measure(lambda: im.loop(lib, f1, 1, s)))))
    print("(c) JPEG/R edit, 3840x2160 files, rotate 90 on both images")
    data = jpegr_4k(lib, s)
    for n in (1, 4, 16):
        e = EditCase(lib, data, n, s)
        print("    n = %2d  uhdr_hip_jpegr_edit_batch  %s" % (n, fmt(measure(e.edit, reps=20, warmup=3))))
        print("    n = %2d  composed from the parts    %s" % (n, fmt(measure(e.composed, reps=20, warmup=3))))
        print("    n = %2d  composed (again)           %s" % (n, fmt(measure(e.composed, reps=20, warmup=3))))


if __name__ == "__main__":
    main()
