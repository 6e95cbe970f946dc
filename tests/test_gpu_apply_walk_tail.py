"""The tail of k_apply_s4's walk: the wave goes on while ANY of its lanes has a next cell, and a lane without one computes its
cell again and stores the same bytes to the same addresses.  Frames whose map is no multiple of a wave, of a block or of a block's
stretch of cells, so that lanes run out at different steps; every output between 4 KiB of sentinel bytes that must come back
untouched (a lane that repeats a cell must never store anywhere else).

All shapes take the scale-4 walk (launch_apply_t: scale 4, map at least two cells wide, aligned planes)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = 3.4028234663852886e38
LSB_TOL = 1        # 10-bit code values      (tests/test_gpu_parity.py)
HALF_ULP_TOL = 1   # half-precision ULPs
GUARD = 4096
BPP = {1: 8, 2: 4, 3: 4, 4: 6}
MAX_BOOST = float(np.float32(1000.0) / np.float32(203.0))
# (display boost, masked kernel?): capped at 1.0 under a content boost of 4.9 the largest factor is 1.38, channels exceed 1.0 and
# launch_apply_t takes k_apply_s4<FMT, true>
BOOSTS = [FLT_MAX, 1.0]

# (width, height, frames in the batch, distinct frames)
SHAPES = [
    (8, 8, 2, 2),            # map 2 x 2: the minimum
    (72, 40, 2, 2),          # 180 cells: two whole waves and 52 lanes
    (260, 132, 2, 2),        # map 65 x 33 = 2 145 cells: waves wrap rows, the last wave has 33 lanes
    (3844, 24, 2, 2),        # map 961 x 6: the last column falls in a different lane on every row; lanes that go on and lanes that
                             # repeat share the last row (the F16 exchange path must not take them for 64 consecutive cells)
    (2052, 1028, 3, 3),      # map 513 x 257 = 131 841 cells, a batch of 3 (1 cell per thread) against single calls
    (2052, 1028, 4, 3),      # the same, 2 cells per thread: the last block's lanes run out at the first or the second step
    (2052, 1028, 50, 3),     # the same, 32 cells per thread, nine blocks per image: the last one ragged, lanes running out at
                             # different steps (inputs repeat, every output is a buffer of its own)
]


class Guarded:
    """an output buffer with GUARD sentinel bytes in front and behind"""

    def __init__(self, nbytes):
        import torch
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (self.t.data_ptr() + GUARD) % 16 == 0

    def ptr(self):
        return self.t.data_ptr() + GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.t[:GUARD] == 0xA5).all()) and bool((self.t[GUARD + self.n:] == 0xA5).all())


def worst_diff(fmt, a, b, wraps):
    """largest distance between two outputs: 10-bit codes per channel (modulo 1024 where channels may wrap), half-precision ULPs"""
    import torch
    if fmt in (2, 3):
        x, y = a.view(torch.int32), b.view(torch.int32)
        assert bool(((x >> 30) & 3 == (y >> 30) & 3).all())
        worst = 0
        for sh in (0, 10, 20):
            d = (((x >> sh) & 0x3ff) - ((y >> sh) & 0x3ff)).abs()
            if wraps:
                d = torch.minimum(d, 1024 - d)
            worst = max(worst, int(d.max()))
        return worst
    x, y = a.view(torch.int16).to(torch.int32), b.view(torch.int16).to(torch.int32)
    d = (x - y).abs()
    if fmt == 4 and wraps:
        d = torch.minimum(d, 1024 - d)
    return int(d.max())


@pytest.fixture(scope="module")
def inputs():
    """frames and maps per shape, made once and left unchanged"""
    import torch
    from libultrahdr_dev_amd import synth
    made = {}
    g = torch.Generator(device="cuda")
    g.manual_seed(4242)
    for w, h, _, distinct in SHAPES:
        if (w, h) not in made:
            frames = [synth.lcg_frame(w, h, 9300 + i) for i in range(distinct)]
            maps = [torch.randint(0, 256, ((w // 4) * (h // 4),), dtype=torch.uint8, device="cuda", generator=g) for _ in range(distinct)]
            made[(w, h)] = (frames, maps)
    return made


@pytest.mark.parametrize("fmt", [1, 2, 3, 4])
def test_walk_tail_bytes_and_sentinels(hip, inputs, fmt):
    import torch
    from tests.gpu_util import stream_ptr
    lib = hip.load()
    md = hip.metadata(MAX_BOOST)
    for w, h, n, distinct in SHAPES:
        assert w % 4 == 0 and h % 4 == 0 and w // 4 >= 2
        frames, maps = inputs[(w, h)]
        nbytes = w * h * BPP[fmt]
        yi = [hip.yuv420_image(frames[i % distinct][1].data_ptr(), w, h, hip.CG_BT709) for i in range(n)]
        mi = [hip.mono_image(maps[i % distinct].data_ptr(), w // 4, h // 4) for i in range(n)]
        for boost in BOOSTS:
            wraps = boost < MAX_BOOST
            big = [Guarded(nbytes) for _ in range(n)]
            ya, ma = hip.image_array(yi), hip.image_array(mi)
            ba = hip.image_array([hip.out_image(t.ptr()) for t in big])
            assert lib.uhdr_hip_apply_gainmap_batch(n, ya, ma, C.byref(md), fmt, boost, ba, hip.APPLY_FAST, stream_ptr()) == 0
            single, exact = [], []
            for i in range(distinct):
                one, ex = Guarded(nbytes), Guarded(nbytes)
                oi, ei = hip.out_image(one.ptr()), hip.out_image(ex.ptr())
                assert lib.uhdr_hip_apply_gainmap(C.byref(yi[i]), C.byref(mi[i]), C.byref(md), fmt, boost, C.byref(oi), hip.APPLY_FAST,
                                                  hip.MEM_DEVICE, stream_ptr()) == 0
                assert lib.uhdr_hip_apply_gainmap(C.byref(yi[i]), C.byref(mi[i]), C.byref(md), fmt, boost, C.byref(ei), hip.APPLY_EXACT,
                                                  hip.MEM_DEVICE, stream_ptr()) == 0
                single.append(one)
                exact.append(ex)
            torch.cuda.synchronize()
            tag = "fmt %d %dx%d x%d boost %s" % (fmt, w, h, n, "max" if boost == FLT_MAX else boost)
            for i, t in enumerate(big):
                assert t.guards_intact(), "%s: frame %d of the batch wrote outside its image" % (tag, i)
                assert torch.equal(t.body(), single[i % distinct].body()), \
                    "%s: frame %d: batch and single-image launches disagree in %d bytes" % (tag, i, int((t.body() != single[i % distinct].body()).sum()))
            worst = 0
            for one, ex in zip(single, exact):
                assert one.guards_intact() and ex.guards_intact(), "%s: a single-image launch wrote outside its image" % tag
                worst = max(worst, worst_diff(fmt, one.body(), ex.body(), wraps))
            print("%s: worst distance from the bit-exact mode %d" % (tag, worst))
            assert worst <= (HALF_ULP_TOL if fmt == 1 else LSB_TOL), (tag, worst)
