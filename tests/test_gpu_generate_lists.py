"""-m gpu: the bookkeeping between generate's filtered kernel (k_generate<..., FILTER, DEFER>) and k_generate_resolve at its limits.

The filtered kernel hands the pairs whose byte its f32 estimate cannot settle to the resolve kernel: per wave, 4 entries that leave
with their sampled values and 15 plain ones (slot mode: images of at most 1024 waves), or per list of 252 (64 lists per image);
anything beyond sweeps the image.  A pixel in doubt nearly always has the right provisional byte already, so comparing final bytes
says little about an entry that is dropped, misplaced or duplicated.  These tests run the two kernels one at a time
(uhdr_hip_generate_probe) on frames whose pixels in doubt are known by construction (tests/generate_list_cases.py), read the header
words the filtered kernel left, fill the maps with a byte no pixel has and let the resolve kernel run: what it wrote is exactly
what is not poison afterwards.  Every case asserts
  (a) every byte the resolve kernel wrote is the oracle's;
  (b) every other byte is still poison: the written set is the designed set, or the whole image where a sweep is designed;
  (c) the production call on the same frames equals GENERATE_UNFILTERED and the oracle byte for byte;
  (d) with statistics, min and max equal the oracle's bit for bit (the minimum, 1.0, is a pixel in doubt's: only the resolve
      kernel can have contributed it);
and, without statistics, that every count word, list count and sweep word equals the designed value (with statistics the
candidates add entries: the designed counts are lower bounds, and the cases keep them at most 6 or at least 40 per wave).
All frames, maps and snapshots of a case live in one allocation each, images side by side."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import generate_list_cases as K

pytestmark = pytest.mark.gpu

A_SHAPE, B_SHAPE, C_SHAPE, D_SHAPE = (1024, 512, 64), (1040, 504, 64), (4096, 2048, 4), (4096, 2056, 4)
E_SHAPE, F_SHAPE = (1024, 512, 8), (3840, 2160, 1)


@pytest.fixture
def side(hip):
    """a stream of the test's own, current while the test runs and handed back at the end: a failure between the two phases
    leaves entries in this stream's workspace only, and the workspace goes with the stream"""
    lib = hip.load()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        assert lib.uhdr_hip_stream_release(C.c_void_p(s.cuda_stream)) == 0


class _Dev:
    """a shape's descriptors over one allocation per plane kind"""

    def __init__(self, hip, w, h, n, tf, stats):
        self.hip, self.lib, self.w, self.h, self.n, self.tf = hip, hip.load(), w, h, n, tf
        fb = w * h * 3 // 2
        self.yuv = torch.empty((n, fb), dtype=torch.uint8, device="cuda")
        self.p010 = torch.empty((n, fb), dtype=torch.int16, device="cuda")
        self.maps = torch.full((n, w * h // 16), K.POISON, dtype=torch.uint8, device="cuda")
        self.mm = torch.full((2 * n,), 7.0, dtype=torch.float32, device="cuda") if stats else None
        self.ya = hip.image_array([hip.yuv420_image(self.yuv.data_ptr() + i * fb, w, h, K.GAMUT) for i in range(n)])
        self.pa = hip.image_array([hip.p010_image(self.p010.data_ptr() + 2 * i * fb, w, h, K.GAMUT) for i in range(n)])
        self.da = hip.image_array([hip.out_image(self.maps.data_ptr() + i * (w * h // 16)) for i in range(n)])
        self.md = hip.Metadata()

    def load(self, case):
        self.yuv.copy_(torch.from_numpy(case.yuv))
        self.p010.copy_(torch.from_numpy(case.p010.view(np.int16)))

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def probe(self, phase, route=None, headers=None, n=None):
        mm = C.c_void_p(self.mm.data_ptr()) if self.mm is not None else None
        return self.lib.uhdr_hip_generate_probe(phase, self.n if n is None else n, self.ya, self.pa, self.tf, C.byref(self.md), self.da, 0,
                                                self.hip.GENERATE_EXACT, mm, self.stream(), route,
                                                None if headers is None else C.c_void_p(headers.data_ptr()))

    def route(self, n=None):
        r = (C.c_uint32 * self.hip.ROUTE_WORDS)()
        assert self.probe(0, route=r, n=n) == 0
        return dict(zip(K.ROUTE_KEYS, list(r)))

    def production(self, mode):
        self.maps.fill_(0xEE)
        mm = None
        if self.mm is not None:
            self.mm.fill_(7.0)
            mm = C.c_void_p(self.mm.data_ptr())
        assert self.lib.uhdr_hip_generate_gainmap_batch_ex(self.n, self.ya, self.pa, self.tf, C.byref(self.md), self.da, 0, mode, mm, self.stream()) == 0
        torch.cuda.current_stream().synchronize()
        return self.maps.cpu().numpy().copy(), (self.mm.cpu().numpy().view(np.uint32).copy() if self.mm is not None else None)


def _route_of(hip, shape, stats=False, tf=1):
    """the route of a shape from descriptors alone (phase 0 reads no pixel)"""
    return _Dev(hip, *shape, tf, stats).route()


def _run(dev, case, route, orc=None):
    """the two phases with the snapshot and the poison between them, then the assertions every case shares; -> the snapshot"""
    n, mw, mh = case.n, case.mw, case.mh
    stats = dev.mm is not None
    t0 = time.time()
    dev.load(case)
    torch.cuda.current_stream().synchronize()
    t1 = time.time()
    dev.maps.fill_(0x11)
    snap_d = torch.full((n, route["hdr_words"]), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    assert dev.probe(1, headers=snap_d) == 0
    dev.maps.fill_(K.POISON)
    assert dev.probe(2) == 0
    torch.cuda.current_stream().synchronize()
    snap = snap_d.cpu().numpy().view(np.uint32)
    got = dev.maps.cpu().numpy().reshape(n, mh, mw)
    hdr, swept = case.header(route)
    want_written = case.designed | swept[:, None, None]
    written = got != K.POISON
    lc = route["list_counts"]
    print("\n%dx%dx%d tf %d stats %d: upload %.3f s, phases %.3f s; designed pixels %d, written %d, swept designed %s, sweep words %s, "
          "list counts (max per image) %s, slot count words set %d, min/max %s"
          % (case.w, case.h, n, case.tf, stats, t1 - t0, time.time() - t1, case.designed.sum(), written.sum(), list(np.nonzero(swept)[0]),
             list(snap[:, route["sweep_word"]]), list(snap[:, lc:lc + route["lists"]].max(axis=1)),
             (snap[:, route["slot_counts"]:route["slot_counts"] + route["slots"]] != 0).sum(),
             dev.mm.cpu().numpy()[:4].tolist() if stats else None))
    for i in range(n):   # (b), then (a)
        assert np.array_equal(written[i], want_written[i]), ("image %d: written but not designed %d, designed but not written %d, swept %s"
                                                             % (i, (written[i] & ~want_written[i]).sum(), (~written[i] & want_written[i]).sum(), swept[i]))
    assert np.array_equal(got[written], case.expect[written])
    if not stats:   # every word the launch owns, exactly
        limit = hdr.shape[1] if route["slots"] else route["slot_counts"]
        bad = np.argwhere(snap[:, :limit] != hdr[:, :limit])
        assert bad.size == 0, [(int(i), int(j), int(snap[i, j]), int(hdr[i, j])) for i, j in bad[:8]]
    else:           # candidates add plain entries: the designed counts are lower bounds, the saved entries are the pairs in doubt's alone
        for (img, blk, wave), k in case.pairs.items():
            if route["slots"]:
                j = route["slot_counts"] + blk * (route["block"] // 64) + wave
                if hdr[img, j] == 0:
                    assert snap[img, j] == 0 and snap[img, route["sweep_word"]] == 1, (img, blk, wave)
                else:
                    assert snap[img, j] >> 8 == hdr[img, j] >> 8 and (snap[img, j] & 0xFF) >= (hdr[img, j] & 0xFF), (img, blk, wave, snap[img, j])
        if not route["slots"]:
            lc = slice(route["list_counts"], route["list_counts"] + route["lists"])
            assert (snap[:, lc] >= hdr[:, lc]).all()
    probe_mm = dev.mm.cpu().numpy().view(np.uint32).copy() if stats else None
    # (c) the production call, filtered and unfiltered, against the oracle
    fm, fmm = dev.production(dev.hip.GENERATE_EXACT)
    um, umm = dev.production(dev.hip.GENERATE_UNFILTERED)
    assert np.array_equal(fm.reshape(n, mh, mw), case.expect) and np.array_equal(um.reshape(n, mh, mw), case.expect)
    if stats:       # (d)
        want = np.empty(2 * n, np.float32)
        for i in range(n):
            st, om, _, omm = orc.generate("orc_", orc.yuv420_image(case.yuv[i], case.w, case.h, K.GAMUT), orc.p010_image(case.p010[i], case.w, case.h, K.GAMUT),
                                          case.tf, False, threads=8, stats=True)
            assert st == 0 and np.array_equal(om, case.expect[i])
            want[2 * i:2 * i + 2] = omm
            assert omm[0] == 1.0 or not case.designed[i].any()
        want = want.view(np.uint32)
        assert np.array_equal(probe_mm, want) and np.array_equal(fmm, want) and np.array_equal(umm, want)
    return snap


def _wave_key(route, img, wave):
    per = route["block"] // 64
    return (img, wave // per, wave % per)


def _slot_placement(route, n, waves, last=63):
    """the layouts of generate_list_cases.wave_layouts, each in a wave of its own: the first wave, the last one and waves between;
    images 0 and 1 without a sweep, images 2 and 3 swept, image n - 1 again without, every other image and wave clean"""
    lay = K.wave_layouts(route, last)
    full = K.wave_layouts(route)
    end = waves - 1
    pl = {}
    pl[_wave_key(route, 0, 0)] = full["first_lane"][0]
    pl[_wave_key(route, 0, end)] = lay["last_lane"][0]
    for j, name in enumerate(k for k in full if k not in ("first_lane", "last_lane", "plain_plus_one", "whole_tile")):
        pl[_wave_key(route, 0, 5 + 2 * j)] = full[name][0]
    pl[_wave_key(route, 1, 0)] = full["plain_full"][0]
    pl[_wave_key(route, 1, end - 1)] = full["saved_full"][0]
    pl[_wave_key(route, 1, end)] = lay["plain_full"][0]
    pl[_wave_key(route, 2, 0)] = full["first_lane"][0]
    pl[_wave_key(route, 2, end)] = lay["plain_plus_one"][0]
    pl[_wave_key(route, 3, 1)] = full["whole_tile"][0]
    pl[_wave_key(route, n - 1, 0)] = full["saved_plus_one"][0]
    pl[_wave_key(route, n - 1, end)] = lay["saved_plus_one"][0]
    return pl


def _assert_slot_route(route, n, waves):
    assert (route["resolve"], route["spans"], route["slots"], route["images"]) == (1, 4, waves, n), route


def test_layout_count_words_at_the_limits(hip):
    """the count words the layouts stand for, spelled out once: 4 pairs 0 | 4 << 8, 5 pairs 1 | 4 << 8, 19 pairs 15 | 4 << 8, 20 pairs 0 + sweep"""
    route = _route_of(hip, A_SHAPE)
    _assert_slot_route(route, 64, 64)
    assert (route["slot_saved"], route["slot_plain"], route["list_cap"], route["lists"]) == (4, 15, 252, 64)
    lay = K.wave_layouts(route)
    assert [(len(lay[k][0]), lay[k][1], lay[k][2]) for k in ("saved_full", "saved_plus_one", "saved_across_tiles", "plain_full", "plain_plus_one", "whole_tile")] == \
        [(4, 0 | 4 << 8, False), (5, 1 | 4 << 8, False), (6, 2 | 4 << 8, False), (19, 15 | 4 << 8, False), (20, 0, True), (64, 0, True)]
    assert min(e for e in lay["saved_across_tiles"][0] if e[0] == 2) == (2, 2, 1)


def test_single_phases_refused_where_the_route_has_no_resolve_kernel(hip, side):
    """1024 x 512 x 63 without statistics is 1008 spans: the small route, no k_generate_resolve -- phases 1 and 2 refuse it, and so they
    do a call of two chunks"""
    dev = _Dev(hip, 1024, 512, 64, 1, False)
    assert dev.route(n=63)["resolve"] == 0 and dev.route(n=64)["resolve"] == 1
    snap = torch.zeros((64, dev.route()["hdr_words"]), dtype=torch.int32, device="cuda")
    for phase in (1, 2):
        assert dev.probe(phase, headers=snap, n=63) == hip.ERROR_UNSUPPORTED_FEATURE
    assert dev.probe(3, headers=snap) == hip.ERROR_UNSUPPORTED_FEATURE
    assert dev.probe(1, headers=None) == hip.ERROR_BAD_PTR
    dev.ya[40].colorGamut = 1   # two chunks: 40 images, then 24
    assert dev.route()["images"] == 40
    for phase in (1, 2):
        assert dev.probe(phase, headers=snap) == hip.ERROR_UNSUPPORTED_FEATURE


@pytest.mark.parametrize("tf", [1, 2])
def test_slot_mode_layouts_in_the_first_and_the_last_wave(hip, side, tf):
    """A: 1024 x 512 x 64 -- 1024 spans, the threshold of the four-span route exactly; 64 waves per image"""
    dev = _Dev(hip, *A_SHAPE, tf, False)
    route = dev.route()
    _assert_slot_route(route, 64, 64)
    case = K.build(route, *A_SHAPE, _slot_placement(route, 64, 64), tf=tf, seed=11 + tf, boundary_every=5)
    snap = _run(dev, case, route)
    assert list(snap[:, route["sweep_word"]]) == [0, 0, 1, 1] + [0] * 60
    sc = route["slot_counts"]
    assert snap[0, sc] == 1 << 8 and snap[0, sc + 63] == 1 << 8 and snap[1, sc] == 15 | 4 << 8 and snap[2, sc + 63] == 0
    assert (snap[4:63, sc:sc + 64] == 0).all()          # the clean control images


def test_slot_mode_partial_last_wave(hip, side):
    """B: 1040 x 504 x 64 -- 16 380 pairs: the last tile of wave 63 has 60 lanes; layouts that end in lane 59 of it"""
    dev = _Dev(hip, *B_SHAPE, 1, False)
    route = dev.route()
    _assert_slot_route(route, 64, 64)
    assert (B_SHAPE[0] // 8) * (B_SHAPE[1] // 4) == 64 * 256 - 4
    case = K.build(route, *B_SHAPE, _slot_placement(route, 64, 64, last=59), seed=21)
    assert case.designed[0].reshape(-1)[-2:].any()      # the image's last pair is a designed one
    _run(dev, case, route)


def _every_wave(route, img, waves, k):
    return {_wave_key(route, img, w): [(j % route["spans"], (w + 9 * j) % 64, 1 + (w + j) % 3) for j in range(k)] for w in range(waves)}


def _c_placement(route):
    pl = _every_wave(route, 0, 1024, 8)                  # 8192 entries: the resolve kernel's loop runs twice
    pl.update(_every_wave(route, 1, 1024, 1))
    full = K.wave_layouts(route)
    pl[_wave_key(route, 2, 0)] = full["plain_full"][0]
    pl[_wave_key(route, 2, 1023)] = full["plain_full"][0]
    pl[_wave_key(route, 3, 1023)] = full["plain_plus_one"][0]
    return pl


def test_slot_mode_at_1024_waves_and_past_4096_entries(hip, side):
    """C: 4096 x 2048 x 4 -- 262 144 pairs = 1024 waves, the slot limit exactly; 8 pairs in every wave of image 0"""
    dev = _Dev(hip, *C_SHAPE, 1, False)
    route = dev.route()
    _assert_slot_route(route, 4, 1024)
    assert route["slots"] == route["slot_waves"] and 8 * 1024 > route["resolve_slices"] * 256
    case = K.build(route, *C_SHAPE, _c_placement(route), seed=31, boundary_every=97)
    snap = _run(dev, case, route)
    sc = route["slot_counts"]
    assert (snap[0, sc:sc + 1024] == (4 | 4 << 8)).all() and snap[3, sc + 1023] == 0 and list(snap[:, route["sweep_word"]]) == [0, 0, 0, 1]


def _d_placement(route, second=False):
    """list 5 (blocks 5, 69, 133, 197): image 0 252 pairs, image 1 253, image 2 245 in one wave and three waves of 5, image 3 251;
    the other lists 0 or 1 entry (the image's last block, 256, among them)"""
    def pairs(k, start=0):   # k distinct (tile, lane) of one wave, whole tiles first
        return [((start + j) // 64, (start + j) % 64, 1 + j % 3) for j in range(k)]
    pl = {}
    if second:
        pl[(0, 5, 0)] = pairs(3)
        pl[(1, 64, 1)] = pairs(1)
        pl[(3, 256, 3)] = pairs(2, 250)
        return pl
    for img, total in ((0, 252), (1, 253), (3, 251)):
        left = total
        for blk in (5, 69, 133, 197):
            for wave in range(4):
                k = min(left, 16)
                if blk == 197 and wave == 3:
                    k = left
                if k:
                    pl[(img, blk, wave)] = pairs(k, 7 * wave)
                left -= k
        assert left == 0
    pl[(2, 69, 2)] = pairs(245)
    for blk in (5, 133, 197):
        pl[(2, blk, 1)] = pairs(5, 100)
    pl[(0, 256, 3)] = pairs(1, 255)      # the image's last pair
    pl[(0, 7, 0)] = pairs(1)
    pl[(3, 63, 2)] = pairs(1, 64)
    pl[(3, 128, 0)] = pairs(1)           # list 0
    return pl


def test_list_mode_at_the_cap(hip, side):
    """D: 4096 x 2056 x 4 -- 1028 waves: past the slots, 64 lists of 252 per image.  252 in a list: resolved entry by entry; 253:
    swept; a wave that straddles the cap: swept, nothing written outside the image.  A second launch shows only its own counts."""
    dev = _Dev(hip, *D_SHAPE, 1, False)
    route = dev.route()
    assert (route["resolve"], route["spans"], route["slots"], route["images"]) == (1, 4, 0, 4), route
    case = K.build(route, *D_SHAPE, _d_placement(route), seed=41, boundary_every=89)
    hdr, swept = case.header(route)
    lc = route["list_counts"]
    assert list(hdr[:, lc + 5]) == [252, 253, 260, 251] and list(swept) == [False, True, True, False]
    assert (np.delete(hdr[:, lc:lc + 64], 5, axis=1) <= 1).all()
    _run(dev, case, route)
    again = K.build(route, *D_SHAPE, _d_placement(route, second=True), seed=42)
    snap = _run(dev, again, route)
    assert list(snap[:, lc + 5]) == [3, 0, 0, 0] and snap[:, lc:lc + 64].sum() == 6


def test_slots_after_more_waves_and_after_lists_on_one_stream(hip, side):
    """C with entries in every wave of every image, then A: the count words of waves 64 .. 1023 are C's and must be ignored (no
    launch clears them); then D, whose lists lie where the slots do, then A again"""
    dev_c, dev_a, dev_d = _Dev(hip, *C_SHAPE, 1, False), _Dev(hip, *A_SHAPE, 1, False), _Dev(hip, *D_SHAPE, 1, False)
    rc, ra, rd = dev_c.route(), dev_a.route(), dev_d.route()
    _assert_slot_route(rc, 4, 1024)
    _assert_slot_route(ra, 64, 64)
    assert rd["resolve"] == 1 and rd["slots"] == 0
    pl = {}
    for img in range(4):
        pl.update(_every_wave(rc, img, 1024, 5 + img))
    snap = _run(dev_c, K.build(rc, *C_SHAPE, pl, seed=51), rc)
    case_a = K.build(ra, *A_SHAPE, _slot_placement(ra, 64, 64), seed=52)
    snap = _run(dev_a, case_a, ra)
    sc = ra["slot_counts"]
    assert (snap[:4, sc + 64:sc + 1024] != 0).all()      # the stale words were there when the resolve kernel ran
    _run(dev_d, K.build(rd, *D_SHAPE, _d_placement(rd), seed=53), rd)
    _run(dev_a, case_a, ra)


def _stats_placement(route, n, waves, heavy_img):
    """at most 6 pairs in doubt per wave, and one image with a wave of 40"""
    pl = {}
    for img in range(n):
        for j, w in enumerate((0, 1, waves // 2, waves - 1)):
            k = 1 + (img + 2 * j) % 6
            pl[_wave_key(route, img, w)] = [(0, (11 * i + w) % 64, 1 + i % 3) for i in range(k)]
    if heavy_img is not None:
        pl[_wave_key(route, heavy_img, 7)] = [(0, l, 1 + l % 3) for l in range(40)]
    return pl


def test_statistics_route_with_slots(hip, orc, side):
    """E: 1024 x 512 x 8 with content_minmax -- 128 spans, the threshold of the pair with statistics; one span per block, 256 waves"""
    dev = _Dev(hip, *E_SHAPE, 1, True)
    route = dev.route()
    assert (route["resolve"], route["spans"], route["slots"], route["spread"], route["images"]) == (1, 1, 256, 0, 8), route
    case = K.build(route, *E_SHAPE, _stats_placement(route, 8, 256, 5), seed=61, boundary_every=7)
    for _ in range(2):
        snap = _run(dev, case, route, orc)
        assert list(snap[:, route["sweep_word"]]) == [0, 0, 0, 0, 0, 1, 0, 0]


def test_statistics_route_with_lists_and_spread(hip, orc, side):
    """F: 3840 x 2160 x 1 with content_minmax -- one span per block, 1013 blocks: lists, estimates published per list.  Sparse, then
    with a list past its cap (seven waves of 40 in blocks of list 9), then sparse again"""
    dev = _Dev(hip, *F_SHAPE, 1, True)
    route = dev.route()
    assert (route["resolve"], route["spans"], route["slots"], route["spread"], route["images"]) == (1, 1, 0, 1, 1), route
    sparse = K.build(route, *F_SHAPE, _stats_placement(route, 1, 4050, None), seed=71, boundary_every=3)
    pl = _stats_placement(route, 1, 4050, None)
    for j in range(7):
        pl[(0, 9 + 64 * j, j % 4)] = [(0, l, 1 + l % 3) for l in range(40)]
    heavy = K.build(route, *F_SHAPE, pl, seed=72)
    assert list(heavy.header(route)[1]) == [True] and list(sparse.header(route)[1]) == [False]
    for case in (sparse, heavy, sparse):
        _run(dev, case, route, orc)
