"""-m gpu: the bookkeeping between EXACT apply's f32 estimate (k_apply_s4_est, k_apply_px_est) and k_apply_resolve at its limits.

The estimate kernels write every pixel and append those whose code their estimate cannot settle to 1024 lists per image, ex_cap
entries each; k_apply_resolve finds each entry's list by binary search over the lists' prefix sums, recomputes the listed pixels on
the f64 path, sweeps the whole image where a list is longer than ex_cap, and clears the header.  A pixel in doubt nearly always
holds the right code already, so comparing final bytes says little about an entry that is dropped, misplaced or duplicated.  These
tests run the two kernels one at a time (uhdr_hip_apply_exact_probe) on frames whose pixels in doubt are a known mask
(tests/apply_doubt_cases.py).  Every case, in every format it runs in:
  (1) after the estimate kernel the header's count words EQUAL the counts the mask predicts -- this also holds the construction of
      the frames to account -- the slice word is 0, and every pixel outside the mask already holds the oracle's value;
  (2) the destinations are filled with a byte pattern no pixel has, then k_apply_resolve runs: without a sweep exactly the mask's
      pixels hold the oracle's value and all others the pattern; a swept image holds the oracle's value everywhere, and its
      neighbours in the batch are touched in their own lists only; the guard bytes behind every destination are intact;
  (3) the headers it left, read through the estimate kernel on an all-black frame of the same size, are zero;
  (4) the production call on the same frames equals the oracle and APPLY_EXACT_UNFILTERED byte for byte, twice on the stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import apply_doubt_cases as K

pytestmark = pytest.mark.gpu

GUARD = 256
# formats 1 and 3 go through every case; 2 and 4 through the capacity cases, the batch and a per-pixel case
RUNS = [(name, fmt) for name in K.ALL for fmt in K.FORMATS if fmt in (1, 3) or name in K.CAPACITY + ("mixed_batch", "px_shared")]


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
    """a case's descriptors: the frames and an all-black twin, one map, the destinations side by side with GUARD bytes behind each"""

    def __init__(self, hip, case, fmt, share=None):
        """share: a _Dev of the same geometry and format whose map and destinations this one takes (other frames, same call)"""
        self.hip, self.lib, self.c, self.fmt = hip, hip.load(), case, fmt
        n, w, h = case.n, case.w, case.h
        fb = w * h * 3 // 2
        self.out_bytes = w * h * K.BPP[fmt]
        self.stride = (self.out_bytes + GUARD + 255) // 256 * 256
        yuv, gmap = case.frames(fmt)
        self.yuv = torch.from_numpy(yuv).cuda()
        black = np.full(fb, 128, np.uint8)
        black[:w * h] = K.levels(fmt)[1]
        self.black = torch.from_numpy(black).cuda()
        if share is not None:
            assert (share.c.w, share.c.h, share.c.scale, share.c.n, share.fmt) == (w, h, case.scale, n, fmt)
        self.map = torch.from_numpy(gmap.copy()).cuda() if share is None else share.map
        self.out = torch.empty((n, self.stride), dtype=torch.uint8, device="cuda") if share is None else share.out
        self.ya = hip.image_array([hip.yuv420_image(self.yuv.data_ptr() + i * fb, w, h, hip.CG_BT709) for i in range(n)])
        self.ba = hip.image_array([hip.yuv420_image(self.black.data_ptr(), w, h, hip.CG_BT709) for _ in range(n)])
        self.ma = hip.image_array([hip.mono_image(self.map.data_ptr(), case.mw, case.mh) for _ in range(n)])
        self.da = hip.image_array([hip.out_image(self.out.data_ptr() + i * self.stride) for i in range(n)])
        self.md = hip.metadata(K.MAX_BOOST)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def probe(self, phase, route=None, headers=None, black=False, n=None, fmt=None):
        return self.lib.uhdr_hip_apply_exact_probe(phase, self.c.n if n is None else n, self.ba if black else self.ya, self.ma, C.byref(self.md),
                                                   self.fmt if fmt is None else fmt, K.FLT_MAX, self.da, self.stream(), route,
                                                   None if headers is None else C.c_void_p(headers.data_ptr()))

    def route(self):
        r = (C.c_uint32 * self.hip.APPLY_ROUTE_WORDS)()
        assert self.probe(0, route=r) == 0
        return dict(zip(K.ROUTE_KEYS, list(r)))

    def production(self, mode):
        self.out.fill_(0xEE)
        assert self.lib.uhdr_hip_apply_gainmap_batch(self.c.n, self.ya, self.ma, C.byref(self.md), self.fmt, K.FLT_MAX, self.da, mode, self.stream()) == 0
        return self.host(self.out, 0xEE)

    def host(self, t, guard):
        """a copy of the destinations as pixels, (n, h, w, k); the guard bytes must hold `guard`"""
        torch.cuda.current_stream().synchronize()
        a = t.cpu().numpy()
        assert (a[:, self.out_bytes:] == guard).all(), "bytes behind a destination were written"
        return np.stack([K.pixels_of(a[i, :self.out_bytes], self.fmt, self.c.w, self.c.h) for i in range(self.c.n)])


def _run(hip, name, fmt):
    """steps (1) to (4) of one case in one format, on the current stream"""
    case = K.case(name)
    dev = _Dev(hip, case, fmt)
    route = dev.route()
    assert route == case.route(), route
    expect = K.expect(name, fmt)
    poison = K.poison_pixel(fmt)
    n, hw, lc, lists = case.n, route["hdr_words"], route["list_counts"], route["lists"]
    want_hdr = np.zeros((n, hw), np.uint32)
    want_hdr[:, lc:lc + lists] = case.counts(route)
    swept = [f["sweep"] for f in case.facts(route)]

    dev.out.fill_(0x11)
    snap_d = torch.full((n, hw), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    assert dev.probe(1, headers=snap_d) == 0
    est_d = dev.out.clone()
    dev.out.fill_(K.POISON)
    assert dev.probe(2) == 0
    res_d = dev.out.clone()
    after_d = torch.full((n, hw), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    assert dev.probe(1, headers=after_d, black=True) == 0     # (3): nothing of a black frame is in doubt, the counts are what was left
    assert dev.probe(2, black=True) == 0
    snap, after = snap_d.cpu().numpy().view(np.uint32), after_d.cpu().numpy().view(np.uint32)
    est, res = dev.host(est_d, 0x11), dev.host(res_d, K.POISON)

    counts = snap[:, lc:lc + lists]
    print("\n%s fmt %d: %dx%d scale %d x %d images, ex_cap %d; in doubt by design %s, counted %s, longest list %s, slice words %s, swept %s; "
          "pixels written by k_apply_resolve %s; header words left behind %d"
          % (name, fmt, case.w, case.h, case.scale, n, route["list_cap"], case.masks.sum(axis=(1, 2)).tolist(), counts.sum(axis=1).tolist(),
             counts.max(axis=1).tolist(), snap[:, route["slice_word"]].tolist(), swept, (~(res == poison).all(axis=-1)).sum(axis=(1, 2)).tolist(),
             int((after != 0).sum())))
    # (1)
    bad = np.argwhere(snap != want_hdr)
    assert bad.size == 0, [(int(i), int(j), int(snap[i, j]), int(want_hdr[i, j])) for i, j in bad[:8]]
    settled = ~case.masks
    assert np.array_equal(est[settled], expect[settled]), "a pixel the estimate did not list differs from the oracle"
    # (2)
    written = ~(res == poison).all(axis=-1)
    for i in range(n):
        want_written = np.ones_like(case.masks[i]) if swept[i] else case.masks[i]
        assert np.array_equal(written[i], want_written), ("image %d: written outside the lists %d, listed but not written %d, swept %s"
                                                          % (i, (written[i] & ~want_written).sum(), (~written[i] & want_written).sum(), swept[i]))
    assert np.array_equal(res[written], expect[written])
    # (3)
    assert not after.any(), [(int(i), int(j), int(after[i, j])) for i, j in np.argwhere(after != 0)[:8]]
    # (4)
    exact = dev.production(hip.APPLY_EXACT)
    assert np.array_equal(exact, expect)
    assert np.array_equal(dev.production(hip.APPLY_EXACT_UNFILTERED), expect)
    assert np.array_equal(dev.production(hip.APPLY_EXACT), expect)


@pytest.mark.parametrize("name,fmt", RUNS)
def test_lists_and_resolve(hip, orc, side, name, fmt):
    _run(hip, name, fmt)


@pytest.mark.parametrize("kind,fmt", [("s4", 1), ("s4", 3), ("px", 1), ("px", 2), ("px", 3), ("px", 4)])
def test_entry_at_ex_cap_is_dropped_and_the_next_image_keeps_its_first_entry(hip, orc, side, kind, fmt):
    """The upper side of `pos < ex_cap` in both estimate kernels.  Entry ex_cap of a list would be slot 0 of the next list -- for
    list 1023 of an image, of list 0 of the NEXT image in the chunk, which is not swept and would lose its own first entry (behind
    the last image: words past the workspace).  Within one launch the two writes race; across two estimate launches on one
    workspace they do not: the first fills image 0's list 1023 to exactly ex_cap and puts pixel p into image 1's list 0, the second
    appends one more pixel q to image 0's list 1023 -- counts ex_cap + 1 and 1, by equality.  k_apply_resolve then sweeps image 0 and
    writes, in image 1, p and nothing else."""
    a, b, u = (K.case("acc_%s_%s" % (kind, part)) for part in "abu")
    dev_u = _Dev(hip, u, fmt)
    dev_a, dev_b = _Dev(hip, a, fmt, share=dev_u), _Dev(hip, b, fmt, share=dev_u)
    route = dev_u.route()
    assert route == u.route() == dev_a.route() == dev_b.route()
    expect, poison = K.expect(u.name, fmt), K.poison_pixel(fmt)
    hw, lc, lists, cap = route["hdr_words"], route["list_counts"], route["lists"], route["list_cap"]
    snaps = [torch.full((2, hw), 0x7FFFFFFF, dtype=torch.int32, device="cuda") for _ in range(3)]
    dev_u.out.fill_(0x11)
    assert dev_a.probe(1, headers=snaps[0]) == 0
    assert dev_b.probe(1, headers=snaps[1]) == 0
    dev_u.out.fill_(K.POISON)
    assert dev_u.probe(2) == 0
    res_d = dev_u.out.clone()
    assert dev_u.probe(1, headers=snaps[2], black=True) == 0
    assert dev_u.probe(2, black=True) == 0
    first, both, after = (s.cpu().numpy().view(np.uint32) for s in snaps)
    res = dev_u.host(res_d, K.POISON)
    want = np.zeros((2, hw), np.uint32)
    want[:, lc:lc + lists] = a.counts(route)
    assert np.array_equal(first, want) and first[0, lc + 1023] == cap and first[1, lc] == 1
    want[:, lc:lc + lists] = u.counts(route)
    assert np.array_equal(both, want) and both[0, lc + 1023] == cap + 1 and both[1, lc] == 1
    written = ~(res == poison).all(axis=-1)
    print("\nacc_%s fmt %d: ex_cap %d; image 0 list 1023: %d then %d; image 1 list 0: %d then %d; written: image 0 %d of %d, image 1 %d (p %s)"
          % (kind, fmt, cap, first[0, lc + 1023], both[0, lc + 1023], first[1, lc], both[1, lc], written[0].sum(), written[0].size, written[1].sum(),
             bool(written[1][a.masks[1]].all())))
    assert written[0].all(), "image 0 has a list longer than ex_cap: swept"
    assert np.array_equal(written[1], a.masks[1]), ("image 1: written outside its list %d, its entry not written %d"
                                                    % ((written[1] & ~a.masks[1]).sum(), (~written[1] & a.masks[1]).sum()))
    assert np.array_equal(res[written], expect[written])
    assert not after.any()
    assert np.array_equal(dev_u.production(hip.APPLY_EXACT), expect)


@pytest.mark.parametrize("fmt", [1, 3])
def test_sizes_in_turn_on_one_stream(hip, orc, side, fmt):
    """small, large, small again without uhdr_hip_stream_release in between: ex_cap goes 65, 96, 65 (the lists move, the headers in
    front of them do not), and every launch finds the headers cleared by the launch before it, whatever ex_cap that one had"""
    for name in ("at_cap", "reuse_large", "cap_plus_one", "second_trip", "last_only"):
        _run(hip, name, fmt)


def test_single_phases_refused_where_the_call_is_not_one_pair(hip, side):
    case = K.case("mixed_batch")
    dev = _Dev(hip, case, 3)
    hdr = torch.zeros((case.n, 1032), dtype=torch.int32, device="cuda")
    dev.out.fill_(0x11)
    for phase in (1, 2):
        assert dev.probe(phase, headers=hdr, fmt=hip.OUTPUT_SDR) == hip.ERROR_UNSUPPORTED_FEATURE     # no output, no pair
    # two chunks: the second image's map is another size
    dev.ma[1] = hip.mono_image(dev.map.data_ptr(), case.mw // 2, case.mh // 2)
    r = (C.c_uint32 * hip.APPLY_ROUTE_WORDS)()
    assert dev.probe(0, route=r) == 0 and r[hip.APPLY_ROUTE_IMAGES] == 1
    for phase in (1, 2):
        assert dev.probe(phase, headers=hdr) == hip.ERROR_UNSUPPORTED_FEATURE
    assert dev.probe(1, headers=None) == hip.ERROR_BAD_PTR
    torch.cuda.current_stream().synchronize()
    assert (dev.out.cpu().numpy() == 0x11).all() and not hdr.cpu().numpy().any()                      # nothing was enqueued
