"""Frames for the tests of the hand-over between generate's filtered kernel and k_generate_resolve (tests/test_gpu_generate_lists.py,
tests/test_generate_lists_cpu.py): the set of pixels the filter leaves in doubt is known BY CONSTRUCTION, pixel by pixel.

Every 4x4 block of both images is uniform grey (U = V = 128, P010 chroma 512 << 6), so a map pixel depends on one (y, p) pair: the
SDR luma byte y and the 10-bit HDR luma code p of its block.  Three kinds of pair:

  in doubt     y = 0.  The SDR luminance is exactly 0, the gain is defined as 1.0 on both paths, and with the metadata generate
               fills in (minContentBoost = 1) the estimate's code value is exactly 0.0: not below flt_lo, not above flt_hi, not
               flt_delta away from an integer -- in doubt whatever the transfer function.  Its exact gain 1.0 is also the smallest
               gain of the image (the background stays above 1.02), its byte is the byte of the minimum, 0.
  boundary     pairs whose code value before truncation, restated in float64, lies within 0.1 x flt_delta of an integer (the
               estimate is within 0.8 x flt_delta of the exact value by the budget flt_delta is made of): in
               doubt as well, with gains all over the range.  A handful exist per transfer function.
  background   random pairs whose gain lies strictly inside (1.02, 0.98 x maxContentBoost) and whose code value keeps at least
               3 x flt_delta from every integer: surely NOT in doubt.

No pair in use has the oracle byte POISON, the byte the tests fill the maps with between the two kernels: a map byte that is not
POISON afterwards has been written.  The expected bytes come from the oracle: pair_table() is oracle.generate over one image that
holds every (y, p) pair once; tests/test_generate_lists_cpu.py checks the look-up against oracle.generate on whole frames.

A case is a placement {(image, block, wave): [(tile, lane, flags)]} -- thread `wave * 64 + lane` of block `block` of the filtered
kernel in its span `tile`; flags 1, 2, 3: the first, the second or both pixels of the thread's pair are in doubt.  The layout
constants (threads per block, spans per block, the slot and list limits) are read from uhdr_hip_generate_probe's route report."""
import functools

import numpy as np

POISON = 0xA5
GAMUT = 0            # BT.709 for both images: no gamut matrix between the pair and its gain
P_LO, P_HI = 64, 940  # the legal 10-bit luma codes
K_LOG2E = 1.4426950408889634
# the words of uhdr_hip_generate_probe's route report (UHDR_HIP_GENERATE_ROUTE_*), as the keys of the `route` dictionaries here
ROUTE_KEYS = ("resolve", "spans", "slots", "spread", "images", "block", "hdr_words", "slot_counts", "slot_plain", "slot_saved", "lists",
              "list_cap", "list_counts", "sweep_word", "resolve_slices", "slot_waves")


def frames_of(yb, pb):
    """block values (mh, mw) -> (yuv uint8[w*h*3/2], p010 uint16[w*h*3/2]) of the 4mw x 4mh image pair"""
    mh, mw = yb.shape
    w, h = 4 * mw, 4 * mh
    yuv = np.full(w * h * 3 // 2, 128, np.uint8)
    yuv[:w * h] = np.repeat(np.repeat(yb.astype(np.uint8), 4, 0), 4, 1).reshape(-1)
    p010 = np.full(w * h * 3 // 2, 512 << 6, np.uint16)
    p010[:w * h] = np.repeat(np.repeat(pb.astype(np.uint16) << 6, 4, 0), 4, 1).reshape(-1)
    return yuv, p010


@functools.lru_cache(None)
def pair_table(tf):
    """oracle byte of every grey pair: [y, p - P_LO], from ONE oracle.generate call over a 3508 x 1024 image"""
    from oracle import oracle as O
    O.load()
    yb = np.repeat(np.arange(256, dtype=np.uint8)[:, None], P_HI - P_LO + 1, 1)
    pb = np.repeat(np.arange(P_LO, P_HI + 1, dtype=np.uint16)[None, :], 256, 0)
    yuv, p010 = frames_of(yb, pb)
    w, h = 4 * yb.shape[1], 4 * yb.shape[0]
    st, m, _ = O.generate("orc_", O.yuv420_image(yuv, w, h, GAMUT), O.p010_image(p010, w, h, GAMUT), tf, False, threads=8)
    assert st == 0
    return m.copy()


def filter_consts(tf):
    """(maxContentBoost, code values per log2 unit, flt_delta) as generate_consts derives them (uhdr_capi.hip)"""
    max_boost = np.float32(10000.0 if tf == 2 else 1000.0) / np.float32(203.0)
    log2_max = np.float32(np.log2(np.float64(max_boost)))
    scale = 255.0 / float(log2_max)          # minContentBoost = 1: log2_min = 0
    k_rel = 1.0e-5 if tf == 2 else 4.0e-6
    delta = float(np.float32(1.25 * (scale * (k_rel * K_LOG2E + 5.0e-7) + 4.0e-5)))
    return float(max_boost), scale, delta


@functools.lru_cache(None)
def pair_codes(tf):
    """(gain, code value before truncation) of every grey pair in float64, [y, p - P_LO]; y = 0: gain 1, code value 0.
    Grey: R = G = B = the luma, and the luminance weights cancel in the gain."""
    from oracle import oracle as O
    sy = np.minimum(np.arange(256, dtype=np.float64) / 255.0, 1.0).astype(np.float32)
    hy = np.minimum((np.arange(P_LO, P_HI + 1, dtype=np.float64) - 64.0) / 876.0, 1.0).astype(np.float32)
    s_lin = O.eval_transfer(0, sy).astype(np.float64) * 203.0
    h_lin = (hy if tf == 0 else O.eval_transfer(tf, hy)).astype(np.float64) * (10000.0 if tf == 2 else 1000.0)
    max_boost, scale, _ = filter_consts(tf)
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = np.where(s_lin[:, None] > 0.0, h_lin[None, :] / s_lin[:, None], 1.0)
        code = np.log2(np.clip(gain, 1.0, max_boost)) * scale
    return gain, code


@functools.lru_cache(None)
def pools(tf):
    """((y, p) of the background pairs, (y, p) of the boundary pairs), both without POISON bytes"""
    gain, code = pair_codes(tf)
    max_boost, _, delta = filter_consts(tf)
    table = pair_table(tf)
    dist = np.abs(code - np.rint(code))
    inside = (gain > 1.02) & (gain < 0.98 * max_boost) & (table != POISON)
    inside[0, :] = False
    bg = inside & (dist >= 3.0 * delta)
    bd = inside & (dist <= 0.1 * delta)
    # the float64 restatement and the oracle agree on every pair that keeps away from the integers
    assert np.array_equal(np.floor(code[bg]).astype(np.uint8), table[bg])
    by, bp = np.nonzero(bg)
    dy, dp = np.nonzero(bd)
    return (by.astype(np.uint8), (bp + P_LO).astype(np.uint16)), (dy.astype(np.uint8), (dp + P_LO).astype(np.uint16))


def pair_index(route, block, wave, tile, lane):
    """the pixel pair thread (wave, lane) of block `block` takes in its span `tile`"""
    assert 0 <= lane < 64 and 0 <= wave < route["block"] // 64 and 0 <= tile < route["spans"]
    return (block * route["spans"] + tile) * route["block"] + wave * 64 + lane


class Case:
    """yuv (n, w*h*3/2) uint8, p010 (n, w*h*3/2) uint16; expect (n, mh, mw): the oracle's bytes; designed (n, mh, mw) bool: the
    pixels in doubt; pairs {(image, block, wave): pairs in doubt}"""

    def __init__(self, w, h, n, tf):
        self.w, self.h, self.n, self.tf = w, h, n, tf
        self.mw, self.mh = w // 4, h // 4

    def header(self, route):
        """(the header words [0, limit) every image must show after the filtered kernel of a launch WITHOUT statistics, which images
        are swept).  Slot mode: the waves' count words, plain | saved << 8, 0 and the sweep word for a wave with more than `plain`
        plain entries; list mode: the lists' counts (a block appends to list block % lists), swept above `cap`."""
        slots, saved_max, plain_max = route["slots"], route["slot_saved"], route["slot_plain"]
        limit = route["slot_counts"] + slots
        hdr = np.zeros((self.n, limit), np.uint32)
        for (img, blk, wave), k in self.pairs.items():
            if slots:
                saved = min(k, saved_max)
                plain = k - saved
                over = plain > plain_max
                hdr[img, route["slot_counts"] + blk * (route["block"] // 64) + wave] = 0 if over else plain | saved << 8
                if over:
                    hdr[img, route["sweep_word"]] = 1
            else:
                hdr[img, route["list_counts"] + blk % route["lists"]] += k
        if slots:
            swept = hdr[:, route["sweep_word"]] != 0
        else:
            swept = (hdr[:, route["list_counts"]:route["list_counts"] + route["lists"]] > route["list_cap"]).any(axis=1)
        return hdr, swept


def build(route, w, h, n, placement, tf=1, seed=1, boundary_every=0):
    """the frames of one case; every boundary_every-th designed pixel is a boundary pair instead of y = 0"""
    assert w % 8 == 0 and h % 4 == 0
    c = Case(w, h, n, tf)
    mw, mh = c.mw, c.mh
    ppr = mw // 2
    (by, bp), (dy, dp) = pools(tf)
    assert by.size > 1000 and (boundary_every == 0 or dy.size > 0)
    table = pair_table(tf)
    rng = np.random.RandomState(seed)
    pick = rng.randint(0, by.size, (n, mh, mw))
    yb, pb = by[pick], bp[pick]
    c.designed = np.zeros((n, mh, mw), bool)
    c.pairs = {}
    count = 0
    for (img, blk, wave), entries in sorted(placement.items()):
        assert 0 <= img < n and len({(t, l) for t, l, _ in entries}) == len(entries)
        c.pairs[(img, blk, wave)] = len(entries)
        for tile, lane, flags in entries:
            idx = pair_index(route, blk, wave, tile, lane)
            assert idx < ppr * mh and flags in (1, 2, 3), (idx, flags)
            my, pr = divmod(idx, ppr)
            for k in range(2):
                if flags >> k & 1:
                    count += 1
                    if boundary_every and count % boundary_every == 0:
                        j = (count // boundary_every) % dy.size
                        yb[img, my, 2 * pr + k], pb[img, my, 2 * pr + k] = dy[j], dp[j]
                    else:
                        yb[img, my, 2 * pr + k] = 0
                    c.designed[img, my, 2 * pr + k] = True
    c.yb, c.pb = yb, pb
    c.expect = table[yb, pb.astype(np.int64) - P_LO]
    assert not (c.expect == POISON).any()          # a byte that is still POISON after the resolve kernel was not written
    assert (yb[~c.designed] != 0).all()
    c.yuv = np.empty((n, w * h * 3 // 2), np.uint8)
    c.p010 = np.empty((n, w * h * 3 // 2), np.uint16)
    for i in range(n):
        c.yuv[i], c.p010[i] = frames_of(yb[i], pb[i])
    return c


# ---- the layouts of one wave (slot mode): name -> (entries, count word, sweeps).  last: the highest lane of the wave's last tile
def wave_layouts(route, last=63):
    t_last = route["spans"] - 1
    saved, plain = route["slot_saved"], route["slot_plain"]

    def spread(k):   # k pairs over the wave's tiles, distinct (tile, lane)
        return [(j % (t_last + 1), (7 * j + 3) % (last + 1), 1 + j % 3) for j in range(k)]

    def word(k):
        return (k - min(k, saved)) | min(k, saved) << 8

    lay = {
        "first_lane": ([(0, 0, 1)], word(1), False),
        "last_lane": ([(t_last, last, 1)], word(1), False),
        "flags_2_and_3": ([(0, 7, 2), (t_last, 33, 3)], word(2), False),
        "saved_full": (spread(saved), word(saved), False),                       # 4 pairs: 0 | 4 << 8
        "saved_plus_one": (spread(saved + 1), word(saved + 1), False),           # 5 pairs: 1 | 4 << 8
        "plain_full": (spread(saved + plain), word(saved + plain), False),       # 19 pairs: 15 | 4 << 8
        "plain_plus_one": (spread(saved + plain + 1), 0, True),                  # 20 pairs: count 0, sweep
        "whole_tile": ([(0, l, 3) for l in range(64 if t_last else last + 1)], 0, True),
    }
    if t_last >= 2:   # three pairs in tile 0, three in tile 2: the last saved entry is the lowest lane of tile 2
        lay["saved_across_tiles"] = ([(0, 9, 1), (0, 20, 3), (0, 41, 2), (2, 2, 1), (2, 30, 1), (2, 50, 3)], word(6), False)
    return lay
