"""Frames for the tests of the hand-over between EXACT apply's f32 estimate (k_apply_s4_est, k_apply_px_est) and k_apply_resolve
(tests/test_gpu_apply_doubt_lists.py, tests/test_apply_doubt_cpu.py): the set of pixels the estimate leaves in doubt is known BY
CONSTRUCTION -- it is a boolean mask.

Every frame is a two-level grey image (U = V = 128: the pixel is its luma) under a uniform gain map, metadata min 1 / max 4 and
display boost FLT_MAX (so the display boost is the content boost, 4).  The unset level is Y = 0 in every format: linear 0, value 0,
and max(v, 1/2) puts its fraction at 1/2 (F16: lin == 0 is no subnormal) -- never in doubt.  The set level:

  formats 2, 3, 4   Y = 255 under map byte 255: factor 4 / display 4, linear 1.0, the code value 1023.0 to within the estimate's
                    error -- an integer, in doubt (tests/test_gpu_exact_filter.py's overflow frame is this level)
  format 1 (F16)    Y = 1 under map byte 0: factor exactly 1, lin = (1 / 255 / 12.92) / 4 ~ 7.6e-5: not 0 and below 2^-13, the range
                    est_channel<1> always hands to the exact path (the hardware conversion does not round half-precision
                    subnormals as the reference does)

Phase 1 of uhdr_hip_apply_exact_probe holds this to account on the GPU: the list counts it leaves must EQUAL counts().

A case is a mask per image and its FACTS -- the longest list against ex_cap, the entries against the 65 536 a trip of
k_apply_resolve's loop covers, the lists in use and those that several blocks share -- computed by facts() from the mask and the
route constants; tests/test_apply_doubt_cpu.py asserts them with the constants restated, so that a case cannot drift into testing
nothing.  The list a pixel in doubt goes to:
  scale-4 route     block b = cells [256 b, 256 b + 256) of the map in row-major order; list b % lists
  per-pixel route   the append of (row y, block bx = x / 256) goes to list (y * grid_x + bx) % lists

The "acc_" cases come in threes (a, b, u): two estimate launches on one workspace, whose counts add up, then k_apply_resolve on their
union -- the one way to decide, without a race, which of two appends reaches a slot first (see case())."""
import functools

import numpy as np

POISON = 0xCD
MAX_BOOST, MIN_BOOST = 4.0, 1.0
FLT_MAX = 3.4028234663852886e38
FORMATS = (1, 2, 3, 4)
BPP = {1: 8, 2: 4, 3: 4, 4: 6}
# the words of uhdr_hip_apply_exact_probe's route report (UHDR_HIP_APPLY_ROUTE_*), as the keys of the `route` dictionaries here
ROUTE_KEYS = ("resolve", "cells", "images", "lists", "list_cap", "hdr_words", "list_counts", "slice_word", "resolve_slices", "grid_x", "grid_y")
TRIP = 65536          # entries one trip of k_apply_resolve's loop covers: kExSlices x 256


def levels(fmt):
    """(luma of a set pixel, luma of an unset pixel, the map's byte)"""
    return (1, 0, 0) if fmt == 1 else (255, 0, 255)


def ex_cap(w, h):
    return w * h // 16384 + 64


def route_of(w, h, scale, n=1):
    """the route a chunk of n such images takes, restated: what phase 0 must report (tests/test_apply_doubt_cpu.py compares)"""
    cells = scale == 4
    gx = (w // 4 * (h // 4) + 255) // 256 if cells else (w + 255) // 256
    gy = n if cells else min(h, 65535)
    return dict(zip(ROUTE_KEYS, (1, int(cells), n, 1024, ex_cap(w, h), 8 + 1024, 8, 3, 256, gx, gy)))


class Case:
    """masks (n, h, w) bool: the pixels in doubt of the n images of one call"""

    def __init__(self, name, w, h, scale, masks):
        masks = np.asarray(masks, bool)
        assert masks.shape[1:] == (h, w) and w % scale == 0 and h % scale == 0 and w % 2 == 0 and h % 2 == 0
        self.name, self.w, self.h, self.scale, self.n, self.masks = name, w, h, scale, masks.shape[0], masks
        self.mw, self.mh = w // scale, h // scale
        self.masks.flags.writeable = False

    def route(self):
        return route_of(self.w, self.h, self.scale, self.n)

    def frames(self, fmt):
        """(yuv (n, w*h*3/2) uint8, map (mh, mw) uint8: the same for every image)"""
        hi, lo, mb = levels(fmt)
        yuv = np.full((self.n, self.w * self.h * 3 // 2), 128, np.uint8)
        yuv[:, :self.w * self.h] = np.where(self.masks, hi, lo).astype(np.uint8).reshape(self.n, -1)
        return yuv, np.full((self.mh, self.mw), mb, np.uint8)

    def appends(self, route):
        """(n, appends) entries of every append of the estimate kernel, in the order of its list rule: append a goes to list
        a % lists"""
        if route["cells"]:
            cells = self.masks.reshape(self.n, self.mh, 4, self.mw, 4).sum(axis=(2, 4)).reshape(self.n, -1)
            pad = route["grid_x"] * 256 - cells.shape[1]
            assert 0 <= pad < 256
            return np.pad(cells, ((0, 0), (0, pad))).reshape(self.n, route["grid_x"], 256).sum(axis=2)
        gx = route["grid_x"]
        assert gx == (self.w + 255) // 256
        padded = np.pad(self.masks, ((0, 0), (0, 0), (0, gx * 256 - self.w)))
        return padded.reshape(self.n, self.h, gx, 256).sum(axis=3).reshape(self.n, self.h * gx)

    def counts(self, route):
        """(n, lists) the count word of every list after the estimate kernel"""
        a = self.appends(route)
        lists = route["lists"]
        out = np.zeros((self.n, lists), np.int64)
        for i in range(self.n):
            out[i] = np.bincount(np.arange(a.shape[1]) % lists, weights=a[i], minlength=lists).astype(np.int64)
        return out

    def facts(self, route):
        """per image: longest list, total entries, lists in use, lists that several non-empty appends share, swept"""
        a, c = self.appends(route), self.counts(route)
        lists = route["lists"]
        out = []
        for i in range(self.n):
            contributors = np.bincount(np.arange(a.shape[1]) % lists, weights=(a[i] > 0), minlength=lists).astype(np.int64)
            out.append(dict(longest=int(c[i].max()), total=int(c[i].sum()), used=int((c[i] > 0).sum()), shared=int((contributors > 1).sum()),
                            appends=int(a.shape[1]), sweep=bool(c[i].max() > route["list_cap"])))
        return out


# ---- what the oracle makes of such frames ------------------------------------------------------------------------------------
def _oracle(yuv, w, h, gmap, fmt):
    from oracle import oracle as O
    O.load()
    md = O.Metadata(MAX_BOOST, MIN_BOOST, 1.0, 0.0, 0.0, MIN_BOOST, MAX_BOOST, 1)
    st, out, _ = O.apply("orc_", O.yuv420_image(yuv, w, h, O.CG_BT709), gmap, md, fmt, FLT_MAX, threads=8)
    assert st == 0
    return out.copy()


def pixels_of(buf, fmt, w, h):
    """an output image as (h, w, k) words that belong to the pixel: F16 four halves, 1010102 one dword, planar 10-bit three uint16"""
    if fmt == 1:
        return buf.view(np.uint16).reshape(h, w, 4)
    if fmt == 4:
        return buf.view(np.uint16).reshape(3, h, w).transpose(1, 2, 0)
    return buf.view(np.uint32).reshape(h, w, 1)


def poison_pixel(fmt):
    return np.full(1 if fmt in (2, 3) else (4 if fmt == 1 else 3), POISON * (0x01010101 if fmt in (2, 3) else 0x0101), np.uint32 if fmt in (2, 3) else np.uint16)


def expect_whole(case, fmt):
    """the oracle on every image of the case: (n, h, w, k)"""
    yuv, gmap = case.frames(fmt)
    return np.stack([pixels_of(_oracle(yuv[i], case.w, case.h, gmap, fmt), fmt, case.w, case.h) for i in range(case.n)])


@functools.lru_cache(None)
def class_table(fmt, scale):
    """[level][y, x]: the oracle's pixel of a uniform frame of one level, 2 x 2 map cells.  Under a uniform map and grey chroma a
    pixel depends on its level, its place in the map cell and on whether the cell is the map's last column / row (sampleMap takes
    other weight tables there): a frame of 2 x 2 cells holds every class"""
    hi, lo, mb = levels(fmt)
    s = scale
    out = []
    for level in (lo, hi):
        yuv = np.full(4 * s * s * 3 // 2, 128, np.uint8)
        yuv[:4 * s * s] = level
        out.append(pixels_of(_oracle(yuv, 2 * s, 2 * s, np.full((2, 2), mb, np.uint8), fmt), fmt, 2 * s, 2 * s))
    return out


def expect_by_class(case, fmt):
    """expect_whole from class_table(): for the frames too large to hand to the oracle in every test"""
    s, w, h = case.scale, case.w, case.h
    lo_t, hi_t = class_table(fmt, s)
    yy = np.arange(h) % s + np.where(np.arange(h) // s == case.mh - 1, s, 0)
    xx = np.arange(w) % s + np.where(np.arange(w) // s == case.mw - 1, s, 0)
    lo_img, hi_img = lo_t[yy][:, xx], hi_t[yy][:, xx]
    return np.where(case.masks[..., None], hi_img[None], lo_img[None])


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _cells_mask(w, h, per_block):
    """scale 4: per_block {block: entries} -> mask; a block's entries fill its cells from its first cell on, 16 pixels per cell,
    the rest of the last cell in pixel order"""
    mw, mh = w // 4, h // 4
    m = np.zeros((h, w), bool)
    for blk, k in per_block.items():
        assert 0 <= k <= 4096
        for j in range((k + 15) // 16):
            cell = blk * 256 + j
            assert cell < mw * mh
            cy, cx = divmod(cell, mw)
            left = min(16, k - 16 * j)
            sub = np.zeros(16, bool)
            sub[:left] = True
            m[4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = sub.reshape(4, 4)
    return m


def _rows_mask(w, h, per_append, from_right=False):
    """per-pixel route: per_append {(y, bx): entries} -> mask; the entries are every third pixel of the block's part of the row
    (from its last pixel downwards: from_right), so that waves and lanes of all kinds hold one"""
    m = np.zeros((h, w), bool)
    for (y, bx), k in per_append.items():
        x0, x1 = bx * 256, min(w, bx * 256 + 256)
        xs = np.arange(x0, x1)
        xs = xs[::-1] if from_right else xs
        pick = np.concatenate([xs[0::3], xs[1::3], xs[2::3]])[:k]
        assert pick.size == k, (y, bx, k)
        m[y, pick] = True
    return m


SMALL = (256, 64)      # scale 4: 64 x 16 cells, 4 blocks, ex_cap 65


def _small(per_block):
    return _cells_mask(*SMALL, per_block)


def _last_only():
    m = np.zeros(SMALL[::-1], bool)
    m[-1, -1] = True
    return m


@functools.lru_cache(None)
def case(name):
    w, h = SMALL
    if name == "at_cap":
        return Case(name, w, h, 4, [_small({0: 65, 2: 1, 3: 64})])
    if name == "cap_plus_one":
        return Case(name, w, h, 4, [_small({0: 66, 2: 1, 3: 64})])
    if name == "empty":
        return Case(name, w, h, 4, [np.zeros((h, w), bool)])
    if name == "last_only":
        return Case(name, w, h, 4, [_last_only()])
    if name == "mixed_batch":   # the sweeping image between two that do not sweep
        return Case(name, w, h, 4, [_small({0: 65, 2: 1, 3: 64}), _small({0: 66, 2: 1, 3: 64}), _last_only(), np.zeros((h, w), bool)])
    if name in ("px_shared", "px_overflow"):
        # 512 x 514, scale 2: grid_x 2, 1028 appends -- the appends of row 512 and 513 share lists 0 .. 3 with those of rows 0 and 1;
        # ex_cap 80.  List 1 = (row 0, block 1) + (row 512, block 1): 50 + 30, or + 31
        w, h = 512, 514
        over = name == "px_overflow"
        pa = {(0, 0): 7, (0, 1): 50, (512, 1): 31 if over else 30, (1, 0): 80, (513, 1): 3, (1, 1): 2, (300, 0): 80, (300, 1): 79, (511, 1): 1}
        return Case(name, w, h, 2, [_rows_mask(w, h, pa)])
    if name == "px_ragged":
        # 330 x 24, scale 3: the second block of a row holds 74 pixels; set pixels from the row's last pixel downwards; ex_cap 64
        w, h = 330, 24
        pa = {(0, 1): 1, (0, 0): 2, (5, 1): 64, (23, 1): 60, (23, 0): 10, (11, 0): 63}
        return Case(name, w, h, 3, [_rows_mask(w, h, pa, from_right=True)])
    if name == "second_trip":
        # 1024 x 512, scale 2: grid_x 4, 2048 appends of 40, two per list: 80 per list under ex_cap 96, 81 920 entries
        w, h = 1024, 512
        return Case(name, w, h, 2, [_rows_mask(w, h, {(y, bx): 40 for y in range(h) for bx in range(4)})])
    if name in ("s4_wrap", "s4_wrap_overflow"):
        # 4096 x 1028, scale 4: 1028 blocks, blocks 1024 .. 1027 (the map's last row: the edge tables) share lists 0 .. 3 with
        # blocks 0 .. 3; ex_cap 321.  List 0 = 200 + 121, or + 122
        w, h = 4096, 1028
        over = name == "s4_wrap_overflow"
        pb = {0: 200, 1024: 122 if over else 121, 1: 10, 1025: 5, 1026: 1, 3: 300, 1027: 21, 515: 321, 1023: 33}
        return Case(name, w, h, 4, [_cells_mask(w, h, pb)])
    if name == "reuse_large":   # between two small cases on one stream: ex_cap 96, a workspace of 1.5 times the lists' words
        w, h = 1024, 512
        return Case(name, w, h, 4, [_cells_mask(w, h, {0: 96, 5: 95, 127: 1, 64: 40})])
    if name.startswith("acc_"):
        # Two estimate launches on one workspace, then one k_apply_resolve: the counts add up, and the second launch's appends go
        # behind the first's.  Two images of at least 1 024 appends; a: image 0's list 1023 at exactly ex_cap, image 1's list 0 one
        # pixel p; b: one more pixel q for image 0's list 1023, nothing for image 1; u: a | b, what k_apply_resolve runs on.  q is
        # entry ex_cap of its list: dropped.  An estimate kernel that kept it would put it where image 1's list 0 begins, over p.
        _, kind, part = name.split("_")
        if kind == "s4":      # 4096 x 1024, scale 4: 1 024 blocks, ex_cap 320; list 1023 is block 1023 alone
            w, h, scale = 4096, 1024, 4
            full, more, first = _cells_mask(w, h, {1023: 320}), _cells_mask(w, h, {1023: 321}), _cells_mask(w, h, {0: 1})
        else:                 # 256 x 1024, scale 2: one block per row, ex_cap 80; list 1023 is row 1023 alone
            w, h, scale = 256, 1024, 2
            full, more, first = _rows_mask(w, h, {(1023, 0): 80}), _rows_mask(w, h, {(1023, 0): 81}), _rows_mask(w, h, {(0, 0): 1})
        none = np.zeros((h, w), bool)
        return Case(name, w, h, scale, {"a": [full, first], "b": [more & ~full, none], "u": [more, first]}[part])
    raise KeyError(name)


CAPACITY = ("at_cap", "cap_plus_one", "empty", "last_only")
PER_PIXEL = ("px_shared", "px_overflow", "px_ragged")
DEPTH = ("second_trip", "s4_wrap", "s4_wrap_overflow")
ALL = CAPACITY + ("mixed_batch",) + PER_PIXEL + DEPTH
ACCUMULATE = ("s4", "px")                      # case("acc_<kind>_a" / "_b" / "_u")
BY_CLASS = ("s4_wrap", "s4_wrap_overflow", "acc_s4_u")     # expected values from class_table(); the others from the oracle on the whole frame


@functools.lru_cache(None)
def expect(name, fmt):
    """the oracle's output of a case, (n, h, w, k), computed once and shared (read-only)"""
    c = case(name)
    e = expect_by_class(c, fmt) if name in BY_CLASS else expect_whole(c, fmt)
    e = np.ascontiguousarray(e)
    assert not (e == poison_pixel(fmt)).all(axis=-1).any()      # a pixel that still is poison after k_apply_resolve was not written
    e.flags.writeable = False
    return e
