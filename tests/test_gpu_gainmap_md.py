"""-m gpu: gain maps with gamma, offsets and an HDR capacity range -- uhdr_hip_apply_gainmap_md_batch,
uhdr_hip_generate_gainmap_md_batch and uhdr_hip_jpegr_decode_md_batch against the existing calls where the metadata is degenerate
(bit-identical) and against the model of tests/gainmap_md_cases.py everywhere else."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gainmap_md_cases as M
from tests import rgbmap_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FORMATS = (M.FMT_F16, M.FMT_PQ, M.FMT_HLG, M.FMT_RGB10)
CASE_NAMES = sorted(M.CASES)
PIX = {(1, 1): "420", (0, 0): "444", (1, 0): "422", (0, 1): "440"}


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


# ---- apply: one call over a list of images ------------------------------------------------------------------------------------------
class Item:
    """an SDR image (planes of any sampling) and its map, on the host; pads: samples added to the luma, chroma and map rows"""

    def __init__(self, Y, U, V, csx, csy, gmap, pads=(0, 0, 0)):
        self.Y, self.U, self.V, self.csx, self.csy, self.gmap, self.pads = Y, U, V, csx, csy, gmap, pads
        self.h, self.w = Y.shape
        self.rgb = gmap.ndim == 3

    def inputs(self):
        """the model's per-pixel inputs (e, g)"""
        return M.linear_sdr(self.Y, self.U, self.V, self.csx, self.csy), M.sampled_gain(self.gmap, self.w, self.h)


def _padded(a, pad, fill):
    if pad == 0:
        return np.ascontiguousarray(a)
    out = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _apply(hip, fn, items, md, fmt, boost, mode):
    """one call of an apply batch entry point: (status, [output bytes per image])"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    keep, ys, ms, outs = [], [], [], []
    for it in items:
        lp, cp, mp = it.pads
        ty = to_dev(_padded(it.Y, lp, 0xEE))
        tc = to_dev(np.concatenate([_padded(it.U, cp, 0xEE), _padded(it.V, cp, 0xEE)]))   # V chroma_stride * rows behind U
        if it.rgb:
            rgba = np.full(it.gmap.shape[:2] + (4,), 0xFF, np.uint8)
            rgba[:, :, :3] = it.gmap[:, :, :3]
            tm = to_dev(_padded(rgba, mp, 0x5A))
            ms.append(hip.rgba_map_image(tm.data_ptr(), it.gmap.shape[1], it.gmap.shape[0], it.gmap.shape[1] + mp))
        else:
            tm = to_dev(it.gmap)
            ms.append(hip.mono_image(tm.data_ptr(), it.gmap.shape[1], it.gmap.shape[0]))
        if (it.csx, it.csy) == (1, 1):
            ys.append(hip.yuv420_image(ty.data_ptr(), it.w, it.h, hip.CG_BT709, luma_stride=it.w + lp, chroma_stride=it.U.shape[1] + cp, chroma_ptr=tc.data_ptr()))
        else:
            fmt_of = {(0, 0): hip.PIX_FMT_YUV444, (1, 0): hip.PIX_FMT_YUV422, (0, 1): hip.PIX_FMT_YUV440}[(it.csx, it.csy)]
            ys.append(hip.ycbcr_image(ty.data_ptr(), it.w, it.h, hip.CG_BT709, fmt_of, luma_stride=it.w + lp, chroma_stride=it.U.shape[1] + cp,
                                      chroma_ptr=tc.data_ptr()))
        outs.append(dev_empty(hip.output_bytes(fmt, it.w, it.h) + 16, 0xCD))
        keep.append((ty, tc, tm))
    dests = hip.image_array([hip.out_image(t.data_ptr()) for t in outs])
    rc = fn(len(items), hip.image_array(ys), hip.image_array(ms), C.byref(md), fmt, boost, dests, mode, stream_ptr())
    got = []
    for it, t in zip(items, outs):
        n = hip.output_bytes(fmt, it.w, it.h)
        full = to_host(t).copy()
        assert (full[n:] == 0xCD).all()   # nothing written behind the image
        got.append(full[:n])
    return rc, got


def _plain_item(w, h, scale, seed, rgb=False, sampling="420", pads=(0, 0, 0)):
    Y, U, V, csx, csy = M.chroma_planes(w, h, sampling, seed)
    shape = (h // scale, w // scale, 3) if rgb else (h // scale, w // scale)
    return Item(Y, U, V, csx, csy, M.lcg_bytes(shape, seed + 7), pads)


def _check_general(hip, items, name, boost, fmt, mode=None, inputs=None):
    """one uhdr_hip_apply_gainmap_md_batch call over `items` against the model: the header's FAST bars"""
    lib = hip.load()
    mode = hip.APPLY_FAST if mode is None else mode
    rc, got = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, items, M.api_metadata(hip, M.CASES[name]), fmt, boost, mode)
    assert rc == 0, rc
    for k, (it, raw) in enumerate(zip(items, got)):
        e, g = inputs[k] if inputs is not None else it.inputs()
        v = M.pre_truncation(e, g, M.CASES[name], boost, fmt)
        codes = M.codes_of(raw, fmt, it.w, it.h)
        if fmt == M.FMT_F16:
            worst = float(M.half_ulp_distance(codes, v).max())
            assert worst <= 1.0, (name, boost, k, worst)
            alpha = raw.view(np.uint16).reshape(-1, 4)[:, 3]
            assert (alpha == 0x3C00).all()
        else:
            d = M.code_distance(codes, v)
            assert d.max() <= 1, (name, boost, fmt, k, int(d.max()), np.argwhere(d > 1)[:4])
            if fmt != M.FMT_RGB10:
                assert (raw.view(np.uint32) >> 30 == 3).all()
    return got


# ---- anchors: degenerate metadata is the existing calls, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("rgb", [False, True], ids=["oneplane", "rgb"])
def test_apply_md_with_degenerate_metadata_is_the_existing_call(hip, rgb):
    lib = hip.load()
    old = lib.uhdr_hip_apply_gainmap_rgb_batch if rgb else lib.uhdr_hip_apply_gainmap_batch
    items = [_plain_item(40, 24, 4, 21, rgb), _plain_item(30, 18, 3, 22, rgb)]   # the scale-4 kernel's shape and a per-pixel one
    md = M.api_metadata(hip, M.DEGENERATE)
    for mode in (hip.APPLY_FAST, hip.APPLY_EXACT):
        for fmt in FORMATS:
            for boost in (2.0, M.FLT_MAX):   # below and above maxContentBoost: the reference's displayBoost / maxContentBoost scaling
                a = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, items, md, fmt, boost, mode)
                b = _apply(hip, old, items, md, fmt, boost, mode)
                assert a[0] == 0 and b[0] == 0
                for x, y in zip(a[1], b[1]):
                    assert np.array_equal(x, y), (rgb, mode, fmt, boost)
    if not rgb:   # the modes only degenerate metadata has
        for mode in (hip.APPLY_LUT, hip.APPLY_EXACT_UNFILTERED):
            a = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, items, md, M.FMT_HLG, 3.0, mode)
            b = _apply(hip, old, items, md, M.FMT_HLG, 3.0, mode)
            assert a[0] == 0 and b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def _generate_md(hip, pairs, tf, md, rgb, offset=0):
    """one uhdr_hip_generate_gainmap_md_batch call over R.lcg_pair tuples: (status, maps, dests)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    from tests.test_gpu_rgbmap import _dev_pair
    lib = hip.load()
    bpp = 4 if rgb else 1
    keep, ys, ps, outs = [], [], [], []
    for yi, pi, arrays in pairs:
        y, p, t = _dev_pair(hip, yi, pi, arrays)
        keep.append(t)
        ys.append(y)
        ps.append(p)
        outs.append(dev_empty(bpp * (yi.width // 4) * (yi.height // 4) + 16 + offset, 0xCD))
    dests = hip.image_array([hip.out_image(t.data_ptr() + offset) for t in outs])
    rc = lib.uhdr_hip_generate_gainmap_md_batch(len(pairs), hip.image_array(ys), hip.image_array(ps), tf, C.byref(md), dests, 0, int(rgb), stream_ptr())
    maps = []
    for (yi, _, _), t in zip(pairs, outs):
        mw, mh = yi.width // 4, yi.height // 4
        full = to_host(t).copy()
        assert (full[offset + bpp * mw * mh:] == 0xCD).all() and (full[:offset] == 0xCD).all()
        m = full[offset:offset + bpp * mw * mh]
        maps.append(m.reshape(mh, mw, 4) if rgb else m.reshape(mh, mw))
    return rc, maps, dests


def _pair(orc, w, h, tf, pad=0):
    return R.lcg_pair(orc, w, h, M.generate_seed(w, tf), R.CG_709, R.CG_2100, pad)


@pytest.mark.parametrize("tf", [M.TF_HLG, M.TF_PQ])
def test_generate_md_anchors(hip, orc, tf):
    """gamma 1 and no offsets: the bytes of the three existing generate calls"""
    from tests.gpu_util import gpu_generate
    from tests.test_gpu_adaptive import Pair, run_adaptive
    from tests.test_gpu_rgbmap import _dev_pair, _gpu_generate_rgb
    lib = hip.load()
    for (w, h) in ((36, 28), (264, 200)):
        pair = _pair(orc, w, h, tf)
        y, p, keep = _dev_pair(hip, *pair)
        st, want, md, _ = gpu_generate(lib, y, p, tf)
        assert st == 0 and md.gamma == 1.0 and md.offsetSdr == 0.0
        rc, maps, dests = _generate_md(hip, [pair], tf, md, False)
        assert rc == 0 and np.array_equal(maps[0], want)
        d = dests[0]
        assert (d.width, d.height, d.luma_stride, d.pixelFormat) == (w // 4, h // 4, w // 4, hip.PIX_FMT_MONOCHROME)
        rc, rgbwant, md2, _ = _gpu_generate_rgb(hip, [pair], tf)
        rc2, maps, dests = _generate_md(hip, [pair], tf, md2, True)
        assert rc == 0 and rc2 == 0 and np.array_equal(maps[0], rgbwant[0]) and dests[0].pixelFormat == hip.PIX_FMT_RGBA8888
        # the content-adaptive call's map, given the range it returned
        apair = Pair(orc, hip, pair[2][0], pair[2][1], w, h, R.CG_709, R.CG_2100)
        rc, amaps, _, rng, _, ok = run_adaptive(hip, [apair], tf, False, hip.BOOST_PER_IMAGE)
        assert rc == 0 and ok
        lo, hi = float(rng[0]), float(rng[1])
        rc, maps, _ = _generate_md(hip, [pair], tf, M.api_metadata(hip, (1.0, 0.0, 0.0, lo, hi, lo, hi)), False)
        assert rc == 0 and np.array_equal(maps[0], amaps[0])


# ---- apply, general metadata ---------------------------------------------------------------------------------------------------------
def _boosts(name):
    b = M.BOOSTS[name]
    return (b[1], b[-1])   # a weight inside (0, 1) (flatcap: 1) and the boost capped above hdrCapacityMax


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("rgb", [False, True], ids=["oneplane", "rgb"])
def test_apply_md_small_shapes(hip, name, rgb):
    """8x8 at scale 4 (a 2x2 map: every edge table); 260x12 at scales 1, 2 and 4 (a second column block) and, 260 being no multiple
    of 3 -- applyGainMap's checks refuse such a map --, 264x12 at scale 3 (a scale that is no power of two, the second block as well)"""
    items = [_plain_item(8, 8, 4, 31, rgb)] + [_plain_item(264 if s == 3 else 260, 12, s, 32 + s, rgb) for s in (1, 2, 3, 4)]
    inputs = [it.inputs() for it in items]
    for boost in M.BOOSTS[name]:
        for fmt in FORMATS:
            _check_general(hip, items, name, boost, fmt, inputs=inputs)
    # EXACT selects the same arithmetic
    lib, md = hip.load(), M.api_metadata(hip, M.CASES[name])
    a = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, items, md, M.FMT_HLG, 2.0, hip.APPLY_FAST)
    b = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, items, md, M.FMT_HLG, 2.0, hip.APPLY_EXACT)
    assert a[0] == 0 and b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# (w, h, scale): an odd factor off the shapes above, the largest power of two below them, the first factor whose weight table lives
# for the call only (uhdr_capi.hip: kIdwCacheMaxScale = 128), and a 1 x 1 map (the corner table for every pixel)
OTHER_FACTORS = [(42, 30, 3), (96, 48, 16), (258, 258, 129), (6, 6, 6)]


@pytest.mark.parametrize("shape", OTHER_FACTORS, ids=lambda s: "%dx%d_s%d" % s)
@pytest.mark.parametrize("rgb", [False, True], ids=["oneplane", "rgb"])
def test_apply_md_other_factors(hip, shape, rgb):
    """k_apply_px_md's taps and weight tables off factors 1 to 4, against the same model and bars as the shapes above.  The gains
    come from M.sampled_gain_by_tables: sampled_gain's values (tests/test_gainmap_md_cpu.py) without its per-pixel table build"""
    w, h, s = shape
    item = _plain_item(w, h, s, 71 + s, rgb)
    inputs = [(M.linear_sdr(item.Y, item.U, item.V, item.csx, item.csy), M.sampled_gain_by_tables(item.gmap, w, h))]
    for name in CASE_NAMES:
        for boost in _boosts(name):
            for fmt in FORMATS:
                _check_general(hip, [item], name, boost, fmt, inputs=inputs)


@pytest.mark.parametrize("sampling", ["444", "422", "440"])
def test_apply_md_other_samplings(hip, sampling):
    """45x37 at scale 1 with 4:4:4, 4:2:2 and 4:4:0 primaries, one-plane and RGB maps, padded chroma rows"""
    items = [_plain_item(45, 37, 1, 41, False, sampling), _plain_item(45, 37, 1, 42, True, sampling, pads=(3, 5, 2))]
    inputs = [it.inputs() for it in items[:1]] + [items[1].inputs()]
    for name in CASE_NAMES:
        for fmt in (M.FMT_HLG, M.FMT_F16):
            _check_general(hip, items[:1], name, _boosts(name)[0], fmt, inputs=inputs[:1])
            _check_general(hip, items[1:], name, _boosts(name)[1], fmt, inputs=inputs[1:])


def test_apply_md_tall_image_strides_batches(hip):
    """4x65600 at scale 4 (the row loop's second trip); padded luma, chroma and RGBA-map rows; 65 images of 8x8 (past one launch's 64);
    a batch of mixed sizes"""
    tile = M.chroma_planes(4, 64, "420", 51)
    reps = 65600 // 64
    Y, U, V = np.tile(tile[0], (reps, 1)), np.tile(tile[1], (reps, 1)), np.tile(tile[2], (reps, 1))
    tall = Item(Y, U, V, 1, 1, M.lcg_bytes((65600 // 4, 1), 52))
    tall_inputs = [tall.inputs()]
    _check_general(hip, [tall], "gamma22", 2.0, M.FMT_HLG, inputs=tall_inputs)
    _check_general(hip, [tall], "default", 100.0, M.FMT_RGB10, inputs=tall_inputs)
    padded = [_plain_item(24, 16, 4, 53, False, pads=(8, 4, 0)), _plain_item(24, 16, 4, 54, True, pads=(5, 3, 3)), _plain_item(24, 16, 2, 55, True, pads=(1, 1, 1))]
    for it in padded:
        for name in ("black", "gamma22"):
            _check_general(hip, [it], name, 3.0, M.FMT_PQ)
            _check_general(hip, [it], name, 3.0, M.FMT_F16)
    for rgb in (False, True):
        many = [_plain_item(8, 8, 4, 600 + k, rgb) for k in range(65)]
        _check_general(hip, many, "flatcap" if rgb else "gamma22", 2.0, M.FMT_HLG)
    mixed = [_plain_item(8, 8, 4, 61), _plain_item(24, 16, 4, 62), _plain_item(8, 8, 4, 63), _plain_item(12, 20, 2, 64)]
    _check_general(hip, mixed, "black", M.FLT_MAX, M.FMT_PQ)


def test_apply_md_differing_shares(hip):
    """the 264x200 folded LCG pair, the three 10-bit formats pooled.  Two bars, both shares measured in the same run and printed.
    (1) The share of channels by which the new path differs from the model's floor(v), per case, may be at most twice the share by
    which the EXISTING FAST call (uhdr_hip_apply_gainmap_batch: on this pair the scale-4 table kernel k_apply_s4) differs from the
    model at degenerate metadata: the general path adds at most one log2 / exp2 pair in front of the same exponent.
    (2) That kernel is a hundred times further from the model than per-pixel f32 arithmetic, so (1) alone would let the new path
    get ten times worse unnoticed.  The comparable kernel is the per-pixel FAST one (k_apply_px_rgb, channel by channel k_apply_px's
    arithmetic): over the channels whose linear value is at most 1.0 -- above it a 10-bit code grows without bound and an f32's
    relative error is that many codes; the degenerate run has no such channel -- the new path's share may be at most FOUR times the
    per-pixel call's.  Four, not two: the per-pixel shares are ~3e-5 of 475200 channels, some 15 events; two Poisson counts of
    that size drawn from the same rate differ by a factor of up to 3 at two sigma each way (8 against 23).  Four clears that and is
    well under the tenfold change the bar is there to catch."""
    lib = hip.load()
    s = M.share_inputs()
    w, h = s["w"], s["h"]
    Y, U, V = M.planes_of(s["yuv"], w, h)
    fmts = (M.FMT_PQ, M.FMT_HLG, M.FMT_RGB10)

    def shares(fn, item, g, case, boost):
        """(share over all channels, share over the channels whose linear value is <= 1)"""
        md = M.api_metadata(hip, case)
        inside = M.linear_out(s["e"], g, case, boost) <= 1.0
        diff = total = diff_in = total_in = 0
        for fmt in fmts:
            rc, got = _apply(hip, fn, [item], md, fmt, boost, hip.APPLY_FAST)
            assert rc == 0
            d = M.code_distance(M.codes_of(got[0], fmt, w, h), M.pre_truncation(s["e"], g, case, boost, fmt))
            assert d.max() <= 1
            diff += int((d != 0).sum())
            total += d.size
            diff_in += int((d[inside] != 0).sum())
            total_in += int(inside.sum())
        return diff / total, diff_in / max(total_in, 1)

    items = {rgb: Item(Y, U, V, 1, 1, s["gmap"] if rgb else np.ascontiguousarray(s["gmap"][:, :, 0])) for rgb in (False, True)}
    base, _ = shares(lib.uhdr_hip_apply_gainmap_batch, items[False], s["g1"], M.DEGENERATE, M.FLT_MAX)
    base_px, base_px_in = shares(lib.uhdr_hip_apply_gainmap_rgb_batch, items[True], s["g3"], M.DEGENERATE, M.FLT_MAX)
    print("differing share: existing FAST call at degenerate metadata %.5f" % base)
    print("differing share: existing per-channel (per-pixel kernel) FAST call at degenerate metadata %.5f" % base_px)
    assert base > 0 and base_px > 0 and base_px == base_px_in
    for rgb in (False, True):
        item, g = items[rgb], s["g3"] if rgb else s["g1"]
        for name in CASE_NAMES:
            for boost in _boosts(name):
                got, got_in = shares(lib.uhdr_hip_apply_gainmap_md_batch, item, g, M.CASES[name], boost)
                print("differing share, %s map: %s at D = %g %.5f; channels with a linear value <= 1: %.5f" %
                      ("RGB" if rgb else "one-plane", name, boost, got, got_in))
                assert got <= 2.0 * base, (rgb, name, boost, got, base)
                assert got_in <= 4.0 * base_px, (rgb, name, boost, got_in, base_px)


# ---- generate, general metadata ------------------------------------------------------------------------------------------------------
def _check_map(got, want, v, what):
    """bytes equal the model's; a pixel whose value in front of the truncation is within 2^-30 of an integer may differ by one"""
    bad = got.astype(np.int32) != want.astype(np.int32)
    if bad.any():
        assert (M.in_doubt(v)[bad]).all() and np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1, (what, int(bad.sum()))


@pytest.mark.parametrize("tf", [M.TF_HLG, M.TF_PQ, M.TF_LINEAR])
@pytest.mark.parametrize("size", [(36, 28), (264, 200)], ids=["36x28", "264x200"])
def test_generate_md_against_the_model(hip, orc, size, tf):
    """36x28: a 9x7 map, the unaligned path with an unpaired last pixel, fewer pairs than one block (35 < kGenBlock = 256);
    264x200: 33 x 50 = 1650 pairs, seven blocks of kGenBlock pairs (such a launch is "small": one span per block; blocks of
    kGenBlock * kGenTiles = 1024 pairs are test_generate_md_blocks_of_several_spans')"""
    w, h = size
    s = M.generate_inputs(w, h, tf)
    pair = _pair(orc, w, h, tf)
    assert np.array_equal(pair[2][0], s["p010"]) and np.array_equal(pair[2][1], s["yuv"])
    for name in CASE_NAMES:
        md = M.api_metadata(hip, M.CASES[name])
        rc, maps, _ = _generate_md(hip, [pair], tf, md, False)
        want, v = M.encode(s["ys"], s["yh"], M.CASES[name])
        assert rc == 0
        _check_map(maps[0], want, v, (name, "one plane"))
        for off in ((0, 4) if w == 264 else (0,)):   # the 8-byte pair stores, and the ragged kernel on the same image
            rc, maps, _ = _generate_md(hip, [pair], tf, md, True, offset=off)
            want, v = M.encode(s["sdr"], s["hdr"], M.CASES[name])
            assert rc == 0 and (maps[0][:, :, 3] == 0xFF).all()
            _check_map(maps[0][:, :, :3], want, v, (name, "rgb", off))
        assert len(np.unique(want)) > 20


def test_generate_md_padded_strides_and_65_images(hip, orc):
    tf = M.TF_HLG
    s = M.generate_inputs(264, 200, tf)
    for pad in (8, 6):   # the aligned path with longer rows, the ragged one
        pair = _pair(orc, 264, 200, tf, pad)
        for rgb in (False, True):
            rc, maps, _ = _generate_md(hip, [pair], tf, M.api_metadata(hip, M.CASES["gamma22"]), rgb)
            want, v = M.encode(*((s["sdr"], s["hdr"]) if rgb else (s["ys"], s["yh"])), M.CASES["gamma22"])
            assert rc == 0
            _check_map(maps[0][:, :, :3] if rgb else maps[0], want, v, (pad, rgb))
    small = M.generate_inputs(36, 28, tf)
    pairs = [_pair(orc, 36, 28, tf)] * 65   # past one launch's 64 images
    for rgb in (False, True):
        rc, maps, _ = _generate_md(hip, pairs, tf, M.api_metadata(hip, M.CASES["black"]), rgb)
        want, v = M.encode(*((small["sdr"], small["hdr"]) if rgb else (small["ys"], small["yh"])), M.CASES["black"])
        assert rc == 0
        for m in (maps[0], maps[63], maps[64]):
            _check_map(m[:, :, :3] if rgb else m, want, v, ("65 images", rgb))
    # maxContentBoost == minContentBoost passes validation: every gain is on a clamp, the byte is 0
    for gamma in (1.0, 2.2):
        rc, maps, _ = _generate_md(hip, pairs[:1], tf, M.api_metadata(hip, (gamma, 1 / 64, 1 / 64, 2.0, 2.0, 2.0, 2.0)), False)
        assert rc == 0 and (maps[0] == 0).all()


def test_generate_md_blocks_of_several_spans(hip, orc):
    """The kernel instances every production-sized batch runs: launch_generate_md hands a block kGenTiles = 4 spans of kGenBlock = 256
    pairs once generate_is_small says no -- ceil(pairs / 1024) x images >= 1024.  64 copies of a 712x704 pair: a 178x176 map,
    89 x 176 = 15664 pairs = 15 x 1024 + 304, 16 blocks per image, the last of which runs out inside its second span (the tile loop's
    `idx >= total` break in a later tile).  One-plane and RGB, the aligned stores and the ragged kernel (map pointers 1 / 4 bytes
    off); gamma 1 without offsets against the existing calls, one general case against the model."""
    from tests.gpu_util import gpu_generate
    from tests.test_gpu_rgbmap import _dev_pair, _gpu_generate_rgb
    w, h, tf, n = 712, 704, M.TF_HLG, 64
    pairs_per_image = ((w // 4 + 1) // 2) * (h // 4)
    assert -(-pairs_per_image // 1024) * n >= 1024 and 256 < pairs_per_image % 1024 < 1024   # not small; the tail ends in a later span
    s = M.generate_inputs(w, h, tf)
    pair = _pair(orc, w, h, tf)
    batch = [pair] * n
    # anchors
    y, p, keep = _dev_pair(hip, *pair)
    st, one_want, md, _ = gpu_generate(hip.load(), y, p, tf)
    rc, rgb_want, md2, _ = _gpu_generate_rgb(hip, batch, tf)
    assert st == 0 and rc == 0
    for off in (0, 1):
        rc, maps, _ = _generate_md(hip, batch, tf, md, False, offset=off)
        assert rc == 0 and all(np.array_equal(m, one_want) for m in maps), off
    for off in (0, 4):
        rc, maps, _ = _generate_md(hip, batch, tf, md2, True, offset=off)
        assert rc == 0 and all(np.array_equal(m, rgb_want[0]) for m in maps), off
    # a general case against the model
    case = M.CASES["gamma22"]
    want1, v1 = M.encode(s["ys"], s["yh"], case)
    want3, v3 = M.encode(s["sdr"], s["hdr"], case)
    for off in (0, 1):
        rc, maps, _ = _generate_md(hip, batch, tf, M.api_metadata(hip, case), False, offset=off)
        assert rc == 0 and all(np.array_equal(m, maps[0]) for m in maps)
        _check_map(maps[0], want1, v1, ("several spans, one plane", off))
    for off in (0, 4):
        rc, maps, _ = _generate_md(hip, batch, tf, M.api_metadata(hip, case), True, offset=off)
        assert rc == 0 and all(np.array_equal(m, maps[0]) for m in maps)
        _check_map(maps[0][:, :, :3], want3, v3, ("several spans, rgb", off))


# ---- files -------------------------------------------------------------------------------------------------------------------------
def _decode_planes(hip, data, flags=0):
    """uhdr_hip_jpeg_decode_batch_ex of one file into host memory: (planes, descriptor)"""
    lib = hip.load()
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    ptrs, sizes = _arr(C.c_void_p, [buf.ctypes.data]), _arr(C.c_size_t, [len(data)])
    d, st = (hip.Image * 1)(), _arr(C.c_int, [7])
    lib.uhdr_hip_jpeg_decode_batch_ex(1, ptrs, sizes, hip.DECODE_TO_YCBCR, None, None, d, st, hip.MEM_HOST, None, flags)
    need = d[0].width * d[0].height * 3
    out = np.zeros(need, np.uint8)
    rc = lib.uhdr_hip_jpeg_decode_batch_ex(1, ptrs, sizes, hip.DECODE_TO_YCBCR, _arr(C.c_void_p, [out.ctypes.data]), _arr(C.c_size_t, [need]), d, st,
                                           hip.MEM_HOST, None, flags)
    assert rc == 0 and st[0] == 0, (rc, st[0])
    return out, d[0]


def _item_of_file(hip, data, flags):
    """the file's own decoded pieces as an Item: the primary's planes and the map's plane (one component) or RGBA (three)"""
    from tests.test_gpu_rgbmap import _info, _jpeg_decode
    primary, gm = _info(hip, data)
    planes, d = _decode_planes(hip, primary, flags)
    w, h = d.width, d.height
    cw, ch = hip.chroma_size(d.pixelFormat, w, h)
    Y = planes[:w * h].reshape(h, w)
    U, V = planes[w * h:w * h + cw * ch].reshape(ch, cw), planes[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    csx, csy = {hip.PIX_FMT_YUV444: (0, 0), hip.PIX_FMT_YUV422: (1, 0), hip.PIX_FMT_YUV440: (0, 1)}.get(d.pixelFormat, (1, 1))
    if _components(gm) == 3:
        rc, rgba, gd = _jpeg_decode(hip, gm, hip.DECODE_TO_RGBA, hip.DECODE_ANY_SAMPLING)
        assert rc == 0
        gmap = rgba.reshape(gd.height, gd.width, 4)[:, :, :3].copy()
    else:
        mp, md_ = _decode_planes(hip, gm, hip.DECODE_ANY_SAMPLING)
        gmap = mp[:md_.width * md_.height].reshape(md_.height, md_.width).copy()
    return Item(Y.copy(), U.copy(), V.copy(), csx, csy, gmap)


def _components(jpeg):
    """Nf of the first SOF0 / SOF2 segment"""
    i = 2
    while i + 4 <= len(jpeg):
        marker, n = jpeg[i + 1], (jpeg[i + 2] << 8) | jpeg[i + 3]
        if marker in (0xC0, 0xC2):
            return jpeg[i + 9]
        i += 2 + n
    return 0


def _mono_jpeg(hip, plane, q=85):
    lib = hip.load()
    h, w = plane.shape
    src = np.ascontiguousarray(plane)
    out, n = np.zeros(w * h * 3 + 4096, np.uint8), C.c_size_t()
    img = hip.mono_image(src.ctypes.data, w, h)
    assert lib.uhdr_hip_jpeg_encode(C.byref(img), q, None, 0, C.c_void_p(out.ctypes.data), out.size, C.byref(n), hip.MEM_HOST, None) == 0
    return out[:n.value].tobytes()


def _md_dict(case):
    g, os_, oh, lo, hi, hmin, hmax = M.fields(case)
    return dict(version="1.0", max=hi, min=lo, gamma=g, off_sdr=os_, off_hdr=oh, capmin=hmin, capmax=hmax)


def _apix_file(hip, yuv, w, h, gmap, case):
    """uhdr_hip_jpegr_encode_apix_batch of host planes and a one-plane map with the case's metadata"""
    lib = hip.load()
    src, mp = np.ascontiguousarray(yuv), np.ascontiguousarray(gmap)
    out, n, st = np.zeros(w * h * 4 + 65536, np.uint8), _arr(C.c_size_t, [0]), _arr(C.c_int, [7])
    y = hip.yuv420_image(src.ctypes.data, w, h, hip.CG_BT709)
    m = hip.mono_image(mp.ctypes.data, gmap.shape[1], gmap.shape[0])
    md = (hip.Metadata * 1)(M.api_metadata(hip, case))
    rc = lib.uhdr_hip_jpegr_encode_apix_batch(1, C.byref(y), C.byref(m), md, 90, None, None, _arr(C.c_void_p, [out.ctypes.data]), _arr(C.c_size_t, [out.size]), n, st,
                                              hip.MEM_HOST, None)
    assert rc == 0 and st[0] == 0, (rc, st[0])
    return out[:n[0]].tobytes()


def _files_of_case(hip, orc, name):
    """generate_md -> files: the one-plane map through API-x, the RGB map as a 4:4:4 JPEG behind the same primary"""
    from oracle import jpegr_oracle as J
    from tests.test_gpu_rgbmap import _encode_rgb, _info
    w, h, tf = 72, 40, M.TF_HLG
    pair = R.lcg_pair(orc, w, h, 81, R.CG_709, R.CG_2100)
    md = M.api_metadata(hip, M.CASES[name]) if name != "degenerate" else M.api_metadata(hip, M.DEGENERATE)
    case = M.CASES[name] if name != "degenerate" else M.DEGENERATE
    rc, one, _ = _generate_md(hip, [pair], tf, md, False)
    rc2, rgb, _ = _generate_md(hip, [pair], tf, md, True)
    assert rc == 0 and rc2 == 0
    f1 = _apix_file(hip, pair[2][1], w, h, one[0], case)
    rc, stat, _, gm = _encode_rgb(hip, [rgb[0]], [90], True)
    assert rc == 0
    f3 = J.append_gainmap(_info(hip, f1)[0], gm[0], _md_dict(case))
    assert isinstance(f3, bytes)
    return f1, f3


@pytest.mark.parametrize("name", CASE_NAMES)
def test_files_round_trip(hip, orc, name):
    """generate_md, API-x (one-plane) or the 4:4:4 map JPEG in the container (three-component), then uhdr_hip_jpegr_decode_md_batch:
    the result is uhdr_hip_apply_gainmap_md_batch on the file's own decoded planes and parsed metadata; the existing decode still
    refuses the file"""
    from tests.test_gpu_rgbmap import _jpegr_decode
    lib = hip.load()
    files = list(_files_of_case(hip, orc, name))
    items = [_item_of_file(hip, f, 0) for f in files]
    assert not items[0].rgb and items[1].rgb
    for out_fmt, boost, device in ((M.FMT_HLG, _boosts(name)[0], True), (M.FMT_F16, _boosts(name)[1], False)):
        rc, stat, got, dests, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, files, out_fmt, hip.APPLY_FAST, device, boost=boost)
        assert rc == 0 and stat == [0, 0], stat
        for k in range(2):
            assert not M.is_degenerate((mds[k].gamma, mds[k].offsetSdr, mds[k].offsetHdr, mds[k].minContentBoost, mds[k].maxContentBoost,
                                        mds[k].hdrCapacityMin, mds[k].hdrCapacityMax))
            rc, want = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, [items[k]], mds[k], out_fmt, boost, hip.APPLY_FAST)
            assert rc == 0 and np.array_equal(got[k], want[0]), (name, out_fmt, k)
    rc, stat, _, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_batch_ex, files, M.FMT_HLG, hip.APPLY_FAST, True, flags=hip.DECODE_ANY_SAMPLING)
    assert rc == hip.ERROR_BAD_METADATA and stat == [hip.ERROR_BAD_METADATA] * 2
    rc, stat, _, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, M.FMT_HLG, hip.APPLY_FAST, True)
    assert stat == [hip.ERROR_BAD_METADATA] * 2
    # LUT has no general form: per file
    rc, stat, _, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, files, M.FMT_HLG, hip.APPLY_LUT, True)
    assert stat == [hip.ERROR_UNSUPPORTED_FEATURE] * 2


def test_files_degenerate_sdr_444_and_a_broken_neighbour(hip, orc):
    from oracle import jpegr_oracle as J
    from tests import sampling_cases as S
    from tests.test_gpu_rgbmap import _jpegr_decode
    lib = hip.load()
    # a degenerate file: identical bytes through both decode calls, in every mode
    deg = list(_files_of_case(hip, orc, "degenerate"))
    for mode in (hip.APPLY_EXACT, hip.APPLY_FAST, hip.APPLY_LUT):
        for out_fmt in (M.FMT_HLG, M.FMT_F16, hip.OUTPUT_SDR):
            files = deg if mode != hip.APPLY_LUT else deg[:1]
            a = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, files, out_fmt, mode, True, boost=2.0)
            b = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, files, out_fmt, mode, True, boost=2.0)
            assert a[0] == 0 and b[0] == 0 and a[1] == b[1]
            assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), (mode, out_fmt)
    # UHDR_HIP_OUTPUT_SDR of a general file: the primary's RGBA, as ever
    gen = list(_files_of_case(hip, orc, "gamma22"))
    a = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, gen, hip.OUTPUT_SDR, hip.APPLY_FAST, True)
    b = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_rgbmap_batch, gen, hip.OUTPUT_SDR, hip.APPLY_FAST, True)
    assert a[0] == 0 and b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    # a 4:4:4 primary (8x8) with a 2x2 one-plane map under UHDR_HIP_DECODE_ANY_SAMPLING
    hs, vs, w, h, primary, _ = S.fixture("s11_base_8x8")
    f444 = J.append_gainmap(primary, _mono_jpeg(hip, M.lcg_bytes((2, 2), 91)), _md_dict(M.CASES["default"]))
    assert isinstance(f444, bytes)
    rc, stat, got, _, mds = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, [f444], M.FMT_HLG, hip.APPLY_FAST, True, flags=hip.DECODE_ANY_SAMPLING, boost=3.0)
    assert rc == 0 and stat == [0]
    item = _item_of_file(hip, f444, hip.DECODE_ANY_SAMPLING)
    assert (item.csx, item.csy) == (0, 0)
    rc, want = _apply(hip, lib.uhdr_hip_apply_gainmap_md_batch, [item], mds[0], M.FMT_HLG, 3.0, hip.APPLY_FAST)
    assert rc == 0 and np.array_equal(got[0], want[0])
    rc, stat, _, _, _ = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, [f444], M.FMT_HLG, hip.APPLY_FAST, True)
    assert stat[0] != 0   # without the flag the primary's sampling is refused, as by the other decode calls
    # a mixed batch: one file with malformed XMP between two good ones, which are unaffected
    broken = gen[0].replace(b'hdrgm:Gamma="2.2"', b'hdrgm:Gamma="x.y"')
    assert broken != gen[0] and len(broken) == len(gen[0])
    alone = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, [gen[0], gen[1]], M.FMT_HLG, hip.APPLY_FAST, True, boost=2.0)
    mixed = _jpegr_decode(hip, lib.uhdr_hip_jpegr_decode_md_batch, [gen[0], broken, gen[1]], M.FMT_HLG, hip.APPLY_FAST, True, boost=2.0)
    assert alone[0] == 0 and mixed[0] == hip.ERROR_METADATA_ERROR and mixed[1] == [0, hip.ERROR_METADATA_ERROR, 0]
    assert np.array_equal(mixed[2][0], alone[2][0]) and np.array_equal(mixed[2][2], alone[2][1])


# ---- the C++ shim --------------------------------------------------------------------------------------------------------------------
def test_the_shims_setter(hip, orc, tmp_path):
    """ultrahdr::JpegRHip::setAnyGainMapMetadata: off (the default) decodeJPEGR refuses a general file as ever; on, it returns
    uhdr_hip_jpegr_decode_md_batch's bytes, and a degenerate file decodes to the same bytes either way; gainMapWeight is the C call"""
    from tests.test_gpu_rgbmap import _jpegr_decode
    lib = hip.load()
    exe = str(tmp_path / "shim_gainmap_md_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_gainmap_md_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    gen, deg = _files_of_case(hip, orc, "gamma22"), _files_of_case(hip, orc, "degenerate")
    for n, data in (("gen1.jpgr", gen[0]), ("gen3.jpgr", gen[1]), ("deg1.jpgr", deg[0])):
        open(tmp_path / n, "wb").write(data)
    r = subprocess.run([exe, str(tmp_path), "72", "40"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = lambda n: np.frombuffer(open(tmp_path / n, "rb").read(), np.uint8)
    dec = lambda fn, f: _jpegr_decode(hip, fn, [f], M.FMT_HLG, hip.APPLY_EXACT, False, boost=3.0)[2][0]
    assert np.array_equal(got("gen1_on.bin"), dec(lib.uhdr_hip_jpegr_decode_md_batch, gen[0]))
    assert np.array_equal(got("gen3_on.bin"), dec(lib.uhdr_hip_jpegr_decode_md_batch, gen[1]))
    assert np.array_equal(got("deg1_on.bin"), dec(lib.uhdr_hip_jpegr_decode_batch_ex, deg[0]))
    assert np.array_equal(got("deg1_on.bin"), got("deg1_off.bin"))
