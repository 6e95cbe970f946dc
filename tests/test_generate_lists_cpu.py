"""CPU tests of what tests/test_gpu_generate_lists.py stands on: the frame builder (tests/generate_list_cases.py) -- margins, poison,
the oracle's bytes -- and phase 0 of uhdr_hip_generate_probe, the route a generate call takes, on both sides of every threshold.
Phase 0 is host arithmetic over the descriptors: no device, and the data pointers are never read."""
import ctypes as C

import numpy as np
import pytest

from tests import generate_list_cases as K
ROUTE_KEYS = K.ROUTE_KEYS


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _route(api, w, h, n, stats, mode=None, tf=1, base=0x10000000, gamut_of=None):
    fb = w * h * 3 // 2
    fb_al = (fb + 255) // 256 * 256
    ya = api.image_array([api.yuv420_image(base + i * fb_al, w, h, K.GAMUT if gamut_of is None else gamut_of(i)) for i in range(n)])
    pa = api.image_array([api.p010_image(base + (n + 2 * i) * fb_al, w, h, K.GAMUT) for i in range(n)])
    da = api.image_array([api.out_image(base + 3 * n * fb_al + i * fb_al) for i in range(n)])
    md = api.Metadata()
    r = (C.c_uint32 * api.ROUTE_WORDS)()
    rc = api.load().uhdr_hip_generate_probe(0, n, ya, pa, tf, C.byref(md), da, 0, api.GENERATE_EXACT if mode is None else mode,
                                           C.c_void_p(0x20000000) if stats else None, None, r, None)
    assert rc == 0
    assert abs(md.maxContentBoost - K.filter_consts(tf)[0]) < 1e-6 and md.minContentBoost == 1.0   # filled as by the call itself
    return dict(zip(ROUTE_KEYS, list(r)))


def _pick(r, *keys):
    return tuple(r[k] for k in keys)


def test_route_constants(api):
    r = _route(api, 1024, 512, 64, False)
    assert _pick(r, "block", "slot_saved", "slot_plain", "lists", "list_cap", "resolve_slices", "slot_waves") == (256, 4, 15, 64, 252, 16, 1024)
    assert r["hdr_words"] == r["slot_counts"] + r["slot_waves"] and r["slot_counts"] % 4 == 0
    assert r["sweep_word"] < r["list_counts"] and r["list_counts"] + r["lists"] <= r["slot_counts"]


def test_route_without_statistics_at_1023_and_1024_spans(api):
    """the four-span kernel + k_generate_resolve from 1024 spans of 1024 pairs in the launch"""
    assert _pick(_route(api, 1024, 512, 64, False), "resolve", "spans", "slots", "images") == (1, 4, 64, 64)     # 16 x 64 = 1024
    assert _pick(_route(api, 1024, 512, 63, False), "resolve", "spans", "slots") == (0, 1, 0)                    # 1008
    # 1056 x 1024: 132 x 256 pairs = 33 spans exactly; 31 images 1023 spans, 32 images 1056
    assert (1056 // 8) * (1024 // 4) == 33 * 1024
    assert _pick(_route(api, 1056, 1024, 31, False), "resolve", "spans") == (0, 1)
    assert _pick(_route(api, 1056, 1024, 32, False), "resolve", "spans", "slots") == (1, 4, 33 * 4)
    # the other modes never take the pair
    assert _route(api, 1024, 512, 64, False, mode=api.GENERATE_UNFILTERED)["resolve"] == 0
    assert _route(api, 1024, 512, 64, False, mode=api.GENERATE_LUT)["resolve"] == 0
    # an image whose planes miss the alignment of the vector loads: the unfiltered kernel
    assert _route(api, 1024, 512, 64, False, base=0x10000001)["resolve"] == 0


def test_route_with_statistics_at_127_and_128_spans(api):
    """with content_minmax the pair pays from 128 spans; below 1024 spans a block walks one span"""
    assert _pick(_route(api, 1024, 512, 8, True), "resolve", "spans", "slots", "spread") == (1, 1, 256, 0)       # 16 x 8 = 128
    assert _pick(_route(api, 1024, 512, 7, True), "resolve", "spans") == (0, 1)                                  # 112
    assert (2032 // 8) * (2048 // 4) == 127 * 1024
    assert _pick(_route(api, 2032, 2048, 1, True), "resolve", "spans") == (0, 1)                                 # 127
    assert _pick(_route(api, 2032, 2056, 1, True), "resolve", "spans", "slots") == (1, 1, 0)                     # 128: 510 blocks of 4 waves
    assert _pick(_route(api, 1024, 512, 64, True), "resolve", "spans", "slots") == (1, 4, 64)


def test_route_slots_at_1024_and_1028_waves(api):
    assert _pick(_route(api, 4096, 2048, 4, False), "resolve", "spans", "slots") == (1, 4, 1024)
    assert _pick(_route(api, 4096, 2056, 4, False), "resolve", "spans", "slots") == (1, 4, 0)
    assert _pick(_route(api, 4096, 2052, 4, False), "resolve", "spans", "slots") == (1, 4, 0)                    # 257 blocks: 1028 waves as well
    # one span per block: 256 blocks of 4 waves
    assert _pick(_route(api, 1024, 1024, 4, True), "resolve", "spans", "slots") == (1, 1, 512)                   # 32 768 pairs: 128 blocks of 4 waves
    assert _pick(_route(api, 2048, 1024, 2, True), "resolve", "spans", "slots") == (1, 1, 1024)                  # 65 536 pairs: 256 blocks, 1024 waves
    assert _pick(_route(api, 2048, 1028, 2, True), "resolve", "spans", "slots") == (1, 1, 0)                     # 257 blocks
    assert _pick(_route(api, 3840, 2160, 1, True), "resolve", "spans", "slots", "spread") == (1, 1, 0, 1)


def test_route_spread_at_16_and_17_images(api):
    """estimates per list: launches of at most 16 images of at least 512 waves' worth of pairs (32 768)"""
    assert (1024 // 8) * (1024 // 4) == 32768
    assert _pick(_route(api, 1024, 1024, 16, True), "resolve", "spread") == (1, 1)
    assert _pick(_route(api, 1024, 1024, 17, True), "resolve", "spread") == (1, 0)
    assert _pick(_route(api, 1024, 1016, 16, True), "resolve", "spread") == (1, 0)                               # 32 512 pairs
    assert _pick(_route(api, 1024, 1024, 16, False), "resolve", "spread") == (0, 0)                              # 512 spans without statistics: small


def test_route_reports_the_first_chunk_and_checks_like_the_call(api):
    assert _route(api, 1024, 512, 64, False, gamut_of=lambda i: 1 if i >= 40 else 0)["images"] == 40
    lib = api.load()
    r = (C.c_uint32 * api.ROUTE_WORDS)()
    md = api.Metadata()
    one = api.image_array([api.yuv420_image(0x1000, 64, 64, 0)])
    p = api.image_array([api.p010_image(0x9000, 64, 64, 0)])
    d = api.image_array([api.out_image(0x20000)])
    args = (1, one, p, 1, C.byref(md), d, 0, api.GENERATE_EXACT, None, None)
    assert lib.uhdr_hip_generate_probe(0, *args, r, None) == 0 and r[0] == 0
    assert lib.uhdr_hip_generate_probe(0, *args, None, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_generate_probe(-1, *args, r, None) == api.ERROR_UNSUPPORTED_FEATURE
    assert lib.uhdr_hip_generate_probe(3, *args, r, None) == api.ERROR_UNSUPPORTED_FEATURE
    assert lib.uhdr_hip_generate_probe(0, 0, one, p, 1, C.byref(md), d, 0, api.GENERATE_EXACT, None, None, r, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_generate_probe(0, 1, one, p, 7, C.byref(md), d, 0, api.GENERATE_EXACT, None, None, r, None) == api.ERROR_INVALID_TRANS_FUNC
    assert lib.uhdr_hip_generate_probe(0, 1, one, p, 1, C.byref(md), d, 0, 9, None, None, r, None) == api.ERROR_UNSUPPORTED_FEATURE
    bad = api.image_array([api.p010_image(0x9000, 64, 32, 0)])
    assert lib.uhdr_hip_generate_probe(0, 1, one, bad, 1, C.byref(md), d, 0, api.GENERATE_EXACT, None, None, r, None) == api.ERROR_RESOLUTION_MISMATCH


# ---- the builder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tf", [0, 1, 2])
def test_pools_keep_their_margins(orc, tf):
    (by, bp), (dy, dp) = K.pools(tf)
    gain, code = K.pair_codes(tf)
    max_boost, scale, delta = K.filter_consts(tf)
    table = K.pair_table(tf)
    assert 0.0008 < delta < 0.001 and by.size > 50000 and 5 <= dy.size <= 40
    g, v = gain[by, bp.astype(int) - K.P_LO], code[by, bp.astype(int) - K.P_LO]
    assert g.min() > 1.02 and g.max() < 0.98 * max_boost and by.min() >= 1
    assert np.abs(v - np.rint(v)).min() >= 3.0 * delta
    vb = code[dy, dp.astype(int) - K.P_LO]
    assert np.abs(vb - np.rint(vb)).max() <= 0.1 * delta
    assert (table[by, bp.astype(int) - K.P_LO] != K.POISON).all() and (table[dy, dp.astype(int) - K.P_LO] != K.POISON).all()
    assert (table[0] == 0).all() and K.POISON != 0      # a pixel without SDR luminance: gain 1.0, the byte of the minimum
    assert len(set(table[dy, dp.astype(int) - K.P_LO])) >= 5   # boundary pairs with distinct gains


ROUTE_A = dict(zip(ROUTE_KEYS, (1, 4, 64, 0, 64, 256, 1224, 200, 15, 4, 64, 252, 8, 6, 16, 1024)))


def test_builder_places_pairs_and_matches_the_oracle_on_whole_frames(orc, api):
    """the smallest shape, two images: the table look-up is oracle.generate's map, the designed pixels are where the kernel's index
    arithmetic puts them, the statistics' minimum is the pixels in doubt's"""
    assert ROUTE_A == _route(api, 1024, 512, 64, False)
    w, h = 1024, 512
    pl = {(0, 0, 0): [(0, 0, 1)], (0, 15, 3): [(3, 63, 3)], (1, 2, 1): [(1, 5, 2), (2, 6, 3)]}
    case = K.build(ROUTE_A, w, h, 2, pl, seed=5, boundary_every=2)
    assert case.designed.sum() == 6 and case.designed[0, 0, 0] and not case.designed[0, 0, 1]
    assert case.designed[0, 127, 254] and case.designed[0, 127, 255]          # the image's last pair: block 15, wave 3, tile 3, lane 63
    idx = (2 * 4 + 1) * 256 + 64 + 5
    assert case.designed[1, idx // 128, 2 * (idx % 128) + 1] and not case.designed[1, idx // 128, 2 * (idx % 128)]
    assert (case.yb[case.designed] == 0).sum() == 3                            # every second designed pixel is a boundary pair
    for i in range(2):
        st, om, _, mm = orc.generate("orc_", orc.yuv420_image(case.yuv[i], w, h, K.GAMUT), orc.p010_image(case.p010[i], w, h, K.GAMUT), 1, False,
                                     threads=8, stats=True)
        assert st == 0 and np.array_equal(om, case.expect[i]) and mm[0] == 1.0
        assert (om[case.yb[i] == 0] == 0).all() and not (om == K.POISON).any()
    hdr, swept = case.header(ROUTE_A)
    assert hdr[0, 200] == 1 << 8 and hdr[0, 200 + 63] == 1 << 8 and hdr[1, 200 + 9] == 2 << 8 and hdr.sum() == 4 << 8 and not swept.any()


def test_expected_headers_at_the_limits():
    lay = K.wave_layouts(ROUTE_A)
    for name, (entries, word, sweeps) in lay.items():
        c = K.Case(1024, 512, 1, 1)
        c.pairs = {(0, 3, 2): len(entries)}
        hdr, swept = c.header(ROUTE_A)
        assert hdr[0, 200 + 14] == word and bool(swept[0]) == sweeps and hdr[0, 6] == int(sweeps), name
        assert len({(t, l) for t, l, _ in entries}) == len(entries)
    lists = dict(ROUTE_A, slots=0)
    c = K.Case(4096, 2056, 2, 1)
    c.pairs = {(0, 5, 0): 200, (0, 69, 1): 52, (1, 5, 0): 200, (1, 133, 3): 53, (1, 256, 0): 1}
    hdr, swept = c.header(lists)
    assert hdr.shape[1] == 200 and list(hdr[:, 8 + 5]) == [252, 253] and hdr[1, 8] == 1 and list(swept) == [False, True]
