"""CPU tests of what tests/test_gpu_apply_doubt_lists.py stands on: the cases of tests/apply_doubt_cases.py -- every case's facts,
with the constants of the hand-over restated here -- and phase 0 of uhdr_hip_apply_exact_probe: the route an EXACT apply call takes
and the statuses of the probe.  Phase 0 is host arithmetic over the descriptors: no device, and the data pointers are never read."""
import ctypes as C

import numpy as np
import pytest

from tests import apply_doubt_cases as K

LISTS, HDR_WORDS, COUNTS_AT, SLICE_WORD, SLICES = 1024, 1032, 8, 3, 256


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _descriptors(api, w, h, scale, n, base=0x10000000, step=None):
    fb = (w * h * 8 + 4095) // 4096 * 4096 if step is None else step
    ya = api.image_array([api.yuv420_image(base + i * fb, w, h, api.CG_BT709) for i in range(n)])
    ma = api.image_array([api.mono_image(base + (n + i) * fb, w // scale, h // scale) for i in range(n)])
    da = api.image_array([api.out_image(base + (2 * n + i) * fb) for i in range(n)])
    return ya, ma, da


def _route(api, w, h, scale, n=1, fmt=3, boost=K.FLT_MAX, md=None, **kw):
    ya, ma, da = _descriptors(api, w, h, scale, n, **kw)
    md = api.metadata(K.MAX_BOOST) if md is None else md
    r = (C.c_uint32 * api.APPLY_ROUTE_WORDS)()
    assert api.load().uhdr_hip_apply_exact_probe(0, n, ya, ma, C.byref(md), fmt, boost, da, None, r, None) == 0
    assert (da[0].width, da[0].height) == (w, h)            # the destination descriptors are filled as by the call itself
    return dict(zip(K.ROUTE_KEYS, list(r)))


def test_route_constants(api):
    assert len(K.ROUTE_KEYS) == api.APPLY_ROUTE_WORDS == 11
    r = _route(api, 256, 64, 4)
    assert (r["lists"], r["hdr_words"], r["list_counts"], r["slice_word"], r["resolve_slices"]) == (LISTS, HDR_WORDS, COUNTS_AT, SLICE_WORD, SLICES)
    assert K.TRIP == SLICES * 256 == 65536 and r["list_counts"] + r["lists"] == r["hdr_words"]


@pytest.mark.parametrize("name", K.ALL + ("reuse_large",))
def test_phase_0_reports_the_route_the_case_assumes(api, name):
    c = K.case(name)
    for fmt in K.FORMATS:
        assert _route(api, c.w, c.h, c.scale, c.n, fmt) == c.route(), (name, fmt)
    assert c.route()["list_cap"] == c.w * c.h // 16384 + 64


def test_route_on_both_sides_of_its_conditions(api):
    pick = lambda r: (r["resolve"], r["cells"], r["images"], r["list_cap"], r["grid_x"], r["grid_y"])
    assert pick(_route(api, 256, 64, 4)) == (1, 1, 1, 65, 4, 1)
    assert pick(_route(api, 256, 64, 4, n=5)) == (1, 1, 5, 65, 4, 5)
    assert pick(_route(api, 256, 64, 2)) == (1, 0, 1, 65, 1, 64)
    assert pick(_route(api, 258, 64, 2, n=3)) == (1, 0, 3, 65, 2, 64)              # one pixel past a block of 256
    assert pick(_route(api, 8, 65540, 2)) == (1, 0, 1, 96, 1, 65535)               # rows beyond the grid are reached by striding
    assert pick(_route(api, 256, 64, 4, base=0x10000004)) == (1, 0, 1, 65, 1, 64)  # a destination off 16 bytes: the per-pixel kernel
    assert pick(_route(api, 4096, 1028, 4)) == (1, 1, 1, 321, 1028, 1)
    assert pick(_route(api, 256, 64, 4, n=70)) == (1, 1, 64, 65, 4, 64)            # the first chunk
    # OUTPUT_SDR writes nothing; boosts beyond the range the estimate was measured for run unfiltered
    assert pick(_route(api, 256, 64, 4, fmt=api.OUTPUT_SDR)) == (0, 0, 1, 0, 0, 0)
    assert pick(_route(api, 256, 64, 4, md=api.metadata(2.0 ** 32)))[:2] == (1, 1)
    assert pick(_route(api, 256, 64, 4, md=api.metadata(np.float32(2.0 ** 32 * 1.01))))[:2] == (0, 0)
    assert pick(_route(api, 256, 64, 4, md=api.metadata(4.0, np.float32(2.0 ** -33))))[:2] == (0, 0)


def test_probe_statuses(api):
    """the checks of uhdr_hip_apply_gainmap_batch, in its order, behind the probe's own"""
    lib = api.load()
    w, h = 256, 64
    ya, ma, da = _descriptors(api, w, h, 4, 2)
    md = api.metadata(K.MAX_BOOST)
    r = (C.c_uint32 * api.APPLY_ROUTE_WORDS)()
    probe = lambda phase, n=2, y=ya, m=ma, meta=md, fmt=3, d=da, route=r, hdr=None: lib.uhdr_hip_apply_exact_probe(
        phase, n, y, m, None if meta is None else C.byref(meta), fmt, K.FLT_MAX, d, None, route, hdr)
    assert probe(0) == 0
    assert probe(-1) == api.ERROR_UNSUPPORTED_FEATURE and probe(3) == api.ERROR_UNSUPPORTED_FEATURE
    assert probe(0, n=0) == api.ERROR_BAD_PTR and probe(0, n=-1) == api.ERROR_BAD_PTR
    assert probe(0, route=None) == api.ERROR_BAD_PTR
    assert probe(1, hdr=None) == api.ERROR_BAD_PTR
    assert probe(0, y=None) == api.ERROR_BAD_PTR and probe(0, m=None) == api.ERROR_BAD_PTR and probe(0, d=None) == api.ERROR_BAD_PTR
    assert probe(0, meta=None) == api.ERROR_BAD_PTR
    bad = api.metadata(K.MAX_BOOST)
    bad.gamma = 2.0
    assert probe(0, meta=bad) == api.ERROR_BAD_METADATA
    odd = api.image_array([ma[0], api.mono_image(0x30000000, 60, 16)])
    assert probe(0, m=odd) == api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR
    assert probe(0, m=odd, meta=bad) == api.ERROR_BAD_METADATA                     # metadata before the scale factor
    nod = api.image_array([da[0], api.out_image(None)])
    assert probe(0, d=nod) == api.ERROR_BAD_PTR
    assert probe(0, d=nod, fmt=api.OUTPUT_SDR) == 0                                # a format that writes nothing needs no destination
    import torch
    if not torch.cuda.is_available():   # phases 1 and 2 need the device: refused behind the argument checks, nothing computed
        assert probe(1, hdr=C.c_void_p(0x40000000)) == api.ERROR_INSUFFICIENT_RESOURCE
        assert probe(2) == api.ERROR_INSUFFICIENT_RESOURCE
        assert probe(2, meta=bad) == api.ERROR_BAD_METADATA


# ---- the cases' facts, constants restated ------------------------------------------------------------------------------------
def _facts(name):
    c = K.case(name)
    return c, c.facts(c.route())


def test_levels_and_poison():
    assert K.levels(1) == (1, 0, 0) and all(K.levels(f) == (255, 0, 255) for f in (2, 3, 4)) and K.POISON == 0xCD
    lin = (1.0 / 255.0 / 12.92) / 4.0
    assert 0.0 < lin < 2.0 ** -13 and 1.0 / 255.0 <= 0.04045                      # the F16 level: the sRGB toe, a half-precision subnormal's range
    c = K.case("at_cap")
    yuv, gmap = c.frames(1)
    assert set(np.unique(yuv[0, :c.w * c.h])) == {0, 1} and (yuv[0, c.w * c.h:] == 128).all() and (gmap == 0).all()
    yuv, gmap = c.frames(3)
    assert set(np.unique(yuv[0, :c.w * c.h])) == {0, 255} and (gmap == 255).all() and gmap.shape == (16, 64)
    assert np.array_equal(yuv[0, :c.w * c.h].reshape(c.h, c.w) == 255, c.masks[0])


def test_capacity_cases():
    for name, longest, sweep, total in (("at_cap", 65, False, 130), ("cap_plus_one", 66, True, 131), ("empty", 0, False, 0), ("last_only", 1, False, 1)):
        c, (f,) = _facts(name)
        assert (c.w, c.h, c.scale, c.route()["list_cap"], c.route()["grid_x"]) == (256, 64, 4, 65, 4)
        assert (f["longest"], f["sweep"], f["total"], f["shared"], f["appends"]) == (longest, sweep, total, 0, 4), name
        assert int(c.masks.sum()) == total
    c, _ = _facts("at_cap")
    assert list(c.counts(c.route())[0, :5]) == [65, 0, 1, 64, 0]
    c, _ = _facts("cap_plus_one")
    assert list(c.counts(c.route())[0, :5]) == [66, 0, 1, 64, 0]
    c, _ = _facts("last_only")
    assert c.masks[0, 63, 255] and list(c.counts(c.route())[0, :5]) == [0, 0, 0, 1, 0]      # the last block's last cell


def test_mixed_batch():
    c, f = _facts("mixed_batch")
    assert c.n == 4 and c.route()["images"] == 4 and c.route()["grid_y"] == 4
    assert [x["sweep"] for x in f] == [False, True, False, False] and [x["longest"] for x in f] == [65, 66, 1, 0]
    for i, name in enumerate(("at_cap", "cap_plus_one", "last_only", "empty")):
        assert np.array_equal(c.masks[i], K.case(name).masks[0])


def test_per_pixel_cases():
    c, (f,) = _facts("px_shared")
    r = c.route()
    assert (c.scale, r["cells"], r["grid_x"], r["grid_y"], r["list_cap"]) == (2, 0, 2, 514, 80) and c.w > 256 and c.h * r["grid_x"] == 1028 > LISTS
    cnt = c.counts(r)[0]
    assert (f["longest"], f["sweep"], f["shared"]) == (80, False, 2) and cnt[1] == 80 and cnt[3] == 5 and cnt[1023] == 1
    assert c.masks[0, 0, 256:].sum() == 50 and c.masks[0, 512, 256:].sum() == 30           # list 1 = (row 0, block 1) + (row 512, block 1)
    assert sorted(cnt[cnt > 0]) == [1, 5, 7, 79, 80, 80, 80]                               # three lists at ex_cap, one of them shared
    c2, (f2,) = _facts("px_overflow")
    assert (f2["longest"], f2["sweep"]) == (81, True) and c2.counts(r)[0, 1] == 81 and (c2.masks ^ c.masks).sum() == 1
    assert c2.masks[0, 512, 256:].sum() == 31
    c3, (f3,) = _facts("px_ragged")
    r3 = c3.route()
    assert (c3.scale, c3.w % 256, r3["grid_x"], r3["list_cap"], r3["cells"]) == (3, 74, 2, 64, 0)
    assert (f3["longest"], f3["sweep"], f3["total"], f3["shared"]) == (64, False, 200, 0)
    assert c3.masks[0, 0, 329] and c3.masks[0, 23, 256:].sum() == 60 and c3.masks[0, :, 256:].sum() == 125   # the partial block, its last pixel


def test_depth_and_wrap_cases():
    c, (f,) = _facts("second_trip")
    r = c.route()
    assert (c.w, c.h, c.scale, r["list_cap"], r["grid_x"], f["appends"]) == (1024, 512, 2, 96, 4, 2048)
    assert (f["total"], f["longest"], f["used"], f["shared"], f["sweep"]) == (81920, 80, 1024, 1024, False) and f["total"] > K.TRIP
    assert (c.counts(r)[0] == 80).all()
    c, (f,) = _facts("s4_wrap")
    r = c.route()
    assert (c.w, c.h, c.scale, r["list_cap"], r["grid_x"], r["cells"]) == (4096, 1028, 4, 321, 1028, 1)
    cnt = c.counts(r)[0]
    assert list(cnt[:4]) == [321, 15, 1, 321] and cnt[515] == 321 and cnt[1023] == 33 and f["shared"] == 3 and not f["sweep"]
    assert c.appends(r)[0, 1024] == 121 and c.appends(r)[0, 0] == 200 and c.appends(r)[0, 1027] == 21
    assert c.masks[0, 1024:].sum() == 121 + 5 + 1 + 21                                     # blocks 1024 .. 1027 are the map's last row
    c2, (f2,) = _facts("s4_wrap_overflow")
    assert c2.counts(r)[0, 0] == 322 and f2["sweep"] and (c2.masks ^ c.masks).sum() == 1
    c, (f,) = _facts("reuse_large")
    assert (c.route()["list_cap"], f["longest"], f["sweep"], c.route()["grid_x"]) == (96, 96, False, 128)


@pytest.mark.parametrize("kind,shape,cap", [("s4", (4096, 1024, 4), 320), ("px", (256, 1024, 2), 80)])
def test_accumulating_cases(api, kind, shape, cap):
    """a: image 0's LAST list at exactly ex_cap, image 1's FIRST list one pixel; b: one pixel more for that last list and nothing
    else; u: their union.  The two lists are neighbours in the workspace: entry ex_cap of image 0's list 1023 would be slot 0 of
    image 1's list 0"""
    a, b, u = (K.case("acc_%s_%s" % (kind, part)) for part in "abu")
    r = a.route()
    assert (a.w, a.h, a.scale) == shape and a.n == 2 and r == b.route() == u.route() == _route(api, *shape, n=2)
    assert (r["list_cap"], r["cells"], r["images"]) == (cap, int(kind == "s4"), 2) and a.appends(r).shape[1] == 1024 == LISTS
    ca, cb, cu = a.counts(r), b.counts(r), u.counts(r)
    assert ca[0, 1023] == cap and ca[0].sum() == cap and ca[1, 0] == 1 and ca[1].sum() == 1
    assert cb[0, 1023] == 1 and cb.sum() == 1
    assert np.array_equal(ca + cb, cu) and cu[0, 1023] == cap + 1
    assert not (a.masks & b.masks).any() and np.array_equal(a.masks | b.masks, u.masks)
    assert [f["sweep"] for f in u.facts(r)] == [True, False] and not any(f["sweep"] for f in a.facts(r) + b.facts(r))
    assert (0 * LISTS + 1023) * cap + cap == (1 * LISTS + 0) * cap     # list l of image i starts at word (i * lists + l) * ex_cap


# ---- the expected values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", K.FORMATS)
def test_expected_values_by_class_are_the_oracle_on_whole_frames(orc, fmt):
    """the look-up the large cases take their expected pixels from equals the oracle on a whole frame, at scale 4 (interior cells,
    the last column, the last row) and at the per-pixel scales; and no expected pixel is the poison pattern"""
    for name in ("at_cap", "last_only", "px_ragged"):
        c = K.case(name)
        whole = K.expect(name, fmt)
        assert whole.shape[:3] == (c.n, c.h, c.w)
        assert np.array_equal(K.expect_by_class(c, fmt), whole), name
    hi, lo = K.class_table(fmt, 4)[1], K.class_table(fmt, 4)[0]
    assert (lo == lo[0, 0]).all() and not (lo[0, 0] == K.poison_pixel(fmt)).all() and not (hi == K.poison_pixel(fmt)).all(axis=-1).any()
    assert not (hi == lo).all(axis=-1).any()               # a set pixel that lost its entry cannot pass for an unset one
