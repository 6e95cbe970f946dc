"""The tone-mapped SDR base image, the part that needs no GPU: uhdr_hip_tonemap_headroom against the model's H bit for bit, the
model's own properties (tests/tonemap_cases.py), the share of samples the GPU tests leave in doubt on every input they use, and the
argument checks of the new calls that return before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from tests import tonemap_cases as T

F = np.float32
TFS = (T.TF_HLG, T.TF_PQ, T.TF_LINEAR)


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api
    api.load()
    return api


def _headroom(api, tf, gamma_max, peak):
    h = C.c_float(-1.0)
    rc = api.load().uhdr_hip_tonemap_headroom(tf, F(gamma_max), F(peak), C.byref(h))
    return rc, F(h.value)


@pytest.mark.parametrize("tf", TFS)
def test_headroom_equals_the_model_bit_for_bit(api, tf):
    # measured: 0, 1, the junctions of the transfer functions, values whose H clamps to 1 and to the cap, and a sweep between them
    sweep = [0.0, 1.0, 0.0001, 0.00011, 0.05, 0.3, 0.5, 0.50000006, 0.58, 0.75, 0.9, 0.99999994] + list(np.linspace(0.0, 1.0, 257, dtype=F))
    seen = set()
    for g in sweep:
        rc, h = _headroom(api, tf, g, 0.0)
        want = T.headroom(tf, F(g))
        assert rc == 0 and h.tobytes() == F(want).tobytes(), (tf, g, h, want)
        seen.add(float(h))
    k = float(T.k_of(tf))
    assert min(seen) == 1.0 and max(seen) == k and len(seen) > 50   # both clamps and the range between them
    # given: below 203 nits (H = 1), inside, above white (H = cap); gamma_max is ignored
    for peak in (1.0, 100.0, 203.0, 204.0, 600.0, 999.0, 1000.0, 4000.0, 10000.0, 20000.0, 3.0e38):
        rc, h = _headroom(api, tf, 0.123, peak)
        want = T.headroom(tf, F(0.9), peak)
        assert rc == 0 and h.tobytes() == F(want).tobytes(), (tf, peak, h, want)
        assert 1.0 <= h <= k
    assert _headroom(api, tf, 0.123, 100.0)[1] == 1.0 and _headroom(api, tf, 0.123, 20000.0)[1] == F(k)
    # a peak of 0 measures; negative and non-finite ones are refused and nothing is written
    assert _headroom(api, tf, 0.75, 0.0)[1].tobytes() == F(T.headroom(tf, F(0.75))).tobytes()
    for bad in (-1.0, -0.0001, float("nan"), float("inf"), float("-inf")):
        assert _headroom(api, tf, 0.5, bad) == (api.ERROR_UNSUPPORTED_FEATURE, F(-1.0)), bad


def test_headroom_argument_checks(api):
    lib = api.load()
    h = C.c_float()
    assert lib.uhdr_hip_tonemap_headroom(T.TF_HLG, 0.5, 0.0, None) == api.ERROR_BAD_PTR
    for tf in (-1, 3, 7):
        assert lib.uhdr_hip_tonemap_headroom(tf, 0.5, 0.0, C.byref(h)) == api.ERROR_INVALID_TRANS_FUNC
    assert api.tonemap_headroom(T.TF_PQ, 1.0) == float(T.k_of(T.TF_PQ))
    assert (api.TONEMAP_SHIFT, api.TONEMAP_REINHARD_MAXRGB) == (0, 1)


@pytest.mark.parametrize("tf", [T.TF_HLG, T.TF_PQ])
def test_content_at_or_below_sdr_white_is_only_srgb_encoded(tf):
    """linear content <= 203 nits: H == 1, step 5 is the identity, the planes are the plain sRGB encoding of the input"""
    luma, chroma = T.ramp_planes(64, 32)
    top = 670 if tf == T.TF_HLG else 568   # just below 203 nits: HLG signal 0.697 (0.203 of 1000 nits), PQ signal 0.58
    luma = ((64 + ((luma >> 6).astype(np.int64) - 64) * (top - 64) // 876).astype(np.uint16) << 6).astype(np.uint16)
    chroma[:] = 512 << 6
    a = T.model(luma, chroma, T.CG_709, tf)
    assert a["H"] == F(1.0) and float(T.inv_oetf(tf, np.array([a["m"]], F))[0]) * float(T.k_of(tf)) <= 1.0
    b = T.model(luma, chroma, T.CG_709, tf, identity=True)
    for p in ("Y", "U", "V"):
        assert np.array_equal(a[p], b[p])
    assert np.allclose(a["vy"], b["vy"], rtol=0, atol=1e-9) and a["Y"].max() > 240   # the ramp's top is close to SDR white


@pytest.mark.parametrize("tf", TFS)
def test_a_grey_ramp_maps_monotonically_and_the_peak_maps_to_one(tf):
    luma, chroma = T.ramp_planes(256, 4, grey=True)
    a = T.model(luma, chroma, T.CG_2100, tf)
    row = a["Y"][0].astype(np.int32)
    assert (np.diff(row) >= 0).all() and row[0] == 0 and row[-1] == 255 and len(np.unique(row)) > 100
    assert (np.abs(a["U"].astype(np.int32) - 128) <= 1).all() and (np.abs(a["V"].astype(np.int32) - 128) <= 1).all()
    assert float(T.k_of(tf)) >= a["H"] > 1.0
    # the brightest pixel lands on o == 1 (H is rounded to f32 once, v is not: 1e-6 covers that)
    o = a["o"]
    assert abs(o[0, -1].max() - 1.0) < 1e-6 and o.max() <= 1.0
    # a dimmer ramp (signal up to 0.75): a given peak above the content's leaves headroom unused, one below it clips
    dim = ((64 + ((luma >> 6).astype(np.int64) - 64) * 3 // 4).astype(np.uint16) << 6).astype(np.uint16)
    d = T.model(dim, chroma, T.CG_2100, tf)
    assert 1.25 * 1.25 < d["H"] * F(1.25) < T.k_of(tf) and abs(d["o"].max() - 1.0) < 1e-6
    hi = T.model(dim, chroma, T.CG_2100, tf, peak_nits=float(d["H"]) * 203.0 * 1.25)
    assert hi["H"] > d["H"] and hi["o"].max() < 1.0 - 1e-3
    lo = T.model(dim, chroma, T.CG_2100, tf, peak_nits=float(d["H"]) * 203.0 / 1.25)
    assert lo["H"] < d["H"] and (lo["o"].max(axis=2) == 1.0).sum() > 1


def test_the_doubt_band_excludes_little_of_every_gpu_input():
    """what tests/test_gpu_tonemap.py may excuse: at most 3 % of each plane's samples, on every input it uses"""
    worst = 0.0
    for case in T.cases():
        want = T.expected(case)
        for v in ("vy", "vu", "vv"):
            share = float(T.in_doubt(want[v]).mean())
            worst = max(worst, share)
            assert share <= 0.03, (case, v, share)
    assert worst > 0.0   # (the band is not empty: 2 / 256 of uniformly spread values fall into it)


def test_model_headroom_of_the_gpu_inputs_spans_the_rule():
    hs = {c.name: float(T.expected(c)["H"]) for c in T.cases()}
    assert any(h == float(T.k_of(T.TF_LINEAR)) for n, h in hs.items() if "-lin-" in n)   # linear noise reaches the cap
    assert any(1.0 < h < float(T.k_of(T.TF_PQ)) for n, h in hs.items() if "-pq-" in n)
    # the large frame: one pixel, in a block row beyond the measuring pass's 512 workgroup rows, decides m' and H
    for c in (c for c in T.cases() if c.content == "lcg_tiled"):
        flat = T.model(*T.planes("lcg_tiled_flat", c.w, c.h), c.gamut, c.tf)
        want = T.expected(c)
        assert want["m"] > flat["m"] and T.k_of(c.tf) > want["H"] > flat["H"] and T.peak_xy(c.w, c.h)[1] // 2 >= 512, c


def test_argument_checks_that_need_no_device(api):
    lib = api.load()
    buf = np.zeros(64 * 64 * 3, np.uint8)
    p = api.p010_image(buf.ctypes.data, 8, 8, api.CG_BT2100)
    d = api.yuv420_image(buf.ctypes.data, 8, 8, api.CG_UNSPECIFIED)
    h = (C.c_float * 2)()
    batch = lambda n, ps, ds, tf, op, peaks, head: lib.uhdr_hip_tonemap_sdr_batch(n, ps, ds, tf, op, peaks, head, None)
    one = C.c_float * 1
    assert batch(-1, C.byref(p), C.byref(d), api.TF_HLG, 1, None, h) == api.ERROR_BAD_PTR
    assert batch(1, None, C.byref(d), api.TF_HLG, 1, None, h) == api.ERROR_BAD_PTR
    assert batch(1, C.byref(p), None, api.TF_HLG, 1, None, h) == api.ERROR_BAD_PTR
    d2 = api.yuv420_image(buf.ctypes.data, 16, 8, api.CG_UNSPECIFIED)
    assert batch(1, C.byref(p), C.byref(d2), api.TF_HLG, 1, None, h) == api.ERROR_RESOLUTION_MISMATCH
    p0 = api.p010_image(buf.ctypes.data, 8, 8, api.CG_BT2100)
    p0.data = None
    assert batch(1, C.byref(p0), C.byref(d), api.TF_HLG, 1, None, h) == api.ERROR_BAD_PTR
    for tf in (api.TF_SRGB, -1, 9):
        assert batch(1, C.byref(p), C.byref(d), tf, 1, None, h) == api.ERROR_INVALID_TRANS_FUNC
        assert batch(1, C.byref(p), C.byref(d), tf, 7, None, h) == api.ERROR_INVALID_TRANS_FUNC   # the transfer function comes first
    for op in (-1, 2, 99):
        assert batch(1, C.byref(p), C.byref(d), api.TF_PQ, op, None, h) == api.ERROR_UNSUPPORTED_FEATURE
    for bad in (-5.0, float("nan"), float("inf")):
        assert batch(1, C.byref(p), C.byref(d), api.TF_PQ, 1, one(bad), h) == api.ERROR_UNSUPPORTED_FEATURE
    assert batch(1, C.byref(p), C.byref(d), api.TF_PQ, 1, None, None) == api.ERROR_BAD_PTR
    odd = api.p010_image(buf.ctypes.data, 9, 8, api.CG_BT2100, luma_stride=10)
    dodd = api.yuv420_image(buf.ctypes.data, 9, 8, api.CG_UNSPECIFIED, luma_stride=10)
    assert batch(1, C.byref(odd), C.byref(dodd), api.TF_PQ, 1, None, h) == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT
    pg = api.p010_image(buf.ctypes.data, 8, 8, api.CG_UNSPECIFIED)
    assert batch(1, C.byref(pg), C.byref(d), api.TF_PQ, 1, None, h) == api.ERROR_INVALID_COLORGAMUT
    ds = api.yuv420_image(buf.ctypes.data, 8, 8, api.CG_UNSPECIFIED, luma_stride=8, chroma_stride=3)
    assert batch(1, C.byref(p), C.byref(ds), api.TF_PQ, 1, None, h) == api.ERROR_INVALID_STRIDE
    assert not buf.any() and h[0] == 0.0   # nothing was written
    # the single call: the same order
    single = lambda ps, ds, tf, op, peak: lib.uhdr_hip_tonemap_sdr(ps, ds, tf, op, peak, h, api.MEM_HOST, None)
    assert single(None, C.byref(d), api.TF_HLG, 1, 0.0) == api.ERROR_BAD_PTR
    assert single(C.byref(p), C.byref(d2), api.TF_HLG, 1, 0.0) == api.ERROR_RESOLUTION_MISMATCH
    assert single(C.byref(p), C.byref(d), api.TF_SRGB, 1, 0.0) == api.ERROR_INVALID_TRANS_FUNC
    assert single(C.byref(p), C.byref(d), api.TF_HLG, 5, 0.0) == api.ERROR_UNSUPPORTED_FEATURE
    assert single(C.byref(p), C.byref(d), api.TF_HLG, 1, -1.0) == api.ERROR_UNSUPPORTED_FEATURE
    assert single(C.byref(odd), C.byref(dodd), api.TF_HLG, 1, 0.0) == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT
    # the encode call: the batch's call-level checks, then the operator and the scope
    out, cap, n = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(buf.size), (C.c_size_t * 1)()
    enc = lambda cnt, quality, op, scope, outs=out: lib.uhdr_hip_jpegr_encode_api0_tonemapped_batch(
        cnt, C.byref(p), api.TF_HLG, quality, None, None, outs, cap, n, None, None, op, None, scope, api.MEM_HOST, None)
    assert enc(-1, 90, 1, -1) == api.ERROR_BAD_PTR
    assert enc(1, 90, 1, -1, None) == api.ERROR_BAD_PTR
    assert enc(1, 101, 1, -1) == api.ERROR_INVALID_QUALITY_FACTOR
    assert enc(1, 90, 3, -1) == api.ERROR_UNSUPPORTED_FEATURE
    assert enc(1, 90, 1, 2) == api.ERROR_UNSUPPORTED_FEATURE and enc(1, 90, 1, -2) == api.ERROR_UNSUPPORTED_FEATURE
    assert enc(0, 90, 1, -1) == api.NO_ERROR and enc(0, 90, 0, api.BOOST_PER_CALL) == api.NO_ERROR
    # per file, with no device in reach: a file that fails its checks is reported and not processed
    st = (C.c_int * 1)(1)
    peaks = one(float("nan"))
    rc = lib.uhdr_hip_jpegr_encode_api0_tonemapped_batch(1, C.byref(p), api.TF_HLG, 90, None, None, out, cap, n, None, st, 1, peaks, -1, api.MEM_HOST, None)
    assert (rc, st[0]) == (api.ERROR_UNSUPPORTED_FEATURE, api.ERROR_UNSUPPORTED_FEATURE)
    st[0] = 1
    rc = lib.uhdr_hip_jpegr_encode_api0_tonemapped_batch(1, C.byref(odd), api.TF_HLG, 90, None, None, out, cap, n, None, st, 1, None, -1, api.MEM_HOST, None)
    assert st[0] == api.ERROR_UNSUPPORTED_WIDTH_HEIGHT
    assert not buf.any()
