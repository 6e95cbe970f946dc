"""Content-adaptive gain maps, the part that needs no GPU: the yardstick (tests/adaptive_cases.py) against the oracle at the
reference's constants, the range rule and the metadata of the two host entry points, the call-level errors of the device entry
points, the XMP round trip of an adaptive range, and what the adaptive range buys on graded content."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import adaptive_cases as A

F = np.float32
W, H = 128, 64


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api
    api.load()
    return api


@pytest.fixture(scope="module")
def pairs(orc):
    """(p010, yuv) of the LCG pair seed 7 and of the graded pair, 128 x 64"""
    return {"lcg7": orc.lcg_frame(W, H, 7), "graded": A.graded_pair(orc, W, H)}


@pytest.fixture(scope="module")
def lum(orc, pairs):
    """luminances of every (content, tf) the tests below use, 709 / 2100, computed once"""
    out = {}
    for name, (p010, yuv) in pairs.items():
        for tf in (A.TF_HLG, A.TF_PQ):
            out[name, tf] = A.luminances(orc, orc.yuv420_image(yuv, W, H, A.CG_709), orc.p010_image(p010, W, H, A.CG_2100), tf)
    return out


@pytest.mark.parametrize("tf", [A.TF_HLG, A.TF_PQ])
@pytest.mark.parametrize("hdr_gamut", [A.CG_709, A.CG_2100])
def test_helper_equals_the_oracle_at_the_constants(orc, pairs, tf, hdr_gamut):
    p010, yuv = pairs["lcg7"]
    yi, pi = orc.yuv420_image(yuv, W, H, A.CG_709), orc.p010_image(p010, W, H, hdr_gamut)
    st, want, md, mm = orc.generate("orc_", yi, pi, tf, stats=True)
    assert st == 0
    ys, yh = A.luminances(orc, yi, pi, tf)
    assert np.array_equal(A.encode(orc, ys, yh, md.minContentBoost, md.maxContentBoost), want)
    g0, g1 = A.minmax(ys, yh)
    assert (F(mm[0]).tobytes(), F(mm[1]).tobytes()) == (g0.tobytes(), g1.tobytes())


def _range(api, tf, g0, g1):
    lo, hi = C.c_float(), C.c_float()
    rc = api.load().uhdr_hip_adaptive_boost_range(tf, g0, g1, C.byref(lo), C.byref(hi))
    return rc, F(lo.value), F(hi.value)


def test_range_rule_and_metadata(api, lum):
    lib = api.load()
    cases = [(tf, *A.minmax(*lum[name, tf])) for name in ("lcg7", "graded") for tf in (A.TF_HLG, A.TF_PQ)]
    for tf in (A.TF_LINEAR, A.TF_HLG, A.TF_PQ):
        cases += [(tf, F(0), F(1e6)), (tf, F(1.63), F(2.40)), (tf, F(3), F(3)), (tf, F(0.3), F(0.9)), (tf, F(-2), F(2)), (tf, F(np.nan), F(2)),
                  (tf, F(np.inf), F(-np.inf))]
    for tf, g0, g1 in cases:
        rc, lo, hi = _range(api, tf, g0, g1)
        wlo, whi = A.rule(tf, g0, g1)
        assert rc == 0 and (lo.tobytes(), hi.tobytes()) == (wlo.tobytes(), whi.tobytes()), (tf, g0, g1, lo, hi)
        assert lo <= 1 < hi and lo >= F(0.25) and hi <= A.cap(tf)
        md = api.Metadata()
        assert lib.uhdr_hip_adaptive_metadata(tf, g0, g1, C.byref(md)) == 0
        assert A.metadata_tuple(md) == (b"1.0", float(whi), float(wlo), 1.0, 0.0, 0.0, float(wlo), float(whi))
    assert _range(api, A.TF_HLG, F(1.63), F(2.40))[1:] == (F(1), F(2.40))
    assert _range(api, A.TF_HLG, F(0.3), F(0.9))[1:] == (F(0.3), F(1.0625))
    assert _range(api, A.TF_HLG, F(0), F(1e6))[1:] == (F(0.25), F(1000) / F(203)) and _range(api, A.TF_PQ, F(0), F(1e6))[2] == F(10000) / F(203)
    assert _range(api, A.TF_PQ, F(np.nan), F(2))[1] == F(0.25) and _range(api, A.TF_PQ, F(-2), F(2))[1] == F(0.25)
    # the graded pair's ranges as the issue measured them
    for tf, want in ((A.TF_HLG, (1.0, 2.40)), (A.TF_PQ, (0.385, 6.25))):
        _, lo, hi = _range(api, tf, *A.minmax(*lum["graded", tf]))
        assert abs(lo - want[0]) < 0.005 and abs(hi - want[1]) < 0.005, (tf, lo, hi)


def test_status_values(api):
    lib = api.load()
    lo, hi, md, n = C.c_float(), C.c_float(), api.Metadata(), C.c_size_t(77)
    for tf in (3, -1, 7):   # SRGB and values outside the enum: what generate refuses
        assert lib.uhdr_hip_adaptive_boost_range(tf, 1.0, 2.0, C.byref(lo), C.byref(hi)) == api.ERROR_INVALID_TRANS_FUNC
        assert lib.uhdr_hip_adaptive_metadata(tf, 1.0, 2.0, C.byref(md)) == api.ERROR_INVALID_TRANS_FUNC
    assert lib.uhdr_hip_adaptive_boost_range(1, 1.0, 2.0, None, C.byref(hi)) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_adaptive_boost_range(1, 1.0, 2.0, C.byref(lo), None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_adaptive_metadata(1, 1.0, 2.0, None) == api.ERROR_BAD_PTR
    # the device entry points' call-level errors come before the device is looked at
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    yi, pi, d = api.yuv420_image(p, 16, 8, api.CG_BT709), api.p010_image(p, 16, 8, api.CG_BT2100), api.out_image(p)
    gen = lambda n_, y, q, tf, dst, scope, rng, ws, nb: lib.uhdr_hip_generate_gainmap_adaptive_batch(
        n_, y, q, tf, dst, 0, scope, None, rng, ws, nb, None)
    assert lib.uhdr_hip_generate_adaptive_workspace_bytes(0, None, C.byref(n)) == 0 and n.value == 0
    assert lib.uhdr_hip_generate_adaptive_workspace_bytes(1, None, C.byref(n)) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_generate_adaptive_workspace_bytes(1, C.byref(yi), None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_generate_adaptive_workspace_bytes(1, C.byref(yi), C.byref(n)) == 0 and n.value >= 4 * 4 * 2 + 8
    assert api.adaptive_workspace_bytes([yi]) == n.value
    assert gen(1, None, C.byref(pi), 1, C.byref(d), 0, p, p, 1 << 20) == api.ERROR_BAD_PTR
    assert gen(-1, C.byref(yi), C.byref(pi), 1, C.byref(d), 0, p, p, 1 << 20) == api.ERROR_BAD_PTR
    assert gen(1, C.byref(yi), C.byref(pi), 3, C.byref(d), 0, p, p, 1 << 20) == api.ERROR_INVALID_TRANS_FUNC
    assert gen(1, C.byref(yi), C.byref(pi), 1, C.byref(d), 2, p, p, 1 << 20) == api.ERROR_UNSUPPORTED_FEATURE
    assert gen(1, C.byref(yi), C.byref(pi), 1, C.byref(d), -1, None, None, 0) == api.ERROR_UNSUPPORTED_FEATURE   # the scope before the pointers
    assert gen(1, C.byref(yi), C.byref(pi), 1, C.byref(d), 1, None, p, 1 << 20) == api.ERROR_BAD_PTR
    assert gen(1, C.byref(yi), C.byref(pi), 1, C.byref(d), 1, p, None, 1 << 20) == api.ERROR_BAD_PTR
    assert gen(1, C.byref(yi), C.byref(pi), 1, C.byref(d), 0, p, p, n.value - 1) == api.ERROR_INSUFFICIENT_RESOURCE
    assert gen(0, None, None, 1, None, 0, None, None, 0) == 0
    assert not buf.any()
    # the file-level call: its call-level errors in the existing batch's order, then the scope
    outs, caps, sizes = (C.c_void_p * 1)(p), (C.c_size_t * 1)(4096), (C.c_size_t * 1)(0)
    enc = lambda n_, pp, q, scope, o=outs: lib.uhdr_hip_jpegr_encode_adaptive_batch(n_, pp, None, 1, q, None, None, o, caps, sizes, None, None, scope,
                                                                                   api.MEM_HOST, None)
    assert enc(1, None, 90, 0) == api.ERROR_BAD_PTR and enc(-1, C.byref(pi), 90, 0) == api.ERROR_BAD_PTR
    assert enc(1, C.byref(pi), 90, 0, None) == api.ERROR_BAD_PTR
    assert enc(1, C.byref(pi), 101, 7) == api.ERROR_INVALID_QUALITY_FACTOR
    assert enc(1, C.byref(pi), 90, 7) == api.ERROR_UNSUPPORTED_FEATURE and enc(1, C.byref(pi), 90, -1) == api.ERROR_UNSUPPORTED_FEATURE
    assert enc(0, None, 90, 1, None) == 0
    assert (api.BOOST_PER_IMAGE, api.BOOST_PER_CALL) == (0, 1)


def test_xmp_round_trip_of_an_adaptive_range(orc, api, lum):
    lib = api.load()
    for tf, g0, g1 in [(tf, *A.minmax(*lum[name, tf])) for name in ("lcg7", "graded") for tf in (A.TF_HLG, A.TF_PQ)] + [(A.TF_PQ, F(0.3), F(0.9))]:
        md = api.Metadata()
        assert lib.uhdr_hip_adaptive_metadata(tf, g0, g1, C.byref(md)) == 0
        got = A.xmp_round_trip(orc, api, md)
        assert got.version == b"1.0" and (got.gamma, got.offsetSdr, got.offsetHdr) == (1.0, 0.0, 0.0)
        # the packet stores log2 of the boosts with %g (six significant digits), hdrCapacity likewise
        for f in ("maxContentBoost", "minContentBoost", "hdrCapacityMin", "hdrCapacityMax"):
            assert abs(math.log2(getattr(got, f)) - math.log2(getattr(md, f))) <= 5.1e-6 * max(1.0, abs(math.log2(getattr(md, f)))), f
        assert got.minContentBoost <= 1.0 < got.maxContentBoost


@pytest.mark.parametrize("tf", [A.TF_HLG, A.TF_PQ])
def test_adaptive_range_recovers_graded_content_better(orc, lum, tf):
    ys, yh = lum["graded", tf]
    g = A.gains(ys, yh)
    lo, hi = A.rule(tf, g.min(), g.max())
    const = A.recovery_error(A.encode(orc, ys, yh, F(1), A.cap(tf)), F(1), A.cap(tf), g)
    adapt = A.recovery_error(A.encode(orc, ys, yh, lo, hi), lo, hi, g)
    print("tf %d: mean |log2 error| constant %.5f (max %.3f), adaptive %.5f (max %.3f), range [%.3f, %.3f]" % (tf, *const, *adapt, lo, hi))
    assert adapt[0] < const[0]


def test_adaptive_metadata_is_what_the_map_was_encoded_against(orc, api, lum):
    """uhdr_hip_adaptive_metadata on the measured pair names the range under which the helper's map decodes best: the link between
    the two host calls and the map bytes"""
    ys, yh = lum["lcg7", A.TF_PQ]
    g0, g1 = A.minmax(ys, yh)
    md = api.Metadata()
    assert api.load().uhdr_hip_adaptive_metadata(A.TF_PQ, g0, g1, C.byref(md)) == 0
    gmap = A.encode(orc, ys, yh, md.minContentBoost, md.maxContentBoost)
    assert gmap.min() == 0 and gmap.max() in (254, 255)   # both clamps are reached (the LCG pair's gains span 0.195 .. 100)
