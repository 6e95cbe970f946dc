"""-m gpu: applyGainMap at map scale factors other than 4 against the oracle's bytes (tests/apply_scale_cases.py; the oracle is pinned
to the reference's object code on these very cases by tests/test_apply_scales_cpu.py).

What runs here is everything that is not the scale-4 walk: px_taps with its shift and its division branch, the four weight tables at
every offset, k_apply_px (FAST, EXACT_UNFILTERED), k_apply_px_est + k_apply_resolve (EXACT), k_apply_lut (LUT), and the weight
table's lease -- kept per device up to factor 128, built for the call and freed behind it above.  Every output lies between 4 KiB of
sentinel bytes that must come back untouched.

Bars: EXACT, EXACT_UNFILTERED and LUT byte-identical to the oracle (LUT: to its LUT pipeline); FAST within tests/test_gpu_parity.py's
LSB_TOL / HALF_ULP_TOL, through its _check_apply."""
import ctypes as C

import numpy as np
import pytest

from tests import apply_scale_cases as A
from tests.test_gpu_apply_walk_tail import GUARD, Guarded
from tests.test_gpu_parity import _check_apply

pytestmark = pytest.mark.gpu
FLT_MAX = A.FLT_MAX


class Inputs:
    """a case's planes and map in device memory, with the descriptors over them"""

    def __init__(self, hip, name, gmap=None):
        from tests.gpu_util import to_dev
        case = A.BY_NAME[name]
        _, self.w, self.h, self.mw, self.mh, chroma = case
        self.name = name
        self.host_planes = A.packed(name)
        self.host_map = np.ascontiguousarray(A.gain_map(name) if gmap is None else gmap)
        self.planes, self.map = to_dev(self.host_planes), to_dev(self.host_map)
        self.img = self.describe(hip, self.planes.data_ptr())
        self.mimg = hip.mono_image(self.map.data_ptr(), self.mw, self.mh)

    def describe(self, hip, ptr):
        chroma = A.BY_NAME[self.name][5]
        if chroma == "420":
            return hip.yuv420_image(ptr, self.w, self.h, hip.CG_BT709)
        fmt = {"444": hip.PIX_FMT_YUV444, "422": hip.PIX_FMT_YUV422, "440": hip.PIX_FMT_YUV440}[chroma]
        return hip.ycbcr_image(ptr, self.w, self.h, hip.CG_BT709, fmt)


def _apply(hip, inp, md, fmt, boost, mode, stream=None):
    """one uhdr_hip_apply_gainmap call into a guarded buffer: the output bytes"""
    from tests.gpu_util import stream_ptr, to_host
    lib = hip.load()
    out = Guarded(A.BPP[fmt] * inp.w * inp.h)
    dest = hip.out_image(out.ptr())
    if stream is not None:
        import torch
        torch.cuda.synchronize()   # the sentinels are filled on the current stream
    rc = lib.uhdr_hip_apply_gainmap(C.byref(inp.img), C.byref(inp.mimg), C.byref(md), fmt, boost, C.byref(dest), mode, hip.MEM_DEVICE,
                                    stream_ptr() if stream is None else stream)
    assert rc == 0, (inp.name, fmt, mode, rc, lib.uhdr_hip_last_error())
    assert (dest.width, dest.height, dest.colorGamut) == (inp.w, inp.h, hip.CG_BT709)
    got = to_host(out.body()).copy()
    assert out.guards_intact(), "%s fmt %d mode %d wrote outside its image" % (inp.name, fmt, mode)
    return got


def _same(got, want, what):
    assert got.size == want.size, what
    assert np.array_equal(got, want), (what, "%d of %d bytes differ, first at %d" % (int((got != want).sum()), got.size, int(np.argmax(got != want))))


def _every_mode(hip, name, fmt, boost, boost_range):
    inp = Inputs(hip, name)
    md = A.api_metadata(hip, boost_range)
    want = A.expected(name, fmt, boost, boost_range)
    # EXACT twice on one stream: the second run finds the list headers as the first one left them
    for run in (1, 2):
        _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_EXACT), want, (name, fmt, "EXACT, run %d" % run))
    _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_EXACT_UNFILTERED), want, (name, fmt, "EXACT_UNFILTERED"))
    _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_LUT), A.expected(name, fmt, boost, boost_range, True), (name, fmt, "LUT"))
    fast = _apply(hip, inp, md, fmt, boost, hip.APPLY_FAST)
    _check_apply(hip, fmt, fast, want, inp.w, inp.h, wrap=boost < boost_range[1])


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("name", A.NAMES)
def test_every_mode_at_every_case(hip, name, fmt):
    _every_mode(hip, name, fmt, FLT_MAX, A.RANGE)


@pytest.mark.parametrize("fmt", A.FORMATS)
@pytest.mark.parametrize("name,boost_range", [(n, A.RANGE) for n in A.CAPPED_NAMES] + [(A.WIDE_NAME, A.RANGE_WIDE)],
                         ids=A.CAPPED_NAMES + [A.WIDE_NAME + "_min0.5_max6"])
def test_capped_display_boost_off_factor_4(hip, name, boost_range, fmt):
    """display boost 2.0 under a content boost of 1000 / 203 (and of 6.0 over 0.5 on the factor-7 case): values pass 1.0, the codes
    wrap through the 0x3ff mask, FAST takes its masked form"""
    assert A.CAPPED < boost_range[1]
    _every_mode(hip, name, fmt, A.CAPPED, boost_range)


# ---- one batch call over cached and transient tables -----------------------------------------------------------------------------------
class _Plain:
    """a 4:2:0 LCG frame and a map that are no case of the list (the factor-4 members of the batch), shaped like Inputs"""

    def __init__(self, hip, orc, w, h, s, seed):
        from tests.gpu_util import to_dev
        self.name, self.w, self.h, self.mw, self.mh = "s%d_%dx%d_seed%d" % (s, w, h, seed), w, h, w // s, h // s
        _, self.host_planes = orc.lcg_frame(w, h, seed)
        self.host_map = np.random.RandomState(seed).randint(0, 256, (self.mh, self.mw)).astype(np.uint8)
        self.planes, self.map = to_dev(self.host_planes), to_dev(self.host_map)
        self.img = hip.yuv420_image(self.planes.data_ptr(), w, h, hip.CG_BT709)
        self.mimg = hip.mono_image(self.map.data_ptr(), self.mw, self.mh)


def _oracle_420(orc, inp, fmt):
    st, out, _ = orc.apply("orc_", orc.yuv420_image(inp.host_planes, inp.w, inp.h, orc.CG_BT709), inp.host_map, A.oracle_metadata(A.RANGE), fmt, FLT_MAX, threads=4)
    assert st == 0
    return out[:A.BPP[fmt] * inp.w * inp.h].copy()


@pytest.fixture(scope="module")
def batch_members(hip, orc):
    """factors 129, 4, 129, 3, 256, 4: six chunks, a table built for the call and freed between tables the library keeps.  The second
    129 image has the first one's map turned round; the factor-4 images are 64 x 32 over 16 x 8 (aligned planes: the scale-4 walk)"""
    turned = np.ascontiguousarray(A.gain_map("s129_258x258")[::-1, ::-1])
    members = [Inputs(hip, "s129_258x258"), _Plain(hip, orc, 64, 32, 4, 41), Inputs(hip, "s129_258x258", turned), Inputs(hip, "s3_300x12"),
               Inputs(hip, "s256_512x256"), _Plain(hip, orc, 64, 32, 4, 42)]
    assert [m.w // m.mw for m in members] == [129, 4, 129, 3, 256, 4]
    want = {fmt: [_oracle_420(orc, m, fmt) for m in members] for fmt in (1, 2)}
    assert np.array_equal(want[2][0], A.expected("s129_258x258", 2)) and not np.array_equal(want[2][0], want[2][2])
    return members, want


@pytest.mark.parametrize("fmt", [2, 1], ids=["PQ", "F16"])
@pytest.mark.parametrize("mode", ["FAST", "EXACT"])
def test_one_batch_call_mixes_cached_and_transient_tables(hip, batch_members, mode, fmt):
    import torch
    from tests.gpu_util import stream_ptr, to_host
    lib = hip.load()
    members, want = batch_members
    want = want[fmt]
    mode_v = hip.APPLY_FAST if mode == "FAST" else hip.APPLY_EXACT
    md = A.api_metadata(hip, A.RANGE)
    n = len(members)
    singles = [_apply(hip, m, md, fmt, FLT_MAX, mode_v) for m in members]
    for k, m in enumerate(members):
        if mode == "EXACT":
            _same(singles[k], want[k], (m.name, fmt, "single EXACT"))
        else:
            _check_apply(hip, fmt, singles[k], want[k], m.w, m.h)
    ya, ma = hip.image_array([m.img for m in members]), hip.image_array([m.mimg for m in members])
    side = torch.cuda.Stream()

    def call(stream):
        outs = [Guarded(A.BPP[fmt] * m.w * m.h) for m in members]
        da = hip.image_array([hip.out_image(o.ptr()) for o in outs])
        if stream is side:
            side.wait_stream(torch.cuda.current_stream())   # the sentinels are filled on the current stream
        s = stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
        assert lib.uhdr_hip_apply_gainmap_batch(n, ya, ma, C.byref(md), fmt, FLT_MAX, da, mode_v, s) == 0
        if stream is side:
            side.synchronize()
        return outs, da

    # the call, the same call again at once on the same stream, and once on a second stream
    for which, stream in (("first", None), ("again", None), ("second stream", side)):
        outs, da = call(stream)
        for k, (m, o) in enumerate(zip(members, outs)):
            got = to_host(o.body()).copy()
            assert o.guards_intact(), (which, k, m.name)
            assert (da[k].width, da[k].height) == (m.w, m.h)
            _same(got, singles[k], (which, k, m.name, fmt, mode, "batch against the single call"))
            if mode == "EXACT":
                _same(got, want[k], (which, k, m.name, fmt, "batch against the oracle"))
            else:
                _check_apply(hip, fmt, got, want[k], m.w, m.h)
    assert lib.uhdr_hip_stream_release(C.c_void_p(side.cuda_stream)) == 0


# ---- host memory, and a reserved stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s129_258x258", "s16_96x48"])
def test_host_memory_call_at_a_transient_factor(hip, name):
    """UHDR_HIP_MEM_HOST planes at factor 129 (a table for the call) and at 16 (a kept one), EXACT"""
    lib = hip.load()
    _, w, h, mw, mh, _ = A.BY_NAME[name]
    planes, gmap = A.packed(name), np.ascontiguousarray(A.gain_map(name))
    md = A.api_metadata(hip, A.RANGE)
    for fmt in (2, 1):
        nbytes = A.BPP[fmt] * w * h
        out = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
        img, mimg = hip.yuv420_image(planes.ctypes.data, w, h, hip.CG_BT709), hip.mono_image(gmap.ctypes.data, mw, mh)
        dest = hip.out_image(out.ctypes.data + GUARD)
        rc = lib.uhdr_hip_apply_gainmap(C.byref(img), C.byref(mimg), C.byref(md), fmt, FLT_MAX, C.byref(dest), hip.APPLY_EXACT, hip.MEM_HOST, None)
        assert rc == 0 and (dest.width, dest.height) == (w, h)
        assert (out[:GUARD] == 0xA5).all() and (out[GUARD + nbytes:] == 0xA5).all()
        _same(out[GUARD:GUARD + nbytes], A.expected(name, fmt), (name, fmt, "host memory"))


def test_stream_reserve_with_a_factor_past_the_cache(hip):
    """uhdr_hip_stream_reserve with factor 129 has no table to keep; the apply on that stream builds its own"""
    import torch
    lib = hip.load()
    name = "s129_258x258"
    inp = Inputs(hip, name)
    md = A.api_metadata(hip, A.RANGE)
    side = torch.cuda.Stream()
    s = C.c_void_p(side.cuda_stream)
    assert lib.uhdr_hip_stream_reserve(s, 1, inp.w, inp.h, 129) == 0
    for fmt in (3, 1):
        side.wait_stream(torch.cuda.current_stream())
        got = _apply(hip, inp, md, fmt, FLT_MAX, hip.APPLY_EXACT, stream=s)
        _same(got, A.expected(name, fmt), (name, fmt, "reserved stream"))
    assert lib.uhdr_hip_stream_release(s) == 0
