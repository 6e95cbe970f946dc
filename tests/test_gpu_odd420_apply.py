"""-m gpu: applyGainMap on odd-sized 4:2:0 images against the oracle's bytes (tests/odd420_cases.py; the oracle is pinned to the
reference's object code on these very buffers by tests/test_odd420_cpu.py).

With an odd width the last column's chroma index is one past its row, with an odd height the last row of pixels reads row h / 2 of Cb
-- which lies in Cr -- and Cr is looked for chroma_stride * (h / 2) behind Cb.  The general kernels restate that in px_inputs' `ci`
and in `im_v = im.u + c_stride * (height / 2)`: k_apply_px (FAST, EXACT_UNFILTERED), k_apply_px_est + k_apply_resolve (EXACT),
k_apply_lut (LUT), k_apply_px_rgb (three-component maps) and k_apply_px_md (general metadata).  A kernel that clamped the column or put
Cr behind ceil(h / 2) rows gives other bytes on these cases.

The image lies in device memory as the reference holds it -- floor(3 w h / 2) bytes (the strided case: as far as the reference reads)
-- followed by guard bytes, and every comparison runs with the guards at 0x00 and at 0xFF: a kernel that reads behind the reference's
buffer cannot give the oracle's bytes both times.  All pixels are compared.

Bars, tests/test_gpu_apply_scales.py's: EXACT, EXACT_UNFILTERED and LUT byte-identical to the oracle (LUT: to its LUT pipeline; a
three-component map: to the per-channel composite); FAST within tests/test_gpu_parity.py's LSB_TOL / HALF_ULP_TOL, through its
_check_apply.  General metadata: tests/test_gpu_gainmap_md.py's, one code / one half-precision ULP from tests/gainmap_md_cases' model."""
import ctypes as C

import numpy as np
import pytest

from tests import apply_scale_cases as A
from tests import odd420_cases as D
from tests.test_gpu_apply_scales import _apply, _Plain, _oracle_420, _same
from tests.test_gpu_apply_walk_tail import Guarded
from tests.test_gpu_parity import _check_apply

pytestmark = pytest.mark.gpu
FLT_MAX = D.FLT_MAX
GUARDS = (0x00, 0xFF)
GUARD_BYTES = 512


class Inputs:
    """a case's buffer and map in device memory, each followed by GUARD_BYTES of `guard` and `shift` bytes off the allocation's start"""

    def __init__(self, hip, name, guard=0x00, shift=0, planes=1):
        from tests.gpu_util import to_dev
        case = D.BY_NAME[name]
        self.name, self.w, self.h, self.mw, self.mh = name, case.w, case.h, case.mw, case.mh
        gmap = D.gain_map(name, planes)
        if planes == 3:
            rgba = np.full((case.mh, case.mw, 4), 0xFF, np.uint8)
            rgba[:, :, :3] = gmap
            gmap = rgba
        self.planes, self.map = to_dev(self._held(D.buffer(name), guard, shift)), to_dev(self._held(gmap.reshape(-1), guard, shift if planes == 1 else 4 * shift))
        ls, cs = D.strides(case)
        self.img = hip.yuv420_image(self.planes.data_ptr() + shift, case.w, case.h, hip.CG_BT709, luma_stride=ls, chroma_stride=cs)
        assert self.img.chroma_data == self.planes.data_ptr() + shift + ls * case.h      # chroma_data follows the luma
        if planes == 1:
            self.mimg = hip.mono_image(self.map.data_ptr() + shift, case.mw, case.mh)
        else:
            self.mimg = hip.rgba_map_image(self.map.data_ptr() + 4 * shift, case.mw, case.mh)

    @staticmethod
    def _held(body, guard, shift):
        host = np.full(shift + body.size + GUARD_BYTES, guard, np.uint8)
        host[shift:shift + body.size] = body
        return host


def _every_mode(hip, name, fmt, boost):
    md = A.api_metadata(hip, D.RANGE)
    want, want_lut = D.expected(name, fmt, boost), D.expected(name, fmt, boost, True)
    for guard in GUARDS:
        inp = Inputs(hip, name, guard)
        # EXACT twice on one stream: the second run finds the list headers as the first one left them
        for run in (1, 2):
            _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_EXACT), want, (name, fmt, guard, "EXACT, run %d" % run))
        _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_EXACT_UNFILTERED), want, (name, fmt, guard, "EXACT_UNFILTERED"))
        _same(_apply(hip, inp, md, fmt, boost, hip.APPLY_LUT), want_lut, (name, fmt, guard, "LUT"))
        fast = _apply(hip, inp, md, fmt, boost, hip.APPLY_FAST)
        _check_apply(hip, fmt, fast, want, inp.w, inp.h, wrap=boost < D.RANGE[1])


@pytest.mark.parametrize("fmt", D.FORMATS)
@pytest.mark.parametrize("name", D.NAMES)
def test_every_mode_at_every_case(hip, name, fmt):
    _every_mode(hip, name, fmt, FLT_MAX)


@pytest.mark.parametrize("fmt", D.FORMATS)
@pytest.mark.parametrize("name", D.CAPPED_NAMES)
def test_capped_display_boost(hip, name, fmt):
    """display boost 2.0 under a content boost of 1000 / 203: values pass 1.0, the codes wrap through the 0x3ff mask"""
    assert D.CAPPED < D.RANGE[1]
    _every_mode(hip, name, fmt, D.CAPPED)


def test_all_planes_at_odd_addresses(hip):
    """luma, chroma and map one byte off their allocations, both parities of the chroma plane's own offset (17 x 9 = 153, 18 x 9 = 162)"""
    md = A.api_metadata(hip, D.RANGE)
    for name in ("f1_17x9", "f1_18x9", "f3_63x45"):
        for guard in GUARDS:
            inp = Inputs(hip, name, guard, shift=1)
            assert inp.img.data % 2 == 1 and inp.mimg.data % 2 == 1
            for fmt in (2, 1):
                want = D.expected(name, fmt)
                _same(_apply(hip, inp, md, fmt, FLT_MAX, hip.APPLY_EXACT), want, (name, fmt, guard, "EXACT, odd addresses"))
                _same(_apply(hip, inp, md, fmt, FLT_MAX, hip.APPLY_LUT), D.expected(name, fmt, lut=True), (name, fmt, guard, "LUT, odd addresses"))
                _check_apply(hip, fmt, _apply(hip, inp, md, fmt, FLT_MAX, hip.APPLY_FAST), want, inp.w, inp.h)


# ---- one batch call per factor, an even-sized factor-4 image among the odd ones ---------------------------------------------------------
@pytest.mark.parametrize("guard", GUARDS, ids=["guard00", "guardff"])
@pytest.mark.parametrize("factor", [1, 3, 5, 7])
def test_one_batch_call_holds_a_factor_and_the_scale_4_walk(hip, orc, factor, guard):
    """all cases of one factor and a 64 x 32 image over a 16 x 8 map (aligned planes: the scale-4 walk) in one
    uhdr_hip_apply_gainmap_batch call: the fast scale-4 path and the general path share the call"""
    from tests.gpu_util import stream_ptr, to_host
    lib = hip.load()
    odd = [Inputs(hip, c.name, guard) for c in D.CASES if D.factor(c) == factor]
    plain = _Plain(hip, orc, 64, 32, 4, 40 + factor)
    members = odd[:1] + [plain] + odd[1:]
    assert len(odd) >= 1 and plain.w // plain.mw == 4
    md = A.api_metadata(hip, D.RANGE)
    ya, ma = hip.image_array([m.img for m in members]), hip.image_array([m.mimg for m in members])
    for fmt in (2, 1):
        wants = [_oracle_420(orc, m, fmt) if m is plain else D.expected(m.name, fmt) for m in members]
        for mode in (hip.APPLY_EXACT, hip.APPLY_FAST):
            outs = [Guarded(D.BPP[fmt] * m.w * m.h) for m in members]
            da = hip.image_array([hip.out_image(o.ptr()) for o in outs])
            assert lib.uhdr_hip_apply_gainmap_batch(len(members), ya, ma, C.byref(md), fmt, FLT_MAX, da, mode, stream_ptr()) == 0
            for k, (m, o) in enumerate(zip(members, outs)):
                got = to_host(o.body()).copy()
                assert o.guards_intact(), (k, m.name)
                assert (da[k].width, da[k].height) == (m.w, m.h)
                if mode == hip.APPLY_EXACT:
                    _same(got, wants[k], (factor, k, m.name, fmt, "batch, EXACT"))
                else:
                    _check_apply(hip, fmt, got, wants[k], m.w, m.h)


# ---- three-component maps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", GUARDS, ids=["guard00", "guardff"])
def test_rgb_batch(hip, guard):
    """uhdr_hip_apply_gainmap_rgb_batch on 17x9, 63x45 and 259x301 in one call (three chunks), every format"""
    from tests.gpu_util import stream_ptr, to_host
    lib = hip.load()
    members = [Inputs(hip, name, guard, planes=3) for name in D.RGB_NAMES]
    md = A.api_metadata(hip, D.RANGE)
    ya, ma = hip.image_array([m.img for m in members]), hip.image_array([m.mimg for m in members])
    for fmt in D.FORMATS:
        for mode in (hip.APPLY_EXACT, hip.APPLY_FAST):
            outs = [Guarded(D.BPP[fmt] * m.w * m.h) for m in members]
            da = hip.image_array([hip.out_image(o.ptr()) for o in outs])
            assert lib.uhdr_hip_apply_gainmap_rgb_batch(len(members), ya, ma, C.byref(md), fmt, FLT_MAX, da, mode, stream_ptr()) == 0
            for m, o in zip(members, outs):
                got, want = to_host(o.body()).copy(), D.expected_rgb(m.name, fmt)
                assert o.guards_intact(), m.name
                if mode == hip.APPLY_EXACT:
                    _same(got, want, (m.name, fmt, "rgb batch, EXACT"))
                else:
                    _check_apply(hip, fmt, got, want, m.w, m.h)


# ---- gamma, offsets and a capacity range -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", GUARDS, ids=["guard00", "guardff"])
def test_md_batch(hip, guard):
    """uhdr_hip_apply_gainmap_md_batch on 45x35 and 63x45 in one call with non-degenerate metadata, against the model of
    tests/gainmap_md_cases.py at tests/test_gpu_gainmap_md.py's bars; the model takes the samples every pixel reads in the buffer"""
    from tests import gainmap_md_cases as M
    from tests.gpu_util import stream_ptr, to_host
    lib = hip.load()
    case = M.CASES[D.MD_CASE]
    assert not M.is_degenerate(case)
    members = [Inputs(hip, name, guard) for name in D.MD_NAMES]
    md = M.api_metadata(hip, case)
    ya, ma = hip.image_array([m.img for m in members]), hip.image_array([m.mimg for m in members])
    b = M.BOOSTS[D.MD_CASE]
    for boost in (b[1], b[-1]):      # a weight inside (0, 1) and the boost capped above hdrCapacityMax
        for fmt in D.FORMATS:
            outs = [Guarded(D.BPP[fmt] * m.w * m.h) for m in members]
            da = hip.image_array([hip.out_image(o.ptr()) for o in outs])
            assert lib.uhdr_hip_apply_gainmap_md_batch(len(members), ya, ma, C.byref(md), fmt, boost, da, hip.APPLY_FAST, stream_ptr()) == 0
            for m, o in zip(members, outs):
                raw = to_host(o.body()).copy()
                assert o.guards_intact(), m.name
                e, g = D.md_inputs(m.name)
                v = M.pre_truncation(e, g, case, boost, fmt)
                codes = M.codes_of(raw, fmt, m.w, m.h)
                if fmt == M.FMT_F16:
                    worst = float(M.half_ulp_distance(codes, v).max())
                    assert worst <= 1.0, (m.name, boost, worst)
                    assert (raw.view(np.uint16).reshape(-1, 4)[:, 3] == 0x3C00).all()
                else:
                    d = M.code_distance(codes, v)
                    assert d.max() <= 1, (m.name, boost, fmt, int(d.max()), np.argwhere(d > 1)[:4])
                    if fmt != M.FMT_RGB10:
                        assert (raw.view(np.uint32) >> 30 == 3).all()
