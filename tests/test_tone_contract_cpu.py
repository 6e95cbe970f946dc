"""No GPU: what the tone-map and convertYuv calls decide before they touch the device.

A process that never calls uhdr_hip_init gets as far as a call's device state and is refused there (INSUFFICIENT_RESOURCE), so
everything a call decides before that point can be observed without a device: the order of its checks, what it answers for n < 0,
n == 0 and NULL arrays, which image of a batch fails it, and that a failing call writes nothing.  rows() builds the argument sets for

    uhdr_hip_tonemap            uhdr_hip_tonemap_batch
    uhdr_hip_tonemap_sdr        uhdr_hip_tonemap_sdr_batch
    uhdr_hip_tonemap_packed     uhdr_hip_tonemap_packed_batch
    uhdr_hip_convert_yuv        uhdr_hip_convert_yuv_batch
    uhdr_hip_tonemap_headroom

the single calls in both memory spaces.  Every row is run in one child process, which never initialises a device (so the table is
the same on a machine that has one).  The fields of a destination descriptor that a call fills are pre-filled with sentinels (SENT_*),
the headroom output with HEAD_SENT.  A row of the table is [return code, the eight fields of every destination descriptor after the
call (pointers as offsets from the test's memory), the headroom words after the call (null: no headroom passed)], one row per line.

The expected table, tests/golden/tone_contract/table.json, was recorded from a library built from commit 1f1047b ("JPEG and JPEG/R
encode batches: one round driver, one of each helper"), the parent of the change that put these calls on one run former, one
headroom driver and one single-call frame:

    python tests/test_tone_contract_cpu.py --lib <that build's libuhdr_hip.so> --record

It is never recorded from the library under test; the test asserts that the current library reproduces it row for row.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from libultrahdr_dev_amd import api  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "tone_contract", "table.json")
SENT_CG, SENT_FMT, SENT_W, SENT_H, SENT_CS = 77, 55, 0x5151, 0x5252, 0x5353
HEAD_SENT = 0x7FC0ABCD               # a NaN no call computes
NULL = "NULL"
_MEM = np.zeros((1 << 16) + 64, np.uint8)
P = (_MEM.ctypes.data + 63) & ~63    # host memory behind every valid image: no row reads it, a stray access would not fault
SRC, DST, DSTC = 0, 8192, 12288      # offsets of the source, the destination and the destination's chroma planes
W, H = 16, 8
NAN, INF = float("nan"), float("inf")
BAD_PEAKS = (("negative", -1.0), ("nan", NAN), ("inf", INF))
TF_NAMES = ((api.TF_LINEAR, "linear"), (api.TF_HLG, "hlg"), (api.TF_PQ, "pq"))


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def planar_pair(k=0):
    """a valid P010 image and its destination (gamut and format: sentinels, the call's to fill)"""
    o = P + 16384 * k
    src = api.p010_image(o + SRC, W, H, api.CG_BT2100)
    dst = api.yuv420_image(o + DST, W, H, SENT_CG, chroma_ptr=o + DSTC)
    dst.pixelFormat = SENT_FMT
    return {"src": src, "dst": dst}


def packed_pair(k=0, f16=False):
    """a valid packed HDR image and its destination, of which only data and luma_stride are the caller's"""
    o = P + 16384 * k
    src = (api.rgba_f16_image if f16 else api.rgba1010102_image)(o + SRC, W, H, api.CG_BT2100)
    return {"src": src, "dst": api.Image(o + DST, SENT_W, SENT_H, SENT_CG, None, W + 4, SENT_CS, SENT_FMT)}


def yuv_image(k=0):
    o = P + 16384 * k
    return {"src": None, "dst": api.yuv420_image(o + DST, W, H, api.CG_BT709, chroma_ptr=o + DSTC)}


def edit(which, **fields):
    def go(pair):
        if fields.get("whole") is None and "whole" in fields:
            pair[which] = None
            return
        for k, v in fields.items():
            setattr(pair[which], k, (getattr(pair[which], "data") + v[1]) if isinstance(v, tuple) else v)
    return go


def both(*edits):
    def go(pair):
        for e in edits:
            e(pair)
    return go


BIG = 1 << 32
# the checks of tonemap_check in its order (ultrahdr.cpp:518-523), then what the operator adds
PLANAR_ERRORS = [
    ("size_differs", edit("dst", width=W + 2)),
    ("height_differs", edit("dst", height=H + 2)),
    ("src_data_null", edit("src", data=None)),
    ("src_chroma_null", edit("src", chroma_data=None)),
    ("dst_data_null", edit("dst", data=None)),
    ("dst_chroma_null", edit("dst", chroma_data=None)),
    ("size_differs_and_data_null", both(edit("dst", width=W + 2), edit("src", data=None))),
]
SDR_ERRORS = [
    ("odd_width", both(edit("src", width=W - 1), edit("dst", width=W - 1))),
    ("odd_height", both(edit("src", height=H - 1), edit("dst", height=H - 1))),
    ("gamut_unspecified", edit("src", colorGamut=api.CG_UNSPECIFIED)),
    ("gamut_7", edit("src", colorGamut=7)),
    ("src_luma_stride_short", edit("src", luma_stride=W - 1)),
    ("src_luma_stride_0_is_width", edit("src", luma_stride=0)),
    ("src_chroma_stride_short", edit("src", chroma_stride=W - 1)),
    ("src_chroma_stride_0", edit("src", chroma_stride=0)),
    ("dst_luma_stride_short", edit("dst", luma_stride=W - 1)),
    ("dst_chroma_stride_short", edit("dst", chroma_stride=W // 2 - 1)),
    ("odd_width_and_gamut_7", both(edit("src", width=W - 1, colorGamut=7), edit("dst", width=W - 1))),
    ("gamut_7_and_stride_short", edit("src", colorGamut=7, luma_stride=W - 1)),
]
PACKED_ERRORS = [     # (name, edit, memory space it needs: None = either)
    ("src_format_rgba8888", edit("src", pixelFormat=api.PIX_FMT_RGBA8888), None),
    ("src_format_p010", edit("src", pixelFormat=api.PIX_FMT_P010), None),
    ("src_data_null", edit("src", data=None), None),
    ("dst_data_null", edit("dst", data=None), None),
    ("format_and_data_null", edit("src", pixelFormat=api.PIX_FMT_RGBA8888, data=None), None),
    ("src_misaligned_2", edit("src", data=("+", 2)), None),
    ("dst_misaligned_2", edit("dst", data=("+", 2)), None),
    ("src_stride_short", edit("src", luma_stride=W - 1), None),
    ("src_stride_0_is_width", edit("src", luma_stride=0), None),
    ("dst_stride_short", edit("dst", luma_stride=W - 1), None),
    ("dst_stride_0_is_width", edit("dst", luma_stride=0), None),
    ("src_stride_2_32", edit("src", luma_stride=BIG), None),
    ("src_stride_2_32_less_1", edit("src", luma_stride=BIG - 1), None),
    ("dst_stride_2_32", edit("dst", luma_stride=BIG), None),
    ("gamut_unspecified", edit("src", colorGamut=api.CG_UNSPECIFIED), None),
    ("gamut_7", edit("src", colorGamut=7), None),
    ("stride_short_and_gamut_7", edit("src", luma_stride=W - 1, colorGamut=7), None),
    ("data_null_and_stride_short", edit("src", data=None, luma_stride=W - 1), None),
]
ENCODINGS = [("709_to_601", 0, 1), ("2100_to_709", 2, 0), ("equal_709", 0, 0), ("equal_2100", 2, 2), ("src_unspecified", -1, 1),
             ("dst_unspecified", 0, -1), ("both_unspecified", -1, -1), ("src_7", 7, 1), ("dst_minus_2", 0, -2), ("equal_7", 7, 7), ("dst_3", 0, 3)]
CONVERT_ERRORS = [("data_null", edit("dst", data=None)), ("chroma_null", edit("dst", chroma_data=None))]


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def rows():
    """(row id, call) for every row of the table; call: dict(fn, pairs (list, or NULL: the arrays are NULL), and the call's scalars)"""
    out = []

    def add(rid, fn, pairs, **kw):
        out.append((rid, dict(kw, fn=fn, pairs=pairs)))

    def made(make, *edits, **kw):
        ps = []
        for k, e in enumerate(edits):
            p = make(k, **kw)
            if e is not None:
                e(p)
            ps.append(p)
        return ps

    mems = (("host", api.MEM_HOST), ("device", api.MEM_DEVICE))
    reinhard, shift = api.TONEMAP_REINHARD_MAXRGB, api.TONEMAP_SHIFT

    # -- uhdr_hip_tonemap, uhdr_hip_tonemap_batch
    for mname, mem in mems:
        t = "tonemap/%s/" % mname
        add(t + "valid", "tonemap", made(planar_pair, None), mem=mem)
        add(t + "src_null", "tonemap", made(planar_pair, edit("src", whole=None)), mem=mem)
        add(t + "dst_null", "tonemap", made(planar_pair, edit("dst", whole=None)), mem=mem)
        for name, e in PLANAR_ERRORS:
            add(t + name, "tonemap", made(planar_pair, e), mem=mem)
    t = "tonemap_batch/"
    add(t + "valid_2", "tonemap_batch", made(planar_pair, None, None))
    add(t + "n_negative", "tonemap_batch", made(planar_pair, None), n=-1)
    add(t + "n_zero", "tonemap_batch", made(planar_pair, None), n=0)
    add(t + "n_zero_null_arrays", "tonemap_batch", NULL, n=0)
    add(t + "n_negative_null_arrays", "tonemap_batch", NULL, n=-1)
    add(t + "null_srcs", "tonemap_batch", made(planar_pair, None, None), null=("srcs",))
    add(t + "null_dests", "tonemap_batch", made(planar_pair, None, None), null=("dests",))
    for name, e in PLANAR_ERRORS:
        add(t + "image1_" + name, "tonemap_batch", made(planar_pair, None, e))
    add(t + "image0_data_null_image1_size_differs", "tonemap_batch", made(planar_pair, PLANAR_ERRORS[2][1], PLANAR_ERRORS[0][1]))

    # -- uhdr_hip_tonemap_sdr, uhdr_hip_tonemap_sdr_batch
    for mname, mem in mems:
        t = "tonemap_sdr/%s/" % mname

        def one(name, e=None, **kw):
            a = dict(tf=api.TF_HLG, op=reinhard, peaks=[0.0], head=True, mem=mem)
            a.update(kw)
            add(t + name, "tonemap_sdr", made(planar_pair, e), **a)
        one("valid")
        one("valid_given_peak", peaks=[600.0])
        one("headroom_null", head=False)
        one("src_null", edit("src", whole=None))
        one("dst_null", edit("dst", whole=None))
        for name, e in PLANAR_ERRORS:
            one(name, e)
            one(name + "_tf_9", e, tf=9)
        for tf, tname in TF_NAMES:
            one("tf_" + tname, tf=tf)
        one("tf_9", tf=9)
        one("tf_srgb", tf=api.TF_SRGB)
        one("tf_9_op_2", tf=9, op=2)
        for op in (2, -1):
            one("op_%d" % op, op=op)
            one("op_%d_odd_width" % op, SDR_ERRORS[0][1], op=op)
        for pname, pk in BAD_PEAKS:
            one("peak_" + pname, peaks=[pk])
            one("peak_%s_odd_width" % pname, SDR_ERRORS[0][1], peaks=[pk])
            one("shift_peak_" + pname, op=shift, peaks=[pk])
        one("shift", op=shift)
        one("shift_headroom_null", op=shift, head=False)
        one("shift_tf_9", op=shift, tf=9)
        one("shift_size_differs", PLANAR_ERRORS[0][1], op=shift)
        for name, e in SDR_ERRORS:
            one(name, e)
            one("shift_" + name, e, op=shift)      # the shift asks none of this
    t = "tonemap_sdr_batch/"

    def sdr(name, pairs, **kw):
        a = dict(tf=api.TF_PQ, op=reinhard, peaks=[0.0, 600.0], head=True)
        a.update(kw)
        add(t + name, "tonemap_sdr_batch", pairs, **a)
    two = lambda e=None, e0=None: made(planar_pair, e0, e)      # noqa: E731
    sdr("valid_2", two())
    sdr("valid_2_null_peaks", two(), peaks=None)
    sdr("n_negative", two(), n=-1)
    sdr("n_negative_tf_9", two(), n=-1, tf=9)
    sdr("n_zero", two(), n=0)
    sdr("n_zero_null_arrays", NULL, n=0, peaks=None, head=False)
    sdr("n_zero_null_arrays_tf_9", NULL, n=0, peaks=None, head=False, tf=9)
    sdr("n_zero_null_arrays_op_2", NULL, n=0, peaks=None, head=False, op=2)
    sdr("n_zero_null_arrays_shift", NULL, n=0, peaks=None, head=False, op=shift)
    sdr("null_srcs", two(), null=("srcs",))
    sdr("null_dests", two(), null=("dests",))
    sdr("null_srcs_tf_9", two(), null=("srcs",), tf=9)
    sdr("headroom_null", two(), head=False)
    sdr("headroom_null_image1_odd_width", two(SDR_ERRORS[0][1]), head=False)
    sdr("headroom_null_peak_nan", two(), head=False, peaks=[0.0, NAN])
    for name, e in PLANAR_ERRORS:
        sdr("image1_" + name, two(e))
        sdr("image1_%s_tf_9" % name, two(e), tf=9)
    sdr("image0_odd_width_image1_size_differs", two(PLANAR_ERRORS[0][1], SDR_ERRORS[0][1]))
    sdr("tf_9", two(), tf=9)
    sdr("tf_9_op_2", two(), tf=9, op=2)
    sdr("op_2", two(), op=2)
    sdr("op_minus_1_peak_nan", two(), op=-1, peaks=[0.0, NAN])
    for pname, pk in BAD_PEAKS:
        sdr("peak1_" + pname, two(), peaks=[0.0, pk])
        sdr("peak1_%s_image0_gamut_7" % pname, two(None, SDR_ERRORS[3][1]), peaks=[0.0, pk])
        sdr("shift_peak1_" + pname, two(), op=shift, peaks=[0.0, pk])
    sdr("shift", two(), op=shift)
    sdr("shift_headroom_null_null_peaks", two(), op=shift, head=False, peaks=None)
    sdr("shift_tf_9", two(), op=shift, tf=9)
    sdr("shift_image1_data_null", two(PLANAR_ERRORS[2][1]), op=shift)
    for name, e in SDR_ERRORS:
        sdr("image1_" + name, two(e))
        sdr("shift_image1_" + name, two(e), op=shift)
    sdr("image0_stride_short_image1_odd_width", two(SDR_ERRORS[0][1], SDR_ERRORS[4][1]))

    # -- uhdr_hip_tonemap_packed, uhdr_hip_tonemap_packed_batch
    forms = (("pq1010102", False, api.TF_PQ), ("hlg1010102", False, api.TF_HLG), ("f16", True, api.TF_LINEAR))
    for mname, mem in mems:
        for fname, f16, ftf in forms:
            t = "tonemap_packed/%s/%s/" % (mname, fname)

            def one(name, e=None, **kw):
                a = dict(tf=ftf, op=reinhard, peaks=[0.0], head=True, mem=mem)
                a.update(kw)
                add(t + name, "tonemap_packed", made(packed_pair, e, f16=f16), **a)
            one("valid")
            one("valid_given_peak", peaks=[450.0])
            one("headroom_null", head=False)           # allowed in the single call
            one("src_null", edit("src", whole=None))
            one("dst_null", edit("dst", whole=None))
            one("src_null_tf_9", edit("src", whole=None), tf=9)
            for tf, tname in TF_NAMES:
                one("tf_" + tname, tf=tf)              # F16 with HLG / PQ, 1010102 with LINEAR
            one("tf_9", tf=9)
            one("shift", op=shift)
            one("op_2", op=2)
            one("shift_tf_9", op=shift, tf=9)
            one("shift_headroom_null", op=shift, head=False)
            for pname, pk in BAD_PEAKS:
                one("peak_" + pname, peaks=[pk])
                one("peak_%s_stride_short" % pname, PACKED_ERRORS[7][1], peaks=[pk])
            for name, e, _ in PACKED_ERRORS:
                one(name, e)
            one("src_misaligned_4", edit("src", data=("+", 4)))      # BAD_PTR for F16 in device memory alone
            one("src_data_null_tf_9", PACKED_ERRORS[2][1], tf=9)
            one("src_format_rgba8888_tf_9", PACKED_ERRORS[0][1], tf=9)
            one("tf_9_stride_short", PACKED_ERRORS[7][1], tf=9)
            one("headroom_null_stride_short", PACKED_ERRORS[7][1], head=False)
    for fname, f16, ftf in forms:
        t = "tonemap_packed_batch/%s/" % fname

        def pk_(name, pairs, **kw):
            a = dict(tf=ftf, op=reinhard, peaks=[0.0, 600.0], head=True)
            a.update(kw)
            add(t + name, "tonemap_packed_batch", pairs, **a)
        two = lambda e=None, e0=None: made(packed_pair, e0, e, f16=f16)      # noqa: E731
        pk_("valid_2", two())
        pk_("valid_2_null_peaks", two(), peaks=None)
        pk_("n_negative", two(), n=-1)
        pk_("n_zero", two(), n=0)
        for tf, tname in TF_NAMES + ((9, "9"),):
            pk_("n_zero_null_arrays_tf_" + tname, NULL, n=0, peaks=None, head=False, tf=tf)
        pk_("n_zero_null_arrays_shift", NULL, n=0, peaks=None, head=False, op=shift)
        pk_("n_zero_null_arrays_tf_9_shift", NULL, n=0, peaks=None, head=False, op=shift, tf=9)
        pk_("null_srcs", two(), null=("srcs",))
        pk_("null_dests", two(), null=("dests",))
        pk_("null_srcs_tf_9", two(), null=("srcs",), tf=9)
        pk_("headroom_null", two(), head=False)                     # BAD_PTR here
        pk_("headroom_null_image1_stride_short", two(PACKED_ERRORS[7][1]), head=False)
        pk_("headroom_null_peak1_nan", two(), head=False, peaks=[0.0, NAN])
        pk_("headroom_null_shift", two(), head=False, op=shift)
        pk_("mixed_formats", two(edit("src", pixelFormat=api.PIX_FMT_RGBA1010102 if f16 else api.PIX_FMT_RGBA_F16)))
        pk_("mixed_formats_image0_data_null", two(edit("src", pixelFormat=api.PIX_FMT_RGBA1010102 if f16 else api.PIX_FMT_RGBA_F16), PACKED_ERRORS[2][1]))
        for tf, tname in TF_NAMES + ((9, "9"),):
            pk_("tf_" + tname, two(), tf=tf)
        pk_("shift", two(), op=shift)
        pk_("op_2", two(), op=2)
        pk_("shift_tf_9", two(), op=shift, tf=9)
        for pname, pk in BAD_PEAKS:
            pk_("peak1_" + pname, two(), peaks=[0.0, pk])
            pk_("peak1_%s_image0_gamut_7" % pname, two(None, PACKED_ERRORS[15][1]), peaks=[0.0, pk])
        for name, e, _ in PACKED_ERRORS:
            pk_("image1_" + name, two(e))
        pk_("image1_src_misaligned_4", two(edit("src", data=("+", 4))))
        pk_("image1_data_null_tf_9", two(PACKED_ERRORS[2][1]), tf=9)
        pk_("image0_gamut_7_image1_stride_short", two(PACKED_ERRORS[7][1], PACKED_ERRORS[15][1]))
        pk_("image0_stride_short_image1_data_null", two(PACKED_ERRORS[2][1], PACKED_ERRORS[7][1]))

    # -- uhdr_hip_convert_yuv, uhdr_hip_convert_yuv_batch
    for mname, mem in mems:
        t = "convert_yuv/%s/" % mname
        for ename, se, de in ENCODINGS:
            add(t + ename, "convert_yuv", made(yuv_image, None), se=se, de=de, mem=mem)
            add(t + ename + "_image_null", "convert_yuv", made(yuv_image, edit("dst", whole=None)), se=se, de=de, mem=mem)
            for name, e in CONVERT_ERRORS:      # equal encodings answer NO_ERROR before the planes are looked at
                add(t + "%s_%s" % (ename, name), "convert_yuv", made(yuv_image, e), se=se, de=de, mem=mem)
    t = "convert_yuv_batch/"
    for ename, se, de in ENCODINGS:
        add(t + ename, "convert_yuv_batch", made(yuv_image, None, None), se=se, de=de)
        add(t + ename + "_n_zero", "convert_yuv_batch", made(yuv_image, None), se=se, de=de, n=0)
        add(t + ename + "_n_zero_null_images", "convert_yuv_batch", NULL, se=se, de=de, n=0)
        add(t + ename + "_n_negative", "convert_yuv_batch", made(yuv_image, None), se=se, de=de, n=-1)
        add(t + ename + "_null_images", "convert_yuv_batch", made(yuv_image, None, None), se=se, de=de, null=("dests",))
        for name, e in CONVERT_ERRORS:
            add(t + "%s_image1_%s" % (ename, name), "convert_yuv_batch", made(yuv_image, None, e), se=se, de=de)
            add(t + "%s_image0_%s" % (ename, name), "convert_yuv_batch", made(yuv_image, e, None), se=se, de=de)

    # -- uhdr_hip_tonemap_headroom: host code, so the valid rows carry values
    t = "tonemap_headroom/"
    for tf, tname in TF_NAMES + ((9, "9"), (api.TF_SRGB, "srgb")):
        for gname, g in (("0", 0.0), ("half", 0.5), ("0.75", 0.75), ("1", 1.0)):
            add(t + "%s_measured_%s" % (tname, gname), "tonemap_headroom", None, tf=tf, gamma_max=g, peak=0.0, head=True)
        for pk in (100.0, 203.0, 600.0, 4000.0, 20000.0):
            add(t + "%s_given_%d" % (tname, pk), "tonemap_headroom", None, tf=tf, gamma_max=0.9, peak=pk, head=True)
        for pname, pk in BAD_PEAKS:
            add(t + "%s_peak_%s" % (tname, pname), "tonemap_headroom", None, tf=tf, gamma_max=0.5, peak=pk, head=True)
        add(t + "%s_null_out" % tname, "tonemap_headroom", None, tf=tf, gamma_max=0.5, peak=0.0, head=False)
        add(t + "%s_null_out_peak_nan" % tname, "tonemap_headroom", None, tf=tf, gamma_max=0.5, peak=NAN, head=False)
    assert len({r[0] for r in out}) == len(out)
    return out


def _fields(im):
    off = lambda p: None if p is None else p - P      # noqa: E731
    return [off(im.data), im.width, im.height, im.colorGamut, off(im.chroma_data), im.luma_stride, im.chroma_stride, im.pixelFormat]


def run_row(lib, call):
    """one call: [its return, the fields of every destination descriptor behind it, the headroom words behind it]"""
    fn, pairs = call["fn"], call["pairs"]
    head_n = 1
    if fn == "tonemap_headroom":
        head = (C.c_uint32 * 1)(HEAD_SENT)
        rc = lib.uhdr_hip_tonemap_headroom(call["tf"], call["gamma_max"], call["peak"], C.cast(head, C.POINTER(C.c_float)) if call["head"] else None)
        return [rc, [], list(head) if call["head"] else None]
    batch = fn.endswith("_batch")
    if pairs == NULL:
        srcs = dests = None
        n = call["n"]
    else:
        n = call.get("n", len(pairs))
        if batch:
            srcs = api.image_array([p["src"] for p in pairs]) if pairs[0]["src"] is not None else None
            dests = api.image_array([p["dst"] for p in pairs])
        else:
            srcs = None if pairs[0]["src"] is None else C.byref(pairs[0]["src"])
            dests = None if pairs[0]["dst"] is None else C.byref(pairs[0]["dst"])
        head_n = len(pairs)
    for name in call.get("null", ()):
        if name == "srcs":
            srcs = None
        else:
            dests = None
    head = (C.c_uint32 * head_n)(*([HEAD_SENT] * head_n))
    peaks = call.get("peaks")
    if fn in ("tonemap", "tonemap_batch"):
        rc = lib.uhdr_hip_tonemap(srcs, dests, call["mem"], None) if not batch else lib.uhdr_hip_tonemap_batch(n, srcs, dests, None)
    elif fn in ("convert_yuv", "convert_yuv_batch"):
        rc = (lib.uhdr_hip_convert_yuv(dests, call["se"], call["de"], call["mem"], None) if not batch else
              lib.uhdr_hip_convert_yuv_batch(n, dests, call["se"], call["de"], None))
    elif batch:
        pk = None if peaks is None else (C.c_float * len(peaks))(*peaks)
        rc = getattr(lib, "uhdr_hip_" + fn)(n, srcs, dests, call["tf"], call["op"], pk, C.cast(head, C.c_void_p) if call["head"] else None, None)
    else:
        rc = getattr(lib, "uhdr_hip_" + fn)(srcs, dests, call["tf"], call["op"], peaks[0], C.cast(head, C.POINTER(C.c_float)) if call["head"] else None,
                                            call["mem"], None)
    if pairs == NULL:
        after = []
    elif batch:
        after = [_fields(pairs[i]["dst"] if dests is None else dests[i]) for i in range(len(pairs))]
    else:
        after = [_fields(p["dst"]) for p in pairs if p["dst"] is not None]
    return [rc, after, list(head) if call.get("head") else None]


def run_table(lib_path):
    """every row against the library at lib_path, in this process: the caller makes sure no device has been initialised in it"""
    lib = C.CDLL(lib_path)
    for name, (res, args) in api.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return {rid: run_row(lib, call) for rid, call in rows()}


def _untouched(rid, row, call):
    """no descriptor field differs from what the row passed in, the headroom words keep their sentinel"""
    if call["pairs"] not in (None, NULL):
        before = [_fields(p["dst"]) for p in call["pairs"] if p["dst"] is not None]
        if row[1] != before:
            return False
    return row[2] is None or set(row[2]) == {HEAD_SENT}


def test_the_calls_answer_as_the_recorded_table_says():
    """the library under test, in a child process that initialises no device, against the table recorded from commit 1f1047b"""
    want = json.load(open(TABLE))
    got = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--lib", api.LIB_PATH], cwd=ROOT))
    assert sorted(got) == sorted(want) == sorted(r[0] for r in rows())
    wrong = {rid: (got[rid], want[rid]) for rid in want if got[rid] != want[rid]}
    assert not wrong, "%d of %d rows differ, the first: %r" % (len(wrong), len(want), sorted(wrong.items())[0])


def test_the_table_shows_what_it_is_meant_to():
    """the recorded rows say what the contract says: a sanity check of the table itself, not of the library"""
    t = json.load(open(TABLE))
    assert len(t) > 900 and os.path.getsize(TABLE) < (1 << 18)
    calls = dict(rows())
    # nothing but uhdr_hip_tonemap_headroom writes anything without a device: a failing call writes nothing, a passing one is refused
    for rid, row in t.items():
        if not rid.startswith("tonemap_headroom/"):
            assert _untouched(rid, row, calls[rid]), rid
            assert row[0] != api.NO_ERROR or "equal_" in rid or "n_zero" in rid or "n_negative" in rid, rid
    rc = lambda rid: t[rid][0]      # noqa: E731
    BAD_PTR, GAMUT, TF, FEATURE, LEASE = (api.ERROR_BAD_PTR, api.ERROR_INVALID_COLORGAMUT, api.ERROR_INVALID_TRANS_FUNC, api.ERROR_UNSUPPORTED_FEATURE,
                                          api.ERROR_INSUFFICIENT_RESOURCE)
    # convertYuv: the oddities that stay
    assert rc("convert_yuv_batch/src_unspecified_n_zero_null_images") == GAMUT and rc("convert_yuv_batch/equal_7_n_zero_null_images") == GAMUT
    assert rc("convert_yuv_batch/equal_709_n_zero_null_images") == api.NO_ERROR and rc("convert_yuv_batch/709_to_601_n_zero_null_images") == LEASE
    assert rc("convert_yuv_batch/709_to_601_n_negative") == BAD_PTR and rc("convert_yuv_batch/src_7_n_negative") == BAD_PTR
    for m in ("host", "device"):
        assert rc("convert_yuv/%s/equal_709_data_null" % m) == api.NO_ERROR and rc("convert_yuv/%s/709_to_601_data_null" % m) == BAD_PTR
        assert rc("convert_yuv/%s/equal_7_data_null" % m) == GAMUT and rc("convert_yuv/%s/src_7_image_null" % m) == BAD_PTR
    assert rc("convert_yuv_batch/equal_2100_image1_chroma_null") == api.NO_ERROR and rc("convert_yuv_batch/2100_to_709_image1_chroma_null") == BAD_PTR
    # TONEMAP_SHIFT through the operator's call: no headroom, no look at the peaks or the operator's own checks, the transfer function first
    for m in ("host", "device"):
        p = "tonemap_sdr/%s/" % m
        assert rc(p + "shift_headroom_null") == LEASE and rc(p + "shift_peak_nan") == LEASE and rc(p + "shift_odd_width") == LEASE
        assert rc(p + "shift_tf_9") == TF and rc(p + "size_differs_tf_9") == api.ERROR_RESOLUTION_MISMATCH and rc(p + "tf_9_op_2") == TF
        assert rc(p + "headroom_null") == LEASE and rc(p + "peak_nan_odd_width") == FEATURE
    p = "tonemap_sdr_batch/"
    assert rc(p + "shift_headroom_null_null_peaks") == LEASE and rc(p + "shift_peak1_nan") == LEASE and rc(p + "shift_tf_9") == TF
    assert rc(p + "headroom_null") == BAD_PTR and rc(p + "headroom_null_peak_nan") == FEATURE
    assert rc(p + "headroom_null_image1_odd_width") == BAD_PTR and rc(p + "n_zero_null_arrays") == LEASE and rc(p + "n_zero_null_arrays_tf_9") == TF
    assert rc(p + "image0_odd_width_image1_size_differs") == api.ERROR_RESOLUTION_MISMATCH
    # the packed operator
    for f in ("pq1010102", "hlg1010102", "f16"):
        for m in ("host", "device"):
            p = "tonemap_packed/%s/%s/" % (m, f)
            assert rc(p + "headroom_null") == LEASE and rc(p + "shift") == FEATURE and rc(p + "shift_tf_9") == TF
            assert rc(p + "src_misaligned_2") == (BAD_PTR if m == "device" else LEASE) == rc(p + "dst_misaligned_2")
            assert rc(p + "src_misaligned_4") == (BAD_PTR if (m, f) == ("device", "f16") else LEASE)
            assert rc(p + "src_stride_2_32") == api.ERROR_INVALID_STRIDE == rc(p + "dst_stride_2_32") and rc(p + "src_stride_2_32_less_1") == LEASE
            assert rc(p + "tf_linear") == (LEASE if f == "f16" else TF) and rc(p + "tf_pq") == (TF if f == "f16" else LEASE) == rc(p + "tf_hlg")
        p = "tonemap_packed_batch/%s/" % f
        assert rc(p + "headroom_null") == BAD_PTR and rc(p + "mixed_formats") == FEATURE and rc(p + "headroom_null_shift") == FEATURE
        assert [rc(p + "n_zero_null_arrays_tf_" + x) for x in ("linear", "hlg", "pq", "9")] == [LEASE, LEASE, LEASE, TF]
        assert rc(p + "n_zero_null_arrays_shift") == FEATURE and rc(p + "image0_gamut_7_image1_stride_short") == GAMUT
    # the headroom rule: values, and its three refusals in the header's order
    assert rc("tonemap_headroom/hlg_null_out_peak_nan") == BAD_PTR and rc("tonemap_headroom/9_peak_nan") == TF
    assert rc("tonemap_headroom/pq_peak_nan") == FEATURE and t["tonemap_headroom/pq_peak_nan"][2] == [HEAD_SENT]
    one, given = np.array(t["tonemap_headroom/hlg_given_100"][2], np.uint32).view(np.float32)[0], np.array(t["tonemap_headroom/pq_given_600"][2], np.uint32).view(np.float32)[0]
    assert one == 1.0 and given == np.float32(600.0) / np.float32(203.0)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libuhdr_hip.so to run the rows against")
    ap.add_argument("--record", action="store_true", help="write the table (from a build of the commit the docstring names) instead of printing it")
    a = ap.parse_args()
    table = run_table(a.lib)
    if a.record:
        os.makedirs(os.path.dirname(TABLE), exist_ok=True)
        with open(TABLE, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + "\n}\n")      # a row per line
        print("%d rows -> %s" % (len(table), TABLE))
    else:
        json.dump(table, sys.stdout)
