"""No GPU: what the JPEG and JPEG/R decode calls decide before they touch the device.

A process that never calls uhdr_hip_init gets as far as a call's device state and is refused there (INSUFFICIENT_RESOURCE), so
everything a call decides before that point can be observed without a device: the order of its gates (flags, scale_denom, decode_to,
display boost, output format), what it answers for n < 0, n == 0 and NULL arrays, what every file of a batch is refused for, the size
probes, and what it has written into descriptors, metadata records and status[] by then.  rows() builds the argument sets for

    uhdr_hip_jpeg_decode          uhdr_hip_jpeg_decode_batch           uhdr_hip_jpegr_decode       uhdr_hip_jpegr_decode_batch
    uhdr_hip_jpeg_decode_rgba     uhdr_hip_jpeg_decode_batch_ex        uhdr_hip_jpegr_decode_ex    uhdr_hip_jpegr_decode_batch_ex
    uhdr_hip_jpeg_decode_ex       uhdr_hip_jpeg_decode_batch_scaled                                uhdr_hip_jpegr_decode_rgbmap_batch
    uhdr_hip_jpeg_decode_scaled   uhdr_hip_jpeg_scaled_geometry                                    uhdr_hip_jpegr_decode_md_batch
                                                                                                   uhdr_hip_jpegr_decode_scaled_batch

The JPEG/R files are assembled on the host (uhdr_hip_jpegr_append_gainmap) from the fixtures under tests/golden/sampling,
tests/golden/rgbmap and the two images of tests/golden/sample_jpegr.jpeg.  Every row is run in one child process, which never
initialises a device (so the table is the same on a machine that has one).  Destination descriptors, metadata records and status[] are
pre-filled with sentinels.  A row of the table is [return code, status[] after the call (null: none passed), the eight fields of every
destination descriptor after the call (pointers as offsets from the test's output memory), every metadata record after the call as
hex (null: none passed), a descriptor or a record that the call left as it was written "="]; the geometry call's rows carry its six output words in place of the descriptors.

The expected table, tests/golden/decode_contract/table.json, was recorded from a library built from commit 4b176f6 ("JPEG encoder:
progressive files (SOF2), every scan built on the device"), the parent of the change that put the JPEG/R decode on the shared round
driver:

    python tests/test_decode_contract_cpu.py --lib <that build's libuhdr_hip.so> --record

It is never recorded from the library under test; the test asserts that the current library reproduces it row for row.

One rule differs from that commit, by intent.  A JPEG/R batch that gets files past their checks needs the device, and without one
fails at its context: both libraries return that failure (INSUFFICIENT_RESOURCE), but the parent left status[] unwritten, and the
round driver writes it -- the refused files' own statuses, the failure for the files that needed the device.  Those are the rows whose
id starts with "jpegr_reach/" (reach_rows() builds most of them; the recorder refuses a row of this kind that is not marked).  Their return code, descriptors and metadata are the
parent's; their status[] is recorded by that rule: the recorder checks that the parent returned INSUFFICIENT_RESOURCE and left every
status word untouched, and takes status[] from the parent's answer to the same call with NULL destinations -- a call that needs no
device, in which every refused file gets the same status and every file that would have reached the device gets its size-probe answer,
which is the same INSUFFICIENT_RESOURCE.
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

GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = os.path.join(GOLDEN, "decode_contract", "table.json")
SENT_W, SENT_H, SENT_CG, SENT_LS, SENT_CS, SENT_FMT, SENT_ST, SENT_GEOM = 0x5151, 0x5252, 77, 0x5353, 0x5454, 55, 7777, -4242
SLOT = 1 << 22                       # output memory per file: the largest rendition a row has room for is the sample's 1280x720 at 4 bytes a pixel
_OUT = np.zeros(12 * SLOT + 64, np.uint8)
P = (_OUT.ctypes.data + 63) & ~63
NAN = float("nan")
NULL = "NULL"
FMT_BPP = {api.OUTPUT_SDR: 4, api.OUTPUT_HDR_LINEAR: 8, api.OUTPUT_HDR_PQ: 4, api.OUTPUT_HDR_HLG: 4, api.OUTPUT_HDR_LINEAR_RGB_10BIT: 6}


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def _read(*parts):
    return open(os.path.join(GOLDEN, *parts), "rb").read()


def _append(lib, primary, gainmap):
    md = api.Metadata(b"1.0", 10.0, 1.0, 1.0, 0.0, 0.0, 1.0, 10.0)
    out, n = np.zeros(len(primary) + len(gainmap) + 8192, np.uint8), C.c_size_t()
    a, b = np.frombuffer(primary, np.uint8), np.frombuffer(gainmap, np.uint8)
    rc = lib.uhdr_hip_jpegr_append_gainmap(a.ctypes.data, a.size, b.ctypes.data, b.size, None, 0, None, 0, C.byref(md), out.ctypes.data, out.size, C.byref(n))
    assert rc == 0, rc
    return out[:n.value].tobytes()


def _wide(jpeg):
    """the same header with a width of 8193"""
    k = jpeg.index(b"\xff\xc0")
    return jpeg[:k + 7] + bytes([0x20, 0x01]) + jpeg[k + 9:]


def files(lib):
    """name -> (bytes, (width, height) of the primary image); host code only"""
    sample = _read("sample_jpegr.jpeg")
    pi, gi = api.JpegInfo(), api.JpegInfo()
    buf = np.frombuffer(sample, np.uint8)
    assert lib.uhdr_hip_jpegr_info(buf.ctypes.data, buf.size, C.byref(pi), C.byref(gi)) == 0
    p420, gray = sample[pi.offset:pi.offset + pi.size], sample[gi.offset:gi.offset + gi.size]
    dims420 = (pi.width, pi.height)
    s444, s422, s440 = (_read("sampling", "s%s_base_130x70.jpg" % s) for s in ("11", "21", "12"))
    s444_odd = _read("sampling", "s11_base_45x37.jpg")
    prog = _read("sampling", "s11_prog_17x9.jpg")
    rgb17, rgb45_420 = _read("rgbmap", "rgb_17x9_q85.jpg"), _read("rgbmap", "rgb_45x37_s2.jpg")
    f = {
        # single JPEGs
        "j420": (p420, dims420), "jgray": (gray, (gi.width, gi.height)), "j444": (s444, (130, 70)), "j422": (s422, (130, 70)), "j440": (s440, (130, 70)),
        "j444_odd": (s444_odd, (45, 37)), "jprog": (prog, (17, 9)), "jwide": (_wide(p420), (8193, dims420[1])), "jcut": (s444[:300], (130, 70)),
        "jhead": (s444[:20], (0, 0)), "jnone": (b"\0" * 64, (0, 0)),
        # JPEG/R files
        "sample": (sample, dims420),
        "r444": (_append(lib, s444, gray), (130, 70)), "r422": (_append(lib, s422, gray), (130, 70)), "r444_odd": (_append(lib, s444_odd, gray), (45, 37)),
        "r444_rgb": (_append(lib, s444, rgb17), (130, 70)), "r444_rgb420odd": (_append(lib, s444, rgb45_420), (130, 70)),
        "r420_rgb": (_append(lib, p420, rgb17), dims420),
        "rgrayprimary": (_append(lib, gray, gray), (gi.width, gi.height)), "rwide": (_append(lib, _wide(p420), gray), (8193, dims420[1])),
        "rone": (p420, dims420), "rnone": (b"\0" * 64, (0, 0)),
    }
    r444 = f["r444"][0]
    f["rcut_primary"] = (r444[:300], (130, 70))
    f["rcut_map"] = (r444[:len(r444) - 2000], (130, 70))
    f["rnoxmp"] = (r444[:len(s444)] + r444[len(s444):].replace(b"http://ns.adobe.com/xap/1.0/", b"http://ns.adobe.com/xap/1.1/"), (130, 70))
    f["rbadxmp"] = (r444[:len(s444)] + r444[len(s444):].replace(b"hdrgm:Version", b"hdrgm:Versiom"), (130, 70))
    return f


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
JPEG_SINGLES = ("jpeg_decode", "jpeg_decode_rgba", "jpeg_decode_ex", "jpeg_decode_scaled")
JPEG_BATCHES = ("jpeg_decode_batch", "jpeg_decode_batch_ex", "jpeg_decode_batch_scaled")
JPEGR_SINGLES = ("jpegr_decode", "jpegr_decode_ex")
JPEGR_BATCHES = ("jpegr_decode_batch", "jpegr_decode_batch_ex", "jpegr_decode_rgbmap_batch", "jpegr_decode_md_batch", "jpegr_decode_scaled_batch")
HAS_FLAGS = ("jpeg_decode_ex", "jpeg_decode_scaled", "jpeg_decode_batch_ex", "jpeg_decode_batch_scaled", "jpegr_decode_ex") + JPEGR_BATCHES[1:]
HAS_SCALE = ("jpeg_decode_scaled", "jpeg_decode_batch_scaled", "jpegr_decode_scaled_batch")
HAS_DECODE_TO = ("jpeg_decode_ex", "jpeg_decode_scaled") + JPEG_BATCHES
ANY = api.DECODE_ANY_SAMPLING
HLG, SDR, F16 = api.OUTPUT_HDR_HLG, api.OUTPUT_SDR, api.OUTPUT_HDR_LINEAR
BAD_FLAGS, BAD_SCALES, BAD_TO, BAD_FMT = (2, -1), (0, 3, 16), (0, 3), (-1, 5)
BAD_BOOST = (("below_1", 0.5), ("nan", NAN))


def reach_rows(add):
    """JPEG/R batches that get files past their checks: the rows the round driver's failure rule rewrites (the docstring)"""
    mixes = [("one_file", ["r444"], {}), ("two_files", ["r444", "r422"], {}),
             ("refused_between", ["r444", "rnone", "r422", "rcut_map", "r444_odd"], {}),
             ("null_file_between", ["r444", None, "r422"], {}),
             ("probe_and_short_between", ["r444", "r422", "r444_odd", "r444"], dict(out_null=(1,), cap_short=(2,))),
             ("refused_first", ["rone", "rwide", "r444"], {}), ("refused_last", ["r444", "rnoxmp", "rbadxmp"], {})]
    for fn in JPEGR_BATCHES[1:]:
        for name, names, kw in mixes:
            wide = name in ("two_files", "refused_between")      # these in SDR and into device memory too
            for fname, fmt in (("hlg", HLG), ("sdr", SDR))[:2 if wide else 1]:
                for mname, mem in (("host", api.MEM_HOST), ("device", api.MEM_DEVICE))[:2 if wide and fmt == HLG else 1]:
                    add("%s/%s_%s_%s" % (fn, name, fname, mname), fn, names, fmt=fmt, mem=mem, flags=ANY,
                        scale=2 if fn in HAS_SCALE and (name, fmt) == ("two_files", SDR) else None, reach=True, **kw)      # (their maps follow at 1 / 1 alone)
    for fname, fmt in (("hlg", HLG), ("sdr", SDR)):      # without the flag: the sample's 4:2:0 primary
        for mname, mem in (("host", api.MEM_HOST), ("device", api.MEM_DEVICE))[:2 if fmt == HLG else 1]:
            add("jpegr_decode_batch/refused_between_%s_%s" % (fname, mname), "jpegr_decode_batch", ["sample", "r444", "rnone", "sample"], fmt=fmt, mem=mem,
                reach=True)
    add("jpegr_decode_rgbmap_batch/rgb_maps_hlg_host", "jpegr_decode_rgbmap_batch", ["r444_rgb", "r444_rgb420odd", "r444"], flags=ANY, reach=True)
    add("jpegr_decode_md_batch/status_null", "jpegr_decode_md_batch", ["r444", "rnone"], flags=ANY, null=("status",), reach=True)
    add("jpegr_decode_batch_ex/md_null", "jpegr_decode_batch_ex", ["rnone", "r444"], flags=ANY, null=("md",), reach=True)


def rows():
    """(row id, call) for every row of the table"""
    out = []

    def add(rid, fn, names, **kw):
        rid = "jpegr_reach/" + rid if kw.get("reach") else rid
        out.append((rid, dict({k: v for k, v in kw.items() if v is not None}, fn=fn, files=names)))

    # -- the single JPEG decodes
    for fn in JPEG_SINGLES:
        fl1, to1 = (ANY if fn in HAS_FLAGS else None), (api.DECODE_TO_YCBCR if fn in HAS_DECODE_TO else None)
        for name, kw in (("j422_probe", dict(out_null=(0,))), ("jgray_short", dict(cap_short=(0,))), ("jnone", {}), ("j444_odd_reaches_device", {})):
            add("%s/device/%s" % (fn, name), fn, [name[:name.index("_", 2) if name != "jnone" else None]], mem=api.MEM_DEVICE, flags=fl1, to=to1, **kw)
        for mname, mem in (("host", api.MEM_HOST),):
            t = "%s/%s/" % (fn, mname)
            tos = (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA) if fn in HAS_DECODE_TO else (None,)
            for to in tos:
                tt = t + ("" if to is None else "to%d_" % to)
                for name in ("j420", "jgray", "j444", "j422", "j440", "j444_odd", "jprog", "jwide", "jcut", "jhead", "jnone"):
                    add(tt + name + "_probe", fn, [name], mem=mem, to=to, out_null=(0,))
                    if fn in HAS_FLAGS and name in ("j444", "j422", "j440", "j444_odd", "jprog"):
                        add(tt + name + "_any_probe", fn, [name], mem=mem, to=to, flags=ANY, out_null=(0,))
                add(tt + "j444_any_short", fn, ["j444"], mem=mem, to=to, flags=ANY if fn in HAS_FLAGS else None, cap_short=(0,))
                add(tt + "jgray_short", fn, ["jgray"], mem=mem, to=to, cap_short=(0,))
                add(tt + "file_null", fn, [None], mem=mem, to=to)
                add(tt + "desc_null", fn, ["j444"], mem=mem, to=to, null=("dests",))
                add(tt + "file_and_desc_null", fn, [None], mem=mem, to=to, null=("dests",))
                add(tt + "reaches_device", fn, ["j444_odd" if fn in HAS_FLAGS else "jgray"], mem=mem, to=api.DECODE_TO_YCBCR if fn in HAS_DECODE_TO else None,
                    flags=ANY if fn in HAS_FLAGS else None) if to in (None, api.DECODE_TO_YCBCR) and fn != "jpeg_decode_rgba" else None
            if fn in HAS_FLAGS:
                for fl in BAD_FLAGS:
                    add(t + "flags_%d" % fl, fn, ["j444"], mem=mem, flags=fl, out_null=(0,))
                    add(t + "flags_%d_file_null" % fl, fn, [None], mem=mem, flags=fl)
                    add(t + "flags_%d_to_0" % fl, fn, ["j444"], mem=mem, flags=fl, to=0)
            if fn in HAS_DECODE_TO:
                for to in BAD_TO:
                    add(t + "to_%d" % to, fn, ["j444"], mem=mem, to=to, flags=ANY, out_null=(0,))
                    add(t + "to_%d_file_null" % to, fn, [None], mem=mem, to=to)
                    add(t + "to_%d_desc_null" % to, fn, ["j444"], mem=mem, to=to, null=("dests",))
            if fn in HAS_SCALE:
                for sc in BAD_SCALES:
                    add(t + "scale_%d" % sc, fn, ["j444"], mem=mem, scale=sc, flags=ANY, out_null=(0,))
                    add(t + "scale_%d_flags_2" % sc, fn, ["j444"], mem=mem, scale=sc, flags=2)
                    add(t + "scale_%d_file_null" % sc, fn, [None], mem=mem, scale=sc)
                    add(t + "scale_%d_to_0" % sc, fn, ["j444"], mem=mem, scale=sc, to=0)
                for sc in (2, 8):
                    for name in ("j420", "jgray", "j422", "j444_odd", "jwide"):
                        for to in (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA):
                            add(t + "scale_%d_to%d_%s_probe" % (sc, to, name), fn, [name], mem=mem, scale=sc, to=to, flags=ANY, out_null=(0,))

    # -- the JPEG decode batches
    for fn in JPEG_BATCHES:
        t = fn + "/"
        fl = ANY if fn in HAS_FLAGS else None
        for to in (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA):
            tt = t + "to%d_" % to
            add(tt + "n_negative", fn, ["j444"], n=-1, to=to, flags=fl)
            add(tt + "n_zero", fn, ["j444"], n=0, to=to, flags=fl)
            add(tt + "n_zero_null_arrays", fn, NULL, n=0, to=to, flags=fl)
            add(tt + "n_negative_null_arrays", fn, NULL, n=-1, to=to, flags=fl)
            for arr in ("files", "sizes", "dests", "out", "cap", "status"):
                add(tt + "null_" + arr, fn, ["j444", "jgray"], to=to, flags=fl, null=(arr,))
            add(tt + "probes_of_every_file", fn, ["j420", "jgray", "j444", "j422", "j440", "j444_odd", "jprog", "jwide", "jcut", "jhead", "jnone"], to=to, flags=fl,
                null=("out", "cap"))
            add(tt + "null_file_between", fn, ["j444", None, "jgray"], to=to, flags=fl, null=("out", "cap"))
            add(tt + "short_between", fn, ["j444", "jgray", "j422"], to=to, flags=fl, cap_short=(0, 1, 2))
            add(tt + "refused_and_reaching", fn, ["jnone", "j444_odd", None, "jgray", "jwide"], to=to, flags=fl, out_null=(3,))
            add(tt + "all_reaching", fn, ["j444_odd", "jprog"] if fl else ["jgray", "jgray"], to=api.DECODE_TO_YCBCR, flags=fl) if to == api.DECODE_TO_YCBCR else None
        for to in BAD_TO:
            add(t + "to_%d" % to, fn, ["j444"], to=to, flags=fl)
            add(t + "to_%d_n_negative" % to, fn, ["j444"], to=to, flags=fl, n=-1)
            add(t + "to_%d_null_files" % to, fn, ["j444"], to=to, flags=fl, null=("files",))
            add(t + "to_%d_n_zero_null_arrays" % to, fn, NULL, n=0, to=to, flags=fl)
        if fn in HAS_FLAGS:
            for f2 in BAD_FLAGS:
                add(t + "flags_%d" % f2, fn, ["j444"], flags=f2, to=api.DECODE_TO_YCBCR)
                add(t + "flags_%d_n_negative" % f2, fn, ["j444"], flags=f2, to=api.DECODE_TO_YCBCR, n=-1)
                add(t + "flags_%d_to_0" % f2, fn, ["j444"], flags=f2, to=0)
                add(t + "flags_%d_null_arrays" % f2, fn, NULL, n=0, flags=f2, to=api.DECODE_TO_YCBCR)
        if fn in HAS_SCALE:
            for sc in BAD_SCALES:
                add(t + "scale_%d" % sc, fn, ["j444"], scale=sc, flags=ANY, to=api.DECODE_TO_YCBCR)
                add(t + "scale_%d_flags_2" % sc, fn, ["j444"], scale=sc, flags=2, to=api.DECODE_TO_YCBCR)
                add(t + "scale_%d_n_negative" % sc, fn, ["j444"], scale=sc, flags=ANY, to=api.DECODE_TO_YCBCR, n=-1)
                add(t + "scale_%d_to_0" % sc, fn, ["j444"], scale=sc, flags=ANY, to=0)
            for sc in (2, 4, 8):
                for to in (api.DECODE_TO_YCBCR, api.DECODE_TO_RGBA):
                    add(t + "scale_%d_to%d_probes" % (sc, to), fn, ["j420", "jgray", "j444", "j422", "j440", "j444_odd", "jwide", "jnone"], scale=sc, to=to, flags=ANY,
                        null=("out", "cap"))

    # -- uhdr_hip_jpeg_scaled_geometry
    for sc in (1, 2, 8, 3):
        for w, h in ((130, 70), (17, 9), (0, 70))[:3 if sc == 2 else 1]:
            for hs, vs, gray in ((2, 2, 0), (1, 1, 0), (2, 1, 0), (1, 2, 0), (1, 1, 1), (3, 1, 0), (3, 1, 1)):
                add("geometry/s%d_%dx%d_%d%d_g%d" % (sc, w, h, hs, vs, gray), "geometry", None, geom=(w, h, hs, vs, gray, sc))
    add("geometry/null_outputs", "geometry", None, geom=(130, 70, 2, 2, 0, 2), null=("out",))
    add("geometry/null_outputs_scale_3", "geometry", None, geom=(130, 70, 2, 2, 0, 3), null=("out",))

    # -- the single JPEG/R decodes
    every = ["sample", "r444", "r422", "r444_odd", "r444_rgb", "r444_rgb420odd", "r420_rgb", "rgrayprimary", "rwide", "rone", "rnone", "rcut_primary", "rcut_map",
             "rnoxmp", "rbadxmp"]
    for fn in JPEGR_SINGLES:
        for name, kw in (("sample_probe", dict(out_null=(0,))), ("sample_short", dict(cap_short=(0,))), ("rnone", {}), ("sample_boost_below_1", dict(boost=0.5))):
            add("%s/device/%s" % (fn, name), fn, [name.split("_")[0]], mem=api.MEM_DEVICE, **kw)
        for mname, mem in (("host", api.MEM_HOST),):
            t = "%s/%s/" % (fn, mname)
            for fname, fmt in (("hlg", HLG), ("sdr", SDR), ("f16", F16)):
                for name in every if fmt != F16 else every[:2]:
                    if fn not in HAS_FLAGS or name in ("sample", "r444", "r444_rgb", "rnone"):
                        add(t + "%s_%s_probe" % (name, fname), fn, [name], mem=mem, fmt=fmt, out_null=(0,))
                    if fn in HAS_FLAGS:
                        add(t + "%s_%s_any_probe" % (name, fname), fn, [name], mem=mem, fmt=fmt, flags=ANY, out_null=(0,))
                add(t + "sample_%s_short" % fname, fn, ["sample"], mem=mem, fmt=fmt, cap_short=(0,))
                add(t + "sample_%s_md_null_probe" % fname, fn, ["sample"], mem=mem, fmt=fmt, out_null=(0,), null=("md",))
                add(t + "rnoxmp_%s_md_null_probe" % fname, fn, ["rnoxmp"], mem=mem, fmt=fmt, out_null=(0,), null=("md",), flags=ANY if fn in HAS_FLAGS else None)
            add(t + "file_null", fn, [None], mem=mem)
            add(t + "dest_null", fn, ["sample"], mem=mem, null=("dests",))
            add(t + "file_and_dest_null", fn, [None], mem=mem, null=("dests",))
            for bname, b in BAD_BOOST:
                add(t + "boost_" + bname, fn, ["sample"], mem=mem, boost=b, out_null=(0,))
                add(t + "boost_%s_fmt_5" % bname, fn, ["sample"], mem=mem, boost=b, fmt=5, out_null=(0,))
                add(t + "boost_%s_file_null" % bname, fn, [None], mem=mem, boost=b)
            for f in BAD_FMT:
                add(t + "fmt_%d" % f, fn, ["sample"], mem=mem, fmt=f, out_null=(0,))
                add(t + "fmt_%d_file_null" % f, fn, [None], mem=mem, fmt=f)
                add(t + "fmt_%d_rnone" % f, fn, ["rnone"], mem=mem, fmt=f)
            if fn in HAS_FLAGS:
                for fl in BAD_FLAGS:
                    add(t + "flags_%d" % fl, fn, ["sample"], mem=mem, flags=fl, out_null=(0,))
                    add(t + "flags_%d_file_null" % fl, fn, [None], mem=mem, flags=fl)
                    add(t + "flags_%d_boost_below_1" % fl, fn, ["sample"], mem=mem, flags=fl, boost=0.5)
                    add(t + "flags_%d_fmt_5" % fl, fn, ["sample"], mem=mem, flags=fl, fmt=5)

    # -- the JPEG/R decode batches
    for fn in JPEGR_BATCHES:
        t = fn + "/"
        fl = ANY if fn in HAS_FLAGS else None
        add(t + "n_negative", fn, ["sample"], n=-1, flags=fl)
        add(t + "n_zero", fn, ["sample"], n=0, flags=fl)
        add(t + "n_zero_null_arrays", fn, NULL, n=0, flags=fl)
        add(t + "n_negative_null_arrays", fn, NULL, n=-1, flags=fl)
        add(t + "n_zero_null_arrays_boost_nan", fn, NULL, n=0, flags=fl, boost=NAN)
        add(t + "n_zero_null_arrays_fmt_5", fn, NULL, n=0, flags=fl, fmt=5)
        for arr in ("files", "sizes", "dests", "out", "cap", "md", "status"):
            add(t + "null_" + arr, fn, ["sample", "r444"], flags=fl, null=(arr,), out_null=(0, 1) if arr in ("files", "sizes", "dests") else (),
                reach=True if arr == "md" else None)      # (without the metadata array the files go on to the device)
            if arr in ("files", "dests"):
                add(t + "null_%s_boost_below_1" % arr, fn, ["sample", "r444"], flags=fl, null=(arr,), boost=0.5)
                add(t + "null_%s_fmt_5" % arr, fn, ["sample", "r444"], flags=fl, null=(arr,), fmt=5)
        for fname, fmt in (("hlg", HLG), ("sdr", SDR), ("f16", F16)):
            add(t + "probes_of_every_file_" + fname, fn, every, fmt=fmt, flags=fl, null=("out", "cap"))
            if fmt == HLG:
                add(t + "probes_of_every_file_md_null_" + fname, fn, every, fmt=fmt, flags=fl, null=("out", "cap", "md"))
            if fl and fmt == HLG:
                add(t + "probes_of_every_file_flags_0_" + fname, fn, every, fmt=fmt, flags=0, null=("out", "cap"))
            add(t + "null_file_between_" + fname, fn, ["sample", None, "r444"], fmt=fmt, flags=fl, null=("out", "cap"))
            add(t + "short_and_null_dests_" + fname, fn, ["sample", "r444", "r444_odd", "rnone"], fmt=fmt, flags=fl, cap_short=(0, 2), out_null=(1,))
        for bname, b in BAD_BOOST:
            add(t + "boost_" + bname, fn, ["sample"], flags=fl, boost=b, null=("out", "cap"))
            add(t + "boost_%s_fmt_5" % bname, fn, ["sample"], flags=fl, boost=b, fmt=5)
            add(t + "boost_%s_n_negative" % bname, fn, ["sample"], flags=fl, boost=b, n=-1)
            add(t + "boost_%s_null_files" % bname, fn, ["sample"], flags=fl, boost=b, null=("files",))
        for f in BAD_FMT:
            add(t + "fmt_%d" % f, fn, ["sample"], flags=fl, fmt=f)
            add(t + "fmt_%d_n_negative" % f, fn, ["sample"], flags=fl, fmt=f, n=-1)
            add(t + "fmt_%d_rnone" % f, fn, ["rnone"], flags=fl, fmt=f)
        if fn in HAS_FLAGS:
            for f2 in BAD_FLAGS:
                add(t + "flags_%d" % f2, fn, ["sample"], flags=f2)
                add(t + "flags_%d_n_negative" % f2, fn, ["sample"], flags=f2, n=-1)
                add(t + "flags_%d_boost_nan" % f2, fn, ["sample"], flags=f2, boost=NAN)
                add(t + "flags_%d_fmt_5" % f2, fn, ["sample"], flags=f2, fmt=5)
                add(t + "flags_%d_null_arrays" % f2, fn, NULL, n=0, flags=f2)
        if fn in HAS_SCALE:
            for sc in BAD_SCALES:
                add(t + "scale_%d" % sc, fn, ["sample"], scale=sc, flags=ANY)
                add(t + "scale_%d_flags_2" % sc, fn, ["sample"], scale=sc, flags=2)
                add(t + "scale_%d_n_negative" % sc, fn, ["sample"], scale=sc, flags=ANY, n=-1)
                add(t + "scale_%d_boost_nan" % sc, fn, ["sample"], scale=sc, flags=ANY, boost=NAN)
                add(t + "scale_%d_fmt_5" % sc, fn, ["sample"], scale=sc, flags=ANY, fmt=5)
            for sc in (2, 8):
                # the sample's map follows its primary (factor 4); the assembled files' maps (320x180 under 130x70, 17x9 under 130x70) cannot
                for fname, fmt in (("hlg", HLG), ("sdr", SDR)):
                    add(t + "scale_%d_probes_of_every_file_%s" % (sc, fname), fn, every, scale=sc, fmt=fmt, flags=ANY, null=("out", "cap"))
                add(t + "scale_%d_map_cannot_follow_valid_dests" % sc, fn, ["r444", "r444_rgb"], scale=sc, flags=ANY)
    reach_rows(add)
    assert len({r[0] for r in out}) == len(out)
    return out


# ---- one row ----------------------------------------------------------------------------------------------------------------------------
def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


def _fields(im):
    off = lambda p: None if p is None else p - P if P <= p < P + _OUT.size else ["outside", p]      # noqa: E731
    return [off(im.data), im.width, im.height, im.colorGamut, off(im.chroma_data), im.luma_stride, im.chroma_stride, im.pixelFormat]


def _need(c, dims, jpegr, gray=False):
    """the bytes a destination must hold (the rows with a capacity one byte short know their files)"""
    w, h = dims
    s = c.get("scale", 1) if c.get("scale", 1) in api.DECODE_SCALE_DENOMS else 1
    w, h = -(-w // s), -(-h // s)
    if jpegr:
        return w * h * FMT_BPP.get(c.get("fmt", HLG), 0)
    if c["fn"] == "jpeg_decode_rgba" or c.get("to") == api.DECODE_TO_RGBA:
        return w * h * 4
    return w * h * (1 if gray else 3)      # (the rows' files: gray or 4:4:4)


def run_row(lib, F, c):
    fn = c["fn"]
    if fn == "geometry":
        o = (C.c_int * 6)(*([SENT_GEOM] * 6))
        p = [None] * 4 if "out" in c.get("null", ()) else [C.cast(C.byref(o, 4 * k), C.POINTER(C.c_int)) for k in (0, 1, 2)] + [C.cast(C.byref(o, 12), C.POINTER(C.c_int))]
        return [lib.uhdr_hip_jpeg_scaled_geometry(*c["geom"], *p), None, list(o), None]
    jpegr = fn.startswith("jpegr")
    names, null = c["files"], c.get("null", ())
    m = 0 if names == NULL else len(names)
    n = c.get("n", m)
    bufs = [None if k is None else np.frombuffer(F[k][0] + b"\0" * 8, np.uint8) for k in (names if m else [])]
    sizes = [0 if k is None else len(F[k][0]) for k in (names if m else [])]
    outs = [None if i in c.get("out_null", ()) else P + SLOT * i for i in range(m)]
    caps = []
    for i in range(m):
        need = 0 if names[i] is None else _need(c, F[names[i]][1], jpegr, names[i] == "jgray")
        assert i not in c.get("cap_short", ()) or need > 0
        caps.append(need - 1 if i in c.get("cap_short", ()) else (0 if outs[i] is None else SLOT))
    dests = api.image_array([api.Image(None, SENT_W, SENT_H, SENT_CG, None, SENT_LS, SENT_CS, SENT_FMT) for _ in range(max(m, 1))])
    mds = (api.Metadata * max(m, 1))()
    C.memset(mds, 0xAB, C.sizeof(mds))
    stat = _arr(C.c_int, [SENT_ST] * m)
    fmt, boost, mem = c.get("fmt", HLG), c.get("boost", api.FLT_MAX), c.get("mem", api.MEM_HOST)
    tail = ([c.get("flags", 0)] if fn in HAS_FLAGS else []) + ([c.get("scale", 1)] if fn in HAS_SCALE else [])
    call = getattr(lib, "uhdr_hip_" + fn)
    if fn in JPEG_SINGLES + JPEGR_SINGLES:
        f0 = None if bufs[0] is None else bufs[0].ctypes.data
        d0 = None if "dests" in null else C.byref(dests[0])
        if jpegr:
            rc = call(f0, sizes[0], fmt, boost, outs[0], caps[0], d0, None if "md" in null else C.byref(mds[0]), api.APPLY_EXACT, mem, None, *tail)
        else:
            to = [c.get("to", api.DECODE_TO_YCBCR)] if fn in HAS_DECODE_TO else []
            rc = call(f0, sizes[0], *to, outs[0], caps[0], d0, mem, None, *tail)
        stat = None
    else:
        a_files = None if names == NULL or "files" in null else _arr(C.c_void_p, [None if b is None else b.ctypes.data for b in bufs])
        a_sizes = None if names == NULL or "sizes" in null else _arr(C.c_size_t, sizes)
        a_out = None if names == NULL or "out" in null else _arr(C.c_void_p, outs)
        a_cap = None if names == NULL or "cap" in null else _arr(C.c_size_t, caps)
        a_dst = None if names == NULL or "dests" in null else dests
        a_st = None if names == NULL or "status" in null else stat
        if jpegr:
            rc = call(n, a_files, a_sizes, fmt, boost, a_out, a_cap, a_dst, None if names == NULL or "md" in null else mds, a_st, api.APPLY_EXACT, mem, None, *tail)
        else:
            rc = call(n, a_files, a_sizes, c.get("to", api.DECODE_TO_YCBCR), a_out, a_cap, a_dst, a_st, mem, None, *tail)
        stat = None if a_st is None else list(stat)[:m]
    after_md = None if not jpegr or names == NULL or "md" in null else [bytes(mds[i]).hex() for i in range(m)]
    same = lambda v, sent: "=" if v == sent else v      # noqa: E731
    return [rc, stat, [same(_fields(dests[i]), [None, SENT_W, SENT_H, SENT_CG, None, SENT_LS, SENT_CS, SENT_FMT]) for i in range(m)],
            None if after_md is None else [same(x, "ab" * 36) for x in after_md]]


def fn_writes_status_late(c, row):
    """a JPEG/R batch row that the parent failed at the context, with status[] untouched"""
    return c["fn"] in JPEGR_BATCHES and row[0] == api.ERROR_INSUFFICIENT_RESOURCE and row[1] and set(row[1]) == {SENT_ST}


def run_table(lib_path, record=False):
    """every row against the library at lib_path, in this process: the caller makes sure no device has been initialised in it"""
    lib = C.CDLL(lib_path)
    for name, (res, args) in api.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    F = files(lib)
    table = {}
    for rid, c in rows():
        row = run_row(lib, F, c)
        if record and c.get("reach"):      # the failure rule (the docstring): status[] by the rule, everything else the parent's
            assert row[0] == api.ERROR_INSUFFICIENT_RESOURCE and (row[1] is None or set(row[1]) == {SENT_ST}), (rid, row[:2])
            probe = run_row(lib, F, dict(c, null=tuple(c.get("null", ())) + ("out", "cap")))
            assert probe[0] != api.NO_ERROR and api.ERROR_INSUFFICIENT_RESOURCE in probe[1] if probe[1] is not None else True, rid
            row[1] = probe[1]
        elif record and fn_writes_status_late(c, row):
            raise AssertionError("%s reaches the device: mark it reach=True" % rid)
        table[rid] = row
    return table


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
def test_the_calls_answer_as_the_recorded_table_says():
    """the library under test, in a child process that initialises no device, against the table recorded from commit 4b176f6"""
    want = json.load(open(TABLE))
    got = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--lib", api.LIB_PATH], cwd=ROOT))
    assert sorted(got) == sorted(want) == sorted(r[0] for r in rows())
    wrong = {rid: (got[rid], want[rid]) for rid in want if got[rid] != want[rid]}
    assert not wrong, "%d of %d rows differ, the first: %r" % (len(wrong), len(want), sorted(wrong.items())[0])


def test_the_table_shows_what_it_is_meant_to():
    """the recorded rows say what the contract says: a sanity check of the table itself, not of the library"""
    t = json.load(open(TABLE))
    assert len(t) > 700 and os.path.getsize(TABLE) < (1 << 20)
    rc = lambda rid: t[rid][0]      # noqa: E731
    st = lambda rid: t[rid][1]      # noqa: E731
    FEATURE, BAD_PTR, LEASE, BOOST, FMT = (api.ERROR_UNSUPPORTED_FEATURE, api.ERROR_BAD_PTR, api.ERROR_INSUFFICIENT_RESOURCE, api.ERROR_INVALID_DISPLAY_BOOST,
                                           api.ERROR_INVALID_OUTPUT_FORMAT)
    # the order of the gates: scale_denom and flags, then the arrays, then decode_to / boost, then the output format
    assert rc("jpeg_decode_batch_scaled/scale_3_n_negative") == FEATURE and rc("jpeg_decode_batch_scaled/to_0_n_negative") == BAD_PTR
    assert rc("jpeg_decode_batch_ex/flags_2_n_negative") == FEATURE and rc("jpeg_decode_batch/to_0_null_files") == BAD_PTR
    assert rc("jpeg_decode_batch/to_0_n_zero_null_arrays") == FEATURE and rc("jpeg_decode_batch/to2_n_zero_null_arrays") == api.NO_ERROR
    assert rc("jpeg_decode_scaled/host/scale_3_file_null") == FEATURE and rc("jpeg_decode_ex/host/flags_2_file_null") == FEATURE
    assert rc("jpeg_decode_ex/host/to_0_file_null") == BAD_PTR and rc("jpeg_decode_ex/host/to_0") == FEATURE
    assert rc("jpegr_decode_scaled_batch/scale_3_n_negative") == FEATURE and rc("jpegr_decode_md_batch/flags_2_boost_nan") == FEATURE
    assert rc("jpegr_decode_batch_ex/boost_below_1_n_negative") == BAD_PTR and rc("jpegr_decode_batch_ex/boost_below_1_fmt_5") == BOOST
    assert rc("jpegr_decode_batch_ex/fmt_5") == FMT and rc("jpegr_decode_batch_ex/n_zero_null_arrays_fmt_5") == FMT
    assert rc("jpegr_decode_ex/host/flags_2_file_null") == FEATURE and rc("jpegr_decode_ex/host/boost_below_1_file_null") == BAD_PTR
    # NaN is a display boost to the calls that read every metadata, and passes (as in the reference) through the others
    assert rc("jpegr_decode_md_batch/boost_nan") == BOOST == rc("jpegr_decode_scaled_batch/boost_nan") and rc("jpegr_decode_batch_ex/boost_nan") != BOOST
    # a refused file in the middle keeps its neighbours' size probes
    assert st("jpegr_decode_batch_ex/null_file_between_hlg") == [LEASE, BAD_PTR, LEASE]
    every = st("jpegr_decode_batch_ex/probes_of_every_file_hlg")
    assert every.count(LEASE) == 7 and api.ERROR_NO_IMAGES_FOUND in every and api.ERROR_GAIN_MAP_IMAGE_NOT_FOUND in every and api.ERROR_METADATA_ERROR in every
    assert st("jpegr_decode_batch/probes_of_every_file_hlg").count(LEASE) == 1      # without the flag: the sample alone (a 4:2:0 primary, a one-component map)
    assert st("jpeg_decode_batch/to2_probes_of_every_file").count(api.ERROR_RESOLUTION_MISMATCH) == 1
    # a map that cannot follow its primary image stops the file in front of its size probe, the SDR rendition does not ask
    assert set(st("jpegr_decode_scaled_batch/scale_2_map_cannot_follow_valid_dests")) == {api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR}
    assert st("jpegr_decode_scaled_batch/scale_2_probes_of_every_file_hlg")[0] == LEASE == st("jpegr_decode_scaled_batch/scale_2_probes_of_every_file_sdr")[1]
    # the rows that reach the device: the context's refusal, and under the round driver's rule a status for every file
    reach = [rid for rid, c in rows() if c.get("reach")]
    assert len(reach) > 50 and all(rid.startswith("jpegr_reach/") for rid in reach) and all(rc(rid) == LEASE for rid in reach)
    assert st("jpegr_reach/jpegr_decode_batch_ex/refused_between_hlg_host") == [LEASE, api.ERROR_NO_IMAGES_FOUND, LEASE, st("jpegr_decode_batch_ex/probes_of_every_file_hlg")[12], LEASE]
    assert st("jpegr_reach/jpegr_decode_md_batch/status_null") is None
    # the JPEG batch was on the round driver already: its rows that reach the device wrote status[] in the parent too
    assert st("jpeg_decode_batch_ex/to2_refused_and_reaching") == [api.UNKNOWN_ERROR, LEASE, BAD_PTR, LEASE, api.ERROR_RESOLUTION_MISMATCH]


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="the libuhdr_hip.so to run the rows against")
    ap.add_argument("--record", action="store_true", help="write the table (from a build of the commit the docstring names) instead of printing it")
    a = ap.parse_args()
    table = run_table(a.lib, a.record)
    if a.record:
        os.makedirs(os.path.dirname(TABLE), exist_ok=True)
        with open(TABLE, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + "\n}\n")      # a row per line
        print("%d rows -> %s" % (len(table), TABLE))
    else:
        json.dump(table, sys.stdout)
