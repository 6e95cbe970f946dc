"""No GPU: the statuses the JPEG and JPEG/R encode batches decide before they touch the device.

A process that never calls uhdr_hip_init gets as far as a batch call's context lease and is refused there, so everything a call
decides before that point can be observed without a device: the order of the call-level checks (options, pointers, quality, sampling,
tonemap_op, boost_scope), which of them fail the whole call without writing a status, and every per-file check with its place among
valid files (a valid file comes back with the lease's refusal).  rows() builds the argument sets for the 22 forms of these calls --
the 13 plain-JPEG batch forms (uhdr_hip_jpeg_encode_rgba_batch_opts counts once per sampling) and the JPEG/R batches of planes and of
packed pixels.  Every row is run in one child process, which never initialises a device (so the table is the same on a machine that
has one), with the status array pre-filled with 7 and out_size with 0xABCDEF to show what a call wrote.  A row of the table is
[return code, status array, [index, value] of every out_size entry the call wrote], one row per line.

The expected table, tests/golden/encode_contract/table.json, was recorded from a library built from commit 4758176 ("JPEG encoder:
4:4:4, 4:2:2 and 4:4:0 files from planes and from RGBA"), the parent of the change that put these calls on one round driver:

    python tests/test_jpeg_encode_batch_contract_cpu.py --lib <that build's libuhdr_hip.so> --record

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

TABLE = os.path.join(ROOT, "tests", "golden", "encode_contract", "table.json")
SENT, SIZE_SENT = 7, 0xABCDEF
NULL = "NULL"                        # an override that passes a NULL pointer
OPTIMIZE_LIMIT_SIDE = 40000          # 40000 x 40000 is above jpeg::kMaxOptimizeBlocks (15,873,015 blocks) in every geometry
_MEM = np.zeros((1 << 16) + 64, np.uint8)
P = (_MEM.ctypes.data + 63) & ~63    # host memory behind every valid image: no row reads it, a stray one would not fault
_OUT = np.zeros(1 << 14, np.uint8)
CAP = 4096


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def _img(make, *a, **fields):
    im = make(*a)
    for k, v in fields.items():
        setattr(im, k, v)
    return im


def _file(img, sdr=None, **kw):
    f = dict(img=img, sdr=sdr, q=90, icc=None, exif=None, out=True, cap=CAP, peak=0.0)
    f.update(kw)
    return f


def _edit(which, **fields):
    def go(f):
        for k, v in fields.items():
            setattr(f[which], k, v)
    return go


def _set(**kw):
    return lambda f: f.update(kw)


# per-file errors: name -> (what it does to a valid file, mem_space it needs (None: host), option it needs (None / "optimize" / "restart"))
COMMON_OUT = {"out_null_with_capacity": (_set(out=False), None, None)}
BIG = dict(width=OPTIMIZE_LIMIT_SIDE, height=OPTIMIZE_LIMIT_SIDE, luma_stride=OPTIMIZE_LIMIT_SIDE)
PLANES_ERRORS = dict(COMMON_OUT, **{
    "data_null": (_edit("img", data=None), None, None),
    "chroma_null": (_edit("img", chroma_data=None), None, None),
    "odd_width": (_edit("img", width=15), None, None),
    "zero_height": (_edit("img", height=0), None, None),
    "above_65500": (_edit("img", width=65502, luma_stride=65502, chroma_stride=32751), None, None),
    "optimize_above_limit": (_edit("img", chroma_stride=OPTIMIZE_LIMIT_SIDE // 2, **BIG), None, "optimize"),
    "restart_above_limit": (_edit("img", chroma_stride=OPTIMIZE_LIMIT_SIDE // 2, **BIG), None, "restart"),
})
SAMPLED_ERRORS = {          # uhdr_hip_jpeg_encode_planes_batch_opts alone: a YUV444 image among the files
    "s444_chroma_null": (_set(img=None, mk=("444", dict(chroma_data=None))), None, None),
    "s444_chroma_stride_short": (_set(img=None, mk=("444", dict(chroma_stride=16))), None, None),
    "s444_luma_stride_short": (_set(img=None, mk=("444", dict(luma_stride=16))), None, None),
    "s444_zero_width": (_set(img=None, mk=("444", dict(width=0))), None, None),
    "s444_above_65500": (_set(img=None, mk=("444", dict(height=65501))), None, None),
    "s444_optimize_above_limit": (_set(img=None, mk=("444", dict(chroma_stride=OPTIMIZE_LIMIT_SIDE, **BIG))), None, "optimize"),
    "s444_restart_above_limit": (_set(img=None, mk=("444", dict(chroma_stride=OPTIMIZE_LIMIT_SIDE, **BIG))), None, "restart"),
}
RGBA_ERRORS = dict(COMMON_OUT, **{
    "data_null": (_edit("img", data=None), None, None),
    "misaligned_device_pointer": (_edit("img", data=P + 2), api.MEM_DEVICE, None),
    "misaligned_host_pointer_is_fine": (_edit("img", data=P + 2), None, None),
    "wrong_pixel_format": (_edit("img", pixelFormat=api.PIX_FMT_YUV420), None, None),
    "zero_width": (_edit("img", width=0), None, None),
    "zero_height": (_edit("img", height=0), None, None),
    "above_65500": (_edit("img", width=65501, luma_stride=65501), None, None),
    "stride_below_width": (_edit("img", luma_stride=16), None, None),
    "stride_above_int_pitch": (_edit("img", luma_stride=(2 ** 31 - 1) // 4 + 1), None, None),
    "optimize_above_limit": (_edit("img", **BIG), None, "optimize"),     # dimensions only: the pointer is never read
    "restart_above_limit": (_edit("img", **BIG), None, "restart"),
})
JPEGR_ERRORS = {
    "hdr_data_null": (_edit("img", data=None), None, None),
    "odd_width": (_edit("img", width=15), None, None),
    "below_8": (_edit("img", height=6), None, None),
    "above_8192": (_edit("img", width=8194, luma_stride=8194), None, None),
    "hdr_gamut_unspecified": (_edit("img", colorGamut=api.CG_UNSPECIFIED), None, None),
    "hdr_stride_short": (_edit("img", luma_stride=8), None, None),
    "out_null": (_set(out=False), None, None),
    "exif_null_with_size": (_set(exif=(None, 12)), None, None),
}
JPEGR_SDR_ERRORS = {
    "sdr_data_null": (_edit("sdr", data=None), None, None),
    "sdr_stride_short": (_edit("sdr", luma_stride=8), None, None),
    "sdr_size_differs": (_edit("sdr", width=32, luma_stride=32), None, None),
    "sdr_gamut_unknown": (_edit("sdr", colorGamut=7), None, None),
}
PACKED_ERRORS = {
    "hdr_pixel_format": (_edit("img", pixelFormat=api.PIX_FMT_RGBA8888), None, None),
    "hdr_misaligned_device_pointer": (_edit("img", data=P + 2), api.MEM_DEVICE, None),
}
PACKED_SDR_ERRORS = {
    "sdr_pixel_format": (_edit("sdr", pixelFormat=api.PIX_FMT_YUV420), None, None),
    "sdr_misaligned_device_pointer": (_edit("sdr", data=P + 2), api.MEM_DEVICE, None),
}
PEAK_ERROR = {"peak_negative": (_set(peak=-1.0), None, None)}


def _valid(family):
    if family == "planes":
        return _file(_img(api.yuv420_image, P, 16, 16, api.CG_BT709))
    if family == "rgba":
        return _file(_img(api.rgba8888_image, P, 17, 9, api.CG_BT709))
    if family == "jpegr":
        return _file(_img(api.p010_image, P, 16, 16, api.CG_BT2100), _img(api.yuv420_image, P + 1024, 16, 16, api.CG_BT709))
    return _file(_img(api.rgba1010102_image, P, 16, 16, api.CG_BT2100), _img(api.rgba8888_image, P + 1024, 16, 16, api.CG_BT709))


def _make(family, error=None):
    f = _valid(family)
    if error is not None:
        error(f)
        if f["img"] is None:     # a sampled image in place of the family's own
            kind, fields = f.pop("mk")
            f["img"] = _img(api.ycbcr_image, P, 17, 9, api.CG_UNSPECIFIED, api.PIX_FMT_YUV444, **fields)
    return f


# ---- the 22 forms -----------------------------------------------------------------------------------------------------------------------
_PLAIN = ["n", "images", "quality", "icc", "icc_size", "out", "out_capacity", "out_size", "status"]
_RGB = ["n", "images", "quality", "out", "out_capacity", "out_size", "status"]
_JR = ["n", "images", "sdr", "hdr_tf", "quality", "exif", "exif_size", "out", "out_capacity", "out_size"]
_JR0 = ["n", "images", "hdr_tf", "quality", "exif", "exif_size", "out", "out_capacity", "out_size"]
_END = ["mem_space", "stream"]


def _form(fid, fn, order, family, errors, options=None, sdr=None, **fixed):
    return dict(id=fid, fn=fn, order=order + _END, family=family, errors=errors, options=options, sdr=sdr, fixed=fixed)


PLANES_ALL = dict(PLANES_ERRORS, **SAMPLED_ERRORS)
JR1 = dict(JPEGR_ERRORS, **JPEGR_SDR_ERRORS)
PK = dict(JPEGR_ERRORS, **PACKED_ERRORS)
PK1 = dict(PK, **dict(JPEGR_SDR_ERRORS, **PACKED_SDR_ERRORS))
FORMS = [
    _form("planes", "uhdr_hip_jpeg_encode_batch", _PLAIN, "planes", PLANES_ERRORS),
    _form("planes_ex", "uhdr_hip_jpeg_encode_batch_ex", _PLAIN + ["flags"], "planes", PLANES_ERRORS, "flags"),
    _form("planes_opts", "uhdr_hip_jpeg_encode_batch_opts", _PLAIN + ["opts"], "planes", PLANES_ERRORS, "opts"),
    _form("planes_any", "uhdr_hip_jpeg_encode_planes_batch_opts", _PLAIN + ["opts"], "planes", PLANES_ALL, "opts"),
    _form("rgb", "uhdr_hip_jpeg_encode_rgb_batch", _RGB, "rgba", RGBA_ERRORS),
    _form("rgb_ex", "uhdr_hip_jpeg_encode_rgb_batch_ex", _RGB + ["flags"], "rgba", RGBA_ERRORS, "flags"),
    _form("rgb_opts", "uhdr_hip_jpeg_encode_rgb_batch_opts", _RGB + ["opts"], "rgba", RGBA_ERRORS, "opts"),
    _form("rgba420", "uhdr_hip_jpeg_encode_rgba420_batch", _PLAIN, "rgba", RGBA_ERRORS),
    _form("rgba420_ex", "uhdr_hip_jpeg_encode_rgba420_batch_ex", _PLAIN + ["flags"], "rgba", RGBA_ERRORS, "flags"),
    _form("rgba420_opts", "uhdr_hip_jpeg_encode_rgba420_batch_opts", _PLAIN + ["opts"], "rgba", RGBA_ERRORS, "opts"),
    _form("rgba_444", "uhdr_hip_jpeg_encode_rgba_batch_opts", _PLAIN + ["sampling", "opts"], "rgba", RGBA_ERRORS, "opts", sampling=api.PIX_FMT_YUV444),
    _form("rgba_422", "uhdr_hip_jpeg_encode_rgba_batch_opts", _PLAIN + ["sampling", "opts"], "rgba", RGBA_ERRORS, "opts", sampling=api.PIX_FMT_YUV422),
    _form("rgba_420", "uhdr_hip_jpeg_encode_rgba_batch_opts", _PLAIN + ["sampling", "opts"], "rgba", RGBA_ERRORS, "opts", sampling=api.PIX_FMT_YUV420),
    _form("jpegr", "uhdr_hip_jpegr_encode_batch", _JR + ["status"], "jpegr", JR1, sdr="optional"),
    _form("jpegr_ex", "uhdr_hip_jpegr_encode_batch_ex", _JR + ["status", "flags"], "jpegr", JR1, "flags", sdr="optional"),
    _form("jpegr_opts", "uhdr_hip_jpegr_encode_batch_opts", _JR + ["status", "opts"], "jpegr", JR1, "opts", sdr="optional"),
    _form("rgbmap", "uhdr_hip_jpegr_encode_rgbmap_batch", _JR + ["status"], "jpegr", JR1, sdr="optional"),
    _form("scaled", "uhdr_hip_jpegr_encode_scaled_batch", _JR + ["status", "rgb_map", "map_scale"], "jpegr", JR1, sdr="optional", rgb_map=0, map_scale=2),
    _form("packed", "uhdr_hip_jpegr_encode_packed_batch", _JR + ["status", "rgb_map"], "packed", PK1, sdr="required", rgb_map=0),
    _form("packed_sampling", "uhdr_hip_jpegr_encode_packed_sampling_batch", _JR + ["status", "rgb_map", "primary_sampling", "opts"], "packed", PK1, "opts",
          sdr="required", rgb_map=1, primary_sampling=api.PIX_FMT_YUV444),
    _form("packed_api0", "uhdr_hip_jpegr_encode_packed_api0_batch", _JR0 + ["metadata", "status", "tonemap_op", "peaks", "rgb_map"], "packed",
          dict(PK, **PEAK_ERROR), tonemap_op=api.TONEMAP_REINHARD_MAXRGB, rgb_map=0),
    _form("packed_adaptive", "uhdr_hip_jpegr_encode_packed_adaptive_batch", _JR + ["metadata", "status", "peaks", "rgb_map", "boost_scope"], "packed", PK1,
          sdr="optional", rgb_map=0, boost_scope=api.BOOST_PER_CALL),
    _form("adaptive", "uhdr_hip_jpegr_encode_adaptive_batch", _JR + ["metadata", "status", "boost_scope"], "jpegr", JR1, sdr="optional",
          boost_scope=api.BOOST_PER_IMAGE),
    _form("api0_tonemapped", "uhdr_hip_jpegr_encode_api0_tonemapped_batch", _JR0 + ["metadata", "status", "tonemap_op", "peaks", "boost_scope"], "jpegr",
          dict(JPEGR_ERRORS, **PEAK_ERROR), tonemap_op=api.TONEMAP_REINHARD_MAXRGB, boost_scope=-1),
]
assert len(FORMS) == 24 and len({f["fn"] for f in FORMS}) == 22      # rgba_batch_opts once per sampling


def _opts(kind):
    o = api.encode_opts()
    if kind == "optimize":
        o.flags = api.ENCODE_OPTIMIZE_HUFFMAN
    elif kind == "restart":
        o.restart_in_rows = 1
    elif kind == "bad_struct_size":
        o.struct_size = 12
    elif kind == "bad_flag":
        o.flags = 2
    elif kind == "restart_interval_65536":
        o.restart_interval = 65536
    return o


def rows():
    """(row id, form, [per-file error name or None], {argument: override}) for every row of the table"""
    out = []
    for form in FORMS:
        fid, order = form["id"], form["order"]

        def add(name, files=(None, None, None), **over):
            out.append(("%s/%s" % (fid, name), form, list(files), over))
        first = sorted(form["errors"])[0]
        add("valid")
        add("n_negative", n=-1)
        add("n_zero_all_null", files=(), images=NULL, quality=NULL, out=NULL, out_capacity=NULL, out_size=NULL, status=NULL)
        for p in ("images", "sdr", "quality", "icc", "exif", "out", "out_capacity", "out_size", "status", "metadata", "peaks"):
            if p in order and not (p == "quality" and "hdr_tf" in order):
                add("null_%s" % p, **{p: NULL})
                add("null_%s_file0_bad" % p, files=(first, None, None), **{p: NULL})
        for p, sizes in (("icc", "icc_size"), ("exif", "exif_size")):
            if p in order:
                add("%s_without_sizes" % p, **{p: "given", sizes: NULL})
                add("%s_with_sizes" % p, **{p: "given"})
                add("%s_and_sizes_null" % p, **{p: NULL, sizes: NULL})
        for q in (-1, 101):             # the quality gate, in a call whose file 0 is also bad
            add("quality_%d_file0_bad" % q, files=(first, None, None), quality=q)
            add("quality_%d_null_out" % q, quality=q, out=NULL)
        if form["options"] == "flags":
            add("bad_flag", flags=2)
            add("bad_flag_null_images_quality_101", flags=2, images=NULL, quality=101)
            add("optimize", flags=api.ENCODE_OPTIMIZE_HUFFMAN)
        if form["options"] == "opts":
            for kind in ("bad_struct_size", "bad_flag", "restart_interval_65536"):
                add("opts_%s" % kind, opts=kind)
                add("opts_%s_null_images_quality_101" % kind, opts=kind, images=NULL, quality=101)
            add("opts_optimize_restart_rows", opts="optimize")
        if "sampling" in order or "primary_sampling" in order:
            key = "sampling" if "sampling" in order else "primary_sampling"
            for s in (api.PIX_FMT_YUV440, api.PIX_FMT_MONOCHROME, 99, -1):
                add("unknown_sampling_%d" % s, **{key: s})
                add("unknown_sampling_%d_null_images" % s, **{key: s, "images": NULL})
                add("unknown_sampling_%d_bad_opts" % s, **{key: s, "opts": "bad_flag"})
                add("unknown_sampling_%d_quality_101" % s, **{key: s, "quality": 101})
        if "boost_scope" in order:
            for s in (2, -2, 99):
                add("unknown_scope_%d" % s, boost_scope=s)
                add("unknown_scope_%d_quality_101" % s, boost_scope=s, quality=101)
                add("unknown_scope_%d_null_out" % s, boost_scope=s, out=NULL)
            add("scope_per_image", boost_scope=api.BOOST_PER_IMAGE)
        if "tonemap_op" in order:
            for t in (api.TONEMAP_SHIFT, 2, -1):
                add("tonemap_op_%d" % t, tonemap_op=t)
                add("tonemap_op_%d_quality_101" % t, tonemap_op=t, quality=101)
                add("tonemap_op_%d_unknown_scope" % t, tonemap_op=t, boost_scope=99)
        if "map_scale" in order:
            for m in (0, 129, 3, 4):
                add("map_scale_%d" % m, map_scale=m)
                add("map_scale_%d_quality_101" % m, map_scale=m, quality=101)
        if "hdr_tf" in order:
            add("unknown_transfer", hdr_tf=9)
            add("linear_transfer", hdr_tf=api.TF_LINEAR)
        if form["sdr"] == "optional":
            add("api0_no_sdr_images", sdr=NULL)
        for mem in (api.MEM_DEVICE, api.MEM_DEVICE_TO_HOST, api.MEM_HOST_TO_DEVICE):
            add("valid_mem_space_%d" % mem, mem_space=mem)
        # one file per per-file error among valid files, as the first, the middle and the last file
        for name in sorted(form["errors"]):
            _, mem, need = form["errors"][name]
            if need is not None and form["options"] is None:
                continue
            if need == "restart" and form["options"] == "flags":
                continue
            over = {}
            if mem is not None:
                over["mem_space"] = mem
            if need is not None:
                over[form["options"]] = api.ENCODE_OPTIMIZE_HUFFMAN if form["options"] == "flags" else need
            for pos in range(3):
                add("file%d_%s" % (pos, name), files=[name if k == pos else None for k in range(3)], **over)
        names = sorted(n for n in form["errors"] if form["errors"][n][1] is None and form["errors"][n][2] is None)
        for k in range(0, len(names) - 2, 3):      # and batches of errors alone
            add("files_%s" % "_".join(names[k:k + 3]), files=names[k:k + 3])
    assert len({r[0] for r in out}) == len(out)
    return out


def run_row(lib, form, files, over):
    """one call: [its return, the status array behind it (7: not written), [index, value] of every out_size entry it wrote]"""
    fl = [_make(form["family"], form["errors"][e][0] if e is not None else None) for e in files]
    n = len(fl)
    keep = []

    def arr(ctype, values):
        a = (ctype * max(n, 1))(*values)
        keep.append(a)
        return a
    blob = np.zeros(16, np.uint8)
    given = over.get("icc") == "given" or over.get("exif") == "given"
    side = [f["exif"] if f["exif"] is not None else ((blob.ctypes.data, 12) if given else (None, 0)) for f in fl]
    status, size = arr(C.c_int, [SENT] * n), arr(C.c_size_t, [SIZE_SENT] * n)
    vals = dict(
        n=n, images=api.image_array([f["img"] for f in fl]) if n else None,
        sdr=api.image_array([f["sdr"] for f in fl]) if n and fl[0]["sdr"] is not None else None,
        quality=arr(C.c_int, [f["q"] for f in fl]), hdr_tf=api.TF_HLG,
        out=arr(C.c_void_p, [_OUT.ctypes.data + CAP * k if f["out"] else None for k, f in enumerate(fl)]),
        out_capacity=arr(C.c_size_t, [f["cap"] for f in fl]), out_size=size, status=status,
        metadata=(api.Metadata * max(n, 1))(), peaks=arr(C.c_float, [f["peak"] for f in fl]),
        icc=None, icc_size=None, exif=None, exif_size=None, flags=0, opts=None, mem_space=api.MEM_HOST, stream=None)
    if any(f["exif"] is not None for f in fl) or given:
        for p, s in (("icc", "icc_size"), ("exif", "exif_size")):
            vals[p], vals[s] = arr(C.c_void_p, [x[0] for x in side]), arr(C.c_size_t, [x[1] for x in side])
    if "hdr_tf" in form["order"]:
        vals["quality"] = 90
    vals.update(form["fixed"])
    for k, v in over.items():
        if v == NULL:
            if not (k == "quality" and "hdr_tf" in form["order"]):      # (the JPEG/R calls take one quality, by value)
                vals[k] = None
        elif v == "given":
            pass
        elif k == "opts":
            o = _opts(v)
            keep.append(o)
            vals[k] = C.byref(o)
        elif k == "quality" and "hdr_tf" not in form["order"]:
            vals[k][min(1, n - 1)] = v      # file 1's: file 0 is the one with the per-file error
        else:
            vals[k] = v
    rc = getattr(lib, form["fn"])(*[vals[p] for p in form["order"]])
    return [rc, list(status)[:n], [[k, v] for k, v in enumerate(list(size)[:n]) if v != SIZE_SENT]]


def run_table(lib_path):
    """every row against the library at lib_path, in this process: the caller makes sure no device has been initialised in it"""
    lib = C.CDLL(lib_path)
    for name, (res, args) in api.SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return {rid: run_row(lib, form, files, over) for rid, form, files, over in rows()}


def test_encode_batches_answer_as_the_recorded_table_says():
    """the library under test, in a child process that initialises no device, against the table recorded from commit 4758176"""
    want = json.load(open(TABLE))
    got = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--lib", api.LIB_PATH], cwd=ROOT))
    assert sorted(got) == sorted(want) == sorted(r[0] for r in rows())
    wrong = {rid: (got[rid], want[rid]) for rid in want if got[rid] != want[rid]}
    assert not wrong, "%d of %d rows differ, the first: %r" % (len(wrong), len(want), sorted(wrong.items())[0])


def test_the_table_shows_what_it_is_meant_to():
    """the recorded rows say what the issue's contract says: a sanity check of the table itself, not of the library"""
    t = json.load(open(TABLE))      # row: [rc, statuses, written out_size entries]
    assert len(t) > 1500 and os.path.getsize(TABLE) < (1 << 17)

    def untouched(r):
        return set(r[1]) <= {SENT} and r[2] == []
    for fid in ("rgb", "rgba420", "rgba_444", "rgba_422", "rgba_420"):
        for q in (-1, 101):      # the RGBA families: the quality gate fails the whole call and writes no status
            r = t["%s/quality_%d_file0_bad" % (fid, q)]
            assert r[0] == api.ERROR_INVALID_QUALITY_FACTOR and untouched(r)
    r = t["planes/quality_101_file0_bad"]   # the planes family has no such gate: file 0 has its own error, the others reach the lease
    assert r[1] == [api.ERROR_RESOLUTION_MISMATCH, api.ERROR_INSUFFICIENT_RESOURCE, api.ERROR_INSUFFICIENT_RESOURCE]
    assert t["rgba_444/file1_optimize_above_limit"][1] == [api.ERROR_INSUFFICIENT_RESOURCE, api.ERROR_UNSUPPORTED_FEATURE, api.ERROR_INSUFFICIENT_RESOURCE]
    assert t["rgba_422/unknown_sampling_99_null_images"][0] == api.ERROR_UNSUPPORTED_FEATURE
    assert t["planes_ex/bad_flag_null_images_quality_101"][0] == api.ERROR_UNSUPPORTED_FEATURE
    assert t["adaptive/unknown_scope_99_quality_101"][0] == api.ERROR_INVALID_QUALITY_FACTOR
    assert t["rgba420/file2_misaligned_device_pointer"][1][2] == api.ERROR_BAD_PTR
    assert all(untouched(r) for r in t.values() if r[0] == api.ERROR_INVALID_QUALITY_FACTOR)


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
