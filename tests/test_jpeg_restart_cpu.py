"""Restart intervals without a GPU: tests/jpeg_restart_oracle.py (the transcoder every GPU test takes its expected bytes from) is
pinned to Pillow's libjpeg-turbo, byte for byte -- a failure there means the restatement is wrong, not the library; the argument
checks of the _opts entry points, which are made before the device is touched; the rows rule with its clamp; and the facts the
constructed images of tests/jpeg_restart_cases.py are there for, so that none of them drifts into testing nothing."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_restart_cases as RC
from tests import jpeg_restart_oracle as RO

# Pillow in a process of its own (it bundles its libjpeg).  Keys: <mode>_<w>x<h>_<quality>, modes L and RGB (4:2:0).  Every image is
# saved without intervals and, optimize off and on, with every setting of RC.SETTINGS.
_PIL_SCRIPT = r"""
import io, sys, json, numpy as np
from PIL import Image
d = np.load(sys.argv[1]); out = {}
settings = json.loads(sys.argv[3])
for key in d.files:
    mode, q = key.split("_")[0], int(key.split("_")[-1])
    im = Image.fromarray(d[key], mode)
    kw = {"subsampling": 2} if mode == "RGB" else {}
    b = io.BytesIO(); im.save(b, "JPEG", quality=q, **kw)
    out[key + "_base"] = np.frombuffer(b.getvalue(), np.uint8)
    for opt in (0, 1):
        for ri, rows in settings:
            b = io.BytesIO(); im.save(b, "JPEG", quality=q, optimize=bool(opt), restart_marker_blocks=ri, restart_marker_rows=rows, **kw)
            out["%s_%d_%d_%d" % (key, opt, ri, rows)] = np.frombuffer(b.getvalue(), np.uint8)
np.savez(sys.argv[2], **out)
"""


def run_pillow(arrays, tmp_path, settings=RC.SETTINGS):
    import json
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("Pillow not installed")
    np.savez(tmp_path / "in.npz", **arrays)
    subprocess.check_call([sys.executable, "-c", _PIL_SCRIPT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), json.dumps(settings)])
    res = np.load(tmp_path / "out.npz")
    return {k: res[k].tobytes() for k in res.files}


@pytest.fixture(scope="module")
def pillow_files(tmp_path_factory):
    rng = np.random.RandomState(21)
    arrays = {}
    for w, h in RC.SIZES:
        for q in RC.QUALITIES:
            arrays["L_%dx%d_%d" % (w, h, q)] = rng.randint(0, 256, (h, w)).astype(np.uint8)
            arrays["RGB_%dx%d_%d" % (w, h, q)] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    return arrays, run_pillow(arrays, tmp_path_factory.mktemp("pil"))


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_transcoder_equals_pillow(pillow_files, mode):
    arrays, files = pillow_files
    keys = [k for k in arrays if k.startswith(mode + "_")]
    assert len(keys) == len(RC.SIZES) * len(RC.QUALITIES)
    n = with_markers = 0
    for k in keys:
        base = files[k + "_base"]
        for opt in (0, 1):
            for ri, rows in RC.SETTINGS:
                want = files["%s_%d_%d_%d" % (k, opt, ri, rows)]
                assert RO.transcode_restart(base, ri, rows, bool(opt)) == want, (k, opt, ri, rows)
                with_markers += len(RO.packed(want)[1]) > 0
                n += 1
    assert n == 294 and with_markers > n // 2


def test_header_and_interval_layout(pillow_files):
    """what the rules say, read off Pillow's own files: DRI between the last DHT and SOS, markers counting modulo 8, none behind the
    last interval -- also where the MCUs are a multiple of the interval -- and DRI alone where the interval holds every MCU"""
    from tests import jpeg_optimize_oracle as JO
    _, files = pillow_files
    for opt in (0, 1):
        f = files["L_72x56_95_%d_3_0" % opt]                 # 63 MCUs = 21 intervals of 3
        kinds = [m for m, _, _ in JO.segments(f)]
        assert kinds[-2:] == [0xDD, 0xDA] and kinds[-3] == 0xC4 and kinds.count(0xDD) == 1
        a = JO.first_segment(f, 0xDD)
        assert f[a:a + 6] == b"\xff\xdd\x00\x04\x00\x03"
        assert len(RO.packed(f)[1]) == 20
        whole = files["L_72x56_95_%d_65535_0" % opt]
        assert len(RO.packed(whole)[1]) == 0
        a = JO.first_segment(whole, 0xDD)
        base = RO.transcode_restart(files["L_72x56_95_base"], 0, 0, bool(opt))
        assert whole[:a] + whole[a + 6:] == base and whole[a:a + 6] == b"\xff\xdd\x00\x04\xff\xff"
    rows = files["RGB_130x66_95_0_0_2"]                      # 9 x 5 MCUs: rows of 9, two at a time
    a = JO.first_segment(rows, 0xDD)
    assert rows[a + 4:a + 6] == b"\x00\x12" and len(RO.packed(rows)[1]) == 2


# ---- argument checks, made before the device is touched ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _all_four(api, opts):
    """the four _opts calls with n = -1 and NULL arrays (BAD_PTR for any opts that pass)"""
    lib = api.load()
    o = None if opts is None else C.byref(opts)
    return [lib.uhdr_hip_jpeg_encode_batch_opts(-1, None, None, None, None, None, None, None, None, o, api.MEM_HOST, None),
            lib.uhdr_hip_jpeg_encode_rgb_batch_opts(-1, None, None, None, None, None, None, o, api.MEM_HOST, None),
            lib.uhdr_hip_jpeg_encode_rgba420_batch_opts(-1, None, None, None, None, None, None, None, None, o, api.MEM_HOST, None),
            lib.uhdr_hip_jpegr_encode_batch_opts(-1, None, None, api.TF_HLG, 90, None, None, None, None, None, None, o, api.MEM_HOST, None)]


def test_bad_options_are_refused_before_anything_else(api):
    bad = []
    for size in (0, 12, 15, 17, 20):
        o = api.encode_opts(0, 8, 0)
        o.struct_size = size
        bad.append(o)
    bad.append(api.encode_opts(0, 65536, 0))
    bad.append(api.encode_opts(1, 1 << 31, 0))
    bad.append(api.encode_opts(0, 65536, 1))                 # (the rows would override it: the field is refused all the same)
    for flags in (2, 3, 4, 0xFFFFFFFF, 1 << 30, 1 << 31):
        bad.append(api.encode_opts(flags, 0, 0))
        bad.append(api.encode_opts(flags, 8, 0))
    for o in bad:
        assert _all_four(api, o) == [api.ERROR_UNSUPPORTED_FEATURE] * 4, (o.struct_size, o.flags, o.restart_interval)


def test_good_options_and_null_reach_the_pointer_checks(api):
    for o in (None, api.encode_opts(), api.encode_opts(1), api.encode_opts(0, 65535, 0), api.encode_opts(1, 1, 0), api.encode_opts(0, 0, 1 << 31)):
        assert _all_four(api, o) == [api.ERROR_BAD_PTR] * 4
    lib = api.load()
    assert lib.uhdr_hip_jpeg_encode_batch_opts(0, None, None, None, None, None, None, None, None, None, api.MEM_HOST, None) == 0
    assert lib.uhdr_hip_jpeg_encode_batch_opts(0, None, None, None, None, None, None, None, None, C.byref(api.encode_opts(1, 7, 0)), api.MEM_HOST, None) == 0
    # the _ex calls' own refusals are where they were
    assert lib.uhdr_hip_jpeg_encode_batch_ex(-1, None, None, None, None, None, None, None, None, 2, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_FEATURE


def _mcus(api, width, mcu_width, ri, rows):
    lib = api.load()
    out = C.c_uint32(0xDEAD)
    o = api.encode_opts(0, ri, rows)
    assert lib.uhdr_hip_jpeg_restart_mcus(C.byref(o), width, mcu_width, C.byref(out)) == 0
    return out.value


def test_rows_rule_and_its_clamp(api):
    lib = api.load()
    assert _mcus(api, 65535, 8, 0, 8) == 65535 and 8192 * 8 == 65536     # one plane 65535 wide: 8192 MCUs a row, eight rows clamped
    assert _mcus(api, 65535, 8, 0, 7) == 8192 * 7
    assert _mcus(api, 65535, 16, 0, 15) == 4096 * 15 and _mcus(api, 65535, 16, 0, 16) == 65535
    assert _mcus(api, 130, 16, 5, 2) == 18 and _mcus(api, 130, 8, 5, 2) == 34 and _mcus(api, 130, 8, 5, 0) == 5    # rows override the interval
    assert _mcus(api, 17, 8, 0, 0) == 0 and _mcus(api, 17, 16, 0, 1 << 31) == 65535
    for w, mw, ri, rows in ((130, 16, 5, 2), (65535, 8, 0, 8), (8, 8, 9, 0), (17, 8, 0, 3)):
        assert _mcus(api, w, mw, ri, rows) == RO.restart_mcus(ri, rows, (w + mw - 1) // mw)
    out = C.c_uint32(0xDEAD)
    assert lib.uhdr_hip_jpeg_restart_mcus(C.byref(api.encode_opts(0, 65536, 0)), 64, 8, C.byref(out)) == api.ERROR_UNSUPPORTED_FEATURE
    assert lib.uhdr_hip_jpeg_restart_mcus(None, 64, 8, C.byref(out)) == 0 and out.value == 0
    out.value = 0xDEAD
    assert lib.uhdr_hip_jpeg_restart_mcus(C.byref(api.encode_opts(0, 3, 0)), 64, 12, C.byref(out)) == api.ERROR_RESOLUTION_MISMATCH
    assert lib.uhdr_hip_jpeg_restart_mcus(C.byref(api.encode_opts(0, 3, 0)), 64, 8, None) == api.ERROR_BAD_PTR and out.value == 0xDEAD


@pytest.mark.parametrize("w,h,gray", [(65500, 65500, True), (40000, 32008, True), (29216, 29216, False)])
def test_an_image_too_large_for_32_bit_stream_offsets_is_refused(api, w, h, gray):
    """more than 20 000 000 blocks with intervals (refused sizes only: an accepted one would be compressed from these pointers)"""
    lib = api.load()
    nblk = ((w + 7) // 8) * ((h + 7) // 8) if gray else ((w + 15) // 16) * ((h + 15) // 16) * 6
    assert nblk > 20000000
    keep = np.zeros(64, np.uint8)
    img = api.Image()
    img.data = img.chroma_data = keep.ctypes.data
    img.width, img.height = w, h
    img.pixelFormat = api.PIX_FMT_MONOCHROME if gray else api.PIX_FMT_YUV420
    q = (C.c_int * 1)(90)
    out, cap, n, st = (C.c_void_p * 1)(keep.ctypes.data), (C.c_size_t * 1)(64), (C.c_size_t * 1)(0), (C.c_int * 1)(12345)
    for o in (api.encode_opts(0, 8, 0), api.encode_opts(0, 0, 1)):
        rc = lib.uhdr_hip_jpeg_encode_batch_opts(1, C.byref(img), q, None, None, out, cap, n, st, C.byref(o), api.MEM_DEVICE, None)
        assert rc == api.ERROR_UNSUPPORTED_FEATURE and st[0] == api.ERROR_UNSUPPORTED_FEATURE and n[0] == 0


# ---- the facts of the constructed images ------------------------------------------------------------------------------------------
def test_facts_many_intervals(orc):
    it, ri = RC.many_intervals()
    base = RC.base_file(orc, it)
    want = RO.transcode_restart(base, ri)
    pk, marks = RO.packed(want)
    assert len(marks) == 2055 and marks == sorted(marks)                     # (packed() has checked that the numbering wraps)
    assert sum(pk[m - 1] == 0xFF for m in marks) >= 1                        # FF 00 FF Dn in the file: measured 274
    assert sum(m % 64 == 63 for m in marks) >= 1                             # 0xFF last in a chunk of the stuffing kernels: measured 33
    assert sum(m % 64 == 62 for m in marks) >= 1
    pads = RO.interval_pads(base, ri)
    assert len(pads) == 2056 and set(pads) == set(range(8))                  # every padding, 0 and 7 among them
    from tests import jpeg_optimize_oracle as JO
    assert want.count(b"\xff\x00", JO.first_segment(want, 0xDA)) > 274       # data 0xFF elsewhere as well


@pytest.mark.parametrize("seed", [RC.STEERED_DATA_PAIR, RC.STEERED_FF_AT_EDGE, RC.STEERED_DN_AT_EDGE])
def test_facts_steered(orc, seed):
    """If this NumPy gives other pixels, or this oracle other streams, the seeds are to be searched again and recorded in
    tests/jpeg_restart_cases.py."""
    it, ri = RC.steered(seed)
    pk, marks = RO.packed(RO.transcode_restart(RC.base_file(orc, it), ri))
    assert len(marks) == (65 * 8 - 1) // 5 and len(pk) > 3 * 16384
    ms = set(marks)
    pairs = [i for i in range(len(pk) - 1) if pk[i] == 0xFF and 0xD0 <= pk[i + 1] <= 0xD7 and i not in ms]
    if seed == RC.STEERED_DATA_PAIR:
        assert pairs
    elif seed == RC.STEERED_FF_AT_EDGE:
        assert 3 * 16384 - 1 in ms
    else:
        assert 3 * 16384 - 2 in ms


def test_facts_steered_images_equal_pillow(orc, tmp_path):
    """the steered streams are libjpeg-turbo's own: the oracle's base file transcoded equals Pillow's file with the same setting"""
    arrays, items = {}, {}
    for seed in (RC.STEERED_DATA_PAIR, RC.STEERED_FF_AT_EDGE, RC.STEERED_DN_AT_EDGE):
        it, ri = RC.steered(seed)
        items["L_seed%d_100" % seed] = it
        arrays["L_seed%d_100" % seed] = it["yb"].reshape(it["h"], it["w"])
    files = run_pillow(arrays, tmp_path, [(RC.STEERED_RI, 0)])
    for k, it in items.items():
        assert RO.transcode_restart(RC.base_file(orc, it), RC.STEERED_RI) == files["%s_0_%d_0" % (k, RC.STEERED_RI)], k
