"""Optimised Huffman tables without a GPU: tests/jpeg_optimize_oracle.py (the transcoder every GPU test takes its expected bytes
from) is pinned to Pillow's libjpeg-turbo, byte for byte; and the argument checks of the _ex entry points and of
uhdr_hip_jpeg_optimal_table, which are made before the device is touched."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_optimize_oracle as JO

QUALITIES = (1, 50, 85, 100)
CONTENTS = ("noise", "ramp", "flat", "bw")
SIZES = ((64, 48), (33, 17), (7, 5))          # even, odd, below one MCU
MCU_SIZES = ((64, 48), (16, 16))

# Pillow in a process of its own (it bundles its libjpeg).  Keys: <mode>_<content>_<w>x<h>_<quality>; modes: rgb420 / rgb444 (an RGB
# image at subsampling 2 / 0), gray ("L"), ycc (a YCbCr image whose chroma is replicated 2x2, subsampling 2), fib (the gray image
# whose AC table needs the length limit, quality 50).  Every image is saved with optimize False and True.
_PIL_SCRIPT = r"""
import io, sys, numpy as np
from PIL import Image
d = np.load(sys.argv[1]); out = {}
for key in d.files:
    mode, q = key.split("_")[0], int(key.split("_")[-1])
    a = d[key]
    if mode in ("gray", "fib"):
        im, kw = Image.fromarray(a, "L"), {}
    elif mode == "ycc":
        im, kw = Image.fromarray(a, "YCbCr"), {"subsampling": 2}
    else:
        im, kw = Image.fromarray(a, "RGB"), {"subsampling": 2 if mode == "rgb420" else 0}
    for opt in (False, True):
        b = io.BytesIO(); im.save(b, "JPEG", quality=q, optimize=opt, **kw)
        out[key + ("_opt" if opt else "_std")] = np.frombuffer(b.getvalue(), np.uint8)
np.savez(sys.argv[2], **out)
"""


def content(kind, shape, rng):
    h, w = shape[:2]
    if kind == "noise":
        return rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "flat":
        return np.full(shape, 77, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((xx * 3 + yy * 5) % 256) if kind == "ramp" else (((xx + yy) & 1) * 255)
    a = a.astype(np.uint8)
    return a if len(shape) == 2 else np.stack([a, np.roll(a, 1, 0), 255 - a][:shape[2]], -1).copy()


def _run_pillow(arrays, tmp_path):
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("Pillow not installed")
    np.savez(tmp_path / "in.npz", **arrays)
    subprocess.check_call([sys.executable, "-c", _PIL_SCRIPT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")])
    res = np.load(tmp_path / "out.npz")
    return {k: res[k].tobytes() for k in res.files}


@pytest.fixture(scope="module")
def pillow_files(tmp_path_factory):
    rng = np.random.RandomState(11)
    arrays = {}
    for q in QUALITIES:
        for kind in CONTENTS:
            for w, h in SIZES:
                arrays["rgb420_%s_%dx%d_%d" % (kind, w, h, q)] = content(kind, (h, w, 3), rng)
                arrays["rgb444_%s_%dx%d_%d" % (kind, w, h, q)] = content(kind, (h, w, 3), rng)
                arrays["gray_%s_%dx%d_%d" % (kind, w, h, q)] = content(kind, (h, w), rng)
            for w, h in MCU_SIZES:
                y = content(kind, (h, w), rng)
                c = content(kind, (h // 2, w // 2, 2), rng)
                arrays["ycc_%s_%dx%d_%d" % (kind, w, h, q)] = np.concatenate([y[:, :, None], np.repeat(np.repeat(c, 2, 0), 2, 1)], -1)
    img, w, h = JO.fibonacci_image(17)
    arrays["fib_chain_%dx%d_50" % (w, h)] = img
    return arrays, _run_pillow(arrays, tmp_path_factory.mktemp("pil"))


@pytest.mark.parametrize("mode", ["rgb420", "rgb444", "gray", "ycc"])
def test_transcoder_equals_pillow_optimize(pillow_files, mode):
    arrays, files = pillow_files
    keys = [k for k in arrays if k.startswith(mode + "_")]
    assert len(keys) == len(QUALITIES) * len(CONTENTS) * (len(MCU_SIZES) if mode == "ycc" else len(SIZES))
    smaller = 0
    for k in keys:
        std, opt = files[k + "_std"], files[k + "_opt"]
        assert JO.transcode(std) == opt, k
        assert len(opt) <= len(std), k    # never longer: at most 12 DC and 162 AC symbols
        smaller += len(opt) < len(std)
    assert smaller > len(keys) // 2


def test_flat_image_has_one_symbol_tables(pillow_files):
    _, files = pillow_files
    t = JO.dht_tables(files["rgb420_flat_64x48_85_opt"])
    assert sorted(t) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for key, (bits, vals) in t.items():
        if key != (0, 0):   # (the first DC difference of the luma plane is not zero)
            assert bits == [1] + [0] * 15 and len(vals) == 1, key


def test_length_limited_table_equals_pillow(pillow_files):
    """the chain image: the AC table's optimal code is deeper than 16 bits, and the limited table is Pillow's"""
    arrays, files = pillow_files
    key = [k for k in arrays if k.startswith("fib_")][0]
    std, opt = files[key + "_std"], files[key + "_opt"]
    hist = JO.histograms(std)
    assert sorted(hist) == [(0, 0), (1, 0)]
    ac = hist[(1, 0)]
    counts = JO.fibonacci_counts(17)
    for s, n in zip(JO.fibonacci_symbols(17), counts):
        assert ac[s] == n, hex(s)
    blocks = arrays[key].size // 64   # (the last row of blocks is filled up with flat ones)
    assert ac[0] == blocks and sum(ac) == blocks + sum(counts)   # every block: at most its one coefficient, then EOB
    depth = JO.huffman_depth(ac)
    assert depth > 16, depth
    bits, vals = JO.optimal_table(ac)
    assert bits[15] > 0 and len(vals) == 18
    assert JO.dht_tables(opt)[(1, 0)] == (bits, vals)
    assert JO.transcode(std) == opt


def test_table_rule_on_shapes_no_image_gives():
    # one symbol: code "0" of length 1 (the pseudo-symbol takes "1")
    f = [0] * 256
    f[5] = 9
    assert JO.optimal_table(f) == ([1] + [0] * 15, [5])
    # two symbols
    f[200] = 1
    bits, vals = JO.optimal_table(f)
    assert bits[:2] == [1, 1] and vals == [5, 200]
    # 256 equal counts: a complete 8-bit code but for the pseudo-symbol's place -- 255 codes of 8 bits, two of 9 ... limited to <= 16
    bits, vals = JO.optimal_table([1] * 256)
    assert sum(bits) == 256 and sorted(vals) == list(range(256)) and sum(b / 2.0 ** (l + 1) for l, b in enumerate(bits)) < 1.0
    for depth in (17, 22, 32):
        f = [0] * 256
        for i, n in enumerate(JO.fibonacci_counts(depth)):
            f[i] = n
        assert JO.huffman_depth(f) == depth
        bits, vals = JO.optimal_table(f)
        assert sum(bits) == depth and bits[15] > 0 and sum(b / 2.0 ** (l + 1) for l, b in enumerate(bits)) < 1.0


# ---- argument checks, made before the device is touched ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _one_file(api, w, h, gray):
    """a descriptor with pointers nothing may follow: the calls below refuse the file on its numbers alone"""
    keep = np.zeros(64, np.uint8)
    img = api.Image()
    img.data = keep.ctypes.data
    img.chroma_data = keep.ctypes.data
    img.width, img.height = w, h
    img.pixelFormat = api.PIX_FMT_MONOCHROME if gray else api.PIX_FMT_YUV420
    return img, keep


def test_unknown_flag_bits_are_refused_before_anything_else(api):
    lib = api.load()
    for flags in (2, 3, 4, -1, 1 << 30):
        # (NULL arrays and n < 0 would be BAD_PTR: the flags are looked at first)
        assert lib.uhdr_hip_jpeg_encode_batch_ex(-1, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_FEATURE
        assert lib.uhdr_hip_jpeg_encode_rgb_batch_ex(-1, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_FEATURE
        assert lib.uhdr_hip_jpeg_encode_rgba420_batch_ex(-1, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_FEATURE
        assert lib.uhdr_hip_jpegr_encode_batch_ex(-1, None, None, api.TF_HLG, 90, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_UNSUPPORTED_FEATURE


@pytest.mark.parametrize("flags", [0, 1])
def test_null_arrays_are_bad_ptr(api, flags):
    lib = api.load()
    assert lib.uhdr_hip_jpeg_encode_batch_ex(1, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_encode_batch_ex(-1, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_encode_rgb_batch_ex(1, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_encode_rgba420_batch_ex(1, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpegr_encode_batch_ex(1, None, None, api.TF_HLG, 90, None, None, None, None, None, None, flags, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    # the calls they extend still answer the same
    assert lib.uhdr_hip_jpeg_encode_batch(1, None, None, None, None, None, None, None, None, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpegr_encode_batch(1, None, None, api.TF_HLG, 90, None, None, None, None, None, None, api.MEM_HOST, None) == api.ERROR_BAD_PTR
    # an empty batch is no error, with or without the flag
    assert lib.uhdr_hip_jpeg_encode_batch_ex(0, None, None, None, None, None, None, None, None, flags, api.MEM_HOST, None) == 0


@pytest.mark.parametrize("w,h,gray", [(65500, 65500, False), (65500, 65500, True), (32000, 31752, True), (26032, 26032, False)])
def test_an_image_too_large_for_the_table_search_is_refused(api, w, h, gray):
    """63 * nblk >= 10^9, i.e. nblk above 15 873 015: the largest sizes, and the smallest round ones past the bound -- one plane of
    4000 x 3969 = 15 876 000 blocks, 4:2:0 with 1627 x 1627 MCUs of six = 15 882 774.  (Refused sizes only: an accepted one would be
    compressed from these pointers.)"""
    lib = api.load()
    nblk = ((w + 7) // 8) * ((h + 7) // 8) if gray else ((w + 15) // 16) * ((h + 15) // 16) * 6
    assert nblk * 63 >= 1000000000 and nblk < 15873015 * 7
    img, keep = _one_file(api, w, h, gray)
    q = (C.c_int * 1)(90)
    out, cap, n, st = (C.c_void_p * 1)(keep.ctypes.data), (C.c_size_t * 1)(64), (C.c_size_t * 1)(0), (C.c_int * 1)(12345)
    rc = lib.uhdr_hip_jpeg_encode_batch_ex(1, C.byref(img), q, None, None, out, cap, n, st, api.ENCODE_OPTIMIZE_HUFFMAN, api.MEM_DEVICE, None)
    assert rc == api.ERROR_UNSUPPORTED_FEATURE and st[0] == api.ERROR_UNSUPPORTED_FEATURE and n[0] == 0


def test_optimal_table_refuses_bad_histograms(api):
    lib = api.load()
    f = (C.c_uint32 * 256)()
    bits, vals, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), C.c_int(-7)
    assert lib.uhdr_hip_jpeg_optimal_table(None, bits, vals, C.byref(n), None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_optimal_table(f, None, vals, C.byref(n), None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, None, C.byref(n), None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, vals, None, None) == api.ERROR_BAD_PTR
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, vals, C.byref(n), None) == api.ERROR_BAD_PTR      # no non-zero count
    f[3] = 1000000000
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, vals, C.byref(n), None) == api.ERROR_BAD_PTR      # libjpeg's "no frequency"
    assert n.value == -7
