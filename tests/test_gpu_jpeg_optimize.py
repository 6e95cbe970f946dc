"""-m gpu: UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN -- files with Huffman tables of their own, built on the device -- BYTE FOR BYTE against
tests/jpeg_optimize_oracle.py's transcode() of the default file (the CPU oracle's for the planar call, which tests/test_gpu_jpeg.py
pins to libjpeg; the default call's own for the RGBA forms, which existing tests pin to Pillow).  transcode() itself is pinned to
Pillow's optimize=True by tests/test_jpeg_optimize_cpu.py."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests import jpeg_optimize_oracle as JO
from tests.test_jpeg_codec_batch import EncBatch
from tests.test_jpeg_oracle import _content, _planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = api.ENCODE_OPTIMIZE_HUFFMAN


def _arr(ctype, vals):
    return (ctype * max(len(vals), 1))(*vals)


class OptBatch(EncBatch):
    """one uhdr_hip_jpeg_encode_batch_ex call (tests/test_jpeg_codec_batch.py's arrays)"""

    def run_ex(self, lib, flags):
        from tests.gpu_util import stream_ptr
        return lib.uhdr_hip_jpeg_encode_batch_ex(self.n, self.imgs, self.q, self.icc, self.iccn, self.optr, self.cap, self.size, self.stat, flags,
                                                 self.mem, stream_ptr())

    def untouched_behind(self, i):
        b = self.bufs[i]
        tail = b[self.size[i]:].cpu().numpy() if self.outs_dev else b[self.size[i]:]
        return bool((tail == 0xCD).all())


def item(y, u=None, v=None, q=85, icc=None):
    """planes (2-D arrays; u, v None: one plane) -> an EncBatch item with tight strides"""
    h, w = y.shape
    it = dict(yb=np.ascontiguousarray(y.reshape(-1)), ub=None, w=w, h=h, ls=w, cs=0, q=q)
    if u is not None:
        it["ub"] = np.ascontiguousarray(np.concatenate([u.reshape(-1), v.reshape(-1)]))
        it["cs"] = w // 2
    if icc is not None:
        it["icc"] = icc
    return it


def default_file(orc, it):
    return orc.jpeg_encode("orc", it["yb"], it["ub"], it["w"], it["h"], it["q"], it["ls"], it["cs"], icc=it.get("icc"))


def expected(orc, it):
    return JO.transcode(default_file(orc, it))


def check(hip, orc, items, planes_dev=True, outs_dev=True):
    b = OptBatch(items, planes_dev, outs_dev)
    rc = b.run_ex(hip.load(), OPT)
    assert rc == 0 and list(b.stat) == [0] * b.n, (rc, list(b.stat))
    for i, it in enumerate(items):
        want = expected(orc, it)
        got = b.file(i)
        assert b.size[i] == len(want), (i, it["w"], it["h"], it["q"], b.size[i], len(want))
        assert got == want, (i, it["w"], it["h"], it["q"], next(k for k in range(len(want)) if got[k] != want[k]))
        assert b.untouched_behind(i), i
    return b


def noise(rng, h, w):
    return rng.randint(0, 256, (h, w)).astype(np.uint8)


def yuv_noise(rng, w, h, q=85, icc=None):
    return item(noise(rng, h, w), noise(rng, h // 2, w // 2), noise(rng, h // 2, w // 2), q, icc)


def flat420(w, h, q=85):
    return item(np.full((h, w), 90, np.uint8), np.full((h // 2, w // 2), 120, np.uint8), np.full((h // 2, w // 2), 140, np.uint8), q)


def checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


# ---- one block, workgroup tails, hot bins, symbol range ---------------------------------------------------------------------------
@pytest.mark.parametrize("outs_dev", [True, False], ids=["device", "host"])
def test_one_block_and_workgroup_tails(hip, orc, outs_dev):
    rng = np.random.RandomState(5)
    items = [item(noise(rng, 1, 1)), item(noise(rng, 8, 8)),                       # one plane: one block
             yuv_noise(rng, 2, 2), yuv_noise(rng, 16, 16),                         # 4:2:0: one MCU (2x2: three dummy blocks)
             yuv_noise(rng, 18, 10),                                               # dummies on both edges
             flat420(18, 10),                                                      # ... and DC tables of one or two symbols
             yuv_noise(rng, 96, 80, 50),                                           # 180 blocks: two workgroups, a tail of 52
             item(noise(rng, 64, 128), q=75),                                      # exactly 128 blocks
             item(noise(rng, 64, 136), q=75)]                                      # 136
    check(hip, orc, items, True, outs_dev)
    check(hip, orc, items[:5], False, outs_dev)                                    # planes staged from host memory


def test_flat_image_every_lane_on_the_same_counters(hip, orc):
    flat = flat420(256, 256)
    t = JO.dht_tables(expected(orc, flat))
    for key in ((1, 0), (1, 1)):
        assert t[key] == ([1] + [0] * 15, [0])                                     # EOB alone: code "0" of length 1
    assert sum(t[(0, 0)][0]) == 2 and sum(t[(0, 1)][0]) <= 3                       # a plane's first difference, then category 0
    rng = np.random.RandomState(6)
    one_noisy = flat420(256, 256)
    one_noisy["yb"] = one_noisy["yb"].copy()
    one_noisy["yb"].reshape(256, 256)[120:128, 40:48] = noise(rng, 8, 8)
    check(hip, orc, [flat, one_noisy, item(np.full((256, 256), 33, np.uint8))])


def test_symbol_range_zrl_and_stuffing(hip, orc):
    rng = np.random.RandomState(7)
    bw = item(checker(48, 64), checker(24, 32), 255 - checker(24, 32), q=100)
    bw_gray = item(checker(40, 40), q=100)
    blocks = item(np.kron(checker(6, 8), np.ones((8, 8), np.uint8)), np.kron(checker(3, 4), np.ones((8, 8), np.uint8)),
                  np.kron(255 - checker(3, 4), np.ones((8, 8), np.uint8)), q=100)      # 0 / 255 from block to block
    assert any(JO.histograms(default_file(orc, bw))[(1, 0)][(r << 4) | 10] for r in range(16))       # AC size 10
    hb = JO.histograms(default_file(orc, blocks))
    assert hb[(0, 0)][11] > 0 and hb[(0, 1)][11] > 0                                                 # DC category 11, both tables
    # runs >= 16: every block is 128 plus the highest basis function alone (zigzag position 63, three ZRL in front of it)
    x = np.arange(8)
    tile = np.clip(np.rint(128 + 0.25 * 297 * np.outer(np.cos((2 * x + 1) * 7 * math.pi / 16), np.cos((2 * x + 1) * 7 * math.pi / 16))), 0, 255)
    zrl = item(np.tile(tile.astype(np.uint8), (5, 9)), q=50)
    hz = JO.histograms(default_file(orc, zrl))[(1, 0)]
    assert hz[0xF0] == 3 * 45 and hz[0] == 0
    stuffed = yuv_noise(rng, 64, 48, 100)
    body = expected(orc, stuffed)
    assert b"\xff\x00" in body[JO.first_segment(body, 0xDA):]                       # stuffing under non-default codes
    check(hip, orc, [bw, bw_gray, blocks, zrl, stuffed, yuv_noise(rng, 40, 24, 1)])


# ---- the length limit -------------------------------------------------------------------------------------------------------------
def test_length_limit_through_the_encoder(hip, orc):
    img, w, h = JO.fibonacci_image(17)
    it = item(img, q=50)
    ac = JO.histograms(default_file(orc, it))[(1, 0)]
    assert JO.huffman_depth(ac) > 16
    b = check(hip, orc, [it])
    assert JO.dht_tables(b.file(0))[(1, 0)][0][15] > 0                               # a 16-bit code


def _fib(depth):
    f = [0] * 256
    for i, n in enumerate(JO.fibonacci_counts(depth)):
        f[(i * 37) % 256] = n
    return f


TABLE_CASES = {
    "fib17": _fib(17), "fib22": _fib(22), "fib32": _fib(32),
    "256_ones": [1] * 256,
    "two": [0] * 7 + [5] + [0] * 200 + [3] + [0] * 47,
    "one": [0] * 255 + [9],
    "ties": [1000] * 162 + [0] * 94,
    "big": [999999999] + [0] * 255,
    "big_and_small": [999999999, 1, 1] + [0] * 253,
}


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_table_kernel_equals_the_rule(hip, name):
    lib = hip.load()
    freq = TABLE_CASES[name]
    assert len(freq) == 256
    if name.startswith("fib"):
        assert JO.huffman_depth(freq) == int(name[3:])
    f = (C.c_uint32 * 256)(*freq)
    bits, vals, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(*([0xEE] * 256)), C.c_int(-7)
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, vals, C.byref(n), None) == 0
    wb, wv = JO.optimal_table(freq)
    assert list(bits) == wb and n.value == len(wv) and list(vals)[:n.value] == wv, (list(bits), wb)
    assert list(vals)[n.value:] == [0xEE] * (256 - n.value)


def test_table_kernel_refuses_a_code_longer_than_32_bits(hip):
    """where libjpeg gives up (JERR_HUFF_CLEN_OVERFLOW): counts 1, 2, 3, 5, ... over 40 symbols (their sum is below 10^9)"""
    lib = hip.load()
    freq = _fib(40)
    assert max(freq) < 1000000000 and sum(freq) < 1000000000 and JO.huffman_depth(freq) > 32
    f = (C.c_uint32 * 256)(*freq)
    bits, vals, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), C.c_int(-7)
    assert lib.uhdr_hip_jpeg_optimal_table(f, bits, vals, C.byref(n), None) == api.ERROR_UNSUPPORTED_FEATURE and n.value == -7


# ---- per-file header length, batches, capacities ----------------------------------------------------------------------------------
@pytest.mark.parametrize("outs_dev", [True, False], ids=["device", "host"])
def test_stream_starts_at_every_byte_alignment(hip, orc, outs_dev):
    rng = np.random.RandomState(8)
    colour, gray = yuv_noise(rng, 48, 16, 50), item(noise(rng, 16, 24), q=100)   # tables of different sizes
    items = []
    for k in range(4):   # ICC payloads of 0 .. 3 bytes mod 4: each image's stream starts at every alignment once
        icc = bytes((3 * j + k) % 256 for j in range(40 + k))
        items += [dict(colour, icc=icc), dict(gray, icc=icc)]
    for base in (0, 1):
        starts = {(JO.first_segment(expected(orc, it), 0xDA) + (14 if base == 0 else 10)) % 4 for it in items[base::2]}
        assert starts == {0, 1, 2, 3}
    check(hip, orc, items, True, outs_dev)


@pytest.mark.parametrize("planes_dev,outs_dev", [(True, True), (False, False), (True, False)])
def test_mixed_batch_with_a_failing_file(hip, orc, planes_dev, outs_dev):
    lib = hip.load()
    rng = np.random.RandomState(9)
    items = []
    for k, (w, h) in enumerate(((64, 48), (130, 66), (16, 16), (48, 32), (256, 144), (34, 18))):
        y, u, v = _content(("smooth", "noise", "extreme", "flat")[k % 4], w, h, rng)
        yb, ub = _planes(y, u, v, w + 2 * (k % 2), w // 2 + (k % 2), rng)
        gray = k % 3 == 2
        items.append(dict(yb=yb, ub=None if gray else ub, w=w, h=h, ls=w + 2 * (k % 2), cs=0 if gray else w // 2 + (k % 2), q=(1, 50, 85, 100, 90, 20)[k]))
    bad = dict(items[1])
    bad["null_data"] = True
    odd = dict(items[0], w=63)
    items[2:2] = [bad, odd]
    b, d = OptBatch(items, planes_dev, outs_dev), OptBatch(items, planes_dev, outs_dev)
    rc, rc_default = b.run_ex(lib, OPT), d.run_ex(lib, 0)
    assert rc == rc_default == api.ERROR_BAD_PTR and list(b.stat) == list(d.stat)
    assert [b.stat[2], b.stat[3]] == [api.ERROR_BAD_PTR, api.ERROR_RESOLUTION_MISMATCH]
    for i, it in enumerate(items):
        if i in (2, 3):
            continue
        assert b.stat[i] == 0 and d.file(i) == default_file(orc, it) and b.file(i) == JO.transcode(d.file(i)), i
        assert b.size[i] < d.size[i]


def test_more_files_than_one_round(hip, orc):
    rng = np.random.RandomState(10)
    items = [item(noise(rng, 8, 8), q=10 + (k % 90)) if k % 3 else yuv_noise(rng, 8, 8, 10 + (k % 90)) for k in range(130)]
    check(hip, orc, items)


def test_device_capacities_and_the_size_probe(hip, orc):
    """below the header, below the total, exactly the total, and out == NULL with capacity 0: the sizes are exact, the statuses the
    existing convention's, and a file that does not fit leaves at most its own capacity written"""
    lib = hip.load()
    rng = np.random.RandomState(12)
    it = yuv_noise(rng, 64, 48, 90, icc=bytes(range(50)))
    want = expected(orc, it)
    header = JO.first_segment(want, 0xDA) + 14
    caps = [16, header - 1, header, header + 5, len(want) - 1, len(want), None]
    for outs_dev in (True, False):
        b = OptBatch([it] * len(caps), True, outs_dev, caps=caps)
        d = OptBatch([it] * len(caps), True, outs_dev, caps=[c if c is None else c + len(default_file(orc, it)) - len(want) for c in caps])
        rc, rc_default = b.run_ex(lib, OPT), d.run_ex(lib, 0)
        assert rc == rc_default == api.ERROR_INSUFFICIENT_RESOURCE
        assert list(b.stat) == list(d.stat) == [api.ERROR_INSUFFICIENT_RESOURCE] * 5 + [0, api.ERROR_INSUFFICIENT_RESOURCE]
        assert list(b.size) == [len(want)] * len(caps)
        assert b.file(5) == want
        for i, c in enumerate(caps[:5]):
            buf = b.bufs[i].cpu().numpy() if outs_dev else b.bufs[i]
            assert (buf[c:] == 0xCD).all(), (outs_dev, i)                           # nothing behind the capacity
            if outs_dev and c < header:
                assert (buf == 0xCD).all(), (i, c)                                  # a header that does not fit: nothing is written


def test_flags_zero_is_the_existing_call(hip, orc):
    lib = hip.load()
    rng = np.random.RandomState(13)
    items = [yuv_noise(rng, 96, 80, 50), flat420(256, 256), item(noise(rng, 64, 136), q=75, icc=bytes(range(41)))]
    for planes_dev, outs_dev in ((True, True), (False, False)):
        a, b = OptBatch(items, planes_dev, outs_dev), OptBatch(items, planes_dev, outs_dev)
        assert a.run(lib) == 0 and b.run_ex(lib, 0) == 0
        for i, it in enumerate(items):
            assert a.file(i) == b.file(i) == default_file(orc, it), i


# ---- RGBA8888 as 4:4:4 and as 4:2:0 -----------------------------------------------------------------------------------------------
def _encode_rgba(hip, form, images, qualities, flags, device):
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    n = len(images)
    keep, descs = [], []
    for im in images:
        h, w = im.shape[:2]
        t = to_dev(im) if device else np.ascontiguousarray(im)
        keep.append(t)
        descs.append(hip.rgba8888_image(t.data_ptr() if device else t.ctypes.data, w, h, hip.CG_BT709, w))
    caps = [im.shape[0] * im.shape[1] * 4 + 4096 for im in images]
    outs = [dev_empty(c, 0xCD) if device else np.full(c, 0xCD, np.uint8) for c in caps]
    optr = _arr(C.c_void_p, [o.data_ptr() if device else o.ctypes.data for o in outs])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    mem = hip.MEM_DEVICE if device else hip.MEM_HOST
    if form == "rgb":
        rc = lib.uhdr_hip_jpeg_encode_rgb_batch_ex(n, hip.image_array(descs), _arr(C.c_int, qualities), optr, _arr(C.c_size_t, caps), sizes, stat, flags, mem,
                                                   stream_ptr())
    else:
        rc = lib.uhdr_hip_jpeg_encode_rgba420_batch_ex(n, hip.image_array(descs), _arr(C.c_int, qualities), None, None, optr, _arr(C.c_size_t, caps), sizes,
                                                       stat, flags, mem, stream_ptr())
    assert rc == 0 and list(stat) == [0] * n, (rc, list(stat))
    return [(to_host(o).copy() if device else o)[:sizes[k]].tobytes() for k, o in enumerate(outs)]


@pytest.fixture(scope="module")
def rgba_images():
    rng = np.random.RandomState(14)
    sizes = ((1, 1), (7, 5), (33, 17), (17, 9))   # odd sizes; 17 x 9 as 4:2:0: dummy blocks on both edges
    imgs = [rng.randint(0, 256, (h, w, 4)).astype(np.uint8) for w, h in sizes]
    yy, xx = np.mgrid[0:17, 0:33]
    ramp = np.stack([(xx * 7) % 256, (yy * 13) % 256, (xx + yy) % 256, xx * 0 + 255], -1).astype(np.uint8)
    return imgs + [ramp, np.full((5, 7, 4), 200, np.uint8)], [85, 50, 100, 90, 75, 85]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("form", ["rgb", "rgba420"])
def test_rgba_forms_equal_the_transcode_of_the_default_call(hip, rgba_images, form, device):
    imgs, quals = rgba_images
    std = _encode_rgba(hip, form, imgs, quals, 0, device)
    opt = _encode_rgba(hip, form, imgs, quals, OPT, device)
    for k, (a, b) in enumerate(zip(std, opt)):
        assert b == JO.transcode(a), (form, k)
        assert len(b) < len(a)


@pytest.mark.parametrize("form", ["rgb", "rgba420"])
def test_rgba_forms_equal_pillow_optimize(hip, rgba_images, form, tmp_path):
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("Pillow not installed")
    from tests.test_jpeg_optimize_cpu import _PIL_SCRIPT
    imgs, quals = rgba_images
    mode = "rgb444" if form == "rgb" else "rgb420"
    keys = ["%s_img%d_%dx%d_%d" % (mode, k, im.shape[1], im.shape[0], q) for k, (im, q) in enumerate(zip(imgs, quals))]
    np.savez(tmp_path / "in.npz", **{key: np.ascontiguousarray(im[:, :, :3]) for key, im in zip(keys, imgs)})
    subprocess.check_call([sys.executable, "-c", _PIL_SCRIPT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")])
    res = np.load(tmp_path / "out.npz")
    opt = _encode_rgba(hip, form, imgs, quals, OPT, True)
    for key, got in zip(keys, opt):
        assert got == res[key + "_opt"].tobytes(), key


# ---- JPEG/R -----------------------------------------------------------------------------------------------------------------------
def mpf_images(f):
    """[(offset, size)] of a JPEG/R file's images, read from the primary image's MPF segment"""
    pos = 2
    while f[pos] == 0xFF and f[pos + 1] not in (0xDA, 0xD9):
        ln = (f[pos + 2] << 8) | f[pos + 3]
        if f[pos + 1] == 0xE2 and f[pos + 4:pos + 8] == b"MPF\0":
            base = pos + 8                                    # the TIFF header: the entries' offsets count from here
            t = f[base:pos + 2 + ln]
            e = ">" if t[:2] == b"MM" else "<"
            ifd = struct.unpack(e + "I", t[4:8])[0]
            for k in range(struct.unpack(e + "H", t[ifd:ifd + 2])[0]):
                tag, _, cnt, val = struct.unpack(e + "HHII", t[ifd + 2 + 12 * k:ifd + 14 + 12 * k])
                if tag == 0xB002:
                    out = []
                    for i in range(cnt // 16):
                        _, size, off, _, _ = struct.unpack(e + "IIIHH", t[val + 16 * i:val + 16 * i + 16])
                        out.append((0 if i == 0 else base + off, size))
                    return out
        pos += 2 + ln
    raise AssertionError("no MPF segment")


def _jpegr(lib, pairs, api0, flags, mem, exifs):
    import torch
    n = len(pairs)
    P = api.image_array([p for p, _ in pairs])
    Y = None if api0 else api.image_array([y for _, y in pairs])
    caps = [1 << 20] * n
    outs = [np.zeros(c, np.uint8) for c in caps]
    ex = [np.frombuffer(e, np.uint8) if e else None for e in exifs]
    exp = _arr(C.c_void_p, [e.ctypes.data if e is not None else None for e in ex])
    exn = _arr(C.c_size_t, [len(e) if e else 0 for e in exifs])
    size, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpegr_encode_batch_ex(n, P, Y, api.TF_HLG, 90, exp, exn, _arr(C.c_void_p, [o.ctypes.data for o in outs]), _arr(C.c_size_t, caps), size,
                                            stat, flags, mem, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and list(stat) == [0] * n, (rc, list(stat))
    return [o[:size[k]].tobytes() for k, o in enumerate(outs)]


def _info(lib, blob):
    b = np.frombuffer(blob, np.uint8)
    a, g = api.JpegInfo(), api.JpegInfo()
    assert lib.uhdr_hip_jpegr_info(C.c_void_p(b.ctypes.data), b.size, C.byref(a), C.byref(g)) == 0
    return a, g


@pytest.mark.parametrize("mem", [api.MEM_DEVICE, api.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("api0", [False, True], ids=["api1", "api0"])
def test_jpegr_both_images_are_the_transcodes_of_the_default_files(hip, orc, api0, mem):
    import torch
    lib = hip.load()
    keep, pairs = [], []
    for k, (w, h) in enumerate(((64, 48), (70, 50))):
        p010, yuv = orc.lcg_frame(w, h, 300 + k)
        if mem == api.MEM_DEVICE:
            dp, dy = torch.from_numpy(p010.view(np.uint8).copy()).cuda(), torch.from_numpy(yuv.copy()).cuda()
            keep += [dp, dy]
            pp, yp = dp.data_ptr(), dy.data_ptr()
        else:
            keep += [p010, yuv]
            pp, yp = p010.ctypes.data, yuv.ctypes.data
        pairs.append((api.p010_image(pp, w, h, api.CG_BT2100), api.yuv420_image(yp, w, h, api.CG_BT709)))
    exifs = [None, b"Exif\0\0optimised"]
    torch.cuda.synchronize()
    std = _jpegr(lib, pairs, api0, 0, mem, exifs)
    opt = _jpegr(lib, pairs, api0, OPT, mem, exifs)
    same = _jpegr(lib, pairs, api0, 0, mem, exifs)
    assert same == std                                        # (the optimised call in between left nothing behind)
    for k, (a, b) in enumerate(zip(std, opt)):
        ia, ib = mpf_images(a), mpf_images(b)
        assert len(ia) == len(ib) == 2 and ib[1][0] + ib[1][1] == len(b) and ib[0][1] == ib[1][0]
        for (oa, na), (ob, nb) in zip(ia, ib):
            # the primary image carries the container's segments in front of its DQT: transcode() leaves them as they are, but the
            # XMP and MPF payloads name the (smaller) sizes, so they are compared from the first DQT on
            ja, jb = a[oa:oa + na], b[ob:ob + nb]
            assert jb[:2] == b"\xff\xd8" and jb[-2:] == b"\xff\xd9"
            ta = JO.transcode(ja)
            assert jb[JO.first_segment(jb, 0xDB):] == ta[JO.first_segment(ta, 0xDB):], (k, oa)
            assert [m for m, _, _ in JO.segments(jb)] == [m for m, _, _ in JO.segments(ta)]
            assert nb < na
        # the container around them: the same segments, of the same lengths, in the same order
        pa, ga = _info(lib, a)
        pb, gb = _info(lib, b)
        assert (pb.offset, pb.size, gb.offset, gb.size) == (ib[0][0], ib[0][1], ib[1][0], ib[1][1])
        for x, y in ((pa, pb), (ga, gb)):
            assert (x.width, x.height, x.icc_size, x.exif_size) == (y.width, y.height, y.icc_size, y.exif_size)
        ma, mb = api.Metadata(), api.Metadata()
        na_, nb_ = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
        assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(na_.ctypes.data), na_.size, C.byref(ma)) == 0
        assert lib.uhdr_hip_jpegr_metadata(C.c_void_p(nb_.ctypes.data), nb_.size, C.byref(mb)) == 0
        assert bytes(ma) == bytes(mb)
        w, h = pa.width, pa.height
        ra, rb = np.zeros(w * h * 4, np.uint8), np.full(w * h * 4, 1, np.uint8)
        rcs = []
        for blob, out in ((na_, ra), (nb_, rb)):
            d, m = api.Image(), api.Metadata()
            rcs.append(lib.uhdr_hip_jpegr_decode(C.c_void_p(blob.ctypes.data), blob.size, api.OUTPUT_HDR_HLG, api.FLT_MAX, C.c_void_p(out.ctypes.data),
                                                 out.size, C.byref(d), C.byref(m), api.APPLY_EXACT, api.MEM_HOST, None))
        # (70 x 50: the map is 17 x 12, which no decoder here takes -- of either file)
        assert rcs == ([0, 0] if (w, h) == (64, 48) else [api.ERROR_UNSUPPORTED_MAP_SCALE_FACTOR] * 2), rcs
        if rcs[0] == 0:
            assert np.array_equal(ra, rb)


def test_the_shims_setter(hip, orc, tmp_path):
    """ultrahdr::JpegRHip::setOptimizeHuffman(true): encodeJPEGR API-1 and API-0 write uhdr_hip_jpegr_encode_batch_ex's bytes"""
    lib = hip.load()
    exe = str(tmp_path / "shim_optimize_test")
    pkg = os.path.join(ROOT, "libultrahdr_dev_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_optimize_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    w, h = 72, 40
    p010, yuv = orc.lcg_frame(w, h, 77)
    p010.tofile(str(tmp_path / "in.p010"))
    yuv.tofile(str(tmp_path / "in.yuv"))
    r = subprocess.run([exe, str(tmp_path / "in.p010"), str(tmp_path / "in.yuv"), str(w), str(h), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n: open(tmp_path / n, "rb").read()   # noqa: E731
    pair = [(api.p010_image(p010.ctypes.data, w, h, api.CG_BT2100), api.yuv420_image(yuv.ctypes.data, w, h, api.CG_BT709))]
    for api0, tag in ((False, "1"), (True, "0")):
        assert _jpegr(lib, pair, api0, 0, api.MEM_HOST, [None]) == [rd("std%s.jpgr" % tag)]
        assert _jpegr(lib, pair, api0, OPT, api.MEM_HOST, [None]) == [rd("opt%s.jpgr" % tag)]
