"""-m gpu: progressive files written on the device -- the _scans calls with UHDR_HIP_SCANS_PROGRESSIVE BYTE FOR BYTE against
tests/jpeg_progressive_encode_oracle.py's transcode_progressive() of the file the existing _opts call writes for the same input
(tests/test_jpeg_progressive_encode_cpu.py pins that oracle to Pillow's libjpeg-turbo), the RGBA call against Pillow's own progressive
files, and the JPEG/R call against its parts."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests import jpeg_optimize_oracle as JO
from tests import jpeg_progressive_encode_cases as PC
from tests import jpeg_restart_cases as RC
from tests import jpeg_sampling_encode_cases as EC
from tests.jpeg_progressive_encode_oracle import transcode_progressive
from tests.test_gpu_jpeg_optimize import _arr, _info, mpf_images
from tests.test_gpu_jpeg_sampling_encode import PlanesBatch, _first_diff

pytestmark = pytest.mark.gpu
PROG, BASE = api.SCANS_PROGRESSIVE, api.SCANS_BASELINE


class ScansBatch(PlanesBatch):
    """one uhdr_hip_jpeg_encode_planes_batch_scans call (PlanesBatch's arguments)"""

    def run_scans(self, lib, opts, mode):
        from tests.gpu_util import stream_ptr
        return lib.uhdr_hip_jpeg_encode_planes_batch_scans(self.n, self.imgs, self.q, self.icc, self.iccn, self.optr, self.cap, self.size, self.stat,
                                                           None if opts is None else C.byref(opts), mode, self.mem, stream_ptr())


def base_files(hip, items, planes_dev=True):
    b = PlanesBatch(items, planes_dev, True)
    assert b.run(hip.load(), None) == 0 and list(b.stat) == [0] * b.n
    return [b.file(i) for i in range(b.n)]


def check(hip, items, want, planes_dev=True, outs_dev=True, opts=None):
    b = ScansBatch(items, planes_dev, outs_dev)
    rc = b.run_scans(hip.load(), opts, PROG)
    assert rc == 0 and list(b.stat) == [0] * b.n, (rc, list(b.stat))
    for i, it in enumerate(items):
        got = b.file(i)
        tag = (i, it["w"], it["h"], it["q"], it.get("hs"), it.get("vs"))
        assert b.size[i] == len(want[i]), tag + (b.size[i], len(want[i]))
        assert got == want[i], tag + (_first_diff(got, want[i]),)
        assert b.untouched_behind(i), tag
    return b


def _gray(img, q):
    return RC.plane_item(np.ascontiguousarray(img), q)


def _yuv420(w, h, kind, q, seed):
    return RC.yuv_item(PC.content(kind, (h, w), seed), PC.content(kind, (h // 2, w // 2), seed + 1), PC.content(kind, (h // 2, w // 2), seed + 2), q)


def _sampled(w, h, hs, vs, kind, q, seed):
    cw, ch = (w + hs - 1) // hs, (h + vs - 1) // vs
    return EC.item(PC.content(kind, (h, w), seed), PC.content(kind, (ch, cw), seed + 1), PC.content(kind, (ch, cw), seed + 2), hs, vs, q)


# ---- 1. the matrix: one plane, 4:2:0, 4:4:4, 4:2:2 and 4:4:0 in one call --------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix(hip):
    """(items, the transcoded forms of the _opts call's files); one plane and 4:2:0 with every (content, quality), the other samplings with
    four pairings each; 4:2:0 at the even sizes (the call takes no other)"""
    items, seed = [], 100
    for (w, h) in PC.SIZES:
        for kind, q in PC.combos((w, h)):
            seed += 3
            items.append(_gray(PC.content(kind, (h, w), seed), q))
            if w % 2 == 0 and h % 2 == 0:
                items.append(_yuv420(w, h, kind, q, seed))
        for k, (hs, vs) in enumerate(EC.SAMPLINGS):
            for kind, q in PC.rotated(k + w):
                seed += 3
                items.append(_sampled(w, h, hs, vs, kind, q, seed))
    return items, [transcode_progressive(f)[0] for f in base_files(hip, items)]


@pytest.mark.parametrize("outs_dev", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("planes_dev", [True, False], ids=["from_device", "from_host"])
def test_matrix_mixed_batch(hip, matrix, planes_dev, outs_dev):
    items, want = matrix
    check(hip, items, want, planes_dev, outs_dev)


def test_single_files_and_the_optimize_flag(hip, matrix):
    """a file on its own is the batch's file; UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN changes nothing"""
    items, want = matrix
    for i in range(0, len(items), 37):
        check(hip, [items[i]], [want[i]])
        check(hip, [items[i]], [want[i]], opts=api.encode_opts(api.ENCODE_OPTIMIZE_HUFFMAN))


def test_baseline_mode_is_the_opts_call(hip, matrix):
    items = matrix[0][::11]
    for opts in (None, api.encode_opts(api.ENCODE_OPTIMIZE_HUFFMAN), api.encode_opts(0, 2, 0)):
        a, b = PlanesBatch(items, True, True), ScansBatch(items, True, True)
        assert a.run(hip.load(), opts) == 0 and b.run_scans(hip.load(), opts, BASE) == 0
        assert list(a.stat) == list(b.stat) == [0] * a.n
        assert [a.file(i) for i in range(a.n)] == [b.file(i) for i in range(b.n)]


# ---- 2. the constructed planes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.constructed()))
def test_constructed(hip, name):
    img, q, _ = PC.constructed()[name]
    items = [_gray(img, q)]
    want, counters = transcode_progressive(base_files(hip, items)[0])
    check(hip, items, [want])


def test_long_run_in_three_components(hip):
    """4:2:0, flat: the luma AC scans are runs of 33 024 blocks, the chroma scans of 8 256"""
    y = PC.long_run()
    items = [RC.yuv_item(y, np.full((PC.LONG_H // 2, PC.LONG_W // 2), 90, np.uint8), np.full((PC.LONG_H // 2, PC.LONG_W // 2), 200, np.uint8), 50)]
    want, counters = transcode_progressive(base_files(hip, items)[0])
    assert counters["eob_7fff"] > 0
    check(hip, items, [want])


# ---- 3. capacities ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outs_dev", [True, False], ids=["device", "host"])
def test_size_probe_and_a_capacity_one_byte_short(hip, matrix, outs_dev):
    items, want = matrix[0][::23][:6], matrix[1][::23][:6]
    caps = [len(w) + 64 for w in want]
    caps[1], caps[2], caps[4] = None, len(want[2]) - 1, len(want[4])   # the probe, one byte short, the exact size
    b = ScansBatch(items, True, outs_dev, caps=caps)
    rc = b.run_scans(hip.load(), None, PROG)
    ir = api.ERROR_INSUFFICIENT_RESOURCE
    assert rc == ir and list(b.stat) == [0, ir, ir, 0, 0, 0], (rc, list(b.stat))
    assert [b.size[k] for k in range(6)] == [len(w) for w in want]
    for k in (0, 3, 4, 5):
        assert b.file(k) == want[k] and b.untouched_behind(k), k
    assert b.untouched_behind(2, caps[2])


# ---- 4. the decoder reads the files -------------------------------------------------------------------------------------------------------------
def test_files_decode_to_the_planes_of_the_baseline_files(hip, matrix):
    from tests.test_gpu_jpeg_sampling import _decode_batch
    items, want = matrix[0][::5], matrix[1][::5]
    base = base_files(hip, items)
    rc, stat, planes, _ = _decode_batch(hip, want, hip.DECODE_TO_YCBCR, True)
    rc2, stat2, planes2, _ = _decode_batch(hip, base, hip.DECODE_TO_YCBCR, True)
    assert rc == rc2 == 0 and stat == stat2 == [0] * len(items)
    for k in range(len(items)):
        assert np.array_equal(planes[k], planes2[k]), k


# ---- 5. RGBA against Pillow ------------------------------------------------------------------------------------------------------------------------
_PIL_SCRIPT = r"""
import io, sys, numpy as np
from PIL import Image, ImageFile
ImageFile.MAXBLOCK = 1 << 22
d = np.load(sys.argv[1]); out = {}
for key in d.files:
    q = int(key.split("_")[-1])
    for sub in (0, 1, 2):
        b = io.BytesIO()
        Image.fromarray(d[key], "RGB").save(b, "JPEG", quality=q, subsampling=sub, progressive=True)
        out["%s_%d" % (key, sub)] = np.frombuffer(b.getvalue(), np.uint8)
np.savez(sys.argv[2], **out)
"""


def _encode_rgba_scans(hip, sampling, images, qualities, mode, device, caps=None):
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    lib = hip.load()
    n = len(images)
    keep = [to_dev(im) if device else np.ascontiguousarray(im) for im in images]
    descs = [hip.rgba8888_image(t.data_ptr() if device else t.ctypes.data, im.shape[1], im.shape[0], hip.CG_BT709, im.shape[1]) for t, im in zip(keep, images)]
    caps = caps or [im.shape[0] * im.shape[1] * 8 + 4096 for im in images]
    outs = [dev_empty(c + 64, 0xCD) if device else np.full(c + 64, 0xCD, np.uint8) for c in caps]
    optr = _arr(C.c_void_p, [(o.data_ptr() if device else o.ctypes.data) if c else None for o, c in zip(outs, caps)])
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpeg_encode_rgba_batch_scans(n, hip.image_array(descs), _arr(C.c_int, qualities), None, None, optr, _arr(C.c_size_t, caps), sizes, stat,
                                                   sampling, None, mode, hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr())
    files = []
    for k in range(n):
        full = to_host(outs[k]).copy() if device else outs[k]
        if stat[k] == 0:
            assert (full[sizes[k]:] == 0xCD).all(), k
        files.append(full[:sizes[k]].tobytes() if stat[k] == 0 else None)
    return rc, list(stat), list(sizes), files


@pytest.fixture(scope="module")
def rgba_case(tmp_path_factory):
    pytest.importorskip("PIL")
    imgs, quals = [], []
    for k, (w, h) in enumerate(((17, 9), (1, 1), (40, 24), (136, 136))):
        for kind, q in PC.rotated(k):
            imgs.append(PC.content(kind, (h, w, 4), 900 + len(imgs)))
            quals.append(q)
    tmp = tmp_path_factory.mktemp("pil")
    np.savez(tmp / "in.npz", **{"%d_%d" % (k, q): np.ascontiguousarray(im[:, :, :3]) for k, (im, q) in enumerate(zip(imgs, quals))})
    subprocess.check_call([sys.executable, "-c", _PIL_SCRIPT, str(tmp / "in.npz"), str(tmp / "out.npz")])
    res = np.load(tmp / "out.npz")
    return imgs, quals, {k: res[k].tobytes() for k in res.files}


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("sub", [0, 1, 2], ids=["444", "422", "420"])
def test_rgba_equals_pillow_progressive(hip, rgba_case, sub, device):
    imgs, quals, files = rgba_case
    sampling = (hip.PIX_FMT_YUV444, hip.PIX_FMT_YUV422, hip.PIX_FMT_YUV420)[sub]
    rc, stat, sizes, got = _encode_rgba_scans(hip, sampling, imgs, quals, PROG, device)
    assert rc == 0 and stat == [0] * len(imgs), (rc, stat)
    for k, g in enumerate(got):
        want = files["%d_%d_%d" % (k, quals[k], sub)]
        assert g == want, (sub, k, len(g), len(want), _first_diff(g, want))
    if device and sub == 1:   # the probe: the exact sizes; and mode 0: the _opts call
        rc, stat, sizes2, _ = _encode_rgba_scans(hip, sampling, imgs, quals, PROG, True, caps=[0] * len(imgs))
        assert rc == api.ERROR_INSUFFICIENT_RESOURCE and sizes2 == sizes
        from tests.test_gpu_jpeg_sampling_encode import _encode_rgba
        assert _encode_rgba_scans(hip, sampling, imgs, quals, BASE, True)[3] == _encode_rgba(hip, sampling, imgs, quals, None, True)[3]


# ---- 6. JPEG/R ------------------------------------------------------------------------------------------------------------------------------------
def _jpegr_scans(lib, pairs, api0, mode, mem):
    import torch
    n = len(pairs)
    P = api.image_array([p for p, _ in pairs])
    Y = None if api0 else api.image_array([y for _, y in pairs])
    caps = [1 << 20] * n
    outs = [np.zeros(c, np.uint8) for c in caps]
    size, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [7] * n)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.uhdr_hip_jpegr_encode_batch_scans(n, P, Y, api.TF_HLG, 90, None, None, _arr(C.c_void_p, [o.ctypes.data for o in outs]), _arr(C.c_size_t, caps),
                                               size, stat, None, mode, mem, s)
    assert rc == 0 and list(stat) == [0] * n, (rc, list(stat))
    return [o[:size[k]].tobytes() for k, o in enumerate(outs)]


@pytest.mark.parametrize("mem", [api.MEM_DEVICE, api.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("api0", [False, True], ids=["api1", "api0"])
def test_jpegr_both_images_are_the_transcoded_forms(hip, orc, api0, mem):
    from tests.test_gpu_jpeg_restart import _hdr, _jpegr, _pair
    lib = hip.load()
    keep = []
    pairs = [_pair(orc, 64, 48, 300, mem, keep), _pair(orc, 136, 72, 301, mem, keep)]
    std = _jpegr(lib, pairs, api0, None, mem)
    got = _jpegr_scans(lib, pairs, api0, PROG, mem)
    assert _jpegr_scans(lib, pairs, api0, BASE, mem) == std
    for k, (w, h) in enumerate(((64, 48), (136, 72))):
        ia, ib = mpf_images(std[k]), mpf_images(got[k])
        assert len(ia) == len(ib) == 2 and ib[1][0] + ib[1][1] == len(got[k]) and ib[0][1] == ib[1][0]
        for which, ((oa, na), (ob, nb)) in enumerate(zip(ia, ib)):
            ja, jb = std[k][oa:oa + na], got[k][ob:ob + nb]
            ta = transcode_progressive(ja)[0]
            # (the primary image's XMP and MPF payloads name the new sizes: compared from the first DQT on)
            assert jb[JO.first_segment(jb, 0xDB):] == ta[JO.first_segment(ta, 0xDB):], (k, which)
        pb, gb = _info(lib, got[k])
        assert (pb.offset, pb.size, gb.offset, gb.size) == (ib[0][0], ib[0][1], ib[1][0], ib[1][1])
        assert np.array_equal(_hdr(lib, got[k], w, h), _hdr(lib, std[k], w, h)), k


# ---- 7. the C++ layer -------------------------------------------------------------------------------------------------------------------------------
def test_the_shims_setter(hip, orc, tmp_path):
    """ultrahdr::JpegRHip::setProgressive: encodeJPEGR writes uhdr_hip_jpegr_encode_batch_scans' bytes, decodeJPEGR reads them, and the
    combinations the setter refuses are refused (tests/cpp/shim_progressive_test.cpp)"""
    from tests.test_gpu_jpeg_restart import _pair
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "libultrahdr_dev_amd")
    exe = str(tmp_path / "shim_progressive_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_progressive_test.cpp"),
                           "-o", exe, "-L" + pkg, "-lultrahdr_shim", "-luhdr_hip", "-Wl,-rpath," + pkg])
    w, h = 64, 48
    p010, yuv = orc.lcg_frame(w, h, 300)
    p010.tofile(str(tmp_path / "in.p010"))
    yuv.tofile(str(tmp_path / "in.yuv"))
    r = subprocess.run([exe, str(tmp_path / "in.p010"), str(tmp_path / "in.yuv"), str(w), str(h), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    keep = []
    pairs = [_pair(orc, w, h, 300, api.MEM_HOST, keep)]
    lib = hip.load()
    assert open(tmp_path / "api1.jpgr", "rb").read() == _jpegr_scans(lib, pairs, False, PROG, api.MEM_HOST)[0]
    assert open(tmp_path / "api0.jpgr", "rb").read() == _jpegr_scans(lib, pairs, True, PROG, api.MEM_HOST)[0]
