"""-m gpu: the plain-JPEG encode batches past one round, in every family of the round driver (jpeg_encode_files in csrc/uhdr_capi.hip).

A round holds at most jpeg::kMaxBatchJobs = 128 files (planes, RGBA as 4:4:4) or jpeg::kRgba420Chunk = 64 (RGBA as 4:2:0 / 4:2:2).  Each
batch here has one file more than that which passes its checks -- 129 or 65 of them, so round two holds exactly one file -- plus two
which do not: one stands among the files of round one, the other between round one's last file and round two's only file, which are
both valid.  One more file of round one gets an out_capacity one byte below its size; that size is learned from a first call with ample
capacity (a property of the file, not a tolerance).  Every batch runs in all four mem_space values, once with default options and
once with UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN plus restart_in_rows = 1 (uhdr_hip_jpeg_encode_rgba420_batch takes no options, so that run
of its family goes through uhdr_hip_jpeg_encode_rgba420_batch_opts).

Every delivered file is compared BYTE FOR BYTE with the oracle the call's own test uses: the CPU oracle's encoder and
tests/jpeg_restart_oracle.py's transcode_restart() for 4:2:0 and one-plane images (tests/test_gpu_jpeg_restart.py),
tests/jpeg_sampling_encode_oracle.py's interleaver for YUV444 / 422 / 440 planes and Pillow's own files for RGBA pixels
(tests/test_gpu_jpeg_sampling_encode.py).

The other limit of a round, 2 GiB of workspace and staging, stays untested, as it is in every other test: reaching it takes
gigabytes of images.
"""
import ctypes as C
import io

import numpy as np
import pytest

from libultrahdr_dev_amd import api
from tests import jpeg_restart_cases as RC
from tests import jpeg_restart_oracle as RO
from tests import jpeg_sampling_encode_cases as EC

pytestmark = pytest.mark.gpu
OPT = api.ENCODE_OPTIMIZE_HUFFMAN
IR = api.ERROR_INSUFFICIENT_RESOURCE
SLOT = 4096                 # bytes of output per file: several times the largest file here
SHORT = 10                  # the file whose out_capacity is one byte short (round one)
MEMS = [api.MEM_HOST, api.MEM_DEVICE, api.MEM_DEVICE_TO_HOST, api.MEM_HOST_TO_DEVICE]
# (flags, restart_interval, restart_in_rows)
SETTINGS = [(0, 0, 0), (OPT, 0, 1)]


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _with_failing(files, cap, bad):
    """`files` (cap + 1 of them, all valid) with two failing ones put in: bad(k) at place 5, among round one's files, and behind the
    last file of round one"""
    assert len(files) == cap + 1
    return files[:5] + [bad(0)] + files[5:cap] + [bad(1)] + files[cap:]


def _run(hip, call, files, mem, opts, short=None):
    """one call over files = [dict(buf=the image's bytes, desc=base pointer -> descriptor, q=, icc=)]: -> (rc, statuses, sizes, buffers)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    n = len(files)
    host_in = mem in (api.MEM_HOST, api.MEM_HOST_TO_DEVICE)
    host_out = mem in (api.MEM_HOST, api.MEM_DEVICE_TO_HOST)
    offs, total = [], 0
    for f in files:
        offs.append(total)
        total += (f["buf"].size + 63) // 64 * 64
    flat = np.zeros(total, np.uint8)
    for f, o in zip(files, offs):
        flat[o:o + f["buf"].size] = f["buf"]
    src = flat if host_in else to_dev(flat)
    base = src.ctypes.data if host_in else src.data_ptr()
    outs = np.full(n * SLOT, 0xCD, np.uint8) if host_out else dev_empty(n * SLOT, 0xCD)
    obase = outs.ctypes.data if host_out else outs.data_ptr()
    caps = [SLOT] * n
    if short is not None:
        caps[short[0]] = short[1] - 1
    iccs = [np.frombuffer(f["icc"], np.uint8) if f.get("icc") else None for f in files]
    sizes, stat = _arr(C.c_size_t, [0] * n), _arr(C.c_int, [12345] * n)
    rc = call(hip.load(), n, api.image_array([f["desc"](base + o) for f, o in zip(files, offs)]), _arr(C.c_int, [f["q"] for f in files]),
              _arr(C.c_void_p, [x.ctypes.data if x is not None else None for x in iccs]), _arr(C.c_size_t, [0 if x is None else x.size for x in iccs]),
              _arr(C.c_void_p, [obase + SLOT * k for k in range(n)]), _arr(C.c_size_t, caps), sizes, stat,
              None if opts is None else C.byref(opts), mem, stream_ptr())
    whole = outs if host_out else to_host(outs).copy()
    return rc, list(stat), list(sizes), [whole[SLOT * k:SLOT * (k + 1)] for k in range(n)]


def _check_family(hip, call, files, want_of, call_default=None):
    """files: dicts as _run takes them, `fail` set to the status of a file that fails its checks.  want_of(file, flags, ri, rows): the
    oracle's bytes."""
    n = len(files)
    for flags, ri, rows in SETTINGS:
        default = (flags, ri, rows) == (0, 0, 0)
        opts = None if default else api.encode_opts(flags, ri, rows)
        fn = call_default if default and call_default is not None else call
        want = [None if f.get("fail") else want_of(f, flags, ri, rows) for f in files]
        expect = [f.get("fail", 0) for f in files]
        first = next(s for s in expect if s != 0)
        # ample capacity: every file that passes its checks is the oracle's, and the short file's size is learned here
        rc, stat, sizes, bufs = _run(hip, fn, files, api.MEM_DEVICE, opts)
        assert stat == expect and rc == first, (rc, [(k, s) for k, s in enumerate(stat) if s != expect[k]])
        for k in range(n):
            if want[k] is None:
                assert (bufs[k] == 0xCD).all(), k
                continue
            assert sizes[k] == len(want[k]) and bufs[k][:sizes[k]].tobytes() == want[k] and (bufs[k][sizes[k]:] == 0xCD).all(), (k, flags, sizes[k], len(want[k]))
        true_size = sizes[SHORT]
        assert want[SHORT] is not None and 0 < true_size < SLOT
        expect[SHORT] = IR
        for mem in MEMS:
            rc, stat, sizes2, bufs = _run(hip, fn, files, mem, opts, short=(SHORT, true_size))
            tag = (mem, flags)
            assert stat == expect and rc == first, tag + (rc, [(k, s) for k, s in enumerate(stat) if s != expect[k]])
            assert sizes2[SHORT] == true_size, tag
            host_out = mem in (api.MEM_HOST, api.MEM_DEVICE_TO_HOST)
            # a file that does not fit: nothing behind its capacity in device memory, nothing at all in host memory
            assert (bufs[SHORT][0 if host_out else true_size - 1:] == 0xCD).all(), tag
            for k in range(n):
                if k == SHORT:
                    continue
                if want[k] is None:
                    assert (bufs[k] == 0xCD).all(), tag + (k,)
                else:
                    assert sizes2[k] == len(want[k]) and bufs[k][:sizes2[k]].tobytes() == want[k] and (bufs[k][sizes2[k]:] == 0xCD).all(), tag + (k,)


# ---- planes ----------------------------------------------------------------------------------------------------------------------------
def _planes_files():
    rng = np.random.RandomState(2101)
    files = []
    for k in range(129):
        q = (50, 90, 100)[k % 3]
        icc = bytes(range(1 + k % 40)) if k % 5 == 0 else None
        kind = {1: "mono", 3: (1, 1), 5: (2, 1), 7: (1, 2)}.get(k % 8)
        if kind is None or kind == "mono":
            w, h = (8, 8) if kind == "mono" else (16, 16)
            y = rng.randint(0, 256, (h, w)).astype(np.uint8)
            if kind == "mono":
                it = RC.plane_item(y, q)
                buf, fmt = it["yb"], api.PIX_FMT_MONOCHROME
            else:
                it = RC.yuv_item(y, rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8), rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8), q)
                buf, fmt = np.concatenate([it["yb"], it["ub"]]), api.PIX_FMT_YUV420
            it["icc"] = icc
            desc = (lambda it, fmt: lambda p: api.Image(p, it["w"], it["h"], api.CG_UNSPECIFIED, None if it["ub"] is None else p + it["w"] * it["h"],
                                                        it["ls"], it["cs"], fmt))(it, fmt)
            files.append(dict(buf=buf, desc=desc, q=q, icc=icc, old=it))
        else:
            hs, vs = kind
            if k in (3, 7):       # libjpeg's own planes of that size (tests/golden/encode_sampling/)
                y, cb, cr, _ = EC.golden(17, 9, hs, vs, 90)
                q = 90
            else:
                y, cb, cr = EC.planes(17, 9, hs, vs, 2101 + k)
            it = EC.item(y, cb, cr, hs, vs, q, icc=icc)
            files.append(dict(buf=EC.laid_out(it)[0], desc=(lambda it: lambda p: EC.descriptor(it, p))(it), q=q, icc=icc, sampled=it))
    return files


def test_planes_batch_of_two_rounds(hip, orc):
    files = _planes_files()
    assert [f["desc"](0).pixelFormat for f in files[:8]] == [api.PIX_FMT_YUV420, api.PIX_FMT_MONOCHROME, api.PIX_FMT_YUV420, api.PIX_FMT_YUV444,
                                                           api.PIX_FMT_YUV420, api.PIX_FMT_YUV422, api.PIX_FMT_YUV420, api.PIX_FMT_YUV440]

    def bad(k):
        f = dict(files[2 if k == 0 else 3])

        def desc(p, inner=f["desc"]):
            d = inner(p)
            if k == 0:
                d.width = 15                       # an odd 4:2:0 image: RESOLUTION_MISMATCH
            else:
                d.chroma_stride = d.width - 1      # a YUV444 image whose chroma rows are too short: INVALID_STRIDE
            return d
        f["desc"], f["fail"] = desc, api.ERROR_RESOLUTION_MISMATCH if k == 0 else api.ERROR_INVALID_STRIDE
        return f

    def want_of(f, flags, ri, rows):
        if "sampled" in f:
            return EC.expected(f["sampled"], ri, rows, bool(flags))
        b = RC.base_file(orc, f["old"])
        return b if (flags, ri, rows) == (0, 0, 0) else RO.transcode_restart(b, ri, rows, bool(flags))

    def call(lib, n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s):
        return lib.uhdr_hip_jpeg_encode_planes_batch_opts(n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s)
    _check_family(hip, call, _with_failing(files, 128, bad), want_of)
    # the golden planes' own file, for good measure: libjpeg's, not only the interleaver's
    assert want_of(files[3], 0, 0, 0)[:2] == b"\xff\xd8" and files[3]["icc"] is None and want_of(files[3], 0, 0, 0) == EC.golden(17, 9, 1, 1, 90)[3]


# ---- RGBA --------------------------------------------------------------------------------------------------------------------------------
def _pillow(rgb, q, sub, flags, rows):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(b, "JPEG", quality=q, subsampling=sub, optimize=bool(flags), restart_marker_rows=rows)
    return b.getvalue()


def _rgba_files(n, sizes, seed, icc=None):
    rng = np.random.RandomState(seed)
    files = []
    for k in range(n):
        w, h = sizes[k % 2]
        px = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
        files.append(dict(buf=px.reshape(-1), px=px, q=(50, 90, 100)[k % 3], icc=icc if icc and k % 3 == 1 else None,
                          desc=(lambda w, h: lambda p: api.rgba8888_image(p, w, h, api.CG_BT709, w))(w, h)))
    return files


def _rgba_bad(files):
    def bad(k):
        f = dict(files[k])

        def desc(p, inner=f["desc"]):
            d = inner(p)
            if k == 0:
                d.pixelFormat = api.PIX_FMT_YUV420     # UNSUPPORTED_FEATURE
            else:
                d.luma_stride = d.width - 1            # RESOLUTION_MISMATCH
            return d
        f["desc"], f["fail"] = desc, api.ERROR_UNSUPPORTED_FEATURE if k == 0 else api.ERROR_RESOLUTION_MISMATCH
        return f
    return bad


def _rgba_want(sub):
    def want_of(f, flags, ri, rows):
        plain = _pillow(f["px"][:, :, :3], f["q"], sub, flags, rows)
        if not f["icc"]:
            return plain
        return plain[:20] + b"\xff\xe2" + (len(f["icc"]) + 2).to_bytes(2, "big") + f["icc"] + plain[20:]      # (behind the JFIF segment)
    return want_of


def test_rgba_444_batch_of_two_rounds(hip):
    lib = hip.load()
    buf, sz = np.zeros(4096, np.uint8), C.c_size_t()
    assert lib.uhdr_hip_icc_profile(hip.TF_SRGB, hip.CG_P3, C.c_void_p(buf.ctypes.data), buf.size, C.byref(sz)) == 0
    files = _rgba_files(129, ((8, 8), (17, 9)), 2102, icc=buf[:sz.value].tobytes())

    def call(lib, n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s):
        return lib.uhdr_hip_jpeg_encode_rgba_batch_opts(n, imgs, q, icc, iccn, out, cap, size, stat, api.PIX_FMT_YUV444, opts, mem, s)
    _check_family(hip, call, _with_failing(files, 128, _rgba_bad(files)), _rgba_want(0))


def test_rgba_422_batch_of_two_rounds(hip):
    files = _rgba_files(65, ((16, 16), (17, 9)), 2103)

    def call(lib, n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s):
        return lib.uhdr_hip_jpeg_encode_rgba_batch_opts(n, imgs, q, icc, iccn, out, cap, size, stat, api.PIX_FMT_YUV422, opts, mem, s)
    _check_family(hip, call, _with_failing(files, 64, _rgba_bad(files)), _rgba_want(1))


def test_rgba_420_batch_of_two_rounds(hip):
    files = _rgba_files(65, ((16, 16), (17, 9)), 2104)

    def call(lib, n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s):
        return lib.uhdr_hip_jpeg_encode_rgba420_batch_opts(n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s)

    def call_default(lib, n, imgs, q, icc, iccn, out, cap, size, stat, opts, mem, s):
        assert opts is None
        return lib.uhdr_hip_jpeg_encode_rgba420_batch(n, imgs, q, icc, iccn, out, cap, size, stat, mem, s)
    _check_family(hip, call, _with_failing(files, 64, _rgba_bad(files)), _rgba_want(2), call_default)
