"""-m gpu: the device JPEG encoder (csrc/uhdr_jpeg.hip) on the constructed images of tests/jpeg_encode_cases.py -- streams that end on
a chunk or a piece of the byte stuffing, 0xFF bytes on either side of those edges, blocks that share a word, a workspace that still
holds the previous call's stream -- through both of its code paths: uhdr_hip_jpeg_encode (k_jpeg_emit / k_jpeg_stuff_* behind a
memset) and uhdr_hip_jpeg_encode_batch (the _multi kernels behind k_jpeg_clear_multi).  The expectation is always the file of the CPU
checker (oracle/jpeg_oracle.c, pinned to libjpeg by tests/test_jpeg_oracle.py), byte for byte; that each image has the property it
is named for is tests/test_jpeg_encode_cases_cpu.py's business."""
import ctypes as C

import numpy as np
import pytest

from tests import jpeg_encode_cases as J

pytestmark = pytest.mark.gpu

_DEV = {}
_STALE = {}


@pytest.fixture(scope="module", autouse=True)
def _device_planes_released():
    """The planes uploaded for this file (about 25 MB, kept so that each is uploaded once) leave the device with it.  Kept alive to
    the end of the session they made tests/test_gpu_mempool.py::test_pixel_path_on_images_that_live_in_a_pool, which runs later
    and reads free device memory and maps pool chunks, read back a map of zeros; releasing them here is what it takes, emptying
    the allocator's cache alone is not."""
    yield
    import torch
    _DEV.clear()
    _STALE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _planes_dev(it):
    """the item's planes in device memory (uploaded once per item)"""
    from tests.gpu_util import to_dev
    key = id(it["yb"])
    if key not in _DEV:
        _DEV[key] = (it["yb"], to_dev(it["yb"]), None if it["ub"] is None else to_dev(it["ub"]))
    return _DEV[key][1], _DEV[key][2]


def _image(hip, it, device):
    gray = it["ub"] is None
    if device:
        dy, du = _planes_dev(it)
        py, pu = dy.data_ptr(), (None if gray else du.data_ptr())
    else:
        py, pu = it["yb"].ctypes.data, (None if gray else it["ub"].ctypes.data)
    return hip.Image(py, it["w"], it["h"], hip.CG_UNSPECIFIED, pu, it["ls"], it["cs"], hip.PIX_FMT_MONOCHROME if gray else hip.PIX_FMT_YUV420)


def _room(it, want):
    return len(want) + 4096


def _single(lib, hip, it, device, out=None, cap=None):
    """uhdr_hip_jpeg_encode, planes and output both in device or both in host memory -> (status, size, buffer as numpy).  out: a
    device tensor to write into (at its start) instead of a fresh one"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    img = _image(hip, it, device)
    n = C.c_size_t()
    icc = it.get("icc")
    iccn = len(icc) if icc else 0
    if device:
        buf = out if out is not None else dev_empty(cap + 64, 0xCD)
        rc = lib.uhdr_hip_jpeg_encode(C.byref(img), it["q"], icc, iccn, C.c_void_p(buf.data_ptr()), cap, C.byref(n), hip.MEM_DEVICE, stream_ptr())
        return rc, n.value, to_host(buf)
    buf = np.full(cap + 64, 0xCD, np.uint8)
    rc = lib.uhdr_hip_jpeg_encode(C.byref(img), it["q"], icc, iccn, C.c_void_p(buf.ctypes.data), cap, C.byref(n), hip.MEM_HOST, None)
    return rc, n.value, buf


def _batch(lib, hip, items, device, outs=None, caps=None, wants=None):
    """uhdr_hip_jpeg_encode_batch, everything in device or everything in host memory -> (rc, statuses, sizes, buffers as numpy)"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    n = len(items)
    imgs = hip.image_array([_image(hip, it, device) for it in items])
    caps = caps if caps is not None else [_room(it, w) for it, w in zip(items, wants)]
    if outs is None:
        outs = [dev_empty(c + 64, 0xCD) if device else np.full(c + 64, 0xCD, np.uint8) for c in caps]
    ptrs = (C.c_void_p * n)(*[(o.data_ptr() if device else o.ctypes.data) for o in outs])
    iccs = [it.get("icc") for it in items]
    icc = iccn = None
    keep = [np.frombuffer(x, np.uint8) if x else None for x in iccs]
    if any(iccs):
        icc = (C.c_void_p * n)(*[k.ctypes.data if k is not None else None for k in keep])
        iccn = (C.c_size_t * n)(*[len(x) if x else 0 for x in iccs])
    size, stat = (C.c_size_t * n)(), (C.c_int * n)(*([12345] * n))
    rc = lib.uhdr_hip_jpeg_encode_batch(n, imgs, (C.c_int * n)(*[it["q"] for it in items]), icc, iccn, ptrs, (C.c_size_t * n)(*caps), size, stat,
                                        hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr() if device else None)
    return rc, list(stat), list(size), [to_host(o) if device else o for o in outs]


def _same(buf, n, want, what):
    """the first n bytes of buf are `want`, and the fill behind them is untouched"""
    assert n == len(want), (what, n, len(want))
    got = buf[:n].tobytes()
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.nonzero(a != b)[0][0])
        hl = J.parse_file(want)["header_len"]
        raise AssertionError("%s: %d bytes differ, the first at %d (header %d bytes): got %s, want %s" % (
            what, int((a != b).sum()), at, hl, got[at:at + 8].hex(), want[at:at + 8].hex()))
    assert (buf[n:] == 0xCD).all(), (what, "bytes behind the file were written")


def _tiny(seed):
    rng = np.random.RandomState(seed)
    y = rng.randint(0, 256, (16, 24)).astype(np.uint8)
    if seed % 2:
        return dict(yb=y, ub=None, w=24, h=16, ls=24, cs=0, q=75)
    return dict(yb=y, ub=rng.randint(0, 256, (16, 12)).astype(np.uint8), w=24, h=16, ls=24, cs=12, q=95)


_TINY = [_tiny(1), _tiny(2), _tiny(3)]

_PATHS = [(name, path) for name in J.CASES for path in (("single_dev", "batch_of_one") if name in J.LARGE else
                                                        ("single_dev", "single_host", "batch_of_one", "mixed_batch"))]


@pytest.mark.parametrize("name,path", _PATHS, ids=["%s-%s" % p for p in _PATHS])
def test_case_equals_the_oracle(hip, orc, name, path):
    """every case through the single call (device and host memory) and the batch call: alone (device, then host memory) and inside
    [tiny, case, tiny, stride_2nd_trip, len_16384, case, tiny], where job_of's starts and a job whose stuffing workgroups stride
    sit next to jobs of one workgroup.  (stride_2nd_trip is checked in every such batch; pieces_257 runs on its own.)"""
    lib = hip.load()
    it = J.case(name)
    want = J.oracle_file(orc, it)
    if path in ("single_dev", "single_host"):
        rc, n, buf = _single(lib, hip, it, path == "single_dev", cap=_room(it, want))
        assert rc == 0
        _same(buf, n, want, (name, path))
    elif path == "batch_of_one":
        for device in (True,) if name in J.LARGE else (True, False):
            rc, stat, size, bufs = _batch(lib, hip, [it], device, wants=[want])
            assert rc == 0 and stat == [0]
            _same(bufs[0], size[0], want, (name, path, device))
    else:
        items = [_TINY[0], it, _TINY[1], J.case("stride_2nd_trip"), J.case("len_16384"), it, _TINY[2]]
        wants = [J.oracle_file(orc, x) for x in items]
        rc, stat, size, bufs = _batch(lib, hip, items, True, wants=wants)
        assert rc == 0 and stat == [0] * len(items)
        for k in range(len(items)):
            _same(bufs[k], size[k], wants[k], (name, path, k))


def _stale_items(orc):
    """four single-plane images of ff_dense's size at quality 100.  A: ff_dense (49152 stream bytes, one in three 0xFF) and noise
    (about 1.4 MB); B: flat 128 (ff_none_long's content: 12288 bytes of 00101000 10100010 10001010) and six_bit_blocks' content"""
    d = J.case("ff_dense")
    bw, bh = d["w"] // 8, d["h"] // 8
    if "noise" not in _STALE:
        _STALE["noise"] = J._item(np.random.RandomState(41).randint(0, 256, (d["h"], d["w"])).astype(np.uint8))
        _STALE["flat"] = J.ff_none_long(bw, bh)
        _STALE["six"] = J.six_bit_blocks(bw, bh)
    items = [d, _STALE["noise"], _STALE["flat"], _STALE["six"]]
    return items, [J.oracle_file(orc, x) for x in items]


def test_batch_after_batch_in_a_workspace_that_holds_the_previous_streams(hip, orc):
    """k_jpeg_clear_multi clears only the words the new stream will occupy and the emit ORs into them: batch A, then batch B of the
    same sizes in the same order (so the slices of the round's workspace coincide), then A again, on one stream"""
    lib = hip.load()
    (dense, noise, flat, six), (wd, wn, wf, ws) = _stale_items(orc)
    for rnd, (items, wants) in enumerate((([dense, noise], [wd, wn]), ([flat, six], [wf, ws]), ([dense, noise], [wd, wn]), ([flat, six], [wf, ws]))):
        rc, stat, size, bufs = _batch(lib, hip, items, True, wants=wants)
        assert rc == 0 and stat == [0, 0]
        for k in range(2):
            _same(bufs[k], size[k], wants[k], ("round", rnd, "job", k))


def test_jobs_that_trade_workspace_slices_inside_one_batch(hip, orc):
    lib = hip.load()
    (dense, noise, flat, six), (wd, wn, wf, ws) = _stale_items(orc)
    for rnd, (items, wants) in enumerate((([dense, flat], [wd, wf]), ([flat, dense], [wf, wd]), ([noise, six], [wn, ws]), ([six, noise], [ws, wn]),
                                          ([dense, flat], [wd, wf]))):
        rc, stat, size, bufs = _batch(lib, hip, items, True, wants=wants)
        assert rc == 0 and stat == [0, 0]
        for k in range(2):
            _same(bufs[k], size[k], wants[k], ("round", rnd, "job", k))


def test_single_calls_in_a_workspace_that_holds_the_previous_stream(hip, orc):
    lib = hip.load()
    (dense, noise, flat, six), (wd, wn, wf, ws) = _stale_items(orc)
    for rnd, (it, want) in enumerate(((dense, wd), (flat, wf), (dense, wd), (noise, wn), (six, ws), (noise, wn))):
        rc, n, buf = _single(lib, hip, it, True, cap=_room(it, want))
        assert rc == 0
        _same(buf, n, want, ("call", rnd))


@pytest.mark.parametrize("name", ["ff_at_16383_and_16384", "ff_dense"])
@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_output_pointer_at_every_alignment(hip, orc, name, batch):
    """the copy's split into head bytes, dwords and tail bytes follows (out + header_len + stuffed bytes in front) & 3"""
    from tests.gpu_util import dev_empty
    lib = hip.load()
    it = J.case(name)
    want = J.oracle_file(orc, it)
    base = dev_empty(len(want) + 4096, 0xCD)
    assert base.data_ptr() % 256 == 0
    for off in range(4):
        base.fill_(0xCD)
        out = base[off:]
        cap = len(want) + 64
        if batch:
            rc, stat, size, bufs = _batch(lib, hip, [it], True, outs=[out], caps=[cap])
            assert rc == 0 and stat == [0]
            n, buf = size[0], bufs[0]
        else:
            rc, n, buf = _single(lib, hip, it, True, out=out, cap=cap)
            assert rc == 0
        _same(buf, n, want, (name, "offset", off))
        assert (base[:off].cpu().numpy() == 0xCD).all()


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_header_length_at_every_residue(hip, orc, batch):
    """4:2:0 with an ICC segment of 200, 201, 202 and 203 bytes: header_len takes all four residues modulo 4"""
    lib = hip.load()
    residues = set()
    for name in ("c420_wg_edge", "dc_cat11"):
        for extra in range(4):
            it = dict(J.case(name))
            it.pop("_want", None)
            it["icc"] = bytes((3 * k + extra) % 256 for k in range(200 + extra))
            want = J.oracle_file(orc, it)
            residues.add(J.parse_file(want)["header_len"] % 4)
            for device in (True, False):
                if batch:
                    rc, stat, size, bufs = _batch(lib, hip, [_TINY[0], it], device, wants=[J.oracle_file(orc, _TINY[0]), want])
                    assert rc == 0 and stat == [0, 0]
                    _same(bufs[1], size[1], want, (name, extra, device))
                else:
                    rc, n, buf = _single(lib, hip, it, device, cap=_room(it, want))
                    assert rc == 0
                    _same(buf, n, want, (name, extra, device))
    assert residues == {0, 1, 2, 3}


@pytest.mark.parametrize("name", ["len_16384", "ff_last_byte", "ff_at_16383_and_16384"])
@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_capacity_edges_inside_one_allocation(hip, orc, name, batch):
    """a device buffer of n + 64 bytes of 0xCD and a capacity at, just below, and far below the file's length n: only n succeeds, the
    size is reported in every case, no byte at or behind the capacity is written -- the guard can fall inside a dword store -- and
    the bytes below it are the file's (stuff_copy_wg writes them, so that is pinned)"""
    from tests.gpu_util import dev_empty
    lib = hip.load()
    it = J.case(name)
    want = J.oracle_file(orc, it)
    n, hl = len(want), J.parse_file(want)["header_len"]
    wb = np.frombuffer(want, np.uint8)
    for cap in (n, n - 1, n - 2, n - 3, n - 4, n - 5, hl, hl + 1):
        out = dev_empty(n + 64, 0xCD)
        if batch:
            rc, stat, size, bufs = _batch(lib, hip, [it], True, outs=[out], caps=[cap])
            rc, got_n, buf = stat[0], size[0], bufs[0]
        else:
            rc, got_n, buf = _single(lib, hip, it, True, out=out, cap=cap)
        assert rc == (0 if cap == n else hip.ERROR_INSUFFICIENT_RESOURCE) and got_n == n, (name, cap, rc, got_n)
        assert (buf[cap:n + 64] == 0xCD).all(), (name, cap, "written at", cap + int(np.nonzero(buf[cap:n + 64] != 0xCD)[0][0]))
        assert np.array_equal(buf[:cap], wb[:cap]), (name, cap, "first difference at", int(np.nonzero(buf[:cap] != wb[:cap])[0][0]))


def test_every_quality_in_one_call_of_two_rounds(hip, orc):
    """a 32 x 16 4:2:0 image and a single-plane image of `extreme` content at each quality 1..100: 200 jobs, more than a round holds"""
    from tests.test_jpeg_oracle import _content, _planes
    lib = hip.load()
    rng = np.random.RandomState(6)
    y, u, v = _content("extreme", 32, 16, rng)
    yb, ub = _planes(y, u, v, 32, 16, rng)
    gy = _content("extreme", 40, 24, rng)[0]
    items = []
    for q in range(1, 101):
        items.append(dict(yb=yb, ub=ub, w=32, h=16, ls=32, cs=16, q=q))
        items.append(dict(yb=gy, ub=None, w=40, h=24, ls=40, cs=0, q=q))
    assert J.MAX_BATCH_JOBS < len(items) <= 2 * J.MAX_BATCH_JOBS
    wants = [J.oracle_file(orc, it) for it in items]
    for device in (True, False):
        rc, stat, size, bufs = _batch(lib, hip, items, device, wants=wants)
        assert rc == 0 and stat == [0] * len(items)
        for k, it in enumerate(items):
            _same(bufs[k], size[k], wants[k], ("quality", it["q"], "gray" if it["ub"] is None else "420", device))
