"""-m gpu: the device JPEG decoder on the constructed streams of tests/jpeg_stream_cases.py (what each case reaches: DESIGN.md,
"JPEG decoder: constructed streams"; that each file has the properties it exists for: tests/test_jpeg_streams_cpu.py).

For every case, in device and in host memory: status 0, the sizes of the file, the planes of the CPU restatement byte for byte
(which the CPU tests hold equal to libjpeg's), and nothing written behind them.  Batches of these files through
uhdr_hip_jpeg_decode_batch give what the single calls give, a failing file between them included.  The route is proved with
uhdr_hip_jpeg_decode_last_sync_launches: the `no_sync` cases need more launches of the synchronisation kernel than the ring of
"changed" flags has slots (64), a small file with the standard tables needs no more than the launches in front of the first look.

Measured on an MI355X: no_sync_gray 154 launches and 38 looks at the ring (601 subsequences), no_sync_420 94 launches and 23
looks (361 subsequences), the standard-table file 6 launches and one look."""
import ctypes as C

import numpy as np
import pytest

from tests import jpeg_stream_cases as K

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(orc, name):
    """(file, planes of the CPU restatement, w, h, gray), once per case"""
    if name not in _WANT:
        data = K.case(name)[0]
        st, planes, w, h, gray = orc.jpeg_decode("orc", data)
        assert st > 0, (name, st)
        _WANT[name] = (data, planes, w, h, gray)
    return _WANT[name]


def _decode(lib, hip, data, device):
    """-> (status, planes, bytes behind the planes that changed, descriptor): the output buffer is 0xCD everywhere and 64 bytes
    longer than the capacity the call is told"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    buf = np.frombuffer(data + b"\0" * 8, np.uint8)
    desc = hip.Image()
    probe = lib.uhdr_hip_jpeg_decode(C.c_void_p(buf.ctypes.data), len(data), None, 0, C.byref(desc), hip.MEM_HOST, None)
    if probe != hip.ERROR_INSUFFICIENT_RESOURCE:
        return probe, None, 0, desc
    mono = desc.pixelFormat == hip.PIX_FMT_MONOCHROME
    need = desc.width * desc.height + (0 if mono else 2 * (desc.width * desc.height // 4))
    if device:
        dout = dev_empty(need + 64, 0xCD)
        rc = lib.uhdr_hip_jpeg_decode(C.c_void_p(buf.ctypes.data), len(data), C.c_void_p(dout.data_ptr()), need, C.byref(desc), hip.MEM_DEVICE, stream_ptr())
        out = to_host(dout, need + 64).copy()
    else:
        out = np.full(need + 64, 0xCD, np.uint8)
        rc = lib.uhdr_hip_jpeg_decode(C.c_void_p(buf.ctypes.data), len(data), C.c_void_p(out.ctypes.data), need, C.byref(desc), hip.MEM_HOST, None)
    return rc, out[:need], int((out[need:] != 0xCD).sum()), desc


def _launches(lib):
    looks, first = C.c_int(-1), C.c_int(-1)
    n = lib.uhdr_hip_jpeg_decode_last_sync_launches(C.byref(looks), C.byref(first))
    return n, looks.value, first.value


def _standard_file(orc):
    from tests.test_jpeg_oracle import _content
    y, u, v = _content("smooth", 64, 48, np.random.RandomState(4))
    uv = np.ascontiguousarray(np.concatenate([u.reshape(-1), v.reshape(-1)]))
    return orc.jpeg_encode("orc", np.ascontiguousarray(y), uv, 64, 48, 90)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_constructed_stream_decodes_to_the_restatements_planes(hip, orc, name, device):
    lib = hip.load()
    data, want, w, h, gray = _want(orc, name)
    rc, got, spilled, desc = _decode(lib, hip, data, device)
    assert rc == 0, (name, rc)
    assert (desc.width, desc.height) == (w, h) and (desc.pixelFormat == hip.PIX_FMT_MONOCHROME) == bool(gray), name
    assert got.size == want.size and spilled == 0, (name, got.size, want.size, spilled)
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.nonzero(got != want)[0][:8])


def test_no_sync_streams_wrap_the_ring_and_a_standard_file_needs_one_look(hip, orc):
    """uhdr_hip_jpeg_decode_last_sync_launches after each decode.  no_sync_gray / no_sync_420: more than 64 launches -- the ring
    index `launch & 63` wrapped -- at least 3 looks at the ring, and no more launches than the host's limit (subsequences + 34).  A
    64x48 file with the standard tables: exactly the launches in front of the first look, one look."""
    lib = hip.load()
    counts = {}
    for name in ("no_sync_gray", "no_sync_420"):
        data, want, w, h, gray = _want(orc, name)
        rc, got, spilled, _ = _decode(lib, hip, data, True)
        n, looks, first = _launches(lib)
        counts[name] = (n, looks, K.case(name)[1]["nsub"])
        print("%s: %d subsequences, %d launches, %d looks at the ring" % (name, counts[name][2], n, looks))
        assert rc == 0 and np.array_equal(got, want), name
        assert n > 64 and looks >= 3, (name, n, looks)
        assert n <= counts[name][2] + 34, (name, n)
        # the true state needs a round per subsequence, four rounds per launch: the files cannot have taken fewer launches
        assert n >= (counts[name][2] - 1) // 4, (name, n)
    small = _standard_file(orc)
    rc, got, spilled, _ = _decode(lib, hip, small, True)
    n, looks, first = _launches(lib)
    print("standard tables, 64x48: %d launches, %d looks (launches in front of the first look: %d)" % (n, looks, first))
    assert rc == 0 and np.array_equal(got, orc.jpeg_decode("orc", small)[1])
    assert first > 0 and n == first and looks == 1, (n, looks, first)


def test_a_long_decode_leaves_nothing_behind_for_the_next_call(hip, orc):
    """no_sync_gray (154 launches, the ring wrapped twice), a small standard file, no_sync_gray again, on one stream: the flags and
    states a long decode leaves in the pooled workspace do not reach the next call"""
    lib = hip.load()
    data, want, w, h, gray = _want(orc, "no_sync_gray")
    small = _standard_file(orc)
    small_want = orc.jpeg_decode("orc", small)[1]
    first_counts = None
    for device in (True, False):
        for k, (d, wnt) in enumerate(((data, want), (small, small_want), (data, want), (small, small_want))):
            rc, got, spilled, _ = _decode(lib, hip, d, device)
            assert rc == 0 and spilled == 0 and np.array_equal(got, wnt), (device, k, rc)
            c = _launches(lib)
            if k == 0 and first_counts is None:
                first_counts = c
            assert c == (first_counts if k % 2 == 0 else (c[2], 1, c[2])), (device, k, c, first_counts)


class _Batch:
    def __init__(self, hip, files, device):
        self.hip, self.device = hip, device
        self.n = n = len(files)
        self.bufs = [np.frombuffer(f + b"\0" * 8, np.uint8) for f in files]
        self.jp = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.js = (C.c_size_t * n)(*[len(f) for f in files])
        self.descs = (hip.Image * n)()
        self.stat = (C.c_int * n)(*([77] * n))

    def run(self, lib, needs):
        from tests.gpu_util import dev_empty, stream_ptr, to_host
        hip, n = self.hip, self.n
        keep, ptrs = [], []
        for k in range(n):
            cap = needs[k] + 64
            if self.device:
                t = dev_empty(cap, 0xCD)
                keep.append(t)
                ptrs.append(t.data_ptr())
            else:
                a = np.full(cap, 0xCD, np.uint8)
                keep.append(a)
                ptrs.append(a.ctypes.data)
        outs = (C.c_void_p * n)(*ptrs)
        caps = (C.c_size_t * n)(*needs)
        rc = lib.uhdr_hip_jpeg_decode_batch(n, self.jp, self.js, hip.DECODE_TO_YCBCR, outs, caps, self.descs, self.stat,
                                            hip.MEM_DEVICE if self.device else hip.MEM_HOST, stream_ptr() if self.device else None)
        res = [to_host(t, needs[k] + 64).copy() if self.device else t for k, t in enumerate(keep)]
        return rc, [self.stat[k] for k in range(n)], res


def _truncated(orc):
    """a valid header over entropy-coded data cut short, EOI glued on: the scan ends before its last block -- a status on the device"""
    good = _standard_file(orc)
    return good[:len(good) - 200] + b"\xff\xd9"


def _batch_against_singles(hip, orc, items, device):
    """items: case names, or ("file", bytes) for a file that must FAIL.  Every file of the batch: the status and the planes of its
    single decode, nothing behind them; the failing one its error status and an untouched buffer"""
    lib = hip.load()
    files, wants, needs = [], [], []
    for it in items:
        if isinstance(it, str):
            data, want, w, h, gray = _want(orc, it)
            files.append(data)
            wants.append(want)
            needs.append(want.size)
        else:
            files.append(it[1])
            wants.append(None)
            needs.append(64 * 48 * 3 // 2)
    single = [_decode(lib, hip, f, device) for f in files]
    rc, stats, outs = _Batch(hip, files, device).run(lib, needs)
    for k, it in enumerate(items):
        assert stats[k] == single[k][0], (k, it if isinstance(it, str) else "failing file", stats[k], single[k][0])
        if wants[k] is None:
            assert stats[k] == hip.UNKNOWN_ERROR, (k, stats[k])
            continue
        assert stats[k] == 0, (k, it, stats[k])
        assert np.array_equal(outs[k][:needs[k]], wants[k]), (k, it, int((outs[k][:needs[k]] != wants[k]).sum()))
        assert np.array_equal(outs[k][:needs[k]], single[k][1])
        assert (outs[k][needs[k]:] == 0xCD).all(), (k, it)
    assert rc == (hip.UNKNOWN_ERROR if any(w is None for w in wants) else 0)


_MIXED = ["stuffing_edges_len_16384", "stuffing_edges_len_16385", "no_sync_gray", "flat_one_bit_gray", "TRUNCATED", "deep_codes_gray"]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_mixed_batch_equals_the_single_decodes(hip, orc, order, device):
    """[a scan of exactly 256 chunks, one of 257 (a second unstuffing workgroup for one byte), no_sync_gray (154 launches while the
    others wait), flat_one_bit_gray, a truncated file, deep_codes_gray] and the same reversed: one decoder launch per step for all
    of them, per-image slices of the batch's scan arrays, the failing file in the middle"""
    assert K.case("stuffing_edges_len_16384")[1]["scan_bytes"] == 256 * K.CHUNK and K.case("stuffing_edges_len_16385")[1]["scan_bytes"] == 256 * K.CHUNK + 1
    items = [("file", _truncated(orc)) if x == "TRUNCATED" else x for x in (_MIXED if order == "forward" else _MIXED[::-1])]
    _batch_against_singles(hip, orc, items, device)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_dc_extremes_on_both_sides_of_a_failing_file(hip, orc, device):
    """dc_extremes (4160 blocks: its slice of the batch's DC scan ends 64 blocks into a scan tile), the truncated file, and
    dc_extremes_rst (predictor resets every 100 blocks): DC sums of +-2047 steps must not leak across images or intervals"""
    _batch_against_singles(hip, orc, ["dc_extremes", ("file", _truncated(orc)), "dc_extremes_rst", "dc_extremes"], device)
