"""-m gpu: k_effect, k_effect_rot and k_effect_chain where their index arithmetic changes character -- beyond the first block of
4096 columns, beyond two 64 x 64 tiles, beyond the grid's 65535 rows, at the capacity of the LDS stretch and of the tile span, and
through every store route (16-byte, dword, byte) -- byte for byte against the oracle's editorhelper restatement, which
tests/test_oracle_pins.py holds to the reference's object code at these very shapes.  The shapes, and the class every chain's planes
must get, are in tests/effects_geometry_cases.py; tests/test_effects_chain_cpu.py checks the same list without a GPU.  Every
destination lies 0, 4 and 1 bytes past a 256-byte boundary in turn; buffers are prefilled and compared whole, or their guard bytes
are asserted untouched.  No tolerance anywhere.

One route is out of reach and stated as such: FXC_TILE's own row loop wraps only beyond 65535 tiles of 64 rows, 4 M rows, which at
one byte per row is an output of 4 MiB and a row table of 16 MiB; the row loop's second trip is taken by the row classes
(rows_past_grid, the mixed call) and by k_effect instead, and the tile loop's stride is the same expression."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import effects_chain_cases as K
from tests import effects_geometry_cases as G
from tests.test_gpu_effects_batch import FILL, _check_image, _run, _untouched_mask

pytestmark = pytest.mark.gpu
DST_OFFSETS = (0, 4, 1)     # from a 256-byte boundary: the 16-byte, the dword and the byte stores
SRC_OFFSETS = (0, 5)        # ASC / DESC: the aligned 16-byte copy and its gather fallback; LDS / TILE: dword loads clamped at the plane's first byte
PAD = 256


def _classes(hip, w, h, mono, chain):
    fused, count, cls = C.c_int(-1), C.c_size_t(99), (C.c_int * 8)()
    rc = hip.load().uhdr_hip_effect_chain_classes(w, h, 0, 0, hip.PIX_FMT_MONOCHROME if mono else hip.PIX_FMT_YUV420, K.effect_array(hip, chain),
                                                  len(chain), C.byref(fused), cls, 8, C.byref(count))
    return rc, fused.value, tuple(cls[:count.value])


@functools.lru_cache(maxsize=None)
def _source(w, h, mono, seed):
    src = K.source(w, h, mono, seed)[0]
    src.setflags(write=False)
    return src


# ---------------------------------------------------------------------------------------------------
# chains through uhdr_hip_add_effects_batch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CHAINS, ids=[c[0] for c in G.CHAINS])
def test_chain_matches_the_oracle_on_its_declared_route(hip, orc, case):
    name, w, h, mono, chain, cls = case
    assert _classes(hip, w, h, mono, chain) == (0, 1, cls), name          # a composer change must not move the case off its route
    src = _source(w, h, mono, 9000 + G.CHAINS.index(case))
    expect = K.oracle_run(orc, src, w, h, mono, chain)
    for src_off in SRC_OFFSETS:
        for align in DST_OFFSETS:
            j = {"w": w, "h": h, "mono": mono, "src": src, "src_off": src_off, "expect": expect}
            rc, st, descs, got, offs, base = _run(hip, [j], chain, align=align)
            assert rc == st[0] == 0, (name, align, src_off, rc)
            assert (base + offs[0]) % 256 == align
            n = _check_image(hip, orc, j, chain, descs[0], got, offs[0], base)
            assert (got[_untouched_mask(got.size, [(offs[0], n)])] == FILL).all(), (name, align, src_off)


@pytest.mark.parametrize("align", DST_OFFSETS + (None,))
def test_one_call_with_jobs_of_every_class_and_extent(hip, orc, align):
    """the grid is the maximum over the jobs (3 blocks across, 65535 rows): a wide ASC job, a tall one, a TILE job, an LDS job and
    a 1 x 1 image, each of which must ignore the blocks that belong to the others' extents"""
    jobs = []
    for k, (w, h, mono, cls) in enumerate(G.MIXED):
        assert _classes(hip, w, h, mono, G.MIXED_CHAIN) == (0, 1, cls), (w, h)
        jobs.append({"w": w, "h": h, "mono": mono, "src": _source(w, h, mono, 9500 + k), "src_off": 5 * (k % 2)})
    rc, st, descs, got, offs, base = _run(hip, jobs, G.MIXED_CHAIN, align=align)
    assert rc == 0 and st == [0] * len(jobs), st
    written = [(offs[i], _check_image(hip, orc, j, G.MIXED_CHAIN, descs[i], got, offs[i], base)) for i, j in enumerate(jobs)]
    assert (got[_untouched_mask(got.size, written)] == FILL).all()


# ---------------------------------------------------------------------------------------------------
# single effects in device memory
# ---------------------------------------------------------------------------------------------------
def _single_image(orc, w, h, mono, ls, seed):
    """-> (bytes, oracle image): chroma right behind luma"""
    stride = ls or w
    rng = np.random.RandomState(seed)
    buf = rng.randint(0, 256, stride * h + (0 if mono else (stride // 2) * h)).astype(np.uint8)
    return buf, orc.Image(buf.ctypes.data, w, h, 1, None, ls, 0, orc.FMT_MONOCHROME if mono else orc.FMT_YUV420)


@pytest.mark.parametrize("case", G.SINGLES, ids=[c[0] for c in G.SINGLES])
def test_single_effects_match_the_oracle(hip, orc, case):
    from tests.gpu_util import dev_empty, stream_ptr, to_dev, to_host
    name, w, h, mono, effects, ls, src_off = case
    lib, L = hip.load(), orc.load()
    buf, o_in = _single_image(orc, w, h, mono, ls, 9700 + G.SINGLES.index(case))
    d_buf = to_dev(np.concatenate([np.zeros(src_off, np.uint8), buf]))
    assert d_buf.data_ptr() % 256 == 0
    for fx, args in effects:
        ow, oh = K.sizes(w, h, [tuple([{"crop": 0, "mirror": 1, "rotate": 2, "resize": 3}[fx]] + list(args) + [0] * (4 - len(args)))])[-1]
        nbytes = 2 * max(buf.size, K.packed(mono, ow, oh)) + 1024
        o_out = np.full(nbytes, 0xCC, np.uint8)
        o_img = orc.Image(o_out.ctypes.data, 0, 0, -1, None, 0, 0, -1)
        assert getattr(L, "orc_" + fx)(C.byref(o_in), *args, C.byref(o_img)) == 0
        assert (o_out[:K.packed(mono, ow, oh)] != 0xCC).any() and (o_out[-1024:] == 0xCC).all()     # (the oracle stayed inside)
        for off in DST_OFFSETS:
            d_out = dev_empty(PAD + nbytes + PAD, 0xCC)
            assert d_out.data_ptr() % 256 == 0
            ptr = d_out.data_ptr() + PAD + off
            g_in = hip.Image(d_buf.data_ptr() + src_off, w, h, 1, None, ls, 0, hip.PIX_FMT_MONOCHROME if mono else hip.PIX_FMT_YUV420)
            g_img = hip.out_image(ptr)
            rc = getattr(lib, "uhdr_hip_" + fx)(C.byref(g_in), *args, C.byref(g_img), hip.MEM_DEVICE, stream_ptr())
            assert rc == 0, (name, fx, args, off, rc)
            got = to_host(d_out)
            assert (g_img.width, g_img.height, g_img.colorGamut, g_img.luma_stride, g_img.pixelFormat) == \
                   (o_img.width, o_img.height, o_img.colorGamut, o_img.luma_stride, o_img.pixelFormat), (name, fx, args)
            if not mono:
                assert g_img.chroma_stride == o_img.chroma_stride
                assert g_img.chroma_data - ptr == o_img.chroma_data - o_out.ctypes.data
            body = got[PAD + off:PAD + off + nbytes]
            assert np.array_equal(body, o_out), (name, fx, args, off, int((body != o_out).sum()), int(np.flatnonzero(body != o_out)[0]))
            assert (got[:PAD + off] == 0xCC).all() and (got[PAD + off + nbytes:] == 0xCC).all(), (name, fx, args, off)
