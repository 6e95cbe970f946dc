"""-m gpu: uhdr_hip_add_effects_batch -- a chain of effects over n images in one launch (k_effect_chain) -- against the oracle's
addEffects (pinned to the reference's object code by tests/test_oracle_pins.py).  Pure byte movement: the result's packed extent is
bit-exact, and not one byte around it is touched."""
import ctypes as C

import numpy as np
import pytest

from tests import effects_chain_cases as K

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xEE


class Arena:
    """out[i] carved from one device allocation prefilled with 0xEE, 64 guard bytes on each side: at odd byte offsets, or with
    align = k at k bytes past a 256-byte boundary (0: the kernels' 16-byte stores, 4: their dword stores, 1: byte stores)"""

    def __init__(self, align=None):
        self.at, self.spans, self.align = GUARD + 1, [], align

    def take(self, nbytes):
        off = self.at | 1 if self.align is None else (self.at - self.align + 255) // 256 * 256 + self.align
        self.spans.append((off, nbytes))
        self.at = off + nbytes + GUARD
        return off

    def alloc(self):
        from tests.gpu_util import dev_empty
        self.dev = dev_empty(self.at + GUARD, FILL)
        assert self.align is None or self.dev.data_ptr() % 256 == 0
        return self.dev.data_ptr()

    def host(self):
        from tests.gpu_util import to_host
        return to_host(self.dev)


def _run(hip, jobs, chain, stream=None, align=None):
    """jobs: dicts with w, h, mono, src (+ ls, cs, chroma, cap, null_in, probe, src_off: the source that many bytes past a 256-byte
    boundary).  One call; -> (rc, statuses, descs, arena bytes, offsets, base)"""
    import torch
    from tests.gpu_util import to_dev, stream_ptr
    lib = hip.load()
    n = len(jobs)
    arena = Arena(align)
    keep, offs = [], []
    for j in jobs:
        size = K.sizes(j["w"], j["h"], chain)[-1]
        offs.append(arena.take(j.get("room", K.packed(j["mono"], *size))))
    base = arena.alloc()
    imgs, out, cap = (hip.Image * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    for i, j in enumerate(jobs):
        so = j.get("src_off", 0)
        d = to_dev(np.concatenate([np.zeros(so, np.uint8), j["src"]]) if so else j["src"])
        assert so == 0 or d.data_ptr() % 256 == 0
        keep.append(d)
        cptr = None
        if j.get("chroma") is not None:
            dc = to_dev(j["chroma"])
            keep.append(dc)
            cptr = dc.data_ptr()
        imgs[i] = hip.Image(None if j.get("null_in") else d.data_ptr() + so, j["w"], j["h"], j.get("gamut", 1), cptr, j.get("ls", 0), j.get("cs", 0),
                            hip.PIX_FMT_MONOCHROME if j["mono"] else hip.PIX_FMT_YUV420)
        out[i] = None if j.get("probe") else base + offs[i]
        cap[i] = 0 if j.get("probe") else j.get("cap", arena.spans[i][1])
    descs, status = (hip.Image * n)(), (C.c_int * n)(*([99] * n))
    torch.cuda.synchronize()
    s = stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    rc = lib.uhdr_hip_add_effects_batch(n, imgs, K.effect_array(hip, chain), len(chain), out, cap, descs, status, s)
    if stream is not None:
        stream.synchronize()
    return rc, list(status), descs, arena.host(), offs, base


def _expect(orc, j, chain):
    if "expect" in j:     # (computed once by a caller that runs the same image several times)
        return j["expect"]
    return K.oracle_run(orc, j["src"], j["w"], j["h"], j["mono"], chain, ls=j.get("ls", 0), cs=j.get("cs", 0), chroma=j.get("chroma"),
                        gamut=j.get("gamut", 1))


def _untouched_mask(total, written):
    m = np.ones(total, bool)
    for off, n in written:
        m[off:off + n] = False
    return m


def _check_image(hip, orc, j, chain, desc, got, off, base):
    orc_rc, obuf, odesc, ochroma = _expect(orc, j, chain)
    assert orc_rc == 0, (j["w"], j["h"], chain)
    assert (desc.width, desc.height, desc.colorGamut, desc.pixelFormat, desc.luma_stride, desc.chroma_stride) == odesc, (j["w"], j["h"], chain)
    assert desc.data == base + off
    if ochroma is not None:
        assert desc.chroma_data - desc.data == ochroma
    n = K.packed(j["mono"], desc.width, desc.height)
    assert np.array_equal(got[off:off + n], obuf[:n]), (j["w"], j["h"], j["mono"], chain, int((got[off:off + n] != obuf[:n]).sum()))
    return n


def _chains_under_test():
    return K.named_chains() + K.generated_chains(200)


def test_chains_match_the_oracle_and_touch_nothing_else(hip, orc):
    for k, (w, h, mono, chain) in enumerate(_chains_under_test()):
        src, _, _ = K.source(w, h, mono, 5000 + k)
        j = {"w": w, "h": h, "mono": mono, "src": src}
        rc, st, descs, got, offs, base = _run(hip, [j], chain)
        if K.has_odd(w, h, mono, chain):
            assert rc == st[0] == hip.ERROR_UNSUPPORTED_FEATURE, (w, h, chain)
            assert (got == FILL).all()
            continue
        assert rc == st[0] == 0, (w, h, mono, chain, rc)
        n = _check_image(hip, orc, j, chain, descs[0], got, offs[0], base)
        assert (got[_untouched_mask(got.size, [(offs[0], n)])] == FILL).all(), (w, h, mono, chain)


@pytest.mark.parametrize("mono", [False, True])
def test_first_step_reads_strided_and_separate_planes(hip, orc, mono):
    w, h = 48, 40
    ls, cs = w + 6, (w + 6) // 2 + 3
    rng = np.random.RandomState(9)
    for first in (K.crop(2, 41, 4, 27), K.rot(90), K.resize(40, 24)):
        chain = [first, K.mirror(1), K.rot(270)]
        jobs = [{"w": w, "h": h, "mono": mono, "src": K.source(w, h, mono, 61, ls=ls)[0], "ls": ls}]
        if not mono:
            jobs.append({"w": w, "h": h, "mono": False, "src": rng.randint(0, 256, ls * h).astype(np.uint8),
                         "chroma": rng.randint(0, 256, cs * h).astype(np.uint8), "ls": ls, "cs": cs})
        rc, st, descs, got, offs, base = _run(hip, jobs, chain)
        assert rc == 0 and st == [0] * len(jobs), (chain, st)
        written = [(offs[i], _check_image(hip, orc, j, chain, descs[i], got, offs[i], base)) for i, j in enumerate(jobs)]
        assert (got[_untouched_mask(got.size, written)] == FILL).all()
    # a mirror of a padded image: the single call's documented deviation, here too
    j = {"w": w, "h": h, "mono": mono, "src": K.source(w, h, mono, 62, ls=ls)[0], "ls": ls}
    rc, st, _, got, _, _ = _run(hip, [j], [K.mirror(1), K.rot(90)])
    assert rc == st[0] == hip.ERROR_UNSUPPORTED_FEATURE and (got == FILL).all()


def test_seventy_images_more_than_a_round_on_a_stream_of_their_own(hip, orc):
    import torch
    lib = hip.load()
    # additive for YUV420 images 44 rows high, not for higher ones (the first crop then moves rows of U into V behind a flip)
    chain = [K.mirror(0), K.crop(1, 20, 0, 43), K.rot(90), K.crop(0, 43, 2, 11), K.mirror(1)]
    rng = np.random.RandomState(70)
    jobs, want = [], []
    for i in range(70):
        mono = i % 3 == 1
        w, h = 22 + 2 * int(rng.randint(0, 40)), 44
        if mono:
            w, h = 21 + int(rng.randint(0, 60)), 44 + int(rng.randint(0, 30))
        j = {"w": w, "h": h, "mono": mono, "src": None, "gamut": i % 3}
        kind = {5: "null", 12: "crop", 19: "short", 33: "probe", 47: "odd", 64: "nonadd", 66: "short"}.get(i, "ok")
        if kind == "null":
            j["null_in"] = True
        elif kind == "crop":
            j["w"], j["mono"] = 20, False                       # the crop's right edge is outside
        elif kind == "odd":
            j["w"], j["mono"] = 23, False
        elif kind == "nonadd":
            j["w"], j["h"], j["mono"] = 28, 48, False
        j["src"] = K.source(j["w"], j["h"], j["mono"], 7000 + i)[0]
        if kind in ("short", "probe"):
            j["room"] = K.packed(j["mono"], 44, 10)
            j["cap"] = j["room"] - 1
            j["probe"] = kind == "probe"
        jobs.append(j)
        want.append({"null": hip.ERROR_BAD_PTR, "crop": hip.ERROR_INVALID_CROPPING_PARAMETERS, "short": hip.ERROR_INSUFFICIENT_RESOURCE,
                     "probe": hip.ERROR_INSUFFICIENT_RESOURCE, "odd": hip.ERROR_UNSUPPORTED_FEATURE}.get(kind, 0))
    # what the composer says about them (host only): the mix the test is about
    fused = []
    for j, wst in zip(jobs, want):
        if wst == 0:
            desc, f, cnt = hip.Image(), C.c_int(-1), C.c_size_t()
            assert lib.uhdr_hip_effect_chain_map(j["w"], j["h"], 0, 0, hip.PIX_FMT_MONOCHROME if j["mono"] else hip.PIX_FMT_YUV420,
                                                 K.effect_array(hip, chain), len(chain), C.byref(desc), C.byref(f), None, 0, C.byref(cnt)) == 0
            fused.append(f.value)
    assert fused.count(0) == 1 and fused.count(1) == 63

    stream = torch.cuda.Stream()
    rc, st, descs, got, offs, base = _run(hip, jobs, chain, stream=stream)
    assert st == want, [(i, a, b) for i, (a, b) in enumerate(zip(st, want)) if a != b]
    assert rc == hip.ERROR_BAD_PTR                               # the first one that is not NO_ERROR
    written = []
    for i, j in enumerate(jobs):
        if want[i] == 0:
            written.append((offs[i], _check_image(hip, orc, j, chain, descs[i], got, offs[i], base)))
        elif want[i] == hip.ERROR_INSUFFICIENT_RESOURCE:         # the descriptor and the size are reported, out[i] is untouched
            assert (descs[i].width, descs[i].height, descs[i].luma_stride) == (44, 10, 44)
            assert descs[i].data == (None if j.get("probe") else base + offs[i])
    assert (got[_untouched_mask(got.size, written)] == FILL).all()


def test_no_effects_copies_the_packed_extent(hip, orc):
    jobs = [{"w": 40, "h": 24, "mono": False, "src": K.source(40, 24, False, 81)[0]}, {"w": 33, "h": 9, "mono": True, "src": K.source(33, 9, True, 82)[0]}]
    rc, st, descs, got, offs, base = _run(hip, jobs, [])
    assert rc == 0 and st == [0, 0]
    written = [(offs[i], _check_image(hip, orc, j, [], descs[i], got, offs[i], base)) for i, j in enumerate(jobs)]
    assert (got[_untouched_mask(got.size, written)] == FILL).all()
