"""Shared by tests/test_effects_chain_cpu.py and tests/test_gpu_effects_batch.py: the named effect chains, the fixed-seed chain
generator and the oracle run every expected value comes from (orc_add_effects, pinned to the reference's object code by
tests/test_oracle_pins.py).  Effects are (type, a, b, c, d): 0 crop(left, right, top, bottom), 1 mirror(direction),
2 rotate(degrees), 3 resize(width, height)."""
import ctypes as C

import numpy as np

UNSUPPORTED = -30000


def crop(l, r, t, b):
    return (0, l, r, t, b)


def mirror(d):
    return (1, d, 0, 0, 0)


def rot(deg):
    return (2, deg, 0, 0, 0)


def resize(w, h):
    return (3, w, h, 0, 0)


NON_ADDITIVE = (28, 44, False, [mirror(0), crop(7, 18, 19, 42), crop(4, 9, 6, 19), rot(270), crop(3, 10, 0, 3)])


# all four kinds, twice over.  (A crop that changes the height moves rows of U into V -- the reference copies the stacked U|V planes as
# one -- and a quarter turn behind it turns that into columns: such chains are the non-additive ones.  These crops keep the height.)
EIGHT_STEPS = [mirror(1), crop(4, 43, 0, 39), rot(90), resize(48, 32), mirror(0), crop(2, 45, 0, 31), rot(270), resize(24, 20)]


def named_chains():
    """[(width, height, mono, chain)]"""
    from tests.test_gpu_effects import CASES
    from tests.test_oracle_pins import FX_CHAINS
    kinds = {"crop": 0, "mirror": 1, "rotate": 2, "resize": 3}
    out = []
    for mono in (False, True):
        for name, args in CASES:
            out.append((64, 40, mono, [tuple([kinds[name]] + list(args) + [0] * (4 - len(args)))]))
        for ch in FX_CHAINS:
            out.append((128, 96, mono, [tuple(e) for e in ch]))
    out += [
        (48, 40, False, [crop(2, 41, 4, 27), rot(90), crop(2, 19, 6, 29)]),
        (48, 40, False, [crop(0, 47, 4, 27), rot(270), crop(0, 23, 6, 29), rot(90), crop(2, 13, 2, 11)]),
        (30, 22, False, [resize(110, 82), mirror(1), rot(180), resize(26, 14)]),
        (4100, 6, False, [mirror(1)]),
        (4100, 6, False, [rot(90)]),
        (4100, 6, False, [crop(1, 4098, 0, 5)]),
        (2, 2, False, [rot(90), mirror(0)]),
        (48, 40, False, EIGHT_STEPS),
        NON_ADDITIVE,
    ]
    for w, h in ((33, 17), (127, 3), (1, 1)):
        out.append((w, h, True, [rot(270), resize(9, 31), mirror(0)]))
    out.append((48, 40, True, EIGHT_STEPS))
    return out


def generated_chains(count, seed=0x5EED):
    """1-5 effects from sizes 8..70; even k: monochrome of any size, odd k: YUV420 with every dimension even; crops inside the
    current image, resize targets in 4..80"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        mono = k % 2 == 0
        step = 1 if mono else 2

        def dim(lo, hi):   # a size in [lo, hi], even for YUV420
            v = int(rng.randint(lo, hi + 1))
            return v if mono else max(2, v & ~1)
        w, h = dim(8, 70), dim(8, 70)
        cw, ch, chain = w, h, []
        for _ in range(int(rng.randint(1, 6))):
            t = int(rng.randint(0, 4))
            if t == 0:
                ow, oh = dim(step, cw), dim(step, ch)
                l, tp = int(rng.randint(0, cw - ow + 1)), int(rng.randint(0, ch - oh + 1))
                chain.append(crop(l, l + ow - 1, tp, tp + oh - 1))
                cw, ch = ow, oh
            elif t == 1:
                chain.append(mirror(int(rng.randint(0, 2))))
            elif t == 2:
                deg = (90, 180, 270)[int(rng.randint(0, 3))]
                chain.append(rot(deg))
                if deg != 180:
                    cw, ch = ch, cw
            else:
                cw, ch = dim(4, 80), dim(4, 80)
                chain.append(resize(cw, ch))
        out.append((w, h, mono, chain))
    return out


def sizes(w, h, chain):
    """[(w, h)] of the input and every image after it"""
    out = [(w, h)]
    for t, a, b, c, d in chain:
        if t == 0:
            w, h = b - a + 1, d - c + 1
        elif t == 2 and a != 180:
            w, h = h, w
        elif t == 3:
            w, h = a, b
        out.append((w, h))
    return out


def packed(mono, w, h):
    return w * h if mono else w * h * 3 // 2


def has_odd(w, h, mono, chain):
    return (not mono) and any((x | y) & 1 for x, y in sizes(w, h, chain))


def source(w, h, mono, seed, ls=None, cs=None):
    """random planes, chroma right behind luma: (bytes, luma_stride, chroma_stride)"""
    ls = ls or w
    cs = cs or ls // 2
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, ls * h + (0 if mono else cs * h)).astype(np.uint8), ls, cs


def effect_array(mod, chain):
    arr = (mod.Effect * max(len(chain), 1))()
    for i, e in enumerate(chain):
        arr[i] = mod.Effect(*e)
    return arr


def oracle_run(orc, src, w, h, mono, chain, ls=0, cs=0, chroma=None, gamut=1):
    """-> (status, bytes, (w, h, gamut, format, luma_stride, chroma_stride), chroma offset or None)"""
    L = orc.load()
    extent = max(packed(mono, max(x, 1), max(y, 1)) for x, y in sizes(w, h, chain)) * 2 + 256
    buf = np.full(extent, 0xEE, np.uint8)
    img = orc.Image(src.ctypes.data, w, h, gamut, chroma.ctypes.data if chroma is not None else None, ls, cs,
                    orc.FMT_MONOCHROME if mono else orc.FMT_YUV420)
    o = orc.Image(buf.ctypes.data, 0, 0, -1, None, 0, 0, -1)
    rc = L.orc_add_effects(C.byref(img), effect_array(orc, chain), len(chain), C.byref(o))
    desc = (o.width, o.height, o.colorGamut, o.pixelFormat, o.luma_stride, o.chroma_stride)
    return rc, buf, desc, (o.chroma_data - o.data) if (chain and not mono and rc == 0) else None
