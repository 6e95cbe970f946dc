"""The images of the progressive-encode tests (tests/test_jpeg_progressive_encode_cpu.py states the counter each constructed one is
there for, tests/test_gpu_jpeg_progressive_encode.py sends them through the encoder): the smallest shapes at which the k_jpeg_prog_*
kernels can go wrong.  WG = 128 is the number of positions of a scan that one workgroup of those kernels handles."""
import math

import numpy as np

WG = 128
# 1x1; one block; 4:2:0 padding blocks across (24x8: 3 luma columns in 2 MCUs) and in both directions (40x24); partial blocks (17x9);
# 4:2:2 and 4:4:0 padding (17x8, 8x17); more than 128 blocks, more than one workgroup (136x136: 289)
SIZES = ((1, 1), (8, 8), (24, 8), (40, 24), (17, 9), (17, 8), (8, 17), (136, 136))
QUALITIES = (1, 50, 85, 100)
CONTENTS = ("noise", "ramp", "flat", "bw")
BIG = (136, 136)
BIG_COMBOS = (("noise", 85), ("noise", 1), ("flat", 50), ("bw", 100), ("ramp", 100))


def content(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "ramp":
        return ((np.indices(shape).sum(0) * 3) % 256).astype(np.uint8)
    if kind == "flat":
        return np.full(shape, 77, np.uint8)
    return (rng.integers(0, 2, shape) * 255).astype(np.uint8)


def combos(size):
    """(content, quality) pairs of one size: all sixteen, but five for the large one"""
    if tuple(size) == BIG:
        return BIG_COMBOS
    return tuple((c, q) for c in CONTENTS for q in QUALITIES)


def rotated(k):
    """four (content, quality) pairs, a different pairing for every k: what the sampled planes and the RGBA images run"""
    return tuple((CONTENTS[i], QUALITIES[(i + k) % 4]) for i in range(4))


# ---- one run longer than 0x7FFF blocks -------------------------------------------------------------------------------------------------
LONG_W, LONG_H = 2048, 1032          # 256 x 129 = 33 024 blocks, all flat: every AC scan is one run
LONG_BLOCKS = (LONG_W // 8) * (LONG_H // 8)


def long_run(textured_at=None):
    """the flat plane; textured_at: the position (raster order) of one block of noise, which codes symbols in every AC scan at quality
    50 -- at 32 766 the run in front of it is flushed one short of the limit, at 32 767 the limit flushes it and nothing is pending"""
    img = np.full((LONG_H, LONG_W), 128, np.uint8)
    if textured_at is not None:
        r, c = divmod(textured_at, LONG_W // 8)
        img[8 * r:8 * r + 8, 8 * c:8 * c + 8] = np.random.default_rng(7).integers(0, 256, (8, 8), dtype=np.uint8)
    return img


# ---- correction bits alone: the 937-bit rule ---------------------------------------------------------------------------------------------
_LUMA_Q50 = {1: 11, 8: 12, 16: 14, 9: 12, 2: 10}   # Annex K luminance quantisers at quality 50, by natural (row * 8 + column) index
CORR_PREFIX = 43            # flat blocks in front, which leave no bits
CORR_BITS = 2               # correction bits per block and refinement scan: coefficients 5 at zigzag 1 and 2
CORR_RUN = 937 // CORR_BITS + 1   # 469 blocks make 938 bits: the run is flushed behind its 469th block with bits
CORR_BW = 40                # 40 x 40 blocks


def _tile(coefs):
    """128 plus the DCT basis functions {natural index: quantised value} at quality 50 (tests/jpeg_optimize_oracle.fibonacci_image)"""
    x = np.arange(8)
    t = np.zeros((8, 8))
    for nat, val in coefs.items():
        v, u = divmod(nat, 8)
        cu, cv = (1 / math.sqrt(2) if u == 0 else 1.0), (1 / math.sqrt(2) if v == 0 else 1.0)
        t += 0.25 * cu * cv * val * _LUMA_Q50[nat] * np.outer(np.cos((2 * x + 1) * v * math.pi / 16), np.cos((2 * x + 1) * u * math.pi / 16))
    return np.clip(np.rint(128 + t), 0, 255).astype(np.uint8)


def corr_flushes():
    """the positions behind which the refinement scans of correction_bits() flush their run: 511 -- the last position of workgroup 3,
    the boundary --, then 980 and 1449, inside workgroups 7 and 11; the run 512 .. 980 spans workgroups 4 to 7"""
    out, e = [], CORR_PREFIX + CORR_RUN - 1
    while e < CORR_BW * CORR_BW:
        out.append(e)
        e += CORR_RUN
    return out


def correction_bits(new_behind_flush=False):
    """identical blocks whose two coefficients quantise to 5: coded at Al 2, one correction bit each in both refinement scans, never a
    new coefficient, so each refinement scan is one run that only the 937-bit rule cuts.  new_behind_flush: the block right behind the
    first forced flush also has a coefficient 1 and a coefficient 2 -- newly non-zero in the last and in the first refinement scan"""
    img = np.full((8 * CORR_BW, 8 * CORR_BW), 128, np.uint8)
    tile = _tile({1: 5, 8: 5})
    for p in range(CORR_PREFIX, CORR_BW * CORR_BW):
        r, c = divmod(p, CORR_BW)
        img[8 * r:8 * r + 8, 8 * c:8 * c + 8] = tile
    if new_behind_flush:
        r, c = divmod(corr_flushes()[0] + 1, CORR_BW)
        img[8 * r:8 * r + 8, 8 * c:8 * c + 8] = _tile({1: 5, 8: 5, 16: 1, 9: 2})
    return img


CORR_QUALITY = 50


# ---- refinement ZRLs, zeros behind the last new coefficient -------------------------------------------------------------------------------
def sparse_noise():
    """noise at quality 1: every quantiser is 255, the few coefficients that survive are small and far apart"""
    return content("noise", (64, 72), 11), 1


def constructed():
    """{name: (plane, quality, the counter of tests/jpeg_progressive_encode_oracle.py it is there for)}"""
    sp, q = sparse_noise()
    return {
        "long_run": (long_run(), 50, "eob_7fff"),
        "long_run_32766": (long_run(32766), 50, None),
        "long_run_32767": (long_run(32767), 50, "eob_7fff"),
        "correction_bits": (correction_bits(), CORR_QUALITY, "eob_corr"),
        "correction_bits_new": (correction_bits(True), CORR_QUALITY, "eob_corr"),
        "sparse_noise": (sp, q, "zrl_refine"),
    }
