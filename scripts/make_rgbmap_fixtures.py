"""Writes tests/golden/rgbmap/: small RGB images and the 4:4:4 (and two 4:2:0) JPEGs libjpeg-turbo makes of them, through Pillow.

    python scripts/make_rgbmap_fixtures.py

Not run by the tests: the corpus is committed.  Pillow's `Image.save(..., "JPEG", quality=q, subsampling=0)` is libjpeg's file for
in_color_space = JCS_RGB with all sampling factors 1 -- baseline, jpeg_set_quality(q, TRUE), JDCT_ISLOW, default Huffman tables --
which is what uhdr_hip_jpeg_encode_rgb_batch has to write byte for byte.  The sizes: a single pixel, an exact block, a partial MCU
in each direction, an odd size of several MCUs, and one whose scan exceeds 16 KiB (more than one stuffing workgroup).

    rgb_<w>x<h>.npy            the image, (h, w, 3) uint8: flat blocks of random colour with noise on top
    rgb_<w>x<h>_q<q>.jpg       subsampling=0 at quality 85 and 95
    rgb_<w>x<h>_s2.jpg         45x37 and 264x200 only: subsampling=2 (4:2:0) at quality 85, a three-component map for the decode
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rgbmap")
SIZES = [(1, 1), (8, 8), (17, 9), (45, 37), (264, 200)]
QUALITIES = [85, 95]
WITH_420 = [(45, 37), (264, 200)]


def blocky_noise(w, h, seed, block=6, noise=24):
    """flat blocks of random colour with noise on top (as scripts/make_sampling_fixtures.py): the three planes differ everywhere"""
    rng = np.random.default_rng(seed)
    by, bx = (h + block - 1) // block, (w + block - 1) // block
    base = rng.integers(0, 256, (by, bx, 3)).astype(np.int32)
    img = np.repeat(np.repeat(base, block, axis=0), block, axis=1)[:h, :w]
    img = img + rng.integers(-noise, noise + 1, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for i, (w, h) in enumerate(SIZES):
        img = blocky_noise(w, h, 3000 + i)
        stem = os.path.join(OUT, "rgb_%dx%d" % (w, h))
        np.save(stem + ".npy", img)
        total += os.path.getsize(stem + ".npy")
        pil = Image.fromarray(img, "RGB")
        for q in QUALITIES:
            pil.save("%s_q%d.jpg" % (stem, q), "JPEG", quality=q, subsampling=0)
            total += os.path.getsize("%s_q%d.jpg" % (stem, q))
        if (w, h) in WITH_420:
            pil.save(stem + "_s2.jpg", "JPEG", quality=85, subsampling=2)
            total += os.path.getsize(stem + "_s2.jpg")
    print("%s: %d bytes" % (OUT, total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
