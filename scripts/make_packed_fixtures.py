"""Writes tests/golden/packed/: small RGBA images and the 4:2:0 JPEGs libjpeg-turbo makes of their R, G, B, through Pillow.

    python scripts/make_packed_fixtures.py

Not run by the tests: the corpus is committed.  Pillow's `Image.save(..., "JPEG", quality=q, subsampling=2)` is libjpeg's file for
in_color_space = JCS_RGB with luma sampling 2x2 and chroma 1x1 -- baseline, jpeg_set_quality(q, TRUE), JDCT_ISLOW, default Huffman
tables, jccolor.c's conversion and jcsample.c's h2v2_downsample with libjpeg's edge padding -- which is what
uhdr_hip_jpeg_encode_rgba420_batch has to write byte for byte.  The sizes and qualities are tests/packed_cases.JPEG_CASES: a single
pixel, exactly one MCU, a width that is no multiple of 16, a partial MCU in both directions, an odd size in both directions, and
an all-noise image whose scan exceeds 16 KiB (more than one stuffing piece).  The generator is tests/packed_cases.jpeg_image;
tests/test_packed_cpu.py checks that it still reproduces the corpus.

    rgba_<w>x<h>.npy              the image, (h, w, 4) uint8 (alpha is noise: the encoder ignores it)
    rgba_<w>x<h>_q<q>_s2.jpg      subsampling=2 at quality q
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import packed_cases as P  # noqa: E402


def main():
    os.makedirs(P.DIR, exist_ok=True)
    total = 0
    for w, h, q in P.JPEG_CASES:
        img = P.jpeg_image(w, h)
        stem = os.path.join(P.DIR, "rgba_%dx%d" % (w, h))
        np.save(stem + ".npy", img)
        name = "%s_q%d_s2.jpg" % (stem, q)
        with open(name, "wb") as f:
            f.write(P.pillow_420(img, q))
        total += os.path.getsize(stem + ".npy") + os.path.getsize(name)
    print("%s: %d bytes" % (P.DIR, total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
