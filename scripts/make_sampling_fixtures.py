"""Writes tests/golden/sampling/: small 4:4:4, 4:2:2 and 4:4:0 JPEGs with the planes IJG libjpeg's raw_data_out returns for them.

    python scripts/make_sampling_fixtures.py [--prefix /opt/conda]

Not run by the tests: the corpus is committed.  Pillow cannot write 4:4:0 and cannot return raw subsampled planes, so a C helper
(scripts/sampling_fixture_helper.c, built here with gcc against <prefix>/include/jpeglib.h) does both.  Per sampling: a baseline
file, one with a restart interval of 2 MCUs and a progressive one at each of SIZES (a partial MCU in each direction, odd sizes, a
number of MCUs per row that is no power of two), quality 90, blocks of flat colour plus noise; and one 264x200 quality-95 noise
file whose entropy-coded segment exceeds 16 KiB, so that its decode crosses a workgroup of 256 subsequences.

    s<hs><vs>_<variant>_<w>x<h>.jpg    the file
    s<hs><vs>_<variant>_<w>x<h>.npy    Y (w x h), Cb, Cr (ceil(w / hs) x ceil(h / vs)), packed: one uint8 array (numpy.save)
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sampling")
SAMPLINGS = [(1, 1), (2, 1), (1, 2)]
VARIANTS = ["base", "rst2", "prog"]
SIZES = [(1, 1), (8, 8), (17, 9), (45, 37), (130, 70)]
BIG = (264, 200)


def blocky_noise(w, h, seed, block=6, noise=24):
    """flat blocks of random colour with noise on top: every block of the JPEG has its own DC and some AC"""
    rng = np.random.default_rng(seed)
    by, bx = (h + block - 1) // block, (w + block - 1) // block
    base = rng.integers(0, 256, (by, bx, 3)).astype(np.int32)
    img = np.repeat(np.repeat(base, block, axis=0), block, axis=1)[:h, :w]
    img = img + rng.integers(-noise, noise + 1, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", default="/opt/conda", help="where IJG libjpeg lives (include/jpeglib.h, lib/libjpeg.so)")
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        helper = os.path.join(tmp, "sampling_fixture_helper")
        lib = os.path.join(args.prefix, "lib")
        subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(args.prefix, "include"), os.path.join(ROOT, "scripts", "sampling_fixture_helper.c"),
                               "-o", helper, "-L" + lib, "-ljpeg", "-Wl,-rpath," + lib])
        rgb_path = os.path.join(tmp, "in.rgb")

        def one(img, hs, vs, quality, variant, name):
            h, w = img.shape[:2]
            img.tofile(rgb_path)
            stem = os.path.join(OUT, "s%d%d_%s_%dx%d" % (hs, vs, name, w, h))
            ycc_path = os.path.join(tmp, "out.ycc")
            subprocess.check_call([helper, rgb_path, str(w), str(h), str(hs), str(vs), str(quality), str(variant), stem + ".jpg", ycc_path])
            np.save(stem + ".npy", np.fromfile(ycc_path, np.uint8))
            return os.path.getsize(stem + ".jpg") + os.path.getsize(stem + ".npy")

        total = 0
        for si, (hs, vs) in enumerate(SAMPLINGS):
            for vi, name in enumerate(VARIANTS):
                for zi, (w, h) in enumerate(SIZES):
                    total += one(blocky_noise(w, h, 1000 + 100 * si + 10 * vi + zi), hs, vs, 90, vi, name)
            total += one(noise(BIG[0], BIG[1], 2000 + si), hs, vs, 95, 0, "big")
    print("%s: %d bytes" % (OUT, total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
