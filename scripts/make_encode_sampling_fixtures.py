"""Writes tests/golden/encode_sampling/: planes and the file IJG libjpeg writes for them in raw-data mode, 4:4:0 above all.

    python scripts/make_encode_sampling_fixtures.py [--prefix /opt/conda] [--libjpeg libjpeg.so.9.4.0]

Not run by the tests: the fixtures are committed.  Pillow cannot write 4:4:0, so the tests' expected 4:4:0 files come from a pure-Python
interleaver (tests/jpeg_sampling_encode_oracle.py); these few files pin it independently: a C helper
(scripts/encode_sampling_fixture_helper.c, built here with gcc against <prefix>/include/jpeglib.h and linked to the library by its
full file name) hands noise planes to jpeg_write_raw_data with 1x2 luma sampling, padded by replication.  One 4:2:2 and one 4:4:4 case
ride along.

    s<hs><vs>_<w>x<h>_q<quality>.npy    Y (w x h), Cb, Cr (ceil(w / hs) x ceil(h / vs)), packed: one uint8 array (numpy.save)
    s<hs><vs>_<w>x<h>_q<quality>.jpg    libjpeg's file
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_sampling_encode_cases as EC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", default="/opt/conda", help="where IJG libjpeg lives (include/jpeglib.h, lib/<libjpeg>)")
    ap.add_argument("--libjpeg", default="libjpeg.so.9.4.0", help="the library's file name under <prefix>/lib")
    args = ap.parse_args()
    os.makedirs(EC.GOLDEN, exist_ok=True)
    total = 0
    with tempfile.TemporaryDirectory() as tmp:
        helper = os.path.join(tmp, "encode_sampling_fixture_helper")
        lib = os.path.join(args.prefix, "lib")
        subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(args.prefix, "include"), os.path.join(ROOT, "scripts", "encode_sampling_fixture_helper.c"),
                               "-o", helper, os.path.join(lib, args.libjpeg), "-Wl,-rpath," + lib])
        for k, (w, h, hs, vs, q) in enumerate(EC.GOLDEN_CASES):
            y, cb, cr = EC.planes(w, h, hs, vs, 7000 + k)
            flat = np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
            stem = os.path.join(EC.GOLDEN, "s%d%d_%dx%d_q%d" % (hs, vs, w, h, q))
            raw = os.path.join(tmp, "in.ycc")
            flat.tofile(raw)
            subprocess.check_call([helper, raw, str(w), str(h), str(hs), str(vs), str(q), stem + ".jpg"])
            np.save(stem + ".npy", flat)
            total += os.path.getsize(stem + ".jpg") + os.path.getsize(stem + ".npy")
    print("%s: %d bytes" % (EC.GOLDEN, total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
