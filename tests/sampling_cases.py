"""The corpus of tests/golden/sampling/ (scripts/make_sampling_fixtures.py): names, geometry, files and libjpeg's planes."""
import functools
import os
import re

import numpy as np

from libultrahdr_dev_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "sampling")
SAMPLINGS = [(1, 1), (2, 1), (1, 2)]
FORMATS = {(1, 1): api.PIX_FMT_YUV444, (2, 1): api.PIX_FMT_YUV422, (1, 2): api.PIX_FMT_YUV440, (2, 2): api.PIX_FMT_YUV420}
SIZES = [(1, 1), (8, 8), (17, 9), (45, 37), (130, 70)]
FIXTURES = ["s%d%d_%s_%dx%d" % (hs, vs, v, w, h) for hs, vs in SAMPLINGS for v in ("base", "rst2", "prog") for w, h in SIZES] + \
           ["s%d%d_big_264x200" % s for s in SAMPLINGS]

# the metadata the assembled JPEG/R files carry (oracle/jpegr_oracle.append_gainmap's dictionary): boost 1 .. 10
JPEGR_MD = dict(version="1.0", max=np.float32(10.0), min=np.float32(1.0), gamma=np.float32(1.0), off_sdr=np.float32(0.0), off_hdr=np.float32(0.0),
                capmin=np.float32(1.0), capmax=np.float32(10.0))


def chroma_size(hs, vs, w, h):
    """libjpeg's downsampled_width / height of a 1x1 component under hs x vs luma"""
    return (w + hs - 1) // hs, (h + vs - 1) // vs


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(hs, vs, w, h, file bytes, planes as one uint8 array: Y, Cb, Cr packed)"""
    m = re.match(r"s(\d)(\d)_[a-z0-9]+_(\d+)x(\d+)$", name)
    hs, vs, w, h = (int(g) for g in m.groups())
    data = open(os.path.join(DIR, name + ".jpg"), "rb").read()
    planes = np.load(os.path.join(DIR, name + ".npy"))
    planes.setflags(write=False)
    return hs, vs, w, h, data, planes


def upsampled_rgb(hs, vs, w, h, planes):
    """libjpeg-turbo's RGB of the planes: "fancy" h2v1 / h1v2 upsampling (jdsample.c), then jdcolor.c's fixed-point conversion"""
    cw, ch = chroma_size(hs, vs, w, h)
    y = planes[:w * h].reshape(h, w).astype(np.int32)
    out = []
    for k in range(2):
        c = planes[w * h + k * cw * ch:w * h + (k + 1) * cw * ch].reshape(ch, cw).astype(np.int32)
        if hs == 2:
            if cw > 2:
                left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
                right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
                even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
                even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
            else:
                even = odd = c
            c = np.stack([even, odd], axis=2).reshape(ch, 2 * cw)[:, :w]
        elif vs == 2:
            up = np.concatenate([c[:1], c[:-1]], axis=0)
            down = np.concatenate([c[1:], c[-1:]], axis=0)
            c = np.stack([(3 * c + up + 1) >> 2, (3 * c + down + 2) >> 2], axis=1).reshape(2 * ch, cw)[:h]
        out.append(c - 128)
    cb, cr = out
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
