"""The batches of tests/test_gpu_tone_runs.py (not a test file): layouts that walk the run and slot bookkeeping of the tone-map and
convertYuv batch calls, their contents, the models' answers, and the runs a layout is meant to take.

A run is what the C layer forms from image i on: up to CAP = 32 consecutive images of image i's size (the planar operator: and
gamut) and one alignment class, which share a launch.  An image's headroom slot is its index in the call, whatever run it is in;
pass 1 of the two operators launches over a run's MEASURED members alone, with their slots compacted to the front.

Images are tiny (a few seconds per test on the device): planar 16 x 8 for the aligned class (width % 16 == 0) and 18 x 6 with ragged
strides for the other; packed 8 x 4 (width % 4 == 0, rows on 16 bytes) and 10 x 4 with ragged strides.  Every image carries its own
brightest pixel, at a position and with a code that vary with its index, so every measured H differs from every other and lies
strictly between 1 and k (tests/test_tone_runs_cpu.py asserts it): a slot or descriptor mix-up shows as a wrong H.
"""
import functools

import numpy as np

from tests import packed_tonemap_cases as K
from tests import tonemap_cases as T

F = np.float32
CAP, HEAD_CAP = 32, 512          # kToneChunk, kToneHeadChunk
N_LAYOUT, N_MANY = 41, 515


class Img:
    """one image of a layout.  aligned: the class its layout is meant to take (the GPU test checks the pointers it really got);
    off: bytes that push the destination (and the source) off its natural alignment; content: index into the contents"""

    def __init__(self, w, h, gamut, aligned, given, content, off=0, strides=None):
        self.w, self.h, self.gamut, self.aligned, self.given, self.content, self.off, self.strides = w, h, gamut, aligned, given, content, off, strides

    def shape(self, by_gamut):
        return (self.w, self.h, self.gamut if by_gamut else None)


def layout(packed):
    """the 41 images: 34 of the aligned size and one gamut (a run of 32, a run of 2); 1 of that size whose destination sits at an odd
    address (a class break inside the size run); 2 of that size, aligned again, with GIVEN peaks (planar: in another gamut, a gamut
    break) -- pass 1 launches nothing for their run; 3 ragged ones (the other class); 1 of the first shape again.  Peaks are given
    for every image with i % 3 == 1, and for images 35 and 36: every other H is measured, so the measured members of every run
    are a sparse subset."""
    w, h = (8, 4) if packed else (16, 8)
    rw, rh = (10, 4) if packed else (18, 6)
    rs = (11, 13) if packed else (21, 20, 23, 11)      # packed: source, destination; planar: luma, chroma, destination luma, chroma
    g0, g1 = (T.CG_2100, T.CG_2100) if packed else (T.CG_2100, T.CG_709)
    out = []
    for i in range(N_LAYOUT):
        given = i % 3 == 1 or i in (35, 36)
        if i < 34 or i == 40:
            out.append(Img(w, h, g0, True, given, i))
        elif i == 34:
            out.append(Img(w, h, g0, False, given, i, off=(4 if packed else 2)))
        elif i < 37:
            out.append(Img(w, h, g1, True, given, i))
        else:
            out.append(Img(rw, rh, g0, False, given, i, off=(4 if packed else 0), strides=rs))
    return out


LAYOUT_RUNS = [(0, 32), (32, 2), (34, 1), (35, 2), (37, 3), (40, 1)]      # (first image, members): what layout() is meant to give


def many(packed):
    """515 images of the aligned size: three more slots than one head chunk.  Contents cycle with period 7, given peaks with period
    3, so a shift by 32 or by 512 slots lands on another expected value; slots 512 and 513 are measured, slot 514 is given."""
    w, h = (8, 4) if packed else (16, 8)
    return [Img(w, h, T.CG_2100, True, i % 3 == 1, i % 7) for i in range(N_MANY)]


def runs(images, by_gamut, cap=CAP):
    """[(first image, members)] by the rule of the module's docstring"""
    out, i = [], 0
    while i < len(images):
        m = 1
        while i + m < len(images) and m < cap and images[i + m].shape(by_gamut) == images[i].shape(by_gamut) and images[i + m].aligned == images[i].aligned:
            m += 1
        out.append((i, m))
        i += m
    return out


def peak_of(img):
    """the given peak in nits (0: measured): its own for every content, H between 1.2 and 4.2 -- below every transfer function's cap"""
    return 250.0 + 15.0 * img.content if img.given else 0.0


def peaks(images, null=False):
    return None if null else [peak_of(im) for im in images]


# ------------------------------------------------------------------ planar contents and answers
# the code of content c's brightest pixel: high enough for H > 1 (HLG: its inverse OETF times k passes 1 only above code 750 or so),
# low enough for H < k, its own for every content
BRIGHT = {T.TF_HLG: (760, 4), T.TF_PQ: (600, 8), T.TF_LINEAR: (560, 8)}


@functools.lru_cache(maxsize=None)
def planar_planes(w, h, content, tf):
    l, c = (a.copy() for a in T.ramp_planes(w, h, swing=60.0, top=300.0))
    base, step = BRIGHT[tf]
    T.set_pixel(l, c, (5 * content + 3) % w, (3 * content + 1) % h, base + step * content)
    for a in (l, c):
        a.setflags(write=False)
    return l, c


@functools.lru_cache(maxsize=None)
def _planar_expected(w, h, content, gamut, tf, peak):
    return T.model(*planar_planes(w, h, content, tf), gamut, tf, peak)


def planar_expected(img, tf, measured=False):
    """the model's answer for an image of a layout (measured: the call passes hdr_peak_nits == NULL): computed once, shared"""
    return _planar_expected(img.w, img.h, img.content, img.gamut, tf, 0.0 if measured else peak_of(img))


# ------------------------------------------------------------------ packed contents and answers
# per form: (first code or value of the brightest channel, step per content)
PACKED_BRIGHT = {(K.FMT_1010102, K.TF_PQ): (620, 9), (K.FMT_1010102, K.TF_HLG): (810, 5), (K.FMT_F16, K.TF_LINEAR): (0.25, 0.0175)}


@functools.lru_cache(maxsize=None)
def packed_image(form, w, h, content):
    """a dim ramp (R along x, G along y, B along the diagonal, up to 0.3 of the signal range; F16: 0.18, so that the ramp alone stays
    below H = 1) and one brighter channel of one pixel"""
    fmt, tf = form
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    t = np.stack([x / max(w - 1, 1), y / max(h - 1, 1), (x + y) / max(w + h - 2, 1)], axis=2) * 0.3
    px, py, ch = (5 * content + 3) % w, (3 * content + 1) % h, content % 3
    base, step = PACKED_BRIGHT[form]
    if fmt == K.FMT_F16:
        img = np.zeros((h, w, 4), np.uint16)
        img[:, :, :3] = (t * 0.6).astype(np.float16).view(np.uint16)
        img[:, :, 3] = 0x3C00
        img[py, px, ch] = np.array([base + step * content], np.float16).view(np.uint16)[0]
    else:
        c = np.round(t * 1023).astype(np.uint32)
        c[py, px, ch] = base + step * content
        img = (c[:, :, 0] | (c[:, :, 1] << 10) | (c[:, :, 2] << 20) | ((x.astype(np.uint32) & 3) << 30)).astype(np.uint32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _packed_expected(form, w, h, content, peak):
    return K.model(packed_image(form, w, h, content), form[0], form[1], peak)


def packed_expected(img, form, measured=False):
    return _packed_expected(form, img.w, img.h, img.content, 0.0 if measured else peak_of(img))


def pooled_doubt(wants, keys):
    """the share of samples in doubt over all planes of all images of one batch"""
    tot = sum(w[k].size for w in wants for k in keys)
    return sum(int(T.in_doubt(w[k]).sum()) for w in wants for k in keys) / tot
