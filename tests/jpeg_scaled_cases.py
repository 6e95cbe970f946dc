"""Files and Pillow expectations shared by tests/test_jpeg_scaled_cpu.py and tests/test_gpu_jpeg_scaled.py."""
import functools
import io

import numpy as np

DENOMS = (2, 4, 8)
SIZES = [(8, 8), (16, 16), (17, 9), (18, 34), (33, 17), (37, 29), (130, 66)]


def content(w, h, seed):
    """flat blocks of colour plus noise"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 5) // 6, (w + 5) // 6, 3))
    img = np.repeat(np.repeat(base, 6, axis=0), 6, axis=1)[:h, :w] + rng.integers(-24, 25, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pillow(w, h, seed, gray, kw):
    from PIL import Image
    b = io.BytesIO()
    img = content(w, h, seed)
    Image.fromarray(img[:, :, 0] if gray else img).save(b, "JPEG", **dict(kw))
    return b.getvalue()


def pillow_jpeg(w, h, seed, **kw):
    kw.setdefault("quality", 90)
    return _pillow(w, h, seed, False, tuple(sorted(kw.items())))


def gray_jpeg(w, h, seed, **kw):
    kw.setdefault("quality", 90)
    return _pillow(w, h, seed, True, tuple(sorted(kw.items())))


def pillow_scaled(data, mode, w, h, s):
    """Pillow's (libjpeg-turbo's) decode of `data` at 1/s: the draft is requested with (w // s, h // s) and must come out
    ceil(w / s) x ceil(h / s).  mode 'L' / 'YCbCr': the samples as decoded; 'RGB': upsampled and converted"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if s != 1:
        im.draft(mode, (max(w // s, 1), max(h // s, 1)))
    elif mode == "YCbCr":
        im.draft(mode, (w, h))
    assert im.size == (-(-w // s), -(-h // s)), (im.size, w, h, s)
    if im.mode != mode:
        assert mode == "RGB" or (mode == "L" and im.mode == "L"), (im.mode, mode)
        im = im.convert(mode)
    return np.asarray(im)


def pillow_scaled_rgba(data, w, h, s):
    rgb = pillow_scaled(data, "RGB", w, h, s)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2).reshape(-1)


JPEGR_MD = dict(version="1.0", max=np.float32(10.0), min=np.float32(1.0), gamma=np.float32(1.0), off_sdr=np.float32(0.0), off_hdr=np.float32(0.0),
                capmin=np.float32(1.0), capmax=np.float32(10.0))


@functools.lru_cache(maxsize=None)
def jpegr_file(w, h, factor):
    """a JPEG/R container of a Pillow 4:2:0 primary and a one-plane map of (w / factor) x (h / factor), assembled on the CPU"""
    from oracle import jpegr_oracle as J
    assert w % factor == 0 and h % factor == 0
    data = J.append_gainmap(pillow_jpeg(w, h, 21, subsampling=2), gray_jpeg(w // factor, h // factor, 22, quality=85), JPEGR_MD)
    assert isinstance(data, bytes)
    return data
