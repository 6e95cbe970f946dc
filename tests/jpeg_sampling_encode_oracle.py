"""Pure-Python interleaver for the tests of the encoder's 4:4:4 / 4:2:2 / 4:4:0 files (uhdr_hip_jpeg_encode_planes_batch_opts).

    encode_planes(y, cb, cr, hs, vs, quality, icc=None)
                          the baseline file libjpeg writes in raw-data mode for three planes with hs x vs luma sampling over 1x1
                          chroma (chroma: ceil(w / hs) x ceil(h / vs)), jpeg_set_quality(quality, TRUE), ISLOW, default tables.
                          Each plane's quantised blocks come from a Pillow single-plane ("L") file -- libjpeg's own FDCT, quantiser
                          and edge expansion (last column out to the block grid, then the last row) on that plane --, read with
                          tests/jpeg_restart_oracle.py's reader and emitted again in the MCU order of (hs, vs): hs * vs luma blocks in
                          rows of hs, then Cb, Cr; a luma block past the component's size in blocks is a dummy (zero AC, the DC of the
                          block before it in the MCU); the DC differences are formed again per component.
    pillow_ycbcr(y, cb, cr, hs, vs, quality, **kw)
                          Pillow's direct file for the same planes, for (1,1), (2,1), (2,2): a mode-YCbCr image (no colour conversion)
                          whose chroma is the planes' samples repeated hs x vs and cropped -- the downsampler's average of equal
                          samples is the sample, for either bias, and the edge expansion of the repeated image is the replicate
                          padding of the plane.  tests/test_jpeg_sampling_encode_cpu.py pins encode_planes to it.

Optimised tables and restart intervals come on top with tests/jpeg_restart_oracle.transcode_restart, which follows any geometry.
"""
import functools
import io

import numpy as np

from tests import jpeg_optimize_oracle as JO
from tests import jpeg_restart_oracle as RO

# ITU-T T.81 Annex K, table K.2 (chrominance), natural order
_STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
_SUBSAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}


def chroma_table(quality):
    """jpeg_set_quality(quality, TRUE) of table K.2, natural order"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((v * scale + 50) // 100, 1), 255) for v in _STD_CHROMA]


def _save(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def _plane_file(plane, quality, chroma):
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(plane), "L")
    if not chroma:
        return _save(im, quality=quality)
    return _save(im, qtables=[chroma_table(quality)])


def _plane_blocks(plane, quality, chroma):
    """-> (blocks wide, blocks high, [(DC value, AC symbols)] in raster order, the file's DQT payload without the table index)"""
    jpg = _plane_file(plane, quality, chroma)
    h, w = plane.shape
    bw, bh = (w + 7) // 8, (h + 7) // 8
    blocks = RO._blocks(jpg)
    assert len(blocks) == bw * bh
    dc, out = 0, []
    for diff, ac in blocks:
        dc += diff
        out.append((dc, ac))
    a = JO.first_segment(jpg, 0xDB)
    assert jpg[a + 2:a + 5] == b"\x00\x43\x00"
    return bw, bh, out, jpg[a + 5:a + 69]


@functools.lru_cache(maxsize=1)
def _default_dht():
    """the four Annex K tables as libjpeg writes them: one DHT segment each, DC0 AC0 DC1 AC1"""
    from PIL import Image
    jpg = _save(Image.new("RGB", (8, 8)), quality=90)
    segs = [jpg[a:b] for m, a, b in JO.segments(jpg) if m == 0xC4]
    assert len(segs) == 4 and [s[4] for s in segs] == [0x00, 0x10, 0x01, 0x11]
    return b"".join(segs)


def encode_planes(y, cb, cr, hs, vs, quality, icc=None):
    h, w = y.shape
    cw, ch = (w + hs - 1) // hs, (h + vs - 1) // vs
    assert cb.shape == (ch, cw) and cr.shape == (ch, cw) and hs in (1, 2) and vs in (1, 2)
    ybw, ybh, yblk, ydqt = _plane_blocks(y, quality, False)
    cbw, cbh, cbblk, cdqt = _plane_blocks(cb, quality, True)
    _, _, crblk, cdqt2 = _plane_blocks(cr, quality, True)
    assert cdqt == cdqt2 == bytes(chroma_table(quality)[n] for n in _zigzag())
    mcus_x, mcus_y = (w + 8 * hs - 1) // (8 * hs), (h + 8 * vs - 1) // (8 * vs)
    assert (cbw, cbh) == (mcus_x, mcus_y)      # a 1x1 component has no dummy blocks
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if icc:
        out += b"\xff\xe2" + (len(icc) + 2).to_bytes(2, "big") + bytes(icc)
    out += b"\xff\xdb\x00\x43\x00" + ydqt + b"\xff\xdb\x00\x43\x01" + cdqt
    out += b"\xff\xc0\x00\x11\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03" + bytes([1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    out += _default_dht()
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    codes = {k: JO._codes(*t) for k, t in JO.dht_tables(bytes(out)).items()}
    last = [0, 0, 0]
    syms = []

    def emit(comp, dc, ac):
        n, extra = RO._dc_symbol(dc - last[comp])
        last[comp] = dc
        t = 0 if comp == 0 else 1
        syms.append((0, t, n, extra, n))
        syms.extend((1, t, s, e, z) for s, e, z in ac)

    for mr in range(mcus_y):
        for mc in range(mcus_x):
            prev = None
            for r in range(vs):
                for c in range(hs):
                    br, bc = vs * mr + r, hs * mc + c
                    if br < ybh and bc < ybw:
                        prev = yblk[br * ybw + bc]
                        emit(0, *prev)
                    else:                      # jccoefct.c: a dummy block -- zero AC, the DC of the block before it in the MCU
                        emit(0, prev[0], [(0, 0, 0)])
            emit(1, *cbblk[mr * cbw + mc])
            emit(2, *crblk[mr * cbw + mc])
    acc = nacc = 0
    body = bytearray()
    for cls, idx, s, extra, n in syms:
        code, l = codes[(cls, idx)][s]
        acc = (acc << (l + n)) | (code << n) | extra
        nacc += l + n
        while nacc >= 8:
            by = (acc >> (nacc - 8)) & 0xFF
            body.append(by)
            if by == 0xFF:
                body.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1
    if nacc:
        by = ((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF
        body.append(by)
        if by == 0xFF:
            body.append(0)
    return bytes(out + body + b"\xff\xd9")


def _zigzag():
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, (n // 8) if (n // 8 + n % 8) % 2 else (n % 8)))
    return order


def repeated(c, hs, vs, w, h):
    """the chroma plane's samples each repeated hs x vs, cropped to w x h"""
    return np.repeat(np.repeat(c, vs, axis=0), hs, axis=1)[:h, :w]


def pillow_ycbcr(y, cb, cr, hs, vs, quality, **kw):
    from PIL import Image
    h, w = y.shape
    arr = np.stack([y, repeated(cb, hs, vs, w, h), repeated(cr, hs, vs, w, h)], axis=2)
    return _save(Image.fromarray(np.ascontiguousarray(arr), "YCbCr"), quality=quality, subsampling=_SUBSAMPLING[(hs, vs)], **kw)


def dummy_blocks(jpg):
    """[(index in scan order, DC value, DC value of the block before it, AC symbols)] of the luma blocks of a file that lie past the
    component's size in blocks"""
    jpg = bytes(jpg)
    a = next(a for m, a, b in JO.segments(jpg) if m == 0xC0)
    h, w = (jpg[a + 5] << 8) | jpg[a + 6], (jpg[a + 7] << 8) | jpg[a + 8]
    hs, vs = jpg[a + 11] >> 4, jpg[a + 11] & 15
    per_row, nmcu, order, which = RO.geometry(jpg)
    blocks = RO._blocks(jpg)
    bpm, ybw, ybh = len(order), (w + 7) // 8, (h + 7) // 8
    out, dc = [], 0
    for i, (diff, ac) in enumerate(blocks):
        k = i % bpm
        if which[k] != 0:
            continue
        before, dc = dc, dc + diff
        mr, mc = divmod(i // bpm, per_row)
        br, bc = vs * mr + k // hs, hs * mc + k % hs
        if not (br < ybh and bc < ybw):
            out.append((i, dc, before, ac))
    return out
