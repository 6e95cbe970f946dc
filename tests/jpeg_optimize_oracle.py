"""Pure-Python restatement of libjpeg's optimize_coding, for the tests of UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN.

    transcode(jpg)        a baseline file as libjpeg-turbo would have written it with optimize_coding = TRUE: the same coefficients,
                          Huffman tables built from the file's own symbol counts (jpeg_gen_optimal_table), one DHT segment per
                          table in the order DC0, AC0, DC1, AC1 in front of SOS, the same stuffing and ones-padding of the last byte
    optimal_table(freq)   the table rule alone: 256 counts -> (bits[16], vals)
    huffman_depth(freq)   the longest code the rule gives BEFORE it limits the lengths to 16
    dht_tables(jpg)       {(class, index): (bits, vals)} of a file
    fibonacci_image(n)    a one-plane image whose AC symbol counts at quality 50 are 1, 2, 3, 5, 8, ...: the merge is a chain

tests/test_jpeg_optimize_cpu.py pins transcode() to Pillow's libjpeg-turbo: transcode(save(optimize=False)) == save(optimize=True).
"""
import math

import numpy as np

NO_FREQ = 1000000000   # jchuff.c: "v = 1000000000L"
MAX_CLEN = 32


def _merge(freq):
    """jpeg_gen_optimal_table up to the code sizes: 256 counts -> codesize[257] (entry 256: the pseudo-symbol)"""
    f = [int(x) for x in freq] + [1]
    assert len(f) == 257
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, NO_FREQ
        for i in range(257):
            if f[i] and f[i] <= v:
                v, c1 = f[i], i
        c2, v = -1, NO_FREQ
        for i in range(257):
            if f[i] and f[i] <= v and i != c1:
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    return codesize


def huffman_depth(freq):
    return max(_merge(freq))


def optimal_table(freq):
    """-> (bits, vals): bits[l - 1] codes of length l (16 entries), vals the symbols by length, then value"""
    codesize = _merge(freq)
    assert max(codesize) <= MAX_CLEN, "libjpeg: JERR_HUFF_CLEN_OVERFLOW"
    bits = [0] * (MAX_CLEN + 1)
    for c in codesize:
        if c:
            bits[c] += 1
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for i in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == i]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def _codes(bits, vals):
    """T.81 Annex C: symbol -> (code, length)"""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[p]] = (code, l)
            code += 1
            p += 1
        code <<= 1
    return out


def _segments(jpg):
    """[(marker, offset of the 0xFF, offset behind the segment)] up to and including SOS"""
    assert jpg[:2] == b"\xff\xd8"
    segs, p = [], 2
    while True:
        assert jpg[p] == 0xFF, "marker expected at %d" % p
        m = jpg[p + 1]
        n = (jpg[p + 2] << 8) | jpg[p + 3]
        segs.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return segs


segments = _segments


def first_segment(jpg, marker):
    """offset of the first segment with this marker (walking the segments: a payload may hold the marker's two bytes)"""
    return next(a for m, a, b in _segments(jpg) if m == marker)


def dht_tables(jpg):
    out = {}
    for m, a, b in _segments(jpg):
        if m != 0xC4:
            continue
        p = a + 4
        while p < b:
            tc_th = jpg[p]
            bits = list(jpg[p + 1:p + 17])
            n = sum(bits)
            out[(tc_th >> 4, tc_th & 15)] = (bits, list(jpg[p + 17:p + 17 + n]))
            p += 17 + n
    return out


class _Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def bit(self):
        b = (self.buf[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, tab):
        first, count, start, vals = tab
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if code - first[l] < count[l] and code >= first[l]:
                return vals[start[l] + code - first[l]]
        raise ValueError("bad Huffman code")


def _decoder(bits, vals):
    first, count, start = [0] * 17, [0] * 17, [0] * 17
    code = p = 0
    for l in range(1, 17):
        first[l], count[l], start[l] = code, bits[l - 1], p
        code = (code + bits[l - 1]) << 1
        p += bits[l - 1]
    return first, count, start, vals


def symbols(jpg):
    """the file's entropy-coded segment as [(table class, table index, symbol, extra bits, their number)], and the header's segments"""
    segs = _segments(jpg)
    tabs = dht_tables(jpg)
    sof = [s for s in segs if s[0] == 0xC0]
    assert len(sof) == 1, "baseline files only"
    a = sof[0][1]
    h, w, nc = (jpg[a + 5] << 8) | jpg[a + 6], (jpg[a + 7] << 8) | jpg[a + 8], jpg[a + 9]
    comps = [(jpg[a + 10 + 3 * c], jpg[a + 11 + 3 * c] >> 4, jpg[a + 11 + 3 * c] & 15) for c in range(nc)]
    sa = segs[-1][1]
    ns = jpg[sa + 4]
    assert ns == nc
    sel = {jpg[sa + 5 + 2 * c]: (jpg[sa + 6 + 2 * c] >> 4, jpg[sa + 6 + 2 * c] & 15) for c in range(ns)}
    if nc == 1:   # a single-component scan is not interleaved: the blocks that cover the image, no dummies
        order = [sel[comps[0][0]]]
        nmcu = ((w + 7) // 8) * ((h + 7) // 8)
    else:
        hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
        order = [sel[cid] for cid, hs, vs in comps for _ in range(hs * vs)]
        nmcu = math.ceil(w / (8 * hmax)) * math.ceil(h / (8 * vmax))
    body = jpg[segs[-1][2]:]
    end = body.rfind(b"\xff\xd9")
    assert end >= 0 and end == len(body) - 2
    raw = body[:end].replace(b"\xff\x00", b"\xff")
    rd = _Reader(raw)
    dec = {k: _decoder(*v) for k, v in tabs.items()}
    out = []
    for _ in range(nmcu):
        for td, ta in order:
            s = rd.symbol(dec[(0, td)])
            out.append((0, td, s, rd.bits(s), s))
            k = 1
            while k < 64:
                s = rd.symbol(dec[(1, ta)])
                r, z = s >> 4, s & 15
                if z == 0:
                    out.append((1, ta, s, 0, 0))
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r + 1
                out.append((1, ta, s, rd.bits(z), z))
    assert rd.pos <= 8 * len(raw) and 8 * len(raw) - rd.pos < 8, "entropy-coded segment not consumed"
    return out, segs


def histograms(jpg):
    """{(class, index): 256 counts} of the file's symbols"""
    syms, _ = symbols(jpg)
    out = {}
    for cls, idx, s, _, _ in syms:
        out.setdefault((cls, idx), [0] * 256)[s] += 1
    return out


def transcode(jpg):
    jpg = bytes(jpg)
    syms, segs = symbols(jpg)
    hist = {}
    for cls, idx, s, _, _ in syms:
        hist.setdefault((cls, idx), [0] * 256)[s] += 1
    tables = {k: optimal_table(f) for k, f in hist.items()}
    codes = {k: _codes(*t) for k, t in tables.items()}
    first_dht = min(a for m, a, b in segs if m == 0xC4)
    out = bytearray(jpg[:first_dht])
    for m, a, b in segs:   # what is neither DHT nor SOS stands in front of the first DHT in every file this is written for
        assert m in (0xC4, 0xDA) or b <= first_dht
    for key in sorted(tables, key=lambda k: (k[1], k[0])):   # DC0, AC0, DC1, AC1
        bits, vals = tables[key]
        out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(key[0] << 4) | key[1]]) + bytes(bits) + bytes(vals)
    out += jpg[segs[-1][1]:segs[-1][2]]
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


# ---- the image whose AC table needs the length limit ------------------------------------------------------------------------------
_NATURAL = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25]   # zigzag positions 0 .. 11 in natural (row * 8 + column) order
_LUMA_Q50 = {1: 11, 8: 12, 16: 14, 9: 12, 2: 10, 3: 16, 10: 14, 17: 13, 24: 14, 32: 18, 25: 17}   # Annex K luminance table there


def fibonacci_counts(nsym):
    c = [1, 2]
    while len(c) < nsym:
        c.append(c[-1] + c[-2])
    return c[:nsym]


def fibonacci_symbols(nsym):
    """the AC symbols of fibonacci_image(nsym), rarest first: zigzag position 1 .. 11, size 1 (coefficient 1) or 2 (coefficient 3)"""
    assert nsym <= 22
    return [(((k // 2) << 4) | (1 + (k & 1))) for k in range(nsym)]


def fibonacci_image(nsym):
    """-> (pixels, width, height): every 8x8 block is 128 plus one DCT basis function whose coefficient quantises, at quality 50, to
    1 or 3 at zigzag position 1 .. 11; the number of blocks per (position, size) follows 1, 2, 3, 5, 8, ...  The other coefficients
    stay zero: the rounding of the pixels moves a coefficient by well under half the smallest quantiser step."""
    counts = fibonacci_counts(nsym)
    total = sum(counts)
    bw = int(math.ceil(math.sqrt(total)))
    bh = (total + bw - 1) // bw
    img = np.full((bh * 8, bw * 8), 128, np.uint8)
    x = np.arange(8)
    blk = 0
    for k, n in enumerate(counts):
        nat = _NATURAL[1 + k // 2]
        v, u = nat // 8, nat % 8
        coef = (1 if (k & 1) == 0 else 3) * _LUMA_Q50[nat]
        cu, cv = (1 / math.sqrt(2) if u == 0 else 1.0), (1 / math.sqrt(2) if v == 0 else 1.0)
        basis = 0.25 * cu * cv * coef * np.outer(np.cos((2 * x + 1) * v * math.pi / 16), np.cos((2 * x + 1) * u * math.pi / 16))
        tile = np.clip(np.rint(128 + basis), 0, 255).astype(np.uint8)
        for _ in range(n):
            r, c = divmod(blk, bw)
            img[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = tile
            blk += 1
    return img, bw * 8, bh * 8
