"""Pure-Python restatement of libjpeg's progressive writer (jcphuff.c, jpeg_simple_progression), for the tests of
UHDR_HIP_SCANS_PROGRESSIVE.

    transcode_progressive(jpg)   a baseline file -> (the SOF2 file libjpeg-turbo writes over the same quantised coefficients, counters):
                                 SOI, APPn and DQT as they stand, SOF2, then per scan its DHT segment(s) -- tables built from the
                                 scan's own symbols by jpeg_optimize_oracle.optimal_table --, SOS and the stuffed, ones-padded
                                 entropy-coded segment; EOI
    coefficients(jpg)            the baseline file's quantised coefficients, per component a [rows][columns][64] grid (zigzag order)
                                 over the MCU-padded block grid
    scan_script(ncomp)           [(component indices, Ss, Se, Ah, Al)]

counters: eob_7fff (runs flushed because they reached 0x7FFF), eob_corr (runs flushed because more than 937 correction bits were
pending), zrl_first, zrl_refine, padding_skipped (blocks of the MCU padding that the non-interleaved scans leave out).

tests/test_jpeg_progressive_encode_cpu.py pins it to Pillow's libjpeg-turbo: transcode_progressive(save(progressive=False)) ==
save(progressive=True).
"""
import math

from tests.jpeg_optimize_oracle import _codes, optimal_table, symbols

MAX_CORR_BITS = 1000
DCTSIZE2 = 64


def scan_script(ncomp):
    if ncomp == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
            ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def _frame(jpg, segs):
    a = next(s for s in segs if s[0] == 0xC0)[1]
    h, w, nc = (jpg[a + 5] << 8) | jpg[a + 6], (jpg[a + 7] << 8) | jpg[a + 8], jpg[a + 9]
    comps = [(jpg[a + 10 + 3 * c], jpg[a + 11 + 3 * c] >> 4, jpg[a + 11 + 3 * c] & 15) for c in range(nc)]
    return w, h, comps


def coefficients(jpg):
    """-> (w, h, comps, grids, mcus_x, mcus_y): grids[c][row][column] = 64 coefficients in zigzag order"""
    jpg = bytes(jpg)
    syms, segs = symbols(jpg)
    w, h, comps = _frame(jpg, segs)
    nc = len(comps)
    blocks, cur = [], None
    for cls, idx, s, extra, n in syms:
        if cls == 0:
            cur = [0] * 64
            blocks.append(cur)
            cur[0] = extra if (n == 0 or extra >> (n - 1)) else extra - (1 << n) + 1   # (the difference, for now)
            k = 1
            continue
        r, z = s >> 4, s & 15
        if z == 0:
            k = k + 16 if r == 15 else 64
            continue
        k += r
        cur[k] = extra if extra >> (z - 1) else extra - (1 << z) + 1
        k += 1
    if nc == 1:
        bw, bh = (w + 7) // 8, (h + 7) // 8
        assert len(blocks) == bw * bh
        pred = 0
        for b in blocks:
            b[0] += pred
            pred = b[0]
        return w, h, comps, [[blocks[r * bw:(r + 1) * bw] for r in range(bh)]], bw, bh
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = math.ceil(w / (8 * hmax)), math.ceil(h / (8 * vmax))
    grids = [[[None] * (mx * hs) for _ in range(my * vs)] for _, hs, vs in comps]
    it = iter(blocks)
    pred = [0] * nc
    for m in range(mx * my):
        mr, mc = divmod(m, mx)
        for c, (_, hs, vs) in enumerate(comps):
            for y in range(vs):
                for x in range(hs):
                    b = next(it)
                    b[0] += pred[c]
                    pred[c] = b[0]
                    grids[c][mr * vs + y][mc * hs + x] = b
    return w, h, comps, grids, mx, my


class _Scan:
    """one scan's symbols: [(table key or None, symbol, extra bits, their number)]; a None key is raw bits"""

    def __init__(self, counters):
        self.out = []
        self.c = counters
        self.eobrun = 0
        self.be = []          # pending correction bits of the run

    def sym(self, key, s, extra=0, n=0):
        self.out.append((key, s, extra, n))

    def raw(self, bits):
        for b in bits:
            self.out.append((None, 0, b, 1))

    def emit_eobrun(self, key):
        if self.eobrun > 0:
            nb = self.eobrun.bit_length() - 1
            self.sym(key, nb << 4, self.eobrun & ((1 << nb) - 1), nb)
            self.eobrun = 0
            self.raw(self.be)
            self.be = []


def _ac_first(sc, key, blk, ss, se, al):
    if not any(blk[ss:se + 1]):   # (a flat block: what the loop below comes to, for the images of 33 024 such blocks)
        sc.eobrun += 1
        if sc.eobrun == 0x7FFF:
            sc.c["eob_7fff"] += 1
            sc.emit_eobrun(key)
        return
    r = 0
    for k in range(ss, se + 1):
        t = blk[k]
        if t == 0:
            r += 1
            continue
        if t < 0:
            t = (-t) >> al
            t2 = ~t
        else:
            t >>= al
            t2 = t
        if t == 0:
            r += 1
            continue
        sc.emit_eobrun(key)
        while r > 15:
            sc.sym(key, 0xF0)
            sc.c["zrl_first"] += 1
            r -= 16
        nb = t.bit_length()
        sc.sym(key, (r << 4) + nb, t2 & ((1 << nb) - 1), nb)
        r = 0
    if r > 0:
        sc.eobrun += 1
        if sc.eobrun == 0x7FFF:
            sc.c["eob_7fff"] += 1
            sc.emit_eobrun(key)


def _ac_refine(sc, key, blk, ss, se, al):
    if not any(blk[ss:se + 1]):
        return _ac_first(sc, key, blk, ss, se, al)
    absv = {k: abs(blk[k]) >> al for k in range(ss, se + 1)}
    eob = 0
    for k in range(ss, se + 1):
        if absv[k] == 1:
            eob = k
    r, br = 0, []
    for k in range(ss, se + 1):
        t = absv[k]
        if t == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            sc.emit_eobrun(key)
            sc.sym(key, 0xF0)
            sc.c["zrl_refine"] += 1
            r -= 16
            sc.raw(br)
            br = []
        if t > 1:
            br.append(t & 1)
            continue
        sc.emit_eobrun(key)
        sc.sym(key, (r << 4) + 1, 0 if blk[k] < 0 else 1, 1)
        sc.raw(br)
        br = []
        r = 0
    if r > 0 or br:
        sc.eobrun += 1
        sc.be += br
        if sc.eobrun == 0x7FFF or len(sc.be) > MAX_CORR_BITS - DCTSIZE2 + 1:
            sc.c["eob_7fff" if sc.eobrun == 0x7FFF else "eob_corr"] += 1
            sc.emit_eobrun(key)


def _stuffed(items, codes):
    acc = nacc = 0
    body = bytearray()
    for key, s, extra, n in items:
        if key is None:
            code, l = 0, 0
        else:
            code, l = codes[key][s]
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
    return body


def transcode_progressive(jpg):
    jpg = bytes(jpg)
    w, h, comps, grids, mx, my = coefficients(jpg)
    _, segs = symbols(jpg)
    nc = len(comps)
    counters = {"eob_7fff": 0, "eob_corr": 0, "zrl_first": 0, "zrl_refine": 0, "padding_skipped": 0}
    sof = next(s for s in segs if s[0] == 0xC0)
    for m, a, b in segs:   # SOI, APPn, DQT, SOF0, then the tables and SOS: what these tests write
        assert m in (0xC4, 0xDA) or b <= sof[2]
    out = bytearray(jpg[:sof[2]])
    out[sof[1] + 1] = 0xC2
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    for cs, ss, se, ah, al in scan_script(nc):
        sc = _Scan(counters)
        if ss == 0:   # DC: interleaved when the scan has more than one component, over whole MCUs
            order = []
            if len(cs) == 1:
                order = [(0, r, c) for r in range(len(grids[0])) for c in range(len(grids[0][0]))]
            else:
                for m in range(mx * my):
                    mr, mc = divmod(m, mx)
                    for c in cs:
                        _, hs, vs = comps[c]
                        order += [(c, mr * vs + y, mc * hs + x) for y in range(vs) for x in range(hs)]
            pred = [0] * nc
            for c, r, col in order:
                v = grids[c][r][col][0]
                if ah:
                    sc.raw([(v >> al) & 1])
                    continue
                t2 = v >> al
                t = t2 - pred[c]
                pred[c] = t2
                t2 = t
                if t < 0:
                    t = -t
                    t2 -= 1
                nb = t.bit_length()
                sc.sym((0, 0 if c == 0 else 1), nb, t2 & ((1 << nb) - 1), nb)
        else:        # AC: one component, its own block grid in raster order
            c = cs[0]
            _, hs, vs = comps[c]
            wc, hc = math.ceil(w * hs / hmax), math.ceil(h * vs / vmax)
            bw, bh = (wc + 7) // 8, (hc + 7) // 8
            counters["padding_skipped"] += len(grids[c]) * len(grids[c][0]) - bw * bh
            key = (1, 0 if c == 0 else 1)
            for r in range(bh):
                for col in range(bw):
                    (_ac_refine if ah else _ac_first)(sc, key, grids[c][r][col], ss, se, al)
            sc.emit_eobrun(key)
        hist = {}
        for key, s, _, _ in sc.out:
            if key is not None:
                hist.setdefault(key, [0] * 256)[s] += 1
        tables = {k: optimal_table(f) for k, f in hist.items()}
        for key in sorted(tables):
            bits, vals = tables[key]
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(key[0] << 4) | key[1]]) + bytes(bits) + bytes(vals)
        out += b"\xff\xda" + (6 + 2 * len(cs)).to_bytes(2, "big") + bytes([len(cs)])
        for c in cs:
            tbl = 0 if c == 0 else 1
            td = tbl if (ss == 0 and ah == 0) else 0
            ta = tbl if se else 0
            out += bytes([comps[c][0], (td << 4) | ta])
        out += bytes([ss, se, (ah << 4) | al])
        out += _stuffed(sc.out, {k: _codes(*t) for k, t in tables.items()})
    return bytes(out + b"\xff\xd9"), counters
