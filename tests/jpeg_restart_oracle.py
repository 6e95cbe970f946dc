"""Pure-Python restatement of libjpeg's restart_interval / restart_in_rows, for the tests of the encoder's _opts entry points.

    transcode_restart(jpg, restart_interval=0, restart_in_rows=0, optimize=False)
                          a baseline file WITHOUT intervals as libjpeg-turbo would have written it with them: the same coefficients,
                          the DC differences formed again with every component's prediction back at 0 at the start of an interval,
                          one DRI segment between the last DHT and SOS, and after every interval but the last the byte filled with
                          ones and RSTn.  optimize: the tables of jpeg_optimize_oracle, from the histogram of the NEW symbols.
    restart_mcus(...)     the interval in MCUs that libjpeg derives from the two parameters for a scan of mcus_per_row MCUs a row
    packed(jpg)           the entropy-coded segment as the encoder holds it before byte stuffing (markers in place), and where each
                          marker's 0xFF stands in it
    interval_pads(...)    the number of ones that fill the last byte of every interval

tests/test_jpeg_restart_cpu.py pins transcode_restart() to Pillow's libjpeg-turbo:
transcode_restart(save(), blocks or rows, optimize) == save(restart_marker_blocks= / restart_marker_rows=, optimize=).
"""
import functools
import math

from tests import jpeg_optimize_oracle as JO


def restart_mcus(restart_interval, restart_in_rows, mcus_per_row):
    if restart_in_rows:
        return min(restart_in_rows * mcus_per_row, 65535)   # jcmaster.c prepare_for_pass
    return restart_interval


def geometry(jpg):
    """-> (mcus_per_row, number of MCUs, [(DC table, AC table)] of an MCU's blocks in order, component of each of them)"""
    segs = JO.segments(jpg)
    sof = [s for s in segs if s[0] == 0xC0]
    assert len(sof) == 1, "baseline files only"
    a = sof[0][1]
    h, w, nc = (jpg[a + 5] << 8) | jpg[a + 6], (jpg[a + 7] << 8) | jpg[a + 8], jpg[a + 9]
    comps = [(jpg[a + 10 + 3 * c], jpg[a + 11 + 3 * c] >> 4, jpg[a + 11 + 3 * c] & 15) for c in range(nc)]
    sa = segs[-1][1]
    assert jpg[sa + 4] == nc
    sel = {jpg[sa + 5 + 2 * c]: (jpg[sa + 6 + 2 * c] >> 4, jpg[sa + 6 + 2 * c] & 15) for c in range(nc)}
    if nc == 1:   # a single-component scan is not interleaved: an MCU is one block
        return (w + 7) // 8, ((w + 7) // 8) * ((h + 7) // 8), [sel[comps[0][0]]], [0]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    per_row = math.ceil(w / (8 * hmax))
    order = [sel[cid] for cid, hs, vs in comps for _ in range(hs * vs)]
    which = [k for k, (cid, hs, vs) in enumerate(comps) for _ in range(hs * vs)]
    return per_row, per_row * math.ceil(h / (8 * vmax)), order, which


@functools.lru_cache(maxsize=512)
def _blocks(jpg):
    """the blocks of a file without intervals, in scan order: [(DC difference, [(AC symbol, extra bits, their number)])]"""
    segs = JO.segments(jpg)
    assert not any(m == 0xDD for m, _, _ in segs), "the base file has no intervals"
    _, nmcu, order, _ = geometry(jpg)
    dec = {k: JO._decoder(*v) for k, v in JO.dht_tables(jpg).items()}
    body = jpg[segs[-1][2]:]
    assert body[-2:] == b"\xff\xd9"
    raw = body[:-2].replace(b"\xff\x00", b"\xff")
    rd = JO._Reader(raw)
    out = []
    for _ in range(nmcu):
        for td, ta in order:
            s = rd.symbol(dec[(0, td)])
            v = rd.bits(s)
            diff = v if s == 0 or v >> (s - 1) else v - (1 << s) + 1
            ac, k = [], 1
            while k < 64:
                s = rd.symbol(dec[(1, ta)])
                r, z = s >> 4, s & 15
                if z == 0:
                    ac.append((s, 0, 0))
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r + 1
                ac.append((s, rd.bits(z), z))
            out.append((diff, ac))
    assert 0 <= 8 * len(raw) - rd.pos < 8, "entropy-coded segment not consumed"
    return out


def _dc_symbol(diff):
    a = abs(diff)
    n = a.bit_length()
    return n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1)


def _encode(jpg, restart_interval, restart_in_rows, optimize):
    jpg = bytes(jpg)
    segs = JO.segments(jpg)
    per_row, nmcu, order, which = geometry(jpg)
    ri = restart_mcus(restart_interval, restart_in_rows, per_row)
    assert 0 <= ri <= 65535
    blocks = _blocks(jpg)
    bpm = len(order)
    assert len(blocks) == nmcu * bpm
    # the DC values back from the differences, then the differences again with the prediction cut
    last = {}
    dc = []
    for i, (diff, _) in enumerate(blocks):
        c = which[i % bpm]
        last[c] = last.get(c, 0) + diff
        dc.append(last[c])
    syms = []   # per block: [(class, index, symbol, extra, n)]
    last = {}
    for i, (_, ac) in enumerate(blocks):
        mcu, c = i // bpm, which[i % bpm]
        if i % bpm == 0 and ri and mcu % ri == 0:
            last = {}
        td, ta = order[i % bpm]
        n, extra = _dc_symbol(dc[i] - last.get(c, 0))
        last[c] = dc[i]
        syms.append([(0, td, n, extra, n)] + [(1, ta, s, e, z) for s, e, z in ac])
    first_dht = min(a for m, a, b in segs if m == 0xC4)
    for m, a, b in segs:   # what is neither DHT nor SOS stands in front of the first DHT in every file this is written for
        assert m in (0xC4, 0xDA) or b <= first_dht
    out = bytearray(jpg[:first_dht])
    if optimize:
        hist = {}
        for blk in syms:
            for cls, idx, s, _, _ in blk:
                hist.setdefault((cls, idx), [0] * 256)[s] += 1
        tables = {k: JO.optimal_table(f) for k, f in hist.items()}
        for key in sorted(tables, key=lambda k: (k[1], k[0])):   # DC0, AC0, DC1, AC1
            bits, vals = tables[key]
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(key[0] << 4) | key[1]]) + bytes(bits) + bytes(vals)
    else:
        tables = JO.dht_tables(jpg)
        out += jpg[first_dht:segs[-1][1]]
    codes = {k: JO._codes(*t) for k, t in tables.items()}
    if ri:
        out += b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big")
    out += jpg[segs[-1][1]:segs[-1][2]]
    body, pads = bytearray(), []
    acc = nacc = 0

    def flush():
        nonlocal acc, nacc
        pads.append((8 - nacc) & 7)
        if nacc:
            by = ((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF
            body.append(by)
            if by == 0xFF:
                body.append(0)
        acc = nacc = 0

    for i, blk in enumerate(syms):
        if ri and i % bpm == 0 and i and (i // bpm) % ri == 0:   # jchuff.c emit_restart, in front of the interval's first MCU
            flush()
            body += bytes([0xFF, 0xD0 + ((i // bpm) // ri - 1) % 8])
        for cls, idx, s, extra, n in blk:
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
    flush()
    return bytes(out + body + b"\xff\xd9"), pads


def transcode_restart(jpg, restart_interval=0, restart_in_rows=0, optimize=False):
    return _encode(jpg, restart_interval, restart_in_rows, optimize)[0]


def interval_pads(jpg, restart_interval=0, restart_in_rows=0, optimize=False):
    """the ones filled into the last byte of each interval (the final one included) of transcode_restart's file"""
    return _encode(jpg, restart_interval, restart_in_rows, optimize)[1]


def packed(jpg):
    """a file WITH intervals -> (the packed stream: stuffing zeros removed, markers kept; [offset of each marker's 0xFF in it])"""
    jpg = bytes(jpg)
    body = jpg[JO.segments(jpg)[-1][2]:-2]
    out, marks, p = bytearray(), [], 0
    while p < len(body):
        b = body[p]
        out.append(b)
        p += 1
        if b != 0xFF:
            continue
        nxt = body[p]
        if nxt == 0:
            p += 1
        else:
            assert 0xD0 <= nxt <= 0xD7, hex(nxt)
            assert nxt == 0xD0 + len(marks) % 8, "markers count modulo 8"
            marks.append(len(out) - 1)
            out.append(nxt)
            p += 1
    return bytes(out), marks
