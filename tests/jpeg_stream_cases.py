"""Constructed baseline JPEG streams for the device decoder (csrc/uhdr_jpeg_dec.hip): a JPEG writer in plain Python that takes
quantised coefficients, ARBITRARY quantiser tables and ARBITRARY Huffman tables, and the named cases built with it.

Every other decoder test feeds files that an encoder wrote (standard tables, or Pillow's optimised ones where Pillow is installed).
Those never place a 16-bit code, a 27-bit symbol across a subsequence end, a stuffed byte on a chunk boundary or a scan that needs
hundreds of synchronisation launches on purpose.  The cases here do; each returns (file bytes, facts), and `facts` are the properties
the case exists for, computed from the file that was produced (tests/test_jpeg_streams_cpu.py asserts them with `check_facts`, so
a case cannot drift into testing nothing).  Where a property needs a byte at an exact offset the parameter that puts it there (a
shift, a seed) was searched once and is recorded in the case; the facts hold the search to account.

The expected planes are not stored: they come from the CPU restatement (oracle/jpeg_oracle.c) at run time, and from the image's
libjpeg where its harness builds.  Every file is a valid baseline JPEG that libjpeg decodes without a warning.

Decoder constants the facts speak about (uhdr_jpeg_dec.hip): 512-bit subsequences, 256 of them per workgroup; unstuffing in
64-byte chunks, 256 chunks (16 KiB) per workgroup; first-level tables of 11 bits.
"""
import numpy as np

SUB_BITS, SUBS_PER_GROUP = 512, 256
CHUNK, GROUP_BYTES = 64, 16384
FAST_BITS = 11

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


# ---------------------------------------------------------------------------------------------------------------------
# Huffman tables: (bits[16], vals) as a DHT segment holds them
# ---------------------------------------------------------------------------------------------------------------------
def table_from_lengths(pairs):
    """[(symbol, code length)] -> (bits, vals): canonical order, symbols of one length in the order given"""
    bits = [0] * 16
    vals = []
    for l in range(1, 17):
        for sym, sl in pairs:
            if sl == l:
                bits[l - 1] += 1
                vals.append(sym)
    assert len(vals) == len(pairs)
    return bits, vals


def huff_codes(bits, vals):
    """T.81 Annex C: {symbol: (code, length)}.  Refuses what is not a prefix code and a table that holds the all-ones code."""
    if len(bits) != 16 or sum(bits) != len(vals) or len(set(vals)) != len(vals) or not vals:
        raise ValueError("malformed table")
    codes, code, k = {}, 0, 0
    for l in range(1, 17):
        if code + bits[l - 1] > (1 << l):
            raise ValueError("not a prefix code: more codes of %d bits than fit" % l)
        for _ in range(bits[l - 1]):
            if code == (1 << l) - 1:
                raise ValueError("the all-ones code of %d bits" % l)
            codes[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return codes


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    return v if v >= 0 else v + (1 << cat) - 1   # T.81 F.1.2.1


# ---------------------------------------------------------------------------------------------------------------------
# the entropy coder
# ---------------------------------------------------------------------------------------------------------------------
class ScanEncoder:
    """Bits -> the entropy-coded segment (0x00 stuffed behind every 0xFF), with a record of every symbol: where it starts in the
    UNSTUFFED bit string (the one the decoder's subsequences cut), its length in bits (code + value bits), whether it is a DC
    difference, and the coefficient index behind it."""

    def __init__(self):
        self.out = bytearray()      # stuffed segment, markers included
        self.acc, self.nacc = 0, 0
        self.raw_bytes = 0          # unstuffed bytes so far (markers not counted)
        self.sym_pos, self.sym_len, self.sym_code_len, self.sym_dc, self.sym_z_after = [], [], [], [], []
        self.interval_raw_start = [0]
        self.marker_at = []         # offsets of the 0xFF of every RSTn inside the segment

    @property
    def raw_bits(self):
        return self.raw_bytes * 8 + self.nacc

    def put(self, code, n):
        self.acc = (self.acc << n) | code
        self.nacc += n
        while self.nacc >= 8:
            self.nacc -= 8
            b = (self.acc >> self.nacc) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.raw_bytes += 1
        self.acc &= (1 << self.nacc) - 1

    def symbol(self, codes, sym, value, is_dc, z_after):
        code, l = codes[sym]
        cat = sym & 15
        self.sym_pos.append(self.raw_bits)
        self.sym_len.append(l + cat)
        self.sym_code_len.append(l)
        self.sym_dc.append(is_dc)
        self.sym_z_after.append(z_after)
        self.put(code, l)
        if cat:
            self.put(_value_bits(value, cat), cat)

    def block(self, coef, pred, dc_codes, ac_codes):
        """one block, zigzag order, coef[0] the DC VALUE; returns the new predictor"""
        diff = int(coef[0]) - pred
        self.symbol(dc_codes, _category(diff), diff, True, 1)
        nz = np.nonzero(coef[1:])[0] + 1
        z = 1
        for k in nz:
            k = int(k)
            run = k - z
            while run >= 16:
                z += 16
                run -= 16
                self.symbol(ac_codes, 0xF0, 0, False, z)
            v = int(coef[k])
            self.symbol(ac_codes, (run << 4) | _category(v), v, False, k + 1)
            z = k + 1
        if z < 64:
            self.symbol(ac_codes, 0x00, 0, False, 64)
        return int(coef[0])

    def pad(self):
        if self.nacc:
            n = 8 - self.nacc
            self.put((1 << n) - 1, n)

    def restart(self, n):
        self.pad()
        self.marker_at.append(len(self.out))
        self.out += bytes([0xFF, 0xD0 + (n & 7)])
        self.interval_raw_start.append(self.raw_bytes)


def _mcu_layout(w, h, sampling):
    if sampling == "gray":
        return (w + 7) // 8 * ((h + 7) // 8), [0]
    if sampling == "420":
        return (w + 15) // 16 * ((h + 15) // 16), [0, 0, 0, 0, 1, 2]
    if sampling == "444":
        return (w + 7) // 8 * ((h + 7) // 8), [0, 1, 2]
    raise ValueError(sampling)


def encode_scan(coef_blocks, w, h, sampling, huff_tables, restart_interval=0):
    mcus, comps = _mcu_layout(w, h, sampling)
    coef_blocks = np.asarray(coef_blocks)
    if coef_blocks.shape != (mcus * len(comps), 64):
        raise ValueError("expected %d blocks of 64 coefficients, got %r" % (mcus * len(comps), coef_blocks.shape))
    codes = {k: huff_codes(*t) for k, t in huff_tables.items()}
    enc = ScanEncoder()
    pred = [0, 0, 0]
    b = 0
    for m in range(mcus):
        if restart_interval and m and m % restart_interval == 0:
            enc.restart(m // restart_interval - 1)
            pred = [0, 0, 0]
        for c in comps:
            t = "0" if c == 0 else "1"
            pred[c] = enc.block(coef_blocks[b], pred[c], codes["dc" + t], codes["ac" + t])
            b += 1
    enc.pad()
    return enc


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def write_jpeg_ex(coef_blocks, w, h, sampling, quant, huff_tables, restart_interval=0):
    """-> (file bytes, ScanEncoder).  coef_blocks: (blocks, 64) quantised coefficients, zigzag order, blocks in scan order (MCU by
    MCU; 4:2:0: four luma, Cb, Cr), [0] the DC value (the writer forms the differences); quant: one zigzag-order table (8 bit) for
    "gray", [luma, chroma] for "420" / "444"; huff_tables: {"dc0", "ac0"[, "dc1", "ac1"]: (bits[16], vals)}."""
    quant = [quant] if sampling == "gray" and np.ndim(quant) == 1 else list(quant)
    out = bytearray(b"\xff\xd8")
    for k, q in enumerate(quant):
        q = np.asarray(q)
        if q.shape != (64,) or q.min() < 1 or q.max() > 255:
            raise ValueError("quantiser table")
        out += _segment(0xDB, bytes([k]) + bytes(int(x) for x in q))
    if sampling == "gray":
        comps = [(1, 0x11, 0)]
    else:
        comps = [(1, 0x22 if sampling == "420" else 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) + b"".join(bytes(c) for c in comps))
    for name in sorted(huff_tables):
        bits, vals = huff_tables[name]
        huff_codes(bits, vals)
        out += _segment(0xC4, bytes([(0x10 if name[:2] == "ac" else 0) | int(name[2])]) + bytes(bits) + bytes(vals))
    if restart_interval:
        out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], 0x00 if c[2] == 0 else 0x11]) for c in comps) + bytes([0, 63, 0]))
    enc = encode_scan(coef_blocks, w, h, sampling, huff_tables, restart_interval)
    enc.scan_offset = len(out)
    out += enc.out
    out += b"\xff\xd9"
    return bytes(out), enc


def write_jpeg(coef_blocks, w, h, sampling, quant, huff_tables, restart_interval=0):
    """a complete baseline JPEG: SOI, DQT, SOF0, DHT, optional DRI, SOS, entropy-coded data with stuffing and RSTn, EOI"""
    return write_jpeg_ex(coef_blocks, w, h, sampling, quant, huff_tables, restart_interval)[0]


# ---------------------------------------------------------------------------------------------------------------------
# what the facts are computed with
# ---------------------------------------------------------------------------------------------------------------------
def scan_facts(enc):
    """the numbers every case reports: sizes of the segment and of the bit string, subsequences (without restart intervals)"""
    seg = bytes(enc.out)
    f = {"scan_bytes": len(seg), "raw_bytes": enc.raw_bytes, "intervals": len(enc.interval_raw_start)}
    if len(enc.interval_raw_start) == 1:
        f["nsub"] = (enc.raw_bytes * 8 + SUB_BITS - 1) // SUB_BITS
    else:
        starts = enc.interval_raw_start + [enc.raw_bytes]
        f["nsub"] = sum((8 * (b - a) + SUB_BITS - 1) // SUB_BITS for a, b in zip(starts[:-1], starts[1:]))
    return f


def stuffed_ff_offsets(enc):
    """offsets inside the segment of every 0xFF that a stuffed 0x00 follows"""
    a = np.frombuffer(bytes(enc.out), np.uint8)
    return np.nonzero((a[:-1] == 0xFF) & (a[1:] == 0))[0]


def group_bases(enc):
    """bytes the unstuffing pass keeps in front of every 16 KiB workgroup span = where the workgroup's output starts"""
    a = np.frombuffer(bytes(enc.out), np.uint8)
    drop = np.zeros(a.size, bool)
    drop[1:] |= (a[:-1] == 0xFF) & (a[1:] == 0)
    for m in enc.marker_at:
        drop[m] = drop[m + 1] = True
    kept = np.concatenate([[0], np.cumsum(~drop)])
    return [int(kept[g]) for g in range(0, a.size, GROUP_BYTES)]


def _lookup(bits, vals):
    look = [0] * 65536
    for sym, (code, l) in huff_codes(bits, vals).items():
        lo = code << (16 - l)
        for k in range(lo, lo + (1 << (16 - l))):
            look[k] = (l << 8) | sym
    return look


def position_walker(enc, sampling, huff_tables):
    """-> walk(p, c, z, end): the decoder's position-only walk over the unstuffed bit string from state (bit p, block-in-MCU c,
    coefficient index z) to the state behind the first symbol that crosses `end` (no code: one bit, as the decoder does)"""
    a = np.frombuffer(bytes(enc.out), np.uint8)
    drop = np.zeros(a.size, bool)
    drop[1:] |= (a[:-1] == 0xFF) & (a[1:] == 0)
    for m in enc.marker_at:
        drop[m] = drop[m + 1] = True
    raw = bytes(a[~drop]) + bytes(16)
    bpm, chroma_at = {"gray": (1, 255), "420": (6, 4), "444": (3, 1)}[sampling]
    looks = [_lookup(*huff_tables["dc0"]), _lookup(*huff_tables["ac0"])]
    looks += [_lookup(*huff_tables["dc1"]), _lookup(*huff_tables["ac1"])] if "dc1" in huff_tables else looks

    def walk(p, c, z, end):
        while p < end:
            tb = (2 if c >= chroma_at else 0) + (1 if z else 0)
            word = int.from_bytes(raw[p >> 3:(p >> 3) + 4], "big")
            e = looks[tb][(word >> (16 - (p & 7))) & 0xFFFF]
            if e == 0:
                p += 1
                continue
            sym = e & 255
            p += (e >> 8) + (sym & 15)
            if tb & 1:
                z += (sym >> 4) + 1 if sym & 15 else (16 if sym == 0xF0 else 64)
            else:
                z += 1
            if z >= 64:
                z = 0
                c = 0 if c + 1 == bpm else c + 1
        return p, c, z
    return walk


def first_pass_hits(enc, sampling, huff_tables):
    """The decoder's first pass starts subsequence i from the guess (bit 512 i, block 0, coefficient 0).  -> (number of
    subsequences i >= 1 whose guess IS the true start state, number whose first pass ends in the true end state).  Both zero: no
    subsequence is right before the true state has travelled to it from subsequence 0, one subsequence per round."""
    walk = position_walker(enc, sampling, huff_tables)
    total = enc.raw_bytes * 8
    nsub = (total + SUB_BITS - 1) // SUB_BITS
    true = [(0, 0, 0)]
    for i in range(nsub):
        true.append(walk(*true[-1], min((i + 1) * SUB_BITS, total)))
    guess_true = sum(1 for i in range(1, nsub) if true[i] == (i * SUB_BITS, 0, 0))
    end_true = sum(1 for i in range(1, nsub) if walk(i * SUB_BITS, 0, 0, min((i + 1) * SUB_BITS, total)) == true[i + 1])
    return guess_true, end_true


def idct_reference(coef_zigzag, quant_zigzag):
    """libjpeg's jidctint.c with 64-bit intermediates on (blocks, 64) zigzag coefficients: -> (the values in front of the range limit,
    the samples after it, range_limit[x & 1023])"""
    d = np.zeros((len(coef_zigzag), 64), np.int64)
    d[:, ZIGZAG] = np.asarray(coef_zigzag, np.int64) * np.asarray(quant_zigzag, np.int64)
    d = d.reshape(-1, 8, 8)

    def one_d(v, shift):   # v[..., k]: the 8 inputs
        z2, z3 = v[..., 2], v[..., 6]
        z1 = (z2 + z3) * 4433
        tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
        z2, z3 = v[..., 0], v[..., 4]
        tmp0, tmp1 = (z2 + z3) << 13, (z2 - z3) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
        z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
        z5 = (z3 + z4) * 9633
        tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
        o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
        return np.stack([(x + (1 << (shift - 1))) >> shift for x in o], -1)

    ws = one_d(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)   # pass 1 runs down the columns
    x = one_d(ws, 18)
    i = x & 1023
    s = np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
    return x, s.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _ones(n=64):
    return np.ones(n, np.int64)


def _with_magnitude(rng, cat, sign=None):
    """a value of the given category (1 <= |v| bit length == cat)"""
    m = int(rng.randint(1 << (cat - 1), 1 << cat))
    s = (1 if rng.randint(0, 2) else -1) if sign is None else sign
    return s * m


# a. / b. ---------------------------------------------------------------------------------------------------------------
# Every AC symbol is 10 bits long (categories 2..9 behind codes of 8..1 bits), every DC difference 11 (categories 3..10 behind
# codes of 8..1 bits), there is no EOB and no ZRL, and the data holds no run of eight 1-bits (the only pattern that is no code).  So
# a decoder in ANY state consumes 11 bits at coefficient index 0 and 10 bits at every other one, a block is 11 + 63 * 10 = 641
# bits for every decoder, and `bit position - bits from the block's start to the index` (the origin of the decoder's block grid,
# modulo 641; modulo 6 * 641 with the block-in-MCU index of a 4:2:0 file) never changes.  The first pass starts subsequence i at
# bit 512 i with index 0: origin 512 i, the true decoder's is 0, and 641 is odd -- the two are equal only for i a multiple of 641
# (of 3 * 641 for 4:2:0).  With fewer subsequences than that, no decoder that did not start from the true state ever reaches it:
# the true state travels from subsequence 0 one subsequence per round, four per launch inside a workgroup, one launch per workgroup
# boundary.  (Tables with the SAME lengths for DC and AC, as one would first build them, make a block 64 equal symbols long and the
# guess true every few subsequences; even with mixed lengths the index offset is zero by chance once in 64 subsequences.)
_NOSYNC_AC = table_from_lengths([(c, 10 - c) for c in range(2, 10)])
_NOSYNC_DC = table_from_lengths([(c, 11 - c) for c in range(3, 11)])
NOSYNC_BLOCK_BITS = 11 + 63 * 10


def _tame(rng, cat, sign=None):
    """a value of the category whose bits end in at most three 1s and hold no run of six"""
    while True:
        v = _with_magnitude(rng, cat, sign)
        bits = format(_value_bits(v, cat), "0%db" % cat)
        if "111111" not in bits and not bits.endswith("1111"):
            return v


def _no_sync_blocks(nblocks, comp_of, rng):
    """63 non-zero coefficients of category 6..9 per block (codes of 4..1 bits: at most three 1s in front of their 0); per component
    DC differences +m, -m, +m', -m', ... of category 7..10, so that every DC value stays within 0..1023"""
    coef = np.zeros((nblocks, 64), np.int64)
    for b in range(nblocks):
        for z in range(1, 64):
            coef[b, z] = _tame(rng, int(rng.randint(6, 10)))
    comp_of = np.array(comp_of)
    for c in set(comp_of.tolist()):
        idx = np.nonzero(comp_of == c)[0]
        for k in range(0, idx.size, 2):
            cat = int(rng.randint(7, 11))
            while True:   # both +m and -m must be tame
                m = _tame(rng, cat, 1)
                nb = format(_value_bits(-m, cat), "0%db" % cat)
                if "111111" not in nb and not nb.endswith("1111"):
                    break
            coef[idx[k], 0] = m
    return coef


def _no_sync(w, h, sampling, seed):
    rng = np.random.RandomState(seed)
    mcus, comps = _mcu_layout(w, h, sampling)
    n = mcus * len(comps)
    coef = _no_sync_blocks(n, comps * mcus, rng)
    tables = {"dc0": _NOSYNC_DC, "ac0": _NOSYNC_AC}
    quant = _ones()
    if sampling != "gray":
        tables.update({"dc1": _NOSYNC_DC, "ac1": _NOSYNC_AC})
        quant = [_ones(), _ones()]
    data, enc = write_jpeg_ex(coef, w, h, sampling, quant, tables)
    f = scan_facts(enc)
    ln, dc = np.array(enc.sym_len), np.array(enc.sym_dc)
    f["symbols_per_block"] = len(enc.sym_pos) / n
    f["symbol_bits"] = sorted(set(ln[~dc].tolist())), sorted(set(ln[dc].tolist()))
    a = np.unpackbits(np.frombuffer(bytes(enc.out), np.uint8))
    f["runs_of_eight_ones"] = int((np.convolve(a, np.ones(8, int), "valid")[:-16] == 8).sum())   # (the padding bits apart)
    f["guess_true"], f["first_pass_true"] = first_pass_hits(enc, sampling, tables)
    f["grid_period_subs"] = NOSYNC_BLOCK_BITS * (1 if sampling == "gray" else 3)
    return data, f


def no_sync_gray():
    """192x160, one plane, 480 blocks of 641 bits: 601 subsequences, three workgroups of the synchronisation kernel.  The true
    state needs 600 rounds: 64 launches for each of the first two workgroups, 23 for the last.  Measured on an MI355X: 154 launches
    reported (the next multiple of the host's look schedule, 6 + 4 k), 38 looks at the ring."""
    return _no_sync(192, 160, "gray", 101)


def no_sync_420():
    """128x96 4:2:0 (48 MCUs, 288 blocks), luma and chroma tables identical: here the block-in-MCU index, which nothing in the bits
    tells, is part of the state that never falls in step.  361 subsequences; measured on an MI355X: 94 launches, 23 looks."""
    return _no_sync(128, 96, "420", 102)


# c. ------------------------------------------------------------------------------------------------------------------
# one code per length 1..16; what a file uses most sits at the long end
_DEEP_AC = table_from_lengths([(0x03, 1), (0x04, 2), (0xF0, 3), (0x21, 4), (0x12, 5), (0x05, 6), (0x31, 7), (0x41, 8), (0x06, 9), (0x07, 10),
                               (0x13, 11), (0x11, 12), (0x02, 13), (0x01, 14), (0x00, 15), (0x0A, 16)])
_DEEP_DC = table_from_lengths([(12, 1), (13, 2), (14, 3), (15, 4), (3, 5), (4, 6), (5, 7), (6, 8), (7, 9), (8, 10), (9, 11), (10, 12), (2, 13),
                               (1, 14), (0, 15), (11, 16)])


def _deep_blocks(nblocks, comp_of, rng, shift_bits):
    """mostly DC differences of category 0..2 with a few +-1 / +-2 coefficients and an EOB (codes of 12..16 bits), every seventh block
    an AC coefficient of category 10 behind a 16-bit code (26 bits), every fifth a DC difference of category 11 (27 bits), the last
    block full up to index 63 with a 26-bit symbol as the scan's last one.  The first six blocks carry `shift_bits` bits of 4-bit
    (0x03) and 15-bit (0x01) symbols: they move everything behind them."""
    coef = np.zeros((nblocks, 64), np.int64)
    pred, target = [0, 0, 0], [1000, 1000, 1000]
    m15 = (-shift_bits) % 4          # 15 m + 4 k == shift_bits (or a multiple of 512 more), and 15 == -1 (mod 4)
    while shift_bits < 15 * m15:
        shift_bits += SUB_BITS
    k4 = (shift_bits - 15 * m15) // 4
    assert k4 >= 0 and 15 * m15 + 4 * k4 == shift_bits and m15 + k4 <= 6 * 60
    for b in range(nblocks):
        c = comp_of[b]
        if b >= 6 and b % 5 == 0:    # to +1000 and to -1000 in turn: differences of about 2000
            diff = target[c] - pred[c]
            target[c] = -target[c]
        else:
            diff = int(rng.randint(-3, 4))
        pred[c] += diff
        coef[b, 0] = pred[c]
        z = 1
        if b < 6:
            while m15 and z < 61:
                coef[b, z], m15, z = 1, m15 - 1, z + 1
            while k4 and z < 61:
                coef[b, z], k4, z = (-7, -5, 4, 6)[(b + z) % 4], k4 - 1, z + 1
        elif b == nblocks - 1:
            coef[b, 1:63] = rng.choice([-7, -6, -5, -4, 4, 5, 6, 7], 62)
            coef[b, 63] = -777
        else:
            for _ in range(int(rng.randint(0, 4))):
                z += int(rng.choice([0, 0, 1]))
                coef[b, z] = int(rng.choice([-2, -1, 1, 2, 3]))
                z += 1
            if b % 7 == 0:
                coef[b, z] = _with_magnitude(rng, 10)
    assert m15 == 0 and k4 == 0
    return coef


def _deep(sampling, w, h, seed, shift_bits):
    rng = np.random.RandomState(seed)
    mcus, comps = _mcu_layout(w, h, sampling)
    n = mcus * len(comps)
    coef = _deep_blocks(n, comps * mcus, rng, shift_bits)
    tables = {"dc0": _DEEP_DC, "ac0": _DEEP_AC}
    if sampling != "gray":
        tables.update({"dc1": _DEEP_DC, "ac1": _DEEP_AC})
    q = _ones() if sampling == "gray" else [_ones(), _ones()]
    data, enc = write_jpeg_ex(coef, w, h, sampling, q, tables)
    pos, ln = np.array(enc.sym_pos), np.array(enc.sym_len)
    long_ = ln >= 26
    f = scan_facts(enc)
    f["long_symbols"] = int(long_.sum())
    f["max_symbol_bits"] = int(ln.max())
    f["has_27_bit_dc"] = bool(((ln == 27) & np.array(enc.sym_dc)).any())
    f["has_26_bit_ac"] = bool(((ln == 26) & ~np.array(enc.sym_dc)).any())
    to_end = SUB_BITS - pos % SUB_BITS
    f["long_crossing_sub_end"] = int((long_ & (to_end < ln) & (pos + ln < enc.raw_bytes * 8)).sum())
    f["long_at_sub_start"] = int((long_ & (pos % SUB_BITS == 0) & (pos > 0)).sum())
    f["last_symbol_bits"] = int(ln[-1])
    cl = np.array(enc.sym_code_len)
    f["share_of_codes_over_11_bits"] = round(float((cl > FAST_BITS).mean()), 3)
    f["code_lengths_used"] = sorted(set(cl.tolist()))
    return data, f, enc


def deep_codes_gray():
    """96x80 one plane; the shift (recorded here, searched once) puts the start of one 26/27-bit symbol on a subsequence start"""
    shift = 127
    return _deep("gray", 96, 80, 201, shift)[:2]


def deep_codes_420():
    """96x96 4:2:0 with the same tables for luma and chroma"""
    shift = 49
    return _deep("420", 96, 96, 202, shift)[:2]


# d. ------------------------------------------------------------------------------------------------------------------
_PAIR_DC = table_from_lengths([(0, 1), (1, 2)])
_PAIR_AC = table_from_lengths([(0x01, 1), (0x00, 2), (0xF0, 3)])


def pairs():
    """128x128 one plane.  DC table {0, 1}, AC table {+-1 behind no zeros, EOB, ZRL} with codes of 1, 2 and 3 bits: nearly every
    11-bit pattern holds two symbols, so the position passes take the pair entries all the time; blocks that fill at index 63 with
    a value (no EOB), runs of 16 and 32 zeros, and subsequence ends that fall between the two symbols of a pair."""
    w, h = 128, 128
    rng = np.random.RandomState(301)
    n = (w // 8) * (h // 8)
    coef = np.zeros((n, 64), np.int64)
    pred, full, zrl = 0, 0, 0
    for b in range(n):
        pred += int(rng.randint(-1, 2)) if abs(pred) < 3 else -int(np.sign(pred))
        coef[b, 0] = pred
        z, kind = 1, b % 4
        while z < 64:
            r = rng.rand()
            if kind == 0 or r < 0.55:                  # a value (kind 0: all the way to index 63)
                coef[b, z] = 1 if rng.randint(0, 2) else -1
                z += 1
            elif r < 0.75 and z + 16 <= 63:            # 16 zeros, then a value must follow
                z += 16
                zrl += 1
                coef[b, z] = 1 if rng.randint(0, 2) else -1
                z += 1
            elif kind != 0:
                break
        full += int(coef[b, 63] != 0)
    tables = {"dc0": _PAIR_DC, "ac0": _PAIR_AC}
    data, enc = write_jpeg_ex(coef, w, h, "gray", _ones(), tables)
    f = scan_facts(enc)
    pos, ln, za = np.array(enc.sym_pos), np.array(enc.sym_len), np.array(enc.sym_z_after)
    f["blocks_full_at_63"] = full
    f["zrl_symbols"] = zrl
    ends = pos + ln
    # an AC symbol that ends exactly on a subsequence end with another AC symbol of the block behind it: the two share a pair entry
    # of the AC table (every code is at most 3 bits), which the position pass must refuse there (`bits of the first < bits left`)
    f["pair_split_by_sub_end"] = int(((ends % SUB_BITS == 0) & (za < 64) & ~np.array(enc.sym_dc) & (ends < enc.raw_bytes * 8)).sum())
    f["max_symbol_bits"] = int(ln.max())
    return data, f


# e. ------------------------------------------------------------------------------------------------------------------
_ONE_DC = table_from_lengths([(0, 1)])
_ONE_AC = table_from_lengths([(0x00, 1)])


def _flat(w, h, sampling, restart):
    mcus, comps = _mcu_layout(w, h, sampling)
    coef = np.zeros((mcus * len(comps), 64), np.int64)
    tables = {"dc0": _ONE_DC, "ac0": _ONE_AC}
    if sampling != "gray":
        tables.update({"dc1": _ONE_DC, "ac1": _ONE_AC})
    q = _ones() if sampling == "gray" else [_ones(), _ones()]
    data, enc = write_jpeg_ex(coef, w, h, sampling, q, tables, restart)
    f = scan_facts(enc)
    f["blocks"] = len(coef)
    f["bits_per_block"] = float(np.array(enc.sym_len).sum()) / len(coef)
    f["blocks_per_sub"] = SUB_BITS // 2 if not restart else None
    return data, f


def flat_one_bit_gray():
    """512x512 one plane, every block the two bits `0 0` (DC difference 0, EOB) of two tables with a single one-bit code: 256 blocks
    complete per subsequence; the tables are incomplete (every pattern that starts with a 1 is no code at all)"""
    return _flat(512, 512, "gray", 0)


def flat_one_bit_420():
    return _flat(256, 256, "420", 0)


def flat_one_bit_rst1():
    """256x256 4:2:0, a restart interval per MCU: 256 intervals of 12 bits"""
    return _flat(256, 256, "420", 1)


def flat_one_bit_rst7():
    """512x512 one plane, intervals of 7 blocks (the last one shorter)"""
    return _flat(512, 512, "gray", 7)


# f. ------------------------------------------------------------------------------------------------------------------
# AC 0x08 gets the code 1110: with the value 255 (eight 1-bits) a coefficient is `1110 1111 1111`, a 0xFF in two bytes out of three
_STUFF_DC = table_from_lengths([(0, 2), (1, 2), (2, 2)])
_STUFF_AC = table_from_lengths([(0x00, 2), (0x01, 2), (0x02, 3), (0x03, 3), (0x04, 4), (0x05, 4), (0x08, 4)])
_STUFF_TABLES = {"dc0": _STUFF_DC, "ac0": _STUFF_AC}


def _stuff_content_block(rng):
    b = np.zeros(64, np.int64)
    b[1:] = 255
    for z in rng.randint(1, 64, int(rng.randint(0, 4))):      # a few short coefficients move the phase of the 0xFF bytes
        b[z] = int(rng.choice([-1, 1, -2, 3, -5, 7, 9, -17]))
    return b


def _stuff_filler(bits_needed, nfill):
    """nfill blocks of `00` (DC difference 0), k times `010` (the coefficient -1) and `00` (EOB) that hold exactly bits_needed bits;
    no byte of them is 0xFF"""
    k_total, rem = divmod(bits_needed - 4 * nfill, 3)
    assert rem == 0 and 0 <= k_total <= 62 * nfill, (bits_needed, nfill)
    blocks = np.zeros((nfill, 64), np.int64)
    for b in range(nfill):
        k = min(62, k_total)
        blocks[b, 1:1 + k] = -1
        k_total -= k
    return blocks


def _stuff_interval(target_len, rng, shift, codes, nfill=8):
    """blocks whose entropy-coded bytes (stuffing included, padded to a byte) are exactly target_len long"""
    enc = ScanEncoder()
    blocks = []
    first = np.zeros(64, np.int64)
    first[1:1 + shift] = -1                                # `shift` coefficients of 3 bits in front of everything
    first[1 + shift:] = 255
    nxt = first
    while target_len - len(enc.out) >= 185:
        enc.block(nxt, 0, codes["dc0"], codes["ac0"])
        blocks.append(nxt)
        nxt = _stuff_content_block(rng)
    assert 40 <= target_len - len(enc.out) <= 185
    # bits still to come: up to the end of byte target_len, less 0..2 bits of padding so that the filler's size fits
    have = len(enc.out) * 8 + enc.nacc
    for pad in range(3):
        need = target_len * 8 - have - pad
        if (need - 4 * nfill) % 3 == 0:
            break
    fill = _stuff_filler(need, nfill)
    for b in fill:
        enc.block(b, 0, codes["dc0"], codes["ac0"])
        blocks.append(b)
    enc.pad()
    assert len(enc.out) == target_len, (len(enc.out), target_len)
    return blocks


def _stuffing_file(blocks, restart=0):
    coef = np.array(blocks)
    data, enc = write_jpeg_ex(coef, 8 * len(coef), 8, "gray", _ones(), _STUFF_TABLES, restart)
    f = scan_facts(enc)
    ff = stuffed_ff_offsets(enc)
    f["ff_share"] = round(float(ff.size) / len(enc.out), 3)
    f["ff_at_chunk_end"] = int((ff % CHUNK == CHUNK - 1).sum())
    f["ff_at_group_end"] = int((ff % GROUP_BYTES == GROUP_BYTES - 1).sum())
    f["group_base_mod4"] = sorted(set(b % 4 for b in group_bases(enc)))
    m = np.array(enc.marker_at, np.int64)
    f["marker_at_chunk_end"] = int((m % CHUNK == CHUNK - 1).sum())
    f["marker_at_group_end"] = int((m % GROUP_BYTES == GROUP_BYTES - 1).sum())
    f["interval_start_mod4"] = sorted(set(int(s) % 4 for s in enc.interval_raw_start[1:]))
    return data, f


def _stuffing_len(target_len, seed, shift):
    codes = {k: huff_codes(*t) for k, t in _STUFF_TABLES.items()}
    return _stuffing_file(_stuff_interval(target_len, np.random.RandomState(seed), shift, codes))


def stuffing_edges_long():
    """one plane, a scan of 65535 bytes (four workgroups of the unstuffing pass, the last one a byte short of full): about a third of
    its bytes are 0xFF; the shift recorded here puts a stuffed pair across a 64-byte chunk end and across a 16 KiB workgroup end, and
    makes the four workgroups start their output at all four alignments"""
    return _stuffing_len(65535, 401, STUFF_SHIFTS["long"])


def stuffing_edges_len_k64():
    return _stuffing_len(64 * 40, 402, STUFF_SHIFTS["k64"])


def stuffing_edges_len_k64_1():
    return _stuffing_len(64 * 40 + 1, 403, STUFF_SHIFTS["k64_1"])


def stuffing_edges_len_16384():
    return _stuffing_len(16384, 404, STUFF_SHIFTS["16384"])


def stuffing_edges_len_16385():
    return _stuffing_len(16385, 405, STUFF_SHIFTS["16385"])


def stuffing_edges_len_32767():
    return _stuffing_len(32767, 406, STUFF_SHIFTS["32767"])


def _stuffing_rst(first_len, seed, shift, more_intervals):
    """restart intervals of as many blocks as the first one, which is exactly first_len bytes long: the 0xFF of RST0 sits at offset
    first_len of the segment"""
    codes = {k: huff_codes(*t) for k, t in _STUFF_TABLES.items()}
    rng = np.random.RandomState(seed)
    blocks = _stuff_interval(first_len, rng, shift, codes)
    per = len(blocks)
    for k in range(more_intervals * per - per // 2):          # the last interval is shorter than the others
        blocks.append(_stuff_content_block(rng) if k % 3 else np.concatenate([[0], rng.choice([-1, 1, 3, 255], 63)]))
    return _stuffing_file(blocks, per)


def stuffing_edges_rst_chunk():
    """RST0's 0xFF is the last byte of a 64-byte chunk (segment offset 575); eight more intervals start at assorted alignments"""
    return _stuffing_rst(575, 407, STUFF_SHIFTS["rst_chunk"], 8)


def stuffing_edges_rst_group():
    """RST0's 0xFF is the last byte of the first 16 KiB workgroup span (segment offset 16383)"""
    return _stuffing_rst(16383, 408, STUFF_SHIFTS["rst_group"], 2)


# the number of 3-bit coefficients in front of each variant's content (searched once: the smallest value with which the variant's
# facts hold; tests/test_jpeg_streams_cpu.py asserts them)
STUFF_SHIFTS = {"long": 3, "k64": 0, "k64_1": 0, "16384": 0, "16385": 0, "32767": 0, "rst_chunk": 0, "rst_group": 0}


# g. ------------------------------------------------------------------------------------------------------------------
_DCX_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))   # T.81 table K.3
_DCX_AC = table_from_lengths([(0x00, 2), (0x01, 2)])


def _dc_extremes(restart):
    w, h = 520, 512                                           # 65 x 64 = 4160 blocks: 16 workgroups of the DC scan's 256 and 64 more
    n = (w // 8) * (h // 8)
    coef = np.zeros((n, 64), np.int64)
    coef[0::2, 0] = -1024
    coef[1::2, 0] = 1023                                      # differences: -1024, then +2047 and -2047 in turn
    coef[5::9, 1] = 1
    q = _ones()
    data, enc = write_jpeg_ex(coef, w, h, "gray", q, {"dc0": _DCX_DC, "ac0": _DCX_AC}, restart)
    f = scan_facts(enc)
    f["blocks"] = n
    f["blocks_mod_256"] = n % 256
    f["restart_mod_256"] = restart % 256
    f["dc_differences_of_category_11"] = int(((np.array(enc.sym_len) == 9 + 11) & np.array(enc.sym_dc)).sum())
    return data, f


def dc_extremes():
    """520x512 one plane, 4160 blocks, DC differences of +-2047 in turn (category 11) over the whole scan"""
    return _dc_extremes(0)


def dc_extremes_rst():
    """the same with restart intervals of 100 blocks: predictor resets at boundaries that are no multiple of 256 blocks"""
    return _dc_extremes(100)


# h. ------------------------------------------------------------------------------------------------------------------
_RL_DC = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
# EOB and every (run, size) with run 0..3 and size 1..10
_RL_AC = table_from_lengths([(0x00, 2)] + [((r << 4) | s, 5 if r == 0 and s <= 6 else 7 if r == 0 or s <= 4 else 9)
                                                      for r in range(4) for s in range(1, 11)])


def _range_limit(w, h, sampling, seed, qmax, cmax, dense=False, qmin=1):
    rng = np.random.RandomState(seed)
    mcus, comps = _mcu_layout(w, h, sampling)
    n = mcus * len(comps)
    q_luma = np.concatenate([[4 if not dense else qmax], rng.randint(qmin, qmax + 1, 63)])
    q_chroma = np.concatenate([[4], rng.randint(qmin, qmax + 1, 63)])
    coef = np.zeros((n, 64), np.int64)
    # every third block of a component is DC only: with the DC quantiser 4 the whole block is (4 dc + 4) >> 3 -- the band edges -513,
    # -512, 511 and 512 exactly, then values far outside and inside.  The other blocks: a DC value within +-500 (every DC difference
    # stays below 2048) and up to five coefficients with at most three zeros in front of each.
    edge_dc = [-1026, -1025, 1021, 1023, -1500, 1500, -200, 0, 31, 32, -1153, 1151]
    comp_of = comps * mcus
    seen = [0, 0, 0]
    for b in range(n):
        c = comp_of[b]
        seen[c] += 1
        if seen[c] % 3 == 1:
            coef[b, 0] = edge_dc[(seen[c] // 3) % len(edge_dc)]
            continue
        coef[b, 0] = int(rng.randint(-500, 501))
        z = 1
        for _ in range(int(rng.randint(1, 6))):
            z += int(rng.randint(0, 4))
            if z > 63:
                break
            coef[b, z] = int(np.clip(_with_magnitude(rng, int(rng.randint(1, 11))), -cmax, cmax))
            z += 1
    if dense:   # every coefficient of some blocks at the largest magnitude, signs at random: the sums of a pass grow with their number
        for b in range(1, n, 4):
            coef[b, 1:] = rng.choice([-cmax, cmax], 63)
            coef[b, 0] = 500 if (b // 4) % 2 else -500
        coef[40:45, 0] = [0, 2047, 0, -2047, 0]   # DC differences of +-2047 (the largest a baseline file holds) under the quantiser 255
    tables = {"dc0": _RL_DC, "ac0": _RL_AC}
    quant = q_luma
    if sampling != "gray":
        tables.update({"dc1": _RL_DC, "ac1": _RL_AC})
        quant = [q_luma, q_chroma]
    data, enc = write_jpeg_ex(coef, w, h, sampling, quant, tables)
    f = scan_facts(enc)
    qs = np.where(np.array(comp_of)[:, None] == 0, q_luma[None, :], q_chroma[None, :])
    x, _ = idct_reference(coef, qs)
    f["max_dequantised"] = int(np.abs(coef * qs).max())
    f["bands"] = [int((x < -512).sum()), int(((x >= -512) & (x < -128)).sum()), int(((x >= -128) & (x < 128)).sum()),
                  int(((x >= 128) & (x < 512)).sum()), int((x >= 512).sum())]
    f["edges"] = [int((x == v).sum()) for v in (-513, -512, 511, 512)]
    return data, f


def range_limit_gray():
    """64x48 one plane: reconstructions (in front of the +128) in every band of libjpeg's range_limit[x & 1023] -- under -512, up to
    -129, -128..127, up to 511, above -- with -513, -512, 511 and 512 exactly; |coefficient x quantiser| <= 32767"""
    return _range_limit(64, 48, "gray", 501, 32, 1023)


def range_limit_420():
    """50x38 4:2:0: neither plane a multiple of 8, so the edge blocks are stored byte by byte"""
    return _range_limit(50, 38, "420", 502, 32, 1023)


def range_limit_wide():
    """quantisers up to 255 with coefficients up to 137 in magnitude: |coefficient x quantiser| reaches past 32768, where the decoder
    switches its first IDCT pass to 64 bits, and stays within the 35081 up to which 32 bits cannot overflow (uhdr_jpeg_dec.hip,
    "dequantisation + IDCT"): blocks on both sides of the switch"""
    return _range_limit(64, 48, "gray", 503, 255, 137, qmin=240)


def range_limit_max():
    """the legal maximum: every quantiser 255, a quarter of the blocks full of +-1023, DC values of +-2047 reached by differences of
    +-2047: dequantised magnitudes of 260865 (AC) and 521985 (DC), where the first IDCT pass overflows 32 bits (libjpeg computes in
    64) and nearly every reconstruction lies outside -512..511"""
    return _range_limit(64, 48, "gray", 504, 255, 1023, dense=True, qmin=255)


CASES = {
    "no_sync_gray": no_sync_gray, "no_sync_420": no_sync_420,
    "deep_codes_gray": deep_codes_gray, "deep_codes_420": deep_codes_420,
    "pairs": pairs,
    "flat_one_bit_gray": flat_one_bit_gray, "flat_one_bit_420": flat_one_bit_420, "flat_one_bit_rst1": flat_one_bit_rst1,
    "flat_one_bit_rst7": flat_one_bit_rst7,
    "stuffing_edges_long": stuffing_edges_long, "stuffing_edges_len_k64": stuffing_edges_len_k64,
    "stuffing_edges_len_k64_1": stuffing_edges_len_k64_1, "stuffing_edges_len_16384": stuffing_edges_len_16384,
    "stuffing_edges_len_16385": stuffing_edges_len_16385, "stuffing_edges_len_32767": stuffing_edges_len_32767,
    "stuffing_edges_rst_chunk": stuffing_edges_rst_chunk, "stuffing_edges_rst_group": stuffing_edges_rst_group,
    "dc_extremes": dc_extremes, "dc_extremes_rst": dc_extremes_rst,
    "range_limit_gray": range_limit_gray, "range_limit_420": range_limit_420, "range_limit_wide": range_limit_wide,
    "range_limit_max": range_limit_max,
}

_BUILT = {}


def case(name):
    """(file bytes, facts) of a case, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]
