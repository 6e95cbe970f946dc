"""Constructed images for the device JPEG encoder (csrc/uhdr_jpeg.hip): pixels chosen so that the entropy-coded stream the encoder
has to write lands on the limits of its kernels -- a stream of exactly one 16 KiB stuffing piece, a 0xFF on either side of a chunk or
piece edge, blocks of 6 bits that share a word, three ZRL codes and no EOB, and so on.

Every other encoder test feeds content (smooth, noise, extreme, flat) and takes what stream comes.  The cases here are steered: each
returns the planes, sizes, strides and quality of one encode plus `facts`, the properties the case exists for.  The facts are
computed from the file the CPU checker (oracle/jpeg_oracle.c, pinned to libjpeg by tests/test_jpeg_oracle.py) writes for those
pixels; tests/test_jpeg_encode_cases_cpu.py asserts them with `check_facts`, so a case cannot drift into testing nothing.  Where a
property needs a byte at an exact offset, the parameters that put it there (filler blocks, a seed) were searched once with the
functions `search_*` at the end of this module and are recorded as constants: a case costs one oracle encode.

The expected files are not stored: they are the oracle's, at run time.

Encoder constants the facts speak about (uhdr_jpeg.hip, uhdr_jpeg.h; tests/test_jpeg_encode_cases_cpu.py reads them from the source
and names the cases that have gone stale when one moves):
  128 blocks per workgroup of the DCT, clear and emit kernels; byte stuffing in chunks of 64 bytes, one thread each, 256 chunks =
  one 16 KiB piece per workgroup; at most 64 stuffing workgroups per job of a batch, striding over the pieces; 128 jobs per round.
"""
import numpy as np

from tests.jpeg_stream_cases import _lookup

CHUNK = 64               # kChunk
PIECE_CHUNKS = 256       # chunks per stuffing workgroup
PIECE = CHUNK * PIECE_CHUNKS
WG_BLOCKS = 128          # blocks per workgroup of k_jpeg_fdct_quant_count / k_jpeg_clear_multi / k_jpeg_emit
STUFF_WG_PER_JOB = 64    # kStuffWgPerJob
MAX_BATCH_JOBS = 128     # kMaxBatchJobs
FLAT_BITS = 6            # a block whose DC difference is 0 and whose AC is zero: DC category 0 (2 bits) + EOB (4 bits), both tables' luma


# ---------------------------------------------------------------------------------------------------------------------
# reading a file back: the packed stream, and the blocks in it
# ---------------------------------------------------------------------------------------------------------------------
def parse_file(data):
    """-> dict(w, h, gray, tables {"dc0", "ac0"[, "dc1", "ac1"]: (bits, vals)}, header_len = offset of the entropy-coded segment,
    icc_len).  Only what the project's encoder writes: baseline, one scan, no restart intervals."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    p, info = 2, {"tables": {}, "icc_len": 0}
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        body = data[p + 4:p + 2 + n]
        if m == 0xC0:
            info["h"], info["w"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            info["gray"] = body[5] == 1
        elif m == 0xC4:
            q = 0
            while q < len(body):
                bits = list(body[q + 1:q + 17])
                nv = sum(bits)
                info["tables"][("ac" if body[q] & 0x10 else "dc") + str(body[q] & 15)] = (bits, list(body[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xE2:
            info["icc_len"] = n - 2
        elif m == 0xDD:
            raise AssertionError("restart intervals: not this encoder's")
        p += 2 + n
        if m == 0xDA:
            info["header_len"] = p
            return info


def packed_stream(data):
    """-> (the entropy-coded bytes between SOS and EOI with the stuffed zeros removed: what k_jpeg_emit writes, as a uint8 array;
    the offsets in it of the 0xFF bytes)"""
    a = np.frombuffer(bytes(data), np.uint8)[parse_file(data)["header_len"]:-2]
    stuffed = np.zeros(a.size, bool)
    stuffed[1:] = (a[:-1] == 0xFF) & (a[1:] == 0)
    assert not ((a[:-1] == 0xFF) & (a[1:] != 0)).any() and (a.size == 0 or a[-1] != 0xFF), "a marker inside the segment"
    packed = a[~stuffed]
    assert int(stuffed.sum()) == int((packed == 0xFF).sum())
    return packed, np.nonzero(packed == 0xFF)[0]


def restuff(packed):
    """the packed stream with a zero behind every 0xFF, as bytes: the segment of the file again"""
    packed = np.asarray(packed, np.uint8)
    out = np.zeros(packed.size + int((packed == 0xFF).sum()), np.uint8)
    at = np.arange(packed.size) + np.concatenate([[0], np.cumsum(packed == 0xFF)[:-1]])
    out[at] = packed
    return out.tobytes()


def block_count(w, h, gray):
    return (w + 7) // 8 * ((h + 7) // 8) if gray else 6 * ((w + 15) // 16) * ((h + 15) // 16)


def locate(i, w, h, gray):
    """block i of the entropy-coding order, as uhdr_jpeg.hip's locate() has it -> (component, block row, block column, dummy)"""
    ybw, ybh = (w + 7) // 8, (h + 7) // 8
    if gray:
        return 0, i // ybw, i % ybw, False
    mcus_x = (w + 15) // 16
    mcu, k = divmod(i, 6)
    mr, mc = divmod(mcu, mcus_x)
    if k >= 4:
        return k - 3, mr, mc, False
    br, bc = 2 * mr + (k >> 1), 2 * mc + (k & 1)
    return 0, br, bc, not (br < ybh and bc < ybw)


def dc_predecessor(i, gray):
    if gray:
        return i - 1 if i else None
    mcu, k = divmod(i, 6)
    if k >= 4:
        return i - 6 if mcu else None
    if k:
        return i - 1
    return i - 3 if mcu else None


def walk_blocks(data):
    """every block of the file's scan, in entropy-coding order -> list of (bit offset in the packed stream, length in bits, symbols);
    symbols: [(DC category, DC difference), (run/size byte, value), ...] -- 0xF0 is ZRL, 0x00 is EOB, both with value 0.
    Also returns the number of padding bits behind the last block (they must be ones)."""
    info = parse_file(data)
    packed, _ = packed_stream(data)
    raw = packed.tobytes() + bytes(8)
    t = info["tables"]
    looks = [_lookup(*t["dc0"]), _lookup(*t["ac0"])]
    looks += [_lookup(*t["dc1"]), _lookup(*t["ac1"])] if not info["gray"] else []
    n = block_count(info["w"], info["h"], info["gray"])
    out, p = [], 0

    def take(tb):
        nonlocal p
        word = int.from_bytes(raw[p >> 3:(p >> 3) + 5], "big")
        e = looks[tb][(word >> (24 - (p & 7))) & 0xFFFF]
        assert e, "no code at bit %d" % p
        p += e >> 8
        sym = e & 255
        s = sym & 15
        v = 0
        if s:
            word = int.from_bytes(raw[p >> 3:(p >> 3) + 4], "big")
            v = (word >> (32 - (p & 7) - s)) & ((1 << s) - 1)
            if v < (1 << (s - 1)):
                v -= (1 << s) - 1
            p += s
        return sym, v

    for i in range(n):
        chroma = 0 if info["gray"] or i % 6 < 4 else 2
        start = p
        syms = [take(chroma)]
        z = 1
        while z < 64:
            sym, v = take(chroma + 1)
            syms.append((sym, v))
            if sym == 0:
                break
            z += 16 if sym == 0xF0 else (sym >> 4) + 1
        assert z <= 64
        out.append((start, p - start, syms))
    pad = 8 * packed.size - p
    assert 0 <= pad < 8 and (pad == 0 or packed[-1] & ((1 << pad) - 1) == (1 << pad) - 1), "padding"
    return out, pad


def coefficients_of(blocks, gray):
    """walk_blocks' symbols -> (blocks, 64) quantised coefficients in zigzag order, the DC values restored from the differences"""
    out = np.zeros((len(blocks), 64), np.int16)
    for i, (_, _n, syms) in enumerate(blocks):
        p = dc_predecessor(i, gray)
        out[i, 0] = (out[p, 0] if p is not None else 0) + syms[0][1]
        z = 1
        for sym, v in syms[1:]:
            if sym == 0:
                break
            if sym == 0xF0:
                z += 16
                continue
            z += sym >> 4
            out[i, z] = v
            z += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def _item(y, uv=None, q=100, **facts):
    """y: the luma plane; uv: the Cb plane above the Cr plane (4:2:0) or None; tight strides"""
    h, w = y.shape
    return dict(yb=np.ascontiguousarray(y), ub=None if uv is None else np.ascontiguousarray(uv), w=w, h=h, ls=w,
                cs=0 if uv is None else w // 2, q=q, facts=facts)


def _gray_from_blocks(blocks, bw):
    """(n, 8, 8) uint8 blocks in raster (= entropy-coding) order -> the single-plane image of bw blocks per row"""
    blocks = np.asarray(blocks, np.uint8)
    n = blocks.shape[0]
    assert n % bw == 0, (n, bw)
    return np.ascontiguousarray(blocks.reshape(n // bw, bw, 8, 8).transpose(0, 2, 1, 3).reshape(n // bw * 8, bw * 8))


def _flat(values):
    return np.repeat(np.asarray(values, np.uint8), 64).reshape(-1, 8, 8)


def _alternating(n, first=0):
    """n flat blocks 0, 255, 0, ...: at quality 100 every DC difference is +-2040 (-1024 in front), category 11; 24 bits a block, and
    one byte in three of a byte-aligned run is 0xFF"""
    v = np.where(np.arange(n) % 2 == 0, first, 255 - first)
    return _flat(v)


def _noise_blocks(seed, n):
    return np.random.RandomState(seed).randint(0, 256, (n, 8, 8)).astype(np.uint8)


def _hf_block(amp):
    """128 + amp cos((2x+1) 7 pi/16) cos((2y+1) 7 pi/16): energy in coefficient 63 alone"""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return np.clip(128 + np.round(amp * np.outer(c, c)), 0, 255).astype(np.uint8)


def _flat_len(nbytes):
    """the number of 6-bit blocks whose stream is nbytes long (the largest)"""
    return 8 * nbytes // FLAT_BITS


def _grid(n):
    """n = bw * bh with bw as close to the square root as n's factors allow, bw >= bh"""
    bh = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return n // bh, bh


def _flat_case(nbytes, **facts):
    n = _flat_len(nbytes)
    bw, _ = _grid(n)
    return _item(_gray_from_blocks(_flat([128] * n), bw), packed_len=nbytes, **facts)


def _mixed_len_case(nbytes, nalt):
    """nalt alternating blocks (3 bytes each) in front of flat ones: a stream of nbytes that is not all zeros and ones in one pattern"""
    n = nalt + _flat_len(nbytes - 3 * nalt)
    bw, _ = _grid(n)
    return _item(_gray_from_blocks(np.concatenate([_alternating(nalt), _flat([255] * (n - nalt))]), bw), packed_len=nbytes)


def _prefix_case(nflat, body, ntail=0, q=100, **facts):
    """nflat flat-128 blocks, the blocks `body`, flat-128 blocks up to a whole grid"""
    n = nflat + len(body) + ntail
    bw, _ = _grid(n)
    blocks = np.concatenate([_flat([128] * nflat), body, _flat([128] * ntail)])
    return _item(_gray_from_blocks(blocks, bw), q=q, **facts)


def _tail_for_grid(n, lo=0):
    """the smallest ntail >= lo for which n + ntail has a grid no more oblong than 8:1"""
    t = lo
    while True:
        bw, bh = _grid(n + t)
        if bw <= 8 * bh:
            return t
        t += 1


# ---------------------------------------------------------------------------------------------------------------------
# constants the searches at the end of the module found (search_ff(), search_pair(), search_long_block())
# ---------------------------------------------------------------------------------------------------------------------
# ff_at_*: (129 / 128 pairs in front, flat-128 blocks behind them, alternating blocks behind those)
FF_SINGLE = {"ff_at_63": (0, 82, 12), "ff_at_64": (1, 80, 12), "ff_at_16383": (0, 21842, 12), "ff_at_16384": (1, 21840, 12)}
# ff_at_*_and_*: (flat-128 blocks in front, then _pair_body(u, v0, m, amp)), quality 90
FF_PAIR = {"ff_at_63_and_64": (78, 129, 45, 237, 20), "ff_at_16383_and_16384": (21838, 129, 45, 237, 20)}
FF_PAIR_QUALITY = 90
# long_blocks: the 64 samples of the block, one bit each (0 / 255), row by row from the top bit down; and the bits it takes
LONG_BLOCK = 0xd721441f3aa26431
LONG_BLOCK_MIN_BITS = 990


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def len_64k():
    return _mixed_len_case(5 * CHUNK, 40)


def len_64k_p1():
    return _mixed_len_case(5 * CHUNK + 1, 40)


def len_64k_m1():
    return _mixed_len_case(5 * CHUNK - 1, 40)


def len_16384():
    return _flat_case(PIECE)


def len_16385():
    return _flat_case(PIECE + 1)


def len_16383():
    return _flat_case(PIECE - 1)


def len_32768():
    return _flat_case(2 * PIECE)


def bits_mod8_0():
    """4 alternating blocks (96 bits) and 16 flat ones (96 bits): 192 bits = 6 words, no padding, the last block ends on a word"""
    return _item(_gray_from_blocks(np.concatenate([_alternating(4), _flat([255] * 16)]), 5), total_bits=192, pad_bits=0, block_ends_on_word=True)


def _ff_single(name, offsets, absent=()):
    npair, nflat, nalt = FF_SINGLE[name]
    head = _flat([129, 128] * npair + [128] * nflat)     # a 129 / 128 pair costs 22 bits, not 12: it moves the run's byte phase
    ntail = _tail_for_grid(len(head) + nalt)
    n = len(head) + nalt + ntail
    bw, _ = _grid(n)
    blocks = np.concatenate([head, _alternating(nalt), _flat([_alternating(nalt)[-1, 0, 0]] * ntail)])
    return _item(_gray_from_blocks(blocks, bw), ff_at=list(offsets), ff_not_at=list(absent))


def ff_at_63():
    return _ff_single("ff_at_63", [CHUNK - 1], [CHUNK])


def ff_at_64():
    return _ff_single("ff_at_64", [CHUNK], [CHUNK - 1])


def ff_at_16383():
    return _ff_single("ff_at_16383", [PIECE - 1], [PIECE])


def ff_at_16384():
    return _ff_single("ff_at_16384", [PIECE], [PIECE - 1])


def _pair_body(u, v0, m, amp):
    """Three blocks that hold 18 one-bits in a row at quality 90: flat u (sets the bit phase), flat v0, and m + amp cos((2y+1) pi/16)
    in every column.  The last one's DC difference to v0 is 2^9 - 1, nine value bits of ones; its rows are constant, so coefficient 1
    is exactly zero, and coefficient 2 is of category 6: the symbol 1/6, whose 16-bit code starts with nine ones."""
    c = np.cos((2 * np.arange(8) + 1) * np.pi / 16)
    blk = np.clip(np.round(m + amp * c)[:, None] * np.ones((1, 8)), 0, 255).astype(np.uint8)
    return np.concatenate([_flat([u, v0]), blk[None]])


def _ff_pair(name, offsets):
    nflat, u, v0, m, amp = FF_PAIR[name]
    return _prefix_case(nflat, _pair_body(u, v0, m, amp), _tail_for_grid(nflat + 3, 2), q=FF_PAIR_QUALITY, ff_at=list(offsets))


def ff_at_63_and_64():
    return _ff_pair("ff_at_63_and_64", [CHUNK - 1, CHUNK])


def ff_at_16383_and_16384():
    return _ff_pair("ff_at_16383_and_16384", [PIECE - 1, PIECE])


def ff_last_byte():
    """one block whose 15-byte stream ends in 0xFF once the last byte is filled with ones: the file ends FF 00 FF D9"""
    return _item(_hf_block(8), packed_len=15, last_byte_ff=True)


def ff_last_byte_chunk_end():
    """236 flat blocks (177 bytes: a multiple of 4 blocks keeps the byte alignment) in front of ff_last_byte's block: 192 bytes"""
    nflat = 236
    assert (nflat * FLAT_BITS // 8 + 15) % CHUNK == 0
    return _item(_gray_from_blocks(np.concatenate([_flat([128] * nflat), _hf_block(8)[None]]), 79), packed_len=nflat * FLAT_BITS // 8 + 15,
                 last_byte_ff=True, len_mod_chunk=0)


def ff_dense(bw=128, bh=128):
    """alternating blocks throughout: 3 bytes a block, one of them 0xFF.  128 x 128 blocks = 3 pieces of 16 KiB, each expanding to
    more than 20 KiB in the stuffing workgroup's LDS"""
    return _item(_gray_from_blocks(_alternating(bw * bh), bw), min_pieces=3, min_ff_per_piece=5000)


def ff_none_long(bw=256, bh=176):
    """flat 128: more than two pieces of 00101000 10100010 10001010"""
    return _item(_gray_from_blocks(_flat([128] * (bw * bh)), bw), min_pieces=2, ff_count=0)


def six_bit_blocks(bw=32, bh=8):
    """8 noise blocks, then flat ones: runs of blocks that fit inside one word next to blocks that store whole words"""
    n = bw * bh
    blocks = np.concatenate([_noise_blocks(5, 8), _flat([128] * (n - 8))])
    return _item(_gray_from_blocks(blocks, bw), six_bit_run=128, word_with_5_blocks=True, block_at_bit0=True)


def zrl3_no_eob():
    """three blocks of 128 + 100 x (the basis function of coefficient 63) at quality 50, where the samples' rounding quantises to
    zero: DC, ZRL, ZRL, ZRL, the symbol 14/n, and no EOB"""
    return _item(np.tile(_hf_block(100), (1, 3)), q=50, zrl3_no_eob=("luma",))


def zrl3_no_eob_420():
    """the same block everywhere in a 32 x 16 4:2:0 image, so that the chroma AC table is walked as well"""
    y = np.tile(_hf_block(100), (2, 4))
    c = np.tile(_hf_block(100), (1, 2))
    return _item(y, np.concatenate([c, c]), q=50, zrl3_no_eob=("luma", "chroma"))


def dc_cat11():
    """4:2:0, quality 100, luma and chroma of flat blocks 0 / 255 that alternate in coding order: DC differences +-2040"""
    mx, my = 4, 3
    # Y00 Y01 Y10 Y11 = 0 255 0 255 in every MCU: differences of +-2040 inside the MCU and across MCUs
    y = np.where((np.arange(16 * mx) // 8 % 2 == 1)[None, :], 255, 0).astype(np.uint8) * np.ones((16 * my, 1), np.uint8)
    cb = _gray_from_blocks(_alternating(mx * my), mx)
    cr = _gray_from_blocks(_alternating(mx * my, 255), mx)
    return _item(y, np.concatenate([cb, cr]), dc_cat11=("luma+", "luma-", "chroma+", "chroma-"))


def max_block_bits_of_samples():
    """An upper bound on the bits of one block that comes from 8-bit samples.  The code's worst case, 20 + 63 x 26 = 1658 bits, needs
    63 coefficients of magnitude >= 512.  The DCT is orthonormal, so the squared coefficients of a block sum to the squared
    level-shifted samples, at most 64 x 128^2: room for four such coefficients, or for 63 of magnitude 128.  The bound: a DC symbol
    of 20 bits plus the most bits 63 run-0 symbols of the luma table (the longer one) take under that energy, a coefficient of
    category c having magnitude >= 2^(c-1).  Symbols with a run are left out: a zero frees at most 128^2 of energy, which buys a
    neighbour 7 bits (category 8 to 9) and costs the 18 of the coefficient it replaces.  Quantisation at quality 100 divides by 1;
    its rounding moves a coefficient by half a unit, which is ignored here."""
    codelen = {1: 2, 2: 2, 3: 3, 4: 4, 5: 5, 6: 7, 7: 8, 8: 10, 9: 16, 10: 16}   # T.81 table K.5, run 0
    unit = 256                                                                   # energies in units of 16^2, rounded down: still a bound
    budget = 64 * 128 * 128 // unit
    best = np.zeros(budget + 1, np.int64)                                        # energy spent -> most bits, over the coefficients so far
    for _ in range(63):
        nxt = best.copy()
        for c, l in codelen.items():
            e = (1 << (2 * (c - 1))) // unit
            nxt[e:] = np.maximum(nxt[e:], best[:budget + 1 - e] + l + c)
        best = nxt
    return 20 + int(best.max())


def _long_block():
    return (np.unpackbits(np.frombuffer(LONG_BLOCK.to_bytes(8, "big"), np.uint8)).reshape(8, 8) * 255).astype(np.uint8)


def long_blocks():
    """The longest block a search over 0 / 255 patterns found at quality 100 (search_long_block), between noise blocks.  8-bit
    samples cannot reach the 1400 bits one might ask for, let alone the code's 1658: see max_block_bits_of_samples (1154)."""
    blocks = np.concatenate([_noise_blocks(3, 3), _long_block()[None], _noise_blocks(4, 4)])
    return _item(_gray_from_blocks(blocks, 4), min_block_bits=LONG_BLOCK_MIN_BITS)


def _smooth(w, h, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip((np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 50 + 128 + rng.randint(-6, 7, (h, w)), 0, 255).astype(np.uint8)


def _nblk(n, q=90):
    bw, bh = _grid(n)
    return _item(_smooth(8 * bw, 8 * bh, n), q=q, nblk=n)


def nblk_127():
    return _nblk(WG_BLOCKS - 1)


def nblk_128():
    return _nblk(WG_BLOCKS)


def nblk_129():
    return _nblk(WG_BLOCKS + 1)


def nblk_16385():
    return _nblk(WG_BLOCKS * WG_BLOCKS + 1)


def nblk_16513():
    """130 workgroups: workgroup 129 is the first whose sum over the workgroups in front (one per thread, 128 threads) takes a second
    trip -- with 129 workgroups (nblk_16385) the last one still sums 128 values in one trip"""
    return _nblk(WG_BLOCKS * (WG_BLOCKS + 1) + 1)


def c420_wg_edge():
    """4:2:0, 242 x 82: 31 x 11 luma blocks in 16 x 6 MCUs, 576 blocks.  Block 512 = Y10 of MCU 85 (last MCU row) is a dummy at
    index 4 x 128; block 384 = Y00 of MCU 64, whose DC predecessor, Y11 of MCU 63 (last MCU column), is a dummy, at index 3 x 128"""
    w, h = 242, 82
    rng = np.random.RandomState(12)
    y = np.clip(_smooth(w, h, 1).astype(int) + rng.randint(-40, 41, (h, w)), 0, 255).astype(np.uint8)
    uv = rng.randint(0, 256, (h // 2 * 2, w // 2)).astype(np.uint8)
    return _item(y, uv, q=90, dummy_at_wg_start=True, y00_after_dummy_at_wg_start=True, min_blocks=WG_BLOCKS + 1)


def _noise_420(w, h, seed, **facts):
    rng = np.random.RandomState(seed)
    return _item(rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h, w // 2)).astype(np.uint8), **facts)


def stride_2nd_trip():
    """more than 64 pieces: the stuffing workgroups of a batch job (kStuffWgPerJob = 64) walk their loop a second time"""
    return _noise_420(832, 640, 31, min_packed_len=STUFF_WG_PER_JOB * PIECE + 1)


def pieces_257():
    """Piece 257 is the first whose sum over the pieces in front (one per thread, 256 threads) takes a second trip, so the case has
    at least 258 pieces -- more than the 256 x 16384 bytes that make piece 256 exist"""
    return _noise_420(1600, 1216, 32, min_packed_len=(PIECE_CHUNKS + 1) * PIECE + 1)


CASES = {f.__name__: f for f in (
    len_64k, len_64k_p1, len_64k_m1, len_16384, len_16385, len_16383, len_32768, bits_mod8_0, ff_at_63, ff_at_64, ff_at_63_and_64,
    ff_at_16383, ff_at_16384, ff_at_16383_and_16384, ff_last_byte, ff_last_byte_chunk_end, ff_dense, ff_none_long, six_bit_blocks,
    zrl3_no_eob, zrl3_no_eob_420, dc_cat11, long_blocks, nblk_127, nblk_128, nblk_129, nblk_16385, nblk_16513, c420_wg_edge,
    stride_2nd_trip, pieces_257)}
LARGE = ("stride_2nd_trip", "pieces_257")
# which cases lean on which constant of the encoder (tests/test_jpeg_encode_cases_cpu.py names them when the constant moves)
USES = {
    "CHUNK": ["len_64k", "len_64k_p1", "len_64k_m1", "ff_at_63", "ff_at_64", "ff_at_63_and_64", "ff_last_byte_chunk_end"],
    "PIECE_CHUNKS": ["len_16384", "len_16385", "len_16383", "len_32768", "ff_at_16383", "ff_at_16384", "ff_at_16383_and_16384", "ff_dense",
                     "ff_none_long", "pieces_257"],
    "WG_BLOCKS": ["nblk_127", "nblk_128", "nblk_129", "nblk_16385", "nblk_16513", "c420_wg_edge", "six_bit_blocks"],
    "STUFF_WG_PER_JOB": ["stride_2nd_trip"],
    "MAX_BATCH_JOBS": ["(the all-qualities batch of tests/test_gpu_jpeg_encode_limits.py: 200 jobs = two rounds)"],
}

_BUILT = {}


def case(name):
    """the case, built once per process (the planes must not be written to)"""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def oracle_file(orc, it):
    """the CPU checker's file for an item (a case, or any dict of the same keys), kept with the item"""
    if "_want" not in it:
        it["_want"] = orc.jpeg_encode("orc", it["yb"], it["ub"], it["w"], it["h"], it["q"], it["ls"], it["cs"], icc=it.get("icc"))
    return it["_want"]


# ---------------------------------------------------------------------------------------------------------------------
# the facts, computed from the oracle's file
# ---------------------------------------------------------------------------------------------------------------------
def check_facts(name, it, data):
    """asserts every fact of case `name` (item `it`) on `data`, the oracle's file for it; returns the figures it looked at"""
    f = it["facts"]
    info = parse_file(data)
    packed, ff = packed_stream(data)
    ffs = set(ff.tolist())
    fig = {"packed_len": int(packed.size), "ff": int(ff.size), "file_len": len(data)}
    assert (info["w"], info["h"], info["gray"]) == (it["w"], it["h"], it["ub"] is None), name
    blocks = None
    if name not in LARGE:
        blocks, pad = walk_blocks(data)
        assert sum(b[1] for b in blocks) + pad == 8 * packed.size, name
        fig["total_bits"], fig["pad_bits"] = 8 * packed.size - pad, pad
        fig["max_block_bits"] = max(b[1] for b in blocks)
    for key, want in f.items():
        if key == "packed_len":
            assert packed.size == want, (name, packed.size)
        elif key == "min_packed_len":
            assert packed.size >= want, (name, packed.size)
        elif key == "len_mod_chunk":
            assert packed.size % CHUNK == want, (name, packed.size)
        elif key == "total_bits":
            assert fig["total_bits"] == want, (name, fig["total_bits"])
        elif key == "pad_bits":
            assert fig["pad_bits"] == want, (name, fig["pad_bits"])
        elif key == "block_ends_on_word":
            assert any((o + n) % 32 == 0 for o, n, _ in blocks), name
        elif key == "ff_at":
            assert all(o in ffs for o in want), (name, sorted(ffs)[:8])
        elif key == "ff_not_at":
            assert not any(o in ffs for o in want), (name, sorted(ffs)[:8])
        elif key == "last_byte_ff":
            assert packed[-1] == 0xFF and data[-4:] == b"\xff\x00\xff\xd9", name
        elif key == "min_pieces":
            assert packed.size > (want - 1) * PIECE, (name, packed.size)
        elif key == "min_ff_per_piece":
            per = [int(((ff >= g) & (ff < g + PIECE)).sum()) for g in range(0, f["min_pieces"] * PIECE, PIECE)]
            assert min(per) >= want and 2 * min(per) + PIECE > 20 * 1024, (name, per)
            fig["ff_per_piece"] = per
        elif key == "ff_count":
            assert ff.size == want, (name, ff.size)
        elif key == "six_bit_run":
            run = best = 0
            for _, n, _s in blocks:
                run = run + 1 if n == FLAT_BITS else 0
                best = max(best, run)
            assert best >= want, (name, best)
        elif key == "word_with_5_blocks":
            firsts = [o for o, n, _ in blocks if n == FLAT_BITS]
            inside = {}
            for o in firsts:
                if o // 32 == (o + FLAT_BITS - 1) // 32:
                    inside[o // 32] = inside.get(o // 32, 0) + 1
            assert max(inside.values()) == 5, name
        elif key == "block_at_bit0":
            assert any(o % 32 == 0 and o for o, _, _s in blocks), name
        elif key == "zrl3_no_eob":
            hit = set()
            for i, (_, _n, syms) in enumerate(blocks):
                if [s[0] for s in syms[1:4]] == [0xF0] * 3 and len(syms) == 5 and syms[4][0] >> 4 == 14 and syms[4][0] & 15:
                    hit.add("luma" if info["gray"] or i % 6 < 4 else "chroma")
            assert hit == set(want), (name, hit)
        elif key == "dc_cat11":
            hit = set()
            for i, (_, _n, syms) in enumerate(blocks):
                if syms[0][0] == 11:
                    hit.add(("luma" if i % 6 < 4 else "chroma") + ("+" if syms[0][1] > 0 else "-"))
            assert hit == set(want), (name, hit)
        elif key == "min_block_bits":
            assert fig["max_block_bits"] >= want, (name, fig["max_block_bits"])
        elif key == "nblk":
            assert len(blocks) == want and info["gray"], (name, len(blocks))
        elif key == "min_blocks":
            assert len(blocks) >= want, (name, len(blocks))
        elif key == "dummy_at_wg_start":
            assert any(locate(i, it["w"], it["h"], False)[3] for i in range(WG_BLOCKS, len(blocks), WG_BLOCKS)), name
        elif key == "y00_after_dummy_at_wg_start":
            assert any(i % 6 == 0 and locate(dc_predecessor(i, False), it["w"], it["h"], False)[3]
                       for i in range(WG_BLOCKS, len(blocks), WG_BLOCKS)), name
            assert (it["w"] + 7) // 8 % 2 == 1 and (it["h"] + 7) // 8 % 2 == 1, name
        else:
            raise AssertionError("unknown fact %s of %s" % (key, name))
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# how the constants above were found (minutes of oracle encodes; not run by any test)
# ---------------------------------------------------------------------------------------------------------------------
def _first_ffs(orc, it):
    data = oracle_file(orc, dict(it))
    return None if data is None else packed_stream(data)[1]


def search_ff(orc, target):
    """FF_SINGLE: the alternating run's first 0xFF at packed offset `target`"""
    for npair in range(4):
        base = (8 * target - 22 * npair) // FLAT_BITS
        for nflat in range(max(0, base - 12), base + 1):
            FF_SINGLE["search"] = (npair, nflat, 12)
            ff = _first_ffs(orc, _ff_single("search", [], []))
            if ff is not None and ff.size and ff[0] == target:
                return npair, nflat, 12


def search_pair(orc, target):
    """FF_PAIR: 0xFF at `target` and `target + 1`"""
    for u in (128, 129, 130, 132, 136):
        for v0 in range(10, 60):
            for amp in (14, 20):
                for nflat in range(max(0, 8 * target // FLAT_BITS - 16), 8 * target // FLAT_BITS + 1):
                    FF_PAIR["search"] = (nflat, u, v0, v0 + 192, amp)
                    ff = _first_ffs(orc, _ff_pair("search", []))
                    if ff is not None and {target, target + 1} <= set(ff.tolist()):
                        return FF_PAIR["search"]


def search_long_block(orc, seeds=3000):
    """LONG_BLOCK: hill climbing over single-sample flips of 0 / 255 patterns, by the size of the one-block file"""
    def size(x):
        y = (np.unpackbits(np.frombuffer(int(x).to_bytes(8, "big"), np.uint8)).reshape(8, 8) * 255).astype(np.uint8)
        return len(orc.jpeg_encode("orc", np.ascontiguousarray(y), None, 8, 8, 100))
    rng, best = np.random.RandomState(1), (0, 0)
    for _ in range(seeds):
        x = int.from_bytes(rng.bytes(8), "big")
        cur, improved = size(x), True
        while improved:
            improved = False
            for k in rng.permutation(64):
                s = size(x ^ (1 << int(k)))
                if s > cur:
                    x, cur, improved = x ^ (1 << int(k)), s, True
        best = max(best, (cur, x))
    return hex(best[1])
