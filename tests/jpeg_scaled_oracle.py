"""A numpy int64 restatement of libjpeg-turbo's scaled decode (scale_num / scale_denom = 1/2, 1/4, 1/8): jdmaster.c's size rule,
jidctred.c's 4x4 and 2x2 and jidctint.c's 1x1 inverse DCTs, the planes a decoder assembles from a coefficient array in scan order,
jdsample.c's upsampling of 4:2:2 / 4:4:0 results and jdcolor.c's colour conversion.  tests/test_jpeg_scaled_cpu.py pins it to Pillow
(libjpeg-turbo); the GPU tests compare the device decoder with it.

A small baseline reader (Huffman, restart intervals, any of the samplings the decoder accepts) supplies the coefficient arrays of
files an encoder wrote, so that the restatement also stands where Pillow cannot be asked (images smaller than the denominator)."""
import numpy as np

from tests.jpeg_stream_cases import ZIGZAG, idct_reference

FORMAT_OF = {(1, 1): "YUV444", (2, 1): "YUV422", (1, 2): "YUV440", (2, 2): "YUV420"}


def ceil_div(a, b):
    return -(-a // b)


# ---- sizes (jdmaster.c, jpeg_calc_output_dimensions / jpeg_core_output_dimensions) --------------------------------------------------
def idct_sizes(hs, vs, gray, s):
    """IDCT size per component: N = 8 / s, doubled while below 8 and both sampling ratios allow it"""
    n = 8 // s
    if gray:
        return [n]
    out = []
    for h_samp, v_samp in ((hs, vs), (1, 1), (1, 1)):
        size = n
        while size < 8 and (hs * n) % (h_samp * size * 2) == 0 and (vs * n) % (v_samp * size * 2) == 0:
            size *= 2
        out.append(size)
    return out


def geometry(w, h, hs, vs, gray, s):
    """-> (ow, oh, format name, idct sizes, [(plane width, plane height)])"""
    sizes = idct_sizes(hs, vs, gray, s)
    ow, oh = ceil_div(w, s), ceil_div(h, s)
    if gray:
        return ow, oh, "MONOCHROME", sizes, [(ow, oh)]
    samp = [(hs, vs), (1, 1), (1, 1)]
    dims = [(ceil_div(w * samp[c][0] * sizes[c], hs * 8), ceil_div(h * samp[c][1] * sizes[c], vs * 8)) for c in range(3)]
    n = 8 // s
    ehs, evs = hs * n // sizes[1], vs * n // sizes[1]   # the sampling of the result
    assert dims[0] == (ow, oh) and dims[1] == (ceil_div(ow, ehs), ceil_div(oh, evs))
    return ow, oh, FORMAT_OF[(ehs, evs)], sizes, dims


# ---- the reduced inverse DCTs -------------------------------------------------------------------------------------------------------
def _ds(x, n):
    return (x + (1 << (n - 1))) >> n


def range_limit(x):
    i = x & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def _one_d_4(v, shift):   # v[..., k], k = 0..7 (k = 4 unused) -> [..., 4]
    t0 = v[..., 0] << 14
    t2 = v[..., 2] * 15137 - v[..., 6] * 6270
    o0 = -v[..., 7] * 1730 + v[..., 5] * 11893 - v[..., 3] * 17799 + v[..., 1] * 8697
    o2 = -v[..., 7] * 4176 - v[..., 5] * 4926 + v[..., 3] * 7373 + v[..., 1] * 20995
    return np.stack([_ds(t0 + t2 + o2, shift), _ds(t0 - t2 + o0, shift), _ds(t0 - t2 - o0, shift), _ds(t0 + t2 - o2, shift)], -1)


def _one_d_2(v, shift):
    t = v[..., 0] << 15
    o = -v[..., 7] * 5906 + v[..., 5] * 6967 - v[..., 3] * 10426 + v[..., 1] * 29692
    return np.stack([_ds(t + o, shift), _ds(t - o, shift)], -1)


def idct_scaled(coef_zigzag, quant_zigzag, size):
    """(blocks, 64) quantised coefficients and quantisers, zigzag order -> (blocks, size, size) samples"""
    coef_zigzag = np.asarray(coef_zigzag, np.int64).reshape(-1, 64)
    if size == 8:
        return idct_reference(coef_zigzag, quant_zigzag)[1]
    d = np.zeros((len(coef_zigzag), 64), np.int64)
    d[:, ZIGZAG] = coef_zigzag * np.asarray(quant_zigzag, np.int64)
    d = d.reshape(-1, 8, 8)   # [block, row, column]
    if size == 1:
        return range_limit(_ds(d[:, 0, 0], 3)).reshape(-1, 1, 1)
    one_d, s1, s2 = (_one_d_4, 12, 19) if size == 4 else (_one_d_2, 13, 20)
    ws = one_d(d.transpose(0, 2, 1), s1)       # pass 1 runs down the columns: ws[block, column, output row]
    ws = ws.transpose(0, 2, 1)                 # [block, output row, column]
    return range_limit(one_d(ws, s2))          # pass 2 along the rows (column 4, and for 2x2 the even ones, are not read)


# ---- planes from coefficients in scan order -----------------------------------------------------------------------------------------
def block_positions(w, h, hs, vs, gray):
    """[(component, block row, block column)] in scan order: MCU by MCU, hs x vs luma blocks in rows, then Cb, Cr"""
    if gray:
        bw, bh = ceil_div(w, 8), ceil_div(h, 8)
        return [(0, r, c) for r in range(bh) for c in range(bw)]
    mx, my = ceil_div(w, 8 * hs), ceil_div(h, 8 * vs)
    out = []
    for mr in range(my):
        for mc in range(mx):
            out += [(0, mr * vs + k // hs, mc * hs + k % hs) for k in range(hs * vs)]
            out += [(1, mr, mc), (2, mr, mc)]
    return out


def planes(coef, quant, w, h, hs, vs, gray, s):
    """coef: (blocks, 64) in scan order, DC as its VALUE; quant: per component, zigzag.  -> the component planes of a decode at 1/s"""
    ow, oh, fmt, sizes, dims = geometry(w, h, hs, vs, gray, s)
    pos = block_positions(w, h, hs, vs, gray)
    coef = np.asarray(coef, np.int64).reshape(len(pos), 64)
    comp = np.array([p[0] for p in pos])
    out = []
    for c, (pw, ph) in enumerate(dims):
        size = sizes[c]
        idx = np.nonzero(comp == c)[0]
        smp = idct_scaled(coef[idx], np.asarray(quant[c], np.int64), size)
        rows = max(pos[i][1] for i in idx) + 1
        cols = max(pos[i][2] for i in idx) + 1
        full = np.zeros((rows * size, cols * size), np.uint8)
        for k, i in enumerate(idx):
            _, br, bc = pos[i]
            full[br * size:(br + 1) * size, bc * size:(bc + 1) * size] = smp[k]
        out.append(np.ascontiguousarray(full[:ph, :pw]))
    return out


def packed(pl):
    return np.concatenate([p.reshape(-1) for p in pl])


# ---- upsampling and colour conversion (jdsample.c, jdcolor.c) -----------------------------------------------------------------------
def _h2v1(c, ow, fancy):
    c = c.astype(np.int64)
    if not fancy or c.shape[1] <= 2:   # jinit_upsampler: fancy only for rows of more than two samples
        return np.repeat(c, 2, axis=1)[:, :ow]
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0] = c[:, 0]
    out[:, -1] = c[:, -1]
    return out[:, :ow]


def _h1v2(c, oh, fancy):
    c = c.astype(np.int64)
    if not fancy:
        return np.repeat(c, 2, axis=0)[:oh]
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    out[0::2] = (3 * c + up + 1) >> 2
    out[1::2] = (3 * c + down + 2) >> 2
    return out[:oh]


def rgb(pl, fmt, fancy=True):
    """the planes of `geometry` -> (oh, ow, 3) RGB as libjpeg-turbo converts them; fancy: do_fancy_upsampling and an IDCT size above 1"""
    y = pl[0].astype(np.int64)
    oh, ow = y.shape
    cb, cr = pl[1], pl[2]
    if fmt == "YUV422":
        cb, cr = _h2v1(cb, ow, fancy), _h2v1(cr, ow, fancy)
    elif fmt == "YUV440":
        cb, cr = _h1v2(cb, oh, fancy), _h1v2(cr, oh, fancy)
    else:
        assert fmt == "YUV444"
    cb, cr = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def rgba(pl, fmt, fancy=True):
    x = rgb(pl, fmt, fancy)
    return np.concatenate([x, np.full(x.shape[:2] + (1,), 255, np.uint8)], 2).reshape(-1)


# ---- a baseline reader: the coefficients of a file an encoder wrote -----------------------------------------------------------------
def _huff_lookup(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def read_baseline(data):
    """-> dict(w, h, gray, hs, vs, quant=[per component, zigzag], coef=(blocks, 64) zigzag with DC values, scan order,
    dht={(class << 4) | id: (bits, vals)})"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    p, qt, ht, dht, dri, frame = 2, {}, {}, {}, 0, None
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        n = int.from_bytes(data[p + 2:p + 4], "big")
        seg = data[p + 4:p + 2 + n]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                qt[seg[q] & 15] = np.frombuffer(seg[q + 1:q + 65], np.uint8).astype(np.int64)
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                nv = sum(bits)
                ht[seg[q]] = _huff_lookup(bits, list(seg[q + 17:q + 17 + nv]))
                dht[seg[q]] = (bits, list(seg[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xC0 or m == 0xC1:
            h, w, nc = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
        elif m == 0xDD:
            dri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            ns = seg[0]
            sel = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            p += 2 + n
            break
        else:
            assert m not in (0xC2, 0xC9, 0xCA), "not a baseline file"
        p += 2 + n
    gray = len(frame) == 1
    hs, vs = (1, 1) if gray else (frame[0][1], frame[0][2])
    assert gray or all(f[1] == 1 and f[2] == 1 for f in frame[1:])
    # the entropy-coded segment: intervals of unstuffed bytes
    intervals, cur = [], bytearray()
    while True:
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
            continue
        nb = data[p + 1]
        if nb == 0:
            cur.append(0xFF)
        elif 0xD0 <= nb <= 0xD7:
            intervals.append(bytes(cur))
            cur = bytearray()
        elif nb == 0xFF:
            p += 1
            continue
        else:
            intervals.append(bytes(cur))
            break
        p += 2
    pos = block_positions(w, h, hs, vs, gray)
    bpm = 1 if gray else hs * vs + 2
    coef = np.zeros((len(pos), 64), np.int64)
    b = 0
    for iv in intervals:
        bitstr = "".join(format(x, "08b") for x in iv) + "1" * 32
        at, pred = 0, [0, 0, 0]

        def sym(table):
            nonlocal at
            code = 0
            for length in range(1, 17):
                code = (code << 1) | (bitstr[at + length - 1] == "1")
                if (length, code) in table:
                    at += length
                    return table[(length, code)]
            raise ValueError("no code")

        def value(cat):
            nonlocal at
            if cat == 0:
                return 0
            v = int(bitstr[at:at + cat], 2)
            at += cat
            return v if v >> (cat - 1) else v - (1 << cat) + 1

        nblocks = (dri if dri else len(pos) // bpm) * bpm
        for _ in range(min(nblocks, len(pos) - b)):
            c = pos[b][0]
            td, ta = sel[c]
            pred[c] += value(sym(ht[td]))
            coef[b, 0] = pred[c]
            k = 1
            while k < 64:
                rs = sym(ht[0x10 | ta])
                r, sz = rs >> 4, rs & 15
                if sz == 0:
                    if r != 15:
                        break
                    k += 16
                    continue
                k += r
                coef[b, k] = value(sz)
                k += 1
            b += 1
    assert b == len(pos), (b, len(pos))
    return dict(w=w, h=h, gray=gray, hs=hs, vs=vs, quant=[qt[f[3]] for f in frame], coef=coef, dht=dht)


def transposed_file(data):
    """The baseline file `data` mirrored at its diagonal, losslessly: every block's coefficients, the quantisers and the block grid
    transposed, width / height and the sampling factors swapped, the file's own Huffman tables (which must be complete ones, such as
    Annex K's).  A 4:2:2 file becomes the 4:4:0 file of the transposed image -- the sampling Pillow does not write."""
    from tests import jpeg_stream_cases as K
    f = read_baseline(data)
    w, h, hs, vs, gray = f["h"], f["w"], f["vs"], f["hs"], f["gray"]
    old = {p: i for i, p in enumerate(block_positions(f["w"], f["h"], f["hs"], f["vs"], gray))}
    pos = block_positions(w, h, hs, vs, gray)
    coef = np.stack([_transpose_block(f["coef"][old[(c, bc, br)]]) for c, br, bc in pos])
    quant = [_transpose_block(q) for q in f["quant"]]
    tables = f["dht"]
    out = bytearray(b"\xff\xd8")
    for k, q in enumerate(quant[:2]):
        out += K._segment(0xDB, bytes([k]) + bytes(int(x) for x in q))
    comps = [(1, 0x11, 0)] if gray else [(1, (hs << 4) | vs, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += K._segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)]) + b"".join(bytes(c) for c in comps))
    for key in sorted(tables):
        out += K._segment(0xC4, bytes([key]) + bytes(tables[key][0]) + bytes(tables[key][1]))
    out += K._segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], 0x00 if c[2] == 0 else 0x11]) for c in comps) + bytes([0, 63, 0]))
    codes = {key: K.huff_codes(*t) for key, t in tables.items()}
    enc = K.ScanEncoder()
    pred = [0, 0, 0]
    for b, (c, _, _) in enumerate(pos):
        t = 0 if c == 0 else 1
        pred[c] = enc.block(coef[b], pred[c], codes[t], codes[0x10 | t])
    enc.pad()
    out += enc.out
    return bytes(out + b"\xff\xd9")


def _transpose_block(z):
    """64 values in zigzag order -> the transposed block's, in zigzag order"""
    nat = np.zeros(64, np.int64)
    nat[ZIGZAG] = z
    return nat.reshape(8, 8).T.reshape(-1)[ZIGZAG]


def decode_scaled(data, s):
    """a baseline file at 1/s -> (ow, oh, format name, planes)"""
    f = read_baseline(data)
    ow, oh, fmt, _, _ = geometry(f["w"], f["h"], f["hs"], f["vs"], f["gray"], s)
    return ow, oh, fmt, planes(f["coef"], f["quant"], f["w"], f["h"], f["hs"], f["vs"], f["gray"], s)
