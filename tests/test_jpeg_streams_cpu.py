"""CPU: the constructed JPEG streams of tests/jpeg_stream_cases.py.  For every case: the facts it exists for hold in the file that
was produced, the CPU restatement of the decoder (oracle/jpeg_oracle.c) reads it, and -- where the image's libjpeg harness builds --
libjpeg returns the same planes byte for byte (only that comparison is skipped without it).  The device decoder is held to the same
planes in tests/test_gpu_jpeg_streams.py.

Also here: the writer refuses tables that are no prefix code or hold the all-ones code; the IDCT's range limit is libjpeg's
range_limit[x & 1023] and not a clamp (the `range_limit_*` cases differ from libjpeg in hundreds of bytes with a clamp); the
magnitude up to which 32-bit intermediates cannot overflow, derived from the constants; and the legal maximum (quantiser 255 under
coefficients of 1023), where 32 bits do overflow and the restatement's 64-bit passes still give libjpeg's bytes."""
import numpy as np
import pytest

from tests import jpeg_stream_cases as K


def _libjpeg(orc):
    return orc.load_libjpeg()


# the facts every case must show: name -> list of (key, predicate)
def _ge(n):
    return lambda v: v >= n


def _eq(x):
    return lambda v: v == x


_STUFF = [("ff_share", _ge(0.2)), ("ff_at_chunk_end", _ge(1))]
EXPECT = {
    "no_sync_gray": [("nsub", _ge(600)), ("nsub", lambda v: v < 641), ("symbols_per_block", _eq(64.0)), ("symbol_bits", _eq(([10], [11]))),
                     ("runs_of_eight_ones", _eq(0)), ("guess_true", _eq(0)), ("first_pass_true", _eq(0))],
    "no_sync_420": [("nsub", _ge(257)), ("nsub", lambda v: v < 1923), ("symbols_per_block", _eq(64.0)), ("symbol_bits", _eq(([10], [11]))),
                    ("runs_of_eight_ones", _eq(0)), ("guess_true", _eq(0)), ("first_pass_true", _eq(0))],
    "deep_codes_gray": [("max_symbol_bits", _eq(27)), ("has_27_bit_dc", _eq(True)), ("has_26_bit_ac", _eq(True)), ("long_crossing_sub_end", _ge(1)),
                        ("long_at_sub_start", _ge(1)), ("last_symbol_bits", _ge(26)), ("share_of_codes_over_11_bits", _ge(0.5)),
                        ("code_lengths_used", lambda v: {12, 13, 14, 15, 16} <= set(v))],
    "pairs": [("blocks_full_at_63", _ge(16)), ("zrl_symbols", _ge(16)), ("pair_split_by_sub_end", _ge(1)), ("max_symbol_bits", _eq(3))],
    "flat_one_bit_gray": [("bits_per_block", _eq(2.0)), ("blocks", _eq(4096)), ("blocks_per_sub", _eq(256)), ("nsub", _eq(16))],
    "flat_one_bit_420": [("bits_per_block", _eq(2.0)), ("blocks", _eq(1536)), ("blocks_per_sub", _eq(256))],
    "flat_one_bit_rst1": [("intervals", _eq(256)), ("bits_per_block", _eq(2.0))],
    "flat_one_bit_rst7": [("intervals", _eq(586)), ("bits_per_block", _eq(2.0))],
    "stuffing_edges_long": _STUFF + [("scan_bytes", _eq(65535)), ("ff_at_group_end", _ge(1)), ("group_base_mod4", _eq([0, 1, 2, 3]))],
    "stuffing_edges_len_k64": _STUFF + [("scan_bytes", _eq(2560))],
    "stuffing_edges_len_k64_1": _STUFF + [("scan_bytes", _eq(2561))],
    "stuffing_edges_len_16384": _STUFF + [("scan_bytes", _eq(16384))],
    "stuffing_edges_len_16385": _STUFF + [("scan_bytes", _eq(16385))],
    "stuffing_edges_len_32767": _STUFF + [("scan_bytes", _eq(32767))],
    "stuffing_edges_rst_chunk": _STUFF + [("marker_at_chunk_end", _ge(1)), ("intervals", _eq(9))],
    "stuffing_edges_rst_group": _STUFF + [("marker_at_group_end", _ge(1)), ("scan_bytes", _ge(32769))],
    "dc_extremes": [("blocks", _ge(4097)), ("blocks_mod_256", lambda v: v != 0), ("dc_differences_of_category_11", _eq(4160)), ("intervals", _eq(1))],
    "dc_extremes_rst": [("restart_mod_256", lambda v: v != 0), ("intervals", _eq(42)), ("dc_differences_of_category_11", _eq(4160))],
    "range_limit_gray": [("bands", lambda v: min(v) >= 100), ("edges", lambda v: min(v) >= 64), ("max_dequantised", lambda v: v <= 32767)],
    "range_limit_420": [("bands", lambda v: min(v) >= 100), ("edges", lambda v: min(v) >= 64), ("max_dequantised", lambda v: v <= 32767)],
    "range_limit_wide": [("bands", lambda v: min(v) >= 100), ("max_dequantised", lambda v: 32768 <= v <= 35081)],
    "range_limit_max": [("bands", lambda v: v[0] >= 100 and v[4] >= 100), ("max_dequantised", _eq(2047 * 255))],
}
EXPECT["deep_codes_420"] = EXPECT["deep_codes_gray"]


def test_every_case_states_its_facts():
    assert set(EXPECT) == set(K.CASES)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_case_facts_and_planes(orc, name):
    data, facts = K.case(name)
    for key, holds in EXPECT[name]:
        assert holds(facts[key]), (name, key, facts[key])
    st, want, w, h, gray = orc.jpeg_decode("orc", data)
    assert st > 0 and want is not None, (name, st)
    assert st == (w * h if gray else w * h + 2 * (w * h // 4))
    if _libjpeg(orc) is None:
        return          # (the facts and the restatement's decode are checked; only the comparison with libjpeg needs its harness)
    st2, lj, w2, h2, gray2 = orc.jpeg_decode("lj", data)
    assert st2 == st and (w2, h2, gray2) == (w, h, gray), (name, st2)
    assert np.array_equal(want, lj), (name, int((want != lj).sum()))


def test_the_interval_alignments_and_output_alignments_are_all_reached():
    """over the restart variants of `stuffing_edges`: intervals that begin 1, 2 and 3 bytes past a word of the bit string (the
    unaligned branch of stage_bits); over all its variants: workgroups whose output starts at each of the four alignments"""
    starts, bases = set(), set()
    for name in K.CASES:
        if name.startswith("stuffing_edges"):
            f = K.case(name)[1]
            starts |= set(f["interval_start_mod4"])
            bases |= set(f["group_base_mod4"])
    assert {1, 2, 3} <= starts and bases == {0, 1, 2, 3}


def test_writer_refuses_bad_tables():
    with pytest.raises(ValueError):
        K.huff_codes([2, 1] + [0] * 14, [0, 1, 2])            # three codes where two 1-bit codes leave no room
    with pytest.raises(ValueError):
        K.huff_codes([1, 1, 2] + [0] * 13, [0, 1, 2, 3])      # complete: its last code is 111
    with pytest.raises(ValueError):
        K.huff_codes([2] + [0] * 15, [0, 1])                  # the 1-bit code 1
    with pytest.raises(ValueError):
        K.huff_codes([1] + [0] * 15, [0, 1])                  # counts and values disagree
    assert K.huff_codes([1, 1, 1] + [0] * 13, [5, 6, 7]) == {5: (0, 1), 6: (2, 2), 7: (6, 3)}
    with pytest.raises(KeyError):                              # a coefficient the table has no symbol for
        K.write_jpeg(np.full((1, 64), 3), 8, 8, "gray", np.ones(64, int), {"dc0": K._ONE_DC, "ac0": K._ONE_AC})


def test_writer_and_oracle_round_trip_with_standard_tables(orc):
    """the writer against the restatement's ENCODER: the coefficients orc_jpeg_coefficients computes for an image, written with the
    tables of Annex K, decode to the planes of the restatement's own file"""
    rng = np.random.RandomState(7)
    w, h = 48, 32
    y = rng.randint(0, 256, (h, w)).astype(np.uint8)
    theirs = orc.jpeg_encode("orc", np.ascontiguousarray(y), None, w, h, 90)
    coef = orc.jpeg_coefficients(np.ascontiguousarray(y), None, w, h, 90)
    coef = np.asarray(coef).reshape(-1, 64).astype(np.int64)
    # DC and AC tables of the restatement's own file
    tables, q, pos = {}, None, 2
    while theirs[pos + 1] != 0xDA:
        n = int.from_bytes(theirs[pos + 2:pos + 4], "big")
        seg = theirs[pos + 4:pos + 2 + n]
        if theirs[pos + 1] == 0xC4:
            o = 0
            while o < len(seg):
                cnt = sum(seg[o + 1:o + 17])
                tables[("ac" if seg[o] >> 4 else "dc") + str(seg[o] & 15)] = (list(seg[o + 1:o + 17]), list(seg[o + 17:o + 17 + cnt]))
                o += 17 + cnt
        if theirs[pos + 1] == 0xDB and q is None:
            q = np.array(list(seg[1:65]))
        pos += 2 + n
    # orc_jpeg_coefficients returns natural order with the DC value in [0]; the writer wants zigzag
    mine = K.write_jpeg(coef[:, K.ZIGZAG], w, h, "gray", q, {"dc0": tables["dc0"], "ac0": tables["ac0"]})
    a, b = orc.jpeg_decode("orc", mine), orc.jpeg_decode("orc", theirs)
    assert a[0] > 0 and np.array_equal(a[1], b[1])


def test_range_limit_is_libjpegs_table_not_a_clamp(orc):
    """orc_jpeg_idct on blocks that are one DC coefficient (quantiser 4: every sample is x = (4 dc + 4) >> 3 in front of the range
    limit): libjpeg's range_limit[x & 1023] -- the clamp of x + 128 inside -512..511, wrapped outside, so x = 600 is 0 and not 255"""
    import ctypes as C
    lib = orc.load()
    lib.orc_jpeg_idct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_jpeg_idct.restype = None
    quant = np.full(64, 4, np.uint16)
    for dc, x, sample in ((1200, 600, 0), (-1200, -600, 255), (1021, 511, 255), (1023, 512, 0), (-1025, -512, 0), (-1026, -513, 255),
                          (0, 0, 128), (254, 127, 255), (-256, -128, 0), (-200, -100, 28), (1500, 750, 0), (1151, 576, 0), (-1153, -576, 255)):
        assert (4 * dc + 4) >> 3 == x
        i = x & 1023
        assert sample == (i + 128 if i < 128 else 255 if i < 512 else 0 if i < 896 else i - 896)
        coef = np.zeros(64, np.int16)
        coef[0] = dc
        out = np.zeros(64, np.uint8)
        lib.orc_jpeg_idct(coef.ctypes.data, quant.ctypes.data, out.ctypes.data)
        assert set(out.tolist()) == {sample}, (dc, x, sample, out[:4])


def test_int32_domain_of_the_idct_is_what_the_decoder_states():
    """the bound in uhdr_jpeg_dec.hip ("dequantisation + IDCT") and DESIGN.md, derived here from the constants: the largest sum of
    absolute weights a pass gives its 8 inputs is 61214, so a first pass in 32 bits cannot overflow up to a dequantised magnitude
    of 35081; the decoder takes 64 bits from 32768 on"""
    eye = np.eye(8, dtype=np.int64)
    v = [eye[k] for k in range(8)]
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (v[0] + v[4]) * 8192, (v[0] - v[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    y1, y2, y3, y4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (y3 + y4) * 9633
    y3, y4 = y3 * -16069 + z5, y4 * -3196 + z5
    y1, y2 = y1 * -7373, y2 * -20995
    parts = [z1, tmp2, tmp3, tmp0, tmp1, tmp10, tmp13, tmp11, tmp12, z5, y1, y2, y3, y4, t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299]
    t0, t1, t2, t3 = t0 * 2446 + y1 + y3, t1 * 16819 + y2 + y4, t2 * 25172 + y2 + y3, t3 * 12299 + y1 + y4
    outs = [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]
    weight = max(int(np.abs(x).sum()) for x in parts + [t0, t1, t2, t3] + outs)
    assert weight == 61214
    assert weight * 35081 + (1 << 10) < (1 << 31) <= weight * 35082 + (1 << 10)
    assert 32768 <= 35081      # the decoder's switch to 64 bits lies inside the safe range


def test_legal_maximum_needs_more_than_32_bits_in_the_first_pass(orc):
    """range_limit_max: quantisers of 255 under full blocks of +-1023.  A first pass in 32 bits wraps there (checked with numpy's
    int32), the restatement's 64-bit passes give libjpeg's planes"""
    data, facts = K.case("range_limit_max")
    assert facts["max_dequantised"] > 35081
    st, want, w, h, gray = orc.jpeg_decode("orc", data)
    assert st == w * h
    if _libjpeg(orc) is not None:
        lj = orc.jpeg_decode("lj", data)[1]
        assert np.array_equal(want, lj), int((want != lj).sum())
    # 61214 x 1023 x 255 alone is past 2^31
    assert 61214 * 1023 * 255 > (1 << 31)
