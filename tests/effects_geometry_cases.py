"""Shared by tests/test_effects_chain_cpu.py and tests/test_gpu_effects_geometry.py: the shapes at which the index arithmetic of
k_effect, k_effect_rot and k_effect_chain changes character -- more than one block of 4096 columns across, more than two 64 x 64
tiles, more rows than the grid's 65535, the LDS stretch and the tile span at their bounds -- and, for every chain, the class
(uhdr_hip_effect_chain_classes) each output plane must get.  A chain case that the composer moves to another route fails; it is
never skipped.  Expected bytes come from the oracle at run time (tests/effects_chain_cases.py: oracle_run)."""
from tests.effects_chain_cases import crop, mirror, resize, rot

GATHER, ASC, DESC, LDS, TILE = 0, 1, 2, 3, 4

# The LDS class's host bound: over every block of columns c0 .. c1 (4096 at most), |b[c1] - b[c0]| <= 4 * (c1 - c0 + 1).
# For [resize(4100, 2)] of a width W, b[c] = floor(c * W / 4100), and the first block (c0 = 0, c1 = 4095) decides:
#   W = 16400: floor(4095 * 16400 / 4100) = 16380 <= 16384                                   LDS, the ratio of exactly 4
#   W = 16405: floor(4095 * 16405 / 4100) = floor(16384.99...) = 16384 <= 16384              LDS, the widest stretch there is
#   W = 16406: floor(4095 * 16406 / 4100) = floor(16385.99...) = 16385 >  16384              one step steeper: not LDS
# (the second block, columns 4096 .. 4099, spans 12 source bytes against a bound of 16 in all three).
# What 16406 x 2 becomes: its two rows lie 16406 bytes apart, not less than 256, so it is no TILE either and takes the byte gather.
# The same width is TILE where every 64 output rows come from one source row: [resize(4100, 128)] has a[0..63] = 0 and
# a[64..127] = 16406, a span of 0 in both tiles.
LDS_W, LDS_W_MAX, LDS_W_OVER = 16400, 16405, 16406

# The TILE class's bound: |a[last row of a 64-row tile] - a[its first row]| < 256.  [resize(130, 6), rot(90)] of a width W has
# a[i] = floor(i * W / 130): W = 520 gives a[63] = 63 * 4 = 252 (TILE), W = 527 gives 255 (TILE, the last span accepted), W = 533 gives floor(63 * 533 / 130) = floor(258.3) = 258
# (not TILE; its columns lie a source row apart, so no LDS either: GATHER).
TILE_CHAIN = [resize(130, 6), rot(90)]

# (name, width, height, mono, chain, classes of the output planes in the launch's order)
CHAINS = [
    # ASC / DESC, two blocks and a bit across.  Left edge 16: whole 16-byte pieces where the row's address allows it (8200 = 8 mod
    # 16, so every other row; the crop to 8176 columns lines source and destination up on the same rows), left edge 3: never.
    ("asc_mono_16", 8200, 4, True, [crop(16, 8199, 0, 3)], (ASC,)),
    ("asc_mono_3", 8200, 4, True, [crop(3, 8199, 0, 3)], (ASC,)),
    ("asc_yuv_16", 8200, 4, False, [crop(16, 8199, 0, 3)], (ASC, ASC)),
    ("asc_yuv_3", 8200, 4, False, [crop(3, 8196, 0, 3)], (ASC, ASC)),
    ("desc_mono", 8200, 4, True, [mirror(1)], (DESC,)),
    ("desc_yuv", 8200, 4, False, [mirror(1)], (DESC, DESC, DESC)),
    ("desc_half_turn_mono", 8200, 4, True, [rot(180)], (DESC,)),
    ("desc_crop_mono_16", 8200, 4, True, [mirror(1), crop(16, 8191, 0, 3)], (DESC,)),
    ("desc_crop_mono_3", 8200, 4, True, [mirror(1), crop(3, 8199, 0, 3)], (DESC,)),
    ("desc_crop_yuv_16", 8200, 4, False, [mirror(1), crop(16, 8191, 0, 3)], (DESC, DESC)),
    ("desc_crop_yuv_3", 8200, 4, False, [mirror(1), crop(3, 8196, 0, 3)], (DESC, DESC)),
    # widths that are multiples of 16 in luma and chroma: every row of every plane moves as whole 16-byte pieces, reversed ones included
    ("asc_yuv_all_rows", 8224, 4, False, [crop(32, 8223, 0, 3)], (ASC, ASC)),
    ("desc_mono_all_rows", 8208, 4, True, [mirror(1)], (DESC,)),
    ("desc_yuv_all_rows", 8224, 4, False, [mirror(1)], (DESC, DESC, DESC)),
    # LDS: at its bound over a full block, ascending and descending b; cb > 0 (s_lo > 0); an odd left edge
    ("lds_ratio4", LDS_W, 2, True, [resize(4100, 2)], (LDS,)),
    ("lds_ratio4_desc", LDS_W, 2, True, [mirror(1), resize(4100, 2)], (LDS,)),
    ("lds_widest", LDS_W_MAX, 2, True, [resize(4100, 2)], (LDS,)),
    ("lds_widest_desc", LDS_W_MAX, 2, True, [mirror(1), resize(4100, 2)], (LDS,)),
    ("lds_up_mono", 8200, 4, True, [resize(12300, 4)], (LDS,)),
    ("lds_up_yuv", 8200, 4, False, [resize(12300, 4)], (LDS, LDS)),
    ("lds_crop_mono", 8200, 4, True, [crop(3, 8198, 0, 3), resize(4100, 4)], (LDS,)),
    ("lds_crop_yuv", 8200, 4, False, [crop(3, 8198, 0, 3), resize(4100, 6)], (LDS, LDS)),
    ("lds_over_gather", LDS_W_OVER, 2, True, [resize(4100, 2)], (GATHER,)),
    # TILE: span 252 over three tiles down; without a quarter turn (span 0 with 65 tiles across; span 200 in one tile); 129 tiles down
    ("tile_span252", 520, 6, True, TILE_CHAIN, (TILE,)),
    # floor(63 * 527 / 130) = 255, the widest span accepted: with the run's alignment slack it needs the tile row's 65th dword
    ("tile_span255", 527, 6, True, TILE_CHAIN, (TILE,)),
    ("tile_no_turn_wide", LDS_W_OVER, 2, True, [resize(4100, 128)], (TILE,)),
    ("tile_no_turn_span200", 100, 3, True, [resize(10, 3)], (TILE,)),
    ("tile_rot90_mono", 8200, 4, True, [rot(90)], (TILE,)),
    ("tile_rot90_yuv", 8200, 4, False, [rot(90)], (TILE, TILE, TILE)),
    ("tile_rot270_flip_mono", 8200, 4, True, [rot(270), mirror(0)], (TILE,)),
    ("tile_rot270_flip_yuv", 8200, 4, False, [rot(270), mirror(0)], (TILE, TILE, TILE)),
    # GATHER: span 258
    ("gather_span258", 533, 6, True, TILE_CHAIN, (GATHER,)),
    # more rows than the grid has (65535): the row loop's second trip
    ("rows_past_grid", 2, 65600, True, [mirror(0), crop(0, 1, 3, 65599)], (ASC,)),
]

# One call, one chain, jobs of every class and extent: the grid is the maximum over the jobs, so blocks outside a job must return.
# A quarter turn makes the source pitch the column step: 1 (ASC), 3 (LDS: at most 4 source bytes per output byte), thousands (TILE).
MIXED_CHAIN = [rot(270)]
MIXED = [
    # (width, height, mono, classes)
    (1, 5000, True, (ASC,)),                 # 5000 x 1: two blocks across
    (70000, 1, True, (ASC,)),                # 1 x 70000: the row loop's second trip (one column: unit step by default)
    (130, 66, False, (TILE, TILE, TILE)),    # 66 x 130: three tiles down, chroma 33 wide
    (3, 9000, True, (LDS,)),                 # 9000 x 3: three blocks across, b = 3 j
    (1, 1, True, (ASC,)),
]

# ---- single effects (uhdr_hip_crop / mirror / rotate / resize in device memory) ----
# (name, width, height, mono, [(effect name, arguments)], luma stride or 0, source pointer offset)
_WIDE = [("crop", (16, 8199, 0, 2)), ("crop", (5, 8196, 1, 2)), ("mirror", (0,)), ("mirror", (1,)), ("rotate", (90,)), ("rotate", (180,)),
         ("rotate", (270,))]
SINGLES = [
    # blocks 1 and 2 across; 129 rot tiles with a partial last one; reversed 16-byte pieces in block 2; LDS resize with s_lo > 0
    ("wide_mono", 8200, 3, True, _WIDE + [("resize", (12300, 3)), ("resize", (4100, 5))], 0, 0),
    ("wide_yuv", 8200, 4, False, [("crop", (16, 8199, 0, 3)), ("crop", (5, 8196, 0, 1))] + _WIDE[2:] + [("resize", (12300, 4)), ("resize", (4100, 6))], 0, 0),
    # 8208 = 16 * 513: the mirrored 16-byte pieces are aligned on both sides in every row (at 8200 only the half turn of the 4-row image's
    # luma is), blocks 1 and 2 included
    ("wide16_mono", 8208, 3, True, [("mirror", (1,)), ("rotate", (180,)), ("mirror", (0,)), ("crop", (16, 8207, 0, 2))], 0, 0),
    # the LDS stretch at capacity (col_num == 4 * col_den), and one column fewer: the fx_quad fallback
    ("ratio4", 16400, 2, True, [("resize", (4100, 2)), ("resize", (4099, 2))], 0, 0),
    # second trip of the row loop; 1025 rot tiles
    ("tall_mono", 3, 65600, True, [("crop", (0, 2, 2, 65599)), ("mirror", (0,)), ("rotate", (180,)), ("rotate", (90,))], 0, 0),
    ("tall_yuv", 2, 65600, False, [("crop", (0, 1, 2, 65599)), ("mirror", (0,)), ("rotate", (180,)), ("rotate", (90,))], 0, 0),
    # 65000 * 66000 = 4 290 000 000 < 2^32 = 4 294 967 296: LDS route with the largest 32-bit products;
    # 65100 * 66000 = 4 296 600 000 and 66000 * 66000 are over: the guarded fallback
    ("tall_resize", 2, 66000, True, [("resize", (2, 65000)), ("resize", (2, 65100)), ("resize", (4, 66000))], 0, 0),
    # unaligned tile loads, negative tile bases (131 = 3 mod 64, 67 = 3 mod 64), odd chroma width (65 x 33)
    ("rot_unaligned_mono", 131, 67, True, [("rotate", (90,)), ("rotate", (270,))], 137, 1),
    ("rot_odd_chroma_yuv", 130, 66, False, [("rotate", (90,)), ("rotate", (270,))], 0, 0),
]

# tests/test_oracle_pins.py: the restatement against the reference's object code at these shapes
# (width, height, mono, effect name, arguments)
PINS = [
    (8200, 4, False, "crop", (5, 8196, 0, 1)), (8200, 4, False, "mirror", (1,)), (8200, 4, False, "rotate", (90,)), (8200, 4, False, "rotate", (270,)),
    (8200, 4, False, "resize", (12300, 4)), (8200, 4, True, "resize", (4100, 6)),
    (2, 66000, True, "mirror", (0,)), (2, 66000, True, "rotate", (90,)), (2, 66000, True, "rotate", (180,)), (2, 66000, True, "resize", (2, 65000)),
    (16400, 2, True, "resize", (4100, 2)), (16400, 2, True, "resize", (4099, 2)),
    (2, 66000, True, "resize", (4, 66000)), (2, 66000, True, "resize", (2, 65100)),
]
