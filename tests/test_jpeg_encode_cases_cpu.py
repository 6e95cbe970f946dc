"""CPU tests (no GPU) of tests/jpeg_encode_cases.py: every constructed image has, in the file the CPU checker writes for it, the
property it was built for; the stream reader and the block walker agree with the checker on the content corpus; the constants the
cases mirror are the encoder's; and the quantiser's reciprocal division is exact over its whole domain."""
import os
import re

import numpy as np
import pytest

from tests import jpeg_encode_cases as J
from tests.jpeg_stream_cases import ZIGZAG
from tests.test_jpeg_oracle import SIZES, _content, _planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libultrahdr_dev_amd", "csrc")


@pytest.mark.parametrize("name", list(J.CASES))
def test_case_has_the_property_it_was_built_for(orc, name):
    it = J.case(name)
    fig = J.check_facts(name, it, J.oracle_file(orc, it))
    print(name, it["w"], it["h"], "q%d" % it["q"], it["facts"], fig)


def test_every_case_of_the_issue_is_there():
    want = """len_64k len_64k_p1 len_64k_m1 len_16384 len_16385 len_16383 len_32768 bits_mod8_0 ff_at_63 ff_at_64 ff_at_63_and_64
              ff_at_16383 ff_at_16384 ff_at_16383_and_16384 ff_last_byte ff_last_byte_chunk_end ff_dense ff_none_long six_bit_blocks
              zrl3_no_eob dc_cat11 long_blocks nblk_128 nblk_129 nblk_127 nblk_16385 c420_wg_edge stride_2nd_trip pieces_257""".split()
    assert not [n for n in want if n not in J.CASES]
    assert J.case("zrl3_no_eob_420")["ub"] is not None and J.case("dc_cat11")["ub"] is not None


def test_no_block_of_8_bit_samples_reaches_1400_bits():
    """long_blocks cannot have the 1400 bits one would like: the energy of 64 samples bounds a block at 1154 bits"""
    bound = J.max_block_bits_of_samples()
    assert bound == 1154 and J.LONG_BLOCK_MIN_BITS >= 0.85 * bound


@pytest.mark.parametrize("kind", ["smooth", "noise", "extreme", "flat"])
def test_reader_and_walker_agree_with_the_oracle_on_the_corpus(orc, kind):
    rng = np.random.RandomState(len(kind))
    for w, h in SIZES:
        y, u, v = _content(kind, w, h, rng)
        yb, ub = _planes(y, u, v, w + 2, w // 2 + 1, rng)
        for uv, cs, q in ((ub, w // 2 + 1, 85), (None, 0, 100), (ub, w // 2 + 1, 20)):
            data = orc.jpeg_encode("orc", yb, uv, w, h, q, w + 2, cs)
            info = J.parse_file(data)
            assert (info["w"], info["h"], info["gray"]) == (w, h, uv is None)
            packed, ff = J.packed_stream(data)
            blocks, pad = J.walk_blocks(data)
            assert len(blocks) == J.block_count(w, h, uv is None)
            assert [b[0] for b in blocks] == [0] + list(np.cumsum([b[1] for b in blocks])[:-1])
            assert sum(b[1] for b in blocks) + pad == 8 * packed.size
            assert data[:info["header_len"]] + J.restuff(packed) + b"\xff\xd9" == data
            assert np.array_equal(ff, np.nonzero(packed == 0xFF)[0])
            want = orc.jpeg_coefficients(yb, uv, w, h, q, w + 2, cs)          # natural order
            assert np.array_equal(J.coefficients_of(blocks, uv is None), want[:, ZIGZAG]), (kind, w, h, q)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, "%s: %d matches of %r -- the source moved, look at the cases again" % (what, len(m), pattern)
    return int(m[0])


def test_the_constants_the_cases_mirror_are_the_encoders():
    hip, hdr = _src("uhdr_jpeg.hip"), _src("uhdr_jpeg.h")
    got = {
        "CHUNK": _one(r"constexpr uint32_t kChunk = (\d+);", hip, "kChunk"),
        "PIECE_CHUNKS": _one(r"const uint32_t first = wg \* (\d+)u, t = first \+ threadIdx\.x;", hip, "chunks per stuffing workgroup"),
        "WG_BLOCKS": _one(r"__device__ __forceinline__ void emit_wg\(const Job& j, const uint32_t wg\) \{\n(?:.*\n){2}  const uint32_t i = wg \* (\d+)u \+ threadIdx\.x;",
                          hip, "blocks per emit workgroup"),
        "STUFF_WG_PER_JOB": _one(r"constexpr uint32_t kStuffWgPerJob = (\d+);", hdr, "kStuffWgPerJob"),
        "MAX_BATCH_JOBS": _one(r"constexpr int kMaxBatchJobs = (\d+);", hdr, "kMaxBatchJobs"),
    }
    # one thread per chunk / per block: the launch bounds are the same numbers
    assert _one(r"__launch_bounds__\((\d+)\) k_jpeg_stuff_copy\(", hip, "k_jpeg_stuff_copy") == got["PIECE_CHUNKS"]
    assert _one(r"__launch_bounds__\((\d+)\) k_jpeg_stuff_count\(", hip, "k_jpeg_stuff_count") == got["PIECE_CHUNKS"]
    assert _one(r"__launch_bounds__\((\d+)\) k_jpeg_emit\(", hip, "k_jpeg_emit") == got["WG_BLOCKS"]
    assert _one(r"__launch_bounds__\((\d+)\) k_jpeg_clear_multi\(", hip, "k_jpeg_clear_multi") == got["WG_BLOCKS"]
    assert _one(r"fdct_quant_count_wg\(const Job& j, const uint32_t wg\) \{\n  const uint32_t i = wg \* (\d+)u", hip, "blocks per DCT workgroup") == got["WG_BLOCKS"]
    for name, value in got.items():
        assert getattr(J, name) == value, "%s is %d in the encoder and %d in tests/jpeg_encode_cases.py: stale cases %s" % (
            name, value, getattr(J, name), ", ".join(J.USES[name]))
    assert J.PIECE == J.CHUNK * J.PIECE_CHUNKS


def test_quantiser_reciprocal_division_is_exact():
    """uhdr_jpeg.hip's quantise(): t / (q << 3) as __umulhi(t, floor(2^32 / (q << 3)) + 1) for every 8-bit table entry q and every
    t it can see -- |coefficient| <= 2^14 plus the rounding term (q << 3) >> 1.  The comment there claims it; this checks it."""
    text = _src("uhdr_capi.hip")
    assert len(re.findall(r"\(uint32_t\)\(\(1ull << 32\) / \(\(uint32_t\)j\.q_(?:lum|chr)\[i\] << 3\)\) \+ 1u;", text)) == 2
    assert re.search(r"t \+= qval >> 1;\n  t = \(int\)__umulhi\(\(uint32_t\)t, m\);", _src("uhdr_jpeg.hip"))
    for q in range(1, 256):
        qval = 8 * q
        m = np.uint64((1 << 32) // qval + 1)
        assert int(m) < (1 << 32)
        t = np.arange(0, 16384 + 4 * q + 1, dtype=np.uint64)
        bad = np.nonzero((t * m) >> np.uint64(32) != t // np.uint64(qval))[0]
        assert bad.size == 0, (q, int(t[bad[0]]))
