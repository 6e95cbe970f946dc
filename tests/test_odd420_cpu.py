"""CPU tests (no GPU) behind tests/test_gpu_odd420_apply.py and tests/test_gpu_odd420_decode.py: the oracle's applyGainMap equals the
reference's object code (oracle/_ref) on every odd-sized 4:2:0 case of tests/odd420_cases.py, the facts about the reference's reads
that the GPU tests lean on hold for every case, the list reaches what it is there for, and oracle/jpegr_oracle.decode gives one answer
for every file case."""
import numpy as np
import pytest

from tests import odd420_cases as D

POISON = (0x5B, 0xFF)      # two values: a byte that matters changes the output under at least one of them


@pytest.mark.parametrize("name", D.NAMES)
def test_oracle_equals_reference_object_code(orc, name):
    """all four output formats, the display boost uncapped and capped below maxContentBoost; the plain and the LUT pipeline"""
    if orc.load_ref() is None:
        pytest.skip("oracle/_ref not built (needs the reference's sources)")
    case, buf = D.BY_NAME[name], D.buffer(name)
    for fmt in D.FORMATS:
        for boost in (D.FLT_MAX, D.CAPPED):
            for lut in (False, True):
                a = D.apply_of(case, buf, "orc_", fmt, boost, lut)
                b = D.apply_of(case, buf, "ref_", fmt, boost, lut)
                assert a.size == D.BPP[fmt] * case.w * case.h
                assert np.array_equal(a, b), (name, fmt, boost, lut, int((a != b).sum()))


def _changes(case, layout, lo, hi, fmt=2, tail=0):
    """whether applyGainMap's bytes change when bytes [lo, hi) of the case's buffer in `layout` (lengthened by `tail` zero bytes) are
    poisoned"""
    base = np.concatenate([D.buffer(case.name, layout), np.zeros(tail, np.uint8)])
    want = D.apply_of(case, base, "orc_", fmt, layout=layout)
    changed = False
    for v in POISON:
        buf = base.copy()
        buf[lo:hi] = v
        changed |= not np.array_equal(D.apply_of(case, buf, "orc_", fmt, layout=layout), want)
    return changed


@pytest.mark.parametrize("name", D.NAMES)
def test_what_the_reference_reads(orc, name):
    """The facts of the reference's layout, for every case: nothing behind floor(3 w h / 2) bytes is read; the gap between Cb's end and
    Cr's start is, wherever it is not empty (so garbage there shows); the byte at `need` is read by exactly the cases marked so.  The
    same by arithmetic on getYuv420Pixel's offsets, and the first fact for the case's own layout too"""
    case = D.BY_NAME[name]
    w, h = case.w, case.h
    end, need = w * h * 3 // 2, D.need(case)
    assert D.extent(case, "ref") == end and end - need in (0, 1)
    offs = np.concatenate([o.reshape(-1) for o in D.read_offsets(case, "ref")])
    assert not _changes(case, "ref", end, end + 64, tail=64) and offs.max() < end
    g0, g1 = D.gap(case)
    assert g1 - g0 == w * h // 4 - (w // 2) * (h // 2)
    if g1 > g0:
        assert _changes(case, "ref", g0, g1) and ((offs >= g0) & (offs < g1)).any()
    else:
        assert name == "f1_2x3"
    assert case.reads_need == bool((offs == need).any())
    if need < end:
        assert _changes(case, "ref", need, need + 1) == case.reads_need
    else:      # the byte at `need` lies behind the reference's buffer
        assert not case.reads_need
    assert case.reads_need == (w % 4 == 2 and h % 2 == 1)
    # the case's own layout: its buffer ends where the reference stops reading
    own = D.extent(case)
    assert D.buffer(name).size == own and not _changes(case, case.layout, own, own + 64, tail=64)
    assert max(int(o.max()) for o in D.read_offsets(case)) < own
    if case.layout == "strided":      # the row padding is read: the last column's chroma sample, the last row's rows
        assert _changes(case, "strided", own - 1, own)


def test_the_list_has_what_it_is_there_for():
    cases = D.CASES
    assert all(c.w == D.factor(c) * c.mw and c.h == D.factor(c) * c.mh for c in cases)      # applyGainMap's own checks
    assert all(c.w >= 2 and c.h >= 2 and (c.w | c.h) & 1 for c in cases)
    assert all(c.w * c.h <= 512 * 258 for c in cases)                                        # every GPU case stays small
    assert {(c.w // 2) % 2 for c in cases if c.w % 2} == {0, 1}                              # both parities of w / 2 ...
    assert (D.BY_NAME["f1_17x9"].w // 2, D.BY_NAME["f3_63x45"].w // 2) == (8, 31)            # ... 17 -> 8, 63 -> 31
    assert any(c.w > 256 and c.w % 2 for c in cases) and any(c.w > 512 for c in cases)
    assert any(c.w % 2 and not c.h % 2 for c in cases) and any(c.h % 2 and not c.w % 2 for c in cases) and any(c.w % 2 and c.h % 2 for c in cases)
    assert {D.factor(c) for c in cases} == {1, 3, 5, 7}
    assert any((c.mw, c.mh) == (1, 1) for c in cases)
    assert {c.layout for c in cases} == {"ref", "tight", "strided"}
    assert [c.name for c in cases if c.layout == "strided"] == ["f3_63x45"]
    assert sorted(c.name for c in cases if c.reads_need) == ["f1_18x9", "f1_2x3", "f1_518x3"]
    ls, cs = D.strides(D.BY_NAME["f3_63x45"])
    assert ls > 63 and cs > 31
    for names in (D.CAPPED_NAMES, D.RGB_NAMES, D.MD_NAMES):
        assert set(names) <= set(D.NAMES)
    # (size, map size, gap) of the reference's layout, as measured on the oracle
    table = {(17, 9): 6, (45, 35): 19, (63, 45): 26, (49, 35): 20, (259, 301): 139, (17, 8): 2, (16, 9): 4, (3, 3): 1, (18, 9): 4, (518, 3): 129, (2, 3): 0}
    assert {(c.w, c.h): D.gap(c)[1] - D.gap(c)[0] for c in cases} == table


def test_buffers_and_maps():
    for c in D.CASES:
        buf, w, h, cw, ch = D.buffer(c.name), c.w, c.h, c.w // 2, c.h // 2
        assert not buf.flags.writeable and buf is D.buffer(c.name)
        if c.layout == "strided":
            continue
        cr = w * h + (w * h // 4 if c.layout == "ref" else cw * ch)
        zero = np.ones(buf.size, bool)
        zero[:w * h + cw * ch] = False
        zero[cr:cr + cw * ch] = False
        assert not buf[zero].any() and buf.size == w * h * 3 // 2
        if w * h >= 100:      # noise in all three planes
            assert len(np.unique(buf[:w * h])) > 30 and len(np.unique(buf[w * h:w * h + cw * ch])) > 10 and len(np.unique(buf[cr:cr + cw * ch])) > 10
        m = D.gain_map(c.name)
        assert m.shape == (c.mh, c.mw) and (m.size < 2 or (m.min() == 0 and m.max() == 255))
    a = D.expected("f1_17x9", 2)
    assert a is D.expected("f1_17x9", 2) and not a.flags.writeable
    assert not np.array_equal(a, D.expected("f1_17x9", 2, D.CAPPED)) and not np.array_equal(a, D.expected("f1_17x9", 2, lut=True))


@pytest.mark.parametrize("name", D.FILE_NAMES)
def test_jpegr_oracle_decode_gives_one_answer(orc, name):
    """oracle/jpegr_oracle.decode of every file case, twice: status 0 and equal bytes, all four HDR formats; the primary image decodes
    into the reference's layout with zeros where the decoder writes nothing"""
    from oracle import jpegr_oracle as J
    f = D.files()[name]
    for fmt in D.FORMATS:
        if f.rgb:      # a three-component map is outside the restatement's decoder: the per-channel composite stands in, twice as well
            assert J.decode(f.data, fmt, D.FLT_MAX, threads=2)[0] == -20002
            a, b = D.file_expected.__wrapped__(name, fmt), D.file_expected.__wrapped__(name, fmt)
            assert a is not b and np.array_equal(a, b) and len(np.unique(a)) > 8
            continue
        a = J.decode(f.data, fmt, D.FLT_MAX, threads=2)
        b = J.decode(f.data, fmt, D.FLT_MAX, threads=2)
        assert a[0] == 0 and b[0] == 0 and (a[2], a[3]) == (f.w, f.h)
        assert np.array_equal(a[1], b[1]) and len(np.unique(a[1][:D.BPP[fmt] * f.w * f.h])) > 8
        assert np.array_equal(a[1][:D.BPP[fmt] * f.w * f.h], D.file_expected(name, fmt))
    buf = D.primary_buffer(name)
    w, h, cw, ch = f.w, f.h, f.w // 2, f.h // 2
    assert buf.size == w * h * 3 // 2
    assert not buf[w * h + cw * ch:w * h + w * h // 4].any() and not buf[w * h + w * h // 4 + cw * ch:].any()
    assert buf[w * h:w * h + cw * ch].any() and buf[w * h + w * h // 4:w * h + w * h // 4 + cw * ch].any()
