"""GPU: the JPEG/R decode batches in one round and in a round per file.

Every call holds 6 to 8 files: 4:2:0 primaries of 17x9, 45x37 and 130x70 with one-component and three-component maps, a 4:4:4 and a
4:2:2 primary of 130x70 (UHDR_HIP_DECODE_ANY_SAMPLING), the 1280x720 sample file, a file whose entropy-coded data is corrupt, a file
that is a size probe (NULL destination) and, in the SDR calls, the odd-sized 4:2:0 files, whose RGBA is refused.  Each of the four
batch entry points runs in both memory spaces, for UHDR_HIP_OUTPUT_SDR and UHDR_HIP_OUTPUT_HDR_HLG (EXACT), the scaled call at 1/1 and
1/2, once with the default byte bound of a codec round (one round) and once with the bound at 4 KiB (uhdr_hip_codec_round_bytes_probe:
every file in a round of its own).  Statuses are asserted as listed, so they are equal in both runs.

Expected bytes, bit for bit, none of them from the library under test:
  SDR: Pillow's (libjpeg-turbo's) RGB of the primary image, at 1/2 its scaled decode, with alpha 255;
  HLG, 4:2:0 primary and one-component map: oracle/jpegr_oracle.decode of the file, the odd-sized primaries (17x9, 45x37) included: the
    reference decodes them into a zeroed buffer and reads Cr shifted, and so does this library (DESIGN.md section 7.3.1;
    tests/test_gpu_odd420_decode.py runs them behind a dirtied pool);
  HLG, 4:2:0 primary and three-component map (g17, g45, and g68: 68x36 over the 17x9 golden): the oracle's applyGainMap per channel
    (tests/rgbmap_cases.composite_apply) over the oracle's decode of the primary image in the reference's buffer and Pillow's RGB of the map;
  HLG, 4:4:4 / 4:2:2 primary (libjpeg's planes from tests/golden/sampling), and at 1/2 every file whose scaled size is even and whose map
    stays whole (the sample, r136, and g68 with its three-component map; Pillow's scaled planes): the same applyGainMap over one 4:2:0
    image per chroma phase, as tests/test_gpu_jpeg_scaled.py does it.
One kind of file has no such reference, and gets a seam check only -- the run with a round per file must give the bytes of the run with
one round, which says nothing about either run being right: the files at 1/2 in HLG whose scaled size is odd (the phase images cannot
carry it) or whose map is scaled too.  They are pinned piecewise in tests/test_gpu_jpeg_scaled.py.
The call with a round per file also checks that the hook held: restoring the default returns the bound that was set.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

from tests import rgbmap_cases as R
from tests.jpeg_scaled_cases import JPEGR_MD, gray_jpeg, pillow_jpeg, pillow_scaled, pillow_scaled_rgba
from tests.sampling_cases import fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = 3.4028234663852886e38
HOOK = "uhdr_hip_codec_round_bytes_probe"
TINY = 4096      # bytes: below what the smallest file holds of a round, so every file gets a round of its own
ENTRIES = ("uhdr_hip_jpegr_decode_batch", "uhdr_hip_jpegr_decode_batch_ex", "uhdr_hip_jpegr_decode_rgbmap_batch", "uhdr_hip_jpegr_decode_md_batch",
           "uhdr_hip_jpegr_decode_scaled_batch")


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


# ---- files ----------------------------------------------------------------------------------------------------------------------------
class F:
    """one file of a call: kind 'good' / 'corrupt' / 'probe'; primary sampling (hs, vs); rgb: a three-component map"""
    def __init__(self, name, data, primary, gmap, w, h, hs, vs, rgb=False, kind="good", planes=None):
        self.name, self.data, self.primary, self.gmap, self.w, self.h, self.hs, self.vs, self.rgb, self.kind, self.planes = (
            name, data, primary, gmap, w, h, hs, vs, rgb, kind, planes)

    def as_kind(self, kind, data=None):
        return F(self.name + "_" + kind, data or self.data, self.primary, self.gmap, self.w, self.h, self.hs, self.vs, self.rgb, kind, self.planes)


_FILES = {}


def _files(hip):
    if _FILES:
        return _FILES
    from oracle import jpegr_oracle as J

    def made(name, primary, gmap, w, h, hs=2, vs=2, rgb=False, planes=None):
        data = J.append_gainmap(primary, gmap, JPEGR_MD)
        assert isinstance(data, bytes)
        _FILES[name] = F(name, data, primary, gmap, w, h, hs, vs, rgb, planes=planes)
    made("r130", pillow_jpeg(130, 70, 31, subsampling=2), gray_jpeg(65, 35, 41, quality=85), 130, 70)
    made("r17", pillow_jpeg(17, 9, 32, subsampling=2), gray_jpeg(17, 9, 42, quality=85), 17, 9)
    made("r45", pillow_jpeg(45, 37, 33, subsampling=2), gray_jpeg(45, 37, 43, quality=85), 45, 37)
    made("g17", pillow_jpeg(17, 9, 34, subsampling=2), R.golden_jpeg(17, 9, 85), 17, 9, rgb=True)
    made("g45", pillow_jpeg(45, 37, 35, subsampling=2), R.golden_jpeg(45, 37, 85), 45, 37, rgb=True)
    made("g68", pillow_jpeg(68, 36, 36, subsampling=2), R.golden_jpeg(17, 9, 85), 68, 36, rgb=True)      # even-sized, factor 4: whole at 1/2 too
    made("r136", pillow_jpeg(136, 72, 37, subsampling=2), gray_jpeg(34, 18, 45, quality=85), 136, 72)
    for name, fx in (("r444", "s11_base_130x70"), ("r422", "s21_base_130x70")):
        hs, vs, w, h, data, planes = fixture(fx)
        made(name, data, gray_jpeg(65, 35, 44, quality=85), w, h, hs, vs, planes=planes)
    sample = open(os.path.join(ROOT, "tests", "golden", "sample_jpegr.jpeg"), "rb").read()
    imgs = J.find_images(sample)
    _FILES["sample"] = F("sample", sample, sample[imgs[0][0]:imgs[0][0] + imgs[0][1]], sample[imgs[1][0]:imgs[1][0] + imgs[1][1]], 1280, 720, 2, 2)
    _FILES["probe"] = _FILES["r130"].as_kind("probe")
    _FILES["corrupt"] = _corrupt(hip, _FILES["r130"])
    return _FILES


def _corrupt(hip, f):
    """f with the primary image's scan cut short by an EOI: the first cut that the device decoder rejects (found with the single call)"""
    from tests.gpu_util import dev_empty, stream_ptr
    lib = hip.load()
    sos = f.primary.find(b"\xff\xda")
    start = sos + 2 + int.from_bytes(f.primary[sos + 2:sos + 4], "big")
    out = dev_empty(hip.output_bytes(hip.OUTPUT_HDR_HLG, f.w, f.h))
    for k in range(1, 12):
        cut = start + (len(f.primary) - 2 - start) * k // 12
        from oracle import jpegr_oracle as J
        data = J.append_gainmap(f.primary[:cut] + b"\xff\xd9", f.gmap, JPEGR_MD)
        buf = np.frombuffer(data, np.uint8)
        d = hip.Image()
        rc = lib.uhdr_hip_jpegr_decode(buf.ctypes.data, buf.size, hip.OUTPUT_HDR_HLG, FLT_MAX, C.c_void_p(out.data_ptr()), out.numel(), C.byref(d), None,
                                       hip.APPLY_EXACT, hip.MEM_DEVICE, stream_ptr())
        if rc == hip.ERROR_DECODE_ERROR and (d.width, d.height) == (f.w, f.h):
            return f.as_kind("corrupt", data)
    raise AssertionError("no cut of the entropy-coded data was rejected by the device decoder")


# ---- expected bytes -------------------------------------------------------------------------------------------------------------------
_WANT = {}


def _omd(orc, f):
    """the metadata the file's XMP carries, as oracle/jpegr_oracle.decode reads it (its boost is 10 only to six digits of its log2)"""
    from oracle import jpegr_oracle as J
    imgs = J.find_images(f.data)
    md = J.metadata_from_xmp(J.app_segment(f.data[imgs[1][0]:imgs[1][0] + imgs[1][1]], 0xE1, J.XMP_NS))
    return orc.Metadata(float(md["max"]), float(md["min"]), float(md["gamma"]), float(md["off_sdr"]), float(md["off_hdr"]), float(md["capmin"]), float(md["capmax"]),
                        1 if md["version"] == "1.0" else 0)


def _by_phase(orc, y, cb, cr, hs, vs, gamut, apply):
    """apply (an oracle applyGainMap on a 4:2:0 image) over planes of luma sampling hs x vs: one 4:2:0 image per chroma phase, every pixel
    from its own"""
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0
    out = np.zeros((h, w), np.uint32)
    sy, sx = (1 if vs == 2 else 2), (1 if hs == 2 else 2)
    for dy in range(sy):
        for dx in range(sx):
            img = np.concatenate([y.reshape(-1), cb[dy::sy, dx::sx].reshape(-1), cr[dy::sy, dx::sx].reshape(-1)])
            v = apply(orc.yuv420_image(np.ascontiguousarray(img), w, h, gamut))[:w * h * 4].view(np.uint32).reshape(h, w)
            out[dy::sy, dx::sx] = v[dy::sy, dx::sx]
    return out.reshape(-1).view(np.uint8)


def _want(hip, orc, f, fmt, s):
    """the bytes the call must give for file f, or None where nothing but the library itself could say (the docstring)"""
    key = (f.name, fmt, s)
    if key not in _WANT:
        _WANT[key] = _want_now(hip, orc, f, fmt, s)
    return _WANT[key]


def _want_now(hip, orc, f, fmt, s):
    from PIL import Image

    from oracle import jpegr_oracle as J
    if fmt == hip.OUTPUT_SDR:
        return pillow_scaled_rgba(f.primary, f.w, f.h, s)
    sw, sh = -(-f.w // s), -(-f.h // s)
    mw = Image.open(io.BytesIO(f.gmap)).size[0]
    if s != 1 and ((sw | sh) & 1 or (f.w // mw) % s != 0):
        return None      # (the docstring: at 1/2 the references below need an even size and a map that stays whole)
    if s == 1 and (f.hs, f.vs) == (2, 2) and not f.rgb:
        st, out, w, h, _, _ = J.decode(f.data, fmt, FLT_MAX, threads=2)
        assert st == 0 and (w, h) == (f.w, f.h)
        return out[:hip.output_bytes(fmt, w, h)]
    gamut, omd = J.gamut_from_icc(J.app_segment(f.primary, 0xE2, J.ICC_ID)), _omd(orc, f)
    if f.rgb:      # a three-component map: Pillow's RGB of it, channel by channel
        rgb = np.asarray(Image.open(io.BytesIO(f.gmap)).convert("RGB"))
        apply = lambda yi: R.composite_apply(orc, yi, rgb, omd, fmt, FLT_MAX)      # noqa: E731
    else:
        st, gplane, gw, gh, _ = orc.jpeg_decode("orc", f.gmap)
        assert st > 0
        gmap = np.ascontiguousarray(gplane[:gw * gh].reshape(gh, gw))

        def apply(yi):
            st, o, _ = orc.apply("orc_", yi, gmap, omd, fmt, FLT_MAX, threads=2)
            assert st == 0
            return o
    if s != 1:      # Pillow's scaled planes: 4:4:4 whatever the file's sampling
        ycc = pillow_scaled(f.primary, "YCbCr", f.w, f.h, s)
        return _by_phase(orc, ycc[:, :, 0], ycc[:, :, 1], ycc[:, :, 2], 1, 1, gamut, apply)
    if (f.hs, f.vs) == (2, 2):      # the oracle's decode of the primary image
        st, planes, w, h, gray = orc.jpeg_decode("orc", f.primary)
        assert st > 0 and not gray and (w, h) == (f.w, f.h)
        planes = J.reference_buffer(planes, w, h)      # (an odd size: floor(3 w h / 2) bytes, zero where the decoder writes nothing)
        return apply(orc.yuv420_image(planes, w, h, gamut))[:hip.output_bytes(fmt, w, h)]
    cw, ch = -(-f.w // f.hs), -(-f.h // f.vs)      # 4:4:4 / 4:2:2: libjpeg's planes
    y, cb, cr = f.planes[:f.w * f.h].reshape(f.h, f.w), f.planes[f.w * f.h:f.w * f.h + cw * ch].reshape(ch, cw), f.planes[f.w * f.h + cw * ch:].reshape(ch, cw)
    return _by_phase(orc, y, cb, cr, f.hs, f.vs, gamut, apply)


# ---- one call -------------------------------------------------------------------------------------------------------------------------
def _call(hip, entry, files, fmt, s, device):
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    n = len(files)
    bufs = [np.frombuffer(f.data, np.uint8) for f in files]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    dests, mds, stat = (hip.Image * n)(), (hip.Metadata * n)(), _arr(C.c_int, [7] * n)
    needs = [hip.output_bytes(fmt, -(-f.w // s), -(-f.h // s)) for f in files]
    outs = [dev_empty(k, 0xCD) if device else np.full(k, 0xCD, np.uint8) for k in needs]
    optr = _arr(C.c_void_p, [None if f.kind == "probe" else (o.data_ptr() if device else o.ctypes.data) for f, o in zip(files, outs)])
    tail = {ENTRIES[0]: (), ENTRIES[4]: (hip.DECODE_ANY_SAMPLING, s)}.get(entry, (hip.DECODE_ANY_SAMPLING,))
    rc = getattr(lib, entry)(n, ptrs, sizes, fmt, FLT_MAX, optr, _arr(C.c_size_t, needs), dests, mds, stat, hip.APPLY_EXACT,
                             hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr(), *tail)
    got = [to_host(o, k).copy() if device else o for o, k in zip(outs, needs)]
    return rc, list(stat), got, dests


def _status(hip, f, fmt, s):
    if f.kind == "probe":
        return hip.ERROR_INSUFFICIENT_RESOURCE
    if f.kind == "corrupt":
        return hip.ERROR_DECODE_ERROR
    if fmt == hip.OUTPUT_SDR and s == 1 and (f.hs, f.vs) == (2, 2) and ((f.w | f.h) & 1):
        return hip.ERROR_UNSUPPORTED_FEATURE      # libjpeg-turbo's RGBA of an odd-sized 4:2:0 image is outside the conversion
    return 0


def _names(entry):
    if entry == ENTRIES[0]:      # no flag: 4:2:0 primaries, one-component maps
        return ["r130", "r17", "corrupt", "r45", "probe", "sample"]
    if entry == ENTRIES[1]:      # a three-component map contributes its luma here: left to tests/test_gpu_jpeg_sampling.py
        return ["r444", "r130", "r17", "corrupt", "r45", "probe", "r422", "sample"]
    if entry == ENTRIES[4]:
        return ["r444", "g17", "r136", "corrupt", "g45", "probe", "g68", "r130"]
    return ["r444", "g17", "r130", "corrupt", "g45", "probe", "r422", "g68", "r17"]


@pytest.fixture
def round_bound(hip):
    """sets the byte bound of a codec round; the default is back when the test ends, however it ends"""
    lib = hip.load()

    def set_bound(nbytes):
        if not hasattr(lib, HOOK):
            pytest.skip("this library has no " + HOOK)
        return getattr(lib, HOOK)(nbytes)
    yield set_bound
    if hasattr(lib, HOOK):
        getattr(lib, HOOK)(0)


_ONE_ROUND = {}


def _run_case(hip, orc, entry, device, fmt, s, tiny, round_bound):
    files = [_files(hip)[k] for k in _names(entry)] + ([_files(hip)["sample"]] if entry == ENTRIES[4] and s == 2 else [])
    assert 5 <= len(files) <= 9
    wants = [None if _status(hip, f, fmt, s) != 0 else _want(hip, orc, f, fmt, s) for f in files]
    key = (entry, device, fmt, s)
    if key not in _ONE_ROUND:
        _ONE_ROUND[key] = _call(hip, entry, files, fmt, s, device)
    if tiny:
        round_bound(TINY)
        rc, stat, got, dests = _call(hip, entry, files, fmt, s, device)
        assert round_bound(0) == TINY      # the bound that call ran under
    else:
        rc, stat, got, dests = _ONE_ROUND[key]
    want_stat = [_status(hip, f, fmt, s) for f in files]
    assert stat == want_stat and rc == next(x for x in want_stat if x != 0), (entry, fmt, s, rc, stat)
    for i, f in enumerate(files):
        if want_stat[i] != 0:
            continue
        assert (dests[i].width, dests[i].height) == (-(-f.w // s), -(-f.h // s)), f.name
        if wants[i] is not None:
            assert np.array_equal(got[i], wants[i]), (entry, f.name, fmt, s, int((got[i] != wants[i]).sum()))
        else:
            assert fmt != hip.OUTPUT_SDR and f.name != "sample" and s == 2, f.name      # (the docstring: these alone have no reference)
            assert np.array_equal(got[i], _ONE_ROUND[key][2][i]), (entry, f.name, fmt, s)


@pytest.mark.parametrize("tiny", [False, True], ids=["one_round", "round_per_file"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("entry", ENTRIES[:4], ids=lambda e: e[len("uhdr_hip_jpegr_decode_"):])
def test_batches(hip, orc, round_bound, entry, device, tiny):
    for fmt in (hip.OUTPUT_SDR, hip.OUTPUT_HDR_HLG):
        _run_case(hip, orc, entry, device, fmt, 1, tiny, round_bound)


@pytest.mark.parametrize("tiny", [False, True], ids=["one_round", "round_per_file"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("s", [1, 2])
def test_scaled_batch(hip, orc, round_bound, s, device, tiny):
    for fmt in (hip.OUTPUT_SDR, hip.OUTPUT_HDR_HLG):
        _run_case(hip, orc, ENTRIES[4], device, fmt, s, tiny, round_bound)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("rgba", [False, True], ids=["ycbcr", "rgba"])
def test_jpeg_decode_batch_across_a_byte_bound_seam(hip, round_bound, rgba, device):
    """uhdr_hip_jpeg_decode_batch_ex on five 130x70 fixtures with the bound at 64 KiB.  Each file holds at least 324 blocks of
    coefficients of its round (128 bytes a block: 41 KiB), two of them more than the bound, so every round holds one file and the
    seams lie where no count of files would put them.  YCbCr: libjpeg's planes; RGBA: Pillow's (libjpeg-turbo's) RGB; bit for bit"""
    from tests.gpu_util import dev_empty, stream_ptr, to_host
    lib = hip.load()
    names = ["s11_base_130x70", "s21_base_130x70", "s12_base_130x70", "s11_rst2_130x70", "s21_prog_130x70"]
    fx = [fixture(k) for k in names]
    n = len(fx)
    bufs = [np.frombuffer(f[4], np.uint8) for f in fx]
    ptrs, sizes = _arr(C.c_void_p, [b.ctypes.data for b in bufs]), _arr(C.c_size_t, [b.size for b in bufs])
    wants = []
    for hs, vs, w, h, data, planes in fx:
        wants.append(pillow_scaled_rgba(data, w, h, 1) if rgba else np.asarray(planes))
    needs = [k.size for k in wants]
    round_bound(1 << 16)
    outs = [dev_empty(k, 0xCD) if device else np.full(k, 0xCD, np.uint8) for k in needs]
    optr = _arr(C.c_void_p, [o.data_ptr() if device else o.ctypes.data for o in outs])
    descs, stat = (hip.Image * n)(), _arr(C.c_int, [7] * n)
    rc = lib.uhdr_hip_jpeg_decode_batch_ex(n, ptrs, sizes, hip.DECODE_TO_RGBA if rgba else hip.DECODE_TO_YCBCR, optr, _arr(C.c_size_t, needs), descs, stat,
                                           hip.MEM_DEVICE if device else hip.MEM_HOST, stream_ptr(), hip.DECODE_ANY_SAMPLING)
    assert rc == 0 and list(stat) == [0] * n
    for i in range(n):
        got = to_host(outs[i], needs[i]) if device else outs[i]
        assert np.array_equal(got, wants[i]), (names[i], int((got != wants[i]).sum()))
