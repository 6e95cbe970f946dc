"""No GPU: tests/jpeg_progressive_encode_oracle.py's transcode_progressive() against Pillow's libjpeg-turbo (byte for byte over the
sizes, qualities and contents of tests/jpeg_progressive_encode_cases.py, in a process of Pillow's own), the counter each constructed
image is there for, what the transcoded files decode to, and the argument checks of the three _scans calls."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_progressive_encode_cases as PC
from tests import jpeg_progressive_encode_oracle as PO

# Pillow in a process of its own.  encode: keys <form>_..._<quality>, form L / 420 / 422 / 444 -> <key>_base, <key>_prog.
# decode: every array is a file -> its pixels
_PIL_SCRIPT = r"""
import io, sys, numpy as np
from PIL import Image, ImageFile
ImageFile.MAXBLOCK = 1 << 22
d = np.load(sys.argv[2]); out = {}
for key in d.files:
    if sys.argv[1] == "decode":
        out[key] = np.asarray(Image.open(io.BytesIO(d[key].tobytes())))
        continue
    form, q = key.split("_")[0], int(key.split("_")[-1])
    kw = {} if form == "L" else {"subsampling": {"444": 0, "422": 1, "420": 2}[form]}
    for name, prog in (("base", False), ("prog", True)):
        b = io.BytesIO()
        Image.fromarray(d[key], "L" if form == "L" else "RGB").save(b, "JPEG", quality=q, progressive=prog, **kw)
        out[key + "_" + name] = np.frombuffer(b.getvalue(), np.uint8)
np.savez(sys.argv[3], **out)
"""


def _pillow(mode, arrays, tmp):
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("Pillow not installed")
    np.savez(tmp / ("in_%s.npz" % mode), **arrays)
    subprocess.check_call([sys.executable, "-c", _PIL_SCRIPT, mode, str(tmp / ("in_%s.npz" % mode)), str(tmp / ("out_%s.npz" % mode))])
    res = np.load(tmp / ("out_%s.npz" % mode))
    return {k: res[k] for k in res.files}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{key: (baseline file, progressive file, transcoded file, counters)}"""
    arrays, seed = {}, 0
    for w, h in PC.SIZES:
        for kind, q in PC.combos((w, h)):
            for form in ("L", "420", "422", "444"):
                seed += 1
                arrays["%s_%s_%dx%d_%d" % (form, kind, w, h, q)] = PC.content(kind, (h, w) if form == "L" else (h, w, 3), seed)
    for name, (img, q, _) in PC.constructed().items():
        arrays["L_%s_%d" % (name.replace("_", "-"), q)] = img
    tmp = tmp_path_factory.mktemp("pil")
    res = _pillow("encode", arrays, tmp)
    out = {}
    for key in arrays:
        base, prog = res[key + "_base"].tobytes(), res[key + "_prog"].tobytes()
        out[key] = (base, prog) + PO.transcode_progressive(base)
    return out, tmp


def test_transcode_equals_pillow_progressive(files):
    out, _ = files
    assert len(out) > 400
    for key, (base, prog, got, _) in out.items():
        assert base[base.find(b"\xff\xc0") + 1] == 0xC0 and b"\xff\xc2" in prog[:1024]
        assert got == prog, (key, len(got), len(prog), next((i for i in range(min(len(got), len(prog))) if got[i] != prog[i]), -1))


def test_every_constructed_image_fires_its_counter(files):
    out, _ = files
    for name, (img, q, counter) in PC.constructed().items():
        c = out["L_%s_%d" % (name.replace("_", "-"), q)][3]
        if counter is not None:
            assert c[counter] > 0, (name, c)
    # the run flushed one block short of the limit: no flush by the limit anywhere, so the textured block codes a symbol in every AC scan
    assert out["L_long-run-32766_50"][3]["eob_7fff"] == 0
    assert out["L_long-run_50"][3]["eob_7fff"] == out["L_long-run-32767_50"][3]["eob_7fff"] == 4      # once per AC scan
    # 937-bit flushes: three per refinement scan (PC.corr_flushes), with and without the new coefficients behind the first
    assert len(PC.corr_flushes()) == 3 and PC.corr_flushes()[0] % PC.WG == PC.WG - 1
    assert out["L_correction-bits_50"][3]["eob_corr"] == out["L_correction-bits-new_50"][3]["eob_corr"] == 6
    # the matrix: ZRLs in first scans, and MCU padding left out of the AC scans, are met on the way
    assert sum(v[3]["zrl_first"] for v in out.values()) > 0
    # (per luma AC scan, of which there are four: 24x8 has 8 luma blocks in its MCUs and 3 in its grid, 40x24 24 and 15, 17x8 at 4:2:2 4 and 3)
    assert out["420_noise_24x8_50"][3]["padding_skipped"] == 4 * 5 and out["420_noise_40x24_50"][3]["padding_skipped"] == 4 * 9
    assert out["422_noise_17x8_50"][3]["padding_skipped"] == 4 * 1 and out["L_noise_17x9_50"][3]["padding_skipped"] == 0


def test_pillow_decodes_the_transcoded_files_to_the_baseline_pixels(files):
    out, tmp = files
    keys = sorted(out)
    arrays = {}
    for k in keys:
        arrays["b_" + k] = np.frombuffer(out[k][0], np.uint8)
        arrays["t_" + k] = np.frombuffer(out[k][2], np.uint8)
    px = _pillow("decode", arrays, tmp)
    for k in keys:
        assert np.array_equal(px["b_" + k], px["t_" + k]), k


def test_the_host_decoder_reads_the_baseline_coefficients(files):
    from libultrahdr_dev_amd import api
    lib = api.load()
    out, _ = files
    n = 0
    for key, (base, _, got, _) in out.items():
        form = key.split("_")[0]
        if form not in ("L", "420") or "long-run" in key:   # (what the decoder reads of progressive files; the long runs: a second for each)
            continue
        w, h, comps, grids, mx, my = PO.coefficients(base)
        pad = []
        if form == "L":
            want = [grids[0][r][c] for r in range(my) for c in range(mx)]
        else:
            want = []
            zero = [0] * 64
            for m in range(mx * my):
                mr, mc = divmod(m, mx)
                for k in range(4):   # blocks of the MCU padding carry nothing of the image: left out, as tests/test_jpeg_progressive.py does
                    r, c = 2 * mr + (k >> 1), 2 * mc + (k & 1)
                    real = r < (h + 7) // 8 and c < (w + 7) // 8
                    if not real:
                        pad.append(len(want))
                    want.append(grids[0][r][c] if real else zero)
                want += [grids[1][mr][mc], grids[2][mr][mc]]
        want = np.array(want, np.int16)
        buf = np.frombuffer(got, np.uint8)
        have = np.zeros(want.size, np.int16)
        nb, gw, gh, gg = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
        rc = lib.uhdr_hip_jpeg_progressive_coefficients(C.c_void_p(buf.ctypes.data), buf.size, C.c_void_p(have.ctypes.data), want.shape[0], C.byref(nb),
                                                        C.byref(gw), C.byref(gh), C.byref(gg))
        assert rc == 0 and nb.value == want.shape[0] and (gw.value, gh.value) == (w, h), key
        have = have.reshape(want.shape)
        have[pad] = 0
        assert np.array_equal(have, want), key
        n += 1
    assert n > 150


# ---- the argument checks of the three calls, with n = -1 as tests/test_jpeg_restart_cpu.py makes them --------------------------------------
@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _all_three(api, opts, mode):
    lib = api.load()
    o = None if opts is None else C.byref(opts)
    return [lib.uhdr_hip_jpeg_encode_planes_batch_scans(-1, None, None, None, None, None, None, None, None, o, mode, api.MEM_HOST, None),
            lib.uhdr_hip_jpeg_encode_rgba_batch_scans(-1, None, None, None, None, None, None, None, None, api.PIX_FMT_YUV422, o, mode, api.MEM_HOST, None),
            lib.uhdr_hip_jpegr_encode_batch_scans(-1, None, None, api.TF_HLG, 90, None, None, None, None, None, None, o, mode, api.MEM_HOST, None)]


def test_bad_scan_modes_and_progressive_with_restart_are_refused_before_the_pointers(api):
    bad = [api.ERROR_UNSUPPORTED_FEATURE] * 3
    for mode in (2, 3, -1, 1 << 20):
        for o in (None, api.encode_opts(), api.encode_opts(1)):
            assert _all_three(api, o, mode) == bad, mode
    for o in (api.encode_opts(0, 1, 0), api.encode_opts(0, 0, 1), api.encode_opts(1, 65535, 0), api.encode_opts(1, 5, 2)):
        assert _all_three(api, o, api.SCANS_PROGRESSIVE) == bad
    # the options' own refusals come first and are the _opts calls'
    o = api.encode_opts()
    o.struct_size = 12
    for mode in (0, 1, 2):
        assert _all_three(api, o, mode) == bad
    assert _all_three(api, api.encode_opts(2), api.SCANS_PROGRESSIVE) == bad


def test_good_modes_reach_the_pointer_checks(api):
    ptr = [api.ERROR_BAD_PTR] * 3
    for mode in (api.SCANS_BASELINE, api.SCANS_PROGRESSIVE):
        for o in (None, api.encode_opts(), api.encode_opts(1)):
            assert _all_three(api, o, mode) == ptr, mode
    for o in (api.encode_opts(0, 7, 0), api.encode_opts(1, 0, 3)):   # restart intervals are the baseline mode's
        assert _all_three(api, o, api.SCANS_BASELINE) == ptr
    assert (api.SCANS_BASELINE, api.SCANS_PROGRESSIVE) == (0, 1)
