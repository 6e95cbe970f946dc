"""The host composer behind uhdr_hip_add_effects_batch (uhdr_hip_effect_chain_map; needs no GPU): a chain of effects is one index
map, source offset = A[row] + B[column] per output plane.  The expanded map, applied to the input bytes, must give the oracle's
addEffects result byte for byte, and the descriptor must be the oracle's."""
import ctypes as C

import numpy as np
import pytest

from tests import effects_chain_cases as K


@pytest.fixture(scope="module")
def api():
    from libultrahdr_dev_amd import api as a
    a.load()
    return a


def _map(api, w, h, ls, cs, mono, chain):
    lib = api.load()
    desc, fused, count = api.Image(), C.c_int(-1), C.c_size_t(0)
    arr = K.effect_array(api, chain)
    fmt = api.PIX_FMT_MONOCHROME if mono else api.PIX_FMT_YUV420
    rc = lib.uhdr_hip_effect_chain_map(w, h, ls, cs, fmt, arr, len(chain), C.byref(desc), C.byref(fused), None, 0, C.byref(count))
    if rc != 0:
        return rc, None, None, None
    off = np.zeros(max(count.value, 1), np.uint32)
    rc = lib.uhdr_hip_effect_chain_map(w, h, ls, cs, fmt, arr, len(chain), C.byref(desc), C.byref(fused), C.c_void_p(off.ctypes.data), off.size,
                                       C.byref(count))
    return rc, desc, fused.value, off[:count.value]


def _check(api, orc, w, h, mono, chain, seed, ls=0):
    """-> fused flag; asserts bytes and descriptor against the oracle when fused"""
    src, sls, scs = K.source(w, h, mono, seed, ls=ls or None)
    rc, desc, fused, off = _map(api, w, h, ls, 0, mono, chain)
    if K.has_odd(w, h, mono, chain):
        assert rc == api.ERROR_UNSUPPORTED_FEATURE, (w, h, chain, rc)
        return None
    orc_rc, obuf, odesc, ochroma = K.oracle_run(orc, src, w, h, mono, chain, ls=ls, gamut=-1)
    assert rc == orc_rc == 0, (w, h, mono, chain, rc, orc_rc)
    assert (desc.width, desc.height, desc.colorGamut, desc.pixelFormat, desc.luma_stride, desc.chroma_stride) == odesc, (w, h, mono, chain)
    assert desc.data is None
    assert off.size == K.packed(mono, desc.width, desc.height)
    if ochroma is not None:
        assert ochroma == desc.luma_stride * desc.height
    if fused:
        assert off.max() < src.size
        assert np.array_equal(src[off], obuf[:off.size]), (w, h, mono, chain)
    return fused


def test_named_chains_compose_to_the_oracles_bytes(api, orc):
    for n, (w, h, mono, chain) in enumerate(K.named_chains()):
        fused = _check(api, orc, w, h, mono, chain, 100 + n)
        if fused is not None and (w, h, mono, chain) != K.NON_ADDITIVE:
            assert fused == 1, (w, h, mono, chain)


def test_first_step_reads_a_strided_image(api, orc):
    for n, chain in enumerate(([K.crop(2, 41, 4, 27), K.rot(90)], [K.rot(90), K.mirror(1)], [K.resize(40, 24), K.rot(270)], [K.rot(270)])):
        for mono in (False, True):
            assert _check(api, orc, 48, 40, mono, chain, 300 + n, ls=54) == 1
    # a mirror or half turn of a padded image: the single call's documented deviation
    rc, _, _, _ = _map(api, 48, 40, 54, 0, False, [K.mirror(1)])
    assert rc == api.ERROR_UNSUPPORTED_FEATURE


def test_generated_chains_compose_to_the_oracles_bytes(api, orc):
    chains = K.generated_chains(400)
    not_fused = 0
    for n, (w, h, mono, chain) in enumerate(chains):
        fused = _check(api, orc, w, h, mono, chain, 1000 + n)
        assert fused is not None, (w, h, mono, chain)     # (the generator keeps YUV420 even)
        not_fused += fused == 0
    # a non-fused image is not checked here: the reference composition itself leaves about 0.1 % non-additive
    assert not_fused <= len(chains) * 2 // 100, not_fused


def test_odd_yuv420_intermediate_is_unsupported(api):
    rc, _, _, _ = _map(api, 64, 48, 0, 0, False, [K.crop(0, 32, 0, 47)])
    assert rc == api.ERROR_UNSUPPORTED_FEATURE
    rc, _, _, _ = _map(api, 63, 48, 0, 0, False, [])
    assert rc == api.ERROR_UNSUPPORTED_FEATURE
    rc, _, fused, off = _map(api, 63, 47, 0, 0, True, [K.rot(90)])     # monochrome: any size
    assert rc == 0 and fused == 1 and off.size == 63 * 47
    # the single call's statuses come first
    rc, _, _, _ = _map(api, 64, 48, 0, 0, False, [K.crop(0, 64, 0, 47)])
    assert rc == api.ERROR_INVALID_CROPPING_PARAMETERS
    rc, _, _, _ = _map(api, 64, 48, 0, 0, False, [K.rot(45)])
    assert rc == api.ERROR_INVALID_CROPPING_PARAMETERS
    rc, _, _, _ = _map(api, 64, 48, 0, 0, False, [(7, 0, 0, 0, 0)])
    assert rc == api.ERROR_BAD_PTR


def test_call_level_errors_and_all_failing_batch_need_no_device(api):
    lib = api.load()
    img = api.image_array([api.Image(None, 16, 16, 0, None, 0, 0, api.PIX_FMT_YUV420), api.Image(0x1000, 16, 16, 0, None, 0, 0, api.PIX_FMT_YUV420),
                           api.Image(0x1000, 16, 16, 0, None, 0, 0, api.PIX_FMT_P010), api.Image(0x1000, 16, 16, 0, None, 0, 0, api.PIX_FMT_YUV420),
                           api.Image(0x1000, 16, 15, 0, None, 0, 0, api.PIX_FMT_YUV420)])
    n = 5
    out = (C.c_void_p * n)(0x2000, 0x2000, 0x2000, None, 0x2000)
    cap = (C.c_size_t * n)(4096, 16 * 16 * 3 // 2 - 1, 4096, 0, 4096)
    descs, status = (api.Image * n)(), (C.c_int * n)(*([77] * n))
    fx = K.effect_array(api, [K.crop(0, 16, 0, 7)])
    one = K.effect_array(api, [K.rot(90)])
    B = api.ERROR_BAD_PTR
    assert lib.uhdr_hip_add_effects_batch(-1, img, fx, 1, out, cap, descs, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, None, fx, 1, out, cap, descs, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, img, fx, 1, None, cap, descs, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, img, fx, 1, out, None, descs, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, img, fx, 1, out, cap, None, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, img, fx, -1, out, cap, descs, status, None) == B
    assert lib.uhdr_hip_add_effects_batch(n, img, None, 1, out, cap, descs, status, None) == B
    assert list(status) == [77] * n                     # call-level errors leave it alone
    assert lib.uhdr_hip_add_effects_batch(0, None, None, 0, None, None, None, None, None) == 0
    # every image stops at a check: the statuses are exact and no device is needed (none has been initialised here)
    assert lib.uhdr_hip_add_effects_batch(n, img, one, 1, out, cap, descs, status, None) == B
    assert list(status) == [B, api.ERROR_INSUFFICIENT_RESOURCE, api.ERROR_UNSUPPORTED_FEATURE, api.ERROR_INSUFFICIENT_RESOURCE, api.ERROR_UNSUPPORTED_FEATURE]
    assert lib.uhdr_hip_add_effects_batch(n, img, fx, 1, out, cap, descs, status, None) == B
    assert list(status) == [B] + [api.ERROR_INVALID_CROPPING_PARAMETERS, api.ERROR_UNSUPPORTED_FEATURE, api.ERROR_INVALID_CROPPING_PARAMETERS,
                                  api.ERROR_INVALID_CROPPING_PARAMETERS]
    assert lib.uhdr_hip_add_effects_batch(n, img, one, 1, out, cap, descs, status, None) == B
    assert status[1] == status[3] == api.ERROR_INSUFFICIENT_RESOURCE      # one byte short; the size probe
    assert (descs[3].width, descs[3].height, descs[3].luma_stride, descs[3].chroma_stride, descs[3].data) == (16, 16, 16, 8, None)
    assert descs[1].data == 0x2000 and descs[1].chroma_data == 0x2000 + 256
    # the diagnostic's own
    desc, fused, count = api.Image(), C.c_int(), C.c_size_t()
    assert lib.uhdr_hip_effect_chain_map(16, 16, 0, 0, api.PIX_FMT_YUV420, None, 1, C.byref(desc), C.byref(fused), None, 0, C.byref(count)) == B
    assert lib.uhdr_hip_effect_chain_map(16, 16, 0, 0, api.PIX_FMT_YUV420, one, 1, None, C.byref(fused), None, 0, C.byref(count)) == B


def test_edit_batch_call_level_errors_need_no_device(api):
    lib = api.load()
    one = K.effect_array(api, [K.rot(90)])
    junk = np.frombuffer(b"\xff\xd8\xff\xd9 not a JPEG/R file", np.uint8)
    jp, jn = (C.c_void_p * 2)(junk.ctypes.data, None), (C.c_size_t * 2)(junk.size, 0)
    buf = np.zeros(64, np.uint8)
    out, cap = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data), (C.c_size_t * 2)(64, 64)
    size, status = (C.c_size_t * 2)(), (C.c_int * 2)(77, 77)
    B = api.ERROR_BAD_PTR
    args = lambda **kw: [kw.get("n", 2), kw.get("jp", jp), kw.get("jn", jn), kw.get("fx", one), kw.get("nfx", 1), kw.get("gfx", one), kw.get("ngfx", 1), None,
                         kw.get("q", 90), kw.get("out", out), kw.get("cap", cap), kw.get("size", size), status, None]
    for bad in (dict(n=-1), dict(jp=None), dict(jn=None), dict(out=None), dict(cap=None), dict(size=None), dict(fx=None), dict(gfx=None), dict(nfx=-1),
                dict(ngfx=-1)):
        assert lib.uhdr_hip_jpegr_edit_batch(*args(**bad)) == B, bad
    assert lib.uhdr_hip_jpegr_edit_batch(*args(q=101)) == api.ERROR_INVALID_QUALITY_FACTOR
    assert lib.uhdr_hip_jpegr_edit_batch(*args(q=-1)) == api.ERROR_INVALID_QUALITY_FACTOR
    assert lib.uhdr_hip_jpegr_edit_batch(*args(q=101, fx=None)) == B            # BAD_PTR first
    assert list(status) == [77, 77]
    # every file stops at a check: no device needed
    rc = lib.uhdr_hip_jpegr_edit_batch(*args())
    assert list(status) == [rc, B] and rc in (api.ERROR_NO_IMAGES_FOUND, api.ERROR_GAIN_MAP_IMAGE_NOT_FOUND)


# ---------------------------------------------------------------------------------------------------
# the class fx_finish picks per output plane (uhdr_hip_effect_chain_classes), both sides of every threshold
# ---------------------------------------------------------------------------------------------------
def _classes(api, w, h, mono, chain, ls=0):
    """-> (status, fused, classes of the output planes)"""
    lib = api.load()
    fused, count, cls = C.c_int(-1), C.c_size_t(99), (C.c_int * 8)(*([-1] * 8))
    rc = lib.uhdr_hip_effect_chain_classes(w, h, ls, 0, api.PIX_FMT_MONOCHROME if mono else api.PIX_FMT_YUV420, K.effect_array(api, chain), len(chain),
                                           C.byref(fused), cls, 8, C.byref(count))
    return rc, fused.value, tuple(cls[:count.value]) if rc == 0 else None


def test_classes_unit_step_columns(api):
    A = api
    assert _classes(api, 64, 40, True, [K.crop(3, 50, 2, 30)]) == (0, 1, (A.FXC_ASC,))
    assert _classes(api, 64, 40, False, [K.crop(2, 51, 2, 31)]) == (0, 1, (A.FXC_ASC, A.FXC_ASC))          # luma, the stacked U|V plane
    assert _classes(api, 64, 40, True, [K.mirror(0)]) == (0, 1, (A.FXC_ASC,))                               # rows reversed, columns as they lie
    assert _classes(api, 64, 40, True, [K.mirror(1)]) == (0, 1, (A.FXC_DESC,))
    assert _classes(api, 64, 40, False, [K.mirror(1)]) == (0, 1, (A.FXC_DESC,) * 3)                         # luma, U, V
    assert _classes(api, 64, 40, True, [K.rot(180)]) == (0, 1, (A.FXC_DESC,))
    assert _classes(api, 64, 40, False, [K.rot(180)])[2][0] == A.FXC_DESC
    assert _classes(api, 64, 40, True, [K.mirror(1), K.mirror(1)]) == (0, 1, (A.FXC_ASC,))
    assert _classes(api, 64, 40, True, [K.resize(64, 20)]) == (0, 1, (A.FXC_ASC,))                          # the width kept: b[j] = j
    assert _classes(api, 7, 5, True, [K.resize(1, 5)]) == (0, 1, (A.FXC_ASC,))                              # one column: no step to judge


def test_classes_lds_bound(api):
    """|b[c1] - b[c0]| <= 4 * (c1 - c0 + 1) per block of 4096 columns; the arithmetic is in tests/effects_geometry_cases.py"""
    A = api
    from tests import effects_geometry_cases as G
    assert _classes(api, 16400, 2, True, [K.resize(4100, 2)]) == (0, 1, (A.FXC_LDS,))                       # the ratio of exactly 4
    assert _classes(api, 16400, 2, True, [K.mirror(1), K.resize(4100, 2)]) == (0, 1, (A.FXC_LDS,))          # descending b
    _, _, _, off = _map(api, 16400, 2, 0, 0, True, [K.mirror(1), K.resize(4100, 2)])
    assert (np.diff(off[:4100].astype(np.int64)) <= 0).all() and off[0] - off[4095] == 16380
    for w in range(16396, 16412):          # floor(4095 * w / 4100) <= 16384 up to 16405
        for chain in ([K.resize(4100, 2)], [K.mirror(1), K.resize(4100, 2)]):
            # two rows 16 KiB apart: no tile either
            assert _classes(api, w, 2, True, chain) == (0, 1, (A.FXC_LDS if 4095 * w // 4100 <= 16384 else A.FXC_GATHER,)), (w, chain)
    assert 4095 * G.LDS_W_MAX // 4100 == 16384 and 4095 * G.LDS_W_OVER // 4100 == 16385 and G.LDS_W_OVER == G.LDS_W_MAX + 1
    # the bound holds per block, not over the row: 4097 columns whose first 4096 are fine and whose last block (one column) is trivially so
    assert _classes(api, 16388, 1, True, [K.resize(4097, 1)]) == (0, 1, (A.FXC_LDS,))
    # not LDS, but every 64 rows read one source row: TILE without a quarter turn
    assert _classes(api, G.LDS_W_OVER, 2, True, [K.resize(4100, 128)]) == (0, 1, (A.FXC_TILE,))
    # rows less than 256 bytes apart: 3 rows of 100 bytes span 200, 3 rows of 128 bytes span 256
    assert _classes(api, 100, 3, True, [K.resize(10, 3)]) == (0, 1, (A.FXC_TILE,))
    assert _classes(api, 128, 3, True, [K.resize(10, 3)]) == (0, 1, (A.FXC_GATHER,))
    assert _classes(api, 128, 2, True, [K.resize(10, 2)]) == (0, 1, (A.FXC_TILE,))                          # span 128


def test_classes_tile_bound(api):
    """|a[i0 + 63] - a[i0]| < 256 per tile of 64 rows: a span of 252 is a tile, 258 is not; 255 and 256 lie between"""
    A = api
    assert _classes(api, 520, 6, True, [K.resize(130, 6), K.rot(90)]) == (0, 1, (A.FXC_TILE,))              # 63 * 4 = 252
    assert _classes(api, 533, 6, True, [K.resize(130, 6), K.rot(90)]) == (0, 1, (A.FXC_GATHER,))            # floor(63 * 533 / 130) = 258
    for w in range(518, 536):              # a[63] = floor(63 * w / 130); the later tiles span no more than the first
        want = A.FXC_TILE if max((min(i0 + 63, 129) * w // 130) - (i0 * w // 130) for i0 in (0, 64, 128)) < 256 else A.FXC_GATHER
        assert _classes(api, w, 6, True, [K.resize(130, 6), K.rot(90)]) == (0, 1, (want,)), w
    assert 63 * 527 // 130 == 255 and 63 * 529 // 130 == 256
    assert _classes(api, 64, 40, True, [K.rot(90)]) == (0, 1, (A.FXC_TILE,))
    assert _classes(api, 64, 40, False, [K.rot(270)]) == (0, 1, (A.FXC_TILE,) * 3)


def test_classes_report_not_fused_where_the_map_does(api):
    B = api.ERROR_BAD_PTR
    lib = api.load()
    w, h, mono, chain = K.NON_ADDITIVE
    assert _map(api, w, h, 0, 0, mono, chain)[2] == 0
    assert _classes(api, w, h, mono, chain) == (0, 0, ())
    assert _classes(api, 40, 24, False, []) == (0, 1, ())                  # no effects: a copy, no plane job
    for n, (w, h, mono, chain) in enumerate(K.named_chains() + K.generated_chains(100)):
        rc, _, fused, _ = _map(api, w, h, 0, 0, mono, chain)
        got = _classes(api, w, h, mono, chain)
        assert got[0] == rc, (w, h, mono, chain)
        if rc == 0:
            assert got[1] == fused and (len(got[2]) > 0) == bool(fused and chain), (w, h, mono, chain)
    assert _classes(api, 48, 40, False, [K.mirror(1)], ls=54)[0] == api.ERROR_UNSUPPORTED_FEATURE
    assert _classes(api, 48, 40, True, [K.rot(90)], ls=54) == (0, 1, (api.FXC_TILE,))
    fused, count = C.c_int(), C.c_size_t()
    one = K.effect_array(api, [K.rot(90)])
    assert lib.uhdr_hip_effect_chain_classes(16, 16, 0, 0, api.PIX_FMT_YUV420, None, 1, C.byref(fused), None, 0, C.byref(count)) == B
    assert lib.uhdr_hip_effect_chain_classes(16, 16, 0, 0, api.PIX_FMT_YUV420, one, 1, None, None, 0, C.byref(count)) == B
    assert lib.uhdr_hip_effect_chain_classes(16, 16, 0, 0, api.PIX_FMT_YUV420, one, 1, C.byref(fused), None, 0, None) == B
    # classes == NULL or too short: the count alone
    assert lib.uhdr_hip_effect_chain_classes(16, 16, 0, 0, api.PIX_FMT_YUV420, one, 1, C.byref(fused), None, 0, C.byref(count)) == 0
    assert (fused.value, count.value) == (1, 3)
    two = (C.c_int * 3)(-7, -7, -7)
    assert lib.uhdr_hip_effect_chain_classes(16, 16, 0, 0, api.PIX_FMT_YUV420, one, 1, C.byref(fused), two, 2, C.byref(count)) == 0
    assert list(two) == [api.FXC_TILE, api.FXC_TILE, -7] and count.value == 3


def test_geometry_chains_compose_to_the_oracles_bytes_in_their_declared_class(api, orc):
    """every chain tests/test_gpu_effects_geometry.py launches: the map's bytes are the oracle's and the route is the declared one"""
    from tests import effects_geometry_cases as G
    assert (G.GATHER, G.ASC, G.DESC, G.LDS, G.TILE) == (api.FXC_GATHER, api.FXC_ASC, api.FXC_DESC, api.FXC_LDS, api.FXC_TILE)
    cases = [(name, w, h, mono, chain, cls) for name, w, h, mono, chain, cls in G.CHAINS]
    cases += [("mixed %dx%d" % (w, h), w, h, mono, G.MIXED_CHAIN, cls) for w, h, mono, cls in G.MIXED]
    for n, (name, w, h, mono, chain, cls) in enumerate(cases):
        assert _check(api, orc, w, h, mono, chain, 2000 + n) == 1, name
        assert _classes(api, w, h, mono, chain) == (0, 1, cls), name
    assert {c for case in cases for c in case[5]} == {G.GATHER, G.ASC, G.DESC, G.LDS, G.TILE}
