// shim_tonemap_test.cpp -- the shim's tone-mapping additions, toneMapSdr and JpegRHip::setToneMap, on a synthetic 64x48 PQ ramp
// (BT.2100), checked against the C-ABI calls they stand on.
// usage: shim_tonemap_test
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uhdr_hip.h"
#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
  const size_t w = 64, h = 48;
  std::vector<uint16_t> p010(w * h * 3 / 2);
  for (size_t y = 0; y < h; ++y)
    for (size_t x = 0; x < w; ++x) p010[y * w + x] = (uint16_t)((64 + (x + y) * 700 / (w + h - 2)) << 6);
  for (size_t y = 0; y < h / 2; ++y)
    for (size_t x = 0; x < w / 2; ++x) {
      p010[w * h + y * w + 2 * x] = (uint16_t)((480 + x) << 6);
      p010[w * h + y * w + 2 * x + 1] = (uint16_t)((530 - y) << 6);
    }
  ultrahdr_uncompressed_struct hdr{};
  hdr.data = p010.data(); hdr.width = w; hdr.height = h; hdr.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  hdr.luma_stride = w; hdr.chroma_data = p010.data() + w * h; hdr.chroma_stride = w;
  uhdr_hip_image_t cp{hdr.data, w, h, UHDR_HIP_CG_BT2100, hdr.chroma_data, w, w, UHDR_HIP_PIX_FMT_P010};

  // toneMapSdr: uhdr_hip_tonemap_sdr on host memory
  std::vector<uint8_t> a(w * h * 3 / 2, 0xCD), b(w * h * 3 / 2, 0xCD), c(w * h * 3 / 2, 0xCD);
  auto sdr_of = [&](std::vector<uint8_t>& v) {
    ultrahdr_uncompressed_struct d{};
    d.data = v.data(); d.width = w; d.height = h; d.colorGamut = ULTRAHDR_COLORGAMUT_UNSPECIFIED;
    d.luma_stride = w; d.chroma_data = v.data() + w * h; d.chroma_stride = w / 2; d.pixelFormat = ULTRAHDR_PIX_FMT_YUV420;
    return d;
  };
  ultrahdr_uncompressed_struct da = sdr_of(a), db = sdr_of(b), dc = sdr_of(c);
  float head = -1.0f, chead = -1.0f, given = -1.0f;
  CHECK(toneMapSdr(nullptr, &da, ULTRAHDR_TF_PQ, UHDR_HIP_TONEMAP_REINHARD_MAXRGB) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(toneMapSdr(&hdr, &da, ULTRAHDR_TF_SRGB, UHDR_HIP_TONEMAP_REINHARD_MAXRGB) == ERROR_ULTRAHDR_INVALID_TRANS_FUNC);
  CHECK(toneMapSdr(&hdr, &da, ULTRAHDR_TF_PQ, 9) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(a[0] == 0xCD);
  CHECK(toneMapSdr(&hdr, &da, ULTRAHDR_TF_PQ, UHDR_HIP_TONEMAP_REINHARD_MAXRGB, 0.0f, &head) == ULTRAHDR_NO_ERROR);
  CHECK(da.colorGamut == ULTRAHDR_COLORGAMUT_BT2100 && head > 1.0f && head < 10000.0f / 203.0f);
  uhdr_hip_image_t cb{b.data(), w, h, UHDR_HIP_CG_UNSPECIFIED, b.data() + w * h, w, w / 2, UHDR_HIP_PIX_FMT_YUV420};
  CHECK(uhdr_hip_tonemap_sdr(&cp, &cb, UHDR_HIP_TF_PQ, UHDR_HIP_TONEMAP_REINHARD_MAXRGB, 0.0f, &chead, UHDR_HIP_MEM_HOST, nullptr) == UHDR_HIP_NO_ERROR);
  CHECK(chead == head && a == b);
  float rule = 0.0f;
  CHECK(uhdr_hip_tonemap_headroom(UHDR_HIP_TF_PQ, 0.0f, 1000.0f, &rule) == UHDR_HIP_NO_ERROR);
  CHECK(toneMapSdr(&hdr, &dc, ULTRAHDR_TF_PQ, UHDR_HIP_TONEMAP_REINHARD_MAXRGB, 1000.0f, &given) == ULTRAHDR_NO_ERROR);
  CHECK(given == rule && c != a);
  // TONEMAP_SHIFT is toneMap
  UltraHdrHip uhdr(0);
  CHECK(toneMapSdr(&hdr, &db, ULTRAHDR_TF_PQ, UHDR_HIP_TONEMAP_SHIFT) == ULTRAHDR_NO_ERROR);
  CHECK(uhdr.toneMap(&hdr, &dc) == ULTRAHDR_NO_ERROR);
  CHECK(b == c && b[0] == (uint8_t)(p010[0] >> 8));

  // JpegRHip::setToneMap: the API-0 overload through uhdr_hip_jpegr_encode_api0_tonemapped_batch, SHIFT back to today's file
  JpegRHip codec;
  std::vector<uint8_t> f_shift(w * h * 3 + 65536), f_tone(f_shift.size()), f_back(f_shift.size()), f_c(f_shift.size()), f_both(f_shift.size());
  ultrahdr_compressed_struct j_shift{f_shift.data(), 0, (int)f_shift.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct j_tone{f_tone.data(), 0, (int)f_tone.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct j_back{f_back.data(), 0, (int)f_back.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct j_both{f_both.data(), 0, (int)f_both.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_shift, 90, nullptr) == ULTRAHDR_NO_ERROR);
  for (float peak : {0.0f, 1000.0f}) {
    codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB, peak);
    CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_tone, 90, nullptr) == ULTRAHDR_NO_ERROR);
    void* out = f_c.data();
    size_t cap = f_c.size(), n = 0;
    CHECK(uhdr_hip_jpegr_encode_api0_tonemapped_batch(1, &cp, UHDR_HIP_TF_PQ, 90, nullptr, nullptr, &out, &cap, &n, nullptr, nullptr,
                                                      UHDR_HIP_TONEMAP_REINHARD_MAXRGB, &peak, -1, UHDR_HIP_MEM_HOST, nullptr) == UHDR_HIP_NO_ERROR);
    CHECK((int)n == j_tone.length && memcmp(f_c.data(), f_tone.data(), n) == 0);
    CHECK(j_tone.length != j_shift.length || memcmp(f_tone.data(), f_shift.data(), n) != 0);
    // with the content-adaptive range on top
    codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
    CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_both, 90, nullptr) == ULTRAHDR_NO_ERROR);
    uhdr_hip_metadata_t fmd, parsed;
    CHECK(uhdr_hip_jpegr_encode_api0_tonemapped_batch(1, &cp, UHDR_HIP_TF_PQ, 90, nullptr, nullptr, &out, &cap, &n, &fmd, nullptr,
                                                      UHDR_HIP_TONEMAP_REINHARD_MAXRGB, &peak, UHDR_HIP_BOOST_PER_IMAGE, UHDR_HIP_MEM_HOST,
                                                      nullptr) == UHDR_HIP_NO_ERROR);
    CHECK((int)n == j_both.length && memcmp(f_c.data(), f_both.data(), n) == 0);
    CHECK(uhdr_hip_jpegr_metadata(f_both.data(), j_both.length, &parsed) == UHDR_HIP_NO_ERROR);
    // (the XMP carries the boost as decimal text: equal to a few units of the last place)
    CHECK(std::fabs(parsed.maxContentBoost - fmd.maxContentBoost) <= 1e-5f * fmd.maxContentBoost && fmd.maxContentBoost <= 10000.0f / 203.0f);
    codec.setContentBoost(-1);
    // the file decodes
    std::vector<uint8_t> dec(w * h * 8);
    ultrahdr_uncompressed_struct ddest{};
    ddest.data = dec.data();
    CHECK(codec.decodeJPEGR(&j_tone, &ddest, 3.4028234663852886e38f, nullptr, ULTRAHDR_OUTPUT_HDR_LINEAR, nullptr, nullptr) == ULTRAHDR_NO_ERROR);
    CHECK(ddest.width == w && ddest.height == h);
  }
  codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB, -1.0f);
  CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_tone, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGR(nullptr, ULTRAHDR_TF_PQ, &j_tone, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  codec.setToneMap(7);
  CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_tone, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setToneMap(UHDR_HIP_TONEMAP_SHIFT);
  CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_PQ, &j_back, 90, nullptr) == ULTRAHDR_NO_ERROR);
  CHECK(j_back.length == j_shift.length && memcmp(f_back.data(), f_shift.data(), j_shift.length) == 0);
  printf("shim tonemap ok: headroom %g (measured), %g (1000 nits)\n", head, given);
  return 0;
}
