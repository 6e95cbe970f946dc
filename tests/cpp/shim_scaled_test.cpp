// Drives ultrahdr::JpegRHip::setGainMapScaleFactor from C++: at 4 (the default) encodeJPEGR API-1 does what it did; at 2 it writes the
// file with the gain map at factor 2, with and without setMultiChannelGainMap, and every overload that could only write a factor-4
// map answers ERROR_ULTRAHDR_UNSUPPORTED_FEATURE.
// usage: shim_scaled_test <p010> <yuv420> <width> <height> <out_dir>
//   -> s4.jpgr, s2.jpgr, s2_rgb.jpgr: API-1 (HLG, BT.2100 over BT.709, quality 90)
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "uhdr_hip.h"
#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static std::vector<uint8_t> slurp(const char* p) {
  std::vector<uint8_t> b;
  FILE* f = fopen(p, "rb");
  if (!f) { perror(p); exit(2); }
  uint8_t buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
static bool dump(const std::string& p, const void* d, size_t n) {
  FILE* f = fopen(p.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(d, 1, n, f) == n;
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  std::vector<uint8_t> p010 = slurp(argv[1]), yuv = slurp(argv[2]);
  const size_t w = (size_t)atoi(argv[3]), h = (size_t)atoi(argv[4]);
  const std::string out = argv[5];
  CHECK(p010.size() == w * h * 3 && yuv.size() == w * h * 3 / 2);
  ultrahdr_uncompressed_struct raw_p010{}, raw_yuv{};
  raw_p010.data = p010.data(); raw_p010.width = w; raw_p010.height = h; raw_p010.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  raw_yuv.data = yuv.data(); raw_yuv.width = w; raw_yuv.height = h; raw_yuv.colorGamut = ULTRAHDR_COLORGAMUT_BT709;

  JpegRHip codec;
  const size_t cap = w * h * 8 + 65536;
  std::vector<uint8_t> b4(cap), b2(cap), b2rgb(cap), scratch(cap);
  ultrahdr_compressed_struct s4{b4.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct s2{b2.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct s2rgb{b2rgb.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct other{scratch.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &s4, 90, nullptr) == ULTRAHDR_NO_ERROR && s4.length > 0);

  codec.setGainMapScaleFactor(2);
  CHECK(codec.encodeJPEGR(&raw_p010, static_cast<uhdr_uncompressed_ptr>(nullptr), ULTRAHDR_TF_HLG, &s2, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &s2, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &s2, 90, nullptr) == ULTRAHDR_NO_ERROR && s2.length > 0);
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &s2rgb, 90, nullptr) == ULTRAHDR_NO_ERROR && s2rgb.length > 0);
  codec.setMultiChannelGainMap(false);
  // API-0 at the factor writes a file as well
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length > 0);
  // what could only write a factor-4 map: API-3, API-2, the packed overloads, the operator, the adaptive range
  ultrahdr_compressed_struct sdr_jpeg{b4.data(), s4.length, s4.length, ULTRAHDR_COLORGAMUT_BT709};
  CHECK(codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &other) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, &sdr_jpeg, ULTRAHDR_TF_HLG, &other) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGRPacked(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGRPacked(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setToneMap(UHDR_HIP_TONEMAP_SHIFT);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  // back at 4 they are what they were
  codec.setGainMapScaleFactor(4);
  CHECK(codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &other) != ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);

  CHECK(dump(out + "/s4.jpgr", s4.data, s4.length) && dump(out + "/s2.jpgr", s2.data, s2.length) && dump(out + "/s2_rgb.jpgr", s2rgb.data, s2rgb.length));
  printf("shim_scaled_test ok\n");
  return 0;
}
