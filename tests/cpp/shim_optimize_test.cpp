// Drives ultrahdr::JpegRHip::setOptimizeHuffman from C++: off (the default) encodeJPEGR API-1 and API-0 do what they did; on, both
// write the file with optimised Huffman tables, the overloads the flag does not reach keep the default tables, and a setter the
// flag has no form with answers ERROR_ULTRAHDR_UNSUPPORTED_FEATURE.
// usage: shim_optimize_test <p010> <yuv420> <width> <height> <out_dir>
//   -> std1.jpgr, opt1.jpgr (API-1), std0.jpgr, opt0.jpgr (API-0): HLG, BT.2100 over BT.709, quality 90
#include <algorithm>
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
  std::vector<uint8_t> b[4] = {std::vector<uint8_t>(cap), std::vector<uint8_t>(cap), std::vector<uint8_t>(cap), std::vector<uint8_t>(cap)}, scratch(cap);
  ultrahdr_compressed_struct std1{b[0].data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct opt1{b[1].data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct std0{b[2].data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct opt0{b[3].data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct other{scratch.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &std1, 90, nullptr) == ULTRAHDR_NO_ERROR && std1.length > 0);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &std0, 90, nullptr) == ULTRAHDR_NO_ERROR && std0.length > 0);

  codec.setOptimizeHuffman(true);
  CHECK(codec.encodeJPEGR(&raw_p010, static_cast<uhdr_uncompressed_ptr>(nullptr), ULTRAHDR_TF_HLG, &opt1, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &opt1, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &opt1, 90, nullptr) == ULTRAHDR_NO_ERROR && opt1.length > 0);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &opt0, 90, nullptr) == ULTRAHDR_NO_ERROR && opt0.length > 0);
  CHECK(opt1.length < std1.length && opt0.length < std0.length);
  // the flag has no form with these yet: no file with default tables in its name
  codec.setGainMapScaleFactor(2);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setGainMapScaleFactor(4);
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setMultiChannelGainMap(false);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setContentBoost(-1);
  // an overload the flag does not reach keeps the default tables: API-3 over the default primary image gives what it gives with the flag off
  ultrahdr_compressed_struct sdr_jpeg{b[0].data(), std1.length, std1.length, ULTRAHDR_COLORGAMUT_BT709};
  std::vector<uint8_t> with(cap), without(cap);
  ultrahdr_compressed_struct a3{with.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED}, b3{without.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  const status_t s_on = codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &a3);
  codec.setOptimizeHuffman(false);
  const status_t s_off = codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &b3);
  CHECK(s_on == s_off && a3.length == b3.length && std::equal(with.begin(), with.begin() + a3.length, without.begin()));
  // and off again, API-1 is what it was
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length == std1.length &&
        std::equal(scratch.begin(), scratch.begin() + other.length, b[0].begin()));

  CHECK(dump(out + "/std1.jpgr", std1.data, std1.length) && dump(out + "/opt1.jpgr", opt1.data, opt1.length) &&
        dump(out + "/std0.jpgr", std0.data, std0.length) && dump(out + "/opt0.jpgr", opt0.data, opt0.length));
  printf("shim_optimize_test ok\n");
  return 0;
}
