// Drives ultrahdr::JpegRHip::setRestartInterval / setRestartInRows from C++: off (the default) encodeJPEGR API-1 and API-0 do what they
// did; set, both write the primary image and the gain map with restart intervals, alone and together with setOptimizeHuffman; the
// overloads the options do not reach write no intervals, and a setter they have no form with answers
// ERROR_ULTRAHDR_UNSUPPORTED_FEATURE.
// usage: shim_restart_test <p010> <yuv420> <width> <height> <out_dir>
//   -> std1.jpgr, std0.jpgr (no intervals), ri1.jpgr, ri0.jpgr (5 MCUs), rows1.jpgr (1 row; the interval of 5 still set), riopt1.jpgr
//      (5 MCUs, optimised tables): API-1 / API-0, HLG, BT.2100 over BT.709, quality 90
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
  std::vector<std::vector<uint8_t>> b(6, std::vector<uint8_t>(cap));
  std::vector<uint8_t> scratch(cap);
  auto dest = [&](std::vector<uint8_t>& v) { return ultrahdr_compressed_struct{v.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED}; };
  ultrahdr_compressed_struct std1 = dest(b[0]), std0 = dest(b[1]), ri1 = dest(b[2]), ri0 = dest(b[3]), rows1 = dest(b[4]), riopt1 = dest(b[5]);
  ultrahdr_compressed_struct other = dest(scratch);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &std1, 90, nullptr) == ULTRAHDR_NO_ERROR && std1.length > 0);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &std0, 90, nullptr) == ULTRAHDR_NO_ERROR && std0.length > 0);

  codec.setRestartInterval(5);
  CHECK(codec.encodeJPEGR(&raw_p010, static_cast<uhdr_uncompressed_ptr>(nullptr), ULTRAHDR_TF_HLG, &ri1, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &ri1, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &ri1, 90, nullptr) == ULTRAHDR_NO_ERROR && ri1.length > std1.length);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &ri0, 90, nullptr) == ULTRAHDR_NO_ERROR && ri0.length > std0.length);
  // no form with these yet: no file without intervals in its name
  codec.setGainMapScaleFactor(2);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setGainMapScaleFactor(4);
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setMultiChannelGainMap(false);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setContentBoost(-1);
  // an overload the options do not reach writes no intervals: API-3 over the default primary image gives what it gives with them off
  ultrahdr_compressed_struct sdr_jpeg{b[0].data(), std1.length, std1.length, ULTRAHDR_COLORGAMUT_BT709};
  std::vector<uint8_t> with(cap), without(cap);
  ultrahdr_compressed_struct a3 = dest(with), b3 = dest(without);
  const status_t s_on = codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &a3);
  // rows override the interval; the interval alone beyond libjpeg's limit is refused
  codec.setRestartInRows(1);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &rows1, 90, nullptr) == ULTRAHDR_NO_ERROR && rows1.length > std1.length);
  codec.setRestartInRows(0);
  codec.setRestartInterval(65536);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setRestartInterval(5);
  codec.setOptimizeHuffman(true);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &riopt1, 90, nullptr) == ULTRAHDR_NO_ERROR && riopt1.length < ri1.length);
  codec.setOptimizeHuffman(false);
  codec.setRestartInterval(0);
  const status_t s_off = codec.encodeJPEGR(&raw_p010, &sdr_jpeg, ULTRAHDR_TF_HLG, &b3);
  CHECK(s_on == s_off && a3.length == b3.length && std::equal(with.begin(), with.begin() + a3.length, without.begin()));
  // and off again, API-1 is what it was
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length == std1.length &&
        std::equal(scratch.begin(), scratch.begin() + other.length, b[0].begin()));

  CHECK(dump(out + "/std1.jpgr", std1.data, std1.length) && dump(out + "/std0.jpgr", std0.data, std0.length) &&
        dump(out + "/ri1.jpgr", ri1.data, ri1.length) && dump(out + "/ri0.jpgr", ri0.data, ri0.length) &&
        dump(out + "/rows1.jpgr", rows1.data, rows1.length) && dump(out + "/riopt1.jpgr", riopt1.data, riopt1.length));
  printf("shim_restart_test ok\n");
  return 0;
}
