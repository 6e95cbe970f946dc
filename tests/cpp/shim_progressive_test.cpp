// Drives ultrahdr::JpegRHip::setProgressive from C++: off (the default) encodeJPEGR API-1 and API-0 do what they did; set, both write
// the primary image and the gain map as progressive files, which decodeJPEGR reads to the rendition of the baseline file; a setter it
// has no form with, and a restart setting, answer ERROR_ULTRAHDR_UNSUPPORTED_FEATURE; setOptimizeHuffman changes nothing.
// usage: shim_progressive_test <p010> <yuv420> <width> <height> <out_dir>
//   -> api1.jpgr, api0.jpgr: progressive, HLG, BT.2100 over BT.709, quality 90
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
static bool has_sof2(const ultrahdr_compressed_struct& j) {
  const uint8_t* d = static_cast<const uint8_t*>(j.data);
  const uint8_t m[2] = {0xFF, 0xC2};
  return std::search(d, d + j.length, m, m + 2) != d + j.length;
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
  std::vector<std::vector<uint8_t>> b(4, std::vector<uint8_t>(cap));
  std::vector<uint8_t> scratch(cap);
  auto dest = [&](std::vector<uint8_t>& v) { return ultrahdr_compressed_struct{v.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED}; };
  ultrahdr_compressed_struct std1 = dest(b[0]), std0 = dest(b[1]), pr1 = dest(b[2]), pr0 = dest(b[3]), other = dest(scratch);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &std1, 90, nullptr) == ULTRAHDR_NO_ERROR && std1.length > 0 && !has_sof2(std1));
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &std0, 90, nullptr) == ULTRAHDR_NO_ERROR && std0.length > 0);

  codec.setProgressive(true);
  CHECK(codec.encodeJPEGR(&raw_p010, static_cast<uhdr_uncompressed_ptr>(nullptr), ULTRAHDR_TF_HLG, &pr1, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &pr1, 90, nullptr) == ULTRAHDR_NO_ERROR && has_sof2(pr1));
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &pr0, 90, nullptr) == ULTRAHDR_NO_ERROR && has_sof2(pr0));
  // the flag changes nothing
  codec.setOptimizeHuffman(true);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length == pr1.length &&
        std::equal(scratch.begin(), scratch.begin() + other.length, b[2].begin()));
  codec.setOptimizeHuffman(false);
  // no form with these: no baseline file under this setting
  codec.setRestartInterval(5);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setRestartInterval(0);
  codec.setRestartInRows(1);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setRestartInRows(0);
  codec.setGainMapScaleFactor(2);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setGainMapScaleFactor(4);
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGR(&raw_p010, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setMultiChannelGainMap(false);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setContentBoost(-1);

  // decodeJPEGR reads the progressive file: the rendition of the baseline one
  std::vector<uint8_t> hdr_a(w * h * 4), hdr_b(w * h * 4);
  ultrahdr_uncompressed_struct da{}, db{};
  da.data = hdr_a.data();
  db.data = hdr_b.data();
  CHECK(codec.decodeJPEGR(&std1, &da, 3.4028234663852886e38f, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ULTRAHDR_NO_ERROR &&
        codec.decodeJPEGR(&pr1, &db, 3.4028234663852886e38f, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ULTRAHDR_NO_ERROR);   // (4 bytes a pixel)
  CHECK(da.width == db.width && da.height == db.height && hdr_a == hdr_b);

  // and off again, API-1 is what it was
  codec.setProgressive(false);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length == std1.length &&
        std::equal(scratch.begin(), scratch.begin() + other.length, b[0].begin()));

  CHECK(dump(out + "/api1.jpgr", pr1.data, pr1.length) && dump(out + "/api0.jpgr", pr0.data, pr0.length));
  printf("shim_progressive_test ok\n");
  return 0;
}
