// Drives ultrahdr::JpegRHip::setMultiChannelGainMap from C++: off (the default) encodeJPEGR API-1 and decodeJPEGR do what they did;
// on, API-1 writes the file with the per-channel gain map and decodeJPEGR applies a three-component map per channel.
// usage: shim_rgbmap_test <p010> <yuv420> <width> <height> <out_dir>
//   -> off.jpgr, on.jpgr: API-1 (HLG, BT.2100 over BT.709, quality 90) with the setter off / on
//      on_dec_on.bin: on.jpgr decoded to HLG RGBA1010102 with the setter on; with it off the file's 4:4:4 map is refused, as ever
//      on_dec_luma.bin: the same with the setter off and setDecodeAnySampling on (the map's luma, as ever)
//      off_dec_on.bin, off_dec_off.bin: off.jpgr with the setter on / off
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

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
  std::vector<uint8_t> file_off(w * h * 4 + 65536), file_on(w * h * 4 + 65536);
  ultrahdr_compressed_struct off{file_off.data(), 0, (int)file_off.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct on{file_on.data(), 0, (int)file_on.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &off, 90, nullptr) == ULTRAHDR_NO_ERROR && off.length > 0);
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGR(&raw_p010, static_cast<uhdr_uncompressed_ptr>(nullptr), ULTRAHDR_TF_HLG, &on, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &on, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGR(&raw_p010, &raw_yuv, ULTRAHDR_TF_HLG, &on, 90, nullptr) == ULTRAHDR_NO_ERROR && on.length > 0);
  CHECK(dump(out + "/off.jpgr", off.data, off.length) && dump(out + "/on.jpgr", on.data, on.length));

  std::vector<uint8_t> px(w * h * 4);
  ultrahdr_uncompressed_struct decoded{};
  decoded.data = px.data();
  codec.setMultiChannelGainMap(false);
  CHECK(codec.decodeJPEGR(&on, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) != ULTRAHDR_NO_ERROR);
  struct { ultrahdr_compressed_struct* file; bool setter, any; const char* name; } runs[4] = {
      {&on, true, false, "/on_dec_on.bin"}, {&on, false, true, "/on_dec_luma.bin"}, {&off, true, false, "/off_dec_on.bin"}, {&off, false, false, "/off_dec_off.bin"}};
  for (auto& r : runs) {
    codec.setMultiChannelGainMap(r.setter);
    codec.setDecodeAnySampling(r.any);
    CHECK(codec.decodeJPEGR(r.file, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ULTRAHDR_NO_ERROR);
    CHECK(decoded.width == w && decoded.height == h);
    CHECK(dump(out + r.name, px.data(), px.size()));
  }
  printf("shim_rgbmap_test ok\n");
  return 0;
}
