// Drives ultrahdr::JpegRHip::setAnyGainMapMetadata and ultrahdr::gainMapWeight from C++: off (the default) decodeJPEGR refuses a file
// whose metadata has a gamma, offsets or a capacity range of its own, as the reference does; on, it decodes it.
// usage: shim_gainmap_md_test <dir> <width> <height>
//   reads  <dir>/gen1.jpgr, gen3.jpgr (general metadata, one- and three-component map), deg1.jpgr (degenerate metadata)
//   writes gen1_on.bin, gen3_on.bin, deg1_on.bin, deg1_off.bin: HLG RGBA1010102 at max_display_boost 3
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static std::vector<uint8_t> slurp(const std::string& p) {
  std::vector<uint8_t> b;
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { perror(p.c_str()); exit(2); }
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
  if (argc < 4) return 2;
  const std::string dir = argv[1];
  const size_t w = (size_t)atoi(argv[2]), h = (size_t)atoi(argv[3]);

  // the weight, host only: hdrCapacity 1.5 .. 6 at a display boost of 3
  ultrahdr_metadata_struct md{};
  md.version = "1.0";
  md.maxContentBoost = 8.0f; md.minContentBoost = 0.5f; md.gamma = 0.5f; md.offsetSdr = 0.0f; md.offsetHdr = 1.0f / 32.0f;
  md.hdrCapacityMin = 1.5f; md.hdrCapacityMax = 6.0f;
  float weight = -1.0f, boost = -1.0f;
  CHECK(gainMapWeight(&md, 3.0f, &weight, &boost) == ULTRAHDR_NO_ERROR);
  CHECK(std::fabs(weight - 0.5f) < 1e-6f && boost == 3.0f);
  CHECK(gainMapWeight(&md, 100.0f, &weight, &boost) == ULTRAHDR_NO_ERROR && weight == 1.0f && boost == 6.0f);
  CHECK(gainMapWeight(nullptr, 3.0f, &weight, &boost) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(gainMapWeight(&md, 0.5f, &weight, &boost) == ERROR_ULTRAHDR_INVALID_DISPLAY_BOOST);
  md.gamma = 0.0f;
  CHECK(gainMapWeight(&md, 3.0f, &weight, &boost) == ERROR_ULTRAHDR_BAD_METADATA);

  JpegRHip codec;
  std::vector<uint8_t> px(w * h * 4);
  ultrahdr_uncompressed_struct decoded{};
  decoded.data = px.data();
  const char* general[2] = {"gen1", "gen3"};
  for (const char* name : general) {
    std::vector<uint8_t> file = slurp(dir + "/" + name + ".jpgr");
    ultrahdr_compressed_struct in{file.data(), (int)file.size(), (int)file.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
    codec.setAnyGainMapMetadata(false);
    codec.setMultiChannelGainMap(true);   // (reads the three-component map; the metadata is refused all the same)
    CHECK(codec.decodeJPEGR(&in, &decoded, 3.0f, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ERROR_ULTRAHDR_BAD_METADATA);
    codec.setMultiChannelGainMap(false);
    codec.setAnyGainMapMetadata(true);
    ultrahdr_metadata_struct got{};
    CHECK(codec.decodeJPEGR(&in, &decoded, 3.0f, nullptr, ULTRAHDR_OUTPUT_HDR_HLG, nullptr, &got) == ULTRAHDR_NO_ERROR);
    CHECK(decoded.width == w && decoded.height == h && std::fabs(got.gamma - 2.2f) < 1e-4f);
    CHECK(dump(dir + "/" + name + "_on.bin", px.data(), px.size()));
  }
  std::vector<uint8_t> file = slurp(dir + "/deg1.jpgr");
  ultrahdr_compressed_struct in{file.data(), (int)file.size(), (int)file.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  for (int on = 0; on < 2; ++on) {
    codec.setAnyGainMapMetadata(on != 0);
    CHECK(codec.decodeJPEGR(&in, &decoded, 3.0f, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ULTRAHDR_NO_ERROR);
    CHECK(dump(dir + (on ? "/deg1_on.bin" : "/deg1_off.bin"), px.data(), px.size()));
  }
  printf("shim_gainmap_md_test ok\n");
  return 0;
}
