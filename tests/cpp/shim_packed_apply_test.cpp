// Drives the free ultrahdr::applyGainMapPacked of the C++ shim (device images, the caller's device buffer).
// usage: shim_packed_apply_test <rgba8888> <map> <width> <height> <map_width> <map_height> <1|4 map channels> <max_boost> <out_dir>
//   -> hlg_exact.bin, hlg_fast.bin, f16_exact.bin: the renditions at display boost 2
// Host code only: the device buffers come from the HIP runtime's C API.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  if (argc < 10) return 2;
  std::vector<uint8_t> sdr = slurp(argv[1]), map = slurp(argv[2]);
  const size_t w = (size_t)atoi(argv[3]), h = (size_t)atoi(argv[4]), mw = (size_t)atoi(argv[5]), mh = (size_t)atoi(argv[6]);
  const size_t ch = (size_t)atoi(argv[7]);
  const float max_boost = (float)atof(argv[8]);
  const std::string out = argv[9];
  CHECK(sdr.size() == w * h * 4 && map.size() == mw * mh * ch && (ch == 1 || ch == 4));
  void *d_sdr = nullptr, *d_map = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_sdr, sdr.size()) == hipSuccess && hipMalloc(&d_map, map.size()) == hipSuccess && hipMalloc(&d_out, w * h * 8) == hipSuccess);
  CHECK(hipMemcpy(d_sdr, sdr.data(), sdr.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_map, map.data(), map.size(), hipMemcpyHostToDevice) == hipSuccess);
  ultrahdr_uncompressed_struct dev_sdr{}, dev_map{};
  dev_sdr.data = d_sdr; dev_sdr.width = w; dev_sdr.height = h; dev_sdr.colorGamut = ULTRAHDR_COLORGAMUT_P3;
  dev_sdr.pixelFormat = ULTRAHDR_PIX_FMT_RGBA8888;
  dev_map.data = d_map; dev_map.width = mw; dev_map.height = mh; dev_map.colorGamut = ULTRAHDR_COLORGAMUT_UNSPECIFIED;
  dev_map.pixelFormat = ch == 4 ? ULTRAHDR_PIX_FMT_RGBA8888 : ULTRAHDR_PIX_FMT_MONOCHROME;
  ultrahdr_metadata_struct md;
  md.version = kGainMapVersion;
  md.maxContentBoost = max_boost; md.minContentBoost = 1.0f; md.gamma = 1.0f; md.offsetSdr = 0.0f; md.offsetHdr = 0.0f;
  md.hdrCapacityMin = 1.0f; md.hdrCapacityMax = max_boost;
  std::vector<uint8_t> host(w * h * 8);
  struct { ultrahdr_output_format fmt; bool exact; size_t bpp; const char* name; } runs[3] = {
      {ULTRAHDR_OUTPUT_HDR_HLG, true, 4, "/hlg_exact.bin"}, {ULTRAHDR_OUTPUT_HDR_HLG, false, 4, "/hlg_fast.bin"},
      {ULTRAHDR_OUTPUT_HDR_LINEAR, true, 8, "/f16_exact.bin"}};
  for (const auto& r : runs) {
    ultrahdr_uncompressed_struct dest{};
    dest.data = d_out;
    CHECK(applyGainMapPacked(&dev_sdr, &dev_map, &md, r.fmt, 2.0f, &dest, r.exact, nullptr) == ULTRAHDR_NO_ERROR);
    CHECK(hipDeviceSynchronize() == hipSuccess);
    CHECK(dest.width == w && dest.height == h && dest.colorGamut == ULTRAHDR_COLORGAMUT_P3);
    CHECK(hipMemcpy(host.data(), d_out, w * h * r.bpp, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(dump(out + r.name, host.data(), w * h * r.bpp));
  }
  ultrahdr_uncompressed_struct dest{};
  dest.data = d_out;
  CHECK(applyGainMapPacked(&dev_sdr, nullptr, &md, ULTRAHDR_OUTPUT_HDR_HLG, 2.0f, &dest) == ERROR_ULTRAHDR_BAD_PTR);
  ultrahdr_uncompressed_struct planar = dev_sdr;
  planar.pixelFormat = ULTRAHDR_PIX_FMT_YUV420;
  CHECK(applyGainMapPacked(&planar, &dev_map, &md, ULTRAHDR_OUTPUT_HDR_HLG, 2.0f, &dest) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(applyGainMapPacked(&dev_sdr, &dev_map, &md, ULTRAHDR_OUTPUT_SDR, 2.0f, &dest) == ERROR_ULTRAHDR_INVALID_OUTPUT_FORMAT);
  CHECK(hipFree(d_sdr) == hipSuccess && hipFree(d_map) == hipSuccess && hipFree(d_out) == hipSuccess);
  printf("shim_packed_apply_test ok\n");
  return 0;
}
