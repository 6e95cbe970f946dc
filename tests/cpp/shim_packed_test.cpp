// Drives the packed-RGBA members of the C++ shim: ultrahdr::JpegRHip::encodeJPEGRPacked (host images; it honours
// setMultiChannelGainMap) and the free ultrahdr::generateGainMapPacked (device images, the caller's device buffer).
// usage: shim_packed_test <rgba8888> <hdr> <width> <height> <1010102|f16> <hdr_tf> <out_dir>
//   -> one.jpgr, rgb.jpgr: encodeJPEGRPacked (BT.2100 over BT.709, quality 90) with the setter off / on
//      one.map, rgb.map:   generateGainMapPacked's one-plane / RGBA map
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
  if (argc < 8) return 2;
  std::vector<uint8_t> sdr = slurp(argv[1]), hdr = slurp(argv[2]);
  const size_t w = (size_t)atoi(argv[3]), h = (size_t)atoi(argv[4]);
  const bool f16 = strcmp(argv[5], "f16") == 0;
  const ultrahdr_transfer_function tf = static_cast<ultrahdr_transfer_function>(atoi(argv[6]));
  const std::string out = argv[7];
  CHECK(sdr.size() == w * h * 4 && hdr.size() == w * h * (f16 ? 8 : 4));
  ultrahdr_uncompressed_struct raw_sdr{}, raw_hdr{};
  raw_sdr.data = sdr.data(); raw_sdr.width = w; raw_sdr.height = h; raw_sdr.colorGamut = ULTRAHDR_COLORGAMUT_BT709;
  raw_sdr.pixelFormat = ULTRAHDR_PIX_FMT_RGBA8888;
  raw_hdr.data = hdr.data(); raw_hdr.width = w; raw_hdr.height = h; raw_hdr.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  raw_hdr.pixelFormat = f16 ? ULTRAHDR_PIX_FMT_RGBAF16 : ULTRAHDR_PIX_FMT_RGBA1010102;

  JpegRHip codec;
  std::vector<uint8_t> file(w * h * 6 + 65536);
  ultrahdr_compressed_struct dest{file.data(), 0, (int)file.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGRPacked(nullptr, &raw_sdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGRPacked(&raw_sdr, &raw_sdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);   // an SDR layout as the HDR image
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, f16 ? ULTRAHDR_TF_HLG : ULTRAHDR_TF_LINEAR, &dest, 90, nullptr) == ERROR_ULTRAHDR_INVALID_TRANS_FUNC);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/one.jpgr", dest.data, dest.length));
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/rgb.jpgr", dest.data, dest.length));

  // generateGainMapPacked: the pair and the map in device memory
  void *d_sdr = nullptr, *d_hdr = nullptr, *d_map = nullptr;
  const size_t mw = w / 4, mh = h / 4;
  CHECK(hipMalloc(&d_sdr, sdr.size()) == hipSuccess && hipMalloc(&d_hdr, hdr.size()) == hipSuccess && hipMalloc(&d_map, 4 * mw * mh) == hipSuccess);
  CHECK(hipMemcpy(d_sdr, sdr.data(), sdr.size(), hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice) == hipSuccess);
  ultrahdr_uncompressed_struct dev_sdr = raw_sdr, dev_hdr = raw_hdr;
  dev_sdr.data = d_sdr;
  dev_hdr.data = d_hdr;
  std::vector<uint8_t> map(4 * mw * mh);
  for (int rgb = 0; rgb < 2; ++rgb) {
    ultrahdr_uncompressed_struct dmap{};
    dmap.data = d_map;
    ultrahdr_metadata_struct md;
    CHECK(generateGainMapPacked(&dev_sdr, &dev_hdr, tf, &md, &dmap, rgb != 0, nullptr) == ULTRAHDR_NO_ERROR);
    CHECK(hipDeviceSynchronize() == hipSuccess);
    CHECK(dmap.width == mw && dmap.height == mh && dmap.pixelFormat == (rgb ? ULTRAHDR_PIX_FMT_RGBA8888 : ULTRAHDR_PIX_FMT_MONOCHROME));
    CHECK(md.version == kGainMapVersion && md.minContentBoost == 1.0f && md.maxContentBoost == (tf == ULTRAHDR_TF_PQ ? 10000.0f : 1000.0f) / 203.0f);
    const size_t n = (rgb ? 4 : 1) * mw * mh;
    CHECK(hipMemcpy(map.data(), d_map, n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(dump(out + (rgb ? "/rgb.map" : "/one.map"), map.data(), n));
  }
  CHECK(generateGainMapPacked(&dev_sdr, nullptr, tf, nullptr, nullptr, false, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(hipFree(d_sdr) == hipSuccess && hipFree(d_hdr) == hipSuccess && hipFree(d_map) == hipSuccess);
  printf("shim_packed_test ok\n");
  return 0;
}
