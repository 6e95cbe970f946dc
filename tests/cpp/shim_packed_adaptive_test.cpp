// Drives what the C++ shim gained for content-adaptive maps from packed RGBA inputs: JpegRHip::setContentBoost on both
// encodeJPEGRPacked overloads (host images; with setMultiChannelGainMap and, for the HDR-only overload, setToneMap's peak) and the
// free ultrahdr::generateGainMapPackedAdaptive (device images, the caller's device buffer, the measured range back).
// usage: shim_packed_adaptive_test <rgba8888> <hdr> <width> <height> <1010102|f16> <hdr_tf> <out_dir>
//   -> const.jpgr, const0.jpgr:   setContentBoost(-1): today's files (pair / HDR alone)
//      img.jpgr, img_rgb.jpgr:    the pair with setContentBoost(PER_IMAGE), one plane / RGB
//      api0.jpgr:                 the HDR image alone with setContentBoost(PER_IMAGE) and setToneMap's peak of 600 nits
//      one.map, rgb.map:          generateGainMapPackedAdaptive's maps; one.range, rgb.range: the two floats of its metadata
// Host code only: the device buffers come from the HIP runtime's C API.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  // -1, the default and set: what the overloads call today
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/const.jpgr", dest.data, dest.length));
  codec.setContentBoost(-1);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/const0.jpgr", dest.data, dest.length));
  // PER_IMAGE
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/img.jpgr", dest.data, dest.length));
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/img_rgb.jpgr", dest.data, dest.length));
  codec.setMultiChannelGainMap(false);
  codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB, 600.0f);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/api0.jpgr", dest.data, dest.length));
  // an unknown scope is the C call's status; a scale factor other than 4 stays unsupported
  codec.setContentBoost(7);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  codec.setGainMapScaleFactor(2);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);

  // generateGainMapPackedAdaptive: the pair and the map in device memory
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
    CHECK(generateGainMapPackedAdaptive(&dev_sdr, &dev_hdr, tf, &md, &dmap, rgb != 0, nullptr) == ULTRAHDR_NO_ERROR);
    // (the call has waited for the stream: the metadata is the measured range and the map is there)
    CHECK(dmap.width == mw && dmap.height == mh && dmap.pixelFormat == (rgb ? ULTRAHDR_PIX_FMT_RGBA8888 : ULTRAHDR_PIX_FMT_MONOCHROME));
    CHECK(md.version == kGainMapVersion && md.gamma == 1.0f && md.offsetSdr == 0.0f && md.offsetHdr == 0.0f);
    CHECK(md.hdrCapacityMin == md.minContentBoost && md.hdrCapacityMax == md.maxContentBoost && md.minContentBoost <= 1.0f && md.maxContentBoost > 1.0f);
    const size_t n = (rgb ? 4 : 1) * mw * mh;
    CHECK(hipMemcpy(map.data(), d_map, n, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(dump(out + (rgb ? "/rgb.map" : "/one.map"), map.data(), n));
    const float range[2] = {md.minContentBoost, md.maxContentBoost};
    CHECK(dump(out + (rgb ? "/rgb.range" : "/one.range"), range, sizeof(range)));
  }
  CHECK(generateGainMapPackedAdaptive(&dev_sdr, nullptr, tf, nullptr, nullptr, false, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(hipFree(d_sdr) == hipSuccess && hipFree(d_hdr) == hipSuccess && hipFree(d_map) == hipSuccess);
  printf("shim_packed_adaptive_test ok\n");
  return 0;
}
