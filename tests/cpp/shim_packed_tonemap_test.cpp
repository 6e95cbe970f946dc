// Drives the packed API-0 members of the C++ shim: the ultrahdr::JpegRHip::encodeJPEGRPacked overload that takes the HDR image
// alone (it honours setMultiChannelGainMap and the peak given to setToneMap) and the free ultrahdr::toneMapPacked.  Host images.
// usage: shim_packed_tonemap_test <hdr> <width> <height> <1010102|f16> <hdr_tf> <peak_nits> <out_dir>
//   -> one.jpgr, rgb.jpgr:  encodeJPEGRPacked (BT.2100, quality 90), measured headroom, with the setter off / on
//      peak.jpgr:           the same with setToneMap(REINHARD_MAXRGB, peak_nits), one-plane map
//      sdr.rgba, peak.rgba: toneMapPacked's image, rows 3 pixels longer than the image, measured / given headroom
//      heads.f32:           the two headrooms toneMapPacked returned
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
  std::vector<uint8_t> hdr = slurp(argv[1]);
  const size_t w = (size_t)atoi(argv[2]), h = (size_t)atoi(argv[3]);
  const bool f16 = strcmp(argv[4], "f16") == 0;
  const ultrahdr_transfer_function tf = static_cast<ultrahdr_transfer_function>(atoi(argv[5]));
  const float peak = (float)atof(argv[6]);
  const std::string out = argv[7];
  CHECK(hdr.size() == w * h * (f16 ? 8 : 4));
  ultrahdr_uncompressed_struct raw_hdr{};
  raw_hdr.data = hdr.data(); raw_hdr.width = w; raw_hdr.height = h; raw_hdr.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  raw_hdr.pixelFormat = f16 ? ULTRAHDR_PIX_FMT_RGBAF16 : ULTRAHDR_PIX_FMT_RGBA1010102;

  JpegRHip codec;
  std::vector<uint8_t> file(w * h * 6 + 65536);
  ultrahdr_compressed_struct dest{file.data(), 0, (int)file.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  CHECK(codec.encodeJPEGRPacked(nullptr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, f16 ? ULTRAHDR_TF_HLG : ULTRAHDR_TF_LINEAR, &dest, 90, nullptr) == ERROR_ULTRAHDR_INVALID_TRANS_FUNC);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/one.jpgr", dest.data, dest.length));
  codec.setMultiChannelGainMap(true);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/rgb.jpgr", dest.data, dest.length));
  codec.setMultiChannelGainMap(false);
  codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB, peak);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ULTRAHDR_NO_ERROR && dest.length > 0);
  CHECK(dump(out + "/peak.jpgr", dest.data, dest.length));
  codec.setToneMap(UHDR_HIP_TONEMAP_REINHARD_MAXRGB, -1.0f);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, tf, &dest, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);

  // toneMapPacked: the caller's buffer and stride; the padding columns stay as they are
  const size_t stride = w + 3;
  float heads[2] = {-1.0f, -1.0f};
  for (int given = 0; given < 2; ++given) {
    std::vector<uint8_t> sdr(stride * h * 4, 0xAB);
    ultrahdr_uncompressed_struct d{};
    d.data = sdr.data();
    d.luma_stride = stride;
    CHECK(toneMapPacked(&raw_hdr, &d, tf, given ? peak : 0.0f, &heads[given]) == ULTRAHDR_NO_ERROR);
    CHECK(d.width == w && d.height == h && d.luma_stride == stride && d.pixelFormat == ULTRAHDR_PIX_FMT_RGBA8888 &&
          d.colorGamut == ULTRAHDR_COLORGAMUT_BT2100 && d.data == sdr.data());
    for (size_t y = 0; y < h; ++y)
      for (size_t x = 4 * w; x < 4 * stride; ++x) CHECK(sdr[y * stride * 4 + x] == 0xAB);
    CHECK(dump(out + (given ? "/peak.rgba" : "/sdr.rgba"), sdr.data(), sdr.size()));
  }
  CHECK(dump(out + "/heads.f32", heads, sizeof(heads)));
  CHECK(toneMapPacked(&raw_hdr, nullptr, tf) == ERROR_ULTRAHDR_BAD_PTR && toneMapPacked(nullptr, &raw_hdr, tf) == ERROR_ULTRAHDR_BAD_PTR);
  ultrahdr_uncompressed_struct d{};
  std::vector<uint8_t> sdr(w * h * 4);
  d.data = sdr.data();
  CHECK(toneMapPacked(&raw_hdr, &d, tf, -5.0f) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(toneMapPacked(&raw_hdr, &d, f16 ? ULTRAHDR_TF_PQ : ULTRAHDR_TF_LINEAR) == ERROR_ULTRAHDR_INVALID_TRANS_FUNC);
  printf("shim_packed_tonemap_test ok\n");
  return 0;
}
