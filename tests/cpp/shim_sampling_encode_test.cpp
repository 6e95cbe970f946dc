// Drives ultrahdr::JpegRHip::setPrimarySampling and JpegEncoderHelperHip::compressPlanes from C++: 4:2:0 (the default) leaves both
// encodeJPEGRPacked overloads what they were; 4:4:4 and 4:2:2 write the primary image at that sampling, alone and with the encoder's
// options; anything else, and the adaptive form, answer ERROR_ULTRAHDR_UNSUPPORTED_FEATURE.
// usage: shim_sampling_encode_test <rgba1010102> <rgba8888> <width> <height> <out_dir>
//   -> std.jpgr, s444.jpgr, s422.jpgr, s422opt.jpgr (optimised tables, one row per interval), api0_422.jpgr: HLG, BT.2100 over BT.709,
//      quality 90; p444.jpg, p422.jpg, p440.jpg: the SDR image's R, G, B bytes taken as Y and (cropped) Cb, Cr planes, quality 90
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
  std::vector<uint8_t> hdr = slurp(argv[1]), sdr = slurp(argv[2]);
  const size_t w = (size_t)atoi(argv[3]), h = (size_t)atoi(argv[4]);
  const std::string out = argv[5];
  CHECK(hdr.size() == w * h * 4 && sdr.size() == w * h * 4);
  ultrahdr_uncompressed_struct raw_hdr{}, raw_sdr{};
  raw_hdr.data = hdr.data(); raw_hdr.width = w; raw_hdr.height = h; raw_hdr.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  raw_hdr.pixelFormat = ULTRAHDR_PIX_FMT_RGBA1010102;
  raw_sdr.data = sdr.data(); raw_sdr.width = w; raw_sdr.height = h; raw_sdr.colorGamut = ULTRAHDR_COLORGAMUT_BT709;
  raw_sdr.pixelFormat = ULTRAHDR_PIX_FMT_RGBA8888;

  JpegRHip codec;
  const size_t cap = w * h * 8 + 65536;
  std::vector<std::vector<uint8_t>> b(6, std::vector<uint8_t>(cap));
  auto dest = [&](std::vector<uint8_t>& v) { return ultrahdr_compressed_struct{v.data(), 0, (int)cap, ULTRAHDR_COLORGAMUT_UNSPECIFIED}; };
  ultrahdr_compressed_struct std_ = dest(b[0]), s444 = dest(b[1]), s422 = dest(b[2]), s422opt = dest(b[3]), api0 = dest(b[4]), other = dest(b[5]);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &std_, 90, nullptr) == ULTRAHDR_NO_ERROR && std_.length > 0);
  codec.setPrimarySampling(UHDR_HIP_PIX_FMT_YUV420);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ULTRAHDR_NO_ERROR && other.length == std_.length &&
        std::equal(b[5].begin(), b[5].begin() + other.length, b[0].begin()));
  codec.setPrimarySampling(UHDR_HIP_PIX_FMT_YUV444);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &s444, 90, nullptr) == ULTRAHDR_NO_ERROR && s444.length > std_.length);
  codec.setContentBoost(UHDR_HIP_BOOST_PER_IMAGE);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setContentBoost(-1);
  codec.setPrimarySampling(UHDR_HIP_PIX_FMT_YUV440);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &other, 90, nullptr) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setPrimarySampling(UHDR_HIP_PIX_FMT_YUV422);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &s422, 90, nullptr) == ULTRAHDR_NO_ERROR && s422.length > std_.length &&
        s422.length < s444.length);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, ULTRAHDR_TF_HLG, &api0, 90, nullptr) == ULTRAHDR_NO_ERROR && api0.length > 0);
  codec.setOptimizeHuffman(true);
  codec.setRestartInRows(1);
  CHECK(codec.encodeJPEGRPacked(&raw_hdr, &raw_sdr, ULTRAHDR_TF_HLG, &s422opt, 90, nullptr) == ULTRAHDR_NO_ERROR && s422opt.length > 0);

  // compressPlanes: R, G, B bytes of the SDR image as three planes
  std::vector<uint8_t> y(w * h), cb(w * h), cr(w * h);
  for (size_t i = 0; i < w * h; ++i) { y[i] = sdr[4 * i]; cb[i] = sdr[4 * i + 1]; cr[i] = sdr[4 * i + 2]; }
  const char* names[3] = {"/p444.jpg", "/p422.jpg", "/p440.jpg"};
  const int fmts[3] = {UHDR_HIP_PIX_FMT_YUV444, UHDR_HIP_PIX_FMT_YUV422, UHDR_HIP_PIX_FMT_YUV440};
  for (int k = 0; k < 3; ++k) {
    const size_t cw = k == 1 ? (w + 1) / 2 : w, ch = k == 2 ? (h + 1) / 2 : h;
    std::vector<uint8_t> c(2 * cw * ch);   // the top-left cw x ch samples of G and of B
    for (size_t r = 0; r < ch; ++r)
      for (size_t x = 0; x < cw; ++x) { c[r * cw + x] = cb[r * w + x]; c[cw * ch + r * cw + x] = cr[r * w + x]; }
    JpegEncoderHelperHip enc;
    CHECK(enc.compressPlanes(y.data(), c.data(), (int)w, (int)h, (int)w, (int)cw, 90, nullptr, 0, fmts[k]));
    CHECK(dump(out + names[k], enc.getCompressedImagePtr(), enc.getCompressedImageSize()));
    CHECK(!enc.compressPlanes(y.data(), c.data(), (int)w, (int)h, (int)w, (int)cw, 90, nullptr, 0, UHDR_HIP_PIX_FMT_RGBA8888));
  }
  CHECK(dump(out + "/std.jpgr", std_.data, std_.length) && dump(out + "/s444.jpgr", s444.data, s444.length) &&
        dump(out + "/s422.jpgr", s422.data, s422.length) && dump(out + "/s422opt.jpgr", s422opt.data, s422opt.length) &&
        dump(out + "/api0_422.jpgr", api0.data, api0.length));
  printf("shim_sampling_encode_test ok\n");
  return 0;
}
