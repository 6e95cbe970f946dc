// Drives ultrahdr::JpegRHip::setDecodeScaleDenom and JpegDecoderHelperHip::decompressImage's scale denominator from C++.
// usage: shim_decode_scaled_test <in.jpegr> <denominator> <out.rgba> <out.pq> <out.planes>
//   -> the SDR rendition (RGBA8888) and the HDR_PQ rendition (RGBA1010102) at 1 / denominator, and the primary image's scaled planes
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

static bool dump(const char* path, const void* p, size_t n) {
  FILE* o = fopen(path, "wb");
  const bool ok = o != nullptr && fwrite(p, 1, n, o) == n;
  if (o != nullptr) fclose(o);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int denom = atoi(argv[2]);
  std::vector<uint8_t> file;
  {
    FILE* f = fopen(argv[1], "rb");
    CHECK(f != nullptr);
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) file.insert(file.end(), buf, buf + n);
    fclose(f);
  }
  JpegRHip codec;
  ultrahdr_compressed_struct jpgr{file.data(), (int)file.size(), (int)file.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  jpeg_info_struct pinfo, ginfo;
  jpegr_info_struct info{0, 0, &pinfo, &ginfo};
  CHECK(codec.getJPEGRInfo(&jpgr, &info) == ULTRAHDR_NO_ERROR && info.width > 0 && info.height > 0);
  const size_t ow = (info.width + denom - 1) / denom, oh = (info.height + denom - 1) / denom;
  std::vector<uint8_t> full(info.width * info.height * 8), out(full.size());
  ultrahdr_uncompressed_struct decoded{};
  decoded.data = full.data();
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ULTRAHDR_NO_ERROR);   // the default: full size
  CHECK(decoded.width == info.width && decoded.height == info.height);
  codec.setDecodeScaleDenom(3);
  decoded.data = out.data();
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ERROR_ULTRAHDR_UNSUPPORTED_FEATURE);
  codec.setDecodeScaleDenom(denom);
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ULTRAHDR_NO_ERROR);
  CHECK(decoded.width == ow && decoded.height == oh);
  CHECK(dump(argv[3], out.data(), ow * oh * 4));
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_PQ) == ULTRAHDR_NO_ERROR);
  CHECK(decoded.width == ow && decoded.height == oh);
  CHECK(dump(argv[4], out.data(), ow * oh * 4));
  codec.setDecodeScaleDenom(1);
  std::vector<uint8_t> again(full.size());
  decoded.data = again.data();
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ULTRAHDR_NO_ERROR && again == full);
  JpegDecoderHelperHip dec;
  CHECK(dec.decompressImage(pinfo.imgData.data(), (int)pinfo.imgData.size(), DECODE_TO_YCBCR, denom));
  CHECK(dec.getDecompressedImageWidth() == ow && dec.getDecompressedImageHeight() == oh && dec.getDecompressedImageSize() == ow * oh * 3);
  CHECK(dump(argv[5], dec.getDecompressedImagePtr(), dec.getDecompressedImageSize()));
  CHECK(!dec.decompressImage(pinfo.imgData.data(), (int)pinfo.imgData.size(), DECODE_TO_YCBCR, 5));
  return 0;
}
