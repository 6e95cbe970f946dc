// Drives ultrahdr::JpegRHip::setDecodeAnySampling from C++: a JPEG/R file whose primary image is not 4:2:0 is refused by default, as the
// reference refuses it, and decodes once the setter is on.
// usage: shim_sampling_test <in.jpegr> <out.rgba>    -> writes the SDR rendition (RGBA8888)
#include <cfloat>
#include <cstdio>
#include <vector>

#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
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
  std::vector<uint8_t> out(info.width * info.height * 8);
  ultrahdr_uncompressed_struct decoded{};
  decoded.data = out.data();
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ERROR_ULTRAHDR_DECODE_ERROR);
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ERROR_ULTRAHDR_DECODE_ERROR);
  codec.setDecodeAnySampling(true);
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_HLG) == ULTRAHDR_NO_ERROR);
  CHECK(codec.decodeJPEGR(&jpgr, &decoded, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ULTRAHDR_NO_ERROR);
  CHECK(decoded.width == info.width && decoded.height == info.height);
  codec.setDecodeAnySampling(false);
  std::vector<uint8_t> again(out.size());
  ultrahdr_uncompressed_struct refused{};
  refused.data = again.data();
  CHECK(codec.decodeJPEGR(&jpgr, &refused, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_SDR) == ERROR_ULTRAHDR_DECODE_ERROR);
  FILE* o = fopen(argv[2], "wb");
  CHECK(o != nullptr && fwrite(out.data(), 1, info.width * info.height * 4, o) == info.width * info.height * 4);
  fclose(o);
  return 0;
}
