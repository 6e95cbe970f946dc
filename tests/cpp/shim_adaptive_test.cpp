// shim_adaptive_test.cpp -- the shim's content-adaptive additions, UltraHdrHip::generateGainMapAdaptive and
// JpegRHip::setContentBoost, on the reference's 1280x720 fixture pair (HLG, P010 BT.2100 vs YUV420 BT.709), checked against the
// C-ABI calls they stand on.
// usage: shim_adaptive_test <raw_p010> <raw_yuv420>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "uhdr_hip.h"
#include "ultrahdr_hip/ultrahdr_hip.h"

using namespace ultrahdr;

static std::vector<uint8_t> slurp(const char* p) {
  FILE* f = fopen(p, "rb");
  if (!f) { perror(p); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> b(n);
  if (fread(b.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return b;
}
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const size_t w = 1280, h = 720;
  std::vector<uint8_t> p010 = slurp(argv[1]), yuv = slurp(argv[2]);
  UltraHdrHip uhdr(0);

  ultrahdr_uncompressed_struct yuv420{}, hdr{};
  yuv420.data = yuv.data(); yuv420.width = w; yuv420.height = h; yuv420.colorGamut = ULTRAHDR_COLORGAMUT_BT709;
  yuv420.luma_stride = w; yuv420.chroma_data = yuv.data() + w * h; yuv420.chroma_stride = w / 2;
  hdr.data = p010.data(); hdr.width = w; hdr.height = h; hdr.colorGamut = ULTRAHDR_COLORGAMUT_BT2100;
  hdr.luma_stride = w; hdr.chroma_data = p010.data() + w * h * 2; hdr.chroma_stride = w;

  // generateGainMapAdaptive: generateGainMap's checks and new[] contract, the measured range in the metadata
  ultrahdr_metadata_struct md, md_const;
  ultrahdr_uncompressed_struct map{}, map_const{};
  CHECK(uhdr.generateGainMapAdaptive(nullptr, &hdr, ULTRAHDR_TF_HLG, &md, &map) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(uhdr.generateGainMapAdaptive(&yuv420, &hdr, ULTRAHDR_TF_SRGB, &md, &map) == ERROR_ULTRAHDR_INVALID_TRANS_FUNC);
  CHECK(uhdr.generateGainMapAdaptive(&yuv420, &hdr, ULTRAHDR_TF_HLG, &md, &map) == ULTRAHDR_NO_ERROR);
  std::unique_ptr<uint8_t[]> map_data(reinterpret_cast<uint8_t*>(map.data));
  CHECK(uhdr.generateGainMap(&yuv420, &hdr, ULTRAHDR_TF_HLG, &md_const, &map_const) == ULTRAHDR_NO_ERROR);
  std::unique_ptr<uint8_t[]> map_const_data(reinterpret_cast<uint8_t*>(map_const.data));
  CHECK(map.width == w / 4 && map.height == h / 4 && map.luma_stride == w / 4 && map.pixelFormat == ULTRAHDR_PIX_FMT_MONOCHROME);
  CHECK(md.version == kGainMapVersion && md.gamma == 1.0f && md.offsetSdr == 0.0f && md.offsetHdr == 0.0f);
  CHECK(md.minContentBoost >= 0.25f && md.minContentBoost <= 1.0f && md.maxContentBoost >= 1.0625f && md.maxContentBoost <= md_const.maxContentBoost);
  CHECK(md.hdrCapacityMin == md.minContentBoost && md.hdrCapacityMax == md.maxContentBoost);
  // the C-ABI call it stands on: the same bytes and range
  std::vector<uint8_t> cmap(w / 4 * (h / 4));
  uhdr_hip_image_t cy{yuv420.data, w, h, UHDR_HIP_CG_BT709, yuv420.chroma_data, w, w / 2, UHDR_HIP_PIX_FMT_YUV420};
  uhdr_hip_image_t cp{hdr.data, w, h, UHDR_HIP_CG_BT2100, hdr.chroma_data, w, w, UHDR_HIP_PIX_FMT_P010};
  uhdr_hip_image_t cd{};
  cd.data = cmap.data();
  uhdr_hip_metadata_t cmd;
  CHECK(uhdr_hip_generate_gainmap_adaptive(&cy, &cp, UHDR_HIP_TF_HLG, &cmd, &cd, 0, UHDR_HIP_MEM_HOST, nullptr) == UHDR_HIP_NO_ERROR);
  CHECK(memcmp(cmap.data(), map.data, cmap.size()) == 0 && cmd.minContentBoost == md.minContentBoost && cmd.maxContentBoost == md.maxContentBoost);
  // a narrower range than the constants spreads the same gains over more codes: the maps differ unless the range is the constant one
  const bool same_range = md.minContentBoost == md_const.minContentBoost && md.maxContentBoost == md_const.maxContentBoost;
  CHECK(same_range == (memcmp(map.data, map_const.data, cmap.size()) == 0));
  // applyGainMap takes the map with its metadata
  std::vector<uint8_t> rgba(w * h * 4);
  ultrahdr_uncompressed_struct dest{};
  dest.data = rgba.data();
  CHECK(uhdr.applyGainMap(&yuv420, &map, &md, ULTRAHDR_OUTPUT_HDR_HLG, FLT_MAX, &dest) == ULTRAHDR_NO_ERROR);

  // JpegRHip::setContentBoost: API-0 and API-1 through uhdr_hip_jpegr_encode_adaptive_batch, -1 back to the constants
  JpegRHip codec;
  std::vector<uint8_t> f_const(w * h * 3), f_adapt(w * h * 3), f_back(w * h * 3), f_c(w * h * 3);
  ultrahdr_compressed_struct j_const{f_const.data(), 0, (int)f_const.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct j_adapt{f_adapt.data(), 0, (int)f_adapt.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  ultrahdr_compressed_struct j_back{f_back.data(), 0, (int)f_back.size(), ULTRAHDR_COLORGAMUT_UNSPECIFIED};
  for (int api = 0; api < 2; ++api) {
    for (int scope = 0; scope < 2; ++scope) {
      auto enc = [&](ultrahdr_compressed_struct* d) {
        return api == 0 ? codec.encodeJPEGR(&hdr, ULTRAHDR_TF_HLG, d, 90, nullptr) : codec.encodeJPEGR(&hdr, &yuv420, ULTRAHDR_TF_HLG, d, 90, nullptr);
      };
      codec.setContentBoost(-1);
      CHECK(enc(&j_const) == ULTRAHDR_NO_ERROR);
      codec.setContentBoost(scope);
      CHECK(enc(&j_adapt) == ULTRAHDR_NO_ERROR);
      codec.setContentBoost(-1);
      CHECK(enc(&j_back) == ULTRAHDR_NO_ERROR);
      CHECK(j_back.length == j_const.length && memcmp(f_back.data(), f_const.data(), j_const.length) == 0);
      // the C-ABI batch of one file: the same bytes
      void* out = f_c.data();
      size_t cap = f_c.size(), n = 0;
      uhdr_hip_metadata_t fmd;
      CHECK(uhdr_hip_jpegr_encode_adaptive_batch(1, &cp, api == 0 ? nullptr : &cy, UHDR_HIP_TF_HLG, 90, nullptr, nullptr, &out, &cap, &n, &fmd, nullptr, scope,
                                                 UHDR_HIP_MEM_HOST, nullptr) == UHDR_HIP_NO_ERROR);
      CHECK((int)n == j_adapt.length && memcmp(f_c.data(), f_adapt.data(), n) == 0);
      // the file carries the measured range and decodes
      uhdr_hip_metadata_t parsed;
      CHECK(uhdr_hip_jpegr_metadata(f_adapt.data(), j_adapt.length, &parsed) == UHDR_HIP_NO_ERROR);
      CHECK(parsed.maxContentBoost < 0.999f * md_const.maxContentBoost || fmd.maxContentBoost == md_const.maxContentBoost);
      CHECK(parsed.hdrCapacityMin == parsed.minContentBoost && parsed.hdrCapacityMax == parsed.maxContentBoost);
      if (api == 1) CHECK(fmd.minContentBoost == md.minContentBoost && fmd.maxContentBoost == md.maxContentBoost);
      std::vector<uint8_t> dec(w * h * 8);
      ultrahdr_uncompressed_struct ddest{};
      ddest.data = dec.data();
      ultrahdr_metadata_struct dmd;
      CHECK(codec.decodeJPEGR(&j_adapt, &ddest, FLT_MAX, nullptr, ULTRAHDR_OUTPUT_HDR_LINEAR, nullptr, &dmd) == ULTRAHDR_NO_ERROR);
      CHECK(dmd.minContentBoost == parsed.minContentBoost && dmd.maxContentBoost == parsed.maxContentBoost && ddest.width == w);
    }
  }
  codec.setContentBoost(0);
  CHECK(codec.encodeJPEGR(&hdr, nullptr, ULTRAHDR_TF_HLG, &j_adapt, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(nullptr, ULTRAHDR_TF_HLG, &j_adapt, 90, nullptr) == ERROR_ULTRAHDR_BAD_PTR);
  CHECK(codec.encodeJPEGR(&hdr, ULTRAHDR_TF_HLG, &j_adapt, 101, nullptr) == ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR);
  printf("shim adaptive ok: range [%g, %g]\n", md.minContentBoost, md.maxContentBoost);
  return 0;
}
