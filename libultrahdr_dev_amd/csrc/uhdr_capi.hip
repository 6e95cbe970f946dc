// uhdr_capi.hip -- the C-ABI of include/uhdr_hip.h: argument validation in the reference's order,
// per-call constants, host staging, batching.  All pixel work happens in uhdr_kernels.hip on the
// GPU; there is deliberately no CPU fallback -- without a usable device every compute entry point
// returns UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/uhdr_hip.h"
#include "uhdr_kernels.h"
#include "uhdr_jpeg.h"
#include "uhdr_jpegr.h"

namespace {

using namespace uhdr;

thread_local char t_err[256] = "";

void set_err(const char* where, hipError_t e) {
  snprintf(t_err, sizeof(t_err), "%s: %s", where, hipGetErrorString(e));
}

#define HIP_TRY(expr)                          \
  do {                                         \
    hipError_t _e = (expr);                    \
    if (_e != hipSuccess) {                    \
      set_err(#expr, _e);                      \
      return UHDR_HIP_UNKNOWN_ERROR;           \
    }                                          \
  } while (0)

// ---- per-device state --------------------------------------------------------------------------
// grow-only device staging buffers of one UHDR_HIP_MEM_HOST call.  The four pixel-path entry points (generate, apply, toneMap,
// convertYuv) lease a set of their own for the duration of a call, so host callers on different streams overlap their copies and
// kernels; the codec entry points lease a whole context (CodecLease).
constexpr int kStageSlots = 8;
struct StageSet {
  void* stage[kStageSlots] = {};
  size_t stage_bytes[kStageSlots] = {};
};
struct DeviceState : StageSet {
  bool ready = false;
  std::map<int, float*> idw;  // scale -> device tables (4 * scale*scale*4 floats)
  float* lut = nullptr;       // the five static transfer-function tables (kLutTotal floats), built at init
  float* tone_tab = nullptr;  // the packed tone-map's inverse OETFs of the 1024 codes, HLG then PQ (2 * kTonePackedCodes floats), built at init
  float* srgb_codes = nullptr;   // the packed apply's srgbInvOetf(code * (1 / 255.0f)) of the 256 codes (kSrgbCodes floats), built at init
  std::vector<std::unique_ptr<StageSet>> sets;   // every set ever leased ...
  std::vector<StageSet*> free_sets;              // ... and those not in use (both under g_mu)
  std::vector<std::pair<hipStream_t, void*>> retired;   // workspaces that were outgrown while a launch may still have named them, by stream
  // uhdr_hip_jpegr_decode[_batch]: per-file decoder workspaces and planes
  std::vector<void*> pool;
  std::vector<size_t> pool_bytes;
  // encodeJPEGR (compress_to_host): page-locked host memory the encoder's descriptors, sizes and compressed streams land in (grow-only)
  void* host_pool = nullptr;
  size_t host_pool_bytes = 0;
  // generate with statistics: the candidate lists of one launch (kStatWsBytes), one workspace per stream the caller has used --
  // launches of one stream follow each other, launches of different streams may overlap
  std::map<hipStream_t, uint32_t*> stat_ws;
  // EXACT apply behind its pre-filter: the lists of pixels in doubt (uhdr_kernels.h: ex_ws_bytes), per stream, grown on demand
  struct ExWs { uint32_t* p = nullptr; size_t bytes = 0; };
  std::map<hipStream_t, ExWs> ex_ws;
  // uhdr_hip_add_effects_batch: the jobs and tables of one round, per stream -- page-locked host memory the round is composed in
  // and its device copy.  `ev` follows the upload on the stream: the host side is rewritten only behind it.
  struct FxWs { void* host = nullptr; size_t host_bytes = 0; void* dev = nullptr; size_t dev_bytes = 0; hipEvent_t ev = nullptr; bool pending = false; };
  std::map<hipStream_t, FxWs> fx_ws;
  // the codec entry points (jpeg_*, jpegr_*, effects and tables through host memory) each lease a context of their own for the
  // duration of a call -- staging slots, device and host pools -- so that callers on different streams overlap
  // (CodecLease); a context is a DeviceState that borrows this one's tables
  std::vector<std::unique_ptr<DeviceState>> codec_sets;   // every context ever leased ...
  std::vector<DeviceState*> free_codec;                    // ... and those not in use (both under g_mu)
};
std::mutex g_mu;                    // guards g_dev (init / table cache)
// a kernel and the resolve kernel behind it share a per-stream workspace: the pair is enqueued as one unit, so that two host threads
// using the same stream cannot interleave their launches (they would read each other's lists)
std::mutex g_pair_mu;
std::map<int, DeviceState> g_dev;

// gainmapmath.cpp:69-110: sqrt runs in double on a float expression, weights are float divisions
float euclid(float x1, float x2, float y1, float y2) {
  return (float)std::sqrt((double)(((y2 - y1) * (y2 - y1)) + (x2 - x1) * (x2 - x1)));
}
void fill_idw(float* w, int scale, int incR, int incB) {
  for (int y = 0; y < scale; y++)
    for (int x = 0; x < scale; x++) {
      const float pos_x = ((float)x) / scale, pos_y = ((float)y) / scale;
      const int curr_x = (int)std::floor((double)pos_x), curr_y = (int)std::floor((double)pos_y);
      const int next_x = curr_x + incR, next_y = curr_y + incB;
      const float d1 = euclid(pos_x, curr_x, pos_y, curr_y);
      float* o = w + y * scale * 4 + x * 4;
      if (d1 == 0) {
        o[0] = 1.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
      } else {
        const float w1 = 1.f / d1;
        const float w2 = 1.f / euclid(pos_x, curr_x, pos_y, next_y);
        const float w3 = 1.f / euclid(pos_x, next_x, pos_y, curr_y);
        const float w4 = 1.f / euclid(pos_x, next_x, pos_y, next_y);
        const float total = w1 + w2 + w3 + w4;
        o[0] = w1 / total; o[1] = w2 / total; o[2] = w3 / total; o[3] = w4 / total;
      }
    }
}
// table order: std (1,1), no-right (0,1), no-bottom (1,0), corner (0,0)  gainmapmath.h:191-194
void build_idw_tables(int scale, std::vector<float>& out) {
  const size_t n = (size_t)scale * scale * 4;
  out.assign(4 * n, 0.f);
  fill_idw(out.data(), scale, 1, 1);
  fill_idw(out.data() + n, scale, 0, 1);
  fill_idw(out.data() + 2 * n, scale, 1, 0);
  fill_idw(out.data() + 3 * n, scale, 0, 0);
}

int current_state(DeviceState** st) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_dev.find(dev);
  if (it == g_dev.end() || !it->second.ready) {
    snprintf(t_err, sizeof(t_err), "uhdr_hip_init(%d) has not been called", dev);
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  *st = &it->second;
  return UHDR_HIP_NO_ERROR;
}

// ShepardsIDW(scale) on the device.  The scale comes from the caller's images (a file, on the decode path): the table holds
// 16 scale^2 floats -- 4.3 GB for an 8192-wide image over a 1-pixel map, which the reference allocates per call and frees.  Tables up
// to kIdwCacheMaxScale (1 MiB) are built once per device and kept; larger ones live for the call (*transient: the caller frees it
// once its launches have finished).  The table is built outside the lock; running out of memory is a status, not an exception.
constexpr int kIdwCacheMaxScale = 128;
int idw_for_scale(DeviceState* st, int scale, const float** dptr, float** transient) {
  *transient = nullptr;
  if (scale <= kIdwCacheMaxScale) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = st->idw.find(scale);
    if (it != st->idw.end()) { *dptr = it->second; return UHDR_HIP_NO_ERROR; }
  }
  std::vector<float> t;
  try {
    build_idw_tables(scale, t);
  } catch (const std::bad_alloc&) {
    snprintf(t_err, sizeof(t_err), "no memory for the weight table of map scale %d", scale);
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  float* d = nullptr;
  if (hipMalloc(&d, t.size() * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(t_err, sizeof(t_err), "no device memory for the weight table of map scale %d", scale);
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  if (hipMemcpy(d, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return UHDR_HIP_UNKNOWN_ERROR; }
  if (scale > kIdwCacheMaxScale) { *transient = d; *dptr = d; return UHDR_HIP_NO_ERROR; }
  std::lock_guard<std::mutex> lk(g_mu);
  auto ins = st->idw.emplace(scale, d);
  if (!ins.second) (void)hipFree(d);   // another thread was faster
  *dptr = ins.first->second;
  return UHDR_HIP_NO_ERROR;
}
// The table of one chunk's launches.  A table too large to keep is freed when the lease ends, behind a wait for the stream: when
// the chunk's launches have finished.
struct IdwLease {
  const float* idw = nullptr;
  IdwLease() = default;
  IdwLease(const IdwLease&) = delete;
  IdwLease& operator=(const IdwLease&) = delete;
  int take(DeviceState* st, int scale, hipStream_t s) { s_ = s; return idw_for_scale(st, scale, &idw, &transient_); }
  ~IdwLease() { if (transient_) { (void)hipStreamSynchronize(s_); (void)hipFree(transient_); } }
 private:
  float* transient_ = nullptr;
  hipStream_t s_ = nullptr;
};

// ---- colour constants (gainmapmath.cpp:121-248, 359-393, 447-481) ------------------------------
struct YuvRgb { float cr, gcb, gcr, cb; };
YuvRgb yuv_rgb_coeffs(int gamut) {
  // G coefficients are float (B*Cb)/G and (R*Cr)/G exactly as the reference's static initialisers
  switch (gamut) {
    case UHDR_HIP_CG_BT709: {
      const float R = 0.2126f, G = 0.7152f, B = 0.0722f, Cb = 1.8556f, Cr = 1.5748f;
      return {Cr, B * Cb / G, R * Cr / G, Cb};
    }
    case UHDR_HIP_CG_P3: {
      const float R = 0.299f, G = 0.587f, B = 0.114f, Cb = 1.772f, Cr = 1.402f;
      return {Cr, B * Cb / G, R * Cr / G, Cb};
    }
    default: {
      const float R = 0.2627f, G = 0.6780f, B = 0.0593f, Cb = 1.8814f, Cr = 1.4746f;
      return {Cr, B * Cb / G, R * Cr / G, Cb};
    }
  }
}
void luminance_coeffs(int gamut, float* o) {
  switch (gamut) {
    case UHDR_HIP_CG_BT709: o[0] = 0.2126f; o[1] = 0.7152f; o[2] = 0.0722f; break;
    case UHDR_HIP_CG_P3: o[0] = 0.20949f; o[1] = 0.72160f; o[2] = 0.06891f; break;
    default: o[0] = 0.2627f; o[1] = 0.6780f; o[2] = 0.0593f; break;
  }
}
const float kBt709ToP3[9] = {0.82254f, 0.17755f, 0.00006f, 0.03312f, 0.96684f, -0.00001f, 0.01706f, 0.07240f, 0.91049f};
const float kBt709ToBt2100[9] = {0.62740f, 0.32930f, 0.04332f, 0.06904f, 0.91958f, 0.01138f, 0.01636f, 0.08799f, 0.89555f};
const float kP3ToBt709[9] = {1.22482f, -0.22490f, -0.00007f, -0.04196f, 1.04199f, 0.00001f, -0.01961f, -0.07865f, 1.09831f};
const float kP3ToBt2100[9] = {0.75378f, 0.19862f, 0.04754f, 0.04576f, 0.94177f, 0.01250f, -0.00121f, 0.01757f, 0.98359f};
const float kBt2100ToBt709[9] = {1.66045f, -0.58764f, -0.07286f, -0.12445f, 1.13282f, -0.00837f, -0.01811f, -0.10057f, 1.11878f};
const float kBt2100ToP3[9] = {1.34369f, -0.28223f, -0.06135f, -0.06533f, 1.07580f, -0.01051f, 0.00283f, -0.01957f, 1.01679f};
// getHdrConversionFn(sdr_gamut, hdr_gamut): nullptr <=> identity
const float* hdr_conversion(int sdr, int hdr) {
  if (sdr == hdr) return nullptr;
  switch (sdr) {
    case UHDR_HIP_CG_BT709: return hdr == UHDR_HIP_CG_P3 ? kP3ToBt709 : kBt2100ToBt709;
    case UHDR_HIP_CG_P3: return hdr == UHDR_HIP_CG_BT709 ? kBt709ToP3 : kBt2100ToP3;
    default: return hdr == UHDR_HIP_CG_BT709 ? kBt709ToBt2100 : kP3ToBt2100;
  }
}
const float kYuv709To601[9] = {1.0f, 0.101579f, 0.196076f, 0.0f, 0.989854f, -0.110653f, 0.0f, -0.072453f, 0.983398f};
const float kYuv709To2100[9] = {1.0f, -0.016969f, 0.096312f, 0.0f, 0.995306f, -0.051192f, 0.0f, 0.011507f, 1.002637f};
const float kYuv601To709[9] = {1.0f, -0.118188f, -0.212685f, 0.0f, 1.018640f, 0.114618f, 0.0f, 0.075049f, 1.025327f};
const float kYuv601To2100[9] = {1.0f, -0.128245f, -0.115879f, 0.0f, 1.010016f, 0.061592f, 0.0f, 0.086969f, 1.029350f};
const float kYuv2100To709[9] = {1.0f, 0.018149f, -0.095132f, 0.0f, 1.004123f, 0.051267f, 0.0f, -0.011524f, 0.996782f};
const float kYuv2100To601[9] = {1.0f, 0.117887f, 0.105521f, 0.0f, 0.995211f, -0.059549f, 0.0f, -0.084085f, 0.976518f};

bool valid_gamut(int g) { return g >= UHDR_HIP_CG_BT709 && g <= UHDR_HIP_CG_BT2100; }
bool al(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
bool tf_known(int tf) { return tf == UHDR_HIP_TF_LINEAR || tf == UHDR_HIP_TF_HLG || tf == UHDR_HIP_TF_PQ; }
// the rows of an image whose luma_stride may be left 0: stride in pixels, 0 means width (gainmapmath.cpp:585)
size_t row_stride(const uhdr_hip_image_t& im) { return im.luma_stride == 0 ? im.width : im.luma_stride; }
// The chunk rule of every batch call: a chunk is up to `cap` consecutive images -- kMaxChunk for the gain-map
// calls, kToneChunk for the tone-map and convertYuv calls, whose runs these are --, from image i on, that have the shape of image i
// (same_shape(j)) and one class (aligned or not, FAST or not).  fill(j, m) fills slot m of the batch from image j and returns image
// j's class: before the classes are compared, so the image that ends a chunk leaves its slot behind and nothing else -- harmless,
// as m < cap there and a launch reads only the slots of its members.  What only the members receive (their destination
// descriptors) the caller fills, for images [i, i + m).
struct Chunk { int m; bool cls; };
template <class Same, class Fill>
Chunk form_chunk(int i, int n, int cap, Same same_shape, Fill fill) {
  Chunk ch{0, true};
  while (i + ch.m < n && ch.m < cap) {
    if (!same_shape(i + ch.m)) break;
    const bool cls = fill(i + ch.m, ch.m);
    if (ch.m == 0) ch.cls = cls;
    else if (cls != ch.cls) break;
    ++ch.m;
  }
  return ch;
}

// ---- generate ------------------------------------------------------------------------------------
// checks of ultrahdr.cpp:189-202 + the switch defaults of :222-302, in the reference's order
int validate_generate(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* p010, int hdr_tf,
                      const uhdr_hip_metadata_t* md, const uhdr_hip_image_t* dest) {
  if (yuv == nullptr || p010 == nullptr || md == nullptr || dest == nullptr || yuv->data == nullptr ||
      yuv->chroma_data == nullptr || p010->data == nullptr || p010->chroma_data == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;
  if (yuv->width != p010->width || yuv->height != p010->height) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  if (yuv->colorGamut == UHDR_HIP_CG_UNSPECIFIED || p010->colorGamut == UHDR_HIP_CG_UNSPECIFIED)
    return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (!valid_gamut(yuv->colorGamut) || !valid_gamut(p010->colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  return UHDR_HIP_NO_ERROR;
}

void fill_generate_metadata(int hdr_tf, uhdr_hip_metadata_t* md) {  // ultrahdr.cpp:250-257
  const float white = hdr_tf == UHDR_HIP_TF_PQ ? 10000.0f : 1000.0f;
  memset(md->version, 0, sizeof(md->version));
  strcpy(md->version, "1.0");
  md->maxContentBoost = white / 203.0f;
  md->minContentBoost = 1.0f;
  md->gamma = 1.0f;
  md->offsetSdr = 0.0f;
  md->offsetHdr = 0.0f;
  md->hdrCapacityMin = 1.0f;
  md->hdrCapacityMax = md->maxContentBoost;
}

// ultrahdr.cpp:210-216, for a map of any scale factor, one plane or RGBA8888
void fill_generate_dest(const uhdr_hip_image_t* yuv, uhdr_hip_image_t* dest, size_t scale = 4, bool rgb = false) {
  dest->width = yuv->width / scale;
  dest->height = yuv->height / scale;
  dest->colorGamut = UHDR_HIP_CG_UNSPECIFIED;
  dest->luma_stride = dest->width;
  dest->chroma_data = nullptr;
  dest->chroma_stride = 0;
  dest->pixelFormat = rgb ? UHDR_HIP_PIX_FMT_RGBA8888 : UHDR_HIP_PIX_FMT_MONOCHROME;
}

// bytes encodeGain (gainmapmath.cpp:529-541) yields for a gain clamped to min / max, evaluated with the
// host libm exactly as the reference does, and the scale of the in-range fast path
void encode_constants(float min_boost, float max_boost, float l2min, float l2max, double* scale, uint32_t* bmin,
                      uint32_t* bmax) {
  const double den = (double)(l2max - l2min);
  if (!(den > 0.0)) {   // maxContentBoost == minContentBoost (the _md generate accepts it): every gain is on a clamp and t is 0 / 0;
    *scale = 0.0;       // byte 0, not a NaN cast to an integer
    *bmin = *bmax = 0u;
    return;
  }
  *scale = (double)255.0f / den;
  *bmin = (uint8_t)((std::log2((double)min_boost) - (double)l2min) / den * (double)255.0f);
  *bmax = (uint8_t)((std::log2((double)max_boost) - (double)l2min) / den * (double)255.0f);
}

GenConsts generate_consts(int sdr_gamut, int hdr_gamut, int hdr_tf, int sdr_is_601, size_t w, size_t h,
                          const uhdr_hip_metadata_t& md) {
  GenConsts c;
  const YuvRgb s = yuv_rgb_coeffs(sdr_is_601 ? UHDR_HIP_CG_P3 : sdr_gamut);  // ultrahdr.cpp:267-286
  const YuvRgb hh = yuv_rgb_coeffs(hdr_gamut);                               // :288-302
  c.sdr_cr = s.cr; c.sdr_gcb = s.gcb; c.sdr_gcr = s.gcr; c.sdr_cb = s.cb;
  c.hdr_cr = hh.cr; c.hdr_gcb = hh.gcb; c.hdr_gcr = hh.gcr; c.hdr_cb = hh.cb;
  float l[3];
  luminance_coeffs(sdr_gamut, l);  // the SDR gamut's luminance is used for BOTH images (:324,330)
  c.lum_r = l[0]; c.lum_g = l[1]; c.lum_b = l[2];
  const float* gm = hdr_conversion(sdr_gamut, hdr_gamut);
  c.gm_identity = gm == nullptr;
  for (int i = 0; i < 9; ++i) c.gm[i] = gm ? gm[i] : (i % 4 == 0 ? 1.0f : 0.0f);
  c.hdr_white_nits = hdr_tf == UHDR_HIP_TF_PQ ? 10000.0f : 1000.0f;
  c.min_boost = md.minContentBoost;
  c.max_boost = md.maxContentBoost;
  c.log2_min = (float)std::log2((double)md.minContentBoost);  // ultrahdr.cpp:259-260
  c.log2_max = (float)std::log2((double)md.maxContentBoost);
  encode_constants(c.min_boost, c.max_boost, c.log2_min, c.log2_max, &c.enc_scale, &c.enc_byte_min, &c.enc_byte_max);
  c.width = (uint32_t)w; c.height = (uint32_t)h;
  c.map_w = (uint32_t)(w / 4); c.map_h = (uint32_t)(h / 4);
  c.stat_keys = nullptr;
  c.stat_stride = 2;
  c.stat_ws = nullptr;
  c.stat_out = nullptr;
  c.stat_spread = 0u;
  c.stat_slots = 0u;
  c.lut = nullptr;
  c.bias4096 = 4096.0f;
  // f32 pre-filter (gen_pair; error budget in DESIGN.md section 5): the fast gain is within kRel of the exact one
  // (3.3e-6 by analysis on top of the exhaustively measured transfer-function errors), v_log_f32 within kLogAbs of
  // log2 on [0.25, 64]; the float evaluation of the code value adds < 2.5e-5.  x1.25 on top.
  // PQ: the f32 inverse OETF (pq_inv_oetf_fast) is within 3.4e-6 instead of 3.4e-7 (the outer power multiplies every error by 6.28):
  // HDR luminance <= 1.82 x 3.4e-6 + 1.5e-6, ratio <= 9e-6.  Its code scale is smaller (log2 range 5.6 instead of 2.3), so the
  // distance in code units comes out the same.
  const double kRel = hdr_tf == UHDR_HIP_TF_PQ ? 1.0e-5 : 4.0e-6, kLogAbs = 5.0e-7;
  c.flt_scale = (float)c.enc_scale;
  c.flt_delta = (float)(1.25 * (c.enc_scale * (kRel * 1.4426950408889634 + kLogAbs) + 4.0e-5));
  c.flt_lo = (float)((double)c.min_boost * (1.0 - 2.0 * kRel));
  c.flt_hi = (float)((double)c.max_boost * (1.0 + 2.0 * kRel));
  c.flt_gain_rel = (float)(2.0 * kRel);
  return c;
}

GenImage gen_image(const uhdr_hip_image_t& yuv, const uhdr_hip_image_t& p010, void* map) {
  GenImage g;
  g.y = static_cast<const uint8_t*>(yuv.data);
  g.u = static_cast<const uint8_t*>(yuv.chroma_data);
  g.hy = static_cast<const uint16_t*>(p010.data);
  g.huv = static_cast<const uint16_t*>(p010.chroma_data);
  g.map = static_cast<uint8_t*>(map);
  g.y_stride = (uint32_t)yuv.luma_stride;
  g.c_stride = (uint32_t)yuv.chroma_stride;
  g.hy_stride = (uint32_t)row_stride(p010);
  g.huv_stride = (uint32_t)p010.chroma_stride;
  return g;
}
bool gen_aligned(const GenImage& g, uint32_t w, uint32_t h) {
  const uint8_t* v = g.u + (size_t)g.c_stride * (h / 2u);
  if ((uint64_t)g.hy_stride * h >= (1ull << 31) || (uint64_t)g.y_stride * h >= (1ull << 32)) return false;  // 32-bit offsets
  return (w % 8u == 0) && al(g.hy, 16) && g.hy_stride % 8u == 0 && al(g.huv, 16) && g.huv_stride % 8u == 0 &&
         al(g.y, 8) && g.y_stride % 8u == 0 && al(g.u, 4) && al(v, 4) && g.c_stride % 4u == 0 && al(g.map, 2);
}
// The chunk of the generate family from image i on (form_chunk): equal size and gamuts; the class is gen_aligned and the call's
// own condition on top, also(slot) -- an 8-byte RGBA pair, the scaled call's strip, or no_more.  map_of(j): where image j's map goes.
bool no_more(const GenImage&) { return true; }
bool rgba_pair_aligned(const GenImage& g) { return al(g.map, 8); }   // (the RGBA pair of a thread is one 8-byte store)
template <class MapOf, class Also>
Chunk gen_chunk(int i, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, GenBatch& b, MapOf map_of, Also also) {
  const uhdr_hip_image_t& y0 = yuvs[i];
  const uhdr_hip_image_t& p0 = p010s[i];
  return form_chunk(i, n, kMaxChunk,
                    [&](int j) {
                      return yuvs[j].width == y0.width && yuvs[j].height == y0.height && yuvs[j].colorGamut == y0.colorGamut &&
                             p010s[j].colorGamut == p0.colorGamut;
                    },
                    [&](int j, int m) {
                      b.img[m] = gen_image(yuvs[j], p010s[j], map_of(j));
                      return gen_aligned(b.img[m], (uint32_t)y0.width, (uint32_t)y0.height) && also(b.img[m]);
                    });
}
// ... with the maps in the destination images, whose descriptors the members of the chunk then receive
template <class Also>
Chunk gen_chunk(int i, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, uhdr_hip_image_t* dests, GenBatch& b, Also also,
                size_t scale = 4, bool rgb = false) {
  const Chunk ch = gen_chunk(i, n, yuvs, p010s, b, [&](int j) { return dests[j].data; }, also);
  for (int k = 0; k < ch.m; ++k) fill_generate_dest(&yuvs[i + k], &dests[i + k], scale, rgb);
  return ch;
}
// The chunk of the packed generate family from pair i on: equal size and gamuts; the class is 16-byte row pieces of both images (a
// dword format: 4 pixels, F16: 2), a width of whole pairs' blocks and a map -- map_of(j), or pair j's gains -- on map_align bytes
template <class MapOf>
Chunk packed_chunk(int i, int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, bool f16, PackedBatch& b, MapOf map_of,
                   size_t map_align) {
  const uhdr_hip_image_t& s0 = sdrs[i];
  return form_chunk(i, n, kMaxChunk,
                    [&](int j) {
                      return sdrs[j].width == s0.width && sdrs[j].height == s0.height && sdrs[j].colorGamut == s0.colorGamut &&
                             hdrs[j].colorGamut == hdrs[i].colorGamut;
                    },
                    [&](int j, int m) {
                      PackedImage& p = b.img[m];
                      p.sdr = static_cast<const uint32_t*>(sdrs[j].data);
                      p.hdr = hdrs[j].data;
                      p.map = static_cast<uint8_t*>(map_of(j));
                      p.sdr_stride = (uint32_t)row_stride(sdrs[j]);
                      p.hdr_stride = (uint32_t)row_stride(hdrs[j]);
                      return s0.width % 8u == 0 && al(p.sdr, 16) && p.sdr_stride % 4u == 0 && al(p.hdr, 16) &&
                             p.hdr_stride % (f16 ? 2u : 4u) == 0 && al(p.map, map_align);
                    });
}

// ---- content-adaptive generate ---------------------------------------------------------------------
// the range rule of include/uhdr_hip.h, in f32; k_adaptive_consts performs the same operations on the device
float adaptive_cap(int hdr_tf) { return (hdr_tf == UHDR_HIP_TF_PQ ? 10000.0f : 1000.0f) / 203.0f; }
void adaptive_range(int hdr_tf, float g_min, float g_max, float* lo, float* hi) {
  *lo = fminf(fmaxf(g_min, 0.25f), 1.0f);
  *hi = fminf(fmaxf(g_max, 1.0625f), adaptive_cap(hdr_tf));
}
void fill_adaptive_metadata(float lo, float hi, uhdr_hip_metadata_t* md) {
  memset(md->version, 0, sizeof(md->version));
  strcpy(md->version, "1.0");
  md->maxContentBoost = hi;
  md->minContentBoost = lo;
  md->gamma = 1.0f;
  md->offsetSdr = 0.0f;
  md->offsetHdr = 0.0f;
  md->hdrCapacityMin = lo;
  md->hdrCapacityMax = hi;
}
bool valid_boost_scope(int scope) { return scope == UHDR_HIP_BOOST_PER_IMAGE || scope == UHDR_HIP_BOOST_PER_CALL; }
// hdr_peak_nits of the tone-mapped SDR base image: 0 (the headroom is measured) or a positive finite figure
bool valid_peak_nits(float peak) { return peak >= 0.0f && std::isfinite(peak); }

// the caller's workspace: the images' key pairs, their constants, then every image's gains (gain_bytes per map pixel: 4, the packed
// call's RGB maps 12), each piece a multiple of 256 bytes
struct AdaptLayout {
  size_t keys = 0, consts = 0, total = 0;
  std::vector<size_t> gains;
};
AdaptLayout adaptive_layout(int n, const uhdr_hip_image_t* yuvs, size_t gain_bytes = sizeof(float)) {
  AdaptLayout l;
  if (n <= 0) return l;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  l.keys = 0;
  l.consts = up(sizeof(uint32_t) * 2 * (size_t)n);
  size_t o = l.consts + up(sizeof(AdaptConsts) * (size_t)n);
  l.gains.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    l.gains[(size_t)i] = o;
    o += up(gain_bytes * (yuvs[i].width / 4) * (yuvs[i].height / 4));
  }
  l.total = o;
  return l;
}

// The two passes of uhdr_hip_generate_gainmap_adaptive_batch on checked arguments, enqueue only.  carry_in / carry_out (DEVICE, two
// key words, or null; PER_CALL only): the pooled extremes of earlier calls join this call's, and the joined pair is left behind --
// a statistic taken over several calls.  encode == false stops after the constants: the call only measures.
// What does not depend on the input form: the workspace's pieces, the keys' init, pass 1 chunk by chunk -- pass1(i, c, gains_of)
// forms the chunk from image i on, launches it and returns its size (or a negative hipError_t); c arrives with the image's constants
// and its key words, gains_of(j) is where image j's gains go --, the constants, and pass 2 over the same chunks (rgb: RGBA maps from
// three gains per map pixel).  sdrs: the images whose sizes and gamuts the chunks follow (the yuv420 or the RGBA8888 ones).
template <class Pass1>
int adaptive_passes(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, int hdr_tf, uhdr_hip_image_t* dests, int sdr_is_601,
                    bool rgb, const AdaptLayout& lay, int boost_scope, float* content_minmax, float* boost_range, void* workspace,
                    const uint32_t* carry_in, uint32_t* carry_out, bool encode, hipStream_t s, Pass1 pass1) {
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + lay.keys);
  AdaptConsts* consts = reinterpret_cast<AdaptConsts*>(ws + lay.consts);
  uhdr_hip_metadata_t md;
  fill_generate_metadata(hdr_tf, &md);   // (pass 1 stores gains, no bytes: what generate_consts derives from the range is not used)
  HIP_TRY(launch_adaptive_init(keys, 2u * (uint32_t)n, s));
  std::vector<std::pair<int, int>> chunks;   // (first image, images) of every launch
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& y0 = sdrs[i];
    GenConsts c = generate_consts(y0.colorGamut, hdrs[i].colorGamut, hdr_tf, sdr_is_601, y0.width, y0.height, md);
    c.stat_keys = keys + 2 * i;
    c.stat_stride = 2;
    const int m = pass1(i, c, [&](int j) { return ws + lay.gains[(size_t)j]; });
    if (m < 0) { set_err("adaptive pass 1", (hipError_t)-m); return UHDR_HIP_UNKNOWN_ERROR; }
    chunks.emplace_back(i, m);
    i += m;
  }
  HIP_TRY(launch_adaptive_consts(keys, n, boost_scope == UHDR_HIP_BOOST_PER_CALL ? 1 : 0, adaptive_cap(hdr_tf), consts, content_minmax,
                                 boost_range, carry_in, carry_out, s));
  if (!encode) return UHDR_HIP_NO_ERROR;
  for (const auto& ch : chunks) {
    EncGainBatch eb;
    for (int k = 0; k < ch.second; ++k) {
      const size_t j = (size_t)(ch.first + k);
      eb.img[k].gains = reinterpret_cast<const float*>(ws + lay.gains[j]);
      eb.img[k].map = static_cast<uint8_t*>(dests[j].data);
      fill_generate_dest(&sdrs[j], &dests[j], 4, rgb);
    }
    const uhdr_hip_image_t& y0 = sdrs[ch.first];
    const uint32_t pixels = (uint32_t)((y0.width / 4) * (y0.height / 4));
    if (rgb) HIP_TRY(launch_encode_gains_rgb(consts + ch.first, eb, ch.second, pixels, s));
    else HIP_TRY(launch_encode_gains(consts + ch.first, eb, ch.second, pixels, s));
  }
  return UHDR_HIP_NO_ERROR;
}
int adaptive_enqueue(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf, uhdr_hip_image_t* dests,
                     int sdr_is_601, int boost_scope, float* content_minmax, float* boost_range, void* workspace,
                     const uint32_t* carry_in, uint32_t* carry_out, bool encode, hipStream_t s) {
  if (n <= 0) return UHDR_HIP_NO_ERROR;
  return adaptive_passes(n, yuvs, p010s, hdr_tf, dests, sdr_is_601, false, adaptive_layout(n, yuvs), boost_scope, content_minmax, boost_range,
                         workspace, carry_in, carry_out, encode, s, [&](int i, const GenConsts& c, auto gains_of) {
                           GenBatch b;
                           const Chunk ch = gen_chunk(i, n, yuvs, p010s, b, gains_of, no_more);
                           const hipError_t e = launch_generate_gains(c, b, ch.m, hdr_tf, ch.cls, s);
                           return e == hipSuccess ? ch.m : -(int)e;
                         });
}
// The same for packed RGBA pairs: pass 1 is k_generate_packed_gains over the packed call's chunks; an RGB
// map keeps three gains per map pixel
size_t packed_gain_bytes(bool rgb) { return sizeof(float) * (rgb ? 3 : 1); }
int packed_adaptive_enqueue(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, int hdr_tf, uhdr_hip_image_t* dests, bool rgb,
                            int boost_scope, float* content_minmax, float* boost_range, void* workspace, const uint32_t* carry_in,
                            uint32_t* carry_out, bool encode, hipStream_t s) {
  if (n <= 0) return UHDR_HIP_NO_ERROR;
  const bool f16 = hdrs[0].pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16;
  return adaptive_passes(n, sdrs, hdrs, hdr_tf, dests, 0, rgb, adaptive_layout(n, sdrs, packed_gain_bytes(rgb)), boost_scope, content_minmax,
                         boost_range, workspace, carry_in, carry_out, encode, s, [&](int i, const GenConsts& c, auto gains_of) {
                           PackedBatch b;
                           const Chunk ch = packed_chunk(i, n, sdrs, hdrs, f16, b, gains_of, 16);   // (a piece of the workspace: always)
                           const hipError_t e = launch_generate_packed_gains(c, b, ch.m, hdr_tf, f16, ch.cls, rgb, s);
                           return e == hipSuccess ? ch.m : -(int)e;
                         });
}

// ---- FAST apply's line-segment tables (uhdr_kernels.h, k_apply_s4) ---------------------------------
// An entry is the chord of the function over its cell, lowered by half its largest deviation, as (c0, c1): f ~ c0 + c1 * argument.
template <class F>
void chord(F f, double lo, double hi, double* c0, double* c1) {
  *c1 = (f(hi) - f(lo)) / (hi - lo);
  *c0 = f(lo) - *c1 * lo;
  double dev = 0.0;
  for (int k = 1; k < 32; ++k) { const double x = lo + (hi - lo) * k / 32.0; const double d = f(x) - (*c0 + *c1 * x); if (std::fabs(d) > std::fabs(dev)) dev = d; }
  *c0 += 0.5 * dev;
}
// Stage 1: T(c) = srgbInvOetf(c)^g (gainmapmath.cpp:149-155).  Cell j holds the arguments whose half-precision conversion, rounded
// toward zero, has the bits j << 3 | 0..7: e = j >> 7, m = j & 127: [2^(e-15) (1 + m/128), 2^(e-15) (1 + (m+1)/128)) for e >= 1, the
// subnormal slots [m, m+1) 2^-21 for e = 0 (no input of the kernel other than 0 falls below 2^-17: (y + k dv) / 255).
void f16_cell(uint32_t j, double* lo, double* hi) {
  const uint32_t e = j >> 7, m = j & 127u;
  if (e == 0) { *lo = std::ldexp((double)m, -21); *hi = std::ldexp((double)(m + 1u), -21); return; }
  *lo = std::ldexp(1.0 + m / 128.0, (int)e - 15);
  *hi = std::ldexp(1.0 + (m + 1u) / 128.0, (int)e - 15);
}
// ... and for g < 1 cell j = (e & 31) << 4 | m with e the biased exponent and m the top four mantissa bits:
// [2^(e-127) (1 + m/16), 2^(e-127) (1 + (m+1)/16)), e = 96 .. 127.  Five exponent bits are enough: a channel is y / 255 plus chroma
// terms, operands of magnitude >= 2^-8, so a non-zero result is a multiple of 2^-31 -- the kernel's inputs are 0 or lie in
// [2^-31, 1].  Cell 0 serves the input 0 (and the sliver above 2^-31): a line through the origin.
void f32_cell16(uint32_t j, double* lo, double* hi) {
  const uint32_t e = 96u + (j >> 4), m = j & 15u;
  *lo = std::ldexp(1.0 + m / 16.0, (int)e - 127);
  *hi = std::ldexp(1.0 + (m + 1u) / 16.0, (int)e - 127);
}
void build_stage1(double g, float* out) {
  const double thr = (double)0.04045f;
  auto eotf = [&](double x) { return x <= thr ? x / (double)12.92f : std::pow((x + (double)0.055f) / (double)1.055f, 2.4); };
  auto f = [&](double x) { return g == 1.0 ? eotf(x) : std::pow(eotf(x), g); };
  const uint32_t cells = (g == 1.0 ? kTabS1Bytes : kTabS1PowBytes) / 8u;
  for (uint32_t j = 0; j < cells; ++j) {
    double lo, hi, c0, c1;
    if (g == 1.0) f16_cell(j, &lo, &hi); else f32_cell16(j, &lo, &hi);
    if (g == 1.0 && hi <= thr) { c0 = 0.0; c1 = 1.0 / (double)12.92f; }
    else if (lo >= 1.0) { c0 = 1.0; c1 = 0.0; }
    else if (j == 0) { c0 = 0.0; c1 = f(hi) / hi; }   // T(0) = 0 exactly
    else chord(f, lo, hi, &c0, &c1);
    out[2 * j] = (float)c0; out[2 * j + 1] = (float)c1;
  }
}
// Stage 2: the 10-bit code (colorToRgba1010102, gainmapmath.cpp:722-727: truncation of OETF * 1023) as a function of
// s = 2 + 2u, cell k = [2 + k/64, 2 + (k+1)/64), cell 128 = s >= 4 (u = 1, nothing above it is reached).  The entry evaluates
// to -(2 + code 2^-22); the kernel's fma rounds toward zero, i.e. truncates the code, and the bits of the result are
// 0xC0000000 | code.  c0 must then be a whole number of half codes (an ulp of [1, 2) is 2^-23), so its fraction is moved into the
// slope: that tilts the line by < 0.002 codes over a cell (the argument stays within 1/256 of the cell's middle, relatively).
// A line never evaluates below 0 (the result would leave the [2, 4) binade): cell 0 passes through (2, 0) exactly.
template <class F>
void build_stage2(F code_of_u, float* out) {
  for (uint32_t k = 0; k < kTabS2Cells; ++k) {
    const double lo = 2.0 + k / 64.0, hi = 2.0 + (k + 1u) / 64.0;
    auto f = [&](double s) { return code_of_u(std::min(1.0, 0.5 * (s - 2.0))); };
    float c0f = -2.0f, c1f = 0.0f;                       // a cell whose codes all truncate to 0
    if (k == kTabS2Cells - 1u) c0f = (float)(-2.0 - std::ldexp(1023.0, -22));
    else if (f(hi) >= 0.99) {
      double c0, c1;
      chord(f, lo, hi, &c0, &c1);
      c0 += 1.0 / 256.0;                                 // margin: the line stays above 0 after the steps below
      // -2 - n 2^-22 must be a float: n a whole number of codes when the magnitude is in [2, 4), of half codes when in [1, 2)
      const double n = c0 < 0.0 ? std::nearbyint(2.0 * c0) / 2.0 : std::nearbyint(c0);
      c1 += (c0 - n) / (0.5 * (lo + hi));
      c0f = (float)(-2.0 - std::ldexp(n, -22));
      c1f = (float)(-std::ldexp(c1, -22));
      auto at = [&](double s) { return -(((double)c1f * s + (double)c0f) + 2.0) * 4194304.0; };
      for (int it = 0; it < 4096 && at(lo) < 0.0; ++it) c1f = std::nextafter(c1f, -INFINITY);
      if (at(lo) < 0.0) { c0f = -2.0f; c1f = 0.0f; }
    }
    out[2 * k] = c0f; out[2 * k + 1] = c1f;
  }
}
void build_line_tables(std::vector<float>& tab) {
  tab.assign(kTabEnd - kTabS1Lin, 0.0f);
  const double m1 = (double)(2610.0f / 16384.0f), m2 = (double)(2523.0f / 4096.0f * 128.0f);
  const double k1 = (double)(3424.0f / 4096.0f), k2 = (double)(2413.0f / 4096.0f * 32.0f), k3 = (double)(2392.0f / 4096.0f * 32.0f);
  build_stage1(1.0, tab.data() + (kTabS1Lin - kTabS1Lin));
  build_stage1(0.5, tab.data() + (kTabS1Hlg - kTabS1Lin));
  build_stage1(m1, tab.data() + (kTabS1Pq - kTabS1Lin));
  // HLG OETF (gainmapmath.cpp:257-267) of x = u^2; PQ OETF (:305-314) of x = u^(1/m1), i.e. of p = u directly
  auto hlg = [](double u) { const double x = u * u; return 1023.0 * (x <= 1.0 / 12.0 ? std::sqrt(3.0) * u : (double)0.17883277f * std::log(12.0 * x - (double)0.28466892f) + (double)0.55991073f); };
  auto pq = [&](double p) { return p <= 0.0 ? 0.0 : 1023.0 * std::pow((k1 + k2 * p) / (1.0 + k3 * p), m2); };
  build_stage2(hlg, tab.data() + (kTabS2Hlg - kTabS1Lin));
  build_stage2(pq, tab.data() + (kTabS2Pq - kTabS1Lin));
}

// ---- apply ---------------------------------------------------------------------------------------
// checks of ultrahdr.cpp:364-406 in order
int validate_apply(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* map, const uhdr_hip_metadata_t* md,
                   const uhdr_hip_image_t* dest) {
  if (yuv == nullptr || map == nullptr || md == nullptr || dest == nullptr || yuv->data == nullptr ||
      yuv->chroma_data == nullptr || map->data == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;
  if (strncmp(md->version, "1.0", sizeof(md->version)) != 0) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->gamma != 1.0f) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->offsetSdr != 0.0f || md->offsetHdr != 0.0f) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->hdrCapacityMin != md->minContentBoost || md->hdrCapacityMax != md->maxContentBoost)
    return UHDR_HIP_ERROR_BAD_METADATA;
  if (map->width == 0 || map->height == 0) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;  // (ref: division by zero)
  if (yuv->width % map->width != 0 || yuv->height % map->height != 0)
    return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
  if (yuv->width * map->height != yuv->height * map->width) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
  return UHDR_HIP_NO_ERROR;
}
// ---- general metadata: gamma, offsets, HDR capacity (the *_md calls) --------
// what validate_apply accepts of the metadata's numbers: the reference's applyGainMap computes nothing else
bool md_degenerate(const uhdr_hip_metadata_t& md) {
  return md.gamma == 1.0f && md.offsetSdr == 0.0f && md.offsetHdr == 0.0f && md.hdrCapacityMin == md.minContentBoost &&
         md.hdrCapacityMax == md.maxContentBoost;
}
int validate_md(const uhdr_hip_metadata_t* md) {
  if (strncmp(md->version, "1.0", sizeof(md->version)) != 0) return UHDR_HIP_ERROR_BAD_METADATA;
  const float f[7] = {md->maxContentBoost, md->minContentBoost, md->gamma, md->offsetSdr, md->offsetHdr, md->hdrCapacityMin, md->hdrCapacityMax};
  for (float v : f)
    if (!std::isfinite(v)) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->maxContentBoost < md->minContentBoost || md->minContentBoost <= 0.0f) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->hdrCapacityMax < md->hdrCapacityMin || md->hdrCapacityMin <= 0.0f) return UHDR_HIP_ERROR_BAD_METADATA;
  if (md->offsetSdr < 0.0f || md->offsetHdr < 0.0f || md->gamma <= 0.0f) return UHDR_HIP_ERROR_BAD_METADATA;
  return UHDR_HIP_NO_ERROR;
}

// ---- the argument checks of the generate batch calls, each order written once (tests/test_*_cpu.py hold the orders) ----------------
// dest_align: what a destination's data pointer must be a multiple of (4 for an RGBA map); hook (or null): a further check of the
// call's own on every image, behind the others of that image
using ImageHook = std::function<int(const uhdr_hip_image_t&)>;
bool null_dest(const uhdr_hip_image_t& d, size_t dest_align) { return d.data == nullptr || !al(d.data, dest_align); }
// Against the reference's metadata (uhdr_hip_generate_gainmap_batch_ex and the calls that take its order): the call's pointers; per
// image validate_generate, then the map buffer the C-ABI's caller provides, then the hook; the transfer function last (n == 0)
int check_generate(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf, const uhdr_hip_metadata_t* md,
                   const uhdr_hip_image_t* dests, size_t dest_align, const ImageHook& hook = nullptr) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || p010s == nullptr || dests == nullptr)) || md == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    int rc = validate_generate(&yuvs[i], &p010s[i], hdr_tf, md, &dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
    if (null_dest(dests[i], dest_align)) return UHDR_HIP_ERROR_BAD_PTR;
    if (hook && (rc = hook(yuvs[i])) != UHDR_HIP_NO_ERROR) return rc;
  }
  return tf_known(hdr_tf) ? UHDR_HIP_NO_ERROR : UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
}
// Against the caller's metadata (uhdr_hip_generate_gainmap_md_batch's order): every image's pointers, the metadata, then per image
// validate_generate and the hook; the transfer function last
int check_generate_md(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf, const uhdr_hip_metadata_t* md,
                      const uhdr_hip_image_t* dests, size_t dest_align, const ImageHook& hook = nullptr) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || p010s == nullptr || dests == nullptr)) || md == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    if (yuvs[i].data == nullptr || yuvs[i].chroma_data == nullptr || p010s[i].data == nullptr || p010s[i].chroma_data == nullptr ||
        null_dest(dests[i], dest_align))
      return UHDR_HIP_ERROR_BAD_PTR;
  }
  int rc = validate_md(md);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  for (int i = 0; i < n; ++i) {
    if ((rc = validate_generate(&yuvs[i], &p010s[i], hdr_tf, md, &dests[i])) != UHDR_HIP_NO_ERROR) return rc;
    if (hook && (rc = hook(yuvs[i])) != UHDR_HIP_NO_ERROR) return rc;
  }
  return tf_known(hdr_tf) ? UHDR_HIP_NO_ERROR : UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
}
// W and d of include/uhdr_hip.h, in double (D >= 1, possibly infinite; the metadata has passed validate_md)
void md_weight(const uhdr_hip_metadata_t& md, float max_display_boost, double* w, double* d) {
  const double D = (double)max_display_boost, hmin = (double)md.hdrCapacityMin, hmax = (double)md.hdrCapacityMax;
  if (md.hdrCapacityMax == md.hdrCapacityMin) *w = D >= hmax ? 1.0 : 0.0;
  else *w = std::fmin(std::fmax((std::log2(D) - std::log2(hmin)) / (std::log2(hmax) - std::log2(hmin)), 0.0), 1.0);
  *d = std::fmin(D, hmax);
}
AppMdConsts apply_md_consts(const uhdr_hip_metadata_t& md, float max_display_boost) {
  double w, d;
  md_weight(md, max_display_boost, &w, &d);
  const double l2min = std::log2((double)md.minContentBoost), l2max = std::log2((double)md.maxContentBoost);
  AppMdConsts m;
  m.A = (float)((l2max - l2min) * w);
  m.B = (float)(l2min * w - std::log2(d));
  m.inv_gamma = (float)(1.0 / (double)md.gamma);
  m.off_sdr = md.offsetSdr;
  m.off_hdr_d = (float)((double)md.offsetHdr / d);
  m.gamma_on = md.gamma != 1.0f ? 1u : 0u;
  return m;
}
// the encode constants of uhdr_hip_generate_gainmap_md_batch beside generate_consts': the offsets in nits and, for gamma != 1, the
// bytes of a gain on either clamp, evaluated as the header states the rule (libm, double)
GenMdConsts generate_md_consts(const uhdr_hip_metadata_t& md, const GenConsts& c) {
  GenMdConsts m;
  m.off_sdr_nits = md.offsetSdr * 203.0f;
  m.off_hdr_nits = md.offsetHdr * 203.0f;
  m.gamma_on = md.gamma != 1.0f ? 1u : 0u;
  m.gamma = (double)md.gamma;
  m.den = (double)(c.log2_max - c.log2_min);
  auto byte_of = [&](float boost) -> uint32_t {
    const double t = (std::log2((double)boost) - (double)c.log2_min) / m.den;
    if (!(t > 0.0)) return 0u;
    return (uint32_t)(uint8_t)std::fmin(std::pow(t, m.gamma) * 255.0, 255.0);
  };
  if (!(m.den > 0.0)) {   // maxContentBoost == minContentBoost: every gain is on a clamp, byte 0 (as encode_constants answers)
    m.byte_min = m.byte_max = 0u;
  } else {
    m.byte_min = byte_of(md.minContentBoost);
    m.byte_max = byte_of(md.maxContentBoost);
  }
  return m;
}

bool apply_writes(int fmt) {
  return fmt == UHDR_HIP_OUTPUT_HDR_LINEAR || fmt == UHDR_HIP_OUTPUT_HDR_PQ || fmt == UHDR_HIP_OUTPUT_HDR_HLG ||
         fmt == UHDR_HIP_OUTPUT_HDR_LINEAR_RGB_10BIT;
}
size_t apply_bpp(int fmt) {
  return fmt == UHDR_HIP_OUTPUT_HDR_LINEAR ? 8 : fmt == UHDR_HIP_OUTPUT_HDR_LINEAR_RGB_10BIT ? 6 : 4;
}
AppConsts apply_consts(const uhdr_hip_image_t& yuv, const uhdr_hip_image_t& map, const uhdr_hip_metadata_t& md,
                       float max_display_boost, const float* idw) {
  AppConsts c;
  c.width = (uint32_t)yuv.width; c.height = (uint32_t)yuv.height;
  c.map_w = (uint32_t)map.width; c.map_h = (uint32_t)map.height;
  c.scale = (uint32_t)(yuv.width / map.width);                                    // ultrahdr.cpp:409
  c.display_boost = (std::min)(max_display_boost, md.maxContentBoost);            // :415
  c.inv_display_boost = 1.0f / c.display_boost;
  c.max_boost = md.maxContentBoost;
  c.inv_max_boost = 1.0f / md.maxContentBoost;
  c.log2_min_d = std::log2((double)md.minContentBoost);                           // gainmapmath.cpp:551-552
  c.log2_max_d = std::log2((double)md.maxContentBoost);
  c.idw = idw;
  c.lut = nullptr;
  c.lut_boost_factor = c.display_boost > 0 ? c.display_boost / md.maxContentBoost : 1.0f;  // gainmapmath.h:162
  // LUT-mode apply divides (sRGB table value x GainLUT entry) by display_boost.  The table values are 0 or lie in [7e-5, 1], the
  // GainLUT entries between 2^(log2 min x factor) and 2^(log2 max x factor): with the divisor in [2^-20, 2^20] and those exponents
  // within +-40 no operand, quotient or remainder of the division's IEEE expansion leaves the normal range, v_div_scale_f32 rescales
  // nothing and the expansion can run as it stands, two quotients per instruction (k_apply_lut_s4: lut_cell_pk).
  // The quotient is then at most 2^(the larger exponent) / display_boost; below 32768 its index product into a 65536-entry table
  // stays under 2^31 (lut_index_pos: no test for the wild range).
  const double lut_top = std::exp2(std::fmax(c.log2_min_d, c.log2_max_d) * (double)c.lut_boost_factor) / (double)c.display_boost;
  c.lut_plain_div = (c.display_boost >= 0x1p-20f && c.display_boost <= 0x1p20f && std::fabs(c.log2_min_d * (double)c.lut_boost_factor) <= 40.0 &&
                     std::fabs(c.log2_max_d * (double)c.lut_boost_factor) <= 40.0 && lut_top <= 32768.0) ? 1u : 0u;
  // FAST scale-4 kernel: factor/display_boost = 2^(gain*A + B); weights pre-multiplied by A / 255 (k_apply_s4)
  const double ratio = (double)c.display_boost / (double)md.maxContentBoost;
  c.fast.A = (float)((c.log2_max_d - c.log2_min_d) * ratio);
  c.fast.B = (float)(c.log2_min_d * ratio - std::log2((double)c.display_boost));
  c.fast.A255 = (float)((c.log2_max_d - c.log2_min_d) * ratio / 255.0);
  std::vector<float> t;
  build_idw_tables(4, t);
  for (int oy = 0; oy < 4; ++oy)
    for (int pr = 0; pr < 2; ++pr)
      for (int k = 1; k < 4; ++k)
        for (int j = 0; j < 2; ++j)
          c.fast.wD[oy][pr][k - 1][j] = t[oy * 16 + (2 * pr + j) * 4 + k];   // the weight itself: launch_apply_t multiplies by the final A / 255
  c.tab = nullptr;
  c.ex_ws = nullptr;
  c.ex_cap = 0;
  c.cells_per_thread = 8;
  c.step_x = c.step_y = 0;
  c.map_stride = c.map_w;
  return c;
}
// The chroma geometry of an 8-bit YCbCr image by its pixelFormat: the shifts from a pixel to its chroma sample and the rows of a
// chroma plane (Cr sits chroma_stride * rows behind Cb).  YUV444 / YUV422 / YUV440 are what the any-sampling decode returns
// (libjpeg's downsampled sizes: rounded up); every other value is 4:2:0 with the reference's height / 2 rows.
struct ChromaGeom { uint32_t csx, csy; size_t rows; };
ChromaGeom chroma_geom(const uhdr_hip_image_t& yuv) {
  switch (yuv.pixelFormat) {
    case UHDR_HIP_PIX_FMT_YUV444: return ChromaGeom{0u, 0u, yuv.height};
    case UHDR_HIP_PIX_FMT_YUV422: return ChromaGeom{1u, 0u, yuv.height};
    case UHDR_HIP_PIX_FMT_YUV440: return ChromaGeom{0u, 1u, (yuv.height + 1) / 2};
    default: return ChromaGeom{1u, 1u, yuv.height / 2};
  }
}
bool is_420(const uhdr_hip_image_t& yuv) { const ChromaGeom g = chroma_geom(yuv); return g.csx == 1u && g.csy == 1u; }
AppImage app_image(const uhdr_hip_image_t& yuv, const uhdr_hip_image_t& map, void* dst) {
  AppImage a;
  const ChromaGeom g = chroma_geom(yuv);
  a.y = static_cast<const uint8_t*>(yuv.data);
  a.u = static_cast<const uint8_t*>(yuv.chroma_data);
  a.v = a.u + yuv.chroma_stride * g.rows;
  a.csx = g.csx; a.csy = g.csy;
  a.map = static_cast<const uint8_t*>(map.data);
  a.dst = dst;
  a.y_stride = (uint32_t)yuv.luma_stride;
  a.c_stride = (uint32_t)yuv.chroma_stride;
  return a;
}
bool app_fast_s4(const AppConsts& c, const AppImage& a) {
  if (a.csx != 1u || a.csy != 1u) return false;   // the scale-4 kernels load 4:2:0 chroma
  // the fast kernels index planes with 32-bit byte offsets (the widest output is 8 bytes per pixel)
  if ((uint64_t)a.y_stride * c.height >= (1ull << 32) || (uint64_t)c.width * c.height >= (1ull << 29)) return false;
  return c.scale == 4 && c.width == 4u * c.map_w && c.height == 4u * c.map_h && al(a.y, 4) && a.y_stride % 4u == 0 &&
         al(a.u, 2) && al(a.v, 2) && a.c_stride % 2u == 0 && al(a.dst, 16);
}
void fill_apply_dest(const uhdr_hip_image_t* yuv, uhdr_hip_image_t* dest) {  // ultrahdr.cpp:411-413
  dest->width = yuv->width;
  dest->height = yuv->height;
  dest->colorGamut = yuv->colorGamut;
}
// The chunk of the apply family from image i on (form_chunk): equal image and map sizes and, for RGBA maps (equal_stride), equal map
// strides.  fast_of: the one-plane call's constants -- its class is app_fast_s4 --, or null: one class.  The members' destination
// descriptors are filled.
Chunk app_chunk(int i, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps, uhdr_hip_image_t* dests, AppBatch& b,
                const AppConsts* fast_of, bool equal_stride) {
  const uhdr_hip_image_t& y0 = yuvs[i];
  const uhdr_hip_image_t& m0 = maps[i];
  const Chunk ch = form_chunk(i, n, kMaxChunk,
                              [&](int j) {
                                return yuvs[j].width == y0.width && yuvs[j].height == y0.height && maps[j].width == m0.width &&
                                       maps[j].height == m0.height && (!equal_stride || row_stride(maps[j]) == row_stride(m0));
                              },
                              [&](int j, int m) {
                                b.img[m] = app_image(yuvs[j], maps[j], dests[j].data);
                                return fast_of == nullptr || app_fast_s4(*fast_of, b.img[m]);
                              });
  for (int k = 0; k < ch.m; ++k) fill_apply_dest(&yuvs[i + k], &dests[i + k]);
  return ch;
}
// The chunks of the apply calls that have one kernel per chunk and no class (RGBA maps, general metadata), on checked arguments:
// launch(constants, batch, images) enqueues a chunk and returns its status.  rgba: the maps' rows are luma_stride pixels (0 = width), else `width` bytes.
template <class Launch>
int apply_pixel_chunks(DeviceState* st, hipStream_t s, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps,
                       const uhdr_hip_metadata_t& md, float max_display_boost, uhdr_hip_image_t* dests, bool rgba, bool writes,
                       Launch launch) {
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& y0 = yuvs[i];
    const uhdr_hip_image_t& m0 = maps[i];
    IdwLease table;
    int rc = table.take(st, (int)(y0.width / m0.width), s);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
    AppConsts c = apply_consts(y0, m0, md, max_display_boost, table.idw);
    c.map_stride = (uint32_t)(rgba ? row_stride(m0) : m0.width);
    c.tab = st->lut;
    AppBatch b;
    const int m = app_chunk(i, n, yuvs, maps, dests, b, nullptr, rgba).m;
    if (writes && (rc = launch(c, b, m)) != UHDR_HIP_NO_ERROR) return rc;
    i += m;
  }
  return UHDR_HIP_NO_ERROR;
}

// ---- host staging ----------------------------------------------------------------------------------
int stage_reserve(StageSet* st, int slot, size_t bytes) {
  if (bytes == 0) bytes = 256;
  if (st->stage_bytes[slot] >= bytes) return UHDR_HIP_NO_ERROR;
  if (st->stage[slot]) HIP_TRY(hipFree(st->stage[slot]));
  st->stage[slot] = nullptr;
  st->stage_bytes[slot] = 0;
  HIP_TRY(hipMalloc(&st->stage[slot], bytes));
  st->stage_bytes[slot] = bytes;
  return UHDR_HIP_NO_ERROR;
}
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// one staging set for the duration of a host-memory call
class StageLease {
 public:
  explicit StageLease(DeviceState* st) : st_(st) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (st_->free_sets.empty()) {
      try {
        st_->sets.emplace_back(new StageSet());
        set_ = st_->sets.back().get();
      } catch (const std::bad_alloc&) {
        set_ = nullptr;   // (the caller returns INSUFFICIENT_RESOURCE: nothing may throw through the C boundary)
      }
    } else {
      set_ = st_->free_sets.back();
      st_->free_sets.pop_back();
    }
  }
  ~StageLease() {
    if (set_ == nullptr) return;
    std::lock_guard<std::mutex> lk(g_mu);
    try { st_->free_sets.push_back(set_); } catch (const std::bad_alloc&) {}   // (the set stays owned by st_->sets)
  }
  StageLease(const StageLease&) = delete;
  StageLease& operator=(const StageLease&) = delete;
  StageSet* get() const { return set_; }   // nullptr: out of host memory
 private:
  DeviceState* st_;
  StageSet* set_;
};

// A codec call's private context.  Round 2 serialised every jpeg_* / jpegr_* call of a process behind two mutexes because the calls
// shared the device's staging slots, decoder pool and side stream; a JPEG decode is latency-bound (tens of synchronisation rounds
// of one lane's work each), so two callers on their own streams now overlap almost completely (tests/test_gpu_async.py).
class CodecLease {
 public:
  explicit CodecLease(DeviceState* st) : st_(st) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!st_->free_codec.empty()) {
      ctx_ = st_->free_codec.back();
      st_->free_codec.pop_back();
    } else {
      try {
        st_->free_codec.reserve(st_->codec_sets.size() + 1);   // (so that giving it back cannot fail)
        st_->codec_sets.emplace_back(new DeviceState());
        ctx_ = st_->codec_sets.back().get();
      } catch (const std::bad_alloc&) {
        ctx_ = nullptr;
      }
    }
    if (ctx_) { ctx_->ready = true; ctx_->lut = st_->lut; }
  }
  ~CodecLease() {
    if (ctx_ == nullptr) return;
    std::lock_guard<std::mutex> lk(g_mu);
    st_->free_codec.push_back(ctx_);
  }
  CodecLease(const CodecLease&) = delete;
  CodecLease& operator=(const CodecLease&) = delete;
  DeviceState* get() const { return ctx_; }

 private:
  DeviceState* st_;
  DeviceState* ctx_ = nullptr;
};

// ---- what every batched codec call shares ------------------------------------------------------------------------------------------
// runs fn(lo, hi) over [0, n) on up to 8 host threads
template <class F>
void on_host_threads(int n, F fn) {
  const int nthreads = n >= 2 ? std::min(n, 8) : 1;
  if (nthreads <= 1) { fn(0, n); return; }
  std::vector<std::thread> workers;
  for (int t = 0; t < nthreads; ++t) workers.emplace_back(fn, (int)((long)n * t / nthreads), (int)((long)n * (t + 1) / nthreads));
  for (auto& w : workers) w.join();
}

// the end of a batched call: every file's status into the caller's array (if it gave one), the first error as the call's own
int finish_statuses(const std::vector<int>& st_, int* status) {
  int first = UHDR_HIP_NO_ERROR;
  for (size_t i = 0; i < st_.size(); ++i) { if (status) status[i] = st_[i]; if (first == UHDR_HIP_NO_ERROR) first = st_[i]; }
  return first;
}

// a single JPEG call's mem_space as the batches read it: every value other than UHDR_HIP_MEM_DEVICE means host memory (the batches give
// UHDR_HIP_MEM_DEVICE_TO_HOST and UHDR_HIP_MEM_HOST_TO_DEVICE their split meaning)
int single_mem_space(int mem_space) { return mem_space == UHDR_HIP_MEM_DEVICE ? UHDR_HIP_MEM_DEVICE : UHDR_HIP_MEM_HOST; }

// A round's device workspace and page-locked staging are held to kCodecRoundBytes (a file larger than that gets a round of its own).
// g_round_bytes is the bound run_rounds reads: kCodecRoundBytes unless a test has moved it (uhdr_hip_codec_round_bytes_probe)
constexpr size_t kCodecRoundBytes = size_t(2) << 30;
std::atomic<size_t> g_round_bytes{kCodecRoundBytes};

// The device part of a batched codec call over its `live` files, in their order: a context of the call's own (CodecLease), then greedy
// rounds of at most `cap` files and g_round_bytes -- bytes_of(k) is what file k holds of its round, the first file of a round is
// always admitted --, each through run(ctx, s, first, m).  The first non-zero round status ends the call behind a stream
// synchronisation, so that nothing of the failed round is still writing into the pools, and is returned; files [0, *done) are
// finished, the others (the failed round's and those behind it) are the caller's to mark.  A round that returns 0 must leave the
// stream idle -- every round here ends in compress_to_host's, jpeg_decode_round's or jpegr_decode_round's synchronisation --, since the
// lease, and with it the pools the round's kernels and copies use, is released without another one.
template <class B, class R>
int run_rounds(size_t live, size_t cap, void* stream, B bytes_of, R run, size_t* done) {
  *done = 0;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  CodecLease lease(st);
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t bound = g_round_bytes.load();
  while (rc == UHDR_HIP_NO_ERROR && *done < live) {
    size_t r1 = *done, bytes = 0;
    while (r1 < live && r1 - *done < cap) {
      const size_t b = bytes_of(r1);
      if (r1 > *done && bytes + b > bound) break;
      bytes += b;
      ++r1;
    }
    rc = run(st, s, *done, (int)(r1 - *done));
    if (rc == UHDR_HIP_NO_ERROR) *done = r1;
  }
  if (rc != UHDR_HIP_NO_ERROR) (void)hipStreamSynchronize(s);
  return rc;
}

// copy `rows` rows of `row_elems` elements of `esz` bytes from a strided host plane into a device
// plane with pitch dpitch_elems.  Only bytes the reference itself would touch are read.
int h2d_plane(void* d, size_t dpitch_elems, const void* h, size_t hstride_elems, size_t row_elems, size_t rows,
              size_t esz, hipStream_t s) {
  if (rows == 0 || row_elems == 0) return UHDR_HIP_NO_ERROR;
  if (hstride_elems == 0) {  // degenerate stride: every row aliases row 0
    for (size_t r = 0; r < rows; ++r)
      HIP_TRY(hipMemcpyAsync(static_cast<char*>(d) + r * dpitch_elems * esz, h, row_elems * esz, hipMemcpyHostToDevice, s));
    return UHDR_HIP_NO_ERROR;
  }
  HIP_TRY(hipMemcpy2DAsync(d, dpitch_elems * esz, h, hstride_elems * esz, row_elems * esz, rows, hipMemcpyHostToDevice, s));
  return UHDR_HIP_NO_ERROR;
}
int d2h_plane(void* h, size_t hstride_elems, const void* d, size_t dpitch_elems, size_t row_elems, size_t rows,
              size_t esz, hipStream_t s) {
  if (rows == 0 || row_elems == 0) return UHDR_HIP_NO_ERROR;
  HIP_TRY(hipMemcpy2DAsync(h, hstride_elems * esz, d, dpitch_elems * esz, row_elems * esz, rows, hipMemcpyDeviceToHost, s));
  return UHDR_HIP_NO_ERROR;
}

int stage_yuv420_in(StageSet* st, int slot, const uhdr_hip_image_t& h, uhdr_hip_image_t* d, hipStream_t s);
// device copy of the host SDR image of applyGainMap, by its pixelFormat: YUV444 / YUV422 / YUV440 with their own chroma extent (Cr
// right behind Cb's rows), anything else as stage_yuv420_in
int stage_ycbcr_in(StageSet* st, int slot, const uhdr_hip_image_t& h, uhdr_hip_image_t* d, hipStream_t s) {
  if (is_420(h)) return stage_yuv420_in(st, slot, h, d, s);
  {
    const ChromaGeom g = chroma_geom(h);
    const size_t w = h.width, cw = (w + g.csx) >> g.csx, ch = g.rows;
    const size_t lp = round_up(w ? w : 1, 64), cp = round_up(cw ? cw : 1, 64);
    int rc;
    if ((rc = stage_reserve(st, slot, lp * (h.height ? h.height : 1))) != 0) return rc;
    if ((rc = stage_reserve(st, slot + 1, cp * (2 * ch + 1))) != 0) return rc;
    *d = h;
    d->data = st->stage[slot]; d->chroma_data = st->stage[slot + 1];
    d->luma_stride = lp; d->chroma_stride = cp;
    if ((rc = h2d_plane(d->data, lp, h.data, h.luma_stride, w, h.height, 1, s)) != 0) return rc;
    const uint8_t* hu = static_cast<const uint8_t*>(h.chroma_data);
    uint8_t* du = static_cast<uint8_t*>(d->chroma_data);
    if ((rc = h2d_plane(du, cp, hu, h.chroma_stride, cw, ch, 1, s)) != 0) return rc;
    return h2d_plane(du + cp * ch, cp, hu + h.chroma_stride * ch, h.chroma_stride, cw, ch, 1, s);
  }
}
// device copy of a host YUV420 image in slots [slot, slot+1]: Y then U|V (pitch = 64-aligned)
int stage_yuv420_in(StageSet* st, int slot, const uhdr_hip_image_t& h, uhdr_hip_image_t* d, hipStream_t s) {
  const size_t w = h.width, hh = h.height, cw = (w + 1) / 2, ch = (hh + 1) / 2;
  const size_t lp = round_up(w ? w : 1, 64), cp = round_up(cw ? cw : 1, 64);
  // the V plane must sit at u + cp*(hh/2) for the kernels (gainmapmath.cpp:568)
  int rc;
  if ((rc = stage_reserve(st, slot, lp * (hh ? hh : 1))) != 0) return rc;
  if ((rc = stage_reserve(st, slot + 1, cp * ((hh / 2) + ch + 1))) != 0) return rc;
  *d = h;
  d->data = st->stage[slot];
  d->chroma_data = st->stage[slot + 1];
  d->luma_stride = lp;
  d->chroma_stride = cp;
  if ((rc = h2d_plane(d->data, lp, h.data, h.luma_stride, w, hh, 1, s)) != 0) return rc;
  const uint8_t* hu = static_cast<const uint8_t*>(h.chroma_data);
  const uint8_t* hv = hu + h.chroma_stride * (hh / 2);
  uint8_t* du = static_cast<uint8_t*>(d->chroma_data);
  if ((rc = h2d_plane(du, cp, hu, h.chroma_stride, cw, ch, 1, s)) != 0) return rc;
  if ((rc = h2d_plane(du + cp * (hh / 2), cp, hv, h.chroma_stride, cw, ch, 1, s)) != 0) return rc;
  return UHDR_HIP_NO_ERROR;
}
int stage_p010_in(StageSet* st, int slot, const uhdr_hip_image_t& h, uhdr_hip_image_t* d, hipStream_t s) {
  const size_t w = h.width, hh = h.height, cw2 = ((w + 1) / 2) * 2, ch = (hh + 1) / 2;
  const size_t lp = round_up(w ? w : 1, 64), cp = round_up(cw2 ? cw2 : 2, 64);
  int rc;
  if ((rc = stage_reserve(st, slot, lp * (hh ? hh : 1) * 2)) != 0) return rc;
  if ((rc = stage_reserve(st, slot + 1, cp * (ch ? ch : 1) * 2)) != 0) return rc;
  *d = h;
  d->data = st->stage[slot];
  d->chroma_data = st->stage[slot + 1];
  d->luma_stride = lp;
  d->chroma_stride = cp;
  if ((rc = h2d_plane(d->data, lp, h.data, row_stride(h), w, hh, 2, s)) != 0) return rc;
  if ((rc = h2d_plane(d->chroma_data, cp, h.chroma_data, h.chroma_stride, cw2, ch, 2, s)) != 0) return rc;
  return UHDR_HIP_NO_ERROR;
}
// A single generate call through host memory: the SDR image staged into slots 0 and 1 of `ss`, the P010 image into 2 and 3, the
// map's width / 4 x height / 4 bytes reserved in slot 4; run(staged SDR, staged P010, staged map) enqueued between, then the map
// copied back.  Enqueues only.
int generate_through_stage(StageSet* ss, const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* p010, uhdr_hip_image_t* dest, hipStream_t s,
                           const std::function<int(const uhdr_hip_image_t&, const uhdr_hip_image_t&, uhdr_hip_image_t&)>& run) {
  int rc;
  uhdr_hip_image_t dy, dp, dm = *dest;
  if ((rc = stage_yuv420_in(ss, 0, *yuv, &dy, s)) != 0) return rc;
  if ((rc = stage_p010_in(ss, 2, *p010, &dp, s)) != 0) return rc;
  const size_t mw = yuv->width / 4, mh = yuv->height / 4;
  if ((rc = stage_reserve(ss, 4, mw * mh)) != 0) return rc;
  dm.data = ss->stage[4];
  if ((rc = run(dy, dp, dm)) != 0) return rc;
  if (mw * mh) HIP_TRY(hipMemcpyAsync(dest->data, dm.data, mw * mh, hipMemcpyDeviceToHost, s));
  return UHDR_HIP_NO_ERROR;
}

}  // namespace

// =====================================================================================================
extern "C" {

int uhdr_hip_abi_version(void) { return UHDR_HIP_ABI_VERSION; }

// host only, a test hook: the byte bound of every later codec round of the process (0: kCodecRoundBytes); returns the one it replaces
size_t uhdr_hip_codec_round_bytes_probe(size_t bytes) { return g_round_bytes.exchange(bytes != 0 ? bytes : kCodecRoundBytes); }

int uhdr_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* uhdr_hip_last_error(void) { return t_err; }

int uhdr_hip_init(int device) {
  if (device < 0 || device >= uhdr_hip_device_count()) {
    snprintf(t_err, sizeof(t_err), "uhdr_hip_init: no HIP device %d (this library has no CPU path)", device);
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  HIP_TRY(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceState& st = g_dev[device];
  if (!st.ready) {
    std::vector<float> t;
    build_idw_tables(4, t);
    HIP_TRY(upload_idw4(t.data()));
    // the reference fills its LUTs at static-initialisation time (gainmapmath.cpp:21-64); here: once per device
    HIP_TRY(hipMalloc(&st.lut, sizeof(float) * kLutBufferFloats));
    HIP_TRY(launch_build_luts(st.lut, nullptr));
    {
      std::vector<float> tab;
      build_line_tables(tab);
      HIP_TRY(hipMemcpy(st.lut + kTabS1Lin, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_build_lut_codes(st.lut, nullptr));
    HIP_TRY(hipMalloc(&st.tone_tab, sizeof(float) * 2 * kTonePackedCodes));
    HIP_TRY(launch_build_packed_tone_tables(st.tone_tab, nullptr));
    HIP_TRY(hipMalloc(&st.srgb_codes, sizeof(float) * kSrgbCodes));
    HIP_TRY(launch_build_srgb_codes(st.srgb_codes, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(jpeg::upload_tables());
    st.ready = true;
  }
  return UHDR_HIP_NO_ERROR;
}

// the workspaces device-memory calls keep per stream (uhdr_hip_stream_reserve / _release hand them out ahead of time / take them back)
int stat_workspace(DeviceState* st, hipStream_t s, uint32_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  uint32_t** wp = nullptr;
  try { wp = &st->stat_ws[s]; } catch (const std::bad_alloc&) { return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; }
  uint32_t*& w = *wp;
  if (w == nullptr) {   // cleared once, in stream order: every launch leaves the headers cleared behind it
    uint32_t* fresh = nullptr;
    HIP_TRY(hipMalloc(&fresh, kStatWsBytes));
    const hipError_t me = hipMemsetAsync(fresh, 0, kStatWsBytes, s);
    if (me != hipSuccess) {   // never publish a workspace whose headers were not cleared
      (void)hipFree(fresh);
      set_err("hipMemsetAsync(statistics workspace)", me);
      return UHDR_HIP_UNKNOWN_ERROR;
    }
    w = fresh;
  }
  *out = w;
  return UHDR_HIP_NO_ERROR;
}
int exact_workspace(DeviceState* st, hipStream_t s, int images, uint32_t cap, uint32_t** out) {
  const size_t need = ((size_t)kMaxChunk * kExHdrWords + (size_t)images * kExLists * cap) * 4u;
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceState::ExWs* wp = nullptr;
  try {
    wp = &st->ex_ws[s];
    if (wp->bytes < need && wp->p) st->retired.reserve(st->retired.size() + 1);
  } catch (const std::bad_alloc&) {
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  DeviceState::ExWs& w = *wp;
  if (w.bytes < need) {
    // another caller of this stream may be about to launch with the old one: it stays allocated (sizes at least double)
    if (w.p) { st->retired.emplace_back(s, static_cast<void*>(w.p)); w.p = nullptr; }
    const size_t grown = std::max(need, 2 * w.bytes);
    w.bytes = 0;
    uint32_t* fresh = nullptr;
    HIP_TRY(hipMalloc(&fresh, grown));
    const hipError_t me = hipMemsetAsync(fresh, 0, (size_t)kMaxChunk * kExHdrWords * 4u, s);   // the headers: cleared once, left cleared by every launch
    if (me != hipSuccess) {                                                                    // (never published uncleared)
      (void)hipFree(fresh);
      set_err("hipMemsetAsync(EXACT workspace)", me);
      return UHDR_HIP_UNKNOWN_ERROR;
    }
    w.p = fresh;
    w.bytes = grown;
  }
  *out = w.p;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_stream_reserve(void* stream, int exact_images, size_t width, size_t height, int map_scale_factor) {
  DeviceState* st = nullptr;
  int rc0 = current_state(&st);
  if (rc0 != UHDR_HIP_NO_ERROR) return rc0;
  if (exact_images < 0 || map_scale_factor < 0 || (exact_images > 0 && (width == 0 || height == 0 || (uint64_t)width * height > 0xFFFFFFFFull)))
    return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t* w = nullptr;
  int rc = stat_workspace(st, s, &w);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (exact_images > 0) {
    const int m = exact_images < kMaxChunk ? exact_images : kMaxChunk;
    if ((rc = exact_workspace(st, s, m, ex_list_cap((uint64_t)width * height), &w)) != UHDR_HIP_NO_ERROR) return rc;
  }
  if (map_scale_factor > 0) {
    const float* idw = nullptr;
    float* transient = nullptr;
    if ((rc = idw_for_scale(st, map_scale_factor, &idw, &transient)) != UHDR_HIP_NO_ERROR) return rc;
    if (transient) { (void)hipStreamSynchronize(s); (void)hipFree(transient); }   // (a table too large to keep: nothing to reserve)
  }
  HIP_TRY(hipStreamSynchronize(s));   // the clears are done: what follows on the stream only enqueues
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_stream_release(void* stream) {
  DeviceState* st = nullptr;
  const int rc0 = current_state(&st);
  if (rc0 != UHDR_HIP_NO_ERROR) return rc0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the pair lock first, THEN the wait: a generate / EXACT-apply pair another thread enqueues on `s` holds g_pair_mu from the moment
  // it takes its workspace until its kernels are enqueued, so whatever names a workspace of `s` is on the stream before the wait
  std::lock_guard<std::mutex> pl(g_pair_mu);
  HIP_TRY(hipStreamSynchronize(s));
  std::lock_guard<std::mutex> lk(g_mu);
  auto a = st->stat_ws.find(s);
  if (a != st->stat_ws.end()) { if (a->second) (void)hipFree(a->second); st->stat_ws.erase(a); }
  auto b = st->ex_ws.find(s);
  if (b != st->ex_ws.end()) { if (b->second.p) (void)hipFree(b->second.p); st->ex_ws.erase(b); }
  auto f = st->fx_ws.find(s);
  if (f != st->fx_ws.end()) {
    if (f->second.dev) (void)hipFree(f->second.dev);
    if (f->second.host) (void)hipHostFree(f->second.host);
    if (f->second.ev) (void)hipEventDestroy(f->second.ev);
    st->fx_ws.erase(f);
  }
  // ... and the lists of this stream that EXACT launches outgrew (kept allocated until nothing on the stream can name them: now)
  size_t keep = 0;
  for (size_t i = 0; i < st->retired.size(); ++i) {
    if (st->retired[i].first == s) (void)hipFree(st->retired[i].second);
    else st->retired[keep++] = st->retired[i];
  }
  st->retired.resize(keep);
  return UHDR_HIP_NO_ERROR;
}

// ---- placement pools (include/uhdr_hip.h: "where resident images lie in device memory") ---------------------------------------
// Chunks are created one after another, so on a device whose memory is mostly free they walk through it; an allocation takes chunks
// spaced evenly over the free ones in that order, i.e. it is spread over the whole pool and interleaves with its neighbours.
struct uhdr_hip_mem_pool {
  int device = 0;
  size_t chunk = 0;
  std::vector<hipMemGenericAllocationHandle_t> handle;
  std::vector<uint8_t> state;   // 0 free, 1 in an allocation, 2 given back to the device (trim)
  struct Range { void* va; size_t chunks; std::vector<size_t> member; };
  std::vector<Range> ranges;
  std::mutex mu;
};
namespace {
struct DeviceGuard {   // the pool's device is current inside a call and the caller's again afterwards
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) { ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess); if (prev == dev) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
void pool_unmap(uhdr_hip_mem_pool* p, uhdr_hip_mem_pool::Range& r) {
  (void)hipMemUnmap(r.va, r.chunks * p->chunk);
  (void)hipMemAddressFree(r.va, r.chunks * p->chunk);
  for (size_t k : r.member) p->state[k] = 0;
}
}  // namespace

int uhdr_hip_mem_pool_create(int device, size_t bytes, size_t chunk_bytes, uhdr_hip_mem_pool_t** pool) {
  if (pool == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  *pool = nullptr;
  if (chunk_bytes == 0) chunk_bytes = (size_t)16 << 20;
  if (bytes == 0 || chunk_bytes % ((size_t)2 << 20) != 0) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (device < 0 || device >= uhdr_hip_device_count()) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  DeviceGuard g(device);
  if (!g.ok) { snprintf(t_err, sizeof(t_err), "uhdr_hip_mem_pool_create: cannot make device %d current", device); return UHDR_HIP_UNKNOWN_ERROR; }
  std::unique_ptr<uhdr_hip_mem_pool> p(new (std::nothrow) uhdr_hip_mem_pool());
  if (!p) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  p->device = device;
  p->chunk = chunk_bytes;
  const size_t n = (bytes + chunk_bytes - 1) / chunk_bytes;
  size_t dev_free = 0, dev_total = 0;
  HIP_TRY(hipMemGetInfo(&dev_free, &dev_total));
  if (n > dev_free / chunk_bytes) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;   // (before a single chunk is taken)
  try { p->handle.reserve(n); p->state.reserve(n); } catch (const std::bad_alloc&) { return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; }
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  for (size_t i = 0; i < n; ++i) {
    hipMemGenericAllocationHandle_t h;
    const hipError_t e = hipMemCreate(&h, chunk_bytes, &prop, 0);
    if (e != hipSuccess) {
      set_err("hipMemCreate(pool chunk)", e);
      for (auto& hh : p->handle) (void)hipMemRelease(hh);
      return e == hipErrorOutOfMemory ? UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE : UHDR_HIP_UNKNOWN_ERROR;
    }
    p->handle.push_back(h);
    p->state.push_back(0);
  }
  *pool = p.release();
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_mem_pool_alloc(uhdr_hip_mem_pool_t* p, size_t bytes, void** ptr) {
  if (p == nullptr || ptr == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  *ptr = nullptr;
  if (bytes == 0) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  std::lock_guard<std::mutex> lk(p->mu);
  DeviceGuard g(p->device);
  if (!g.ok) return UHDR_HIP_UNKNOWN_ERROR;
  const size_t m = (bytes + p->chunk - 1) / p->chunk;
  std::vector<size_t> freec;
  uhdr_hip_mem_pool::Range r;
  try {
    for (size_t i = 0; i < p->state.size(); ++i) if (p->state[i] == 0) freec.push_back(i);
    if (freec.size() < m) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
    // member j = the free chunk at position (j + 1/2) F / m: evenly spaced over the free ones, distinct because F >= m
    for (size_t j = 0; j < m; ++j) r.member.push_back(freec[(size_t)(((2 * (unsigned long long)j + 1) * freec.size()) / (2 * (unsigned long long)m))]);
    p->ranges.reserve(p->ranges.size() + 1);
  } catch (const std::bad_alloc&) { return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; }
  r.chunks = m;
  r.va = nullptr;
  HIP_TRY(hipMemAddressReserve(&r.va, m * p->chunk, 0, nullptr, 0));
  size_t mapped = 0;
  hipError_t e = hipSuccess;
  for (; mapped < m; ++mapped) {
    e = hipMemMap(static_cast<char*>(r.va) + mapped * p->chunk, p->chunk, 0, p->handle[r.member[mapped]], 0);
    if (e != hipSuccess) break;
  }
  if (e == hipSuccess) {
    hipMemAccessDesc a = {};
    a.location.type = hipMemLocationTypeDevice;
    a.location.id = p->device;
    a.flags = hipMemAccessFlagsProtReadWrite;
    e = hipMemSetAccess(r.va, m * p->chunk, &a, 1);
  }
  if (e != hipSuccess) {
    set_err("hipMemMap / hipMemSetAccess(pool allocation)", e);
    if (mapped) (void)hipMemUnmap(r.va, mapped * p->chunk);
    (void)hipMemAddressFree(r.va, m * p->chunk);
    return UHDR_HIP_UNKNOWN_ERROR;
  }
  for (size_t k : r.member) p->state[k] = 1;
  *ptr = r.va;
  p->ranges.push_back(std::move(r));
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_mem_pool_free(uhdr_hip_mem_pool_t* p, void* ptr) {
  if (p == nullptr || ptr == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  std::lock_guard<std::mutex> lk(p->mu);
  DeviceGuard g(p->device);
  if (!g.ok) return UHDR_HIP_UNKNOWN_ERROR;
  for (size_t i = 0; i < p->ranges.size(); ++i)
    if (p->ranges[i].va == ptr) {
      pool_unmap(p, p->ranges[i]);
      p->ranges.erase(p->ranges.begin() + (long)i);
      return UHDR_HIP_NO_ERROR;
    }
  return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
}

int uhdr_hip_mem_pool_trim(uhdr_hip_mem_pool_t* p) {
  if (p == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  std::lock_guard<std::mutex> lk(p->mu);
  DeviceGuard g(p->device);
  if (!g.ok) return UHDR_HIP_UNKNOWN_ERROR;
  for (size_t i = 0; i < p->state.size(); ++i)
    if (p->state[i] == 0) { (void)hipMemRelease(p->handle[i]); p->state[i] = 2; }
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_mem_pool_stats(uhdr_hip_mem_pool_t* p, size_t* chunks, size_t* free_chunks) {
  if (p == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  std::lock_guard<std::mutex> lk(p->mu);
  size_t held = 0, fr = 0;
  for (uint8_t s : p->state) { held += s != 2; fr += s == 0; }
  if (chunks) *chunks = held;
  if (free_chunks) *free_chunks = fr;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_mem_pool_destroy(uhdr_hip_mem_pool_t* p) {
  if (p == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    DeviceGuard g(p->device);
    if (!g.ok) return UHDR_HIP_UNKNOWN_ERROR;
    (void)hipDeviceSynchronize();
    for (auto& r : p->ranges) pool_unmap(p, r);
    p->ranges.clear();
    for (size_t i = 0; i < p->state.size(); ++i)
      if (p->state[i] != 2) (void)hipMemRelease(p->handle[i]);
  }
  delete p;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  for (auto& kv : g_dev) {
    if (hipSetDevice(kv.first) != hipSuccess) continue;
    (void)hipDeviceSynchronize();
    for (auto& t : kv.second.idw) (void)hipFree(t.second);
    if (kv.second.lut) (void)hipFree(kv.second.lut);
    if (kv.second.tone_tab) (void)hipFree(kv.second.tone_tab);
    if (kv.second.srgb_codes) (void)hipFree(kv.second.srgb_codes);
    for (void* q : kv.second.pool) if (q) (void)hipFree(q);
    for (auto& w : kv.second.stat_ws) if (w.second) (void)hipFree(w.second);
    for (auto& w : kv.second.ex_ws) if (w.second.p) (void)hipFree(w.second.p);
    for (auto& w : kv.second.fx_ws) {
      if (w.second.dev) (void)hipFree(w.second.dev);
      if (w.second.host) (void)hipHostFree(w.second.host);
      if (w.second.ev) (void)hipEventDestroy(w.second.ev);
    }
    for (int i = 0; i < kStageSlots; ++i)
      if (kv.second.stage[i]) (void)hipFree(kv.second.stage[i]);
    for (auto& set : kv.second.sets)
      for (int i = 0; i < kStageSlots; ++i)
        if (set->stage[i]) (void)hipFree(set->stage[i]);
    for (auto& q : kv.second.retired) (void)hipFree(q.second);
    for (auto& cx : kv.second.codec_sets) {   // the leased codec contexts (their tables are this state's: not freed here)
      for (void* q : cx->pool) if (q) (void)hipFree(q);
      if (cx->host_pool) (void)hipHostFree(cx->host_pool);
      for (int i = 0; i < kStageSlots; ++i)
        if (cx->stage[i]) (void)hipFree(cx->stage[i]);
    }
  }
  g_dev.clear();
  if (prev >= 0) (void)hipSetDevice(prev);
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_synth_lcg_frame(size_t width, size_t height, unsigned int seed, void* p010, void* yuv, void* stream) {
  if (p010 == nullptr || yuv == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if ((width | height) & 1u) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
  const uint64_t n_luma = (uint64_t)width * height, n = n_luma + n_luma / 2u;
  if (n >= (1ull << 31)) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;   // state indices 2 i + 2 stay below 2^32
  DeviceState* st = nullptr;
  const int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  HIP_TRY(launch_synth_lcg(static_cast<uint16_t*>(p010), static_cast<uint8_t*>(yuv), (uint32_t)n_luma, (uint32_t)n, seed,
                           static_cast<hipStream_t>(stream)));
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_eval_transfer(int fn, const float* in, float* out, size_t n, float min_boost, float max_boost,
                           void* stream) {
  if (in == nullptr || out == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  const int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  EvalConsts ec;
  ec.min_boost = min_boost;
  ec.max_boost = max_boost;
  ec.log2_min = (float)std::log2((double)min_boost);
  ec.log2_max = (float)std::log2((double)max_boost);
  encode_constants(min_boost, max_boost, ec.log2_min, ec.log2_max, &ec.enc_scale, &ec.enc_byte_min, &ec.enc_byte_max);
  ec.lut = st->lut;
  ec.log2_min_d = std::log2((double)min_boost);
  ec.log2_max_d = std::log2((double)max_boost);
  HIP_TRY(launch_eval_transfer(fn, in, out, n, ec, static_cast<hipStream_t>(stream)));
  return UHDR_HIP_NO_ERROR;
}

}  // extern "C"

namespace {
// block geometry and quantisation tables of one image (jpeg_set_quality(q, TRUE), jpegencoderhelper.cpp:119-136)
void encode_job_tables(size_t w, size_t h, jpeg::Geometry geom, int quality, jpeg::Job* jp) {
  jpeg::Job& j = *jp;
  memset(&j, 0, sizeof(j));
  const bool gray = geom == jpeg::kGeomGray, rgb = geom == jpeg::kGeomRgb444;
  j.gray = gray ? 1 : 0;
  j.rgb = rgb ? 1 : 0;
  j.ybw = (uint32_t)((w + 7) / 8); j.ybh = (uint32_t)((h + 7) / 8);
  j.mcus_x = rgb ? j.ybw : (uint32_t)((w + 15) / 16);
  j.nblk = gray ? j.ybw * j.ybh : rgb ? j.ybw * j.ybh * 3u : j.mcus_x * (uint32_t)((h + 15) / 16) * 6u;
  j.hs = (uint32_t)jpeg::geom_hs(geom); j.vs = (uint32_t)jpeg::geom_vs(geom);
  if (geom == jpeg::kGeom444 || geom == jpeg::kGeom422 || geom == jpeg::kGeom440) {   // MCUs of 8 hs x 8 vs pixels, hs * vs + 2 blocks
    j.sampled = 1;
    j.mcus_x = (uint32_t)((w + 8 * j.hs - 1) / (8 * j.hs));
    j.nblk = j.mcus_x * (uint32_t)((h + 8 * j.vs - 1) / (8 * j.vs)) * (j.hs * j.vs + 2u);
  }
  uint16_t qn[64];
  jpeg::quant_table(quality, false, qn); jpeg::zigzag_table(qn, j.q_lum);
  jpeg::quant_table(quality, true, qn); jpeg::zigzag_table(qn, j.q_chr);
  for (int i = 0; i < 64; ++i) {
    j.m_lum[i] = (uint32_t)((1ull << 32) / ((uint32_t)j.q_lum[i] << 3)) + 1u;
    j.m_chr[i] = (uint32_t)((1ull << 32) / ((uint32_t)j.q_chr[i] << 3)) + 1u;
  }
}
jpeg::Plane encode_plane(const uint8_t* p, size_t pw, size_t ph, size_t stride, bool pad, bool replicate = false) {
  jpeg::Plane q;
  q.p = p; q.w = (int)pw; q.h = (int)ph; q.stride = (int)stride; q.pad_cols = replicate ? jpeg::kPadReplicate : pad ? 1 : 0;
  q.aligned4 = (reinterpret_cast<uintptr_t>(p) % 4 == 0 && stride % 4 == 0) ? 1 : 0;
  return q;
}
// the encoder job of one image with device planes (luma_stride set); pad_ls / pad_cs: the strides that decide the column padding,
// the caller's for planes staged from host memory
// The geometry of an image the encoder compresses.  rgb is said by the caller, never read off the descriptor: only the calls that
// take RGBA8888 images pass it, and the older calls go on treating every pixelFormat other than MONOCHROME as 4:2:0.
jpeg::Geometry enc_geom(const uhdr_hip_image_t& img, bool rgb) {
  return rgb ? jpeg::kGeomRgb444 : img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME ? jpeg::kGeomGray : jpeg::kGeom420;
}
// mcu_planes: the planes are jpeg::launch_rgba_to_ycc420's -- whole MCUs, padded by that kernel, Cb at chroma_data -- of an image of
// any size, odd ones included
// geom >= 0: the geometry is the caller's word (the calls that take YUV444 / 422 / 440 planes, or make 4:2:2 planes of RGBA pixels):
// planes of ceil(w / hs) x ceil(h / vs) chroma samples, padded as libjpeg pads (jpeg::kPadReplicate); mcu_planes: whole MCUs of
// jpeg::launch_rgba_to_ycc422's
jpeg::Job encode_job(const uhdr_hip_image_t& img, int q, size_t pad_ls, size_t pad_cs, bool rgb = false, bool mcu_planes = false, int geom = -1) {
  const bool gray = img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  const size_t w = img.width, h = img.height, aw = (w + 15) / 16 * 16, acw = (w / 2 + 7) / 8 * 8;
  jpeg::Job j;
  encode_job_tables(w, h, geom >= 0 ? (jpeg::Geometry)geom : enc_geom(img, rgb), q, &j);
  if (geom >= 0) {
    const uint8_t* pu = static_cast<const uint8_t*>(img.chroma_data);
    if (mcu_planes) {   // (4:2:2)
      const size_t mcw = (w + 15) / 16, mch = (h + 7) / 8;
      j.plane[0] = encode_plane(static_cast<const uint8_t*>(img.data), 16 * mcw, 8 * mch, 16 * mcw, false);
      j.plane[1] = encode_plane(pu, 8 * mcw, 8 * mch, 8 * mcw, false);
      j.plane[2] = encode_plane(pu + 64 * mcw * mch, 8 * mcw, 8 * mch, 8 * mcw, false);
      return j;
    }
    const size_t cw = (w + j.hs - 1) / j.hs, ch = (h + j.vs - 1) / j.vs, cs = img.chroma_stride;
    j.plane[0] = encode_plane(static_cast<const uint8_t*>(img.data), w, h, img.luma_stride, false, true);
    j.plane[1] = encode_plane(pu, cw, ch, cs, false, true);
    j.plane[2] = encode_plane(pu + cs * ch, cw, ch, cs, false, true);
    return j;
  }
  if (mcu_planes) {
    const size_t mcw = (w + 15) / 16, mch = (h + 15) / 16;
    const uint8_t* pu = static_cast<const uint8_t*>(img.chroma_data);
    j.plane[0] = encode_plane(static_cast<const uint8_t*>(img.data), 16 * mcw, 16 * mch, 16 * mcw, false);
    j.plane[1] = encode_plane(pu, 8 * mcw, 8 * mch, 8 * mcw, false);
    j.plane[2] = encode_plane(pu + 64 * mcw * mch, 8 * mcw, 8 * mch, 8 * mcw, false);
    return j;
  }
  if (j.rgb) {   // RGBA pixels, 4-byte aligned, luma_stride in pixels; edges are replicated by the kernel, nothing is padded
    j.plane[0] = jpeg::Plane{static_cast<const uint8_t*>(img.data), (int)w, (int)h, (int)(img.luma_stride * 4), 0, 1};
    return j;
  }
  j.plane[0] = encode_plane(static_cast<const uint8_t*>(img.data), w, h, img.luma_stride, pad_ls < aw);
  if (!gray) {
    const uint8_t* pu = static_cast<const uint8_t*>(img.chroma_data);
    const size_t cs = img.chroma_stride;
    j.plane[1] = encode_plane(pu, w / 2, h / 2, cs, pad_cs < acw);
    j.plane[2] = encode_plane(pu + cs * (h / 2), w / 2, h / 2, cs, pad_cs < acw);   // chromaStride * height / 2 (jpegencoderhelper.cpp:140)
  }
  return j;
}
// the sizes compressImage takes: libjpeg's JPEG_MAX_DIMENSION, and whole 2x2 blocks for 4:2:0
bool encodable(const uhdr_hip_image_t& img) {
  const size_t w = img.width, h = img.height;
  return w != 0 && h != 0 && w <= 65500 && h <= 65500 && (img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME || ((w | h) & 1) == 0);
}

// the columns of a host image the encoder reads -- w when it pads, the 16-aligned width otherwise -- and the pitches they are staged at
struct EncStageCols {
  size_t ycols, ccols, dls, dcs;
};
EncStageCols enc_stage_cols(const uhdr_hip_image_t& h) {
  const size_t w = h.width, ls = h.luma_stride, cs = h.chroma_stride;
  const size_t aw = (w + 15) / 16 * 16, acw = (w / 2 + 7) / 8 * 8;
  const size_t ycols = ls < aw ? w : aw, ccols = cs < acw ? w / 2 : acw;
  return EncStageCols{ycols, ccols, round_up(ycols, 64), round_up(ccols ? ccols : 1, 64)};
}

// device copy of a host image for the encoder in slots [slot, slot+1] (luma_stride set): exactly the bytes the reference would
// touch -- w columns when it pads, the 16-aligned width otherwise
int stage_encoder_in(StageSet* st, int slot, const uhdr_hip_image_t& h, uhdr_hip_image_t* d, hipStream_t s) {
  const size_t hh = h.height, ls = h.luma_stride, cs = h.chroma_stride;
  const EncStageCols g = enc_stage_cols(h);
  const size_t ycols = g.ycols, ccols = g.ccols, dls = g.dls, dcs = g.dcs;
  int rc;
  if ((rc = stage_reserve(st, slot, dls * hh)) != 0) return rc;
  if ((rc = h2d_plane(st->stage[slot], dls, h.data, ls, ycols, hh, 1, s)) != 0) return rc;
  *d = h;
  d->data = st->stage[slot];
  d->luma_stride = dls;
  if (h.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME) return UHDR_HIP_NO_ERROR;
  if ((rc = stage_reserve(st, slot + 1, dcs * hh + 64)) != 0) return rc;
  const uint8_t* hu = static_cast<const uint8_t*>(h.chroma_data);
  uint8_t* du = static_cast<uint8_t*>(st->stage[slot + 1]);
  if ((rc = h2d_plane(du, dcs, hu, cs, ccols, hh / 2, 1, s)) != 0) return rc;
  if ((rc = h2d_plane(du + dcs * (hh / 2), dcs, hu + cs * hh / 2, cs, ccols, hh / 2, 1, s)) != 0) return rc;
  d->chroma_data = du;
  d->chroma_stride = dcs;
  return UHDR_HIP_NO_ERROR;
}

// grow-only buffers of the caller's leased context: device memory (the JPEG/R decode and encode entry points) ...
int pool_reserve(DeviceState* st, size_t idx, size_t bytes) {
  if (st->pool.size() <= idx) { st->pool.resize(idx + 1, nullptr); st->pool_bytes.resize(idx + 1, 0); }
  if (bytes == 0) bytes = 256;
  if (st->pool_bytes[idx] >= bytes) return UHDR_HIP_NO_ERROR;
  if (st->pool[idx]) HIP_TRY(hipFree(st->pool[idx]));
  st->pool[idx] = nullptr; st->pool_bytes[idx] = 0;
  HIP_TRY(hipMalloc(&st->pool[idx], bytes));
  st->pool_bytes[idx] = bytes;
  return UHDR_HIP_NO_ERROR;
}
// ... and page-locked host memory (the JPEG encoder's descriptors, sizes and compressed streams)
int host_pool_reserve(DeviceState* st, size_t bytes) {
  if (st->host_pool_bytes >= bytes) return UHDR_HIP_NO_ERROR;
  if (st->host_pool) HIP_TRY(hipHostFree(st->host_pool));
  st->host_pool = nullptr;
  st->host_pool_bytes = 0;
  HIP_TRY(hipHostMalloc(&st->host_pool, bytes, hipHostMallocDefault));
  st->host_pool_bytes = bytes;
  return UHDR_HIP_NO_ERROR;
}
// the JPEG encoder's pool slots, then encodeJPEGR's planes
enum : size_t { kEncWs = 0, kEncDesc, kEncSdr, kEncMap, kEncP010, kEncYuv };
// the adaptive encode's workspace and the key pair it carries from round to round: slots no other codec path of a context names
enum : size_t { kEncAdaptWs = 8, kEncAdaptCarry = 9 };
// the tone-mapped API-0 encode's headroom array (one float per file of the round): likewise
enum : size_t { kEncToneHead = 10 };

// one image of compress_to_host: device planes and how to compress them in, the JPEG out
struct EncJpeg {
  uhdr_hip_image_t img;                  // luma_stride set; MONOCHROME: one plane
  int quality;
  const std::vector<uint8_t>* icc;       // nullptr: none
  size_t pad_ls, pad_cs;                 // the strides that decide the column padding (encode_job)
  size_t cap = 0;                        // host staging of the file; 0: the single calls' first guess, w * h + 64 KiB
  const uint8_t* bytes = nullptr;        // the JPEG: in the context's host pool, or in `big`
  size_t n = 0;
  std::vector<uint8_t> big;              // a file larger than its staging, compressed again on its own
  size_t keep_max = SIZE_MAX;            // a file larger than this is not wanted (its size is): it is not compressed again
  bool to_dev = false;                   // the JPEG goes to dev_out (device memory, dev_cap bytes; the header only if it fits) instead
  uint8_t* dev_out = nullptr;
  size_t dev_cap = 0;
  bool rgb = false;                      // img is RGBA8888 (luma_stride in pixels), compressed as 4:4:4 (jpeg::kGeomRgb444)
  bool mcu_planes = false;               // img's planes are jpeg::launch_rgba_to_ycc420's (encode_job)
  int geom = -1;                         // >= 0: a jpeg::Geometry the descriptor does not say on its own -- kGeom444 / 422 / 440 planes
                                         // (mcu_planes: jpeg::launch_rgba_to_ycc422's)
  bool optimize = false;                 // UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN: the file's own Huffman tables, built on the device
  uint32_t restart_interval = 0, restart_in_rows = 0;   // uhdr_hip_jpeg_encode_opts_t's, as given: the file's width decides (enc_restart)
  bool progressive = false;              // UHDR_HIP_SCANS_PROGRESSIVE: SOF2 and libjpeg's simple progression, every scan built on the device
  bool clen_overflow = false;            // out: such a file whose tables libjpeg would refuse (jpeg::kProgClenOverflow): no bytes, no size
};

// what the _ex and _opts encode calls say beyond their arguments (encode_flags, encode_opts)
struct EncOpt {
  bool optimize = false;
  uint32_t restart_interval = 0, restart_in_rows = 0;
  bool progressive = false;   // the _scans calls' scan_mode (encode_scans)
  void to(EncJpeg* e) const {
    e->optimize = optimize; e->restart_interval = restart_interval; e->restart_in_rows = restart_in_rows; e->progressive = progressive;
  }
};

// the flags of the _ex encode calls: a bit this library does not know is the call's error, seen before the device is touched
bool encode_flags_known(int flags) { return (flags & ~UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN) == 0; }
// The options struct of the _opts calls, checked before anything else (as the _ex calls check their flags): its size, the flag
// bits and libjpeg's limit on restart_interval.  NULL is no option at all.
int encode_opts(const uhdr_hip_jpeg_encode_opts_t* opts, EncOpt* eo) {
  *eo = EncOpt();
  if (opts == nullptr) return UHDR_HIP_NO_ERROR;
  if (opts->struct_size != sizeof(uhdr_hip_jpeg_encode_opts_t) || !encode_flags_known((int)opts->flags) ||
      opts->restart_interval > 65535u)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  eo->optimize = (opts->flags & UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN) != 0;
  eo->restart_interval = opts->restart_interval;
  eo->restart_in_rows = opts->restart_in_rows;
  return UHDR_HIP_NO_ERROR;
}
// The _scans calls: the options, then the scan mode -- both before any pointer is looked at.  A progressive file has tables of its own
// in every scan whatever the flag says (libjpeg forces optimize_coding), and no restart intervals here
int encode_scans(const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, EncOpt* eo) {
  const int rc = encode_opts(opts, eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (scan_mode != UHDR_HIP_SCANS_BASELINE && scan_mode != UHDR_HIP_SCANS_PROGRESSIVE) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (scan_mode == UHDR_HIP_SCANS_BASELINE) return UHDR_HIP_NO_ERROR;
  if (eo->restart_interval != 0 || eo->restart_in_rows != 0) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  eo->progressive = true;
  eo->optimize = false;
  return UHDR_HIP_NO_ERROR;
}
// the same for the flags word of the _ex calls
int encode_flags(int flags, EncOpt* eo) {
  *eo = EncOpt();
  if (!encode_flags_known(flags)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  eo->optimize = (flags & UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN) != 0;
  return UHDR_HIP_NO_ERROR;
}
// MCUs per restart interval of one file (0: none) and, at *intervals, how many intervals that makes
uint32_t enc_restart(const jpeg::Job& j, uint32_t restart_interval, uint32_t restart_in_rows, uint32_t* intervals) {
  const uint32_t bpm = j.gray ? 1u : j.hs * j.vs + 2u;
  const uint32_t ri = jpeg::restart_mcus(restart_interval, restart_in_rows, j.gray ? j.ybw : j.mcus_x);
  *intervals = ri == 0 ? 0u : (j.nblk / bpm + ri - 1u) / ri;
  return ri;
}
// the encoder workspace of one file with the call's options
size_t enc_workspace_bytes(size_t w, size_t h, jpeg::Geometry geom, const EncOpt& eo) {
  jpeg::Job j;
  encode_job_tables(w, h, geom, 75, &j);
  uint32_t intervals = 0;
  enc_restart(j, eo.restart_interval, eo.restart_in_rows, &intervals);
  jpeg::Layout l;
  return jpeg::workspace_bytes(j.nblk, &l, intervals, eo.progressive);
}
// The first guess at a file's size, restart markers apart: what compress_to_host stages a file at when nobody says (cap == 0), and
// what a file of a plain-JPEG batch holds of its round's page-locked memory.  One byte per pixel for 4:2:0 and monochrome files, three
// for every geometry with more chroma (4:2:2 and 4:4:0 among them, for which two would do: the rule decides which files share a round).
size_t enc_first_guess(size_t w, size_t h, jpeg::Geometry geom) {
  return w * h * (geom == jpeg::kGeom420 || geom == jpeg::kGeomGray ? 1 : 3) + 65536;
}
// a file with restart intervals addresses its packed stream in 32 bits (jpeg::kMaxRestartBlocks); the table search has its own limit
bool encodable_with(size_t w, size_t h, jpeg::Geometry geom, const EncOpt& eo);
// libjpeg's table search reads a count of 10^9 as "none": an image whose AC histogram could reach it gets no optimised tables
bool optimizable(size_t w, size_t h, jpeg::Geometry geom) {
  jpeg::Job j;
  encode_job_tables(w, h, geom, 75, &j);
  return j.nblk <= jpeg::kMaxOptimizeBlocks;
}
bool encodable_with(size_t w, size_t h, jpeg::Geometry geom, const EncOpt& eo) {
  if ((eo.optimize || eo.progressive) && !optimizable(w, h, geom)) return false;
  if (eo.progressive) {   // (and the limit of its own: the segments' markers are kept as 32-bit offsets into the packed stream)
    jpeg::Job j;
    encode_job_tables(w, h, geom, 75, &j);
    return j.nblk <= jpeg::kMaxProgressiveBlocks;
  }
  if (eo.restart_interval == 0 && eo.restart_in_rows == 0) return true;
  jpeg::Job j;
  encode_job_tables(w, h, geom, 75, &j);
  return j.nblk <= jpeg::kMaxRestartBlocks;
}

// JpegEncoderHelper::compressImage (jpegencoderhelper.cpp:39-52) of k images in the leased context st: the headers are written into
// its page-locked host pool, one jpeg::encode_batch_async writes the streams behind them and their sizes, and one synchronisation
// ends it.  A file larger than its staging was cut off: it is compressed again in a context of its own, so that this one's host
// pool, which holds the other files, is left alone.  A non-zero return is an error of the device or the runtime.
// extra.dev (or null): extra.bytes of device memory that come down with the streams -- copied into the host pool behind the same
// synchronisation, then to extra.host (the adaptive encode's boost ranges).
struct EncExtra {
  const void* dev = nullptr;
  size_t bytes = 0;
  void* host = nullptr;
};
int compress_to_host(DeviceState* st, hipStream_t s, int k, EncJpeg* im, bool may_retry = true, const EncExtra& extra = EncExtra()) {
  std::vector<jpeg::Job> jobs((size_t)k);
  std::vector<jpeg::Layout> lay((size_t)k);
  std::vector<jpeg::BatchOut> outs((size_t)k);
  std::vector<uint8_t*> wss((size_t)k);
  std::vector<size_t> ws_off((size_t)k), off((size_t)k);
  const size_t desc = round_up(jpeg::batch_desc_bytes(k), 256);
  size_t hp_total = desc + round_up(8 * (size_t)k, 256), ws_total = 0;
  std::vector<std::vector<uint8_t>> header((size_t)k);
  for (int i = 0; i < k; ++i) {
    const EncJpeg& e = im[i];
    jobs[i] = encode_job(e.img, e.quality, e.pad_ls, e.pad_cs, e.rgb, e.mcu_planes, e.geom);
    ws_off[i] = ws_total;
    uint32_t intervals = 0;
    const uint32_t ri = enc_restart(jobs[i], e.restart_interval, e.restart_in_rows, &intervals);
    if (ri != 0) {   // the file runs through the encoder's restart launches, and its header says DRI
      jobs[i].rst_bpm = jobs[i].gray ? 1u : jobs[i].hs * jobs[i].vs + 2u;
      jobs[i].rst_blocks = ri * jobs[i].rst_bpm;
      jobs[i].rst_marks = intervals - 1u;
    }
    ws_total += round_up(jpeg::workspace_bytes(jobs[i].nblk, &lay[i], intervals, e.progressive), 256);
    jobs[i].optimize = e.optimize ? 1 : 0;
    jobs[i].progressive = e.progressive ? 1 : 0;   // (the prefix ends in SOF2; every scan's DHT and SOS segments are the device's)
    // The header split: with optimised tables the host writes SOI ... SOF alone, and the device appends its DHT and SOS segments.
    // Such a header is never longer than the default one -- baseline 8-bit data has at most 12 DC and 162 AC symbols, the sizes of
    // the Annex K tables --, so whatever is sized for the default header (a file's first-guess staging, a caller's capacity that
    // holds the default file) holds this one.
    const jpeg::Geometry geom = e.geom >= 0 ? (jpeg::Geometry)e.geom : enc_geom(e.img, e.rgb);
    jpeg::build_header((int)e.img.width, (int)e.img.height, geom, e.quality, e.icc ? e.icc->data() : nullptr,
                       e.icc ? e.icc->size() : 0, header[i], e.optimize || e.progressive, ri, e.progressive);
    // (the first guess holds the DRI segment and three bytes per interval as well)
    if (im[i].cap == 0) im[i].cap = enc_first_guess(e.img.width, e.img.height, geom) + (ri != 0 ? 6 + 3 * (size_t)intervals : 0);
    off[i] = hp_total;
    hp_total += round_up(e.to_dev ? header[i].size() : im[i].cap, 256);   // a device destination: the header's way there only
  }
  const size_t extra_off = hp_total;
  if (extra.dev != nullptr) hp_total += round_up(extra.bytes, 256);
  int rc;
  if ((rc = host_pool_reserve(st, hp_total)) != 0) return rc;
  if ((rc = pool_reserve(st, kEncWs, ws_total)) != 0) return rc;
  if ((rc = pool_reserve(st, kEncDesc, jpeg::batch_desc_bytes(k))) != 0) return rc;
  uint8_t* hp = static_cast<uint8_t*>(st->host_pool);
  uint64_t* sizes = reinterpret_cast<uint64_t*>(hp + desc);
  for (int i = 0; i < k; ++i) {
    const EncJpeg& e = im[i];
    const size_t hn = header[i].size();
    memcpy(hp + off[i], header[i].data(), hn);
    sizes[i] = 0;
    if (e.to_dev && (e.optimize || e.progressive)) {   // whether the header fits is the device's to say: it copies the prefix from here if it does
      outs[i] = jpeg::BatchOut{e.dev_out, e.dev_cap, hn, &sizes[i], hp + off[i]};
    } else if (e.to_dev) {   // as uhdr_hip_jpeg_encode into device memory: the header only where it fits, no stream byte otherwise
      const bool fits = e.dev_cap >= hn;
      if (fits) HIP_TRY(hipMemcpyAsync(e.dev_out, hp + off[i], hn, hipMemcpyHostToDevice, s));
      outs[i] = jpeg::BatchOut{e.dev_out, fits ? e.dev_cap : 0, hn, &sizes[i]};
    } else {
      outs[i] = jpeg::BatchOut{hp + off[i], e.cap, hn, &sizes[i]};
    }
    wss[i] = static_cast<uint8_t*>(st->pool[kEncWs]) + ws_off[i];
  }
  HIP_TRY(jpeg::encode_batch_async(k, jobs.data(), lay.data(), wss.data(), outs.data(), hp, static_cast<uint8_t*>(st->pool[kEncDesc]), s));
  if (extra.dev != nullptr) HIP_TRY(hipMemcpyAsync(hp + extra_off, extra.dev, extra.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (extra.dev != nullptr) memcpy(extra.host, hp + extra_off, extra.bytes);
  for (int i = 0; i < k; ++i) {
    EncJpeg& e = im[i];
    const uint64_t total = sizes[i];
    if (total == jpeg::kProgClenOverflow) { e.bytes = nullptr; e.n = 0; e.clen_overflow = true; continue; }
    if (total != 0 && e.to_dev) { e.bytes = nullptr; e.n = (size_t)total; continue; }   // the kernels kept to dev_cap
    if (total != 0 && total <= e.cap) { e.bytes = hp + off[i]; e.n = (size_t)total; continue; }
    if (total != 0 && total > e.keep_max) { e.bytes = nullptr; e.n = (size_t)total; continue; }
    if (total == 0 || !may_retry) return UHDR_HIP_ERROR_ENCODE_ERROR;
    DeviceState* root = nullptr;
    if (current_state(&root) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_ENCODE_ERROR;
    CodecLease lease(root);
    EncJpeg one{e.img, e.quality, e.icc, e.pad_ls, e.pad_cs, (size_t)total};
    one.rgb = e.rgb;
    one.mcu_planes = e.mcu_planes;
    one.geom = e.geom;
    one.optimize = e.optimize;
    one.restart_interval = e.restart_interval;
    one.restart_in_rows = e.restart_in_rows;
    one.progressive = e.progressive;
    if (lease.get() == nullptr || compress_to_host(lease.get(), s, 1, &one, false) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_ENCODE_ERROR;
    e.big.assign(one.bytes, one.bytes + one.n);
    e.bytes = e.big.data();
    e.n = e.big.size();
  }
  return UHDR_HIP_NO_ERROR;
}

// ---- plain JPEG for n files (uhdr_hip_jpeg_encode_batch, uhdr_hip_jpeg_decode_batch) -----------------------------------------------
// uhdr_hip_jpeg_encode's image as it compresses it: luma_stride defaulted, no chroma stride for a single plane
uhdr_hip_image_t enc_image(const uhdr_hip_image_t& in) {
  uhdr_hip_image_t img = in;
  if (img.luma_stride == 0) img.luma_stride = img.width;
  if (img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME) img.chroma_stride = 0;
  return img;
}
// bytes of the staged planes of a host image (luma, then chroma, each 256-aligned)
size_t enc_stage_bytes(const uhdr_hip_image_t& img) {
  const EncStageCols g = enc_stage_cols(img);
  const size_t luma = round_up(g.dls * img.height, 256);
  return img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME ? luma : luma + round_up(g.dcs * img.height + 64, 256);
}
// stage_encoder_in's bytes and pitches for a host image (luma_stride set), into the enc_stage_bytes(img) bytes at dy; *d: the staged image
int stage_encoder_slice(uint8_t* dy, const uhdr_hip_image_t& img, uhdr_hip_image_t* d, hipStream_t s) {
  const EncStageCols g = enc_stage_cols(img);
  const size_t hh = img.height;
  int rc;
  if ((rc = h2d_plane(dy, g.dls, img.data, img.luma_stride, g.ycols, hh, 1, s)) != 0) return rc;
  *d = img;
  d->data = dy;
  d->luma_stride = g.dls;
  if (img.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME) return UHDR_HIP_NO_ERROR;
  const uint8_t* hu = static_cast<const uint8_t*>(img.chroma_data);
  const size_t cs = img.chroma_stride;
  uint8_t* du = dy + round_up(g.dls * hh, 256);
  if ((rc = h2d_plane(du, g.dcs, hu, cs, g.ccols, hh / 2, 1, s)) != 0) return rc;
  if ((rc = h2d_plane(du + g.dcs * (hh / 2), g.dcs, hu + cs * hh / 2, cs, g.ccols, hh / 2, 1, s)) != 0) return rc;
  d->chroma_data = du;
  d->chroma_stride = g.dcs;
  return UHDR_HIP_NO_ERROR;
}
// what one image holds of its round: encoder workspace, staged planes, page-locked staging of the file
size_t enc_round_bytes(const uhdr_hip_image_t& img, bool host_in, bool host_out, const EncOpt& eo = EncOpt()) {
  size_t b = enc_workspace_bytes(img.width, img.height, enc_geom(img, false), eo);
  if (host_in) b += enc_stage_bytes(img);
  if (host_out) b += enc_first_guess(img.width, img.height, enc_geom(img, false));
  return b;
}

// ---- planes of any sampling (uhdr_hip_jpeg_encode_planes_batch_opts) ----------------------------------------------------------------
// the geometry of a YUV444 / 422 / 440 image, -1 for every other format (which that call compresses as uhdr_hip_jpeg_encode_batch does)
int sampled_geom(const uhdr_hip_image_t& img) {
  return img.pixelFormat == UHDR_HIP_PIX_FMT_YUV444   ? (int)jpeg::kGeom444
         : img.pixelFormat == UHDR_HIP_PIX_FMT_YUV422 ? (int)jpeg::kGeom422
         : img.pixelFormat == UHDR_HIP_PIX_FMT_YUV440 ? (int)jpeg::kGeom440
                                                      : -1;
}
// such an image as the encoder reads it: chroma of ceil(w / hs) x ceil(h / vs) samples, strides defaulted to the widths
struct SampledDims {
  size_t cw, ch;
};
SampledDims sampled_dims(const uhdr_hip_image_t& img, int geom) {
  const size_t hs = (size_t)jpeg::geom_hs((jpeg::Geometry)geom), vs = (size_t)jpeg::geom_vs((jpeg::Geometry)geom);
  return SampledDims{(img.width + hs - 1) / hs, (img.height + vs - 1) / vs};
}
uhdr_hip_image_t sampled_image(const uhdr_hip_image_t& in, int geom) {
  uhdr_hip_image_t img = in;
  if (img.luma_stride == 0) img.luma_stride = img.width;
  if (img.chroma_stride == 0) img.chroma_stride = sampled_dims(in, geom).cw;
  return img;
}
// the call's checks of such an image behind the pointers: 1x1 to 65500x65500, odd sizes included; rows at least as long as the plane
int sampled_check(const uhdr_hip_image_t& im, int geom, const EncOpt& eo) {
  if (im.width == 0 || im.height == 0 || im.width > 65500 || im.height > 65500) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  const uhdr_hip_image_t d = sampled_image(im, geom);
  if (d.luma_stride < d.width || d.chroma_stride < sampled_dims(im, geom).cw || d.luma_stride > (size_t)INT32_MAX ||
      d.chroma_stride > (size_t)INT32_MAX)
    return UHDR_HIP_ERROR_INVALID_STRIDE;
  if (!encodable_with(im.width, im.height, (jpeg::Geometry)geom, eo)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return UHDR_HIP_NO_ERROR;
}
// bytes of the staged planes of such a host image: the samples alone at 64-byte pitches, luma, then Cb and Cr in one piece
size_t sampled_stage_bytes(const uhdr_hip_image_t& img, int geom) {
  const SampledDims g = sampled_dims(img, geom);
  return round_up(round_up(img.width, 64) * img.height, 256) + round_up(round_up(g.cw, 64) * 2 * g.ch, 256);
}
int stage_sampled_slice(uint8_t* dy, const uhdr_hip_image_t& img, int geom, uhdr_hip_image_t* d, hipStream_t s) {
  const SampledDims g = sampled_dims(img, geom);
  const size_t dls = round_up(img.width, 64), dcs = round_up(g.cw, 64);
  int rc;
  if ((rc = h2d_plane(dy, dls, img.data, img.luma_stride, img.width, img.height, 1, s)) != 0) return rc;
  uint8_t* du = dy + round_up(dls * img.height, 256);
  if ((rc = h2d_plane(du, dcs, img.chroma_data, img.chroma_stride, g.cw, 2 * g.ch, 1, s)) != 0) return rc;   // (Cr follows Cb)
  *d = img;
  d->data = dy; d->luma_stride = dls;
  d->chroma_data = du; d->chroma_stride = dcs;
  return UHDR_HIP_NO_ERROR;
}

}  // namespace

extern "C" {

// JpegEncoderHelper::compressImage (jpegencoderhelper.cpp:39-52) on the device.  The one single call that is not a batch of one: a
// 4K q95 file into host memory takes 0.49 ms through compress_to_host's page-locked staging and 0.43 ms staged in device memory at its
// worst-case size and copied down once, as here (profiles/r06_single_calls.txt)
int uhdr_hip_jpeg_encode(const uhdr_hip_image_t* image, int quality, const void* icc, size_t icc_size, void* out,
                         size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  if (image == nullptr || out_size == nullptr || image->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const bool gray = image->pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  if (!gray && image->chroma_data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (out == nullptr && out_capacity != 0) return UHDR_HIP_ERROR_BAD_PTR;
  if (!encodable(*image)) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CodecLease lease(st);   // the encoder workspace: this call's own
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;

  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  uhdr_hip_image_t img = *image;
  if (img.luma_stride == 0) img.luma_stride = img.width;
  if (gray) img.chroma_stride = 0;
  uhdr_hip_image_t d = img;
  if (host && (rc = stage_encoder_in(st, 0, img, &d, s)) != 0) return rc;
  const jpeg::Job j = encode_job(d, quality, img.luma_stride, img.chroma_stride);
  std::vector<uint8_t> header;
  jpeg::build_header((int)img.width, (int)img.height, enc_geom(img, false), quality, icc, icc_size, header);
  jpeg::Layout l;
  if ((rc = stage_reserve(st, 7, jpeg::workspace_bytes(j.nblk, &l))) != 0) return rc;
  uint8_t* ws = static_cast<uint8_t*>(st->stage[7]);
  uint8_t* dout = static_cast<uint8_t*>(out);
  size_t dcap = out_capacity;
  if (host) {   // worst case: every stream byte stuffed
    dcap = header.size() + 2 * l.stream_bytes + 2;
    if ((rc = stage_reserve(st, 5, dcap)) != 0) return rc;
    dout = static_cast<uint8_t*>(st->stage[5]);
  }
  if (dcap >= header.size()) HIP_TRY(hipMemcpyAsync(dout, header.data(), header.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(jpeg::encode_async(j, l, ws, dout, dcap >= header.size() ? dcap : 0, header.size(), s));
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, ws + l.totals + 8, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out_size = (size_t)total;
  if (total > out_capacity) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if (host) {
    HIP_TRY(hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return UHDR_HIP_NO_ERROR;
}

}  // extern "C"

namespace {
// uhdr_hip_jpeg_encode_rgb_batch's per-file checks of an RGBA8888 image and its output
int rgba_file_check(const uhdr_hip_image_t& im, bool host_in, const void* out, size_t out_capacity) {
  if (im.data == nullptr || (!host_in && !al(im.data, 4)) || (out == nullptr && out_capacity != 0)) return UHDR_HIP_ERROR_BAD_PTR;
  if (im.pixelFormat != UHDR_HIP_PIX_FMT_RGBA8888) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (im.width == 0 || im.height == 0 || im.width > 65500 || im.height > 65500 || (im.luma_stride != 0 && im.luma_stride < im.width) ||
      im.luma_stride > (size_t)INT32_MAX / 4)   // (rows are addressed with an int byte pitch)
    return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  return UHDR_HIP_NO_ERROR;
}
// The 4:2:0 encoder's planes of m RGBA8888 images in device memory (luma_stride set), slices of pool slot `slot`: one
// jpeg::launch_rgba_to_ycc420 for all of them (m <= jpeg::kRgba420Chunk).  e[k * step].img / .mcu_planes describe image k's planes.
// s422: jpeg::launch_rgba_to_ycc422's planes instead (MCUs of 16 x 8 pixels), and the jobs' geometry with them
int rgba420_planes(DeviceState* st, size_t slot, hipStream_t s, int m, const uhdr_hip_image_t* imgs, EncJpeg* e, int step, bool s422 = false) {
  auto plane_bytes = [s422](const uhdr_hip_image_t& im) {
    return round_up(s422 ? jpeg::rgba422_plane_bytes(im.width, im.height) : jpeg::rgba420_plane_bytes(im.width, im.height), 256);
  };
  size_t total = 0;
  for (int k = 0; k < m; ++k) total += plane_bytes(imgs[k]);
  int rc;
  if ((rc = pool_reserve(st, slot, total)) != 0) return rc;
  jpeg::Rgba420Batch b;
  size_t o = 0;
  for (int k = 0; k < m; ++k) {
    const uhdr_hip_image_t& im = imgs[k];
    jpeg::Rgba420Image& d = b.img[k];
    d.src = static_cast<const uint32_t*>(im.data);
    d.w = (uint32_t)im.width; d.h = (uint32_t)im.height; d.stride = (uint32_t)im.luma_stride;
    d.mcw = (uint32_t)((im.width + 15) / 16); d.mch = (uint32_t)(s422 ? (im.height + 7) / 8 : (im.height + 15) / 16);
    d.y = static_cast<uint8_t*>(st->pool[slot]) + o;
    d.cb = d.y + (s422 ? 128 : 256) * (size_t)d.mcw * d.mch;
    o += plane_bytes(im);
    uhdr_hip_image_t& p = e[(size_t)k * step].img;
    memset(&p, 0, sizeof(p));
    p.data = d.y; p.chroma_data = d.cb; p.width = im.width; p.height = im.height; p.colorGamut = im.colorGamut;
    p.luma_stride = 16 * (size_t)d.mcw; p.chroma_stride = 8 * (size_t)d.mcw; p.pixelFormat = UHDR_HIP_PIX_FMT_YUV420;
    e[(size_t)k * step].mcu_planes = true;
    if (s422) { e[(size_t)k * step].geom = jpeg::kGeom422; p.pixelFormat = UHDR_HIP_PIX_FMT_YUV422; }
    e[(size_t)k * step].pad_ls = p.luma_stride; e[(size_t)k * step].pad_cs = p.chroma_stride;
  }
  HIP_TRY(s422 ? jpeg::launch_rgba_to_ycc422(b, m, s) : jpeg::launch_rgba_to_ycc420(b, m, s));
  return UHDR_HIP_NO_ERROR;
}

// Rows of width * bpp bytes of a host image of packed pixels (luma_stride set, in pixels) into the slice at dst, at a 64-byte pitch:
// *d (which may be the image itself) is the staged image, and the slice takes *bytes = rgba_stage_bytes of its pool slot.
size_t rgba_stage_bytes(size_t width, size_t height, size_t bpp) { return round_up(round_up(width * bpp, 64) * height, 256); }
int stage_rgba_rows(uint8_t* dst, const uhdr_hip_image_t h, size_t bpp, uhdr_hip_image_t* d, size_t* bytes, hipStream_t s) {
  const size_t pitch = round_up(h.width * bpp, 64);
  const int rc = h2d_plane(dst, pitch, h.data, h.luma_stride * bpp, h.width * bpp, h.height, 1, s);
  if (rc != 0) return rc;
  *d = h;
  d->data = dst; d->luma_stride = pitch / bpp;
  *bytes = rgba_stage_bytes(h.width, h.height, bpp);
  return UHDR_HIP_NO_ERROR;
}

// ---- the plain-JPEG encode batches: three families of files behind one driver (jpeg_encode_files) -------------------------------
// A family says what the driver cannot know: kRoundCap (files per round), kQualityGate (a quality outside 0 .. 100 is the call's
// error), check (one file's checks, in the family's order), geometry, extra_bytes (the device bytes a file holds of its round beyond
// encoder workspace and first-guess file staging) and prepare: the round's files idx[0, m) into device memory -- host inputs staged
// at the slot kEncYuv, converted planes at kEncSdr --, e[k] left with img, pad_ls / pad_cs, geom, rgb and mcu_planes.

// planes as they are: 4:2:0 and monochrome images, and YUV444 / 422 / 440 ones where the call takes them (any_sampling:
// uhdr_hip_jpeg_encode_planes_batch_opts; every other call compresses such an image as 4:2:0)
struct PlanesFamily {
  static constexpr size_t kRoundCap = (size_t)jpeg::kMaxBatchJobs;
  static constexpr bool kQualityGate = false;
  bool any_sampling;
  int sampled(const uhdr_hip_image_t& im) const { return any_sampling ? sampled_geom(im) : -1; }
  // the single call's checks, in its order
  int check(const uhdr_hip_image_t& im, bool, const void* out, size_t out_capacity, const EncOpt& eo) const {
    if (im.data == nullptr || (im.pixelFormat != UHDR_HIP_PIX_FMT_MONOCHROME && im.chroma_data == nullptr) ||
        (out == nullptr && out_capacity != 0))
      return UHDR_HIP_ERROR_BAD_PTR;
    if (sampled(im) >= 0) return sampled_check(im, sampled(im), eo);
    if (!encodable(im)) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
    if (!encodable_with(im.width, im.height, enc_geom(im, false), eo)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    return UHDR_HIP_NO_ERROR;
  }
  jpeg::Geometry geometry(const uhdr_hip_image_t& im) const { return sampled(im) >= 0 ? (jpeg::Geometry)sampled(im) : enc_geom(im, false); }
  size_t extra_bytes(const uhdr_hip_image_t& im, bool host_in) const {
    if (!host_in) return 0;
    return sampled(im) >= 0 ? sampled_stage_bytes(im, sampled(im)) : enc_stage_bytes(enc_image(im));
  }
  int prepare(DeviceState* st, hipStream_t s, const uhdr_hip_image_t* images, bool host_in, const int* idx, int m, EncJpeg* e) const {
    int rc;
    size_t stage_total = 0, o = 0;
    for (int k = 0; k < m; ++k) stage_total += extra_bytes(images[idx[k]], host_in);
    if (host_in && (rc = pool_reserve(st, kEncYuv, stage_total)) != 0) return rc;
    for (int k = 0; k < m; ++k) {
      const int geom = sampled(images[idx[k]]);
      const uhdr_hip_image_t img = geom >= 0 ? sampled_image(images[idx[k]], geom) : enc_image(images[idx[k]]);
      uhdr_hip_image_t d = img;
      if (host_in) {   // into the round's slice
        uint8_t* dst = static_cast<uint8_t*>(st->pool[kEncYuv]) + o;
        if ((rc = geom >= 0 ? stage_sampled_slice(dst, img, geom, &d, s) : stage_encoder_slice(dst, img, &d, s)) != 0) return rc;
        o += geom >= 0 ? sampled_stage_bytes(img, geom) : enc_stage_bytes(img);
      }
      e[k].img = d;
      e[k].pad_ls = img.luma_stride;
      e[k].pad_cs = img.chroma_stride;
      e[k].geom = geom;
    }
    return UHDR_HIP_NO_ERROR;
  }
};

// what the two RGBA8888 families share: rgba_file_check, then the options against the geometry; and the images of a round in device
// memory, luma_stride set
int rgba_family_check(const uhdr_hip_image_t& im, bool host_in, const void* out, size_t out_capacity, jpeg::Geometry geom, const EncOpt& eo) {
  const int rc = rgba_file_check(im, host_in, out, out_capacity);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return encodable_with(im.width, im.height, geom, eo) ? UHDR_HIP_NO_ERROR : UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
}
int rgba_round_images(DeviceState* st, hipStream_t s, const uhdr_hip_image_t* images, bool host_in, const int* idx, int m, uhdr_hip_image_t* dev) {
  int rc;
  size_t stage_total = 0, o = 0;
  for (int k = 0; host_in && k < m; ++k) stage_total += rgba_stage_bytes(images[idx[k]].width, images[idx[k]].height, 4);
  if (host_in && (rc = pool_reserve(st, kEncYuv, stage_total)) != 0) return rc;
  for (int k = 0; k < m; ++k) {
    dev[k] = images[idx[k]];
    if (dev[k].luma_stride == 0) dev[k].luma_stride = dev[k].width;
    if (!host_in) continue;
    size_t bytes = 0;
    if ((rc = stage_rgba_rows(static_cast<uint8_t*>(st->pool[kEncYuv]) + o, dev[k], 4, &dev[k], &bytes, s)) != 0) return rc;
    o += bytes;
  }
  return UHDR_HIP_NO_ERROR;
}
// RGBA8888 pixels as 4:4:4 (jpeg::kGeomRgb444): the file libjpeg writes for in_color_space = JCS_RGB with all sampling factors 1; the
// encoder converts as it loads, so there is no launch in front
struct Rgba444Family {
  static constexpr size_t kRoundCap = (size_t)jpeg::kMaxBatchJobs;
  static constexpr bool kQualityGate = true;
  int check(const uhdr_hip_image_t& im, bool host_in, const void* out, size_t out_capacity, const EncOpt& eo) const {
    return rgba_family_check(im, host_in, out, out_capacity, jpeg::kGeomRgb444, eo);
  }
  jpeg::Geometry geometry(const uhdr_hip_image_t&) const { return jpeg::kGeomRgb444; }
  size_t extra_bytes(const uhdr_hip_image_t& im, bool host_in) const { return host_in ? rgba_stage_bytes(im.width, im.height, 4) : 0; }
  int prepare(DeviceState* st, hipStream_t s, const uhdr_hip_image_t* images, bool host_in, const int* idx, int m, EncJpeg* e) const {
    std::vector<uhdr_hip_image_t> dev((size_t)m);
    const int rc = rgba_round_images(st, s, images, host_in, idx, m, dev.data());
    if (rc != 0) return rc;
    for (int k = 0; k < m; ++k) {
      e[k].img = dev[(size_t)k];
      e[k].img.chroma_data = nullptr; e[k].img.chroma_stride = 0;
      e[k].pad_ls = e[k].pad_cs = 0;
      e[k].rgb = true;
    }
    return UHDR_HIP_NO_ERROR;
  }
};
// RGBA8888 pixels as 4:2:0, or as 4:2:2 (s422): the planes libjpeg's colour conversion and downsampler hand its FDCT come from one
// k_rgba_to_ycc420 / k_rgba_to_ycc422 launch per round (rgba420_planes), which is what holds a round to jpeg::kRgba420Chunk files
struct RgbaSubsampledFamily {
  static constexpr size_t kRoundCap = (size_t)jpeg::kRgba420Chunk;
  static constexpr bool kQualityGate = true;
  bool s422;
  int check(const uhdr_hip_image_t& im, bool host_in, const void* out, size_t out_capacity, const EncOpt& eo) const {
    return rgba_family_check(im, host_in, out, out_capacity, geometry(im), eo);
  }
  jpeg::Geometry geometry(const uhdr_hip_image_t&) const { return s422 ? jpeg::kGeom422 : jpeg::kGeom420; }
  size_t extra_bytes(const uhdr_hip_image_t& im, bool host_in) const {
    return round_up(s422 ? jpeg::rgba422_plane_bytes(im.width, im.height) : jpeg::rgba420_plane_bytes(im.width, im.height), 256) +
           (host_in ? rgba_stage_bytes(im.width, im.height, 4) : 0);
  }
  int prepare(DeviceState* st, hipStream_t s, const uhdr_hip_image_t* images, bool host_in, const int* idx, int m, EncJpeg* e) const {
    std::vector<uhdr_hip_image_t> dev((size_t)m);
    const int rc = rgba_round_images(st, s, images, host_in, idx, m, dev.data());
    return rc != 0 ? rc : rgba420_planes(st, kEncSdr, s, m, dev.data(), e, 1, s422);
  }
};

// the arrays of a plain-JPEG encode batch, as the caller gave them (icc and status may be NULL)
struct JpegBatch {
  int n;
  const uhdr_hip_image_t* images;
  const int* quality;
  const void* const* icc;
  const size_t* icc_size;
  void* const* out;
  const size_t* out_capacity;
  size_t* out_size;
  int* status;
};

// uhdr_hip_jpeg_encode for n images of one family in one call.  The call's own checks first -- pointers, then the quality gate where
// the family has one --, after which nothing fails the call: a file that fails its checks is not processed and has its status, the
// others go through in rounds (run_rounds) whose files share one jpeg::encode_batch_async launch set and one synchronisation
// (compress_to_host).  mem_space: UHDR_HIP_MEM_DEVICE_TO_HOST and UHDR_HIP_MEM_HOST_TO_DEVICE say the inputs' and the files' side apart.
template <class Family>
int jpeg_encode_files(const JpegBatch& a, const EncOpt& eo, int mem_space, void* stream, const Family& fam) {
  if (a.n < 0 || (a.n > 0 && (a.images == nullptr || a.quality == nullptr || a.out == nullptr || a.out_capacity == nullptr || a.out_size == nullptr)) ||
      (a.icc != nullptr && a.icc_size == nullptr))
    return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; Family::kQualityGate && i < a.n; ++i)
    if (a.quality[i] < 0 || a.quality[i] > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;
  const bool host_in = mem_space == UHDR_HIP_MEM_HOST || mem_space == UHDR_HIP_MEM_HOST_TO_DEVICE;
  const bool host_out = mem_space != UHDR_HIP_MEM_DEVICE && mem_space != UHDR_HIP_MEM_HOST_TO_DEVICE;
  std::vector<int> st_((size_t)a.n, UHDR_HIP_NO_ERROR);
  std::vector<int> live;
  for (int i = 0; i < a.n; ++i)
    if ((st_[i] = fam.check(a.images[i], host_in, a.out[i], a.out_capacity[i], eo)) == UHDR_HIP_NO_ERROR) live.push_back(i);
  if (live.empty()) return finish_statuses(st_, a.status);
  size_t done = 0;
  const int rc = run_rounds(
      live.size(), Family::kRoundCap, stream,
      [&](size_t k) {   // what one file holds of its round: encoder workspace, the family's planes, page-locked staging of the file
        const uhdr_hip_image_t& im = a.images[live[k]];
        const jpeg::Geometry geom = fam.geometry(im);
        return enc_workspace_bytes(im.width, im.height, geom, eo) + fam.extra_bytes(im, host_in) +
               (host_out ? enc_first_guess(im.width, im.height, geom) : 0);
      },
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        const int* idx = &live[r0];
        std::vector<EncJpeg> im((size_t)m);
        std::vector<std::vector<uint8_t>> iccs((size_t)m);
        int rc = fam.prepare(st, s, a.images, host_in, idx, m, im.data());
        if (rc != UHDR_HIP_NO_ERROR) return rc;
        for (int k = 0; k < m; ++k) {
          const int i = idx[k];
          const void* ip = a.icc ? a.icc[i] : nullptr;
          const size_t in = a.icc ? a.icc_size[i] : 0;
          if (ip != nullptr && in > 0) iccs[(size_t)k].assign(static_cast<const uint8_t*>(ip), static_cast<const uint8_t*>(ip) + in);
          EncJpeg& e = im[(size_t)k];
          e.quality = a.quality[i];
          e.icc = iccs[(size_t)k].empty() ? nullptr : &iccs[(size_t)k];
          eo.to(&e);
          if (host_out) {
            e.keep_max = a.out_capacity[i];   // a file that will not fit is only measured
          } else {
            e.to_dev = true;
            e.dev_out = static_cast<uint8_t*>(a.out[i]);
            e.dev_cap = a.out_capacity[i];
          }
        }
        if ((rc = compress_to_host(st, s, m, im.data())) != UHDR_HIP_NO_ERROR) return rc;
        // the files from the page-locked staging into the caller's buffers: megabytes per 4K file, so a few host threads side by side
        auto deliver = [&](int lo, int hi) {
          for (int k = lo; k < hi; ++k) {
            const int i = idx[k];
            a.out_size[i] = im[(size_t)k].n;
            if (im[(size_t)k].clen_overflow) { st_[i] = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; continue; }
            if (im[(size_t)k].n > a.out_capacity[i]) { st_[i] = UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; continue; }
            if (host_out) memcpy(a.out[i], im[(size_t)k].bytes, im[(size_t)k].n);
            st_[i] = UHDR_HIP_NO_ERROR;
          }
        };
        if (host_out) on_host_threads(m, deliver);
        else deliver(0, m);
        return (int)UHDR_HIP_NO_ERROR;
      },
      &done);
  for (size_t k = done; k < live.size(); ++k) st_[live[k]] = rc;   // the files of a failed round and of those behind it
  return finish_statuses(st_, a.status);
}
}  // namespace

extern "C" {

// uhdr_hip_jpeg_encode for n images in one call (jpeg_encode_files, the planes family)
int uhdr_hip_jpeg_encode_batch(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                               void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream) {
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, EncOpt(), mem_space, stream,
                           PlanesFamily{false});
}
// flags == 0 is uhdr_hip_jpeg_encode_batch.  UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN: every file with Huffman tables of its own (DESIGN.md
// section 7.1.1) -- the same pixels in fewer bytes; a file too large for libjpeg's table search is UNSUPPORTED_FEATURE
int uhdr_hip_jpeg_encode_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                  void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int flags, int mem_space,
                                  void* stream) {
  EncOpt eo;
  const int rc = encode_flags(flags, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           PlanesFamily{false});
}
// opts == NULL, or no restart field set: uhdr_hip_jpeg_encode_batch_ex with opts->flags.  Otherwise every file with restart intervals
// (DESIGN.md section 7.1.2), with either kind of tables
int uhdr_hip_jpeg_encode_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                    void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                    const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           PlanesFamily{false});
}
// uhdr_hip_jpeg_encode_batch_opts with YUV444 / 422 / 440 images compressed as what they are; every other image of
// the call is that call's, and all share the round's launches
int uhdr_hip_jpeg_encode_planes_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                           void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                           const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           PlanesFamily{true});
}

// uhdr_hip_jpeg_encode_planes_batch_opts with the scan mode said: UHDR_HIP_SCANS_BASELINE is that call,
// UHDR_HIP_SCANS_PROGRESSIVE writes every file as libjpeg's jpeg_simple_progression does
int uhdr_hip_jpeg_encode_planes_batch_scans(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                            const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                            const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_scans(opts, scan_mode, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           PlanesFamily{true});
}

// uhdr_hip_jpeg_encode_batch's conventions for RGBA8888 images, compressed as 4:4:4 (Rgba444Family).  No ICC.
int uhdr_hip_jpeg_encode_rgb_batch(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                   size_t* out_size, int* status, int mem_space, void* stream) {
  return jpeg_encode_files(JpegBatch{n, images, quality, nullptr, nullptr, out, out_capacity, out_size, status}, EncOpt(), mem_space, stream,
                           Rgba444Family{});
}
// flags as in uhdr_hip_jpeg_encode_batch_ex
int uhdr_hip_jpeg_encode_rgb_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                      size_t* out_size, int* status, int flags, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_flags(flags, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, nullptr, nullptr, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           Rgba444Family{});
}
// opts as in uhdr_hip_jpeg_encode_batch_opts
int uhdr_hip_jpeg_encode_rgb_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                        size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, nullptr, nullptr, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           Rgba444Family{});
}

// uhdr_hip_jpeg_encode_batch's conventions for RGBA8888 images compressed as 4:2:0 (RgbaSubsampledFamily)
int uhdr_hip_jpeg_encode_rgba420_batch(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                       void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream) {
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, EncOpt(), mem_space, stream,
                           RgbaSubsampledFamily{false});
}
// flags as in uhdr_hip_jpeg_encode_batch_ex
int uhdr_hip_jpeg_encode_rgba420_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                          void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int flags, int mem_space,
                                          void* stream) {
  EncOpt eo;
  const int rc = encode_flags(flags, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           RgbaSubsampledFamily{false});
}
// opts as in uhdr_hip_jpeg_encode_batch_opts
int uhdr_hip_jpeg_encode_rgba420_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                            const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                            const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpeg_encode_files(JpegBatch{n, images, quality, icc, icc_size, out, out_capacity, out_size, status}, eo, mem_space, stream,
                           RgbaSubsampledFamily{false});
}
// RGBA8888 images at the sampling said: YUV420 is the call above, YUV444 uhdr_hip_jpeg_encode_rgb_batch_opts'
// file with an APP2 segment for a file's ICC profile where the other calls put it, YUV422 the 4:2:0 call's course with
// k_rgba_to_ycc422 in front
int uhdr_hip_jpeg_encode_rgba_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                         void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int sampling,
                                         const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  const JpegBatch a{n, images, quality, icc, icc_size, out, out_capacity, out_size, status};
  if (sampling == UHDR_HIP_PIX_FMT_YUV444) return jpeg_encode_files(a, eo, mem_space, stream, Rgba444Family{});
  if (sampling != UHDR_HIP_PIX_FMT_YUV422 && sampling != UHDR_HIP_PIX_FMT_YUV420) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return jpeg_encode_files(a, eo, mem_space, stream, RgbaSubsampledFamily{sampling == UHDR_HIP_PIX_FMT_YUV422});
}
// the same with the scan mode said, as uhdr_hip_jpeg_encode_planes_batch_scans takes it
int uhdr_hip_jpeg_encode_rgba_batch_scans(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                          void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int sampling,
                                          const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_scans(opts, scan_mode, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  const JpegBatch a{n, images, quality, icc, icc_size, out, out_capacity, out_size, status};
  if (sampling == UHDR_HIP_PIX_FMT_YUV444) return jpeg_encode_files(a, eo, mem_space, stream, Rgba444Family{});
  if (sampling != UHDR_HIP_PIX_FMT_YUV422 && sampling != UHDR_HIP_PIX_FMT_YUV420) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return jpeg_encode_files(a, eo, mem_space, stream, RgbaSubsampledFamily{sampling == UHDR_HIP_PIX_FMT_YUV422});
}


// Diagnostics (host only, no GPU): the quantised coefficients of a PROGRESSIVE file after all of its scans, as the host-side
// entropy decoder hands them to the device (csrc/uhdr_jpeg_prog.cpp) -- blocks in MCU order, zigzag order inside a block, DC as the
// value.  tests/test_jpeg_progressive.py compares them with libjpeg's jpeg_read_coefficients.  Returns the number of blocks through
// *blocks; baseline files: UNSUPPORTED_FEATURE (their entropy decoding runs on the device).
int uhdr_hip_jpeg_progressive_coefficients(const void* jpeg, size_t jpeg_size, int16_t* coef, size_t capacity_blocks, size_t* blocks, int* width,
                                           int* height, int* gray) {
  if (jpeg == nullptr || blocks == nullptr || width == nullptr || height == nullptr || gray == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  jpeg::DecInfo info;
  const int prc = jpeg::parse_header(static_cast<const uint8_t*>(jpeg), jpeg_size, &info);
  if (prc == -3) return UHDR_HIP_UNKNOWN_ERROR;   // host allocation failed; INSUFFICIENT_RESOURCE is the size-probe answer (*blocks set)
  if (prc == -2 || (prc == 0 && !info.progressive)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (prc != 0) return UHDR_HIP_UNKNOWN_ERROR;
  *width = info.w; *height = info.h; *gray = info.gray;
  *blocks = info.coef.size() / 64u;
  if (coef == nullptr || capacity_blocks < *blocks) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  memcpy(coef, info.coef.data(), info.coef.size() * sizeof(int16_t));
  int prev[3] = {0, 0, 0};   // differences back to values
  for (size_t b = 0; b < *blocks; ++b) {
    const int c = info.gray ? 0 : ((b % 6u) < 4u ? 0 : (int)(b % 6u) - 3);
    prev[c] += coef[b * 64u];
    coef[b * 64u] = (int16_t)prev[c];
  }
  return UHDR_HIP_NO_ERROR;
}

}  // extern "C"

namespace {
// what the host learns from one JPEG/R file before anything is launched: the checks and the parsing of decodeJPEGR up to its
// first decompressImage call (jpegr.cpp:655-699) plus what it reads from the decoders afterwards (XMP :756-760, ICC :796-801)
struct JpegrFile {
  const uint8_t* jpg[2] = {nullptr, nullptr};   // primary image, gain map
  size_t len[2] = {0, 0};
  jpeg::DecInfo info[2];
  uhdr_hip_metadata_t md;
  int gamut = UHDR_HIP_CG_UNSPECIFIED;
};
// The image that starts at `begin`, found through its header: the header parser's walk over the (only) scan of a baseline file
// ends at EOI, and that is where the image ends.  Anything else -- more scans, other markers behind the scan, a header this decoder
// does not read -- is left to the container's own marker walk (jpegr::find_images), which then walks the scan a second time.
bool image_by_header(const uint8_t* file, size_t n, size_t begin, jpeg::DecInfo* info, size_t* len, bool any_sampling) {
  if (begin + 4 > n || jpeg::parse_header(file + begin, n - begin, info, any_sampling) != 0) return false;
  const size_t e = begin + info->scan_offset + info->scan_bytes;
  if (e + 2 > n || file[e] != 0xFF || file[e + 1] != 0xD9) return false;
  *len = e + 2 - begin;
  return true;
}

// any_sampling: of the primary image; map_any_sampling: of the gain map (the rgbmap decode reads three-component maps of every
// sampling the RGBA conversion handles whatever the flag says of the primary)
int parse_jpegr_file(const void* jpegr, size_t jpegr_size, int output_format, bool want_metadata, JpegrFile* f, bool any_sampling,
                     bool map_any_sampling) {
  const uint8_t* file = static_cast<const uint8_t*>(jpegr);
  const bool sdr = output_format == UHDR_HIP_OUTPUT_SDR;   // the gain map is neither decompressed nor (unless asked for) read (:728, :754)
  jpegr::Range img[2];
  bool by_header = false;   // both ranges and both headers in one walk per image (the file the reference's encoder writes)
  bool have0 = false;       // the primary image at least (kept when the second image needs the container's walk: a progressive
                            // primary has had all its scans entropy-decoded by then, once is enough)
  size_t len0 = 0;
  if (file != nullptr && jpegr_size >= 4 && file[0] == 0xFF && file[1] == 0xD8 && image_by_header(file, jpegr_size, 0, &f->info[0], &img[0].len, any_sampling)) {
    have0 = true; len0 = img[0].len;
    img[0].begin = 0;
    size_t pos = img[0].len;
    while (pos + 1 < jpegr_size) {   // the next SOI, as find_images looks for it
      const void* q = memchr(file + pos, 0xFF, jpegr_size - 1 - pos);
      if (q == nullptr) break;
      pos = (size_t)(static_cast<const uint8_t*>(q) - file);
      if (file[pos + 1] == 0xD8) {
        by_header = image_by_header(file, jpegr_size, pos, &f->info[1], &img[1].len, map_any_sampling);
        img[1].begin = pos;
        break;
      }
      pos++;
    }
  }
  if (!by_header) {
    const int found = jpegr::find_images(file, jpegr_size, img);                                        // :823-876
    if (found == 0) return UHDR_HIP_ERROR_NO_IMAGES_FOUND;
    if (found == 1) return UHDR_HIP_ERROR_GAIN_MAP_IMAGE_NOT_FOUND;
  }
  for (int k = 0; k < (sdr ? 1 : 2); ++k) {   // the headers, parsed once (jpeg_read_header of either decompressImage call, :690-694 / :731-733)
    f->jpg[k] = file + img[k].begin; f->len[k] = img[k].len;
    const bool parsed = by_header || (k == 0 && have0 && img[0].begin == 0 && img[0].len == len0);
    const int prc = parsed ? 0 : jpeg::parse_header(f->jpg[k], f->len[k], &f->info[k], k == 0 ? any_sampling : map_any_sampling);
    if (prc == -3) return UHDR_HIP_UNKNOWN_ERROR;   // host allocation failed (never the capacity-probe status)
    if (prc == -2) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (prc != 0 || f->info[k].w > 8192 || f->info[k].h > 8192) return UHDR_HIP_ERROR_DECODE_ERROR;
  }
  if (f->info[0].gray) return UHDR_HIP_ERROR_DECODE_ERROR;   // the primary image must come back as three planes
  // metadata from the gain map's XMP packet (:754-760)
  f->jpg[1] = file + img[1].begin; f->len[1] = img[1].len;
  if (!sdr || want_metadata) {
    const uint8_t* xmp = nullptr;
    size_t xmp_len = 0;
    if (!jpegr::first_xmp(f->jpg[1], f->len[1], &xmp, &xmp_len) || !jpegr::metadata_from_xmp(xmp, xmp_len, &f->md))
      return UHDR_HIP_ERROR_METADATA_ERROR;
  }
  const uint8_t* icc = nullptr;
  size_t icc_len = 0;
  f->gamut = jpegr::first_icc(f->jpg[0], f->len[0], &icc, &icc_len) ? jpegr::gamut_from_icc(icc, icc_len)
                                                                                                             : UHDR_HIP_CG_UNSPECIFIED;
  return UHDR_HIP_NO_ERROR;
}

// What a decoded image looks like in memory: the w x h luma plane, then Cb and Cr of cw x ch samples each, cbytes apart.  4:2:0
// keeps the reference's (w / 2) x (h / 2) planes luma / 4 bytes apart (even sizes; odd ones as before); the samplings only the
// any-sampling decode parses get libjpeg's downsampled sizes, ceil(w / hs) x ceil(h / vs), packed.
// An image decoded at 1 / info.scale (the *_scaled calls; 1 everywhere else) is the image jpeg::scaled_geometry describes: w x h luma of
// the scaled extent and the sampling of the result, which for a 4:2:0 file at 1/2, 1/4, 1/8 is 4:4:4 -- its layout never 4:2:0's.
struct DecGeom { size_t w, h; int hs, vs; size_t cw, ch, cbytes; int fmt; };
DecGeom dec_geom(const jpeg::DecInfo& info) {
  const jpeg::ScaledGeom sg = jpeg::scaled_geometry(info.w, info.h, info.hs, info.vs, info.gray != 0, info.scale);
  const size_t w = (size_t)sg.w, h = (size_t)sg.h;
  if (info.gray) return DecGeom{w, h, 1, 1, 0, 0, 0, UHDR_HIP_PIX_FMT_MONOCHROME};
  if (sg.hs == 2 && sg.vs == 2) return DecGeom{w, h, 2, 2, w / 2, h / 2, w * h / 4, UHDR_HIP_PIX_FMT_YUV420};
  const size_t cw = (w + sg.hs - 1) / sg.hs, ch = (h + sg.vs - 1) / sg.vs;
  return DecGeom{w, h, sg.hs, sg.vs, cw, ch, cw * ch, sg.hs == 2 ? UHDR_HIP_PIX_FMT_YUV422 : sg.vs == 2 ? UHDR_HIP_PIX_FMT_YUV440 : UHDR_HIP_PIX_FMT_YUV444};
}
// libjpeg-turbo's RGBA of an odd-sized 4:2:0 image is outside the conversion kernels (uhdr_hip_jpeg_decode_rgba: UNSUPPORTED_FEATURE)
bool rgba_refuses(const DecGeom& g) { return g.fmt == UHDR_HIP_PIX_FMT_YUV420 && ((g.w | g.h) & 1) != 0; }
// a decoded image at p as the apply calls read it: its planes in `fmt` = g.fmt, its first plane alone (MONOCHROME), or the RGBA made of it
uhdr_hip_image_t dec_image(const DecGeom& g, void* p, int fmt, int gamut) {
  uhdr_hip_image_t im;
  memset(&im, 0, sizeof(im));
  im.data = p; im.width = g.w; im.height = g.h; im.luma_stride = g.w; im.colorGamut = gamut; im.pixelFormat = fmt;
  if (fmt != UHDR_HIP_PIX_FMT_MONOCHROME && fmt != UHDR_HIP_PIX_FMT_RGBA8888) { im.chroma_data = static_cast<uint8_t*>(p) + g.w * g.h; im.chroma_stride = g.cw; }
  return im;
}
// the gates every decode call shares, in this order: the denominator (1 where the call has none), then the flags
int decode_gate(int flags, int scale_denom) {
  if (scale_denom != 1 && scale_denom != 2 && scale_denom != 4 && scale_denom != 8) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return (flags & ~UHDR_HIP_DECODE_ANY_SAMPLING) != 0 ? UHDR_HIP_ERROR_UNSUPPORTED_FEATURE : UHDR_HIP_NO_ERROR;
}
int decode_to_gate(int to) { return to != UHDR_HIP_DECODE_TO_RGBA && to != UHDR_HIP_DECODE_TO_YCBCR ? UHDR_HIP_ERROR_UNSUPPORTED_FEATURE : UHDR_HIP_NO_ERROR; }
// the three planes of a decode into the packed buffer at p
void dec_planes(const jpeg::DecInfo& info, uint8_t* p, jpeg::DecPlane out[3]);
// an image's entry in either RGBA conversion batch (4:2:0: k_ycc420_rgba_batch, the other samplings: k_yccx_rgba_batch)
struct RgbaBatches {
  YccRgbaBatch b420; int n420 = 0;
  YccxRgbaBatch bx; int nx = 0;
  uint8_t* add(const jpeg::DecInfo& info, const uint8_t* ycc, uint8_t* rgba) {
    const DecGeom g = dec_geom(info);
    const size_t luma = g.w * g.h;
    const YccRgbaImage im{ycc, ycc + luma, ycc + luma + g.cbytes, rgba, (uint32_t)g.w, (uint32_t)g.h, (uint32_t)g.w, (uint32_t)g.cw};
    if (g.fmt == UHDR_HIP_PIX_FMT_YUV420) b420.img[n420++] = im;
    else bx.img[nx++] = YccxRgbaImage{im, (uint32_t)g.hs, (uint32_t)g.vs, info.scale == 8 ? 1u : 0u};   // (at 1/8 libjpeg replicates the chroma)
    return rgba;
  }
  int size() const { return n420 + nx; }
  hipError_t launch(hipStream_t s) {
    hipError_t e = launch_ycc420_to_rgba_batch(b420, n420, s);
    if (e == hipSuccess) e = launch_yccx_to_rgba_batch(bx, nx, s);
    n420 = nx = 0;
    return e;
  }
};

// The host part of uhdr_hip_jpeg_decode (rgba false) or uhdr_hip_jpeg_decode_rgba (rgba true) for one file: the checks in their
// order, the header parsed into *info, *desc filled.  NO_ERROR: the file is decoded on the device into `need` bytes at out.
// INSUFFICIENT_RESOURCE is the size-probe answer (out == NULL / capacity too small: the header parsed and *desc is filled); every
// status returned before that point leaves *desc zeroed (the RGBA call: untouched), and a host allocation failure inside the parser
// (std::bad_alloc, -3: a progressive file's coefficient array) is reported as UNKNOWN_ERROR so that it cannot be taken for it.
int jpeg_decode_host(const void* jpeg, size_t jpeg_size, bool rgba, bool any_sampling, void* out, size_t out_capacity, uhdr_hip_image_t* desc,
                     jpeg::DecInfo* info, size_t* need, int scale_denom = 1) {
  if (jpeg == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (!rgba) memset(desc, 0, sizeof(*desc));
  const int prc = jpeg::parse_header(static_cast<const uint8_t*>(jpeg), jpeg_size, info, any_sampling);
  if (prc == -3) return UHDR_HIP_UNKNOWN_ERROR;
  if (prc == -2) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (prc != 0 || info->w <= 0 || info->h <= 0) return UHDR_HIP_UNKNOWN_ERROR;
  if (info->w > 8192 || info->h > 8192) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;   // kMaxWidth / kMaxHeight, jpegdecoderhelper.h:42-43
  info->scale = scale_denom;   // from here on the image is the scaled one: extent, layout, bytes
  const DecGeom g = dec_geom(*info);
  const size_t w = g.w, h = g.h, luma = w * h;
  if (!rgba) {
    *need = luma + 2 * g.cbytes;
    desc->data = out;
    desc->width = w; desc->height = h;
    desc->colorGamut = UHDR_HIP_CG_UNSPECIFIED;
    desc->luma_stride = w;
    desc->chroma_data = info->gray ? nullptr : static_cast<uint8_t*>(out) + luma;
    desc->chroma_stride = g.cw;
    desc->pixelFormat = g.fmt;
    return out == nullptr || out_capacity < *need ? UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE : UHDR_HIP_NO_ERROR;
  }
  if (info->gray) return UHDR_HIP_UNKNOWN_ERROR;   // jpegdecoderhelper.cpp:258-270: YCbCr 4:2:0 only
  *need = luma * 4;
  memset(desc, 0, sizeof(*desc));
  desc->data = out; desc->width = w; desc->height = h; desc->colorGamut = UHDR_HIP_CG_UNSPECIFIED; desc->luma_stride = w;
  desc->pixelFormat = UHDR_HIP_PIX_FMT_UNSPECIFIED;
  if (out == nullptr || out_capacity < *need) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if (rgba_refuses(g)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return UHDR_HIP_NO_ERROR;
}

// The decode paths' pool slots: decode_images' workspaces, pooled planes and scratch; the JPEG batch's RGBA staging of a host caller; the
// JPEG/R round's three-component maps as RGBA and a host caller's renditions, in slots no other codec path names (the encode paths hold
// 0-6 and 8-10).  The uhdr_hip_apply_gainmap* calls nested in that round touch no slot: they work in the device's own state, not the lease's.
enum : size_t { kDecWs = 0, kDecPlanes, kDecRgba, kDecScratch, kJrMapRgba = 11, kJrOut = 12 };
constexpr int kDecRound = kRgbaChunk;   // files per JPEG decode round: their RGBA conversion is one launch

// a packed w x h plane at p for the decoder to write
jpeg::DecPlane dec_plane(uint8_t* p, size_t w, size_t h) {
  jpeg::DecPlane q;
  q.p = p; q.w = (int)w; q.h = (int)h; q.stride = (int)w;
  q.aligned8 = (reinterpret_cast<uintptr_t>(p) % 8 == 0 && w % 8 == 0) ? 1 : 0;
  return q;
}
size_t dec_ycc_bytes(const jpeg::DecInfo& info) { const DecGeom g = dec_geom(info); return g.w * g.h + 2 * g.cbytes; }
// An odd-sized 4:2:0 image at full size.  The decoder writes (w / 2) x (h / 2) chroma planes with Cr w h / 4 bytes behind Cb, while
// applyGainMap looks for Cr chroma_stride (h / 2) bytes behind Cb and reads up to floor(3 w h / 2) bytes from the luma on.  The reference
// decodes into a zeroed buffer of that size (jpegdecoderhelper.cpp:291, :360-362; jpegr.cpp:796-801), so the bytes the decoder leaves
// alone are zeros here too (decode_images).  dec_pooled_bytes: what a pooled plane set holds -- floor(3 w h / 2) exceeds dec_ycc_bytes
// by one byte where w h mod 4 is 2 or 3.
bool dec_odd_420(const jpeg::DecInfo& info, const DecGeom& g) { return info.scale == 1 && g.fmt == UHDR_HIP_PIX_FMT_YUV420 && ((g.w | g.h) & 1) != 0; }
size_t dec_pooled_bytes(const jpeg::DecInfo& info) {
  const DecGeom g = dec_geom(info);
  const size_t need = g.w * g.h + 2 * g.cbytes, read = g.w * g.h * 3 / 2;
  return dec_odd_420(info, g) && read > need ? read : need;
}
void dec_planes(const jpeg::DecInfo& info, uint8_t* p, jpeg::DecPlane out[3]) {
  const DecGeom g = dec_geom(info);
  const size_t luma = g.w * g.h;
  memset(out, 0, 3 * sizeof(jpeg::DecPlane));
  out[0] = dec_plane(p, g.w, g.h);
  if (!info.gray) { out[1] = dec_plane(p + luma, g.cw, g.ch); out[2] = dec_plane(p + luma + g.cbytes, g.cw, g.ch); }
}
// what one file holds of its round
size_t dec_round_bytes(const jpeg::DecInfo& info, bool rgba, bool host_out, size_t need) {
  jpeg::DecLayout l;
  size_t b = jpeg::dec_workspace_bytes(info, &l);
  if (rgba || host_out) b += dec_pooled_bytes(info) + 64;
  if (rgba && host_out) b += need;
  return b;
}

// one image of a device decode: its header, its entropy-coded segment on the host, where its planes go (nullptr: a slice of kDecPlanes)
struct DecImage { const jpeg::DecInfo* info; const uint8_t* scan; uint8_t* out; };

// The decode every round shares, enqueued on s: workspaces as 256-aligned slices of kDecWs, pooled planes as slices of kDecPlanes,
// kDecScratch, the segments copied up, one jpeg::decode_device_batch for all.  ycc[k]: image k's planes (dec_planes' layout); image_rc[k]
// != 0: corrupt entropy-coded data.  A non-zero return is an error of the device or the runtime (`who` names the call in its message).
int decode_images(DeviceState* st, hipStream_t s, const char* who, const std::vector<DecImage>& im, std::vector<uint8_t*>* ycc,
                  std::vector<int>* image_rc) {
  const size_t m = im.size();
  std::vector<jpeg::DecLayout> lay(m);
  std::vector<size_t> ws_off(m), pl_off(m);
  size_t ws_total = 0, pl_total = 0;
  for (size_t k = 0; k < m; ++k) {
    ws_off[k] = ws_total; pl_off[k] = pl_total;
    ws_total += round_up(jpeg::dec_workspace_bytes(*im[k].info, &lay[k]), 256);
    if (im[k].out == nullptr) pl_total += round_up(dec_pooled_bytes(*im[k].info) + 64, 256);
  }
  int rc;
  if ((rc = pool_reserve(st, kDecWs, ws_total)) != 0) return rc;
  if ((rc = pool_reserve(st, kDecPlanes, pl_total)) != 0) return rc;
  if ((rc = pool_reserve(st, kDecScratch, jpeg::dec_batch_scratch_bytes((int)m, lay.data()))) != 0) return rc;
  std::vector<const jpeg::DecInfo*> infos(m);
  std::vector<uint8_t*> wss(m);
  std::vector<jpeg::DecPlane> planes(3 * m);
  std::vector<jpeg::DecPlane (*)[3]> pl(m);
  ycc->assign(m, nullptr); image_rc->assign(m, 0);
  for (size_t k = 0; k < m; ++k) {
    const jpeg::DecInfo& in = *im[k].info;
    infos[k] = &in;
    wss[k] = static_cast<uint8_t*>(st->pool[kDecWs]) + ws_off[k];
    if (in.scan_bytes) HIP_TRY(hipMemcpyAsync(wss[k] + lay[k].src, im[k].scan, in.scan_bytes, hipMemcpyHostToDevice, s));
    (*ycc)[k] = im[k].out != nullptr ? im[k].out : static_cast<uint8_t*>(st->pool[kDecPlanes]) + pl_off[k];
    dec_planes(in, (*ycc)[k], &planes[3 * k]);
    pl[k] = reinterpret_cast<jpeg::DecPlane (*)[3]>(&planes[3 * k]);
    const DecGeom g = dec_geom(in);
    if (dec_odd_420(in, g)) {   // zeros where the reference has them: the gap behind Cb, and behind Cr to the end of what is read (pooled
                                // planes) or of the caller's `need` bytes
      const size_t luma = g.w * g.h, cwh = g.cw * g.ch, end = im[k].out != nullptr ? dec_ycc_bytes(in) : dec_pooled_bytes(in);
      if (g.cbytes > cwh) HIP_TRY(hipMemsetAsync((*ycc)[k] + luma + cwh, 0, g.cbytes - cwh, s));
      if (end > luma + g.cbytes + cwh) HIP_TRY(hipMemsetAsync((*ycc)[k] + luma + g.cbytes + cwh, 0, end - (luma + g.cbytes + cwh), s));
    }
  }
  hipError_t herr = hipSuccess;
  const int drc = jpeg::decode_device_batch((int)m, infos.data(), lay.data(), wss.data(), pl.data(), s, static_cast<uint8_t*>(st->pool[kDecScratch]), &herr,
                                            image_rc->data());
  if (drc > 0) { set_err(who, herr); return UHDR_HIP_UNKNOWN_ERROR; }
  return UHDR_HIP_NO_ERROR;
}

// One round of uhdr_hip_jpeg_decode_batch: files idx[0, m) (m <= kDecRound) through decode_images, their RGBA conversion through one
// k_ycc420_rgba_batch launch, then one synchronisation.  A file whose device decode fails gets UNKNOWN_ERROR in st_; a non-zero return
// is an error of the device or the runtime.
int jpeg_decode_round(DeviceState* st, hipStream_t s, bool rgba, bool host_out, const void* const* jpeg, void* const* out,
                      const jpeg::DecInfo* info, const size_t* need, const int* idx, int m, int* st_) {
  std::vector<DecImage> im((size_t)m);
  std::vector<size_t> rg_off((size_t)m);
  size_t rg_total = 0;
  for (int k = 0; k < m; ++k) {
    const int i = idx[k];
    // YCbCr to a device caller: straight into its buffer
    im[k] = DecImage{&info[i], static_cast<const uint8_t*>(jpeg[i]) + info[i].scan_offset, rgba || host_out ? nullptr : static_cast<uint8_t*>(out[i])};
    rg_off[k] = rg_total;
    if (rgba && host_out) rg_total += round_up(need[i], 256);
  }
  int rc;
  if ((rc = pool_reserve(st, kDecRgba, rg_total)) != 0) return rc;
  std::vector<uint8_t*> ycc; std::vector<int> image_rc;
  if ((rc = decode_images(st, s, "uhdr_hip_jpeg_decode", im, &ycc, &image_rc)) != 0) return rc;
  RgbaBatches b;
  std::vector<uint8_t*> res((size_t)m, nullptr);   // where each good file's output lies on the device
  for (int k = 0; k < m; ++k) {
    const int i = idx[k];
    if (image_rc[k] != 0) {
      st_[i] = UHDR_HIP_UNKNOWN_ERROR;
      snprintf(t_err, sizeof(t_err), "uhdr_hip_jpeg_decode: corrupt entropy-coded data");
      continue;
    }
    res[k] = ycc[k];
    if (rgba)   // libjpeg-turbo's DECODE_TO_RGBA on the planes just decoded
      res[k] = b.add(info[i], ycc[k], host_out ? static_cast<uint8_t*>(st->pool[kDecRgba]) + rg_off[k] : static_cast<uint8_t*>(out[i]));
  }
  HIP_TRY(b.launch(s));
  if (host_out)
    for (int k = 0; k < m; ++k)
      if (res[k] != nullptr) HIP_TRY(hipMemcpyAsync(out[idx[k]], res[k], need[idx[k]], hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return UHDR_HIP_NO_ERROR;
}

// ---- decodeJPEGR for n files (the uhdr_hip_jpegr_decode* calls) --------------------------------------------------------------------
// The caller's arguments, and what the entry points differ in.  rgb_maps: a three-component map, of any sampling the RGBA conversion handles,
// is applied per channel through its RGBA.  any_md: metadata that validate_apply refuses goes through uhdr_hip_apply_gainmap_md_batch.
struct JrBatch {
  int n; const void* const* jpegr; const size_t* jpegr_size; int output_format; float max_display_boost; void* const* dest_data;
  const size_t* dest_capacity; uhdr_hip_image_t* dests; uhdr_hip_metadata_t* metadata; int* status; int apply_mode, mem_space; void* stream; int flags;
};
struct JrOpt { bool rgb_maps = false, any_md = false; int scale_denom = 1; };
// whether a file's three-component map goes through its RGBA, that RGBA's bytes, and what the file holds of its round: workspaces and
// planes (SDR: of the primary image alone), the RGBA, a host caller's rendition
bool jr_rgb_map(const JrBatch& a, const JrOpt& o, const JpegrFile& f) { return o.rgb_maps && a.output_format != UHDR_HIP_OUTPUT_SDR && !f.info[1].gray; }
size_t jr_map_rgba_bytes(const JpegrFile& f) { const DecGeom g = dec_geom(f.info[1]); return g.w * g.h * 4; }
size_t jr_round_bytes(const JrBatch& a, const JrOpt& o, const JpegrFile& f, size_t out_bytes) {
  return dec_round_bytes(f.info[0], false, true, 0) + (a.output_format != UHDR_HIP_OUTPUT_SDR ? dec_round_bytes(f.info[1], false, true, 0) : 0) +
         (jr_rgb_map(a, o, f) ? jr_map_rgba_bytes(f) : 0) + (a.mem_space != UHDR_HIP_MEM_DEVICE ? out_bytes : 0);
}

// One round of JPEG/R files idx[0, m): both images of every file through decode_images, one apply call per HDR file in the caller's order,
// one synchronisation; every per-file buffer a 256-aligned slice of a slot.  Statuses go to st_; non-zero: an error of the device or the runtime.
int jpegr_decode_round(DeviceState* st, hipStream_t s, const JrBatch& a, const JrOpt& o, const JpegrFile* files, const size_t* out_bytes,
                       const int* idx, int m, int* st_) {
  const bool sdr = a.output_format == UHDR_HIP_OUTPUT_SDR, host = a.mem_space != UHDR_HIP_MEM_DEVICE;
  const size_t per_file = sdr ? 1 : 2;   // the SDR rendition is the primary image alone (:768-786)
  std::vector<DecImage> im;
  std::vector<size_t> map_off((size_t)m), out_off((size_t)m);
  size_t map_total = 0, out_total = 0;
  for (int k = 0; k < m; ++k) {
    const JpegrFile& f = files[idx[k]];
    for (size_t j = 0; j < per_file; ++j) im.push_back(DecImage{&f.info[j], f.jpg[j] + f.info[j].scan_offset, nullptr});
    map_off[k] = map_total; out_off[k] = out_total;
    if (jr_rgb_map(a, o, f)) map_total += round_up(jr_map_rgba_bytes(f), 256);
    if (host) out_total += round_up(out_bytes[idx[k]], 256);
  }
  int rc;
  if (map_total && (rc = pool_reserve(st, kJrMapRgba, map_total)) != 0) return rc;
  if (out_total && (rc = pool_reserve(st, kJrOut, out_total)) != 0) return rc;
  std::vector<uint8_t*> ycc; std::vector<int> image_rc;
  if ((rc = decode_images(st, s, "uhdr_hip_jpegr_decode", im, &ycc, &image_rc)) != 0) return rc;
  for (size_t g = 0; g < im.size(); ++g)
    if (image_rc[g] != 0) st_[idx[g / per_file]] = UHDR_HIP_ERROR_DECODE_ERROR;
  // three-component maps: an odd-sized 4:2:0 map is refused as uhdr_hip_jpeg_decode_rgba refuses the file (full size only: a scaled map is never 4:2:0)
  RgbaBatches mb;
  for (int k = 0; k < m; ++k) {
    const JpegrFile& f = files[idx[k]];
    if (st_[idx[k]] != UHDR_HIP_NO_ERROR || !jr_rgb_map(a, o, f)) continue;
    if (rgba_refuses(dec_geom(f.info[1]))) { st_[idx[k]] = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; continue; }
    mb.add(f.info[1], ycc[2 * (size_t)k + 1], static_cast<uint8_t*>(st->pool[kJrMapRgba]) + map_off[k]);
    if (mb.size() == kRgbaChunk) HIP_TRY(mb.launch(s));
  }
  HIP_TRY(mb.launch(s));
  // the renditions.  SDR: libjpeg-turbo's DECODE_TO_RGBA on the planes just decoded (k_ycc420_rgba_batch / k_yccx_rgba_batch), up to
  // kRgbaChunk files per launch.  HDR, :796-801: the planes as an image with the ICC gamut under the first plane of the map's JPEG, or its RGBA
  RgbaBatches rgb;
  for (int k = 0; k < m; ++k) {
    const int i = idx[k];
    if (st_[i] != UHDR_HIP_NO_ERROR) continue;
    const JpegrFile& f = files[i];
    const DecGeom pg = dec_geom(f.info[0]);
    uint8_t* yp = ycc[per_file * (size_t)k];
    uint8_t* out = host ? static_cast<uint8_t*>(st->pool[kJrOut]) + out_off[k] : static_cast<uint8_t*>(a.dest_data[i]);
    if (sdr) {
      if (rgba_refuses(pg)) { st_[i] = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; continue; }
      rgb.add(f.info[0], yp, out);
      if (rgb.size() == kRgbaChunk) HIP_TRY(rgb.launch(s));
    } else {
      const bool rgb_map = jr_rgb_map(a, o, f);
      uint8_t* mp = rgb_map ? static_cast<uint8_t*>(st->pool[kJrMapRgba]) + map_off[k] : ycc[2 * (size_t)k + 1];
      const uhdr_hip_image_t ydesc = dec_image(pg, yp, pg.fmt, f.gamut);
      const uhdr_hip_image_t gimg = dec_image(dec_geom(f.info[1]), mp, rgb_map ? UHDR_HIP_PIX_FMT_RGBA8888 : UHDR_HIP_PIX_FMT_MONOCHROME, UHDR_HIP_CG_UNSPECIFIED);
      uhdr_hip_image_t ddev = a.dests[i];
      ddev.data = out;
      if (o.any_md && !md_degenerate(f.md))   // (degenerate metadata: the path and the bytes of the rgbmap decode)
        st_[i] = uhdr_hip_apply_gainmap_md_batch(1, &ydesc, &gimg, &f.md, a.output_format, a.max_display_boost, &ddev, a.apply_mode, a.stream);
      else if (rgb_map)
        st_[i] = uhdr_hip_apply_gainmap_rgb_batch(1, &ydesc, &gimg, &f.md, a.output_format, a.max_display_boost, &ddev, a.apply_mode, a.stream);
      else
        st_[i] = uhdr_hip_apply_gainmap(&ydesc, &gimg, &f.md, a.output_format, a.max_display_boost, &ddev, a.apply_mode, UHDR_HIP_MEM_DEVICE, a.stream);
      if (st_[i] != UHDR_HIP_NO_ERROR) continue;
      a.dests[i].width = ddev.width; a.dests[i].height = ddev.height;
    }
    a.dests[i].data = a.dest_data[i];
  }
  HIP_TRY(rgb.launch(s));
  for (int k = 0; host && k < m; ++k)   // a host caller's renditions go down behind the last launch
    if (st_[idx[k]] == UHDR_HIP_NO_ERROR)
      HIP_TRY(hipMemcpyAsync(a.dest_data[idx[k]], static_cast<uint8_t*>(st->pool[kJrOut]) + out_off[k], out_bytes[idx[k]], hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return UHDR_HIP_NO_ERROR;
}

// JpegR::decodeJPEGR (jpegr.cpp:655-822) for n files: checks and parsing on the host, then the live files through jpegr_decode_round in
// rounds held to the byte bound alone -- a device decode is latency-bound, so every image of a call that fits shares each launch.  A
// round that fails on the device ends the call with its status; status[] holds the other files' own and it for its files and those behind.
int jpegr_decode_files(const JrBatch& a, const JrOpt& o) {
  const int n = a.n;
  int rc = decode_gate(a.flags, o.scale_denom);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  const bool any_sampling = (a.flags & UHDR_HIP_DECODE_ANY_SAMPLING) != 0;
  if (n < 0 || (n > 0 && (a.jpegr == nullptr || a.jpegr_size == nullptr || a.dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  if (a.max_display_boost < 1.0f || (o.any_md && std::isnan(a.max_display_boost))) return UHDR_HIP_ERROR_INVALID_DISPLAY_BOOST;   // :666-669
  if (a.output_format < UHDR_HIP_OUTPUT_SDR || a.output_format > UHDR_HIP_OUTPUT_HDR_LINEAR_RGB_10BIT) return UHDR_HIP_ERROR_INVALID_OUTPUT_FORMAT;
  std::vector<JpegrFile> files((size_t)n);
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  std::vector<size_t> out_bytes((size_t)n, 0);
  // walking a 2 MB file's markers costs ~0.2 ms of host time and touches nothing shared: a few threads parse the files side by side
  on_host_threads(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i)
      st_[i] = a.jpegr[i] == nullptr ? UHDR_HIP_ERROR_BAD_PTR
                                     : parse_jpegr_file(a.jpegr[i], a.jpegr_size[i], a.output_format, a.metadata != nullptr, &files[i], any_sampling, any_sampling || o.rgb_maps);
  });
  std::vector<int> live;
  for (int i = 0; i < n; ++i) {
    if (st_[i] != UHDR_HIP_NO_ERROR) continue;
    if (a.metadata != nullptr) a.metadata[i] = files[i].md;
    if (o.scale_denom != 1) {
      // the map's denominator.  With f = W / MW (W = f MW, H = f MH): f % s == 0 leaves the map whole, ceil(W / s) = (f / s) MW; s % f == 0
      // takes it to 1 / (s / f), ceil(W / s) = ceil(MW / (s / f)): an exact ratio either way
      jpeg::DecInfo& pi = files[i].info[0];
      jpeg::DecInfo& gi = files[i].info[1];
      pi.scale = o.scale_denom;
      if (a.output_format != UHDR_HIP_OUTPUT_SDR) {
        const int f = gi.w > 0 && gi.h > 0 && pi.w % gi.w == 0 && pi.h % gi.h == 0 && (size_t)pi.w * (size_t)gi.h == (size_t)pi.h * (size_t)gi.w ? pi.w / gi.w : 0;
        if (f != 0 && f % o.scale_denom == 0) gi.scale = 1;
        else if (f != 0 && o.scale_denom % f == 0) gi.scale = o.scale_denom / f;
        else {   // the map cannot follow its primary image: known from the two headers, so the file stops here, in front of its size probe
          // (the apply call's metadata checks stand in front of its scale-factor checks)
          const int mrc = validate_md(&files[i].md);
          st_[i] = mrc != UHDR_HIP_NO_ERROR ? mrc : UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
          continue;
        }
      }
    }
    const DecGeom og = dec_geom(files[i].info[0]);
    a.dests[i].width = og.w; a.dests[i].height = og.h; a.dests[i].colorGamut = files[i].gamut;
    out_bytes[i] = og.w * og.h * apply_bpp(a.output_format);
    if (a.dest_data == nullptr || a.dest_capacity == nullptr || a.dest_data[i] == nullptr || a.dest_capacity[i] < out_bytes[i]) { st_[i] = UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; continue; }
    live.push_back(i);
  }
  if (live.empty()) return finish_statuses(st_, a.status);   // every file stopped at its checks or its size probe: the device is not touched
  size_t done = 0;
  rc = run_rounds(
      live.size(), live.size(), a.stream, [&](size_t k) { return jr_round_bytes(a, o, files[live[k]], out_bytes[live[k]]); },
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) { return jpegr_decode_round(st, s, a, o, files.data(), out_bytes.data(), &live[r0], m, st_.data()); }, &done);
  for (size_t k = done; k < live.size(); ++k) st_[live[k]] = rc;   // the files of a failed round and of those behind it
  const int first = finish_statuses(st_, a.status);
  return rc != UHDR_HIP_NO_ERROR ? rc : first;
}

}  // namespace

extern "C" {

// uhdr_hip_jpeg_decode (YCBCR) or uhdr_hip_jpeg_decode_rgba (RGBA) for n files in one call: the headers are parsed by a few host
// threads, the files of a round share every decoder launch (jpeg::decode_device_batch) and one RGBA conversion launch
int uhdr_hip_jpeg_decode_batch(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out, const size_t* out_capacity,
                               uhdr_hip_image_t* descs, int* status, int mem_space, void* stream) {
  return uhdr_hip_jpeg_decode_batch_ex(n, jpeg, jpeg_size, decode_to, out, out_capacity, descs, status, mem_space, stream, 0);
}

// the same with flags: UHDR_HIP_DECODE_ANY_SAMPLING also reads 4:4:4, 4:2:2 and 4:4:0 files (descs[i].pixelFormat names the layout)
int uhdr_hip_jpeg_decode_batch_ex(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out, const size_t* out_capacity,
                                  uhdr_hip_image_t* descs, int* status, int mem_space, void* stream, int flags) {
  return uhdr_hip_jpeg_decode_batch_scaled(n, jpeg, jpeg_size, decode_to, out, out_capacity, descs, status, mem_space, stream, flags, 1);
}

// the same at 1 / scale_denom of every file's size (libjpeg's scale_num / scale_denom = 1 / 2, 1 / 4, 1 / 8): the reduced IDCTs of
// k_jd_idct_scaled_multi behind the shared entropy decode, the existing conversions on the scaled planes.  scale_denom 1: the call above
int uhdr_hip_jpeg_decode_batch_scaled(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out,
                                      const size_t* out_capacity, uhdr_hip_image_t* descs, int* status, int mem_space, void* stream, int flags,
                                      int scale_denom) {
  int rc = decode_gate(flags, scale_denom);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  const bool any_sampling = (flags & UHDR_HIP_DECODE_ANY_SAMPLING) != 0;
  if (n < 0 || (n > 0 && (jpeg == nullptr || jpeg_size == nullptr || descs == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  if ((rc = decode_to_gate(decode_to)) != UHDR_HIP_NO_ERROR) return rc;
  const bool rgba = decode_to == UHDR_HIP_DECODE_TO_RGBA;
  std::vector<jpeg::DecInfo> info((size_t)n);
  std::vector<size_t> need((size_t)n, 0);
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  on_host_threads(n, [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i) {
      void* o = out != nullptr ? out[i] : nullptr;
      const size_t cap = out != nullptr && out_capacity != nullptr ? out_capacity[i] : 0;
      try {
        st_[i] = jpeg_decode_host(jpeg[i], jpeg_size[i], rgba, any_sampling, o, cap, &descs[i], &info[i], &need[i], scale_denom);
      } catch (const std::bad_alloc&) {
        st_[i] = UHDR_HIP_UNKNOWN_ERROR;
      }
    }
  });
  std::vector<int> live;
  for (int i = 0; i < n; ++i)
    if (st_[i] == UHDR_HIP_NO_ERROR) live.push_back(i);
  if (live.empty()) return finish_statuses(st_, status);   // every file stopped at its checks or its size probe: the device is not touched
  const bool host_out = mem_space != UHDR_HIP_MEM_DEVICE;
  size_t done = 0;
  rc = run_rounds(
      live.size(), (size_t)kDecRound, stream, [&](size_t k) { return dec_round_bytes(info[live[k]], rgba, host_out, need[live[k]]); },
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        return jpeg_decode_round(st, s, rgba, host_out, jpeg, out, info.data(), need.data(), &live[r0], m, st_.data());
      },
      &done);
  for (size_t k = done; k < live.size(); ++k) st_[live[k]] = rc;   // the files of a failed round and of those behind it
  return finish_statuses(st_, status);
}

// JpegDecoderHelper::decompressImage(..., DECODE_TO_YCBCR) (jpegdecoderhelper.cpp:188-327) on the device: a batch of one file
int uhdr_hip_jpeg_decode(const void* jpeg, size_t jpeg_size, void* out, size_t out_capacity, uhdr_hip_image_t* desc,
                         int mem_space, void* stream) {
  if (jpeg == nullptr || desc == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return uhdr_hip_jpeg_decode_batch(1, &jpeg, &jpeg_size, UHDR_HIP_DECODE_TO_YCBCR, &out, &out_capacity, desc, nullptr, single_mem_space(mem_space), stream);
}

// JpegDecoderHelper::decompressImage(..., DECODE_TO_RGBA) (jpegdecoderhelper.cpp:251-281), a 4:2:0 JPEG -> RGBA8888: a batch of one file
int uhdr_hip_jpeg_decode_rgba(const void* jpeg, size_t jpeg_size, void* out, size_t out_capacity, uhdr_hip_image_t* desc, int mem_space, void* stream) {
  if (jpeg == nullptr || desc == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return uhdr_hip_jpeg_decode_batch(1, &jpeg, &jpeg_size, UHDR_HIP_DECODE_TO_RGBA, &out, &out_capacity, desc, nullptr, single_mem_space(mem_space), stream);
}

// host only: the synchronisation launches the last device decode of this host thread enqueued (jpeg::last_sync_counts)
int uhdr_hip_jpeg_decode_last_sync_launches(int* ring_looks, int* first_launches) {
  uint32_t launches = 0, looks = 0, first = 0;
  jpeg::last_sync_counts(&launches, &looks, &first);
  if (ring_looks != nullptr) *ring_looks = (int)looks;
  if (first_launches != nullptr) *first_launches = (int)first;
  return (int)launches;
}

// either single decode with flags (decode_to: UHDR_HIP_DECODE_TO_YCBCR / _RGBA): a batch of one file
int uhdr_hip_jpeg_decode_ex(const void* jpeg, size_t jpeg_size, int decode_to, void* out, size_t out_capacity, uhdr_hip_image_t* desc, int mem_space,
                            void* stream, int flags) {
  if (decode_gate(flags, 1) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (jpeg == nullptr || desc == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return uhdr_hip_jpeg_decode_batch_ex(1, &jpeg, &jpeg_size, decode_to, &out, &out_capacity, desc, nullptr, single_mem_space(mem_space), stream, flags);
}

int uhdr_hip_jpeg_decode_scaled(const void* jpeg, size_t jpeg_size, int decode_to, void* out, size_t out_capacity, uhdr_hip_image_t* desc, int mem_space,
                                void* stream, int flags, int scale_denom) {
  if (decode_gate(flags, scale_denom) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (jpeg == nullptr || desc == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return uhdr_hip_jpeg_decode_batch_scaled(1, &jpeg, &jpeg_size, decode_to, &out, &out_capacity, desc, nullptr, single_mem_space(mem_space), stream, flags,
                                           scale_denom);
}

// host only: what a decode at 1 / scale_denom of a width x height file with luma sampling hs x vs (gray: one plane) gives
int uhdr_hip_jpeg_scaled_geometry(int width, int height, int hs, int vs, int gray, int scale_denom, int* out_width, int* out_height, int* pixel_format,
                                  int idct_size[3]) {
  if (decode_gate(0, scale_denom) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (width <= 0 || height <= 0) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
  if (!gray && !((hs == 1 || hs == 2) && (vs == 1 || vs == 2))) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  jpeg::DecInfo info;
  info.w = width; info.h = height; info.hs = gray ? 1 : hs; info.vs = gray ? 1 : vs; info.gray = gray ? 1 : 0; info.scale = scale_denom;
  const DecGeom g = dec_geom(info);
  const jpeg::ScaledGeom sg = jpeg::scaled_geometry(width, height, info.hs, info.vs, gray != 0, scale_denom);
  if (out_width != nullptr) *out_width = (int)g.w;
  if (out_height != nullptr) *out_height = (int)g.h;
  if (pixel_format != nullptr) *pixel_format = g.fmt;
  if (idct_size != nullptr) { idct_size[0] = sg.idct[0]; idct_size[1] = gray ? 0 : sg.idct[1]; idct_size[2] = gray ? 0 : sg.idct[2]; }
  return UHDR_HIP_NO_ERROR;
}

// JpegR::decodeJPEGR for n files at once (jpegr_decode_files): all images of a call share every decoder launch (blockIdx.y = image)
int uhdr_hip_jpegr_decode_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests, uhdr_hip_metadata_t* metadata,
                                int* status, int apply_mode, int mem_space, void* stream) {
  return uhdr_hip_jpegr_decode_batch_ex(n, jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dests, metadata, status,
                                        apply_mode, mem_space, stream, 0);
}

int uhdr_hip_jpegr_decode_batch_ex(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                   void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests, uhdr_hip_metadata_t* metadata,
                                   int* status, int apply_mode, int mem_space, void* stream, int flags) {
  return jpegr_decode_files(JrBatch{n, jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dests, metadata, status, apply_mode, mem_space,
                                    stream, flags}, JrOpt{});
}

int uhdr_hip_jpegr_decode_rgbmap_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                       void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests, uhdr_hip_metadata_t* metadata,
                                       int* status, int apply_mode, int mem_space, void* stream, int flags) {
  return jpegr_decode_files(JrBatch{n, jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dests, metadata, status, apply_mode, mem_space,
                                    stream, flags}, JrOpt{true, false, 1});
}

int uhdr_hip_jpegr_decode_md_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                   void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests, uhdr_hip_metadata_t* metadata,
                                   int* status, int apply_mode, int mem_space, void* stream, int flags) {
  return uhdr_hip_jpegr_decode_scaled_batch(n, jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dests, metadata, status,
                                            apply_mode, mem_space, stream, flags, 1);
}

int uhdr_hip_jpegr_decode_scaled_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                       void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests, uhdr_hip_metadata_t* metadata,
                                       int* status, int apply_mode, int mem_space, void* stream, int flags, int scale_denom) {
  return jpegr_decode_files(JrBatch{n, jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dests, metadata, status, apply_mode, mem_space,
                                    stream, flags}, JrOpt{true, true, scale_denom});
}

int uhdr_hip_jpegr_decode(const void* jpegr, size_t jpegr_size, int output_format, float max_display_boost, void* dest_data,
                          size_t dest_capacity, uhdr_hip_image_t* dest, uhdr_hip_metadata_t* metadata, int apply_mode,
                          int mem_space, void* stream) {
  return uhdr_hip_jpegr_decode_ex(jpegr, jpegr_size, output_format, max_display_boost, dest_data, dest_capacity, dest, metadata, apply_mode,
                                  mem_space, stream, 0);
}

int uhdr_hip_jpegr_decode_ex(const void* jpegr, size_t jpegr_size, int output_format, float max_display_boost, void* dest_data,
                             size_t dest_capacity, uhdr_hip_image_t* dest, uhdr_hip_metadata_t* metadata, int apply_mode,
                             int mem_space, void* stream, int flags) {
  if (decode_gate(flags, 1) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (jpegr == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                   // :658-661
  if (dest == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                    // :662-665
  return uhdr_hip_jpegr_decode_batch_ex(1, &jpegr, &jpegr_size, output_format, max_display_boost, &dest_data, &dest_capacity, dest, metadata, nullptr,
                                        apply_mode, mem_space, stream, flags);
}

int uhdr_hip_jpegr_append_gainmap(const void* primary_jpeg, size_t primary_size, const void* gainmap_jpeg, size_t gainmap_size,
                                  const void* exif, size_t exif_size, const void* icc, size_t icc_size,
                                  const uhdr_hip_metadata_t* metadata, void* out, size_t out_capacity, size_t* out_size) {
  if (primary_jpeg == nullptr || gainmap_jpeg == nullptr || metadata == nullptr || out_size == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return jpegr::append_gainmap_to(static_cast<const uint8_t*>(primary_jpeg), primary_size, static_cast<const uint8_t*>(gainmap_jpeg), gainmap_size,
                                  static_cast<const uint8_t*>(exif), exif_size, static_cast<const uint8_t*>(icc), icc_size, *metadata,
                                  static_cast<uint8_t*>(out), out_capacity, out_size);
}

int uhdr_hip_icc_profile(int transfer_function, int color_gamut, void* out, size_t out_capacity, size_t* out_size) {
  if (out_size == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (transfer_function != UHDR_HIP_TF_SRGB) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;   // HLG / PQ profiles (tone-map LUTs) are not built
  std::vector<uint8_t> icc;
  if (!jpegr::icc_profile_srgb_transfer(color_gamut, icc)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  *out_size = icc.size();
  if (out == nullptr || out_capacity < icc.size()) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  memcpy(out, icc.data(), icc.size());
  return UHDR_HIP_NO_ERROR;
}

}  // extern "C"

namespace {

// JpegR::areInputArgumentsValid, the four-argument form (jpegr.cpp:75-173), checks in the reference's order
int check_encode_inputs(const uhdr_hip_image_t* p010, const uhdr_hip_image_t* yuv, int hdr_tf, const void* out, const size_t* out_size) {
  if (p010 == nullptr || p010->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if ((p010->width | p010->height) & 1) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
  if (p010->width < 8 || p010->height < 8 || p010->width > 8192 || p010->height > 8192) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
  if (p010->colorGamut <= UHDR_HIP_CG_UNSPECIFIED || p010->colorGamut > UHDR_HIP_CG_BT2100) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  if (p010->luma_stride != 0 && p010->luma_stride < p010->width) return UHDR_HIP_ERROR_INVALID_STRIDE;
  if (p010->chroma_data != nullptr && p010->chroma_stride < p010->width) return UHDR_HIP_ERROR_INVALID_STRIDE;
  if (out == nullptr || out_size == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (yuv == nullptr) return UHDR_HIP_NO_ERROR;
  if (yuv->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (yuv->luma_stride != 0 && yuv->luma_stride < yuv->width) return UHDR_HIP_ERROR_INVALID_STRIDE;
  if (yuv->chroma_data != nullptr && yuv->chroma_stride < yuv->width / 2) return UHDR_HIP_ERROR_INVALID_STRIDE;
  if (p010->width != yuv->width || p010->height != yuv->height) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  if (yuv->colorGamut <= UHDR_HIP_CG_UNSPECIFIED || yuv->colorGamut > UHDR_HIP_CG_BT2100) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  return UHDR_HIP_NO_ERROR;
}

// "clean up input structure for later usage" (jpegr.cpp:261-275 and the same lines of every API)
void default_p010(uhdr_hip_image_t* im) {
  if (im->luma_stride == 0) im->luma_stride = im->width;
  if (im->chroma_data == nullptr) { im->chroma_data = static_cast<uint16_t*>(im->data) + im->luma_stride * im->height; im->chroma_stride = im->luma_stride; }
  im->pixelFormat = UHDR_HIP_PIX_FMT_P010;
}
void default_yuv(uhdr_hip_image_t* im) {
  if (im->luma_stride == 0) im->luma_stride = im->width;
  if (im->chroma_data == nullptr) { im->chroma_data = static_cast<uint8_t*>(im->data) + im->luma_stride * im->height; im->chroma_stride = im->luma_stride >> 1; }
  im->pixelFormat = UHDR_HIP_PIX_FMT_YUV420;
}

// the 3x3 of JpegR::convertYuv for a pair of different encodings (jpegr.cpp:1134-1197)
const float* yuv_matrix(int src_encoding, int dest_encoding) {
  switch (src_encoding) {
    case UHDR_HIP_CG_BT709: return dest_encoding == UHDR_HIP_CG_P3 ? kYuv709To601 : kYuv709To2100;
    case UHDR_HIP_CG_P3: return dest_encoding == UHDR_HIP_CG_BT709 ? kYuv601To709 : kYuv601To2100;
    default: return dest_encoding == UHDR_HIP_CG_BT709 ? kYuv2100To709 : kYuv2100To601;
  }
}
// descriptor of one convertYuv: `src`'s samples through m into `dst`'s planes (the same image for the in-place form)
CvtImage cvt_image(const uhdr_hip_image_t& src, const uhdr_hip_image_t& dst, const float* m, bool* aligned) {
  CvtImage t;
  t.y = static_cast<uint8_t*>(dst.data);
  t.u = static_cast<uint8_t*>(dst.chroma_data);
  t.v = t.u + dst.chroma_stride * (dst.height / 2);
  t.y_stride = (uint32_t)dst.luma_stride; t.c_stride = (uint32_t)dst.chroma_stride;
  t.width = (uint32_t)dst.width; t.height = (uint32_t)dst.height;
  for (int i = 0; i < 9; ++i) t.m[i] = m[i];
  t.sy = static_cast<const uint8_t*>(src.data);
  t.su = static_cast<const uint8_t*>(src.chroma_data);
  t.sv = t.su + src.chroma_stride * (src.height / 2);
  t.sy_stride = (uint32_t)src.luma_stride; t.sc_stride = (uint32_t)src.chroma_stride;
  *aligned = t.width % 8u == 0 && al(t.y, 8) && t.y_stride % 8u == 0 && al(t.u, 4) && al(t.v, 4) && t.c_stride % 4u == 0 &&
             al(t.sy, 8) && t.sy_stride % 8u == 0 && al(t.su, 4) && al(t.sv, 4) && t.sc_stride % 4u == 0;
  return t;
}
// ---- encodeJPEGR for n files (uhdr_hip_jpegr_encode_batch) ---------------------------------------------------------------------
// Files go through in rounds of up to kEncRound (2 JPEGs each: the batched encoder's job limit); every device buffer of a round is
// a slice of one grow-only pool slot of the leased context, the compressed streams land in its page-locked host pool.
constexpr int kEncRound = jpeg::kMaxBatchJobs / 2;

struct EncFile {
  int idx = 0;                 // the caller's index
  uhdr_hip_image_t p010, yuv;  // defaulted (yuv: API-1 only); device planes once staged
  uhdr_hip_image_t enc, map;   // the planes the two JPEGs compress (device)
  size_t pad_ls = 0, pad_cs = 0;   // the strides that decide the encoder's column padding (the caller's for a P3 image)
  bool own_copy = false;       // enc is a private zero-padded copy with 16-aligned strides
  float peak = 0.0f;           // tone-mapped API-0: the caller's hdr_peak_nits (0: the headroom is measured)
  std::vector<uint8_t> icc;
};

// compressGainMap (jpegr.cpp:806-821): one plane at kMapCompressQuality = 85
EncJpeg gainmap_jpeg(uhdr_hip_image_t map, size_t pad_ls) {
  map.chroma_data = nullptr; map.chroma_stride = 0; map.pixelFormat = UHDR_HIP_PIX_FMT_MONOCHROME;
  return EncJpeg{map, 85, nullptr, pad_ls, 0};
}
// the per-channel map (RGBA pixels) at the same quality, as a 4:4:4 file
EncJpeg gainmap_rgb_jpeg(uhdr_hip_image_t map) {
  map.chroma_data = nullptr; map.chroma_stride = 0; map.pixelFormat = UHDR_HIP_PIX_FMT_RGBA8888;
  EncJpeg e{map, 85, nullptr, 0, 0};
  e.rgb = true;
  return e;
}

// what a JPEG/R encode batch says beyond its files, each entry point naming what it sets (encode_files, encode_packed_files)
struct JpegrOpt {
  int boost_scope = -1;                               // >= 0: the adaptive generate (UHDR_HIP_BOOST_*)
  uhdr_hip_metadata_t* metadata = nullptr;            // or one entry per file: what every processed file's container carries
  int tonemap_op = UHDR_HIP_TONEMAP_SHIFT;            // API-0 from planes: the operator that derives the SDR image
  const float* peaks = nullptr;                       // or hdr_peak_nits, one per file (tone-mapped API-0, packed API-0)
  bool rgb_map = false;                               // the per-channel map, compressed as a 4:4:4 file
  int map_scale = 4;                                  // the map's factor (planes)
  int primary_sampling = UHDR_HIP_PIX_FMT_YUV420;     // the primary image's sampling (packed)
  EncOpt enc;                                         // the encoder's options, for both compressions
};

// the call-level gate of the JPEG/R encode batches: the arrays every form needs (hdr_images, and sdr_images where the form has no
// API-0 reading: `need_sdr`), exif without its sizes, then the quality (jpegr.cpp:175-183)
int jpegr_batch_gate(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, bool need_sdr, int quality,
                     const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity, const size_t* out_size) {
  if (n < 0 || (n > 0 && (hdr_images == nullptr || (need_sdr && sdr_images == nullptr) || out == nullptr || out_capacity == nullptr ||
                          out_size == nullptr)) ||
      (exif != nullptr && exif_size == nullptr))
    return UHDR_HIP_ERROR_BAD_PTR;
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;
  return UHDR_HIP_NO_ERROR;
}

// UHDR_HIP_BOOST_PER_CALL over several rounds: the statistic of all rounds first.  The carry slot of the context is reserved and
// initialised, then round(st, s, f, m, 1) stages and measures every kEncRound-sized slice of the files -- probe copies, since a round
// rewrites its files' descriptors -- with the pooled extremes carried along in device memory; the rounds proper then encode against
// the carried pair (carry == 2).
template <class File, class Round>
int measure_all_rounds(DeviceState* st, hipStream_t s, const std::vector<File>& files, Round round) {
  int rc = pool_reserve(st, kEncAdaptCarry, 256);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  const hipError_t e = launch_adaptive_init(static_cast<uint32_t*>(st->pool[kEncAdaptCarry]), 2u, s);
  if (e != hipSuccess) { set_err("launch_adaptive_init", e); return UHDR_HIP_UNKNOWN_ERROR; }
  for (size_t q0 = 0; rc == UHDR_HIP_NO_ERROR && q0 < files.size(); q0 += kEncRound) {
    const int m = (int)std::min(files.size() - q0, (size_t)kEncRound);
    std::vector<File> probe(files.begin() + (long)q0, files.begin() + (long)q0 + m);
    rc = round(st, s, probe.data(), m, 1);
  }
  return rc;
}

// appendGainMap (jpegr.cpp:951-1130) for the m files of a round, straight into the caller's buffers, a few host threads side by
// side: file k's JPEGs are jpg[2 k] (SDR) and jpg[2 k + 1] (gain map), idx(k) its place in the caller's arrays.  range == NULL: every
// container carries md; else (adaptive) file k's own, from range[2 k] and range[2 k + 1].  metadata (or NULL) receives each file's.
template <class Idx>
void append_containers(int m, const EncJpeg* jpg, Idx idx, const uhdr_hip_metadata_t& md, const float* range, const void* const* exif,
                       const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* st_,
                       uhdr_hip_metadata_t* metadata) {
  on_host_threads(m, [&](int lo, int hi) {
    for (int k = lo; k < hi; ++k) {
      const int i = idx(k);
      const EncJpeg& sdr = jpg[2 * (size_t)k];
      const EncJpeg& gm = jpg[2 * (size_t)k + 1];
      uhdr_hip_metadata_t mk = md;
      if (range != nullptr) fill_adaptive_metadata(range[2 * (size_t)k], range[2 * (size_t)k + 1], &mk);
      if (sdr.clen_overflow || gm.clen_overflow) { st_[i] = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; continue; }   // (a progressive file)
      st_[i] =jpegr::append_gainmap_to(sdr.bytes, sdr.n, gm.bytes, gm.n, static_cast<const uint8_t*>(exif ? exif[i] : nullptr), exif ? exif_size[i] : 0,
                                        nullptr, 0, mk, static_cast<uint8_t*>(out[i]), out_capacity[i], &out_size[i], range != nullptr);
      if (metadata != nullptr) metadata[i] = mk;
    }
  });
}

// One round: staging (host callers), toneMap (API-0), generateGainMap, BT.601 re-encode -- one launch per step for the round's
// files -- then the 2 m compressions with one synchronisation (compress_to_host).  Leaves file k's JPEGs in (*jpg)[2 k] (SDR) and
// (*jpg)[2 k + 1] (gain map).  A non-zero return is an error of the device or the runtime (every file of the round fails with it).
// boost_scope >= 0: the adaptive generate instead; range (2 m floats) receives the files' (lo, hi) behind the round's synchronisation.
// carry != 0 (PER_CALL over several rounds): the rounds' pooled extremes travel in the context's carry slot; carry == 1 measures
// only -- staging, toneMap and pass 1, no map, no compression, no synchronisation --, carry == 2 encodes against the carried pair.
// tonemap_op (API-0): the operator that derives the SDR planes; its headroom array is a pool slot of the context.
int encode_round(DeviceState* st, hipStream_t s, bool api0, bool host, int hdr_tf, int quality, EncFile* f, int m, uhdr_hip_metadata_t* md,
                 std::vector<EncJpeg>* jpg, const JpegrOpt& opt, float* range = nullptr, int carry = 0) {
  const int boost_scope = opt.boost_scope, tonemap_op = opt.tonemap_op, map_scale = opt.map_scale;
  const bool rgb_map = opt.rgb_map;
  const EncOpt& eo = opt.enc;
  const size_t msf = (size_t)map_scale;     // the map's factor: uhdr_hip_jpegr_encode_scaled_batch's, 4 in every other call
  const size_t map_bpp = rgb_map ? 4 : 1;   // rgb_map: uhdr_hip_generate_gainmap_rgb_batch's RGBA map, compressed as 4:4:4
  auto al256 = [](size_t v) { return (v + 255) / 256 * 256; };
  int rc;
  // sizes of the round's slices
  size_t sdr_total = 0, map_total = 0, p010_total = 0, yuv_total = 0;
  for (int k = 0; k < m; ++k) {
    const size_t w = f[k].p010.width, h = f[k].p010.height, aw = (w + 15) / 16 * 16, mw = w / msf, mh = h / msf;
    if (host) {
      p010_total += al256(round_up(w, 64) * h * 2) + al256(round_up(w, 64) * (h / 2) * 2);
      if (!api0) yuv_total += al256(round_up(aw, 64) * h) + al256(round_up(aw, 64) * h);
    }
    if (f[k].own_copy) sdr_total += al256(aw * h * 3 / 2 + 64);
    map_total += al256(mw * mh * map_bpp + 64);
  }
  if ((rc = pool_reserve(st, kEncMap, map_total)) != 0) return rc;
  if (sdr_total && (rc = pool_reserve(st, kEncSdr, sdr_total)) != 0) return rc;
  if (p010_total && (rc = pool_reserve(st, kEncP010, p010_total)) != 0) return rc;
  if (yuv_total && (rc = pool_reserve(st, kEncYuv, yuv_total)) != 0) return rc;
  const bool tone_sdr = api0 && tonemap_op != UHDR_HIP_TONEMAP_SHIFT;
  if (tone_sdr && (rc = pool_reserve(st, kEncToneHead, round_up(sizeof(float) * (size_t)m, 256))) != 0) return rc;

  // planes: staged inputs (host callers), private copies, maps
  size_t o_p010 = 0, o_yuv = 0, o_sdr = 0, o_map = 0;
  for (int k = 0; k < m; ++k) {
    EncFile& e = f[k];
    const size_t w = e.p010.width, h = e.p010.height, aw = (w + 15) / 16 * 16, acw = (w / 2 + 7) / 8 * 8;
    if (host) {   // the same bytes the single calls stage
      uint8_t* d = static_cast<uint8_t*>(st->pool[kEncP010]) + o_p010;
      const size_t lp = round_up(w, 64), cp = round_up(w, 64);
      if ((rc = h2d_plane(d, lp, e.p010.data, e.p010.luma_stride, w, h, 2, s)) != 0) return rc;
      uint8_t* dc = d + al256(lp * h * 2);
      if ((rc = h2d_plane(dc, cp, e.p010.chroma_data, e.p010.chroma_stride, w, h / 2, 2, s)) != 0) return rc;
      o_p010 += al256(lp * h * 2) + al256(cp * (h / 2) * 2);
      e.p010.data = d; e.p010.chroma_data = dc; e.p010.luma_stride = lp; e.p010.chroma_stride = cp;
      if (!api0) {
        const size_t ls = e.yuv.luma_stride, cs = e.yuv.chroma_stride;
        const size_t ycols = ls < aw ? w : aw, ccols = cs < acw ? w / 2 : acw, dls = round_up(ycols, 64), dcs = round_up(ccols, 64);
        uint8_t* y = static_cast<uint8_t*>(st->pool[kEncYuv]) + o_yuv;
        uint8_t* u = y + al256(dls * h);
        const uint8_t* hu = static_cast<const uint8_t*>(e.yuv.chroma_data);
        if ((rc = h2d_plane(y, dls, e.yuv.data, ls, ycols, h, 1, s)) != 0) return rc;
        if ((rc = h2d_plane(u, dcs, hu, cs, ccols, h / 2, 1, s)) != 0) return rc;
        if ((rc = h2d_plane(u + dcs * (h / 2), dcs, hu + cs * (h / 2), cs, ccols, h / 2, 1, s)) != 0) return rc;
        o_yuv += al256(round_up(aw, 64) * h) + al256(round_up(aw, 64) * h);
        e.yuv.data = y; e.yuv.chroma_data = u; e.yuv.luma_stride = dls; e.yuv.chroma_stride = dcs;
      }
    }
    if (e.own_copy) {   // 16-aligned strides, zero padded (a width of whole 16-column batches has no padding: the kernels write it all)
      uint8_t* d = static_cast<uint8_t*>(st->pool[kEncSdr]) + o_sdr;
      o_sdr += al256(aw * h * 3 / 2 + 64);
      if (aw != w) HIP_TRY(hipMemsetAsync(d, 0, aw * h * 3 / 2, s));
      memset(&e.enc, 0, sizeof(e.enc));
      e.enc.data = d; e.enc.chroma_data = d + aw * h; e.enc.width = w; e.enc.height = h;
      e.enc.luma_stride = aw; e.enc.chroma_stride = aw >> 1; e.enc.pixelFormat = UHDR_HIP_PIX_FMT_YUV420;
      e.enc.colorGamut = api0 ? e.p010.colorGamut : e.yuv.colorGamut;
      e.pad_ls = aw; e.pad_cs = aw >> 1;
    } else {
      e.enc = e.yuv;   // P3: compressed as it is, padded by the caller's strides
    }
    if (api0) e.yuv = e.enc;
    e.map = e.yuv;
    e.map.data = static_cast<uint8_t*>(st->pool[kEncMap]) + o_map;
    o_map += al256((w / msf) * (h / msf) * map_bpp + 64);
  }
  std::vector<uhdr_hip_image_t> a((size_t)m), b((size_t)m), c((size_t)m);
  if (api0) {   // :208-226
    for (int k = 0; k < m; ++k) { a[k] = f[k].p010; b[k] = f[k].enc; }
    if (tone_sdr) {
      std::vector<float> peaks((size_t)m);
      for (int k = 0; k < m; ++k) peaks[(size_t)k] = f[k].peak;
      rc = uhdr_hip_tonemap_sdr_batch(m, a.data(), b.data(), hdr_tf, tonemap_op, peaks.data(), static_cast<float*>(st->pool[kEncToneHead]), s);
    } else {
      rc = uhdr_hip_tonemap_batch(m, a.data(), b.data(), s);
    }
    if (rc != UHDR_HIP_NO_ERROR) return rc;
  }
  // generateGainMap: the files are sorted by size and gamuts, so equal ones share its launches
  for (int k = 0; k < m; ++k) { a[k] = f[k].yuv; b[k] = f[k].p010; c[k] = f[k].map; }
  float* dev_range = nullptr;
  if (map_scale != 4) {   // (never with an adaptive range)
    if ((rc = uhdr_hip_generate_gainmap_scaled_batch(m, a.data(), b.data(), hdr_tf, nullptr, md, c.data(), 0, rgb_map ? 1 : 0, map_scale, s)) != UHDR_HIP_NO_ERROR)
      return rc;
  } else if (rgb_map) {
    if ((rc = uhdr_hip_generate_gainmap_rgb_batch(m, a.data(), b.data(), hdr_tf, md, c.data(), 0, s)) != UHDR_HIP_NO_ERROR) return rc;
  } else if (boost_scope < 0) {
    if ((rc = uhdr_hip_generate_gainmap_batch(m, a.data(), b.data(), hdr_tf, md, c.data(), 0, nullptr, s)) != UHDR_HIP_NO_ERROR) return rc;
  } else {
    const size_t ws_bytes = adaptive_layout(m, a.data()).total;
    if ((rc = pool_reserve(st, kEncAdaptWs, ws_bytes + 256 + round_up(8 * (size_t)m, 256))) != 0) return rc;
    uint8_t* ws = static_cast<uint8_t*>(st->pool[kEncAdaptWs]);
    dev_range = reinterpret_cast<float*>(ws + ws_bytes + 256);
    uint32_t* cw = carry != 0 ? static_cast<uint32_t*>(st->pool[kEncAdaptCarry]) : nullptr;
    if ((rc = adaptive_enqueue(m, a.data(), b.data(), hdr_tf, c.data(), 0, boost_scope, nullptr, dev_range, ws, cw, carry == 1 ? cw : nullptr,
                               carry != 1, s)) != UHDR_HIP_NO_ERROR)
      return rc;
    if (carry == 1) return UHDR_HIP_NO_ERROR;
  }
  // convertYuv to BT.601 unless P3: API-0 in place, API-1 into the private copy; equal sizes and gamuts share a launch
  for (int k = 0; k < m;) {
    if (f[k].enc.colorGamut == UHDR_HIP_CG_P3) { ++k; continue; }
    CvtBatch cb;
    const uhdr_hip_image_t& e0 = f[k].enc;
    const Chunk ch = form_chunk(k, m, kToneChunk,
                                [&](int j) { return f[j].enc.colorGamut == e0.colorGamut && f[j].enc.width == e0.width && f[j].enc.height == e0.height; },
                                [&](int j, int slot) {
                                  bool aligned;
                                  cb.img[slot] = cvt_image(api0 ? f[j].enc : f[j].yuv, f[j].enc, yuv_matrix(e0.colorGamut, UHDR_HIP_CG_P3), &aligned);
                                  return aligned;
                                });
    HIP_TRY(launch_convert_yuv(cb, ch.m, ch.cls, s));
    k += ch.m;
  }
  // the 2 m compressions
  jpg->clear();
  jpg->reserve(2 * (size_t)m);
  for (int k = 0; k < m; ++k) {
    const EncFile& e = f[k];
    uhdr_hip_image_t g = e.map;
    g.width = e.enc.width / msf; g.height = e.enc.height / msf; g.luma_stride = g.width;
    jpg->push_back(EncJpeg{e.enc, quality, &e.icc, e.pad_ls, e.pad_cs});
    jpg->push_back(rgb_map ? gainmap_rgb_jpeg(g) : gainmap_jpeg(g, g.luma_stride));
  }
  for (EncJpeg& e : *jpg) eo.to(&e);   // the primary image and the gain map alike (intervals in rows: each from its own width)
  return compress_to_host(st, s, 2 * m, jpg->data(), true, EncExtra{dev_range, dev_range ? 8 * (size_t)m : 0, range});
}

// encodeJPEGR API-1 (yuv420_images != NULL) or API-0 for n pairs, the quality checked: the files' kernels share their launches, the
// call synchronises once per round of up to kEncRound files, and the containers are assembled by a few host threads
int encode_files(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                 const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                 int* status, int mem_space, void* stream, const JpegrOpt& opt = JpegrOpt()) {
  const int boost_scope = opt.boost_scope, tonemap_op = opt.tonemap_op, map_scale = opt.map_scale;
  const float* hdr_peak_nits = opt.peaks;
  const EncOpt& eo = opt.enc;
  const bool api0 = yuv420_images == nullptr;
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  std::vector<EncFile> files;
  for (int i = 0; i < n; ++i) {   // the single call's checks, in its order; a file that fails them is not processed
    const void* ex = exif ? exif[i] : nullptr;
    const size_t exn = exif ? exif_size[i] : 0;
    int rc = check_encode_inputs(p010_images + i, api0 ? nullptr : yuv420_images + i, hdr_tf, out[i], out_size + i);
    if (rc == UHDR_HIP_NO_ERROR && ex == nullptr && exn != 0) rc = UHDR_HIP_ERROR_BAD_PTR;                     // :190-193 / :258-261
    const float peak = tonemap_op != UHDR_HIP_TONEMAP_SHIFT && hdr_peak_nits ? hdr_peak_nits[i] : 0.0f;
    if (rc == UHDR_HIP_NO_ERROR && !valid_peak_nits(peak)) rc = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    // a factor of the call's own: every reader refuses a map whose size does not divide the image's (validate_apply)
    if (rc == UHDR_HIP_NO_ERROR && map_scale != 4 &&
        (p010_images[i].width % (size_t)map_scale != 0 || p010_images[i].height % (size_t)map_scale != 0))
      rc = UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
    if (rc == UHDR_HIP_NO_ERROR && !encodable_with(p010_images[i].width, p010_images[i].height, jpeg::kGeom420, eo))
      rc = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (rc != UHDR_HIP_NO_ERROR) { st_[i] = rc; continue; }
    EncFile e;
    e.idx = i;
    e.peak = peak;
    e.p010 = p010_images[i];
    default_p010(&e.p010);
    memset(&e.yuv, 0, sizeof(e.yuv));
    if (!api0) { e.yuv = yuv420_images[i]; default_yuv(&e.yuv); }
    e.pad_ls = e.yuv.luma_stride; e.pad_cs = e.yuv.chroma_stride;
    const int sdr_gamut = api0 ? e.p010.colorGamut : e.yuv.colorGamut;
    e.own_copy = api0 || sdr_gamut != UHDR_HIP_CG_P3;
    if (!jpegr::icc_profile_srgb_transfer(sdr_gamut, e.icc)) { st_[i] = UHDR_HIP_ERROR_INVALID_COLORGAMUT; continue; }
    files.push_back(std::move(e));
  }
  if (files.empty()) return finish_statuses(st_, status);
  // runs of equal size and gamuts, whatever the caller's order: equal files share the launches of toneMap, generate and convertYuv
  auto key = [&](const EncFile& e) {
    return std::make_tuple(e.p010.width, e.p010.height, api0 ? e.p010.colorGamut : e.yuv.colorGamut, e.p010.colorGamut);
  };
  std::stable_sort(files.begin(), files.end(), [&](const EncFile& x, const EncFile& y) { return key(x) < key(y); });
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  // PER_CALL over several rounds: the statistic of all rounds first (every round staged and measured, the pooled extremes carried
  // along in device memory), then the rounds proper, encoded against the carried pair
  const int carry = boost_scope == UHDR_HIP_BOOST_PER_CALL && files.size() > (size_t)kEncRound ? 2 : 0;
  std::vector<float> range(2 * (size_t)kEncRound);
  // the measuring pass (pass == 1) stops behind the statistic: it takes the scope and the operator alone, and no range comes down
  JpegrOpt measure_opt;
  measure_opt.boost_scope = boost_scope;
  measure_opt.tonemap_op = tonemap_op;
  auto round = [&](DeviceState* st, hipStream_t s, EncFile* f, int m, int pass) -> int {
    uhdr_hip_metadata_t md{};
    std::vector<EncJpeg> jpg;
    const int rc = encode_round(st, s, api0, host, hdr_tf, quality, f, m, &md, &jpg, pass == 1 ? measure_opt : opt,
                                pass == 1 ? nullptr : range.data(), pass);
    if (rc != UHDR_HIP_NO_ERROR || pass == 1) return rc;
    append_containers(m, jpg.data(), [f](int k) { return f[k].idx; }, md, boost_scope >= 0 ? range.data() : nullptr, exif, exif_size, out,
                      out_capacity, out_size, st_.data(), opt.metadata);
    return UHDR_HIP_NO_ERROR;
  };
  size_t done = 0;
  const int rc = run_rounds(
      files.size(), (size_t)kEncRound, stream, [](size_t) { return (size_t)0; },   // rounds by count alone
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        // the measuring pass needs the leased context, which the driver hands over with a round: it goes in front of the first one
        const int rc = carry != 0 && r0 == 0 ? measure_all_rounds(st, s, files, round) : (int)UHDR_HIP_NO_ERROR;
        return rc != UHDR_HIP_NO_ERROR ? rc : round(st, s, &files[r0], m, carry);
      },
      &done);
  for (size_t k = done; k < files.size(); ++k) st_[files[k].idx] = rc;   // the files of the failed round and of those behind it
  return finish_statuses(st_, status);
}

// ---- the host-side checks of API-2, API-3, API-4 and API-x, shared by the single calls and the batches ----------------------------
// API-4's checks on the SDR JPEG (jpegr.cpp:520-541), which API-2 and API-3 make as well: *icc receives the ICC profile the container
// adds to a JPEG that carries none
int sdr_jpeg_check(const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut, std::vector<uint8_t>* icc) {
  const uint8_t* pj = static_cast<const uint8_t*>(sdr_jpeg);
  if (!jpegr::has_valid_header(pj, sdr_jpeg_size)) return UHDR_HIP_ERROR_DECODE_ERROR;                            // :520-524
  const uint8_t* have = nullptr;
  size_t have_len = 0;
  icc->clear();
  if (!jpegr::first_icc(pj, sdr_jpeg_size, &have, &have_len)) {          // :527-541
    if (sdr_jpeg_gamut <= UHDR_HIP_CG_UNSPECIFIED || sdr_jpeg_gamut > UHDR_HIP_CG_BT2100) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    jpegr::icc_profile_srgb_transfer(sdr_jpeg_gamut, *icc);
  }
  return UHDR_HIP_NO_ERROR;
}

// API-2's checks before its device work (jpegr.cpp:390-397, then areInputArgumentsValid)
int api2_check(const uhdr_hip_image_t* p010, const uhdr_hip_image_t* yuv, const void* sdr_jpeg, int hdr_tf, const void* out, const size_t* out_size) {
  if (yuv == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                              // :390-393
  if (sdr_jpeg == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                         // :394-397
  return check_encode_inputs(p010, yuv, hdr_tf, out, out_size);
}

// API-3's checks before its device decode (jpegr.cpp:443-462): uhdr_hip_jpeg_decode's size probe on the SDR JPEG, host work, its
// header into *info
int api3_check(const uhdr_hip_image_t* p010, const void* sdr_jpeg, size_t sdr_jpeg_size, int hdr_tf, const void* out, const size_t* out_size,
               jpeg::DecInfo* info) {
  if (sdr_jpeg == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                         // :443-446
  int rc = check_encode_inputs(p010, nullptr, hdr_tf, out, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  uhdr_hip_image_t desc;
  size_t need = 0;
  try {
    rc = jpeg_decode_host(sdr_jpeg, sdr_jpeg_size, false, false, nullptr, 0, &desc, info, &need);
  } catch (const std::bad_alloc&) {
    rc = UHDR_HIP_UNKNOWN_ERROR;
  }
  if (rc == UHDR_HIP_ERROR_UNSUPPORTED_FEATURE) return rc;
  if (rc != UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE || desc.pixelFormat != UHDR_HIP_PIX_FMT_YUV420 || desc.width == 0 || desc.height == 0)
    return UHDR_HIP_ERROR_DECODE_ERROR;
  return UHDR_HIP_NO_ERROR;
}

// API-3's checks after its decode of a w x h JPEG (jpegr.cpp:467-499): the SDR gamut into *gamut -- the ICC profile's when there is
// one (it must agree with a configured gamut), else the configured one -- then the P010 size against the JPEG's
int api3_check_decoded(const uhdr_hip_image_t& p010, const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut, size_t w, size_t h,
                       int* gamut) {
  const uint8_t* icc = nullptr;
  size_t icc_len = 0;
  if (jpegr::first_icc(static_cast<const uint8_t*>(sdr_jpeg), sdr_jpeg_size, &icc, &icc_len)) {
    const int cg = jpegr::gamut_from_icc(icc, icc_len);
    if (cg == UHDR_HIP_CG_UNSPECIFIED || (sdr_jpeg_gamut != UHDR_HIP_CG_UNSPECIFIED && sdr_jpeg_gamut != cg)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    *gamut = cg;
  } else {
    if (sdr_jpeg_gamut <= UHDR_HIP_CG_UNSPECIFIED || sdr_jpeg_gamut > UHDR_HIP_CG_BT2100) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    *gamut = sdr_jpeg_gamut;
  }
  if (p010.width != w || p010.height != h) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;                             // :496-499
  return UHDR_HIP_NO_ERROR;
}

// API-x's checks after its NULL pointers (jpegr.cpp:590-611): *yuv and *map come back as they are compressed (strides and chroma
// defaulted, the map a single plane), *icc holds the SDR image's ICC profile
int apix_check(const uhdr_hip_image_t& yuv_in, const uhdr_hip_image_t& gainmap, uhdr_hip_image_t* yuv, uhdr_hip_image_t* map,
               std::vector<uint8_t>* icc) {
  *yuv = yuv_in;
  default_yuv(yuv);
  uhdr_hip_image_t g = gainmap;
  if (g.luma_stride == 0) g.luma_stride = g.width;
  *map = gainmap_jpeg(g, g.luma_stride).img;
  if (!encodable(*map)) return UHDR_HIP_ERROR_ENCODE_ERROR;                                                       // :590-597
  if (!jpegr::icc_profile_srgb_transfer(yuv->colorGamut, *icc)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;          // :599-600
  if (!encodable(*yuv)) return UHDR_HIP_ERROR_ENCODE_ERROR;                                                       // :602-611
  return UHDR_HIP_NO_ERROR;
}

// uhdr_hip_jpegr_encode_batch behind its three forms: API-1 (yuv420_images != NULL) or API-0, the encoder's options said
int jpegr_encode_batch_with(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                            const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                            int* status, const EncOpt& eo, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, p010_images, yuv420_images, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  JpegrOpt opt;
  opt.enc = eo;
  return encode_files(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

}  // namespace

extern "C" {

int uhdr_hip_jpegr_encode_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                                int* status, int mem_space, void* stream) {
  return jpegr_encode_batch_with(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, EncOpt(),
                                 mem_space, stream);
}
// flags == 0 is uhdr_hip_jpegr_encode_batch.  UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN: the primary image and the gain-map JPEG of every file
// with Huffman tables of their own; XMP, MPF offsets and ICC follow from the new sizes through the same container writer
int uhdr_hip_jpegr_encode_batch_ex(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                   const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                   size_t* out_size, int* status, int flags, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_flags(flags, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpegr_encode_batch_with(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, eo, mem_space,
                                 stream);
}
// opts == NULL, or no restart field set: uhdr_hip_jpegr_encode_batch_ex with opts->flags.  Otherwise the primary image and the gain-map
// JPEG of every file with restart intervals, restart_in_rows counting each one's own MCU rows
int uhdr_hip_jpegr_encode_batch_opts(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                     const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                     size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpegr_encode_batch_with(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, eo, mem_space,
                                 stream);
}

// the same with the scan mode said: the primary image and the gain-map JPEG of every file are both written in it
int uhdr_hip_jpegr_encode_batch_scans(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                      const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                      size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space,
                                      void* stream) {
  EncOpt eo;
  const int rc = encode_scans(opts, scan_mode, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return jpegr_encode_batch_with(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, eo, mem_space,
                                 stream);
}

// the interval rule on its own, host only: what compress_to_host derives for a scan of this width (enc_restart)
int uhdr_hip_jpeg_restart_mcus(const uhdr_hip_jpeg_encode_opts_t* opts, size_t width, int mcu_width, uint32_t* restart_mcus) {
  EncOpt eo;
  const int rc = encode_opts(opts, &eo);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (restart_mcus == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if ((mcu_width != 8 && mcu_width != 16) || width == 0 || width > 65535) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  *restart_mcus = jpeg::restart_mcus(eo.restart_interval, eo.restart_in_rows, (uint32_t)((width + (size_t)mcu_width - 1) / (size_t)mcu_width));
  return UHDR_HIP_NO_ERROR;
}

// jpeg_gen_optimal_table of a caller's histogram by the encoder's table kernel: what an image's symbol
// counts would have to be is the caller's to say, so table shapes no small image produces can be reached
int uhdr_hip_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256], int* nvals, void* stream) {
  if (freq == nullptr || bits == nullptr || vals == nullptr || nvals == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  bool any = false;
  for (int i = 0; i < 256; ++i) {
    if (freq[i] >= jpeg::kHuffFreqLimit) return UHDR_HIP_ERROR_BAD_PTR;
    any = any || freq[i] != 0;
  }
  if (!any) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CodecLease lease(st);
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if ((rc = pool_reserve(st, kEncWs, 2048)) != 0) return rc;
  uint8_t* d = static_cast<uint8_t*>(st->pool[kEncWs]);   // [0, 1024) counts, [1024, 1040) BITS, [1040, 1296) HUFFVAL, [1296, 1300) their number
  HIP_TRY(hipMemcpyAsync(d, freq, 1024, hipMemcpyHostToDevice, s));
  HIP_TRY(jpeg::optimal_table_async(reinterpret_cast<const uint32_t*>(d), d + 1024, d + 1040, reinterpret_cast<int*>(d + 1296), s));
  uint8_t h[276];
  HIP_TRY(hipMemcpyAsync(h, d + 1024, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int n = 0;
  memcpy(&n, h + 272, 4);
  if (n < 0) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;   // a code longer than 32 bits: libjpeg gives up there
  memcpy(bits, h, 16);
  memcpy(vals, h + 16, (size_t)n);
  *nvals = n;
  return UHDR_HIP_NO_ERROR;
}

// the same with the per-channel map of uhdr_hip_generate_gainmap_rgb_batch, compressed at quality 85 as a 4:4:4 file; primary image,
// metadata and container are uhdr_hip_jpegr_encode_batch's
int uhdr_hip_jpegr_encode_rgbmap_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                       const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                       size_t* out_size, int* status, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, p010_images, yuv420_images, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  JpegrOpt opt;
  opt.rgb_map = true;
  return encode_files(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

// uhdr_hip_jpegr_encode_batch / _rgbmap_batch with the gain map at the call's factor; factor 4 IS those calls
int uhdr_hip_jpegr_encode_scaled_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                       const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                       size_t* out_size, int* status, int rgb_map, int map_scale_factor, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, p010_images, yuv420_images, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (map_scale_factor < 1 || map_scale_factor > 128) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
  JpegrOpt opt;
  opt.rgb_map = rgb_map != 0;
  opt.map_scale = map_scale_factor;
  return encode_files(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

// JPEG/R files from packed RGBA pairs: API-1's checks where they apply, then those of
// uhdr_hip_generate_gainmap_packed_batch; per round one generate call (equal files share its launches), one k_rgba_to_ycc420 launch
// for the primaries and the 2 m compressions behind one synchronisation, as in encode_files
// sdr_images == NULL: the packed API-0 -- the SDR side of the checks falls away, a file's SDR image is
// uhdr_hip_tonemap_packed_batch's in a pool slot of the round's context (peaks: one per file, or NULL), in the HDR image's gamut;
// metadata (or NULL) receives what every processed file's container carries
// boost_scope >= 0: the adaptive generate in the generate step's place, as in encode_round -- the workspace and
// the carried key pair are the same pool slots, a round's ranges come down with its streams, and PER_CALL over several rounds stages
// and measures every round (carry == 1) in front of the first one
// primary_sampling, enc (uhdr_hip_jpegr_encode_packed_sampling_batch): the primary image as uhdr_hip_jpeg_encode_rgba_batch_opts writes it
// at that sampling -- YUV444 straight from the pixels, YUV422 through k_rgba_to_ycc422 --, enc for both compressions
static int encode_packed_files(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf, int quality,
                               const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                               size_t* out_size, int* status, int mem_space, void* stream, const JpegrOpt& opt) {
  const int boost_scope = opt.boost_scope, primary_sampling = opt.primary_sampling;
  const bool rgb_map = opt.rgb_map;
  const float* peaks = opt.peaks;
  const EncOpt& eo = opt.enc;
  const bool api0 = sdr_images == nullptr;
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  auto stride_bad = [](const uhdr_hip_image_t& im) { return im.luma_stride != 0 && (im.luma_stride < im.width || im.luma_stride > 0xFFFFFFFFull); };
  auto check = [&](const uhdr_hip_image_t& hd, const uhdr_hip_image_t& sd, int i) -> int {
    if (hd.data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
    if ((hd.width | hd.height) & 1) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
    if (hd.width < 8 || hd.height < 8 || hd.width > 8192 || hd.height > 8192) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
    if (!valid_gamut(hd.colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    if (stride_bad(hd)) return UHDR_HIP_ERROR_INVALID_STRIDE;
    if (out[i] == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
    if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
    if (!api0) {
      if (sd.data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
      if (stride_bad(sd)) return UHDR_HIP_ERROR_INVALID_STRIDE;
      // (the 4:4:4 encoder addresses the pixels' rows with an int byte pitch)
      if (primary_sampling == UHDR_HIP_PIX_FMT_YUV444 && sd.luma_stride > (size_t)INT32_MAX / 4) return UHDR_HIP_ERROR_INVALID_STRIDE;
      if (hd.width != sd.width || hd.height != sd.height) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
      if (!valid_gamut(sd.colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    }
    if (exif != nullptr && exif[i] == nullptr && exif_size[i] != 0) return UHDR_HIP_ERROR_BAD_PTR;
    // uhdr_hip_generate_gainmap_packed_batch's own
    if (!api0 && sd.pixelFormat != UHDR_HIP_PIX_FMT_RGBA8888) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (hd.pixelFormat != UHDR_HIP_PIX_FMT_RGBA1010102 && hd.pixelFormat != UHDR_HIP_PIX_FMT_RGBA_F16) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    const bool f16 = hd.pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16;
    if (!host && ((!api0 && !al(sd.data, 4)) || !al(hd.data, f16 ? 8 : 4))) return UHDR_HIP_ERROR_BAD_PTR;
    if (f16 ? hdr_tf != UHDR_HIP_TF_LINEAR : hdr_tf == UHDR_HIP_TF_LINEAR) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
    if (api0 && peaks != nullptr && !valid_peak_nits(peaks[i])) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    return UHDR_HIP_NO_ERROR;
  };
  struct PackedFile {
    int idx;
    uhdr_hip_image_t hdr, sdr;   // luma_stride set; device images once staged
    std::vector<uint8_t> icc;
  };
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  std::vector<PackedFile> files;
  for (int i = 0; i < n; ++i) {
    if ((st_[i] = check(hdr_images[i], api0 ? hdr_images[i] : sdr_images[i], i)) != UHDR_HIP_NO_ERROR) continue;
    PackedFile f{i, hdr_images[i], api0 ? hdr_images[i] : sdr_images[i], {}};
    if (api0) {   // the SDR image to come: the HDR image's size and gamut, rows of its own in the round's pool
      f.sdr.data = nullptr; f.sdr.luma_stride = 0; f.sdr.pixelFormat = UHDR_HIP_PIX_FMT_RGBA8888;
    }
    if (f.hdr.luma_stride == 0) f.hdr.luma_stride = f.hdr.width;
    if (f.sdr.luma_stride == 0) f.sdr.luma_stride = f.sdr.width;
    if (!jpegr::icc_profile_srgb_transfer(f.sdr.colorGamut, f.icc)) { st_[i] = UHDR_HIP_ERROR_INVALID_COLORGAMUT; continue; }
    files.push_back(std::move(f));
  }
  if (files.empty()) return finish_statuses(st_, status);
  // hdr_tf is shared, so every file that passed has the same HDR format
  const size_t hdr_bpp = files[0].hdr.pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16 ? 8 : 4, map_bpp = rgb_map != 0 ? 4 : 1;
  auto key = [](const PackedFile& f) { return std::make_tuple(f.sdr.width, f.sdr.height, f.sdr.colorGamut, f.hdr.colorGamut); };
  std::stable_sort(files.begin(), files.end(), [&](const PackedFile& x, const PackedFile& y) { return key(x) < key(y); });
  auto al256 = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t done = 0;
  const int carry_all = boost_scope == UHDR_HIP_BOOST_PER_CALL && files.size() > (size_t)kEncRound ? 2 : 0;
  std::vector<float> range(2 * (size_t)kEncRound);
  // one round: f[0 .. m) staged, tone-mapped, generated; carry == 1 stops behind the measuring pass
  auto round = [&](DeviceState* st, hipStream_t s, PackedFile* f, int m, int carry) -> int {
        int rc;
        size_t map_total = 0, sdr_total = 0, hdr_total = 0;
        for (int k = 0; k < m; ++k) {
          const size_t w = f[k].sdr.width, h = f[k].sdr.height;
          map_total += al256((w / 4) * (h / 4) * map_bpp + 64);
          if (host || api0) sdr_total += rgba_stage_bytes(w, h, 4);
          if (host) hdr_total += rgba_stage_bytes(w, h, hdr_bpp);
        }
        if (api0 && (rc = pool_reserve(st, kEncToneHead, sizeof(float) * (size_t)m)) != 0) return rc;
        if ((rc = pool_reserve(st, kEncMap, map_total)) != 0) return rc;
        if (sdr_total && (rc = pool_reserve(st, kEncYuv, sdr_total)) != 0) return rc;
        if (hdr_total && (rc = pool_reserve(st, kEncP010, hdr_total)) != 0) return rc;
        std::vector<uhdr_hip_image_t> a((size_t)m), b((size_t)m), c((size_t)m);
        size_t o_map = 0, o_sdr = 0, o_hdr = 0;
        for (int k = 0; k < m; ++k) {
          PackedFile& e = f[k];
          const size_t w = e.sdr.width, h = e.sdr.height;
          size_t bytes = 0;
          if (api0) {   // the SDR image to come: rows of its own at the staged pitch
            e.sdr.data = static_cast<uint8_t*>(st->pool[kEncYuv]) + o_sdr; e.sdr.luma_stride = round_up(w * 4, 64) / 4;
            o_sdr += rgba_stage_bytes(w, h, 4);
          } else if (host) {
            if ((rc = stage_rgba_rows(static_cast<uint8_t*>(st->pool[kEncYuv]) + o_sdr, e.sdr, 4, &e.sdr, &bytes, s)) != 0) return rc;
            o_sdr += bytes;
          }
          if (host) {
            if ((rc = stage_rgba_rows(static_cast<uint8_t*>(st->pool[kEncP010]) + o_hdr, e.hdr, hdr_bpp, &e.hdr, &bytes, s)) != 0) return rc;
            o_hdr += bytes;
          }
          a[(size_t)k] = e.sdr; b[(size_t)k] = e.hdr;
          memset(&c[(size_t)k], 0, sizeof(uhdr_hip_image_t));
          c[(size_t)k].data = static_cast<uint8_t*>(st->pool[kEncMap]) + o_map;
          o_map += al256((w / 4) * (h / 4) * map_bpp + 64);
        }
        if (api0) {   // the SDR images, H in a pool slot
          std::vector<float> pk((size_t)m, 0.0f);
          for (int k = 0; peaks != nullptr && k < m; ++k) pk[(size_t)k] = peaks[f[k].idx];
          if ((rc = uhdr_hip_tonemap_packed_batch(m, b.data(), a.data(), hdr_tf, UHDR_HIP_TONEMAP_REINHARD_MAXRGB, pk.data(),
                                                  static_cast<float*>(st->pool[kEncToneHead]), s)) != UHDR_HIP_NO_ERROR)
            return rc;
        }
        uhdr_hip_metadata_t md{};
        float* dev_range = nullptr;
        if (boost_scope < 0) {
          if ((rc = uhdr_hip_generate_gainmap_packed_batch(m, a.data(), b.data(), hdr_tf, nullptr, &md, c.data(), rgb_map, s)) != UHDR_HIP_NO_ERROR) return rc;
        } else {
          const size_t ws_bytes = adaptive_layout(m, a.data(), packed_gain_bytes(rgb_map != 0)).total;
          if ((rc = pool_reserve(st, kEncAdaptWs, ws_bytes + 256 + round_up(8 * (size_t)m, 256))) != 0) return rc;
          uint8_t* ws = static_cast<uint8_t*>(st->pool[kEncAdaptWs]);
          dev_range = reinterpret_cast<float*>(ws + ws_bytes + 256);
          uint32_t* cw = carry != 0 ? static_cast<uint32_t*>(st->pool[kEncAdaptCarry]) : nullptr;
          if ((rc = packed_adaptive_enqueue(m, a.data(), b.data(), hdr_tf, c.data(), rgb_map != 0, boost_scope, nullptr, dev_range, ws, cw,
                                            carry == 1 ? cw : nullptr, carry != 1, s)) != UHDR_HIP_NO_ERROR)
            return rc;
          if (carry == 1) return UHDR_HIP_NO_ERROR;
        }
        std::vector<EncJpeg> jpg(2 * (size_t)m);
        if (primary_sampling == UHDR_HIP_PIX_FMT_YUV444) {
          for (int k = 0; k < m; ++k) {   // the pixels as they stand: the encoder converts as it loads (jpeg::kGeomRgb444)
            EncJpeg& e = jpg[2 * (size_t)k];
            e.img = a[(size_t)k];
            e.img.chroma_data = nullptr; e.img.chroma_stride = 0;
            e.pad_ls = e.pad_cs = 0;
            e.rgb = true;
          }
        } else if ((rc = rgba420_planes(st, kEncSdr, s, m, a.data(), jpg.data(), 2, primary_sampling == UHDR_HIP_PIX_FMT_YUV422)) != 0) {
          return rc;
        }
        for (int k = 0; k < m; ++k) {
          jpg[2 * (size_t)k].quality = quality;
          jpg[2 * (size_t)k].icc = &f[k].icc;
          uhdr_hip_image_t g = c[(size_t)k];   // (generate has filled in width, height and stride)
          jpg[2 * (size_t)k + 1] = rgb_map != 0 ? gainmap_rgb_jpeg(g) : gainmap_jpeg(g, g.luma_stride);
          eo.to(&jpg[2 * (size_t)k]);
          eo.to(&jpg[2 * (size_t)k + 1]);
        }
        if ((rc = compress_to_host(st, s, 2 * m, jpg.data(), true, EncExtra{dev_range, dev_range ? 8 * (size_t)m : 0, range.data()})) != UHDR_HIP_NO_ERROR)
          return rc;
        append_containers(m, jpg.data(), [f](int k) { return f[k].idx; }, md, boost_scope >= 0 ? range.data() : nullptr, exif, exif_size, out,
                          out_capacity, out_size, st_.data(), opt.metadata);
        return (int)UHDR_HIP_NO_ERROR;
  };
  const int rc = run_rounds(
      files.size(), (size_t)kEncRound, stream, [](size_t) { return (size_t)0; },   // rounds by count alone
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        // the measuring pass needs the leased context, which the driver hands over with a round: it goes in front of the first one
        const int rc = carry_all != 0 && r0 == 0 ? measure_all_rounds(st, s, files, round) : (int)UHDR_HIP_NO_ERROR;
        return rc != UHDR_HIP_NO_ERROR ? rc : round(st, s, &files[r0], m, carry_all);
      },
      &done);
  for (size_t k = done; k < files.size(); ++k) st_[files[k].idx] = rc;   // the files of the failed round and of those behind it
  return finish_statuses(st_, status);
}

int uhdr_hip_jpegr_encode_packed_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf, int quality,
                                       const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                       size_t* out_size, int* status, int rgb_map, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, hdr_images, sdr_images, true, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  // (n == 0 with sdr_images == NULL: no file, so nothing distinguishes the two forms)
  static const uhdr_hip_image_t none{};
  JpegrOpt opt;
  opt.rgb_map = rgb_map != 0;
  return encode_packed_files(n, hdr_images, sdr_images != nullptr ? sdr_images : &none, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size,
                             status, mem_space, stream, opt);
}

// the packed call with the primary image's sampling and the encoder's options said; YUV420 and NULL opts:
// that call
int uhdr_hip_jpegr_encode_packed_sampling_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf,
                                                int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                                const size_t* out_capacity, size_t* out_size, int* status, int rgb_map, int primary_sampling,
                                                const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream) {
  EncOpt eo;
  const int orc = encode_opts(opts, &eo);
  if (orc != UHDR_HIP_NO_ERROR) return orc;
  if (primary_sampling != UHDR_HIP_PIX_FMT_YUV444 && primary_sampling != UHDR_HIP_PIX_FMT_YUV422 && primary_sampling != UHDR_HIP_PIX_FMT_YUV420)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  const int rc = jpegr_batch_gate(n, hdr_images, sdr_images, true, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  static const uhdr_hip_image_t none{};
  JpegrOpt opt;
  opt.rgb_map = rgb_map != 0;
  opt.primary_sampling = primary_sampling;
  opt.enc = eo;
  return encode_packed_files(n, hdr_images, sdr_images != nullptr ? sdr_images : &none, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size,
                             status, mem_space, stream, opt);
}

// the packed API-0: the same files from the HDR images alone
int uhdr_hip_jpegr_encode_packed_api0_batch(int n, const uhdr_hip_image_t* hdr_images, int hdr_tf, int quality, const void* const* exif,
                                            const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                                            uhdr_hip_metadata_t* metadata, int* status, int tonemap_op, const float* hdr_peak_nits, int rgb_map,
                                            int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, hdr_images, nullptr, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (tonemap_op != UHDR_HIP_TONEMAP_REINHARD_MAXRGB) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  JpegrOpt opt;
  opt.metadata = metadata;
  opt.peaks = hdr_peak_nits;
  opt.rgb_map = rgb_map != 0;
  return encode_packed_files(n, hdr_images, nullptr, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

// both with the adaptive generate: sdr_images == NULL is the packed API-0
int uhdr_hip_jpegr_encode_packed_adaptive_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf, int quality,
                                                const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                                size_t* out_size, uhdr_hip_metadata_t* metadata, int* status, const float* hdr_peak_nits,
                                                int rgb_map, int boost_scope, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, hdr_images, sdr_images, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!valid_boost_scope(boost_scope)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  JpegrOpt opt;
  opt.boost_scope = boost_scope;
  opt.metadata = metadata;
  opt.peaks = sdr_images == nullptr ? hdr_peak_nits : nullptr;
  opt.rgb_map = rgb_map != 0;
  return encode_packed_files(n, hdr_images, sdr_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

int uhdr_hip_jpegr_encode_adaptive_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf,
                                         int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                         const size_t* out_capacity, size_t* out_size, uhdr_hip_metadata_t* metadata, int* status,
                                         int boost_scope, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, p010_images, yuv420_images, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!valid_boost_scope(boost_scope)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  JpegrOpt opt;
  opt.boost_scope = boost_scope;
  opt.metadata = metadata;
  return encode_files(n, p010_images, yuv420_images, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

int uhdr_hip_jpegr_encode_api0_tonemapped_batch(int n, const uhdr_hip_image_t* p010_images, int hdr_tf, int quality, const void* const* exif,
                                                const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                                                uhdr_hip_metadata_t* metadata, int* status, int tonemap_op, const float* hdr_peak_nits,
                                                int boost_scope, int mem_space, void* stream) {
  const int rc = jpegr_batch_gate(n, p010_images, nullptr, false, quality, exif, exif_size, out, out_capacity, out_size);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (tonemap_op != UHDR_HIP_TONEMAP_SHIFT && tonemap_op != UHDR_HIP_TONEMAP_REINHARD_MAXRGB) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (boost_scope != -1 && !valid_boost_scope(boost_scope)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  JpegrOpt opt;
  opt.boost_scope = boost_scope;
  opt.metadata = metadata;
  opt.tonemap_op = tonemap_op;
  opt.peaks = hdr_peak_nits;
  return encode_files(n, p010_images, nullptr, hdr_tf, quality, exif, exif_size, out, out_capacity, out_size, status, mem_space, stream, opt);
}

// JpegR::encodeJPEGR API-0 (jpegr.cpp:186-247): a batch of one file
int uhdr_hip_jpegr_encode_api0(const uhdr_hip_image_t* p010_in, int hdr_tf, int quality, const void* exif, size_t exif_size, void* out,
                               size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;                                 // :175-183
  return encode_files(1, p010_in, nullptr, hdr_tf, quality, &exif, &exif_size, &out, &out_capacity, out_size, nullptr, mem_space, stream);
}

// JpegR::encodeJPEGR API-1 (jpegr.cpp:249-381): a batch of one file
int uhdr_hip_jpegr_encode_api1(const uhdr_hip_image_t* p010_in, const uhdr_hip_image_t* yuv_in, int hdr_tf, int quality, const void* exif,
                               size_t exif_size, void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  if (yuv_in == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                           // :253-256
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;                                 // :175-183
  return encode_files(1, p010_in, yuv_in, hdr_tf, quality, &exif, &exif_size, &out, &out_capacity, out_size, nullptr, mem_space, stream);
}

// JpegR::encodeJPEGR API-4 (jpegr.cpp:502-560): host bytes only, nothing runs on the device
int uhdr_hip_jpegr_encode_api4(const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut, const void* gainmap_jpeg, size_t gainmap_jpeg_size,
                               const uhdr_hip_metadata_t* metadata, void* out, size_t out_capacity, size_t* out_size) {
  if (sdr_jpeg == nullptr || gainmap_jpeg == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                              // :505-512
  if (out == nullptr || out_size == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                       // :513-516
  std::vector<uint8_t> icc;
  const int rc = sdr_jpeg_check(sdr_jpeg, sdr_jpeg_size, sdr_jpeg_gamut, &icc);                                   // :520-541
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (metadata == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                         // :955-958
  return jpegr::append_gainmap_to(static_cast<const uint8_t*>(sdr_jpeg), sdr_jpeg_size, static_cast<const uint8_t*>(gainmap_jpeg), gainmap_jpeg_size,
                                  nullptr, 0, icc.empty() ? nullptr : icc.data(), icc.size(), *metadata, static_cast<uint8_t*>(out), out_capacity, out_size);
}

}  // extern "C"

namespace {
// ---- encodeJPEGR API-2 / API-3 / API-x for n files (uhdr_hip_jpegr_encode_sdr_jpeg_batch, uhdr_hip_jpegr_encode_apix_batch) -------
// Their rounds' pool slots: jpeg_decode_round holds kDecWs .. kDecScratch (0-3) and compress_to_host kEncWs and kEncDesc (0, 1), so
// the staged P010 planes, the SDR planes (staged, or decoded by API-3) and the gain maps lie in slots that neither touches.  Every slot
// of a round is reserved before its first enqueue.
enum : size_t { kSjP010 = kEncP010, kSjSdr = kEncYuv, kSjMap };

// one API-2 / API-3 file
struct SjFile {
  int idx = 0;                 // the caller's index
  uhdr_hip_image_t p010, sdr;  // defaulted P010 and SDR planes (API-2: the caller's YUV420, API-3: the decoded JPEG); device once staged
  int sdr_gamut = 0;           // what the runs are sorted by (API-3: the ICC profile's gamut, else the configured one)
  std::vector<uint8_t> icc;    // the ICC profile the container adds (the SDR JPEG carries none)
  size_t o_p010 = 0, o_sdr = 0, o_map = 0;   // the file's slices of its round
};

// the staging of stage_p010_in / stage_yuv420_in (pitches 64-aligned; the V plane at u + cp * (h / 2)), as one slice each
size_t sj_p010_bytes(size_t w, size_t h) { return round_up(round_up(w, 64) * h * 2, 256) + round_up(round_up(w, 64) * (h / 2) * 2, 256); }
size_t sj_yuv_bytes(size_t w, size_t h) { return round_up(round_up(w, 64) * h, 256) + round_up(round_up(w / 2, 64) * (h + 1), 256); }
size_t sj_map_bytes(size_t w, size_t h) { return round_up((w / 4) * (h / 4) + 64, 256); }
// what one file holds of its round: P010 / SDR planes, decoder workspace, gain map, its encoder workspace and page-locked staging
size_t sj_round_bytes(const SjFile& e, const jpeg::DecInfo* info, bool host) {
  const size_t w = e.p010.width, h = e.p010.height;
  uhdr_hip_image_t map;
  memset(&map, 0, sizeof(map));
  map.width = w / 4; map.height = h / 4; map.pixelFormat = UHDR_HIP_PIX_FMT_MONOCHROME;
  size_t b = sj_map_bytes(w, h) + enc_round_bytes(map, false, true);
  if (host) b += sj_p010_bytes(w, h) + (info ? 0 : sj_yuv_bytes(w, h));
  if (info) {
    jpeg::DecLayout l;
    b += jpeg::dec_workspace_bytes(*info, &l) + round_up(dec_ycc_bytes(*info) + 64, 256);
  }
  return b;
}

// One round of API-2 / API-3 files f[0, m): API-3's decode (one jpeg::decode_device_batch through jpeg_decode_round, with its own
// synchronisations) and the checks that follow it, the staging of host planes, generateGainMap for the files still live (equal files
// share a launch), their gain maps through one compress_to_host, then the containers around the caller's SDR JPEGs.  Statuses go
// to st_; a non-zero return is an error of the device or the runtime.
int sdr_jpeg_round(DeviceState* st, hipStream_t s, bool api3, bool host, int hdr_tf, SjFile* f, int m, const void* const* sdr_jpeg,
                   const size_t* sdr_jpeg_size, const int* sdr_jpeg_gamut, const jpeg::DecInfo* info, void** dec_out, const size_t* dec_need,
                   void* const* out, const size_t* out_capacity, size_t* out_size, int* st_) {
  int rc;
  size_t p010_total = 0, sdr_total = 0, map_total = 0;
  for (int k = 0; k < m; ++k) {
    SjFile& e = f[k];
    const size_t w = e.p010.width, h = e.p010.height;
    e.o_p010 = p010_total; e.o_sdr = sdr_total; e.o_map = map_total;
    if (host) p010_total += sj_p010_bytes(w, h);
    if (api3) sdr_total += round_up(dec_ycc_bytes(info[e.idx]) + 64, 256);
    else if (host) sdr_total += sj_yuv_bytes(w, h);
    map_total += sj_map_bytes(w, h);
  }
  if ((rc = pool_reserve(st, kSjMap, map_total)) != 0) return rc;   // (the last slot: the pool has all of them from here on)
  if (p010_total && (rc = pool_reserve(st, kSjP010, p010_total)) != 0) return rc;
  if (sdr_total && (rc = pool_reserve(st, kSjSdr, sdr_total)) != 0) return rc;
  uint8_t* const p010_pool = static_cast<uint8_t*>(st->pool[kSjP010]);
  uint8_t* const sdr_pool = static_cast<uint8_t*>(st->pool[kSjSdr]);
  uint8_t* const map_pool = static_cast<uint8_t*>(st->pool[kSjMap]);

  std::vector<int> live;   // the round's files that reach generateGainMap
  if (api3) {   // :457-462, every file of the round in one decode; the planes as uhdr_hip_jpeg_decode lays them out
    std::vector<int> idx((size_t)m);
    for (int k = 0; k < m; ++k) {
      idx[k] = f[k].idx;
      dec_out[f[k].idx] = sdr_pool + f[k].o_sdr;
    }
    if ((rc = jpeg_decode_round(st, s, false, false, sdr_jpeg, dec_out, info, dec_need, idx.data(), m, st_)) != 0) return rc;
    for (int k = 0; k < m; ++k) {
      SjFile& e = f[k];
      const int i = e.idx;
      if (st_[i] != UHDR_HIP_NO_ERROR) { st_[i] = UHDR_HIP_ERROR_DECODE_ERROR; continue; }   // corrupt entropy-coded data
      const size_t w = (size_t)info[i].w, h = (size_t)info[i].h;
      uint8_t* y = sdr_pool + e.o_sdr;
      memset(&e.sdr, 0, sizeof(e.sdr));
      e.sdr.data = y; e.sdr.chroma_data = y + w * h;
      e.sdr.width = w; e.sdr.height = h; e.sdr.luma_stride = w; e.sdr.chroma_stride = w / 2;
      e.sdr.pixelFormat = UHDR_HIP_PIX_FMT_YUV420;
      int gamut = UHDR_HIP_CG_UNSPECIFIED;
      rc = api3_check_decoded(e.p010, sdr_jpeg[i], sdr_jpeg_size[i], sdr_jpeg_gamut[i], w, h, &gamut);   // :467-499
      if (rc == UHDR_HIP_NO_ERROR) rc = sdr_jpeg_check(sdr_jpeg[i], sdr_jpeg_size[i], sdr_jpeg_gamut[i], &e.icc);
      st_[i] = rc;
      if (rc != UHDR_HIP_NO_ERROR) continue;
      e.sdr.colorGamut = gamut;
      live.push_back(k);
    }
  } else {
    for (int k = 0; k < m; ++k) live.push_back(k);
  }
  if (live.empty()) return UHDR_HIP_NO_ERROR;

  // host planes: the bytes the single calls stage
  if (host) {
    for (const int k : live) {
      SjFile& e = f[k];
      const size_t w = e.p010.width, h = e.p010.height, lp = round_up(w, 64);
      uint8_t* d = p010_pool + e.o_p010;
      uint8_t* dc = d + round_up(lp * h * 2, 256);
      if ((rc = h2d_plane(d, lp, e.p010.data, e.p010.luma_stride, w, h, 2, s)) != 0) return rc;
      if ((rc = h2d_plane(dc, lp, e.p010.chroma_data, e.p010.chroma_stride, w, h / 2, 2, s)) != 0) return rc;
      e.p010.data = d; e.p010.chroma_data = dc; e.p010.luma_stride = lp; e.p010.chroma_stride = lp;
      if (api3) continue;
      const size_t cp = round_up(w / 2, 64), cs = e.sdr.chroma_stride;
      uint8_t* y = sdr_pool + e.o_sdr;
      uint8_t* u = y + round_up(lp * h, 256);
      const uint8_t* hu = static_cast<const uint8_t*>(e.sdr.chroma_data);
      if ((rc = h2d_plane(y, lp, e.sdr.data, e.sdr.luma_stride, w, h, 1, s)) != 0) return rc;
      if ((rc = h2d_plane(u, cp, hu, cs, w / 2, h / 2, 1, s)) != 0) return rc;
      if ((rc = h2d_plane(u + cp * (h / 2), cp, hu + cs * (h / 2), cs, w / 2, h / 2, 1, s)) != 0) return rc;
      e.sdr.data = y; e.sdr.chroma_data = u; e.sdr.luma_stride = lp; e.sdr.chroma_stride = cp;
    }
  }
  // generateGainMap (:416-427 / :490-492): the files are sorted by size and gamuts, so equal ones share its launches
  const int ml = (int)live.size();
  std::vector<uhdr_hip_image_t> a((size_t)ml), b((size_t)ml), c((size_t)ml);
  for (int j = 0; j < ml; ++j) {
    const SjFile& e = f[live[j]];
    a[j] = e.sdr; b[j] = e.p010; c[j] = e.sdr;
    c[j].data = map_pool + e.o_map;
  }
  uhdr_hip_metadata_t md;
  if ((rc = uhdr_hip_generate_gainmap_batch(ml, a.data(), b.data(), hdr_tf, &md, c.data(), api3 ? 1 : 0, nullptr, s)) != UHDR_HIP_NO_ERROR) return rc;
  // compressGainMap (:428-434), every map of the round in one compress_to_host
  std::vector<EncJpeg> gm((size_t)ml);
  for (int j = 0; j < ml; ++j) {
    uhdr_hip_image_t g = c[j];
    g.width = a[j].width / 4; g.height = a[j].height / 4; g.luma_stride = g.width;
    gm[j] = gainmap_jpeg(g, g.luma_stride);
  }
  if (compress_to_host(st, s, ml, gm.data()) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_ENCODE_ERROR;
  // appendGainMap around the caller's SDR JPEG (API-4, :543-559), straight into the caller's buffers
  on_host_threads(ml, [&](int lo, int hi) {
    for (int j = lo; j < hi; ++j) {
      const SjFile& e = f[live[j]];
      const int i = e.idx;
      st_[i] = jpegr::append_gainmap_to(static_cast<const uint8_t*>(sdr_jpeg[i]), sdr_jpeg_size[i], gm[j].bytes, gm[j].n, nullptr, 0,
                                        e.icc.empty() ? nullptr : e.icc.data(), e.icc.size(), md, static_cast<uint8_t*>(out[i]), out_capacity[i],
                                        &out_size[i]);
    }
  });
  return UHDR_HIP_NO_ERROR;
}

// encodeJPEGR API-2 (yuv420_images != NULL) or API-3 for n files: every host check first (API-3's header probes on a few threads),
// then rounds of up to kEncRound files and kCodecRoundBytes, sorted into runs of equal size and gamuts
int sdr_jpeg_files(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, const void* const* sdr_jpeg,
                   const size_t* sdr_jpeg_size, const int* sdr_jpeg_gamut, int hdr_tf, void* const* out, const size_t* out_capacity,
                   size_t* out_size, int* status, int mem_space, void* stream) {
  const bool api3 = yuv420_images == nullptr;
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  std::vector<jpeg::DecInfo> info(api3 ? (size_t)n : 0);
  std::vector<void*> dec_out(api3 ? (size_t)n : 0, nullptr);   // API-3: where each file is decoded, and its bytes
  std::vector<size_t> dec_need(api3 ? (size_t)n : 0, 0);
  std::vector<std::vector<uint8_t>> icc(api3 ? 0 : (size_t)n);
  on_host_threads(n, [&](int lo, int hi) {   // the single call's checks, in its order; API-2's checks of the SDR JPEG included
    for (int i = lo; i < hi; ++i) {
      if (api3) {
        st_[i] = api3_check(p010_images + i, sdr_jpeg[i], sdr_jpeg_size[i], hdr_tf, out[i], out_size + i, &info[i]);
        if (st_[i] == UHDR_HIP_NO_ERROR) dec_need[i] = dec_ycc_bytes(info[i]);
      } else {
        st_[i] = api2_check(p010_images + i, yuv420_images + i, sdr_jpeg[i], hdr_tf, out[i], out_size + i);
        if (st_[i] == UHDR_HIP_NO_ERROR) st_[i] = sdr_jpeg_check(sdr_jpeg[i], sdr_jpeg_size[i], sdr_jpeg_gamut[i], &icc[i]);
      }
    }
  });
  std::vector<SjFile> files;
  for (int i = 0; i < n; ++i) {
    if (st_[i] != UHDR_HIP_NO_ERROR) continue;
    SjFile e;
    e.idx = i;
    e.p010 = p010_images[i];
    default_p010(&e.p010);
    memset(&e.sdr, 0, sizeof(e.sdr));
    if (api3) {
      const uint8_t* ip = nullptr;
      size_t in = 0;
      e.sdr_gamut = jpegr::first_icc(static_cast<const uint8_t*>(sdr_jpeg[i]), sdr_jpeg_size[i], &ip, &in) ? jpegr::gamut_from_icc(ip, in) : sdr_jpeg_gamut[i];
    } else {
      e.sdr = yuv420_images[i];
      default_yuv(&e.sdr);
      e.sdr_gamut = e.sdr.colorGamut;
      e.icc = std::move(icc[i]);
    }
    files.push_back(std::move(e));
  }
  if (files.empty()) return finish_statuses(st_, status);   // every file stopped at its checks: the device is not touched
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  auto key = [](const SjFile& e) { return std::make_tuple(e.p010.width, e.p010.height, e.sdr_gamut, e.p010.colorGamut); };
  std::stable_sort(files.begin(), files.end(), [&](const SjFile& x, const SjFile& y) { return key(x) < key(y); });
  size_t done = 0;
  const int rc = run_rounds(
      files.size(), (size_t)kEncRound, stream, [&](size_t k) { return sj_round_bytes(files[k], api3 ? &info[files[k].idx] : nullptr, host); },
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        return sdr_jpeg_round(st, s, api3, host, hdr_tf, &files[r0], m, sdr_jpeg, sdr_jpeg_size, sdr_jpeg_gamut, api3 ? info.data() : nullptr,
                              dec_out.data(), dec_need.data(), out, out_capacity, out_size, st_.data());
      },
      &done);
  for (size_t k = done; k < files.size(); ++k)   // the files of a failed round still open, and those behind it
    if (st_[files[k].idx] == UHDR_HIP_NO_ERROR) st_[files[k].idx] = rc;
  return finish_statuses(st_, status);
}

// one API-x file
struct XFile {
  int idx = 0;
  uhdr_hip_image_t yuv, map;   // as apix_check leaves them; device once staged
  std::vector<uint8_t> icc;
};

// One round of API-x files f[0, m): host planes staged by stage_encoder_in's rules, the 2 m JPEGs (the SDR image at `quality` with its ICC
// profile, the gain map at 85) through one compress_to_host, then the containers.  A non-zero return is an error of the device or the runtime.
int apix_round(DeviceState* st, hipStream_t s, bool host, int quality, const XFile* f, int m, const uhdr_hip_metadata_t* metadata,
               const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* st_) {
  std::vector<EncJpeg> jpg;
  jpg.reserve(2 * (size_t)m);
  int rc;
  if (host) {
    size_t total = 0;
    for (int k = 0; k < m; ++k) total += enc_stage_bytes(f[k].yuv) + enc_stage_bytes(f[k].map);
    if ((rc = pool_reserve(st, kEncYuv, total)) != 0) return rc;
  }
  size_t o = 0;
  for (int k = 0; k < m; ++k) {
    const XFile& e = f[k];
    jpg.push_back(EncJpeg{e.yuv, quality, &e.icc, e.yuv.luma_stride, e.yuv.chroma_stride});
    jpg.push_back(gainmap_jpeg(e.map, e.map.luma_stride));
    if (!host) continue;
    uint8_t* pool = static_cast<uint8_t*>(st->pool[kEncYuv]);
    if ((rc = stage_encoder_slice(pool + o, e.yuv, &jpg[2 * (size_t)k].img, s)) != 0) return rc;
    o += enc_stage_bytes(e.yuv);
    if ((rc = stage_encoder_slice(pool + o, e.map, &jpg[2 * (size_t)k + 1].img, s)) != 0) return rc;
    o += enc_stage_bytes(e.map);
  }
  if (compress_to_host(st, s, 2 * m, jpg.data()) != UHDR_HIP_NO_ERROR) return UHDR_HIP_ERROR_ENCODE_ERROR;
  on_host_threads(m, [&](int lo, int hi) {   // appendGainMap (:613-630) straight into the caller's buffers
    for (int k = lo; k < hi; ++k) {
      const int i = f[k].idx;
      const EncJpeg& sdr = jpg[2 * (size_t)k];
      const EncJpeg& gm = jpg[2 * (size_t)k + 1];
      st_[i] = jpegr::append_gainmap_to(sdr.bytes, sdr.n, gm.bytes, gm.n, static_cast<const uint8_t*>(exif ? exif[i] : nullptr), exif ? exif_size[i] : 0,
                                        nullptr, 0, metadata[i], static_cast<uint8_t*>(out[i]), out_capacity[i], &out_size[i]);
    }
  });
  return UHDR_HIP_NO_ERROR;
}
}  // namespace

extern "C" {

int uhdr_hip_jpegr_encode_sdr_jpeg_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images,
                                         const void* const* sdr_jpeg, const size_t* sdr_jpeg_size, const int* sdr_jpeg_gamut, int hdr_tf,
                                         void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream) {
  if (n < 0 || (n > 0 && (p010_images == nullptr || sdr_jpeg == nullptr || sdr_jpeg_size == nullptr || sdr_jpeg_gamut == nullptr || out == nullptr ||
                          out_capacity == nullptr || out_size == nullptr)))
    return UHDR_HIP_ERROR_BAD_PTR;
  return sdr_jpeg_files(n, p010_images, yuv420_images, sdr_jpeg, sdr_jpeg_size, sdr_jpeg_gamut, hdr_tf, out, out_capacity, out_size, status,
                        mem_space, stream);
}

int uhdr_hip_jpegr_encode_apix_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* gainmap_images,
                                     const uhdr_hip_metadata_t* metadata, int quality, const void* const* exif, const size_t* exif_size,
                                     void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream) {
  if (n < 0 || (n > 0 && (yuv420_images == nullptr || gainmap_images == nullptr || metadata == nullptr || out == nullptr || out_capacity == nullptr ||
                          out_size == nullptr)) ||
      (exif != nullptr && exif_size == nullptr))
    return UHDR_HIP_ERROR_BAD_PTR;
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;                                 // :566-568
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  std::vector<XFile> files;
  for (int i = 0; i < n; ++i) {   // the single call's checks, in its order, then appendGainMap's metadata checks (:961-984)
    const uhdr_hip_image_t& y = yuv420_images[i];
    const uhdr_hip_image_t& g = gainmap_images[i];
    if (y.data == nullptr || g.data == nullptr || out[i] == nullptr) { st_[i] = UHDR_HIP_ERROR_BAD_PTR; continue; }
    XFile e;
    e.idx = i;
    int rc = apix_check(y, g, &e.yuv, &e.map, &e.icc);
    if (rc == UHDR_HIP_NO_ERROR && !jpegr::metadata_valid(metadata[i])) rc = UHDR_HIP_ERROR_BAD_METADATA;
    if (rc != UHDR_HIP_NO_ERROR) { st_[i] = rc; continue; }
    files.push_back(std::move(e));
  }
  if (files.empty()) return finish_statuses(st_, status);   // every file stopped at its checks: the device is not touched
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  size_t done = 0;
  const int rc = run_rounds(
      files.size(), (size_t)kEncRound, stream,
      [&](size_t k) { return enc_round_bytes(files[k].yuv, host, true) + enc_round_bytes(files[k].map, host, true); },
      [&](DeviceState* st, hipStream_t s, size_t r0, int m) {
        return apix_round(st, s, host, quality, &files[r0], m, metadata, exif, exif_size, out, out_capacity, out_size, st_.data());
      },
      &done);
  for (size_t k = done; k < files.size(); ++k) st_[files[k].idx] = rc;   // the files of a failed round and of those behind it
  return finish_statuses(st_, status);
}

// JpegR::encodeJPEGR API-2 (jpegr.cpp:384-437): a batch of one file
int uhdr_hip_jpegr_encode_api2(const uhdr_hip_image_t* p010_in, const uhdr_hip_image_t* yuv_in, const void* sdr_jpeg, size_t sdr_jpeg_size,
                               int sdr_jpeg_gamut, int hdr_tf, void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  if (yuv_in == nullptr) return UHDR_HIP_ERROR_BAD_PTR;                                                           // :390-393
  return sdr_jpeg_files(1, p010_in, yuv_in, &sdr_jpeg, &sdr_jpeg_size, &sdr_jpeg_gamut, hdr_tf, &out, &out_capacity, out_size, nullptr, mem_space,
                        stream);
}

// JpegR::encodeJPEGR API-3 (jpegr.cpp:439-500), the SDR rendition arrives as a JPEG only and is decoded on the device: a batch of one file
int uhdr_hip_jpegr_encode_api3(const uhdr_hip_image_t* p010_in, const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut, int hdr_tf,
                               void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  return sdr_jpeg_files(1, p010_in, nullptr, &sdr_jpeg, &sdr_jpeg_size, &sdr_jpeg_gamut, hdr_tf, &out, &out_capacity, out_size, nullptr, mem_space,
                        stream);
}

// JpegR::encodeJPEGR "API-x" (jpegr.cpp:562-631), SDR planes + a ready gain map + its metadata, no BT.601 re-encode: a batch of one file
int uhdr_hip_jpegr_encode_apix(const uhdr_hip_image_t* yuv_in, const uhdr_hip_image_t* gainmap, const uhdr_hip_metadata_t* metadata, int quality,
                               const void* exif, size_t exif_size, void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream) {
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;                                 // :566-568
  if (yuv_in == nullptr || gainmap == nullptr || metadata == nullptr || out_size == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return uhdr_hip_jpegr_encode_apix_batch(1, yuv_in, gainmap, metadata, quality, &exif, &exif_size, &out, &out_capacity, out_size, nullptr, mem_space,
                                          stream);
}

// JpegR::getJPEGRInfo (jpegr.cpp:633-653)
int uhdr_hip_jpegr_info(const void* jpegr, size_t jpegr_size, uhdr_hip_jpeg_info_t* primary, uhdr_hip_jpeg_info_t* gainmap) {
  if (jpegr == nullptr || primary == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const uint8_t* file = static_cast<const uint8_t*>(jpegr);
  jpegr::Range img[2];
  const int found = jpegr::find_images(file, jpegr_size, img);
  if (found == 0) return UHDR_HIP_ERROR_NO_IMAGES_FOUND;
  if (found == 1) return UHDR_HIP_ERROR_GAIN_MAP_IMAGE_NOT_FOUND;
  auto parse = [&](const jpegr::Range& r, uhdr_hip_jpeg_info_t* info) -> int {   // parseJpegInfo :878-915
    const uint8_t* j = file + r.begin;
    struct { int w, h; } di;
    if (!jpegr::has_valid_header(j, r.len) || !jpegr::dimensions(j, r.len, &di.w, &di.h)) return UHDR_HIP_ERROR_DECODE_ERROR;
    if (di.w > 8192 || di.h > 8192) return UHDR_HIP_ERROR_DECODE_ERROR;                                         // jpegdecoderhelper.cpp:251-256
    memset(info, 0, sizeof(*info));
    info->offset = r.begin; info->size = r.len;
    info->width = (size_t)di.w; info->height = (size_t)di.h;
    jpegr::first_packets(j, r.len, &info->xmp_offset, &info->xmp_size, &info->exif_offset, &info->exif_size, &info->icc_offset, &info->icc_size);
    if (info->xmp_size) info->xmp_offset += r.begin;
    if (info->exif_size) info->exif_offset += r.begin;
    if (info->icc_size) info->icc_offset += r.begin;
    return UHDR_HIP_NO_ERROR;
  };
  int rc = parse(img[0], primary);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  return gainmap != nullptr ? parse(img[1], gainmap) : UHDR_HIP_NO_ERROR;
}

int uhdr_hip_jpegr_metadata(const void* jpegr, size_t jpegr_size, uhdr_hip_metadata_t* metadata) {
  if (jpegr == nullptr || metadata == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const uint8_t* file = static_cast<const uint8_t*>(jpegr);
  jpegr::Range img[2];
  const int found = jpegr::find_images(file, jpegr_size, img);
  if (found == 0) return UHDR_HIP_ERROR_NO_IMAGES_FOUND;
  if (found == 1) return UHDR_HIP_ERROR_GAIN_MAP_IMAGE_NOT_FOUND;
  const uint8_t* xmp = nullptr;
  size_t xmp_len = 0;
  if (!jpegr::first_xmp(file + img[1].begin, img[1].len, &xmp, &xmp_len) ||
      !jpegr::metadata_from_xmp(xmp, xmp_len, metadata))
    return UHDR_HIP_ERROR_METADATA_ERROR;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_lut_table(int which, float* out, size_t capacity, size_t* count) {
  if (out == nullptr || count == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  const int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  uint32_t off = 0, n = 0;
  switch (which) {
    case 0: off = kLutSrgbInv; n = kLutSrgbInvN; break;
    case 1: off = kLutHlgInv; n = kLutHlgInvN; break;
    case 2: off = kLutPqInv; n = kLutPqInvN; break;
    case 4: off = kLutHlg; n = kLutHlgN; break;
    case 5: off = kLutPq; n = kLutPqN; break;
    default: return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  }
  *count = n;
  if (capacity < n) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  HIP_TRY(hipMemcpy(out, st->lut + off, sizeof(float) * n, hipMemcpyDeviceToHost));
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_gain_lut(const uhdr_hip_metadata_t* metadata, int with_display_boost, float display_boost, float* out) {
  if (metadata == nullptr || out == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  float factor = 1.0f;  // gainmapmath.h:152-159 (no display boost) | :161-169
  if (with_display_boost) factor = display_boost > 0 ? display_boost / metadata->maxContentBoost : 1.0f;
  CodecLease lease(st);
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if ((rc = stage_reserve(st, 6, sizeof(float) * kGainLutN)) != 0) return rc;
  float* d = static_cast<float*>(st->stage[6]);
  HIP_TRY(launch_build_gain_lut(d, std::log2((double)metadata->minContentBoost), std::log2((double)metadata->maxContentBoost),
                                factor, nullptr));
  HIP_TRY(hipMemcpy(out, d, sizeof(float) * kGainLutN, hipMemcpyDeviceToHost));
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_idw_tables(int scale, float* out) {
  if (out == nullptr || scale <= 0) return UHDR_HIP_ERROR_BAD_PTR;
  std::vector<float> t;
  build_idw_tables(scale, t);
  memcpy(out, t.data(), t.size() * sizeof(float));
  return UHDR_HIP_NO_ERROR;
}

// ---------------------------------------------------------------------------------------------------
// One chunk of uhdr_hip_generate_gainmap_batch_ex: up to kMaxChunk consecutive images, from image i on, of identical size, gamuts
// and alignment class; *m_out receives their number.  `phases` selects what is enqueued: kGenPhaseFilter the chunk's k_generate
// launch (with the clear or the finalize kernel of the routes that keep their keys in content_minmax), kGenPhaseResolve the
// k_generate_resolve launch behind a filtered one; the production call passes both.  0 enqueues nothing and needs no device
// (st may be null): the plan only -- `route` (or null) receives it, UHDR_HIP_GENERATE_ROUTE_* words.  `headers` (or null; device,
// kStatHdr words per image): after kGenPhaseFilter of a filtered + resolve pair, every image's header words, copied in stream order.
enum : unsigned { kGenPhaseFilter = 1u, kGenPhaseResolve = 2u };
static int generate_chunk(DeviceState* st, hipStream_t s, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s,
                          int hdr_tf, const uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601,
                          int generate_mode, float* content_minmax, int i, unsigned phases, int* m_out, uint32_t* route,
                          uint32_t* headers) {
  const bool lut = generate_mode == UHDR_HIP_GENERATE_LUT;
  // Content min / max.  The filtered kernel (the usual case) works in a workspace of the library: its candidates are resolved, the
  // result written to content_minmax and the workspace cleared by k_stats_resolve.  The other kernels keep exact keys in
  // content_minmax itself: cleared here, turned into floats by k_stats_finalize at the end.
  uint32_t* keys = reinterpret_cast<uint32_t*>(content_minmax);
  const uhdr_hip_image_t& y0 = yuvs[i];
  GenConsts c = generate_consts(y0.colorGamut, p010s[i].colorGamut, hdr_tf, sdr_is_601, y0.width, y0.height, *metadata);
  c.stat_keys = keys ? keys + 2 * i : nullptr;
  c.stat_stride = 2;
  c.lut = (lut && st != nullptr) ? st->lut : nullptr;
  GenBatch b;
  const Chunk ch = gen_chunk(i, n, yuvs, p010s, dests, b, no_more);   // (the descriptors are filled in the plan-only mode too)
  const int m = ch.m;
  const bool aligned = ch.cls;
  *m_out = m;
  bool filter = generate_mode == UHDR_HIP_GENERATE_EXACT && c.flt_delta < 0.25f && c.min_boost >= 0.25f && c.max_boost <= 64.0f;
  // The filtered kernel of a large launch leaves its pixels in doubt and the exact extremes to k_generate_resolve.  A small
  // launch (one 4K image) would pay that second kernel's latency with nothing to hide it behind: without statistics it runs the
  // filtered kernel that falls back to the exact path in place.  With statistics the choice is between the two kernels and the
  // exact kernel (every pixel on the f64 path: 5.5 us per megapixel against 0.75 + the resolve kernel's ~20 us): the pair from
  // about half a 4K frame up (round 3: 8 x 1080p 91 -> 30 us, 8 x 4K 141 -> 80), the exact kernel below.
  const bool small = generate_is_small(c, m);
  const bool pair = keys != nullptr ? generate_resolve_pays(c, m) : !small;
  if (keys != nullptr && !pair) filter = false;
  const bool resolve = filter && aligned && !lut && pair;
  if (resolve) {
    c.stat_stride = kStatWords;
    c.stat_out = keys ? content_minmax + 2 * i : nullptr;
    c.stat_spread = (m <= 16 && (uint64_t)((c.map_w + 1u) >> 1) * c.map_h >= 512u * 64u) ? 1u : 0u;
    c.stat_slots = generate_slot_waves(c, m);
  }
  if (route != nullptr) {
    memset(route, 0, sizeof(uint32_t) * UHDR_HIP_GENERATE_ROUTE_WORDS);
    route[UHDR_HIP_GENERATE_ROUTE_RESOLVE] = resolve ? 1u : 0u;
    route[UHDR_HIP_GENERATE_ROUTE_SPANS] = small ? 1u : (uint32_t)kGenTiles;
    route[UHDR_HIP_GENERATE_ROUTE_SLOTS] = c.stat_slots;
    route[UHDR_HIP_GENERATE_ROUTE_SPREAD] = c.stat_spread;
    route[UHDR_HIP_GENERATE_ROUTE_IMAGES] = (uint32_t)m;
    route[UHDR_HIP_GENERATE_ROUTE_BLOCK] = (uint32_t)kGenBlock;
    route[UHDR_HIP_GENERATE_ROUTE_HDR_WORDS] = kStatHdr;
    route[UHDR_HIP_GENERATE_ROUTE_SLOT_COUNTS] = kStatSlotCnt;
    route[UHDR_HIP_GENERATE_ROUTE_SLOT_PLAIN] = kStatSlotPlain;
    route[UHDR_HIP_GENERATE_ROUTE_SLOT_SAVED] = kStatSlotSaved;
    route[UHDR_HIP_GENERATE_ROUTE_LISTS] = kStatLists;
    route[UHDR_HIP_GENERATE_ROUTE_LIST_CAP] = kStatCap;
    route[UHDR_HIP_GENERATE_ROUTE_LIST_COUNTS] = 8u;   // GenConsts::stat_ws: [8 + l] entries in list l,
    route[UHDR_HIP_GENERATE_ROUTE_SWEEP_WORD] = 6u;    // [6] set by a wave whose slots overflowed
    route[UHDR_HIP_GENERATE_ROUTE_RESOLVE_SLICES] = kResolveSlices;
    route[UHDR_HIP_GENERATE_ROUTE_SLOT_WAVES] = kStatSlotWaves;
  }
  if (phases == 0u) return UHDR_HIP_NO_ERROR;
  std::unique_lock<std::mutex> pair_lk(g_pair_mu, std::defer_lock);
  if (resolve) pair_lk.lock();
  if (resolve) {
    uint32_t* w = nullptr;
    const int wrc = stat_workspace(st, s, &w);
    if (wrc != UHDR_HIP_NO_ERROR) return wrc;
    c.stat_ws = w;
    c.stat_keys = keys ? w + 4 : nullptr;
  } else if (keys != nullptr && (phases & kGenPhaseFilter)) {
    HIP_TRY(launch_stats_init(keys + 2 * i, m, s));
  }
  if (phases & kGenPhaseFilter) {
    HIP_TRY(launch_generate(c, b, m, hdr_tf, aligned, lut, filter, s));
    if (resolve && headers != nullptr)
      HIP_TRY(hipMemcpy2DAsync(headers, sizeof(uint32_t) * kStatHdr, c.stat_ws, sizeof(uint32_t) * kStatWords, sizeof(uint32_t) * kStatHdr,
                               (size_t)m, hipMemcpyDeviceToDevice, s));
  }
  if (resolve) {
    if (phases & kGenPhaseResolve) HIP_TRY(launch_stats_resolve(c, b, m, hdr_tf, aligned, s));
  } else if (keys != nullptr && (phases & kGenPhaseFilter)) {
    HIP_TRY(launch_stats_finalize(keys + 2 * i, m, s));
  }
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_generate_gainmap_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                    uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601,
                                    float* content_minmax, void* stream) {
  return uhdr_hip_generate_gainmap_batch_ex(n, yuvs, p010s, hdr_tf, metadata, dests, sdr_is_601, UHDR_HIP_GENERATE_EXACT,
                                            content_minmax, stream);
}

int uhdr_hip_generate_gainmap_batch_ex(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                       uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601,
                                       int generate_mode, float* content_minmax, void* stream) {
  if (generate_mode != UHDR_HIP_GENERATE_EXACT && generate_mode != UHDR_HIP_GENERATE_LUT &&
      generate_mode != UHDR_HIP_GENERATE_UNFILTERED)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  int rc = check_generate(n, yuvs, p010s, hdr_tf, metadata, dests, 1);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);

  fill_generate_metadata(hdr_tf, metadata);
  int i = 0;
  while (i < n) {
    int m = 0;
    rc = generate_chunk(st, s, n, yuvs, p010s, hdr_tf, metadata, dests, sdr_is_601, generate_mode, content_minmax, i,
                        kGenPhaseFilter | kGenPhaseResolve, &m, nullptr, nullptr);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
    i += m;
  }
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_generate_probe(int phase, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                            uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601, int generate_mode,
                            float* content_minmax, void* stream, uint32_t* route, uint32_t* headers) {
  if (phase < 0 || phase > 2) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (generate_mode != UHDR_HIP_GENERATE_EXACT && generate_mode != UHDR_HIP_GENERATE_LUT &&
      generate_mode != UHDR_HIP_GENERATE_UNFILTERED)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (n <= 0 || yuvs == nullptr || p010s == nullptr || dests == nullptr || metadata == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if ((phase == 0 && route == nullptr) || (phase == 1 && headers == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = check_generate(n, yuvs, p010s, hdr_tf, metadata, dests, 1);   // (n >= 1: validate_generate has seen the transfer function)
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  fill_generate_metadata(hdr_tf, metadata);
  int m = 0;
  uint32_t r[UHDR_HIP_GENERATE_ROUTE_WORDS];
  if (phase == 0) {   // the plan of the first chunk: host arithmetic only, no device state
    rc = generate_chunk(nullptr, nullptr, n, yuvs, p010s, hdr_tf, metadata, dests, sdr_is_601, generate_mode, content_minmax, 0, 0u,
                        &m, r, nullptr);
    if (rc == UHDR_HIP_NO_ERROR) memcpy(route, r, sizeof(r));
    return rc;
  }
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  // one kernel of the pair by itself: only where the call IS one such pair (the workspace is handed from one phase to the other)
  rc = generate_chunk(nullptr, nullptr, n, yuvs, p010s, hdr_tf, metadata, dests, sdr_is_601, generate_mode, content_minmax, 0, 0u,
                      &m, r, nullptr);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (m != n || r[UHDR_HIP_GENERATE_ROUTE_RESOLVE] == 0u) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return generate_chunk(st, static_cast<hipStream_t>(stream), n, yuvs, p010s, hdr_tf, metadata, dests, sdr_is_601, generate_mode,
                        content_minmax, 0, phase == 1 ? kGenPhaseFilter : kGenPhaseResolve, &m, nullptr, headers);
}

// Per-channel (RGB) gain maps: uhdr_hip_generate_gainmap_batch's checks, chunks and metadata; the map is
// RGBA8888 and every chunk one k_generate_rgb launch on the exact path
int uhdr_hip_generate_gainmap_rgb_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                        uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601, void* stream) {
  int rc = check_generate(n, yuvs, p010s, hdr_tf, metadata, dests, 4);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  fill_generate_metadata(hdr_tf, metadata);
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& y0 = yuvs[i];
    const GenConsts c = generate_consts(y0.colorGamut, p010s[i].colorGamut, hdr_tf, sdr_is_601, y0.width, y0.height, *metadata);
    GenBatch b;
    const Chunk ch = gen_chunk(i, n, yuvs, p010s, dests, b, rgba_pair_aligned, 4, true);
    HIP_TRY(launch_generate_rgb(c, b, ch.m, hdr_tf, ch.cls, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// uhdr_hip_apply_gainmap_batch's checks and chunks for RGBA8888 maps (luma_stride in pixels, 0 = width): every chunk one
// k_apply_px_rgb launch, FAST or the unfiltered exact arithmetic
int uhdr_hip_apply_gainmap_rgb_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps, const uhdr_hip_metadata_t* metadata,
                                     int output_format, float max_display_boost, uhdr_hip_image_t* dests, int apply_mode, void* stream) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || maps == nullptr || dests == nullptr)) || metadata == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const int rc = validate_apply(&yuvs[i], &maps[i], metadata, &dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
    if (!al(maps[i].data, 4)) return UHDR_HIP_ERROR_BAD_PTR;
    if (row_stride(maps[i]) < maps[i].width || row_stride(maps[i]) > 0xFFFFFFFFull) return UHDR_HIP_ERROR_INVALID_STRIDE;
  }
  if (apply_mode != UHDR_HIP_APPLY_FAST && apply_mode != UHDR_HIP_APPLY_EXACT)   // (LUT and EXACT_UNFILTERED among the rest)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  DeviceState* st = nullptr;
  const int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool writes = apply_writes(output_format);
  for (int i = 0; i < n; ++i)
    if (writes && dests[i].data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return apply_pixel_chunks(st, s, n, yuvs, maps, *metadata, max_display_boost, dests, true, writes,
                            [&](const AppConsts& c, const AppBatch& b, int m) -> int {
                              HIP_TRY(launch_apply_rgb(c, b, m, output_format, apply_mode == UHDR_HIP_APPLY_EXACT, s));
                              return UHDR_HIP_NO_ERROR;
                            });
}

// ---- content-adaptive generate -----------------------------------------------------------------------
int uhdr_hip_adaptive_boost_range(int hdr_tf, float g_min, float g_max, float* lo, float* hi) {
  if (lo == nullptr || hi == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  adaptive_range(hdr_tf, g_min, g_max, lo, hi);
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_adaptive_metadata(int hdr_tf, float g_min, float g_max, uhdr_hip_metadata_t* metadata) {
  if (metadata == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  float lo, hi;
  const int rc = uhdr_hip_adaptive_boost_range(hdr_tf, g_min, g_max, &lo, &hi);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  fill_adaptive_metadata(lo, hi, metadata);
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_generate_adaptive_workspace_bytes(int n, const uhdr_hip_image_t* yuvs, size_t* bytes) {
  if (n < 0 || (n > 0 && yuvs == nullptr) || bytes == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  *bytes = adaptive_layout(n, yuvs).total;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_generate_gainmap_adaptive_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                             uhdr_hip_image_t* dests, int sdr_is_601, int boost_scope, float* content_minmax,
                                             float* boost_range, void* workspace, size_t workspace_bytes, void* stream) {
  uhdr_hip_metadata_t md;   // (the checks of uhdr_hip_generate_gainmap_batch_ex take one)
  int rc = check_generate(n, yuvs, p010s, hdr_tf, &md, dests, 1);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!valid_boost_scope(boost_scope)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (n > 0 && (boost_range == nullptr || workspace == nullptr || !al(workspace, 16))) return UHDR_HIP_ERROR_BAD_PTR;
  if (workspace_bytes < adaptive_layout(n, yuvs).total) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if (n == 0) return UHDR_HIP_NO_ERROR;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  return adaptive_enqueue(n, yuvs, p010s, hdr_tf, dests, sdr_is_601, boost_scope, content_minmax, boost_range, workspace, nullptr,
                          nullptr, true, static_cast<hipStream_t>(stream));
}

// uhdr_hip_apply_gainmap_batch's checks in front of current_state() ...
static int check_apply(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps, const uhdr_hip_metadata_t* metadata,
                       uhdr_hip_image_t* dests, int apply_mode) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || maps == nullptr || dests == nullptr)) || metadata == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const int rc = validate_apply(&yuvs[i], &maps[i], metadata, &dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
  }
  if (apply_mode != UHDR_HIP_APPLY_FAST && apply_mode != UHDR_HIP_APPLY_EXACT && apply_mode != UHDR_HIP_APPLY_LUT &&
      apply_mode != UHDR_HIP_APPLY_EXACT_UNFILTERED)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return UHDR_HIP_NO_ERROR;
}
// ... and the one behind current_state()
static int check_apply_dests(int n, const uhdr_hip_image_t* dests, int output_format) {
  const bool writes = apply_writes(output_format);
  for (int i = 0; i < n; ++i)
    if (writes && dests[i].data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  return UHDR_HIP_NO_ERROR;
}

// One chunk of uhdr_hip_apply_gainmap_batch: up to kMaxChunk consecutive images, from image i on, of one size, map size and class
// (app_chunk); *m_out receives their number.  `phases` selects which kernels of EXACT's pair are enqueued (launch_apply's ex_phases;
// every other route is one launch, enqueued when phases != 0); the production call passes both.  0 enqueues nothing and needs no
// device (st may be null): the plan only -- `route` (or null) receives it, UHDR_HIP_APPLY_ROUTE_* words.  `headers` (or null; device,
// kExHdrWords words per image): behind kExPhaseEst on the pair's route, every image's header words, copied in stream order.
static int apply_chunk(DeviceState* st, hipStream_t s, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps,
                       const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost, uhdr_hip_image_t* dests,
                       int apply_mode, int i, unsigned phases, int* m_out, uint32_t* route, uint32_t* headers) {
  const uhdr_hip_image_t& y0 = yuvs[i];
  const uhdr_hip_image_t& m0 = maps[i];
  const bool writes = apply_writes(output_format);
  IdwLease table;
  int rc;
  if (phases != 0u && (rc = table.take(st, (int)(y0.width / m0.width), s)) != UHDR_HIP_NO_ERROR) return rc;
  AppConsts c = apply_consts(y0, m0, *metadata, max_display_boost, table.idw);
  c.lut = (apply_mode == UHDR_HIP_APPLY_LUT && st != nullptr) ? st->lut : nullptr;
  c.tab = st != nullptr ? st->lut : nullptr;
  AppBatch b;
  const Chunk ch = app_chunk(i, n, yuvs, maps, dests, b, &c, false);   // (the descriptors are filled in the plan-only mode too)
  const int m = ch.m;
  const bool fast = ch.cls;
  *m_out = m;
  // EXACT: f32 estimate, then the exact path on the pixels it leaves in doubt.  The estimate's error bounds are measured for
  // |log2 boost| <= 32 (tests/test_gpu_exact_filter.py); beyond that every pixel takes the exact path.
  const bool pair = writes && apply_mode == UHDR_HIP_APPLY_EXACT && (uint64_t)c.width * c.height <= 0xFFFFFFFFull &&
                    std::fabs(c.log2_min_d) <= 32.0 && std::fabs(c.log2_max_d) <= 32.0;
  const uint32_t cap = pair ? ex_list_cap((uint64_t)c.width * c.height) : 0u;
  if (route != nullptr) {
    memset(route, 0, sizeof(uint32_t) * UHDR_HIP_APPLY_ROUTE_WORDS);
    uint32_t grid[2] = {0u, 0u};
    if (pair) apply_est_grid(c, m, fast, grid);
    route[UHDR_HIP_APPLY_ROUTE_RESOLVE] = pair ? 1u : 0u;
    route[UHDR_HIP_APPLY_ROUTE_CELLS] = (pair && fast) ? 1u : 0u;
    route[UHDR_HIP_APPLY_ROUTE_IMAGES] = (uint32_t)m;
    route[UHDR_HIP_APPLY_ROUTE_LISTS] = kExLists;
    route[UHDR_HIP_APPLY_ROUTE_LIST_CAP] = cap;
    route[UHDR_HIP_APPLY_ROUTE_HDR_WORDS] = kExHdrWords;
    route[UHDR_HIP_APPLY_ROUTE_LIST_COUNTS] = 8u;   // AppConsts::ex_ws: words 8 ..: the lengths of the image's lists,
    route[UHDR_HIP_APPLY_ROUTE_SLICE_WORD] = 3u;    // word 3: slices of k_apply_resolve that have finished
    route[UHDR_HIP_APPLY_ROUTE_RESOLVE_SLICES] = kExSlices;
    route[UHDR_HIP_APPLY_ROUTE_GRID_X] = grid[0];
    route[UHDR_HIP_APPLY_ROUTE_GRID_Y] = grid[1];
  }
  if (phases == 0u) return UHDR_HIP_NO_ERROR;
  std::unique_lock<std::mutex> pair_lk(g_pair_mu, std::defer_lock);
  if (pair) {
    pair_lk.lock();
    uint32_t* w = nullptr;
    const int wrc = exact_workspace(st, s, m, cap, &w);
    if (wrc != UHDR_HIP_NO_ERROR) return wrc;
    c.ex_ws = w;
    c.ex_cap = cap;
  }
  if (writes) HIP_TRY(launch_apply(c, b, m, output_format, apply_mode, fast, s, phases));
  if (pair && headers != nullptr && (phases & kExPhaseEst))   // (the headers of a launch's images lie side by side in front)
    HIP_TRY(hipMemcpyAsync(headers, c.ex_ws, sizeof(uint32_t) * kExHdrWords * (size_t)m, hipMemcpyDeviceToDevice, s));
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_apply_gainmap_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps,
                                 const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                                 uhdr_hip_image_t* dests, int apply_mode, void* stream) {
  int rc = check_apply(n, yuvs, maps, metadata, dests, apply_mode);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = check_apply_dests(n, dests, output_format)) != UHDR_HIP_NO_ERROR) return rc;

  int i = 0;
  while (i < n) {
    int m = 0;
    rc = apply_chunk(st, s, n, yuvs, maps, metadata, output_format, max_display_boost, dests, apply_mode, i,
                     kExPhaseEst | kExPhaseResolve, &m, nullptr, nullptr);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
    i += m;
  }
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_apply_exact_probe(int phase, int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps,
                               const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                               uhdr_hip_image_t* dests, void* stream, uint32_t* route, uint32_t* headers) {
  if (phase < 0 || phase > 2) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (n <= 0) return UHDR_HIP_ERROR_BAD_PTR;
  if ((phase == 0 && route == nullptr) || (phase == 1 && headers == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = check_apply(n, yuvs, maps, metadata, dests, UHDR_HIP_APPLY_EXACT);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if (phase != 0 && (rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  if ((rc = check_apply_dests(n, dests, output_format)) != UHDR_HIP_NO_ERROR) return rc;
  int m = 0;
  uint32_t r[UHDR_HIP_APPLY_ROUTE_WORDS];
  // the plan of the first chunk: host arithmetic only, no device state.  Phases 1 and 2 take it first as well: it is what tells them
  // that the call spans several chunks or is not on the pair's route, before anything is enqueued
  rc = apply_chunk(nullptr, nullptr, n, yuvs, maps, metadata, output_format, max_display_boost, dests, UHDR_HIP_APPLY_EXACT, 0, 0u, &m, r,
                   nullptr);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (phase == 0) {
    memcpy(route, r, sizeof(r));
    return UHDR_HIP_NO_ERROR;
  }
  // one kernel of the pair by itself: only where the call IS one such pair (the workspace is handed from one phase to the other)
  if (m != n || r[UHDR_HIP_APPLY_ROUTE_RESOLVE] == 0u) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return apply_chunk(st, static_cast<hipStream_t>(stream), n, yuvs, maps, metadata, output_format, max_display_boost, dests,
                     UHDR_HIP_APPLY_EXACT, 0, phase == 1 ? kExPhaseEst : kExPhaseResolve, &m, nullptr, headers);
}

// ---- general metadata: gamma, offsets, HDR capacity ---------------------------
int uhdr_hip_gainmap_weight(const uhdr_hip_metadata_t* metadata, float max_display_boost, float* weight, float* display_boost) {
  if (metadata == nullptr || weight == nullptr || display_boost == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const int rc = validate_md(metadata);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!(max_display_boost >= 1.0f)) return UHDR_HIP_ERROR_INVALID_DISPLAY_BOOST;
  double w, d;
  md_weight(*metadata, max_display_boost, &w, &d);
  *weight = (float)w;
  *display_boost = (float)d;
  return UHDR_HIP_NO_ERROR;
}

// Degenerate metadata: the existing call of the maps' form, with its checks, routes and bytes.  General metadata:
// uhdr_hip_apply_gainmap_rgb_batch's chunks (equal sizes and map strides share a launch), every chunk one k_apply_px_md launch.
int uhdr_hip_apply_gainmap_md_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* maps, const uhdr_hip_metadata_t* metadata,
                                    int output_format, float max_display_boost, uhdr_hip_image_t* dests, int apply_mode, void* stream) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || maps == nullptr || dests == nullptr)) || metadata == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i)
    if (yuvs[i].data == nullptr || yuvs[i].chroma_data == nullptr || maps[i].data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = validate_md(metadata);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!(max_display_boost >= 1.0f)) return UHDR_HIP_ERROR_INVALID_DISPLAY_BOOST;
  const int form = n > 0 ? maps[0].pixelFormat : UHDR_HIP_PIX_FMT_MONOCHROME;
  if (form != UHDR_HIP_PIX_FMT_MONOCHROME && form != UHDR_HIP_PIX_FMT_UNSPECIFIED && form != UHDR_HIP_PIX_FMT_RGBA8888)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  const bool rgb = form == UHDR_HIP_PIX_FMT_RGBA8888;
  if (md_degenerate(*metadata))
    return rgb ? uhdr_hip_apply_gainmap_rgb_batch(n, yuvs, maps, metadata, output_format, max_display_boost, dests, apply_mode, stream)
               : uhdr_hip_apply_gainmap_batch(n, yuvs, maps, metadata, output_format, max_display_boost, dests, apply_mode, stream);
  // a one-plane map's rows are `width` bytes, an RGBA map's luma_stride pixels (0 = width)
  for (int i = 0; i < n; ++i) {   // validate_apply's scale-factor checks, then uhdr_hip_apply_gainmap_rgb_batch's of the map
    const uhdr_hip_image_t& y = yuvs[i];
    const uhdr_hip_image_t& mp = maps[i];
    if (mp.width == 0 || mp.height == 0) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
    if (y.width % mp.width != 0 || y.height % mp.height != 0) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
    if (y.width * mp.height != y.height * mp.width) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
    if (rgb && !al(mp.data, 4)) return UHDR_HIP_ERROR_BAD_PTR;
    if (rgb && (row_stride(mp) < mp.width || row_stride(mp) > 0xFFFFFFFFull)) return UHDR_HIP_ERROR_INVALID_STRIDE;
  }
  // FAST and EXACT select the one arithmetic there is: EXACT promises the reference's bytes, and the reference refuses this metadata
  if (apply_mode != UHDR_HIP_APPLY_FAST && apply_mode != UHDR_HIP_APPLY_EXACT) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool writes = apply_writes(output_format);
  for (int i = 0; i < n; ++i)
    if (writes && dests[i].data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const AppMdConsts mc = apply_md_consts(*metadata, max_display_boost);
  return apply_pixel_chunks(st, s, n, yuvs, maps, *metadata, max_display_boost, dests, rgb, writes,
                            [&](const AppConsts& c, const AppBatch& b, int m) -> int {
                              HIP_TRY(launch_apply_md(c, mc, b, m, output_format, rgb, s));
                              return UHDR_HIP_NO_ERROR;
                            });
}

// HDR from a packed SDR image and its gain map.  Chunks: consecutive images of one size, map size and (RGBA
// maps) map stride whose rows are all 16-byte aligned at scale factor 4 (the strip form) or not (one pixel per lane); every chunk one
// k_apply_packed_s4 / k_apply_packed_px launch.  The checks are in the header's order.
int uhdr_hip_apply_gainmap_packed_batch(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* maps, const uhdr_hip_metadata_t* metadata,
                                        int output_format, float max_display_boost, uhdr_hip_image_t* dests, int apply_mode, void* stream) {
  if (n < 0 || (n > 0 && (sdrs == nullptr || maps == nullptr || dests == nullptr)) || metadata == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  auto one_plane = [](int f) { return f == UHDR_HIP_PIX_FMT_MONOCHROME || f == UHDR_HIP_PIX_FMT_UNSPECIFIED; };
  const bool rgb = n > 0 && maps[0].pixelFormat == UHDR_HIP_PIX_FMT_RGBA8888;
  for (int i = 0; i < n; ++i) {
    if (sdrs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA8888) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (!(rgb ? maps[i].pixelFormat == UHDR_HIP_PIX_FMT_RGBA8888 : one_plane(maps[i].pixelFormat))) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  }
  const bool writes = apply_writes(output_format);
  for (int i = 0; i < n; ++i) {
    if (sdrs[i].data == nullptr || maps[i].data == nullptr || dests[i].data == nullptr || !al(sdrs[i].data, 4) || (rgb && !al(maps[i].data, 4)))
      return UHDR_HIP_ERROR_BAD_PTR;
    // (a pixel of the output is one store: RGBA F16 8 bytes, RGBA1010102 4, a planar sample 2)
    if (writes && !al(dests[i].data, output_format == UHDR_HIP_OUTPUT_HDR_LINEAR ? 8 : output_format == UHDR_HIP_OUTPUT_HDR_LINEAR_RGB_10BIT ? 2 : 4))
      return UHDR_HIP_ERROR_BAD_PTR;
  }
  int rc = validate_md(metadata);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!(max_display_boost >= 1.0f)) return UHDR_HIP_ERROR_INVALID_DISPLAY_BOOST;
  if (!writes) return UHDR_HIP_ERROR_INVALID_OUTPUT_FORMAT;
  const bool general = !md_degenerate(*metadata);
  // degenerate metadata: every pixel takes the exact path, so EXACT and EXACT_UNFILTERED are one kernel; general metadata: one f32
  // arithmetic under FAST and EXACT, as in uhdr_hip_apply_gainmap_md_batch
  if (apply_mode != UHDR_HIP_APPLY_FAST && apply_mode != UHDR_HIP_APPLY_EXACT && (general || apply_mode != UHDR_HIP_APPLY_EXACT_UNFILTERED))
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  for (int i = 0; i < n; ++i) {
    const uhdr_hip_image_t& sd = sdrs[i];
    const uhdr_hip_image_t& mp = maps[i];
    if (row_stride(sd) < sd.width || row_stride(sd) > 0xFFFFFFFFull) return UHDR_HIP_ERROR_INVALID_STRIDE;
    if (rgb && (row_stride(mp) < mp.width || row_stride(mp) > 0xFFFFFFFFull)) return UHDR_HIP_ERROR_INVALID_STRIDE;
    if (mp.width == 0 || mp.height == 0) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;   // validate_apply's scale-factor checks
    if (sd.width % mp.width != 0 || sd.height % mp.height != 0) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
    if (sd.width * mp.height != sd.height * mp.width) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
  }
  if (n == 0) return UHDR_HIP_NO_ERROR;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const AppMdConsts mc = apply_md_consts(*metadata, max_display_boost);
  const int kind = general ? (mc.gamma_on != 0u ? kPackedMdGamma : kPackedMd) : (apply_mode == UHDR_HIP_APPLY_FAST ? kPackedFast : kPackedExact);
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& s0 = sdrs[i];
    const uhdr_hip_image_t& m0 = maps[i];
    IdwLease table;
    if ((rc = table.take(st, (int)(s0.width / m0.width), s)) != UHDR_HIP_NO_ERROR) return rc;
    AppConsts c = apply_consts(s0, m0, *metadata, max_display_boost, table.idw);
    c.map_stride = (uint32_t)(rgb ? row_stride(m0) : m0.width);
    PackedAppBatch b;
    const Chunk ch = form_chunk(i, n, kMaxChunk,
                                [&](int j) {
                                  return sdrs[j].width == s0.width && sdrs[j].height == s0.height && maps[j].width == m0.width &&
                                         maps[j].height == m0.height && (!rgb || row_stride(maps[j]) == row_stride(m0));
                                },
                                [&](int j, int m) {
                                  PackedAppImage& p = b.img[m];
                                  p.sdr = static_cast<const uint32_t*>(sdrs[j].data);
                                  p.map = static_cast<const uint8_t*>(maps[j].data);
                                  p.dst = dests[j].data;
                                  p.sdr_stride = (uint32_t)row_stride(sdrs[j]);
                                  p.pad_ = 0u;
                                  // the strip form: a lane's four pixels are one 16-byte load and leave as 16-byte (planar: 8-byte) stores
                                  return c.scale == 4u && c.width % 4u == 0u && al(p.sdr, 16) && p.sdr_stride % 4u == 0u && al(p.dst, 16);
                                });
    for (int k = 0; k < ch.m; ++k) fill_apply_dest(&sdrs[i + k], &dests[i + k]);
    HIP_TRY(launch_apply_packed(c, mc, b, st->srgb_codes, ch.m, output_format, kind, rgb, ch.cls, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// uhdr_hip_generate_gainmap_rgb_batch's chunks; every chunk one k_generate_md launch on the exact path
int uhdr_hip_generate_gainmap_md_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                       const uhdr_hip_metadata_t* md_in, uhdr_hip_image_t* dests, int sdr_is_601, int rgb, void* stream) {
  int rc = check_generate_md(n, yuvs, p010s, hdr_tf, md_in, dests, rgb != 0 ? 4 : 1);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& y0 = yuvs[i];
    const GenConsts c = generate_consts(y0.colorGamut, p010s[i].colorGamut, hdr_tf, sdr_is_601, y0.width, y0.height, *md_in);
    const GenMdConsts mc = generate_md_consts(*md_in, c);
    GenBatch b;
    const Chunk ch = gen_chunk(i, n, yuvs, p010s, dests, b, rgb != 0 ? rgba_pair_aligned : no_more, 4, rgb != 0);
    HIP_TRY(launch_generate_md(c, mc, b, ch.m, hdr_tf, ch.cls, rgb != 0, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// uhdr_hip_generate_gainmap_packed_batch's checks, in the header's order; *f16: the HDR images are RGBA F16
static int check_generate_packed(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, int hdr_tf, const uhdr_hip_metadata_t* md_in,
                                 const uhdr_hip_image_t* dests, int rgb, bool* f16_out) {
  if (n < 0 || (n > 0 && (sdrs == nullptr || hdrs == nullptr || dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    if (sdrs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA8888) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (hdrs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA1010102 && hdrs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA_F16) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (hdrs[i].pixelFormat != hdrs[0].pixelFormat) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  }
  const bool f16 = n > 0 && hdrs[0].pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16;
  for (int i = 0; i < n; ++i) {
    if (sdrs[i].data == nullptr || hdrs[i].data == nullptr || dests[i].data == nullptr || !al(sdrs[i].data, 4) ||
        !al(hdrs[i].data, f16 ? 8 : 4) || (rgb != 0 && !al(dests[i].data, 4)))
      return UHDR_HIP_ERROR_BAD_PTR;
  }
  int rc;
  if (md_in != nullptr && (rc = validate_md(md_in)) != UHDR_HIP_NO_ERROR) return rc;
  for (int i = 0; i < n; ++i) {   // validate_generate's order around the packed images' own checks
    const uhdr_hip_image_t& sd = sdrs[i];
    const uhdr_hip_image_t& hd = hdrs[i];
    if (row_stride(sd) < sd.width || row_stride(hd) < hd.width || row_stride(sd) > 0xFFFFFFFFull || row_stride(hd) > 0xFFFFFFFFull)
      return UHDR_HIP_ERROR_INVALID_STRIDE;
    if (sd.width != hd.width || sd.height != hd.height) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
    if (sd.colorGamut == UHDR_HIP_CG_UNSPECIFIED || hd.colorGamut == UHDR_HIP_CG_UNSPECIFIED) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
    if (f16 ? hdr_tf != UHDR_HIP_TF_LINEAR : (hdr_tf != UHDR_HIP_TF_HLG && hdr_tf != UHDR_HIP_TF_PQ)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
    if (!valid_gamut(sd.colorGamut) || !valid_gamut(hd.colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  }
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  *f16_out = f16;
  return UHDR_HIP_NO_ERROR;
}

// Packed RGBA inputs: uhdr_hip_generate_gainmap_md_batch's chunks over an RGBA8888 SDR image and an
// RGBA1010102 / RGBA F16 HDR image; every chunk one k_generate_packed launch on the exact path
int uhdr_hip_generate_gainmap_packed_batch(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, int hdr_tf,
                                           const uhdr_hip_metadata_t* md_in, uhdr_hip_metadata_t* md_out, uhdr_hip_image_t* dests, int rgb,
                                           void* stream) {
  bool f16 = false;
  int rc = check_generate_packed(n, sdrs, hdrs, hdr_tf, md_in, dests, rgb, &f16);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uhdr_hip_metadata_t md;
  if (md_in != nullptr) md = *md_in;
  else fill_generate_metadata(hdr_tf, &md);
  if (md_out != nullptr) *md_out = md;
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& s0 = sdrs[i];
    const GenConsts c = generate_consts(s0.colorGamut, hdrs[i].colorGamut, hdr_tf, 0, s0.width, s0.height, md);
    const GenMdConsts mc = generate_md_consts(md, c);
    PackedBatch b;
    // (the pair's bytes are one store)
    const Chunk ch = packed_chunk(i, n, sdrs, hdrs, f16, b, [&](int j) { return dests[j].data; }, rgb != 0 ? 8 : 2);
    for (int k = 0; k < ch.m; ++k) fill_generate_dest(&sdrs[i + k], &dests[i + k], 4, rgb != 0);
    HIP_TRY(launch_generate_packed(c, mc, b, ch.m, hdr_tf, f16, ch.cls, rgb != 0, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// ---- content-adaptive maps from packed RGBA -------------------------------
int uhdr_hip_generate_packed_adaptive_workspace_bytes(int n, const uhdr_hip_image_t* sdrs, int rgb, size_t* bytes) {
  if (bytes == nullptr || n < 0 || (n > 0 && sdrs == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  *bytes = adaptive_layout(n, sdrs, packed_gain_bytes(rgb != 0)).total;
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_generate_gainmap_packed_adaptive_batch(int n, const uhdr_hip_image_t* sdrs, const uhdr_hip_image_t* hdrs, int hdr_tf,
                                                    uhdr_hip_image_t* dests, int rgb, int boost_scope, float* content_minmax,
                                                    float* boost_range, void* workspace, size_t workspace_bytes, void* stream) {
  bool f16 = false;
  int rc = check_generate_packed(n, sdrs, hdrs, hdr_tf, nullptr, dests, rgb, &f16);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!valid_boost_scope(boost_scope)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (n > 0 && (workspace == nullptr || !al(workspace, 16) || boost_range == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  if (workspace_bytes < adaptive_layout(n, sdrs, packed_gain_bytes(rgb != 0)).total) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if (n == 0) return UHDR_HIP_NO_ERROR;   // (nothing to enqueue: no device is asked for)
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  return packed_adaptive_enqueue(n, sdrs, hdrs, hdr_tf, dests, rgb != 0, boost_scope, content_minmax, boost_range, workspace, nullptr, nullptr,
                                 true, static_cast<hipStream_t>(stream));
}

// Gain maps at any scale factor: the checks of the call whose arithmetic is selected, in its order, with the
// factor's own behind the call-level BAD_PTR and behind every image's; factor 4 IS those calls; every chunk one k_generate_scaled launch
// doubt_count: null, or the probe's device word
static int generate_scaled(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf, const uhdr_hip_metadata_t* md_in,
                           uhdr_hip_metadata_t* md_out, uhdr_hip_image_t* dests, int sdr_is_601, int rgb, int map_scale_factor, void* stream,
                           uint32_t* doubt_count) {
  if (n < 0 || (n > 0 && (yuvs == nullptr || p010s == nullptr || dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  if (map_scale_factor < 1 || map_scale_factor > 128) return UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR;
  const size_t sf = (size_t)map_scale_factor;
  int rc;
  if (map_scale_factor == 4) {
    uhdr_hip_metadata_t md;
    if (md_in != nullptr) {
      md = *md_in;
      rc = uhdr_hip_generate_gainmap_md_batch(n, yuvs, p010s, hdr_tf, md_in, dests, sdr_is_601, rgb, stream);
    } else if (rgb != 0) {
      rc = uhdr_hip_generate_gainmap_rgb_batch(n, yuvs, p010s, hdr_tf, &md, dests, sdr_is_601, stream);
    } else {
      rc = uhdr_hip_generate_gainmap_batch(n, yuvs, p010s, hdr_tf, &md, dests, sdr_is_601, nullptr, stream);
    }
    if (rc == UHDR_HIP_NO_ERROR && md_out != nullptr) *md_out = md;
    return rc;
  }
  // the image has no map pixel at this factor
  const ImageHook too_small = [sf](const uhdr_hip_image_t& y) {
    return y.width / sf == 0 || y.height / sf == 0 ? UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR : UHDR_HIP_NO_ERROR;
  };
  uhdr_hip_metadata_t md;
  if (md_in != nullptr) md = *md_in;
  rc = md_in != nullptr ? check_generate_md(n, yuvs, p010s, hdr_tf, md_in, dests, rgb != 0 ? 4 : 1, too_small)
                        : check_generate(n, yuvs, p010s, hdr_tf, &md, dests, rgb != 0 ? 4 : 1, too_small);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (md_in == nullptr) fill_generate_metadata(hdr_tf, &md);
  if (md_out != nullptr) *md_out = md;
  GenScaleConsts sc;
  sc.s = (uint32_t)map_scale_factor;
  sc.area = (float)(map_scale_factor * map_scale_factor);
  sc.doubt_count = doubt_count;
  const uint32_t strip = (sc.s == 1u || sc.s == 2u || sc.s == 8u) ? 8u / sc.s : 0u;   // map pixels a thread of the aligned forms stores at once
  const size_t strip_bytes = (size_t)strip * (rgb != 0 ? 4u : 1u);
  int i = 0;
  while (i < n) {
    const uhdr_hip_image_t& y0 = yuvs[i];
    GenConsts c = generate_consts(y0.colorGamut, p010s[i].colorGamut, hdr_tf, sdr_is_601, y0.width, y0.height, md);
    c.map_w = (uint32_t)(y0.width / sf);
    c.map_h = (uint32_t)(y0.height / sf);
    const GenMdConsts mc = generate_md_consts(md, c);
    // the reference's metadata and one channel: the filtered kernel, where the filter's bounds hold (they start from the sampled values,
    // so generate_consts' flt_* constants serve every factor)
    const bool filter = md_in == nullptr && rgb == 0 && c.flt_delta < 0.25f && c.min_boost >= 0.25f && c.max_boost <= 64.0f;
    const int mode = filter ? 0 : (rgb != 0 ? 2 : 1);
    GenBatch b;
    const Chunk ch = gen_chunk(i, n, yuvs, p010s, dests, b,
                               [&](const GenImage& g) { return strip != 0u && c.height % 2u == 0 && al(g.map, strip_bytes > 8u ? 8u : strip_bytes); },
                               sf, rgb != 0);
    HIP_TRY(launch_generate_scaled(c, mc, sc, b, ch.m, hdr_tf, ch.cls, mode, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}
int uhdr_hip_generate_gainmap_scaled_batch(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                           const uhdr_hip_metadata_t* md_in, uhdr_hip_metadata_t* md_out, uhdr_hip_image_t* dests,
                                           int sdr_is_601, int rgb, int map_scale_factor, void* stream) {
  return generate_scaled(n, yuvs, p010s, hdr_tf, md_in, md_out, dests, sdr_is_601, rgb, map_scale_factor, stream, nullptr);
}
// the same call, counting: *doubt_count (a device word the caller has cleared) grows by the map pixels the f32 pre-filter left to the
// exact path.  Only the filtered form counts (metadata_in == NULL, rgb == 0, a factor other than 4)
int uhdr_hip_generate_gainmap_scaled_probe(int n, const uhdr_hip_image_t* yuvs, const uhdr_hip_image_t* p010s, int hdr_tf,
                                           uhdr_hip_image_t* dests, int sdr_is_601, int map_scale_factor, uint32_t* doubt_count, void* stream) {
  if (doubt_count == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (map_scale_factor == 4) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  return generate_scaled(n, yuvs, p010s, hdr_tf, nullptr, nullptr, dests, sdr_is_601, 0, map_scale_factor, stream, doubt_count);
}

// ---------------------------------------------------------------------------------------------------
int uhdr_hip_generate_gainmap(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* p010, int hdr_tf,
                              uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest, int sdr_is_601, int mem_space,
                              void* stream) {
  return uhdr_hip_generate_gainmap_ex(yuv, p010, hdr_tf, metadata, dest, sdr_is_601, UHDR_HIP_GENERATE_EXACT, mem_space, stream);
}

int uhdr_hip_generate_gainmap_ex(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* p010, int hdr_tf,
                                 uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest, int sdr_is_601, int generate_mode,
                                 int mem_space, void* stream) {
  int rc = validate_generate(yuv, p010, hdr_tf, metadata, dest);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (dest->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (mem_space == UHDR_HIP_MEM_DEVICE)
    return uhdr_hip_generate_gainmap_batch_ex(1, yuv, p010, hdr_tf, metadata, dest, sdr_is_601, generate_mode, nullptr, stream);

  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  StageLease lease(st);
  StageSet* ss = lease.get();
  if (ss == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = generate_through_stage(ss, yuv, p010, dest, s, [&](const uhdr_hip_image_t& dy, const uhdr_hip_image_t& dp, uhdr_hip_image_t& dm) {
    return uhdr_hip_generate_gainmap_batch_ex(1, &dy, &dp, hdr_tf, metadata, &dm, sdr_is_601, generate_mode, nullptr, stream);
  });
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  fill_generate_dest(yuv, dest);
  return UHDR_HIP_NO_ERROR;
}

// one image through the adaptive batch, the measured metadata back on the host: the call waits for the stream in either memory space
int uhdr_hip_generate_gainmap_adaptive(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* p010, int hdr_tf,
                                       uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest, int sdr_is_601, int mem_space,
                                       void* stream) {
  int rc = validate_generate(yuv, p010, hdr_tf, metadata, dest);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (dest->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  StageLease lease(st);
  StageSet* ss = lease.get();
  if (ss == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* dev_range = nullptr;
  auto run = [&](const uhdr_hip_image_t& dy, const uhdr_hip_image_t& dp, uhdr_hip_image_t& dm) {
    const size_t ws_bytes = adaptive_layout(1, &dy).total;
    const int wrc = stage_reserve(ss, 5, ws_bytes + 256);
    if (wrc != 0) return wrc;
    uint8_t* ws = static_cast<uint8_t*>(ss->stage[5]);
    dev_range = reinterpret_cast<float*>(ws + ws_bytes);
    return adaptive_enqueue(1, &dy, &dp, hdr_tf, &dm, sdr_is_601, UHDR_HIP_BOOST_PER_IMAGE, nullptr, dev_range, ws, nullptr, nullptr, true, s);
  };
  uhdr_hip_image_t dm = *dest;
  rc = mem_space != UHDR_HIP_MEM_DEVICE ? generate_through_stage(ss, yuv, p010, dest, s, run) : run(*yuv, *p010, dm);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  float range[2];
  HIP_TRY(hipMemcpyAsync(range, dev_range, sizeof(range), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  fill_adaptive_metadata(range[0], range[1], metadata);
  fill_generate_dest(yuv, dest);
  return UHDR_HIP_NO_ERROR;
}

// one packed pair in device memory through the packed adaptive batch, the workspace the library's, the measured metadata back on the
// host: the call waits for the stream
int uhdr_hip_generate_gainmap_packed_adaptive(const uhdr_hip_image_t* sdr, const uhdr_hip_image_t* hdr, int hdr_tf, uhdr_hip_metadata_t* metadata,
                                              uhdr_hip_image_t* dest, int rgb, void* stream) {
  if (sdr == nullptr || hdr == nullptr || metadata == nullptr || dest == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  bool f16 = false;
  int rc = check_generate_packed(1, sdr, hdr, hdr_tf, nullptr, dest, rgb, &f16);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  StageLease lease(st);
  StageSet* ss = lease.get();
  if (ss == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t ws_bytes = adaptive_layout(1, sdr, packed_gain_bytes(rgb != 0)).total;
  if ((rc = stage_reserve(ss, 5, ws_bytes + 256)) != 0) return rc;
  uint8_t* ws = static_cast<uint8_t*>(ss->stage[5]);
  float* dev_range = reinterpret_cast<float*>(ws + ws_bytes);
  if ((rc = packed_adaptive_enqueue(1, sdr, hdr, hdr_tf, dest, rgb != 0, UHDR_HIP_BOOST_PER_IMAGE, nullptr, dev_range, ws, nullptr, nullptr, true,
                                    s)) != UHDR_HIP_NO_ERROR)
    return rc;
  float range[2];
  HIP_TRY(hipMemcpyAsync(range, dev_range, sizeof(range), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  fill_adaptive_metadata(range[0], range[1], metadata);
  return UHDR_HIP_NO_ERROR;
}

int uhdr_hip_apply_gainmap(const uhdr_hip_image_t* yuv, const uhdr_hip_image_t* map, const uhdr_hip_metadata_t* metadata,
                           int output_format, float max_display_boost, uhdr_hip_image_t* dest, int apply_mode,
                           int mem_space, void* stream) {
  int rc = validate_apply(yuv, map, metadata, dest);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (mem_space == UHDR_HIP_MEM_DEVICE)
    return uhdr_hip_apply_gainmap_batch(1, yuv, map, metadata, output_format, max_display_boost, dest, apply_mode, stream);

  const bool writes = apply_writes(output_format);
  if (writes && dest->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  StageLease lease(st);
  StageSet* ss = lease.get();
  if (ss == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uhdr_hip_image_t dy, dm = *map, dd = *dest;
  if ((rc = stage_ycbcr_in(ss, 0, *yuv, &dy, s)) != 0) return rc;
  const size_t map_bytes = map->width * map->height;  // the reference reads the map with stride == width
  if ((rc = stage_reserve(ss, 4, map_bytes)) != 0) return rc;
  HIP_TRY(hipMemcpyAsync(ss->stage[4], map->data, map_bytes, hipMemcpyHostToDevice, s));
  dm.data = ss->stage[4];
  const size_t out_bytes = writes ? yuv->width * yuv->height * apply_bpp(output_format) : 0;
  if ((rc = stage_reserve(ss, 5, out_bytes)) != 0) return rc;
  dd.data = ss->stage[5];
  rc = uhdr_hip_apply_gainmap_batch(1, &dy, &dm, metadata, output_format, max_display_boost, &dd, apply_mode, stream);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (out_bytes) HIP_TRY(hipMemcpyAsync(dest->data, dd.data, out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  fill_apply_dest(yuv, dest);
  return UHDR_HIP_NO_ERROR;
}

namespace {
ToneImage tone_image(const uhdr_hip_image_t& sd, const uhdr_hip_image_t& dd, bool* aligned) {
  ToneImage t;
  t.sy = static_cast<const uint16_t*>(sd.data);
  t.suv = static_cast<const uint16_t*>(sd.chroma_data);
  t.dy = static_cast<uint8_t*>(dd.data);
  t.du = static_cast<uint8_t*>(dd.chroma_data);
  t.dv = t.du + (dd.chroma_stride * dd.height / 2);  // ultrahdr.cpp:539
  t.sy_stride = (uint32_t)sd.luma_stride; t.suv_stride = (uint32_t)sd.chroma_stride;
  t.dy_stride = (uint32_t)dd.luma_stride; t.dc_stride = (uint32_t)dd.chroma_stride;
  t.width = (uint32_t)sd.width; t.height = (uint32_t)sd.height;
  *aligned = t.width % 16u == 0 && al(t.sy, 16) && t.sy_stride % 8u == 0 && al(t.suv, 16) &&
             t.suv_stride % 8u == 0 && al(t.dy, 8) && t.dy_stride % 8u == 0 && t.dy_stride >= t.width &&
             al(t.du, 8) && al(t.dv, 8) && t.dc_stride % 8u == 0 && t.dc_stride >= t.width / 2u;
  return t;
}
int tonemap_check(const uhdr_hip_image_t* src, const uhdr_hip_image_t* dest) {   // ultrahdr.cpp:518-523
  if (src == nullptr || dest == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (src->width != dest->width || src->height != dest->height) return UHDR_HIP_ERROR_RESOLUTION_MISMATCH;
  if (src->data == nullptr || src->chroma_data == nullptr || dest->data == nullptr || dest->chroma_data == nullptr)
    return UHDR_HIP_ERROR_BAD_PTR;  // (the reference would dereference them)
  return UHDR_HIP_NO_ERROR;
}
// The frame of the single tone-map and convertYuv calls: one image in either memory space through its batch of one, and the headroom
// H, where the operator has one (with_head), back on the host.  A context is leased and, for H, 256 bytes of its slot 4 reserved;
// in host memory stage_in(ss, &sd, &dd) stages the image and reserves its destination; run(source, destination, device H) is the
// batch of one on the staged descriptors (device memory: on the caller's own, sd and dd are not used); in host memory
// copy_back(dd) enqueues what the call returns; H is read once, the stream waited for, and in host memory fill() completes the
// caller's descriptor (device memory: the batch has).
extern "C++" {   // (a template: this part of the file lies inside extern "C")
template <class StageIn, class Run, class CopyBack, class Fill>
int single_call(const uhdr_hip_image_t* src, uhdr_hip_image_t* dest, bool host, bool with_head, float* headroom, hipStream_t s,
                StageIn stage_in, Run run, CopyBack copy_back, Fill fill) {
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  StageLease lease(st);
  StageSet* ss = lease.get();
  if (ss == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  if (with_head && (rc = stage_reserve(ss, 4, 256)) != 0) return rc;
  float* dh = with_head ? static_cast<float*>(ss->stage[4]) : nullptr;
  uhdr_hip_image_t sd, dd;
  if (host && (rc = stage_in(ss, &sd, &dd)) != 0) return rc;
  if ((rc = host ? run(&sd, &dd, dh) : run(src, dest, dh)) != UHDR_HIP_NO_ERROR) return rc;
  if (host && (rc = copy_back(dd)) != 0) return rc;
  float h_out = 0.0f;
  if (with_head) HIP_TRY(hipMemcpyAsync(&h_out, dh, sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (host) fill();
  if (with_head && headroom) *headroom = h_out;
  return UHDR_HIP_NO_ERROR;
}
}  // extern "C++"
// A toneMap's host planes, for both operators: the P010 planes staged into slots 2 and 3 of `ss`, destination planes in slots 0
// and 1 ...
int stage_tonemap_in(StageSet* ss, const uhdr_hip_image_t& src, const uhdr_hip_image_t& dest, uhdr_hip_image_t* sd, uhdr_hip_image_t* dd,
                     hipStream_t s) {
  int rc;
  if ((rc = stage_p010_in(ss, 2, src, sd, s)) != 0) return rc;
  const size_t h = dest.height, ls = dest.luma_stride, cs = dest.chroma_stride;
  if ((rc = stage_reserve(ss, 0, ls * h)) != 0) return rc;
  if ((rc = stage_reserve(ss, 1, cs * h + cs)) != 0) return rc;
  *dd = dest;
  dd->data = ss->stage[0];
  dd->chroma_data = ss->stage[1];
  return UHDR_HIP_NO_ERROR;
}
// ... and what the reference writes copied back: luma_stride bytes per luma row, chroma_stride bytes per chroma row, V
// chroma_stride * height / 2 behind U.  Enqueues only.
int tonemap_copy_back(const uhdr_hip_image_t& dd, const uhdr_hip_image_t& dest, hipStream_t s) {
  const size_t h = dest.height, ls = dest.luma_stride, cs = dest.chroma_stride;
  if (ls * h) HIP_TRY(hipMemcpyAsync(dest.data, dd.data, ls * h, hipMemcpyDeviceToHost, s));
  const size_t v_off = cs * h / 2;
  if (cs * (h / 2)) {
    HIP_TRY(hipMemcpyAsync(dest.chroma_data, dd.chroma_data, cs * (h / 2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(dest.chroma_data) + v_off, static_cast<uint8_t*>(dd.chroma_data) + v_off,
                           cs * (h / 2), hipMemcpyDeviceToHost, s));
  }
  return UHDR_HIP_NO_ERROR;
}
}  // namespace

// UltraHdr::toneMap over n images in device memory: images of equal size (and equal alignment class) share a launch, grid.z = image
int uhdr_hip_tonemap_batch(int n, const uhdr_hip_image_t* srcs, uhdr_hip_image_t* dests, void* stream) {
  if (n < 0 || (n > 0 && (srcs == nullptr || dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const int rc = tonemap_check(&srcs[i], &dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
  }
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n;) {
    ToneBatch b;
    const Chunk ch = form_chunk(i, n, kToneChunk, [&](int j) { return srcs[j].width == srcs[i].width && srcs[j].height == srcs[i].height; },
                                [&](int j, int m) {
                                  bool aligned;
                                  b.img[m] = tone_image(srcs[j], dests[j], &aligned);
                                  return aligned;
                                });
    HIP_TRY(launch_tonemap(b, ch.m, ch.cls, s));
    for (int k = 0; k < ch.m; ++k) dests[i + k].colorGamut = srcs[i + k].colorGamut;  // ultrahdr.cpp:556
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// One image: in device memory the batch of one, which only enqueues; host planes go through single_call
int uhdr_hip_tonemap(const uhdr_hip_image_t* src, uhdr_hip_image_t* dest, int mem_space, void* stream) {
  int rc = tonemap_check(src, dest);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (mem_space == UHDR_HIP_MEM_DEVICE) return uhdr_hip_tonemap_batch(1, src, dest, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return single_call(
      src, dest, true, false, nullptr, s, [&](StageSet* ss, uhdr_hip_image_t* sd, uhdr_hip_image_t* dd) { return stage_tonemap_in(ss, *src, *dest, sd, dd, s); },
      [&](const uhdr_hip_image_t* sd, uhdr_hip_image_t* dd, float*) { return uhdr_hip_tonemap_batch(1, sd, dd, stream); },
      [&](const uhdr_hip_image_t& dd) { return tonemap_copy_back(dd, *dest, s); }, [&] { dest->colorGamut = src->colorGamut; });
}

// ---- tone-mapped SDR base image (include/uhdr_hip.h) -------------------------------------------------
namespace {
// the inverse OETFs on the host, for the headroom rule by itself: the reference's expressions (gainmapmath.cpp:279-286, :326-338)
// with libm in double, like the reference -- the values the device's exact functions return
float hlg_inv_oetf_host(float e) {
  const float a = 0.17883277f, b = 0.28466892f, c = (float)0.55991073;
  if (e <= 0.5f) return (float)(std::pow((double)e, (double)2.0f) / (double)3.0f);
  return (float)((std::exp((double)((e - c) / a)) + (double)b) / (double)12.0f);
}
float pq_inv_oetf_host(float e) {
  if (e <= 0.0001f) return 0.0f;
  const double p = std::pow((double)e, (double)0.0126833f);
  return (float)std::pow(((double)128.0f * p - (double)107.0f) / ((double)2413.0f - (double)2392.0f * p), (double)6.2773946361f);
}
// H of include/uhdr_hip.h, in f32; k_tonemap_head_finish performs the measured branch's operations on the device
float tone_headroom(int hdr_tf, float gamma_max, float peak_nits) {
  const float k = adaptive_cap(hdr_tf), cap = k;
  if (peak_nits > 0.0f) return fminf(fmaxf(peak_nits / 203.0f, 1.0f), cap);
  const float lin = hdr_tf == UHDR_HIP_TF_HLG ? hlg_inv_oetf_host(gamma_max) : hdr_tf == UHDR_HIP_TF_PQ ? pq_inv_oetf_host(gamma_max) : gamma_max;
  return fminf(fmaxf(lin * k, 1.0f), cap);
}
bool valid_tonemap_op(int op) { return op == UHDR_HIP_TONEMAP_SHIFT || op == UHDR_HIP_TONEMAP_REINHARD_MAXRGB; }

// what the operator asks of an image pair beyond tonemap_check: whole 2x2 blocks, a gamut, rows no shorter than the image
int tonemap_sdr_check(const uhdr_hip_image_t& src, const uhdr_hip_image_t& dest) {
  if ((src.width | src.height) & 1) return UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT;
  if (!valid_gamut(src.colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  if ((src.luma_stride != 0 && src.luma_stride < src.width) || src.chroma_stride < src.width || dest.luma_stride < dest.width ||
      dest.chroma_stride < dest.width / 2)
    return UHDR_HIP_ERROR_INVALID_STRIDE;
  return UHDR_HIP_NO_ERROR;
}
ToneImage tone_sdr_image(const uhdr_hip_image_t& sd, const uhdr_hip_image_t& dd, bool* aligned) {
  bool unused;
  ToneImage t = tone_image(sd, dd, &unused);
  t.sy_stride = (uint32_t)row_stride(sd);
  *aligned = t.width % 16u == 0 && al(t.sy, 16) && t.sy_stride % 8u == 0 && al(t.suv, 16) && t.suv_stride % 8u == 0 && al(t.dy, 16) &&
             t.dy_stride % 16u == 0 && al(t.du, 8) && al(t.dv, 8) && t.dc_stride % 8u == 0;
  return t;
}
ToneSdrConsts tone_sdr_consts(int gamut, int hdr_tf, float* headroom) {
  ToneSdrConsts c;
  const YuvRgb m = yuv_rgb_coeffs(gamut);
  c.cr = m.cr; c.gcb = m.gcb; c.gcr = m.gcr; c.cb = m.cb;
  float l[3] = {0.299f, 0.587f, 0.114f};   // p3RgbToYuv takes the BT.601 weights (gainmapmath.cpp:187-190)
  if (gamut != UHDR_HIP_CG_P3) luminance_coeffs(gamut, l);
  c.lr = l[0]; c.lg = l[1]; c.lb = l[2];
  c.ycb = m.cb; c.rycb = 1.0f / m.cb; c.ycr = m.cr; c.rycr = 1.0f / m.cr;
  c.k = adaptive_cap(hdr_tf);
  c.headroom = headroom;
  for (int i = 0; i < kToneChunk; ++i) c.slot[i] = 0u;
  return c;
}
// what the launches of one run take: the planar operator's descriptors and constants, the packed operator's batch; in both, slot[j]
// is the headroom slot of img[j]
extern "C++" {   // (overloads and a template inside extern "C")
struct ToneSdrRun { ToneBatch b; ToneSdrConsts c; };
ToneImage* run_img(ToneSdrRun& r) { return r.b.img; }
uint32_t* run_slot(ToneSdrRun& r) { return r.c.slot; }
TonePackedImage* run_img(TonePackedBatch& r) { return r.img; }
uint32_t* run_slot(TonePackedBatch& r) { return r.slot; }

// The four steps of both tone-map operators over n images in device memory, image i's headroom in slot i:
// the slots set -- 0, or the given H --, kToneHeadChunk at a time; pass 1 over the MEASURED members of every run, their descriptors
// and slots moved to the front of the run's; the slots finished, if anything was measured; pass 2 over every run.
//   form(i, &run) -> Chunk   the run from image i on (form_chunk), its descriptors in run_img(run)[0 .. m), every slot 0
//   pass1(run, cnt, cls)     the measuring launch over the first cnt members of `run`
//   pass2(run, i, m, cls)    the writing launch over the run, then the destination descriptors of images [i, i + m)
template <class Run, class Form, class Pass1, class Pass2>
int tone_head_passes(int n, int hdr_tf, const float* hdr_peak_nits, float* headroom, hipStream_t s, Form form, Pass1 pass1, Pass2 pass2) {
  const float k = adaptive_cap(hdr_tf);
  auto given = [&](int i) { return hdr_peak_nits != nullptr && hdr_peak_nits[i] > 0.0f; };
  auto heads = [&](bool finish) -> int {
    for (int base = 0; base < n; base += kToneHeadChunk) {
      ToneHeadInit v;
      const int cnt = std::min(n - base, kToneHeadChunk);
      for (int j = 0; j < cnt; ++j) v.h[j] = given(base + j) ? tone_headroom(hdr_tf, 0.0f, hdr_peak_nits[base + j]) : 0.0f;
      if (finish) HIP_TRY(launch_tonemap_head_finish(headroom + base, v, cnt, hdr_tf, k, k, s));
      else HIP_TRY(launch_tonemap_head_init(headroom + base, v, cnt, s));
    }
    return UHDR_HIP_NO_ERROR;
  };
  int rc = heads(false);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  bool any_measured = false;
  for (int i = 0; i < n;) {   // pass 1
    Run r;
    const Chunk ch = form(i, &r);
    int cnt = 0;
    for (int j = 0; j < ch.m; ++j)
      if (!given(i + j)) { run_img(r)[cnt] = run_img(r)[j]; run_slot(r)[cnt++] = (uint32_t)(i + j); }
    if (cnt) {
      any_measured = true;
      if ((rc = pass1(r, cnt, ch.cls)) != UHDR_HIP_NO_ERROR) return rc;
    }
    i += ch.m;
  }
  if (any_measured && (rc = heads(true)) != UHDR_HIP_NO_ERROR) return rc;
  for (int i = 0; i < n;) {   // pass 2
    Run r;
    const Chunk ch = form(i, &r);
    for (int j = 0; j < ch.m; ++j) run_slot(r)[j] = (uint32_t)(i + j);
    if ((rc = pass2(r, i, ch.m, ch.cls)) != UHDR_HIP_NO_ERROR) return rc;
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}
}  // extern "C++"
}  // namespace

int uhdr_hip_tonemap_headroom(int hdr_tf, float gamma_max, float peak_nits, float* headroom) {
  if (headroom == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (!valid_peak_nits(peak_nits)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  *headroom = tone_headroom(hdr_tf, gamma_max, peak_nits);
  return UHDR_HIP_NO_ERROR;
}

// n images in device memory: the checks, then tone_head_passes with the planar kernels -- images of equal size, gamut and alignment
// class that follow each other share the launches of either pass (grid.z = image)
int uhdr_hip_tonemap_sdr_batch(int n, const uhdr_hip_image_t* srcs, uhdr_hip_image_t* dests, int hdr_tf, int tonemap_op,
                               const float* hdr_peak_nits, float* headroom, void* stream) {
  if (n < 0 || (n > 0 && (srcs == nullptr || dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const int rc = tonemap_check(&srcs[i], &dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
  }
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (!valid_tonemap_op(tonemap_op)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (tonemap_op == UHDR_HIP_TONEMAP_SHIFT) return uhdr_hip_tonemap_batch(n, srcs, dests, stream);
  for (int i = 0; hdr_peak_nits != nullptr && i < n; ++i)
    if (!valid_peak_nits(hdr_peak_nits[i])) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (n > 0 && headroom == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const int rc = tonemap_sdr_check(srcs[i], dests[i]);
    if (rc != UHDR_HIP_NO_ERROR) return rc;
  }
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return tone_head_passes<ToneSdrRun>(
      n, hdr_tf, hdr_peak_nits, headroom, s,
      [&](int i, ToneSdrRun* r) {
        r->c = tone_sdr_consts(srcs[i].colorGamut, hdr_tf, headroom);
        return form_chunk(i, n, kToneChunk,
                          [&](int j) { return srcs[j].width == srcs[i].width && srcs[j].height == srcs[i].height && srcs[j].colorGamut == srcs[i].colorGamut; },
                          [&](int j, int m) {
                            bool aligned;
                            r->b.img[m] = tone_sdr_image(srcs[j], dests[j], &aligned);
                            return aligned;
                          });
      },
      [&](const ToneSdrRun& r, int cnt, bool aligned) -> int {
        HIP_TRY(launch_tonemap_peak(r.c, r.b, cnt, aligned, s));
        return UHDR_HIP_NO_ERROR;
      },
      [&](const ToneSdrRun& r, int i, int m, bool aligned) -> int {
        HIP_TRY(launch_tonemap_sdr(r.c, r.b, m, hdr_tf, aligned, s));
        for (int j = 0; j < m; ++j) dests[i + j].colorGamut = srcs[i + j].colorGamut;
        return UHDR_HIP_NO_ERROR;
      });
}

int uhdr_hip_tonemap_sdr(const uhdr_hip_image_t* src, uhdr_hip_image_t* dest, int hdr_tf, int tonemap_op, float hdr_peak_nits, float* headroom,
                         int mem_space, void* stream) {
  int rc = tonemap_check(src, dest);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (!tf_known(hdr_tf)) return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (!valid_tonemap_op(tonemap_op)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (tonemap_op == UHDR_HIP_TONEMAP_SHIFT) {   // no headroom to report
    if ((rc = uhdr_hip_tonemap(src, dest, mem_space, stream)) != UHDR_HIP_NO_ERROR) return rc;
    if (mem_space == UHDR_HIP_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return UHDR_HIP_NO_ERROR;
  }
  if (!valid_peak_nits(hdr_peak_nits)) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if ((rc = tonemap_sdr_check(*src, *dest)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return single_call(
      src, dest, mem_space != UHDR_HIP_MEM_DEVICE, true, headroom, s,
      [&](StageSet* ss, uhdr_hip_image_t* sd, uhdr_hip_image_t* dd) { return stage_tonemap_in(ss, *src, *dest, sd, dd, s); },
      [&](const uhdr_hip_image_t* sd, uhdr_hip_image_t* dd, float* dh) {
        return uhdr_hip_tonemap_sdr_batch(1, sd, dd, hdr_tf, tonemap_op, &hdr_peak_nits, dh, stream);
      },
      [&](const uhdr_hip_image_t& dd) { return tonemap_copy_back(dd, *dest, s); }, [&] { dest->colorGamut = src->colorGamut; });
}

// ---- the same operator on packed HDR images (include/uhdr_hip.h) ----------------------------------------
namespace {
size_t packed_stride(const uhdr_hip_image_t& im, size_t width) { return im.luma_stride == 0 ? width : im.luma_stride; }
// uhdr_hip_tonemap_packed_batch's checks behind its array pointers, in the header's order; host: the images lie in host memory,
// where nothing is asked of their alignment.  need_headroom: a NULL headroom is BAD_PTR where n > 0
int tone_packed_check(int n, const uhdr_hip_image_t* srcs, const uhdr_hip_image_t* dests, int hdr_tf, int tonemap_op, const float* peaks,
                      bool need_headroom, const float* headroom, bool host) {
  for (int i = 0; i < n; ++i) {
    if (srcs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA1010102 && srcs[i].pixelFormat != UHDR_HIP_PIX_FMT_RGBA_F16) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
    if (srcs[i].pixelFormat != srcs[0].pixelFormat) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  }
  const bool f16 = n > 0 && srcs[0].pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16;
  for (int i = 0; i < n; ++i) {
    if (srcs[i].data == nullptr || dests[i].data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
    if (!host && (!al(srcs[i].data, f16 ? 8 : 4) || !al(dests[i].data, 4))) return UHDR_HIP_ERROR_BAD_PTR;
  }
  if (n > 0 ? (f16 ? hdr_tf != UHDR_HIP_TF_LINEAR : (hdr_tf != UHDR_HIP_TF_HLG && hdr_tf != UHDR_HIP_TF_PQ))
            : !tf_known(hdr_tf))
    return UHDR_HIP_ERROR_INVALID_TRANS_FUNC;
  if (tonemap_op != UHDR_HIP_TONEMAP_REINHARD_MAXRGB) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;   // (TONEMAP_SHIFT means nothing here)
  for (int i = 0; peaks != nullptr && i < n; ++i)
    if (!valid_peak_nits(peaks[i])) return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (need_headroom && n > 0 && headroom == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  for (int i = 0; i < n; ++i) {
    const size_t ss = row_stride(srcs[i]), ds = packed_stride(dests[i], srcs[i].width);
    if (ss < srcs[i].width || ds < srcs[i].width || ss > 0xFFFFFFFFull || ds > 0xFFFFFFFFull) return UHDR_HIP_ERROR_INVALID_STRIDE;
    if (!valid_gamut(srcs[i].colorGamut)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  }
  return UHDR_HIP_NO_ERROR;
}
void fill_tone_packed_dest(const uhdr_hip_image_t& src, uhdr_hip_image_t* dest) {
  dest->luma_stride = packed_stride(*dest, src.width);
  dest->width = src.width;
  dest->height = src.height;
  dest->colorGamut = src.colorGamut;
  dest->pixelFormat = UHDR_HIP_PIX_FMT_RGBA8888;
}
}  // namespace

// n images in device memory: the checks, then tone_head_passes with the packed kernels
int uhdr_hip_tonemap_packed_batch(int n, const uhdr_hip_image_t* srcs, uhdr_hip_image_t* dests, int hdr_tf, int tonemap_op,
                                  const float* hdr_peak_nits, float* headroom, void* stream) {
  if (n < 0 || (n > 0 && (srcs == nullptr || dests == nullptr))) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = tone_packed_check(n, srcs, dests, hdr_tf, tonemap_op, hdr_peak_nits, true, headroom, false);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool f16 = n > 0 && srcs[0].pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16;
  return tone_head_passes<TonePackedBatch>(
      n, hdr_tf, hdr_peak_nits, headroom, s,
      [&](int i, TonePackedBatch* b) {   // the run: equal size and alignment class
        b->headroom = headroom;
        b->table = f16 ? nullptr : st->tone_tab + (hdr_tf == UHDR_HIP_TF_PQ ? kTonePackedCodes : 0u);
        b->k = adaptive_cap(hdr_tf);
        for (int j = 0; j < kToneChunk; ++j) b->slot[j] = 0u;
        return form_chunk(i, n, kToneChunk, [&](int j) { return srcs[j].width == srcs[i].width && srcs[j].height == srcs[i].height; },
                          [&](int j, int m) {
                            TonePackedImage& t = b->img[m];
                            t.src = srcs[j].data;
                            t.dst = static_cast<uint32_t*>(dests[j].data);
                            t.src_stride = (uint32_t)row_stride(srcs[j]);
                            t.dst_stride = (uint32_t)packed_stride(dests[j], srcs[j].width);
                            t.width = (uint32_t)srcs[j].width; t.height = (uint32_t)srcs[j].height;
                            // 16-byte pieces of the destination (4 pixels) and what they are made of (RGBA1010102: 16 bytes, RGBA F16: 32)
                            return t.width % 4u == 0 && al(t.src, 16) && t.src_stride % (f16 ? 2u : 4u) == 0 && al(t.dst, 16) && t.dst_stride % 4u == 0;
                          });
      },
      [&](const TonePackedBatch& b, int cnt, bool aligned) -> int {
        HIP_TRY(launch_tonemap_packed_peak(b, cnt, f16, aligned, s));
        return UHDR_HIP_NO_ERROR;
      },
      [&](const TonePackedBatch& b, int i, int m, bool aligned) -> int {
        HIP_TRY(launch_tonemap_packed(b, m, hdr_tf, aligned, s));
        for (int j = 0; j < m; ++j) fill_tone_packed_dest(srcs[i + j], &dests[i + j]);
        return UHDR_HIP_NO_ERROR;
      });
}

int uhdr_hip_tonemap_packed(const uhdr_hip_image_t* src, uhdr_hip_image_t* dest, int hdr_tf, int tonemap_op, float hdr_peak_nits,
                            float* headroom, int mem_space, void* stream) {
  if (src == nullptr || dest == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  int rc = tone_packed_check(1, src, dest, hdr_tf, tonemap_op, &hdr_peak_nits, false, nullptr, host);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // host memory: rows of the pixels alone, at a 64-byte pitch; only the pixels come back: the columns [width, stride) stay as they are
  const size_t w = src->width, h = src->height, bpp = src->pixelFormat == UHDR_HIP_PIX_FMT_RGBA_F16 ? 8 : 4;
  const size_t sp = round_up(w * bpp, 64), dp = round_up(w * 4, 64);
  return single_call(
      src, dest, host, true, headroom, s,
      [&](StageSet* ss, uhdr_hip_image_t* sd, uhdr_hip_image_t* dd) {
        int rc;
        if ((rc = stage_reserve(ss, 2, sp * h)) != 0) return rc;
        if ((rc = stage_reserve(ss, 0, dp * h)) != 0) return rc;
        if ((rc = h2d_plane(ss->stage[2], sp, src->data, packed_stride(*src, w) * bpp, w * bpp, h, 1, s)) != 0) return rc;
        *sd = *src; *dd = *dest;
        sd->data = ss->stage[2]; sd->luma_stride = sp / bpp;
        dd->data = ss->stage[0]; dd->luma_stride = dp / 4;
        return (int)UHDR_HIP_NO_ERROR;
      },
      [&](const uhdr_hip_image_t* sd, uhdr_hip_image_t* dd, float* dh) {
        return uhdr_hip_tonemap_packed_batch(1, sd, dd, hdr_tf, tonemap_op, &hdr_peak_nits, dh, stream);
      },
      [&](const uhdr_hip_image_t& dd) -> int {
        if (w * h) HIP_TRY(hipMemcpy2DAsync(dest->data, packed_stride(*dest, w) * 4, dd.data, dp, w * 4, h, hipMemcpyDeviceToHost, s));
        return UHDR_HIP_NO_ERROR;
      },
      [&] { fill_tone_packed_dest(*src, dest); });
}

namespace {
// JpegR::convertYuv's checks (jpegr.cpp:1134-1197): the encodings, which decide alone when they are equal (NO_ERROR, whatever the
// planes) or when there is no image to look at (n == 0), and then the planes of every image
int convert_encodings_check(int src_encoding, int dest_encoding) {
  if (src_encoding == UHDR_HIP_CG_UNSPECIFIED || dest_encoding == UHDR_HIP_CG_UNSPECIFIED)
    return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  if (!valid_gamut(src_encoding) || !valid_gamut(dest_encoding)) return UHDR_HIP_ERROR_INVALID_COLORGAMUT;
  return UHDR_HIP_NO_ERROR;
}
int convert_planes_check(const uhdr_hip_image_t& image) {
  return image.data == nullptr || image.chroma_data == nullptr ? UHDR_HIP_ERROR_BAD_PTR : UHDR_HIP_NO_ERROR;
}
}  // namespace

// JpegR::convertYuv over n images in device memory, in place: images of equal size (and equal alignment class) share a launch
int uhdr_hip_convert_yuv_batch(int n, uhdr_hip_image_t* images, int src_encoding, int dest_encoding, void* stream) {
  if (n < 0 || (n > 0 && images == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = convert_encodings_check(src_encoding, dest_encoding);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (src_encoding == dest_encoding) return UHDR_HIP_NO_ERROR;
  for (int i = 0; i < n; ++i)
    if ((rc = convert_planes_check(images[i])) != UHDR_HIP_NO_ERROR) return rc;
  const float* m = yuv_matrix(src_encoding, dest_encoding);
  DeviceState* st = nullptr;
  if ((rc = current_state(&st)) != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n;) {
    CvtBatch b;
    const Chunk ch = form_chunk(i, n, kToneChunk, [&](int j) { return images[j].width == images[i].width && images[j].height == images[i].height; },
                                [&](int j, int k) {
                                  bool aligned;
                                  b.img[k] = cvt_image(images[j], images[j], m, &aligned);
                                  return aligned;
                                });
    HIP_TRY(launch_convert_yuv(b, ch.m, ch.cls, s));
    i += ch.m;
  }
  return UHDR_HIP_NO_ERROR;
}

// One image: in device memory the batch of one, which only enqueues; host planes go through single_call -- the image staged into
// slots 0 and 1, converted in place there, and its pixels (whole 2x2 blocks of them) copied back
int uhdr_hip_convert_yuv(uhdr_hip_image_t* image, int src_encoding, int dest_encoding, int mem_space, void* stream) {
  if (image == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  int rc = convert_encodings_check(src_encoding, dest_encoding);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  if (src_encoding == dest_encoding) return UHDR_HIP_NO_ERROR;
  if ((rc = convert_planes_check(*image)) != UHDR_HIP_NO_ERROR) return rc;
  if (mem_space == UHDR_HIP_MEM_DEVICE) return uhdr_hip_convert_yuv_batch(1, image, src_encoding, dest_encoding, stream);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return single_call(
      nullptr, image, true, false, nullptr, s, [&](StageSet* ss, uhdr_hip_image_t*, uhdr_hip_image_t* d) { return stage_yuv420_in(ss, 0, *image, d, s); },
      [&](const uhdr_hip_image_t*, uhdr_hip_image_t* d, float*) { return uhdr_hip_convert_yuv_batch(1, d, src_encoding, dest_encoding, stream); },
      [&](const uhdr_hip_image_t& d) {
        const size_t h = image->height, cw = image->width / 2, ch = h / 2;
        int rc;
        if ((rc = d2h_plane(image->data, image->luma_stride, d.data, d.luma_stride, cw * 2, ch * 2, 1, s)) != 0) return rc;
        uint8_t* hu = static_cast<uint8_t*>(image->chroma_data);
        const uint8_t* du = static_cast<const uint8_t*>(d.chroma_data);
        if ((rc = d2h_plane(hu, image->chroma_stride, du, d.chroma_stride, cw, ch, 1, s)) != 0) return rc;
        return d2h_plane(hu + image->chroma_stride * (h / 2), image->chroma_stride, du + d.chroma_stride * (h / 2), d.chroma_stride, cw, ch, 1, s);
      },
      [] {});
}

// ---------------------------------------------------------------------------------------------------
// editorhelper effects.  fx_plan() restates the layout rules of editorhelper.cpp (output dims / strides /
// chroma placement, plane-by-plane index maps); the bytes are moved by k_effect.
// ---------------------------------------------------------------------------------------------------
namespace {
enum { FXK_CROP, FXK_MIRROR, FXK_ROTATE, FXK_RESIZE };

FxJob fx_job(const uint8_t* src, uint8_t* dst, size_t rows, size_t cols, size_t dst_stride, size_t src_stride, size_t in_w,
             size_t in_h, int op) {
  FxJob j;
  j.src = src; j.dst = dst; j.rows = (uint32_t)rows; j.cols = (uint32_t)cols;
  j.dst_stride = (uint32_t)dst_stride; j.src_stride = (uint32_t)src_stride;
  j.in_w = (uint32_t)in_w; j.in_h = (uint32_t)in_h;
  j.row_num = j.row_den = j.col_num = j.col_den = 1; j.op = op;
  return j;
}

// in/out hold pointers valid in the memory space the kernel will run in
int fx_plan(int kind, const uhdr_hip_image_t& in, int a, int b, int c, int d, uhdr_hip_image_t* out, FxJobs* jobs) {
  const bool mono = in.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  const size_t iw = in.width, ih = in.height;
  const size_t ls = row_stride(in);                 // editorhelper.cpp:44
  const size_t cs = in.chroma_stride != 0 ? in.chroma_stride : (ls >> 1);      // :60-61
  const uint8_t* sy = static_cast<const uint8_t*>(in.data);
  const uint8_t* sc = in.chroma_data ? static_cast<const uint8_t*>(in.chroma_data) : sy + ls * ih;  // :66-69
  uint8_t* dy = static_cast<uint8_t*>(out->data);
  out->colorGamut = in.colorGamut;
  out->pixelFormat = in.pixelFormat;
  jobs->n = 0;
  size_t ow, oh, ols;
  if (kind == FXK_CROP) {           // a=left b=right c=top d=bottom   (:26-76)
    ow = (size_t)(b - a + 1); oh = (size_t)(d - c + 1); ols = ow;
    jobs->job[jobs->n++] = fx_job(sy + ls * c + a, dy, oh, ow, ols, ls, iw, ih, FX_COPY);
  } else if (kind == FXK_MIRROR) {  // a=direction                      (:78-170)
    ow = iw; oh = ih; ols = ls;
    jobs->job[jobs->n++] = fx_job(sy, dy, oh, ow, ols, ls, iw, ih, a == 0 ? FX_FLIP_V : FX_FLIP_H);
  } else if (kind == FXK_ROTATE) {  // a=degrees                        (:172-306)
    if (a == 180) { ow = iw; oh = ih; ols = ls; } else { ow = ih; oh = iw; ols = ow; }
    jobs->job[jobs->n++] = fx_job(sy, dy, oh, ow, ols, ls, iw, ih, a == 90 ? FX_ROT90 : a == 180 ? FX_ROT180 : FX_ROT270);
  } else {                          // a=out_width b=out_height         (:308-360)
    ow = (size_t)a; oh = (size_t)b; ols = ow;
    FxJob j = fx_job(sy, dy, oh, ow, ols, ls, iw, ih, FX_RESIZE);
    j.row_num = (uint32_t)ih; j.row_den = (uint32_t)oh; j.col_num = (uint32_t)iw; j.col_den = (uint32_t)ow;
    jobs->job[jobs->n++] = j;
  }
  out->width = ow; out->height = oh; out->luma_stride = ols;
  if (mono) return UHDR_HIP_NO_ERROR;
  const size_t ocs = ols / 2;
  uint8_t* dc = dy + ols * oh;
  out->chroma_stride = ocs;
  out->chroma_data = dc;
  if (kind == FXK_CROP) {           // one copy of `oh` rows starting in the U plane (:70-73)
    jobs->job[jobs->n++] = fx_job(sc + cs * (c / 2) + (a / 2), dc, oh, ow / 2, ocs, cs, iw / 2, ih, FX_COPY);
  } else if (kind == FXK_RESIZE) {  // one pass over U and V (:350-357): rows and columns use the LUMA ratios
    FxJob j = fx_job(sc, dc, oh, ow / 2, ocs, cs, iw / 2, ih, FX_RESIZE);
    j.row_num = (uint32_t)ih; j.row_den = (uint32_t)oh; j.col_num = (uint32_t)iw; j.col_den = (uint32_t)ow;
    jobs->job[jobs->n++] = j;
  } else {                          // U then V, each (ih/2) x (iw/2)
    const int op = jobs->job[0].op;
    for (int p = 0; p < 2; ++p)
      jobs->job[jobs->n++] = fx_job(sc + (p ? cs * (ih / 2) : 0), dc + (p ? ocs * (oh / 2) : 0), oh / 2, ow / 2, ocs, cs, iw / 2,
                                    ih / 2, op);
  }
  return UHDR_HIP_NO_ERROR;
}

int fx_run(int kind, const uhdr_hip_image_t* in, int a, int b, int c, int d, uhdr_hip_image_t* out, int mem_space, void* stream) {
  // argument checks in the reference's order (editorhelper.cpp:29-39, 81-88, 174-185, 310-317)
  if (in == nullptr || in->data == nullptr || out == nullptr || out->data == nullptr) return UHDR_HIP_ERROR_BAD_PTR;
  if (kind == FXK_CROP && (a < 0 || (size_t)b >= in->width || c < 0 || (size_t)d >= in->height))
    return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;
  if (kind == FXK_ROTATE && a != 90 && a != 180 && a != 270) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;
  if (in->pixelFormat != UHDR_HIP_PIX_FMT_YUV420 && in->pixelFormat != UHDR_HIP_PIX_FMT_MONOCHROME)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  if (kind == FXK_RESIZE && (a <= 0 || b <= 0)) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;  // (ref: division by zero)
  if (kind == FXK_CROP && (b < a || d < c)) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;      // (ref: negative memcpy size)
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FxJobs jobs;
  if (mem_space == UHDR_HIP_MEM_DEVICE) {
    if ((rc = fx_plan(kind, *in, a, b, c, d, out, &jobs)) != 0) return rc;
    HIP_TRY(launch_effect(jobs, s));
    return UHDR_HIP_NO_ERROR;
  }
  // host memory: stage exactly the bytes the reference touches
  CodecLease lease(st);
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  const bool mono = in->pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  const size_t iw = in->width, ih = in->height;
  const size_t ls = row_stride(*in);
  const size_t cs = in->chroma_stride != 0 ? in->chroma_stride : (ls >> 1);
  const size_t luma_bytes = ih ? ls * (ih - 1) + iw : 0;
  const size_t chroma_rows = mono ? 0 : ih;  // U and V stacked (crop / resize walk them as one plane)
  const size_t chroma_bytes = chroma_rows ? cs * (chroma_rows - 1) + iw / 2 : 0;
  if ((rc = stage_reserve(st, 0, luma_bytes)) != 0) return rc;
  if ((rc = stage_reserve(st, 1, chroma_bytes)) != 0) return rc;
  if (luma_bytes) HIP_TRY(hipMemcpyAsync(st->stage[0], in->data, luma_bytes, hipMemcpyHostToDevice, s));
  const uint8_t* hc = in->chroma_data ? static_cast<const uint8_t*>(in->chroma_data)
                                      : static_cast<const uint8_t*>(in->data) + ls * ih;
  if (chroma_bytes) HIP_TRY(hipMemcpyAsync(st->stage[1], hc, chroma_bytes, hipMemcpyHostToDevice, s));
  uhdr_hip_image_t din = *in, dout = *out;
  din.data = st->stage[0];
  din.chroma_data = mono ? nullptr : st->stage[1];
  din.luma_stride = ls; din.chroma_stride = cs;
  // upper bound of the output extent: every layout rule yields <= max(ls, ow) * oh * 3/2 bytes
  uhdr_hip_image_t probe = *out;
  uint8_t dummy = 0;
  probe.data = &dummy;
  FxJobs pj;
  fx_plan(kind, *in, a, b, c, d, &probe, &pj);
  const size_t out_luma = probe.luma_stride * probe.height;
  const size_t out_chroma_rows = mono ? 0 : ((kind == FXK_CROP || kind == FXK_RESIZE) ? probe.height : 2 * (probe.height / 2));
  const size_t out_bytes = out_luma + (out_chroma_rows ? probe.chroma_stride * (out_chroma_rows - 1) + probe.width / 2 : 0);
  if ((rc = stage_reserve(st, 5, out_bytes)) != 0) return rc;
  dout.data = st->stage[5];
  if ((rc = fx_plan(kind, din, a, b, c, d, &dout, &jobs)) != 0) return rc;
  // bytes the kernel does not write (stride padding of mirror / rotate-180) must keep the caller's content
  if (out_bytes) HIP_TRY(hipMemcpyAsync(st->stage[5], out->data, out_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_effect(jobs, s));
  if (out_bytes) HIP_TRY(hipMemcpyAsync(out->data, st->stage[5], out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  out->width = dout.width; out->height = dout.height; out->colorGamut = dout.colorGamut; out->pixelFormat = dout.pixelFormat;
  out->luma_stride = dout.luma_stride;
  if (!mono) {
    out->chroma_stride = dout.chroma_stride;
    out->chroma_data = static_cast<uint8_t*>(out->data) + out->luma_stride * out->height;
  }
  return UHDR_HIP_NO_ERROR;
}
}  // namespace

int uhdr_hip_crop(const uhdr_hip_image_t* in_img, int left, int right, int top, int bottom, uhdr_hip_image_t* out_img,
                  int mem_space, void* stream) {
  return fx_run(FXK_CROP, in_img, left, right, top, bottom, out_img, mem_space, stream);
}
int uhdr_hip_mirror(const uhdr_hip_image_t* in_img, int mirror_dir, uhdr_hip_image_t* out_img, int mem_space, void* stream) {
  return fx_run(FXK_MIRROR, in_img, mirror_dir, 0, 0, 0, out_img, mem_space, stream);
}
int uhdr_hip_rotate(const uhdr_hip_image_t* in_img, int clockwise_degree, uhdr_hip_image_t* out_img, int mem_space,
                    void* stream) {
  return fx_run(FXK_ROTATE, in_img, clockwise_degree, 0, 0, 0, out_img, mem_space, stream);
}
int uhdr_hip_resize(const uhdr_hip_image_t* in_img, int out_width, int out_height, uhdr_hip_image_t* out_img, int mem_space,
                    void* stream) {
  return fx_run(FXK_RESIZE, in_img, out_width, out_height, 0, 0, out_img, mem_space, stream);
}

// addEffects (editorhelper.cpp:362-446): the chain stays in device memory, two ping-pong temporaries
int uhdr_hip_add_effects(const uhdr_hip_image_t* in, const uhdr_hip_effect_t* effects, int n, uhdr_hip_image_t* out, int mem_space,
                         void* stream) {
  if (in == nullptr || in->data == nullptr || out == nullptr || out->data == nullptr || n < 0 || (n > 0 && effects == nullptr))
    return UHDR_HIP_ERROR_BAD_PTR;
  if (in->pixelFormat != UHDR_HIP_PIX_FMT_YUV420 && in->pixelFormat != UHDR_HIP_PIX_FMT_MONOCHROME)
    return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;
  const bool mono = in->pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  const bool host = mem_space != UHDR_HIP_MEM_DEVICE;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  CodecLease lease(st);   // the temporaries: this call's own
  if ((st = lease.get()) == nullptr) return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;

  auto packed = [mono](size_t w, size_t h) { return mono ? w * h : w * h * 3 / 2; };
  size_t size = packed(in->width, in->height);
  const size_t size0 = size;
  // extents of every intermediate image (all tightly packed after the first effect)
  size_t max_bytes = size0;
  {
    size_t w = in->width, h = in->height;
    for (int i = 0; i < n; ++i) {
      const uhdr_hip_effect_t& e = effects[i];
      if (e.type == 0) { if (e.b < e.a || e.d < e.c) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; w = (size_t)(e.b - e.a + 1); h = (size_t)(e.d - e.c + 1); }
      else if (e.type == 2) { if (e.a == 90 || e.a == 270) std::swap(w, h); }
      else if (e.type == 3) { if (e.a <= 0 || e.b <= 0) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; w = (size_t)e.a; h = (size_t)e.b; }
      else if (e.type != 1) return UHDR_HIP_ERROR_BAD_PTR;
      max_bytes = std::max(max_bytes, packed(w, h));
    }
  }
  // The reference's out image is written after every step (:432-437), so beyond the last result it keeps the tails of the
  // earlier, larger ones.  dev_out plays that image: the caller's buffer itself, or its device stand-in for host calls.
  uint8_t* dev_out = static_cast<uint8_t*>(out->data);
  if (host) {
    if ((rc = stage_reserve(st, 5, max_bytes + 64)) != 0) return rc;
    dev_out = static_cast<uint8_t*>(st->stage[5]);
  }
  // :383-390: the descriptor and width*height(*3/2) bytes starting at the luma pointer are copied first
  out->width = in->width; out->height = in->height; out->colorGamut = in->colorGamut; out->pixelFormat = in->pixelFormat;
  out->luma_stride = in->luma_stride; out->chroma_stride = in->chroma_stride;
  if (size0) HIP_TRY(hipMemcpyAsync(dev_out, in->data, size0, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  // the first effect reads the caller's image (any strides); host images are staged as fx_run does
  uhdr_hip_image_t last = *in;
  const size_t ls0 = row_stride(*in);
  const size_t cs0 = in->chroma_stride != 0 ? in->chroma_stride : (ls0 >> 1);
  if (host && n > 0) {
    const size_t luma_bytes = in->height ? ls0 * (in->height - 1) + in->width : 0;
    const size_t chroma_bytes = (!mono && in->height) ? cs0 * (in->height - 1) + in->width / 2 : 0;
    if ((rc = stage_reserve(st, 0, luma_bytes)) != 0) return rc;
    if ((rc = stage_reserve(st, 1, chroma_bytes)) != 0) return rc;
    if (luma_bytes) HIP_TRY(hipMemcpyAsync(st->stage[0], in->data, luma_bytes, hipMemcpyHostToDevice, s));
    const uint8_t* hc = in->chroma_data ? static_cast<const uint8_t*>(in->chroma_data) : static_cast<const uint8_t*>(in->data) + ls0 * in->height;
    if (chroma_bytes) HIP_TRY(hipMemcpyAsync(st->stage[1], hc, chroma_bytes, hipMemcpyHostToDevice, s));
    last.data = st->stage[0];
    last.chroma_data = mono ? nullptr : st->stage[1];
    last.luma_stride = ls0; last.chroma_stride = cs0;
  }
  if ((rc = stage_reserve(st, 2, max_bytes + 64)) != 0) return rc;
  for (int i = 0; i < n; ++i) {
    const uhdr_hip_effect_t& e = effects[i];
    const size_t lls = row_stride(last);
    const bool keeps_stride = e.type == 1 || (e.type == 2 && e.a == 180);
    if (keeps_stride && (lls != last.width || (!mono && last.chroma_stride != 0 && last.chroma_stride != last.width / 2)))
      return UHDR_HIP_ERROR_UNSUPPORTED_FEATURE;   // the reference writes past its `size`-byte temporary here
    // same argument checks as the single effects (fx_run)
    if (e.type == 0 && (e.a < 0 || (size_t)e.b >= last.width || e.c < 0 || (size_t)e.d >= last.height)) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;
    if (e.type == 2 && e.a != 90 && e.a != 180 && e.a != 270) return UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS;
    uhdr_hip_image_t tmp = *out;
    tmp.data = st->stage[2];
    FxJobs jobs;
    const int kind = e.type == 0 ? FXK_CROP : e.type == 1 ? FXK_MIRROR : e.type == 2 ? FXK_ROTATE : FXK_RESIZE;
    if ((rc = fx_plan(kind, last, e.a, e.b, e.c, e.d, &tmp, &jobs)) != 0) return rc;
    HIP_TRY(launch_effect(jobs, s));
    size = e.type == 0 ? packed((size_t)(e.b - e.a + 1), (size_t)(e.d - e.c + 1))
         : e.type == 3 ? packed((size_t)e.a, (size_t)e.b) : packed(last.width, last.height);   // :395-430
    if (size) HIP_TRY(hipMemcpyAsync(dev_out, tmp.data, size, hipMemcpyDeviceToDevice, s));    // the "deep copy", :437
    last = tmp;
    last.data = dev_out;                                                                         // last = out_img, :442
    last.chroma_data = mono ? nullptr : dev_out + last.luma_stride * last.height;               // :438-440
  }
  if (n > 0) {
    out->width = last.width; out->height = last.height; out->colorGamut = last.colorGamut; out->pixelFormat = last.pixelFormat;
    out->luma_stride = last.luma_stride; out->chroma_stride = last.chroma_stride;
    if (!mono) out->chroma_data = static_cast<uint8_t*>(out->data) + out->luma_stride * out->height;
  }
  if (host) {
    if (max_bytes) HIP_TRY(hipMemcpyAsync(out->data, dev_out, max_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return UHDR_HIP_NO_ERROR;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// A chain as one gather (uhdr_hip_add_effects_batch).  fx_compose() walks the chain with fx_plan() over images that exist as
// address ranges only: every step's jobs say which bytes of the step's input each output byte comes from, and the input's bytes
// are known, region by region, as source offset a[row] + b[col] of the caller's image.  A step whose jobs keep that form for
// every region (checked, not assumed: a job that reads rows of two regions must find their column tables a constant apart)
// yields the next image's regions; one that does not ends the composition and the image runs step by step.
// ---------------------------------------------------------------------------------------------------
namespace {
struct FxcRegion {          // `rows` rows of `cols` bytes at address `addr`, `stride` apart: byte (r, c) is source byte a[r] + b[c] of plane `base`
  uint64_t addr = 0;
  size_t rows = 0, cols = 0, stride = 0;
  int base = 0;             // 0: offsets from the luma pointer, 1: from the chroma pointer
  std::vector<int64_t> a, b;
};
struct FxcPlan {
  int status = UHDR_HIP_NO_ERROR;
  bool fused = false;
  uhdr_hip_image_t out = {};       // the final descriptor, data == NULL
  size_t packed = 0;               // bytes of the result
  std::vector<FxcRegion> planes;   // fused: the result's regions, addr = offset from out[i]
  std::vector<int> cls;            // ... and their classes, after fx_finish
  std::vector<uint32_t> lo, hi;
};
constexpr uint64_t kFxcLuma = 1ull << 40, kFxcChroma = 2ull << 40, kFxcOut = 3ull << 40;   // where the imaginary images lie

size_t fx_packed(bool mono, size_t w, size_t h) { return mono ? w * h : w * h * 3 / 2; }

// one step: `cur` describes the bytes fx_plan's jobs read; false: the step's map is not of the form a[i] + b[j]
bool fx_compose_step(const std::vector<FxcRegion>& cur, const FxJobs& jobs, std::vector<FxcRegion>* next) {
  next->clear();
  for (int k = 0; k < jobs.n; ++k) {
    const FxJob& j = jobs.job[k];
    if (j.rows == 0 || j.cols == 0) continue;
    const bool transposed = j.op == FX_ROT90 || j.op == FX_ROT270;
    // source row of output row i (of output column i when transposed) and source column of output column i (row when transposed)
    const size_t nr = transposed ? j.cols : j.rows, nc = transposed ? j.rows : j.cols;
    auto src_row = [&](size_t i) -> size_t {
      switch (j.op) {
        case FX_FLIP_V: return j.rows - 1 - i;
        case FX_ROT180: case FX_ROT90: return j.in_h - 1 - i;
        case FX_RESIZE: return (size_t)((uint64_t)i * j.row_num / j.row_den);
        default: return i;   // FX_COPY, FX_FLIP_H, FX_ROT270
      }
    };
    auto src_col = [&](size_t i) -> size_t {
      switch (j.op) {
        case FX_FLIP_H: case FX_ROT180: case FX_ROT270: return j.in_w - 1 - i;
        case FX_RESIZE: return (size_t)((uint64_t)i * j.col_num / j.col_den);
        default: return i;   // FX_COPY, FX_FLIP_V, FX_ROT90
      }
    };
    size_t max_col = 0;
    for (size_t i = 0; i < nc; ++i) max_col = std::max(max_col, src_col(i));
    FxcRegion r;
    r.addr = reinterpret_cast<uint64_t>(j.dst);
    r.rows = j.rows; r.cols = j.cols; r.stride = j.dst_stride;
    std::vector<int64_t> va(nr), vb(nc);
    // the (region, first column) pairs the job's source rows fall into, and how far each pair's column table lies from the first one's
    struct Key { int region; size_t x0; int64_t delta; };
    std::vector<Key> keys;
    const uint64_t src0 = reinterpret_cast<uint64_t>(j.src);
    for (size_t i = 0; i < nr; ++i) {
      const uint64_t addr = src0 + (uint64_t)src_row(i) * j.src_stride;
      int reg = -1;
      for (size_t q = 0; q < cur.size(); ++q)
        if (addr >= cur[q].addr && addr < cur[q].addr + (uint64_t)cur[q].rows * cur[q].stride) { reg = (int)q; break; }
      if (reg < 0) return false;
      const FxcRegion& c = cur[reg];
      if (c.stride != j.src_stride && nr > 1) return false;
      const size_t rr = (size_t)((addr - c.addr) / c.stride), x0 = (size_t)((addr - c.addr) % c.stride);
      if (x0 + max_col >= c.cols) return false;
      size_t kk = 0;
      while (kk < keys.size() && !(keys[kk].region == reg && keys[kk].x0 == x0)) ++kk;
      if (kk == keys.size()) {
        if (keys.empty()) {
          r.base = c.base;
          for (size_t q = 0; q < nc; ++q) vb[q] = c.b[x0 + src_col(q)];
          keys.push_back({reg, x0, 0});
        } else {
          if (transposed || c.base != r.base) return false;
          const int64_t delta = c.b[x0 + src_col(0)] - vb[0];
          for (size_t q = 0; q < nc; ++q)
            if (c.b[x0 + src_col(q)] - vb[q] != delta) return false;   // the two regions' columns are not a constant apart
          keys.push_back({reg, x0, delta});
        }
      }
      va[i] = c.a[rr] + keys[kk].delta;
    }
    if (transposed) { r.a = std::move(vb); r.b = std::move(va); }
    else { r.a = std::move(va); r.b = std::move(vb); }
    next->push_back(std::move(r));
  }
  return true;
}

// classes and bounds of a fused plan's regions.  ext[base]: bytes of the source plane the caller described
int fx_finish(FxcPlan* p, const size_t ext[2]) {
  for (FxcRegion& r : p->planes) {
    int64_t amin = r.a[0], amax = r.a[0], bmin = r.b[0], bmax = r.b[0];
    for (int64_t v : r.a) { amin = std::min(amin, v); amax = std::max(amax, v); }
    for (int64_t v : r.b) { bmin = std::min(bmin, v); bmax = std::max(bmax, v); }
    // the guard: nothing is launched that could read outside the caller's plane
    if (amin + bmin < 0 || amax + bmax < 0 || (uint64_t)(amax + bmax) >= ext[r.base] || (uint64_t)(amax + bmax) > 0xFFFFFFFFull ||
        r.rows > 0x7FFFFFFFull || r.cols > 0x7FFFFFF0ull || r.stride > 0xFFFFFFFFull)
      return UHDR_HIP_UNKNOWN_ERROR;
    for (int64_t& v : r.a) v += bmin;     // both tables non-negative
    for (int64_t& v : r.b) v -= bmin;
    p->lo.push_back((uint32_t)(amin + bmin));
    p->hi.push_back((uint32_t)(amax + bmax));
    bool asc = true, desc = true, bup = true, bdown = true, aup = true, adown = true;
    for (size_t q = 1; q < r.cols; ++q) {
      const int64_t d = r.b[q] - r.b[q - 1];
      asc = asc && d == 1; desc = desc && d == -1; bup = bup && d >= 0; bdown = bdown && d <= 0;
    }
    for (size_t q = 1; q < r.rows; ++q) {
      const int64_t d = r.a[q] - r.a[q - 1];
      aup = aup && d >= 0; adown = adown && d <= 0;
    }
    int cls = FXC_GATHER;
    if (asc) cls = FXC_ASC;
    else if (desc) cls = FXC_DESC;
    else {
      bool lds = bup || bdown;      // at most 4 source bytes per output byte in every block of 4096 columns (k_effect's bound for resize)
      for (size_t c0 = 0; lds && c0 < r.cols; c0 += 4096) {
        const size_t c1 = std::min(c0 + 4095, r.cols - 1);
        lds = (uint64_t)std::llabs(r.b[c1] - r.b[c0]) <= 4ull * (c1 - c0 + 1);
      }
      bool tile = aup || adown;     // the rows of every 64-row tile less than 256 bytes apart
      for (size_t i0 = 0; tile && i0 < r.rows; i0 += 64) tile = std::llabs(r.a[std::min(i0 + 63, r.rows - 1)] - r.a[i0]) < 256;
      cls = lds ? FXC_LDS : tile ? FXC_TILE : FXC_GATHER;
    }
    p->cls.push_back(cls);
  }
  return UHDR_HIP_NO_ERROR;
}

// Checks in uhdr_hip_add_effects' order, then the composition.  `in` holds the caller's descriptor (its pointers are not followed).
void fx_compose(const uhdr_hip_image_t& in, const uhdr_hip_effect_t* fx, int n, FxcPlan* p) {
  p->status = UHDR_HIP_NO_ERROR;
  p->fused = false;
  if (in.pixelFormat != UHDR_HIP_PIX_FMT_YUV420 && in.pixelFormat != UHDR_HIP_PIX_FMT_MONOCHROME) { p->status = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; return; }
  const bool mono = in.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
  for (int i = 0; i < n; ++i) {
    const uhdr_hip_effect_t& e = fx[i];
    if (e.type == 0) { if (e.b < e.a || e.d < e.c) { p->status = UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; return; } }
    else if (e.type == 3) { if (e.a <= 0 || e.b <= 0) { p->status = UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; return; } }
    else if (e.type != 1 && e.type != 2) { p->status = UHDR_HIP_ERROR_BAD_PTR; return; }
  }
  const size_t iw = in.width, ih = in.height;
  const size_t ls0 = row_stride(in);
  const size_t cs0 = in.chroma_stride != 0 ? in.chroma_stride : (ls0 >> 1);
  bool odd = !mono && ((iw | ih) & 1u) != 0;
  bool additive = iw != 0 && ih != 0 && iw < (1u << 30) && ih < (1u << 30) && ls0 < (1ull << 31) && cs0 < (1ull << 31);
  std::vector<FxcRegion> cur, next;
  if (additive && !odd) {
    FxcRegion y;
    y.addr = kFxcLuma; y.rows = ih; y.cols = iw; y.stride = ls0; y.base = 0;
    y.a.resize(ih); y.b.resize(iw);
    for (size_t i = 0; i < ih; ++i) y.a[i] = (int64_t)(i * ls0);
    for (size_t i = 0; i < iw; ++i) y.b[i] = (int64_t)i;
    cur.push_back(std::move(y));
    for (int pl = 0; pl < 2 && !mono; ++pl) {   // U, then V at chroma + chroma_stride * (height / 2)
      FxcRegion c;
      c.addr = kFxcChroma + (pl ? cs0 * (ih / 2) : 0); c.rows = ih / 2; c.cols = iw / 2; c.stride = cs0; c.base = 1;
      c.a.resize(c.rows); c.b.resize(c.cols);
      for (size_t i = 0; i < c.rows; ++i) c.a[i] = (int64_t)((i + (pl ? ih / 2 : 0)) * cs0);
      for (size_t i = 0; i < c.cols; ++i) c.b[i] = (int64_t)i;
      cur.push_back(std::move(c));
    }
  }
  // the chain as uhdr_hip_add_effects walks it
  uhdr_hip_image_t last = in;
  last.data = reinterpret_cast<void*>(kFxcLuma);
  last.chroma_data = mono ? nullptr : reinterpret_cast<void*>(kFxcChroma);
  uhdr_hip_image_t out = in;
  out.data = nullptr;
  for (int i = 0; i < n; ++i) {
    const uhdr_hip_effect_t& e = fx[i];
    const size_t lls = row_stride(last);
    const bool keeps_stride = e.type == 1 || (e.type == 2 && e.a == 180);
    if (keeps_stride && (lls != last.width || (!mono && last.chroma_stride != 0 && last.chroma_stride != last.width / 2))) { p->status = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; return; }
    if (e.type == 0 && (e.a < 0 || (size_t)e.b >= last.width || e.c < 0 || (size_t)e.d >= last.height)) { p->status = UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; return; }
    if (e.type == 2 && e.a != 90 && e.a != 180 && e.a != 270) { p->status = UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS; return; }
    uhdr_hip_image_t tmp = out;
    tmp.data = reinterpret_cast<void*>(kFxcOut);
    FxJobs jobs;
    const int kind = e.type == 0 ? FXK_CROP : e.type == 1 ? FXK_MIRROR : e.type == 2 ? FXK_ROTATE : FXK_RESIZE;
    fx_plan(kind, last, e.a, e.b, e.c, e.d, &tmp, &jobs);
    if (additive && !odd) {
      additive = fx_compose_step(cur, jobs, &next);
      cur.swap(next);
    }
    out = tmp;
    last = tmp;   // the next step reads what this one wrote: tightly packed at kFxcOut, chroma behind luma
    last.chroma_data = mono ? nullptr : reinterpret_cast<void*>(kFxcOut + last.luma_stride * last.height);
    odd = odd || (!mono && ((last.width | last.height) & 1u) != 0);
  }
  if (odd) { p->status = UHDR_HIP_ERROR_UNSUPPORTED_FEATURE; return; }   // the reference reads chroma rows it never wrote
  out.data = nullptr;
  out.chroma_data = nullptr;
  p->out = out;
  p->packed = fx_packed(mono, out.width, out.height);
  if (n == 0 || !additive) return;
  size_t ext[2];
  ext[0] = ls0 * (ih - 1) + iw;
  ext[1] = mono ? 0 : cs0 * (ih - 1) + iw / 2;
  for (FxcRegion& r : cur) r.addr -= kFxcOut;
  p->planes = std::move(cur);
  p->status = fx_finish(p, ext);
  p->fused = p->status == UHDR_HIP_NO_ERROR;
}
}  // namespace

namespace {
// the tables the kernel gets for one region: a[rows], b[cols rounded up to 16] (the padding repeats the last entry)
void fx_tables(const FxcRegion& r, uint32_t* a, uint32_t* b) {
  for (size_t i = 0; i < r.rows; ++i) a[i] = (uint32_t)r.a[i];
  const size_t padded = round_up(r.cols, 16);
  for (size_t i = 0; i < padded; ++i) b[i] = (uint32_t)r.b[std::min(i, r.cols - 1)];
}

// the stream's workspace with room for `bytes`, its host side free to be rewritten
int fx_workspace(DeviceState* st, hipStream_t s, size_t bytes, DeviceState::FxWs** out) {
  DeviceState::FxWs* w = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    try {
      w = &st->fx_ws[s];
      st->retired.reserve(st->retired.size() + 1);
    } catch (const std::bad_alloc&) {
      return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
    }
  }
  if (w->ev == nullptr) HIP_TRY(hipEventCreateWithFlags(&w->ev, hipEventDisableTiming));
  if (w->pending) { HIP_TRY(hipEventSynchronize(w->ev)); w->pending = false; }   // the last round's upload has left the host side
  if (w->host_bytes < bytes) {
    if (w->host) HIP_TRY(hipHostFree(w->host));
    w->host = nullptr; w->host_bytes = 0;
    const size_t grown = std::max(bytes, (size_t)1 << 16);
    HIP_TRY(hipHostMalloc(&w->host, grown, hipHostMallocDefault));
    w->host_bytes = grown;
  }
  if (w->dev_bytes < bytes) {
    if (w->dev) {   // a launch already on the stream may name it: kept until the stream is released
      std::lock_guard<std::mutex> lk(g_mu);
      st->retired.emplace_back(s, w->dev);
      w->dev = nullptr; w->dev_bytes = 0;
    }
    const size_t grown = std::max(bytes, 2 * w->host_bytes);
    HIP_TRY(hipMalloc(&w->dev, grown));
    w->dev_bytes = grown;
  }
  *out = w;
  return UHDR_HIP_NO_ERROR;
}

struct FxcItem {
  const uhdr_hip_image_t* in;
  const uhdr_hip_effect_t* fx;
  int n_fx;
  void* out;
  size_t cap;
  uhdr_hip_image_t* out_img;
  int status;
  FxcPlan plan;
};

// every check of one image that needs no device, and its plan
void fx_item_prepare(FxcItem* it) {
  it->status = UHDR_HIP_NO_ERROR;
  if (it->in->data == nullptr || (it->out == nullptr && it->cap != 0)) { it->status = UHDR_HIP_ERROR_BAD_PTR; return; }
  fx_compose(*it->in, it->fx, it->n_fx, &it->plan);
  if (it->plan.status != UHDR_HIP_NO_ERROR) { it->status = it->plan.status; return; }
  uhdr_hip_image_t d = it->plan.out;
  d.data = it->out;
  if (d.pixelFormat == UHDR_HIP_PIX_FMT_YUV420 && it->out != nullptr) d.chroma_data = static_cast<uint8_t*>(it->out) + d.luma_stride * d.height;
  *it->out_img = d;
  if (it->out == nullptr || it->cap < it->plan.packed) it->status = UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;   // (out == NULL: a size probe)
}

// the prepared images that passed their checks, in rounds of `round` images: one upload and one launch per round, the images
// whose chain is not one gather step by step behind it.  Enqueues on s; statuses of images that fail here are updated.
int fx_items_run(std::vector<FxcItem>& items, int round, hipStream_t s) {
  std::vector<size_t> todo;
  for (size_t i = 0; i < items.size(); ++i)
    if (items[i].status == UHDR_HIP_NO_ERROR && items[i].plan.packed != 0) todo.push_back(i);
  if (todo.empty()) return UHDR_HIP_NO_ERROR;
  DeviceState* st = nullptr;
  int rc = current_state(&st);
  if (rc != UHDR_HIP_NO_ERROR) return rc;
  std::lock_guard<std::mutex> pl(g_pair_mu);   // workspace, upload and launch of a stream as one unit
  for (size_t r0 = 0; r0 < todo.size(); r0 += (size_t)round) {
    const size_t r1 = std::min(todo.size(), r0 + (size_t)round);
    // layout of the round: the jobs, then every job's two tables, 16-byte aligned
    size_t n_jobs = 0, words = 0;
    for (size_t q = r0; q < r1; ++q) {
      const FxcItem& it = items[todo[q]];
      if (it.n_fx == 0 || !it.plan.fused) continue;
      for (const FxcRegion& g : it.plan.planes) { ++n_jobs; words += round_up(g.rows, 4) + round_up(g.cols, 16); }
    }
    if (n_jobs != 0) {
      const size_t job_bytes = round_up(n_jobs * sizeof(FxChainJob), 256), bytes = job_bytes + words * 4;
      DeviceState::FxWs* w = nullptr;
      if ((rc = fx_workspace(st, s, bytes, &w)) != UHDR_HIP_NO_ERROR) return rc;
      FxChainJob* hj = static_cast<FxChainJob*>(w->host);
      uint32_t* ht = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(w->host) + job_bytes);
      const uint32_t* dt = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(w->dev) + job_bytes);
      size_t k = 0, at = 0;
      for (size_t q = r0; q < r1; ++q) {
        const FxcItem& it = items[todo[q]];
        if (it.n_fx == 0 || !it.plan.fused) continue;
        const uhdr_hip_image_t& in = *it.in;
        const size_t ls = row_stride(in);
        const uint8_t* sy = static_cast<const uint8_t*>(in.data);
        const uint8_t* sc = in.chroma_data ? static_cast<const uint8_t*>(in.chroma_data) : sy + ls * in.height;
        for (size_t g = 0; g < it.plan.planes.size(); ++g) {
          const FxcRegion& reg = it.plan.planes[g];
          FxChainJob& j = hj[k++];
          j.src = reg.base ? sc : sy;
          j.dst = static_cast<uint8_t*>(it.out) + reg.addr;
          j.rows = (uint32_t)reg.rows; j.cols = (uint32_t)reg.cols; j.dst_stride = (uint32_t)reg.stride;
          j.lo = it.plan.lo[g]; j.hi = it.plan.hi[g]; j.cls = it.plan.cls[g];
          fx_tables(reg, ht + at, ht + at + round_up(reg.rows, 4));
          j.a = dt + at;
          j.b = dt + at + round_up(reg.rows, 4);
          at += round_up(reg.rows, 4) + round_up(reg.cols, 16);
        }
      }
      HIP_TRY(hipMemcpyAsync(w->dev, w->host, bytes, hipMemcpyHostToDevice, s));
      HIP_TRY(hipEventRecord(w->ev, s));
      w->pending = true;
      HIP_TRY(launch_effect_chain(static_cast<const FxChainJob*>(w->dev), hj, (int)n_jobs, s));
    }
    for (size_t q = r0; q < r1; ++q) {
      FxcItem& it = items[todo[q]];
      if (it.n_fx == 0) {   // addEffects without effects: the packed extent, copied as it lies (editorhelper.cpp:383-390)
        HIP_TRY(hipMemcpyAsync(it.out, it.in->data, it.plan.packed, hipMemcpyDeviceToDevice, s));
      } else if (!it.plan.fused) {
        // step by step, as uhdr_hip_add_effects does it, into a temporary the size of the largest intermediate image; only the
        // result's own bytes reach out[i]
        const bool mono = it.in->pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME;
        size_t w2 = it.in->width, h2 = it.in->height, max_bytes = fx_packed(mono, w2, h2);
        for (int e = 0; e < it.n_fx; ++e) {
          const uhdr_hip_effect_t& f = it.fx[e];
          if (f.type == 0) { w2 = (size_t)(f.b - f.a + 1); h2 = (size_t)(f.d - f.c + 1); }
          else if (f.type == 2 && f.a != 180) std::swap(w2, h2);
          else if (f.type == 3) { w2 = (size_t)f.a; h2 = (size_t)f.b; }
          max_bytes = std::max(max_bytes, fx_packed(mono, w2, h2));
        }
        CodecLease lease(st);
        DeviceState* cx = lease.get();
        if (cx == nullptr) { it.status = UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE; continue; }
        if ((rc = stage_reserve(cx, 3, max_bytes + 64)) != 0) { it.status = rc; continue; }
        uhdr_hip_image_t tmp = {};
        tmp.data = cx->stage[3];
        rc = uhdr_hip_add_effects(it.in, it.fx, it.n_fx, &tmp, UHDR_HIP_MEM_DEVICE, s);
        if (rc != UHDR_HIP_NO_ERROR) { it.status = rc; continue; }
        HIP_TRY(hipMemcpyAsync(it.out, tmp.data, it.plan.packed, hipMemcpyDeviceToDevice, s));
      }
    }
  }
  return UHDR_HIP_NO_ERROR;
}
}  // namespace

extern "C" {

int uhdr_hip_add_effects_batch(int n, const uhdr_hip_image_t* in_imgs, const uhdr_hip_effect_t* effects, int n_effects, void* const* out,
                               const size_t* out_capacity, uhdr_hip_image_t* out_imgs, int* status, void* stream) {
  if (n < 0 || n_effects < 0 || (n_effects > 0 && effects == nullptr) ||
      (n > 0 && (in_imgs == nullptr || out == nullptr || out_capacity == nullptr || out_imgs == nullptr)))
    return UHDR_HIP_ERROR_BAD_PTR;
  std::vector<FxcItem> items;
  try {
    items.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
      FxcItem& it = items[i];
      it.in = &in_imgs[i]; it.fx = effects; it.n_fx = n_effects; it.out = out[i]; it.cap = out_capacity[i]; it.out_img = &out_imgs[i];
      fx_item_prepare(&it);
    }
  } catch (const std::bad_alloc&) {
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  int rc = UHDR_HIP_NO_ERROR;
  try {
    rc = fx_items_run(items, kFxChainRound, static_cast<hipStream_t>(stream));
  } catch (const std::bad_alloc&) {
    rc = UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  int first = UHDR_HIP_NO_ERROR;
  for (int i = 0; i < n; ++i) {
    if (status) status[i] = items[i].status;
    if (first == UHDR_HIP_NO_ERROR) first = items[i].status;
  }
  return first != UHDR_HIP_NO_ERROR ? first : rc;
}

int uhdr_hip_effect_chain_map(size_t width, size_t height, size_t luma_stride, size_t chroma_stride, int pixel_format,
                              const uhdr_hip_effect_t* effects, int n_effects, uhdr_hip_image_t* out_desc, int* fused, uint32_t* offsets,
                              size_t capacity, size_t* count) {
  if (out_desc == nullptr || fused == nullptr || count == nullptr || n_effects < 0 || (n_effects > 0 && effects == nullptr))
    return UHDR_HIP_ERROR_BAD_PTR;
  try {
    uhdr_hip_image_t in = {};
    in.width = width; in.height = height; in.luma_stride = luma_stride; in.chroma_stride = chroma_stride;
    in.colorGamut = UHDR_HIP_CG_UNSPECIFIED; in.pixelFormat = pixel_format;
    FxcPlan plan;
    fx_compose(in, effects, n_effects, &plan);
    if (plan.status != UHDR_HIP_NO_ERROR) return plan.status;
    *out_desc = plan.out;
    *count = plan.packed;
    *fused = (n_effects == 0 || plan.fused) ? 1 : 0;
    if (!*fused || offsets == nullptr || capacity < plan.packed) return UHDR_HIP_NO_ERROR;
    if (n_effects == 0) {
      for (size_t k = 0; k < plan.packed; ++k) offsets[k] = (uint32_t)k;
      return UHDR_HIP_NO_ERROR;
    }
    const size_t ls = luma_stride != 0 ? luma_stride : width;
    std::vector<uint32_t> a, b;
    for (const FxcRegion& r : plan.planes) {
      a.assign(r.rows, 0);
      b.assign(round_up(r.cols, 16), 0);
      fx_tables(r, a.data(), b.data());
      const uint32_t base = r.base ? (uint32_t)(ls * height) : 0u;   // chroma right behind luma
      for (size_t i = 0; i < r.rows; ++i)
        for (size_t c = 0; c < r.cols; ++c) offsets[r.addr + i * r.stride + c] = base + a[i] + b[c];
    }
    return UHDR_HIP_NO_ERROR;
  } catch (const std::bad_alloc&) {
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
}

int uhdr_hip_effect_chain_classes(size_t width, size_t height, size_t luma_stride, size_t chroma_stride, int pixel_format,
                                  const uhdr_hip_effect_t* effects, int n_effects, int* fused, int* classes, size_t capacity,
                                  size_t* count) {
  if (fused == nullptr || count == nullptr || n_effects < 0 || (n_effects > 0 && effects == nullptr)) return UHDR_HIP_ERROR_BAD_PTR;
  try {
    uhdr_hip_image_t in = {};
    in.width = width; in.height = height; in.luma_stride = luma_stride; in.chroma_stride = chroma_stride;
    in.colorGamut = UHDR_HIP_CG_UNSPECIFIED; in.pixelFormat = pixel_format;
    FxcPlan plan;
    fx_compose(in, effects, n_effects, &plan);
    if (plan.status != UHDR_HIP_NO_ERROR) return plan.status;
    *fused = (n_effects == 0 || plan.fused) ? 1 : 0;
    *count = plan.fused ? plan.cls.size() : 0;   // (no effects: a plain copy of the packed extent, no plane job)
    for (size_t k = 0; classes != nullptr && k < *count && k < capacity; ++k) classes[k] = plan.cls[k];
    return UHDR_HIP_NO_ERROR;
  } catch (const std::bad_alloc&) {
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// n JPEG/R files in, n edited JPEG/R files out: split, decode both JPEGs of every file into device memory (one decoder launch set
// per round), the two chains over all 2 m images of the round in one launch, API-x encode of the round.  Nothing uncompressed
// crosses PCIe.
// ---------------------------------------------------------------------------------------------------
namespace {
struct EditFile {
  int idx;
  const uint8_t* jpg[2];
  size_t len[2];
  uhdr_hip_metadata_t md;
  int gamut;
  const uint8_t* exif;
  size_t exif_len;
  uhdr_hip_image_t dec[2];     // the decoded primary image and gain map
  size_t dec_bytes[2], out_bytes[2];
};
size_t edit_file_bytes(const EditFile& f) {
  return round_up(f.dec_bytes[0], 256) + round_up(f.dec_bytes[1], 256) + round_up(f.out_bytes[0], 256) + round_up(f.out_bytes[1], 256);
}

int edit_round(DeviceState* cx, hipStream_t s, EditFile* f, int m, const uhdr_hip_effect_t* const fx[2], const int n_fx[2], int quality,
               void* const* out, const size_t* out_capacity, size_t* out_size, int* st_) {
  size_t bytes = 0;
  for (int k = 0; k < m; ++k) bytes += edit_file_bytes(f[k]);
  int rc;
  if ((rc = stage_reserve(cx, 4, bytes)) != 0) return rc;
  uint8_t* ws = static_cast<uint8_t*>(cx->stage[4]);
  // 1. the 2 m JPEGs through the batched decoder
  std::vector<const void*> jp(2 * (size_t)m);
  std::vector<size_t> jn(2 * (size_t)m), cap(2 * (size_t)m);
  std::vector<void*> dst(2 * (size_t)m), fxo(2 * (size_t)m);
  std::vector<uhdr_hip_image_t> dec(2 * (size_t)m), edited(2 * (size_t)m);
  std::vector<int> dst_st(2 * (size_t)m, 0);
  size_t o = 0;
  for (int k = 0; k < m; ++k)
    for (int p = 0; p < 2; ++p) {
      const size_t q = 2 * (size_t)k + p;
      jp[q] = f[k].jpg[p]; jn[q] = f[k].len[p];
      dst[q] = ws + o; cap[q] = f[k].dec_bytes[p];
      o += round_up(f[k].dec_bytes[p], 256);
      fxo[q] = ws + o;
      o += round_up(f[k].out_bytes[p], 256);
    }
  (void)uhdr_hip_jpeg_decode_batch(2 * m, jp.data(), jn.data(), UHDR_HIP_DECODE_TO_YCBCR, dst.data(), cap.data(), dec.data(), dst_st.data(),
                                   UHDR_HIP_MEM_DEVICE, s);
  // 2. both chains of every file that decoded: one launch
  std::vector<FxcItem> items(2 * (size_t)m);
  for (int k = 0; k < m; ++k) {
    const size_t q = 2 * (size_t)k;
    if (dst_st[q] != UHDR_HIP_NO_ERROR || dst_st[q + 1] != UHDR_HIP_NO_ERROR) st_[f[k].idx] = UHDR_HIP_ERROR_DECODE_ERROR;
    dec[q + 1].pixelFormat = UHDR_HIP_PIX_FMT_MONOCHROME;   // (a gain map with chroma planes: its luma)
    dec[q + 1].chroma_data = nullptr;
    for (int p = 0; p < 2; ++p) {
      FxcItem& it = items[q + p];
      it.in = &dec[q + p]; it.fx = fx[p]; it.n_fx = n_fx[p]; it.out = fxo[q + p]; it.cap = f[k].out_bytes[p]; it.out_img = &edited[q + p];
      if (st_[f[k].idx] == UHDR_HIP_NO_ERROR) fx_item_prepare(&it);
      else it.status = st_[f[k].idx];
    }
  }
  if ((rc = fx_items_run(items, 2 * kFxChainRound, s)) != UHDR_HIP_NO_ERROR) return rc;
  // 3. API-x over the files still standing
  std::vector<uhdr_hip_image_t> yuv, map;
  std::vector<uhdr_hip_metadata_t> md;
  std::vector<const void*> exif;
  std::vector<size_t> exif_n, ocap, osize;
  std::vector<void*> optr;
  std::vector<int> who, xst;
  uint8_t probe_byte = 0;
  for (int k = 0; k < m; ++k) {
    const size_t q = 2 * (size_t)k;
    const int i = f[k].idx;
    if (st_[i] == UHDR_HIP_NO_ERROR) st_[i] = items[q].status != UHDR_HIP_NO_ERROR ? items[q].status : items[q + 1].status;
    if (st_[i] != UHDR_HIP_NO_ERROR) continue;
    edited[q].colorGamut = f[k].gamut;
    yuv.push_back(edited[q]); map.push_back(edited[q + 1]); md.push_back(f[k].md);
    exif.push_back(f[k].exif_len ? f[k].exif : nullptr); exif_n.push_back(f[k].exif_len);
    optr.push_back(out[i] ? out[i] : &probe_byte); ocap.push_back(out[i] ? out_capacity[i] : 0); osize.push_back(0);
    who.push_back(i); xst.push_back(0);
  }
  if (!who.empty()) {
    (void)uhdr_hip_jpegr_encode_apix_batch((int)who.size(), yuv.data(), map.data(), md.data(), quality, exif.data(), exif_n.data(), optr.data(),
                                           ocap.data(), osize.data(), xst.data(), UHDR_HIP_MEM_DEVICE, s);
    for (size_t k = 0; k < who.size(); ++k) { st_[who[k]] = xst[k]; out_size[who[k]] = osize[k]; }
  }
  HIP_TRY(hipStreamSynchronize(s));   // the workspace is the next round's
  return UHDR_HIP_NO_ERROR;
}
}  // namespace

extern "C" {

int uhdr_hip_jpegr_edit_batch(int n, const void* const* jpegr, const size_t* jpegr_size, const uhdr_hip_effect_t* sdr_effects, int n_sdr_effects,
                              const uhdr_hip_effect_t* gainmap_effects, int n_gainmap_effects, const int* sdr_gamut, int quality, void* const* out,
                              const size_t* out_capacity, size_t* out_size, int* status, void* stream) {
  if (n < 0 || n_sdr_effects < 0 || n_gainmap_effects < 0 || (n_sdr_effects > 0 && sdr_effects == nullptr) ||
      (n_gainmap_effects > 0 && gainmap_effects == nullptr) ||
      (n > 0 && (jpegr == nullptr || jpegr_size == nullptr || out == nullptr || out_capacity == nullptr || out_size == nullptr)))
    return UHDR_HIP_ERROR_BAD_PTR;
  if (quality < 0 || quality > 100) return UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR;
  const uhdr_hip_effect_t* const fx[2] = {sdr_effects, gainmap_effects};
  const int n_fx[2] = {n_sdr_effects, n_gainmap_effects};
  std::vector<int> st_((size_t)n, UHDR_HIP_NO_ERROR);
  try {
    // everything that needs no device: the split, the two headers, the metadata, the chains' own checks
    std::vector<EditFile> files;
    for (int i = 0; i < n; ++i) {
      out_size[i] = 0;
      if (jpegr[i] == nullptr || (out[i] == nullptr && out_capacity[i] != 0)) { st_[i] = UHDR_HIP_ERROR_BAD_PTR; continue; }
      const uint8_t* file = static_cast<const uint8_t*>(jpegr[i]);
      jpegr::Range img[2];
      const int found = jpegr::find_images(file, jpegr_size[i], img);
      if (found < 2) { st_[i] = found == 0 ? UHDR_HIP_ERROR_NO_IMAGES_FOUND : UHDR_HIP_ERROR_GAIN_MAP_IMAGE_NOT_FOUND; continue; }
      EditFile f = {};
      f.idx = i;
      for (int p = 0; p < 2; ++p) { f.jpg[p] = file + img[p].begin; f.len[p] = img[p].len; }
      files.push_back(f);
    }
    if (!files.empty()) {   // the headers, as size probes of the batched decoder (host work)
      const size_t m2 = 2 * files.size();
      std::vector<const void*> jp(m2);
      std::vector<size_t> jn(m2);
      std::vector<uhdr_hip_image_t> desc(m2);
      std::vector<int> pst(m2, 0);
      for (size_t k = 0; k < files.size(); ++k)
        for (int p = 0; p < 2; ++p) { jp[2 * k + p] = files[k].jpg[p]; jn[2 * k + p] = files[k].len[p]; }
      (void)uhdr_hip_jpeg_decode_batch((int)m2, jp.data(), jn.data(), UHDR_HIP_DECODE_TO_YCBCR, nullptr, nullptr, desc.data(), pst.data(),
                                       UHDR_HIP_MEM_DEVICE, stream);
      std::vector<EditFile> live;
      for (size_t k = 0; k < files.size(); ++k) {
        EditFile& f = files[k];
        const int i = f.idx;
        if (pst[2 * k] != UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE || pst[2 * k + 1] != UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE ||
            desc[2 * k].pixelFormat != UHDR_HIP_PIX_FMT_YUV420) { st_[i] = UHDR_HIP_ERROR_DECODE_ERROR; continue; }
        const uint8_t* xmp = nullptr;
        size_t xmp_len = 0;
        if (!jpegr::first_xmp(f.jpg[1], f.len[1], &xmp, &xmp_len) || !jpegr::metadata_from_xmp(xmp, xmp_len, &f.md)) { st_[i] = UHDR_HIP_ERROR_METADATA_ERROR; continue; }
        for (int p = 0; p < 2 && st_[i] == UHDR_HIP_NO_ERROR; ++p) {
          uhdr_hip_image_t d = desc[2 * k + p];
          f.dec_bytes[p] = fx_packed(d.pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME, d.width, d.height);
          if (p == 1) d.pixelFormat = UHDR_HIP_PIX_FMT_MONOCHROME;
          FxcPlan plan;
          fx_compose(d, fx[p], n_fx[p], &plan);
          st_[i] = plan.status;
          f.out_bytes[p] = plan.packed;
        }
        if (st_[i] != UHDR_HIP_NO_ERROR) continue;
        const uint8_t* icc = nullptr;
        size_t icc_len = 0;
        f.gamut = jpegr::first_icc(f.jpg[0], f.len[0], &icc, &icc_len) ? jpegr::gamut_from_icc(icc, icc_len) : UHDR_HIP_CG_UNSPECIFIED;
        if (f.gamut == UHDR_HIP_CG_UNSPECIFIED) f.gamut = sdr_gamut ? sdr_gamut[i] : UHDR_HIP_CG_UNSPECIFIED;
        size_t a, b, eo = 0, el = 0, c, d2;
        jpegr::first_packets(f.jpg[0], f.len[0], &a, &b, &eo, &el, &c, &d2);
        f.exif = el ? f.jpg[0] + eo : nullptr;
        f.exif_len = el;
        live.push_back(f);
      }
      if (!live.empty()) {
        size_t done = 0;
        const int rc = run_rounds(
            live.size(), (size_t)kFxChainRound, stream, [&](size_t k) { return edit_file_bytes(live[k]); },
            [&](DeviceState* cx, hipStream_t s, size_t r0, int m) {
              return edit_round(cx, s, &live[r0], m, fx, n_fx, quality, out, out_capacity, out_size, st_.data());
            },
            &done);
        for (size_t k = done; k < live.size(); ++k) st_[live[k].idx] = rc;
      }
    }
  } catch (const std::bad_alloc&) {
    return UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE;
  }
  return finish_statuses(st_, status);
}

}  // extern "C"
