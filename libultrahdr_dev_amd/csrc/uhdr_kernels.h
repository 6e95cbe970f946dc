// uhdr_kernels.h -- internal host<->kernel interface (POD kernel arguments + launchers).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace uhdr {

// Per image (321 KiB since round 4, 64 KiB before): header, then EITHER kStatLists lists of kStatCap entries (0.2 % of a 4K map's pixels are in doubt: ~1000 entries per
// image, ~16 per list).  Several lists per image because a wave appends with ONE returning atomic on its list's count, and atomics
// on one address are served one after the other at the memory side (~1 us each: a single count per image cost the kernel 30 %).
// kStatEst: in launches of few images every wave of an image starts at once, finds nothing published and publishes its estimates' extremes:
// thousands of atomics on two words, served one after the other (one 4K image: 80 us for a 10 us kernel).  Such launches
// (GenConsts::stat_spread: at most 16 images of at least 512 waves) publish to and prune by one pair of words per LIST instead;
// the others keep the single pair, which prunes better.
// Round 4: launches whose images have at most kStatSlotWaves waves each (a 4K frame at four spans per block: 1016) need no
// atomic at all -- every wave owns kStatSlotWords words behind the header (word 0 of them is unused) and one count word IN the
// header, at kStatSlotCnt + wave (written by every wave of every launch, so nothing has to be cleared; the resolve kernel ignores
// the words of waves the launch does not have); a wave with more entries than fit writes a count of 0, sets word 6 of the header
// and the image is swept.  The returning atomic cost the streaming kernel 17 us per 64 x 4K launch (0.435 ms against 0.418 with it compiled out,
// profiles/r02_generate_ab.txt): a wave waits a trip to the memory side for it before it can exit.  Other launches keep the lists.
// A wave's count word (kStatSlotCnt + wave): plain entries | saved entries << 8.  Its slots: [1, kStatSlotPlain]: plain entries (pair index << 3 | flags: the resolve
// kernel samples the pair again); then kStatSlotSaved entries of 16 words (64 B): (pair index << 3 | flags) and the pair AS SAMPLED --
// r, g, b, hr, hg, hb of both pixels, what the transfer functions start from -- written by the streaming kernel the moment its
// filter finds a pixel in doubt (the twelve floats are still in registers then), so that the resolve kernel reads one contiguous
// line per such pair instead of fourteen scattered ones (that round of reads was 14 of its 24 us).
constexpr uint32_t kStatSlotWaves = 1024, kStatSlotPlain = 15, kStatSlotSaved = 4, kStatSlotWords = 16 + 16 * kStatSlotSaved;
// (slot mode keeps the waves' count words side by side in front of the slots, kStatSlotCnt: the resolve kernel reads them as 4 KiB)
constexpr uint32_t kStatLists = 64, kStatCap = 252, kStatEst = 8 + kStatLists, kStatSlotCnt = kStatEst + 2 * kStatLists,
                   kStatHdr = kStatSlotCnt + kStatSlotWaves,
                   kStatWords = kStatHdr + (kStatLists * kStatCap > kStatSlotWaves * kStatSlotWords ? kStatLists * kStatCap : kStatSlotWaves * kStatSlotWords);
static_assert(kStatHdr % 4u == 0u && kStatSlotWords % 4u == 0u && kStatWords % 4u == 0u, "saved entries are read and written as 16-byte pieces");
static_assert(kStatSlotCnt % 4u == 0u, "k_generate_resolve reads four waves' count words as one 16-byte piece");
constexpr int kMaxChunk = 64;  // images per launch (descriptors travel in the 4 KiB kernarg segment: 64 x 56 B + consts)
// launch geometry of k_generate (threads per block, spans of kGenBlock pairs a block of a large launch walks) and the blocks
// k_generate_resolve spends per image; chosen in uhdr_kernels.hip, here because uhdr_hip_generate_probe reports them
constexpr int kGenBlock = 256, kGenTiles = 4;
constexpr uint32_t kResolveSlices = 16;

// ---- LUT mode (gainmapmath.cpp:21-64 static tables; opt-in) --------------------
// one device buffer per device, filled once at uhdr_hip_init() by k_build_luts: table[i] = f((float)i / (float)(N - 1))
constexpr uint32_t kLutSrgbInvN = 1024, kLutHlgInvN = 4096, kLutPqInvN = 4096, kLutHlgN = 65536, kLutPqN = 65536;
constexpr uint32_t kLutSrgbInv = 0, kLutHlgInv = kLutSrgbInv + kLutSrgbInvN, kLutPqInv = kLutHlgInv + kLutHlgInvN,
                   kLutHlg = kLutPqInv + kLutPqInvN, kLutPq = kLutHlg + kLutHlgN, kLutTotal = kLutPq + kLutPqN;
// FAST apply only (not the reference's tables): transfer functions as line segments (c0, c1), 8 bytes per cell (k_apply_s4).
// A channel is  code = OETF(EOTF_sRGB(c) * F) * 1023  with F = 2^E the gain factor.  Both OETFs are smooth, nearly linear
// functions of a POWER of their argument -- HLG of u = sqrt(x) (exactly linear below its junction), PQ of u = x^m1 (a rational
// function) -- so the path is  u = T(c) * 2^(g E),  T = EOTF^g  (g = 1/2 for HLG, m1 for PQ, 1 for the linear formats):
//   stage 1  T(c):     cell = the float's own exponent and top 4 mantissa bits (16 cells per octave: the sRGB toe makes T
//                      singular at 0, cells that follow the exponent hold a power law to a constant relative error, 6e-5 here);
//                      `(bits >> 16) & 0x0FF8` -- one SDWA v_and -- is the byte offset of the entry as it stands: five exponent
//                      bits (inputs are 0 or lie in [2^-31, 1]), 4 KiB; the pixels use the top few octaves: 1-2 entries per bank.
//                      For g = 1 (linear output formats, calls whose values may pass 1.0) 16 cells per octave are too coarse:
//                      that table takes its cell from the HALF-PRECISION bit pattern of c (bits 14..3: 128 cells per octave).
//   stage 2  code(u):  129 UNIFORM cells over 2 + 2u in [2, 4] -- the cell is byte 2 of the float itself -- each entry
//                      replicated into 32 lane slots in LDS (cell * 256 + (lane & 31) * 8): no bank conflicts whatever the data.
//                      The entry evaluates to -(2 + n 2^-22), n the integer code (the kernel rounds toward zero), whose bits are
//                      0xC0000000 | n: red as it stands (alpha included), green and blue after a shift that drops the upper bits.
// Appended to the LUT buffer by uhdr_hip_init; byte sizes are multiples of 16.
constexpr uint32_t kTabS1Bytes = 0x3C00 + 16;                    // g = 1, half-precision cells up to 1.0
constexpr uint32_t kTabS1PowBytes = 512u * 8u;                   // g < 1: cell = (exponent & 31) << 4 | top 4 mantissa bits (inputs are 0 or in [2^-31, 1])
constexpr uint32_t kTabS2Cells = 129, kTabS2Floats = 260;        // 129 x (c0, c1), padded
constexpr uint32_t kTabS2LdsBytes = kTabS2Cells * 256u;          // replicated
constexpr uint32_t kTabS1Lin = kLutTotal, kTabS1Hlg = kTabS1Lin + kTabS1Bytes / 4, kTabS1Pq = kTabS1Hlg + kTabS1PowBytes / 4,
                   kTabS2Hlg = kTabS1Pq + kTabS1PowBytes / 4, kTabS2Pq = kTabS2Hlg + kTabS2Floats, kTabEnd = kTabS2Pq + kTabS2Floats;
// LUT-mode apply, scale 4: what becomes of an OETF table entry is its 10-bit code, (uint32_t)(table[i] * 1023.0f) & 0x3ff
// (gainmapmath.cpp:722-727) -- the 65536 codes of a table are 128 KiB of uint16 and fit into a workgroup's LDS where the 256 KiB of
// floats do not.  Built once per device behind the float tables (k_build_lut_codes).
constexpr uint32_t kCodeHlg = kTabEnd, kCodePq = kCodeHlg + kLutHlgN / 2, kLutBufferFloats = kCodePq + kLutPqN / 2;
constexpr uint32_t kGainLutN = 1024;  // kGainFactorNumEntries, gainmapmath.h:149-150

// ---- generate ----------------------------------------------------------------------------------
struct GenConsts {
  float sdr_cr, sdr_gcb, sdr_gcr, sdr_cb;  // SDR YUV->RGB (gamut of the SDR image, or 601)
  float hdr_cr, hdr_gcb, hdr_gcr, hdr_cb;  // HDR YUV->RGB (gamut of the P010 image)
  float lum_r, lum_g, lum_b;               // luminance of the SDR gamut (used for both images)
  float gm[9];                             // HDR->SDR gamut matrix
  int gm_identity;
  float hdr_white_nits;
  float bias4096;                          // == 4096.0f (kept opaque to the optimizer, see gen_pair)
  float min_boost, max_boost, log2_min, log2_max;
  // encode_gain_guarded: 255/(double)(log2_max - log2_min) and the bytes of gain == min / gain == max
  double enc_scale;
  uint32_t enc_byte_min, enc_byte_max;
  uint32_t width, height, map_w, map_h;
  uint32_t* stat_keys;  // 2 words per image of the launch (min key, max key), or nullptr
  uint32_t stat_stride; // words between the key pairs of consecutive images (2 in a caller's min/max array)
  // filtered kernel (always): per image kStatWords words -- [0] ~key of the smallest ESTIMATE seen, [1] key of the largest,
  // [3] slices of k_generate_resolve that have finished, [4] [5] the exact keys (stat_keys points here, stat_stride = kStatWords),
  // [8 + l] entries in list l, [kStatEst + 2 l], [kStatEst + 2 l + 1] words 0 and 1 once more per list (launches of few images),
  // [kStatHdr + l * kStatCap ..] list l: pairs with a pixel in doubt or a statistics candidate (a block
  // appends to list blk % kStatLists; a count beyond kStatCap means: sweep the image).  k_generate_resolve
  // redoes them on the exact path, writes the image's (min, max) to stat_out (when not null) and clears the header for the next
  // launch: no memset and no finalize kernel around the launch.
  uint32_t* stat_ws;
  float* stat_out;
  const float* lut;     // device LUT buffer (LUT mode only)
  // f32 pre-filter of the exact path (see gen_pair): code-value scale, half-width of the "too close to an integer"
  // band, and the gains below / above which the clamp certainly applies
  float flt_scale, flt_delta, flt_lo, flt_hi;
  float flt_gain_rel;   // 2 x kRel: how far (relatively) a filter estimate of the gain may sit from the exact one
  uint32_t stat_spread; // the estimates' extremes are published per list (kStatEst): launches of few, large images
  uint32_t stat_slots;  // != 0: the waves of an image (this many, <= kStatSlotWaves) append to slots of their own, no atomics (above)
};
struct EvalConsts {
  float min_boost, max_boost, log2_min, log2_max;
  double enc_scale;
  uint32_t enc_byte_min, enc_byte_max;
  const float* lut;
  double log2_min_d, log2_max_d;
};
struct GenImage {  // 56 bytes; the V plane is u + c_stride * (height / 2) (gainmapmath.cpp:568)
  const uint8_t* y;
  const uint8_t* u;
  const uint16_t* hy;
  const uint16_t* huv;
  uint8_t* map;
  uint32_t y_stride, c_stride, hy_stride, huv_stride;
};
struct GenBatch {
  GenImage img[kMaxChunk];
};

// ---- content-adaptive generate ---------------------------------------------
// Two passes over a caller-provided workspace: k_generate_gains leaves every map pixel's exact unclamped f32 gain there and the
// images' extremes as keys; k_adaptive_consts turns the extremes into each image's boost range and encodeGain constants -- on the
// device, the range never visits the host --; k_encode_gains turns the stored gains into bytes.
struct AdaptConsts {   // what generate_consts / encode_constants compute on the host for a fixed range
  float min_boost, max_boost, log2_min, log2_max;
  double enc_scale;
  uint32_t enc_byte_min, enc_byte_max;
};
struct EncGainImage {
  const float* gains;   // map_w * map_h floats, 16-byte aligned
  uint8_t* map;
};
struct EncGainBatch {
  EncGainImage img[kMaxChunk];
};
static_assert(sizeof(AdaptConsts) == 32, "one image's constants are read as two 16-byte pieces");

// ---- apply -------------------------------------------------------------------------------------
// constants of the FAST scale-4 kernel (see k_apply_s4): wD[oy][pair][k-2] = (w_k(ox=2*pair), w_k(ox=2*pair+1)) * A / 255
// E = B + A255 * m1 + sum_{k=2..4} (m_k - m1) * wD[.][.][k-2][.]   (m: the four map bytes as floats; the weights of a cell sum to 1)
struct AppFast {
  float A, B, A255;
  float wD[4][2][3][2];
};
struct AppConsts {
  uint32_t width, height, map_w, map_h, scale;
  uint32_t cells_per_thread;      // k_apply_s4: map cells a thread walks (set by launch_apply from the size of the launch)
  uint32_t step_x, step_y;        // k_apply_s4: a block's 512 cells as (rows, columns) of the map: 512 = step_y * map_w + step_x
  float display_boost, inv_display_boost, max_boost, inv_max_boost;
  double log2_min_d, log2_max_d;  // log2((double)minContentBoost), log2((double)maxContentBoost)
  const float* idw;               // device: 4 tables (std, NR, NB, C) of scale*scale*4 floats
  const float* lut;               // device LUT buffer (LUT mode only)
  const float* tab;               // device: the LUT buffer (line-segment tables at kTabS1* / kTabS2*), FAST scale-4 kernel
  float lut_boost_factor;         // GainLUT(metadata, displayBoost): displayBoost > 0 ? displayBoost / max : 1 (gainmapmath.h:162)
  uint32_t lut_plain_div;         // LUT mode: x / display_boost may run as the IEEE expansion WITHOUT its operand scaling (lut_cell_pk):
                                  // the operands of this call cannot reach the ranges in which v_div_scale_f32 rescales them
  uint32_t* ex_ws;                // EXACT mode behind the f32 pre-filter: the lists of pixels in doubt (layout below), or nullptr
  uint32_t ex_cap;                // entries per list
  AppFast fast;
  uint32_t map_stride;            // k_apply_px_rgb: pixels between the rows of the RGBA map (the single-channel kernels: rows of map_w bytes)
};
// EXACT apply's workspace, one per stream: kMaxChunk headers of kExHdrWords words (word 3: slices of k_apply_resolve that have
// finished; words 8 ..: the lengths of the image's kExLists lists), then kMaxChunk x kExLists lists of ex_cap pixel indices.  The
// headers sit in front so that their place does not depend on the image size: every launch leaves them cleared.
constexpr uint32_t kExLists = 1024;
constexpr uint32_t kExHdrWords = 8 + kExLists;
constexpr uint32_t kExSlices = 256;   // blocks of k_apply_resolve per image (here because uhdr_hip_apply_exact_probe reports it)
inline size_t ex_ws_bytes(uint32_t cap) { return ((size_t)kMaxChunk * kExHdrWords + (size_t)kMaxChunk * kExLists * cap) * 4u; }
// capacity for a sixteenth of the image's pixels (the filter leaves ~1 % in doubt), spread over the lists
inline uint32_t ex_list_cap(uint64_t pixels) { return (uint32_t)(pixels / 16u / kExLists) + 64u; }
struct AppImage {
  const uint8_t* y;
  const uint8_t* u;
  const uint8_t* v;
  const uint8_t* map;
  void* dst;
  uint32_t y_stride, c_stride;
  // pixel (x, y) takes the chroma sample (x >> csx, y >> csy): 1, 1 for 4:2:0; 0, 0 for 4:4:4; 1, 0 for 4:2:2; 0, 1 for 4:4:0.  Only
  // the per-pixel kernels read them: the scale-4 kernels are 4:2:0's (app_fast_s4)
  uint32_t csx, csy;
};
struct AppBatch {
  AppImage img[kMaxChunk];
};

// ---- toneMap / convertYuv ----------------------------------------------------------------------
struct ToneImage {
  const uint16_t* sy;
  const uint16_t* suv;
  uint8_t* dy;
  uint8_t* du;
  uint8_t* dv;
  uint32_t sy_stride, suv_stride, dy_stride, dc_stride;
  uint32_t width, height;
};
constexpr int kToneChunk = 32;  // images per toneMap / convertYuv launch (grid.z = image; 32 x 112 B of descriptors)
struct ToneBatch {
  ToneImage img[kToneChunk];
};
// Tone-mapped SDR base image (no reference counterpart): the launches take a ToneBatch of equally sized
// images of one gamut and these constants.  Image z of a launch owns headroom[slot[z]].
struct ToneSdrConsts {
  float cr, gcb, gcr, cb;       // the HDR gamut's YUV -> RGB (gainmapmath.cpp:142-146 and its siblings)
  float lr, lg, lb;             // the same gamut's RGB -> YUV (:131-134): luma weights,
  float ycb, rycb, ycr, rycr;   // the Cb and Cr divisors and their reciprocals
  float k;                      // hdr white / 203
  float* headroom;              // the caller's array: max of the gamma-domain channels (k_tonemap_peak), then H
  uint32_t slot[kToneChunk];
};
// the headroom slots are set and finished kToneHeadChunk at a time: h[i] = 0 (measured) or the given H of slot i
constexpr int kToneHeadChunk = 512;
struct ToneHeadInit {
  float h[kToneHeadChunk];
};
struct CvtImage {
  uint8_t* y;   // where the converted planes go ...
  uint8_t* u;
  uint8_t* v;
  uint32_t y_stride, c_stride, width, height;
  float m[9];
  const uint8_t* sy;   // ... and where the samples come from: the same planes (JpegR::convertYuv works in place), or the caller's
  const uint8_t* su;   // image when the conversion is also the private copy encodeJPEGR API-1 takes first (jpegr.cpp:297-358)
  const uint8_t* sv;
  uint32_t sy_stride, sc_stride;
};
struct CvtBatch {   // m, width, height are taken from img[0]: one launch converts equally sized images between the same encodings
  CvtImage img[kToneChunk];
};

// ---- editorhelper effects (crop / mirror / rotate / resize): byte gathers over planes ---------------
enum FxOp : int { FX_COPY = 0, FX_FLIP_V, FX_FLIP_H, FX_ROT90, FX_ROT180, FX_ROT270, FX_RESIZE };
struct FxJob {            // dst[i][j] = src[f(i, j)] for i < rows, j < cols
  const uint8_t* src;
  uint8_t* dst;
  uint32_t rows, cols, dst_stride, src_stride;
  uint32_t in_w, in_h;    // extent of the source plane the index maps refer to
  uint32_t row_num, row_den, col_num, col_den;  // FX_RESIZE: src row = i*row_num/row_den, src col = j*col_num/col_den
  int op;
};
struct FxJobs {
  FxJob job[3];
  int n;
};

// A whole chain of effects as one gather: dst[i][j] = src[a[i] + b[j]], one job per output plane (k_effect_chain).  The tables hold
// byte offsets from `src`; `b` is padded to a multiple of 16 entries.  The host picks the column-pattern class and has checked,
// before the launch, that every a[i] + b[j] lies in [lo, hi] and that [lo, hi] lies inside the plane the caller described.
enum FxChainClass : int {
  FXC_GATHER = 0,  // anything: one byte load per output byte
  FXC_ASC,         // b[j] = b[0] + j: aligned 16-byte pieces
  FXC_DESC,        // b[j] = b[0] - j: 16-byte pieces, bytes reversed
  FXC_LDS,         // b monotone, at most 16 KiB between the ends of any 4096 columns (resize): gathered from a copy of the row stretch in LDS
  FXC_TILE         // a monotone, less than 256 bytes between the ends of any 64 rows, b far apart (odd number of quarter turns): 64 x 64 LDS tile
};
struct FxChainJob {
  const uint8_t* src;
  uint8_t* dst;
  const uint32_t* a;   // [rows]
  const uint32_t* b;   // [cols rounded up to 16]
  uint32_t rows, cols, dst_stride;
  uint32_t lo, hi;     // the smallest and the largest source offset of the job: nothing outside [src + lo, src + hi] is ever read
  int cls;
};
constexpr int kFxChainRound = 64;   // images per round of uhdr_hip_add_effects_batch (three plane jobs each)

// ---- general gain-map metadata: what k_apply_px_md / k_generate_md take beside the usual constants ----
struct AppMdConsts {       // out = max(0, (e + off_sdr) * 2^(A g' + B) - off_hdr_d),  g' = g^inv_gamma
  float A, B;              // (log2 max - log2 min) W  and  log2 min W - log2 d, formed in double
  float inv_gamma;
  float off_sdr, off_hdr_d;   // offsetSdr; offsetHdr / d
  uint32_t gamma_on;       // gamma != 1: selects the kernel with the v_log_f32 / v_exp_f32 pair
};
struct GenMdConsts {
  float off_sdr_nits, off_hdr_nits;   // offset * 203.0f, in f32
  uint32_t gamma_on;                  // gamma != 1 (launch-uniform branch in encode_gain_md)
  uint32_t byte_min, byte_max;        // gamma != 1: the bytes of gain <= min / gain >= max
  double gamma, den;                  // (double)gamma; (double)(log2_max - log2_min)
};

// ---- gain maps from packed RGBA: what k_generate_packed takes in GenBatch's place ----
struct PackedImage {       // strides in pixels
  const uint32_t* sdr;     // RGBA8888
  const void* hdr;         // RGBA1010102 (a dword per pixel) or RGBA F16 (8 bytes per pixel)
  uint8_t* map;
  uint32_t sdr_stride, hdr_stride;
};
struct PackedBatch {
  PackedImage img[kMaxChunk];
};

// ---- tone-mapped SDR image from a packed HDR image: what k_tonemap_packed[_peak] take ----
struct TonePackedImage {   // strides in pixels
  const void* src;         // RGBA1010102 (a dword per pixel) or RGBA F16 (8 bytes per pixel)
  uint32_t* dst;           // RGBA8888
  uint32_t src_stride, dst_stride, width, height;
};
struct TonePackedBatch {   // equally sized images of one alignment class; image z owns headroom[slot[z]]
  TonePackedImage img[kToneChunk];
  uint32_t slot[kToneChunk];
  float* headroom;
  const float* table;      // RGBA1010102: the transfer function's kTonePackedCodes inverse-OETF values (16-byte aligned)
  float k;                 // hdr white / 203
};
constexpr uint32_t kTonePackedCodes = 1024;
constexpr uint32_t kTonePackedPeakGroups = 128;   // the most workgroup rows (of 4 image rows) the measuring pass spends per image
static_assert(sizeof(TonePackedBatch) <= 4096, "packed tone-map kernel arguments exceed the kernarg segment");

// ---- HDR from a packed SDR image and its gain map: what k_apply_packed_s4 / _px take in AppBatch's place ----
struct PackedAppImage {    // 32 bytes
  const uint32_t* sdr;     // RGBA8888, rows sdr_stride pixels apart
  const uint8_t* map;      // one byte per map pixel in rows of map_w bytes, or RGBA8888 (4-byte aligned) in rows of AppConsts::map_stride pixels
  void* dst;
  uint32_t sdr_stride;
  uint32_t pad_;
};
struct PackedAppBatch {
  PackedAppImage img[kMaxChunk];
};
constexpr uint32_t kSrgbCodes = 256;   // the table of srgbInvOetf(code * (1 / 255.0f)), built once per device by the exact function
// what becomes of a gain: the reference's applyGain in FAST or in the exact arithmetic, or general metadata's factor (AppMdConsts)
enum PackedApplyKind : int { kPackedFast = 0, kPackedExact = 1, kPackedMd = 2, kPackedMdGamma = 3 };
static_assert(sizeof(AppConsts) + sizeof(AppMdConsts) + sizeof(PackedAppBatch) + 16 <= 4096, "packed apply kernel arguments exceed the kernarg segment");

static_assert(sizeof(GenConsts) + sizeof(GenMdConsts) + sizeof(GenBatch) <= 4096, "generate kernel arguments exceed the kernarg segment");
static_assert(sizeof(GenConsts) + sizeof(GenMdConsts) + sizeof(PackedBatch) <= 4096, "generate kernel arguments exceed the kernarg segment");
static_assert(sizeof(AppConsts) + sizeof(AppMdConsts) + sizeof(AppBatch) + 16 <= 4096, "apply kernel arguments exceed the kernarg segment");
static_assert(sizeof(AppConsts) + sizeof(AppBatch) <= 4096, "apply kernel arguments exceed the kernarg segment");

// launchers (enqueue only; return hipError_t of the launch)
hipError_t launch_generate(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, bool lut,
                           bool filter, hipStream_t s);
// a launch of n images this size is too small to be worth k_generate_resolve's latency (a single 4K image: 13 us against 24)
bool generate_is_small(const GenConsts& c, int n);
bool generate_resolve_pays(const GenConsts& c, int n);   // a launch with statistics: the filtered kernel + k_generate_resolve beat the exact kernel
uint32_t generate_slot_waves(const GenConsts& c, int n);  // waves per image of the filtered + deferred launch of n such images, or 0 when they exceed kStatSlotWaves
hipError_t launch_stats_init(uint32_t* keys, int n, hipStream_t s);
// after every filtered launch: the pixels it left in doubt and its statistics candidates on the exact path
hipError_t launch_stats_resolve(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s);
constexpr size_t kStatWsBytes = sizeof(uint32_t) * kStatWords * (size_t)kMaxChunk;
hipError_t launch_stats_finalize(uint32_t* keys, int n, hipStream_t s);
// content-adaptive generate.  Keys: two words per image, ~key(min) and key(max), both only grow from 0 (publish_minmax).
hipError_t launch_adaptive_init(uint32_t* keys, uint32_t words, hipStream_t s);   // keys[0 .. words) = 0, as a kernel
// pass 1 of n <= kMaxChunk images of one size: GenImage::map points at the image's GAINS (float, 16-byte aligned), c.stat_keys at its keys
hipError_t launch_generate_gains(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s);
// per-channel (RGB) map of n <= kMaxChunk images of one size: GenImage::map points at map_w * map_h RGBA pixels, 4-byte aligned
// (aligned launches: 8-byte aligned, map_w even); the exact path throughout, no statistics
hipError_t launch_generate_rgb(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s);
// the range rule and the encode constants of n images from their keys.  per_call: one range from the extremes of all n images and of
// carry_in (two key words of earlier launches, or null); carry_out (or null) receives the merged pair.  content_minmax may be null.
hipError_t launch_adaptive_consts(const uint32_t* keys, int n, int per_call, float cap, AdaptConsts* consts, float* content_minmax,
                                  float* boost_range, const uint32_t* carry_in, uint32_t* carry_out, hipStream_t s);
// pass 2 of n <= kMaxChunk images of `pixels` map pixels each; consts[i] belongs to b.img[i]
hipError_t launch_encode_gains(const AdaptConsts* consts, const EncGainBatch& b, int n, uint32_t pixels, hipStream_t s);
// mode: 0 FAST, 1 EXACT, 2 LUT.  ex_phases: which kernels of EXACT's pair (c.ex_ws set) are enqueued -- kExPhaseEst the estimate
// (k_apply_s4_est or k_apply_px_est), kExPhaseResolve k_apply_resolve; every call but uhdr_hip_apply_exact_probe passes both
enum : unsigned { kExPhaseEst = 1u, kExPhaseResolve = 2u };
hipError_t launch_apply(const AppConsts& c, const AppBatch& b, int n, int fmt, int mode,
                        bool fast_s4, hipStream_t s, unsigned ex_phases = kExPhaseEst | kExPhaseResolve);
// the grid of that estimate kernel for n images: grid[0] = gridDim.x (blocks of 256 cells, or of 256 pixels of a row), grid[1] =
// gridDim.y of the per-pixel kernel (rows; the scale-4 kernel's is the image)
void apply_est_grid(const AppConsts& c, int n, bool fast_s4, uint32_t grid[2]);
// per-pixel apply of RGBA maps (AppImage::map 4-byte aligned, AppConsts::map_stride set): FAST or the unfiltered EXACT arithmetic
hipError_t launch_apply_rgb(const AppConsts& c, const AppBatch& b, int n, int fmt, bool exact, hipStream_t s);
// general metadata: per-pixel apply of one-plane maps (rows of map_w bytes) or RGBA maps (launch_apply_rgb's layout); one f32 arithmetic
hipError_t launch_apply_md(const AppConsts& c, const AppMdConsts& m, const AppBatch& b, int n, int fmt, bool rgb, hipStream_t s);
// packed apply (uhdr_packed_apply.hip).  table: kSrgbCodes floats (16-byte aligned), filled once per device ...
hipError_t launch_build_srgb_codes(float* table, hipStream_t s);
// ... and n <= kMaxChunk images of one size (and, for RGBA maps, one map stride).  kind: PackedApplyKind (m is read by the two
// general-metadata kinds only); rgb: RGBA maps.  strip: the scale-4 form -- c.scale == 4, c.width % 4 == 0 and every image's source
// and destination rows start on 16 bytes --, otherwise one pixel per lane at any scale factor and alignment
hipError_t launch_apply_packed(const AppConsts& c, const AppMdConsts& m, const PackedAppBatch& b, const float* table, int n, int fmt, int kind,
                               bool rgb, bool strip, hipStream_t s);
// general metadata: launch_generate_rgb's launch; rgb: its RGBA map, otherwise one byte per map pixel (aligned launches: 2-byte aligned)
hipError_t launch_generate_md(const GenConsts& c, const GenMdConsts& m, const GenBatch& b, int n, int hdr_tf, bool aligned, bool rgb,
                              hipStream_t s);
// packed RGBA inputs: launch_generate_md's launch and maps for n <= kMaxChunk pairs of one size; f16: the HDR images are RGBA F16
// (hdr_tf must be 0), otherwise RGBA1010102 (hdr_tf 1 or 2).  aligned: both images' rows start on 16 bytes, the width is a multiple
// of 8 and the map is aligned as launch_generate_md's
hipError_t launch_generate_packed(const GenConsts& c, const GenMdConsts& m, const PackedBatch& b, int n, int hdr_tf, bool f16, bool aligned,
                                  bool rgb, hipStream_t s);
// content-adaptive maps from packed RGBA, pass 1 of n <= kMaxChunk pairs of one size: launch_generate_packed's
// launch; PackedImage::map points at the image's GAINS (float, 16-byte aligned; 1 per map pixel, rgb: 3), c.stat_keys at its keys
hipError_t launch_generate_packed_gains(const GenConsts& c, const PackedBatch& b, int n, int hdr_tf, bool f16, bool aligned, bool rgb,
                                        hipStream_t s);
// pass 2 of such RGB maps: launch_encode_gains on three gains per map pixel, EncGainImage::map an RGBA8888 map (4-byte aligned)
hipError_t launch_encode_gains_rgb(const AdaptConsts* consts, const EncGainBatch& b, int n, uint32_t pixels, hipStream_t s);
// gain maps at any scale factor for n <= kMaxChunk pairs of one size; c.map_w / c.map_h are width / s and
// height / s.  mode 0: the single-channel map of the reference's metadata behind the f32 pre-filter (m is not read); 1: launch_generate_md's
// one-plane map; 2: its RGBA map -- both on the exact path.  aligned: gen_aligned's conditions, an even height and a map whose strip
// stores (8 / s map pixels) are aligned; it selects the 16-byte forms for s = 1, 2, 8 and is ignored for every other factor
struct GenScaleConsts {
  uint32_t s;      // the factor, 1 .. 128
  float area;      // (float)(s * s)
  uint32_t* doubt_count;   // null, or (uhdr_hip_generate_gainmap_scaled_probe) a device word: += the map pixels the filter left in doubt
};
constexpr int kScaledBlock = 256;   // threads per block of k_generate_scaled; a thread owns 8 / s map pixels (s = 1, 2, 8) or a pair
static_assert(sizeof(GenConsts) + sizeof(GenMdConsts) + sizeof(GenScaleConsts) + sizeof(GenBatch) <= 4096, "generate kernel arguments exceed the kernarg segment");
hipError_t launch_generate_scaled(const GenConsts& c, const GenMdConsts& m, const GenScaleConsts& sc, const GenBatch& b, int n, int hdr_tf,
                                  bool aligned, int mode, hipStream_t s);
hipError_t launch_build_luts(float* lut /* kLutTotal floats */, hipStream_t s);
hipError_t launch_build_lut_codes(float* lut /* the whole buffer: reads the two OETF tables, writes kCodeHlg / kCodePq */, hipStream_t s);
// GainLUT table (kGainLutN floats, device) for (log2 min, log2 max, boost factor)
hipError_t launch_build_gain_lut(float* table, double log2_min, double log2_max, float boost_factor, hipStream_t s);
hipError_t launch_tonemap(const ToneBatch& b, int n, bool aligned, hipStream_t s);      // n <= kToneChunk images of equal width / height
hipError_t launch_convert_yuv(const CvtBatch& b, int n, bool aligned, hipStream_t s);
static_assert(sizeof(CvtBatch) <= 4096 && sizeof(ToneBatch) <= 4096, "toneMap / convertYuv kernel arguments exceed the kernarg segment");
// tone-mapped SDR base image.  headroom[0 .. n) = v.h (n <= kToneHeadChunk) ...
hipError_t launch_tonemap_head_init(float* headroom, const ToneHeadInit& v, int n, hipStream_t s);
// ... pass 1 over the measured images (n <= kToneChunk of equal width / height, both even): headroom[slot] = max(headroom[slot], m') ...
hipError_t launch_tonemap_peak(const ToneSdrConsts& c, const ToneBatch& b, int n, bool aligned, hipStream_t s);
// ... every slot with v.h[i] == 0 from m' to H = min(max(invOETF(m') * k, 1), cap) ...
hipError_t launch_tonemap_head_finish(float* headroom, const ToneHeadInit& v, int n, int hdr_tf, float k, float cap, hipStream_t s);
// ... and the planes of n <= kToneChunk images
hipError_t launch_tonemap_sdr(const ToneSdrConsts& c, const ToneBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s);
static_assert(sizeof(ToneSdrConsts) + sizeof(ToneBatch) <= 4096 && sizeof(ToneHeadInit) + 64 <= 4096, "tone-map kernel arguments exceed the kernarg segment");
// the same operator on packed HDR images.  tab: 2 * kTonePackedCodes floats, the HLG table, then the PQ one (built once per device) ...
hipError_t launch_build_packed_tone_tables(float* tab, hipStream_t s);
// ... pass 1 over the measured images (n <= kToneChunk of one size; f16: RGBA F16, otherwise RGBA1010102).  aligned: source and
// destination rows start on 16 bytes and width % 4 == 0 ...
hipError_t launch_tonemap_packed_peak(const TonePackedBatch& b, int n, bool f16, bool aligned, hipStream_t s);
// ... and the pixels: hdr_tf 0 reads RGBA F16, 1 / 2 RGBA1010102 through b.table.  The slots are launch_tonemap_head_init / _finish's
hipError_t launch_tonemap_packed(const TonePackedBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s);
// decoded 4:2:0 planes -> RGBA8888 with libjpeg-turbo's arithmetic; w, h even, strides in bytes: up to kRgbaChunk images of any
// (even) sizes in one launch (k_ycc420_rgba_batch: grid.z = image)
constexpr int kRgbaChunk = 64;
struct YccRgbaImage {
  const uint8_t* y;
  const uint8_t* cb;
  const uint8_t* cr;
  uint8_t* rgba;        // w * h * 4 bytes, rows packed
  uint32_t w, h, ys, cs;
};
struct YccRgbaBatch {
  YccRgbaImage img[kRgbaChunk];
};
static_assert(sizeof(YccRgbaBatch) <= 4096, "k_ycc420_rgba_batch's kernel arguments exceed the kernarg segment");
hipError_t launch_ycc420_to_rgba_batch(const YccRgbaBatch& b, int n, hipStream_t s);
// the same for decoded 4:4:4, 4:2:2 and 4:4:0 planes of any size, odd ones included (k_yccx_rgba_batch); an image's sampling is
// (hs, vs) = the luma samples per chroma sample across and down, its chroma planes are ceil(w / hs) x ceil(h / vs).  plain: the chroma
// is replicated instead of filtered -- what libjpeg does for planes of a decode at 1/8 (jinit_upsampler: fancy upsampling needs an IDCT
// size above 1)
struct YccxRgbaImage {
  YccRgbaImage im;
  uint32_t hs, vs;
  uint32_t plain;
};
struct YccxRgbaBatch {
  YccxRgbaImage img[kRgbaChunk];
};
static_assert(sizeof(YccxRgbaBatch) <= 4096, "k_yccx_rgba_batch's kernel arguments exceed the kernarg segment");
hipError_t launch_yccx_to_rgba_batch(const YccxRgbaBatch& b, int n, hipStream_t s);
hipError_t upload_idw4(const float* tables /* 4*64 floats */);
hipError_t launch_effect(const FxJobs& j, hipStream_t s);
// dev_jobs: n descriptors in DEVICE memory (a round is not bounded by the kernarg segment); host_jobs: the same descriptors, read
// here for the grid's size only
hipError_t launch_effect_chain(const FxChainJob* dev_jobs, const FxChainJob* host_jobs, int n, hipStream_t s);
hipError_t launch_eval_transfer(int fn, const float* in, float* out, size_t n, const EvalConsts& ec, hipStream_t s);
hipError_t launch_synth_lcg(uint16_t* p010, uint8_t* yuv, uint32_t n_luma, uint32_t n, uint32_t seed, hipStream_t s);

}  // namespace uhdr
