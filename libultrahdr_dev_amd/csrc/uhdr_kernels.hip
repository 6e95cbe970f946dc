// uhdr_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the Ultra HDR gain-map path.
//
//   k_generate<TF,ALIGNED>   UltraHdr::generateGainMap hot loop   (ref lib/src/ultrahdr.cpp:308-338)
//   k_apply_s4<FMT,MASK>     UltraHdr::applyGainMap hot loop, scale 4, FAST arithmetic (:427-496)
//   k_apply_px<FMT,EXACT>    same loop, any integer scale / any alignment / EXACT arithmetic
//   k_apply_s4_est, k_apply_px_est, k_apply_resolve   EXACT arithmetic as an f32 estimate + the exact path on the pixels in doubt
//   k_apply_lut_s4, k_apply_lut   the loops with the reference's LUT accessors (opt-in LUT mode)
//   k_apply_px_md, k_generate_md   gain maps with gamma, offsets and an HDR capacity range (no reference counterpart)
//   k_generate_packed        gain maps from packed RGBA pairs: RGBA8888 with RGBA1010102 or RGBA F16 (no reference counterpart)
//   k_generate_packed_gains, k_encode_gains_rgb   the same pairs against the boost range their content has
//   k_tonemap_*              UltraHdr::toneMap                    (:517-558)
//   k_tonemap_packed[_peak]  the tone-mapped SDR image of a packed HDR image: RGBA1010102 / RGBA F16 -> RGBA8888 (no reference counterpart)
//   k_convert_yuv<ALIGNED>   JpegR::convertYuv + transformYuv420  (lib/src/jpegr.cpp:1199-1203,
//                                                                  lib/src/gainmapmath.cpp:483-520)
//   k_effect, k_effect_rot   crop / mirror / rotate / resize      (lib/src/editorhelper.cpp:26-360)
//   k_effect_chain           a whole chain of them as one gather  (lib/src/editorhelper.cpp:362-446)
//   k_eval_transfer          scalar transfer functions over arrays (diagnostics for the exhaustive tests)
//
// All of it is pointwise byte/float work: no MFMA.  Measured: generate runs within 10 % of what its own
// read pattern reaches on the same box, apply 3-8 % above a build of itself without arithmetic (its writes cap at 5.5 TB/s);
// both got there by taking work off the VALU -- an f32 pre-filter with the exact path deferred to a resolve kernel in generate,
// both transfer functions as line-segment tables in LDS in apply.  Design rules followed here:
//   * one wave64 reads whole contiguous row segments (16 B/lane for P010, 8 B/lane for 8-bit luma),
//     stores are 16 B/lane; no LDS round trip is needed because every input byte is consumed by
//     exactly one lane;
//   * every per-call variant (gamut matrices, transfer function, boosts) is a kernel argument held
//     in SGPRs or a template parameter -- never a per-lane function pointer;
//   * a batch of equally sized images is ONE launch (grid.y = image), descriptors in the kernarg
//     segment, so 64 frames x 2 kernels fill all 256 CUs without per-image launch gaps;
//   * compiled with -ffp-contract=off; float op order is the reference's.
#include "uhdr_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "uhdr_apply_px.h"
#include "uhdr_device_math.h"
#include "uhdr_wave_scan.h"

namespace uhdr {

// Shepard IDW weights for map scale 4: [table][oy*16 + ox*4 + k]; tables: 0 std, 1 no-right,
// 2 no-bottom, 3 corner (gainmapmath.h:184-228).  Filled by the host at uhdr_hip_init().
__constant__ float c_idw4[4 * 64];

// the standard table once more, arranged for two horizontally adjacent pixels per instruction:
// [oy][pair][tap][pixel of the pair] (an aligned 8-byte scalar load is one packed operand)
__constant__ float c_idw4p[64];

hipError_t upload_idw4(const float* tables) {
  float p[64];
  for (int oy = 0; oy < 4; ++oy)
    for (int pr = 0; pr < 2; ++pr)
      for (int k = 0; k < 4; ++k)
        for (int h = 0; h < 2; ++h) p[((oy * 2 + pr) * 4 + k) * 2 + h] = tables[oy * 16 + (2 * pr + h) * 4 + k];
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_idw4p), p, sizeof(p));
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_idw4), tables, sizeof(float) * 4 * 64);
}

constexpr float k876 = 1 / 876.0f;  // gainmapmath.cpp:598
constexpr float k896 = 1 / 896.0f;  // gainmapmath.cpp:599

// BT.601 YUV->RGB used by apply for every image (ultrahdr.cpp:431, gainmapmath.cpp:184-202)
constexpr float kP3YR = 0.299f, kP3YG = 0.587f, kP3YB = 0.114f;
constexpr float kP3Cb = 1.772f, kP3Cr = 1.402f;
constexpr float kP3GCb = kP3YB * kP3Cb / kP3YG;
constexpr float kP3GCr = kP3YR * kP3Cr / kP3YG;

// two floats per lane: v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 process both in one 4-cycle issue slot
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float v) { return (f2){v, v}; }
// one half of a pair in both lanes of a packed operand (VOP3P op_sel / op_sel_hi: no instruction)
__device__ __forceinline__ f2 bc_lo(f2 v) { return __builtin_shufflevector(v, v, 0, 0); }
__device__ __forceinline__ f2 bc_hi(f2 v) { return __builtin_shufflevector(v, v, 1, 1); }

// packed add / mul with the VOP3P clamp modifier: both lanes saturate to [0, 1] for free (hipcc only
// folds clamps into scalar ops, so these two are spelled out)
__device__ __forceinline__ f2 pk_add_sat(f2 a, f2 b) {
  f2 r;
  asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f2 pk_mul_sat(f2 a, f2 b) {
  f2 r;
  asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f2 pk_fma_sat(f2 a, f2 b, f2 c) {
  f2 r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// a * b + (c.lo, c.lo) or (c.hi, c.hi), clamped: VOP3P's op_sel broadcasts one half of the third operand for free
template <int HI>
__device__ __forceinline__ f2 pk_fma_sat_bc(f2 a, f2 b, f2 c) {
  f2 r;
  if (HI) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,1,1] clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,1,0] clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}


// =================================================================================================
// LUT mode: the reference's table accessors (gainmapmath.cpp:162-171,269-277,292-302,316-324,344-354) and
// GainLUT (gainmapmath.h:151-182).  Everything here is float/integer arithmetic plus table reads, so the
// LUT pipelines are bit-exact by construction once the tables are (they are built by the exact functions).
// =================================================================================================
// `uint32_t value = static_cast<uint32_t>(e * (N - 1) + 0.5); value = CLIP3(value, 0, N - 1);`
// float product, double sum, truncation.  Outside [0, 2^32) the C++ conversion is undefined; the oracle pins
// what the reference's x86-64 build does (64-bit cvttsd2si, low word kept) and this restates it.
__device__ __attribute__((noinline)) uint32_t lut_index_wild(float t) {
  const double pos = (double)t + 0.5;
  uint32_t v = 0u;  // NaN, inf and |pos| >= 2^63 convert to 0x8000000000000000: low word 0
  if (__builtin_fabs(pos) < 9223372036854775808.0) v = (uint32_t)(long long)pos;
  return v;
}
// floor(t + 0.5) in ONE instruction: v_cvt_rpi_i32_f32 rounds to the nearest integer, ties toward +infinity, with no intermediate
// rounding -- for every float in [0, 2^31) and for -0 the value of (uint32_t)((double)t + 0.5), the reference's expression
// (scripts/ab/cvt_rpi_check.hip compares all 1.3e9 of them; tests/test_gpu_lut.py through eval case 40).  The f64 form costs
// v_cvt_f64_f32 + v_add_f64 + v_cvt_u32_f64.
__device__ __forceinline__ uint32_t round_half_up(float t) {
  int r;
  asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(t));
  return (uint32_t)r;
}
__device__ __forceinline__ uint32_t lut_index(float e, uint32_t n) {
  const float t = e * (float)(n - 1u);
  uint32_t v;
  if (__builtin_expect(__float_as_uint(t) < 0x4F000000u, 1)) v = round_half_up(t);  // +0 <= t < 2^31
  else v = lut_index_wild(t);
  return min(v, n - 1u);
}
// e in [0, 1] (what clampPixelFloat returns: the sRGB lookups of apply): no clip can bite and the conversion is in range
__device__ __forceinline__ uint32_t lut_index_unit(float e, uint32_t n) {
  return round_half_up(e * (float)(n - 1u));
}
// GainLUT::mGainTable[idx] (gainmapmath.h:153-168); boost_factor == 1.0f reproduces the one-argument constructor
__device__ __forceinline__ float gain_lut_entry(uint32_t idx, double log2_min, double log2_max, float boost_factor) {
  const float value = (float)idx / (float)(kGainLutN - 1u);
  const float log_boost = (float)(log2_min * (double)(1.0f - value) + log2_max * (double)value);
  return (float)exp2((double)(log_boost * boost_factor));
}

__global__ void __launch_bounds__(256) k_build_luts(float* lut) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= kLutTotal) return;
  float y;
  if (i < kLutHlgInv) y = srgb_inv_oetf_exact((float)(i - kLutSrgbInv) / (float)(kLutSrgbInvN - 1u));
  else if (i < kLutPqInv) y = hlg_inv_oetf_exact((float)(i - kLutHlgInv) / (float)(kLutHlgInvN - 1u));
  else if (i < kLutHlg) y = pq_inv_oetf_exact((float)(i - kLutPqInv) / (float)(kLutPqInvN - 1u));
  else if (i < kLutPq) y = hlg_oetf_exact((float)(i - kLutHlg) / (float)(kLutHlgN - 1u));
  else y = pq_oetf_exact((float)(i - kLutPq) / (float)(kLutPqN - 1u));
  lut[i] = y;
}
hipError_t launch_build_luts(float* lut, hipStream_t s) {
  hipLaunchKernelGGL(k_build_luts, dim3((kLutTotal + 255u) / 256u), dim3(256), 0, s, lut);
  return hipGetLastError();
}
__global__ void __launch_bounds__(256) k_build_lut_codes(float* lut) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // 2 x 65536 entries
  const uint32_t t = i >> 16, k = i & 0xFFFFu;
  uint16_t* codes = reinterpret_cast<uint16_t*>(lut + (t ? kCodePq : kCodeHlg));
  codes[k] = (uint16_t)(0x3ffu & (uint32_t)(lut[(t ? kLutPq : kLutHlg) + k] * 1023.0f));
}
hipError_t launch_build_lut_codes(float* lut, hipStream_t s) {
  hipLaunchKernelGGL(k_build_lut_codes, dim3(2u * 65536u / 256u), dim3(256), 0, s, lut);
  return hipGetLastError();
}
__global__ void __launch_bounds__(256) k_build_gain_lut(float* table, double log2_min, double log2_max, float boost_factor) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < kGainLutN) table[i] = gain_lut_entry(i, log2_min, log2_max, boost_factor);
}
hipError_t launch_build_gain_lut(float* table, double log2_min, double log2_max, float boost_factor, hipStream_t s) {
  hipLaunchKernelGGL(k_build_gain_lut, dim3(kGainLutN / 256u), dim3(256), 0, s, table, log2_min, log2_max, boost_factor);
  return hipGetLastError();
}

// =================================================================================================
// generate
// =================================================================================================

template <int TF>
__device__ __forceinline__ float hdr_inv_oetf(float e) {
  if (TF == 1) return hlg_inv_oetf_guarded(e);
  if (TF == 2) return pq_inv_oetf_guarded(e);
  return e;  // ULTRAHDR_TF_LINEAR: identityConversion (ultrahdr.cpp:223-228)
}

// Two horizontally adjacent map pixels (index 0|1 of every array) from their 4x4 blocks, processed as one
// packed float2 wherever the arithmetic is float: both pixels run the identical IEEE operation sequence,
// so packing changes nothing but the issue count.  hy[k][r][0|1]: P010 luma cols (0,1)|(2,3) packed lo/hi
// 16 bits; huv[k][r][0|1]: (U,V) of chroma col 0|1 of chroma row r; y8[k][r]: 4 luma bytes; u8/v8[k][r]:
// 2 chroma bytes in bits 0-15.  Accumulation order is samplePixels' (gainmapmath.cpp:605-615): dy outer,
// dx inner, one running float sum per channel.
// float of the low / high 16-bit word of w in ONE instruction (SDWA operand select); hipcc emits an extract
// (v_and_b32_sdwa / v_lshrrev_b32) followed by v_cvt_f32_u32 for the plain C expression
__device__ __forceinline__ float cvt_word0(uint32_t w) {
  float r;
  asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(r) : "v"(w));
  return r;
}
__device__ __forceinline__ float cvt_word1(uint32_t w) {
  float r;
  asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(r) : "v"(w));
  return r;
}


// LUT: the inverse OETFs are the reference's table accessors (ultrahdr.cpp:230,238,319 with USE_*_LUT = 1), read
// from the LDS copies s_srgb (1024 entries) / s_hdr (4096 entries of the HLG or PQ table)
// FILTER: before the exact (f64) evaluation, the same chain is run with the f32 special-function unit.  Its gain is
// within kFilterRelErr of the exact one (bounds measured exhaustively per function), so the
// truncated code value can only differ when it lies within flt_delta of an integer; only waves holding such a
// pixel (or one whose clamp decision is in doubt) pay for the exact path.  Bytes are identical either way.
// Returns a mask: bit k (k = 0, 1) set <=> gain[k] is the exact (reference) unclamped gain; a clear bit means gain[k] is the
// filter's estimate, within GenConsts::flt_gain_rel of it -- unless bit 2 + k is set: that pixel is in doubt (FILTER only), its
// byte and gain are provisional.
// PART: the function in two halves, for the pairs the streaming kernel hands to k_generate_resolve WITH their sampled values:
// kGenFront stops in front of the transfer functions and returns their inputs in *mid (both pixels' r, g, b, hr, hg, hb -- what the
// filter and the exact path both start from), kGenBack takes them from *mid instead of sampling; kGenWhole with mid != nullptr runs
// as ever and leaves a copy in *mid.  kGenLinear (exact path only) stops in front of the luminances and returns in *mid the two
// LINEAR colours of both pixels -- SDR, and HDR converted into the SDR gamut --, which is where the per-channel map (k_generate_rgb)
// parts from the single-channel one.  kGenBackLinear is kGenLinear from the sampled values in *mid, as kGenBack: the packed-RGBA
// generate (k_generate_packed) samples its own two images and has no YUV -> RGB step.
constexpr int kGenWhole = 0, kGenFront = 1, kGenBack = 2, kGenLinear = 3, kGenBackLinear = 4;
struct GenMid { f2 r, g, b, hr, hg, hb; };
template <int TF, bool LUT, bool FILTER, bool DEFER = false, int PART = kGenWhole>
__device__ __forceinline__ uint32_t gen_pair(const GenConsts& c, const uint32_t (&hy)[2][4][2],
                                             const uint32_t (&huv)[2][2][2], const uint32_t (&y8)[2][4],
                                             const uint32_t (&u8)[2][2], const uint32_t (&v8)[2][2],
                                             uint8_t (&out)[2], float (&gain)[2], const float* s_srgb, const float* s_hdr,
                                             GenMid* mid = nullptr) {
  f2 r, g, b, hr, hg, hb;
  if (PART == kGenBack || PART == kGenBackLinear) {
    r = mid->r; g = mid->g; b = mid->b; hr = mid->hr; hg = mid->hg; hb = mid->hb;
  } else {
  f2 sy = splat(0.0f), su = splat(0.0f), sv = splat(0.0f);
  f2 hsy = splat(0.0f), hsu = splat(0.0f), hsv = splat(0.0f);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    f2 uf[2], vf[2], huf[2], hvf[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      // float(u - 128) * (1/255.0f)   (gainmapmath.cpp:579-580): ONE rounding of an exact product -- which is what
      // fma(float(u), k, -128 k) computes as well: 128 k is exact (a power of two times k), so the fma's unrounded value is
      // (u - 128) k exactly.  One packed fma in place of a packed subtract and a packed multiply, the same float.
      const f2 ub = (f2){(float)((u8[0][r] >> (8 * k)) & 0xffu), (float)((u8[1][r] >> (8 * k)) & 0xffu)};
      const f2 vb = (f2){(float)((v8[0][r] >> (8 * k)) & 0xffu), (float)((v8[1][r] >> (8 * k)) & 0xffu)};
      uf[k] = pk_fma(ub, splat(k255), splat(-128.0f * k255));
      vf[k] = pk_fma(vb, splat(k255), splat(-128.0f * k255));
      // float((x >> 6) - 64) * (1/896) - 0.5   (gainmapmath.cpp:593-600), evaluated as
      // fma(float(x & 0xFFC0), (1/896)/64, -64 (1/896)) - 0.5: the masked 16-bit word is 64 * (x >> 6), so one mask per
      // two samples and one SDWA word->float conversion per sample replace shift + mask + subtract + convert; both
      // constants are exact scalings of 1/896 by powers of two, so the fma rounds the reference's exact product
      // ((x >> 6) - 64) * (1/896) -- once, like the reference's multiply.  (Round 4: the fma form; a subtract and a
      // multiply before, 32 packed instructions more per pixel pair over the three places it applies.)
      const uint32_t m0 = huv[0][r][k] & 0xFFC0FFC0u, m1 = huv[1][r][k] & 0xFFC0FFC0u;
      const f2 hu = (f2){cvt_word0(m0), cvt_word0(m1)};
      const f2 hv = (f2){cvt_word1(m0), cvt_word1(m1)};
      huf[k] = pk_fma(hu, splat(k896 * 0.015625f), splat(-64.0f * k896)) - splat(0.5f);
      hvf[k] = pk_fma(hv, splat(k896 * 0.015625f), splat(-64.0f * k896)) - splat(0.5f);
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const int dy = 2 * r + d;
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const f2 yb = (f2){(float)((y8[0][dy] >> (8 * dx)) & 0xffu), (float)((y8[1][dy] >> (8 * dx)) & 0xffu)};
        sy += yb * splat(k255);
        su += uf[dx >> 1];
        sv += vf[dx >> 1];
        const uint32_t w0 = hy[0][dy][dx >> 1] & 0xFFC0FFC0u, w1 = hy[1][dy][dx >> 1] & 0xFFC0FFC0u;
        const f2 hb = (dx & 1) ? (f2){cvt_word1(w0), cvt_word1(w1)} : (f2){cvt_word0(w0), cvt_word0(w1)};
        hsy += pk_fma(hb, splat(k876 * 0.015625f), splat(-64.0f * k876));   // ((x >> 6) - 64) * (1/876), one rounding (see above)
        hsu += huf[dx >> 1];
        hsv += hvf[dx >> 1];
      }
    }
  }
  // e / float(scale*scale): division by 16 == multiplication by 1/16 exactly
  sy *= splat(0.0625f); su *= splat(0.0625f); sv *= splat(0.0625f);
  hsy *= splat(0.0625f); hsu *= splat(0.0625f); hsv *= splat(0.0625f);

  // SDR: YUV->RGB (gainmapmath.cpp:142-146 shape), sRGB EOTF, luminance * 203 (ultrahdr.cpp:316-324)
  // clampPixelFloat (gainmapmath.cpp:115-118) rides on the last add of each expression: the sum is the same IEEE
  // operation, and min(max(x,0),1) differs from the reference's compare chain only in the sign of a zero,
  // which no later step can observe
  r = pk_add_sat(sy, splat(c.sdr_cr) * sv);
  g = pk_add_sat(sy - splat(c.sdr_gcb) * su, -(splat(c.sdr_gcr) * sv));
  b = pk_add_sat(sy, splat(c.sdr_cb) * su);
  // HDR: YUV->RGB (ultrahdr.cpp:326-327)
  hr = pk_add_sat(hsy, splat(c.hdr_cr) * hsv);
  hg = pk_add_sat(hsy - splat(c.hdr_gcb) * hsu, -(splat(c.hdr_gcr) * hsv));
  hb = pk_add_sat(hsy, splat(c.hdr_cb) * hsu);
  }
  static_assert((PART != kGenLinear && PART != kGenBackLinear) || (!LUT && !FILTER), "kGenLinear is the exact path's");
  if (PART != kGenBack && PART != kGenLinear && PART != kGenBackLinear && mid != nullptr) { mid->r = r; mid->g = g; mid->b = b; mid->hr = hr; mid->hg = hg; mid->hb = hb; }
  if (PART == kGenFront) return 0u;

  if (FILTER && !LUT) {
    const f2 fr = (f2){srgb_inv_oetf_fast(r.x), srgb_inv_oetf_fast(r.y)};
    const f2 fg = (f2){srgb_inv_oetf_fast(g.x), srgb_inv_oetf_fast(g.y)};
    const f2 fb = (f2){srgb_inv_oetf_fast(b.x), srgb_inv_oetf_fast(b.y)};
    const f2 fs = (splat(c.lum_r) * fr + splat(c.lum_g) * fg + splat(c.lum_b) * fb) * splat(203.0f);
    f2 qr = hr, qg = hg, qb = hb;
    if (TF == 1) {
      qr = (f2){hlg_inv_oetf_fast(hr.x), hlg_inv_oetf_fast(hr.y)};
      qg = (f2){hlg_inv_oetf_fast(hg.x), hlg_inv_oetf_fast(hg.y)};
      qb = (f2){hlg_inv_oetf_fast(hb.x), hlg_inv_oetf_fast(hb.y)};
    } else if (TF == 2) {
      qr = (f2){pq_inv_oetf_fast(hr.x), pq_inv_oetf_fast(hr.y)};
      qg = (f2){pq_inv_oetf_fast(hg.x), pq_inv_oetf_fast(hg.y)};
      qb = (f2){pq_inv_oetf_fast(hb.x), pq_inv_oetf_fast(hb.y)};
    }
    if (!c.gm_identity) {
      const f2 t0 = splat(c.gm[0]) * qr + splat(c.gm[1]) * qg + splat(c.gm[2]) * qb;
      const f2 t1 = splat(c.gm[3]) * qr + splat(c.gm[4]) * qg + splat(c.gm[5]) * qb;
      const f2 t2 = splat(c.gm[6]) * qr + splat(c.gm[7]) * qg + splat(c.gm[8]) * qb;
      qr = t0; qg = t1; qb = t2;
    }
    const f2 fh = (splat(c.lum_r) * qr + splat(c.lum_g) * qg + splat(c.lum_b) * qb) * splat(c.hdr_white_nits);
    uint32_t fbyte[2], fexact = 0u, doubt = 0u;
    float fgain[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float ys = k ? fs.y : fs.x, yh = k ? fh.y : fh.x;
      const float gf = (ys > 0.0f) ? yh * __builtin_amdgcn_rcpf(ys) : 1.0f;
      const float gc = __builtin_amdgcn_fmed3f(gf, c.min_boost, c.max_boost);
      const float v = (__builtin_amdgcn_logf(gc) - c.log2_min) * c.flt_scale;
      const float fl = __builtin_floorf(v), fr2 = v - fl;
      const bool lo = gf < c.flt_lo, hi = gf > c.flt_hi;
      const bool mid = (fr2 >= c.flt_delta) && (fr2 <= 1.0f - c.flt_delta);
      // luminances below 1e-10 leave the relative-error regime of the fast functions (denormal intermediates)
      const bool sane = !(ys > 0.0f && ys < 1e-10f) && !(yh != 0.0f && __builtin_fabsf(yh) < 1e-10f);
      if (!((lo || hi || mid) && sane)) doubt |= 1u << k;
      fbyte[k] = lo ? c.enc_byte_min : hi ? c.enc_byte_max : (uint32_t)fl;
      fgain[k] = gf;
      // the fast and the exact sRGB EOTF are zero for the same inputs only, so "SDR luminance is zero" (gain := 1,
      // gainmapmath.cpp:531) is decided identically on both paths
      if (!(ys > 0.0f)) fexact |= 1u << k;
    }
    // DEFER (large launches): the kernel never runs the exact path: a pixel in doubt keeps its estimate's byte for now and is
    // handed (bits 2, 3 of the result) to k_generate_resolve, which replaces the byte and accounts for the pixel's exact gain.
    // Otherwise (a launch too small to be worth a second kernel's latency) a wave holding such a pixel runs the exact path below.
    if (DEFER || __builtin_amdgcn_ballot_w64(doubt != 0u) == 0ull) {
      out[0] = (uint8_t)fbyte[0]; out[1] = (uint8_t)fbyte[1];
      gain[0] = fgain[0]; gain[1] = fgain[1];
      return fexact | (doubt << 2);
    }
  }
  // independent f64 evaluations advanced in lock step: 6 = 3 channels x 2 pixels.  Measured on MI355X
  // (scripts/ab): 6 -> 0.388 ms per 32-frame launch, 3 -> 0.432, 2 -> 0.490 although the narrower forms
  // need fewer VGPRs (98 / 84 / 78): exposed f64 FMA latency costs more than the lost occupancy.
  constexpr int kLockstep = 6;
  if (LUT) {
    r = (f2){s_srgb[lut_index_unit(r.x, kLutSrgbInvN)], s_srgb[lut_index_unit(r.y, kLutSrgbInvN)]};
    g = (f2){s_srgb[lut_index_unit(g.x, kLutSrgbInvN)], s_srgb[lut_index_unit(g.y, kLutSrgbInvN)]};
    b = (f2){s_srgb[lut_index_unit(b.x, kLutSrgbInvN)], s_srgb[lut_index_unit(b.y, kLutSrgbInvN)]};
  } else {
    float ch[6] = {r.x, r.y, g.x, g.y, b.x, b.y};
#pragma unroll
    for (int i = 0; i < 6; i += kLockstep) {
      float part[kLockstep];
#pragma unroll
      for (int j = 0; j < kLockstep; ++j) part[j] = ch[i + j];
      srgb_inv_oetf_guarded_n<kLockstep>(part);
#pragma unroll
      for (int j = 0; j < kLockstep; ++j) ch[i + j] = part[j];
    }
    r = (f2){ch[0], ch[1]}; g = (f2){ch[2], ch[3]}; b = (f2){ch[4], ch[5]};
  }
  const f2 sdr_nits = (splat(c.lum_r) * r + splat(c.lum_g) * g + splat(c.lum_b) * b) * splat(203.0f);

  // HDR: inverse OETF, gamut conversion, luminance * white (ultrahdr.cpp:328-330)
  if (TF != 0 && LUT) {  // both HDR tables have 4096 entries (gainmapmath.h:342-343,368-369)
    hr = (f2){s_hdr[lut_index_unit(hr.x, kLutHlgInvN)], s_hdr[lut_index_unit(hr.y, kLutHlgInvN)]};
    hg = (f2){s_hdr[lut_index_unit(hg.x, kLutHlgInvN)], s_hdr[lut_index_unit(hg.y, kLutHlgInvN)]};
    hb = (f2){s_hdr[lut_index_unit(hb.x, kLutHlgInvN)], s_hdr[lut_index_unit(hb.y, kLutHlgInvN)]};
  } else if (TF != 0) {  // ULTRAHDR_TF_LINEAR: identityConversion (ultrahdr.cpp:223-228)
    float ch[6] = {hr.x, hr.y, hg.x, hg.y, hb.x, hb.y};
#pragma unroll
    for (int i = 0; i < 6; i += kLockstep) {
      float part[kLockstep];
#pragma unroll
      for (int j = 0; j < kLockstep; ++j) part[j] = ch[i + j];
      if (TF == 1) hlg_inv_oetf_guarded_n<kLockstep>(part);
      else pq_inv_oetf_guarded_n<kLockstep>(part);
#pragma unroll
      for (int j = 0; j < kLockstep; ++j) ch[i + j] = part[j];
    }
    hr = (f2){ch[0], ch[1]}; hg = (f2){ch[2], ch[3]}; hb = (f2){ch[4], ch[5]};
  }
  if (!c.gm_identity) {
    const f2 t0 = splat(c.gm[0]) * hr + splat(c.gm[1]) * hg + splat(c.gm[2]) * hb;
    const f2 t1 = splat(c.gm[3]) * hr + splat(c.gm[4]) * hg + splat(c.gm[5]) * hb;
    const f2 t2 = splat(c.gm[6]) * hr + splat(c.gm[7]) * hg + splat(c.gm[8]) * hb;
    hr = t0; hg = t1; hb = t2;
  }
  if (PART == kGenLinear || PART == kGenBackLinear) { mid->r = r; mid->g = g; mid->b = b; mid->hr = hr; mid->hg = hg; mid->hb = hb; return 0u; }
  const f2 hdr_nits = (splat(c.lum_r) * hr + splat(c.lum_g) * hg + splat(c.lum_b) * hb) * splat(c.hdr_white_nits);

  gain[0] = raw_gain(sdr_nits.x, hdr_nits.x);
  gain[1] = raw_gain(sdr_nits.y, hdr_nits.y);
#pragma unroll
  for (int k = 0; k < 2; ++k)
    out[k] = encode_gain_guarded(gain[k], c.min_boost, c.max_boost, c.log2_min, c.log2_max, c.enc_scale, c.enc_byte_min,
                                 c.enc_byte_max);
  return 3u;
}

// Frames are read once and outputs written once: the aligned fast paths use non-temporal loads and stores
// so that 2 GB of apply output do not sit dirty in L2 / Infinity Cache when the next kernel starts reading.
// Same-box A/B (scripts/ab, 64 x 4K, ms per launch): generate 0.484 -> 0.444 with either, 0.394 with both;
// apply 0.98 -> 0.996.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 ld_stream(const uint4* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint2 ld_stream(const uint2* p) {
  const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint32_t ld_stream(const uint32_t* p) {
  return __builtin_nontemporal_load(p);
}
__device__ __forceinline__ void st_stream(uint4* p, uint4 v) {
  __builtin_nontemporal_store((u32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4*>(p));
}
__device__ __forceinline__ void st_stream(uint2* p, uint2 v) {
  __builtin_nontemporal_store((u32x2){v.x, v.y}, reinterpret_cast<u32x2*>(p));
}
__device__ __forceinline__ uint32_t ld8(const uint8_t* p) { return *p; }
__device__ __forceinline__ uint32_t ld16(const uint16_t* p) { return *p; }

// launch geometry of k_generate, chosen by same-box A/B (scripts/ab, ms per 32-frame 4K launch):
//   block 64/128/256/512/1024, 1 span: 0.64 / 0.50 / 0.39 / 0.355 / 0.43;   block 256, 4 spans: 0.350
// (kGenBlock = 256, kGenTiles = 4: uhdr_kernels.h, the host layer reports them)

// inputs of pair `idx` (two horizontally adjacent map pixels = an 8x4 pixel block of both images) -> registers
template <bool ALIGNED>
__device__ __forceinline__ void load_pair(const GenConsts& c, const GenImage& im, const uint8_t* im_v, uint32_t my, uint32_t pr,
                                          bool two, uint32_t (&hy)[2][4][2], uint32_t (&huv)[2][2][2], uint32_t (&y8)[2][4],
                                          uint32_t (&u8)[2][2], uint32_t (&v8)[2][2]) {
  const uint32_t mx = pr * 2u;
  if (ALIGNED) {
    // 32-bit element offsets (every plane is < 4 GiB on this path): one 64-bit add per address
    const uint32_t hoff = 4u * my * im.hy_stride + 8u * pr, yoff = 4u * my * im.y_stride + 8u * pr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint4 q = ld_stream(reinterpret_cast<const uint4*>(im.hy + (hoff + r * im.hy_stride)));
      hy[0][r][0] = q.x; hy[0][r][1] = q.y; hy[1][r][0] = q.z; hy[1][r][1] = q.w;
      const uint2 p = ld_stream(reinterpret_cast<const uint2*>(im.y + (yoff + r * im.y_stride)));
      y8[0][r] = p.x; y8[1][r] = p.y;
    }
    const uint32_t huvoff = 2u * my * im.huv_stride + 8u * pr, coff = 2u * my * im.c_stride + 4u * pr;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const uint4 q = ld_stream(reinterpret_cast<const uint4*>(im.huv + (huvoff + r * im.huv_stride)));
      huv[0][r][0] = q.x; huv[0][r][1] = q.y; huv[1][r][0] = q.z; huv[1][r][1] = q.w;
      const uint32_t uu = ld_stream(reinterpret_cast<const uint32_t*>(im.u + (coff + r * im.c_stride)));
      const uint32_t vv = ld_stream(reinterpret_cast<const uint32_t*>(im_v + (coff + r * im.c_stride)));
      u8[0][r] = uu & 0xffffu; u8[1][r] = uu >> 16;
      v8[0][r] = vv & 0xffffu; v8[1][r] = vv >> 16;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool on = (k == 0) || two;
      const uint32_t x0 = 4u * (mx + k);  // first image column of this map pixel
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint16_t* hrow = im.hy + (size_t)(4u * my + r) * im.hy_stride + x0;
        const uint8_t* yrow = im.y + (size_t)(4u * my + r) * im.y_stride + x0;
        hy[k][r][0] = on ? (ld16(hrow) | (ld16(hrow + 1) << 16)) : 0u;
        hy[k][r][1] = on ? (ld16(hrow + 2) | (ld16(hrow + 3) << 16)) : 0u;
        y8[k][r] = on ? (ld8(yrow) | (ld8(yrow + 1) << 8) | (ld8(yrow + 2) << 16) | (ld8(yrow + 3) << 24)) : 0u;
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const uint16_t* crow = im.huv + (size_t)(2u * my + r) * im.huv_stride + x0;  // (x & ~1)
        const uint8_t* urow = im.u + (size_t)(2u * my + r) * im.c_stride + (x0 >> 1);
        const uint8_t* vrow = im_v + (size_t)(2u * my + r) * im.c_stride + (x0 >> 1);
        huv[k][r][0] = on ? (ld16(crow) | (ld16(crow + 1) << 16)) : 0u;
        huv[k][r][1] = on ? (ld16(crow + 2) | (ld16(crow + 3) << 16)) : 0u;
        u8[k][r] = on ? (ld8(urow) | (ld8(urow + 1) << 8)) : 0u;
        v8[k][r] = on ? (ld8(vrow) | (ld8(vrow + 1) << 8)) : 0u;
      }
    }
  }
}

// wave64 reduction: every lane ends up with the wave's min / max.  Six DPP steps -- the lane exchanges ride on the VALU operand
// path: quad_perm (xor 1, xor 2), row_half_mirror, row_mirror put a row's extreme into its 16 lanes, row_bcast:15 / row_bcast:31
// carry it across the four rows into lane 63 -- and one v_readlane.  (Round 4.  __shfl_xor compiles to ds_bpermute_b32: six
// dependent trips through the LDS crossbar per value, 36 of them in k_generate's tail, ~0.6 us during which a wave that has
// finished its pixels still holds its slot.)  All 64 lanes are active wherever this is called.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_move(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROWS, 0xF, false));
}
// one value's ladder: MAX ? the wave's maximum : its minimum
template <bool MAX>
__device__ __forceinline__ float wave_extreme(float v) {
#define UHDR_EXT(CTRL, ROWS) v = MAX ? fmaxf(v, dpp_move<CTRL, ROWS>(v)) : fminf(v, dpp_move<CTRL, ROWS>(v))
  UHDR_EXT(0xB1, 0xF);    // quad_perm:[1,0,3,2]
  UHDR_EXT(0x4E, 0xF);    // quad_perm:[2,3,0,1]
  UHDR_EXT(0x141, 0xF);   // row_half_mirror
  UHDR_EXT(0x140, 0xF);   // row_mirror
  UHDR_EXT(0x142, 0xA);   // row_bcast:15 -> rows 1, 3
  UHDR_EXT(0x143, 0xC);   // row_bcast:31 -> rows 2, 3
#undef UHDR_EXT
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ void wave_minmax(float& vmin, float& vmax) {
  vmin = wave_extreme<false>(vmin);
  vmax = wave_extreme<true>(vmax);
}
// one lane per wave publishes; keys[0] holds ~key(min), keys[1] holds key(max); both only grow, both start at 0
__device__ __forceinline__ void publish_minmax(float gmin, float gmax, uint32_t* keys) {
  if ((threadIdx.x & 63u) == 0u && gmin <= gmax) {  // wave saw at least one pixel
    const uint32_t kmin = ~float_to_key(gmin), kmax = float_to_key(gmax);
    // a stale (smaller) value read here only costs an unnecessary atomic, never a lost update
    if (__hip_atomic_load(&keys[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kmin) atomicMax(&keys[0], kmin);
    if (__hip_atomic_load(&keys[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kmax) atomicMax(&keys[1], kmax);
  }
}

// exact bytes and unclamped gains of pair (my, pr): what k_generate_resolve runs on the pixels the filtered kernel left to it
template <int TF, bool ALIGNED, bool LUT>
__device__ __forceinline__ void exact_pair(const GenConsts& c, const GenImage& im, const uint8_t* im_v, uint32_t my,
                                           uint32_t pr, bool two, const float* s_srgb, const float* s_hdr, uint8_t (&o)[2], float (&gn)[2]) {
  uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
  load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);
  gen_pair<TF, LUT, false>(c, hy, huv, y8, u8, v8, o, gn, s_srgb, s_hdr);
}

// (the relative distance within which a filter estimate may sit from the exact gain is GenConsts::flt_gain_rel: generate_consts' kRel, doubled)

// Thread = 2 horizontally adjacent map pixels = an 8x4 pixel block of both images.
// A wave64 therefore consumes 1 KiB contiguous per P010 row (dwordx4/lane), 512 B per 8-bit luma
// row (dwordx2/lane) and 256 B per chroma row (dword/lane).
//
// Statistics (content min / max of the unclamped gain) stay EXACT under the filter: every thread keeps the gains of its
// pixels with an "exact" bit; when a wave has finished its tiles, only pixels whose estimate could be the wave's exact
// extreme -- and could still beat the extreme already published for the image -- are re-evaluated on the exact path
// (typically none).  Waves never wait for each other: a block-wide reduction here measured +25 % on the whole kernel,
// because one wave in seven takes the exact path in some tile and its three siblings would idle at the barrier.
template <int TF, bool ALIGNED, bool LUT, bool FILTER, int TILES, bool DEFER, int BLOCK = kGenBlock>
__global__ void __launch_bounds__(BLOCK, 1) k_generate(const GenConsts c, const GenBatch b) {
  // LUT mode: block-private copies of the two tables (4 KiB + 16 KiB), so every lookup is an LDS gather
  __shared__ float s_srgb[LUT ? kLutSrgbInvN : 1];
  __shared__ float s_hdr[(LUT && TF != 0) ? kLutHlgInvN : 1];
  __shared__ float s_kept[(FILTER && DEFER) ? TILES * 2 * BLOCK : 1];  // FILTER: every thread's gains, for the candidate pass
  if (LUT) {
    for (uint32_t i = threadIdx.x; i < kLutSrgbInvN / 4u; i += BLOCK)
      reinterpret_cast<float4*>(s_srgb)[i] = reinterpret_cast<const float4*>(c.lut + kLutSrgbInv)[i];
    if (TF != 0) {
      const float4* src = reinterpret_cast<const float4*>(c.lut + (TF == 1 ? kLutHlgInv : kLutPqInv));
      for (uint32_t i = threadIdx.x; i < kLutHlgInvN / 4u; i += BLOCK) reinterpret_cast<float4*>(s_hdr)[i] = src[i];
    }
    __syncthreads();
  }
  // consecutive workgroups belong to different images (grid.x = image): the images of a launch progress together, so
  // the extremes a finished wave publishes prune the statistics candidates of the image's later waves
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const GenImage& im = b.img[img_i];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
  const bool stats = c.stat_keys != nullptr;
  float emin = __builtin_inff(), emax = -__builtin_inff();   // over gains known exactly
  float amin = __builtin_inff(), amax = -__builtin_inff();   // over all gains (estimates included)
  uint32_t kept_exact = 0u, kept_valid = 0u, kept_doubt = 0u;   // 2 bits per tile
  uint32_t n_saved = 0u;   // slot mode: pairs of this wave that have left with their sampled values (wave-uniform count)
  uint32_t* wslot = (FILTER && DEFER && c.stat_slots != 0u)
                        ? c.stat_ws + (size_t)kStatWords * blockIdx.x + kStatHdr + (blockIdx.y * (uint32_t)(BLOCK / 64) + (threadIdx.x >> 6)) * kStatSlotWords
                        : nullptr;

  // each block walks TILES consecutive spans of BLOCK pairs: fewer, longer-lived waves
  // (wave launch + descriptor fetch is a measurable share of a ~10 us wave)
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)BLOCK + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);

    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
    load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);

    uint8_t o[2];
    float gn[2];
    // a missing second pixel is computed on zeros and dropped
    GenMid mid;
    const uint32_t ex = gen_pair<TF, LUT, FILTER, DEFER>(c, hy, huv, y8, u8, v8, o, gn, s_srgb, s_hdr, (FILTER && DEFER) ? &mid : nullptr);
    const uint8_t o0 = o[0], o1 = o[1];
    if (FILTER && DEFER) {
      // pixels in doubt: their bytes are provisional -- the pair goes onto the image's list once the wave has finished its tiles,
      // flags = which of its two pixels k_generate_resolve has to redo -- and their gains take no part in the statistics here
      uint32_t dm = (ex >> 2) & (two ? 3u : 1u);
      if (c.stat_slots != 0u) {
        // slot mode: the pair leaves WITH its sampled values, now, while they are still in registers (one tile in five holds such a
        // pair; the wave's first kStatSlotSaved go this way, any beyond that onto the plain list below)
        const unsigned long long dmask = __builtin_amdgcn_ballot_w64(dm != 0u);
        if (dmask != 0ull) {
          const uint32_t pos = n_saved + (uint32_t)__builtin_popcountll(dmask & ((1ull << (threadIdx.x & 63u)) - 1ull));
          n_saved += (uint32_t)__builtin_popcountll(dmask);
          if (dm != 0u && pos < kStatSlotSaved) {
            float4* e = reinterpret_cast<float4*>(wslot + 16u + pos * 16u);
            e[0] = make_float4(__uint_as_float((idx << 3) | dm), mid.r.x, mid.r.y, mid.g.x);
            e[1] = make_float4(mid.g.y, mid.b.x, mid.b.y, mid.hr.x);
            e[2] = make_float4(mid.hr.y, mid.hg.x, mid.hg.y, mid.hb.x);
            e[3] = make_float4(mid.hb.y, 0.0f, 0.0f, 0.0f);
            dm = 0u;   // (not onto the plain list; its gains stay out of the statistics here all the same: `valid` below)
          }
        }
      }
      kept_doubt |= dm << (2u * t);
      if (stats) {
        s_kept[(2u * t) * BLOCK + threadIdx.x] = gn[0];
        s_kept[(2u * t + 1u) * BLOCK + threadIdx.x] = gn[1];
        const uint32_t valid = (two ? 3u : 1u) & ~((ex >> 2) & 3u);
        kept_exact |= (ex & 3u) << (2u * t);
        kept_valid |= valid << (2u * t);
        if (valid & 1u) { amin = fminf(amin, gn[0]); amax = fmaxf(amax, gn[0]); }
        if (valid & 2u) { amin = fminf(amin, gn[1]); amax = fmaxf(amax, gn[1]); }
        if (ex & valid & 1u) { emin = fminf(emin, gn[0]); emax = fmaxf(emax, gn[0]); }
        if (ex & valid & 2u) { emin = fminf(emin, gn[1]); emax = fmaxf(emax, gn[1]); }
      }
    } else {
      emin = fminf(emin, gn[0]); emax = fmaxf(emax, gn[0]);
      if (two) { emin = fminf(emin, gn[1]); emax = fmaxf(emax, gn[1]); }
    }
    uint8_t* mp = im.map + (size_t)my * c.map_w + mx;
    if (ALIGNED) {
      *reinterpret_cast<uint16_t*>(mp) = (uint16_t)(o0 | ((uint32_t)o1 << 8));
    } else {
      mp[0] = o0;
      if (two) mp[1] = o1;
    }
  }
  if (FILTER && !DEFER) return;   // (small launches without statistics: launch_generate_t)
  if (!FILTER && !stats) return;
  uint32_t* keys = stats ? c.stat_keys + (size_t)c.stat_stride * img_i : nullptr;

  if (FILTER) {
    uint32_t* ws = c.stat_ws + (size_t)kStatWords * img_i;
    uint32_t cand = 0u;   // one bit per tile: a statistics candidate
    if (stats) {
      // Which estimates could be the image's exact minimum / maximum?  An estimate a stands for an exact gain within e|a| of it, so
      // the exact minimum of the image lies at or below (1 + e) x any estimate and at or below any exact gain seen -- by this wave
      // or, through the image's words in device memory, by any wave before it.  A pixel whose a (1 - e) lies above that bound
      // cannot be the minimum; the others (the pixel that IS the minimum always among them) go onto the image's list, which
      // k_generate_resolve evaluates on the exact path after this kernel.
      wave_minmax(amin, amax);
      float wmin = emin, wmax = emax;          // what this wave already knows exactly (gain := 1 of pixels without SDR luminance)
      wave_minmax(wmin, wmax);
      const float e = c.flt_gain_rel;
      // (the words the estimates' extremes are published in: one pair per image, or -- launches of few images, kStatEst -- per list)
      uint32_t* est = c.stat_spread != 0u ? ws + kStatEst + 2u * (blk % kStatLists) : ws;
      uint32_t e0 = __hip_atomic_load(&est[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t e1 = __hip_atomic_load(&est[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t k0 = __hip_atomic_load(&keys[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t k1 = __hip_atomic_load(&keys[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (amin <= amax) {   // publish this wave's estimates (one lane; the words only grow)
        const uint32_t m0 = ~float_to_key(amin), m1 = float_to_key(amax);
        if ((threadIdx.x & 63u) == 0u) {
          if (e0 < m0) atomicMax(&est[0], m0);
          if (e1 < m1) atomicMax(&est[1], m1);
        }
        e0 = e0 < m0 ? m0 : e0; e1 = e1 < m1 ? m1 : e1;
      }
      float min_hi = fminf(k1 != 0u ? key_to_float(~k0) : __builtin_inff(), wmin);   // exact gains: the bound as it stands
      float max_lo = fmaxf(k1 != 0u ? key_to_float(k1) : -__builtin_inff(), wmax);
      if (e1 != 0u) {
        const float pmin = key_to_float(~e0), pmax = key_to_float(e1);
        min_hi = fminf(min_hi, pmin + e * __builtin_fabsf(pmin));
        max_lo = fmaxf(max_lo, pmax - e * __builtin_fabsf(pmax));
      }
#pragma unroll
      for (uint32_t t = 0; t < (uint32_t)TILES; ++t)
#pragma unroll
        for (uint32_t k = 0; k < 2u; ++k) {
          const uint32_t bit = 1u << (2u * t + k);
          if ((kept_valid & bit) && !(kept_exact & bit)) {
            const float a = s_kept[(2u * t + k) * BLOCK + threadIdx.x], slack = e * __builtin_fabsf(a);
            if ((a - slack <= min_hi) || (a + slack >= max_lo)) cand |= 1u << t;
          }
        }
    }
    // One append per wave for everything it leaves to k_generate_resolve: a returning atomic per tile would park the wave for a
    // trip to the memory side in one tile out of five.
    unsigned long long mask[TILES];
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
      mask[t] = __builtin_amdgcn_ballot_w64((((kept_doubt >> (2u * t)) & 3u) | ((cand >> t) & 1u)) != 0u);
      total += (uint32_t)__builtin_popcountll(mask[t]);
    }
    if (total != 0u || c.stat_slots != 0u) {
      const uint32_t lane = threadIdx.x & 63u, list = blk % kStatLists;
      uint32_t base = 0u, cap = kStatCap;
      uint32_t* lw = ws + kStatHdr + list * kStatCap;
      if (c.stat_slots != 0u) {
        // the wave's own slots: plain stores, nothing to wait for (every wave of the launch writes its count, also a zero)
        lw = wslot;
        const bool over = total > kStatSlotPlain;
        const uint32_t ns = n_saved < kStatSlotSaved ? n_saved : kStatSlotSaved;
        if (lane == 0u) {
          ws[kStatSlotCnt + blk * (uint32_t)(BLOCK / 64) + (threadIdx.x >> 6)] = over ? 0u : (total | (ns << 8));
          if (over) __hip_atomic_store(&ws[6], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sweep this image
        }
        ++lw;
        cap = over ? 0u : kStatSlotPlain;
      } else {
        if (lane == 0u) base = atomicAdd(&ws[8u + list], total);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
      }
#pragma unroll
      for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
        const uint32_t flags = ((kept_doubt >> (2u * t)) & 3u) | (((cand >> t) & 1u) << 2);
        const uint32_t pos = base + (uint32_t)__builtin_popcountll(mask[t] & ((1ull << lane) - 1ull));
        if (flags != 0u && pos < cap) lw[pos] = (((blk * (uint32_t)TILES + t) * (uint32_t)BLOCK + threadIdx.x) << 3) | flags;
        base += (uint32_t)__builtin_popcountll(mask[t]);
      }
    }
    if (!stats) return;
  }
  wave_minmax(emin, emax);
  publish_minmax(emin, emax, keys);
}

__global__ void k_stats_finalize(uint32_t* keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k0 = keys[2 * i], k1 = keys[2 * i + 1];
  float mn = __builtin_inff(), mx = -__builtin_inff();  // image without map pixels
  if (k1 != 0u) { mn = key_to_float(~k0); mx = key_to_float(k1); }
  keys[2 * i] = __float_as_uint(mn);
  keys[2 * i + 1] = __float_as_uint(mx);
}

// What the filtered kernel left for an image, on the exact path: list entries are (pair index << 3 | flags) -- flags 1 / 2: that
// pixel of the pair was in doubt, its byte is replaced and its exact gain joins the statistics; flag 4: a statistics candidate,
// both gains join.  An image whose list overflowed (flat content at a code boundary: every pixel in doubt) is swept whole.
// grid = (image, kResolveSlices), each block a slice of the work; the slice that finishes last writes the image's (min, max) and
// clears the header words for the next launch.
static_assert(kStatLists == 64u, "k_generate_resolve reads the list counts with one wave");
template <int TF, bool ALIGNED>
__global__ void __launch_bounds__(256) k_generate_resolve(const GenConsts c, const GenBatch b) {
  const uint32_t img_i = blockIdx.x;
  const GenImage& im = b.img[img_i];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  uint32_t* ws = c.stat_ws + (size_t)kStatWords * img_i;
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1, total = pairs_per_row * c.map_h;
  const bool stats = c.stat_out != nullptr;
  float emin = __builtin_inff(), emax = -__builtin_inff();
  // one loop for both forms (the exact path is large): thread g of the image takes pair g (sweep) or entry g of the image's lists
  // laid end to end (their exclusive prefix sums in LDS), so that the few entries fill whole waves
  __shared__ uint32_t s_first[kStatSlotWaves + 1u];
  __shared__ uint8_t s_ns[kStatSlotWaves];   // slot mode: the saved entries among a wave's entries (they come first)
  __shared__ uint32_t s_sweep;
  const bool slots = c.stat_slots != 0u;
  if (slots) {
    // slot mode: the counts of the image's waves (word 0 of every wave's slots), four per thread, prefix sums over the block
    static_assert(kStatSlotWaves == 4u * 256u, "four waves' counts per thread");
    __shared__ uint32_t s_part[4];
    uint32_t n4[4];
    const uint4 cw4 = *reinterpret_cast<const uint4*>(ws + kStatSlotCnt + 4u * threadIdx.x);   // plain entries | saved entries << 8, four waves'
    const uint32_t cws[4] = {cw4.x, cw4.y, cw4.z, cw4.w};
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t w = 4u * threadIdx.x + j;
      const uint32_t cw = w < c.stat_slots ? cws[j] : 0u;
      s_ns[w] = (uint8_t)(cw >> 8);
      n4[j] = (cw & 0xFFu) + (cw >> 8);
    }
    const uint32_t over = __hip_atomic_load(&ws[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t mine = n4[0] + n4[1] + n4[2] + n4[3];
    const uint32_t before = block_exclusive_sum<256>(mine, s_part);
    s_first[4u * threadIdx.x] = before;
    s_first[4u * threadIdx.x + 1u] = before + n4[0];
    s_first[4u * threadIdx.x + 2u] = before + n4[0] + n4[1];
    s_first[4u * threadIdx.x + 3u] = before + n4[0] + n4[1] + n4[2];
    if (threadIdx.x == 255u) { s_first[kStatSlotWaves] = before + mine; s_sweep = over; }
  } else if (threadIdx.x < 64u) {   // the counts in one trip to memory (kStatLists == 64), prefix sums by wave shuffles
    const uint32_t cnt = ws[8u + threadIdx.x];
    const bool over = __builtin_amdgcn_ballot_w64(cnt > kStatCap) != 0ull;
    uint32_t inc = min(cnt, kStatCap);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
      if ((int)threadIdx.x >= off) inc += v;
    }
    s_first[threadIdx.x + 1u] = inc;
    if (threadIdx.x == 0) { s_first[0] = 0u; s_sweep = over ? 1u : 0u; }
  }
  __syncthreads();
  const bool sweep = s_sweep != 0u;
  const uint32_t nl = slots ? kStatSlotWaves : kStatLists;
  const uint32_t n = sweep ? total : s_first[nl];
#pragma unroll 1
  for (uint32_t g = blockIdx.y * 256u + threadIdx.x; g < n; g += kResolveSlices * 256u) {
    uint32_t entry = (g << 3) | 7u;
    GenMid mid;
    bool have = false;   // the pair came with its sampled values
    if (!sweep) {
      uint32_t l = 0u;
      for (uint32_t s2 = nl / 2u; s2 != 0u; s2 >>= 1) if (s_first[l + s2] <= g) l += s2;   // the list (the wave's slots) that holds entry g
      const uint32_t k = g - s_first[l];
      if (!slots) {
        entry = ws[kStatHdr + l * kStatCap + k];
      } else if (k >= (uint32_t)s_ns[l]) {
        entry = ws[kStatHdr + l * kStatSlotWords + 1u + (k - (uint32_t)s_ns[l])];
      } else {
        const uint4* e = reinterpret_cast<const uint4*>(ws + kStatHdr + l * kStatSlotWords + 16u + k * 16u);
        const uint4 e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
        entry = e0.x;
        mid.r = (f2){__uint_as_float(e0.y), __uint_as_float(e0.z)};
        mid.g = (f2){__uint_as_float(e0.w), __uint_as_float(e1.x)};
        mid.b = (f2){__uint_as_float(e1.y), __uint_as_float(e1.z)};
        mid.hr = (f2){__uint_as_float(e1.w), __uint_as_float(e2.x)};
        mid.hg = (f2){__uint_as_float(e2.y), __uint_as_float(e2.z)};
        mid.hb = (f2){__uint_as_float(e2.w), __uint_as_float(e3.x)};
        have = true;
      }
    }
    const uint32_t idx = entry >> 3;
    const uint32_t my = idx / pairs_per_row, pr = idx - my * pairs_per_row;
    const bool two = ALIGNED || (pr * 2u + 1u < c.map_w);
    uint8_t o[2];
    float gn[2];
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
    if (!have) {   // sample the pair (again): fourteen scattered lines
      load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);
      gen_pair<TF, false, false, false, kGenFront>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &mid);
    }
    gen_pair<TF, false, false, false, kGenBack>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &mid);
    uint8_t* mp = im.map + (size_t)my * c.map_w + 2u * pr;
    if (entry & 1u) mp[0] = o[0];
    if ((entry & 2u) && two) mp[1] = o[1];
    if ((entry & 5u) != 0u) { emin = fminf(emin, gn[0]); emax = fmaxf(emax, gn[0]); }
    if ((entry & 6u) != 0u && two) { emin = fminf(emin, gn[1]); emax = fmaxf(emax, gn[1]); }
  }
  if (stats) {
    wave_minmax(emin, emax);
    publish_minmax(emin, emax, ws + 4);
  }
  // (no fence: a release at agent scope would write this XCD's whole L2 back -- the maps k_generate has just stored.  The keys
  // are only ever touched by agent-scope atomics, which are performed at the memory side; waiting for this wave's to be
  // acknowledged before the slice counts itself finished is the order that is needed.)
  __shared__ uint32_t s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(&ws[3], 1u);
  __syncthreads();
  if (s_last == kResolveSlices - 1u && threadIdx.x == 0) {
    if (stats) {
      const uint32_t k0 = __hip_atomic_load(&ws[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t k1 = __hip_atomic_load(&ws[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      float mn = __builtin_inff(), mx = -__builtin_inff();  // image without map pixels
      if (k1 != 0u) { mn = key_to_float(~k0); mx = key_to_float(k1); }
      c.stat_out[2u * img_i] = mn;
      c.stat_out[2u * img_i + 1u] = mx;
    }
  }
  __syncthreads();   // (words 4 and 5 have been read)
  static_assert(kStatSlotCnt <= 256u, "one header word per thread");
  if (s_last == kResolveSlices - 1u && threadIdx.x < kStatSlotCnt)   // the header, cleared for the next launch (the waves' count words behind it are rewritten by every launch)
    __hip_atomic_store(&ws[threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int TF>
static hipError_t launch_stats_resolve_tf(const GenConsts& c, const GenBatch& b, int n, bool aligned, hipStream_t s) {
  if (aligned) hipLaunchKernelGGL((k_generate_resolve<TF, true>), dim3((unsigned)n, kResolveSlices), dim3(256), 0, s, c, b);
  else hipLaunchKernelGGL((k_generate_resolve<TF, false>), dim3((unsigned)n, kResolveSlices), dim3(256), 0, s, c, b);
  return hipGetLastError();
}
hipError_t launch_stats_resolve(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s) {
  if (n <= 0 || c.stat_ws == nullptr) return hipSuccess;
  switch (hdr_tf) {
    case 0: return launch_stats_resolve_tf<0>(c, b, n, aligned, s);
    case 1: return launch_stats_resolve_tf<1>(c, b, n, aligned, s);
    case 2: return launch_stats_resolve_tf<2>(c, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

bool generate_is_small(const GenConsts& c, int n) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  const uint32_t span = (uint32_t)kGenBlock * (uint32_t)kGenTiles;
  return (uint64_t)((total + span - 1u) / span) * (uint64_t)n < 1024u;
}

// waves per image of the filtered + deferred launch launch_generate_t makes of n such images (one span per block when the launch is
// small, kGenTiles otherwise); 0 when they do not fit the per-wave slots of the statistics workspace
uint32_t generate_slot_waves(const GenConsts& c, int n) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  const uint32_t per = (uint32_t)kGenBlock * (generate_is_small(c, n) ? 1u : (uint32_t)kGenTiles);
  const uint64_t waves = (uint64_t)((total + per - 1u) / per) * (uint64_t)(kGenBlock / 64);
  return waves <= kStatSlotWaves ? (uint32_t)waves : 0u;
}

// a launch WITH statistics: is the filtered kernel + k_generate_resolve faster than the exact kernel?  (from 128 spans of 1024 pairs)
bool generate_resolve_pays(const GenConsts& c, int n) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  const uint32_t span = (uint32_t)kGenBlock * (uint32_t)kGenTiles;
  return (uint64_t)((total + span - 1u) / span) * (uint64_t)n >= 128u;
}

template <int TF, bool ALIGNED, bool LUT, bool FILTER>
static hipError_t launch_generate_t(const GenConsts& c, const GenBatch& b, int n, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  // Spans per block: kGenTiles (fewer, longer-lived waves) where the launch still fills the chip, one otherwise -- a single
  // 4K image is 1013 spans: 254 blocks of 4 would put one wave on each SIMD and leave the memory system nothing to overlap.
  // Filtered kernel: a large launch leaves its pixels in doubt to k_generate_resolve (c.stat_ws set by the caller); a small one
  // (c.stat_ws null) runs the exact path in place, for the waves that hold such a pixel.
  const bool small = generate_is_small(c, n);
  const unsigned b4 = (total + (uint32_t)kGenBlock * (uint32_t)kGenTiles - 1u) / ((uint32_t)kGenBlock * (uint32_t)kGenTiles);
  const unsigned b1 = (total + kGenBlock - 1u) / kGenBlock;
  const dim3 g4 = dim3((unsigned)n, b4, 1);
  const dim3 g1 = dim3((unsigned)n, b1, 1);
  if (FILTER) {
    if (c.stat_ws != nullptr) {
      if (small) hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, 1, true>), g1, dim3(kGenBlock, 1, 1), 0, s, c, b);
      else hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, kGenTiles, true>), g4, dim3(kGenBlock, 1, 1), 0, s, c, b);
    } else {
      if (c.stat_keys != nullptr) return hipErrorInvalidValue;   // statistics of a filtered launch need the workspace
      // a launch whose waves are all resident at once, from one 4K image up (1013 blocks of 256 threads): 128-thread blocks give
      // the dispatcher twice the workgroups to spread -- same-box A/B: one 4K frame 11.9 -> 11.0 us; one 1080p frame (254 blocks)
      // is better off as it is (6.9 against 7.9 us)
      const unsigned h1 = (total + 127u) / 128u;
      if ((uint64_t)h1 * (uint64_t)n >= 2000u) {
        const dim3 gh = dim3((unsigned)n, h1, 1);
        hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, 1, false, 128>), gh, dim3(128, 1, 1), 0, s, c, b);
      } else {
        hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, 1, false>), g1, dim3(kGenBlock, 1, 1), 0, s, c, b);
      }
    }
  } else if (small) {
    hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, 1, false>), g1, dim3(kGenBlock, 1, 1), 0, s, c, b);
  } else {
    hipLaunchKernelGGL((k_generate<TF, ALIGNED, LUT, FILTER, kGenTiles, false>), g4, dim3(kGenBlock, 1, 1), 0, s, c, b);
  }
  return hipGetLastError();
}

template <int TF>
static hipError_t launch_generate_tf(const GenConsts& c, const GenBatch& b, int n, bool aligned, bool lut, bool filter,
                                     hipStream_t s) {
  if (lut) return aligned ? launch_generate_t<TF, true, true, false>(c, b, n, s) : launch_generate_t<TF, false, true, false>(c, b, n, s);
  if (filter && aligned) return launch_generate_t<TF, true, false, true>(c, b, n, s);
  return aligned ? launch_generate_t<TF, true, false, false>(c, b, n, s) : launch_generate_t<TF, false, false, false>(c, b, n, s);
}
hipError_t launch_generate(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, bool lut,
                           bool filter, hipStream_t s) {
  if (lut && c.lut == nullptr) return hipErrorInvalidValue;
  switch (hdr_tf) {
    case 0: return launch_generate_tf<0>(c, b, n, aligned, lut, filter, s);
    case 1: return launch_generate_tf<1>(c, b, n, aligned, lut, filter, s);
    case 2: return launch_generate_tf<2>(c, b, n, aligned, lut, filter, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_stats_init(uint32_t* keys, int n, hipStream_t s) {
  return hipMemsetAsync(keys, 0, sizeof(uint32_t) * 2 * (size_t)n, s);
}
hipError_t launch_stats_finalize(uint32_t* keys, int n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_stats_finalize, dim3((n + 63) / 64), dim3(64), 0, s, keys, n);
  return hipGetLastError();
}

// =================================================================================================
// content-adaptive generate (uhdr_hip_generate_gainmap_adaptive_batch)
// =================================================================================================
__global__ void __launch_bounds__(256) k_adaptive_init(uint32_t* keys, uint32_t words) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < words) keys[i] = 0u;
}
hipError_t launch_adaptive_init(uint32_t* keys, uint32_t words, hipStream_t s) {
  if (words == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_adaptive_init, dim3((words + 255u) / 256u), dim3(256), 0, s, keys, words);
  return hipGetLastError();
}

// Pass 1: k_generate's front end on the exact path -- the same sampling, the same luminances -- but what a thread stores is the
// unclamped f32 gain of its two map pixels (raw_gain: 1 where the SDR luminance is 0), 4 bytes per map pixel into the image's part
// of the workspace (GenImage::map), and no byte: the range they are encoded against is not known before the whole image has been
// seen.  The image's extremes are the extremes of exactly these floats (publish_minmax on the image's two key words).
template <int TF, bool ALIGNED, int TILES>
__global__ void __launch_bounds__(kGenBlock, 1) k_generate_gains(const GenConsts c, const GenBatch b) {
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const GenImage& im = b.img[img_i];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  float* gains = reinterpret_cast<float*>(im.map);
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
  float emin = __builtin_inff(), emax = -__builtin_inff();
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)kGenBlock + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
    load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);
    uint8_t o[2];
    float gn[2];
    gen_pair<TF, false, false>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr);   // (a missing second pixel is computed on zeros and dropped)
    emin = fminf(emin, gn[0]); emax = fmaxf(emax, gn[0]);
    if (two) { emin = fminf(emin, gn[1]); emax = fmaxf(emax, gn[1]); }
    float* gp = gains + (size_t)my * c.map_w + mx;
    if (ALIGNED) {   // map_w is even and the image's gains are 16-byte aligned: the pair is one 8-byte store
      *reinterpret_cast<float2*>(gp) = make_float2(gn[0], gn[1]);
    } else {
      gp[0] = gn[0];
      if (two) gp[1] = gn[1];
    }
  }
  wave_minmax(emin, emax);   // (every lane arrives here)
  publish_minmax(emin, emax, c.stat_keys + (size_t)c.stat_stride * img_i);
}
template <int TF>
static hipError_t launch_generate_gains_tf(const GenConsts& c, const GenBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  const bool small = generate_is_small(c, n);   // spans per block as launch_generate_t chooses them
  const unsigned per = (unsigned)kGenBlock * (small ? 1u : (unsigned)kGenTiles);
  const dim3 g((unsigned)n, (total + per - 1u) / per, 1), blk(kGenBlock, 1, 1);
  if (small) {
    if (aligned) hipLaunchKernelGGL((k_generate_gains<TF, true, 1>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_gains<TF, false, 1>), g, blk, 0, s, c, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_generate_gains<TF, true, kGenTiles>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_gains<TF, false, kGenTiles>), g, blk, 0, s, c, b);
  }
  return hipGetLastError();
}
hipError_t launch_generate_gains(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s) {
  if (c.stat_keys == nullptr) return hipErrorInvalidValue;
  switch (hdr_tf) {
    case 0: return launch_generate_gains_tf<0>(c, b, n, aligned, s);
    case 1: return launch_generate_gains_tf<1>(c, b, n, aligned, s);
    case 2: return launch_generate_gains_tf<2>(c, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

// Per-channel (RGB) gain map: k_generate_gains' grid and front end on the exact path up to the two linear
// colours (gen_pair<kGenLinear>), then encodeGain(sdr.c * 203, hdr.c * white) per channel instead of once on the luminances.  A map
// pixel is the dword R | G << 8 | B << 16 | 0xFF << 24 (GenImage::map: 4-byte aligned, rows of map_w pixels); the aligned form
// stores a thread's pair as 8 bytes.
template <int TF, bool ALIGNED, int TILES>
__global__ void __launch_bounds__(kGenBlock, 1) k_generate_rgb(const GenConsts c, const GenBatch b) {
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const GenImage& im = b.img[img_i];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  uint32_t* map = reinterpret_cast<uint32_t*>(im.map);
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)kGenBlock + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
    load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);
    uint8_t o[2];
    float gn[2];
    GenMid lin;
    gen_pair<TF, false, false, false, kGenLinear>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &lin);   // (a missing second pixel: zeros, dropped)
    const f2 sdr[3] = {lin.r * splat(203.0f), lin.g * splat(203.0f), lin.b * splat(203.0f)};
    const f2 hdr[3] = {lin.hr * splat(c.hdr_white_nits), lin.hg * splat(c.hdr_white_nits), lin.hb * splat(c.hdr_white_nits)};
    uint32_t px[2] = {0xFF000000u, 0xFF000000u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float gain = raw_gain(k ? sdr[ch].y : sdr[ch].x, k ? hdr[ch].y : hdr[ch].x);
        px[k] |= (uint32_t)encode_gain_guarded(gain, c.min_boost, c.max_boost, c.log2_min, c.log2_max, c.enc_scale, c.enc_byte_min,
                                               c.enc_byte_max) << (8 * ch);
      }
    }
    uint32_t* mp = map + (size_t)my * c.map_w + mx;
    if (ALIGNED) {   // map_w is even and the map 8-byte aligned
      *reinterpret_cast<uint2*>(mp) = make_uint2(px[0], px[1]);
    } else {
      mp[0] = px[0];
      if (two) mp[1] = px[1];
    }
  }
}
template <int TF>
static hipError_t launch_generate_rgb_tf(const GenConsts& c, const GenBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  const bool small = generate_is_small(c, n);   // spans per block as launch_generate_t chooses them
  const unsigned per = (unsigned)kGenBlock * (small ? 1u : (unsigned)kGenTiles);
  const dim3 g((unsigned)n, (total + per - 1u) / per, 1), blk(kGenBlock, 1, 1);
  if (small) {
    if (aligned) hipLaunchKernelGGL((k_generate_rgb<TF, true, 1>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_rgb<TF, false, 1>), g, blk, 0, s, c, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_generate_rgb<TF, true, kGenTiles>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_rgb<TF, false, kGenTiles>), g, blk, 0, s, c, b);
  }
  return hipGetLastError();
}
hipError_t launch_generate_rgb(const GenConsts& c, const GenBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s) {
  switch (hdr_tf) {
    case 0: return launch_generate_rgb_tf<0>(c, b, n, aligned, s);
    case 1: return launch_generate_rgb_tf<1>(c, b, n, aligned, s);
    case 2: return launch_generate_rgb_tf<2>(c, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

// Gain maps against caller-given metadata: k_generate_rgb's grid and front end on the exact path; what
// is encoded is (hdr + offsetHdr * 203) / (sdr + offsetSdr * 203) -- of the luminances, or per channel (RGB) -- and the byte is
// t^gamma * 255, truncated.  gamma == 1 is encode_gain_guarded, the reference's bytes.  Otherwise t and the power run on the lean
// f64 log2 / exp2 (relative error < 2^-50 each): the value in front of the truncation is within 2^-36 of the libm evaluation's.
__device__ __forceinline__ uint8_t encode_gain_md(const GenConsts& c, const GenMdConsts& m, float sdr_nits, float hdr_nits) {
  const float gain = raw_gain(sdr_nits + m.off_sdr_nits, hdr_nits + m.off_hdr_nits);
  if (m.gamma_on == 0u)   // (launch-uniform)
    return encode_gain_guarded(gain, c.min_boost, c.max_boost, c.log2_min, c.log2_max, c.enc_scale, c.enc_byte_min, c.enc_byte_max);
  if (!(gain > c.min_boost)) return (uint8_t)m.byte_min;
  if (!(gain < c.max_boost)) return (uint8_t)m.byte_max;
  const double t = (fast_log2((double)gain) - (double)c.log2_min) / m.den;
  if (!(t > 0.0)) return 0;
  const double v = fast_exp2(m.gamma * fast_log2(t)) * 255.0;
  return (uint8_t)(uint32_t)fmin(v, 255.0);
}
template <int TF, bool ALIGNED, int TILES, bool RGB>
__global__ void __launch_bounds__(kGenBlock, 1) k_generate_md(const GenConsts c, const GenMdConsts m, const GenBatch b) {
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const GenImage& im = b.img[img_i];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)kGenBlock + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];
    load_pair<ALIGNED>(c, im, im_v, my, pr, two, hy, huv, y8, u8, v8);
    uint8_t o[2];
    float gn[2];
    GenMid lin;
    gen_pair<TF, false, false, false, kGenLinear>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &lin);   // (a missing second pixel: zeros, dropped)
    if (RGB) {
      const f2 sdr[3] = {lin.r * splat(203.0f), lin.g * splat(203.0f), lin.b * splat(203.0f)};
      const f2 hdr[3] = {lin.hr * splat(c.hdr_white_nits), lin.hg * splat(c.hdr_white_nits), lin.hb * splat(c.hdr_white_nits)};
      uint32_t px[2] = {0xFF000000u, 0xFF000000u};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
          px[k] |= (uint32_t)encode_gain_md(c, m, k ? sdr[ch].y : sdr[ch].x, k ? hdr[ch].y : hdr[ch].x) << (8 * ch);
      }
      uint32_t* mp = reinterpret_cast<uint32_t*>(im.map) + (size_t)my * c.map_w + mx;
      if (ALIGNED) {   // map_w is even and the map 8-byte aligned
        *reinterpret_cast<uint2*>(mp) = make_uint2(px[0], px[1]);
      } else {
        mp[0] = px[0];
        if (two) mp[1] = px[1];
      }
    } else {
      // the two luminances, as gen_pair forms them behind the linear colours
      const f2 sdr_nits = (splat(c.lum_r) * lin.r + splat(c.lum_g) * lin.g + splat(c.lum_b) * lin.b) * splat(203.0f);
      const f2 hdr_nits = (splat(c.lum_r) * lin.hr + splat(c.lum_g) * lin.hg + splat(c.lum_b) * lin.hb) * splat(c.hdr_white_nits);
      const uint8_t b0 = encode_gain_md(c, m, sdr_nits.x, hdr_nits.x), b1 = encode_gain_md(c, m, sdr_nits.y, hdr_nits.y);
      uint8_t* mp = im.map + (size_t)my * c.map_w + mx;
      if (ALIGNED) {   // map_w is even and the map 2-byte aligned
        *reinterpret_cast<uint16_t*>(mp) = (uint16_t)((uint32_t)b0 | ((uint32_t)b1 << 8));
      } else {
        mp[0] = b0;
        if (two) mp[1] = b1;
      }
    }
  }
}
template <int TF, bool RGB>
static hipError_t launch_generate_md_tf(const GenConsts& c, const GenMdConsts& m, const GenBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  const bool small = generate_is_small(c, n);   // spans per block as launch_generate_t chooses them
  const unsigned per = (unsigned)kGenBlock * (small ? 1u : (unsigned)kGenTiles);
  const dim3 g((unsigned)n, (total + per - 1u) / per, 1), blk(kGenBlock, 1, 1);
  if (small) {
    if (aligned) hipLaunchKernelGGL((k_generate_md<TF, true, 1, RGB>), g, blk, 0, s, c, m, b);
    else hipLaunchKernelGGL((k_generate_md<TF, false, 1, RGB>), g, blk, 0, s, c, m, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_generate_md<TF, true, kGenTiles, RGB>), g, blk, 0, s, c, m, b);
    else hipLaunchKernelGGL((k_generate_md<TF, false, kGenTiles, RGB>), g, blk, 0, s, c, m, b);
  }
  return hipGetLastError();
}
hipError_t launch_generate_md(const GenConsts& c, const GenMdConsts& m, const GenBatch& b, int n, int hdr_tf, bool aligned, bool rgb,
                              hipStream_t s) {
  switch (hdr_tf) {
    case 0: return rgb ? launch_generate_md_tf<0, true>(c, m, b, n, aligned, s) : launch_generate_md_tf<0, false>(c, m, b, n, aligned, s);
    case 1: return rgb ? launch_generate_md_tf<1, true>(c, m, b, n, aligned, s) : launch_generate_md_tf<1, false>(c, m, b, n, aligned, s);
    case 2: return rgb ? launch_generate_md_tf<2, true>(c, m, b, n, aligned, s) : launch_generate_md_tf<2, false>(c, m, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

// Gain maps from packed RGBA: an RGBA8888 SDR image and an RGBA1010102 (HLG / PQ) or RGBA F16 (linear) HDR
// image, strides in pixels.  A thread owns a pair of map pixels as in the other generate kernels -- an 8 x 4 pixel block of both
// images, per row 32 bytes of a dword format and 64 bytes of F16 -- and sums each channel as samplePixels does (gainmapmath.cpp:
// 605-615: dy outer, dx inner, one running f32 sum, code * (1 / max) and the add two roundings).  There is no YUV -> RGB step and no
// clamp: the six sums / 16 are what gen_pair's transfer functions start from (kGenBackLinear), and the bytes are k_generate_md's.
constexpr float k1023 = 1 / 1023.0f;
// k_generate_md's tail as a function: the pair's bytes from its two linear colours -- per channel (RGB: one RGBA pixel each), or of the
// two luminances as gen_pair forms them -- and their store.  (k_generate_md keeps its own copy: its instructions stay the parent's.)
template <bool ALIGNED, bool RGB>
__device__ __forceinline__ void encode_store_md(const GenConsts& c, const GenMdConsts& m, const GenMid& lin, uint8_t* map, uint32_t my,
                                                uint32_t mx, bool two) {
  if (RGB) {
    const f2 sdr[3] = {lin.r * splat(203.0f), lin.g * splat(203.0f), lin.b * splat(203.0f)};
    const f2 hdr[3] = {lin.hr * splat(c.hdr_white_nits), lin.hg * splat(c.hdr_white_nits), lin.hb * splat(c.hdr_white_nits)};
    uint32_t px[2] = {0xFF000000u, 0xFF000000u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int k = 0; k < 2; ++k)
        px[k] |= (uint32_t)encode_gain_md(c, m, k ? sdr[ch].y : sdr[ch].x, k ? hdr[ch].y : hdr[ch].x) << (8 * ch);
    }
    uint32_t* mp = reinterpret_cast<uint32_t*>(map) + (size_t)my * c.map_w + mx;
    if (ALIGNED) {   // map_w is even and the map 8-byte aligned
      *reinterpret_cast<uint2*>(mp) = make_uint2(px[0], px[1]);
    } else {
      mp[0] = px[0];
      if (two) mp[1] = px[1];
    }
  } else {
    // the two luminances, as gen_pair forms them behind the linear colours
    const f2 sdr_nits = (splat(c.lum_r) * lin.r + splat(c.lum_g) * lin.g + splat(c.lum_b) * lin.b) * splat(203.0f);
    const f2 hdr_nits = (splat(c.lum_r) * lin.hr + splat(c.lum_g) * lin.hg + splat(c.lum_b) * lin.hb) * splat(c.hdr_white_nits);
    const uint8_t b0 = encode_gain_md(c, m, sdr_nits.x, hdr_nits.x), b1 = encode_gain_md(c, m, sdr_nits.y, hdr_nits.y);
    uint8_t* mp = map + (size_t)my * c.map_w + mx;
    if (ALIGNED) {   // map_w is even and the map 2-byte aligned
      *reinterpret_cast<uint16_t*>(mp) = (uint16_t)((uint32_t)b0 | ((uint32_t)b1 << 8));
    } else {
      mp[0] = b0;
      if (two) mp[1] = b1;
    }
  }
}
// float of the low / high half of w, exactly (a subnormal half is a normal float; the kernel keeps the default FP mode, in which
// v_cvt_f32_f16 does not flush)
__device__ __forceinline__ float half_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }
// rows r = 0..3 of the pair's block of a dword format: px[r][0..3] the first map pixel's columns, px[r][4..7] the second's
template <bool ALIGNED>
__device__ __forceinline__ void load_packed32(const uint32_t* base, uint32_t stride, uint32_t my, uint32_t pr, bool two, uint32_t (&px)[4][8]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t* row = base + ((size_t)(4u * my + (uint32_t)r) * stride + 8u * pr);
    if (ALIGNED) {
      const uint4 a = ld_stream(reinterpret_cast<const uint4*>(row)), b = ld_stream(reinterpret_cast<const uint4*>(row) + 1);
      px[r][0] = a.x; px[r][1] = a.y; px[r][2] = a.z; px[r][3] = a.w;
      px[r][4] = b.x; px[r][5] = b.y; px[r][6] = b.z; px[r][7] = b.w;
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) px[r][x] = (x < 4 || two) ? ld_stream(row + x) : 0u;
    }
  }
}
// the same of RGBA F16: px[r][x] = (R | G << 16, B | A << 16)
template <bool ALIGNED>
__device__ __forceinline__ void load_packed64(const uint2* base, uint32_t stride, uint32_t my, uint32_t pr, bool two, uint2 (&px)[4][8]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint2* row = base + ((size_t)(4u * my + (uint32_t)r) * stride + 8u * pr);
    if (ALIGNED) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 a = ld_stream(reinterpret_cast<const uint4*>(row) + q);
        px[r][2 * q] = make_uint2(a.x, a.y); px[r][2 * q + 1] = make_uint2(a.z, a.w);
      }
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) px[r][x] = (x < 4 || two) ? ld_stream(row + x) : make_uint2(0u, 0u);
    }
  }
}
// samplePixels per channel over both blocks; TEN: 10-bit codes (RGBA1010102), otherwise bytes (RGBA8888)
template <bool TEN>
__device__ __forceinline__ void sample_packed32(const uint32_t (&px)[4][8], f2 (&e)[3]) {
  e[0] = e[1] = e[2] = splat(0.0f);
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const uint32_t p0 = px[dy][dx], p1 = px[dy][4 + dx];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const f2 code = TEN ? (f2){(float)((p0 >> (10 * ch)) & 0x3ffu), (float)((p1 >> (10 * ch)) & 0x3ffu)}
                            : (f2){(float)((p0 >> (8 * ch)) & 0xffu), (float)((p1 >> (8 * ch)) & 0xffu)};
        e[ch] += code * splat(TEN ? k1023 : k255);
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) e[ch] *= splat(0.0625f);   // e / 16.0f
}
__device__ __forceinline__ void sample_packed64(const uint2 (&px)[4][8], f2 (&e)[3]) {
  e[0] = e[1] = e[2] = splat(0.0f);
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const uint2 p0 = px[dy][dx], p1 = px[dy][4 + dx];
      e[0] += (f2){half_lo(p0.x), half_lo(p1.x)};
      e[1] += (f2){half_hi(p0.x), half_hi(p1.x)};
      e[2] += (f2){half_lo(p0.y), half_lo(p1.y)};
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) e[ch] *= splat(0.0625f);
}
template <int TF, bool F16, bool ALIGNED, int TILES, bool RGB>
__global__ void __launch_bounds__(kGenBlock, 1) k_generate_packed(const GenConsts c, const GenMdConsts m, const PackedBatch b) {
  static_assert(F16 ? TF == 0 : TF != 0, "F16 is linear light, RGBA1010102 carries HLG or PQ");
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const PackedImage& im = b.img[img_i];
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)kGenBlock + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);
    GenMid mid;
    f2 e[3];
    {
      uint32_t px[4][8];
      load_packed32<ALIGNED>(im.sdr, im.sdr_stride, my, pr, two, px);
      sample_packed32<false>(px, e);
      mid.r = e[0]; mid.g = e[1]; mid.b = e[2];
    }
    if (F16) {
      uint2 px[4][8];
      load_packed64<ALIGNED>(static_cast<const uint2*>(im.hdr), im.hdr_stride, my, pr, two, px);
      sample_packed64(px, e);
    } else {
      uint32_t px[4][8];
      load_packed32<ALIGNED>(static_cast<const uint32_t*>(im.hdr), im.hdr_stride, my, pr, two, px);
      sample_packed32<true>(px, e);
    }
    mid.hr = e[0]; mid.hg = e[1]; mid.hb = e[2];
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];   // (gen_pair's planar inputs: not read from kGenBack on)
    uint8_t o[2];
    float gn[2];
    gen_pair<TF, false, false, false, kGenBackLinear>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &mid);   // (a missing second pixel: zeros, dropped)
    encode_store_md<ALIGNED, RGB>(c, m, mid, im.map, my, mx, two);
  }
}
template <int TF, bool F16, bool RGB>
static hipError_t launch_generate_packed_tf(const GenConsts& c, const GenMdConsts& m, const PackedBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  const bool small = generate_is_small(c, n);   // spans per block as launch_generate_t chooses them
  const unsigned per = (unsigned)kGenBlock * (small ? 1u : (unsigned)kGenTiles);
  const dim3 g((unsigned)n, (total + per - 1u) / per, 1), blk(kGenBlock, 1, 1);
  if (small) {
    if (aligned) hipLaunchKernelGGL((k_generate_packed<TF, F16, true, 1, RGB>), g, blk, 0, s, c, m, b);
    else hipLaunchKernelGGL((k_generate_packed<TF, F16, false, 1, RGB>), g, blk, 0, s, c, m, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_generate_packed<TF, F16, true, kGenTiles, RGB>), g, blk, 0, s, c, m, b);
    else hipLaunchKernelGGL((k_generate_packed<TF, F16, false, kGenTiles, RGB>), g, blk, 0, s, c, m, b);
  }
  return hipGetLastError();
}
hipError_t launch_generate_packed(const GenConsts& c, const GenMdConsts& m, const PackedBatch& b, int n, int hdr_tf, bool f16, bool aligned,
                                  bool rgb, hipStream_t s) {
  if (f16 != (hdr_tf == 0)) return hipErrorInvalidValue;
  switch (hdr_tf) {
    case 0: return rgb ? launch_generate_packed_tf<0, true, true>(c, m, b, n, aligned, s) : launch_generate_packed_tf<0, true, false>(c, m, b, n, aligned, s);
    case 1: return rgb ? launch_generate_packed_tf<1, false, true>(c, m, b, n, aligned, s) : launch_generate_packed_tf<1, false, false>(c, m, b, n, aligned, s);
    case 2: return rgb ? launch_generate_packed_tf<2, false, true>(c, m, b, n, aligned, s) : launch_generate_packed_tf<2, false, false>(c, m, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

// Content-adaptive maps from packed RGBA, pass 1: k_generate_packed's front end -- its grid, its loads, its
// sampling, the SDR block summed before the HDR block is loaded, gen_pair<kGenBackLinear> -- and k_generate_gains' tail: the
// unclamped f32 gains (raw_gain) into the image's part of the workspace (PackedImage::map) and their extremes into the image's two
// key words.  One plane: the gain of the two luminances as gen_pair forms them, 4 bytes per map pixel.  RGB: the gain per channel of
// sdr.c * 203 and hdr.c * white, 12 bytes per map pixel (R, G, B), one pair of extremes over the three.  The aligned form stores a
// thread's pair in 8-byte pieces, one (RGB: three): map_w is even and the image's gains are 16-byte aligned.
template <int TF, bool F16, bool ALIGNED, int TILES, bool RGB>
__global__ void __launch_bounds__(kGenBlock, 1) k_generate_packed_gains(const GenConsts c, const PackedBatch b) {
  static_assert(F16 ? TF == 0 : TF != 0, "F16 is linear light, RGBA1010102 carries HLG or PQ");
  constexpr int NCH = RGB ? 3 : 1;
  const uint32_t img_i = blockIdx.x, blk = blockIdx.y;
  const PackedImage& im = b.img[img_i];
  float* gains = reinterpret_cast<float*>(im.map);
  const uint32_t pairs_per_row = (c.map_w + 1u) >> 1;
  const uint32_t total = pairs_per_row * c.map_h;
  float emin = __builtin_inff(), emax = -__builtin_inff();
#pragma unroll 1
  for (uint32_t t = 0; t < (uint32_t)TILES; ++t) {
    const uint32_t idx = (blk * (uint32_t)TILES + t) * (uint32_t)kGenBlock + threadIdx.x;
    if (idx >= total) break;
    const uint32_t my = idx / pairs_per_row;
    const uint32_t pr = idx - my * pairs_per_row;
    const uint32_t mx = pr * 2u;
    const bool two = ALIGNED || (mx + 1u < c.map_w);
    GenMid mid;
    f2 e[3];
    {
      uint32_t px[4][8];
      load_packed32<ALIGNED>(im.sdr, im.sdr_stride, my, pr, two, px);
      sample_packed32<false>(px, e);
      mid.r = e[0]; mid.g = e[1]; mid.b = e[2];
    }
    if (F16) {
      uint2 px[4][8];
      load_packed64<ALIGNED>(static_cast<const uint2*>(im.hdr), im.hdr_stride, my, pr, two, px);
      sample_packed64(px, e);
    } else {
      uint32_t px[4][8];
      load_packed32<ALIGNED>(static_cast<const uint32_t*>(im.hdr), im.hdr_stride, my, pr, two, px);
      sample_packed32<true>(px, e);
    }
    mid.hr = e[0]; mid.hg = e[1]; mid.hb = e[2];
    uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];   // (gen_pair's planar inputs: not read from kGenBack on)
    uint8_t o[2];
    float gn[2];
    gen_pair<TF, false, false, false, kGenBackLinear>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &mid);   // (a missing second pixel: zeros, gain 1, dropped)
    f2 g[3];   // (one plane: g[0] alone)
    if (RGB) {
      const f2 sdr[3] = {mid.r * splat(203.0f), mid.g * splat(203.0f), mid.b * splat(203.0f)};
      const f2 hdr[3] = {mid.hr * splat(c.hdr_white_nits), mid.hg * splat(c.hdr_white_nits), mid.hb * splat(c.hdr_white_nits)};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) g[ch] = (f2){raw_gain(sdr[ch].x, hdr[ch].x), raw_gain(sdr[ch].y, hdr[ch].y)};
    } else {
      // the two luminances, as gen_pair forms them behind the linear colours
      const f2 sdr_nits = (splat(c.lum_r) * mid.r + splat(c.lum_g) * mid.g + splat(c.lum_b) * mid.b) * splat(203.0f);
      const f2 hdr_nits = (splat(c.lum_r) * mid.hr + splat(c.lum_g) * mid.hg + splat(c.lum_b) * mid.hb) * splat(c.hdr_white_nits);
      g[0] = (f2){raw_gain(sdr_nits.x, hdr_nits.x), raw_gain(sdr_nits.y, hdr_nits.y)};
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      emin = fminf(emin, g[ch].x); emax = fmaxf(emax, g[ch].x);
      if (two) { emin = fminf(emin, g[ch].y); emax = fmaxf(emax, g[ch].y); }
    }
    float* gp = gains + ((size_t)my * c.map_w + mx) * (size_t)NCH;
    if (ALIGNED && RGB) {   // R0 G0 | B0 R1 | G1 B1
      float2* gp2 = reinterpret_cast<float2*>(gp);
      gp2[0] = make_float2(g[0].x, g[1].x);
      gp2[1] = make_float2(g[2].x, g[0].y);
      gp2[2] = make_float2(g[1].y, g[2].y);
    } else if (ALIGNED) {
      *reinterpret_cast<float2*>(gp) = make_float2(g[0].x, g[0].y);
    } else {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        gp[ch] = g[ch].x;
        if (two) gp[NCH + ch] = g[ch].y;
      }
    }
  }
  wave_minmax(emin, emax);   // (every lane arrives here)
  publish_minmax(emin, emax, c.stat_keys + (size_t)c.stat_stride * img_i);
}
template <int TF, bool F16, bool RGB>
static hipError_t launch_generate_packed_gains_tf(const GenConsts& c, const PackedBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t total = ((c.map_w + 1u) >> 1) * c.map_h;
  if (total == 0 || n == 0) return hipSuccess;
  const bool small = generate_is_small(c, n);   // spans per block as launch_generate_t chooses them
  const unsigned per = (unsigned)kGenBlock * (small ? 1u : (unsigned)kGenTiles);
  const dim3 g((unsigned)n, (total + per - 1u) / per, 1), blk(kGenBlock, 1, 1);
  if (small) {
    if (aligned) hipLaunchKernelGGL((k_generate_packed_gains<TF, F16, true, 1, RGB>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_packed_gains<TF, F16, false, 1, RGB>), g, blk, 0, s, c, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_generate_packed_gains<TF, F16, true, kGenTiles, RGB>), g, blk, 0, s, c, b);
    else hipLaunchKernelGGL((k_generate_packed_gains<TF, F16, false, kGenTiles, RGB>), g, blk, 0, s, c, b);
  }
  return hipGetLastError();
}
hipError_t launch_generate_packed_gains(const GenConsts& c, const PackedBatch& b, int n, int hdr_tf, bool f16, bool aligned, bool rgb,
                                        hipStream_t s) {
  if (f16 != (hdr_tf == 0) || c.stat_keys == nullptr) return hipErrorInvalidValue;
  switch (hdr_tf) {
    case 0: return rgb ? launch_generate_packed_gains_tf<0, true, true>(c, b, n, aligned, s) : launch_generate_packed_gains_tf<0, true, false>(c, b, n, aligned, s);
    case 1: return rgb ? launch_generate_packed_gains_tf<1, false, true>(c, b, n, aligned, s) : launch_generate_packed_gains_tf<1, false, false>(c, b, n, aligned, s);
    case 2: return rgb ? launch_generate_packed_gains_tf<2, false, true>(c, b, n, aligned, s) : launch_generate_packed_gains_tf<2, false, false>(c, b, n, aligned, s);
    default: return hipErrorInvalidValue;
  }
}

// =================================================================================================
// Gain maps at any scale factor (uhdr_hip_generate_gainmap_scaled_batch)
// =================================================================================================
// samplePixels (gainmapmath.cpp:605-615) at scale s: one running f32 sum per channel over the s x s block, dy outer and dx inner, of
// getYuv420Pixel / getP010Pixel values (every product its own rounding; the chroma sample of a pixel is the one at (x/2, y/2)), divided
// by (float)(s*s).  Everything behind the six sampled values is gen_pair's: the kernels here only sample.
//   S = 1, 2, 8 (aligned inputs): a thread owns a strip of 8 luma columns and S rows -- 8, 4 or 1 map pixels -- and moves per row one
//       16-byte piece of P010 luma, 8 bytes of 8-bit luma and, per chroma row, 16 bytes of P010 chroma and 4 bytes of U and of V,
//       with the non-temporal helpers.  Dividing by S*S is an exact multiply.
//   S = 0: a thread owns a pair of map pixels at the run-time factor GenScaleConsts::s and sums from single loads straight into its
//       running registers: every other factor (odd ones included, where a block straddles chroma samples) and every layout the
//       aligned form does not take.  The division is the correctly rounded f32 one.
// MODE 0: the single-channel map of the reference's metadata behind gen_pair's f32 pre-filter.  Pixels in doubt are resolved COMPACTED:
//       the thread that finds one appends its six sampled values and its place in the wave's tile to the wave's list in LDS; when the
//       wave's pixels are through the filter, consecutive lanes run the exact path over the entries, two per lane as gen_pair takes
//       them, and hand the bytes back through LDS to the owners, which then store their pixels once.  The list holds every pixel of
//       the wave's tile (an all-black SDR frame puts every pixel in doubt): there is no overflow path.  Waves never wait for each other.
// MODE 1 / 2: the exact path throughout and k_generate_md's rule -- one plane, or RGBA per channel.
__device__ __forceinline__ float yuv8_luma(uint32_t y) { return (float)y * k255; }                          // gainmapmath.cpp:579
__device__ __forceinline__ float yuv8_chroma(uint32_t u) { return (float)((int)u - 128) * k255; }           // :580
__device__ __forceinline__ float p010_y(uint32_t w) { return (float)((int)(w >> 6) - 64) * k876; }          // :598
__device__ __forceinline__ float p010_c(uint32_t w) { return (float)((int)(w >> 6) - 64) * k896 - 0.5f; }   // :599-600
__device__ __forceinline__ uint32_t half_word(uint32_t w, int hi) { return hi ? (w >> 16) : (w & 0xffffu); }

// yuvToRgb of both images and clampPixelFloat, as gen_pair has them in front of its transfer functions
__device__ __forceinline__ GenMid sampled_to_mid(const GenConsts& c, f2 sy, f2 su, f2 sv, f2 hsy, f2 hsu, f2 hsv) {
  GenMid m;
  m.r = pk_add_sat(sy, splat(c.sdr_cr) * sv);
  m.g = pk_add_sat(sy - splat(c.sdr_gcb) * su, -(splat(c.sdr_gcr) * sv));
  m.b = pk_add_sat(sy, splat(c.sdr_cb) * su);
  m.hr = pk_add_sat(hsy, splat(c.hdr_cr) * hsv);
  m.hg = pk_add_sat(hsy - splat(c.hdr_gcb) * hsu, -(splat(c.hdr_gcr) * hsv));
  m.hb = pk_add_sat(hsy, splat(c.hdr_cb) * hsu);
  return m;
}

// the strip (8 luma columns from 8 * sx, S rows from S * my) of the aligned forms: acc[channel][map pixel], channels sy su sv hsy hsu hsv
template <int S>
__device__ __forceinline__ void sample_strip(const GenImage& im, const uint8_t* im_v, uint32_t my, uint32_t sx, float (&acc)[6][8 / S]) {
  constexpr int NPX = 8 / S;
#pragma unroll
  for (int ch = 0; ch < 6; ++ch)
#pragma unroll
    for (int p = 0; p < NPX; ++p) acc[ch][p] = 0.0f;
  const uint32_t x0 = 8u * sx;
  float uf[4], vf[4], huf[4], hvf[4];
#pragma unroll
  for (int dy = 0; dy < S; ++dy) {
    const uint32_t y = (uint32_t)S * my + (uint32_t)dy;
    const uint4 q = ld_stream(reinterpret_cast<const uint4*>(im.hy + ((size_t)y * im.hy_stride + x0)));
    const uint2 p8 = ld_stream(reinterpret_cast<const uint2*>(im.y + ((size_t)y * im.y_stride + x0)));
    if (S == 1 || (dy & 1) == 0) {   // (S even: the strip starts on an even row)
      const uint32_t cy = y >> 1;
      const uint4 cq = ld_stream(reinterpret_cast<const uint4*>(im.huv + ((size_t)cy * im.huv_stride + x0)));
      const uint32_t uu = ld_stream(reinterpret_cast<const uint32_t*>(im.u + ((size_t)cy * im.c_stride + (x0 >> 1))));
      const uint32_t vv = ld_stream(reinterpret_cast<const uint32_t*>(im_v + ((size_t)cy * im.c_stride + (x0 >> 1))));
      const uint32_t cw[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uf[k] = yuv8_chroma((uu >> (8 * k)) & 0xffu);
        vf[k] = yuv8_chroma((vv >> (8 * k)) & 0xffu);
        huf[k] = p010_c(cw[k] & 0xffffu);
        hvf[k] = p010_c(cw[k] >> 16);
      }
    }
    const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
    const uint32_t pw[2] = {p8.x, p8.y};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = j / S;
      acc[0][p] += yuv8_luma((pw[j >> 2] >> (8 * (j & 3))) & 0xffu);
      acc[1][p] += uf[j >> 1];
      acc[2][p] += vf[j >> 1];
      acc[3][p] += p010_y(half_word(qw[j >> 1], j & 1));
      acc[4][p] += huf[j >> 1];
      acc[5][p] += hvf[j >> 1];
    }
  }
  if (S != 1) {   // e / float(S*S): a power of two
#pragma unroll
    for (int ch = 0; ch < 6; ++ch)
#pragma unroll
      for (int p = 0; p < NPX; ++p) acc[ch][p] *= 1.0f / (float)(S * S);
  }
}

// the pair of map pixels (mx, my), (mx + 1, my) at the run-time factor; a missing second pixel reads the first one's samples again
__device__ __forceinline__ GenMid sample_pair_any(const GenConsts& c, const GenScaleConsts& sc, const GenImage& im, const uint8_t* im_v,
                                                  uint32_t my, uint32_t mx, bool two) {
  const uint32_t s = sc.s;
  const uint32_t xa0 = mx * s, xb0 = two ? xa0 + s : xa0;
  f2 sy = splat(0.0f), su = splat(0.0f), sv = splat(0.0f), hsy = splat(0.0f), hsu = splat(0.0f), hsv = splat(0.0f);
#pragma unroll 1
  for (uint32_t dy = 0; dy < s; ++dy) {
    const size_t y = (size_t)my * s + dy, cy = y >> 1;
    const uint8_t* yrow = im.y + y * im.y_stride;
    const uint16_t* hrow = im.hy + y * im.hy_stride;
    const uint8_t* urow = im.u + cy * im.c_stride;
    const uint8_t* vrow = im_v + cy * im.c_stride;
    const uint16_t* crow = im.huv + cy * im.huv_stride;
#pragma unroll 1
    for (uint32_t dx = 0; dx < s; ++dx) {
      const uint32_t xa = xa0 + dx, xb = xb0 + dx;
      sy += (f2){yuv8_luma(ld8(yrow + xa)), yuv8_luma(ld8(yrow + xb))};
      su += (f2){yuv8_chroma(ld8(urow + (xa >> 1))), yuv8_chroma(ld8(urow + (xb >> 1)))};
      sv += (f2){yuv8_chroma(ld8(vrow + (xa >> 1))), yuv8_chroma(ld8(vrow + (xb >> 1)))};
      hsy += (f2){p010_y(ld16(hrow + xa)), p010_y(ld16(hrow + xb))};
      hsu += (f2){p010_c(ld16(crow + (xa & ~1u))), p010_c(ld16(crow + (xb & ~1u)))};
      hsv += (f2){p010_c(ld16(crow + (xa & ~1u) + 1u)), p010_c(ld16(crow + (xb & ~1u) + 1u))};
    }
  }
  const float a = sc.area;   // (float)(s*s); the division is the correctly rounded one (the build keeps hipcc's default)
  sy = (f2){sy.x / a, sy.y / a}; su = (f2){su.x / a, su.y / a}; sv = (f2){sv.x / a, sv.y / a};
  hsy = (f2){hsy.x / a, hsy.y / a}; hsu = (f2){hsu.x / a, hsu.y / a}; hsv = (f2){hsv.x / a, hsv.y / a};
  return sampled_to_mid(c, sy, su, sv, hsy, hsu, hsv);
}

__device__ __forceinline__ float mid_word(const GenMid& m, int ch, int k) {
  const f2 v = ch == 0 ? m.r : ch == 1 ? m.g : ch == 2 ? m.b : ch == 3 ? m.hr : ch == 4 ? m.hg : m.hb;
  return k ? v.y : v.x;
}

// Geometry: blocks of kScaledBlock threads, one unit (strip or pair) per thread, units in row-major order; grid = (image, y, z) with
// block y + z * gridDim.y of the image.  MODE 0 keeps per wave 64 * NPX list entries of 7 words and as many bytes in LDS.
constexpr int scaled_px(int s) { return s != 0 ? 8 / s : 2; }   // map pixels of a thread: a strip's, or a pair
template <int TF, int S, int MODE>
__global__ void __launch_bounds__(kScaledBlock) k_generate_scaled(const GenConsts c, const GenMdConsts m, const GenScaleConsts sc, const GenBatch b) {
  constexpr int NPX = scaled_px(S);          // map pixels of a thread ...
  constexpr int NP = (NPX + 1) / 2;           // ... in this many pairs
  constexpr uint32_t kCap = 64u * NPX;        // map pixels of a wave's tile
  constexpr uint32_t kWaves = kScaledBlock / 64;
  const GenImage& im = b.img[blockIdx.x];
  const uint8_t* im_v = im.u + (size_t)im.c_stride * (c.height / 2u);
  const uint32_t units_per_row = S != 0 ? c.width / 8u : (c.map_w + 1u) >> 1;
  const uint32_t total = units_per_row * c.map_h;
  const uint32_t idx = (blockIdx.z * gridDim.y + blockIdx.y) * (uint32_t)kScaledBlock + threadIdx.x;
  const bool live = idx < total;
  if (MODE != 0 && !live) return;
  if (MODE == 0 && (idx & ~63u) >= total) return;   // (the whole wave)
  const uint32_t my = live ? idx / units_per_row : 0u;
  const uint32_t ux = live ? idx - my * units_per_row : 0u;
  const uint32_t mx = ux * (uint32_t)NPX;
  const bool two = S != 0 ? NPX > 1 : (mx + 1u < c.map_w);

  GenMid mid[NP];
  if constexpr (S != 0) {
    float acc[6][NPX];
    if (live) {
      sample_strip<S>(im, im_v, my, ux, acc);
    } else {
#pragma unroll
      for (int ch = 0; ch < 6; ++ch)
#pragma unroll
        for (int p = 0; p < NPX; ++p) acc[ch][p] = 0.0f;
    }
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      const int p0 = 2 * pp, p1 = NPX > 1 ? 2 * pp + 1 : 0;   // (a strip of one map pixel: the pair's second is a copy, dropped)
      mid[pp] = sampled_to_mid(c, (f2){acc[0][p0], acc[0][p1]}, (f2){acc[1][p0], acc[1][p1]}, (f2){acc[2][p0], acc[2][p1]},
                               (f2){acc[3][p0], acc[3][p1]}, (f2){acc[4][p0], acc[4][p1]}, (f2){acc[5][p0], acc[5][p1]});
    }
  } else {
    if (live) mid[0] = sample_pair_any(c, sc, im, im_v, my, mx, two);
    else mid[0] = sampled_to_mid(c, splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f));
  }

  uint32_t hy[2][4][2], huv[2][2][2], y8[2][4], u8[2][2], v8[2][2];   // (gen_pair's planar inputs: not read from kGenBack on)
  uint8_t o[2];
  float gn[2];
  if (MODE != 0) {
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      GenMid lin = mid[pp];
      gen_pair<TF, false, false, false, kGenBackLinear>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &lin);
      if constexpr (S != 0 && NPX > 1) encode_store_md<true, MODE == 2>(c, m, lin, im.map, my, mx + 2u * pp, true);
      else encode_store_md<false, MODE == 2>(c, m, lin, im.map, my, mx, two);
    }
    return;
  }

  __shared__ float s_list[kWaves][7][kCap];
  __shared__ uint8_t s_byte[kWaves][kCap];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t bytes[NPX], doubt = 0u;
#pragma unroll
  for (int pp = 0; pp < NP; ++pp) {
    const uint32_t ex = gen_pair<TF, false, true, true, kGenBack>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &mid[pp]);
    bytes[2 * pp] = o[0];
    if constexpr (NPX > 1) bytes[2 * pp + 1] = o[1];
    doubt |= ((ex >> 2) & 3u) << (2 * pp);
  }
  doubt &= !live ? 0u : (NPX > 1 && two) ? (1u << NPX) - 1u : 1u;
  uint32_t cnt = 0u;   // entries of the wave's list (wave-uniform)
#pragma unroll
  for (int k = 0; k < NPX; ++k) {
    const bool mine = ((doubt >> k) & 1u) != 0u;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
    if (mask != 0ull) {
      const uint32_t pos = cnt + (uint32_t)__builtin_popcountll(mask & below);
      if (mine) {
#pragma unroll
        for (int ch = 0; ch < 6; ++ch) s_list[wave][ch][pos] = mid_word(mid[k >> 1], ch, k & 1);
        s_list[wave][6][pos] = __uint_as_float(lane * (uint32_t)NPX + (uint32_t)k);
      }
      cnt += (uint32_t)__builtin_popcountll(mask);
    }
  }
  if (sc.doubt_count != nullptr && cnt != 0u && lane == 0u) atomicAdd(sc.doubt_count, cnt);   // (the probe only: launch-uniform null otherwise)
  if (cnt != 0u) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll 1
    for (uint32_t e0 = 0u; e0 < cnt; e0 += 128u) {
      const uint32_t i0 = e0 + 2u * lane, i1 = i0 + 1u;
      const bool have0 = i0 < cnt, have1 = i1 < cnt;
      const uint32_t j0 = have0 ? i0 : 0u, j1 = have1 ? i1 : j0;   // (a lane without an entry evaluates a copy and drops it)
      GenMid em;
      em.r = (f2){s_list[wave][0][j0], s_list[wave][0][j1]};
      em.g = (f2){s_list[wave][1][j0], s_list[wave][1][j1]};
      em.b = (f2){s_list[wave][2][j0], s_list[wave][2][j1]};
      em.hr = (f2){s_list[wave][3][j0], s_list[wave][3][j1]};
      em.hg = (f2){s_list[wave][4][j0], s_list[wave][4][j1]};
      em.hb = (f2){s_list[wave][5][j0], s_list[wave][5][j1]};
      const uint32_t t0 = __float_as_uint(s_list[wave][6][j0]), t1 = __float_as_uint(s_list[wave][6][j1]);
      gen_pair<TF, false, false, false, kGenBack>(c, hy, huv, y8, u8, v8, o, gn, nullptr, nullptr, &em);
      if (have0) s_byte[wave][t0] = o[0];
      if (have1) s_byte[wave][t1] = o[1];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
    for (int k = 0; k < NPX; ++k)
      if ((doubt >> k) & 1u) bytes[k] = s_byte[wave][lane * (uint32_t)NPX + (uint32_t)k];
  }
  if (!live) return;
  uint8_t* mp = im.map + (size_t)my * c.map_w + mx;
  if constexpr (S == 1) {
    st_stream(reinterpret_cast<uint2*>(mp), make_uint2(bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24),
                                                        bytes[4] | (bytes[5] << 8) | (bytes[6] << 16) | (bytes[7] << 24)));
  } else if constexpr (S == 2) {
    *reinterpret_cast<uint32_t*>(mp) = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
  } else {
    mp[0] = (uint8_t)bytes[0];
    if constexpr (NPX > 1) { if (two) mp[1] = (uint8_t)bytes[1]; }
  }
}

template <int TF, int S>
static hipError_t launch_generate_scaled_s(const GenConsts& c, const GenMdConsts& m, const GenScaleConsts& sc, const GenBatch& b, int n,
                                           int mode, hipStream_t s) {
  const uint64_t units = (uint64_t)(S != 0 ? c.width / 8u : (c.map_w + 1u) >> 1) * c.map_h;
  if (units == 0u || n == 0) return hipSuccess;
  const uint64_t blocks = (units + kScaledBlock - 1u) / kScaledBlock;
  if (units > 0xFFFFFFFFull || blocks > 65535ull * 65535ull) return hipErrorInvalidValue;
  const unsigned gy = (unsigned)(blocks < 65535u ? blocks : 65535u), gz = (unsigned)((blocks + gy - 1u) / gy);
  const dim3 g((unsigned)n, gy, gz), blk(kScaledBlock, 1, 1);
  if (mode == 0) hipLaunchKernelGGL((k_generate_scaled<TF, S, 0>), g, blk, 0, s, c, m, sc, b);
  else if (mode == 1) hipLaunchKernelGGL((k_generate_scaled<TF, S, 1>), g, blk, 0, s, c, m, sc, b);
  else hipLaunchKernelGGL((k_generate_scaled<TF, S, 2>), g, blk, 0, s, c, m, sc, b);
  return hipGetLastError();
}
template <int TF>
static hipError_t launch_generate_scaled_tf(const GenConsts& c, const GenMdConsts& m, const GenScaleConsts& sc, const GenBatch& b, int n,
                                            bool aligned, int mode, hipStream_t s) {
  if (aligned && sc.s == 1u) return launch_generate_scaled_s<TF, 1>(c, m, sc, b, n, mode, s);
  if (aligned && sc.s == 2u) return launch_generate_scaled_s<TF, 2>(c, m, sc, b, n, mode, s);
  if (aligned && sc.s == 8u) return launch_generate_scaled_s<TF, 8>(c, m, sc, b, n, mode, s);
  return launch_generate_scaled_s<TF, 0>(c, m, sc, b, n, mode, s);
}
hipError_t launch_generate_scaled(const GenConsts& c, const GenMdConsts& m, const GenScaleConsts& sc, const GenBatch& b, int n, int hdr_tf,
                                  bool aligned, int mode, hipStream_t s) {
  if (sc.s == 0u || mode < 0 || mode > 2) return hipErrorInvalidValue;
  switch (hdr_tf) {
    case 0: return launch_generate_scaled_tf<0>(c, m, sc, b, n, aligned, mode, s);
    case 1: return launch_generate_scaled_tf<1>(c, m, sc, b, n, aligned, mode, s);
    case 2: return launch_generate_scaled_tf<2>(c, m, sc, b, n, aligned, mode, s);
    default: return hipErrorInvalidValue;
  }
}

// The range rule (include/uhdr_hip.h, uhdr_hip_adaptive_boost_range: the same f32 operations) and, from the range, what
// generate_consts / encode_constants derive on the host for a fixed one: the two logarithms as (float)log2((double)boost), the
// scale of encode_gain_guarded's in-range path and the bytes encodeGain yields for a gain on either clamp.  One block: image i is
// thread i's (strided).  per_call: every image gets the range of the pooled extremes -- the keys are ~key(min) and key(max), so
// pooling is a maximum of both words -- joined with carry_in's; the pooled pair goes to carry_out.
__global__ void __launch_bounds__(256) k_adaptive_consts(const uint32_t* keys, int n, int per_call, float cap, AdaptConsts* consts,
                                                         float* content_minmax, float* boost_range, const uint32_t* carry_in,
                                                         uint32_t* carry_out) {
  __shared__ uint32_t s_k[2];
  if (threadIdx.x < 2u) s_k[threadIdx.x] = (per_call && carry_in != nullptr) ? carry_in[threadIdx.x] : 0u;
  __syncthreads();
  if (per_call) {
    uint32_t k0 = 0u, k1 = 0u;
    for (int i = (int)threadIdx.x; i < n; i += 256) { k0 = max(k0, keys[2 * i]); k1 = max(k1, keys[2 * i + 1]); }
    if (k1 != 0u) { atomicMax(&s_k[0], k0); atomicMax(&s_k[1], k1); }
    __syncthreads();
    if (carry_out != nullptr && threadIdx.x < 2u) carry_out[threadIdx.x] = s_k[threadIdx.x];
  }
  for (int i = (int)threadIdx.x; i < n; i += 256) {
    uint32_t k0 = keys[2 * i], k1 = keys[2 * i + 1];
    if (content_minmax != nullptr) {   // the image's own extremes in either scope (an image without map pixels: +inf, -inf)
      content_minmax[2 * i] = k1 != 0u ? key_to_float(~k0) : __builtin_inff();
      content_minmax[2 * i + 1] = k1 != 0u ? key_to_float(k1) : -__builtin_inff();
    }
    if (per_call) { k0 = s_k[0]; k1 = s_k[1]; }
    const float g_min = k1 != 0u ? key_to_float(~k0) : __builtin_inff(), g_max = k1 != 0u ? key_to_float(k1) : -__builtin_inff();
    AdaptConsts a;
    a.min_boost = fminf(fmaxf(g_min, 0.25f), 1.0f);
    a.max_boost = fminf(fmaxf(g_max, 1.0625f), cap);
    a.log2_min = log2_to_float(a.min_boost);
    a.log2_max = log2_to_float(a.max_boost);
    a.enc_scale = (double)255.0f / (double)(a.log2_max - a.log2_min);
    a.enc_byte_min = encode_gain(a.min_boost, a.min_boost, a.max_boost, a.log2_min, a.log2_max);
    a.enc_byte_max = encode_gain(a.max_boost, a.min_boost, a.max_boost, a.log2_min, a.log2_max);
    consts[i] = a;
    boost_range[2 * i] = a.min_boost;
    boost_range[2 * i + 1] = a.max_boost;
  }
}
hipError_t launch_adaptive_consts(const uint32_t* keys, int n, int per_call, float cap, AdaptConsts* consts, float* content_minmax,
                                  float* boost_range, const uint32_t* carry_in, uint32_t* carry_out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_adaptive_consts, dim3(1), dim3(256), 0, s, keys, n, per_call, cap, consts, content_minmax, boost_range, carry_in,
                     carry_out);
  return hipGetLastError();
}

// Pass 2: the reference's three-argument encodeGain on the stored gains with the image's constants from device memory
// (encode_gain_guarded: the clamp bytes, the lean f64 log2 and its distance-to-integer test, the exact path behind it).  A thread
// takes four consecutive map pixels: one 16-byte load, one 4-byte store where the map allows it.
__global__ void __launch_bounds__(256) k_encode_gains(const AdaptConsts* consts, const EncGainBatch b, uint32_t pixels) {
  const EncGainImage& im = b.img[blockIdx.y];
  const uint32_t p = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (p >= pixels) return;
  const AdaptConsts a = consts[blockIdx.y];
  const uint32_t cnt = min(4u, pixels - p);
  float g[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  if (cnt == 4u) {
    const float4 v = *reinterpret_cast<const float4*>(im.gains + p);
    g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) if (k < cnt) g[k] = im.gains[p + k];
  }
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = encode_gain_guarded(g[k], a.min_boost, a.max_boost, a.log2_min, a.log2_max, a.enc_scale, a.enc_byte_min, a.enc_byte_max);
  uint8_t* mp = im.map + p;
  if (cnt == 4u && (reinterpret_cast<uintptr_t>(mp) & 3u) == 0u) {
    *reinterpret_cast<uint32_t*>(mp) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) if (k < cnt) mp[k] = (uint8_t)o[k];
  }
}
hipError_t launch_encode_gains(const AdaptConsts* consts, const EncGainBatch& b, int n, uint32_t pixels, hipStream_t s) {
  if (n <= 0 || pixels == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_encode_gains, dim3((pixels + 1023u) / 1024u, (unsigned)n), dim3(256), 0, s, consts, b, pixels);
  return hipGetLastError();
}
// Pass 2 of RGB maps: the same rule on the three stored gains of a map pixel (k_generate_packed_gains:
// 12 bytes per pixel), the pixel R | G << 8 | B << 16 | 0xFF << 24.  A thread takes four consecutive map pixels: three 16-byte
// loads, one 16-byte store where the map allows it.
__global__ void __launch_bounds__(256) k_encode_gains_rgb(const AdaptConsts* consts, const EncGainBatch b, uint32_t pixels) {
  const EncGainImage& im = b.img[blockIdx.y];
  const uint32_t p = (blockIdx.x * 256u + threadIdx.x) * 4u;
  if (p >= pixels) return;
  const AdaptConsts a = consts[blockIdx.y];
  const uint32_t cnt = min(4u, pixels - p);
  const float* gp = im.gains + (size_t)p * 3u;
  float g[12];
  if (cnt == 4u) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 v = reinterpret_cast<const float4*>(gp)[q];
      g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 12u; ++k) g[k] = k < 3u * cnt ? gp[k] : 1.0f;
  }
  uint32_t o[4] = {0xFF000000u, 0xFF000000u, 0xFF000000u, 0xFF000000u};
#pragma unroll
  for (int k = 0; k < 12; ++k)
    o[k / 3] |= (uint32_t)encode_gain_guarded(g[k], a.min_boost, a.max_boost, a.log2_min, a.log2_max, a.enc_scale, a.enc_byte_min,
                                              a.enc_byte_max) << (8 * (k % 3));
  uint32_t* mp = reinterpret_cast<uint32_t*>(im.map) + p;
  if (cnt == 4u && (reinterpret_cast<uintptr_t>(mp) & 15u) == 0u) {
    *reinterpret_cast<uint4*>(mp) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) if (k < cnt) mp[k] = o[k];
  }
}
hipError_t launch_encode_gains_rgb(const AdaptConsts* consts, const EncGainBatch& b, int n, uint32_t pixels, hipStream_t s) {
  if (n <= 0 || pixels == 0u) return hipSuccess;
  hipLaunchKernelGGL(k_encode_gains_rgb, dim3((pixels + 1023u) / 1024u, (unsigned)n), dim3(256), 0, s, consts, b, pixels);
  return hipGetLastError();
}

// =================================================================================================
// apply
// =================================================================================================

// FMT: 1 HDR_LINEAR (F16), 2 HDR_PQ, 3 HDR_HLG, 4 HDR_LINEAR_RGB_10BIT (ultrahdr.h:56-64)

// Everything of ultrahdr.cpp:431-451 after the loads, for one pixel: BT.601 YUV->RGB was folded
// into (yf, crv, gcbu, gcrv, cbu) by the caller, `gain` is sampleMap's result.
template <bool EXACT>
__device__ __forceinline__ F3 recover_hdr(const AppConsts& c, float yf, float crv, float gcbu,
                                          float gcrv, float cbu, float gain) {
  float r = clamp01(yf + crv);
  float g = clamp01(yf - gcbu - gcrv);
  float b = clamp01(yf + cbu);
  // applyGain(e, gain, metadata, displayBoost)   gainmapmath.cpp:550-555
  const float log_boost = (float)(c.log2_min_d * (double)(1.0f - gain) + c.log2_max_d * (double)gain);
  F3 o;
  if (EXACT) {
    // the reference's double-precision pow / exp2, as lean f64 + a rounding test (uhdr_device_math.h): the float each call
    // returns is the one the libm call rounds to (tests/test_gpu_transfer_exhaustive.py), three channels in lock step
    float ch[3] = {r, g, b};
    srgb_inv_oetf_guarded_n<3>(ch);
    r = ch[0]; g = ch[1]; b = ch[2];
    const float factor = exp2_to_float_guarded(log_boost * c.display_boost / c.max_boost);
    o.x = (r * factor) / c.display_boost;  // ultrahdr.cpp:451
    o.y = (g * factor) / c.display_boost;
    o.z = (b * factor) / c.display_boost;
  } else {
    r = srgb_inv_oetf_fast(r); g = srgb_inv_oetf_fast(g); b = srgb_inv_oetf_fast(b);
    const float factor = __builtin_amdgcn_exp2f((log_boost * c.display_boost) * c.inv_max_boost);
    o.x = (r * factor) * c.inv_display_boost;
    o.y = (g * factor) * c.inv_display_boost;
    o.z = (b * factor) * c.inv_display_boost;
  }
  return o;
}

// (hdr_oetf, map_to_float and map_to_float_fast: uhdr_apply_px.h)

// ---- FAST path, scale factor 4 ---------------------------------------------------------------
// Thread = one gain-map cell = a 4x4 pixel block.  The four map taps and the four 2x2 chroma samples
// are loaded once and shared by the 16 pixels; each output row of the block leaves as one 16 B
// (1010102) / 2x16 B (F16) / 3x8 B (planar 10 bit) store per lane, so a wave64 writes 1 KiB contiguous
// per row.  The kernel is bound by VALU issue, not by HBM (13 special-function ops per pixel, see
// DESIGN.md section 6), so the arithmetic is organised to minimise issue slots:
//   * two horizontally adjacent pixels (they share one chroma sample) are processed as one packed
//     float2 (v_pk_mul/add/fma_f32: two pixels per 4-cycle issue slot);
//   * gain -> log-boost -> display scaling collapse into one exponent:
//       factor/display_boost = 2^E,  E = sum_i e_i*(w_i*A) + B,
//       A = (log2 max - log2 min) * display_boost / max,  B = log2 min * display_boost / max - log2 display_boost
//     with the products w_i*A pre-multiplied on the host (AppFast::wA, SGPR operands);
//   * the *1023 of the 10-bit pack is folded into the OETF constants;
//   * clamps are written as min(max()) so that they fold into the producing add's clamp modifier.
__device__ __forceinline__ f2 log2_2(f2 v) { return (f2){__builtin_amdgcn_logf(v.x), __builtin_amdgcn_logf(v.y)}; }
__device__ __forceinline__ f2 exp2_2(f2 v) { return (f2){__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y)}; }
__device__ __forceinline__ f2 sqrt_2(f2 v) { return (f2){__builtin_amdgcn_sqrtf(v.x), __builtin_amdgcn_sqrtf(v.y)}; }
__device__ __forceinline__ f2 rcp_2(f2 v) { return (f2){__builtin_amdgcn_rcpf(v.x), __builtin_amdgcn_rcpf(v.y)}; }
__device__ __forceinline__ f2 sel_le(f2 x, float thr, f2 a, f2 b) {  // x <= thr ? a : b
  return (f2){x.x <= thr ? a.x : b.x, x.y <= thr ? a.y : b.y};
}

// The piecewise transfer functions are evaluated WITHOUT per-lane selects (v_cmp + v_cndmask cost 2 issue
// slots per value and cannot be packed).  For a function  f(e) = A(e) for e <= j,  B(e) for e > j :
//     f(e) = A(min(e, j)) - A(j) + B(max(e, j)),
// with  min(e, j) = j * sat(e / j)  and  max(e, j) = j + sat(e - j)  (0 <= e <= ~1), both packed ops with the
// clamp modifier.  The identity is exact for e > j; for e <= j it adds B(j) - A(j), the reference function's own
// jump at the junction (2.3e-9 for sRGB, ~1e-7 for HLG): far inside the 1-LSB tolerance.

// sRGB EOTF of two values (gainmapmath.cpp:149-155): x^2.4 = x^2 * 2^(0.4 log2 x)
__device__ __forceinline__ f2 srgb_eotf2(f2 e) {
  constexpr float kThr = 0.04045f;
  const f2 a = pk_mul_sat(e, splat(1.0f / kThr));                                      // min(e, thr) / thr
  const f2 lin = pk_fma(a, splat(kThr / 12.92f), splat(-(kThr / 12.92f)));             // lin(min) - lin(thr)
  const f2 d = pk_add_sat(e, splat(-kThr));                                            // max(e, thr) - thr
  const f2 x = pk_fma(d, splat(1.0f / 1.055f), splat((kThr + 0.055f) / 1.055f));
  const f2 t = exp2_2(log2_2(x) * splat(0.4f));
  return pk_fma(x * x, t, lin);
}

// ---- transfer functions as line segments in LDS ---------------------------------------------------
// Both transfer functions of a channel -- the sRGB EOTF in front of the gain, the HLG / PQ OETF behind it -- cost 13 (PQ: 22)
// special-function evaluations per pixel on the VALU; they are read from line-segment tables in LDS instead (the LDS pipe is
// otherwise idle in this kernel).  What bounds a table in LDS is not its size but bank conflicts: 32 lanes reading 32 random
// 8-byte entries take 3-4 cycles instead of 1, and six such gathers per pixel made the LDS the bottleneck (PMC: 2/3 of its
// cycles were conflicts).  So the path is arranged for ONE conflicting gather per value (uhdr_kernels.h has the arithmetic):
//   stage 1: T(c) = EOTF(c)^g.  Cell = bits 14..3 of the half-precision bit pattern of c: v_cvt_pkrtz_f16_f32 converts two
//     values in one issue slot, one v_and each (the upper half through SDWA's WORD_1 select) gives the byte offset of the
//     8-byte (c0, c1) entry as it stands; one ds_read_b64, one fma.  Shared table, 15 KiB, conflicts as they come.
//   u = T * 2^(g E) is formed as s = 2 + 2u by one packed fma; s lies in [2, 4], so byte 2 of its bit pattern IS the number of
//     its 1/128-wide cell: v_perm_b32 puts that byte next to the lane's slot number -- the address of a private copy of the
//     entry (cell * 256 + (lane & 31) * 8).  32 lanes, 32 different bank pairs: no conflict whatever the pixels hold.
//   stage 2: the fma on that entry yields -(2 + code 2^-22) rounded toward zero (the kernel runs in that rounding mode), whose
//     bits are 0xC0000000 | code: the pixel is two v_lshl_or_b32 of the three results.
// Errors: stage 1 <= 2e-6 relative; stage 2 <= 0.05 codes next to the HLG junction, <= 0.01 elsewhere and for PQ
// (tests/test_gpu_apply_tables.py measures both for every float).
// byte offset of the cell of one value (diagnostics; the kernel converts two at a time)
__device__ __forceinline__ uint32_t tab_offset(float x) {
  typedef __fp16 h2 __attribute__((ext_vector_type(2)));
  const h2 q = __builtin_amdgcn_cvt_pkrtz(x, 0.0f);
  return __builtin_bit_cast(uint32_t, q) & 0x7FF8u;
}
// stage-1 tables for g < 1: the byte offset of a value's cell is its own bits 27..19 (the low five exponent bits -- the kernel's
// inputs are 0 or lie in [2^-31, 1], exponents 96..127: build_stage1 in uhdr_capi.hip -- and the top four of the mantissa), in
// place: one SDWA v_and on the upper half.  4 KiB per table; offset 0 is the entry of the input 0.
__device__ __forceinline__ uint32_t pow_offset(float x) {
  uint32_t off;
  asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(off) : "v"(0x0FF8u), "v"(x));
  return off;
}
__device__ __forceinline__ void pow_pair(f2 x, const char* lut, float2& a, float2& b) {
  a = *reinterpret_cast<const float2*>(lut + pow_offset(x.x));
  b = *reinterpret_cast<const float2*>(lut + pow_offset(x.y));
}
template <uint32_t BASE>
__device__ __forceinline__ void tab_pair(f2 x, const char* lut, float2& a, float2& b) {
  typedef __fp16 h2 __attribute__((ext_vector_type(2)));
  const h2 q = __builtin_amdgcn_cvt_pkrtz(x.x, x.y);
  const uint32_t d = __builtin_bit_cast(uint32_t, q);
  uint32_t hi_off;
  asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(hi_off) : "v"(0x7FF8u), "v"(d));
  a = *reinterpret_cast<const float2*>(lut + BASE + (d & 0x7FF8u));
  b = *reinterpret_cast<const float2*>(lut + BASE + hi_off);
}
// c0 + c1 * x for both values.  Two plain fmas on purpose (asm: the vectoriser would re-pack them behind three v_movs that shuffle
// the operands into pairs)
template <uint32_t BASE>
__device__ __forceinline__ f2 tab_eval2(f2 x, const char* lut) {
  float2 a, b;
  tab_pair<BASE>(x, lut, a, b);
  f2 o;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o.x) : "v"(a.y), "v"(x.x), "v"(a.x));
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o.y) : "v"(b.y), "v"(x.y), "v"(b.x));
  return o;
}
// stage 2 on s = 2 + 2u (both values): the lane's private copy of the cell's entry sits at byte2(s) * 256 + slot8
__device__ __forceinline__ uint32_t s2_address(float s, uint32_t slot8) {
  return __builtin_amdgcn_perm(__float_as_uint(s), slot8, 0x0C0C0600u);   // {0, 0, s.byte2, slot8.byte0}
}
__device__ __forceinline__ f2 code_eval2(f2 s, uint32_t slot8, const char* lut) {   // lut: the stage-2 table
  const float2 a = *reinterpret_cast<const float2*>(lut + s2_address(s.x, slot8));
  const float2 b = *reinterpret_cast<const float2*>(lut + s2_address(s.y, slot8));
  f2 o;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o.x) : "v"(a.y), "v"(s.x), "v"(a.x));
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o.y) : "v"(b.y), "v"(s.y), "v"(b.x));
  return o;
}

// LDS layout of the kernel for an output format: the replicated stage-2 table (HLG / PQ output of a call whose values stay within
// [0, 1]), then the stage-1 table
template <int FMT, bool MASK> struct ApplyTab {
  static constexpr bool kOetf = !MASK && (FMT == 2 || FMT == 3);
  static constexpr uint32_t kS1Bytes = kOetf ? kTabS1PowBytes : kTabS1Bytes;   // at LDS offset 0: its cell offsets are addresses
  static constexpr uint32_t kS2Base = kS1Bytes;
  static constexpr uint32_t kS2Bytes = kOetf ? kTabS2LdsBytes : 0u;
  static constexpr uint32_t kBytes = kS1Bytes + kS2Bytes;
  static constexpr uint32_t kS1Float = !kOetf ? kTabS1Lin : FMT == 3 ? kTabS1Hlg : kTabS1Pq;
  static constexpr uint32_t kS2Float = FMT == 3 ? kTabS2Hlg : kTabS2Pq;
};

// OETF of two linear values, scaled to 10-bit code units where the format is 10 bit: the special-function forms, used where the
// values may exceed 1.0 (max_display_boost < maxContentBoost: the tables end at 1.0, and the HLG junction is selected per lane
// because max(e, j) - j cannot be had from a [0,1] clamp) and for the two linear formats.
template <int FMT>
__device__ __forceinline__ f2 oetf2_scaled(f2 e) {
  if (FMT == 3) {  // HLG (gainmapmath.cpp:259-265): sqrt(3e) | a ln(12e-b)+c, times 1023
    const f2 lo = sqrt_2(e * splat(3.0f * 1023.0f * 1023.0f));
    const f2 hi = pk_fma(log2_2(pk_fma(e, splat(12.0f), splat(-UHDR_HLG_B))),
                         splat(UHDR_HLG_A * 0.693147180559945f * 1023.0f), splat(UHDR_HLG_C * 1023.0f));
    return sel_le(e, 1.0f / 12.0f, lo, hi);
  } else if (FMT == 2) {  // PQ (gainmapmath.cpp:309-312): ((c1 + c2 e^m1) / (1 + c3 e^m1))^m2, times 1023
    // e == 0: log2 -> -inf, e^m1 -> 0, result c1^m2 * 1023 = 7e-4, which truncates to the reference's 0
    const f2 p = exp2_2(log2_2(e) * splat(UHDR_PQ_M1));
    const f2 q = pk_fma(p, splat(UHDR_PQ_C2), splat(UHDR_PQ_C1)) * rcp_2(pk_fma(p, splat(UHDR_PQ_C3), splat(1.0f)));
    return exp2_2(pk_fma(log2_2(q), splat(UHDR_PQ_M2), splat(9.99859042974533f)));     // + log2(1023)
  } else if (FMT == 4) {
    return e * splat(1023.0f);
  }
  return e;
}

struct PairOut { f2 r, g, b; };

// inputs already *1023.  The reference's `& 0x3ff` (gainmapmath.cpp:723-725) can only bite when a channel
// reaches 1024, i.e. when max_display_boost < maxContentBoost lets values exceed 1.0; MASK is a per-call
// (wave-uniform) property, so the common case packs with two v_lshl_or_b32 and one v_or_b32.
template <bool MASK>
__device__ __forceinline__ uint32_t pack10_scaled(float r, float g, float b) {
  uint32_t ri = (uint32_t)r, gi = (uint32_t)g, bi = (uint32_t)b;
  if (MASK) { ri &= 0x3ffu; gi &= 0x3ffu; bi &= 0x3ffu; }
  uint32_t t;  // hipcc splits (g << 10) | r into a shift and an or; v_lshl_or_b32 does it in one slot
  asm("v_lshl_or_b32 %0, %1, 10, %2" : "=v"(t) : "v"(gi), "v"(ri));
  asm("v_lshl_or_b32 %0, %1, 20, %2" : "=v"(t) : "v"(bi), "v"(t));
  return t | 0xC0000000u;
}
// the same from three OETF-table results: red's bits are 0xC0000000 | code (alpha included); the shifts push the upper bits of
// green and blue out of the word
__device__ __forceinline__ uint32_t pack10_bits(float r, float g, float b) {
  uint32_t t;
  asm("v_lshl_or_b32 %0, %1, 10, %2" : "=v"(t) : "v"(__float_as_uint(g)), "v"(__float_as_uint(r)));
  asm("v_lshl_or_b32 %0, %1, 20, %2" : "=v"(t) : "v"(__float_as_uint(b)), "v"(t));
  return t;
}

// one float of byte k of a word: v_cvt_f32_ubyte<k>
template <int K>
__device__ __forceinline__ float cvt_byte(uint32_t w) { return (float)((w >> (8 * K)) & 0xffu); }

// One map cell (4x4 pixels) for HLG / PQ output through both tables, as a software pipeline over its 8 pixel pairs (two
// horizontally adjacent pixels share one chroma sample and run as one packed float2).  A pair needs two LDS round
// trips (stage 1, stage 2), and the compiler, left alone, waits for each pair of reads right after issuing it (a SIMD's four waves
// then spend 60 % of their time parked at s_waitcnt).  Here every iteration runs three stages of three different pairs,
//   F(k):   E, factor, r g b of pair k, their cells; issues the 6 stage-1 reads of pair k
//   M(k-1): the 6 fmas on the stage-1 entries of pair k-1, s = 2 + 2 T factor, the 6 slot addresses; issues its 6 stage-2 reads
//   B(k-2): the 6 fmas on the stage-2 entries of pair k-2, packs its two pixels (and stores the row when it is complete)
// so that every read has a whole iteration (~50 VALU instructions) between issue and use.  sched_barrier keeps the stages apart.
struct PairF { f2 c[3]; f2 factor; float2 e[6]; };
struct PairM { f2 s[3]; float2 e[6]; };
// the chroma terms of the BT.601 YUV->RGB of gainmapmath.cpp:184-202 for one row of two chroma samples, scaled like the luma
struct ChromaRow { f2 crv, ngs, cbu; };
__device__ __forceinline__ ChromaRow chroma_row(uint32_t uu, uint32_t vv) {
  constexpr float kCrS = kP3Cr * k255, kCbS = kP3Cb * k255, kGCbS = kP3GCb * k255, kGCrS = kP3GCr * k255;
  const f2 uf = (f2){cvt_byte<0>(uu), cvt_byte<1>(uu)};
  const f2 vf = (f2){cvt_byte<0>(vv), cvt_byte<1>(vv)};
  ChromaRow o;
  o.crv = pk_fma(vf, splat(kCrS), splat(-128.0f * kCrS));
  o.cbu = pk_fma(uf, splat(kCbS), splat(-128.0f * kCbS));
  o.ngs = pk_fma(uf, splat(-kGCbS), pk_fma(vf, splat(-kGCrS), splat(128.0f * kGCbS + 128.0f * kGCrS)));
  return o;
}
template <int FMT>
__device__ __forceinline__ void apply_cell_piped(const AppConsts& c, void* dst, uint32_t cx, uint32_t cy,
                                                 const uint32_t (&yrow)[4], const uint16_t (&uu)[2], const uint16_t (&vv)[2],
                                                 float m1, float m2, float m3, float m4, uint32_t slot8, const char* lut) {
  typedef ApplyTab<FMT, false> T;
  // only the chroma row in use is kept as floats (the second row's six values are formed when rows 2 and 3 start): the cell runs
  // at the register budget of four waves per SIMD
  ChromaRow cr = chroma_row(uu[0], vv[0]);
  const float a255 = c.fast.A255;
  // The four per-cell scalars of the exponent travel as two register PAIRS whose halves v_pk_fma_f32 broadcasts through op_sel: a
  // scalar splat by the compiler occupies a pair as well, with an undefined upper register -- which the allocator is free to
  // place on a register an outstanding load of the next cell will write, and the s_waitcnt in front of the fma then waits for
  // that load (seen in the ISA: one full trip to HBM per cell).
  f2 d23 = (f2){m2 - m1, m3 - m1}, d4b = (f2){m4 - m1, __builtin_fmaf(m1, a255, c.fast.B)};
  asm("" : "+v"(d23), "+v"(d4b));   // (opaque: or the pairs are taken apart again)
  PairF pf[2];
  PairM pm[2];
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    if (k < 8) {  // ---- F(k)
      const int oy = k >> 1, pr = k & 1;
      // sampleMap's standard weights (cells of the last column / row: apply_cell_edge) times A / 255: SGPR pairs
      const f2 w1 = (f2){c.fast.wD[oy][pr][0][0], c.fast.wD[oy][pr][0][1]}, w2 = (f2){c.fast.wD[oy][pr][1][0], c.fast.wD[oy][pr][1][1]};
      const f2 w3 = (f2){c.fast.wD[oy][pr][2][0], c.fast.wD[oy][pr][2][1]};
      if (k == 4) cr = chroma_row(uu[1], vv[1]);
      PairF& f = pf[k & 1];
      const f2 E = pk_fma(bc_lo(d4b), w3, pk_fma(bc_hi(d23), w2, pk_fma(bc_lo(d23), w1, bc_hi(d4b))));
      const f2 yraw = pr ? (f2){cvt_byte<2>(yrow[oy]), cvt_byte<3>(yrow[oy])} : (f2){cvt_byte<0>(yrow[oy]), cvt_byte<1>(yrow[oy])};
      if (pr) {
        f.c[0] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.crv); f.c[1] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.ngs);
        f.c[2] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.cbu);
      } else {
        f.c[0] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.crv); f.c[1] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.ngs);
        f.c[2] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.cbu);
      }
      f.factor = exp2_2(E);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pow_pair(f.c[ch], lut, f.e[2 * ch], f.e[2 * ch + 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1 && k <= 8) {  // ---- M(k-1)
      PairF& f = pf[(k - 1) & 1];
      PairM& m = pm[(k - 1) & 1];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        f2 t;
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.x) : "v"(f.e[2 * ch].y), "v"(f.c[ch].x), "v"(f.e[2 * ch].x));
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.y) : "v"(f.e[2 * ch + 1].y), "v"(f.c[ch].y), "v"(f.e[2 * ch + 1].x));
        m.s[ch] = pk_fma(t, f.factor, splat(2.0f));
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        m.e[2 * ch] = *reinterpret_cast<const float2*>(lut + T::kS2Base + s2_address(m.s[ch].x, slot8));
        m.e[2 * ch + 1] = *reinterpret_cast<const float2*>(lut + T::kS2Base + s2_address(m.s[ch].y, slot8));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 2) {  // ---- B(k-2)
      const int q = k - 2, oy = q >> 1, pr = q & 1;
      PairM& m = pm[q & 1];
      float o[6];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o[2 * ch]) : "v"(m.e[2 * ch].y), "v"(m.s[ch].x), "v"(m.e[2 * ch].x));
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o[2 * ch + 1]) : "v"(m.e[2 * ch + 1].y), "v"(m.s[ch].y), "v"(m.e[2 * ch + 1].x));
      }
      px[2 * pr] = pack10_bits(o[0], o[2], o[4]);
      px[2 * pr + 1] = pack10_bits(o[1], o[3], o[5]);
      if (pr) {
        const uint32_t off = ((4u * cy + oy) * c.width + 4u * cx) * 4u;  // (a 32-bit byte offset: app_fast_s4 keeps the image below 4 GiB)
        st_stream(reinterpret_cast<uint4*>(static_cast<char*>(dst) + off), make_uint4(px[0], px[1], px[2], px[3]));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The cell for the outputs without a stage-2 table (the two linear formats; HLG / PQ of a call whose values may exceed 1.0) in the
// same manner, two stages: F(k) as above on the g = 1 table, B(k-1) = the 6 fmas on its entries, the factor, the special-function
// OETF where there is one, the pack.
constexpr uint32_t kXchSecond = 72;    // in uint4: the second halves start 1152 bytes into the wave's exchange area ...
constexpr uint32_t kXchPerWave = 136;  // ... of 2176 bytes
template <int FMT, bool MASK>
__device__ __forceinline__ void apply_cell_piped1(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy,
                                                  const uint32_t (&yrow)[4], const uint16_t (&uu)[2], const uint16_t (&vv)[2],
                                                  float m1, float m2, float m3, float m4, const char* lut, uint4* xch,
                                                  bool via_xch /* wave-uniform: the branch on it must not mask lanes */) {
  ChromaRow cr = chroma_row(uu[0], vv[0]);
  const float a255 = c.fast.A255;
  // The four per-cell scalars of the exponent travel as two register PAIRS whose halves v_pk_fma_f32 broadcasts through op_sel: a
  // scalar splat by the compiler occupies a pair as well, with an undefined upper register -- which the allocator is free to
  // place on a register an outstanding load of the next cell will write, and the s_waitcnt in front of the fma then waits for
  // that load (seen in the ISA: one full trip to HBM per cell).
  f2 d23 = (f2){m2 - m1, m3 - m1}, d4b = (f2){m4 - m1, __builtin_fmaf(m1, a255, c.fast.B)};
  asm("" : "+v"(d23), "+v"(d4b));   // (opaque: or the pairs are taken apart again)
  PairF pf[2];
  PairOut po[2];
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    if (k < 8) {  // ---- F(k)
      const int oy = k >> 1, pr = k & 1;
      // sampleMap's standard weights (cells of the last column / row: apply_cell_edge) times A / 255: SGPR pairs
      const f2 w1 = (f2){c.fast.wD[oy][pr][0][0], c.fast.wD[oy][pr][0][1]}, w2 = (f2){c.fast.wD[oy][pr][1][0], c.fast.wD[oy][pr][1][1]};
      const f2 w3 = (f2){c.fast.wD[oy][pr][2][0], c.fast.wD[oy][pr][2][1]};
      if (k == 4) cr = chroma_row(uu[1], vv[1]);
      PairF& f = pf[k & 1];
      const f2 E = pk_fma(bc_lo(d4b), w3, pk_fma(bc_hi(d23), w2, pk_fma(bc_lo(d23), w1, bc_hi(d4b))));
      const f2 yraw = pr ? (f2){cvt_byte<2>(yrow[oy]), cvt_byte<3>(yrow[oy])} : (f2){cvt_byte<0>(yrow[oy]), cvt_byte<1>(yrow[oy])};
      if (pr) {
        f.c[0] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.crv); f.c[1] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.ngs);
        f.c[2] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.cbu);
      } else {
        f.c[0] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.crv); f.c[1] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.ngs);
        f.c[2] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.cbu);
      }
      f.factor = exp2_2(E);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) tab_pair<0>(f.c[ch], lut, f.e[2 * ch], f.e[2 * ch + 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 1) {  // ---- B(k-1)
      const int q = k - 1, oy = q >> 1, pr = q & 1;
      PairF& f = pf[q & 1];
      f2 lin[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        f2 t;
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.x) : "v"(f.e[2 * ch].y), "v"(f.c[ch].x), "v"(f.e[2 * ch].x));
        asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.y) : "v"(f.e[2 * ch + 1].y), "v"(f.c[ch].y), "v"(f.e[2 * ch + 1].x));
        lin[ch] = oetf2_scaled<FMT>(t * f.factor);
      }
      po[pr].r = lin[0]; po[pr].g = lin[1]; po[pr].b = lin[2];
      if (pr) {
        const uint32_t pix0 = (4u * cy + oy) * c.width + 4u * cx;  // < 2^27 pixels per image
        if (FMT == 2 || FMT == 3) {
          uint4 o;
          o.x = pack10_scaled<MASK>(po[0].r.x, po[0].g.x, po[0].b.x); o.y = pack10_scaled<MASK>(po[0].r.y, po[0].g.y, po[0].b.y);
          o.z = pack10_scaled<MASK>(po[1].r.x, po[1].g.x, po[1].b.x); o.w = pack10_scaled<MASK>(po[1].r.y, po[1].g.y, po[1].b.y);
          st_stream(reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + pix0), o);
        } else if (FMT == 1) {
          const uint2 a = pack_f16_hw(po[0].r.x, po[0].g.x, po[0].b.x), bb = pack_f16_hw(po[0].r.y, po[0].g.y, po[0].b.y);
          const uint2 cc = pack_f16_hw(po[1].r.x, po[1].g.x, po[1].b.x), d = pack_f16_hw(po[1].r.y, po[1].g.y, po[1].b.y);
          if (via_xch) {
            // A lane's row is 32 bytes: stored as it stands, every store instruction would fill half of each line it touches
            // (measured: 2.0 instead of 5.6 TB/s, scripts/ab/store_pattern).  The wave's 64 rows pass through LDS so that each of
            // the two instructions writes 1 KiB contiguous: lane L stores half (L & 1) of the row of lane L / 2 (then of lane
            // 32 + L / 2).  First halves at 16 L, second halves at 1152 + 16 L: no bank conflict either way.
            xch[lane] = make_uint4(a.x, a.y, bb.x, bb.y);
            xch[kXchSecond + lane] = make_uint4(cc.x, cc.y, d.x, d.y);
            __builtin_amdgcn_wave_barrier();
            const uint32_t from = (lane & 1u) * kXchSecond + (lane >> 1);
            const uint4 s0 = xch[from], s1 = xch[from + 32u];
            __builtin_amdgcn_wave_barrier();
            uint4* o = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + (uint32_t)__builtin_amdgcn_readfirstlane((int)pix0));
            st_stream(o + lane, s0);
            st_stream(o + 64u + lane, s1);
          } else {
            uint4* o = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + pix0);
            o[0] = make_uint4(a.x, a.y, bb.x, bb.y);
            o[1] = make_uint4(cc.x, cc.y, d.x, d.y);
          }
        } else {  // FMT == 4: planar R,G,B uint16 (ultrahdr.cpp:460-468)
          const size_t plane = (size_t)c.width * c.height;
          uint16_t* base16 = static_cast<uint16_t*>(im.dst);
          const f2 ch[3][2] = {{po[0].r, po[1].r}, {po[0].g, po[1].g}, {po[0].b, po[1].b}};
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            const uint32_t q0 = 0x3ffu & (uint32_t)ch[p][0].x, q1 = 0x3ffu & (uint32_t)ch[p][0].y;
            const uint32_t q2 = 0x3ffu & (uint32_t)ch[p][1].x, q3 = 0x3ffu & (uint32_t)ch[p][1].y;
            st_stream(reinterpret_cast<uint2*>(base16 + p * plane + pix0), make_uint2(q0 | (q1 << 16), q2 | (q3 << 16)));
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the bytes of one map cell's 4x4 pixels: four luma words, two rows of two chroma samples per plane, the four sampleMap taps
// (gainmapmath.cpp:690-703: the reference indexes the map with map->width).  The taps stay bytes: the / 255 of gainmapmath.cpp:632
// is folded into the weights.  32-bit offsets (an image plane is < 4 GiB): one 64-bit add per address.
struct ApplyCellIn { uint32_t yrow[4], uu[2], vv[2], mb[4]; };
__device__ __forceinline__ void apply_load_cell(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, ApplyCellIn& o) {
  const uint32_t yoff = 4u * cy * im.y_stride + 4u * cx;
#pragma unroll
  for (int r = 0; r < 4; ++r) o.yrow[r] = ld_stream(reinterpret_cast<const uint32_t*>(im.y + (yoff + r * im.y_stride)));
  const uint32_t coff = 2u * cy * im.c_stride + 2u * cx;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    o.uu[r] = *reinterpret_cast<const uint16_t*>(im.u + (coff + r * im.c_stride));
    o.vv[r] = *reinterpret_cast<const uint16_t*>(im.v + (coff + r * im.c_stride));
  }
  const uint32_t xu = min(cx + 1u, c.map_w - 1u), yu = min(cy + 1u, c.map_h - 1u);
  const uint32_t m0 = cy * c.map_w, m1 = yu * c.map_w;
  o.mb[0] = im.map[m0 + cx]; o.mb[1] = im.map[m1 + cx]; o.mb[2] = im.map[m0 + xu]; o.mb[3] = im.map[m1 + xu];
}

// A cell with per-lane weights (the last column / row of the map: the NR / NB / C tables of gainmapmath.h:184-228): the arithmetic
// of the walk's cells, row by row in a rolled loop, a row's two pixel pairs side by side.  Some 1500 cells of a 4K frame take this
// path, in the waves of the walk that touch the last column / row.  It is short and needs few registers -- a second copy of the
// pipelined cell with per-lane weights, inlined next to the first, made the allocator spill in the loop they share -- and nothing
// in it is pipelined.
template <int FMT, bool MASK>
__device__ __forceinline__ void apply_cell_edge(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy,
                                                const uint32_t (&yrow)[4], const uint16_t (&uu)[2], const uint16_t (&vv)[2],
                                                float m1, float m2, float m3, float m4, const float* wt /* the lane's table, in LDS */,
                                                uint32_t slot8, const char* lut) {
  typedef ApplyTab<FMT, MASK> T;
  const float a255 = c.fast.A255;
  const float base = __builtin_fmaf(m1, a255, c.fast.B), d2 = m2 - m1, d3 = m3 - m1, d4 = m4 - m1;
  // The loop leaves the cell's rows in registers (its inputs are dead by then) and the stores follow it in straight-line code: a
  // store inside the rolled loop is one the compiler cannot count at the loop's exit, and every wait behind it drained them all.
  // A finished row enters at the top of the window and has moved down to its own place after the fourth.
  constexpr int kW = FMT == 4 ? 3 : FMT == 1 ? 2 : 1;   // 16-byte (FMT 4: 8-byte) pieces per row
  uint4 rows[4][kW];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < kW; ++q) rows[r][q] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
  for (uint32_t oy = 0; oy < 4u; ++oy) {   // (uniform: the selects below are scalar)
    const uint32_t yw = oy == 0u ? yrow[0] : oy == 1u ? yrow[1] : oy == 2u ? yrow[2] : yrow[3];
    const ChromaRow cr = chroma_row(oy < 2u ? uu[0] : uu[1], oy < 2u ? vv[0] : vv[1]);
    uint32_t px[4];
    uint4 row[kW];
    PairOut po[2];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const f2 yraw = pr ? (f2){cvt_byte<2>(yw), cvt_byte<3>(yw)} : (f2){cvt_byte<0>(yw), cvt_byte<1>(yw)};
      const float* p0 = wt + oy * 16u + pr * 8;
      const f2 w1 = (f2){p0[1], p0[5]}, w2 = (f2){p0[2], p0[6]}, w3 = (f2){p0[3], p0[7]};   // (times A / 255 already: the kernel's prologue)
      const f2 E = pk_fma(splat(d4), w3, pk_fma(splat(d3), w2, pk_fma(splat(d2), w1, splat(base))));
      const f2 factor = exp2_2(E);
      f2 ch[3];
      if (pr) {
        ch[0] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.crv); ch[1] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.ngs); ch[2] = pk_fma_sat_bc<1>(yraw, splat(k255), cr.cbu);
      } else {
        ch[0] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.crv); ch[1] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.ngs); ch[2] = pk_fma_sat_bc<0>(yraw, splat(k255), cr.cbu);
      }
      if (T::kOetf) {
        float o[6];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          float2 a, b;
          pow_pair(ch[q], lut, a, b);
          f2 t;
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.x) : "v"(a.y), "v"(ch[q].x), "v"(a.x));
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.y) : "v"(b.y), "v"(ch[q].y), "v"(b.x));
          const f2 s = pk_fma(t, factor, splat(2.0f));
          const float2 ea = *reinterpret_cast<const float2*>(lut + T::kS2Base + s2_address(s.x, slot8));
          const float2 eb = *reinterpret_cast<const float2*>(lut + T::kS2Base + s2_address(s.y, slot8));
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o[2 * q]) : "v"(ea.y), "v"(s.x), "v"(ea.x));
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(o[2 * q + 1]) : "v"(eb.y), "v"(s.y), "v"(eb.x));
        }
        px[2 * pr] = pack10_bits(o[0], o[2], o[4]);
        px[2 * pr + 1] = pack10_bits(o[1], o[3], o[5]);
      } else {
        f2 lin[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          float2 a, b;
          tab_pair<0>(ch[q], lut, a, b);
          f2 t;
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.x) : "v"(a.y), "v"(ch[q].x), "v"(a.x));
          asm("v_fma_f32 %0, %1, %2, %3" : "=v"(t.y) : "v"(b.y), "v"(ch[q].y), "v"(b.x));
          lin[q] = oetf2_scaled<FMT>(t * factor);
        }
        po[pr].r = lin[0]; po[pr].g = lin[1]; po[pr].b = lin[2];
      }
    }
    if (T::kOetf) {
      row[0] = make_uint4(px[0], px[1], px[2], px[3]);
    } else if (FMT == 2 || FMT == 3) {
      row[0].x = pack10_scaled<MASK>(po[0].r.x, po[0].g.x, po[0].b.x); row[0].y = pack10_scaled<MASK>(po[0].r.y, po[0].g.y, po[0].b.y);
      row[0].z = pack10_scaled<MASK>(po[1].r.x, po[1].g.x, po[1].b.x); row[0].w = pack10_scaled<MASK>(po[1].r.y, po[1].g.y, po[1].b.y);
    } else if (FMT == 1) {
      const uint2 a = pack_f16_hw(po[0].r.x, po[0].g.x, po[0].b.x), bb = pack_f16_hw(po[0].r.y, po[0].g.y, po[0].b.y);
      const uint2 cc = pack_f16_hw(po[1].r.x, po[1].g.x, po[1].b.x), d = pack_f16_hw(po[1].r.y, po[1].g.y, po[1].b.y);
      row[0] = make_uint4(a.x, a.y, bb.x, bb.y);
      row[kW - 1] = make_uint4(cc.x, cc.y, d.x, d.y);
    } else {  // FMT == 4: planar R,G,B uint16 (ultrahdr.cpp:460-468)
      const f2 pl[3][2] = {{po[0].r, po[1].r}, {po[0].g, po[1].g}, {po[0].b, po[1].b}};
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint32_t q0 = 0x3ffu & (uint32_t)pl[p][0].x, q1 = 0x3ffu & (uint32_t)pl[p][0].y;
        const uint32_t q2 = 0x3ffu & (uint32_t)pl[p][1].x, q3 = 0x3ffu & (uint32_t)pl[p][1].y;
        row[p % kW] = make_uint4(q0 | (q1 << 16), q2 | (q3 << 16), 0u, 0u);
      }
    }
#pragma unroll
    for (int q = 0; q < kW; ++q) { rows[0][q] = rows[1][q]; rows[1][q] = rows[2][q]; rows[2][q] = rows[3][q]; rows[3][q] = row[q]; }
  }
  // the same stores as the pipelined forms issue: a 32-bit byte offset on the image's base (app_fast_s4 keeps the image below 4 GiB)
  char* const dst = static_cast<char*>(im.dst);
  const uint32_t pix0 = 4u * cy * c.width + 4u * cx;  // < 2^27 pixels per image
#pragma unroll
  for (uint32_t oy = 0; oy < 4u; ++oy) {
    const uint32_t pix = pix0 + oy * c.width;
    if (FMT == 2 || FMT == 3) {
      st_stream(reinterpret_cast<uint4*>(dst + pix * 4u), rows[oy][0]);
    } else if (FMT == 1) {
      uint4* o = reinterpret_cast<uint4*>(dst + pix * 8u);
      o[0] = rows[oy][0];
      o[1] = rows[oy][kW - 1];
    } else {
      const uint32_t plane2 = c.width * c.height * 2u;
#pragma unroll
      for (int p = 0; p < 3; ++p)
        st_stream(reinterpret_cast<uint2*>(dst + (p * plane2 + pix * 2u)), make_uint2(rows[oy][p % kW].x, rows[oy][p % kW].y));
    }
  }
}

// The same bytes as the walk of k_apply_s4 keeps them across a cell (the next cell's are in flight while the current one is
// computed, so every dword counts against the 128 registers of four waves per SIMD): the two taps of a map row arrive as ONE
// 16-bit load, mrow[j] = the bytes (mx, mx + 1) of map row cy (j = 0) / cy1 (j = 1).  The loads are unaligned half the time; global
// memory takes that.  Needs map_w >= 2 (launch_apply_t).
// The 16-bit words stay 16-bit values: as dwords the compiler widened the set that travels round the loop's back edge there, six
// v_and behind six waits, although every use reads bytes 0 and 1 only.
struct ApplyCellPk { uint32_t yrow[4]; uint16_t uu[2], vv[2], mrow[2]; };
struct __attribute__((packed)) U16Any { uint16_t v; };
// (mx < map_w - 1: the column of the byte pairs; cy1: the row of the lower taps)
__device__ __forceinline__ void apply_load_cell_pk(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, uint32_t mx, uint32_t cy1, ApplyCellPk& o) {
  const uint32_t yoff = 4u * cy * im.y_stride + 4u * cx;
#pragma unroll
  for (int r = 0; r < 4; ++r) o.yrow[r] = ld_stream(reinterpret_cast<const uint32_t*>(im.y + (yoff + r * im.y_stride)));
  const uint32_t coff = 2u * cy * im.c_stride + 2u * cx;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    o.uu[r] = *reinterpret_cast<const uint16_t*>(im.u + (coff + r * im.c_stride));
    o.vv[r] = *reinterpret_cast<const uint16_t*>(im.v + (coff + r * im.c_stride));
  }
  o.mrow[0] = reinterpret_cast<const U16Any*>(im.map + (cy * c.map_w + mx))->v;
  o.mrow[1] = reinterpret_cast<const U16Any*>(im.map + (cy1 * c.map_w + mx))->v;
}

// Each block copies its tables into LDS once (4 KiB + 32 KiB for the replicated stage-2 table of HLG / PQ output, 15 KiB for the
// other outputs, 1 KiB of sampleMap weights: two blocks of 512 threads per CU) and then walks c.cells_per_thread map cells per
// thread.  Consecutive blocks belong to different images, as in generate (grid.x = image): the images of a launch progress
// together and the blocks in flight spread over the whole batch's memory (same-box A/B, round 2: 0.608 -> 0.576 ms per 64 frames).
//
// The walk is ONE straight line of code per cell: no memory instruction sits behind a branch (the request for the next cell is
// issued even when there is none -- it repeats the current cell's --, no lane is masked, and where a wave chooses between the two
// forms of the cell both issue the same memory instructions).  That is what lets s_waitcnt count: behind a branch the compiler
// has to assume an instruction was not issued, and a wait for the inputs of the next cell then also waits for every store issued
// after them -- round 2's loop drained its stores at every cell, reloaded six spilled registers, and waited for loads of the NEXT
// cell through registers the allocator had placed under undefined halves of operand pairs (apply_cell_piped).  Same box, 64 x 4K:
// 0.579 -> 0.536 ms.
//
// The cells of the last column and row have per-lane weights (the NR / NB / C tables of gainmapmath.h:184-228): a wave that
// touches one (one in fifteen on a 4K frame) runs apply_cell_edge for its 64 cells instead of the pipelined form.  Measured and
// dropped: handing those cells to blocks of their own behind a walk on SGPR weights only (a lane on the last column recomputing
// its left neighbour): 2 % slower on 64 x 4K (0.604 against 0.594 ms, same box), and in a one-round launch the handful of
// latency-bound edge blocks is what the launch waits for (one 4K frame: 13 -> 17-23 us).
constexpr uint32_t kApplyBlock = 512;
constexpr uint32_t kApplyMaxCellsPerThread = 32;   // (64 x 4K, same box: 32 cells per thread 0.594 ms, 64: 0.598, 128: 0.607; 48 / 80 / 96: 0.63-0.65)

// One cell of the walk: requests the inputs of the thread's next cell into `nxt` (a block's waves start together, and without this
// they would also all wait for HBM together and all compute together), computes the cell whose inputs `cur` holds, and steps
// (cx, cy) on.  The kernel calls it with its two register sets swapped from cell to cell, so nothing is copied between them.
// Returns whether there is a next cell; when there is none the request repeats the current cell's (issued all the same: see above).
template <int FMT, bool MASK>
__device__ __forceinline__ bool apply_walk_cell(const AppConsts& c, const AppImage& im, uint32_t& cx, uint32_t& cy, uint32_t& left,
                                                const ApplyCellPk& cur, ApplyCellPk& nxt, uint32_t slot8, const char* lut,
                                                const float* s_idw, uint4* s_xch) {
  typedef ApplyTab<FMT, MASK> T;
  // the block's next stretch of cells lies kApplyBlock = step_y * map_w + step_x cells further on
  uint32_t ncx = cx + c.step_x, ncy = cy + c.step_y;
  if (ncx >= c.map_w) { ncx -= c.map_w; ++ncy; }
  --left;
  // The wave goes on while any of its lanes has a next cell; a lane without one stays where it is and computes its cell again,
  // storing the same bytes to the same addresses (only in the ragged wave at an image's end).  So no lane is ever masked in the
  // loop and the compiler has one path, with one sequence of memory instructions, to count along.
  const bool mine = left != 0u && ncy < c.map_h;
  const bool more = __builtin_amdgcn_ballot_w64(mine) != 0ull;
  if (!mine) { ncx = cx; ncy = cy; }
  // In the last column sampleMap's right tap IS the left one (gainmapmath.cpp:690-703, xu == xl): the two bytes are loaded one
  // column to the left, the right tap is byte 1 either way, the left tap byte 0 -- or byte 1 in the last column.
  apply_load_cell_pk(c, im, ncx, ncy, ncx - (ncx + 1u == c.map_w ? 1u : 0u), min(ncy + 1u, c.map_h - 1u), nxt);
  const bool edge_x = cx + 1u == c.map_w, edge_y = cy + 1u == c.map_h;
  const float e3 = cvt_byte<1>(cur.mrow[0]), e4 = cvt_byte<1>(cur.mrow[1]);
  const float e1 = edge_x ? e3 : cvt_byte<0>(cur.mrow[0]), e2 = edge_x ? e4 : cvt_byte<0>(cur.mrow[1]);
  // all waves but those touching the last column / row take the pipelined form on SGPR weights
  const bool interior = __builtin_amdgcn_ballot_w64(edge_x || edge_y) == 0ull;
  const float* wt = s_idw + (edge_x ? (edge_y ? 192 : 64) : (edge_y ? 128 : 0));   // tables: 0 std, 1 no-right, 2 no-bottom, 3 corner
  if (T::kOetf) {
    if (interior) apply_cell_piped<FMT>(c, im.dst, cx, cy, cur.yrow, cur.uu, cur.vv, e1, e2, e3, e4, slot8, lut);
    else apply_cell_edge<FMT, MASK>(c, im, cx, cy, cur.yrow, cur.uu, cur.vv, e1, e2, e3, e4, wt, slot8, lut);
  } else {
    // F16: a full wave on 64 consecutive cells of one row stores through the exchange area (apply_cell_piped1); lanes that repeat
    // their cell beside lanes that went on break the sequence of columns, also where all of them are on the last row
    uint4* const xch = s_xch + (FMT == 1 ? (threadIdx.x >> 6) * kXchPerWave : 0u);
    const bool via_xch = FMT == 1 && __builtin_amdgcn_ballot_w64(true) == ~0ull &&
        __builtin_amdgcn_ballot_w64(cy != (uint32_t)__builtin_amdgcn_readfirstlane((int)cy) ||
                                    cx != (uint32_t)__builtin_amdgcn_readfirstlane((int)cx) + (threadIdx.x & 63u)) == 0ull;
    if (interior) apply_cell_piped1<FMT, MASK>(c, im, cx, cy, cur.yrow, cur.uu, cur.vv, e1, e2, e3, e4, lut, xch, via_xch);
    else apply_cell_edge<FMT, MASK>(c, im, cx, cy, cur.yrow, cur.uu, cur.vv, e1, e2, e3, e4, wt, slot8, lut);
  }
  cx = ncx; cy = ncy;
  return more;
}

template <int FMT, bool MASK>
__global__ void __launch_bounds__(kApplyBlock, 4) k_apply_s4(const AppConsts c, const AppBatch b) {
  typedef ApplyTab<FMT, MASK> T;
  __shared__ uint4 s_tab[T::kBytes / 16u];
  __shared__ uint4 s_xch[FMT == 1 ? (kApplyBlock / 64) * kXchPerWave : 1];   // F16: the waves' exchange areas
  __shared__ float s_idw[4 * 64];   // sampleMap's four weight tables times A / 255: per-lane weights are an LDS read, not a trip to L2 per pixel pair
  const uint32_t img_i = blockIdx.x, span = blockIdx.y;
  const AppImage& im = b.img[img_i];
  const uint32_t idx = span * c.cells_per_thread * kApplyBlock + threadIdx.x;
  uint32_t cy = idx / c.map_w;
  uint32_t cx = idx - cy * c.map_w;
  const bool any = cy < c.map_h;
  // the first cell's pixels are requested before the tables: both trips to memory overlap
  ApplyCellPk ca, cb;
  if (any) apply_load_cell_pk(c, im, cx, cy, cx - (cx + 1u == c.map_w ? 1u : 0u), min(cy + 1u, c.map_h - 1u), ca);
  {
    // all loads first, then all stores: one trip through L2's latency per block instead of one per piece
    constexpr uint32_t kN1 = T::kS1Bytes / 16u, kPer1 = (kN1 + kApplyBlock - 1u) / kApplyBlock;
    constexpr uint32_t kN2 = T::kOetf ? kTabS2Cells * 32u : 0u, kPer2 = (kN2 + kApplyBlock - 1u) / kApplyBlock;
    const uint4* src1 = reinterpret_cast<const uint4*>(c.tab + T::kS1Float);
    const uint2* src2 = reinterpret_cast<const uint2*>(c.tab + T::kS2Float);
    uint4 t1[kPer1];
    uint2 t2[kPer2 ? kPer2 : 1u];
    const float w = c_idw4[threadIdx.x & 255u] * c.fast.A255;   // (before the rounding mode changes: launch_apply_t's product)
#pragma unroll
    for (uint32_t k = 0; k < kPer1; ++k) { const uint32_t i = k * kApplyBlock + threadIdx.x; t1[k] = src1[i < kN1 ? i : kN1 - 1u]; }
#pragma unroll
    for (uint32_t k = 0; k < kPer2; ++k) { const uint32_t i = k * kApplyBlock + threadIdx.x; t2[k] = src2[(i < kN2 ? i : 0u) >> 5]; }
    if (threadIdx.x < 256u) s_idw[threadIdx.x] = w;
#pragma unroll
    for (uint32_t k = 0; k < kPer1; ++k) { const uint32_t i = k * kApplyBlock + threadIdx.x; if (i < kN1) s_tab[i] = t1[k]; }
#pragma unroll
    for (uint32_t k = 0; k < kPer2; ++k) { const uint32_t i = k * kApplyBlock + threadIdx.x; if (i < kN2) reinterpret_cast<uint2*>(s_tab)[T::kS2Base / 8u + i] = t2[k]; }
    // The last pieces are stored by some lanes only, and behind such a branch the compiler counts their loads as still in flight:
    // into the walk's loop, where every write to one of these registers then waited for stores (seen in the ISA: vmcnt(11) and
    // vmcnt(10) in the first cell of each pair).  An unconditional use ends that here.
#pragma unroll
    for (uint32_t k = 0; k < kPer1; ++k) asm volatile("" :: "v"(t1[k].w));
#pragma unroll
    for (uint32_t k = 0; k < kPer2; ++k) asm volatile("" :: "v"(t2[k].y));
  }
  __syncthreads();
  const char* lut = reinterpret_cast<const char*>(s_tab);
  const uint32_t slot8 = (threadIdx.x & 31u) << 3;
  if (!any) return;
  if (T::kOetf) {
    // Round toward zero from here on: stage 2 truncates the code inside its fma.  The integer division above is expanded into
    // float operations that assume round-to-nearest, hence the (fake) dependence of its results on this statement; the cells that
    // follow are reached by addition.
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3" : "+v"(cx), "+v"(cy));
  }
  uint32_t left = c.cells_per_thread;
#pragma unroll 1
  for (;;) {
    if (!apply_walk_cell<FMT, MASK>(c, im, cx, cy, left, ca, cb, slot8, lut, s_idw, s_xch)) return;
    if (!apply_walk_cell<FMT, MASK>(c, im, cx, cy, left, cb, ca, slot8, lut, s_idw, s_xch)) return;
  }
}

// General path: one thread per pixel; any integer scale, any pointer/stride alignment, FAST or
// EXACT arithmetic.  Mirrors ultrahdr.cpp:427-496 + gainmapmath.cpp:686-720 literally.
struct PxIn { float yf, u, v, gain; };
// (PxTaps, px_taps, px_grid and px_store: uhdr_apply_px.h)
// the loads of ultrahdr.cpp:431-438 and sampleMap for pixel (x, y)
__device__ __forceinline__ PxIn px_inputs(const AppConsts& c, const AppImage& im, uint32_t x, uint32_t y) {
  PxIn in;
  in.yf = (float)im.y[(size_t)y * im.y_stride + x] * k255;
  const size_t ci = (size_t)(y >> im.csy) * im.c_stride + (x >> im.csx);   // 4:2:0: (x >> 1, y >> 1), as getYuv420Pixel
  in.u = (float)((int)im.u[ci] - 128) * k255;
  in.v = (float)((int)im.v[ci] - 128) * k255;
  const PxTaps t = px_taps(c, x, y);
  // (byte / 255.0f through the constant division that is proven equal for all 256 bytes, tests/test_gpu_transfer_exhaustive.py)
  const float e1 = map_to_float_fast(im.map[(size_t)t.yl * c.map_w + t.xl]);
  const float e2 = map_to_float_fast(im.map[(size_t)t.yu * c.map_w + t.xl]);
  const float e3 = map_to_float_fast(im.map[(size_t)t.yl * c.map_w + t.xu]);
  const float e4 = map_to_float_fast(im.map[(size_t)t.yu * c.map_w + t.xu]);
  in.gain = e1 * t.w[0] + e2 * t.w[1] + e3 * t.w[2] + e4 * t.w[3];
  return in;
}

template <int FMT, bool EXACT>
__global__ void __launch_bounds__(256) k_apply_px(const AppConsts c, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.z];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= c.width) return;
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {
    const PxIn in = px_inputs(c, im, x, y);
    const F3 lin = recover_hdr<EXACT>(c, in.yf, kP3Cr * in.v, kP3GCb * in.u, kP3GCr * in.v, kP3Cb * in.u, in.gain);
    px_store<FMT>(im, (size_t)y * c.width + x, total, hdr_oetf<FMT, EXACT>(lin));
  }
}

// ---- per-channel (RGB) gain maps -----------------------------------------------------------------------
// The map is interleaved R, G, B, A bytes (AppImage::map 4-byte aligned, rows AppConsts::map_stride pixels apart): one dword load per
// tap holds its three gains.  sampleMap's taps and weights are the pixel's (px_taps), applied to each channel of the taps; applyGain
// runs per channel.  Every operation behind the gain is per channel, so channel c of a pixel is, bit for bit, channel c of
// k_apply_px<FMT, EXACT> run with plane c of the map.
template <bool EXACT>
__device__ __forceinline__ F3 recover_hdr_rgb(const AppConsts& c, float yf, float crv, float gcbu, float gcrv, float cbu,
                                              const float (&gain)[3]) {
  float ch[3] = {clamp01(yf + crv), clamp01(yf - gcbu - gcrv), clamp01(yf + cbu)};
  float o[3];
  if (EXACT) srgb_inv_oetf_guarded_n<3>(ch);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float log_boost = (float)(c.log2_min_d * (double)(1.0f - gain[k]) + c.log2_max_d * (double)gain[k]);
    if (EXACT) {
      const float factor = exp2_to_float_guarded(log_boost * c.display_boost / c.max_boost);
      o[k] = (ch[k] * factor) / c.display_boost;
    } else {
      const float factor = __builtin_amdgcn_exp2f((log_boost * c.display_boost) * c.inv_max_boost);
      o[k] = (srgb_inv_oetf_fast(ch[k]) * factor) * c.inv_display_boost;
    }
  }
  F3 r;
  r.x = o[0]; r.y = o[1]; r.z = o[2];
  return r;
}
template <int FMT, bool EXACT>
__global__ void __launch_bounds__(256) k_apply_px_rgb(const AppConsts c, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.z];
  const uint32_t* map = reinterpret_cast<const uint32_t*>(im.map);
  const size_t total = (size_t)c.width * c.height;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= c.width) return;
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {
    const float yf = (float)im.y[(size_t)y * im.y_stride + x] * k255;
    const size_t ci = (size_t)(y >> im.csy) * im.c_stride + (x >> im.csx);
    const float u = (float)((int)im.u[ci] - 128) * k255, v = (float)((int)im.v[ci] - 128) * k255;
    const PxTaps t = px_taps(c, x, y);
    const uint32_t m1 = map[(size_t)t.yl * c.map_stride + t.xl], m2 = map[(size_t)t.yu * c.map_stride + t.xl];
    const uint32_t m3 = map[(size_t)t.yl * c.map_stride + t.xu], m4 = map[(size_t)t.yu * c.map_stride + t.xu];
    const float w0 = t.w[0], w1 = t.w[1], w2 = t.w[2], w3 = t.w[3];
    float gain[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      gain[k] = map_to_float_fast((m1 >> (8 * k)) & 0xffu) * w0 + map_to_float_fast((m2 >> (8 * k)) & 0xffu) * w1 +
                map_to_float_fast((m3 >> (8 * k)) & 0xffu) * w2 + map_to_float_fast((m4 >> (8 * k)) & 0xffu) * w3;
    const F3 lin = recover_hdr_rgb<EXACT>(c, yf, kP3Cr * v, kP3GCb * u, kP3GCr * v, kP3Cb * u, gain);
    px_store<FMT>(im, (size_t)y * c.width + x, total, hdr_oetf<FMT, EXACT>(lin));
  }
}
template <int FMT>
static hipError_t launch_apply_rgb_t(const AppConsts& c, const AppBatch& b, int n, bool exact, hipStream_t s) {
  if (n == 0 || c.width == 0 || c.height == 0) return hipSuccess;
  const dim3 grid = px_grid(c.width, c.height, n);
  if (exact) hipLaunchKernelGGL((k_apply_px_rgb<FMT, true>), grid, dim3(256), 0, s, c, b);
  else hipLaunchKernelGGL((k_apply_px_rgb<FMT, false>), grid, dim3(256), 0, s, c, b);
  return hipGetLastError();
}
hipError_t launch_apply_rgb(const AppConsts& c, const AppBatch& b, int n, int fmt, bool exact, hipStream_t s) {
  switch (fmt) {
    case 1: return launch_apply_rgb_t<1>(c, b, n, exact, s);
    case 2: return launch_apply_rgb_t<2>(c, b, n, exact, s);
    case 3: return launch_apply_rgb_t<3>(c, b, n, exact, s);
    case 4: return launch_apply_rgb_t<4>(c, b, n, exact, s);
    default: return hipErrorInvalidValue;
  }
}

// ---- general gain-map metadata: gamma, offsets, HDR capacity -----------------------------------------------
// The per-pixel kernels' loop, loads and sampleMap (px_inputs / px_taps; the RGBA map as k_apply_px_rgb reads it), then
//   g' = g^(1/gamma)                                           (GAMMA only: one v_log_f32 / v_exp_f32 pair per gain; 0 stays 0)
//   out = max(0, (e + offsetSdr) * 2^(A g' + B) - offsetHdr / d)
// with e the FAST sRGB EOTF's value and A, B, offsetHdr / d the host's (AppMdConsts).  One f32 arithmetic: there is no reference
// path for such metadata that an EXACT form could reproduce.
// (md_factor: uhdr_apply_px.h)
__device__ __forceinline__ float md_channel(const AppMdConsts& m, float e, float factor) {
  return fmaxf(__builtin_fmaf(srgb_inv_oetf_fast(e) + m.off_sdr, factor, -m.off_hdr_d), 0.0f);
}
template <int FMT, bool RGB, bool GAMMA>
__global__ void __launch_bounds__(256) k_apply_px_md(const AppConsts c, const AppMdConsts m, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.z];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= c.width) return;
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {
    float yf, u, v, f[3];
    if (RGB) {
      const uint32_t* map = reinterpret_cast<const uint32_t*>(im.map);
      yf = (float)im.y[(size_t)y * im.y_stride + x] * k255;
      const size_t ci = (size_t)(y >> im.csy) * im.c_stride + (x >> im.csx);
      u = (float)((int)im.u[ci] - 128) * k255; v = (float)((int)im.v[ci] - 128) * k255;
      const PxTaps t = px_taps(c, x, y);
      const uint32_t m1 = map[(size_t)t.yl * c.map_stride + t.xl], m2 = map[(size_t)t.yu * c.map_stride + t.xl];
      const uint32_t m3 = map[(size_t)t.yl * c.map_stride + t.xu], m4 = map[(size_t)t.yu * c.map_stride + t.xu];
      const float w0 = t.w[0], w1 = t.w[1], w2 = t.w[2], w3 = t.w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        f[k] = md_factor<GAMMA>(m, map_to_float_fast((m1 >> (8 * k)) & 0xffu) * w0 + map_to_float_fast((m2 >> (8 * k)) & 0xffu) * w1 +
                                      map_to_float_fast((m3 >> (8 * k)) & 0xffu) * w2 + map_to_float_fast((m4 >> (8 * k)) & 0xffu) * w3);
    } else {
      const PxIn in = px_inputs(c, im, x, y);
      yf = in.yf; u = in.u; v = in.v;
      f[0] = f[1] = f[2] = md_factor<GAMMA>(m, in.gain);
    }
    F3 lin;
    lin.x = md_channel(m, clamp01(yf + kP3Cr * v), f[0]);
    lin.y = md_channel(m, clamp01(yf - kP3GCb * u - kP3GCr * v), f[1]);
    lin.z = md_channel(m, clamp01(yf + kP3Cb * u), f[2]);
    px_store<FMT>(im, (size_t)y * c.width + x, total, hdr_oetf<FMT, false>(lin));
  }
}
template <int FMT, bool RGB>
static hipError_t launch_apply_md_t(const AppConsts& c, const AppMdConsts& m, const AppBatch& b, int n, hipStream_t s) {
  if (n == 0 || c.width == 0 || c.height == 0) return hipSuccess;
  const dim3 grid = px_grid(c.width, c.height, n);
  if (m.gamma_on != 0u) hipLaunchKernelGGL((k_apply_px_md<FMT, RGB, true>), grid, dim3(256), 0, s, c, m, b);
  else hipLaunchKernelGGL((k_apply_px_md<FMT, RGB, false>), grid, dim3(256), 0, s, c, m, b);
  return hipGetLastError();
}
hipError_t launch_apply_md(const AppConsts& c, const AppMdConsts& m, const AppBatch& b, int n, int fmt, bool rgb, hipStream_t s) {
  switch (fmt) {
    case 1: return rgb ? launch_apply_md_t<1, true>(c, m, b, n, s) : launch_apply_md_t<1, false>(c, m, b, n, s);
    case 2: return rgb ? launch_apply_md_t<2, true>(c, m, b, n, s) : launch_apply_md_t<2, false>(c, m, b, n, s);
    case 3: return rgb ? launch_apply_md_t<3, true>(c, m, b, n, s) : launch_apply_md_t<3, false>(c, m, b, n, s);
    case 4: return rgb ? launch_apply_md_t<4, true>(c, m, b, n, s) : launch_apply_md_t<4, false>(c, m, b, n, s);
    default: return hipErrorInvalidValue;
  }
}

// ---- EXACT mode behind an f32 pre-filter (HLG, F16 and planar 10-bit outputs) ----------------------------------------------------
// The bit-exact pixel costs ~40 f64 operations per channel; what it decides in the end is an integer code (or a half-precision
// pattern).  k_apply_px_est evaluates the pixel on the f32 units -- the front end up to the exponent's argument exactly as the
// reference rounds it, then v_exp_f32 / v_log_f32 forms whose distance from the exact functions is measured for every float
// (tests/test_gpu_exact_filter.py) -- and writes that result.  A channel is IN DOUBT when the interval the exact value must lie in
// straddles a code boundary; pixels with such a channel (~1 %) go to per-image lists and k_apply_resolve recomputes exactly them
// with the exact path and overwrites.  Error budget, in the reference's own quantities:
//   lin = (srgbInvOetf(c) * factor) / displayBoost: relative error of the estimate <= kEstRel (srgb_inv_oetf_fast 6e-7, v_exp_f32
//     2e-7, the two roundings are the reference's own), so the 10-bit planar code floor(lin * 1023) and the half-precision pattern are
//     settled when both ends of lin (1 +- kEstRel) give the same;
//   hlgOetf: x h'(x) <= 1/4, so the input's error moves the code value by <= 1023 / 4 * kEstRel = 4e-4; hlg_oetf_fast itself is
//     within 3e-7 (3e-4 codes) of the exact function up to 1 and within 3e-7 relative above: doubt when
//     floor(v - d) != floor(v + d), d = kEstOetfAbs + v * kEstOetfRel;
//   pqOetf: v S(x) <= 112 codes per unit of relative input error (2.2e-4), pq_oetf_est is within 2.5e-4 codes: the same d.
constexpr float kEstRel = 2.0e-6f;
constexpr float kEstOetfAbs = 8.0e-4f, kEstOetfRel = 6.0e-7f;

__device__ __forceinline__ F3 recover_hdr_est(const AppConsts& c, float yf, float crv, float gcbu, float gcrv, float cbu, float gain) {
  const float r = clamp01(yf + crv), g = clamp01(yf - gcbu - gcrv), b = clamp01(yf + cbu);
  const float log_boost = (float)(c.log2_min_d * (double)(1.0f - gain) + c.log2_max_d * (double)gain);
  const float factor = __builtin_amdgcn_exp2f(log_boost * c.display_boost / c.max_boost);   // the argument as the reference rounds it
  F3 o;
  o.x = (srgb_inv_oetf_fast(r) * factor) / c.display_boost;
  o.y = (srgb_inv_oetf_fast(g) * factor) / c.display_boost;
  o.z = (srgb_inv_oetf_fast(b) * factor) / c.display_boost;
  return o;
}
// one channel: lin -> the value whose integer part is the code (the half-precision source for F16), and the doubt test (below)
template <int FMT>
__device__ __forceinline__ void est_channel(float lin, float& out, float& doubt_min) {
  if (FMT != 1) {
    const float v = (FMT == 3 ? hlg_oetf_fast(lin) : FMT == 2 ? pq_oetf_est(lin) : lin) * 1023.0f;
    const float d = FMT == 4 ? v * kEstRel : __builtin_fmaf(v, kEstOetfRel, kEstOetfAbs);
    const float f = __builtin_amdgcn_fractf(fmaxf(v, 0.5f));
    doubt_min = fminf(doubt_min, fminf(f, 1.0f - f) - d);   // < 0: in doubt
    out = v;
  } else {
    const _Float16 lo = (_Float16)(lin * (1.0f - kEstRel)), hi = (_Float16)(lin * (1.0f + kEstRel));
    // (beyond the largest half the reference's floatToHalf does not saturate to infinity like the conversion above: it leaves
    // 0x7C00 | mantissa bits, 0x7FFF from 2^17 on -- gainmapmath.cpp:745-780; reachable with minContentBoost > maxContentBoost)
    if (lo != hi || (lin != 0.0f && lin < 0x1p-13f) || !(lin * (1.0f + kEstRel) < 65504.0f)) doubt_min = -1.0f;
    out = lin;
  }
}

template <int FMT>
__global__ void __launch_bounds__(256) k_apply_px_est(const AppConsts c, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.z];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  uint32_t* hdr = c.ex_ws + (size_t)blockIdx.z * kExHdrWords;
  __shared__ uint32_t s_cnt[4], s_base;
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {   // (block-uniform trip count: the barriers below are safe)
    const size_t idx = (size_t)y * c.width + x;
    bool doubt = false;
    if (x < c.width) {
      const PxIn in = px_inputs(c, im, x, y);
      const F3 lin = recover_hdr_est(c, in.yf, kP3Cr * in.v, kP3GCb * in.u, kP3GCr * in.v, kP3Cb * in.u, in.gain);
      float o[3], dm = 1.0f;
      est_channel<FMT>(lin.x, o[0], dm);
      est_channel<FMT>(lin.y, o[1], dm);
      est_channel<FMT>(lin.z, o[2], dm);
      doubt = dm < 0.0f;
      if (FMT == 2 || FMT == 3) {
        static_cast<uint32_t*>(im.dst)[idx] = (0x3ffu & (uint32_t)o[0]) | ((0x3ffu & (uint32_t)o[1]) << 10) | ((0x3ffu & (uint32_t)o[2]) << 20) | (0x3u << 30);
      } else if (FMT == 1) {
        static_cast<uint2*>(im.dst)[idx] = pack_f16_hw(o[0], o[1], o[2]);
      } else {
        uint16_t* base = static_cast<uint16_t*>(im.dst);
        base[idx] = (uint16_t)(0x3ffu & (uint32_t)o[0]);
        base[total + idx] = (uint16_t)(0x3ffu & (uint32_t)o[1]);
        base[2 * total + idx] = (uint16_t)(0x3ffu & (uint32_t)o[2]);
      }
    }
    // one append per block and row: the list is chosen by the block so that neighbouring blocks do not share a counter
    const uint64_t mask = __ballot(doubt);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    __syncthreads();   // (the previous row's s_cnt / s_base have been read)
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    const uint32_t list = (y * gridDim.x + blockIdx.x) % kExLists;
    if (threadIdx.x == 0) {
      const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      s_base = t ? atomicAdd(hdr + 8u + list, t) : 0u;
    }
    __syncthreads();
    if (doubt) {
      uint32_t pos = s_base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      for (uint32_t w = 0; w < wave; ++w) pos += s_cnt[w];
      if (pos < c.ex_cap)
        c.ex_ws[(size_t)kMaxChunk * kExHdrWords + ((size_t)blockIdx.z * kExLists + list) * c.ex_cap + pos] = (uint32_t)idx;
    }
  }
}

// The same estimate for the common geometry (scale 4, aligned planes: app_fast_s4): thread = one map cell = 4x4 pixels, as in
// k_apply_s4 -- the taps, the chroma terms and the addresses are formed once per cell, rows leave as 16-byte stores, and every
// operation of the front end is the reference's own (same order, no contraction) up to the exponent's argument.  Doubt, per channel,
// with v the value whose integer part is the code: the distance of v from the nearest integer against d (v < 1 can only be code 0
// from below, hence the max).  F16: the hardware conversion rounds ties to even where the reference rounds them up; a value the
// interval of which holds a tie is in doubt anyway, and so is the half-precision subnormal range.
template <int FMT, bool INTERIOR>
__device__ __forceinline__ uint32_t est_cell(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, const ApplyCellIn& in, int tbl) {
  const float e1 = map_to_float_fast(in.mb[0]), e2 = map_to_float_fast(in.mb[1]);   // == byte / 255.0f for every byte
  const float e3 = map_to_float_fast(in.mb[2]), e4 = map_to_float_fast(in.mb[3]);
  float crv[2][2], gcbu[2][2], gcrv[2][2], cbu[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float u = (float)((int)((in.uu[r] >> (8 * k)) & 0xffu) - 128) * k255;
      const float v = (float)((int)((in.vv[r] >> (8 * k)) & 0xffu) - 128) * k255;
      crv[r][k] = kP3Cr * v; gcbu[r][k] = kP3GCb * u; gcrv[r][k] = kP3GCr * v; cbu[r][k] = kP3Cb * u;
    }
  const float* wt = c_idw4 + (INTERIOR ? 0 : tbl * 64);
  const bool min_is_one = c.log2_min_d == 0.0;   // log2(min) (1 - g) is then +-0 and leaves the sum as it is
  uint32_t doubt = 0u;
#pragma unroll
  for (int oy = 0; oy < 4; ++oy) {
    float o[4][3];
#pragma unroll
    for (int ox = 0; ox < 4; ++ox) {
      const float* w = wt + oy * 16 + ox * 4;
      const float gain = e1 * w[0] + e2 * w[1] + e3 * w[2] + e4 * w[3];
      const float log_boost = min_is_one ? (float)(c.log2_max_d * (double)gain)
                                         : (float)(c.log2_min_d * (double)(1.0f - gain) + c.log2_max_d * (double)gain);
      const float factor = __builtin_amdgcn_exp2f(log_boost * c.display_boost / c.max_boost) * c.inv_display_boost;
      const float yf = (float)((in.yrow[oy] >> (8 * ox)) & 0xffu) * k255;
      const int r2 = oy >> 1, k2 = ox >> 1;
      // clamp01 as one v_med3_f32 (the same value for every finite input but -0, which ends as code 0 either way)
      const float r = __builtin_amdgcn_fmed3f(yf + crv[r2][k2], 0.0f, 1.0f), g = __builtin_amdgcn_fmed3f(yf - gcbu[r2][k2] - gcrv[r2][k2], 0.0f, 1.0f);
      const float b = __builtin_amdgcn_fmed3f(yf + cbu[r2][k2], 0.0f, 1.0f);
      float dm = 1.0f;
      est_channel<FMT>(srgb_inv_oetf_fast(r) * factor, o[ox][0], dm);
      est_channel<FMT>(srgb_inv_oetf_fast(g) * factor, o[ox][1], dm);
      est_channel<FMT>(srgb_inv_oetf_fast(b) * factor, o[ox][2], dm);
      if (dm < 0.0f) doubt |= 1u << (oy * 4 + ox);
    }
    const uint32_t pix0 = (4u * cy + oy) * c.width + 4u * cx;
    if (FMT == 2 || FMT == 3) {
      uint4 q;
      uint32_t* qq = &q.x;
#pragma unroll
      for (int ox = 0; ox < 4; ++ox)
        qq[ox] = (0x3ffu & (uint32_t)o[ox][0]) | ((0x3ffu & (uint32_t)o[ox][1]) << 10) | ((0x3ffu & (uint32_t)o[ox][2]) << 20) | (0x3u << 30);
      st_stream(reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + pix0), q);
    } else if (FMT == 1) {
      const uint2 a = pack_f16_hw(o[0][0], o[0][1], o[0][2]), bb = pack_f16_hw(o[1][0], o[1][1], o[1][2]);
      const uint2 cc = pack_f16_hw(o[2][0], o[2][1], o[2][2]), d = pack_f16_hw(o[3][0], o[3][1], o[3][2]);
      // (plain stores: a lane's 32 bytes leave as two instructions, each filling half of every line it touches -- L2 merges them,
      // a non-temporal store would send the halves on their own)
      uint4* dst = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + pix0);
      dst[0] = make_uint4(a.x, a.y, bb.x, bb.y);
      dst[1] = make_uint4(cc.x, cc.y, d.x, d.y);
    } else {
      const size_t plane = (size_t)c.width * c.height;
      uint16_t* base16 = static_cast<uint16_t*>(im.dst);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint32_t q0 = 0x3ffu & (uint32_t)o[0][p], q1 = 0x3ffu & (uint32_t)o[1][p];
        const uint32_t q2 = 0x3ffu & (uint32_t)o[2][p], q3 = 0x3ffu & (uint32_t)o[3][p];
        *reinterpret_cast<uint2*>(base16 + p * plane + pix0) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
      }
    }
  }
  return doubt;
}

// ---- the same estimate, two horizontally adjacent pixels per instruction (interior waves of k_apply_s4_est) --------------------------
// The scalar cell above spends ~115 VALU instructions per pixel; v_pk_mul / v_pk_add / v_pk_fma_f32 do two floats per issue slot.
// Every elementary function below performs, per element, the operation sequence of its scalar twin (srgb_inv_oetf_fast,
// hlg_oetf_fast, pq_oetf_est: the error bounds tests/test_gpu_exact_filter.py measures for those hold unchanged); what differs:
//   * the exponent's argument.  The reference rounds log2(max) * gain (a double product) to float, multiplies by the display boost
//     and divides by the content boost.  Here, for |argument| <= 6 and minContentBoost == 1: the double product as a two-float
//     product (exact but for a 2^-48 relative slip that moves the rounded result by one ulp once in 2^24 pixels; one ulp of an
//     argument <= 6 moves the factor by <= 5e-7 relative: part of the budget the test checks) and the division as
//     q + fma(-q, a, x) / a (div_const); other launches keep the scalar cell;
//   * the doubt test: fract(max(v, 1/2) + d) < 2 d instead of min(f, 1 - f) < d -- the same interval but for one rounding at the
//     magnitude of the code value, which kEstPkAbs carries.
constexpr float kEstPkAbs = 6.2e-5f;   // one ulp at 1023
__device__ __forceinline__ f2 srgb_inv_oetf_fast2(f2 e) {
  const f2 lin = e * splat(1.0f / 12.92f);
  const f2 x = (e + splat(0.055f)) * splat(1.0f / 1.055f);
  const f2 p = (x * x) * exp2_2(splat(0.4f) * log2_2(x));
  return (f2){e.x <= 0.04045f ? lin.x : p.x, e.y <= 0.04045f ? lin.y : p.y};
}
__device__ __forceinline__ f2 hlg_oetf_fast2(f2 e) {
  const f2 lo = sqrt_2(splat(3.0f) * e);
  const f2 hi = splat(UHDR_HLG_A * 0.693147180559945f) * log2_2(splat(12.0f) * e - splat(UHDR_HLG_B)) + splat(UHDR_HLG_C);
  return (f2){e.x <= 1.0f / 12.0f ? lo.x : hi.x, e.y <= 1.0f / 12.0f ? lo.y : hi.y};
}
__device__ __forceinline__ f2 pq_oetf_est2(f2 e) {
  const f2 p = exp2_2(splat(UHDR_PQ_M1) * log2_2(e));
  const f2 w = (splat(1.0f - UHDR_PQ_C1) * (splat(1.0f) - p)) * rcp_2(pk_fma(splat(UHDR_PQ_C3), p, splat(1.0f)));
  const f2 s = w * rcp_2(splat(2.0f) - w);
  const f2 s2 = s * s;
  f2 h = pk_fma(s2, splat(1.0f / 7.0f), splat(1.0f / 5.0f));
  h = pk_fma(s2, h, splat(1.0f / 3.0f));
  h = pk_fma(s2 * s, h, s);
  const f2 r = exp2_2(h * splat(-2.0f * 1.4426950408889634f * UHDR_PQ_M2));
  return (f2){e.x <= 0.0f ? 0.0f : r.x, e.y <= 0.0f ? 0.0f : r.y};
}
// one channel of a pixel pair: lin -> code values; dx / dy: that pixel has a channel in doubt (conditions, so that the three
// channels of a pixel combine on the scalar unit)
template <int FMT>
__device__ __forceinline__ void est_channel2(f2 lin, f2& out, bool& dx, bool& dy) {
  if (FMT != 1) {
    const f2 v = (FMT == 3 ? hlg_oetf_fast2(lin) : FMT == 2 ? pq_oetf_est2(lin) : lin) * splat(1023.0f);
    const f2 d = FMT == 4 ? pk_fma(v, splat(kEstRel), splat(kEstPkAbs)) : pk_fma(v, splat(kEstOetfRel), splat(kEstOetfAbs + kEstPkAbs));
    const f2 w = (f2){fmaxf(v.x, 0.5f), fmaxf(v.y, 0.5f)} + d;
    const f2 d2 = d + d;
    out = v;
    dx = dx || __builtin_amdgcn_fractf(w.x) < d2.x;
    dy = dy || __builtin_amdgcn_fractf(w.y) < d2.y;
  } else {
    float o0, o1, m0 = 1.0f, m1 = 1.0f;
    est_channel<1>(lin.x, o0, m0);
    est_channel<1>(lin.y, o1, m1);
    out = (f2){o0, o1};
    dx = dx || m0 < 0.0f;
    dy = dy || m1 < 0.0f;
  }
}
template <int FMT>
__device__ __forceinline__ uint32_t est_cell_pk(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, const ApplyCellIn& in) {
  const f2 e1 = splat(map_to_float_fast(in.mb[0])), e2 = splat(map_to_float_fast(in.mb[1]));
  const f2 e3 = splat(map_to_float_fast(in.mb[2])), e4 = splat(map_to_float_fast(in.mb[3]));
  float crv[2][2], gcbu[2][2], gcrv[2][2], cbu[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float u = (float)((int)((in.uu[r] >> (8 * k)) & 0xffu) - 128) * k255;
      const float v = (float)((int)((in.vv[r] >> (8 * k)) & 0xffu) - 128) * k255;
      crv[r][k] = kP3Cr * v; gcbu[r][k] = kP3GCb * u; gcrv[r][k] = kP3GCr * v; cbu[r][k] = kP3Cb * u;
    }
  // log2(max) as two floats (the caller has checked |log2 max| display / max <= 6 and min == 1)
  const float lh = (float)c.log2_max_d, ll = (float)(c.log2_max_d - (double)lh);
  uint32_t doubt = 0u;
#pragma unroll
  for (int oy = 0; oy < 4; ++oy) {
    f2 o[2][3];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const float* w = c_idw4p + (oy * 2 + pr) * 8;
      f2 gain = e1 * (f2){w[0], w[1]};
      gain = gain + e2 * (f2){w[2], w[3]};
      gain = gain + e3 * (f2){w[4], w[5]};
      gain = gain + e4 * (f2){w[6], w[7]};
      // (float)(log2(max) * (double)gain), then * display / max as the reference rounds them
      const f2 p = gain * splat(lh);
      const f2 log_boost = p + pk_fma(gain, splat(ll), pk_fma(gain, splat(lh), -p));
      const f2 x = log_boost * splat(c.display_boost);
      const f2 q = x * splat(c.inv_max_boost);
      const f2 arg = pk_fma(pk_fma(-q, splat(c.max_boost), x), splat(c.inv_max_boost), q);
      const f2 factor = exp2_2(arg) * splat(c.inv_display_boost);
      const f2 yf = (pr ? (f2){cvt_byte<2>(in.yrow[oy]), cvt_byte<3>(in.yrow[oy])} : (f2){cvt_byte<0>(in.yrow[oy]), cvt_byte<1>(in.yrow[oy])}) * splat(k255);
      const int r2 = oy >> 1;
      const f2 r = pk_add_sat(yf, splat(crv[r2][pr])), g = pk_add_sat(yf - splat(gcbu[r2][pr]), splat(-gcrv[r2][pr]));
      const f2 b = pk_add_sat(yf, splat(cbu[r2][pr]));
      bool dx = false, dy = false;
      est_channel2<FMT>(srgb_inv_oetf_fast2(r) * factor, o[pr][0], dx, dy);
      est_channel2<FMT>(srgb_inv_oetf_fast2(g) * factor, o[pr][1], dx, dy);
      est_channel2<FMT>(srgb_inv_oetf_fast2(b) * factor, o[pr][2], dx, dy);
      doubt |= (dx ? 1u << (oy * 4 + 2 * pr) : 0u) | (dy ? 2u << (oy * 4 + 2 * pr) : 0u);
    }
    const uint32_t pix0 = (4u * cy + oy) * c.width + 4u * cx;
    if (FMT == 2 || FMT == 3) {
      uint4 qv;
      uint32_t* qq = &qv.x;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        qq[2 * pr] = (0x3ffu & (uint32_t)o[pr][0].x) | ((0x3ffu & (uint32_t)o[pr][1].x) << 10) | ((0x3ffu & (uint32_t)o[pr][2].x) << 20) | (0x3u << 30);
        qq[2 * pr + 1] = (0x3ffu & (uint32_t)o[pr][0].y) | ((0x3ffu & (uint32_t)o[pr][1].y) << 10) | ((0x3ffu & (uint32_t)o[pr][2].y) << 20) | (0x3u << 30);
      }
      st_stream(reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + pix0), qv);
    } else if (FMT == 1) {
      const uint2 a = pack_f16_hw(o[0][0].x, o[0][1].x, o[0][2].x), bb = pack_f16_hw(o[0][0].y, o[0][1].y, o[0][2].y);
      const uint2 cc = pack_f16_hw(o[1][0].x, o[1][1].x, o[1][2].x), d = pack_f16_hw(o[1][0].y, o[1][1].y, o[1][2].y);
      uint4* dst = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + pix0);
      dst[0] = make_uint4(a.x, a.y, bb.x, bb.y);
      dst[1] = make_uint4(cc.x, cc.y, d.x, d.y);
    } else {
      const size_t plane = (size_t)c.width * c.height;
      uint16_t* base16 = static_cast<uint16_t*>(im.dst);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint32_t q0 = 0x3ffu & (uint32_t)o[0][p].x, q1 = 0x3ffu & (uint32_t)o[0][p].y;
        const uint32_t q2 = 0x3ffu & (uint32_t)o[1][p].x, q3 = 0x3ffu & (uint32_t)o[1][p].y;
        *reinterpret_cast<uint2*>(base16 + p * plane + pix0) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
      }
    }
  }
  return doubt;
}

template <int FMT>
__global__ void __launch_bounds__(256) k_apply_s4_est(const AppConsts c, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.y];
  const uint32_t cells = c.map_w * c.map_h;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  uint32_t doubt = 0u, cx = 0u, cy = 0u;
  if (idx < cells) {
    cy = idx / c.map_w;
    cx = idx - cy * c.map_w;
    ApplyCellIn in;
    apply_load_cell(c, im, cx, cy, in);
    const bool edge_x = cx + 1u == c.map_w, edge_y = cy + 1u == c.map_h;
    const int tbl = edge_x ? (edge_y ? 3 : 1) : (edge_y ? 2 : 0);
    // (launch-uniform: the packed cell's exponent is budgeted for arguments up to 6 and takes minContentBoost == 1)
    const bool pk = c.log2_min_d == 0.0 && __builtin_fabs(c.log2_max_d) * (double)(c.display_boost * c.inv_max_boost) <= 6.0;
    if (__builtin_amdgcn_ballot_w64(tbl != 0) != 0ull) doubt = est_cell<FMT, false>(c, im, cx, cy, in, tbl);
    else if (pk) doubt = est_cell_pk<FMT>(c, im, cx, cy, in);
    else doubt = est_cell<FMT, true>(c, im, cx, cy, in, 0);
  }
  // one append per block
  __shared__ uint32_t s_part[4], s_base;
  const uint32_t mine = (uint32_t)__popc(doubt);
  const uint32_t before = block_exclusive_sum<256>(mine, s_part);
  const uint32_t list = blockIdx.x % kExLists;
  uint32_t* hdr = c.ex_ws + (size_t)blockIdx.y * kExHdrWords;
  if (threadIdx.x == 255) s_base = (before + mine) ? atomicAdd(hdr + 8u + list, before + mine) : 0u;
  __syncthreads();
  uint32_t pos = s_base + before;
  uint32_t* entries = c.ex_ws + (size_t)kMaxChunk * kExHdrWords + ((size_t)blockIdx.y * kExLists + list) * c.ex_cap;
  while (doubt) {
    const uint32_t k = (uint32_t)__builtin_ctz(doubt);
    doubt &= doubt - 1u;
    if (pos < c.ex_cap) entries[pos] = (4u * cy + (k >> 2)) * c.width + 4u * cx + (k & 3u);
    ++pos;
  }
}

// grid (images, kExSlices).  Every block forms the prefix sums of the image's list lengths, takes its share of the entries and
// recomputes them with the exact path; a list that overflowed turns the image into a sweep of all pixels.  The block that
// finishes last clears the header for the next launch.
template <int FMT>
__global__ void __launch_bounds__(256) k_apply_resolve(const AppConsts c, const AppBatch b) {
  const AppImage& im = b.img[blockIdx.x];
  uint32_t* hdr = c.ex_ws + (size_t)blockIdx.x * kExHdrWords;
  const uint32_t* entries = c.ex_ws + (size_t)kMaxChunk * kExHdrWords + (size_t)blockIdx.x * kExLists * c.ex_cap;
  const size_t total = (size_t)c.width * c.height;
  static_assert(kExLists == 1024, "four lists per thread");
  __shared__ uint32_t s_first[kExLists + 1];
  __shared__ uint32_t s_over;
  if (threadIdx.x == 0) s_over = 0u;
  __syncthreads();
  const uint4 n4 = *reinterpret_cast<const uint4*>(hdr + 8u + 4u * threadIdx.x);
  if (max(max(n4.x, n4.y), max(n4.z, n4.w)) > c.ex_cap) s_over = 1u;
  __shared__ uint32_t s_part[4];
  const uint32_t mine = n4.x + n4.y + n4.z + n4.w;
  const uint32_t before = block_exclusive_sum<256>(mine, s_part);
  s_first[4u * threadIdx.x] = before;
  s_first[4u * threadIdx.x + 1u] = before + n4.x;
  s_first[4u * threadIdx.x + 2u] = before + n4.x + n4.y;
  s_first[4u * threadIdx.x + 3u] = before + n4.x + n4.y + n4.z;
  if (threadIdx.x == 255) s_first[kExLists] = before + mine;
  __syncthreads();
  const bool sweep = s_over != 0u;
  const size_t count = sweep ? total : (size_t)s_first[kExLists];
  for (size_t g = (size_t)blockIdx.y * 256u + threadIdx.x; g < count; g += (size_t)kExSlices * 256u) {
    size_t idx = g;
    if (!sweep) {
      uint32_t lo = 0, hi = kExLists;   // the list with s_first[list] <= g < s_first[list + 1]
      while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_first[mid] <= (uint32_t)g) lo = mid; else hi = mid; }
      idx = entries[(size_t)lo * c.ex_cap + ((uint32_t)g - s_first[lo])];
    }
    const uint32_t py = (uint32_t)(idx / c.width), px = (uint32_t)(idx - (size_t)py * c.width);
    const PxIn in = px_inputs(c, im, px, py);
    const F3 lin = recover_hdr<true>(c, in.yf, kP3Cr * in.v, kP3GCb * in.u, kP3GCr * in.v, kP3Cb * in.u, in.gain);
    px_store<FMT>(im, idx, total, hdr_oetf<FMT, true>(lin));
  }
  // the header is cleared by the slice that finishes last (every slice has read the counts by then)
  __shared__ uint32_t s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(hdr + 3u, 1u) == kExSlices - 1u;
  __syncthreads();
  if (s_last) {
    reinterpret_cast<uint4*>(hdr + 8u)[threadIdx.x] = make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 0) hdr[3] = 0u;
  }
}

// LUT mode (ultrahdr.cpp:433,446,470,481 with USE_*_LUT = 1): srgbInvOetfLUT, applyGainLUT, hlg/pqOetfLUT.
// One thread per pixel, any integer scale.  Each block first builds its private copies of the sRGB table and of
// GainLUT(metadata, display_boost) in LDS (the latter costs 4 double exp2 per thread, hence kLutPixelsPerThread
// pixels per thread); the 65536-entry OETF tables (256 KiB each) are gathered from L2.
constexpr uint32_t kLutPixelsPerThread = 16;
template <int FMT>
__global__ void __launch_bounds__(256) k_apply_lut(const AppConsts c, const AppBatch b) {
  __shared__ float s_srgb[kLutSrgbInvN];
  __shared__ float s_gain[kGainLutN];
  for (uint32_t i = threadIdx.x; i < kLutSrgbInvN; i += 256u) {
    s_srgb[i] = c.lut[kLutSrgbInv + i];
    s_gain[i] = gain_lut_entry(i, c.log2_min_d, c.log2_max_d, c.lut_boost_factor);
  }
  __syncthreads();
  const float* oetf = c.lut + (FMT == 3 ? kLutHlg : kLutPq);
  const AppImage& im = b.img[blockIdx.y];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t s = c.scale;
  for (size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256u) {
    const uint32_t y = (uint32_t)(idx / c.width);
    const uint32_t x = (uint32_t)(idx - (size_t)y * c.width);
    const float yf = (float)im.y[(size_t)y * im.y_stride + x] * k255;
    const size_t ci = (size_t)(y >> im.csy) * im.c_stride + (x >> im.csx);
    const float u = (float)((int)im.u[ci] - 128) * k255;
    const float v = (float)((int)im.v[ci] - 128) * k255;
    // sampleMap (gainmapmath.cpp:686-720), as in k_apply_px
    uint32_t xl = x / s, yl = y / s;
    uint32_t xu = xl + 1u, yu = yl + 1u;
    xl = min(xl, c.map_w - 1u); xu = min(xu, c.map_w - 1u);
    yl = min(yl, c.map_h - 1u); yu = min(yu, c.map_h - 1u);
    const float e1 = map_to_float(im.map[(size_t)yl * c.map_w + xl]);
    const float e2 = map_to_float(im.map[(size_t)yu * c.map_w + xl]);
    const float e3 = map_to_float(im.map[(size_t)yl * c.map_w + xu]);
    const float e4 = map_to_float(im.map[(size_t)yu * c.map_w + xu]);
    const uint32_t ox = x % s, oy = y % s;
    int tbl = 0;
    if (xl == xu && yl == yu) tbl = 3;
    else if (xl == xu) tbl = 1;
    else if (yl == yu) tbl = 2;
    const float* w = c.idw + (size_t)tbl * s * s * 4u + (size_t)oy * s * 4u + ox * 4u;
    const float gain = e1 * w[0] + e2 * w[1] + e3 * w[2] + e4 * w[3];

    const float r = s_srgb[lut_index_unit(clamp01(yf + kP3Cr * v), kLutSrgbInvN)];
    const float g = s_srgb[lut_index_unit(clamp01(yf - kP3GCb * u - kP3GCr * v), kLutSrgbInvN)];
    const float bl = s_srgb[lut_index_unit(clamp01(yf + kP3Cb * u), kLutSrgbInvN)];
    const float factor = s_gain[lut_index(gain, kGainLutN)];       // GainLUT::getGainFactor, gainmapmath.h:173-178
    F3 e;
    e.x = (r * factor) / c.display_boost;                          // applyGainLUT, then ultrahdr.cpp:451
    e.y = (g * factor) / c.display_boost;
    e.z = (bl * factor) / c.display_boost;
    if (FMT == 2 || FMT == 3) {
      e.x = oetf[lut_index(e.x, kLutHlgN)]; e.y = oetf[lut_index(e.y, kLutHlgN)]; e.z = oetf[lut_index(e.z, kLutHlgN)];
      static_cast<uint32_t*>(im.dst)[idx] = pack_1010102(e.x, e.y, e.z);
    } else if (FMT == 1) {
      static_cast<uint2*>(im.dst)[idx] = pack_f16(e.x, e.y, e.z);
    } else {
      uint16_t* base = static_cast<uint16_t*>(im.dst);
      base[idx] = (uint16_t)(0x3ffu & (uint32_t)(e.x * 1023.0f));
      base[total + idx] = (uint16_t)(0x3ffu & (uint32_t)(e.y * 1023.0f));
      base[2 * total + idx] = (uint16_t)(0x3ffu & (uint32_t)(e.z * 1023.0f));
    }
  }
}

// LUT mode for the common geometry (scale 4, aligned planes: app_fast_s4).  Thread = one map cell; 1024-thread blocks, one per CU,
// that live for the whole launch (block b takes the 1024-cell chunks b, b + G, ... of the batch): what makes them expensive to
// start is what makes them fast -- the OETF table sits in LDS as its 65536 10-bit codes (128 KiB; uhdr_kernels.h), next to the
// sRGB table and GainLUT(metadata, display_boost), so no lookup leaves the CU.  The arithmetic is k_apply_lut's, operation for
// operation (the taps' / 255 through the constant division that is proven equal, the weights from the scale-4 table).
template <int FMT, bool INTERIOR>
__device__ __forceinline__ void lut_cell(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, const ApplyCellIn& in, int tbl,
                                         const float* s_srgb, const float* s_gain, const uint16_t* s_code) {
  const float e1 = map_to_float_fast(in.mb[0]), e2 = map_to_float_fast(in.mb[1]);
  const float e3 = map_to_float_fast(in.mb[2]), e4 = map_to_float_fast(in.mb[3]);
  float crv[2][2], gcbu[2][2], gcrv[2][2], cbu[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float u = (float)((int)((in.uu[r] >> (8 * k)) & 0xffu) - 128) * k255;
      const float v = (float)((int)((in.vv[r] >> (8 * k)) & 0xffu) - 128) * k255;
      crv[r][k] = kP3Cr * v; gcbu[r][k] = kP3GCb * u; gcrv[r][k] = kP3GCr * v; cbu[r][k] = kP3Cb * u;
    }
  const float* wt = c_idw4 + (INTERIOR ? 0 : tbl * 64);
#pragma unroll
  for (int oy = 0; oy < 4; ++oy) {
    float o[4][3];
#pragma unroll
    for (int ox = 0; ox < 4; ++ox) {
      const float* w = wt + oy * 16 + ox * 4;
      const float gain = e1 * w[0] + e2 * w[1] + e3 * w[2] + e4 * w[3];
      const float factor = s_gain[lut_index(gain, kGainLutN)];
      const float yf = (float)((in.yrow[oy] >> (8 * ox)) & 0xffu) * k255;
      const int r2 = oy >> 1, k2 = ox >> 1;
      const float r = s_srgb[lut_index_unit(clamp01(yf + crv[r2][k2]), kLutSrgbInvN)];
      const float g = s_srgb[lut_index_unit(clamp01(yf - gcbu[r2][k2] - gcrv[r2][k2]), kLutSrgbInvN)];
      const float bl = s_srgb[lut_index_unit(clamp01(yf + cbu[r2][k2]), kLutSrgbInvN)];
      o[ox][0] = (r * factor) / c.display_boost;
      o[ox][1] = (g * factor) / c.display_boost;
      o[ox][2] = (bl * factor) / c.display_boost;
    }
    const uint32_t pix0 = (4u * cy + oy) * c.width + 4u * cx;
    if (FMT == 2 || FMT == 3) {
      uint4 q;
      uint32_t* qq = &q.x;
#pragma unroll
      for (int ox = 0; ox < 4; ++ox)
        qq[ox] = (uint32_t)s_code[lut_index(o[ox][0], kLutHlgN)] | ((uint32_t)s_code[lut_index(o[ox][1], kLutHlgN)] << 10) |
                 ((uint32_t)s_code[lut_index(o[ox][2], kLutHlgN)] << 20) | (0x3u << 30);
      st_stream(reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + pix0), q);
    } else if (FMT == 1) {
      const uint2 a = pack_f16(o[0][0], o[0][1], o[0][2]), bb = pack_f16(o[1][0], o[1][1], o[1][2]);
      const uint2 cc = pack_f16(o[2][0], o[2][1], o[2][2]), d = pack_f16(o[3][0], o[3][1], o[3][2]);
      uint4* dst = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + pix0);
      dst[0] = make_uint4(a.x, a.y, bb.x, bb.y);
      dst[1] = make_uint4(cc.x, cc.y, d.x, d.y);
    } else {
      const size_t plane = (size_t)c.width * c.height;
      uint16_t* base16 = static_cast<uint16_t*>(im.dst);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint32_t q0 = 0x3ffu & (uint32_t)(o[0][p] * 1023.0f), q1 = 0x3ffu & (uint32_t)(o[1][p] * 1023.0f);
        const uint32_t q2 = 0x3ffu & (uint32_t)(o[2][p] * 1023.0f), q3 = 0x3ffu & (uint32_t)(o[3][p] * 1023.0f);
        *reinterpret_cast<uint2*>(base16 + p * plane + pix0) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
      }
    }
  }
}

// The same cell for interior waves of calls whose division cannot need operand scaling (AppConsts::lut_plain_div), two horizontally
// adjacent pixels per instruction: every float operation is lut_cell's, in its order, on both pixels at once (v_pk_mul / add / fma;
// clampPixelFloat through the packed clamp modifier: the same value but for the sign of a zero, which indexes the same table
// entry).  The division x / display_boost is the IEEE expansion hipcc emits for it --
//     y0 = rcp(b), e0 = fma(-b, y0, 1), y1 = fma(e0, y0, y0);  q0 = x y1, r0 = fma(-b, q0, x), q1 = fma(r0, y1, q0),
//     r1 = fma(-b, q1, x), q = fma(r1, y1, q1)
// -- without v_div_scale_f32 / v_div_fixup_f32 around it: for operands in the ranges the host has checked those change nothing
// (no rescaling, no special case but x = 0, which the chain maps to +0 by itself), so the quotient is the correctly rounded one,
// bit for bit what the scalar cell computes.  y1 is formed once per thread; a quotient costs five packed instructions per two
// values where the expansion spends eleven per value, a quarter-rate v_rcp_f32 among them.
template <int FMT>
__device__ __forceinline__ void lut_cell_pk(const AppConsts& c, const AppImage& im, uint32_t cx, uint32_t cy, const ApplyCellIn& in,
                                            const float* s_srgb, const float* s_gain, const uint16_t* s_code) {
  const f2 e1 = splat(map_to_float_fast(in.mb[0])), e2 = splat(map_to_float_fast(in.mb[1]));
  const f2 e3 = splat(map_to_float_fast(in.mb[2])), e4 = splat(map_to_float_fast(in.mb[3]));
  float crv[2][2], gcbu[2][2], gcrv[2][2], cbu[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float u = (float)((int)((in.uu[r] >> (8 * k)) & 0xffu) - 128) * k255;
      const float v = (float)((int)((in.vv[r] >> (8 * k)) & 0xffu) - 128) * k255;
      crv[r][k] = kP3Cr * v; gcbu[r][k] = kP3GCb * u; gcrv[r][k] = kP3GCr * v; cbu[r][k] = kP3Cb * u;
    }
  const float db = c.display_boost, y0 = __builtin_amdgcn_rcpf(db), e0 = __builtin_fmaf(-db, y0, 1.0f), y1 = __builtin_fmaf(e0, y0, y0);
  const f2 nb = splat(-db), yy = splat(y1);
#pragma unroll
  for (int oy = 0; oy < 4; ++oy) {
    f2 o[2][3];
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const float* w = c_idw4p + (oy * 2 + pr) * 8;
      f2 gain = e1 * (f2){w[0], w[1]};
      gain = gain + e2 * (f2){w[2], w[3]};
      gain = gain + e3 * (f2){w[4], w[5]};
      gain = gain + e4 * (f2){w[6], w[7]};
      // (0 <= gain <= 1 + a few ulps -- weights that sum to 1, taps in [0, 1] -- so the product stays below N - 1/2: CLIP3 cannot bite)
      const f2 tg = gain * splat((float)(kGainLutN - 1u));
      const f2 factor = (f2){s_gain[round_half_up(tg.x)], s_gain[round_half_up(tg.y)]};
      const f2 yf = (pr ? (f2){cvt_byte<2>(in.yrow[oy]), cvt_byte<3>(in.yrow[oy])} : (f2){cvt_byte<0>(in.yrow[oy]), cvt_byte<1>(in.yrow[oy])}) * splat(k255);
      const int r2 = oy >> 1;
      const f2 rr = pk_add_sat(yf, splat(crv[r2][pr])), gg = pk_add_sat(yf - splat(gcbu[r2][pr]), splat(-gcrv[r2][pr]));
      const f2 bb = pk_add_sat(yf, splat(cbu[r2][pr]));
      const f2 tr = rr * splat((float)(kLutSrgbInvN - 1u)), tgr = gg * splat((float)(kLutSrgbInvN - 1u)), tb = bb * splat((float)(kLutSrgbInvN - 1u));
      const f2 ch[3] = {(f2){s_srgb[round_half_up(tr.x)], s_srgb[round_half_up(tr.y)]},
                        (f2){s_srgb[round_half_up(tgr.x)], s_srgb[round_half_up(tgr.y)]},
                        (f2){s_srgb[round_half_up(tb.x)], s_srgb[round_half_up(tb.y)]}};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f2 x = ch[q] * factor;                           // applyGainLUT
        const f2 q0 = x * yy, r0 = pk_fma(nb, q0, x), q1 = pk_fma(r0, yy, q0), r1 = pk_fma(nb, q1, x);
        // / display_boost (ultrahdr.cpp:451).  HLG / PQ: the quotient only indexes the OETF table, where everything from 1.0 up
        // lands on the last entry (CLIP3): saturating it to 1.0 -- the instruction's clamp bit -- stands in for the clip of the index
        if (FMT == 2 || FMT == 3) o[pr][q] = pk_fma_sat(r1, yy, q1) * splat((float)(kLutHlgN - 1u));
        else o[pr][q] = pk_fma(r1, yy, q1);
      }
    }
    const uint32_t pix0 = (4u * cy + oy) * c.width + 4u * cx;
    if (FMT == 2 || FMT == 3) {
      uint4 qv;
      uint32_t* qq = &qv.x;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        qq[2 * pr] = (uint32_t)s_code[round_half_up(o[pr][0].x)] | ((uint32_t)s_code[round_half_up(o[pr][1].x)] << 10) |
                     ((uint32_t)s_code[round_half_up(o[pr][2].x)] << 20) | (0x3u << 30);
        qq[2 * pr + 1] = (uint32_t)s_code[round_half_up(o[pr][0].y)] | ((uint32_t)s_code[round_half_up(o[pr][1].y)] << 10) |
                         ((uint32_t)s_code[round_half_up(o[pr][2].y)] << 20) | (0x3u << 30);
      }
      st_stream(reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + pix0), qv);
    } else if (FMT == 1) {
      const uint2 a = pack_f16(o[0][0].x, o[0][1].x, o[0][2].x), b2 = pack_f16(o[0][0].y, o[0][1].y, o[0][2].y);
      const uint2 cc = pack_f16(o[1][0].x, o[1][1].x, o[1][2].x), d = pack_f16(o[1][0].y, o[1][1].y, o[1][2].y);
      uint4* dst = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + pix0);
      dst[0] = make_uint4(a.x, a.y, b2.x, b2.y);
      dst[1] = make_uint4(cc.x, cc.y, d.x, d.y);
    } else {
      const size_t plane = (size_t)c.width * c.height;
      uint16_t* base16 = static_cast<uint16_t*>(im.dst);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint32_t q0 = 0x3ffu & (uint32_t)(o[0][p].x * 1023.0f), q1 = 0x3ffu & (uint32_t)(o[0][p].y * 1023.0f);
        const uint32_t q2 = 0x3ffu & (uint32_t)(o[1][p].x * 1023.0f), q3 = 0x3ffu & (uint32_t)(o[1][p].y * 1023.0f);
        *reinterpret_cast<uint2*>(base16 + p * plane + pix0) = make_uint2(q0 | (q1 << 16), q2 | (q3 << 16));
      }
    }
  }
}

constexpr uint32_t kLutS4Block = 1024;
template <int FMT>
__global__ void __launch_bounds__(1024) k_apply_lut_s4(const AppConsts c, const AppBatch b, uint32_t n) {
  constexpr bool kOetf = FMT == 2 || FMT == 3;
  extern __shared__ uint4 s_dyn[];                       // [codes 128 KiB (HLG / PQ output only)] [sRGB 4 KiB] [gain 4 KiB]
  uint16_t* s_code = reinterpret_cast<uint16_t*>(s_dyn);
  float* s_srgb = reinterpret_cast<float*>(reinterpret_cast<char*>(s_dyn) + (kOetf ? kLutHlgN * 2u : 0u));
  float* s_gain = s_srgb + kLutSrgbInvN;
  static_assert(kLutSrgbInvN == kLutS4Block && kGainLutN == kLutS4Block, "one table entry per thread");
  s_srgb[threadIdx.x] = c.lut[kLutSrgbInv + threadIdx.x];
  s_gain[threadIdx.x] = gain_lut_entry(threadIdx.x, c.log2_min_d, c.log2_max_d, c.lut_boost_factor);
  if (kOetf) {
    const uint4* src = reinterpret_cast<const uint4*>(c.lut + (FMT == 3 ? kCodeHlg : kCodePq));
    uint4 t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = src[k * kLutS4Block + threadIdx.x];
#pragma unroll
    for (int k = 0; k < 8; ++k) s_dyn[k * kLutS4Block + threadIdx.x] = t[k];
  }
  __syncthreads();
  const uint32_t cells = c.map_w * c.map_h, per_img = (cells + kLutS4Block - 1u) / kLutS4Block, total = per_img * n;
  for (uint32_t id = blockIdx.x; id < total; id += gridDim.x) {
    const uint32_t img = id / per_img, idx = (id - img * per_img) * kLutS4Block + threadIdx.x;
    if (idx >= cells) continue;
    const AppImage& im = b.img[img];
    const uint32_t cy = idx / c.map_w, cx = idx - cy * c.map_w;
    ApplyCellIn in;
    apply_load_cell(c, im, cx, cy, in);
    const bool edge_x = cx + 1u == c.map_w, edge_y = cy + 1u == c.map_h;
    const int tbl = edge_x ? (edge_y ? 3 : 1) : (edge_y ? 2 : 0);
    if (__builtin_amdgcn_ballot_w64(tbl != 0) != 0ull) lut_cell<FMT, false>(c, im, cx, cy, in, tbl, s_srgb, s_gain, s_code);
    else if (c.lut_plain_div != 0u) lut_cell_pk<FMT>(c, im, cx, cy, in, s_srgb, s_gain, s_code);
    else lut_cell<FMT, true>(c, im, cx, cy, in, 0, s_srgb, s_gain, s_code);
  }
}

// the estimate kernel's grid: k_apply_s4_est (blocks of 256 cells, image) or k_apply_px_est (px_grid)
static dim3 est_grid(const AppConsts& c, int n, bool fast_s4) {
  return fast_s4 ? dim3((c.map_w * c.map_h + 255u) / 256u, n) : px_grid(c.width, c.height, n);
}
void apply_est_grid(const AppConsts& c, int n, bool fast_s4, uint32_t grid[2]) {
  const dim3 g = est_grid(c, n, fast_s4);
  grid[0] = g.x;
  grid[1] = g.y;
}

template <int FMT>
static hipError_t launch_apply_t(const AppConsts& c, const AppBatch& b, int n, int mode,
                                 bool fast_s4, hipStream_t s, unsigned ex_phases) {
  if (n == 0 || c.width == 0 || c.height == 0) return hipSuccess;
  const bool exact = mode == 1 || mode == 3;
  if (mode == 2) {
    if (c.lut == nullptr) return hipErrorInvalidValue;
    if (fast_s4) {
      constexpr bool kOetf = FMT == 2 || FMT == 3;
      const uint32_t lds = (kOetf ? kLutHlgN * 2u : 0u) + (kLutSrgbInvN + kGainLutN) * 4u;
      const uint32_t chunks = (c.map_w * c.map_h + kLutS4Block - 1u) / kLutS4Block * (uint32_t)n;
      // more than 64 KiB of LDS has to be allowed per function (and per device: set on every launch, it is a host-side flag)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_apply_lut_s4<FMT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) {
        hipLaunchKernelGGL((k_apply_lut_s4<FMT>), dim3(chunks < 256u ? chunks : 256u), dim3(kLutS4Block), lds, s, c, b, (uint32_t)n);
        return hipGetLastError();
      }
      (void)hipGetLastError();   // (a device that does not grant the LDS: the per-pixel kernel below gives the same bytes)
    }
    const size_t total = (size_t)c.width * c.height, per_block = 256u * (size_t)kLutPixelsPerThread;
    hipLaunchKernelGGL((k_apply_lut<FMT>), dim3((unsigned)((total + per_block - 1u) / per_block), n), dim3(256), 0, s, c, b);
    return hipGetLastError();
  }
  if (fast_s4 && !exact && c.map_w >= 2u) {   // (a map one cell wide: the per-pixel kernel; apply_load_cell_pk reads two columns)
    // Cells per thread: a block copies 15-37 KB of tables into LDS before its first pixel, so it should walk many cells -- but a
    // launch also has to fill 256 CUs x 2 resident blocks, or a single 4K image (2025 blocks of 256 cells) would leave three
    // quarters of the chip idle with 8 cells per thread.
    AppConsts cc = c;
    const uint32_t total = c.map_w * c.map_h;
    uint32_t cpt = kApplyMaxCellsPerThread;
    auto blocks = [&](uint32_t k) { return (uint64_t)((total + kApplyBlock * k - 1u) / (kApplyBlock * k)) * (uint64_t)n; };
    while (cpt > 1u && blocks(cpt) < 448u) cpt >>= 1;   // (a single 4K image: 507 blocks of 2 cells per thread, all resident at once)
    cc.cells_per_thread = cpt;
    cc.step_x = kApplyBlock % c.map_w;
    cc.step_y = kApplyBlock / c.map_w;
    const dim3 grid(n, (unsigned)((total + kApplyBlock * cpt - 1u) / (kApplyBlock * cpt)));
    // Channels can only exceed 1.0 (reach code 1024 and wrap through the reference's & 0x3ff; leave the stage-2 table) when the
    // display boost is capped below the content boost -- and then only if the largest factor the call can produce,
    // max(minBoost, maxBoost)^(display / max) / display, is above 1: a display boost of 2 under a content boost of 4.9 stays
    // below (0.955), a display boost of 1 does not (1.38).
    // The factor alone decides: with minContentBoost > maxContentBoost (nothing on the apply path refuses it, ultrahdr.cpp:360-425;
    // a crafted XMP gets here through decodeJPEGR) `top` is far above 1 although display_boost == max_boost, and stage 2's cell
    // number -- byte 2 of 2 + 2u, unclamped -- would index past its 129 cells.
    const double top = std::exp2(std::fmax(c.log2_min_d, c.log2_max_d) * (double)c.display_boost / (double)c.max_boost) / (double)c.display_boost;
    const bool mask = !(top <= 1.0 + 1e-6);
    if (!mask && ApplyTab<FMT, false>::kOetf) {
      // u = T(c) * 2^(g E), handed to stage 2 as 2 + 2u: the exponent's constants times g (1/2 for HLG: sqrt; m1 for PQ), plus 1
      const float g = FMT == 3 ? 0.5f : UHDR_PQ_M1;
      cc.fast.A *= g; cc.fast.A255 *= g; cc.fast.B = cc.fast.B * g + 1.0f;
    }
    // sampleMap's standard weights times A / 255: ONE float product per weight, the same one the kernel forms for the per-lane
    // tables of the last column / row (its prologue, round to nearest) -- a cell gets the same bytes whichever form computes it
    for (int i = 0; i < 4 * 2 * 3 * 2; ++i) (&cc.fast.wD[0][0][0][0])[i] *= cc.fast.A255;
    if (mask) hipLaunchKernelGGL((k_apply_s4<FMT, true>), grid, dim3(kApplyBlock), 0, s, cc, b);
    else hipLaunchKernelGGL((k_apply_s4<FMT, false>), grid, dim3(kApplyBlock), 0, s, cc, b);
  } else {
    const dim3 grid = px_grid(c.width, c.height, n);
    if (exact && c.ex_ws != nullptr) {
      if (ex_phases & kExPhaseEst) {
        if (fast_s4) hipLaunchKernelGGL((k_apply_s4_est<FMT>), est_grid(c, n, true), dim3(256), 0, s, c, b);
        else hipLaunchKernelGGL((k_apply_px_est<FMT>), est_grid(c, n, false), dim3(256), 0, s, c, b);
      }
      if (ex_phases & kExPhaseResolve) hipLaunchKernelGGL((k_apply_resolve<FMT>), dim3(n, kExSlices), dim3(256), 0, s, c, b);
    } else if (exact) hipLaunchKernelGGL((k_apply_px<FMT, true>), grid, dim3(256), 0, s, c, b);
    else hipLaunchKernelGGL((k_apply_px<FMT, false>), grid, dim3(256), 0, s, c, b);
  }
  return hipGetLastError();
}

hipError_t launch_apply(const AppConsts& c, const AppBatch& b, int n, int fmt, int mode,
                        bool fast_s4, hipStream_t s, unsigned ex_phases) {
  switch (fmt) {
    case 1: return launch_apply_t<1>(c, b, n, mode, fast_s4, s, ex_phases);
    case 2: return launch_apply_t<2>(c, b, n, mode, fast_s4, s, ex_phases);
    case 3: return launch_apply_t<3>(c, b, n, mode, fast_s4, s, ex_phases);
    case 4: return launch_apply_t<4>(c, b, n, mode, fast_s4, s, ex_phases);
    default: return hipErrorInvalidValue;
  }
}

// =================================================================================================
// The SDR rendition of decodeJPEGR (jpegr.cpp:768-786): what JpegDecoderHelper::decompressImage(..., DECODE_TO_RGBA) makes of the
// primary image (jpegdecoderhelper.cpp:251-281), i.e. libjpeg-turbo's own path from the decoded 4:2:0 planes to RGBA:
//   jdsample.c h2v2_fancy_upsample  triangle filter over the four nearest chroma samples, weights 9 3 3 1 / 16, rounding constant 8
//                                    on even and 7 on odd columns, edges replicated; chroma planes at most 2 samples wide are
//                                    replicated instead (jinit_upsampler)
//   jdcolor.c ycc_rgb_convert        R = Y + ((91881 (Cr-128) + 32768) >> 16) etc., the tables of build_ycc_rgb_table evaluated in
//                                    place, clamp to 0..255, alpha 0xFF
// One thread per horizontal pixel pair (they share the centre chroma column).  Restated in oracle/jpeg_oracle.c and pinned there
// against libjpeg-turbo itself (Pillow's).
// =================================================================================================
// libjpeg-turbo's conversion of one pixel: R, G, B in bytes 0..2, alpha 0xFF
__device__ __forceinline__ uint32_t ycc_rgba_px(int y, int cb, int cr) {
  const int xb = cb - 128, xr = cr - 128;
  int R = y + ((91881 * xr + 32768) >> 16);
  int G = y + ((-22554 * xb + 32768 - 46802 * xr) >> 16);
  int B = y + ((116130 * xb + 32768) >> 16);
  R = min(max(R, 0), 255); G = min(max(G, 0), 255); B = min(max(B, 0), 255);
  return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16) | 0xFF000000u;
}
// the pixel pair (2c, 2c+1) of row r
__device__ __forceinline__ void ycc420_rgba_pair(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cbp, const uint8_t* __restrict__ crp,
                                                 uint32_t w, uint32_t h, uint32_t ys, uint32_t cs, uint8_t* __restrict__ rgba, uint32_t c, uint32_t r) {
  const uint32_t cw = w >> 1, ch = h >> 1;
  const uint32_t i = r >> 1;
  const uint32_t o = (r & 1u) ? min(i + 1u, ch - 1u) : (i ? i - 1u : 0u);
  const uint32_t cl = c ? c - 1u : 0u, cr_ = min(c + 1u, cw - 1u);
  int cb[2], cr[2];
  if (cw > 2u) {
    auto colsum = [&](const uint8_t* p, uint32_t col) { return 3 * (int)p[i * cs + col] + (int)p[o * cs + col]; };
    const int b0 = colsum(cbp, c), r0 = colsum(crp, c);
    cb[0] = (3 * b0 + colsum(cbp, cl) + 8) >> 4; cb[1] = (3 * b0 + colsum(cbp, cr_) + 7) >> 4;
    cr[0] = (3 * r0 + colsum(crp, cl) + 8) >> 4; cr[1] = (3 * r0 + colsum(crp, cr_) + 7) >> 4;
  } else {
    cb[0] = cb[1] = cbp[i * cs + c];
    cr[0] = cr[1] = crp[i * cs + c];
  }
  const uint8_t* yrow = yp + (size_t)r * ys + 2u * c;
  const uint32_t y2 = (uint32_t)yrow[0] | ((uint32_t)yrow[1] << 8);
  uint32_t px[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) px[k] = ycc_rgba_px((int)((y2 >> (8 * k)) & 0xffu), cb[k], cr[k]);
  *reinterpret_cast<uint2*>(rgba + ((size_t)r * w + 2u * c) * 4u) = make_uint2(px[0], px[1]);
}

// The chroma sample libjpeg-turbo's upsampler (jdsample.c) puts under pixel (x, y) of a plane subsampled in ONE direction:
//   4:4:4  the sample itself
//   4:2:2  h2v1_fancy_upsample along the row: even columns (3 c[i] + c[i-1] + 1) >> 2, odd ones (3 c[i] + c[i+1] + 2) >> 2, the first
//          and the last output column of the (even-width) upsampled row the end samples themselves; rows of at most 2 samples
//          are replicated (jinit_upsampler takes h2v1_upsample for them)
//   4:4:0  h1v2_fancy_upsample down the column: even rows (3 c[j] + c[j-1] + 1) >> 2, odd ones (3 c[j] + c[j+1] + 2) >> 2, the
//          neighbour clamped to the plane
// plain: h2v1_upsample / h1v2 replication, the sample itself in every case
__device__ __forceinline__ int yccx_chroma(const uint8_t* __restrict__ p, uint32_t cs, uint32_t cw, uint32_t ch, uint32_t hs, uint32_t vs,
                                           uint32_t x, uint32_t y, bool plain) {
  if (hs == 2u) {
    const uint32_t i = x >> 1;
    const uint8_t* row = p + (size_t)y * cs;
    const int c = row[i];
    if (cw <= 2u || plain) return c;
    if (x & 1u) return i + 1u < cw ? (3 * c + (int)row[i + 1u] + 2) >> 2 : c;
    return i ? (3 * c + (int)row[i - 1u] + 1) >> 2 : c;
  }
  if (vs == 2u) {
    const uint32_t j = y >> 1;
    const int c = p[(size_t)j * cs + x];
    if (plain) return c;
    const uint32_t o = (y & 1u) ? min(j + 1u, ch - 1u) : (j ? j - 1u : 0u);
    return (3 * c + (int)p[(size_t)o * cs + x] + ((y & 1u) ? 2 : 1)) >> 2;
  }
  return p[(size_t)y * cs + x];
}
// 4:4:4 / 4:2:2 / 4:4:0 planes -> RGBA: a thread converts pixels [4g, 4g + 4) of the packed w * h output, so that its store is one
// aligned 16 bytes whatever the width (the four may lie in two rows); a tail of w * h % 4 pixels, and an output that is not 16-byte
// aligned, go out pixel by pixel.  grid.z = image, grid.x strided over the image's groups.
__global__ void __launch_bounds__(256) k_yccx_rgba_batch(const YccxRgbaBatch b) {
  const YccRgbaImage& im = b.img[blockIdx.z].im;
  const uint32_t hs = b.img[blockIdx.z].hs, vs = b.img[blockIdx.z].vs;
  const bool plain = b.img[blockIdx.z].plain != 0u;
  const uint32_t cw = (im.w + hs - 1u) / hs, ch = (im.h + vs - 1u) / vs;
  const uint32_t total = im.w * im.h, groups = (total + 3u) >> 2;   // (w, h <= 8192: 2^26 pixels)
  const bool aligned = (reinterpret_cast<uintptr_t>(im.rgba) & 15u) == 0u;
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
    const uint32_t p0 = 4u * g, cnt = min(4u, total - p0);
    uint32_t y = p0 / im.w, x = p0 - y * im.w;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if (k < cnt) {
        px[k] = ycc_rgba_px((int)im.y[(size_t)y * im.ys + x], yccx_chroma(im.cb, im.cs, cw, ch, hs, vs, x, y, plain),
                            yccx_chroma(im.cr, im.cs, cw, ch, hs, vs, x, y, plain));
        if (++x == im.w) { x = 0u; ++y; }
      }
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(im.rgba) + p0;
    if (aligned && cnt == 4u) *reinterpret_cast<uint4*>(out) = make_uint4(px[0], px[1], px[2], px[3]);
    else {
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k)
        if (k < cnt) out[k] = px[k];
    }
  }
}

hipError_t launch_yccx_to_rgba_batch(const YccxRgbaBatch& b, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kRgbaChunk) return hipErrorInvalidValue;
  uint32_t groups = 1;
  for (int k = 0; k < n; ++k) groups = std::max(groups, (b.img[k].im.w * b.img[k].im.h + 3u) / 4u);
  hipLaunchKernelGGL(k_yccx_rgba_batch, dim3(std::min((groups + 255u) / 256u, 4096u), 1, (unsigned)n), dim3(256), 0, s, b);
  return hipGetLastError();
}

// n images of any sizes in one launch: grid.z = image, grid.x over the widest image's pixel pairs, rows strided by grid.y
__global__ void __launch_bounds__(256) k_ycc420_rgba_batch(const YccRgbaBatch b) {
  const YccRgbaImage& im = b.img[blockIdx.z];
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= (im.w >> 1)) return;
  for (uint32_t r = blockIdx.y; r < im.h; r += gridDim.y) ycc420_rgba_pair(im.y, im.cb, im.cr, im.w, im.h, im.ys, im.cs, im.rgba, c, r);
}

hipError_t launch_ycc420_to_rgba_batch(const YccRgbaBatch& b, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kRgbaChunk) return hipErrorInvalidValue;
  uint32_t gx = 1, gy = 1;
  for (int k = 0; k < n; ++k) {
    gx = std::max(gx, (b.img[k].w / 2u + 255u) / 256u);
    gy = std::max(gy, b.img[k].h);
  }
  hipLaunchKernelGGL(k_ycc420_rgba_batch, dim3(gx, std::min(gy, 65535u), (unsigned)n), dim3(256), 0, s, b);
  return hipGetLastError();
}

// =================================================================================================
// toneMap (ultrahdr.cpp:517-558): Y8 = (Y16 >> 6 >> 2) & 0xff == bits 15..8 of the P010 word
// =================================================================================================

// luma: grid.y = row, grid.z = image; one thread per 8 (ALIGNED) or 1 destination bytes across [0, dy_stride)
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_luma(const ToneBatch b) {
  const ToneImage& t = b.img[blockIdx.z];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  for (uint32_t row = blockIdx.y; row < t.height; row += gridDim.y) {   // (rows beyond the grid's 65535 by striding)
    const uint16_t* src = t.sy + (size_t)row * t.sy_stride;
    uint8_t* dst = t.dy + (size_t)row * t.dy_stride;
    if (ALIGNED) {
      const uint32_t x = i * 8u;
      if (x >= t.dy_stride) return;
      uint2 o = make_uint2(0u, 0u);
      if (x < t.width) {  // width % 8 == 0 on this path
        const uint4 q = *reinterpret_cast<const uint4*>(src + x);
        o.x = ((q.x >> 8) & 0xffu) | ((q.x >> 24) << 8) | (((q.y >> 8) & 0xffu) << 16) | ((q.y >> 24) << 24);
        o.y = ((q.z >> 8) & 0xffu) | ((q.z >> 24) << 8) | (((q.w >> 8) & 0xffu) << 16) | ((q.w >> 24) << 24);
      }
      *reinterpret_cast<uint2*>(dst + x) = o;
    } else {
      if (i >= t.dy_stride && i >= t.width) return;
      if (i < t.width) dst[i] = (uint8_t)((src[i] >> 6 >> 2) & 0xff);
      else dst[i] = 0;  // memset(dst_y_row + width, 0, luma_stride - width)
    }
  }
}

// chroma: grid.y = chroma row; U and V de-interleaved, padding [width/2, dc_stride) zeroed
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_chroma(const ToneBatch b) {
  const ToneImage& t = b.img[blockIdx.z];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cw = t.width / 2u;
  for (uint32_t row = blockIdx.y; row < t.height / 2u; row += gridDim.y) {
    const uint16_t* src = t.suv + (size_t)row * t.suv_stride;
    uint8_t* du = t.du + (size_t)row * t.dc_stride;
    uint8_t* dv = t.dv + (size_t)row * t.dc_stride;
    if (ALIGNED) {
      const uint32_t x = i * 8u;  // chroma sample index; cw % 8 == 0 on this path
      if (x >= t.dc_stride) return;
      uint2 ou = make_uint2(0u, 0u), ov = make_uint2(0u, 0u);
      if (x < cw) {
        const uint4 a = *reinterpret_cast<const uint4*>(src + 2u * x);
        const uint4 bq = *reinterpret_cast<const uint4*>(src + 2u * x + 8u);
        ou.x = ((a.x >> 8) & 0xffu) | (((a.y >> 8) & 0xffu) << 8) | (((a.z >> 8) & 0xffu) << 16) | (((a.w >> 8) & 0xffu) << 24);
        ov.x = (a.x >> 24) | ((a.y >> 24) << 8) | ((a.z >> 24) << 16) | ((a.w >> 24) << 24);
        ou.y = ((bq.x >> 8) & 0xffu) | (((bq.y >> 8) & 0xffu) << 8) | (((bq.z >> 8) & 0xffu) << 16) | (((bq.w >> 8) & 0xffu) << 24);
        ov.y = (bq.x >> 24) | ((bq.y >> 24) << 8) | ((bq.z >> 24) << 16) | ((bq.w >> 24) << 24);
      }
      *reinterpret_cast<uint2*>(du + x) = ou;
      *reinterpret_cast<uint2*>(dv + x) = ov;
    } else {
      if (i >= t.dc_stride && i >= cw) return;
      if (i < cw) {
        du[i] = (uint8_t)((src[2u * i] >> 6 >> 2) & 0xff);
        dv[i] = (uint8_t)((src[2u * i + 1u] >> 6 >> 2) & 0xff);
      } else {
        du[i] = 0; dv[i] = 0;
      }
    }
  }
}

hipError_t launch_tonemap(const ToneBatch& b, int n, bool aligned, hipStream_t s) {
  const ToneImage& t = b.img[0];
  if (n <= 0 || t.width == 0 || t.height == 0) return hipSuccess;
  // the grid covers the widest destination row of the launch (every thread checks its own image's strides)
  uint32_t lcols = t.width, ccols = t.width / 2u;
  for (int i = 0; i < n; ++i) { lcols = b.img[i].dy_stride > lcols ? b.img[i].dy_stride : lcols; ccols = b.img[i].dc_stride > ccols ? b.img[i].dc_stride : ccols; }
  if (aligned) {
    hipLaunchKernelGGL((k_tonemap_luma<true>), dim3((lcols / 8u + 255u) / 256u, t.height < 65535u ? t.height : 65535u, n), dim3(256), 0, s, b);
    if (t.height / 2u)
      hipLaunchKernelGGL((k_tonemap_chroma<true>), dim3((ccols / 8u + 255u) / 256u, t.height / 2u < 65535u ? t.height / 2u : 65535u, n), dim3(256), 0, s, b);
  } else {
    hipLaunchKernelGGL((k_tonemap_luma<false>), dim3((lcols + 255u) / 256u, t.height < 65535u ? t.height : 65535u, n), dim3(256), 0, s, b);
    if (t.height / 2u && ccols)
      hipLaunchKernelGGL((k_tonemap_chroma<false>), dim3((ccols + 255u) / 256u, t.height / 2u < 65535u ? t.height / 2u : 65535u, n), dim3(256), 0, s, b);
  }
  return hipGetLastError();
}

// =================================================================================================
// convertYuv (jpegr.cpp:1199-1203 over transformYuv420, gainmapmath.cpp:483-520), in place.
// Every 2x2 block reads and writes only its own 4 luma + 1 U + 1 V bytes, so blocks are independent.
// =================================================================================================

struct Yuv { float y, u, v; };
__device__ __forceinline__ Yuv yuv_mat(const float (&m)[9], float y, float u, float v) {
  Yuv o;
  o.y = m[0] * y + m[1] * u + m[2] * v;
  o.u = m[3] * y + m[4] * u + m[5] * v;
  o.v = m[6] * y + m[7] * u + m[8] * v;
  return o;
}
__device__ __forceinline__ uint32_t round_u8(float x) {  // (uint8_t)CLIP3(x, 0, 255), x already + 0.5f
  x = (x < 0.0f) ? 0.0f : (x > 255.0f) ? 255.0f : x;
  return (uint32_t)x;
}
// one 2x2 block; y00..y11 luma bytes, ub/vb chroma bytes.  The kernel is bound by VALU issue, not by its 3 bytes per pixel, so
// the four pixels run as two packed pairs: every float operation below is the reference's own (the products and sums of its yuvXToY
// matrices in their order, gainmapmath.cpp:447-481; the chroma average and the +0.5 / CLIP3 of transformYuv420, :483-520), two at a
// time; the products of the block's single (u, v) with the matrix are formed once.
__device__ __forceinline__ void cvt_block(const float (&m)[9], uint32_t (&yb)[4], uint32_t& ub, uint32_t& vb) {
  const float u = (float)((int)ub - 128) * k255, v = (float)((int)vb - 128) * k255;
  const f2 y01 = (f2){(float)yb[0], (float)yb[1]} * splat(k255), y23 = (f2){(float)yb[2], (float)yb[3]} * splat(k255);
  const float yu = m[1] * u, yv = m[2] * v, uu = m[4] * u, uv = m[5] * v, vu = m[7] * u, vv = m[8] * v;
  const f2 py01 = (splat(m[0]) * y01 + splat(yu)) + splat(yv), py23 = (splat(m[0]) * y23 + splat(yu)) + splat(yv);
  const f2 pu01 = (splat(m[3]) * y01 + splat(uu)) + splat(uv), pu23 = (splat(m[3]) * y23 + splat(uu)) + splat(uv);
  const f2 pv01 = (splat(m[6]) * y01 + splat(vu)) + splat(vv), pv23 = (splat(m[6]) * y23 + splat(vu)) + splat(vv);
  // (((p0 + p1) + p2) + p3) / 4 for u and v side by side
  f2 c = (f2){pu01.x, pv01.x} + (f2){pu01.y, pv01.y};
  c = c + (f2){pu23.x, pv23.x};
  c = c + (f2){pu23.y, pv23.y};
  c = c * splat(0.25f);                                    // == / 4.0f
  c = (c * splat(255.0f) + splat(128.0f)) + splat(0.5f);
  const f2 o01 = py01 * splat(255.0f) + splat(0.5f), o23 = py23 * splat(255.0f) + splat(0.5f);
  // (uint8_t)CLIP3(x, 0, 255): one v_med3_f32 (the same value as the reference's compare chain for every x but NaN, which
  // bytes times a finite matrix cannot produce) and a truncating conversion
  yb[0] = (uint32_t)__builtin_amdgcn_fmed3f(o01.x, 0.0f, 255.0f); yb[1] = (uint32_t)__builtin_amdgcn_fmed3f(o01.y, 0.0f, 255.0f);
  yb[2] = (uint32_t)__builtin_amdgcn_fmed3f(o23.x, 0.0f, 255.0f); yb[3] = (uint32_t)__builtin_amdgcn_fmed3f(o23.y, 0.0f, 255.0f);
  ub = (uint32_t)__builtin_amdgcn_fmed3f(c.x, 0.0f, 255.0f);
  vb = (uint32_t)__builtin_amdgcn_fmed3f(c.y, 0.0f, 255.0f);
}

template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_convert_yuv(const CvtBatch b) {
  const CvtImage& t = b.img[blockIdx.z];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t cw = t.width / 2u;
  for (uint32_t cyr = blockIdx.y; cyr < t.height / 2u; cyr += gridDim.y) {   // chroma row (rows beyond the grid's 65535 by striding)
    uint8_t* y0 = t.y + (size_t)(2u * cyr) * t.y_stride;
    uint8_t* y1 = y0 + t.y_stride;
    uint8_t* ur = t.u + (size_t)cyr * t.c_stride;
    uint8_t* vr = t.v + (size_t)cyr * t.c_stride;
    const uint8_t* sy0 = t.sy + (size_t)(2u * cyr) * t.sy_stride;
    const uint8_t* sy1 = sy0 + t.sy_stride;
    const uint8_t* sur = t.su + (size_t)cyr * t.sc_stride;
    const uint8_t* svr = t.sv + (size_t)cyr * t.sc_stride;
    if (ALIGNED) {  // 4 chroma samples = 8 luma columns per thread; cw % 4 == 0
      const uint32_t cx = i * 4u;
      if (cx >= cw) return;
      uint2 a = *reinterpret_cast<const uint2*>(sy0 + 2u * cx);
      uint2 bq = *reinterpret_cast<const uint2*>(sy1 + 2u * cx);
      uint32_t uw = *reinterpret_cast<const uint32_t*>(sur + cx);
      uint32_t vw = *reinterpret_cast<const uint32_t*>(svr + cx);
      const uint32_t top[2] = {a.x, a.y}, bot[2] = {bq.x, bq.y};
      uint32_t otop[2] = {0u, 0u}, obot[2] = {0u, 0u}, ou = 0u, ov = 0u;
  #pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sh = 16 * (k & 1);
        uint32_t yb[4] = {(top[k >> 1] >> sh) & 0xffu, (top[k >> 1] >> (sh + 8)) & 0xffu,
                          (bot[k >> 1] >> sh) & 0xffu, (bot[k >> 1] >> (sh + 8)) & 0xffu};
        uint32_t ub = (uw >> (8 * k)) & 0xffu, vb = (vw >> (8 * k)) & 0xffu;
        cvt_block(b.img[0].m, yb, ub, vb);
        otop[k >> 1] |= (yb[0] << sh) | (yb[1] << (sh + 8));
        obot[k >> 1] |= (yb[2] << sh) | (yb[3] << (sh + 8));
        ou |= ub << (8 * k); ov |= vb << (8 * k);
      }
      *reinterpret_cast<uint2*>(y0 + 2u * cx) = make_uint2(otop[0], otop[1]);
      *reinterpret_cast<uint2*>(y1 + 2u * cx) = make_uint2(obot[0], obot[1]);
      *reinterpret_cast<uint32_t*>(ur + cx) = ou;
      *reinterpret_cast<uint32_t*>(vr + cx) = ov;
    } else {
      if (i >= cw) return;
      uint32_t yb[4] = {sy0[2u * i], sy0[2u * i + 1u], sy1[2u * i], sy1[2u * i + 1u]};
      uint32_t ub = sur[i], vb = svr[i];
      cvt_block(b.img[0].m, yb, ub, vb);
      y0[2u * i] = (uint8_t)yb[0]; y0[2u * i + 1u] = (uint8_t)yb[1];
      y1[2u * i] = (uint8_t)yb[2]; y1[2u * i + 1u] = (uint8_t)yb[3];
      ur[i] = (uint8_t)ub; vr[i] = (uint8_t)vb;
    }
  }
}

hipError_t launch_convert_yuv(const CvtBatch& b, int n, bool aligned, hipStream_t s) {
  const uint32_t cw = b.img[0].width / 2u, ch = b.img[0].height / 2u;
  if (n <= 0 || cw == 0 || ch == 0) return hipSuccess;
  const uint32_t rows = ch < 65535u ? ch : 65535u;
  if (aligned) hipLaunchKernelGGL((k_convert_yuv<true>), dim3((cw / 4u + 255u) / 256u, rows, n), dim3(256), 0, s, b);
  else hipLaunchKernelGGL((k_convert_yuv<false>), dim3((cw + 255u) / 256u, rows, n), dim3(256), 0, s, b);
  return hipGetLastError();
}

// =================================================================================================
// Tone-mapped SDR base image for encodeJPEGR API-0 (no reference counterpart): P010 -> linear light with
// generate's exact inverse OETFs -> extended Reinhard on the maximum channel against the image's headroom H -> sRGB OETF -> 8-bit
// YUV420 in the HDR image's gamut, quantised like transformYuv420 (gainmapmath.cpp:513-519).
//   k_tonemap_head_init    headroom[i] = 0 (H is measured) or the given H
//   k_tonemap_peak         measured images only: max over pixels and channels of the clamped gamma-domain r', g', b' -- the matrix
//                          alone, no special function: the inverse OETFs are monotone, so the largest r' is the largest linear value
//   k_tonemap_head_finish  measured slots from m' to H = min(max(invOETF(m') * k, 1), cap)
//   k_tonemap_sdr          the planes
// A lane owns whole 2x2 blocks (ALIGNED: eight of them, 2 rows x 16 columns, read and written as 16-byte pieces; otherwise one), so
// every P010 chroma sample is read once and the four pixels' output chroma is averaged in registers.
// =================================================================================================

// getP010Pixel (gainmapmath.cpp:583-601) of one 16-bit word
__device__ __forceinline__ float p010_luma(uint32_t w) { return (float)((int)(w >> 6) - 64) * k876; }
__device__ __forceinline__ float p010_chroma(uint32_t w) { return (float)((int)(w >> 6) - 64) * k896 - 0.5f; }
// <gamut>YuvToRgb (gainmapmath.cpp:142-146, :198-202, :250-254): the reference's operations in its order, clamped as it clamps
__device__ __forceinline__ void tone_rgb(const ToneSdrConsts& c, float y, float u, float v, float& r, float& g, float& b) {
  r = clamp01(y + c.cr * v);
  g = clamp01(y - c.gcb * u - c.gcr * v);
  b = clamp01(y + c.cb * u);
}
__device__ __forceinline__ float tone_block_max(const ToneSdrConsts& c, const uint32_t (&yw)[4], uint32_t uw, uint32_t vw) {
  const float u = p010_chroma(uw), v = p010_chroma(vw);
  float m = 0.0f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float r, g, b;
    tone_rgb(c, p010_luma(yw[p]), u, v, r, g, b);
    m = fmaxf(m, fmaxf(r, fmaxf(g, b)));
  }
  return m;
}

// sRGB OETF on the special-function unit: o^(1/2.4) = 2^(log2(o) / 2.4), |log2 o| <= 8.4 on the branch that uses it, so v_log_f32's
// and v_exp_f32's errors leave the result within ~1e-6 relative: 3e-4 of an 8-bit code
__device__ __forceinline__ float srgb_oetf_fast(float o) {
  const float lo = 12.92f * o;
  const float hi = 1.055f * __builtin_amdgcn_exp2f((1.0f / 2.4f) * __builtin_amdgcn_logf(o)) - 0.055f;
  return (o <= 0.0031308f) ? lo : hi;
}

// one 2x2 block: yw[0..3] the P010 luma words of (0,0) (0,1) (1,0) (1,1), uw / vw its chroma words; ihh = 1 / (H * H).
// Returns the four luma bytes in yo, the block's chroma bytes in uo / vo.
template <int TF>
__device__ __forceinline__ void tone_block(const ToneSdrConsts& c, float ihh, const uint32_t (&yw)[4], uint32_t uw, uint32_t vw,
                                           uint32_t (&yo)[4], uint32_t& uo, uint32_t& vo) {
  const float u = p010_chroma(uw), v = p010_chroma(vw);
  float ch[12];
#pragma unroll
  for (int p = 0; p < 4; ++p) tone_rgb(c, p010_luma(yw[p]), u, v, ch[3 * p], ch[3 * p + 1], ch[3 * p + 2]);
  if (TF != 0) {   // generate's exact inverse OETFs, six evaluations in lock step (see gen_pair)
#pragma unroll
    for (int i = 0; i < 12; i += 6) {
      float part[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) part[j] = ch[i + j];
      if (TF == 1) hlg_inv_oetf_guarded_n<6>(part);
      else pq_inv_oetf_guarded_n<6>(part);
#pragma unroll
      for (int j = 0; j < 6; ++j) ch[i + j] = part[j];
    }
  }
  float su = 0.0f, sv = 0.0f;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float vr = ch[3 * p] * c.k, vg = ch[3 * p + 1] * c.k, vb = ch[3 * p + 2] * c.k;   // SDR-white-relative
    const float M = fmaxf(vr, fmaxf(vg, vb));
    const float s = (M > 0.0f) ? (1.0f + M * ihh) * __builtin_amdgcn_rcpf(1.0f + M) : 1.0f;
    const float er = srgb_oetf_fast(clamp01(vr * s)), eg = srgb_oetf_fast(clamp01(vg * s)), eb = srgb_oetf_fast(clamp01(vb * s));
    const float y = c.lr * er + c.lg * eg + c.lb * eb;
    const float pu = div_const(eb - y, c.ycb, c.rycb), pv = div_const(er - y, c.ycr, c.rycr);
    yo[p] = round_u8(y * 255.0f + 0.5f);
    su = (p == 0) ? pu : su + pu;   // ((u00 + u01) + u10) + u11
    sv = (p == 0) ? pv : sv + pv;
  }
  uo = round_u8(((su * 0.25f) * 255.0f + 128.0f) + 0.5f);
  vo = round_u8(((sv * 0.25f) * 255.0f + 128.0f) + 0.5f);
}

__global__ void __launch_bounds__(256) k_tonemap_head_init(float* headroom, const ToneHeadInit v, int n) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) headroom[i] = v.h[i];
}
hipError_t launch_tonemap_head_init(float* headroom, const ToneHeadInit& v, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kToneHeadChunk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tonemap_head_init, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, headroom, v, n);
  return hipGetLastError();
}
template <int TF>
__global__ void __launch_bounds__(256) k_tonemap_head_finish(float* headroom, const ToneHeadInit v, int n, float k, float cap) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n && v.h[i] == 0.0f) headroom[i] = fminf(fmaxf(hdr_inv_oetf<TF>(headroom[i]) * k, 1.0f), cap);
}
hipError_t launch_tonemap_head_finish(float* headroom, const ToneHeadInit& v, int n, int hdr_tf, float k, float cap, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kToneHeadChunk) return hipErrorInvalidValue;
  const dim3 grid(((unsigned)n + 255u) / 256u), block(256);
  if (hdr_tf == 1) hipLaunchKernelGGL((k_tonemap_head_finish<1>), grid, block, 0, s, headroom, v, n, k, cap);
  else if (hdr_tf == 2) hipLaunchKernelGGL((k_tonemap_head_finish<2>), grid, block, 0, s, headroom, v, n, k, cap);
  else hipLaunchKernelGGL((k_tonemap_head_finish<0>), grid, block, 0, s, headroom, v, n, k, cap);
  return hipGetLastError();
}

// the 16-bit word `k` (0 .. 7) of a 16-byte piece
__device__ __forceinline__ uint32_t word_of(const uint4& q, int k) {
  const uint32_t d = (k >> 1) == 0 ? q.x : (k >> 1) == 1 ? q.y : (k >> 1) == 2 ? q.z : q.w;
  return (k & 1) ? d >> 16 : d & 0xffffu;
}

// grid.x: the lanes' columns, grid.y: block rows (strided), grid.z: image.  One atomicMax per workgroup, on the bit pattern: the
// values are non-negative floats, which order as unsigned integers.
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_peak(const ToneSdrConsts c, const ToneBatch b) {
  const ToneImage& t = b.img[blockIdx.z];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  float m = 0.0f;
  for (uint32_t cyr = blockIdx.y; cyr < t.height / 2u; cyr += gridDim.y) {
    const uint16_t* y0 = t.sy + (size_t)(2u * cyr) * t.sy_stride;
    const uint16_t* y1 = y0 + t.sy_stride;
    const uint16_t* uv = t.suv + (size_t)cyr * t.suv_stride;
    if (ALIGNED) {   // width % 16 == 0
      const uint32_t x = i * 16u;
      if (x < t.width) {   // plain loads: a frame that fits the caches is still there for k_tonemap_sdr
        const uint4 a0 = *reinterpret_cast<const uint4*>(y0 + x), a1 = *reinterpret_cast<const uint4*>(y0 + x + 8u);
        const uint4 b0 = *reinterpret_cast<const uint4*>(y1 + x), b1 = *reinterpret_cast<const uint4*>(y1 + x + 8u);
        const uint4 c0 = *reinterpret_cast<const uint4*>(uv + x), c1 = *reinterpret_cast<const uint4*>(uv + x + 8u);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint4& ta = k < 4 ? a0 : a1;
          const uint4& tb = k < 4 ? b0 : b1;
          const uint4& tc = k < 4 ? c0 : c1;
          const int w = 2 * (k & 3);
          const uint32_t yw[4] = {word_of(ta, w), word_of(ta, w + 1), word_of(tb, w), word_of(tb, w + 1)};
          m = fmaxf(m, tone_block_max(c, yw, word_of(tc, w), word_of(tc, w + 1)));
        }
      }
    } else {
      const uint32_t x = i * 2u;
      if (x < t.width) {   // width is even
        const uint32_t yw[4] = {ld16(y0 + x), ld16(y0 + x + 1u), ld16(y1 + x), ld16(y1 + x + 1u)};
        m = fmaxf(m, tone_block_max(c, yw, ld16(uv + x), ld16(uv + x + 1u)));
      }
    }
  }
  __shared__ float s_part[4];
  m = wave_extreme<true>(m);   // (all 64 lanes are active here)
  if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const uint32_t key = __float_as_uint(fmaxf(fmaxf(s_part[0], s_part[1]), fmaxf(s_part[2], s_part[3])));
    uint32_t* slot = reinterpret_cast<uint32_t*>(c.headroom + c.slot[blockIdx.z]);
    // a stale (smaller) value read here only costs an unnecessary atomic, never a lost update
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
  }
}

// the grid of both kernels: lanes across the widest row they touch, block rows down (strided beyond max_rows)
static dim3 tone_sdr_grid(const ToneBatch& b, int n, bool aligned, bool dest, uint32_t max_rows) {
  const ToneImage& t = b.img[0];
  uint32_t lanes = aligned ? t.width / 16u : t.width / 2u;
  if (dest)
    for (int i = 0; i < n; ++i) {
      const uint32_t l = aligned ? b.img[i].dy_stride / 16u : (b.img[i].dy_stride + 1u) / 2u;
      const uint32_t cl = aligned ? b.img[i].dc_stride / 8u : b.img[i].dc_stride;
      lanes = std::max(lanes, std::max(l, cl));
    }
  return dim3((lanes + 255u) / 256u, std::min(t.height / 2u, max_rows), (unsigned)n);
}

hipError_t launch_tonemap_peak(const ToneSdrConsts& c, const ToneBatch& b, int n, bool aligned, hipStream_t s) {
  const ToneImage& t = b.img[0];
  if (n <= 0 || t.width < 2u || t.height < 2u) return hipSuccess;
  if (n > kToneChunk) return hipErrorInvalidValue;
  // one atomic per workgroup: enough workgroups to fill the device (~4096 per launch), no more than 512 per image
  dim3 grid = tone_sdr_grid(b, n, aligned, false, 65535u);
  const uint32_t rows = std::min(std::max(4096u / (grid.x * (uint32_t)n), 32u), 512u);
  grid.y = std::min(grid.y, rows);
  if (aligned) hipLaunchKernelGGL((k_tonemap_peak<true>), grid, dim3(256), 0, s, c, b);
  else hipLaunchKernelGGL((k_tonemap_peak<false>), grid, dim3(256), 0, s, c, b);
  return hipGetLastError();
}

// ALIGNED: width % 16 == 0; sources 16-byte aligned with strides of whole 16-byte pieces; dy 16-byte aligned, dy_stride % 16 == 0;
// du, dv 8-byte aligned, dc_stride % 8 == 0.  Either way width and height are even, dy_stride >= width, dc_stride >= width / 2, and
// the padding columns [width, dy_stride) and [width / 2, dc_stride) are zeroed like toneMap's.
template <int TF, bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_sdr(const ToneSdrConsts c, const ToneBatch b) {
  const ToneImage& t = b.img[blockIdx.z];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const float H = c.headroom[c.slot[blockIdx.z]];   // (wave-uniform: scalar loads)
  const float ihh = 1.0f / (H * H);
  const uint32_t cw = t.width / 2u;
  for (uint32_t cyr = blockIdx.y; cyr < t.height / 2u; cyr += gridDim.y) {   // (rows beyond the grid's 65535 by striding)
    const uint16_t* y0 = t.sy + (size_t)(2u * cyr) * t.sy_stride;
    const uint16_t* y1 = y0 + t.sy_stride;
    const uint16_t* uv = t.suv + (size_t)cyr * t.suv_stride;
    uint8_t* d0 = t.dy + (size_t)(2u * cyr) * t.dy_stride;
    uint8_t* d1 = d0 + t.dy_stride;
    uint8_t* du = t.du + (size_t)cyr * t.dc_stride;
    uint8_t* dv = t.dv + (size_t)cyr * t.dc_stride;
    if (ALIGNED) {
      const uint32_t x = i * 16u, cx = i * 8u;
      uint32_t ot[4] = {0u, 0u, 0u, 0u}, ob[4] = {0u, 0u, 0u, 0u}, ou[2] = {0u, 0u}, ov[2] = {0u, 0u};
      if (x < t.width) {
        const uint4 a0 = ld_stream(reinterpret_cast<const uint4*>(y0 + x)), a1 = ld_stream(reinterpret_cast<const uint4*>(y0 + x + 8u));
        const uint4 b0 = ld_stream(reinterpret_cast<const uint4*>(y1 + x)), b1 = ld_stream(reinterpret_cast<const uint4*>(y1 + x + 8u));
        const uint4 c0 = ld_stream(reinterpret_cast<const uint4*>(uv + x)), c1 = ld_stream(reinterpret_cast<const uint4*>(uv + x + 8u));
        // one block (a dword of either luma row and of the chroma row) per trip; the loop stays rolled -- the transfer functions are
        // long -- and the pieces are handed down by register moves, so that nothing is indexed at run time
        uint32_t top[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bot[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        uint32_t chr[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll 1
        for (int trip = 0; trip < 8; ++trip) {
          const uint32_t yw[4] = {top[0] & 0xffffu, top[0] >> 16, bot[0] & 0xffffu, bot[0] >> 16};
          uint32_t yo[4], uo, vo;
          tone_block<TF>(c, ihh, yw, chr[0] & 0xffffu, chr[0] >> 16, yo, uo, vo);
#pragma unroll
          for (int k = 0; k < 7; ++k) { top[k] = top[k + 1]; bot[k] = bot[k + 1]; chr[k] = chr[k + 1]; }
          // the new bytes enter at the top of the 128-bit (luma) and 64-bit (chroma) pieces, which move down: trip 0 ends up lowest
#pragma unroll
          for (int k = 0; k < 3; ++k) { ot[k] = (ot[k] >> 16) | (ot[k + 1] << 16); ob[k] = (ob[k] >> 16) | (ob[k + 1] << 16); }
          ot[3] = (ot[3] >> 16) | ((yo[0] | (yo[1] << 8)) << 16);
          ob[3] = (ob[3] >> 16) | ((yo[2] | (yo[3] << 8)) << 16);
          ou[0] = (ou[0] >> 8) | (ou[1] << 24); ou[1] = (ou[1] >> 8) | (uo << 24);
          ov[0] = (ov[0] >> 8) | (ov[1] << 24); ov[1] = (ov[1] >> 8) | (vo << 24);
        }
      }
      if (x < t.dy_stride) {
        st_stream(reinterpret_cast<uint4*>(d0 + x), make_uint4(ot[0], ot[1], ot[2], ot[3]));
        st_stream(reinterpret_cast<uint4*>(d1 + x), make_uint4(ob[0], ob[1], ob[2], ob[3]));
      }
      if (cx < t.dc_stride) {
        st_stream(reinterpret_cast<uint2*>(du + cx), make_uint2(ou[0], ou[1]));
        st_stream(reinterpret_cast<uint2*>(dv + cx), make_uint2(ov[0], ov[1]));
      }
    } else {
      const uint32_t x = i * 2u;
      if (i < cw) {
        const uint32_t yw[4] = {ld16(y0 + x), ld16(y0 + x + 1u), ld16(y1 + x), ld16(y1 + x + 1u)};
        uint32_t yo[4], uo, vo;
        tone_block<TF>(c, ihh, yw, ld16(uv + x), ld16(uv + x + 1u), yo, uo, vo);
        d0[x] = (uint8_t)yo[0]; d0[x + 1u] = (uint8_t)yo[1];
        d1[x] = (uint8_t)yo[2]; d1[x + 1u] = (uint8_t)yo[3];
        du[i] = (uint8_t)uo; dv[i] = (uint8_t)vo;
      } else {
        if (x < t.dy_stride) { d0[x] = 0; d1[x] = 0; }
        if (x + 1u < t.dy_stride) { d0[x + 1u] = 0; d1[x + 1u] = 0; }
        if (i < t.dc_stride) { du[i] = 0; dv[i] = 0; }
      }
    }
  }
}

hipError_t launch_tonemap_sdr(const ToneSdrConsts& c, const ToneBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s) {
  const ToneImage& t = b.img[0];
  if (n <= 0 || t.width < 2u || t.height < 2u) return hipSuccess;
  if (n > kToneChunk) return hipErrorInvalidValue;
  const dim3 grid = tone_sdr_grid(b, n, aligned, true, 65535u), block(256);
#define UHDR_TONE_SDR(TF)                                                                            \
  do {                                                                                               \
    if (aligned) hipLaunchKernelGGL((k_tonemap_sdr<TF, true>), grid, block, 0, s, c, b);            \
    else hipLaunchKernelGGL((k_tonemap_sdr<TF, false>), grid, block, 0, s, c, b);                   \
  } while (0)
  if (hdr_tf == 1) UHDR_TONE_SDR(1);
  else if (hdr_tf == 2) UHDR_TONE_SDR(2);
  else UHDR_TONE_SDR(0);
#undef UHDR_TONE_SDR
  return hipGetLastError();
}

// =================================================================================================
// Tone-mapped SDR image from a packed HDR image (no reference counterpart): RGBA1010102 / RGBA F16 ->
// linear light -> the operator of k_tonemap_sdr (extended Reinhard on the maximum channel against H, sRGB OETF) -> RGBA8888.
//   k_build_packed_tone_tables  once per device: generate's exact inverse OETFs of the 1024 codes, HLG then PQ
//   k_tonemap_packed_peak       measured images only: the maximum of the clamped pixel values into the image's headroom slot
//   k_tonemap_packed            the pixels; an RGBA1010102 channel is linearised by one LDS read of the block's copy of the table
// k_tonemap_head_init / k_tonemap_head_finish serve both operators unchanged.  A block is 64 x 4 threads: a wave walks along one
// row (ALIGNED: a lane owns a 16-byte piece of the destination, 4 pixels; otherwise one pixel), the block's rows stride by the grid.
// =================================================================================================
__global__ void __launch_bounds__(256) k_build_packed_tone_tables(float* tab) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // 2 x 1024 entries
  const float e = (float)(i & 1023u) * k1023;
  tab[i] = (i < 1024u) ? hdr_inv_oetf<1>(e) : hdr_inv_oetf<2>(e);
}
hipError_t launch_build_packed_tone_tables(float* tab, hipStream_t s) {
  hipLaunchKernelGGL(k_build_packed_tone_tables, dim3(2u * kTonePackedCodes / 256u), dim3(256), 0, s, tab);
  return hipGetLastError();
}

// step 1's clamp: -0, negative and NaN halves give 0, halves above 1.0 (infinity included) give 1
__device__ __forceinline__ float clamp01_nan(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ uint32_t max_code10(uint32_t p) { return max(p & 0x3ffu, max((p >> 10) & 0x3ffu, (p >> 20) & 0x3ffu)); }
__device__ __forceinline__ float max_half3(uint32_t rg, uint32_t ba) {
  return fmaxf(clamp01_nan(half_lo(rg)), fmaxf(clamp01_nan(half_hi(rg)), clamp01_nan(half_lo(ba))));
}

// grid.x: the lanes' columns, grid.y: groups of 4 rows (strided), grid.z: image.  RGBA1010102: an integer maximum of the codes,
// converted once.  The hand-over is k_tonemap_peak's: one atomicMax per workgroup on the bit pattern of a non-negative float.
template <bool F16, bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_packed_peak(const TonePackedBatch b) {
  const TonePackedImage& t = b.img[blockIdx.z];
  const uint32_t col = blockIdx.x * 64u + threadIdx.x, cols = ALIGNED ? t.width / 4u : t.width;
  const uint32_t step = gridDim.y * 4u;
  uint32_t mc = 0u;
  float m = 0.0f;
  if (col < cols) {
    for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < t.height; y += step) {   // plain loads: see k_tonemap_peak
      if (F16) {
        const uint2* row = static_cast<const uint2*>(t.src) + (size_t)y * t.src_stride;
        if (ALIGNED) {
          const uint4 a = *reinterpret_cast<const uint4*>(row + 4u * col), c = *reinterpret_cast<const uint4*>(row + 4u * col + 2u);
          m = fmaxf(fmaxf(m, fmaxf(max_half3(a.x, a.y), max_half3(a.z, a.w))), fmaxf(max_half3(c.x, c.y), max_half3(c.z, c.w)));
        } else {
          const uint2 p = row[col];
          m = fmaxf(m, max_half3(p.x, p.y));
        }
      } else {
        const uint32_t* row = static_cast<const uint32_t*>(t.src) + (size_t)y * t.src_stride;
        if (ALIGNED) {
          const uint4 a = *reinterpret_cast<const uint4*>(row + 4u * col);
          mc = max(max(mc, max(max_code10(a.x), max_code10(a.y))), max(max_code10(a.z), max_code10(a.w)));
        } else {
          mc = max(mc, max_code10(row[col]));
        }
      }
      if (t.height - y <= step) break;   // (y + step may not wrap)
    }
  }
  if (!F16) m = (float)mc * k1023;
  __shared__ float s_part[4];
  m = wave_extreme<true>(m);   // (all 64 lanes are active here)
  if (threadIdx.x == 0u) s_part[threadIdx.y] = m;
  __syncthreads();
  if (threadIdx.x == 0u && threadIdx.y == 0u) {
    const uint32_t key = __float_as_uint(fmaxf(fmaxf(s_part[0], s_part[1]), fmaxf(s_part[2], s_part[3])));
    uint32_t* slot = reinterpret_cast<uint32_t*>(b.headroom + b.slot[blockIdx.z]);
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot, key);
  }
}

// steps 3 and 5 of the operator on one pixel's linear channels: k_tonemap_sdr's arithmetic (tone_block), then the bytes
__device__ __forceinline__ uint32_t tone_packed_pixel(float r, float g, float bl, float k, float ihh) {
  const float vr = r * k, vg = g * k, vb = bl * k;
  const float M = fmaxf(vr, fmaxf(vg, vb));
  const float s = (M > 0.0f) ? (1.0f + M * ihh) * __builtin_amdgcn_rcpf(1.0f + M) : 1.0f;
  const uint32_t R = round_u8(srgb_oetf_fast(clamp01(vr * s)) * 255.0f + 0.5f);
  const uint32_t G = round_u8(srgb_oetf_fast(clamp01(vg * s)) * 255.0f + 0.5f);
  const uint32_t B = round_u8(srgb_oetf_fast(clamp01(vb * s)) * 255.0f + 0.5f);
  return R | (G << 8) | (B << 16) | 0xFF000000u;
}
__device__ __forceinline__ uint32_t tone_packed_1010102(const float* s_tab, uint32_t p, float k, float ihh) {
  return tone_packed_pixel(s_tab[p & 0x3ffu], s_tab[(p >> 10) & 0x3ffu], s_tab[(p >> 20) & 0x3ffu], k, ihh);
}
__device__ __forceinline__ uint32_t tone_packed_f16(uint32_t rg, uint32_t ba, float k, float ihh) {
  return tone_packed_pixel(clamp01_nan(half_lo(rg)), clamp01_nan(half_hi(rg)), clamp01_nan(half_lo(ba)), k, ihh);
}

// ALIGNED: width % 4 == 0, source and destination rows start on 16 bytes.  The columns [width, dst_stride) are not written.
template <int TF, bool F16, bool ALIGNED>
__global__ void __launch_bounds__(256) k_tonemap_packed(const TonePackedBatch b) {
  static_assert(F16 ? TF == 0 : TF != 0, "F16 is linear light, RGBA1010102 carries HLG or PQ");
  __shared__ float s_tab[F16 ? 4 : kTonePackedCodes];
  if (!F16) {   // 256 threads x 16 bytes: the whole table
    const uint32_t tid = threadIdx.y * 64u + threadIdx.x;
    reinterpret_cast<uint4*>(s_tab)[tid] = reinterpret_cast<const uint4*>(b.table)[tid];
    __syncthreads();
  }
  const TonePackedImage& t = b.img[blockIdx.z];
  const uint32_t col = blockIdx.x * 64u + threadIdx.x, cols = ALIGNED ? t.width / 4u : t.width;
  if (col >= cols) return;
  const float H = b.headroom[b.slot[blockIdx.z]];   // (wave-uniform: scalar loads)
  const float ihh = 1.0f / (H * H), k = b.k;
  const uint32_t step = gridDim.y * 4u;
  for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < t.height; y += step) {
    uint32_t* drow = t.dst + (size_t)y * t.dst_stride;
    if (F16) {
      const uint2* row = static_cast<const uint2*>(t.src) + (size_t)y * t.src_stride;
      if (ALIGNED) {
        const uint4 a = ld_stream(reinterpret_cast<const uint4*>(row + 4u * col)), c = ld_stream(reinterpret_cast<const uint4*>(row + 4u * col + 2u));
        st_stream(reinterpret_cast<uint4*>(drow + 4u * col), make_uint4(tone_packed_f16(a.x, a.y, k, ihh), tone_packed_f16(a.z, a.w, k, ihh),
                                                                         tone_packed_f16(c.x, c.y, k, ihh), tone_packed_f16(c.z, c.w, k, ihh)));
      } else {
        const uint2 p = ld_stream(row + col);
        drow[col] = tone_packed_f16(p.x, p.y, k, ihh);
      }
    } else {
      const uint32_t* row = static_cast<const uint32_t*>(t.src) + (size_t)y * t.src_stride;
      if (ALIGNED) {
        const uint4 a = ld_stream(reinterpret_cast<const uint4*>(row + 4u * col));
        st_stream(reinterpret_cast<uint4*>(drow + 4u * col), make_uint4(tone_packed_1010102(s_tab, a.x, k, ihh), tone_packed_1010102(s_tab, a.y, k, ihh),
                                                                         tone_packed_1010102(s_tab, a.z, k, ihh), tone_packed_1010102(s_tab, a.w, k, ihh)));
      } else {
        drow[col] = tone_packed_1010102(s_tab, ld_stream(row + col), k, ihh);
      }
    }
    if (t.height - y <= step) break;   // (y + step may not wrap)
  }
}

// lanes across the row, groups of 4 rows down: about `blocks` workgroups per launch, between lo and hi groups per image
static dim3 tone_packed_grid(const TonePackedBatch& b, int n, bool aligned, uint32_t blocks, uint32_t lo, uint32_t hi) {
  const TonePackedImage& t = b.img[0];
  const uint32_t gx = ((aligned ? t.width / 4u : t.width) + 63u) / 64u, groups = (t.height + 3u) / 4u;
  return dim3(gx, std::min(groups, std::min(std::max(blocks / (gx * (uint32_t)n), lo), hi)), (unsigned)n);
}
hipError_t launch_tonemap_packed_peak(const TonePackedBatch& b, int n, bool f16, bool aligned, hipStream_t s) {
  const TonePackedImage& t = b.img[0];
  if (n <= 0 || t.width == 0u || t.height == 0u) return hipSuccess;
  if (n > kToneChunk) return hipErrorInvalidValue;
  // one atomic per workgroup: no more than kTonePackedPeakGroups workgroup rows per image (1080 rows are 270 groups: strided)
  const dim3 grid = tone_packed_grid(b, n, aligned, 4096u, 16u, kTonePackedPeakGroups), block(64, 4);
  if (f16) {
    if (aligned) hipLaunchKernelGGL((k_tonemap_packed_peak<true, true>), grid, block, 0, s, b);
    else hipLaunchKernelGGL((k_tonemap_packed_peak<true, false>), grid, block, 0, s, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_tonemap_packed_peak<false, true>), grid, block, 0, s, b);
    else hipLaunchKernelGGL((k_tonemap_packed_peak<false, false>), grid, block, 0, s, b);
  }
  return hipGetLastError();
}
hipError_t launch_tonemap_packed(const TonePackedBatch& b, int n, int hdr_tf, bool aligned, hipStream_t s) {
  const TonePackedImage& t = b.img[0];
  if (n <= 0 || t.width == 0u || t.height == 0u) return hipSuccess;
  if (n > kToneChunk || hdr_tf < 0 || hdr_tf > 2) return hipErrorInvalidValue;
  // every block copies the 4 KiB table first: enough rows per block to make that small beside its pixels
  const dim3 grid = tone_packed_grid(b, n, aligned, 2048u, 16u, 1024u), block(64, 4);
  if (hdr_tf == 1) {
    if (aligned) hipLaunchKernelGGL((k_tonemap_packed<1, false, true>), grid, block, 0, s, b);
    else hipLaunchKernelGGL((k_tonemap_packed<1, false, false>), grid, block, 0, s, b);
  } else if (hdr_tf == 2) {
    if (aligned) hipLaunchKernelGGL((k_tonemap_packed<2, false, true>), grid, block, 0, s, b);
    else hipLaunchKernelGGL((k_tonemap_packed<2, false, false>), grid, block, 0, s, b);
  } else {
    if (aligned) hipLaunchKernelGGL((k_tonemap_packed<0, true, true>), grid, block, 0, s, b);
    else hipLaunchKernelGGL((k_tonemap_packed<0, true, false>), grid, block, 0, s, b);
  }
  return hipGetLastError();
}

// =================================================================================================
// editorhelper effects (ref lib/src/editorhelper.cpp:26-360): pure byte gathers.  One thread produces 4
// consecutive output bytes of one plane row (one dword store when the row is aligned), grid.z = plane job.
// =================================================================================================
__device__ __forceinline__ size_t fx_src_index(const FxJob& j, uint32_t i, uint32_t c) {
  switch (j.op) {
    case FX_FLIP_V: return (size_t)(j.rows - i - 1u) * j.src_stride + c;
    case FX_FLIP_H: return (size_t)i * j.src_stride + (j.in_w - c - 1u);
    case FX_ROT90: return (size_t)(j.in_h - c - 1u) * j.src_stride + i;
    case FX_ROT180: return (size_t)(j.in_h - i - 1u) * j.src_stride + (j.in_w - c - 1u);
    case FX_ROT270: return (size_t)c * j.src_stride + (j.in_w - i - 1u);
    case FX_RESIZE: return ((size_t)i * j.row_num / j.row_den) * j.src_stride + (size_t)c * j.col_num / j.col_den;
    default: return (size_t)i * j.src_stride + c;  // FX_COPY
  }
}

// 4 output bytes at column c0 of output row i, gathered one by one (any operation, any alignment)
__device__ __forceinline__ void fx_quad(const FxJob& j, uint32_t i, uint32_t c0, uint8_t* d) {
  if (c0 + 4u <= j.cols && ((reinterpret_cast<uintptr_t>(d) & 3u) == 0u)) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v |= (uint32_t)j.src[fx_src_index(j, i, c0 + k)] << (8 * k);
    *reinterpret_cast<uint32_t*>(d) = v;
  } else {
    for (uint32_t k = 0; k < 4u && c0 + k < j.cols; ++k) d[k] = j.src[fx_src_index(j, i, c0 + k)];
  }
}
__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_amdgcn_perm(v, v, 0x00010203u); }

// One thread produces 16 consecutive output bytes of one plane row.  Copies, flips and the half turn move whole 16-byte pieces
// when both sides are aligned (the mirrored ones with their bytes reversed: four v_perm_b32); resize gathers from a copy of the
// source stretch in LDS.
__global__ void __launch_bounds__(256) k_effect(const FxJobs jobs) {
  const FxJob& j = jobs.job[blockIdx.z];
  const uint32_t cb = blockIdx.x * 4096u;                 // the block's first output column
  if (cb >= j.cols) return;                               // (block-uniform)
  const uint32_t c0 = cb + threadIdx.x * 16u;
  const bool active = c0 < j.cols;
  // resize, at most 4 source bytes per output byte: the block's stretch of the source row is copied into LDS with dword loads and
  // gathered from there (16 byte loads per thread made the kernel load-instruction bound: 44 us for a 4K -> 5760x3240 resize)
  __shared__ uint32_t s_row[(4096u * 4u + 16u) / 4u];
  const bool lds_resize = j.op == FX_RESIZE && j.col_num <= 4u * j.col_den && (uint64_t)j.rows * j.row_num < (1ull << 32) &&
                          (uint64_t)j.cols * j.col_num < (1ull << 32);
  for (uint32_t i = blockIdx.y; i < j.rows; i += gridDim.y) {   // (rows beyond the grid's 65535 by striding)
    uint8_t* d = j.dst + (size_t)i * j.dst_stride + c0;
    const bool whole = active && c0 + 16u <= j.cols && (reinterpret_cast<uintptr_t>(d) & 15u) == 0u;
    if (lds_resize) {
      const uint8_t* srow = j.src + (size_t)(i * j.row_num / j.row_den) * j.src_stride;
      const uint32_t c_last = min(cb + 4095u, j.cols - 1u);
      const uint32_t s_lo = cb * j.col_num / j.col_den, s_hi = min(c_last * j.col_num / j.col_den, j.in_w - 1u);
      const uint8_t* first = srow + s_lo;
      const uint32_t off0 = (uint32_t)(reinterpret_cast<uintptr_t>(first) & 3u);
      const uint8_t* p_al = first - off0;
      const uint32_t nbytes = s_hi - s_lo + 1u + off0;
      const uint8_t* row_end = srow + j.in_w;
      __syncthreads();                                      // (the previous row's gathers are done)
      for (uint32_t k = threadIdx.x; k < (nbytes + 3u) / 4u; k += 256u) {
        const uint8_t* p = p_al + 4u * k;
        uint32_t v;
        if (p >= srow && p + 4 <= row_end) v = *reinterpret_cast<const uint32_t*>(p);
        else {                                              // the row's first / last bytes: never read outside [srow, row_end)
          v = 0;
          for (int b = 0; b < 4; ++b) if (p + b >= srow && p + b < row_end) v |= (uint32_t)p[b] << (8 * b);
        }
        s_row[k] = v;
      }
      __syncthreads();
      if (active) {
        const uint8_t* lrow = reinterpret_cast<const uint8_t*>(s_row) + off0;
        const uint32_t step = j.col_num / j.col_den, rem = j.col_num - step * j.col_den;
        const uint32_t p0 = c0 * j.col_num;
        uint32_t q = p0 / j.col_den, r = p0 - q * j.col_den;
        q -= s_lo;
        if (whole) {
          uint32_t w[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              v |= (uint32_t)lrow[q] << (8 * k);
              q += step; r += rem;
              if (r >= j.col_den) { r -= j.col_den; ++q; }
            }
            w[g] = v;
          }
          *reinterpret_cast<uint4*>(d) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
          for (uint32_t k = 0; k < 16u && c0 + k < j.cols; ++k) {
            d[k] = lrow[q];
            q += step; r += rem;
            if (r >= j.col_den) { r -= j.col_den; ++q; }
          }
        }
      }
      continue;
    }
    if (!active) continue;
    if (whole && (j.op == FX_COPY || j.op == FX_FLIP_V || j.op == FX_FLIP_H || j.op == FX_ROT180)) {
      const bool rev = j.op == FX_FLIP_H || j.op == FX_ROT180;
      const uint32_t sr = j.op == FX_COPY || j.op == FX_FLIP_H ? i : (j.op == FX_FLIP_V ? j.rows - i - 1u : j.in_h - i - 1u);
      const uint8_t* sp = j.src + (size_t)sr * j.src_stride + (rev ? j.in_w - c0 - 16u : c0);
      if ((reinterpret_cast<uintptr_t>(sp) & 15u) == 0u) {
        const uint4 v = *reinterpret_cast<const uint4*>(sp);
        *reinterpret_cast<uint4*>(d) = rev ? make_uint4(bswap32(v.w), bswap32(v.z), bswap32(v.y), bswap32(v.x)) : v;
        continue;
      }
    }
#pragma unroll 1
    for (uint32_t q = 0; q < 4u; ++q)
      if (c0 + 4u * q < j.cols) fx_quad(j, i, c0 + 4u * q, d + 4u * q);
  }
}

// 90 / 270 degree rotations are transposes: a 64x64 source tile is read row-wise (coalesced), parked in LDS and
// written row-wise in the rotated orientation, so neither side of the copy walks a column of the image in HBM
// (the plain gather above reaches 0.45 TB/s on a 4K frame, this one is limited by launch latency).
__global__ void __launch_bounds__(256) k_effect_rot(const FxJobs jobs) {
  const FxJob& j = jobs.job[blockIdx.z];
  __shared__ __attribute__((aligned(4))) uint8_t tile[64][68];
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;  // output tile origin (row, col)
  if (i0 >= (int)j.rows || j0 >= (int)j.cols) return;
  const bool r90 = j.op == FX_ROT90;
  // source tile origin: ROT90 out[i][j] = src[in_h-1-j][i];  ROT270 out[i][j] = src[j][in_w-1-i]
  const int row_base = r90 ? (int)j.in_h - 64 - j0 : j0;
  const int col_base = r90 ? i0 : (int)j.in_w - 64 - i0;
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int ry = p * 16 + (t >> 4), cx = 4 * (t & 15);
    const int sr = row_base + ry;
    const int sc0 = col_base + cx;
    const uint8_t* sp = j.src + (size_t)(sr < 0 ? 0 : sr) * j.src_stride + sc0;
    if (sr >= 0 && sr < (int)j.in_h && sc0 >= 0 && sc0 + 3 < (int)j.in_w && (reinterpret_cast<uintptr_t>(sp) & 3u) == 0u) {
      *reinterpret_cast<uint32_t*>(&tile[ry][cx]) = *reinterpret_cast<const uint32_t*>(sp);   // (a row of the tile is 68 bytes: cx a multiple of 4)
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sc = sc0 + k;
        uint8_t v = 0;
        if (sr >= 0 && sr < (int)j.in_h && sc >= 0 && sc < (int)j.in_w) v = j.src[(size_t)sr * j.src_stride + sc];
        tile[ry][cx + k] = v;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int a = p * 16 + (t >> 4), b0 = 4 * (t & 15);  // output row a, columns b0..b0+3 of the tile
    const int oi = i0 + a;
    if (oi >= (int)j.rows) continue;
    uint8_t* d = j.dst + (size_t)oi * j.dst_stride + j0 + b0;
    uint8_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r90 ? tile[63 - (b0 + k)][a] : tile[b0 + k][63 - a];
    if (j0 + b0 + 4 <= (int)j.cols && ((reinterpret_cast<uintptr_t>(d) & 3u) == 0u)) {
      *reinterpret_cast<uint32_t*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
      for (int k = 0; k < 4 && j0 + b0 + k < (int)j.cols; ++k) d[k] = v[k];
    }
  }
}

hipError_t launch_effect(const FxJobs& j, hipStream_t s) {
  uint32_t rows = 0, cols = 0;
  for (int k = 0; k < j.n; ++k) { rows = rows > j.job[k].rows ? rows : j.job[k].rows; cols = cols > j.job[k].cols ? cols : j.job[k].cols; }
  if (j.n == 0 || rows == 0 || cols == 0) return hipSuccess;
  if (j.job[0].op == FX_ROT90 || j.job[0].op == FX_ROT270) {
    hipLaunchKernelGGL(k_effect_rot, dim3((cols + 63u) / 64u, (rows + 63u) / 64u, (unsigned)j.n), dim3(256), 0, s, j);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_effect, dim3(((cols + 15u) / 16u + 255u) / 256u, rows < 65535u ? rows : 65535u, (unsigned)j.n), dim3(256), 0, s, j);
  return hipGetLastError();
}

// =================================================================================================
// A chain of effects as ONE gather (uhdr_hip_add_effects_batch): every effect is an index map, so a chain is one as well, and for
// all but a handful of chains the source offset of output byte (i, j) of a plane is a[i] + b[j].  The host composes the two tables
// (uhdr_capi.hip: fx_compose) and picks the job's class from them; one launch moves every plane of every image of a round, reading
// the input once and writing the result once.  The classes restate what k_effect and k_effect_rot do for a single step; a class
// only selects the faster route, every route yields dst[i][j] = src[a[i] + b[j]] and none reads outside [src + lo, src + hi].
// =================================================================================================
// the dword at p (p a multiple of 4); bytes outside [vlo, vhi] are not read and come back as 0
__device__ __forceinline__ uint32_t fxc_load4(const uint8_t* p, const uint8_t* vlo, const uint8_t* vhi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), lo = reinterpret_cast<uintptr_t>(vlo), hi = reinterpret_cast<uintptr_t>(vhi);
  if (a >= lo && a + 3u <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k)
    if (a + k >= lo && a + k <= hi) v |= (uint32_t)p[k] << (8u * k);
  return v;
}

// 16 output bytes at column c0 (a multiple of 16) gathered byte by byte from `base` (global memory or LDS) through b[] - sub.
// whole: all 16 columns exist and d is 16-byte aligned -> one store; otherwise dword stores where d allows them, byte stores else.
template <typename Ptr>
__device__ __forceinline__ void fxc_gather16(Ptr base, const uint32_t* __restrict__ b, uint32_t sub, uint32_t c0, uint32_t cols, bool whole,
                                             uint8_t* d) {
  if (whole) {
    uint32_t w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint4 bb = *reinterpret_cast<const uint4*>(b + c0 + 4 * g);   // (b is padded to a multiple of 16 entries and 16-byte aligned)
      w[g] = (uint32_t)base[bb.x - sub] | ((uint32_t)base[bb.y - sub] << 8) | ((uint32_t)base[bb.z - sub] << 16) | ((uint32_t)base[bb.w - sub] << 24);
    }
    *reinterpret_cast<uint4*>(d) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
#pragma unroll 1
  for (uint32_t q = 0; q < 4u; ++q) {
    const uint32_t c = c0 + 4u * q;
    if (c >= cols) break;
    const uint4 bb = *reinterpret_cast<const uint4*>(b + c);
    if (c + 4u <= cols && (reinterpret_cast<uintptr_t>(d + 4u * q) & 3u) == 0u) {
      *reinterpret_cast<uint32_t*>(d + 4u * q) =
          (uint32_t)base[bb.x - sub] | ((uint32_t)base[bb.y - sub] << 8) | ((uint32_t)base[bb.z - sub] << 16) | ((uint32_t)base[bb.w - sub] << 24);
    } else {
      d[4u * q] = base[bb.x - sub];
      if (c + 1u < cols) d[4u * q + 1u] = base[bb.y - sub];
      if (c + 2u < cols) d[4u * q + 2u] = base[bb.z - sub];
      if (c + 3u < cols) d[4u * q + 3u] = base[bb.w - sub];
    }
  }
}

__global__ void __launch_bounds__(256) k_effect_chain(const FxChainJob* __restrict__ jobs, int n_jobs) {
  __shared__ uint32_t s_mem[64u * 65u];   // FXC_LDS: the row stretch of 4096 columns (at most 16 KiB + 4); FXC_TILE: uint8_t[64][260]
  if ((int)blockIdx.z >= n_jobs) return;
  const FxChainJob j = jobs[blockIdx.z];
  const uint8_t* vlo = j.src + j.lo;
  const uint8_t* vhi = j.src + j.hi;
  const uint32_t t = threadIdx.x;

  if (j.cls == FXC_TILE) {
    // Output tile rows i0 .. i0+63, columns j0 .. j0+63.  For one column the 64 source bytes lie within a[] 's span of the tile's rows,
    // less than 256 bytes (64 for a plain quarter turn, more behind a reduction): that run (at most 65 dwords with its alignment
    // slack) is read by 16 adjacent lanes, parked as row jj of the tile and picked up transposed, so neither side of the copy walks a
    // column of an image in HBM.  (A tile row is 65 dwords: the transposed reads of 16 lanes fall into 16 banks.)
    uint8_t(*tile)[260] = reinterpret_cast<uint8_t(*)[260]>(s_mem);
    const uint32_t j0 = blockIdx.x * 64u;
    if (j0 >= j.cols) return;                               // (block-uniform)
    const uint32_t src_lsb = (uint32_t)reinterpret_cast<uintptr_t>(j.src);
    for (uint32_t i0 = blockIdx.y * 64u; i0 < j.rows; i0 += gridDim.y * 64u) {
      const uint32_t il = min(i0 + 63u, j.rows - 1u);
      const uint32_t a0 = j.a[i0], a1 = j.a[il];
      const uint32_t alo = min(a0, a1), span = max(a0, a1) - alo;   // (a is monotone: the ends bound the tile's rows; span < 256)
      __syncthreads();                                      // (the previous tile has been written out)
#pragma unroll
      for (uint32_t p = 0; p < 4u; ++p) {
        const uint32_t jj = p * 16u + (t >> 4);
        if (j0 + jj < j.cols) {
          const uint8_t* s0 = j.src + alo + j.b[j0 + jj];
          const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(s0) & 3u);
          const uint8_t* sal = s0 - off;
          for (uint32_t q = t & 15u; q < 65u && 4u * q <= off + span; q += 16u)
            *reinterpret_cast<uint32_t*>(&tile[jj][4u * q]) = fxc_load4(sal + 4u * q, vlo, vhi);
        }
      }
      __syncthreads();
#pragma unroll
      for (uint32_t p = 0; p < 4u; ++p) {
        const uint32_t r = p * 16u + (t >> 4), c = 4u * (t & 15u);
        const uint32_t oi = i0 + r;
        if (oi >= j.rows || j0 + c >= j.cols) continue;
        const uint32_t ar = j.a[oi] - alo;
        const uint4 bb = *reinterpret_cast<const uint4*>(j.b + j0 + c);
        const uint32_t base = src_lsb + alo;
        const uint32_t v0 = tile[c][((base + bb.x) & 3u) + ar], v1 = tile[c + 1u][((base + bb.y) & 3u) + ar];
        const uint32_t v2 = tile[c + 2u][((base + bb.z) & 3u) + ar], v3 = tile[c + 3u][((base + bb.w) & 3u) + ar];
        uint8_t* d = j.dst + (size_t)oi * j.dst_stride + j0 + c;
        if (j0 + c + 4u <= j.cols && (reinterpret_cast<uintptr_t>(d) & 3u) == 0u) {
          *reinterpret_cast<uint32_t*>(d) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
        } else {
          d[0] = (uint8_t)v0;
          if (j0 + c + 1u < j.cols) d[1] = (uint8_t)v1;
          if (j0 + c + 2u < j.cols) d[2] = (uint8_t)v2;
          if (j0 + c + 3u < j.cols) d[3] = (uint8_t)v3;
        }
      }
    }
    return;
  }

  // the row classes: one thread produces 16 consecutive output bytes of one row, a block 4096 columns
  const uint32_t cb = blockIdx.x * 4096u;
  if (cb >= j.cols) return;                                 // (block-uniform)
  const uint32_t c0 = cb + t * 16u;
  const bool active = c0 < j.cols;
  for (uint32_t i = blockIdx.y; i < j.rows; i += gridDim.y) {
    const uint32_t ai = j.a[i];
    uint8_t* d = j.dst + (size_t)i * j.dst_stride + c0;
    const bool whole = active && c0 + 16u <= j.cols && (reinterpret_cast<uintptr_t>(d) & 15u) == 0u;
    if (j.cls == FXC_LDS) {
      // b is monotone over the block's columns: its ends bound the stretch of the source row, at most 16 KiB + 1 bytes (host-checked)
      const uint32_t c_last = min(cb + 4095u, j.cols - 1u);
      const uint32_t b0 = j.b[cb], b1 = j.b[c_last];
      const uint32_t s_lo = min(b0, b1), s_hi = max(b0, b1);
      const uint8_t* first = j.src + ai + s_lo;
      const uint32_t off0 = (uint32_t)(reinterpret_cast<uintptr_t>(first) & 3u);
      const uint8_t* p_al = first - off0;
      const uint32_t nbytes = s_hi - s_lo + 1u + off0;
      __syncthreads();                                      // (the previous row's gathers are done)
      for (uint32_t k = t; k < (nbytes + 3u) / 4u; k += 256u) s_mem[k] = fxc_load4(p_al + 4u * k, vlo, vhi);
      __syncthreads();
      if (active) fxc_gather16(reinterpret_cast<const uint8_t*>(s_mem) + off0, j.b, s_lo, c0, j.cols, whole, d);
      continue;
    }
    if (!active) continue;
    if (whole && (j.cls == FXC_ASC || j.cls == FXC_DESC)) {
      const bool rev = j.cls == FXC_DESC;
      const uint8_t* sp = j.src + ai + j.b[c0] - (rev ? 15u : 0u);
      if ((reinterpret_cast<uintptr_t>(sp) & 15u) == 0u) {
        const uint4 v = *reinterpret_cast<const uint4*>(sp);
        *reinterpret_cast<uint4*>(d) = rev ? make_uint4(bswap32(v.w), bswap32(v.z), bswap32(v.y), bswap32(v.x)) : v;
        continue;
      }
    }
    fxc_gather16(j.src + ai, j.b, 0u, c0, j.cols, whole, d);
  }
}

hipError_t launch_effect_chain(const FxChainJob* dev_jobs, const FxChainJob* host_jobs, int n, hipStream_t s) {
  uint32_t gx = 0, gy = 0;
  for (int k = 0; k < n; ++k) {
    const FxChainJob& j = host_jobs[k];
    if (j.rows == 0 || j.cols == 0) continue;
    const bool tile = j.cls == FXC_TILE;
    const uint32_t x = tile ? (j.cols + 63u) / 64u : (j.cols + 4095u) / 4096u;
    const uint32_t y = tile ? (j.rows + 63u) / 64u : j.rows;
    gx = gx > x ? gx : x;
    gy = gy > y ? gy : y;
  }
  if (n <= 0 || gx == 0 || gy == 0) return hipSuccess;
  hipLaunchKernelGGL(k_effect_chain, dim3(gx, gy < 65535u ? gy : 65535u, (unsigned)n), dim3(256), 0, s, dev_jobs, n);
  return hipGetLastError();
}

// =================================================================================================
// diagnostics: evaluate one transfer function over an array (tests/test_gpu_transfer_exhaustive.py)
// =================================================================================================
__global__ void __launch_bounds__(256) k_eval_transfer(int fn, const float* in, float* out, size_t n, EvalConsts ec) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float x = in[i];
  float y = 0.0f;
  switch (fn) {
    case 0: y = srgb_inv_oetf_guarded(x); break;
    case 1: y = hlg_inv_oetf_guarded(x); break;
    case 2: y = pq_inv_oetf_guarded(x); break;
    case 3: y = (float)encode_gain_guarded(x, ec.min_boost, ec.max_boost, ec.log2_min, ec.log2_max, ec.enc_scale,
                                           ec.enc_byte_min, ec.enc_byte_max); break;
    case 4: { float v[1] = {x}; hlg_oetf_guarded_n<1>(v); y = v[0]; break; }
    case 5: { float v[1] = {x}; pq_oetf_guarded_n<1>(v); y = v[0]; break; }
    case 6: y = exp2_to_float_guarded(x); break;
    case 16: y = (float)exp2((double)x); break;
    case 10: y = srgb_inv_oetf_exact(x); break;
    case 11: y = hlg_inv_oetf_exact(x); break;
    case 12: y = pq_inv_oetf_exact(x); break;
    case 13: y = (float)encode_gain(x, ec.min_boost, ec.max_boost, ec.log2_min, ec.log2_max); break;
    case 14: y = hlg_oetf_exact(x); break;
    case 15: y = pq_oetf_exact(x); break;
    case 24: y = hlg_oetf_fast(x); break;
    case 26: y = __builtin_amdgcn_exp2f(x); break;
    case 27: y = pq_oetf_est(x); break;
    case 25: y = pq_oetf_fast(x); break;
    case 20: y = srgb_inv_oetf_fast(x); break;
    case 21: y = hlg_inv_oetf_fast(x); break;
    case 22: y = pq_inv_oetf_fast(x); break;
    case 23: y = __builtin_amdgcn_logf(x); break;
    // the reference's LUT accessors over the device tables; 46: GainLUT(min, max, displayBoost = max).getGainFactor
    case 40: y = ec.lut[kLutSrgbInv + lut_index(x, kLutSrgbInvN)]; break;
    case 41: y = ec.lut[kLutHlgInv + lut_index(x, kLutHlgInvN)]; break;
    case 42: y = ec.lut[kLutPqInv + lut_index(x, kLutPqInvN)]; break;
    case 44: y = ec.lut[kLutHlg + lut_index(x, kLutHlgN)]; break;
    case 45: y = ec.lut[kLutPq + lut_index(x, kLutPqN)]; break;
    case 46: y = gain_lut_entry(lut_index(x, kGainLutN), ec.log2_min_d, ec.log2_max_d, 1.0f); break;
    case 47: y = round_half_up(x) == (uint32_t)((double)x + 0.5) ? 1.0f : 0.0f; break;   // (the accessors' one-instruction index: +0 <= x < 2^31 and -0)
    // FAST apply's line-segment tables, read from the device buffer with the kernel's own index arithmetic.  50 / 53 / 54: stage 1,
    // T(x) = srgbInvOetf(x)^g for g = 1, 1/2, m1.  51 / 52: the 10-bit code stage 2 yields for u in [0, 1] (HLG: u = sqrt(e), PQ:
    // u = e^m1); the kernel's fma rounds toward zero, which is the truncation of the exact sum formed here in double.
    case 50: case 53: case 54: {
      const uint32_t base = fn == 50 ? kTabS1Lin : fn == 53 ? kTabS1Hlg : kTabS1Pq;
      const float2 t = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(ec.lut + base) + (fn == 50 ? tab_offset(x) : pow_offset(x)));
      y = __builtin_fmaf(t.y, x, t.x); break; }
    case 51: case 52: {
      const float s = __builtin_fmaf(x, 2.0f, 2.0f);
      const float2 t = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(ec.lut + (fn == 51 ? kTabS2Hlg : kTabS2Pq)) + (s2_address(s, 0u) >> 5));
      const double v = -(((double)t.y * (double)s + (double)t.x) + 2.0) * 4194304.0;
      y = (float)(long long)v + (v < 0.0 ? -1000.0f : 0.0f); break; }   // (a negative sum would leave the binade: flagged)
    case 60: y = log2_to_float(x); break;   // the log2 constant the content-adaptive path derives on the device for boost x
    case 30: y = map_to_float_fast((uint32_t)x); break;
    case 31: y = map_to_float((uint32_t)x); break;
    // 1.0 where the lean f64 path was accepted by the rounding test, 0.0 where the exact path ran
    case 100: { const float t = div_const(x + 0.055f, 1.055f, 1.0f / 1.055f);
                float v1[1] = {x};
                srgb_inv_oetf_guarded_n<1>(v1);   // (kept for symmetry; the acceptance rate is measured below)
                const double xd = (double)t, z0 = (double)__builtin_amdgcn_exp2f(0.4f * __builtin_amdgcn_logf(t));
                const double X = xd * xd, z2 = z0 * z0, z4 = z2 * z2;
                const double yy = X * __builtin_fma(-__builtin_fma(z4, z0, -X), (double)(0.2f * __builtin_amdgcn_rcpf((float)z4)), z0);
                y = (x <= 0.04045f || ziv_safe(yy)) ? 1.0f : 0.0f; break; }
    case 101: { const float v = div_const(x - UHDR_HLG_C, UHDR_HLG_A, 1.0f / UHDR_HLG_A);
                y = (x <= 0.5f || ziv_safe((fast_exp2((double)v * 0x1.71547652b82fep+0) + (double)UHDR_HLG_B) * (1.0 / 12.0))) ? 1.0f : 0.0f; break; }
    default: break;
  }
  out[i] = y;
}

// The deterministic frame pair of SURVEY.md section 8(d), written straight into HBM: s <- s * 1664525 + 1013904223 (mod 2^32),
// draw = s >> 8, draws alternating between the P010 word and the 8-bit sample of element i.  Thread i jumps to state 2 i + 1 by
// composing the affine map with itself (binary exponentiation on (a, c)), so the elements are independent.
__global__ void __launch_bounds__(256) k_synth_lcg(uint16_t* p010, uint8_t* yuv, uint32_t n_luma, uint32_t n, uint32_t seed) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t ar = 1u, cr = 0u, ap = 1664525u, cp = 1013904223u;
  for (uint32_t k = 2u * i + 1u; k != 0u; k >>= 1) {
    if (k & 1u) { ar *= ap; cr = cr * ap + cp; }
    cp = cp * ap + cp;
    ap *= ap;
  }
  const uint32_t s1 = ar * seed + cr, s2 = s1 * 1664525u + 1013904223u;
  // Both remainders by constant divisors (multiply-high forms).  With a divisor chosen at run time hipcc, knowing the draw to be
  // below 2^24, expands the division through v_rcp_iflag_f32 + one upward correction, which returns quotient + 1 where the true
  // quotient lies within 2^-23 below an integer (15172754 / 897 = 16914.9989 -> 16915: 18 wrong words in a 640x480 frame).
  const uint32_t d = s1 >> 8, r = i < n_luma ? d % 877u : d % 897u;
  p010[i] = (uint16_t)((64u + r) << 6);
  yuv[i] = (uint8_t)(s2 >> 8);
}
hipError_t launch_synth_lcg(uint16_t* p010, uint8_t* yuv, uint32_t n_luma, uint32_t n, uint32_t seed, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_synth_lcg, dim3((n + 255u) / 256u), dim3(256), 0, s, p010, yuv, n_luma, n, seed);
  return hipGetLastError();
}

hipError_t launch_eval_transfer(int fn, const float* in, float* out, size_t n, const EvalConsts& ec, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_eval_transfer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fn, in, out, n, ec);
  return hipGetLastError();
}

}  // namespace uhdr
