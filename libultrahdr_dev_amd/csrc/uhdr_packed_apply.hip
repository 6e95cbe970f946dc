// uhdr_packed_apply.hip -- HDR from an RGBA8888 SDR image and its gain map (gfx950, wave64).
//
//   k_build_srgb_codes            the 256 values srgbInvOetf(code * (1 / 255.0f)), once per device, by the exact function
//   k_apply_packed_s4<FMT,KIND,RGB>   scale factor 4, 16-byte-aligned rows: a lane owns four adjacent pixels of one map cell
//   k_apply_packed_px<FMT,KIND,RGB>   one pixel per lane: any scale factor, any alignment, ragged widths
//
// The reference's applyGainMap (ultrahdr.cpp:429-489) with its YUV loads and yuvToRgb replaced by the packed pixel's codes: a channel
// of the SDR colour is srgbInvOetf(code * (1 / 255.0f)), and a code has 256 values, so the sRGB stage is a table of the reference's
// own floats -- in LDS, shared by FAST and EXACT.  What remains per pixel is sampleMap, one exp2 per gain and the OETF.  Both forms
// run the same arithmetic (packed_lin) and give the same bytes; the strip form only loads and stores in 16-byte pieces and loads a
// cell's four taps once for four pixels.  The kernels live in a translation unit of their own so that nothing here enters the
// code generation of uhdr_kernels.hip; what the two share is uhdr_apply_px.h.
#include "uhdr_kernels.h"

#include <hip/hip_runtime.h>

#include "uhdr_apply_px.h"
#include "uhdr_device_math.h"

namespace uhdr {

__global__ void __launch_bounds__(kSrgbCodes) k_build_srgb_codes(float* table) {
  table[threadIdx.x] = srgb_inv_oetf_guarded((float)threadIdx.x * k255);   // ultrahdr.cpp:429-431 on a packed code, then :440
}
hipError_t launch_build_srgb_codes(float* table, hipStream_t s) {
  hipLaunchKernelGGL(k_build_srgb_codes, dim3(1), dim3(kSrgbCodes), 0, s, table);
  return hipGetLastError();
}

// applyGain's factor of one interpolated gain (gainmapmath.cpp:550-555 with the display boost, as recover_hdr forms it; FAST: that
// factor over the display boost), or the factor of general metadata
template <int KIND>
__device__ __forceinline__ float packed_factor(const AppConsts& c, const AppMdConsts& m, float gain) {
  if (KIND == kPackedMd) return md_factor<false>(m, gain);
  if (KIND == kPackedMdGamma) return md_factor<true>(m, gain);
  // FAST: gain -> log boost -> display scaling as ONE exponent, factor / display_boost = 2^(gain A + B) with the host's A and B
  // (AppFast, as k_apply_s4 forms it): one f32 fma in place of the reference's two f64 products, and no division behind it
  if (KIND == kPackedFast) return __builtin_amdgcn_exp2f(__builtin_fmaf(gain, c.fast.A, c.fast.B));
  const float log_boost = (float)(c.log2_min_d * (double)(1.0f - gain) + c.log2_max_d * (double)gain);
  return exp2_to_float_guarded(log_boost * c.display_boost / c.max_boost);
}
// one channel: e is the table's value of its code
template <int KIND>
__device__ __forceinline__ float packed_channel(const AppConsts& c, const AppMdConsts& m, float e, float factor) {
  if (KIND == kPackedExact) return (e * factor) / c.display_boost;   // ultrahdr.cpp:451
  if (KIND == kPackedFast) return e * factor;   // (the factor carries 1 / display_boost)
  return fmaxf(__builtin_fmaf(e + m.off_sdr, factor, -m.off_hdr_d), 0.0f);   // md_channel's shape
}
// the linear HDR colour of one packed pixel p from its gains (a one-plane map: g[0] alone, one exp2 for the three channels)
template <int KIND, bool RGB>
__device__ __forceinline__ F3 packed_lin(const AppConsts& c, const AppMdConsts& m, const float* tab, uint32_t p, const float (&g)[3]) {
  float f[3];
  f[0] = packed_factor<KIND>(c, m, g[0]);
  if (RGB) { f[1] = packed_factor<KIND>(c, m, g[1]); f[2] = packed_factor<KIND>(c, m, g[2]); }
  else f[1] = f[2] = f[0];
  F3 lin;
  lin.x = packed_channel<KIND>(c, m, tab[p & 0xffu], f[0]);
  lin.y = packed_channel<KIND>(c, m, tab[(p >> 8) & 0xffu], f[1]);
  lin.z = packed_channel<KIND>(c, m, tab[(p >> 16) & 0xffu], f[2]);
  return lin;
}
// the four taps of a pixel or a cell as floats, e[tap][channel] (a one-plane map: channel 0), in sampleMap's order: (xl, yl), (xl, yu),
// (xu, yl), (xu, yu)
template <bool RGB>
__device__ __forceinline__ void packed_taps(const AppConsts& c, const PackedAppImage& im, uint32_t xl, uint32_t xu, uint32_t yl, uint32_t yu,
                                            float (&e)[4][3]) {
  if (RGB) {
    const uint32_t* map = reinterpret_cast<const uint32_t*>(im.map);
    const uint32_t t[4] = {map[(size_t)yl * c.map_stride + xl], map[(size_t)yu * c.map_stride + xl],
                           map[(size_t)yl * c.map_stride + xu], map[(size_t)yu * c.map_stride + xu]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k][0] = map_to_float_fast(t[k] & 0xffu);
      e[k][1] = map_to_float_fast((t[k] >> 8) & 0xffu);
      e[k][2] = map_to_float_fast((t[k] >> 16) & 0xffu);
    }
  } else {
    e[0][0] = map_to_float_fast(im.map[(size_t)yl * c.map_w + xl]);
    e[1][0] = map_to_float_fast(im.map[(size_t)yu * c.map_w + xl]);
    e[2][0] = map_to_float_fast(im.map[(size_t)yl * c.map_w + xu]);
    e[3][0] = map_to_float_fast(im.map[(size_t)yu * c.map_w + xu]);
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k][1] = e[k][2] = e[k][0];
  }
}
// sampleMap's weighted sum (gainmapmath.cpp:715-719), per channel
template <bool RGB>
__device__ __forceinline__ void packed_gains(const float (&e)[4][3], float w0, float w1, float w2, float w3, float (&g)[3]) {
#pragma unroll
  for (int k = 0; k < (RGB ? 3 : 1); ++k) g[k] = e[0][k] * w0 + e[1][k] * w1 + e[2][k] * w2 + e[3][k] * w3;
  if (!RGB) g[1] = g[2] = g[0];
}

template <int FMT, int KIND, bool RGB>
__global__ void __launch_bounds__(256) k_apply_packed_px(const AppConsts c, const AppMdConsts m, const PackedAppBatch b,
                                                         const float* __restrict__ table) {
  __shared__ float s_tab[kSrgbCodes];
  s_tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const PackedAppImage& im = b.img[blockIdx.z];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x >= c.width) return;
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {
    const uint32_t p = im.sdr[(size_t)y * im.sdr_stride + x];
    const PxTaps t = px_taps(c, x, y);
    float e[4][3], g[3];
    packed_taps<RGB>(c, im, t.xl, t.xu, t.yl, t.yu, e);
    packed_gains<RGB>(e, t.w[0], t.w[1], t.w[2], t.w[3], g);
    const F3 lin = packed_lin<KIND, RGB>(c, m, s_tab, p, g);
    px_store<FMT>(im.dst, (size_t)y * c.width + x, total, hdr_oetf<FMT, KIND == kPackedExact>(lin));
  }
}

// The strip form.  Lane = the four pixels (4 cx .. 4 cx + 3, y) of map cell (cx, y / 4): one 16-byte load; the cell's taps and its
// weight table are the strip's (oy = y % 4, ox = 0 .. 3), the weights come from a copy of the four scale-4 tables in LDS (lanes of a
// row read the same 16 bytes: a broadcast).  A row leaves as 16 bytes per lane (RGBA1010102), two contiguous 16-byte pieces (F16) or
// 8 bytes per plane (planar 10 bit).  Rows beyond the grid's 65535 are reached by striding, as in the per-pixel kernels.
template <int FMT, int KIND, bool RGB>
__global__ void __launch_bounds__(256) k_apply_packed_s4(const AppConsts c, const AppMdConsts m, const PackedAppBatch b,
                                                         const float* __restrict__ table) {
  __shared__ float s_tab[kSrgbCodes];
  __shared__ __attribute__((aligned(16))) float s_idw[4 * 64];
  s_tab[threadIdx.x] = table[threadIdx.x];
  s_idw[threadIdx.x] = c.idw[threadIdx.x];   // (scale 4: 4 tables of 64 floats)
  __syncthreads();
  const PackedAppImage& im = b.img[blockIdx.z];
  const size_t total = (size_t)c.width * c.height;
  const uint32_t cx = blockIdx.x * 256u + threadIdx.x;
  if (cx >= c.map_w) return;
  const uint32_t xu = min(cx + 1u, c.map_w - 1u);
  for (uint32_t y = blockIdx.y; y < c.height; y += gridDim.y) {
    const uint4 px = *reinterpret_cast<const uint4*>(im.sdr + (size_t)y * im.sdr_stride + 4u * cx);
    const uint32_t yl = y >> 2, oy = y & 3u, yu = min(yl + 1u, c.map_h - 1u);
    const uint32_t tbl = cx == xu ? (yl == yu ? 3u : 1u) : (yl == yu ? 2u : 0u);   // px_taps' choice: corner, no-right, no-bottom, standard
    const float4* w = reinterpret_cast<const float4*>(s_idw + tbl * 64u + oy * 16u);
    float e[4][3];
    packed_taps<RGB>(c, im, cx, xu, yl, yu, e);
    const uint32_t p[4] = {px.x, px.y, px.z, px.w};
    F3 o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 wj = w[j];
      float g[3];
      packed_gains<RGB>(e, wj.x, wj.y, wj.z, wj.w, g);
      o[j] = hdr_oetf<FMT, KIND == kPackedExact>(packed_lin<KIND, RGB>(c, m, s_tab, p[j], g));
    }
    const size_t idx = (size_t)y * c.width + 4u * cx;
    if (FMT == 2 || FMT == 3) {
      *reinterpret_cast<uint4*>(static_cast<uint32_t*>(im.dst) + idx) =
          make_uint4(pack_1010102(o[0].x, o[0].y, o[0].z), pack_1010102(o[1].x, o[1].y, o[1].z), pack_1010102(o[2].x, o[2].y, o[2].z),
                     pack_1010102(o[3].x, o[3].y, o[3].z));
    } else if (FMT == 1) {
      uint2 h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = pack_f16(o[j].x, o[j].y, o[j].z);
      uint4* d = reinterpret_cast<uint4*>(static_cast<uint2*>(im.dst) + idx);
      d[0] = make_uint4(h[0].x, h[0].y, h[1].x, h[1].y);
      d[1] = make_uint4(h[2].x, h[2].y, h[3].x, h[3].y);
    } else {
      uint16_t* base = static_cast<uint16_t*>(im.dst);
      uint32_t q[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[j][0] = 0x3ffu & (uint32_t)(o[j].x * 1023.0f);
        q[j][1] = 0x3ffu & (uint32_t)(o[j].y * 1023.0f);
        q[j][2] = 0x3ffu & (uint32_t)(o[j].z * 1023.0f);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)
        *reinterpret_cast<uint2*>(base + (size_t)k * total + idx) = make_uint2(q[0][k] | (q[1][k] << 16), q[2][k] | (q[3][k] << 16));
    }
  }
}

template <int FMT, int KIND, bool RGB>
static hipError_t launch_apply_packed_t(const AppConsts& c, const AppMdConsts& m, const PackedAppBatch& b, const float* table, int n, bool strip,
                                        hipStream_t s) {
  if (strip) hipLaunchKernelGGL((k_apply_packed_s4<FMT, KIND, RGB>), px_grid(c.map_w, c.height, n), dim3(256), 0, s, c, m, b, table);
  else hipLaunchKernelGGL((k_apply_packed_px<FMT, KIND, RGB>), px_grid(c.width, c.height, n), dim3(256), 0, s, c, m, b, table);
  return hipGetLastError();
}
template <int FMT>
static hipError_t launch_apply_packed_f(const AppConsts& c, const AppMdConsts& m, const PackedAppBatch& b, const float* table, int n, int kind,
                                        bool rgb, bool strip, hipStream_t s) {
  switch (kind * 2 + (rgb ? 1 : 0)) {
    case 0: return launch_apply_packed_t<FMT, kPackedFast, false>(c, m, b, table, n, strip, s);
    case 1: return launch_apply_packed_t<FMT, kPackedFast, true>(c, m, b, table, n, strip, s);
    case 2: return launch_apply_packed_t<FMT, kPackedExact, false>(c, m, b, table, n, strip, s);
    case 3: return launch_apply_packed_t<FMT, kPackedExact, true>(c, m, b, table, n, strip, s);
    case 4: return launch_apply_packed_t<FMT, kPackedMd, false>(c, m, b, table, n, strip, s);
    case 5: return launch_apply_packed_t<FMT, kPackedMd, true>(c, m, b, table, n, strip, s);
    case 6: return launch_apply_packed_t<FMT, kPackedMdGamma, false>(c, m, b, table, n, strip, s);
    case 7: return launch_apply_packed_t<FMT, kPackedMdGamma, true>(c, m, b, table, n, strip, s);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_apply_packed(const AppConsts& c, const AppMdConsts& m, const PackedAppBatch& b, const float* table, int n, int fmt, int kind,
                               bool rgb, bool strip, hipStream_t s) {
  if (n == 0 || c.width == 0 || c.height == 0) return hipSuccess;
  if (strip && (c.scale != 4u || c.width != 4u * c.map_w)) return hipErrorInvalidValue;
  switch (fmt) {
    case 1: return launch_apply_packed_f<1>(c, m, b, table, n, kind, rgb, strip, s);
    case 2: return launch_apply_packed_f<2>(c, m, b, table, n, kind, rgb, strip, s);
    case 3: return launch_apply_packed_f<3>(c, m, b, table, n, kind, rgb, strip, s);
    case 4: return launch_apply_packed_f<4>(c, m, b, table, n, kind, rgb, strip, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace uhdr
