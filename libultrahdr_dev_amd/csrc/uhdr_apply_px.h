// uhdr_apply_px.h -- what the per-pixel apply kernels of uhdr_kernels.hip and the packed apply kernels of uhdr_packed_apply.hip
// share: sampleMap's address arithmetic, the per-pixel grid, the OETF of an output format, the store of a pixel and the gain factor
// of general metadata.  Device code only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "uhdr_device_math.h"
#include "uhdr_kernels.h"

namespace uhdr {

constexpr float k255 = 1 / 255.0f;  // gainmapmath.cpp:579

// FMT: 1 HDR_LINEAR (F16), 2 HDR_PQ, 3 HDR_HLG, 4 HDR_LINEAR_RGB_10BIT (ultrahdr.h:56-64)
template <int FMT, bool EXACT>
__device__ __forceinline__ F3 hdr_oetf(F3 e) {
  if (FMT == 3) {
    if (EXACT) { float ch[3] = {e.x, e.y, e.z}; hlg_oetf_guarded_n<3>(ch); e.x = ch[0]; e.y = ch[1]; e.z = ch[2]; }
    else { e.x = hlg_oetf_fast(e.x); e.y = hlg_oetf_fast(e.y); e.z = hlg_oetf_fast(e.z); }
  } else if (FMT == 2) {
    if (EXACT) { float ch[3] = {e.x, e.y, e.z}; pq_oetf_guarded_n<3>(ch); e.x = ch[0]; e.y = ch[1]; e.z = ch[2]; }
    else { e.x = pq_oetf_est(e.x); e.y = pq_oetf_est(e.y); e.z = pq_oetf_est(e.z); }   // (within 3e-4 of a code; pq_oetf_fast: 0.3)
  }
  return e;
}

__device__ __forceinline__ float map_to_float(uint32_t v) { return (float)v / 255.0f; }  // gainmapmath.cpp:632
// the same value in 3 issue slots instead of the ~10 of an IEEE division: exact for all 256 map bytes
// (tests/test_gpu_transfer_exhaustive.py::test_map_byte_to_float_is_exact)
__device__ __forceinline__ float map_to_float_fast(uint32_t v) { return div_const((float)v, 255.0f, 1.0f / 255.0f); }

// sampleMap's address arithmetic (gainmapmath.cpp:686-720) for pixel (x, y): the four taps' map coordinates and the pixel's weights
struct PxTaps { uint32_t xl, xu, yl, yu; const float* w; };
__device__ __forceinline__ PxTaps px_taps(const AppConsts& c, uint32_t x, uint32_t y) {
  const uint32_t s = c.scale;
  uint32_t xl, yl, ox, oy;
  if ((s & (s - 1u)) == 0u) {   // (a launch-uniform branch: scale factors are powers of two in practice)
    const uint32_t sh = (uint32_t)__builtin_ctz(s);
    xl = x >> sh; yl = y >> sh; ox = x & (s - 1u); oy = y & (s - 1u);
  } else {
    xl = x / s; yl = y / s; ox = x - xl * s; oy = y - yl * s;
  }
  uint32_t xu = xl + 1u, yu = yl + 1u;
  xl = min(xl, c.map_w - 1u); xu = min(xu, c.map_w - 1u);
  yl = min(yl, c.map_h - 1u); yu = min(yu, c.map_h - 1u);
  int tbl = 0;
  if (xl == xu && yl == yu) tbl = 3;
  else if (xl == xu) tbl = 1;
  else if (yl == yu) tbl = 2;
  PxTaps t;
  t.xl = xl; t.xu = xu; t.yl = yl; t.yu = yu;
  t.w = c.idw + (size_t)tbl * s * s * 4u + (size_t)oy * s * 4u + ox * 4u;
  return t;
}
// the per-pixel kernels run on a (column block, row, image) grid: no division by the width; rows beyond the grid's 65535 are
// reached by striding
__host__ __device__ inline dim3 px_grid(uint32_t width, uint32_t height, int n) {
  return dim3((width + 255u) / 256u, height < 65535u ? height : 65535u, (unsigned)n);
}
template <int FMT>
__device__ __forceinline__ void px_store(void* dst, size_t idx, size_t total, F3 e) {
  if (FMT == 2 || FMT == 3) {
    static_cast<uint32_t*>(dst)[idx] = pack_1010102(e.x, e.y, e.z);
  } else if (FMT == 1) {
    static_cast<uint2*>(dst)[idx] = pack_f16(e.x, e.y, e.z);
  } else {
    uint16_t* base = static_cast<uint16_t*>(dst);
    base[idx] = (uint16_t)(0x3ffu & (uint32_t)(e.x * 1023.0f));
    base[total + idx] = (uint16_t)(0x3ffu & (uint32_t)(e.y * 1023.0f));
    base[2 * total + idx] = (uint16_t)(0x3ffu & (uint32_t)(e.z * 1023.0f));
  }
}
template <int FMT>
__device__ __forceinline__ void px_store(const AppImage& im, size_t idx, size_t total, F3 e) {
  px_store<FMT>(im.dst, idx, total, e);
}

// general metadata: the factor 2^(A g' + B) of one gain, g' = g^(1 / gamma)
template <bool GAMMA>
__device__ __forceinline__ float md_factor(const AppMdConsts& m, float g) {
  if (GAMMA) g = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(g) * m.inv_gamma);   // log2(0) = -inf, 2^-inf = 0
  return __builtin_amdgcn_exp2f(__builtin_fmaf(g, m.A, m.B));   // (one rounding of an exponent that reaches log2 max)
}

}  // namespace uhdr
