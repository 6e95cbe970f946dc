// uhdr_jpeg.hip -- baseline JPEG compression of the path's outputs on the GPU (encode side).
//
// Drop-in for the reference's JpegEncoderHelper::compressImage (lib/src/jpegencoderhelper.cpp:39-283, declared
// lib/include/ultrahdr/jpegencoderhelper.h:43-60): YUV 4:2:0 planar or a single 8-bit plane (the gain map,
// jpegr.cpp:294-297) -> the byte stream libjpeg writes in raw-data mode with default tables, quality scaling with
// force_baseline and the ISLOW DCT.  The whole encoder runs on the device; the host only builds the ~600-byte header:
//
//   k_jpeg_fdct_quant_count   one thread per 8x8 block (in entropy-coding order, dummy edge blocks included): level shift,
//                       13-bit fixed-point FDCT, quantisation by rounded division -> 64 int16 in zigzag order; and, from the same
//                       registers, DC difference + run/size symbols -> the block's number of bits
//   k_jpeg_emit         one thread per block: its bit offset (the totals of the workgroups in front + a block scan), then its
//                       codes written MSB-first there (whole words stored,
//                       the two boundary words OR-ed atomically); the last block pads the final byte with ones
//   k_jpeg_stuff_count  one thread per 64 bytes of the packed stream: number of 0xFF bytes (and per workgroup)
//   k_jpeg_stuff_copy   one thread per 64 bytes: copy to the output with 0x00 stuffed after every 0xFF, EOI at the end
//   k_rgba_to_ycc420    (in front of the chain, uhdr_hip_jpeg_encode_rgba420_batch only) RGBA8888 -> the Y, Cb, Cr planes libjpeg's
//                       colour conversion and h2v2 downsampler hand its FDCT, padded to whole MCUs as libjpeg pads them
//   k_rgba_to_ycc422    the same for a 4:2:2 file: h2v1 downsampler, MCUs of 16 x 8 pixels
//   k_jpeg_opt_*        (Job::optimize) the same chain with Huffman tables built from the image's own symbol counts, see below
//   k_jpeg_rst_*        (Job::rst_blocks) the same chain with restart intervals -- padding, RSTn markers, the DC prediction cut --, see below
//   k_jpeg_prog_*       (Job::progressive) SOF2: libjpeg's simple progression, ten scans over the same coefficients, see below
//
// Byte-exact against libjpeg for every size, stride regime and quality tested (tests/test_gpu_jpeg.py against
// oracle/jpeg_oracle.c, which tests/test_jpeg_oracle.py pins to the libjpeg builds of the image).
#include <hip/hip_runtime.h>
#include "uhdr_wave_scan.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "uhdr_jpeg.h"

namespace uhdr {
namespace jpeg {

// ---- ITU-T T.81 Annex K tables ----------------------------------------------------------------------------------
static const uint8_t kStdLumQuant[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                         14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                         18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                         49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kStdChrQuant[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t kBitsDcLum[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kBitsDcChr[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kValsDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kBitsAcLum[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kValsAcLum[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kBitsAcChr[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kValsAcChr[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Huffman codes of the four default tables: [0] DC lum, [1] AC lum, [2] DC chroma, [3] AC chroma.  Packed (size << 16) | code.
__constant__ uint32_t c_huff[4][256];
// the default tables' DHT bodies (BITS, then HUFFVAL), same order: what k_jpeg_opt_tables_batch falls back to for a histogram whose
// optimal code would be longer than 32 bits (libjpeg gives up on those)
__constant__ uint8_t c_std_dht[4][16 + 162];

static void derive_codes(const uint8_t bits[16], const uint8_t* vals, uint32_t out[256]) {  // T.81 Annex C
  memset(out, 0, sizeof(uint32_t) * 256);
  uint32_t code = 0;
  int p = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++p) out[vals[p]] = ((uint32_t)l << 16) | code++;
    code <<= 1;
  }
}

hipError_t upload_tables() {
  uint32_t t[4][256];
  derive_codes(kBitsDcLum, kValsDc, t[0]);
  derive_codes(kBitsAcLum, kValsAcLum, t[1]);
  derive_codes(kBitsDcChr, kValsDc, t[2]);
  derive_codes(kBitsAcChr, kValsAcChr, t[3]);
  uint8_t d[4][16 + 162] = {};
  const uint8_t* bits[4] = {kBitsDcLum, kBitsAcLum, kBitsDcChr, kBitsAcChr};
  const uint8_t* vals[4] = {kValsDc, kValsAcLum, kValsDc, kValsAcChr};
  for (int k = 0; k < 4; ++k) {
    memcpy(d[k], bits[k], 16);
    memcpy(d[k] + 16, vals[k], (k & 1) ? 162 : 12);
  }
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_std_dht), d, sizeof(d));
  if (e != hipSuccess) return e;
  return hipMemcpyToSymbol(HIP_SYMBOL(c_huff), t, sizeof(t));
}

// jpeg_set_quality(quality, TRUE): jpeg_quality_scaling + jpeg_add_quant_table with force_baseline
void quant_table(int quality, bool chroma, uint16_t out_natural[64]) {
  if (quality <= 0) quality = 1;
  if (quality > 100) quality = 100;
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
  const uint8_t* base = chroma ? kStdChrQuant : kStdLumQuant;
  for (int i = 0; i < 64; ++i) {
    long t = ((long)base[i] * scale + 50L) / 100L;
    if (t <= 0L) t = 1L;
    if (t > 255L) t = 255L;
    out_natural[i] = (uint16_t)t;
  }
}

void zigzag_table(const uint16_t natural[64], uint16_t zz[64]) {
  for (int i = 0; i < 64; ++i) zz[i] = natural[kNatural[i]];
}

// ---- header (everything up to and including SOS), marker layout of libjpeg's jcmarker.c --------------------------------
namespace {
void put16(std::vector<uint8_t>& b, unsigned v) { b.push_back((uint8_t)(v >> 8)); b.push_back((uint8_t)v); }
void put_dqt(std::vector<uint8_t>& b, int idx, const uint16_t q[64]) {
  put16(b, 0xFFDB); put16(b, 67); b.push_back((uint8_t)idx);
  for (int i = 0; i < 64; ++i) b.push_back((uint8_t)q[kNatural[i]]);
}
void put_dht(std::vector<uint8_t>& b, int cls_idx, const uint8_t bits[16], const uint8_t* vals) {
  int n = 0;
  for (int i = 0; i < 16; ++i) n += bits[i];
  put16(b, 0xFFC4); put16(b, (unsigned)(19 + n)); b.push_back((uint8_t)cls_idx);
  b.insert(b.end(), bits, bits + 16);
  b.insert(b.end(), vals, vals + n);
}
}  // namespace

void build_header(int w, int h, Geometry geom, int quality, const void* icc, size_t icc_n, std::vector<uint8_t>& b, bool prefix_only,
                  uint32_t restart_interval, bool progressive) {
  const bool gray = geom == kGeomGray;
  uint16_t ql[64], qc[64];
  quant_table(quality, false, ql);
  quant_table(quality, true, qc);
  b.clear();
  put16(b, 0xFFD8);
  put16(b, 0xFFE0); put16(b, 16);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};  // 1.01, no units, 1:1, no thumbnail
  b.insert(b.end(), jfif, jfif + 14);
  if (icc != nullptr && icc_n > 0) {  // jpeg_write_marker(JPEG_APP0 + 2) right after jpeg_start_compress (:98-100)
    put16(b, 0xFFE2); put16(b, (unsigned)(icc_n + 2));
    b.insert(b.end(), static_cast<const uint8_t*>(icc), static_cast<const uint8_t*>(icc) + icc_n);
  }
  put_dqt(b, 0, ql);
  if (!gray) put_dqt(b, 1, qc);
  const int nc = gray ? 1 : 3;
  put16(b, progressive ? 0xFFC2 : 0xFFC0); put16(b, (unsigned)(8 + 3 * nc)); b.push_back(8); put16(b, (unsigned)h); put16(b, (unsigned)w);
  b.push_back((uint8_t)nc);
  for (int c = 0; c < nc; ++c) {
    b.push_back((uint8_t)(c + 1));
    b.push_back((uint8_t)(c == 0 ? (geom_hs(geom) << 4) | geom_vs(geom) : 0x11));
    b.push_back((uint8_t)(c == 0 ? 0 : 1));
  }
  if (prefix_only) return;   // DHT and SOS: write_opt_header's, in this order
  put_dht(b, 0x00, kBitsDcLum, kValsDc);
  put_dht(b, 0x10, kBitsAcLum, kValsAcLum);
  if (!gray) {
    put_dht(b, 0x01, kBitsDcChr, kValsDc);
    put_dht(b, 0x11, kBitsAcChr, kValsAcChr);
  }
  if (restart_interval != 0) { put16(b, 0xFFDD); put16(b, 4); put16(b, restart_interval); }   // jcmarker.c write_scan_header: emit_dri
  put16(b, 0xFFDA); put16(b, (unsigned)(6 + 2 * nc)); b.push_back((uint8_t)nc);
  for (int c = 0; c < nc; ++c) { b.push_back((uint8_t)(c + 1)); b.push_back((uint8_t)(c == 0 ? 0x00 : 0x11)); }
  b.push_back(0); b.push_back(63); b.push_back(0);
}

// ---- block geometry -----------------------------------------------------------------------------------------------
// Entropy-coding order (libjpeg jccoefct.c): one plane: blocks in raster order; 4:2:0: per MCU (16x16 pixels) Y00 Y01 Y10 Y11
// Cb Cr.  Blocks past the component's size in blocks are dummies: zero AC, DC of the block before them in the MCU.
// 4:4:4 from RGBA (Job::rgb): per MCU (8x8 pixels) Y Cb Cr, MCUs in raster order; no dummies.
// Planes of any other sampling (Job::hs, vs; the planar 4:4:4 among them): locate_sampled.
struct BlockRef {
  int comp;        // 0 Y, 1 Cb, 2 Cr
  int br, bc;      // block row / column inside the component (of the source block for a dummy)
  bool dummy;
};
__device__ __forceinline__ BlockRef locate_rgb(const Job& j, uint32_t i) {
  BlockRef b;
  const uint32_t mcu = i / 3u;
  b.comp = (int)(i - mcu * 3u);
  b.br = (int)(mcu / j.ybw); b.bc = (int)(mcu - (uint32_t)b.br * j.ybw); b.dummy = false;
  return b;
}
// three planes with luma sampling other than 2x2 (Job::hs, vs): per MCU hs * vs luma blocks in rows of hs, then Cb Cr -- 3 blocks
// (4:4:4, 8x8 pixels) or 4 (4:2:2, 16x8: Y0 Y1; 4:4:0, 8x16: Y0 above Y1).  The dummy rule is the 4:2:0 one: for 2x1 the right-hand
// block of the last MCU column when the luma width in blocks is odd, for 1x2 the bottom block of the last MCU row
__device__ __forceinline__ BlockRef locate_sampled(const Job& j, uint32_t i) {
  BlockRef b;
  const uint32_t nl = j.hs * j.vs;   // 1 or 2
  uint32_t mcu, k;
  if (nl == 1u) { mcu = i / 3u; k = i - mcu * 3u; }
  else { mcu = i >> 2; k = i & 3u; }
  const int mr = (int)(mcu / j.mcus_x), mc = (int)(mcu - (uint32_t)mr * j.mcus_x);
  if (k >= nl) { b.comp = (int)(k - nl) + 1; b.br = mr; b.bc = mc; b.dummy = false; return b; }
  b.comp = 0;
  b.br = (int)j.vs * mr + (j.vs == 2u ? (int)k : 0); b.bc = (int)j.hs * mc + (j.hs == 2u ? (int)k : 0);
  b.dummy = !(b.br < (int)j.ybh && b.bc < (int)j.ybw);
  if (b.dummy) { b.br = (int)j.vs * mr; b.bc = (int)j.hs * mc; }   // (only block 1 of two can be one; block 0 is always real)
  return b;
}
__device__ __forceinline__ BlockRef locate(const Job& j, uint32_t i) {
  BlockRef b;
  if (j.gray) {
    b.comp = 0; b.br = (int)(i / j.ybw); b.bc = (int)(i - (uint32_t)b.br * j.ybw); b.dummy = false;
    return b;
  }
  const uint32_t mcu = i / 6u, k = i - mcu * 6u;
  const int mr = (int)(mcu / j.mcus_x), mc = (int)(mcu - (uint32_t)mr * j.mcus_x);
  if (k >= 4u) { b.comp = (int)k - 3; b.br = mr; b.bc = mc; b.dummy = false; return b; }
  b.comp = 0;
  int kk = (int)k;
  b.br = 2 * mr + (kk >> 1); b.bc = 2 * mc + (kk & 1);
  b.dummy = !(b.br < (int)j.ybh && b.bc < (int)j.ybw);
  while (!(b.br < (int)j.ybh && b.bc < (int)j.ybw)) {  // a dummy inherits the DC of the block before it; block 0 is always real
    --kk;
    b.br = 2 * mr + (kk >> 1); b.bc = 2 * mc + (kk & 1);
  }
  return b;
}
// index of the previous block of the same component (DC prediction), or UINT32_MAX for the first one
__device__ __forceinline__ uint32_t dc_predecessor_sampled(const Job& j, uint32_t i) {   // 3 or 4 blocks per MCU (locate_sampled)
  if (j.hs * j.vs == 1u) return i < 3u ? 0xFFFFFFFFu : i - 3u;
  const uint32_t k = i & 3u;
  if (k == 1u) return i - 1u;
  if (i < 4u) return 0xFFFFFFFFu;
  return k == 0u ? i - 3u : i - 4u;   // Y1 of the previous MCU; its Cb or Cr
}
// ANY false: the caller knows the job to be none of locate_sampled's (the planar FDCT kernels)
template <bool ANY = true>
__device__ __forceinline__ uint32_t dc_predecessor(const Job& j, uint32_t i) {
  if (j.gray) return i == 0u ? 0xFFFFFFFFu : i - 1u;
  if (j.rgb) return i < 3u ? 0xFFFFFFFFu : i - 3u;
  if (ANY && j.sampled) return dc_predecessor_sampled(j, i);   // (uniform per job)
  const uint32_t mcu = i / 6u, k = i - mcu * 6u;
  if (k >= 4u) return mcu == 0u ? 0xFFFFFFFFu : i - 6u;
  if (k != 0u) return i - 1u;
  return mcu == 0u ? 0xFFFFFFFFu : i - 3u;  // Y11 of the previous MCU
}

// sample with the helper's padding rules (jpegencoderhelper.cpp:147-222, :239-278): rows past the height come from an
// all-zero row; columns past the width are zero when the row was copied into a zero-padded buffer (stride < aligned
// width) and the caller's bytes otherwise
__device__ __forceinline__ int sample(const Plane& p, int r, int c) {
  if (r >= p.h) return 0;
  if (c >= p.w && p.pad_cols) return 0;
  return p.p[(size_t)r * p.stride + c];
}

#define UJ_CONST_BITS 13
#define UJ_PASS1_BITS 2
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one 8-point pass of libjpeg's jfdctint.c ("islow"): in/out are 8 values with the given register stride
template <int PASS>
__device__ __forceinline__ void fdct8(int (&d)[64], int base, int stride) {
  const int d0 = d[base], d1 = d[base + stride], d2 = d[base + 2 * stride], d3 = d[base + 3 * stride];
  const int d4 = d[base + 4 * stride], d5 = d[base + 5 * stride], d6 = d[base + 6 * stride], d7 = d[base + 7 * stride];
  int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int sh = PASS == 0 ? UJ_CONST_BITS - UJ_PASS1_BITS : UJ_CONST_BITS + UJ_PASS1_BITS;
  if (PASS == 0) {
    d[base] = (tmp10 + tmp11) << UJ_PASS1_BITS;
    d[base + 4 * stride] = (tmp10 - tmp11) << UJ_PASS1_BITS;
  } else {
    d[base] = descale(tmp10 + tmp11, UJ_PASS1_BITS);
    d[base + 4 * stride] = descale(tmp10 - tmp11, UJ_PASS1_BITS);
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[base + 2 * stride] = descale(z1 + tmp13 * 6270, sh);
  d[base + 6 * stride] = descale(z1 + tmp12 * (-15137), sh);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  d[base + 7 * stride] = descale(tmp4 + z1 + z3, sh);
  d[base + 5 * stride] = descale(tmp5 + z2 + z4, sh);
  d[base + 3 * stride] = descale(tmp6 + z2 + z3, sh);
  d[base + stride] = descale(tmp7 + z1 + z4, sh);
}
// jcdctmgr.c: the 8x-scaled coefficient divided by (quant << 3), rounded half away from zero.  The division is a 32-bit
// multiply-high by m = floor(2^32 / qval) + 1: exact for 0 <= t < 2^16 because t * qval < 2^27 (|coefficient| <= 2^14,
// qval <= 2040); an integer division costs ~35 instructions, and there are 64 per block.
__device__ __forceinline__ int quantise(int v, int q, uint32_t m) {
  const int qval = q << 3;
  int t = v < 0 ? -v : v;
  t += qval >> 1;
  t = (int)__umulhi((uint32_t)t, m);
  return v < 0 ? -t : t;
}

// the 64 level-shifted samples of block b (of its source block for a dummy), with the helper's padding rules
// REPL: the plane may ask for libjpeg's own edge expansion (kPadReplicate) -- planes of the sampled jobs alone, so that the 4:2:0 and
// one-plane kernels carry none of its code
template <bool REPL = false>
__device__ __forceinline__ void load_samples(const Plane& p, const BlockRef& b, int (&d)[64]) {
  const int r0 = b.br * 8, c0 = b.bc * 8;
  const bool inside = r0 + 8 <= p.h && (c0 + 8 <= p.w || !p.pad_cols);
  if (inside && p.aligned4) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint32_t* row = reinterpret_cast<const uint32_t*>(p.p + (size_t)(r0 + r) * p.stride + c0);
      const uint32_t a = row[0], bq = row[1];
      d[r * 8 + 0] = (int)(a & 0xff) - 128; d[r * 8 + 1] = (int)((a >> 8) & 0xff) - 128;
      d[r * 8 + 2] = (int)((a >> 16) & 0xff) - 128; d[r * 8 + 3] = (int)(a >> 24) - 128;
      d[r * 8 + 4] = (int)(bq & 0xff) - 128; d[r * 8 + 5] = (int)((bq >> 8) & 0xff) - 128;
      d[r * 8 + 6] = (int)((bq >> 16) & 0xff) - 128; d[r * 8 + 7] = (int)(bq >> 24) - 128;
    }
  } else if (REPL && p.pad_cols == kPadReplicate) {   // libjpeg's expand_right_edge, then its bottom-edge rows, on the plane's own grid
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint8_t* row = p.p + (size_t)min(r0 + r, p.h - 1) * p.stride;
#pragma unroll
      for (int c = 0; c < 8; ++c) d[r * 8 + c] = (int)row[min(c0 + c, p.w - 1)] - 128;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) d[r * 8 + c] = sample(p, r0 + r, c0 + c) - 128;
  }
}

// the same for component b.comp of an RGBA image (p: the pixels, 4-byte aligned, stride in bytes): jccolor.c's fixed-point RGB ->
// YCbCr per sample; a block over the right or bottom edge repeats the last column, then the last row (libjpeg's expand_right_edge /
// expand_bottom_edge -- on converted samples there, which is the conversion of the repeated pixel)
__device__ __forceinline__ void load_samples_rgb(const Plane& p, const BlockRef& b, int (&d)[64]) {
  const int r0 = b.br * 8, c0 = b.bc * 8;
  const int kr = b.comp == 0 ? 19595 : b.comp == 1 ? -11059 : 32768;
  const int kg = b.comp == 0 ? 38470 : b.comp == 1 ? -21709 : -27439;
  const int kb = b.comp == 0 ? 7471 : b.comp == 1 ? 32768 : -5329;
  const int bias = b.comp == 0 ? 32768 : (128 << 16) + 32767;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int rr = min(r0 + r, p.h - 1);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(p.p + (size_t)rr * p.stride);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint32_t px = row[min(c0 + c, p.w - 1)];
      const int v = kr * (int)(px & 0xffu) + kg * (int)((px >> 8) & 0xffu) + kb * (int)((px >> 16) & 0xffu) + bias;
      d[r * 8 + c] = (v >> 16) - 128;
    }
  }
}

// ---- entropy coding ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int nbits_of(int a) { return a == 0 ? 0 : 32 - __builtin_clz((unsigned)a); }

// walks one block's symbols (jchuff.c encode_one_block); SINK::put(code, size) receives MSB-first bit strings.
// c: the block's 64 quantised coefficients in zigzag order (registers: every index is a compile-time constant)
// HUFF: where a symbol's code comes from, asked once per symbol emitted -- the default tables in constant memory, a job's own tables
// in LDS (LdsHuff), or nowhere: HistHuff counts the symbol instead
struct ConstHuff {
  __device__ __forceinline__ uint32_t operator()(int tbl, int sym) const { return c_huff[tbl][sym]; }
};
struct LdsHuff {
  static __device__ __forceinline__ uint32_t* table() {   // 4 x 256, the workgroup's one copy (load_job_huff fills it)
    __shared__ uint32_t t[4 * 256];
    return t;
  }
  __device__ __forceinline__ uint32_t operator()(int tbl, int sym) const { return table()[tbl * 256 + sym]; }
};
struct HistHuff {
  uint32_t* hist;      // 4 x 256 counters in LDS
  __device__ __forceinline__ uint32_t operator()(int tbl, int sym) const { atomicAdd(&hist[tbl * 256 + sym], 1u); return 0u; }
};
template <typename SINK, typename HUFF = ConstHuff>
__device__ __forceinline__ void walk_coefs(const int16_t (&c)[64], int pred, int tbl_dc, int tbl_ac, SINK& s, const HUFF huff = HUFF()) {
  int temp = (int)c[0] - pred, temp2 = temp;
  if (temp < 0) { temp = -temp; temp2--; }
  int nb = nbits_of(temp);
  uint32_t h = huff(tbl_dc, nb);
  s.put(h & 0xffffu, (int)(h >> 16));
  if (nb) s.put((uint32_t)temp2 & ((1u << nb) - 1u), nb);
  int r = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    temp = c[k];
    if (temp == 0) { r++; continue; }
    while (r > 15) { h = huff(tbl_ac, 0xF0); s.put(h & 0xffffu, (int)(h >> 16)); r -= 16; }
    temp2 = temp;
    if (temp < 0) { temp = -temp; temp2--; }
    nb = nbits_of(temp);
    h = huff(tbl_ac, (r << 4) + nb);
    s.put(((h & 0xffffu) << nb) | ((uint32_t)temp2 & ((1u << nb) - 1u)), (int)(h >> 16) + nb);   // <= 16 + 10 bits
    r = 0;
  }
  if (r > 0) { h = huff(tbl_ac, 0); s.put(h & 0xffffu, (int)(h >> 16)); }
}
template <typename SINK, typename HUFF = ConstHuff>
__device__ __forceinline__ void walk_block(const int16_t* __restrict__ zz, int pred, int tbl_dc, int tbl_ac, SINK& s, const HUFF huff = HUFF()) {
  int16_t c[64];
#pragma unroll
  for (int k = 0; k < 8; ++k) {   // 128 B per block
    const uint4 v = reinterpret_cast<const uint4*>(zz)[k];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) { c[8 * k + 2 * m] = (int16_t)(w[m] & 0xffffu); c[8 * k + 2 * m + 1] = (int16_t)(w[m] >> 16); }
  }
  walk_coefs(c, pred, tbl_dc, tbl_ac, s, huff);
}

struct CountSink {
  uint32_t bits = 0;
  __device__ __forceinline__ void put(uint32_t, int size) { bits += (uint32_t)size; }
};

__device__ __forceinline__ int pred_of(const Job& j, uint32_t i) {
  const uint32_t p = dc_predecessor(j, i);
  return p == 0xFFFFFFFFu ? 0 : (int)j.coef[(size_t)p * 64u];
}
// a job with restart intervals (Job::rst_blocks): the prediction of every component starts again at 0 with the interval -- its first MCU's
// chroma blocks and first luma block have no predecessor; the other luma blocks of an MCU (three for 4:2:0, one for 4:2:2 and 4:4:0)
// chain inside it as ever.  The chroma blocks are the MCU's last two -- all but the first of three, and the only block of one plane
__device__ __forceinline__ int pred_of_rst(const Job& j, uint32_t i) {
  const uint32_t r = i % j.rst_blocks;
  if (r < j.rst_bpm && (r == 0u || r + 2u >= j.rst_bpm)) return 0;
  return pred_of(j, i);
}
// ANY false: the caller knows the job to be none of locate_sampled's (the planar FDCT kernels)
template <bool ANY = true>
__device__ __forceinline__ int comp_of(const Job& j, uint32_t i) {
  if (j.rgb) return (i % 3u) == 0u ? 0 : 1;
  if (ANY && j.sampled) return j.hs * j.vs == 2u ? ((i & 3u) < 2u ? 0 : 1) : ((i % 3u) == 0u ? 0 : 1);   // (uniform per job)
  return j.gray ? 0 : ((i % 6u) < 4u ? 0 : 1);
}

// One thread per 8x8 block: forward DCT, quantisation, the block's 64 coefficients to memory (zigzag order) -- and, while they are
// in registers, the number of bits its Huffman code takes (the prefix sum of those is where k_jpeg_emit writes).  The DC code needs
// the quantised DC of the component's previous block, which another thread computes: the islow DC is the plain sum of the 64
// level-shifted samples (pass 1 scales the row sums by 4, pass 2 descales by 4: exact), so it is had from that block's 64 bytes.
// KIND: what the job is -- 4:2:0 or one plane (kKindPlanar), 4:4:4 from RGBA pixels (kKindRgb, Job::rgb) or three planes of another
// sampling (kKindSampled, Job::hs, vs) --, known at compile time so that the planar kernels carry none of the others' code
// COUNT false (a job with optimised tables): the coefficients alone -- the block's bits wait for its tables (k_jpeg_opt_count_batch)
constexpr int kKindPlanar = 0, kKindRgb = 1, kKindSampled = 2;
__device__ __forceinline__ int kind_of(const Job& j) { return j.rgb ? kKindRgb : j.sampled ? kKindSampled : kKindPlanar; }
template <int KIND, bool COUNT = true>
__device__ __forceinline__ uint32_t fdct_quant_count_block(const Job& j, const uint32_t i);
// workgroup wg of the image's grid (blockIdx.x of the single-image launch; the batched launch passes its workgroup inside the job)
template <int KIND>
__device__ __forceinline__ void fdct_quant_count_wg(const Job& j, const uint32_t wg) {
  const uint32_t i = wg * 128u + threadIdx.x;
  __shared__ uint32_t s_part[2];
  uint32_t my_bits = 0;
  if (i < j.nblk) my_bits = fdct_quant_count_block<KIND>(j, i);
  // bits_blk[g]: the bits of workgroup g's 128 blocks.  k_jpeg_emit needs the bit offset of every block: inside a workgroup a block
  // scan, across workgroups the sum of the totals in front (a 4K frame has 1519), formed by every workgroup of the emit for itself
  const uint32_t total = block_sum<128>(my_bits, s_part);
  if (threadIdx.x == 0u) j.bits_blk[wg] = total;
}
__global__ void __launch_bounds__(128) k_jpeg_fdct_quant_count(const Job j) { fdct_quant_count_wg<kKindPlanar>(j, blockIdx.x); }

// the work of one thread of k_jpeg_fdct_quant_count: block i's coefficients to memory, its number of bits returned
template <int KIND, bool COUNT>
__device__ __forceinline__ uint32_t fdct_quant_count_block(const Job& j, const uint32_t i) {
  constexpr bool RGB = KIND == kKindRgb, SAMPLED = KIND == kKindSampled;
  const BlockRef b = RGB ? locate_rgb(j, i) : SAMPLED ? locate_sampled(j, i) : locate(j, i);
  const Plane& p = j.plane[RGB ? 0 : b.comp];
  const uint16_t* q = b.comp == 0 ? j.q_lum : j.q_chr;   // zigzag order
  const uint32_t* qm = b.comp == 0 ? j.m_lum : j.m_chr;
  int16_t* out = j.coef + (size_t)i * 64u;
  int d[64];
  if (RGB) load_samples_rgb(p, b, d);
  else load_samples<SAMPLED>(p, b, d);
  int16_t c[64];
  if (b.dummy) {  // zero AC, DC of the source block
    int s = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) s += d[k];
#pragma unroll
    for (int k = 1; k < 64; ++k) c[k] = 0;
    c[0] = (int16_t)quantise(s, q[0], qm[0]);
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<0>(d, r * 8, 1);
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) fdct8<1>(d, cc, 8);
    constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      if (COUNT) {
        c[k] = (int16_t)quantise(d[nat[k]], q[k], qm[k]);
      } else {
        // both tables' entries through the scalar unit and a select per lane: q and qm differ from lane to lane, so q[k] and qm[k]
        // are 128 vector loads in flight at once -- 182 VGPRs in this form of the kernel, 118 with the entries in SGPRs
        const int ql = __builtin_amdgcn_readfirstlane((int)j.q_lum[k]), qc = __builtin_amdgcn_readfirstlane((int)j.q_chr[k]);
        const uint32_t ml = __builtin_amdgcn_readfirstlane(j.m_lum[k]), mc = __builtin_amdgcn_readfirstlane(j.m_chr[k]);
        c[k] = (int16_t)quantise(d[nat[k]], b.comp == 0 ? ql : qc, b.comp == 0 ? ml : mc);
      }
    }
  }
  uint4* o = reinterpret_cast<uint4*>(out);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint32_t w[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) w[m] = (uint32_t)(uint16_t)c[8 * k + 2 * m] | ((uint32_t)(uint16_t)c[8 * k + 2 * m + 1] << 16);
    o[k] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (!COUNT) return 0u;
  int pred = 0;
  const uint32_t pi = SAMPLED ? dc_predecessor_sampled(j, i) : dc_predecessor<false>(j, i);
  if (pi != 0xFFFFFFFFu) {
    int e[64];
    if (RGB) load_samples_rgb(p, locate_rgb(j, pi), e);
    else if (SAMPLED) load_samples<true>(p, locate_sampled(j, pi), e);
    else load_samples(p, locate(j, pi), e);   // (the same component, so the same plane and quantiser)
    int s = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) s += e[k];
    pred = (int)(int16_t)quantise(s, q[0], qm[0]);
  }
  const int chroma = comp_of<SAMPLED>(j, i);
  CountSink cs;
  walk_coefs(c, pred, 2 * chroma, 2 * chroma + 1, cs);
  j.bits[i] = cs.bits;
  return cs.bits;
}

// MSB-first writer into a zero-initialised word buffer that other threads write next to: whole words are stored, the first
// and the last (partial) word are OR-ed atomically.  Words are kept big-endian in memory so that the buffer is the byte stream.
struct EmitSink {
  uint32_t* words;
  uint64_t acc;
  int nacc;       // valid low bits of acc (includes the leading alignment zeros at the start)
  uint32_t wi;    // next word index
  bool first;
  __device__ __forceinline__ void flush_word(uint32_t w, bool atomic) {
    const uint32_t be = __builtin_bswap32(w);
    if (atomic) atomicOr(&words[wi], be);
    else words[wi] = be;
    ++wi;
  }
  __device__ __forceinline__ void put(uint32_t code, int size) {
    acc = (acc << size) | (uint64_t)code;
    nacc += size;
    if (nacc >= 32) {
      flush_word((uint32_t)(acc >> (nacc - 32)), first);
      first = false;
      nacc -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nacc > 0) flush_word((uint32_t)(acc << (32 - nacc)), true);
  }
};

// RST (a job with restart intervals): Job::bits of an interval's last block holds its padding and its marker too (k_jpeg_rst_adjust_batch),
// so the offsets are the same plain sum; that block fills its byte with ones, writes RSTn behind it and says where the marker stands
template <typename HUFF = ConstHuff, bool RST = false>
__device__ __forceinline__ void emit_wg(const Job& j, const uint32_t wg) {
  __shared__ uint64_t s_part[2];
  __shared__ uint64_t s_base;
  const uint32_t i = wg * 128u + threadIdx.x;
  uint64_t before = 0;
  for (uint32_t g = threadIdx.x; g < wg; g += 128u) before += j.bits_blk[g];
  before = block_sum<128>(before, s_part);
  if (threadIdx.x == 0u) s_base = before;
  __syncthreads();
  const uint64_t my_bits = i < j.nblk ? j.bits[i] : 0u;
  const uint64_t in_front = block_exclusive_sum<128>(my_bits, s_part);
  if (i >= j.nblk) return;
  const uint64_t off = s_base + in_front;
  if (i == j.nblk - 1u) *j.total_bits = off + my_bits;   // read by the stuffing kernels behind this one
  EmitSink s;
  s.words = j.stream;
  s.acc = 0;
  s.nacc = (int)(off & 31u);   // bits of this word that belong to earlier blocks: zeros here, OR-ed there
  s.wi = (uint32_t)(off >> 5);
  s.first = true;
  const int chroma = comp_of(j, i);
  walk_block(j.coef + (size_t)i * 64u, RST ? pred_of_rst(j, i) : pred_of(j, i), 2 * chroma, 2 * chroma + 1, s, HUFF());
  if (RST && i != j.nblk - 1u && (i + 1u) % j.rst_blocks == 0u) {   // jchuff.c emit_restart: flush_bits, then the marker
    const int pad = (8 - (s.nacc & 7)) & 7;   // (words are whole bytes: the sink's position in its word is the stream's in its byte)
    if (pad) s.put((1u << pad) - 1u, pad);
    const uint32_t t = i / j.rst_blocks;
    s.put(0xFFD0u | (t & 7u), 16);
    j.rst_mark[t] = (uint32_t)((off + my_bits) >> 3) - 2u;
  }
  if (i == j.nblk - 1u) {      // jchuff.c flush_bits: fill the last byte with ones
    const uint64_t end = off + my_bits;
    const int pad = (int)((8u - (uint32_t)(end & 7u)) & 7u);
    if (pad) s.put((1u << pad) - 1u, pad);
  }
  s.finish();
}
__global__ void __launch_bounds__(128) k_jpeg_emit(const Job j) { emit_wg(j, blockIdx.x); }

// ---- byte stuffing -------------------------------------------------------------------------------------------------
constexpr uint32_t kChunk = 64;
// ff_count[t]: 0xFF bytes in chunk t; ff_blk[g]: in the 256 chunks of workgroup g.  The copy needs the number of stuffed zeros in
// front of every chunk: inside a workgroup a block scan of 256 counts, across workgroups the sum of the totals in front, which
// every workgroup of the copy forms for itself (a 4K frame has ~100 of them) -- no device-wide scan between the two kernels.
// RST (a job with restart intervals): the 0xFF of an RSTn marker is no data byte and gets no zero.  The bytes cannot tell -- a data
// 0xFF in front of a data 0xD0..0xD7 occurs --, so the emit left the markers' offsets in Job::rst_mark, ascending: a chunk looks up
// the first one at or behind its start and walks on from there.
__device__ __forceinline__ uint32_t first_mark_from(const Job& j, uint32_t b) {
  uint32_t lo = 0, hi = j.rst_marks;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (j.rst_mark[mid] < b) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}
template <bool RST = false>
__device__ __forceinline__ void stuff_count_wg(const Job& j, const uint64_t* total_bits, const uint32_t wg) {
  __shared__ uint32_t s_part[4];
  const uint32_t t = wg * 256u + threadIdx.x;
  const uint64_t nbytes = (*total_bits + 7u) >> 3;
  const uint64_t b0 = (uint64_t)t * kChunk;
  if ((uint64_t)wg * 256u * kChunk >= nbytes) return;   // uniform per workgroup: behind the end of the stream
  uint32_t n = 0;
  if (t < j.max_chunks && b0 < nbytes) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(j.stream) + b0;
    const uint32_t len = (uint32_t)(nbytes - b0 < kChunk ? nbytes - b0 : kChunk);
    if (RST) {
      uint32_t mi = first_mark_from(j, (uint32_t)b0);
      uint32_t next = mi < j.rst_marks ? j.rst_mark[mi] : 0xFFFFFFFFu;
      for (uint32_t k = 0; k < len; ++k) {
        if (p[k] != 0xFFu) continue;
        if ((uint32_t)b0 + k != next) { ++n; continue; }
        ++mi;
        next = mi < j.rst_marks ? j.rst_mark[mi] : 0xFFFFFFFFu;
      }
    } else {
      for (uint32_t k = 0; k < len; ++k) n += p[k] == 0xFFu;
    }
    j.ff_count[t] = n;
  }
  const uint32_t total = block_sum<256>(n, s_part);
  if (threadIdx.x == 0u) j.ff_blk[wg] = total;
}
__global__ void __launch_bounds__(256) k_jpeg_stuff_count(const Job j, const uint64_t* total_bits) { stuff_count_wg(j, total_bits, blockIdx.x); }
// One workgroup = 256 chunks = 16 KiB of the packed stream.  Every thread expands its chunk into LDS (0x00 after each
// 0xFF), then the workgroup writes the expanded run to the output as aligned dwords: the run's start in the output is
// arbitrary (header length + stuffed bytes before it), so a thread per chunk writing its own bytes would scatter byte
// stores over 256 cache lines per instruction (28 us per 4K frame measured; this form: see DESIGN.md).
template <bool RST = false>
__device__ __forceinline__ void stuff_copy_wg(const Job& j, const uint64_t* total_bits, uint8_t* out, uint64_t out_cap, uint64_t header_len,
                                              uint64_t* out_size, const uint32_t wg) {
  __shared__ uint32_t s_part[4];
  __shared__ uint8_t s_buf[256 * kChunk * 2 + 8];
  __shared__ uint32_t s_len, s_base;
  const uint32_t first = wg * 256u, t = first + threadIdx.x;
  const uint64_t nbytes = (*total_bits + 7u) >> 3;
  const uint64_t blk_b0 = (uint64_t)first * kChunk;
  if (blk_b0 >= nbytes) return;                       // uniform per workgroup
  uint32_t before = 0;
  for (uint32_t g = threadIdx.x; g < wg; g += 256u) before += j.ff_blk[g];
  before = block_sum<256>(before, s_part);
  if (threadIdx.x == 0) { s_len = 0u; s_base = before; }
  __syncthreads();
  const uint32_t base_ff = s_base;
  const uint64_t b0 = (uint64_t)t * kChunk;
  const bool mine = t < j.max_chunks && b0 < nbytes;
  const uint32_t ff_before = block_exclusive_sum<256>(mine ? j.ff_count[t] : 0u, s_part);
  if (mine) {
    const uint32_t len = (uint32_t)(nbytes - b0 < kChunk ? nbytes - b0 : kChunk);
    uint32_t lo = (uint32_t)(b0 - blk_b0) + ff_before;
    const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(j.stream) + b0);
    uint32_t mi = 0, next = 0xFFFFFFFFu;   // RST: the next marker at or behind this byte (stuff_count_wg)
    if (RST) {
      mi = first_mark_from(j, (uint32_t)b0);
      if (mi < j.rst_marks) next = j.rst_mark[mi];
    }
#pragma unroll
    for (uint32_t q = 0; q < kChunk / 16u; ++q) {
      const uint4 v = src[q];                         // (reads up to 15 bytes past len inside the zeroed workspace)
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t k = 0; k < 16u; ++k) {
        if (q * 16u + k < len) {
          const uint8_t by = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
          s_buf[lo++] = by;
          if (RST) {
            if (by == 0xFFu) {
              if ((uint32_t)b0 + q * 16u + k != next) {
                s_buf[lo++] = 0;
              } else {
                ++mi;
                next = mi < j.rst_marks ? j.rst_mark[mi] : 0xFFFFFFFFu;
              }
            }
          } else {
            if (by == 0xFFu) s_buf[lo++] = 0;
          }
        }
      }
    }
    const bool last_of_stream = b0 + len == nbytes;
    if (last_of_stream) { s_buf[lo++] = 0xFF; s_buf[lo++] = 0xD9; }   // EOI
    if (last_of_stream || threadIdx.x == 255u) s_len = lo;
    if (last_of_stream) *out_size = header_len + blk_b0 + base_ff + lo;
  }
  __syncthreads();
  const uint32_t len = s_len;
  const uint64_t dst0 = header_len + blk_b0 + base_ff;              // offset of s_buf[0] in the output
  const uint32_t head = (uint32_t)((4u - ((reinterpret_cast<uintptr_t>(out) + dst0) & 3u)) & 3u);
  const uint32_t head_n = head < len ? head : len;
  if (threadIdx.x < head_n && dst0 + threadIdx.x < out_cap) out[dst0 + threadIdx.x] = s_buf[threadIdx.x];
  const uint32_t nwords = (len - head_n) >> 2;
  for (uint32_t k = threadIdx.x; k < nwords; k += 256u) {
    const uint32_t o = head_n + 4u * k;
    const uint32_t v = (uint32_t)s_buf[o] | ((uint32_t)s_buf[o + 1] << 8) | ((uint32_t)s_buf[o + 2] << 16) | ((uint32_t)s_buf[o + 3] << 24);
    if (dst0 + o + 4u <= out_cap) *reinterpret_cast<uint32_t*>(out + dst0 + o) = v;
    else for (uint32_t m = 0; m < 4u; ++m) if (dst0 + o + m < out_cap) out[dst0 + o + m] = s_buf[o + m];
  }
  const uint32_t tail0 = head_n + 4u * nwords;
  if (threadIdx.x < len - tail0 && dst0 + tail0 + threadIdx.x < out_cap) out[dst0 + tail0 + threadIdx.x] = s_buf[tail0 + threadIdx.x];
}
__global__ void __launch_bounds__(256) k_jpeg_stuff_copy(const Job j, const uint64_t* total_bits, uint8_t* out, uint64_t out_cap,
                                                         uint64_t header_len, uint64_t* out_size) {
  stuff_copy_wg(j, total_bits, out, out_cap, header_len, out_size, blockIdx.x);
}

// ---- batched form ---------------------------------------------------------------------------------------------------
// All JPEGs of a call -- colour and grey, large and small -- share one launch per encoder step.  The grid is the concatenation of
// the jobs' own grids: job k owns workgroups [start[k], start[k + 1]), so a gain map (64 workgroups at 4K) does not dispatch the
// 1519 of its SDR image.  A Job is ~900 B, so the descriptors are read from device memory rather than the kernarg segment; the
// per-workgroup bodies are the single-image kernels' own, so both forms write the same bytes.
// The workgroup's job: the starts into LDS with one round of loads, a binary search there (<= 7 steps), the result made uniform.
template <int NT>
__device__ __forceinline__ uint32_t job_of(const uint32_t* __restrict__ start, uint32_t n, uint32_t* first, uint32_t* count) {
  __shared__ uint32_t s_start[kMaxBatchJobs + 1];
  for (uint32_t t = threadIdx.x; t <= n; t += NT) s_start[t] = start[t];
  __syncthreads();
  const uint32_t g = blockIdx.x;
  uint32_t lo = 0, hi = n;   // s_start[lo] <= g < s_start[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_start[mid] <= g) lo = mid;
    else hi = mid;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);
  *first = s_start[lo];
  *count = s_start[lo + 1u] - s_start[lo];
  return lo;
}
// the job's descriptor through the constant address space: its fields (the 128 quantisation entries and multipliers among them) are
// read with scalar loads into SGPRs, as from the single-image kernels' kernarg segment, instead of into VGPRs
template <class T>
__device__ __forceinline__ const T& uniform_ref(const T* p, uint32_t k) {
  return *(const T*)((const __attribute__((address_space(4))) T*)p + k);
}

__global__ void __launch_bounds__(128) k_jpeg_fdct_quant_count_multi(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (j.rgb | j.sampled) return;   // (uniform per workgroup) k_jpeg_fdct_quant_count_multi_rgb's or _sampled's
  fdct_quant_count_wg<kKindPlanar>(j, blockIdx.x - first);
}
// the 4:4:4 jobs of the same grid; the two kernels are launched as the batch holds jobs of either kind
__global__ void __launch_bounds__(128) k_jpeg_fdct_quant_count_multi_rgb(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (!j.rgb) return;
  fdct_quant_count_wg<kKindRgb>(j, blockIdx.x - first);
}
// and the jobs of three planes with 1x1, 2x1 or 1x2 luma sampling
__global__ void __launch_bounds__(128) k_jpeg_fdct_quant_count_multi_sampled(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (kind_of(j) != kKindSampled) return;
  fdct_quant_count_wg<kKindSampled>(j, blockIdx.x - first);
}

// The single-image path clears the whole worst-case stream area (208 B per block, 40 MB for a 4K frame) before the emit ORs into
// it.  Here every workgroup clears the words whose first bit falls into its own blocks' bit range [before, before + bits): over a
// job's workgroups that is exactly the words [0, ceil(total_bits / 32)) the emit writes, the padding of the last byte included.
__global__ void __launch_bounds__(128) k_jpeg_clear_multi(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint64_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint32_t wg = blockIdx.x - first;
  uint64_t before = 0;
  for (uint32_t g = threadIdx.x; g < wg; g += 128u) before += j.bits_blk[g];
  before = block_sum<128>(before, s_part);
  const uint64_t end = before + j.bits_blk[wg];
  const uint64_t w1 = (end + 31u) >> 5;
  for (uint64_t w = ((before + 31u) >> 5) + threadIdx.x; w < w1; w += 128u) j.stream[w] = 0u;
}

__global__ void __launch_bounds__(128) k_jpeg_emit_multi(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  emit_wg(uniform_ref(jobs, k), blockIdx.x - first);
}

// The stuffing grid of a job cannot be sized by its stream, which is only known on the device: each job gets up to
// kStuffWgPerJob workgroups, and they walk the stream's 16 KiB pieces with that stride until its end.
__global__ void __launch_bounds__(256) k_jpeg_stuff_count_multi(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_count_wg(j, j.total_bits, wg);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_jpeg_stuff_copy_multi(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs,
                                                               const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const BatchOut& o = uniform_ref(outs, k);
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_copy_wg(j, j.total_bits, o.out, o.out_cap, o.header_len, o.out_size, wg);
    __syncthreads();   // (s_buf and s_len are the next piece's)
  }
}

// ---- optimised Huffman tables (Job::optimize) ------------------------------------------------------------------------------------
// libjpeg's optimize_coding for the jobs of a round that ask for it, without a word to the host: the code lengths follow from a
// histogram of the whole image, so these jobs run through launches of their own (the default jobs keep theirs, untouched):
//   k_jpeg_opt_zero_batch        the job's 4 x 256 counters to zero
//   k_jpeg_opt_fdct_batch        k_jpeg_fdct_quant_count_multi's coefficients, without the count
//   k_jpeg_opt_hist_batch        the symbols walk_coefs codes are counted -- per workgroup in LDS, then one global atomic per non-zero bin
//   k_jpeg_opt_tables_batch      one workgroup per job, one wave per table: jpeg_gen_optimal_table, the canonical codes into the job's
//                                workspace, the DHT and SOS segments behind the host's prefix, the header's length into a device word
//   k_jpeg_opt_count_batch       bits per block and per workgroup from the job's codes (the coefficients are read again)
//   k_jpeg_clear_multi, k_jpeg_opt_emit_batch, k_jpeg_stuff_count_multi, k_jpeg_opt_stuff_copy_batch
//                                the default steps, with the job's codes in LDS and the stream behind the device's header length
struct TableLds {
  uint32_t bits[33];                        // codes per length (index = length); the pseudo-symbol is in it until build_table takes it out
  uint32_t first_code[17], first_rank[17];  // per final length: its first code and that code's position in HUFFVAL
  uint32_t nvals, overflow;
  uint8_t size[256];                        // each symbol's code length before the limit (0: not in the table)
  uint8_t vals[256];                        // HUFFVAL
};
// the wave's two smallest keys (distinct but for the "none" of all ones), each lane giving its own two (k1 <= k2): one butterfly of
// six shuffle rounds for both instead of two in a row
__device__ __forceinline__ void wave_min2(uint64_t& k1, uint64_t& k2) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t u1 = __shfl_xor(k1, off, 64), u2 = __shfl_xor(k2, off, 64);
    const uint64_t lo = k1 < u1 ? k1 : u1, hi = k1 < u1 ? u1 : k1, nx = k2 < u2 ? k2 : u2;
    k1 = lo;
    k2 = hi < nx ? hi : nx;
  }
}
// jpeg_gen_optimal_table (jchuff.c) of the 256 counts at freq, by one wave; every wave of the workgroup calls it, since the barriers
// are the workgroup's -- a wave with active == false builds nothing.  Lane l holds the entries l, l + 64, ... (256, the pseudo-symbol
// of count 1 that keeps the all-ones code free, is lane 0's fifth) in registers, every index a compile-time constant.
// libjpeg merges the two least frequent trees (of equal counts the one with the LARGEST index) and walks their symbols along a chain
// to lengthen each by a bit; here a symbol carries the index of its tree's head, and every lane lengthens its members of the two.
// Leaves L.bits[1..16], L.vals[0, L.nvals) and, at huff (or nullptr), the 256 canonical codes; returns true, and no table, where
// a code would be longer than 32 bits (libjpeg: JERR_HUFF_CLEN_OVERFLOW).
__device__ __forceinline__ bool build_table(const uint32_t* __restrict__ freq, const bool active, TableLds& L, uint32_t* __restrict__ huff) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t f[5], size[5], head[5];
#pragma unroll
  for (uint32_t s = 0; s < 5u; ++s) {
    const uint32_t idx = lane + 64u * s;
    f[s] = (active && idx < 256u) ? freq[idx] : 0u;
    size[s] = 0u;
    head[s] = idx;
  }
  if (active && lane == 0u) f[4] = 1u;
  if (lane < 33u) L.bits[lane] = 0u;
  if (lane == 0u) { L.overflow = 0u; L.nvals = 0u; }
  const uint64_t none = ~0ull;
  while (active) {   // (uniform per wave)
    uint64_t k1 = none, k2 = none;
    for (uint32_t s = 0; s < 5u; ++s) {   // smallest count, then largest index: the key's low half falls as the index rises
      const uint64_t key = (f[s] != 0u && f[s] <= kHuffFreqLimit) ? ((uint64_t)f[s] << 16) | (uint64_t)(0xFFFFu - (lane + 64u * s)) : none;
      if (key < k1) { k2 = k1; k1 = key; }
      else if (key < k2) k2 = key;
    }
    wave_min2(k1, k2);
    if (k2 == none) break;   // one tree left
    const uint32_t c1 = 0xFFFFu - (uint32_t)(k1 & 0xFFFFu), c2 = 0xFFFFu - (uint32_t)(k2 & 0xFFFFu);
    const uint32_t sum = (uint32_t)(k1 >> 16) + (uint32_t)(k2 >> 16);   // both <= 10^9: no overflow
#pragma unroll
    for (uint32_t s = 0; s < 5u; ++s) {
      const uint32_t idx = lane + 64u * s;
      if (idx == c1) f[s] = sum;
      if (idx == c2) f[s] = 0u;
      if (head[s] == c1 || head[s] == c2) ++size[s];
      if (head[s] == c2) head[s] = c1;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t s = 0; s < 5u; ++s) {
    const uint32_t idx = lane + 64u * s;
    const uint32_t z = size[s] > 32u ? 32u : size[s];
    if (size[s] > 32u) L.overflow = 1u;
    if (z != 0u) atomicAdd(&L.bits[z], 1u);
    if (idx < 256u) L.size[idx] = (uint8_t)z;
  }
  __syncthreads();
  const bool overflow = L.overflow != 0u;
  // HUFFVAL lists the symbols by length (before the limit), then by value: a symbol's place is the number of symbols in front of it
  uint32_t rank[4] = {0u, 0u, 0u, 0u};
  if (active && !overflow) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(L.size);
    for (uint32_t w = 0; w < 64u; ++w) {
      const uint32_t v = sw[w];
#pragma unroll
      for (uint32_t b = 0; b < 4u; ++b) {
        const uint32_t zz = (v >> (8u * b)) & 0xffu, jj = 4u * w + b;
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s)
          rank[s] += (zz != 0u && (zz < size[s] || (zz == size[s] && jj < lane + 64u * s))) ? 1u : 0u;
      }
    }
    if (lane == 0u) {   // the length limit (T.81 K.2, figure K.3), the pseudo-symbol out of the longest length, the canonical codes' starts
      for (int i = 32; i > 16; --i) {
        while (L.bits[i] >= 2u) {   // (the deepest level of a code tree holds pairs)
          int jn = i - 2;
          while (jn > 0 && L.bits[jn] == 0u) --jn;
          L.bits[i] -= 2u; L.bits[i - 1] += 1u; L.bits[jn + 1] += 2u; L.bits[jn] -= 1u;
        }
      }
      int i = 16;
      while (i > 0 && L.bits[i] == 0u) --i;
      if (i > 0) L.bits[i] -= 1u;
      uint32_t code = 0u, p = 0u;
      for (int l = 1; l <= 16; ++l) {
        L.first_code[l] = code; L.first_rank[l] = p;
        code = (code + L.bits[l]) << 1;
        p += L.bits[l];
      }
      L.nvals = p;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t s = 0; s < 4u; ++s) {
    const uint32_t idx = lane + 64u * s;
    uint32_t hv = 0u;
    if (active && !overflow && size[s] != 0u) {
      const uint32_t r = rank[s];
      L.vals[r] = (uint8_t)idx;
      for (uint32_t l = 1; l <= 16u; ++l)
        if (r >= L.first_rank[l] && r - L.first_rank[l] < L.bits[l]) hv = (l << 16) | (L.first_code[l] + r - L.first_rank[l]);
    }
    if (active && huff != nullptr) huff[idx] = hv;
  }
  __syncthreads();
  return overflow;
}

__global__ void __launch_bounds__(256) k_jpeg_opt_zero_batch(const Job* __restrict__ jobs) {
  const Job& j = uniform_ref(jobs, blockIdx.x);
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) j.hist[threadIdx.x + 256u * k] = 0u;
}

// k_jpeg_fdct_quant_count_multi without the count.  With the symbol walk in it, counting into LDS, the 4:4:4 form needs 168 VGPRs
// (three waves per SIMD), so the histogram is a launch of its own over the coefficients, as the bit count is.
__global__ void __launch_bounds__(128) k_jpeg_opt_fdct_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (j.rgb | j.sampled) return;   // (uniform per workgroup) k_jpeg_opt_fdct_batch_rgb's or _sampled's
  const uint32_t i = (blockIdx.x - first) * 128u + threadIdx.x;
  if (i < j.nblk) fdct_quant_count_block<kKindPlanar, false>(j, i);
}
__global__ void __launch_bounds__(128) k_jpeg_opt_fdct_batch_rgb(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (!j.rgb) return;
  const uint32_t i = (blockIdx.x - first) * 128u + threadIdx.x;
  if (i < j.nblk) fdct_quant_count_block<kKindRgb, false>(j, i);
}
__global__ void __launch_bounds__(128) k_jpeg_sampled_opt_fdct_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (kind_of(j) != kKindSampled) return;
  const uint32_t i = (blockIdx.x - first) * 128u + threadIdx.x;
  if (i < j.nblk) fdct_quant_count_block<kKindSampled, false>(j, i);
}
// The symbols walk_coefs codes, counted.  The counters of a workgroup's 128 blocks live in LDS: a flat image sends every lane to the
// same two bins (EOB, DC category 0), which the LDS adds up at its own rate, and device memory sees one atomic per bin that is not
// zero -- two per workgroup there.
struct NullSink {
  __device__ __forceinline__ void put(uint32_t, int) {}
};
__global__ void __launch_bounds__(128) k_jpeg_opt_hist_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_hist[4 * 256];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint32_t nbins = j.gray ? 512u : 1024u;
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) s_hist[b] = 0u;
  __syncthreads();
  const uint32_t i = (blockIdx.x - first) * 128u + threadIdx.x;
  if (i < j.nblk) {
    const int chroma = comp_of(j, i);
    NullSink ns;
    walk_block(j.coef + (size_t)i * 64u, pred_of(j, i), 2 * chroma, 2 * chroma + 1, ns, HistHuff{s_hist});
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) {
    const uint32_t v = s_hist[b];
    if (v != 0u) atomicAdd(&j.hist[b], v);
  }
}

// One workgroup per job, wave t builds table t (a one-plane job has two).  Then the rest of the header, in build_header's order: one
// DHT segment per table, each under its own marker, and SOS.  A header that does not fit into out_cap is not written; its length is.
__global__ void __launch_bounds__(256) k_jpeg_opt_tables_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs) {
  __shared__ TableLds s_tbl[4];
  const Job& j = uniform_ref(jobs, blockIdx.x);
  const BatchOut& o = uniform_ref(outs, blockIdx.x);
  const uint32_t t = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t ntab = j.gray ? 2u : 4u;
  const bool active = t < ntab;
  TableLds& L = s_tbl[t];
  if (build_table(j.hist + 256u * t, active, L, j.huff + 256u * t) && active) {   // the default table in its place: it codes every symbol
    const uint32_t nv = (t & 1u) ? 162u : 12u;
    if (lane < 16u) L.bits[lane + 1u] = c_std_dht[t][lane];
    for (uint32_t k = lane; k < nv; k += 64u) L.vals[k] = c_std_dht[t][16u + k];
    for (uint32_t k = lane; k < 256u; k += 64u) j.huff[256u * t + k] = c_huff[t][k];
    if (lane == 0u) L.nvals = nv;
  }
  __syncthreads();
  uint64_t at = o.header_len, total = o.header_len + (j.gray ? 10u : 14u);
  for (uint32_t k = 0; k < ntab; ++k) {
    const uint32_t seg = 21u + s_tbl[k].nvals;   // marker, length, class and index, BITS, HUFFVAL
    if (k < t) at += seg;
    total += seg;
  }
  if (threadIdx.x == 0u) *j.hdr_len = (uint32_t)total;
  if (total > o.out_cap) return;
  if (o.prefix != nullptr)
    for (uint32_t k = threadIdx.x; k < (uint32_t)o.header_len; k += 256u) o.out[k] = o.prefix[k];
  if (active) {
    const uint32_t nv = L.nvals;
    uint8_t* d = o.out + at;
    for (uint32_t k = lane; k < 21u + nv; k += 64u) {
      uint32_t v;
      if (k == 0u) v = 0xFFu;
      else if (k == 1u) v = 0xC4u;
      else if (k == 2u) v = (19u + nv) >> 8;
      else if (k == 3u) v = (19u + nv) & 0xffu;
      else if (k == 4u) v = ((t & 1u) << 4) | (t >> 1);
      else if (k < 21u) v = L.bits[k - 4u];
      else v = L.vals[k - 21u];
      d[k] = (uint8_t)v;
    }
  }
  const uint32_t nc = j.gray ? 1u : 3u, sos = 8u + 2u * nc;
  if (threadIdx.x < sos) {   // jcmarker.c emit_sos
    const uint32_t k = threadIdx.x;
    uint32_t v;
    if (k == 0u) v = 0xFFu;
    else if (k == 1u) v = 0xDAu;
    else if (k == 2u) v = 0u;
    else if (k == 3u) v = 6u + 2u * nc;
    else if (k == 4u) v = nc;
    else if (k < 5u + 2u * nc) v = ((k - 5u) & 1u) ? (k == 6u ? 0x00u : 0x11u) : (k - 5u) / 2u + 1u;
    else v = k == 6u + 2u * nc ? 63u : 0u;
    o.out[total - sos + k] = (uint8_t)v;
  }
}
// the table step on its own (uhdr_hip_jpeg_optimal_table)
__global__ void __launch_bounds__(64) k_jpeg_opt_table_one(const uint32_t* __restrict__ freq, uint8_t* __restrict__ bits, uint8_t* __restrict__ vals,
                                                          int* __restrict__ nvals) {
  __shared__ TableLds L;
  const bool overflow = build_table(freq, true, L, nullptr);
  if (threadIdx.x == 0u) *nvals = overflow ? -1 : (int)L.nvals;
  if (overflow) return;
  if (threadIdx.x < 16u) bits[threadIdx.x] = (uint8_t)L.bits[threadIdx.x + 1u];
  for (uint32_t k = threadIdx.x; k < L.nvals; k += 64u) vals[k] = L.vals[k];
}

// the job's four tables into LDS (a one-plane job: two)
__device__ __forceinline__ void load_job_huff(const Job& j) {
  uint32_t* s_huff = LdsHuff::table();
  const uint32_t n = j.gray ? 512u : 1024u;
  for (uint32_t k = threadIdx.x; k < n; k += 128u) s_huff[k] = j.huff[k];
  __syncthreads();
}
__global__ void __launch_bounds__(128) k_jpeg_opt_count_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  load_job_huff(j);
  const uint32_t wg = blockIdx.x - first, i = wg * 128u + threadIdx.x;
  uint32_t my_bits = 0;
  if (i < j.nblk) {
    const int chroma = comp_of(j, i);
    CountSink cs;
    walk_block(j.coef + (size_t)i * 64u, pred_of(j, i), 2 * chroma, 2 * chroma + 1, cs, LdsHuff());
    j.bits[i] = my_bits = cs.bits;
  }
  const uint32_t total = block_sum<128>(my_bits, s_part);
  if (threadIdx.x == 0u) j.bits_blk[wg] = total;
}
__global__ void __launch_bounds__(128) k_jpeg_opt_emit_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  load_job_huff(j);
  emit_wg<LdsHuff>(j, blockIdx.x - first);
}
// k_jpeg_stuff_copy_multi behind a header whose length only the device knows; a header that did not fit left the output untouched,
// and so does the stream
__global__ void __launch_bounds__(256) k_jpeg_opt_stuff_copy_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs,
                                                                   const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const BatchOut& o = uniform_ref(outs, k);
  const uint64_t header_len = *j.hdr_len, cap = header_len <= o.out_cap ? o.out_cap : 0u;
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_copy_wg(j, j.total_bits, o.out, cap, header_len, o.out_size, wg);
    __syncthreads();   // (s_buf and s_len are the next piece's)
  }
}

// ---- restart intervals (Job::rst_blocks != 0) ---------------------------------------------------------------------------------------
// libjpeg's restart_interval for the jobs of a round that ask for it: after every Ri MCUs but the last group the byte is filled with
// ones, RSTn follows, and the DC prediction starts again.  These jobs, with default and with optimised tables alike, run through
// launches of their own (the others keep theirs, untouched); none grows with the number of intervals:
//   k_jpeg_opt_zero_batch, k_jpeg_opt_fdct_batch[_rgb]   as they are: coefficients know no prediction
//   k_jpeg_rst_hist_batch      (optimised tables) the histogram of the symbols with the prediction cut
//   k_jpeg_rst_tables_batch    optimised tables: DHT, DRI, SOS behind the host's prefix; default tables: the Annex K codes into the job's
//                              workspace -- one chain reads its codes from LDS for both
//   k_jpeg_rst_count_batch     bits per block and per workgroup, the prediction cut
//   k_jpeg_rst_prefix_batch    every block's bits in front, modulo 2^32, as a plain sum without padding or markers
//   k_jpeg_rst_adjust_batch    an interval's unpadded length is the difference of that sum at its two ends, and its padding follows from
//                              the length modulo 8 alone since every interval starts on a byte: the last block of each interval but the
//                              final one takes padding + 16 bits onto its own count, the workgroup totals are formed again
//   k_jpeg_clear_multi, k_jpeg_rst_emit_batch
//                              with the padding and the marker part of a block's bits, offsets are the plain sum of Job::bits the other
//                              jobs use -- the segmented sum is gone; the emit records where each marker stands
//   k_jpeg_rst_stuff_count_batch, k_jpeg_rst_stuff_copy_batch
//                              0x00 behind every data 0xFF and behind no marker's
__global__ void __launch_bounds__(128) k_jpeg_rst_hist_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_hist[4 * 256];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  if (!j.optimize) return;   // (uniform per workgroup) default tables: nothing to count
  const uint32_t nbins = j.gray ? 512u : 1024u;
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) s_hist[b] = 0u;
  __syncthreads();
  const uint32_t i = (blockIdx.x - first) * 128u + threadIdx.x;
  if (i < j.nblk) {
    const int chroma = comp_of(j, i);
    NullSink ns;
    walk_block(j.coef + (size_t)i * 64u, pred_of_rst(j, i), 2 * chroma, 2 * chroma + 1, ns, HistHuff{s_hist});
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) {
    const uint32_t v = s_hist[b];
    if (v != 0u) atomicAdd(&j.hist[b], v);
  }
}
// k_jpeg_opt_tables_batch's work for a job with restart intervals: the DRI segment stands between the last DHT and SOS (jcmarker.c
// write_scan_header)
__device__ __forceinline__ void rst_tables_wg(const Job& j, const BatchOut& o) {
  __shared__ TableLds s_tbl[4];
  const uint32_t t = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t ntab = j.gray ? 2u : 4u;
  const bool active = t < ntab;
  TableLds& L = s_tbl[t];
  if (build_table(j.hist + 256u * t, active, L, j.huff + 256u * t) && active) {   // the default table in its place: it codes every symbol
    const uint32_t nv = (t & 1u) ? 162u : 12u;
    if (lane < 16u) L.bits[lane + 1u] = c_std_dht[t][lane];
    for (uint32_t k = lane; k < nv; k += 64u) L.vals[k] = c_std_dht[t][16u + k];
    for (uint32_t k = lane; k < 256u; k += 64u) j.huff[256u * t + k] = c_huff[t][k];
    if (lane == 0u) L.nvals = nv;
  }
  __syncthreads();
  uint64_t at = o.header_len, total = o.header_len + (j.gray ? 10u : 14u) + 6u;
  for (uint32_t k = 0; k < ntab; ++k) {
    const uint32_t seg = 21u + s_tbl[k].nvals;   // marker, length, class and index, BITS, HUFFVAL
    if (k < t) at += seg;
    total += seg;
  }
  if (threadIdx.x == 0u) *j.hdr_len = (uint32_t)total;
  if (total > o.out_cap) return;
  if (o.prefix != nullptr)
    for (uint32_t k = threadIdx.x; k < (uint32_t)o.header_len; k += 256u) o.out[k] = o.prefix[k];
  if (active) {
    const uint32_t nv = L.nvals;
    uint8_t* d = o.out + at;
    for (uint32_t k = lane; k < 21u + nv; k += 64u) {
      uint32_t v;
      if (k == 0u) v = 0xFFu;
      else if (k == 1u) v = 0xC4u;
      else if (k == 2u) v = (19u + nv) >> 8;
      else if (k == 3u) v = (19u + nv) & 0xffu;
      else if (k == 4u) v = ((t & 1u) << 4) | (t >> 1);
      else if (k < 21u) v = L.bits[k - 4u];
      else v = L.vals[k - 21u];
      d[k] = (uint8_t)v;
    }
  }
  const uint32_t nc = j.gray ? 1u : 3u, sos = 8u + 2u * nc;
  if (threadIdx.x < sos) {   // jcmarker.c emit_sos
    const uint32_t k = threadIdx.x;
    uint32_t v;
    if (k == 0u) v = 0xFFu;
    else if (k == 1u) v = 0xDAu;
    else if (k == 2u) v = 0u;
    else if (k == 3u) v = 6u + 2u * nc;
    else if (k == 4u) v = nc;
    else if (k < 5u + 2u * nc) v = ((k - 5u) & 1u) ? (k == 6u ? 0x00u : 0x11u) : (k - 5u) / 2u + 1u;
    else v = k == 6u + 2u * nc ? 63u : 0u;
    o.out[total - sos + k] = (uint8_t)v;
  }
  if (threadIdx.x >= 64u && threadIdx.x < 70u) {   // jcmarker.c emit_dri
    const uint32_t k = threadIdx.x - 64u, ri = j.rst_blocks / j.rst_bpm;
    const uint32_t v = k == 0u ? 0xFFu : k == 1u ? 0xDDu : k == 2u ? 0u : k == 3u ? 4u : k == 4u ? ri >> 8 : ri & 0xffu;
    o.out[total - sos - 6u + k] = (uint8_t)v;
  }
}
__global__ void __launch_bounds__(256) k_jpeg_rst_tables_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs) {
  const Job& j = uniform_ref(jobs, blockIdx.x);
  const BatchOut& o = uniform_ref(outs, blockIdx.x);
  if (j.optimize) {   // (uniform per workgroup)
    rst_tables_wg(j, o);
    return;
  }
  const uint32_t ntab = j.gray ? 2u : 4u;   // the host wrote the whole header, DRI included
  for (uint32_t t = 0; t < ntab; ++t) j.huff[256u * t + threadIdx.x] = c_huff[t][threadIdx.x];
  if (threadIdx.x == 0u) *j.hdr_len = (uint32_t)o.header_len;
}
__global__ void __launch_bounds__(128) k_jpeg_rst_count_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  load_job_huff(j);
  const uint32_t wg = blockIdx.x - first, i = wg * 128u + threadIdx.x;
  uint32_t my_bits = 0;
  if (i < j.nblk) {
    const int chroma = comp_of(j, i);
    CountSink cs;
    walk_block(j.coef + (size_t)i * 64u, pred_of_rst(j, i), 2 * chroma, 2 * chroma + 1, cs, LdsHuff());
    j.bits[i] = my_bits = cs.bits;
  }
  const uint32_t total = block_sum<128>(my_bits, s_part);
  if (threadIdx.x == 0u) j.bits_blk[wg] = total;
}
__global__ void __launch_bounds__(128) k_jpeg_rst_prefix_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint32_t wg = blockIdx.x - first, i = wg * 128u + threadIdx.x;
  uint32_t before = 0;
  for (uint32_t g = threadIdx.x; g < wg; g += 128u) before += j.bits_blk[g];
  before = block_sum<128>(before, s_part);
  const uint32_t in_front = block_exclusive_sum<128>(i < j.nblk ? j.bits[i] : 0u, s_part);
  if (i < j.nblk) j.rst_pfx[i] = before + in_front;
}
__global__ void __launch_bounds__(128) k_jpeg_rst_adjust_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint32_t wg = blockIdx.x - first, i = wg * 128u + threadIdx.x;
  uint32_t my_bits = 0;
  if (i < j.nblk) {
    my_bits = j.bits[i];
    if (i != j.nblk - 1u && (i + 1u) % j.rst_blocks == 0u) {   // the last block of an interval that a marker follows
      const uint32_t len = j.rst_pfx[i] + my_bits - j.rst_pfx[i + 1u - j.rst_blocks];   // (modulo 2^32: a multiple of 8)
      my_bits += ((8u - (len & 7u)) & 7u) + 16u;
      j.bits[i] = my_bits;
    }
  }
  const uint32_t total = block_sum<128>(my_bits, s_part);
  if (threadIdx.x == 0u) j.bits_blk[wg] = total;
}
__global__ void __launch_bounds__(128) k_jpeg_rst_emit_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  load_job_huff(j);
  emit_wg<LdsHuff, true>(j, blockIdx.x - first);
}
__global__ void __launch_bounds__(256) k_jpeg_rst_stuff_count_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_count_wg<true>(j, j.total_bits, wg);
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_jpeg_rst_stuff_copy_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs,
                                                                   const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const BatchOut& o = uniform_ref(outs, k);
  const uint64_t header_len = *j.hdr_len, cap = header_len <= o.out_cap ? o.out_cap : 0u;
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_copy_wg<true>(j, j.total_bits, o.out, cap, header_len, o.out_size, wg);
    __syncthreads();   // (s_buf and s_len are the next piece's)
  }
}

// ---- progressive files (Job::progressive != 0) ---------------------------------------------------------------------------------------
// libjpeg's jpeg_simple_progression (jcphuff.c) for the jobs of a round that ask for it: SOF2 and ten scans (six for one plane) over the
// job's coefficients, each with tables of its own.  These jobs run through launches of their own, whose grids are (workgroups of 128
// positions) x (scans): blockIdx.y is the scan, and a position is a block's place in that scan's order -- MCU order, the workspace's own,
// for the DC scans; the component's block grid in raster order, MCU padding left out, for the AC scans (prog_block).
//   k_jpeg_prog_zero_batch     the job's kProgTables x 256 counters to zero
//   k_jpeg_opt_fdct_batch[...] as they are
//   k_jpeg_prog_info_batch     AC scans: per position whether it codes a symbol, whether its band ends in an end-of-band run and the
//                              correction bits it leaves to that run (refinement scans); per workgroup their sums
//   k_jpeg_prog_prefix_batch   the exclusive sums of both over the scan's positions
//   k_jpeg_prog_walk_batch     where runs are flushed.  A run lives between two positions that code a symbol; it is flushed in front
//                              of the second, at the scan's end, when it is 0x7FFF blocks long and -- refinement scans -- when more
//                              than 937 correction bits are pending.  The last rule is greedy, hence not associative: the thread of
//                              the position a run starts behind walks it, one binary search in the prefix sums per flush (a walk per
//                              run)
//   k_jpeg_prog_hist_batch     the symbols of every scan, the EOBn ones of the flushes among them, counted
//   k_jpeg_prog_tables_batch   one workgroup per job, one wave per table: jpeg_gen_optimal_table; then one wave per scan: its DHT and
//                              SOS segments into the job's workspace
//   k_jpeg_prog_count_batch    bits per position and per workgroup
//   k_jpeg_prog_layout_batch   where each scan's segments and bits start in the one packed stream, the stream's length, the markers'
//                              positions
//   k_jpeg_prog_clear_batch, k_jpeg_prog_emit_batch
//                              the words cleared and written; the first workgroup of a scan copies its segments in front
//   k_jpeg_prog_stuff_count_batch, k_jpeg_prog_stuff_copy_batch
//                              the restart jobs' stuffing: 0x00 behind every 0xFF but a marker's (Job::rst_mark holds the segments')
struct ProgScan {
  int8_t comp;   // the scan's component, -1: all of them, interleaved (the DC scans)
  int8_t ss, se, ah, al;
  int8_t tbl;    // its first table among the job's kProgTables (a DC scan of three components has two: luma, chroma); -1: none
};
__constant__ ProgScan c_prog_scans[2][kProgScans] = {
    {{-1, 0, 0, 0, 1, 0}, {0, 1, 5, 0, 2, 2}, {2, 1, 63, 0, 1, 3}, {1, 1, 63, 0, 1, 4}, {0, 6, 63, 0, 2, 5},
     {0, 1, 63, 2, 1, 6}, {-1, 0, 0, 1, 0, -1}, {2, 1, 63, 1, 0, 7}, {1, 1, 63, 1, 0, 8}, {0, 1, 63, 1, 0, 9}},
    {{-1, 0, 0, 0, 1, 0}, {0, 1, 5, 0, 2, 1}, {0, 6, 63, 0, 2, 2}, {0, 1, 63, 2, 1, 3}, {-1, 0, 0, 1, 0, -1},
     {0, 1, 63, 1, 0, 4}, {0, 0, 0, 0, 0, -1}, {0, 0, 0, 0, 0, -1}, {0, 0, 0, 0, 0, -1}, {0, 0, 0, 0, 0, -1}}};
__device__ __forceinline__ uint32_t prog_nscans(const Job& j) { return j.gray ? 6u : 10u; }
__device__ __forceinline__ uint32_t prog_ntables(const Job& j) { return j.gray ? 5u : 10u; }
__device__ __forceinline__ uint32_t prog_scan_tables(const Job& j, const ProgScan& d) { return d.tbl < 0 ? 0u : (d.ss == 0 && !j.gray) ? 2u : 1u; }
__device__ __forceinline__ uint32_t prog_positions(const Job& j, const ProgScan& d) {
  if (d.comp < 0 || j.gray) return j.nblk;
  return d.comp == 0 ? j.ybw * j.ybh : j.nblk / (j.hs * j.vs + 2u);
}
// the workspace index (MCU order) of position p of a scan
__device__ __forceinline__ uint32_t prog_block(const Job& j, const ProgScan& d, uint32_t p) {
  if (d.comp < 0 || j.gray) return p;
  const uint32_t nl = j.hs * j.vs, bpm = nl + 2u;
  if (d.comp > 0) return p * bpm + nl + (uint32_t)(d.comp - 1);
  const uint32_t br = p / j.ybw, bc = p - br * j.ybw;
  return ((br / j.vs) * j.mcus_x + bc / j.hs) * bpm + (br % j.vs) * j.hs + (bc % j.hs);
}
// the preamble of the (workgroup, scan) kernels: false where the workgroup has nothing to do
struct ProgWg {
  uint32_t s, wg, p, npos;
  ProgScan d;
};
__device__ __forceinline__ bool prog_wg(const Job& j, uint32_t first, bool ac_only, ProgWg* w) {
  w->s = blockIdx.y;
  if (w->s >= prog_nscans(j)) return false;
  w->d = c_prog_scans[j.gray ? 1 : 0][w->s];
  if (ac_only && w->d.ss == 0) return false;
  w->npos = prog_positions(j, w->d);
  w->wg = blockIdx.x - first;
  w->p = w->wg * 128u + threadIdx.x;
  return w->wg * 128u < w->npos;
}
__device__ __forceinline__ ProgMeta* prog_meta(const Job& j) { return reinterpret_cast<ProgMeta*>(j.pg_meta); }
__device__ __forceinline__ uint32_t* prog_wg_sums(const Job& j, uint32_t what, uint32_t s) { return j.pg_wg + ((size_t)what * kProgScans + s) * j.pg_nwg; }

// The sinks of a position's symbols.  sym: a Huffman symbol of the scan's table t (0; 1: the chroma DC table) with n extra bits; raw:
// n <= 63 bits as they are; corr: the `be` correction bits the positions [a, b) of a run left to it (Job::pg_left), in their order
struct ProgHistSink {
  uint32_t* hist;   // the scan's 1 or 2 x 256 counters in LDS
  __device__ __forceinline__ void sym(int t, int symbol, uint32_t, int) { atomicAdd(&hist[t * 256 + symbol], 1u); }
  __device__ __forceinline__ void raw(uint64_t, int) {}
  __device__ __forceinline__ void corr(const Job&, size_t, uint32_t, uint32_t, uint32_t) {}
};
struct ProgCountSink {
  uint32_t bits = 0;
  __device__ __forceinline__ void sym(int t, int symbol, uint32_t, int n) { bits += (LdsHuff::table()[t * 256 + symbol] >> 16) + (uint32_t)n; }
  __device__ __forceinline__ void raw(uint64_t, int n) { bits += (uint32_t)n; }
  __device__ __forceinline__ void corr(const Job&, size_t, uint32_t, uint32_t, uint32_t be) { bits += be; }
};
struct ProgEmitSink {
  EmitSink es;
  __device__ __forceinline__ void sym(int t, int symbol, uint32_t extra, int n) {   // <= 16 + 14 bits
    const uint32_t h = LdsHuff::table()[t * 256 + symbol];
    es.put(((h & 0xffffu) << n) | extra, (int)(h >> 16) + n);
  }
  __device__ __forceinline__ void raw(uint64_t v, int n) {
    if (n > 32) { es.put((uint32_t)(v >> 32), n - 32); n = 32; }
    if (n > 0) es.put((uint32_t)v & (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u), n);
  }
  // few of a run's blocks leave bits (a run of flat blocks: none), so the next one that does is searched in the prefix sums
  __device__ __forceinline__ void corr(const Job& j, size_t row, uint32_t a, uint32_t b, uint32_t be) {
    const uint32_t* __restrict__ cs = j.pg_corr + row;
    uint32_t x = a;
    while (be != 0u) {
      const uint32_t base = cs[x];
      uint32_t y = x;
      if (cs[x + 1u] == base) {
        uint32_t lo = x + 1u, hi = b - 1u;   // the first y with cs[y + 1] > base; there is one
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (cs[mid + 1u] > base) hi = mid;
          else lo = mid + 1u;
        }
        y = lo;
      }
      const uint32_t nb = cs[y + 1u] - base;
      raw(j.pg_left[row + y], (int)nb);
      be -= nb;
      x = y + 1u;
    }
  }
};

// One block of an AC scan as bit masks over its zigzag positions, the band applied (bit k: coefficient k), v = abs(coefficient) >> Al:
// nzm: v != 0; one: v == 1 -- in a refinement scan the newly non-zero coefficients; lsb: v & 1, a correction bit where v > 1; neg: the
// coefficient's sign.  The walks below visit the set bits alone -- a loop over all 63 positions, unrolled so that the coefficients'
// registers are indexed at compile time, costs over 100 VGPRs and spills scalar registers once per scan shape.
// lds (a first scan, or nullptr): the thread's row of ProgCoefLds, which takes the coefficients themselves for the walk to index
constexpr uint32_t kProgCoefRow = 33;   // dwords per thread: 64 coefficients and one of padding against bank conflicts
struct ProgMasks {
  uint64_t nzm, one, lsb, neg;
};
__device__ __forceinline__ ProgMasks prog_masks(const int16_t* __restrict__ zz, const ProgScan& d, uint32_t* lds) {
  ProgMasks r = {0, 0, 0, 0};
  const int al = d.al;
#pragma nounroll
  for (int k = 0; k < 8; ++k) {   // (rolled: unrolled, the eight loads and their 64 values are all in flight and take 100 VGPRs)
    const uint4 v = reinterpret_cast<const uint4*>(zz)[k];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t nz = 0, one = 0, lsb = 0, neg = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (lds != nullptr) lds[4 * k + m] = w[m];
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        const int q = 2 * m + hlf;
        const int t = (int)(int16_t)(hlf ? w[m] >> 16 : w[m] & 0xffffu), a = (t < 0 ? -t : t) >> al;
        nz |= (a != 0 ? 1u : 0u) << q;
        one |= (a == 1 ? 1u : 0u) << q;
        lsb |= (uint32_t)(a & 1) << q;
        neg |= (t < 0 ? 1u : 0u) << q;
      }
    }
    r.nzm |= (uint64_t)nz << (8 * k);
    r.one |= (uint64_t)one << (8 * k);
    r.lsb |= (uint64_t)lsb << (8 * k);
    r.neg |= (uint64_t)neg << (8 * k);
  }
  const uint64_t band = (~0ull >> (63 - d.se)) & (~0ull << d.ss);
  r.nzm &= band;
  r.one &= band;
  return r;
}
// jcphuff.c encode_mcu_AC_first without its end-of-band bookkeeping: the symbols of a block that has any
template <class SINK>
__device__ __forceinline__ void prog_ac_first(const ProgMasks& b, const ProgScan& d, const uint32_t* lds, SINK& sk) {
  const int16_t* c = reinterpret_cast<const int16_t*>(lds);
  int prev = d.ss - 1;
#pragma nounroll
  for (uint64_t m = b.nzm; m != 0; m &= m - 1u) {
    const int k = __builtin_ctzll(m);
    int r = k - prev - 1;
    prev = k;
    while (r > 15) { sk.sym(0, 0xF0, 0u, 0); r -= 16; }
    const int t = c[k], a = (t < 0 ? -t : t) >> d.al;
    const int nb = nbits_of(a);
    sk.sym(0, (r << 4) + nb, (uint32_t)(t < 0 ? ~a : a) & ((1u << nb) - 1u), nb);
  }
}
// encode_mcu_AC_refine likewise: run/1 symbols with a sign bit for the newly non-zero coefficients, ZRL up to the last of them, the
// correction bits of the coefficients in between behind the next symbol.  What is left behind the last symbol is the run's (pg_left)
template <class SINK>
__device__ __forceinline__ void prog_ac_refine(const ProgMasks& b, const ProgScan& d, SINK& sk) {
  if (b.one == 0) return;
  const int eob = 63 - __builtin_clzll(b.one);
  int prev = d.ss - 1, r = 0, br = 0;
  uint64_t bb = 0;
#pragma nounroll
  for (uint64_t m = b.nzm & (~0ull >> (63 - eob)); m != 0; m &= m - 1u) {
    const int k = __builtin_ctzll(m);
    r += k - prev - 1;
    prev = k;
    while (r > 15) {
      sk.sym(0, 0xF0, 0u, 0);
      r -= 16;
      sk.raw(bb, br);
      bb = 0; br = 0;
    }
    if (!((b.one >> k) & 1u)) { bb = (bb << 1) | ((b.lsb >> k) & 1u); ++br; continue; }
    sk.sym(0, (r << 4) + 1, (uint32_t)((b.neg >> k) & 1u) ^ 1u, 1);
    sk.raw(bb, br);
    bb = 0; br = 0; r = 0;
  }
}
// a run of the positions [a, b) flushed (emit_eobrun): EOBn, the low bits of its length, its correction bits
template <class SINK>
__device__ __forceinline__ void prog_flush(const Job& j, size_t row, uint32_t a, uint32_t b, SINK& sk) {
  const uint32_t cnt = b - a;   // 1 .. 0x7FFF
  const int nb = 31 - __builtin_clz(cnt);
  sk.sym(0, nb << 4, cnt & ((1u << nb) - 1u), nb);
  const uint32_t be = j.pg_corr[row + b] - j.pg_corr[row + a];
  if (be != 0u) sk.corr(j, row, a, b, be);
}
// everything position p of scan w.s writes, in order
// s_coef: the workgroup's 128 x kProgCoefRow dwords of LDS
template <class SINK>
__device__ __forceinline__ void prog_position(const Job& j, const ProgWg& w, uint32_t* s_coef, SINK& sk) {
  const ProgScan d = w.d;
  const uint32_t p = w.p;
  if (d.ss == 0) {   // encode_mcu_DC_first / encode_mcu_DC_refine
    const int v = (int)j.coef[(size_t)p * 64u] >> d.al;
    if (d.ah != 0) { sk.raw((uint64_t)(v & 1), 1); return; }
    int t2 = v - (pred_of(j, p) >> d.al), t = t2;
    if (t < 0) { t = -t; t2--; }
    const int nb = nbits_of(t);
    sk.sym(comp_of(j, p), nb, (uint32_t)t2 & ((1u << nb) - 1u), nb);
    return;
  }
  const size_t row = (size_t)w.s * j.pg_stride;
  if (j.pg_info[row + p] & 1u) {
    const uint32_t s0 = j.pg_pend[row + p];
    if (s0 < p) prog_flush(j, row, s0, p, sk);
    uint32_t* lds = d.ah != 0 ? nullptr : s_coef + threadIdx.x * kProgCoefRow;   // (uniform per workgroup, as the scan is)
    const ProgMasks b = prog_masks(j.coef + (size_t)prog_block(j, d, p) * 64u, d, lds);
    if (d.ah != 0) prog_ac_refine(b, d, sk);
    else prog_ac_first(b, d, lds, sk);
  }
  uint32_t fs = j.pg_fstart[row + p];
  if (p == w.npos - 1u && fs == kProgNone) {   // the scan's end flushes what is pending; a run flushed behind p left nothing
    const uint32_t s0 = j.pg_pend[row + w.npos];
    if (s0 < w.npos) fs = s0;
  }
  if (fs != kProgNone) prog_flush(j, row, fs, p + 1u, sk);
}
// the tables of the workgroup's scan into LDS
__device__ __forceinline__ void prog_load_huff(const Job& j, const ProgScan& d) {
  uint32_t* s_huff = LdsHuff::table();
  const uint32_t n = 256u * prog_scan_tables(j, d);
  for (uint32_t k = threadIdx.x; k < n; k += 128u) s_huff[k] = j.huff[256u * (uint32_t)d.tbl + k];
  __syncthreads();
}

__global__ void __launch_bounds__(256) k_jpeg_prog_zero_batch(const Job* __restrict__ jobs) {
  const Job& j = uniform_ref(jobs, blockIdx.x);
  for (uint32_t k = threadIdx.x; k < (uint32_t)kProgTables * 256u; k += 256u) j.hist[k] = 0u;
}
__global__ void __launch_bounds__(128) k_jpeg_prog_info_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, true, &w)) return;   // (uniform per workgroup)
  const size_t row = (size_t)w.s * j.pg_stride;
  uint32_t nz = 0, tb = 0;
  if (w.p < w.npos) {
    // nz: the block codes a symbol; tail: its band ends in an end-of-band run -- the band's last coefficient decides: a zero (a first
    // scan), anything but a newly non-zero one (a refinement); tb, bb: the correction bits behind its last symbol, which the run takes
    const ProgMasks b = prog_masks(j.coef + (size_t)prog_block(j, w.d, w.p) * 64u, w.d, nullptr);
    const uint64_t sym = w.d.ah != 0 ? b.one : b.nzm;
    nz = sym != 0 ? 1u : 0u;
    const uint32_t tail = (uint32_t)((sym >> w.d.se) & 1u) ^ 1u;
    uint64_t bb = 0;
    if (w.d.ah != 0) {
      uint64_t m = b.nzm & ~b.one;
      if (b.one != 0) m &= ~(~0ull >> __builtin_clzll(b.one));   // (those above the last newly non-zero one)
#pragma nounroll
      for (; m != 0; m &= m - 1u) { bb = (bb << 1) | ((b.lsb >> __builtin_ctzll(m)) & 1u); ++tb; }
    }
    j.pg_info[row + w.p] = (uint16_t)(nz | (tail << 1) | (tb << 2));
    j.pg_left[row + w.p] = bb;
    j.pg_fstart[row + w.p] = kProgNone;
    j.pg_pend[row + w.p] = w.p;
    if (w.p == w.npos - 1u) j.pg_pend[row + w.npos] = w.npos;
  }
  const uint32_t nzs = block_sum<128>(nz, s_part), tbs = block_sum<128>(tb, s_part);
  if (threadIdx.x == 0u) { prog_wg_sums(j, 0, w.s)[w.wg] = nzs; prog_wg_sums(j, 1, w.s)[w.wg] = tbs; }
}
__global__ void __launch_bounds__(128) k_jpeg_prog_prefix_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, true, &w)) return;
  const size_t row = (size_t)w.s * j.pg_stride;
  uint32_t nz0 = 0, tb0 = 0;
  for (uint32_t g = threadIdx.x; g < w.wg; g += 128u) { nz0 += prog_wg_sums(j, 0, w.s)[g]; tb0 += prog_wg_sums(j, 1, w.s)[g]; }
  nz0 = block_sum<128>(nz0, s_part);
  tb0 = block_sum<128>(tb0, s_part);
  const uint32_t info = w.p < w.npos ? j.pg_info[row + w.p] : 0u;
  const uint32_t nz = info & 1u, tb = (info >> 2) & 127u;
  const uint32_t nzx = nz0 + block_exclusive_sum<128>(nz, s_part), tbx = tb0 + block_exclusive_sum<128>(tb, s_part);
  if (w.p >= w.npos) return;
  j.pg_nzc[row + w.p] = nzx;
  j.pg_corr[row + w.p] = tbx;
  if (w.p == w.npos - 1u) { j.pg_nzc[row + w.npos] = nzx + nz; j.pg_corr[row + w.npos] = tbx + tb; }
}
// One thread per position h that a run can start behind: the first position and every one that codes a symbol.  Its run ends in front
// of the next such position `lim`; most of them follow at once.
__global__ void __launch_bounds__(128) k_jpeg_prog_walk_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, true, &w)) return;
  if (w.p >= w.npos) return;
  const size_t row = (size_t)w.s * j.pg_stride;
  const uint32_t N = w.npos, h = w.p;
  const uint32_t info = j.pg_info[row + h];
  if (h != 0u && !(info & 1u)) return;
  const uint32_t* __restrict__ nzc = j.pg_nzc + row;
  const uint32_t* __restrict__ cs = j.pg_corr + row;
  uint32_t s = (info & 3u) == 1u ? h + 1u : h;   // a block that codes a symbol and ends on one starts no run itself
  uint32_t lim = h + 1u;
  if (lim < N && !(j.pg_info[row + lim] & 1u)) {   // the first position behind h that codes a symbol, N if none does
    uint32_t lo = h + 2u, hi = N;
    const uint32_t base = nzc[h + 1u];
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (nzc[mid + 1u] > base) hi = mid;
      else lo = mid + 1u;
    }
    lim = lo;
  }
  const bool refine = w.d.ah != 0;
  while (s < lim) {
    if (lim - s < 0x7FFFu && cs[lim] - cs[s] <= 937u) break;   // nothing forces a flush any more
    uint32_t e = s + 0x7FFEu;   // the run's 0x7FFF-th block
    if (refine) {               // or the first one with more than MAX_CORR_BITS - DCTSIZE2 + 1 bits pending behind it
      const uint32_t target = cs[s] + 937u;
      uint32_t lo = s, hi = lim;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cs[mid + 1u] > target) hi = mid;
        else lo = mid + 1u;
      }
      e = lo < e ? lo : e;
    }
    if (e >= lim) break;
    j.pg_fstart[row + e] = s;
    s = e + 1u;
  }
  j.pg_pend[row + lim] = s;
}
__global__ void __launch_bounds__(128) k_jpeg_prog_hist_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_hist[2 * 256];
  __shared__ uint32_t s_coef[128 * kProgCoefRow];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, false, &w)) return;
  const uint32_t nbins = 256u * prog_scan_tables(j, w.d);
  if (nbins == 0u) return;   // (a DC refinement scan has no symbols)
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) s_hist[b] = 0u;
  __syncthreads();
  if (w.p < w.npos) {
    ProgHistSink sk{s_hist};
    prog_position(j, w, s_coef, sk);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += 128u) {
    const uint32_t v = s_hist[b];
    if (v != 0u) atomicAdd(&j.hist[256u * (uint32_t)w.d.tbl + b], v);
  }
}
// One workgroup per job.  Wave t builds table t; a table libjpeg would refuse has no default to stand in -- Annex K's AC table knows no
// EOBn symbol --, so the file is refused (ProgMeta::clen_overflow).  Then wave t writes the DHT and SOS segments of scan t
// (jcmarker.c write_scan_header) into ProgMeta::hdr, and says where their markers stand.
__global__ void __launch_bounds__(64 * kProgTables) k_jpeg_prog_tables_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs) {
  __shared__ TableLds s_tbl[kProgTables];
  const Job& j = uniform_ref(jobs, blockIdx.x);
  const BatchOut& o = uniform_ref(outs, blockIdx.x);
  ProgMeta* m = prog_meta(j);
  const uint32_t t = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const bool active = t < prog_ntables(j);
  if (threadIdx.x == 0u) m->clen_overflow = 0u;
  const bool overflow = build_table(j.hist + 256u * t, active, s_tbl[t], j.huff + 256u * t);   // (its barriers order the two stores)
  if (overflow && active && lane == 0u) m->clen_overflow = 1u;
  if (threadIdx.x == 0u) *j.hdr_len = (uint32_t)o.header_len;
  if (o.prefix != nullptr && o.header_len <= o.out_cap)
    for (uint32_t q = threadIdx.x; q < (uint32_t)o.header_len; q += 64u * kProgTables) o.out[q] = o.prefix[q];
  if (t >= prog_nscans(j)) return;
  const ProgScan d = c_prog_scans[j.gray ? 1 : 0][t];
  uint8_t* hd = m->hdr[t];
  uint32_t at = 0, nm = 0;
  const uint32_t ntab = prog_scan_tables(j, d);
  for (uint32_t q = 0; q < ntab; ++q) {
    const TableLds& L = s_tbl[(uint32_t)d.tbl + q];
    const uint32_t nv = L.nvals;
    const uint32_t id = d.ss == 0 ? q : (0x10u | (d.comp == 0 ? 0u : 1u));
    for (uint32_t b = lane; b < 21u + nv; b += 64u) {
      uint32_t v;
      if (b == 0u) v = 0xFFu;
      else if (b == 1u) v = 0xC4u;
      else if (b == 2u) v = (19u + nv) >> 8;
      else if (b == 3u) v = (19u + nv) & 0xffu;
      else if (b == 4u) v = id;
      else if (b < 21u) v = L.bits[b - 4u];
      else v = L.vals[b - 21u];
      hd[at + b] = (uint8_t)v;
    }
    if (lane == 0u) m->mark_rel[t][nm] = at;
    ++nm;
    at += 21u + nv;
  }
  const uint32_t ns = d.comp < 0 ? (j.gray ? 1u : 3u) : 1u, sos = 8u + 2u * ns;
  if (lane < sos) {   // jcmarker.c emit_sos: no table selector where the scan uses none
    uint32_t v;
    if (lane == 0u) v = 0xFFu;
    else if (lane == 1u) v = 0xDAu;
    else if (lane == 2u) v = 0u;
    else if (lane == 3u) v = 6u + 2u * ns;
    else if (lane == 4u) v = ns;
    else if (lane < 5u + 2u * ns) {
      const uint32_t c = d.comp < 0 ? (lane - 5u) / 2u : (uint32_t)d.comp, tb = c == 0u ? 0u : 1u;
      v = ((lane - 5u) & 1u) ? ((d.ss == 0 && d.ah == 0 ? tb << 4 : 0u) | (d.se != 0 ? tb : 0u)) : c + 1u;
    } else {
      const uint32_t q = lane - (5u + 2u * ns);
      v = q == 0u ? (uint32_t)d.ss : q == 1u ? (uint32_t)d.se : ((uint32_t)d.ah << 4) | (uint32_t)d.al;
    }
    hd[at + lane] = (uint8_t)v;
  }
  if (lane == 0u) { m->mark_rel[t][nm] = at; m->nmark[t] = nm + 1u; m->hdr_bytes[t] = at + sos; }
}
__global__ void __launch_bounds__(128) k_jpeg_prog_count_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint32_t s_part[2];
  __shared__ uint32_t s_coef[128 * kProgCoefRow];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, false, &w)) return;
  if (prog_meta(j)->clen_overflow) return;
  prog_load_huff(j, w.d);
  uint32_t my_bits = 0;
  if (w.p < w.npos) {
    ProgCountSink sk;
    prog_position(j, w, s_coef, sk);
    j.pg_bits[(size_t)w.s * j.pg_stride + w.p] = my_bits = sk.bits;
  }
  const uint32_t total = block_sum<128>(my_bits, s_part);
  if (threadIdx.x == 0u) prog_wg_sums(j, 2, w.s)[w.wg] = total;
}
// One workgroup per job: the scans' lengths, then where everything stands in the packed stream -- scan after scan its segments, its
// bits, the padding to a byte
__global__ void __launch_bounds__(256) k_jpeg_prog_layout_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs) {
  __shared__ uint64_t s_part[4];
  __shared__ uint64_t s_tot[kProgScans];
  const Job& j = uniform_ref(jobs, blockIdx.x);
  const BatchOut& o = uniform_ref(outs, blockIdx.x);
  ProgMeta* m = prog_meta(j);
  const uint32_t nsc = prog_nscans(j);
  if (m->clen_overflow) {   // (uniform) no stream: the stuffing launches find nothing to do
    if (threadIdx.x == 0u) { *j.total_bits = 0u; *o.out_size = kProgClenOverflow; }
    return;
  }
  for (uint32_t s = 0; s < nsc; ++s) {
    const uint32_t nw = (prog_positions(j, c_prog_scans[j.gray ? 1 : 0][s]) + 127u) / 128u;
    uint64_t v = 0;
    for (uint32_t g = threadIdx.x; g < nw; g += 256u) v += prog_wg_sums(j, 2, s)[g];
    v = block_sum<256>(v, s_part);
    if (threadIdx.x == 0u) s_tot[s] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  uint64_t at = 0;
  uint32_t nm = 0;
  for (uint32_t s = 0; s < nsc; ++s) {
    m->seg_start[s] = at;
    for (uint32_t q = 0; q < m->nmark[s]; ++q) j.rst_mark[nm++] = (uint32_t)(at >> 3) + m->mark_rel[s][q];
    m->data_start[s] = at + 8u * (uint64_t)m->hdr_bytes[s];
    at = (m->data_start[s] + s_tot[s] + 7u) & ~7ull;
  }
  m->seg_start[nsc] = at;
  *j.total_bits = at;
}
// the bit range of workgroup w.wg of scan w.s: its positions' bits, the scan's segments in front of the first workgroup's, the scan's
// padding behind the last one's -- over a job's workgroups and scans exactly the stream
__device__ __forceinline__ void prog_wg_range(const Job& j, const ProgWg& w, uint64_t* s_part, uint64_t* lo, uint64_t* hi) {
  const ProgMeta* m = prog_meta(j);
  const uint32_t* bits_wg = prog_wg_sums(j, 2, w.s);
  uint64_t before = 0;
  for (uint32_t g = threadIdx.x; g < w.wg; g += 128u) before += bits_wg[g];
  before = block_sum<128>(before, s_part);
  *lo = m->data_start[w.s] + before;
  *hi = *lo + bits_wg[w.wg];
}
__global__ void __launch_bounds__(128) k_jpeg_prog_clear_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint64_t s_part[2];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, false, &w)) return;
  const ProgMeta* m = prog_meta(j);
  if (m->clen_overflow) return;
  uint64_t lo, hi;
  prog_wg_range(j, w, s_part, &lo, &hi);
  if (w.wg == 0u) lo = m->seg_start[w.s];
  if (w.wg == (w.npos + 127u) / 128u - 1u) hi = m->seg_start[w.s + 1u];
  const uint64_t w1 = (hi + 31u) >> 5;
  for (uint64_t q = ((lo + 31u) >> 5) + threadIdx.x; q < w1; q += 128u) j.stream[q] = 0u;
}
__global__ void __launch_bounds__(128) k_jpeg_prog_emit_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  __shared__ uint64_t s_part[2];
  __shared__ uint32_t s_coef[128 * kProgCoefRow];
  uint32_t first, count;
  const uint32_t k = job_of<128>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  ProgWg w;
  if (!prog_wg(j, first, false, &w)) return;
  const ProgMeta* m = prog_meta(j);
  if (m->clen_overflow) return;
  prog_load_huff(j, w.d);
  uint64_t lo, hi;
  prog_wg_range(j, w, s_part, &lo, &hi);
  const uint64_t my_bits = w.p < w.npos ? j.pg_bits[(size_t)w.s * j.pg_stride + w.p] : 0u;
  const uint64_t off = lo + block_exclusive_sum<128>(my_bits, s_part);
  if (w.wg == 0u) {   // the scan's segments: whole bytes, OR-ed into the cleared words next to the neighbours' bits
    const uint64_t b0 = m->seg_start[w.s] >> 3;
    for (uint32_t q = threadIdx.x; q < m->hdr_bytes[w.s]; q += 128u) {
      const uint64_t b = b0 + q;
      atomicOr(&j.stream[b >> 2], (uint32_t)m->hdr[w.s][q] << (8u * (uint32_t)(b & 3u)));
    }
  }
  if (w.p >= w.npos) return;
  ProgEmitSink sk;
  sk.es.words = j.stream;
  sk.es.acc = 0;
  sk.es.nacc = (int)(off & 31u);
  sk.es.wi = (uint32_t)(off >> 5);
  sk.es.first = true;
  prog_position(j, w, s_coef, sk);
  if (w.p == w.npos - 1u) {   // jcphuff.c finish_pass_phuff: flush_bits
    const int pad = (int)((8u - (uint32_t)((off + my_bits) & 7u)) & 7u);
    if (pad) sk.es.put((1u << pad) - 1u, pad);
  }
  sk.es.finish();
}
__global__ void __launch_bounds__(256) k_jpeg_prog_stuff_count_batch(const Job* __restrict__ jobs, const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_count_wg<true>(j, j.total_bits, wg);
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_jpeg_prog_stuff_copy_batch(const Job* __restrict__ jobs, const BatchOut* __restrict__ outs,
                                                                    const uint32_t* __restrict__ start, uint32_t n) {
  uint32_t first, count;
  const uint32_t k = job_of<256>(start, n, &first, &count);
  const Job& j = uniform_ref(jobs, k);
  const BatchOut& o = uniform_ref(outs, k);
  const uint64_t header_len = *j.hdr_len, cap = header_len <= o.out_cap ? o.out_cap : 0u;
  const uint64_t nbytes = (*j.total_bits + 7u) >> 3;
  for (uint32_t wg = blockIdx.x - first; (uint64_t)wg * 256u * kChunk < nbytes; wg += count) {
    stuff_copy_wg<true>(j, j.total_bits, o.out, cap, header_len, o.out_size, wg);
    __syncthreads();   // (s_buf and s_len are the next piece's)
  }
}

hipError_t optimal_table_async(const uint32_t* freq, uint8_t* bits, uint8_t* vals, int* nvals, hipStream_t s) {
  hipLaunchKernelGGL(k_jpeg_opt_table_one, dim3(1), dim3(64), 0, s, freq, bits, vals, nvals);
  return hipGetLastError();
}

// ---- host side -----------------------------------------------------------------------------------------------------
uint32_t restart_mcus(uint32_t restart_interval, uint32_t restart_in_rows, uint32_t mcus_per_row) {
  if (restart_in_rows == 0) return restart_interval;
  const uint64_t v = (uint64_t)restart_in_rows * mcus_per_row;   // jcmaster.c prepare_for_pass
  return (uint32_t)(v < 65535u ? v : 65535u);
}

size_t workspace_bytes(uint32_t nblk, Layout* l, uint32_t intervals, bool progressive) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  size_t o = 0;
  l->coef = o; o += up((size_t)nblk * 128);
  l->bits = o; o += up((size_t)(nblk + 1) * 4);
  l->bits_blk = o; o += up((size_t)(nblk / 128u + 2) * 4);
  // worst case per block: 20 bits of DC + 63 x 26 bits of AC = 1658 bits
  // an interval's padding and marker: up to 7 + 16 bits, of which its blocks' slack of 6 bits each need not hold any
  l->stream_bytes = up((size_t)nblk * 208 + 64 + (size_t)intervals * 3);
  // all scans of a progressive file: over its life a coefficient costs at most 26 bits where it is first coded and a correction bit in
  // each of up to two refinements (one that a refinement codes: 17 and a bit), a block at most three ZRLs of 16 bits and one EOBn of
  // 30 per AC scan -- four for luma -- and 28 bits of DC: 63 x 28 + 4 x 78 + 28 = 2104 bits, 263 bytes; the area takes 496 a block,
  // and the scans' segments and padding behind that
  if (progressive) l->stream_bytes = up((size_t)nblk * 496 + (size_t)kProgScans * (kProgHdrMax + 8) + 64);
  l->stream = o; o += l->stream_bytes;
  l->max_chunks = (uint32_t)(l->stream_bytes / kChunk);
  l->ff_count = o; o += up((size_t)l->max_chunks * 4);
  l->ff_blk = o; o += up((size_t)(l->max_chunks / 256u + 2) * 4);
  l->totals = o; o += 256;   // [0] total bits (uint64), [1] output size (uint64), [2] header length (uint32; optimised tables)
  l->hist = o; o += 4 * 256 * 4;
  l->huff = o; o += 4 * 256 * 4;
  l->rst_pfx = l->rst_mark = o;
  if (intervals != 0) {   // (a job without intervals keeps its layout)
    l->rst_pfx = o; o += up((size_t)nblk * 4);
    l->rst_mark = o; o += up((size_t)intervals * 4);
  }
  l->pg_info = l->pg_left = l->pg_corr = l->pg_nzc = l->pg_fstart = l->pg_pend = l->pg_bits = l->pg_wg = l->pg_meta = o;
  if (progressive) {   // (every other job keeps its layout)
    const size_t rows = (size_t)kProgScans * ((size_t)nblk + 1), nwg = (size_t)(nblk + 127u) / 128u;
    l->hist = o; o += up((size_t)kProgTables * 256 * 4);
    l->huff = o; o += up((size_t)kProgTables * 256 * 4);
    l->rst_mark = o; o += up((size_t)kProgScans * 3 * 4);
    l->pg_left = o; o += up(rows * 8);
    l->pg_corr = o; o += up(rows * 4);
    l->pg_nzc = o; o += up(rows * 4);
    l->pg_fstart = o; o += up(rows * 4);
    l->pg_pend = o; o += up(rows * 4);
    l->pg_bits = o; o += up(rows * 4);
    l->pg_info = o; o += up(rows * 2);
    l->pg_wg = o; o += up(3 * (size_t)kProgScans * nwg * 4);
    l->pg_meta = o; o += up(sizeof(ProgMeta));
  }
  l->scan_tmp_bytes = 0;
  l->scan_tmp = o;
  return o;
}

hipError_t encode_async(Job j, const Layout& l, uint8_t* ws, uint8_t* out, uint64_t out_cap, uint64_t header_len, hipStream_t s) {
  j.coef = reinterpret_cast<int16_t*>(ws + l.coef);
  j.bits = reinterpret_cast<uint32_t*>(ws + l.bits);
  j.bits_blk = reinterpret_cast<uint32_t*>(ws + l.bits_blk);
  j.stream = reinterpret_cast<uint32_t*>(ws + l.stream);
  j.ff_count = reinterpret_cast<uint32_t*>(ws + l.ff_count);
  j.ff_blk = reinterpret_cast<uint32_t*>(ws + l.ff_blk);
  j.max_chunks = l.max_chunks;
  uint64_t* totals = reinterpret_cast<uint64_t*>(ws + l.totals);
  hipError_t e;
  if ((e = hipMemsetAsync(j.stream, 0, l.stream_bytes, s)) != hipSuccess) return e;
  const dim3 gb((j.nblk + 127u) / 128u), bb(128);
  hipLaunchKernelGGL(k_jpeg_fdct_quant_count, gb, bb, 0, s, j);
  const uint64_t* total_bits = totals;   // written by the last thread of k_jpeg_emit
  j.total_bits = totals;
  hipLaunchKernelGGL(k_jpeg_emit, gb, bb, 0, s, j);
  const dim3 gc((j.max_chunks + 255u) / 256u), bc(256);
  hipLaunchKernelGGL(k_jpeg_stuff_count, gc, bc, 0, s, j, total_bits);
  hipLaunchKernelGGL(k_jpeg_stuff_copy, gc, bc, 0, s, j, total_bits, out, out_cap, header_len, totals + 1);
  return hipGetLastError();
}

namespace {
size_t up256(size_t v) { return (v + 255) / 256 * 256; }
}  // namespace

size_t batch_desc_bytes(int n) {
  return up256((size_t)n * sizeof(Job)) + up256((size_t)n * sizeof(BatchOut)) + 8 * up256(((size_t)n + 1) * 4);
}

hipError_t encode_batch_async(int n, const Job* jobs_in, const Layout* l, uint8_t* const* ws, const BatchOut* outs, uint8_t* host_desc,
                              uint8_t* dev_desc, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kMaxBatchJobs) return hipErrorInvalidValue;
  Job* jobs = reinterpret_cast<Job*>(host_desc);
  BatchOut* o = reinterpret_cast<BatchOut*>(host_desc + up256((size_t)n * sizeof(Job)));
  uint32_t* blk_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(o) + up256((size_t)n * sizeof(BatchOut)));
  uint32_t* stuff_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(blk_start) + up256(((size_t)n + 1) * 4));
  // The jobs with optimised tables stand behind the default ones in the descriptors, with grids of their own (opt_*_start count
  // from their first): the default jobs' launches see neither them nor a flag
  uint32_t* opt_blk_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(stuff_start) + up256(((size_t)n + 1) * 4));
  uint32_t* opt_stuff_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(opt_blk_start) + up256(((size_t)n + 1) * 4));
  // and behind those the jobs with restart intervals, whatever their tables, likewise
  uint32_t* rst_blk_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(opt_stuff_start) + up256(((size_t)n + 1) * 4));
  uint32_t* rst_stuff_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(rst_blk_start) + up256(((size_t)n + 1) * 4));
  // and last the progressive jobs
  uint32_t* prog_blk_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(rst_stuff_start) + up256(((size_t)n + 1) * 4));
  uint32_t* prog_stuff_start = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(prog_blk_start) + up256(((size_t)n + 1) * 4));
  blk_start[0] = stuff_start[0] = opt_blk_start[0] = opt_stuff_start[0] = rst_blk_start[0] = rst_stuff_start[0] = 0;
  prog_blk_start[0] = prog_stuff_start[0] = 0;
  int nd = 0, no = 0, nr = 0;
  for (int k = 0; k < n; ++k) {
    if (jobs_in[k].progressive != 0) continue;
    if (jobs_in[k].rst_blocks != 0) { ++nr; continue; }
    (jobs_in[k].optimize ? no : nd) += 1;
  }
  // which of the three FDCT kernels each group of jobs needs: [0] 4:2:0 and one plane, [1] RGBA pixels, [2] planes of another sampling
  bool any_def[3] = {false, false, false}, any_opt[3] = {false, false, false}, any_rst[3] = {false, false, false};
  bool any_rst_opt = false, any_prog[3] = {false, false, false}, any_prog_colour = false;
  for (int k = 0, at_d = 0, at_o = nd, at_r = nd + no, at_p = nd + no + nr; k < n; ++k) {
    const bool prog = jobs_in[k].progressive != 0, rst = !prog && jobs_in[k].rst_blocks != 0, opt = !prog && !rst && jobs_in[k].optimize != 0;
    const int kind = jobs_in[k].rgb ? 1 : jobs_in[k].sampled ? 2 : 0;   // (kind_of)
    (prog ? any_prog : rst ? any_rst : opt ? any_opt : any_def)[kind] = true;
    if (rst) any_rst_opt = any_rst_opt || jobs_in[k].optimize != 0;
    if (prog) any_prog_colour = any_prog_colour || !jobs_in[k].gray;
    const int at = prog ? at_p++ : rst ? at_r++ : opt ? at_o++ : at_d++;
    Job& j = jobs[at];
    j = jobs_in[k];
    uint8_t* w = ws[k];
    j.coef = reinterpret_cast<int16_t*>(w + l[k].coef);
    j.bits = reinterpret_cast<uint32_t*>(w + l[k].bits);
    j.bits_blk = reinterpret_cast<uint32_t*>(w + l[k].bits_blk);
    j.stream = reinterpret_cast<uint32_t*>(w + l[k].stream);
    j.ff_count = reinterpret_cast<uint32_t*>(w + l[k].ff_count);
    j.ff_blk = reinterpret_cast<uint32_t*>(w + l[k].ff_blk);
    j.max_chunks = l[k].max_chunks;
    j.total_bits = reinterpret_cast<uint64_t*>(w + l[k].totals);
    j.hist = reinterpret_cast<uint32_t*>(w + l[k].hist);
    j.huff = reinterpret_cast<uint32_t*>(w + l[k].huff);
    j.hdr_len = reinterpret_cast<uint32_t*>(w + l[k].totals + 16);
    j.rst_pfx = reinterpret_cast<uint32_t*>(w + l[k].rst_pfx);
    j.rst_mark = reinterpret_cast<uint32_t*>(w + l[k].rst_mark);
    if (prog) {
      j.pg_stride = j.nblk + 1u;
      j.pg_nwg = (j.nblk + 127u) / 128u;
      j.rst_marks = j.gray ? 11u : 20u;   // the markers of the scans' DHT and SOS segments (k_jpeg_prog_tables_batch)
      j.pg_info = reinterpret_cast<uint16_t*>(w + l[k].pg_info);
      j.pg_left = reinterpret_cast<uint64_t*>(w + l[k].pg_left);
      j.pg_corr = reinterpret_cast<uint32_t*>(w + l[k].pg_corr);
      j.pg_nzc = reinterpret_cast<uint32_t*>(w + l[k].pg_nzc);
      j.pg_fstart = reinterpret_cast<uint32_t*>(w + l[k].pg_fstart);
      j.pg_pend = reinterpret_cast<uint32_t*>(w + l[k].pg_pend);
      j.pg_bits = reinterpret_cast<uint32_t*>(w + l[k].pg_bits);
      j.pg_wg = reinterpret_cast<uint32_t*>(w + l[k].pg_wg);
      j.pg_meta = w + l[k].pg_meta;
    }
    o[at] = outs[k];
    const uint32_t stuff_wgs = (j.max_chunks + 255u) / 256u;
    uint32_t* bs = prog ? prog_blk_start + (at - nd - no - nr) : rst ? rst_blk_start + (at - nd - no) : opt ? opt_blk_start + (at - nd) : blk_start + at;
    uint32_t* ss = prog ? prog_stuff_start + (at - nd - no - nr) : rst ? rst_stuff_start + (at - nd - no) : opt ? opt_stuff_start + (at - nd) : stuff_start + at;
    bs[1] = bs[0] + (j.nblk + 127u) / 128u;
    ss[1] = ss[0] + (stuff_wgs < kStuffWgPerJob ? stuff_wgs : kStuffWgPerJob);
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(dev_desc, host_desc, batch_desc_bytes(n), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  const Job* dj = reinterpret_cast<const Job*>(dev_desc);
  const BatchOut* dout = reinterpret_cast<const BatchOut*>(dev_desc + (reinterpret_cast<uint8_t*>(o) - host_desc));
  const uint32_t* dblk = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(blk_start) - host_desc));
  const uint32_t* dstuff = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(stuff_start) - host_desc));
  const dim3 bb(128), bc(256);
  if (nd > 0) {
    const uint32_t nj = (uint32_t)nd;
    const dim3 gb(blk_start[nd]), gc(stuff_start[nd]);
    if (any_def[0]) hipLaunchKernelGGL(k_jpeg_fdct_quant_count_multi, gb, bb, 0, s, dj, dblk, nj);
    if (any_def[1]) hipLaunchKernelGGL(k_jpeg_fdct_quant_count_multi_rgb, gb, bb, 0, s, dj, dblk, nj);
    if (any_def[2]) hipLaunchKernelGGL(k_jpeg_fdct_quant_count_multi_sampled, gb, bb, 0, s, dj, dblk, nj);
    hipLaunchKernelGGL(k_jpeg_clear_multi, gb, bb, 0, s, dj, dblk, nj);
    hipLaunchKernelGGL(k_jpeg_emit_multi, gb, bb, 0, s, dj, dblk, nj);
    hipLaunchKernelGGL(k_jpeg_stuff_count_multi, gc, bc, 0, s, dj, dstuff, nj);
    hipLaunchKernelGGL(k_jpeg_stuff_copy_multi, gc, bc, 0, s, dj, dout, dstuff, nj);
  }
  if (no > 0) {
    const uint32_t nj = (uint32_t)no;
    const Job* oj = dj + nd;
    const BatchOut* oout = dout + nd;
    const uint32_t* oblk = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(opt_blk_start) - host_desc));
    const uint32_t* ostuff = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(opt_stuff_start) - host_desc));
    const dim3 gb(opt_blk_start[nj]), gc(opt_stuff_start[nj]);
    hipLaunchKernelGGL(k_jpeg_opt_zero_batch, dim3(nj), bc, 0, s, oj);
    if (any_opt[0]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch, gb, bb, 0, s, oj, oblk, nj);
    if (any_opt[1]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch_rgb, gb, bb, 0, s, oj, oblk, nj);
    if (any_opt[2]) hipLaunchKernelGGL(k_jpeg_sampled_opt_fdct_batch, gb, bb, 0, s, oj, oblk, nj);
    hipLaunchKernelGGL(k_jpeg_opt_hist_batch, gb, bb, 0, s, oj, oblk, nj);
    hipLaunchKernelGGL(k_jpeg_opt_tables_batch, dim3(nj), bc, 0, s, oj, oout);
    hipLaunchKernelGGL(k_jpeg_opt_count_batch, gb, bb, 0, s, oj, oblk, nj);
    hipLaunchKernelGGL(k_jpeg_clear_multi, gb, bb, 0, s, oj, oblk, nj);
    hipLaunchKernelGGL(k_jpeg_opt_emit_batch, gb, bb, 0, s, oj, oblk, nj);
    hipLaunchKernelGGL(k_jpeg_stuff_count_multi, gc, bc, 0, s, oj, ostuff, nj);
    hipLaunchKernelGGL(k_jpeg_opt_stuff_copy_batch, gc, bc, 0, s, oj, oout, ostuff, nj);
  }
  if (nr > 0) {
    const uint32_t nj = (uint32_t)nr;
    const Job* rj = dj + nd + no;
    const BatchOut* rout = dout + nd + no;
    const uint32_t* rblk = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(rst_blk_start) - host_desc));
    const uint32_t* rstuff = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(rst_stuff_start) - host_desc));
    const dim3 gb(rst_blk_start[nj]), gc(rst_stuff_start[nj]);
    if (any_rst_opt) hipLaunchKernelGGL(k_jpeg_opt_zero_batch, dim3(nj), bc, 0, s, rj);
    if (any_rst[0]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch, gb, bb, 0, s, rj, rblk, nj);
    if (any_rst[1]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch_rgb, gb, bb, 0, s, rj, rblk, nj);
    if (any_rst[2]) hipLaunchKernelGGL(k_jpeg_sampled_opt_fdct_batch, gb, bb, 0, s, rj, rblk, nj);
    if (any_rst_opt) hipLaunchKernelGGL(k_jpeg_rst_hist_batch, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_rst_tables_batch, dim3(nj), bc, 0, s, rj, rout);
    hipLaunchKernelGGL(k_jpeg_rst_count_batch, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_rst_prefix_batch, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_rst_adjust_batch, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_clear_multi, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_rst_emit_batch, gb, bb, 0, s, rj, rblk, nj);
    hipLaunchKernelGGL(k_jpeg_rst_stuff_count_batch, gc, bc, 0, s, rj, rstuff, nj);
    hipLaunchKernelGGL(k_jpeg_rst_stuff_copy_batch, gc, bc, 0, s, rj, rout, rstuff, nj);
  }
  if (n > nd + no + nr) {
    const uint32_t nj = (uint32_t)(n - nd - no - nr);
    const Job* pj = dj + nd + no + nr;
    const BatchOut* pout = dout + nd + no + nr;
    const uint32_t* pblk = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(prog_blk_start) - host_desc));
    const uint32_t* pstuff = reinterpret_cast<const uint32_t*>(dev_desc + (reinterpret_cast<uint8_t*>(prog_stuff_start) - host_desc));
    const dim3 gb(prog_blk_start[nj]), gc(prog_stuff_start[nj]);
    const dim3 gs(prog_blk_start[nj], any_prog_colour ? 10u : 6u);   // (workgroups of positions) x (scans)
    hipLaunchKernelGGL(k_jpeg_prog_zero_batch, dim3(nj), bc, 0, s, pj);
    if (any_prog[0]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch, gb, bb, 0, s, pj, pblk, nj);
    if (any_prog[1]) hipLaunchKernelGGL(k_jpeg_opt_fdct_batch_rgb, gb, bb, 0, s, pj, pblk, nj);
    if (any_prog[2]) hipLaunchKernelGGL(k_jpeg_sampled_opt_fdct_batch, gb, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_info_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_prefix_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_walk_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_hist_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_tables_batch, dim3(nj), dim3(64 * kProgTables), 0, s, pj, pout);
    hipLaunchKernelGGL(k_jpeg_prog_count_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_layout_batch, dim3(nj), bc, 0, s, pj, pout);
    hipLaunchKernelGGL(k_jpeg_prog_clear_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_emit_batch, gs, bb, 0, s, pj, pblk, nj);
    hipLaunchKernelGGL(k_jpeg_prog_stuff_count_batch, gc, bc, 0, s, pj, pstuff, nj);
    hipLaunchKernelGGL(k_jpeg_prog_stuff_copy_batch, gc, bc, 0, s, pj, pout, pstuff, nj);
  }
  return hipGetLastError();
}

// ---- RGBA8888 -> 4:2:0 planes (uhdr_jpeg.h) --------------------------------------------------------------------------------------
// A thread owns an 8 x 2 pixel piece of the padded image (blockIdx.y = image): two rows of 32 bytes in, two rows of 8 luma bytes
// and four bytes each of Cb and Cr out.  Padding is a clamp of the source coordinates: columns to w - 1 (expand_right_edge works
// on the full-resolution rows, chroma included); rows to h - 1 for luma, while a chroma row below the image repeats the last
// DOWNSAMPLED row, i.e. takes the rows of chroma row ceil(h / 2) - 1.  The second of those is always row h - 1: what luma needs there.
__global__ void __launch_bounds__(256) k_rgba_to_ycc420(const Rgba420Batch b) {
  const Rgba420Image& im = b.img[blockIdx.y];
  const uint32_t ucols = 2u * im.mcw, units = ucols * 8u * im.mch;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= units) return;
  const uint32_t uy = idx / ucols, ux = idx - uy * ucols;
  const uint32_t x0 = ux * 8u, last_c = (im.h + 1u) / 2u - 1u;
  const bool below = uy > last_c;
  const uint32_t cy = below ? last_c : uy;
  uint32_t px[2][8];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint32_t rr = min(2u * cy + (uint32_t)r, im.h - 1u);
    const uint32_t* row = im.src + (size_t)rr * im.stride;
    if (x0 + 8u <= im.w && (reinterpret_cast<uintptr_t>(row + x0) & 15u) == 0u) {
      const uint4 a = reinterpret_cast<const uint4*>(row + x0)[0], c = reinterpret_cast<const uint4*>(row + x0)[1];
      px[r][0] = a.x; px[r][1] = a.y; px[r][2] = a.z; px[r][3] = a.w;
      px[r][4] = c.x; px[r][5] = c.y; px[r][6] = c.z; px[r][7] = c.w;
    } else {
#pragma unroll
      for (int x = 0; x < 8; ++x) px[r][x] = row[min(x0 + (uint32_t)x, im.w - 1u)];
    }
  }
  // jccolor.c rgb_ycc_convert: 16-bit fixed point, the chroma offset with its rounding term (the constants of load_samples_rgb)
  uint32_t yv[2][2] = {{0u, 0u}, {0u, 0u}};
  int cbs[2][8], crs[2][8];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const int R = (int)(px[r][x] & 0xffu), G = (int)((px[r][x] >> 8) & 0xffu), B = (int)((px[r][x] >> 16) & 0xffu);
      const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
      cbs[r][x] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
      crs[r][x] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      yv[r][x >> 2] |= (uint32_t)Y << (8 * (x & 3));
    }
  }
  // h2v2_downsample: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along the row (this thread's first chroma column is even)
  uint32_t cbw = 0u, crw = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int bias = 1 + (q & 1);
    cbw |= (uint32_t)((cbs[0][2 * q] + cbs[0][2 * q + 1] + cbs[1][2 * q] + cbs[1][2 * q + 1] + bias) >> 2) << (8 * q);
    crw |= (uint32_t)((crs[0][2 * q] + crs[0][2 * q + 1] + crs[1][2 * q] + crs[1][2 * q + 1] + bias) >> 2) << (8 * q);
  }
  const size_t ys = 16u * (size_t)im.mcw, cs = 8u * (size_t)im.mcw;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int sr = below ? 1 : r;   // below the image both luma rows repeat row h - 1
    *reinterpret_cast<uint2*>(im.y + (2u * (size_t)uy + (size_t)r) * ys + x0) = make_uint2(yv[sr][0], yv[sr][1]);
  }
  uint8_t* cbp = im.cb + (size_t)uy * cs + 4u * ux;
  *reinterpret_cast<uint32_t*>(cbp) = cbw;
  *reinterpret_cast<uint32_t*>(cbp + 64u * (size_t)im.mcw * im.mch) = crw;
}
// ---- RGBA8888 -> 4:2:2 planes ---------------------------------------------------------------------------------------------------------
// A thread owns an 8 x 1 pixel piece of the padded image (16 mcw x 8 mch pixels; blockIdx.y = image): 32 bytes in -- neighbouring
// threads read neighbouring pieces of a row --, 8 luma bytes and four bytes each of Cb and Cr out.  Padding is a clamp of the source
// coordinates: columns to w - 1 (expand_right_edge on the full-resolution row, in front of the downsampler), rows to h - 1 (the
// chroma keeps the image's rows, so the last downsampled row is the last row's).
__global__ void __launch_bounds__(256) k_rgba_to_ycc422(const Rgba420Batch b) {
  const Rgba420Image& im = b.img[blockIdx.y];
  const uint32_t ucols = 2u * im.mcw, units = ucols * 8u * im.mch;
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= units) return;
  const uint32_t uy = idx / ucols, ux = idx - uy * ucols;
  const uint32_t x0 = ux * 8u;
  const uint32_t* row = im.src + (size_t)min(uy, im.h - 1u) * im.stride;
  uint32_t px[8];
  if (x0 + 8u <= im.w && (reinterpret_cast<uintptr_t>(row + x0) & 15u) == 0u) {
    const uint4 a = reinterpret_cast<const uint4*>(row + x0)[0], c = reinterpret_cast<const uint4*>(row + x0)[1];
    px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
    px[4] = c.x; px[5] = c.y; px[6] = c.z; px[7] = c.w;
  } else {
#pragma unroll
    for (int x = 0; x < 8; ++x) px[x] = row[min(x0 + (uint32_t)x, im.w - 1u)];
  }
  uint32_t yv[2] = {0u, 0u};
  int cbs[8], crs[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) {   // jccolor.c rgb_ycc_convert (k_rgba_to_ycc420's constants)
    const int R = (int)(px[x] & 0xffu), G = (int)((px[x] >> 8) & 0xffu), B = (int)((px[x] >> 16) & 0xffu);
    const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    cbs[x] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    crs[x] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    yv[x >> 2] |= (uint32_t)Y << (8 * (x & 3));
  }
  // h2v1_downsample: (a + b + bias) >> 1, bias 0, 1, 0, 1 ... along the row (this thread's first chroma column is even)
  uint32_t cbw = 0u, crw = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int bias = q & 1;
    cbw |= (uint32_t)((cbs[2 * q] + cbs[2 * q + 1] + bias) >> 1) << (8 * q);
    crw |= (uint32_t)((crs[2 * q] + crs[2 * q + 1] + bias) >> 1) << (8 * q);
  }
  *reinterpret_cast<uint2*>(im.y + (size_t)uy * 16u * im.mcw + x0) = make_uint2(yv[0], yv[1]);
  uint8_t* cbp = im.cb + (size_t)uy * 8u * im.mcw + 4u * ux;
  *reinterpret_cast<uint32_t*>(cbp) = cbw;
  *reinterpret_cast<uint32_t*>(cbp + 64u * (size_t)im.mcw * im.mch) = crw;
}
hipError_t launch_rgba_to_ycc422(const Rgba420Batch& b, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kRgba420Chunk) return hipErrorInvalidValue;
  uint32_t units = 0;
  for (int k = 0; k < n; ++k) units = std::max(units, 16u * b.img[k].mcw * b.img[k].mch);
  hipLaunchKernelGGL(k_rgba_to_ycc422, dim3((units + 255u) / 256u, (unsigned)n), dim3(256), 0, s, b);
  return hipGetLastError();
}
hipError_t launch_rgba_to_ycc420(const Rgba420Batch& b, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > kRgba420Chunk) return hipErrorInvalidValue;
  uint32_t units = 0;
  for (int k = 0; k < n; ++k) units = std::max(units, 16u * b.img[k].mcw * b.img[k].mch);
  hipLaunchKernelGGL(k_rgba_to_ycc420, dim3((units + 255u) / 256u, (unsigned)n), dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace jpeg
}  // namespace uhdr
