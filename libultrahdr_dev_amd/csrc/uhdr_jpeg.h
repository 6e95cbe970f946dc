// uhdr_jpeg.h -- internal interface of the GPU baseline-JPEG encoder (uhdr_jpeg.hip)
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

namespace uhdr {
namespace jpeg {

struct Plane {
  const uint8_t* p;
  int w, h, stride;
  int pad_cols;   // columns >= w read as zero (the reference copies the row into a zero-padded buffer) instead of from p;
                  // kPadReplicate: libjpeg's own edge expansion instead of either rule -- the last column repeated, then the last row
  int aligned4;   // p and stride are multiples of 4: whole-dword row loads
};
constexpr int kPadReplicate = 2;
struct Job {
  Plane plane[3];          // Y, Cb, Cr (one plane: only [0])
  uint16_t q_lum[64], q_chr[64];   // quantisation tables in zigzag order
  uint32_t m_lum[64], m_chr[64];   // floor(2^32 / (q << 3)) + 1: n / (q << 3) == mulhi(n, m) for n < 2^16 (exact: n * (q << 3) < 2^32)
  uint32_t nblk;           // blocks in entropy-coding order, dummy edge blocks included
  uint32_t ybw, ybh;       // luma size in blocks
  uint32_t mcus_x;         // MCUs per row (three planes)
  uint32_t hs, vs;         // luma sampling factors of three planes, {1,2} x {1,2}, both chroma components 1x1 (as DecInfo's): an MCU is
                           // hs * vs luma blocks, in rows of hs, followed by Cb and Cr.  2x2 = 4:2:0; one plane and rgb: 1x1
  int sampled;             // three planes whose hs x vs is not 2x2: the block geometry is locate_sampled's (0 for 4:2:0, one plane and rgb)
  int gray;
  int rgb;                 // 4:4:4 from interleaved RGBA (plane[0]: the pixels, stride in bytes); an MCU is one block each of Y, Cb, Cr
  // workspace (device)
  int16_t* coef;           // nblk x 64, zigzag order
  uint32_t* bits;          // nblk (+1 zero)
  uint32_t* bits_blk;      // per workgroup of 128 blocks: their bits
  uint64_t* total_bits;    // the stream's length in bits (written by k_jpeg_emit)
  uint32_t* stream;        // packed entropy-coded bits before byte stuffing, big-endian words
  uint32_t* ff_count;      // per 64-byte chunk of the stream
  uint32_t* ff_blk;
  uint32_t max_chunks;
  // optimised Huffman tables (optimize != 0): the job runs through the k_jpeg_opt_* launches of its round
  int optimize;
  uint32_t* hist;          // 4 x 256 symbol counts ([0] DC lum, [1] AC lum, [2] DC chroma, [3] AC chroma), zeroed on the stream
  uint32_t* huff;          // 4 x 256 codes built from them, (size << 16) | code as in c_huff
  uint32_t* hdr_len;       // the header's length, known once k_jpeg_opt_tables_batch has written the DHT and SOS segments
  // restart intervals (rst_blocks != 0): the job runs through the k_jpeg_rst_* launches of its round, with either kind of tables
  uint32_t rst_blocks;     // blocks per interval: libjpeg's restart_interval (MCUs, 1 .. 65535) x rst_bpm
  uint32_t rst_bpm;        // blocks per MCU: hs * vs + 2 (6 for 4:2:0, 4 for 4:2:2 and 4:4:0, 3 for 4:4:4) or 1
  uint32_t rst_marks;      // RSTn markers in the stream: one behind every interval but the last
  uint32_t* rst_pfx;       // nblk: the bits of the blocks in front of each, modulo 2^32, without padding and markers
  uint32_t* rst_mark;      // rst_marks: where each marker's 0xFF stands in the packed stream (bytes), ascending
  // progressive files (progressive != 0): the job runs through the k_jpeg_prog_* launches of its round.  All scans share one packed
  // stream -- each scan's DHT and SOS segments in front of its bits, every scan padded to a byte --; rst_mark / rst_marks hold the
  // positions of those segments' markers, which get no stuffed zero.  hist and huff hold kProgTables tables.  The arrays below have one
  // row of pg_stride entries per scan, indexed by a block's position in the scan's own order
  int progressive;
  uint32_t pg_stride;      // nblk + 1
  uint32_t pg_nwg;         // workgroups of 128 positions in the longest scan
  uint16_t* pg_info;       // AC scans: bit 0: the block codes a symbol; bit 1: its band ends in an end-of-band run; bits 2..8: correction
                           // bits it leaves to the run
  uint64_t* pg_left;       // those bits, first one highest
  uint32_t* pg_corr;       // correction bits left to runs by the positions in front (position N: all)
  uint32_t* pg_nzc;        // positions in front that code a symbol
  uint32_t* pg_fstart;     // a run is flushed behind this position: its first position (kProgNone: no flush)
  uint32_t* pg_pend;       // the first position of the run pending in front of this position (the position itself: none); entry N: at
                           // the scan's end
  uint32_t* pg_bits;       // bits this position writes
  uint32_t* pg_wg;         // per scan and workgroup: [0] positions that code a symbol, [1] correction bits left, [2] bits; 3 x scans x pg_nwg
  uint8_t* pg_meta;        // ProgMeta
};
constexpr int kProgScans = 10, kProgTables = 10;
constexpr uint32_t kProgNone = 0xFFFFFFFFu;
constexpr uint32_t kProgHdrMax = 576;     // a scan's DHT and SOS segments: at most two tables of 21 + 256 bytes and 14 bytes
struct ProgMeta {
  uint64_t seg_start[kProgScans + 1];     // bit offset of each scan's segments in the packed stream; [scans]: the stream's length
  uint64_t data_start[kProgScans];        // ... of its entropy-coded bits
  uint32_t hdr_bytes[kProgScans];
  uint32_t nmark[kProgScans], mark_rel[kProgScans][3];   // the markers inside a scan's segments
  uint32_t clen_overflow;                 // a table's optimal code is deeper than 32 bits: no file (libjpeg: JERR_HUFF_CLEN_OVERFLOW)
  uint8_t hdr[kProgScans][kProgHdrMax];
};
struct Layout {
  size_t coef, bits, bits_blk, stream, stream_bytes, ff_count, ff_blk, totals, scan_tmp, scan_tmp_bytes, hist, huff, rst_pfx, rst_mark;
  size_t pg_info, pg_left, pg_corr, pg_nzc, pg_fstart, pg_pend, pg_bits, pg_wg, pg_meta;   // progressive jobs only
  uint32_t max_chunks;
};

hipError_t upload_tables();
void quant_table(int quality, bool chroma, uint16_t out_natural[64]);
void zigzag_table(const uint16_t natural[64], uint16_t zz[64]);
// geom: what the frame header declares -- the 4:2:0 and single-plane files of the reference's encoder, three 1x1 components from
// RGBA pixels (kGeomRgb444) or from planes (kGeom444), or 2x1 / 1x2 luma over 1x1 chroma planes (kGeom422 / kGeom440)
enum Geometry : int { kGeom420 = 0, kGeomGray = 1, kGeomRgb444 = 2, kGeom444 = 3, kGeom422 = 4, kGeom440 = 5 };
inline int geom_hs(Geometry g) { return (g == kGeom420 || g == kGeom422) ? 2 : 1; }
inline int geom_vs(Geometry g) { return (g == kGeom420 || g == kGeom440) ? 2 : 1; }
// prefix_only: SOI ... SOF alone -- the DHT and SOS segments of a file with optimised tables are written on the device
// restart_interval != 0 (and not prefix_only): a DRI segment between the last DHT and SOS
// progressive (with prefix_only): the frame header is SOF2
void build_header(int w, int h, Geometry geom, int quality, const void* icc, size_t icc_n, std::vector<uint8_t>& out, bool prefix_only = false,
                  uint32_t restart_interval = 0, bool progressive = false);
// libjpeg's restart_in_rows over restart_interval: MCUs per interval of a scan with mcus_per_row MCUs in a row (0: none)
uint32_t restart_mcus(uint32_t restart_interval, uint32_t restart_in_rows, uint32_t mcus_per_row);
// a job with restart intervals (Job::rst_blocks) works in a stream area that also holds their padding and markers; the packed stream
// is addressed in 32 bits there, so such a job has at most kMaxRestartBlocks blocks
constexpr uint32_t kMaxRestartBlocks = 20000000u;
// intervals: ceil(MCUs / restart interval) of such a job, 0 for every other
// progressive: the workspace of a progressive job (no intervals): a stream area for all scans, kProgTables tables, the per-scan arrays
size_t workspace_bytes(uint32_t nblk, Layout* l, uint32_t intervals = 0, bool progressive = false);
// a progressive job marks its segments' markers in 32-bit stream offsets, and its stream takes up to 496 bytes per block
constexpr uint32_t kMaxProgressiveBlocks = 8000000u;
// out_size of a progressive file whose tables libjpeg would refuse (ProgMeta::clen_overflow)
constexpr uint64_t kProgClenOverflow = ~0ull;
// enqueues the whole encoder; the JPEG (without the header, which the caller places at out[0, header_len)) lands at
// out + header_len, its total size (header included) in the uint64 at ws + l.totals + 8
hipError_t encode_async(Job j, const Layout& l, uint8_t* ws, uint8_t* out, uint64_t out_cap, uint64_t header_len, hipStream_t s);

// ---- batched encoder: n JPEGs, one launch per encoder step for all of them ----------------------------------------------
constexpr int kMaxBatchJobs = 128;      // jobs per encode_batch_async (their starts are searched in LDS)
constexpr uint32_t kStuffWgPerJob = 64; // byte-stuffing workgroups per job; they stride over the stream's 16 KiB pieces
struct BatchOut {                       // where job k's JPEG goes: header at out[0, header_len) written by the caller
  uint8_t* out;                         // device-accessible (device or page-locked host memory)
  uint64_t out_cap, header_len;
  uint64_t* out_size;                   // the file's size, header included (device-accessible)
  // a job with optimised tables: header_len is the length of the prefix SOI ... SOF, the rest of the header is the device's.  Where
  // the caller cannot tell whether the header fits (a device destination), the prefix waits here (device-accessible) and the device
  // copies it with the rest; nullptr: it is at out already
  const uint8_t* prefix = nullptr;
};
// libjpeg's "no frequency" in jpeg_gen_optimal_table: a table's counts must stay below it, so a job with optimised tables has
// 63 * nblk < kHuffFreqLimit
constexpr uint32_t kHuffFreqLimit = 1000000000u;
constexpr uint32_t kMaxOptimizeBlocks = (kHuffFreqLimit - 1u) / 63u;
// jpeg_gen_optimal_table of one histogram on the device (the table step of the encoder, on its own): freq: 256 counts, each below
// kHuffFreqLimit; bits[16], vals[256], *nvals (-1: a code longer than 32 bits, which libjpeg refuses) -- all device memory
hipError_t optimal_table_async(const uint32_t* freq, uint8_t* bits, uint8_t* vals, int* nvals, hipStream_t s);
size_t batch_desc_bytes(int n);
// jobs: tables, geometry and planes as for encode_async; job k works in ws[k] (workspace_bytes(jobs[k].nblk, &l[k]) bytes).  The
// descriptors are assembled in host_desc (page-locked, batch_desc_bytes(n); not to be touched until the stream has passed this
// point) and copied to dev_desc (device, the same size).  n <= kMaxBatchJobs.
hipError_t encode_batch_async(int n, const Job* jobs, const Layout* l, uint8_t* const* ws, const BatchOut* outs, uint8_t* host_desc,
                              uint8_t* dev_desc, hipStream_t s);

// ---- RGBA8888 -> the planes of a 4:2:0 file (uhdr_hip_jpeg_encode_rgba420_batch) ----------------------------------------------
// What libjpeg hands its FDCT for in_color_space = JCS_RGB with 2x2 luma sampling: jccolor.c's RGB -> YCbCr at full resolution,
// jcsample.c's h2v2_downsample of the chroma, every plane padded to whole MCUs the way libjpeg pads (last column out to the padded
// width, last row to an even count, then the last -- downsampled -- row).  With mcw x mch MCUs: Y is 16 mcw x 16 mch at y, Cb and
// Cr are 8 mcw x 8 mch each at cb and cb + 64 mcw mch, rows packed.  The encoder reads them as they are (no padding rule applies).
constexpr int kRgba420Chunk = 64;       // images per launch (descriptors in the kernarg segment)
struct Rgba420Image {
  const uint32_t* src;     // RGBA pixels, 4-byte aligned
  uint8_t* y;              // 8-byte aligned
  uint8_t* cb;             // 4-byte aligned
  uint32_t w, h, stride;   // stride in pixels
  uint32_t mcw, mch;
};
struct Rgba420Batch {
  Rgba420Image img[kRgba420Chunk];
};
static_assert(sizeof(Rgba420Batch) <= 4096, "k_rgba_to_ycc420's kernel arguments exceed the kernarg segment");
inline size_t rgba420_plane_bytes(size_t w, size_t h) { return 384 * ((w + 15) / 16) * ((h + 15) / 16); }
hipError_t launch_rgba_to_ycc420(const Rgba420Batch& b, int n, hipStream_t s);   // one launch for n <= kRgba420Chunk images of any sizes
// The same for a 4:2:2 file (2x1 luma sampling): jcsample.c's h2v1_downsample of the chroma.  With mcw x mch MCUs (16 x 8 pixels):
// Y is 16 mcw x 8 mch at y, Cb and Cr are 8 mcw x 8 mch each at cb and cb + 64 mcw mch, rows packed.  Rgba420Image's fields, with mcw
// and mch counting these MCUs.
inline size_t rgba422_plane_bytes(size_t w, size_t h) { return 256 * ((w + 15) / 16) * ((h + 7) / 8); }
hipError_t launch_rgba_to_ycc422(const Rgba420Batch& b, int n, hipStream_t s);

// ---- decoder (uhdr_jpeg_dec.hip) -------------------------------------------------------------------------------------
struct HuffSpec {            // one DHT table in canonical form (T.81 Annex C)
  uint16_t first_code[17];   // first code of each length (index = length)
  uint16_t first_val[17];    // index into vals of that code
  uint16_t count[17];
  uint8_t vals[256];
  int present;
};
struct DecTables { HuffSpec huff[4]; };   // [0] DC luma, [1] AC luma, [2] DC chroma, [3] AC chroma
struct DecPlane {
  uint8_t* p;
  int w, h, stride;
  int aligned8;
};
struct DecInfo {
  int w = 0, h = 0, gray = 0;
  // luma sampling factors of a three-component frame (both chroma components are 1x1): 2x2 = 4:2:0, 1x1 = 4:4:4, 2x1 = 4:2:2,
  // 1x2 = 4:4:0.  An MCU is hs * vs luma blocks (rows of hs) followed by Cb and Cr; a single plane: 1x1 and one block.
  int hs = 2, vs = 2;
  uint16_t quant[3][64] = {};     // per component, zigzag order (as stored in the file)
  DecTables tables = {};
  int td[2] = {0, 0}, ta[2] = {0, 0};
  size_t scan_offset = 0, scan_bytes = 0;   // the entropy-coded segment inside the file
  // restart intervals (DRI / RSTn, T.81 B.2.4.4 + E.2.4): MCUs per interval (0 = none) and, from a host scan of the segment, where
  // each interval starts in the UNSTUFFED stream (stuffed zeros and the RSTn markers themselves removed), and that stream's length
  uint32_t restart_interval = 0;
  std::vector<uint32_t> interval_start;
  uint32_t raw_bytes = 0;
  // progressive files (SOF2): every scan is entropy-decoded on the host (uhdr_jpeg_prog.cpp); coef = nblk x 64 coefficients, zigzag
  // order, blocks in the device decoder's order, DC as the difference to the component's previous block; scan_bytes = 0 and
  // scan_offset = the position of EOI.  The device runs its DC prefix sum and the IDCT.
  bool progressive = false;
  std::vector<int16_t> coef;
  // set by the caller, not by the parsers: the image is decoded at 1 / scale of its size (1, 2, 4, 8; libjpeg's scale_denom) into
  // planes of scaled_geometry's sizes.  Everything in front of the IDCT works on the file's own w x h
  int scale = 1;
};
struct DecLayout {
  size_t src, raw, lut, adv, st_a, st_b, dirty_a, dirty_b, coef;
  size_t sub_start, sub_end, sub_key;   // restart-interval files only
  uint32_t nchunks, nsub_max, nblk, mcus_x;
  uint32_t hs, vs;           // luma blocks per MCU row / column (a single plane: 1, 1)
};
struct DecJob {
  const uint32_t* raw;       // unstuffed entropy-coded bits, big-endian words, zero padded
  const uint32_t* lut;       // 4 first-level tables of the final pass (coef_entry), see build_lut_body
  const uint32_t* adv;       // 4 first-level tables of position-only entries (one symbol | two symbols)
  uint32_t total_bits, nsub, nblk, mcus_x;
  // restart-interval files: subsequence i covers bits [sub_start[i], sub_end[i]) of restart interval sub_key[i] (it never spans
  // two intervals); restart_blocks = blocks per interval.  NULL / 0: one interval, subsequence i = bits [512 i, 512 (i + 1))
  const uint32_t* sub_start;
  const uint32_t* sub_end;
  const uint32_t* sub_key;
  uint32_t restart_blocks;
  int gray;
  uint32_t hs, vs;           // luma blocks per MCU row / column
  uint32_t bpm, chroma_at;   // blocks per MCU (hs * vs + 2; a single plane: 1) and the first chroma block in it (a single plane: 0xFF, never reached)
  uint32_t dc_tbl[2], ac_tbl[2];
  int16_t* coef;             // nblk x 64, zigzag order
  DecPlane plane[3];
  uint16_t quant[3][64];
};
// What a decode at 1 / scale gives (jdmaster.c's jpeg_calc_output_dimensions, libjpeg-turbo's rule): ceil(w / scale) x ceil(h / scale)
// luma; idct[c]: the IDCT size of component c, 8 / scale, doubled for the chroma of 4:2:0 -- which is thereby scaled up in the IDCT, so
// hs x vs, the luma sampling of the RESULT, is 1 x 1 for such a file at scale > 1 and the file's own otherwise
struct ScaledGeom { int w, h, hs, vs, idct[3]; };
void scaled_idct_sizes(int hs, int vs, bool gray, int scale, int size[3]);
inline ScaledGeom scaled_geometry(int w, int h, int hs, int vs, bool gray, int scale) {
  ScaledGeom g;
  g.w = (w + scale - 1) / scale; g.h = (h + scale - 1) / scale;
  scaled_idct_sizes(hs, vs, gray, scale, g.idct);
  const int n = 8 / scale;
  g.hs = gray ? 1 : hs * n / g.idct[1]; g.vs = gray ? 1 : vs * n / g.idct[1];
  return g;
}
// 0 ok, -1 malformed, -2 outside what this decoder (or the reference: sampling) supports.  any_sampling false: three components
// must be 4:2:0, as in the reference; true: luma 1x1, 2x1, 1x2 or 2x2 over 1x1 chroma (DecInfo::hs, vs)
int parse_header(const uint8_t* jpg, size_t n, DecInfo* info, bool any_sampling = false);
// the same for a progressive file, all scans decoded (parse_header calls it when it meets SOF2)
int decode_progressive(const uint8_t* jpg, size_t n, DecInfo* info, bool any_sampling = false);
bool sampling_accepted(int nc, const int hs[3], const int vs[3], bool any_sampling);   // what both parsers accept of a frame header
// the walk over an entropy-coded segment on its own (the container scan uses it): position of the 0xFF of the first marker at or
// behind `e` that is neither a stuffed zero, a fill byte nor an RSTn; n if there is none
size_t skip_entropy_coded(const uint8_t* p, size_t e, size_t n);
size_t dec_workspace_bytes(const DecInfo& info, DecLayout* l);
// n images on one stream with one launch per decoder step for all of them (blockIdx.y = image); batch_ws: device scratch of
// dec_batch_scratch_bytes(n, layouts)
size_t dec_batch_scratch_bytes(int n, const DecLayout l[]);
int decode_device_batch(int n, const DecInfo* const info[], const DecLayout l[], uint8_t* const ws[], DecPlane (*planes[])[3], hipStream_t s,
                        uint8_t* batch_ws, hipError_t* herr, int* image_rc);
// of this host thread's last decode_device_batch: k_jd_sync_multi<1> launches enqueued up to the look at the ring that read "no
// change", the number of looks; and the launches in front of the first look (a constant)
void last_sync_counts(uint32_t* launches, uint32_t* ring_looks, uint32_t* first_launches);

}  // namespace jpeg
}  // namespace uhdr
