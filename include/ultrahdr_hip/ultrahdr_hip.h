/*
 * ultrahdr_hip/ultrahdr_hip.h -- C++ host-side mirror of the reference's hot-path interface, implemented
 * on top of the C-ABI in include/uhdr_hip.h (MI355X kernels).
 *
 * The reference keeps the pixel path behind protected members of ultrahdr::UltraHdr
 * (lib/include/ultrahdr/ultrahdr.h:333-381) and private JpegR::convertYuv
 * (lib/include/ultrahdr/jpegr.h:329-330).  `ultrahdr::UltraHdrHip` exposes the same four operations
 * with the same names, argument meaning, ownership rules and status_t values, so that a caller written
 * like lib/src/jpegr.cpp (encodeJPEGR :200,:284,:421,:502; decodeJPEGR :801; :224,:360 for convertYuv)
 * compiles against it unchanged.  Type and enumerator names/values are the reference's.
 *
 * Ownership (same as the reference):
 *   generateGainMap  allocates dest->data with new uint8_t[]; the caller frees it with delete[]
 *                    (jpegr.cpp:207-208 wraps it in unique_ptr<uint8_t[]>);
 *   applyGainMap / toneMap / convertYuv: the caller owns every buffer.
 * All calls are synchronous on host memory (the image is staged through HBM and back).
 */
#ifndef ULTRAHDR_HIP_SHIM_H
#define ULTRAHDR_HIP_SHIM_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ultrahdr {

// Enumerator names and numeric values are the reference's (lib/include/ultrahdr/ultrahdr.h:36-120), so that
// caller code compiles unchanged; only the codes the pixel path can return are listed for status_t.
enum ultrahdr_color_gamut : int {
  ULTRAHDR_COLORGAMUT_UNSPECIFIED = -1, ULTRAHDR_COLORGAMUT_BT709 = 0, ULTRAHDR_COLORGAMUT_P3 = 1,
  ULTRAHDR_COLORGAMUT_BT2100 = 2, ULTRAHDR_COLORGAMUT_MAX = 2
};
enum ultrahdr_transfer_function : int {
  ULTRAHDR_TF_UNSPECIFIED = -1, ULTRAHDR_TF_LINEAR = 0, ULTRAHDR_TF_HLG = 1, ULTRAHDR_TF_PQ = 2, ULTRAHDR_TF_SRGB = 3,
  ULTRAHDR_TF_MAX = 3
};
enum ultrahdr_output_format : int {
  ULTRAHDR_OUTPUT_UNSPECIFIED = -1, ULTRAHDR_OUTPUT_SDR = 0, ULTRAHDR_OUTPUT_HDR_LINEAR = 1, ULTRAHDR_OUTPUT_HDR_PQ = 2,
  ULTRAHDR_OUTPUT_HDR_HLG = 3, ULTRAHDR_OUTPUT_HDR_LINEAR_RGB_10BIT = 4, ULTRAHDR_OUTPUT_MAX = 4
};
enum ultrahdr_pixel_format : int {
  ULTRAHDR_PIX_FMT_UNSPECIFIED = -1, ULTRAHDR_PIX_FMT_P010 = 0, ULTRAHDR_PIX_FMT_YUV420 = 1,
  ULTRAHDR_PIX_FMT_MONOCHROME = 2, ULTRAHDR_PIX_FMT_RGBA8888 = 3, ULTRAHDR_PIX_FMT_RGBAF16 = 4,
  ULTRAHDR_PIX_FMT_RGBA1010102 = 5
};
enum status_t : int {
  ULTRAHDR_NO_ERROR = 0, ULTRAHDR_UNKNOWN_ERROR = -1, ERROR_ULTRAHDR_BAD_PTR = -10001,
  ERROR_ULTRAHDR_INVALID_COLORGAMUT = -10003, ERROR_ULTRAHDR_INVALID_TRANS_FUNC = -10005,
  ERROR_ULTRAHDR_RESOLUTION_MISMATCH = -10006, ERROR_ULTRAHDR_BAD_METADATA = -10010,
  ERROR_ULTRAHDR_INVALID_CROPPING_PARAMETERS = -10011, ERROR_ULTRAHDR_UNSUPPORTED_FEATURE = -30000,
  ERROR_ULTRAHDR_UNSUPPORTED_MAP_SCALE_FACTOR = -20008, ERROR_ULTRAHDR_INSUFFICIENT_RESOURCE = -20009,
  // the container path (JpegRHip below)
  ERROR_ULTRAHDR_UNSUPPORTED_WIDTH_HEIGHT = -10002, ERROR_ULTRAHDR_INVALID_STRIDE = -10004,
  ERROR_ULTRAHDR_INVALID_QUALITY_FACTOR = -10007, ERROR_ULTRAHDR_INVALID_DISPLAY_BOOST = -10008,
  ERROR_ULTRAHDR_INVALID_OUTPUT_FORMAT = -10009, ERROR_ULTRAHDR_ENCODE_ERROR = -20001, ERROR_ULTRAHDR_DECODE_ERROR = -20002,
  ERROR_ULTRAHDR_GAIN_MAP_IMAGE_NOT_FOUND = -20003, ERROR_ULTRAHDR_BUFFER_TOO_SMALL = -20004,
  ERROR_ULTRAHDR_METADATA_ERROR = -20005, ERROR_ULTRAHDR_NO_IMAGES_FOUND = -20006,
  ERROR_ULTRAHDR_MULTIPLE_EXIFS_RECEIVED = -20007
};

// ultrahdr_metadata_struct / ultrahdr_uncompressed_struct: same members, order and defaults as the reference
// (ultrahdr.h:129-147,152-181): linear boosts, strides in pixels, chroma_data == nullptr meaning "right after luma"
// is resolved by the CALLER (jpegr.cpp:265-278) before these functions are entered.
struct ultrahdr_metadata_struct {
  std::string version;
  float maxContentBoost, minContentBoost, gamma, offsetSdr, offsetHdr, hdrCapacityMin, hdrCapacityMax;
};
using ultrahdr_metadata_ptr = ultrahdr_metadata_struct*;

struct ultrahdr_uncompressed_struct {
  void* data;
  size_t width, height;
  ultrahdr_color_gamut colorGamut;
  void* chroma_data = nullptr;
  size_t luma_stride = 0, chroma_stride = 0;
  ultrahdr_pixel_format pixelFormat = ULTRAHDR_PIX_FMT_UNSPECIFIED;
};
using uhdr_uncompressed_ptr = ultrahdr_uncompressed_struct*;

static const char* const kGainMapVersion = "1.0";
static const size_t kMapDimensionScaleFactor = 4;

class UltraHdrHip {
 public:
  // device: HIP device ordinal this object runs on (uhdr_hip_init is called lazily, once)
  explicit UltraHdrHip(int device = 0);

  status_t generateGainMap(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr p010_image_ptr,
                           ultrahdr_transfer_function hdr_tf, ultrahdr_metadata_ptr metadata,
                           uhdr_uncompressed_ptr dest, bool sdr_is_601 = false);

  // generateGainMap against the range the content has (include/uhdr_hip.h, "content-adaptive gain maps"): the same arguments,
  // checks and new[] contract; *metadata receives the measured range instead of the reference's constants
  status_t generateGainMapAdaptive(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr p010_image_ptr,
                                   ultrahdr_transfer_function hdr_tf, ultrahdr_metadata_ptr metadata,
                                   uhdr_uncompressed_ptr dest, bool sdr_is_601 = false);

  status_t applyGainMap(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr gainmap_image_ptr,
                        ultrahdr_metadata_ptr metadata, ultrahdr_output_format output_format,
                        float max_display_boost, uhdr_uncompressed_ptr dest);

  status_t toneMap(uhdr_uncompressed_ptr src, uhdr_uncompressed_ptr dest);

  status_t convertYuv(uhdr_uncompressed_ptr image, ultrahdr_color_gamut src_encoding,
                      ultrahdr_color_gamut dest_encoding);

  // UHDR_HIP_APPLY_FAST (default), UHDR_HIP_APPLY_EXACT or UHDR_HIP_APPLY_LUT, see include/uhdr_hip.h
  void setApplyMode(int mode) { mApplyMode = mode; }
  // UHDR_HIP_GENERATE_EXACT (default), UHDR_HIP_GENERATE_LUT or UHDR_HIP_GENERATE_UNFILTERED
  void setGenerateMode(int mode) { mGenerateMode = mode; }

 private:
  status_t ensureInit();
  status_t generateImpl(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr p010_image_ptr, ultrahdr_transfer_function hdr_tf,
                        ultrahdr_metadata_ptr metadata, uhdr_uncompressed_ptr dest, bool sdr_is_601, bool adaptive);
  int mDevice;
  bool mReady = false;
  int mApplyMode = 0;
  int mGenerateMode = 0;
};

// The SDR base image of a P010 image tone-mapped from linear light (include/uhdr_hip.h, "tone-mapped SDR base image"; no reference
// counterpart): host images in and out like toneMap's, executed on HIP device 0.  tonemap_op: UHDR_HIP_TONEMAP_SHIFT (toneMap) or
// UHDR_HIP_TONEMAP_REINHARD_MAXRGB; hdr_peak_nits = 0 measures the image's headroom, which *headroom (optional) receives.
status_t toneMapSdr(uhdr_uncompressed_ptr src, uhdr_uncompressed_ptr dest, ultrahdr_transfer_function hdr_tf, int tonemap_op,
                    float hdr_peak_nits = 0.0f, float* headroom = nullptr);

// The same operator on a packed HDR image (uhdr_hip_tonemap_packed): an ULTRAHDR_PIX_FMT_RGBA1010102 (HLG / PQ) or
// ULTRAHDR_PIX_FMT_RGBAF16 (linear) image in host memory becomes an ULTRAHDR_PIX_FMT_RGBA8888 one in dest->data (the caller's,
// rows dest->luma_stride pixels apart, 0 = width; the padding columns are left alone).  dest comes back described.
status_t toneMapPacked(uhdr_uncompressed_ptr hdr_image_ptr, uhdr_uncompressed_ptr dest, ultrahdr_transfer_function hdr_tf,
                       float hdr_peak_nits = 0.0f, float* headroom = nullptr);

// generateGainMap from a packed RGBA pair in DEVICE memory (uhdr_hip_generate_gainmap_packed_batch; no reference counterpart), on HIP
// device 0: an ULTRAHDR_PIX_FMT_RGBA8888 SDR image and an ULTRAHDR_PIX_FMT_RGBA1010102 (HLG / PQ) or ULTRAHDR_PIX_FMT_RGBAF16 (linear)
// HDR image, strides in pixels.  dest->data is the caller's device buffer -- (width / 4) * (height / 4) bytes, four times that
// (4-byte aligned, RGBA) with multi_channel; the call only enqueues on `stream`.  *metadata (optional) receives the reference's
// constants for hdr_tf, which the map is encoded against.
status_t generateGainMapPacked(uhdr_uncompressed_ptr sdr_image_ptr, uhdr_uncompressed_ptr hdr_image_ptr, ultrahdr_transfer_function hdr_tf,
                               ultrahdr_metadata_ptr metadata, uhdr_uncompressed_ptr dest, bool multi_channel = false, void* stream = nullptr);

// generateGainMapPacked against the range the content has (uhdr_hip_generate_gainmap_packed_adaptive; include/uhdr_hip.h,
// "content-adaptive gain maps for packed RGBA inputs"): the same arguments and buffers; *metadata (optional) receives the measured
// range, so the call waits for `stream`, as generateGainMapAdaptive does.
status_t generateGainMapPackedAdaptive(uhdr_uncompressed_ptr sdr_image_ptr, uhdr_uncompressed_ptr hdr_image_ptr, ultrahdr_transfer_function hdr_tf,
                                       ultrahdr_metadata_ptr metadata, uhdr_uncompressed_ptr dest, bool multi_channel = false,
                                       void* stream = nullptr);

// applyGainMap on a packed SDR image in DEVICE memory (uhdr_hip_apply_gainmap_packed_batch; no reference counterpart), on HIP device 0:
// an ULTRAHDR_PIX_FMT_RGBA8888 SDR image (stride in pixels) and its gain map -- ULTRAHDR_PIX_FMT_MONOCHROME / _UNSPECIFIED: one plane;
// ULTRAHDR_PIX_FMT_RGBA8888: per channel -- at any integer scale factor, with any valid metadata.  dest->data is the caller's device
// buffer of the output format's size; the call only enqueues on `stream`.  exact: the reference's bytes (UHDR_HIP_APPLY_EXACT),
// otherwise UHDR_HIP_APPLY_FAST.  dest comes back with width, height and the SDR image's gamut.
status_t applyGainMapPacked(uhdr_uncompressed_ptr sdr_image_ptr, uhdr_uncompressed_ptr gainmap_image_ptr, ultrahdr_metadata_ptr metadata,
                            ultrahdr_output_format output_format, float max_display_boost, uhdr_uncompressed_ptr dest, bool exact = false,
                            void* stream = nullptr);

// generateGainMap at the scale factor map_scale_factor, 1 .. 128, from a planar pair in DEVICE memory
// (uhdr_hip_generate_gainmap_scaled_batch; the reference's factor is 4), on HIP device 0.  dest->data is the caller's device buffer --
// (width / s) * (height / s) bytes, four times that (4-byte aligned, RGBA) with multi_channel; the call only enqueues on `stream`.
// *metadata (optional) receives the reference's constants for hdr_tf, which the map is encoded against.
status_t generateGainMapScaled(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr p010_image_ptr, ultrahdr_transfer_function hdr_tf,
                               ultrahdr_metadata_ptr metadata, uhdr_uncompressed_ptr dest, int map_scale_factor, bool multi_channel = false,
                               bool sdr_is_601 = false, void* stream = nullptr);

// The weight W of the gain-map exponent and the divisor d = min(max_display_boost, hdrCapacityMax) that a decode with
// JpegRHip::setAnyGainMapMetadata forms for this metadata (uhdr_hip_gainmap_weight; host code, no device needed)
status_t gainMapWeight(ultrahdr_metadata_ptr metadata, float max_display_boost, float* weight, float* display_boost);

// ---- editing effects: the free functions of lib/include/ultrahdr/editorhelper.h:49-63, same signatures ----------
enum ultrahdr_mirroring_direction : int { ULTRAHDR_MIRROR_VERTICAL = 0, ULTRAHDR_MIRROR_HORIZONTAL = 1 };

// host images in, host images out (out_img->data caller-allocated), executed on HIP device 0
status_t crop(uhdr_uncompressed_ptr const in_img, int left, int right, int top, int bottom, uhdr_uncompressed_ptr out_img);
status_t mirror(uhdr_uncompressed_ptr const in_img, ultrahdr_mirroring_direction mirror_dir, uhdr_uncompressed_ptr out_img);
status_t rotate(uhdr_uncompressed_ptr const in_img, int clockwise_degree, uhdr_uncompressed_ptr out_img);
status_t resize(uhdr_uncompressed_ptr const in_img, int out_width, int out_height, uhdr_uncompressed_ptr out_img);

// addEffects (lib/include/ultrahdr/editorhelper.h:27-47,62-63): the effect structs and the chaining call, same names
struct ultrahdr_effect {
  virtual ~ultrahdr_effect() = default;
};
struct ultrahdr_crop_effect : ultrahdr_effect { int left, right, top, bottom; };
struct ultrahdr_mirror_effect : ultrahdr_effect { ultrahdr_mirroring_direction mirror_dir; };
struct ultrahdr_rotate_effect : ultrahdr_effect { int clockwise_degree; };
struct ultrahdr_resize_effect : ultrahdr_effect { int new_width, new_height; };
status_t addEffects(uhdr_uncompressed_ptr const in_img, std::vector<ultrahdr_effect*>& effects, uhdr_uncompressed_ptr out_image);

// ---- JPEG helpers: the members callers use of JpegEncoderHelper (lib/include/ultrahdr/jpegencoderhelper.h:43-60) and of
// JpegDecoderHelper (lib/include/ultrahdr/jpegdecoderhelper.h:54-100), same names and meaning; host buffers in and out, the
// codec itself runs on HIP device 0 (uhdr_hip_jpeg_encode / uhdr_hip_jpeg_decode).
class JpegEncoderHelperHip {
 public:
  // uvBuffer == nullptr compresses the single plane yBuffer (the gain map, jpegr.cpp:294-297)
  bool compressImage(const uint8_t* yBuffer, const uint8_t* uvBuffer, int width, int height, int lumaStride, int chromaStride,
                     int quality, const void* iccBuffer, unsigned int iccSize);
  // Three planes of another sampling (no reference counterpart): pixelFormat UHDR_HIP_PIX_FMT_YUV444, YUV422 or YUV440, chroma of
  // ceil(width / hs) x ceil(height / vs) samples at cbBuffer, Cr chromaStride x chroma height behind Cb -- the layout
  // JpegDecoderHelperHip hands out for such files.  Any size from 1x1, odd ones included; edges are padded as libjpeg pads them
  // (uhdr_hip_jpeg_encode_planes_batch_opts).  UHDR_HIP_PIX_FMT_YUV420 and MONOCHROME: compressImage.
  bool compressPlanes(const uint8_t* yBuffer, const uint8_t* cbBuffer, int width, int height, int lumaStride, int chromaStride, int quality,
                      const void* iccBuffer, unsigned int iccSize, int pixelFormat);
  void* getCompressedImagePtr() { return mResultBuffer.data(); }
  size_t getCompressedImageSize() { return mResultBuffer.size(); }

 private:
  std::vector<uint8_t> mResultBuffer;
};

// jpegdecoderhelper.h:34-38 (PARSE_ONLY is served by getCompressedImageParameters there and by JpegRHip::getJPEGRInfo here)
enum decode_mode_t : int { DECODE_TO_RGBA = 1, DECODE_TO_YCBCR = 2 };

class JpegDecoderHelperHip {
 public:
  // DECODE_TO_YCBCR (what applyGainMap's caller asks for, jpegr.cpp:780-801): 4:2:0 -> Y, Cb, Cr planes; grayscale -> Y.
  // DECODE_TO_RGBA (the SDR rendition, jpegr.cpp:686-690): 4:2:0 -> RGBA8888 with libjpeg-turbo's arithmetic.
  // scaleDenom 2, 4 or 8 (uhdr_hip_jpeg_decode_scaled): the image at ceil(size / scaleDenom) -- a 4:2:0 file as three planes of that
  // size (Y, Cb, Cr: 4:4:4) or RGBA8888, a single-plane file as its plane; any other value but 1 fails.
  bool decompressImage(const void* image, int length, decode_mode_t decodeTo = DECODE_TO_YCBCR, int scaleDenom = 1);
  void* getDecompressedImagePtr() { return mResultBuffer.data(); }
  size_t getDecompressedImageSize() { return mResultBuffer.size(); }
  size_t getDecompressedImageWidth() { return mWidth; }
  size_t getDecompressedImageHeight() { return mHeight; }
  bool isSingleChannel() { return mSingleChannel; }

 private:
  std::vector<uint8_t> mResultBuffer;
  size_t mWidth = 0, mHeight = 0;
  bool mSingleChannel = false;
};

// ---- the JPEG/R codec: the public members of ultrahdr::JpegR (lib/include/ultrahdr/jpegr.h:59-265), same names, argument meaning,
// defaults and status values; structs as in ultrahdr.h:186-207 and jpegr.h:37-57.  Host buffers in and out; toneMap, gain-map
// generation / application and both JPEG codecs run on HIP device 0 (uhdr_hip_jpegr_*), the container is parsed / assembled on
// the host.  decodeJPEGR(ULTRAHDR_OUTPUT_SDR) returns the primary image as RGBA8888 with libjpeg-turbo's DECODE_TO_RGBA arithmetic.
struct ultrahdr_compressed_struct {
  void* data;
  int length;
  int maxLength;
  ultrahdr_color_gamut colorGamut;
};
using uhdr_compressed_ptr = ultrahdr_compressed_struct*;
struct ultrahdr_exif_struct {
  void* data;
  size_t length;
};
using uhdr_exif_ptr = ultrahdr_exif_struct*;
struct jpeg_info_struct {
  std::vector<uint8_t> imgData, iccData, exifData, xmpData;
  size_t width, height;
};
struct jpegr_info_struct {
  size_t width, height;
  jpeg_info_struct* primaryImgInfo = nullptr;
  jpeg_info_struct* gainmapImgInfo = nullptr;
};
using j_info_ptr = jpeg_info_struct*;
using uhdr_info_ptr = jpegr_info_struct*;

class JpegRHip {
 public:
  // API-0 (jpegr.h:81) and API-1 (:103)
  status_t encodeJPEGR(uhdr_uncompressed_ptr p010_image_ptr, ultrahdr_transfer_function hdr_tf, uhdr_compressed_ptr dest, int quality,
                       uhdr_exif_ptr exif);
  status_t encodeJPEGR(uhdr_uncompressed_ptr p010_image_ptr, uhdr_uncompressed_ptr yuv420_image_ptr, ultrahdr_transfer_function hdr_tf,
                       uhdr_compressed_ptr dest, int quality, uhdr_exif_ptr exif);
  // API-2 (:127), API-3 (:150), API-4 (:168)
  status_t encodeJPEGR(uhdr_uncompressed_ptr p010_image_ptr, uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_compressed_ptr yuv420jpg_image_ptr,
                       ultrahdr_transfer_function hdr_tf, uhdr_compressed_ptr dest);
  status_t encodeJPEGR(uhdr_uncompressed_ptr p010_image_ptr, uhdr_compressed_ptr yuv420jpg_image_ptr, ultrahdr_transfer_function hdr_tf,
                       uhdr_compressed_ptr dest);
  status_t encodeJPEGR(uhdr_compressed_ptr yuv420jpg_image_ptr, uhdr_compressed_ptr gainmapjpg_image_ptr, ultrahdr_metadata_ptr metadata,
                       uhdr_compressed_ptr dest);
  // "API-x" (:263): SDR planes + ready gain map + metadata
  status_t encodeJPEGR(uhdr_uncompressed_ptr yuv420_image_ptr, uhdr_uncompressed_ptr gainmap_image_ptr, ultrahdr_metadata_ptr metadata,
                       uhdr_compressed_ptr dest, int quality, uhdr_exif_ptr exif);
  // Packed RGBA inputs (include/uhdr_hip.h, "packed RGBA inputs"; no reference counterpart): an ULTRAHDR_PIX_FMT_RGBA1010102 (HLG / PQ)
  // or ULTRAHDR_PIX_FMT_RGBAF16 (linear) HDR image and an ULTRAHDR_PIX_FMT_RGBA8888 SDR image, host memory, luma_stride in pixels
  // (0 = width), full range.  The gain map comes from the packed pair itself, the primary image is the SDR image compressed as
  // 4:2:0 from RGB, the container is API-1's (uhdr_hip_jpegr_encode_packed_batch).  Honours setMultiChannelGainMap and, together
  // with it, setContentBoost (uhdr_hip_jpegr_encode_packed_adaptive_batch); setToneMap does not apply: the SDR image is given.
  status_t encodeJPEGRPacked(uhdr_uncompressed_ptr hdr_image_ptr, uhdr_uncompressed_ptr sdr_image_ptr, ultrahdr_transfer_function hdr_tf,
                             uhdr_compressed_ptr dest, int quality, uhdr_exif_ptr exif);
  // The packed API-0 (include/uhdr_hip.h, "tone-mapped SDR image from a packed HDR image"): the HDR image alone; the SDR image is
  // tone-mapped from it on the device (uhdr_hip_jpegr_encode_packed_api0_batch).  Honours setMultiChannelGainMap and the
  // hdr_peak_nits given to setToneMap (0, the default, measures the headroom); the operator is always REINHARD_MAXRGB.  Honours
  // setContentBoost as the overload above does, with that peak.
  status_t encodeJPEGRPacked(uhdr_uncompressed_ptr hdr_image_ptr, ultrahdr_transfer_function hdr_tf, uhdr_compressed_ptr dest, int quality,
                             uhdr_exif_ptr exif);
  // (:213) dest->data, exif->data and gainmap_image_ptr->data are caller-allocated, as in the reference
  status_t decodeJPEGR(uhdr_compressed_ptr jpegr_image_ptr, uhdr_uncompressed_ptr dest, float max_display_boost = 3.4028234663852886e38f,
                       uhdr_exif_ptr exif = nullptr, ultrahdr_output_format output_format = ULTRAHDR_OUTPUT_HDR_LINEAR,
                       uhdr_uncompressed_ptr gainmap_image_ptr = nullptr, ultrahdr_metadata_ptr metadata = nullptr);
  // (:231)
  status_t getJPEGRInfo(uhdr_compressed_ptr jpegr_image_ptr, uhdr_info_ptr jpeg_image_info_ptr);

  void setApplyMode(int mode) { mApplyMode = mode; }   // UHDR_HIP_APPLY_EXACT (default here: decoded files equal the reference's), FAST, LUT
  // -1 (default): the reference's constant boost range.  UHDR_HIP_BOOST_PER_IMAGE / UHDR_HIP_BOOST_PER_CALL: the API-0 and API-1
  // overloads encode the gain map against the range the content has (uhdr_hip_jpegr_encode_adaptive_batch), and so do both
  // encodeJPEGRPacked overloads (uhdr_hip_jpegr_encode_packed_adaptive_batch); the others are unchanged
  void setContentBoost(int scope_or_minus_one) { mContentBoost = scope_or_minus_one; }
  // UHDR_HIP_TONEMAP_SHIFT (default): the API-0 overload derives its SDR image like the reference, by bit shift.
  // UHDR_HIP_TONEMAP_REINHARD_MAXRGB: tone-mapped from linear light against the image's headroom -- measured, or hdr_peak_nits / 203
  // when hdr_peak_nits > 0 (uhdr_hip_jpegr_encode_api0_tonemapped_batch); combines with setContentBoost.  The others are unchanged
  void setToneMap(int tonemap_op, float hdr_peak_nits = 0.0f) { mToneMapOp = tonemap_op; mHdrPeakNits = hdr_peak_nits; }
  // false (default): decodeJPEGR reads what the reference reads, 4:2:0 primaries.  true: also 4:4:4, 4:2:2 and 4:4:0 ones
  // (UHDR_HIP_DECODE_ANY_SAMPLING)
  void setDecodeAnySampling(bool on) { mDecodeAnySampling = on; }
  // false (default): one-plane gain maps, as the reference writes and reads them.  true: the API-0 and API-1 overloads of encodeJPEGR
  // write a per-channel (RGB) gain map (uhdr_hip_jpegr_encode_rgbmap_batch; it takes precedence over setToneMap and setContentBoost,
  // which are single-channel) and decodeJPEGR applies a three-component gain map per channel
  // (uhdr_hip_jpegr_decode_rgbmap_batch; files with one-plane maps decode as ever).  The other encodeJPEGR overloads are unchanged.
  void setMultiChannelGainMap(bool on) { mMultiChannelGainMap = on; }
  // 4 (default): the reference's kMapDimensionScaleFactor.  Any other factor, 1 .. 128: the API-0 and API-1 overloads write the gain
  // map at that factor (uhdr_hip_jpegr_encode_scaled_batch; it combines with setMultiChannelGainMap; an image the factor does not
  // divide is ERROR_ULTRAHDR_UNSUPPORTED_WIDTH_HEIGHT).  Every other way of generating a map -- API-2, API-3, encodeJPEGRPacked, the
  // setToneMap operator, setContentBoost -- then answers ERROR_ULTRAHDR_UNSUPPORTED_FEATURE instead of silently writing a factor-4 map.
  // decodeJPEGR reads every factor as it is.
  void setGainMapScaleFactor(int map_scale_factor) { mGainMapScaleFactor = map_scale_factor; }
  // false (default): decodeJPEGR refuses, as the reference does, every file whose metadata has a gamma other than 1, an offset
  // other than 0 or an HDR capacity range other than the content boost range (ERROR_ULTRAHDR_BAD_METADATA).  true: such files --
  // what current libultrahdr, cameras and editors write -- are decoded with the full gain-map formula, one- and three-component
  // maps alike (uhdr_hip_jpegr_decode_md_batch); files the reference reads give the bytes they gave.
  void setAnyGainMapMetadata(bool on) { mAnyGainMapMetadata = on; }
  // 1 (default): decodeJPEGR as it is.  2, 4 or 8: the rendition at ceil(size / denominator), decoded at that size -- reduced inverse
  // DCTs, the gain map at the factor (or the size) that follows (uhdr_hip_jpegr_decode_scaled_batch; it reads what
  // setAnyGainMapMetadata(true) and setMultiChannelGainMap(true) read).  dest->data holds the scaled image; gainmap_image_ptr, if
  // given, still receives the map at its full size.  Any other value: ERROR_ULTRAHDR_UNSUPPORTED_FEATURE from decodeJPEGR.
  void setDecodeScaleDenom(int scale_denom) { mDecodeScaleDenom = scale_denom; }
  // false (default): the Annex K Huffman tables, as the reference writes them.  true: the API-0 and API-1 overloads of encodeJPEGR
  // write the primary image and the gain-map JPEG with Huffman tables of their own (uhdr_hip_jpegr_encode_batch_ex with
  // UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN): the same pixels in smaller files.  Combined with setGainMapScaleFactor, setMultiChannelGainMap,
  // setToneMap or setContentBoost those two overloads answer ERROR_ULTRAHDR_UNSUPPORTED_FEATURE instead of silently writing default
  // tables.  Every other encodeJPEGR overload and encodeJPEGRPacked keep the default tables, whatever is set here.
  void setOptimizeHuffman(bool on) { mOptimizeHuffman = on; }
  // libjpeg's restart_interval and restart_in_rows for the same two overloads (uhdr_hip_jpegr_encode_batch_opts): the primary image
  // and the gain-map JPEG are written with a DRI segment and RSTn markers after every `mcus` MCUs, or after every `rows` MCU rows of
  // each image's own width (rows override mcus; 0 and 0, the default: none).  The pixels do not change.  They combine with
  // setOptimizeHuffman and refuse what it refuses: with setGainMapScaleFactor, setMultiChannelGainMap, setToneMap or setContentBoost
  // those overloads answer ERROR_ULTRAHDR_UNSUPPORTED_FEATURE, as they do for an interval above 65535.  Every other overload writes
  // no intervals, whatever is set here.
  void setRestartInterval(unsigned mcus) { mRestartInterval = mcus; }
  void setRestartInRows(unsigned rows) { mRestartInRows = rows; }
  // false (default): baseline files.  true: the same two overloads write the primary image and the gain-map JPEG as progressive files
  // (uhdr_hip_jpegr_encode_batch_scans with UHDR_HIP_SCANS_PROGRESSIVE: SOF2, libjpeg's simple progression, tables of its own in
  // every scan whatever setOptimizeHuffman says).  The pixels do not change, and decodeJPEGR reads the file.  It refuses what
  // setOptimizeHuffman refuses -- setGainMapScaleFactor, setMultiChannelGainMap, setToneMap, setContentBoost -- and a restart setting
  // with ERROR_ULTRAHDR_UNSUPPORTED_FEATURE, as does encodeJPEGRPacked with a setPrimarySampling other than 4:2:0, the one place where
  // a packed overload reads these options.  Every other overload writes baseline files, whatever is set here.
  void setProgressive(bool on) { mProgressive = on; }
  // UHDR_HIP_PIX_FMT_YUV420 (default): both encodeJPEGRPacked overloads compress the SDR image as 4:2:0.  UHDR_HIP_PIX_FMT_YUV444 or
  // YUV422: the primary image keeps its chroma at full or at half horizontal resolution (uhdr_hip_jpegr_encode_packed_sampling_batch;
  // the overload without an SDR image tone-maps one first, as the packed API-0 does); gain map, metadata and container do not change,
  // and decodeJPEGR reads the file with setDecodeAnySampling(true).  With such a sampling those overloads also honour
  // setOptimizeHuffman, setRestartInterval and setRestartInRows, and answer ERROR_ULTRAHDR_UNSUPPORTED_FEATURE for setContentBoost and
  // for any other value given here.  Every encodeJPEGR overload is unchanged: its SDR image is 4:2:0.
  void setPrimarySampling(int pixel_format) { mPrimarySampling = pixel_format; }

 private:
  int mApplyMode = 1;
  int mContentBoost = -1;
  int mToneMapOp = 0;
  float mHdrPeakNits = 0.0f;
  bool mDecodeAnySampling = false;
  int mDecodeScaleDenom = 1;
  bool mMultiChannelGainMap = false;
  bool mAnyGainMapMetadata = false;
  bool mOptimizeHuffman = false;
  unsigned mRestartInterval = 0, mRestartInRows = 0;
  bool mProgressive = false;
  int mGainMapScaleFactor = 4;
  int mPrimarySampling = 1;   // UHDR_HIP_PIX_FMT_YUV420
};

}  // namespace ultrahdr

#endif  // ULTRAHDR_HIP_SHIM_H
