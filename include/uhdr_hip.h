/*
 * uhdr_hip.h -- C-ABI of the MI355X (gfx950) gain-map pixel path.
 *
 * This is the drop-in boundary for the per-pixel hot path of libultrahdr_dev.  The reference has
 * no FFI layer: the path sits behind three protected C++ members of ultrahdr::UltraHdr plus one
 * private member of JpegR.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference tree); INTEGRATION.md shows the binding a maintainer adds.
 *
 *   uhdr_hip_generate_gainmap   <- UltraHdr::generateGainMap   lib/include/ultrahdr/ultrahdr.h:348-350
 *                                                              lib/src/ultrahdr.cpp:185-358
 *   uhdr_hip_apply_gainmap      <- UltraHdr::applyGainMap      lib/include/ultrahdr/ultrahdr.h:370-372
 *                                                              lib/src/ultrahdr.cpp:360-515
 *   uhdr_hip_tonemap            <- UltraHdr::toneMap           lib/include/ultrahdr/ultrahdr.h:381
 *                                                              lib/src/ultrahdr.cpp:517-558
 *   uhdr_hip_convert_yuv        <- JpegR::convertYuv           lib/include/ultrahdr/jpegr.h:329-330
 *                                                              lib/src/jpegr.cpp:1132-1206
 *
 * Conventions
 *  - plain C, POD only; no torch / STL types.  Enum VALUES are the reference's
 *    (lib/include/ultrahdr/ultrahdr.h:36-120).  Return value is the reference's status_t value
 *    for the same inputs (first failing check wins, same order); HIP failures map to
 *    UHDR_HIP_UNKNOWN_ERROR (-1); "no usable GPU / library not initialised" is
 *    UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE (-20009).  There is NO CPU fallback.
 *  - images use the reference descriptor (ultrahdr_uncompressed_struct, ultrahdr.h:152-181):
 *    strides in PIXELS (P010 chroma stride counts uint16 elements of the interleaved plane),
 *    chroma_data must be non-NULL (callers normalise exactly as jpegr.cpp:265-278 does).
 *    YUV420: U plane at chroma_data, V plane at chroma_data + chroma_stride*(height/2).
 *  - mem_space says where every data pointer of the call lives:
 *      UHDR_HIP_MEM_DEVICE  device pointers; the call only enqueues kernels on `stream`
 *                           (asynchronous; graph-capturable; nothing is allocated or copied -- with three
 *                           exceptions, each the FIRST use of a stream's workspace: a generate launch of more
 *                           than a few images allocates the stream's 21 MiB statistics workspace, an EXACT apply
 *                           its lists of pixels in doubt (first call, and again for larger images), and an apply
 *                           with a map scale factor the device holds no weight table for uploads one and waits.
 *                           uhdr_hip_stream_reserve() does all of that ahead of time -- call it before capturing
 *                           a graph --, uhdr_hip_stream_release() gives a stream's workspace back);
 *      UHDR_HIP_MEM_HOST    host pointers; the library stages through its own device workspace
 *                           (H2D, kernels, D2H) and returns after the result is back in host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - the library never allocates result memory on behalf of the caller: the gain map buffer
 *    ((width/4)*(height/4) bytes) is caller-provided in dest->data.  (The C++ shim in
 *    include/ultrahdr_hip/ultrahdr_hip.h reproduces the reference's new[] contract on top of this.)
 */
#ifndef UHDR_HIP_H
#define UHDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UHDR_HIP_ABI_VERSION 3

/* ultrahdr_color_gamut, ultrahdr.h:36-42 */
#define UHDR_HIP_CG_UNSPECIFIED (-1)
#define UHDR_HIP_CG_BT709 0
#define UHDR_HIP_CG_P3 1
#define UHDR_HIP_CG_BT2100 2
/* ultrahdr_transfer_function, ultrahdr.h:46-53 */
#define UHDR_HIP_TF_LINEAR 0
#define UHDR_HIP_TF_HLG 1
#define UHDR_HIP_TF_PQ 2
#define UHDR_HIP_TF_SRGB 3
/* ultrahdr_output_format, ultrahdr.h:56-64 */
#define UHDR_HIP_OUTPUT_SDR 0
#define UHDR_HIP_OUTPUT_HDR_LINEAR 1            /* RGBA F16, 8 B/pixel */
#define UHDR_HIP_OUTPUT_HDR_PQ 2                /* RGBA1010102, 4 B/pixel */
#define UHDR_HIP_OUTPUT_HDR_HLG 3               /* RGBA1010102, 4 B/pixel */
#define UHDR_HIP_OUTPUT_HDR_LINEAR_RGB_10BIT 4  /* three planar uint16 planes, 6 B/pixel */
/* ultrahdr_pixel_format, ultrahdr.h:67-75 */
#define UHDR_HIP_PIX_FMT_UNSPECIFIED (-1)
#define UHDR_HIP_PIX_FMT_P010 0
#define UHDR_HIP_PIX_FMT_YUV420 1
#define UHDR_HIP_PIX_FMT_MONOCHROME 2
/* (no counterpart in the reference) 8-bit YCbCr at other samplings: what the UHDR_HIP_DECODE_ANY_SAMPLING decodes return and
 * uhdr_hip_apply_gainmap[_batch] reads as the SDR image.  As for YUV420, data = Y, chroma_data = Cb, and Cr sits
 * chroma_stride * chroma_height bytes behind Cb; the chroma extent is libjpeg's downsampled size, rounded up (any width / height): */
#define UHDR_HIP_PIX_FMT_YUV444 3               /* chroma width x height */
#define UHDR_HIP_PIX_FMT_YUV422 4               /* chroma ceil(width / 2) x height */
#define UHDR_HIP_PIX_FMT_YUV440 5               /* chroma width x ceil(height / 2) */
/* A per-channel (RGB) gain map, read and written only by the *_rgb_* / *_rgbmap_* calls: interleaved R, G, B, A bytes, 4 per map
 * pixel; data points at pixel (0, 0) and is 4-byte aligned, luma_stride is in PIXELS (0 = width), chroma_data = NULL.  Calls that
 * write a map set A = 0xFF, calls that read one ignore A.  It is the layout UHDR_HIP_DECODE_TO_RGBA produces. */
#define UHDR_HIP_PIX_FMT_RGBA8888 6
/* Packed RGBA images, read by the *_packed_* calls and uhdr_hip_jpeg_encode_rgba420_batch (no counterpart in the reference; current
 * libultrahdr takes the same three layouts as raw encode inputs).  They are the layouts the apply / decode calls WRITE.
 *   RGBA8888 (6, above)  also an SDR image: sRGB transfer, full range, R, G, B, A bytes in that order, alpha ignored.
 *   RGBA1010102          an HDR image, one dword per pixel, R | G << 10 | B << 20 | A << 30, full range, HLG or PQ: what
 *                        UHDR_HIP_OUTPUT_HDR_HLG / UHDR_HIP_OUTPUT_HDR_PQ write.  Alpha ignored.
 *   RGBA_F16             an HDR image, four halves R, G, B, A per pixel, linear light, 1.0 = 1000 nits (the reference's kHlgMaxNits,
 *                        what its ULTRAHDR_TF_LINEAR means, ultrahdr.cpp:223-228): what UHDR_HIP_OUTPUT_HDR_LINEAR writes.  Alpha ignored.
 * For all three, as for RGBA maps: data points at pixel (0, 0), luma_stride is in PIXELS (0 = width), chroma_data is not read; data
 * is 4-byte aligned, 8-byte for RGBA_F16. */
#define UHDR_HIP_PIX_FMT_RGBA1010102 7
#define UHDR_HIP_PIX_FMT_RGBA_F16 8
/* status_t, ultrahdr.h:91-120 */
#define UHDR_HIP_NO_ERROR 0
#define UHDR_HIP_UNKNOWN_ERROR (-1)
#define UHDR_HIP_ERROR_BAD_PTR (-10001)
#define UHDR_HIP_ERROR_INVALID_COLORGAMUT (-10003)
#define UHDR_HIP_ERROR_INVALID_TRANS_FUNC (-10005)
#define UHDR_HIP_ERROR_RESOLUTION_MISMATCH (-10006)
#define UHDR_HIP_ERROR_BAD_METADATA (-10010)
#define UHDR_HIP_ERROR_INVALID_CROPPING_PARAMETERS (-10011)
#define UHDR_HIP_ERROR_UNSUPPORTED_FEATURE (-30000)
#define UHDR_HIP_ERROR_UNSUPPORTED_MAP_SCALE_FACTOR (-20008)
#define UHDR_HIP_ERROR_INSUFFICIENT_RESOURCE (-20009)

/* where the planes of a call live.  DEVICE: the call only enqueues kernels on `stream` (asynchronous, graph-capturable).  HOST
 * (what a caller of the reference binds): the call copies the planes in, runs, copies the result out and returns when it is there.
 * Threads: every entry point may be called from several host threads.  Device-memory calls on different streams overlap; the
 * host-memory forms of generate / apply / tonemap / convert_yuv lease a staging set per call, so callers on their own streams
 * overlap their copies and kernels as well (one thread moves 0.54, eight 0.94 4K pairs per ms over the host link); the codec entry
 * points (jpeg_*, jpegr_*, the effects and table calls through host memory) lease a codec context per call -- staging buffers,
 * decoder workspaces, encoder pools -- so callers on their own streams overlap too (a JPEG decode is latency-bound: two threads
 * decode nearly twice as many files per second as one). */
#define UHDR_HIP_MEM_HOST 0
#define UHDR_HIP_MEM_DEVICE 1
/* uhdr_hip_jpeg_encode_batch only: planes and outputs in different memory spaces */
#define UHDR_HIP_MEM_DEVICE_TO_HOST 2   /* planes in device memory, outputs in host memory */
#define UHDR_HIP_MEM_HOST_TO_DEVICE 3   /* planes in host memory, outputs in device memory */

/* arithmetic mode of uhdr_hip_apply_gainmap*:
 *   FAST  : transfer functions from line-segment tables in LDS (special-function unit where a call can exceed 1.0); every
 *           10-bit channel within 1 LSB and every F16 channel within 1 half-ULP of the reference CPU path;
 *   EXACT : the same bytes as the reference CPU path: its float/double promotion pattern replayed with correctly
 *           rounded pow/exp/log/exp2, on the pixels an f32 estimate with measured error bounds cannot settle (~1 %).
 *           The first EXACT call on a stream (and the first with larger images) allocates that stream's list workspace;
 *           after it the call only enqueues two kernels and can be captured into a graph like the others.
 * generate/tonemap/convert_yuv have a single, bit-exact mode. */
#define UHDR_HIP_APPLY_FAST 0
#define UHDR_HIP_APPLY_EXACT 1
/* LUT mode (opt-in): the loops as a build that sees jpegr.cpp:33-38's
 * USE_*_LUT = 1 compiles them (upstream libultrahdr's configuration; dead code in this fork, whose
 * ultrahdr.cpp never sees those macros).  apply: srgbInvOetfLUT + applyGainLUT(GainLUT(metadata,
 * display_boost)) + hlgOetfLUT / pqOetfLUT (ultrahdr.cpp:433,446,470,481); generate: srgbInvOetfLUT +
 * hlgInvOetfLUT / pqInvOetfLUT (:230,238,319).  Tables are built on the device by the exact functions
 * (gainmapmath.cpp:21-64); with them the LUT pipelines are pure float/integer work and BIT-EXACT against
 * the reference's LUT functions. */
#define UHDR_HIP_APPLY_LUT 2
/* EXACT without its f32 pre-filter: every pixel takes the double-precision path (what EXACT always does for HDR_PQ).  Same
 * bytes as UHDR_HIP_APPLY_EXACT; kept as a verification switch for tests. */
#define UHDR_HIP_APPLY_EXACT_UNFILTERED 3
#define UHDR_HIP_GENERATE_EXACT 0
#define UHDR_HIP_GENERATE_LUT 1
/* EXACT without the f32 pre-filter: every pixel takes the double-precision path.  Same bytes and statistics as
 * UHDR_HIP_GENERATE_EXACT by construction (the filter only decides which waves can skip that path); kept as a
 * verification switch for tests. */
#define UHDR_HIP_GENERATE_UNFILTERED 2

/* POD mirror of ultrahdr_uncompressed_struct (ultrahdr.h:152-181) */
typedef struct uhdr_hip_image {
  void* data;           /* luma plane (or gain map / packed output) */
  size_t width;         /* luma width in pixels */
  size_t height;        /* luma height in pixels */
  int32_t colorGamut;   /* UHDR_HIP_CG_* */
  void* chroma_data;    /* U plane (YUV420) / interleaved UV plane (P010); must be non-NULL */
  size_t luma_stride;   /* pixels */
  size_t chroma_stride; /* pixels (P010: uint16 elements of the interleaved plane) */
  int32_t pixelFormat;  /* UHDR_HIP_PIX_FMT_* */
} uhdr_hip_image_t;

/* POD mirror of ultrahdr_metadata_struct (ultrahdr.h:129-147); version is the NUL-terminated
 * string the reference keeps in a std::string ("1.0", ultrahdr.h:210) */
typedef struct uhdr_hip_metadata {
  char version[8];
  float maxContentBoost;
  float minContentBoost;
  float gamma;
  float offsetSdr;
  float offsetHdr;
  float hdrCapacityMin;
  float hdrCapacityMax;
} uhdr_hip_metadata_t;

/* ---- library / device management -------------------------------------------------------- */

/* ABI version of the loaded library (== UHDR_HIP_ABI_VERSION of the header it was built from) */
int uhdr_hip_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU; never fails) */
int uhdr_hip_device_count(void);
/* bind the calling process to `device` (hipSetDevice), upload the constant tables, create the
 * staging workspace.  Must be called once per device before any compute call. */
int uhdr_hip_init(int device);
/* release the workspace of every initialised device */
int uhdr_hip_shutdown(void);
/* Allocate, now, what device-memory calls on `stream` would otherwise allocate at their first use (see mem_space above): the
 * statistics workspace of generate, and -- when exact_images > 0 -- the lists EXACT apply needs for launches of up to
 * exact_images images of width x height pixels (at most 64 per launch; 0 for width / height with exact_images == 0), and the
 * sampleMap weight table of `map_scale_factor` (0: none; 4 is always resident).  After this the calls it covers only enqueue. */
int uhdr_hip_stream_reserve(void* stream, int exact_images, size_t width, size_t height, int map_scale_factor);
/* Free what the library holds for `stream` (waits for the stream first): its statistics workspace, its EXACT-apply lists and the
 * smaller lists those outgrew.  A service that creates and destroys streams calls this before hipStreamDestroy: workspaces are
 * keyed by the stream handle, and a recycled handle would inherit the old one.  NOT returned: what belongs to the device rather
 * than to a stream (staging sets of host-memory calls, codec contexts, weight tables) -- uhdr_hip_shutdown() frees those. */
int uhdr_hip_stream_release(void* stream);
/* last HIP error text seen by the library on this thread ("" if none) */
const char* uhdr_hip_last_error(void);

/* ---- where resident images lie in device memory (no reference counterpart: the reference's images live in malloc'ed host memory) ----
 * Any device pointer works with every call.  But WHICH physical memory a batch of images occupies decides what the card's HBM gives
 * the streaming kernels: a batch in one physically contiguous stretch (what hipMalloc returns on a device whose memory is mostly free)
 * runs apply 6-7 % slower than the same batch in pieces taken from all over a region three or more times its size, whatever the
 * virtual layout (profiles/r04_placement.txt).  A pool takes `bytes` of device memory as chunks of `chunk_bytes` through
 * the HIP virtual-memory calls; an allocation is one contiguous range of virtual addresses backed by chunks spaced evenly over the
 * pool's free ones -- so the images of several allocations interleave physically.  Intended use: at start-up, one pool over a wide
 * stretch of the card (tens of GiB and more: a pool no larger than what it holds is fast or not by where it happens to lie), one
 * allocation per arena of what stays resident (frames, maps, renditions), then uhdr_hip_mem_pool_trim() for the rest.
 *   bytes        rounded up to whole chunks; fails with ERROR_INSUFFICIENT_RESOURCE when the device does not have them
 *   chunk_bytes  0 = 16 MiB; a multiple of 2 MiB
 * ERROR_BAD_PTR for a NULL argument, ERROR_UNSUPPORTED_FEATURE for a size of 0, a chunk size that is no multiple of 2 MiB, a device
 * that does not exist or a pointer the pool did not hand out.
 * alloc: ERROR_INSUFFICIENT_RESOURCE when fewer free chunks are left than the size needs; free returns the chunks to the pool (the
 * pointer must be one alloc returned, with no work outstanding on it); trim gives the chunks no allocation uses back to the device;
 * destroy unmaps and releases everything (allocations included).  Calls on one pool are serialised by the library. */
typedef struct uhdr_hip_mem_pool uhdr_hip_mem_pool_t;
int uhdr_hip_mem_pool_create(int device, size_t bytes, size_t chunk_bytes, uhdr_hip_mem_pool_t** pool);
int uhdr_hip_mem_pool_alloc(uhdr_hip_mem_pool_t* pool, size_t bytes, void** ptr);
int uhdr_hip_mem_pool_free(uhdr_hip_mem_pool_t* pool, void* ptr);
int uhdr_hip_mem_pool_trim(uhdr_hip_mem_pool_t* pool);
int uhdr_hip_mem_pool_destroy(uhdr_hip_mem_pool_t* pool);
/* chunks the pool holds / of those, chunks no allocation uses (either pointer may be NULL) */
int uhdr_hip_mem_pool_stats(uhdr_hip_mem_pool_t* pool, size_t* chunks, size_t* free_chunks);

/* ---- single image ------------------------------------------------------------------------ */

/* UltraHdr::generateGainMap (ultrahdr.cpp:185-358).  Writes the (width/4)x(height/4) u8 map into
 * dest->data (caller-allocated, stride == map width), fills dest->{width,height,colorGamut,
 * luma_stride,chroma_data,chroma_stride,pixelFormat} and *metadata (the reference's constants,
 * ultrahdr.cpp:250-257). */
int uhdr_hip_generate_gainmap(const uhdr_hip_image_t* yuv420_image, const uhdr_hip_image_t* p010_image,
                              int hdr_tf, uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest,
                              int sdr_is_601, int mem_space, void* stream);

/* the same with an arithmetic mode: UHDR_HIP_GENERATE_EXACT (what uhdr_hip_generate_gainmap runs) or _LUT */
int uhdr_hip_generate_gainmap_ex(const uhdr_hip_image_t* yuv420_image, const uhdr_hip_image_t* p010_image,
                                 int hdr_tf, uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest,
                                 int sdr_is_601, int generate_mode, int mem_space, void* stream);

/* UltraHdr::applyGainMap (ultrahdr.cpp:360-515).  dest->data is caller-allocated:
 * width*height*{8|4|6} bytes for HDR_LINEAR | HDR_PQ,HDR_HLG | HDR_LINEAR_RGB_10BIT; any other
 * output_format writes nothing and returns NO_ERROR, like the reference (ultrahdr.cpp:491-493).
 * What is read of a 4:2:0 image: chroma sample (y >> 1) * chroma_stride + (x >> 1), Cb from chroma_data and Cr chroma_stride *
 * (height / 2) bytes behind it, exactly as the reference's getYuv420Pixel.  For an odd width or height (both at least 2) that reaches
 * past the (width / 2) x (height / 2) planes: when chroma_data follows the luma (luma_stride == width, chroma_stride == width / 2),
 * floor(3 * width * height / 2) bytes are read from `data`, and they must be readable.  For width = 2 (mod 4) with an odd height
 * (and wherever width*height mod 4 is 2 or 3) that is ONE BYTE MORE than the width*height + 2 * (width*height / 4) bytes
 * uhdr_hip_jpeg_decode asks for and writes, and with such a width and height the last Cr sample read is that byte: a caller who
 * applies a map to such a decoded image gives the buffer one byte more and sets it to zero, which is what the reference's zeroed
 * result buffer holds there.  The same holds for every uhdr_hip_apply_gainmap* call below. */
int uhdr_hip_apply_gainmap(const uhdr_hip_image_t* yuv420_image, const uhdr_hip_image_t* gainmap_image,
                           const uhdr_hip_metadata_t* metadata, int output_format,
                           float max_display_boost, uhdr_hip_image_t* dest, int apply_mode,
                           int mem_space, void* stream);

/* UltraHdr::toneMap (ultrahdr.cpp:517-558): P010 -> YUV420 by bit shift, stride padding zeroed. */
int uhdr_hip_tonemap(const uhdr_hip_image_t* src, uhdr_hip_image_t* dest, int mem_space, void* stream);

/* JpegR::convertYuv (jpegr.cpp:1132-1206): in-place YUV420 matrix re-encode between
 * BT.709 / BT.601(P3) / BT.2100 encodings. */
int uhdr_hip_convert_yuv(uhdr_hip_image_t* image, int src_encoding, int dest_encoding, int mem_space,
                         void* stream);

/* The same two over n images in DEVICE memory (every op in single and batched form; the reference runs them once
 * per image, ultrahdr.cpp:517-558 / jpegr.cpp:1132-1206).  Images of equal size share one launch (grid.z = image, up to 32), so an
 * API-0 / API-1 encode of a batch does not pay a launch pair per image.  Checks are the single form's, all images before any launch. */
int uhdr_hip_tonemap_batch(int n, const uhdr_hip_image_t* srcs, uhdr_hip_image_t* dests, void* stream);
int uhdr_hip_convert_yuv_batch(int n, uhdr_hip_image_t* images, int src_encoding, int dest_encoding, void* stream);

/* ---- editing effects (SURVEY.md 8(f) "next", rank 3) -------------------------------------------------
 * crop / mirror / rotate / resize of lib/src/editorhelper.cpp:26-360 (lib/include/ultrahdr/editorhelper.h:49-63)
 * on YUV420 or MONOCHROME images, byte-identical to the reference including its layout rules: the output is
 * tightly packed (luma then U then V at out->data) except mirror and rotate-180, whose output strides follow
 * the INPUT luma stride; crop's chroma copy runs over the full output height (:72).  out->data is
 * caller-allocated; the call fills the other fields of *out.  in->chroma_data == NULL means "right after luma",
 * strides of 0 mean "width" / "luma stride / 2", as in the reference. */
int uhdr_hip_crop(const uhdr_hip_image_t* in_img, int left, int right, int top, int bottom, uhdr_hip_image_t* out_img,
                  int mem_space, void* stream);
/* mirror_dir: 0 = ULTRAHDR_MIRROR_VERTICAL, 1 = ULTRAHDR_MIRROR_HORIZONTAL */
int uhdr_hip_mirror(const uhdr_hip_image_t* in_img, int mirror_dir, uhdr_hip_image_t* out_img, int mem_space, void* stream);
int uhdr_hip_rotate(const uhdr_hip_image_t* in_img, int clockwise_degree, uhdr_hip_image_t* out_img, int mem_space,
                    void* stream);
int uhdr_hip_resize(const uhdr_hip_image_t* in_img, int out_width, int out_height, uhdr_hip_image_t* out_img,
                    int mem_space, void* stream);

/* addEffects (lib/src/editorhelper.cpp:362-446; the way ultrahdr.cpp applies a configuration's effects to the SDR image and to
 * the gain map, :886-1429): the effects in order, every intermediate image tightly packed in device memory, the last one
 * copied to out->data (caller-allocated: the largest intermediate extent must fit) with out's fields set as the reference
 * leaves them (chroma_data = data + luma_stride * height for YUV420).  n == 0 copies width*height(*3/2) bytes and the
 * descriptor.  Where the reference is undefined this call reports instead: the status of a failing effect (the reference
 * ignores it and copies uninitialised fields), and ERROR_UNSUPPORTED_FEATURE for a mirror / rotate-180 of an image whose
 * strides exceed its width (the reference overruns its temporary buffer). */
typedef struct uhdr_hip_effect {
  int32_t type;          /* 0 crop, 1 mirror, 2 rotate, 3 resize */
  int32_t a, b, c, d;    /* crop: left, right, top, bottom; mirror: direction; rotate: clockwise degrees; resize: width, height */
} uhdr_hip_effect_t;
int uhdr_hip_add_effects(const uhdr_hip_image_t* in_img, const uhdr_hip_effect_t* effects, int n, uhdr_hip_image_t* out_img,
                         int mem_space, void* stream);

/* uhdr_hip_add_effects for n images in DEVICE memory, one chain shared by all of them (no reference counterpart; it is what
 * UltraHdr::convert does to the SDR image and to the gain map of every file, ultrahdr.cpp:933-1045).  Enqueued on `stream`; the
 * descriptor arrays are HOST memory and consumed before the call returns.  Sizes, strides and formats (YUV420 or MONOCHROME) may
 * differ per image.  All four effects are index maps, so the chain is composed on the host into one map per output plane, source
 * offset = A[row] + B[column], and a round of up to 64 images costs one upload of those tables and ONE launch whatever n_effects
 * is: the input is read once and the result written once.  The few chains whose map is not of that form (a crop that cuts the
 * stacked U|V planes at different columns after a quarter turn) run step by step inside the same call; the bytes are the same.
 * Per image, out[i][0 .. packed(w', h')) holds exactly what uhdr_hip_add_effects leaves there for the same image and chain
 * (packed = w'*h' for MONOCHROME, w'*h'*3/2 for YUV420) and out_imgs[i] is that call's descriptor (data = out[i], YUV420:
 * chroma_data = data + luma_stride * height).  Differences from the single call:
 *  - bytes of out[i] beyond packed(w', h') are NOT touched (the single call leaves the tails of larger intermediates there), so
 *    out_capacity[i] >= packed(w', h') suffices;
 *  - ERROR_UNSUPPORTED_FEATURE for a YUV420 image whose input or any intermediate or final image has an odd width or height: the
 *    reference reads chroma rows it never wrote there;
 *  - ERROR_INSUFFICIENT_RESOURCE with out_imgs[i] filled when out_capacity[i] < packed(w', h'); out[i] == NULL with capacity 0 is
 *    a size probe; out[i] == NULL with a capacity is BAD_PTR.
 * Inputs and outputs must not overlap.  status (optional) receives every image's status, the return value is the first that is not
 * NO_ERROR; a failing image does not disturb the others, and a batch whose every image stops at a check does not touch the device.
 * Call-level errors (status untouched): BAD_PTR for n < 0, n_effects < 0, NULL effects with n_effects > 0, or a NULL in_imgs / out /
 * out_capacity / out_imgs where n > 0. */
int uhdr_hip_add_effects_batch(int n, const uhdr_hip_image_t* in_imgs, const uhdr_hip_effect_t* effects, int n_effects,
                               void* const* out, const size_t* out_capacity, uhdr_hip_image_t* out_imgs, int* status, void* stream);

/* Host-only diagnostic of the composition above (needs no GPU): the image is width x height with chroma right behind luma
 * (chroma_data == NULL semantics; strides of 0 mean tight).  Fills the final descriptor (data NULL), *fused = 1 when the chain is
 * one A[row] + B[column] map per plane and 0 when uhdr_hip_add_effects_batch would run it step by step, *count = packed(w', h').
 * When fused and capacity >= *count, offsets[k] is the byte offset into the input allocation of output byte k, expanded from the
 * very tables the kernel would get.  Statuses as above. */
int uhdr_hip_effect_chain_map(size_t width, size_t height, size_t luma_stride, size_t chroma_stride, int pixel_format,
                              const uhdr_hip_effect_t* effects, int n_effects, uhdr_hip_image_t* out_desc, int* fused,
                              uint32_t* offsets, size_t capacity, size_t* count);

/* Host-only diagnostic of the same composition (needs no GPU): which route of the chain kernel each output plane takes.  Inputs
 * and statuses as uhdr_hip_effect_chain_map, and *fused is that call's.  *count = number of output planes the one launch would
 * serve (fused chain with effects: 1 for MONOCHROME; for YUV420 luma first, then the chroma planes, of which crop and resize
 * leave one stacked U|V plane; 0 when not fused and for n_effects == 0, which is a plain copy).  classes (may be NULL) receives
 * min(capacity, *count) codes: 0 byte gather, 1 unit-step ascending columns (aligned 16-byte copies), 2 unit-step descending
 * columns (16-byte pieces reversed), 3 monotone columns gathered from an LDS copy of the row stretch, 4 64 x 64 LDS tile. */
int uhdr_hip_effect_chain_classes(size_t width, size_t height, size_t luma_stride, size_t chroma_stride, int pixel_format,
                                  const uhdr_hip_effect_t* effects, int n_effects, int* fused, int* classes, size_t capacity,
                                  size_t* count);

/* ---- JPEG compression of the path's outputs (encode side) -------------------------------
 * JpegEncoderHelper::compressImage (lib/src/jpegencoderhelper.cpp:39-283; lib/include/ultrahdr/jpegencoderhelper.h:43-60):
 * baseline JPEG of a YUV420 image (image->data = Y, image->chroma_data = U, V at chroma_stride * height / 2) or, when
 * image->pixelFormat == UHDR_HIP_PIX_FMT_MONOCHROME, of the single plane image->data -- the bytes libjpeg writes in
 * raw-data mode with default tables, jpeg_set_quality(quality, TRUE) and the ISLOW DCT, including the reference's padding
 * rules (rows past the height are zero; columns past the width are zero when the stride is smaller than the 16-aligned
 * width, the caller's bytes otherwise).  icc (HOST memory, may be NULL) becomes an APP2 segment after the JFIF header.
 * FDCT, quantisation, Huffman coding and byte stuffing all run on the device.  out (capacity out_capacity) lives in the
 * memory space given by mem_space like the image planes; *out_size (HOST) receives the JPEG size.  The call waits for
 * the stream.  Returns ERROR_INSUFFICIENT_RESOURCE with *out_size set when out_capacity is too small. */
int uhdr_hip_jpeg_encode(const uhdr_hip_image_t* image, int quality, const void* icc, size_t icc_size, void* out,
                         size_t out_capacity, size_t* out_size, int mem_space, void* stream);
/* uhdr_hip_jpeg_encode for n images in one call (no reference counterpart).  Arrays are indexed by file; out[i] (capacity
 * out_capacity[i]) receives file i, out_size[i] (HOST) its size.  Every file's status, size and bytes are those of the single call
 * with the same arguments: its check order (BAD_PTR for NULL data, NULL chroma on 4:2:0 or out[i] == NULL with a capacity;
 * RESOLUTION_MISMATCH), its quality clamping, ERROR_INSUFFICIENT_RESOURCE with the exact size (out[i] == NULL with capacity 0
 * is a size probe).  status (optional) receives them, the return value is the first one that is not NO_ERROR; a file that fails its
 * checks is not processed and does not disturb the others.  YUV420 and MONOCHROME images, sizes, strides, qualities and ICC
 * profiles may differ per file.  icc == NULL: no file has a profile (icc[i] / icc_size[i] otherwise, HOST memory).  Call-level
 * errors, before any file is looked at: BAD_PTR for n < 0, a NULL images / quality / out / out_capacity / out_size where n > 0, or
 * icc != NULL with icc_size == NULL.  mem_space: UHDR_HIP_MEM_HOST or UHDR_HIP_MEM_DEVICE for planes and outputs alike, or
 * UHDR_HIP_MEM_DEVICE_TO_HOST / UHDR_HIP_MEM_HOST_TO_DEVICE; host planes are staged to the device first, device outputs are
 * written in place, host outputs arrive through page-locked staging.  The files go through in rounds: one launch per encoder step
 * for every image of a round and one synchronisation.  A round holds at most 128 images and at most 2 GiB of device workspace
 * and page-locked staging (a larger image gets a round of its own).  The call waits for the stream; a batch whose every file fails
 * its checks does not touch the device. */
int uhdr_hip_jpeg_encode_batch(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                               void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream);

/* n UHDR_HIP_PIX_FMT_RGBA8888 images -> the baseline 4:4:4 files libjpeg writes for in_color_space = JCS_RGB with all sampling
 * factors 1: jpeg_set_quality(quality, TRUE), JDCT_ISLOW, default Huffman tables, jccolor.c's fixed-point RGB -> YCbCr, an MCU of
 * one block each of Y, Cb, Cr, partial blocks padded by repeating the last column, then the last row.  Byte for byte what
 * libjpeg-turbo writes (Pillow: quality=q, subsampling=0).  Alpha is ignored.  The conventions of uhdr_hip_jpeg_encode_batch (memory
 * spaces, size probe with ERROR_INSUFFICIENT_RESOURCE and the exact size, per-file statuses), no ICC.  Any size from 1 x 1 to
 * 65500 x 65500, odd ones included.  Call-level: BAD_PTR for n < 0 or a NULL array where n > 0, INVALID_QUALITY_FACTOR for a
 * quality outside 0..100.  Per file: BAD_PTR (data NULL or, in device memory, not 4-byte aligned), UNSUPPORTED_FEATURE (another
 * pixelFormat), RESOLUTION_MISMATCH (size out of range, or a luma_stride below the width). */
int uhdr_hip_jpeg_encode_rgb_batch(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                   size_t* out_size, int* status, int mem_space, void* stream);
/* Diagnostics, host only (no GPU): the quantised coefficients of a progressive (SOF2) file after all of its scans -- what the
 * host-side entropy decoder hands to the device: blocks in MCU order (4:2:0: Y00 Y01 Y10 Y11 Cb Cr), zigzag order inside a block.
 * *blocks receives the block count (also when coef is NULL / too small: INSUFFICIENT_RESOURCE).  Baseline files, whose entropy
 * decoding runs on the device: UNSUPPORTED_FEATURE. */
int uhdr_hip_jpeg_progressive_coefficients(const void* jpeg, size_t jpeg_size, int16_t* coef, size_t capacity_blocks, size_t* blocks,
                                           int* width, int* height, int* gray);

/* JpegDecoderHelper::decompressImage(image, length, DECODE_TO_YCBCR) (lib/src/jpegdecoderhelper.cpp:188-516;
 * lib/include/ultrahdr/jpegdecoderhelper.h:54-56): a baseline 4:2:0 YCbCr or grayscale JPEG (HOST memory) -> the bytes
 * libjpeg returns with raw_data_out and JDCT_ISLOW, laid out as the reference's result buffer: width x height luma, then
 * (4:2:0) the (width/2) x (height/2) Cb and Cr planes at width*height and width*height + width*height/4; for an odd width or
 * height the bytes between and behind the planes are zero, as in the reference's zeroed buffer (:291).  out lives in
 * the memory space given by mem_space.  *desc is filled (data = out, chroma_data, strides, pixelFormat YUV420 or
 * MONOCHROME) when the header is readable, also on ERROR_INSUFFICIENT_RESOURCE (out_capacity too small: width*height*3/2
 * resp. width*height bytes are needed).  Huffman decoding (self-synchronising parallel decoder), dequantisation and IDCT
 * run on the device; restart intervals (DRI / RSTn) are read.  Progressive files (SOF2) are read too: their scans are entropy-decoded
 * on the host, dequantisation and IDCT run on the device (complete files; the planes are libjpeg's).  ERROR_UNSUPPORTED_FEATURE:
 * arithmetic-coded / lossless files (libjpeg reads some of them, this decoder does not); UNKNOWN_ERROR: malformed file, or a sampling other than 4:2:0 / single plane, where the reference's call
 * returns false as well (:283-289) -- and a host allocation that failed while parsing (a progressive file's coefficient array).
 * ERROR_INSUFFICIENT_RESOURCE with out == NULL is therefore always the size probe's answer: the header parsed and *desc holds the
 * size; on every status returned before that point *desc is zeroed.  The call waits for the stream. */
int uhdr_hip_jpeg_decode(const void* jpeg, size_t jpeg_size, void* out, size_t out_capacity, uhdr_hip_image_t* desc,
                         int mem_space, void* stream);

/* JpegDecoderHelper::decompressImage(..., DECODE_TO_RGBA) (lib/src/jpegdecoderhelper.cpp:251-281): a YCbCr 4:2:0 baseline JPEG ->
 * width*height RGBA8888 pixels (alpha 0xFF) with libjpeg-turbo's arithmetic (fancy upsampling, fixed-point colour conversion; see
 * uhdr_hip_jpegr_decode's UHDR_HIP_OUTPUT_SDR).  Same calling convention and status values as uhdr_hip_jpeg_decode; a single-plane
 * JPEG is UNKNOWN_ERROR (the reference's call returns false). */
int uhdr_hip_jpeg_decode_rgba(const void* jpeg, size_t jpeg_size, void* out, size_t out_capacity, uhdr_hip_image_t* desc, int mem_space,
                              void* stream);

/* uhdr_hip_jpeg_decode (decode_to = UHDR_HIP_DECODE_TO_YCBCR) or uhdr_hip_jpeg_decode_rgba (UHDR_HIP_DECODE_TO_RGBA) for n files
 * in one call (no reference counterpart; the values are those of the reference's decode_mode_t, jpegdecoderhelper.h:45-49).
 * Arrays are indexed by file; jpeg[i] (HOST memory) is file i, out[i] (memory space mem_space, capacity out_capacity[i]) receives
 * its pixels, descs[i] its descriptor.  Every file's status, bytes and descriptor are those of the single call with the same
 * arguments, size probes and early failures included; status (optional) receives them, the return value is the first one that is
 * not NO_ERROR; a file that fails does not disturb the others.  out or out_capacity may be NULL: every file is a size probe.
 * Call-level errors: BAD_PTR for n < 0 or a NULL jpeg / jpeg_size / descs where n > 0; ERROR_UNSUPPORTED_FEATURE for any other
 * decode_to.  The headers are parsed by up to 8 host threads; baseline, progressive, restart-interval and grayscale files of a round
 * share every decoder launch, so their latency-bound synchronisation rounds run side by side, and (RGBA) one conversion launch.  A
 * round holds at most 64 files and at most 2 GiB of device workspace (a larger file gets a round of its own).  The call waits for
 * the stream; a batch whose every file stops at its checks or its size probe does not touch the device. */
#define UHDR_HIP_DECODE_TO_RGBA 1
#define UHDR_HIP_DECODE_TO_YCBCR 2
int uhdr_hip_jpeg_decode_batch(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out,
                               const size_t* out_capacity, uhdr_hip_image_t* descs, int* status, int mem_space, void* stream);

/* Opt-in decode of samplings the reference refuses.  The *_ex calls are the calls above plus `flags`; with flags == 0 every status,
 * byte and descriptor is that of the call without the suffix, and a bit this header does not define is ERROR_UNSUPPORTED_FEATURE at
 * call level.  UHDR_HIP_DECODE_ANY_SAMPLING: a three-component YCbCr file (baseline, restart intervals or progressive) is also read
 * when its luma sampling is 1x1 (4:4:4), 2x1 (4:2:2) or 1x2 (4:4:0) and both chroma components are 1x1 -- what editors write at high
 * quality, many cameras, and a lossless rotation of a 4:2:2 file.  Any other sampling (4:1:1, chroma factors above 1) stays
 * UNKNOWN_ERROR (JPEG/R: ERROR_DECODE_ERROR).  The planes are byte-identical to libjpeg's raw_data_out, packed: width x height luma,
 * then Cb, then Cr of the chroma extent given at UHDR_HIP_PIX_FMT_YUV444 / 422 / 440 with chroma_stride = chroma width, i.e.
 * width * height + 2 * chroma_width * chroma_height bytes; descs[i].pixelFormat names the layout.  Odd widths and heights are
 * read for these three samplings (4:2:0 keeps its even-size rule).  UHDR_HIP_DECODE_TO_RGBA is byte-identical to libjpeg-turbo's
 * decode: no upsampling (4:4:4), h2v1 (4:2:2) or h1v2 (4:4:0) "fancy" upsampling, then the colour conversion of the 4:2:0 path.
 * Size probes work as in the calls without flags.  The decoder's steps are the same kernels with the MCU shape per image, so files
 * of every sampling share a batch's launches.  Measured on one MI355X (profiles/r06_jpeg_sampling.txt): a 4K quality-95 file decodes in
 * 382 us as 4:4:4 and 428 us as 4:2:2, beside 682 us as 4:2:0; against the commit before this interface a single 4:2:0 decode and a
 * 16-file 4:2:0 batch cost the same (within 0.5 %, inside that commit's own run-to-run spread, four sessions). */
#define UHDR_HIP_DECODE_ANY_SAMPLING 1
int uhdr_hip_jpeg_decode_batch_ex(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out,
                                  const size_t* out_capacity, uhdr_hip_image_t* descs, int* status, int mem_space, void* stream,
                                  int flags);
/* uhdr_hip_jpeg_decode (decode_to = UHDR_HIP_DECODE_TO_YCBCR) or uhdr_hip_jpeg_decode_rgba (UHDR_HIP_DECODE_TO_RGBA) with flags */
int uhdr_hip_jpeg_decode_ex(const void* jpeg, size_t jpeg_size, int decode_to, void* out, size_t out_capacity, uhdr_hip_image_t* desc,
                            int mem_space, void* stream, int flags);

/* Scaled decode: libjpeg's scale_num / scale_denom = 1 / scale_denom.  The *_scaled calls are the *_ex calls plus `scale_denom`, one of
 * 1, 2, 4, 8 (any other value: ERROR_UNSUPPORTED_FEATURE at call level); with scale_denom == 1 every status, byte and descriptor is
 * the *_ex call's.  The image comes out ceil(width / scale_denom) x ceil(height / scale_denom), computed by libjpeg's reduced inverse
 * DCTs (jidctred.c's 4x4 and 2x2, the 1x1 of the DC value) on the device, byte-identical to libjpeg-turbo's C arithmetic
 * (JSIMD_FORCENONE; its SIMD routines differ on coefficients no encoder produces from 8-bit samples).  The size per component is
 * libjpeg-turbo's (jdmaster.c): 8 / scale_denom, doubled for the chroma of a 4:2:0 file, which is thereby scaled up in the IDCT
 * instead of being upsampled.  So a 4:2:0 file gives three planes of the same size, UHDR_HIP_PIX_FMT_YUV444 (and odd sizes are read:
 * 4:2:0's even-size rule has no layout to apply to); 4:4:4, 4:2:2, 4:4:0 and single-plane files keep their layout, with the chroma
 * extents of those formats applied to the scaled size.  Descriptors, size probes and capacities speak of the scaled image;
 * DECODE_TO_YCBCR packs the planes as the *_ex call does, DECODE_TO_RGBA is libjpeg-turbo's RGBA of them (colour conversion for
 * 4:4:4 results, fancy h2v1 / h1v2 upsampling for 4:2:2 / 4:4:0 -- replicated chroma at 1/8, where libjpeg has no fancy upsampling).  Statuses that depend on the file alone -- what `flags` admits,
 * the 8192 limit on the file's own size, malformed data -- are the full-size call's, in its order.  Everything in front of the IDCT
 * is the full-size decoder, so scaled and full-size files share a batch's launches.  Measured on one MI355X
 * (profiles/r19_jpeg_scaled.txt), a 4K quality-95 4:2:0 file at 1, 1/2, 1/4, 1/8: planes into device memory 716 / 706 / 706 / 698 us (the
 * entropy decode dominates), RGBA into host memory 1331 / 874 / 755 / 741 us; the full-size calls cost what they cost before. */
int uhdr_hip_jpeg_decode_batch_scaled(int n, const void* const* jpeg, const size_t* jpeg_size, int decode_to, void* const* out,
                                      const size_t* out_capacity, uhdr_hip_image_t* descs, int* status, int mem_space, void* stream,
                                      int flags, int scale_denom);
/* a batch of one file */
int uhdr_hip_jpeg_decode_scaled(const void* jpeg, size_t jpeg_size, int decode_to, void* out, size_t out_capacity, uhdr_hip_image_t* desc,
                                int mem_space, void* stream, int flags, int scale_denom);
/* Host only: what a scaled decode of a width x height file gives.  hs x vs: the luma sampling factors (1 or 2 each, chroma 1x1);
 * gray != 0: a single-plane file (hs, vs ignored).  *out_width, *out_height: the scaled extent; *pixel_format: the layout
 * (UHDR_HIP_PIX_FMT_MONOCHROME / YUV444 / YUV422 / YUV440; YUV420 only at scale_denom 1); idct_size[c]: the inverse DCT's size for
 * component c (0 for the chroma of a single-plane file).  Every output pointer is optional.  ERROR_UNSUPPORTED_FEATURE for another
 * scale_denom or sampling, ERROR_UNSUPPORTED_WIDTH_HEIGHT for a size below 1. */
int uhdr_hip_jpeg_scaled_geometry(int width, int height, int hs, int vs, int gray, int scale_denom, int* out_width, int* out_height,
                                  int* pixel_format, int idct_size[3]);

/* Host only, for tests that prove their route: the number of launches of the synchronisation kernel (k_jd_sync_multi<1>, four rounds
 * each) that the last device decode of the calling host thread enqueued up to the look at the flags that read "no change" -- a
 * multiple of the launches between two looks, not the number the file needed.  A call of several decode rounds, or a JPEG/R decode
 * (two JPEGs in one batch), reports its last batch; a call that did not reach the device leaves the values.  *ring_looks (optional):
 * how often the host read the flags; *first_launches (optional): the launches in front of the first look, what a file reports that
 * needs no more (a constant of the build). */
int uhdr_hip_jpeg_decode_last_sync_launches(int* ring_looks, int* first_launches);

/* JpegR::decodeJPEGR (lib/src/jpegr.cpp:655-822) for the HDR output formats: a JPEG/R file (HOST memory: primary JPEG + gain
 * map JPEG, the gain map's APP1 carrying the hdrgm:* XMP attributes) -> the HDR rendition applyGainMap produces.  Container
 * scan (extractPrimaryImageAndGainMap, :823-876), XMP metadata (getMetadataFromXMP, jpegrutils.cpp:436-545) and the ICC gamut
 * of the primary image (IccHelper::readIccColorGamut, icc.cpp:615-685) are host bookkeeping; both JPEGs are decompressed and
 * combined on the device.  dest_data (memory space mem_space) receives width*height*{8|4|6} bytes; *dest gets width, height
 * and colorGamut; *metadata (optional) the parsed metadata.  Status values are the reference's: BAD_PTR,
 * INVALID_DISPLAY_BOOST (max_display_boost < 1), INVALID_OUTPUT_FORMAT, NO_IMAGES_FOUND, GAIN_MAP_IMAGE_NOT_FOUND, DECODE_ERROR,
 * METADATA_ERROR, then applyGainMap's own; plus ERROR_INSUFFICIENT_RESOURCE when dest_capacity is too small (*dest is filled)
 * and ERROR_UNSUPPORTED_FEATURE for arithmetic-coded JPEGs (progressive ones are read).  UHDR_HIP_OUTPUT_SDR (:768-786) returns the primary image alone as
 * RGBA8888 (4 bytes per pixel, alpha 0xFF) with the arithmetic libjpeg-turbo applies for DECODE_TO_RGBA (fancy 4:2:0 upsampling and
 * its fixed-point YCbCr -> RGB tables; jpegdecoderhelper.cpp:251-281); the gain map is then not decompressed and its XMP packet is
 * only read when `metadata` is not NULL, as in the reference. */
#define UHDR_HIP_ERROR_INVALID_DISPLAY_BOOST (-10008)
#define UHDR_HIP_ERROR_INVALID_OUTPUT_FORMAT (-10009)
#define UHDR_HIP_ERROR_DECODE_ERROR (-20002)
#define UHDR_HIP_ERROR_GAIN_MAP_IMAGE_NOT_FOUND (-20003)
#define UHDR_HIP_ERROR_METADATA_ERROR (-20005)
#define UHDR_HIP_ERROR_NO_IMAGES_FOUND (-20006)
int uhdr_hip_jpegr_decode(const void* jpegr, size_t jpegr_size, int output_format, float max_display_boost, void* dest_data,
                          size_t dest_capacity, uhdr_hip_image_t* dest, uhdr_hip_metadata_t* metadata, int apply_mode,
                          int mem_space, void* stream);

/* The same for n files in one call (no reference counterpart: the reference decodes one file per call).  A JPEG decode on the
 * device is latency-bound, so the 2 n JPEGs of the call share every kernel launch (one grid row per image) and their
 * synchronisation rounds run side by side: 16 4K files take 4.5x the time of one.  Arrays are indexed by file; dest_data[i] (memory space mem_space) needs dest_capacity[i] bytes; status (optional)
 * receives each file's status, the return value is the first one that is not NO_ERROR; a file that fails does not disturb the
 * others.  dest_data[i] == NULL asks for file i's size only (ERROR_INSUFFICIENT_RESOURCE, dests[i] filled). */
int uhdr_hip_jpegr_decode_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests,
                                uhdr_hip_metadata_t* metadata, int* status, int apply_mode, int mem_space, void* stream);

/* uhdr_hip_jpegr_decode[_batch] with flags (see UHDR_HIP_DECODE_ANY_SAMPLING; flags == 0: the calls above).  With the flag the
 * primary image may be 4:4:4, 4:2:2 or 4:4:0: UHDR_HIP_OUTPUT_SDR is libjpeg-turbo's RGBA of it, the HDR outputs are applyGainMap
 * over its planes with every pixel reading the chroma sample libjpeg's downsampled grid gives it (the rule of the reference's
 * getYuv420Pixel, no interpolation), through the general per-pixel kernels in every apply_mode (the scale-4 fast kernels are
 * 4:2:0's).  A gain-map JPEG with chroma of any accepted sampling contributes its luma (uhdr_hip_jpegr_decode_rgbmap_batch applies
 * such a map per channel). */
int uhdr_hip_jpegr_decode_ex(const void* jpegr, size_t jpegr_size, int output_format, float max_display_boost, void* dest_data,
                             size_t dest_capacity, uhdr_hip_image_t* dest, uhdr_hip_metadata_t* metadata, int apply_mode,
                             int mem_space, void* stream, int flags);
int uhdr_hip_jpegr_decode_batch_ex(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                   void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests,
                                   uhdr_hip_metadata_t* metadata, int* status, int apply_mode, int mem_space, void* stream, int flags);

/* uhdr_hip_jpegr_decode_batch_ex for files with per-channel gain maps: the same signature, flags included
 * (UHDR_HIP_DECODE_ANY_SAMPLING keeps its meaning for the primary image).  A file whose gain-map JPEG has THREE components -- 4:4:4,
 * 4:2:2, 4:4:0 or 4:2:0, whatever the flag -- has that JPEG converted to RGBA with libjpeg-turbo's arithmetic
 * (UHDR_HIP_DECODE_TO_RGBA; an odd-sized 4:2:0 map: ERROR_UNSUPPORTED_FEATURE, as there) and applied per channel
 * (uhdr_hip_apply_gainmap_rgb_batch, so UHDR_HIP_APPLY_FAST or _EXACT).  A file whose gain-map JPEG has one component takes the
 * path of uhdr_hip_jpegr_decode_batch_ex, with identical bytes; UHDR_HIP_OUTPUT_SDR is unchanged. */
int uhdr_hip_jpegr_decode_rgbmap_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                       void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests,
                                       uhdr_hip_metadata_t* metadata, int* status, int apply_mode, int mem_space, void* stream, int flags);

/* JpegR::appendGainMap (lib/src/jpegr.cpp:951-1130): primary JPEG + gain-map JPEG + metadata -> JPEG/R container (XMP packets of
 * jpegrutils.cpp:547-611, MPF segment of multipictureformat.cpp:30-92).  exif / icc: payloads of an APP1 / APP2 segment to add, or
 * NULL; an EXIF segment found inside primary_jpeg moves in front of the XMP segment (and ERROR_MULTIPLE_EXIFS_RECEIVED if exif is
 * given as well), with JpegDecoderHelper::extractEXIF's position arithmetic (jpegdecoderhelper.cpp:146-188).  Pure host code, no
 * device needed.  *out_size receives the size (also when out_capacity is too small: ERROR_INSUFFICIENT_RESOURCE). */
#define UHDR_HIP_ERROR_MULTIPLE_EXIFS_RECEIVED (-20007)
int uhdr_hip_jpegr_append_gainmap(const void* primary_jpeg, size_t primary_size, const void* gainmap_jpeg, size_t gainmap_size,
                                  const void* exif, size_t exif_size, const void* icc, size_t icc_size,
                                  const uhdr_hip_metadata_t* metadata, void* out, size_t out_capacity, size_t* out_size);
/* IccHelper::writeIccProfile (lib/src/icc.cpp:410-600) for transfer_function == UHDR_HIP_TF_SRGB (the profile of the SDR base
 * image): "ICC_PROFILE\0" + chunk bytes + profile, as it goes into the primary JPEG's APP2.  Host code. */
int uhdr_hip_icc_profile(int transfer_function, int color_gamut, void* out, size_t out_capacity, size_t* out_size);

/* JpegR::encodeJPEGR, every overload (lib/include/ultrahdr/jpegr.h:81-185,263-265; lib/src/jpegr.cpp:186-631).  toneMap,
 * generateGainMap, the BT.601 re-encode of the SDR image (16-aligned zero-padded copy + convertYuv unless it is P3 already), the
 * JPEG compressions (gain map at quality 85, SDR image at `quality` with the ICC profile) and API-3's JPEG decode run on the
 * device; the container is assembled on the host.  Raw images live in mem_space; compressed inputs, exif and `out` are HOST
 * memory.  exif: payload of the APP1 segment ("Exif\0\0"...), or NULL.  sdr_jpeg_gamut: the colorGamut field of the reference's
 * compressed struct (used when the JPEG carries no ICC profile).  Status values and their order are the reference's
 * (areInputArgumentsValid :75-183, then each overload's own checks); ERROR_INSUFFICIENT_RESOURCE (with *out_size set) when
 * out_capacity is too small, where the reference's Write() fails the same way (:46-61).
 *   api0: P010                       -> toneMap, then as api1                          (:186-247)
 *   api1: P010 + YUV420                                                                (:249-381)
 *   api2: P010 + YUV420 + SDR JPEG   -> gain map from the planes, container around the given JPEG   (:384-437)
 *   api3: P010 + SDR JPEG            -> JPEG decoded (BT.601), gain map, container     (:439-500)
 *   api4: SDR JPEG + gain-map JPEG + metadata -> container; host only                  (:502-560)
 *   apix: YUV420 + gain-map plane + metadata  -> both compressed, container            (:562-631) */
#define UHDR_HIP_ERROR_UNSUPPORTED_WIDTH_HEIGHT (-10002)
#define UHDR_HIP_ERROR_INVALID_STRIDE (-10004)
#define UHDR_HIP_ERROR_INVALID_QUALITY_FACTOR (-10007)
#define UHDR_HIP_ERROR_ENCODE_ERROR (-20001)
int uhdr_hip_jpegr_encode_api0(const uhdr_hip_image_t* p010_image, int hdr_tf, int quality, const void* exif, size_t exif_size,
                               void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_api1(const uhdr_hip_image_t* p010_image, const uhdr_hip_image_t* yuv420_image, int hdr_tf, int quality,
                               const void* exif, size_t exif_size, void* out, size_t out_capacity, size_t* out_size, int mem_space,
                               void* stream);
/* encodeJPEGR API-1 (yuv420_images != NULL) or API-0 (yuv420_images == NULL) for n pairs in one call (no reference
 * counterpart).  Arrays are indexed by file; out[i] (HOST memory) receives file i, out_size[i] its size.  Every file's status,
 * size and bytes are those of the single call with the same arguments (ERROR_INSUFFICIENT_RESOURCE with the exact size included);
 * status (optional) receives them, the return value is the first one that is not NO_ERROR.  hdr_tf and quality are shared; gamuts
 * and sizes may differ per file.  exif == NULL: no file has EXIF (exif[i] / exif_size[i] otherwise, host memory).  Call-level
 * errors, before any file is looked at: n < 0, a NULL array where n > 0, a quality outside 0..100.  A file that fails its checks
 * is not processed and does not disturb the others.  Planes in mem_space; host planes are staged to the device first.  The files'
 * toneMap / generate / convertYuv and all 2 n JPEG compressions share their kernel launches, one synchronisation per round of up
 * to 64 files. */
int uhdr_hip_jpegr_encode_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf,
                                int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream);
/* uhdr_hip_jpegr_encode_batch with a per-channel gain map: the same signature and conventions (API-1, or API-0 when
 * yuv420_images == NULL); the primary image and the container are exactly that call's, the gain map is
 * uhdr_hip_generate_gainmap_rgb_batch's, compressed at quality 85 as uhdr_hip_jpeg_encode_rgb_batch compresses it.  XMP, MPF and ICC
 * are untouched and the metadata is the same single range.  Read such files with uhdr_hip_jpegr_decode_rgbmap_batch. */
int uhdr_hip_jpegr_encode_rgbmap_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf,
                                       int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                       const size_t* out_capacity, size_t* out_size, int* status, int mem_space, void* stream);
/* encodeJPEGR API-2 (yuv420_images != NULL) or API-3 (yuv420_images == NULL) for n files in one call, and API-x for n files in one
 * call (no reference counterparts).  The conventions of uhdr_hip_jpegr_encode_batch: arrays indexed by file, hdr_tf / quality shared,
 * everything else per file; planes in mem_space, compressed inputs, exif and out[i] HOST memory; every file's status, size and bytes
 * those of uhdr_hip_jpegr_encode_api2 / _api3 / _apix with the same arguments (ERROR_INSUFFICIENT_RESOURCE with the exact size
 * included); status optional, the return value the first status that is not NO_ERROR; a file that fails does not disturb the others.
 * Call-level errors, before any file is looked at (status untouched): BAD_PTR for n < 0 or a NULL required array where n > 0
 * (API-2/3: p010_images, sdr_jpeg, sdr_jpeg_size, sdr_jpeg_gamut, out, out_capacity, out_size; API-x: yuv420_images,
 * gainmap_images, metadata, out, out_capacity, out_size; exif != NULL with exif_size == NULL), then API-x's
 * INVALID_QUALITY_FACTOR.  Every per-file check that needs no device runs first, also those the single calls make after their
 * device work (API-2's checks of the SDR JPEG, API-x's after its NULL pointers); only API-3's gamut and size checks follow its
 * decode, as in the single call.  A batch whose every file stops at such a check does not touch the device.  Rounds of up to 64
 * files and 2 GiB of workspace and staging, sorted into runs of equal size and gamuts: API-3's JPEGs share one decoder launch
 * set, the generate launches are shared by equal files, every JPEG compression of a round goes through one launch set, one
 * synchronisation per round (plus the decoder's own), and the containers are assembled by up to 8 host threads. */
int uhdr_hip_jpegr_encode_sdr_jpeg_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images,
                                         const void* const* sdr_jpeg, const size_t* sdr_jpeg_size, const int* sdr_jpeg_gamut,
                                         int hdr_tf, void* const* out, const size_t* out_capacity, size_t* out_size,
                                         int* status, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_apix_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* gainmap_images,
                                     const uhdr_hip_metadata_t* metadata, int quality, const void* const* exif,
                                     const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                                     int* status, int mem_space, void* stream);
/* n JPEG/R files in, n edited JPEG/R files out (no reference counterpart; it is UltraHdr::convert's edit flow, ultrahdr.cpp:933-1045:
 * decode, addEffects on the SDR image and on the gain map, encodeJPEGR API-x).  Compressed data is HOST memory; the call waits for
 * the stream.  Per file: the container is split, the primary JPEG is decoded to YCbCr planes and the gain-map JPEG to one plane in
 * device memory by the batched decoder (all 2 n JPEGs of a round share its launches), the metadata is read from the gain map's XMP,
 * sdr_effects runs on the primary's planes and gainmap_effects on the map through uhdr_hip_add_effects_batch's machinery (all
 * planes of the round in one launch), and the round is encoded by uhdr_hip_jpegr_encode_apix_batch.  Nothing uncompressed crosses
 * PCIe.  out[i] receives what uhdr_hip_jpegr_encode_apix writes for the edited planes, the parsed metadata, `quality`, the primary's
 * EXIF payload (the range uhdr_hip_jpegr_info reports; none if it has none) and colorGamut = the gamut of the primary's ICC profile
 * when it has a readable one, otherwise sdr_gamut[i] (sdr_gamut == NULL: UNSPECIFIED for every file).  The reference passes one
 * chain to both images (ultrahdr.cpp:951-952); two are taken because the map is usually a quarter of the size, callers who want the
 * reference's behaviour pass the same array twice.  Orientation tags inside the EXIF payload are NOT rewritten.
 * Per-file status, in this order: BAD_PTR (jpegr[i] == NULL, or out[i] == NULL with a capacity); NO_IMAGES_FOUND or
 * GAIN_MAP_IMAGE_NOT_FOUND; DECODE_ERROR (either JPEG unreadable, or a single-plane primary); METADATA_ERROR; the SDR chain's status;
 * the gain-map chain's status (both as in uhdr_hip_add_effects_batch); API-x's own; ERROR_INSUFFICIENT_RESOURCE with the exact size
 * in out_size[i] (out[i] == NULL with capacity 0 is a size probe).  status is optional, the return value is the first status that is
 * not NO_ERROR, a failing file does not disturb the others.  Call-level errors (status untouched): BAD_PTR for n < 0, a NULL
 * jpegr / jpegr_size / out / out_capacity / out_size where n > 0, a negative effect count or a NULL chain with a positive one; then
 * INVALID_QUALITY_FACTOR.  A round holds at most 64 files and 2 GiB of workspace. */
int uhdr_hip_jpegr_edit_batch(int n, const void* const* jpegr, const size_t* jpegr_size, const uhdr_hip_effect_t* sdr_effects,
                              int n_sdr_effects, const uhdr_hip_effect_t* gainmap_effects, int n_gainmap_effects, const int* sdr_gamut,
                              int quality, void* const* out, const size_t* out_capacity, size_t* out_size, int* status, void* stream);
int uhdr_hip_jpegr_encode_api2(const uhdr_hip_image_t* p010_image, const uhdr_hip_image_t* yuv420_image, const void* sdr_jpeg,
                               size_t sdr_jpeg_size, int sdr_jpeg_gamut, int hdr_tf, void* out, size_t out_capacity,
                               size_t* out_size, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_api3(const uhdr_hip_image_t* p010_image, const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut,
                               int hdr_tf, void* out, size_t out_capacity, size_t* out_size, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_api4(const void* sdr_jpeg, size_t sdr_jpeg_size, int sdr_jpeg_gamut, const void* gainmap_jpeg,
                               size_t gainmap_jpeg_size, const uhdr_hip_metadata_t* metadata, void* out, size_t out_capacity,
                               size_t* out_size);
int uhdr_hip_jpegr_encode_apix(const uhdr_hip_image_t* yuv420_image, const uhdr_hip_image_t* gainmap_image,
                               const uhdr_hip_metadata_t* metadata, int quality, const void* exif, size_t exif_size, void* out,
                               size_t out_capacity, size_t* out_size, int mem_space, void* stream);

/* JpegR::getJPEGRInfo (lib/src/jpegr.cpp:633-653; parseJpegInfo :878-915): the two images of a JPEG/R file and what
 * JpegDecoderHelper::getCompressedImageParameters reports for each -- size and the first ICC / EXIF / XMP packets
 * (jpegdecoderhelper.cpp:221-249; the reference copies them into vectors, here they are [offset, size) ranges into the file, size 0
 * = absent; the XMP range is the reference's buffer minus its extra terminating zero).  gainmap may be NULL.  Host code.
 * NO_IMAGES_FOUND / GAIN_MAP_IMAGE_NOT_FOUND from the split, DECODE_ERROR for an unreadable header or one over 8192x8192. */
typedef struct uhdr_hip_jpeg_info {
  size_t offset, size;            /* the JPEG itself (imgData) */
  size_t width, height;
  size_t icc_offset, icc_size;    /* iccData: "ICC_PROFILE\0" + chunk bytes + profile */
  size_t exif_offset, exif_size;  /* exifData: "Exif\0\0" + TIFF */
  size_t xmp_offset, xmp_size;    /* xmpData: namespace + '\0' + packet */
} uhdr_hip_jpeg_info_t;
int uhdr_hip_jpegr_info(const void* jpegr, size_t jpegr_size, uhdr_hip_jpeg_info_t* primary, uhdr_hip_jpeg_info_t* gainmap);

/* getMetadataFromXMP (lib/src/jpegrutils.cpp:436-545) on the gain-map image of a JPEG/R file, as uhdr_dec_probe does after
 * getJPEGRInfo (lib/src/ultrahdr_api.cpp:1038-1108).  Host code.  METADATA_ERROR when the packet is missing or malformed. */
int uhdr_hip_jpegr_metadata(const void* jpegr, size_t jpegr_size, uhdr_hip_metadata_t* metadata);

/* ---- batches (device memory only, asynchronous on `stream`) ------------------------------ */
/* The reference processes one image per call; a batch is n independent calls with identical
 * (hdr_tf, sdr_is_601 | metadata, output_format, max_display_boost).  Images of equal size share
 * one kernel launch (grid.y = image).  Descriptor arrays live in HOST memory and are consumed
 * before the call returns; the data pointers inside them are DEVICE pointers. */

/* content_minmax (optional, DEVICE pointer to 2*n floats): per image i, [2i] = min and [2i+1] =
 * max over map pixels of the UNCLAMPED gain (gainmapmath.cpp:531-534 before the clamp).  This
 * statistic has no reference counterpart (the reference writes constants, ultrahdr.cpp:250-257);
 * the emitted metadata stays the reference's constants. */
int uhdr_hip_generate_gainmap_batch(int n, const uhdr_hip_image_t* yuv420_images,
                                    const uhdr_hip_image_t* p010_images, int hdr_tf,
                                    uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests,
                                    int sdr_is_601, float* content_minmax, void* stream);

int uhdr_hip_generate_gainmap_batch_ex(int n, const uhdr_hip_image_t* yuv420_images,
                                       const uhdr_hip_image_t* p010_images, int hdr_tf,
                                       uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests,
                                       int sdr_is_601, int generate_mode, float* content_minmax, void* stream);

int uhdr_hip_apply_gainmap_batch(int n, const uhdr_hip_image_t* yuv420_images,
                                 const uhdr_hip_image_t* gainmap_images,
                                 const uhdr_hip_metadata_t* metadata, int output_format,
                                 float max_display_boost, uhdr_hip_image_t* dests, int apply_mode,
                                 void* stream);

/* ---- per-channel (RGB) gain maps (the reference's one-plane maps carry one luminance ratio per map pixel; current libultrahdr also
 * writes three-channel maps, use_multi_channel_gainmap) ------------------------------------
 * Everything of generateGainMap up to the luminance is unchanged (sampling at scale 4, yuvToRgb, the inverse OETFs, the gamut
 * conversion into the SDR gamut).  With sdr_rgb and hdr_rgb those two linear colours, byte c of a map pixel is the reference's
 * encodeGain(sdr_rgb.c * 203.0f, hdr_rgb.c * hdr_white_nits, metadata), the products in f32: a channel <= 0 on the SDR side gives
 * gain 1, a negative HDR channel (out of gamut after the conversion) clamps to minContentBoost.  The metadata is the reference's
 * constants, identical to what uhdr_hip_generate_gainmap_batch returns.  The exact arithmetic throughout (no f32 pre-filter).
 * Device memory, asynchronous; conventions, checks and status order of uhdr_hip_generate_gainmap_batch.  dests[i].data needs
 * 4 * (width / 4) * (height / 4) bytes, 4-byte aligned (BAD_PTR otherwise); dests[i] comes back as UHDR_HIP_PIX_FMT_RGBA8888. */
int uhdr_hip_generate_gainmap_rgb_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images, int hdr_tf,
                                        uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601, void* stream);
/* applyGainMap with an RGBA8888 map: sampleMap's four taps and weights are the pixel's, applied to each channel of the taps, and
 * applyGain runs per channel -- channel c of the linear SDR colour times exp2(log2Min * (1 - gain_c) + log2Max * gain_c), the
 * display-boost form alike.  Every operation behind the gain is per channel, so channel c of the result is, bit for bit, channel c
 * of uhdr_hip_apply_gainmap_batch run with plane c of the map (UHDR_HIP_APPLY_EXACT; UHDR_HIP_APPLY_FAST: every 10-bit channel
 * within 1 code, every F16 channel within 1 half-precision ULP of it).  Conventions, checks and status order of
 * uhdr_hip_apply_gainmap_batch -- any integer scale factor, 4:2:0 / 4:4:4 / 4:2:2 / 4:4:0 primaries by pixelFormat --, plus
 * BAD_PTR for a map pointer that is not 4-byte aligned, INVALID_STRIDE for a luma_stride below the map's width, and
 * ERROR_UNSUPPORTED_FEATURE for UHDR_HIP_APPLY_LUT and UHDR_HIP_APPLY_EXACT_UNFILTERED.  The maps' pixelFormat is not read. */
int uhdr_hip_apply_gainmap_rgb_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* gainmap_images,
                                     const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                                     uhdr_hip_image_t* dests, int apply_mode, void* stream);

/* ---- gain maps with gamma, offsets and an HDR capacity range (no reference counterpart) ------
 * The reference's applyGainMap refuses every file whose metadata is not DEGENERATE -- gamma == 1, both offsets 0, hdrCapacityMin ==
 * minContentBoost and hdrCapacityMax == maxContentBoost -- and so do the calls above (ERROR_BAD_METADATA).  Files in the field use
 * all of these fields (current libultrahdr writes offsets of 1/64 by default).  The *_md calls implement the gain-map formula in
 * full.  Symbols: min, max = min / maxContentBoost; Hmin, Hmax = hdrCapacityMin / Max; os, oh = offsetSdr / offsetHdr; D =
 * max_display_boost.
 *
 * Validation, after the pointer checks, in this order: ERROR_BAD_METADATA for a version other than "1.0", a non-finite field,
 * max < min, min <= 0, Hmax < Hmin, Hmin <= 0, an offset < 0 or gamma <= 0; (apply and decode) ERROR_INVALID_DISPLAY_BOOST for
 * D < 1 or NaN; then the checks of the call whose conventions are named.
 *
 * Apply.  DEGENERATE metadata is forwarded to uhdr_hip_apply_gainmap_batch / uhdr_hip_apply_gainmap_rgb_batch: the bytes are those
 * calls' in every apply mode, including the reference's exponent scaling by displayBoost / maxContentBoost.  For every other
 * (GENERAL) metadata, per pixel and channel c (a one-plane map: one gain for the three channels):
 *     W     = clamp((log2 D - log2 Hmin) / (log2 Hmax - log2 Hmin), 0, 1);   Hmax == Hmin: W = D >= Hmax ? 1 : 0
 *     d     = min(D, Hmax)
 *     g     = sampleMap's interpolated value in [0, 1], as in every other apply call
 *     g'    = g^(1 / gamma)   (gamma == 1: g; 0 stays 0)
 *     out_c = max(0, (e_c + os) * 2^((log2 min * (1 - g') + log2 max * g') * W) - oh) / d
 * with e_c the linear SDR channel (p3YuvToRgb, srgbInvOetf); the OETF and the packing of output_format follow as in the other
 * calls (the 10-bit formats keep the reference's `& 0x3ff`: a value above 1.0 is not clamped).  The weight rule therefore DIFFERS
 * between degenerate and general metadata when D < max: degenerate metadata scales the exponent by D / max as the reference does,
 * general metadata by W, the gain-map specification's weight (log-domain).  The host forms W, log2 d and the exponent's two
 * constants in double; the device works in f32 with the hardware exp2 / log2 and the FAST transfer functions.  There is ONE
 * arithmetic for general metadata: UHDR_HIP_APPLY_FAST and UHDR_HIP_APPLY_EXACT both select it -- EXACT means "the bytes of the
 * reference's CPU path", and the reference refuses these files, so there is nothing to be exact against.  Against the formula
 * evaluated in double every 10-bit channel is within 1 code and every F16 channel within 1 half-precision ULP (FAST's bars).
 * UHDR_HIP_APPLY_LUT and UHDR_HIP_APPLY_EXACT_UNFILTERED return ERROR_UNSUPPORTED_FEATURE for general metadata. */
/* W and d = min(D, Hmax) by themselves, host code, as the apply calls form them (in double, returned as float).  BAD_PTR for NULL,
 * then the validation above. */
int uhdr_hip_gainmap_weight(const uhdr_hip_metadata_t* metadata, float max_display_boost, float* weight, float* display_boost);
/* Conventions of uhdr_hip_apply_gainmap_batch.  The maps' pixelFormat selects the form: MONOCHROME or UNSPECIFIED -- one plane, rows
 * of `width` bytes; RGBA8888 -- per channel, uhdr_hip_apply_gainmap_rgb_batch's layout rules (4-byte aligned, luma_stride in pixels,
 * 0 = width); any other value is ERROR_UNSUPPORTED_FEATURE.  All maps of a call have the same form (the first map's). */
int uhdr_hip_apply_gainmap_md_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* gainmap_images,
                                    const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                                    uhdr_hip_image_t* dests, int apply_mode, void* stream);
/* generateGainMap against the caller's metadata (metadata_in is read, not written).  Everything up to the two luminances -- in
 * nits, as encodeGain receives them -- is unchanged, on the exact path (no f32 pre-filter).  Then, in f32,
 *     a = y_sdr + os * 203.0f,  b = y_hdr + oh * 203.0f,  gain = a > 0 ? b / a : 1, clamped to [min, max]
 *     t = (log2(gain) - log2Min) / (log2Max - log2Min)      with the reference's promotions (gainmapmath.cpp:529-541)
 *     byte = (uint8_t)(t * 255.0f)                          gamma == 1
 *     byte = (uint8_t)(pow(t, (double)gamma) * 255.0)       otherwise, in double (t <= 0 gives 0)
 * truncated as the reference truncates.  With gamma == 1 and zero offsets this is encodeGain bit for bit.  rgb != 0: the same rule
 * per channel on sdr.c * 203.0f and hdr.c * hdr_white_nits, and the conventions (RGBA8888 dests, 4-byte aligned) of
 * uhdr_hip_generate_gainmap_rgb_batch; rgb == 0: those of uhdr_hip_generate_gainmap_batch.  hdrCapacityMin / Max are validated but
 * do not enter the map.  For gamma != 1 the device evaluates the power with its own f64 log2 / exp2: the value in front of the
 * truncation is within 2^-30 of the libm evaluation's.  Such maps go into files through uhdr_hip_jpegr_encode_apix_batch with the
 * same metadata: no further encode call is needed (an RGBA map: uhdr_hip_jpeg_encode_rgb_batch, then
 * uhdr_hip_jpegr_append_gainmap).  Content-adaptive ranges: pass the adaptive call's range as metadata_in. */
int uhdr_hip_generate_gainmap_md_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images, int hdr_tf,
                                       const uhdr_hip_metadata_t* metadata_in, uhdr_hip_image_t* dests, int sdr_is_601, int rgb,
                                       void* stream);
/* uhdr_hip_jpegr_decode_rgbmap_batch -- its signature, flags and per-file status rules, one- and three-component gain-map JPEGs --
 * for files with any valid metadata: a file whose metadata is degenerate takes that call's path (identical bytes), any other goes
 * through uhdr_hip_apply_gainmap_md_batch with the file's own metadata (per file: BAD_METADATA for invalid fields, UNSUPPORTED_FEATURE
 * for LUT / EXACT_UNFILTERED).  UHDR_HIP_OUTPUT_SDR is unchanged. */
int uhdr_hip_jpegr_decode_md_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                   void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests,
                                   uhdr_hip_metadata_t* metadata, int* status, int apply_mode, int mem_space, void* stream, int flags);
/* uhdr_hip_jpegr_decode_md_batch at 1 / scale_denom of every file's size (1, 2, 4, 8; any other value: ERROR_UNSUPPORTED_FEATURE at call
 * level; 1: that call exactly).  The primary image is decoded as uhdr_hip_jpeg_decode_batch_scaled decodes it; dests[i], the size probe
 * and dest_capacity speak of the scaled extent.  UHDR_HIP_OUTPUT_SDR is the scaled RGBA.  For the HDR formats the gain map follows
 * the primary image: with f the file's map scale factor (the file must pass the full-size checks: width and height multiples of the
 * map's, one ratio), f % scale_denom == 0 decodes the map at full size and applies it at factor f / scale_denom;
 * scale_denom % f == 0 decodes the map at 1 / (scale_denom / f) and applies it at factor 1; any other pair is
 * ERROR_UNSUPPORTED_MAP_SCALE_FACTOR for that file, answered from the two headers: behind the statuses of its container and its
 * metadata, in front of the size probe.  The
 * result is uhdr_hip_apply_gainmap_md_batch on the scaled planes and the (scaled) map, in every apply_mode that call accepts -- for a
 * 4:2:0 primary the YUV444 planes of the scaled decode, through the per-pixel kernels.  The primary image and the map of one file may
 * carry different denominators in the one decoder launch.  16 4K files to HDR_PQ, device memory: 3.25 ms at full size, 2.87 ms at 1/8
 * (profiles/r19_jpeg_scaled.txt). */
int uhdr_hip_jpegr_decode_scaled_batch(int n, const void* const* jpegr, const size_t* jpegr_size, int output_format, float max_display_boost,
                                       void* const* dest_data, const size_t* dest_capacity, uhdr_hip_image_t* dests,
                                       uhdr_hip_metadata_t* metadata, int* status, int apply_mode, int mem_space, void* stream, int flags,
                                       int scale_denom);

/* ---- packed RGBA inputs (no reference counterpart; current libultrahdr takes the same raw inputs) ------
 * Every encode-side call above takes a P010 HDR frame and planar 8-bit YUV 4:2:0.  The calls of this section take what the apply and
 * decode calls write and what a renderer or a compositor holds: an UHDR_HIP_PIX_FMT_RGBA8888 SDR image and an
 * UHDR_HIP_PIX_FMT_RGBA1010102 (hdr_tf HLG or PQ) or UHDR_HIP_PIX_FMT_RGBA_F16 (hdr_tf LINEAR) HDR image, layouts as at the
 * pixel-format constants.  No narrow-range quantisation and no chroma subsampling enter the map.
 *
 * uhdr_hip_generate_gainmap_packed_batch.  Device memory, asynchronous on `stream`.  The arithmetic, every step f32 unless said:
 *   pixel values   RGBA8888: (float)code * (1 / 255.0f) per channel; RGBA1010102: (float)code10 * (1 / 1023.0f); RGBA_F16: the exact
 *                  f32 of each half (subnormal halves included).
 *   sampling       the map is (width / 4) x (height / 4); a map pixel's sample is the reference's samplePixels (gainmapmath.cpp:
 *                  605-615) per channel over its 4 x 4 block, for both images: e = 0; for dy, for dx: e += pixel; e / 16.0f -- the
 *                  product and the running sum are separate roundings.  Columns and rows past 4 * (width / 4), 4 * (height / 4) are
 *                  not read.
 *   the rest       generateGainMap's (ultrahdr.cpp:317-334) without its two yuvToRgb steps and without their clamp: srgbInvOetf on
 *                  the SDR colour; hdrInvOetf(hdr_tf) on the HDR colour, then the conversion into the SDR image's gamut; the SDR
 *                  gamut's luminance of both, times 203.0f and times hdr_white_nits (PQ 10000, otherwise 1000); encodeGain.
 *   rgb != 0       the split of uhdr_hip_generate_gainmap_rgb_batch: encodeGain per channel on sdr.c * 203.0f and
 *                  hdr.c * hdr_white_nits, RGBA8888 dests (4-byte aligned), A = 0xFF.
 * The exact path throughout, as in the *_rgb_* and *_md_* calls.  metadata_in == NULL selects the reference's constants for hdr_tf
 * (what uhdr_hip_generate_gainmap_batch returns); otherwise the rule, the validation and the gamma handling are those of
 * uhdr_hip_generate_gainmap_md_batch.  metadata_out (optional) receives the metadata that was used.  A map pixel that reads a
 * non-finite half is unspecified; nothing outside the dests is written.  dests[i].data needs (width / 4) * (height / 4) bytes, four
 * times that with rgb != 0; dests[i] comes back described as in uhdr_hip_generate_gainmap_md_batch.  All HDR images of a call have
 * one format.  Checks, in this order:
 *   BAD_PTR              n < 0, or a NULL sdr_images / hdr_images / dests where n > 0
 *   UNSUPPORTED_FEATURE  (every image, before anything else of any image) an SDR pixelFormat other than RGBA8888; an HDR pixelFormat
 *                        other than RGBA1010102 / RGBA_F16; an HDR pixelFormat that differs from hdr_images[0]'s
 *   BAD_PTR              (every image) a NULL data or dests[i].data; SDR or RGBA1010102 data not 4-byte aligned, RGBA_F16 data not
 *                        8-byte aligned; with rgb != 0 a dest not 4-byte aligned
 *   BAD_METADATA         metadata_in != NULL: uhdr_hip_generate_gainmap_md_batch's validation
 *   then per image       INVALID_STRIDE (a luma_stride below the width, or above 2^32 - 1); RESOLUTION_MISMATCH; INVALID_COLORGAMUT
 *                        (UNSPECIFIED); INVALID_TRANS_FUNC (RGBA_F16 with anything but LINEAR, RGBA1010102 with anything but HLG /
 *                        PQ); INVALID_COLORGAMUT (any other value outside BT709 / P3 / BT2100)
 *   INVALID_TRANS_FUNC   n == 0 and hdr_tf none of LINEAR / HLG / PQ */
int uhdr_hip_generate_gainmap_packed_batch(int n, const uhdr_hip_image_t* sdr_images, const uhdr_hip_image_t* hdr_images, int hdr_tf,
                                           const uhdr_hip_metadata_t* metadata_in, uhdr_hip_metadata_t* metadata_out,
                                           uhdr_hip_image_t* dests, int rgb, void* stream);
/* n UHDR_HIP_PIX_FMT_RGBA8888 images -> the baseline 4:2:0 files libjpeg writes for in_color_space = JCS_RGB, luma sampling 2x2 and
 * chroma 1x1, jpeg_set_quality(quality, TRUE), JDCT_ISLOW and default Huffman tables: jccolor.c's fixed-point RGB -> YCbCr at full
 * resolution, then jcsample.c's h2v2_downsample, (a + b + c + d + bias) >> 2 with the bias alternating 1, 2 along a row.  Edges as
 * libjpeg makes them: the last column of the full-resolution rows is repeated out to the padded width and the last row to an even
 * count before the downsampling, the last downsampled row is repeated after it (luma: last column, then last row).  Byte for byte
 * what libjpeg-turbo writes (Pillow: quality=q, subsampling=2).  Alpha is ignored.  Signature and conventions of
 * uhdr_hip_jpeg_encode_batch -- memory spaces, ICC per file (an APP2 segment where uhdr_hip_jpeg_encode puts it), size probe with
 * ERROR_INSUFFICIENT_RESOURCE and the exact size, per-file statuses --; any size from 1 x 1 to 65500 x 65500, odd ones included.  One
 * conversion / downsample launch covers every image of a round (at most 64 images), the FDCT / Huffman / stuffing chain is
 * uhdr_hip_jpeg_encode_batch's.  Call-level: BAD_PTR for n < 0, a NULL array where n > 0 or icc != NULL with icc_size == NULL;
 * INVALID_QUALITY_FACTOR for a quality outside 0..100.  Per file, as in uhdr_hip_jpeg_encode_rgb_batch: BAD_PTR (data NULL or, in device
 * memory, not 4-byte aligned; out[i] NULL with a capacity), UNSUPPORTED_FEATURE (another pixelFormat), RESOLUTION_MISMATCH (size out
 * of range, or a luma_stride below the width). */
int uhdr_hip_jpeg_encode_rgba420_batch(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                       const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                       int mem_space, void* stream);
/* JPEG/R files from packed RGBA pairs: uhdr_hip_jpegr_encode_rgbmap_batch's signature and conventions with the packed pair in place of
 * the planar one and rgb_map choosing the map's form.  Per file: the gain map is uhdr_hip_generate_gainmap_packed_batch's with
 * metadata_in == NULL (rgb = rgb_map), compressed at quality 85 as uhdr_hip_jpeg_encode compresses a single plane, or as
 * uhdr_hip_jpeg_encode_rgb_batch does when rgb_map != 0; the primary image is uhdr_hip_jpeg_encode_rgba420_batch's at `quality` with the
 * ICC profile uhdr_hip_icc_profile(UHDR_HIP_TF_SRGB, the SDR gamut); the container is uhdr_hip_jpegr_append_gainmap(primary, map,
 * exif, NULL, 0, metadata), as API-1 calls it (jpegr.cpp:365-381).  Call-level: BAD_PTR (n < 0, a NULL array where n > 0, exif without
 * exif_size), INVALID_QUALITY_FACTOR.  Per file, API-1's checks where they apply, on the HDR image first: BAD_PTR (NULL data),
 * UNSUPPORTED_WIDTH_HEIGHT (odd, below 8 or above 8192), INVALID_COLORGAMUT, INVALID_STRIDE, BAD_PTR (out[i] NULL), INVALID_TRANS_FUNC
 * (none of LINEAR / HLG / PQ); then on the SDR image BAD_PTR, INVALID_STRIDE, RESOLUTION_MISMATCH, INVALID_COLORGAMUT; BAD_PTR for a
 * NULL exif[i] with a size; then uhdr_hip_generate_gainmap_packed_batch's own (pixel formats, alignment in device memory, the transfer
 * function against the HDR format -- every file by itself: hdr_tf is shared, so the files that pass have one HDR format).  The
 * files' generate, conversion and all 2 n compressions share their launches, one synchronisation per round of up to 64 files. */
int uhdr_hip_jpegr_encode_packed_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf, int quality,
                                       const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                       size_t* out_size, int* status, int rgb_map, int mem_space, void* stream);
/* uhdr_hip_apply_gainmap_packed_batch: HDR from an UHDR_HIP_PIX_FMT_RGBA8888 SDR image -- what UHDR_HIP_OUTPUT_SDR and
 * UHDR_HIP_DECODE_TO_RGBA hand out -- and its gain map: decode a file once, keep the two layers, render at any display boost.
 * Device memory, asynchronous on `stream`, graph-capturable; the one exception is the weight-table upload for a scale factor seen
 * for the first time, as in uhdr_hip_apply_gainmap_batch (uhdr_hip_stream_reserve covers it).
 *   sdr_images[i]      RGBA8888 as defined at the pixel-format constants: sRGB, full range, alpha ignored, 4-byte aligned, luma_stride
 *                      in pixels (0 = width).
 *   gainmap_images[i]  pixelFormat selects the form, as in uhdr_hip_apply_gainmap_md_batch: MONOCHROME or UNSPECIFIED -- one plane,
 *                      rows of `width` bytes; RGBA8888 -- per channel, 4-byte aligned, luma_stride in pixels (0 = width).  Every map
 *                      of a call has the first map's form.  Any integer scale factor, checked as the reference's applyGainMap checks it.
 *   DEGENERATE metadata (the *_md_* section's term): the reference's applyGainMap (ultrahdr.cpp:429-489) with lines 429-431 replaced by
 *                      rgb_gamma_sdr.c = (float)code_c * (1 / 255.0f); srgbInvOetf, sampleMap with the IDW tables, applyGain(...,
 *                      display_boost), / display_boost, the OETF and the packing of output_format follow unchanged.
 *   the contract       every step behind the pixel value is per channel, so channel c of a result pixel is channel c of
 *                      uhdr_hip_apply_gainmap_batch run on a grey image: Y = plane c of the SDR image, Cb = Cr = 128 (an RGBA map:
 *                      that run with plane c of the map).  UHDR_HIP_APPLY_EXACT and _EXACT_UNFILTERED: bit for bit -- every pixel
 *                      takes the exact path (the sRGB stage is a 256-entry table of the exact function's floats), there is no f32
 *                      pre-filter.  UHDR_HIP_APPLY_FAST: every 10-bit channel within 1 code and every F16 channel within 1
 *                      half-precision ULP of it.  UHDR_HIP_APPLY_LUT: ERROR_UNSUPPORTED_FEATURE.
 *   GENERAL metadata   the formula of the *_md_* section with e_c = srgbInvOetf((float)code_c * (1 / 255.0f)), the table's value; one
 *                      f32 arithmetic under FAST and EXACT, held to that section's bars against the formula in double; LUT and
 *                      EXACT_UNFILTERED return ERROR_UNSUPPORTED_FEATURE.
 *   output_format      1 .. 4 as in the planar calls; dests[i] comes back with width, height and the SDR image's colorGamut.  Alpha of
 *                      RGBA1010102 and RGBA F16 is what the planar calls write.  Nothing outside the output's bytes is written.
 * n == 0 is a no-op after the call-level checks.  Checks, in this order (the first that fails is the status):
 *   BAD_PTR                 n < 0, a NULL sdr_images / gainmap_images / dests where n > 0, or a NULL metadata
 *   UNSUPPORTED_FEATURE     (every image, before anything else of any image) an SDR pixelFormat other than RGBA8888; a map
 *                           pixelFormat other than MONOCHROME / UNSPECIFIED / RGBA8888; a map whose form differs from the first map's
 *   BAD_PTR                 (every image) a NULL data of the SDR image, the map or dests[i]; SDR data or an RGBA map's data not 4-byte
 *                           aligned; dests[i].data not aligned to a pixel's store (RGBA F16 8 bytes, RGBA1010102 4, planar 2)
 *   BAD_METADATA            the *_md_* section's validation (max < min included)
 *   INVALID_DISPLAY_BOOST   max_display_boost < 1 or NaN
 *   INVALID_OUTPUT_FORMAT   an output_format outside 1 .. 4
 *   UNSUPPORTED_FEATURE     the apply_mode, as stated above
 *   then per image          INVALID_STRIDE (a luma_stride of the SDR image or of an RGBA map below its width, or above 2^32 - 1);
 *                           UNSUPPORTED_MAP_SCALE_FACTOR (an empty map, a map size that does not divide the image's, or different
 *                           factors across and down).  Images of different sizes may share a call, as in the planar batch. */
int uhdr_hip_apply_gainmap_packed_batch(int n, const uhdr_hip_image_t* sdr_images, const uhdr_hip_image_t* gainmap_images,
                                        const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                                        uhdr_hip_image_t* dests, int apply_mode, void* stream);

/* ---- gain maps at any scale factor (no reference counterpart; current libultrahdr: uhdr_enc_set_gainmap_scale_factor) ------
 * The apply and decode calls read maps at any integer factor; every generate call above writes them at the reference's
 * kMapDimensionScaleFactor, 4.  This call takes the factor s = map_scale_factor, 1 .. 128.  Device memory, asynchronous on `stream`: it
 * only enqueues kernels -- no allocation, copy or host synchronisation, so it can be captured into a graph.
 *   map size       (width / s) x (height / s)
 *   sampling       map pixel (x, y) is the reference's samplePixels (gainmapmath.cpp:605-615) at scale s, for both images: one running
 *                  f32 sum per channel over the s x s block, dy outer and dx inner, of getYuv420Pixel / getP010Pixel values with their
 *                  own roundings -- y * (1/255.0f), (u - 128) * (1/255.0f), (y10 - 64) * (1/876.0f), (u10 - 64) * (1/896.0f) - 0.5f;
 *                  the chroma sample of a pixel is the one at (x/2, y/2) -- then each sum / (float)(s*s), correctly rounded.  Columns
 *                  and rows past s * (width / s), s * (height / s) are not read.
 *   the rest       metadata_in == NULL, rgb == 0: uhdr_hip_generate_gainmap_batch's arithmetic (behind the same f32 pre-filter, bytes
 *                  unchanged by it); metadata_in == NULL, rgb != 0: uhdr_hip_generate_gainmap_rgb_batch's; metadata_in != NULL:
 *                  uhdr_hip_generate_gainmap_md_batch's rule, validation and gamma handling.
 * metadata_out (optional) receives the metadata that was used.  dests[i].data needs (width / s) * (height / s) bytes, four times that
 * with rgb != 0, and comes back described as the selected call describes it, with the new size.  With s == 4 the bytes are those
 * three calls'.  There is no content_minmax.  Checks: those of the selected call in its order, and UNSUPPORTED_MAP_SCALE_FACTOR
 *   - directly after the call-level BAD_PTR for s outside 1 .. 128,
 *   - per image, after that image's other checks, when width / s == 0 or height / s == 0.
 * A failing call writes nothing. */
int uhdr_hip_generate_gainmap_scaled_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images, int hdr_tf,
                                           const uhdr_hip_metadata_t* metadata_in, uhdr_hip_metadata_t* metadata_out,
                                           uhdr_hip_image_t* dests, int sdr_is_601, int rgb, int map_scale_factor, void* stream);
/* Measurement only: the call above with metadata_in == NULL, rgb == 0 (the filtered kernel), counting.  *doubt_count -- one device
 * word, cleared by the caller -- grows by the number of map pixels the f32 pre-filter left to the exact path; the maps are the call's.
 * BAD_PTR for a NULL doubt_count, UNSUPPORTED_FEATURE for s == 4 (that kernel keeps lists of its own, uhdr_hip_generate_probe), then
 * the call's checks. */
int uhdr_hip_generate_gainmap_scaled_probe(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images, int hdr_tf,
                                           uhdr_hip_image_t* dests, int sdr_is_601, int map_scale_factor, uint32_t* doubt_count,
                                           void* stream);
/* uhdr_hip_jpegr_encode_batch (rgb_map == 0) or uhdr_hip_jpegr_encode_rgbmap_batch (rgb_map != 0) -- API-1, or API-0 when
 * yuv420_images == NULL -- with the gain map at s = map_scale_factor: the generate step is the call above with metadata_in == NULL;
 * the map is compressed at quality 85 as those calls compress theirs; primary image, ICC, XMP, MPF, container, per-file status rules
 * and the one synchronisation per round are unchanged.  With s == 4 the call IS the existing one, checks and bytes included.
 * Otherwise: call-level UNSUPPORTED_MAP_SCALE_FACTOR for s outside 1 .. 128, after INVALID_QUALITY_FACTOR; per file, behind API-1's own
 * checks, UNSUPPORTED_WIDTH_HEIGHT when width % s != 0 or height % s != 0 -- every reader, uhdr_hip_apply_gainmap_batch included,
 * refuses a map whose size does not divide the image's.  A round's map pool grows with the maps (up to 16 times a factor-4 map's
 * bytes at s = 1, 64 times with rgb_map); a round whose pool cannot be had fails as a whole, it is never truncated.  Read the files
 * with uhdr_hip_jpegr_decode_batch / uhdr_hip_jpegr_decode_rgbmap_batch. */
int uhdr_hip_jpegr_encode_scaled_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf,
                                       int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                       const size_t* out_capacity, size_t* out_size, int* status, int rgb_map, int map_scale_factor,
                                       int mem_space, void* stream);

/* ---- content-adaptive gain maps (no reference counterpart) ---------------------------------
 * The reference encodes every map against minContentBoost = 1, maxContentBoost = hdr_white / 203 (ultrahdr.cpp:250-257): 255 codes
 * over 2.3 stops (HLG, LINEAR) or 5.6 stops (PQ) whatever the picture holds, gains below 1 clipped.  The adaptive calls encode
 * against the range the content has.  With (g_min, g_max) the min and max over map pixels of the reference's unclamped f32 gain
 * (gainmapmath.cpp:531-534: 1 where y_sdr <= 0, else y_hdr / y_sdr -- the content_minmax statistic above), in f32:
 *     cap = (hdr_tf == PQ ? 10000.0f : 1000.0f) / 203.0f
 *     lo  = fminf(fmaxf(g_min, 0.25f),   1.0f)
 *     hi  = fminf(fmaxf(g_max, 1.0625f), cap)
 * so lo <= 1 < hi always (never a degenerate range, gain 1 always inside, never beyond the reference's maximum; a NaN or negative
 * g_min gives 0.25).  Metadata: version "1.0", minContentBoost = hdrCapacityMin = lo, maxContentBoost = hdrCapacityMax = hi,
 * gamma 1, offsets 0.  Map byte: the reference's three-argument encodeGain(y_sdr, y_hdr, metadata) (gainmapmath.cpp:524-541) with
 * log2MinContentBoost = (float)log2((double)lo), likewise for hi, on exactly the luminances generate computes.  Every decoder of the
 * format takes such a map: applyGainMap reads the range from the metadata.
 * boost_scope: PER_IMAGE -- every image its own range; PER_CALL -- one range for all n images of the call, the rule applied to
 * (min of the g_min, max of the g_max): bursts and frame sequences that must share metadata. */
#define UHDR_HIP_BOOST_PER_IMAGE 0
#define UHDR_HIP_BOOST_PER_CALL 1
/* The rule by itself, host code.  INVALID_TRANS_FUNC for a transfer function generate refuses, BAD_PTR for NULL. */
int uhdr_hip_adaptive_boost_range(int hdr_tf, float g_min, float g_max, float* lo, float* hi);
int uhdr_hip_adaptive_metadata(int hdr_tf, float g_min, float g_max, uhdr_hip_metadata_t* metadata);
/* generateGainMap for n pairs against the measured range.  Device memory only; the call only enqueues kernels on `stream` -- no
 * allocation, no copy, no host synchronisation -- and can be captured into a graph.  The range never visits the host: pass 1
 * (k_generate_gains) stores every map pixel's unclamped f32 gain, 4 bytes per map pixel, into `workspace` and finds the exact
 * extremes; one small launch (k_adaptive_consts) applies the rule and derives the encode constants per image, or once for the call;
 * pass 2 (k_encode_gains) turns the stored gains into bytes.  Pass 1 evaluates every pixel on the exact (f64) path.
 *   content_minmax  DEVICE, 2 n floats, optional: every image's own (g_min, g_max), in either scope
 *   boost_range     DEVICE, 2 n floats, required: the (lo, hi) map i was encoded against (PER_CALL: n equal pairs)
 *   workspace       DEVICE, 16-byte aligned, at least what uhdr_hip_generate_adaptive_workspace_bytes answers for the same n and
 *                   images (it reads their sizes only; 0 for n == 0); its contents before and after the call mean nothing
 * dests[i] is filled as by uhdr_hip_generate_gainmap_batch.  Checks, in this order: those of uhdr_hip_generate_gainmap_batch_ex;
 * UNSUPPORTED_FEATURE for an unknown boost_scope; BAD_PTR for a NULL (or misaligned) workspace or a NULL boost_range where n > 0;
 * ERROR_INSUFFICIENT_RESOURCE for a workspace smaller than the query's answer.  Nothing is written by a call that fails them. */
int uhdr_hip_generate_adaptive_workspace_bytes(int n, const uhdr_hip_image_t* yuv420_images, size_t* bytes);
int uhdr_hip_generate_gainmap_adaptive_batch(int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images,
                                             int hdr_tf, uhdr_hip_image_t* dests, int sdr_is_601, int boost_scope,
                                             float* content_minmax, float* boost_range, void* workspace, size_t workspace_bytes,
                                             void* stream);
/* One image through the adaptive batch with the measured metadata returned to the host: planes in mem_space (host planes are staged
 * like uhdr_hip_generate_gainmap's), the workspace is the library's, and the call waits for `stream` in either memory space. */
int uhdr_hip_generate_gainmap_adaptive(const uhdr_hip_image_t* yuv420_image, const uhdr_hip_image_t* p010_image, int hdr_tf,
                                       uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest, int sdr_is_601, int mem_space,
                                       void* stream);
/* uhdr_hip_jpegr_encode_batch with the generate step replaced by the adaptive one: the same checks in the same order, the same
 * rounds, the same single synchronisation per round, the same per-file status semantics; the primary JPEG of every file is the one
 * uhdr_hip_jpegr_encode_batch writes.  An unknown boost_scope is UNSUPPORTED_FEATURE, right after INVALID_QUALITY_FACTOR.  A round's
 * boost_range pairs come down with its compressed streams; the containers carry the measured range in the gain map's XMP, and
 * metadata (HOST, n entries, optional) receives it for every file that was processed.  The workspace is a pool slot of the call's
 * codec context.  PER_CALL pools the files that passed their checks; with more than one round (more than 64 such files) the
 * statistic of ALL rounds is taken before any map is encoded: every round is staged and measured once, then staged again and
 * encoded. */
int uhdr_hip_jpegr_encode_adaptive_batch(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images,
                                         int hdr_tf, int quality, const void* const* exif, const size_t* exif_size,
                                         void* const* out, const size_t* out_capacity, size_t* out_size,
                                         uhdr_hip_metadata_t* metadata, int* status, int boost_scope, int mem_space, void* stream);

/* ---- tone-mapped SDR base image for API-0 (no reference counterpart) -------------------------
 * UltraHdr::toneMap shifts the P010 code values to 8 bits: the PQ- or HLG-encoded signal becomes the "SDR" image, which a legacy
 * viewer shows washed out and against which most of the gain map clips to the floor of its range.  REINHARD_MAXRGB derives an SDR
 * rendition instead.  For an HDR image with transfer function hdr_tf (HLG, PQ, LINEAR, as generate accepts) and gamut G, in f32:
 *   1. per pixel: yuv = getP010Pixel(x, y) (a 2x2 block shares its chroma sample), rgb' = <G>YuvToRgb(yuv), clamped to [0, 1]
 *   2. lin = invOETF_hdr_tf(rgb') per channel -- generate's exact functions; LINEAR is the identity; no HLG OOTF, as in generate
 *   3. white = 10000 for PQ, else 1000;  k = white / 203.0f;  cap = k
 *   4. the image's headroom H.  Given (hdr_peak_nits[i] > 0):  H = fminf(fmaxf(hdr_peak_nits[i] / 203.0f, 1.0f), cap).
 *      Measured (hdr_peak_nits == NULL or hdr_peak_nits[i] == 0):  m' = the maximum over all pixels and the three channels of the
 *      clamped rgb' of step 1 -- taken before linearisation: the inverse OETFs are monotone --,
 *      H = fminf(fmaxf(invOETF(m') * k, 1.0f), cap)
 *   5. extended Reinhard on the maximum channel: v = lin * k; M = max(v.r, v.g, v.b); s = M > 0 ? (1 + M / (H * H)) / (1 + M) : 1;
 *      o = clamp(v * s, 0, 1).  H == 1 is the identity on [0, 1]; the gain the map has to restore is 1 / s, in [1, H], inside the
 *      reference's constant boost range
 *   6. e = sRGB OETF(o) per channel: o <= 0.0031308f ? 12.92f * o : 1.055f * powf(o, 1 / 2.4f) - 0.055f
 *   7. yuv_out = <G>RgbToYuv(e): the SDR image keeps the HDR image's gamut, as API-0's does today
 *   8. quantised like transformYuv420 (gainmapmath.cpp:513-519): Y = (uint8)CLIP3(y * 255.0f + 0.5f, 0, 255) per pixel; per 2x2
 *      block u = (((u00 + u01) + u10) + u11) * 0.25f, U = (uint8)CLIP3(u * 255.0f + 128.0f + 0.5f, 0, 255), V likewise
 * The destination is laid out like uhdr_hip_tonemap's: planar Y, U, V, V chroma_stride * height / 2 behind U, the padding columns
 * [width, stride) zeroed, dest->colorGamut = src->colorGamut.  Step 2 is bit-exact; the steps behind it run on the f32 units. */
#define UHDR_HIP_TONEMAP_SHIFT 0            /* the reference's toneMap: what every other call does */
#define UHDR_HIP_TONEMAP_REINHARD_MAXRGB 1  /* the operator above */
/* The headroom rule by itself, host code: gamma_max = m' of step 4 (ignored when peak_nits > 0).  BAD_PTR for NULL,
 * INVALID_TRANS_FUNC for a transfer function generate refuses, UNSUPPORTED_FEATURE for a negative or non-finite peak_nits. */
int uhdr_hip_tonemap_headroom(int hdr_tf, float gamma_max, float peak_nits, float* headroom);
/* n images in DEVICE memory.  The call only enqueues kernels on `stream` -- no allocation, no copy, no host synchronisation -- and
 * the headroom never visits the host: the slots are set (0 or the given H), k_tonemap_peak reduces m' of the measured images into
 * them, one small launch turns m' into H, k_tonemap_sdr writes the planes.  Images of equal size and gamut that follow each other
 * share launches (grid.z = image, up to 32).
 *   hdr_peak_nits  HOST, n floats, or NULL (every headroom measured)
 *   headroom       DEVICE, n floats, required for REINHARD_MAXRGB: image i's H
 * Checks, in this order, all before any launch (a failing call writes nothing): those of uhdr_hip_tonemap_batch;
 * INVALID_TRANS_FUNC; UNSUPPORTED_FEATURE for an unknown tonemap_op -- TONEMAP_SHIFT is uhdr_hip_tonemap_batch from here --;
 * UNSUPPORTED_FEATURE for a negative or non-finite hdr_peak_nits[i]; BAD_PTR for a NULL headroom where n > 0; then per image
 * UNSUPPORTED_WIDTH_HEIGHT for an odd width or height, INVALID_COLORGAMUT, INVALID_STRIDE for a stride shorter than its row.
 * Strides: a source luma_stride of 0 means width, as getP010Pixel reads it (gainmapmath.cpp:585).  Nothing else is defaulted:
 * chroma_data is required (uhdr_hip_tonemap_batch's check), and beside a chroma pointer a chroma_stride below width -- 0 included
 * -- is INVALID_STRIDE, as in the encode calls' areInputArgumentsValid, which default the chroma stride only together with a NULL
 * chroma pointer; the destination strides are the caller's, as for uhdr_hip_tonemap. */
int uhdr_hip_tonemap_sdr_batch(int n, const uhdr_hip_image_t* p010_images, uhdr_hip_image_t* dests, int hdr_tf, int tonemap_op,
                               const float* hdr_peak_nits, float* headroom, void* stream);
/* One image, planes in mem_space (host planes are staged like uhdr_hip_tonemap's); waits for `stream` in either memory space and
 * returns H to the host (headroom: HOST, optional; untouched by TONEMAP_SHIFT). */
int uhdr_hip_tonemap_sdr(const uhdr_hip_image_t* p010_image, uhdr_hip_image_t* dest, int hdr_tf, int tonemap_op, float hdr_peak_nits,
                         float* headroom, int mem_space, void* stream);
/* encodeJPEGR API-0 for n files with the chosen operator: uhdr_hip_jpegr_encode_batch with yuv420_images == NULL whose toneMap step
 * is uhdr_hip_tonemap_sdr_batch (the headroom array is a pool slot of the round's codec context); generate, the BT.601 re-encode,
 * the compressions, the single synchronisation per round and the containers are that call's.  boost_scope = -1: the reference's
 * constant range; UHDR_HIP_BOOST_PER_IMAGE / PER_CALL: the adaptive generate of uhdr_hip_jpegr_encode_adaptive_batch.  metadata
 * (HOST, n entries, optional) receives what every processed file's container carries.  Checks: those of
 * uhdr_hip_jpegr_encode_batch, then UNSUPPORTED_FEATURE for an unknown tonemap_op or boost_scope; per file, behind that call's
 * checks, UNSUPPORTED_FEATURE for a negative or non-finite hdr_peak_nits[i] (REINHARD_MAXRGB only).  With TONEMAP_SHIFT and
 * boost_scope = -1 the call is uhdr_hip_jpegr_encode_batch. */
int uhdr_hip_jpegr_encode_api0_tonemapped_batch(int n, const uhdr_hip_image_t* p010_images, int hdr_tf, int quality,
                                                const void* const* exif, const size_t* exif_size, void* const* out,
                                                const size_t* out_capacity, size_t* out_size, uhdr_hip_metadata_t* metadata,
                                                int* status, int tonemap_op, const float* hdr_peak_nits, int boost_scope,
                                                int mem_space, void* stream);

/* ---- tone-mapped SDR image from a packed HDR image: the packed API-0 (no reference counterpart) ----
 * The operator above for a caller that holds only a packed HDR image: an UHDR_HIP_PIX_FMT_RGBA1010102 (hdr_tf HLG or PQ) or
 * UHDR_HIP_PIX_FMT_RGBA_F16 (hdr_tf LINEAR) image, layouts and alignment as the packed section defines them, becomes an
 * UHDR_HIP_PIX_FMT_RGBA8888 one -- no narrow-range quantisation, no chroma subsampling.  In f32:
 *   1. per pixel and channel the pixel value of the packed generate: RGBA1010102 (float)code10 * (1 / 1023.0f); RGBA_F16 the exact f32
 *      of the half, subnormals included; then clamped to [0, 1] with fminf(fmaxf(x, 0), 1): -0 and negative halves give 0, halves
 *      above 1.0 give 1.  Alpha is ignored
 *   2. lin = invOETF_hdr_tf(value) per channel -- generate's exact functions; LINEAR is the identity; no HLG OOTF.  (An RGBA1010102
 *      channel has 1024 values: the device reads the exact function's result from a table of them.)
 *   3. white = 10000 for PQ, else 1000;  k = white / 203.0f;  cap = k
 *   4. the image's headroom H.  Given (hdr_peak_nits[i] > 0):  H = fminf(fmaxf(hdr_peak_nits[i] / 203.0f, 1.0f), cap).
 *      Measured (hdr_peak_nits == NULL or hdr_peak_nits[i] == 0):  m' = the maximum over all pixels and the three channels of step 1's
 *      clamped value -- for RGBA1010102 an integer maximum of the codes, converted once --,
 *      H = fminf(fmaxf(invOETF(m') * k, 1.0f), cap): uhdr_hip_tonemap_headroom states the rule for both operators
 *   5. extended Reinhard on the maximum channel: v = lin * k; M = max(v.r, v.g, v.b); s = M > 0 ? (1 + M / (H * H)) / (1 + M) : 1;
 *      o = clamp(v * s, 0, 1)
 *   6. e = sRGB OETF(o) per channel: o <= 0.0031308f ? 12.92f * o : 1.055f * powf(o, 1 / 2.4f) - 0.055f
 *   7. R, G, B = (uint8)CLIP3(e * 255.0f + 0.5f, 0, 255) per channel, A = 0xFF
 * The destination: dest->data, rows dest->luma_stride pixels apart (0 = width; the caller's, in pixels), 4-byte aligned.  The columns
 * [width, stride) are NOT written.  The call sets dest->width / height to the source's, dest->luma_stride to the stride used,
 * dest->pixelFormat = RGBA8888 and dest->colorGamut = src->colorGamut: the SDR image keeps the HDR gamut, as API-0's does.  Step 2 is
 * bit-exact; the steps behind it run on the f32 units.  A pixel holding a non-finite half: its own output is unspecified, a measured
 * H is then unspecified within [1, cap]; nothing outside the destination is written, and nothing faults.
 *
 * n images in DEVICE memory.  The call only enqueues kernels on `stream` -- no allocation, no copy, no host synchronisation; it can be
 * captured into a graph on any stream, nothing needs reserving -- and H never visits the host: the slots are set, the measuring
 * pass reduces m' of the measured images into them, one small launch turns m' into H, the last pass writes the pixels.  Images of
 * equal size that follow each other share launches (grid.z = image, up to 32).
 *   tonemap_op     UHDR_HIP_TONEMAP_REINHARD_MAXRGB; UHDR_HIP_TONEMAP_SHIFT has no meaning for these formats
 *   hdr_peak_nits  HOST, n floats, or NULL (every headroom measured)
 *   headroom       DEVICE, n floats, required: image i's H
 * Checks, in this order, all before any launch (a failing call writes nothing):
 *   BAD_PTR              n < 0, or a NULL hdr_images / dests where n > 0
 *   UNSUPPORTED_FEATURE  (every image) a pixelFormat other than RGBA1010102 / RGBA_F16, or one that differs from hdr_images[0]'s
 *   BAD_PTR              (every image) a NULL data on either side; source data not 4-byte aligned (RGBA_F16: 8-byte), destination data
 *                        not 4-byte aligned
 *   INVALID_TRANS_FUNC   RGBA_F16 with anything but LINEAR, RGBA1010102 with anything but HLG / PQ; n == 0: hdr_tf none of the three
 *   UNSUPPORTED_FEATURE  a tonemap_op other than REINHARD_MAXRGB; a negative or non-finite hdr_peak_nits[i]
 *   BAD_PTR              a NULL headroom where n > 0
 *   then per image       INVALID_STRIDE (on either side a luma_stride below the width, or above 2^32 - 1); INVALID_COLORGAMUT */
int uhdr_hip_tonemap_packed_batch(int n, const uhdr_hip_image_t* hdr_images, uhdr_hip_image_t* dests, int hdr_tf, int tonemap_op,
                                  const float* hdr_peak_nits, float* headroom, void* stream);
/* One image in mem_space (host pixels are staged; only the pixels come back, the host destination's padding columns stay as they
 * are; nothing is asked of a host pointer's alignment); waits for `stream` in either memory space and returns H to the host
 * (headroom: HOST, optional).  BAD_PTR for a NULL hdr_image or dest, then the batch call's checks for n = 1. */
int uhdr_hip_tonemap_packed(const uhdr_hip_image_t* hdr_image, uhdr_hip_image_t* dest, int hdr_tf, int tonemap_op, float hdr_peak_nits,
                            float* headroom, int mem_space, void* stream);
/* JPEG/R files from packed HDR images alone: uhdr_hip_jpegr_encode_packed_batch without sdr_images.  Per round of up to 64 files the
 * SDR images are uhdr_hip_tonemap_packed_batch's, written into a pool slot of the round's codec context (rows at a 64-byte pitch;
 * the headroom array is a pool slot too); everything behind that is uhdr_hip_jpegr_encode_packed_batch's own: the generate with
 * metadata_in == NULL, the RGBA8888 -> 4:2:0 primary with the ICC profile of the HDR image's gamut, the 2 m compressions behind one
 * synchronisation, the container.  A file equals, byte for byte, what uhdr_hip_jpegr_encode_packed_batch writes for the same HDR image
 * and the RGBA8888 image uhdr_hip_tonemap_packed_batch derives from it.
 *   metadata       HOST, n entries, optional: what every processed file's container carries
 *   hdr_peak_nits  HOST, n floats, or NULL
 * Checks: call-level BAD_PTR and INVALID_QUALITY_FACTOR as uhdr_hip_jpegr_encode_packed_batch, then UNSUPPORTED_FEATURE for a
 * tonemap_op other than REINHARD_MAXRGB; per file that call's HDR-side checks in their order (the SDR-side ones fall away), then
 * UNSUPPORTED_FEATURE for a negative or non-finite hdr_peak_nits[i], which fails that file alone. */
int uhdr_hip_jpegr_encode_packed_api0_batch(int n, const uhdr_hip_image_t* hdr_images, int hdr_tf, int quality, const void* const* exif,
                                            const size_t* exif_size, void* const* out, const size_t* out_capacity, size_t* out_size,
                                            uhdr_hip_metadata_t* metadata, int* status, int tonemap_op, const float* hdr_peak_nits,
                                            int rgb_map, int mem_space, void* stream);

/* ---- content-adaptive gain maps for packed RGBA inputs (no reference counterpart) -------------
 * The two sections above joined: the packed pair of uhdr_hip_generate_gainmap_packed_batch, encoded against the boost range its
 * content has.  The definition:
 *   sampling, colours  those of uhdr_hip_generate_gainmap_packed_batch, word for word: samplePixels per channel over the 4 x 4 block of
 *                      both images, srgbInvOetf / hdrInvOetf(hdr_tf), the conversion into the SDR image's gamut -- the exact path.
 *   rgb == 0           g = y_sdr > 0 ? y_hdr / y_sdr : 1 in f32 (gainmapmath.cpp:531-534), on the two luminances in nits that call
 *                      hands to encodeGain: the SDR gamut's luminance of both colours, times 203.0f and times hdr_white_nits.
 *   rgb != 0           the same gain per channel, on sdr.c * 203.0f and hdr.c * hdr_white_nits.
 *   (g_min, g_max)     the extremes over all map pixels; with rgb != 0 over all three channels of all map pixels: the metadata
 *                      carries one range.
 *   range, metadata    uhdr_hip_adaptive_boost_range(hdr_tf, g_min, g_max) and uhdr_hip_adaptive_metadata, unchanged.
 *   map byte           the reference's three-argument encodeGain against that metadata: what uhdr_hip_generate_gainmap_packed_batch
 *                      writes when it is given that metadata as metadata_in.
 *   boost_scope        PER_IMAGE and PER_CALL as in uhdr_hip_generate_gainmap_adaptive_batch.
 * A map pixel that reads a non-finite half is unspecified, as in the packed generate; the range still satisfies lo <= 1 < hi (the
 * rule's fminf / fmaxf drop a NaN and cap an infinity).
 * uhdr_hip_generate_gainmap_packed_adaptive_batch.  Device memory only; the call only enqueues kernels on `stream` -- no allocation,
 * no copy, no host synchronisation -- and can be captured into a graph.  The sources are read once: pass 1 (k_generate_packed_gains)
 * stores every map pixel's unclamped f32 gains into `workspace`, 4 bytes per map pixel, 12 (R, G, B) with rgb != 0, and finds the
 * extremes; k_adaptive_consts applies the rule; pass 2 (k_encode_gains, k_encode_gains_rgb) turns the stored gains into the map.
 *   content_minmax  DEVICE, 2 n floats, optional: every image's own (g_min, g_max), in either scope
 *   boost_range     DEVICE, 2 n floats, required: the (lo, hi) map i was encoded against (PER_CALL: n equal pairs)
 *   workspace       DEVICE, 16-byte aligned, at least what uhdr_hip_generate_packed_adaptive_workspace_bytes answers for the same n,
 *                   images and rgb (it reads the images' sizes only; 0 for n == 0; BAD_PTR for a NULL bytes, n < 0 or a NULL array
 *                   where n > 0); its contents before and after the call mean nothing
 * dests[i] needs what uhdr_hip_generate_gainmap_packed_batch's needs and comes back described as that call describes it.  Checks, in
 * this order: those of uhdr_hip_generate_gainmap_packed_batch with metadata_in == NULL; UNSUPPORTED_FEATURE for an unknown
 * boost_scope; BAD_PTR for a NULL or not 16-byte aligned workspace or a NULL boost_range where n > 0; ERROR_INSUFFICIENT_RESOURCE for a
 * workspace smaller than the query's answer.  Nothing is written by a call that fails them. */
int uhdr_hip_generate_packed_adaptive_workspace_bytes(int n, const uhdr_hip_image_t* sdr_images, int rgb, size_t* bytes);
int uhdr_hip_generate_gainmap_packed_adaptive_batch(int n, const uhdr_hip_image_t* sdr_images, const uhdr_hip_image_t* hdr_images,
                                                    int hdr_tf, uhdr_hip_image_t* dests, int rgb, int boost_scope, float* content_minmax,
                                                    float* boost_range, void* workspace, size_t workspace_bytes, void* stream);
/* One pair in DEVICE memory through that call with PER_IMAGE, the workspace the library's, the measured metadata returned to the
 * host (required): the call waits for `stream`.  BAD_PTR for a NULL argument, then the batch call's image checks for n = 1. */
int uhdr_hip_generate_gainmap_packed_adaptive(const uhdr_hip_image_t* sdr_image, const uhdr_hip_image_t* hdr_image, int hdr_tf,
                                              uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dest, int rgb, void* stream);
/* uhdr_hip_jpegr_encode_packed_batch (sdr_images != NULL) or uhdr_hip_jpegr_encode_packed_api0_batch (sdr_images == NULL: the SDR
 * images are uhdr_hip_tonemap_packed_batch's, hdr_peak_nits as in that call -- HOST, n floats or NULL; it is not read when sdr_images
 * is given) with the generate step replaced by the call above: the same checks in the same order, the same rounds and sort, the same
 * single synchronisation per round, the same primary JPEG, ICC profile and container.  An unknown boost_scope is UNSUPPORTED_FEATURE,
 * right after INVALID_QUALITY_FACTOR.  A round's boost_range pairs come down with its compressed streams; the containers carry the
 * measured range in the gain map's XMP, and metadata (HOST, n entries, optional) receives it for every file that was processed.  The
 * workspace is a pool slot of the call's codec context.  PER_CALL pools the files that passed their checks; over more than one round
 * (more than 64 such files) it follows uhdr_hip_jpegr_encode_adaptive_batch's rule: every round is staged (API-0: tone-mapped) and
 * measured first, the pooled extremes carried from round to round in device memory, then every round is staged again and encoded. */
int uhdr_hip_jpegr_encode_packed_adaptive_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf,
                                                int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                                const size_t* out_capacity, size_t* out_size, uhdr_hip_metadata_t* metadata, int* status,
                                                const float* hdr_peak_nits, int rgb_map, int boost_scope, int mem_space, void* stream);

/* ---- introspection for tests -------------------------------------------------------------- */
/* copies the 4 Shepard IDW weight tables (standard, no-right, no-bottom, corner; each
 * scale*scale*4 floats; gainmapmath.h:184-228) the apply kernels use for `scale` into out[] */
int uhdr_hip_idw_tables(int scale, float* out);

/* copies static LUT `which` (0 kSrgbInvOETF[1024], 1 kHlgInvOETF[4096], 2 kPqInvOETF[4096], 4 kHlgOETF[65536],
 * 5 kPqOETF[65536]; gainmapmath.cpp:21-64) from the device into out[capacity] (HOST); *count = its length */
int uhdr_hip_lut_table(int which, float* out, size_t capacity, size_t* count);
/* GainLUT::mGainTable (gainmapmath.h:151-182) as LUT-mode apply builds it: 1024 floats into out (HOST);
 * with_display_boost == 0 is GainLUT(metadata), otherwise GainLUT(metadata, display_boost) */
int uhdr_hip_gain_lut(const uhdr_hip_metadata_t* metadata, int with_display_boost, float display_boost, float* out);

/* evaluates one scalar device function over n floats (DEVICE pointers), out[i] = f(in[i]):
 *   fn 0/1/2  sRGB / HLG / PQ inverse OETF as generate computes them (lean f64 + rounding test + exact fallback)
 *   fn 3      encodeGain byte (as float) of gain in[i] for (min_boost, max_boost), generate's version
 *   fn 10..13 the same four through the exact (ocml f64) path;  14/15 HLG / PQ OETF exact
 *   fn 20/24/25 apply-FAST sRGB EOTF / HLG OETF / PQ OETF;  21/22 the f32 HLG / PQ inverse OETF of generate's pre-filter; 23 v_log_f32
 *   fn 40/41/42/44/45 srgbInvOetfLUT / hlgInvOetfLUT / pqInvOetfLUT / hlgOetfLUT / pqOetfLUT; 46 GainLUT(min, max,
 *              displayBoost = max).getGainFactor(in[i])
 *   fn 60      (float)log2((double)in[i]): the log2 constant the content-adaptive path derives on the device for boost in[i]
 *              (50-54 read FAST apply's line-segment tables)
 *   fn 30/31   gain-map byte -> float through the constant division / the IEEE division (in[i] = byte as float)
 *   fn 100/101 1.0 where the lean path of fn 0/1 passed its rounding test, else 0.0
 * Used by the exhaustive transfer-function tests. */
int uhdr_hip_eval_transfer(int fn, const float* in, float* out, size_t n, float min_boost, float max_boost,
                           void* stream);

/* The route uhdr_hip_generate_gainmap_batch_ex takes for a call, and the two kernels of its filtered route one at a time -- what
 * the tests of the hand-over between k_generate's filter and k_generate_resolve are built on.  The arguments up to `stream` are
 * that call's and are checked as there (n >= 1); only the FIRST chunk of the call (the leading images of one size, gamut pair and
 * alignment class, at most 64) is looked at.
 *   phase 0  host only, nothing is launched and no device is needed (the data pointers are examined for alignment, never read):
 *            route[0 .. UHDR_HIP_GENERATE_ROUTE_WORDS) receives the chunk's route and the layout constants of the statistics
 *            workspace, indexed by the UHDR_HIP_GENERATE_ROUTE_* names below.
 *   phase 1  enqueues the filtered kernel alone, then copies, in stream order, the header words [0, route[HDR_WORDS]) of every
 *            image's workspace to headers (DEVICE, n * route[HDR_WORDS] uint32): word route[SWEEP_WORD] is set when a wave's slots
 *            overflowed, [route[LIST_COUNTS] + l] holds the entries of list l, [route[SLOT_COUNTS] + w] the count word of wave w
 *            (plain entries | saved entries << 8) where route[SLOTS] != 0.  The map bytes of pixels in doubt are provisional.
 *   phase 2  enqueues k_generate_resolve alone, on the stream's workspace as phase 1 left it: same arguments, same stream, nothing
 *            of the library on that stream in between.
 * Phases 1 and 2 serve a call that is ONE chunk on the filtered-kernel-plus-k_generate_resolve route; ERROR_UNSUPPORTED_FEATURE
 * otherwise, and for a phase outside 0..2.  BAD_PTR for n < 1, a NULL route in phase 0 or NULL headers in phase 1. */
enum {
  UHDR_HIP_GENERATE_ROUTE_RESOLVE = 0,     /* 1: the filtered kernel followed by k_generate_resolve */
  UHDR_HIP_GENERATE_ROUTE_SPANS = 1,       /* spans of BLOCK pairs a block walks: 1 or 4 */
  UHDR_HIP_GENERATE_ROUTE_SLOTS = 2,       /* GenConsts::stat_slots: waves per image when they append to slots of their own, else 0 */
  UHDR_HIP_GENERATE_ROUTE_SPREAD = 3,      /* GenConsts::stat_spread */
  UHDR_HIP_GENERATE_ROUTE_IMAGES = 4,      /* images in the chunk */
  UHDR_HIP_GENERATE_ROUTE_BLOCK = 5,       /* kGenBlock: threads (= pixel pairs per span) of a block */
  UHDR_HIP_GENERATE_ROUTE_HDR_WORDS = 6,   /* kStatHdr */
  UHDR_HIP_GENERATE_ROUTE_SLOT_COUNTS = 7, /* kStatSlotCnt: first of the waves' count words */
  UHDR_HIP_GENERATE_ROUTE_SLOT_PLAIN = 8,  /* kStatSlotPlain */
  UHDR_HIP_GENERATE_ROUTE_SLOT_SAVED = 9,  /* kStatSlotSaved */
  UHDR_HIP_GENERATE_ROUTE_LISTS = 10,      /* kStatLists */
  UHDR_HIP_GENERATE_ROUTE_LIST_CAP = 11,   /* kStatCap */
  UHDR_HIP_GENERATE_ROUTE_LIST_COUNTS = 12,/* first of the lists' count words */
  UHDR_HIP_GENERATE_ROUTE_SWEEP_WORD = 13, /* the word a wave sets whose slots overflowed */
  UHDR_HIP_GENERATE_ROUTE_RESOLVE_SLICES = 14, /* kResolveSlices: blocks of 256 threads k_generate_resolve spends per image */
  UHDR_HIP_GENERATE_ROUTE_SLOT_WAVES = 15, /* kStatSlotWaves: the most waves per image the slots serve */
  UHDR_HIP_GENERATE_ROUTE_WORDS = 16
};
int uhdr_hip_generate_probe(int phase, int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* p010_images,
                            int hdr_tf, uhdr_hip_metadata_t* metadata, uhdr_hip_image_t* dests, int sdr_is_601,
                            int generate_mode, float* content_minmax, void* stream, uint32_t* route, uint32_t* headers);

/* The same for EXACT apply: the route uhdr_hip_apply_gainmap_batch takes for a call in UHDR_HIP_APPLY_EXACT mode, and the two
 * kernels of its estimate-plus-k_apply_resolve route one at a time -- what the tests of the hand-over between the f32 estimate's
 * lists of pixels in doubt and k_apply_resolve are built on.  The arguments up to `stream` are that call's (apply_mode is
 * UHDR_HIP_APPLY_EXACT) and are checked as there, in its order, but n >= 1; only the FIRST chunk of the call (the leading images
 * of one size, map size and alignment class, at most 64) is looked at.
 *   phase 0  host only, nothing is launched and no device is needed (the data pointers are examined for alignment, never read):
 *            route[0 .. UHDR_HIP_APPLY_ROUTE_WORDS) receives the chunk's route and the layout constants of the stream's workspace,
 *            indexed by the UHDR_HIP_APPLY_ROUTE_* names below.  Like the call itself, every phase fills width, height and colorGamut
 *            of the chunk's destination descriptors.
 *   phase 1  enqueues the estimate kernel alone (every pixel's f32 estimate is written; the pixels in doubt are appended to the
 *            image's lists), then copies, in stream order, the header words [0, route[HDR_WORDS]) of every image to headers
 *            (DEVICE, n * route[HDR_WORDS] uint32): [route[LIST_COUNTS] + l] holds the appends to list l -- beyond route[LIST_CAP]
 *            the entries are dropped and the image is swept --, [route[SLICE_WORD]] the slices of k_apply_resolve that have finished.
 *   phase 2  enqueues k_apply_resolve alone, on the stream's workspace as phase 1 left it: same arguments, same stream, nothing
 *            of the library on that stream in between but further phases 1 of the same geometry (their appends go behind those
 *            already there: the counts add up).  It leaves the headers cleared.
 * Phases 1 and 2 serve a call that is ONE chunk on the estimate-plus-k_apply_resolve route; ERROR_UNSUPPORTED_FEATURE otherwise,
 * and for a phase outside 0..2.  BAD_PTR for n < 1, a NULL route in phase 0 or NULL headers in phase 1. */
enum {
  UHDR_HIP_APPLY_ROUTE_RESOLVE = 0,        /* 1: an estimate kernel followed by k_apply_resolve */
  UHDR_HIP_APPLY_ROUTE_CELLS = 1,          /* 1: k_apply_s4_est (a thread per 4x4 map cell), 0: k_apply_px_est (a thread per pixel) */
  UHDR_HIP_APPLY_ROUTE_IMAGES = 2,         /* images in the chunk */
  UHDR_HIP_APPLY_ROUTE_LISTS = 3,          /* kExLists: lists per image */
  UHDR_HIP_APPLY_ROUTE_LIST_CAP = 4,       /* ex_cap: entries a list holds at this image size (0 without RESOLVE) */
  UHDR_HIP_APPLY_ROUTE_HDR_WORDS = 5,      /* kExHdrWords */
  UHDR_HIP_APPLY_ROUTE_LIST_COUNTS = 6,    /* first of the lists' count words */
  UHDR_HIP_APPLY_ROUTE_SLICE_WORD = 7,     /* the word that counts the finished slices of k_apply_resolve */
  UHDR_HIP_APPLY_ROUTE_RESOLVE_SLICES = 8, /* kExSlices: blocks of 256 threads k_apply_resolve spends per image */
  UHDR_HIP_APPLY_ROUTE_GRID_X = 9,         /* the estimate kernel's gridDim.x: blocks of 256 cells (CELLS) or of 256 pixels of a row */
  UHDR_HIP_APPLY_ROUTE_GRID_Y = 10,        /* its gridDim.y: rows of the per-pixel kernel (further rows by striding); CELLS: the images */
  UHDR_HIP_APPLY_ROUTE_WORDS = 11
};
int uhdr_hip_apply_exact_probe(int phase, int n, const uhdr_hip_image_t* yuv420_images, const uhdr_hip_image_t* gainmaps,
                               const uhdr_hip_metadata_t* metadata, int output_format, float max_display_boost,
                               uhdr_hip_image_t* dests, void* stream, uint32_t* route, uint32_t* headers);

/* A test hook, host only.  The batched codec calls (JPEG and JPEG/R encode, decode and edit) take their files through the device in
 * rounds whose workspace and staging are held to a byte bound, 2 GiB by default.  This call sets that bound for
 * every later call of the process and returns the one it replaces; 0 restores the default.  The bound changes how many rounds a call
 * takes, never a byte or a status of its result: a file larger than the bound gets a round of its own.  tests take a call across a
 * round seam with it at sizes of a few kilobytes; nothing else has a reason to call it. */
size_t uhdr_hip_codec_round_bytes_probe(size_t bytes);

/* ---- Optimised Huffman tables for the JPEG encoder --------------------------------------------------------
 * libjpeg's optimize_coding: a file's four Huffman tables (two for a single plane) are built from the histogram of its own symbols
 * instead of being the Annex K defaults.  No pixel changes; the file is smaller and equals, byte for byte, what libjpeg-turbo
 * writes with optimize_coding for the same coefficients.  Histogram, tables (jpeg_gen_optimal_table), DHT and SOS segments and the
 * entropy-coded stream are all made on the device: the call synchronises no more often than without the flag.
 *
 * The _ex calls take every argument and convention of the call they extend, plus `flags` in front of mem_space.  flags == 0 IS that
 * call, bytes and statuses included.  A bit other than those below is the call's ERROR_UNSUPPORTED_FEATURE, checked before the
 * device is touched.  With OPTIMIZE_HUFFMAN a file of more than 15 873 015 blocks (63 symbols a block could reach libjpeg's
 * "no frequency" of 10^9; about a gigapixel) is that file's ERROR_UNSUPPORTED_FEATURE.  In the JPEG/R call both the primary image
 * and the gain-map JPEG get their own tables; the container follows from their sizes.  A header with optimised tables is never
 * longer than the default one, so a capacity that holds the default file holds the optimised one. */
#define UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN 1
int uhdr_hip_jpeg_encode_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                  void* const* out, const size_t* out_capacity, size_t* out_size, int* status, int flags, int mem_space,
                                  void* stream);
int uhdr_hip_jpeg_encode_rgb_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                      size_t* out_size, int* status, int flags, int mem_space, void* stream);
int uhdr_hip_jpeg_encode_rgba420_batch_ex(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                          const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                          int flags, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_batch_ex(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                   const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                   size_t* out_size, int* status, int flags, int mem_space, void* stream);
/* Diagnostic: the encoder's table kernel on a caller's histogram (HOST arrays): freq[s] = count of symbol s; bits[l - 1] receives
 * the number of codes of length l, vals[0, *nvals) the symbols by code length, then value (a DHT segment's body).  BAD_PTR for a
 * NULL array, a histogram without a non-zero count, or a count >= 1 000 000 000; ERROR_UNSUPPORTED_FEATURE where a code would be
 * longer than 32 bits before the limit to 16 (libjpeg gives up there; the encoder then keeps that table's default). */
int uhdr_hip_jpeg_optimal_table(const uint32_t freq[256], uint8_t bits[16], uint8_t vals[256], int* nvals, void* stream);

/* ---- Restart intervals for the JPEG encoder ---------------------------------------------------------------
 * libjpeg's restart_interval / restart_in_rows: a DRI segment between the last DHT and SOS, and after every `interval` MCUs except
 * the last group the partial byte filled with ones, RSTn (n counting modulo 8) and the DC prediction of every component back at 0.
 * The file equals, byte for byte, what libjpeg-turbo writes with the same setting; it decodes to the same pixels, in independent
 * byte-aligned pieces.  Padding, markers and the cut prediction are the device's work: the call synchronises no more often.
 *
 * The _opts calls take every argument and convention of their _ex call with `opts` in place of `flags`; one opts holds for the
 * whole call.  opts == NULL, or both restart fields 0, IS the _ex call with opts->flags, bytes and statuses included.
 * restart_in_rows > 0 overrides restart_interval: the interval is min(restart_in_rows * MCUs per row, 65535) with the MCUs per row
 * of the scan written -- ceil(width / 16) for 4:2:0, ceil(width / 8) for a single plane and for 4:4:4 -- so in the JPEG/R call the
 * primary image and the gain map each get their own.  An interval of at least the image's MCUs writes DRI and no marker.
 * A wrong struct_size, an unknown flag bit or restart_interval > 65535 is the call's ERROR_UNSUPPORTED_FEATURE, checked before the
 * device is touched and before any pointer.  A file of more than 20 000 000 blocks with intervals is that file's
 * ERROR_UNSUPPORTED_FEATURE.  The file grows by the 6 bytes of DRI and at most 3 bytes per interval. */
typedef struct {
  uint32_t struct_size;       /* sizeof(uhdr_hip_jpeg_encode_opts_t); anything else: ERROR_UNSUPPORTED_FEATURE */
  uint32_t flags;             /* the _ex calls' bits (UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN) */
  uint32_t restart_interval;  /* libjpeg's restart_interval: MCUs per interval, 0 = none, at most 65535 */
  uint32_t restart_in_rows;   /* libjpeg's restart_in_rows: MCU rows per interval, 0 = use restart_interval */
} uhdr_hip_jpeg_encode_opts_t;
int uhdr_hip_jpeg_encode_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc, const size_t* icc_size,
                                    void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                    const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
int uhdr_hip_jpeg_encode_rgb_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, void* const* out, const size_t* out_capacity,
                                        size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
int uhdr_hip_jpeg_encode_rgba420_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                            const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                            const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_batch_opts(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                     const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                     size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
/* Host only: the MCUs per interval the encoder derives from opts for a scan of `width` pixels whose MCUs are mcu_width (8 or 16)
 * pixels wide; 0: no intervals.  *restart_mcus is left alone where opts would be refused (the call's ERROR_UNSUPPORTED_FEATURE).
 * The two widths cover every sampling the encoder writes: 16 for 4:2:0 and 4:2:2, 8 for 4:4:4, 4:4:0 and a single plane. */
int uhdr_hip_jpeg_restart_mcus(const uhdr_hip_jpeg_encode_opts_t* opts, size_t width, int mcu_width, uint32_t* restart_mcus);

/* ---- 4:4:4, 4:2:2 and 4:4:0 files from planes and from RGBA8888 -------------------------------------------
 * The encoder's counterpart of UHDR_HIP_DECODE_ANY_SAMPLING: luma sampling 1x1, 2x1 or 1x2 over 1x1 chroma in the frame header, MCUs
 * of 3, 4 and 4 blocks (Y blocks in rows of hs, then Cb, Cr).  Optimised tables and restart intervals (opts) apply as for 4:2:0;
 * restart_in_rows counts the MCUs per row of the sampling written: ceil(width / 16) for 4:2:2, ceil(width / 8) for 4:4:4 and 4:4:0.
 *
 * uhdr_hip_jpeg_encode_planes_batch_opts: uhdr_hip_jpeg_encode_batch_opts -- arguments, memory spaces, ICC per file, size probe
 * (out[i] == NULL with capacity 0), per-file statuses, rounds, NULL opts -- where an image of UHDR_HIP_PIX_FMT_YUV444 / YUV422 /
 * YUV440 is compressed as what it says, from planes laid out as uhdr_hip_jpeg_decode_batch_ex hands them out: chroma of
 * ceil(width / hs) x ceil(height / vs) samples at chroma_data, rows chroma_stride apart, Cr behind Cb at chroma_stride x chroma
 * height (a stride of 0: the plane's width).  The file is the baseline file libjpeg writes in raw-data mode for those planes with
 * jpeg_set_quality(q, TRUE) and the ISLOW DCT.  Partial blocks are padded as libjpeg pads them, each plane on its own grid: the last
 * column repeated out to the block grid, then the last row -- NOT the zero rows and columns of the 4:2:0 and single-plane calls,
 * which keep theirs here as everywhere.  Every other pixelFormat in the same call behaves exactly as in
 * uhdr_hip_jpeg_encode_batch_opts, and a mixed batch shares its launches.  Per file, in this order: BAD_PTR for NULL data or
 * chroma_data, or a NULL out[i] with a capacity; ERROR_RESOLUTION_MISMATCH outside 1x1 .. 65500x65500 (odd sizes are accepted);
 * ERROR_INVALID_STRIDE for a luma stride below the width or a chroma stride below the chroma width; ERROR_UNSUPPORTED_FEATURE where
 * the block limits of the options are exceeded; ERROR_INSUFFICIENT_RESOURCE with the size in out_size[i] for a file that does not fit.
 *
 * uhdr_hip_jpeg_encode_rgba_batch_opts: uhdr_hip_jpeg_encode_rgba420_batch_opts with `sampling` in front of opts.
 * UHDR_HIP_PIX_FMT_YUV420 IS that call.  YUV444 writes uhdr_hip_jpeg_encode_rgb_batch_opts' file, with the ICC segment where the
 * other calls put it.  YUV422 is libjpeg's file for JCS_RGB input with 2x1 luma sampling: jccolor.c's conversion at full resolution,
 * jcsample.c's h2v1_downsample of the chroma, edges expanded as libjpeg expands them -- converted and downsampled on the device in
 * one launch per round.  Any other value (YUV440 among them) is the call's ERROR_UNSUPPORTED_FEATURE, returned after the opts check
 * and before anything else.
 *
 * uhdr_hip_jpegr_encode_packed_sampling_batch: uhdr_hip_jpegr_encode_packed_batch with `primary_sampling` (YUV444 / YUV422 / YUV420;
 * anything else: ERROR_UNSUPPORTED_FEATURE) and `opts` behind rgb_map.  The primary image is the call above at that sampling with the
 * file's ICC profile; opts holds for the primary image and the gain-map JPEG alike.  Gain map, metadata, container and checks are
 * the packed call's; with YUV420 and NULL opts it IS that call.  uhdr_hip_jpegr_decode_batch_ex reads a 4:4:4 or 4:2:2 file with
 * UHDR_HIP_DECODE_ANY_SAMPLING. */
int uhdr_hip_jpeg_encode_planes_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                           const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                           const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
int uhdr_hip_jpeg_encode_rgba_batch_opts(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                         const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                         int sampling, const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_packed_sampling_batch(int n, const uhdr_hip_image_t* hdr_images, const uhdr_hip_image_t* sdr_images, int hdr_tf,
                                                int quality, const void* const* exif, const size_t* exif_size, void* const* out,
                                                const size_t* out_capacity, size_t* out_size, int* status, int rgb_map, int primary_sampling,
                                                const uhdr_hip_jpeg_encode_opts_t* opts, int mem_space, void* stream);

/* ---- Progressive files from the JPEG encoder ---------------------------------------------------------------
 * libjpeg's jpeg_simple_progression, which Pillow writes for progressive=True: SOF2 and ten scans (six for a single plane) over the
 * quantised coefficients the baseline call computes -- DC at Al 1, luma AC 1-5 at Al 2, Cr and Cb AC 1-63 at Al 1, luma AC 6-63 at
 * Al 2, the luma refinement to Al 1, the DC refinement, and the refinements of Cr, Cb and luma to Al 0 --, each scan behind the DHT
 * segment(s) of tables built from its own symbols and its SOS.  The file equals, byte for byte, what libjpeg-turbo writes; it
 * decodes to the baseline file's pixels and is usually a few per cent smaller than the optimised baseline file.  Symbols,
 * end-of-band runs across blocks, buffered correction bits, histograms, tables, segments, bit offsets, emission and stuffing of
 * every scan are the device's work: the call synchronises no more often, and its launches do not grow with images or blocks.
 *
 * The _scans calls take every argument and convention of their _opts call with `scan_mode` directly behind opts.
 * UHDR_HIP_SCANS_BASELINE IS that call: bytes, statuses, order of checks.  Any other value than the two below is the call's
 * ERROR_UNSUPPORTED_FEATURE, checked right after the opts check, before any pointer is looked at and before the device is touched.
 * With UHDR_HIP_SCANS_PROGRESSIVE:
 *   - a non-zero restart_interval or restart_in_rows is the call's ERROR_UNSUPPORTED_FEATURE at the same place: restart intervals
 *     inside progressive scans are not written;
 *   - UHDR_HIP_ENCODE_OPTIMIZE_HUFFMAN is accepted and changes nothing: a progressive file has tables of its own in every scan, as
 *     libjpeg forces optimize_coding for it;
 *   - the planes call covers YUV420, MONOCHROME, YUV444, YUV422 and YUV440, the RGBA call the samplings 4:4:4, 4:2:2 and 4:2:0; in
 *     the JPEG/R call the primary image and the gain-map JPEG are both progressive;
 *   - memory spaces, ICC, the size probe, per-file statuses and rounds are the _opts call's.  A file of more than 8 000 000 blocks
 *     is that file's ERROR_UNSUPPORTED_FEATURE (the optimised path's limit is 15 873 015);
 *   - a scan whose optimal code would be deeper than 32 bits has no default table to fall back to (Annex K's AC table has no EOBn
 *     symbols): that file's status is ERROR_UNSUPPORTED_FEATURE, as libjpeg fails with JERR_HUFF_CLEN_OVERFLOW;
 *   - a progressive file can be longer than its baseline form (small images: ten scan headers); size a buffer by the size probe.
 * uhdr_hip_jpeg_decode_batch_ex, uhdr_hip_jpegr_decode and the shim's decodeJPEGR read these files. */
#define UHDR_HIP_SCANS_BASELINE 0
#define UHDR_HIP_SCANS_PROGRESSIVE 1
int uhdr_hip_jpeg_encode_planes_batch_scans(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                            const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                            const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space, void* stream);
int uhdr_hip_jpeg_encode_rgba_batch_scans(int n, const uhdr_hip_image_t* images, const int* quality, const void* const* icc,
                                          const size_t* icc_size, void* const* out, const size_t* out_capacity, size_t* out_size, int* status,
                                          int sampling, const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space, void* stream);
int uhdr_hip_jpegr_encode_batch_scans(int n, const uhdr_hip_image_t* p010_images, const uhdr_hip_image_t* yuv420_images, int hdr_tf, int quality,
                                      const void* const* exif, const size_t* exif_size, void* const* out, const size_t* out_capacity,
                                      size_t* out_size, int* status, const uhdr_hip_jpeg_encode_opts_t* opts, int scan_mode, int mem_space,
                                      void* stream);

/* Bench / test support: the deterministic synthetic frame pair of SURVEY.md 8(d) (an LCG; tests/ and bench.py compare it with the
 * oracle's serial loop), written into device memory: p010 = width*height*3/2 uint16 (luma, then interleaved UV, values in the
 * legal 10-bit ranges << 6), yuv = width*height*3/2 bytes (Y, U, V).  width and height even; enqueued on `stream`. */
int uhdr_hip_synth_lcg_frame(size_t width, size_t height, unsigned int seed, void* p010, void* yuv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UHDR_HIP_H */
