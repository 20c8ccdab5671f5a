/*
 * flyimg_hip.h -- C-ABI of libflyimg_hip.so, the MI355X (gfx950) image hot
 * path of flyimg.  Plain C: pointers, sizes and PODs only.
 *
 * What each entry point replaces in the reference (v1o/flyimg):
 *
 *   fi_plan / fi_process_batch / fi_process_batch_device
 *       replace ImageProcessor::processNewImage -> generateCommand ->
 *       Processor::execute("convert ...") (src/Core/Processor/
 *       ImageProcessor.php:49-57, :66-110; Processor.php:44-62): the resize
 *       operator (-thumbnail/-resize, :264-272) with its geometry
 *       (generateCropSize :138-148 / generateSimpleSize :154-162),
 *       -gravity/-extent (c_1), -colorspace Gray (clsp_Gray, :88),
 *       -rotate (forwarded option, :303-315), and -- when FI_SMARTCROP is set --
 *       SmartCropProcessor::smartCrop (SmartCropProcessor.php:21-36: the
 *       python3 smartcrop.py exec plus the "convert -crop" exec).
 *   fi_smartcrop / fi_smartcrop_ex
 *       replace SmartCrop().crop(...) of python/smartcrop.py:137-191 (the
 *       ctypes path of the drop-in smartcrop CLI, smartcrop.py:341-377).
 *
 * Error convention (Processor.php:53-59 throws ExecFailedException on a
 * non-zero exit): every call returns FI_OK (0) or a negative FI_E* code and
 * fi_last_error() returns the thread-local message of the last failure.
 * The PHP FFI shim maps a non-zero return to ExecFailedException; the Python
 * shim maps FI_ENOCROP to ValueError (smartcrop.py:227-228) and the rest to
 * RuntimeError.
 *
 * Ownership: host buffers are caller-owned; device memory, pinned staging and
 * tap tables are owned by the fi_ctx.  Threading: calls on one fi_ctx are
 * serialised by an internal mutex.  One fi_ctx per process per GPU (one
 * process per GPU; torch.distributed-style launch).
 */
#ifndef FLYIMG_HIP_H
#define FLYIMG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FI_ABI_VERSION 2  /* 2: forwarded convolution operators (unsharp/sharpen/blur fields) */

/* ---- status codes ---------------------------------------------------- */
#define FI_OK 0
#define FI_EINVAL (-1)       /* bad argument / geometry                     */
#define FI_ENOCROP (-2)      /* smartcrop.py crops(): ValueError (:227-228) */
#define FI_ENOMEM (-3)       /* host or device allocation failed            */
#define FI_EDEVICE (-4)      /* HIP runtime / kernel error                  */
#define FI_EUNSUPPORTED (-5) /* operator not implemented on this path       */
#define FI_ECAPACITY (-6)    /* dst_capacity too small (see fi_plan)        */

/* ---- per-image operator flags (mirror the convert argv) --------------- */
#define FI_OP_THUMBNAIL (1u << 0)      /* -thumbnail (default, ImageProcessor.php:269)   */
#define FI_OP_RESIZE (1u << 1)         /* -resize (rz_1)                                  */
#define FI_GEOM_FILL (1u << 2)         /* '^' geometry flag (generateCropSize :143)       */
#define FI_GEOM_SHRINK_ONLY (1u << 3)  /* '>' geometry flag (generateSimpleSize :159)     */
#define FI_OP_EXTENT (1u << 4)         /* -gravity G -extent WxH (c_1, :144-145)          */
#define FI_OP_GRAY (1u << 5)           /* -colorspace Gray (clsp_Gray, :88)               */
#define FI_OP_MONOCHROME (1u << 6)     /* -monochrome (mnchr_1, :90-92); implies Gray      */
#define FI_OP_ROTATE (1u << 7)         /* -rotate <deg>, multiples of 90 (r_90, :306)     */
#define FI_OP_SMARTCROP (1u << 8)      /* compute smartcrop.py's box on the result (smc_1) */
#define FI_OP_SMARTCROP_APPLY (1u << 9) /* and crop to it (SmartCropProcessor.php:30-34)   */
/* forwarded convolutions (ImageProcessor.php:303-315), after -rotate, in this order: */
#define FI_OP_UNSHARP (1u << 10)       /* -unsharp RxS+gain+threshold (unsh_)               */
#define FI_OP_SHARPEN (1u << 11)       /* -sharpen RxS (sh_)                                */
#define FI_OP_BLUR (1u << 12)          /* -blur RxS (blr_)                                  */
/* The source is an IM PseudoClass image (palette PNG/GIF, 8-bit gray PNG,
 * 1-component JPEG -- IM's readers give them a colormap): ResizeImage's
 * default filter is then Mitchell, not Lanczos (resize.c). */
#define FI_SRC_PSEUDOCLASS (1u << 13)
/* -rotate by any integer number of degrees (opt-in): with FI_OP_ROTATE, the part
 * of `rotate` that is no multiple of 90 runs IM's RotateImage three-shear
 * rotation (shear.c) after the integral rotation.  Opaque RGB / Gray images
 * only; without this flag such an angle is FI_EUNSUPPORTED, as it always was. */
#define FI_OP_ROTATE_SHEAR (1u << 14)
/* -background: `background` (0x00RRGGBB) fills what a shear rotation uncovers;
 * without the flag IM's default, white.  No effect without a shear rotation. */
#define FI_OP_BACKGROUND (1u << 15)

/* ImageMagick GravityType values used by -gravity (parameters.yml:99). */
#define FI_GRAVITY_NORTHWEST 1
#define FI_GRAVITY_NORTH 2
#define FI_GRAVITY_NORTHEAST 3
#define FI_GRAVITY_WEST 4
#define FI_GRAVITY_CENTER 5
#define FI_GRAVITY_EAST 6
#define FI_GRAVITY_SOUTHWEST 7
#define FI_GRAVITY_SOUTH 8
#define FI_GRAVITY_SOUTHEAST 9

/* One image of a batch.  Caller fills the inputs; the library fills the
 * "filled by library" fields.  For fi_process_batch the pointers are host
 * pointers; for fi_process_batch_device they are device pointers. */
typedef struct fi_image {
  const uint8_t *src;      /* HWC RGB8, or RGBA8 (straight alpha)             */
  int32_t src_w, src_h;    /* pixels                                          */
  int32_t src_stride;      /* bytes per row                                   */
  int32_t src_channels;    /* 3, or 4: an IM matte image (PNG with alpha) --   *
                            * Mitchell, alpha-weighted passes (resize.c), out *
                            * RGBA8 or gray+alpha (2); no smartcrop / mono    */
  int32_t target_w;        /* geometry W (0 = absent, getDimensions :240-259) */
  int32_t target_h;        /* geometry H (0 = absent)                         */
  uint32_t flags;          /* FI_OP_* | FI_GEOM_*                             */
  int32_t gravity;         /* FI_GRAVITY_*, 0 = Center                        */
  int32_t rotate;          /* degrees for FI_OP_ROTATE (multiple of 90, or    *
                            * any integer with FI_OP_ROTATE_SHEAR)            */
  int32_t smartcrop_w;     /* smartcrop.py --width  (0 = 100, CLI default)    */
  int32_t smartcrop_h;     /* smartcrop.py --height (0 = 100)                 */
  uint32_t background;     /* 0x00RRGGBB, read only with FI_OP_BACKGROUND (in  *
                            * what was the padding before dst: no field moved) */
  uint8_t *dst;            /* output pixels, HWC, out_stride bytes per row    */
  int64_t dst_capacity;    /* bytes available at dst                          */
  /* ---- filled by library ---- */
  int32_t out_w, out_h, out_channels, out_stride;
  int32_t crop_x, crop_y, crop_w, crop_h; /* smartcrop top_crop (smartcrop.py:184-190 rescaled) */
  double crop_score;                      /* top_crop["score"]["total"]           */
  int32_t status;                         /* FI_OK or FI_E* for this image        */
  int32_t n_candidates;                   /* crops re-scored exactly (diagnostic) */
  /* ---- inputs of the forwarded convolutions (ABI 2), IM ParseGeometry values ---- */
  double unsharp[4];       /* radius, sigma (1), gain (1), threshold (0.05) -- FI_OP_UNSHARP */
  double sharpen[2];       /* radius, sigma (1)                             -- FI_OP_SHARPEN */
  double blur[2];          /* radius, sigma (1)                             -- FI_OP_BLUR    */
} fi_image;

/* SmartCrop.__init__ keyword arguments (python/smartcrop.py:41-77). */
typedef struct fi_smartcrop_params {
  double detail_weight;             /* 0.2  */
  double edge_radius;               /* 0.4  */
  double edge_weight;               /* -10  */
  double outside_importance;        /* -0.5 */
  int32_t rule_of_thirds;           /* 1    */
  double saturation_bias;           /* 0.2  */
  double saturation_brightness_max; /* 0.9  */
  double saturation_brightness_min; /* 0.05 */
  double saturation_threshold;      /* 0.4  */
  double saturation_weight;         /* 0.3  */
  int32_t score_down_sample;        /* 1 (only 1 is supported)  */
  double skin_bias;                 /* 0.01 */
  double skin_brightness_max;       /* 1    */
  double skin_brightness_min;       /* 0.2  */
  double skin_color[3];             /* 0.78, 0.57, 0.44 */
  double skin_threshold;            /* 0.8  */
  double skin_weight;               /* 1.8  */
} fi_smartcrop_params;

/* SmartCrop.crop() keyword arguments (smartcrop.py:137-147). */
typedef struct fi_smartcrop_options {
  int32_t prescale;   /* 1 */
  double max_scale;   /* 1 */
  double min_scale;   /* 0.9 */
  double scale_step;  /* 0.1 */
  int32_t step;       /* 8 */
  int32_t exact_all;  /* 1 = score every crop with the reference's sequential sum */
} fi_smartcrop_options;

/* One entry of result["crops"] (smartcrop.py:184-190, score :300-338). */
typedef struct fi_crop_score {
  int32_t x, y, width, height;      /* rescaled ints (crop() :184-190)                  */
  double fx, fy, fw, fh;            /* analysed-image geometry before rescale           */
  double detail, saturation, skin, total; /* exact when `exact` != 0                   */
  int32_t exact;                    /* 1: sequential reference sum; 0: fast-pass value */
  int32_t pad;
} fi_crop_score;

typedef struct fi_ctx fi_ctx;

int32_t fi_abi_version(void);
const char *fi_last_error(void);

/* Devices and contexts. device = HIP ordinal (one process per GPU). */
int fi_device_count(int32_t *count);
int fi_create(fi_ctx **out, int32_t device);
void fi_destroy(fi_ctx *ctx);

/* Geometry only (no pixel work, no GPU): fills out_w/out_h/out_channels/
 * out_stride for each image; status per image.  Returns FI_OK if all ok. */
int fi_plan(fi_image *imgs, int32_t n);
/* Per-image algorithmic HBM bytes of the hot path (SURVEY.md 8(d)/(e)
 * B_img = R_touched * W_in * C_in + out_w * out_h * out_c + 16 when
 * FI_OP_SMARTCROP, + the integral Q16 image a shear rotation reads), R_touched = source rows with a non-zero vertical tap
 * after the ThumbnailImage sample step.  The multi-GPU sharder balances
 * these (greedy LPT).  bytes[i] = -1 for an image that does not plan. */
int fi_plan_bytes(const fi_image *imgs, int32_t n, int64_t *bytes);

/* Face-blur pixelation (FaceDetectProcessor::blurFaces,
 * FaceDetectProcessor.php:58-74): for each box (x, y, w, h) in order -- the
 * facedetect output lines "x y w h" -- the effect of
 *   mogrify -gravity NorthWest -region WxH+X+Y -scale 10% -scale 1000% <img>
 * on an 8-bit HWC image (channels 1 or 3), in place.  FI_EINVAL for a box
 * outside the image or whose 10% scale is empty (IM: NegativeOrZeroImageSize);
 * boxes before it are applied.  Host buffer (synchronous) and device-resident
 * forms (img on ctx's device, stream-ordered after earlier batches). */
int fi_pixelate_regions(fi_ctx *ctx, uint8_t *img, int32_t w, int32_t h, int32_t stride, int32_t channels,
                        const int32_t *boxes, int32_t nboxes);
int fi_pixelate_regions_device(fi_ctx *ctx, uint8_t *img, int32_t w, int32_t h, int32_t stride, int32_t channels,
                               const int32_t *boxes, int32_t nboxes);

/* Host buffers: H2D -> kernels -> D2H.  Synchronous. */
int fi_process_batch(fi_ctx *ctx, fi_image *imgs, int32_t n);
/* Asynchronous form of fi_process_batch: sources are staged to the device
 * and the batch is queued; outputs and records are final after fi_wait.
 * Three batches can be in flight (the next one's staging and upload overlap the
 * earlier ones' kernels).  Sources and outputs in pinned memory
 * (fi_host_alloc) are copied by DMA directly; pageable ones go through the
 * library's pinned staging.  imgs and the buffers must stay valid until
 * fi_wait returns for this batch. */
int fi_submit_batch(fi_ctx *ctx, fi_image *imgs, int32_t n);
/* Pinned host memory for decode targets and outputs of fi_submit_batch. */
void *fi_host_alloc(fi_ctx *ctx, size_t bytes);
int fi_host_free(fi_ctx *ctx, void *p);
/* Device-resident buffers (src/dst are device pointers on ctx's device).
 * Synchronous; the timed kernels are recorded in fi_kernel_stats. */
int fi_process_batch_device(fi_ctx *ctx, fi_image *imgs, int32_t n);
/* Asynchronous form of fi_process_batch_device for pipelined serving: plans,
 * uploads and launches the batch, then returns; `imgs` must stay valid until
 * fi_wait().  Batch k+1 is planned and uploaded on the host while batch k runs
 * on the GPU (three pinned staging slots; a fourth submit waits for the
 * oldest batch).  Streams: the resample, smartcrop and -monochrome /
 * convolution kernels of every batch run on the context's main stream in
 * submission order; the FI_OP_SMARTCROP_APPLY crop of batch k runs on a
 * second stream beside batch k+1's resample (one small workgroup per CU; with
 * FI_SC_CX=3 the whole smartcrop stage of an eligible batch does), and batch
 * k's records and outputs are final once that apply is done (fi_wait covers it).
 * Ordering across the two streams is kept for the caller: a later batch whose
 * sources overlap an earlier batch's dst, and the device-ordered entry points
 * (fi_pixelate_regions_device, fi_jpeg_decode_device, fi_jpeg_encode_device,
 * fi_fill_synthetic) wait for the applies still running.  The dst buffers of two in-flight batches
 * must not overlap (sources may be shared).
 * fi_wait(ctx, keep) finalizes submitted batches in order -- fills their
 * result fields -- until at most `keep` remain in flight (0 = drain all) and
 * returns the first error.  fi_query(ctx, &running) returns, without
 * blocking, how many submitted batches are still running on the GPU. */
int fi_submit_batch_device(fi_ctx *ctx, fi_image *imgs, int32_t n);
int fi_wait(fi_ctx *ctx, int32_t keep);
int fi_query(fi_ctx *ctx, int32_t *running);

/* smartcrop.py SmartCrop().crop(rgb, target_w, target_h) on host RGB8.
 * out_xywh = top_crop x, y, width, height; *out_score = its total. */
void fi_smartcrop_default_params(fi_smartcrop_params *p);
void fi_smartcrop_default_options(fi_smartcrop_options *o);
int fi_smartcrop(fi_ctx *ctx, const uint8_t *rgb, int32_t w, int32_t h, int32_t stride,
                 int32_t target_w, int32_t target_h, const fi_smartcrop_params *params,
                 int32_t out_xywh[4], double *out_score);
/* Full result: every crop, top index, analysed maps (skin, edge, sat HWC) and
 * the prescaled image (both analyse_w*analyse_h*3 bytes, may be NULL). */
int fi_smartcrop_ex(fi_ctx *ctx, const uint8_t *rgb, int32_t w, int32_t h, int32_t stride,
                    int32_t target_w, int32_t target_h, const fi_smartcrop_params *params,
                    const fi_smartcrop_options *opts, fi_crop_score *crops, int32_t crops_cap,
                    int32_t *n_crops, int32_t *top_index, int32_t analyse_wh[2],
                    double *prescale, uint8_t *prescaled_out, uint8_t *maps_out,
                    int64_t out_cap);

/* Device memory and synthetic inputs (device-resident batches / benchmarks). */
int fi_device_malloc(fi_ctx *ctx, void **ptr, uint64_t bytes);
int fi_device_free(fi_ctx *ctx, void *ptr);
int fi_memcpy_h2d(fi_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int fi_memcpy_d2h(fi_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* Seeded synthetic RGB8 image (flyimg_amd/synth.py bit for bit). */
int fi_fill_synthetic(fi_ctx *ctx, uint8_t *dev, int32_t w, int32_t h, int32_t stride,
                      uint32_t seed);

/* Stage timing (HIP event ranges on the launch streams).  enable: 0 off, 1
 * every stage ("batch", "resize", "rotate", "sc_prep", "sc_score", "crop_apply", "mono",
 * "conv", "h2d_src", "d2h_out"), 2 the resample stage only (each event range
 * adds a few microseconds between dependent kernels).  fi_kernel_stats also
 * reports host timings ("host_*", "host_total") and per-path image counters
 * ("path_vr", "path_vm", "path_hv", "path_generic_v", "path_generic_h",
 * "path_copy", "sc_path_fd", "sc_path_fz", "sc_path_cx"; "vr_fork": batches
 * whose later k_rs_vr launches ran on the forked stream).  bytes = algorithmic bytes
 * accounted to that stage. */
int fi_set_timing(fi_ctx *ctx, int32_t enable);
int fi_reset_stats(fi_ctx *ctx);
int fi_kernel_stats(fi_ctx *ctx, const char *name, double *total_ms, int64_t *launches,
                    double *bytes);

/* Multi-GPU: the one exchange step is the gather of per-image result
 * records to rank 0 over RCCL (xGMI).  The 128-byte unique id is created by
 * rank 0 and distributed out of band. */
typedef struct fi_record {
  int32_t image, status, out_w, out_h;
  int32_t crop_x, crop_y, crop_w, crop_h;
} fi_record;
int fi_rccl_get_unique_id(uint8_t id[128]);
int fi_rccl_init(fi_ctx *ctx, int32_t rank, int32_t world, const uint8_t id[128]);
/* Every rank sends `count` records (same count on every rank); rank 0
 * receives world*count records in rank order.  The gather runs on a stream
 * of its own (no dependency on the batch streams: the records are host data
 * once fi_wait has filled them).  fi_rccl_gather_start enqueues it and
 * returns (send is copied before it returns; recv is written by the matching
 * fi_rccl_gather_finish, which waits); one gather is in flight at a time (a
 * second start finishes the first).  fi_rccl_gather_records = start +
 * finish.  Every rank issues the same sequence of gathers. */
int fi_rccl_gather_start(fi_ctx *ctx, const fi_record *send, int32_t count, fi_record *recv);
int fi_rccl_gather_finish(fi_ctx *ctx);
int fi_rccl_gather_records(fi_ctx *ctx, const fi_record *send, int32_t count, fi_record *recv);

/* Test hook (not a reference interface): the -monochrome kernels on a
 * caller-supplied Q16 gray image (host buffers), w x h row-major, rotated by
 * rot (0/90/180/270) into out (0/255 bytes).  Lets the parity tests feed the
 * oracle's or_im_monochrome the identical input. */
/* Test hook (not a reference interface): the forwarded convolution kernels
 * (FI_OP_UNSHARP/SHARPEN/BLUR bits 0/1/2 of `ops`, conv = the fi_image
 * unsharp[4], sharpen[2], blur[2] values) on a rotated Q16 HWC image
 * (ch 1 or 3) -> 8-bit out (w * ch bytes per row), so tests can run the
 * oracle's or_im_convolve_ops on the identical input. */
int fi_debug_convolve(fi_ctx *ctx, const uint16_t *q16, int32_t w, int32_t h, int32_t ch, const double conv[8],
                      uint32_t ops, uint8_t *out);
int fi_debug_monochrome(fi_ctx *ctx, const uint16_t *gray, int32_t w, int32_t h, int32_t rot, uint8_t *out,
                        int32_t out_stride);
/* Test hook (not a reference interface): the rotation stage (fi_rotate.hip) on
 * a caller-supplied Q16 HWC image (host buffers, ch 1 or 3): -rotate `degrees`
 * with -background `background` (0x00RRGGBB), the integral part included.
 * *out_w x *out_h = the rotated image's size; out_q16 (its Q16 pixels) and out8
 * (ScaleQuantumToChar of them, *out_w * ch bytes per row) may each be NULL.
 * ctx == NULL: the planner alone -- the size, or FI_EUNSUPPORTED where a shear
 * would leave IM's canvas -- with no GPU. */
int fi_debug_rotate(fi_ctx *ctx, const uint16_t *q16, int32_t w, int32_t h, int32_t ch, int32_t degrees,
                    uint32_t background, uint16_t *out_q16, uint8_t *out8, int32_t *out_w, int32_t *out_h);
/* Its host model: the per-pixel procedure the kernel runs (taps, blends,
 * rounding), compiled for the CPU and run over the same arguments with no GPU,
 * so the CPU suite holds the kernel's arithmetic to the literal restatement. */
int fi_debug_rotate_host(const uint16_t *q16, int32_t w, int32_t h, int32_t ch, int32_t degrees,
                         uint32_t background, uint16_t *out_q16, uint8_t *out8, int32_t *out_w, int32_t *out_h);
/* GPU JPEG decode: the decode step of ImageProcessor's `convert` (IM reads
 * the source with libjpeg; ImageProcessor.php:66-110) moved onto the device,
 * bit-exact with libjpeg-turbo's default decompression (islow IDCT, fancy
 * upsampling, YCbCr->RGB).  Baseline / extended sequential Huffman 8-bit
 * streams with one scan: gray, or YCbCr with 4:4:4, 4:2:2 or 4:2:0 chroma.
 * fi_jpeg_info (host only): dimensions and output channels (1 gray, 3 RGB),
 * FI_EUNSUPPORTED for streams to decode on the host (progressive, CMYK, ...).
 * fi_jpeg_decode_device: decodes n streams (host memory) into caller device
 * buffers dst[i] (HWC rows of dst_stride[i] bytes; out_channels 0 = the
 * source's, 3 = RGB for every source, gray replicated) and waits; status[i]
 * per image; returns the first failing status (the others are decoded).
 * Damaged streams decode as libjpeg decodes them (entropy data that runs out
 * leaves the rest of its restart interval grey) or are FI_EUNSUPPORTED:
 * restart markers out of sequence already in fi_jpeg_info; corrupt data whose
 * coefficients leave the range in which the decoders agree only in the
 * decode's status[i], so a caller always handles FI_EUNSUPPORTED there. */
int fi_jpeg_info(const uint8_t *data, size_t len, int32_t *w, int32_t *h, int32_t *channels);
int fi_jpeg_decode_device(fi_ctx *ctx, const uint8_t *const *data, const size_t *len, int32_t n,
                          uint8_t *const *dst, const int64_t *dst_stride, int32_t out_channels,
                          int32_t *status);
/* Progressive sources, opt-in: with FI_JPEG_PROGRESSIVE in `flags` the two
 * functions below also take SOF2 (Huffman progressive, 8-bit) streams of the
 * same colour spaces and samplings, provided the scan script is complete --
 * every coefficient of every component sent and refined to its last bit, as
 * every encoder's output is; an incomplete file (libjpeg smooths its blocks),
 * a scan script libjpeg would warn about, more than 64 scans, or data after
 * EOI is FI_EUNSUPPORTED, and a scan libjpeg rejects (JERR_BAD_PROGRESSION)
 * FI_EINVAL.  The pixels are libjpeg-turbo's, bit for bit.  With flags 0 both
 * are fi_jpeg_info / fi_jpeg_decode_device.
 * fi_jpeg_info_ex (host only): also the stream's scan count and the number of
 * launch levels its scans are scheduled in (scans that share no component
 * over overlapping coefficient bands run in one launch); 1 and 1 for a
 * baseline stream; nscans / nlevels may be NULL.
 * fi_jpeg_decode_device_ex: a batch may mix baseline and progressive streams
 * (one upload, one IDCT and one colour launch for all).  Kernel time of the
 * progressive entropy decode: "k_jpeg_prog" in fi_kernel_stats
 * (fi_set_timing(1)). */
#define FI_JPEG_PROGRESSIVE 1u   /* also take SOF2 Huffman progressive streams */
int fi_jpeg_info_ex(const uint8_t *data, size_t len, uint32_t flags, int32_t *w, int32_t *h, int32_t *channels,
                    int32_t *nscans, int32_t *nlevels);
int fi_jpeg_decode_device_ex(fi_ctx *ctx, const uint8_t *const *data, const size_t *len, int32_t n,
                             uint8_t *const *dst, const int64_t *dst_stride, int32_t out_channels,
                             uint32_t flags, int32_t *status);
/* Views, opt-in: `-auto-orient` (ImageProcessor.php:78) and ExtractProcessor's
 * `-crop` applied by the decoder's colour stage, so an EXIF-rotated source or
 * an extract never exists unrotated or uncropped in device memory.  A view is
 * an EXIF orientation (1..8, what Pillow's ImageOps.exif_transpose applies;
 * 5..8 swap width and height) and a rectangle of the ORIENTED image; dst[i]
 * receives h rows of w pixels: bytes [0, w * channels) of each row, nothing
 * else of the buffer.  The pixels are those of the oriented, cropped host
 * decode, bit for bit (chroma upsampling reads across the rectangle's edge).
 * fi_jpeg_orientation (host only): the file's EXIF orientation as Pillow
 * 12.2's Image.getexif reads it, 1 when there is none; FI_EUNSUPPORTED where
 * Pillow's answer takes more than an IFD0 lookup (several Exif segments, an
 * XMP packet without an EXIF orientation, a tag of another type or count, a
 * malformed TIFF structure): decide on the host; FI_EINVAL without SOI.
 * fi_jpeg_decode_device_view: fi_jpeg_decode_device_ex with views[i] per
 * image (views NULL: exactly fi_jpeg_decode_device_ex, which ignores EXIF, as
 * does an image whose view is {1, 0, 0, 0, 0}).  Per image: orientation 0 on a
 * file fi_jpeg_orientation cannot tell is FI_EUNSUPPORTED; an orientation
 * outside 0..8, a negative origin, a non-positive size other than the
 * all-zero form, or a rectangle reaching outside the oriented image is
 * FI_EINVAL; the rest of the batch decodes.  Kernel time of the viewed images'
 * colour stage: "k_jpeg_color_view" in fi_kernel_stats (the others':
 * "k_jpeg_color"). */
typedef struct fi_jpeg_view {
  int32_t orientation;   /* 1..8: apply this EXIF orientation; 0: read it from the file */
  int32_t x, y, w, h;    /* rectangle of the oriented image; all 0: the whole image */
} fi_jpeg_view;
int fi_jpeg_orientation(const uint8_t *data, size_t len, int32_t *orientation);
int fi_jpeg_decode_device_view(fi_ctx *ctx, const uint8_t *const *data, const size_t *len, int32_t n,
                               uint8_t *const *dst, const int64_t *dst_stride, int32_t out_channels,
                               uint32_t flags, const fi_jpeg_view *views, int32_t *status);
/* Test hook (not a reference interface): the progressive entropy decode on
 * the CPU, through the block procedures the device kernel runs: info =
 * {components, bw[3], bh[3]} (block grid of each component), qt = each
 * component's quantisation table (natural order), coefs (NULL: sizes only) =
 * the int16 blocks in zigzag order, component after component. */
int fi_debug_jpeg_coefs_host(const uint8_t *data, size_t len, uint32_t flags, int32_t info[7], uint16_t qt[192],
                             int16_t *coefs, size_t coefs_cap);
/* GPU JPEG encode: the write step of `convert` (IM writes the output with
 * libjpeg at -quality) on the device, so the outputs of a device batch leave
 * it compressed.  Baseline, Annex K Huffman tables, one restart interval per
 * MCU row; the file is byte-identical with libjpeg-turbo's for the same
 * pixels and settings (Pillow: Image.save(buf, "JPEG", quality=q,
 * subsampling=s, restart_marker_rows=1)), and any baseline decoder reads it.
 * subsampling: 0 = 4:4:4, 2 = 4:2:0 (3-channel images; ignored for gray).
 * fi_jpeg_encode_bound (host only): an upper bound of the encoded size of any
 * w x h image with these settings -- header, worst-case Huffman codes, 0xFF
 * stuffing, restart markers, EOI; a worst case, many times a typical file.
 * fi_jpeg_encode_device: encodes n device-resident images src[i] (HWC u8
 * rows, 1 or 3 channels, any src_stride[i] >= w * channels, no alignment
 * assumed: fi_process_batch_device outputs go in as they are) into the host
 * buffers out[i] of out_cap[i] bytes and waits; out_len[i] = the encoded
 * size.  status[i]: FI_EUNSUPPORTED for 2 or 4 channels (alpha: fi_png_encode_device) or
 * another subsampling, FI_EINVAL for quality outside 1..100 or a side outside
 * 1..65535, FI_ENOMEM when out_cap[i] < out_len[i] (nothing is written past
 * out_cap[i]; out_len[i] is the size needed).  Returns the first failing
 * status; the other images are encoded.  Kernel times: "k_jpeg_fdct",
 * "k_jpeg_henc", "k_jpeg_pack" in fi_kernel_stats (fi_set_timing(1)). */
int fi_jpeg_encode_bound(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling,
                         size_t *bytes);
int fi_jpeg_encode_device(fi_ctx *ctx, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                          const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                          const int32_t *subsampling, int32_t n, uint8_t *const *out, const size_t *out_cap,
                          size_t *out_len, int32_t *status);
/* Progressive GPU JPEG encode (opt-in): flags = FI_JPEG_ENC_PROGRESSIVE writes
 * the file class flyimg ships -- SOF2, the scan script of libjpeg's
 * jpeg_simple_progression (10 scans for YCbCr, 6 for gray), Huffman tables
 * fitted to every scan, one restart interval per block row of every scan --
 * byte-identical with libjpeg-turbo's file for the same pixels and settings
 * (Pillow: Image.save(buf, "JPEG", quality=q, subsampling=s, progressive=True,
 * restart_marker_rows=1)).  Arguments, statuses and the out_cap rule are those
 * of fi_jpeg_encode_bound / fi_jpeg_encode_device; with flags 0 both calls are
 * those functions; any other flag bit is FI_EINVAL.  Kernel times:
 * "k_jpeg_fdct", "k_jpeg_pstat", "k_jpeg_ptab", "k_jpeg_pcode", "k_jpeg_ppack". */
#define FI_JPEG_ENC_PROGRESSIVE 1u
int fi_jpeg_encode_bound_ex(int32_t w, int32_t h, int32_t channels, int32_t quality, int32_t subsampling,
                            uint32_t flags, size_t *bytes);
int fi_jpeg_encode_device_ex(fi_ctx *ctx, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                             const int32_t *channels, const int64_t *src_stride, const int32_t *quality,
                             const int32_t *subsampling, int32_t n, uint8_t *const *out, const size_t *out_cap,
                             size_t *out_len, int32_t *status, uint32_t flags);
/* Test hook (not a reference interface): the progressive encoder's host model,
 * which runs the entropy coder, table builder and file layout the device
 * kernels run.  coefs: ncoefs quantised coefficients in the layout
 * fi_debug_jpeg_coefs_host hands out (zigzag int16 blocks, a plane per
 * component, whole MCUs).  Writes the file to out (out_cap bytes; *out_len =
 * its size, FI_ENOMEM when it does not fit) and *flushes = how often the
 * correction-bit buffer ended an EOB run inside a restart interval. */
int fi_debug_jpeg_prog_write_host(const int16_t *coefs, size_t ncoefs, int32_t w, int32_t h, int32_t channels,
                                  int32_t quality, int32_t subsampling, uint8_t *out, size_t out_cap,
                                  size_t *out_len, int32_t *flushes);
/* GPU PNG encode: the outputs JPEG cannot carry (2 or 4 channels: alpha) leave
 * the device as PNG files -- signature, IHDR (bit depth 8, colour type 0 / 4 /
 * 2 / 6 for 1 / 2 / 3 / 4 channels, no interlace), IDAT chunks, IEND, no
 * ancillary chunks.  The filtered stream (h rows of a filter-type byte + w *
 * channels bytes) is cut into bands of 32768 bytes; each band is deflated on
 * its own (greedy LZ77 inside the band; dynamic Huffman codes, the fixed codes
 * or stored blocks, whichever is smallest) into its own IDAT chunk; one zlib stream
 * (32 KiB window) runs across the chunks.  Lossless: any conforming decoder
 * returns the source pixels.
 * fi_png_encode_bound (host only): a true upper bound of the file size of any
 * w x h image -- every band stored: 51 bytes + the filtered stream + 17 bytes
 * per band; callers size buffers to it.
 * fi_png_encode_device: encodes n device-resident images src[i] (HWC u8 rows,
 * 1..4 channels, any src_stride[i] >= w * channels, no alignment assumed) into
 * the host buffers out[i] of out_cap[i] bytes and waits; out_len[i] = the
 * encoded size.  filter[i]: -1 = per row the filter type (0..4) with the
 * lowest sum of min(x, 256 - x) over its filtered bytes, ties to the lower
 * type; 0..4 = that type on every row; filter == NULL: -1 for every image.
 * status[i]: FI_EINVAL for other channel counts, a side outside 1..65535 or a
 * bad filter value, FI_EUNSUPPORTED when the filtered stream h * (w * channels
 * + 1) exceeds 2^31 - 1 bytes, FI_ENOMEM when out_cap[i] < out_len[i] (nothing
 * is written past out_cap[i]; out_len[i] is the size needed).  Returns the
 * first failing status; the other images are encoded.  Kernel times:
 * "k_png_filter", "k_png_lz", "k_png_codes", "k_png_emit", "k_png_pack" in
 * fi_kernel_stats (fi_set_timing(1)). */
int fi_png_encode_bound(int32_t w, int32_t h, int32_t channels, size_t *bytes);
int fi_png_encode_device(fi_ctx *ctx, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                         const int32_t *channels, const int64_t *src_stride, const int32_t *filter, int32_t n,
                         uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status);

/* GPU lossless WebP encode (opt-in): RIFF / WEBP / VP8L files without a VP8X
 * chunk or metadata.  1 / 2 / 3 / 4 channels are gray / gray + alpha / RGB /
 * RGBA (gray replicates into R, G and B; alpha_is_used is set for 2 and 4).
 * The file carries a subtract-green transform, a predictor transform with one
 * mode per 16 x 16 block, backward references inside bands of 8192 pixels
 * (plain distance codes, no colour cache) and one Huffman group.  Lossless:
 * any decoder returns the source pixels, RGB under alpha 0 included.
 * fi_webp_encode_bound (host only): a true upper bound of the file size of
 * any w x h image: the encoder's fallback form (no predictor, no references,
 * flat 8-bit codes for every channel that varies), w * h * channels bytes plus
 * a constant header below 1 KiB; the encoder prices both forms and writes the
 * smaller.
 * fi_webp_encode_device: encodes n device-resident images src[i] (HWC u8
 * rows, any src_stride[i] >= w * channels, no alignment assumed) into the host
 * buffers out[i] of out_cap[i] bytes and waits; out_len[i] = the encoded size.
 * predictor[i]: -1 = per block the mode (0..13) with the lowest sum of min(x,
 * 256 - x) over its residual bytes, ties to the lower mode; 0..13 = that mode
 * on every block; predictor == NULL: -1 for every image.  status[i]: FI_EINVAL
 * for other channel counts, a side below 1 or a bad predictor, FI_EUNSUPPORTED
 * for a side above 16384, FI_ENOMEM when out_cap[i] < out_len[i] (nothing is
 * written past out_cap[i]; out_len[i] is the size needed).  Returns the first
 * failing status; the other images are encoded.  FI_EDEVICE if what a kernel
 * emitted differs from what was priced.  Kernel times: "k_webp_pred",
 * "k_webp_lz", "k_webp_codes", "k_webp_emit", "k_webp_pack" in fi_kernel_stats
 * (fi_set_timing(1)).
 * fi_debug_webp_encode_host (no GPU): the same inline code on the CPU; its
 * file is the specification of the device's file, byte for byte. */
int fi_webp_encode_bound(int32_t w, int32_t h, int32_t channels, size_t *bytes);
int fi_webp_encode_device(fi_ctx *ctx, const uint8_t *const *src, const int32_t *w, const int32_t *h,
                          const int32_t *channels, const int64_t *src_stride, const int32_t *predictor, int32_t n,
                          uint8_t *const *out, const size_t *out_cap, size_t *out_len, int32_t *status);
int fi_debug_webp_encode_host(const uint8_t *src, int32_t w, int32_t h, int32_t channels, int64_t src_stride,
                              int32_t predictor, uint8_t *out, size_t out_cap, size_t *out_len);

/* GPU PNG decode (opt-in): 8-bit, non-interlaced PNG sources of colour type
 * 0 / 2 / 4 / 6, or 3 with a PLTE and an optional tRNS, decoded into device
 * memory bit for bit as Pillow reads them: one 64-lane workgroup inflates an
 * image (a serial chain; the batch supplies the parallelism), a second kernel
 * checks the Adler-32 and a third undoes the row filters as a wavefront.
 * fi_png_info (host only): FI_OK only for files the device path reproduces
 * exactly; channels = the natural count (1 / 2 / 3 / 4 for colour type 0 / 4 /
 * 2 / 6, palette 3, palette with tRNS 4); color_type and meta may be NULL.
 * FI_EUNSUPPORTED = decode this one on the host: bit depth 1, 2, 4 or 16, Adam7
 * interlace, tRNS on colour type 0 or 2, an acTL chunk, a filtered stream h *
 * (w * c + 1) above 2^31 - 1 bytes, a CRC mismatch on IHDR, PLTE, tRNS, IDAT or
 * IEND (ancillary chunks are not checked), a zlib header with FDICT or a
 * method or window zlib would refuse, a missing IEND, bytes after IEND.
 * FI_EINVAL: no PNG signature or a broken IHDR.  meta gets FI_PNG_META_ORIENT
 * when the file carries, anywhere, an eXIf chunk or a tEXt / zTXt / iTXt chunk
 * with the keyword "Raw profile type exif", "Raw profile type APP1" or
 * "XML:com.adobe.xmp": the library does not interpret them, the caller keeps
 * such files on the host.
 * fi_png_decode_device: decodes n files from host memory into the device
 * buffers dst[i] (HWC rows of dst_stride[i] bytes, no alignment assumed) and
 * waits.  out_channels[i] (or a NULL array: 0): 0 = the natural count; 3 = RGB,
 * gray replicated and palette expanded, FI_EINVAL for a source with alpha; 4 =
 * RGBA, alpha 255 where the source has none.  A palette index beyond PLTE
 * gives (0, 0, 0) with alpha 255, one beyond tRNS alpha 255 (Pillow's
 * convert).  status[i]: what fi_png_info says of the file, or FI_EINVAL where
 * the device finds a corrupt deflate stream (zlib's validity rules), a filter
 * byte above 4, a stream that does not inflate to exactly h * (w * c + 1) bytes
 * or an Adler-32 mismatch (the buffer's contents are then undefined).  Returns
 * the first failing status; the other images are decoded.  Kernel times:
 * "k_png_inflate", "k_png_adler", "k_png_unfilter" in fi_kernel_stats
 * (fi_set_timing(1)). */
#define FI_PNG_META_ORIENT 1   /* a chunk Pillow's exif_transpose could take an orientation from */
int fi_png_info(const uint8_t *data, size_t len, int32_t *w, int32_t *h,
                int32_t *channels, int32_t *color_type, int32_t *meta);
int fi_png_decode_device(fi_ctx *ctx, const uint8_t *const *data, const size_t *len, int32_t n,
                         uint8_t *const *dst, const int64_t *dst_stride,
                         const int32_t *out_channels, int32_t *status);

/* Test hook (not a reference interface): the skin / saturation table k_sc_fz
 * reads (2^24 entries, index (r << 16) | (g << 8) | b, value skin | sat << 8)
 * built for `params` (NULL: defaults) and copied to out, so a test can compare
 * every colour with the oracle's detect_skin / detect_saturation. */
int fi_debug_skinsat(fi_ctx *ctx, const fi_smartcrop_params *params, uint16_t *out);

/* Test hook (not a reference interface): the batch planner alone, on the
 * host -- no device: the image pointers are planned, never dereferenced --
 * over `iters` passes of the n images; ms[0..6] += per-stage host
 * milliseconds (images, smartcrop, workspace, vm + vr tiles, of which vr, hv
 * tiles, blob).  One host-only context persists across calls (its caches, as
 * a serving context's): (NULL, 0, ...) drops it, (NULL, 1, ...) clears its
 * statistics, (NULL, 2, 0, ms) reads the resample plan's counters since:
 * ms[0] images planned onto k_rs_vr, ms[1] vertical-first images, ms[2]
 * k_rs_vr launches; (NULL, 3, 0, ms) reads what the last planned batch
 * emitted: ms[0], ms[1] the low and high 32 bits of a 64-bit FNV-1a digest of
 * the packed upload blob followed by the workspace size (eight bytes, low
 * first), ms[2] the blob's bytes, ms[3..5] the k_rs_vm, k_rs_vr and k_rs_hv
 * tiles, ms[6] the smartcrop items. */
int fi_debug_host_plan(const fi_image *imgs, int32_t n, int32_t iters, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* FLYIMG_HIP_H */
