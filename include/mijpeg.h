/*
 * mijpeg.h — C ABI of libmijpeg.so: the MI355X (gfx950) replacement for the per-MCU hot path of
 * tbpaolini/PyJpegDecoder.
 *
 * The reference is one Python class with no FFI; the seam this library plugs into is method level
 * (SURVEY.md §8b).  Each entry point names the reference code it replaces (all citations are into
 * /root/reference/jpeg_decoder.py):
 *
 *   mj_plan_create / mj_plan_execute    JpegDecoder.baseline_dct_scan       :697-906   (Huffman decode,
 *                                       + InverseDCT.__call__               :1561-1573  dequantise, IDCT,
 *                                       + ResizeGrid.__call__               :1588-1626  upsample,
 *                                       + end_of_image crop / YCbCr_to_RGB  :1373-1386, :1683-1700  colour)
 *   (progressive batches: stage 1 is JpegDecoder.progressive_dct_scan :908-1304, one launch per scan ordinal,
 *    stage 2 is the final pass :1306-1362)
 *   mj_decode_baseline_batch            the same, one call (create + execute + sync + read back)
 *   mj_idct_batch                       the same minus the entropy decoder: caller supplies the zig-zag
 *                                       coefficients seen at :869 (BASELINE.json configs[1], "host Huffman")
 *
 * Inputs are exactly what start_of_scan (:505-650) has prepared when it calls the scan decoder: the
 * file bytes, the offset of the first entropy-coded byte, per-component table selectors, the DHT
 * BITS/HUFFVAL lists, the DQT tables, the restart interval and the MCU geometry — plus the offsets of
 * the restart segments, because stage 1 decodes one restart segment per wavefront.
 *
 * Conventions
 *   - plain C, no torch / numpy types; every pointer is either host or device memory as said by the
 *     accompanying MJ_MEM_* flag; the caller owns every buffer it passes and the library never frees it.
 *   - every function returns MJ_OK (0) or a negative MJ_ERR_*; mj_last_error() gives the text.
 *   - per-image decode outcomes go to status[] (MJ_ST_*), they are not API errors.
 *   - one context per GPU per host thread; a context is not thread safe.
 *   - mj_plan_execute is asynchronous on the plan's stream; everything else is synchronous at return.
 *   - there is NO CPU fallback anywhere in this library.
 */
#ifndef MIJPEG_H
#define MIJPEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJ_VERSION 2

/* API results */
#define MJ_OK               0
#define MJ_ERR_INVALID     (-1)   /* bad argument / inconsistent description */
#define MJ_ERR_HIP         (-2)   /* a HIP runtime call failed (no GPU, OOM, launch failure, ...) */
#define MJ_ERR_UNSUPPORTED (-3)   /* sampling layout / feature outside the MI355X path */

/* per-image status */
#define MJ_ST_OK          0
#define MJ_ST_BAD_CODE    1   /* no Huffman code within 16 bits: the reference raises CorruptedJpeg (:718-719) */
#define MJ_ST_OVERRUN     2   /* a segment needed more bits than it holds (reference: IndexError / garbage)     */
#define MJ_ST_DESYNC      3   /* a segment's MCUs end before its next RSTn: the reference's count-driven restart
                                 (:667-669, :898-900) would lose synchronisation here                           */

#define MJ_ST_TAIL        4   /* MJ_FLAG_GPU_SEGMENT only: the scan is not followed by EOI (more scans, DNL, ...): the
                                 host-side marker loop (:78-110) has to segment this file                          */
#define MJ_ST_UNCONVERGED 5   /* long restart segments (files without DRI) are cut into pieces whose decoder states are found
                                 by a fixed number of synchronisation rounds on the device; this image's states had not
                                 settled when the rounds were over (a pathological or crafted stream): nothing is wrong
                                 with the file — decode it again in a plan created with MJ_FLAG_NO_SYNC                */

#define MJ_ST_INTERNAL    6   /* a wavefront of a fused launch gave up waiting for its workgroup's decoder wavefronts (a bound on
                                 what is otherwise a spin loop: cannot happen; the image's pixels are not valid)        */

/* memory spaces */
#define MJ_MEM_NONE   0
#define MJ_MEM_HOST   1
#define MJ_MEM_DEVICE 2

/* pixel layouts of the RGB / grey output */
#define MJ_LAYOUT_XMAJOR   0   /* reference image_array: (W, H, C), x-major */
#define MJ_LAYOUT_ROWMAJOR 1   /* (H, W, C) */
#define MJ_LAYOUT_PLANAR_XMAJOR   2   /* (C, W, H): the components of the array the reference leaves at :1373-1386 as
                                         three planes per image (one for greyscale), image after image              */
#define MJ_LAYOUT_PLANAR_ROWMAJOR 3   /* (C, H, W) */

/* flags of mj_batch.flags */
#define MJ_FLAG_KEEP_COEF    1u   /* keep the zig-zag coefficient array (:869 seam) readable after execute */
#define MJ_FLAG_KEEP_PLANES  2u   /* also produce the cropped int16 YCbCr planes (:1373 seam)               */
#define MJ_FLAG_KEEP_IDCT    4u   /* also produce the per-block IDCT output (:872 return value)             */
#define MJ_FLAG_EXACT_ONLY   8u   /* stage 2: use only the exact-order fp64 summation (no fast path)        */
#define MJ_FLAG_SPEC_REFINE 16u   /* progressive AC refinement per ITU-T T.81 G.1.2.3 (move negative values away
                                     from zero) instead of the reference's `|=` on two's complement (:1114)  */

#define MJ_FLAG_GPU_SEGMENT 32u  /* baseline batches: find the RSTn markers and the end of the scan on the GPU (what
                                     _parse.py's find_entropy_end / find_restart_segments do on the host).  Every
                                     image then has n_segments = 1 and seg_begin/seg_end = first entropy-coded byte /
                                     any bound at or behind the end of the scan (e.g. the end of the file); the blob
                                     must be 16-byte aligned with 16 readable bytes behind blob_len.  (The marker scan
                                     and stage 0 read it inside [seg_begin, seg_end) + 16 bytes and the lane forms of
                                     stage 1 read stage 0's stream, so the 512-byte rule of MJ_MEM_DEVICE blobs below
                                     does not apply; a plan that takes the wave form of stage 1 — small batches,
                                     unusual sampling layouts — reads the blob itself, further ahead, and works on a
                                     padded copy of it made at plan creation when the blob lacks those 512 bytes.)  */

#define MJ_FLAG_NO_SYNC     64u  /* never cut restart segments into synchronised pieces: one serial walk per segment (the
                                     fallback for images that came back MJ_ST_UNCONVERGED)                          */

typedef struct mj_context mj_context;
typedef struct mj_plan mj_plan;

/* One DHT table (:293-324): BITS[16] then HUFFVAL. */
typedef struct {
    uint8_t bits[16];
    uint8_t vals[256];
} mj_huff_spec;

/* One image = one interleaved baseline scan (or a single-component greyscale scan). */
typedef struct {
    int32_t width, height;        /* image_width, image_height (:160-169)                                    */
    int32_t ncomp;                /* 1 or 3 (:177-183)                                                        */
    int32_t hs[3], vs[3];         /* sampling factors in frame order Y, Cb, Cr (:205-207)                     */
    int32_t qt_sel[3];            /* index into mj_batch.qt of each component's table (:212)                  */
    int32_t dc_sel[3], ac_sel[3]; /* index into mj_batch.huff of each component's DC / AC table (:543-544)    */
    int32_t restart_interval;     /* MCUs per restart segment, 0 = none (:476)                                */
    int32_t mcu_count_h, mcu_count_v; /* (:609-619)                                                           */
    int32_t n_segments;           /* number of restart segments = ceil(mcu_count / restart_interval) or 1     */
    int64_t first_segment;        /* index of this image's first entry in seg_begin / seg_end                 */
} mj_image_desc;

/* One SOS of an image that is decoded scan by scan: what start_of_scan (:505-650) hands to progressive_dct_scan
 * (:908) for a progressive (SOF2) image, or to baseline_dct_scan (:697) for a baseline image with one scan per
 * component (then ss = 0, se = 63, ah = al = 0, n_comp = 1, no component subsampled).
 * Scans must be listed image by image, in file order. */
typedef struct {
    int32_t image;                /* index into mj_batch.images                                               */
    int32_t n_comp;               /* components in the scan (:530)                                            */
    int32_t comp[3];              /* their positions in the frame (0 = Y, 1 = Cb, 2 = Cr)                     */
    int32_t dc_sel[3], ac_sel[3]; /* per scan component: index into mj_batch.huff (:543-544)                  */
    int32_t ss, se, ah, al;       /* spectral selection, successive approximation (:559-562)                  */
    int32_t restart_interval;     /* value in force for this scan (:501-502)                                  */
    int32_t mcu_count_h, mcu_count_v; /* of this scan (:609-621): interleaved MCUs or the component's 8x8 blocks */
    int32_t n_segments;           /* restart segments of this scan                                            */
    int64_t first_segment;        /* index of the scan's first entry in seg_begin / seg_end                   */
} mj_scan_desc;

typedef struct {
    int32_t n_images;
    const mj_image_desc *images;          /* host */

    const uint8_t *blob;                  /* the file bytes of all images, back to back or not              */
    int64_t blob_len;
    int32_t blob_mem;                     /* MJ_MEM_HOST or MJ_MEM_DEVICE (device: 4-byte aligned, must stay valid for the
                                             plan, and blob_len must include at least 512 readable bytes behind the last
                                             segment's end: the stage-1 bit readers fetch ahead; checked at plan creation.
                                             Host blobs are uploaded with that slack added.) */

    int64_t n_segments;                   /* total entries of the two arrays below                          */
    const int64_t *seg_begin;             /* host: blob offset of the first entropy byte of each segment; list them in
                                             ascending blob order (any order works, but only ordered batches take the
                                             lane-parallel stage 1)                                          */
    const int64_t *seg_end;               /* host: blob offset one past its last entropy byte (= position of
                                             the RSTn / next marker)                                         */
    int32_t n_huff;
    const mj_huff_spec *huff;             /* host */
    int32_t n_qt;
    const uint16_t *qt;                   /* host: n_qt tables of 64 entries in zig-zag (file) order (:454)  */

    int32_t layout;                       /* MJ_LAYOUT_*                                                     */
    uint32_t flags;                       /* MJ_FLAG_*                                                       */

    int32_t n_scans;                      /* 0 = single-scan baseline batch; > 0 = scan-by-scan batch: every image is
                                             progressive (SOF2) or non-interleaved baseline                    */
    const mj_scan_desc *scans;            /* host; the images' own n_segments / first_segment / table selectors
                                             are ignored in a scan-by-scan batch                              */
} mj_batch;

/* Sizes and per-image offsets of a plan's outputs (all outputs are packed image after image). */
typedef struct {
    int64_t total_blocks;                 /* coefficient blocks in the batch                                 */
    int64_t total_mcus;
    int64_t total_pixels;                 /* sum of width*height                                              */
    int64_t rgb_bytes;                    /* sum of width*height*ncomp                                        */
    int64_t entropy_bytes;                /* sum of segment lengths                                           */
} mj_plan_info;

/* ---- context ------------------------------------------------------------------------------------- */
int mj_create(int device_id, mj_context **out);
void mj_destroy(mj_context *ctx);
const char *mj_last_error(const mj_context *ctx);   /* ctx may be NULL: error of the failed mj_create */
int mj_version(void);
/* Make the context's stream wait for a hipEvent_t (passed as void*) recorded elsewhere — e.g. behind the upload of a
 * batch's files on a copy stream — before anything queued on it afterwards runs. */
int mj_context_wait_event(mj_context *ctx, void *hip_event);

/* ---- plan: upload once, execute many times (bench.py times mj_plan_execute only) ------------------ */
/* What a plan's output is to be, beyond the batch itself: every feature is one field of mj_plan_request, specified where the
 * field is declared below.  A zeroed request asks for nothing — the plain plan: every image whole, as stored, in the files' own
 * components, at its own size, packed image after image — and every field whose value is its DEFAULT (named with the field)
 * gives exactly the plan of the request without it: the library turns such a field into its absence before anything is made,
 * so the same code makes the plan and the same kernels run it.  All arrays are host memory with batch->n_images entries (in a
 * request with views, the per-output ones — slots, output->mirror, places, affine, perspective, colour — with n_views), read during the call only.
 *
 * Order of operations on an image, whichever fields are set: decode (only what the windows need) -> mode -> orientation ->
 * affine transform -> window -> resize with the filter (to the place's size, onto the canvas) -> colour operations
 * (the `colour` field) -> mirror -> the output's element type (-> erase: not a field, mj_plan_set_erase).  In Pillow's terms the result is
 * exif_transpose(img.convert(mode))[.transform(img.size, AFFINE or PERSPECTIVE, a, resample, fillcolor)].crop(window).resize(size, filter) —
 * with reducing_gap, Pillow's argument of that name to that resize.
 *
 * Refusals common to all fields: MJ_ERR_INVALID with a message in mj_last_error — naming the image where there is one — for a
 * value outside what the field takes; MJ_FLAG_KEEP_PLANES / MJ_FLAG_KEEP_IDCT together with ANY field that changes the plan
 * (the seam outputs are whole images in stored order, in the files' components, at the files' sizes; a window plan refuses
 * MJ_FLAG_KEEP_COEF too).  Checked in this order, the first fault reported: filter, mode, orientations, output — these before
 * the context is looked at, so that a bad description is diagnosed without a GPU (the message is then mj_last_error(NULL)'s) —,
 * ctx / batch / out, the size, the KEEP flags, affine (filter, array, reducing_gap), views, affine's matrices, slots, places, windows, then the batch itself.  (reducing_gap's value is checked
 * with the first four.) */
typedef struct {
    int32_t x, y, width, height;
} mj_roi;
#define MJ_MODE_NATIVE 0
#define MJ_MODE_L      1
#define MJ_MODE_RGB    3
#define MJ_DTYPE_U8   0
#define MJ_DTYPE_F16  1
#define MJ_DTYPE_BF16 2
#define MJ_DTYPE_F32  3
typedef struct {
    int32_t dtype;              /* MJ_DTYPE_* */
    int32_t normalize;          /* 0: value / 255 (float types); 1: (value / 255 - mean[c]) / std[c] */
    float mean[3], std[3];
    const uint8_t *mirror;      /* NULL, or one flag per image of the batch */
} mj_output_desc;
#define MJ_FILTER_BILINEAR 0
#define MJ_FILTER_BOX      1
#define MJ_FILTER_HAMMING  2
#define MJ_FILTER_BICUBIC  3
#define MJ_FILTER_LANCZOS  4
typedef struct {
    int32_t width, height;
    int32_t x, y;
} mj_place;
typedef struct {
    int32_t image;              /* index into the batch */
    mj_roi window;              /* of the oriented image, after the mode; all zero: the whole (oriented) image */
} mj_view;
/* One output's affine transform (mj_plan_request.affine): the matrix maps OUTPUT pixel centres to source coordinates, as the
 * `data` of Pillow's Image.transform(size, Image.AFFINE, data) and torchvision's inverse matrix do.  All six 0: no transform. */
typedef struct {
    double a[6];
} mj_affine;
#define MJ_AFFINE_NEAREST  1
#define MJ_AFFINE_BILINEAR 2
#define MJ_AFFINE_BICUBIC  3
/* One output's perspective transform (mj_plan_request.perspective): the eight coefficients map OUTPUT pixel
 * centres to source coordinates, as the `data` of Pillow's Image.transform(size, Image.PERSPECTIVE, data) and torchvision's
 * _get_perspective_coeffs do.  All eight 0: no transform. */
typedef struct {
    double a[8];
} mj_perspective;
/* One output's colour operations (mj_plan_request.colour) */
#define MJ_COLOUR_MAX_OPS 4
#define MJ_COLOUR_BRIGHTNESS   1
#define MJ_COLOUR_COLOR        2
#define MJ_COLOUR_CONTRAST     3
#define MJ_COLOUR_SHARPNESS    4
#define MJ_COLOUR_POSTERIZE    5
#define MJ_COLOUR_SOLARIZE     6
#define MJ_COLOUR_AUTOCONTRAST 7
#define MJ_COLOUR_EQUALIZE     8
#define MJ_COLOUR_INVERT       9
#define MJ_COLOUR_GAUSSIAN_BLUR 10
#define MJ_COLOUR_BOX_BLUR     11
#define MJ_COLOUR_ADJUST_HUE   13      /* (12 is no kind) */
typedef struct {
    int32_t kind;               /* MJ_COLOUR_* */
    float value;                /* the factor, bits, threshold or radius; ignored by autocontrast, equalize and invert */
} mj_colour_op;
typedef struct {
    int32_t n;                  /* 0..MJ_COLOUR_MAX_OPS ops, applied in order */
    mj_colour_op op[MJ_COLOUR_MAX_OPS];
} mj_colour_chain;
typedef struct {
    /* Region of interest.  DEFAULT NULL: whole images.  Else the output for image i is the window rois[i] of the image — x along
     * image_width, y along image_height — and nothing else.  Window i in the plan's layout:
     *   MJ_LAYOUT_XMAJOR    full[x:x+width, y:y+height]      of the (W, H, C) image
     *   MJ_LAYOUT_ROWMAJOR  full_rm[y:y+height, x:x+width]   of the (H, W, C) image
     *   planar layouts      the same windows, one component after another (greyscale: one component)
     * Outputs are packed window after window: mj_plan_info.total_pixels / rgb_bytes are sums over the windows and
     * mj_plan_image_offsets' rgb_off lies in that packing.  A pixel depends only on the MCU that covers it (the reference
     * upsamples inside the MCU), so a window is bit-exact: the whole image's decode, sliced.
     * Only the restart segments that hold an MCU of the window are decoded (host-segmented baseline batches list only those;
     * MJ_FLAG_GPU_SEGMENT batches gather them after the marker scan).  Files without restart markers, progressive and
     * non-interleaved batches decode every scan whole; stage 2 runs on the windows' MCUs only.
     * Status: status[i] reports what the DECODED segments found — a damaged restart segment outside the window does not fail
     * the image (the marker scan of MJ_FLAG_GPU_SEGMENT still checks every marker of the image).
     * A plan with windows — windows that are the whole images included — never takes the fused launch (MJ_FORM_FUSED); a
     * request without windows makes the plain plan, which may.  With orientations the windows are windows of the ORIENTED
     * images; the library maps them to the stored images (orient_model.stored_window) and the plan is a window plan of those.
     * MJ_ERR_INVALID: an empty window or one not inside its (oriented) image. */
    const mj_roi *rois;
    /* EXIF orientation, one byte 1..8 per image.  DEFAULT NULL, or all of them 1: as stored.  Else the outputs are the images
     * as their Orientation tag says they are to be shown — exactly Pillow's ImageOps.exif_transpose (tools/orient_model.py): 1 as
     * stored, 2 left-right flip, 3 rotated by 180, 4 top-bottom flip, 5 transposed, 6 ROTATE_270, 7 transverse, 8 ROTATE_90;
     * 5..8 exchange width and height.
     *   without a size   outputs packed image after image as the plain plan's are — an image keeps its offset
     *     (mj_plan_image_offsets) and its size in bytes; its shape in the plan's layout is the oriented one.  Stage 2 writes into a
     *     plan-owned buffer in stored order and one more launch (csrc/orient.hip) writes every image oriented into the caller's
     *     output; mj_plan_fill_source / mj_plan_time_resize work on that buffer / launch.
     *   with a size      element by element Pillow's resize of the oriented pixels, inside the one resize launch — no extra pass
     *     over memory.  output->mirror applies after the orientation.  All images of such a plan either exchange width and height
     *     (5..8) or do not: MJ_ERR_UNSUPPORTED naming the first image that differs from image 0 otherwise (two plans into one
     *     array, with slots). */
    const uint8_t *orientations;
    /* Output colour mode, MJ_MODE_*.  DEFAULT MJ_MODE_NATIVE (0), or the mode that is the batch's own component count (its first
     * image's): the files' own components.  Else the outputs have the components the CALLER names — Pillow's img.convert(mode)
     * (tools/mode_model.py) of the decoded pixels, before everything else.
     *   MJ_MODE_L       one component.  A colour image's pixel becomes L = (19595 R + 38470 G + 7471 B + 32768) >> 16 of the RGB
     *                   bytes a plan without the mode gives (not the file's Y plane: the colour conversion's rounding lies in between)
     *   MJ_MODE_RGB     three components.  A greyscale image's byte goes into all three
     * A plan that converts: mj_plan_info.rgb_bytes, the slots' offsets and mj_plan_image_offsets' rgb_off count OUTPUT components;
     * output->mean / std are read for the mode's components (a greyscale file under MJ_MODE_RGB gets three tables applied to its
     * one byte).
     *   without a size   outputs packed image after image, every image width * height * <the mode's components> bytes.  The one
     *     extra launch of an oriented plan (csrc/orient.hip) converts on its way; a plan that converts has that launch for upright
     *     images too.
     *   with a size      the resize launch converts: colour to L where the source is read, in front of the width pass (resize-then-
     *     convert is another result), grey to RGB where the output is stored; both passes run on one component, and no extra pass
     *     over memory is made in either direction.
     * mj_host_convert_mode is the host twin of the kernels' conversion. */
    int32_t mode;
    /* Decode to a fixed size.  DEFAULT both 0: outputs at the files' own sizes.  Else, both 1..65535, the output is every image —
     * or window — resized to out_width x out_height: ONE dense array of n_slots images in the plan's layout,
     *   MJ_LAYOUT_XMAJOR (n_slots, out_width, out_height, C)    MJ_LAYOUT_PLANAR_XMAJOR   (n_slots, C, out_width, out_height)
     *   MJ_LAYOUT_ROWMAJOR (n_slots, out_height, out_width, C)  MJ_LAYOUT_PLANAR_ROWMAJOR (n_slots, C, out_height, out_width)
     * (C = the output's component count), and mj_plan_info.rgb_bytes = n_slots * out_width * out_height * C is that array's size.
     * The resize is Pillow's Image.resize((out_width, out_height), filter) of the row-major image, byte for byte: integer taps
     * from the filter's weights, whose support grows with the scale when shrinking (antialiased), along the width first, then the
     * height, with an 8-bit image in between (mj_host_resize_table; csrc/resize.hip).  mj_plan_execute runs stage 1, stage 2 — into
     * a buffer of the files' own sizes that the plan owns — and the resize as its last launch; mj_plan_execute_stage2 includes it.
     * slots, output, filter, places and fill say more about this array: set without a size they are MJ_ERR_INVALID ("... needs a
     * size").  MJ_ERR_INVALID also: one of the two 0, or either outside 1..65535.  MJ_ERR_UNSUPPORTED: a shrink so strong that one
     * pixel's taps do not fit a workgroup's LDS, or more output tiles than one launch takes (about 6.8e10: split the batch). */
    int32_t out_width, out_height;
    /* Affine transform — rotate, shear, translate, scale — of the whole oriented image, in front of the window and the resize
     * (tools/affine_model.py).  DEFAULT NULL — also every matrix all zero: no transform.  Else, with a size, `affine` holds one
     * mj_affine per OUTPUT (n_views entries in a request with views, else n_images), transform_filter is the resample filter
     * MJ_AFFINE_* and transform_fill (the request's last member) the fill byte of output components 0, 1, 2: output k is, bit for bit,
     *   exif_transpose(img.convert(mode)).transform(img.size, Image.AFFINE, affine[k].a, resample, fillcolor=fill)
     *       .crop(window_k).resize(target_k, filter)
     * on the canvas, mirrored if mirror[k], through the output table.  The transformed image has the oriented image's size
     * (Pillow's expand=False); rois / views' windows, places and the size refer to it.  An output whose matrix is all zero is the
     * output of the request without the field.  Pillow's rules, restated (w x h: the oriented image; (x, y): a pixel of it):
     *   MJ_AFFINE_BILINEAR / MJ_AFFINE_BICUBIC   xin = a0 (x + 0.5) + a1 (y + 0.5) + a2, yin = a3 (x + 0.5) + a4 (y + 0.5) + a5 in
     *       doubles, every operation rounded on its own; fill where xin < 0, xin >= w, yin < 0 or yin >= h; else 2 x 2 / 4 x 4 taps
     *       around (xin - 0.5, yin - 0.5) with clipped columns, a row outside the image taking the value of the row before it,
     *       interpolated in doubles along x, then y; bilinear truncates, bicubic clips to 0..255 and truncates
     *   MJ_AFFINE_NEAREST with a1 == 0 and a3 == 0   the source column of output column x is found by ACCUMULATION: xo = a2 + a0 * 0.5,
     *       then per column (xo < 0 ? -1 : (int)xo) and xo += a0; rows likewise with a5 + a4 * 0.5 and a4 (host-built tables)
     *   MJ_AFFINE_NEAREST otherwise   16.16 fixed point: FIX(v) = floor(v * 65536 + 0.5); A2 = FIX(a2 + a0 * 0.5 + a1 * 0.5),
     *       A5 = FIX(a5 + a3 * 0.5 + a4 * 0.5); xi = (int32)(A2 + x FIX(a0) + y FIX(a1)) >> 16 in wrapping 32-bit arithmetic, yi likewise
     * A pixel whose source lies outside the image is fill.  mj_host_affine is the host twin.
     * The plan is the PLAIN plan of its images, as a plan with views is: images decoded whole and once, the fused launch wherever
     * the plain plan takes it; rois with the field become per-output records, not a window plan (a rotated window needs source
     * pixels outside itself).  One more launch (csrc/affine.hip) between stage 2 and the resize launch writes, for every output,
     * ONLY its window of the transformed image — evaluated at the window's absolute coordinates —, densely, in the output's
     * components, into a second plan-owned buffer the resize launch reads as upright images.  Orientation costs no pass (the
     * kernel maps oriented to stored coordinates where it fetches); MJ_MODE_L converts every fetched tap before interpolating.
     * MJ_ERR_INVALID, naming the output: set without a size ("affine needs a size"); a transform_filter that is none of
     * MJ_AFFINE_*; a matrix entry that is not finite; an image with a side of 32768 or more; a matrix under which a corner pixel of the
     * output has a source coordinate of magnitude 32768 or more (Pillow leaves its defined arithmetic there), and, under
     * MJ_AFFINE_NEAREST, the same for the corner values Pillow's check_fixed tests; together with reducing_gap ("not yet": the
     * reduce would have to read the new buffer).  Left for later as well: expand=True, use without a size.
     * transform_filter and transform_fill serve whichever of `affine` and `perspective` is set: either of them set while both
     * arrays are NULL is MJ_ERR_INVALID, and so are both arrays in one request ("affine and perspective do not go together").
     * A perspective transform has coefficients and rules of its own: see `perspective` below. */
    int32_t transform_filter;
    const mj_affine *affine;
    /* Perspective transform.  DEFAULT NULL — also every entry all zero: no transform.  Else, with a size, `perspective` holds one
     * entry per OUTPUT (n_views entries in a request with views, else n_images), with transform_filter and transform_fill as under
     * `affine`.  Everything mj_plan_request.affine says of its place in the order of
     * operations, of the plan (the PLAIN plan of its images; rois become per-output records), of the one more launch (csrc/affine.hip:
     * k_perspective, the affine launch's geometry), of the second plan-owned buffer, of orientation and MJ_MODE_L holds here: output k
     * is, bit for bit,
     *   exif_transpose(img.convert(mode)).transform(img.size, Image.PERSPECTIVE, perspective[k].a, resample, fillcolor=fill)
     *       .crop(window_k).resize(target_k, filter)
     * and an output whose coefficients are all zero is the output of the request without the field; where ALL are, the request is that
     * request (mj_debug_normalise_request clears the field).  Pillow's rules (Geometry.c: perspective_transform,
     * ImagingGenericTransform), restated in tools/perspective_model.py — (X, Y): a pixel of the transformed image in ABSOLUTE
     * coordinates (a window is the transform evaluated at the window's coordinates); w x h: the oriented image; every double
     * operation rounded on its own, in this order:
     *   xc = X + 0.5, yc = Y + 0.5;  d = a6 xc + a7 yc + 1;  xin = (a0 xc + a1 yc + a2) / d;  yin = (a3 xc + a4 yc + a5) / d
     *   the divisions are IEEE double divisions.  The pixel is INSIDE iff xin >= 0 && xin < w && yin >= 0 && yin < h — NaN and +-inf
     *   are outside —, and an outside pixel is fill
     *   MJ_AFFINE_NEAREST    source pixel ((int)xin, (int)yin): no 0.5 shift, no fixed point, no tables
     *   MJ_AFFINE_BILINEAR / MJ_AFFINE_BICUBIC   the 2 x 2 / 4 x 4 taps around (xin - 0.5, yin - 0.5) exactly as under mj_plan_request.affine
     * The pole — the line d = 0 — may cross the frame: coordinates near it are huge or infinite, hence outside, hence fill, and beyond
     * it the source is sampled where the formula says.  0 / 0 gives NaN, which Pillow's C converts to an int (undefined); here that
     * pixel is fill.  No double is converted to an int before it is known to be inside, so NO coefficient magnitude is refused.
     * MJ_ERR_INVALID, naming the output: set without a size ("perspective needs a size"); a transform_filter that is none of
     * MJ_AFFINE_*; a coefficient that is not finite; an image with a side of 32768 or more; together with reducing_gap ("not yet").
     * An affine and a perspective transform in one request are not offered.  Left for later as well: expand=True, use without a
     * size. */
    const mj_perspective *perspective;
    /* DEFAULT NULL: image k goes to slot k, the array has n_images slots, and n_slots is ignored.  Else image k goes to slot
     * slots[k] < n_slots — several plans can fill one array this way (files of several kinds are one plan per kind); slots the
     * plan does not name are not touched.  MJ_ERR_INVALID: a slot outside n_slots. */
    const int32_t *slots; int32_t n_slots;
    /* Views: several sized outputs per image from one decode (tools/views_model.py).  DEFAULT 0 — also n_views == n_images with
     * views[k] = {k, whole} for every k: one output per image.  Else, with a size, `views` holds n_views entries: the plan has n_views outputs and output k is the window
     * views[k].window of image views[k].image — byte for byte output 0 of the plan of that ONE image with rois = {the window}, the
     * k-th entry of every per-output field and every other field as given: exif_transpose(img.convert(mode)).crop(window)
     * .resize(target_k, filter[, reducing_gap]) on the canvas, mirrored if mirror[k], through the output table.  Taps stop at the
     * window's edge (crop().resize(), not resize(box=)); reducing_gap's factors come from the window's size and view k's target,
     * and its cell grid starts at the window's origin (an axis the orientation reverses: at the oriented window's end, with
     * mj_debug_reduce_shape's phase convention).  Views come in any order and several may name one image.
     *   per output (n_views entries, entry k for view k): slots, output->mirror, places; n_slots defaults to n_views
     *   per image  (n_images entries): orientations, status[]
     * An image is decoded ONCE however many views name it: the plan is the plain plan of its images — whole images, the fused launch
     * wherever the plain plan takes it, every image once in the intermediate buffer (mj_plan_time_resize's source_bytes) — and the
     * resize launch, and the reduce launch of a reducing plan, run one record per view that reads its window of that buffer.  A
     * placed plan with views never derives windows.  mj_plan_info.rgb_bytes / total_pixels count n_slots outputs;
     * mj_debug_reduce_shape's index is the view.
     * MJ_ERR_INVALID: views without a size ("views needs a size"); views together with rois; n_views < 0 or a NULL `views`; an image
     * outside the batch; an empty window or one not inside its oriented image (naming the view); an image that no view names. */
    int32_t n_views; const mj_view *views;
    /* Model-ready output.  DEFAULT NULL, or {MJ_DTYPE_U8, 0, .., NULL}: the resized bytes.  Else the dense array holds what a
     * model takes — elements of `dtype`, normalised, some images mirrored:
     *   dtype      MJ_DTYPE_U8: the resized byte itself.  MJ_DTYPE_F32: for a resized byte v of component c, torchvision's
     *              Normalize(mean, std)(to_tensor(img)) in float32, every operation rounded on its own,
     *                  y = fl32( fl32( fl32( float(v) / 255.0f ) - mean[c] ) / std[c] )
     *              (normalize == 0: mean 0, std 1, i.e. v / 255).  MJ_DTYPE_F16 / MJ_DTYPE_BF16: y rounded to nearest even to IEEE
     *              binary16 / bfloat16.  The function is applied to the integer result of the two passes, as the height pass stores
     *              it (mj_host_normalize_table is its table).
     *   normalize  0 or 1; with 1, mean[c] and std[c] for the output's components (the rest ignored), in units of value / 255.
     *   mirror     NULL, or n_images flags: image k with mirror[k] != 0 is stored flipped along its width axis — element
     *              (x, y, c) of the un-mirrored result goes to column out_width - 1 - x, in whichever layout.  Any dtype.
     * mj_plan_info.rgb_bytes of such a plan is in BYTES of the chosen type: n_slots * out_width * out_height * C * (1, 2 or 4).  It
     * is what mj_plan_execute's rgb_device buffer must hold and what mj_plan_read's rgb copies; slot offsets scale likewise.
     * MJ_ERR_INVALID: a dtype that is none of the four, normalize with MJ_DTYPE_U8, a mean that is not finite, a std that is not
     * finite or not > 0. */
    const mj_output_desc *output;
    /* Resample filter, MJ_FILTER_*.  DEFAULT MJ_FILTER_BILINEAR (0).  Any of Pillow's convolution filters, byte for byte, in every
     * layout, with everything the other fields do inside the same one launch:
     *   MJ_FILTER_BILINEAR  support 1    triangle
     *   MJ_FILTER_BOX       support 0.5  1 on (-0.5, 0.5]
     *   MJ_FILTER_HAMMING   support 1    sinc(x) * (0.54 + 0.46 cos(pi x))
     *   MJ_FILTER_BICUBIC   support 2    Keys' cubic with a = -0.5
     *   MJ_FILTER_LANCZOS   support 3    sinc(x) * sinc(x / 3) on [-3, 3)
     * (Pillow's NEAREST is not a convolution — it walks an affine transform, the walk mj_plan_request.affine offers with
     * MJ_AFFINE_NEAREST — and is not offered as a resize filter.)  Weights in doubles, normalised,
     * rounded away from zero to 22 bits (mj_host_resize_table_filtered); per pixel clip((2^21 + sum taps * in) >> 22, 0, 255) with a
     * signed sum and an arithmetic shift: the taps of BICUBIC and LANCZOS are negative in their side lobes, and plans of those two
     * run signed instances of the resize kernels (the other three share the unsigned ones: their taps are >= 0).
     * MJ_ERR_UNSUPPORTED: a table with a tap of 2^23 or more in magnitude or with 2^21 + 255 * sum |tap| above 2^31 - 1 (the
     * kernels multiply in 24 bits and add in 32; no size up to 129 comes near either bound). */
    int32_t filter;
    /* Two-step resize: Pillow's Image.resize(size, filter, reducing_gap=g) (tools/reduce_model.py).  DEFAULT 0: no first step —
     * also when no image of the batch gets a factor above 1.  Else a finite number >= 1.0, and every image is first shrunk by
     * integer factors — Image.reduce((fx, fy)), a box average with one rounding — and the reduced image is then resampled with
     * the filter over the fractional box (0, 0, w / fx, h / fy):
     *   fx = (int)(w / target_width / g), at least 1, in doubles, divided in that order; fy likewise.  w x h is the image that is
     *        resized — oriented, its window, after the mode — and the target the size it is resized to (its place's, with places)
     *   reduce   the output is ceil(w / fx) x ceil(h / fy); a cell of n pixels becomes ((sum + n / 2) * m(n)) >> 24 per component
     *        in 32-bit unsigned arithmetic, m(n) = (uint32)(float32(2^32) / float32(256 n)); partial cells at the right and
     *        bottom edges use their own n (mj_host_reduce)
     *   resample the tap tables of the reduced size over the box, whose bounds are rounded to 32-bit floats as Pillow's are
     *        (mj_host_resize_table_boxed)
     * The result is NOT the single-step result (Pillow calls it indistinguishable from g = 3 on); it is, bit for bit,
     * exif_transpose(img.convert(mode)).crop(window).resize(target, filter, reducing_gap=g) on the canvas.  One more launch
     * (csrc/reduce.hip) runs between stage 2 and the resize launch, for ALL images of the plan (a 1 x 1 cell is the identity), into
     * a second plan-owned buffer the resize launch then reads: it cuts the bytes and the taps of the resize of a strong shrink.
     * mj_plan_time_resize times both launches; its source_bytes stays what was decoded.  With places and windows the windows are
     * decoded as given (a shrunk window would move the cells).  Pillow's height-first pass order for images more than 100 times
     * taller than wide is not reproduced (nor is it without the field).
     * MJ_ERR_INVALID: a value that is not 0 and not a finite number >= 1.0 (checked with filter / mode / orientations / output,
     * before the context is looked at); set without a size.  MJ_ERR_UNSUPPORTED, naming the image: a cell of more than 65536 pixels.
     * The field is a float.  A gap a float does
     * not hold exactly would give other factors than Pillow's double does, so the Python layer refuses such a gap (1.0, 1.5, 2.0,
     * 3.0 and every other multiple of 2^-20 up to 16 are exact). */
    float reducing_gap;
    /* Aspect-preserving sizing.  DEFAULT NULL, or every place {out_width, out_height, 0, 0}: every image stretched over the whole
     * of out_width x out_height.  Else that size is a CANVAS, and every image is resized to a size of its own and placed on it
     * (tools/place_model.py): torchvision's Resize(s) + CenterCrop, a letterbox (Pillow's ImageOps.pad), a crop of the resized
     * image, all in the one resize launch.
     *   places[k]  width, height: the size image k (oriented, or its window) is resized to, 1..65535 each.  x, y: where its top-left
     *              lies on the canvas, |x|, |y| <= 65535 — negative: the image is cropped there, positive: padded.
     * Canvas element (ox, oy, c) of image k is the byte Image.resize((width_k, height_k), filter) has at (ox - x_k, oy - y_k) where
     * that lies inside the resized image, fill[c] elsewhere; either byte then takes the output's path (the dtype's table, the
     * normalisation: the fill is a byte that gets normalised, as torchvision's pad before ToTensor yields).  The mode converts
     * first, the geometry refers to the oriented image or window, and a mirror flag flips the finished canvas, padding included.
     * Only the canvas's elements are computed.  With windows, only the source rows and columns whose taps reach the canvas are
     * decoded: every window shrinks to that range (mj_plan_time_resize's source_bytes counts what was decoded); whole images are
     * decoded whole, which measured faster (option MJ_PLACE_WINDOW, csrc/resize.hip).
     * MJ_ERR_INVALID: a size or offset outside the ranges above, an image that does not meet the canvas. */
    const mj_place *places;
    /* With places.  DEFAULT NULL: zeros.  Else one byte per OUTPUT component (fill[0] alone for one component). */
    const uint8_t *fill;
    /* Colour operations on the finished canvas (tools/colour_model.py): what
     * one call of Pillow's ImageEnhance.* / ImageOps.* does to the bytes, bit for bit — the colour half of ColorJitter, RandAugment,
     * AutoAugment and TrivialAugment.  DEFAULT NULL — also every chain empty: none.  Else, with a size, `colour` holds one chain
     * per OUTPUT (n_views entries in a request with views, else n_images).  The order of operations
     * becomes decode -> mode -> orientation -> affine -> window -> resize / place / fill -> COLOUR OPS -> mirror -> element type:
     *   let C_k be the uint8 canvas of output k that the same request gives without the field, without output->mirror and with
     *   MJ_DTYPE_U8, fill pixels included.  Output k is chain k applied to C_k as a Pillow image of the output's components ("RGB" or
     *   "L"), op after op, then mirrored if mirror[k] and passed through the output table — in all four layouts.
     * An output whose chain is empty (n == 0) is the output of the request without the field; a request whose chains are ALL empty is
     * that request (mj_debug_normalise_request clears the field), with no extra launch and no extra buffer.  The rules, restated
     * (v: a byte of the canvas; every float32 / double operation rounded on its own):
     *   blend(d, v, f)         Image.blend: alpha = (float)f, t = (float)d + alpha * (float)(v - d) with v - d an int; for 0 <= alpha <= 1
     *                          the byte (uint8)t, else 0 where t <= 0, 255 where t >= 255, else (uint8)t
     *   MJ_COLOUR_BRIGHTNESS   blend(0, v, value)
     *   MJ_COLOUR_COLOR        blend(L, v, value) in all three components, L = (19595 R + 38470 G + 7471 B + 32768) >> 16 of the pixel;
     *                          the identity on a one-component output
     *   MJ_COLOUR_CONTRAST     blend(m, v, value) in every component, m = (int)(sum of i * hist_L[i] / n + 0.5) in doubles, hist_L the
     *                          histogram of the canvas's L (of the canvas itself for one component), n its pixels
     *   MJ_COLOUR_SHARPNESS    blend(s, v, value), s = ImageFilter.SMOOTH per component: k = (float)(e / 13.0) for e in (1,1,1, 1,5,1,
     *                          1,1,1); ss = 0.5f, then ss += row(y + 1), row(y), row(y - 1) with row(r) = (p[x-1] k0 + p[x] k1) + p[x+1] k2
     *                          of that row's kernel entries; s = 0 where ss <= 0, 255 where ss >= 255, else (uint8)ss; pixels of the
     *                          first and last row and column are copied (a canvas with a side below 3 is unchanged)
     *   MJ_COLOUR_POSTERIZE    v & ~(2^(8 - value) - 1), value 1..8
     *   MJ_COLOUR_SOLARIZE     v where v < t, else 255 - v; t = min(max(ceil(value), 0), 256)
     *   MJ_COLOUR_INVERT       255 - v
     *   MJ_COLOUR_AUTOCONTRAST per component (cutoff 0, no mask): lo, hi the first and last non-empty bins; hi <= lo: the identity; else
     *                          scale = 255.0 / (hi - lo), offset = -lo * scale, v -> clip((int)(v * scale + offset), 0, 255) in doubles
     *   MJ_COLOUR_EQUALIZE     per component with histogram h (no mask): one non-empty bin, or step = (pixels - the last non-empty bin's
     *                          count) / 255 == 0: the identity; else n = step / 2 and for i = 0..255: i -> min(255, n / step), n += h[i]
     *   pass(fr) along an axis of length n, per component (Pillow's BoxBlur.c; fr a float32 box radius): r = (int)fr, ww = (uint32)((float)
     *                          (1 << 24) / (fr * 2 + 1)), fw = ((1 << 24) - (2 r + 1) ww) / 2, and out[x] = (ww * sum of in[clamp(x + d)],
     *                          d = -r..r, + fw * (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + (1 << 23)) >> 24 with clamp to 0 .. n - 1,
     *                          in 32-bit unsigned arithmetic.  Every pass stores bytes, and the next pass reads those bytes.  Width and
     *                          height are the image's axes in every layout; the width passes come first
     *   MJ_COLOUR_BOX_BLUR     im.filter(ImageFilter.BoxBlur(value)): pass((float)value) along the width, then along the height
     *   MJ_COLOUR_GAUSSIAN_BLUR  im.filter(ImageFilter.GaussianBlur(value)): three passes along the width, then three along the height,
     *                          all with fr = l + a, in float32 but for the double square root and floor: sigma2 = value * value / 3,
     *                          L = (float)sqrt(12.0 * sigma2 + 1.0), l = (float)floor((L - 1.0) / 2.0), a = (2 l + 1) * (l (l + 1) - 3 sigma2),
     *                          a = a / (6 * (sigma2 - (l + 1) (l + 1)))
     *                          Both take one radius 0 <= value <= 1024 (0: the identity; Pillow's per-axis radii are not offered); the
     *                          fill pixels take part as in every op, and the blur commutes with the mirror
     *   MJ_COLOUR_ADJUST_HUE   torchvision's F.adjust_hue(im, value) on a PIL image, -0.5 <= value <= 0.5: im.convert("HSV"), H = (H + shift)
     *                          mod 256 with shift = (int)((double)value * 255) & 255 (truncated toward zero, then wrapped: 0.1 -> 25,
     *                          -0.1 -> 231, +-0.5 -> 127 / 129), and convert("RGB") — Pillow's Convert.c both ways.  To HSV: V = max; max ==
     *                          min: H = S = 0; else, in float32, cr = max - min, s = cr / max, rc = (max - r) / cr (gc, bc alike), h =
     *                          bc - gc where r is the max, else 2.0 + rc - bc where g is, else 4.0 + gc - rc, in double and rounded to
     *                          float32; h = (float)fmod(h / 6.0 + 1.0, 1.0), H = (int)(h * 255.0), S = (int)(s * 255.0) in double, clipped
     *                          to a byte.  To RGB: S == 0: V thrice; else hf = (float)H * 6.0 / 255.0 in double, i = floor(hf), f = (float)
     *                          (hf - i), fs = (float)(S / 255.0), p = round(V * (1.0 - fs)), q = round(V * (1.0 - fs * f)) with fs * f a
     *                          float32 product, t = round(V * (1.0 - fs * (1.0 - f))), else in double, round half away from zero; i % 6
     *                          picks (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q).  value 0 is NOT the identity: the round trip through
     *                          HSV bytes moves most colours by a few units, and torchvision takes it whenever the op is called.  On a
     *                          one-component output the op is the identity (it still takes up a step)
     * The launches (csrc/colour.hip): the plan's resize launch runs exactly as that of the MJ_DTYPE_U8, unmirrored, identity-slot
     * request would, into a plan-owned canvas buffer in the plan's layout.  Then, for every step s of the longest chain: a histogram
     * launch over the outputs whose op s is contrast, autocontrast or equalize (32-bit bins: LDS atomics, merged into a zeroed
     * per-output array); a launch of one wavefront per output that builds the 3 x 256 byte table of every table-shaped op, from the
     * statistics where it has some — they never leave the device, nothing synchronises —; and one launch that applies step s to
     * every output (a table look-up, color, sharpness, or a copy where the chain has ended) from one canvas into a second, the last
     * step into the caller's array at the output's slot, mirrored if flagged, through the output table.  The outputs whose op s is a
     * blur are left out by that launch (which is not made where every output's op s is a blur) and taken by one more: a workgroup holds one component plane of one output in LDS, runs all
     * the passes there and stores the last one as above; a plan whose canvas is too large for that (two planes of ow rounded up to
     * four, times oh, bytes: more than 160 KB) runs one launch per pass through a third plan-owned canvas instead (option MJ_BLUR
     * forces that route).  r, ww and fw are computed on the host, once per op.  The three-component outputs whose op s is adjust_hue
     * are left out in the same way and taken by a launch of their own, four neighbouring pixels per lane, with the second
     * conversion's per-byte terms (i % 6, f, fs) tabled on the host and held in LDS; the launches see the shift only.  mj_plan_time_resize times
     * these launches too.  mj_host_colour_ops is the host twin.
     * MJ_ERR_INVALID, naming the output: the field without a size ("colour_ops needs a size"), n outside 0..4, a kind that
     * is none of MJ_COLOUR_*, a value that is not finite, posterize bits that are not one of 1..8, a blur radius outside 0..1024
     * (Pillow takes a negative Gaussian radius; this library refuses it), an adjust_hue factor outside -0.5..0.5 (torchvision raises
     * there too).  Not offered yet: autocontrast's cutoffs and masks, more than MJ_COLOUR_MAX_OPS ops. */
    const mj_colour_chain *colour;
    /* The fill bytes of `affine` / `perspective`, beside transform_filter (specified with `affine`; the member lies here, last, so that
     * the request has no hole).  DEFAULT zeros.  One byte per OUTPUT component; set without either array: MJ_ERR_INVALID. */
    uint8_t transform_fill[3];
} mj_plan_request;
/* The host twin of the colour launches (no context): src is a row-major w x h image of ncomp (1 or 3) interleaved components, out
 * receives the chain applied to it (w * h * ncomp bytes; out may be src).  MJ_ERR_INVALID: what mj_plan_request.colour refuses of a chain, a size
 * below 1, ncomp neither 1 nor 3, NULL. */
int mj_host_colour_ops(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const mj_colour_chain *chain, uint8_t *out);
/* request NULL: a zeroed request. */
int mj_plan_create_with(mj_context *ctx, const mj_batch *batch, const mj_plan_request *request, mj_plan **out);
/* The plain plan: exactly mj_plan_create_with(ctx, batch, NULL, out). */
int mj_plan_create(mj_context *ctx, const mj_batch *batch, mj_plan **out);
/* A plan derived from a plan: several outputs — sizes, views, modes, filters, transforms, colour chains — from ONE decode.
 * `parent` is a sized plan of mj_plan_create_with (out_width / out_height set; not a window plan — no rois, no placed windows —,
 * not an own-size oriented plan, not itself derived): it leaves its decoded images, whole, in a buffer of its own, and everything
 * behind its decode reads them there.  The derived plan is a second set of exactly those launches — reduce / affine / perspective,
 * resize, colour — with arguments of its own, over the same decoded images into an output of its own.
 * `batch`: the batch the parent was made from.  Only its image count, the images' sizes and component counts and the layout are
 * read, and checked against the parent's (MJ_ERR_INVALID: not the parent's batch); no blob, table or segment is looked at.
 * `request`: out_width / out_height are required and rois must be NULL (a derived plan's windows are views).  Every other field —
 * orientations, mode, views / n_views, output, filter, reducing_gap, places, fill, slots, affine / perspective with transform_filter /
 * transform_fill, colour — means what it means to mj_plan_create_with, is checked and refused as there (same codes, same messages),
 * and is independent of the parent's request: orientation and mode are applied behind the decode, so a derived plan may differ from
 * its parent in both.  The derived plan's output equals, bit for bit, that of mj_plan_create_with(ctx, batch, request, ..).
 * MJ_ERR_INVALID besides: a NULL argument; a parent that has no size, is a window plan or is derived; a request without a size or
 * with rois.
 * ORDER: mj_plan_execute(derived, stream, out) queues only those launches.  The caller puts it BEHIND an execute of the parent —
 * the same stream, or an event — and IN FRONT OF the parent's next execute, which overwrites the images it reads; several plans
 * derived from one parent may follow one execute of it, in any order.  A derived execute is never replayed from a captured graph.
 * OWNERSHIP: a derived plan owns its tables, records, canvases, reduce / affine buffers and (rgb_device NULL) its output; the buffer
 * of decoded images stays the parent's.  Plans are counted and a derived plan holds its parent: mj_plan_destroy of the two in either
 * order is fine — a destroyed parent must not be used again, but its buffers return to the context's cache only when it and every
 * plan derived from it have been destroyed (each destroy first waits for that plan's own latest execute).
 * What a derived plan answers: mj_plan_get_info — rgb_bytes / total_pixels of its output, total_blocks / total_mcus /
 * entropy_bytes 0; mj_plan_read — its output and a status of 0 per image (the files' statuses are the parent's), MJ_ERR_INVALID
 * for the coefficient and seam pointers; mj_plan_sync, mj_plan_time_resize / _reduce / _affine / _colour and the mj_debug_*_shape
 * calls as on any sized plan; MJ_ERR_INVALID from mj_plan_execute_stage1 / _stage2, mj_plan_write_coef, mj_plan_fill_coef,
 * mj_plan_fill_source (fill the parent's), mj_plan_tune_placement, mj_plan_time_stages / _execute and mj_plan_idct_levels. */
int mj_plan_derive(mj_plan *parent, const mj_batch *batch, const mj_plan_request *request, mj_plan **out);
/* Erase: boxes of the finished outputs overwritten — torchvision's RandomErasing / F.erase(img, i, j, h, w, v), whose whole body is
 * img[..., i:i+h, j:j+w] = v, timm's RandomErasing with count > 1 (tools/erase_model.py).  It is the one step of the usual training
 * recipes that comes AFTER Normalize, so it is not a field of mj_plan_request but a call on a sized plan (derived plans included)
 * that says what to write over the output the plan's launches leave; the order of operations becomes decode -> mode ->
 * orientation -> affine / perspective -> window -> resize / place / fill -> colour ops -> mirror -> element type -> ERASE.  Boxes are
 * in the coordinates of what the caller receives — x along out_width, y along out_height, after the mirror — and the result
 * equals, bit for bit, that of the plan without the call with those elements overwritten, in all four layouts.
 *   rects          n records, host memory, copied into a plan-owned device buffer at the call.  The boxes of one output are applied
 *                  in the order they are listed: where two overlap, the later one's elements stay.
 *   MJ_ERASE_CONST value[c] for output component c (value[0] alone for one component), a float32 converted to the plan's dtype with
 *                  one rounding to nearest even — torch.tensor(v) assigned into the tensor; MJ_DTYPE_U8: an integer 0..255
 *   MJ_ERASE_VALUES  one element per element of the box: element (c, yy, xx) of the box is values_device[offset + (c * height +
 *                  yy) * width + xx] — (C, height, width) order whatever the plan's layout —, elements of the plan's dtype in
 *                  DEVICE memory.  values_device is BORROWED: the caller keeps it valid and unchanged until the executes that
 *                  read it have finished.  Noise (torchvision's value="random", timm's mode="pixel") is the caller's to draw: no
 *                  bit-exact reference exists for an in-library generator, so none is offered.  CutMix / MixUp, which mix across
 *                  outputs and plans, are a call of their own behind the plans: mj_mix, below.
 * n == 0 takes the erase off the plan again.  The call waits for the plan's latest execute, drops the plan's captured graph — the
 * next execute launches plainly and a later one may capture again, with the new pointers — and from then on mj_plan_execute (and
 * mj_plan_execute_stage2) queues the erase launch(es) last, behind the plan's final store, on the same stream, inside a capture
 * too.  Only bytes inside boxes are written — 16-byte stores in the aligned body of every contiguous run, element stores at its
 * ends, never a read-modify-write over a box's edge: the neighbouring elements may be another plan's slot, written on another
 * stream at that moment.  The work is dealt out by a job list over the runs (csrc/erase_addr.h), so the grid follows the sum of
 * the boxes; it is ONE launch where no two boxes of one output intersect, else one launch per box ordinal (box 0 of every
 * output, then box 1, ...).  No LDS, no atomics, nothing synchronises with the host.
 * MJ_ERR_INVALID, naming the box: a plan without a size; n < 0; NULL rects with n > 0; an output outside the plan's outputs; a box
 * with a width or height below 1 or not inside out_width x out_height; a kind that is neither of the two; a CONST value that is
 * not finite, or for MJ_DTYPE_U8 not an integer 0..255; a VALUES box with NULL values_device or a negative offset. */
#define MJ_ERASE_CONST  0
#define MJ_ERASE_VALUES 1
typedef struct {
    int32_t output;                /* the plan's output: view k, else image k; the launch addresses its slot */
    int32_t x, y, width, height;   /* inside out_width x out_height, after the mirror */
    int32_t kind;
    float   value[3];              /* CONST: per output component; converted float32 -> the plan's dtype, nearest even; U8: an integer 0..255 */
    int64_t offset;                /* VALUES: element offset of this box's (C, height, width) block in `values` */
} mj_erase_rect;
int mj_plan_set_erase(mj_plan *plan, int32_t n, const mj_erase_rect *rects, const void *values_device);
/* The erase launch(es) of a plan alone (after an execute: into where it wrote), `iters` times: ms per run of all of them, and the
 * bytes one run writes (VALUES boxes read as many).  MJ_ERR_INVALID: no erase set, nothing executed yet. */
int mj_plan_time_erase(mj_plan *plan, int iters, float *ms, int64_t *bytes_written);
/* The host twin of the erase launch (no context): the same records over a HOST array of n_slots slots of width x height pixels of
 * ncomp (1 or 3) components of `dtype` in `layout` — `output` is the slot, `values` host memory —, through the launch's own address
 * arithmetic (csrc/erase_addr.h).  MJ_ERR_INVALID (mj_last_error(NULL)): what mj_plan_set_erase refuses, an unknown layout or dtype,
 * ncomp neither 1 nor 3, a size outside 1..65535, n_slots below 1, NULL. */
int mj_host_erase(void *array, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height, int32_t n_slots, int32_t n,
                  const mj_erase_rect *rects, const void *values);
/* Mix: MixUp and CutMix over the finished outputs of a CALL (tools/mix_model.py) — the step the training recipes put in the collate
 * function, behind RandomErasing: ... -> mirror -> element type -> erase -> MIX.  Output k's partner may be any output of the
 * array, which another plan may have written on another stream; so this is no field of mj_plan_request and no call on a plan,
 * but the library's one launch that belongs to the caller's whole batch: it runs over the array once every plan that writes it
 * has been synchronised, reads `src` and writes `dst`, and every output reads `src` as it stands — the mixing is simultaneous,
 * as it is where torchvision and timm mix from a roll / flip copy.
 *   src, dst       n_outputs slots of width x height pixels of ncomp (1 or 3) components of MJ_DTYPE_* `dtype` in MJ_LAYOUT_*
 *                  `layout`, DEVICE memory; they must not overlap.  dst is written in full.  Any alignment is taken: 16 bytes
 *                  per lane where src and dst are congruent mod 16 and aligned to their elements, element by element at a
 *                  slot's ends and otherwise.
 *   ops            n_outputs records, host memory, copied at the call into a context-owned device buffer; a call that finds the
 *                  previous mix launch still in flight waits for it before it rewrites that buffer.
 *   MJ_MIX_NONE    dst[k] = src[k]
 *   MJ_MIX_CUTMIX  dst[k] = src[k] with the box (x along width, inside the canvas, sides >= 1) taken from src[partner]; any dtype
 *   MJ_MIX_MIXUP   float dtypes.  With ws = float32(lam), wp = float32(1.0 - lam) (subtracted in double, rounded once), per element
 *                  dst = T(f32(T(f32(src[partner]) * wp)) + f32(T(f32(src[k]) * ws))), T rounding to nearest even into the dtype,
 *                  every float32 operation rounded on its own: x.roll(1, 0).mul(1.0 - lam).add_(x.mul(lam)) of torch's CPU ops,
 *                  bit for bit.  partner == k still runs the arithmetic.  A NaN result is some NaN.
 *   stream         a hipStream_t, or 0 for the context's, as mj_plan_execute takes it.
 * One launch (csrc/mix.hip: k_mix); nothing synchronises with the host behind it.  MJ_ERR_INVALID, naming the output: a kind that
 * is none of the three, a partner outside 0 .. n_outputs - 1, lam not finite or outside 0..1, MIXUP with MJ_DTYPE_U8, a box with
 * a side below 1 or not inside the canvas; overlapping src / dst; NULL; an unknown layout or dtype; ncomp neither 1 nor 3; a size
 * outside 1..65535; n_outputs below 1. */
#define MJ_MIX_NONE   0
#define MJ_MIX_MIXUP  1
#define MJ_MIX_CUTMIX 2
typedef struct {
    int32_t kind;                  /* MJ_MIX_* */
    int32_t partner;               /* an output of the same array; may be the output itself */
    int32_t x, y, width, height;   /* CUTMIX: the box, after the mirror */
    double  lam;                   /* MIXUP: the output's own weight, 0..1 */
} mj_mix_op;
int mj_mix(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width,
           int32_t height, int32_t n_outputs, const mj_mix_op *ops);
/* The mix launch alone on the context's stream, `iters` times behind one warm run: ms per launch. */
int mj_mix_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width,
                int32_t height, int32_t n_outputs, const mj_mix_op *ops, float *ms);
/* The host twin of the mix launch (no context): the same records over HOST arrays, through the launch's own rule and box test
 * (csrc/mix_rule.h).  MJ_ERR_INVALID (mj_last_error(NULL)): what mj_mix refuses. */
int mj_host_mix(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height,
                int32_t n_outputs, const mj_mix_op *ops);
/* Compose: several finished outputs of a CALL pasted onto one canvas (tools/compose_model.py) — Mosaic, image grids, a crop of one
 * sample in another at another place: ... -> mirror -> element type -> erase -> COMPOSE.  A canvas's tiles may be outputs of
 * several plans, so, like mj_mix, this is no field of mj_plan_request and no call on a plan but a launch over the caller's whole
 * batch, once every plan that writes it has been synchronised.  It reads `src` and writes `dst`, an array of another size:
 *     dst[m] = a dst_width x dst_height canvas of fill
 *     for every tile with output == m, in the order of `tiles`:     (a later tile wins where two overlap)
 *         dst[m][dy .. dy + height, dx .. dx + width] = src[source][sy .. sy + height, sx .. sx + width], clipped to the canvas
 * Elements are copied as bits; a tile that misses the canvas wholly pastes nothing.
 *   src            n_sources slots of src_width x src_height pixels of ncomp (1 or 3) components of MJ_DTYPE_* `dtype` in
 *                  MJ_LAYOUT_* `layout`, DEVICE memory, aligned to its elements.
 *   dst            n_outputs slots of dst_width x dst_height pixels, same components, dtype and layout; DEVICE memory, aligned to
 *                  its elements; it must not overlap src.  dst is written in full, every element exactly once, and never read.
 *   fill_bits      one element bit pattern per component, in the low bytes (what a normalised fill byte is stored as is the
 *                  caller's business: mj_host_normalize_table).
 *   tiles          n_tiles records, host memory (n_tiles may be 0: all fill), in paste order; the outputs need not be grouped.
 *                  At most 64 per output.  x runs along the width; the window lies wholly inside the source canvas, sides >= 1;
 *                  dx and dy may be negative or beyond the canvas, |dx|, |dy| < 2^20.
 *   stream         a hipStream_t, or 0 for the context's, as mj_plan_execute takes it.
 * The host resolves every output's tiles into disjoint rectangles that partition the canvas exactly (csrc/compose_addr.h; "later
 * wins" is decided there) and cuts them into jobs of lines, copied at the call into a context-owned device buffer; a call that
 * finds the previous compose launch still in flight waits for it before it rewrites that buffer.  One launch (csrc/compose.hip:
 * k_compose); nothing synchronises with the host behind it.  MJ_ERR_INVALID, naming the tile: an output or source that is none,
 * a window with a side below 1 or not inside the source canvas, an offset of 2^20 or more, more than 64 tiles in one output;
 * overlapping src / dst; pointers not aligned to their elements; NULL; an unknown layout or dtype; ncomp neither 1 nor 3; a size
 * outside 1..65535; n_sources or n_outputs below 1; n_tiles below 0. */
typedef struct {
    int32_t output;                /* the canvas the tile is pasted on, 0 .. n_outputs - 1 */
    int32_t source;                /* the slot it is taken from, 0 .. n_sources - 1 */
    int32_t sx, sy, width, height; /* the window of the source canvas, after the mirror */
    int32_t dx, dy;                /* where the window's top-left corner lands on the output canvas */
} mj_compose_tile;
int mj_compose(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp,
               int32_t src_width, int32_t src_height, int32_t n_sources, int32_t dst_width, int32_t dst_height, int32_t n_outputs,
               const uint32_t fill_bits[3], int32_t n_tiles, const mj_compose_tile *tiles);
/* The compose launch alone on the context's stream, `iters` times behind one warm run: ms per launch. */
int mj_compose_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp,
                    int32_t src_width, int32_t src_height, int32_t n_sources, int32_t dst_width, int32_t dst_height, int32_t n_outputs,
                    const uint32_t fill_bits[3], int32_t n_tiles, const mj_compose_tile *tiles, float *ms);
/* The host twin of the compose launch (no context): the same records over HOST arrays, through the launch's own resolve and job
 * list (csrc/compose_addr.h), line by line.  MJ_ERR_INVALID (mj_last_error(NULL)): what mj_compose refuses. */
int mj_host_compose(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height,
                    int32_t n_sources, int32_t dst_width, int32_t dst_height, int32_t n_outputs, const uint32_t fill_bits[3],
                    int32_t n_tiles, const mj_compose_tile *tiles);
/* The rectangles the launch resolves the tiles into (host only): per output, in order, disjoint rectangles whose union is the
 * canvas; `source` -1: fill, else (x, y) of the canvas is (sx, sy) of that source slot.  Cells of one owner are merged along the
 * layout's contiguous axis first, then across it.  rects NULL: *n_rects is a capacity that always suffices, the sum over the
 * outputs of (2 * its tiles + 1)^2.  Else *n_rects is the number of rectangles; MJ_ERR_INVALID when `cap` is below it (nothing
 * is written then), and for what mj_compose refuses of the geometry and the tiles. */
typedef struct {
    int32_t output, x, y, width, height;
    int32_t source;                /* -1: fill */
    int32_t sx, sy;
} mj_compose_rect;
int mj_host_compose_resolve(int32_t layout, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources, int32_t dst_width,
                            int32_t dst_height, int32_t n_outputs, int32_t n_tiles, const mj_compose_tile *tiles, mj_compose_rect *rects,
                            int32_t cap, int32_t *n_rects);
/* Patchify: the finished outputs of a CALL cut into patch x patch patches and packed as the token rows of a native-resolution
 * vision encoder (tools/patch_model.py) — Qwen2-VL's pixel_values, NaFlex's patches: ... -> erase -> mix | compose -> PATCHES.
 * Like mj_mix and mj_compose a launch over the caller's whole batch, once every plan that writes it has been synchronised.  It
 * reads `src` and writes `dst`, a matrix of rows of D = ncomp * repeat * patch * patch elements.  With source k's window
 * (x, y, width, height), gh = height / patch, gw = width / patch, m = merge, t = repeat, P = patch:
 *     row = row0[k] + ((py / m) * (gw / m) + px / m) * m * m + (py % m) * m + px % m             patch (py, px) of source k
 *     MJ_PATCH_CHW:  dst[row][((c * t + r) * P + j) * P + i] = window_k[c][py * P + j][px * P + i]        for r in 0 .. t - 1
 *     MJ_PATCH_HWC:  dst[row][(j * P + i) * ncomp + c]       = window_k[c][py * P + j][px * P + i]
 * whatever `layout` is.  Elements are copied as bits.  length 0, the packed form: row0[k] is the number of tokens of the sources
 * before k and dst has sum(gh_k * gw_k) rows.  length L >= 1, the padded form: row0[k] = k * L, dst has n_sources * L rows and
 * the rows behind a source's last token hold element bit pattern 0.
 *   src            n_sources slots of src_width x src_height pixels of ncomp (1 or 3) components of MJ_DTYPE_* `dtype` in
 *                  MJ_LAYOUT_* `layout`, DEVICE memory, aligned to its elements.
 *   dst            exactly rows * D elements (mj_host_patchify_count gives the rows); DEVICE memory, aligned to its elements —
 *                  no more: a row starts wherever it starts —; it must not overlap src.  dst is written in full, every element
 *                  exactly once, and never read.
 *   patch, merge, repeat   1..64, 1..8, 1..4; MJ_PATCH_HWC needs repeat 1.  A merge block, merge * merge * D elements, is at
 *                  most 65536 bytes.
 *   windows        one record per source, host memory, or NULL: the whole canvas of every source.  x runs along the width; the
 *                  window lies wholly inside the canvas; width and height are multiples of patch * merge, at least one.
 *   stream         a hipStream_t, or 0 for the context's, as mj_plan_execute takes it.
 * The host cuts the output into jobs — runs of merge blocks of one merge band, whose tokens are one contiguous range of dst
 * (csrc/patch_addr.h) —, copied at the call into a context-owned device buffer; a call that finds the previous patchify launch
 * still in flight waits for it before it rewrites that buffer.  One launch (csrc/patch.hip: k_patchify); nothing synchronises
 * with the host behind it.  MJ_ERR_INVALID, naming the source: a window with a side below 1, not inside the canvas or not a
 * multiple of patch * merge (the whole canvas under NULL likewise); a source of more than `length` tokens; patch, merge or repeat
 * outside its range; an unknown order, MJ_PATCH_HWC with repeat above 1; length below 0; a merge block of more than 65536 bytes;
 * overlapping src / dst; pointers not aligned to their elements; NULL; an unknown layout or dtype; ncomp neither 1 nor 3; a size
 * outside 1..65535; n_sources below 1; more bytes than an address holds. */
#define MJ_PATCH_CHW 0   /* a token is (C, t, P, P): Qwen2-VL */
#define MJ_PATCH_HWC 1   /* a token is (P, P, C): SigLIP 2 NaFlex, timm NaFlexVit */
typedef struct {
    int32_t x, y, width, height;
} mj_patch_window;
int mj_patchify(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp,
                int32_t src_width, int32_t src_height, int32_t n_sources, int32_t patch, int32_t merge, int32_t repeat, int32_t order,
                int32_t length, const mj_patch_window *windows);
/* The patchify launch alone on the context's stream, `iters` times behind one warm run: ms per launch. */
int mj_patchify_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp,
                     int32_t src_width, int32_t src_height, int32_t n_sources, int32_t patch, int32_t merge, int32_t repeat,
                     int32_t order, int32_t length, const mj_patch_window *windows, float *ms);
/* The host twin of the patchify launch (no context): the same over HOST arrays, through the launch's own job list and address
 * rule (csrc/patch_addr.h), element by element.  MJ_ERR_INVALID (mj_last_error(NULL)): what mj_patchify refuses. */
int mj_host_patchify(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height,
                     int32_t n_sources, int32_t patch, int32_t merge, int32_t repeat, int32_t order, int32_t length,
                     const mj_patch_window *windows);
/* The rows of dst (host only): the geometry checked as mj_patchify checks it — MJ_ERR_INVALID for what it refuses of it — and
 * *rows the number of token rows, n_sources * length in the padded form.  Callers size dst by it. */
int mj_host_patchify_count(int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources,
                           int32_t patch, int32_t merge, int32_t repeat, int32_t order, int32_t length, const mj_patch_window *windows,
                           int64_t *rows);
/* The host twin of the kernels' mode conversion (no context): n_pixels pixels of src_ncomp (1 or 3) interleaved components into
 * out, which holds n_pixels * (mode, or src_ncomp for MJ_MODE_NATIVE) bytes.  MJ_ERR_INVALID: an unknown mode, a src_ncomp that
 * is neither 1 nor 3, NULL with pixels to convert. */
int mj_host_convert_mode(int32_t mode, const uint8_t *src, int32_t src_ncomp, int64_t n_pixels, uint8_t *out);
/* The host twin of the affine launch (no context): src is a row-major w x h image of ncomp (1 or 3) interleaved components;
 * out receives the window (x0, y0, win_w, win_h) of its transform under matrix a[6] with MJ_AFFINE_* `filter` and fill[ncomp] —
 * row-major, win_w * win_h * ncomp bytes, evaluated at the window's absolute coordinates.  The window may reach beyond w x h:
 * Image.transform(size, ..) with a size of its own is the window (0, 0, size).  MJ_ERR_INVALID: what mj_plan_request.affine
 * refuses (its corner tests on the larger of the image and the window's end), an empty window, NULL. */
int mj_host_affine(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const double *a, int32_t filter, const uint8_t *fill,
                   int32_t x0, int32_t y0, int32_t win_w, int32_t win_h, uint8_t *out);
/* The host twin of the perspective launch (no context), shaped like mj_host_affine: the window (x0, y0, win_w, win_h) of the
 * transform of the row-major w x h image under coefficients a[8] with MJ_AFFINE_NEAREST / BILINEAR / BICUBIC `filter` and
 * fill[ncomp] (NULL: zeros).  The window may reach beyond w x h.  MJ_ERR_INVALID: a filter that is none of the three, a
 * coefficient that is not finite, a side of 32768 or more, an empty window or one that ends at 32768 or beyond, NULL. */
int mj_host_perspective(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, const double *a, int32_t filter, const uint8_t *fill,
                        int32_t x0, int32_t y0, int32_t win_w, int32_t win_h, uint8_t *out);
void mj_plan_destroy(mj_plan *plan);
int mj_plan_get_info(const mj_plan *plan, mj_plan_info *info);
/* Which form of stage 1 the plan chose: one restart segment per wavefront, one per lane, long segments
 * cut into self-synchronised pieces, or scan by scan (progressive / non-interleaved); MJ_FORM_WG_TABLES is or-ed in when
 * the batch has more Huffman tables than LDS holds and every workgroup loads only the tables of its own images,
 * MJ_FORM_RESOLVED when the lane / synchronisation form decodes with the resolved 13-bit AC tables (huffman_lanes13.hip:
 * every batch whose distinct tables fit LDS in that format — at most 3 AC and 4 DC tables). */
#define MJ_FORM_WAVE      0
#define MJ_FORM_LANES     1
#define MJ_FORM_SYNC      2
#define MJ_FORM_SCANS     3
#define MJ_FORM_WG_TABLES 16
#define MJ_FORM_RESOLVED  32
#define MJ_FORM_COUNT_RESOLVED 128   /* MJ_FORM_SYNC: the counting walks run on resolved tables with a repair work list
                                        (huffman_sync.hip: k_count) instead of the classic rounds; MJ_FORM_SCANS: the first AC
                                        scans are walked in self-synchronising chunks (progressive_chunks.hip) */
#define MJ_FORM_FUSED     64   /* mj_plan_execute runs stages 1 and 2 as ONE launch (fused.hip): lane-walk wavefronts and
                                  reconstruction wavefronts side by side in one workgroup per CU.  Uniform x-major batches of
                                  4:4:4 / 4:2:2 / 4:4:0 / 4:2:0 files with one restart interval per MCU row and the resolved
                                  tables; mj_plan_execute_stage1 / _stage2 of such a plan are the two launches as ever */
int mj_plan_stage1_form(const mj_plan *plan);
/* offsets (in elements of the respective output) of image i inside the packed outputs */
int mj_plan_image_offsets(const mj_plan *plan, int32_t image, int64_t *block_off, int64_t *rgb_off);

/* Launch stage 1 (Huffman) + stage 2 (dequant/IDCT/upsample/colour) on `stream` (a hipStream_t passed as
 * void*, NULL = the context's own stream).  `rgb_device` is a device buffer of rgb_bytes bytes, or NULL to
 * use a plan-owned one.  Asynchronous for every kind of batch: nothing in it waits for the device. */
int mj_plan_execute(mj_plan *plan, void *stream, uint8_t *rgb_device);
/* (A plan owns ONE coefficient store, one set of stage-1 scratch and one stage-2 work counter: executes of the same plan must
 * not overlap — queue them on one stream, or wait for mj_plan_sync before using another.  Different plans overlap freely.) */
/* The two stages separately (profiling, config 2). */
int mj_plan_execute_stage1(mj_plan *plan, void *stream);
int mj_plan_execute_stage2(mj_plan *plan, void *stream, uint8_t *rgb_device);
int mj_plan_sync(mj_plan *plan);   /* waits for this plan's latest execute (on whichever stream it went), not for other work on that stream */

/* Device pointers of plan-owned buffers (valid until mj_plan_destroy): zero-copy hand-off to torch etc. */
int mj_plan_device_buffers(mj_plan *plan, int16_t **coef, uint8_t **rgb, int16_t **planes, int16_t **idct);

/* Copy results to host memory (after mj_plan_sync).  Any pointer may be NULL. */
int mj_plan_read(mj_plan *plan, uint8_t *rgb_host, int16_t *coef_host, int16_t *planes_host,
                 int16_t *idct_host, int32_t *status_host);
/* Replace the plan's coefficient array (config 2: coefficients decoded elsewhere). mem = MJ_MEM_*. */
int mj_plan_write_coef(mj_plan *plan, const int16_t *coef, int32_t mem);

/* Test hook, host only (no GPU, no context): the form stage 1 would take for a batch with these restart-segment byte lengths —
 * csrc/form_select.h's rule, the one mj_plan_create applies.  traits: 1 a table serves as DC and AC table, 2 segments not in blob
 * order, 4 progressive, 8 a sampling layout outside the common five, 16 MJ_FLAG_GPU_SEGMENT, 32 ... with one segment per image,
 * 64 a DC size above 15, 128 MJ_FLAG_NO_SYNC, 256 per-workgroup table lists do not fit.  force: MJ_HUFFMAN's value or NULL;
 * forced_chunk: MJ_SYNC_CHUNK or 0.  out = { MJ_FORM_* (| MJ_FORM_WG_TABLES), chunk bytes, chunks, 1 if the segments would be
 * dealt out by length }. */
int mj_debug_stage1_form(const int32_t *seg_len, int64_t n_segs, uint64_t blob_len, int32_t n_huff, uint32_t traits, const char *force,
                         int32_t forced_chunk, int32_t out[4]);

/* Test hook, host only: the tables the counting walks of MJ_FORM_SYNC look symbols up in (csrc/huffman_sync.hip: k_count), as
 * mj_plan_create builds them for a batch with these n_huff <= 8 tables — roles[t] 1 = DC table, 2 = AC table —, wbits index bits.
 * *tab_bytes = bytes from one table to the next; out (may be NULL) receives n_huff * tab_bytes / 4 words.  MJ_ERR_UNSUPPORTED:
 * such a batch takes the classic rounds (a table in both roles, a DC size above 15, tables too large). */
int mj_debug_count_tables(const mj_huff_spec *huff, int32_t n_huff, const int32_t *roles, int32_t wbits, uint32_t *out, int64_t cap_words,
                          int32_t *tab_bytes);

/* Test hook, host only: the resolved AC tables of the lane walk (csrc/lanes13_walk.h) as mj_plan_create builds them for a batch with
 * these n_huff <= 8 tables — roles[t] 2 = AC table, anything else: not built; slot_of_table[t] = the slot (0 .. n_ac - 1) of AC table t;
 * ab_of_slot[s] = 10..13 index bits of slot s.  fixed_slot_bytes: the stride from one slot to the next (the stage-1 kernel's), or 0: back
 * to back, each as small as its codes allow (a fused launch's).  slot_off[s] = byte offset of slot s, *total_bytes = bytes in all; out
 * (may be NULL) receives total_bytes / 4 words.  MJ_ERR_UNSUPPORTED: does not fit (more second-level tables than a slot holds). */
int mj_debug_resolved_tables(const mj_huff_spec *huff, int32_t n_huff, const int32_t *roles, const int32_t *slot_of_table, int32_t n_ac,
                             const int32_t ab_of_slot[4], int32_t fixed_slot_bytes, uint32_t *out, int64_t cap_words, int32_t slot_off[4],
                             int32_t *total_bytes);

/* Test hook, host only: how a fused launch (MJ_FORM_FUSED) would be cut for a batch of n_images images of segments_per_image
 * restart segments on a chip of `cus` CUs — out = { applies (LDS), images per workgroup and pass, producer wavefronts, lanes per
 * producer, consumer wavefronts beside them, bytes of LDS the producers take, passes per workgroup, workgroups }. */
int mj_debug_fused_shape(int32_t cus, int32_t n_ac, int32_t n_dc, int32_t ac_slot_bytes, int32_t hmax, int32_t vmax, int32_t transposed,
                         int32_t n_images, int32_t segments_per_image, int32_t want_consumers, int32_t out[8]);

/* Test hook, host only: would mj_plan_execute of such a batch be ONE fused launch (csrc/form_select.h: fused_applies, the rule
 * mj_plan_create applies before it asks mj_debug_fused_shape's question)?  layout: MJ_LAYOUT_*; every image mcus_per_row x
 * mcu_rows MCUs with one restart interval (0: none); traits: 1 not the lane form on resolved tables, 2 segments dealt out by length
 * (files of mixed content), 4 segments in another order, 8 images of several geometries, 16 a sampling layout outside the common
 * five, 32 progressive, 64 images with different restart intervals; flags: the plan's MJ_FLAG_*.
 * *mode_out = 0 the two launches, 1 fused with whole images per workgroup, 2 fused with the hand-off across workgroups. */
int mj_debug_fused_applies(int32_t layout, int32_t ncomp, int32_t hmax, int32_t vmax, int32_t mcus_per_row, int32_t mcu_rows,
                           int32_t restart_interval, int32_t n_images, uint32_t traits, uint32_t flags, int32_t *mode_out);

/* Test hook, host only: which scans of a progressive batch would be walked as scout + parts (csrc/form_select.h:
 * choose_prog_split, the rule mj_plan_create applies).  mode: MJ_PROG_SPLIT (1 = by the size of the batch); n_bands: band launches
 * per scan (MCU rows / rows per band); wave_slots: CUs x 32, 0 = MI355X's; parts: MJ_PROG_PARTS or 0 (not set: the rule may
 * choose); per scan its image, restart segments and entropy-coded bytes (< 0: not a refining AC scan of one component).
 * split_out[k] = 1: scan k is split; *parts_out = parts per band. */
int mj_debug_prog_split(int32_t mode, int32_t n_images, int32_t n_bands, int32_t wave_slots, int32_t parts, int32_t n_scans,
                        const int32_t *image, const int32_t *n_segments, const int64_t *bytes, uint8_t *split_out, int32_t *parts_out);

/* Test hook: every byte of the plan's coefficient store := byte_value (synchronous).  The parity tests poison the store in
 * front of a fused execute: a reconstruction wavefront that read a block before its decoder wavefront had written it would
 * show (a store that still holds the previous execute's blocks of the same files hides exactly that). */
int mj_plan_fill_coef(mj_plan *plan, int byte_value);

/* Test hook: every byte of a resized plan's intermediate buffer (the un-resized pixels) := byte_value (synchronous). */
int mj_plan_fill_source(mj_plan *plan, int byte_value);

/* Test hook: how a resized plan's launch is cut and which instances it runs — out = { output rows per tile, output columns per
 * tile, tiles along the width, tiles along the height (per image), bytes of LDS per workgroup, the plan's MJ_FILTER_*, 1 if it
 * runs the signed instances, the most taps one pixel has along an axis }.  MJ_ERR_INVALID: not a resized plan. */
int mj_debug_resize_shape(const mj_plan *plan, int32_t out[8]);

/* Test hook: the first step of a resized plan for one image — out = { fx, fy, phase along the width, phase along the height, reduced
 * width, reduced height, 1 if the plan reduces at all (else 0, factors 1 and the decoded size) }, all in the STORED image's axes: an
 * axis the orientation reverses has its cell boundaries at phase + k * f, phase = size mod f, and orientations 5..8 exchange the
 * factors.  A plan with views: `image` is the view, and the sizes are its window's.  MJ_ERR_INVALID: not a resized plan, no such
 * image (view). */
int mj_debug_reduce_shape(const mj_plan *plan, int32_t image, int32_t out[7]);

/* Test hook (host only, reads fields): how a reducing plan's reduce launch is cut — out = { reduced rows per tile, reduced pixels of
 * a row per tile (along the contiguous axis), tiles along the rows, tiles along the contiguous axis (per image: those of the largest
 * reduced image), source pixels of a row a wavefront stages at a time in the instance the plan launches }.  MJ_ERR_INVALID: not a
 * reducing plan. */
int mj_debug_reduce_launch(const mj_plan *plan, int32_t out[5]);

/* Test hook (host only, no context): *normal = the request as plan creation sees it after its checks — every field that names its
 * default turned into its absence (pointers are the caller's; where the library derived the views of a request with a transform
 * itself, n_views is their count and views is NULL) — or the code of the first fault that needs no context
 * (mj_last_error(NULL) has the message).  request NULL: a zeroed one. */
int mj_debug_normalise_request(const mj_batch *batch, const mj_plan_request *request, mj_plan_request *normal);

/* Test hook (host only, reads fields): what plan creation decided, MJ_DEBUG_PLAN_SHAPE_WORDS values in this order —
 *   0 mj_plan_stage1_form's word, 1 fused launch, 2 table slots per image, 3 restart segments, 4 marker-scan jobs;
 *   5 chunk bytes of the synchronisation form, 6 its chunks, 7 stage-0 pieces, 8 index bits and 9 bytes per table of the resolved
 *   counting tables (0: classic rounds), 10 / 11 tables per workgroup of the lane launch's / the counting rounds' lists (0: none),
 *   12 segment order (0 blob, 1 binned, 2 striped);
 *   13 / 14 resolved AC / DC tables, 15..18 index bits per LDS slot and 19 bytes of a fused launch's AC tables;
 *   20 images per workgroup, 21 passes, 22 producers, 23 lanes per producer, 24 consumers, 25 segments dealt out by length,
 *   26 workgroups of such a launch, 27 restart segments per image of a fused launch;
 *   28 strips per stage-2 job, 29 jobs per ticket, 30 jobs of image 0, 31 jobs in all (low word);
 *   32 the plan works on a padded copy of the caller's device blob;
 *   33 progressive: stage-0 stream read, 34 band pipeline, 35 its launches, 36 segments of split scans, 37 first scans in chunks.
 * cap: room in out, at least MJ_DEBUG_PLAN_SHAPE_WORDS (MJ_ERR_INVALID otherwise). */
#define MJ_DEBUG_PLAN_SHAPE_WORDS 38
int mj_debug_plan_shape(const mj_plan *plan, int32_t *out, int32_t cap);

/* Test hook (host only): the context's device buffer cache — out = { blocks handed out now, their bytes, requests made so far,
 * a running hash of the requested sizes in order (h = h * 0x100000001b3 + bytes per request) }. */
int mj_debug_cache_stats(const mj_context *ctx, uint64_t out[4]);

/* ---- one-shot conveniences ----------------------------------------------------------------------- */
/* create + execute + sync + read + destroy; rgb_out/status_out host, coef_out may be NULL. */
int mj_decode_baseline_batch(mj_context *ctx, const mj_batch *batch, uint8_t *rgb_out, int16_t *coef_out,
                             int32_t *status_out);
/* Stage 2 only on caller-supplied coefficients (host), descriptors as above (segment fields ignored). */
int mj_idct_batch(mj_context *ctx, const mj_batch *batch, const int16_t *coef, uint8_t *rgb_out);

/* ---- measurement --------------------------------------------------------------------------------- */
/* Average device time (ms) of each stage's kernel over `iters` back-to-back launches on the plan's
 * stream, measured with HIP events recorded on that stream. */
int mj_plan_time_stages(mj_plan *plan, int iters, uint8_t *rgb_device, float *stage1_ms, float *stage2_ms);
/* The same for the launches mj_plan_execute makes.  A plan whose execute is ONE fused launch (MJ_FORM_FUSED): front_ms = what
 * runs in front of it (marker scan with MJ_FLAG_GPU_SEGMENT, stage 0), main_ms = the fused launch.  Any other plan: the two
 * stages as mj_plan_time_stages reports them (front = stage 0+1, main = stage 2). */
int mj_plan_time_execute(mj_plan *plan, int iters, uint8_t *rgb_device, float *front_ms, float *main_ms);

/* A resized plan's resize launch alone (after an execute: it reads what stage 2 left), `iters` times into rgb_device (NULL: where the
 * latest execute wrote): ms per launch, and the bytes of un-resized pixels it reads (written bytes: mj_plan_info.rgb_bytes). */
int mj_plan_time_resize(mj_plan *plan, int iters, uint8_t *rgb_device, float *ms, int64_t *source_bytes);
/* A plan's affine — or perspective — launch alone (mj_plan_request.affine; after an execute): ms per launch, and the bytes it writes (it reads, at
 * most, mj_plan_time_resize's source_bytes).  MJ_ERR_INVALID: not a plan with an affine transform. */
int mj_plan_time_affine(mj_plan *plan, int iters, float *ms, int64_t *written_bytes);
/* The colour launches of a plan with colour operations alone (mj_plan_request.colour; after an execute: they read the canvases the
 * resize launch left), `iters` times into where the latest execute wrote: ms per run of all of them — the histogram, table and
 * apply launches of every step —, and the bytes of one set of canvases (outputs x out_width x out_height x components).
 * MJ_ERR_INVALID: not a plan with colour operations, nothing executed yet. */
int mj_plan_time_colour(mj_plan *plan, int iters, float *ms, int64_t *canvas_bytes);
/* A reducing plan's reduce launch alone (mj_plan_request.reducing_gap; after an execute): ms per launch.  It reads the decoded
 * pixels (mj_plan_time_resize's source_bytes) and writes the reduced images.  MJ_ERR_INVALID: not a reducing plan. */
int mj_plan_time_reduce(mj_plan *plan, int iters, float *ms);

/* Placement tuning of a plan that is executed many times into ONE output buffer (a service's output slot, a benchmark's step).
 * Where the plan's coefficient store lies relative to that buffer — physically: nothing the virtual addresses show — puts the
 * fused launch (MJ_FORM_FUSED) into one of two classes 8-9 % apart (profiles/r06_placement.txt).  Tries `candidates` (1..16)
 * stores — the plan's own, then fresh allocations —, each with a few timed executes into rgb_device on `stream` (NULL: the
 * context's), keeps the fastest and releases the others; then the same for the plan's stage-0 stream buffer (the other buffer
 * the launch's traffic runs through).  ms_out[candidates] (may be NULL): ms per execute of each coefficient store tried (0 = not
 * tried); *chosen (may be NULL): which one stayed; *best_ms (may be NULL): ms per execute with what the plan ends up with.  The
 * output buffer is the caller's: a caller that owns several can call this for each and keep the best pair (bench.py does).  Plans
 * that are not fused are left alone (all zeros).  Synchronous. */
int mj_plan_tune_placement(mj_plan *plan, void *stream, uint8_t *rgb_device, int32_t candidates, float *ms_out, int32_t *chosen,
                           float *best_ms);

/* The plain device-to-device copy the rooflines are held against (SURVEY 8d's second denominator): `bytes` (a multiple of 16)
 * copied `iters` times between two buffers of the context's own by a kernel that moves sixteen bytes per lane, in each of a few
 * launch shapes (workgroups per CU, loads in flight, temporal or not: what a copy reaches on this chip depends on them by
 * 20 %); device time per copy in ms of the BEST shape (HIP events on the context's stream).  2 * bytes / ms = the copy rate
 * the chip reaches between these two buffers — a ceiling to hold the decode kernels against, not an average. */
int mj_device_copy_rate(mj_context *ctx, int64_t bytes, int iters, float *ms_per_copy);
/* The shader clock (MHz) the chip held during the context's latest fused launch (MJ_FORM_FUSED) and that launch's duration as
 * its first workgroup saw it: the launch leaves the shader-clock counter and the 100 MHz counter at its start and end.  The
 * launch is power-limited on MI355X, so a time without its clock does not compare across boards.  Zeros: no fused launch yet.
 * Call after the launch has completed (mj_plan_sync). */
int mj_context_launch_clock(mj_context *ctx, float *shader_mhz, float *launch_ms);

/* Test and tuning switches, process-wide.  The defaults are what the library measured as best; the parity tests use the
 * switches to force every form of a stage through the same inputs, the probe scripts to sweep geometries.  The library does
 * NOT read them from the environment (a stray variable must not change how a production decode runs).  Read when a plan is
 * created (forms, orders, chunk sizes) or when it executes (lane geometry).  value NULL or "" = back to the default.
 *   MJ_HUFFMAN        wave | lanes | lanes11 | sync   stage-1 form              MJ_SEG_ORDER     blob | binned | striped
 *   MJ_SYNC_ROUNDS    0..64  repair rounds (classic) / chunks a repair lane may walk on (resolved); 0 = no repairs
 *   MJ_SYNC_CHUNK     256..65536 bytes   MJ_SYNC_WARM   run-up bytes in front of every chunk (half a chunk)
 *   MJ_SYNC_COUNT     classic | resolved   the counting walks of MJ_FORM_SYNC: the round-3 kernel and its repair rounds, or the
 *                     walk on resolved tables with a repair work list (default wherever the batch allows: <= 8 tables, one role each)
 *   MJ_SYNC_BITS      10..13  index bits of those tables (12, fewer if LDS asks for it)
 *   MJ_PROG_BANDS     0 | 1   MJ_PROG_ROWS  frame MCU rows per band   MJ_PROG_FAST  0 | 1 (0 = the general scan walk only)
 *   MJ_PROG_SPLIT     0 | 1 | 2 | 3  refining AC scans as scout + parts: never | by the size of the batch (all of them, then only each
 *                     image's largest with two parts, then none) | always | each image's largest
 *   MJ_PROG_PARTS     1..8  parts per band of a split scan (4)
 *   MJ_PROG_CHUNKS    0 | 1 | 2  the first AC scans of progressive files in self-synchronising chunks, one per lane, in front of the
 *                     band pipeline: never | from 2 048 images on | always;  MJ_PROG_CHUNK  128..65536 bytes per chunk (512)
 *   MJ_PLACE_WINDOW   0 | 1  a placed plan decodes only the source range its canvas needs: never | whenever that is less than the
 *                     images or windows (default: where the caller gave windows; whole images stay whole, see csrc/resize.hip)
 *   MJ_BLUR           passes  the blur ops of a plan with colour operations run one launch per pass through a third canvas, whatever
 *                     the canvas's size (default: only where two planes of the canvas do not fit in LDS, see MJ_COLOUR_GAUSSIAN_BLUR)
 *   MJ_LANES_WAVES    1..16   MJ_LANES_PER_WAVE  1..64 (the 11-bit lane form reads 1 as 2)   MJ_LANES_RING  64 | 128
 *   MJ_STAGE2_CHUNK   1..4096 strips per stage-2 job
 *   MJ_FUSED          0 | 1  (0 = mj_plan_execute always launches the stages separately)
 *   MJ_FUSED_CONSUMERS 0..15  reconstruction wavefronts beside the lane walk of a fused launch (8, or as many as LDS allows)
 *   MJ_FUSED_PRODUCERS 1..8   walking wavefronts of a fused launch (fewer, fuller ones: 272 segments as 6 x 46 lanes instead of 8 x 34)
 *   MJ_FUSED_ACBITS    10..13  index bits of a fused launch's AC tables (12; 11 frees 16 KB of LDS for two more strips)
 *                     (these three: the balance experiments of profiles/r06_fused_balance.txt — measured, defaults unchanged)
 *   MJ_FUSED_PIECE    1..4096  MCUs per job of a row-major fused launch (its jobs are pieces of MCU rows; 20, rounded down to strips)
 *   MJ_FUSED_LUMA13   0 | 1  component 0's AC table of a fused launch with a 13-bit main level (default: only where the segments are
 *                     dealt out by length) or with 12 bits like the others
 *   MJ_FUSED_PATIENCE 0..1000000  polls before a consumer of a fused launch whose jobs cross workgroups gives a job up to the
 *                     clean-up launch (2000; 0: every job that is not ready at once — the tests' way into that path)
 * Returns MJ_ERR_INVALID for a name that is none of these AND for a value outside the range or word list given here (a probe
 * sweep must not report the default under another label); the option then keeps what it had.  Values are copied when they are
 * read: setting an option from one thread while another creates or executes a plan is safe (that plan sees the old or the new
 * value, each option read once).  mj_plan_stage1_form() reports what a plan ended up with. */
int mj_set_option(const char *name, const char *value);
/* The value an option holds ("" = the default) into value_out[cap]; MJ_ERR_INVALID for a name that is no option. */
int mj_get_option(const char *name, char *value_out, int32_t cap);

/* Diagnostic of the fast stage 2 (reference :1561-1573): of the blocks the plan's latest stage-2 execute WITH seam outputs
 * (MJ_FLAG_KEEP_IDCT / MJ_FLAG_KEEP_PLANES) put through the IDCT, counts[0] = all of them, counts[1] = how many the fp32
 * first level could not decide (they went to the fp64 level), counts[2] = how many of those went on to the exact-order
 * routine.  Waits for that execute. */
int mj_plan_idct_levels(mj_plan *plan, uint64_t counts[3]);

/* ---- host-side helper (no GPU needed) -------------------------------------------------------------- */
/* The IDCT table as the library builds it: 4096 doubles laid out [u*8+v][x*8+y], the transpose of the
 * reference's InverseDCT.idct_table (:1541-1553).  Lets CPU tests pin it bit-for-bit. */
void mj_host_idct_table(double *tt);

/* The tap table of one axis of a resized plan, as the library builds it (in_size -> out_size entries): output index i is
 * clip8((2^21 + sum over t < count[i] of taps[i * taps_stride + t] * in[xmin[i] + t]) >> 22); taps behind count[i] are zero.
 * *ksize = taps a row can hold at most (taps_stride must be at least that).  xmin = count = taps = NULL: only *ksize. */
int mj_host_resize_table(int32_t in_size, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps, int32_t taps_stride,
                         int32_t *ksize);
/* mj_host_resize_table for any MJ_FILTER_* (filter MJ_FILTER_BILINEAR: the identical table); taps may be negative.
 * MJ_ERR_INVALID also for a filter that is none of them. */
int mj_host_resize_table_filtered(int32_t filter, int32_t in_size, int32_t out_size, int32_t *xmin, int32_t *count, int32_t *taps,
                                  int32_t taps_stride, int32_t *ksize);
/* mj_host_resize_table_filtered over the part [in0, in1) of the in_size entries — Pillow's precompute_coeffs(in_size, in0, in1,
 * out_size): scale = (in1 - in0) / out_size, centres at in0 + (i + 0.5) * scale, bounds clipped to in_size.  in0 and in1 are
 * rounded to 32-bit floats by the function, as Pillow carries them (mj_plan_request.reducing_gap).  MJ_ERR_INVALID also for a box
 * that is empty or not inside [0, in_size]. */
int mj_host_resize_table_boxed(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size, int32_t *xmin, int32_t *count,
                               int32_t *taps, int32_t taps_stride, int32_t *ksize);
/* mj_plan_request.reducing_gap's factors for a src_w x src_h image resized to dst_w x dst_h (host only).  MJ_ERR_INVALID: a size
 * outside 1..65535, a gap that is not a finite number >= 1.0, NULL. */
int mj_host_reduce_factors(int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h, double gap, int32_t *fx, int32_t *fy);
/* The reduce kernel's arithmetic on a row-major (h, w, ncomp) array (host only): out = the (ceil(h / fy), ceil(w / fx), ncomp) reduced
 * image.  phase_x / phase_y: 0 — cell boundaries at k * f, the partial cell last, Image.reduce itself — or size mod f: boundaries
 * at phase + k * f, the partial cell first (what the kernel does along an axis the orientation reverses).  MJ_ERR_INVALID: NULL,
 * a size outside 1..65535, ncomp neither 1 nor 3, a factor below 1, fx * fy above 65536, any other phase. */
int mj_host_reduce(const uint8_t *src, int32_t w, int32_t h, int32_t ncomp, int32_t fx, int32_t fy, int32_t phase_x, int32_t phase_y,
                   uint8_t *out);
/* The output table of one component of a plan with mj_plan_request.output, as the library builds it (host only, no context): out
 * = 256 elements of `dtype` (MJ_DTYPE_F16 / BF16: 2 bytes each, MJ_DTYPE_F32: 4), element v what resized byte v is stored as with
 * this mean and std (mean 0, std 1 = no normalisation).  MJ_ERR_INVALID: MJ_DTYPE_U8 or an unknown dtype, NULL, a mean that is
 * not finite, a std that is not finite or not > 0. */
int mj_host_normalize_table(int32_t dtype, float mean, float std, void *out);

/* ---- host front end (no GPU work, no context) -------------------------------------------------------
 * Header parse + batch assembly for the everyday case, on host threads: what pyjpegdecoder_amd/_parse.py
 * (parse_jpeg(headers_only=True): the reference's marker loop :78-110 and its SOF0/DHT/DQT/DRI/SOS handlers
 * :112-650, stopped at the SOS) and batch.prepare_batch do in Python, file by file.  For every file: walk the
 * segments in front of the scan, copy the file to blob + file_off[i], fill images[i] and its one byte range
 * (seg_begin[i] = first entropy-coded byte, seg_end[i] = end of the file: the arrays of a MJ_FLAG_GPU_SEGMENT
 * batch), and number the distinct Huffman / quantisation tables of the batch in order of first use.
 *
 * Accepted: SOF0, 8 bit, 1 or 3 components, a first SOS naming every frame component in frame order, with only
 * APPn / COM / DQT / DHT / DRI / SOF0 segments in front of it.  Everything else (progressive, scans of single
 * components, DNL, unknown markers, short or inconsistent headers) is not diagnosed here: the call returns
 * MJ_HOST_DECLINED with declined_file = the first such file and the caller runs the full marker loop, which
 * raises what the reference raises.  All arrays are the caller's (mj_image_desc images[n_files], int64
 * seg_begin/seg_end[n_files], huff[huff_cap], qt[qt_cap * 64]; 6 / 3 per file always suffice); file_off must be
 * ascending multiples of 4 with file_off[i] + sizes[i] <= file_off[i + 1] (blob_len for the last); the gaps and the
 * tail of the blob are zeroed (stage 1 reads ahead of a segment's end). */
#define MJ_HOST_DECLINED 1
typedef struct {
    int32_t n_files;
    const uint8_t *const *files;          /* in: the files' bytes                                             */
    const int64_t *sizes;                 /* in                                                                */
    const int64_t *file_off;              /* in: blob offset of every file                                     */
    uint8_t *blob;                        /* out: host buffer of blob_len bytes                                */
    int64_t blob_len;
    mj_image_desc *images;                /* out                                                               */
    int64_t *seg_begin, *seg_end;         /* out                                                               */
    mj_huff_spec *huff;                   /* out */
    int32_t huff_cap;
    uint16_t *qt;                         /* out: zig-zag order, like mj_batch.qt                              */
    int32_t qt_cap;
    int32_t n_threads;                    /* in: host threads to use (>= 1)                                    */
    int32_t n_huff, n_qt;                 /* out: distinct tables written                                      */
    int32_t declined_file;                /* out: -1, or the first file this front end does not take           */
    uint8_t *skip;                        /* in, optional: n_files bytes.  Non-NULL: files the front end does not take are
                                             marked 1 here and left out (their slot in the blob stays zeroed) instead of
                                             ending the call; the output arrays then hold the accepted files only, in order */
    int32_t n_accepted;                   /* out: files assembled (= n_files without `skip`)                   */
} mj_host_job;
int mj_host_assemble(mj_host_job *job);

/* The EXIF Orientation tag of n_files files on host threads (host only, no context): out[i] = 1..8.  File i is files[i], or —
 * files == NULL — blob + offsets[i]; lengths[i] bytes either way.  Read: the marker segments in front of the first SOS, the first
 * APP1 whose payload starts "Exif\0\0", its TIFF header (II or MM), tag 0x0112 of IFD0 as one SHORT.  Declines nothing: 1 when
 * there is no such tag, its value is outside 1..8, or anything is malformed or truncated; never reads outside a segment.
 * pyjpegdecoder_amd.exif_orientation is the specification. */
int mj_host_exif_orientations(const uint8_t *const *files, const uint8_t *blob, const int64_t *offsets, const int64_t *lengths,
                              int32_t n_files, int32_t n_threads, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* MIJPEG_H */
