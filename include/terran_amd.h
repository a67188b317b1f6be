/* terran_amd.h -- C ABI of the MI355X-native (gfx950) per-frame human-perception path.
 *
 * This is the drop-in boundary for Terran's three model wrappers: the functions below
 * are exactly what a binding for the reference's plugin classes
 *
 *     terran/face/detection/retinaface/wrapper.py:92-238   class RetinaFace  (.call)
 *     terran/face/recognition/arcface/wrapper.py:102-184   class ArcFace     (.call)
 *     terran/pose/openpose/wrapper.py:166-485              class OpenPose    (.call)
 *
 * (selected through the checkpoint registry, terran/checkpoint.py:29-103,213-245) calls
 * instead of running torch.nn graphs + torch/numpy post-processing.  `terran_amd/` holds the
 * ctypes binding and the Python mirror of those classes; INTEGRATION.md shows the registry
 * entries a Terran maintainer would add.
 *
 * Conventions
 *   - plain C: opaque handles, pointers and sizes only; no exceptions cross the ABI.
 *   - every function returns TA_OK (0) or a negative TA_E_* code; ta_last_error(ctx) holds the text.
 *   - all pointers are HOST memory unless the name ends in _dev.
 *   - variable-length results use caller-allocated arrays with a `capacity` (in objects) and a
 *     `required` out-value; TA_E_CAPACITY is returned (nothing truncated silently) when too small.
 *   - one ta_ctx per GPU; a ctx and everything created from it belong to ONE host thread.
 *   - there is NO CPU fallback: every entry point fails with TA_E_DEVICE when no gfx950 device
 *     is usable.  One exception: ta_jpeg_coefficients (the host half of the JPEG decoder, no pixels)
 *     needs no context and no device.
 */
#ifndef TERRAN_AMD_H
#define TERRAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TA_OK 0
#define TA_E_INVALID (-1)   /* bad argument / malformed model blob            */
#define TA_E_DEVICE (-2)    /* HIP error, no device, or out of device memory  */
#define TA_E_CAPACITY (-3)  /* caller-provided result arrays are too small    */
#define TA_E_OVERFLOW (-4)  /* an addressing limit was hit (ta_openpose_run: more than 65535 peaks of ONE body part in one image) */
#define TA_E_RANGE (-5)     /* f16x3 / f16x2 / f16 arithmetic modes only: an activation left the half-float range (stored |x| > 65504, inf
                             * or NaN; tensors are stored times a pack-time power of two that puts the expected maximum near 2^10);
                             * no numbers are returned -- run the input on a model packed for f32 (or bf16x3).  Checked on every tensor
                             * some op READS; final float32 results no op reads (embeddings, detector heads) are not range-checked */

#define TA_MODEL_RETINAFACE 1
#define TA_MODEL_ARCFACE 2
#define TA_MODEL_OPENPOSE 3

typedef struct ta_ctx ta_ctx;       /* one per device: stream, scratch, error text           */
typedef struct ta_model ta_model;   /* packed weights + op program + per-shape activation plan */
typedef struct ta_frames ta_frames; /* a batch of uint8 RGB frames resident in HBM (N,H,W,3)   */

/* ---- context -------------------------------------------------------------------------- */
const char* ta_version(void);
int ta_device_count(void);
/* PCI address ("0000:c1:00.0") of a device: what the host side needs to find the NUMA node / local CPUs of a GPU in sysfs
 * (terran_amd/affinity.py binds a rank's or a lane's host threads and pinned staging to them).  capacity >= 16. */
int ta_device_pci_bus_id(int device_id, char* out, int capacity);
int ta_ctx_create(int device_id, ta_ctx** out);
void ta_ctx_destroy(ta_ctx* ctx);
const char* ta_last_error(const ta_ctx* ctx);
int ta_ctx_sync(ta_ctx* ctx);
/* Per-kernel-class HIP-event timing (bench.py `roofline`): enable, run, then read.
 * klass: 0 = implicit-GEMM conv, 1 = depthwise/pool/elementwise, 2 = pre-processing,
 * 3 = post-processing.  ms = summed event time, launches = #kernels, work = algorithmic
 * FLOP (klass 0) or bytes (others) summed over those launches. */
int ta_profile_enable(ta_ctx* ctx, int on);
int ta_profile_reset(ta_ctx* ctx);
int ta_profile_read(ta_ctx* ctx, int klass, double* ms, int64_t* launches, double* work);
/* Event pair on the ctx stream (whole-step timing). */
int ta_timer_start(ta_ctx* ctx);
int ta_timer_stop(ta_ctx* ctx, double* ms);

/* Pinned (page-locked) host memory for staging frame batches: H2D copies from it run at full PCIe rate and
 * overlap with kernels of other contexts (terran/io/video/reader.py:88-117 hands over pageable numpy batches). */
int ta_host_alloc(ta_ctx* ctx, size_t bytes, void** out);
void ta_host_free(ta_ctx* ctx, void* ptr);

/* ---- frames (replaces `torch.as_tensor(images, device=...)`,
 *      retinaface/wrapper.py:144, openpose/wrapper.py:121, arcface/wrapper.py:170) -------- */
int ta_frames_upload(ta_ctx* ctx, const uint8_t* nhwc_rgb, int n, int h, int w, ta_frames** out);
int ta_frames_alloc(ta_ctx* ctx, int n, int h, int w, ta_frames** out);
int ta_frames_shape(const ta_frames* f, int* n, int* h, int* w);
int ta_frames_download(const ta_frames* f, uint8_t* nhwc_rgb);
/* Releases the handle.  The device buffer is parked in its context (a few recent sizes, bounded in bytes) and handed
 * to the next batch of the same size: the steady state of a video loop performs no hipMalloc / hipFree (a hipFree
 * waits for every stream of the process).  Parked buffers are freed with the context. */
void ta_frames_free(ta_frames* f);
/* cv2.resize(..., INTER_LINEAR) semantics on the device
 * (face/detection/__init__.py:33-38, pose/openpose/wrapper.py:106-111). */
int ta_frames_resize(ta_ctx* ctx, const ta_frames* src, int dst_h, int dst_w, ta_frames** out);
/* Pillow Image.resize(size, resample=BICUBIC) of every image of the batch (arcface/wrapper.py:83-85, the no-landmark
 * crop path): the pixels are ta_frames_resample's for one whole-frame region per image and TA_RESAMPLE_BICUBIC, without
 * its 16384 cap on a side.  An empty batch gives an empty (0, dst_h, dst_w) batch.  TA_E_INVALID, before anything is
 * allocated: a null argument, dst_h or dst_w <= 0, a batch of another device, or a size the launches do not cover --
 * more than 65535 workgroups along y (dst_h above 4 x 65535, or a resized width with more than 16 x 65535 source rows),
 * 2^32 threads or more along x (n * ceil(dst_w / 64) * 256), axis tables of 2^32 entries or more. */
int ta_frames_resize_bicubic(ta_ctx* ctx, const ta_frames* src, int dst_h, int dst_w, ta_frames** out);
/* Zero-pad `src` image `src_index` into image `dst_index` of `dst` at (top, left)
 * (merge_in, face/detection/__init__.py:96-139 / pose/__init__.py:48-88). */
int ta_frames_paste(ta_ctx* ctx, const ta_frames* src, int src_index, ta_frames* dst, int dst_index,
                    int top, int left);

/* ---- drawing (terran/vis/pillow.py: vis_faces / vis_poses) ----------------------------- */
/* Draws an ordered list of primitives into `frames` in place, Pillow's ImageDraw.Draw(img, 'RGBA') semantics bit for bit:
 * ink blended as DIV255(in * (255 - a) + ink * a), each pixel once per primitive, everything clipped to the frame.  Where
 * primitives of one frame overlap, a pixel sees them in list order; primitives of different frames may be interleaved.
 *   TA_DRAW_BAR   filled axis-aligned rectangle, pixels x0..x1 x y0..y1 inclusive (x1 >= x0, y1 >= y0).  A rectangle
 *                 outline of alpha 255 (draw.rectangle(outline=, width=)) is a set of bars.
 *   TA_DRAW_LINE  draw.line([x0, y0, x1, y1], width=width): width <= 1 is the thin Bresenham line (both end points
 *                 drawn), a wider one the quadrilateral Pillow builds around the segment (coincident end points: one pixel).
 *   TA_DRAW_DISC  draw.ellipse([x0, y0, x1, y1], fill=): the filled ellipse in that box (x1 >= x0, y1 >= y0; the
 *                 box's width and height at most 32768).
 *   TA_DRAW_MASK  draw.text's bitmap (ta_frames_draw_masks only): an 8-bit coverage bitmap whose top-left pixel lies at
 *                 (x0, y0) and whose bottom-right one at (x1, y1), blended per pixel as DIV255(in * (255 - m) + ink * m)
 *                 with the primitive's rgb; alpha must be 255.  A pixel whose coverage is 0 is left untouched.
 * Coordinates are pixels (what Pillow's int() of the float coordinates gives), |coordinate| <= 2^24.  The call runs on
 * `ctx`'s stream (a batch of another context on the same device may be drawn into) and returns when the drawing is done.
 * TA_E_INVALID: frame index out of range, unknown kind, inverted box, negative width, coordinate out of range. */
#define TA_DRAW_BAR 0
#define TA_DRAW_LINE 1
#define TA_DRAW_DISC 2
#define TA_DRAW_MASK 3
typedef struct ta_draw_prim {
  int32_t frame;       /* image index in the batch                  */
  int32_t kind;        /* TA_DRAW_*                                 */
  int32_t x0, y0, x1, y1;
  int32_t width;       /* TA_DRAW_LINE: width; TA_DRAW_MASK: byte offset of the bitmap in `masks` */
  uint8_t rgba[4];     /* ink and alpha                             */
} ta_draw_prim;
int ta_frames_draw(ta_ctx* ctx, ta_frames* frames, const ta_draw_prim* prims, int n);
/* ta_frames_draw with TA_DRAW_MASK primitives among the others.  `masks` is a host buffer of `mask_bytes` bytes that holds
 * the coverage bitmaps: a mask primitive's `width` is the byte offset of its first row, rows are packed (pitch
 * x1 - x0 + 1).  Any number of primitives, of any frames, may name the same bitmap.  The buffer travels to the device in
 * the staging copy of the primitives.  TA_E_INVALID, before anything is drawn: what ta_frames_draw refuses, a mask
 * primitive of alpha other than 255, a negative offset, a bitmap that reaches past `mask_bytes`, `masks` NULL with a mask
 * primitive present.  (ta_frames_draw itself takes no masks: TA_DRAW_MASK is an unknown kind there.) */
int ta_frames_draw_masks(ta_ctx* ctx, ta_frames* frames, const ta_draw_prim* prims, int n, const uint8_t* masks,
                         size_t mask_bytes);

/* ---- blurring regions (anonymising faces) ---------------------------------------------- */
/* Blurs rectangles of `frames` in place, Pillow's
 *     region = im.crop(box).filter(ImageFilter.GaussianBlur(radius)); im.paste(region, box)
 * bit for bit: three box-blur passes along the rows, then three along the columns, each rounded to uint8, the weights
 * derived from `radius` in float32 as libImaging does.  The blur sees only the region's own pixels (edges are extended at
 * the region's border, not the frame's).  The box [x0, x1) x [y0, y1) is half-open and must lie inside the frame.
 *   TA_BLUR_BOX      every pixel of the box takes its blurred value.
 *   TA_BLUR_ELLIPSE  only the pixels of ImageDraw.ellipse([0, 0, w - 1, h - 1], fill=) in the box do (TA_DRAW_DISC's
 *                    coverage; a 1 x 1 box has none); the blur itself is still computed over the whole box.
 * radius = 0 leaves the region as it is.  Regions of one frame are applied in list order: a later one blurs what an
 * earlier one it overlaps left; regions of different frames may be interleaved.  The library sorts the regions into rounds
 * of pairwise disjoint ones (the usual case: one round) and runs two kernels per round.  The call runs on `ctx`'s stream
 * (a batch of another context on the same device may be blurred) and returns when it is done.  n = 0: TA_OK.
 * TA_E_INVALID, before any pixel changes: frame index out of range; a box that is empty, inverted or not inside the
 * frame, or has a side longer than 16384; unknown shape; a radius that is negative, NaN, infinite or above 1024. */
#define TA_BLUR_BOX 0
#define TA_BLUR_ELLIPSE 1
typedef struct ta_blur_region {
  int32_t frame;       /* image index in the batch                  */
  int32_t x0, y0, x1, y1;
  int32_t shape;       /* TA_BLUR_*                                 */
  float radius;        /* GaussianBlur's radius (a standard deviation, in pixels) */
} ta_blur_region;
int ta_frames_blur(ta_ctx* ctx, ta_frames* frames, const ta_blur_region* regions, int n);
/* HOST ONLY, no context: what ta_frames_blur derives from the regions before it launches anything.  rounds[i]: the round
 * region i runs in (one more than the latest round of an earlier region of its frame that it intersects).
 * box_radius[i]: the fractional radius of the box passes; weights[2 i], weights[2 i + 1]: the 2^-24 fixed-point weights
 * of a window pixel and of the two pixels beside the window.  Any output may be NULL.  Frame indices only group the
 * regions here.  TA_E_INVALID: an empty or inverted box, an unknown shape, a bad radius. */
int ta_blur_plan(const ta_blur_region* regions, int n, int32_t* rounds, float* box_radius, uint32_t* weights);

/* ---- resampling regions (face chips, resizing, pixelation) -------------------------------- */
/* Pillow's Image.resize(size, filter, box=) on uint8 RGB, bit for bit (libImaging ImagingResample: two passes of 2^22
 * fixed-point convolution, the horizontal one first and rounded to uint8; NEAREST: the affine scaler, whose source
 * coordinate starts at b0 + step / 2 and is advanced by adding step = (b1 - b0) / out).  The filter codes are Pillow's. */
#define TA_RESAMPLE_NEAREST 0
#define TA_RESAMPLE_LANCZOS 1
#define TA_RESAMPLE_BILINEAR 2
#define TA_RESAMPLE_BICUBIC 3
#define TA_RESAMPLE_BOX 4
#define TA_RESAMPLE_HAMMING 5
typedef struct ta_resample_region {
  int32_t frame;         /* image index in the batch                  */
  float x0, y0, x1, y1;  /* Pillow's box=: fractional source rectangle */
} ta_resample_region;
/* *out: a NEW batch (n, out_h, out_w, 3), owned by `ctx`; image i is
 *     Image.fromarray(src[regions[i].frame]).resize((out_w, out_h), filter, box=regions[i] box)
 * Regions may name the frames in any order and any frame any number of times.  One horizontal and one vertical launch
 * serve all regions; a pass is skipped for a region where Pillow skips it (same size and the box over the whole axis).
 * The horizontal results (only the source rows the vertical pass reads) live in the context's scratch.  Returns when done.
 * n = 0: TA_OK and *out = NULL.  TA_E_INVALID, before any launch (*out = NULL): n < 0; unknown filter; out_h or out_w
 * outside 1 .. 16384; a frame index out of range; a box that is not 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H (Pillow's rule). */
int ta_frames_resample(ta_ctx* ctx, const ta_frames* src, const ta_resample_region* regions, int n, int out_h, int out_w,
                       int filter, ta_frames** out);
/* HOST ONLY, no context: one axis' tables exactly as ta_frames_resample derives them for an axis it does not skip.
 * bounds[2 i], bounds[2 i + 1]: first source sample and number of taps of output sample i; coefs[i * *ksize + t]: the
 * 2^22 fixed-point weight of tap t (0 beyond the count).  NEAREST: one tap of weight 2^22.  b0, b1 are rounded to
 * float32 first (the box is float32 in Pillow).  *ksize is set whenever the arguments are valid; TA_E_CAPACITY when
 * out_size * *ksize > capacity (nothing else written: call with capacity 0 to size the arrays).  TA_E_INVALID:
 * in_size <= 0, out_size outside 1 .. 16384, unknown filter, a box that is not 0 <= b0 < b1 <= in_size, a null pointer. */
int ta_resample_plan(int in_size, double b0, double b1, int out_size, int filter, int32_t* bounds, int32_t* coefs,
                     int capacity, int* ksize);

/* Pixelates rectangles of `frames` in place, Pillow's
 *     w, h = box size; sw, sh = max(1, w // block), max(1, h // block)
 *     im.paste(im.crop(box).resize((sw, sh), BOX).resize((w, h), NEAREST), box)
 * bit for bit.  Regions are as ta_frames_blur takes them: a half-open box inside the frame, TA_BLUR_BOX or
 * TA_BLUR_ELLIPSE (only the pixels of ImageDraw.ellipse([0, 0, w - 1, h - 1], fill=) are replaced), applied in list
 * order where they overlap within a frame (rounds of pairwise disjoint regions, three launches per round).  block = 1
 * leaves the region as it is.  n = 0: TA_OK.  TA_E_INVALID, before any pixel changes: as for ta_frames_blur, or a block
 * outside 1 .. 16384. */
typedef struct ta_pixelate_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  int32_t block;         /* side of a mosaic cell, in pixels          */
} ta_pixelate_region;
int ta_frames_pixelate(ta_ctx* ctx, ta_frames* frames, const ta_pixelate_region* regions, int n);

/* ---- transforming frames (rotation, flips, affine and perspective warps) ------------------- */
/* Pillow's Image.transform(size, method, data, resample, fillcolor=) on uint8 RGB, bit for bit (libImaging Geometry.c).
 * `a` is Pillow's `data`: it maps OUTPUT pixel centres to INPUT coordinates, in double without fused multiply-adds:
 *     xin = x + 0.5, yin = y + 0.5;  xs = a0 xin + a1 yin + a2,  ys = a3 xin + a4 yin + a5
 *     PERSPECTIVE: both divided by a6 xin + a7 yin + 1
 * A pixel whose point fails 0 <= xs < W && 0 <= ys < H gets the fill colour.  BILINEAR / BICUBIC: 2 x 2 / 4 x 4 taps
 * around (xs - 0.5, ys - 0.5), clipped to the image, interpolated in double, truncated (bicubic: clamped first).
 * NEAREST takes Pillow's routes: an affine map with a1 == a3 == 0 its scaler (coordinates accumulated by adding a0, a4),
 * another affine map 16.16 fixed point while its output corners stay below 32768 and accumulated doubles beyond (one
 * thread per output row: slow, and of no practical use), PERSPECTIVE (int) of the double point.
 * Where Pillow is undefined (it converts non-finite or out-of-range doubles to int: a perspective denominator of exactly 0
 * at a pixel centre, NEAREST coordinates of 2^31 or more) the result here is defined and differs: every point is
 * range-tested in double first and one that is not inside, NaN included, gets the fill colour. */
#define TA_TRANSFORM_AFFINE 0      /* Pillow's Image.AFFINE      : a[0..5] (a[6], a[7] are not read) */
#define TA_TRANSFORM_PERSPECTIVE 2 /* Pillow's Image.PERSPECTIVE : a[0..7] */
typedef struct ta_transform_region {
  int32_t frame;  /* image index in the batch */
  int32_t method; /* TA_TRANSFORM_*           */
  double a[8];    /* Pillow's `data`          */
} ta_transform_region;
/* *out: a NEW batch (n, out_h, out_w, 3), owned by `ctx`; image i is
 *     Image.fromarray(src[r.frame]).transform((out_w, out_h), r.method, r.a, resample=filter, fillcolor=fill), r = regions[i]
 * fill_rgb = NULL is fillcolor=None (zeros).  filter: TA_RESAMPLE_NEAREST, _BILINEAR or _BICUBIC.  Regions may name the
 * frames in any order and any frame any number of times; one launch serves all of them (a second one only for NEAREST
 * regions on the accumulated-double route).  Returns when done.
 * n = 0: TA_OK and *out = NULL.  TA_E_INVALID, before any launch (*out = NULL): n < 0; another filter; out_h or out_w
 * outside 1 .. 16384; a frame index out of range; an unknown method; a coefficient the method reads that is not finite. */
int ta_frames_transform(ta_ctx* ctx, const ta_frames* src, const ta_transform_region* regions, int n, int out_h, int out_w,
                        int filter, const uint8_t* fill_rgb, ta_frames** out);
/* Pillow's Image.transform(size, MESH, [(box, quad), ...], resample, fillcolor=) -- and with it QUAD, a mesh of the one cell
 * ((0, 0, out_w, out_h), quad), and ImageOps.deform -- on uint8 RGB, bit for bit.  A cell maps its `box` of the OUTPUT
 * (half-open, ints) onto the quadrilateral `quad` of the INPUT, corners in Pillow's order nw, sw, se, ne, (x, y) each.
 * In double, unfused, left to right, with w = x1 - x0, h = y1 - y0, As = 1.0 / w, At = 1.0 / h:
 *     a0 = nw.x, a1 = (ne.x - nw.x) * As, a2 = (sw.x - nw.x) * At, a3 = (se.x - sw.x - ne.x + nw.x) * As * At
 *     a4 = nw.y, a5 = (ne.y - nw.y) * As, a6 = (sw.y - nw.y) * At, a7 = (se.y - sw.y - ne.y + nw.y) * As * At
 * The box is clamped to the output, cx0 = max(x0, 0), cy0 = max(y0, 0), cx1 = min(x1, out_w), cy1 = min(y1, out_h), and
 * for every pixel (x, y) of the clamped box
 *     xin = (x - cx0) + 0.5, yin = (y - cy0) + 0.5          (relative to the CLAMPED origin while w, h are the unclamped
 *     xs = a0 + a1 xin + a2 yin + a3 xin yin                  box's: Pillow's behaviour for a box that starts left of or
 *     ys = a4 + a5 xin + a6 yin + a7 xin yin                  above the output)
 * A point with 0 <= xs < W && 0 <= ys < H gives the pixel the filter's sample there, the taps of ta_frames_transform's
 * PERSPECTIVE route (NEAREST: (int) of the point).  A point outside makes the pixel 0 without a fill colour and leaves it
 * as it is with one.  The output starts as the fill colour (zeros without one) and the cells apply in list order: they may
 * overlap, leave gaps and reach outside the output.  Non-finite points count as outside, as in ta_frames_transform. */
typedef struct ta_mesh_cell {
  int32_t x0, y0, x1, y1; /* the cell's box of the output, half-open            */
  double quad[8];         /* nw.x, nw.y, sw.x, sw.y, se.x, se.y, ne.x, ne.y     */
} ta_mesh_cell;
typedef struct ta_mesh_image {
  int32_t frame; /* image index in the batch                           */
  int32_t mesh;  /* which mesh warps it: cells mesh_first[mesh] .. mesh_first[mesh + 1] - 1 */
} ta_mesh_image;
/* The output is cut into tiles of TA_MESH_TILE_W x TA_MESH_TILE_H pixels, one workgroup each; the host bins every mesh's
 * cells into the tiles their clamped boxes touch. */
#define TA_MESH_TILE_W 64
#define TA_MESH_TILE_H 16
#define TA_MESH_MAX_CELLS (1 << 20)   /* cells of one call                                           */
#define TA_MESH_MAX_ENTRIES (1 << 24) /* of one call: (cell, tile) pairs, and n_meshes x tiles + 1   */
/* *out: a NEW batch (n_images, out_h, out_w, 3), owned by `ctx`; image i is
 *     Image.fromarray(src[images[i].frame]).transform((out_w, out_h), MESH, the cells of mesh images[i].mesh, filter, fillcolor=fill)
 * mesh_first: n_meshes + 1 ascending offsets into `cells`.  A mesh is built, binned and staged once per call, however many
 * images share it; ONE launch serves all images, and every pixel is written once: a lane walks its tile's cells from the
 * last to the first and takes the first whose clamped box holds its pixel (with a fill colour: and whose point lies inside
 * the source), else the fill.  fill_rgb = NULL is fillcolor=None.  filter: TA_RESAMPLE_NEAREST, _BILINEAR or _BICUBIC.
 * Images may name frames and meshes in any order and any number of times; a mesh may be empty.  Returns when done.
 * n_images = 0: TA_OK and *out = NULL.  TA_E_INVALID, before any launch (*out = NULL): a negative count; another filter;
 * out_h or out_w outside 1 .. 16384; offsets that do not ascend from >= 0 to <= n_cells; a box with x1 <= x0 or y1 <= y0
 * (Pillow divides by zero or draws nothing there) or a coordinate beyond +-2^24; a corner that is not finite; a frame or
 * mesh index out of range; more than TA_MESH_MAX_CELLS cells; more than TA_MESH_MAX_ENTRIES tile entries.  A box partly or
 * wholly outside the output is valid. */
int ta_frames_transform_mesh(ta_ctx* ctx, const ta_frames* src, const ta_mesh_cell* cells, int n_cells, const int32_t* mesh_first,
                             int n_meshes, const ta_mesh_image* images, int n_images, int out_h, int out_w, int filter,
                             const uint8_t* fill_rgb, ta_frames** out);
/* HOST ONLY, no context: what ta_frames_transform_mesh derives from ONE mesh and an output size before it launches anything.
 * coefs[8 i .. 8 i + 7]: a0 .. a7 of cell i; boxes[4 i .. 4 i + 3]: its clamped box cx0, cy0, cx1, cy1 (empty when the
 * cell lies outside the output); tile_first[t], t = 0 .. tiles (tiles = ceil(out_w / TA_MESH_TILE_W) x
 * ceil(out_h / TA_MESH_TILE_H), row-major): tile t's cells are tile_cells[tile_first[t] .. tile_first[t + 1] - 1], in list
 * order.  Any output may be NULL.  *n_entries is set whenever the arguments are valid; TA_E_CAPACITY when it exceeds
 * `capacity` (nothing else written: call with capacity 0 to size tile_cells).  TA_E_INVALID: what ta_frames_transform_mesh
 * refuses about cells and output size. */
int ta_mesh_plan(const ta_mesh_cell* cells, int n_cells, int out_h, int out_w, double* coefs, int32_t* boxes, int32_t* tile_first,
                 int32_t* tile_cells, int capacity, int* n_entries);
/* Image.transpose(op) of every image of the batch into a NEW batch, owned by `ctx`: (n, h, w, 3) for the flips and
 * ROTATE_180, (n, w, h, 3) for the four ops that swap the axes (ROTATE_90 is counter-clockwise, as in Pillow).  The op
 * codes are Pillow's.  One launch, a tiled copy through LDS.  TA_E_INVALID (*out = NULL): an unknown op. */
#define TA_FLIP_LEFT_RIGHT 0
#define TA_FLIP_TOP_BOTTOM 1
#define TA_ROTATE_90 2
#define TA_ROTATE_180 3
#define TA_ROTATE_270 4
#define TA_TRANSPOSE 5
#define TA_TRANSVERSE 6
int ta_frames_transpose(ta_ctx* ctx, const ta_frames* src, int op, ta_frames** out);

/* ---- pixel values: histograms, look-up tables, saturation ---------------------------------- */
/* Regions of the three calls below are as ta_frames_blur takes them: a half-open box [x0, x1) x [y0, y1) inside the
 * frame, no side longer than 16384, TA_BLUR_BOX or TA_BLUR_ELLIPSE (only the pixels of
 * ImageDraw.ellipse([0, 0, w - 1, h - 1], fill=) in the box count or change; a 1 x 1 box has none).  Every call runs on
 * `ctx`'s stream (a batch of another context on the same device may be passed) and returns when it is done.  n = 0:
 * TA_OK.  TA_E_INVALID, before any launch, any changed pixel and any written output: a frame index out of range; a box
 * that is empty, inverted, not inside the frame or has a side longer than 16384; an unknown shape; and what each call adds.
 *
 * Histogram of every region, Pillow's
 *     TA_HIST_RGB  im.crop(box).histogram(mask)                768 counts: R bins, G bins, B bins
 *     TA_HIST_L    im.crop(box).convert('L').histogram(mask)   256 counts of (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 * into the HOST array hist[n][768 or 256] (mask: the shape's coverage).  Regions only read: they may overlap, repeat and
 * name the frames in any order; a clear and one launch serve them all.  Counts are integers, so the result does not
 * depend on the order of accumulation.  TA_E_INVALID also: an unknown mode, hist = NULL. */
#define TA_HIST_RGB 0
#define TA_HIST_L 1
typedef struct ta_hist_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
} ta_hist_region;
int ta_frames_histogram(ta_ctx* ctx, const ta_frames* frames, const ta_hist_region* regions, int n, int mode, uint32_t* hist);

/* Applies look-up tables to regions of `frames` in place, Pillow's
 *     im.paste(im.crop(box).point(lut), box)             under the ellipse shape only the ellipse's pixels change
 * `luts`: a HOST array of n_luts tables of 768 bytes, Pillow's point() argument for RGB (R table, G table, B table);
 * region i uses table regions[i].lut.  Regions of one frame apply in list order where they overlap (rounds of pairwise
 * disjoint regions, one launch per round).  TA_E_INVALID also: a `lut` outside 0 .. n_luts - 1, luts = NULL. */
typedef struct ta_point_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  int32_t lut;           /* index into `luts`                         */
} ta_point_region;
int ta_frames_point(ta_ctx* ctx, ta_frames* frames, const ta_point_region* regions, int n, const uint8_t* luts, int n_luts);

/* Blends every pixel of the regions with its own luma in place, Pillow's
 *     im.paste(ImageEnhance.Color(im.crop(box)).enhance(factor), box)
 * bit for bit: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, then per band Image.blend's float32 expression
 * L + factor * (v - L), a multiply and an add, never fused: truncated when 0 <= factor <= 1, clipped to 0 .. 255 first
 * otherwise; factor 0 is convert('L').convert('RGB'), factor 1 leaves the region as it is.  Order and rounds are
 * ta_frames_point's.  TA_E_INVALID also: a factor that is NaN or infinite. */
typedef struct ta_saturate_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  float factor;          /* ImageEnhance.Color's                      */
} ta_saturate_region;
int ta_frames_saturate(ta_ctx* ctx, ta_frames* frames, const ta_saturate_region* regions, int n);

/* ---- colour: matrices, YCbCr and HSV conversions, 3-D look-up tables ------------------------- */
/* Converts the colours of regions of `frames` in place, Pillow's
 *     im.paste(X(im.crop(box)), box)                      under the ellipse shape only the ellipse's pixels change
 * bit for bit, where X is the region's op, ops[regions[i].op]:
 *     TA_COLOR_MATRIX     convert('RGB', m): the 12 floats at tables[table ..], row by row.  Per band, in float32 with
 *                         every multiply and add rounded on its own: v = m0 r + m1 g + m2 b + m3 (left to right), v + 0.5;
 *                         0 if v <= 0, 255 if v >= 255, else truncated
 *     TA_COLOR_RGB2YCBCR  convert('YCbCr'): libImaging's int16 tables at 6 fractional bits, entry (int)(c 64 i + 0.5),
 *                         (T_R[r] + T_G[g] + T_B[b]) >> 6, + 128 for Cb and Cr
 *     TA_COLOR_YCBCR2RGB  convert('RGB') of a 'YCbCr' image: the inverse tables over i - 128, clipped to 0 .. 255
 *     TA_COLOR_RGB2HSV    convert('HSV'): V = max, S = (max - min) / max and H from float32 quotients, each times 255
 *                         and truncated
 *     TA_COLOR_HSV2RGB    convert('RGB') of an 'HSV' image
 *     TA_COLOR_LUT3D      filter(ImageFilter.Color3DLUT(size, table)), 3 channels in and out: size = (s0, s1, s2), every
 *                         axis 2 .. 65; the 3 s0 s1 s2 floats at tables[table ..] as Pillow stores them, R fastest:
 *                         entry 3 (r + s0 (g + s1 b)) + channel.  The table is quantised on the host as libImaging does
 *                         it (the float32 product t * 16320, rounded half away from zero, saturated at +-32767); a node
 *                         travels as four int16 (8 bytes).  Trilinear interpolation in integers along R, then G, then B.
 *                         A table of at most 65536 bytes of nodes (up to 20^3) is held in LDS, a larger one is read
 *                         through the cache.
 * A batch carries three bytes per pixel and NO mode: after RGB2YCBCR the three bytes of a pixel are Y, Cb, Cr, after
 * RGB2HSV they are H, S, V, and every other call goes on treating them as R, G, B.  The caller keeps track of what a
 * region holds, as a Pillow image's mode does.
 * Regions are as ta_frames_point takes them (half-open box inside the frame, no side longer than 16384, TA_BLUR_BOX or
 * TA_BLUR_ELLIPSE); ops of different kinds may be mixed in one call.  Regions of one frame apply in list order where they
 * overlap (rounds of pairwise disjoint regions, one launch per round); regions of different frames may be interleaved.
 * `tables`: a HOST array of n_tables floats, read by the MATRIX and LUT3D ops; records and tables travel in one staging
 * copy.  The call runs on `ctx`'s stream (a batch of another context on the same device may be passed) and returns when it
 * is done.  n = 0: TA_OK.
 * TA_E_INVALID, before any launch and any changed pixel, naming the region or the op: what ta_frames_point refuses of a
 * region; an `op` outside 0 .. n_ops - 1; an unknown kind; a LUT3D axis below 2 or above 65; a table that is missing
 * (tables = NULL, a negative `table`) or reaches past n_tables; a matrix or table entry that is NaN or infinite.  Every
 * op is checked, used or not. */
#define TA_COLOR_MATRIX 0
#define TA_COLOR_RGB2YCBCR 1
#define TA_COLOR_YCBCR2RGB 2
#define TA_COLOR_RGB2HSV 3
#define TA_COLOR_HSV2RGB 4
#define TA_COLOR_LUT3D 5
typedef struct ta_color_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  int32_t op;            /* index into `ops`                          */
} ta_color_region;
typedef struct ta_color_op {
  int32_t kind;          /* TA_COLOR_*                                */
  int32_t size[3];       /* LUT3D: s0 (R), s1 (G), s2 (B)             */
  int32_t table;         /* MATRIX, LUT3D: the first float of the op's table in `tables` */
} ta_color_op;
int ta_frames_color(ta_ctx* ctx, ta_frames* frames, const ta_color_region* regions, int n, const ta_color_op* ops, int n_ops,
                    const float* tables, size_t n_tables);
/* HOST ONLY, no context: what ta_frames_color derives before it launches anything.  rounds[i]: the round region i runs
 * in, as ta_blur_plan's.  nodes: the int16 entries the device reads, the LUT3D ops' tables one after the other in op
 * order, four int16 per node (R, G, B entry and 0), s0 s1 s2 nodes per op; nothing for an op of another kind.  Either
 * output may be NULL.  Frame indices only group the regions here.  TA_E_INVALID: what ta_frames_color refuses without
 * looking at a frame. */
int ta_color_plan(const ta_color_region* regions, int n, const ta_color_op* ops, int n_ops, const float* tables, size_t n_tables,
                  int32_t* rounds, int16_t* nodes);

/* ---- raw YUV video frames: yuv420p, nv12, yuv444p in and out --------------------------------- */
/* Frames as `ffmpeg -f rawvideo -pix_fmt yuv420p | nv12 | yuv444p` lays them out, back to back without padding, with
 * cw = (w + 1) >> 1 and ch = (h + 1) >> 1:
 *     TA_YUV_420P   Y h x w, U ch x cw, V ch x cw         w h + 2 cw ch bytes (may be odd: a frame starts at any address)
 *     TA_YUV_NV12   Y h x w, ch rows of cw (U, V) pairs   the same size
 *     TA_YUV_444P   Y, U, V, each h x w                   3 w h bytes
 * The conversion is the standards' affine map with exact rational coefficients, rounded once, half up -- NOT swscale's
 * tables; no parity with ffmpeg's own converter is claimed.  Kr, Kb = 299/1000, 114/1000 (TA_YUV_BT601) or 2126/10000,
 * 722/10000 (TA_YUV_BT709), Kg = 1 - Kr - Kb.
 *   YUV -> RGB: y' = (Y - 16) / 219, c' = (C - 128) / 224 (TA_YUV_TV) or Y / 255, (C - 128) / 255 (TA_YUV_PC);
 *     R' = y' + 2 (1 - Kr) cr', B' = y' + 2 (1 - Kb) cb', G' = y' - (2 Kr (1 - Kr) / Kg) cr' - (2 Kb (1 - Kb) / Kg) cb';
 *     every output is clip(floor(255 X' + 1/2), 0, 255), also for inputs outside the nominal range.
 *     The chroma of pixel (x, y) of a 4:2:0 format is an 8-bit value, every index clamped to the plane:
 *     TA_YUV_NEAREST: C[y >> 1][x >> 1].  TA_YUV_BILINEAR: vertically 3 C[j] + C[j - 1] for y = 2 j and 3 C[j] + C[j + 1] for
 *     y = 2 j + 1; horizontally with TA_YUV_LEFT (MPEG-2, H.264) 2 C[x / 2] for even x and C[i] + C[i + 1], i = (x - 1) / 2,
 *     for odd x, the value (sum + 4) >> 3; with TA_YUV_CENTER (JPEG, MPEG-1) the 3 : 1 rule again, (sum + 8) >> 4.
 *   RGB -> YUV: L = Kr R + Kg G + Kb B; TV: Y = 16 + 219 L / 255, Cb = 128 + 224 (B - L) / (255 * 2 (1 - Kb)), Cr likewise
 *     with R and Kr; PC: Y = L, Cb = 128 + (B - L) / (2 (1 - Kb)); each clip(floor(v + 1/2), 0, 255).  In a 4:2:0 format
 *     Cb and Cr come from the exact mean of R, G, B over the pixels of the 2 x 2 block that lie inside the frame, rounded
 *     once; `chroma` and `siting` are checked but not used in this direction, nor by TA_YUV_444P in either.
 * ta_frames_from_yuv copies n frames from `host_yuv` (pinned or pageable) into a grow-only staging block of the context
 * that no other call uses and converts them into a NEW batch in one launch; ta_frames_to_yuv converts a batch into the
 * context's scratch block in one launch and copies the n frames to `host_yuv`.  Both run on `ctx`'s stream and return when
 * they are done.  A video reader's thread may therefore call ta_frames_from_yuv on its own context while another thread
 * runs the other frame calls on that context's batches, as it may with ta_frames_upload.
 * TA_E_INVALID, before any launch and with *out untouched: a null pointer, an unknown value of a spec field, n, h or w
 * below 1, a side above 65535, a batch of another device. */
#define TA_YUV_420P 0
#define TA_YUV_NV12 1
#define TA_YUV_444P 2
#define TA_YUV_BT601 0
#define TA_YUV_BT709 1
#define TA_YUV_TV 0
#define TA_YUV_PC 1
#define TA_YUV_NEAREST 0
#define TA_YUV_BILINEAR 1
#define TA_YUV_LEFT 0
#define TA_YUV_CENTER 1
typedef struct ta_yuv_spec {
  int32_t format, matrix, range, chroma, siting;
} ta_yuv_spec;
/* HOST ONLY: the bytes of one frame; 0 for an unknown format or a side outside 1 .. 65535 */
size_t ta_yuv_frame_bytes(int format, int h, int w);
int ta_frames_from_yuv(ta_ctx* ctx, const uint8_t* host_yuv, int n, int h, int w, const ta_yuv_spec* spec, ta_frames** out);
int ta_frames_to_yuv(ta_ctx* ctx, const ta_frames* frames, const ta_yuv_spec* spec, uint8_t* host_yuv);
/* HOST ONLY, no context: n triples through the arithmetic the kernels run.  to_yuv = 0: (Y, Cb, Cr) -> (R, G, B);
 * 1: (R, G, B) -> (Y, Cb, Cr) of a single pixel.  in3 and out3 may be the same array. */
int ta_yuv_convert_samples(const ta_yuv_spec* spec, int to_yuv, const uint8_t* in3, size_t n, uint8_t* out3);

/* ---- neighbourhood filters: convolution kernels, rank filters, unsharp mask ----------------- */
/* Filters regions of `frames` in place, Pillow's
 *     im.paste(im.crop(box).filter(F), box[, ellipse mask])
 * bit for bit.  Regions are as ta_frames_blur takes them (a half-open box inside the frame, no side longer than 16384,
 * TA_BLUR_BOX or TA_BLUR_ELLIPSE) plus `spec`, the index of the region's filter in `specs`.  The filter sees only the
 * region's own pixels: its border rules apply at the region's border, never the frame's.  Regions of one frame apply in
 * list order where they overlap (rounds of pairwise disjoint regions); regions of different frames may be interleaved.
 * A filter reads neighbours that the same call overwrites, so every round is staged: the results of a round go to the
 * region's packed image in the context's scratch and are copied into the frame under the shape afterwards (kernels,
 * ranks), or the frame is written from a blurred copy in scratch (unsharp).  The result does not depend on the launch
 * geometry.  n = 0: TA_OK.
 *
 * TA_FILTER_KERNEL   ImageFilter.Kernel((size, size), kernel, scale, offset) with size 3 or 5, and through it the ten
 *   built-in filters.  r = size / 2.  A region narrower or shorter than `size` is left as it is, and the outer r pixels
 *   of a region keep their values.  Elsewhere, per channel, in float32 with every multiply and add rounded on its own:
 *       k[i] = kernel[i] / scale  and  ss = offset + 0.5f          (on the host: the device never sees `scale`)
 *       kernel row j (j = 0 first) belongs to image row y + r - j  (the kernel is applied bottom-up)
 *       row = p[x-r] k[j][0];  row = row + p[x-r+1] k[j][1]; ...   (left to right);   ss = ss + row
 *       output: 0 if ss <= 0, 255 if ss >= 255, else (uint8)ss, truncated.
 *   has_factor != 0: ImageEnhance.Sharpness' Image.blend(filtered, original, factor): t = f + factor (o - f), the
 *   unfused float32 expression of ta_frames_saturate: truncated when 0 <= factor <= 1, clipped to 0 .. 255 first otherwise;
 *   factor 0 gives the filtered pixel, factor 1 the original.
 * TA_FILTER_RANK     ImageFilter.RankFilter(size, rank), and through it MinFilter, MedianFilter and MaxFilter: odd size
 *   1 .. 7, 0 <= rank < size^2; per channel the rank-th smallest value of the size x size window, whose coordinates are
 *   clamped to the region (edge replication): every pixel is filtered, in regions smaller than the window too.
 * TA_FILTER_UNSHARP  ImageFilter.UnsharpMask(radius, percent, threshold): b = the region's Gaussian blur exactly as
 *   ta_frames_blur computes it, d = in - b in integers; out = in when |d| <= threshold, otherwise
 *   clip(in + d percent / 100) with C integer division (towards zero; the product is taken in 64 bits).
 *
 * TA_E_INVALID, before any pixel changes: everything ta_frames_blur refuses; a `spec` outside 0 .. n_specs - 1; an unknown
 * kind; a kernel size other than 3 or 5; a kernel entry, offset or factor that is not finite; a scale that is 0 or not
 * finite; a rank size that is even or outside 1 .. 7, or a rank outside 0 .. size^2 - 1; a radius that is negative, not
 * finite or above 1024; a negative percent or threshold.  Every spec is checked, used or not. */
#define TA_FILTER_KERNEL 0
#define TA_FILTER_RANK 1
#define TA_FILTER_UNSHARP 2
typedef struct ta_filter_region {
  int32_t frame;
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  int32_t spec;          /* index into `specs`                        */
} ta_filter_region;
typedef struct ta_filter_spec {
  int32_t kind;          /* TA_FILTER_*                               */
  int32_t size;          /* KERNEL: 3 or 5; RANK: 1, 3, 5 or 7        */
  int32_t rank;          /* RANK                                      */
  int32_t has_factor;    /* KERNEL: blend the result with the original */
  float kernel[25];      /* KERNEL: size x size entries, row by row as Pillow takes them */
  float scale, offset;   /* KERNEL                                    */
  float factor;          /* KERNEL with has_factor: ImageEnhance.Sharpness' */
  float radius;          /* UNSHARP: GaussianBlur's                   */
  int32_t percent, threshold; /* UNSHARP                              */
} ta_filter_spec;
int ta_frames_filter(ta_ctx* ctx, ta_frames* frames, const ta_filter_region* regions, int n, const ta_filter_spec* specs,
                     int n_specs);
/* HOST ONLY, no context: what ta_frames_filter derives before it launches anything.  rounds[i]: the round region i runs
 * in, as ta_blur_plan's.  kernels[25 s .. 25 s + 24]: the normalised entries kernel[i] / scale of spec s, zeros behind
 * size^2 and for a spec of another kind; offsets[s]: its offset + 0.5f (0 for another kind).  Any output may be NULL.
 * Frame indices only group the regions here.  TA_E_INVALID: what ta_frames_filter refuses without looking at a frame. */
int ta_filter_plan(const ta_filter_region* regions, int n, const ta_filter_spec* specs, int n_specs, int32_t* rounds,
                   float* kernels, float* offsets);

/* ---- combining two batches: paste, blend, ImageChops ---------------------------------------- */
/* Pillow's operations of two images on regions of `dst`, in place and bit for bit.  Per region, with a = dst.crop(box) and
 * b = src.crop(the equally sized box at (src_x, src_y) of frame src_frame), the call does dst.paste(R, box) -- under
 * TA_BLUR_ELLIPSE only the ellipse's pixels change -- where R is
 *     TA_COMBINE_PASTE   a with b pasted under the region's mask: a.paste(b, (0, 0), mask), and so Image.composite
 *     TA_COMBINE_BLEND   Image.blend(a, b, alpha): the unfused float32 expression of ta_frames_saturate
 *     the others         ImageChops.lighter / darker / difference / multiply / screen / add(a, b, scale = alpha, offset) /
 *                        subtract(likewise) / add_modulo / subtract_modulo / soft_light / hard_light / overlay
 * Per sample (libImaging/Paste.c, Chops.c), in integers unless said otherwise:
 *     PASTE under mask m   t = a (255 - m) + b m + 128; ((t >> 8) + t) >> 8      (one division, not two)
 *     MULTIPLY  a b / 255        SCREEN  255 - (255 - a) (255 - b) / 255          DIFFERENCE  |a - b|
 *     ADD       float32 (a + b) / scale + offset: a correctly rounded division, then an addition; 0 at or below 0, 255 at
 *               or above 255, truncated between.  SUBTRACT: (a - b) likewise.  (Where the quotient leaves int's range Pillow
 *               is undefined; here it saturates.)
 *     ADD_MODULO (a + b) mod 256   SUBTRACT_MODULO (a - b) mod 256
 *     SOFT_LIGHT  (255 - a) (a b) / 65536 + a (255 - (255 - a) (255 - b) / 255) / 255
 *     HARD_LIGHT  b < 128 ? a b / 127 : 255 - (255 - b) (255 - a) / 127;  OVERLAY: the same with a < 128 as the test
 * The mask of a PASTE region (mode 'L'; the other ops take TA_MASK_NONE only):
 *     TA_MASK_NONE      none: b replaces a
 *     TA_MASK_CONSTANT  Image.new('L', size, mask_value), mask_value 0 .. 255
 *     TA_MASK_BITMAP    the packed w x h bitmap at byte offset mask_value of the HOST buffer `masks`; any number of
 *                       regions may name one bitmap; the buffer travels in the staging copy of the regions
 *     TA_MASK_FRAMES    band mask_band (0 .. 2) of the equally sized box at (mask_x, mask_y) of frame mask_frame of
 *                       `mask_frames`: getchannel(band)
 * The destination box is as ta_frames_point takes it (half-open, inside the frame, no side longer than 16384); `src` and
 * `mask_frames` may have any n, h, w.  Regions of one destination frame apply in list order where they overlap (rounds of
 * pairwise disjoint regions, one launch per round).  `src` and `mask_frames` may be `dst` itself only if no frame that any
 * region writes is read by any region as its source or mask frame.  All batches must live on `ctx`'s device; the call
 * runs on `ctx`'s stream and returns when it is done.  n = 0: TA_OK.
 * TA_E_INVALID, before any launch and any changed pixel, naming the region: what ta_frames_point refuses of a box; a
 * source or mask box that is not inside its frame; a frame index out of range; an unknown op or mask kind; a mask on an op
 * other than PASTE; alpha that is NaN or infinite, or 0 as the scale of ADD / SUBTRACT; a mask_value outside 0 .. 255
 * (CONSTANT); a band outside 0 .. 2; a bitmap that reaches past mask_bytes; `masks` or `mask_frames` NULL where a region
 * needs them; a frame both written and read as said above. */
#define TA_COMBINE_PASTE 0
#define TA_COMBINE_BLEND 1
#define TA_COMBINE_LIGHTER 2
#define TA_COMBINE_DARKER 3
#define TA_COMBINE_DIFFERENCE 4
#define TA_COMBINE_MULTIPLY 5
#define TA_COMBINE_SCREEN 6
#define TA_COMBINE_ADD 7
#define TA_COMBINE_SUBTRACT 8
#define TA_COMBINE_ADD_MODULO 9
#define TA_COMBINE_SUBTRACT_MODULO 10
#define TA_COMBINE_SOFT_LIGHT 11
#define TA_COMBINE_HARD_LIGHT 12
#define TA_COMBINE_OVERLAY 13
#define TA_MASK_NONE 0
#define TA_MASK_CONSTANT 1
#define TA_MASK_BITMAP 2
#define TA_MASK_FRAMES 3
typedef struct ta_combine_region {
  int32_t frame;         /* image index in `dst`                      */
  int32_t x0, y0, x1, y1;
  int32_t shape;         /* TA_BLUR_*                                 */
  int32_t src_frame, src_x, src_y; /* the source box's frame and top-left corner in `src` */
  int32_t op;            /* TA_COMBINE_*                              */
  float alpha;           /* BLEND: Image.blend's alpha; ADD, SUBTRACT: scale */
  int32_t offset;        /* ADD, SUBTRACT                             */
  int32_t mask_kind;     /* TA_MASK_* (PASTE)                         */
  int32_t mask_value;    /* CONSTANT: 0 .. 255; BITMAP: byte offset in `masks` */
  int32_t mask_frame, mask_x, mask_y, mask_band; /* FRAMES            */
} ta_combine_region;
int ta_frames_combine(ta_ctx* ctx, ta_frames* dst, const ta_frames* src, const ta_frames* mask_frames,
                      const ta_combine_region* regions, int n, const uint8_t* masks, size_t mask_bytes);

/* ---- tiles: cut many tiles of many frames in one launch (the front of tiled detection) ---------------------------------- */
/* *out = a NEW resident batch (n, th, tw, 3): tile i is src[frame, y : y + th, x : x + tw], byte for byte.  One launch for
 * all tiles; wide loads and stores whatever the byte alignment of the two sides; 64-bit offsets throughout.
 * TA_E_INVALID: a tile that leaves its frame or a frame out of range (the message names the tile), th or tw <= 0.
 * n == 0: TA_OK and *out = NULL. */
typedef struct ta_tile {
  int32_t frame, y, x;
} ta_tile;
int ta_frames_tiles(ta_ctx* ctx, const ta_frames* src, const ta_tile* tiles, int n, int th, int tw, ta_frames** out);

/* ---- JPEG decode (terran/io/image.py: open_image = Pillow's Image.open(f).convert('RGB')) ------------------------------ */
/* Baseline and extended-sequential Huffman JPEGs, 8-bit, 1 or 3 components in one interleaved scan, every component's
 * sampling ratio 1 or 2 in each direction (4:4:4, 4:2:2, 4:2:0, 4:4:0, grayscale), any width and height, restart
 * intervals, the standard Huffman tables where a file defines none (Motion-JPEG frames).  The markers and the Huffman
 * stream are decoded on the host; dequantisation, the 8x8 inverse DCT
 * (libjpeg's JDCT_ISLOW with its range-limit table), fancy upsampling and the YCbCr -> RGB tables run on the device.
 * Pixels equal libjpeg-turbo's default decode bit for bit.  Anything else is a FALLBACK image, decided on the host from
 * its markers before any GPU work: its path says why, and the caller decodes it with Pillow. */
#define TA_JPEG_DEVICE 0                 /* decoded by this library                                                  */
#define TA_JPEG_FALLBACK_PROCESS 1       /* progressive, lossless or hierarchical                                    */
#define TA_JPEG_FALLBACK_ARITHMETIC 2    /* arithmetic-coded                                                         */
#define TA_JPEG_FALLBACK_PRECISION 3     /* samples of other than 8 bits                                             */
#define TA_JPEG_FALLBACK_COMPONENTS 4    /* neither 1 nor 3 components (CMYK, YCCK)                                  */
#define TA_JPEG_FALLBACK_COLOR 5         /* 3 components stored as RGB (Adobe transform 0, or component ids R, G, B) */
#define TA_JPEG_FALLBACK_SCANS 6         /* the components are not all in one interleaved scan                       */
#define TA_JPEG_FALLBACK_SAMPLING 7      /* a sampling ratio other than 1 or 2                                       */
#define TA_JPEG_INVALID (-1)             /* ta_jpeg_decode failed with TA_E_INVALID: this image is malformed or truncated  */
typedef struct ta_jpeg_header {
  int32_t width, height, components;
  int32_t path;                        /* TA_JPEG_DEVICE or a TA_JPEG_FALLBACK_* reason                              */
  int32_t h_samp[3], v_samp[3];        /* sampling factors of the components                                         */
  int32_t quant_index[3];              /* quantisation table of each component (row of `quant`)                      */
  int32_t blocks_w[3], blocks_h[3];    /* coefficient block grid of each component (whole MCUs)                      */
  int32_t restart_interval;            /* MCUs, 0 = none                                                             */
  int32_t reserved[2];
  int64_t block_offset[3];             /* first block of each component in the coefficient array                     */
  int64_t blocks_total;
  uint16_t quant[4][64];               /* quantisation tables, natural (row-major) order                             */
} ta_jpeg_header;
/* HOST ONLY -- the one entry point that needs no context and no device (the exception to "no CPU fallback"; it decodes
 * no pixels): parses one JPEG and entropy-decodes it into header->blocks_total blocks of 64 int16 quantised
 * coefficients in natural order, component after component, each component's block grid in raster order.  coefs may be
 * NULL (header only); capacity_blocks < blocks_total gives TA_E_CAPACITY with the header filled in.  A fallback image
 * returns TA_OK with its path and whatever header facts were read, and no coefficients.  Malformed or truncated data:
 * TA_E_INVALID with the reason in err (may be NULL). */
int ta_jpeg_coefficients(const uint8_t* data, size_t size, ta_jpeg_header* header, int16_t* coefs, int64_t capacity_blocks,
                         char* err, int err_capacity);
/* Decodes n JPEGs (data[i], sizes[i] bytes) into resident frames.  All images of one size -- an MJPEG or burst batch --
 * give ONE (n,H,W,3) batch in out[0] (*required = 1); otherwise out[i] is a (1,H_i,W_i,3) batch per image
 * (*required = n).  capacity < *required: TA_E_CAPACITY before any work.  paths[i] (n entries) gets TA_JPEG_DEVICE or
 * the image's TA_JPEG_FALLBACK_* reason; a fallback image's pixels are left zero for the caller to fill
 * (ta_frames_paste).  The Huffman streams are decoded on `threads` host threads (0: min(n, 16); at most 16) straight
 * into the context's pinned staging; both kernels run once for the whole call.  Returns when the frames are written.
 * TA_E_INVALID: not a JPEG, malformed or truncated data; no frames are returned then, ta_last_error names the first
 * such image and paths[i] is TA_JPEG_INVALID for every one of them (the rest as above), so a caller can hand those to a
 * more lenient decoder and decode the others again. */
int ta_jpeg_decode(ta_ctx* ctx, const uint8_t* const* data, const size_t* sizes, int n, int threads, int capacity,
                   ta_frames** out, int32_t* paths, int32_t* required);
/* Figures of the last ta_jpeg_decode on this context.  ms[4]: host parse + Huffman wall time, host-to-device copy, then
 * the dequantise + IDCT kernel and the upsample + colour kernel (HIP events; 0 unless ta_profile_enable is on).
 * counts[4]: images decoded on the device, coefficient blocks, bytes copied to the device, fallback images. */
int ta_jpeg_last_stats(const ta_ctx* ctx, double* ms, int64_t* counts);

/* ---- JPEG encode (Image.fromarray(frame).save(f, 'JPEG', quality=q, subsampling=s) with Pillow's other defaults) ---- */
/* Baseline JFIF files byte for byte as Pillow / libjpeg-turbo writes them: Annex K quantisation tables scaled by
 * `quality` (1..100, force_baseline), islow forward DCT, standard Huffman tables, no restart markers, no smoothing.
 * subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (Pillow's default).  Optimized Huffman tables: ta_jpeg_encode_opt.
 * Progressive, custom quantisation tables, restart intervals and metadata segments are not offered. */
/* HOST ONLY, no context: the header Pillow writes for an h x w RGB image (SOI .. SOS).  *size gets its length; capacity
 * < *size gives TA_E_CAPACITY.  Bad arguments: TA_E_INVALID. */
int ta_jpeg_encode_header(int h, int w, int quality, int subsampling, uint8_t* out, size_t capacity, size_t* size);
/* frames -> n complete JPEG files, back to back in context-owned pinned memory (*out) that stays valid until the next
 * ta_jpeg_encode on ctx; sizes[i] bytes each (n entries).  Runs on ctx's stream, after whatever was queued there (a
 * ta_frames_draw, say); every stage runs on the device and only the files are copied back.  Returns when they are
 * there.  Bad arguments: TA_E_INVALID before any launch. */
int ta_jpeg_encode(ta_ctx* ctx, const ta_frames* frames, int quality, int subsampling, const uint8_t** out,
                   size_t* sizes);
/* Figures of the last ta_jpeg_encode on this context.  ms[8]: HIP-event times (0 unless ta_profile_enable is on) of the
 * staging copy, E1 (pixels -> coefficients), E2 (bit lengths + scan), E3 (emit), E4a (0xFF count + scan), E4b (stuff +
 * pack), the device-to-host copy of the files; then the host wall time of the whole call.  counts[4]: images, blocks,
 * bytes copied to the host, entropy-coded bytes before stuffing. */
int ta_jpeg_encode_last_stats(const ta_ctx* ctx, double* ms, int64_t* counts);
/* ta_jpeg_encode with Pillow's `optimize` option.  optimize = 0 is ta_jpeg_encode itself (the standard Huffman tables,
 * the same launches, the same bytes).  optimize = 1 writes what save(..., optimize=True) writes: every image is coded
 * with tables built from its own symbol statistics (libjpeg's jpeg_gen_optimal_table; Cb and Cr share table 1), which
 * its header carries in four DHT segments.  One more device pass counts the symbols and the histograms (2 176 bytes an
 * image) visit the host, which builds the tables.  An image of 10^9 / 64 blocks or more is refused (TA_E_INVALID,
 * before any launch): libjpeg's frequency arithmetic assumes counts below 10^9. */
int ta_jpeg_encode_opt(ta_ctx* ctx, const ta_frames* frames, int quality, int subsampling, int optimize,
                       const uint8_t** out, size_t* sizes);
/* HOST ONLY, no context: libjpeg's optimal Huffman table for the symbol frequencies freq[0..255] (each 0 .. 10^9 - 1,
 * at least one nonzero; freq[256], the reserved pseudo-symbol that keeps the all-ones code free, is taken as 1 whatever
 * it holds).  bits[1..16] get the number of codes of each length (bits[0] = 0), vals[0 .. *nvals) the symbols in code
 * order.  Bad arguments: TA_E_INVALID. */
int ta_jpeg_optimal_table(const int64_t* freq, uint8_t* bits, uint8_t* vals, int* nvals);
/* More figures of the last ta_jpeg_encode_opt on this context (zeros after an optimize = 0 call).  ms[2]: HIP-event
 * time of the statistics pass (0 unless ta_profile_enable is on; its histogram copy and synchronisation are not in it),
 * host wall time of building the tables and headers. */
int ta_jpeg_encode_last_opt_stats(const ta_ctx* ctx, double* ms);

/* ---- models ---------------------------------------------------------------------------- */
/* `blob` is the packed model produced by terran_amd/pack.py from a Terran state_dict
 * (replaces load_model(): retinaface/wrapper.py:16-22, arcface/wrapper.py:13-19,
 * openpose/wrapper.py:27-36).  The blob is copied; the caller may free it. */
int ta_model_load(ta_ctx* ctx, int kind, const void* blob, size_t bytes, ta_model** out);
/* HOST ONLY, no context: every check of a blob that depends on the program alone -- header, tables, weight offsets, op
 * records, tensor formats, data flow, lanes.  ta_model_load runs it first, so a program it accepts can only be refused
 * later for the shape of an input or by the device.  TA_OK, or TA_E_INVALID with the defect in `msg` (may be NULL). */
int ta_program_check(int kind, const void* blob, size_t bytes, char* msg, size_t msg_capacity);
void ta_model_free(ta_model* m);
int ta_model_kind(const ta_model* m);

/* Debug taps for parity tests: run only the network on `frames` (RetinaFace / OpenPose) or on
 * uint8 BGR CHW crops (ArcFace), then read any tensor of the op program back as float32 NCHW.
 * `tensor` is a tensor id of the packed program; `ch_off/ch` select a channel slice. */
int ta_model_forward_frames(ta_model* m, const ta_frames* frames);
int ta_model_forward_crops(ta_model* m, const uint8_t* crops_nchw_bgr, int n);
int ta_model_tensor_shape(ta_model* m, int tensor, int* n, int* c, int* h, int* w);
int ta_model_read_tensor(ta_model* m, int tensor, int ch_off, int ch, float* dst_nchw);

/* f16x3 / f16 programs store every CHANNEL of every tensor times a power of two chosen at pack time (terran_amd/pack.py:
 * tensor_scales); ta_model_read_tensor divides it out.  ta_model_tensor_unscale copies the per-channel factors 2^-a[c]
 * (ones where nothing is scaled; capacity >= the tensor's channels).  ta_model_debug_amax (tools / tests: does the packer's
 * expectation hold?): enable != 0 starts (or restarts, zeroed) the collection of the largest |x| every conv / dw+pw op STORES
 * (in stored, i.e. scaled, units: the figure that must stay below 65504); with out != NULL the maxima collected so far are
 * copied out first: out[2 i] = op i's output, out[2 i + 1] = the depthwise intermediate of a dw+pw op; capacity >= 2 x the
 * number of ops (TA_E_CAPACITY otherwise).  enable == 2 only reads (the collection goes on), enable == 0 ends it. */
int ta_model_tensor_unscale(const ta_model* m, int tensor, float* out, int capacity);
int ta_model_debug_amax(ta_model* m, int enable, float* out, int capacity);
/* tools (tools/graph_probe.py): replays the op program of the last forward `reps` times as stream launches and as a hipGraph
 * captured from them.  out_ms[5]: GPU ms per replay (streams, graph), host enqueue ms per replay (streams, graph), capture +
 * instantiate ms.  Measurement aid for DESIGN.md section 4 ("why the programs are not hipGraphs"); no product path calls it. */
int ta_model_graph_probe(ta_model* m, int reps, double* out_ms);

/* ---- RetinaFace.call (retinaface/wrapper.py:133-238) ------------------------------------ */
/* frames: (N,H,W,3) uint8 RGB at network resolution.  Per image: threshold (>=), sort by
 * descending score (ties: ascending anchor index), greedy NMS (IoU > nms_thr suppressed).
 * Results are concatenated over images in order; counts[i] = detections of image i.
 * boxes (x1,y1,x2,y2), landmarks 5x(x,y), network-input pixels, float32. */
int ta_retinaface_run(ta_model* m, const ta_frames* frames, float score_thr, float nms_thr,
                      int capacity, int32_t* counts, float* boxes, float* landmarks, float* scores,
                      int32_t* required);
/* Post-processing only, on host head tensors in the reference layout (nine NCHW float32 arrays,
 * order stride 32,16,8 x cls_prob(4ch), bbox(8ch), landmark(20ch); model.py:304-316). */
int ta_retinaface_postprocess(ta_ctx* ctx, const float* const heads[9], int n, int h, int w,
                              float score_thr, float nms_thr, int capacity, int32_t* counts,
                              float* boxes, float* landmarks, float* scores, int32_t* required);

/* ---- tiled detection: detections of tiles -> detections of their frames ----------------------------------------------- */
/* Candidates (host arrays: boxes (C,4), landmarks (C,5,2), scores (C,), float32, finite) come in GROUPS: the detections
 * of one tile, or of one whole-frame pass, of one output frame.  Groups are sorted by frame and share no row; a row in
 * no group is ignored.  Per candidate, in float32:
 *   map    every coordinate v of its box and landmarks becomes v / zoom + o (one correctly rounded division, one
 *          addition; o = ox for x, oy for y); scores are unchanged
 *   edge   (edge > 0) it is dropped if its mapped box comes within `edge` pixels of an INTERIOR side of its group's
 *          rectangle: bx1 < x0 + edge (left, bit 0), by1 < y0 + edge (top, bit 1), bx2 > x1 - edge (right, bit 2),
 *          by2 > y1 - edge (bottom, bit 3): a face cut by the tile, which the overlapping neighbour sees whole
 * Per frame the survivors are ordered by descending score (-0 = +0), equal scores by ascending row, and go through
 * greedy NMS: ovr = inter / (area_a + area_b - inter) with area = (x2 - x1) * (y2 - y1), ta_retinaface_run's expression
 * and operation order (metric 0), or inter / fminf(area_a, area_b), intersection over the smaller box (metric 1);
 * suppressed iff ovr > nms_thr.  Outputs: the kept candidates per frame in that order, frames concatenated, counts[f]
 * of frame f; out_source = each one's candidate row.  Capacity protocol of ta_retinaface_run: a short `capacity` gives
 * TA_E_CAPACITY with *required and counts set.  Everything but the checks runs on the device; the suppression bit matrix
 * lives in the context's scratch block (frames are processed in batches whose matrices fit 256 MiB).
 * TA_E_OVERFLOW: more than 16384 candidates in the groups of one frame.  TA_E_INVALID: unsorted or overlapping groups, rows
 * outside the arrays, zoom <= 0, an unknown metric, edge < 0. */
typedef struct ta_merge_group {
  int32_t frame;          /* which output frame this group of candidates belongs to; groups come sorted by frame    */
  int32_t first, count;   /* its candidates: rows first .. first+count-1 of the candidate arrays                    */
  float ox, oy, zoom;     /* frame = tile / zoom + origin                                                           */
  float x0, y0, x1, y1;   /* the group's rectangle in frame coordinates                                             */
  int32_t interior;       /* bit 0 left, 1 top, 2 right, 3 bottom: that side of the rectangle lies inside the frame */
} ta_merge_group;
int ta_detections_merge(ta_ctx* ctx, const ta_merge_group* groups, int n_groups, int n_frames, const float* boxes,
                        const float* landmarks, const float* scores, int n_candidates, float nms_thr, int metric,
                        float edge, int capacity, int32_t* counts, float* out_boxes, float* out_landmarks,
                        float* out_scores, int32_t* out_source, int32_t* required);

/* ---- ArcFace.call (arcface/wrapper.py:109-184) ------------------------------------------ */
/* Embed n pre-cropped faces, uint8 (n,3,112,112) BGR.  normalize != 0 applies the row-wise L2
 * normalisation of wrapper.py:176.  out: (n,512) float32. */
int ta_arcface_embed_crops(ta_model* m, const uint8_t* crops_nchw_bgr, int n, int normalize, float* out);
/* Align + embed on the device: face k is warped from frames[frame_index[k]] with the inverse
 * similarity inv_affine[k] (6 doubles, PIL Image.transform(AFFINE) convention, wrapper.py:61-69),
 * bilinear, fill 0, to 112x112 BGR.  crops_out (optional, may be NULL): (n,3,112,112) uint8. */
int ta_arcface_embed_faces(ta_model* m, const ta_frames* frames, const int32_t* frame_index,
                           const double* inv_affine, int n, int normalize, float* out,
                           uint8_t* crops_out);
/* The same for faces cut from SEVERAL resident frame batches in one launch (a video loop's embedder sees the faces of every
 * batch in flight: the network fills the chip at ~256 crops, one 32-frame batch brings ~64): face k comes from
 * frames[source_index[k]] (source_index NULL: all from frames[0]), image frame_index[k] of that batch.  All batches must live
 * on the model's device (any context).  A face's embedding does not depend on the launch it rides in. */
int ta_arcface_embed_faces_multi(ta_model* m, const ta_frames* const* frames, int n_sources, const int32_t* source_index,
                                 const int32_t* frame_index, const double* inv_affine, int n, int normalize,
                                 float* out, uint8_t* crops_out);
/* Cosine distance matrix 1 - a.b/(|a||b|) (examples/match.py:38): a (na,dim), b (nb,dim) -> (na,nb). */
int ta_cosine_distance(ta_ctx* ctx, const float* a, int na, const float* b, int nb, int dim, float* out);

/* ---- gallery: who is this face? (examples/match.py:30-41 asked of a watch-list) --------- */
/* A grow-only set of `dim`-float embeddings (dim 1..1024) resident on the device, stored L2-normalised, each with a
 * caller-chosen int32 id >= 0 (several rows may share an id).  Rows keep their index for the gallery's life: removing
 * marks a row, it does not move the others.  At most 2^31-1 rows (TA_E_INVALID beyond).  `reserve_rows` allocates ahead;
 * growth doubles the buffer with a device copy.  A gallery grown in steps answers bit for bit like one reserved up front. */
typedef struct ta_gallery ta_gallery;
int ta_gallery_create(ta_ctx* ctx, int dim, int64_t reserve_rows, ta_gallery** out);
void ta_gallery_free(ta_gallery* g);
/* Appends n rows (n, dim) with their ids (>= 0).  normalize != 0: each row is divided by its float32 L2 norm as
 * ta_arcface_embed_* does (a zero row stays zero); 0: the rows are stored as given (they should have unit length). */
int ta_gallery_add(ta_gallery* g, const float* rows, const int32_t* ids, int64_t n, int normalize);
/* Every live row that carries one of the n ids is marked removed (its stored id becomes -1) and never found again;
 * *removed = how many rows that were. */
int ta_gallery_remove(ta_gallery* g, const int32_t* ids, int n, int64_t* removed);
/* Forgets every row (the memory is kept); row indices start at 0 again. */
int ta_gallery_clear(ta_gallery* g);
/* *rows = rows ever added since the last clear (removed ones included: the range of row indices), *live = those not removed. */
int ta_gallery_size(const ta_gallery* g, int64_t* rows, int64_t* live);
/* The stored (normalised) rows (rows, dim) and ids (rows,), -1 for removed rows: ta_gallery_add(..., normalize = 0) of them
 * into a fresh gallery rebuilds this one bit for bit. */
int ta_gallery_download(const ta_gallery* g, float* rows_out, int32_t* ids_out);
/* The k (1..16) nearest live rows of each of nq queries (nq, dim) by cosine distance 1.0f - dot(query, row) in float32
 * (normalize != 0: the queries are L2-normalised first), ordered by (distance, row index) ascending: ties go to the
 * lower row.  out_row / out_id / out_dist are (nq, k); with fewer than k live rows the tail is (-1, -1, +inf).
 * nq == 0 and an empty gallery succeed.  The result does not depend on how the gallery was grown.
 * Rows and queries must be finite; they are not checked.  A NaN or infinite component gives NaN distances, which take the
 * place their bit pattern gives them (sign bit clear: behind +inf; set: in front of every number) and mean nothing. */
int ta_gallery_search(ta_gallery* g, const float* queries, int nq, int k, int normalize, int32_t* out_row, int32_t* out_id,
                      float* out_dist);
/* Which rows are the same person?  DBSCAN over the stored rows, indices 0 .. rows-1 (removed ones included in the index
 * space).  i ~ j iff both rows are live and 1.0f - dot(row_i, row_j) < threshold in float32, the distance of
 * ta_gallery_search; every unordered pair is decided once, so ~ is symmetric; a row is its own neighbour like any other
 * (a zero row or one with a NaN component is nobody's).  degree_out[i] = number of j with i ~ j (0 for removed rows); a row
 * is core iff its degree >= min_samples (>= 1).  Clusters are the connected components of ~ among core rows, numbered
 * 0, 1, ... by ascending smallest core row; a live non-core row with a core neighbour joins the lowest-numbered cluster
 * among its core neighbours'; every other row gets -1.  That is sklearn.cluster.DBSCAN(metric='precomputed') on the same
 * adjacency, numbering included; min_samples = 1 is single linkage at the threshold.  labels_out / degree_out are (rows,);
 * degree_out, n_clusters and rounds (the label propagation rounds the call ran) may be NULL.  The labels do not depend
 * on how the gallery was grown or on anything the device schedules.  An empty gallery succeeds with *n_clusters = 0.
 * TA_E_INVALID: min_samples < 1, a threshold that is not finite, labels_out NULL with rows > 0, more than 2^18 rows (the
 * call allocates rows^2 / 8 bytes for its bit matrix, 8 GiB at the limit, and frees them before it returns).  TA_E_DEVICE:
 * that allocation failed; the gallery is untouched. */
int ta_gallery_cluster(ta_gallery* g, float threshold, int min_samples, int32_t* labels_out, int32_t* degree_out,
                       int32_t* n_clusters, int32_t* rounds);

/* ---- OpenPose.call (openpose/wrapper.py:182-485) ---------------------------------------- */
/* frames: uint8 RGB ALREADY at network resolution (the wrapper's resize is ta_frames_resize);
 * scale = short_side / min(H_orig, W_orig) maps keypoints back ((coord/scale) truncated).
 * keypoints: (M,18,3) int32 (x, y, present); scores: (M,) float64; counts[i] humans of image i.
 * No caps, like the reference (wrapper.py:235-262,335-366): the grouping kernels' fast path keeps 1024 peaks per part,
 * 8192 candidate pairs per limb and 192 people under assembly per image in LDS (~50x what a real frame produces); an
 * image that outgrows them -- a saturated heat-map plateau does -- is recomputed alone with lists in global memory sized
 * from its own counts, and network-resolution maps too large for the LDS staging (beyond ~90 x 160 cells) take the same
 * global-memory kernels for the whole batch.  Only > 65535 peaks of one part in one image fail (TA_E_OVERFLOW). */
int ta_openpose_run(ta_model* m, const ta_frames* frames, double scale, int capacity,
                    int32_t* counts, int32_t* keypoints, double* scores, int32_t* required);
/* Grouping only (x8 bicubic, peaks, PAF scoring, greedy matching, assembly) on host maps at
 * network-output resolution: pafs (N,38,h,w), heatmaps (N,19,h,w) float32 NCHW. */
int ta_openpose_group(ta_ctx* ctx, const float* pafs, const float* heatmaps, int n, int h, int w,
                      double scale, int capacity, int32_t* counts, int32_t* keypoints,
                      double* scores, int32_t* required);
/* ---- tiled pose estimation: poses of tiles -> poses of their frames ---------------------------------------------------- */
/* Candidates (host arrays: keypoints (C,18,3) int32 (x, y, present), what ta_openpose_run answers; scores (C,) float64,
 * finite) come in GROUPS: the poses of one tile, or of one whole-frame pass, of one output frame.  Groups are sorted by
 * frame and share no row; a row in no group is ignored.  Everything below is integer arithmetic, or one IEEE double
 * multiply followed by a compare: the answer is defined bit for bit.  Per candidate:
 *   present  joint j is present iff kp[j][2] != 0; a candidate with no present joint is dropped
 *   map      a present joint becomes (x + ox, y + oy, kp[j][2]), an absent one (0, 0, 0); there is no zoom here, because
 *            ta_openpose_run already divided by its scale; scores are unchanged
 *   extent   bx0, bx1, by0, by1 = min and max over the mapped present joints; s2 = (bx1 - bx0 + 1) * (by1 - by0 + 1) as
 *            int64; np = the number of present joints
 *   edge     (edge > 0) it is dropped if bx0 < x0 + edge (left, bit 0), by0 < y0 + edge (top, bit 1), bx1 >= x1 - edge
 *            (right, bit 2) or by1 >= y1 - edge (bottom, bit 3) on a side whose bit is set in `interior`: a body the tile
 *            cut, which the overlapping neighbour sees more of
 * Per frame the survivors are ordered by descending np, then descending score (-0 = +0), then ascending row: the most
 * complete skeleton wins.  Two candidates a, b of one frame are DUPLICATES iff
 *   - they come from different groups (the network's own assembly decided that two poses of one tile are two people:
 *     a same-group pair is never compared), and
 *   - shared = popcount(present_a & present_b) >= min_shared, and
 *   - (double)matched >= agree * (double)shared, where matched counts the shared joints with
 *     (double)(dx * dx + dy * dy) <= r2 * S, dx and dy in int64, r2 = radius * radius computed once in double,
 *     S = (double)max(s2_a, s2_b): one double multiply on each side of each compare, in this order.
 * The relation is symmetric.  Greedy suppression over the order: a candidate is kept iff no earlier KEPT candidate is its
 * duplicate.  Outputs: the kept candidates per frame in that order, frames concatenated; counts[f] of frame f, the mapped
 * keypoints, the unchanged scores, out_source = each one's candidate row.  Capacity protocol of ta_detections_merge: a
 * short `capacity` gives TA_E_CAPACITY with *required and counts set and nothing else written.  Everything but the checks
 * runs on the device; the suppression bit matrix lives in the context's scratch block (frames are processed in batches
 * whose matrices fit 256 MiB, $TA_PM_MATRIX_BYTES overrides).
 * TA_E_OVERFLOW: more than 16384 candidates in the groups of one frame (checked before any launch).  TA_E_INVALID:
 * unsorted or overlapping groups, rows outside the arrays, a frame out of range, radius not finite or < 0, agree outside
 * (0, 1], min_shared outside 1 .. 18, edge < 0, any |x|, |y| of a row in a group (present or not) or |ox|, |oy| at or
 * above 2^22 -- below that bound s2 < 2^48 and dx * dx + dy * dy < 2^49 are exact in int64 and in double alike. */
typedef struct ta_pose_group {
  int32_t frame;          /* which output frame this group of candidates belongs to; groups come sorted by frame    */
  int32_t first, count;   /* its candidates: rows first .. first+count-1 of the candidate arrays                    */
  int32_t ox, oy;         /* frame = tile + origin                                                                  */
  int32_t x0, y0, x1, y1; /* the group's rectangle in frame coordinates                                             */
  int32_t interior;       /* bit 0 left, 1 top, 2 right, 3 bottom: that side of the rectangle lies inside the frame */
} ta_pose_group;
int ta_poses_merge(ta_ctx* ctx, const ta_pose_group* groups, int n_groups, int n_frames, const int32_t* keypoints,
                   const double* scores, int n_candidates, double radius, double agree, int min_shared, int edge,
                   int capacity, int32_t* counts, int32_t* out_keypoints, double* out_scores, int32_t* out_source,
                   int32_t* required);

/* ---- whose face is this body's?  faces of frames <-> skeletons of frames ------------------------------------------------ */
/* Host arrays, frames concatenated: face_counts / pose_counts (n_frames,) int32; boxes (n_faces, 4) int32 (x0, y0, x1, y1),
 * the detector's bbox; keypoints (n_poses, 18, 3) int32 (x, y, present), what ta_openpose_run and ta_poses_merge answer.
 * All arithmetic is integer, so the answer is defined bit for bit.  Per frame, for its face f and pose p (indices local to
 * the frame):
 *   head      joints 0, 14, 15, 16, 17 (nose, both eyes, both ears); a joint is present iff its third value is != 0, and
 *             the x, y of an absent joint are ignored whatever they hold; n = the number of present head joints; a pose with
 *             n == 0 links to nothing
 *   box       w = x1 - x0, h = y1 - y0; a box with w < 0 or h < 0 contains nothing (its face links to nothing; no error);
 *             mx = (w * margin_permille) / 1000, my = (h * margin_permille) / 1000 in int64, truncating (both >= 0); a
 *             joint is inside iff x0 - mx <= x <= x1 + mx and y0 - my <= y <= y1 + my, inclusive on all four sides
 *   pair      inside = the present head joints inside; the pair QUALIFIES iff inside >= min_inside and 2 * inside >= n
 *             (a neighbour whose one ear pokes into the box stays out)
 *   cost      cx = x0 + x1, cy = y0 + y1 (doubled coordinates); S = the sum over ALL present head joints of
 *             (2x - cx)^2 + (2y - cy)^2 in int64; cost = S * (60 / n), 60 / n being 60, 30, 20, 15 or 12: 60 x the mean
 *             squared distance to the box centre as one int64
 *   range     every |x|, |y| and box coordinate is below 2^22, so |2x - cx| < 2^24, a joint adds less than 2^49,
 *             S < n * 2^49 and cost < 60 * 2^49 < 2^55: exact in int64, which the device keeps throughout (costs pass
 *             2^53; no float appears anywhere)
 *   match     the qualifying pairs of a frame are ordered by (cost, f, p) ascending, a strict total order, and walked in that
 *             order: a pair is linked iff neither its face nor its pose is linked yet
 * Outputs: pose_of_face (n_faces,) the frame-local pose index or -1; face_of_pose (n_poses,) the frame-local face index or
 * -1; links (n_frames,) the pairs linked per frame, may be NULL; rounds, may be NULL: the device commits every mutually
 * best pair (the cheapest free pair of its face by (cost, p) and of its pose by (cost, f)) round after round until a round
 * commits nothing, which gives the walk's answer; a frame runs its committing rounds and that silent one, *rounds is the
 * largest number over the frames (1 when nothing links, 0 for n_frames == 0).  The answer depends on nothing the device
 * schedules and on nothing but the frame's own faces and poses.  The matrix of qualifying pairs, one bit a pair and once
 * per side, lives in the context's scratch block (frames are processed in batches whose matrices fit 256 MiB,
 * $TA_FL_MATRIX_BYTES overrides); nothing else grows with n_faces * n_poses.
 * Checked on the host before any launch, outputs untouched on failure.  TA_E_OVERFLOW: more than 16384 faces or more than
 * 16384 poses in one frame, the per-frame limit of the two merge calls that feed this one.  TA_E_INVALID: a negative count;
 * counts that do not sum to n_faces / n_poses; a NULL array that has rows; margin_permille outside 0 .. 4000; min_inside
 * outside 1 .. 5; any box coordinate, or any x, y of any of the 18 joints of a row (present or not), at or above 2^22 in
 * size.  n_frames == 0 and frames with no faces or no poses succeed. */
int ta_faces_poses_link(ta_ctx* ctx, int n_frames, const int32_t* face_counts, const int32_t* boxes, int n_faces,
                        const int32_t* pose_counts, const int32_t* keypoints, int n_poses, int margin_permille,
                        int min_inside, int32_t* pose_of_face, int32_t* face_of_pose, int32_t* links, int32_t* rounds);

/* ---- which skeleton of an earlier frame is this one?  skeletons followed over the frames of a sequence -------------------- */
/* Host arrays, sequences and frames concatenated: frames_per_sequence (n_sequences,) int32 -- independent streams (cameras,
 * shots of a clip), nothing links across a sequence boundary; history_frames (n_sequences,) int32, 0 .. the sequence's frame
 * count: the first h frames of a sequence are history of earlier calls, their skeletons can be predecessors but look for none;
 * pose_counts (n_frames,) int32; keypoints (n_poses, 18, 3) int32 (x, y, present) as above: a joint is present iff its third
 * value is != 0, the x, y of an absent joint are ignored; closed (n_poses,) uint8, may be NULL: nonzero = this skeleton
 * already has a successor (from an earlier call) and cannot be a predecessor.  All arithmetic is integer, so the answer is
 * defined bit for bit.
 *   pairs     skeleton a of frame ta and skeleton b of frame tb, both frames in the same sequence, tb not a history frame,
 *             g = tb - ta with 1 <= g <= max_gap + 1
 *   shared    the joints present in both; s = their number
 *   size      per skeleton the larger of (max x - min x) and (max y - min y) over its present joints (0 with no joint or one);
 *             M = the larger size of the two
 *   D         the sum over the shared joints of dx^2 + dy^2, in int64
 *   pair      QUALIFIES iff s >= min_shared and D * 1 000 000 <= radius_permille^2 * g * M^2 * s: the mean squared displacement
 *             of the shared joints is at most (radius * M)^2 * g; the bound grows with the gap as a random walk's does
 *   cost      D * (12 252 240 / s), one int64; 12 252 240 = lcm(1 .. 18), so this is exactly that multiple of the mean squared
 *             displacement
 *   range     every |x|, |y| of every joint of a row, present or not, is below 2^14 (checked), so |dx| < 2^15, dx^2 + dy^2 <
 *             2^31, D < 18 * 2^31 < 2^36; D * 10^6 < 2^56; the right side is below 2^20 * 2^5 * 2^30 * 2^5 = 2^60; the cost is
 *             below 2^36 * 2^24 = 2^60: exact in int64, which the device keeps throughout (no float appears anywhere)
 *   match     the frames of a sequence are taken in ascending order.  At frame t the candidates are the qualifying pairs whose
 *             b lies in t and whose a is OPEN: not closed on input and without a successor so far.  They are ordered by
 *             (cost, g, a, b) ascending, a and b as global rows: a strict total order; they are walked in that order and a pair
 *             is linked iff a has no successor and b no predecessor yet
 * Outputs: prev (n_poses,) int32, the global row of the predecessor or -1 (history rows always -1); root (n_poses,) int32, the
 * row reached by following prev to its end (a row that links to nothing is its own root); links (n_frames,) int32, may be
 * NULL: the links made into each frame.  The device commits every mutually best pair of a frame round after round, which gives
 * the walk's answer; it depends on nothing the device schedules.  The matrix of qualifying pairs, one bit a pair and once per
 * side, lives in the context's scratch block (frames are processed in batches whose matrices fit 256 MiB, $TA_PT_MATRIX_BYTES
 * overrides; one frame at the limit with max_gap 30 takes about 130 MB).
 * Checked on the host before any launch, outputs untouched on failure.  TA_E_OVERFLOW: more than 4096 skeletons in one frame.
 * TA_E_INVALID: a negative count; frames_per_sequence that does not sum to n_frames, or pose_counts that does not sum to
 * n_poses; history_frames out of range; a NULL array that has rows; radius_permille outside 1 .. 1000; min_shared outside
 * 1 .. 18; max_gap outside 0 .. 30; any x, y of any joint of a row at or above 2^14 in size.  Zero sequences, empty frames
 * and sequences that are all history succeed. */
int ta_poses_track(ta_ctx* ctx, int n_sequences, const int32_t* frames_per_sequence, const int32_t* history_frames,
                   int n_frames, const int32_t* pose_counts, const int32_t* keypoints, const uint8_t* closed, int n_poses,
                   int radius_permille, int min_shared, int max_gap, int32_t* prev, int32_t* root, int32_t* links);

/* ---- where is this person?  skeletons painted into resident frames as silhouettes, in place ----------------------------- */
/* Host arrays, frames concatenated: pose_counts (n_frames,) int32 lists the FIRST n_frames frames of the batch (n_frames <= the
 * batch's n; later frames are untouched); keypoints (n_poses, 18, 3) int32 (x, y, present) as above: a joint is present iff its
 * third value is != 0, the x, y of an absent joint are ignored; rgba (n_poses, 4) uint8: ink r, g, b and alpha per pose;
 * radius_permille: three ints, one per class.  All arithmetic is integer, so the answer is defined bit for bit.
 *   size      M = the larger of (max x - min x) and (max y - min y) over the pose's present joints (0 with one joint); a pose
 *             with no present joint paints nothing
 *   classes   HEAD = 0, TORSO = 1, LIMB = 2; r_c = max(min_radius, M * radius_permille[c] / 1000), the product in int64, the
 *             division truncating
 *   joints    every present joint is a disc of its class's radius.  HEAD: joints 0, 14, 15, 16, 17; TORSO: 1, 2, 5, 8, 11;
 *             LIMB: 3, 4, 6, 7, 9, 10, 12, 13
 *   segments  each only if both its ends are present, a capsule of its class's radius.  HEAD: (0,1) (0,14) (14,16) (0,15)
 *             (15,17); TORSO: (1,2) (1,5) (1,8) (1,11) (8,11); LIMB: (2,3) (3,4) (8,9) (9,10) (5,6) (6,7) (11,12) (12,13)
 *   covered   pixel P = (px, py) by the segment A -> B of radius r, with d = B - A, L2 = d.d, p = P - A, t = p.d, all int64:
 *             if t <= 0: p.p <= r^2; else if t >= L2: |P - B|^2 <= r^2; else cross^2 <= r^2 * L2 with cross = p.x d.y - p.y d.x.
 *             Every comparison is inclusive.  A disc is the segment with A == B (L2 = 0, t = 0: the first case).  A pose covers
 *             a pixel iff one of its discs or capsules does
 *   range     every |x|, |y| of every joint of a row, present or not, is below 2^14 (checked) and a frame has at most 16384
 *             pixels a side (checked), so |p|, |d| < 2^15, L2 < 2^31, |t| < 2^31, |cross| < 2^31, cross^2 < 2^62, r < 2^15 and
 *             r^2 * L2 < 2^61: exact in int64, which the device keeps throughout (no float appears anywhere)
 *   paint     clear != 0: every byte of the listed frames is first set to 0 (by this call's own writes: a pixel nobody covers
 *             ends as 0).  Then the poses of a frame are applied in list order; a pixel is blended ONCE per pose that covers it,
 *             however many of that pose's shapes do; per band with a = the pose's alpha
 *                 v = in * (255 - a) + ink * a + 128;  out = ((v >> 8) + v) >> 8
 *             which is ta_frames_draw's blend (TA_DRAW_BAR).  Alpha 255 replaces, alpha 0 changes nothing.  With clear == 0 a
 *             listed frame with count 0 is not written at all, and no pixel outside a pose's coverage is written
 * The answer depends on nothing the device schedules: a pixel is owned by one thread, which walks the frame's poses in order.
 * Which poses a tile of pixels must look at is a tile x pose bit matrix in the context's scratch block (frames are processed in
 * batches whose matrices fit 256 MiB, a single larger frame in runs of its poses; $TA_PP_MATRIX_BYTES overrides).
 * Checked on the host before any launch, pixels untouched on failure.  TA_E_OVERFLOW: more than 16384 poses in one frame.
 * TA_E_INVALID: a negative count; pose_counts that does not sum to n_poses; n_frames above the batch's n; a NULL array that has
 * rows; a permille outside 0 .. 1000; min_radius outside 0 .. 4096; any x, y of any joint of a row at or above 2^14 in size; a
 * frame side above 16384.  n_frames == 0 and n_poses == 0 succeed (with clear they just clear the listed frames). */
int ta_poses_paint(ta_ctx* ctx, ta_frames* frames, int n_frames, const int32_t* pose_counts, const int32_t* keypoints,
                   const uint8_t* rgba, int n_poses, const int32_t radius_permille[3], int min_radius, int clear);

/* ---- where was this person in between?  tracked rows filled across missed frames and points ------------------------------ */
/* Host arrays, frames concatenated as in ta_poses_track: counts (n_frames,) int32, the frames consecutive frames of ONE
 * sequence; points (n_rows, n_points, 3) int32 (x, y, present): a point is present iff its third value is != 0, the x, y of
 * an absent point are ignored; n_points 1 .. 18: 18 for skeletons, 7 for faces (the two corners of the box and the five
 * landmarks); prev (n_rows,) int32, the global row of each row's predecessor or -1, exactly what ta_poses_track answers.  All
 * arithmetic is integer, so the answer is defined bit for bit.  G = max_gap + 1.
 *   frame(r)  the frame that row r lies in
 *   link      a = prev[b], d = frame(b) - frame(a) >= 1 (checked); a chain is the rows joined by links, whatever their d; no
 *             two rows have the same predecessor (checked), so a chain is a line and a row has at most one successor
 *   rows      every input row is an output row of its frame, in input order, first.  A link with 2 <= d <= G adds one
 *             SYNTHESIZED row to every frame t with frame(a) < t < frame(b); a link with d > G adds none.  The synthesized rows
 *             of a frame follow its real rows, ordered by their link's b ascending (b is a global row: a strict order)
 *   points    for output row R at frame t, of chain C, and point j: if R is a real row whose j is present, its x, y and third
 *             value are copied unchanged.  Otherwise let r0 be the nearest real row of C in a frame before t whose j is
 *             present, r1 the nearest one in a frame after t, t0 = frame(r0), t1 = frame(r1), (x0, y0) and (x1, y1) their j.
 *             If both exist and t1 - t0 <= G, the point is present with the third value `mark`, and each of x, y is
 *                 v = v0 + floor((2 * (v1 - v0) * (t - t0) + (t1 - t0)) / (2 * (t1 - t0)))      (floor division)
 *             the linear interpolation rounded to nearest, halves towards +infinity.  Otherwise the point is (0, 0, 0): a
 *             row in no chain, or one whose neighbours with that point are too far apart, keeps its absent points absent,
 *             nothing is held past a chain's first or last observation of a point, and nothing is filled across a link
 *             with d > G
 *   range     every |x|, |y| of every point of a row, present or not, is below 2^22 (checked), so |v1 - v0| < 2^23, t - t0
 *             <= 30 and t1 - t0 <= 31: the numerator is below 2^23 * 31 * 2 + 31 < 2^29 in size, exact in int32 (and in any
 *             wider type); the device keeps int32
 * Outputs: out_counts (n_frames,) int32, the rows of each output frame; out_points (n_out, n_points, 3) int32; out_source
 * (n_out, 2) int32: (r, r) for the real row r, (a, b) for a synthesized row of the link a = prev[b]; *n_out = n_rows + the sum
 * of d - 1 over the links that add rows, which a caller can compute from counts and prev alone.  The answer depends on nothing
 * the device schedules: the rank of a synthesized row is a prefix count over the rows of the G frames behind its frame,
 * walked in order by one workgroup, and every output word has one writer.  Scratch (the context's scratch block) is the
 * input, the output and four words a row; nothing grows faster than rows x points.
 * Checked on the host before any launch; outputs untouched on failure, except *n_out.  TA_E_OVERFLOW: more than 16384 input
 * rows, or more than 16384 output rows, in one frame; more than 2^31 - 1 output rows in all (*n_out = INT32_MAX); out_capacity
 * below the rows needed -- *n_out is then written with that number, so a caller may ask with capacity 0 (and NULL outputs).
 * TA_E_INVALID: a negative count; counts that do not sum to n_rows; a NULL array that has rows; n_points outside 1 .. 18;
 * max_gap outside 0 .. 30; mark outside 1 .. 255; any x, y of any point of a row at or above 2^22 in size; a prev that is
 * neither -1 nor a row of an earlier frame; two rows with the same prev (a chain, not a tree).  n_frames == 0, empty frames and
 * rows without links succeed.  n_out may be NULL. */
int ta_tracks_fill(ta_ctx* ctx, int n_frames, const int32_t* counts, const int32_t* points, int n_points,
                   const int32_t* prev, int n_rows, int max_gap, int mark, int32_t* out_counts, int32_t* out_points,
                   int32_t* out_source, int out_capacity, int32_t* n_out);

/* Workload statistics of the last ta_openpose_run / ta_openpose_group on this context: heat-map peaks found over
 * all images and parts (wrapper.py:235-262) and limb connections accepted by the greedy matching (wrapper.py:335-366). */
int ta_openpose_last_stats(const ta_ctx* ctx, int64_t* peaks, int64_t* connections);

/* Debug taps of the last ta_openpose_run / ta_openpose_group on this context (valid until the next call on it), for
 * parity tests of the seams between the grouping stages: per image and part the peaks found (wrapper.py:235-262, rows
 * in the reference's row-major order), per image and limb the connections kept by the greedy matching
 * (wrapper.py:335-366, in acceptance order).  n must equal the batch of that call.
 *   peak_counts (n,18) int32; peaks_yx (n,18,cap_peaks,2) int32 (y,x in the x8 map); peak_scores (n,18,cap_peaks) f32
 *   conn_counts (n,19) int32, -1 = limb skipped because one of its parts has no peak (wrapper.py:293-296);
 *   conn_ij (n,19,cap_conn,2) int32 (index into the source / destination part's peak list); conn_scores (n,19,cap_conn) f32
 * Rows beyond cap_* are dropped (the counts still report the true numbers). */
int ta_openpose_debug_read(ta_ctx* ctx, int n, int cap_peaks, int32_t* peak_counts, int32_t* peaks_yx,
                           float* peak_scores, int cap_conn, int32_t* conn_counts, int32_t* conn_ij,
                           float* conn_scores);
/* Which work area those taps come from: peak_capacity (n,) int32 = rows per part of image i's lists.  1024 for an
 * image the batch pass kept; an image that outgrew a list and was re-run alone reports the capacity its re-run was
 * sized to (its largest peak count of one part). */
int ta_openpose_debug_capacity(ta_ctx* ctx, int n, int32_t* peak_capacity);

/* x8 bicubic upsample alone (wrapper.py:214-223): maps (N,C,h,w) -> (N,C,8h,8w). */
int ta_bicubic_x8(ta_ctx* ctx, const float* maps, int n, int c, int h, int w, float* out);

/* ---- conv kernel selection (parity tests and tools) ------------------------------------------ */
/* Every dense conv / FC of the three networks runs on one of these implicit-GEMM kernels (terran_amd/csrc/conv_igemm.hip);
 * the library picks per layer (TA_CONV_AUTO).  ta_debug_conv_variant makes every following conv launch on this context
 * that the variant CAN run use it (layers it cannot run stay automatic); a packed model may also pin single convs to a
 * variant (ta_op_desc.variant, terran_amd/pack.py `variant=`), which fails with TA_E_INVALID when that kernel cannot run
 * the layer.  ta_debug_conv_counts reports (and optionally clears) the launches per variant since the last reset,
 * counts16[TA_CONV_*], so a parity test knows which kernels produced the numbers it compared (counts16[15]: how many
 * of those launches ran the split-role kernels' compile-time specialised epilogue rather than the generic one).
 * Under TA_CONV_AUTO a frame's result does not depend on the batch it arrives in (every kernel the automatic choice
 * can give one layer sums in the same order); a forced preference keeps the parity tolerances but not that bit-level
 * batch invariance (the symmetric-wave kernels pair K differently inside a slab and take no K-split). */
#define TA_CONV_AUTO 0
#define TA_CONV_GENERIC 1      /* K-offset table, any Cin, float32 activations                       */
#define TA_CONV_PIPE64 2       /* 64 cout x 128 px tiles, symmetric waves, 3-stage LDS ring          */
#define TA_CONV_PIPE128 3      /* 128 x 128 tiles, symmetric waves (float32 activations only)        */
#define TA_CONV_SPLIT_2x2 4    /* producer/consumer waves, 128 cout x 128 px                         */
#define TA_CONV_SPLIT_2x2_P8 5 /* ... with 8 producer waves                                          */
#define TA_CONV_SPLIT_2x4 6    /* producer/consumer waves, 128 cout x 256 px (8 consumer waves)      */
#define TA_CONV_SPLIT_1x4 7    /* producer/consumer waves, 64 cout x 256 px                          */
#define TA_CONV_WIN_2x2 8      /* ... 128 x 128 with the pixel operand of a channel block resident in LDS (stride-1 convs with >= 4 taps on
                                * pre-split half-float tensors; the K-split and the fused pool stay with the streaming kernels)  */
#define TA_CONV_WIN_2x4 9      /* ... 128 x 256                                                       */
#define TA_CONV_WIN_1x4 10     /* ... 64 cout x 256 px                                                */
#define TA_CONV_SPLIT_1x4_W2 11 /* producer/consumer waves, 64 x 256, 2-stage ring: TWO workgroups per CU (short-K layers)  */
#define TA_CONV_SPLIT_2x2_W2 12 /* ... 128 x 128                                                      */
int ta_debug_conv_variant(ta_ctx* ctx, int variant);
/* f16x3 mode: after ta_model_forward_* (the debug taps; the task entry points do this themselves), wait for the stream
 * and report whether an epilogue met |x| > 65504: TA_OK or TA_E_RANGE.  Clears the condition. */
int ta_debug_range_check(ta_ctx* ctx);
int ta_debug_conv_counts(ta_ctx* ctx, int64_t* counts16, int reset);
/* Algorithmic FLOPs per dense-conv kernel INSTANCE since the last reset, as text: one "name;launches;flops;ms" line per
 * template instance (ms: HIP-event time of the launches made while ta_ctx_profile was on) (the names rocprofv3 prints, without spaces: conv_igemm_split<2,4,4,3,3>).  Lets a per-kernel time
 * table from a profiler be turned into TFLOP/s per instance (profiles/summarize_round.py).  TA_E_CAPACITY if too small. */
int ta_debug_kernel_work(ta_ctx* ctx, char* csv, size_t capacity, int reset);

#ifdef __cplusplus
}
#endif
#endif /* TERRAN_AMD_H */
