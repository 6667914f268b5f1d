/*
 * dwtx.h — C ABI of the MI355X-native encode/decode hot path of xdsopl/dwt.
 *
 * The reference (/root/reference) has no FFI layer: its hot path is a set of
 * header-defined C functions called from two main()s.  This header declares the
 * entry points a maintainer would bind in their place; each cites the
 * reference call site / function it replaces.  Plain C types only: device and
 * host buffers are raw pointers, sizes are ints/size_t, errors are negative
 * ints like the reference's (-1 I/O or EOF, -2 capacity; see bytes.h:75-105).
 *
 * Conventions
 *   - `dev` pointers are HIP device pointers (from dwtx_malloc or any HIP
 *     allocator, e.g. a torch tensor's data_ptr()).  `host` pointers are plain
 *     host memory.
 *   - Images inside the library are PLANAR int32: plane p = image*C + channel,
 *     each plane H rows of W ints, row pitch W (dense).  The reference keeps
 *     interleaved int buffers (image.h:12-15); dwtx_planes_from_pixels /
 *     dwtx_pixels_from_planes convert at the edge, fused with the colour
 *     transform.
 *   - All functions are asynchronous on the context's stream unless they
 *     return data to the host; dwtx_sync() waits.
 *   - Thread-compatible: one context per host thread.
 */
#ifndef DWTX_H
#define DWTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWTX_OK            0
#define DWTX_ERR_IO       -1   /* bytes.h:79-83,99-103 */
#define DWTX_ERR_CAPACITY -2   /* bytes.h:77-78 */
#define DWTX_ERR_ARG      -3   /* encode.c:139-146, decode.c:145-159 (exit code 1 there) */
#define DWTX_ERR_DEVICE   -4   /* HIP runtime failure; dwtx_last_error() has the text */
#define DWTX_ERR_NOMEM    -5

#define DWTX_MAX_LEVELS 16
#define DWTX_MIN_LEN     8     /* encode.c:144, decode.c:157 */
/* Largest image side.  encode.c:140 lets sides up to 65536 through, but above 32768 the finest level's Hilbert square is
 * 65536 wide and encode.c:45 / decode.c:47 compute `lengths[l+1] * lengths[l+1]` in int: it wraps to 0, the finest ring
 * is never visited and the reference binary writes a stream its own decoder does not turn back into the picture.  There
 * is nothing to be bit-exact with beyond this side, so every entry point refuses it (DWTX_ERR_ARG; the CLIs exit 1 with
 * a message) — a documented difference, DESIGN.md section 7. */
#define DWTX_MAX_SIDE    32768

typedef struct dwtx_ctx dwtx_ctx;

/* Level geometry, utils.h:17-40.  Index 0 = root LL, index `levels` = full image. */
typedef struct dwtx_geom {
	int levels;
	int widths[DWTX_MAX_LEVELS];
	int heights[DWTX_MAX_LEVELS];
	int pixels[DWTX_MAX_LEVELS];
	int lengths[DWTX_MAX_LEVELS];
} dwtx_geom;

/* encode.c:175-180,226-230 stderr counters */
typedef struct dwtx_stats {
	int meta_bits;
	int root_bits;
	int total_bits;
	int kib;
	int levels;
	int planes[3];
} dwtx_stats;

/* Per-image result record of the entropy stage (device or host memory). */
typedef struct dwtx_stream_info {
	int planes[3];                 /* encode.c:163-165 */
	int pmax;
	int segments;                  /* (channel, level, plane) segments coded, encode.c:183-221 (all of the schedule unless CAPACITY cut it) */
	int entries;
	unsigned tokens;               /* VLI token slots (incl. void ones) */
	int order0;                    /* VLI order after header, root image and plane counts */
	unsigned hdr_bits;             /* 48 header bits + root image + plane counts */
	unsigned root_bits;            /* encode.c:179-180, as the reference counts it (CAPACITY can cut into the root image) */
	unsigned meta_bits;            /* encode.c:175-176: 48 unless CAPACITY < 6 */
	unsigned segments_cut;         /* segments of the schedule left uncoded because they start beyond CAPACITY (encode.c:192,204,216) */
	unsigned long long total_bits; /* encode.c:226: bit count before padding (8*capacity when truncated) */
	unsigned long long nbytes;     /* bytes of the .dwt stream: min(capacity, ceil(total_bits/8)) */
	int error;                     /* non-zero: unsupported data (more than 16 bit planes) */
	int exact_orders;              /* 1: the fast VLI-order pass did not resolve this image, the exact one ran */
} dwtx_stream_info;

/* Per-image result record of the decoder's entropy stage (host memory). */
typedef struct dwtx_decode_info {
	int status;                    /* 0 ok; 1 = header, root image or plane counts unreadable (decode.c exits 1);
	                                * 2 = the stream claims more than 16 bit planes: refused (decode.c:183-186 would go on;
	                                * only damage produces such a count — the one documented difference) */
	int W, H, C;
	int levels;
	int planes[3];                 /* decode.c:183-186 */
	int pmax;
	int level;                     /* finest level any segment touched (decode.c:197,203,219,236); -1 = none */
	int nsegs;
	int truncated;                 /* bit 0: the walk stopped early (end of data or PIXELS cap); bit 1: a read ran past
	                                * the end of the data (where decode prints bytes.h:101 "reached end of file") */
	int missing[48];               /* decode.c:193-196: planes not fully decoded, [channel*16 + level] */
	unsigned long long bits_used;
	unsigned hops, hopped_chunks;  /* token walker statistics: jumps over stitched 128-bit chunks */
	unsigned walked_tokens;        /* tokens the walker parsed itself */
	unsigned zeros_left;           /* run-length counter at the end; decode prints rle.h:45 "%d zeros not read." if > 1 */
} dwtx_decode_info;

/* ---- sidecar index ---------------------------------
 * Not part of the reference and never inside a .dwt: an optional companion that records, for every
 * (channel, level, plane) segment of decode.c:198-243's schedule, the decoder's state where the segment's first
 * pass begins (decode.c:67-100: stream position, vli.h:24 order, rle.h:25 run counter, how many coefficients
 * are still insignificant).  A decode that is given the index walks all segments at once instead of one after
 * the other; it checks on the way that the segments fit together, so a wrong, stale or foreign index cannot
 * change the result: the decoder then falls back to the plain walk.  A decode produces the index of every stream
 * it decodes to its end, and an encode that of every stream it writes whole (dwtx_ctx_set_encode_index). */
#define DWTX_INDEX_MAGIC 0x49545744u   /* "DWTI" */
#define DWTX_INDEX_MAX_SEGS 768         /* 3 channels x 16 levels x 16 planes */
typedef struct dwtx_seg_index {
	unsigned long long bit;            /* stream position of the segment's first pass */
	unsigned long long sym_base;       /* decoder-internal: first symbol slot of the segment */
	unsigned n1;                       /* symbols of the first pass */
	unsigned cnt;                      /* rle.h:25 on entry */
	unsigned desc;                     /* channel | level << 4 | (plane + 1) << 8 */
	unsigned order;                    /* vli.h:24 on entry */
} dwtx_seg_index;
typedef struct dwtx_index {
	unsigned magic;                    /* DWTX_INDEX_MAGIC */
	int W, H, C;
	int nsegs;                         /* 0: no index (stream unreadable, cut short, or decoded with a PIXELS cap) */
	int reserved;
	unsigned long long stream_bits;    /* bits of the stream the decoder used */
	dwtx_seg_index seg[DWTX_INDEX_MAX_SEGS];
} dwtx_index;

/* ---- context / memory ---------------------------------------------------- */

/* Create a context on HIP device `device` with a stream of its own. */
int dwtx_ctx_create(int device, dwtx_ctx **ctx);
/* Same, but run on an existing hipStream_t (e.g. torch's current stream);
 * NULL means the device's default stream. */
int dwtx_ctx_create_on_stream(int device, void *stream, dwtx_ctx **ctx);
void dwtx_ctx_destroy(dwtx_ctx *ctx);
const char *dwtx_last_error(void);
int dwtx_sync(dwtx_ctx *ctx);
/* Sidecar indices for the decode calls that follow on this context (dwtx_decode_planes / _device / _images):
 * entry i of `in` (may be NULL) is offered for image i of a call, entry i of `out` (may be NULL) receives the
 * index of image i (nsegs = 0 if it has none).  Both are host arrays that must stay valid until replaced;
 * dwtx_ctx_set_index(ctx, NULL, NULL) ends it. */
int dwtx_ctx_set_index(dwtx_ctx *ctx, const dwtx_index *in, dwtx_index *out);
/* Sidecar indices from the ENCODE calls that follow on this context: entry i of `out` receives the index of image i of
 * a call.  For dwtx_encode_planes / dwtx_encode_device `out` is DEVICE memory, written asynchronously on the context's
 * stream like dev_info; for dwtx_encode_images it is HOST memory, filled on return.  NULL ends it.  The encoder writes
 * the index the decoder would make of the same stream (only the header and seg[0 .. nsegs) of an entry are written); a
 * stream that CAPACITY shortened, a flat picture and one that is refused have none (nsegs = 0, stream_bits = 0).
 * Independent of dwtx_ctx_set_index, which belongs to the decode calls. */
int dwtx_ctx_set_encode_index(dwtx_ctx *ctx, dwtx_index *out);
void *dwtx_stream(dwtx_ctx *ctx);

/* Diagnostic switches of a context, all off (0) by default.  They exist for the tests, the profiling tools and
 * the CLIs' debugging aids: none of them changes a result, they choose between code paths that must agree
 * (DESIGN.md section 8).  The library itself reads no environment variables. */
enum dwtx_option {
	DWTX_OPT_EXACT_ORDERS = 0,     /* encoder: every image takes the exact 32-state VLI-order pass */
	DWTX_OPT_NO_SQUARE_TILES,      /* no tiles straight from / to the pyramid: everything through the linearised copy */
	DWTX_OPT_PART_IMAGES,          /* host-buffer pipelines: images per part (0 = automatic) */
	DWTX_OPT_ONE_STREAM,           /* decoder: the whole batch on one HIP stream (clean per-kernel profiles) */
	DWTX_OPT_DECODE_PARTS,         /* decoder: parts a batch is cut into, 2..4 (0 = automatic) */
	DWTX_OPT_TWO_FAMILIES,         /* decoder: both speculative path families from the start */
	DWTX_OPT_NO_SECOND_WALK,       /* decoder: a token walk that gives up is an error instead of being repeated */
	DWTX_OPT_NO_INDEX,             /* decoder: offered sidecar indices are ignored */
	DWTX_OPT_NO_INDEX_FALLBACK,    /* decoder: an index that is turned down is an error instead of the serial walk */
	DWTX_OPT_NO_CAPACITY_CUT,      /* encoder: CAPACITY only clips the finished stream (all segments are coded) */
	DWTX_OPT_NO_FINE16,            /* the finest ring stays in the int32 pyramid (no 16-bit planes for it) */
	DWTX_OPT_NO_FUSED_LEVELS,      /* transforms on int32 planes: one launch per level (no two-levels-per-pass kernels) */
	DWTX_OPT_NO_PIXELS16,          /* deep pixels: the finest level never reads / writes the uint16_t pixels itself (widened int32 planes in between) */
	DWTX_OPT_LIFT_ROWS,            /* transforms: row pairs per wave strip of every lifting launch, 4, 8, 16, 32 or 64 (0 = automatic, by the size of the batch);
	                                * the two-levels-per-pass kernels take max(2, value / 8) of their coarser row pairs; any other value: DWTX_ERR_ARG from the call */
	DWTX_OPT_COUNT_EVERY_PLANE,    /* decoder: the ones count reads every (plane, ring) segment, also those in which no one was set */
	DWTX_OPT_CROP_ROUTE,           /* dwtx_decode_view_crop: 1 = windowed levels above the LDS tail, 2 = the whole inverse transform into int32 planes and
	                                * a gather of the windows (what a picture that is all tail takes anyway); 0 = automatic; any other value: DWTX_ERR_ARG from the call */
	DWTX_OPT_COUNT
};
int dwtx_ctx_set_option(dwtx_ctx *ctx, int option, long value);
long dwtx_ctx_get_option(dwtx_ctx *ctx, int option);

void *dwtx_malloc(dwtx_ctx *ctx, size_t bytes);
void dwtx_free(dwtx_ctx *ctx, void *dev);
/* Page-locked host memory for the host-buffer entry points below: their transfers then overlap the
 * kernels of the previous part of the batch (pageable buffers work too, only slower). */
void *dwtx_host_alloc(dwtx_ctx *ctx, size_t bytes);
void dwtx_host_free(dwtx_ctx *ctx, void *host);
int dwtx_upload(dwtx_ctx *ctx, void *dev, const void *host, size_t bytes);
int dwtx_download(dwtx_ctx *ctx, void *host, const void *dev, size_t bytes);

/* ---- host-side geometry --------------------------------------------------- */

/* utils.h:28-40 compute_lengths(): same argument order and return value. */
int dwtx_compute_lengths(int *lengths, int *pixels, int *widths, int *heights, int W, int H, int N0);
int dwtx_geometry(dwtx_geom *g, int W, int H);

/* ---- stage kernels (device buffers, batches of n images) ------------------ */

/* Benchmark/test utility (no reference counterpart): render n synthetic 8-bit
 * frames [n][H][W][C] on the device with the integer-only generator of
 * SURVEY.md §8d; frame i uses seed seed0+i.  kind 0 = smooth+noise, 1 = noise. */
int dwtx_synth_pixels(dwtx_ctx *ctx, uint8_t *dev_pix, int W, int H, int C, int n, unsigned seed0, int kind);

/* pnm.h:69-74 widening + image.h:67-72 ycocg_from_rgb (C==3): interleaved
 * 8-bit pixels [n][H][W][C] -> planar int32 [n*C][H][W]. */
int dwtx_planes_from_pixels(dwtx_ctx *ctx, int32_t *dev_planes, const uint8_t *dev_pix, int W, int H, int C, int n);
/* image.h:74-79 rgb_from_ycocg (with its clamps, image.h:41-43) + pnm.h:108 clamp. */
int dwtx_pixels_from_planes(dwtx_ctx *ctx, uint8_t *dev_pix, const int32_t *dev_planes, int W, int H, int C, int n);

/* ---- deep pixels: samples of more than 8 bits (maxval up to 65535) ---------------------------------------------
 * The reference reads and writes 8-bit PNM only and calls that temporary (pnm.h:63-64 "only 8 bit per channel SRGB
 * supported at the moment"); nothing else in its algorithm knows the depth: encode.c:155-221 and decode.c:174-264
 * work on `int` throughout.  The *16 entry points are the same pipelines with native-endian uint16_t pixels,
 * interleaved [n][H][W][C] like the bytes, C = 1 or 3; strides of pixel buffers count SAMPLES (uint16_t elements).
 * The .dwt format is unchanged and records no depth: `maxval` (1..65535, else DWTX_ERR_ARG) is the caller's
 * knowledge, like the pixel format of a raw buffer.  Only the decoder needs it, for the clamps of image.h:41-43 and
 * pnm.h:108 with maxval where those have 255 — which only act on streams that were cut short.  With maxval 255 the
 * results are the 8-bit entry points', widened.  The coder's limit of 16 bit planes stays: a picture whose detail
 * coefficients need more is refused per image as ever (dwtx_stream_info.error).  Pictures with maxval <= 4095 never
 * are, gray ones up to 8191 neither; above that it depends on the data. */

/* pnm.h:69-74 widening + image.h:67-72 ycocg_from_rgb (C==3) for 16-bit samples. */
int dwtx_planes_from_pixels16(dwtx_ctx *ctx, int32_t *dev_planes, const uint16_t *dev_pix, int W, int H, int C, int n);
/* image.h:74-79 rgb_from_ycocg with the clamps of image.h:41-43 at maxval (Y to [0, maxval], Co and Cg to
 * [-maxval, maxval]) + pnm.h:108's clamp to [0, maxval]. */
int dwtx_pixels16_from_planes(dwtx_ctx *ctx, uint16_t *dev_pix, const int32_t *dev_planes, int W, int H, int C, int n, int maxval);

/* encode.c:16-30 transformation(): multi-level forward CDF 5/3 of `nplanes`
 * planar W*H images.  dev_in is preserved; dev_out receives the Mallat pyramid. */
int dwtx_transformation_fwd(dwtx_ctx *ctx, int32_t *dev_out, const int32_t *dev_in, int W, int H, int nplanes);
/* decode.c:16-30 transformation(): inverse.  dev_in (pyramid) is preserved. */
int dwtx_transformation_inv(dwtx_ctx *ctx, int32_t *dev_out, const int32_t *dev_in, int W, int H, int nplanes);

/* The same two transforms as the whole-image pipelines run them when the pictures are 8-bit pixels with W % 4 == 0 and more
 * than 64 pixels on a side (else DWTX_ERR_ARG: use the two calls above): encode.c:155-159 — widening, ycocg_from_rgb and
 * transformation() — in one pass over interleaved pixels [n][H][W][C], the finest level in packed 16-bit arithmetic; and
 * decode.c:258-264 — transformation(), rgb_from_ycocg with its clamps and write_pnm's clamp.  The detail rings of the up to
 * five finest levels (those in *levels16 / levels16, bit l = ring level l) are kept as int16 in dev_rings16 [n*C][H][W] —
 * same positions and pitch as in the pyramid, whose positions for those rings are then not touched; results are the
 * int32 transform's (an 8-bit source cannot leave 16 bits there: DESIGN.md section 4.1).  dev_rings16 == NULL: everything
 * in dev_pyr [n*C][H][W] int32.  What bench.py's `roofline_codec` times. */
int dwtx_transformation_fwd_pixels(dwtx_ctx *ctx, int32_t *dev_pyr, int16_t *dev_rings16, unsigned *levels16,
	const uint8_t *dev_pix, int W, int H, int C, int n);
int dwtx_transformation_inv_pixels(dwtx_ctx *ctx, uint8_t *dev_pix, const int32_t *dev_pyr, const int16_t *dev_rings16,
	unsigned levels16, int W, int H, int C, int n);

/* encode.c:155-159 and decode.c:258-264 for deep pixels, any shape: the two transforms as dwtx_encode_device16 /
 * dwtx_decode_device16 run them, everything in dev_pyr [n*C][H][W].  Pictures with W % 4 == 0, more than 64 pixels on a
 * side and 8-byte aligned pixels take the finest level straight from / to the uint16_t pixels (widening, colour transform
 * and clamps fused into it); every other shape goes through 16-bit ingest / egress kernels and widened int32 planes
 * (DWTX_OPT_NO_PIXELS16 forces that for all).  Same results either way. */
int dwtx_transformation_fwd_pixels16(dwtx_ctx *ctx, int32_t *dev_pyr, const uint16_t *dev_pix, int W, int H, int C, int n);
int dwtx_transformation_inv_pixels16(dwtx_ctx *ctx, uint16_t *dev_pix, const int32_t *dev_pyr, int W, int H, int C, int n, int maxval);

/* encode.c:32-58 linearization(): Mallat pyramid planes [nplanes][H][W] ->
 * Hilbert-linearised planes [nplanes][W*H] (root raster first, then the detail
 * ring of each level in curve order, hilbert.h:15-34). */
int dwtx_linearization(dwtx_ctx *ctx, int32_t *dev_lin, const int32_t *dev_pyr, int W, int H, int nplanes);
/* decode.c:32-65 reconstruction(): the inverse scatter, for the first
 * `levels_out` levels only (output planes are widths[levels_out] x
 * heights[levels_out], dense).  dev_missing is NULL or int[n][3][16] as in
 * decode.c:193-196 (planes not decoded per channel and level -> dequantisation
 * bias, decode.c:51-58). */
int dwtx_reconstruction(dwtx_ctx *ctx, int32_t *dev_pyr, const int32_t *dev_lin, const int *dev_missing,
	int levels_out, int W, int H, int C, int n);

/* encode.c:166-221: header, root image, plane counts, bit-plane segments in
 * schedule order, final run flush — for n images at once.  dev_lin is the
 * output of dwtx_linearization ([n*C][W*H], two's complement).  Image i's
 * stream is written to dev_out + i*out_stride (out_stride a multiple of 4, at
 * least 8, else DWTX_ERR_ARG; at most out_stride bytes are ever written, so it
 * should be >= capacity when capacity > 0).  capacity <= 0 means unlimited
 * (encode.c:150-152).  dev_info[i].nbytes and .total_bits are those of the
 * whole stream even when it is longer than out_stride: the slot then holds its
 * first out_stride bytes.  A stream that CAPACITY does not cut and that ends
 * inside its slot is followed by zeros up to min(out_stride, 4*ceil(nbytes/4) + 16)
 * bytes; the slot's bytes beyond are left as they were.  (When CAPACITY cuts,
 * the rest of the last segment coded may follow, up to out_stride.) */
int dwtx_encode_planes(dwtx_ctx *ctx, const int32_t *dev_lin, int W, int H, int C, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);

/* decode.c:174-250: root image, plane counts and all bit-plane segments of n
 * streams of identical geometry (W, H, C as in their headers) into linearised
 * two's-complement planes dev_lin [n*C][W*H] (zero where the stream ended
 * early).  Stream i occupies dev_streams + i*stream_stride (stride a multiple
 * of 8, at least 64), its byte length is dev_lens[i] (a length beyond the
 * stride is taken as the stride).  The decoder reads nothing outside the n
 * rows (no slack behind the last one), and whatever a row holds past its
 * stream's length — the rest of a longer stream, another stream, garbage —
 * does not change any result: a prefix decodes in place.  levels_max < 0 = all levels
 * (decode.c:163-171 computes it from the PIXELS argument).  Synchronous:
 * host_info[i] is filled on return (level and missing[] drive
 * dwtx_reconstruction / dwtx_transformation_inv). */
int dwtx_decode_planes(dwtx_ctx *ctx, int32_t *dev_lin, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max, dwtx_decode_info *host_info);

/* ---- whole-image pipelines (batches of n same-geometry images) -------------- */

/* A safe out_stride for unlimited-capacity encodes of W*H*C images (multiple of 8). */
size_t dwtx_encode_bound(int W, int H, int C);

/* The same for dwtx_encode_device16 / dwtx_encode_images16: the coder's 16 bit planes x 2 bits = 4 bytes per sample,
 * plus 4096, a multiple of 8 (encode.c:183-221 cannot write more for a picture that is not refused). */
size_t dwtx_encode_bound16(int W, int H, int C);

/* encode.c:155-221 with everything resident in HBM: 8-bit interleaved pixels
 * [n][H][W][C] -> n streams at dev_out + i*out_stride.  Asynchronous. */
int dwtx_encode_device(dwtx_ctx *ctx, const uint8_t *dev_pix, int W, int H, int C, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);

/* decode.c:174-264 with everything resident in HBM (streams as for
 * dwtx_decode_planes).  Image i is written densely at dev_pix + i*pix_stride
 * with the size the stream supports (widths/heights[host_info[i].level + 1],
 * decode.c:251-254); no other byte of dev_pix is written, so pix_stride may
 * carry padding and dev_pix needs no alignment.  A picture larger than
 * pix_stride is DWTX_ERR_ARG, and nothing is written for it.  Synchronises once
 * (after the token walk) to learn that size. */
int dwtx_decode_device(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max,
	uint8_t *dev_pix, size_t pix_stride, dwtx_decode_info *host_info);

/* encode.c:155-221 / decode.c:174-264 for deep pixels, everything resident in HBM: dwtx_encode_device /
 * dwtx_decode_device in every respect but the samples (pix_stride counts samples; dev_pix 2-byte aligned).  Encoding
 * takes no maxval: samples are what they are, and a picture that needs more than 16 bit planes gets
 * dev_info[i].error = 1 while the others of its batch are coded. */
int dwtx_encode_device16(dwtx_ctx *ctx, const uint16_t *dev_pix, int W, int H, int C, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_device16(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max,
	uint16_t *dev_pix, size_t pix_stride, int maxval, dwtx_decode_info *host_info);

/* ---- strided views: windows and tile grids of a larger frame ------------------------------------------------------
 * dwtx_encode_device / dwtx_decode_device (and their 16 versions) for pictures that are parts of something larger that
 * stays where it is in HBM: a crop, a pitch-aligned surface, a stack of padded pictures, or the tiles of a frame too big
 * to code whole — n same-geometry W x H windows, addressed by a row pitch and a grid.  All strides count SAMPLES, as in
 * the *16 calls.  Window i starts at dev + (i / cols) * band_stride + (i % cols) * image_stride, its row y row_pitch * y
 * further on.  Three layouts: a stack of padded pictures (cols = 0); a row of windows side by side in one frame
 * (image_stride = W*channels, row_pitch = the frame's width * channels); a whole tile grid in one call (cols tiles per
 * band, band_stride = H * row_pitch).
 * RGB pixels are interleaved (channel_stride = 0: sample c of pixel x at 3*x + c) or PLANAR, channel-first
 * (channel_stride != 0): a window is three planes channel_stride samples apart, each H rows of W samples, columns one
 * sample apart, rows row_pitch apart — torch's [N,3,H,W] and [3,H,W] as they lie, permuted to channel-last without a copy.
 * The window origin is channel 0's first sample; image_stride, band_stride and cols mean what they mean for interleaved
 * windows.  The streams are those of the interleaved copy: the .dwt format knows nothing of the layout. */
typedef struct dwtx_view {
	void  *dev;            /* first sample of window 0 */
	int    sample_bytes;   /* 1: uint8_t, 2: native-endian uint16_t (deep pixels; int16_t in the dwtx_*_view_signed calls and, with sgn, in the delta calls) */
	int    channels;       /* 1 or 3 (interleaved, or planar: channel_stride) */
	int    maxval;         /* decode: clamp bound (255 required when sample_bytes == 1); encode ignores it (but dwtx_encode_view_float: the quantiser's clamp) */
	int    cols;           /* windows per band; 0 or >= n: all n windows in one band */
	size_t row_pitch;      /* samples from a window's row to its next row, >= W*channels (planar: >= W) */
	size_t image_stride;   /* samples from a window to the next one of its band */
	size_t band_stride;    /* samples from a band's first window to the next band's */
	size_t channel_stride; /* 0: interleaved (sample c of pixel x at 3*x + c). Otherwise planar: channel c of a
	                          window starts c * channel_stride samples after the window's first sample, columns
	                          are 1 sample apart, rows row_pitch apart. Ignored when channels == 1. */
} dwtx_view;

/* dwtx_encode_device / dwtx_encode_device16 from a view: stream i and dev_info[i] are those of window i's pixels, the same
 * bytes as from a dense copy (a planar window's: those of its interleaved copy).  Only the W*channels samples of a window's
 * H rows are read (planar: the W samples of the H rows of its three planes); windows, and planes, may overlap.
 * DWTX_ERR_ARG (with a dwtx_last_error() text): row_pitch < W*channels (planar: < W), dev not aligned to sample_bytes. */
int dwtx_encode_view(dwtx_ctx *ctx, const dwtx_view *src, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
/* dwtx_decode_device / dwtx_decode_device16 into a view.  A stream that supports only ow x oh (cut short, or levels_max)
 * is written into its window's top-left corner, rows row_pitch apart; no sample outside the ow x oh rectangle of a window
 * is written — not in the rest of the window and not in the frame around it.  The windows must be provably disjoint, else
 * DWTX_ERR_ARG and nothing is written: with cols_eff = min(cols ? cols : n, n), either
 *   image_stride >= (H-1)*row_pitch + W*channels                                            (stacked), or
 *   image_stride >= W*channels and row_pitch >= (cols_eff-1)*image_stride + W*channels      (side by side);
 * and with more than one band, band_stride >= (cols_eff-1)*image_stride + (H-1)*row_pitch + W*channels.
 * A planar destination (channel_stride != 0, channels == 3): the ow x oh rectangle of each of the window's three planes is
 * written and no other sample.  With pw = (H-1)*row_pitch + W (a plane of a window) and nbands = ceil(n / cols_eff), one of
 * two forms must hold, else DWTX_ERR_ARG and nothing is written:
 *   planes inside the window (an NCHW stack): channel_stride >= pw, and with win = 2*channel_stride + pw:
 *     image_stride >= win if cols_eff > 1, band_stride >= (cols_eff-1)*image_stride + win with more than one band; or
 *   the planes of the whole view apart (a CHW frame, a tile grid of one, CNHW): the rules above for one channel (a row is W
 *     samples), and channel_stride >= (nbands-1)*band_stride + (cols_eff-1)*image_stride + pw.
 * Both are sufficient, not necessary, like the rules above. */
int dwtx_decode_view(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max,
	const dwtx_view *dst, dwtx_decode_info *host_info);

/* ---- pixel step: pixels that lie further apart than their own samples ------------------------------------------------
 * dwtx_encode_view / dwtx_decode_view for surfaces whose pixels are more than the coded channels: the RGB of an RGBA8 /
 * RGBX8 render target (channels 3, pixel_step 4), its alpha (channels 1, dev + 3, pixel_step 4), one chroma plane of NV12
 * (channels 1, pixel_step 2), one plane of a Bayer mosaic (channels 1, pixel_step 2, twice the frame's row pitch).
 * pixel_step counts SAMPLES like every stride of a view: sample c of pixel x of a window's row lies x * pixel_step + c
 * samples after the row's first sample.  Everything else the dwtx_view says keeps its meaning, so grids of tiles, stacks
 * and deep samples work with a step; dwtx_view itself is unchanged.  pixel_step == 0 or == channels is the dense case:
 * the call is then dwtx_encode_view / dwtx_decode_view in every respect.  The streams are those of the dense interleaved
 * copy: the .dwt format knows nothing of the layout.  (An RGBA surface is an RGB stream and a gray stream, in two calls;
 * the channel order is R, G, B as it lies; B, G, R surfaces: dwtx_*_view_order below.)
 * With row = (W-1)*pixel_step + channels, the samples from a window row's first to behind its last, DWTX_ERR_ARG (with a
 * dwtx_last_error() text, nothing written): pixel_step non-zero and below channels; a planar view (channels == 3,
 * channel_stride != 0) with any step but 0 and 3 — the rows of a plane stay dense; row_pitch < row.
 * Encode: only the windows' samples are read — the `channels` samples of each of the W pixels of a window's H rows.  One
 * exception: 8-bit RGB in 4-byte pixels (sample_bytes 1, channels 3, pixel_step 4) whose dev, row_pitch, image_stride and
 * band_stride are multiples of 4 — pictures with W % 4 == 0 and more than 64 pixels on a side are then read a pixel's four
 * bytes at a time: the fourth byte of a window's OWN pixels is loaded and never used.  The pixel is 4-byte aligned there,
 * so that byte is addressable whenever the pixel is.  Nothing else of the surface is read. */
int dwtx_encode_view_step(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
/* Decode: the disjointness rules of dwtx_decode_view hold with that `row` in place of W*channels, in the stacked, the
 * side-by-side and the band form alike (the bounds themselves are accepted).  The `channels` samples of each pixel of the
 * ow x oh rectangle a stream supports are written and NO OTHER SAMPLE, in particular not the pixel_step - channels samples
 * between two pixels — the alpha byte of an RGBA surface, the other planes of a mosaic: another stream may be writing
 * those at the same moment, so nothing is read, merged and written back there. */
int dwtx_decode_view_step(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, dwtx_decode_info *host_info);

/* ---- channel order: B, G, R pixels coded where they lie --------------------------------------------------------------
 * dwtx_encode_view_step / dwtx_decode_view_step for surfaces whose three channels lie the other way round: B8G8R8A8 / BGRX
 * swap-chain and capture surfaces (channels 3, pixel_step 4), video decoders' RGB outputs, OpenCV's BGR Mat (channels 3,
 * pixel_step 0).  `order` says which colour the three channels of a pixel are AS THEY LIE IN MEMORY: with DWTX_ORDER_BGR,
 * memory sample 0 of an interleaved pixel is B and sample 2 is R; of a planar view (channel_stride != 0) the plane at dev
 * is B and the plane at dev + 2*channel_stride is R.  dev stays the lowest-addressed channel's first sample, and every
 * stride keeps its meaning.  Every rule of the calls above holds word for word as it does for RGB: row length and
 * alignment, the disjointness of destinations, "no other sample written", and the one documented read of a pixel's own
 * fourth byte (8-bit pixels on the 4-byte grid are read and written by the same wide kernels in either order; a view
 * takes the same path whatever its order).
 * The streams are those of the dense interleaved R, G, B copy: a BGR view and the channel-reversed copy of it encode to the
 * same bytes, and a decode writes what the RGB decode would, with R and B at each other's places.  The clamps of a
 * truncated stream's decode (image.h:41-43, pnm.h:108) act on the colours, not on memory positions.
 * DWTX_ORDER_RGB is dwtx_*_view_step in every respect.  Any other value is DWTX_ERR_ARG (with a dwtx_last_error() text,
 * nothing written).  `order` is ignored when channels == 1, as channel_stride is.
 * Alpha-first surfaces (A8R8G8B8: DWTX_ORDER_RGB, A8B8G8R8: DWTX_ORDER_BGR) are the same calls with dev + 1 and pixel_step 4.
 * Their pixels leave the 4-byte grid, so they take the general conversions, not the wide kernels: correct, and slower. */
enum { DWTX_ORDER_RGB = 0, DWTX_ORDER_BGR = 1 };
int dwtx_encode_view_order(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_order(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, dwtx_decode_info *host_info);

/* ---- float views: decode straight into, and encode straight from, fp32, fp16 and bf16 tensors ------------------------
 * dwtx_decode_view_order for destinations that hold floating-point samples: what a training or inference pipeline does
 * with a decoded batch on its next line — `x.float() * scale + bias`, or `.half()` — without the integer frame in between,
 * its second pass and its memory.  (Float sources: dwtx_encode_view_float below, whose quantiser is part of its contract.)
 * Destination: dst->sample_bytes must equal the size of fmt->type (4, or 2 for the two half types); every stride of the
 * view, and pixel_step, count samples of that type; dev is aligned to the sample.  dst->maxval is what the streams were
 * encoded from, 1..65535: the same call covers 8-bit and deep streams.
 * Value written: for colour c of a pixel, with v the integer that dwtx_decode_view_order would write there with that maxval
 * (all clamps of image.h:41-43 and pnm.h:108 applied, on colours): f = (float)v * scale[c], rounded to fp32, then
 * f + bias[c], rounded to fp32 — two roundings, no fused multiply-add: bit for bit the unfused line above — then converted
 * to fmt->type, round to nearest even.  fp16 overflow goes to infinity and fp16 subnormals are kept, as torch's conversion
 * does; what becomes of an fp32-subnormal intermediate is not pinned.  scale and bias belong to COLOURS (R, G, B), not to
 * memory positions: with DWTX_ORDER_BGR the sample at the lowest address gets scale[2] and bias[2].  Gray uses [0].
 * Everything the integer views guarantee holds word for word: only the `channels` samples of the pixels of the ow x oh
 * rectangle a stream supports are written, nothing between pixels, nothing of the frame around the windows; the
 * disjointness rules apply with the same formulas; planar, stacked, side-by-side and band forms are accepted; pixel_step
 * and order keep their meaning; the windows of streams with status 1 or 2 are left untouched.
 * Gray and planar RGB windows with W % 4 == 0, more than 64 pixels on a side and every row on the quad grid of the float
 * sample (16 bytes for fp32, 8 for the half types) are written by the inverse transform's last level itself; every other
 * view (interleaved float RGB among them) through int32 planes and the general conversion — the same bits, one pass more.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): fmt == NULL, an unknown type, a sample_bytes that does not
 * match the type, a scale or bias that is not finite, and everything dwtx_decode_view_order refuses. */
enum { DWTX_FLOAT32 = 0, DWTX_FLOAT16 = 1, DWTX_BFLOAT16 = 2 };
typedef struct dwtx_float_format {
	int   type;       /* DWTX_FLOAT32 / _FLOAT16 / _BFLOAT16 */
	float scale[3];   /* per COLOUR (R, G, B — not memory position); gray uses [0] */
	float bias[3];
} dwtx_float_format;
int dwtx_decode_view_float(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order,
	const dwtx_float_format *fmt, dwtx_decode_info *host_info);

/* dwtx_encode_view_order for sources that hold floating-point samples: a model's output in [-1, 1], a renderer's tone-mapped
 * frame — without the line `(x.float() * s + b).round().clamp(0, maxval).to(uint8)`, its launches, its temporaries and the
 * integer copy of the batch in between.  The quantiser is part of the contract, so the stream is the lossless code of a
 * picture that is defined bit for bit.
 * Source: src->sample_bytes must equal the size of fmt->type (4, or 2 for the two half types); every stride of the view,
 * and pixel_step, count samples of that type; dev is aligned to the sample.  Asynchronous on the context's stream.
 * The picture that is coded: for colour c of a pixel holding the sample x, widened exactly to fp32 (fp16 subnormals kept):
 *   m = x * scale[c], rounded to fp32;  r = m + bias[c], rounded to fp32 — two roundings, no fused multiply-add —;
 *   q = rint(r): to nearest, ties to even (torch.round, np.rint);  v = min(max(q, 0), maxval),
 * with NaN -> 0, +inf -> maxval, -inf -> 0 and -0.0 -> 0.  What becomes of an fp32-subnormal m or r is not pinned (it
 * quantises to 0 or to the same integer either way).  src->maxval is the clamp bound, 1..65535: the one encode that reads
 * it.  scale and bias belong to COLOURS (R, G, B), not to memory positions: with DWTX_ORDER_BGR the sample at the lowest
 * address takes scale[2] and bias[2].  Gray uses [0].
 * Stream i and dev_info[i] are byte for byte those of dwtx_encode_device (maxval <= 255) or dwtx_encode_device16 (maxval
 * above) on the dense interleaved R, G, B picture of those v; capacity, out_stride, the zero padding after a stream and
 * the encode index (dwtx_ctx_set_encode_index) keep their meaning, and so does the refusal of a picture that needs more
 * than 16 bit planes (dev_info[i].error = 1, the others of its batch are coded): with maxval <= 4095 none is refused.
 * dwtx_encode_bound (maxval <= 255) and dwtx_encode_bound16 (maxval > 255) are the safe out_strides.
 * Only the `channels` samples of the W pixels of a window's H rows are read (planar: the W samples of the H rows of its
 * three planes): nothing between stepped pixels, nothing of the frame around the windows — there is no counterpart of the
 * 8-bit RGBX path's read of a pixel's own fourth byte.  Windows and planes may overlap, as for any encode.
 * Gray and planar RGB windows with W % 4 == 0, more than 64 pixels on a side and every row on the quad grid of the float
 * sample (16 bytes for fp32, 8 for the half types) are read and quantised by the forward transform's finest level itself;
 * every other view (interleaved float RGB among them) through the general conversion into int32 planes — the same bytes.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written to dev_out or dev_info): fmt == NULL, an unknown type, a
 * sample_bytes that does not match the type, a scale or bias that is not finite, a maxval outside 1..65535, and everything
 * dwtx_encode_view_order refuses. */
int dwtx_encode_view_float(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order,
	const dwtx_float_format *fmt, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);

/* ---- crop decode: a window of each picture straight into a view ---------------------------------------------------------
 * dwtx_decode_view_order (fmt == NULL: integer samples) or dwtx_decode_view_float (fmt given) for the step an image pipeline
 * takes next: a training loader's random crop, a viewer's viewport, one detection box of a large frame — without the
 * full-size frame, the inverse transform and the egress of what nobody keeps, and the copy per picture that crops with
 * origins of their own need afterwards.  W, H are the streams' geometry; the windows of dst are crop_w x crop_h, and every
 * rule of the plain call holds word for word with the crop's sides in place of the picture's: disjointness, row length,
 * alignment, the planar forms, pixel_step, order and maxval.  A crop side may be anything from 1 up (the 8-pixel minimum
 * belongs to pictures, not to windows).  host_origins: [n][2] ints in host memory, (x0, y0) of picture i's crop, read
 * before the call returns; NULL: all (0, 0).
 * Contract: let P_i be what the plain call would write into a full W x H window for stream i — the ow x oh picture the stream
 * supports, all clamps and the missing-plane bias of decode.c:51-58 applied.  Sample (x, y) of window i receives
 * P_i(x0_i + x, y0_i + y) for every (x0_i + x, y0_i + y) inside ow x oh, and NO OTHER SAMPLE is written: not the rest of the
 * window when the stream came out reduced, not the space between stepped pixels, not the frame around the windows, not the
 * windows of streams with status 1 or 2.  A crop that lies wholly outside a reduced picture writes nothing.  host_info[i]
 * is exactly what the plain call reports, and the call synchronises where the plain call does.
 * With crop_w == W, crop_h == H and all origins (0, 0) the call IS the plain call: it takes its path.
 * Otherwise the entropy stage runs as ever, with every ring in the int32 pyramid (as under DWTX_OPT_NO_FINE16); above the
 * LDS tail (levels of at most 64 per side) the inverse transform rebuilds only the rectangle of each level that the crop
 * needs (dwtx_crop_plan), and the general conversion writes the windows.  DWTX_OPT_CROP_ROUTE chooses between that and
 * the whole inverse transform followed by a gather; the results are the same.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): crop_w outside 1..W or crop_h outside 1..H; an origin with
 * x0 < 0, y0 < 0, x0 + crop_w > W or y0 + crop_h > H; and everything the plain calls refuse. */
int dwtx_decode_view_crop(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, dwtx_decode_info *host_info);

/* Host arithmetic only, like dwtx_tile_groups: the rectangle of every level that the cw x ch crop at (x0, y0) of a W x H
 * picture needs.  out[l] is the rectangle of the widths[l] x heights[l] LL band (dwtx_geometry; l = levels is the picture
 * itself, l = 0 the root) that must be held — and, at the same coordinates, of each of the three detail bands beside it —
 * clipped to the band.  From icdf53 (cdf53.h:36-61): sample 2k is s[k] - (d[k-1] + d[k]) / 4 (cdf53.h:40-46), sample 2k+1
 * is d[k] + (x[2k] + x[2k+2]) / 2 (cdf53.h:47-53), so outputs [xa, xb) — the pairs k0 = xa / 2 .. ceil(xb / 2) - 1 — need
 * columns k0 - 1 .. k1 = ceil(xb / 2) of the level below, and rows likewise (decode.c:21-29 undoes columns first, so the
 * row pass's inputs are the column pass's outputs and both bands' margins apply to all four bands).  Returns `levels`;
 * DWTX_ERR_ARG for a picture no entry point takes, a crop side below 1 and a crop that leaves the picture. */
typedef struct dwtx_crop_rect { int x0, y0, w, h; } dwtx_crop_rect;
int dwtx_crop_plan(int W, int H, int x0, int y0, int cw, int ch, dwtx_crop_rect out[DWTX_MAX_LEVELS + 1]);

/* ---- window lists: encode from and decode into one pointer per picture ---------------------------------------------------
 * The most general view call of each direction — dwtx_encode_view_order or dwtx_encode_view_float (fmt given), and
 * dwtx_decode_view_crop — for windows that lie on no grid: separately allocated pictures (a list of tensors, a decoder's
 * surface pool, the images of a swap chain), patches at arbitrary places of a frame (detection boxes of one size), a subset
 * or a permutation of a tile grid (only the dirty tiles, tiles in priority order).
 * host_windows: [n] device pointers in HOST memory, read before the call returns — the caller may free or overwrite the
 * array at once, after the asynchronous encode too.  Entry i is window i's lowest-addressed channel's first sample: what
 * `dev` is for window 0 of a grid.  view->dev, cols, image_stride and band_stride are ignored (dev may be NULL); row_pitch,
 * channel_stride, sample_bytes, channels, maxval, pixel_step, order and fmt keep their meaning word for word.  A list that
 * spells out a grid gives exactly what the grid call gives: streams, dev_info and host_info, every written sample, and
 * nothing else written.  host_windows == NULL is DWTX_ERR_ARG, not silently the grid call.
 * Encode: windows may overlap and a pointer may occur twice; stream i is that of window i's dense interleaved R, G, B copy.
 * Asynchronous on the context's stream; the call does not wait for earlier work on that stream (the table travels through
 * a page-locked buffer of the context; a second listed call waits for the first one's table to have left that buffer).
 * Decode: with crop_w == W, crop_h == H and host_origins == NULL (or all (0, 0)) the plain decode; otherwise the rules of
 * dwtx_decode_view_crop with the listed windows of the crop's size.  The windows must be provably disjoint, else
 * DWTX_ERR_ARG and nothing is written.  The units are the n windows, for planar RGB the 3n planes at p_i + c *
 * channel_stride, with the crop's sides where there is a crop.  With row = W for a plane, else (W-1)*step + channels (step:
 * pixel_step, or channels), pitch = row_pitch and span = (H-1)*pitch + row, every two units, their first samples d samples
 * apart, must meet one of
 *   d >= span                                                  (one unit ends before the other begins), or
 *   with dx = d % pitch: dx >= row and dx + row <= pitch       (different columns of one pitch lattice: tiles or boxes
 *                                                               side by side in one frame).
 * Sufficient, not necessary, like the rules of dwtx_decode_view.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): a NULL entry; an entry not aligned to sample_bytes; more
 * windows than a call takes (65535 planes to encode, 21845 streams to decode); and everything the plain call of the same
 * direction refuses.
 * Gray, interleaved or planar windows are read / written by the transform's finest level itself when the grid call's
 * conditions hold for row_pitch and channel_stride and EVERY pointer is on the lane's quad, 4 * sample_bytes bytes; one
 * pointer off the quad sends the whole call through the general conversions: the same bytes. */
int dwtx_encode_view_list(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order,
	const dwtx_float_format *fmt /* NULL: integer samples */, const void *const *host_windows,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_list(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows, dwtx_decode_info *host_info);
/* Host arithmetic only, like dwtx_crop_plan: what the two calls above accept of a list — DWTX_OK, or the DWTX_ERR_ARG (and
 * text) they would return for the view, the step and the list.  W x H: the windows' sides (the crop's where there is one,
 * from 1 up); dst != 0: the list is a decode's and must be disjoint.  A view of 4-byte samples is taken for fp32 samples. */
int dwtx_view_list_check(const dwtx_view *v, size_t pixel_step, int W, int H, int n, const void *const *host_windows, int dst);

/* ---- flips in views: bottom-up surfaces and mirrored pictures coded in place ------------------------------------------------
 * The most general call of each direction — dwtx_encode_view_list and dwtx_decode_view_list — plus a flip per window, for
 * pictures whose rows run upwards (OpenGL read-backs, BMP / DIB sections, arrays with y pointing up) or whose columns run
 * backwards (a loader's random horizontal flip): every stride of a dwtx_view is a size_t, so neither can be written as a
 * view, and the caller's flip before an encode or after a decode is a pass over the batch.  (No reference counterpart: the
 * reference reads and writes upright PNM files and nothing else.)
 * Everything the two list calls say about their arguments holds, except that host_windows == NULL is allowed here and means
 * the grid the view describes, as in dwtx_encode_view_float and dwtx_decode_view_crop.  Window i's flags are host_flips ?
 * host_flips[i] : flip, a mask of DWTX_FLIP_X and DWTX_FLIP_Y.  host_flips is [n] bytes of HOST memory, read before the call
 * returns, like host_windows, after the asynchronous encode too.
 * Contract: let the window's sides be Ww x Hw (W x H, or crop_w x crop_h where there is a crop).  Memory position (x, y) of
 * window i is what it is in every other view call: the pixel whose samples lie at first_i + y * row_pitch + x * step (+ c, or
 * + c * channel_stride), first_i the window's lowest-addressed sample as the view or the list gives it.  A flip changes no
 * stride, no `dev` and no pointer: with flags f, memory position (x, y) holds pixel (u, v) of the window's picture, where
 *   u = (f & DWTX_FLIP_X) ? Ww - 1 - x : x        v = (f & DWTX_FLIP_Y) ? Hw - 1 - y : y.
 * order, pixel_step, channel_stride, scale and bias keep their meaning (scale and bias belong to colours).  A flip does not
 * change which samples a window covers, so row length, alignment and the disjointness rules are the unflipped call's.
 * Encode: stream i and dev_info[i] are byte for byte those of the dense interleaved R, G, B picture Q(u, v) = memory(x(u),
 * y(v)); only the windows' samples are read.
 * Decode: with P_i the plain call's picture (dwtx_decode_view_crop), memory position (x, y) receives P_i(x0 + u, y0 + v) for
 * every (x0 + u, y0 + v) inside ow x oh, and NO OTHER SAMPLE is written: a picture that comes out reduced lies in the corner
 * of its window where its pixel (0, 0) lies — with DWTX_FLIP_Y the bottom rows, with DWTX_FLIP_X the right-hand columns.
 * host_info is the plain call's, and the call synchronises where the plain call does.
 * With all flags 0 the call IS dwtx_encode_view_list / dwtx_decode_view_list when host_windows is given, and otherwise
 * dwtx_encode_view_float (fmt given), dwtx_encode_view_order or dwtx_decode_view_crop: it takes their path.
 * A call with any flag set travels as a listed one (a grid is spelled out on the host) with the flags in the top two bits of
 * each window's 8-byte table entry.  Wherever the unflipped call's windows are read / written by the transform's finest level
 * itself, a flipped call's are too, per window: every wave takes its window's first row and the sign of the pitch from the
 * table (DWTX_FLIP_Y, both directions), and a DECODE writes a mirrored window's quads at the mirrored place with their four
 * pixels reversed (DWTX_FLIP_X: gray, planar, interleaved RGB and RGBX sinks of every sample type; a window wider than its
 * reduced picture must then have Ww % 4 == 0).  An ENCODE with one mirrored window (DWTX_FLIP_X) goes through the general
 * conversion into int32 planes, like an alpha-first surface — the same bytes, one pass more: the forward kernels' halo words
 * would swap sides.  Crops, and views off the quad grid, take the general conversions as they do unflipped.  (Measured:
 * DESIGN.md section 4.19.)
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): a flag outside 0..3; a non-zero `flip` together with
 * host_flips; and everything the list calls (host_windows given) or the grid calls (NULL) refuse. */
enum { DWTX_FLIP_X = 1, DWTX_FLIP_Y = 2 };
int dwtx_encode_view_flip(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order,
	const dwtx_float_format *fmt /* NULL: integer samples */, const void *const *host_windows /* NULL: the view's own grid */,
	int flip, const unsigned char *host_flips /* [n] or NULL */,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_flip(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows /* NULL: the view's own grid */,
	int flip, const unsigned char *host_flips, dwtx_decode_info *host_info);
/* Host arithmetic only, like dwtx_view_list_check: DWTX_OK, or the DWTX_ERR_ARG (and text) the two calls above would return
 * for this view, step, list and flags — and the one table the kernels walk a flipped window with.  W x H: the windows' sides
 * (the crop's where there is one); dst != 0: the windows are a decode's.  origin[i]: where pixel (0, 0) of window i's PICTURE
 * lies — its lowest-addressed channel — in samples from v->dev (a grid) or from the lowest pointer of the list; pitch[i] and
 * step[i]: the signed row pitch and pixel step with which the picture is walked from there (negative where the flag is set).
 * Each of the three may be NULL.  A view of 4-byte samples is taken for fp32 samples. */
int dwtx_view_flip_plan(const dwtx_view *v, size_t pixel_step, int W, int H, int n, const void *const *host_windows,
	int flip, const unsigned char *host_flips, int dst, long long *origin /* [n] */, long long *pitch /* [n] */, long long *step /* [n] */);

/* ---- signed samples: int16_t pictures coded as they are ------------------------------------------------------------------------
 * The most general call of each direction — dwtx_encode_view_flip and dwtx_decode_view_flip — for pictures whose samples are
 * signed: CT slices in Hounsfield units, elevation tiles, sensor frames after black-level subtraction, residuals.  Nothing in
 * the algorithm knows a sign of the samples: encode.c:97-131 codes signs in the root image and in every plane (Co and Cg are
 * negative in every RGB picture), and image.h:53-65 is reversible on any int.  The .dwt format is unchanged, with no new field:
 * the coded picture is the signed integers as they lie, RGB through YCoCg-R on signed ints.  The range is the caller's knowledge,
 * as maxval is: [minval, maxval] with -32768 <= minval < maxval <= 32767.  With R = maxval - minval, the decoder's clamps
 * (image.h:41-43, pnm.h:108) become: gray and Y to [minval, maxval], Co and Cg to [-R, R], every output sample to [minval,
 * maxval] — with minval = 0 today's clamps; they only act on streams that were cut short.  (No reference counterpart beyond
 * those lines: the reference reads and writes 8-bit PNM.)
 * Everything the two flip calls say about their arguments holds word for word; `minval` is the one argument more.
 * Encode, integer samples (fmt NULL): src->sample_bytes must be 2; the samples are native-endian int16_t and are coded as they
 * are; minval and src->maxval are not read.  Float samples (fmt given): the quantiser of dwtx_encode_view_float with
 * v = min(max(q, minval), maxval); NaN and -0.0 -> 0, clamped into the range; +inf -> maxval, -inf -> minval.  Streams and
 * dev_info are byte for byte those of the reference's stages (encode.c:155-221) on that integer picture: the same bytes as
 * dwtx_encode_device16's where no sample is negative.  dwtx_encode_bound16 is the safe out_stride.  A picture that needs more
 * than 16 bit planes is refused as ever (dev_info[i].error = 1, the others of its batch are coded): with R <= 4095 none is,
 * gray ones with R <= 8191 neither.
 * Decode: the upper bound is dst->maxval.  Integer destinations are int16_t (sample_bytes 2), two's complement.  Float
 * destinations receive (float)v * scale + bias of the signed, clamped v, under dwtx_decode_view_float's rounding contract.
 * Everything the view calls guarantee holds word for word: nothing written outside the ow x oh rectangle, the disjointness
 * rules, status 1 / 2 windows untouched, crops, lists, flips, reduced pictures in their corners, planar, step, B-G-R.
 * Equivalences: fmt given and minval == 0: the call IS the flip call and takes its path.  Integer samples all in [0, 32767]: the
 * encode gives the bytes of the unsigned call.  minval == 0: the decode gives the unsigned call's samples bit for bit.
 * Route: signed pictures, and float sources with minval < 0, take the deep pictures' route in every respect (histograms from
 * the entropy stage's own pass, no 16-bit ring planes; DWTX_OPT_NO_PIXELS16 covers them).  Wherever a uint16_t view is read /
 * written by the transform's finest level itself, an int16_t view of the same layout is too — gray, interleaved, planar and
 * B-G-R, windows and lists, bottom-up both ways and mirrored decodes — and float views keep their path whatever minval is;
 * every other view goes through the general conversions: the same bytes.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): a range outside the rule above (decodes, and float encodes
 * with minval != 0); sample_bytes 1 without fmt; and everything the flip calls refuse. */
int dwtx_encode_view_signed(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order,
	const dwtx_float_format *fmt /* NULL: int16_t samples */, const void *const *host_windows /* NULL: the view's own grid */,
	int flip, const unsigned char *host_flips /* [n] or NULL */, int minval,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_signed(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows /* NULL: the view's own grid */,
	int flip, const unsigned char *host_flips, int minval, dwtx_decode_info *host_info);

/* ---- delta views: a picture coded as its difference from a base view -----------------------------------------------------------
 * Residual coding without the caller's pass over the batch: a CT slice against the slice before it, a static camera's frame
 * against its background plate, a render against the previous frame.  The .dwt format is unchanged, with no new field: the coded
 * picture is the integers D = S - B, and the base is the caller's knowledge, as maxval is.  (No reference counterpart beyond the
 * stages named below: the reference codes the pictures it is given.)
 * Views: `src` / `dst` and `base` are two grid views of n windows of W x H, window i of `base` belonging to window i of the
 * other.  Each has its own dev, cols, row_pitch, image_stride, band_stride, channel_stride and pixel step — a pitched base under
 * a dense picture, a planar one under an interleaved one —; channels (1 or 3), sample_bytes (1 or 2), the sample type and
 * `order` are shared.  sgn == 0: uint8_t or uint16_t samples, and minval must be 0.  sgn == 1: int16_t samples (sample_bytes 2)
 * and the range rule of the signed calls for [minval, dst->maxval].  base->maxval is not read; an encode reads no maxval at all.
 * Encode: asynchronous on the context's stream.  D = S - B on integers, per colour (with DWTX_ORDER_BGR both views lie as B, G,
 * R); stream i and dev_info[i] are byte for byte those of the reference's stages (encode.c:155-221) on the integer picture D.
 * Both views are only read and may overlap each other and themselves in any way: frames 1.. of a stack against frames 0.. is
 * one call.  A residual lies in [-R, R], R = maxval - minval, twice its pictures' range: one that needs more than 16 bit planes
 * is refused as ever (dev_info[i].error = 1, the others of its batch are coded); RGB pictures with R <= 2047 and gray ones with
 * R <= 4095 never are, all 8-bit pictures among them.  dwtx_encode_bound16 is the safe out_stride for
 * every delta encode, 8-bit ones included.  capacity, the zero padding behind a stream and the encode index keep their meaning.
 * Decode: synchronises where dwtx_decode_view does.  A stream with status 0 that supports the whole picture (host_info[i].level
 * + 1 == levels) is written: with E the inverse transform's output (the missing-plane bias of decode.c:51-58 included), d is E
 * under the signed clamps for [-R, R] — gray and Y to [-R, R], Co and Cg to [-2R, 2R], YCoCg-R inverse, every sample to [-R, R]
 * (R may be 65535) — and the sample written is min(max(B + d, minval), maxval) in dst's type.  A whole stream gives back S
 * exactly; the clamps only act on streams that lost planes, which give an approximation of S.  A stream with status 1 or 2
 * leaves its window untouched, and so does one that supports less than W x H (cut before its finest level: a coarse residual has
 * no base of its size); host_info[i] is the plain call's either way.  Nothing but the `channels` samples of the W x H pixels of a
 * written window is written, and every disjointness rule of dwtx_decode_view_step holds for dst.
 * Base against destination (decode): either the two views are identical — dev, every stride and the step: the decode is in
 * place, each sample read and written by the same lane — or every unit of dst is disjoint from every unit of base, a unit being a
 * window (for planar RGB a plane) and disjoint meaning that the spans [first, first + (H-1)*row_pitch + row) do not intersect.
 * The rule is sufficient, not necessary: it takes odd frames against even frames and a frame against another allocation, and
 * refuses frames 1.. against frames 0.. of one stack — that decode is a chain of n calls, or one dwtx_decode_view_chain (below).
 * Not in this call, left for later: float samples, window lists, flips, crops and levels_max.
 * Route: a delta view takes the deep pictures' route in both directions whatever its sample size (histograms from the entropy
 * stage's own pass, no 16-bit ring planes; DWTX_OPT_NO_PIXELS16 covers it).  Where both views are ones the transform's finest
 * level reads / writes itself (W % 4 == 0, more than 64 pixels on a side, every row of every window on the quad of its samples)
 * and hold dense gray pixels of any of the three sample types, or dense interleaved 8-bit RGB in either order, the finest level
 * loads both views, or adds the base and clamps, itself; every other pair — planar, stepped, 16-bit RGB, off the quad, mixed —
 * goes through the general conversions' delta instances: the same bytes and samples.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): mismatched channels or sample_bytes, sgn with 1-byte samples,
 * minval != 0 without sgn, a range outside the rule, a destination that meets its base, and everything dwtx_encode_view_order /
 * dwtx_decode_view_order refuse for either view. */
int dwtx_encode_view_delta(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step,
	int order, int sgn, int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_delta(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step,
	int order, int sgn, int minval, dwtx_decode_info *host_info);
/* Host arithmetic only, like dwtx_view_list_check: DWTX_OK, or the DWTX_ERR_ARG (and text) the two calls above would return for
 * these two views (dst != 0: the decode's rules, base against destination among them). */
int dwtx_view_delta_check(const dwtx_view *v, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step,
	int sgn, int minval, int W, int H, int n, int dst);

/* ---- delta chains: each picture coded against its predecessor, the first against a key, in one call ------------------------------
 * The CT volume and the clip of the delta views: slice i against slice i - 1.  The encode of such a chain was one call already
 * (frames 1.. against frames 0.. of a stack); the decode was a chain of n delta decodes of one picture each, because picture i's
 * base is picture i - 1 and that is not there yet.  These calls are that chain: the entropy stage, the reconstruction and the
 * inverse transform of the n residuals run as the batch they are, and one kernel walks S_i = clamp(S_{i-1} + d_i) along the chain.
 * Views: `src` / `dst` is a grid view of n windows, exactly as in the delta calls.  `key` describes ONE window, the base of
 * picture 0, and is required: its dev, row_pitch, channel_stride and pixel step are its own (a planar key under an interleaved
 * stack), its cols, image_stride and band_stride are ignored; channels, sample_bytes, sgn and order are shared with the other
 * view, and sgn, minval and the range follow the delta calls' rules.
 * Decode, stated by equivalence: the result — every byte of the destination and of the key, and host_info — is that of n calls
 * of dwtx_decode_view_delta, call i decoding stream i alone into window i with window i - 1 as it lies in memory after call
 * i - 1 as its base, and the key for i == 0.  So the base of picture i is the clamped sample that was written for picture i - 1,
 * not an unclamped running sum; a stream with status 1 or 2, or one that stops before its finest level, leaves its window as it
 * is, and picture i + 1 takes the bytes the caller left in window i as its base; host_info[i] is the plain call's; the call
 * synchronises where dwtx_decode_view does.  n == 1 IS dwtx_decode_view_delta with base = key and takes its path.
 * Disjointness (decode): dst must pass dwtx_decode_view_step's rules, and every unit of dst (a window; for planar RGB a plane) must
 * be disjoint from every unit of the key: their spans [first, first + (H-1)*row_pitch + row) do not intersect, or both have the
 * same row pitch in bytes and lie in different columns of the lattice of rows that pitch apart (a key in a window's pitch gap).
 * Frame 0 of a stack as the key and frames 1.. as the destination is the layout this is made for.
 * Encode: asynchronous.  Stream 0 is window 0 minus the key, stream i window i minus window i - 1; the bytes and dev_info are
 * those of dwtx_encode_view_delta on those pairs — the call is two of them, with the encode index landing at entry i for stream
 * i.  The views are only read and may overlap in any way.
 * Route (decode, n > 1): the deep pictures' route as for every delta view, never the fused sinks: the int32 inverse transform
 * into planes, then per group of the batch one launch of lift.hip's k_chain_from_planes, each lane walking its pixel through
 * the group's pictures in order with the running sample in a register.
 * Not in these calls, for the reasons the delta calls give: float samples, window lists, flips, crops, levels_max and a NULL key.
 * One call is one chain; several chains per call, their keys inside the stack, are the *_view_clips calls below.
 * DWTX_ERR_ARG (with a dwtx_last_error() text, nothing written): a NULL key, mismatched channels or sample_bytes, sgn with 1-byte
 * samples, minval != 0 without sgn, a range outside the rule, a destination that meets the key, and everything
 * dwtx_encode_view_order / dwtx_decode_view_order refuse for either view. */
int dwtx_decode_view_chain(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step,
	int order, int sgn, int minval, dwtx_decode_info *host_info);
int dwtx_encode_view_chain(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step,
	int order, int sgn, int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
/* Host arithmetic only, like dwtx_view_delta_check: DWTX_OK, or the DWTX_ERR_ARG (and text) the two calls above would return for
 * this view and key (dst != 0: the decode's rules, the key against the destination among them). */
int dwtx_view_chain_check(const dwtx_view *v, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step,
	int sgn, int minval, int W, int H, int n, int dst);

/* ---- clips: chains with their keys inside the stack, many per call ------------------------------------------------------------
 * A clip with a key frame every `period` frames, a batch of short clips for a loader, a study of several CT volumes: one stack
 * of n windows in which window i with i % period == 0 is a KEY, coded as itself, and every other window a LINK, coded against
 * window i - 1 of the same stack.  period >= 1; period >= n is one clip with its key at window 0; period == 1 makes every picture
 * a key; the last clip may be short.  With the chain calls each clip costs two calls, a plain one for its key and a chain.
 * Views: `src` / `dst` is ONE grid view of n windows, as in the delta calls, and every layout they take carries over: dense,
 * pitched, stacks and tile grids, planar and stepped pixels, either channel order, uint8_t, uint16_t and, with sgn, int16_t
 * samples, gray and RGB.  sgn, minval and the range follow the delta calls' rules.  There is no second view.
 * Encode: asynchronous, one pass through the pipeline for all n pictures.  Stream i and dev_info[i] of a key are byte for byte
 * those of the plain call on window i — dwtx_encode_view_signed, or dwtx_encode_view_order when sgn == 0, i.e. of the reference's
 * stages (encode.c:155-221) on the picture itself: a key is an ordinary stream that any reader shows.  A link's are those of
 * dwtx_encode_view_delta of window i against window i - 1.  The view is only read.  A picture that needs more than 16 bit planes
 * gets error = 1 and the others of its batch are coded; dwtx_encode_bound16 is the safe stride; capacity, the zero padding behind
 * a stream and the encode index (entry i for stream i) keep their meaning.
 * Decode, stated by equivalence: the result — every byte of the destination's buffer, and host_info — is that of walking i = 0 ..
 * n - 1 in order.  A key: if stream i has status 0 and supports the whole picture (host_info[i].level + 1 == levels), window i
 * receives what the plain decode of stream i alone writes there (dwtx_decode_view_signed / dwtx_decode_view_order:
 * decode.c:174-264 with the missing-plane bias of decode.c:51-58 and their clamps for [minval, maxval]); otherwise the window
 * stays as it is — the one deliberate difference from a plain call: a key cut before its finest level is NOT written into its
 * window's corner, for the call has no levels_max and writes whole pictures only.  A link: dwtx_decode_view_delta of stream i
 * alone into window i with window i - 1 as it lies in memory at that moment as its base; an unreadable link or one cut before its
 * finest level leaves its window as it is, and the next link takes what lies there.  host_info[i] is the plain call's; the call
 * synchronises where dwtx_decode_view does.
 * Disjointness (decode): dwtx_decode_view_step's rules for dst, nothing else.
 * Route (decode): the deep pictures' route as for every delta view, never the fused sinks: the int32 inverse transform into
 * planes, then per group of the batch ONE launch of lift.hip's k_clips_from_planes, which walks the group's segments (a run of
 * windows from a key, or from the group's start, to before the next key) side by side, each lane walking its pixel through a
 * segment's pictures with the running sample in a register.  Encode: the general conversion's clips
 * instance (a key subtracts nothing and loads no base), then the deep pictures' pipeline, once.
 * Not in these calls: float samples, window lists, flips, crops, levels_max, and a key outside the stack (dwtx_*_view_chain).
 * DWTX_ERR_ARG (with a dwtx_last_error() text that starts "clips view:", nothing written): period < 1, a NULL view, sgn with
 * 1-byte samples, minval != 0 without sgn, a range outside the signed calls' rule, and everything dwtx_encode_view_order /
 * dwtx_decode_view_order refuse for the view. */
int dwtx_encode_view_clips(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int period, int order, int sgn,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info);
int dwtx_decode_view_clips(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, int period, int order, int sgn, int minval,
	dwtx_decode_info *host_info);
/* Host arithmetic only, like dwtx_view_chain_check: DWTX_OK, or the DWTX_ERR_ARG (and text) the two calls above would return for
 * this view (dst != 0: the decode's rules). */
int dwtx_view_clips_check(const dwtx_view *v, size_t pixel_step, int period, int sgn, int minval, int W, int H, int n, int dst);

/* ---- clips for loaders: a crop per clip, and float destinations ---------------------------------------------------------------
 * What a video loader does next with a batch of clips — one random crop per clip, then x.float() * scale + bias into fp16 or bf16
 * — inside the decode: dwtx_decode_view_clips with the windows of `dst` crop_w x crop_h and, with fmt, float samples.  W, H are the
 * streams' geometry.  host_origins holds one (x0, y0) per CLIP, ceil(n / period) pairs: clip k is windows [k * period, (k + 1) *
 * period) and every one of them receives the crop_w x crop_h window of its picture that starts there.  Host memory, read before the
 * call returns; NULL: all (0, 0).  One origin per clip is the contract: links with origins of their own would not be a chain.
 * Every rule of dwtx_decode_view_clips holds with the crop's sides — disjointness by dwtx_decode_view_step's rules, row length,
 * alignment, planar and stepped forms, order, sgn, minval and the range.
 * Identity: with fmt == NULL, crop_w == W, crop_h == H and all origins zero the call IS dwtx_decode_view_clips and takes its path.
 * Integer destinations (fmt == NULL), by equivalence: the walk of dwtx_decode_view_clips, word for word, on crop-sized windows.  A
 * key whose stream has status 0 and supports the whole picture receives the crop, at its clip's origin, of what the plain decode of
 * stream i writes (dwtx_decode_view_crop's window of picture i, the clamps for [minval, maxval] included).  A link receives
 * clamp(B + d), d the same crop of the residual under the signed clamps for [-R, R] (dwtx_decode_view_delta) and B window i - 1 of
 * dst as it lies in memory at that moment — both are per pixel, so the crop of the walk is the walk of the crops.  A window whose
 * stream is unreadable or cut before its finest level stays as it is, and the next link takes what lies there.
 * Float destinations (fmt given): dst->sample_bytes matches fmt->type; dst->maxval, sgn and minval give the range as above (sgn ==
 * 0 requires minval == 0).  The value written for colour c is (float)v * scale[c], rounded to fp32, plus bias[c], rounded to fp32,
 * then converted to the type — dwtx_decode_view_float's rounding contract exactly — where v is the clamped integer the integer walk
 * holds for that sample; scale and bias belong to colours, not to memory positions.  A float window cannot serve as a base, so the
 * float walk has ONE deliberate difference: A BREAK ENDS THE CLIP.  The walk keeps a flag per clip: a whole key (status 0, level +
 * 1 == levels) sets it and is written; a key that is not whole clears it, its window untouched; a link is written only if the flag
 * is set and its own stream is readable and whole; otherwise the link clears the flag and its window stays untouched, and so does
 * every later link up to the next key.  The float walk never reads the destination.
 * host_info[i] is the plain call's either way; the call synchronises where dwtx_decode_view does.
 * Route: the deep pictures' route into the int32 pyramid, as for every clip stack; with a crop dwtx_decode_view_crop's windowed
 * inverse (or, by DWTX_OPT_CROP_ROUTE, the whole inverse and a gather) for the pictures of a group, each at its clip's origin, then
 * ONE launch of the clips conversion on crop_w x crop_h planes: k_clips_from_planes, or its float twin k_clips_float_from_planes.
 * A float group that starts mid-clip takes its running integers from a carry picture (int32, context scratch) that the launch
 * before it left; two carry pictures alternate per launch, so that no launch reads the one it writes.
 * Only launches with something live to write are made.
 * Still not in the call: window lists, flips, levels_max, and a key outside the stack.
 * DWTX_ERR_ARG (with a dwtx_last_error() text that starts "clips view:", nothing written): everything dwtx_decode_view_clips
 * refuses; crop_w outside 1..W or crop_h outside 1..H; an origin that leaves the picture; an unknown float type; a sample_bytes
 * that does not match the type; a scale or bias that is not finite. */
int dwtx_decode_view_clips_crop(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, int period, int order, int sgn, int minval,
	const dwtx_float_format *fmt /* NULL: integer samples */, int crop_w, int crop_h,
	const int *host_origins /* [ceil(n / period)][2] or NULL */, dwtx_decode_info *host_info);
/* Host arithmetic only, like dwtx_view_clips_check: DWTX_OK, or the DWTX_ERR_ARG (and text) the call above would return for this
 * destination view, crop and format. */
int dwtx_view_clips_crop_check(const dwtx_view *v, size_t pixel_step, int period, int sgn, int minval, const dwtx_float_format *fmt,
	int W, int H, int n, int crop_w, int crop_h, const int *host_origins);

/* A frame cut into tiles (host arithmetic only; no reference counterpart): the 1 to 4 groups of same-geometry tiles —
 * interior, right column, bottom row, corner, in that order, those that exist — each a cols x rows grid of W x H tiles
 * whose first tile's corner is (x0, y0): one dwtx_encode_view / dwtx_decode_view call per group.  Per axis, with
 * rem = side % tile: rem == 0 gives side / tile tiles; rem >= 8 one more tile of rem; 0 < rem < 8 widens the last tile to
 * tile + rem; side < tile gives one tile of side — every tile side lies in [8, tile + 7].  tile >= 8 and a multiple of 4,
 * frame sides >= 8 (and of any size: only the tiles' sides have to meet DWTX_MAX_SIDE), else DWTX_ERR_ARG.  Returns the
 * number of groups.  A tiled frame is that many ordinary .dwt streams plus the caller's knowledge of the plan. */
typedef struct dwtx_tile_group {
	int x0, y0;
	int W, H;
	int cols, rows;
} dwtx_tile_group;
int dwtx_tile_groups(int frameW, int frameH, int tile, dwtx_tile_group out[4]);

/* The sender's side of the one exchange step between GPUs (the encoded streams of a step travel to one
 * rank; no reference counterpart — the reference writes one file per process): the n streams of a batch, stream i at
 * dev_streams + i*stream_stride with dev_lens[i] bytes (as dwtx_encode_device leaves them), are moved together into ONE
 * contiguous buffer, stream i at byte offset sum over j < i of round8(dev_lens[j]) — so that a step's streams travel as one
 * message per peer instead of one per frame.  dev_offsets (optional, [n + 1]) receives the offsets, [n] = the total; the
 * receiver computes the same offsets from the gathered lengths.  A length beyond the stride is clamped to it; nothing is
 * written beyond out_bytes (size it from the lengths: the sum of the rounded lengths, at most n * stream_stride).  A
 * shorter out_bytes receives the first out_bytes bytes of the message, and dev_offsets[n] still reports the size the
 * whole message needs: the caller detects the cut by comparing the two.  Asynchronous on the context's stream. */
int dwtx_pack_streams(dwtx_ctx *ctx, uint8_t *dev_out, size_t out_bytes, unsigned long long *dev_offsets,
	const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens, int n);

/* Host-buffer wrappers: what encode.c:133-232 / decode.c:136-268 do between
 * read_pnm/write_pnm and the byte sink.  pixels_max < 0 = no PIXELS argument.
 * dwtx_decode_images returns DWTX_ERR_ARG for a bad header and DWTX_ERR_IO when
 * the root image or plane counts cannot be read (both exit code 1 in decode.c); a
 * single stream that claims more than 16 bit planes is DWTX_ERR_ARG too (status 2).
 * dwtx_encode_images: out_stride a multiple of 8; a stream longer than out_stride is
 * DWTX_ERR_CAPACITY, its slot is not written, and neither is anything past
 * out_lens[i] bytes of a slot.  dwtx_decode_images: lens[i] <= stream_stride (a
 * multiple of 8), else DWTX_ERR_ARG; pixels as for dwtx_decode_device (a picture
 * larger than pix_stride is DWTX_ERR_ARG and is not written). */
int dwtx_encode_images(dwtx_ctx *ctx, const uint8_t *host_pix, int W, int H, int C, int n, long capacity,
	uint8_t *host_out, size_t out_stride, size_t *out_lens, dwtx_stats *stats);
int dwtx_decode_images(dwtx_ctx *ctx, const uint8_t *host_streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint8_t *host_pix, size_t pix_stride, int *outW, int *outH, int *outC);
/* Same, and copies the n decoder records to `infos` (may be NULL): what decode.c needs for its
 * stderr diagnostics (bytes.h:101, rle.h:45). */
int dwtx_decode_images_info(dwtx_ctx *ctx, const uint8_t *host_streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint8_t *host_pix, size_t pix_stride, int *outW, int *outH, int *outC, dwtx_decode_info *infos);

/* encode.c:133-232 / decode.c:136-268 between the PNM and the byte sink for deep pixels: dwtx_encode_images /
 * dwtx_decode_images_info with 16-bit samples (pix_stride in samples; `infos` may be NULL).  A picture that needs more
 * than 16 bit planes is DWTX_ERR_ARG ("image %d needs more than 16 bit planes"). */
int dwtx_encode_images16(dwtx_ctx *ctx, const uint16_t *host_pix, int W, int H, int C, int n, long capacity,
	uint8_t *host_out, size_t out_stride, size_t *out_lens, dwtx_stats *stats);
int dwtx_decode_images16(dwtx_ctx *ctx, const uint8_t *host_streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint16_t *host_pix, size_t pix_stride, int maxval, int *outW, int *outH, int *outC, dwtx_decode_info *infos);

/* dwtx_encode_images16 / dwtx_decode_images16 with native-endian int16_t pixels, coded as they are (see dwtx_encode_view_signed
 * for what that means, and for the clamps a decode applies at [minval, maxval], -32768 <= minval < maxval <= 32767, else
 * DWTX_ERR_ARG): the same staging, parts and errors. */
int dwtx_encode_images_s16(dwtx_ctx *ctx, const int16_t *host_pix, int W, int H, int C, int n, long capacity,
	uint8_t *host_out, size_t out_stride, size_t *out_lens, dwtx_stats *stats);
int dwtx_decode_images_s16(dwtx_ctx *ctx, const uint8_t *host_streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, int16_t *host_pix, size_t pix_stride, int minval, int maxval, int *outW, int *outH, int *outC, dwtx_decode_info *infos);

#ifdef __cplusplus
}
#endif
#endif
