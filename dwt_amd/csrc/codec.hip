// codec.hip — whole-image entry points: the device pipelines behind the
// reference's two main()s (encode.c:133-232, decode.c:136-268 minus file I/O),
// for batches of same-geometry images.
#include "dwtx_internal.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

static size_t encode_bound(int bytes_per_sample, int W, int H, int C)
{
	size_t b = (size_t)bytes_per_sample * W * H * C + 4096;
	return (b + 7) / 8 * 8;
}

extern "C" size_t dwtx_encode_bound(int W, int H, int C)
{
	// 8-bit sources: at most 12 bit planes per coefficient (the transform's worst gain is 4.54 for gray and 9.07 for the
	// chroma of YCoCg-R, whose range is twice the pixels': 9.07 * 255 < 2^12; DESIGN.md sections 4.8 and 7), each plane
	// costs a coefficient at most 2 bits (a raw refinement bit, or a pass-1 symbol: VLI(0) at order 0 is one bit, plus
	// the sign) -> 3 bytes per sample; uniform noise measures ~9 bit/sample
	return encode_bound(3, W, H, C);
}

extern "C" size_t dwtx_encode_bound16(int W, int H, int C)
{
	// deep sources: the coder's 16 planes x 2 bits = 4 bytes per sample (a picture that needs more is refused)
	return encode_bound(4, W, H, C);
}

// The pixels a pipeline starts from or ends in travel as a dwtx_pixels view (dwtx_internal.h): the reference's bytes or
// deep pixels, with the channels, the distance between images (in samples) and the maxval the caller names.

// Which ring levels of a W*H transform from / to `px` live in 16-bit planes, and the planes: `own`, or SLOT_CD_F16 of the
// context for n images.  The finest rings of a transform that starts from 8-bit pixels — the finest ring, three quarters
// of all coefficients, cannot leave 11 bits then, and lift.hip bounds how many levels stay below 16 (dwtx_levels16) — when
// the lifting kernels reach the pixels themselves (the planes start / end in those kernels: not for deep pictures), and
// the coder reads / writes their squares in place (sq: the levels whose squares stay in the pyramid; 0: none wanted).
static int rings16(dwtx_ctx *ctx, const dwtx_pixels &px, int W, int H, int n, unsigned sq, int16_t *own, dwtx_p16 *f)
{
	*f = dwtx_p16{ nullptr, 0u };
	unsigned levels;
	if (px.deep() || !sq || !dwtx_pixels_ok(px, W, H) || !(levels = dwtx_levels16(W, H, sq)))
		return DWTX_OK;
	int16_t *planes = own ? own : (int16_t *)dwtx_scratch(ctx, SLOT_CD_F16, sizeof(int16_t) * (size_t)W * H * px.channels * n);
	if (!planes)
		return DWTX_ERR_NOMEM;
	*f = dwtx_p16{ planes, levels };
	return DWTX_OK;
}

// the int32 planes of n images between the general conversions and the general transforms: `tmp`, or SLOT_CD_A
static int32_t *planes_between(dwtx_ctx *ctx, int32_t *tmp, int W, int H, int C, int n)
{
	return tmp ? tmp : (int32_t *)dwtx_scratch(ctx, SLOT_CD_A, sizeof(int32_t) * (size_t)W * H * C * n);
}

// pixels -> pyramid (encode.c:155-159): in one pass where the finest level can read the pixels itself (dwtx_pixels_ok;
// DWTX_OPT_NO_PIXELS16 keeps deep pictures off it), else ingest into planes (`tmp`, or scratch) and the int32 transform.
// Bytes only: the transform leaves the tiles' magnitude histograms behind where it can (*hist_levels; encode.c:112-131's
// maximum and everything the entropy stage counts before it codes: the coefficients are not read a second time for them),
// and the finest rings go to 16-bit planes (*fine16, see rings16: of the levels in sq16, into own16 or scratch).
// (Not for deep pixels: lift.hip's histogram accumulators hold magnitudes below 2^15, a deep picture's coefficients reach
// 2^16 — pack.hip's k_hist counts every level then, as it does for dwtx_encode_planes.)
static int pyramid_from_pixels(dwtx_ctx *ctx, int32_t *pyr, int32_t *tmp, const dwtx_pixels &px, int W, int H, int n, unsigned sq16, int16_t *own16,
	unsigned *hist_levels, dwtx_p16 *fine16)
{
	const int C = px.channels;
	int rc;
	dwtx_hist_sink sink;
	// (deep_source(): deep pixels, and float pixels that quantise beyond 255 — dwtx_encode_view_float — which take their route)
	const dwtx_hist_sink *hist = px.deep_source() ? nullptr : &sink;
	*hist_levels = 0u;
	*fine16 = dwtx_p16{ nullptr, 0u };
	if (hist && (rc = dwtx_hist_begin(ctx, W, H, C, n, &sink)))
		return rc;
	if ((rc = rings16(ctx, px, W, H, n, px.deep_source() ? 0u : sq16, own16, fine16)))
		return rc;
	if (dwtx_pixels_ok(px, W, H) && !(px.deep() && ctx->opt[DWTX_OPT_NO_PIXELS16]))
		return dwtx_fwd_pixels(ctx, pyr, px, W, H, n, hist, hist_levels, *fine16);             // encode.c:155-159 in one pass
	if (!(tmp = planes_between(ctx, tmp, W, H, C, n)))
		return DWTX_ERR_NOMEM;
	if ((rc = dwtx_pixels_to_planes(ctx, tmp, px, W, H, n)))                                   // encode.c:155-156
		return rc;
	return dwtx_transformation_fwd_hist(ctx, pyr, tmp, W, H, n * C, hist, hist_levels);        // encode.c:159
}

// pyramid -> pixels (decode.c:258-264), image i of the n at px.image(i): in one pass where the finest level can write the
// pixels itself (as above; f16: rings the decoder left in 16-bit planes), else the int32 transform into planes (`tmp`, or
// scratch) and egress, which knows the view's strides
static int pixels_from_pyramid(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *pyr, int32_t *tmp, int W, int H, int n, const dwtx_p16 *f16)
{
	const int C = px.channels;
	int rc;
	if (dwtx_pixels_ok(px, W, H) && !(px.deep() && ctx->opt[DWTX_OPT_NO_PIXELS16]))
		return dwtx_inv_pixels(ctx, px, pyr, W, H, n, f16);                                    // decode.c:258-264 in one pass
	if (!(tmp = planes_between(ctx, tmp, W, H, C, n)))
		return DWTX_ERR_NOMEM;
	if ((rc = dwtx_transformation_inv(ctx, tmp, pyr, W, H, n * C)))                            // decode.c:258
		return rc;
	return dwtx_planes_to_pixels(ctx, px, tmp, W, H, n);                                       // decode.c:262-264
}

// pixels (device) -> streams (device) for one part of a batch, on the part's context; `lifted` (optional) is recorded
// once the part's transform and linearisation are queued
static int encode_part(dwtx_ctx *ctx, const dwtx_pixels &px, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info, hipEvent_t lifted, dwtx_index *dev_index)
{
	const int C = px.channels;
	const size_t bytes = sizeof(int) * (size_t)W * H * C * n;
	int *a = (int *)dwtx_scratch(ctx, SLOT_CD_A, bytes);
	int *b = (int *)dwtx_scratch(ctx, SLOT_CD_B, bytes);
	if (!a || !b)
		return DWTX_ERR_NOMEM;
	int rc;
	// encode.c:160: levels that are full power-of-two squares stay in the pyramid (the coder reads their tiles there)
	const unsigned sq = ctx->opt[DWTX_OPT_NO_SQUARE_TILES] ? 0u : dwtx_square_levels(W, H);
	// (the finest rings in 16-bit planes: the transform writes, and the coder reads, half the bytes for them)
	unsigned hist_levels;
	dwtx_p16 fine16;
	if ((rc = pyramid_from_pixels(ctx, b, a, px, W, H, n, ctx->opt[DWTX_OPT_NO_FINE16] ? 0u : sq, nullptr, &hist_levels, &fine16)))
		return rc;
	if ((rc = dwtx_linearization_ex(ctx, a, b, W, H, n * C, sq, fine16)))
		return rc;
	if (lifted)
		DWTX_HIP(hipEventRecord(lifted, ctx->stream));
	return dwtx_encode_planes_ex(ctx, a, b, sq, hist_levels, W, H, C, n, capacity, dev_out, out_stride, dev_info, fine16, dev_index);   // encode.c:163-221
}

// The pipelines' transforms on their own (include/dwtx.h): what encode_part / dwtx_decode_device's `finish` run around the
// entropy stage, with the tiles' histograms riding along in the forward direction as they do there.  The 8-bit calls are
// the fused pass and refuse a shape it does not take; the deep calls take every shape, through a scratch copy of the
// planes (the 16-bit ingest / egress kernel and the int32 transform) where the fused pass does not.
static bool fused_shape(const dwtx_pixels &px, int W, int H)
{
	if (dwtx_pixels_ok(px, W, H))
		return true;
	dwtx_set_error("the pixel transforms need W %% 4 == 0, more than 64 pixels on a side and 4-byte aligned pixels (%dx%d)", W, H);
	return false;
}

extern "C" int dwtx_transformation_fwd_pixels(dwtx_ctx *ctx, int32_t *dev_pyr, int16_t *dev_rings16, unsigned *levels16,
	const uint8_t *dev_pix, int W, int H, int C, int n)
{
	if (!ctx || !dev_pyr || !dev_pix || (C != 1 && C != 3) || n < 1 || (dev_rings16 && !levels16))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	if (levels16)
		*levels16 = 0u;
	const dwtx_pixels px = dwtx_pixels8(dev_pix, C, (size_t)W * H * C);
	if (!fused_shape(px, W, H))
		return DWTX_ERR_ARG;
	unsigned hist_levels;
	dwtx_p16 fine16;
	// (the caller's ring planes, if it brought any: asked for by the call, whatever DWTX_OPT_NO_FINE16 says about the pipelines')
	const int rc = pyramid_from_pixels(ctx, dev_pyr, nullptr, px, W, H, n, dev_rings16 ? dwtx_square_levels(W, H) : 0u, dev_rings16, &hist_levels, &fine16);
	if (levels16)
		*levels16 = fine16.levels;
	return rc;
}

extern "C" int dwtx_transformation_inv_pixels(dwtx_ctx *ctx, uint8_t *dev_pix, const int32_t *dev_pyr, const int16_t *dev_rings16,
	unsigned levels16, int W, int H, int C, int n)
{
	if (!ctx || !dev_pyr || !dev_pix || (C != 1 && C != 3) || n < 1 || (levels16 && !dev_rings16))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	const dwtx_pixels px = dwtx_pixels8(dev_pix, C, (size_t)W * H * C);
	if (!fused_shape(px, W, H))
		return DWTX_ERR_ARG;
	if (levels16 && levels16 != dwtx_levels16(W, H, dwtx_square_levels(W, H))) {   // (the mask the forward call reported for this geometry, or none)
		dwtx_set_error("levels16 mask 0x%x is not the one the forward transform reports for %dx%d (0x%x)", levels16, W, H,
			dwtx_levels16(W, H, dwtx_square_levels(W, H)));
		return DWTX_ERR_ARG;
	}
	const dwtx_p16 f16 = { levels16 ? const_cast<int16_t *>(dev_rings16) : nullptr, levels16 };
	return pixels_from_pyramid(ctx, px, dev_pyr, nullptr, W, H, n, &f16);
}

extern "C" int dwtx_transformation_fwd_pixels16(dwtx_ctx *ctx, int32_t *dev_pyr, const uint16_t *dev_pix, int W, int H, int C, int n)
{
	if (!ctx || !dev_pyr || !dev_pix || (C != 1 && C != 3) || n < 1)
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	unsigned hist_levels;
	dwtx_p16 fine16;
	return pyramid_from_pixels(ctx, dev_pyr, nullptr, dwtx_pixels16(dev_pix, C, (size_t)W * H * C), W, H, n, 0u, nullptr, &hist_levels, &fine16);
}

extern "C" int dwtx_transformation_inv_pixels16(dwtx_ctx *ctx, uint16_t *dev_pix, const int32_t *dev_pyr, int W, int H, int C, int n, int maxval)
{
	if (!ctx || !dev_pyr || !dev_pix || (C != 1 && C != 3) || n < 1 || !dwtx_maxval_ok(maxval))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	return pixels_from_pyramid(ctx, dwtx_pixels16(dev_pix, C, (size_t)W * H * C, maxval), dev_pyr, nullptr, W, H, n, nullptr);
}

// pixels (device) -> streams (device); async on the context's stream.
// The transform is bound by memory, the entropy stage by vector-instruction issue: a batch runs as parts on streams of
// their own, staggered so that part k's transform runs beside part k-1's entropy stage (the transforms follow one
// another: each fills the memory system by itself).  The caller's stream waits for all parts.
// dev_index (device memory, or null): entry i receives the sidecar index of image i (dwtx_ctx_set_encode_index)
static int encode_device(dwtx_ctx *ctx, const dwtx_pixels &px, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info, dwtx_index *dev_index)
{
	const int C = px.channels;
	if (!ctx || !px.base || !dev_out || !dev_info || (C != 1 && C != 3) || n < 1 || !px.sample_aligned())
		return DWTX_ERR_ARG;
	if (!dwtx_count_ok((long)n * C, DWTX_MAX_PLANES_PER_CALL, "planes"))   // (before any scratch is asked for)
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	// (parts pay from about 32 images each: measured at the end of round 3, when the transform no longer waits on memory
	// the way it did — 1024 frames of 1080p RGB 43.2 -> 41.9 ms, 256 frames 11.0 -> 10.9, but 64 frames of 4096x4096 gray
	// 6.57 -> 6.72 and 16 frames 1.98 -> 2.17 the wrong way)
	const int K = ctx->opt[DWTX_OPT_ONE_STREAM] || n < 32 * DWTX_ENC_PARTS ? 1 : DWTX_ENC_PARTS;
	if (K == 1)
		return encode_part(ctx, px, W, H, n, capacity, dev_out, out_stride, dev_info, nullptr, dev_index);
	dwtx_ctx *part[DWTX_ENC_PARTS];
	int rc;
	for (int k = 0; k < K; ++k)
		if ((rc = dwtx_encoder_part(ctx, k, &part[k])))
			return rc;
	hipEvent_t *lifted = ctx->enc_ev.lifted, *done = ctx->enc_ev.done, start = ctx->enc_ev.start;
	DWTX_HIP(hipEventRecord(start, ctx->stream));   // the pixels are the caller's earlier work on its stream
	rc = DWTX_OK;
	int queued = 0;
	for (int k = 0; k < K && !rc; ++k) {
		const int i0 = (int)((long)n * k / K), cnt = (int)((long)n * (k + 1) / K) - i0;
		hipStream_t st = part[k]->stream;
		// (a failure here must not leave the function: parts already queued read the caller's buffers, the join loop below waits for them)
		if (hipStreamWaitEvent(st, start, 0) != hipSuccess || (k && hipStreamWaitEvent(st, lifted[k - 1], 0) != hipSuccess)) {
			dwtx_set_error("%s:%d hipStreamWaitEvent failed for encoder part %d", __FILE__, __LINE__, k);
			rc = DWTX_ERR_DEVICE;
			break;
		}
		rc = encode_part(part[k], px.image(i0), W, H, cnt, capacity, dev_out + out_stride * (size_t)i0, out_stride,
			dev_info + i0, lifted[k], dev_index ? dev_index + i0 : nullptr);
		if (hipEventRecord(done[k], st) != hipSuccess && !rc)
			rc = DWTX_ERR_DEVICE;
		queued = k + 1;
	}
	for (int k = 0; k < queued; ++k)   // (also after a failure: what was queued reads the caller's buffers)
		if (hipStreamWaitEvent(ctx->stream, done[k], 0) != hipSuccess && !rc)
			rc = DWTX_ERR_DEVICE;
	return rc;
}

extern "C" int dwtx_encode_device(dwtx_ctx *ctx, const uint8_t *dev_pix, int W, int H, int C, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	return encode_device(ctx, dwtx_pixels8(dev_pix, C, (size_t)W * H * C), W, H, n, capacity, dev_out, out_stride, dev_info, ctx ? ctx->enc_index : nullptr);
}

extern "C" int dwtx_encode_device16(dwtx_ctx *ctx, const uint16_t *dev_pix, int W, int H, int C, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	return encode_device(ctx, dwtx_pixels16(dev_pix, C, (size_t)W * H * C), W, H, n, capacity, dev_out, out_stride, dev_info, ctx ? ctx->enc_index : nullptr);
}

// dwtx_decode_view_crop: the windows of px are w x h, picture i's crop starts at origins[2 * i], origins[2 * i + 1] (host
// memory; null: all at (0, 0)); checked by the caller
struct CropCall {
	int w, h;
	const int *origins;
};

// streams (device) -> pixels (device).  Image i is written at px.image(i) — densely (ow*oh*C samples), or with the view's
// row pitch into its window's corner; its size is widths/heights[info[i].level + 1].
// crop (optional): only that window of every picture is written, into the view's windows of its size.  The entropy stage,
// the reconstruction and the host's part / finish logic are the plain call's, with every ring in the int32 pyramid; then
// dwtx_inv_crop and the general conversion take the place of pixels_from_pyramid.
static int decode_device(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max, const dwtx_pixels &px, dwtx_decode_info *host_info,
	const CropCall *crop = nullptr)
{
	const int C = px.channels;
	if (!ctx || !dev_streams || !dev_lens || !px.base || !host_info || n < 1 || !px.sample_aligned())
		return DWTX_ERR_ARG;
	if (!px.range_ok() || !dwtx_count_ok(n, DWTX_MAX_PLANES_PER_CALL / 3, "streams to decode"))   // (before any scratch is asked for)
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	dwtx_geom g;
	int rc = dwtx_geometry(&g, W, H);
	if (rc)
		return rc;
	const size_t bytes = sizeof(int) * (size_t)W * H * C * n;
	int *a = (int *)dwtx_scratch(ctx, SLOT_CD_A, bytes);
	int *b = (int *)dwtx_scratch(ctx, SLOT_CD_B, bytes);
	if (!a || !b)
		return DWTX_ERR_NOMEM;
	const size_t plane_ints = (size_t)W * H;
	// 16-bit planes for the finest rings of whole pictures (rings16; the decoder checks the streams' plane counts):
	// every ring the 16-byte-per-lane inverse kernels take: what a stream holds is bounded by its plane counts on
	// every level; the LL bands between the levels are sums of those and stay int32
	dwtx_p16 fine16;
	const unsigned sq = ctx->opt[DWTX_OPT_NO_SQUARE_TILES] ? 0u : dwtx_square_levels(W, H);
	if ((rc = rings16(ctx, px, W, H, n, ctx->opt[DWTX_OPT_NO_FINE16] || crop ? 0u : sq, nullptr, &fine16)))
		return rc;
	// A crop's rectangles, for the pictures that come out whole: where picture i's rectangle of plane t starts, [t][i] (x, y),
	// rows 0 .. tail_from (dwtx_inv_crop).  One small copy that is over before the walk begins — the call synchronises anyway,
	// and the host table does not outlive this block.  (On the context's stream: an earlier call's kernels may still read the slot.)
	long route = 0;
	int *crop_tab = nullptr;
	if (crop) {
		route = ctx->opt[DWTX_OPT_CROP_ROUTE];
		if (route < 0 || route > 2) {
			dwtx_set_error("DWTX_OPT_CROP_ROUTE is %ld: it takes 0 (automatic), 1 (windowed levels) or 2 (whole inverse, then a gather)", route);
			return DWTX_ERR_ARG;
		}
		// (automatic: the windowed levels for every crop but the whole picture, which never comes here — no crop size has
		// been measured slower than decode-then-slice yet)
		if (!route)
			route = 1;
		dwtx_crop_steps S;
		if ((rc = dwtx_crop_steps_of(W, H, crop->w, crop->h, &S)))
			return rc;
		const size_t rows = (size_t)S.tail_from + 1, tab_bytes = sizeof(int) * 2 * rows * (size_t)n;
		crop_tab = (int *)dwtx_scratch(ctx, SLOT_CD_CROP, tab_bytes);
		int *host_tab = (int *)malloc(tab_bytes);
		if (!crop_tab || !host_tab) {
			free(host_tab);
			return DWTX_ERR_NOMEM;
		}
		for (int i = 0; i < n; ++i) {
			int xs[DWTX_MAX_LEVELS + 2], ys[DWTX_MAX_LEVELS + 2];
			dwtx_crop_origins(S, crop->origins ? crop->origins[2 * i] : 0, crop->origins ? crop->origins[2 * i + 1] : 0, xs, ys);
			for (size_t t = 0; t < rows; ++t) {
				host_tab[2 * (t * (size_t)n + i)] = xs[t];
				host_tab[2 * (t * (size_t)n + i) + 1] = ys[t];
			}
		}
		hipError_t e = hipMemcpyAsync(crop_tab, host_tab, tab_bytes, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess)
			e = hipStreamSynchronize(ctx->stream);
		free(host_tab);
		if (e != hipSuccess) {
			dwtx_set_error("crop origins -> %s", hipGetErrorString(e));
			return DWTX_ERR_DEVICE;
		}
	}
	// scratch both parts of the batch will ask for, sized once for the larger request (a slot that grows waits for the
	// stream: `finish` must not grow one in the middle of the pipeline)
	if (!dwtx_scratch(ctx, SLOT_CD_INFO, sizeof(int) * 48 * (size_t)n))
		return DWTX_ERR_NOMEM;
	if ((rc = dwtx_lift_scratch(ctx, W, H, (n < 4 ? n : n - n / 2) * C)))
		return rc;
	// A clip stack of float windows (dwtx_decode_view_clips_crop with a format): the walk's running INTEGERS cannot be read back
	// from the view, so a clip that crosses a group — a decoder part, or the one-window launches of `part`'s fallback — hands them
	// on in a carry picture: int32, C planes of the windows' size.  TWO of them, sized here once like the slots above.  A launch
	// reads the one the launch before it wrote (its first segment, where that starts mid-clip on a live clip) and writes the
	// OTHER one (its last segment, where that ends mid-clip): with three segments or more both happen in one launch, in
	// different workgroups, and one picture would be a read/write race between them.  With two, the only launch that still reads
	// the picture launch k writes is launch k + 1, behind it on ctx->stream; launch k + 1 writes the picture launch k read, whose
	// readers are all in launch k — ahead of it on the same stream.  A carry is read only where `live` says
	// that the launch before left one: never before it is written within a call, and nothing of it outlives the call.
	struct {
		int32_t *carry[2] = { nullptr, nullptr };
		int last = 0;        // the carry picture the latest launch wrote
		int seen = 0;        // the windows before this one are decided: written, or left as they are
		bool live = false;   // window seen - 1 was written and its clip goes on: a link at `seen` has a running sample
	} walk;
	if (px.clips && px.is_float()) {
		const size_t one = dwtx_align_up(sizeof(int32_t) * (size_t)(crop ? crop->w : W) * (size_t)(crop ? crop->h : H) * C, 256);
		char *slot = (char *)dwtx_scratch(ctx, SLOT_CD_CARRY, 2 * one);
		if (!slot)
			return DWTX_ERR_NOMEM;
		walk.carry[0] = (int32_t *)slot;
		walk.carry[1] = (int32_t *)(slot + one);
	}
	// The float walk's break rule (include/dwtx.h) for the group [*first, *first + *count), every window of which is readable and
	// whole; `finish` and `part` come in ascending order, so a window below *first that no call of this has seen was not written
	// and broke its clip.  A first segment that starts mid-clip on a dead clip is dropped: the group starts at its first key.
	// -> whether anything is left to launch; *in / *out: the carry pictures that launch reads and writes, or null.
	auto float_run = [&](int *first, int *count, const int32_t **in, int32_t **out) -> bool {
		const int period = px.clips, end = *first + *count;
		if (walk.seen < *first)
			walk.live = false;
		walk.seen = end;
		const int phase = *first % period, lead = phase ? period - phase : 0;
		if (lead && !walk.live) {
			const int skip = lead < *count ? lead : *count;
			*first += skip;
			*count -= skip;
		} else if (lead)
			*in = walk.carry[walk.last];
		if (*count < 1)
			return false;   // (live stays false: the clip is dead up to the next key)
		if (end < n && end % period != 0) {
			walk.last ^= 1;
			*out = walk.carry[walk.last];
		}
		walk.live = true;
		return true;
	};
	// reconstruction -> inverse transform -> pixels for images [first, first+count), queued on ctx->stream
	auto finish = [&](int first, int count, unsigned fused) -> int {
		const dwtx_decode_info &I = host_info[first];
		const int lo = I.level + 1;                                          // decode.c:251
		const int ow = g.widths[lo], oh = g.heights[lo];
		if (px.is_delta() && lo != g.levels)   // (a delta view: a coarse residual has no base of its size — the group's windows stay as they are)
			return DWTX_OK;
		if (!px.row_pitch && (size_t)ow * oh * C > px.image_stride)   // (dense slots; a window with a pitch holds its own corner)
			return DWTX_ERR_ARG;
		int *miss = nullptr;
		bool biased = false;
		for (int k = 0; k < 48; ++k)
			biased = biased || I.missing[k] >= 2;
		if (biased) {
			miss = (int *)dwtx_scratch(ctx, SLOT_CD_INFO, sizeof(int) * 48 * (size_t)n) + 48 * (size_t)first;
			for (int i = 0; i < count; ++i) {
				int r = (int)hipMemcpyAsync(miss + 48 * i, host_info[first + i].missing, sizeof(int) * 48,
					hipMemcpyHostToDevice, ctx->stream);
				if (r)
					return DWTX_ERR_DEVICE;
			}
		}
		int *lin = a + plane_ints * C * first;
		int *pyr = b + plane_ints * C * first;
		// A reduced pyramid (pitch ow) may go through the wide inverse kernels where the whole picture does not: 263x135 at
		// 132x68.  They read it 8 and 16 bytes at a time, and image `first` of odd-sized pictures starts on an odd int: the
		// reduced planes, little more than a quarter of the slot, start on the next 16 bytes instead.
		if (lo < g.levels)
			pyr += (4 - ((size_t)(pyr - b) & 3)) & 3;
		int *img = a + plane_ints * C * first;   // lin is dead once reconstructed
		dwtx_p16 f16 = { nullptr, 0u };
		if (fused & DWTX_FUSED_FINE16) {   // the decoder put the part's finest rings there
			f16.planes = fine16.planes + plane_ints * C * first;
			f16.levels = fine16.levels;
		}
		fused &= ~DWTX_FUSED_FINE16;
		if (const int r = dwtx_reconstruction_ex(ctx, pyr, lin, miss, lo, W, H, C, count, fused, f16))    // decode.c:257 (the rest of it)
			return r;
		if (px.chain) {
			// A chain (dwtx_decode_view_chain): the group's residuals through the int32 transform into planes, never the fused sinks,
			// then one launch that walks windows first .. first + count in order from window first - 1 as it lies in memory (first
			// == 0: the key).  That window is in memory when the launch runs: dwtx_decode_planes_ex calls `part` for the parts in
			// ascending order (unpack.hip, run()), the non-uniform fallback of `part` calls finish(i, 1) in ascending order, and
			// everything either queues goes onto ctx->stream — so every launch that writes a window before `first` is ahead of this
			// one on one stream.  A window no launch writes (status 1 or 2, cut before its finest level) needs no table: the next
			// group reads the bytes the caller left there.
			if (const int r = dwtx_transformation_inv(ctx, img, pyr, W, H, count * C))                   // decode.c:258
				return r;
			return dwtx_planes_to_pixels_chain(ctx, px, img, W, H, first, count);
		}
		if (px.clips) {
			// A clip stack (dwtx_decode_view_clips): the chain's route and the chain's ordering argument, word for word — the group's
			// pictures (a key's own, a link's residual) through the int32 transform into planes, then ONE launch for windows first ..
			// first + count that walks the group's segments side by side.  Only a first segment that starts mid-clip reads a window of
			// another group, window first - 1, and every launch that writes it is ahead of this one on ctx->stream.  A group that
			// stops before its finest level has returned above, its keys included: the call writes whole pictures only.
			// With a crop (dwtx_decode_view_clips_crop) the walk is per pixel, so the crop of a clip is the walk over the same crop of its
			// key and of every residual: dwtx_inv_crop for the group's pictures, each at its CLIP's origin, then the same one launch on
			// crop-sized planes.  Float windows cannot serve as a base: float_run says which windows of the group a launch writes
			// and where its running integers come from and go to (the carry pictures, below).
			int at = first, run = count;
			const int32_t *carry_in = nullptr;
			int32_t *carry_out = nullptr;
			if (px.is_float() && !float_run(&at, &run, &carry_in, &carry_out))
				return DWTX_OK;
			const int32_t *planes = img;
			if (crop) {
				if (const int r = dwtx_inv_crop(ctx, img, pyr, W, H, count, C, crop->w, crop->h, crop_tab + 2 * (size_t)first, n, 0, 0, (int)route, &planes))
					return r;
			} else if (const int r = dwtx_transformation_inv(ctx, img, pyr, W, H, count * C))            // decode.c:258
				return r;
			const int pw = crop ? crop->w : W, ph = crop ? crop->h : H;
			if (!px.is_float())
				return dwtx_planes_to_pixels_clips(ctx, px, planes, pw, ph, first, count);
			return dwtx_planes_to_pixels_clips_float(ctx, px, planes + (size_t)pw * ph * C * (size_t)(at - first), pw, ph, at, run, carry_in, carry_out);
		}
		if (crop) {
			const int32_t *planes;
			if (lo == g.levels) {   // whole pictures: one launch per level for all of them, each with its own origin
				if (const int r = dwtx_inv_crop(ctx, img, pyr, W, H, count, C, crop->w, crop->h, crop_tab + 2 * (size_t)first, n, 0, 0, (int)route, &planes))
					return r;
				return dwtx_planes_to_pixels(ctx, px.image(first), planes, crop->w, crop->h, count);
			}
			// reduced pictures one by one: what of the crop lies inside ow x oh, if anything
			for (int i = 0; i < count; ++i) {
				const int x0 = crop->origins ? crop->origins[2 * (first + i)] : 0, y0 = crop->origins ? crop->origins[2 * (first + i) + 1] : 0;
				const int cw = (x0 + crop->w < ow ? x0 + crop->w : ow) - x0, ch = (y0 + crop->h < oh ? y0 + crop->h : oh) - y0;
				if (cw < 1 || ch < 1)
					continue;
				const size_t at = (size_t)ow * oh * C * i;
				if (const int r = dwtx_inv_crop(ctx, img + at, pyr + at, ow, oh, 1, C, cw, ch, nullptr, 0, x0, y0, (int)route, &planes))
					return r;
				if (const int r = dwtx_planes_to_pixels(ctx, px.image(first + i), planes, cw, ch, 1))
					return r;
			}
			return DWTX_OK;
		}
		return pixels_from_pyramid(ctx, px.image(first), pyr, img, ow, oh, count, &f16);          // decode.c:258-264
	};
	// called by the decoder for each part of the batch as soon as its coefficients are on their way
	auto part = [&](int first, int count, unsigned fused) -> int {
		bool uniform = true;
		for (int i = first; i < first + count; ++i)
			uniform = uniform && !host_info[i].status && host_info[i].level == host_info[first].level &&
				memcmp(host_info[i].missing, host_info[first].missing, sizeof(host_info[first].missing)) == 0;
		if (uniform)
			return finish(first, count, fused);
		for (int i = first; i < first + count; ++i) {   // (a fused part's images all come out whole; their square levels are in the pyramid already)
			int r;
			if (!host_info[i].status && (r = finish(i, 1, fused)))
				return r;
		}
		return DWTX_OK;
	};
	using Part = decltype(part);
	return dwtx_decode_planes_ex(ctx, a, b, dev_streams, stream_stride, dev_lens, W, H, C, n, levels_max, host_info,
		[](void *user, int first, int count, unsigned fused) { return (*(Part *)user)(first, count, fused); }, &part, fine16);
}

extern "C" int dwtx_decode_device(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max,
	uint8_t *dev_pix, size_t pix_stride, dwtx_decode_info *host_info)
{
	return decode_device(ctx, dev_streams, stream_stride, dev_lens, W, H, n, levels_max, dwtx_pixels8(dev_pix, C, pix_stride), host_info);
}

extern "C" int dwtx_decode_device16(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max,
	uint16_t *dev_pix, size_t pix_stride, int maxval, dwtx_decode_info *host_info)
{
	return decode_device(ctx, dev_streams, stream_stride, dev_lens, W, H, n, levels_max, dwtx_pixels16(dev_pix, C, pix_stride, maxval), host_info);
}

// ---- views (include/dwtx.h): windows and tile grids of a larger frame ----------------------------------------------

// Everything a view entry point can say, each field's default its neutral value: an extern "C" entry names the fields its ABI
// has and calls encode_views / decode_views, which resolve the call with plan_view.
enum { PAIR_NONE = 0, PAIR_DELTA, PAIR_CHAIN, PAIR_CLIPS };
struct ViewCall {
	const dwtx_view *view = nullptr;
	size_t pixel_step = 0;                       // samples from a pixel to the next one of its row; 0 and `channels` are both the dense case
	int order = DWTX_ORDER_RGB;                  // kept for RGB views and checked first, nothing else on the host looks at it
	const dwtx_float_format *fmt = nullptr;      // null: integer samples
	const void *const *windows = nullptr;        // [n] device pointers in host memory; null: the view's own grid
	int flip = 0;                                // DWTX_FLIP_* flags for all windows, or
	const unsigned char *host_flips = nullptr;   // one mask per window
	const int *minval = nullptr;                 // the *_view_signed calls' lower bound (a pair call's: what `sgn` makes of it); null: the unsigned call
	bool crop = false;                           // a decode writes a crop_w x crop_h window of each picture, picture i's from host_origins[2 * i], [2 * i + 1]
	int crop_w = 0, crop_h = 0;
	const int *host_origins = nullptr;           // (host memory; null: all at (0, 0))
	int levels_max = -1;                         // a decode's
	int pair = PAIR_NONE;                        // a delta or chain call: `other` is the base view / the key, with its own step
	const dwtx_view *other = nullptr;
	size_t other_step = 0;
	int sgn = 0;
	int period = 0;                              // a clips call (PAIR_CLIPS, no `other`): every period-th window of the view is a key
	bool clip_crop = false;                      // dwtx_decode_view_clips_crop: host_origins holds one pair per CLIP, fmt is optional, and the crop's and the
	                                             // format's refusals are the clips call's own (clips_crop_refusals), worded as its
	int W = 0, H = 0, n = 0;                     // the pictures' size and number
	bool dst = false;                            // the view will be written (maxval, disjoint windows)
	// what single entries insist on: the float calls on a format, the list calls on a list
	bool needs_fmt = false, needs_windows = false;
	// the host-only exports: a view of 4-byte samples is one of fp32 samples (fp16 and bf16 views are addressed, and checked, like
	// 16-bit integers); windows with sides from 1 up; the table of windows is built whatever the flags (dwtx_view_flip_plan reads it)
	bool kind_from_bytes = false, thin = false, table = false;

	int win_w() const { return crop ? crop_w : W; }   // the windows' sides
	int win_h() const { return crop ? crop_h : H; }
};

// dwtx_view -> dwtx_pixels for c.n windows of win_w() x win_h(), checked; the call as plan_view has normalised it.
// kind: the float samples the view must hold — its sample_bytes their size, any maxval a deep picture may have; every stride counts
// those samples, and every rule below holds as it stands — or -1 for integer samples.
// Listed windows (c.windows): the view's dev, cols, image_stride and band_stride are not looked at, every other check is the
// grid's, and list_windows (the caller's next step) takes the place of the rules about where the windows lie.
// c.minval: integer samples are int16_t (sample_bytes 2, nothing else), coded as they are, and a destination's range is [*minval,
// maxval] (dwtx_range_ok); float samples get that range as their lower bound too.
static int view_pixels(const ViewCall &c, int kind, dwtx_pixels *px)
{
	const dwtx_view *v = c.view;
	const int W = c.win_w(), H = c.win_h(), n = c.n;
	const bool dst = c.dst, list = c.windows || c.needs_windows, sgn = c.minval != nullptr;
	// whose view it is, in front of every text: a clips call's refusals all start "clips view:" (include/dwtx.h), also those that
	// the other calls word without a prefix (`bare`)
	const bool clips = c.pair == PAIR_CLIPS;
	const char *who = clips ? "clips view" : "view", *bare = clips ? "clips view: " : "";
	if (c.order != DWTX_ORDER_RGB && c.order != DWTX_ORDER_BGR) {
		dwtx_set_error("%s: channel order %d (DWTX_ORDER_RGB = 0 or DWTX_ORDER_BGR = 1)", who, c.order);
		return DWTX_ERR_ARG;
	}
	if (list && !c.windows) {
		dwtx_set_error("view list: no list of windows (the grid calls take a view without one)");
		return DWTX_ERR_ARG;
	}
	if (!v || (!list && !v->dev) || n < 1) {
		dwtx_set_error("%sno view, no pixels or no windows", bare);
		return DWTX_ERR_ARG;
	}
	if (clips && !c.crop && !dwtx_dims_ok(W, H)) {   // (a clip stack's crop: clips_crop_refusals has seen the pictures' own size)
		dwtx_set_error("clips view: unsupported image size %dx%d (8..%d per side)", W, H, DWTX_MAX_SIDE);
		return DWTX_ERR_ARG;
	}
	if (!c.crop && !c.thin)
		DWTX_CHECK_DIMS(W, H);
	else if (W < 1 || H < 1 || W > DWTX_MAX_SIDE || H > DWTX_MAX_SIDE)   // (a crop of a picture that crop_of_call has checked)
		return DWTX_ERR_ARG;
	if (kind >= 0 && v->sample_bytes != (kind == DWTX_SAMPLE_F32 ? 4 : 2)) {
		dwtx_set_error("%s: sample_bytes %d does not match the float type (%d bytes a sample)", who, v->sample_bytes, kind == DWTX_SAMPLE_F32 ? 4 : 2);
		return DWTX_ERR_ARG;
	}
	if ((kind < 0 && v->sample_bytes != 1 && v->sample_bytes != 2) || (v->channels != 1 && v->channels != 3) || (!list && v->cols < 0)) {
		dwtx_set_error("%s: sample_bytes %d (1 or 2), channels %d (1 or 3), cols %d (>= 0)", who, v->sample_bytes, v->channels, v->cols);
		return DWTX_ERR_ARG;
	}
	if (sgn && kind < 0 && v->sample_bytes != 2) {
		dwtx_set_error("%s: signed integer samples are int16_t: sample_bytes %d (2)", who, v->sample_bytes);
		return DWTX_ERR_ARG;
	}
	const size_t cs = v->channels == 3 ? v->channel_stride : 0;   // planar RGB; a gray view has no use for it
	const size_t step = c.pixel_step == (size_t)v->channels ? 0 : c.pixel_step;   // (the dense case: everything downstream is the plain call's)
	if (step && (step < (size_t)v->channels || step > 0x7fffffffu)) {
		dwtx_set_error("%s: pixel_step %zu is less than the %d channels of a pixel (or beyond 2^31)", who, c.pixel_step, v->channels);
		return DWTX_ERR_ARG;
	}
	if (step && cs) {
		dwtx_set_error("%s: pixel_step %zu with planar pixels (channel_stride %zu): the rows of a plane are dense", who, c.pixel_step, cs);
		return DWTX_ERR_ARG;
	}
	const size_t image_stride = list ? 0 : v->image_stride;
	*px = kind >= 0            ? dwtx_pixels_float(v->dev, kind, v->channels, image_stride, v->maxval)
		: sgn                  ? dwtx_pixels_s16((const int16_t *)v->dev, v->channels, image_stride, dst ? *c.minval : -32768, dst ? v->maxval : 32767)
		: v->sample_bytes == 1 ? dwtx_pixels8((const uint8_t *)v->dev, v->channels, image_stride)
		                       : dwtx_pixels16((const uint16_t *)v->dev, v->channels, image_stride, dst ? v->maxval : 65535);
	if (sgn && kind >= 0)
		px->minval = *c.minval;
	px->row_pitch = v->row_pitch;
	px->channel_stride = cs;
	px->pixel_step = step;
	px->order = v->channels == 3 ? c.order : DWTX_ORDER_RGB;
	const size_t row = px->row_samples(W);
	if (v->row_pitch < row) {
		dwtx_set_error("%s: row_pitch %zu is less than a window's row of %zu samples", who, v->row_pitch, row);
		return DWTX_ERR_ARG;
	}
	if (!list && (uintptr_t)v->dev % (size_t)v->sample_bytes) {
		dwtx_set_error("%s: dev is not aligned to its %d-byte samples", who, v->sample_bytes);
		return DWTX_ERR_ARG;
	}
	const size_t cols = list ? (size_t)n : v->cols && v->cols < n ? (size_t)v->cols : (size_t)n;
	const bool bands = cols < (size_t)n;
	if (dst && sgn) {
		if (!dwtx_range_ok(*c.minval, v->maxval, bare))
			return DWTX_ERR_ARG;
	} else if (dst && (v->sample_bytes == 1 ? v->maxval != 255 : !dwtx_maxval_ok(v->maxval, bare))) {
		if (v->sample_bytes == 1)
			dwtx_set_error("%s: maxval %d with 1-byte samples (255)", who, v->maxval);
		return DWTX_ERR_ARG;
	}
	if (dst && !list) {
		const size_t window = (size_t)(H - 1) * v->row_pitch + row;   // from a window's (a plane's) first sample to behind its last
		const bool stacked = v->image_stride >= window;
		const bool beside = v->image_stride >= row && v->row_pitch >= (cols - 1) * v->image_stride + row;
		// planar, first form: a window holds its three planes (an NCHW stack): the windows are then 2 * cs + window long
		const size_t win3 = 2 * cs + window;
		const bool inside = cs >= window && (cols == 1 || v->image_stride >= win3) && (!bands || v->band_stride >= (cols - 1) * v->image_stride + win3);
		if (cs && inside)
			;   // (disjoint as they are)
		else if (cols > 1 && !stacked && !beside) {
			dwtx_set_error("%s: windows overlap (image_stride %zu, row_pitch %zu, %zu windows per band of %zu x %d samples)", who,
				v->image_stride, v->row_pitch, cols, row, H);
			return DWTX_ERR_ARG;
		} else if (bands && v->band_stride < (cols - 1) * v->image_stride + window) {
			dwtx_set_error("%s: bands overlap (band_stride %zu, a band spans %zu samples)", who, v->band_stride, (cols - 1) * v->image_stride + window);
			return DWTX_ERR_ARG;
		} else if (cs) {
			// planar, second form: the channel planes of the whole view apart (a CHW frame and its tiles, CNHW)
			const size_t nbands = ((size_t)n + cols - 1) / cols;
			const size_t span = (nbands - 1) * (bands ? v->band_stride : 0) + (cols - 1) * v->image_stride + window;
			if (cs < span) {
				dwtx_set_error("%s: planes overlap (channel_stride %zu: neither at least a window's plane of %zu samples with windows of %zu apart, "
					"nor at least one channel of the whole view, %zu samples)", who, cs, window, win3, span);
				return DWTX_ERR_ARG;
			}
		}
	}
	if (bands) {
		px->cols = (int)cols;
		px->band_stride = v->band_stride;
	}
	return DWTX_OK;
}

// The planes of a call that walks a table of windows, listed or flipped: refused before the table is built
static bool table_count_ok(const ViewCall &c, int channels)
{
	return c.dst ? dwtx_count_ok(c.n, DWTX_MAX_PLANES_PER_CALL / 3, "streams to decode") : dwtx_count_ok((long)c.n * channels, DWTX_MAX_PLANES_PER_CALL, "planes");
}

// The lattice rule for two units whose rows lie `pitch` apart: unit A covers the columns [0, row_a) of the lattice that starts at
// its first sample, unit B, which starts in column dx of it, the columns [dx, dx + row_b).  Disjoint columns: disjoint units.
static bool other_columns(unsigned long long dx, unsigned long long row_a, unsigned long long row_b, unsigned long long pitch)
{
	return dx >= row_a && dx + row_b <= pitch;
}

// What a listed view adds to view_pixels (include/dwtx.h, the *_view_list calls): every pointer given and on its sample;
// px->base the lowest of them and *offs the windows' offsets from it, in samples; whether all of them are on the wide kernels'
// quad; and, for a destination, that the units — the n windows, or the 3n planes of planar RGB — are provably disjoint.
// Two units whose first samples lie d apart are disjoint if d >= span (one ends before the other begins), or by the lattice rule
// with dx = d % pitch.  Sorted by address, only the units that begin inside a unit's span have to be held against it: a frame of
// tiles costs each tile the tiles of its own band.  px->offs is not set yet: send_list brings the table to the device.
static int list_windows(const ViewCall &c, std::vector<long long> *offs, dwtx_pixels *px)
{
	const int n = c.n;
	const size_t cs = px->channel_stride, row = px->row_samples(c.win_w());
	const uintptr_t sb = (uintptr_t)px->sample_bytes;
	uintptr_t lowest = ~(uintptr_t)0;
	bool quad = true;
	for (int i = 0; i < n; ++i) {
		const uintptr_t p = (uintptr_t)c.windows[i];
		if (!p) {
			dwtx_set_error("view list: window %d of %d is NULL", i, n);
			return DWTX_ERR_ARG;
		}
		if (p % sb) {
			dwtx_set_error("view list: window %d (%p) is not aligned to its %d-byte samples", i, c.windows[i], px->sample_bytes);
			return DWTX_ERR_ARG;
		}
		quad = quad && p % (4 * sb) == 0;
		lowest = p < lowest ? p : lowest;
	}
	struct Unit {
		unsigned long long at;
		int window;
	};
	std::vector<Unit> units;
	try {
		offs->resize((size_t)n);
		if (c.dst)
			units.reserve((size_t)n * (cs ? 3 : 1));
	} catch (...) {
		return DWTX_ERR_NOMEM;
	}
	for (int i = 0; i < n; ++i)
		(*offs)[(size_t)i] = (long long)(((uintptr_t)c.windows[i] - lowest) / sb);
	if (c.dst) {
		const unsigned long long pitch = px->row_pitch, span = (unsigned long long)(c.win_h() - 1) * pitch + row;
		for (int i = 0; i < n; ++i)
			for (int ch = 0; ch < (cs ? 3 : 1); ++ch)
				units.push_back(Unit{ (unsigned long long)(*offs)[(size_t)i] + (unsigned long long)ch * cs, i });
		std::sort(units.begin(), units.end(), [](const Unit &a, const Unit &b) { return a.at < b.at; });
		for (size_t i = 0; i < units.size(); ++i)
			for (size_t j = i + 1; j < units.size() && units[j].at - units[i].at < span; ++j) {
				const unsigned long long d = units[j].at - units[i].at, dx = d % pitch;
				if (other_columns(dx, row, row, pitch))
					continue;
				dwtx_set_error("view list: windows %d and %d are not provably disjoint (%s %llu samples apart: less than the %llu a %s spans, "
					"and column %llu of a pitch of %llu leaves no room for two rows of %zu)", units[i].window, units[j].window,
					cs ? "two of their planes lie" : "they lie", d, span, cs ? "plane" : "window", dx, pitch, row);
				return DWTX_ERR_ARG;
			}
	}
	px->base = (void *)lowest;
	px->offs_on_quad = quad;
	return DWTX_OK;
}

// The table's way to the device: into the context's page-locked buffer — the caller's array and `offs` may go as soon as the
// call returns — and from there into SLOT_CD_LIST by an asynchronous copy on the context's stream, in order with the kernels of an
// earlier listed call that still read the slot and ahead of this call's.  The host waits only for list_sent, the earlier listed
// call's own copy; a slot or a buffer that has to grow waits for more, as every scratch slot does.  Sets px->offs.
static int send_list(dwtx_ctx *ctx, const std::vector<long long> &offs, dwtx_pixels *px)
{
	DWTX_ENTER(ctx);
	const size_t n = offs.size(), bytes = sizeof(long long) * n;
	if (!ctx->have_list_sent) {
		DWTX_HIP(hipEventCreateWithFlags(&ctx->list_sent, hipEventDisableTiming));
		ctx->have_list_sent = true;
	}
	DWTX_HIP(hipEventSynchronize(ctx->list_sent));   // (an event that was never recorded counts as reached)
	if (ctx->list_cap < n) {
		if (ctx->list_host)
			(void)hipHostFree(ctx->list_host);
		ctx->list_host = nullptr;
		ctx->list_cap = 0;
		const size_t want = n + n / 8 + 64;
		DWTX_HIP(hipHostMalloc((void **)&ctx->list_host, sizeof(long long) * want, hipHostMallocDefault));
		ctx->list_cap = want;
	}
	long long *dev = (long long *)dwtx_scratch(ctx, SLOT_CD_LIST, bytes);
	if (!dev)
		return DWTX_ERR_NOMEM;
	memcpy(ctx->list_host, offs.data(), bytes);
	DWTX_HIP(hipMemcpyAsync(dev, ctx->list_host, bytes, hipMemcpyHostToDevice, ctx->stream));
	DWTX_HIP(hipEventRecord(ctx->list_sent, ctx->stream));
	px->offs = dev;
	return DWTX_OK;
}

// dwtx_float_format -> the sample kind of dwtx_pixels, checked (what both float calls refuse alike)
static int float_kind(const dwtx_float_format *fmt, int *kind)
{
	if (!fmt) {
		dwtx_set_error("float view: no dwtx_float_format");
		return DWTX_ERR_ARG;
	}
	if (fmt->type != DWTX_FLOAT32 && fmt->type != DWTX_FLOAT16 && fmt->type != DWTX_BFLOAT16) {
		dwtx_set_error("float view: type %d (DWTX_FLOAT32 = 0, DWTX_FLOAT16 = 1 or DWTX_BFLOAT16 = 2)", fmt->type);
		return DWTX_ERR_ARG;
	}
	for (int c = 0; c < 3; ++c)
		if (!isfinite(fmt->scale[c]) || !isfinite(fmt->bias[c])) {
			dwtx_set_error("float view: scale[%d] = %g, bias[%d] = %g: both must be finite", c, (double)fmt->scale[c], c, (double)fmt->bias[c]);
			return DWTX_ERR_ARG;
		}
	*kind = fmt->type == DWTX_FLOAT32 ? DWTX_SAMPLE_F32 : fmt->type == DWTX_FLOAT16 ? DWTX_SAMPLE_F16 : DWTX_SAMPLE_BF16;
	return DWTX_OK;
}

extern "C" int dwtx_crop_plan(int W, int H, int x0, int y0, int cw, int ch, dwtx_crop_rect out[DWTX_MAX_LEVELS + 1])
{
	DWTX_CHECK_DIMS(W, H);
	if (!out || cw < 1 || ch < 1 || x0 < 0 || y0 < 0 || x0 > W - cw || y0 > H - ch) {
		dwtx_set_error("crop plan: %dx%d at (%d, %d) is no window of a %dx%d picture", cw, ch, x0, y0, W, H);
		return DWTX_ERR_ARG;
	}
	dwtx_geom g;
	if (const int rc = dwtx_geometry(&g, W, H))
		return rc;
	// (margins: include/dwtx.h, and lift.hip where the kernel is) outputs [a, b) of a line need k0 - 1 .. k1 of the level below
	int xa = x0, xb = x0 + cw, ya = y0, yb = y0 + ch;
	out[g.levels] = dwtx_crop_rect{ xa, ya, xb - xa, yb - ya };
	for (int l = g.levels - 1; l >= 0; --l) {
		xa = xa / 2 - 1 > 0 ? xa / 2 - 1 : 0;
		ya = ya / 2 - 1 > 0 ? ya / 2 - 1 : 0;
		xb = (xb + 1) / 2 + 1 < g.widths[l] ? (xb + 1) / 2 + 1 : g.widths[l];
		yb = (yb + 1) / 2 + 1 < g.heights[l] ? (yb + 1) / 2 + 1 : g.heights[l];
		out[l] = dwtx_crop_rect{ xa, ya, xb - xa, yb - ya };
	}
	return g.levels;
}

// what the crop calls refuse of a crop and its origins; *whole: the crop is every picture itself (the plain call)
static int crop_of_call(const ViewCall &c, bool *whole)
{
	const int W = c.W, H = c.H;
	DWTX_CHECK_DIMS(W, H);
	if (c.crop_w < 1 || c.crop_w > W || c.crop_h < 1 || c.crop_h > H) {
		dwtx_set_error("crop: %dx%d is no window of a %dx%d picture (sides of 1 up to the picture's)", c.crop_w, c.crop_h, W, H);
		return DWTX_ERR_ARG;
	}
	if (c.n < 1) {
		dwtx_set_error("no view, no pixels or no windows");
		return DWTX_ERR_ARG;
	}
	*whole = c.crop_w == W && c.crop_h == H;
	for (int i = 0; c.host_origins && i < c.n; ++i) {
		const int x0 = c.host_origins[2 * i], y0 = c.host_origins[2 * i + 1];
		if (x0 < 0 || y0 < 0 || x0 > W - c.crop_w || y0 > H - c.crop_h) {
			dwtx_set_error("crop: origin (%d, %d) of picture %d puts its %dx%d window outside the %dx%d picture", x0, y0, i, c.crop_w, c.crop_h, W, H);
			return DWTX_ERR_ARG;
		}
		*whole = *whole && !x0 && !y0;
	}
	return DWTX_OK;
}

// window i's flags of a call with flips, checked: host_flips[i], or `flip` for all; *any: one of them is not 0
static int flip_flags(const ViewCall &c, std::vector<unsigned char> *flags, bool *any)
{
	*any = false;
	if (c.host_flips && c.flip) {
		dwtx_set_error("flip: flags for all windows (%d) together with a flag per window (host_flips): one of the two", c.flip);
		return DWTX_ERR_ARG;
	}
	if (c.flip < 0 || c.flip > (DWTX_FLIP_X | DWTX_FLIP_Y)) {
		dwtx_set_error("flip: flags %d (a mask of DWTX_FLIP_X = 1 and DWTX_FLIP_Y = 2: 0..3)", c.flip);
		return DWTX_ERR_ARG;
	}
	if (c.n < 1) {
		dwtx_set_error("no view, no pixels or no windows");
		return DWTX_ERR_ARG;
	}
	try {
		flags->assign((size_t)c.n, (unsigned char)c.flip);
	} catch (...) {
		return DWTX_ERR_NOMEM;
	}
	for (int i = 0; i < c.n; ++i) {
		if (c.host_flips)
			(*flags)[(size_t)i] = c.host_flips[i];
		if ((*flags)[(size_t)i] > (DWTX_FLIP_X | DWTX_FLIP_Y)) {
			dwtx_set_error("flip: flags %d of window %d (a mask of DWTX_FLIP_X = 1 and DWTX_FLIP_Y = 2: 0..3)", (int)(*flags)[(size_t)i], i);
			return DWTX_ERR_ARG;
		}
		*any = *any || (*flags)[(size_t)i];
	}
	return DWTX_OK;
}

// What the delta and the chain calls refuse of their two views before either is looked at alone: `what` view and its `other`
static int pair_refusals(const ViewCall &c, const char *what, const char *other)
{
	const int minval = c.minval ? *c.minval : 0;
	if (c.sgn != 0 && c.sgn != 1) {
		dwtx_set_error("%s view: sgn %d (0: uint8_t / uint16_t samples, 1: int16_t samples)", what, c.sgn);
		return DWTX_ERR_ARG;
	}
	if (!c.sgn && minval != 0) {
		dwtx_set_error("%s view: minval %d without sgn (unsigned samples start at 0)", what, minval);
		return DWTX_ERR_ARG;
	}
	if (c.view->channels != c.other->channels) {
		dwtx_set_error("%s view: the view has %d channels, its %s %d", what, c.view->channels, other, c.other->channels);
		return DWTX_ERR_ARG;
	}
	if (c.view->sample_bytes != c.other->sample_bytes) {
		dwtx_set_error("%s view: the view has %d-byte samples, its %s %d-byte ones", what, c.view->sample_bytes, other, c.other->sample_bytes);
		return DWTX_ERR_ARG;
	}
	return DWTX_OK;
}

// What the clips calls refuse before the view is looked at (pair_refusals' place and, without a second view, its rules).  What
// view_pixels refuses of the view itself — everything dwtx_encode_view_order / dwtx_decode_view_order refuse, the signed calls'
// sample size and range — it words as theirs: every text of a clips call starts "clips view:"
static int clips_refusals(const ViewCall &c)
{
	const int minval = c.minval ? *c.minval : 0;
	if (c.period < 1) {
		dwtx_set_error("clips view: period %d (every period-th window is a key: 1 or more; period >= n is one clip)", c.period);
		return DWTX_ERR_ARG;
	}
	if (!c.view) {
		dwtx_set_error("clips view: no view");
		return DWTX_ERR_ARG;
	}
	if (c.sgn != 0 && c.sgn != 1) {
		dwtx_set_error("clips view: sgn %d (0: uint8_t / uint16_t samples, 1: int16_t samples)", c.sgn);
		return DWTX_ERR_ARG;
	}
	if (c.sgn && c.view->sample_bytes == 1) {
		dwtx_set_error("clips view: sgn with 1-byte samples (signed samples are int16_t)");
		return DWTX_ERR_ARG;
	}
	if (!c.sgn && minval != 0) {
		dwtx_set_error("clips view: minval %d without sgn (unsigned samples start at 0)", minval);
		return DWTX_ERR_ARG;
	}
	return DWTX_OK;
}

// What dwtx_decode_view_clips_crop adds to them, in the same place: the pictures' size (the view's windows are the crop's), the
// crop's sides, one origin per CLIP (clip k: windows [k * period, (k + 1) * period)), the float type and its scale and bias.
// *whole: the crop is every picture itself; *kind: the float samples, -1 for integer ones; *per_picture: the origins as
// dwtx_inv_crop's table is built from them, one pair per picture (empty: all at (0, 0)).
static int clips_crop_refusals(const ViewCall &c, bool *whole, int *kind, std::vector<int> *per_picture)
{
	const int W = c.W, H = c.H;
	if (!dwtx_dims_ok(W, H)) {
		dwtx_set_error("clips view: unsupported image size %dx%d (8..%d per side)", W, H, DWTX_MAX_SIDE);
		return DWTX_ERR_ARG;
	}
	if (c.n < 1) {
		dwtx_set_error("clips view: no view, no pixels or no windows");
		return DWTX_ERR_ARG;
	}
	if (c.crop_w < 1 || c.crop_w > W || c.crop_h < 1 || c.crop_h > H) {
		dwtx_set_error("clips view: crop %dx%d is no window of a %dx%d picture (sides of 1 up to the picture's)", c.crop_w, c.crop_h, W, H);
		return DWTX_ERR_ARG;
	}
	*whole = c.crop_w == W && c.crop_h == H;
	const int nclips = (int)(((long)c.n + c.period - 1) / c.period);
	for (int k = 0; c.host_origins && k < nclips; ++k) {
		const int x0 = c.host_origins[2 * k], y0 = c.host_origins[2 * k + 1];
		if (x0 < 0 || y0 < 0 || x0 > W - c.crop_w || y0 > H - c.crop_h) {
			dwtx_set_error("clips view: origin (%d, %d) of clip %d puts its %dx%d window outside the %dx%d picture", x0, y0, k, c.crop_w, c.crop_h, W, H);
			return DWTX_ERR_ARG;
		}
		*whole = *whole && !x0 && !y0;
	}
	*kind = -1;
	if (c.fmt) {
		if (c.fmt->type != DWTX_FLOAT32 && c.fmt->type != DWTX_FLOAT16 && c.fmt->type != DWTX_BFLOAT16) {
			dwtx_set_error("clips view: float type %d (DWTX_FLOAT32 = 0, DWTX_FLOAT16 = 1 or DWTX_BFLOAT16 = 2)", c.fmt->type);
			return DWTX_ERR_ARG;
		}
		for (int k = 0; k < 3; ++k)
			if (!isfinite(c.fmt->scale[k]) || !isfinite(c.fmt->bias[k])) {
				dwtx_set_error("clips view: scale[%d] = %g, bias[%d] = %g: both must be finite", k, (double)c.fmt->scale[k], k, (double)c.fmt->bias[k]);
				return DWTX_ERR_ARG;
			}
		*kind = c.fmt->type == DWTX_FLOAT32 ? DWTX_SAMPLE_F32 : c.fmt->type == DWTX_FLOAT16 ? DWTX_SAMPLE_F16 : DWTX_SAMPLE_BF16;
	}
	per_picture->clear();
	if (c.host_origins && !*whole) {
		try {
			per_picture->resize(2 * (size_t)c.n);
		} catch (...) {
			return DWTX_ERR_NOMEM;
		}
		for (int i = 0; i < c.n; ++i) {
			(*per_picture)[2 * (size_t)i] = c.host_origins[2 * (i / c.period)];
			(*per_picture)[2 * (size_t)i + 1] = c.host_origins[2 * (i / c.period) + 1];
		}
	}
	return DWTX_OK;
}

// The units of a grid view — its n windows, or the 3n planes of planar RGB, as in list_windows — as byte spans [first, first +
// (H-1)*row_pitch + row) of the address space, appended to `spans` with `tag`
struct DeltaSpan {
	uintptr_t at, end;
	int tag, window;
};
static void delta_spans(const dwtx_pixels &px, int W, int H, int n, int tag, std::vector<DeltaSpan> *spans)
{
	const size_t span = (size_t)(H - 1) * px.pitch(W) + px.row_samples(W);
	for (int i = 0; i < n; ++i)
		for (int c = 0; c < (px.planar() ? 3 : 1); ++c) {
			const uintptr_t at = (uintptr_t)px.at(px.grid_offset((size_t)i) + (size_t)c * px.channel_stride);
			spans->push_back(DeltaSpan{ at, at + px.bytes(span), tag, i });
		}
}

// A delta decode whose base is not the destination itself (the in-place decode: each sample read and written by the same lane):
// no unit of the destination may meet a unit of the base.  One sort and one sweep: by address, a span that begins before a span
// of the other view has ended meets it.
static int delta_disjoint(const dwtx_pixels &px, const dwtx_pixels &bp, int W, int H, int n)
{
	std::vector<DeltaSpan> spans;
	try {
		spans.reserve(6 * (size_t)n);
		delta_spans(px, W, H, n, 0, &spans);
		delta_spans(bp, W, H, n, 1, &spans);
	} catch (...) {
		return DWTX_ERR_NOMEM;
	}
	std::sort(spans.begin(), spans.end(), [](const DeltaSpan &a, const DeltaSpan &b) { return a.at < b.at; });
	uintptr_t end[2] = { 0, 0 };
	int last[2] = { -1, -1 };
	for (const DeltaSpan &s : spans) {
		const int other = 1 - s.tag;
		if (s.at < end[other]) {
			const int wd = s.tag ? last[other] : s.window, wb = s.tag ? s.window : last[other];
			dwtx_set_error("delta view: window %d of the destination meets window %d of the base (neither the same view, which decodes in place, "
				"nor disjoint spans: a decode that writes what it has yet to read is a chain, not one call)", wd, wb);
			return DWTX_ERR_ARG;
		}
		if (s.end > end[s.tag]) {
			end[s.tag] = s.end;
			last[s.tag] = s.window;
		}
	}
	return DWTX_OK;
}

// A chain decode: every unit of the destination (a window; a plane of planar RGB) must be disjoint from every unit of the key:
// delta_disjoint's spans with one base window, so each destination unit is held against the key's one or three directly, no
// sort.  Two spans that intersect are still disjoint where both units have the same pitch in bytes and lie in different columns of
// the lattice of rows that pitch apart (other_columns): a key in the gap between a window's rows and its pitch.
static int chain_disjoint(const dwtx_pixels &px, const dwtx_pixels &kp, int W, int H, int n)
{
	std::vector<DeltaSpan> spans;
	try {
		spans.reserve(3 * (size_t)n + 3);
		delta_spans(kp, W, H, 1, 1, &spans);
		delta_spans(px, W, H, n, 0, &spans);
	} catch (...) {
		return DWTX_ERR_NOMEM;
	}
	const size_t nkey = kp.planar() ? 3 : 1;
	const uintptr_t pitch = px.bytes(px.pitch(W)), kpitch = kp.bytes(kp.pitch(W));
	const uintptr_t row = px.bytes(px.row_samples(W)), krow = kp.bytes(kp.row_samples(W));
	for (size_t i = nkey; i < spans.size(); ++i) {
		const DeltaSpan &d = spans[i];
		for (size_t k = 0; k < nkey; ++k) {
			const DeltaSpan &b = spans[k];
			if (d.end <= b.at || b.end <= d.at)
				continue;
			// (the key's columns on the lattice of the window's rows)
			if (pitch == kpitch && other_columns(b.at >= d.at ? (b.at - d.at) % pitch : (pitch - (d.at - b.at) % pitch) % pitch, row, krow, pitch))
				continue;
			dwtx_set_error("chain view: window %d of the destination meets the key (every unit of the destination must be disjoint from the key's: "
				"frame 0 of a stack as the key of frames 1.. is the layout to use)", d.window);
			return DWTX_ERR_ARG;
		}
	}
	return DWTX_OK;
}

// What plan_view makes of a call: all that encode_device / decode_device are told
struct ViewPlan {
	dwtx_pixels px;                // the view (offs not set yet: send_list)
	std::vector<long long> offs;   // the windows' table in host memory: each one's first sample, in samples from px.base, a flipped one's
	                               // flags on top (dwtx_pixels::flips); empty unless the call is listed or flipped
	bool cropped = false;          // crop: only that window of every picture is written; else whole pictures
	CropCall crop;
	std::vector<int> origins;      // a clip stack's crop: its per-clip origins spelled out per picture (crop.origins points here)
	dwtx_pixels key;               // a chain encode: the key's one window
};

// The one resolver of every view call: host arithmetic only, no context and no device.  It refuses, in this order (DESIGN.md
// section 4.23): the flags; the crop and its origins; the float format; of a delta or chain pair the missing view, sgn, minval,
// channels and sample bytes (of a clips call, in that place: the period, the missing view, sgn, its sample size and minval);
// the view itself (view_pixels), the size of its table and its list (list_windows); a float source's range; the pair's other
// view and the places where the two meet.  Four calls are, by the header's word, another call with fewer arguments, and become
// that call here — nowhere else is a neutral argument looked at.
static int plan_view(const ViewCall &call, ViewPlan *plan)
{
	ViewCall c = call;
	dwtx_pixels &px = plan->px;
	int rc;
	std::vector<unsigned char> flags;
	bool flipped = false;
	if (c.flip || c.host_flips || c.table) {
		// no window flipped: "the list / plain call, and takes its path" — `flipped` stays false, and a grid stays a grid
		if ((rc = flip_flags(c, &flags, &flipped)))
			return rc;
		flipped = flipped || c.table;
	}
	if (c.crop && !c.clip_crop) {
		bool whole;
		if ((rc = crop_of_call(c, &whole)))
			return rc;
		// the whole picture at (0, 0): "the call without a crop"
		c.crop = !whole;
	}
	int kind = -1;
	if (c.clip_crop)
		;   // (the format of a clip stack's crop call is looked at with the crop, below)
	else if (c.fmt || c.needs_fmt) {
		if ((rc = float_kind(c.fmt, &kind)))
			return rc;
	} else if (c.kind_from_bytes && c.view && c.view->sample_bytes == 4)
		kind = DWTX_SAMPLE_F32;
	// float samples with minval == 0: "the unsigned call's"
	if (kind >= 0 && c.minval && *c.minval == 0)
		c.minval = nullptr;
	if (c.pair == PAIR_DELTA) {
		if (!c.view || !c.other) {
			dwtx_set_error("delta view: no view or no base view");
			return DWTX_ERR_ARG;
		}
		if ((rc = pair_refusals(c, "delta", "base")))
			return rc;
	} else if (c.pair == PAIR_CHAIN) {
		if (!c.view) {
			dwtx_set_error("chain view: no view");
			return DWTX_ERR_ARG;
		}
		if (!c.other || !c.other->dev) {
			dwtx_set_error("chain view: no key (the base of picture 0 is required: a chain without one is a plain call and n - 1 links)");
			return DWTX_ERR_ARG;
		}
		if ((rc = pair_refusals(c, "chain", "key")))
			return rc;
	} else if (c.pair == PAIR_CLIPS) {
		if ((rc = clips_refusals(c)))
			return rc;
		if (c.clip_crop) {
			bool whole;
			if ((rc = clips_crop_refusals(c, &whole, &kind, &plan->origins)))
				return rc;
			// the whole picture at (0, 0): the clips call on full-size windows (with integer samples: dwtx_decode_view_clips itself)
			c.crop = !whole;
			c.host_origins = plan->origins.empty() ? nullptr : plan->origins.data();   // (per picture from here on, as decode_device reads them)
			if (kind >= 0 && c.minval && *c.minval == 0)   // float samples from 0 up: the unsigned range rule, as in the float calls
				c.minval = nullptr;
		}
	}
	if (c.pair && !c.sgn)
		c.minval = nullptr;
	if ((rc = view_pixels(c, kind, &px)))
		return rc;
	if ((c.windows || flipped) && !table_count_ok(c, px.channels))
		return DWTX_ERR_ARG;
	if (c.windows && (rc = list_windows(c, &plan->offs, &px)))
		return rc;
	if (c.fmt) {
		// the quantiser's clamp of a float source: maxval alone, or the range of a signed call with a lower bound other than 0
		if (!c.dst && !(c.minval ? dwtx_range_ok(*c.minval, c.view->maxval) : dwtx_maxval_ok(c.view->maxval)))
			return DWTX_ERR_ARG;
		for (int k = 0; k < 3; ++k) {
			px.scale[k] = c.fmt->scale[k];
			px.bias[k] = c.fmt->bias[k];
		}
	}
	if (c.pair == PAIR_CLIPS) {
		// no second view: the base of a link is the window before it, of the view itself (lift.hip's clips conversions)
		px.clips = c.period;
	} else if (c.pair) {
		// The other view, checked as the *_view_order / *_view_signed calls check theirs: it is only ever read, and its maxval is not.
		// A key is one window: what lies between windows is not the key's to say.
		ViewCall o = c;
		dwtx_view one = *c.other;
		if (c.pair == PAIR_CHAIN) {
			one.cols = 0;
			one.image_stride = one.band_stride = 0;
			o.n = 1;
		}
		o.view = &one;
		o.pixel_step = c.other_step;
		o.dst = false;
		dwtx_pixels op;
		if ((rc = view_pixels(o, kind, &op)))
			return rc;
		const int W = c.win_w(), H = c.win_h();
		if (c.pair == PAIR_DELTA) {
			if (c.dst && !(px.grid() == op.grid()) && (rc = delta_disjoint(px, op, W, H, c.n)))
				return rc;
			px.delta = op.grid();
		} else {
			if (c.dst && (rc = chain_disjoint(px, op, W, H, c.n)))
				return rc;
			if (!c.dst)
				plan->key = op;   // (two delta encodes: encode_views)
			else if (c.n == 1)
				px.delta = op.grid();   // one link: "dwtx_decode_view_delta with base = key", the fused sinks where the pair qualifies
			else {
				px.chain = true;
				px.key = op.grid();
			}
		}
	}
	if (flipped) {
		// Every flipped call travels as a listed one: a grid is spelled out, its table from the view's own strides
		if (!c.windows) {
			try {
				plan->offs.resize((size_t)c.n);
			} catch (...) {
				return DWTX_ERR_NOMEM;
			}
			px.offs_on_quad = true;   // (what wide() asks of a list: every window's own first sample on the quad)
			for (size_t i = 0; i < (size_t)c.n; ++i) {
				plan->offs[i] = (long long)px.grid_offset(i);
				px.offs_on_quad = px.offs_on_quad && plan->offs[i] % 4 == 0;
			}
			px.cols = 0;
			px.band_stride = px.image_stride = 0;
		}
		px.flips = true;
		px.flip_w = c.win_w();
		px.flip_h = c.win_h();
		// a source: bottom-up windows go through the wide forward kernels like upright ones, a mirrored one sends the call through the
		// general conversion; a destination: the FL instances of the wide inverse kernels, which ask whether any window is mirrored
		bool mirrored = false;
		for (size_t i = 0; i < (size_t)c.n; ++i) {
			mirrored = mirrored || (flags[i] & DWTX_FLIP_X);
			// the flags into the top bits of the windows' table entries (offsets are sample counts of one allocation, far below)
			plan->offs[i] = (long long)((unsigned long long)plan->offs[i] | (unsigned long long)flags[i] << DWTX_FLIP_SHIFT);
		}
		px.flip_wide = !c.dst && !mirrored;
		px.flip_sink = c.dst;
		px.flip_x = c.dst && mirrored;
	}
	plan->cropped = c.crop;
	plan->crop = CropCall{ c.crop_w, c.crop_h, c.host_origins };
	return DWTX_OK;
}

// A view call's pixels (device) -> streams (device): resolve, check the call's own pointers, send the table if there is one, encode
static int encode_views(dwtx_ctx *ctx, const ViewCall &call, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	ViewPlan plan;
	if (const int rc = plan_view(call, &plan))
		return rc;
	if (!ctx || !dev_out || !dev_info)
		return DWTX_ERR_ARG;
	if (!plan.offs.empty())
		if (const int rc = send_list(ctx, plan.offs, &plan.px))
			return rc;
	dwtx_index *index = ctx->enc_index;
	if (call.pair != PAIR_CHAIN)
		return encode_device(ctx, plan.px, call.W, call.H, call.n, capacity, dev_out, out_stride, dev_info, index);
	// A chain: stream 0 is window 0 minus the key, stream i window i minus window i - 1: two delta encodes, the second `src[1:]`
	// against `src[:-1]` — the streams, the records and the encode index land at entry i for stream i.
	dwtx_pixels head = plan.px;
	head.delta = plan.key.grid();
	if (const int rc = encode_device(ctx, head, call.W, call.H, 1, capacity, dev_out, out_stride, dev_info, index))
		return rc;
	if (call.n == 1)
		return DWTX_OK;
	dwtx_pixels tail = plan.px.image(1);   // (the view has no base yet: only the view moves, and its base is the view from window 0 on)
	tail.delta = plan.px.grid();
	return encode_device(ctx, tail, call.W, call.H, call.n - 1, capacity, dev_out + out_stride, out_stride, dev_info + 1, index ? index + 1 : nullptr);
}

// streams (device) -> a view call's pixels (device): the same steps
static int decode_views(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens, const ViewCall &call,
	dwtx_decode_info *host_info)
{
	ViewPlan plan;
	if (const int rc = plan_view(call, &plan))
		return rc;
	if (!ctx || !dev_streams || !dev_lens || !host_info)
		return DWTX_ERR_ARG;
	if (!plan.offs.empty())
		if (const int rc = send_list(ctx, plan.offs, &plan.px))
			return rc;
	return decode_device(ctx, dev_streams, stream_stride, dev_lens, call.W, call.H, call.n, call.levels_max, plan.px, host_info,
		plan.cropped ? &plan.crop : nullptr);
}

// The entry points (include/dwtx.h): each names the fields that its ABI has, and nothing else

extern "C" int dwtx_encode_view(dwtx_ctx *ctx, const dwtx_view *src, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_step(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_order(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, int W, int H, int n, long capacity,
	uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

// The source's maxval is the quantiser's clamp (the one encode that reads it): up to 255 the picture is one of bytes and takes
// their route, beyond it a deep picture's (dwtx_pixels::deep_source()); the streams are those of dwtx_encode_device /
// dwtx_encode_device16 on the quantised picture either way.
extern "C" int dwtx_encode_view_float(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .fmt = fmt, .W = W, .H = H, .n = n, .needs_fmt = true };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_list(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, const dwtx_float_format *fmt,
	const void *const *host_windows, int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .W = W, .H = H, .n = n,
		.needs_windows = true };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_flip(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, const dwtx_float_format *fmt,
	const void *const *host_windows, int flip, const unsigned char *host_flips,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .flip = flip,
		.host_flips = host_flips, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_signed(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int order, const dwtx_float_format *fmt,
	const void *const *host_windows, int flip, const unsigned char *host_flips, int minval,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .flip = flip,
		.host_flips = host_flips, .minval = &minval, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_delta(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step,
	int order, int sgn, int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const int minval = 0;   // (a source is only read: its range is its samples')
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_DELTA, .other = base,
		.other_step = base_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_encode_view_chain(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step,
	int order, int sgn, int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const int minval = 0;   // (a source is only read: its range is its samples')
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_CHAIN, .other = key,
		.other_step = key_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

// (one encode_device call: the clips instance of the forward conversion subtracts window i - 1 from every window but the keys)
extern "C" int dwtx_encode_view_clips(dwtx_ctx *ctx, const dwtx_view *src, size_t pixel_step, int period, int order, int sgn,
	int W, int H, int n, long capacity, uint8_t *dev_out, size_t out_stride, dwtx_stream_info *dev_info)
{
	const int minval = 0;   // (a source is only read: its range is its samples')
	const ViewCall c = { .view = src, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_CLIPS, .sgn = sgn, .period = period,
		.W = W, .H = H, .n = n };
	return encode_views(ctx, c, capacity, dev_out, out_stride, dev_info);
}

extern "C" int dwtx_decode_view(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max, const dwtx_view *dst, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_step(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_order(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_float(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order,
	const dwtx_float_format *fmt, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .levels_max = levels_max, .W = W, .H = H, .n = n,
		.dst = true, .needs_fmt = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_crop(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .crop = true, .crop_w = crop_w, .crop_h = crop_h,
		.host_origins = host_origins, .levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_list(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .crop = true, .crop_w = crop_w,
		.crop_h = crop_h, .host_origins = host_origins, .levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true, .needs_windows = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_flip(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows, int flip, const unsigned char *host_flips,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .flip = flip,
		.host_flips = host_flips, .crop = true, .crop_w = crop_w, .crop_h = crop_h, .host_origins = host_origins, .levels_max = levels_max,
		.W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_signed(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, int levels_max, const dwtx_view *dst, size_t pixel_step, int order, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, void *const *host_windows, int flip, const unsigned char *host_flips, int minval,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .windows = host_windows, .flip = flip,
		.host_flips = host_flips, .minval = &minval, .crop = true, .crop_w = crop_w, .crop_h = crop_h, .host_origins = host_origins,
		.levels_max = levels_max, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_delta(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step, int order, int sgn, int minval,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_DELTA, .other = base,
		.other_step = base_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_chain(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step, int order, int sgn, int minval,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_CHAIN, .other = key,
		.other_step = key_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

extern "C" int dwtx_decode_view_clips(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, int period, int order, int sgn, int minval,
	dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .minval = &minval, .pair = PAIR_CLIPS, .sgn = sgn, .period = period,
		.W = W, .H = H, .n = n, .dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

// (the clips call with a crop per clip and an optional float format: plan_view makes the full-size integer call the call above)
extern "C" int dwtx_decode_view_clips_crop(dwtx_ctx *ctx, const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens,
	int W, int H, int n, const dwtx_view *dst, size_t pixel_step, int period, int order, int sgn, int minval, const dwtx_float_format *fmt,
	int crop_w, int crop_h, const int *host_origins, dwtx_decode_info *host_info)
{
	const ViewCall c = { .view = dst, .pixel_step = pixel_step, .order = order, .fmt = fmt, .minval = &minval, .crop = true, .crop_w = crop_w,
		.crop_h = crop_h, .host_origins = host_origins, .pair = PAIR_CLIPS, .sgn = sgn, .period = period, .clip_crop = true, .W = W, .H = H, .n = n,
		.dst = true };
	return decode_views(ctx, dev_streams, stream_stride, dev_lens, c, host_info);
}

// The host-only exports: the resolver's verdict, and for the flip plan its table read back

extern "C" int dwtx_view_list_check(const dwtx_view *v, size_t pixel_step, int W, int H, int n, const void *const *host_windows, int dst)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .windows = host_windows, .W = W, .H = H, .n = n, .dst = dst != 0,
		.needs_windows = true, .kind_from_bytes = true, .thin = true };
	ViewPlan plan;
	return plan_view(c, &plan);
}

extern "C" int dwtx_view_flip_plan(const dwtx_view *v, size_t pixel_step, int W, int H, int n, const void *const *host_windows,
	int flip, const unsigned char *host_flips, int dst, long long *origin, long long *pitch, long long *step)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .windows = host_windows, .flip = flip, .host_flips = host_flips,
		.W = W, .H = H, .n = n, .dst = dst != 0, .kind_from_bytes = true, .thin = true, .table = true };
	ViewPlan plan;
	if (const int rc = plan_view(c, &plan))
		return rc;
	const long long p = (long long)plan.px.row_pitch, s = (long long)plan.px.step();
	for (int i = 0; i < n; ++i) {
		const unsigned long long entry = (unsigned long long)plan.offs[(size_t)i], flags = entry >> DWTX_FLIP_SHIFT;
		const bool fx = flags & DWTX_FLIP_X, fy = flags & DWTX_FLIP_Y;
		if (origin)
			origin[i] = (long long)(entry & ((1ull << DWTX_FLIP_SHIFT) - 1)) + (fy ? (long long)(H - 1) * p : 0) + (fx ? (long long)(W - 1) * s : 0);
		if (pitch)
			pitch[i] = fy ? -p : p;
		if (step)
			step[i] = fx ? -s : s;
	}
	return DWTX_OK;
}

extern "C" int dwtx_view_delta_check(const dwtx_view *v, size_t pixel_step, const dwtx_view *base, size_t base_pixel_step,
	int sgn, int minval, int W, int H, int n, int dst)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .minval = &minval, .pair = PAIR_DELTA, .other = base,
		.other_step = base_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n, .dst = dst != 0 };
	ViewPlan plan;
	return plan_view(c, &plan);
}

extern "C" int dwtx_view_chain_check(const dwtx_view *v, size_t pixel_step, const dwtx_view *key, size_t key_pixel_step,
	int sgn, int minval, int W, int H, int n, int dst)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .minval = &minval, .pair = PAIR_CHAIN, .other = key,
		.other_step = key_pixel_step, .sgn = sgn, .W = W, .H = H, .n = n, .dst = dst != 0 };
	ViewPlan plan;
	return plan_view(c, &plan);
}

extern "C" int dwtx_view_clips_check(const dwtx_view *v, size_t pixel_step, int period, int sgn, int minval, int W, int H, int n, int dst)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .minval = &minval, .pair = PAIR_CLIPS, .sgn = sgn, .period = period,
		.W = W, .H = H, .n = n, .dst = dst != 0 };
	ViewPlan plan;
	return plan_view(c, &plan);
}

extern "C" int dwtx_view_clips_crop_check(const dwtx_view *v, size_t pixel_step, int period, int sgn, int minval, const dwtx_float_format *fmt,
	int W, int H, int n, int crop_w, int crop_h, const int *host_origins)
{
	const ViewCall c = { .view = v, .pixel_step = pixel_step, .order = DWTX_ORDER_RGB, .fmt = fmt, .minval = &minval, .crop = true, .crop_w = crop_w,
		.crop_h = crop_h, .host_origins = host_origins, .pair = PAIR_CLIPS, .sgn = sgn, .period = period, .clip_crop = true, .W = W, .H = H, .n = n,
		.dst = true };
	ViewPlan plan;
	return plan_view(c, &plan);
}

// one axis of dwtx_tile_groups: `full` tiles of `tile`, then one of `last` (0: none)
static void tile_axis(int side, int tile, int *full, int *last)
{
	const int rem = side % tile;
	*full = side / tile;
	*last = rem;
	if (*full && rem && rem < DWTX_MIN_LEN) {   // too thin to be a picture: the last full tile takes it
		--*full;
		*last = tile + rem;
	}
}

extern "C" int dwtx_tile_groups(int frameW, int frameH, int tile, dwtx_tile_group out[4])
{
	if (!out || tile < DWTX_MIN_LEN || tile % 4 || tile > DWTX_MAX_SIDE || frameW < DWTX_MIN_LEN || frameH < DWTX_MIN_LEN) {
		dwtx_set_error("tile plan: tile %d (a multiple of 4 in 8..%d), frame %dx%d (8 or more per side)", tile, DWTX_MAX_SIDE, frameW, frameH);
		return DWTX_ERR_ARG;
	}
	int fx, lx, fy, ly;
	tile_axis(frameW, tile, &fx, &lx);
	tile_axis(frameH, tile, &fy, &ly);
	if (lx > DWTX_MAX_SIDE || ly > DWTX_MAX_SIDE) {
		dwtx_set_error("tile plan: the widened last tile (%d x %d) is beyond %d", lx, ly, DWTX_MAX_SIDE);
		return DWTX_ERR_ARG;
	}
	// columns of tiles: the full ones, then the last; rows the same — interior, right column, bottom row, corner
	const int xs[2][3] = { { 0, tile, fx }, { fx * tile, lx, lx ? 1 : 0 } }, ys[2][3] = { { 0, tile, fy }, { fy * tile, ly, ly ? 1 : 0 } };
	int k = 0;
	for (int b = 0; b < 2; ++b)
		for (int a = 0; a < 2; ++a)
			if (xs[a][2] && ys[b][2])
				out[k++] = dwtx_tile_group{ xs[a][0], ys[b][0], xs[a][1], ys[b][1], xs[a][2], ys[b][2] };
	return k;
}

// ---- dwtx_pack_streams: a step's streams as one message (include/dwtx.h) -------------------------------------------
namespace {
constexpr int PK_THREADS = 256;
constexpr int PK_PIECE = 1 << 16;   // bytes of one stream a workgroup moves

__device__ __forceinline__ unsigned long long pk_round8(unsigned long long len, unsigned long long stride)
{
	return ((len < stride ? len : stride) + 7ull) & ~7ull;
}

// grid (pieces of the longest possible stream, n): every workgroup adds up the rounded lengths before its stream
// (n is a batch size: a few hundred 8-byte loads from L2) and moves its piece with 8-byte accesses — rows and offsets are
// multiples of 8 bytes
__global__ __launch_bounds__(PK_THREADS) void k_pack_streams(uint8_t *out, unsigned long long out_bytes, unsigned long long *offsets,
	const uint8_t *streams, unsigned long long stride, const unsigned long long *lens, int n)
{
	__shared__ unsigned long long part[PK_THREADS / 64];
	const int i = blockIdx.y;
	unsigned long long mine = 0;
	for (int j = threadIdx.x; j < i; j += PK_THREADS)
		mine += pk_round8(lens[j], stride);
	for (int o = 32; o; o >>= 1)
		mine += __shfl_down(mine, o);
	if ((threadIdx.x & 63) == 0)
		part[threadIdx.x >> 6] = mine;
	__syncthreads();
	unsigned long long off = 0;
	for (int k = 0; k < PK_THREADS / 64; ++k)
		off += part[k];
	const unsigned long long len8 = pk_round8(lens[i], stride);
	if (offsets && blockIdx.x == 0 && threadIdx.x == 0) {
		offsets[i] = off;
		if (i == n - 1)
			offsets[n] = off + len8;
	}
	const unsigned long long first = (unsigned long long)blockIdx.x * PK_PIECE;
	if (first >= len8)
		return;
	const unsigned long long last = first + PK_PIECE < len8 ? first + PK_PIECE : len8;
	const unsigned long long *src = reinterpret_cast<const unsigned long long *>(streams + (unsigned long long)i * stride);
	unsigned long long *dst = reinterpret_cast<unsigned long long *>(out + off);
	for (unsigned long long b = first + 8ull * threadIdx.x; b < last; b += 8ull * PK_THREADS) {
		if (off + b + 8 <= out_bytes) {
			dst[b >> 3] = src[b >> 3];
		} else if (off + b < out_bytes) {   // the piece out_bytes cuts: its bytes before the cut, one by one
			const uint8_t *s8 = streams + (unsigned long long)i * stride + b;
			for (unsigned long long k = 0; off + b + k < out_bytes; ++k)
				out[off + b + k] = s8[k];
		}
	}
}
} // namespace

extern "C" int dwtx_pack_streams(dwtx_ctx *ctx, uint8_t *dev_out, size_t out_bytes, unsigned long long *dev_offsets,
	const uint8_t *dev_streams, size_t stream_stride, const unsigned long long *dev_lens, int n)
{
	if (!ctx || !dev_out || !dev_streams || !dev_lens || n < 1 || (stream_stride & 7) || !stream_stride ||
		((uintptr_t)dev_out & 7) || ((uintptr_t)dev_streams & 7) || !dwtx_count_ok(n, DWTX_MAX_PLANES_PER_CALL, "streams to pack"))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	const unsigned pieces = (unsigned)((stream_stride + PK_PIECE - 1) / PK_PIECE);
	hipLaunchKernelGGL(k_pack_streams, dim3(pieces, n), dim3(PK_THREADS), 0, ctx->stream, dev_out, (unsigned long long)out_bytes, dev_offsets,
		dev_streams, (unsigned long long)stream_stride, dev_lens, n);
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// ---- host-buffer wrappers (what the CLIs call) ---------------------------------
// A batch is cut into parts of at most part_size() images.  Part k's kernels run on the context's
// stream while part k+1's input is on its way in and part k-1's output on its way out (a second
// stream, two device staging buffers each way): device memory stays bounded for any n, and with
// page-locked host buffers (dwtx_host_alloc) the PCIe transfers hide behind the kernels.

static int part_size(const dwtx_ctx *ctx, int W, int H, int C, int n)
{
	const size_t samples = (size_t)W * H * C;
	size_t p = ((size_t)64 << 20) / (samples ? samples : 1);   // about 64 M samples per part (16 frames of 4096x4096 gray)
	p = p < 4 ? 4 : p > 256 ? 256 : p;
	if (ctx->opt[DWTX_OPT_PART_IMAGES] > 0)   // test hook: force small parts
		p = (size_t)ctx->opt[DWTX_OPT_PART_IMAGES];
	return (size_t)n < p ? n : (int)p;
}

static int sync_all(dwtx_ctx *ctx)
{
	hipError_t a = hipStreamSynchronize(ctx->stream);
	hipError_t b = ctx->have_copy ? hipStreamSynchronize(ctx->copy) : hipSuccess;
	return a == hipSuccess && b == hipSuccess ? DWTX_OK : DWTX_ERR_DEVICE;
}

// host: the caller's pictures (host memory), dense
static int encode_images(dwtx_ctx *ctx, const dwtx_pixels &host, int W, int H, int n, long capacity,
	uint8_t *out, size_t out_stride, size_t *out_lens, dwtx_stats *stats)
{
	const int C = host.channels;
	if (!ctx || !host.base || !out || !out_lens || (out_stride & 7) || n < 1 || (C != 1 && C != 3))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	DWTX_CHECK_DIMS(W, H);
	const int P = part_size(ctx, W, H, C, n), parts = (n + P - 1) / P;
	int rc = dwtx_need_copy_stream(ctx);
	if (rc)
		return rc;
	const dwtx_pixels stage = host.moved(dwtx_scratch(ctx, SLOT_CD_IO, host.bytes(2 * host.image_stride * P)));   // [2][P] images
	uint8_t *dout = (uint8_t *)dwtx_scratch(ctx, SLOT_CD_IO2, 2 * out_stride * (size_t)P);
	dwtx_stream_info *dinfo = (dwtx_stream_info *)dwtx_scratch(ctx, SLOT_CD_LENS, 2 * sizeof(dwtx_stream_info) * (size_t)P);
	// sidecar indices (dwtx_ctx_set_encode_index; host memory here): a part's records are made on the device, their headers
	// come over with the part's info records, and drain() fetches what each holds — header and seg[0 .. nsegs)
	dwtx_index *hix = ctx->enc_index;
	dwtx_index *dix = hix ? (dwtx_index *)dwtx_scratch(ctx, SLOT_CD_INDEX, 2 * sizeof(dwtx_index) * (size_t)P) : nullptr;
	constexpr size_t ix_head = offsetof(dwtx_index, seg);
	const size_t hinfo_bytes = 2 * sizeof(dwtx_stream_info) * (size_t)P;
	dwtx_stream_info *hinfo = nullptr;   // page-locked: its copy must not block the host
	if (hipHostMalloc((void **)&hinfo, hinfo_bytes + (hix ? 2 * ix_head * (size_t)P : 0), hipHostMallocDefault) != hipSuccess)
		hinfo = nullptr;
	char *hhead = (char *)hinfo + hinfo_bytes;   // [2][P] index headers
	if (!stage.base || !dout || !dinfo || !hinfo || (hix && !dix)) {
		if (hinfo)
			(void)hipHostFree(hinfo);
		return DWTX_ERR_NOMEM;
	}
	hipStream_t ms = ctx->stream, cs = ctx->copy;
	hipEvent_t *ev_in = ctx->copy_ev.in, *ev_enc = ctx->copy_ev.coded, *ev_out = ctx->copy_ev.out;   // per staging slot
	hipError_t e = hipSuccess;
	rc = DWTX_OK;
	auto first_of = [&](int k) { return k * P; };
	auto count_of = [&](int k) { return k == parts - 1 ? n - k * P : P; };
	// part k's streams to the host, once its lengths are known
	auto drain = [&](int k) {
		const int slot = k & 1, i0 = first_of(k), cnt = count_of(k);
		const dwtx_stream_info *hi = hinfo + (size_t)slot * P;
		e = hipEventSynchronize(ev_enc[slot]);
		for (int i = 0; e == hipSuccess && rc == DWTX_OK && i < cnt; ++i) {
			if (hi[i].error) {
				dwtx_set_error("image %d needs more than 16 bit planes", i0 + i);
				rc = DWTX_ERR_ARG;
				break;
			}
			if (hi[i].nbytes > out_stride) {
				dwtx_set_error("image %d: stream of %llu bytes exceeds out_stride %zu", i0 + i, hi[i].nbytes, out_stride);
				rc = DWTX_ERR_CAPACITY;
				break;
			}
			out_lens[i0 + i] = (size_t)hi[i].nbytes;
			e = hipMemcpyAsync(out + out_stride * (i0 + i), dout + out_stride * ((size_t)slot * P + i), (size_t)hi[i].nbytes,
				hipMemcpyDeviceToHost, cs);
			if (hix) {
				dwtx_index &X = hix[i0 + i];
				memcpy(&X, hhead + ix_head * ((size_t)slot * P + i), ix_head);
				if (e == hipSuccess && X.nsegs > 0)
					e = hipMemcpyAsync(X.seg, dix[(size_t)slot * P + i].seg, sizeof(dwtx_seg_index) * (size_t)X.nsegs, hipMemcpyDeviceToHost, cs);
			}
			if (stats) {
				dwtx_stats &st = stats[i0 + i];
				st.meta_bits = (int)hi[i].meta_bits;                 // encode.c:175
				st.root_bits = (int)hi[i].root_bits;                 // encode.c:179
				st.total_bits = (int)hi[i].total_bits;               // encode.c:226 (int there too)
				st.kib = (int)((hi[i].nbytes + 512) / 1024);         // encode.c:228
				st.levels = 0;
				for (int c = 0; c < 3; ++c)
					st.planes[c] = hi[i].planes[c];
			}
		}
		if (e == hipSuccess)
			e = hipEventRecord(ev_out[slot], cs);
	};
	for (int k = 0; k < parts && e == hipSuccess && rc == DWTX_OK; ++k) {
		const int slot = k & 1, i0 = first_of(k), cnt = count_of(k);
		if (k >= 2) {
			e = hipStreamWaitEvent(cs, ev_enc[slot], 0);     // part k-2 has read this pixel buffer
			if (e == hipSuccess)
				e = hipStreamWaitEvent(ms, ev_out[slot], 0); // and its streams have left this output buffer
		}
		if (e == hipSuccess)
			e = hipMemcpyAsync(stage.image((size_t)slot * P).base, host.image(i0).base, host.bytes(host.image_stride * cnt),
				hipMemcpyHostToDevice, cs);
		if (e == hipSuccess)
			e = hipEventRecord(ev_in[slot], cs);
		if (e == hipSuccess)
			e = hipStreamWaitEvent(ms, ev_in[slot], 0);
		if (e != hipSuccess)
			break;
		rc = encode_device(ctx, stage.image((size_t)slot * P), W, H, cnt, capacity,
			dout + out_stride * (size_t)slot * P, out_stride, dinfo + (size_t)slot * P, dix ? dix + (size_t)slot * P : nullptr);
		if (rc)
			break;
		e = hipMemcpyAsync(hinfo + (size_t)slot * P, dinfo + (size_t)slot * P, sizeof(dwtx_stream_info) * (size_t)cnt,
			hipMemcpyDeviceToHost, ms);
		if (e == hipSuccess && dix)
			e = hipMemcpy2DAsync(hhead + ix_head * (size_t)slot * P, ix_head, dix + (size_t)slot * P, sizeof(dwtx_index), ix_head, (size_t)cnt,
				hipMemcpyDeviceToHost, ms);
		if (e == hipSuccess)
			e = hipEventRecord(ev_enc[slot], ms);
		if (k >= 1 && e == hipSuccess)
			drain(k - 1);   // overlaps part k's kernels
	}
	if (e == hipSuccess && rc == DWTX_OK)
		drain(parts - 1);
	const int s = sync_all(ctx);
	(void)hipHostFree(hinfo);
	if (e != hipSuccess || s) {
		dwtx_set_error("encode_images transfer -> %s", hipGetErrorString(e));
		return DWTX_ERR_DEVICE;
	}
	return rc;
}

extern "C" int dwtx_encode_images(dwtx_ctx *ctx, const uint8_t *pix, int W, int H, int C, int n, long capacity,
	uint8_t *out, size_t out_stride, size_t *out_lens, dwtx_stats *stats)
{
	return encode_images(ctx, dwtx_pixels8(pix, C, (size_t)W * H * C), W, H, n, capacity, out, out_stride, out_lens, stats);
}

extern "C" int dwtx_encode_images16(dwtx_ctx *ctx, const uint16_t *pix, int W, int H, int C, int n, long capacity,
	uint8_t *out, size_t out_stride, size_t *out_lens, dwtx_stats *stats)
{
	return encode_images(ctx, dwtx_pixels16(pix, C, (size_t)W * H * C), W, H, n, capacity, out, out_stride, out_lens, stats);
}

extern "C" int dwtx_encode_images_s16(dwtx_ctx *ctx, const int16_t *pix, int W, int H, int C, int n, long capacity,
	uint8_t *out, size_t out_stride, size_t *out_lens, dwtx_stats *stats)
{
	return encode_images(ctx, dwtx_pixels_s16(pix, C, (size_t)W * H * C), W, H, n, capacity, out, out_stride, out_lens, stats);
}

extern "C" int dwtx_decode_images(dwtx_ctx *ctx, const uint8_t *streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint8_t *pix, size_t pix_stride, int *outW, int *outH, int *outC)
{
	return dwtx_decode_images_info(ctx, streams, stream_stride, lens, n, pixels_max, pix, pix_stride, outW, outH, outC, nullptr);
}

// host: the caller's pixel slots (host memory); its channels are the streams' and are filled in here
static int decode_images(dwtx_ctx *ctx, const uint8_t *streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, dwtx_pixels host, int *outW, int *outH, int *outC, dwtx_decode_info *infos)
{
	if (!ctx || !streams || !lens || !host.base || !outW || !outH || !outC || n < 1 || (stream_stride & 7))
		return DWTX_ERR_ARG;
	if (!host.range_ok())
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	// decode.c:142-159: geometry comes from the first stream's header; all streams of a batch share it
	if (lens[0] < 6 || streams[0] != 'W' || (streams[1] != '5' && streams[1] != '6'))
		return DWTX_ERR_ARG;
	for (int i = 0; i < n; ++i)
		if (lens[i] > stream_stride) {
			dwtx_set_error("stream %d: %zu bytes do not fit the stream stride %zu", i, lens[i], stream_stride);
			return DWTX_ERR_ARG;
		}
	const int C = streams[1] == '6' ? 3 : 1;
	const int W = (streams[2] | (streams[3] << 8)) + 1, H = (streams[4] | (streams[5] << 8)) + 1;
	host.channels = C;
	DWTX_CHECK_DIMS(W, H);
	dwtx_geom g;
	dwtx_geometry(&g, W, H);
	int levels_max = -1;
	if (pixels_max >= 0) {   // decode.c:165-171
		levels_max = g.levels;
		while (levels_max > 0 && g.pixels[levels_max] > pixels_max)
			--levels_max;
	}
	const int P = part_size(ctx, W, H, C, n), parts = (n + P - 1) / P;
	const size_t img_samples = (size_t)W * H * C;
	int rc = dwtx_need_copy_stream(ctx);
	if (rc)
		return rc;
	uint8_t *dstr = (uint8_t *)dwtx_scratch(ctx, SLOT_CD_IO, 2 * stream_stride * (size_t)P + 64);
	dwtx_pixels stage = host.moved(dwtx_scratch(ctx, SLOT_CD_IO2, host.bytes(2 * img_samples * P)));   // [2][P] images, dense at full size
	stage.image_stride = img_samples;
	unsigned long long *dlens = (unsigned long long *)dwtx_scratch(ctx, SLOT_CD_LENS, 2 * sizeof(unsigned long long) * (size_t)P);
	unsigned long long *hl = (unsigned long long *)malloc(sizeof(unsigned long long) * (size_t)n);
	dwtx_decode_info *info = (dwtx_decode_info *)malloc(sizeof(dwtx_decode_info) * (size_t)n);
	if (!dstr || !stage.base || !dlens || !hl || !info) {
		free(hl);
		free(info);
		return DWTX_ERR_NOMEM;
	}
	for (int i = 0; i < n; ++i)
		hl[i] = lens[i];
	hipStream_t ms = ctx->stream, cs = ctx->copy;
	hipEvent_t *ev_in = ctx->copy_ev.in, *ev_dec = ctx->copy_ev.coded, *ev_out = ctx->copy_ev.out;   // per staging slot
	hipError_t e = hipSuccess;
	rc = DWTX_OK;
	auto count_of = [&](int k) { return k == parts - 1 ? n - k * P : P; };
	// part k's streams and lengths to the device (copy stream)
	auto feed = [&](int k) {
		const int slot = k & 1, i0 = k * P, cnt = count_of(k);
		if (k >= 2)
			e = hipStreamWaitEvent(cs, ev_dec[slot], 0);   // part k-2 has read this staging buffer
		if (e == hipSuccess)
			e = hipMemcpyAsync(dstr + stream_stride * (size_t)slot * P, streams + stream_stride * (size_t)i0, stream_stride * (size_t)cnt,
				hipMemcpyHostToDevice, cs);
		if (e == hipSuccess)
			e = hipMemcpyAsync(dlens + (size_t)slot * P, hl + i0, sizeof(unsigned long long) * (size_t)cnt, hipMemcpyHostToDevice, cs);
		if (e == hipSuccess)
			e = hipEventRecord(ev_in[slot], cs);
	};
	feed(0);
	for (int k = 0; k < parts && e == hipSuccess; ++k) {
		const int slot = k & 1, i0 = k * P, cnt = count_of(k);
		if (k + 1 < parts)
			feed(k + 1);   // travels while part k is decoded
		if (e == hipSuccess)
			e = hipStreamWaitEvent(ms, ev_in[slot], 0);
		if (e == hipSuccess && k >= 2)
			e = hipStreamWaitEvent(ms, ev_out[slot], 0);   // part k-2's pixels have left this buffer
		if (e != hipSuccess)
			break;
		ctx->index_base = (size_t)i0;   // sidecar index entries follow the images (dwtx_ctx_set_index)
		const int r = decode_device(ctx, dstr + stream_stride * (size_t)slot * P, stream_stride, dlens + (size_t)slot * P, W, H, cnt,
			levels_max, stage.image((size_t)slot * P), info + i0);
		ctx->index_base = 0;
		if (r) {
			rc = r;
			break;
		}
		e = hipEventRecord(ev_dec[slot], ms);
		if (e == hipSuccess)
			e = hipStreamWaitEvent(cs, ev_dec[slot], 0);
		for (int i = 0; e == hipSuccess && i < cnt; ++i) {
			const dwtx_decode_info &I = info[i0 + i];
			outC[i0 + i] = C;
			if (I.status) {
				outW[i0 + i] = outH[i0 + i] = 0;
				if (n == 1 && I.status == 2) {   // refused, not unreadable: the caller is told why
					dwtx_set_error("the stream claims more than 16 bit planes: damaged, refused (the reference would decode garbage)");
					rc = DWTX_ERR_ARG;
				} else {
					rc = n == 1 ? DWTX_ERR_IO : rc;   // decode.c:181,185: unreadable root/planes -> exit 1
				}
				continue;
			}
			const int lo = I.level + 1;
			if ((size_t)g.widths[lo] * g.heights[lo] * C > host.image_stride) {   // as dwtx_decode_device: nothing written past a slot
				dwtx_set_error("image %d: %dx%dx%d pixels do not fit the pixel stride %zu", i0 + i, g.widths[lo], g.heights[lo], C, host.image_stride);
				outW[i0 + i] = outH[i0 + i] = 0;
				rc = DWTX_ERR_ARG;
				break;
			}
			outW[i0 + i] = g.widths[lo];
			outH[i0 + i] = g.heights[lo];
			e = hipMemcpyAsync(host.image(i0 + i).base, stage.image((size_t)slot * P + i).base,
				host.bytes((size_t)outW[i0 + i] * outH[i0 + i] * C), hipMemcpyDeviceToHost, cs);
		}
		if (e == hipSuccess)
			e = hipEventRecord(ev_out[slot], cs);
		if (rc == DWTX_ERR_ARG)
			break;
	}
	const int s = sync_all(ctx);
	if (infos && e == hipSuccess && !s && (rc == DWTX_OK || rc == DWTX_ERR_IO || rc == DWTX_ERR_ARG))
		memcpy(infos, info, sizeof(dwtx_decode_info) * (size_t)n);
	free(hl);
	free(info);
	if (e != hipSuccess || s) {
		dwtx_set_error("decode_images transfer -> %s", hipGetErrorString(e));
		return DWTX_ERR_DEVICE;
	}
	return rc;
}

extern "C" int dwtx_decode_images_info(dwtx_ctx *ctx, const uint8_t *streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint8_t *pix, size_t pix_stride, int *outW, int *outH, int *outC, dwtx_decode_info *infos)
{
	return decode_images(ctx, streams, stream_stride, lens, n, pixels_max, dwtx_pixels8(pix, 0, pix_stride), outW, outH, outC, infos);
}

extern "C" int dwtx_decode_images16(dwtx_ctx *ctx, const uint8_t *streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, uint16_t *pix, size_t pix_stride, int maxval, int *outW, int *outH, int *outC, dwtx_decode_info *infos)
{
	return decode_images(ctx, streams, stream_stride, lens, n, pixels_max, dwtx_pixels16(pix, 0, pix_stride, maxval), outW, outH, outC, infos);
}

extern "C" int dwtx_decode_images_s16(dwtx_ctx *ctx, const uint8_t *streams, size_t stream_stride, const size_t *lens, int n,
	int pixels_max, int16_t *pix, size_t pix_stride, int minval, int maxval, int *outW, int *outH, int *outC, dwtx_decode_info *infos)
{
	return decode_images(ctx, streams, stream_stride, lens, n, pixels_max, dwtx_pixels_s16(pix, 0, pix_stride, minval, maxval), outW, outH, outC, infos);
}
