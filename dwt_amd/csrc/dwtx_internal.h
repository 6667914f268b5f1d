// dwtx_internal.h — shared internals of libdwtx (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/dwtx.h"

#define DWTX_SCRATCH_SLOTS 27
#define DWTX_PART_STREAMS 4   // parts a batch runs as at the most, one stream each
#define DWTX_ENC_PARTS DWTX_PART_STREAMS

struct dwtx_linplan;

// Streams: a context works on the caller's stream, on up to three side streams and on a copy stream, and no more
// (DESIGN 6).  A batch is cut into parts, and part k of the encoder (codec.hip) and of the decoder (unpack.hip) alike runs
// on dwtx_part_stream(ctx, k): the runtime maps streams onto a handful of hardware queues, and streams that share a queue
// run one after the other.  Events are members named after what has happened when they fire; the arrays among them
// have one event per part, or per staging slot of the host-buffer pipelines.
struct dwtx_ctx {
	int device;
	hipStream_t stream;
	bool own_stream;
	void *scratch[DWTX_SCRATCH_SLOTS];
	size_t scratch_bytes[DWTX_SCRATCH_SLOTS];
	dwtx_linplan *plans;   // per-geometry Hilbert block tables (linearize.hip)
	hipStream_t side[DWTX_PART_STREAMS - 1];   // the streams of parts 1.. (dwtx_need_part_streams)
	int nside;                                 // how many of them exist: 0, 1 or all; dec_ev exists with the first
	// decoder (unpack.hip): one part's serial token walk overlaps the other parts' parallel kernels.  start, cleared: the
	// bitmap clear's fork from the caller's stream and its end on side[0]; tables[k]: part k's chunk tables are queued (part
	// k + 1 builds its own; the last part records none); scattered[k]: part k's scatter is queued (k >= 1: the caller's stream goes on)
	struct { hipEvent_t start, cleared, tables[DWTX_PART_STREAMS], scattered[DWTX_PART_STREAMS]; } dec_ev;
	// dwtx_encode_device cuts a batch into parts that run on contexts of their own (stream + scratch each): one part's
	// memory-bound lifting overlaps the instruction-bound entropy stage of the part before (codec.hip)
	dwtx_ctx *enc_part[DWTX_ENC_PARTS];
	// start: the caller's stream when the call began; lifted[k]: part k's transform is queued; done[k]: part k is done
	struct { hipEvent_t start, lifted[DWTX_ENC_PARTS], done[DWTX_ENC_PARTS]; } enc_ev;
	bool have_enc_ev;
	// host-buffer wrappers: transfers of one part of a batch overlap the kernels of another (codec.hip).  Per staging slot:
	// its input has arrived, it is encoded / decoded, its output has left
	hipStream_t copy;
	struct { hipEvent_t in[2], coded[2], out[2]; } copy_ev;
	bool have_copy;        // copy and copy_ev exist
	const dwtx_index *index_in;   // dwtx_ctx_set_index: sidecar indices offered to / asked from the decode calls
	dwtx_index *index_out;
	size_t index_base;            // entry of the current call's first image (the host pipeline decodes a batch in parts)
	dwtx_index *enc_index;        // dwtx_ctx_set_encode_index: where the encode calls leave the sidecar indices of their streams
	long opt[DWTX_OPT_COUNT];     // dwtx_ctx_set_option: diagnostic switches (tests, tools), all 0 by default
	// the *_view_list calls (codec.hip): the window table's way to SLOT_CD_LIST.  A page-locked buffer of list_cap offsets that an
	// asynchronous copy reads after the call has returned; list_sent fires when the copy has read it, and the next listed call
	// waits for that — for its own predecessor's copy, never for the stream — before it fills the buffer again
	long long *list_host;
	size_t list_cap;
	hipEvent_t list_sent;
	bool have_list_sent;
};

// Every entry point that allocates, launches or copies makes the context's device the calling thread's current
// one first: a host that drives several contexts (one per GPU) from one thread gets its kernels and scratch on the
// right device.  On a single-GPU process it is one hipGetDevice().
int dwtx_enter(dwtx_ctx *ctx);
#define DWTX_ENTER(ctx)              \
	do {                             \
		const int rc_ = dwtx_enter(ctx); \
		if (rc_)                     \
			return rc_;              \
	} while (0)
#ifdef DWTX_DEBUG_HOOKS
// debug builds: every kernel-launching function checks that it runs on its context's device
int dwtx_debug_check_device(dwtx_ctx *ctx, const char *file, int line);
#endif

void dwtx_free_plans(dwtx_ctx *ctx);
// ctx.hip: the side streams that `parts` parts need, made on first use: one for two parts (or for the decoder's bitmap
// clear alone), all three beyond — a process that never runs big batches opens two streams, not four
int dwtx_need_part_streams(dwtx_ctx *ctx, int parts);
// the stream of part k: the caller's, then the side streams (the one place that maps parts to streams)
static inline hipStream_t dwtx_part_stream(const dwtx_ctx *ctx, int k) { return k == 0 ? ctx->stream : ctx->side[k - 1]; }
// ctx.hip: the encoder's part k: a context (made on first use) on dwtx_part_stream(ctx, k) with the parent's options
int dwtx_encoder_part(dwtx_ctx *ctx, int k, dwtx_ctx **part);
int dwtx_need_copy_stream(dwtx_ctx *ctx);   // creates ctx->copy / ctx->copy_ev on first use

void dwtx_set_error(const char *fmt, ...);
// grow-only per-slot device scratch; contents undefined after a grow
void *dwtx_scratch(dwtx_ctx *ctx, int slot, size_t bytes);

#define DWTX_HIP(call)                                                          \
	do {                                                                        \
		hipError_t e_ = (call);                                                 \
		if (e_ != hipSuccess) {                                                 \
			dwtx_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
			return DWTX_ERR_DEVICE;                                             \
		}                                                                       \
	} while (0)

#ifdef DWTX_DEBUG_HOOKS
#define DWTX_LAUNCH_CHECK()                                            \
	do {                                                               \
		if (dwtx_debug_check_device(ctx, __FILE__, __LINE__))          \
			return DWTX_ERR_DEVICE;                                    \
		DWTX_HIP(hipGetLastError());                                   \
	} while (0)
#else
#define DWTX_LAUNCH_CHECK() DWTX_HIP(hipGetLastError())
#endif

static inline int dwtx_cdiv(int a, int b) { return (a + b - 1) / b; }

// the maxval a deep decode is told (include/dwtx.h): what a 16-bit sample can hold
// (`whose`: what stands in front of the text, with its colon and blank)
static inline bool dwtx_maxval_ok(int maxval, const char *whose = "")
{
	if (maxval >= 1 && maxval <= 65535)
		return true;
	dwtx_set_error("%smaxval %d is outside 1..65535", whose, maxval);
	return false;
}
// the range a signed call is told (include/dwtx.h, dwtx_*_view_signed): what an int16_t sample can hold
static inline bool dwtx_range_ok(int minval, int maxval, const char *whose = "")
{
	if (minval >= -32768 && minval < maxval && maxval <= 32767)
		return true;
	dwtx_set_error("%srange [%d, %d]: signed samples need -32768 <= minval < maxval <= 32767", whose, minval, maxval);
	return false;
}

// The planes (images * channels) of one call: a dimension of most launches' grids (blockIdx.y / .z), which holds 65535, and
// what WinGrid's unsigned `first + i` (lift.hip) and the kernels' int plane indices count.  32-bit by design (DESIGN.md
// section 4.13): every entry point that takes a count refuses more, before it allocates or launches anything.  The
// decoder takes a third of it whatever the channels (its launches are sized for three planes per image).
#define DWTX_MAX_PLANES_PER_CALL 65535
static inline bool dwtx_count_ok(long count, long most, const char *what)
{
	if (count <= most)
		return true;
	dwtx_set_error("%ld %s in one call: at most %ld (the planes of a call are a grid dimension of its launches); split the batch", count, what, most);
	return false;
}

// Image sizes: sides of 8..DWTX_MAX_SIDE (above it the reference's own arithmetic overflows, include/dwtx.h), and the
// kernels' int indices want one plane (W*H) below 2^31 — which 32768 x 32768 = 2^30 always is; the check stays for
// whoever raises DWTX_MAX_SIDE (the reference itself indexes with int, encode.c:40 `channels*(width*y+x)`).
static inline bool dwtx_dims_ok(int W, int H)
{
	return W >= DWTX_MIN_LEN && H >= DWTX_MIN_LEN && W <= DWTX_MAX_SIDE && H <= DWTX_MAX_SIDE && (long)W * H <= 0x7fffffffL - 4096;
}
#define DWTX_CHECK_DIMS(W, H)                                                              \
	do {                                                                                    \
		if (!dwtx_dims_ok(W, H)) {                                                          \
			dwtx_set_error("unsupported image size %dx%d (8..%d per side)", W, H, DWTX_MAX_SIDE); \
			return DWTX_ERR_ARG;                                                            \
		}                                                                                   \
	} while (0)

// scratch slot assignment, for every file in one place
enum {
	SLOT_LIFT_A = 0, SLOT_LIFT_B,   // lift.hip
	SLOT_PK_CUM, SLOT_PK_SMALL, SLOT_PK_ENT, SLOT_PK_TOKBIG, SLOT_PK_TOK16, SLOT_PK_LUT, SLOT_PK_CHUNK, SLOT_PK_STAGE,   // pack.hip
	SLOT_UP_SMALL = 12, SLOT_UP_BITS, SLOT_UP_TILES, SLOT_UP_CHUNKS,   // unpack.hip
	SLOT_CD_A, SLOT_CD_B, SLOT_CD_INFO, SLOT_CD_IO, SLOT_CD_IO2, SLOT_CD_LENS, SLOT_CD_F16, SLOT_CD_INDEX, SLOT_CD_CROP, SLOT_CD_LIST, SLOT_CD_CARRY,   // codec.hip
};
static_assert(SLOT_CD_CARRY < DWTX_SCRATCH_SLOTS, "more scratch slots than dwtx_ctx has");

static inline size_t dwtx_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Host: typed tables one after the other in one scratch slot, each starting on a 256-byte boundary (the slot's size
// is rounded up to one too).  carve() calls fn(Carve &) twice: once to measure the slot (base null: only offsets
// move), then, once dwtx_scratch has it, to point every table into it.  Returns the slot, or null if it could not
// be had (the tables are then not set).
struct Carve {
	char *base;
	size_t off;
	template <class T> void take(T *&table, size_t count)
	{
		if (base)
			table = (T *)(base + off);
		off = dwtx_align_up(off + sizeof(T) * count, 256);
	}
};
template <class F> char *carve(dwtx_ctx *ctx, int slot, F &&fn)
{
	Carve c{ nullptr, 0 };
	fn(c);
	c.base = (char *)dwtx_scratch(ctx, slot, c.off);
	if (c.base) {
		c.off = 0;
		fn(c);
	}
	return c.base;
}

// A batch of pictures in memory (device memory, or the host buffers codec.hip stages them from / to): the
// reference's bytes, or deep pixels (include/dwtx.h: native-endian uint16_t samples).  The one place that knows how a
// sample offset becomes an address: everything that is counted here — the strides, the argument of at() — counts
// samples, whatever their size.  (A view of a source is only read; the view does not say which it is.)
// The pictures may be windows of a larger frame (include/dwtx.h, dwtx_view): rows row_pitch apart, the windows a grid of
// bands of `cols` each.  Window i of the view is window first + i of the grid, which starts at `base`.
// Or the windows lie wherever the caller's list says (offs, the *_view_list calls): window i of the view starts offs[first + i]
// samples after `base`, the lowest pointer of the list; cols, image_stride and band_stride then say nothing.
// RGB samples are interleaved, or planar (channel_stride != 0, views only: include/dwtx.h): three planes per window,
// columns one sample apart; the host-buffer pipelines and every dense entry point stay interleaved.
// Interleaved and gray pixels may lie further apart than their own samples (pixel_step, the *_view_step calls only): the
// RGB of an RGBA surface, its alpha, one plane of a mosaic — what lies between a pixel's samples and the next pixel is
// never written, and read only by lift.hip's Rgbx8 source (the fourth byte of a window's own 4-byte pixels, never used).
// The three channels may lie as B, G, R (order, the *_view_order calls only): base and every stride stay what they are — base
// is the lowest-addressed channel's first sample — and only lift.hip's last step to the kernels (red(), colour_stride())
// knows: no check and no choice of path looks at the order.
// A destination may hold floating-point samples (kind, dwtx_decode_view_float): what the integer sinks would write
// there, times scale plus bias per COLOUR, converted.  sample_bytes stays the addressing unit (4, or 2 for the half types);
// a float destination takes the 8-bit pixels' route through the pipelines whatever its maxval (deep() is false: 16-bit ring
// planes where the streams' plane counts allow them), with the clamp bound always passed along.
// A source may hold them too (dwtx_encode_view_float): the picture that is coded is rint(x * scale + bias) per COLOUR, two
// fp32 roundings, clamped to [0, maxval] (NaN: 0) — lift.hip's quant_of.  Up to a maxval of 255 those integers meet every
// bound of 8-bit samples and the source takes their route; above it the deep pictures' (deep_source()).
// Signed samples (the *_view_signed calls and the *_images_s16 pair): native-endian int16_t, coded as the integers they are;
// and float samples with a lower bound other than 0 (minval).  The inverse direction clamps gray, Y and every output sample
// to [minval, maxval] and Co, Cg to [-R, R], R = maxval - minval; the quantiser clamps to [minval, maxval].  Both take the
// deep pictures' route — no histograms from the transform, no 16-bit ring planes: those bounds are for samples in [0, 255] —
// through the wide kernels wherever a deep view of the same layout goes through them (lift.hip: the deep sources' signed twins,
// the deep and float sinks with the lower clamp), else through the general conversions, which know the bound too.
// A delta view (dwtx_encode_view_delta / dwtx_decode_view_delta) carries a second grid of windows, its base pictures (`delta`:
// where they lie; kind, channels, sample_bytes and order are the view's own): the picture that is coded is S - B on integers,
// the sample that is written min(max(B + d, minval), maxval) with d the residual under the signed clamps for [-R, R], R = maxval -
// minval.  A residual has twice its pictures' range, so a delta view takes the deep pictures' route whatever its sample size
// (deep() and deep_source() hold): through the wide kernels where both views qualify and are gray, or interleaved 8-bit RGB
// (lift.hip: the delta sources and sinks), else through the general conversions' delta instances, which take every pair of layouts.
enum dwtx_sample_kind { DWTX_SAMPLE_U8 = 0, DWTX_SAMPLE_U16, DWTX_SAMPLE_S16, DWTX_SAMPLE_F32, DWTX_SAMPLE_F16, DWTX_SAMPLE_BF16 };
// where the base pictures of a delta view lie: a grid of its own (dwtx_pixels' fields of the same names); base null: no delta view
struct dwtx_base_grid {
	void *base = nullptr;
	size_t image_stride = 0, row_pitch = 0, band_stride = 0, first = 0, channel_stride = 0, pixel_step = 0;
	int cols = 0;
	// the same windows: every field that places a sample is equal
	bool operator==(const dwtx_base_grid &o) const
	{
		return base == o.base && image_stride == o.image_stride && row_pitch == o.row_pitch && band_stride == o.band_stride && first == o.first &&
			channel_stride == o.channel_stride && pixel_step == o.pixel_step && cols == o.cols;
	}
};
struct dwtx_pixels {
	void *base;            // the grid's window 0, first sample
	int sample_bytes;      // 1 or 2; a float destination's 4 or 2 (kind says which samples they are)
	int channels;          // 1 gray, 3 RGB (interleaved unless channel_stride says otherwise)
	size_t image_stride;   // from a window to the next one of its band
	int maxval;            // 255 for bytes; a deep picture's own (what the inverse direction clamps at)
	int minval = 0;        // the lower bound beside it: 0 but for signed samples and the float views of the *_view_signed calls
	size_t row_pitch = 0;  // from a row to the next; 0: dense rows — the width a call works at (a reduced decode's own) times channels
	int cols = 0;          // windows per band; 0: one band
	size_t band_stride = 0;   // from a band's first window to the next band's
	size_t first = 0;      // the view's first window in the grid (parts of a batch start anywhere in it)
	size_t channel_stride = 0;   // 0: interleaved; else planar RGB: from a window's plane of one channel to the next one's (image() and moved() keep it)
	size_t pixel_step = 0;       // 0: dense (a pixel is its channels); else from a pixel to the next one of its row, above channels (image() and moved() keep it)
	int order = DWTX_ORDER_RGB;  // which colour the three channels are as they lie (DWTX_ORDER_*; image() and moved() keep it); gray pixels have none
	int kind = DWTX_SAMPLE_U8;   // dwtx_sample_kind (dwtx_pixels8 / dwtx_pixels16 / dwtx_pixels_s16 / dwtx_pixels_float set it with sample_bytes)
	float scale[3] = { 1.f, 1.f, 1.f }, bias[3] = { 0.f, 0.f, 0.f };   // float samples: per colour R, G, B (gray: [0])
	const long long *offs = nullptr;   // listed windows: DEVICE table of their first samples' offsets from base (>= 0), read-only while kernels run; image() and moved() keep it
	bool offs_on_quad = true;          // listed windows: every offset is a multiple of 4 (what wide() asks of each window beyond base)
	// flipped windows (the *_view_flip calls, always listed): entry i of offs carries window i's DWTX_FLIP_* flags in its top two
	// bits (DWTX_FLIP_SHIFT), which only lift.hip's general conversions and the FY instances of its wide forward kernels take
	// apart — dwtx_pixels_ok says no to every other kernel, so that none meets such an entry — and flip_w x flip_h are the
	// WINDOWS' sides: a picture that comes out reduced, or a part of a crop, is mirrored inside its window, not inside itself.
	// flip_wide: the view is an encode's SOURCE and no window carries DWTX_FLIP_X: the wide forward kernels may read it
	// flip_sink: the view is a decode's DESTINATION, which the FL instances of the wide inverse kernels write; flip_x: a window
	// of it carries DWTX_FLIP_X (those need the windows' width on the quad: a mirrored quad is one aligned access)
	bool flips = false, flip_wide = false, flip_sink = false, flip_x = false;
	int flip_w = 0, flip_h = 0;
	dwtx_base_grid delta;   // a delta view's base pictures, window for window (image() moves both grids; moved() keeps the base where it is)
	// A chain (dwtx_decode_view_chain): a delta view whose window i has window i - 1 of the view itself as its base, and window 0
	// the one window at `key` (its own pitch, channel stride and step; image_stride, band_stride, first and cols stay 0).  `delta`
	// stays empty: no kernel that walks two grids window for window meets a chain, whose one conversion (lift.hip,
	// dwtx_planes_to_pixels_chain) walks the windows of a group in order.  image() and moved() keep both fields.
	bool chain = false;
	dwtx_base_grid key;
	// A clip stack (the *_view_clips calls): a stack of chains with their keys inside it.  clips is the period (0: no clip stack):
	// window i of the STACK with i % clips == 0 is a key, coded as itself, every other one a link whose base is window i - 1 of the
	// view itself.  clip_at is the stack index of the view's window 0, which image() moves (a part of an encode starts anywhere in a
	// clip).  `delta` and `key` stay empty: like a chain, a clip stack never meets a kernel that walks two grids window for window;
	// its conversions (lift.hip: the clips instance of the forward delta conversion, dwtx_planes_to_pixels_clips) take the period.
	int clips = 0;
	size_t clip_at = 0;

	bool is_delta() const { return delta.base != nullptr || chain || clips; }
	// where the view's own windows lie, and the same samples on another grid: the one place that knows which fields are the layout
	dwtx_base_grid grid() const { return dwtx_base_grid{ base, image_stride, row_pitch, band_stride, first, channel_stride, pixel_step, cols }; }
	dwtx_pixels with_grid(const dwtx_base_grid &g) const
	{
		dwtx_pixels p = *this;
		p.base = g.base;
		p.image_stride = g.image_stride;
		p.row_pitch = g.row_pitch;
		p.band_stride = g.band_stride;
		p.first = g.first;
		p.channel_stride = g.channel_stride;
		p.pixel_step = g.pixel_step;
		p.cols = g.cols;
		return p;
	}
	// the key of a chain as a view of its own, one window
	dwtx_pixels key_pixels() const
	{
		dwtx_pixels p = with_grid(key);
		p.chain = false;
		p.key = dwtx_base_grid();
		return p;
	}
	// the base pictures as a view of their own: the samples, the channels and their order are this view's
	dwtx_pixels base_pixels() const
	{
		dwtx_pixels p = with_grid(delta);
		p.delta = dwtx_base_grid();
		return p;
	}
	// uint16_t or int16_t samples, or a delta view of any — and with them the kernel family that clamps at [minval, maxval] and keeps no 16-bit ring planes
	bool deep() const { return kind == DWTX_SAMPLE_U16 || kind == DWTX_SAMPLE_S16 || is_delta(); }
	bool is_float() const { return kind >= DWTX_SAMPLE_F32; }
	// int16_t samples, or a lower bound of their own: the range rule of the signed calls holds (range_ok)
	bool signed_range() const { return kind == DWTX_SAMPLE_S16 || minval != 0; }
	// as a SOURCE: the family whose forward transform keeps no histograms and no 16-bit ring planes (both bounds are for samples
	// in [0, 255]): uint16_t and int16_t samples, and floats that quantise to more than 255 or to less than 0
	bool deep_source() const { return deep() || (is_float() && (maxval > 255 || minval < 0)); }
	// what the inverse direction is told: maxval alone, or the range of a signed call
	bool range_ok() const { return signed_range() ? dwtx_range_ok(minval, maxval) : dwtx_maxval_ok(maxval); }
	size_t bytes(size_t samples) const { return samples * (size_t)sample_bytes; }
	void *at(size_t sample) const { return static_cast<char *>(base) + bytes(sample); }
	// typed for the kernels: u16() for deep pixels; u8() for bytes — and for the fields that carry either kind as bytes
	// (lift.hip's LevelArgs::src8 / dst8, whose kernels know which they were compiled for)
	uint8_t *u8() const { return static_cast<uint8_t *>(base); }
	uint16_t *u16() const { return static_cast<uint16_t *>(base); }
	bool listed() const { return offs != nullptr; }
	bool one_band() const { return cols == 0 && !listed(); }
	bool planar() const { return channel_stride != 0; }
	bool stepped() const { return pixel_step != 0; }
	bool bgr() const { return order == DWTX_ORDER_BGR && channels == 3; }
	// The colours of a pixel for kernels that walk R, G, B through a signed stride (planar pixels, and the general
	// conversions' interleaved ones): from a colour's sample to the next colour's, and the R sample of the grid's first pixel —
	// B, G, R pixels are walked down from their highest-addressed channel
	long colour_stride() const
	{
		const long cs = planar() ? (long)channel_stride : 1L;
		return bgr() ? -cs : cs;
	}
	void *red() const { return bgr() ? at(2 * (planar() ? channel_stride : (size_t)1)) : base; }
	// from a pixel to the next one of its row
	size_t step() const { return planar() ? 1 : pixel_step ? pixel_step : (size_t)channels; }
	// 8-bit RGB in 4-byte pixels (RGBA / RGBX surfaces): the one stepped layout lift.hip's wide kernels take
	bool rgbx8() const { return pixel_step == 4 && channels == 3 && sample_bytes == 1 && !planar(); }
	size_t pitch(int W) const { return row_pitch ? row_pitch : (size_t)W * (planar() ? 1 : channels); }
	// a row of a W-wide window (planar: of one of its planes), from its first sample to behind its last
	size_t row_samples(int W) const { return planar() ? (size_t)W : stepped() ? (size_t)(W - 1) * pixel_step + channels : (size_t)W * channels; }
	// where window i of a grid view starts, in samples from base
	size_t grid_offset(size_t i) const
	{
		const size_t w = first + i;
		return cols ? w / (size_t)cols * band_stride + w % (size_t)cols * image_stride : w * image_stride;
	}
	// the same pictures from image i on: a one-band view moves its base (first stays 0), a grid or a list keeps its origin and moves the index
	dwtx_pixels image(size_t i) const
	{
		dwtx_pixels p = *this;
		if (one_band())
			p.base = at(image_stride * i);
		else
			p.first += i;
		if (delta.base) {
			if (delta.cols == 0)
				p.delta.base = static_cast<char *>(delta.base) + bytes(delta.image_stride * i);
			else
				p.delta.first += i;
		}
		if (clips)
			p.clip_at += i;
		return p;
	}
	// the same layout somewhere else
	dwtx_pixels moved(void *to) const
	{
		dwtx_pixels p = *this;
		p.base = to;
		return p;
	}
	bool aligned(size_t a) const { return ((uintptr_t)base & (a - 1)) == 0; }
	bool sample_aligned() const { return aligned((size_t)sample_bytes); }
	// What lift.hip's wide kernels ask of the buffer when the finest level reads / writes the pixels itself: a lane's
	// quad of samples — 4 bytes, 8 of a deep picture or of half floats, 16 of fp32 (gray, and each plane of planar RGB;
	// interleaved RGB lanes take three) — is one aligned access in every row of every image
	bool wide() const
	{
		if (listed())   // (no grid: the strides between windows say nothing; every window's own pointer is on the quad instead)
			return row_pitch % 4 == 0 && channel_stride % 4 == 0 && aligned(4 * (size_t)sample_bytes) && offs_on_quad;
		return image_stride % 4 == 0 && row_pitch % 4 == 0 && band_stride % 4 == 0 && channel_stride % 4 == 0 && aligned(4 * (size_t)sample_bytes);
	}
};
constexpr int DWTX_FLIP_SHIFT = 62;   // a flipped window's flags in its 8-byte table entry; the offset is what lies below
static inline dwtx_pixels dwtx_pixels8(const uint8_t *pix, int channels, size_t image_stride)
{
	return dwtx_pixels{ const_cast<uint8_t *>(pix), 1, channels, image_stride, 255 };
}
static inline dwtx_pixels dwtx_pixels16(const uint16_t *pix, int channels, size_t image_stride, int maxval = 65535)
{
	dwtx_pixels p{ const_cast<uint16_t *>(pix), 2, channels, image_stride, maxval };
	p.kind = DWTX_SAMPLE_U16;
	return p;
}
// signed samples: coded as they are; minval and maxval are what the inverse direction clamps at
static inline dwtx_pixels dwtx_pixels_s16(const int16_t *pix, int channels, size_t image_stride, int minval = -32768, int maxval = 32767)
{
	dwtx_pixels p{ const_cast<int16_t *>(pix), 2, channels, image_stride, maxval };
	p.kind = DWTX_SAMPLE_S16;
	p.minval = minval;
	return p;
}
// a float destination or source (kind: DWTX_SAMPLE_F32 / _F16 / _BF16); the caller fills scale and bias
static inline dwtx_pixels dwtx_pixels_float(void *pix, int kind, int channels, size_t image_stride, int maxval)
{
	dwtx_pixels p{ pix, kind == DWTX_SAMPLE_F32 ? 4 : 2, channels, image_stride, maxval };
	p.kind = kind;
	return p;
}

// lift.hip: the finest lifting level reads / writes pixels itself (the widening of pnm.h:69-74, the clamp of pnm.h:108
// and, for RGB, the YCoCg-R colour transform of image.h:39-65 fused into it).  dwtx_pixels_ok says whether the shape and
// the buffer allow it: W % 4 == 0, more than 64 pixels on a side (the wide kernel, not the LDS tail), px.wide() (a planar
// picture's channel stride on the quad grid too), and windows the kernels can address (lift.hip).  Of the stepped views
// (dwtx_pixels::pixel_step) only 8-bit RGB in 4-byte pixels qualifies: every other one takes the general conversions.
// Of float views gray and planar RGB qualify, in both directions; interleaved float RGB takes the general way.
// Flipped windows (dwtx_pixels::flips) qualify as their unflipped twins do: a destination (flip_sink) with any flags — a mirrored
// window needs its width on the quad —, a source (flip_wide) unless one of its windows carries DWTX_FLIP_X.
// A delta view (dwtx_pixels::delta) qualifies when the view and its base each would, both are dense pixels (no step, not planar),
// and the pictures are gray — uint8_t, uint16_t or int16_t — or interleaved 8-bit RGB, in either order.
bool dwtx_pixels_ok(const dwtx_pixels &px, int W, int H);
// lift.hip: asks for the scratch planes every lifting call of a W*H transform over nplanes planes asks for
int dwtx_lift_scratch(dwtx_ctx *ctx, int W, int H, int nplanes);
// lift.hip: the general way between pixels and int32 planes [n*C][H][W] (pnm.h:69-74 / pnm.h:108, YCoCg-R if C == 3): what
// the extern "C" conversions of include/dwtx.h run, and every view the wide kernels do not take: one launch for the n
// windows, whatever their pitch, strides (a planar view's channel stride too) and grid; only the W*C samples of a window's H rows are read / written
int dwtx_pixels_to_planes(dwtx_ctx *ctx, int32_t *planes, const dwtx_pixels &px, int W, int H, int n);
int dwtx_planes_to_pixels(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int n);
// lift.hip: the one conversion of a chain (dwtx_pixels::chain; px is the whole view of the call): the planes of the residuals of
// windows first .. first + count, in order, onto window first - 1 as it lies in memory when the launch runs (first == 0: the
// key) — window i receives clamp(window i - 1 + d_i), the running sample kept in a register.  One launch, on ctx->stream.
int dwtx_planes_to_pixels_chain(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count);
// lift.hip: the one inverse conversion of a clip stack (dwtx_pixels::clips; px is the whole view of the call, clip_at 0): the planes
// of windows first .. first + count — a key's its own picture's, a link's its residual's — in ONE launch that walks the group's
// segments side by side: a key receives the plain conversion of its planes, a link clamp(window before + d).  A first segment that
// starts mid-clip reads window first - 1 as it lies in memory when the launch runs.  On ctx->stream.
int dwtx_planes_to_pixels_clips(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count);
// lift.hip: the same for a clip stack of FLOAT windows (dwtx_decode_view_clips_crop with a format; px.kind a float kind): every
// window of the group is written through the view's scale and bias, and the view is never read — a first segment that starts
// mid-clip takes its running integers from carry_in (int32 [C][H][W], required then), and where carry_out is given the launch's
// last segment leaves its own there.  The two are different pictures (the launch refuses one for both).  On ctx->stream.
int dwtx_planes_to_pixels_clips_float(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count,
	const int32_t *carry_in, int32_t *carry_out);

// The entropy stage's tiles (linearize.hip): the Hilbert curve of ring level l visits every aligned 32x32 square of
// its lengths[l+1]-sided square contiguously ("curve block"), so the ring's coefficients, in the order of
// encode.c:46-56, are the blocks' points one block after the other.  A tile is one non-empty curve block: `base` =
// ring index of its first coefficient, `cnt` = its coefficients (1024 for a block that lies wholly inside the ring),
// `blk` = the block's index on the curve.  Levels below 32x32 are one block each.  Tiles are numbered level by level.
// What the kernels read of a tile is one 16-byte record (built with the plan, once per geometry): everything that follows
// from (W, H, tile) alone, so that a wave finds its tile's facts with one load instead of a search over tile_first[], three
// table reads and the curve's recursion for the block (hilbert_dev.h square_map; unpacked by tile_rec there).
//   x: base    y: pixels[l] + base, the coefficient's place in a linearised plane (< 2^30)
//   z: cnt | l << DWTX_REC_LEVEL_SHIFT | swap << DWTX_REC_SWAP_SHIFT    w: mx | my << 16, square_map(lengths[l+1], blk)
struct dwtx_tile_rec {
	int base, at;
	unsigned info, masks;
};
static_assert(sizeof(dwtx_tile_rec) == 16, "a tile's record is one 16-byte load");
constexpr int DWTX_REC_LEVEL_SHIFT = 16, DWTX_REC_SWAP_SHIFT = 31;
static_assert(DWTX_MAX_SIDE <= (1 << 15), "a square map's XOR mask is below the curve's side: 16 bits each hold it");
static_assert(DWTX_MAX_LEVELS <= 16, "the record keeps the level in four bits");
struct dwtx_tiles {
	int NT;
	int tile_first[DWTX_MAX_LEVELS + 1];
	const dwtx_tile_rec *rec;     // device, [NT], 16-byte aligned
	const unsigned short *cnt;    // device, [NT]: the counts once more, dense (k_entries_count: a thread per entry reads nothing else of a tile)
	// block (bx, by) of level l's curve square (32x32 pyramid positions each, lengths[l+1] / 32 = nbs[l] blocks per side)
	// -> its tile, -1 for a block without ring coefficients: xy2tile[xy_first[l] + by * nbs[l] + bx]; levels below 64 have none
	const int *xy2tile;           // device
	int xy_first[DWTX_MAX_LEVELS + 1];
	int nbs[DWTX_MAX_LEVELS];
};

// Where the forward transform drops the tiles' magnitude histograms while it still holds the coefficients in registers
// (lift.hip k_fwd_level_w; what k_hist would otherwise read them from memory again for).  cum32: [plane][NT][16] words,
// word b of a tile = #(|v| < 2^(2b)) | #(|v| < 2^(2b+1)) << 16, zero before the transform adds to them; tile_mx:
// [plane][NTP] OR of the tile's magnitudes.
struct dwtx_hist_sink {
	unsigned *cum32;
	unsigned *tile_mx;
	int NT, NTP;
	dwtx_tiles tiles;
};
int dwtx_hist_begin(dwtx_ctx *ctx, int W, int H, int C, int n, dwtx_hist_sink *sink);   // pack.hip
// lift.hip: the forward transform with the histograms of the levels it can take (returned in *hist_levels, bit l = ring level l)
// p16 (optional, everywhere below): the detail coefficients of the ring levels in `levels` (a mask; the finest levels)
// are kept as 16-bit values in planes of their own — [n*C][H][W] int16, the positions of the pyramid — instead of in the
// int32 pyramid, whose positions for those rings are then never touched.  An 8-bit source cannot leave 16 bits on
// its finest ring (|HL|, |LH|, |HH| <= 1020: cdf53.h:13-21 on samples of magnitude <= 255) — three quarters of
// everything the entropy stage reads and writes; a decoder may keep every ring that way whose streams claim at most 15 bit planes.
struct dwtx_p16 {
	int16_t *planes;
	unsigned levels;
};
// The transforms whose finest level reads / writes the pixels itself; both need dwtx_pixels_ok(px, W, H), and image i of
// the inverse is written at px.image(i).  Deep pixels: int32 arithmetic and int32 bands; no histograms ride along
// (lift.hip hist_add) and no 16-bit ring planes — both bounds are for 8-bit sources, and a deep view with either is DWTX_ERR_ARG
// (dwtx_pixels::deep_source(): float sources that quantise beyond 255 among them).
int dwtx_fwd_pixels(dwtx_ctx *ctx, int32_t *out, const dwtx_pixels &px, int W, int H, int n, const dwtx_hist_sink *sink = nullptr,
	unsigned *hist_levels = nullptr, dwtx_p16 p16 = dwtx_p16{ nullptr, 0u });
int dwtx_inv_pixels(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *in, int W, int H, int n, const dwtx_p16 *p16 = nullptr);
int dwtx_transformation_fwd_hist(dwtx_ctx *ctx, int32_t *out, const int32_t *in, int W, int H, int nplanes, const dwtx_hist_sink *sink,
	unsigned *hist_levels);
// lift.hip: the inverse transform of a window of each picture (dwtx_decode_view_crop).  Plane t of a W x H transform (0: the
// picture, T: the root) is ws[t] x hs[t]; of it every picture of a call holds a w[t] x h[t] rectangle — the crop itself for
// t = 0, the whole plane from the LDS tail's first step on (t >= tail_from), in between what the finer rectangle's margins
// ask for, for either parity of its origin.  dwtx_crop_origins: where the rectangles of a picture whose crop starts at
// (x0, y0) start, xs / ys [T + 1].
struct dwtx_crop_steps {
	int T, tail_from;
	int ws[DWTX_MAX_LEVELS + 2], hs[DWTX_MAX_LEVELS + 2];
	int w[DWTX_MAX_LEVELS + 2], h[DWTX_MAX_LEVELS + 2];
};
int dwtx_crop_steps_of(int W, int H, int cw, int ch, dwtx_crop_steps *S);
void dwtx_crop_origins(const dwtx_crop_steps &S, int x0, int y0, int *xs, int *ys);
// pyramids [n*C][H][W] -> dense planes [n*C][ch][cw], *result: the cw x ch window at (x0, y0) of every picture, or — dev_org,
// device memory — at a place of its own for each: (x, y) pairs, the rectangle of picture i on plane t at dev_org[2 * (t *
// org_stride + i)], rows 0 .. tail_from (dwtx_crop_origins).  route 1: windowed levels above the LDS tail, into `planes`;
// route 2 (and any picture that is all tail): the whole inverse into `planes` [n*C][H][W], then a gather into `pyr`, which is
// dead by then.  Either way *result says where the window's planes are.
int dwtx_inv_crop(dwtx_ctx *ctx, int32_t *planes, int32_t *pyr, int W, int H, int n, int C, int cw, int ch,
	const int *dev_org, long org_stride, int x0, int y0, int route, const int32_t **result);
int dwtx_get_tiles(dwtx_ctx *ctx, int W, int H, dwtx_tiles *out);

// What the entropy stage's geometries (PackGeom in pack.hip, UnpackGeom in unpack.hip) share: sizes, rings and tiles,
// with no pyramid to read or write yet
template <class G> int dwtx_fill_geom(dwtx_ctx *ctx, int W, int H, int C, G &g, dwtx_tiles &tiles)
{
	int lengths[DWTX_MAX_LEVELS], pixels[DWTX_MAX_LEVELS], widths[DWTX_MAX_LEVELS], heights[DWTX_MAX_LEVELS];
	g.levels = dwtx_compute_lengths(lengths, pixels, widths, heights, W, H, DWTX_MIN_LEN);
	for (int l = 0; l <= g.levels; ++l)
		g.pixels[l] = pixels[l];
	g.C = C;
	g.W = W;
	g.H = H;
	g.total = (long)W * H;
	g.pyr = nullptr;
	g.fine16 = nullptr;
	g.lv16 = 0u;
	g.sq_levels = 0;
	const int rc = dwtx_get_tiles(ctx, W, H, &tiles);
	if (rc)
		return rc;
	for (int l = 0; l <= g.levels; ++l)
		g.tile_first[l] = tiles.tile_first[l];
	g.tile_rec = tiles.rec;
	return DWTX_OK;
}

// Tiles straight from / to the pyramid (hilbert_dev.h): on the ring levels in the mask, tiles that are whole 32x32
// squares need no linearised copy — the entropy stage reads (pack.hip) / writes (unpack.hip) them in the pyramid itself;
// only the blocks the ring's edges cut (image border, LL quadrant) still go through `lin`.
unsigned dwtx_square_levels(int W, int H);
// lift.hip: the finest ring levels that may live in 16-bit planes: whole squares read / written in place (in sq_levels)
// and transformed by the 16-byte-per-lane lifting kernels, as many as those allow; 0 if the finest one does not qualify
unsigned dwtx_levels16(int W, int H, unsigned sq_levels);
int dwtx_linearization_ex(dwtx_ctx *ctx, int32_t *lin, const int32_t *pyr, int W, int H, int nplanes, unsigned skip_levels,
	dwtx_p16 p16 = dwtx_p16{ nullptr, 0u });
int dwtx_reconstruction_ex(dwtx_ctx *ctx, int32_t *pyr, const int32_t *lin, const int *dev_missing, int levels_out, int W, int H,
	int C, int n, unsigned skip_levels, dwtx_p16 p16 = dwtx_p16{ nullptr, 0u });
// hist_levels: ring levels whose tile histograms the forward transform has already written (dwtx_hist_begin)
// dev_index (optional, device memory): entry i receives the sidecar index of image i's stream
int dwtx_encode_planes_ex(dwtx_ctx *ctx, const int32_t *lin, const int32_t *pyr, unsigned sq_levels, unsigned hist_levels, int W, int H, int C, int n,
	long capacity, uint8_t *out, size_t out_stride, dwtx_stream_info *dev_info, dwtx_p16 p16 = dwtx_p16{ nullptr, 0u },
	dwtx_index *dev_index = nullptr);

// unpack.hip: dwtx_decode_planes with a host callback per finished part of the batch (see there)
// `pyr` (optional): pyramid planes [n*C][H][W]; for parts of the batch that decode at full resolution the tiles of
// the full-square ring levels are written there (bias included) and `done` is told which levels (fused_levels).
constexpr unsigned DWTX_FUSED_FINE16 = 1u << 31;   // in `fused_levels`: the part's rings of p16.levels were written to the 16-bit planes, not to pyr
int dwtx_decode_planes_ex(dwtx_ctx *ctx, int32_t *lin, int32_t *pyr, const uint8_t *streams, size_t stream_stride,
	const unsigned long long *dev_lens, int W, int H, int C, int n, int levels_max, dwtx_decode_info *host_info,
	int (*done)(void *user, int first, int count, unsigned fused_levels), void *user, dwtx_p16 p16 = dwtx_p16{ nullptr, 0u });

// The wave's lanes for which `pred` holds.  (HIP's __ballot() takes an int: the condition would be turned
// into 0/1 in a register and compared again — two extra instructions per use in the ballot-heavy kernels.)
__device__ __forceinline__ unsigned long long ballot64(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// The wave's index inside its workgroup, as a SCALAR.  The compiler takes threadIdx.x >> 6 for a per-lane value, so what a
// wave-per-item kernel derives from it (its tile, its LDS slice, every branch and table look-up on them) would stay in vector
// registers under exec masks although no lane differs; readfirstlane says that it is one value.  That rests on one-dimensional
// workgroups (threadIdx.y == threadIdx.z == 0) and wave64: lanes 64k .. 64k+63 of a workgroup are one wave, so all the lanes
// of a wave share threadIdx.x >> 6, whichever of them are active and however long the workgroup's last wave is.  Every launch
// of a kernel that calls this is dim3(N) or a plain thread count.
__device__ __forceinline__ int wave_in_block() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// C truncating division by 2 and 4 on the device (cdf53.h:13,20 use `/`)
__device__ __forceinline__ int tdiv2(int a) { return (a + (int)((unsigned)a >> 31)) >> 1; }
__device__ __forceinline__ int tdiv4(int a) { return (a + ((a >> 31) & 3)) >> 2; }
