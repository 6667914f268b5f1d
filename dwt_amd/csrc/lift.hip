// lift.hip — colour transform at the image edge and the multi-level 2-D CDF 5/3
// integer lifting transform (forward: encode.c:16-30 over cdf53.h:9-34; inverse:
// decode.c:16-30 over cdf53.h:36-61) as streaming gfx950 kernels.
//
// Layout: planar int32, plane p = image*C + channel, dense rows; the finest level can
// also read / write 8-bit pixels directly (gray or interleaved RGB with YCoCg-R fused).
//
// Kernel shape (one level, both directions): a 64-lane wave owns 64 adjacent
// column PAIRS (x = 2k, 2k+1) and walks down a strip of row pairs.  The
// horizontal lifting step is done in registers with wave shuffles (the pair to
// the left supplies its detail value, the pair to the right its even sample),
// the vertical step is a 3-row sliding window held in registers.  No LDS, no
// re-reads: every input sample is loaded once per level (plus a 2+1 row halo
// per strip) and every output written once, each as a coalesced row segment.
//
// Edge rules (cdf53.h:13-21), expressed so the interior formula
// covers them:
//   predict at the last odd sample of an even-length line: x[N] := x[N-2]
//   update at sample 0: d[-1] := d[0]      (tdiv(2a,4) == tdiv(a,2))
//   odd-length line: the last even sample is NOT updated (not symmetric!)
#include "dwtx_internal.h"
#include <type_traits>

#include <stdlib.h>

namespace {

constexpr int WAVES = 4;          // waves per block, stacked along y
// The wide forward kernel: 2^wx_log2 of a block's waves sit side by side, the rest on top of each other.  Side by side
// the strips' left / right halo columns are lines the neighbour wave on the same CU loads at the same time, and a block
// reads rows of up to 4 KB in one piece: forward 34.1 -> 31.9 us per 4096x4096 int32 plane, the RGB finest level 2.93 ->
// 2.31 ms per 256 frames of 1080p on two of three boxes, no change on the third (never slower).  (The inverse, whose waves overlap by eight lanes instead of loading halo columns,
// loses with the same arrangement — 36.1 -> 39.8 us — and keeps its four waves stacked.)
constexpr int MAX_ROWS_PER_WAVE = 64; // output row pairs per wave strip (fewer on small levels, to keep the chip full); 64 instead of 32: half the halo rows, forward 37 -> 34.5 us per 4096x4096 plane

// Where the pictures of a launch that reads / writes pixels lie when they are windows of a larger frame (dwtx_pixels):
// picture i is window first + i of a grid of bands of `cols` windows, the windows of a band `ps` samples apart (the
// launch's src_ps / ll_ps / dst_ps), the bands band_ps.  cols == 0: one band, picture i at i * ps as ever.  Or, offs set,
// picture i is window first + i of a list (dwtx_pixels::offs): offs[first + i] samples from the origin, whatever ps says.
struct WinGrid {
	unsigned cols, first;
	long band_ps;
	const long long *offs;   // device memory that no launch writes: [first + pictures of the launch]
};

// The one place the kernels take a window's first sample from: its offset from the grid's origin, in samples.  The
// picture's index is the same for a whole wave, so the division is scalar arithmetic (readfirstlane says so where the
// index was computed from a vector register), and a one-band launch pays a compare for it.
// A list's offset is one 8-byte load at a wave-uniform index of a table that no kernel writes while a launch reads it: read
// through a pointer to the constant address space (memory that does not change during a kernel), with the index from
// readfirstlane, it is a scalar load at every site, beside kernels that store through pointers of their own too (DESIGN.md
// section 4.18: with a plain const __restrict__ pointer 28 of the sites kept a vector load per lane).
__device__ __forceinline__ long win_off(const WinGrid &g, long ps, int image)
{
	if (g.cols == 0 && !g.offs)   // (the one-band launch first: it pays two scalar compares and nothing else)
		return image * ps;
	const unsigned i = (unsigned)__builtin_amdgcn_readfirstlane(image) + g.first;   // (both below 65536: a call's windows, dwtx_count_ok)
	if (g.offs) {
		typedef const long long __attribute__((address_space(4))) *ConstTable;
		return (long)((ConstTable)g.offs)[i];
	}
	const unsigned band = i / g.cols;
	return (long)band * g.band_ps + (long)(i - band * g.cols) * ps;
}

// A flipped call's window (the *_view_flip calls; dwtx_pixels::flips): the same scalar load of the same table, whose entry
// carries the window's DWTX_FLIP_* flags above DWTX_FLIP_SHIFT.  Only the FLIP instances of the general conversions call
// it and the FY instances of the wide forward kernels call it, and only their launches see such a table (dwtx_pixels_ok).
__device__ __forceinline__ long win_off_flip(const WinGrid &g, int image, unsigned &flags)
{
	typedef const unsigned long long __attribute__((address_space(4))) *ConstTable;
	const unsigned i = (unsigned)__builtin_amdgcn_readfirstlane(image) + g.first;
	const unsigned long long e = ((ConstTable)g.offs)[i];
	flags = (unsigned)(e >> DWTX_FLIP_SHIFT);
	return (long)(e & ((1ull << DWTX_FLIP_SHIFT) - 1));
}

// A destination window as a wave of an inverse kernel that writes pixels finds it.  FL 0: win_off, today's code.  FL 1 and 2, the
// instances for a flipped call's windows: the entry's offset and flags; a bottom-up window
// (DWTX_FLIP_Y) starts at its last row in memory — row fh - 1 of the WINDOW, so that a reduced picture lies in its bottom rows
// — with the pitch negated.  FL 2 alone looks at DWTX_FLIP_X: a mirrored window's quad q goes to quad fwq - 1 - q with its four
// pixels reversed (flip_quad, flip_q).  -> the offset of the picture's row 0 in samples; pitch and fx are the wave's.
template <int FL>
__device__ __forceinline__ long flip_dst(const WinGrid &g, long ps, int image, int fh, int &pitch, bool &fx)
{
	fx = false;
	if constexpr (FL == 0) {
		return win_off(g, ps, image);
	} else {
		unsigned flags;
		long off = win_off_flip(g, image, flags);
		if (flags & DWTX_FLIP_Y) {
			off += (long)(fh - 1) * pitch;
			pitch = -pitch;
		}
		fx = FL == 2 && (flags & DWTX_FLIP_X) != 0;
		return off;
	}
}

struct LevelArgs {
	const int *src;  long src_ps;  int spitch;  // forward: input w*h      | inverse: LL (w2*h2)
	int *ll;         long ll_ps;   int llpitch; // forward: LL out (w2*h2) | inverse: output w*h
	int *det;        long det_ps;  int dpitch;  // Mallat pyramid: HL at (w2+x, y), LH at (x, h2+y), HH at (w2+x, h2+y)
	int w, h, w2, h2;
	int rpw;          // output row pairs per wave strip
	const uint8_t *src8;   // forward, finest level of a gray image: 8-bit pixels instead of src (pnm.h:69-74 widening fused)
	uint8_t *dst8;         // inverse, finest level of a gray image: clamped 8-bit pixels instead of ll (pnm.h:108 fused)
	short *det16;          // or null: this level's detail bands live here as 16-bit values (same positions, pitch and plane stride as det)
	const short *src16;    // forward, or null: the input band as 16-bit values (pitch and plane stride of src)
	short *ll16;           // forward, or null: the LL band goes out as 16-bit values (pitch and plane stride of ll)
	int maxval;            // deep pixels (uint16_t samples behind src8 / dst8, strides in samples): the inverse's clamps; 0 = 8-bit pixels
	WinGrid grid;          // the windows behind src8 / dst8 (src_ps / ll_ps apart in a band)
	int minval;            // the lower bound beside maxval (dwtx_pixels::minval): 0 but for int16_t samples behind dst8 and float views of the *_view_signed calls
};

// What a sink clamps at (image.h:41-43, pnm.h:108): gray, Y and every sample written to [lo, hi], Co and Cg to [-r(), r()] — with
// lo = 0 the unsigned pixels' [0, maxval] and [-maxval, maxval].  The 8-bit sinks are handed constants and read none of it.
struct Clamp {
	int lo, hi;
	__device__ __forceinline__ int r() const { return hi - lo; }
};
__device__ __forceinline__ Clamp clamp_of(const LevelArgs &a) { return Clamp{ a.minval, a.maxval }; }
__device__ __forceinline__ int clamp_to(int v, int lo, int hi)
{
	return v < lo ? lo : v > hi ? hi : v;
}
// a delta sink's sample: the residual v under the clamp of [-R, R], R = hi - lo, onto the base's sample b, the sum clamped to the range
__device__ __forceinline__ int delta_sample(int v, int b, Clamp M)
{
	return clamp_to(b + clamp_to(v, -M.r(), M.r()), M.lo, M.hi);
}

// ---- the colour transform, once: every source and sink of RGB pixels in this file calls these ----
// image.h:52-65 rgb2ycocg, reversible on any int: output ch of it — 0 Y, 1 Co, 2 Cg.  A wave of the wide forward kernels works on
// one plane and asks with its (uniform) channel, so that what the other channels alone need is not evaluated; ycocg_of is the
// whole triple, in which the compiler finds the three calls' common terms.
__device__ __forceinline__ int ycocg_ch(int r, int g, int b, int ch)
{
	const int co = r - b;
	if (ch == 1)
		return co;
	const int t = b + tdiv2(co);
	const int cg = g - t;
	return ch == 2 ? cg : t + tdiv2(cg);
}
__device__ __forceinline__ void ycocg_of(int r, int g, int b, int &y, int &co, int &cg)
{
	y = ycocg_ch(r, g, b, 0);
	co = ycocg_ch(r, g, b, 1);
	cg = ycocg_ch(r, g, b, 2);
}
// image.h:39-50 ycocg2rgb without its clamps
__device__ __forceinline__ void rgb_of_ycocg(int y, int co, int cg, int &r, int &g, int &b)
{
	const int t = y - tdiv2(cg);
	g = cg + t;
	b = t - tdiv2(co);
	r = b + co;
}
// The two front ends of the inverse.  Both read Y, Co and Cg at src[0], src[step] and src[2 * step] — planes in memory, or a lane's
// three registers with step 1 — each just before its clamp, and hand on one colour after the other: the form in which every caller
// keeps the registers it had (a by-value form cost the general conversions one each).
// The plain regime (a picture's own samples; image.h:41-43 and pnm.h:108 with M for [0, 255]): Y to [lo, hi], Co and Cg to
// [-R, R], the inverse, each colour to [lo, hi]; out(c, sample) receives colour c = 0, 1, 2 (R, G, B).
template <class Out>
__device__ __forceinline__ void rgb_plain(const int *src, long step, Clamp M, Out &&out)
{
	const int R = M.r();
	const int y = clamp_to(src[0], M.lo, M.hi);
	const int co = clamp_to(src[step], -R, R);
	const int cg = clamp_to(src[2 * step], -R, R);
	int r, g, b;
	rgb_of_ycocg(y, co, cg, r, g, b);
	out(0, clamp_to(r, M.lo, M.hi));
	out(1, clamp_to(g, M.lo, M.hi));
	out(2, clamp_to(b, M.lo, M.hi));
}
// The residual regime (a delta view's, a chain's or a clip's link: the planes hold S - B, whose range is [-R, R]): Y to [-R, R],
// Co and Cg to [-2R, 2R], the inverse, then each colour as delta_sample onto the base's colour — r, g, b: the base in, the sample out.
__device__ __forceinline__ void rgb_residual(const int *src, long step, Clamp M, int &r, int &g, int &b)
{
	const int R = M.r();
	const int y = clamp_to(src[0], -R, R);
	const int co = clamp_to(src[step], -2 * R, 2 * R);
	const int cg = clamp_to(src[2 * step], -2 * R, 2 * R);
	int dr, dg, db;
	rgb_of_ycocg(y, co, cg, dr, dg, db);
	r = delta_sample(dr, r, M);
	g = delta_sample(dg, g, M);
	b = delta_sample(db, b, M);
}
// (the same two for a lane that holds Y, Co and Cg of a pixel in registers: the wide inverse kernels' rows)
__device__ __forceinline__ void rgb_plain(int y, int co, int cg, Clamp M, int &r, int &g, int &b)
{
	const int v[3] = { y, co, cg };
	int o[3];
	rgb_plain(v, 1, M, [&](int c, int s) { o[c] = s; });
	r = o[0];
	g = o[1];
	b = o[2];
}
__device__ __forceinline__ void rgb_residual(int y, int co, int cg, Clamp M, int &r, int &g, int &b)
{
	const int v[3] = { y, co, cg };
	rgb_residual(v, 1, M, r, g, b);
}

// A float destination (dwtx_pixels::kind): scale and bias per COLOUR — R, G, B, whatever the order the channels lie in; gray
// uses [0] — and which of the two 16-bit types a Half16 sink writes (the two differ in the convert only: one kernel for both)
struct FloatFmt {
	float scale[3], bias[3];
	int bf16;
	int sext;   // the fp32 planar sink's rows wait as 16-bit integers: negative ones among them (minval < 0), to be widened with their sign
};

// ---------------------------------------------------------------- forward ---

struct FwdLane {
	int k;            // pair index
	int lane;
	bool valid;       // 2k   < w
	bool has_odd;     // 2k+1 < w
	bool right_in;    // 2k+2 < w
	bool frozen;      // w odd and 2k == w-1: even sample passes through
};

// horizontal lifting of one input row for this lane's pair -> (low, high)
__device__ __forceinline__ void fwd_row(const int *__restrict__ row, const FwdLane &L, int &lo, int &hi)
{
	int x0 = L.valid ? row[2 * L.k] : 0;
	int x1 = L.has_odd ? row[2 * L.k + 1] : 0;
	int xr = __shfl_down(x0, 1);
	if (L.lane == 63 && L.right_in)
		xr = row[2 * L.k + 2];
	if (!L.right_in)
		xr = x0;
	int d = x1 - tdiv2(x0 + xr);
	int dl = __shfl_up(d, 1);
	if (L.lane == 0 && L.k > 0) {
		int xm2 = row[2 * L.k - 2], xm1 = row[2 * L.k - 1];
		dl = xm1 - tdiv2(xm2 + x0);
	}
	if (L.k == 0)
		dl = d;
	lo = L.frozen ? x0 : x0 + tdiv4(dl + d);
	hi = d;
}

__global__ __launch_bounds__(64 * WAVES) void k_fwd_level(LevelArgs a)
{
	FwdLane L;
	L.lane = threadIdx.x & 63;
	const int wv = wave_in_block();
	L.k = blockIdx.x * 64 + L.lane;
	const int j0 = (blockIdx.y * WAVES + wv) * a.rpw;
	if (j0 >= a.h2)
		return;
	const int j1 = min(j0 + a.rpw, a.h2);
	const int plane = blockIdx.z;
	L.valid = 2 * L.k < a.w;
	L.has_odd = 2 * L.k + 1 < a.w;
	L.right_in = 2 * L.k + 2 < a.w;
	L.frozen = (a.w & 1) && 2 * L.k == a.w - 1;

	const int *src = a.src + plane * a.src_ps;
	int *ll = a.ll + plane * a.ll_ps;
	int *det = a.det + plane * a.det_ps;

	int jj = j0 > 0 ? j0 - 1 : 0;
	int l0, h0;              // even row 2jj
	int pl = 0, ph = 0;      // vertical detail of the previous row pair
	fwd_row(src + (long)(2 * jj) * a.spitch, L, l0, h0);
	for (; jj < j1; ++jj) {
		const int r1 = 2 * jj + 1, r2 = r1 + 1;
		const bool odd_in = r1 < a.h;
		int l1 = 0, h1 = 0, l2 = l0, h2v = h0;
		if (odd_in)
			fwd_row(src + (long)r1 * a.spitch, L, l1, h1);
		if (r2 < a.h)
			fwd_row(src + (long)r2 * a.spitch, L, l2, h2v);
		const int dl = l1 - tdiv2(l0 + l2);
		const int dh = h1 - tdiv2(h0 + h2v);
		if (jj >= j0) {
			int sl = l0, sh = h0;
			if (odd_in) {    // an odd-height plane leaves its last even row untouched
				sl += tdiv4((jj ? pl : dl) + dl);
				sh += tdiv4((jj ? ph : dh) + dh);
			}
			if (L.valid)
				ll[(long)jj * a.llpitch + L.k] = sl;
			if (L.has_odd)
				det[(long)jj * a.dpitch + a.w2 + L.k] = sh;
			if (odd_in) {
				if (L.valid)
					det[(long)(a.h2 + jj) * a.dpitch + L.k] = dl;
				if (L.has_odd)
					det[(long)(a.h2 + jj) * a.dpitch + a.w2 + L.k] = dh;
			}
		}
		pl = dl;
		ph = dh;
		l0 = l2;
		h0 = h2v;
	}
}

// ---------------------------------------------------------------- inverse ---
//
// Columns are undone first, rows last (decode.c:21-29), so the horizontal step
// needs its neighbours' values AFTER their vertical step.  Each wave therefore
// carries one halo pair on either side: lane i works on pair kb-1+i, lanes
// 1..62 produce output (62 pairs = 124 columns per wave).

constexpr int INV_PAIRS = 62;
// wide inverse: 56 quads of output per wave = 896 bytes per row = seven whole 128-byte lines, so the
// row stores of neighbouring waves never share a line (lanes 0 and 57 are the halo, 58-63 idle)
constexpr int INV_QUADS = 56;

struct InvLane {
	int k;
	bool valid;      // 0 <= k and 2k < w
	bool has_odd;    // valid and 2k+1 < w
	bool right_in;   // 2k+2 < w
	bool frozen;     // w odd and 2k == w-1
	bool writes;     // lanes 1..62 and valid
};

// horizontal inverse of one row: (low, high) of this pair -> samples 2k, 2k+1
__device__ __forceinline__ void inv_row(int *__restrict__ row, const InvLane &L, int lo, int hi)
{
	int hl = __shfl_up(hi, 1);
	if (L.k <= 0)
		hl = hi;
	const int e = L.frozen ? lo : lo - tdiv4(hl + hi);
	int er = __shfl_down(e, 1);
	if (!L.right_in)
		er = e;
	const int o = hi + tdiv2(e + er);
	if (L.writes) {
		row[2 * L.k] = e;
		if (L.has_odd)
			row[2 * L.k + 1] = o;
	}
}

__global__ __launch_bounds__(64 * WAVES) void k_inv_level(LevelArgs a)
{
	InvLane L;
	const int lane = threadIdx.x & 63;
	const int wv = wave_in_block();
	L.k = blockIdx.x * INV_PAIRS - 1 + lane;
	const int j0 = (blockIdx.y * WAVES + wv) * a.rpw;
	if (j0 >= a.h2)
		return;
	const int j1 = min(j0 + a.rpw, a.h2);
	const int plane = blockIdx.z;
	L.valid = L.k >= 0 && 2 * L.k < a.w;
	L.has_odd = L.k >= 0 && 2 * L.k + 1 < a.w;
	L.right_in = 2 * L.k + 2 < a.w;
	L.frozen = (a.w & 1) && 2 * L.k == a.w - 1;
	L.writes = L.valid && lane >= 1 && lane <= INV_PAIRS;

	const int *llp = a.src + plane * a.src_ps;
	const int *det = a.det + plane * a.det_ps;
	int *dst = a.ll + plane * a.ll_ps;
	const int kk = L.k < 0 ? 0 : L.k;

	// s/d of the current pair j, detail of pair j-1, even output row of pair j
	int sl, sh, dl = 0, dh = 0, pdl = 0, pdh = 0;
	int el, eh;
	const bool h_odd = a.h & 1;

	auto fetch = [&](int j, int &fsl, int &fsh, int &fdl, int &fdh) {
		fsl = L.valid ? llp[(long)j * a.spitch + kk] : 0;
		fsh = L.has_odd ? det[(long)j * a.dpitch + a.w2 + kk] : 0;
		const bool d_in = 2 * j + 1 < a.h;
		fdl = (d_in && L.valid) ? det[(long)(a.h2 + j) * a.dpitch + kk] : 0;
		fdh = (d_in && L.has_odd) ? det[(long)(a.h2 + j) * a.dpitch + a.w2 + kk] : 0;
	};

	// even row of pair j from s[j], d[j-1], d[j]
	auto even_of = [&](int j, int s, int dprev, int dcur) {
		if (h_odd && 2 * j == a.h - 1)
			return s;
		return s - tdiv4((j ? dprev : dcur) + dcur);
	};

	if (j0 > 0) {
		int t0, t1;
		fetch(j0 - 1, t0, t1, pdl, pdh);
	}
	fetch(j0, sl, sh, dl, dh);
	el = even_of(j0, sl, pdl, dl);
	eh = even_of(j0, sh, pdh, dh);
	for (int jj = j0; jj < j1; ++jj) {
		const int r0 = 2 * jj, r1 = r0 + 1;
		int nsl = 0, nsh = 0, ndl = 0, ndh = 0;
		int nel = el, neh = eh;          // mirror: x[h] := x[h-2]
		if (r1 + 1 < a.h) {
			fetch(jj + 1, nsl, nsh, ndl, ndh);
			nel = even_of(jj + 1, nsl, dl, ndl);
			neh = even_of(jj + 1, nsh, dh, ndh);
		}
		inv_row(dst + (long)r0 * a.llpitch, L, el, eh);
		if (r1 < a.h) {
			const int ol = dl + tdiv2(el + nel);
			const int oh = dh + tdiv2(eh + neh);
			inv_row(dst + (long)r1 * a.llpitch, L, ol, oh);
		}
		dl = ndl;
		dh = ndh;
		el = nel;
		eh = neh;
	}
}


// ------------------------------------------------------ wide (16-byte) path ---
// Same algorithm with two column pairs per lane: 16-byte loads of the input rows,
// 8-byte stores of each subband row (forward) / 8-byte subband loads and 16-byte
// stores (inverse), and the next rows' loads issued one loop iteration ahead of
// their use.  Needs w % 4 == 0 and 16-byte aligned rows; other shapes take the
// narrow kernels above.

struct I2 {
	int a, b;
};

// The tiles' magnitude histograms, dropped by the forward kernel while it holds the coefficients (dwtx_hist_sink):
// the level's blocks of 32x32 pyramid positions are the entropy stage's tiles.
struct HistArgs {
	unsigned *cum32;       // [plane][NT][16]
	unsigned *tile_mx;     // [plane][NTP]
	const int *xy2tile;    // this level's [by * nbs + bx] -> tile
	int NT, NTP, nbs;
};

struct LevelArgsW {
	LevelArgs a;
	int nquads;       // w / 4
	int wx_log2;      // forward: 1 << wx_log2 waves of a block side by side
	HistArgs hist;
	long cstride;     // planar RGB pixels behind src8 / dst8 (dwtx_pixels::colour_stride(), in samples): from a window's R plane to its G plane, from G to B — negative
	                  // where the planes lie as B, G, R (src8 / dst8 is then the R plane all the same); 0: interleaved.
	                  // (After everything else, so that the interleaved kernels find their arguments where they were.)
	FloatFmt fmt;     // inverse, float pixels behind dst8 (only the float sinks read it)
	int ppw;          // the FY instances of the forward kernels: planes per window, 1 or 3 (which entry of the windows' table a plane reads)
	int fh, fwq;      // the flipped instances of the inverse kernels (FL): the WINDOWS' height and quads per row (dwtx_pixels::flip_h, flip_w / 4)
	// the delta sources of the forward kernels and the delta sinks of the inverse ones (dwtx_pixels::delta): the base pictures behind
	// base8 as the pixels lie behind src8 / dst8 — their own window stride, pitch and grid, in samples; no other kernel reads them
	const uint8_t *base8;
	long base_ps;
	int bpitch;
	WinGrid bgrid;
};

// Per lane and subband: counts of "magnitude below 2^q" for q = 0..15 — nibbles of R for the last few coefficients
// (adding 0x1111.. << 4t per coefficient, t its bit count), folded into the bytes of ev (even q) and od (odd q) before a
// nibble can overflow; mx = OR of the magnitudes.  The same counts k_hist (pack.hip) makes from memory.
struct HistAcc {
	unsigned long long R, ev, od;
	unsigned mx;
};

__device__ __forceinline__ void hist_add(HistAcc &h, int v)
{
	const unsigned a = (unsigned)(v < 0 ? -v : v);
	h.mx |= a;
	// (a magnitude of 2^15 and more counts as 15 bits here.  Magnitudes in [2^15, 2^16) are 16 bit planes, which the
	// coder accepts (k_plan in pack.hip refuses pmax > 16), and would be miscounted: these accumulators are for transforms
	// of 8-bit pixels, whose coefficients stay below 2^12 — a transform of deep pixels leaves every histogram to k_hist)
	const unsigned t = min(32u - (unsigned)__clz((int)a), 15u);
	h.R += 0x1111111111111111ull << (4u * t);
}

__device__ __forceinline__ void hist_fold(HistAcc &h)
{
	h.ev += h.R & 0x0f0f0f0f0f0f0f0full;
	h.od += (h.R >> 4) & 0x0f0f0f0f0f0f0f0full;
	h.R = 0;
}

// sum over the 16 lanes of a DPP row (its last lane ends up with the total)
__device__ __forceinline__ unsigned row16_add(unsigned v)
{
	v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
	v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
	v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
	v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
	return v;
}

__device__ __forceinline__ unsigned row16_or(unsigned v)
{
	v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
	v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
	v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
	v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
	return v;
}

// The 16 lanes of a row hold one block's columns: their counts, summed, are added to the block's tile (blocks that
// straddle two strips or two subbands get several such contributions).  All lanes of the wave take part.
__device__ __forceinline__ void hist_flush(HistAcc &h, const HistArgs &H, int plane, int bx, int by, int lane)
{
	hist_fold(h);
	unsigned D[8];
#pragma unroll
	for (int b = 0; b < 8; ++b)
		D[b] = row16_add(((unsigned)(h.ev >> (8 * b)) & 0xffu) | ((unsigned)(h.od >> (8 * b)) & 0xffu) << 16);
	const unsigned mx = row16_or(h.mx);
	if ((lane & 15) == 15 && bx < H.nbs && by < H.nbs) {
		const int tile = H.xy2tile[by * H.nbs + bx];
		if (tile >= 0) {
			unsigned *rec = H.cum32 + ((long)plane * H.NT + tile) * 16;
#pragma unroll
			for (int b = 0; b < 8; ++b)
				if (D[b])
					atomicAdd(rec + b, D[b]);
			if (mx)
				atomicOr(H.tile_mx + (long)plane * H.NTP + tile, mx);
		}
	}
	h.ev = h.od = 0;
	h.mx = 0;
}

// One row of the wave's strip, widened: what the int32 arithmetic lifts
struct FwdRaw {
	int4 x;
	int xr;           // x[4q+4] for lane 63
	int2 left;        // x[4q-2], x[4q-1] for lane 0
};

__device__ __forceinline__ void fwd_lift_w(const FwdRaw &r, int q, int lane, int nquads, I2 &lo, I2 &hi)
{
	int xr = __shfl_down(r.x.x, 1);
	if (lane == 63)
		xr = r.xr;
	if (q + 1 >= nquads)
		xr = r.x.z;                       // x[w] := x[w-2]
	const int d0 = r.x.y - tdiv2(r.x.x + r.x.z);
	const int d1 = r.x.w - tdiv2(r.x.z + xr);
	int dl = __shfl_up(d1, 1);
	if (lane == 0)
		dl = r.left.y - tdiv2(r.left.x + r.x.x);
	if (q == 0)
		dl = d0;                          // d[-1] := d[0]
	lo.a = r.x.x + tdiv4(dl + d0);
	lo.b = r.x.z + tdiv4(d0 + d1);
	hi.a = d0;
	hi.b = d1;
}

// The lane's two column pairs of a row as the vertical step sees them, in the int32 arithmetic (the packed 16-bit one,
// P2, is further down): the loop of fwd_level_body meets either through these overloads.
__device__ __forceinline__ I2 lift_pred(I2 odd, I2 e0, I2 e2)   // cdf53.h:13 down the columns
{
	I2 r = { odd.a - tdiv2(e0.a + e2.a), odd.b - tdiv2(e0.b + e2.b) };
	return r;
}

__device__ __forceinline__ I2 lift_upd(I2 even, I2 dprev, I2 d)   // cdf53.h:20
{
	I2 r = { even.a + tdiv4(dprev.a + d.a), even.b + tdiv4(dprev.b + d.b) };
	return r;
}

__device__ __forceinline__ void st2(int *p, I2 v)
{
	*reinterpret_cast<int2 *>(p) = make_int2(v.a, v.b);
}

__device__ __forceinline__ void st2(short *p, I2 v)
{
	*reinterpret_cast<unsigned *>(p) = ((unsigned)v.a & 0xffffu) | ((unsigned)v.b << 16);
}

__device__ __forceinline__ void hist_add(HistAcc &h, I2 v)
{
	hist_add(h, v.a);
	hist_add(h, v.b);
}

// the OR of the magnitudes as hist_add(.., I2) left it in HistAcc::mx: what hist_flush takes
__device__ __forceinline__ unsigned hist_mx(unsigned mx, I2) { return mx; }

// Workgroups are dealt round-robin over the 8 XCDs (each with an L2 of its own): with the plain mapping the
// strips left and right of a strip — whose edge sectors it also loads as halo — sit on other XCDs and those
// sectors come from HBM a second time.  Remap so that an XCD owns a contiguous run of strips (whole bands of
// rows): workgroup D of a plane works on strip (D mod 8) * (N/8) + D / 8.  Speed only; any mapping is correct.
__device__ __forceinline__ void xcd_strip(int &bx, int &by)
{
	bx = blockIdx.x;
	by = blockIdx.y;
	const int n = gridDim.x * gridDim.y;
	if ((n & 7) == 0) {
		const int d = bx + gridDim.x * by;
		const int s = (d & 7) * (n >> 3) + (d >> 3);
		by = s / gridDim.x;
		bx = s - by * gridDim.x;
	}
}

// The RGB source: every plane's workgroup reads all three bytes of its pixels, so the three channels of a strip are
// made neighbours in time ON ONE XCD (grid.x holds three workgroups per strip, grid.z the images): the second and the
// third find the pixels in that XCD's L2 instead of fetching them from HBM again.
__device__ __forceinline__ void xcd_strip_rgb(int &bx, int &by, int &c)
{
	const int gx = gridDim.x / 3, n = gx * gridDim.y;
	const int d = blockIdx.x + gridDim.x * blockIdx.y;   // 0 .. 3n-1; workgroup d runs on XCD d mod 8
	int s;
	if ((n & 7) == 0) {
		const int slot = d >> 3;
		s = (d & 7) * (n >> 3) + slot / 3;
		c = slot % 3;
	} else {
		s = d / 3;
		c = d % 3;
	}
	by = s / gx;
	bx = s - by * gx;
}

// A row moves from the registers it was loaded into to the registers it is used from: a move the register allocator
// cannot fold away, placed where the wave is to wait for the row (see the loop of fwd_level_body).  Every kind of row
// as it is loaded has its hold() below.
__device__ __forceinline__ unsigned hold(unsigned v)
{
	unsigned o;
	asm volatile("v_mov_b32 %0, %1" : "=v"(o) : "v"(v));
	return o;
}
__device__ __forceinline__ int hold(int v) { return (int)hold((unsigned)v); }
__device__ __forceinline__ uint2 hold(uint2 v) { return make_uint2(hold(v.x), hold(v.y)); }

// Rows for the batched loop of fwd_level_body: every lane loads — lanes beyond the row from the row's last quad, the
// edge piece from a clamped place — so that no load sits behind a branch or feeds a select (either would make the wave
// wait for it at once); what the extra lanes get is never used.  Where a lane loads in a row, the same for every row, in
// samples of the source: its quad, and the edge piece — before the quad for lane 0 (x[4q-2], x[4q-1] are its end),
// after it for the others (x[4q+4] is its start).
struct LaneAt {
	int main, edge;
};

// per_quad: source samples in a lane's four pixels; reach: samples in an edge piece
__device__ __forceinline__ LaneAt lane_at(int q, int lane, int nquads, int per_quad, int reach)
{
	const int m = per_quad * min(q, nquads - 1);
	LaneAt o = { m, lane == 0 ? max(m - reach, 0) : min(m + per_quad, per_quad * nquads - reach) };
	return o;
}

// an int32 row as it is loaded
struct FwdRawI {
	int4 x;           // x[4q .. 4q+3]
	int2 e;           // lane 0: x[4q-2], x[4q-1]; the other lanes: e.x = x[4q+4]
};

__device__ __forceinline__ FwdRawI fwd_load_i(const int *__restrict__ row, const LaneAt &at)
{
	FwdRawI r;
	r.x = *reinterpret_cast<const int4 *>(row + at.main);
	r.e = *reinterpret_cast<const int2 *>(row + at.edge);
	return r;
}

__device__ __forceinline__ FwdRawI hold(const FwdRawI &r)
{
	FwdRawI o;
	o.x = make_int4(hold(r.x.x), hold(r.x.y), hold(r.x.z), hold(r.x.w));
	o.e = make_int2(hold(r.e.x), hold(r.e.y));
	return o;
}

__device__ __forceinline__ FwdRaw widen(const FwdRawI &r)
{
	FwdRaw o;
	o.x = r.x;
	o.xr = r.e.x;
	o.left = r.e;
	return o;
}

// A row of 16-bit samples as it is loaded — a lane's quad is 8 bytes: a band kept as 16-bit values (the levels of an
// 8-bit source whose range allows it), widened with its sign, or deep gray pixels (uint16_t samples, include/dwtx.h),
// widened without one (pnm.h:69-74).
struct FwdRawS {
	uint2 x;          // x[4q .. 4q+3]
	unsigned e;       // lane 0: x[4q-2], x[4q-1]; the other lanes: its low half = x[4q+4]
};

__device__ __forceinline__ FwdRawS fwd_load_s(const void *row, const LaneAt &at)
{
	const uint16_t *p = static_cast<const uint16_t *>(row);
	FwdRawS r;
	r.x = *reinterpret_cast<const uint2 *>(p + at.main);
	r.e = *reinterpret_cast<const unsigned *>(p + at.edge);
	return r;
}

__device__ __forceinline__ FwdRawS hold(const FwdRawS &r)
{
	FwdRawS o = { hold(r.x), hold(r.e) };
	return o;
}

__device__ __forceinline__ FwdRaw widen_s(const FwdRawS &r)
{
	FwdRaw o;
	o.x = make_int4((int)(short)(r.x.x & 0xffffu), (int)r.x.x >> 16, (int)(short)(r.x.y & 0xffffu), (int)r.x.y >> 16);
	o.xr = (int)(short)(r.e & 0xffffu);
	o.left = make_int2(o.xr, (int)r.e >> 16);
	return o;
}

__device__ __forceinline__ FwdRaw widen_u(const FwdRawS &r)
{
	FwdRaw o;
	o.x = make_int4((int)(r.x.x & 0xffffu), (int)(r.x.x >> 16), (int)(r.x.y & 0xffffu), (int)(r.x.y >> 16));
	o.xr = (int)(r.e & 0xffffu);
	o.left = make_int2(o.xr, (int)(r.e >> 16));
	return o;
}

// The colour transform on a pixel's three samples AS THEY LIE (s0 the lowest-addressed): R, G, B, or — BGR, dwtx_pixels::order —
// B, G, R, where the triple handed on takes R from the third sample and B from the first.  Which is which is decided when
// the kernel is compiled: the interleaved sources below exist once per order, and the two differ in no instruction but
// the operands of the transform.  (Planar pixels need none of it: the host hands their kernels the R plane and a negative stride.)
template <bool BGR>
__device__ __forceinline__ int ycocg_lies(int s0, int s1, int s2, int ch)
{
	return BGR ? ycocg_ch(s2, s1, s0, ch) : ycocg_ch(s0, s1, s2, ch);
}

// Interleaved RGB16: a lane's four pixels are 24 bytes (three 8-byte loads; rows of W % 4 == 0 pixels are multiples of
// 24 bytes, so they stay 8-byte aligned), the neighbours' pixels three words: lane 0 pixels 4q-2 and 4q-1, the other lanes
// pixel 4q+4 in the first three samples.  Every plane's launch takes its own channel of image.h:52-65 when the row is used.
struct FwdRawRgb16 {
	uint2 a, b, c;
	unsigned e0, e1, e2;
};

__device__ __forceinline__ FwdRawRgb16 hold(const FwdRawRgb16 &r)
{
	FwdRawRgb16 o = { hold(r.a), hold(r.b), hold(r.c), hold(r.e0), hold(r.e1), hold(r.e2) };
	return o;
}

// (SGN, here and for the planar row: int16_t samples, widened with their sign — the signed twins of the deep sources)
template <bool BGR = false, bool SGN = false>
__device__ __forceinline__ FwdRaw widen(const FwdRawRgb16 &r, int ch)
{
	auto lo = [](unsigned w) { return SGN ? (int)(short)(w & 0xffffu) : (int)(w & 0xffffu); };
	auto hi = [](unsigned w) { return SGN ? (int)w >> 16 : (int)(w >> 16); };
	FwdRaw o;
	o.x.x = ycocg_lies<BGR>(lo(r.a.x), hi(r.a.x), lo(r.a.y), ch);
	o.x.y = ycocg_lies<BGR>(hi(r.a.y), lo(r.b.x), hi(r.b.x), ch);
	o.x.z = ycocg_lies<BGR>(lo(r.b.y), hi(r.b.y), lo(r.c.x), ch);
	o.x.w = ycocg_lies<BGR>(hi(r.c.x), lo(r.c.y), hi(r.c.y), ch);
	o.xr = ycocg_lies<BGR>(lo(r.e0), hi(r.e0), lo(r.e1), ch);
	o.left = make_int2(o.xr, ycocg_lies<BGR>(hi(r.e1), lo(r.e2), hi(r.e2), ch));
	return o;
}

// Planar RGB16: the same row of the window's three planes, each loaded as a gray deep row is (8 bytes for the lane's quad, a
// word of neighbours, inside the row's own W samples of that plane); the plane's launch takes its channel of image.h:52-65
struct FwdRawRgbS3 {
	FwdRawS r, g, b;
};

__device__ __forceinline__ FwdRawRgbS3 hold(const FwdRawRgbS3 &p)
{
	FwdRawRgbS3 o = { hold(p.r), hold(p.g), hold(p.b) };
	return o;
}

template <bool SGN = false>
__device__ __forceinline__ FwdRaw widen(const FwdRawRgbS3 &p, int ch)
{
	const FwdRaw r = SGN ? widen_s(p.r) : widen_u(p.r), g = SGN ? widen_s(p.g) : widen_u(p.g), b = SGN ? widen_s(p.b) : widen_u(p.b);
	FwdRaw o;
	o.x.x = ycocg_ch(r.x.x, g.x.x, b.x.x, ch);
	o.x.y = ycocg_ch(r.x.y, g.x.y, b.x.y, ch);
	o.x.z = ycocg_ch(r.x.z, g.x.z, b.x.z, ch);
	o.x.w = ycocg_ch(r.x.w, g.x.w, b.x.w, ch);
	o.xr = ycocg_ch(r.xr, g.xr, b.xr, ch);
	o.left = make_int2(o.xr, ycocg_ch(r.left.y, g.left.y, b.left.y, ch));
	return o;
}

// ---- two levels per pass (forward, int32 planes) ----
// One launch per level moves every LL band twice more than the transform needs: written by level k, read by level k+1
// (16 B x sum 4^-k = 21.33 B per sample forward + inverse against 16 algorithmic).  Here a wave runs level k as above and
// hands each LL row — the lane's two LL samples are exactly one column PAIR of level k+1 — straight to a second lifting
// stage in registers: the LL band of level k never exists in memory.
// Seams.  Level k+1 of a lane needs the LL samples of the lanes beside it, which need the input samples beside theirs.
// Instead of halo loads the waves OVERLAP: lane 1's level-k results are right without any edge load (lane 0 supplies d,
// lane 2 its even sample), lane 2's level-k+1 results need lane 1's; on the right one lane is enough.  Vertically a
// strip's first row pair of level k+1 needs the pair before it: three row pairs of level k ahead of the strip, one behind.
// What decides the kernel's speed is how its STORES meet the 128-byte lines (round 4's ablation, 64 planes of 4096x4096:
// a pass that only reads takes 13 us per plane, the level-k detail stores add 12-16, level k+1's 4-byte stores 4-7 —
// reads and writes do not overlap, a written byte costs 1.5 read bytes, and owning 61 lanes of 64 (rows of 488 bytes
// at multiples of 488) was 17 % SLOWER than one launch per level although it moved 14 % fewer bytes): a wave owns the
// outputs of 48 lanes — rows of 384 bytes (level k) and 192 bytes (level k+1; the block's four waves side by side make
// whole lines of them) at multiples of themselves; lanes 8 .. 56 take part (the lanes before them keep the loads on
// whole lines, the lanes after them repeat lane 56's quad), and the stores bypass the L2's allocation (nontemporal: 5 %).
// Shapes: w % 4 == 0 (a lane's quad) and h % 4 == 0 (both levels have even heights: every row pair is whole);
// everything else takes one launch per level.
struct Level2Args {
	const int *src;  long src_ps;  int spitch;   // level k input, w x h
	int *ll2;        long ll2_ps;  int ll2pitch; // LL of level k+1, w/4 x h/4
	int *det;        long det_ps;  int dpitch;   // the pyramid: detail bands of both levels (Mallat layout)
	int w, h, nquads;
	int mpw;          // level k+1 row pairs per wave strip
};
// (strips of 8 row pairs of level k+1 — 32 input rows — measured best, against 4, 16, 32 and 64: the halo rows a strip shares with its
// neighbours are then still in the XCD's L2 when the neighbour asks for them, and there are eight times the waves to hide latency behind)
constexpr int F2_MPW = 8;
constexpr int F2_FIRST = 8, F2_OWN = 48, F2_ACTIVE = F2_FIRST + F2_OWN + 1;   // lanes F2_FIRST .. F2_FIRST + F2_OWN - 1 own a wave's outputs; lanes from F2_ACTIVE on only repeat the last active lane's loads

// cdf53.h:9-34 along the row for a lane's quad, neighbours by shuffle only (lanes 0 and 63 get wrong values where they
// would need a lane that is not there: lo.a of lane 0, lo.b / hi.b of lane 63 — never used, see above)
__device__ __forceinline__ void fwd_lift_q(const int4 &x, int q, int nquads, I2 &lo, I2 &hi)
{
	int xr = __shfl_down(x.x, 1);
	if (q + 1 >= nquads)
		xr = x.z;                         // x[w] := x[w-2]
	const int d0 = x.y - tdiv2(x.x + x.z);
	const int d1 = x.w - tdiv2(x.z + xr);
	int dl = __shfl_up(d1, 1);
	if (q <= 0)
		dl = d0;                          // d[-1] := d[0]
	lo.a = x.x + tdiv4(dl + d0);
	lo.b = x.z + tdiv4(d0 + d1);
	hi.a = d0;
	hi.b = d1;
}

// the same one level down: the lane's LL pair (x0, x1) of a row -> (low, high)
__device__ __forceinline__ void fwd_lift_pair(int x0, int x1, int q, int nquads, int &lo, int &hi)
{
	int xr = __shfl_down(x0, 1);
	if (q + 1 >= nquads)
		xr = x0;
	const int d = x1 - tdiv2(x0 + xr);
	int dl = __shfl_up(d, 1);
	if (q <= 0)
		dl = d;
	lo = x0 + tdiv4(dl + d);
	hi = d;
}

__device__ __forceinline__ int4 hold(const int4 &v) { return make_int4(hold(v.x), hold(v.y), hold(v.z), hold(v.w)); }
__device__ __forceinline__ void st2nt(int *p, I2 v)
{
	typedef int v2i __attribute__((ext_vector_type(2)));
	v2i x = { v.a, v.b };
	__builtin_nontemporal_store(x, reinterpret_cast<v2i *>(p));
}

__global__ __launch_bounds__(64 * WAVES) void k_fwd2_level_w(Level2Args a)
{
	const int lane = threadIdx.x & 63, wv = wave_in_block();
	int bx, by;
	xcd_strip(bx, by);
	const int strip = bx * WAVES + wv;                      // the block's waves side by side
	if (strip * F2_OWN >= a.nquads)
		return;
	const int q = strip * F2_OWN - F2_FIRST + lane;         // the lane's quad of level k = its column pair of level k+1
	const int h2 = a.h >> 1, h4 = a.h >> 2, w2 = a.w >> 1, w4 = a.w >> 2;
	const int m0 = by * a.mpw;
	if (m0 >= h4)
		return;
	const int m1 = min(m0 + a.mpw, h4);
	const int plane = blockIdx.z;
	const bool own = lane >= F2_FIRST && lane < F2_FIRST + F2_OWN && q < a.nquads;
	// (every lane loads, from a clamped place: the lanes beyond the right-hand halo lane repeat its quad — no line of their own)
	const int *src = a.src + plane * a.src_ps + 4 * min(max(q - max(lane - (F2_ACTIVE - 1), 0), 0), a.nquads - 1);
	int *ll2 = a.ll2 + plane * a.ll2_ps;
	int *det = a.det + plane * a.det_ps;

	// LL rows of level k that the strip's row pairs m0 .. m1-1 of level k+1 need: 2 m0 - 2 (for the pair before: its
	// detail enters the first update) .. 2 m1 (the last predict; the plane's last row pair mirrors instead)
	const int r_lo = max(2 * m0 - 2, 0), r_hi = min(2 * m1, h2 - 1);
	const int jfirst = max(r_lo - 1, 0);        // level k: one row pair more, for its detail
	constexpr int S = 2;
	auto rowp = [&](int r) { return src + (long)min(r, a.h - 1) * a.spitch; };
	I2 l0, h0, pl = { 0, 0 }, ph = { 0, 0 };
	fwd_lift_q(*reinterpret_cast<const int4 *>(rowp(2 * jfirst)), q, a.nquads, l0, h0);
	int4 cur[2 * S], nxt[2 * S];
#pragma unroll
	for (int k = 0; k < 2 * S; ++k)
		nxt[k] = *reinterpret_cast<const int4 *>(rowp(2 * jfirst + 1 + k));
	// what a batch leaves for the next iteration's stores
	I2 osh[S], odl[S], odh[S];
	int o2[4] = { 0, 0, 0, 0 }, o2m = -1;   // a finished row pair of level k+1: LL, HL, LH, HH and its index
	auto store_batch = [&](int jb) {
		if (!own)
			return;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int j = jb + s;
			if (j >= 2 * m0 && j < 2 * m1) {
				st2nt(det + (long)j * a.dpitch + w2 + 2 * q, osh[s]);
				st2nt(det + (long)(h2 + j) * a.dpitch + 2 * q, odl[s]);
				st2nt(det + (long)(h2 + j) * a.dpitch + w2 + 2 * q, odh[s]);
			}
		}
		if (o2m >= m0) {
			__builtin_nontemporal_store(o2[0], ll2 + (long)o2m * a.ll2pitch + q);
			__builtin_nontemporal_store(o2[1], det + (long)o2m * a.dpitch + w4 + q);
			__builtin_nontemporal_store(o2[2], det + (long)(h4 + o2m) * a.dpitch + q);
			__builtin_nontemporal_store(o2[3], det + (long)(h4 + o2m) * a.dpitch + w4 + q);
		}
		o2m = -1;
	};
	// level k+1, column direction: A = the pair's even row, B = its odd row, (pd*) the details of the pair before
	int Al = 0, Ah = 0, Bl = 0, Bh = 0, pdl = 0, pdh = 0;
	auto finish_pair = [&](int m, int Cl, int Ch) {
		const int dl2 = Bl - tdiv2(Al + Cl), dh2 = Bh - tdiv2(Ah + Ch);
		o2[0] = Al + tdiv4((m ? pdl : dl2) + dl2);
		o2[1] = Ah + tdiv4((m ? pdh : dh2) + dh2);
		o2[2] = dl2;
		o2[3] = dh2;
		o2m = m;          // (the pair before the strip, m0 - 1, is only here for its details: never stored)
		pdl = dl2;
		pdh = dh2;
	};
	for (int jb = jfirst; jb <= r_hi; jb += S) {
#pragma unroll
		for (int k = 0; k < 2 * S; ++k)
			cur[k] = hold(nxt[k]);   // the one wait of the iteration (see fwd_level_body)
		if (jb > jfirst)
			store_batch(jb - S);
		if (jb + S <= r_hi) {
#pragma unroll
			for (int k = 0; k < 2 * S; ++k)
				nxt[k] = *reinterpret_cast<const int4 *>(rowp(2 * (jb + S) + 1 + k));
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int jj = jb + s;
			if (jj > r_hi)
				break;
			I2 l1, h1, l2 = l0, h2v = h0;
			fwd_lift_q(cur[2 * s], q, a.nquads, l1, h1);
			if (2 * jj + 2 < a.h)
				fwd_lift_q(cur[2 * s + 1], q, a.nquads, l2, h2v);
			const I2 dl = lift_pred(l1, l0, l2);
			const I2 dh = lift_pred(h1, h0, h2v);
			const I2 sl = lift_upd(l0, jj ? pl : dl, dl);
			osh[s] = lift_upd(h0, jj ? ph : dh, dh);
			odl[s] = dl;
			odh[s] = dh;
			pl = dl;
			ph = dh;
			l0 = l2;
			h0 = h2v;
			if (jj >= r_lo) {   // sl is LL row jj of level k: the lane's pair of level k+1
				int lo2, hi2;
				fwd_lift_pair(sl.a, sl.b, q, a.nquads, lo2, hi2);
				if (jj & 1) {
					Bl = lo2;
					Bh = hi2;
				} else {
					if (jj > r_lo)
						finish_pair((jj >> 1) - 1, lo2, hi2);
					Al = lo2;
					Ah = hi2;
				}
			}
		}
	}
	const int jlast = jfirst + (r_hi - jfirst) / S * S;
	if (m1 == h4) {
		// the plane's last row pair of level k+1 has no even row below it: x[N] := x[N-2] (its B row came with the last batch)
		store_batch(jlast);
		finish_pair(h4 - 1, Al, Ah);
		store_batch(jlast + S);   // (beyond the strip's rows of level k: only the finished pair goes out)
	} else {
		store_batch(jlast);
	}
}

// ---- the finest level from 8-bit pixels, in packed 16-bit arithmetic ----
// Samples of magnitude <= 255 cannot leave 16 bits anywhere in one level of cdf53.h:9-34 (|d| <= 510 after the row
// pass, <= 1020 after the column pass; every intermediate sum stays below 2^12): the lane's two column pairs ride in
// the halves of one register and every add / shift / subtract is a v_pk_* instruction on both.  Same results as
// the int32 arithmetic, with about half the vector instructions.
typedef short P2 __attribute__((ext_vector_type(2)));
typedef unsigned short U2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ P2 p2_of(unsigned u) { return __builtin_bit_cast(P2, u); }
__device__ __forceinline__ unsigned bits_of(P2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ P2 tdiv2p(P2 a) { return (a + (P2)((U2)a >> (U2)15)) >> (P2)1; }
__device__ __forceinline__ P2 tdiv4p(P2 a) { return (a + ((a >> (P2)15) & (P2)3)) >> (P2)2; }

// what the loop of fwd_level_body asks of an arithmetic (the int32 one: I2 above)
__device__ __forceinline__ P2 lift_pred(P2 odd, P2 e0, P2 e2) { return odd - tdiv2p(e0 + e2); }
__device__ __forceinline__ P2 lift_upd(P2 even, P2 dprev, P2 d) { return even + tdiv4p(dprev + d); }
__device__ __forceinline__ void st2(int *p, P2 v) { *reinterpret_cast<int2 *>(p) = make_int2((int)v.x, (int)v.y); }
__device__ __forceinline__ void st2(short *p, P2 v) { *reinterpret_cast<unsigned *>(p) = bits_of(v); }

// (no clamp at 15 bits as in hist_add(.., int): the magnitudes of a level from 8-bit samples are below 2^12)
__device__ __forceinline__ void hist_add(HistAcc &h, P2 v)
{
	const unsigned a = bits_of(__builtin_elementwise_max(v, -v));   // both magnitudes
	h.mx |= a;
	const unsigned t0 = 32u - (unsigned)__clz((int)(a & 0xffffu)), t1 = 32u - (unsigned)__clz((int)(a >> 16));
	h.R += 0x1111111111111111ull << (4u * t0);
	h.R += 0x1111111111111111ull << (4u * t1);
}

// (HistAcc::mx gathered both halves: one OR more before a flush)
__device__ __forceinline__ unsigned hist_mx(unsigned mx, P2) { return (mx | (mx >> 16)) & 0xffffu; }

// image.h:52-65 on two pixels at once: channel ch of (R, G, B) pairs
__device__ __forceinline__ P2 ycocg_p(P2 r, P2 g, P2 b, int ch)
{
	const P2 co = r - b;
	const P2 t = b + tdiv2p(co);
	const P2 cg = g - t;
	return ch == 0 ? t + tdiv2p(cg) : ch == 1 ? co : cg;
}

// one row's samples of this lane as packed pairs: E = (x[4q], x[4q+2]), O = (x[4q+1], x[4q+3]); xr = x[4q+4] in its low
// half (lane 63 only), left = (x[4q-2], x[4q-1]) (lane 0 only)
struct RowP {
	P2 E, O, xr, left;
};

// cdf53.h:9-34 along the row for the lane's two pairs: L = (s[2q], s[2q+1]), Hh = (d[2q], d[2q+1])
__device__ __forceinline__ void fwd_lift_p(const RowP &r, int q, int lane, int nquads, P2 &L, P2 &Hh)
{
	const unsigned e = bits_of(r.E);
	unsigned nx = (unsigned)__shfl_down((int)e, 1);          // the next lane's (x[4q+4], ..)
	if (lane == 63)
		nx = bits_of(r.xr);
	if (q + 1 >= nquads)
		nx = e >> 16;                                        // x[w] := x[w-2]
	const P2 En = p2_of(__builtin_amdgcn_alignbit(nx, e, 16));   // (x[4q+2], x[4q+4])
	const P2 D = r.O - tdiv2p(r.E + En);
	const unsigned d = bits_of(D);
	unsigned pv = (unsigned)__shfl_up((int)d, 1);            // high half: the previous lane's d[2q-1]
	if (lane == 0) {
		const P2 dm = r.left.yy - tdiv2p(r.left.xx + r.E.xx);   // d[2q-1] from the two samples before the strip
		pv = bits_of(dm) << 16;
	}
	if (q == 0)
		pv = d << 16;                                        // d[-1] := d[0]
	const P2 Dl = p2_of(__builtin_amdgcn_alignbit(d, pv, 16));   // (d[2q-1], d[2q])
	L = r.E + tdiv4p(Dl + D);
	Hh = D;
}

// 8-bit rows wait for their turn as they were loaded and become a RowP — widened, RGB through the colour transform of
// image.h:52-65 — when they are used.  Gray: four pixels in a word, the neighbours' in another.
struct FwdRaw8 {
	unsigned v;       // pixels 4q .. 4q+3
	unsigned edge;    // the word after them (lane 63: its first byte is x[4q+4]) or before them (lane 0: its last two are x[4q-2], x[4q-1])
};

__device__ __forceinline__ FwdRaw8 fwd_load_8(const uint8_t *__restrict__ row, const LaneAt &at)
{
	FwdRaw8 r;
	r.v = *reinterpret_cast<const unsigned *>(row + at.main);
	r.edge = *reinterpret_cast<const unsigned *>(row + at.edge);
	return r;
}

__device__ __forceinline__ FwdRaw8 hold(const FwdRaw8 &r)
{
	FwdRaw8 o = { hold(r.v), hold(r.edge) };
	return o;
}

__device__ __forceinline__ RowP row_p(const FwdRaw8 &r, int)
{
	RowP o;
	o.E = p2_of(r.v & 0x00ff00ffu);
	o.O = p2_of((r.v >> 8) & 0x00ff00ffu);
	o.xr = p2_of(r.edge & 255u);
	o.left = p2_of(__builtin_amdgcn_perm(0u, r.edge, 0x0c030c02u));   // the last two bytes of the word before
	return o;
}

// ycocg_lies for packed pairs
template <bool BGR>
__device__ __forceinline__ P2 ycocg_lies_p(P2 s0, P2 s1, P2 s2, int ch)
{
	return BGR ? ycocg_p(s2, s1, s0, ch) : ycocg_p(s0, s1, s2, ch);
}

// Interleaved RGB: the row as the two loads deliver it — the four pixels' three words and two words of neighbours in
// consecutive registers; taking single words out of them at load time would be a use of the load.
typedef unsigned U32x2 __attribute__((ext_vector_type(2)));
typedef unsigned U32x3 __attribute__((ext_vector_type(3)));
typedef unsigned U32x4 __attribute__((ext_vector_type(4)));
struct FwdRawRgb {
	U32x3 abc;   // pixels 4q .. 4q+3
	U32x2 e;     // lane 63: e.x = the word with pixel 4q+4; lane 0: bytes 12q-8 .. 12q-1 (pixels 4q-2 and 4q-1 are the last six)
};

__device__ __forceinline__ FwdRawRgb hold(const FwdRawRgb &r)
{
	FwdRawRgb o = { { hold(r.abc.x), hold(r.abc.y), hold(r.abc.z) }, { hold(r.e.x), hold(r.e.y) } };
	return o;
}

template <bool BGR = false>
__device__ __forceinline__ RowP row_p(const FwdRawRgb &r, int ch)
{
	// a = R0 G0 B0 R1, b = G1 B1 R2 G2, c = B2 R3 G3 B3 — BGR: R and B the other way round, here and in the edge words — (v_perm_b32: selector bytes 0-3 pick from the second operand, 4-7 from the first, 0x0c is zero)
	const unsigned a = r.abc.x, b = r.abc.y, c = r.abc.z, e0 = r.e.x, e1 = r.e.y;
	RowP o;
	o.E = ycocg_lies_p<BGR>(p2_of(__builtin_amdgcn_perm(b, a, 0x0c060c00u)), p2_of(__builtin_amdgcn_perm(b, a, 0x0c070c01u)),
		p2_of(__builtin_amdgcn_perm(c, a, 0x0c040c02u)), ch);
	o.O = ycocg_lies_p<BGR>(p2_of(__builtin_amdgcn_perm(c, a, 0x0c050c03u)), p2_of(__builtin_amdgcn_perm(c, b, 0x0c060c00u)),
		p2_of(__builtin_amdgcn_perm(c, b, 0x0c070c01u)), ch);
	// lane 63: e0 = R4 G4 B4 ..; lane 0: e0, e1 = bytes 12q-8 .. 12q-1, pixels 4q-2 and 4q-1 are the last six
	o.xr = ycocg_lies_p<BGR>(p2_of(e0 & 255u), p2_of((e0 >> 8) & 255u), p2_of((e0 >> 16) & 255u), ch);
	o.left = ycocg_lies_p<BGR>(p2_of(__builtin_amdgcn_perm(e1, e0, 0x0c050c02u)), p2_of(__builtin_amdgcn_perm(e1, e0, 0x0c060c03u)),
		p2_of(__builtin_amdgcn_perm(e1, e0, 0x0c070c04u)), ch);
	return o;
}

// Planar RGB rows: the same row of the window's three planes, each as a gray row is loaded — the lane's quad is one aligned
// word per channel and the neighbours' another, both inside the row's own W bytes of that plane.
// Nothing is unpacked: the bytes of a word are four pixels of ONE channel, so the even / odd pairs of row_p(FwdRaw8) feed
// the packed colour transform as they are (against six v_perm_b32 per row and two for the edges from interleaved pixels).
struct FwdRawRgb3 {
	FwdRaw8 r, g, b;
};

__device__ __forceinline__ FwdRawRgb3 hold(const FwdRawRgb3 &r)
{
	FwdRawRgb3 o = { hold(r.r), hold(r.g), hold(r.b) };
	return o;
}

__device__ __forceinline__ RowP row_p(const FwdRawRgb3 &r, int ch)
{
	const RowP R = row_p(r.r, 0), G = row_p(r.g, 0), B = row_p(r.b, 0);
	RowP o = { ycocg_p(R.E, G.E, B.E, ch), ycocg_p(R.O, G.O, B.O, ch), ycocg_p(R.xr, G.xr, B.xr, ch), ycocg_p(R.left, G.left, B.left, ch) };
	return o;
}

// RGB in 4-byte pixels: the lane's four pixels are one 16-byte load (rows and window origins are multiples of 4 bytes:
// dwtx_pixels::wide()), a word per pixel, the fourth byte of each never used; the edge is the neighbours' two words — lane 0:
// pixels 4q-2 and 4q-1, the others: pixel 4q+4 first — clamped into the row's own 4*W bytes like every edge here.
struct FwdRawRgbx {
	U32x4 px;    // pixels 4q .. 4q+3
	U32x2 e;
};

__device__ __forceinline__ FwdRawRgbx hold(const FwdRawRgbx &r)
{
	FwdRawRgbx o = { { hold(r.px.x), hold(r.px.y), hold(r.px.z), hold(r.px.w) }, { hold(r.e.x), hold(r.e.y) } };
	return o;
}

// channel ch of the pixels in the words lo and hi, as a packed pair (v_perm_b32 as in row_p(FwdRawRgb): a word is R G B x, or B G R x)
template <bool BGR>
__device__ __forceinline__ P2 rgbx_pair(unsigned lo, unsigned hi, int ch)
{
	return ycocg_lies_p<BGR>(p2_of(__builtin_amdgcn_perm(hi, lo, 0x0c040c00u)), p2_of(__builtin_amdgcn_perm(hi, lo, 0x0c050c01u)),
		p2_of(__builtin_amdgcn_perm(hi, lo, 0x0c060c02u)), ch);
}

template <bool BGR = false>
__device__ __forceinline__ RowP row_p(const FwdRawRgbx &r, int ch)
{
	const unsigned e0 = r.e.x, e1 = r.e.y;
	RowP o = { rgbx_pair<BGR>(r.px.x, r.px.z, ch), rgbx_pair<BGR>(r.px.y, r.px.w, ch),
		ycocg_lies_p<BGR>(p2_of(e0 & 255u), p2_of((e0 >> 8) & 255u), p2_of((e0 >> 16) & 255u), ch),   // lane 63: e0 = pixel 4q+4
		rgbx_pair<BGR>(e0, e1, ch) };                                                          // lane 0: e0, e1 = pixels 4q-2, 4q-1
	return o;
}

// ---- the sources of a wide forward level ----
// FwdSrc<Src>: what the one loop below needs to know about where its samples come from.
//   Pair        the arithmetic the level is lifted in: I2 (int32) or P2 (packed 16-bit: 8-bit pixels only, see above)
//   Loaded      a row as it is loaded, and as it waits for its turn
//   Used        a row in cur[], as a batch's arithmetic takes it: the int32 sources widen it there (FwdRaw), the packed
//               ones leave it as loaded and make a RowP of it in lift()
//   S           row pairs per batch of the loop
//   RGB_GRID    the three channels of a strip are three workgroups side by side (xcd_strip_rgb) and the channel a
//               compile-time constant of the body; otherwise a workgroup column per plane and base() says the channel
//   det16(a, plane), details16(p)   the plane's 16-bit detail bands, and whether the details go there: always for
//               16-bit bands, never for int32 and deep sources, where the pointer is set for 8-bit pixels
//   base(a, plane, ch)   the plane's first sample (RGB: of its window; the planar ones: in channel 0's plane) and its channel
//   at(q, lane, nquads)  where the lane loads in every row
//   load(row, at, cstride, ch), used(loaded, ch), lift(used, ch, q, lane, nquads, lo, hi)
// (the pitch, the strides and `at` count samples of the source — bytes for 8-bit pixels.)
template <typename Src>
struct FwdSrc;

// the band a level of k_fwd_level_w reads: int32 planes, 16-bit planes (dwtx_p16: the detail bands go out as 16-bit values
// too), or — the finest level of a deep picture — uint16_t pixels, gray, interleaved RGB or planar RGB; and the pixels
// k_fwd_pixels_w reads (names for Band<>'s five and for uint8_t, Rgb8, RgbP8 and Rgbx8, then the
// three B, G, R twins: Band<SRC_BGR16>, Bgr8, Bgrx8).  The values are template arguments of Band<>, and so part of the kernels'
// names, and nothing else: no table is indexed by them (the host's table of pixel ends, wide_row(), names its rows by what the pixels are)
enum { SRC_I32 = 0, SRC_I16, SRC_U16, SRC_RGB16, SRC_RGBP16, SRC_U8, SRC_RGB8, SRC_RGBP8, SRC_RGBX8, SRC_BGR16, SRC_BGR8, SRC_BGRX8,
	// float pixels (FloatPix<> below), gray and planar (P) fp32 and fp16 / bf16: quantised to at most 255, and (D) beyond
	SRC_F32, SRC_H16, SRC_F32P, SRC_H16P, SRC_F32D, SRC_H16D, SRC_F32PD, SRC_H16PD,
	// int16_t pixels (dwtx_encode_view_signed): the twins of SRC_U16, SRC_RGB16, SRC_RGBP16 and SRC_BGR16 that widen with the sign
	SRC_S16, SRC_RGB16S, SRC_RGBP16S, SRC_BGR16S,
	// delta views (dwtx_encode_view_delta): the picture and its base, gray of the three sample types and interleaved 8-bit RGB in both orders
	SRC_DELTA_U8, SRC_DELTA_U16, SRC_DELTA_S16, SRC_DELTA_RGB8, SRC_DELTA_BGR8 };
template <int SRC>
struct Band {};
// 8-bit interleaved RGB pixels, of which each plane's workgroup takes its own YCoCg-R channel (image.h:52-65 fused; 8-bit
// gray pixels — pnm.h:69-74 fused — are FwdSrc<uint8_t>)
struct Rgb8 {};
// 8-bit planar RGB pixels (dwtx_pixels::channel_stride): three gray-style rows per row, one per plane, no unpacking
struct RgbP8 {};
// 8-bit RGB in 4-byte pixels (dwtx_pixels::rgbx8(): RGBA / RGBX surfaces, pixel step 4): interleaved like Rgb8, a lane's
// four pixels one 16-byte piece whose every fourth byte is loaded and never used
struct Rgbx8 {};
// The interleaved sources for pixels that lie as B, G, R (dwtx_pixels::order): Band<SRC_BGR16>, and these two.  Each is its RGB
// twin — loads, addresses, registers — with the colour triple taken the other way round where the row is used.
struct Bgr8 {};
struct Bgrx8 {};

// plane p of an RGB picture = channel p % 3 of window p / 3 (src_ps from a window to the next)
__device__ __forceinline__ long rgb_window(const LevelArgs &a, int plane, int &ch)
{
	ch = plane % 3;
	return win_off(a.grid, a.src_ps, plane / 3);
}

struct FwdInt32 {
	static constexpr bool FLOAT = false;   // (the float sources' used() takes the launch's arguments as well)
	static constexpr bool DELTA = false;   // (the delta sources walk two views: rows() for base(), DeltaRows for the row pointer)
	typedef I2 Pair;
	typedef FwdRaw Used;
	static constexpr int S = 2;
	static constexpr bool RGB_GRID = false;
	static __device__ __forceinline__ short *det16(const LevelArgs &, int) { return nullptr; }
	static __device__ __forceinline__ bool details16(const short *) { return false; }
	static __device__ __forceinline__ void lift(const FwdRaw &r, int, int q, int lane, int nquads, I2 &lo, I2 &hi) { fwd_lift_w(r, q, lane, nquads, lo, hi); }
};

struct FwdPacked {
	static constexpr bool FLOAT = false;
	static constexpr bool DELTA = false;
	typedef P2 Pair;
	static constexpr int S = 2;
	static constexpr bool RGB_GRID = false;
	static __device__ __forceinline__ short *det16(const LevelArgs &a, int plane) { return a.det16 ? a.det16 + plane * a.det_ps : nullptr; }   // (uniform)
	static __device__ __forceinline__ bool details16(const short *p) { return p != nullptr; }
	template <typename Row>
	static __device__ __forceinline__ Row used(const Row &r, int) { return r; }
	template <typename Row>
	static __device__ __forceinline__ void lift(const Row &r, int ch, int q, int lane, int nquads, P2 &lo, P2 &hi) { fwd_lift_p(row_p(r, ch), q, lane, nquads, lo, hi); }
};

template <>
struct FwdSrc<Band<SRC_I32>> : FwdInt32 {
	typedef FwdRawI Loaded;
	static __device__ __forceinline__ const int *base(const LevelArgs &a, int plane, int &) { return a.src + plane * a.src_ps; }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 2); }
	static __device__ __forceinline__ Loaded load(const int *row, const LaneAt &at, long, int) { return fwd_load_i(row, at); }
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int) { return widen(r); }
};

// The level's input band and its detail bands are 16-bit values (levels 2..5 of an 8-bit source in the codec: with
// |x| <= 255 a sample of level k's input stays below 255 * 2.25^(k-1) and its details below four times that — the
// low-pass of cdf53.h:9-34 has an l1 norm of 1.5 per direction, the high-pass of 2 — i.e. 26 142 on the fifth level;
// that bound is loose: the composed five-level response has an l1 norm of 7.95, 2 028 for 8-bit samples, and
// tests/test_codec_gpu.py builds the picture that gets there); the arithmetic is int32 either way.
template <>
struct FwdSrc<Band<SRC_I16>> : FwdInt32 {
	typedef FwdRawS Loaded;
	static __device__ __forceinline__ short *det16(const LevelArgs &a, int plane) { return a.det16 + plane * a.det_ps; }
	static __device__ __forceinline__ bool details16(const short *) { return true; }
	static __device__ __forceinline__ const short *base(const LevelArgs &a, int plane, int &) { return a.src16 + plane * a.src_ps; }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 2); }
	static __device__ __forceinline__ Loaded load(const short *row, const LaneAt &at, long, int) { return fwd_load_s(row, at); }
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int) { return widen_s(r); }
};

// Deep pixels: the finest level reads the uint16_t samples itself (widening and YCoCg-R fused); everything it writes is
// int32, and it leaves every histogram to k_hist (hist_add(.., int))
template <>
struct FwdSrc<Band<SRC_U16>> : FwdInt32 {
	typedef FwdRawS Loaded;
	static __device__ __forceinline__ const uint16_t *base(const LevelArgs &a, int plane, int &)
	{
		return reinterpret_cast<const uint16_t *>(a.src8) + win_off(a.grid, a.src_ps, plane);
	}
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 2); }
	static __device__ __forceinline__ Loaded load(const uint16_t *row, const LaneAt &at, long, int) { return fwd_load_s(row, at); }
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int) { return widen_u(r); }
};

template <>
struct FwdSrc<Band<SRC_RGB16>> : FwdInt32 {
	typedef FwdRawRgb16 Loaded;
	static __device__ __forceinline__ const uint16_t *base(const LevelArgs &a, int plane, int &ch)
	{
		return reinterpret_cast<const uint16_t *>(a.src8) + rgb_window(a, plane, ch);
	}
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 12, 6); }
	static __device__ __forceinline__ Loaded load(const uint16_t *row, const LaneAt &at, long, int)
	{
		const uint2 *m = reinterpret_cast<const uint2 *>(row + at.main);
		const unsigned *e = reinterpret_cast<const unsigned *>(row + at.edge);
		Loaded r = { m[0], m[1], m[2], e[0], e[1], e[2] };
		return r;
	}
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen(r, ch); }
};

template <>
struct FwdSrc<Band<SRC_BGR16>> : FwdSrc<Band<SRC_RGB16>> {
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen<true>(r, ch); }
};

template <>
struct FwdSrc<Band<SRC_RGBP16>> : FwdInt32 {
	typedef FwdRawRgbS3 Loaded;
	static __device__ __forceinline__ const uint16_t *base(const LevelArgs &a, int plane, int &ch) { return FwdSrc<Band<SRC_RGB16>>::base(a, plane, ch); }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 2); }
	static __device__ __forceinline__ Loaded load(const uint16_t *row, const LaneAt &at, long cs, int)
	{
		Loaded r = { fwd_load_s(row, at), fwd_load_s(row + cs, at), fwd_load_s(row + 2 * cs, at) };
		return r;
	}
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen(r, ch); }
};

// Signed pixels: each deep source with the one difference that the samples widen with their sign (image.h:52-65 is reversible on
// any int, and nothing after the widening knows where the samples came from)
template <>
struct FwdSrc<Band<SRC_S16>> : FwdSrc<Band<SRC_U16>> {
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int) { return widen_s(r); }
};
template <>
struct FwdSrc<Band<SRC_RGB16S>> : FwdSrc<Band<SRC_RGB16>> {
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen<false, true>(r, ch); }
};
template <>
struct FwdSrc<Band<SRC_BGR16S>> : FwdSrc<Band<SRC_RGB16>> {
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen<true, true>(r, ch); }
};
template <>
struct FwdSrc<Band<SRC_RGBP16S>> : FwdSrc<Band<SRC_RGBP16>> {
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return widen<true>(r, ch); }
};

template <>
struct FwdSrc<uint8_t> : FwdPacked {
	typedef FwdRaw8 Loaded;
	typedef FwdRaw8 Used;
	static __device__ __forceinline__ const uint8_t *base(const LevelArgs &a, int plane, int &) { return a.src8 + win_off(a.grid, a.src_ps, plane); }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 4); }
	static __device__ __forceinline__ Loaded load(const uint8_t *row, const LaneAt &at, long, int) { return fwd_load_8(row, at); }
};

template <>
struct FwdSrc<Rgb8> : FwdPacked {
	typedef FwdRawRgb Loaded;
	typedef FwdRawRgb Used;
	static constexpr bool RGB_GRID = true;
	static __device__ __forceinline__ const uint8_t *base(const LevelArgs &a, int plane, int &ch) { return a.src8 + rgb_window(a, plane, ch); }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 12, 8); }
	static __device__ __forceinline__ Loaded load(const uint8_t *__restrict__ row, const LaneAt &at, long, int)
	{
		Loaded r = { *reinterpret_cast<const U32x3 *>(row + at.main), *reinterpret_cast<const U32x2 *>(row + at.edge) };
		return r;
	}
};

template <>
struct FwdSrc<RgbP8> : FwdPacked {
	typedef FwdRawRgb3 Loaded;
	typedef FwdRawRgb3 Used;
	static constexpr bool RGB_GRID = true;
	static constexpr int S = 1;   // (a row is six registers: batches of two pairs took the kernel with histograms to 133, three waves per SIMD)
	static __device__ __forceinline__ const uint8_t *base(const LevelArgs &a, int plane, int &ch) { return a.src8 + rgb_window(a, plane, ch); }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 4); }
	// (ch: the channel the workgroup extracts, a constant where this is inlined: Co is R - B and leaves the G plane unloaded)
	static __device__ __forceinline__ Loaded load(const uint8_t *__restrict__ row, const LaneAt &at, long cs, int ch)
	{
		const FwdRaw8 r = fwd_load_8(row, at), b = fwd_load_8(row + 2 * cs, at);
		Loaded o = { r, ch == 1 ? r : fwd_load_8(row + cs, at), b };
		return o;
	}
};

template <>
struct FwdSrc<Rgbx8> : FwdPacked {
	typedef FwdRawRgbx Loaded;
	typedef FwdRawRgbx Used;
	static constexpr bool RGB_GRID = true;
	static __device__ __forceinline__ const uint8_t *base(const LevelArgs &a, int plane, int &ch) { return a.src8 + rgb_window(a, plane, ch); }
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 16, 8); }
	static __device__ __forceinline__ Loaded load(const uint8_t *__restrict__ row, const LaneAt &at, long, int)
	{
		Loaded r = { *reinterpret_cast<const U32x4 *>(row + at.main), *reinterpret_cast<const U32x2 *>(row + at.edge) };
		return r;
	}
};

template <>
struct FwdSrc<Bgr8> : FwdSrc<Rgb8> {
	static __device__ __forceinline__ void lift(const FwdRawRgb &r, int ch, int q, int lane, int nquads, P2 &lo, P2 &hi) { fwd_lift_p(row_p<true>(r, ch), q, lane, nquads, lo, hi); }
};

template <>
struct FwdSrc<Bgrx8> : FwdSrc<Rgbx8> {
	static __device__ __forceinline__ void lift(const FwdRawRgbx &r, int ch, int q, int lane, int nquads, P2 &lo, P2 &hi) { fwd_lift_p(row_p<true>(r, ch), q, lane, nquads, lo, hi); }
};

// ---- delta sources (dwtx_encode_view_delta): the finest level reads a picture S and its base B and lifts S - B ----
// Sources of the int32 family (a residual has twice its pictures' range: no histograms, no 16-bit bands).  A lane loads its quad
// and its edge piece of S and of B — two views with a window stride, a pitch and a grid each, of one layout: the same LaneAt
// serves both — widens both by the sample type, and the row that is lifted is their difference, per colour before image.h:52-65
// (the colour transform rounds: it does not commute with the subtraction).  Both rows' loads travel in one Loaded and are in
// flight together, a batch ahead of their use, as every source's are.
template <typename P>
struct DeltaRows {
	const P *s, *b;   // the same row of the picture's and of the base's window
	int bpitch;
};
// a source's row r from its window's first row: a pointer and the wave's pitch, or both views of a delta source
template <typename Ptr>
__device__ __forceinline__ Ptr row_at(Ptr p, int r, int spitch) { return p + (long)r * spitch; }
template <typename P>
__device__ __forceinline__ DeltaRows<P> row_at(DeltaRows<P> p, int r, int spitch)
{
	DeltaRows<P> o = { p.s + (long)r * spitch, p.b + (long)r * p.bpitch, p.bpitch };
	return o;
}
template <typename Raw>
struct DeltaRaw {
	Raw s, b;
};
template <typename Raw>
__device__ __forceinline__ DeltaRaw<Raw> hold(const DeltaRaw<Raw> &r)
{
	DeltaRaw<Raw> o = { hold(r.s), hold(r.b) };
	return o;
}
__device__ __forceinline__ FwdRaw operator-(const FwdRaw &a, const FwdRaw &b)
{
	FwdRaw o;
	o.x = make_int4(a.x.x - b.x.x, a.x.y - b.x.y, a.x.z - b.x.z, a.x.w - b.x.w);
	o.xr = a.xr - b.xr;
	o.left = make_int2(a.left.x - b.left.x, a.left.y - b.left.y);
	return o;
}
// a gray 8-bit row as ints (fwd_load_8: lane 0's edge word ends in x[4q-2], x[4q-1], the other lanes' begins with x[4q+4])
__device__ __forceinline__ FwdRaw widen_8(const FwdRaw8 &r)
{
	FwdRaw o;
	o.x = make_int4((int)(r.v & 255u), (int)((r.v >> 8) & 255u), (int)((r.v >> 16) & 255u), (int)(r.v >> 24));
	o.xr = (int)(r.edge & 255u);
	o.left = make_int2((int)((r.edge >> 16) & 255u), (int)(r.edge >> 24));
	return o;
}
// byte k (a constant) of a lane's twelve, and of its eight edge bytes
__device__ __forceinline__ int rgb_byte(const U32x3 &v, int k) { return (int)(((k < 4 ? v.x : k < 8 ? v.y : v.z) >> (8 * (k & 3))) & 255u); }
__device__ __forceinline__ int rgb_byte(const U32x2 &v, int k) { return (int)(((k < 4 ? v.x : v.y) >> (8 * (k & 3))) & 255u); }
// channel ch of image.h:52-65 on the difference of two interleaved 8-bit rows (FwdSrc<Rgb8>::load's layout: pixel p of the
// quad in bytes 3p .. 3p+2; the edge: pixel 4q+4 in bytes 0 .. 2, or — lane 0 — pixels 4q-2 and 4q-1 in bytes 2 .. 7)
template <bool BGR>
__device__ __forceinline__ FwdRaw delta_rgb8(const FwdRawRgb &s, const FwdRawRgb &b, int ch)
{
	auto quad = [&](int k) { return ycocg_lies<BGR>(rgb_byte(s.abc, k) - rgb_byte(b.abc, k), rgb_byte(s.abc, k + 1) - rgb_byte(b.abc, k + 1), rgb_byte(s.abc, k + 2) - rgb_byte(b.abc, k + 2), ch); };
	auto edge = [&](int k) { return ycocg_lies<BGR>(rgb_byte(s.e, k) - rgb_byte(b.e, k), rgb_byte(s.e, k + 1) - rgb_byte(b.e, k + 1), rgb_byte(s.e, k + 2) - rgb_byte(b.e, k + 2), ch); };
	FwdRaw o;
	o.x = make_int4(quad(0), quad(3), quad(6), quad(9));
	o.xr = edge(0);
	o.left = make_int2(edge(2), edge(5));
	return o;
}

template <int SRC>
struct FwdDeltaGray : FwdInt32 {
	static constexpr bool DELTA = true;
	typedef typename std::conditional<SRC == SRC_DELTA_U8, uint8_t, uint16_t>::type P;
	typedef typename std::conditional<SRC == SRC_DELTA_U8, FwdRaw8, FwdRawS>::type Raw;
	typedef DeltaRaw<Raw> Loaded;
	static __device__ __forceinline__ DeltaRows<P> rows(const LevelArgsW &A, int plane, int &)
	{
		DeltaRows<P> o = { reinterpret_cast<const P *>(A.a.src8) + win_off(A.a.grid, A.a.src_ps, plane),
			reinterpret_cast<const P *>(A.base8) + win_off(A.bgrid, A.base_ps, plane), A.bpitch };
		return o;
	}
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, SRC == SRC_DELTA_U8 ? 4 : 2); }
	static __device__ __forceinline__ Loaded load(const DeltaRows<P> &row, const LaneAt &at, long, int)
	{
		if constexpr (SRC == SRC_DELTA_U8) {
			Loaded r = { fwd_load_8(row.s, at), fwd_load_8(row.b, at) };
			return r;
		} else {
			Loaded r = { fwd_load_s(row.s, at), fwd_load_s(row.b, at) };
			return r;
		}
	}
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int)
	{
		if constexpr (SRC == SRC_DELTA_U8)
			return widen_8(r.s) - widen_8(r.b);
		else if constexpr (SRC == SRC_DELTA_S16)
			return widen_s(r.s) - widen_s(r.b);
		else
			return widen_u(r.s) - widen_u(r.b);
	}
};
template <>
struct FwdSrc<Band<SRC_DELTA_U8>> : FwdDeltaGray<SRC_DELTA_U8> {};
template <>
struct FwdSrc<Band<SRC_DELTA_U16>> : FwdDeltaGray<SRC_DELTA_U16> {};
template <>
struct FwdSrc<Band<SRC_DELTA_S16>> : FwdDeltaGray<SRC_DELTA_S16> {};

// interleaved 8-bit RGB: a workgroup column per plane, each taking its channel (as the deep interleaved source does)
template <bool BGR>
struct FwdDeltaRgb8 : FwdInt32 {
	static constexpr bool DELTA = true;
	typedef DeltaRaw<FwdRawRgb> Loaded;
	static __device__ __forceinline__ DeltaRows<uint8_t> rows(const LevelArgsW &A, int plane, int &ch)
	{
		ch = plane % 3;
		DeltaRows<uint8_t> o = { A.a.src8 + win_off(A.a.grid, A.a.src_ps, plane / 3), A.base8 + win_off(A.bgrid, A.base_ps, plane / 3), A.bpitch };
		return o;
	}
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 12, 8); }
	static __device__ __forceinline__ Loaded load(const DeltaRows<uint8_t> &row, const LaneAt &at, long, int)
	{
		Loaded r = { FwdSrc<Rgb8>::load(row.s, at, 0, 0), FwdSrc<Rgb8>::load(row.b, at, 0, 0) };
		return r;
	}
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int ch) { return delta_rgb8<BGR>(r.s, r.b, ch); }
};
template <>
struct FwdSrc<Band<SRC_DELTA_RGB8>> : FwdDeltaRgb8<false> {};
template <>
struct FwdSrc<Band<SRC_DELTA_BGR8>> : FwdDeltaRgb8<true> {};

// ---- float sources (dwtx_encode_view_float): the finest level reads fp32, fp16 or bf16 samples and quantises them itself ----
// The picture that is coded, per sample x of colour c: m = fl32(x * scale[c]), r = fl32(m + bias[c]) — two roundings, as the
// line a caller would otherwise write in torch has them, under the pragma float_of() (below, the inverse direction) stands
// under for the same reason —, q = rint(r) (v_rndne_f32: ties to even), clamped to [0, M] with NaN -> 0: both compares are
// false for a NaN, which therefore takes the 0; +inf takes M, -inf and -0.0 become 0.
__device__ __forceinline__ int quant_of(float x, float scale, float bias, float M)
{
#pragma clang fp contract(off)
	const float m = x * scale;
	const float r = m + bias;
	const float q = __builtin_rintf(r);
	const float lo = q >= 0.f ? q : 0.f;
	return (int)(lo > M ? M : lo);
}

// The same quantiser with a lower bound of its own (the *_view_signed calls: what every source runs, L = 0 elsewhere): v = min(max(q, L), M),
// and a NaN becomes 0 BEFORE the clamp — 0 clamped into [L, M] — so that L = 0 gives quant_of above bit for bit: -inf takes L.
__device__ __forceinline__ int quant_of(float x, float scale, float bias, float L, float M)
{
#pragma clang fp contract(off)
	const float m = x * scale;
	const float r = m + bias;
	const float q = __builtin_rintf(r);
	const float z = q == q ? q : 0.f;
	const float lo = z >= L ? z : L;
	return (int)(lo > M ? M : lo);
}

// the 16-bit float types widen exactly (fp16 subnormals kept): which of the two the bits are is uniform (FloatFmt::bf16)
__device__ __forceinline__ float half_float(unsigned bits16, int bf16)
{
	return bf16 ? __builtin_bit_cast(float, bits16 << 16) : (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}

struct Half16;   // (the sample type of the 16-bit float sinks, further down: here the tag of the sources that read either type)

// A row of one plane as it is loaded, F = float: the lane's quad is 16 bytes, its neighbours' two samples 8 (lane 0: x[4q-2],
// x[4q-1]; the other lanes: the first is x[4q+4]); F = Half16: the 8 and 4 bytes of a deep gray row (FwdRawS).  Both inside
// the row's own W samples, as every source's.
template <typename F>
struct FwdRawF {
	uint4 x;
	uint2 e;
};
template <>
struct FwdRawF<Half16> : FwdRawS {};

__device__ __forceinline__ FwdRawF<float> fwd_load_f(const float *__restrict__ row, const LaneAt &at)
{
	FwdRawF<float> r = { *reinterpret_cast<const uint4 *>(row + at.main), *reinterpret_cast<const uint2 *>(row + at.edge) };
	return r;
}
__device__ __forceinline__ FwdRawF<Half16> fwd_load_f(const uint16_t *__restrict__ row, const LaneAt &at)
{
	FwdRawF<Half16> r;
	static_cast<FwdRawS &>(r) = fwd_load_s(row, at);
	return r;
}
__device__ __forceinline__ FwdRawF<float> hold(const FwdRawF<float> &r)
{
	FwdRawF<float> o = { make_uint4(hold(r.x.x), hold(r.x.y), hold(r.x.z), hold(r.x.w)), hold(r.e) };
	return o;
}
__device__ __forceinline__ FwdRawF<Half16> hold(const FwdRawF<Half16> &r)
{
	FwdRawF<Half16> o;
	static_cast<FwdRawS &>(o) = hold(static_cast<const FwdRawS &>(r));
	return o;
}

// the six samples of a loaded row, quantised with colour c's scale and bias (c: uniform)
struct Quant6 {
	int x0, x1, x2, x3, e0, e1;
};
__device__ __forceinline__ Quant6 quant_row(const FwdRawF<float> &r, const LevelArgsW &A, int c)
{
	const float s = A.fmt.scale[c], b = A.fmt.bias[c], L = (float)A.a.minval, M = (float)A.a.maxval;
	auto q = [s, b, L, M](unsigned bits) { return quant_of(__builtin_bit_cast(float, bits), s, b, L, M); };
	Quant6 o = { q(r.x.x), q(r.x.y), q(r.x.z), q(r.x.w), q(r.e.x), q(r.e.y) };
	return o;
}
__device__ __forceinline__ Quant6 quant_row(const FwdRawF<Half16> &r, const LevelArgsW &A, int c)
{
	const float s = A.fmt.scale[c], b = A.fmt.bias[c], L = (float)A.a.minval, M = (float)A.a.maxval;
	const int bf16 = A.fmt.bf16;
	auto q = [s, b, L, M, bf16](unsigned bits16) { return quant_of(half_float(bits16, bf16), s, b, L, M); };
	Quant6 o = { q(r.x.x & 0xffffu), q(r.x.x >> 16), q(r.x.y & 0xffffu), q(r.x.y >> 16), q(r.e & 0xffffu), q(r.e >> 16) };
	return o;
}
// ... as the row an 8-bit gray source loads (M <= 255: every value is a byte): everything after the load is that source's
__device__ __forceinline__ FwdRaw8 raw8_of(const Quant6 &v)
{
	FwdRaw8 o = { (unsigned)v.x0 | ((unsigned)v.x1 << 8) | ((unsigned)v.x2 << 16) | ((unsigned)v.x3 << 24),
		(unsigned)v.e0 | ((unsigned)v.e0 << 16) | ((unsigned)v.e1 << 24) };   // (byte 0: x[4q+4]; bytes 2, 3 — lane 0 —: x[4q-2], x[4q-1])
	return o;
}
// ... and as the widened row of the int32 arithmetic (deep quantised values)
__device__ __forceinline__ FwdRaw raw_of(const Quant6 &v)
{
	FwdRaw o;
	o.x = make_int4(v.x0, v.x1, v.x2, v.x3);
	o.xr = v.e0;
	o.left = make_int2(v.e0, v.e1);
	return o;
}

// The sources' names: F = float or Half16 (fp16 and bf16 share a kernel, as in the sinks), gray or planar RGB (in either
// order: the host hands the R plane and a signed stride, as to RgbP8), and the route.  DEEP false — maxval <= 255 —: the row
// becomes the packed row of the 8-bit source of its layout when it is used (FwdRaw8 / FwdRawRgb3: cur[] holds two / six
// registers a row, only nxt[] the floats) and the level is that source's: packed arithmetic, histograms, 16-bit bands, the
// three channels of a strip side by side.  DEEP true: the int32 arithmetic of the deep sources, no histograms, a workgroup
// column per plane.  used() takes the launch's arguments for the format (FLOAT: fwd_level_body calls it that way).
template <typename F, bool PLANAR, bool DEEP>
struct FloatPix {};

// a planar window's three rows
template <typename F>
struct FwdRawF3 {
	FwdRawF<F> r, g, b;
};
template <typename F>
__device__ __forceinline__ FwdRawF3<F> hold(const FwdRawF3<F> &p)
{
	FwdRawF3<F> o = { hold(p.r), hold(p.g), hold(p.b) };
	return o;
}

template <typename F>
struct FwdFloatRows {
	typedef typename std::conditional<std::is_same<F, float>::value, float, uint16_t>::type Sample;
	static __device__ __forceinline__ LaneAt at(int q, int lane, int nquads) { return lane_at(q, lane, nquads, 4, 2); }
	static __device__ __forceinline__ const Sample *pixels(const LevelArgs &a) { return reinterpret_cast<const Sample *>(a.src8); }
	// (ch: a constant where this is inlined for the 8-bit route: Co is R - B and leaves the G plane unloaded; below 0: all three)
	static __device__ __forceinline__ FwdRawF3<F> load3(const Sample *__restrict__ row, const LaneAt &at, long cs, int ch)
	{
		const FwdRawF<F> r = fwd_load_f(row, at), b = fwd_load_f(row + 2 * cs, at);
		FwdRawF3<F> o = { r, ch == 1 ? r : fwd_load_f(row + cs, at), b };
		return o;
	}
};

template <typename F>
struct FwdSrc<FloatPix<F, false, false>> : FwdPacked, FwdFloatRows<F> {
	static constexpr bool FLOAT = true;
	typedef FwdRawF<F> Loaded;
	typedef FwdRaw8 Used;
	using typename FwdFloatRows<F>::Sample;
	static __device__ __forceinline__ const Sample *base(const LevelArgs &a, int plane, int &) { return FwdFloatRows<F>::pixels(a) + win_off(a.grid, a.src_ps, plane); }
	static __device__ __forceinline__ Loaded load(const Sample *row, const LaneAt &at, long, int) { return fwd_load_f(row, at); }
	static __device__ __forceinline__ Used used(const Loaded &r, int, const LevelArgsW &A) { return raw8_of(quant_row(r, A, 0)); }
};

template <typename F>
struct FwdSrc<FloatPix<F, true, false>> : FwdPacked, FwdFloatRows<F> {
	static constexpr bool FLOAT = true;
	typedef FwdRawF3<F> Loaded;
	typedef FwdRawRgb3 Used;
	using typename FwdFloatRows<F>::Sample;
	static constexpr bool RGB_GRID = true;
	static constexpr int S = 1;   // (as RgbP8)
	static __device__ __forceinline__ const Sample *base(const LevelArgs &a, int plane, int &ch) { return FwdFloatRows<F>::pixels(a) + rgb_window(a, plane, ch); }
	static __device__ __forceinline__ Loaded load(const Sample *row, const LaneAt &at, long cs, int ch) { return FwdFloatRows<F>::load3(row, at, cs, ch); }
	static __device__ __forceinline__ Used used(const Loaded &p, int ch, const LevelArgsW &A)
	{
		const FwdRaw8 r = raw8_of(quant_row(p.r, A, 0)), b = raw8_of(quant_row(p.b, A, 2));
		Used o = { r, ch == 1 ? r : raw8_of(quant_row(p.g, A, 1)), b };
		return o;
	}
};

template <typename F>
struct FwdSrc<FloatPix<F, false, true>> : FwdInt32, FwdFloatRows<F> {
	static constexpr bool FLOAT = true;
	typedef FwdRawF<F> Loaded;
	using typename FwdFloatRows<F>::Sample;
	static __device__ __forceinline__ const Sample *base(const LevelArgs &a, int plane, int &) { return FwdFloatRows<F>::pixels(a) + win_off(a.grid, a.src_ps, plane); }
	static __device__ __forceinline__ Loaded load(const Sample *row, const LaneAt &at, long, int) { return fwd_load_f(row, at); }
	static __device__ __forceinline__ FwdRaw used(const Loaded &r, int, const LevelArgsW &A) { return raw_of(quant_row(r, A, 0)); }
};

template <typename F>
struct FwdSrc<FloatPix<F, true, true>> : FwdInt32, FwdFloatRows<F> {
	static constexpr bool FLOAT = true;
	typedef FwdRawF3<F> Loaded;
	using typename FwdFloatRows<F>::Sample;
	static __device__ __forceinline__ const Sample *base(const LevelArgs &a, int plane, int &ch) { return FwdFloatRows<F>::pixels(a) + rgb_window(a, plane, ch); }
	static __device__ __forceinline__ Loaded load(const Sample *row, const LaneAt &at, long cs, int) { return FwdFloatRows<F>::load3(row, at, cs, -1); }
	static __device__ __forceinline__ FwdRaw used(const Loaded &p, int ch, const LevelArgsW &A)
	{
		const Quant6 r = quant_row(p.r, A, 0), g = quant_row(p.g, A, 1), b = quant_row(p.b, A, 2);
		const Quant6 o = { ycocg_ch(r.x0, g.x0, b.x0, ch), ycocg_ch(r.x1, g.x1, b.x1, ch), ycocg_ch(r.x2, g.x2, b.x2, ch), ycocg_ch(r.x3, g.x3, b.x3, ch),
			ycocg_ch(r.e0, g.e0, b.e0, ch), ycocg_ch(r.e1, g.e1, b.e1, ch) };
		return raw_of(o);
	}
};

// One wide forward level of the wave's strip, for every source (FwdSrc above): int32 planes on every level of
// dwtx_transformation_fwd and below the finest in the codec, pixels on the codec's finest.
// Memory operations retire in order on this part (one counter for loads and stores): a wave that waits for rows it
// loaded also waits for everything it issued before them, and a wait the compiler cannot count exactly waits for
// everything.  So the loop works in batches of S row pairs: wait once (where the rows are moved to the registers they
// are used from), send the previous batch's results out, ask for the next batch's rows, then compute S row pairs
// without touching memory — by the next wait both the stores and the loads are a whole batch of arithmetic old.
// CH: the YCoCg-R channel the workgroup extracts as a compile-time constant (the 8-bit RGB sources, whose kernel branches
// — uniformly — into the three instances: Co is one subtraction per pixel pair, and neither it nor Cg needs what only Y needs;
// with the channel as a run-time value every workgroup computed all three and selected: 1.84 -> 1.6 ms per 256 frames of
// 1080p); below 0: whatever base() says, a run-time uniform.
// FY: the windows are a flipped call's whose flags are 0 or DWTX_FLIP_Y (dwtx_pixels::flip_wide): the wave takes its window's
// offset and flag from the table entry (win_off_flip) and, bottom-up, starts at the window's last row in memory with the
// pitch negated — picture row r is memory row h - 1 - r, every address it forms is one the upright walk forms, and the
// columns, the halo words and the quad alignment are untouched.  Instances of their own: the others keep their code.
template <typename Src, bool HIST, int CH, bool FY = false>
__device__ __forceinline__ void fwd_level_body(const LevelArgsW &A, int bx, int by)
{
	typedef FwdSrc<Src> T;
	typedef typename T::Pair Pair;
	const LevelArgs &a = A.a;
	// (the RGB sources' histogram kernels hold three bodies and spill scalar registers already: there the index stays per lane)
	const int lane = threadIdx.x & 63, wv = HIST && T::RGB_GRID ? (int)(threadIdx.x >> 6) : wave_in_block();
	const int sx = (bx << A.wx_log2) + (wv & ((1 << A.wx_log2) - 1));   // the wave's strip of 64 quads
	const int q = sx * 64 + lane;
	const int j0 = (by * (WAVES >> A.wx_log2) + (wv >> A.wx_log2)) * a.rpw;
	if (j0 >= a.h2 || sx * 64 >= A.nquads)
		return;
	const int j1 = min(j0 + a.rpw, a.h2);
	const int plane = T::RGB_GRID ? (int)blockIdx.z * 3 + CH : (int)blockIdx.z;
	const bool valid = q < A.nquads;
	int ch_rt = 0;
	int spitch = a.spitch;   // (the wave's: negated for a bottom-up window)
	const auto src = [&] {
		if constexpr (T::DELTA) {
			return T::rows(A, plane, ch_rt);
		} else if constexpr (FY) {
			LevelArgs b = a;   // base() without a window: the pixels' first sample and the channel
			b.grid = WinGrid{ 0u, 0u, 0, nullptr };
			b.src_ps = 0;
			unsigned flags;
			auto p = T::base(b, plane, ch_rt) + win_off_flip(a.grid, A.ppw == 3 ? plane / 3 : plane, flags);
			if (flags & DWTX_FLIP_Y) {
				p += (long)(a.h - 1) * a.spitch;
				spitch = -spitch;
			}
			return p;
		} else {
			return T::base(a, plane, ch_rt);
		}
	}();
	const int ch = CH >= 0 ? CH : ch_rt;   // (uniform)
	int *ll = a.ll + plane * a.ll_ps;
	short *ll16 = a.ll16 ? a.ll16 + plane * a.ll_ps : nullptr;   // (uniform)
	int *det = a.det + plane * a.det_ps;
	short *det16 = T::det16(a, plane);

	constexpr int S = T::S;
	const int jfirst = j0 > 0 ? j0 - 1 : 0;
	const LaneAt at = T::at(q, lane, A.nquads);
	const Pair zero = {};
	Pair l0, h0, pl = zero, ph = zero;
	auto use = [&](const typename T::Loaded &r) {
		if constexpr (T::FLOAT)
			return T::used(r, ch, A);
		else
			return T::used(r, ch);
	};
	T::lift(use(T::load(row_at(src, 2 * jfirst, spitch), at, A.cstride, ch)), ch, q, lane, A.nquads, l0, h0);
	auto rowp = [&](int r) { return row_at(src, min(r, a.h - 1), spitch); };
	typename T::Used cur[2 * S];
	typename T::Loaded nxt[2 * S];
#pragma unroll
	for (int k = 0; k < 2 * S; ++k)
		nxt[k] = T::load(rowp(2 * jfirst + 1 + k), at, A.cstride, ch);
	Pair osl[S], osh[S], odl[S], odh[S];   // a batch's results wait here for the next iteration's stores
	auto store_batch = [&](int jb) {
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int j = jb + s;
			if (j >= j0 && j < j1 && valid) {
				const bool odd_in = 2 * j + 1 < a.h;
				if (ll16)
					st2(ll16 + (long)j * a.llpitch + 2 * q, osl[s]);
				else
					st2(ll + (long)j * a.llpitch + 2 * q, osl[s]);
				if (T::details16(det16)) {
					st2(det16 + (long)j * a.dpitch + a.w2 + 2 * q, osh[s]);
					if (odd_in) {
						st2(det16 + (long)(a.h2 + j) * a.dpitch + 2 * q, odl[s]);
						st2(det16 + (long)(a.h2 + j) * a.dpitch + a.w2 + 2 * q, odh[s]);
					}
				} else {
					st2(det + (long)j * a.dpitch + a.w2 + 2 * q, osh[s]);
					if (odd_in) {
						st2(det + (long)(a.h2 + j) * a.dpitch + 2 * q, odl[s]);
						st2(det + (long)(a.h2 + j) * a.dpitch + a.w2 + 2 * q, odh[s]);
					}
				}
			}
		}
	};
	HistAcc hHL = { 0, 0, 0, 0 }, hLH = { 0, 0, 0, 0 }, hHH = { 0, 0, 0, 0 };
	auto flush = [&](HistAcc &h, int hbx, int hby) {
		h.mx = hist_mx(h.mx, Pair());
		hist_flush(h, A.hist, plane, hbx, hby, lane);
	};
	for (int jb = jfirst; jb < j1; jb += S) {
#pragma unroll
		for (int k = 0; k < 2 * S; ++k)
			cur[k] = use(hold(nxt[k]));   // the one wait of the iteration: everything outstanding is a batch old
		if (jb > jfirst)
			store_batch(jb - S);
		if (jb + S < j1) {
#pragma unroll
			for (int k = 0; k < 2 * S; ++k)
				nxt[k] = T::load(rowp(2 * (jb + S) + 1 + k), at, A.cstride, ch);
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int jj = jb + s;
			if (jj >= j1)
				break;
			const int r1 = 2 * jj + 1, r2 = r1 + 1;
			const bool odd_in = r1 < a.h;
			Pair l1 = zero, h1 = zero, l2 = l0, h2v = h0;
			if (odd_in)
				T::lift(cur[2 * s], ch, q, lane, A.nquads, l1, h1);
			if (r2 < a.h)
				T::lift(cur[2 * s + 1], ch, q, lane, A.nquads, l2, h2v);
			const Pair dl = lift_pred(l1, l0, l2);
			const Pair dh = lift_pred(h1, h0, h2v);
			Pair sl = l0, sh = h0;
			if (odd_in) {    // an odd-height plane leaves its last even row untouched
				sl = lift_upd(l0, jj ? pl : dl, dl);
				sh = lift_upd(h0, jj ? ph : dh, dh);
			}
			osl[s] = sl;
			osh[s] = sh;
			odl[s] = dl;
			odh[s] = dh;
			if (HIST && jj >= j0) {
				// the detail coefficients of this row pair (cdf53.h:9-34 output): HL row jj, LH and HH row h2 + jj
				if (valid) {
					hist_add(hHL, sh);
					if (odd_in) {
						hist_add(hLH, dl);
						hist_add(hHH, dh);
					}
				}
				if ((jj & 3) == 3) {   // eight coefficients per subband since the last fold: a nibble holds fifteen
					hist_fold(hHL);
					hist_fold(hLH);
					hist_fold(hHH);
				}
				// a block ends where its 32 rows end (or the strip does): the rows of HL are jj, those of LH / HH h2 + jj
				const bool last = jj == j1 - 1;
				const int bxl = (2 * q) >> 5, bxh = (a.w2 + 2 * q) >> 5;
				if (last || ((jj + 1) & 31) == 0)
					flush(hHL, bxh, jj >> 5);
				if (last || ((a.h2 + jj + 1) & 31) == 0) {
					flush(hLH, bxl, (a.h2 + jj) >> 5);
					flush(hHH, bxh, (a.h2 + jj) >> 5);
				}
			}
			pl = dl;
			ph = dh;
			l0 = l2;
			h0 = h2v;
		}
	}
	store_batch(jfirst + (j1 - 1 - jfirst) / S * S);   // the last batch (a strip has at least one row pair)
}

// The two entry points pick the strip mapping and the channel dispatch.  k_fwd_level_w: bands and deep pixels, a workgroup
// column per plane.  k_fwd_pixels_w: 8-bit pixels.
template <bool HIST, int SRC, bool FY = false>
__global__ __launch_bounds__(64 * WAVES) void k_fwd_level_w(LevelArgsW A)
{
	int bx, by;
	xcd_strip(bx, by);
	fwd_level_body<Band<SRC>, HIST, -1, FY>(A, bx, by);
}

template <typename SrcT, bool HIST, bool FY = false>
__global__ __launch_bounds__(64 * WAVES) void k_fwd_pixels_w(LevelArgsW A)
{
	int bx, by, chan = 0;
	if (FwdSrc<SrcT>::RGB_GRID) {
		xcd_strip_rgb(bx, by, chan);
		if (chan == 0)
			fwd_level_body<SrcT, HIST, 0, FY>(A, bx, by);
		else if (chan == 1)
			fwd_level_body<SrcT, HIST, 1, FY>(A, bx, by);
		else
			fwd_level_body<SrcT, HIST, 2, FY>(A, bx, by);
	} else {
		xcd_strip(bx, by);
		fwd_level_body<SrcT, HIST, 0, FY>(A, bx, by);
	}
}

// k_fwd_float_w: float pixels (FloatPix<>).  The 8-bit route's planar RGB as k_fwd_pixels_w runs RgbP8; gray and the deep
// route a workgroup column per plane, the channel whatever base() says.
template <typename SrcT, bool HIST, bool FY = false>
__global__ __launch_bounds__(64 * WAVES) void k_fwd_float_w(LevelArgsW A)
{
	int bx, by, chan = 0;
	if (FwdSrc<SrcT>::RGB_GRID) {
		xcd_strip_rgb(bx, by, chan);
		if (chan == 0)
			fwd_level_body<SrcT, HIST, 0, FY>(A, bx, by);
		else if (chan == 1)
			fwd_level_body<SrcT, HIST, 1, FY>(A, bx, by);
		else
			fwd_level_body<SrcT, HIST, 2, FY>(A, bx, by);
	} else {
		xcd_strip(bx, by);
		fwd_level_body<SrcT, HIST, -1, FY>(A, bx, by);
	}
}

// ---------------------------------------------------------------- inverse ---
// LL | HL | LH | HH samples of one row pair as they are loaded (F16: the detail bands are words of two 16-bit values,
// widened when used).  Every lane loads — lanes outside the row from a clamped quad, row pairs beyond the band from
// the last one — so that no load sits behind a branch or feeds a select; what those get is never used.
template <bool F16>
struct InvRawT {
	int2 sl, sh, dl, dh;
};
template <>
struct InvRawT<true> {
	int2 sl;
	unsigned sh, dl, dh;
};

__device__ __forceinline__ int2 ld2(const int *p) { return *reinterpret_cast<const int2 *>(p); }

// where a lane reads: its (clamped) column pair, and the clamps for the row pair index
struct InvAt {
	int col;          // 2 * clamped quad
	int jmax, jdmax;  // last row pair of the LL / HL bands, last of the LH / HH bands (an odd height has one row less there)
	int colr, coll;   // the column after the lane's pair and the one before it (clamped to the band)
};

__device__ __forceinline__ InvAt inv_at(const LevelArgs &a, int qd, int nquads)
{
	const int col = 2 * min(max(qd, 0), nquads - 1);
	InvAt o = { col, a.h2 - 1, a.h / 2 - 1, min(col + 2, 2 * nquads - 1), max(col - 1, 0) };
	return o;
}

// The columns next to a lane's pair, as loaded: the inverse undoes the columns first, so the row step of a wave's
// first and last lane needs its neighbours' samples AFTER their column step — every lane carries the column to the
// right of its pair (both bands) and the high band's column to its left through the column step as well; only lanes
// 0 and 63 use them (the others get the same values from their neighbours' registers), and what all 64 lanes load
// for them are lines their neighbours load anyway.  (Before: waves that overlapped by eight lanes of 64, i.e. 14 %
// more rows loaded than written.)
struct InvHalo {
	int sl_r, sh_r, dl_r, dh_r;   // LL | HL | LH | HH at column 2q+2
	int sh_l, dh_l;               // HL | HH at column 2q-1
};

__device__ __forceinline__ InvHalo inv_load_halo(const LevelArgs &a, const int *llp, const int *det, int j, const InvAt &at)
{
	InvHalo r;
	const int ja = min(j, at.jmax), jd = min(j, at.jdmax);
	r.sl_r = llp[(long)ja * a.spitch + at.colr];
	r.sh_r = det[(long)ja * a.dpitch + a.w2 + at.colr];
	r.dl_r = det[(long)(a.h2 + jd) * a.dpitch + at.colr];
	r.dh_r = det[(long)(a.h2 + jd) * a.dpitch + a.w2 + at.colr];
	r.sh_l = det[(long)ja * a.dpitch + a.w2 + at.coll];
	r.dh_l = det[(long)(a.h2 + jd) * a.dpitch + a.w2 + at.coll];
	return r;
}

__device__ __forceinline__ InvHalo inv_load_halo(const LevelArgs &a, const int *llp, const short *det16, int j, const InvAt &at)
{
	InvHalo r;   // (16-bit bands: the load itself widens)
	const int ja = min(j, at.jmax), jd = min(j, at.jdmax);
	r.sl_r = llp[(long)ja * a.spitch + at.colr];
	r.sh_r = det16[(long)ja * a.dpitch + a.w2 + at.colr];
	r.dl_r = det16[(long)(a.h2 + jd) * a.dpitch + at.colr];
	r.dh_r = det16[(long)(a.h2 + jd) * a.dpitch + a.w2 + at.colr];
	r.sh_l = det16[(long)ja * a.dpitch + a.w2 + at.coll];
	r.dh_l = det16[(long)(a.h2 + jd) * a.dpitch + a.w2 + at.coll];
	return r;
}

// the halo columns as one more pair per band: .a = the column to the right, .b = the column to the left (high band only)
struct HaloPairs {
	I2 sl, sh, dl, dh;
};

__device__ __forceinline__ InvRawT<false> inv_load_w(const LevelArgs &a, const int *llp, const int *det, int j, const InvAt &at)
{
	InvRawT<false> r;
	const int ja = min(j, at.jmax), jd = min(j, at.jdmax);
	r.sl = ld2(llp + (long)ja * a.spitch + at.col);
	r.sh = ld2(det + (long)ja * a.dpitch + a.w2 + at.col);
	r.dl = ld2(det + (long)(a.h2 + jd) * a.dpitch + at.col);
	r.dh = ld2(det + (long)(a.h2 + jd) * a.dpitch + a.w2 + at.col);
	return r;
}

__device__ __forceinline__ InvRawT<true> inv_load_w(const LevelArgs &a, const int *llp, const short *det16, int j, const InvAt &at)
{
	InvRawT<true> r;
	const int ja = min(j, at.jmax), jd = min(j, at.jdmax);
	r.sl = ld2(llp + (long)ja * a.spitch + at.col);
	r.sh = *reinterpret_cast<const unsigned *>(det16 + (long)ja * a.dpitch + a.w2 + at.col);
	r.dl = *reinterpret_cast<const unsigned *>(det16 + (long)(a.h2 + jd) * a.dpitch + at.col);
	r.dh = *reinterpret_cast<const unsigned *>(det16 + (long)(a.h2 + jd) * a.dpitch + a.w2 + at.col);
	return r;
}

__device__ __forceinline__ int2 hold(int2 v) { return make_int2(hold(v.x), hold(v.y)); }
__device__ __forceinline__ InvRawT<false> hold(const InvRawT<false> &r)
{
	InvRawT<false> o = { hold(r.sl), hold(r.sh), hold(r.dl), hold(r.dh) };
	return o;
}
__device__ __forceinline__ InvRawT<true> hold(const InvRawT<true> &r)
{
	InvRawT<true> o = { hold(r.sl), hold(r.sh), hold(r.dl), hold(r.dh) };
	return o;
}

__device__ __forceinline__ I2 to_i2(int2 v)
{
	I2 r = { v.x, v.y };
	return r;
}
__device__ __forceinline__ I2 to_i2(I2 v) { return v; }

__device__ __forceinline__ HaloPairs hold(const InvHalo &r)
{
	HaloPairs o;
	o.sl.a = hold(r.sl_r);
	o.sl.b = 0;
	o.sh.a = hold(r.sh_r);
	o.sh.b = hold(r.sh_l);
	o.dl.a = hold(r.dl_r);
	o.dl.b = 0;
	o.dh.a = hold(r.dh_r);
	o.dh.b = hold(r.dh_l);
	return o;
}
__device__ __forceinline__ HaloPairs as_pairs(const InvHalo &r)
{
	HaloPairs o = { { r.sl_r, 0 }, { r.sh_r, r.sh_l }, { r.dl_r, 0 }, { r.dh_r, r.dh_l } };
	return o;
}

__device__ __forceinline__ I2 to_i2(unsigned u)   // two 16-bit values
{
	I2 r = { (int)(short)(u & 0xffffu), (int)u >> 16 };
	return r;
}

// the plane's detail bands as the kernel variant reads them
template <bool F16>
struct DetPtr {
	typedef const int *type;
	static __device__ __forceinline__ type of(const LevelArgs &a, long plane) { return a.det + plane * a.det_ps; }
};
template <>
struct DetPtr<true> {
	typedef const short *type;
	static __device__ __forceinline__ type of(const LevelArgs &a, long plane) { return a.det16 + plane * a.det_ps; }
};

// horizontal inverse of one output row for this lane's two pairs: x[4qd .. 4qd+3]
struct Quad4 {
	int v[4];
};
// the FL 2 instances: a mirrored window's quad, its four pixels the other way round, and where it goes (flip_dst)
template <int FL>
__device__ __forceinline__ Quad4 flip_quad(const Quad4 &q, bool fx)
{
	if constexpr (FL != 2) {
		return q;
	} else {
		Quad4 r = { { fx ? q.v[3] : q.v[0], fx ? q.v[2] : q.v[1], fx ? q.v[1] : q.v[2], fx ? q.v[0] : q.v[3] } };
		return r;
	}
}
template <int FL>
__device__ __forceinline__ int flip_q(int q, int fwq, bool fx)
{
	if constexpr (FL != 2)
		return q;
	else
		return fx ? fwq - 1 - q : q;
}

__device__ __forceinline__ Quad4 inv_row_vals(int qd, int nquads, I2 lo, I2 hi)
{
	int hl = __shfl_up(hi.b, 1);
	if (qd <= 0)
		hl = hi.a;
	const int e0 = lo.a - tdiv4(hl + hi.a);
	const int e1 = lo.b - tdiv4(hi.a + hi.b);
	int er = __shfl_down(e0, 1);
	if (qd + 1 >= nquads)
		er = e1;
	Quad4 r;
	r.v[0] = e0;
	r.v[1] = hi.a + tdiv2(e0 + e1);
	r.v[2] = e1;
	r.v[3] = hi.b + tdiv2(e1 + er);
	return r;
}

// a finished output row in the registers it waits in for its store: four int32 samples, or four clamped 8-bit pixels (pnm.h:108)
template <typename DstT>
struct OutRow {
	typedef int4 type;
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp) { return make_int4(v.v[0], v.v[1], v.v[2], v.v[3]); }
	static __device__ __forceinline__ void store(int *__restrict__ row, int qd, const type &v) { *reinterpret_cast<int4 *>(row + 4 * qd) = v; }
};
// four deep pixels clamped to [0, maxval] (pnm.h:108 with the picture's maxval for 255; signed ones to [minval, maxval]): 8 bytes per lane
template <>
struct OutRow<uint16_t> {
	typedef uint2 type;
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp M)
	{
		auto c = [M](int x) { return (unsigned)(x < M.lo ? M.lo : x > M.hi ? M.hi : x) & 0xffffu; };   // (two's complement: int16_t samples)
		return make_uint2(c(v.v[0]) | (c(v.v[1]) << 16), c(v.v[2]) | (c(v.v[3]) << 16));
	}
	static __device__ __forceinline__ void store(uint16_t *__restrict__ row, int qd, const type &v) { *reinterpret_cast<uint2 *>(row + 4 * qd) = v; }
};
template <>
struct OutRow<uint8_t> {
	typedef unsigned type;
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp)
	{
		auto c8 = [](int x) { return (unsigned)(x < 0 ? 0 : x > 255 ? 255 : x); };
		return c8(v.v[0]) | (c8(v.v[1]) << 8) | (c8(v.v[2]) << 16) | (c8(v.v[3]) << 24);
	}
	static __device__ __forceinline__ void store(uint8_t *__restrict__ row, int qd, const type &v) { *reinterpret_cast<unsigned *>(row + 4 * qd) = v; }
};

// ---- delta sinks (dwtx_decode_view_delta): the finest level adds the base pictures' samples and clamps twice ----
// DeltaPix<P> as a kernel's DstT / PixT: the pixels are P samples (uint8_t, uint16_t, int16_t) of a delta view.  A lane loads the
// quad of the base B that lies where its own quad goes — from the base's own window, pitch and grid (LevelArgsW::base8 ..), a
// batch ahead of its use, as every row is — and the sample it writes is min(max(B + d, lo), hi), d the inverse transform's value
// under the clamps of the range [-R, R], R = hi - lo (R may be 65535: ints throughout).  Every sample is read and written by the
// same lane, the read a batch before the write, and the lanes and rows that only ride along (halo lanes, clamped rows) use nothing
// of what they load: the base may be the destination itself (the in-place decode).  InvPix: what a kernel's pointer counts.
template <typename P>
struct DeltaPix {};
struct NoBase {};   // the rows of a base in a kernel instance that has none
__device__ __forceinline__ NoBase hold(NoBase) { return NoBase{}; }
template <typename DstT>
struct InvPix {
	typedef DstT type;
	typedef NoBase base;
	static constexpr bool DELTA = false;
};
template <typename P>
struct OutRow<DeltaPix<P>> {
	typedef typename std::conditional<sizeof(P) == 1, unsigned, uint2>::type type;   // four samples: the finished row, and the base's quad as it is loaded
	static __device__ __forceinline__ type load(const P *row, int qd) { return *reinterpret_cast<const type *>(row + 4 * qd); }
	static __device__ __forceinline__ int base_of(unsigned b, int k) { return (int)((b >> (8 * k)) & 255u); }
	static __device__ __forceinline__ int base_of(uint2 b, int k)
	{
		const unsigned w = k < 2 ? b.x : b.y;
		if (std::is_signed<P>::value)
			return k & 1 ? (int)w >> 16 : (int)(short)(w & 0xffffu);
		return (int)(k & 1 ? w >> 16 : w & 0xffffu);
	}
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp M, const type &b)
	{
		unsigned o[4];
#pragma unroll
		for (int k = 0; k < 4; ++k)
			o[k] = (unsigned)delta_sample(v.v[k], base_of(b, k), M);
		if constexpr (sizeof(P) == 1)
			return o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
		else
			return make_uint2((o[0] & 0xffffu) | (o[1] << 16), (o[2] & 0xffffu) | (o[3] << 16));   // (two's complement: int16_t samples)
	}
	static __device__ __forceinline__ void store(P *row, int qd, const type &v) { *reinterpret_cast<type *>(row + 4 * qd) = v; }
};
template <typename P>
struct InvPix<DeltaPix<P>> {
	typedef P type;
	typedef typename OutRow<DeltaPix<P>>::type base;
	static constexpr bool DELTA = true;
};

// ---- float sinks: the value an integer sink would write, as a float: v * scale + bias in fp32, then the sample's type ----
// Two roundings, as torch's unfused `x.float() * scale + bias` has them.  hipcc contracts a * b + c into an fma by default, and
// __fmul_rn / __fadd_rn are plain operators in a header compiled that way — they fuse all the same (v_fma_f32, and
// v_fma_mixlo_f16 straight into the half) — so the two operations stand here, under a pragma that forbids it.
__device__ __forceinline__ float float_of(int v, float scale, float bias)
{
#pragma clang fp contract(off)
	const float m = (float)v * scale;
	return m + bias;
}
// round to nearest even, overflow to infinity, subnormals kept: v_cvt_f16_f32 / v_cvt_pk_f16_f32 and v_cvt_pk_bf16_f32 under the
// default rounding mode (the compiler picks the packed forms itself; never v_cvt_pkrtz_f16_f32, which truncates)
__device__ __forceinline__ unsigned f16_bits(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ unsigned bf16_bits(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)f); }
// four 16-bit floats of either type (uniform choice: a scalar branch)
__device__ __forceinline__ uint2 half_quad(const float (&f)[4], int bf16)
{
	if (bf16)
		return make_uint2(bf16_bits(f[0]) | (bf16_bits(f[1]) << 16), bf16_bits(f[2]) | (bf16_bits(f[3]) << 16));
	return make_uint2(f16_bits(f[0]) | (f16_bits(f[1]) << 16), f16_bits(f[2]) | (f16_bits(f[3]) << 16));
}
// the sample type of the wide kernels' 16-bit float sinks: fp16 or bf16, FloatFmt::bf16 says which
struct Half16 {
	uint16_t bits;
};
// value: a float sink, whose of() takes the conversion; AT_STORE: its RGB sink converts in store() instead (see RgbOut<float, PIX_PLANAR>)
template <typename T>
struct FloatSample {
	static constexpr bool value = false, AT_STORE = false;
};
template <>
struct FloatSample<float> {
	static constexpr bool value = true, AT_STORE = true;
};
template <>
struct FloatSample<Half16> {
	static constexpr bool value = true, AT_STORE = false;
};
// four gray pixels clamped to [0, M] (pnm.h:108 at the picture's maxval) as floats: 16 bytes per lane, 8 of the half types
template <>
struct OutRow<float> {
	typedef float4 type;
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp M, const FloatFmt &f)
	{
		auto c = [M, &f](int x) { return float_of(x < M.lo ? M.lo : x > M.hi ? M.hi : x, f.scale[0], f.bias[0]); };
		return make_float4(c(v.v[0]), c(v.v[1]), c(v.v[2]), c(v.v[3]));
	}
	static __device__ __forceinline__ void store(float *__restrict__ row, int qd, const type &v) { *reinterpret_cast<float4 *>(row + 4 * qd) = v; }
};
template <>
struct OutRow<Half16> {
	typedef uint2 type;
	static __device__ __forceinline__ type of(const Quad4 &v, Clamp M, const FloatFmt &f)
	{
		auto c = [M, &f](int x) { return float_of(x < M.lo ? M.lo : x > M.hi ? M.hi : x, f.scale[0], f.bias[0]); };
		const float q[4] = { c(v.v[0]), c(v.v[1]), c(v.v[2]), c(v.v[3]) };
		return half_quad(q, f.bf16);
	}
	static __device__ __forceinline__ void store(Half16 *__restrict__ row, int qd, const type &v) { *reinterpret_cast<uint2 *>(row + 4 * qd) = v; }
};

template <typename DstT>
__device__ __forceinline__ typename InvPix<DstT>::type *inv_dst(const LevelArgs &a);
template <>
__device__ __forceinline__ int *inv_dst<int>(const LevelArgs &a) { return a.ll; }
template <>
__device__ __forceinline__ uint8_t *inv_dst<uint8_t>(const LevelArgs &a) { return a.dst8; }
template <>
__device__ __forceinline__ uint16_t *inv_dst<uint16_t>(const LevelArgs &a) { return reinterpret_cast<uint16_t *>(a.dst8); }   // (ll_ps, llpitch in samples)
template <>
__device__ __forceinline__ float *inv_dst<float>(const LevelArgs &a) { return reinterpret_cast<float *>(a.dst8); }
template <>
__device__ __forceinline__ Half16 *inv_dst<Half16>(const LevelArgs &a) { return reinterpret_cast<Half16 *>(a.dst8); }
// (planes lie one after the other; pixels may be windows of a frame)
template <>
__device__ __forceinline__ uint8_t *inv_dst<DeltaPix<uint8_t>>(const LevelArgs &a) { return a.dst8; }
template <>
__device__ __forceinline__ uint16_t *inv_dst<DeltaPix<uint16_t>>(const LevelArgs &a) { return reinterpret_cast<uint16_t *>(a.dst8); }
template <>
__device__ __forceinline__ int16_t *inv_dst<DeltaPix<int16_t>>(const LevelArgs &a) { return reinterpret_cast<int16_t *>(a.dst8); }

template <typename DstT>
__device__ __forceinline__ long inv_dst_off(const LevelArgs &a, int plane) { return win_off(a.grid, a.ll_ps, plane); }
template <>
__device__ __forceinline__ long inv_dst_off<int>(const LevelArgs &a, int plane) { return plane * a.ll_ps; }

// The vertical state of one plane between row pairs: detail rows dl / dh and even rows el / eh of the current pair.
struct InvCols {
	I2 dl, dh, el, eh;
};

// cdf53.h:40-47 down the columns: the even row of pair j from its subband samples and the details around it
__device__ __forceinline__ I2 inv_even(const LevelArgs &a, int j, I2 s, I2 dprev, I2 dcur)
{
	if ((a.h & 1) && 2 * j == a.h - 1)
		return s;
	const I2 dp = j ? dprev : dcur;
	I2 r = { s.a - tdiv4(dp.a + dcur.a), s.b - tdiv4(dp.b + dcur.b) };
	return r;
}

// the strip's first row pair: what the loop carries
template <class Raw>
__device__ __forceinline__ InvCols inv_first(const LevelArgs &a, int j0, const Raw &before, const Raw &first)
{
	I2 pdl = { 0, 0 }, pdh = { 0, 0 };
	if (j0 > 0) {
		pdl = to_i2(before.dl);
		pdh = to_i2(before.dh);
	}
	InvCols c;
	c.dl = to_i2(first.dl);
	c.dh = to_i2(first.dh);
	c.el = inv_even(a, j0, to_i2(first.sl), pdl, c.dl);
	c.eh = inv_even(a, j0, to_i2(first.sh), pdh, c.dh);
	return c;
}

// one row pair, the column step: the (low, high) samples of its even and its odd row from the state and the next
// pair's samples `n`
struct RowLH {
	I2 lo, hi;
};

template <class Raw>
__device__ __forceinline__ void inv_cols(const LevelArgs &a, int jj, InvCols &c, const Raw &n, RowLH &even, RowLH &odd)
{
	const int r1 = 2 * jj + 1;
	I2 ndl = { 0, 0 }, ndh = { 0, 0 }, nel = c.el, neh = c.eh;   // mirror x[h] := x[h-2]
	if (r1 + 1 < a.h) {
		if (r1 + 2 < a.h) {
			ndl = to_i2(n.dl);
			ndh = to_i2(n.dh);
		}
		nel = inv_even(a, jj + 1, to_i2(n.sl), c.dl, ndl);
		neh = inv_even(a, jj + 1, to_i2(n.sh), c.dh, ndh);
	}
	even.lo = c.el;
	even.hi = c.eh;
	odd.lo.a = c.dl.a + tdiv2(c.el.a + nel.a);   // cdf53.h:49-56
	odd.lo.b = c.dl.b + tdiv2(c.el.b + nel.b);
	odd.hi.a = c.dh.a + tdiv2(c.eh.a + neh.a);
	odd.hi.b = c.dh.b + tdiv2(c.eh.b + neh.b);
	c.dl = ndl;
	c.dh = ndh;
	c.el = nel;
	c.eh = neh;
}

// (waves that overlap by a lane on each side: the RGB kernel)
template <class Raw>
__device__ __forceinline__ void inv_pair(const LevelArgs &a, int jj, int qd, int nquads, InvCols &c, const Raw &n, Quad4 &even, Quad4 &odd)
{
	RowLH e, o;
	inv_cols(a, jj, c, n, e, o);
	even = inv_row_vals(qd, nquads, e.lo, e.hi);
	odd = inv_row_vals(qd, nquads, o.lo, o.hi);
}

// the row step with the halo columns' samples x (x.lo.a, x.hi.a: the column to the right; x.hi.b: the one to the left)
__device__ __forceinline__ Quad4 inv_row_vals_h(int qd, int nquads, int lane, const RowLH &r, const RowLH &x)
{
	int hl = __shfl_up(r.hi.b, 1);
	if (lane == 0)
		hl = x.hi.b;
	if (qd <= 0)
		hl = r.hi.a;
	const int e0 = r.lo.a - tdiv4(hl + r.hi.a);
	const int e1 = r.lo.b - tdiv4(r.hi.a + r.hi.b);
	int er = __shfl_down(e0, 1);
	if (lane == 63)
		er = x.lo.a - tdiv4(r.hi.b + x.hi.a);
	if (qd + 1 >= nquads)
		er = e1;
	Quad4 q;
	q.v[0] = e0;
	q.v[1] = r.hi.a + tdiv2(e0 + e1);
	q.v[2] = e1;
	q.v[3] = r.hi.b + tdiv2(e1 + er);
	return q;
}

// Inverse level: int32 planes, or — the finest level of a gray image — clamped 8-bit pixels out (and, F16, the detail
// bands in as 16-bit values); DstT = float / Half16: the clamped pixels (at a.maxval, whatever it is) as floats, A.fmt.
// The loop is batched like the forward kernel's (see there): one wait per S row pairs.
template <typename DstT, bool F16, int FL = 0>
__global__ __launch_bounds__(64 * WAVES) void k_inv_level_w(LevelArgsW A)
{
	const LevelArgs &a = A.a;
	const int lane = threadIdx.x & 63, wv = wave_in_block();
	int bx, by;
	xcd_strip(bx, by);
	const int qd = bx * 64 + lane;   // all 64 lanes write: the halo columns ride along (InvHalo)
	const int j0 = (by * WAVES + wv) * a.rpw;
	if (j0 >= a.h2)
		return;
	const int j1 = min(j0 + a.rpw, a.h2);
	const int plane = blockIdx.z;
	const bool writes = qd < A.nquads;
	const int *llp = a.src + plane * a.src_ps;
	const typename DetPtr<F16>::type det = DetPtr<F16>::of(a, plane);
	typedef InvRawT<F16> InvRaw;
	typedef OutRow<DstT> Out;
	int opitch = a.llpitch;   // (the wave's: negated for a bottom-up window)
	bool fx = false;
	typename InvPix<DstT>::type *dst = inv_dst<DstT>(a);
	if constexpr (FL == 0)
		dst += inv_dst_off<DstT>(a, plane);
	else
		dst += flip_dst<FL>(a.grid, a.ll_ps, plane, A.fh, opitch, fx);
	const int qs = flip_q<FL>(qd, A.fwq, fx);   // the quad of the row that the lane's quad goes to
	const InvAt at = inv_at(a, qd, A.nquads);
	// a delta sink's base rows (DeltaPix<>): row r of the base's window at the lane's quad, clamped into the window
	typedef typename InvPix<DstT>::base BaseRow;
	auto load_base = [&](int r) {
		if constexpr (InvPix<DstT>::DELTA) {
			const typename InvPix<DstT>::type *b = reinterpret_cast<const typename InvPix<DstT>::type *>(A.base8) + win_off(A.bgrid, A.base_ps, plane);
			return Out::load(b + (long)min(r, a.h - 1) * A.bpitch, min(qd, A.nquads - 1));
		} else {
			return NoBase{};
		}
	};

	constexpr int S = 2;
	const int jb4 = j0 > 0 ? j0 - 1 : 0;
	InvCols c = inv_first(a, j0, inv_load_w(a, llp, det, jb4, at), inv_load_w(a, llp, det, j0, at));
	InvCols cx = inv_first(a, j0, as_pairs(inv_load_halo(a, llp, det, jb4, at)), as_pairs(inv_load_halo(a, llp, det, j0, at)));
	InvRaw nxt[S], cur[S];
	InvHalo nxtx[S];
	HaloPairs curx[S];
	BaseRow nxtb[2 * S], curb[2 * S];
#pragma unroll
	for (int s = 0; s < S; ++s) {
		nxt[s] = inv_load_w(a, llp, det, j0 + 1 + s, at);
		nxtx[s] = inv_load_halo(a, llp, det, j0 + 1 + s, at);
		nxtb[2 * s] = load_base(2 * (j0 + s));
		nxtb[2 * s + 1] = load_base(2 * (j0 + s) + 1);
	}
	typename Out::type orow[2 * S];   // a batch's rows wait here for the next iteration's stores
	auto store_batch = [&](int jb) {
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int j = jb + s;
			if (j < j1 && writes) {
				Out::store(dst + (long)(2 * j) * opitch, qs, orow[2 * s]);
				if (2 * j + 1 < a.h)
					Out::store(dst + (long)(2 * j + 1) * opitch, qs, orow[2 * s + 1]);
			}
		}
	};
	for (int jb = j0; jb < j1; jb += S) {
#pragma unroll
		for (int s = 0; s < S; ++s) {
			cur[s] = hold(nxt[s]);   // the one wait of the iteration
			curx[s] = hold(nxtx[s]);
			curb[2 * s] = hold(nxtb[2 * s]);
			curb[2 * s + 1] = hold(nxtb[2 * s + 1]);
		}
		if (jb > j0)
			store_batch(jb - S);
		if (jb + S < j1) {
#pragma unroll
			for (int s = 0; s < S; ++s) {
				nxt[s] = inv_load_w(a, llp, det, jb + S + 1 + s, at);
				nxtx[s] = inv_load_halo(a, llp, det, jb + S + 1 + s, at);
				nxtb[2 * s] = load_base(2 * (jb + S + s));
				nxtb[2 * s + 1] = load_base(2 * (jb + S + s) + 1);
			}
		}
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const int jj = jb + s;
			if (jj >= j1)
				break;
			RowLH e, o, ex, ox;
			inv_cols(a, jj, c, cur[s], e, o);
			inv_cols(a, jj, cx, curx[s], ex, ox);
			if constexpr (InvPix<DstT>::DELTA) {
				orow[2 * s] = Out::of(inv_row_vals_h(qd, A.nquads, lane, e, ex), clamp_of(a), curb[2 * s]);
				orow[2 * s + 1] = Out::of(inv_row_vals_h(qd, A.nquads, lane, o, ox), clamp_of(a), curb[2 * s + 1]);
			} else if constexpr (FloatSample<DstT>::value) {
				orow[2 * s] = Out::of(flip_quad<FL>(inv_row_vals_h(qd, A.nquads, lane, e, ex), fx), clamp_of(a), A.fmt);
				orow[2 * s + 1] = Out::of(flip_quad<FL>(inv_row_vals_h(qd, A.nquads, lane, o, ox), fx), clamp_of(a), A.fmt);
			} else {
				orow[2 * s] = Out::of(flip_quad<FL>(inv_row_vals_h(qd, A.nquads, lane, e, ex), fx), clamp_of(a));
				orow[2 * s + 1] = Out::of(flip_quad<FL>(inv_row_vals_h(qd, A.nquads, lane, o, ox), fx), clamp_of(a));
			}
		}
	}
	store_batch(j0 + (j1 - 1 - j0) / S * S);
}

// ---- two levels per pass (inverse, int32 planes): the mirror image of k_fwd2_level_w ----
// A wave undoes level k+1 for its column pairs — one pair per lane: the lane's LL sample and its three details — and
// hands every rebuilt LL row of level k (the lane's two samples of it) straight to the level-k stage, whose other
// inputs are that level's detail bands: the LL band of level k is neither written nor read.  Rows of the output leave
// as whole 128-byte lines: a wave owns the quads of lanes 4..59 (56 x 16 bytes = seven lines, at a multiple of seven
// lines), lanes 3 and 60 load their columns only for their neighbours' row steps (undoing the columns first leaves
// every lane's high-band samples right whatever its neighbours hold; cdf53.h:36-61), the other lanes repeat those
// lanes' loads.  Shapes as in k_fwd2_level_w: w % 4 == 0, h % 4 == 0.
struct Inv2Args {
	const int *ll2;  long ll2_ps;  int ll2pitch;   // LL of level k+1, w/4 x h/4
	const int *det;  long det_ps;  int dpitch;     // the pyramid: detail bands of both levels
	int *dst;        long dst_ps;  int opitch;     // output, w x h
	int w, h, nquads;
	int mpw;          // level k+1 row pairs per wave strip
	const short *det16;   // F16: the detail bands of BOTH levels as 16-bit values (positions, pitch and plane stride of det)
	uint8_t *dst8;        // 8-bit output (the finest level of a gray picture: pnm.h:108's clamp fused), dst_ps / opitch in bytes
	WinGrid grid;         // the windows behind dst8 (dst_ps apart in a band)
	long cstride;         // planar RGB pixels behind dst8: from a window's R plane to G, from G to B (bytes; signed as in LevelArgsW); 0: interleaved.  (Last, as in LevelArgsW.)
	int fh, fwq;          // the flipped instances (FL): the WINDOWS' height and quads per row
};
constexpr int V2_FIRST = 4, V2_OWN = 56;

struct Raw2 {       // one row of level k+1 at the lane's pair: LL | HL | LH | HH
	int sl, sh, dl, dh;
};
// (one row pair of level k at the lane's two pairs — HL | LH | HH, its LL comes from level k+1 — is DetBand<F16>::raw1 below)
__device__ __forceinline__ Raw2 hold(const Raw2 &r)
{
	Raw2 o = { hold(r.sl), hold(r.sh), hold(r.dl), hold(r.dh) };
	return o;
}

// cdf53.h:36-61 along a row of level k+1 for the lane's pair (low, high) -> its two samples of level k's LL row
__device__ __forceinline__ I2 inv_row_pair(int q, int nquads, int lo, int hi)
{
	int hl = __shfl_up(hi, 1);
	if (q <= 0)
		hl = hi;
	const int e = lo - tdiv4(hl + hi);
	int er = __shfl_down(e, 1);
	if (q + 1 >= nquads)
		er = e;
	I2 r = { e, hi + tdiv2(e + er) };
	return r;
}

__device__ __forceinline__ I2 i2_sub4(I2 s, I2 dp, I2 d)   // cdf53.h:40-47: the even row from its low-pass sample and the details around it
{
	I2 r = { s.a - tdiv4(dp.a + d.a), s.b - tdiv4(dp.b + d.b) };
	return r;
}
__device__ __forceinline__ I2 i2_add2(I2 d, I2 e0, I2 e1)   // cdf53.h:49-56: the odd row
{
	I2 r = { d.a + tdiv2(e0.a + e1.a), d.b + tdiv2(e0.b + e1.b) };
	return r;
}

// the detail bands a two-level inverse step reads, and the rows it writes, as the kernel variant sees them
template <bool F16>
struct DetBand {
	typedef const int *ptr;
	struct raw1 {
		int2 sh, dl, dh;
	};
	static __device__ __forceinline__ ptr of(const Inv2Args &a, long plane) { return a.det + plane * a.det_ps; }
	static __device__ __forceinline__ int2 pair(const int *p) { return ld2(p); }
};
template <>
struct DetBand<true> {
	typedef const short *ptr;
	struct raw1 {
		unsigned sh, dl, dh;   // two 16-bit values each
	};
	static __device__ __forceinline__ ptr of(const Inv2Args &a, long plane) { return a.det16 + plane * a.det_ps; }
	static __device__ __forceinline__ unsigned pair(const short *p) { return *reinterpret_cast<const unsigned *>(p); }
};
__device__ __forceinline__ DetBand<false>::raw1 hold(const DetBand<false>::raw1 &r)
{
	DetBand<false>::raw1 o = { hold(r.sh), hold(r.dl), hold(r.dh) };
	return o;
}
__device__ __forceinline__ DetBand<true>::raw1 hold(const DetBand<true>::raw1 &r)
{
	DetBand<true>::raw1 o = { hold(r.sh), hold(r.dl), hold(r.dh) };
	return o;
}
template <typename DstT>
struct OutPlane {
	typedef int4 row;
	static __device__ __forceinline__ int *of(const Inv2Args &a, long plane) { return a.dst + plane * a.dst_ps; }
	static __device__ __forceinline__ void store(int *p, const int4 &v)
	{
		typedef int v4i __attribute__((ext_vector_type(4)));
		const v4i x = { v.x, v.y, v.z, v.w };
		__builtin_nontemporal_store(x, reinterpret_cast<v4i *>(p));
	}
};
template <>
struct OutPlane<uint8_t> {
	typedef unsigned row;
	static __device__ __forceinline__ uint8_t *of(const Inv2Args &a, long plane) { return a.dst8 + win_off(a.grid, a.dst_ps, (int)plane); }
	static __device__ __forceinline__ void store(uint8_t *p, unsigned v) { __builtin_nontemporal_store(v, reinterpret_cast<unsigned *>(p)); }
};

// DstT = int: int32 rows out (nontemporal 16-byte stores; the block's four waves on top of each other).  DstT = uint8_t: the finest
// level of a gray picture — clamped pixels, 4 bytes per lane: a wave's 224 bytes are seven 32-byte pieces, and the block's four waves
// sit SIDE BY SIDE so that together they write seven whole lines.  F16: both levels' detail bands are 16-bit values (the codec's
// pipelines, dwtx_p16); the arithmetic is int32 either way.
template <typename DstT, bool F16, int FL = 0>
__global__ __launch_bounds__(64 * WAVES) void k_inv2_level_w(Inv2Args a)
{
	constexpr bool SIDE = sizeof(DstT) == 1;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	int bx, by;
	xcd_strip(bx, by);
	const int strip = SIDE ? bx * WAVES + wv : bx;
	if (strip * V2_OWN >= a.nquads)
		return;
	const int q = strip * V2_OWN - V2_FIRST + lane;
	const int h2 = a.h >> 1, h4 = a.h >> 2, w2 = a.w >> 1, w4 = a.w >> 2;
	const int m0 = (SIDE ? by : by * WAVES + wv) * a.mpw;
	if (m0 >= h4)
		return;
	const int m1 = min(m0 + a.mpw, h4);
	const int plane = blockIdx.z;
	const bool own = lane >= V2_FIRST && lane < V2_FIRST + V2_OWN && q < a.nquads;
	// every lane loads: lanes 3 and 60 for their neighbours, the ones beyond them repeat those two lanes' columns
	const int qc = min(max(q + max(V2_FIRST - 1 - lane, 0) - max(lane - (V2_FIRST + V2_OWN), 0), 0), a.nquads - 1);
	const int *ll2 = a.ll2 + plane * a.ll2_ps + qc;
	const typename DetBand<F16>::ptr det = DetBand<F16>::of(a, plane);
	int opitch = a.opitch;   // (the wave's: negated for a bottom-up window)
	bool fx = false;
	DstT *dst;
	if constexpr (FL == 0)
		dst = OutPlane<DstT>::of(a, plane);
	else
		dst = a.dst8 + flip_dst<FL>(a.grid, a.dst_ps, plane, a.fh, opitch, fx);   // (FL: 8-bit gray pixels only)
	const int qs = flip_q<FL>(q, a.fwq, fx);
	typedef typename DetBand<F16>::raw1 Raw1;
	auto load2 = [&](int m) {
		const int mm = min(max(m, 0), h4 - 1);
		Raw2 r = { ll2[(long)mm * a.ll2pitch], (int)det[(long)mm * a.dpitch + w4 + qc], (int)det[(long)(h4 + mm) * a.dpitch + qc],
			(int)det[(long)(h4 + mm) * a.dpitch + w4 + qc] };
		return r;
	};
	auto load1 = [&](int j) {
		const int jc = min(max(j, 0), h2 - 1);
		Raw1 r = { DetBand<F16>::pair(det + (long)jc * a.dpitch + w2 + 2 * qc), DetBand<F16>::pair(det + (long)(h2 + jc) * a.dpitch + 2 * qc),
			DetBand<F16>::pair(det + (long)(h2 + jc) * a.dpitch + w2 + 2 * qc) };
		return r;
	};
	// level k+1, column direction: the state of pair m0
	int d2l, d2h, e2l, e2h;
	{
		const Raw2 before = load2(m0 - 1), first = load2(m0);
		d2l = first.dl;
		d2h = first.dh;
		e2l = first.sl - tdiv4((m0 ? before.dl : d2l) + d2l);
		e2h = first.sh - tdiv4((m0 ? before.dh : d2h) + d2h);
	}
	// level k: the state of row pair 2 m0 (its LL row is level k+1's even row of pair m0)
	I2 cdl, cdh, cel, ceh;
	{
		const Raw1 before = load1(2 * m0 - 1), first = load1(2 * m0);
		const I2 sl = inv_row_pair(q, a.nquads, e2l, e2h);
		cdl = to_i2(first.dl);
		cdh = to_i2(first.dh);
		cel = i2_sub4(sl, m0 ? to_i2(before.dl) : cdl, cdl);
		ceh = i2_sub4(to_i2(first.sh), m0 ? to_i2(before.dh) : cdh, cdh);
	}
	Raw2 n2 = load2(m0 + 1), c2;
	Raw1 n1a = load1(2 * m0 + 1), n1b = load1(2 * m0 + 2), c1a, c1b;
	typename OutPlane<DstT>::row orow[4];
	auto store_rows = [&](int m) {
		if (!own)
			return;
#pragma unroll
		for (int k = 0; k < 4; ++k)
			OutPlane<DstT>::store(dst + (long)(4 * m + k) * opitch + 4 * qs, orow[k]);
	};
	// one row pair of level k: state (pair jj) + the next pair's samples -> its two output rows; the state moves on
	auto pair1 = [&](int jj, I2 nsl, const Raw1 &n, typename OutPlane<DstT>::row &even, typename OutPlane<DstT>::row &odd) {
		I2 ndl = { 0, 0 }, ndh = { 0, 0 }, nel = cel, neh = ceh;   // the plane's last pair mirrors: x[h] := x[h-2]
		if (jj + 1 < h2) {
			ndl = to_i2(n.dl);
			ndh = to_i2(n.dh);
			nel = i2_sub4(nsl, cdl, ndl);
			neh = i2_sub4(to_i2(n.sh), cdh, ndh);
		}
		const Quad4 ev = inv_row_vals(q, a.nquads, cel, ceh);
		const Quad4 od = inv_row_vals(q, a.nquads, i2_add2(cdl, cel, nel), i2_add2(cdh, ceh, neh));
		even = OutRow<DstT>::of(flip_quad<FL>(ev, fx), Clamp{ 0, 0 });
		odd = OutRow<DstT>::of(flip_quad<FL>(od, fx), Clamp{ 0, 0 });
		cdl = ndl;
		cdh = ndh;
		cel = nel;
		ceh = neh;
	};
	for (int m = m0; m < m1; ++m) {
		c2 = hold(n2);   // the one wait of the iteration (see fwd_level_body)
		c1a = hold(n1a);
		c1b = hold(n1b);
		if (m > m0)
			store_rows(m - 1);
		if (m + 1 < m1) {
			n2 = load2(m + 2);
			n1a = load1(2 * m + 3);
			n1b = load1(2 * m + 4);
		}
		// level k+1, pair m: its odd row, and the even row of the pair after it
		int nd2l = 0, nd2h = 0, ne2l = e2l, ne2h = e2h;
		if (m + 1 < h4) {
			nd2l = c2.dl;
			nd2h = c2.dh;
			ne2l = c2.sl - tdiv4(d2l + nd2l);
			ne2h = c2.sh - tdiv4(d2h + nd2h);
		}
		const I2 ll_odd = inv_row_pair(q, a.nquads, d2l + tdiv2(e2l + ne2l), d2h + tdiv2(e2h + ne2h));   // LL row 2m+1 of level k
		const I2 ll_next = inv_row_pair(q, a.nquads, ne2l, ne2h);                                           // LL row 2m+2
		d2l = nd2l;
		d2h = nd2h;
		e2l = ne2l;
		e2h = ne2h;
		pair1(2 * m, ll_odd, c1a, orow[0], orow[1]);
		pair1(2 * m + 1, ll_next, c1b, orow[2], orow[3]);
	}
	store_rows(m1 - 1);
}

// The finest inverse level of an RGB image: one wave carries the same columns of the three planes
// (Y, Co, Cg) and writes interleaved 8-bit pixels — image.h:39-50 ycocg2rgb with its input clamps and
// the output clamp of pnm.h:108 fused in (rgb_plain).  grid.z = image; dst8 rows are 3*w bytes.
struct Rgb12 {
	unsigned w[3];   // four pixels
};
struct Rgb24 {
	unsigned w[6];   // four deep pixels
};

// the same for deep pixels: the clamps at the picture's maxval M
// (BGR, here and in rgbx_of and rgb_of: the pixels lie as B, G, R — dwtx_pixels::order — so R and B trade places AFTER the
// clamps, which act on the colours)
template <bool BGR = false>
__device__ __forceinline__ Rgb24 rgb16_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M)
{
	unsigned px[12];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		int r, g, b;
		rgb_plain(y.v[k], co.v[k], cg.v[k], M, r, g, b);
		px[3 * k + (BGR ? 2 : 0)] = (unsigned)r;
		px[3 * k + 1] = (unsigned)g;
		px[3 * k + (BGR ? 0 : 2)] = (unsigned)b;
	}
	Rgb24 o;
#pragma unroll
	for (int k = 0; k < 6; ++k)
		o.w[k] = (px[2 * k] & 0xffffu) | (px[2 * k + 1] << 16);   // (two's complement: a negative sample's upper bits stay out of its neighbour)
	return o;
}

// the same colour transform and clamps (M: 255, or a deep picture's maxval) for planar pixels: the lane's four pixels as one
// quad per channel — px[c][k] = channel c of pixel k
__device__ __forceinline__ void rgb_planes_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, unsigned (&px)[3][4])
{
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		int r, g, b;
		rgb_plain(y.v[k], co.v[k], cg.v[k], M, r, g, b);
		px[0][k] = (unsigned)r;
		px[1][k] = (unsigned)g;
		px[2][k] = (unsigned)b;
	}
}
// w[c] = the four bytes of channel c
__device__ __forceinline__ Rgb12 rgb_planar_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg)
{
	unsigned px[3][4];
	rgb_planes_of(y, co, cg, Clamp{ 0, 255 }, px);
	Rgb12 o;
#pragma unroll
	for (int c = 0; c < 3; ++c)
		o.w[c] = px[c][0] | (px[c][1] << 8) | (px[c][2] << 16) | (px[c][3] << 24);
	return o;
}
// w[2c], w[2c+1] = the four samples of channel c
__device__ __forceinline__ Rgb24 rgb16_planar_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M)
{
	unsigned px[3][4];
	rgb_planes_of(y, co, cg, M, px);
	Rgb24 o;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		o.w[2 * c] = (px[c][0] & 0xffffu) | (px[c][1] << 16);   // (two's complement, as in rgb16_of)
		o.w[2 * c + 1] = (px[c][2] & 0xffffu) | (px[c][3] << 16);
	}
	return o;
}

// what the RGB kernel's lanes write per row: twelve bytes of 8-bit pixels, or twenty-four of deep ones — interleaved in one
// piece (PIX_PACKED), or (PIX_PLANAR; cs = the channel stride in samples) as three aligned quads, one per plane: 4 bytes each,
// 8 of deep pixels, or (PIX_STEP4: 8-bit RGB in 4-byte pixels, dwtx_pixels::rgbx8()) the three colour bytes of each of the four
// pixels and NOT the fourth: a halfword and a byte per pixel, nothing read, merged and written back (include/dwtx.h: another
// stream may be writing the fourth bytes at the same moment)
// PIX_PACKED_BGR, PIX_STEP4_BGR: the two interleaved layouts for pixels that lie as B, G, R: the same stores of the same bytes,
// R and B at each other's places in what is stored.  (Planar pixels have no such twin: the host gives cs a sign.)
enum PixLayout { PIX_PACKED = 0, PIX_PLANAR = 1, PIX_STEP4 = 2, PIX_PACKED_BGR = 3, PIX_STEP4_BGR = 4 };
struct Rgbx16 {
	unsigned w[4];   // four pixels: R | G << 8 | B << 16 (PIX_STEP4_BGR: B | G << 8 | R << 16)
};
template <bool NT>
__device__ __forceinline__ void rgbx_store(uint8_t *p, const Rgbx16 &v)
{
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const unsigned short rg = (unsigned short)v.w[k];
		const uint8_t b = (uint8_t)(v.w[k] >> 16);
		if (NT) {
			__builtin_nontemporal_store(rg, reinterpret_cast<unsigned short *>(p + 4 * k));
			__builtin_nontemporal_store(b, p + 4 * k + 2);
		} else {
			*reinterpret_cast<unsigned short *>(p + 4 * k) = rg;
			p[4 * k + 2] = b;
		}
	}
}
template <typename PixT, PixLayout LAYOUT = PIX_PACKED>
struct RgbOut {
	typedef Rgb12 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp);
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long)
	{
		U32x3 x = { v.w[0], v.w[1], v.w[2] };
		*reinterpret_cast<U32x3 *>(dst + r * pitch + 12 * qd) = x;
	}
};
template <>
struct RgbOut<uint16_t, PIX_PACKED> {
	typedef Rgb24 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M) { return rgb16_of(y, co, cg, M); }
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long)   // (pitch in samples; rows and quads are multiples of 8 bytes)
	{
		uint2 *p = reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(dst) + r * pitch + 12 * qd);
		p[0] = make_uint2(v.w[0], v.w[1]);
		p[1] = make_uint2(v.w[2], v.w[3]);
		p[2] = make_uint2(v.w[4], v.w[5]);
	}
};
template <>
struct RgbOut<uint8_t, PIX_PLANAR> {
	typedef Rgb12 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp) { return rgb_planar_of(y, co, cg); }
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long cs)
	{
		uint8_t *p = dst + r * pitch + 4 * qd;
#pragma unroll
		for (int c = 0; c < 3; ++c)
			*reinterpret_cast<unsigned *>(p + c * cs) = v.w[c];
	}
};
template <>
struct RgbOut<uint16_t, PIX_PLANAR> {
	typedef Rgb24 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M) { return rgb16_planar_of(y, co, cg, M); }
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long cs)
	{
		uint16_t *p = reinterpret_cast<uint16_t *>(dst) + r * pitch + 4 * qd;
#pragma unroll
		for (int c = 0; c < 3; ++c)
			*reinterpret_cast<uint2 *>(p + c * cs) = make_uint2(v.w[2 * c], v.w[2 * c + 1]);
	}
};
// planar float pixels: the colour transform and its clamps at M, then each plane's quad through its own colour's scale and
// bias (px[c] is colour c wherever its plane lies: B, G, R planes come with a negative cs): 16 bytes per plane and lane, or 8.
// fp32 rows wait for their store as the deep sink's clamped integers — six registers, not twelve, which keeps the kernel
// below 128 — and become floats in store(), which takes the conversion (FloatSample<float>::AT_STORE)
template <>
struct RgbOut<float, PIX_PLANAR> {
	typedef Rgb24 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, const FloatFmt &) { return rgb16_planar_of(y, co, cg, M); }
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long cs, const FloatFmt &f)
	{
		float *p = reinterpret_cast<float *>(dst) + r * pitch + 4 * qd;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const unsigned lo = v.w[2 * c], hi = v.w[2 * c + 1];
			const int sx = f.sext;   // (uniform: a range below 0 never reaches beyond 32767)
			auto l16 = [sx](unsigned w) { return sx ? (int)(short)(w & 0xffffu) : (int)(w & 0xffffu); };
			auto h16 = [sx](unsigned w) { return sx ? (int)w >> 16 : (int)(w >> 16); };
			*reinterpret_cast<float4 *>(p + c * cs) = make_float4(float_of(l16(lo), f.scale[c], f.bias[c]), float_of(h16(lo), f.scale[c], f.bias[c]),
				float_of(l16(hi), f.scale[c], f.bias[c]), float_of(h16(hi), f.scale[c], f.bias[c]));
		}
	}
};
template <>
struct RgbOut<Half16, PIX_PLANAR> : RgbOut<uint16_t, PIX_PLANAR> {   // (the deep planar sink's row and store: the same 8 bytes per plane)
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, const FloatFmt &f)
	{
		unsigned px[3][4];
		rgb_planes_of(y, co, cg, M, px);
		row o;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const float q[4] = { float_of((int)px[c][0], f.scale[c], f.bias[c]), float_of((int)px[c][1], f.scale[c], f.bias[c]),
				float_of((int)px[c][2], f.scale[c], f.bias[c]), float_of((int)px[c][3], f.scale[c], f.bias[c]) };
			const uint2 h = half_quad(q, f.bf16);
			o.w[2 * c] = h.x;
			o.w[2 * c + 1] = h.y;
		}
		return o;
	}
};
template <bool BGR = false>
__device__ __forceinline__ Rgbx16 rgbx_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg)
{
	unsigned px[3][4];
	rgb_planes_of(y, co, cg, Clamp{ 0, 255 }, px);
	Rgbx16 o;
#pragma unroll
	for (int k = 0; k < 4; ++k)
		o.w[k] = px[BGR ? 2 : 0][k] | (px[1][k] << 8) | (px[BGR ? 0 : 2][k] << 16);
	return o;
}
template <>
struct RgbOut<uint8_t, PIX_STEP4> {
	typedef Rgbx16 row;
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp) { return rgbx_of(y, co, cg); }
	static __device__ __forceinline__ void store(uint8_t *dst, long pitch, int r, int qd, const row &v, long)
	{
		rgbx_store<false>(dst + r * pitch + 16 * qd, v);
	}
};

template <bool BGR = false>
__device__ __forceinline__ Rgb12 rgb_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg)
{
	unsigned char px[12];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		int r, g, b;
		rgb_plain(y.v[k], co.v[k], cg.v[k], Clamp{ 0, 255 }, r, g, b);
		px[3 * k + (BGR ? 2 : 0)] = (unsigned char)r;
		px[3 * k + 1] = (unsigned char)g;
		px[3 * k + (BGR ? 0 : 2)] = (unsigned char)b;
	}
	Rgb12 o;
#pragma unroll
	for (int k = 0; k < 3; ++k)
		o.w[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
	return o;
}

template <typename PixT, PixLayout LAYOUT>
__device__ __forceinline__ typename RgbOut<PixT, LAYOUT>::row RgbOut<PixT, LAYOUT>::of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp) { return rgb_of(y, co, cg); }

// the B, G, R twins: their RGB layout's row and store, R and B swapped in the row
template <>
struct RgbOut<uint8_t, PIX_PACKED_BGR> : RgbOut<uint8_t, PIX_PACKED> {
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp) { return rgb_of<true>(y, co, cg); }
};
template <>
struct RgbOut<uint16_t, PIX_PACKED_BGR> : RgbOut<uint16_t, PIX_PACKED> {
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M) { return rgb16_of<true>(y, co, cg, M); }
};
template <>
struct RgbOut<uint8_t, PIX_STEP4_BGR> : RgbOut<uint8_t, PIX_STEP4> {
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp) { return rgbx_of<true>(y, co, cg); }
};

// a delta view's interleaved 8-bit pixels (DeltaPix<uint8_t>): the residual's clamps for [-R, R] — Y and every colour to [-R, R], Co
// and Cg to [-2R, 2R] — then each colour plus the base's byte of the same place, clamped to the range; the base's twelve bytes
// travel as they were loaded
template <bool BGR>
__device__ __forceinline__ Rgb12 rgb_delta_of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, const U32x3 &base)
{
	unsigned char px[12];
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		int r = rgb_byte(base, 3 * k + (BGR ? 2 : 0)), g = rgb_byte(base, 3 * k + 1), b = rgb_byte(base, 3 * k + (BGR ? 0 : 2));
		rgb_residual(y.v[k], co.v[k], cg.v[k], M, r, g, b);
		px[3 * k + (BGR ? 2 : 0)] = (unsigned char)r;
		px[3 * k + 1] = (unsigned char)g;
		px[3 * k + (BGR ? 0 : 2)] = (unsigned char)b;
	}
	Rgb12 o;
#pragma unroll
	for (int k = 0; k < 3; ++k)
		o.w[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
	return o;
}
template <>
struct RgbOut<DeltaPix<uint8_t>, PIX_PACKED> : RgbOut<uint8_t, PIX_PACKED> {
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, const U32x3 &base) { return rgb_delta_of<false>(y, co, cg, M, base); }
};
template <>
struct RgbOut<DeltaPix<uint8_t>, PIX_PACKED_BGR> : RgbOut<uint8_t, PIX_PACKED> {
	static __device__ __forceinline__ row of(const Quad4 &y, const Quad4 &co, const Quad4 &cg, Clamp M, const U32x3 &base) { return rgb_delta_of<true>(y, co, cg, M, base); }
};
template <typename PixT>
struct RgbBase {
	typedef NoBase type;
};
template <>
struct RgbBase<DeltaPix<uint8_t>> {
	typedef U32x3 type;
};
__device__ __forceinline__ U32x3 hold(const U32x3 &v)
{
	U32x3 o = { hold(v.x), hold(v.y), hold(v.z) };
	return o;
}

// PixT = uint16_t: deep pixels (dst8 points to uint16_t samples, ll_ps / llpitch count samples, clamps at a.maxval)
// PIX_PLANAR: dst8 is the R plane of the window, G and B A.cstride samples apart each (signed), llpitch the pitch of a plane's rows
// PIX_STEP4: llpitch is the pitch of rows of 4-byte pixels; the step is the constant 4 here, no argument carries it
// PixT = float / Half16 (PIX_PLANAR only): float samples, strides in samples, clamps at a.maxval, the conversion in A.fmt
template <bool F16, typename PixT = uint8_t, PixLayout LAYOUT = PIX_PACKED, int FL = 0>
__global__ __launch_bounds__(64 * WAVES) void k_inv_level_w_rgb(LevelArgsW A)
{
	const LevelArgs &a = A.a;
	const int lane = threadIdx.x & 63, wv = wave_in_block();
	int bx, by;
	xcd_strip(bx, by);
	const int qd = bx * INV_QUADS - 1 + lane;
	const int j0 = (by * WAVES + wv) * a.rpw;
	if (j0 >= a.h2)
		return;
	const int j1 = min(j0 + a.rpw, a.h2);
	const int image = blockIdx.z;
	const bool valid = qd >= 0 && qd < A.nquads;
	const bool writes = valid && lane >= 1 && lane <= INV_QUADS;
	const int *llp[3];
	typename DetPtr<F16>::type det[3];
	typedef InvRawT<F16> InvRaw;
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		llp[ch] = a.src + (long)(3 * image + ch) * a.src_ps;
		det[ch] = DetPtr<F16>::of(a, 3 * image + ch);
	}
	typedef RgbOut<PixT, LAYOUT> Out;
	int opitch = a.llpitch;   // (the wave's: negated for a bottom-up window)
	bool fx = false;
	uint8_t *dst = a.dst8 + flip_dst<FL>(a.grid, a.ll_ps, image, A.fh, opitch, fx) * (long)sizeof(PixT);
	const int qs = flip_q<FL>(qd, A.fwq, fx);   // the quad of the row that the lane's quad goes to
	const InvAt at = inv_at(a, qd, A.nquads);

	// a delta sink's base rows (DeltaPix<uint8_t>): the twelve bytes of row r of the base's window where the lane's quad goes, clamped into the window
	typedef typename RgbBase<PixT>::type BaseRow;
	constexpr bool DELTA = !std::is_same<BaseRow, NoBase>::value;
	auto load_base = [&](int r) {
		if constexpr (DELTA) {
			const uint8_t *b = A.base8 + win_off(A.bgrid, A.base_ps, image);
			return *reinterpret_cast<const U32x3 *>(b + (long)min(r, a.h - 1) * A.bpitch + 12 * min(max(qd, 0), A.nquads - 1));
		} else {
			return NoBase{};
		}
	};
	// (one row pair per batch: three planes' worth of arithmetic lies between two waits as it is)
	InvCols c[3];
	InvRaw nxt[3], cur[3];
	BaseRow nxtb[2], curb[2];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		c[ch] = inv_first(a, j0, inv_load_w(a, llp[ch], det[ch], j0 > 0 ? j0 - 1 : 0, at), inv_load_w(a, llp[ch], det[ch], j0, at));
		nxt[ch] = inv_load_w(a, llp[ch], det[ch], j0 + 1, at);
	}
	nxtb[0] = load_base(2 * j0);
	nxtb[1] = load_base(2 * j0 + 1);
	typename Out::row orow[2];
	auto store_pair = [&](int j) {
		if (writes) {   // twelve bytes per lane in one store: the wave's 56 lanes write 672 consecutive bytes (deep pixels: twice that; planar: a third of it to each plane)
			if constexpr (FloatSample<PixT>::AT_STORE) {
				Out::store(dst, opitch, 2 * j, qs, orow[0], A.cstride, A.fmt);
				if (2 * j + 1 < a.h)
					Out::store(dst, opitch, 2 * j + 1, qs, orow[1], A.cstride, A.fmt);
			} else {
				Out::store(dst, opitch, 2 * j, qs, orow[0], A.cstride);
				if (2 * j + 1 < a.h)
					Out::store(dst, opitch, 2 * j + 1, qs, orow[1], A.cstride);
			}
		}
	};
	for (int jj = j0; jj < j1; ++jj) {
#pragma unroll
		for (int ch = 0; ch < 3; ++ch)
			cur[ch] = hold(nxt[ch]);   // the one wait of the iteration
		curb[0] = hold(nxtb[0]);
		curb[1] = hold(nxtb[1]);
		if (jj > j0)
			store_pair(jj - 1);
		if (jj + 1 < j1) {
#pragma unroll
			for (int ch = 0; ch < 3; ++ch)
				nxt[ch] = inv_load_w(a, llp[ch], det[ch], jj + 2, at);
			nxtb[0] = load_base(2 * (jj + 1));
			nxtb[1] = load_base(2 * (jj + 1) + 1);
		}
		Quad4 even[3], odd[3];
#pragma unroll
		for (int ch = 0; ch < 3; ++ch)
			inv_pair(a, jj, qd, A.nquads, c[ch], cur[ch], even[ch], odd[ch]);
		if constexpr (FL == 2) {
#pragma unroll
			for (int ch = 0; ch < 3; ++ch) {
				even[ch] = flip_quad<FL>(even[ch], fx);
				odd[ch] = flip_quad<FL>(odd[ch], fx);
			}
		}
		if constexpr (DELTA) {
			orow[0] = Out::of(even[0], even[1], even[2], clamp_of(a), curb[0]);
			orow[1] = Out::of(odd[0], odd[1], odd[2], clamp_of(a), curb[1]);
		} else if constexpr (FloatSample<PixT>::value) {
			orow[0] = Out::of(even[0], even[1], even[2], clamp_of(a), A.fmt);
			orow[1] = Out::of(odd[0], odd[1], odd[2], clamp_of(a), A.fmt);
		} else {
			orow[0] = Out::of(even[0], even[1], even[2], clamp_of(a));
			orow[1] = Out::of(odd[0], odd[1], odd[2], clamp_of(a));
		}
	}
	store_pair(j1 - 1);
}

// The two finest levels of an RGB picture in one pass: k_inv2_level_w's two stages for the same columns of the three planes
// (Y, Co, Cg; both levels' detail bands as 16-bit values), the colour transform and the clamps of image.h:39-50 / pnm.h:108 on
// the finished rows, interleaved 8-bit pixels out — twelve bytes per lane: a wave's 56 owning lanes write 672 bytes = 21
// 32-byte pieces, the block's four waves side by side 21 whole lines.  Three planes' state and rows in flight: ~150 vector
// registers, three waves per SIMD — and still the faster way: the int32 LL planes of the second level (3 B per pixel written,
// 3 B read) are gone.  grid.z = image.
// PIX_PLANAR: the lane's four pixels go out as one word to each of the window's three planes (a.cstride apart) instead
// PIX_STEP4: into 4-byte pixels, three bytes of each (rgbx_store)
template <bool F16, PixLayout LAYOUT = PIX_PACKED, int FL = 0>
__global__ __launch_bounds__(64 * WAVES) void k_inv2_level_w_rgb(Inv2Args a)
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	int bx, by;
	xcd_strip(bx, by);
	const int strip = bx * WAVES + wv;
	if (strip * V2_OWN >= a.nquads)
		return;
	const int q = strip * V2_OWN - V2_FIRST + lane;
	const int h2 = a.h >> 1, h4 = a.h >> 2, w2 = a.w >> 1, w4 = a.w >> 2;
	const int m0 = by * a.mpw;
	if (m0 >= h4)
		return;
	const int m1 = min(m0 + a.mpw, h4);
	const int image = blockIdx.z;
	const bool own = lane >= V2_FIRST && lane < V2_FIRST + V2_OWN && q < a.nquads;
	const int qc = min(max(q + max(V2_FIRST - 1 - lane, 0) - max(lane - (V2_FIRST + V2_OWN), 0), 0), a.nquads - 1);
	typedef typename DetBand<F16>::raw1 Raw1;
	const int *ll2[3];
	typename DetBand<F16>::ptr det[3];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		ll2[ch] = a.ll2 + (long)(3 * image + ch) * a.ll2_ps + qc;
		det[ch] = DetBand<F16>::of(a, 3 * image + ch);
	}
	int opitch = a.opitch;   // (the wave's: negated for a bottom-up window)
	bool fx = false;
	uint8_t *dst = a.dst8 + flip_dst<FL>(a.grid, a.dst_ps, image, a.fh, opitch, fx);
	const int qs = flip_q<FL>(q, a.fwq, fx);
	auto load2 = [&](int ch, int m) {
		const int mm = min(max(m, 0), h4 - 1);
		Raw2 r = { ll2[ch][(long)mm * a.ll2pitch], (int)det[ch][(long)mm * a.dpitch + w4 + qc], (int)det[ch][(long)(h4 + mm) * a.dpitch + qc],
			(int)det[ch][(long)(h4 + mm) * a.dpitch + w4 + qc] };
		return r;
	};
	auto load1 = [&](int ch, int j) {
		const int jc = min(max(j, 0), h2 - 1);
		Raw1 r = { DetBand<F16>::pair(det[ch] + (long)jc * a.dpitch + w2 + 2 * qc), DetBand<F16>::pair(det[ch] + (long)(h2 + jc) * a.dpitch + 2 * qc),
			DetBand<F16>::pair(det[ch] + (long)(h2 + jc) * a.dpitch + w2 + 2 * qc) };
		return r;
	};
	int d2l[3], d2h[3], e2l[3], e2h[3];
	I2 cdl[3], cdh[3], cel[3], ceh[3];
	Raw2 n2[3], c2[3];
	Raw1 n1a[3], n1b[3], c1a[3], c1b[3];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		const Raw2 before2 = load2(ch, m0 - 1), first2 = load2(ch, m0);
		d2l[ch] = first2.dl;
		d2h[ch] = first2.dh;
		e2l[ch] = first2.sl - tdiv4((m0 ? before2.dl : d2l[ch]) + d2l[ch]);
		e2h[ch] = first2.sh - tdiv4((m0 ? before2.dh : d2h[ch]) + d2h[ch]);
		const Raw1 before1 = load1(ch, 2 * m0 - 1), first1 = load1(ch, 2 * m0);
		const I2 sl = inv_row_pair(q, a.nquads, e2l[ch], e2h[ch]);
		cdl[ch] = to_i2(first1.dl);
		cdh[ch] = to_i2(first1.dh);
		cel[ch] = i2_sub4(sl, m0 ? to_i2(before1.dl) : cdl[ch], cdl[ch]);
		ceh[ch] = i2_sub4(to_i2(first1.sh), m0 ? to_i2(before1.dh) : cdh[ch], cdh[ch]);
		n2[ch] = load2(ch, m0 + 1);
		n1a[ch] = load1(ch, 2 * m0 + 1);
		n1b[ch] = load1(ch, 2 * m0 + 2);
	}
	typename RgbOut<uint8_t, LAYOUT>::row orow[4];
	auto store_rows = [&](int m) {
		if (!own)
			return;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			if constexpr (LAYOUT == PIX_STEP4 || LAYOUT == PIX_STEP4_BGR) {
				rgbx_store<true>(dst + (long)(4 * m + k) * opitch + 16 * qs, orow[k]);
			} else if constexpr (LAYOUT == PIX_PLANAR) {
				uint8_t *p = dst + (long)(4 * m + k) * opitch + 4 * qs;
#pragma unroll
				for (int c = 0; c < 3; ++c)
					__builtin_nontemporal_store(orow[k].w[c], reinterpret_cast<unsigned *>(p + c * a.cstride));
			} else {
				const U32x3 v = { orow[k].w[0], orow[k].w[1], orow[k].w[2] };
				__builtin_nontemporal_store(v, reinterpret_cast<U32x3 *>(dst + (long)(4 * m + k) * opitch + 12 * qs));
			}
		}
	};
	for (int m = m0; m < m1; ++m) {
#pragma unroll
		for (int ch = 0; ch < 3; ++ch) {
			c2[ch] = hold(n2[ch]);   // the one wait of the iteration (see fwd_level_body)
			c1a[ch] = hold(n1a[ch]);
			c1b[ch] = hold(n1b[ch]);
		}
		if (m > m0)
			store_rows(m - 1);
		if (m + 1 < m1) {
#pragma unroll
			for (int ch = 0; ch < 3; ++ch) {
				n2[ch] = load2(ch, m + 2);
				n1a[ch] = load1(ch, 2 * m + 3);
				n1b[ch] = load1(ch, 2 * m + 4);
			}
		}
		Quad4 rows[3][4];
#pragma unroll
		for (int ch = 0; ch < 3; ++ch) {
			// level k+1, pair m: its odd row, and the even row of the pair after it
			int nd2l = 0, nd2h = 0, ne2l = e2l[ch], ne2h = e2h[ch];
			if (m + 1 < h4) {
				nd2l = c2[ch].dl;
				nd2h = c2[ch].dh;
				ne2l = c2[ch].sl - tdiv4(d2l[ch] + nd2l);
				ne2h = c2[ch].sh - tdiv4(d2h[ch] + nd2h);
			}
			const I2 ll_odd = inv_row_pair(q, a.nquads, d2l[ch] + tdiv2(e2l[ch] + ne2l), d2h[ch] + tdiv2(e2h[ch] + ne2h));
			const I2 ll_next = inv_row_pair(q, a.nquads, ne2l, ne2h);
			d2l[ch] = nd2l;
			d2h[ch] = nd2h;
			e2l[ch] = ne2l;
			e2h[ch] = ne2h;
			// level k, row pairs 2m and 2m+1
#pragma unroll
			for (int half = 0; half < 2; ++half) {
				const int jj = 2 * m + half;
				const I2 nsl = half ? ll_next : ll_odd;
				const Raw1 &n = half ? c1b[ch] : c1a[ch];
				I2 ndl = { 0, 0 }, ndh = { 0, 0 }, nel = cel[ch], neh = ceh[ch];   // the plane's last pair mirrors: x[h] := x[h-2]
				if (jj + 1 < h2) {
					ndl = to_i2(n.dl);
					ndh = to_i2(n.dh);
					nel = i2_sub4(nsl, cdl[ch], ndl);
					neh = i2_sub4(to_i2(n.sh), cdh[ch], ndh);
				}
				rows[ch][2 * half] = inv_row_vals(q, a.nquads, cel[ch], ceh[ch]);
				rows[ch][2 * half + 1] = inv_row_vals(q, a.nquads, i2_add2(cdl[ch], cel[ch], nel), i2_add2(cdh[ch], ceh[ch], neh));
				cdl[ch] = ndl;
				cdh[ch] = ndh;
				cel[ch] = nel;
				ceh[ch] = neh;
			}
		}
#pragma unroll
		for (int k = 0; k < 4; ++k)
			orow[k] = RgbOut<uint8_t, LAYOUT>::of(flip_quad<FL>(rows[0][k], fx), flip_quad<FL>(rows[1][k], fx), flip_quad<FL>(rows[2][k], fx), Clamp{ 0, 255 });
	}
	store_rows(m1 - 1);
}

// ------------------------------------------------------------ coarse tail ---
// Once a plane is at most 64x64 all remaining levels run in one workgroup.s LDS:
// one launch per direction replaces five to six latency-bound level launches.
// Two 64x64 int planes in LDS ping-pong between the row and the column pass.

constexpr int TAIL_MAX = 64;
constexpr int TAIL_THREADS = 1024;

struct TailArgs {
	const int *src;  long src_ps;  int spitch;   // fwd: input plane (w0*h0) | inv: unused
	int *dst;        long dst_ps;  int dpitch2;  // inv: output plane (w0*h0) | fwd: unused
	int *pyr;        long pyr_ps;  int ppitch;   // Mallat pyramid
	int nsteps;
	int ws[DWTX_MAX_LEVELS + 2], hs[DWTX_MAX_LEVELS + 2];   // ws[0]xhs[0] is the tail's finest size
};

// forward lifting of sample pair k of a line (stride st) of length n: low and high
__device__ __forceinline__ void tail_fwd_pair(const int *x, int st, int n, int k, int &lo, int &hi)
{
	const int x0 = x[2 * k * st];
	const bool has_odd = 2 * k + 1 < n;
	const int x1 = has_odd ? x[(2 * k + 1) * st] : 0;
	const int xr = 2 * k + 2 < n ? x[(2 * k + 2) * st] : x0;
	const int d = x1 - tdiv2(x0 + xr);
	const int dl = k ? x[(2 * k - 1) * st] - tdiv2(x[(2 * k - 2) * st] + x0) : d;
	lo = has_odd ? x0 + tdiv4(dl + d) : x0;   // odd length: last even sample passes through
	hi = d;
}

__global__ __launch_bounds__(TAIL_THREADS) void k_fwd_tail(TailArgs t)
{
	__shared__ int A[TAIL_MAX * TAIL_MAX];
	__shared__ int B[TAIL_MAX * TAIL_MAX];
	const int plane = blockIdx.x;
	const int *src = t.src + plane * t.src_ps;
	int *pyr = t.pyr + plane * t.pyr_ps;
	int w = t.ws[0], h = t.hs[0];
	for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {
		const int y = i / w, x = i - y * w;
		A[y * TAIL_MAX + x] = src[(long)y * t.spitch + x];
	}
	__syncthreads();
	for (int s = 0; s < t.nsteps; ++s) {
		const int w2 = t.ws[s + 1], h2 = t.hs[s + 1];
		for (int i = threadIdx.x; i < h * w2; i += TAIL_THREADS) {   // rows: A -> B
			const int r = i / w2, k = i - r * w2;
			int lo, hi;
			tail_fwd_pair(A + r * TAIL_MAX, 1, w, k, lo, hi);
			B[r * TAIL_MAX + k] = lo;
			if (2 * k + 1 < w)
				B[r * TAIL_MAX + w2 + k] = hi;
		}
		__syncthreads();
		for (int i = threadIdx.x; i < h2 * w; i += TAIL_THREADS) {   // columns: B -> A
			const int j = i / w, c = i - j * w;
			int lo, hi;
			tail_fwd_pair(B + c, TAIL_MAX, h, j, lo, hi);
			A[j * TAIL_MAX + c] = lo;
			if (2 * j + 1 < h)
				A[(h2 + j) * TAIL_MAX + c] = hi;
		}
		__syncthreads();
		for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {    // detail subbands out
			const int y = i / w, x = i - y * w;
			if (y >= h2 || x >= w2)
				pyr[(long)y * t.ppitch + x] = A[y * TAIL_MAX + x];
		}
		w = w2;
		h = h2;
	}
	for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {        // root LL
		const int y = i / w, x = i - y * w;
		pyr[(long)y * t.ppitch + x] = A[y * TAIL_MAX + x];
	}
}

// inverse lifting: samples 2k and 2k+1 of a line from its low half s[] and high half d[]
__device__ __forceinline__ void tail_inv_pair(const int *s, const int *d, int st, int n, int k, int &e, int &o)
{
	auto even = [&](int j) {
		const int sj = s[j * st];
		if ((n & 1) && 2 * j == n - 1)
			return sj;
		const int dj = d[j * st];
		const int dp = j ? d[(j - 1) * st] : dj;
		return sj - tdiv4(dp + dj);
	};
	e = even(k);
	o = 0;
	if (2 * k + 1 < n) {
		const int en = 2 * k + 2 < n ? even(k + 1) : e;
		o = d[k * st] + tdiv2(e + en);
	}
}

__global__ __launch_bounds__(TAIL_THREADS) void k_inv_tail(TailArgs t)
{
	__shared__ int A[TAIL_MAX * TAIL_MAX];
	__shared__ int B[TAIL_MAX * TAIL_MAX];
	const int plane = blockIdx.x;
	const int *pyr = t.pyr + plane * t.pyr_ps;
	int *dst = t.dst + plane * t.dst_ps;
	{
		const int w = t.ws[t.nsteps], h = t.hs[t.nsteps];
		for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {
			const int y = i / w, x = i - y * w;
			A[y * TAIL_MAX + x] = pyr[(long)y * t.ppitch + x];
		}
	}
	for (int s = t.nsteps - 1; s >= 0; --s) {
		const int w = t.ws[s], h = t.hs[s], w2 = t.ws[s + 1], h2 = t.hs[s + 1];
		for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {    // detail subbands in
			const int y = i / w, x = i - y * w;
			if (y >= h2 || x >= w2)
				A[y * TAIL_MAX + x] = pyr[(long)y * t.ppitch + x];
		}
		__syncthreads();
		for (int i = threadIdx.x; i < h2 * w; i += TAIL_THREADS) {   // columns: A -> B
			const int j = i / w, c = i - j * w;
			int e, o;
			tail_inv_pair(A + c, A + h2 * TAIL_MAX + c, TAIL_MAX, h, j, e, o);
			B[(2 * j) * TAIL_MAX + c] = e;
			if (2 * j + 1 < h)
				B[(2 * j + 1) * TAIL_MAX + c] = o;
		}
		__syncthreads();
		for (int i = threadIdx.x; i < h * w2; i += TAIL_THREADS) {   // rows: B -> A
			const int r = i / w2, k = i - r * w2;
			int e, o;
			tail_inv_pair(B + r * TAIL_MAX, B + r * TAIL_MAX + w2, 1, w, k, e, o);
			A[r * TAIL_MAX + 2 * k] = e;
			if (2 * k + 1 < w)
				A[r * TAIL_MAX + 2 * k + 1] = o;
		}
		__syncthreads();
	}
	const int w = t.ws[0], h = t.hs[0];
	for (int i = threadIdx.x; i < w * h; i += TAIL_THREADS) {
		const int y = i / w, x = i - y * w;
		dst[(long)y * t.dpitch2 + x] = A[y * TAIL_MAX + x];
	}
}

// ------------------------------------------------------- pixels <-> planes ---

// Where the windows of a view lie (dwtx_pixels; win_off finds window i), in samples, and the planes' side of the
// conversion: W x H pixels of C channels per window, n windows.
struct PixGrid {
	long image_stride, row_pitch;
	WinGrid grid;
	int W, H, C, n;
	long chan_stride;   // RGB: from a pixel's R sample to its G, from G to B (dwtx_pixels::colour_stride()) — 1 interleaved, the channel stride planar, negative where the pixels lie as B, G, R
	int col_step;       // from a pixel to the next one of its row: C interleaved (dwtx_pixels::pixel_step where a view has one), 1 planar
	int fw, fh;         // the FLIP instances: the windows' sides (dwtx_pixels::flip_w, flip_h), inside which a W x H picture is mirrored
};

// The FLIP instances of the conversions (a flipped call's windows): pixel (x, y) of window `win`'s PICTURE lies at the mirrored
// memory position of the window — column fw - 1 - x under DWTX_FLIP_X, row fh - 1 - y under DWTX_FLIP_Y — by the flags of the
// window's table entry.  -> the memory row, and x becomes the memory column.  The flags are the wave's; the two selects are all
// a lane adds.  The other instances keep the code they had.
template <class P>
__device__ __forceinline__ P *flipped_row(P *pix, const PixGrid &g, unsigned win, int &x, int y)
{
	unsigned flags;
	const long off = win_off_flip(g.grid, (int)win, flags);
	x = (flags & DWTX_FLIP_X) ? g.fw - 1 - x : x;
	return pix + off + (long)((flags & DWTX_FLIP_Y) ? g.fh - 1 - y : y) * g.row_pitch;
}

constexpr int PX_LANES = 64, PX_ROWS = 4;   // a workgroup of the conversions: one wave per row, a lane per pixel
// the lane's pixel in that grid -> whether it lies inside w x h
__device__ __forceinline__ bool px_lane(int w, int h, int &x, int &y)
{
	x = blockIdx.x * PX_LANES + (threadIdx.x & (PX_LANES - 1));
	y = blockIdx.y * PX_ROWS + (threadIdx.x / PX_LANES);
	return x < w && y < h;
}
// a pixel's colours (or their residuals) as Y, Co and Cg into its place in the three planes, npix apart
__device__ __forceinline__ void planes_of_rgb(int r, int g, int b, int *dst, long npix)
{
	int y, co, cg;
	ycocg_of(r, g, b, y, co, cg);
	dst[0] = y;
	dst[npix] = co;
	dst[2 * npix] = cg;
}

// pnm.h:69-74 (byte -> int) fused with image.h:52-65 rgb2ycocg.  P = uint8_t, uint16_t for deep pixels or int16_t for signed
// ones, which widen with their sign (the same arithmetic: nothing in it knows the depth, and image.h:53-65 is reversible on
// any int).  grid: (64 pixels of a row, 4 rows, window): a wave reads 64 neighbouring
// pixels of one row, and nothing divides per sample.  Planar RGB: the wave reads 64 neighbouring samples of each plane.
// P = float, _Float16 or __bf16 (dwtx_encode_view_float): the integers the samples quantise to — quant_of with colour c's scale
// and bias, clamped to [L, M] (L: dwtx_pixels::minval, 0 but in the *_view_signed calls) — in any layout the integer instances
// take; those read neither f nor the bounds.
template <class P>
__device__ __forceinline__ int sample_in(P v, const FloatFmt &, int, int, int) { return (int)v; }
template <>
__device__ __forceinline__ int sample_in<float>(float v, const FloatFmt &f, int c, int L, int M) { return quant_of(v, f.scale[c], f.bias[c], (float)L, (float)M); }
template <>
__device__ __forceinline__ int sample_in<_Float16>(_Float16 v, const FloatFmt &f, int c, int L, int M) { return quant_of((float)v, f.scale[c], f.bias[c], (float)L, (float)M); }
template <>
__device__ __forceinline__ int sample_in<__bf16>(__bf16 v, const FloatFmt &f, int c, int L, int M) { return quant_of((float)v, f.scale[c], f.bias[c], (float)L, (float)M); }

// the sample types whose lower bound is 0 whatever the launch says: their instances keep the constant
template <class P>
constexpr bool px_unsigned = std::is_same<P, uint8_t>::value || std::is_same<P, uint16_t>::value;

template <class P, bool FLIP = false>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_planes_from_pixels(int *__restrict__ planes, const P *__restrict__ pix, PixGrid g, int L, int M, FloatFmt f)
{
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const long npix = (long)g.W * g.H;
	for (unsigned win = blockIdx.z; win < (unsigned)g.n; win += gridDim.z) {
		int mx = x;   // (the memory column: x itself but in a mirrored window)
		const P *row = FLIP ? flipped_row(pix, g, win, mx, y) : pix + win_off(g.grid, g.image_stride, (int)win) + (long)y * g.row_pitch;
		int *dst = planes + (long)win * g.C * npix + (long)y * g.W + x;
		if (g.C == 1) {
			dst[0] = sample_in<P>(row[(long)mx * g.col_step], f, 0, L, M);
		} else {
			const P *p = row + (long)mx * g.col_step;
			const int r = sample_in<P>(p[0], f, 0, L, M), gr = sample_in<P>(p[g.chan_stride], f, 1, L, M), b = sample_in<P>(p[2 * g.chan_stride], f, 2, L, M);
			planes_of_rgb(r, gr, b, dst, npix);
		}
	}
}

// image.h:39-50 ycocg2rgb (input clamps included) + pnm.h:108 output clamp, with M (the pixels' maxval) where the
// reference has 255: Y and the output to [0, M], Co and Cg to [-M, M].  P = uint8_t (M = 255) or uint16_t.  With a lower
// bound L of its own (P = int16_t, written as two's complement, and the float types: dwtx_pixels::minval) Y and the output go to
// [L, M] and Co and Cg to [-R, R], R = M - L: the extremes R - B and G - T can reach on samples in [L, M].  Same grid as
// above; only the C samples of the W pixels of a window's H rows are written — with a column step above C nothing between
// the pixels is: no word is read, merged and written back (another stream may be writing the samples in between).
// P = float, _Float16 or __bf16: the same clamped integers through float_of with colour c's scale and bias (f; the integer
// instances do not read it), any layout the integer instances take.
template <class P>
__device__ __forceinline__ P sample_of(int v, const FloatFmt &, int) { return (P)v; }
template <>
__device__ __forceinline__ float sample_of<float>(int v, const FloatFmt &f, int c) { return float_of(v, f.scale[c], f.bias[c]); }
template <>
__device__ __forceinline__ _Float16 sample_of<_Float16>(int v, const FloatFmt &f, int c) { return (_Float16)float_of(v, f.scale[c], f.bias[c]); }
template <>
__device__ __forceinline__ __bf16 sample_of<__bf16>(int v, const FloatFmt &f, int c) { return (__bf16)float_of(v, f.scale[c], f.bias[c]); }

// One pixel of that arithmetic, which the general conversion below and the keys of a clip stack (k_clips_from_planes) share:
// plain_gray is a gray sample's one clamp; an RGB pixel's is rgb_plain.
__device__ __forceinline__ int plain_gray(int v, Clamp M) { return clamp_to(v, M.lo, M.hi); }

template <class P, bool FLIP = false>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_pixels_from_planes(P *__restrict__ pix, const int *__restrict__ planes, PixGrid g, int L_, int M_, FloatFmt f)
{
	const Clamp M = { px_unsigned<P> ? 0 : L_, M_ };
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const long npix = (long)g.W * g.H;
	for (unsigned win = blockIdx.z; win < (unsigned)g.n; win += gridDim.z) {
		int mx = x;   // (the memory column: x itself but in a mirrored window)
		P *row = FLIP ? flipped_row(pix, g, win, mx, y) : pix + win_off(g.grid, g.image_stride, (int)win) + (long)y * g.row_pitch;
		const int *src = planes + (long)win * g.C * npix + (long)y * g.W + x;
		if (g.C == 1) {
			row[(long)mx * g.col_step] = sample_of<P>(plain_gray(src[0], M), f, 0);
		} else {
			rgb_plain(src, npix, M, [&](int c, int v) {
				P *p = row + (long)mx * g.col_step;
				p[c * g.chan_stride] = sample_of<P>(v, f, c);
			});
		}
	}
}

// The conversions of a delta view (dwtx_pixels::delta; P = uint8_t, uint16_t or int16_t): a second pointer and a second grid,
// the base pictures', window for window and colour for colour — each view with its own pitch, strides, step and planar or
// interleaved form; the samples' type, the channels and their order are shared.  Kernels of their own: the instances above keep
// their arguments and their code.  Forward: the planes of the integer picture S - B, both samples widened by their type.
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_planes_from_pixels_delta(int *__restrict__ planes, const P *pix, PixGrid g, const P *base, PixGrid gb)
{
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const long npix = (long)g.W * g.H;
	for (unsigned win = blockIdx.z; win < (unsigned)g.n; win += gridDim.z) {
		const P *p = pix + win_off(g.grid, g.image_stride, (int)win) + (long)y * g.row_pitch + (long)x * g.col_step;
		const P *q = base + win_off(gb.grid, gb.image_stride, (int)win) + (long)y * gb.row_pitch + (long)x * gb.col_step;
		int *dst = planes + (long)win * g.C * npix + (long)y * g.W + x;
		if (g.C == 1)
			dst[0] = (int)p[0] - (int)q[0];
		else
			planes_of_rgb((int)p[0] - (int)q[0], (int)p[g.chan_stride] - (int)q[gb.chan_stride], (int)p[2 * g.chan_stride] - (int)q[2 * gb.chan_stride], dst, npix);
	}
}

// The delta conversion that takes a period (a clip stack, dwtx_pixels::clips: dwtx_encode_view_clips): the base pictures are the
// view's own, window `win` against window win - 1 — one pointer, one grid, and win_off is asked for win - 1 — and the window whose
// index in the stack, at + win, is a multiple of `period` is a key: nothing is subtracted and nothing of a base is loaded (the
// key test is the wave's, a scalar branch), so that window 0's "window -1" is never addressed.  win - 1 of a launch's window 0 is
// the window before a part of the batch (dwtx_pixels::image moved the view and `at` with it: a one-band view's pointer, a grid's
// `first`, which is then at least 1 — win_off's unsigned sum comes out at first - 1).  The view is only read.
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_planes_from_pixels_clips(int *__restrict__ planes, const P *__restrict__ pix, PixGrid g, unsigned at, unsigned period)
{
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const long npix = (long)g.W * g.H;
	const long in = (long)y * g.row_pitch + (long)x * g.col_step;
	for (unsigned win = blockIdx.z; win < (unsigned)g.n; win += gridDim.z) {
		const P *p = pix + win_off(g.grid, g.image_stride, (int)win) + in;
		int *dst = planes + (long)win * g.C * npix + (long)y * g.W + x;
		int q0 = 0, q1 = 0, q2 = 0;
		if ((at + win) % period != 0) {   // a link: the window before
			const P *q = pix + win_off(g.grid, g.image_stride, (int)win - 1) + in;
			q0 = (int)q[0];
			if (g.C != 1) {
				q1 = (int)q[g.chan_stride];
				q2 = (int)q[2 * g.chan_stride];
			}
		}
		if (g.C == 1)
			dst[0] = (int)p[0] - q0;
		else
			planes_of_rgb((int)p[0] - q0, (int)p[g.chan_stride] - q1, (int)p[2 * g.chan_stride] - q2, dst, npix);
	}
}

// Inverse: the residual d under the signed clamps for [-R, R], R = M - L (k_pixels_from_planes with lo = -R, hi = R: gray, Y and
// every sample of d to [-R, R], Co and Cg to [-2R, 2R]), then min(max(B + d, L), M) in P.  R reaches 65535 and 2R + R stays far
// inside an int.  Every sample is read (base) and written (pix) by the same lane, the read first: the two views may be the
// same memory (the in-place decode); the host refuses every other overlap.  Neither pointer is __restrict__ for that.
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_pixels_from_planes_delta(P *pix, const int *__restrict__ planes, PixGrid g, const P *base, PixGrid gb, int L, int M_)
{
	const Clamp M = { L, M_ };
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const long npix = (long)g.W * g.H;
	for (unsigned win = blockIdx.z; win < (unsigned)g.n; win += gridDim.z) {
		P *p = pix + win_off(g.grid, g.image_stride, (int)win) + (long)y * g.row_pitch + (long)x * g.col_step;
		const P *q = base + win_off(gb.grid, gb.image_stride, (int)win) + (long)y * gb.row_pitch + (long)x * gb.col_step;
		const int *src = planes + (long)win * g.C * npix + (long)y * g.W + x;
		if (g.C == 1) {
			const int b0 = (int)q[0];
			p[0] = (P)delta_sample(src[0], b0, M);
		} else {
			int r = (int)q[0], gr = (int)q[gb.chan_stride], b = (int)q[2 * gb.chan_stride];
			rgb_residual(src, npix, M, r, gr, b);
			p[0] = (P)r;
			p[g.chan_stride] = (P)gr;
			p[2 * g.chan_stride] = (P)b;
		}
	}
}

// The conversion of a chain (dwtx_decode_view_chain; dwtx_pixels::chain): windows first .. first + count of ONE view, each the
// delta decode of its residual onto the window before it — S_i = clamp(S_{i-1} + d_i) with exactly the arithmetic of
// k_pixels_from_planes_delta — and the base of the first of them at `base` (the window before the group as it lies in memory,
// or the key: one window behind its own PixGrid).  grid: (64 pixels of a row, 4 rows) and nothing over windows: a lane owns one
// pixel position, loads its base sample(s) once and walks the pictures in order, the running sample in a register.  The chain's
// only dependence is that register: the plane samples of the next CHAIN_AHEAD pictures are loaded before the current one's
// arithmetic and store run (a batch of loads, one wait, then the batch's serial adds), so that the walk waits on memory once a
// batch and not once a picture.  The host guarantees that the base window is disjoint from the written ones (codec.hip,
// chain_disjoint, and decode_device's ordering argument): planes, pixels and base are __restrict__.
constexpr int CHAIN_AHEAD = 4;
struct ChainRaw {
	int v[3];
};
template <int C>
__device__ __forceinline__ ChainRaw chain_load(const int *__restrict__ src, long npix)
{
	ChainRaw r;
	r.v[0] = src[0];
	if (C == 3) {
		r.v[1] = src[npix];
		r.v[2] = src[2 * npix];
	}
	return r;
}
// the first sample of pixel (x, y) of window `win` of a view
template <class P>
__device__ __forceinline__ P *pixel_at(P *pix, const PixGrid &g, int win, int x, int y)
{
	return pix + win_off(g.grid, g.image_stride, win) + (long)y * g.row_pitch + (long)x * g.col_step;
}
// one link: delta_sample, or rgb_residual, onto the running sample — b[] in, b[] out
template <int C>
__device__ __forceinline__ void chain_link(const ChainRaw &r, int (&b)[3], Clamp M)
{
	if (C == 1)
		b[0] = delta_sample(r.v[0], b[0], M);
	else
		rgb_residual(r.v, 1, M, b[0], b[1], b[2]);
}
// The walk of both kernels below: pictures win0 .. win0 + n of the view behind g, their planes from `planes` on, at the lane's
// pixel (x, y).  How the running sample starts is the caller's: `keyed`, and the first picture is a key — its own plain
// conversion, nothing read (q is not looked at) — or the first picture is a link onto the base sample at q, whose G and B are
// qstep and 2 * qstep samples on.  Every later picture is a link onto the one before it.  Keyed is bool where the answer is the
// wave's (a scalar branch), and std::false_type where a caller has no keys: then the key's code is not compiled at all (behind a
// bool that is false the chain kernel's loop came out peeled, twice the code and three SGPRs more).  That caller also forms q
// once per instance of the walk, inside its branch on C, not once before it (two VGPRs).
// Sink: where the running sample goes and, without a key, where it comes from.  IntSink (every integer instance, the code they
// always had): the sample itself into the view, the start from the base sample at q.  FloatSink (k_clips_float_from_planes): the
// view holds floats, which cannot be read back as a base — every picture is stored through sample_of<P> with colour c's scale and
// bias, the running INTEGER starts from the carry picture `in` (int32 planes of the view's W x H, the lane's pixel: one coalesced
// load per colour; q is not looked at), and after the last picture it is left in the carry picture `out` where there is one.
struct IntSink {
	static constexpr bool floats = false;
};
struct FloatSink {
	static constexpr bool floats = true;
	FloatFmt f;
	const int *__restrict__ in;
	int *__restrict__ out;
};
template <class P, int C, class Keyed, class Sink = IntSink>
__device__ __forceinline__ void chain_walk(P *__restrict__ pix, const int *__restrict__ planes, const PixGrid &g, const P *__restrict__ q, long qstep, Keyed keyed,
	Clamp M, int x, int y, int win0, int n, const Sink &sink = Sink())
{
	const long npix = (long)g.W * g.H;
	const long wstep = (long)C * npix;   // from a picture's planes to the next one's
	const long at = (long)y * g.row_pitch + (long)x * g.col_step;
	int b[3] = { 0, 0, 0 };
	if (!keyed) {
		if constexpr (Sink::floats) {
			const int *ci = sink.in + (long)y * g.W + x;
			for (int c = 0; c < C; ++c)
				b[c] = ci[c * npix];
		} else {
			b[0] = (int)q[0];
			if (C == 3) {
				b[1] = (int)q[qstep];
				b[2] = (int)q[2 * qstep];
			}
		}
	}
	const int *src = planes + (long)y * g.W + x;
	auto store = [&](int win) {
		P *p = pix + win_off(g.grid, g.image_stride, win) + at;
		if constexpr (Sink::floats) {
			for (int c = 0; c < C; ++c)
				p[c * g.chan_stride] = sample_of<P>(b[c], sink.f, c);
		} else {
			p[0] = (P)b[0];
			if (C == 3) {
				p[g.chan_stride] = (P)b[1];
				p[2 * g.chan_stride] = (P)b[2];
			}
		}
	};
	ChainRaw nxt[CHAIN_AHEAD], cur[CHAIN_AHEAD];
#pragma unroll
	for (int k = 0; k < CHAIN_AHEAD; ++k)   // (a picture past the walk's end: the last one's planes once more, never used)
		nxt[k] = chain_load<C>(src + (long)min(k, n - 1) * wstep, npix);
	for (int w0 = 0; w0 < n; w0 += CHAIN_AHEAD) {
#pragma unroll
		for (int k = 0; k < CHAIN_AHEAD; ++k)   // the one wait of the iteration
			for (int c = 0; c < C; ++c)
				cur[k].v[c] = hold(nxt[k].v[c]);
		if (w0 + CHAIN_AHEAD < n) {   // the next batch's loads go out before this batch's arithmetic and stores
#pragma unroll
			for (int k = 0; k < CHAIN_AHEAD; ++k)
				nxt[k] = chain_load<C>(src + (long)min(w0 + CHAIN_AHEAD + k, n - 1) * wstep, npix);
		}
#pragma unroll
		for (int k = 0; k < CHAIN_AHEAD; ++k)
			if (w0 + k < n) {
				if (keyed && k == 0 && w0 == 0) {   // the key: its own picture, no base
					if (C == 3)
						rgb_plain(cur[k].v, 1, M, [&](int c, int v) { b[c] = v; });
					else
						b[0] = plain_gray(cur[k].v[0], M);
				} else
					chain_link<C>(cur[k], b, M);
				store(win0 + w0 + k);
			}
	}
	if constexpr (Sink::floats)
		if (sink.out) {   // (the wave's) the segment ends mid-clip: the next launch's first segment goes on from here
			int *co = sink.out + (long)y * g.W + x;
			for (int c = 0; c < C; ++c)
				co[c * npix] = b[c];
		}
}
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_chain_from_planes(P *__restrict__ pix, const int *__restrict__ planes, PixGrid g, const P *__restrict__ base,
	PixGrid gb, int L, int M)
{
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	if (g.C == 1)
		chain_walk<P, 1>(pix, planes, g, pixel_at(base, gb, 0, x, y), gb.chan_stride, std::false_type(), Clamp{ L, M }, x, y, 0, g.n);
	else
		chain_walk<P, 3>(pix, planes, g, pixel_at(base, gb, 0, x, y), gb.chan_stride, std::false_type(), Clamp{ L, M }, x, y, 0, g.n);
}

// The conversion of a clip stack (dwtx_decode_view_clips; dwtx_pixels::clips): windows first .. first + g.n of ONE view, window i of
// the stack a key where i % period == 0 — its samples the plain conversion of its planes, plain_gray / rgb_plain, exactly k_pixels_from_planes'
// arithmetic for the sample type — and a link otherwise: chain_link onto the window before it, unchanged.  grid: (64 pixels of a
// row, 4 rows, SEGMENT): a segment is a maximal run of the group's windows with no key but possibly at its start, and the launch
// walks all of them side by side, each with the walk k_chain_from_planes has (chain_walk) — a lane owns one pixel position, the running sample
// stays in a register, CHAIN_AHEAD pictures' plane loads are in flight ahead of a batch's arithmetic and stores.  Where segment z
// begins and ends follows from first, the count and the period alone: with lead = the windows before the group's first key,
// segment z covers [s, s + period) cut to the group, s = lead + (z - (lead != 0)) * period — blockIdx.z and kernel arguments only,
// so the scalar unit computes it once per wave; no table, nothing from the host.  Only the group's first segment can start
// mid-clip (lead != 0, z == 0): it alone loads a base, window first - 1 as it lies in memory.  Every other segment starts at a key
// and reads no pixels at all.  So within one launch no segment reads a window another segment writes: the one window that is read,
// first - 1, lies before every window of the group, and the launch writes windows first .. first + g.n only (a lane writes each
// position once).  The host's ordering argument (codec.hip, decode_device) has window first - 1 in memory: planes, pixels and
// base are __restrict__.  g is the WHOLE view's grid (windows counted from the stack's first), g.n the group's count.
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_clips_from_planes(P *__restrict__ pix, const int *__restrict__ planes, PixGrid g, const P *__restrict__ base,
	int first, int period, int L_, int M_)
{
	const Clamp M = { px_unsigned<P> ? 0 : L_, M_ };
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	// segment blockIdx.z of the group, in windows of the group: [r0, r1)
	const int phase = first % period, lead = phase ? period - phase : 0;
	const int s = lead + ((int)blockIdx.z - (lead ? 1 : 0)) * period;
	const int r0 = max(s, 0), r1 = min(s + period, g.n);
	if (r0 >= r1)   // (never: the host launches the group's segments and no more)
		return;
	const int *seg = planes + (long)r0 * g.C * g.W * g.H;
	const bool keyed = s >= 0;   // (the wave's)
	const P *q = base;
	if (!keyed)   // the one segment that starts mid-clip: a link onto window first - 1 as it lies in memory
		q = pixel_at(base, g, first + r0 - 1, x, y);
	if (g.C == 1)
		chain_walk<P, 1>(pix, seg, g, q, g.chan_stride, keyed, M, x, y, first + r0, r1 - r0);
	else
		chain_walk<P, 3>(pix, seg, g, q, g.chan_stride, keyed, M, x, y, first + r0, r1 - r0);
}

// The clip stack's conversion into FLOAT windows (dwtx_decode_view_clips_crop with a format; P = float, _Float16 or __bf16): the
// same grid, the same segments and the same walk, with chain_walk's FloatSink.  The view is never read: the one segment that starts
// mid-clip (z == 0 with lead != 0) takes its running integer from the carry picture carry_in, which the launch before this one
// left behind, and the launch's LAST segment leaves its own in carry_out where the host asks for it (the segment ends mid-clip).
// With three segments or more both happen in one launch, in different workgroups: the host hands in two DIFFERENT pictures
// (codec.hip, decode_device: they alternate per launch), so that no workgroup of a launch reads what another one of it writes.
// A kernel of its own: the integer instances above keep their arguments and their code.
template <class P>
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_clips_float_from_planes(P *__restrict__ pix, const int *__restrict__ planes, PixGrid g, int first, int period,
	int L, int M_, FloatFmt f, const int *__restrict__ carry_in, int *__restrict__ carry_out)
{
	const Clamp M = { L, M_ };
	int x, y;
	if (!px_lane(g.W, g.H, x, y))
		return;
	const int phase = first % period, lead = phase ? period - phase : 0;
	const int s = lead + ((int)blockIdx.z - (lead ? 1 : 0)) * period;
	const int r0 = max(s, 0), r1 = min(s + period, g.n);
	if (r0 >= r1)   // (never: the host launches the group's segments and no more)
		return;
	const int *seg = planes + (long)r0 * g.C * g.W * g.H;
	const bool keyed = s >= 0;   // (the wave's)
	const FloatSink sink = { f, carry_in, blockIdx.z == gridDim.z - 1 ? carry_out : nullptr };
	const P *none = nullptr;
	if (g.C == 1)
		chain_walk<P, 1>(pix, seg, g, none, 0, keyed, M, x, y, first + r0, r1 - r0, sink);
	else
		chain_walk<P, 3>(pix, seg, g, none, 0, keyed, M, x, y, first + r0, r1 - r0, sink);
}

// Integer-only synthetic frames: seed = frame index, so every box
// renders identical bytes.  kind 0 "smooth+noise", kind 1 uniform noise.
__global__ __launch_bounds__(256) void k_synth(uint8_t *__restrict__ pix, int W, int H, int C, long total,
	unsigned seed0, int kind)
{
	const long per = (long)W * H * C;
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
		const long img = i / per;
		long r = i - img * per;
		const unsigned k = (unsigned)(r % C);
		r /= C;
		const unsigned x = (unsigned)(r % W), y = (unsigned)(r / W);
		unsigned u = x * 0x9E3779B1u ^ y * 0x85EBCA77u ^ k * 0xC2B2AE3Du ^ (seed0 + (unsigned)img) * 0x27D4EB2Fu;
		u ^= u >> 15;
		u *= 0x2C1B3C6Du;
		u ^= u >> 12;
		u *= 0x297A2D39u;
		u ^= u >> 15;
		int p;
		if (kind) {
			p = (int)(u >> 24);
		} else {
			int tx = (int)(x % 192u) - 96, ty = (int)(y % 128u) - 64;
			p = 40 + (tx < 0 ? -tx : tx) + (ty < 0 ? -ty : ty) + 10 * (int)k + (int)(u >> 29);
		}
		pix[i] = (uint8_t)p;
	}
}

// The steps of a W*H transform, fine to coarse: step t takes the ws[t] x hs[t] plane to its ws[t+1] x hs[t+1] LL band and
// three detail bands (encode.c:24-29: recurse while both halves are >= N0; the first step always runs).  The steps from
// tail_from on run in one launch of the LDS tail kernel.  The LL bands between the finest step and the pyramid live in two
// scratch planes: level1 holds the ws[1] x hs[1] band of every plane, small the bands from ws[2] x hs[2] down.
struct LiftLayout {
	int T, tail_from;
	int ws[DWTX_MAX_LEVELS + 2], hs[DWTX_MAX_LEVELS + 2];
	int *level1, *small;   // null where no step needs them
};

// (cols and first in 32 bits: both are window counts of one call, at most DWTX_MAX_PLANES_PER_CALL — dwtx_count_ok — so that
// win_off's unsigned `i + first` cannot wrap)
WinGrid win_grid(const dwtx_pixels &px) { return WinGrid{ (unsigned)px.cols, (unsigned)px.first, (long)px.band_stride, px.offs }; }

// ctx null: the sizes only
int lift_layout(dwtx_ctx *ctx, int W, int H, int nplanes, LiftLayout &L)
{
	int n = 0;
	L.ws[0] = W;
	L.hs[0] = H;
	do {
		L.ws[n + 1] = (L.ws[n] + 1) >> 1;
		L.hs[n + 1] = (L.hs[n] + 1) >> 1;
		++n;
	} while (n < DWTX_MAX_LEVELS && L.ws[n] >= DWTX_MIN_LEN && L.hs[n] >= DWTX_MIN_LEN);
	L.T = n;
	int t = 0;
	while (t < n && (L.ws[t] > TAIL_MAX || L.hs[t] > TAIL_MAX))
		++t;
	L.tail_from = t;
	L.level1 = L.small = nullptr;
	if (ctx && n > 1 && !(L.level1 = (int *)dwtx_scratch(ctx, SLOT_LIFT_A, sizeof(int) * (size_t)L.ws[1] * L.hs[1] * nplanes)))
		return DWTX_ERR_NOMEM;
	if (ctx && n > 2 && !(L.small = (int *)dwtx_scratch(ctx, SLOT_LIFT_B, sizeof(int) * (size_t)L.ws[2] * L.hs[2] * nplanes)))
		return DWTX_ERR_NOMEM;
	return DWTX_OK;
}

// 16-bit detail bands (dwtx_p16) come from the wide forward kernel reading 8-bit pixels, on at most this many of the
// finest levels: the magnitude bound of k_fwd_level_w
constexpr int LEVELS16_MAX = 5;

} // namespace

extern "C" int dwtx_synth_pixels(dwtx_ctx *ctx, uint8_t *pix, int W, int H, int C, int n, unsigned seed0, int kind)
{
	if (!ctx || !pix || W < 1 || H < 1 || (C != 1 && C != 3) || n < 1)
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	const long total = (long)W * H * C * n;
	const int blocks = (int)min((total + 255) / 256, (long)256 * 16);
	hipLaunchKernelGGL(k_synth, dim3(blocks), dim3(256), 0, ctx->stream, pix, W, H, C, total, seed0, kind);
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// the conversions' view of px and their launch grid; the kernels' `pix` is px.red(): the R sample of the grid's first pixel,
// from which chan_stride leads to G and B — upwards, or down to the base for B, G, R pixels
static PixGrid pix_grid(const dwtx_pixels &px, int W, int H, int n, dim3 *grid)
{
	*grid = dim3((unsigned)dwtx_cdiv(W, PX_LANES), (unsigned)dwtx_cdiv(H, PX_ROWS), (unsigned)min(n, 65535));
	return PixGrid{ (long)px.image_stride, (long)px.pitch(W), win_grid(px), W, H, px.channels, n, px.colour_stride(), (int)px.step(), px.flip_w, px.flip_h };
}

// the kernels' copy of a float destination's conversion (integer pixels: the identity, which nothing reads)
static FloatFmt float_fmt(const dwtx_pixels &px)
{
	FloatFmt f;
	for (int c = 0; c < 3; ++c) {
		f.scale[c] = px.scale[c];
		f.bias[c] = px.bias[c];
	}
	f.bf16 = px.kind == DWTX_SAMPLE_BF16;
	f.sext = px.minval < 0;
	return f;
}

// The one place a view's sample kind (dwtx_pixels::kind) becomes the kernels' sample type: call(SampleType<P>()) with the kind's P,
// once, -> DWTX_OK; or nothing is called -> DWTX_ERR_ARG: a kind that is none, or a float kind where the caller admits
// INT_SAMPLES only (the delta, chain and clips conversions, which have integer instances and no others: `call` is not
// compiled for a float type there).
template <class P>
struct SampleType {
	typedef P type;
};
enum SampleKinds { INT_SAMPLES, ANY_SAMPLES };
template <SampleKinds ADMITS, class F>
static int with_sample_type(int kind, F &&call)
{
	switch (kind) {
	case DWTX_SAMPLE_U8:
		call(SampleType<uint8_t>());
		return DWTX_OK;
	case DWTX_SAMPLE_U16:
		call(SampleType<uint16_t>());
		return DWTX_OK;
	case DWTX_SAMPLE_S16:
		call(SampleType<int16_t>());
		return DWTX_OK;
	}
	if constexpr (ADMITS == ANY_SAMPLES)
		switch (kind) {
		case DWTX_SAMPLE_F32:
			call(SampleType<float>());
			return DWTX_OK;
		case DWTX_SAMPLE_F16:
			call(SampleType<_Float16>());
			return DWTX_OK;
		case DWTX_SAMPLE_BF16:
			call(SampleType<__bf16>());
			return DWTX_OK;
		}
	return DWTX_ERR_ARG;
}

// what the two general entry points ask of their arguments before anything else
static bool conversion_args_ok(const dwtx_ctx *ctx, const int32_t *planes, const dwtx_pixels &px, int W, int H, int n)
{
	const int C = px.channels;
	if (!ctx || !planes || !px.base || W < 1 || H < 1 || (C != 1 && C != 3) || n < 1 || !px.sample_aligned())
		return false;
	return !px.flips || (px.offs && W <= px.flip_w && H <= px.flip_h);   // (a picture is mirrored inside its window: the mirrored index stays in it)
}

// a delta view's conversions (dwtx_pixels::delta): to_planes, or from_planes — integer samples on a grid, nothing flipped or listed
static int launch_delta(dwtx_ctx *ctx, dim3 grid, const dwtx_pixels &px, const PixGrid &g, int W, int H, int n, int32_t *to_planes, const int32_t *from_planes)
{
	if (px.chain || px.clips || px.is_float() || px.flips || px.listed() || !px.base_pixels().sample_aligned())   // (a chain and a clip stack have conversions of their own, below)
		return DWTX_ERR_ARG;
	const dwtx_pixels bp = px.base_pixels();
	dim3 same;
	const PixGrid gb = pix_grid(bp, W, H, n, &same);
	return with_sample_type<INT_SAMPLES>(px.kind, [&](auto t) {
		using P = typename decltype(t)::type;
		if (to_planes)
			hipLaunchKernelGGL(k_planes_from_pixels_delta<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, to_planes, static_cast<const P *>(px.red()), g,
				static_cast<const P *>(bp.red()), gb);
		else
			hipLaunchKernelGGL(k_pixels_from_planes_delta<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, static_cast<P *>(px.red()), from_planes, g,
				static_cast<const P *>(bp.red()), gb, px.minval, px.maxval);
	});
}

int dwtx_planes_to_pixels_chain(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count)
{
	const int C = px.channels;
	if (!ctx || !planes || !px.base || !px.chain || !px.key.base || W < 1 || H < 1 || (C != 1 && C != 3) || first < 0 || count < 1)
		return DWTX_ERR_ARG;
	if (px.is_float() || px.flips || px.listed() || !px.sample_aligned() || !px.key_pixels().sample_aligned() || !px.range_ok())
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	// the written windows, and the one before them as a view of one window: the key, or window first - 1 of the view itself
	dwtx_pixels own = px;
	own.chain = false;
	own.key = dwtx_base_grid();
	const dwtx_pixels dst = own.image((size_t)first);
	const dwtx_pixels bp = first ? own.image((size_t)first - 1) : px.key_pixels();
	dim3 grid, one;
	const PixGrid g = pix_grid(dst, W, H, count, &grid);
	const PixGrid gb = pix_grid(bp, W, H, 1, &one);
	grid.z = 1;   // (the pictures of a chain are walked in order by each lane)
	const int rc = with_sample_type<INT_SAMPLES>(px.kind, [&](auto t) {
		using P = typename decltype(t)::type;
		hipLaunchKernelGGL(k_chain_from_planes<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, static_cast<P *>(dst.red()), planes, g,
			static_cast<const P *>(bp.red()), gb, dst.minval, dst.maxval);
	});
	if (rc)
		return rc;
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// A clip stack's conversion back (dwtx_pixels::clips): the view's own grid is the base pictures' too
int dwtx_planes_to_pixels_clips(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count)
{
	const int C = px.channels;
	if (!ctx || !planes || !px.base || px.clips < 1 || px.clip_at || px.chain || px.delta.base || W < 1 || H < 1 || (C != 1 && C != 3) || first < 0 || count < 1)
		return DWTX_ERR_ARG;
	if (px.is_float() || px.flips || px.listed() || !px.sample_aligned() || !px.range_ok())
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	dim3 grid;
	const PixGrid g = pix_grid(px, W, H, count, &grid);
	// the group's segments: the run before its first key, if it starts mid-clip, and one per key
	const int phase = first % px.clips, lead = phase ? px.clips - phase : 0;
	grid.z = lead >= count ? 1u : (unsigned)((lead ? 1 : 0) + dwtx_cdiv(count - lead, px.clips));
	const int rc = with_sample_type<INT_SAMPLES>(px.kind, [&](auto t) {
		using P = typename decltype(t)::type;
		hipLaunchKernelGGL(k_clips_from_planes<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, static_cast<P *>(px.red()), planes, g,
			static_cast<const P *>(px.red()), first, px.clips, px.minval, px.maxval);
	});
	if (rc)
		return rc;
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// A clip stack's conversion into float windows: the same segments, the carry pictures in place of the view as a base
int dwtx_planes_to_pixels_clips_float(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int first, int count,
	const int32_t *carry_in, int32_t *carry_out)
{
	const int C = px.channels;
	if (!ctx || !planes || !px.base || px.clips < 1 || px.clip_at || px.chain || px.delta.base || W < 1 || H < 1 || (C != 1 && C != 3) || first < 0 || count < 1)
		return DWTX_ERR_ARG;
	if (!px.is_float() || px.flips || px.listed() || !px.sample_aligned() || !px.range_ok())
		return DWTX_ERR_ARG;
	const int phase = first % px.clips, lead = phase ? px.clips - phase : 0;
	if ((lead && !carry_in) || (carry_in && carry_in == carry_out))   // a segment that starts mid-clip has nothing else to start from
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	dim3 grid;
	const PixGrid g = pix_grid(px, W, H, count, &grid);
	grid.z = lead >= count ? 1u : (unsigned)((lead ? 1 : 0) + dwtx_cdiv(count - lead, px.clips));
	const FloatFmt f = float_fmt(px);
	auto launch = [&](auto t) {
		using P = typename decltype(t)::type;
		hipLaunchKernelGGL(k_clips_float_from_planes<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, static_cast<P *>(px.red()), planes, g,
			first, px.clips, px.minval, px.maxval, f, carry_in, carry_out);
	};
	switch (px.kind) {   // (the float kinds alone: with_sample_type would compile an integer walk through FloatSink too)
	case DWTX_SAMPLE_F32:
		launch(SampleType<float>());
		break;
	case DWTX_SAMPLE_F16:
		launch(SampleType<_Float16>());
		break;
	default:
		launch(SampleType<__bf16>());
		break;
	}
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// The general conversions: a clip stack's and a delta view's have kernels of their own (integer samples), every other view takes
// the instance for its sample type — the FLIP one for a flipped call's windows.
int dwtx_pixels_to_planes(dwtx_ctx *ctx, int32_t *planes, const dwtx_pixels &px, int W, int H, int n)
{
	if (!conversion_args_ok(ctx, planes, px, W, H, n))
		return DWTX_ERR_ARG;
	if (px.is_float() && !px.range_ok())   // (the quantiser's clamp; integer sources have no use for a maxval)
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	dim3 grid;
	const PixGrid g = pix_grid(px, W, H, n, &grid);
	const FloatFmt f = float_fmt(px);
	int rc;
	if (px.clips) {   // (before the delta views: a clip stack has no second grid, the view's own is the base pictures' too)
		if (px.chain || px.delta.base || px.is_float() || px.flips || px.listed())
			return DWTX_ERR_ARG;
		rc = with_sample_type<INT_SAMPLES>(px.kind, [&](auto t) {
			using P = typename decltype(t)::type;
			hipLaunchKernelGGL(k_planes_from_pixels_clips<P>, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, planes, static_cast<const P *>(px.red()), g,
				(unsigned)(px.clip_at % (size_t)px.clips), (unsigned)px.clips);
		});
	} else if (px.is_delta()) {
		rc = launch_delta(ctx, grid, px, g, W, H, n, planes, nullptr);
	} else {
		rc = with_sample_type<ANY_SAMPLES>(px.kind, [&](auto t) {
			using P = typename decltype(t)::type;
			const auto kernel = px.flips ? k_planes_from_pixels<P, true> : k_planes_from_pixels<P, false>;
			hipLaunchKernelGGL(kernel, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, planes, static_cast<const P *>(px.red()), g, px.minval, px.maxval, f);
		});
	}
	if (rc)
		return rc;
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

int dwtx_planes_to_pixels(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *planes, int W, int H, int n)
{
	if (!conversion_args_ok(ctx, planes, px, W, H, n))
		return DWTX_ERR_ARG;
	if (!px.range_ok())
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	dim3 grid;
	const PixGrid g = pix_grid(px, W, H, n, &grid);
	const FloatFmt f = float_fmt(px);
	int rc;
	if (px.is_delta()) {
		rc = launch_delta(ctx, grid, px, g, W, H, n, nullptr, planes);
	} else {
		rc = with_sample_type<ANY_SAMPLES>(px.kind, [&](auto t) {
			using P = typename decltype(t)::type;
			const auto kernel = px.flips ? k_pixels_from_planes<P, true> : k_pixels_from_planes<P, false>;
			hipLaunchKernelGGL(kernel, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, static_cast<P *>(px.red()), planes, g, px.minval, px.maxval, f);
		});
	}
	if (rc)
		return rc;
	DWTX_LAUNCH_CHECK();
	return DWTX_OK;
}

// (an odd pointer to 16-bit samples fails the launchers' sample_aligned())
extern "C" int dwtx_planes_from_pixels(dwtx_ctx *ctx, int32_t *planes, const uint8_t *pix, int W, int H, int C, int n)
{
	return dwtx_pixels_to_planes(ctx, planes, dwtx_pixels8(pix, C, (size_t)W * H * C), W, H, n);
}

extern "C" int dwtx_planes_from_pixels16(dwtx_ctx *ctx, int32_t *planes, const uint16_t *pix, int W, int H, int C, int n)
{
	return dwtx_pixels_to_planes(ctx, planes, dwtx_pixels16(pix, C, (size_t)W * H * C), W, H, n);
}

extern "C" int dwtx_pixels_from_planes(dwtx_ctx *ctx, uint8_t *pix, const int32_t *planes, int W, int H, int C, int n)
{
	return dwtx_planes_to_pixels(ctx, dwtx_pixels8(pix, C, (size_t)W * H * C), planes, W, H, n);
}

extern "C" int dwtx_pixels16_from_planes(dwtx_ctx *ctx, uint16_t *pix, const int32_t *planes, int W, int H, int C, int n, int maxval)
{
	return dwtx_planes_to_pixels(ctx, dwtx_pixels16(pix, C, (size_t)W * H * C, maxval), planes, W, H, n);
}

static bool aligned_to(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Fewer rows per wave on small levels so that a few thousand waves are in flight: `start` halved, not below `floor`,
// while `strips` columns of waves (all planes) over `rows` rows make fewer than 4096
static int fill_chip(int start, int floor, long strips, int rows)
{
	int r = start;
	while (r > floor && strips * dwtx_cdiv(rows, r) < 4096)
		r >>= 1;
	return r;
}

// DWTX_OPT_LIFT_ROWS: 0, or the row pairs per wave strip that every one-level launch of the context takes instead of
// fill_chip()'s choice (the two-level launches an eighth of it) — the launch shapes a large batch gets, on any batch
static int forced_rows(const dwtx_ctx *ctx, int *forced)
{
	const long v = ctx->opt[DWTX_OPT_LIFT_ROWS];
	if (v != 0 && v != 4 && v != 8 && v != 16 && v != 32 && v != MAX_ROWS_PER_WAVE) {
		dwtx_set_error("DWTX_OPT_LIFT_ROWS is %ld: it takes 0 (automatic), 4, 8, 16, 32 or %d row pairs per wave strip", v, MAX_ROWS_PER_WAVE);
		return DWTX_ERR_ARG;
	}
	*forced = (int)v;
	return DWTX_OK;
}

// row pairs per wave of the one-level kernels (their waves are counted on h2 rounded up to whole strips of the start)
static int pick_rpw(int strips_x, int h2, int nplanes, int forced)
{
	if (forced)
		return forced;
	return fill_chip(MAX_ROWS_PER_WAVE, 4, (long)strips_x * nplanes, dwtx_cdiv(h2, MAX_ROWS_PER_WAVE) * MAX_ROWS_PER_WAVE);
}

// coarse row pairs per wave of the two-level kernels
static int pick_mpw(int strips_x, int h4, int nplanes, int forced)
{
	if (forced)
		return forced / 8 > 2 ? forced / 8 : 2;
	return fill_chip(F2_MPW, 2, (long)strips_x * nplanes, h4);
}

// the LDS tail's steps tail_from .. T-1 of a pyramid; the caller adds the plane it reads (forward) or writes (inverse)
static TailArgs tail_args(const LiftLayout &L, int *pyr)
{
	TailArgs ta{};
	ta.pyr = pyr;
	ta.pyr_ps = (long)L.ws[0] * L.hs[0];
	ta.ppitch = L.ws[0];
	ta.nsteps = L.T - L.tail_from;
	for (int k = 0; k <= ta.nsteps; ++k) {
		ta.ws[k] = L.ws[L.tail_from + k];
		ta.hs[k] = L.hs[L.tail_from + k];
	}
	return ta;
}

using WideKernel = void (*)(LevelArgsW);
using Inv2Kernel = void (*)(Inv2Args);

// ------------------------------------------------------------- pixel ends ---
// A pixel end: the pixels that the finest wide level reads (forward) or writes (inverse) in place of an int32 plane, as far as
// they choose a kernel.  wide_end() is the one place that looks at a view's layout for that, once per
// call; wide_row() finds the end's row in the one table of kernels, and a view has wide kernels if it has a row
// (dwtx_pixels_ok).  A new pixel format is its kernels and one row.
enum WideKind { WK_U8, WK_U16, WK_S16, WK_F32, WK_H16 };   // (H16: fp16 and bf16, which FloatFmt::bf16 tells apart)
enum WideLayout { WL_NONE, WL_GRAY, WL_PACKED, WL_STEP4, WL_PLANAR };   // NONE: a pixel step that no wide kernel addresses; STEP4: dwtx_pixels::rgbx8()
// BGR: interleaved pixels that lie as B, G, R run their layout's twin kernels (planar ones their layout's own, from the R plane with
// a negative channel stride: wide_base, wide_cstride).  DELTA: a delta view.  FAR: float samples that quantise beyond [0, 255]
// (dwtx_pixels::deep_source()), whose forward kernels keep neither histograms nor 16-bit bands.
enum WideFlags { WE_BGR = 1, WE_DELTA = 2, WE_FAR = 4 };
struct WideEnd {
	int kind, layout;
	unsigned flags;
	bool operator==(const WideEnd &o) const { return kind == o.kind && layout == o.layout && flags == o.flags; }
};

static WideEnd wide_end(const dwtx_pixels &px)
{
	WideEnd e;
	e.kind = px.kind == DWTX_SAMPLE_U8 ? WK_U8 : px.kind == DWTX_SAMPLE_U16 ? WK_U16 : px.kind == DWTX_SAMPLE_S16 ? WK_S16 : px.kind == DWTX_SAMPLE_F32 ? WK_F32 : WK_H16;
	e.layout = px.stepped() && !px.rgbx8() ? WL_NONE : px.channels != 3 ? WL_GRAY : px.planar() ? WL_PLANAR : px.rgbx8() ? WL_STEP4 : WL_PACKED;
	e.flags = (px.bgr() && e.layout != WL_PLANAR ? WE_BGR : 0u) | (px.is_delta() ? WE_DELTA : 0u) | (px.is_float() && px.deep_source() ? WE_FAR : 0u);
	return e;
}

// What the wide kernels get as src8 / dst8 and as cstride (the order of planar channels changes no kernel, see WE_BGR)
static const uint8_t *wide_base(const dwtx_pixels &px) { return px.planar() ? static_cast<const uint8_t *>(px.red()) : px.u8(); }
static long wide_cstride(const dwtx_pixels &px) { return px.channels == 3 && px.planar() ? px.colour_stride() : 0; }

// The kernels of a pixel end; a null entry: the instance is not built, and a call that needs it is refused.
struct FwdSet {
	WideKernel k[2][2];   // [histograms ride along][a flipped call's windows: FY]
};
struct InvSet {
	WideKernel k[2][3];   // one level, [the detail bands are 16-bit values][FL: flip_level()]
	Inv2Kernel k2[3];     // two levels in one pass, [FL]: from 16-bit bands only, which only 8-bit pixels take
};
struct WideRow {
	WideEnd end;     // the key
	bool rgb_grid;   // forward, FwdSrc<>::RGB_GRID: three workgroups per strip and nplanes / 3 in z, against one workgroup column per plane
	                 // (every inverse RGB kernel takes three planes per wave: WideRow::rgb())
	FwdSet fwd;
	InvSet inv;
	bool rgb() const { return end.layout != WL_GRAY; }
};

// The sets the rows are made of.  Forward: deep samples (no histograms: the bounds are for 8-bit sources), delta views (nor flips),
// 8-bit pixels, float samples by their route.  Inverse: the sink's sample type, and for RGB its layout.
#define FL3(kernel, ...) { kernel<__VA_ARGS__, 0>, kernel<__VA_ARGS__, 1>, kernel<__VA_ARGS__, 2> }
template <int SRC> static constexpr FwdSet fwd_deep() { return { { { k_fwd_level_w<false, SRC>, k_fwd_level_w<false, SRC, true> }, {} } }; }
template <int SRC> static constexpr FwdSet fwd_delta() { return { { { k_fwd_level_w<false, SRC>, nullptr }, {} } }; }
template <class S> static constexpr FwdSet fwd_pix8()
{
	return { { { k_fwd_pixels_w<S, false>, k_fwd_pixels_w<S, false, true> }, { k_fwd_pixels_w<S, true>, k_fwd_pixels_w<S, true, true> } } };
}
template <class S> static constexpr FwdSet fwd_float()
{
	return { { { k_fwd_float_w<S, false>, k_fwd_float_w<S, false, true> }, { k_fwd_float_w<S, true>, k_fwd_float_w<S, true, true> } } };
}
template <class S> static constexpr FwdSet fwd_float_far() { return { { { k_fwd_float_w<S, false>, k_fwd_float_w<S, false, true> }, {} } }; }
static constexpr InvSet inv_gray8() { return { { FL3(k_inv_level_w, uint8_t, false), FL3(k_inv_level_w, uint8_t, true) }, FL3(k_inv2_level_w, uint8_t, true) }; }
static constexpr InvSet inv_gray_deep() { return { { FL3(k_inv_level_w, uint16_t, false), {} }, {} }; }   // (int16_t samples too: the lower clamp, LevelArgs::minval)
template <class F> static constexpr InvSet inv_gray_float() { return { { FL3(k_inv_level_w, F, false), FL3(k_inv_level_w, F, true) }, {} }; }
template <class P> static constexpr InvSet inv_gray_delta() { return { { { k_inv_level_w<DeltaPix<P>, false, 0>, nullptr, nullptr }, {} }, {} }; }
template <PixLayout L> static constexpr InvSet inv_rgb8()
{
	return { { FL3(k_inv_level_w_rgb, false, uint8_t, L), FL3(k_inv_level_w_rgb, true, uint8_t, L) }, FL3(k_inv2_level_w_rgb, true, L) };
}
template <PixLayout L> static constexpr InvSet inv_rgb_deep() { return { { FL3(k_inv_level_w_rgb, false, uint16_t, L), {} }, {} }; }
template <class F> static constexpr InvSet inv_planar_float()
{
	return { { FL3(k_inv_level_w_rgb, false, F, PIX_PLANAR), FL3(k_inv_level_w_rgb, true, F, PIX_PLANAR) }, {} };
}
template <PixLayout L> static constexpr InvSet inv_rgb_delta() { return { { { k_inv_level_w_rgb<false, DeltaPix<uint8_t>, L, 0>, nullptr, nullptr }, {} }, {} }; }
#undef FL3

static const WideRow *wide_row(const WideEnd &e)
{
	static constexpr WideRow ROWS[] = {
		// 8-bit pixels: histograms, 16-bit bands and the two-level inverse
		{ { WK_U8, WL_GRAY, 0 }, false, fwd_pix8<uint8_t>(), inv_gray8() },
		{ { WK_U8, WL_PACKED, 0 }, true, fwd_pix8<Rgb8>(), inv_rgb8<PIX_PACKED>() },
		{ { WK_U8, WL_PACKED, WE_BGR }, true, fwd_pix8<Bgr8>(), inv_rgb8<PIX_PACKED_BGR>() },
		{ { WK_U8, WL_STEP4, 0 }, true, fwd_pix8<Rgbx8>(), inv_rgb8<PIX_STEP4>() },
		{ { WK_U8, WL_STEP4, WE_BGR }, true, fwd_pix8<Bgrx8>(), inv_rgb8<PIX_STEP4_BGR>() },
		{ { WK_U8, WL_PLANAR, 0 }, true, fwd_pix8<RgbP8>(), inv_rgb8<PIX_PLANAR>() },
		// deep pixels, and their signed twins: sources of their own, the same sinks
		{ { WK_U16, WL_GRAY, 0 }, false, fwd_deep<SRC_U16>(), inv_gray_deep() },
		{ { WK_U16, WL_PACKED, 0 }, false, fwd_deep<SRC_RGB16>(), inv_rgb_deep<PIX_PACKED>() },
		{ { WK_U16, WL_PACKED, WE_BGR }, false, fwd_deep<SRC_BGR16>(), inv_rgb_deep<PIX_PACKED_BGR>() },
		{ { WK_U16, WL_PLANAR, 0 }, false, fwd_deep<SRC_RGBP16>(), inv_rgb_deep<PIX_PLANAR>() },
		{ { WK_S16, WL_GRAY, 0 }, false, fwd_deep<SRC_S16>(), inv_gray_deep() },
		{ { WK_S16, WL_PACKED, 0 }, false, fwd_deep<SRC_RGB16S>(), inv_rgb_deep<PIX_PACKED>() },
		{ { WK_S16, WL_PACKED, WE_BGR }, false, fwd_deep<SRC_BGR16S>(), inv_rgb_deep<PIX_PACKED_BGR>() },
		{ { WK_S16, WL_PLANAR, 0 }, false, fwd_deep<SRC_RGBP16S>(), inv_rgb_deep<PIX_PLANAR>() },
		// float samples, gray or planar RGB (interleaved float RGB has no wide kernel); the sinks do not ask about the route
		{ { WK_F32, WL_GRAY, 0 }, false, fwd_float<FloatPix<float, false, false>>(), inv_gray_float<float>() },
		{ { WK_H16, WL_GRAY, 0 }, false, fwd_float<FloatPix<Half16, false, false>>(), inv_gray_float<Half16>() },
		{ { WK_F32, WL_PLANAR, 0 }, true, fwd_float<FloatPix<float, true, false>>(), inv_planar_float<float>() },
		{ { WK_H16, WL_PLANAR, 0 }, true, fwd_float<FloatPix<Half16, true, false>>(), inv_planar_float<Half16>() },
		{ { WK_F32, WL_GRAY, WE_FAR }, false, fwd_float_far<FloatPix<float, false, true>>(), inv_gray_float<float>() },
		{ { WK_H16, WL_GRAY, WE_FAR }, false, fwd_float_far<FloatPix<Half16, false, true>>(), inv_gray_float<Half16>() },
		{ { WK_F32, WL_PLANAR, WE_FAR }, false, fwd_float_far<FloatPix<float, true, true>>(), inv_planar_float<float>() },
		{ { WK_H16, WL_PLANAR, WE_FAR }, false, fwd_float_far<FloatPix<Half16, true, true>>(), inv_planar_float<Half16>() },
		// delta views: dense pixels, gray or interleaved 8-bit RGB; never flipped, never from 16-bit bands
		{ { WK_U8, WL_GRAY, WE_DELTA }, false, fwd_delta<SRC_DELTA_U8>(), inv_gray_delta<uint8_t>() },
		{ { WK_U16, WL_GRAY, WE_DELTA }, false, fwd_delta<SRC_DELTA_U16>(), inv_gray_delta<uint16_t>() },
		{ { WK_S16, WL_GRAY, WE_DELTA }, false, fwd_delta<SRC_DELTA_S16>(), inv_gray_delta<int16_t>() },
		{ { WK_U8, WL_PACKED, WE_DELTA }, false, fwd_delta<SRC_DELTA_RGB8>(), inv_rgb_delta<PIX_PACKED>() },
		{ { WK_U8, WL_PACKED, WE_DELTA | WE_BGR }, false, fwd_delta<SRC_DELTA_BGR8>(), inv_rgb_delta<PIX_PACKED_BGR>() },
	};
	for (const WideRow &r : ROWS)
		if (r.end == e)
			return &r;
	return nullptr;
}

// No pixels: the wide kernels from plane to plane, which no row chooses — forward from int32 planes or (src16) from the 16-bit
// bands of the level before, inverse from int32 or (det16) from 16-bit detail bands
static WideKernel fwd_band_kernel(bool src16, bool hist)
{
	static constexpr WideKernel K[2][2] = { { k_fwd_level_w<false, SRC_I32>, k_fwd_level_w<true, SRC_I32> }, { k_fwd_level_w<false, SRC_I16>, k_fwd_level_w<true, SRC_I16> } };
	return K[src16][hist];
}
static WideKernel inv_band_kernel(bool det16) { return det16 ? k_inv_level_w<int, true> : k_inv_level_w<int, false>; }
static Inv2Kernel inv2_band_kernel(bool det16) { return det16 ? k_inv2_level_w<int, true> : k_inv2_level_w<int, false>; }

// FL of the kernels that write these pixels: 0, or for a flipped call's windows 1 (upright and bottom-up ones) or 2 (a mirrored one among them)
static int flip_level(const dwtx_pixels *px) { return !px || !px->flips ? 0 : px->flip_x ? 2 : 1; }

// What the drivers below fill in more than one place.
// A view behind src8 / dst8 / base8: its base, its window stride, its pitch (in samples, like the stride) and its grid of windows
template <class B>
static void pixel_block(const dwtx_pixels &px, int W, B *&base, long &image_ps, int &pitch, WinGrid &grid)
{
	base = const_cast<B *>(wide_base(px));
	image_ps = (long)px.image_stride;
	pitch = (int)px.pitch(W);
	grid = win_grid(px);
}

// a delta view's base pictures for its source or sink (every other view leaves the fields empty: no other kernel reads them)
static void delta_base(LevelArgsW &A, const dwtx_pixels &px, int W)
{
	if (px.is_delta())
		pixel_block(px.base_pixels(), W, A.base8, A.base_ps, A.bpitch, A.bgrid);
}

// Can a level of width w run its wide kernel?  `quads` is the band whose lanes take four samples of a row at once — the source of
// a forward step, the output of an inverse one; pixels where pix is not null, whose own rule is dwtx_pixels::wide() — and the other
// two bands are touched a pair at a time.
struct BandAt {
	const void *p;
	long ps;
	int pitch;
};
static bool wide_level(int w, const dwtx_pixels *pix, const BandAt &quads, const BandAt &pairs_a, const BandAt &pairs_b)
{
	return w % 4 == 0 && quads.pitch % 4 == 0 && quads.ps % 4 == 0 && (pix ? pix->wide() : aligned_to(quads.p, 16)) &&
		pairs_a.pitch % 2 == 0 && pairs_a.ps % 2 == 0 && aligned_to(pairs_a.p, 8) &&
		pairs_b.pitch % 2 == 0 && pairs_b.ps % 2 == 0 && aligned_to(pairs_b.p, 8);
}

// The inverse LDS tail, steps T-1 .. tail_from of the pyramid in one launch: plane tail_from of every picture goes to dst, whole,
// and is the LL band that the next launch reads
static int inv_tail(dwtx_ctx *ctx, const LiftLayout &L, int *pyr, int nplanes, int *dst, const int *&cur, long &cur_ps, int &cur_pitch)
{
	TailArgs ta = tail_args(L, pyr);
	ta.dst = dst;
	ta.dst_ps = (long)L.ws[L.tail_from] * L.hs[L.tail_from];
	ta.dpitch2 = L.ws[L.tail_from];
	hipLaunchKernelGGL(k_inv_tail, dim3(nplanes), dim3(TAIL_THREADS), 0, ctx->stream, ta);
	DWTX_LAUNCH_CHECK();
	cur = ta.dst;
	cur_ps = ta.dst_ps;
	cur_pitch = ta.dpitch2;
	return DWTX_OK;
}

// px != nullptr (`in` is then not read): the source is pixels, gray (plane p = image p) or RGB, interleaved or planar (plane p =
// channel p%3 of image p/3 after YCoCg-R), image i at px->image(i); needs a finest level the wide kernel takes
// (dwtx_pixels_ok).  Deep pixels: no histograms, no 16-bit bands (their bounds are for 8-bit sources).  Float pixels: the
// integers they quantise to (quant_of) by the same rule, dwtx_pixels::deep_source().
static int lift_fwd(dwtx_ctx *ctx, int32_t *out, const int32_t *in, const dwtx_pixels *px, int W, int H, int nplanes,
	const dwtx_hist_sink *sink = nullptr, unsigned *hist_levels = nullptr, dwtx_p16 p16 = dwtx_p16{ nullptr, 0u })
{
	if (px && ((px->deep_source() && (sink || p16.planes)) || (px->is_float() && !px->range_ok())))
		return DWTX_ERR_ARG;
	if (hist_levels)
		*hist_levels = 0u;
	if (!ctx || !out || (!in && !px) || W < 2 || H < 2 || nplanes < 1 || !dwtx_count_ok(nplanes, DWTX_MAX_PLANES_PER_CALL, "planes"))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	int forced;
	if (const int rc = forced_rows(ctx, &forced))
		return rc;
	LiftLayout L;
	if (const int rc = lift_layout(ctx, W, H, nplanes, L))
		return rc;
	const int T = L.T, tail_from = L.tail_from, *ws = L.ws, *hs = L.hs;
	const long full_ps = (long)W * H;
	// histograms ride along from the finest level down for as long as the levels allow it (the wide kernel, blocks
	// that the 16-lane rows cover exactly): pack.hip's k_hist counts the tiles of the levels below
	bool hist_on = sink != nullptr && hist_levels != nullptr;
	{
		dwtx_geom gg;
		if (hist_on && (dwtx_geometry(&gg, W, H) || gg.levels != T))
			hist_on = false;
	}
	// the LL band ping-pongs between the two scratch planes; the last level writes it into the pyramid itself
	const int *src = in;
	long src_ps = full_ps;
	int spitch = W;
	const WideRow *row = px ? wide_row(wide_end(*px)) : nullptr;
	if (px && (tail_from == 0 || !row))
		return DWTX_ERR_ARG;
	auto ll_dest =[&](int k, int *&p, long &ps, int &pitch) {   // destination of the ws[k]*hs[k] LL band
		if (k == T) {
			p = out;
			ps = full_ps;
			pitch = W;
			return;
		}
		p = src == L.level1 ? L.small : L.level1;   // never the plane being read; from level1 only bands <= ws[2]*hs[2] follow
		ps = (long)ws[k] * hs[k];
		pitch = ws[k];
	};
	for (int t = 0; t < T;) {
		if (t == tail_from) {
			TailArgs ta = tail_args(L, out);
			ta.src = src;
			ta.src_ps = src_ps;
			ta.spitch = spitch;
			hipLaunchKernelGGL(k_fwd_tail, dim3(nplanes), dim3(TAIL_THREADS), 0, ctx->stream, ta);
			DWTX_LAUNCH_CHECK();
			break;
		}
		// two levels in one pass where the shapes allow it (k_fwd2_level_w): plain int32 planes, no histograms
		if (!px && !p16.planes && !hist_on && !ctx->opt[DWTX_OPT_NO_FUSED_LEVELS] && t + 1 < tail_from && t + 2 <= T &&
			ws[t] % 4 == 0 && hs[t] % 4 == 0 && spitch % 4 == 0 && src_ps % 4 == 0 && aligned_to(src, 16) && W % 2 == 0 && aligned_to(out, 8)) {
			Level2Args f{};
			f.src = src;
			f.src_ps = src_ps;
			f.spitch = spitch;
			ll_dest(t + 2, f.ll2, f.ll2_ps, f.ll2pitch);
			f.det = out;
			f.det_ps = full_ps;
			f.dpitch = W;
			f.w = ws[t];
			f.h = hs[t];
			f.nquads = ws[t] / 4;
			const int strips = dwtx_cdiv(f.nquads, F2_OWN), h4 = hs[t] / 4;
			f.mpw = pick_mpw(strips, h4, nplanes, forced);
			hipLaunchKernelGGL(k_fwd2_level_w, dim3(dwtx_cdiv(strips, WAVES), dwtx_cdiv(h4, f.mpw), nplanes), dim3(64 * WAVES), 0, ctx->stream, f);
			DWTX_LAUNCH_CHECK();
			src = f.ll2;
			src_ps = f.ll2_ps;
			spitch = f.ll2pitch;
			t += 2;
			continue;
		}
		LevelArgs a{};
		a.w = ws[t];
		a.h = hs[t];
		a.w2 = ws[t + 1];
		a.h2 = hs[t + 1];
		const dwtx_pixels *pix_in = t == 0 ? px : nullptr;   // this step reads the pixels
		if (pix_in) {   // (deep pixels: uint16_t samples behind src8; src_ps and spitch count samples either way)
			pixel_block(*px, W, a.src8, a.src_ps, a.spitch, a.grid);
			if (px->is_float()) {
				a.maxval = px->maxval;   // (what the quantiser clamps at; no other forward source reads them)
				a.minval = px->minval;
			}
		} else {
			a.src = src;
			a.src_ps = src_ps;
			a.spitch = spitch;
		}
		ll_dest(t + 1, a.ll, a.ll_ps, a.llpitch);
		a.det = out;
		a.det_ps = full_ps;
		a.dpitch = W;
		// 16-bit bands (dwtx_p16): the levels in the mask write their details there; between two such levels the LL
		// band travels as 16-bit values too (in the scratch planes, which are sized for int32).  Only from 8-bit pixels:
		// that is what bounds the magnitudes (see fwd_level_body).
		auto in_mask = [&](int step) { return p16.planes && step < tail_from && ((p16.levels >> (T - 1 - step)) & 1u); };
		if (in_mask(t)) {
			if (!px || t >= LEVELS16_MAX || (t > 0 && !in_mask(t - 1)) || !aligned_to(p16.planes, 16))
				return DWTX_ERR_ARG;
			a.det16 = p16.planes;
			if (t > 0)
				a.src16 = reinterpret_cast<const short *>(src);
			if (in_mask(t + 1))
				a.ll16 = reinterpret_cast<short *>(a.ll);
		}
		const bool wide = wide_level(a.w, pix_in, { a.src, a.src_ps, a.spitch }, { a.ll, a.ll_ps, a.llpitch }, { a.det, a.det_ps, a.dpitch });
		if ((pix_in || a.det16) && !wide)
			return DWTX_ERR_ARG;   // callers check dwtx_pixels_ok() / dwtx_levels16() first
		const int level = T - 1 - t;   // the ring level this step's detail bands are
		// (the RGB kernel is bound by its own arithmetic — every plane's launch unpacks the pixels and does the colour
		// transform — and pays for the histogram in full: 3.2 -> 4.7 ms per 256 frames of 1080p against the 1.4 ms k_hist takes)
		const bool hist_here = hist_on && wide && a.w2 % 32 == 0 && sink->tiles.nbs[level] > 0;
		if (wide) {
			LevelArgsW A{};
			A.nquads = a.w / 4;
			const int strips = dwtx_cdiv(A.nquads, 64);
			a.rpw = pick_rpw(strips, a.h2, nplanes, forced);
			A.wx_log2 = strips >= 4 ? 2 : strips >= 2 ? 1 : 0;
			A.a = a;
			if (pix_in) {
				A.cstride = wide_cstride(*px);
				if (px->is_float())
					A.fmt = float_fmt(*px);
				delta_base(A, *px, W);
			}
			if (hist_here) {
				A.hist = HistArgs{ sink->cum32, sink->tile_mx, sink->tiles.xy2tile + sink->tiles.xy_first[level], sink->NT, sink->NTP,
					sink->tiles.nbs[level] };
				*hist_levels |= 1u << level;
			}
			const int sx = dwtx_cdiv(strips, 1 << A.wx_log2), gy = dwtx_cdiv(a.h2, (WAVES >> A.wx_log2) * a.rpw);
			// (8-bit RGB: the three channels of a strip side by side, xcd_strip_rgb; deep RGB: a block per plane, each taking its channel)
			const dim3 grid = pix_in && row->rgb_grid ? dim3(sx * 3, gy, nplanes / 3) : dim3(sx, gy, nplanes);
			A.ppw = pix_in ? px->channels : 1;
			const WideKernel kernel = pix_in ? row->fwd.k[hist_here][px->flips] : fwd_band_kernel(a.src16 != nullptr, hist_here);
			if (!kernel)
				return DWTX_ERR_ARG;
			hipLaunchKernelGGL(kernel, grid, dim3(64 * WAVES), 0, ctx->stream, A);
		} else {
			const int sx = dwtx_cdiv(a.w2, 64);
			a.rpw = pick_rpw(sx, a.h2, nplanes, forced);
			hipLaunchKernelGGL(k_fwd_level, dim3(sx, dwtx_cdiv(a.h2, WAVES * a.rpw), nplanes), dim3(64 * WAVES), 0, ctx->stream, a);
		}
		DWTX_LAUNCH_CHECK();
		src = a.ll;
		src_ps = a.ll_ps;
		spitch = a.llpitch;
		++t;
	}
	return DWTX_OK;
}

extern "C" int dwtx_transformation_fwd(dwtx_ctx *ctx, int32_t *out, const int32_t *in, int W, int H, int nplanes)
{
	if (!in)
		return DWTX_ERR_ARG;
	return lift_fwd(ctx, out, in, nullptr, W, H, nplanes);
}

// Can the finest level of a W*H image read / write these pixels directly?  (wide kernel, not the LDS tail)
// Which formats have wide kernels is what the table of pixel ends says (wide_row): a view without a row, like every view refused
// here, goes through the general conversions (dwtx_pixels_to_planes / dwtx_planes_to_pixels).  What the table does not say:
// - the shape: a width on the quad, and a side beyond the LDS tail's;
// - windows of a frame (dwtx_pixels: row pitch, bands): the kernels touch only the W * channels samples of a window's rows, so all
//   they ask is that every row of every window — of every plane of a planar window — starts on a quad (px.wide()) and that the
//   pitch fits their int;
// - a flipped call's windows (dwtx_pixels::flips) carry flags in their table entries that only win_off_flip takes apart: a SOURCE
//   qualifies when no window carries DWTX_FLIP_X (flip_wide: the FY instances of the wide forward kernels read it), a destination
//   (flip_sink: the FL instances of the wide inverse kernels write it) with any flags, a mirrored one if the windows' width is on the quad;
// - a delta view's base pictures: dense interleaved pixels like the view's own, which the delta rows' kernels address alike, and
//   both views must qualify as the plain views of their samples would.
bool dwtx_pixels_ok(const dwtx_pixels &px, int W, int H)
{
	if (px.chain || px.clips)   // (a chain's and a clip stack's base is the window before: no sink that walks the windows side by side takes it,
		return false;           // and a clip stack's source goes through the general conversion's clips instance, which knows the keys)
	if (!wide_row(wide_end(px)))
		return false;
	if (px.is_delta()) {
		dwtx_pixels own = px;
		own.delta = dwtx_base_grid();
		const dwtx_pixels bp = px.base_pixels();
		return !px.planar() && !bp.planar() && !bp.stepped() && dwtx_pixels_ok(own, W, H) && dwtx_pixels_ok(bp, W, H);
	}
	return (!px.flips || px.flip_wide || (px.flip_sink && (!px.flip_x || px.flip_w % 4 == 0))) && W % 4 == 0 && (W > TAIL_MAX || H > TAIL_MAX) && px.wide() &&
		px.pitch(W) <= 0x7fffffffu;
}

unsigned dwtx_levels16(int W, int H, unsigned sq_levels)
{
	LiftLayout L;
	lift_layout(nullptr, W, H, 0, L);
	unsigned mask = 0u;
	for (int t = 0; t < LEVELS16_MAX && t < L.tail_from; ++t) {
		const int l = L.T - 1 - t;   // ring level of step t
		if (!((sq_levels >> l) & 1u) || L.ws[t] % 4 != 0)
			break;
		mask |= 1u << l;
	}
	return mask;
}

int dwtx_lift_scratch(dwtx_ctx *ctx, int W, int H, int nplanes)
{
	LiftLayout L;
	return lift_layout(ctx, W, H, nplanes, L);
}

int dwtx_fwd_pixels(dwtx_ctx *ctx, int32_t *out, const dwtx_pixels &px, int W, int H, int n, const dwtx_hist_sink *sink, unsigned *hist_levels,
	dwtx_p16 p16)
{
	if (!px.base || (px.channels != 1 && px.channels != 3) || !dwtx_pixels_ok(px, W, H))
		return DWTX_ERR_ARG;
	return lift_fwd(ctx, out, nullptr, &px, W, H, n * px.channels, sink, hist_levels, p16);
}

int dwtx_transformation_fwd_hist(dwtx_ctx *ctx, int32_t *out, const int32_t *in, int W, int H, int nplanes, const dwtx_hist_sink *sink,
	unsigned *hist_levels)
{
	if (!in)
		return DWTX_ERR_ARG;
	return lift_fwd(ctx, out, in, nullptr, W, H, nplanes, sink, hist_levels);
}

// px != nullptr (`out` is then not written): the finest level writes clamped pixels (gray, or RGB — interleaved or planar — after the
// inverse colour transform), image i at px->image(i); deep pixels are clamped at px->maxval and take no 16-bit bands
static int lift_inv(dwtx_ctx *ctx, int32_t *out, const dwtx_pixels *px, const int32_t *in, int W, int H, int nplanes, const dwtx_p16 *p16 = nullptr)
{
	if (px && px->deep() && p16 && p16->planes)
		return DWTX_ERR_ARG;
	// (a flipped window holds its picture, mirrored quads and all: what keeps a mirrored index inside the window)
	if (px && px->flips && (!px->offs || W > px->flip_w || H > px->flip_h || (px->flip_x && px->flip_w % 4 != 0)))
		return DWTX_ERR_ARG;
	if (!ctx || (!out && !px) || !in || W < 2 || H < 2 || nplanes < 1 || !dwtx_count_ok(nplanes, DWTX_MAX_PLANES_PER_CALL, "planes"))
		return DWTX_ERR_ARG;
	DWTX_ENTER(ctx);
	int forced;
	if (const int rc = forced_rows(ctx, &forced))
		return rc;
	LiftLayout L;
	if (const int rc = lift_layout(ctx, W, H, nplanes, L))
		return rc;
	const int T = L.T, tail_from = L.tail_from, *ws = L.ws, *hs = L.hs;
	const long full_ps = (long)W * H;
	// Step t rebuilds plane t, ws[t] x hs[t], from plane t+1: plane T is the pyramid's root, plane 0 the output.  The planes in
	// between live in the two scratch planes, and a step never writes the plane it reads: plane k goes to level1 if k + fl is
	// odd, to small if it is even.  One step at a time alternates by itself; a two-level step (k_inv2_level_w) reads plane k+2
	// and writes plane k, same parity, so it flips `fl` for everything after it — allowed only if all later planes still fit.
	auto plane_of = [&](int k, int fl) { return (k + fl) & 1 ? L.level1 : L.small; };
	auto fits = [&](int k, int fl) { return ((k + fl) & 1) == 1 || k >= 2; };   // (small holds the planes from 2 on)
	// two levels per pass (k_inv2_level_w): int32 planes throughout, or — the codec's pipelines — both levels' detail bands as 16-bit values
	// (dwtx_p16), the finest step then writing a gray picture's 8-bit pixels itself; an RGB picture's last step keeps its own kernel
	const bool have16 = p16 && p16->planes;
	const bool fusing = !ctx->opt[DWTX_OPT_NO_FUSED_LEVELS] && W % 4 == 0 && aligned_to(in, 8) && (px ? px->wide() : aligned_to(out, 16)) &&
		(!have16 || aligned_to(p16->planes, 4));
	auto in16 = [&](int t) { return have16 && ((p16->levels >> (T - 1 - t)) & 1u) != 0; };   // step t's detail bands are 16-bit values
	auto can_fuse = [&](int t) {   // (t == T - 1 reads the root LL in the pyramid itself: no pair there)
		if (!fusing || t < 1 || t == T - 1 || ws[t - 1] % 4 != 0 || hs[t - 1] % 4 != 0 || in16(t) != in16(t - 1))
			return false;
		if (t - 1 == 0 && px)   // (the 8-bit variants exist for 16-bit bands only: what the pipelines run; RGB: three planes per wave; no float ones)
			return !px->is_float() && in16(0) && (px->channels == 1 || (px->channels == 3 && nplanes % 3 == 0));
		return true;
	};
	// Steps t .. 0 with the planes from here on assigned with `fl`: the most samples that can go through two-level steps (a pair is
	// worth the plane it writes: fusing the two finest levels saves sixteen times what the pair below them saves), -1 if the planes
	// do not fit, and whether step t starts a pair on that path (a pair wins ties).  At most 2^16 paths, a handful in practice.
	struct Best {
		long samples;
		bool pair;
	};
	auto best = [&](auto &&self, int t, int fl) -> Best {
		if (t < 0)
			return { 0, false };
		Best b = { -1, false };
		if (can_fuse(t) && (t - 1 == 0 || fits(t - 1, fl ^ 1))) {
			const long r = self(self, t - 2, fl ^ 1).samples;
			if (r >= 0)
				b = { r + (long)ws[t - 1] * hs[t - 1], true };
		}
		if (t == 0 || fits(t, fl)) {
			const long r = self(self, t - 1, fl).samples;
			if (r > b.samples)
				b = { r, false };
		}
		return b;
	};
	// The plan, made before the first launch: pair[t], steps t and t-1 run as one two-level launch, and plane[k], the scratch plane
	// that plane k goes to
	bool pair[DWTX_MAX_LEVELS + 1] = {};
	int *plane[DWTX_MAX_LEVELS + 2] = {};
	if (tail_from > 0 && tail_from < T)
		plane[tail_from] = plane_of(tail_from, 0);
	for (int t = tail_from - 1, fl = 0; t >= 0; --t) {
		if (can_fuse(t) && best(best, t, fl).pair) {   // (no search where no pair can start)
			pair[t] = true;
			fl ^= 1;
			--t;
		} else if (t > 0 && (!fits(t, fl) || plane_of(t, fl) == plane[t + 1])) {
			dwtx_set_error("inverse transform: no scratch plane for step %d", t);
			return DWTX_ERR_ARG;
		}
		if (t > 0)
			plane[t] = plane_of(t, fl);
	}
	// the LL band the next launch reads: the pyramid's root, then the output of the launch before
	const int *cur = in;
	long cur_ps = full_ps;
	int cur_pitch = W;
	const WideRow *row = px ? wide_row(wide_end(*px)) : nullptr;
	const int flip = flip_level(px);
	if (px && !row)
		return DWTX_ERR_ARG;
	if (tail_from < T) {
		if (tail_from == 0 && px)
			return DWTX_ERR_ARG;
		if (const int rc = inv_tail(ctx, L, const_cast<int *>(in), nplanes, tail_from == 0 ? out : plane[tail_from], cur, cur_ps, cur_pitch))
			return rc;
	}
	for (int t = tail_from - 1; t >= 0; --t) {
		if (pair[t]) {   // steps t and t-1: shapes whose two levels have whole row pairs
			Inv2Args f{};
			f.ll2 = cur;           // the LL band step t reads: ws[t+1] x hs[t+1]
			f.ll2_ps = cur_ps;
			f.ll2pitch = cur_pitch;
			f.det = in;
			f.det_ps = full_ps;
			f.dpitch = W;
			f.det16 = in16(t) ? p16->planes : nullptr;
			const dwtx_pixels *pix_out = t - 1 == 0 ? px : nullptr;   // the pair writes the pixels
			if (pix_out) {
				pixel_block(*px, W, f.dst8, f.dst_ps, f.opitch, f.grid);
				f.cstride = wide_cstride(*px);
				f.fh = px->flip_h;
				f.fwq = px->flip_w / 4;
			} else if (t - 1 == 0) {
				f.dst = out;
				f.dst_ps = full_ps;
				f.opitch = W;
			} else {
				f.dst = plane[t - 1];
				f.dst_ps = (long)ws[t - 1] * hs[t - 1];
				f.opitch = ws[t - 1];
			}
			f.w = ws[t - 1];
			f.h = hs[t - 1];
			f.nquads = f.w / 4;
			const int strips = dwtx_cdiv(f.nquads, V2_OWN), h4 = f.h / 4;
			f.mpw = pick_mpw(strips, h4, nplanes, forced);
			// (the 8-bit kernels put a block's waves side by side; RGB: three planes per wave)
			const dim3 grid = pix_out ? dim3(dwtx_cdiv(strips, WAVES), dwtx_cdiv(h4, f.mpw), nplanes / px->channels)
			                          : dim3(strips, dwtx_cdiv(h4, WAVES * f.mpw), nplanes);
			const Inv2Kernel kernel = pix_out ? row->inv.k2[flip] : inv2_band_kernel(f.det16 != nullptr);
			if (!kernel)
				return DWTX_ERR_ARG;
			hipLaunchKernelGGL(kernel, grid, dim3(64 * WAVES), 0, ctx->stream, f);
			DWTX_LAUNCH_CHECK();
			cur = f.dst;
			cur_ps = f.dst_ps;
			cur_pitch = f.opitch;
			--t;   // (the loop's own step takes the second)
			continue;
		}
		LevelArgs a{};
		a.w = ws[t];
		a.h = hs[t];
		a.w2 = ws[t + 1];
		a.h2 = hs[t + 1];
		a.src = cur;   // (without a tail the first step reads the root LL in the pyramid itself)
		a.src_ps = cur_ps;
		a.spitch = cur_pitch;
		const dwtx_pixels *pix_out = t == 0 ? px : nullptr;   // this step writes the pixels
		if (pix_out) {   // (deep pixels: uint16_t samples behind dst8; ll_ps and llpitch count samples either way)
			pixel_block(*px, W, a.dst8, a.ll_ps, a.llpitch, a.grid);
			a.maxval =px->deep() || px->is_float() ? px->maxval : 0;   // (float sinks clamp at whatever the maxval is, 255 included)
			a.minval = px->minval;   // (0 but for int16_t samples and the float views of the signed calls)
		} else if (t == 0) {
			a.ll = out;
			a.ll_ps = full_ps;
			a.llpitch = W;
		} else {
			a.ll = plane[t];
			a.ll_ps = (long)a.w * a.h;
			a.llpitch = a.w;
		}
		a.det = const_cast<int *>(in);
		a.det_ps = full_ps;
		a.dpitch = W;
		if (in16(t)) {
			if (!px || !aligned_to(p16->planes, 4))
				return DWTX_ERR_ARG;
			a.det16 = p16->planes;
		}
		const bool wide = wide_level(a.w, pix_out, { a.ll, a.ll_ps, a.llpitch }, { a.src, a.src_ps, a.spitch }, { a.det, a.det_ps, a.dpitch });
		if ((pix_out || a.det16) && !wide)
			return DWTX_ERR_ARG;
		if (wide) {
			LevelArgsW A{};
			A.nquads = a.w / 4;
			const bool rgb = pix_out && row->rgb();
			const int sx = dwtx_cdiv(A.nquads, rgb ? INV_QUADS : 64);   // (the RGB kernel's waves overlap by a lane on each side)
			a.rpw = pick_rpw(sx, a.h2, nplanes, forced);
			A.a = a;
			if (pix_out) {
				A.cstride = wide_cstride(*px);
				A.fmt = float_fmt(*px);
				A.fh = px->flip_h;
				A.fwq = px->flip_w / 4;
				delta_base(A, *px, W);
			}
			const dim3 grid(sx, dwtx_cdiv(a.h2, WAVES * a.rpw), rgb ? nplanes / 3 : nplanes);
			const WideKernel kernel = pix_out ? row->inv.k[a.det16 != nullptr][flip] : inv_band_kernel(a.det16 != nullptr);
			if (!kernel)
				return DWTX_ERR_ARG;
			hipLaunchKernelGGL(kernel, grid, dim3(64 * WAVES), 0, ctx->stream, A);
		} else {
			const int sx = dwtx_cdiv(a.w2, INV_PAIRS);
			a.rpw = pick_rpw(sx, a.h2, nplanes, forced);
			hipLaunchKernelGGL(k_inv_level, dim3(sx, dwtx_cdiv(a.h2, WAVES * a.rpw), nplanes), dim3(64 * WAVES), 0, ctx->stream, a);
		}
		DWTX_LAUNCH_CHECK();
		cur = a.ll;   // (null after the last step, which may have written 8-bit pixels: nothing reads it)
		cur_ps = a.ll_ps;
		cur_pitch = a.llpitch;
	}
	return DWTX_OK;
}

extern "C" int dwtx_transformation_inv(dwtx_ctx *ctx, int32_t *out, const int32_t *in, int W, int H, int nplanes)
{
	if (!out)
		return DWTX_ERR_ARG;
	return lift_inv(ctx, out, nullptr, in, W, H, nplanes);
}

int dwtx_inv_pixels(dwtx_ctx *ctx, const dwtx_pixels &px, const int32_t *in, int W, int H, int n, const dwtx_p16 *p16)
{
	if (!px.base || W < 2 || H < 2 || (px.channels != 1 && px.channels != 3) || !px.range_ok() || !dwtx_pixels_ok(px, W, H))
		return DWTX_ERR_ARG;
	return lift_inv(ctx, nullptr, &px, in, W, H, n * px.channels, p16);
}

// ------------------------------------------------------------- crop decode ---
// The inverse transform of a window (dwtx_decode_view_crop): every plane t of the transform is held
// as a compact rectangle instead of whole, and k_inv_level_roi — k_inv_level for the pair range of a rectangle — rebuilds
// the rectangle of plane t from the rectangle of plane t + 1 and the detail bands, which it reads from the int32 pyramid at
// their absolute Mallat positions.
//
// Margins (cdf53.h:36-61, icdf53): sample 2k of a line is s[k] - (d[k-1] + d[k]) / 4 (cdf53.h:40-46; d[-1] := d[0], and the
// last even sample of an odd line is s[k] itself), sample 2k+1 is d[k] + (x[2k] + x[2k+2]) / 2 (cdf53.h:47-53; x[N] := x[N-2]).
// Outputs [xa, xb) are the pairs k0 = xa / 2 .. k1 - 1 with k1 = ceil(xb / 2); their even samples need d[k0-1 .. k1-1], and the
// last odd one, 2 k1 - 1, needs x[2 k1], that is s[k1], d[k1-1] and d[k1].  Columns are undone first, rows last
// (decode.c:21-29), so s and d of the row pass are themselves outputs of the column pass: the row pass needs columns
// k0-1 .. k1 of its inputs, the column pass rows j0-1 .. j1 of LL and of the three detail bands — one pair more on every
// side, clipped to the band.  (The s[k0-1] this keeps is never read; a rectangle is simpler than two.)
//
// All pictures of a launch share the rectangles' sizes, so that one grid serves them: the size that fits both parities of
// an origin, s / 2 + 3 for a finer side of s (s / 2 + 1 pairs at the most, and the margins), or the whole band where that is
// smaller.  A picture's rectangle starts at k0 - 1, shifted back inside the band where it would cross an edge: it then holds
// more than its pictures' margins ask for, never less.  Planes from the LDS tail on are whole bands.
namespace {

struct RoiArgs {
	const int *src;  long src_ps;  int spitch;  int sw, sh;   // LL rectangles of plane t + 1: sw x sh each, compact
	int *dst;        long dst_ps;  int opitch;  int dw, dh;   // output rectangles of plane t: dw x dh each, compact
	const int *det;  long det_ps;  int dpitch;                // Mallat pyramid, absolute positions
	int w, h, w2, h2;                                         // the whole planes t and t + 1
	int rpw;
	int C;                                                    // planes per picture
	const int2 *src_org, *dst_org;                            // [picture]: where its rectangles start in their planes; null: (sx, sy) / (dx, dy) for all
	int sx, sy, dx, dy;
};

struct RoiLane {
	int k;
	bool valid, has_odd, right_in, frozen, writes;   // InvLane's, from the absolute pair index and the whole line's length
};

// inv_row for a rectangle's row: `row` is where column dx of the plane lies; only samples dx .. dx + dw - 1 are written
__device__ __forceinline__ void inv_row_roi(int *__restrict__ row, const RoiLane &L, int dx, int dw, int lo, int hi)
{
	int hl = __shfl_up(hi, 1);
	if (L.k <= 0)
		hl = hi;
	const int e = L.frozen ? lo : lo - tdiv4(hl + hi);
	int er = __shfl_down(e, 1);
	if (!L.right_in)
		er = e;
	const int o = hi + tdiv2(e + er);
	const int x = 2 * L.k - dx;
	if (L.writes) {
		if (x >= 0 && x < dw)
			row[x] = e;
		if (L.has_odd && x + 1 >= 0 && x + 1 < dw)
			row[x + 1] = o;
	}
}

// grid (strips of 62 pairs over the widest pair range, strips of rpw row pairs, plane).  The picture's origins are the same
// for the whole workgroup: they come from blockIdx alone, so the table is read with scalar loads and every range below
// (kA, kB, jA, jB, the strip's rows) is scalar arithmetic; readfirstlane only says so once more.
__global__ __launch_bounds__(64 * WAVES) void k_inv_level_roi(RoiArgs a)
{
	const int lane = threadIdx.x & 63;
	const int wv = wave_in_block();
	const int plane = blockIdx.z;
	int sx = a.sx, sy = a.sy, dx = a.dx, dy = a.dy;
	if (a.dst_org) {
		const int img = a.C == 3 ? plane / 3 : plane;
		const int2 d = a.dst_org[img];
		dx = __builtin_amdgcn_readfirstlane(d.x);
		dy = __builtin_amdgcn_readfirstlane(d.y);
		if (a.src_org) {
			const int2 s = a.src_org[img];
			sx = __builtin_amdgcn_readfirstlane(s.x);
			sy = __builtin_amdgcn_readfirstlane(s.y);
		}
	}
	// the pairs and row pairs that hold the rectangle's samples
	const int kA = dx >> 1, kB = (dx + a.dw + 1) >> 1;
	const int jA = dy >> 1, jB = (dy + a.dh + 1) >> 1;
	const int kb = kA + blockIdx.x * INV_PAIRS;
	const int j0 = jA + (blockIdx.y * WAVES + wv) * a.rpw;
	if (kb >= kB || j0 >= jB)
		return;
	if (dx < 0 || dy < 0 || dx + a.dw > a.w || dy + a.dh > a.h)   // (no rectangle of the plane: the host never makes one)
		return;
	const int j1 = min(j0 + a.rpw, jB);
	RoiLane L;
	L.k = kb - 1 + lane;
	const bool mine = L.k >= 0 && L.k <= kB;   // (pair kB is the halo of the rectangle's last odd sample: nothing beyond it is read)
	L.valid = mine && 2 * L.k < a.w;
	L.has_odd = mine && 2 * L.k + 1 < a.w;
	L.right_in = 2 * L.k + 2 < a.w;
	L.frozen = (a.w & 1) && 2 * L.k == a.w - 1;
	L.writes = L.valid && lane >= 1 && lane <= INV_PAIRS;

	const int *llp = a.src + plane * a.src_ps;
	const int *det = a.det + plane * a.det_ps;
	int *dst = a.dst + plane * a.dst_ps;
	const int kk = L.k < 0 ? 0 : L.k;
	// the LL rectangle holds every (j, k) the margins ask for; the test keeps a lane inside it whatever the table says
	const int lx = kk - sx;
	const bool ll_col = L.valid && lx >= 0 && lx < a.sw;
	const bool h_odd = a.h & 1;

	auto details = [&](int j, int &fsh, int &fdl, int &fdh) {
		fsh = L.has_odd ? det[(long)j * a.dpitch + a.w2 + kk] : 0;
		const bool d_in = 2 * j + 1 < a.h;
		fdl = (d_in && L.valid) ? det[(long)(a.h2 + j) * a.dpitch + kk] : 0;
		fdh = (d_in && L.has_odd) ? det[(long)(a.h2 + j) * a.dpitch + a.w2 + kk] : 0;
	};
	auto fetch = [&](int j, int &fsl, int &fsh, int &fdl, int &fdh) {
		const int ly = j - sy;
		fsl = (ll_col && ly >= 0 && ly < a.sh) ? llp[(long)ly * a.spitch + lx] : 0;
		details(j, fsh, fdl, fdh);
	};
	auto even_of = [&](int j, int s, int dprev, int dcur) {
		if (h_odd && 2 * j == a.h - 1)
			return s;
		return s - tdiv4((j ? dprev : dcur) + dcur);
	};

	int sl, sh, dl = 0, dh = 0, pdl = 0, pdh = 0;
	if (j0 > 0) {
		int t1;
		details(j0 - 1, t1, pdl, pdh);
	}
	fetch(j0, sl, sh, dl, dh);
	int el = even_of(j0, sl, pdl, dl);
	int eh = even_of(j0, sh, pdh, dh);
	for (int jj = j0; jj < j1; ++jj) {
		const int r0 = 2 * jj, r1 = r0 + 1;
		int nsl = 0, nsh = 0, ndl = 0, ndh = 0;
		int nel = el, neh = eh;          // mirror: x[h] := x[h-2]
		if (r1 + 1 < a.h) {
			fetch(jj + 1, nsl, nsh, ndl, ndh);
			nel = even_of(jj + 1, nsl, dl, ndl);
			neh = even_of(jj + 1, nsh, dh, ndh);
		}
		if (r0 >= dy && r0 < dy + a.dh)
			inv_row_roi(dst + (long)(r0 - dy) * a.opitch, L, dx, a.dw, el, eh);
		if (r1 < a.h && r1 >= dy && r1 < dy + a.dh) {
			const int ol = dl + tdiv2(el + nel);
			const int oh = dh + tdiv2(eh + neh);
			inv_row_roi(dst + (long)(r1 - dy) * a.opitch, L, dx, a.dw, ol, oh);
		}
		dl = ndl;
		dh = ndh;
		el = nel;
		eh = neh;
	}
}

// compact cw x ch planes out of whole w x h planes: grid (64 columns, 4 rows, plane), a wave per row as the conversions have it
__global__ __launch_bounds__(PX_LANES * PX_ROWS) void k_crop_planes(int *__restrict__ dst, const int *__restrict__ src, int w, int h, int cw, int ch, int C,
	const int2 *__restrict__ org, int x0, int y0)
{
	const int plane = blockIdx.z;
	if (org) {
		const int2 o = org[C == 3 ? plane / 3 : plane];
		x0 = __builtin_amdgcn_readfirstlane(o.x);
		y0 = __builtin_amdgcn_readfirstlane(o.y);
	}
	int x, y;
	if (!px_lane(cw, ch, x, y) || x0 + x >= w || y0 + y >= h)
		return;
	dst[(long)plane * cw * ch + (long)y * cw + x] = src[(long)plane * w * h + (long)(y0 + y) * w + x0 + x];
}

} // namespace

int dwtx_crop_steps_of(int W, int H, int cw, int ch, dwtx_crop_steps *S)
{
	if (!S || cw < 1 || ch < 1 || cw > W || ch > H)
		return DWTX_ERR_ARG;
	LiftLayout L;
	lift_layout(nullptr, W, H, 0, L);
	S->T = L.T;
	S->tail_from = L.tail_from;
	for (int t = 0; t <= L.T; ++t) {
		S->ws[t] = L.ws[t];
		S->hs[t] = L.hs[t];
		const bool whole = t >= L.tail_from;
		S->w[t] = t == 0 ? cw : whole ? L.ws[t] : min(L.ws[t], S->w[t - 1] / 2 + 3);
		S->h[t] = t == 0 ? ch : whole ? L.hs[t] : min(L.hs[t], S->h[t - 1] / 2 + 3);
	}
	return DWTX_OK;
}

void dwtx_crop_origins(const dwtx_crop_steps &S, int x0, int y0, int *xs, int *ys)
{
	xs[0] = x0;
	ys[0] = y0;
	for (int t = 1; t <= S.T; ++t) {
		xs[t] = max(0, min((xs[t - 1] >> 1) - 1, S.ws[t] - S.w[t]));
		ys[t] = max(0, min((ys[t - 1] >> 1) - 1, S.hs[t] - S.h[t]));
	}
}

int dwtx_inv_crop(dwtx_ctx *ctx, int32_t *planes, int32_t *pyr, int W, int H, int n, int C, int cw, int ch,
	const int *dev_org, long org_stride, int x0, int y0, int route, const int32_t **result)
{
	if (!ctx || !planes || !pyr || !result || n < 1 || (C != 1 && C != 3) || W < 2 || H < 2 || x0 < 0 || y0 < 0 ||
		!dwtx_count_ok((long)n * C, DWTX_MAX_PLANES_PER_CALL, "planes"))
		return DWTX_ERR_ARG;
	if (!dev_org && (x0 + cw > W || y0 + ch > H))
		return DWTX_ERR_ARG;
	dwtx_crop_steps S;
	if (const int rc = dwtx_crop_steps_of(W, H, cw, ch, &S))
		return rc;
	DWTX_ENTER(ctx);
	const int nplanes = n * C;
	const int2 *org = reinterpret_cast<const int2 *>(dev_org);
	if (route == 2 || S.tail_from == 0) {   // the whole inverse, then the gather (a transform that is all tail has no windowed level)
		if (const int rc = lift_inv(ctx, planes, nullptr, pyr, W, H, nplanes))
			return rc;
		const dim3 grid((unsigned)dwtx_cdiv(cw, PX_LANES), (unsigned)dwtx_cdiv(ch, PX_ROWS), (unsigned)nplanes);
		hipLaunchKernelGGL(k_crop_planes, grid, dim3(PX_LANES * PX_ROWS), 0, ctx->stream, pyr, planes, W, H, cw, ch, C, org, x0, y0);
		DWTX_LAUNCH_CHECK();
		*result = pyr;
		return DWTX_OK;
	}
	int forced;
	if (const int rc = forced_rows(ctx, &forced))
		return rc;
	LiftLayout L;
	if (const int rc = lift_layout(ctx, W, H, nplanes, L))
		return rc;
	const int T = L.T, tail_from = L.tail_from;
	const long full_ps = (long)W * H;
	// the rectangles of plane k: level1 for odd k, small for even k (k >= 2), as lift_inv's one-level steps have it — a
	// rectangle is never larger than its plane
	auto plane_of = [&](int k) { return k & 1 ? L.level1 : L.small; };
	int xs[DWTX_MAX_LEVELS + 2], ys[DWTX_MAX_LEVELS + 2];
	dwtx_crop_origins(S, x0, y0, xs, ys);
	const int *cur = pyr;   // (without a tail the first step reads the root LL in the pyramid itself)
	long cur_ps = full_ps;
	int cur_pitch = W;
	if (tail_from < T)
		if (const int rc = inv_tail(ctx, L, pyr, nplanes, plane_of(tail_from), cur, cur_ps, cur_pitch))
			return rc;
	for (int t = tail_from - 1; t >= 0; --t) {
		RoiArgs a{};
		a.src = cur;
		a.src_ps = cur_ps;
		a.spitch = cur_pitch;
		a.sw = S.w[t + 1];
		a.sh = S.h[t + 1];
		a.dst = t == 0 ? planes : plane_of(t);
		a.dst_ps = (long)S.w[t] * S.h[t];
		a.opitch = S.w[t];
		a.dw = S.w[t];
		a.dh = S.h[t];
		a.det = pyr;
		a.det_ps = full_ps;
		a.dpitch = W;
		a.w = L.ws[t];
		a.h = L.hs[t];
		a.w2 = L.ws[t + 1];
		a.h2 = L.hs[t + 1];
		a.C = C;
		a.dst_org = org ? org + (long)t * org_stride : nullptr;
		a.src_org = org ? org + (long)(t + 1) * org_stride : nullptr;
		a.sx = xs[t + 1];
		a.sy = ys[t + 1];
		a.dx = xs[t];
		a.dy = ys[t];
		const int pairs_x = a.dw / 2 + 1, pairs_y = a.dh / 2 + 1;   // the most a rectangle's samples lie in, whatever its origin's parity
		const int sx = dwtx_cdiv(pairs_x, INV_PAIRS);
		a.rpw = pick_rpw(sx, pairs_y, nplanes, forced);
		hipLaunchKernelGGL(k_inv_level_roi, dim3(sx, dwtx_cdiv(pairs_y, WAVES * a.rpw), nplanes), dim3(64 * WAVES), 0, ctx->stream, a);
		DWTX_LAUNCH_CHECK();
		cur = a.dst;
		cur_ps = a.dst_ps;
		cur_pitch = a.opitch;
	}
	*result = planes;
	return DWTX_OK;
}
