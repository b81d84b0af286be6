// dvp_weak_wave.hpp — the weak-pixel update (CheckerboardPropagationWeak +
// PlaneHypothesisRefinementWeak, APD.cu:2739-3089, 1897-2008) with ONE WAVEFRONT PER WEAK PIXEL.
//
// Why not one lane per pixel (round 1): the deformable NCC of a WEAK pixel (ComputeBilateralNCCNew,
// APD.cu:835-1021) gathers, per (plane, view), 36 centre taps + up to 11 anchors x 9 taps around
// STRONG points that every pixel draws at random.  With a pixel per lane the 64 gathers of one load
// instruction land on 64 unrelated cache lines, nothing is reused before it is evicted, and PMC showed
// the kernel at the HBM roofline moving 64 B per 16-B footprint (6.7 G L2 misses per launch at
// 6208x4128, L2 hit rate 20 %).  Here the 64 lanes of a wave own the (plane, tap) pairs of one pixel:
// the <= 8 planes of a phase project a tap to neighbouring texels, so one load instruction touches a
// few lines instead of 64 and the lines are shared inside the instruction; the per-pixel state
// (cost vectors, weights, tables) lives in LDS instead of 4 KB of scratch per lane.
//
// Code shape.  A wave runs the function below in lock step, in the lane sections of dvp_wave.hpp (DVP_LANES, DVP_LANE0,
// wave_sync): per-lane shares inside a section, per-pixel ("uniform") code outside.  All floating-point
// expressions, their order and their operands are those of the per-pixel formulation (the oracle's),
// only the assignment of independent work items to lanes is new.
#ifndef DVP_WEAK_WAVE_HPP_
#define DVP_WEAK_WAVE_HPP_

#include "dvp_strong.hpp"
#include "dvp_wave.hpp"

namespace dvp {

constexpr int kAnchors = DVP_NEIGHBOUR_NUM - 1;   // 11
constexpr int kAnchorTaps = kAnchors * 9;         // 99
#ifndef DVP_WEAK_PAIRS
#define DVP_WEAK_PAIRS 40
#endif
// (source view, plane) pairs per shared-memory hand-over of the weak update: a batch takes as many views as fit,
// 5 with the 8 candidate planes, 20 / 8 with the 2 and 5 planes of the refinement phases (8.6 KB of LDS per wave:
// four workgroups per CU)
constexpr int kWeakPairs = DVP_WEAK_PAIRS;
constexpr int kWeakViews = 7;   // ... and at most this many views (size of the (view, anchor) prefetch table)

// per-wave shared state (LDS on the device).  TAB = 1 (the anchor reference sides come from the pass' table): no offset
// table, and the homographies of the batch's (view, plane) pairs instead — in the bytes of cost_array, which is dead
// while a batch is evaluated (written by the epilogue of the propagation phase, read by the view selection).
template <int TAB>
struct WeakSharedT {
	f2 ctab[kTaps * kTaps];        // centre patch: (w, w*ref) per tap, row-major
	float caa[kTaps * kTaps];      // w*ref*ref per tap (reference moments only)
	float rows[kWeakPairs][kTaps][3];    // centre-patch row sums (s_s, s_ss, s_rs) per pair (view slot * np + plane) and row; the final-cost section uses pairs 0..7 for 8 views
	float acost[kWeakPairs][kAnchors];   // anchor cost per (pair, anchor), < 0: does not count
	int inq[kWeakPairs];                 // pair: the centre projects inside the source image
	// (view slot, anchor) of the batch, fetched once before the items run: the anchor's 8 visibility-prior offsets
	// for that view as signed bytes (x, y) and what anchor_cost has to do with the pair
	uint32_t aoff[TAB ? 1 : kWeakViews * kAnchors][4];
	uint8_t astate[kWeakViews * kAnchors];   // 0: no anchor; 1: the anchor did not select the view; 2: sub-patch
	union {
		float cost_array[8][32];
		float Hq[TAB ? kWeakPairs : 1][9];   // homography of the batch's pair (view slot * np + live-plane index)
	};
	float ev[8][32];
	float gtab[8][32];             // geometric-consistency cost per (plane, view)
	float probs[32];
	float priors[32];
	float fcost[8];
	int positions[8];
	uint8_t vw[32];
	f4 pl[8];
};
using WeakShared = WeakSharedT<0>;

// build_patch_ctx (dvp_ncc.hpp) by the wave: lane t < 36 owns tap t; the reference moments are then
// summed in the row-then-total order by every lane.
template <int FMT, class SH>
DVP_HD void wave_patch_ctx(const Dev& d, int px, int py, int radius, int inc, int colour_only, SH& sh, PatchCtx* c) {
	c->radius = radius;
	c->inc = inc;
	c->fast = (inc > 0 && (2 * radius) / inc + 1 == kTaps) ? 1 : 0;
	c->sum_ref = c->sum_ref_ref = c->wsum = 0.0f;
	if (!c->fast) return;
	const int W = d.width, H = d.height, P = d.pitch;
	const float cpix = ref_texel_t<FMT>(d, px, py);
	DVP_LANES(t) {
		if (t >= kTaps * kTaps) continue;
		const int ty = t / kTaps, tx = t - ty * kTaps;
		const int i = -radius + tx * inc, j = -radius + ty * inc;
		const float a = ref_texel_t<FMT>(d, px + i, py + j);
		const float w = bilateral_weight((float)i, (float)j, a, cpix, d.params.sigma_spatial, d.params.sigma_color, colour_only);
		const float wa = w * a;
		sh.ctab[t] = mk2(w, wa);
		sh.caa[t] = wa * a;
	}
	wave_sync();
	float sr = 0.0f, srr = 0.0f, ws = 0.0f;
	for (int ty = 0; ty < kTaps; ++ty) {
		float sr_row = 0.0f, srr_row = 0.0f, ws_row = 0.0f;
		for (int tx = 0; tx < kTaps; ++tx) {
			const f2 t = sh.ctab[ty * kTaps + tx];
			sr_row += t.y;
			srr_row += sh.caa[ty * kTaps + tx];
			ws_row += t.x;
		}
		sr += sr_row;
		srr += srr_row;
		ws += ws_row;
	}
	c->sum_ref = sr;
	c->sum_ref_ref = srr;
	c->wsum = ws;
}

// one row (6 taps) of the 36-tap patch for homography H: the row's three source-side sums
// (ncc_patch_fast, dvp_ncc.hpp: same products, same shared division per row, same order)
template <int SMP, int FMT, class SH>
DVP_HD void patch_row_sums(const Dev& d, const SH& sh, const float* H, const void* src, int px, int py, int radius, int inc, int row, float* out /*[3]*/) {
	const int W = d.width, Hh = d.height, P = d.pitch;
	const float fy = (float)(py - radius + row * inc);
	const float hy1 = H[1] * fy, hy4 = H[4] * fy, hy7 = H[7] * fy;
	float X[kTaps], Y[kTaps], Z[kTaps], IZ[kTaps];
#pragma unroll
	for (int tx = 0; tx < kTaps; ++tx) {
		const float fx = (float)(px - radius + tx * inc);
		X[tx] = H[0] * fx + hy1 + H[2];
		Y[tx] = H[3] * fx + hy4 + H[5];
		Z[tx] = H[6] * fx + hy7 + H[8];
	}
	batch_rcp(Z, kTaps, IZ);
	unsigned off[kTaps];
	TapW<SMP> tw[kTaps];
	float q[kTaps][4];
#pragma unroll
	for (int tx = 0; tx < kTaps; ++tx) tex_coord_t<FMT>(d, X[tx] * IZ[tx], Y[tx] * IZ[tx], &off[tx], &tw[tx]);
#pragma unroll
	for (int tx = 0; tx < kTaps; ++tx) load_quad_t<FMT>(src, off[tx], &q[tx][0], &q[tx][1], &q[tx][2], &q[tx][3]);
	float r_s = 0.0f, r_ss = 0.0f, r_rs = 0.0f;
#pragma unroll
	for (int tx = 0; tx < kTaps; ++tx) {
		float fa, fb;
		tap_weights(tw[tx], &fa, &fb);
		const float b = tex_lerp(fa, fb, q[tx][0], q[tx][1], q[tx][2], q[tx][3]);
		const f2 t = sh.ctab[row * kTaps + tx];
		const float wsb = t.x * b;
		r_s += wsb;
		r_ss = fmaf(wsb, b, r_ss);
		r_rs = fmaf(t.y, b, r_rs);
	}
	out[0] = r_s;
	out[1] = r_ss;
	out[2] = r_rs;
}

// index of the n-th set bit of m (n < popcount(m))
DVP_HD int nth_set_bit(uint32_t m, int n) {
	for (int i = 0; i < n; ++i) m &= m - 1;
	return __builtin_ctz(m);
}

// One anchor sub-patch of ComputeBilateralNCCNew (APD.cu:905-1000): the anchor `nb` of the pixel against source
// view v (1-based) under homography H.  < 0: the anchor does not count.  The anchor's 9 reference taps (the 8
// visibility-prior offsets of (anchor, view) + the anchor itself: offsets, texels, weights, sums) and the 9 gathers
// in the source image all stay in registers.
template <int SMP, int FMT>
DVP_HD float anchor_cost(const Dev& d, const float* H, const void* src, s2 nb, int state, const uint32_t* offs, float cpix) {
	const int W = d.width, Hh = d.height, Pt = d.pitch;
	if (state == 0) return -1.0f;
	const bool visible = state == 2;
	const f2 nsp = apply_homography(H, nb.x, nb.y);
	const bool outside = nsp.x < 0 || nsp.y < 0 || nsp.x >= W || nsp.y >= Hh;
	if (outside) return visible ? 2.0f : -1.0f;
	if (!visible) return 2.0f;   // anchor not visible in this view: the reference's 0/0 path yields exactly 2
	int tx[9], ty[9];
	float ti[9], tj[9];
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		int i = 0, j = 0;
		if (t < 8) {
			const uint32_t o = offs[t >> 1] >> (16 * (t & 1));
			i = (int)(int8_t)(o & 255u);
			j = (int)(int8_t)((o >> 8) & 255u);
			if (i == 0 && j == 0) {   // default +-5 ring (APD.cu:943-952): {-5,0,5}^2 without its centre, x-major
				const int u = t + (t >= 4 ? 1 : 0);
				i = (u / 3 - 1) * 5;
				j = (u % 3 - 1) * 5;
			}
		}
		tx[t] = nb.x + i;
		ty[t] = nb.y + j;
		ti[t] = (float)i;
		tj[t] = (float)j;
	}
	// source side first (addresses need only the offsets): 9 gathers in flight
	unsigned off[9];
	TapW<SMP> tw[9];
	float qd[9][4];
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		const f2 sp = apply_homography(H, tx[t], ty[t]);
		tex_coord_t<FMT>(d, sp.x, sp.y, &off[t], &tw[t]);
	}
#pragma unroll
	for (int t = 0; t < 9; ++t) load_quad_t<FMT>(src, off[t], &qd[t][0], &qd[t][1], &qd[t][2], &qd[t][3]);
	float av[9];
#pragma unroll
	for (int t = 0; t < 9; ++t) av[t] = ref_texel_t<FMT>(d, tx[t], ty[t]);
	float a_sr = 0.0f, a_srr = 0.0f, a_sw = 0.0f;
	float s_s = 0.0f, s_ss = 0.0f, s_rs = 0.0f;
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		const float w = bilateral_weight(ti[t], tj[t], av[t], cpix, d.params.sigma_spatial, d.params.sigma_color, 1);
		const float wa = w * av[t];
		a_sr += wa;
		a_srr += wa * av[t];
		a_sw += w;
		float fa, fb;
		tap_weights(tw[t], &fa, &fb);
		const float b = tex_lerp(fa, fb, qd[t][0], qd[t][1], qd[t][2], qd[t][3]);
		const float wb = w * b;
		s_s += wb;
		s_ss = fmaf(wb, b, s_ss);
		s_rs = fmaf(wa, b, s_rs);
	}
	return ncc_from_sums(a_sr, a_srr, s_s, s_ss, s_rs, a_sw);
}

// ---- the anchor sub-patches' reference side, once per pass -------------------------------------------------------------
// Of an anchor sub-patch (APD.cu:936-1006) only the nine gathers in the source image and the three source-side sums
// depend on the plane hypothesis.  The nine tap positions (anchor + the visibility-prior offsets of (anchor, view)), the
// colour weights w = exp(-|I(tap) - I(pixel)| / 2 sigma_c^2), the products w * I(tap) and the three reference sums depend
// on (WEAK pixel, view, anchor) only — and anchors (GenNeighbours / NeigbourUpdate) and offsets (GenEdgeInform) are fixed
// before the first iteration.  anchor_cost() recomputes them for every (view, anchor, PLANE) item of all three phases of
// every weak-update launch: 9 reference texel loads, 9 exp and 27 multiply-adds per item.  build_anchor_record() forms
// them ONCE per pass — same operations, same order, hence the same bits — into one 128-byte record per (WEAK pixel, view,
// anchor) (Dev::anchor_tab: 12.4 KB per WEAK pixel at S = 9; 22 GB at 6208x4128 with 7 % WEAK — it is a 288 GB part), and
// anchor_cost_tab() reads the record with eight 16-byte loads that the eight plane lanes of a pair share.
struct alignas(16) AnchorRec {
	f2 wt[9];            // (w, w * ref) per tap
	uint32_t pos[9];     // tap position: (x & 0xffff) | (y << 16), signed 16-bit halves
	float a_sr, a_srr, a_sw;
	uint32_t pad[2];
};
static_assert(sizeof(AnchorRec) == 128, "one cache line per (WEAK pixel, view, anchor)");
DVP_HD size_t anchor_rec_index(const Dev& d, int weak_index, int v0, int k) {
	return ((size_t)weak_index * (size_t)(d.params.num_images - 1) + (size_t)v0) * kAnchors + (size_t)k;
}
// record of anchor k (0-based: neighbours[k + 1]) of the WEAK pixel `center` for source view v0 (0-based); FMT: the plane format
// the reference texels are read from (the same values either way)
// -> *out, *index (its place in Dev::anchor_tab); false: no anchor, the record is never read (state 0)
template <int FMT>
DVP_HD bool make_anchor_record(const Dev& d, int center, int v0, int k, AnchorRec* out, size_t* index) {
	const int W = d.width;
	const int py = center / W, px = center - py * W;
	const int wi = d.neighbours_map[center];
	const s2 nb = d.neighbours[(size_t)wi * DVP_NEIGHBOUR_NUM + k + 1];
	if (nb.x == -1 || nb.y == -1) return false;
	const float cpix = ref_texel_t<FMT>(d, px, py);
	// the anchor's eight visibility-prior offsets for the view: one 32-byte record, two 16-byte loads (as eight 4-byte loads they
	// were 8 of the thread's 20 L2 requests, and the launch issues 160 G requests/s: PMC r05)
	s2 cand[8];
	{
		const s2* cp = d.candidate + cand_index(d, nb.x + nb.y * W, v0);
#if defined(__HIP_DEVICE_COMPILE__)
		typedef uint32_t u4 __attribute__((ext_vector_type(4)));
		const u4 lo = reinterpret_cast<const u4*>(cp)[0], hi = reinterpret_cast<const u4*>(cp)[1];
		const uint32_t w[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
#pragma unroll
		for (int t = 0; t < 8; ++t) cand[t] = mks2((int)(int16_t)(w[t] & 0xffffu), (int)(int16_t)(w[t] >> 16));
#else
		for (int t = 0; t < 8; ++t) cand[t] = cp[t];
#endif
	}
	AnchorRec& r = *out;
	float a_sr = 0.0f, a_srr = 0.0f, a_sw = 0.0f;
	// the nine texels first (one round trip; fetched inside the tap loop they were nine, each behind the `default ring` branch)
	int ti[9], tj[9];
	float tav[9];
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		int i = 0, j = 0;
		if (t < 8) {
			i = cand[t].x;
			j = cand[t].y;
			const bool ring = i == 0 && j == 0;   // default +-5 ring (APD.cu:943-952): {-5,0,5}^2 without its centre, x-major
			const int u = t + (t >= 4 ? 1 : 0);
			i = ring ? (u / 3 - 1) * 5 : i;
			j = ring ? (u % 3 - 1) * 5 : j;
		}
		ti[t] = i; tj[t] = j;
		tav[t] = ref_texel_t<FMT>(d, nb.x + i, nb.y + j);
	}
	sched_fence();
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		const int i = ti[t], j = tj[t];
		const int tx = nb.x + i, ty = nb.y + j;
		const float av = tav[t];
		const float w = bilateral_weight((float)i, (float)j, av, cpix, d.params.sigma_spatial, d.params.sigma_color, 1);
		const float wa = w * av;
		a_sr += wa;
		a_srr += wa * av;
		a_sw += w;
		r.wt[t] = mk2(w, wa);
		r.pos[t] = ((uint32_t)tx & 0xffffu) | ((uint32_t)ty << 16);
	}
	r.a_sr = a_sr;
	r.a_srr = a_srr;
	r.a_sw = a_sw;
	r.pad[0] = r.pad[1] = 0u;
	*index = anchor_rec_index(d, wi, v0, k);
	return true;
}
template <int FMT = 0>
DVP_HD void build_anchor_record(const Dev& d, int center, int v0, int k) {
	AnchorRec r;
	size_t index;
	if (!make_anchor_record<FMT>(d, center, v0, k, &r, &index)) return;
#if defined(__HIP_DEVICE_COMPILE__)
	{   // eight 16-byte stores
		typedef uint32_t u4 __attribute__((ext_vector_type(4)));
		const u4* src4 = reinterpret_cast<const u4*>(&r);
		u4* dst4 = reinterpret_cast<u4*>(d.anchor_tab + index);
#pragma unroll
		for (int i = 0; i < 8; ++i) dst4[i] = src4[i];
	}
#else
	d.anchor_tab[index] = r;
#endif
}

// anchor_cost() with the reference side taken from the pass' table
template <int SMP, int FMT>
DVP_HD float anchor_cost_tab(const Dev& d, const float* H, const void* src, s2 nb, int state, const AnchorRec* recp) {
	const int W = d.width, Hh = d.height, Pt = d.pitch;
	if (state == 0) return -1.0f;
	const bool visible = state == 2;
	const f2 nsp = apply_homography(H, nb.x, nb.y);
	const bool outside = nsp.x < 0 || nsp.y < 0 || nsp.x >= W || nsp.y >= Hh;
	if (outside) return visible ? 2.0f : -1.0f;
	if (!visible) return 2.0f;   // anchor not visible in this view: the reference's 0/0 path yields exactly 2
#if defined(DVP_ABL_NO_ANCHOR)   // timing ablation (wrong results): what the launch costs without the anchor sub-patches
	return 1.0f;
#endif
	AnchorRec r;
#if defined(__HIP_DEVICE_COMPILE__)
	{   // eight 16-byte loads (a plain struct copy is split into 30 dword loads)
		typedef uint32_t u4 __attribute__((ext_vector_type(4)));
		const u4* src4 = reinterpret_cast<const u4*>(recp);
		u4* dst4 = reinterpret_cast<u4*>(&r);
#pragma unroll
		for (int i = 0; i < 8; ++i) dst4[i] = src4[i];
	}
#else
	r = *recp;
#endif
	unsigned off[9];
	TapW<SMP> tw[9];
	float qd[9][4];
#if defined(DVP_ABL_ANCHOR_BATCH_RCP)
	// TIMING A/B OF A CONTRACT CHANGE (different bits): the nine projective divides of a sub-patch through ONE
	// correctly rounded division (prefix products, as batch_rcp does for the six taps of a centre-patch row) instead of one each
	{
		float X[9], Y[9], Z[9], P[9], IZ[9];
#pragma unroll
		for (int t = 0; t < 9; ++t) {
			const int tx = (int)(int16_t)(r.pos[t] & 0xffffu), ty = (int)(int16_t)(r.pos[t] >> 16);
			X[t] = H[0] * tx + H[1] * ty + H[2];
			Y[t] = H[3] * tx + H[4] * ty + H[5];
			Z[t] = H[6] * tx + H[7] * ty + H[8];
		}
		P[0] = Z[0];
#pragma unroll
		for (int t = 1; t < 9; ++t) P[t] = P[t - 1] * Z[t];
		float rr = 1.0f / P[8];
#pragma unroll
		for (int t = 8; t >= 1; --t) { IZ[t] = rr * P[t - 1]; rr = rr * Z[t]; }
		IZ[0] = rr;
#pragma unroll
		for (int t = 0; t < 9; ++t) tex_coord_t<FMT>(d, X[t] * IZ[t], Y[t] * IZ[t], &off[t], &tw[t]);
	}
#else
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		const f2 sp = apply_homography(H, (int)(int16_t)(r.pos[t] & 0xffffu), (int)(int16_t)(r.pos[t] >> 16));
		tex_coord_t<FMT>(d, sp.x, sp.y, &off[t], &tw[t]);
#if defined(DVP_ABL_ANCHOR_NOGATHER)   // timing ablation (wrong results): every gather hits one line
		off[t] = (unsigned)t * 4u;
#endif
	}
#endif
#pragma unroll
	for (int t = 0; t < 9; ++t) load_quad_t<FMT>(src, off[t], &qd[t][0], &qd[t][1], &qd[t][2], &qd[t][3]);
	float s_s = 0.0f, s_ss = 0.0f, s_rs = 0.0f;
#pragma unroll
	for (int t = 0; t < 9; ++t) {
		float fa, fb;
		tap_weights(tw[t], &fa, &fb);
		const float b = tex_lerp(fa, fb, qd[t][0], qd[t][1], qd[t][2], qd[t][3]);
		const float wb = r.wt[t].x * b;
		s_s += wb;
		s_ss = fmaf(wb, b, s_ss);
		s_rs = fmaf(r.wt[t].y, b, s_rs);
	}
	return ncc_from_sums(r.a_sr, r.a_srr, s_s, s_ss, s_rs, r.a_sw);
}

// ComputeBilateralNCCNew (APD.cu:835-1021) for the live planes sh.pl[q] (q in pmask) and the source views
// in vmask: sh.ev[q][view] = cost.  c = centre-patch context (colour-only weights) built by wave_patch_ctx.
// Views are taken kWeakPairs / np at a time with ONE shared-memory hand-over per batch:
//   section 1  per view of the batch, back to back:
//              lane (plane q, anchor k): the whole anchor sub-patch of that pair in registers — the
//              anchor's 9 reference taps (offsets, texels, weights, sums: identical in the 8 plane lanes
//              of an anchor, which costs nothing in lock step) and the 9 gathers in the source image;
//              the 8 planes of one tap sit in adjacent lanes of ONE load instruction and share lines.
//              The anchor pixel and its view mask do not depend on the view and are fetched once.
//              Then lane (plane q, row r): one row of the 36-tap centre patch.
//   section 2  lane (view slot, plane q): rows and anchors summed in the reference's order -> ev.
template <int SMP, int FMT>
DVP_HD void wave_ncc_new(const Dev& d, const PatchCtx& c, const s2* nbs, float cpix, int px, int py, uint32_t vmask, uint32_t pmask, WeakShared& sh) {
	const int W = d.width, Hh = d.height, Pt = d.pitch;
	const int np = 32 - __builtin_clz(pmask | 1u);   // plane slots in use (8 candidates, then 2 and 5)
	uint32_t rest = vmask;
	while (rest) {
		uint32_t batch = 0;
		for (int n = 0; n < kWeakPairs / np && n < kWeakViews && rest; ++n) { const uint32_t low = rest & (0u - rest); batch |= low; rest ^= low; }
		// Work items of the batch, 64 per round over the lanes:
		//   anchor items (view slot, anchor k, plane q), q fastest: the np planes of one (view, anchor) sit in
		//   adjacent lanes, so a load instruction's lanes share lines; a round is full whatever np is (the 2- and
		//   5-plane refinement phases and the second half of the 88 pairs of an 8-plane view used to leave
		//   60-75 % of a round's lanes idle);
		//   centre items (view slot, plane, patch row).
		// A lane's view changes from item to item, so the per-view constants are per-lane loads here.
		const int nv = __builtin_popcount(batch);
		const int rows_per = c.fast ? kTaps : 1;
		// the (view, anchor) pairs of the batch: what the anchor is worth in that view and its offsets, loaded by 64
		// lanes at a time BEFORE the items (every item used to start with two dependent loads — the anchor's
		// selected_views word, then its offsets — in front of its gathers)
		for (int i0 = 0; i0 < nv * kAnchors; i0 += 64) {
			DVP_LANES(l) {
				const int i = i0 + l;
				if (i >= nv * kAnchors) continue;
				const int slot = i / kAnchors, k = i - slot * kAnchors;
				const s2 nb = nbs[k + 1];
				int state = 0;
				if (!(nb.x == -1 || nb.y == -1)) {
					const int nbc = nb.x + nb.y * W;
					const int v0 = nth_set_bit(batch, slot);   // 0-based view
					state = is_set(d.selected_views[nbc], v0) ? 2 : 1;
					if (state == 2) {
						const s2* cand = d.candidate + cand_index(d, nbc, v0);
#pragma unroll
						for (int t = 0; t < 4; ++t) {
							const s2 a = cand[2 * t], b = cand[2 * t + 1];
							sh.aoff[i][t] = ((uint32_t)(uint8_t)(int8_t)a.x) | ((uint32_t)(uint8_t)(int8_t)a.y << 8) |
							                ((uint32_t)(uint8_t)(int8_t)b.x << 16) | ((uint32_t)(uint8_t)(int8_t)b.y << 24);
						}
					}
				}
				sh.astate[i] = (uint8_t)state;
			}
		}
		wave_sync();
		DVP_LANES(l) {
			const int n_anchor = nv * kAnchors * np;
			for (int it0 = 0; it0 < n_anchor; it0 += 64) {
				const int it = it0 + l;
				if (it >= n_anchor) continue;
				const int q = it % np, t2 = it / np;
				const int k = t2 % kAnchors, slot = t2 / kAnchors;
				if (!((pmask >> q) & 1)) continue;
				const int v = nth_set_bit(batch, slot) + 1;   // 1-based image index of the source view
				const ViewConst vc = d.views[v];
				float H[9];
				homography(vc, sh.pl[q], H);
				const f2 pt = apply_homography(H, px, py);
				const bool inside = !(pt.x >= vc.fw || pt.x < 0.0f || pt.y >= vc.fh || pt.y < 0.0f);
				if (k == 0) sh.inq[slot * np + q] = inside ? 1 : 0;
				if (!inside) continue;
				sh.acost[slot * np + q][k] = anchor_cost<SMP, FMT>(d, H, img_plane<FMT>(d, v), nbs[k + 1], sh.astate[slot * kAnchors + k], sh.aoff[slot * kAnchors + k], cpix);
			}
			const int n_centre = nv * np * rows_per;
			for (int it0 = 0; it0 < n_centre; it0 += 64) {
				const int it = it0 + l;
				if (it >= n_centre) continue;
				const int r = it % rows_per, t2 = it / rows_per;
				const int cq = t2 % np, slot = t2 / np;
				if (!((pmask >> cq) & 1)) continue;
				const int v = nth_set_bit(batch, slot) + 1;
				const ViewConst vc = d.views[v];
				float Hc[9];
				homography(vc, sh.pl[cq], Hc);
				const f2 pt = apply_homography(Hc, px, py);
				if (pt.x >= vc.fw || pt.x < 0.0f || pt.y >= vc.fh || pt.y < 0.0f) continue;
#if defined(DVP_ABL_NO_CENTRE)   // timing ablation (wrong results): what the launch costs without the centre patches
				continue;
#endif
				if (c.fast) {
					float o[3];
					patch_row_sums<SMP, FMT>(d, sh, Hc, img_plane<FMT>(d, v), px, py, c.radius, c.inc, r, o);
					sh.rows[slot * np + cq][r][0] = o[0];
					sh.rows[slot * np + cq][r][1] = o[1];
					sh.rows[slot * np + cq][r][2] = o[2];
				} else {   // generic (non-6-tap) patches sample the float planes
					sh.rows[slot * np + cq][0][0] = ncc_patch_generic(d, Hc, d.images + (size_t)v * d.plane_stride * 2, px, py, c.radius, c.inc, 1);
				}
			}
		}
		wave_sync();
		DVP_LANES(l) {
		for (int it0 = 0; it0 < nv * np; it0 += 64) {   // items (view slot, plane)
			const int it = it0 + l;
			if (it >= nv * np) continue;
			const int slot = it / np, q = it % np;
			if (!((pmask >> q) & 1)) continue;
			const int v = nth_set_bit(batch, slot);   // 0-based view index
			if (!sh.inq[slot * np + q]) { sh.ev[q][v] = 2.0f; continue; }
			float cc;
			if (c.fast) {
				float s_s = 0.0f, s_ss = 0.0f, s_rs = 0.0f;
				for (int r = 0; r < kTaps; ++r) {
					s_s += sh.rows[slot * np + q][r][0];
					s_ss += sh.rows[slot * np + q][r][1];
					s_rs += sh.rows[slot * np + q][r][2];
				}
				cc = ncc_from_sums(c.sum_ref, c.sum_ref_ref, s_s, s_ss, s_rs, c.wsum);
			} else {
				cc = sh.rows[slot * np + q][0][0];
			}
			float scost = 0.0f, scnt = 0.0f;
			for (int k = 0; k < kAnchors; ++k) {
				const float ac = sh.acost[slot * np + q][k];
				if (ac >= 0.0f) { scost += ac; scnt += 1.0f; }
			}
			float out = cc;
			if (scnt > 0.0f) {
				float sc2 = scost / scnt;   // strong_cost /= strong_count (int -> float, exact)
				sc2 = DVP_MIN(sc2, 2.0f);
				out = (float)(0.25 * cc + 0.75 * sc2);
			}
			sh.ev[q][v] = out;
		}
		}
		wave_sync();
	}
}

// it / n for 0 <= it < 65536, 1 <= n <= 64 through one float multiplication (exact: (it + 0.5) / n is at least 1 / 2n away from
// an integer, the rounding error of the product is below 2^-7); the generic 32-bit division is ~25 instructions
DVP_HD int small_div(int it, float inv_n) { return (int)(((float)it + 0.5f) * inv_n); }

// wave_ncc_new with the anchor reference sides from the pass' table (TAB = 1).  Same evaluations, same bits; what changes
// is the bookkeeping around them:
//   * the homography of a (view, plane) pair is formed ONCE per batch into sh.Hq (section 0) instead of by each of the
//     pair's 17 items — 11 anchor sub-patches and 6 centre rows — (a quarter of an anchor round's instructions);
//   * the live planes are compacted: pair = view slot * np + (index among the set bits of pmask), np = popcount(pmask),
//     so the refinement phase's survivors (e.g. hypotheses 1 and 4 of 5) fill whole rounds;
//   * items decode with small_div.
template <int SMP, int FMT>
DVP_HD void wave_ncc_new_tab(const Dev& d, const PatchCtx& c, const s2* nbs, int px, int py, uint32_t vmask, uint32_t pmask, WeakSharedT<1>& sh) {
	const int W = d.width;
	const int np = __builtin_popcount(pmask);
	if (np == 0) return;
	const float inv_np = 1.0f / (float)np;
	const int weak_index = d.neighbours_map[px + py * W];
	uint32_t rest = vmask;
	while (rest) {
		uint32_t batch = 0;
		for (int n = 0; n < kWeakPairs / np && n < kWeakViews && rest; ++n) { const uint32_t low = rest & (0u - rest); batch |= low; rest ^= low; }
		const int nv = __builtin_popcount(batch);
		const int rows_per = c.fast ? kTaps : 1;
		// section 0: (view slot, anchor) states and the homographies of the (view slot, plane) pairs
		for (int i0 = 0; i0 < nv * kAnchors; i0 += 64) {
			DVP_LANES(l) {
				const int i = i0 + l;
				if (i >= nv * kAnchors) continue;
				const int slot = i / kAnchors, k = i - slot * kAnchors;
				const s2 nb = nbs[k + 1];
				int state = 0;
				if (!(nb.x == -1 || nb.y == -1)) state = is_set(d.selected_views[nb.x + nb.y * W], nth_set_bit(batch, slot)) ? 2 : 1;
				sh.astate[i] = (uint8_t)state;
			}
		}
		DVP_LANES(l) {
			if (l >= nv * np) continue;
			const int slot = small_div(l, inv_np), qi = l - slot * np;
			const int v = nth_set_bit(batch, slot) + 1;   // 1-based image index of the source view
			const ViewConst vc = d.views[v];
			float H[9];
			homography(vc, sh.pl[nth_set_bit(pmask, qi)], H);
			const f2 pt = apply_homography(H, px, py);
			sh.inq[l] = !(pt.x >= vc.fw || pt.x < 0.0f || pt.y >= vc.fh || pt.y < 0.0f) ? 1 : 0;
#pragma unroll
			for (int i = 0; i < 9; ++i) sh.Hq[l][i] = H[i];
		}
		wave_sync();
		// section 1: anchor items (view slot, anchor k, live plane qi), qi fastest — the np planes of one (view, anchor) sit in
		// adjacent lanes, so a load instruction's lanes share lines —, then centre items (pair, patch row)
		DVP_LANES(l) {
			const int n_anchor = nv * kAnchors * np;
			for (int it0 = 0; it0 < n_anchor; it0 += 64) {
				const int it = it0 + l;
				if (it >= n_anchor) continue;
				const int t2 = small_div(it, inv_np), qi = it - t2 * np;
				const int slot = t2 / kAnchors, k = t2 - slot * kAnchors;
				const int pair = slot * np + qi;
				if (!sh.inq[pair]) continue;
				const int v = nth_set_bit(batch, slot) + 1;
				float H[9];
#pragma unroll
				for (int i = 0; i < 9; ++i) H[i] = sh.Hq[pair][i];
				sh.acost[pair][k] = anchor_cost_tab<SMP, FMT>(d, H, img_plane<FMT>(d, v), nbs[k + 1], sh.astate[slot * kAnchors + k], d.anchor_tab + anchor_rec_index(d, weak_index, v - 1, k));
			}
			const int n_centre = nv * np * rows_per;
			for (int it0 = 0; it0 < n_centre; it0 += 64) {
				const int it = it0 + l;
				if (it >= n_centre) continue;
				const int pair = it / rows_per, r = it - pair * rows_per;
				if (!sh.inq[pair]) continue;
#if defined(DVP_ABL_NO_CENTRE)   // timing ablation (wrong results)
				continue;
#endif
				const int slot = small_div(pair, inv_np);
				const int v = nth_set_bit(batch, slot) + 1;
				float Hc[9];
#pragma unroll
				for (int i = 0; i < 9; ++i) Hc[i] = sh.Hq[pair][i];
				if (c.fast) {
					float o[3];
					patch_row_sums<SMP, FMT>(d, sh, Hc, img_plane<FMT>(d, v), px, py, c.radius, c.inc, r, o);
					sh.rows[pair][r][0] = o[0];
					sh.rows[pair][r][1] = o[1];
					sh.rows[pair][r][2] = o[2];
				} else {   // generic (non-6-tap) patches sample the float planes
					sh.rows[pair][0][0] = ncc_patch_generic(d, Hc, d.images + (size_t)v * d.plane_stride * 2, px, py, c.radius, c.inc, 1);
				}
			}
		}
		wave_sync();
		// section 2: lane = pair: rows and anchors summed in the reference's order -> ev
		DVP_LANES(l) {
			for (int it0 = 0; it0 < nv * np; it0 += 64) {
				const int pair = it0 + l;
				if (pair >= nv * np) continue;
				const int slot = small_div(pair, inv_np), qi = pair - slot * np;
				const int q = nth_set_bit(pmask, qi);
				const int v = nth_set_bit(batch, slot);   // 0-based view index
				if (!sh.inq[pair]) { sh.ev[q][v] = 2.0f; continue; }
				float cc;
				if (c.fast) {
					float s_s = 0.0f, s_ss = 0.0f, s_rs = 0.0f;
					for (int r = 0; r < kTaps; ++r) {
						s_s += sh.rows[pair][r][0];
						s_ss += sh.rows[pair][r][1];
						s_rs += sh.rows[pair][r][2];
					}
					cc = ncc_from_sums(c.sum_ref, c.sum_ref_ref, s_s, s_ss, s_rs, c.wsum);
				} else {
					cc = sh.rows[pair][0][0];
				}
				float scost = 0.0f, scnt = 0.0f;
				for (int k = 0; k < kAnchors; ++k) {
					const float ac = sh.acost[pair][k];
					if (ac >= 0.0f) { scost += ac; scnt += 1.0f; }
				}
				float out = cc;
				if (scnt > 0.0f) {
					float sc2 = scost / scnt;   // strong_cost /= strong_count (int -> float, exact)
					sc2 = DVP_MIN(sc2, 2.0f);
					out = (float)(0.25 * cc + 0.75 * sc2);
				}
				sh.ev[q][v] = out;
			}
		}
		wave_sync();
	}
}

// gtab[q][j] = ComputeGeomConsistencyCost(pixel, view j+1, sh.pl[q]) for q in pmask, views with weight > 0
template <class SH>
DVP_HD void wave_geom_table(const Dev& d, const DvpCamera& rc, int px, int py, uint32_t pmask, SH& sh) {
	const int S = d.params.num_images - 1;
	for (int j0 = 0; j0 < S; j0 += 8) {
		DVP_LANES(l) {
			const int q = l >> 3, j = j0 + (l & 7);
			if (j >= S || !((pmask >> q) & 1) || sh.vw[j] == 0) continue;
			sh.gtab[q][j] = geom_cost_cams(d, rc, d.cameras[j + 1], j + 1, px, py, sh.pl[q]);
		}
	}
	wave_sync();
}

template <int SMP, int FMT>
DVP_HD void weak_eval(const Dev& d, const PatchCtx& c, const s2* nbs, float cpix, int px, int py, uint32_t vmask, uint32_t pmask, WeakSharedT<0>& sh) {
	wave_ncc_new<SMP, FMT>(d, c, nbs, cpix, px, py, vmask, pmask, sh);
}
template <int SMP, int FMT>
DVP_HD void weak_eval(const Dev& d, const PatchCtx& c, const s2* nbs, float cpix, int px, int py, uint32_t vmask, uint32_t pmask, WeakSharedT<1>& sh) {
	wave_ncc_new_tab<SMP, FMT>(d, c, nbs, px, py, vmask, pmask, sh);
}

template <int SMP, int FMT, int TAB>
DVP_HD void weak_update_wave(const Dev& d, int px, int py, int iter, unsigned long long* nevals, WeakSharedT<TAB>& sh) {
	const int W = d.width, Hh = d.height;
	const int center = py * W + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const uint32_t all_views = (S >= 32) ? 0xFFFFFFFFu : ((1u << S) - 1u);
	const s2* nbs = d.neighbours + (size_t)d.neighbours_map[center] * DVP_NEIGHBOUR_NUM;
	const float cpix = ref_texel_t<FMT>(d, px, py);
	unsigned long long evals = 0;

	PatchCtx c;
	c.tab = PatchTab{nullptr, 0};
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		wave_patch_ctx<FMT>(d, px, py, radius, inc, 1, sh, &c);
	}
	DVP_LANES(l) {
		if (l < 32) sh.vw[l] = 0;
		if (l < 8) sh.positions[l] = 0;
	}
	wave_sync();
	// (cost_array: `= { 2.0f }` sets one element, the rest is 0 (APD.cu:2769) — written whole by the epilogue of the propagation
	// phase below; until then its bytes hold the batch homographies of the TAB form)
	uint32_t flag = 0;
	uint32_t sel_mask = 0;
	uint32_t sel_now = d.selected_views[center];   // what random_normal_yzl reads (updated on adoption)
	float weight_norm = 0.0f;
	int min_cost_idx = 0;
	float cost_now = 0.0f, costs_center = 0.0f, depth_now = 0.0f;
	f4 plane_now = mk4(0, 0, 0, 0);
	bool skip_refine = false;
	f4 pl1 = mk4(0, 0, 0, 0);

	for (int phase = 0; phase < 3; ++phase) {
		uint32_t pmask = 0, vmask = 0;
		if (phase == 0) {
			for (int k = 0; k < 8; ++k) {
				const s2 nb = nbs[k + 1];
				if (!(nb.x == -1 || nb.y == -1) && d.weak_info[nb.x + nb.y * W] == DVP_STRONG) {
					flag |= 1u << k;
					if (DVP_LANE0) {
						sh.positions[k] = nb.x + nb.y * W;
						sh.pl[k] = d.planes[nb.x + nb.y * W];
					}
				}
			}
			pmask = flag;
			vmask = all_views;
		} else if (phase == 1) {
			// joint view selection (APD.cu:2781-2850): lane j owns view j for the per-view parts
			const float thr = (float)(0.8 * dvp_expf((iter) * (iter) / (-90.0f)));
			DVP_LANES(j) {
				if (j >= S) continue;
				float pr = 0.0f;
				for (int i = 0; i < 8; ++i) {
					const s2 nb = nbs[i + 1];
					if (nb.x == -1 || nb.y == -1) continue;
					pr += is_set(d.selected_views[nb.x + nb.y * W], j) ? 0.9f : 0.1f;
				}
				float count = 0;
				int count_false = 0;
				float tmpw = 0;
				for (int k = 0; k < 8; k++) {
					const float cst = sh.cost_array[k][j];
					if (cst < thr) { tmpw += dvp_expf(cst * cst / (-0.18f)); count++; }
					if (cst > 1.2f) count_false++;
				}
				float p = 0.0f;
				if (count > 2 && count_false < 3) p = tmpw / count;
				else if (count_false < 3) p = dvp_expf(thr * thr / (-0.32f));
				sh.probs[j] = p * pr;
			}
			wave_sync();
			float psum = 0.0f;
			for (int i = 0; i < S; ++i) psum += sh.probs[i];
			const float inv = 1.0f / psum;
			float cum = 0.0f;
			wave_sync();
			for (int i = 0; i < S; ++i) {
				cum += sh.probs[i] * inv;
				if (DVP_LANE0) sh.priors[i] = cum;   // the CDF (priors[] is free from here on)
			}
			wave_sync();
			Rng rv(d.seed, (uint32_t)center, rng_site(PH_WEAK, iter, SUB_VIEW));
			for (int s = 0; s < 15; ++s) {
				const float rp = rv.uniform() - FLT_EPSILON;
				for (int v = 0; v < S; ++v)
					if (sh.priors[v] > rp) { if (DVP_LANE0) sh.vw[v] += 1; break; }
			}
			wave_sync();
			sel_mask = 0;
			weight_norm = 0;
			for (int i = 0; i < S; ++i)
				if (sh.vw[i] > 0) { set_bit(&sel_mask, i); weight_norm += sh.vw[i]; }
			DVP_LANES(i) { if (i < 32) d.view_weight[(size_t)center * 32 + i] = sh.vw[i]; }
			// weighted candidate costs (APD.cu:2852-2874); sh.pl[k] still holds the anchors' planes
			if (P.geom_consistency) wave_geom_table(d, rc, px, py, flag, sh);
			DVP_LANES(k) {
				if (k >= 8) continue;
				float fc = 0.0f;
				for (int j = 0; j < S; ++j) {
					const int w = sh.vw[j];
					if (w > 0) {
						if (P.geom_consistency) {
							if ((flag >> k) & 1) fc += w * (sh.cost_array[k][j] + P.geom_factor * sh.gtab[k][j]);
							else fc += w * (sh.cost_array[k][j] + P.geom_factor * 3.0f);
						} else {
							fc += w * sh.cost_array[k][j];
						}
					}
				}
				sh.fcost[k] = fc / weight_norm;
			}
			wave_sync();
			min_cost_idx = 0;
			{
				float mc = sh.fcost[0];
				for (int k = 1; k < 8; ++k)
					if (sh.fcost[k] <= mc) { mc = sh.fcost[k]; min_cost_idx = k; }
			}
			const f4 fp = d.fit_planes[center];
			pl1 = fp;
			pmask = 1u;
			if (fp.x == 0 && fp.y == 0 && fp.z == 0) skip_refine = true;
			else pmask |= 2u;
			wave_sync();
			if (DVP_LANE0) {
				sh.pl[0] = d.planes[center];
				if (!skip_refine) sh.pl[1] = fp;
			}
			vmask = sel_mask;
		} else {
			if (skip_refine) break;
			Rng rd(d.seed, (uint32_t)center, rng_site(PH_WEAK, iter, SUB_DEPTH_RAND));
			Rng rn(d.seed, (uint32_t)center, rng_site(PH_WEAK, iter, SUB_NORMAL));
			Rng rp(d.seed, (uint32_t)center, rng_site(PH_WEAK, iter, SUB_DEPTH_PERT));
			const float depth_rand = rd.uniform() * (P.depth_max - P.depth_min) + P.depth_min;
			const f4 n_rand = random_normal_yzl_sel(d, px, py, rn, depth_now, sel_now);
			const float dmin_p = (1 - 0.02f) * depth_now, dmax_p = (1 + 0.02f) * depth_now;
			const float depth_pert = rp.uniform() * (dmax_p - dmin_p) + dmin_p;
			f4 n_pert = plane_now;
			normalize3(&n_pert);
			const float rdep[5] = { depth_rand, depth_now, depth_rand, depth_now, depth_pert };
			const f4 rnrm[5] = { plane_now, n_rand, n_rand, n_pert, plane_now };
			wave_sync();
#pragma unroll
			for (int i = 0; i < 5; ++i) {
				f4 h = rnrm[i];
				h.w = distance_to_origin(rc, px, py, rdep[i], h);
				if (DVP_LANE0) sh.pl[i] = h;
			}
			pmask = 0x1Fu;
			vmask = sel_mask;
		}
		wave_sync();

		// ---- evaluate: view by view ----------------------------------------------------------------------
		if (phase == 2 && pmask && vmask) {
			// The five refinement hypotheses are adopted iff their depth is in range and their weighted cost is below the
			// running best, which only ever decreases (APD.cu:1361-1383).  Two exact short cuts — the costs themselves are
			// only kept on adoption: (i) out-of-range hypotheses are not evaluated; (ii) the weighted sum only grows (weights
			// > 0, costs >= 0, IEEE addition and division are monotone), so a hypothesis whose FIRST selected view alone is
			// not below the best cost at entry can never be adopted: it drops out before the remaining views are evaluated.
			uint32_t keep = 0;
			for (int i = 0; i < 5; ++i) {
				const float db = depth_from_plane(rc, sh.pl[i], px, py);
				if (db >= P.depth_min && db <= P.depth_max) keep |= 1u << i;
			}
			pmask = keep;
			int first = 0;
			while (!((vmask >> first) & 1)) ++first;
			if (pmask) {
				weak_eval<SMP, FMT>(d, c, nbs, cpix, px, py, 1u << first, pmask, sh);
				evals += (unsigned long long)__builtin_popcount(pmask);
				if (P.geom_consistency) wave_geom_table(d, rc, px, py, pmask, sh);
				uint32_t alive = 0;
				const int w = sh.vw[first];
				for (int i = 0; i < 5; ++i) {
					if (!((pmask >> i) & 1)) continue;
					float tc = 0.0f;
					if (P.geom_consistency) tc += w * (sh.ev[i][first] + P.geom_factor * sh.gtab[i][first]);
					else tc += w * sh.ev[i][first];
					if (tc / weight_norm < cost_now) alive |= 1u << i;
				}
				pmask = alive;
				const uint32_t rest = vmask & ~(1u << first);
				if (pmask && rest) {
					weak_eval<SMP, FMT>(d, c, nbs, cpix, px, py, rest, pmask, sh);
					evals += (unsigned long long)__builtin_popcount(pmask) * (unsigned long long)__builtin_popcount(rest);
				}
			}
		} else if (pmask && vmask) {
			weak_eval<SMP, FMT>(d, c, nbs, cpix, px, py, vmask, pmask, sh);
			evals += (unsigned long long)__builtin_popcount(pmask) * (unsigned long long)__builtin_popcount(vmask);
		}

		// ---- epilogue ----------------------------------------------------------------------------------------
		if (phase == 0) {
			DVP_LANES(l) {
				for (int i = l; i < 8 * 32; i += 64) {
					const int k = i >> 5, v = i & 31;
					sh.cost_array[k][v] = (((flag >> k) & 1) && v < S) ? sh.ev[k][v] : (i == 0 ? 2.0f : 0.0f);
				}
			}
			wave_sync();
		} else if (phase == 1) {
			if (P.geom_consistency) wave_geom_table(d, rc, px, py, pmask, sh);
			float cn = 0.0f;
			for (int v = 0; v < S; ++v) {
				const int w = sh.vw[v];
				if (w > 0) {
					if (P.geom_consistency) cn += w * (sh.ev[0][v] + P.geom_factor * sh.gtab[0][v]);
					else cn += w * sh.ev[0][v];
				}
			}
			cost_now = cn / weight_norm;
			costs_center = cost_now;
			plane_now = sh.pl[0];
			depth_now = depth_from_plane(rc, plane_now, px, py);
			if ((flag >> min_cost_idx) & 1) {
				const f4 cand = d.planes[sh.positions[min_cost_idx]];
				const float db = depth_from_plane(rc, cand, px, py);
				if (db >= P.depth_min && db <= P.depth_max && sh.fcost[min_cost_idx] < cost_now) {
					depth_now = db;
					plane_now = cand;
					cost_now = sh.fcost[min_cost_idx];
					sel_now = sel_mask;
					if (DVP_LANE0) d.selected_views[center] = sel_mask;
				}
			}
			if (!skip_refine) {   // fit-plane test
				float tc = 0.0f;
				for (int j = 0; j < S; ++j) {
					const int w = sh.vw[j];
					if (w > 0) {
						if (P.geom_consistency) tc += w * (sh.ev[1][j] + P.geom_factor * sh.gtab[1][j]);
						else tc += w * sh.ev[1][j];
					}
				}
				tc /= weight_norm;
				const float db = depth_from_plane(rc, pl1, px, py);
				if (db >= P.depth_min && db <= P.depth_max && tc < cost_now) {
					depth_now = db;
					plane_now = pl1;
					cost_now = tc;
				}
			}
		} else {
			// (geometric table: filled in the evaluate step; pmask = the hypotheses that are still candidates)
			for (int i = 0; i < 5; ++i) {
				if (!((pmask >> i) & 1)) continue;
				float tc = 0.0f;
				for (int j = 0; j < S; ++j) {
					const int w = sh.vw[j];
					if (w > 0) {
						if (P.geom_consistency) tc += w * (sh.ev[i][j] + P.geom_factor * sh.gtab[i][j]);
						else tc += w * sh.ev[i][j];
					}
				}
				tc /= weight_norm;
				const f4 h = sh.pl[i];
				const float db = depth_from_plane(rc, h, px, py);
				if (db >= P.depth_min && db <= P.depth_max && tc < cost_now) {
					depth_now = db;
					plane_now = h;
					cost_now = tc;
				}
			}
		}
	}

	f4 final_plane = d.planes[center];
	if (P.state == DVP_REFINE_INIT) {
		if (cost_now < costs_center - 0.1) final_plane = plane_now;
	} else {
		final_plane = plane_now;
	}
	wave_sync();
	if (DVP_LANE0) d.planes[center] = final_plane;

	// cost of the final plane with the plain bilateral NCC at the default radius (APD.cu:3072-3088):
	// lane = (view slot, patch row), eight views per round
	PatchCtx c2;
	c2.tab = PatchTab{nullptr, 0};
	{
		int r = P.strong_radius, inc = P.strong_increment;
		if (P.use_radius) inc = DVP_MAX(2, (int)(2.0 * r / 5.0));
		wave_patch_ctx<FMT>(d, px, py, r, inc, 0, sh, &c2);
	}
	for (int v0 = 0; v0 < S; v0 += 8) {
		DVP_LANES(l) {
			const int vs = l >> 3, r = l & 7, v = v0 + vs;
			if (v >= S || sh.vw[v] == 0) continue;
			if (c2.fast ? r >= kTaps : r != 0) continue;
			const ViewConst vc = d.views[v + 1];
			float H[9];
			homography(vc, final_plane, H);
			const f2 pt = apply_homography(H, px, py);
			const bool in = !(pt.x >= vc.fw || pt.x < 0.0f || pt.y >= vc.fh || pt.y < 0.0f);
			const void* src = img_plane<FMT>(d, v + 1);
			if (!c2.fast) {
				sh.ev[0][v] = in ? ncc_patch_generic(d, H, d.images + (size_t)(v + 1) * d.plane_stride * 2, px, py, c2.radius, c2.inc, 0) : 2.0f;
			} else if (in) {
				float o[3];
				patch_row_sums<SMP, FMT>(d, sh, H, src, px, py, c2.radius, c2.inc, r, o);
				sh.rows[vs][r][0] = o[0];
				sh.rows[vs][r][1] = o[1];
				sh.rows[vs][r][2] = o[2];
			} else if (r == 0) {
				sh.ev[0][v] = 2.0f;
				sh.inq[vs] = 0;   // "outside" for the totalling lane
			}
			if (c2.fast && in && r == 0) sh.inq[vs] = 1;
		}
		wave_sync();
		if (c2.fast) {
			DVP_LANES(l) {
				const int v = v0 + l;
				if (l >= 8 || v >= S || sh.vw[v] == 0 || !sh.inq[l]) continue;
				float s_s = 0.0f, s_ss = 0.0f, s_rs = 0.0f;
				for (int r = 0; r < kTaps; ++r) {
					s_s += sh.rows[l][r][0];
					s_ss += sh.rows[l][r][1];
					s_rs += sh.rows[l][r][2];
				}
				sh.ev[0][v] = ncc_from_sums(c2.sum_ref, c2.sum_ref_ref, s_s, s_ss, s_rs, c2.wsum);
			}
			wave_sync();
		}
	}
	float cn = 0.0f;
	for (int v = 0; v < S; ++v) {
		if (sh.vw[v] == 0) continue;
		cn += sh.vw[v] * sh.ev[0][v];
		evals += 1;
	}
	if (DVP_LANE0) {
		d.costs[center] = cn / weight_norm;
		if (nevals) *nevals += evals;
	}
	wave_sync();
}

}  // namespace dvp
#endif
