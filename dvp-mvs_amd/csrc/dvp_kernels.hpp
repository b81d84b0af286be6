// dvp_kernels.hpp — the gfx950 entry points of dvp_engine.hip: LaunchArgs / ListArgs, the launch-bound and list-run defaults
// (DVP_LB_*, DVP_LIST_RUN, DVP_WAVE_RUN), the kernel body templates and every extern "C" __global__ of the engine.  The
// per-pixel and per-wave bodies they call are in the device headers behind dvp_stages.hpp ("Where the code is").
// The entry points are at global scope and name the dvp:: types unqualified: the using-directive below is theirs.
#ifndef DVP_KERNELS_HPP_
#define DVP_KERNELS_HPP_

#include "dvp_stages.hpp"
#include <hip/hip_runtime.h>

using namespace dvp;

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct LaunchArgs {
	int tiles_x, tiles, rows, half, colour, iter;
};

template <int STAGE, int SMP, int MV = 32>
__device__ __forceinline__ void stage_body(const Dev& d, const LaunchArgs& a) {
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	int px, py;
	unsigned long long n = 0;
	// per-lane (w, w*ref) table of the hoisted patch context: [tap][lane] in LDS (72 KiB / workgroup)
	__shared__ f2 lds_tab[stage_uses_tab(STAGE) ? kTaps * kTaps * 256 : 1];
	const PatchTab tab{&lds_tab[stage_uses_tab(STAGE) ? threadIdx.x : 0], 256};
	if (block_to_pixel(blockIdx.x, lane, wave, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py))
		run_pixel<STAGE, SMP, MV>(d, px, py, a.iter, d.eval_counter ? &n : nullptr, tab);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}

// Compacted launch for the weak-pixel path: lane t owns the t-th WEAK pixel of the list segment.
// WEAK pixels are 1-30 % of a view; a lane-per-image-pixel launch leaves 70-99 % of the lanes idle.
struct ListArgs { int base, count, iter, covered_rows, group, run; };   // group: pixels per wave of the weak update's evaluation launches
// XCD-aware block -> list-block map.  Workgroup b runs on XCD b % 8 (observed placement, a speed matter
// only); the list is in super-tile order, so giving every XCD RUNS of kListRun consecutive list blocks
// (instead of every 8th block) keeps the workgroups that share anchors — and the source-image lines
// their anchor sub-patches gather — behind one L2.  Bijection on [0, nblocks): whole groups of
// 8 * kListRun blocks are permuted, the ragged tail keeps its order.
#ifndef DVP_LIST_RUN
#define DVP_LIST_RUN 16
#endif
constexpr int kListRun = DVP_LIST_RUN;
// The wave-per-pixel kernels (workgroup = 4 WEAK pixels) use shorter runs: 1 .. 64 blocks measure the same (weak update 400-402 ms
// per cfg3 pass), 256 blocks 405, the 1 024 of round 2 (the lane kernels' run in pixels) 419 — a run longer than what an XCD has
// in flight only delays the neighbours.
#ifndef DVP_WAVE_RUN
#define DVP_WAVE_RUN 16
#endif
constexpr int kWaveRun = DVP_WAVE_RUN;
__device__ __forceinline__ int list_block(int b, int nblocks, int run) {
	const int group = 8 * run;
	if (b >= nblocks / group * group) return b;
	const int g = b / group, r = b - g * group;
	const int xcd = r & 7, i = r >> 3;
	return g * group + xcd * run + i;
}
template <int STAGE, int SMP, int MV = 32>
__device__ __forceinline__ void stage_body_list(const Dev& d, const ListArgs& a) {
	__shared__ f2 lds_tab[stage_uses_tab(STAGE) ? kTaps * kTaps * 256 : 1];
	const PatchTab tab{&lds_tab[stage_uses_tab(STAGE) ? threadIdx.x : 0], 256};
	const int t = list_block(blockIdx.x, gridDim.x, kListRun) * 256 + threadIdx.x;
	unsigned long long n = 0;
	if (t < a.count) {
		const int center = d.weak_list[a.base + t];
		const int py = center / d.width, px = center - py * d.width;
		// red/black launches never reach rows beyond the reference's half grid (APD.cu:4421-4424)
		if (!stage_is_half_c(STAGE) || py < a.covered_rows)
			run_pixel<STAGE, SMP, MV>(d, px, py, a.iter, d.eval_counter ? &n : nullptr, tab);
	}
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
// The same launch sites with ONE wave per workgroup (18 KB of LDS each): tile t = the workgroups b with
// (b >> 5) * 8 + (b & 7) == t, its row (b >> 3) & 3 — the four rows of a tile stay on the XCD block_to_pixel's map gives the tile.
// No wave waits for the slowest of its workgroup before the LDS is given back: the strong update's evaluation and refinement
// kernels gain 11 ms per cfg3 pass (DepthToWeak nothing: stays on 256-lane workgroups).
template <int STAGE, int SMP, int MV = 32>
__device__ __forceinline__ void stage_body64(const Dev& d, const LaunchArgs& a) {
	const int lane = threadIdx.x;
	const int b = blockIdx.x;
	const int tile = (b >> 5) * 8 + (b & 7), wave = (b >> 3) & 3;
	int px, py;
	unsigned long long n = 0;
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	const PatchTab tab{&lds_tab[lane], 64};
	if (block_to_pixel(tile, lane, wave, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py))
		run_pixel<STAGE, SMP, MV>(d, px, py, a.iter, d.eval_counter ? &n : nullptr, tab);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
#define DVP_KERNEL64(NAME, STAGE, MINW)                                                                    \
	extern "C" __global__ void __launch_bounds__(64, MINW) NAME(const Dev d, const LaunchArgs a) {          \
		stage_body64<STAGE, 0>(d, a);                                                                       \
	}                                                                                                       \
	extern "C" __global__ void __launch_bounds__(64, MINW) NAME##_exact(const Dev d, const LaunchArgs a) {  \
		stage_body64<STAGE, 1>(d, a);                                                                       \
	}
#define DVP_KERNEL_LIST_MV(NAME, STAGE, MINW, MV)                                                         \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME(const Dev d, const ListArgs a) {         \
		stage_body_list<STAGE, 0, MV>(d, a);                                                               \
	}                                                                                                      \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME##_exact(const Dev d, const ListArgs a) { \
		stage_body_list<STAGE, 1, MV>(d, a);                                                               \
	}
#define DVP_KERNEL_LIST(NAME, STAGE, MINW)                                                                \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME(const Dev d, const ListArgs a) {         \
		stage_body_list<STAGE, 0>(d, a);                                                                   \
	}                                                                                                      \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME##_exact(const Dev d, const ListArgs a) { \
		stage_body_list<STAGE, 1>(d, a);                                                                   \
	}

// One named kernel per launch site so that rocprofv3 --kernel-trace shows the reference's names.
// NAME: sampler 0 (8-bit interpolation weights, default); NAME_exact: sampler 1.
#define DVP_KERNEL(NAME, STAGE, MINW)                                                                      \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME(const Dev d, const LaunchArgs a) {         \
		stage_body<STAGE, 0>(d, a);                                                                         \
	}                                                                                                       \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME##_exact(const Dev d, const LaunchArgs a) { \
		stage_body<STAGE, 1>(d, a);                                                                         \
	}

// same launch site, private per-view arrays sized for MV views (strong update with S <= 8)
#define DVP_KERNEL_MV(NAME, STAGE, MINW, MV)                                                               \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME(const Dev d, const LaunchArgs a) {         \
		stage_body<STAGE, 0, MV>(d, a);                                                                     \
	}                                                                                                       \
	extern "C" __global__ void __launch_bounds__(256, MINW) NAME##_exact(const Dev d, const LaunchArgs a) { \
		stage_body<STAGE, 1, MV>(d, a);                                                                     \
	}

DVP_KERNEL(dvp_gen_edge_inform, DVP_ST_GEN_EDGE_INFORM, 1)
#ifndef DVP_LB_HEAVY
// min waves/SIMD the NCC kernels are compiled for: 2 = 256 VGPRs per lane (the pipelined 36-tap
// evaluation keeps 12 sixteen-byte gathers + the next 12 footprints live) and two 72 KiB patch
// tables per CU in LDS.
#define DVP_LB_HEAVY 2
#endif
DVP_KERNEL(dvp_random_init, DVP_ST_RANDOM_INIT, DVP_LB_HEAVY)
DVP_KERNEL(dvp_strong_update, DVP_ST_STRONG_UPDATE, DVP_LB_HEAVY)
DVP_KERNEL_MV(dvp_strong_update_v8, DVP_ST_STRONG_UPDATE, DVP_LB_HEAVY, kNarrowViews)
DVP_KERNEL_MV(dvp_strong_update_v16, DVP_ST_STRONG_UPDATE, DVP_LB_HEAVY, 16)
// split strong update (dvp_strong.hpp): evaluations of the 17 snapshot planes, decisions, refinement (S <= 16; S <= 31 with DVP_STRONG_WIDE)
DVP_KERNEL64(dvp_strong_eval, kStageStrongEval, DVP_LB_HEAVY)
// dvp_strong_eval with the (pixel, slot) items of the wave's 64 pixels compacted over its lanes.  With a pixel per lane a
// wave makes 17 trips x S views whatever its lanes hold: WEAK and off-image lanes idle, edge pixels have 9 slots instead of
// 17, and 11 % of the remaining planes are bitwise repeats of an earlier slot (strong_slot_sources) — 18 % of the lane-trips
// at cfg3.  Here every lane first builds its pixel's patch table (LDS, [tap][pixel]) and lists its distinct slots; the
// items are then numbered across the wave (prefix sum of the counts) and taken 64 per round: lane l evaluates item
// round * 64 + l = (pixel p, slot s) against the S views with p's table column and p's reference sums (fetched from the
// owner lane by ds_bpermute).  Same evaluations as strong_eval_px, hence the same bits.  LDS: 18 KB table + 1088 B of item
// list = 8 workgroups per CU, as before.
template <int SMP>
__device__ __forceinline__ void strong_eval_items_body(const Dev& d, const LaunchArgs& a) {
	const int lane = threadIdx.x;
	const int b = blockIdx.x;
	const int tile = (b >> 5) * 8 + (b & 7), wave = (b >> 3) & 3;
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	__shared__ uint8_t items[64 * kSlotCount];
	int px = 0, py = 0;
	bool active = block_to_pixel(tile, lane, wave, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py);
	if (active && d.weak_info[px + py * d.width] == DVP_WEAK) active = false;
	PatchCtx c;
	c.tab = PatchTab{&lds_tab[lane], 64};
	c.sum_ref = c.sum_ref_ref = c.wsum = 0.0f;
	c.radius = c.inc = c.fast = 0;
	uint32_t uniq = 0;
	if (active) {
		const int center = px + py * d.width;
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, c.tab, &c);
		if (d.reuse_hdr) uniq = d.reuse_hdr[center].eval;   // dvp_strong_plan has listed the slots and written their places
		else {
			uint32_t src[3], w[3];
			uniq = strong_slot_sources(d, center, src);
			strong_source_places(src, w);
			const size_t Lh = (size_t)d.half_w * (size_t)d.height;
			uint32_t* dup = reinterpret_cast<uint32_t*>(d.strong_rec) + half_index(d, px, py);
			dup[SR_DUP * Lh] = w[0]; dup[(SR_DUP + 1) * Lh] = w[1]; dup[(SR_DUP + 2) * Lh] = w[2];
		}
	}
	// Item order: pixel-major — all distinct slots of pixel 0, then pixel 1, ...; exclusive prefix sum of the lanes' item
	// counts.  (Rank-major — the first distinct slot of every pixel, then the second, ... — keeps neighbouring pixels with the
	// same direction's sample side by side like the pixel-per-lane kernel: L2 hit rate of the launch site 0.58 -> 0.84 and 65
	// -> 48 B of fabric traffic per evaluation, but the same time at cfg3 (467 vs 466 ms) and 3.8 % more at cfg2 (148 vs 143
	// ms): the kernel issues VALU instructions, it does not wait for lines, and the lanes of one pixel share its table column.)
	const int n = __popc(uniq);
	int incl = n;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int t = __shfl_up(incl, o, 64);
		if (lane >= o) incl += t;
	}
	const int off = incl - n;
	const int total = __shfl(incl, 63, 64);
	{
		int k = 0;
		for (uint32_t m = uniq; m; m &= m - 1, ++k) items[off + k] = (uint8_t)lane;
	}
	__syncthreads();
	unsigned long long cnt = 0;
	for (int i0 = 0; i0 < total; i0 += 64) {
		const bool valid = i0 + lane < total;
		const int i = valid ? i0 + lane : total - 1;   // the tail of the last round repeats its last item without storing
		const int pl = items[i];
		const int k = i - __shfl(off, pl, 64);
		uint32_t m = (uint32_t)__shfl((int)uniq, pl, 64);
		for (int j = 0; j < k; ++j) m &= m - 1;
		const int slot = dvp_ctz(m);
		PatchCtx ci;
		ci.tab = PatchTab{&lds_tab[pl], 64};
		ci.sum_ref = __shfl(c.sum_ref, pl, 64);
		ci.sum_ref_ref = __shfl(c.sum_ref_ref, pl, 64);
		ci.wsum = __shfl(c.wsum, pl, 64);
		ci.radius = __shfl(c.radius, pl, 64);
		ci.inc = __shfl(c.inc, pl, 64);
		ci.fast = __shfl(c.fast, pl, 64);
		const int ipx = __shfl(px, pl, 64), ipy = __shfl(py, pl, 64);
		strong_eval_item<SMP>(d, ci, ipx, ipy, slot, valid, d.eval_counter ? &cnt : nullptr);
	}
	if (d.eval_counter && cnt) atomicAdd(d.eval_counter, cnt);
}
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_strong_eval_items(const Dev d, const LaunchArgs a) { strong_eval_items_body<0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_strong_eval_items_exact(const Dev d, const LaunchArgs a) { strong_eval_items_body<1>(d, a); }
DVP_KERNEL64(dvp_strong_refine, kStageStrongRefine, DVP_LB_HEAVY)
DVP_KERNEL64(dvp_strong_refine_lanes, kStageStrongRefineLanes, DVP_LB_HEAVY)
template <int MV>
__device__ __forceinline__ void strong_decide_body(const Dev& d, const LaunchArgs& a) {
	int px, py;
	if (!block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py)) return;
	if (d.weak_info[px + py * d.width] != DVP_WEAK) strong_decide_px<MV>(d, px, py, a.iter);
}
// the cost vectors of the 8 directions live in registers: one instantiation per view-count bracket
// (4 waves per SIMD: the kernel waits for its cost loads 70 % of the time; 128 VGPRs cost the v10 instantiation 20 spilled registers and
// win 1.7 ms of 10 per cfg3 launch; 5 waves the same, 6 less)
#ifndef DVP_LB_DECIDE
#define DVP_LB_DECIDE 4
#endif
#define DVP_DECIDE_KERNEL(MV) extern "C" __global__ void __launch_bounds__(256, DVP_LB_DECIDE) dvp_strong_decide_v##MV(const Dev d, const LaunchArgs a) { strong_decide_body<MV>(d, a); }
// (Round 6 built the same decisions with the wave's 64 cost records staged in LDS by coalesced loads — 39 KB per wave at S = 9, i.e.
// four waves per CU: 17.8 ms per cfg3 launch against 8.0 for the plain loads below on the pixel-major records; removed,
// profiles/r06_ab_notes.txt.)
DVP_DECIDE_KERNEL(4)
DVP_DECIDE_KERNEL(6)
DVP_DECIDE_KERNEL(8)
DVP_DECIDE_KERNEL(10)
DVP_DECIDE_KERNEL(12)
DVP_DECIDE_KERNEL(16)
// any S <= 31 (DVP_STRONG_WIDE): the vectors are streamed in 16-byte pieces instead of held (strong_decide_wide_px)
extern "C" __global__ void __launch_bounds__(256, DVP_LB_DECIDE) dvp_strong_decide_wide(const Dev d, const LaunchArgs a) {
	int px, py;
	if (!block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py)) return;
	if (d.weak_info[px + py * d.width] != DVP_WEAK) strong_decide_wide_px(d, px, py, a.iter);
}
DVP_KERNEL(dvp_get_depth_normal, DVP_ST_GET_DEPTH_NORMAL, 1)
DVP_KERNEL(dvp_filter_strong, DVP_ST_FILTER_STRONG, 1)
DVP_KERNEL(dvp_depth_to_weak, DVP_ST_DEPTH_TO_WEAK, DVP_LB_HEAVY)
DVP_KERNEL(dvp_local_refine, DVP_ST_LOCAL_REFINE, DVP_LB_HEAVY)
DVP_KERNEL(dvp_depth_to_weak_refine, kStageSweeps, DVP_LB_HEAVY)   // the two sweeps in one launch (dvp_run_patchmatch)
// ... and the same launch site as view-compacted passes (dvp_sweep.hpp: sweep_*)
template <int WHAT>
__device__ __forceinline__ void sweep_light_body(const Dev& d, const LaunchArgs& a) {
	int px, py;
	if (!block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py)) return;
	if (WHAT != 0 && d.sweep_row1 > 0 && (py < d.sweep_row0 || py >= d.sweep_row1)) return;   // a band's decision pass
	if (WHAT == 0) sweep_prepare_px(d, px, py);
	else if (WHAT == 1) sweep_decide1_px(d, px, py);
	else sweep_decide2_px(d, px, py);
}
extern "C" __global__ void __launch_bounds__(256) dvp_sweep_prepare(const Dev d, const LaunchArgs a) { sweep_light_body<0>(d, a); }
extern "C" __global__ void __launch_bounds__(256) dvp_sweep_decide1(const Dev d, const LaunchArgs a) { sweep_light_body<1>(d, a); }
extern "C" __global__ void __launch_bounds__(256) dvp_sweep_decide2(const Dev d, const LaunchArgs a) { sweep_light_body<2>(d, a); }
// Evaluation pass, tile form (DVP_SWEEP_LIST=0, or no room for the lists below): workgroup = one wave = one 64 x kSweepRows (14)
// tile of the launch map, grid.y = source view (dispatched view after view: the workgroups in flight gather from ONE image).  The
// tile's pixels that take part — they selected the view with a weight > 0 — are compacted into a list in LDS (ballot ranks, row
// after row) and taken 64 per round, so that every lane of a round but the tile's last evaluates (71 % of the pixels select a given
// view at cfg3: 9.9 rounds of 64 instead of 14 rows with 29 % of the lanes idle).
// a.iter = stage (0: central window + LocalRefine's extra slot, 1: the rest of the line for pixels with a central peak).
// (a tile is 64 x kSweepRows pixels: dvp_forms.hpp)
template <int SMP, bool ALL>
__device__ __forceinline__ void sweep_eval_body(const Dev& d, const LaunchArgs& a) {
	const int lane = threadIdx.x;
	const int v = blockIdx.y;
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	__shared__ uint16_t list[64 * kSweepRows];   // tile-local pixel index (row * 64 + x): 18 KB + 2 KB = 8 workgroups per CU
	__shared__ DvpCamera cams[2];                // reference camera, camera of the launch's view
	const PatchTab tab{&lds_tab[lane], 64};
	static_assert(sizeof(DvpCamera) == 112, "28 dwords");
	if (lane < 56) {
		const int which = lane >= 28 ? 1 : 0;
		reinterpret_cast<uint32_t*>(&cams[which])[lane - 28 * which] = reinterpret_cast<const uint32_t*>(d.cameras + (which ? v + 1 : 0))[lane - 28 * which];
	}
	// tile of this workgroup: the strip map of block_to_pixel (XCD b % 8 owns a column of a strip of 8 tile columns) over
	// tiles of kSweepRows rows; a.tiles_x / a.tiles = that grid
	const int tiles_y = a.tiles / a.tiles_x;
	int tx, ty;
	{
		const int per_strip = 8 * tiles_y;
		const int st = (int)blockIdx.x / per_strip, rem = (int)blockIdx.x - st * per_strip;
		const int w_last = a.tiles_x - st * 8;
		if (w_last >= 8) { ty = rem >> 3; tx = st * 8 + (rem & 7); }
		else { ty = rem / w_last; tx = st * 8 + (rem - ty * w_last); }
	}
	ty += a.rows;   // first tile row of the launch (a band of the image; 0: all of it)
	const int x = tx * 64 + lane;
	int n = 0;
	for (int r = 0; r < kSweepRows; ++r) {
		const int y = ty * kSweepRows + r;
		const bool go = x < d.width && y < d.height && sweep_go(d, x + y * d.width, v, a.iter);
		const unsigned long long m = __ballot(go);
		if (go) list[n + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(r * 64 + lane);
		n += __popcll(m);
	}
	__syncthreads();
	unsigned long long cnt = 0;
	for (int i0 = 0; i0 < n; i0 += 64) {
		if (i0 + lane < n) {
			const int e = list[i0 + lane];
			sweep_eval_px<SMP, ALL>(d, tx * 64 + (e & 63), ty * kSweepRows + (e >> 6), v, a.iter, tab, d.eval_counter ? &cnt : nullptr, cams);
		}
	}
	if (d.eval_counter && cnt) atomicAdd(d.eval_counter, cnt);
}
// The 6-pixel frame of the view-compacted form (UNKNOWN for DepthToWeak, a full LocalRefine: the fused kernel's per-pixel
// code) over the frame's pixels only: lane t of the launch = the t-th frame pixel (6 rows on top, 6 at the bottom, 2 x 6
// columns between them).  The full-grid launch kept 8 800 waves resident for 6 active lanes each at 6208 x 4128 (6.6 ms).
template <int SMP>
__device__ __forceinline__ void sweep_border_body(const Dev& d, const LaunchArgs& a) {
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	const PatchTab tab{&lds_tab[threadIdx.x], 64};
	const int W = d.width, H = d.height;
	const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
	int px, py;
	if (t < 12ll * W) {
		const int r = (int)(t / W);
		px = (int)(t - (long long)r * W);
		py = r < 6 ? r : H - 12 + r;
	} else {
		const long long u = t - 12ll * W;
		const int r = (int)(u / 12), cidx = (int)(u - 12ll * r);
		if (r >= H - 12) return;
		py = 6 + r;
		px = cidx < 6 ? cidx : W - 12 + cidx;
	}
	unsigned long long n = 0;
	run_pixel<kStageSweeps, SMP>(d, px, py, kSweepBorderOnly, d.eval_counter ? &n : nullptr, tab);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_border(const Dev d, const LaunchArgs a) { sweep_border_body<0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_border_exact(const Dev d, const LaunchArgs a) { sweep_border_body<1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval(const Dev d, const LaunchArgs a) { sweep_eval_body<0, false>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_exact(const Dev d, const LaunchArgs a) { sweep_eval_body<1, false>(d, a); }
// DVP_SWEEP_ALL_SLOTS=1 (A/B): the same with the two end slots of the line, which no decision reads (dvp_forms.hpp: sweep_slot_read)
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_all(const Dev d, const LaunchArgs a) { sweep_eval_body<0, true>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_exact_all(const Dev d, const LaunchArgs a) { sweep_eval_body<1, true>(d, a); }

// ---- the same evaluations from per-view (pixel, view) lists (DVP_SWEEP_LIST; dvp_sweep_list.hpp) ----
// The lists of stage a.iter over the launch's tiles (a.tiles_x, a.tiles, a.rows as for dvp_sweep_eval): one wave per tile, lane =
// column of the tile; lane v < S keeps view v's running count / offset.
extern "C" __global__ void __launch_bounds__(256) dvp_sweep_list_counts(const Dev d, const LaunchArgs a) {
	const int lane = threadIdx.x & 63;
	const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= a.tiles) return;
	const int S = d.params.num_images - 1;
	int tx, ty;
	sweep_list_tile(t, a.tiles_x, a.tiles / a.tiles_x, &tx, &ty);
	ty += a.rows;
	const int x = tx * 64 + lane;
	int cnt = 0;
	for (int r = 0; r < kSweepRows; ++r) {
		const int y = ty * kSweepRows + r;
		const uint32_t m = (x < d.width && y < d.height) ? sweep_go_mask(d, x + y * d.width, a.iter) : 0u;
		if (__ballot(m != 0) == 0) continue;
		for (int v = 0; v < S; ++v) {
			const int k = __popcll(__ballot((m >> v) & 1u));
			if (lane == v) cnt += k;
		}
	}
	if (lane < S) d.sweep_list_counts[(size_t)lane * a.tiles + t] = cnt;
}
// (between the two: dvp_scan3 over each view's counts; its totals are the lists' lengths, d.sweep_list_n)
extern "C" __global__ void __launch_bounds__(256) dvp_sweep_list_fill(const Dev d, const LaunchArgs a) {
	const int lane = threadIdx.x & 63;
	const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= a.tiles) return;
	const int S = d.params.num_images - 1;
	int tx, ty;
	sweep_list_tile(t, a.tiles_x, a.tiles / a.tiles_x, &tx, &ty);
	ty += a.rows;
	const int x = tx * 64 + lane;
	int off = lane < S ? d.sweep_list_counts[(size_t)lane * a.tiles + t] : 0;
	for (int r = 0; r < kSweepRows; ++r) {
		const int y = ty * kSweepRows + r;
		const uint32_t m = (x < d.width && y < d.height) ? sweep_go_mask(d, x + y * d.width, a.iter) : 0u;
		if (__ballot(m != 0) == 0) continue;
		for (int v = 0; v < S; ++v) {
			const unsigned long long b = __ballot((m >> v) & 1u);
			sweep_list_put(d.sweep_list + (size_t)v * d.sweep_list_cap, __shfl(off, v, 64), b, lane, x, y);
			if (lane == v) off += __popcll(b);
		}
	}
}
// Evaluation pass from the lists: workgroup = one wave = R consecutive rounds of 64 entries of the list of view blockIdx.y (a chunk:
// sweep_list_chunk).  The grid is the upper bound over the list's room; the length stays on the device, and a workgroup past the
// end leaves after one scalar load.  Only the last round of a view's list can be part-empty.  a.iter = stage, as above.
template <int SMP, bool ALL, int R>
__device__ __forceinline__ void sweep_eval_list_body(const Dev& d, const LaunchArgs& a) {
	const int lane = threadIdx.x;
	const int v = blockIdx.y;
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	__shared__ DvpCamera cams[2];                // reference camera, camera of the launch's view
	const int n = d.sweep_list_n[v];
	const int chunk = sweep_list_chunk((int)blockIdx.x, n, R);
	if (chunk < 0) return;
	const PatchTab tab{&lds_tab[lane], 64};
	static_assert(sizeof(DvpCamera) == 112, "28 dwords");
	if (lane < 56) {
		const int which = lane >= 28 ? 1 : 0;
		reinterpret_cast<uint32_t*>(&cams[which])[lane - 28 * which] = reinterpret_cast<const uint32_t*>(d.cameras + (which ? v + 1 : 0))[lane - 28 * which];
	}
	__syncthreads();
	const uint32_t* list = d.sweep_list + (size_t)v * d.sweep_list_cap;
	const int first = chunk * (64 * R), end = DVP_MIN(n, first + 64 * R);
	unsigned long long cnt = 0;
	for (int i0 = first; i0 < end; i0 += 64) {
		if (i0 + lane < end) {
			const uint32_t e = list[i0 + lane];
			sweep_eval_px<SMP, ALL>(d, sweep_list_x(e), sweep_list_y(e), v, a.iter, tab, d.eval_counter ? &cnt : nullptr, cams);
		}
	}
	if (d.eval_counter && cnt) atomicAdd(d.eval_counter, cnt);
}
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_list(const Dev d, const LaunchArgs a) { sweep_eval_list_body<0, false, kSweepListRounds>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_list_exact(const Dev d, const LaunchArgs a) { sweep_eval_list_body<1, false, kSweepListRounds>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_list_all(const Dev d, const LaunchArgs a) { sweep_eval_list_body<0, true, kSweepListRounds>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_HEAVY) dvp_sweep_eval_list_exact_all(const Dev d, const LaunchArgs a) { sweep_eval_list_body<1, true, kSweepListRounds>(d, a); }

// the weak-path launch sites: one lane per entry of the WEAK-pixel list
DVP_KERNEL_LIST(dvp_find_nearest_strong_list, DVP_ST_FIND_NEAREST_STRONG, 1)
// GenNeighbours' directional search: one lane per WEAK pixel, the list of found points in LDS (one column per lane)
extern "C" __global__ void __launch_bounds__(256) dvp_gen_neighbours_list(const Dev d, const ListArgs a) {
	__shared__ s2 pts[kGnDirSlots * 256];
	const int t = list_block(blockIdx.x, gridDim.x, kListRun) * 256 + threadIdx.x;
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const int py = center / d.width, px = center - py * d.width;
	gen_neighbours_px(d, px, py, pts + threadIdx.x, 256);
}
DVP_KERNEL_LIST(dvp_neighbour_update_list, DVP_ST_NEIGHBOUR_UPDATE, 1)
DVP_KERNEL_LIST(dvp_ransac_fit_plane_list, DVP_ST_RANSAC_FIT, 1)
// ... and the same launch site with one wave per WEAK pixel, lane = draw (dvp_ransac.hpp: ransac_fit_plane_wave; DVP_RANSAC_WAVE=1 —
// measured no faster than the lane kernel, whose 0.18 lane utilisation turns out not to be what it waits for: kept as the record of that)
extern "C" __global__ void __launch_bounds__(64) dvp_ransac_fit_plane_wave(const Dev d, const ListArgs a) {
	__shared__ RansacShared sh[1];
	const int t = list_block(blockIdx.x, gridDim.x, kWaveRun * 4);
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const int py = center / d.width, px = center - py * d.width;
	ransac_fit_plane_wave(d, px, py, a.iter, sh[0]);
}

// Black/RedPixelUpdateWeak (APD.cu:4487-4489): one WAVE per WEAK pixel of the list segment, per-pixel state in LDS
// (dvp_weak_wave.hpp)
template <int SMP, int FMT, int TAB>
__device__ __forceinline__ void weak_wave_body(const Dev& d, const ListArgs& a) {
	// one wave = one WEAK pixel = one workgroup (10 KB of LDS): with four pixels per workgroup the LDS of a finished pixel waited
	// for the slowest of the four (weak update 400 -> 376 ms per cfg3 pass); the XCD runs keep their length in pixels
	__shared__ WeakSharedT<TAB> sh[1];
	const int wave = 0;
	const int t = list_block(blockIdx.x, gridDim.x, kWaveRun * 4);
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const int py = center / d.width, px = center - py * d.width;
	if (py >= a.covered_rows) return;   // rows beyond the reference's half grid (APD.cu:4421-4424)
	if (d.weak_info[center] != DVP_WEAK) return;   // NeigbourUpdate turned it UNKNOWN since the list was built (APD.cu:3119-3123)
	unsigned long long n = 0;
	weak_update_wave<SMP, FMT, TAB>(d, px, py, a.iter, d.eval_counter ? &n : nullptr, sh[wave]);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
// first half of GenNeighbours (directional anchor search + label extension): one wave per WEAK pixel, the tries of a
// direction over the lanes (dvp_neighbours.hpp: gen_neighbours_search_wave)
#ifndef DVP_LB_GN
#define DVP_LB_GN 8   // waves per SIMD (64 VGPRs + 164 B scratch; measured 86 ms per cfg3 pass, 4 waves without scratch: 105 ms)
#endif
extern "C" __global__ void __launch_bounds__(256, DVP_LB_GN) dvp_gen_neighbours_search(const Dev d, const ListArgs a) {
	__shared__ GnShared sh[4];
	const int wave = threadIdx.x >> 6;
	const int t = list_block(blockIdx.x, gridDim.x, kWaveRun) * 4 + wave;
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	if (d.weak_info[center] != DVP_WEAK) return;
	const int py = center / d.width, px = center - py * d.width;
	gen_neighbours_search_wave(d, px, py, sh[wave]);
}
// second half of GenNeighbours (RANSAC plane + ranking): one wave per WEAK pixel, point tables in LDS
// (3 workgroups per CU is what the 12.6 KB of LDS per wave allow; stated, the compiler fits the kernel in 108 VGPRs, left alone it takes 179: 2 waves per SIMD)
extern "C" __global__ void __launch_bounds__(64, 3) dvp_gen_neighbours_fit(const Dev d, const ListArgs a) {
	__shared__ FitShared sh[1];   // (one wave per workgroup, as the weak update: 65 -> 59 ms per cfg3 launch)
	const int wave = 0;
	const int t = list_block(blockIdx.x, gridDim.x, kWaveRun * 4);
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	if (d.weak_info[center] != DVP_WEAK) return;
	const int py = center / d.width, px = center - py * d.width;
	gen_neighbours_fit_wave(d, px, py, sh[wave]);
}

#ifndef DVP_LB_WEAK
#define DVP_LB_WEAK 4   // waves per SIMD the wave kernel is compiled for (LDS: 34 KB per workgroup -> 4 workgroups per CU; 128 VGPRs)
#endif
// (no suffix: the anchor sub-patches' reference side comes from the pass' table, Dev::anchor_tab; _notab: formed per item —
// the definition, used when the table does not fit or DVP_WEAK_ANCHOR_TAB=0)
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave(const Dev d, const ListArgs a) { weak_wave_body<0, 0, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact(const Dev d, const ListArgs a) { weak_wave_body<1, 0, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_notab(const Dev d, const ListArgs a) { weak_wave_body<0, 0, 0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact_notab(const Dev d, const ListArgs a) { weak_wave_body<1, 0, 0>(d, a); }
// the same launch site reading the byte planes (Dev::images8: all images 8-bit exact)
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_u8(const Dev d, const ListArgs a) { weak_wave_body<0, 1, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact_u8(const Dev d, const ListArgs a) { weak_wave_body<1, 1, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_u8_notab(const Dev d, const ListArgs a) { weak_wave_body<0, 1, 0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact_u8_notab(const Dev d, const ListArgs a) { weak_wave_body<1, 1, 0>(d, a); }
// ... and the binary16 planes (Dev::images16: down-sampled levels of 8-bit images)
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_f16(const Dev d, const ListArgs a) { weak_wave_body<0, 2, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact_f16(const Dev d, const ListArgs a) { weak_wave_body<1, 2, 1>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_f16_notab(const Dev d, const ListArgs a) { weak_wave_body<0, 2, 0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) dvp_weak_update_wave_exact_f16_notab(const Dev d, const ListArgs a) { weak_wave_body<1, 2, 0>(d, a); }
// The same launch site as EIGHT launches (dvp_weak_phased.hpp): the evaluation launches E0 / E1 / E2a / E2b take one wave per
// GROUP of a.group consecutive WEAK pixels of the list, the per-pixel decisions D1 / D2 / D3 and the final plain-NCC cost E3
// run one LANE per WEAK pixel.
template <int SMP, int FMT, int MODE>
__device__ __forceinline__ void weak_group_body(const Dev& d, const ListArgs& a) {
	constexpr int GRP = MODE == 0 ? kGrpWide : kGrp;
	__shared__ WeakGroupSharedT<GRP> sh;
	const int G = a.group < GRP ? a.group : GRP;
	const int run = a.run / G;          // XCD runs of a.run pixels (the one-wave kernel's: kWaveRun * 4)
	const int blk = list_block(blockIdx.x, gridDim.x, run < 1 ? 1 : run);
	if (blk * G >= a.count) return;
	if (threadIdx.x < (unsigned)GRP) {
		const int t = blk * G + (int)threadIdx.x;
		int center = -1;
		if ((int)threadIdx.x < G && t < a.count) {
			center = d.weak_list[a.base + t];
			// rows beyond the reference's half grid (APD.cu:4421-4424); NeigbourUpdate turned it UNKNOWN since the list was built (APD.cu:3119-3123)
			if (center / d.width >= a.covered_rows || d.weak_info[center] != DVP_WEAK) center = -1;
		}
		sh.center[threadIdx.x] = center;
	}
	wave_sync();
	unsigned long long n = 0;
	weak_group_eval<SMP, FMT, MODE, GRP>(d, G, d.eval_counter ? &n : nullptr, sh);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
#define DVP_WEAK_PHASE_KERNELS(NAME, MODE)                                                                                                              \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME(const Dev d, const ListArgs a) { weak_group_body<0, 0, MODE>(d, a); }           \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME##_exact(const Dev d, const ListArgs a) { weak_group_body<1, 0, MODE>(d, a); }   \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME##_u8(const Dev d, const ListArgs a) { weak_group_body<0, 1, MODE>(d, a); }      \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME##_exact_u8(const Dev d, const ListArgs a) { weak_group_body<1, 1, MODE>(d, a); }    \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME##_f16(const Dev d, const ListArgs a) { weak_group_body<0, 2, MODE>(d, a); }     \
	extern "C" __global__ void __launch_bounds__(64, DVP_LB_WEAK) NAME##_exact_f16(const Dev d, const ListArgs a) { weak_group_body<1, 2, MODE>(d, a); }
DVP_WEAK_PHASE_KERNELS(dvp_weak_eval_candidates, 0)
DVP_WEAK_PHASE_KERNELS(dvp_weak_eval_planes, 1)
DVP_WEAK_PHASE_KERNELS(dvp_weak_eval_first_view, 2)
DVP_WEAK_PHASE_KERNELS(dvp_weak_eval_survivors, 3)
template <int PART>
__device__ __forceinline__ void weak_phase_lane_body(const Dev& d, const ListArgs& a) {
	const int t = list_block(blockIdx.x, gridDim.x, kListRun) * 256 + threadIdx.x;
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const int py = center / d.width, px = center - py * d.width;
	if (py >= a.covered_rows) return;
	if (d.weak_info[center] != DVP_WEAK) return;
	if (PART == 0) weak_d1_px(d, px, py, a.iter);
	else if (PART == 1) weak_d2_px(d, px, py, a.iter);
	else weak_d3_px(d, px, py);
}
#ifndef DVP_LB_WEAK_DECIDE
#define DVP_LB_WEAK_DECIDE 2   // 256-lane workgroups per SIMD... (waves per SIMD = this; the kernels wait for scattered loads)
#endif
extern "C" __global__ void __launch_bounds__(256, DVP_LB_WEAK_DECIDE) dvp_weak_select_views(const Dev d, const ListArgs a) { weak_phase_lane_body<0>(d, a); }
extern "C" __global__ void __launch_bounds__(256, DVP_LB_WEAK_DECIDE) dvp_weak_make_hypotheses(const Dev d, const ListArgs a) { weak_phase_lane_body<1>(d, a); }
extern "C" __global__ void __launch_bounds__(256, DVP_LB_WEAK_DECIDE) dvp_weak_adopt(const Dev d, const ListArgs a) { weak_phase_lane_body<2>(d, a); }
// E3: the per-lane evaluator of the strong path over the WEAK list (one-wave workgroups, 18 KB of patch table each)
template <int SMP>
__device__ __forceinline__ void weak_final_cost_body(const Dev& d, const ListArgs& a) {
	__shared__ f2 lds_tab[kTaps * kTaps * 64];
	const PatchTab tab{&lds_tab[threadIdx.x], 64};
	const int t = list_block(blockIdx.x, gridDim.x, kListRun * 4) * 64 + threadIdx.x;
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const int py = center / d.width, px = center - py * d.width;
	if (py >= a.covered_rows) return;
	if (d.weak_info[center] != DVP_WEAK) return;
	unsigned long long n = 0;
	weak_final_cost_px<SMP>(d, px, py, tab, d.eval_counter ? &n : nullptr);
	if (d.eval_counter && n) atomicAdd(d.eval_counter, n);
}
extern "C" __global__ void __launch_bounds__(64, 2) dvp_weak_final_cost(const Dev d, const ListArgs a) { weak_final_cost_body<0>(d, a); }
extern "C" __global__ void __launch_bounds__(64, 2) dvp_weak_final_cost_exact(const Dev d, const ListArgs a) { weak_final_cost_body<1>(d, a); }

// the pass' table of anchor reference sides: thread = (WEAK list entry, view, anchor), anchor fastest (neighbouring lanes write
// neighbouring 128-byte records)
extern "C" __global__ void __launch_bounds__(256) dvp_weak_anchor_table(const Dev d, const ListArgs a) {
	const int S = d.params.num_images - 1;
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= (long long)a.count * S * kAnchors) return;
	const int k = (int)(i % kAnchors);
	const long long r = i / kAnchors;
	const int v0 = (int)(r % S);
	const int t = (int)(r / S);
	// (the records written through an LDS transpose — eight whole records per store instruction instead of 16 bytes into each of
	// 64 lines — measure the same 19 ms per cfg3 pass: the launch does not wait for its stores)
	if (d.images8) build_anchor_record<1>(d, d.weak_list[a.base + t], v0, k);
	else if (d.images16) build_anchor_record<2>(d, d.weak_list[a.base + t], v0, k);
	else build_anchor_record<0>(d, d.weak_list[a.base + t], v0, k);
}

// replicate the image border into the kImgPad-wide frame of a padded plane set
extern "C" __global__ void dvp_pad_replicate(float* planes, int W, int H, int pitch, size_t plane_stride, int n_planes) {
	const int PW = W + 2 * kImgPad, PH = H + 2 * kImgPad;
	const int frame = 2 * kImgPad * PW + 2 * kImgPad * H;   // border cells per plane
	const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= (long long)frame * n_planes) return;
	const int pl = (int)(t / frame);
	int k = (int)(t - (long long)pl * frame);
	int x, y;
	if (k < 2 * kImgPad * PW) {           // top and bottom bands
		y = k / PW;
		x = k - y * PW;
		if (y >= kImgPad) y += H;
	} else {                              // left and right bands of the interior rows
		k -= 2 * kImgPad * PW;
		y = kImgPad + k / (2 * kImgPad);
		x = k % (2 * kImgPad);
		if (x >= kImgPad) x += W;
	}
	float* p = planes + (size_t)pl * plane_stride;
	const int sx = clampi(x - kImgPad, 0, W - 1) + kImgPad, sy = clampi(y - kImgPad, 0, H - 1) + kImgPad;
	p[(size_t)y * pitch + x] = p[(size_t)sy * pitch + sx];
}

// plain padded planes -> row-pair planes: out[(y*pitch + x)*2 + {0,1}] = {in[y][x], in[y+1][x]}
// (the last padded row pairs with itself; the sampler never reads its second component)
extern "C" __global__ void dvp_interleave_rows(const float* __restrict__ in, float* __restrict__ out, int PH, int pitch, size_t plane_stride, int n_planes) {
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = blockIdx.y;
	const int pl = blockIdx.z;
	if (x >= pitch) return;
	const float* p = in + (size_t)pl * plane_stride;
	const int y1 = y + 1 < PH ? y + 1 : y;
	const float2 v = make_float2(p[(size_t)y * pitch + x], p[(size_t)y1 * pitch + x]);
	reinterpret_cast<float2*>(out + (size_t)pl * plane_stride * 2)[(size_t)y * pitch + x] = v;
}

// row-pair float planes -> tiled byte planes (Dev::images8), and the format probe of the upload: *inexact collects the bits of
// tile_pair_rule (dvp_dev.hpp) over every element — bit 0: some texel is not an integer in [0, 255] (no byte planes), bit 1: some
// texel is not a binary16 value in [0, 255] (no binary16 planes either).
// One thread per tile element: tile (tx, ty), element (ex, ey) = padded pixel (tx*7 + ex, ty*8 + ey), clamped to the
// padded plane (the right-most column of a tile repeats the first pixel of the next tile).
extern "C" __global__ void dvp_pairs_to_tiles(const float* __restrict__ pairs, uint8_t* __restrict__ out, int PW, int PH, int pitch, size_t plane_stride,
                                              int tiles_x, int tiles_y, int n_planes, int* inexact) {
	const size_t per_plane = (size_t)tiles_x * tiles_y * 64;
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= per_plane * n_planes) return;
	const int pl = (int)(i / per_plane);
	const size_t r = i - (size_t)pl * per_plane;
	const int tile = (int)(r >> 6), e = (int)(r & 63);
	const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
	const int sx = min(tx * kT8W + (e % kT8E), PW - 1), sy = min(ty * kT8H + (e / kT8E), PH - 1);
	if (e >= kT8E * kT8H) return;
	const float* plane = pairs + (size_t)pl * plane_stride * 2;
	const float2 v = reinterpret_cast<const float2*>(plane)[(size_t)sy * pitch + sx];
	const float2 u = reinterpret_cast<const float2*>(plane)[(size_t)sy * pitch + min(sx + 1, PW - 1)];
	uint32_t h;
	const unsigned bad = tile_pair_rule(v.x, v.y, &h);
	if (bad) {
		if ((*inexact & bad) != bad) atomicOr(inexact, (int)bad);
		if (bad & 1u) return;
	}
	uint8_t* dst = out + ((size_t)pl * tiles_x * tiles_y + tile) * 128 + (size_t)e * kT8B;
	dst[0] = (uint8_t)v.x;
	dst[1] = (uint8_t)v.y;
	if (kT8Quad) { dst[2] = (uint8_t)u.x; dst[3] = (uint8_t)u.y; }
}

// row-pair float planes -> tiled binary16 planes (Dev::images16), after dvp_pairs_to_tiles found every texel binary16-exact.
// One thread per tile element: tile (tx, ty), element (ex, ey) = padded pixel (tx*7 + ex, ty*4 + ey), clamped to the padded plane.
extern "C" __global__ void dvp_pairs_to_tiles16(const float* __restrict__ pairs, uint32_t* __restrict__ out, int PW, int PH, int pitch, size_t plane_stride,
                                                int tiles_x, int tiles_y, int n_planes) {
	constexpr int kPer = kT16E * kT16H;   // 32 elements per tile
	const size_t per_plane = (size_t)tiles_x * tiles_y * kPer;
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= per_plane * n_planes) return;
	const int pl = (int)(i / per_plane);
	const size_t r = i - (size_t)pl * per_plane;
	const int tile = (int)(r / kPer), e = (int)(r % kPer);
	const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
	const int sx = min(tx * kT16W + (e % kT16E), PW - 1), sy = min(ty * kT16H + (e / kT16E), PH - 1);
	const float2 v = reinterpret_cast<const float2*>(pairs + (size_t)pl * plane_stride * 2)[(size_t)sy * pitch + sx];
	uint32_t h;
	(void)tile_pair_rule(v.x, v.y, &h);
	out[((size_t)pl * tiles_x * tiles_y + tile) * (128 / 4) + e] = h;
}

// byte edge map -> 32x32 bit tiles (one thread per 32-bit word)
extern "C" __global__ void dvp_pack_edge_bits(const uint8_t* __restrict__ edge, uint32_t* __restrict__ bits, int W, int H, int tiles_x, size_t words, int equals) {
	const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (w < words) bits[w] = pack_edge_word(edge, W, H, tiles_x, w, equals);
}

// visibility-prior candidates of GenEdgeInform: pixels x source views (blockIdx.y = view, wave-uniform)
extern "C" __global__ void __launch_bounds__(256) dvp_gen_candidates(const Dev d, const LaunchArgs a) {
	int px, py;
	if (block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py))
		gen_candidates_px(d, px, py, (int)blockIdx.y);
}

// all views of a pixel by one lane (gen_candidates_views_px: the tap weights once instead of once per view)
extern "C" __global__ void __launch_bounds__(256) dvp_gen_candidates_views(const Dev d, const LaunchArgs a) {
	int px, py;
	if (block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py))
		gen_candidates_views_px<kCandGroup>(d, px, py, (int)blockIdx.y * kCandGroup);
}
extern "C" __global__ void __launch_bounds__(256) dvp_gen_candidates_views_list(const Dev d, const unsigned* list, const unsigned* n_list) {
	const unsigned t = blockIdx.x * 256 + threadIdx.x;
	if (t >= *n_list) return;
	const int center = (int)list[t];
	const int py = center / d.width, px = center - py * d.width;
	gen_candidates_views_px<kCandGroup>(d, px, py, (int)blockIdx.y * kCandGroup);
}

// ... and the same for the ANCHOR pixels only (dvp_run_patchmatch).  The weak update is the records' one reader, and it reads
// them at the anchors of WEAK pixels (make_anchor_record, wave_ncc_new: the anchor's eight offsets per view, APD.cu:938-952) —
// after GenNeighbours that is a few percent of the image where the reference's GenEdgeInform fills every pixel x view (52 ms
// of side-stream work at 6208x4128, S = 9).  Three launches: mark the anchors of the WEAK list, compact the marks into a
// list (any order), one lane per (listed pixel, view).  They read the selected-view map as GenEdgeInform saw it (a snapshot
// taken before RandomInitialization rewrites it), so the records are those of the full launch.
extern "C" __global__ void __launch_bounds__(256) dvp_anchor_mask(const Dev d, const ListArgs a, uint8_t* mask) {
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= a.count) return;
	const int center = d.weak_list[a.base + t];
	const s2* nb = d.neighbours + (size_t)d.neighbours_map[center] * DVP_NEIGHBOUR_NUM;
	for (int k = 1; k < DVP_NEIGHBOUR_NUM; ++k) {
		const s2 q = nb[k];
		if (q.x >= 0 && q.y >= 0 && q.x < d.width && q.y < d.height) mask[(size_t)q.y * d.width + q.x] = 1;
	}
}
extern "C" __global__ void __launch_bounds__(256) dvp_mask_compact(const uint8_t* mask, size_t L, unsigned* list, unsigned* n_list) {
	const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool go = p < L && mask[p] != 0;
	const unsigned long long m = __ballot(go);
	if (!m) return;
	const int lane = threadIdx.x & 63;
	unsigned base = 0;
	if (lane == __builtin_ctzll(m)) base = atomicAdd(n_list, (unsigned)__popcll(m));
	base = __shfl(base, __builtin_ctzll(m), 64);
	if (go) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned)p;
}
extern "C" __global__ void __launch_bounds__(256) dvp_gen_candidates_list(const Dev d, const unsigned* list, const unsigned* n_list) {
	const unsigned t = blockIdx.x * 256 + threadIdx.x;
	if (t >= *n_list) return;
	const int center = (int)list[t];
	const int py = center / d.width, px = center - py * d.width;
	gen_candidates_px(d, px, py, (int)blockIdx.y);
}

extern "C" __global__ void dvp_pack_bits_transposed(const uint8_t* __restrict__ map, uint32_t* __restrict__ bits, int W, int H, int tiles_x, size_t words, int equals) {
	const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (w < words) bits[w] = pack_edge_word_t(map, W, H, tiles_x, w, equals);
}

// cell table of the edge map (edge_count_upper): counts per 8x8 cell from the bit tiles, then the two prefix passes
extern "C" __global__ void dvp_edge_cell_counts(const Dev d) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= d.sat_cells_x * d.sat_cells_y) return;
	const int cy = c / d.sat_cells_x, cx = c - cy * d.sat_cells_x;
	int n = 0;
	for (int r = 0; r < 8; ++r) {
		const int y = cy * 8 + r;
		if (y >= d.height) break;
		const unsigned w = d.edge_bits[(size_t)(((y >> 5) * d.edge_tiles_x + (cx >> 2)) * 32 + (y & 31))];
		n += __popc((w >> ((cx & 3) * 8)) & 255u);
	}
	d.edge_sat[(cy + 1) * (d.sat_cells_x + 1) + cx + 1] = n;
}
extern "C" __global__ void dvp_edge_sat_rows(const Dev d) {   // one thread per table row: running sum along x
	const int r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > d.sat_cells_y) return;
	int* row = d.edge_sat + (size_t)r * (d.sat_cells_x + 1);
	int acc = 0;
	for (int x = 0; x <= d.sat_cells_x; ++x) { acc += (r == 0 || x == 0) ? 0 : row[x]; row[x] = acc; }
}
extern "C" __global__ void dvp_edge_sat_cols(const Dev d) {   // one thread per table column: running sum along y
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x > d.sat_cells_x) return;
	const int P = d.sat_cells_x + 1;
	int acc = 0;
	for (int r = 0; r <= d.sat_cells_y; ++r) { acc += d.edge_sat[(size_t)r * P + x]; d.edge_sat[(size_t)r * P + x] = acc; }
}

// sample search of the strong update (same red/black launch geometry, no LDS, small register footprint)
extern "C" __global__ void __launch_bounds__(256) dvp_strong_search(const Dev d, const LaunchArgs a) {
	int px, py;
	if (block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py))
		strong_search_px(d, px, py);
}

// plane-cache plan of the split strong update (strong_reuse_plan): which of the pixel's planes still have their vector from its
// previous visit, and where every slot's vector lies.  Light like the search, so that the 256-VGPR evaluation kernel only reads the result.
extern "C" __global__ void __launch_bounds__(256) dvp_strong_plan(const Dev d, const LaunchArgs a) {
	int px, py;
	if (block_to_pixel(blockIdx.x, threadIdx.x & 63, threadIdx.x >> 6, a.tiles_x, a.tiles, a.rows, a.half, a.colour, d.width, d.height, &px, &py) &&
	    d.weak_info[px + py * d.width] != DVP_WEAK)
		strong_plan_px(d, px, py);
}

// line-scan pre-pass of GenEdgeInform: nearest edge pixel in 8 directions (blockIdx.y = direction)
extern "C" __global__ void __launch_bounds__(256) dvp_edge_rays(const Dev d, int what) {
	edge_ray_line(d, blockIdx.y, blockIdx.x * blockDim.x + threadIdx.x, what);
}

// ---- WEAK-pixel bookkeeping on the device (dvp_upload_state) -------------------------------------------------
// neighbours_map (running index of WEAK pixels in raster order, APD.cpp:1182-1193) and the compacted WEAK list of the
// list kernels used to be built by serial host loops over all L pixels per pass (25.6 M at full resolution: 0.2 s, plus a
// 26 MB download when the weak map was already on the device).  Three small launches instead: ballot counts per unit,
// one exclusive scan, ballot-rank scatter.
// List order: 64 x 64 super-tiles row-major over the image, 16 x 16 tiles row-major inside them, rows inside those; black
// ((x + y) even) pixels first, then red.  "Slot" = (super-tile, tile position 0..15); a slot outside the image counts zero.
constexpr int kWeakTile = 16, kWeakSuper = 64, kWeakChunk = 1024;   // raster chunk of the neighbours_map scan
DVP_HD void weak_slot_origin(int slot, int supers_x, int* tx, int* ty) {
	const int super = slot >> 4, t = slot & 15;
	*tx = (super % supers_x) * kWeakSuper + (t & 3) * kWeakTile;
	*ty = (super / supers_x) * kWeakSuper + (t >> 2) * kWeakTile;
}
// one wave per slot: counts[slot] = black WEAK pixels, counts[n_slots + slot] = red ones;
// one wave per raster chunk: counts[2 * n_slots + chunk] = WEAK pixels of the chunk
extern "C" __global__ void __launch_bounds__(256) dvp_weak_counts(const uint8_t* __restrict__ weak, int W, int H, int supers_x, int n_slots, int n_chunks, int* __restrict__ counts) {
	const int lane = threadIdx.x & 63;
	const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (unit < n_slots) {
		int tx, ty;
		weak_slot_origin(unit, supers_x, &tx, &ty);
		int nb = 0, nr = 0;
		for (int step = 0; step < 4; ++step) {
			const int x = tx + (lane & 15), y = ty + step * 4 + (lane >> 4);
			const bool wk = x < W && y < H && weak[(size_t)y * W + x] == DVP_WEAK;
			nb += __popcll(__ballot(wk && !((x + y) & 1)));
			nr += __popcll(__ballot(wk && ((x + y) & 1)));
		}
		if (lane == 0) { counts[unit] = nb; counts[n_slots + unit] = nr; }
	} else if (unit < n_slots + n_chunks) {
		const int chunk = unit - n_slots;
		const size_t L = (size_t)W * H;
		int n = 0;
		for (int step = 0; step < kWeakChunk / 64; ++step) {
			const size_t i = (size_t)chunk * kWeakChunk + step * 64 + lane;
			n += __popcll(__ballot(i < L && weak[i] == DVP_WEAK));
		}
		if (lane == 0) counts[2 * n_slots + chunk] = n;
	}
}
// exclusive scan of three int arrays in place (one workgroup each): blockIdx.x selects [start[b], start[b + 1]); totals[b] = sum
extern "C" __global__ void __launch_bounds__(1024) dvp_scan3(int* __restrict__ data, int s0, int s1, int s2, int s3, int* __restrict__ totals) {
	__shared__ int part[1024];
	__shared__ int carry;
	const int starts[4] = { s0, s1, s2, s3 };
	const int lo = starts[blockIdx.x], hi = starts[blockIdx.x + 1];
	if (threadIdx.x == 0) carry = 0;
	__syncthreads();
	for (int base = lo; base < hi; base += 1024) {
		const int i = base + (int)threadIdx.x;
		const int v = i < hi ? data[i] : 0;
		part[threadIdx.x] = v;
		__syncthreads();
		for (int off = 1; off < 1024; off <<= 1) {
			const int add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
			__syncthreads();
			part[threadIdx.x] += add;
			__syncthreads();
		}
		if (i < hi) data[i] = carry + part[threadIdx.x] - v;
		__syncthreads();
		if (threadIdx.x == 1023) carry += part[1023];
		__syncthreads();
	}
	if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
// scatter: the list entries of a slot / the running indices of a chunk, in pixel order, by ballot rank
extern "C" __global__ void __launch_bounds__(256) dvp_weak_fill(const uint8_t* __restrict__ weak, int W, int H, int supers_x, int n_slots, int n_chunks,
                                                               const int* __restrict__ offs, const int* __restrict__ totals, int* __restrict__ list, int* __restrict__ map) {
	const int lane = threadIdx.x & 63;
	const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
	const unsigned long long below = (1ull << lane) - 1ull;
	if (unit < n_slots) {
		int tx, ty;
		weak_slot_origin(unit, supers_x, &tx, &ty);
		int ob = offs[unit], orr = totals[0] + offs[n_slots + unit];   // red entries follow all black ones
		for (int step = 0; step < 4; ++step) {
			const int x = tx + (lane & 15), y = ty + step * 4 + (lane >> 4);
			const bool wk = x < W && y < H && weak[(size_t)y * W + x] == DVP_WEAK;
			const bool red = (x + y) & 1;
			const unsigned long long mb = __ballot(wk && !red), mr = __ballot(wk && red);
			if (wk) list[red ? orr + __popcll(mr & below) : ob + __popcll(mb & below)] = y * W + x;
			ob += __popcll(mb);
			orr += __popcll(mr);
		}
	} else if (unit < n_slots + n_chunks) {
		const int chunk = unit - n_slots;
		const size_t L = (size_t)W * H;
		int o = offs[2 * n_slots + chunk];
		for (int step = 0; step < kWeakChunk / 64; ++step) {
			const size_t i = (size_t)chunk * kWeakChunk + step * 64 + lane;
			const bool wk = i < L && weak[i] == DVP_WEAK;
			const unsigned long long m = __ballot(wk);
			if (i < L) map[i] = wk ? o + __popcll(m & below) : 0;
			o += __popcll(m);
		}
	}
}

// RescaleMatToTargetSize (APD.cpp:1773-1795) for the five maps a REFINE_INIT pass inherits from the coarser pyramid level
// (APD.cpp:1428-1456 depth + normal -> planes, selected views, :1169-1181 pixel states, :1648-1667 radius map): nearest
// neighbour with the source's index rule — the ROW index is divided by the WIDTH ratio and the column index by the height
// ratio (`o_r = r / scale_x`, `o_c = c / scale_y`, :1787-1788; the same unless the aspect ratios differ) — one IEEE float
// division and a truncation each; a pixel whose source index falls outside the coarse map stays zero.  Then the radius
// rule of APD.cpp:1660-1666: a pixel whose state is UNKNOWN restarts with the default patch radius.
struct RescaleArgs {
	int W, H, sw, sh;
	float scale_x, scale_y;
	const float* depth; const float* normal; const uint32_t* views; const uint8_t* weak; const int* radius;   // coarse maps; weak / radius may be null
	f4* planes; uint32_t* out_views; uint8_t* out_weak; int* out_radius;
	int radius_fallback;
};
extern "C" __global__ void __launch_bounds__(256) dvp_rescale_state(const RescaleArgs a) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
	if (c >= a.W) return;
	const int o_r = static_cast<int>(r / a.scale_x);
	const int o_c = static_cast<int>(c / a.scale_y);
	const bool in = o_r >= 0 && o_c >= 0 && o_r < a.sh && o_c < a.sw;
	const size_t o = (size_t)r * a.W + c, i = in ? (size_t)o_r * a.sw + o_c : 0;
	a.planes[o] = in ? mk4(a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2], a.depth[i]) : mk4(0.0f, 0.0f, 0.0f, 0.0f);
	a.out_views[o] = in ? a.views[i] : 0u;
	const uint8_t st = a.weak ? (in ? a.weak[i] : (uint8_t)0) : (uint8_t)DVP_STRONG;
	a.out_weak[o] = st;
	if (a.radius) a.out_radius[o] = st == DVP_UNKNOWN ? a.radius_fallback : (in ? a.radius[i] : 0);
}

// What the driver makes of the downloaded planes (main.cpp:300-309): depth map = plane.w where it lies inside
// [depth_min, depth_max], else 0 and the pixel's state becomes UNKNOWN; normal map = plane.xyz.  (`!(w < min || w > max)`
// as the source writes it: a NaN depth is kept.)
extern "C" __global__ void __launch_bounds__(256) dvp_unpack_maps(const f4* __restrict__ planes, const uint8_t* __restrict__ weak, size_t L, float dmin, float dmax,
                                                                 float* __restrict__ depth, float* __restrict__ normal, uint8_t* __restrict__ state) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= L) return;
	const f4 ph = planes[i];
	const bool usable = !(ph.w < dmin || ph.w > dmax);
	depth[i] = usable ? ph.w : 0.0f;
	normal[3 * i] = ph.x; normal[3 * i + 1] = ph.y; normal[3 * i + 2] = ph.z;
	state[i] = usable ? weak[i] : (uint8_t)DVP_UNKNOWN;
}

extern "C" __global__ void dvp_prepare_views(const DvpCamera* cams, ViewConst* views, int n) {
	const int v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v >= 1 && v < n) compute_view_const(cams[0], cams[v], &views[v]);
}

// ComputeMultiViewCostVectorOld over a list of (pixel, plane) pairs — KATs and the roofline
// micro-benchmark.  One lane per pair.
extern "C" __global__ void __launch_bounds__(256) dvp_cost_vectors(const Dev d, const int* px, const f4* planes, int n, float* out) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int x = px[2 * i], y = px[2 * i + 1];
	const int S = d.num_images - 1;
	PatchCtx c;
	__shared__ f2 lds_tab[kTaps * kTaps * 256];
	int radius, inc;
	patch_geometry(d, x + y * d.width, &radius, &inc);
	build_patch_ctx(d, x, y, radius, inc, 0, PatchTab{&lds_tab[threadIdx.x], 256}, &c);
	const f4 pl = planes[i];
	for (int v = 0; v < S; ++v) out[(size_t)i * S + v] = d.sampler ? ncc_old<1>(d, c, x, y, v + 1, pl) : ncc_old<0>(d, c, x, y, v + 1, pl);
}

// same computation on every pixel with its current plane (camera frame); writes the view-mean
extern "C" __global__ void __launch_bounds__(256) dvp_cost_all_pixels(const Dev d, const LaunchArgs a, float* out) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int px, py;
	if (!block_to_pixel(blockIdx.x, lane, wave, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py)) return;
	const int center = px + py * d.width;
	const int S = d.num_images - 1;
	PatchCtx c;
	__shared__ f2 lds_tab[kTaps * kTaps * 256];
	int radius, inc;
	patch_geometry(d, center, &radius, &inc);
	build_patch_ctx(d, px, py, radius, inc, 0, PatchTab{&lds_tab[threadIdx.x], 256}, &c);
	const f4 pl = d.planes[center];
	float acc = 0.0f;
	for (int v = 0; v < S; ++v) acc += ncc_old<0>(d, c, px, py, v + 1, pl);
	out[center] = acc / S;
}

#endif
