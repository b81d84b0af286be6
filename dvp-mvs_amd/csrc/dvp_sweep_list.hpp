// dvp_sweep_list.hpp — the sweep passes' evaluation launches from per-view (pixel, view) lists (DVP_SWEEP_LIST).
// The tile form of dvp_sweep_eval compacts the participating pixels of ONE 64 x kSweepRows tile and walks them 64 per round: the
// last round of every (tile, view) is part-empty and still issues the whole slot loop (about 640 pairs per workgroup at cfg3: 9.9
// rounds of work issued as 10.4).  Here every stage gets one list per source view of the pixels for which sweep_go is true, and a
// wave takes kSweepListRounds consecutive rounds of it: only the last round of a view's list can be part-empty.
// Order of a list = the order the tile form visits the same pixels in: tiles in strip order (sweep_list_tile: the launch map of
// dvp_sweep_eval), rows inside a tile top to bottom, x ascending inside a row — neighbours in the list are the neighbours they are in
// the tile form.  Built like the WEAK list (dvp_weak_counts / dvp_scan3 / dvp_weak_fill): counts per (view, tile), an exclusive scan
// per view, a ballot-rank scatter — no atomics, the order does not depend on timing.
// The per-pixel and per-row pieces are shared by the kernels (dvp_kernels.hpp: dvp_sweep_list_counts / _fill, dvp_sweep_eval_list)
// and by the host forms below (tests/sweep_list_host: the list program and the emulation of the passes), which take a wave's 64
// lanes one after the other.
#ifndef DVP_SWEEP_LIST_HPP_
#define DVP_SWEEP_LIST_HPP_

#include "dvp_sweep.hpp"
#include <cstring>

namespace dvp {

// rounds of 64 entries a workgroup (one wave) of dvp_sweep_eval_list takes.  Measured at cfg3, site ms per pass against the tile
// form's 486.4: R = 2 467.3, 4 477.4, 8 483.3, 16 488.5 (profiles/sweep_lists.txt) — the shorter the chunks, the closer together
// the entries the waves in flight work on
#ifndef DVP_SWEEP_LIST_R
#define DVP_SWEEP_LIST_R 2
#endif
constexpr int kSweepListRounds = DVP_SWEEP_LIST_R;

// Bit v: sweep_go(d, center, v, stage).  One read of the pixel's flags, selected-view word and 32 weight bytes serves all views.
DVP_HD uint32_t sweep_go_mask(const Dev& d, int center, int stage) {
	const size_t L = (size_t)d.width * (size_t)d.height;
	const int flags = (int)d.sweep_rec[L + center].w;
	if (!(flags & (stage == 0 ? SWF_VALID : SWF_PEAK))) return 0;
	const int S = d.params.num_images - 1;
	uint32_t sel = d.selected_views[center];
	if (S < 32) sel &= (1u << S) - 1u;
	const uint8_t* vw = static_cast<const uint8_t*>(__builtin_assume_aligned(d.view_weight + (size_t)center * 32, 4));
	uint32_t m = 0;
	for (int q = 0; q * 4 < S; ++q) {
		uint32_t w;
		memcpy(&w, vw + 4 * q, 4);   // weights of the views 4q ... 4q + 3, one per byte
		uint32_t nz = 0;
		for (int b = 0; b < 4; ++b) nz |= ((w >> (8 * b)) & 255u) ? 1u << b : 0u;
		m |= nz << (4 * q);
	}
	return sel & m;
}

// tile t of a launch over tiles_x x tiles_y tiles: the strip map of dvp_sweep_eval (block_to_pixel's, over tiles of kSweepRows rows)
DVP_HD void sweep_list_tile(int t, int tiles_x, int tiles_y, int* tx, int* ty) {
	const int per_strip = 8 * tiles_y;
	const int st = t / per_strip, rem = t - st * per_strip;
	const int w_last = tiles_x - st * 8;
	if (w_last >= 8) { *ty = rem >> 3; *tx = st * 8 + (rem & 7); }
	else { *ty = rem / w_last; *tx = st * 8 + (rem - *ty * w_last); }
}
// a list entry (contexts require coordinates below 2^15)
DVP_HD uint32_t sweep_list_pack(int x, int y) { return ((uint32_t)y << 16) | (uint32_t)x; }
DVP_HD int sweep_list_x(uint32_t e) { return (int)(e & 0xFFFFu); }
DVP_HD int sweep_list_y(uint32_t e) { return (int)(e >> 16); }
// lane `lane` of a tile row whose participation mask is m (bit = lane) writes its entry behind the `at` entries before the row
DVP_HD void sweep_list_put(uint32_t* list, int at, unsigned long long m, int lane, int x, int y) {
	if ((m >> lane) & 1ull) list[at + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = sweep_list_pack(x, y);
}

// Workgroups (x extent of the grid) of an evaluation launch over lists with room for `cap` entries: the upper bound — the lengths
// stay on the device.
DVP_HD int sweep_list_grid(int cap, int rounds) { return (cap + 64 * rounds - 1) / (64 * rounds); }
// The chunk (`rounds` rounds of 64 entries) of a list of n entries that workgroup b takes, or -1: past the end.  Chunk = workgroup
// id: workgroups reach the XCDs round-robin by their id, so the waves in flight on all XCDs together walk one contiguous part of
// the list, as they walk one neighbourhood of the image under the strip map of the tile form.  (Measured against an XCD walking a
// contiguous eighth of the view's list, which put eight XCDs on eight distant parts of the source images: 36 to 54 ms per cfg3
// pass slower at every R, profiles/sweep_lists.txt.)
DVP_HD int sweep_list_chunk(int b, int n, int rounds) {
	const int chunks = (n + 64 * rounds - 1) / (64 * rounds);
	return b < chunks ? b : -1;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the three launches on the host: a.tiles_x / a.tiles = the tile grid, a.rows = its first tile row, a.iter = stage ----
// counts[v * tiles + t] = entries of (view v, tile t)
inline void sweep_list_counts_host(const Dev& d, int tiles_x, int tiles, int rows, int stage, int* counts) {
	const int S = d.params.num_images - 1;
	for (int t = 0; t < tiles; ++t) {
		int tx, ty;
		sweep_list_tile(t, tiles_x, tiles / tiles_x, &tx, &ty);
		ty += rows;
		for (int v = 0; v < S; ++v) counts[(size_t)v * tiles + t] = 0;
		for (int r = 0; r < kSweepRows; ++r)
			for (int lane = 0; lane < 64; ++lane) {
				const int x = tx * 64 + lane, y = ty * kSweepRows + r;
				const uint32_t m = (x < d.width && y < d.height) ? sweep_go_mask(d, x + y * d.width, stage) : 0u;
				for (int v = 0; v < S; ++v) counts[(size_t)v * tiles + t] += (int)((m >> v) & 1u);
			}
	}
}
// dvp_scan3 per view: the counts become the tiles' first entries, n[v] = the list's length
inline void sweep_list_scan_host(int S, int tiles, int* counts, int* n) {
	for (int v = 0; v < S; ++v) {
		int run = 0;
		for (int t = 0; t < tiles; ++t) { const int k = counts[(size_t)v * tiles + t]; counts[(size_t)v * tiles + t] = run; run += k; }
		n[v] = run;
	}
}
// list[v * cap + i] = the i-th entry of view v
inline void sweep_list_fill_host(const Dev& d, int tiles_x, int tiles, int rows, int stage, const int* offs, uint32_t* list, int cap) {
	const int S = d.params.num_images - 1;
	for (int t = 0; t < tiles; ++t) {
		int tx, ty, o[32];
		sweep_list_tile(t, tiles_x, tiles / tiles_x, &tx, &ty);
		ty += rows;
		for (int v = 0; v < S; ++v) o[v] = offs[(size_t)v * tiles + t];
		for (int r = 0; r < kSweepRows; ++r) {
			const int y = ty * kSweepRows + r;
			uint32_t mk[64];
			for (int lane = 0; lane < 64; ++lane) {
				const int x = tx * 64 + lane;
				mk[lane] = (x < d.width && y < d.height) ? sweep_go_mask(d, x + y * d.width, stage) : 0u;
			}
			for (int v = 0; v < S; ++v) {
				unsigned long long m = 0;   // the wave's ballot
				for (int lane = 0; lane < 64; ++lane) m |= (unsigned long long)((mk[lane] >> v) & 1u) << lane;
				for (int lane = 0; lane < 64; ++lane) sweep_list_put(list + (size_t)v * cap, o[v], m, lane, tx * 64 + lane, y);
				o[v] += __builtin_popcountll(m);
			}
		}
	}
}
#endif

}  // namespace dvp
#endif
