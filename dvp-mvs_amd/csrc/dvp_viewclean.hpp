// dvp_viewclean.hpp — the visibility-mask clean-up of ProcessProblem (main.cpp:311-363; host/main.cpp on top of host/cc.cpp) as
// per-pixel and per-tile functions for the device (dvp_viewclean.hip) and, the same text, for a serial host build
// (tests/viewclean_host).  Integer arithmetic only.  For every bit b < num_src of the selected-view words:
//   out bit b = in bit b  or  (the pixel's 4-connected component of pixels whose bit b is clear has fewer than min_region pixels)
// and the bits >= num_src are 0.  One bit plane is labelled in four steps:
//   1. tile    a TILE_W x TILE_H tile is labelled on its own (tile_init / tile_union_up / tile_count / tile_store): the clear
//              pixels of a row form runs, a run is named after its first lane (run_head: bit arithmetic on the row's 64-bit
//              mask), runs of adjacent rows that overlap are united (dvp_edges.hpp uf_union on tile-local labels), the pixels of
//              a tile-local component are counted once per run.  Out go, per pixel, the GLOBAL index of its local root
//              (parent) and, at the local root, the count (size; 0 at every other pixel)
//   2. seams   pixels on a tile's last column / last row unite with their E / S neighbour in the next tile (seam_item):
//              uf_union on the global parent words — only local roots are ever roots there
//   3. roll-up every local root that is not its component's root adds its count to the root's size word and links to it
//              (rollup_pixel): one addition per tile and component
//   4. resolve a clear pixel follows parent to the root and compares the root's size (resolve_word), all planes of a word at once
// parent[i] <= i throughout (a root is the smallest index of its set, in a tile as in the image), as in dvp_edges.hpp.
#ifndef DVP_VIEWCLEAN_HPP_
#define DVP_VIEWCLEAN_HPP_

#include <stddef.h>
#include <stdint.h>

#include "dvp_edges.hpp"

namespace dvpvc {

using dvpedge::uf_find;
using dvpedge::uf_union;

enum { TILE_W = 64, TILE_H = 16, TILE_PIXELS = TILE_W * TILE_H };   // TILE_W = the wave: a row's mask is one __ballot

DVP_EHD uint32_t low_mask(int num_src) { return num_src >= 32 ? 0xffffffffu : ((1u << num_src) - 1u); }

// clear: bit l = pixel l of the row is clear.  The run of a clear lane starts after the nearest lane below it that is not clear.
DVP_EHD int run_head(uint64_t clear, int lane) {
	const uint64_t below = ~clear & (((uint64_t)1 << lane) - 1);
	return below ? 64 - __builtin_clzll(below) : 0;
}
// ... and ends before the nearest lane above its head that is not clear (head is a clear lane)
DVP_EHD int run_length(uint64_t clear, int head) {
	const uint64_t stop = ~clear >> head;
	return stop ? __builtin_ctzll(stop) : 64 - head;
}

// ---- step 1.  lab, cnt: [TILE_PIXELS] words, rows: [TILE_H] masks of one tile (LDS on the device); a label is row * TILE_W +
// lane < 1024.  The four functions run for every (row, lane) of the tile, each after the one before has finished for all.
DVP_EHD void tile_init(unsigned* lab, unsigned* cnt, uint64_t* rows, int r, int lane, uint64_t clear) {
	const int l = r * TILE_W + lane;
	lab[l] = ((clear >> lane) & 1) ? (unsigned)(r * TILE_W + run_head(clear, lane)) : (unsigned)l;
	cnt[l] = 0;
	if (lane == 0) rows[r] = clear;
}
// the run of (r, lane) and the run above it: united by the first lane of every stretch the two rows share
template <class Mem>
DVP_EHD void tile_union_up(Mem& mem, unsigned* lab, const uint64_t* rows, int r, int lane) {
	if (r == 0) return;
	const uint64_t both = rows[r] & rows[r - 1];
	if (!((both >> lane) & 1)) return;
	if (lane > 0 && ((both >> (lane - 1)) & 1)) return;
	uf_union(mem, lab, (unsigned)(r * TILE_W + run_head(rows[r], lane)), (unsigned)((r - 1) * TILE_W + run_head(rows[r - 1], lane)));
}
// no unions run any more: a run's head adds the run's length to the local root's count
template <class Mem>
DVP_EHD void tile_count(Mem& mem, unsigned* lab, unsigned* cnt, const uint64_t* rows, int r, int lane) {
	const uint64_t clear = rows[r];
	if (!((clear >> lane) & 1) || run_head(clear, lane) != lane) return;
	const unsigned l = (unsigned)(r * TILE_W + lane);
	const unsigned root = uf_find(mem, lab, l);
	mem.min(lab + l, root);
	mem.add(cnt + root, (unsigned)run_length(clear, lane));
}
// (x0, y0): the tile's first pixel; parent, size: the plane's words
template <class Mem>
DVP_EHD void tile_store(Mem& mem, unsigned* lab, const unsigned* cnt, const uint64_t* rows, int r, int lane, int x0, int y0, int W, int H, unsigned* parent, unsigned* size) {
	const int x = x0 + lane, y = y0 + r;
	if (x >= W || y >= H) return;
	const size_t i = (size_t)y * W + x;
	const uint64_t clear = rows[r];
	if (!((clear >> lane) & 1)) { size[i] = 0; return; }   // (its parent word is never read)
	const unsigned l = (unsigned)(r * TILE_W + lane);
	const unsigned root = uf_find(mem, lab, (unsigned)(r * TILE_W + run_head(clear, lane)));
	parent[i] = (unsigned)((size_t)(y0 + (int)(root / TILE_W)) * W + (size_t)(x0 + (int)(root % TILE_W)));
	size[i] = root == l ? cnt[root] : 0u;   // a component holds its root: the count is never 0 there
}

// ---- step 2.  Seams: (W - 1) / TILE_W vertical ones of H pixels, then (H - 1) / TILE_H horizontal ones of W pixels
DVP_EHD size_t seam_items(int W, int H) { return (size_t)((W - 1) / TILE_W) * (size_t)H + (size_t)((H - 1) / TILE_H) * (size_t)W; }
// A pair whose predecessor along the seam, in the same two tiles, is a clear pair too has nothing to do: each of its pixels
// touches the predecessor's on its own side, inside a tile, so step 1 put them under one local root already, and the first pair
// of such a stretch unites the two sides.  A region that lies against a seam for its whole length costs one union per tile edge.
template <class Mem>
DVP_EHD void seam_item(Mem& mem, const uint32_t* views, int bit, unsigned* parent, size_t t, int W, int H) {
	const size_t sx = (size_t)((W - 1) / TILE_W), vertical = sx * (size_t)H;
	size_t i, j, back;   // the pair (i, j); its predecessor is (i - back, j - back), back = 0: none in these tiles
	if (t < vertical) {
		const size_t y = t / sx, s = t - y * sx;
		i = y * (size_t)W + s * TILE_W + (TILE_W - 1);
		j = i + 1;
		back = y % TILE_H ? (size_t)W : 0;
	} else {
		const size_t u = t - vertical, s = u / (size_t)W, x = u - s * (size_t)W;
		i = (s * TILE_H + (TILE_H - 1)) * (size_t)W + x;
		j = i + (size_t)W;
		back = x % TILE_W ? 1 : 0;
	}
	if (((views[i] | views[j]) >> bit) & 1u) return;
	if (back && !(((views[i - back] | views[j - back]) >> bit) & 1u)) return;
	uf_union(mem, parent, (unsigned)i, (unsigned)j);
}

// ---- step 3.  No unions run any more: uf_find returns the component's root
template <class Mem>
DVP_EHD void rollup_pixel(Mem& mem, unsigned* parent, unsigned* size, size_t i) {
	const unsigned s = size[i];   // (only a root's word changes in this step, and a root does nothing here)
	if (!s) return;
	const unsigned r = uf_find(mem, parent, (unsigned)i);
	if (r == (unsigned)i) return;
	mem.min(parent + i, r);
	mem.add(size + r, s);
}

// ---- step 4.  parent, size: plane b at + b * L.  Steps 1-3 are over: plain loads
DVP_EHD uint32_t resolve_word(uint32_t word, int num_src, int min_region, const unsigned* parent, const unsigned* size, size_t L, size_t i) {
	uint32_t out = word & low_mask(num_src);
	for (int b = 0; b < num_src; ++b) {
		if ((word >> b) & 1u) continue;
		const unsigned* p = parent + (size_t)b * L;
		unsigned x = (unsigned)i, q = p[x];
		while (q != x) { x = q; q = p[x]; }
		if ((long long)size[(size_t)b * L + x] < (long long)min_region) out |= 1u << b;
	}
	return out;
}

}   // namespace dvpvc
#endif
