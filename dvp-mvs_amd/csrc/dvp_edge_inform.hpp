// dvp_edge_inform.hpp — per-pixel bodies of GenEdgeInform (APD.cu:3731-3890), the prior preparation of the weak path:
// the rays to the nearest edge pixel and label stop (APD.cu:3799-3824, 3861-3873), the visibility-prior tap candidates
// of every (pixel, source view) (APD.cu:3746-3794, calculateAngle / getRegion APD.cu:797-821) and the per-pixel rest
// (APD.cu:3796-3890).
#ifndef DVP_EDGE_INFORM_HPP_
#define DVP_EDGE_INFORM_HPP_

#include "dvp_ncc.hpp"

namespace dvp {

#include "dvp_sector5.inc"

// ---- GenEdgeInform (APD.cu:3731-3890) ----------------------------------------------------------
// The reference bins the 120 offsets of the 11x11 window into 30-degree sectors with fp64 atan2
// per offset, bubble-sorts each sector and then the 12 winners (24-byte structs in scratch).
// Here the sector of an offset comes from a 121-entry table and each sector keeps a running
// arg-max; the stable descending sort of the 12 winners is kept.
// Nearest edge pixel in each of the 8 directions (APD.cu:3799-3824).  The reference marches a ray
// per pixel and direction (up to max(W,H) steps each: O(L*(W+H)) reads).  Here one thread owns
// one image line of one direction and walks it once AGAINST the direction, carrying the last edge
// pixel seen: O(L) reads per direction, same result.
DVP_HD int edge_ray_lines(int W, int H, int k) { return k < 2 ? W : (k < 4 ? H : W + H - 1); }
// what = 0: nearest edge pixel -> edge_neigh;  what = 1: nearest pixel with label -1 -> label_stop
// (the walks of the label-boundary search stop there, APD.cu:3861-3873)
DVP_HD void edge_ray_line(const Dev& d, int k, int line, int what = 0) {
	const int W = d.width, H = d.height;
	const int dxs[8] = { 0, 0, -1, 1, -1, 1, -1, 1 };
	const int dys[8] = { -1, 1, 0, 0, -1, 1, 1, -1 };
	const int dx = dxs[k], dy = dys[k];
	if (line >= edge_ray_lines(W, H, k)) return;
	// first pixel of the line in walking order (-d): the pixel whose +d neighbour is outside
	int x, y;
	if (dx == 0) { x = line; y = dy < 0 ? 0 : H - 1; }
	else if (dy == 0) { x = dx < 0 ? 0 : W - 1; y = line; }
	else {
		const int xb = dx < 0 ? 0 : W - 1, yb = dy < 0 ? 0 : H - 1;
		if (line < H) { x = xb; y = line; }
		else { const int t = line - H; x = (xb == 0) ? t + 1 : t; y = yb; }
	}
	s2 last = mks2(-1, -1);
	while (x >= 0 && x < W && y >= 0 && y < H) {
		const int c = x + y * W;
		if (what == 0) {
			d.edge_neigh[(size_t)c * 8 + k] = last;
			if (d.edge[c]) last = mks2(x, y);
		} else {
			d.label_stop[(size_t)c * 8 + k] = last;
			if (d.label[c] == -1) last = mks2(x, y);
		}
		x -= dx;
		y -= dy;
	}
}

// Visibility-prior tap candidates of (pixel, source view v) (APD.cu:3746-3794): the window offsets whose
// pixel sees view v are binned into twelve 30-degree sectors (at most 20 per sector, visit order), each
// sector keeps its heaviest offset (first one among equals: the reference's stable bubble sort), the
// twelve winners are sorted by weight and the top eight stored.
// Launch shape (this function: more than 32 views, or another window than the default; else gen_candidates_views_px below):
// pixels x views (the view is wave-uniform), one pass over the window per lane, the twelve
// winners in registers.  (Round 1 walked the window once per pixel for all views and kept S x 12 running
// maxima in a dynamically indexed private array: 3.2 KB of scratch per lane, 330 GB of write-back per
// launch at 6208x4128.)  For the default window (weak_radius = 5, main.h:104; the reference never
// changes it) the sector lists are compile-time constants (dvp_sector5.inc): every load has a static
// offset and no branch in front of it, so the compiler batches them.
DVP_HD void gen_candidates_px(const Dev& d, int px, int py, int v) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const float* ref = d.images;
	const float cpix = img_texel(ref, d.org, d.pitch, W, H, px, py);
	struct Best { float w; int i, j; };
	struct alignas(16) Cand8 { s2 o[8]; };
	Best win[12];
	bool any = false;
#ifndef DVP_GEI_GENERIC
	if (P.weak_radius == 5) {
#else
	if (false) {
#endif
#pragma unroll
		for (int r = 0; r < 12; ++r) {
			Best b = Best{ 0.0f, 0, 0 };
			bool has = false;
#pragma unroll
			for (int t = 0; t < kSector5Max; ++t) {
				if (t >= kSector5Count[r]) continue;
				const int i = kSector5[r][t][0], j = kSector5[r][t][1];
				const int x = px + i, y = py + j;
				const bool in = x >= 0 && x < W && y >= 0 && y < H;
				// clamped address: the load is unconditional (in-bounds), its value is used only when `in`
				const uint32_t sv = d.selected_views[clampi(y, 0, H - 1) * W + clampi(x, 0, W - 1)];
				const float a = img_texel(ref, d.org, d.pitch, W, H, x, y);
				const float w = bilateral_weight((float)i, (float)j, a, cpix, P.sigma_spatial, P.sigma_color, 1);
				if (in && ((sv >> v) & 1) && (!has || w > b.w)) { has = true; b = Best{ w, i, j }; }
			}
			win[r] = b;
			any |= has;
		}
	} else {
		const int radius = P.weak_radius;
#pragma unroll
		for (int r = 0; r < 12; ++r) {
			Best b = Best{ 0.0f, 0, 0 };
			bool has = false;
			int cnt = 0;
			const int t1 = uniform_load_i32(d.sector_start, r + 1);
			for (int t = uniform_load_i32(d.sector_start, r); t < t1; ++t) {
				const int code = uniform_load_i32(d.sector_taps, t);
				const int i = (code & 0xffff) - radius, j = (code >> 16) - radius;
				const int x = px + i, y = py + j;
				if (!(x >= 0 && x < W && y >= 0 && y < H)) continue;
				if (!((d.selected_views[x + y * W] >> v) & 1)) continue;
				if (cnt >= 20) continue;   // regionCounts[region] < 20 (APD.cu:3768)
				cnt++;
				const float a = img_texel(ref, d.org, d.pitch, W, H, x, y);
				const float w = bilateral_weight((float)i, (float)j, a, cpix, P.sigma_spatial, P.sigma_color, 1);
				if (!has || w > b.w) { has = true; b = Best{ w, i, j }; }
			}
			win[r] = b;
			any |= has;
		}
	}
	if (any) {   // stable descending sort of the 12 sector winners (empty sectors: weight 0, offset (0,0))
#pragma unroll
		for (int a = 1; a < 12; ++a) {
#pragma unroll
			for (int b = a; b >= 1; --b) {
				const bool sw = win[b - 1].w < win[b].w;
				const Best lo = win[b - 1], hi = win[b];
				win[b - 1] = sw ? hi : lo;
				win[b] = sw ? lo : hi;
			}
		}
	}
	Cand8 rec;
#pragma unroll
	for (int k = 0; k < 8; ++k) rec.o[k] = mks2(win[k].i, win[k].j);
	*reinterpret_cast<Cand8*>(d.candidate + cand_index(d, center, v)) = rec;   // two 16-byte stores
}

// The same records for ALL source views of a pixel by one lane (round 6).  A tap's weight does not depend on the view — only
// whether the tap's pixel sees it does — so the pixels x views launch evaluated every weight (an exp among ~35 instructions) and
// fetched every texel and selected-view word S times (52 ms per 25-Mpx launch with S = 9).  Here: one pass over the window, the
// weight once, S running sector maxima in registers (views unrolled over MV, nothing indexed dynamically), and instead of twelve
// winners per view to sort at the end, each view's sorted top eight kept as the sectors finish: inserting the sectors' winners in
// sector order, each BELOW the entries that are not lighter, is the reference's stable bubble sort (APD.cu:3786-3792) step by step,
// and an entry that falls out of the first eight cannot come back.  Empty sectors take part with weight 0 and offset (0, 0) as they
// do there (a view no tap sees: eight zero offsets either way).  weak_radius == 5 (dvp_sector5.inc) only; a lane takes MV views, the
// launch has ceil(S / MV) lanes per pixel.
template <int MV>
DVP_HD void gen_candidates_views_px(const Dev& d, int px, int py, int v0 = 0) {   // views v0 .. v0 + MV - 1
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const int S = P.num_images - 1;
	const float* ref = d.images;
	const float cpix = img_texel(ref, d.org, d.pitch, W, H, px, py);
	float top_w[MV][8];
	uint32_t top_o[MV][8];   // offset as the record stores it: (uint16)i | (uint16)j << 16
#pragma unroll
	for (int v = 0; v < MV; ++v)
#pragma unroll
		for (int k = 0; k < 8; ++k) { top_w[v][k] = -1.0f; top_o[v][k] = 0u; }   // (-1: below every weight, an empty place)
#pragma unroll
	for (int r = 0; r < 12; ++r) {
		float bw[MV];
		uint32_t bo[MV];
		uint32_t has = 0;
#pragma unroll
		for (int v = 0; v < MV; ++v) { bw[v] = 0.0f; bo[v] = 0u; }
#pragma unroll
		for (int t = 0; t < kSector5Max; ++t) {
			if (t >= kSector5Count[r]) continue;
			const int i = kSector5[r][t][0], j = kSector5[r][t][1];
			const int x = px + i, y = py + j;
			const bool in = x >= 0 && x < W && y >= 0 && y < H;
			const uint32_t sv = d.selected_views[clampi(y, 0, H - 1) * W + clampi(x, 0, W - 1)];   // (in-bounds; used only when `in`)
			const float a = img_texel(ref, d.org, d.pitch, W, H, x, y);
			const float w = bilateral_weight((float)i, (float)j, a, cpix, P.sigma_spatial, P.sigma_color, 1);
			const uint32_t o = ((uint32_t)i & 0xffffu) | ((uint32_t)j << 16);
			const uint32_t seen = in ? (sv >> v0) : 0u;
#pragma unroll
			for (int v = 0; v < MV; ++v) {
				const bool take = ((seen >> v) & 1u) && (!((has >> v) & 1u) || w > bw[v]);
				bw[v] = take ? w : bw[v];
				bo[v] = take ? o : bo[v];
				has |= take ? (1u << v) : 0u;
			}
		}
		// the sector's winners into the views' lists
#pragma unroll
		for (int v = 0; v < MV; ++v) {
			const float w = bw[v];
			const uint32_t o = bo[v];
#pragma unroll
			for (int k = 7; k >= 1; --k) {
				const bool from_above = top_w[v][k - 1] < w;   // the entry above is lighter: it moves down to k
				const bool here = top_w[v][k] < w;              // (else) the new entry lands at k if k's is lighter
				top_o[v][k] = from_above ? top_o[v][k - 1] : (here ? o : top_o[v][k]);
				top_w[v][k] = from_above ? top_w[v][k - 1] : (here ? w : top_w[v][k]);
			}
			const bool first = top_w[v][0] < w;
			top_o[v][0] = first ? o : top_o[v][0];
			top_w[v][0] = first ? w : top_w[v][0];
		}
	}
#pragma unroll
	for (int v = 0; v < MV; ++v) {
		if (v0 + v >= S) continue;
		uint32_t* out = reinterpret_cast<uint32_t*>(d.candidate + cand_index(d, center, v0 + v));
#if defined(__HIP_DEVICE_COMPILE__)
		typedef uint32_t u4 __attribute__((ext_vector_type(4)));
		u4 lo, hi;
		lo.x = top_o[v][0]; lo.y = top_o[v][1]; lo.z = top_o[v][2]; lo.w = top_o[v][3];
		hi.x = top_o[v][4]; hi.y = top_o[v][5]; hi.z = top_o[v][6]; hi.w = top_o[v][7];
		reinterpret_cast<u4*>(out)[0] = lo;
		reinterpret_cast<u4*>(out)[1] = hi;
#else
		for (int k = 0; k < 8; ++k) d.candidate[cand_index(d, center, v0 + v) + k] = mks2((int)(int16_t)(top_o[v][k] & 0xffffu), (int)(int16_t)(top_o[v][k] >> 16));
#endif
	}
}
#ifndef DVP_CAND_GROUP
#define DVP_CAND_GROUP 5   // 25-Mpx launch, S = 9: 42 ms (10: 110 ms at one wave per SIMD, 3: 47, 1: 97; a lane per (pixel, view) with a sort at the end: 53)
#endif
constexpr int kCandGroup = DVP_CAND_GROUP;   // views per lane (16 + 2 registers each); the launch has ceil(S / kCandGroup) lanes per pixel
constexpr int kCandViewsMax = 32;
DVP_HD bool gen_candidates_all_views(const Dev& d) {
#if defined(DVP_GEI_GENERIC) || defined(DVP_CAND_PER_VIEW)
	return false;
#else
	return d.params.weak_radius == 5 && d.params.num_images - 1 <= kCandViewsMax;
#endif
}

// the per-pixel rest of GenEdgeInform (APD.cu:3796-3890); candidates: gen_candidates_px, edge_neigh: edge_ray_line
DVP_HD void gen_edge_inform_px(const Dev& d, int px, int py) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const int dxs[8] = { 0, 0, -1, 1, -1, 1, -1, 1 };
	const int dys[8] = { -1, 1, 0, 0, -1, 1, 1, -1 };
	if (P.use_edge) {
		// edge_neigh is filled by the line-scan pre-pass (edge_ray_line) of the same launch site
		if (d.weak_info[center] == DVP_WEAK) {
			const int radius = P.strong_radius;
			int edge_pix = 0, tot_pix = 0;
			for (int i = -radius; i <= radius; i++)
				for (int j = -radius; j <= radius; j++) {
					const int nx = px + i, ny = py + j;
					if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
					if (d.edge[ny * W + nx]) edge_pix++;
					tot_pix++;
				}
			const float density = 1.0f * edge_pix / tot_pix;
			d.complex_[d.neighbours_map[center]] = 1.0f / (1.0f + dvp_expf(-25.0f * (density - 0.35f)));
		}
		if (P.state == DVP_REFINE_INIT && P.use_detail && d.edge[center]) {
			if (d.weak_info[center] != DVP_STRONG) d.weak_info[center] = DVP_UNKNOWN;
		}
	}
	if (P.use_label && d.weak_info[center] == DVP_WEAK) {
		s2* lb = d.label_boundary + (size_t)d.neighbours_map[center] * 8;
		const int cl = d.label[center];
		if (cl > 0) {
			for (int k = 0; k < 8; k++) {
				// The reference walks from the pixel to the first label -1 (or the border) and keeps the LAST
				// pixel of its own label it passed (APD.cu:3861-3873): thousands of dependent loads per ray
				// on a large region.  Same answer from the other end: the line-scan pre-pass (edge_ray_line,
				// what = 1) gives the stop pixel, and the farthest pixel of the own label is the first one
				// met walking BACK from there — on a region bounded by edges that is the first probe.
				const s2 stop = d.label_stop[(size_t)center * 8 + k];
				int nx, ny;   // last pixel before the stop (or the last pixel inside the image)
				if (stop.x != -1) { nx = stop.x - dxs[k]; ny = stop.y - dys[k]; }
				else {
					int steps = 1 << 30;   // pixels from (px,py) to the border along k
					if (dxs[k] > 0) steps = DVP_MIN(steps, W - 1 - px); else if (dxs[k] < 0) steps = DVP_MIN(steps, px);
					if (dys[k] > 0) steps = DVP_MIN(steps, H - 1 - py); else if (dys[k] < 0) steps = DVP_MIN(steps, py);
					nx = px + steps * dxs[k];
					ny = py + steps * dys[k];
				}
				int lx = -1, ly = -1;
				while (nx != px || ny != py) {
					if (d.label[nx + ny * W] == cl) { lx = nx; ly = ny; break; }
					nx -= dxs[k];
					ny -= dys[k];
				}
				lb[k] = mks2(lx, ly);
			}
		}
		if (P.state == DVP_REFINE_INIT && P.use_detail && d.label[center] == 0) {
			if (d.weak_info[center] != DVP_STRONG) d.weak_info[center] = DVP_UNKNOWN;
		}
	}
}

}  // namespace dvp
#endif
