// dvp_neighbours.hpp — the anchor search of the weak path: FindNearestStrongPoint (APD.cu:4159-4193), the geometry and
// line-walk predicates (APD.cu:244-311), GenNeighbours (APD.cu:3330-3711) and NeigbourUpdate (APD.cu:3713-3729).
// First the per-lane forms, which are the definition (one lane per WEAK pixel), then GenNeighbours with one wave per
// WEAK pixel: the directional search (APD.cu:3330-3505), the label extension (APD.cu:3455-3560) and the RANSAC fit through
// the candidate anchors (APD.cu:3562-3711).
#ifndef DVP_NEIGHBOURS_HPP_
#define DVP_NEIGHBOURS_HPP_

#include "dvp_wave.hpp"

#if defined(DVP_GN_STATS) && !defined(__HIPCC__)
#include <cstdio>
#endif
namespace dvp {

// ---- FindNearestStrongPoint (APD.cu:4159-4193) -------------------------------------------------
DVP_HD void find_nearest_strong_px(const Dev& d, int px, int py) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	s2 res = mks2(-1, -1);
	if (d.weak_info[center] == DVP_WEAK) {
		// The reference scans the whole (2r+1)^2 square of every ring and skips the interior (APD.cu:4176-4179):
		// O(r^3) dependent loads.  Its visiting order on a ring is x ascending — the whole left column (y
		// ascending), then per inner column the top pixel before the bottom one, then the whole right column — so
		// the first hit is: the first set bit of the left column segment, else the smaller of the first set bits
		// of the top and bottom row segments (top wins a tie), else the first set bit of the right column segment.
		// Row segments come from the row-major bit tiles of (weak_info == STRONG), column segments from the
		// transposed tiles: a ring costs 4-8 word loads instead of 8r byte loads.
		for (int radius = 1; radius <= 100; ++radius) {   // (ring 0 is the WEAK pixel itself)
			const int xl = px - radius, xr = px + radius, yt = py - radius, yb = py + radius;
			const int ya = DVP_MAX(yt, 0), yz = DVP_MIN(yb, H - 1);
			if (xl >= 0) {
				const int y = first_set_bit_in<true>(d.strong_bits_t, d.edge_tiles_x, xl, ya, yz);
				if (y >= 0) { res = mks2(xl, y); break; }
			}
			const int xa = DVP_MAX(xl + 1, 0), xz = DVP_MIN(xr - 1, W - 1);
			if (xa <= xz) {
				const int xt = yt >= 0 ? first_set_bit_in<false>(d.strong_bits, d.edge_tiles_x, yt, xa, xz) : -1;
				const int xb = yb < H ? first_set_bit_in<false>(d.strong_bits, d.edge_tiles_x, yb, xa, xz) : -1;
				if (xt >= 0 && (xb < 0 || xt <= xb)) { res = mks2(xt, yt); break; }
				if (xb >= 0) { res = mks2(xb, yb); break; }
			}
			if (xr < W) {
				const int y = first_set_bit_in<true>(d.strong_bits_t, d.edge_tiles_x, xr, ya, yz);
				if (y >= 0) { res = mks2(xr, y); break; }
			}
		}
	}
	d.weak_nearest_strong[center] = res;
}

// ---- geometry predicates (APD.cu:244-311) -------------------------------------------------------
DVP_HD bool point_in_triangle(s2 A, s2 B, s2 C, int px, int py) {
	const f2 AB = mk2((float)(B.x - A.x), (float)(B.y - A.y));
	const f2 BC = mk2((float)(C.x - B.x), (float)(C.y - B.y));
	const f2 CA = mk2((float)(A.x - C.x), (float)(A.y - C.y));
	const float ab = sqrtf(AB.x * AB.x + AB.y * AB.y);
	const float bc = sqrtf(BC.x * BC.x + BC.y * BC.y);
	const float ca = sqrtf(CA.x * CA.x + CA.y * CA.y);
	if (ab <= 2 || bc <= 2 || ca <= 2) return false;
	if (!(ab + bc > ca && bc + ca > ab && ab + ca > bc)) return false;
	const f2 PA = mk2((float)(A.x - px), (float)(A.y - py));
	const f2 PB = mk2((float)(B.x - px), (float)(B.y - py));
	const f2 PC = mk2((float)(C.x - px), (float)(C.y - py));
	const float t1 = PA.x * PB.y - PA.y * PB.x;
	const float t2 = PB.x * PC.y - PB.y * PC.x;
	const float t3 = PC.x * PA.y - PC.y * PA.x;
	return t1 * t2 >= 0 && t1 * t3 >= 0;
}

// true = the segment B->A crosses an edge pixel (APD.cu:267-311) — the definition: every step of the reference's walk is made.
// The reference walks the line one pixel per loop iteration and tests the edge map after every step
// (one dependent load per step, up to max(W,H)/30 of them).  The answer is "any visited pixel is
// an edge pixel", so the walk is done in blocks of 8 steps: eight positions from the integer
// line state, eight independent loads from the bit-tiled edge map (dvp_dev.hpp: edge_bit), one OR.
// Visited set, step limit and the one-pixel
// overshoot past the end point (the loop condition is tested after the step) are the reference's.
DVP_HD bool bresenham_hits_edge_steps(const Dev& d, int Ax, int Ay, int Bx, int By) {
	const int W = d.width, H = d.height;
	const int max_step = (int)(DVP_MAX(H, W) / 30.0);
	int x0 = Bx, y0 = By;
	const int x1 = Ax, y1 = Ay;
	const int ABx = Ax - Bx, ABy = Ay - By;
	if (ABx * ABx + ABy * ABy > 9 * max_step * max_step) return false;
	// Every pixel the walk can visit lies in the end points' bounding box widened by two pixels: the major
	// axis advances on every step and keeps going while the minor axis catches up, and the exit is tested
	// after the step (exhaustive check over all |dx|, |dy| < 260 and random ones up to 3 x 1092 steps: the walk
	// leaves the box by at most 2).  If the widened box holds no edge pixel at all — four loads from the cell
	// table — neither end point is an edge pixel and the walk cannot hit.
	if (edge_count_upper(d, DVP_MIN(x0, x1) - 2, DVP_MIN(y0, y1) - 2, DVP_MAX(x0, x1) + 2, DVP_MAX(y0, y1) + 2) == 0) return false;
	if (edge_bit(d, x0, y0) || edge_bit(d, x1, y1)) return false;
	const int dx = x1 > x0 ? x1 - x0 : x0 - x1, sx = x0 < x1 ? 1 : -1;
	const int dy = y1 > y0 ? y1 - y0 : y0 - y1, sy = y0 < y1 ? 1 : -1;
	int erro = (dx > dy ? dx : dy) / 2;
	int step = 0;
	bool tagx = true, tagy = true;
	bool alive = true;       // the reference's loop would still be running
	while (alive) {
		int wi[8], sh[8];   // word index in the bit-tiled map (-1: outside the image), bit
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			wi[k] = -1;
			sh[k] = 0;
			if (alive) {
				if (x0 == x1) tagx = false;
				if (y0 == y1) tagy = false;
				const int e2 = erro;
				if (e2 > -dx) { erro -= dy; x0 += sx; }
				if (e2 < dy) { erro += dx; y0 += sy; }
				if (x0 >= 0 && x0 < W && y0 >= 0 && y0 < H) {
					wi[k] = tile_word(d.edge_tiles_x, x0, y0);
					sh[k] = x0 & 31;
				}
				step += 1;
				if (step >= max_step || !(tagx || tagy)) alive = false;
			}
		}
		unsigned hit = 0;
#pragma unroll
		for (int k = 0; k < 8; ++k) hit |= (d.edge_bits[wi[k] < 0 ? 0 : wi[k]] >> sh[k]) & (wi[k] < 0 ? 0u : 1u);
		if (hit) return true;
	}
	return false;
}

// The same answer without making every step (round 5).  The reference's walk — e2 = err; if (e2 > -dx) { err -= dy; x += sx; }
// if (e2 < dy) { err += dx; y += sy; }, err0 = max(dx, dy) / 2 — is autonomous: its state after k iterations has a closed
// form (checked against the loop for all dx, dy < 120 and k <= 300, and through the engine's own tests):
//   dx >= dy:  x steps every iteration,  y has stepped floor((k dy + dx - 1 - err0) / dx) times,  err_k = dx - 1 - remainder
//   dx <  dy:  y steps every iteration,  x has stepped min(k, q), q = floor((err0 + k dx + dy - 1) / dy) times
// and it tests the positions after iterations 1 .. N, N = min(max(dx, dy) + 1, max_step) (both end-point flags are down at
// the start of iteration max(dx, dy), which still makes its step: the one-pixel overshoot).  Both coordinates are monotone
// along the walk, so the eight positions of a block lie in the box of its first and last: a block whose box (widened to
// whole 8 x 8 cells: the cell table, four loads) holds no edge pixel is skipped WITHOUT stepping through it; a block that may
// hit restarts the reference's stepping from the closed-form state.  GenNeighbours' searches spent 36 + 14 of their 113 ms per
// cfg3 pass in these walks (tools/gn_ablate.sh), most of it integer stepping through edge-free pixels on the way to the
// one edge that blocks a direction.
DVP_HD int line_div(int n, int dvs, float inv) {   // floor(n / dvs) for 0 <= n < 2^23, dvs >= 1: one multiplication + fix-up
	int q = (int)((float)n * inv);
	const int r = n - q * dvs;
	q += (r >= dvs) ? 1 : 0;
	q -= (r < 0) ? 1 : 0;
	return q;
}
DVP_HD bool bresenham_hits_edge(const Dev& d, int Ax, int Ay, int Bx, int By) {
#if defined(DVP_WALK_STEPS)   // A/B builds: the stepping definition
	return bresenham_hits_edge_steps(d, Ax, Ay, Bx, By);
#endif
	const int W = d.width, H = d.height;
	const int max_step = (int)(DVP_MAX(H, W) / 30.0);
	const int x0 = Bx, y0 = By;
	const int x1 = Ax, y1 = Ay;
	const int ABx = Ax - Bx, ABy = Ay - By;
	if (ABx * ABx + ABy * ABy > 9 * max_step * max_step) return false;
	if (edge_count_upper(d, DVP_MIN(x0, x1) - 2, DVP_MIN(y0, y1) - 2, DVP_MAX(x0, x1) + 2, DVP_MAX(y0, y1) + 2) == 0) return false;
	if (edge_bit(d, x0, y0) || edge_bit(d, x1, y1)) return false;
	const int dx = x1 > x0 ? x1 - x0 : x0 - x1, sx = x0 < x1 ? 1 : -1;
	const int dy = y1 > y0 ? y1 - y0 : y0 - y1, sy = y0 < y1 ? 1 : -1;
	if (dx == 0 && dy == 0) return false;   // the walk never leaves its first pixel, which is not an edge pixel
	const bool xmaj = dx >= dy;
	const int major = xmaj ? dx : dy;
	const int e0 = major / 2;
	const int N = DVP_MIN(major + 1, max_step);
	if (N <= 0) return false;
	const float inv = 1.0f / (float)major;
	// state after k iterations: steps along x and y, the error term
	auto state = [&](int k, int* a, int* b, int* e) {
		if (xmaj) {
			const int n = k * dy + dx - 1 - e0, q = line_div(n, dx, inv);
			*a = k; *b = q; *e = dx - 1 - (n - q * dx);
		} else {
			const int n = e0 + k * dx + dy - 1, q = line_div(n, dy, inv);
			*b = k;
			if (q < k) { *a = q; *e = (n - q * dy) - dy + 1; }
			else { *a = k; *e = e0 + k * (dx - dy); }
		}
	};
	for (int k0 = 1; k0 <= N; k0 += 8) {
		const int k1 = DVP_MIN(k0 + 7, N);
		int a0, b0, e, a1, b1, e1, ap, bp;
		state(k0 - 1, &ap, &bp, &e);   // where the block's first iteration starts
		state(k1, &a1, &b1, &e1);
		{   // first position of the block: one iteration from (ap, bp, e)
			a0 = ap + ((e > -dx) ? 1 : 0);
			b0 = bp + ((e < dy) ? 1 : 0);
		}
		const int xa = x0 + sx * a0, ya = y0 + sy * b0, xb = x0 + sx * a1, yb = y0 + sy * b1;
		if (edge_count_upper(d, DVP_MIN(xa, xb), DVP_MIN(ya, yb), DVP_MAX(xa, xb), DVP_MAX(ya, yb)) == 0) continue;
		// the reference's steps k0 .. k1 from the state after k0 - 1 iterations
		int x = x0 + sx * ap, y = y0 + sy * bp, erro = e;
		int wi[8], sh[8];
#pragma unroll
		for (int j = 0; j < 8; ++j) {
			wi[j] = -1;
			sh[j] = 0;
			if (k0 + j <= k1) {
				const int e2 = erro;
				if (e2 > -dx) { erro -= dy; x += sx; }
				if (e2 < dy) { erro += dx; y += sy; }
				if (x >= 0 && x < W && y >= 0 && y < H) {
					wi[j] = tile_word(d.edge_tiles_x, x, y);
					sh[j] = x & 31;
				}
			}
		}
		unsigned hit = 0;
#pragma unroll
		for (int j = 0; j < 8; ++j) hit |= (d.edge_bits[wi[j] < 0 ? 0 : wi[j]] >> sh[j]) & (wi[j] < 0 ? 0u : 1u);
		if (hit) return true;
	}
	return false;
}

// ---- GenNeighbours (APD.cu:3330-3711) -----------------------------------------------------------
// First third, one lane per WEAK pixel: the directional search (APD.cu:3382-3452).  The search of a direction depends on
// the points found for the directions before it and on how many random tries those consumed, so a pixel is sequential
// here, and the lanes of a wave — neighbouring WEAK pixels — walk the SAME direction at the same time: their tries land
// near each other (measured: letting every lane run through its directions at its own pace costs 50 ms of 80, a wave per
// pixel with the tries over the lanes 6-25 ms).  The list of found points lives in LDS (`pts`, one
// column per lane): as a private array it is scratch memory, re-read for every try's duplicate test — 100 GB of HBM
// fetch per cfg3 launch (FETCH_SIZE, profiles/pmc_r03.json) for 0.2 GB of state.  The label extension (:3455-3560)
// and the plane fit (:3562-3711) are one wave per pixel: gen_neighbours_extend_wave / gen_neighbours_fit_wave.
constexpr int kGnMaxPoints = 160;   // max_pt_num (APD.cu:3338)
constexpr int kGnDirSlots = 32;     // 8 octants x 4 rotations: the directional slots at the head of the list
DVP_HD void gen_neighbours_px(const Dev& d, int px, int py, s2* pts, int stride) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	if (d.weak_info[center] != DVP_WEAK) return;
	const DvpParams& P = d.params;
	const int min_margin = 6;
	const int wi = d.neighbours_map[center];
	s2* neighbours = d.neighbours + (size_t)wi * DVP_NEIGHBOUR_NUM;
	Rng r_limit(d.seed, (uint32_t)center, rng_site(PH_NEIGHBOURS, 0, SUB_LIMIT));
	Rng r_search(d.seed, (uint32_t)center, rng_site(PH_NEIGHBOURS, 0, SUB_SEARCH));

	for (int i = 0; i < DVP_NEIGHBOUR_NUM; ++i) neighbours[i] = mks2(-1, -1);
	neighbours[0] = mks2(px, py);
	// (-1,-1) == not valid (the reference's dir_valid[])
	for (int i = 0; i < kGnDirSlots; ++i) pts[i * stride] = mks2(-1, -1);
	int strong_point_size = 0;
	const int rotate_time = P.rotate_time;

	bool edge_limit = false;
	if (P.use_limit) {
		edge_limit = true;
		if (P.use_edge) {
			const float complex_val = d.complex_[wi];
			const float rp = r_limit.uniform() - FLT_EPSILON;
			if (rp < complex_val) edge_limit = false;
		}
	}

	int odi = -1;
	for (int odx = -1; odx <= 1; ++odx) {
		for (int ody = -1; ody <= 1; ++ody) {
			if (odx == 0 && ody == 0) continue;
			f2 od = mk2((float)odx, (float)ody);
			normalize2(&od);
			odi++;
			for (int rot = 0; rot < rotate_time; ++rot) {
				const int dir_index = odi * 4 + rot;
				// The (radius, try) double loop of APD.cu:3396-3452 as a state machine in two alternating
				// phases: (A) advance through the tries until one passes the cheap tests, (B) the line walk
				// of that try for all lanes of the wave together.  Try order and RNG consumption per lane
				// are unchanged.
				bool found_dir = false, out = false;
				int radius = 2, ri = 0;
				while (!found_dir && !out) {
					bool cand = false;
					s2 np = mks2(-1, -1);
					while (!out) {
						if (ri == 0) {   // entering a new radius: the ray must still be inside the image
							const float tx = px + od.x * radius, ty = py + od.y * radius;
							if (tx < 0 || ty < 0 || tx >= W || ty >= H) { out = true; break; }
						}
						const int cur_radius = radius;
						// advance the state first: the try below may leave the inner loop
						if (++ri == 4) {
							ri = 0;
							radius = DVP_MIN(radius * 2, radius + 25);
							if (radius > 4096) out = true;
						}
						const uint32_t sgx = (r_search.next() % 2 == 0) ? 1u : 0xFFFFFFFFu;
						const int xs = (int)((sgx * r_search.next()) % (uint32_t)d.nb_shift_range);
						const uint32_t sgy = (r_search.next() % 2 == 0) ? 1u : 0xFFFFFFFFu;
						const int ys = (int)((sgy * r_search.next()) % (uint32_t)d.nb_shift_range);
						f2 dir = mk2(od.x * 20 + xs, od.y * 20 + ys);
						normalize2(&dir);
						np = mks2((int)(px + dir.x * cur_radius), (int)(py + dir.y * cur_radius));
						if (np.x < min_margin || np.y < min_margin || np.x >= W - min_margin || np.y >= H - min_margin) continue;
						int npc = np.x + np.y * W;
						if (!strong_bit(d, np.x, np.y)) {   // weak_info[npc] != STRONG, from the L2-resident bit map
							np = d.weak_nearest_strong[npc];
							if (np.x == -1 || np.y == -1) continue;
							npc = np.x + np.y * W;
						}
						// the angle test before the duplicate test (the reference has them the other way round, APD.cu:3425-3440;
						// both only skip the try): the cheap one first
						f2 td = mk2((float)(np.x - px), (float)(np.y - py));
						normalize2(&td);
						const float cos_a = td.x * od.x + td.y * od.y;
						if (!(cos_a > d.nb_thresh)) continue;
						bool same = false;   // (no early exit: the loads are independent and pipeline)
						for (int k = 0; k < dir_index; k++) {
							const s2 q = pts[k * stride];
							same |= (q.x == np.x) & (q.y == np.y);
						}
						if (same) continue;
						cand = true;
						break;
					}
					if (!cand) break;
					if (!edge_limit || !bresenham_hits_edge(d, px, py, np.x, np.y)) {
						pts[dir_index * stride] = np;
						strong_point_size++;
						found_dir = true;
					}
				}
				f2 rd;
				rd.x = od.x * d.nb_cos - od.y * d.nb_sin;
				rd.y = od.x * d.nb_sin + od.y * d.nb_cos;
				normalize2(&rd);
				od = rd;
			}
		}
	}

	// hand-over to the wave-per-pixel rest (below): the 32 directional slots with their holes, and how many are filled
	s2* out = d.gn_points + (size_t)wi * kGnDirSlots;
	for (int i = 0; i < kGnDirSlots; ++i) out[i] = pts[i * stride];
	d.gn_count[wi] = strong_point_size;
}

// NeigbourUpdate (APD.cu:3713-3729)
DVP_HD void neighbour_update_px(const Dev& d, int px, int py) {
	const int center = px + py * d.width;
	if (d.weak_info[center] != DVP_WEAK) return;
	if (d.weak_reliable[center] != 1) d.weak_info[center] = DVP_UNKNOWN;
}

// ---- GenNeighbours, first half (APD.cu:3330-3505): the anchor search, ONE WAVE PER WEAK PIXEL ------------------------
// gen_neighbours_px (above) walks, per lane, 32 directions x a sequence of tries with two to four dependent loads
// each (and a line walk per surviving try): 80 ms per cfg3 pass at 7 % VALU activity, the slowest lane of 64 unrelated
// pixels setting the pace of every direction.  What is sequential in it is only (i) the shared random stream — but a try
// always consumes exactly four draws, so try t of a direction that starts at counter k0 uses k0 + 4 t .. + 3 — and (ii)
// "this point was already found by an earlier direction".  Within ONE direction the tries are therefore independent
// functions of (k0, t): the lanes evaluate tries t0 .. t0 + kGnTries - 1 at once (RNG, candidate point, STRONG test,
// nearest-strong fall-back, duplicate test against the earlier directions, angle test), the edge-limited line walks of
// the surviving tries run eight tries at a time, and the direction takes the FIRST try that passes, exactly like the
// sequential loop; the stream advances by 4 x (tries the sequential loop would have made).  The label-extension points
// are found the same way ((direction, step) items over the lanes) and appended in item order.  Same points, same order,
// same random numbers: the per-lane function stays in the tree as the definition and the tests compare the two.
#ifndef DVP_GN_TRIES
#define DVP_GN_TRIES 64
#endif
constexpr int kGnTries = DVP_GN_TRIES;   // tries of one direction evaluated per round (<= 64)
struct GnShared {
	s2 pts[kGnDirSlots];    // the directional slots (holes = (-1,-1))
	s2 cnp[64];             // the candidate of this lane's try
	uint8_t flag[64];       // 0 = try failed, 1 = try accepted, 2 = the try does not exist, 4 = candidate, line walk pending
};
// first lane < limit whose flag has one of the bits in `mask` (64 = none)
DVP_HD int wave_first_flag(const uint8_t* flag, int mask, int limit) {
#if defined(__HIP_DEVICE_COMPILE__)
	const int l = (int)(threadIdx.x & 63u);
	const unsigned long long m = __ballot(l < limit && (flag[l] & mask) != 0);
	return m ? (int)__builtin_ctzll(m) : 64;
#else
	for (int l = 0; l < limit; ++l) if (flag[l] & mask) return l;
	return 64;
#endif
}
#if defined(DVP_GN_STATS) && !defined(__HIPCC__)
// test instrumentation (tests/emul, -DDVP_GN_STATS): histogram of the try index a direction ends at
struct GnStats { long hist[8] = {0}, found = 0, out = 0; ~GnStats() { fprintf(stderr, "gn tries <1 <4 <8 <16 <32 <64 <128 more: %ld %ld %ld %ld %ld %ld %ld %ld found %ld out %ld\n", hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7], found, out); } };
inline void gn_stats_note(int t, bool found) {
	static GnStats g;
	const int lim[7] = { 1, 4, 8, 16, 32, 64, 128 };
	int b = 7;
	for (int i = 6; i >= 0; --i) if (t < lim[i]) b = i;
#pragma omp critical
	{ g.hist[b]++; if (found) g.found++; else g.out++; }
}
#endif
DVP_HD int gn_radius_of_group(int g) { return g <= 4 ? (2 << g) : 32 + 25 * (g - 4); }   // 2, 4, 8, 16, 32, 57, 82, ... (APD.cu:3449: min(2r, r + 25))

DVP_HD void gen_neighbours_search_wave(const Dev& d, int px, int py, GnShared& sh) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const int min_margin = 6;
	const int wi = d.neighbours_map[center];
	s2* neighbours = d.neighbours + (size_t)wi * DVP_NEIGHBOUR_NUM;
	const uint32_t site_search = rng_site(PH_NEIGHBOURS, 0, SUB_SEARCH);
	DVP_LANES(l) {
		if (l < DVP_NEIGHBOUR_NUM) neighbours[l] = l == 0 ? mks2(px, py) : mks2(-1, -1);
		if (l < 32) sh.pts[l] = mks2(-1, -1);
	}
	wave_sync();
	int strong_point_size = 0;
	const int rotate_time = P.rotate_time;
	bool edge_limit = false;
	if (P.use_limit) {
		edge_limit = true;
		if (P.use_edge) {
			Rng r_limit(d.seed, (uint32_t)center, rng_site(PH_NEIGHBOURS, 0, SUB_LIMIT));
			const float rp = r_limit.uniform() - FLT_EPSILON;
			if (rp < d.complex_[wi]) edge_limit = false;
		}
	}
	uint32_t k0 = 0;   // r_search's counter at the start of the current direction
	int odi = -1;
	for (int odx = -1; odx <= 1; ++odx) {
		for (int ody = -1; ody <= 1; ++ody) {
			if (odx == 0 && ody == 0) continue;
			f2 od = mk2((float)odx, (float)ody);
			normalize2(&od);
			odi++;
			for (int rot = 0; rot < rotate_time; ++rot) {
				const int dir_index = odi * 4 + rot;
				bool resolved = false;
				for (int t0 = 0; !resolved; t0 += kGnTries) {
					DVP_LANES(l) {
						const int t = t0 + l;
						const int cur_radius = gn_radius_of_group(t >> 2);
						uint8_t f = 0;
						s2 np = mks2(-1, -1);
						// the try exists iff its radius group was entered: radius <= 4096 and the ray still inside the image
						const float tx = px + od.x * cur_radius, ty = py + od.y * cur_radius;
						if (l >= kGnTries) f = 0;
						else if (cur_radius > 4096 || tx < 0 || ty < 0 || tx >= W || ty >= H) f = 2;
						else {
							const uint32_t kk = k0 + 4u * (uint32_t)t;
							const uint32_t sgx = (rand_u32(d.seed, (uint32_t)center, site_search, kk) % 2 == 0) ? 1u : 0xFFFFFFFFu;
							const int xs = (int)((sgx * rand_u32(d.seed, (uint32_t)center, site_search, kk + 1)) % (uint32_t)d.nb_shift_range);
							const uint32_t sgy = (rand_u32(d.seed, (uint32_t)center, site_search, kk + 2) % 2 == 0) ? 1u : 0xFFFFFFFFu;
							const int ys = (int)((sgy * rand_u32(d.seed, (uint32_t)center, site_search, kk + 3)) % (uint32_t)d.nb_shift_range);
							f2 dir = mk2(od.x * 20 + xs, od.y * 20 + ys);
							normalize2(&dir);
							np = mks2((int)(px + dir.x * cur_radius), (int)(py + dir.y * cur_radius));
							bool ok = !(np.x < min_margin || np.y < min_margin || np.x >= W - min_margin || np.y >= H - min_margin);
							if (ok && !strong_bit(d, np.x, np.y)) {
								np = d.weak_nearest_strong[np.x + np.y * W];
								ok = !(np.x == -1 || np.y == -1);
							}
							if (ok) {
								bool same = false;
								for (int k = 0; k < dir_index; k++) same |= (sh.pts[k].x == np.x) & (sh.pts[k].y == np.y);
								f2 td = mk2((float)(np.x - px), (float)(np.y - py));
								normalize2(&td);
								const float cos_a = td.x * od.x + td.y * od.y;
								if (!same && cos_a > d.nb_thresh) f = edge_limit ? 4 : 1;
							}
						}
						sh.cnp[l] = np;
						sh.flag[l] = f;
					}
					wave_sync();
					// the sequential loop's outcome: the first try that is accepted (1) or does not exist (2); a pending try (4)
					// in front of it has to be walked first — eight tries per round, most directions end in the first
					int first = 64;
					for (int r0 = 0; r0 < kGnTries; r0 += 8) {
						if (edge_limit) {
							DVP_LANES(l) {
								if (l >= r0 && l < r0 + 8 && sh.flag[l] == 4) {
									const s2 np = sh.cnp[l];
									sh.flag[l] = bresenham_hits_edge(d, px, py, np.x, np.y) ? 0 : 1;
								}
							}
							wave_sync();
						}
						first = wave_first_flag(sh.flag, 3, r0 + 8);
						if (first < 64) break;
					}
#if defined(DVP_GN_STATS) && !defined(__HIPCC__)
					if (first < 64) gn_stats_note(t0 + first, sh.flag[first] == 1);
#endif
					if (first < 64) {
						resolved = true;
						if (sh.flag[first] == 1) {
							const s2 np = sh.cnp[first];
							wave_sync();
							if (DVP_LANE0) sh.pts[dir_index] = np;
							strong_point_size++;
							k0 += 4u * (uint32_t)(t0 + first + 1);
						} else {
							k0 += 4u * (uint32_t)(t0 + first);
						}
					}
					wave_sync();
				}
				f2 rd;
				rd.x = od.x * d.nb_cos - od.y * d.nb_sin;
				rd.y = od.x * d.nb_sin + od.y * d.nb_cos;
				normalize2(&rd);
				od = rd;
			}
		}
	}

	// hand-over: the 32 directional slots with their holes, and how many are filled (the same as gen_neighbours_px)
	s2* out = d.gn_points + (size_t)wi * kGnDirSlots;
	DVP_LANES(l) { if (l < kGnDirSlots) out[l] = sh.pts[l]; }
	if (DVP_LANE0) d.gn_count[wi] = strong_point_size;
}

// ---- GenNeighbours, the label extension (APD.cu:3455-3560): one wave per WEAK pixel --------------------------------
// Points on 16 rays through the pixel's label region, every one mapped to a STRONG pixel and appended to the list unless
// it is in the list already.  The (ray, step) items are independent but for that duplicate test: 64 items per round over
// the lanes, each tested against the list as it stood before the round and against the EARLIER items of the round, then
// appended in item order — the list the reference's sequential loop builds.  `pts` is the list (LDS, kGnMaxPoints
// entries, the first 32 filled by the directional search); returns the index of the last entry, *n_appended how many
// were added.  cnp / flag / keep: 64 entries of shared scratch each.
DVP_HD int gen_neighbours_extend_wave(const Dev& d, int px, int py, int wi, s2* pts, s2* cnp, uint8_t* flag, uint8_t* keep, int* n_appended) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const int min_margin = 6;
	const int rotate_time = P.rotate_time;
	int extend_index = kGnDirSlots - 1;
	int total_appended = 0;
	if (P.use_label && d.label[center] > 0) {
		const int ldx[16] = { 0, 0, -1, 1, -1, 1, -1, 1, 1, 0, 0, -1, -1, 0, 0, 1 };   // APD.cu:3462 (0.5 -> 0)
		const int ldy[16] = { -1, 1, 0, 0, -1, 1, 1, -1, 0, 1, 1, 0, 0, -1, -1, 0 };
		const s2* lb = d.label_boundary + (size_t)wi * 8;
		float bound_dist[16];
		int dir_step[16];
#pragma unroll
		for (int i = 0; i < 16; ++i) { bound_dist[i] = 0.0f; dir_step[i] = 0; }
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			const s2 bp = lb[i];
			float dist = 0.0f;
			if (bp.x != -1 && bp.y != -1) {
				const double ex = (double)(px - bp.x), ey = (double)(py - bp.y);
				dist = (float)sqrt(ex * ex + ey * ey);
				if (i >= 4) dist = (float)((double)dist / sqrt(2.0));
			}
			bound_dist[i] = dist;
			if (i % 2 == 1) { dir_step[i - 1] = 4 * rotate_time - 1; dir_step[i] = 1; }   // APD.cu:3477: step == 1
		}
		const int ca[8] = { 3, 1, 1, 2, 2, 4, 7, 7 };
		const int cb[8] = { 5, 5, 6, 6, 4, 0, 0, 3 };
#pragma unroll
		for (int q = 0; q < 8; ++q) {
			dir_step[8 + q] = (dir_step[ca[q]] + dir_step[cb[q]]) / 2;
			bound_dist[8 + q] = (bound_dist[ca[q]] + bound_dist[cb[q]]) / 2;
		}
		int n_items = 0;     // items = (direction i, step 1 .. dir_step[i]) in the reference's loop order
#pragma unroll
		for (int i = 0; i < 16; ++i) n_items += dir_step[i] > 0 ? dir_step[i] : 0;
		for (int c0 = 0; c0 < n_items; c0 += 64) {
			DVP_LANES(l) {
				const int c = c0 + l;
				uint8_t f = 0;
				s2 np = mks2(-1, -1);
				if (c < n_items) {
					int first = 0, step = 0, step_len = 1, ddx = 0, ddy = 0;   // (a select chain: the tables stay in registers)
#pragma unroll
					for (int i = 0; i < 16; ++i) {
						const int n = dir_step[i] > 0 ? dir_step[i] : 0;
						if (c >= first && c < first + n) {
							step = c - first + 1;
							step_len = DVP_MAX(1, (int)floor(1.0 * bound_dist[i] / (dir_step[i] + 1)));
							ddx = ldx[i];
							ddy = ldy[i];
						}
						first += n;
					}
					np = mks2(px + step * step_len * ddx, py + step * step_len * ddy);
					bool ok = !(np.x < min_margin || np.y < min_margin || np.x >= W - min_margin || np.y >= H - min_margin);
					if (ok && !strong_bit(d, np.x, np.y)) {
						np = d.weak_nearest_strong[np.x + np.y * W];
						ok = !(np.x == -1 || np.y == -1);
					}
					if (ok) {
						bool same = false;      // against everything accepted before this batch ...
						for (int k = 0; k <= extend_index; k++) same |= (pts[k].x == np.x) & (pts[k].y == np.y);
						if (!same) f = 1;
					}
				}
				cnp[l] = np;
				flag[l] = f;
			}
			wave_sync();
			DVP_LANES(l) {
				// ... and against the earlier items of the batch: the first occurrence of a point is the one the sequential
				// loop appends (an earlier equal item that was itself dropped had an even earlier equal one)
				const s2 np = cnp[l];
				bool kp = flag[l] == 1;
				for (int q = 0; q < l; ++q) kp &= !((flag[q] == 1) & (cnp[q].x == np.x) & (cnp[q].y == np.y));
				keep[l] = kp ? 1 : 0;
			}
			wave_sync();
			int appended = 0;
			DVP_LANES(l) {
				int before = 0, total = 0;    // kept items in front of this one / in the batch
#if defined(__HIP_DEVICE_COMPILE__)
				{
					const unsigned long long m = __ballot(keep[l] != 0);
					total = __popcll(m);
					before = __popcll(m & ((1ull << l) - 1ull));
				}
#else
				for (int k = 0; k < 64; ++k) { total += keep[k]; before += k < l ? keep[k] : 0; }
#endif
				const int pos = extend_index + 1 + before;
				if (keep[l] && pos < kGnMaxPoints) pts[pos] = cnp[l];
				appended = DVP_MIN(total, kGnMaxPoints - 1 - extend_index);
			}
			wave_sync();
			extend_index += appended;
			total_appended += appended;
		}
	}
	*n_appended = total_appended;
	return extend_index;
}

// ---- GenNeighbours, second half (APD.cu:3562-3711): RANSAC plane through the candidate anchors, then the
// anchors ranked by their distance to that plane — ONE WAVE per WEAK pixel.
//
// A pixel per lane keeps its 160-entry point tables in scratch and reads them at random indices for 200
// draws: 64 lanes x divergent indices = one cache sector per access, 600 GB of fetches per launch at
// 6208x4128 with the vector ALUs 28 % busy.  Here the tables of one pixel live in LDS and the wave splits
// the work that is independent:
//   1. the 200 draws (index triples + the cheap rejections) — the RNG is counter-based and every draw
//      consumes exactly three numbers, so draw t owns counters 3t..3t+2;
//   2. in draw order (cheap, every lane in step): which unordered pairs need a line test and in which
//      orientation they are asked FIRST — the reference caches the test per pair, symmetric, first asker
//      wins (APD.cu:3574, 3588-3604);
//   3. the line walks, one per lane;
//   4. per draw: plane, label test, inlier count, distance of the pixel's own depth to the plane;
//   5. in draw order (every lane in step): the reference's running best (APD.cu:3646-3668);
//   6. residuals of all points, their stable rank by residual (== the reference's insertion sort,
//      APD.cu:125-138), neighbours[1..11].
constexpr int kGnDraws = 200;
constexpr int kGnPairWords = (kGnMaxPoints * (kGnMaxPoints - 1) / 2 + 31) / 32;
struct FitShared {
	uint8_t slot_of[kGnMaxPoints]; // valid point j -> index in raw
	s2 spv[kGnMaxPoints];
	f3 sp3[kGnMaxPoints];          // camera-frame 3-D point
	f2 fxy[kGnMaxPoints];          // ((x - cx) / fx, (y - cy) / fy)
	union { s2 raw[kGnMaxPoints]; float weight[kGnMaxPoints]; };   // the list as handed over (holes = (-1,-1)), dead once the tables are built; then the residuals
	uint32_t trip[kGnDraws];       // a | b << 8 | c << 16 | passed << 24
	uint32_t seen[kGnPairWords];   // unordered pair already queued for its line test
	uint32_t hit[kGnPairWords];    // ... and the test found an edge pixel
	uint16_t walk[3 * kGnDraws];   // queued tests: from | to << 8 (orientation of the first asker)
	float cand_dist[kGnDraws];
	int cand_info[kGnDraws];       // bit 0 valid, bit 1 "strong plane", bits 8..: inlier count
	uint8_t plist[kGnDraws];       // draws that passed the index and triangle tests, in draw order
	int req_idx[64], mark[64];     // one batch of line-test requests: pair index / pair to mark
	uint8_t req_from[64], req_to[64];
	int part_t[64];                // per-lane winner of the running best
	uint8_t part_nan[64];
	int n_pass, n_walk, n_valid;
};

// The RANSAC inlier test is `|fit_depth - z| / depth_diff < ransac_threshold` (APD.cu:3632) — one IEEE division per (candidate
// plane, point) in the hottest loop of the launch (44 % of dvp_gen_neighbours_fit at 25 % WEAK, tools/ab_variant_trace.sh with
// -DDVP_ABL_FIT=4), by the SAME positive divisor every time.  x -> fl(x / d) is monotone for d > 0 (correct rounding keeps
// order), so { x >= 0 : fl(x / d) < t } is an initial segment of the floats: the test is x <= X* with X* = its largest element
// — found once per pixel from the guess t * d by stepping to the neighbouring floats, the division itself deciding.  Same
// decisions, bit for bit (NaN fails both forms).  Returns -1 when no x >= 0 passes.
DVP_HD float largest_ratio_below(float d, float t) {
	if (!(t > 0.0f)) return -1.0f;
	const float g = t * d;
	uint32_t b = (g >= 0.0f && g <= FLT_MAX) ? f32_bits(g) : 0x7F7FFFFFu;   // start at t * d (FLT_MAX if that overflows)
	while (b > 0u && !(__builtin_bit_cast(float, b) / d < t)) --b;
	while (b < 0x7F7FFFFFu && (__builtin_bit_cast(float, b + 1u) / d < t)) ++b;
	return __builtin_bit_cast(float, b);   // (0 / d = 0 < t: the set is never empty here)
}

// plane through three camera-frame points, as the candidate step builds it (APD.cu:3609-3622)
DVP_HD f4 gn_plane(const f3 A, const f3 B, const f3 C) {
	const f3 AC = mk3(A.x - C.x, A.y - C.y, A.z - C.z);
	const f3 BC = mk3(B.x - C.x, B.y - C.y, B.z - C.z);
	f4 cv;
	cv.x = AC.y * BC.z - BC.y * AC.z;
	cv.y = -(AC.x * BC.z - BC.x * AC.z);
	cv.z = AC.x * BC.y - BC.x * AC.y;
	cv.w = 0.0f;
	return cv;
}
DVP_HD int gn_pair_index(int a, int b) { const int hi = a > b ? a : b, lo = a > b ? b : a; return hi * (hi - 1) / 2 + lo; }

// the plane of candidate draw t again (same operations on the same operands as the candidate step)
DVP_HD f4 cand_plane_of(const FitShared& sh, int t) {
	const uint32_t tr = sh.trip[t];
	const f3 A = sh.sp3[tr & 255u];
	f4 cv = gn_plane(A, sh.sp3[(tr >> 8) & 255u], sh.sp3[(tr >> 16) & 255u]);
	normalize3(&cv);
	cv.w = -(cv.x * A.x + cv.y * A.y + cv.z * A.z);
	return cv;
}

DVP_HD void gen_neighbours_fit_wave(const Dev& d, int px, int py, FitShared& sh) {
	const int W = d.width;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const int wi = d.neighbours_map[center];
	// ---- the list: the directional slots from the search kernel, then the label extension -------------------------
	DVP_LANES(l) { if (l < kGnDirSlots) sh.raw[l] = d.gn_points[(size_t)wi * kGnDirSlots + l]; }
	wave_sync();
	int n_extended = 0;
#if defined(DVP_ABL_FIT) && DVP_ABL_FIT == 1   // timing ablation (wrong results): no label extension
	const int listed = kGnDirSlots;
#else
	const int listed = 1 + gen_neighbours_extend_wave(d, px, py, wi, sh.raw, sh.spv, sh.req_from, sh.req_to, &n_extended);
#endif
	if (d.gn_count[wi] + n_extended <= 3) {   // fewer than four candidates (APD.cu:3562): not reliable, no plane
		if (DVP_LANE0) d.weak_reliable[center] = 0;
		return;
	}
	const DvpCamera cam = load_camera(d, 0);
	const float depth_diff = P.depth_max - P.depth_min;
	const bool by_limit = depth_diff > 0.0f;   // (else: the division, whatever it yields)
	const float inlier_limit = by_limit ? largest_ratio_below(depth_diff, P.ransac_threshold) : 0.0f;
	s2* neighbours = d.neighbours + (size_t)wi * DVP_NEIGHBOUR_NUM;
	const uint32_t site = rng_site(PH_NEIGHBOURS, 0, SUB_RANSAC);
	bool edge_limit = false;   // same draw as in the first half (APD.cu:3366-3374)
	if (P.use_limit) {
		edge_limit = true;
		if (P.use_edge) {
			Rng r_limit(d.seed, (uint32_t)center, rng_site(PH_NEIGHBOURS, 0, SUB_LIMIT));
			if (r_limit.uniform() - FLT_EPSILON < d.complex_[wi]) edge_limit = false;
		}
	}

	// ---- the point tables -------------------------------------------------------------------------------
	if (DVP_LANE0) sh.n_valid = 0;
	wave_sync();
	for (int i0 = 0; i0 < listed; i0 += 64) {
		DVP_LANES(l) {
			s2 r = mks2(-1, -1);
			if (i0 + l < listed) r = sh.raw[i0 + l];
			const bool valid = r.x != -1;
			const int slot = wave_ordered_slot(valid, &sh.n_valid);   // the list without its holes, order kept
			if (valid) sh.slot_of[slot] = (uint8_t)(i0 + l);
		}
	}
	wave_sync();
	const int valid_count = sh.n_valid;
	for (int j0 = 0; j0 < valid_count; j0 += 64) {
		DVP_LANES(l) {
			const int j = j0 + l;
			if (j >= valid_count) continue;
			const s2 sp = sh.raw[sh.slot_of[j]];
			const f4 pl = d.planes[sp.x + sp.y * W];
			float X[3];
			get_3d_point(cam, sp.x, sp.y, pl.w, X);
			sh.spv[j] = sp;
			sh.sp3[j] = mk3(X[0], X[1], X[2]);
			sh.fxy[j] = mk2((sp.x - cam.K[2]) / cam.K[0], (sp.y - cam.K[5]) / cam.K[4]);
		}
	}
	float Xc[3];
	get_3d_point(cam, px, py, d.planes[center].w, Xc);
	const float center_z = Xc[2];
	DVP_LANES(l) { for (int i = l; i < kGnPairWords; i += 64) { sh.seen[i] = 0u; sh.hit[i] = 0u; } sh.mark[l] = -1; }
	wave_sync();

	// ---- 1. the draws; the ones that pass the index and triangle tests are queued ----------------------------
	if (DVP_LANE0) { sh.n_pass = 0; sh.n_walk = 0; }
	wave_sync();
	for (int t0 = 0; t0 < kGnDraws; t0 += 64) {
		DVP_LANES(l) {
			const int t = t0 + l;
			bool pass = false;
			if (t < kGnDraws) {
				const int ai = (int)(rand_u32(d.seed, (uint32_t)center, site, 3u * t) % (uint32_t)valid_count);
				const int bi = (int)(rand_u32(d.seed, (uint32_t)center, site, 3u * t + 1u) % (uint32_t)valid_count);
				const int ci = (int)(rand_u32(d.seed, (uint32_t)center, site, 3u * t + 2u) % (uint32_t)valid_count);
				pass = !(ai == bi || bi == ci || ai == ci) && point_in_triangle(sh.spv[ai], sh.spv[bi], sh.spv[ci], px, py);
				sh.trip[t] = (uint32_t)ai | ((uint32_t)bi << 8) | ((uint32_t)ci << 16) | (pass ? 1u << 24 : 0u);
				sh.cand_info[t] = 0;
			}
			const int slot = wave_ordered_slot(pass, &sh.n_pass);   // plist in draw order
			if (pass) sh.plist[slot] = (uint8_t)t;
		}
	}
	wave_sync();
	const int n_pass = sh.n_pass;
	// ---- 2. + 3. line tests: who asks first, then the walks -----------------------------------------------------
	// Requests in the reference's order: draw t asks (a,b), (b,c), (c,a).  64 requests at a time: a request is
	// a first asker when its pair is neither marked from an earlier batch nor asked by a lower lane of this
	// batch; first askers mark the pair and queue the walk in THEIR orientation.
#if defined(DVP_ABL_FIT) && DVP_ABL_FIT == 2   // timing ablation: no line tests at all (requests + walks)
	if (false) {
#else
	if (edge_limit) {
#endif
		for (int r0 = 0; r0 < 3 * n_pass; r0 += 64) {   // only the draws that passed ask; plist keeps their order
			DVP_LANES(l) {
				const int r = r0 + l, j = r / 3, e = r - 3 * j;
				int idx = -1;
				if (r < 3 * n_pass) {
					const uint32_t tr = sh.trip[sh.plist[j]];
					const int p[4] = { (int)(tr & 255u), (int)((tr >> 8) & 255u), (int)((tr >> 16) & 255u), (int)(tr & 255u) };
					idx = gn_pair_index(p[e], p[e + 1]);
					sh.req_from[l] = (uint8_t)p[e];
					sh.req_to[l] = (uint8_t)p[e + 1];
				}
				sh.req_idx[l] = idx;
			}
			wave_sync();
			DVP_LANES(l) {
				const int idx = sh.req_idx[l];
				if (idx < 0 || ((sh.seen[idx >> 5] >> (idx & 31)) & 1u)) continue;
				bool dup = false;
				for (int m = 0; m < l; ++m) dup = dup || sh.req_idx[m] == idx;
				if (dup) continue;
				sh.walk[wave_counter_add(&sh.n_walk)] = (uint16_t)(sh.req_from[l] | (sh.req_to[l] << 8));
				sh.mark[l] = idx;
			}
			wave_sync();
			DVP_LANES(l) {   // marks after every lane of the batch has looked at the old state
				const int idx = sh.mark[l];
				if (idx >= 0) { wave_bits_or(&sh.seen[idx >> 5], 1u << (idx & 31)); sh.mark[l] = -1; }
			}
			wave_sync();
		}
#if defined(DVP_ABL_FIT) && DVP_ABL_FIT == 3   // timing ablation: requests, but no walks
		const int n_walk = 0;
#else
		const int n_walk = sh.n_walk;
#endif
		for (int j0 = 0; j0 < n_walk; j0 += 64) {
			DVP_LANES(l) {
				const int j = j0 + l;
				if (j >= n_walk) continue;
				const int a = sh.walk[j] & 255, b = sh.walk[j] >> 8;
				if (bresenham_hits_edge(d, sh.spv[a].x, sh.spv[a].y, sh.spv[b].x, sh.spv[b].y)) {
					const int idx = gn_pair_index(a, b);
					wave_bits_or(&sh.hit[idx >> 5], 1u << (idx & 31));
				}
			}
		}
		wave_sync();
	}
	// ---- 4. candidates: one queued draw per lane ------------------------------------------------------------------
	const bool label_test = P.use_label && d.label[center] > 0;
	const float fxc = (px - cam.K[2]) / cam.K[0], fyc = (py - cam.K[5]) / cam.K[4];
	for (int j0 = 0; j0 < n_pass; j0 += 64) {
		DVP_LANES(l) {
			if (j0 + l >= n_pass) continue;
			const int t = sh.plist[j0 + l];
			const uint32_t tr = sh.trip[t];
			const int ai = (int)(tr & 255u), bi = (int)((tr >> 8) & 255u), ci = (int)((tr >> 16) & 255u);
			if (edge_limit) {
				const int i0 = gn_pair_index(ai, bi), i1 = gn_pair_index(bi, ci), i2 = gn_pair_index(ci, ai);
				if (((sh.hit[i0 >> 5] >> (i0 & 31)) | (sh.hit[i1 >> 5] >> (i1 & 31)) | (sh.hit[i2 >> 5] >> (i2 & 31))) & 1u) continue;
			}
			// camera-frame normal of point a — the reference uses a_index for all three normals (APD.cu:3605-3607);
			// fetched again from the plane map instead of a 2 KB table (a third workgroup per CU fits)
			const f4 AN = normal_world_to_cam(cam, d.planes[sh.spv[ai].x + sh.spv[ai].y * W]);
			if (AN.x * AN.x + AN.y * AN.y + AN.z * AN.z < 0.9f) continue;
			const f3 A = sh.sp3[ai];
			f4 cv = gn_plane(A, sh.sp3[bi], sh.sp3[ci]);
			if ((cv.x == 0 && cv.y == 0 && cv.z == 0) || cv.x != cv.x || cv.y != cv.y || cv.z != cv.z) continue;
			normalize3(&cv);
			cv.w = -(cv.x * A.x + cv.y * A.y + cv.z * A.z);
			const bool strong = !(label_test && fabsf(AN.x * cv.x + AN.y * cv.y + AN.z * cv.z) < 0.9f);
			int count = 0;
#if defined(DVP_ABL_FIT) && DVP_ABL_FIT == 4   // timing ablation: no inlier loop
			for (int si = 0; si < 0; ++si) {
#else
			if (by_limit) {   // (two loops: as one loop with the choice inside, both forms are computed and selected)
				for (int si = 0; si < valid_count; ++si) {
					const f2 f = sh.fxy[si];
					const float fit_depth = -cv.w / (cv.x * f.x + cv.y * f.y + cv.z);
					if (fabsf(fit_depth - sh.sp3[si].z) <= inlier_limit) count++;
				}
			} else
			for (int si = 0; si < valid_count; ++si) {
#endif
				const f2 f = sh.fxy[si];
				const float fit_depth = -cv.w / (cv.x * f.x + cv.y * f.y + cv.z);
				if (fabsf(fit_depth - sh.sp3[si].z) / depth_diff < P.ransac_threshold) count++;
			}
			const float fit_depth = -cv.w / (cv.x * fxc + cv.y * fyc + cv.z);
			sh.cand_dist[t] = fabsf(fit_depth - center_z);
			sh.cand_info[t] = 1 | (strong ? 2 : 0) | (count << 8);
		}
	}
	wave_sync();
	// ---- 5. the running best, in draw order (APD.cu:3646-3668) ------------------------------------------------------
	// The reference's update rule — a candidate with at least 6 inliers replaces the best one when it has
	// more inliers, or as many and a strictly smaller distance, and the FIRST "strong" candidate replaces
	// whatever came before, after which only strong ones are looked at — selects, among the strong
	// candidates if there is one (else among all), the one with (most inliers, then smallest distance, then
	// earliest draw).  Every lane folds the draws t = l, l + 64, ... that way, then the 64 partial winners are
	// folded.  A NaN distance does not obey that order: then the scan is done literally.
	f4 best_plane = mk4(0, 0, 0, 0);
	bool has_valid_plane = false;
	{
		DVP_LANES(l) {
			int bt = -1, bstrong = 0, bcount = 0;
			float bdist = 0.0f;
			bool nan = false;
			for (int t = l; t < kGnDraws; t += 64) {
				const int info = sh.cand_info[t];
				if (!(info & 1) || (info >> 8) < 6) continue;
				const int strong = (info >> 1) & 1, count = info >> 8;
				const float dist = sh.cand_dist[t];
				nan = nan || dist != dist;
				if (bt < 0 || strong > bstrong || (strong == bstrong && (count > bcount || (count == bcount && dist < bdist)))) { bt = t; bstrong = strong; bcount = count; bdist = dist; }
			}
			sh.part_t[l] = bt;
			sh.part_nan[l] = nan ? 1 : 0;
		}
		wave_sync();
		bool nan = false;
		int bt = -1, bstrong = 0, bcount = 0;
		float bdist = 0.0f;
		for (int m = 0; m < 64; ++m) {
			nan = nan || sh.part_nan[m] != 0;
			const int t = sh.part_t[m];
			if (t < 0) continue;
			const int info = sh.cand_info[t];
			const int strong = (info >> 1) & 1, count = info >> 8;
			const float dist = sh.cand_dist[t];
			const bool better = bt < 0 || strong > bstrong || (strong == bstrong && (count > bcount || (count == bcount && (dist < bdist || (dist == bdist && t < bt)))));
			if (better) { bt = t; bstrong = strong; bcount = count; bdist = dist; }
		}
		if (!nan) {
			if (bt >= 0) { best_plane = cand_plane_of(sh, bt); has_valid_plane = true; }
		} else {
			bool has_strong_plane = false;
			float min_cost = FLT_MAX;
			int max_count = 3;
			for (int t = 0; t < kGnDraws; ++t) {
				const int info = sh.cand_info[t];
				if (!(info & 1)) continue;
				const bool strong = (info & 2) != 0;
				if (has_strong_plane && !strong) continue;
				const int count = info >> 8;
				if (count < 6) continue;
				const float center_distance = sh.cand_dist[t];
				if (count > max_count || (!has_strong_plane && strong)) {
					if (!has_strong_plane && strong) has_strong_plane = true;
					best_plane = cand_plane_of(sh, t);
					max_count = count;
					min_cost = center_distance;
					has_valid_plane = true;
				} else if (count == max_count) {
					if (center_distance < min_cost) { best_plane = cand_plane_of(sh, t); max_count = count; min_cost = center_distance; }
				}
			}
		}
	}
	if (!has_valid_plane) { if (DVP_LANE0) d.weak_reliable[center] = 0; return; }
	// ---- 6. residuals, stable rank, neighbours ---------------------------------------------------------------------
	for (int j0 = 0; j0 < valid_count; j0 += 64) {
		DVP_LANES(l) {
			const int j = j0 + l;
			if (j >= valid_count) continue;
			const f2 f = sh.fxy[j];
			const float fit_depth = -best_plane.w / (best_plane.x * f.x + best_plane.y * f.y + best_plane.z);
			const float dist = fabsf(fit_depth - sh.sp3[j].z);
			sh.weight[j] = (by_limit ? dist > inlier_limit : dist / depth_diff >= P.ransac_threshold) ? FLT_MAX : dist;
		}
	}
	wave_sync();
	bool any_nan = false;   // a NaN residual (0/0 in the plane equation) has no rank: take the reference's insertion sort literally
	for (int i = 0; i < valid_count; ++i) any_nan = any_nan || sh.weight[i] != sh.weight[i];
	if (any_nan) {
		DVP_LANES(l) {
			if (l != 0) continue;
			for (int i = 0; i < valid_count; ++i)
				if (sh.weight[i] == FLT_MAX) sh.spv[i] = mks2(-1, -1);
			for (int i = 1; i < valid_count; i++) {   // sort_small_weighted (APD.cu:125-138)
				const s2 tp = sh.spv[i];
				const float tw = sh.weight[i];
				int j = i;
				for (; j >= 1 && tw < sh.weight[j - 1]; j--) { sh.spv[j] = sh.spv[j - 1]; sh.weight[j] = sh.weight[j - 1]; }
				sh.spv[j] = tp;
				sh.weight[j] = tw;
			}
			for (int i = 1; i < DVP_NEIGHBOUR_NUM; ++i) neighbours[i] = (i - 1 < valid_count) ? sh.spv[i - 1] : mks2(-1, -1);
			d.weak_reliable[center] = 1;
		}
		return;
	}
	for (int j0 = 0; j0 < valid_count; j0 += 64) {
		DVP_LANES(l) {
			const int j = j0 + l;
			if (j >= valid_count) continue;
			const float w = sh.weight[j];
			int rank = 0;
			for (int i = 0; i < valid_count; ++i) {
				const float wi_ = sh.weight[i];
				rank += (wi_ < w || (wi_ == w && i < j)) ? 1 : 0;
			}
			if (rank < DVP_NEIGHBOUR_NUM - 1) neighbours[1 + rank] = (w == FLT_MAX) ? mks2(-1, -1) : sh.spv[j];
		}
	}
	if (DVP_LANE0) d.weak_reliable[center] = 1;
}

}  // namespace dvp
#endif
