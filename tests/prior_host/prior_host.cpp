// Host build of the device plane prior (dvp-mvs_amd/csrc/dvp_prior.hpp + dvp_prior_mid.hpp), one item after the other (TEST
// INFRASTRUCTURE): lets the CPU tests hold the kernels' arithmetic and their decomposition of the sweep — one counter sequence
// per triangle, an owner map, one pass over the pixels — against the numpy model and the host mirror's BuildPlanePrior without a
// GPU.  Same text, same build flags for the arithmetic (-ffp-contract=off) as dvp_prior.hip.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_prior_mid.hpp"

using dvpprior::Tri;

// The host part.  cam: K[9], R[9], t[3] of the camera file.  Returns the status of dvp_plane_prior (0: usable, 1: not); *count
// = the swept triangles, of which the first min(*count, capacity) are written to out (40 bytes each: six int32 corners, three
// float rates, the float step); skipped[3]: how often each skip rule fired.
extern "C" int dvp_prior_triangles_serial(const float* raw, int cols, int rows, const float* xy, const float* xyz, int n, const float* K, const float* R, const float* t,
                                          float* middle_rate, Tri* out, int capacity, int* count, long long* skipped) {
	std::vector<Tri> tris;
	size_t sk[3] = { 0, 0, 0 };
	*count = 0;
	if (!dvppriormid::PriorTriangles(raw, cols, rows, xy, xyz, n > 0 ? (size_t)n : 0, K, R, t, middle_rate, &tris, sk)) return 1;
	*count = (int)tris.size();
	for (size_t i = 0; i < tris.size() && (int)i < capacity; ++i) out[i] = tris[i];
	if (skipped) for (int k = 0; k < 3; ++k) skipped[k] = (long long)sk[k];
	return 0;
}

// dvp_prior_sequences + dvp_prior_owners: owner is cols x rows.  Returns the number of sweep rows over all triangles.
extern "C" long long dvp_prior_owner_serial(const Tri* tris, int T, int cols, int rows, int32_t* owner) {
	for (size_t i = 0; i < (size_t)cols * rows; ++i) owner[i] = -1;
	long long total = 0;
	std::vector<float> seq;
	for (int t = 0; t < T; ++t) {
		const unsigned n = dvpprior::seq_count(tris[t].step);
		seq.resize(n);
		float s = 0;
		for (unsigned k = 0; k < n; ++k) { seq[k] = s; s = dvpprior::seq_next(s, tris[t].step); }
		total += n;
		for (unsigned i = 0; i < n; ++i)
			for (unsigned j = 0; j < n; ++j) {
				if (!dvpprior::column_exists(seq[i], seq[j])) break;
				const int x = dvpprior::sweep_coord(seq[i], seq[j], tris[t].x1, tris[t].x2, tris[t].x3);
				const int y = dvpprior::sweep_coord(seq[i], seq[j], tris[t].y1, tris[t].y2, tris[t].y3);
				if (x >= 0 && x < cols && y >= 0 && y < rows && owner[(size_t)y * cols + x] < t) owner[(size_t)y * cols + x] = t;
			}
	}
	return total;
}

extern "C" void dvp_prior_rate_serial(const Tri* tris, const int32_t* owner, float middle_rate, int cols, int rows, float* rate) {
	for (int y = 0; y < rows; ++y)
		for (int x = 0; x < cols; ++x) rate[(size_t)y * cols + x] = dvpprior::rate_at(tris, owner[(size_t)y * cols + x], middle_rate, x, y);
}

extern "C" void dvp_prior_depth_serial(const float* raw, const float* rate, int cols, int rows, int W, int H, float* depth) {
	const float scale_x = W / static_cast<float>(cols), scale_y = H / static_cast<float>(rows);
	for (int r = 0; r < H; ++r)
		for (int c = 0; c < W; ++c) depth[(size_t)r * W + c] = dvpprior::working_depth(raw, rate, cols, rows, scale_x, scale_y, r, c);
}

// planes: W * H * 4 floats (world normal, depth)
extern "C" void dvp_prior_planes_serial(const float* depth, int W, int H, const float* K, const float* R, float* planes) {
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) {
			const dvpprior::P4 p = dvpprior::plane_at(depth, W, H, K, R, x, y);
			float* o = planes + 4 * ((size_t)y * W + x);
			o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.w;
		}
}
