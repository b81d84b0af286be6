// dvp_pairs.hpp — the two numeric steps of `apd --convert-from` (the reference's colmap2mvsnet.py) as per-item functions for the
// device (dvp_pairs.hip) and, the same text, for the host (`--convert-on host`, tests/convert_host):
//   view-selection scores (calc_score, colmap2mvsnet.py:280-302).  For i < j: S = the entries of image i's point list that are not
//     -1 and occur in image j's list (a duplicate in i counts each time); per such entry the angle at the point between the two
//     camera centres; the score is S, or 0 when S > 0 and the element at int(S * 0.75) of the sorted angles is below 1 degree.
//     With L = how many of the S angles are below 1 that element is below 1 iff L > (3 * S) >> 2: no sort, and the matrix is two
//     integer count matrices filled point by point.  A point's track is {(image a, multiplicity m_a)}, sorted by image; for every
//     a < b in it cnt[a][b] += m_a, and low[a][b] += m_a when the angle is below 1.  Integer sums: the same matrix whatever the
//     order of the items.
//   the written image (colmap2mvsnet.py:462-469): zero padding on the right and bottom to the set's largest size, then
//     cv::resize(INTER_NEAREST) with OpenCV's index rule in double.
// Binary64 arithmetic is one IEEE rounding per operator (-ffp-contract=off) in the reference's operand order.
// Departure: the cosine is clamped to [-1, 1] before acos.  The reference gets NaN there and sorts a list that holds it, whose
// order Python does not define.  A point at a camera centre still gives NaN (0 / 0): it counts towards S and never towards L.
#ifndef DVP_PAIRS_HPP_
#define DVP_PAIRS_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DVP_PHD __host__ __device__ inline
#else
#define DVP_PHD inline
#endif

#include <algorithm>
#include <string>
#include <vector>

namespace dvppairs {

// (180 / pi) * arccos(dot(ci - p, cj - p) / |ci - p| / |cj - p|) < 1   (colmap2mvsnet.py:293)
DVP_PHD bool angle_below_one(const double* ci, const double* cj, const double* p) {
	const double u0 = ci[0] - p[0], u1 = ci[1] - p[1], u2 = ci[2] - p[2];
	const double v0 = cj[0] - p[0], v1 = cj[1] - p[1], v2 = cj[2] - p[2];
	const double dot = u0 * v0 + u1 * v1 + u2 * v2;
	const double nu = sqrt(u0 * u0 + u1 * u1 + u2 * u2), nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
	double c = dot / nu / nv;
	if (c > 1.0) c = 1.0;
	if (c < -1.0) c = -1.0;
	return (180 / 3.141592653589793) * acos(c) < 1;
}

// The tracks as a CSR array: elements off[k] .. off[k + 1] belong to point `point[e]` = k, in ascending image order.
struct Tracks {
	const uint32_t* off;     // num_points + 1
	const uint32_t* point;   // per element: its point
	const uint32_t* image;   // per element
	const uint32_t* mult;    // per element: how often the image's list names the point
	const double* xyz;       // per point
	const double* centres;   // per image
};

// element e of a track against element f > e of the same track
template <class Add>
DVP_PHD void pair_item(const Tracks& t, uint32_t e, uint32_t f, int N, uint32_t* cnt, uint32_t* low, const Add& add) {
	const uint32_t a = t.image[e], b = t.image[f], m = t.mult[e];
	const size_t at = (size_t)a * (size_t)N + b;
	add(cnt + at, m);
	if (angle_below_one(t.centres + 3 * (size_t)a, t.centres + 3 * (size_t)b, t.xyz + 3 * (size_t)t.point[e])) add(low + at, m);
}

// entry (i, j) of the symmetric matrix from the upper triangles of the counts
DVP_PHD uint32_t score_at(const uint32_t* cnt, const uint32_t* low, int N, int i, int j) {
	if (i == j) return 0;
	const size_t at = i < j ? (size_t)i * (size_t)N + j : (size_t)j * (size_t)N + i;
	const uint32_t S = cnt[at], L = low[at];
	return (S > 0 && (unsigned long long)L > ((3ull * S) >> 2)) ? 0u : S;
}

// cv::resize(INTER_NEAREST)'s source index of destination index d: fx = 1.0 / ((double)dst_n / src_n)
DVP_PHD int nearest_source(int d, int dst_n, int src_n) {
	const double f = 1.0 / ((double)dst_n / src_n);
	const int s = (int)floor(d * f);
	return s < src_n - 1 ? s : src_n - 1;
}
// byte k of row y of the written image (k = 3 * x + channel): the w x h picture padded with zeros to pad_w x pad_h, resampled
DVP_PHD uint8_t converted_byte(const uint8_t* bgr, int w, int h, size_t pitch, int pad_w, int pad_h, int out_w, int out_h, int k, int y) {
	const int x = k / 3, c = k - 3 * x;
	const int sx = nearest_source(x, out_w, pad_w), sy = nearest_source(y, out_h, pad_h);
	return (sx < w && sy < h) ? bgr[(size_t)sy * pitch + 3 * (size_t)sx + c] : (uint8_t)0;
}

// ---- host only: the argument checks and the tracks, built from the images' own lists (the reference takes positions only from
// points3D)
constexpr int kMaxImages = 16384;

struct TrackArrays {
	std::vector<uint32_t> off, point, image, mult;
	Tracks view(const double* xyz, const double* centres) const { return Tracks{ off.data(), point.data(), image.data(), mult.data(), xyz, centres }; }
};

// "" = done, else what is wrong
inline std::string build_tracks(int N, const long long* obs_offsets, const long long* obs_point_ids, long long P, const long long* point_ids, TrackArrays* t) {
	if (N < 1 || N > kMaxImages) return "num_images must be 1 ... " + std::to_string(kMaxImages);
	if (P < 0 || P > 0x7fffffffLL) return "num_points must be 0 ... 2^31 - 1";
	if (!obs_offsets || obs_offsets[0] != 0) return "obs_offsets must start at 0";
	for (int i = 0; i < N; ++i)
		if (obs_offsets[i + 1] < obs_offsets[i]) return "obs_offsets must not decrease";
	if (obs_offsets[N] > 0x7fffffffLL) return "more than 2^31 - 1 observations";
	std::vector<std::pair<long long, uint32_t>> ids((size_t)P);
	for (long long k = 0; k < P; ++k) ids[(size_t)k] = { point_ids[k], (uint32_t)k };
	std::sort(ids.begin(), ids.end());
	for (size_t k = 1; k < ids.size(); ++k)
		if (ids[k].first == ids[k - 1].first) return "point id " + std::to_string(ids[k].first) + " occurs twice";
	// (point, image) of every observation that names a point, image-major; a stable counting sort by point keeps the image order
	std::vector<uint32_t> of_obs, img_obs;
	of_obs.reserve((size_t)obs_offsets[N]);
	img_obs.reserve((size_t)obs_offsets[N]);
	std::vector<uint32_t> count((size_t)P + 1, 0);
	for (int i = 0; i < N; ++i)
		for (long long o = obs_offsets[i]; o < obs_offsets[i + 1]; ++o) {
			const long long id = obs_point_ids[o];
			if (id == -1) continue;
			const auto it = std::lower_bound(ids.begin(), ids.end(), std::make_pair(id, (uint32_t)0));
			if (it == ids.end() || it->first != id) return "image " + std::to_string(i) + ", observation " + std::to_string(o - obs_offsets[i]) + " names point " + std::to_string(id) + ", which is not among the points";
			of_obs.push_back(it->second);
			img_obs.push_back((uint32_t)i);
			++count[it->second + 1];
		}
	for (size_t k = 0; k < (size_t)P; ++k) count[k + 1] += count[k];
	std::vector<uint32_t> sorted_img(of_obs.size()), fill(count.begin(), count.end() - 1);
	for (size_t o = 0; o < of_obs.size(); ++o) sorted_img[fill[of_obs[o]]++] = img_obs[o];
	t->off.assign((size_t)P + 1, 0);
	t->point.clear(); t->image.clear(); t->mult.clear();
	for (size_t k = 0; k < (size_t)P; ++k) {
		t->off[k] = (uint32_t)t->image.size();
		for (uint32_t o = count[k]; o < count[k + 1]; ++o) {
			if (o > count[k] && sorted_img[o] == t->image.back()) { ++t->mult.back(); continue; }
			t->point.push_back((uint32_t)k);
			t->image.push_back(sorted_img[o]);
			t->mult.push_back(1);
		}
	}
	t->off[(size_t)P] = (uint32_t)t->image.size();
	return "";
}

// the whole matrix, one item after the other: what `--convert-on host` and tests/convert_host run
inline std::string view_scores_serial(int N, const long long* obs_offsets, const long long* obs_point_ids, const double* centres, long long P, const long long* point_ids,
                                      const double* xyz, uint32_t* score_out) {
	TrackArrays arrays;
	const std::string what = build_tracks(N, obs_offsets, obs_point_ids, P, point_ids, &arrays);
	if (!what.empty()) return what;
	const Tracks t = arrays.view(xyz, centres);
	std::vector<uint32_t> cnt((size_t)N * N, 0), low((size_t)N * N, 0);
	const auto add = [](uint32_t* p, uint32_t v) { *p += v; };
	for (uint32_t e = 0; e < (uint32_t)arrays.image.size(); ++e)
		for (uint32_t f = e + 1; f < t.off[t.point[e] + 1]; ++f) pair_item(t, e, f, N, cnt.data(), low.data(), add);
	for (int i = 0; i < N; ++i)
		for (int j = 0; j < N; ++j) score_out[(size_t)i * N + j] = score_at(cnt.data(), low.data(), N, i, j);
	return "";
}

// "" = the sizes are usable
inline std::string check_convert(const void* bgr, int w, int h, long long pitch, int pad_w, int pad_h, int out_w, int out_h, const void* out) {
	if (!bgr || !out) return "the picture and the output are required";
	if (w < 1 || h < 1 || w > 65535 || h > 65535) return "bad image geometry (sizes of 1 ... 65535)";
	if (pitch < 3ll * w) return "the pitch is below 3 * width bytes";
	if (pad_w < w || pad_h < h || pad_w > 65535 || pad_h > 65535) return "the padded size must be at least the picture's and at most 65535";
	if (out_w < 1 || out_h < 1 || out_w > 65535 || out_h > 65535) return "bad output size (1 ... 65535)";
	return "";
}
inline void convert_image_serial(const uint8_t* bgr, int w, int h, size_t pitch, int pad_w, int pad_h, int out_w, int out_h, uint8_t* out) {
	for (int y = 0; y < out_h; ++y)
		for (int k = 0; k < 3 * out_w; ++k) out[(size_t)y * 3 * out_w + k] = converted_byte(bgr, w, h, pitch, pad_w, pad_h, out_w, out_h, k, y);
}

}   // namespace dvppairs
#endif
